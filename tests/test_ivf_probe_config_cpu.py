"""HIP_IVF_PROBE and HIP_IVF_HYBRID (rag/config.py): opt-in, read at use, anything else than the named values raises."""
import pytest


def test_probe_setting_defaults_to_any_and_refuses_other_values(monkeypatch):
    from rag.config import config
    monkeypatch.delenv("HIP_IVF_PROBE", raising=False)
    assert config.HIP_IVF_PROBE == "any"
    for raw, want in (("scope", "scope"), (" Scope ", "scope"), ("ANY", "any")):
        monkeypatch.setenv("HIP_IVF_PROBE", raw)
        assert config.HIP_IVF_PROBE == want
    for raw in ("project", "", "1"):
        monkeypatch.setenv("HIP_IVF_PROBE", raw)
        with pytest.raises(ValueError, match="HIP_IVF_PROBE"):
            config.HIP_IVF_PROBE


def test_hybrid_setting_defaults_to_false(monkeypatch):
    from rag.config import config
    monkeypatch.delenv("HIP_IVF_HYBRID", raising=False)
    assert config.HIP_IVF_HYBRID is False
    for raw, want in (("true", True), (" TRUE ", True), ("false", False), ("yes", False), ("", False)):
        monkeypatch.setenv("HIP_IVF_HYBRID", raw)
        assert config.HIP_IVF_HYBRID is want


def test_probe_argument_of_the_index_maps_to_the_header_constants():
    import re
    import os
    from hiprag import HipIVFIndex, _native as nat
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hiprag.h")).read()
    assert int(re.search(r"#define HIPIVF_PROBE_ANY\s+(\d+)", header).group(1)) == nat.PROBE_ANY == HipIVFIndex._probe_mode("any")
    assert int(re.search(r"#define HIPIVF_PROBE_SCOPE\s+(\d+)", header).group(1)) == nat.PROBE_SCOPE == HipIVFIndex._probe_mode("scope")
    assert HipIVFIndex._probe_mode(5) == 5
    with pytest.raises(ValueError, match="probe"):
        HipIVFIndex._probe_mode("project")
