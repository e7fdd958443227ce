"""The IVF settings of the drop-in (rag/config.py): opt-in, defaults that leave today's flat files alone, and the automatic
nlist rule max(1, min(n // 39, 4 * ceil(sqrt(n))))."""
import math

import pytest


def test_ivf_settings_default_to_the_flat_index(monkeypatch):
    from rag.config import Config
    for name in ("HIP_INDEX_TYPE", "HIP_IVF_NLIST", "HIP_IVF_NPROBE"):
        monkeypatch.delenv(name, raising=False)
    c = Config()
    assert (c.HIP_INDEX_TYPE, c.HIP_IVF_NLIST, c.HIP_IVF_NPROBE) == ("flat", 0, 16)
    monkeypatch.setenv("HIP_INDEX_TYPE", "IVF")
    monkeypatch.setenv("HIP_IVF_NLIST", "64")
    monkeypatch.setenv("HIP_IVF_NPROBE", "4")
    assert (c.HIP_INDEX_TYPE, c.HIP_IVF_NLIST, c.HIP_IVF_NPROBE) == ("ivf", 64, 4)
    monkeypatch.setenv("HIP_INDEX_TYPE", "hnsw")
    with pytest.raises(ValueError):
        c.HIP_INDEX_TYPE


def test_auto_nlist_rule():
    from rag.config import ivf_auto_nlist
    assert [ivf_auto_nlist(n) for n in (0, 1, 38, 39, 78, 1000, 10_000, 1_000_000, 10_000_000)] == \
        [1, 1, 1, 1, 2, 25, 256, 4000, 12652]
    for n in range(1, 5000, 7):
        assert ivf_auto_nlist(n) == max(1, min(n // 39, 4 * math.ceil(math.sqrt(n))))
