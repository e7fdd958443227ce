"""
CPU: the five update entry points of the IVF-Flat index exist (hipivf_from_centroids, hipivf_add(_dev), hipivf_remove_ranges,
hipivf_update_info), and the numpy MODEL of an updatable IVF index that tests/test_ivf_update_gpu.py compares the library
with.  The model knows nothing of the library's run tables or kernels: it keeps the current rows in id order and the ids of
every list, and derives offsets, original ids, stored rows and HIPIVF01 file bytes by the layout rule include/hiprag.h states
for hipivf_build (lists in list order, ascending id within a list, every list padded to whole 32-row blocks with zero rows
of id -1).
"""
import ctypes
import os

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

BLOCK = 32
UPDATE_SYMBOLS = ("hipivf_from_centroids", "hipivf_add_dev", "hipivf_add", "hipivf_remove_ranges", "hipivf_update_info")


def pad32(v):
    return (v + BLOCK - 1) // BLOCK * BLOCK


class IvfModel:
    def __init__(self, cents, metric):
        self.cents = np.ascontiguousarray(cents, dtype=np.float32)
        self.metric = int(metric)
        self.nlist, self.d = self.cents.shape
        self.x = np.zeros((0, self.d), dtype=np.float32)                    # the current rows, row i has id i
        self.lists = [np.zeros(0, dtype=np.int64) for _ in range(self.nlist)]   # ids of every list, ascending

    @classmethod
    def from_lists(cls, cents, metric, x, offs, orig):
        """the state of an index as its lists() reports it"""
        m = cls(cents, metric)
        m.x = np.ascontiguousarray(x, dtype=np.float32)
        for l in range(m.nlist):
            ids = orig[offs[l]:offs[l + 1]]
            m.lists[l] = ids[ids >= 0].astype(np.int64)
        return m

    @property
    def n(self):
        return len(self.x)

    def lengths(self):
        return np.asarray([len(ids) for ids in self.lists], dtype=np.int64)

    def layout(self):
        """(offsets [nlist + 1], original id of every stored row)"""
        offs = np.zeros(self.nlist + 1, dtype=np.int64)
        offs[1:] = np.cumsum([pad32(len(ids)) for ids in self.lists])
        orig = np.full(offs[-1], -1, dtype=np.int64)
        for l, ids in enumerate(self.lists):
            orig[offs[l]:offs[l] + len(ids)] = ids
        return offs, orig

    def stored_rows(self):
        _, orig = self.layout()
        rows = np.zeros((len(orig), self.d), dtype=np.float32)
        rows[orig >= 0] = self.x[orig[orig >= 0]]
        return rows

    def _place(self):
        """stored row of every id"""
        _, orig = self.layout()
        place = np.full(self.n, -1, dtype=np.int64)
        place[orig[orig >= 0]] = np.nonzero(orig >= 0)[0]
        return place

    def _chunks(self, old_orig):
        """Staging chunks of an update of a small index: one if any stored row of the NEW layout holds something else than
        it held before (old_orig, in the new numbering), none if every one stands as it stood -- then nothing is staged:
        an update that adds or removes nothing, a removal that leaves no row, or one that only drops whole blocks at the
        very end of the storage."""
        new_orig = self.layout()[1]
        was = np.full(len(new_orig), -2, dtype=np.int64)                          # -2: no such stored row before
        keep = min(len(new_orig), len(old_orig))
        was[:keep] = old_orig[:keep]
        return int(np.any(was != new_orig))

    def add(self, x_new, assign):
        """x_new [m, d] joins with the ids n .. n + m - 1, row j in list assign[j]; returns the expected update_info"""
        x_new = np.ascontiguousarray(x_new, dtype=np.float32).reshape(-1, self.d)
        assign = np.asarray(assign, dtype=np.int64)
        before, n0 = self._place(), self.n
        old_orig = self.layout()[1]
        self.x = np.concatenate([self.x, x_new])
        for l in range(self.nlist):
            self.lists[l] = np.concatenate([self.lists[l], n0 + np.nonzero(assign == l)[0]])
        moved = int(np.sum(self._place()[:n0] != before))
        return {"added": len(x_new), "removed": 0, "moved": moved, "chunks": self._chunks(old_orig)}

    def remove(self, ranges):
        """half-open id ranges go, the survivors are renumbered densely; returns the expected update_info"""
        gone = np.zeros(self.n, dtype=bool)
        for lo, hi in np.asarray(ranges, dtype=np.int64).reshape(-1, 2):
            gone[lo:hi] = True
        before = self._place()
        new_id = np.where(gone, -1, np.cumsum(~gone) - 1)
        old_orig = self.layout()[1]
        old_orig = np.where(old_orig >= 0, new_id[np.maximum(old_orig, 0)], -1)      # in the new numbering, -1 = gone or padding
        self.x = self.x[~gone]
        self.lists = [new_id[ids[~gone[ids]]] for ids in self.lists]
        moved = int(np.sum(self._place() != before[~gone]))
        return {"added": 0, "removed": int(gone.sum()), "moved": moved, "chunks": self._chunks(old_orig)}

    def file_bytes(self):
        """the whole HIPIVF01 file (the format tests/test_ivf_build_gpu.py's read_ivf_file reads)"""
        offs, orig = self.layout()
        return b"".join([b"HIPIVF01", np.asarray([1, self.d, self.metric, self.nlist], dtype=np.int32).tobytes(),
                         np.asarray([self.n, len(orig)], dtype=np.int64).tobytes(), self.cents.tobytes(), offs.tobytes(),
                         orig.tobytes(), self.stored_rows().tobytes()])

    def check(self):
        offs, orig = self.layout()
        assert offs[0] == 0 and np.all(offs % BLOCK == 0) and np.all(np.diff(offs) >= 0) and offs[-1] == len(orig)
        assert np.array_equal(np.sort(orig[orig >= 0]), np.arange(self.n))          # every id exactly once
        for l in range(self.nlist):
            ids = orig[offs[l]:offs[l + 1]]
            real = ids[ids >= 0]
            assert np.all(np.diff(real) > 0) and np.all(ids[len(real):] == -1)        # ascending, padding at the tail
            assert offs[l + 1] - offs[l] == pad32(len(real)) and np.array_equal(real, self.lists[l])


def separated_centroids(nlist, d, seed):
    """orthonormal rows: a row of clustered_rows is nearest to its own centroid under both metrics, with a wide margin"""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, nlist)))
    return np.ascontiguousarray(q.T, dtype=np.float32)


def clustered_rows(cents, labels, rng, sigma=0.01):
    labels = np.asarray(labels, dtype=np.int64)
    noise = rng.standard_normal((len(labels), cents.shape[1])).astype(np.float32)
    return (cents[labels] + np.float32(sigma) * noise).astype(np.float32)


def ranges_of(ids):
    """ascending half-open ranges that cover exactly `ids`"""
    ids = np.unique(np.asarray(ids, dtype=np.int64))
    if len(ids) == 0:
        return np.zeros((0, 2), dtype=np.int64)
    cut = np.nonzero(np.diff(ids) > 1)[0]
    return np.stack([ids[np.concatenate([[0], cut + 1])], ids[np.concatenate([cut, [len(ids) - 1]])] + 1], axis=1)


# ---- the library's surface -------------------------------------------------------------------------------------------
def test_library_exports_and_binding_declares_the_update_symbols():
    from hiprag import _native as nat
    assert os.path.exists(nat.LIB_PATH), "build the library first: __graft_entry__.build()"
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in UPDATE_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in nat.SIGNATURES, f"{name} is not declared in hiprag/_native.py"
    from hiprag import HipIVFIndex
    for method in ("from_centroids", "add", "remove_ranges", "update_info"):
        assert callable(getattr(HipIVFIndex, method))


# ---- the model's own invariants --------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [ho.METRIC_IP, ho.METRIC_L2])
@pytest.mark.parametrize("d", [64, 36])
def test_model_invariants_through_adds_and_removals(metric, d):
    nlist = 5
    rng = np.random.default_rng(7)
    cents = separated_centroids(nlist, d, seed=3)
    m = IvfModel(cents, metric)
    m.check()
    labels = rng.permutation(np.repeat(np.arange(nlist), [31, 32, 255, 0, 40]))
    x = clustered_rows(cents, labels, rng)
    # the data is what it claims to be: the exact assignment is the label, with a margin far above the noise
    s, i = ho.flat_search(cents, x, 2, metric)
    assert np.array_equal(i[:, 0], labels) and np.all(np.abs(s[:, 0] - s[:, 1]) > 0.5)
    info = m.add(x, labels)
    m.check()
    assert info == {"added": len(x), "removed": 0, "moved": 0, "chunks": 1} and np.array_equal(m.lengths(), [31, 32, 255, 0, 40])
    assert m.add(clustered_rows(cents, [0], rng), [0])["moved"] == 0          # 31 -> 32 fills the padding
    m.check()
    assert m.add(clustered_rows(cents, [1], rng), [1])["moved"] == 255 + 40   # 32 -> 33 takes a block: lists 2.. move
    m.check()
    assert m.add(np.zeros((0, d), np.float32), [])["chunks"] == 0
    n = m.n
    info = m.remove([[3, 9], [100, 101], [n - 5, n]])
    m.check()
    assert info["removed"] == 12 and m.n == n - 12
    info = m.remove([[0, m.n]])
    m.check()
    assert m.n == 0 and info["moved"] == 0 and info["chunks"] == 0 and np.array_equal(m.layout()[0], np.zeros(nlist + 1))
    assert m.file_bytes() == IvfModel(cents, metric).file_bytes()             # the from_centroids state
    again = IvfModel.from_lists(cents, metric, m.x, *m.layout())
    assert again.add(x, labels)["added"] == len(x)
    again.check()


def test_ranges_of_covers_exactly_the_ids():
    r = ranges_of([9, 3, 4, 5, 11, 12, 20])
    assert r.tolist() == [[3, 6], [9, 10], [11, 13], [20, 21]]
    assert ranges_of([]).shape == (0, 2)


def test_add_everything_to_empty_is_the_build_rule():
    """the layout the build test checks (tests/test_ivf_build_gpu.py test_layout_and_file_contents): same rule, same arrays"""
    rng = np.random.default_rng(11)
    nlist, d, n = 24, 16, 5003
    assign = rng.integers(0, nlist, size=n)
    assign[assign == 7] = 8                                                   # an empty list
    x = rng.standard_normal((n, d)).astype(np.float32)
    m = IvfModel(np.zeros((nlist, d), np.float32), ho.METRIC_L2)
    m.add(x, assign)
    offs, orig = m.layout()
    assert offs[0] == 0 and np.all(offs % 32 == 0) and np.all(np.diff(offs) >= 0) and offs[-1] == len(orig)
    for l in range(nlist):
        ids = orig[offs[l]:offs[l + 1]]
        real = ids[ids >= 0]
        assert np.array_equal(real, np.nonzero(assign == l)[0])               # the list's rows, ascending original id
        assert np.all(ids[len(real):] == -1)
        assert offs[l + 1] - offs[l] == (len(real) + 31) // 32 * 32
    assert offs[8] == offs[7]
    rows = m.stored_rows()
    assert np.array_equal(rows[orig >= 0], x[orig[orig >= 0]]) and not np.any(rows[orig < 0])
    raw = m.file_bytes()
    assert len(raw) == 40 + nlist * d * 4 + (nlist + 1) * 8 + len(orig) * 8 + len(orig) * d * 4
