"""ctypes loader of tests/bowdb_ref.c, the plain-C restatement of docs/SPEC.md S107-S112 (the image database: add, weights
and ilog2_q8, norms, the exact L1 score and the ordered selection).  Built on first use by cref.py; shared by
test_bowdb_cpu.py, test_bowdb_gpu.py, bowdb_cases.py and tools/prof_bowdb.py."""
import ctypes as C

import numpy as np

import cref
from cref import ptr as _p

_lib = None


def lib():
    global _lib
    if _lib is None:
        v, i = C.c_void_p, C.c_int
        _lib = cref.load("bowdb_ref", {
            "br_create": [i, i, i],
            "br_destroy": [v],
            "br_clear": [v],
            "br_add": [v, v],
            "br_set_weights": [v, v],
            "br_ilog2_q8": [C.c_uint32, C.c_uint32],
            "br_idf": [v],
            "br_query": [v, v, i, i, i, v, v, v],
            "br_get": [v, v, v, v, v, v, v, v, v],
            "br_load": [v, C.c_int32, C.c_int32, v, v, v, v, v, v],
        }, {"br_create": v, "br_destroy": None, "br_clear": None, "br_add": C.c_int32, "br_ilog2_q8": C.c_uint32, "br_idf": None,
            "br_query": C.c_int32, "br_get": None})
    return _lib


def ilog2_q8(N, d):
    return int(lib().br_ilog2_q8(N, d))


def _hist(h, K):
    h = np.ascontiguousarray(h, np.uint32).reshape(-1)
    assert h.size == K
    return h


class RefDb:
    """The restatement's database; the methods mirror points_matching_amd.api.BowDb's blocking forms."""

    def __init__(self, K, max_images, max_entries):
        self.K, self.max_images, self.max_entries = K, max_images, max_entries
        self._h = lib().br_create(K, max_images, max_entries)

    def close(self):
        if self._h:
            lib().br_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def clear(self):
        lib().br_clear(self._h)

    def add(self, hist):
        return int(lib().br_add(self._h, _p(_hist(hist, self.K))))

    def set_weights(self, weights):
        """0, or -1 when a weight is above 8191 (nothing changes)."""
        return int(lib().br_set_weights(self._h, _p(_hist(weights, self.K))))

    def idf(self):
        lib().br_idf(self._h)

    def counts(self):
        n, e = C.c_int32(), C.c_int32()
        lib().br_get(self._h, C.byref(n), C.byref(e), None, None, None, None, None, None)
        return n.value, e.value

    def get(self):
        n, e = self.counts()
        d = dict(n_images=n, n_entries=e, offsets=np.zeros(n + 1, np.uint32), words=np.zeros(e, np.uint32), tfs=np.zeros(e, np.uint16),
                 norms=np.zeros(n, np.uint32), df=np.zeros(self.K, np.uint32), weights=np.zeros(self.K, np.uint32))
        lib().br_get(self._h, None, None, _p(d["offsets"]), _p(d["words"]), _p(d["tfs"]), _p(d["norms"]), _p(d["df"]), _p(d["weights"]))
        return d

    def load(self, d):
        """Takes over a get() dictionary (of this or of the device's database)."""
        a = {k: np.ascontiguousarray(d[k], t) for k, t in (("offsets", np.uint32), ("words", np.uint32), ("tfs", np.uint16),
                                                           ("norms", np.uint32), ("df", np.uint32), ("weights", np.uint32))}
        assert a["offsets"].size == d["n_images"] + 1 and a["words"].size == a["tfs"].size == d["n_entries"] and a["df"].size == self.K
        rc = lib().br_load(self._h, d["n_images"], d["n_entries"], _p(a["offsets"]), _p(a["words"]), _p(a["tfs"]), _p(a["norms"]),
                           _p(a["df"]), _p(a["weights"]))
        assert rc == 0

    def query(self, hist, top, excl_lo=0, excl_hi=0):
        """(ids int32 (top,), scores float64 (top,), count, the score of every image): tails -1 / quiet NaN."""
        n = self.counts()[0]
        ids, scores, every = np.zeros(top, np.int32), np.zeros(top, np.float64), np.zeros(n, np.float64)
        count = int(lib().br_query(self._h, _p(_hist(hist, self.K)), top, excl_lo, excl_hi, _p(ids), _p(scores), _p(every)))
        return ids, scores, count, every


def same_dump(a, b):
    """Two get() dictionaries are equal in every field."""
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a) and a.keys() == b.keys()
