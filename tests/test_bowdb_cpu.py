"""CPU: the image database (docs/SPEC.md S107-S112) through the plain-C restatement tests/bowdb_ref.c — against a Python
model written independently here (dictionaries and big integers: S is an unbounded int, the score float(S) / float(Nq * Nd),
the order a sort by (-score, id)), ilog2_q8 against the exact floor found with big-integer comparisons, retrieval on the
planted scene — and the C ABI surface of libpm_hip.so: the prototypes, the exports and the refusals that need no device.

ilog2_q8 against the exact floor, as measured here: 5158 of the 5158 exhaustive cases (every d <= N for N in 1, 2, 3, 7, 48,
1000, 4097) and 3044 of 3044 sampled d at N = 2^22 are equal; none is one below.  Retrieval on the planted scene: 24 of 24
places right under both weightings, the second score at least 1.80 times the third; unit weights give 709 exact ties."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bowdb_cases as cases
import bowdb_ref as R
from points_matching_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"pm_bowdb_create": 5, "pm_bowdb_destroy": 1, "pm_bowdb_clear_dev": 2, "pm_bowdb_add_dev": 4, "pm_bowdb_add": 4,
         "pm_bowdb_set_weights": 3, "pm_bowdb_get_weights": 3, "pm_bowdb_idf_dev": 2, "pm_bowdb_query_dev": 10,
         "pm_bowdb_query": 10, "pm_bowdb_get": 10}


# ---- the model -------------------------------------------------------------------------------------------------------------------
def model_ilog2_q8(N, d):
    """S109's algorithm on Python integers."""
    e = 0
    while (d << (e + 1)) <= N:
        e += 1
    m = (N << 30) // (d << e)
    f = 0
    for _ in range(8):
        m = (m * m) >> 30
        f <<= 1
        if m >= 1 << 31:
            f |= 1
            m >>= 1
    return (e << 8) | f


def true_floor(N, d):
    """floor(256 * log2(N / d)) exactly: the largest v with d^256 * 2^v <= N^256."""
    v = (N ** 256 // d ** 256).bit_length() - 1
    assert d ** 256 << v <= N ** 256 < d ** 256 << (v + 1)
    return v


class Model:
    """An image is a dict word -> tf; nothing is cached: every norm is summed anew from the current weights."""

    def __init__(self, K, max_images, max_entries):
        self.K, self.max_images, self.max_entries = K, max_images, max_entries
        self.images, self.weights = [], [1] * K

    def _entries(self):
        return sum(len(i) for i in self.images)

    def add_many(self, hists):
        ids = []
        for h in hists:
            img = {int(w): int(h[w]) for w in np.flatnonzero(h)}
            T = sum(img.values())
            if not 1 <= T <= 65535:
                ids.append(-1)
            elif len(self.images) >= self.max_images or self._entries() + len(img) > self.max_entries:
                ids.append(-2)
            else:
                ids.append(len(self.images))
                self.images.append(img)
        return np.array(ids, np.int32)

    def set_weights(self, w):
        if max(int(v) for v in w) > 8191:
            return -1
        self.weights = [int(v) for v in w]
        return 0

    def df(self):
        df = [0] * self.K
        for img in self.images:
            for w in img:
                df[w] += 1
        return df

    def idf(self):
        N = len(self.images)
        if N:
            self.weights = [model_ilog2_q8(N, max(d, 1)) for d in self.df()]

    def clear(self):
        self.images = []

    def norm(self, img):
        return sum(tf * self.weights[w] for w, tf in img.items())

    def get(self):
        off = np.cumsum([0] + [len(i) for i in self.images]).astype(np.uint32)
        words = np.array([w for i in self.images for w in sorted(i)], np.uint32)
        tfs = np.array([i[w] for i in self.images for w in sorted(i)], np.uint16)
        return dict(n_images=len(self.images), n_entries=int(off[-1]), offsets=off, words=words, tfs=tfs,
                    norms=np.array([self.norm(i) for i in self.images], np.uint32), df=np.array(self.df(), np.uint32),
                    weights=np.array(self.weights, np.uint32))

    def query(self, hist, top, lo, hi):
        hist = [int(v) for v in hist]
        T = sum(hist)
        q = {w: hist[w] * self.weights[w] for w in range(self.K) if hist[w]}
        Nq = sum(q.values()) if 1 <= T <= 65535 else 0
        every, cands = [], []
        for i, img in enumerate(self.images):
            Nd = self.norm(img)
            S = sum(min(q.get(w, 0) * Nd, tf * self.weights[w] * Nq) for w, tf in img.items()) if Nq and Nd else 0
            s = float(S) / float(Nq * Nd) if Nq and Nd else 0.0
            every.append(s)
            if S > 0 and not lo <= i < hi:
                cands.append((-s, i))
        cands.sort()
        ids, scores = np.full(top, -1, np.int32), np.full(top, cases.QNAN, np.float64)
        count = min(top, len(cands))
        for j in range(count):
            ids[j], scores[j] = cands[j][1], -cands[j][0]
        return ids, scores, count, np.array(every, np.float64)


class Ref:
    """bowdb_ref.RefDb behind the adapter interface of bowdb_cases."""

    def __init__(self, K, max_images, max_entries):
        self.K, self.db = K, R.RefDb(K, max_images, max_entries)

    def add_many(self, hists):
        return np.array([self.db.add(h) for h in hists], np.int32)

    def __getattr__(self, name):
        return getattr(self.db, name)


def both(K, max_images, max_entries, ops):
    ref, model = cases.run(Ref(K, max_images, max_entries), ops), cases.run(Model(K, max_images, max_entries), ops)
    assert cases.same(ref, model) == ""
    return ref


# ---- S109: ilog2_q8 --------------------------------------------------------------------------------------------------------------
def test_ilog2_q8_is_the_floor_or_one_below():
    equal = total = 0
    for N in (1, 2, 3, 7, 48, 1000, 4097):
        for d in range(1, N + 1):
            v, t = R.ilog2_q8(N, d), true_floor(N, d)
            assert v == model_ilog2_q8(N, d) and 0 <= t - v <= 1, (N, d, v, t)
            equal += v == t
            total += 1
    sampled_equal = 0
    N = 1 << 22
    ds = np.unique(np.concatenate([np.random.default_rng(22).integers(1, N + 1, size=3000), 2 ** np.arange(23), N - np.arange(23)]))
    for d in (int(x) for x in ds):
        v, t = R.ilog2_q8(N, d), true_floor(N, d)
        assert v == model_ilog2_q8(N, d) and 0 <= t - v <= 1, (N, d, v, t)
        sampled_equal += v == t
    print("ilog2_q8 equal to the exact floor: %d of %d exhaustive, %d of %d sampled at N = 2^22" % (equal, total, sampled_equal, len(ds)))
    assert total == 1 + 2 + 3 + 7 + 48 + 1000 + 4097


def test_ilog2_q8_is_exact_on_powers_of_two():
    for N in (1, 2, 3, 7, 48, 1000, 4097, 1 << 22, (1 << 22) - 1, 3 << 20):
        k = 0
        while N % (1 << k) == 0 and (N >> k) >= 1:
            assert R.ilog2_q8(N, N >> k) == k << 8 == true_floor(N, N >> k), (N, k)
            k += 1
    assert R.ilog2_q8(1 << 22, 1) == 22 * 256 < 8192


# ---- S108-S111 against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", cases.ADD_KS)
def test_add(K):
    mi, me, ops, names = cases.add_case(K)
    res = both(K, mi, me, ops)
    ids = dict(zip(names, (int(r[0]) for r in res[0::2])))
    assert ids["first_word"] == 0 and ids["T_65536"] == -1 and ids["all_zero"] == -1 and ids["T_65535"] >= 0, ids
    dumps = dict(zip(names, res[1::2]))
    assert R.same_dump(dumps["T_65535"], dumps["T_65536"]) and R.same_dump(dumps["T_65535"], dumps["all_zero"])
    last = dumps["one_more"]
    assert last["n_images"] == ids["one_more"] + 1 == len(names) - 2
    for i in range(last["n_images"]):
        w = last["words"][last["offsets"][i]:last["offsets"][i + 1]]
        assert (np.diff(w.astype(np.int64)) > 0).all()


@pytest.mark.parametrize("case", cases.limit_cases(), ids=lambda c: c[0])
def test_limits(case):
    name, K, mi, me, ops = case
    res = both(K, mi, me, ops)
    if name == "entries_full":
        assert [int(r[0]) for r in res[0:8:2]] == [0, 1, -2, -1] and res[3]["n_entries"] == 10
        assert R.same_dump(res[3], res[5]) and R.same_dump(res[3], res[7])
    else:
        assert res[0][0] == 0 and res[1][0] == 1 and res[3][0] == -2 and R.same_dump(res[2], res[4])


@pytest.mark.parametrize("N", [1, 2, 3, 48])
def test_weights(N):
    K, mi, me, ops = cases.weight_case(N)
    res = both(K, mi, me, ops)
    first, after_idf, given, after_bad, cleared, idf_on_empty = res[1], res[4], res[7], res[10], res[12], res[14]
    assert first["df"][0] == 0 and first["df"][1] == 1 and first["df"][2] == N and (first["weights"] == 1).all()
    assert after_idf["weights"][2] == 0 and after_idf["weights"][0] == after_idf["weights"][1] == R.ilog2_q8(N, 1)
    assert res[6] == 0 and res[9] == -1 and R.same_dump(given, after_bad)
    assert (given["weights"] == ops[6][1]).all() and 0 in given["weights"] and 8191 in given["weights"]
    if N > 1:
        assert not (given["norms"] == after_idf["norms"]).all()
    assert cleared["n_images"] == 0 and cleared["n_entries"] == 0 and (cleared["df"] == 0).all() and (cleared["weights"] == given["weights"]).all()
    assert R.same_dump(cleared, idf_on_empty)


@pytest.mark.parametrize("idf", [False, True], ids=["unit", "idf"])
def test_scene_scores(idf):
    K, mi, me, ops = cases.scene_case(idf)
    res = both(K, mi, me, ops)
    ids, scores, count, every = res[-24]                                 # query 0: the image equal to it is image 48
    assert ids[0] == 48 and scores[0] == cases.u64([1.0])[0] and every[48] == cases.u64([1.0])[0] and count == 5


def test_shapes_and_range():
    for make in (cases.shapes_case, cases.range_case):
        K, mi, me, ops = make()
        res = both(K, mi, me, ops)
        if make is cases.shapes_case:
            ids, scores, count, every = res[3]
            every = every.view(np.float64)
            assert ids[0] == 7 and every[7] == 1.0 and every[5] == 0.0 and every[6] == 0.0 and (every[:5] > 0).all()
            assert set(ids[:count].tolist()) == {0, 1, 2, 3, 4, 7} and res[4][0][0] == 4
        else:
            every = res[3][3].view(np.float64)
            assert every[0] == 1.0 and every[3] == 1.0 and res[3][0][0] == 0 and res[3][0][1] == 3    # a tie at 1.0: the lower id first
            Nq, Nd = 25535 * 8191 + 40000 * 8189, 40001 * 8191 + 25534 * 8189          # query 1 against image 1
            S = min(25535 * 8191 * Nd, 40001 * 8191 * Nq) + min(40000 * 8189 * Nd, 25534 * 8189 * Nq)
            assert S > 1 << 53 and Nq * Nd > 1 << 53 and S & 1 and Nq * Nd & 1       # past 2^53 with the lowest bit set
            assert res[4][3].view(np.float64)[1] == float(S) / float(Nq * Nd)
            Nq, Nd = 30001 * 8191 + 20003 * 8189 + 15531 * 8187, 21845 * 8191 + 21847 * 8189 + 21843 * 8187      # query 2, image 2
            S = sum(min(q * w * Nd, d * w * Nq) for q, d, w in ((30001, 21845, 8191), (20003, 21847, 8189), (15531, 21843, 8187)))
            assert S > 1 << 53 and S & 0xFFFF and Nq * Nd & 1 and res[5][3].view(np.float64)[2] == float(S) / float(Nq * Nd)


@pytest.mark.parametrize("N", cases.SELECT_NS)
def test_selection(N):
    K, mi, me, ops = cases.selection_case(N)
    res = both(K, mi, me, ops)
    full = res[1]                                                        # top = 1, no window
    assert full[2] == min(1, N)
    for r, op in zip(res[1:], ops[1:]):
        if op[0] == "query":
            ids, scores, count, every = r
            s = scores.view(np.float64)
            assert (ids[count:] == -1).all() and (scores[count:] == cases.u64([cases.QNAN])[0]).all()
            assert (np.diff(s[:count]) <= 0).all()
            for a, b in zip(range(count - 1), range(1, count)):
                assert s[a] > s[b] or ids[a] < ids[b]
        elif op[0] == "query_without_best":
            best, ids, _, count, _ = r
            assert best not in ids[:count].tolist()
    assert res[-3][2] == 0 and res[-2][2] == 0 and not res[-3][3].any() and not res[-2][3].any()    # the refused queries
    if N >= 1025:
        assert len(set(res[1 + 7 * 3][1][:256].tolist())) < 64           # top = 256: exact ties decide most places


def test_a_dump_loads_into_an_equal_database():
    K, mi, me, ops = cases.scene_case(True)
    a, b = Ref(K, mi, me), R.RefDb(K, mi, me)
    cases.run(a, ops[:3])
    b.load(a.get())
    assert R.same_dump(a.get(), b.get())
    q = cases.place_scene()[1][5]
    x, y = a.query(q, 9, 3, 7), b.query(q, 9, 3, 7)
    assert (x[0] == y[0]).all() and (cases.u64(x[1]) == cases.u64(y[1])).all() and x[2] == y[2] == 9 and (x[3] == y[3]).all()


# ---- retrieval ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idf", [False, True], ids=["unit", "idf"])
def test_retrieval_puts_both_images_of_the_place_first(idf):
    """48 images of 24 places (bowdb_cases.place_scene, default_rng(7)): a fresh image of each place must rank that place's
    two images first and second.  The margin behind the assertion is printed: the second score over the third."""
    dbh, qs = cases.place_scene()
    db = R.RefDb(512, 48, int((dbh != 0).sum()))
    for h in dbh:
        assert db.add(h) >= 0
    if idf:
        db.idf()
    margins, ties = [], 0
    for p, q in enumerate(qs):
        ids, scores, count, every = db.query(q, 3)
        assert count == 3 and sorted(ids[:2].tolist()) == [2 * p, 2 * p + 1], (p, ids, scores)
        margins.append(scores[1] / scores[2])
        ties += len(every) - len(set(every.tolist()))
    print("second / third score: min %.3f; exact ties among the 24 x 48 scores: %d" % (min(margins), ties))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_prototypes_and_exports():
    hdr = open(os.path.join(ROOT, "include", "pm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = api.lib()
    for name, arity in ARITY.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == arity, name
        assert name in api.EXPORTS and hasattr(L, name), name
    assert "typedef struct pm_bowdb pm_bowdb;" in code
    r = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    syms = {ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip()}
    assert not [n for n in ARITY if n not in syms]


def test_refusals_without_a_device():
    L = api.lib()
    INV = api.PM_E_INVALID
    h = C.c_void_p(7)
    d = C.c_void_p(256)                                       # never dereferenced: every call below is refused first

    def refused(rc, msg):
        return rc == INV and msg in L.pm_last_error()

    def create(K=8, mi=10, me=100, out=True):
        h.value = 7
        return L.pm_bowdb_create(None, K, mi, me, C.byref(h) if out else None)

    assert refused(create(out=False), b"null output")
    for K in (0, -1, 262145):
        assert refused(create(K=K), b"1 <= K <= 262144") and not h.value
    for mi in (0, -1, (1 << 22) + 1):
        assert refused(create(mi=mi), b"max_images <= 2^22") and not h.value
    for me in (0, -1, (1 << 28) + 1):
        assert refused(create(me=me), b"max_entries <= 2^28") and not h.value
    for K, mi, me in ((1, 1, 1), (262144, 1 << 22, 1 << 28)):
        assert refused(create(K, mi, me), b"ctx is null") and not h.value                      # the limits themselves pass
    assert refused(L.pm_bowdb_add_dev(None, None, d, None), b"null argument")
    assert refused(L.pm_bowdb_add(None, None, d, None), b"null argument")
    assert refused(L.pm_bowdb_clear_dev(None, None), b"null argument") and refused(L.pm_bowdb_idf_dev(None, None), b"null argument")
    assert refused(L.pm_bowdb_set_weights(None, None, d), b"null argument") and refused(L.pm_bowdb_get_weights(None, None, d), b"null argument")
    assert refused(L.pm_bowdb_get(None, None, None, None, None, None, None, None, None, None), b"null argument")
    h.value = 7                                               # a database that is never looked at
    for fn in (L.pm_bowdb_query_dev, L.pm_bowdb_query):
        assert refused(fn(None, None, d, 5, 0, 0, None, None, None, None), b"null argument")
        for top in (0, -1, 257):
            assert refused(fn(None, h, d, top, 0, 0, None, None, None, None), b"1 <= top <= 256")
    assert L.pm_bowdb_destroy(None) == api.PM_OK
