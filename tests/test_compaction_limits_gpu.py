"""GPU: the two one-launch stable compactions past one look-back round and at their row limits.

(a) pm_filter_{ratio,midpoint,cross}_gather_dev on the by-construction records of compaction_ref.py from 256 blocks (one
    poll round) to 4096 blocks (16 rounds), every pattern, against the numpy rules;
(b) the 1 048 576-row limit of those calls;
(c) the compaction fused into the L2 refinement past 256 tiles on every route, against the oracle's 2-NN + the numpy rule;
(d) growth of the fused form's per-context words past 4096 tiles, and the matcher at 131 105 queries;
(e) pm_concat_points_dev at its part limit, with strides above one workgroup and counts that need clamping.
Every output is compared bit for bit, and everything behind the survivors must still hold the sentinel the test wrote.

What would make these fail (block or tile b polls its predecessors j = lane, lane + 256, ... < b, so b = 257 is the first
to poll twice: 258 blocks or tiles):
  * a look-back that stops after its first round: (a) from 66309 rows on and (c) from 258 tiles on, for every pattern or
    train set in which a block behind the 256th has survivors in front of it (all, checker, first_of_block, half; mix,
    all) - its survivors land 256 blocks too early and the count is short; (d) likewise at 4098 tiles;
  * the count written by a block other than the last: last_only (n = 1 comes from the last block alone), and every case
    whose last block or tile has survivors in front of it;
  * a count field too narrow: a full block's 256 is bit 8 of the 10-bit field and a full tile's 32 bit 5 of the 8-bit
    one, so ONE bit less changes no result (both fields have bits to spare); two bits less zero the count of every full
    block: all and checker in (a);
  * the fused count words not re-based on the grown allocation: step 2 of (d) would publish its counts into the arrival
    words of the new block;
  * none / last_only hold the other end: nothing may be written, or exactly one record at offset 0, however many rounds
    are polled.  (b) and (e) guard argument limits, not a look-back."""
import functools

import numpy as np
import pytest

import points_matching_amd as pm
from points_matching_amd import api
import compaction_ref as cr
from util import assert_matches_equal

pytestmark = pytest.mark.gpu

FWD, REV = api.PM_CROSS_RATIO_FWD, api.PM_CROSS_RATIO_REV
THREADS = 16
SENT_I, SENT_F = -7, -7.0
ROW_LIMIT = 1 << 20


def _dev():
    import torch
    return torch.device("cuda", 0)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _up_records(rec):
    return _up(np.ascontiguousarray(rec).view(np.int32).reshape(rec.shape[0], -1))


class _Outputs:
    """Device outputs of one compaction call, refilled with sentinels before every call."""

    def __init__(self, cap):
        import torch
        self.torch = torch
        self.good = torch.empty((cap, 4), dtype=torch.int32, device=_dev())
        self.xy1 = torch.empty((cap, 2), dtype=torch.float32, device=_dev())
        self.xy2 = torch.empty((cap, 2), dtype=torch.float32, device=_dev())
        self.n = torch.empty(1, dtype=torch.int32, device=_dev())
        self.reset()

    def reset(self):
        self.good.fill_(SENT_I)
        self.xy1.fill_(SENT_F)
        self.xy2.fill_(SENT_F)
        self.n.fill_(-1)
        self.torch.cuda.synchronize()

    def ptrs(self, with_kp):
        return (self.good.data_ptr(), self.xy1.data_ptr() if with_kp else 0, self.xy2.data_ptr() if with_kp else 0,
                self.n.data_ptr())

    def check(self, want, kp1, kp2, with_kp, what):
        """Count, survivors bit for bit, both gathers, and the sentinel behind them."""
        n = int(self.n.item())
        assert n == want.size, (what, n, want.size)
        raw = self.good.cpu().numpy()
        assert_matches_equal(raw[:n].view(cr.MATCH_DTYPE).reshape(-1), want, what)
        assert (raw[n:] == SENT_I).all(), what + ": record written behind the survivors"
        xy1, xy2 = self.xy1.cpu().numpy(), self.xy2.cpu().numpy()
        m = n if with_kp else 0
        if with_kp:
            w1, w2 = cr.gather(kp1, kp2, want)
            assert np.array_equal(xy1[:n], w1) and np.array_equal(xy2[:n], w2), what + ": gathered points"
        assert (xy1[m:] == SENT_F).all() and (xy2[m:] == SENT_F).all(), what + ": point written behind the survivors"

    def untouched(self):
        self.torch.cuda.synchronize()
        return (int(self.n.item()) == -1 and bool((self.good == SENT_I).all()) and bool((self.xy1 == SENT_F).all()) and
                bool((self.xy2 == SENT_F).all()))


# ---- (a) the three predicates on synthetic records -----------------------------------------------------------------------

SMALL = (65536, 65537, 66309, 131073)       # 256 blocks; 257 blocks: the last polls all 256 lanes once; 260 blocks, ragged
                                            # tail: blocks 257-259 poll twice; 513 blocks: three rounds
LARGE = (ROW_LIMIT - 1, ROW_LIMIT)          # 4096 blocks, 16 rounds
CASES_A = [(nq, p) for nq in SMALL for p in cr.PATTERNS] + [(nq, p) for nq in LARGE for p in ("all", "last_only", "half")]


@functools.lru_cache(maxsize=1)
def _device_records(nq, pattern):
    """The records of one (size, pattern), generated and uploaded once for the three rules."""
    r = cr.make_records(nq, pattern, np.random.default_rng([nq, cr.PATTERNS.index(pattern)]), k=3)
    r.fwd2 = np.ascontiguousarray(r.fwd[:, :2])
    r.d_fwd3, r.d_fwd2, r.d_rev, r.d_mid = _up_records(r.fwd), _up_records(r.fwd2), _up_records(r.rev), _up_records(r.mid[:, None])
    r.d_kp1, r.d_kp2 = _up(r.kp1), _up(r.kp2)
    r.out = _Outputs(nq)
    r.want = r.fwd[r.keep, 0].copy()                    # by construction; the numpy rules agree (test_compaction_ref_cpu.py)
    return r


def _kp(r, with_kp):
    return (r.d_kp1.data_ptr(), r.d_kp2.data_ptr()) if with_kp else (0, 0)


def _check_ratio(ctx, nq, pattern):
    r = _device_records(nq, pattern)
    assert_matches_equal(cr.ratio_rule(r.fwd, r.ratio), r.want, "reference")
    for k, d_knn in ((2, r.d_fwd2), (3, r.d_fwd3)):
        for with_kp in (True, False):
            for rep in range(2):                           # the second call reuses the epoch-tagged words
                r.out.reset()
                ctx.filter_ratio_gather_dev(d_knn.data_ptr(), nq, k, r.ratio, *_kp(r, with_kp), *r.out.ptrs(with_kp))
                ctx.synchronize()
                r.out.check(r.want, r.kp1, r.kp2, with_kp, "ratio k=%d kp=%d rep=%d" % (k, with_kp, rep))


def _check_midpoint(ctx, nq, pattern):
    import torch
    r = _device_records(nq, pattern)
    want, lo, hi = cr.midpoint_rule(r.mid)
    assert_matches_equal(want, r.mid[r.keep], "reference")
    assert [lo, hi] == r.mid_minmax
    d_mm = torch.empty(2, dtype=torch.float64, device=_dev())
    for with_kp in (True, False):
        for rep in range(2):
            r.out.reset()
            d_mm.fill_(SENT_F)
            ctx.filter_midpoint_gather_dev(r.d_mid.data_ptr(), nq, 1, *_kp(r, with_kp), *r.out.ptrs(with_kp), d_mm.data_ptr())
            ctx.synchronize()
            r.out.check(want, r.kp1, r.kp2, with_kp, "midpoint kp=%d rep=%d" % (with_kp, rep))
            assert d_mm.cpu().numpy().tolist() == r.mid_minmax
    # the same rule reading the first record of each k = 2 row of a list whose distances are the midpoint ones
    two = r.fwd2.copy()
    two["distance"][:, 0] = r.mid["distance"]
    two["trainIdx"][:, 0] = r.mid["trainIdx"]
    d_two = _up_records(two)
    r.out.reset()
    ctx.filter_midpoint_gather_dev(d_two.data_ptr(), nq, 2, *_kp(r, True), *r.out.ptrs(True), 0)
    ctx.synchronize()
    r.out.check(want, r.kp1, r.kp2, True, "midpoint k=2")


def _check_cross(ctx, nq, pattern):
    r = _device_records(nq, pattern)
    for flags in (0, FWD | REV):
        assert_matches_equal(cr.cross_rule(r.fwd2, r.rev, flags, r.ratio), r.want, "reference flags %d" % flags)
        for with_kp in (True, False):
            for rep in range(2):
                r.out.reset()
                ctx.filter_cross_gather_dev(r.d_fwd2.data_ptr(), nq, 2, r.d_rev.data_ptr(), r.nt, 2, flags, r.ratio,
                                            *_kp(r, with_kp), *r.out.ptrs(with_kp))
                ctx.synchronize()
                r.out.check(r.want, r.kp1, r.kp2, with_kp, "cross flags=%d kp=%d rep=%d" % (flags, with_kp, rep))


@pytest.mark.parametrize("nq,pattern,rule", [(nq, p, rule) for nq, p in CASES_A for rule in ("ratio", "midpoint", "cross")])
def test_gather_past_one_poll_round(ctx, nq, pattern, rule):
    """(the three rules of one (size, pattern) run back to back: they share its records on the device)"""
    {"ratio": _check_ratio, "midpoint": _check_midpoint, "cross": _check_cross}[rule](ctx, nq, pattern)


# ---- (b) the 1M-row limit -----------------------------------------------------------------------------------------------------

def test_more_than_1m_rows_is_refused_and_the_context_survives(ctx):
    import torch
    nq = ROW_LIMIT + 1
    d_rec = torch.zeros((nq, 8), dtype=torch.int32, device=_dev())          # trainIdx 0 everywhere: valid records
    d_kp = torch.zeros((nq, 2), dtype=torch.float32, device=_dev())
    d_mm = torch.full((2,), SENT_F, dtype=torch.float64, device=_dev())
    out = _Outputs(nq)
    small = cr.make_records(300, "half", np.random.default_rng(300))
    d_f, d_r, d_m = _up_records(small.fwd), _up_records(small.rev), _up_records(small.mid[:, None])
    d_k1, d_k2 = _up(small.kp1), _up(small.kp2)
    want = small.fwd[small.keep, 0]
    kp = (d_kp.data_ptr(), d_kp.data_ptr())
    skp = (d_k1.data_ptr(), d_k2.data_ptr())
    calls = {
        "ratio": (lambda: ctx.filter_ratio_gather_dev(d_rec.data_ptr(), nq, 2, 0.8, *kp, *out.ptrs(True)),
                  lambda: ctx.filter_ratio_gather_dev(d_f.data_ptr(), 300, 2, small.ratio, *skp, *out.ptrs(True)), want),
        "midpoint": (lambda: ctx.filter_midpoint_gather_dev(d_rec.data_ptr(), nq, 2, *kp, *out.ptrs(True), d_mm.data_ptr()),
                     lambda: ctx.filter_midpoint_gather_dev(d_m.data_ptr(), 300, 1, *skp, *out.ptrs(True), d_mm.data_ptr()),
                     small.mid[small.keep]),
        "cross": (lambda: ctx.filter_cross_gather_dev(d_rec.data_ptr(), nq, 2, d_rec.data_ptr(), nq, 2, FWD | REV, 0.8, *kp,
                                                      *out.ptrs(True)),
                  lambda: ctx.filter_cross_gather_dev(d_f.data_ptr(), 300, 2, d_r.data_ptr(), 300, 2, FWD | REV, small.ratio,
                                                      *skp, *out.ptrs(True)), want),
    }
    for name, (too_many, fits, want_small) in calls.items():
        out.reset()
        d_mm.fill_(SENT_F)
        with pytest.raises(pm.PmError) as e:
            too_many()
        assert e.value.status == api.PM_E_UNSUPPORTED and "1M query rows" in str(e.value), name
        ctx.synchronize()
        assert out.untouched() and (d_mm.cpu().numpy() == SENT_F).all(), name
        fits()                                              # the context is not disturbed
        ctx.synchronize()
        out.check(want_small, small.kp1, small.kp2, True, name + " after the refusal")
        assert d_mm.cpu().numpy().tolist() == (small.mid_minmax if name == "midpoint" else [SENT_F, SENT_F]), name


# ---- (c) the fused form past 256 tiles -----------------------------------------------------------------------------------------

def _sift_quant(x):
    x = x / np.linalg.norm(x, axis=1, keepdims=True)
    x = np.minimum(x, 0.2)
    x = x / np.linalg.norm(x, axis=1, keepdims=True)
    return np.clip(np.rint(x * 512.0), 0, 255).astype(np.float32)


def _descriptors(kind, nq, nt, train_set, seed):
    """kind 'float': unit-norm general floats; 'int': SIFT-like u8-valued floats.  train_set:
    mix   two queries in three are noisy copies of a train row, the others are unrelated
    all   every query is a train row plus small noise; the other train rows are far away
    none  the train set is every row twice, so d1 == d2 and the strict test fails for every query"""
    rng = np.random.default_rng([seed, nq, nt])
    base_n = nt // 2 if train_set == "none" else nt
    g = rng.standard_normal((base_n, 128))
    g = np.abs(g) if kind == "int" else g
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    src = np.arange(nq) % base_n
    sigma = 0.01 if train_set == "all" else 0.04
    q = g[src] + sigma * rng.standard_normal((nq, 128))
    if train_set != "all":
        loose = np.arange(nq) % 3 == 0
        q[loose] = rng.standard_normal((int(loose.sum()), 128))
    if kind == "int":
        q, t = _sift_quant(np.abs(q)), _sift_quant(g)
    else:
        q, t = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32), g.astype(np.float32)
    if train_set == "none":
        t = np.repeat(t, 2, axis=0)
    kp1 = (rng.random((nq, 2)) * 900).astype(np.float32)
    kp2 = (rng.random((t.shape[0], 2)) * 600).astype(np.float32)
    return np.ascontiguousarray(q), np.ascontiguousarray(t), kp1, kp2


TRAIN_SETS = {"mix": 300, "all": 150, "none": 200}        # name -> nt (64 <= nt <= 300)


@functools.lru_cache(maxsize=2)
def _fused_case(kind, nq, train_set):
    """Descriptors, keypoints and the expected records / survivors of one case: the oracle's 2-NN + the numpy ratio rule,
    computed once and shared by the routes that read this data."""
    from oracle import pm_oracle
    pm_oracle.build()
    q, t, kp1, kp2 = _descriptors(kind, nq, TRAIN_SETS[train_set], train_set, seed=0xF05E)
    knn = pm_oracle.bf_knn_l2(q, t, 2, nthreads=THREADS)
    good = cr.ratio_rule(knn, cr.RATIO)
    if train_set == "all":
        assert good.size == nq, "vacuous input: not every query survives"
    elif train_set == "none":
        assert good.size == 0 and (knn["distance"][:, 0] == knn["distance"][:, 1]).all(), "vacuous input"
    else:
        assert nq // 4 < good.size < nq - nq // 8, "vacuous input"
    return q, t, kp1, kp2, knn, good


ROUTES = {                       # name -> (descriptor kind, knn flags or None for true u8 rows, queries per tile)
    "auto": ("float", 0, 32), "integer": ("int", api.PM_KNN_HINT_INTEGER, 32), "force_f32": ("float", api.PM_KNN_FORCE_F32, 32),
    "hint_u8": ("int", api.PM_KNN_HINT_U8, 16), "u8_rows": ("int", None, 16),
}
CASES_C = [(route, (256 * per + extra), ts) for kind in ("float", "int") for per in (32, 16)
           for extra in (0, 1, per + 1, 256 * per + 1) for ts in TRAIN_SETS
           for route, (rk, _, rper) in ROUTES.items() if rk == kind and rper == per]


def _run_fused(c, route, q, t, kp1, kp2, knn, good, fusion, with_knn, with_kp, what):
    """One configuration of the one-call matcher + filter, twice, checked against (knn, good)."""
    import torch
    flags = ROUTES[route][1]
    nq, nt = q.shape[0], t.shape[0]
    d_q, d_t = (_up(q.astype(np.uint8)), _up(t.astype(np.uint8))) if flags is None else (_up(q), _up(t))
    d_kp1, d_kp2 = _up(kp1), _up(kp2)
    d_knn = torch.empty((nq, 8), dtype=torch.int32, device=_dev())
    out = _Outputs(nq)
    kp = (d_kp1.data_ptr(), d_kp2.data_ptr()) if with_kp else (0, 0)
    c.set_option(api.PM_OPT_FILTER_FUSION, fusion)
    try:
        for rep in range(2):                               # twice: arrival words back at zero, the epoch moves on
            out.reset()
            d_knn.fill_(SENT_I)
            torch.cuda.synchronize()
            tail = (d_knn.data_ptr() if with_knn else 0,) + out.ptrs(with_kp)
            if flags is None:
                c.bf_knn_l2_u8_ratio_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, 128, cr.RATIO, *kp, *tail)
            else:
                c.bf_knn_l2_ratio_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, 128, flags, cr.RATIO, *kp, *tail)
            c.synchronize()
            w = "%s rep=%d" % (what, rep)
            assert c.filter_fusion_gave_up() == 0, w
            out.check(good, kp1, kp2, with_kp, w)
            rec = d_knn.cpu().numpy()
            if with_knn:
                assert_matches_equal(rec.view(cr.MATCH_DTYPE).reshape(nq, 2), knn, w + ": records")
            else:
                assert (rec == SENT_I).all(), w + ": record buffer was not given"
    finally:
        c.set_option(api.PM_OPT_FILTER_FUSION, 0)


@pytest.mark.parametrize("route,nq,train_set", CASES_C)
def test_fused_compaction_past_256_tiles(ctx, route, nq, train_set):
    q, t, kp1, kp2, knn, good = _fused_case(ROUTES[route][0], nq, train_set)
    what = "%s nq=%d %s" % (route, nq, train_set)
    _run_fused(ctx, route, q, t, kp1, kp2, knn, good, 2, True, True, what + " fusion=2")
    _run_fused(ctx, route, q, t, kp1, kp2, knn, good, 2, True, False, what + " fusion=2, no keypoints")
    if ROUTES[route][1] is not None:                        # (the u8-row entry point requires the record buffer)
        _run_fused(ctx, route, q, t, kp1, kp2, knn, good, 0, False, True, what + " d_knn=NULL")


# ---- (d) growth of the fused words, and the matcher at a large query count ------------------------------------------

def test_fused_words_grow_past_4096_tiles_and_the_matcher_at_131105_queries(oracle):
    nq_big, nt = 131105, 40                                  # 4098 tiles of 32 queries
    q, t, kp1, kp2 = _descriptors("int", nq_big, nt, "mix", seed=0xD0)
    knn = oracle.bf_knn_l2(q, t, 2, nthreads=THREADS)        # once; a prefix of the queries has a prefix of the records
    steps = (("integer", 4000, 2), ("integer", nq_big, 2),   # the second step needs 4098 > 4096 tiles: reallocation
             ("integer", 100, 2), ("u8_rows", 65553, 2),     # 4098 tiles of 16 queries
             ("integer", nq_big, 2), ("integer", nq_big, 1))  # 1: the two-launch form, the plain matcher + filter
    c = pm.Context(0)                                        # its own context: the tile words start at their first size
    try:
        for i, (route, nq, fusion) in enumerate(steps):
            good = cr.ratio_rule(knn[:nq], cr.RATIO)
            assert 0 < good.size < nq
            _run_fused(c, route, q[:nq], t, kp1[:nq], kp2, knn[:nq], good, fusion, True, True,
                       "step %d: %s nq=%d fusion=%d" % (i + 1, route, nq, fusion))
    finally:
        c.close()


# ---- (e) pm_concat_points_dev ----------------------------------------------------------------------------------------------

def _concat_case(ctx, parts, stride, counts):
    import torch
    rng = np.random.default_rng([parts, stride])
    a = rng.random((parts, stride, 2), dtype=np.float32)
    b = rng.random((parts, stride, 2), dtype=np.float32)
    counts = np.asarray(counts, np.int32)
    d_a, d_b, d_c = _up(a), _up(b), _up(counts)
    o1 = torch.full((parts * stride, 2), SENT_F, dtype=torch.float32, device=_dev())
    o2 = torch.full((parts * stride, 2), SENT_F, dtype=torch.float32, device=_dev())
    d_n = torch.full((1,), -1, dtype=torch.int32, device=_dev())
    torch.cuda.synchronize()
    ctx.concat_points_dev(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), parts, stride, o1.data_ptr(), o2.data_ptr(),
                          d_n.data_ptr())
    ctx.synchronize()
    clamped = np.clip(counts, 0, stride)                    # a count below 0 is read as 0, one above the stride as the stride
    take = np.arange(stride)[None, :] < clamped[:, None]
    want1, want2 = a[take], b[take]
    total = int(clamped.sum())
    assert int(d_n.item()) == total == want1.shape[0]
    g1, g2 = o1.cpu().numpy(), o2.cpu().numpy()
    assert np.array_equal(g1[:total], want1) and np.array_equal(g2[:total], want2)
    assert (g1[total:] == SENT_F).all() and (g2[total:] == SENT_F).all()
    return total


def test_concat_points_uneven_parts_and_clamped_counts(ctx):
    parts, stride = 64, 1000                                 # four workgroups per part, the last one ragged
    counts = np.random.default_rng(64).integers(1, stride, parts)
    counts[[0, 5, 17, 30, 31, 63]] = [0, stride, -3, stride + 500, 2 ** 31 - 1, 257]
    counts[40:43] = [256, 255, -2 ** 31]
    total = _concat_case(ctx, parts, stride, counts)
    assert 0 < total < parts * stride


def test_concat_points_part_limit(ctx):
    import torch
    parts = 65535
    counts = np.random.default_rng(7).integers(-1, 3, parts)  # -1, 0, 1, 2 -> 0, 0, 1, 1
    assert 0 < _concat_case(ctx, parts, 1, counts) < parts
    buf = torch.zeros((parts + 1, 2), dtype=torch.float32, device=_dev())
    cnt = torch.zeros(parts + 1, dtype=torch.int32, device=_dev())
    d_n = torch.full((1,), -1, dtype=torch.int32, device=_dev())
    torch.cuda.synchronize()
    with pytest.raises(pm.PmError) as e:
        ctx.concat_points_dev(buf.data_ptr(), buf.data_ptr(), cnt.data_ptr(), parts + 1, 1, buf.data_ptr(), buf.data_ptr(),
                              d_n.data_ptr())
    assert e.value.status == api.PM_E_INVALID
    ctx.synchronize()
    assert int(d_n.item()) == -1
