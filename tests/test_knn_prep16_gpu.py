"""GPU parity of the f16 prep family (knn_l2_prep16: norms + premise + integer copies; knn_l2_prep16g: scaled copies from the
stored norms; knn_l2_prep16u: both in one launch) at the shapes and values where it can go wrong: pad rows, partial last
workgroups of the query and of the train half of its grid, the block where the two halves meet, both widths of the copies
(128 / 256 columns), both ways of reading a row (16-byte vectors / element by element, also dim % 4 == 0 on a misaligned
base), and the edges of the premises (the integer bound, the unit-norm bound, a query too large to rank, NaN and inf).

Every comparison of a result is exact: trainIdx and the distance bits against oracle.pm_oracle.bf_knn_l2 on the same arrays.
knn_stats() (route, nonfinite, rescans) must equal tests/golden/knn_prep16_stats.json, recorded with
tools/record_knn_prep16_stats.py on the library of the commit before the kernels were filed by stage: the arithmetic of the
prep kernels decides the candidate lists, and with them the re-scan counts, so none of the three may move.  (Two recordings
of that library agreed on every case, rescans included, so every case asserts all three.)

Instantiations reached (knn_l2_plan.hpp: dp16 = 128 up to dim 128, else 256; vec = dim % 4 == 0 and aligned pointers):
dim 4, 128 -> <128, true>; 7, and 128 on a misaligned base -> <128, false>; 256 -> <256, true>; 130 -> <256, false>, each for
knn_l2_prep16<false, ..> (+ knn_l2_prep16g on the automatic route) and, with PM_KNN_HINT_UNIT_NORM, for knn_l2_prep16u;
PM_OPT_KNN_SEEDED = 2 with PM_KNN_HINT_INTEGER -> knn_l2_prep16<true, 128, true>."""
import json
import os

import numpy as np
import pytest

import points_matching_amd as pm
from points_matching_amd.api import PM_KNN_HINT_INTEGER, PM_KNN_HINT_UNIT_NORM, PM_OPT_KNN_SEEDED

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2), (15, 17), (16, 16), (63, 65), (257, 129), (300, 1000)]
DIMS = [4, 7, 128, 130, 256]
KINDS = ["int_bound", "int_past", "gen_1e-3", "gen_1e4", "unit"]
EDGE_SHAPE = (63, 65)                    # pad rows and partial workgroups on both halves
EDGE_DIMS = [128, 130]                   # both widths of the copies
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_prep16_stats.json")


def _bound(dim):
    return 361 if dim <= 128 else 255    # floor(sqrt(2^24 / DP)): every partial sum of a dot product stays below 2^24


def _plant(rng, q, t, noise):
    """a third of the queries get a near copy of a train row (from its end: the last, partial block takes part)"""
    m = min(q.shape[0], t.shape[0]) // 3
    if m:
        q[:m] = t[t.shape[0] - m:] + noise(m)
    return q, t


def make(kind, nq, nt, dim, seed):
    """-> (q, t, flags) of one seeded case"""
    rng = np.random.default_rng(seed)
    b = _bound(dim)
    if kind in ("int_bound", "int_past"):
        q = rng.integers(-b, b + 1, (nq, dim)).astype(np.float32)
        t = rng.integers(-b, b + 1, (nt, dim)).astype(np.float32)
        q, t = _plant(rng, q, t, lambda m: rng.integers(-1, 2, (m, dim)))
        np.clip(q, -b, b, out=q)
        q[-1], t[0] = b, -b                                  # whole rows at the bound: the largest norm the premise allows
        t[-1, dim - 1], q[0, 0] = b, -b
        if kind == "int_past":
            t[nt // 2, dim // 2] = b + 1                     # one element one past the bound: knn_l2_prep16g does the work
        return q, t, 0
    if kind.startswith("gen_"):
        scale = np.float32(float(kind[4:]))
        q = (rng.standard_normal((nq, dim)) * scale).astype(np.float32)
        t = (rng.standard_normal((nt, dim)) * scale).astype(np.float32)
        q, t = _plant(rng, q, t, lambda m: (rng.standard_normal((m, dim)) * scale * 0.05).astype(np.float32))
        return q, t, 0
    assert kind.startswith("unit")
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    t = rng.standard_normal((nt, dim)).astype(np.float32)
    q, t = _plant(rng, q, t, lambda m: (rng.standard_normal((m, dim)) * 0.05).astype(np.float32))
    q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
    t /= np.linalg.norm(t, axis=1, keepdims=True).astype(np.float32)
    if kind == "unit_train_1.01":
        t[nt - 1] *= np.float32(1.01)                        # beyond the stated bound: the call stays exact
    if kind == "unit_query_16":
        q[nq - 1] *= np.float32(16.0)                        # more than 8x every train row: unranked, scanned exactly
    return q, t, PM_KNN_HINT_UNIT_NORM


def edge_cases():
    """-> (id, q, t, k, flags, misaligned, seeded) of the cases that ride on one shape"""
    nq, nt = EDGE_SHAPE
    for dim in EDGE_DIMS:
        for kind in ("unit_train_1.01", "unit_query_16"):
            q, t, flags = make(kind, nq, nt, dim, 9000 + dim)
            yield "%s-%d" % (kind, dim), q, t, 2, flags, False, False
        for name, poison in (("nan", np.nan), ("inf", np.inf)):
            for side in ("q", "t"):
                q, t, flags = make("gen_1e-3", nq, nt, dim, 9100 + dim)
                (q if side == "q" else t)[-1, dim - 1] = poison
                yield "%s_%s-%d" % (name, side, dim), q, t, 2, flags, False, False
        for kind in ("int_bound", "gen_1e4", "unit"):
            q, t, flags = make(kind, nq, nt, dim, 9200 + dim)
            yield "k4_%s-%d" % (kind, dim), q, t, 4, flags, False, False
    for kind in ("int_bound", "int_past", "unit"):           # dim % 4 == 0 on a base pointer that is not 16-byte aligned
        q, t, flags = make(kind, nq, nt, 128, 9300)
        yield "misaligned_%s-128" % kind, q, t, 2, flags, True, False
    q, t, _ = make("int_bound", nq, nt, 128, 9400)
    yield "seeded_int_bound-128", q, t, 2, PM_KNN_HINT_INTEGER, False, True


def knn_dev(ctx, q, t, k, flags, misaligned=False, seeded=False):
    """-> (records, knn_stats()) of pm_bf_knn_l2_f32_dev on device copies of q and t"""
    import torch
    dev = torch.device("cuda", 0)

    def put(a):
        if not misaligned:
            return torch.from_numpy(a).to(dev)
        flat = torch.zeros(a.size + 1, dtype=torch.float32, device=dev)
        flat[1:] = torch.from_numpy(a.reshape(-1)).to(dev)
        return flat[1:]                                      # one float past a 256-byte aligned allocation

    d_q, d_t = put(q), put(t)
    assert (d_q.data_ptr() % 16 != 0) == misaligned
    d_out = torch.zeros((q.shape[0], k, 4), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.knn_diag_enable(True)
    try:
        if seeded:
            ctx.set_option(PM_OPT_KNN_SEEDED, 2)
        ctx.bf_knn_l2_dev(d_q.data_ptr(), q.shape[0], d_t.data_ptr(), t.shape[0], q.shape[1], k, d_out.data_ptr(), flags)
        ctx.synchronize()
        st = ctx.knn_stats()
    finally:
        ctx.set_option(PM_OPT_KNN_SEEDED, 0)
        ctx.knn_diag_enable(False)
    return d_out.cpu().numpy().view(pm.MATCH_DTYPE).reshape(q.shape[0], k), st


def shape_id(kind, nq, nt, dim):
    return "%s-%dx%dx%d" % (kind, nq, nt, dim)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _check(ctx, oracle, golden, cid, q, t, k, flags, misaligned=False, seeded=False):
    from util import assert_matches_equal
    want = oracle.bf_knn_l2(q, t, k, nthreads=8)
    got, st = knn_dev(ctx, q, t, k, flags, misaligned, seeded)
    assert_matches_equal(got, want, cid)
    assert st == golden[cid], (cid, st, golden[cid])


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("nq,nt", SHAPES)
def test_shapes(ctx, oracle, golden, nq, nt, dim):
    for i, kind in enumerate(KINDS):
        q, t, flags = make(kind, nq, nt, dim, 100000 * nq + 100 * nt + dim + 7 * i)
        _check(ctx, oracle, golden, shape_id(kind, nq, nt, dim), q, t, 2, flags)


@pytest.mark.parametrize("case", list(edge_cases()), ids=[c[0] for c in edge_cases()])
def test_edges(ctx, oracle, golden, case):
    cid, q, t, k, flags, misaligned, seeded = case
    _check(ctx, oracle, golden, cid, q, t, k, flags, misaligned, seeded)
