"""GPU: cross-check matching (docs/SPEC.md S41-S42).  The fused device filter against the host rule on the same records;
the one-call forms on all three descriptor routes against the oracle's k-NN both ways + the numpy rule of cross_ref.py,
bit for bit; the chain into the device RANSAC entry points; the stream-capture refusal; the CLI switch."""
import os
import subprocess

import numpy as np
import pytest

import points_matching_amd as pm
from points_matching_amd import api, build, io, synth
from cross_ref import cross_ref
from util import assert_matches_equal

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FWD, REV = api.PM_CROSS_RATIO_FWD, api.PM_CROSS_RATIO_REV
ALL_FLAGS = (0, FWD, REV, FWD | REV)
THREADS = 16


def _records(t):
    return t.cpu().numpy().view(pm.MATCH_DTYPE).reshape(t.shape[0], -1)


# ---- the fused filter on given records ---------------------------------------------------------------------------------

def _random_records(rng, nq, nt):
    """Forward / reverse 2-NN lists with about half the rows mutual, out-of-range and -1 first neighbours, tail rows
    and equal distances (the ratio test sees d1 == d2)."""
    fwd = np.zeros((nq, 2), pm.MATCH_DTYPE)
    rev = np.zeros((nt, 2), pm.MATCH_DTYPE)
    fwd["queryIdx"] = np.arange(nq)[:, None]
    rev["queryIdx"] = np.arange(nt)[:, None]
    fwd["trainIdx"] = rng.integers(0, nt, (nq, 2))
    rev["trainIdx"] = rng.integers(0, nq, (nt, 2))
    fwd["distance"] = np.sort(rng.random((nq, 2)).astype(np.float32), axis=1)
    rev["distance"] = np.sort(rng.random((nt, 2)).astype(np.float32), axis=1)
    mutual = rng.permutation(nq)[:nq // 2 + 1]                       # make these rows mutual where the train row is free
    rev["trainIdx"][fwd["trainIdx"][mutual, 0], 0] = mutual
    odd = rng.permutation(nq)[:nq // 16]
    fwd["trainIdx"][odd, 0] = rng.choice([-1, nt, nt + 5, 2 ** 31 - 1, -2 ** 31], odd.size)
    tail = rng.permutation(nq)[:nq // 20]
    fwd["trainIdx"][tail, 1] = -1
    fwd["distance"][tail, 1] = np.inf
    tie = rng.permutation(nt)[:nt // 20]
    rev["distance"][tie, 1] = rev["distance"][tie, 0]
    return fwd, rev


@pytest.mark.parametrize("nq", [1, 255, 256, 257, 8192, 40000])
def test_fused_filter_equals_host_rule(ctx, nq):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(nq)
    nt = max(1, (nq * 3) // 4 + 3)
    fwd, rev = _random_records(rng, nq, nt)
    kp1 = (rng.random((nq, 2)) * 900).astype(np.float32)
    kp2 = (rng.random((nt, 2)) * 600).astype(np.float32)
    d_fwd = torch.from_numpy(fwd.view(np.int32).reshape(nq, 8)).to(dev)
    d_rev = torch.from_numpy(rev.view(np.int32).reshape(nt, 8)).to(dev)
    d_kp1, d_kp2 = torch.from_numpy(kp1).to(dev), torch.from_numpy(kp2).to(dev)
    d_good = torch.zeros((nq, 4), dtype=torch.int32, device=dev)
    d_xy1 = torch.zeros((nq, 2), dtype=torch.float32, device=dev)
    d_xy2 = torch.zeros((nq, 2), dtype=torch.float32, device=dev)
    d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    kept_any = dropped_any = False
    for flags in ALL_FLAGS:
        for ratio in (0.8, 1.0):
            want = api.filter_cross(fwd, rev, flags, ratio)
            kept_any |= want.size > 0
            dropped_any |= want.size < nq
            for with_kp in (True, False):
                for rep in range(2):                               # the second call reuses the epoch-tagged words
                    d_n.fill_(-1)
                    d_xy1.fill_(-7.0)
                    torch.cuda.synchronize()
                    ctx.filter_cross_gather_dev(d_fwd.data_ptr(), nq, 2, d_rev.data_ptr(), nt, 2, flags, ratio,
                                                d_kp1.data_ptr() if with_kp else 0, d_kp2.data_ptr() if with_kp else 0,
                                                d_good.data_ptr(), d_xy1.data_ptr() if with_kp else 0,
                                                d_xy2.data_ptr() if with_kp else 0, d_n.data_ptr())
                    ctx.synchronize()
                    n = int(d_n.item())
                    assert n == want.size, (flags, ratio, with_kp, rep)
                    assert_matches_equal(_records(d_good)[:n, 0], want, "fused filter flags %d" % flags)
                    if with_kp:
                        assert np.array_equal(d_xy1.cpu().numpy()[:n], kp1[want["queryIdx"]])
                        assert np.array_equal(d_xy2.cpu().numpy()[:n], kp2[want["trainIdx"]])
                    else:
                        assert (d_xy1.cpu().numpy() == -7.0).all()
    assert kept_any and (dropped_any or nq == 1)
    # the k = 1 form of the plain rule: every second record dropped from the lists
    f1, r1 = np.ascontiguousarray(fwd[:, :1]), np.ascontiguousarray(rev[:, :1])
    d_f1 = torch.from_numpy(f1.view(np.int32).reshape(nq, 4)).to(dev)
    d_r1 = torch.from_numpy(r1.view(np.int32).reshape(nt, 4)).to(dev)
    torch.cuda.synchronize()
    ctx.filter_cross_gather_dev(d_f1.data_ptr(), nq, 1, d_r1.data_ptr(), nt, 1, 0, 0.8, 0, 0, d_good.data_ptr(), 0, 0,
                                d_n.data_ptr())
    ctx.synchronize()
    want = api.filter_cross(f1, r1, 0)
    assert int(d_n.item()) == want.size
    assert_matches_equal(_records(d_good)[:want.size, 0], want, "k = 1")


def test_fused_filter_argument_errors_and_empty_sets(ctx):
    import torch
    dev = torch.device("cuda", 0)
    buf = torch.zeros((64, 4), dtype=torch.int32, device=dev)
    d_n = torch.full((1,), 5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for kf, kr, flags in ((1, 2, FWD), (2, 1, REV), (2, 2, 4), (0, 1, 0)):
        with pytest.raises(pm.PmError) as e:
            ctx.filter_cross_gather_dev(buf.data_ptr(), 8, kf, buf.data_ptr(), 8, kr, flags, 0.8, 0, 0, buf.data_ptr(), 0, 0,
                                        d_n.data_ptr())
        assert e.value.status == api.PM_E_INVALID
    for nq, nt in ((0, 8), (8, 0), (0, 0)):
        d_n.fill_(5)
        torch.cuda.synchronize()
        ctx.filter_cross_gather_dev(buf.data_ptr() if nq else 0, nq, 1, buf.data_ptr() if nt else 0, nt, 1, 0, 0.8, 0, 0,
                                    buf.data_ptr(), 0, 0, d_n.data_ptr())
        ctx.synchronize()
        assert int(d_n.item()) == 0


# ---- the one-call forms ----------------------------------------------------------------------------------------------------

_ORACLE_CACHE = {}


def _oracle_both_ways(oracle, key, q, t, binary):
    """The oracle's 2-NN lists of (q, t) and (t, q); the k = 1 lists are their first columns (S3)."""
    if key not in _ORACLE_CACHE:
        knn = oracle.bf_knn_hamming if binary else oracle.bf_knn_l2
        qq, tt = (q, t) if binary else (q.astype(np.float32), t.astype(np.float32))
        _ORACLE_CACHE[key] = (knn(qq, tt, 2, nthreads=THREADS), knn(tt, qq, 2, nthreads=THREADS))
    return _ORACLE_CACHE[key]


def _run_one_call(ctx, route, q, t, kp1, kp2, knn_flags, cross_flags, ratio):
    """route: 'f32' | 'u8' | 'hamming'.  Returns (fwd, rev, good, xy1, xy2) as the device left them."""
    import torch
    dev = torch.device("cuda", 0)
    nq, nt, width = q.shape[0], t.shape[0], q.shape[1]
    kf, kr = (2 if cross_flags & FWD else 1), (2 if cross_flags & REV else 1)
    d_q, d_t = torch.from_numpy(np.ascontiguousarray(q)).to(dev), torch.from_numpy(np.ascontiguousarray(t)).to(dev)
    d_kp1, d_kp2 = torch.from_numpy(kp1).to(dev), torch.from_numpy(kp2).to(dev)
    d_fwd = torch.full((nq, kf * 4), -3, dtype=torch.int32, device=dev)
    d_rev = torch.full((nt, kr * 4), -3, dtype=torch.int32, device=dev)
    d_good = torch.zeros((nq, 4), dtype=torch.int32, device=dev)
    d_xy1 = torch.zeros((nq, 2), dtype=torch.float32, device=dev)
    d_xy2 = torch.zeros((nq, 2), dtype=torch.float32, device=dev)
    d_n = torch.full((1,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    tail = (cross_flags, ratio, d_kp1.data_ptr(), d_kp2.data_ptr(), d_fwd.data_ptr(), d_rev.data_ptr(), d_good.data_ptr(),
            d_xy1.data_ptr(), d_xy2.data_ptr(), d_n.data_ptr())
    if route == "f32":
        ctx.bf_match_cross_l2_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, width, knn_flags, *tail)
    elif route == "u8":
        ctx.bf_match_cross_l2_u8_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, width, *tail)
    else:
        ctx.bf_match_cross_hamming_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, width, *tail)
    ctx.synchronize()
    n = int(d_n.item())
    assert 0 <= n <= nq
    return (_records(d_fwd), _records(d_rev), _records(d_good)[:n, 0], d_xy1.cpu().numpy()[:n], d_xy2.cpu().numpy()[:n])


def _check_one_call(ctx, oracle, key, route, q, t, knn_flags=0, flag_set=ALL_FLAGS, ratio=0.8, binary=False):
    fwd2, rev2 = _oracle_both_ways(oracle, key, q, t, binary)
    nq, nt = q.shape[0], t.shape[0]
    rng = np.random.default_rng(nq * 7 + nt)
    kp1 = (rng.random((nq, 2)) * 900).astype(np.float32)
    kp2 = (rng.random((nt, 2)) * 600).astype(np.float32)
    plain = cross_ref(fwd2, rev2)
    print("%s %s: %d x %d, %d mutual survivors" % (key, route, nq, nt, plain.size))
    assert 0 < plain.size < nq, "vacuous input"
    for flags in flag_set:
        kf, kr = (2 if flags & FWD else 1), (2 if flags & REV else 1)
        fwd, rev, good, xy1, xy2 = _run_one_call(ctx, route, q, t, kp1, kp2, knn_flags, flags, ratio)
        what = "%s %s flags %d" % (key, route, flags)
        assert_matches_equal(fwd, fwd2[:, :kf], what + " forward records")
        assert_matches_equal(rev, rev2[:, :kr], what + " reverse records")
        want = cross_ref(fwd2, rev2, flags, ratio)
        assert_matches_equal(good, want, what + " survivors")
        assert np.array_equal(xy1, kp1[want["queryIdx"]]) and np.array_equal(xy2, kp2[want["trainIdx"]])
        # every survivor's reverse record carries the same distance bits
        r = rev[good["trainIdx"], 0]
        assert (r["distance"].view(np.uint32) == good["distance"].view(np.uint32)).all()


@pytest.mark.parametrize("name", ["knn_l2_sift_256x256x128", "knn_l2_surf_96x160x128", "knn_l2_surf_40x50x20_k3",
                                  "knn_hamming_256x256x32"])
def test_one_call_on_golden_fixtures(ctx, oracle, name):
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    if "hamming" in name:
        _check_one_call(ctx, oracle, name, "hamming", g["q"], g["t"], binary=True)
        return
    q, t = g["q"].astype(np.float32), g["t"].astype(np.float32)
    _check_one_call(ctx, oracle, name, "f32", q, t)
    if g["q"].dtype == np.uint8:
        _check_one_call(ctx, oracle, name, "f32", q, t, knn_flags=api.PM_KNN_HINT_U8)
        _check_one_call(ctx, oracle, name, "u8", g["q"], g["t"])
    else:
        _check_one_call(ctx, oracle, name, "f32", q, t, knn_flags=api.PM_KNN_HINT_UNIT_NORM)


@pytest.mark.parametrize("n", [2048, 8192])
def test_one_call_on_c2_and_c3_sift(ctx, oracle, n):
    """C2 (2048 x 2048) and C3 (8192 x 8192) SIFT-128 of synth.pair_workload: float rows on the automatic route, float
    rows with PM_KNN_HINT_U8, and true u8 rows."""
    w = synth.pair_workload(nq=n, nt=n, dim=128)
    key = "pair_sift_%d" % n
    some = ALL_FLAGS if n == 2048 else (FWD, FWD | REV)
    _check_one_call(ctx, oracle, key, "f32", w["q"], w["t"], knn_flags=0, flag_set=some)
    _check_one_call(ctx, oracle, key, "f32", w["q"], w["t"], knn_flags=api.PM_KNN_HINT_U8, flag_set=some)
    _check_one_call(ctx, oracle, key, "u8", w["q"].astype(np.uint8), w["t"].astype(np.uint8), flag_set=some)


def test_one_call_on_general_floats(ctx, oracle):
    q, t, _ = synth.surf_like(2048, 2048, 128, seed=0xC2)
    _check_one_call(ctx, oracle, "surf_2048", "f32", q, t)
    _check_one_call(ctx, oracle, "surf_2048", "f32", q, t, knn_flags=api.PM_KNN_HINT_UNIT_NORM, flag_set=(FWD, REV))


@pytest.mark.parametrize("nq,nt", [(3000, 700), (700, 3000)])
def test_one_call_rectangular(ctx, oracle, nq, nt):
    """nq != nt: the reverse pass is a matcher run of another shape, not a square re-run."""
    w = synth.pair_workload(nq=nq, nt=nt, dim=128, seed=0xD1)
    key = "rect_sift_%dx%d" % (nq, nt)
    _check_one_call(ctx, oracle, key, "f32", w["q"], w["t"], knn_flags=api.PM_KNN_HINT_U8)
    _check_one_call(ctx, oracle, key, "u8", w["q"].astype(np.uint8), w["t"].astype(np.uint8), flag_set=(0, FWD | REV))
    q, t, _ = synth.surf_like(nq, nt, 64, seed=nq)
    _check_one_call(ctx, oracle, "rect_surf_%dx%d" % (nq, nt), "f32", q, t, flag_set=(0, FWD | REV))
    q, t, _ = synth.orb_like(nq, nt, 32, seed=nt)
    _check_one_call(ctx, oracle, "rect_orb_%dx%d" % (nq, nt), "hamming", q, t, flag_set=(0, FWD | REV), binary=True)


def test_one_call_hamming_routes(ctx, oracle):
    q, t, _ = synth.orb_like(2048, 2048, 32, seed=0xC4)                 # ORB-256: matrix-core route
    _check_one_call(ctx, oracle, "orb256_2048", "hamming", q, t, binary=True)
    q, t, _ = synth.orb_like(500, 400, 64, seed=9)                      # 64-byte rows: integer VALU scan
    _check_one_call(ctx, oracle, "orb512_500x400", "hamming", q, t, binary=True)


def test_one_call_on_the_exact_kernel(ctx, oracle):
    q, t, _ = synth.surf_like(300, 260, 30, seed=3)                     # dim % 4 != 0
    _check_one_call(ctx, oracle, "surf_dim30", "f32", q, t)
    q, t, _ = synth.sift_like(260, 300, 30, seed=4)
    _check_one_call(ctx, oracle, "sift_dim30", "u8", q.astype(np.uint8), t.astype(np.uint8), flag_set=(0, FWD | REV))


def test_host_conveniences_and_empty_sets(ctx, oracle):
    q, t, _ = synth.sift_like(300, 200, seed=1300)
    fwd2, rev2 = _oracle_both_ways(oracle, "host_sift", q, t, False)
    for flags in ALL_FLAGS:
        want = cross_ref(fwd2, rev2, flags, 0.8)
        assert_matches_equal(ctx.bf_match_cross_l2(q, t, flags, 0.8), want, "host f32")
        assert_matches_equal(ctx.bf_match_cross_l2(q, t, flags, 0.8, knn_flags=api.PM_KNN_HINT_U8), want, "host f32 u8 hint")
        assert_matches_equal(ctx.bf_match_cross_l2_u8(q.astype(np.uint8), t.astype(np.uint8), flags, 0.8), want, "host u8")
    qb, tb, _ = synth.orb_like(300, 180, seed=1300)
    fb, rb = _oracle_both_ways(oracle, "host_orb", qb, tb, True)
    for flags in ALL_FLAGS:
        assert_matches_equal(ctx.bf_match_cross_hamming(qb, tb, flags, 0.8), cross_ref(fb, rb, flags, 0.8), "host hamming")
    assert ctx.bf_match_cross_l2(q, t[:0], FWD).size == 0 and ctx.bf_match_cross_l2(q[:0], t, REV).size == 0
    assert ctx.bf_match_cross_hamming(qb, tb[:0]).size == 0 and ctx.bf_match_cross_l2_u8(q[:0].astype(np.uint8), t.astype(np.uint8)).size == 0
    with pytest.raises(pm.PmError) as e:
        ctx.bf_match_cross_l2(q, t, 8)
    assert e.value.status == api.PM_E_INVALID


# ---- chain into the estimators ------------------------------------------------------------------------------------------------

def test_chain_into_device_ransac_without_host_copy(ctx):
    """One-call cross-check -> pm_points_view{counts = d_n_good} -> pm_ransac_run_dev and pm_ransac_homography_run_dev on
    one stream; key, model and mask equal the host entry points run on the downloaded survivors."""
    import torch
    dev = torch.device("cuda", 0)
    nq, nt = 1800, 1700
    w = synth.pair_workload(nq=nq, nt=nt, dim=128, seed=12, planted=0.6)
    q, t = w["q"].astype(np.uint8), w["t"].astype(np.uint8)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        ctx.set_stream(s.cuda_stream)
        try:
            d_q, d_t = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
            d_kp1, d_kp2 = torch.from_numpy(w["kp1"]).to(dev), torch.from_numpy(w["kp2"]).to(dev)
            d_fwd = torch.empty((nq, 8), dtype=torch.int32, device=dev)
            d_rev = torch.empty((nt, 4), dtype=torch.int32, device=dev)
            d_good = torch.zeros((nq, 4), dtype=torch.int32, device=dev)
            d_xy1 = torch.zeros((nq, 2), dtype=torch.float32, device=dev)
            d_xy2 = torch.zeros((nq, 2), dtype=torch.float32, device=dev)
            d_n = torch.zeros(1, dtype=torch.int32, device=dev)
            kF, kH = (torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(2))
            dF, dH = (torch.full((9,), 7.0, dtype=torch.float64, device=dev) for _ in range(2))
            mF, mH = (torch.full((nq,), 7, dtype=torch.uint8, device=dev) for _ in range(2))
            cF, cH = (torch.full((1,), 99, dtype=torch.int32, device=dev) for _ in range(2))
            s.synchronize()
            ctx.bf_match_cross_l2_u8_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, 128, FWD, 0.8, d_kp1.data_ptr(),
                                         d_kp2.data_ptr(), d_fwd.data_ptr(), d_rev.data_ptr(), d_good.data_ptr(),
                                         d_xy1.data_ptr(), d_xy2.data_ptr(), d_n.data_ptr())
            ctx.ransac_run_dev(d_xy1.data_ptr(), d_xy2.data_ptr(), nq, d_n.data_ptr(), 0, 1500, 1.0, 0xC0FFEE, kF.data_ptr(),
                               dF.data_ptr(), mF.data_ptr(), cF.data_ptr())
            view = api.PointsView(d_xy1.data_ptr(), d_xy2.data_ptr(), d_n.data_ptr(), 1, nq, 0, 1, 0)
            ctx.ransac_homography_run_dev(view, 0, 1500, 2.0, 0xC0FFEE, kH.data_ptr(), dH.data_ptr(), mH.data_ptr(), nq,
                                          cH.data_ptr())
            ctx.synchronize()
        finally:
            ctx.set_stream(0)
    n = int(d_n.item())
    assert n >= 300
    good = _records(d_good)[:n, 0]
    assert np.unique(good["trainIdx"]).size == n
    xy1, xy2 = d_xy1.cpu().numpy()[:n].copy(), d_xy2.cpu().numpy()[:n].copy()
    assert np.array_equal(xy1, w["kp1"][good["queryIdx"]]) and np.array_equal(xy2, w["kp2"][good["trainIdx"]])
    mask64 = (1 << 64) - 1
    rc, F, mask, ninl, key = ctx.ransac_fundamental(xy1, xy2, 1500, 1.0, 0xC0FFEE)
    assert rc == api.PM_OK and (int(kF.item()) & mask64) == key and int(cF.item()) == ninl
    assert (dF.cpu().numpy().view(np.uint64) == F.reshape(9).view(np.uint64)).all()
    assert (mF.cpu().numpy()[:n] == mask).all() and not mF.cpu().numpy()[n:].any()
    rc, H, mask, ninl, key = ctx.ransac_homography(xy1, xy2, 1500, 2.0, 0xC0FFEE)
    assert rc in (api.PM_OK, api.PM_E_NO_MODEL) and (int(kH.item()) & mask64) == key and int(cH.item()) == ninl
    assert (dH.cpu().numpy().view(np.uint64) == H.reshape(9).view(np.uint64)).all()
    assert (mH.cpu().numpy()[:n] == mask).all() and not mH.cpu().numpy()[n:].any()


# ---- graph capture ----------------------------------------------------------------------------------------------------------

@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_new_entry_points_refuse_a_capturing_stream():
    import gc
    import torch
    n = 600
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    prev = torch.cuda.current_stream(dev)
    torch.cuda.set_stream(st)
    c = pm.Context(0)
    c.set_stream(st.cuda_stream)
    try:
        w = synth.pair_workload(n, n, 128, seed=11, kind="sift")
        o = synth.orb_like(n, n, 32, seed=11)
        d_q, d_t, d_kp1, d_kp2 = [torch.from_numpy(np.ascontiguousarray(w[k])).to(dev) for k in ("q", "t", "kp1", "kp2")]
        d_q8, d_t8 = d_q.to(torch.uint8), d_t.to(torch.uint8)
        d_qb, d_tb = torch.from_numpy(o[0]).to(dev), torch.from_numpy(o[1]).to(dev)
        fwd = torch.empty((n, 8), dtype=torch.int32, device=dev)
        rev = torch.empty((n, 8), dtype=torch.int32, device=dev)
        good = torch.empty((n, 4), dtype=torch.int32, device=dev)
        xy1 = torch.empty((n, 2), dtype=torch.float32, device=dev)
        xy2 = torch.empty((n, 2), dtype=torch.float32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        tail = (FWD | REV, 0.8, d_kp1.data_ptr(), d_kp2.data_ptr(), fwd.data_ptr(), rev.data_ptr(), good.data_ptr(),
                xy1.data_ptr(), xy2.data_ptr(), cnt.data_ptr())
        calls = {
            "f32": lambda: c.bf_match_cross_l2_dev(d_q.data_ptr(), n, d_t.data_ptr(), n, 128, api.PM_KNN_HINT_U8, *tail),
            "u8": lambda: c.bf_match_cross_l2_u8_dev(d_q8.data_ptr(), n, d_t8.data_ptr(), n, 128, *tail),
            "hamming": lambda: c.bf_match_cross_hamming_dev(d_qb.data_ptr(), n, d_tb.data_ptr(), n, 32, *tail),
            "filter": lambda: c.filter_cross_gather_dev(fwd.data_ptr(), n, 2, rev.data_ptr(), n, 2, *tail[:4], *tail[6:]),
        }

        def result(name):
            calls[name]()
            torch.cuda.synchronize()
            m = int(cnt[0])
            return m, good.cpu().numpy()[:m].tobytes(), xy2.cpu().numpy()[:m].tobytes()

        base = {name: result(name) for name in ("f32", "u8", "hamming")}
        assert all(b[0] > 30 for b in base.values()) and base["f32"] == base["u8"]
        for name in calls:
            gc.collect()                 # no finaliser of an earlier test's context (hipFree) inside the capture
            g = torch.cuda.CUDAGraph()
            with pytest.raises(pm.PmError) as err:
                with torch.cuda.graph(g, stream=st, capture_error_mode="relaxed"):
                    calls[name]()
            assert err.value.status == api.PM_E_UNSUPPORTED and "capturing" in str(err.value), name
            del g
            torch.cuda.set_stream(st)
        for name in ("hamming", "u8", "f32"):                    # the context still works
            assert result(name) == base[name]
        assert result("filter") == base["f32"]                  # fwd / rev hold the f32 call's records
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)
        c.close()


# ---- the CLI switch ---------------------------------------------------------------------------------------------------------

def _write(tmp_path, w):
    paths = {}
    for name in ("q", "t", "kp1", "kp2"):
        paths[name] = str(tmp_path / (name + ".pmm"))
        io.save_pmm(paths[name], w[name])
    return ["--desc1", paths["q"], "--desc2", paths["t"], "--kp1", paths["kp1"], "--kp2", paths["kp2"]]


@pytest.mark.parametrize("kind", ["surf", "orb"])
def test_cli_cross_filters(tmp_path, oracle, kind):
    exe = build.HOST_BIN
    assert os.path.exists(exe), "run python -m points_matching_amd.build"
    binary = kind == "orb"
    w = synth.pair_workload(nq=300, nt=280, dim=32 if binary else 128, seed=77, planted=0.5, kind=kind)
    files = _write(tmp_path, w)
    fwd2, rev2 = _oracle_both_ways(oracle, "cli_" + kind, w["q"], w["t"], binary)
    for mode, flags, ratio in (("cross", 0, 0.8), ("cross-ratio", FWD, 0.8), ("cross-ratio", FWD, 0.6)):
        cmd = [exe] + files + ["--filter", mode, "--ratio", str(ratio), "--method", "ransac8", "--iters", "300", "--seed", "99"]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        want = cross_ref(fwd2, rev2, flags, ratio)
        assert 8 < want.size < 300
        exp = api.format_match_list(want).splitlines()
        lines = out.stdout.splitlines()
        assert lines[:len(exp)] == exp
        assert lines[len(exp)].startswith("result = 0 ") and sum(ln.startswith("result = ") for ln in lines) == want.size


def test_cli_cross_usage_errors(tmp_path):
    exe = build.HOST_BIN
    w = synth.pair_workload(nq=64, nt=64, dim=128, seed=3, planted=0.5, kind="surf")
    files = _write(tmp_path, w)
    for extra in (["--matcher", "flann", "--filter", "cross"], ["--matcher", "flann", "--filter", "cross-ratio"],
                  ["--filter", "cross", "--gpus", "2", "--method", "ransac8"], ["--filter", "cross", "--mgpu", "--method", "ransac8"],
                  ["--filter", "crosscheck"]):
        out = subprocess.run([exe] + files + extra, capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "pm_cli:" in out.stderr and out.stdout == "", extra
