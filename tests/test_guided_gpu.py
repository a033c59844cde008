"""GPU: guided matching (docs/SPEC.md S48-S50) against the plain-C restatement tests/guided_ref.c, bit for bit: records
and admitted counts over the shape grid, batch boundaries, ties, the all-admitting gate against the existing matchers,
agreement with the RANSAC masks, chaining behind the device estimators, the one-call forms and the argument errors."""
import os

import numpy as np
import pytest

import points_matching_amd as pm
from points_matching_amd import api
import guided_cases as GC
import guided_ref as GR
from util import assert_matches_equal

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HOST = {GR.DESC_F32: "bf_knn_guided_l2", GR.DESC_U8: "bf_knn_guided_l2_u8", GR.DESC_BINARY: "bf_knn_guided_hamming"}
KNN_DEV = {GR.DESC_F32: "bf_knn_guided_l2_dev", GR.DESC_U8: "bf_knn_guided_l2_u8_dev", GR.DESC_BINARY: "bf_knn_guided_hamming_dev"}
MATCH_DEV = {GR.DESC_F32: "bf_match_guided_l2_dev", GR.DESC_U8: "bf_match_guided_l2_u8_dev",
             GR.DESC_BINARY: "bf_match_guided_hamming_dev"}


def _guided(ctx, desc, *args):
    return getattr(ctx, HOST[desc])(*args)


def _check(ctx, desc, q, t, kp1, kp2, kind, M, tau, k, what):
    got, adm = _guided(ctx, desc, q, t, kp1, kp2, kind, M, tau, k)
    want, wadm = GR.knn(desc, q, t, kp1, kp2, kind, M, tau, k)
    assert np.array_equal(adm, wadm), (what, adm[:8], wadm[:8])
    assert_matches_equal(got, want, what)
    return want, wadm


def _records(t):
    return t.cpu().numpy().view(pm.MATCH_DTYPE).reshape(t.shape[0], -1)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


# ---- the shape grid ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", GC.KINDS)
@pytest.mark.parametrize("name", sorted(GC.DESCS))
def test_grid_equals_reference(ctx, name, kind):
    desc, width = GC.DESCS[name]
    short = full = 0
    for nq, nt, kp1, kp2, M, tau in GC.grid_cases(kind):
        q, t = GC.descriptors(desc, width, nq, nt, seed=1)
        for k in GC.KS:
            _, adm = _check(ctx, desc, q, t, kp1, kp2, kind, M, tau, k, "%s kind %d %dx%d tau %g k %d" % (name, kind, nq, nt, tau, k))
            short += int((adm < k).sum())
            full += int((adm >= k).sum())
    assert short > 0 and full > 0


def test_wide_u8_rows_take_the_float_sum(ctx):
    """u8 rows beyond 256 columns: partial sums pass 2^24, the S1 order decides the bits (dim 300: with a tail)."""
    kp1, kp2, F = GC.geometry(GR.F_SAMPSON, 17, 200)
    for width in (300, 512):
        rng = np.random.default_rng(width)
        q = rng.integers(200, 256, (17, width), dtype=np.uint8)
        t = rng.integers(0, 56, (200, width), dtype=np.uint8)
        _check(ctx, GR.DESC_U8, q, t, kp1, kp2, GR.F_SAMPSON, F, 30.0, 4, "u8 dim %d" % width)


@pytest.mark.parametrize("name", ["f32_20", "u8_32", "ham_8"])
def test_unaligned_rows_and_odd_widths(ctx, name):
    """Device buffers offset by one row element (float rows) or by 4 bytes, and u8 rows whose width is no multiple of 4."""
    import torch
    desc, width = GC.DESCS[name]
    widths = (width, 21) if desc == GR.DESC_U8 else (width,)
    kp1, kp2, M = GC.geometry(GR.F_SYM, 17, 65)
    d_kp1, d_kp2, d_M = _dev(kp1), _dev(kp2), _dev(M.reshape(9))
    for w in widths:
        q, t = GC.descriptors(desc, w, 17, 65, seed=8)
        pad = 1 if desc == GR.DESC_F32 else 4
        d_q = _dev(np.concatenate([np.zeros(pad, q.dtype), q.reshape(-1)]))
        d_t = _dev(np.concatenate([np.zeros(pad, t.dtype), t.reshape(-1)]))
        d_out = torch.zeros((17, 4 * 4), dtype=torch.int32, device=d_q.device)
        d_adm = torch.zeros(17, dtype=torch.int32, device=d_q.device)
        torch.cuda.synchronize()
        item = q.dtype.itemsize
        getattr(ctx, KNN_DEV[desc])(d_q.data_ptr() + pad * item, 17, d_t.data_ptr() + pad * item, 65, w, d_kp1.data_ptr(),
                                    d_kp2.data_ptr(), GR.F_SYM, d_M.data_ptr(), 30.0, 4, d_out.data_ptr(), d_adm.data_ptr())
        ctx.synchronize()
        want, wadm = GR.knn(desc, q, t, kp1, kp2, GR.F_SYM, M, 30.0, 4)
        assert np.array_equal(d_adm.cpu().numpy(), wadm)
        assert_matches_equal(_records(d_out), want, "%s width %d, offset rows" % (name, w))


# ---- batch boundaries and ties -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["f32_20", "u8_32", "ham_8"])
def test_every_admitted_count_up_to_130_and_a_full_sweep(ctx, name):
    desc, width = GC.DESCS[name]
    kp1, kp2, H, tau, counts = GC.batch_scene()
    nt = kp2.shape[0]
    q, t = GC.descriptors(desc, width, 131, nt, seed=3)
    for k in GC.KS:
        _, adm = _check(ctx, desc, q, t, kp1, kp2, GR.H, H, tau, k, "%s batch scene k %d" % (name, k))
        assert np.array_equal(adm, counts)
    # the same scene under a gate that admits every row (tau = 1e5 px): nt = 8515 >= 1000 admitted rows per query
    _, adm = _check(ctx, desc, q[:3], t, kp1[:3], kp2, GR.H, H, 1e5, 4, name + " full sweep")
    assert (adm == nt).all() and nt >= 1000


@pytest.mark.parametrize("name", sorted(GC.DESCS))
def test_ties_go_to_the_lower_train_index(ctx, name):
    desc, width = GC.DESCS[name]
    q, t, kp1, kp2, H, tau, copies = GC.tie_scene(desc, width)
    for k in GC.KS:
        want, _ = _check(ctx, desc, q, t, kp1, kp2, GR.H, H, tau, k, "%s ties k %d" % (name, k))
        got, _ = _guided(ctx, desc, q, t, kp1, kp2, GR.H, H, tau, k)
        assert got["trainIdx"].tolist() == [copies[:k], copies[:k]]
        assert (got["distance"] == got["distance"][:, :1]).all()


# ---- second, independent check through the existing matchers --------------------------------------------------------

@pytest.mark.parametrize("name", sorted(GC.DESCS))
def test_all_admitting_gate_equals_the_plain_matchers(ctx, name):
    desc, width = GC.DESCS[name]
    nq, nt = 67, 200
    q, t = GC.descriptors(desc, width, nq, nt, seed=4)
    kp1, kp2, F = GC.geometry(GR.F_SAMPSON, nq, nt)
    for k in GC.KS:
        got, adm = _guided(ctx, desc, q, t, kp1, kp2, GR.F_SAMPSON, F, 1e6, k)
        assert (adm == nt).all()
        if desc == GR.DESC_F32:
            want = ctx.bf_knn_l2(q, t, k, api.PM_KNN_FORCE_EXACT)
        elif desc == GR.DESC_U8:
            want = ctx.bf_knn_l2_u8(q, t, k)
        else:
            want = ctx.bf_knn_hamming(q, t, k)
        assert_matches_equal(got, want, "%s k %d" % (name, k))


# ---- agreement with RANSAC --------------------------------------------------------------------------------------------

def _identity_descriptors(n, seed=6):
    """Pairwise distinct rows with q[i] == t[i]."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 32)).astype(np.float32)
    d[:, 0] = np.arange(n)
    return d, d.copy()


@pytest.mark.parametrize("model", ["F_sampson", "F_sym", "H"])
def test_gate_agrees_with_the_ransac_mask(ctx, model):
    g = np.load(os.path.join(GOLD, "twoview_N512_outliers.npz"), allow_pickle=False)
    xy1, xy2 = g["xy1"], g["xy2"]
    if model == "H":
        rc, M, mask, n, _ = ctx.ransac_homography(xy1, xy2, 500, 3.0, 42)
        kind = GR.H
    else:
        err = api.PM_ERR_SAMPSON if model == "F_sampson" else api.PM_ERR_SYM_EPIPOLAR
        rc, M, mask, n, _ = ctx.ransac_fundamental(xy1, xy2, 500, 3.0, 42, err)
        kind = GR.F_SAMPSON if model == "F_sampson" else GR.F_SYM
    assert rc == api.PM_OK and 4 <= n < 512
    q, t = _identity_descriptors(512)
    out, adm = ctx.bf_knn_guided_l2(q, t, xy1, xy2, kind, M, 3.0, 1)
    hit = (out["trainIdx"][:, 0] == np.arange(512)) & (out["distance"][:, 0] == 0)
    assert np.array_equal(hit, mask.astype(bool))
    assert (adm >= mask).all()


# ---- chaining behind the device estimators ---------------------------------------------------------------------------

def test_model_pointer_straight_from_the_device_estimators(ctx):
    import torch
    dev = torch.device("cuda", 0)
    g = np.load(os.path.join(GOLD, "twoview_N512_outliers.npz"), allow_pickle=False)
    xy1, xy2 = g["xy1"], g["xy2"]
    n = 512
    q, t = GC.descriptors(GR.DESC_F32, 64, n, n, seed=12)
    d_q, d_t, d_xy1, d_xy2 = _dev(q), _dev(t), _dev(xy1), _dev(xy2)
    d_key = torch.zeros(1, dtype=torch.int64, device=dev)
    d_M = torch.zeros(9, dtype=torch.float64, device=dev)
    d_Mr = torch.zeros(9, dtype=torch.float64, device=dev)
    d_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    d_out = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    d_adm = torch.zeros(n, dtype=torch.int32, device=dev)
    d_n = torch.tensor([n], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    # RANSAC-F, then guided 2-NN with its d_F, nothing in between
    ctx.ransac_run_dev(d_xy1.data_ptr(), d_xy2.data_ptr(), n, 0, 0, 500, 3.0, 42, d_key.data_ptr(), d_M.data_ptr(),
                       d_mask.data_ptr(), d_cnt.data_ptr())
    ctx.bf_knn_guided_l2_dev(d_q.data_ptr(), n, d_t.data_ptr(), n, 64, d_xy1.data_ptr(), d_xy2.data_ptr(), GR.F_SAMPSON,
                             d_M.data_ptr(), 3.0, 2, d_out.data_ptr(), d_adm.data_ptr())
    ctx.synchronize()
    F = d_M.cpu().numpy()
    assert int(d_cnt.item()) >= 8 and np.abs(F).max() > 0
    want, wadm = ctx.bf_knn_guided_l2(q, t, xy1, xy2, GR.F_SAMPSON, F, 3.0, 2)
    assert_matches_equal(_records(d_out), want, "d_F from pm_ransac_run_dev")
    assert np.array_equal(d_adm.cpu().numpy(), wadm) and wadm.max() >= 2
    ref, radm = GR.knn(GR.DESC_F32, q, t, xy1, xy2, GR.F_SAMPSON, F, 3.0, 2)
    assert_matches_equal(want, ref, "host-model call")
    assert np.array_equal(wadm, radm)
    # RANSAC-H, refinement, guided 2-NN with the refined d_H
    view = api.PointsView(d_xy1.data_ptr(), d_xy2.data_ptr(), d_n.data_ptr(), 1, n, 0, 1, 0)
    ctx.ransac_homography_run_dev(view, 0, 500, 3.0, 42, d_key.data_ptr(), d_M.data_ptr(), d_mask.data_ptr(), n, d_cnt.data_ptr())
    ctx.homography_refine_dev(view, d_mask.data_ptr(), d_M.data_ptr(), 10, d_Mr.data_ptr(), None)
    ctx.bf_knn_guided_l2_dev(d_q.data_ptr(), n, d_t.data_ptr(), n, 64, d_xy1.data_ptr(), d_xy2.data_ptr(), GR.H,
                             d_Mr.data_ptr(), 3.0, 2, d_out.data_ptr(), d_adm.data_ptr())
    ctx.synchronize()
    H = d_Mr.cpu().numpy()
    assert np.abs(H).max() > 0
    want, wadm = ctx.bf_knn_guided_l2(q, t, xy1, xy2, GR.H, H, 3.0, 2)
    assert_matches_equal(_records(d_out), want, "d_H from pm_homography_refine_dev")
    assert np.array_equal(d_adm.cpu().numpy(), wadm)


def test_no_model_admits_nothing(ctx):
    """RANSAC on a device count below 8 leaves F = 0: every row is -1, n_admitted = 0 and n_good = 0."""
    import torch
    dev = torch.device("cuda", 0)
    nq, nt = 67, 200
    q, t = GC.descriptors(GR.DESC_F32, 64, nq, nt, seed=13)
    kp1, kp2, _ = GC.geometry(GR.F_SAMPSON, nq, nt)
    d_q, d_t, d_kp1, d_kp2 = _dev(q), _dev(t), _dev(kp1), _dev(kp2)
    d_key = torch.zeros(1, dtype=torch.int64, device=dev)
    d_F = torch.full((9,), 5.0, dtype=torch.float64, device=dev)
    d_mask = torch.zeros(nq, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    d_knn = torch.zeros((nq, 8), dtype=torch.int32, device=dev)
    d_adm = torch.full((nq,), 9, dtype=torch.int32, device=dev)
    d_good = torch.zeros((nq, 4), dtype=torch.int32, device=dev)
    d_xy1 = torch.zeros((nq, 2), dtype=torch.float32, device=dev)
    d_xy2 = torch.zeros((nq, 2), dtype=torch.float32, device=dev)
    d_ng = torch.full((1,), 7, dtype=torch.int32, device=dev)
    d_seven = torch.tensor([7], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.ransac_run_dev(d_kp1.data_ptr(), d_kp2.data_ptr(), nq, d_seven.data_ptr(), 0, 100, 3.0, 42, d_key.data_ptr(),
                       d_F.data_ptr(), d_mask.data_ptr(), d_cnt.data_ptr())
    ctx.synchronize()
    assert (d_F.cpu().numpy() == 0).all(), "the estimator leaves F = 0 when it finds no model"
    ctx.bf_knn_guided_l2_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, 64, d_kp1.data_ptr(), d_kp2.data_ptr(), GR.F_SAMPSON,
                             d_F.data_ptr(), 3.0, 2, d_knn.data_ptr(), d_adm.data_ptr())
    ctx.synchronize()
    rec = _records(d_knn)
    assert (rec["trainIdx"] == -1).all() and np.isinf(rec["distance"]).all() and (rec["queryIdx"] == np.arange(nq)[:, None]).all()
    assert (d_adm.cpu().numpy() == 0).all()
    ctx.bf_match_guided_l2_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, 64, d_kp1.data_ptr(), d_kp2.data_ptr(), GR.F_SAMPSON,
                               d_F.data_ptr(), 3.0, 0.8, d_knn.data_ptr(), d_good.data_ptr(), d_xy1.data_ptr(), d_xy2.data_ptr(),
                               d_ng.data_ptr())
    ctx.synchronize()
    assert int(d_ng.item()) == 0
    # non-finite models and models that round to nine zeros, through the host form
    for M in (np.full(9, np.nan), np.full(9, 1e-60), np.array([1, 0, 0, 0, np.inf, 0, 0, 0, 1.0]), np.full(9, 1e300)):
        for kind in GC.KINDS:
            rec, adm = ctx.bf_knn_guided_l2(q, t, kp1, kp2, kind, M, 3.0, 2)
            assert (rec["trainIdx"] == -1).all() and (adm == 0).all()


# ---- the one-call forms ---------------------------------------------------------------------------------------------------

def _one_call_buffers(nq):
    import torch
    dev = torch.device("cuda", 0)
    return {"knn": torch.zeros((nq, 8), dtype=torch.int32, device=dev), "good": torch.zeros((nq, 4), dtype=torch.int32, device=dev),
            "xy1": torch.zeros((nq, 2), dtype=torch.float32, device=dev), "xy2": torch.zeros((nq, 2), dtype=torch.float32, device=dev),
            "n": torch.full((1,), -1, dtype=torch.int32, device=dev)}


@pytest.mark.parametrize("name", ["f32_64", "u8_128", "ham_32"])
def test_one_call_equals_guided_2nn_plus_ratio_filter(ctx, name):
    import torch
    desc, width = GC.DESCS[name]
    nq, nt = 300, 700
    q, t = GC.descriptors(desc, width, nq, nt, seed=14)
    kp1, kp2, F = GC.geometry(GR.F_SAMPSON, nq, nt)
    d_q, d_t, d_kp1, d_kp2, d_M = _dev(q), _dev(t), _dev(kp1), _dev(kp2), _dev(F.reshape(9))
    a, b = _one_call_buffers(nq), _one_call_buffers(nq)
    torch.cuda.synchronize()
    for tau, ratio in ((30.0, 0.95), (3.0, 1.0)):
        getattr(ctx, MATCH_DEV[desc])(d_q.data_ptr(), nq, d_t.data_ptr(), nt, width, d_kp1.data_ptr(), d_kp2.data_ptr(),
                                      GR.F_SAMPSON, d_M.data_ptr(), tau, ratio, a["knn"].data_ptr(), a["good"].data_ptr(),
                                      a["xy1"].data_ptr(), a["xy2"].data_ptr(), a["n"].data_ptr())
        getattr(ctx, KNN_DEV[desc])(d_q.data_ptr(), nq, d_t.data_ptr(), nt, width, d_kp1.data_ptr(), d_kp2.data_ptr(),
                                    GR.F_SAMPSON, d_M.data_ptr(), tau, 2, b["knn"].data_ptr(), 0)
        ctx.filter_ratio_gather_dev(b["knn"].data_ptr(), nq, 2, ratio, d_kp1.data_ptr(), d_kp2.data_ptr(), b["good"].data_ptr(),
                                    b["xy1"].data_ptr(), b["xy2"].data_ptr(), b["n"].data_ptr())
        ctx.synchronize()
        n = int(a["n"].item())
        assert n == int(b["n"].item()) and 0 < n < nq
        assert torch.equal(a["knn"], b["knn"]) and torch.equal(a["good"][:n], b["good"][:n])
        assert torch.equal(a["xy1"][:n], b["xy1"][:n]) and torch.equal(a["xy2"][:n], b["xy2"][:n])
        rec, good, xy1, xy2 = GR.match_guided(desc, q, t, kp1, kp2, GR.F_SAMPSON, F, tau, ratio)
        assert good.size == n
        assert_matches_equal(_records(a["knn"]), rec, name + " 2-NN records")
        assert_matches_equal(_records(a["good"])[:n, 0], good, name + " survivors")
        assert np.array_equal(a["xy1"].cpu().numpy()[:n], xy1) and np.array_equal(a["xy2"].cpu().numpy()[:n], xy2)
    # match list only: no point outputs
    getattr(ctx, MATCH_DEV[desc])(d_q.data_ptr(), nq, d_t.data_ptr(), nt, width, d_kp1.data_ptr(), d_kp2.data_ptr(),
                                  GR.F_SAMPSON, d_M.data_ptr(), 3.0, 1.0, a["knn"].data_ptr(), b["good"].data_ptr(), 0, 0,
                                  b["n"].data_ptr())
    ctx.synchronize()
    assert int(b["n"].item()) == n and torch.equal(a["good"][:n], b["good"][:n])


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_capture_refused_by_the_one_call_forms_and_allowed_for_the_plain_knn():
    import gc
    import torch
    dev = torch.device("cuda", 0)
    nq, nt = 67, 200
    st = torch.cuda.Stream(device=dev)
    prev = torch.cuda.current_stream(dev)
    torch.cuda.set_stream(st)
    c = pm.Context(0)
    c.set_stream(st.cuda_stream)
    try:
        kp1, kp2, F = GC.geometry(GR.F_SAMPSON, nq, nt)
        d_kp1, d_kp2, d_M = _dev(kp1), _dev(kp2), _dev(F.reshape(9))
        data = {desc: [_dev(x) for x in GC.descriptors(desc, width, nq, nt, seed=15)]
                for desc, width in ((GR.DESC_F32, 64), (GR.DESC_U8, 128), (GR.DESC_BINARY, 32))}
        widths = {GR.DESC_F32: 64, GR.DESC_U8: 128, GR.DESC_BINARY: 32}
        b = _one_call_buffers(nq)
        out = torch.zeros((nq, 8), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def one_call(desc):
            getattr(c, MATCH_DEV[desc])(data[desc][0].data_ptr(), nq, data[desc][1].data_ptr(), nt, widths[desc], d_kp1.data_ptr(),
                                        d_kp2.data_ptr(), GR.F_SAMPSON, d_M.data_ptr(), 30.0, 0.95, b["knn"].data_ptr(),
                                        b["good"].data_ptr(), b["xy1"].data_ptr(), b["xy2"].data_ptr(), b["n"].data_ptr())

        def plain(desc):
            getattr(c, KNN_DEV[desc])(data[desc][0].data_ptr(), nq, data[desc][1].data_ptr(), nt, widths[desc], d_kp1.data_ptr(),
                                      d_kp2.data_ptr(), GR.F_SAMPSON, d_M.data_ptr(), 30.0, 2, out.data_ptr(), 0)

        for desc in data:
            one_call(desc)
            torch.cuda.synchronize()
            before = (int(b["n"].item()), b["knn"].clone(), b["good"].clone())
            b["n"].fill_(-5)
            b["knn"].fill_(0)
            torch.cuda.synchronize()
            gc.collect()                 # no finaliser of an earlier test's context (hipFree) inside the capture
            g = torch.cuda.CUDAGraph()
            with pytest.raises(pm.PmError) as err:
                with torch.cuda.graph(g, stream=st, capture_error_mode="relaxed"):
                    one_call(desc)
            assert err.value.status == api.PM_E_UNSUPPORTED and "capturing" in str(err.value)
            del g
            torch.cuda.set_stream(st)
            torch.cuda.synchronize()
            assert int(b["n"].item()) == -5 and int(b["knn"].abs().sum().item()) == 0      # nothing was enqueued
            one_call(desc)                                                                  # the context still works
            torch.cuda.synchronize()
            assert int(b["n"].item()) == before[0] and torch.equal(b["knn"], before[1])
            # the plain guided k-NN carries no epoch: captured once, replayed twice, same records
            gc.collect()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st, capture_error_mode="relaxed"):
                plain(desc)
            torch.cuda.set_stream(st)
            for _ in range(2):
                out.fill_(0)
                g.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, before[1])
            del g
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)
        c.close()


def test_one_call_refuses_more_than_1048576_queries(ctx):
    import torch
    dev = torch.device("cuda", 0)
    buf = torch.zeros(64, dtype=torch.float64, device=dev)
    d_n = torch.full((1,), 3, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    p = buf.data_ptr()
    for name in MATCH_DEV.values():
        with pytest.raises(pm.PmError) as e:                 # refused before any pointer is read
            getattr(ctx, name)(p, (1 << 20) + 1, p, 8, 4, p, p, GR.F_SAMPSON, p, 3.0, 0.8, p, p, p, p, d_n.data_ptr())
        assert e.value.status == api.PM_E_UNSUPPORTED
    ctx.synchronize()
    assert int(d_n.item()) == 3


# ---- what it is for ---------------------------------------------------------------------------------------------------------

def test_guided_matching_keeps_more_correct_matches_on_repeated_texture(ctx):
    import torch
    s = GC.texture_scene()
    nq, nt, dim = s["q"].shape[0], s["t"].shape[0], s["q"].shape[1]
    d_q, d_t, d_kp1, d_kp2, d_F = _dev(s["q"]), _dev(s["t"]), _dev(s["kp1"]), _dev(s["kp2"]), _dev(s["F"].reshape(9))
    a, b = _one_call_buffers(nq), _one_call_buffers(nq)
    torch.cuda.synchronize()
    ctx.bf_knn_l2_ratio_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, dim, 0, 0.8, d_kp1.data_ptr(), d_kp2.data_ptr(),
                            a["knn"].data_ptr(), a["good"].data_ptr(), a["xy1"].data_ptr(), a["xy2"].data_ptr(), a["n"].data_ptr())
    ctx.bf_match_guided_l2_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, dim, d_kp1.data_ptr(), d_kp2.data_ptr(), GR.F_SAMPSON,
                               d_F.data_ptr(), 3.0, 0.8, b["knn"].data_ptr(), b["good"].data_ptr(), b["xy1"].data_ptr(),
                               b["xy2"].data_ptr(), b["n"].data_ptr())
    ctx.synchronize()
    plain = _records(a["good"])[:int(a["n"].item()), 0]
    good = _records(b["good"])[:int(b["n"].item()), 0]
    ok_plain = int((plain["trainIdx"] == s["truth"][plain["queryIdx"]]).sum())
    ok_guided = int((good["trainIdx"] == s["truth"][good["queryIdx"]]).sum())
    print("texture scene: plain ratio test keeps %d (%d correct), guided keeps %d (%d correct)"
          % (plain.size, ok_plain, good.size, ok_guided))
    assert ok_guided > ok_plain
    xy1, xy2 = b["xy1"].cpu().numpy()[:good.size], b["xy2"].cpu().numpy()[:good.size]
    assert np.array_equal(xy1, s["kp1"][good["queryIdx"]]) and np.array_equal(xy2, s["kp2"][good["trainIdx"]])
    assert GR.gate_pairs(GR.F_SAMPSON, s["F"], 3.0, xy1, xy2).all()           # every survivor passes the gate
    _, ref_good, _, _ = GR.match_guided(GR.DESC_F32, s["q"], s["t"], s["kp1"], s["kp2"], GR.F_SAMPSON, s["F"], 3.0, 0.8)
    assert_matches_equal(good, ref_good, "texture scene survivors")


# ---- argument errors and empty sets ----------------------------------------------------------------------------------

def test_argument_errors_and_empty_sets(ctx):
    import torch
    dev = torch.device("cuda", 0)
    buf = torch.zeros(4096, dtype=torch.float64, device=dev)
    out = torch.full((8, 8), 7, dtype=torch.int32, device=dev)
    adm = torch.full((8,), 7, dtype=torch.int32, device=dev)
    d_n = torch.full((1,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    p, o = buf.data_ptr(), out.data_ptr()
    good = dict(dq=p, nq=8, dt=p, nt=8, width=8, kp1=p, kp2=p, kind=GR.F_SAMPSON, M=p, tau=3.0, k=2, out=o, adm=adm.data_ptr())
    bad = [dict(k=0), dict(k=5), dict(kind=3), dict(kind=-1), dict(width=0), dict(M=0), dict(dq=0), dict(dt=0), dict(kp1=0),
           dict(kp2=0), dict(out=0), dict(nq=-1), dict(nt=-1)]
    for name in KNN_DEV.values():
        for change in bad:
            a = dict(good, **change)
            with pytest.raises(pm.PmError) as e:
                getattr(ctx, name)(a["dq"], a["nq"], a["dt"], a["nt"], a["width"], a["kp1"], a["kp2"], a["kind"], a["M"], a["tau"],
                                   a["k"], a["out"], a["adm"])
            assert e.value.status == api.PM_E_INVALID, (name, change)
    for width in (6, 33):                                                   # bytes % 4 != 0
        with pytest.raises(pm.PmError) as e:
            ctx.bf_knn_guided_hamming_dev(p, 8, p, 8, width, p, p, GR.H, p, 3.0, 1, o, 0)
        assert e.value.status == api.PM_E_INVALID
    for name in MATCH_DEV.values():
        for args in ((p, 8, p, 8, 8, p, p, GR.H, p, 3.0, 0.8, 0, p, p, p, d_n.data_ptr()),       # no record buffer
                     (p, 8, p, 8, 8, p, p, GR.H, p, 3.0, 0.8, o, p, p, p, 0),                    # no count
                     (p, 8, p, 8, 8, p, p, GR.H, p, 3.0, 0.8, o, p, p, 0, d_n.data_ptr()),       # one point output only
                     (p, 8, p, 8, 8, p, p, 7, p, 3.0, 0.8, o, p, p, p, d_n.data_ptr())):         # unknown kind
            with pytest.raises(pm.PmError) as e:
                getattr(ctx, name)(*args)
            assert e.value.status == api.PM_E_INVALID, name
    ctx.synchronize()
    assert int(d_n.item()) == 7 and (out.cpu().numpy() == 7).all()
    # nq == 0: PM_OK, nothing written; the one-call form reports no survivor
    ctx.bf_knn_guided_l2_dev(0, 0, p, 8, 8, 0, p, GR.H, p, 3.0, 2, 0, 0)
    ctx.bf_match_guided_l2_dev(0, 0, p, 8, 8, 0, p, GR.H, p, 3.0, 0.8, 0, 0, 0, 0, d_n.data_ptr())
    ctx.synchronize()
    assert int(d_n.item()) == 0 and (out.cpu().numpy() == 7).all() and (adm.cpu().numpy() == 7).all()
    # nt == 0: every row is -1 / +inf, nothing admitted (null train pointers are fine)
    M = _dev(np.eye(3).reshape(9))
    for name in KNN_DEV.values():
        out.fill_(7)
        adm.fill_(7)
        torch.cuda.synchronize()
        getattr(ctx, name)(p, 8, 0, 0, 8, p, 0, GR.H, M.data_ptr(), 3.0, 2, o, adm.data_ptr())
        ctx.synchronize()
        rec = _records(out)
        assert (rec["trainIdx"] == -1).all() and np.isinf(rec["distance"]).all() and (rec["imgIdx"] == 0).all()
        assert (rec["queryIdx"] == np.arange(8)[:, None]).all() and (adm.cpu().numpy() == 0).all()
    rec, a0 = ctx.bf_knn_guided_l2(np.zeros((3, 8), np.float32), np.zeros((0, 8), np.float32), np.zeros((3, 2)), np.zeros((0, 2)),
                                   GR.H, np.eye(3), 3.0, 4)
    assert rec.shape == (3, 4) and (rec["trainIdx"] == -1).all() and (a0 == 0).all()
