"""GPU: the device feature front end (pm_detect_describe[_dev], SPEC S53-S57) against the host extractor it ports
(host/pm_features.cpp, run through `pm_cli --features host --extract-only --save-features`).

Keypoints, their order and the Gaussian levels must equal the host's bit for bit.  Descriptors may differ only where the
device's atan2f / fp64 exp differ from glibc's in the last bit: at most 2 % of rows (at least one allowed) may differ at
all, at most 0.5 % (at least one allowed) by more than 1 in any element.  Measured shares: profiles/features_parity.txt."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

from features_ref import bits, blobs, candidate_responses, check_descriptors, gaussian_np, image
from points_matching_amd import api, build, io

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


_HOST = {}
MAX_KP = 512        # above the candidate count of every input here (at most 315), so nothing is cut unless a test asks for it


@pytest.fixture(scope="module")
def ctx():
    """A context of this module's own: its feature buffer, its capacity option and the buffers of the calls below are
    released when the module is done, and the suite's shared context stays as the other modules expect it."""
    import gc
    import torch
    import points_matching_amd as pm
    c = pm.Context(0)
    yield c
    torch.cuda.synchronize()
    c.close()
    gc.collect()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """host(name, max_kp) -> (kp (n, 2) f32, desc (n, 128) f32) of the host extractor; computed once per key."""
    build.build_host()
    d = tmp_path_factory.mktemp("hostfeat")

    def run(name, max_kp=MAX_KP):
        key = (name, max_kp)
        if key not in _HOST:
            img = image(name)
            pgm = str(d / ("%s.pgm" % name))
            with open(pgm, "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
            pre = str(d / ("%s_%d" % (name, max_kp)))
            out = subprocess.run([build.HOST_BIN, "--features", "host", "--img1", pgm, "--img2", pgm, "--extract-only", "--save-features",
                                  pre, "--quiet", "--max-kp", str(max_kp)], capture_output=True, text=True, timeout=300)
            assert out.returncode == 0, out.stderr
            _HOST[key] = (io.load_pmm(pre + "_kp1.pmm").reshape(-1, 2), io.load_pmm(pre + "_desc1.pmm").reshape(-1, 128))
        return _HOST[key]
    return run


def dev_extract(ctx, img, max_kp=MAX_KP):
    """pm_detect_describe_dev on torch buffers -> (n, kp, u8, f32, meta) with n rows each (n = -1: none)."""
    import torch
    dev = torch.device("cuda", 0)
    h, w = img.shape
    d_img = torch.from_numpy(img).to(dev)
    d_kp = torch.full((max_kp, 2), -7.0, dtype=torch.float32, device=dev)
    d_u8 = torch.full((max_kp, 128), 77, dtype=torch.uint8, device=dev)
    d_f = torch.full((max_kp, 128), -7.0, dtype=torch.float32, device=dev)
    d_meta = torch.full((max_kp, 4), -7.0, dtype=torch.float32, device=dev)
    d_n = torch.full((1,), 12345, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.detect_describe_dev(d_img.data_ptr(), w, h, w, max_kp, d_kp.data_ptr(), d_u8.data_ptr(), d_f.data_ptr(), d_meta.data_ptr(),
                            d_n.data_ptr())
    ctx.synchronize()
    n = int(d_n.item())
    m = max(n, 0)
    res = (n, d_kp[:m].cpu().numpy(), d_u8[:m].cpu().numpy(), d_f[:m].cpu().numpy(), d_meta[:m].cpu().numpy())
    if n >= 0:      # nothing is written behind the count
        assert (d_kp[m:] == -7.0).all() and (d_u8[m:] == 77).all() and (d_f[m:] == -7.0).all() and (d_meta[m:] == -7.0).all()
    return res


@pytest.mark.parametrize("name", ["97x131", "129x128", "160x65", "golden1", "golden2", "tiled"])
def test_keypoints_bit_equal_and_descriptors_within_caps(ctx, host, name):
    kp_h, desc_h = host(name)
    assert kp_h.shape[0] >= 5
    n, kp, u8, f32, meta = dev_extract(ctx, image(name))
    assert n == kp_h.shape[0]
    assert (bits(kp) == bits(kp_h)).all()
    assert (u8.astype(np.float32) == f32).all()
    check_descriptors(name, f32, desc_h)
    # meta: responses descending (the selection order), octave consistent with the coordinate scale
    assert (np.diff(meta[:, 2]) <= 0).all() and (meta[:, 2] > 0.01).all()
    scale = np.exp2(meta[:, 3])
    assert (kp == np.rint(kp / scale[:, None]) * scale[:, None]).all()
    assert (meta[:, 0] > 1.6 * scale).all() and (np.abs(meta[:, 1]) < math.pi).all()
    # the blocking form gives the same rows
    kp_b, u8_b, f32_b, meta_b = ctx.detect_describe(image(name), MAX_KP)
    assert (bits(kp_b) == bits(kp)).all() and (u8_b == u8).all() and (bits(f32_b) == bits(f32)).all() and (bits(meta_b) == bits(meta)).all()


def test_small_image_gives_no_keypoints(ctx):
    img = blobs(31, 40, 11, 20)
    n, kp, u8, f32, meta = dev_extract(ctx, img, 64)
    assert n == 0
    kp_b, u8_b, f32_b, meta_b = ctx.detect_describe(img, 64)
    assert kp_b.shape == (0, 2) and u8_b.shape == (0, 128)


def test_cap_inside_a_tie(ctx, host):
    """max_kp = 20 on the tiled image: candidates 19 and 20 of the selection order have bit-equal responses (translated
    copies), so the cut falls inside a tie and the scan-order rule decides.  d_meta holds the rows that survive the border
    skips, not every candidate, so the candidate responses come from the numpy restatement of the scan on the device's
    own Gaussian levels; d_meta of the uncapped run must be a subsequence of them."""
    img = image("tiled")
    n_all, kp_all, _, _, meta_all = dev_extract(ctx, img)
    resp = candidate_responses(ctx, 3)
    assert resp.size == 142 and n_all == 83
    assert resp[19] == resp[20]
    assert (np.diff(resp) == 0).sum() >= 100                     # nearly every adjacent pair is an exact tie
    it = iter(resp.tolist())
    assert all(any(v == r for r in it) for v in meta_all[:, 2].tolist())
    kp_h, desc_h = host("tiled", 20)
    m = kp_h.shape[0]
    assert 5 <= m <= 20
    n, kp, u8, f32, meta = dev_extract(ctx, img, 20)
    assert n == m and (bits(kp) == bits(kp_h)).all()
    assert (bits(kp) == bits(kp_all[:m])).all() and (bits(meta) == bits(meta_all[:m])).all()
    check_descriptors("tiled, max_kp 20", f32, desc_h)


def test_cap_cuts_the_candidates_of_a_photograph(ctx, host):
    kp_h, desc_h = host("golden1", 100)
    n, kp, u8, f32, meta = dev_extract(ctx, image("golden1"), 100)
    assert 5 <= kp_h.shape[0] <= 100 and n == kp_h.shape[0]
    assert (bits(kp) == bits(kp_h)).all()
    check_descriptors("golden1, max_kp 100", f32, desc_h)


def test_gaussian_levels_bit_equal_to_the_host_arithmetic(ctx):
    img = image("97x131")
    sigma0, kf = 1.6, math.pow(2.0, 1.0 / 3)
    levels = [gaussian_np(img.astype(np.float32) / np.float32(255.0), math.sqrt(max(sigma0 * sigma0 - 0.25, 0.01)))]
    for i in range(1, 6):
        sp = sigma0 * math.pow(kf, i - 1)
        st = sp * kf
        levels.append(gaussian_np(levels[-1], math.sqrt(st * st - sp * sp)))
    oct1 = levels[3][::2, ::2]
    n = dev_extract(ctx, img)[0]
    assert n >= 5
    for (o, l), want in (((0, 0), levels[0]), ((0, 5), levels[5]), ((1, 0), oct1)):
        got = ctx.detect_level(o, l)
        assert got.shape == want.shape == ((131, 97) if o == 0 else (66, 49))
        assert (bits(got) == bits(want)).all(), (o, l, int((bits(got) != bits(want)).sum()))


def test_two_calls_are_byte_identical(ctx):
    img = image("golden2")
    a = dev_extract(ctx, img)
    b = dev_extract(ctx, img)
    assert a[0] == b[0] > 0
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()


def test_candidate_overflow_is_reported_not_truncated(ctx, host):
    img = image("129x128")
    kp_h, desc_h = host("129x128")
    ctx.set_option(api.PM_OPT_FEAT_CAPACITY, 16)
    try:
        assert ctx.get_option(api.PM_OPT_FEAT_CAPACITY) == 16
        n, kp, u8, f32, meta = dev_extract(ctx, img)
        assert n == -1
        kp_b, u8_b, f32_b, meta_b = ctx.detect_describe(img, MAX_KP)    # grows and runs again by itself
    finally:
        ctx.set_option(api.PM_OPT_FEAT_CAPACITY, 0)
    assert kp_b.shape[0] == kp_h.shape[0] and (bits(kp_b) == bits(kp_h)).all()
    n, kp, u8, f32, meta = dev_extract(ctx, img)
    assert n == kp_h.shape[0] and (u8 == u8_b).all() and (bits(meta) == bits(meta_b)).all()
    check_descriptors("129x128 after growing", f32_b, desc_h)


def test_pipeline_on_device_pointers(ctx, host):
    """extract -> pm_bf_knn_l2_u8_ratio_dev -> pm_ransac_run_dev on device buffers; only counts and F come to the host."""
    import torch
    dev = torch.device("cuda", 0)
    max_kp = MAX_KP
    bufs = []
    for name in ("golden1", "golden2"):
        img = image(name)
        d_img = torch.from_numpy(img).to(dev)
        d_kp = torch.zeros((max_kp, 2), dtype=torch.float32, device=dev)
        d_u8 = torch.zeros((max_kp, 128), dtype=torch.uint8, device=dev)
        d_n = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.detect_describe_dev(d_img.data_ptr(), img.shape[1], img.shape[0], img.shape[1], max_kp, d_kp.data_ptr(), d_u8.data_ptr(), 0, 0,
                                d_n.data_ptr())
        ctx.synchronize()
        bufs.append((d_kp, d_u8, int(d_n.item())))
    (d_kp1, d_q, n1), (d_kp2, d_t, n2) = bufs
    assert n1 > 60 and n2 > 60
    d_knn = torch.zeros((n1, 8), dtype=torch.int32, device=dev)
    d_good = torch.zeros((n1, 4), dtype=torch.int32, device=dev)
    d_xy1 = torch.zeros((n1, 2), dtype=torch.float32, device=dev)
    d_xy2 = torch.zeros((n1, 2), dtype=torch.float32, device=dev)
    d_ng = torch.zeros(1, dtype=torch.int32, device=dev)
    d_key = torch.zeros(1, dtype=torch.int64, device=dev)
    d_F = torch.zeros(9, dtype=torch.float64, device=dev)
    d_mask = torch.zeros(n1, dtype=torch.uint8, device=dev)
    d_ninl = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.bf_knn_l2_u8_ratio_dev(d_q.data_ptr(), n1, d_t.data_ptr(), n2, 128, 0.8, d_kp1.data_ptr(), d_kp2.data_ptr(), d_knn.data_ptr(),
                               d_good.data_ptr(), d_xy1.data_ptr(), d_xy2.data_ptr(), d_ng.data_ptr())
    ctx.ransac_run_dev(d_xy1.data_ptr(), d_xy2.data_ptr(), n1, d_ng.data_ptr(), 0, 2000, 1.0, 0x5EED, d_key.data_ptr(), d_F.data_ptr(),
                       d_mask.data_ptr(), d_ninl.data_ptr())
    ctx.synchronize()
    n_good, n_inl = int(d_ng.item()), int(d_ninl.item())
    F = d_F.cpu().numpy()
    assert n_good > 60
    assert n_inl >= 8 and np.isfinite(F).all() and abs(np.linalg.norm(F) - 1.0) < 1e-9
    # the match list from the host's features, when the device's descriptors equal them
    (kp1_h, desc1_h), (kp2_h, desc2_h) = host("golden1"), host("golden2")
    same = (d_q[:n1].cpu().numpy() == desc1_h).all() and (d_t[:n2].cpu().numpy() == desc2_h).all()
    print("pipeline: %d / %d keypoints, %d good matches, %d inliers, descriptors equal to the host's: %s" % (n1, n2, n_good, n_inl, same))
    if same:
        want = api.filter_ratio(ctx.bf_knn_l2_u8(desc1_h.astype(np.uint8), desc2_h.astype(np.uint8), 2), 0.8)
        got = d_good[:n_good].cpu().numpy().view(api.MATCH_DTYPE).reshape(-1)
        assert got.size == want.size and got.tobytes() == want.tobytes()
        assert (bits(d_xy1[:n_good].cpu().numpy()) == bits(kp1_h[want["queryIdx"]])).all()
        assert (bits(d_xy2[:n_good].cpu().numpy()) == bits(kp2_h[want["trainIdx"]])).all()


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_capturing_stream_is_refused():
    """Refused first thing: nothing is allocated or enqueued, and the context keeps working afterwards."""
    import gc
    import torch
    import points_matching_amd as pm
    dev = torch.device("cuda", 0)
    img = image("97x131")
    st = torch.cuda.Stream(device=dev)
    prev = torch.cuda.current_stream(dev)
    torch.cuda.set_stream(st)
    c = pm.Context(0)
    c.set_stream(st.cuda_stream)
    d_img = d_kp = d_n = None
    try:
        d_img = torch.from_numpy(img).to(dev)
        d_kp = torch.zeros((64, 2), dtype=torch.float32, device=dev)
        d_n = torch.full((1,), -5, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def call():
            c.detect_describe_dev(d_img.data_ptr(), 97, 131, 97, 64, d_kp.data_ptr(), 0, 0, 0, d_n.data_ptr())

        gc.collect()                     # no finaliser of an earlier test's context (hipFree) inside the capture
        g = torch.cuda.CUDAGraph()
        with pytest.raises(pm.PmError) as err:
            with torch.cuda.graph(g, stream=st, capture_error_mode="relaxed"):
                call()
        assert err.value.status == api.PM_E_UNSUPPORTED and "capturing" in str(err.value)
        del g, err                       # (the exception's traceback holds this frame: no cycle is left for a later collection)
        torch.cuda.set_stream(st)
        torch.cuda.synchronize()
        assert int(d_n.item()) == -5
        call()
        torch.cuda.synchronize()
        assert 5 <= int(d_n.item()) <= 64
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)
        c.close()
        del d_img, d_kp, d_n
        gc.collect()


def test_cli_device_features(tmp_path):
    build.build_host()
    img = [os.path.join(GOLD, "img01_half.pgm"), os.path.join(GOLD, "img02_half.pgm")]
    run = subprocess.run([build.HOST_BIN, "--features", "device", "--img1", img[0], "--img2", img[1], "--filter", "ratio", "--method", "ransac8",
                          "--json", "--quiet"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    rep = json.loads(run.stdout.strip().splitlines()[-1])
    assert rep["n1"] > 60 and rep["n2"] > 60 and rep["matches"] > 60 and rep["inliers"] >= 8 and rep["ransac_status"] == 0
    for where in ("host", "device"):
        out = subprocess.run([build.HOST_BIN, "--features", where, "--img1", img[0], "--img2", img[1], "--extract-only", "--save-features",
                              str(tmp_path / where), "--quiet"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
    for k in ("kp1", "kp2"):
        a, b = io.load_pmm(str(tmp_path / ("host_%s.pmm" % k))), io.load_pmm(str(tmp_path / ("device_%s.pmm" % k)))
        assert a.shape == b.shape and (bits(a) == bits(b)).all()
    for k in ("desc1", "desc2"):
        a, b = io.load_pmm(str(tmp_path / ("host_%s.pmm" % k))), io.load_pmm(str(tmp_path / ("device_%s.pmm" % k)))
        check_descriptors("cli " + k, b, a)
