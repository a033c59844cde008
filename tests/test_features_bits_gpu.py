"""GPU: the binary descriptors of the device feature front end (pm_detect_describe_bits[_dev], SPEC S58-S60).

Three references: the numpy restatement of tests/features_bits_ref.py on the device's own Gaussian levels (every byte
equal: gathers, ballot packing and row gather, independent of the host C++), the host extractor behind
`pm_cli --features host --descriptor bits` (count, keypoints and order bit-equal; rows may differ only where the device's
atan2f moved a histogram bin: at most 2 % of rows, at least one allowed, the cap of the 128-D parity test; measured
shares: profiles/features_bits_parity.txt), and the 128-D form (its rows are a subsequence with equal keypoints and meta).
The inlier floor of the pipeline test is 80 % of the 131 inliers that the host extractor's rows give on the CPU
(profiles/features_bits_quality.txt, tools/features_bits_quality.py)."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import features_bits_ref as ref
from features_ref import bits, blobs, image
from points_matching_amd import api, build, io

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["97x131", "129x128", "160x65", "golden1", "golden2", "tiled"]
MAX_KP = 512        # above the candidate count of every input here (at most 315)
CPU_BITS_INLIERS = 131


@pytest.fixture(scope="module")
def ctx():
    import gc
    import torch
    import points_matching_amd as pm
    c = pm.Context(0)
    yield c
    torch.cuda.synchronize()
    c.close()
    gc.collect()


_HOST = {}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """host(name, max_kp) -> (kp (n, 2) f32, rows (n, 32) u8) of the host extractor; computed once per key."""
    build.build_host()
    d = tmp_path_factory.mktemp("hostbits")

    def run(name, max_kp=MAX_KP):
        key = (name, max_kp)
        if key not in _HOST:
            img = image(name)
            pgm = str(d / ("%s.pgm" % name))
            with open(pgm, "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
            pre = str(d / ("%s_%d" % (name, max_kp)))
            out = subprocess.run([build.HOST_BIN, "--features", "host", "--descriptor", "bits", "--img1", pgm, "--img2", pgm, "--extract-only",
                                  "--save-features", pre, "--quiet", "--max-kp", str(max_kp)], capture_output=True, text=True, timeout=300)
            assert out.returncode == 0, out.stderr
            rows = io.load_pmm(pre + "_desc1.pmm")
            assert rows.dtype == np.uint8
            _HOST[key] = (io.load_pmm(pre + "_kp1.pmm").reshape(-1, 2), rows.reshape(-1, 32))
        return _HOST[key]
    return run


def dev_extract(ctx, img, max_kp=MAX_KP):
    """pm_detect_describe_bits_dev on torch buffers -> (n, kp, rows, meta) with n rows each (n = -1: none)."""
    import torch
    dev = torch.device("cuda", 0)
    h, w = img.shape
    d_img = torch.from_numpy(img).to(dev)
    d_kp = torch.full((max_kp, 2), -7.0, dtype=torch.float32, device=dev)
    d_b = torch.full((max_kp, 32), 77, dtype=torch.uint8, device=dev)
    d_meta = torch.full((max_kp, 4), -7.0, dtype=torch.float32, device=dev)
    d_n = torch.full((1,), 12345, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.detect_describe_bits_dev(d_img.data_ptr(), w, h, w, max_kp, d_kp.data_ptr(), d_b.data_ptr(), d_meta.data_ptr(), d_n.data_ptr())
    ctx.synchronize()
    n = int(d_n.item())
    m = max(n, 0)
    # nothing is written behind the count (and nothing at all on overflow)
    assert (d_kp[m:] == -7.0).all() and (d_b[m:] == 77).all() and (d_meta[m:] == -7.0).all()
    return n, d_kp[:m].cpu().numpy(), d_b[:m].cpu().numpy(), d_meta[:m].cpu().numpy()


_DEV = {}


@pytest.fixture(scope="module")
def dev(ctx):
    """dev(name) -> (n, kp, rows, meta, want): the uncapped device run of an input, once, with the numpy restatement of its
    rows evaluated right behind it on the Gaussian levels this run left (pm_detect_level_get after the bits form)."""
    _, steer = api.detect_bits_table()
    kf = math.pow(2.0, 1.0 / 3)

    def run(name):
        if name not in _DEV:
            n, kp, rows, meta = dev_extract(ctx, image(name))
            planes = {}
            want = np.zeros((max(n, 0), 32), np.uint8)
            for i in range(max(n, 0)):
                o = int(meta[i, 3])
                scale = float(1 << o)
                lev = int(round(math.log(meta[i, 0] / scale / 1.6) / math.log(kf)))          # sigma = 1.6 * 2^(lev / 3) * 2^octave
                b = int(round((float(meta[i, 1]) + math.pi) / (2 * math.pi) * 36 - 0.5))      # theta = bin-centre angle
                assert 1 <= lev <= 3 and 0 <= b < 36
                if (o, lev) not in planes:
                    planes[(o, lev)] = ctx.detect_level(o, lev)
                x, y = kp[i] / scale
                assert x == int(x) and y == int(y)
                want[i] = ref.describe(planes[(o, lev)], int(x), int(y), steer[lev - 1, b])
            _DEV[name] = (n, kp, rows, meta, want, sorted(planes))
        return _DEV[name]
    return run


@pytest.mark.parametrize("name", NAMES)
def test_every_byte_equals_the_numpy_restatement(dev, name):
    n, kp, rows, meta, want, used = dev(name)
    assert n >= 5 and rows.shape == (n, 32)
    assert (rows == want).all(), (name, int((rows != want).any(axis=1).sum()), n)
    share = np.unpackbits(rows).mean()
    assert 0.35 < share < 0.65, share
    if name != "tiled":                                               # (the tiles are translated copies: equal rows there)
        assert len({r.tobytes() for r in rows}) > n // 2              # rows are not copies of one another


def test_inputs_cover_octaves_levels_and_border_drops(ctx, dev):
    used = set()
    for name in NAMES:
        used |= set(dev(name)[5])
    assert {l for _, l in used} == {1, 2, 3} and len({o for o, _ in used}) >= 2
    # the tiled image: 142 candidates, 59 of them dropped by the border rule (the count of the 128-D form's test)
    assert dev("tiled")[0] == 83


@pytest.mark.parametrize("name", NAMES)
def test_keypoints_bit_equal_and_rows_within_the_cap_of_the_host_twin(host, dev, name):
    kp_h, rows_h = host(name)
    n, kp, rows, meta, _, _ = dev(name)
    assert n == kp_h.shape[0] and (bits(kp) == bits(kp_h)).all()
    differ = int((rows != rows_h).any(axis=1).sum())
    print("features bits parity %s: rows %d, rows that differ %d (%.4f)" % (name, n, differ, differ / n))
    assert differ <= max(1, int(0.02 * n)), (name, differ, n)


@pytest.mark.parametrize("name", NAMES)
def test_gradient_rows_are_a_subsequence_with_equal_keypoints_and_meta(ctx, dev, name):
    import torch
    n, kp, rows, meta, _, _ = dev(name)
    img = image(name)
    d = torch.device("cuda", 0)
    d_img = torch.from_numpy(img).to(d)
    d_kp = torch.zeros((MAX_KP, 2), dtype=torch.float32, device=d)
    d_u8 = torch.zeros((MAX_KP, 128), dtype=torch.uint8, device=d)
    d_meta = torch.zeros((MAX_KP, 4), dtype=torch.float32, device=d)
    d_n = torch.zeros(1, dtype=torch.int32, device=d)
    torch.cuda.synchronize()
    ctx.detect_describe_dev(d_img.data_ptr(), img.shape[1], img.shape[0], img.shape[1], MAX_KP, d_kp.data_ptr(), d_u8.data_ptr(), 0,
                            d_meta.data_ptr(), d_n.data_ptr())
    ctx.synchronize()
    m = int(d_n.item())
    assert 5 <= m <= n
    kp_g, meta_g = d_kp[:m].cpu().numpy(), d_meta[:m].cpu().numpy()
    key = [bits(kp[i]).tobytes() + bits(meta[i]).tobytes() for i in range(n)]
    it = iter(key)
    for j in range(m):
        k = bits(kp_g[j]).tobytes() + bits(meta_g[j]).tobytes()
        assert any(k == v for v in it), (name, j)


def test_two_calls_and_the_blocking_form_are_byte_identical(ctx, dev):
    for name in ("golden2", "160x65"):
        a = dev(name)
        b = dev_extract(ctx, image(name))
        assert a[0] == b[0] > 0
        for x, y in zip(a[1:4], b[1:]):
            assert x.tobytes() == y.tobytes()
        kp_b, rows_b, meta_b = ctx.detect_describe_bits(image(name), MAX_KP)
        assert kp_b.tobytes() == a[1].tobytes() and rows_b.tobytes() == a[2].tobytes() and meta_b.tobytes() == a[3].tobytes()


def test_small_image_gives_no_keypoints(ctx):
    img = blobs(31, 40, 11, 20)
    assert dev_extract(ctx, img, 64)[0] == 0
    kp_b, rows_b, meta_b = ctx.detect_describe_bits(img, 64)
    assert kp_b.shape == (0, 2) and rows_b.shape == (0, 32) and meta_b.shape == (0, 4)


def test_cap_inside_the_candidate_list_keeps_the_selection_order(ctx, host, dev):
    n_all, kp_all, rows_all, meta_all, _, _ = dev("tiled")
    kp_h, rows_h = host("tiled", 20)
    m = kp_h.shape[0]
    assert 5 <= m <= 20
    n, kp, rows, meta = dev_extract(ctx, image("tiled"), 20)
    assert n == m and (bits(kp) == bits(kp_h)).all()
    assert kp.tobytes() == kp_all[:m].tobytes() and meta.tobytes() == meta_all[:m].tobytes() and rows.tobytes() == rows_all[:m].tobytes()
    assert int((rows != rows_h).any(axis=1).sum()) <= 1


def test_candidate_overflow_is_reported_not_truncated(ctx, dev):
    name = "129x128"
    n_all, kp_all, rows_all, meta_all, _, _ = dev(name)
    ctx.set_option(api.PM_OPT_FEAT_CAPACITY, 16)
    try:
        n, kp, rows, meta = dev_extract(ctx, image(name))           # asserts that no row was written
        assert n == -1
        kp_b, rows_b, meta_b = ctx.detect_describe_bits(image(name), MAX_KP)     # grows and runs again by itself
    finally:
        ctx.set_option(api.PM_OPT_FEAT_CAPACITY, 0)
    assert kp_b.tobytes() == kp_all.tobytes() and rows_b.tobytes() == rows_all.tobytes() and meta_b.tobytes() == meta_all.tobytes()
    n, kp, rows, meta = dev_extract(ctx, image(name))
    assert n == n_all and rows.tobytes() == rows_all.tobytes()


def test_pipeline_on_device_pointers(ctx, host):
    """bits extract -> pm_bf_knn_hamming_u8_dev (k = 2) -> pm_filter_ratio_gather_dev (0.8) -> pm_ransac_run_dev on device
    buffers; only counts and F come to the host."""
    import torch
    dev = torch.device("cuda", 0)
    bufs = []
    for name in ("golden1", "golden2"):
        img = image(name)
        d_img = torch.from_numpy(img).to(dev)
        d_kp = torch.zeros((MAX_KP, 2), dtype=torch.float32, device=dev)
        d_b = torch.zeros((MAX_KP, 32), dtype=torch.uint8, device=dev)
        d_n = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.detect_describe_bits_dev(d_img.data_ptr(), img.shape[1], img.shape[0], img.shape[1], MAX_KP, d_kp.data_ptr(), d_b.data_ptr(), 0,
                                     d_n.data_ptr())
        ctx.synchronize()
        bufs.append((d_kp, d_b, int(d_n.item())))
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
    ctx.bf_knn_hamming_dev(d_q.data_ptr(), n1, d_t.data_ptr(), n2, 32, 2, d_knn.data_ptr())
    ctx.filter_ratio_gather_dev(d_knn.data_ptr(), n1, 2, 0.8, d_kp1.data_ptr(), d_kp2.data_ptr(), d_good.data_ptr(), d_xy1.data_ptr(),
                                d_xy2.data_ptr(), d_ng.data_ptr())
    ctx.ransac_run_dev(d_xy1.data_ptr(), d_xy2.data_ptr(), n1, d_ng.data_ptr(), 0, 2000, 1.0, 0x5EED, d_key.data_ptr(), d_F.data_ptr(),
                       d_mask.data_ptr(), d_ninl.data_ptr())
    ctx.synchronize()
    n_good, n_inl = int(d_ng.item()), int(d_ninl.item())
    F = d_F.cpu().numpy()
    (kp1_h, rows1_h), (kp2_h, rows2_h) = host("golden1"), host("golden2")
    same = (d_q[:n1].cpu().numpy() == rows1_h).all() and (d_t[:n2].cpu().numpy() == rows2_h).all()
    print("bits pipeline: %d / %d keypoints, %d good matches, %d inliers, rows equal to the host's: %s" % (n1, n2, n_good, n_inl, same))
    assert np.isfinite(F).all() and abs(np.linalg.norm(F) - 1.0) < 1e-9
    assert n_inl >= math.ceil(0.8 * CPU_BITS_INLIERS), (n_good, n_inl)
    if same:
        want = api.filter_ratio(ctx.bf_knn_hamming(rows1_h, rows2_h, 2), 0.8)
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
    d_img = d_kp = d_b = d_n = None
    try:
        d_img = torch.from_numpy(img).to(dev)
        d_kp = torch.zeros((64, 2), dtype=torch.float32, device=dev)
        d_b = torch.zeros((64, 32), dtype=torch.uint8, device=dev)
        d_n = torch.full((1,), -5, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def call():
            c.detect_describe_bits_dev(d_img.data_ptr(), 97, 131, 97, 64, d_kp.data_ptr(), d_b.data_ptr(), 0, d_n.data_ptr())

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
        del d_img, d_kp, d_b, d_n
        gc.collect()


def test_cli_device_bits(tmp_path):
    build.build_host()
    img = [os.path.join(GOLD, "img01_half.pgm"), os.path.join(GOLD, "img02_half.pgm")]
    saved, listing = {}, {}
    for where in ("host", "device"):
        out = subprocess.run([build.HOST_BIN, "--features", where, "--descriptor", "bits", "--img1", img[0], "--img2", img[1], "--filter", "ratio",
                              "--method", "ransac8", "--json", "--save-features", str(tmp_path / where)], capture_output=True, text=True,
                             timeout=300)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.strip().splitlines()
        rep = json.loads(lines[-1])
        assert rep["n1"] > 60 and rep["n2"] > 60 and rep["ransac_status"] == 0
        assert rep["inliers"] >= math.ceil(0.8 * CPU_BITS_INLIERS), rep
        listing[where] = out.stdout
        saved[where] = {k: io.load_pmm(str(tmp_path / ("%s_%s.pmm" % (where, k)))) for k in ("kp1", "kp2", "desc1", "desc2")}
    equal = True
    for k in ("kp1", "kp2"):
        a, b = saved["host"][k], saved["device"][k]
        assert a.shape == b.shape and (bits(a) == bits(b)).all()
    for k in ("desc1", "desc2"):
        a, b = saved["host"][k], saved["device"][k]
        assert a.dtype == b.dtype == np.uint8 and a.shape == b.shape and a.shape[1] == 32
        differ = int((a != b).any(axis=1).sum())
        print("features bits parity cli %s: rows %d, rows that differ %d" % (k, a.shape[0], differ))
        assert differ <= max(1, int(0.02 * a.shape[0]))
        equal = equal and differ == 0
    if equal:
        strip = [[ln for ln in listing[w].splitlines() if not ln.lstrip().startswith("{")] for w in ("host", "device")]
        assert strip[0] == strip[1] and len(strip[0]) > 60
