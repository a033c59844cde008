"""GPU: the device feature front end (csrc/features.hip, pm_detect_describe* and pm_detect_describe_bits*, SPEC S53-S60) at
its limits: selections of more than 1024 and more than 2048 rows, max_kp = 1, the capacity edge, selections of which every
row is border-skipped, first-octave widths of 32, 33, 63, 64 and 65, five octaves, thresholds other than the defaults, and
every refusal.

The reference is the host extractor with every argument (tests/features_ref.py: tests/features_host_main.cpp around
host/pm_features.cpp, the specification); tests/test_features_limits_cpu.py pins it to pm_cli and pins what it makes of the
inputs used here.  Unless a test says otherwise the count, the keypoints and their order equal the host's bit for bit, the
gradient rows pass the caps of tests/test_features_device_gpu.py (2 % of rows may differ, 0.5 % by more than 1, at least one
row allowed) and the bit rows the cap of tests/test_features_bits_gpu.py (2 % of rows, at least one).  Every _dev call writes
into guard-filled outputs, and nothing behind the count (nothing at all on overflow or refusal) may change.  Measured shares:
profiles/features_parity.txt."""
import ctypes as C
import math

import numpy as np
import pytest

import features_ref as R
from features_ref import bits, candidate_responses, check_bit_rows, check_descriptors, host_features, image
from points_matching_amd import api

pytestmark = pytest.mark.gpu
KINDS = ["grad", "bits"]
GUARD_F, GUARD_B, GUARD_N = -7.0, 77, 12345


@pytest.fixture(scope="module")
def ctx():
    """A context of this module's own: its feature buffer and its capacity option go when the module is done."""
    import gc
    import torch
    import points_matching_amd as pm
    c = pm.Context(0)
    yield c
    torch.cuda.synchronize()
    c.close()
    gc.collect()


class Outputs:
    """Guard-filled device outputs of one _dev call of either kind, sized for max_kp rows."""

    def __init__(self, max_kp, kind):
        import torch
        dev = torch.device("cuda", 0)
        self.kind = kind
        self.kp = torch.full((max_kp, 2), GUARD_F, dtype=torch.float32, device=dev)
        self.meta = torch.full((max_kp, 4), GUARD_F, dtype=torch.float32, device=dev)
        self.n = torch.full((1,), GUARD_N, dtype=torch.int32, device=dev)
        if kind == "grad":
            self.u8 = torch.full((max_kp, 128), GUARD_B, dtype=torch.uint8, device=dev)
            self.f32 = torch.full((max_kp, 128), GUARD_F, dtype=torch.float32, device=dev)
        else:
            self.rows = torch.full((max_kp, 32), GUARD_B, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    def tensors(self):
        return [self.kp, self.meta] + ([self.u8, self.f32] if self.kind == "grad" else [self.rows])

    def untouched_from(self, m):
        """No row from m on was written."""
        return all(bool((t[m:] == (GUARD_B if t.dtype.itemsize == 1 else GUARD_F)).all()) for t in self.tensors())


class Result:
    pass


def dev_run(ctx, img, max_kp, kind, contrast=0.03, edge_r=10.0):
    """One _dev call into guard-filled outputs -> Result with n and the n rows of kp, meta and u8 + f32 (grad) or rows (bits).
    Nothing behind the count is written, nothing at all when the count is -1."""
    import torch
    h, w = img.shape
    d_img = torch.from_numpy(img).to(torch.device("cuda", 0))
    out = Outputs(max_kp, kind)
    if kind == "grad":
        ctx.detect_describe_dev(d_img.data_ptr(), w, h, w, max_kp, out.kp.data_ptr(), out.u8.data_ptr(), out.f32.data_ptr(), out.meta.data_ptr(),
                                out.n.data_ptr(), contrast, edge_r)
    else:
        ctx.detect_describe_bits_dev(d_img.data_ptr(), w, h, w, max_kp, out.kp.data_ptr(), out.rows.data_ptr(), out.meta.data_ptr(),
                                     out.n.data_ptr(), contrast, edge_r)
    ctx.synchronize()
    res = Result()
    res.kind, res.n = kind, int(out.n.item())
    assert -1 <= res.n <= max_kp
    m = max(res.n, 0)
    assert out.untouched_from(m)
    res.kp, res.meta = out.kp[:m].cpu().numpy(), out.meta[:m].cpu().numpy()
    if kind == "grad":
        res.u8, res.f32 = out.u8[:m].cpu().numpy(), out.f32[:m].cpu().numpy()
        res.desc = res.u8
    else:
        res.rows = out.rows[:m].cpu().numpy()
        res.desc = res.rows
    return res


_DEV = {}


def dev_cached(ctx, name, max_kp, kind):
    """dev_run at the default thresholds, once per (input, max_kp, kind)."""
    key = (name, max_kp, kind)
    if key not in _DEV:
        _DEV[key] = dev_run(ctx, image(name), max_kp, kind)
    return _DEV[key]


def same_bytes(a, b, rows=None):
    """kp, meta and descriptor rows of two results (or their first `rows` rows) are byte-identical."""
    s = slice(None, rows)
    return (a.kp[s].tobytes() == b.kp[s].tobytes() and a.meta[s].tobytes() == b.meta[s].tobytes() and
            a.desc[s].tobytes() == b.desc[s].tobytes() and (a.kind == "bits" or a.f32[s].tobytes() == b.f32[s].tobytes()))


def check_against_host(label, res, host):
    """Count, keypoints and order bit-equal to the host's; descriptors within the caps; meta in selection order."""
    kp_h, rows_h = host
    assert res.n == kp_h.shape[0], (label, res.n, kp_h.shape[0])
    assert (bits(res.kp) == bits(kp_h)).all(), label
    if res.n == 0:
        return
    if res.kind == "grad":
        assert (res.u8.astype(np.float32) == res.f32).all()
        check_descriptors(label, res.f32, rows_h)
    else:
        check_bit_rows(label, res.rows, rows_h)
    assert (np.diff(res.meta[:, 2]) <= 0).all() and (res.meta[:, 2] > 0).all(), label      # responses: non-increasing
    scale = np.exp2(res.meta[:, 3])
    assert (res.kp == np.rint(res.kp / scale[:, None]) * scale[:, None]).all()
    assert (res.meta[:, 0] > 1.6 * scale).all() and (np.abs(res.meta[:, 1]) < math.pi).all()


# ---- 1. more than 1024 and more than 2048 rows -----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,max_kp", R.LARGE_CASES)
def test_selections_past_one_and_two_compaction_rounds(ctx, name, max_kp, kind):
    """700x520 at max_kp 4000 keeps 2217 rows of a selection of more than 2048: feat_compact takes its second and third
    round (the s_base carry, s_wave reused), feat_rank runs more than two workgroups and a ragged last tile, feat_describe,
    feat_gather and feat_gather_bits run grids of more than 2048 rows (2217 is no multiple of 8), and the octave plan has
    five octaves (octave 4, 44x33, has no candidate on this input: test_octaves_three_and_four_decide_the_result has one).
    640x480 selects more than 1024 rows (two rounds).  max_kp 1025, 1024 and 1023 put the cut one row past, on and one row before the round boundary."""
    res = dev_cached(ctx, name, max_kp, kind)
    check_against_host("%s, max_kp %d, %s" % (name, max_kp, kind), res, host_features(name, max_kp, kind=kind))
    if max_kp == 4000:
        assert res.n > (2048 if name == "700x520" else 1024)
        octaves = set(res.meta[:, 3].astype(int).tolist())
        assert octaves >= {0, 1, 2}, octaves


def test_selection_sizes_and_five_octaves_on_the_device_s_own_levels(ctx):
    """The candidate counts behind the test above, from the numpy restatement of the scan on the device's levels: more than
    2048 candidates for 700x520 (third round of feat_compact, ninth workgroup of feat_rank), more than 1024 for 640x480, no
    candidate buffer near its automatic capacity of 65536.  Octave 4 of 700x520 is 44x33 and is the [::2, ::2] decimation of
    level 3 of octave 3, as every octave is of the one before."""
    for name, n_oct, floor in (("700x520", 5, 2048), ("640x480", 4, 1024)):
        res = dev_run(ctx, image(name), 4000, "bits")
        assert res.n == host_features(name, 4000, kind="bits")[0].shape[0]
        w, h = (int(v) for v in name.split("x"))
        plan = R.plan_octaves(w, h)
        assert len(plan) == n_oct
        with pytest.raises(api.PmError):
            ctx.detect_level(n_oct, 0)                                       # there is no further octave
        for o in range(1, n_oct):
            got, src = ctx.detect_level(o, 0), ctx.detect_level(o - 1, 3)
            assert got.shape == (plan[o][1], plan[o][0]) and src.shape == (plan[o - 1][1], plan[o - 1][0])
            assert (bits(got) == bits(src[::2, ::2])).all(), (name, o)
        cand = candidate_responses(ctx, n_oct)
        print("candidates of %s: %d, rows %d" % (name, cand.size, res.n))
        assert floor < cand.size < 4000 and cand.size >= res.n
        # every kept row's response is a candidate's, in the same order
        it = iter(cand.tolist())
        assert all(any(v == r for r in it) for v in res.meta[:, 2].tolist())
        if name == "700x520":
            assert (ctx.detect_level(4, 0).shape, ctx.detect_level(4, 5).shape) == ((33, 44), (33, 44))
        # the device's own count is exactly the restatement's: that capacity runs, one less overflows
        try:
            ctx.set_option(api.PM_OPT_FEAT_CAPACITY, cand.size)
            at_cap = dev_run(ctx, image(name), 4000, "bits")
            ctx.set_option(api.PM_OPT_FEAT_CAPACITY, cand.size - 1)
            below = dev_run(ctx, image(name), 4000, "bits")
        finally:
            ctx.set_option(api.PM_OPT_FEAT_CAPACITY, 0)
        assert at_cap.n == res.n and same_bytes(at_cap, res) and below.n == -1


@pytest.mark.parametrize("kind", KINDS)
def test_octaves_three_and_four_decide_the_result(ctx, kind):
    """"five" (512x512) has one candidate in each of five octaves.  Octave 4's is the strongest: pos_base, oct_off and the geom
    record of octave 4 put it first in the selection, where its 32x32 plane makes feat_describe skip it (max_kp = 1: no row).
    Octave 3's is next and is kept (its geom record and plane offset reach the descriptor).  The device counts exactly five
    candidates: capacity 5 runs, capacity 4 overflows."""
    img = image("five")
    for max_kp in (1, 2, 3, 4, 5, R.DEFAULT_MAX_KP):
        res = dev_run(ctx, img, max_kp, kind)
        assert res.n == max(0, min(max_kp, 5) - 1)
        assert res.kp.tolist() == [list(p) for p in R.FIVE_KEPT[:res.n]]
        check_against_host("five, max_kp %d, %s" % (max_kp, kind), res, host_features("five", max_kp, kind=kind))
        assert res.meta[:, 3].tolist() == [3.0, 0.0, 1.0, 2.0][:res.n]
    assert ctx.detect_level(4, 0).shape == (32, 32) and candidate_responses(ctx, 5).size == 5
    try:
        ctx.set_option(api.PM_OPT_FEAT_CAPACITY, 5)
        at_cap = dev_run(ctx, img, 8, kind)
        ctx.set_option(api.PM_OPT_FEAT_CAPACITY, 4)
        below = dev_run(ctx, img, 8, kind)
    finally:
        ctx.set_option(api.PM_OPT_FEAT_CAPACITY, 0)
    assert at_cap.n == 4 and same_bytes(at_cap, res) and below.n == -1


@pytest.mark.parametrize("kind", KINDS)
def test_cut_is_a_prefix_and_calls_repeat_byte_for_byte(ctx, kind):
    """The first 1024 selected are a prefix of the selection, so the rows kept of them are the leading rows of the uncapped
    result: kp, meta and descriptor bytes.  The blocking form and a second _dev call give the same bytes as the first."""
    full = dev_cached(ctx, "700x520", 4000, kind)
    assert full.n > 2048
    for max_kp in (1025, 1024, 1023):
        cut = dev_cached(ctx, "700x520", max_kp, kind)
        assert 512 < cut.n <= max_kp and same_bytes(cut, full, cut.n)
    again = dev_run(ctx, image("700x520"), 4000, kind)
    assert again.n == full.n and same_bytes(again, full)
    if kind == "grad":
        kp_b, u8_b, f32_b, meta_b = ctx.detect_describe(image("700x520"), 4000)
        assert f32_b.tobytes() == full.f32.tobytes()
    else:
        kp_b, u8_b, meta_b = ctx.detect_describe_bits(image("700x520"), 4000)
    assert kp_b.tobytes() == full.kp.tobytes() and u8_b.tobytes() == full.desc.tobytes() and meta_b.tobytes() == full.meta.tobytes()


# ---- 2. max_kp = 1 -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["97x131", "700x520"])
def test_max_kp_one(ctx, name, kind):
    """One selected row: the strongest candidate, kept or border-skipped, exactly as the host decides."""
    res = dev_run(ctx, image(name), 1, kind)
    assert res.n in (0, 1)
    check_against_host("%s, max_kp 1, %s" % (name, kind), res, host_features(name, 1, kind=kind))


# ---- 3. the capacity edge ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_capacity_edge(ctx, kind):
    """cnt > cap is overflow, so cnt == cap must run: with PM_OPT_FEAT_CAPACITY equal to the candidate count C of the tiled
    image the result is the full one, with C - 1 the count is -1 and no output byte changes, and with capacity C and
    max_kp = C + 50 the scratch rows are rows = cap < max_kp and the result is the full one again."""
    img = image("tiled")
    full = dev_run(ctx, img, 512, kind)
    cand = candidate_responses(ctx, 3).size
    assert cand > 83 and full.n == 83
    host = host_features("tiled", 512, kind=kind)
    check_against_host("tiled, %s" % kind, full, host)
    try:
        ctx.set_option(api.PM_OPT_FEAT_CAPACITY, cand)
        at_cap = dev_run(ctx, img, 512, kind)
        ctx.set_option(api.PM_OPT_FEAT_CAPACITY, cand - 1)
        below = dev_run(ctx, img, 512, kind)                      # (dev_run asserts that no row was written)
        ctx.set_option(api.PM_OPT_FEAT_CAPACITY, cand)
        rows_cap = dev_run(ctx, img, cand + 50, kind)
    finally:
        ctx.set_option(api.PM_OPT_FEAT_CAPACITY, 0)
    assert at_cap.n == full.n and same_bytes(at_cap, full)
    assert below.n == -1
    assert rows_cap.n == full.n and same_bytes(rows_cap, full)
    check_against_host("tiled, capacity = candidates, max_kp = capacity + 50, %s" % kind, rows_cap, host)
    after = dev_run(ctx, img, 512, kind)                          # the automatic capacity again
    assert after.n == full.n and same_bytes(after, full)


# ---- 4. small inputs -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", R.NO_ROWS)
def test_every_selected_row_is_border_skipped(ctx, name, kind):
    """At least 32 pixels a side, so every kernel runs (widths 32, 33, 63, 64 and 96: one feat_blur tile, one tile and a
    column, and feat_extrema's w - 16 below, one short of and equal to a lane group), but no candidate has r2 >= 23 pixels to
    every border: valid[] is 0 for every selected row, feat_compact publishes 0 from a selection that is not empty (63x64,
    64x64: asserted on the device's own levels), and no gather thread writes."""
    res = dev_run(ctx, image(name), R.DEFAULT_MAX_KP, kind)      # (dev_run asserts that no row was written)
    assert res.n == 0 and host_features(name, kind=kind)[0].shape[0] == 0
    if name in ("63x64", "64x64"):
        w, h = (int(v) for v in name.split("x"))
        cand = candidate_responses(ctx, len(R.plan_octaves(w, h)))
        assert cand.size >= 1
        assert cand.size == candidate_responses(R.NumpyLevels(image(name)), len(R.plan_octaves(w, h))).size
    if kind == "grad":
        out = ctx.detect_describe(image(name), 64)
    else:
        out = ctx.detect_describe_bits(image(name), 64)
    assert all(a.shape[0] == 0 for a in out)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,rows", R.FEW_ROWS)
def test_near_minimum_sizes_that_keep_rows(ctx, name, rows, kind):
    """65x65 (one feat_blur tile and a column; two octaves) keeps two rows, 72x70 one: a valid row among skipped ones."""
    res = dev_run(ctx, image(name), R.DEFAULT_MAX_KP, kind)
    assert res.n == rows
    check_against_host("%s, %s" % (name, kind), res, host_features(name, kind=kind))


@pytest.mark.parametrize("name", ["32x32", "33x40", "63x64", "64x64", "65x65"])
def test_levels_at_the_tile_widths(ctx, name):
    """Widths 32, 33, 63, 64 and 65: the first and the last Gaussian level of octave 0 equal the numpy restatement of the
    host's gaussian() bit for bit (reflection at both borders inside one tile, and across the tile boundary at 65)."""
    img = image(name)
    dev_run(ctx, img, 64, "bits")
    levels = R.octave_levels_np(R.first_level_np(img))
    for lev in (0, 5):
        got = ctx.detect_level(0, lev)
        assert got.shape == img.shape == levels[lev].shape
        assert (bits(got) == bits(levels[lev])).all(), (name, lev, int((bits(got) != bits(levels[lev])).sum()))


# ---- 5. thresholds ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("contrast,edge_r", R.THRESHOLDS)
@pytest.mark.parametrize("name", [R.THRESHOLD_IMAGE, R.THRESHOLD_PHOTO])
def test_thresholds_other_than_the_defaults(ctx, name, contrast, edge_r, kind):
    """contrast and edge_r reach feat_extrema (thr = contrast / 3 and the edge test, in float as on the host): count,
    keypoints, order and descriptors against the host extractor with the same arguments.  The CPU file asserts that the
    pairs change the count (all four on golden1; on 97x131 all but (0.03, 30), which no extremum of that image notices)."""
    res = dev_run(ctx, image(name), R.DEFAULT_MAX_KP, kind, contrast, edge_r)
    host = host_features(name, contrast=contrast, edge_r=edge_r, kind=kind)
    if name == R.THRESHOLD_PHOTO:
        assert host[0].shape[0] != host_features(name, kind=kind)[0].shape[0]
    check_against_host("%s, contrast %g, edge_r %g, %s" % (name, contrast, edge_r, kind), res, host)
    cand = candidate_responses(ctx, len(R.plan_octaves(image(name).shape[1], image(name).shape[0])), contrast, edge_r)
    assert cand.size >= res.n and (cand > np.float32(contrast) / np.float32(3)).all()


def test_negative_contrast_keypoints_only(ctx):
    """contrast = -1: !(fabsf(c) > thr) with a negative threshold rejects nothing, every extremum that passes the edge test is
    a candidate.  Keypoints only: the descriptor and meta outputs are NULL."""
    import torch
    img = image(R.THRESHOLD_IMAGE)
    h, w = img.shape
    dev = torch.device("cuda", 0)
    d_img = torch.from_numpy(img).to(dev)
    d_kp = torch.full((R.DEFAULT_MAX_KP, 2), GUARD_F, dtype=torch.float32, device=dev)
    d_n = torch.full((1,), GUARD_N, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.detect_describe_dev(d_img.data_ptr(), w, h, w, R.DEFAULT_MAX_KP, d_kp.data_ptr(), 0, 0, 0, d_n.data_ptr(), -1.0, 10.0)
    ctx.synchronize()
    kp_h, _ = host_features(R.THRESHOLD_IMAGE, contrast=-1.0)
    n = int(d_n.item())
    assert n == kp_h.shape[0] > host_features(R.THRESHOLD_IMAGE)[0].shape[0]
    assert (bits(d_kp[:n].cpu().numpy()) == bits(kp_h)).all() and bool((d_kp[n:] == GUARD_F).all())


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------

def test_argument_statuses_leave_the_outputs_untouched(ctx):
    """check_args in its order, through all four entry points: every PM_E_INVALID (null context, image, keypoints, count and,
    for the bits forms, rows; w = 0, h = 0, stride = w - 1, max_kp = 0 and -1, NaN contrast, NaN edge_r), PM_E_UNSUPPORTED
    above 100 000 000 pixels (never reading the image), an INVALID ahead of the pixel cap where both apply, and the
    small-image rule (31x32, 32x31), which writes the count and nothing else.  No refusal writes an output or the count."""
    import torch
    dev = torch.device("cuda", 0)
    L = api.lib()
    name, max_kp = R.THRESHOLD_IMAGE, 64
    img = image(name)
    H, W = img.shape
    d_img = torch.from_numpy(img).to(dev)
    nan = float("nan")
    vp = lambda v: C.c_void_p(v or 0)

    for kind in KINDS:
        bits_form = kind == "bits"
        # -- the _dev form
        out = Outputs(max_kp, kind)

        def call_dev(**kw):
            a = dict(ctx=ctx._h, img=d_img.data_ptr(), w=W, h=H, stride=W, max_kp=max_kp, contrast=0.03, edge_r=10.0, kp=out.kp.data_ptr(),
                     desc=(out.rows if bits_form else out.u8).data_ptr(), meta=out.meta.data_ptr(), n=out.n.data_ptr())
            a.update(kw)
            head = (a["ctx"], vp(a["img"]), a["w"], a["h"], a["stride"], a["max_kp"], C.c_float(a["contrast"]), C.c_float(a["edge_r"]), vp(a["kp"]))
            if bits_form:
                return L.pm_detect_describe_bits_dev(*head, vp(a["desc"]), vp(a["meta"]), vp(a["n"]))
            return L.pm_detect_describe_dev(*head, vp(a["desc"]), vp(out.f32.data_ptr()), vp(a["meta"]), vp(a["n"]))

        def dev_untouched():
            ctx.synchronize()
            return out.untouched_from(0) and int(out.n.item()) == GUARD_N

        # -- the blocking form: host arrays with the same guards
        h_kp = np.full((max_kp, 2), GUARD_F, np.float32)
        h_desc = np.full((max_kp, 32 if bits_form else 128), GUARD_B, np.uint8)
        h_f32 = np.full((max_kp, 128), GUARD_F, np.float32)
        h_meta = np.full((max_kp, 4), GUARD_F, np.float32)
        h_n = C.c_int32(GUARD_N)

        def call_host(**kw):
            a = dict(ctx=ctx._h, img=img.ctypes.data, w=W, h=H, stride=W, max_kp=max_kp, contrast=0.03, edge_r=10.0, kp=h_kp.ctypes.data,
                     desc=h_desc.ctypes.data, meta=h_meta.ctypes.data, n=C.addressof(h_n))
            a.update(kw)
            head = (a["ctx"], vp(a["img"]), a["w"], a["h"], a["stride"], a["max_kp"], C.c_float(a["contrast"]), C.c_float(a["edge_r"]), vp(a["kp"]))
            if bits_form:
                return L.pm_detect_describe_bits(*head, vp(a["desc"]), vp(a["meta"]), vp(a["n"]))
            return L.pm_detect_describe(*head, vp(a["desc"]), vp(h_f32.ctypes.data), vp(a["meta"]), vp(a["n"]))

        def host_untouched(n=GUARD_N):
            return ((h_kp == GUARD_F).all() and (h_desc == GUARD_B).all() and (h_f32 == GUARD_F).all() and (h_meta == GUARD_F).all() and
                    h_n.value == n)

        big = dict(w=10001, h=10001, stride=10001)                           # 100 020 001 pixels
        invalid = [dict(ctx=None), dict(img=0), dict(kp=0), dict(n=0), dict(w=0), dict(h=0), dict(stride=W - 1), dict(max_kp=0),
                   dict(max_kp=-1), dict(contrast=nan), dict(edge_r=nan),
                   # an INVALID ahead of the pixel cap, and ahead of the small-image rule
                   dict(big, max_kp=0), dict(big, contrast=nan), dict(big, kp=0), dict(big, stride=10000),
                   dict(w=31, h=32, stride=31, kp=0), dict(w=31, h=32, stride=31, edge_r=nan)]
        if bits_form:
            invalid += [dict(desc=0), dict(big, desc=0)]
        for call, untouched in ((call_dev, dev_untouched), (call_host, host_untouched)):
            for kw in invalid:
                assert call(**kw) == api.PM_E_INVALID, (kind, call.__name__, kw)
                assert untouched(), (kind, call.__name__, kw)
            assert call(**big) == api.PM_E_UNSUPPORTED and untouched(), (kind, call.__name__)
            assert call(w=1, h=100000001, stride=1) == api.PM_E_UNSUPPORTED and untouched(), (kind, call.__name__)
        # the small-image rule: the count is 0, nothing else is written (the stride of the 97-wide image serves both shapes)
        for w, h in ((31, 32), (32, 31)):
            out.n.fill_(GUARD_N)
            h_n.value = GUARD_N
            assert call_dev(w=w, h=h) == api.PM_OK and call_host(w=w, h=h) == api.PM_OK
            ctx.synchronize()
            assert int(out.n.item()) == 0 and out.untouched_from(0) and host_untouched(0)
        # and a good call through the same path gives the host's result
        out.n.fill_(GUARD_N)
        h_n.value = GUARD_N
        assert call_dev() == api.PM_OK and call_host() == api.PM_OK
        ctx.synchronize()
        kp_h, rows_h = host_features(name, max_kp, kind=kind)
        n = int(out.n.item())
        assert n == h_n.value == kp_h.shape[0] and 5 <= n < max_kp
        assert (bits(out.kp[:n].cpu().numpy()) == bits(kp_h)).all() and (bits(h_kp[:n]) == bits(kp_h)).all()
        assert out.untouched_from(n) and (h_kp[n:] == GUARD_F).all() and (h_desc[n:] == GUARD_B).all() and (h_meta[n:] == GUARD_F).all()
        d_desc = (out.rows if bits_form else out.u8)[:n].cpu().numpy()
        assert d_desc.tobytes() == h_desc[:n].tobytes() and out.meta[:n].cpu().numpy().tobytes() == h_meta[:n].tobytes()
        if bits_form:
            check_bit_rows("%s, max_kp %d, raw call" % (name, max_kp), d_desc, rows_h)
        else:
            assert (out.f32[:n].cpu().numpy() == d_desc).all() and (h_f32[:n] == h_desc[:n]).all()
            check_descriptors("%s, max_kp %d, raw call" % (name, max_kp), d_desc.astype(np.float32), rows_h)
