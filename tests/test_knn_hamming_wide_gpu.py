"""GPU parity of the 512-bit matrix-core route of pm_bf_knn_hamming_u8 (descriptors of 36 .. 64 bytes, k <= 2; SPEC
S51/S52) against the CPU oracle, bit for bit; plus pm_pad_rows_u8_dev and pm_cli on 61-byte rows.

The yardstick is oracle.bf_knn_hamming on rows zero-padded to a multiple of 4 bytes (tests/test_hamming_wide_cpu.py checks
the yardstick itself against a numpy popcount)."""
import subprocess
import time

import numpy as np
import pytest

import points_matching_amd as pm
from points_matching_amd import api, build, io, synth
from test_hamming_wide_cpu import pad4
from test_knn_large_train_gpu import THREADS, Plants, _mem_used_mib, _record, _records, interesting_rows, near_bit
from util import assert_matches_equal

pytestmark = pytest.mark.gpu

WIDE_NAMES = ("knn_hamming512_expand", "knn_hamming512_mfma_i8", "knn_hamming512_refine")
ALL_NAMES = WIDE_NAMES + ("knn_hamming_expand", "knn_hamming_mfma_i8", "knn_hamming_refine", "knn_hamming", "knn_hamming_merge")


def _launches(ctx, fn):
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        out = fn()
        return out, {n: ctx.timing_get(n)[1] for n in ALL_NAMES}
    finally:
        ctx.timing_enable(False)


def _with_options(ctx, opts, fn):
    try:
        for o, v in opts.items():
            ctx.set_option(o, v)
        return fn()
    finally:
        for o in opts:
            ctx.set_option(o, 0)


# ---- route taken ----------------------------------------------------------------------------------------------------------

def test_wide_route_is_the_one_timed(ctx):
    """64 bytes, k = 2, 512 x 512: expansion, coarse kernel and refinement of the 512-bit route once each, under names of
    their own; k = 3 and PM_OPT_HAMMING_ROUTE = 1 launch only the scan."""
    q, t, _ = synth.orb_like(512, 512, 64, seed=5)
    _, n = _launches(ctx, lambda: ctx.bf_knn_hamming(q, t, 2))
    assert n == {"knn_hamming512_expand": 1, "knn_hamming512_mfma_i8": 1, "knn_hamming512_refine": 1, "knn_hamming_expand": 0,
                 "knn_hamming_mfma_i8": 0, "knn_hamming_refine": 0, "knn_hamming": 0, "knn_hamming_merge": 0}, n
    _, n = _launches(ctx, lambda: ctx.bf_knn_hamming(q, t, 3))
    assert all(n[x] == 0 for x in WIDE_NAMES) and n["knn_hamming_mfma_i8"] == 0 and n["knn_hamming"] == 1, n
    _, n = _with_options(ctx, {api.PM_OPT_HAMMING_ROUTE: 1}, lambda: _launches(ctx, lambda: ctx.bf_knn_hamming(q, t, 2)))
    assert all(n[x] == 0 for x in WIDE_NAMES) and n["knn_hamming_mfma_i8"] == 0 and n["knn_hamming"] == 1, n
    # every length of the route, and the lengths next to it
    for nbytes, wide in ((28, False), (36, True), (48, True), (60, True), (68, False)):
        q, t, _ = synth.orb_like(300, 300, nbytes, seed=nbytes)
        _, n = _launches(ctx, lambda: ctx.bf_knn_hamming(q, t, 2))
        assert n["knn_hamming512_mfma_i8"] == (1 if wide else 0) and n["knn_hamming"] == (0 if wide else 1), (nbytes, n)
        assert n["knn_hamming_mfma_i8"] == 0 and n["knn_hamming512_expand"] == n["knn_hamming512_mfma_i8"], (nbytes, n)


# ---- records equal the oracle ---------------------------------------------------------------------------------------------

SHAPES = [(257, 129, 1), (5, 128, 2), (64, 2, 2), (1, 1, 1), (700, 1000, 2), (1030, 4100, 2), (33, 9000, 2)]


@pytest.mark.parametrize("nbytes", [64, 60, 48, 36])
@pytest.mark.parametrize("nq,nt,k", SHAPES)
def test_wide_records_equal_the_oracle(ctx, oracle, nq, nt, k, nbytes):
    """Across the 256-query block, the 128-row tile, one split and several; default route, scan and 64-bit keys; all three
    refinement forms."""
    q, t, _ = synth.orb_like(nq, nt, nbytes, seed=7 * nq + nt + nbytes)
    want = oracle.bf_knn_hamming(q, t, k, nthreads=8)
    try:
        for route in (0, 1, 2):
            ctx.set_option(api.PM_OPT_HAMMING_ROUTE, route)
            for form in (0, 1, 2):
                ctx.set_option(api.PM_OPT_HAMMING_REFINE, form)
                assert_matches_equal(ctx.bf_knn_hamming(q, t, k), want, "route %d refinement form %d" % (route, form))
    finally:
        ctx.set_option(api.PM_OPT_HAMMING_ROUTE, 0)
        ctx.set_option(api.PM_OPT_HAMMING_REFINE, 0)


@pytest.mark.parametrize("nbytes", [64, 48])
def test_wide_register_staging_same_result(ctx, oracle, nbytes):
    q, t, _ = synth.orb_like(1030, 4100, nbytes, seed=99 + nbytes)
    want = oracle.bf_knn_hamming(q, t, 2, nthreads=8)
    got, n = _with_options(ctx, {api.PM_OPT_KNN_STAGING: 1}, lambda: _launches(ctx, lambda: ctx.bf_knn_hamming(q, t, 2)))
    assert n["knn_hamming512_mfma_i8"] == 1 and n["knn_hamming"] == 0, n
    assert_matches_equal(got, want, "register staging")
    assert_matches_equal(ctx.bf_knn_hamming(q, t, 2), want, "LDS-DMA (default)")


def _dev_call(ctx, d_q, d_t, nq, nt, nbytes, k):
    import torch
    d_out = torch.full((nq, k, 4), -5, dtype=torch.int32, device=d_q.device)
    ctx.bf_knn_hamming_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, nbytes, k, d_out.data_ptr())
    ctx.synchronize()
    return _records(d_out, nq, k)


@pytest.mark.parametrize("nbytes", [64, 60])
def test_wide_device_pointers_4_bytes_off_a_16_byte_boundary(ctx, oracle, nbytes):
    """4-byte-aligned buffers that are not 16-byte aligned: the route reads through its padded packed copy."""
    import torch
    dev = torch.device("cuda", 0)
    nq, nt, k = 700, 1000, 2
    q, t, _ = synth.orb_like(nq, nt, nbytes, seed=3 + nbytes)
    want = oracle.bf_knn_hamming(q, t, k, nthreads=8)
    bq = torch.zeros(nq * nbytes + 64, dtype=torch.uint8, device=dev)
    bt = torch.zeros(nt * nbytes + 64, dtype=torch.uint8, device=dev)
    assert bq.data_ptr() % 16 == 0 and bt.data_ptr() % 16 == 0
    d_q, d_t = bq[4:4 + nq * nbytes], bt[4:4 + nt * nbytes]
    d_q.copy_(torch.from_numpy(q.reshape(-1)).to(dev))
    d_t.copy_(torch.from_numpy(t.reshape(-1)).to(dev))
    assert d_q.data_ptr() % 16 == 4 and d_t.data_ptr() % 16 == 4
    got, n = _launches(ctx, lambda: _dev_call(ctx, d_q, d_t, nq, nt, nbytes, k))
    assert n["knn_hamming512_mfma_i8"] == 1 and n["knn_hamming"] == 0, n
    assert_matches_equal(got, want, "offset pointers")
    # only the train side off the boundary
    d_q2 = torch.from_numpy(q).to(dev)
    assert_matches_equal(_dev_call(ctx, d_q2, d_t, nq, nt, nbytes, k), want, "offset train pointer")


# ---- ties and limits ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nbytes", [64, 48])
def test_wide_degenerate_ties_and_the_complement(ctx, oracle, nbytes):
    rng = np.random.default_rng(3 + nbytes)
    t = np.zeros((600, nbytes), np.uint8)
    q = np.zeros((70, nbytes), np.uint8)
    assert_matches_equal(ctx.bf_knn_hamming(q, t, 2), oracle.bf_knn_hamming(q, t, 2), "all zero")
    # three distinct rows repeated: many exact ties at the k-th distance
    base = rng.integers(0, 256, (3, nbytes), dtype=np.uint8)
    t = base[rng.integers(0, 3, 900)]
    q = base[rng.integers(0, 3, 130)]
    q[::7] ^= 1
    assert_matches_equal(ctx.bf_knn_hamming(q, t, 2), oracle.bf_knn_hamming(q, t, 2), "three values")
    # complemented queries: query i is at the bit count (512 at 64 bytes) from row i, and at about half of it from the
    # others; the all-zero rows padding the 128-row tile (coarse distance 256) must still lose.  A distance of 512 does not
    # fit (distance << 23 | row): it would wrap to key 0 and win
    t = rng.integers(0, 256, (130, nbytes), dtype=np.uint8)
    q = (~t[:40]).copy()
    want = oracle.bf_knn_hamming(q, t, 2)
    assert (want["trainIdx"][:, 0] != np.arange(40)).all() and (want["trainIdx"] >= 0).all()
    for route in (0, 2):
        got = _with_options(ctx, {api.PM_OPT_HAMMING_ROUTE: route}, lambda: ctx.bf_knn_hamming(q, t, 2))
        assert_matches_equal(got, want, "complement, route %d" % route)
    # ... and with ONLY the complements to choose from the answer IS the bit count
    t2 = t[:2].copy()
    q2 = (~t2).copy()
    t2[1] = t2[0]
    want = oracle.bf_knn_hamming(q2, t2, 2)
    assert want["distance"][0, 0] == 8 * nbytes and list(want["trainIdx"][0]) == [0, 1]
    for route in (0, 2):
        got = _with_options(ctx, {api.PM_OPT_HAMMING_ROUTE: route}, lambda: ctx.bf_knn_hamming(q2, t2, 2))
        assert_matches_equal(got, want, "only complements, route %d" % route)


@pytest.mark.parametrize("nbytes", [64, 48])
def test_wide_cluster_in_one_group_stream_and_lowest_index(ctx, oracle, nbytes):
    """More than 4 near rows inside one lane stream (same split, same half): the 4-deep list overflows.  Planted duplicates:
    the lower index first."""
    rng = np.random.default_rng(11 + nbytes)
    t = rng.integers(0, 256, (2048, nbytes), dtype=np.uint8)
    q = rng.integers(0, 256, (96, nbytes), dtype=np.uint8)
    rows = [0, 8, 16, 24, 32, 40, 64, 72]            # rows with (row % 8) < 4: lane half 0, distinct groups
    for i, r in enumerate(rows):
        t[r] = q[0]
        t[r, nbytes - 1] ^= np.uint8(1 << (i % 8))   # distance 1 each
    t[1000] = q[0]
    t[400] = t[3]
    t[100] = t[3]
    t[2047] = t[3]
    q[1] = t[3]
    want = oracle.bf_knn_hamming(q, t, 2)
    assert list(want["trainIdx"][0]) == [1000, 0] and list(want["trainIdx"][1]) == [3, 100]
    for form in (0, 1):
        got = _with_options(ctx, {api.PM_OPT_HAMMING_REFINE: form}, lambda: ctx.bf_knn_hamming(q, t, 2))
        assert_matches_equal(got, want, "cluster, refinement form %d" % form)


def test_wide_randomised_shapes(ctx, oracle):
    """Seeded sweep over shapes, descriptor sizes on both sides of the route's limits, and k."""
    rng = np.random.default_rng(0x512)
    for case in range(30):
        nq = int(rng.integers(1, 900))
        nt = int(rng.integers(1, 1500))
        nbytes = int(rng.choice([4, 8, 16, 28, 36, 48, 60, 64]))
        k = int(rng.choice([1, 2, 3, 5]))
        if case % 3 == 0:                              # few distinct values: ties everywhere
            base = rng.integers(0, 256, (4, nbytes), dtype=np.uint8)
            q = base[rng.integers(0, 4, nq)].copy()
            t = base[rng.integers(0, 4, nt)].copy()
            t[::5, 0] ^= 1
        else:
            q = rng.integers(0, 256, (nq, nbytes), dtype=np.uint8)
            t = rng.integers(0, 256, (nt, nbytes), dtype=np.uint8)
            sel = rng.integers(0, nt, max(1, nq // 2))
            q[:sel.size] = t[sel]
            q[:sel.size, rng.integers(0, nbytes)] ^= np.uint8(rng.integers(0, 256))
        assert_matches_equal(ctx.bf_knn_hamming(q, t, k), oracle.bf_knn_hamming(q, t, k),
                             "case %d: nq=%d nt=%d bytes=%d k=%d" % (case, nq, nt, nbytes, k))


# ---- what is built on the matcher -----------------------------------------------------------------------------------------

def test_wide_cross_check_equals_the_filter_on_the_oracles_lists(ctx, oracle):
    nq, nt = 600, 700
    q, t, _ = synth.orb_like(nq, nt, 64, seed=41)
    flags = api.PM_CROSS_RATIO_FWD | api.PM_CROSS_RATIO_REV
    fwd = oracle.bf_knn_hamming(q, t, 2, nthreads=8)
    rev = oracle.bf_knn_hamming(t, q, 2, nthreads=8)
    want = api.filter_cross(fwd, rev, flags, 0.8)
    assert 0 < want.size < nq
    got, n = _launches(ctx, lambda: ctx.bf_match_cross_hamming(q, t, flags, 0.8))
    assert n["knn_hamming512_mfma_i8"] == 2 and n["knn_hamming"] == 0, n
    assert_matches_equal(got, want, "cross-check")


def test_pad_rows_dev_and_the_matcher_on_padded_rows(ctx, oracle):
    """AKAZE's 61 bytes -> 64 on the device (one launch, any source alignment); the matcher on the padded rows = the
    yardstick."""
    import torch
    dev = torch.device("cuda", 0)
    nq, nt, k = 300, 777, 2
    q, t, _ = synth.orb_like(nq, nt, 61, seed=61)
    d_q, d_t = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
    p_q = torch.full((nq, 64), 0xEE, dtype=torch.uint8, device=dev)
    p_t = torch.full((nt, 64), 0xEE, dtype=torch.uint8, device=dev)
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        ctx.pad_rows_u8_dev(d_q.data_ptr(), nq, 61, p_q.data_ptr(), 64)
        ctx.pad_rows_u8_dev(d_t.reshape(-1)[61:].data_ptr(), nt - 1, 61, p_t[1:].data_ptr(), 64)     # an odd source address
        ctx.pad_rows_u8_dev(d_t.data_ptr(), 1, 61, p_t.data_ptr(), 64)
        ctx.pad_rows_u8_dev(0, 0, 61, 0, 64)                                                          # n == 0: PM_OK, no launch
        ctx.synchronize()
        assert ctx.timing_get("pad_rows_u8")[1] == 3
    finally:
        ctx.timing_enable(False)
    assert (p_q.cpu().numpy() == pad4(q)).all() and (p_t.cpu().numpy() == pad4(t)).all()
    with pytest.raises(pm.PmError):
        ctx.pad_rows_u8_dev(d_q.data_ptr(), nq, 61, p_q.data_ptr(), 60)
    with pytest.raises(pm.PmError):
        ctx.pad_rows_u8_dev(0, nq, 61, p_q.data_ptr(), 64)
    want = oracle.bf_knn_hamming(pad4(q), pad4(t), k, nthreads=8)
    assert_matches_equal(_dev_call(ctx, p_q, p_t, nq, nt, 64, k), want, "padded rows")
    assert_matches_equal(ctx.bf_knn_hamming(api.pad_rows_u8(q, 64), api.pad_rows_u8(t, 64), k), want, "host-padded rows")


def test_cli_pads_61_column_files(tmp_path, oracle):
    """uint8 descriptor files with 61 columns: pm_cli pads both to 64 and prints the match list of the padded pair."""
    nq, nt = 300, 280
    q, t, _ = synth.orb_like(nq, nt, 61, seed=77)
    rng = np.random.default_rng(77)
    arrays = {"q": q, "t": t, "kp1": rng.uniform(0, 900, (nq, 2)).astype(np.float32),
              "kp2": rng.uniform(0, 600, (nt, 2)).astype(np.float32)}
    paths = {}
    for name, a in arrays.items():
        paths[name] = str(tmp_path / (name + ".pmm"))
        io.save_pmm(paths[name], a)
    cmd = [build.HOST_BIN, "--desc1", paths["q"], "--desc2", paths["t"], "--kp1", paths["kp1"], "--kp2", paths["kp2"],
           "--filter", "ratio", "--method", "ransac8", "--iters", "100", "--seed", "3"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    good = oracle.filter_ratio(oracle.bf_knn_hamming(pad4(q), pad4(t), 2), 0.8)
    exp = oracle.format_match_list(good).splitlines()
    assert good.size > 100 and out.stdout.splitlines()[:len(exp)] == exp
    cross = subprocess.run(cmd[:9] + ["--filter", "cross", "--method", "ransac8", "--iters", "100", "--seed", "3"],
                           capture_output=True, text=True, timeout=120)
    assert cross.returncode == 0, cross.stderr
    want = api.filter_cross(oracle.bf_knn_hamming(pad4(q), pad4(t), 1), oracle.bf_knn_hamming(pad4(t), pad4(q), 1))
    exp = oracle.format_match_list(want).splitlines()
    assert want.size > 100 and cross.stdout.splitlines()[:len(exp)] == exp


# ---- size limits (the pattern of test_tier7_hamming_across_the_staging_and_key_width_limits) ------------------------------

WIDE_PREFIXES = (4194175, 4194176, 4194303, 4194304, 4194400)


def wide_dma_ok(nt):
    """LDS-DMA staging of the 512-byte +-1 rows: 32-bit byte offsets over (nt + 128) rows."""
    return (nt + 128) * 512 < 2 ** 31 - 1


def test_wide_across_the_staging_and_key_width_limits(ctx, oracle, capsys):
    """One 4 194 400-row array of 64-byte rows and prefixes of it: (nt + 128) * 512 < 2^31 - 1 holds up to 4 194 175 rows
    (LDS-DMA staging), keys are (distance << 22 | row) below 2^22 = 4 194 304 rows and 64-bit from there on.  Plants in the
    last rows of every prefix; row nt - 4 is the complement of a query (distance 512: must come last, not first)."""
    import torch
    dev = torch.device("cuda", 0)
    assert wide_dma_ok(4194175) and not wide_dma_ok(4194176)
    free, _ = torch.cuda.mem_get_info()
    assert free >= 3 * 2 ** 30, "this test needs 3 GiB of free device memory, %.2f GiB are free" % (free / 2.0 ** 30)
    nt_all, nq, k = WIDE_PREFIXES[-1], 67, 2
    rng = np.random.default_rng(22)
    t = rng.integers(0, 256, (nt_all, 64), dtype=np.uint8)
    mem0 = _mem_used_mib()
    try:
        for nt in WIDE_PREFIXES:
            rows = sorted(set(interesting_rows(nt)) | {r for r in (2 ** 22 - 3, 2 ** 22 - 5) if r < nt - 4})
            rows = [r for r in rows if r != nt - 4]
            q = rng.integers(0, 256, (nq, 64), dtype=np.uint8)
            pl = Plants(nt, rng)
            pl.used |= set(range(nt - 4, nt_all))                # (rows past this prefix belong to the longer ones)
            n = pl.plant(q, t[:nt], near_bit, rows)
            assert n < nq - 1
            src = rng.integers(0, nt - 8, nq)
            for i in range(n, nq - 1, 2):
                q[i] = t[src[i]]
                q[i, :3] ^= np.uint8(0x21)
            t[nt - 4] = ~q[nq - 1]                               # the complement of the last query, in the last tile
            want = oracle.bf_knn_hamming(q, t[:nt], k, nthreads=THREADS)
            pl.check_oracle(want, "wide nt=%d" % nt)
            assert (want["trainIdx"][nq - 1] != nt - 4).all()
            d_t = torch.from_numpy(t).to(dev)                    # (the plants changed rows: upload again)
            d_q = torch.from_numpy(q).to(dev)
            try:
                for route in (0, 2):
                    ctx.set_option(api.PM_OPT_HAMMING_ROUTE, route)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got, ln = _launches(ctx, lambda: _dev_call(ctx, d_q, d_t, nq, nt, 64, k))
                    ms = (time.perf_counter() - t0) * 1e3
                    case = "wide hamming nt=%d route=%d" % (nt, route)
                    first = nt == WIDE_PREFIXES[0] and route == 0
                    _record(capsys, case, "i8-512" if ln["knn_hamming512_mfma_i8"] else "VALU", "-", ms, mem0 if first else None,
                            _mem_used_mib() if first else None)
                    assert ln["knn_hamming512_mfma_i8"] == 1 and ln["knn_hamming"] == 0, (case, ln)
                    assert_matches_equal(got, want, case)
            finally:
                ctx.set_option(api.PM_OPT_HAMMING_ROUTE, 0)
                del d_t, d_q
    finally:
        torch.cuda.empty_cache()
