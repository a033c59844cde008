"""GPU parity of the matchers on map-sized train sets: more than 131072 train rows, where the launch geometry changes form
(include/pm.h "Train-set size regimes", docs/SPEC.md S1b / S1c / S2).  The splits stop growing at 64, so a split holds more
than 16 (f16) or 32 (f32) tiles; the candidate id takes 10 .. 16 mantissa bits and the refinement window widens with it;
PM_KNN_HINT_U8 and the u8 entry points leave the u8 route; above 2 GiB of coarse copy the train tiles are staged through
registers; Hamming keys go from 32 to 64 bits at 2^23 rows; above 16 id bits the exact kernel (L2) or the VALU scan (Hamming)
takes the call.

Reference: the CPU oracle, every comparison bit for bit (indices and distance bit patterns).  Every case plants exact and
near-duplicate neighbours where the new arithmetic is (first and last tile, row nt - 1, both sides of a split boundary and
of 2^16 / 2^17 / 2^23, twins far apart, a run of identical rows inside one split) and checks ON THE ORACLE's answer that
the plants are what it found before the device result is compared.

Printed per case (not asserted): route, re-scans (knn_stats), wall time of the call, device memory in use.
The two largest tiers need free device memory (5.5 GiB for 16 777 216 x 4 floats, 11 GiB for 33 554 432 binary rows) and fail
with that message when it is not there."""
import time

import numpy as np
import pytest

import points_matching_amd as pm
from points_matching_amd import api
from test_cross_check_gpu import _check_one_call
from util import assert_matches_equal

pytestmark = pytest.mark.gpu

THREADS = 16
EXACT, F32, INTEGER, U8, UNIT = (api.PM_KNN_FORCE_EXACT, api.PM_KNN_FORCE_F32, api.PM_KNN_HINT_INTEGER, api.PM_KNN_HINT_U8,
                                 api.PM_KNN_HINT_UNIT_NORM)
FLAG_NAME = {0: "auto", EXACT: "exact", F32: "f32", INTEGER: "int-hint", U8: "u8-hint", UNIT: "unit-hint"}
ROUTE_NAME = {0: "f16 integer", 1: "f16 rounded", 2: "f32", 3: "u8"}
RUN_LEN = 48          # rows of the identical run: more than KNN_C groups of 4, 8 or 16 rows


# ---- the documented geometry (pm.h, SPEC S1b): 64 splits at most, whole tiles per split ---------------------------------

def split_rows(nt, tile):
    """Rows per split once the split count is capped at 64 (every nt >= 131072): ceil(tiles / 64) whole tiles."""
    ntiles = -(-nt // tile)
    assert -(-ntiles // (2048 // tile)) >= 64, "below the capped regime the split count depends on nq and the CU count"
    return -(-ntiles // 64) * tile


def id_bits(nt, tile):
    """Mantissa bits of the candidate id: a lane stream has rows_per_split / 8 row groups, times two lane halves."""
    ids = split_rows(nt, tile) // 8 * 2
    b = 4 if tile == 128 else 3
    while (1 << b) < ids:
        b += 1
    return b


def f16_dma_ok(nt):
    """LDS-DMA staging of the f16 copies: 32-bit byte offsets over (nt + 128) rows of 288 bytes."""
    return (nt + 128) * 288 < 2 ** 31 - 1


def i8_dma_ok(nt):
    return (nt + 128) * 256 < 2 ** 31 - 1


def interesting_rows(nt):
    rows = {0, 1, 3, 4, 127, 128, nt - 2, nt - 3, (nt - 1) // 128 * 128, (nt - 1) // 128 * 128 - 1}
    for tile in (128, 64):
        r = split_rows(nt, tile)
        for s in (1, 2, 31, 63):
            rows |= {s * r - 1, s * r}
    for p in (16, 17, 23):
        rows |= {2 ** p - 1, 2 ** p}
    return sorted(x for x in rows if 0 <= x < nt - 1 and x != 5)         # (5 and nt - 1 are the twins)


class Plants:
    """Writes the planted rows into (q, t) and remembers what the oracle must answer for them."""

    def __init__(self, nt, rng):
        self.nt, self.rng = nt, rng
        self.used = {5, nt - 1}
        self.first = {}                     # query -> train row that must come first
        self.pair = {}                      # query -> (first, second) where the second is determined too

    def _free_far(self, a, i):
        b = (a + self.nt // 2 + 641 * i + 13) % self.nt
        while b in self.used or b in self.reserved:
            b = (b + 1) % self.nt
        self.used.add(b)
        return b

    def plant(self, q, t, near, rows=None):
        """near(row_vector, strength) -> a slightly different row.  Returns the number of queries used."""
        nt, rng = self.nt, self.rng
        rows = interesting_rows(nt) if rows is None else rows
        self.reserved = set(rows)
        i = 0
        for a in rows:
            b = self._free_far(a, i)
            exact_row, near_row = (a, b) if rng.integers(0, 2) else (b, a)
            t[exact_row] = q[i]
            t[near_row] = near(q[i], 1 + i % 3)
            self.first[i] = exact_row
            self.pair[i] = (exact_row, near_row)
            self.used.add(a)
            i += 1
        # twins far apart: the lowest index wins, the other one is second at the same distance
        t[5] = q[i]
        t[nt - 1] = q[i]
        self.first[i] = 5
        self.pair[i] = (5, nt - 1)
        i += 1
        # a run of identical best rows inside one split of either geometry
        r0 = 17 * split_rows(nt, 128) + 200
        while r0 // split_rows(nt, 64) != (r0 + RUN_LEN - 1) // split_rows(nt, 64) or any(r in self.used for r in range(r0, r0 + RUN_LEN)):
            r0 += RUN_LEN
        assert r0 // split_rows(nt, 128) == (r0 + RUN_LEN - 1) // split_rows(nt, 128) and r0 + RUN_LEN < nt
        t[r0:r0 + RUN_LEN] = q[i]
        self.used |= set(range(r0, r0 + RUN_LEN))
        self.first[i] = r0
        self.pair[i] = (r0, r0 + 1)
        i += 1
        return i

    def check_oracle(self, want, what):
        """The conditions that keep a case from passing vacuously, on the oracle's answer alone."""
        k = want.shape[1]
        for qi, row in self.first.items():
            assert want["trainIdx"][qi, 0] == row, "%s: planted query %d: the oracle found %d, not %d" % (
                what, qi, want["trainIdx"][qi, 0], row)
        if k >= 2:
            for qi, (a, b) in self.pair.items():
                assert want["trainIdx"][qi, 1] == b, "%s: planted query %d: second neighbour %d, not %d" % (
                    what, qi, want["trainIdx"][qi, 1], b)
            for tile in (128, 64):
                r = split_rows(self.nt, tile)
                apart = (want["trainIdx"][:, 0] // r) != (want["trainIdx"][:, 1] // r)
                assert apart.sum() >= len(self.first) // 2, "%s: too few queries with neighbours in different splits" % what


def near_int(row, strength):
    out = row.copy()
    out[strength] = out[strength] + 1 if out[strength] < 128 else out[strength] - 1
    return out


def near_ulps(row, strength):
    """A few f32 ulps on three elements: below the f16 resolution and far below any widened window."""
    out = row.copy()
    idx = np.array([0, len(row) // 2, len(row) - 1])
    out[idx] = out[idx] * np.float32(1.0 + 1.2e-7 * (strength + 1))
    assert (out != row).any()
    return out


def near_bit(row, strength):
    out = row.copy()
    out[strength] ^= np.uint8(1 << strength)
    return out


def make_int_case(nq, nt, dim, seed, hi=256, as_u8=False):
    """u8-valued (or small-integer) rows generated as uint8; half of the free queries are noisy copies of train rows."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, hi, (nt, dim), dtype=np.uint8)
    q = rng.integers(0, hi, (nq, dim), dtype=np.uint8)
    pl = Plants(nt, rng)
    if hi < 256:
        # tie-heavy alphabet: the planted queries live outside it (values hi + 3 * digit), so that their plants stay
        # the unique best rows; every other query ties with many train rows at the same distance
        n_pl = len(interesting_rows(nt)) + 2
        digits = (np.arange(n_pl)[:, None] // 5 ** np.arange(dim)[None, :]) % 5
        assert n_pl <= 5 ** dim
        q[:n_pl] = (hi + 3 * digits).astype(np.uint8)
    n = pl.plant(q, t, near_int)
    src = rng.integers(0, nt, nq)
    for i in range(n, nq, 2):
        row = t[src[i]].copy()
        sel = rng.integers(0, dim, max(1, dim // 10))
        row[sel] = rng.integers(0, hi, sel.size, dtype=np.uint8)
        q[i] = row
    if as_u8:
        return q, t, pl
    return q.astype(np.float32), t.astype(np.float32), pl


def make_float_case(nq, nt, dim, seed, unit=True):
    """General floats generated as float32 (SURF-like: unit-norm rows)."""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((nt, dim), dtype=np.float32)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    if unit:
        t /= np.linalg.norm(t, axis=1, keepdims=True)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    pl = Plants(nt, rng)
    n = pl.plant(q, t, near_ulps)
    src = rng.integers(0, nt, nq)
    for i in range(n, nq, 2):
        row = t[src[i]] + np.float32(0.02) * rng.standard_normal(dim, dtype=np.float32)
        q[i] = row / np.linalg.norm(row) if unit else row
    return q, t, pl


# ---- running and recording -----------------------------------------------------------------------------------------------

def _mem_used_mib():
    import torch
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 2.0 ** 20


def _record(capsys, case, route, rescans, ms, mem_before=None, mem_after=None):
    line = "large-train | %-44s | %-11s | rescans %7s | %9.2f ms" % (case, route, rescans, ms)
    if mem_before is not None:
        line += " | device memory in use %.0f -> %.0f MiB" % (mem_before, mem_after)
    with capsys.disabled():
        print("\n" + line, end="", flush=True)


def _records(d_out, nq, k):
    return d_out.cpu().numpy().view(pm.MATCH_DTYPE).reshape(nq, k)


def _knn_dev(ctx, d_q, d_t, k, flags, u8=False):
    """One device-pointer matcher call; returns (records, stats, milliseconds).  A status other than PM_OK raises."""
    import torch
    nq, dim = d_q.shape
    nt = d_t.shape[0]
    d_out = torch.full((nq, k, 4), -5, dtype=torch.int32, device=d_q.device)
    torch.cuda.synchronize()
    ctx.knn_diag_enable(True)
    try:
        t0 = time.perf_counter()
        if u8:
            ctx.bf_knn_l2_u8_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, dim, k, d_out.data_ptr())
        else:
            ctx.bf_knn_l2_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, dim, k, d_out.data_ptr(), flags)
        ctx.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        st = ctx.knn_stats()
    finally:
        ctx.knn_diag_enable(False)
    return _records(d_out, nq, k), st, ms


def _is_fast(nt, dim, k, flags):
    """The exact kernel takes the call when it is forced, for k > 4 and beyond 16 id bits (pm.h)."""
    if flags & EXACT or k > 4 or dim > 256:
        return False
    tile = 64 if flags & F32 else 128
    if flags & F32 and (dim % 4 or dim > 128):
        return False
    return id_bits(nt, tile) <= 16


def run_l2_case(ctx, oracle, capsys, name, q, t, pl, ks, flag_list, expect_route=None, first_of_tier=False, wrong_hints=(),
                want=None):
    """Oracle first (and its vacuity checks), then every (flags, k) on the device against it.  wrong_hints: flags whose
    premise the data break (they may only cost time: the device reports them through `nonfinite`)."""
    import torch
    dev = torch.device("cuda", 0)
    nq, dim = q.shape
    nt = t.shape[0]
    kmax = max(ks)
    if want is None:
        want = oracle.bf_knn_l2(q, t, kmax, nthreads=THREADS)     # the k-NN list is a prefix of the (k+1)-NN list (S3)
        pl.check_oracle(want, name)
    mem0 = _mem_used_mib()
    d_q, d_t = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
    try:
        for fi, flags in enumerate(flag_list):
            for k in ks:
                got, st, ms = _knn_dev(ctx, d_q, d_t, k, flags)
                fast = _is_fast(nt, dim, k, flags)
                case = "%s %s k=%d" % (name, FLAG_NAME[flags], k)
                show_mem = first_of_tier and fi == 0 and k == ks[0]
                _record(capsys, case, ROUTE_NAME[st["route"]] if fast else "exact", st["rescans"] if fast else "-", ms,
                        mem0 if show_mem else None, _mem_used_mib() if show_mem else None)
                assert_matches_equal(got, np.ascontiguousarray(want[:, :k]), case)
                if fast:
                    assert st["nonfinite"] == (1 if flags in wrong_hints else 0), (case, st)
                    if expect_route is not None and flags in expect_route:
                        assert st["route"] == expect_route[flags], (case, st)
    finally:
        del d_q, d_t
        torch.cuda.empty_cache()
    return want


# ---- tier 1: both sides of the 9-bit regime ------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["u8valued", "floats"])
@pytest.mark.parametrize("nt", [131072, 131073])
def test_tier1_boundary_of_the_9_bit_regime(ctx, oracle, capsys, nt, kind):
    """131072 rows: 64 splits of 16 f16 tiles, 9 id bits, the u8 route still applies.  131073: 17 tiles per split, 10 bits,
    PM_KNN_HINT_U8 is served by the f16 integer route."""
    assert id_bits(131072, 128) == 9 and id_bits(131073, 128) == 10 and split_rows(131073, 128) == 17 * 128
    nq, dim = 701, 128
    if kind == "u8valued":
        q, t, pl = make_int_case(nq, nt, dim, seed=nt)
        # the rule of the code: the u8 route's integer candidates leave 9 bits for the id
        expect = {U8: 3 if id_bits(nt, 128) <= 9 else 0, INTEGER: 0, 0: 0, F32: 2}
        wrong = (UNIT,)
    else:
        q, t, pl = make_float_case(nq, nt, dim, seed=nt + 1)
        expect = {0: 1, UNIT: 1, F32: 2}
        wrong = (INTEGER, U8)
    # every flag on both kinds of data: a hint that does not hold (integer hints on floats, the unit-norm hint on u8
    # values) may only cost time
    run_l2_case(ctx, oracle, capsys, "t1 %s nt=%d" % (kind, nt), q, t, pl, (1, 2, 4), (0, INTEGER, U8, F32, UNIT, EXACT),
                expect_route=expect, first_of_tier=True, wrong_hints=wrong)


# ---- tier 2: 300 001 rows, 11 id bits ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,kind", [(128, "u8valued"), (64, "floats"), (30, "floats"), (200, "u8valued")])
def test_tier2_300001_rows(ctx, oracle, capsys, dim, kind):
    nt, nq = 300001, 1003
    assert id_bits(nt, 128) == 11 and id_bits(nt, 64) == 11
    if kind == "u8valued":
        q, t, pl = make_int_case(nq, nt, dim, seed=dim)
        flag_list = (0, INTEGER, U8, EXACT) + ((F32,) if dim <= 128 else ())
        expect = {0: 0, INTEGER: 0, U8: 0, F32: 2}
    else:
        q, t, pl = make_float_case(nq, nt, dim, seed=dim)
        flag_list = (0, UNIT, EXACT) + ((F32,) if dim % 4 == 0 else ())
        expect = {0: 1, UNIT: 1, F32: 2}
    if dim % 4 or dim > 128:
        expect.pop(F32, None)
    run_l2_case(ctx, oracle, capsys, "t2 %s dim=%d" % (kind, dim), q, t, pl, (2, 4) if dim == 128 else (2,), flag_list,
                expect_route=expect, first_of_tier=dim == 128)


# ---- tier 3: 1 200 000 rows, 13 id bits; the u8 entry points and the fused ratio forms -------------------------------

def _ratio_calls(ctx, oracle, capsys, name, d_q, d_t, want_knn, u8, flags):
    import torch
    dev = d_q.device
    nq, dim = d_q.shape
    nt = d_t.shape[0]
    rng = np.random.default_rng(nq + nt)
    kp1 = (rng.random((nq, 2)) * 900).astype(np.float32)
    kp2 = (rng.random((nt, 2)) * 600).astype(np.float32)
    d_kp1, d_kp2 = torch.from_numpy(kp1).to(dev), torch.from_numpy(kp2).to(dev)
    want = oracle.filter_ratio(want_knn, 0.8)
    assert 0 < want.size < nq, "vacuous ratio case"
    for fusion in (0, 1, 2):
        d_knn = torch.zeros((nq, 2, 4), dtype=torch.int32, device=dev)
        d_good = torch.full((nq, 4), -7, dtype=torch.int32, device=dev)
        d_xy1 = torch.full((nq, 2), -1.0, dtype=torch.float32, device=dev)
        d_xy2 = torch.full((nq, 2), -1.0, dtype=torch.float32, device=dev)
        d_n = torch.full((1,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.set_option(api.PM_OPT_FILTER_FUSION, fusion)
        try:
            t0 = time.perf_counter()
            tail = (0.8, d_kp1.data_ptr(), d_kp2.data_ptr(), d_knn.data_ptr(), d_good.data_ptr(), d_xy1.data_ptr(),
                    d_xy2.data_ptr(), d_n.data_ptr())
            if u8:
                ctx.bf_knn_l2_u8_ratio_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, dim, *tail)
            else:
                ctx.bf_knn_l2_ratio_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, dim, flags, *tail)
            ctx.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
        finally:
            ctx.set_option(api.PM_OPT_FILTER_FUSION, 0)
        case = "%s ratio %s fusion=%d" % (name, "u8 rows" if u8 else FLAG_NAME[flags], fusion)
        _record(capsys, case, "-", "-", ms)
        n = int(d_n.item())
        assert n == want.size, case
        assert ctx.filter_fusion_gave_up() == 0, case
        assert_matches_equal(d_good.cpu().numpy().view(pm.MATCH_DTYPE).reshape(-1)[:n], want, case + " good list")
        assert np.array_equal(d_xy1.cpu().numpy()[:n], kp1[want["queryIdx"]]), case
        assert np.array_equal(d_xy2.cpu().numpy()[:n], kp2[want["trainIdx"]]), case
        assert_matches_equal(_records(d_knn, nq, 2), want_knn, case + " records")


@pytest.mark.parametrize("dim,kind", [(64, "floats"), (128, "u8valued")])
def test_tier3_1200000_rows(ctx, oracle, capsys, dim, kind):
    import torch
    dev = torch.device("cuda", 0)
    nt, nq = 1200001, 515
    assert id_bits(nt, 128) == 13 and id_bits(nt, 64) == 13
    name = "t3 %s dim=%d" % (kind, dim)
    if kind == "floats":
        q, t, pl = make_float_case(nq, nt, dim, seed=3)
        want = run_l2_case(ctx, oracle, capsys, name, q, t, pl, (2,), (0, UNIT, F32, EXACT), expect_route={0: 1, UNIT: 1, F32: 2},
                           first_of_tier=True)
        d_q, d_t = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
        _ratio_calls(ctx, oracle, capsys, name, d_q, d_t, want, False, 0)
        del d_q, d_t
        torch.cuda.empty_cache()
        return
    q8, t8, pl = make_int_case(nq, nt, dim, seed=4, as_u8=True)
    q, t = q8.astype(np.float32), t8.astype(np.float32)
    want4 = run_l2_case(ctx, oracle, capsys, name, q, t, pl, (2, 4), (0, INTEGER, U8, F32, EXACT),
                        expect_route={0: 0, INTEGER: 0, U8: 0, F32: 2})
    want = np.ascontiguousarray(want4[:, :2])
    d_q, d_t = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
    _ratio_calls(ctx, oracle, capsys, name, d_q, d_t, want, False, U8)
    del d_q, d_t, q, t
    torch.cuda.empty_cache()
    # true u8 rows: pm_bf_knn_l2_u8_dev widens them on the device and re-enters on the f16 integer route
    d_q8, d_t8 = torch.from_numpy(q8).to(dev), torch.from_numpy(t8).to(dev)
    mem0 = _mem_used_mib()
    for k in (1, 2, 4):
        got, st, ms = _knn_dev(ctx, d_q8, d_t8, k, 0, u8=True)
        _record(capsys, "%s u8 rows k=%d" % (name, k), ROUTE_NAME[st["route"]], st["rescans"], ms, mem0 if k == 1 else None,
                _mem_used_mib() if k == 1 else None)
        assert_matches_equal(got, np.ascontiguousarray(want4[:, :k]), "u8 rows k=%d" % k)
        assert st["route"] == 0 and st["nonfinite"] == 0, st
    _ratio_calls(ctx, oracle, capsys, name, d_q8, d_t8, want, True, 0)
    assert_matches_equal(ctx.bf_knn_l2_u8(q8[:40], t8, 2), want[:40], "host form")


# ---- tier 4: across the 2 GiB limit of the LDS-DMA staging -----------------------------------------------------------

@pytest.mark.parametrize("kind", ["integers", "floats"])
@pytest.mark.parametrize("nt", [7456000, 7456412, 7456413, 7457000])
def test_tier4_across_the_staging_limit(ctx, oracle, capsys, nt, kind):
    """(nt + 128) * 288 < 2^31 - 1 holds up to nt = 7 456 412: up to there the f16 copies are staged by LDS-DMA, above through
    registers.  Same records on both sides; PM_OPT_KNN_STAGING = 1 (registers) below the limit and PM_OPT_KNN_SEEDED = 2
    above it (the seeded kernel: LDS-DMA only, but on 256-byte rows of its own, which still fit) change nothing."""
    assert f16_dma_ok(7456412) and not f16_dma_ok(7456413)
    nq, dim = 259, 4
    if kind == "integers":
        q, t, pl = make_int_case(nq, nt, dim, seed=nt, hi=16)       # 65536 distinct rows: ties everywhere
        flag_list, expect = (0, INTEGER, EXACT), {0: 0, INTEGER: 0}
    else:
        q, t, pl = make_float_case(nq, nt, dim, seed=nt, unit=False)
        flag_list, expect = (0, EXACT), {0: 1}
    name = "t4 %s nt=%d" % (kind, nt)
    want = run_l2_case(ctx, oracle, capsys, name, q, t, pl, (2,), flag_list, expect_route=expect, first_of_tier=nt == 7456000)
    opt, val = (api.PM_OPT_KNN_STAGING, 1) if f16_dma_ok(nt) else (api.PM_OPT_KNN_SEEDED, 2)
    ctx.set_option(opt, val)
    try:
        run_l2_case(ctx, oracle, capsys, name + (" staging=1" if f16_dma_ok(nt) else " seeded=2"), q, t, pl, (2,),
                    (INTEGER,) if kind == "integers" else (0,), expect_route=expect, want=want)
    finally:
        ctx.set_option(opt, 0)


# ---- tier 5: across the exact fall-back ------------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", [16777216, 16777217])
def test_tier5_across_the_exact_fallback(ctx, oracle, capsys, nt):
    """16 777 216 rows: 16 id bits, the last size of the matrix-core routes (4.8 GB of f16 copy).  One row more: 17 bits,
    the whole call goes to the exact kernel."""
    import torch
    assert id_bits(16777216, 128) == 16 and id_bits(16777217, 128) == 17
    assert id_bits(16777216, 64) == 16 and id_bits(16777217, 64) == 17
    free, _ = torch.cuda.mem_get_info()
    assert free >= 5.5 * 2 ** 30, "this tier needs 5.5 GiB of free device memory, %.2f GiB are free" % (free / 2.0 ** 30)
    nq, dim = 131, 4
    q, t, pl = make_int_case(nq, nt, dim, seed=5, hi=16)
    want = run_l2_case(ctx, oracle, capsys, "t5 integers nt=%d" % nt, q, t, pl, (2,), (0, INTEGER, F32, EXACT),
                       expect_route={0: 0, INTEGER: 0, F32: 2} if nt == 16777216 else None, first_of_tier=True)
    # PM_OPT_KNN_SEEDED = 2 names a kernel that exists with LDS-DMA staging only (its 256-byte rows pass 2 GiB above
    # 8 388 352 train rows): the launcher has to route round it here, with the same records and the status PM_OK
    ctx.set_option(api.PM_OPT_KNN_SEEDED, 2)
    try:
        run_l2_case(ctx, oracle, capsys, "t5 integers nt=%d seeded=2" % nt, q, t, pl, (2,), (INTEGER,), want=want,
                    expect_route={INTEGER: 0} if nt == 16777216 else None)
    finally:
        ctx.set_option(api.PM_OPT_KNN_SEEDED, 0)
    del q, t
    q, t, pl = make_float_case(nq, nt, dim, seed=6, unit=False)
    run_l2_case(ctx, oracle, capsys, "t5 floats nt=%d" % nt, q, t, pl, (2,), (0,), expect_route={0: 1} if nt == 16777216 else None)


# ---- Hamming --------------------------------------------------------------------------------------------------------------

def make_hamming_case(nq, nt, nbytes, seed, rows=None):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (nt, nbytes), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, nbytes), dtype=np.uint8)
    pl = Plants(nt, rng)
    n = pl.plant(q, t, near_bit, rows)
    src = rng.integers(0, nt, nq)
    for i in range(n, nq, 2):
        row = t[src[i]].copy()
        row[rng.integers(0, nbytes, 4)] ^= np.uint8(0x11)
        q[i] = row
    return q, t, pl


def _hamming_dev(ctx, d_q, d_t, nt, k):
    import torch
    nq, nbytes = d_q.shape
    d_out = torch.full((nq, k, 4), -5, dtype=torch.int32, device=d_q.device)
    torch.cuda.synchronize()
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        t0 = time.perf_counter()
        ctx.bf_knn_hamming_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, nbytes, k, d_out.data_ptr())
        ctx.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        i8 = ctx.timing_get("knn_hamming_mfma_i8")[1] > 0
    finally:
        ctx.timing_enable(False)
    return _records(d_out, nq, k), "i8" if i8 else "VALU", ms


@pytest.mark.parametrize("nbytes,k,route", [(32, 1, "i8"), (32, 2, "i8"), (64, 3, "VALU"), (32, 5, "VALU")])
def test_tier6_hamming_300001_rows(ctx, oracle, capsys, nbytes, k, route):
    import torch
    dev = torch.device("cuda", 0)
    nt, nq = 300001, 517
    vrows = -(-nt // 32)                                         # the VALU scan: 32 splits of ceil(nt / 32) rows
    rows = sorted(set(interesting_rows(nt)) | {vrows - 1, vrows, 31 * vrows - 1, 31 * vrows})
    q, t, pl = make_hamming_case(nq, nt, nbytes, seed=nbytes + k, rows=rows)
    want = oracle.bf_knn_hamming(q, t, k, nthreads=THREADS)
    pl.check_oracle(want, "t6")
    mem0 = _mem_used_mib()
    d_q, d_t = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
    got, took, ms = _hamming_dev(ctx, d_q, d_t, nt, k)
    _record(capsys, "t6 hamming %dB k=%d" % (nbytes, k), took, "-", ms, mem0, _mem_used_mib())
    assert took == route
    assert_matches_equal(got, want, "t6 hamming %dB k=%d" % (nbytes, k))


HAMMING_PREFIXES = (8388479, 8388480, 8388607, 8388608, 8388900)
HAMMING_PREFIXES_VALU = (2 ** 25, 2 ** 25 + 200)


def hamming_i8_ok(nt):
    """The matrix-core route's candidate holds 16 id bits; a split has rows_per_split / 16 row groups per lane half, times two
    halves.  Beyond 2^16 ids the VALU scan takes the call."""
    return split_rows(nt, 128) // 8 <= 2 ** 16


def _hamming_prefixes(ctx, oracle, capsys, name, prefixes, nq, seed, extra_rows=()):
    """One train array of prefixes[-1] rows and its prefixes, ascending (a prefix's plants lie inside every longer one).
    PM_OPT_HAMMING_ROUTE 0 / 2 (32- or 64-bit keys as the size asks / 64-bit keys) x PM_OPT_HAMMING_REFINE 0 / 1."""
    import torch
    dev = torch.device("cuda", 0)
    nt_all, k = prefixes[-1], 2
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (nt_all, 32), dtype=np.uint8)
    mem0 = _mem_used_mib()
    try:
        for nt in prefixes:
            rows = sorted(set(interesting_rows(nt)) | {r for r in extra_rows if r < nt - 1})
            q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
            pl = Plants(nt, rng)
            pl.used |= set(range(nt - 4, nt_all))                # (rows past this prefix belong to the longer ones)
            n = pl.plant(q, t[:nt], near_bit, rows)
            assert n < nq
            src = rng.integers(0, nt, nq)
            for i in range(n, nq, 2):
                q[i] = t[src[i]]
                q[i, :3] ^= np.uint8(0x21)
            want = oracle.bf_knn_hamming(q, t[:nt], k, nthreads=THREADS)
            pl.check_oracle(want, "%s nt=%d" % (name, nt))
            d_t = torch.from_numpy(t).to(dev)                    # (the plants changed rows: upload again)
            d_q = torch.from_numpy(q).to(dev)
            try:
                for route in (0, 2):
                    for refine in (0, 1):
                        ctx.set_option(api.PM_OPT_HAMMING_ROUTE, route)
                        ctx.set_option(api.PM_OPT_HAMMING_REFINE, refine)
                        got, took, ms = _hamming_dev(ctx, d_q, d_t, nt, k)
                        case = "%s hamming nt=%d route=%d refine=%d" % (name, nt, route, refine)
                        first = nt == prefixes[0] and route == 0 and refine == 0
                        _record(capsys, case, took, "-", ms, mem0 if first else None, _mem_used_mib() if first else None)
                        assert took == ("i8" if hamming_i8_ok(nt) else "VALU"), case
                        assert_matches_equal(got, want, case)
            finally:
                ctx.set_option(api.PM_OPT_HAMMING_ROUTE, 0)
                ctx.set_option(api.PM_OPT_HAMMING_REFINE, 0)
                del d_t, d_q
    finally:
        torch.cuda.empty_cache()


def test_tier7_hamming_across_the_staging_and_key_width_limits(ctx, oracle, capsys):
    """One 8 388 900-row array and prefixes of it: (nt + 128) * 256 < 2^31 - 1 holds up to 8 388 479 rows (LDS-DMA staging of
    the +-1 byte copies), keys are (distance << 23 | row) below 2^23 = 8 388 608 rows and 64-bit from there on."""
    assert i8_dma_ok(8388479) and not i8_dma_ok(8388480)
    assert all(hamming_i8_ok(nt) for nt in HAMMING_PREFIXES)
    _hamming_prefixes(ctx, oracle, capsys, "t7", HAMMING_PREFIXES, 131, seed=7, extra_rows=(2 ** 23 - 3, 2 ** 23 - 4))


def test_tier8_hamming_across_the_return_to_the_valu_scan(ctx, oracle, capsys):
    """33 554 432 rows: 4096 tiles per split, 2^16 candidate ids, the last size of the matrix-core route (8.6 GB of +-1 byte
    copies).  200 rows more: the call returns to the VALU scan."""
    import torch
    assert hamming_i8_ok(2 ** 25) and not hamming_i8_ok(2 ** 25 + 1)
    free, _ = torch.cuda.mem_get_info()
    assert free >= 11 * 2 ** 30, "this tier needs 11 GiB of free device memory, %.2f GiB are free" % (free / 2.0 ** 30)
    _hamming_prefixes(ctx, oracle, capsys, "t8", HAMMING_PREFIXES_VALU, 67, seed=8)


# ---- cross-check: a map-sized train set is a map-sized QUERY set of the reverse pass ---------------------------------------

def _cross_data(route, n_small, n_big, seed):
    """n_small rows that are mostly noisy copies of distinct rows of the big set (mutual neighbours), the rest random."""
    rng = np.random.default_rng(seed)
    src = rng.permutation(n_big)[:n_small]
    if route == "f32":
        big = rng.standard_normal((n_big, 32), dtype=np.float32)
        small = big[src] + np.float32(0.05) * rng.standard_normal((n_small, 32), dtype=np.float32)
        small[::3] = rng.standard_normal((len(small[::3]), 32), dtype=np.float32)
    elif route == "u8":
        big = rng.integers(0, 256, (n_big, 32), dtype=np.uint8)
        small = big[src].copy()
        small[:, ::7] = rng.integers(0, 256, small[:, ::7].shape, dtype=np.uint8)
        small[::3] = rng.integers(0, 256, small[::3].shape, dtype=np.uint8)
    else:
        big = rng.integers(0, 256, (n_big, 32), dtype=np.uint8)
        small = big[src].copy()
        small[:, :2] ^= np.uint8(0x5A)
        small[::3] = rng.integers(0, 256, small[::3].shape, dtype=np.uint8)
    # plants at the rows where the id arithmetic of the big side changes: exact copies, and one pair of twins
    rows = interesting_rows(n_big)
    for i, r in enumerate(rows):
        big[r] = small[3 * i + 1]
    big[5] = small[3 * len(rows) + 1]
    big[n_big - 1] = small[3 * len(rows) + 1]
    return small, big


@pytest.mark.parametrize("route", ["f32", "u8", "hamming"])
def test_cross_check_map_sized_both_shapes(ctx, oracle, capsys, route):
    """3000 x 300001 and 300001 x 3000: forward and reverse records, survivors, gathered points (the helper of
    test_cross_check_gpu.py, which also guards 0 < survivors < nq)."""
    import torch
    n_small, n_big = 3000, 300001
    small, big = _cross_data(route, n_small, n_big, seed=9)
    binary = route == "hamming"
    flag_set = (0, api.PM_CROSS_RATIO_FWD | api.PM_CROSS_RATIO_REV)
    key = "large_%s_%dx%d" % (route, n_small, n_big)
    mem0 = _mem_used_mib()
    t0 = time.perf_counter()
    _check_one_call(ctx, oracle, key, route, small, big, flag_set=flag_set, binary=binary)
    _record(capsys, "cross %s %d x %d (oracle included)" % (route, n_small, n_big), "-", "-", (time.perf_counter() - t0) * 1e3,
            mem0, _mem_used_mib())
    key_t = "large_%s_%dx%d" % (route, n_big, n_small)
    try:
        t0 = time.perf_counter()
        _check_one_call(ctx, oracle, key_t, route, big, small, flag_set=flag_set, binary=binary)
        _record(capsys, "cross %s %d x %d (oracle included)" % (route, n_big, n_small), "-", "-", (time.perf_counter() - t0) * 1e3)
    finally:
        torch.cuda.empty_cache()
