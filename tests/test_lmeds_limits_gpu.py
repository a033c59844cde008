"""GPU: the 7-point + LMedS kernels and the adaptive 7-point RANSAC (csrc/lmeds.hip, docs/SPEC.md S13-S16) at their
limits.  Every case is bit-exact against the CPU oracle (winner id, median bits, F bits, mask, count), and where it
says so also checked against the independent fp64 reference of tests/lmeds_ref.py with the bounds stated there
(median within 2^-22 relative from 1e-6 px^2 up; mask equal outside |e - thr| <= 1e-5 * thr, at most 0.1 % of n inside).

  LDS sizes      n on both sides of 64 KiB of dynamic LDS (16122 is exactly 65536 bytes) and at the documented
                 maximum 32768 (132120 bytes); 32769 is refused
  ties           every correspondence two or three times: the even-n median pair v[n/2 - 1], v[n/2] ties bit for bit
                 (fewer than n/2 keys strictly below the pivot) or splits exactly, asserted on the fp64 reference
  per hypothesis one call per id: the answer is the best of at most three models, so every model's median shows
  non-finite     NaN / Inf rows in sampled and in scored positions; more than half the rows NaN
  device form    pm_lmeds_fundamental_dev: poisoned outputs, sentinel bytes, reuse across sizes, no-model outcomes
  adaptive       n = 65536 (no LDS key array, so no 32768 bound), partial / full / second batches of 512 ids

Measured on an MI355X (the figures each check prints): worst median difference 5.59e-8 relative against the bound
2^-22 = 2.38e-7 (the same value as the CPU oracle in tests/test_lmeds_independent_cpu.py: the results are equal bit
for bit); 0 correspondences in the border band and 0 mask disagreements outside it, in every case."""
import numpy as np
import pytest

import points_matching_amd as pm
from points_matching_amd.api import PM_E_NO_MODEL, PM_E_UNSUPPORTED, PM_OK, lmeds_fundamental, ransac7_adaptive
from test_lmeds_independent_cpu import (ADAPT_ITERS, ADAPT_THRESH, DEV_SIZES, DUP_CASES, LDS_SIZES, adaptive_case,
                                        adaptive_survivor_case, check_adaptive, check_independent, check_mostly_nan,
                                        check_poisoned, check_tie_side, dev_case, dup_case, lds_case, mostly_nan_case,
                                        poisoned_case, sweep)
from util import assert_lmeds_equal

pytestmark = pytest.mark.gpu

GUARD = 256


def _runner(ctx):
    return lambda x1, x2, hyp_end, seed, hyp_begin=0: lmeds_fundamental(ctx, x1, x2, hyp_end, seed, hyp_begin=hyp_begin)


def _both(ctx, oracle, x1, x2, hyp_end, seed, what, hyp_begin=0, nthreads=8):
    got = lmeds_fundamental(ctx, x1, x2, hyp_end, seed, hyp_begin=hyp_begin)
    want = oracle.lmeds_fundamental(x1, x2, hyp_end, seed, hyp_begin=hyp_begin, nthreads=nthreads)
    assert_lmeds_equal(got, want, what)
    return got


def _sweep_both(ctx, oracle, x1, x2, seed, what):
    def each(h, got):
        assert_lmeds_equal(got, oracle.lmeds_fundamental(x1, x2, h + 1, seed, hyp_begin=h), (what, h))
    return sweep(_runner(ctx), x1, x2, seed, what, each)


@pytest.mark.parametrize("n", LDS_SIZES)
def test_lds_sizes_around_64k_and_at_the_maximum(ctx, oracle, n):
    x1, x2, iters, seed = lds_case(n)
    check_independent(_both(ctx, oracle, x1, x2, iters, seed, n), x1, x2, "lds")


def test_one_correspondence_beyond_the_maximum_is_unsupported(ctx):
    z = np.zeros((32769, 2), np.float32)
    with pytest.raises(pm.PmError) as e:
        lmeds_fundamental(ctx, z, z, 10, 1)
    assert e.value.status == PM_E_UNSUPPORTED


@pytest.mark.parametrize("name", sorted(DUP_CASES))
def test_ties_at_the_median(ctx, oracle, name):
    x1, x2, iters, seed = dup_case(name)
    got = _both(ctx, oracle, x1, x2, iters, seed, name)
    check_independent(got, x1, x2, name)
    check_tie_side(got, x1, x2, name)
    _sweep_both(ctx, oracle, x1, x2, seed, name)


def test_per_hypothesis_at_the_largest_n(ctx, oracle):
    x1, x2, iters, seed = lds_case(32768)
    _sweep_both(ctx, oracle, x1, x2, seed, "n32768")


def test_non_finite_rows(ctx, oracle):
    got = check_poisoned(_runner(ctx), oracle.sample7)
    x1, x2, iters, seed, rows = poisoned_case()
    assert_lmeds_equal(got, oracle.lmeds_fundamental(x1, x2, iters, seed, nthreads=8), "poisoned")
    check_mostly_nan(_runner(ctx))
    x1, x2, iters, seed = mostly_nan_case()
    assert_lmeds_equal(lmeds_fundamental(ctx, x1, x2, iters, seed), oracle.lmeds_fundamental(x1, x2, iters, seed, nthreads=8),
                       "mostly NaN")


# ---- pm_lmeds_fundamental_dev ----------------------------------------------------------------------------------
def _run_dev(ctx, x1, x2, hyp_begin, hyp_end, seed):
    """The device form on torch-owned buffers, outputs poisoned, GUARD sentinel bytes behind the mask and sentinel
    doubles behind F.  Returns (F, mask, n_inliers, best_model, median)."""
    import torch
    dev = torch.device("cuda", 0)
    n = x1.shape[0]
    d1, d2 = torch.from_numpy(np.ascontiguousarray(x1)).to(dev), torch.from_numpy(np.ascontiguousarray(x2)).to(dev)
    F = torch.full((9 + 4,), 7.0, dtype=torch.float64, device=dev)
    m = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    c = torch.full((1 + 2,), 99, dtype=torch.int32, device=dev)
    b = torch.full((1 + 2,), 99, dtype=torch.int64, device=dev)
    med = torch.full((1 + 2,), 7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.lmeds_fundamental_dev(d1.data_ptr(), d2.data_ptr(), n, hyp_begin, hyp_end, seed, F.data_ptr(), m.data_ptr(),
                              c.data_ptr(), b.data_ptr(), med.data_ptr())
    ctx.synchronize()
    Fh, mh, ch, bh, medh = F.cpu().numpy(), m.cpu().numpy(), c.cpu().numpy(), b.cpu().numpy(), med.cpu().numpy()
    assert (mh[n:] == 0xA5).all() and (Fh[9:] == 7.0).all(), "bytes behind the mask / F were written"
    assert (ch[1:] == 99).all() and (bh[1:] == 99).all() and (medh[1:] == 7.0).all()
    return Fh[:9].reshape(3, 3).copy(), mh[:n].copy(), int(ch[0]), int(bh[0]), float(medh[0])


def _assert_dev_equals_host(dev, host, what):
    rc, F, mask, ninl, best, med = host
    if rc == PM_OK:
        assert_lmeds_equal((PM_OK,) + dev, host, what)
    else:                                             # the device form reports "no model" through its outputs
        assert rc == PM_E_NO_MODEL, what
        assert_lmeds_equal((rc,) + dev, (rc, np.zeros((3, 3)), np.zeros_like(mask), 0, -1, np.inf), what)


def test_device_form_equals_the_host_form(ctx, oracle):
    host = {}
    for n in DEV_SIZES:
        x1, x2, iters, seed = dev_case(n)
        host[n] = _both(ctx, oracle, x1, x2, iters, seed, ("host", n))
        assert host[n][0] == PM_OK
    # twice in a row, then after a larger and after a smaller n on the same context
    for n in (2275, 2275, 32768, 8, 9, 32768, 2275, 9):
        x1, x2, iters, seed = dev_case(n)
        _assert_dev_equals_host(_run_dev(ctx, x1, x2, 0, iters, seed), host[n], ("dev", n))
    # a sub-range with global model ids
    x1, x2, iters, seed = dev_case(2275)
    h = host[2275][4] // 3
    part = _run_dev(ctx, x1, x2, h, h + 1, seed)
    assert part[3] == host[2275][4]
    _assert_dev_equals_host(part, _both(ctx, oracle, x1, x2, h + 1, seed, "part", hyp_begin=h), "dev part")


def test_device_form_without_a_model(ctx, oracle):
    # every sample degenerate
    x1 = np.tile(np.float32([[10, 20]]), (50, 1))
    x2 = np.tile(np.float32([[11, 21]]), (50, 1))
    assert lmeds_fundamental(ctx, x1, x2, 30, 1)[0] == PM_E_NO_MODEL == oracle.lmeds_fundamental(x1, x2, 30, 1)[0]
    # an empty hypothesis range over a good input, and every median +inf
    y1, y2, iters, seed = dev_case(2275)
    z1, z2, ziters, zseed = mostly_nan_case()
    for a, b, hb, he, s in ((x1, x2, 0, 30, 1), (y1, y2, 5, 5, seed), (y1, y2, 0, 0, seed), (z1, z2, 0, ziters, zseed)):
        F, mask, ninl, best, med = _run_dev(ctx, a, b, hb, he, s)          # PM_OK: the wrapper raises otherwise
        assert (F.view(np.uint64) == 0).all() and not mask.any() and ninl == 0 and best == -1 and med == np.inf, (hb, he)
    # and the context still works
    _assert_dev_equals_host(_run_dev(ctx, y1, y2, 0, iters, seed), _both(ctx, oracle, y1, y2, iters, seed, "after"), "after")


# ---- adaptive-iteration RANSAC over the same models (SPEC S16) ------------------------------------------------------
def _adaptive_both(ctx, oracle, x1, x2, max_iters, thresh, seed):
    got = ransac7_adaptive(ctx, x1, x2, max_iters, 0.99, thresh, seed)
    want = oracle.ransac7_adaptive(x1, x2, max_iters, 0.99, thresh, seed)
    assert got[0] == want[0] and got[4] == want[4] and got[5] == want[5], (got[0], want[0], got[4:], want[4:])
    assert got[3] == want[3] and (got[2] == want[2]).all()
    assert (got[1].view(np.uint64) == want[1].view(np.uint64)).all()
    return got


@pytest.mark.parametrize("max_iters", ADAPT_ITERS)
def test_adaptive_beyond_the_lmeds_bound_and_across_batches(ctx, oracle, max_iters):
    x1, x2, seed = adaptive_case()
    assert x1.shape[0] == 65536
    got = _adaptive_both(ctx, oracle, x1, x2, max_iters, ADAPT_THRESH, seed)
    assert got[0] == PM_OK and got[5] == max_iters           # 70 % outliers: the budget never shrinks below the cap
    check_adaptive(got, x1, x2, (max_iters, ADAPT_THRESH))


def test_adaptive_winner_of_the_first_batch_survives_the_second(ctx, oracle):
    x1, x2, max_iters, thresh, seed = adaptive_survivor_case()
    got = _adaptive_both(ctx, oracle, x1, x2, max_iters, thresh, seed)
    assert got[0] == PM_OK and got[4] < 3 * 512 and got[5] > 512, got[4:]
    check_adaptive(got, x1, x2, (max_iters, thresh))
