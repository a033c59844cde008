"""The LMedS scoring rule (docs/SPEC.md S15) against an independent fp64 reference (tests/lmeds_ref.py: textbook
symmetric epipolar residual by numpy matrix products, np.sort medians, robust sigma, mask), not against the C oracle
that is written from the same SPEC paragraph.  Here the C oracle stands in for the device, at every size and input
family of tests/test_lmeds_limits_gpu.py, which proves the reference and its tolerances without a GPU; the GPU module
imports the cases and the checks below and runs them on the HIP kernels.

Bounds (lmeds_ref.py): reported median within 2^-22 relative of the fp64 median wherever that is >= 1e-6 px^2; mask
equal to the fp64 one outside |e - thr| <= 1e-5 * thr, a band that may hold at most 0.1 % of the correspondences.

Measured (worst over every case of this module / of the GPU module, which covers the same cases):
  CPU oracle   median: 5.59e-8 relative (bound 2.38e-7); border band: 0 correspondences in every case; 0 mask
               disagreements outside it
  MI355X       median: 5.59e-8 relative, the same cases bit for bit; border band: 0; 0 disagreements"""
import numpy as np
import pytest

import lmeds_ref as R
from points_matching_amd import synth

PM_OK, PM_E_NO_MODEL = 0, -3

LDS_SIZES = (16121, 16122, 16123, 32767, 32768)      # 4 * (n + 262) bytes of LDS: 65532, 65536, 65540, ..., 132120
DEV_SIZES = (8, 9, 2275, 32768)
SWEEP = range(200)

# name -> (distinct correspondences, copies of each, extra single rows, median pair ties?)  With every residual
# present `copies` times, the sorted keys are runs of equal values; v[n/2 - 1] and v[n/2] lie in one run (a tie: fewer
# than n/2 keys are strictly below v[n/2]) or in two neighbouring runs (exactly n/2 are).  None: n is odd.
DUP_CASES = {
    "x2_n2000": (1000, 2, 0, False),                 # n/2 = 1000 even: keys 999 | 1000 belong to pairs 499 | 500
    "x2_n2002": (1001, 2, 0, True),                  # n/2 = 1001 odd: keys 1000, 1001 are both pair 500
    "x3_n1998": (666, 3, 0, False),                  # keys 998 | 999: triples 332 | 333
    "x3_n2001": (667, 3, 0, None),                   # odd n: the rank falls inside a run of three
    "x2p1_n2001": (1000, 2, 1, None),
    "x3p1_n2002": (667, 3, 1, True),                 # keys 1000, 1001: one triple wherever the single row falls
}


def lds_case(n):
    x1, x2, _, _ = synth.two_view(n, seed=3 * n + 1, outlier_frac=0.3, noise_px=0.5)
    return x1, x2, 300, 0x15D5 + n


def dev_case(n):
    if n <= 9:
        x1, x2, _, _ = synth.two_view(n, seed=50 + n, outlier_frac=0.0, noise_px=0.0)
        return x1, x2, 40, 0xD0 + n
    if n == 32768:
        return lds_case(n)
    x1, x2, _, _ = synth.two_view(n, seed=50 + n, outlier_frac=0.4, noise_px=1.0)
    return x1, x2, 300, 0xD0 + n


def dup_case(name):
    base, copies, extra, _ = DUP_CASES[name]
    x1, x2, _, _ = synth.two_view(base + extra, seed=base + 7 * copies + extra, outlier_frac=0.3, noise_px=0.5)
    x1 = np.concatenate([np.repeat(x1[:base], copies, axis=0), x1[base:]])
    x2 = np.concatenate([np.repeat(x2[:base], copies, axis=0), x2[base:]])
    perm = np.random.default_rng(base + copies).permutation(x1.shape[0])
    return np.ascontiguousarray(x1[perm]), np.ascontiguousarray(x2[perm]), 300, 0xD0B1E + copies


def poisoned_case(n=2000, frac=0.05):
    """`frac` of the rows get NaN, +Inf or -Inf in one coordinate of one image.  Returns also the poisoned rows."""
    x1, x2, _, _ = synth.two_view(n, seed=977, outlier_frac=0.3, noise_px=0.5)
    rows = np.random.default_rng(5).choice(n, int(frac * n), replace=False)
    for j, r in enumerate(rows):
        (x1, x2)[j & 1][r, (j >> 1) & 1] = (np.nan, np.inf, -np.inf)[j % 3]
    return x1, x2, 300, 0xBAD, np.sort(rows)


def mostly_nan_case(n=2000):
    """55 % of the rows of image 2 are NaN: more than half of every model's residuals are +inf, so is every median."""
    x1, x2, _, _ = synth.two_view(n, seed=978, outlier_frac=0.3, noise_px=0.5)
    rows = np.random.default_rng(6).choice(n, int(0.55 * n), replace=False)
    x2[rows] = np.nan
    return x1, x2, 300, 0xBAD2


ADAPT_N = 65536
ADAPT_ITERS = (511, 512, 513, 1024)                  # batches of 512 ids: partial, full, full + 1, two full
ADAPT_THRESH = 0.5


def adaptive_case():
    x1, x2, _, _ = synth.two_view(ADAPT_N, seed=65536, outlier_frac=0.7, noise_px=0.5)
    return x1, x2, 0xADA7


def adaptive_survivor_case():
    """The winner is found among the first 512 ids and the budget stays above 512: a second batch runs and must not
    replace it (seed and sizes chosen with the CPU oracle; the tests assert both properties)."""
    x1, x2, _, _ = synth.two_view(3000, seed=31, outlier_frac=0.6, noise_px=0.5)
    return x1, x2, 1024, 1.0, 0x5EC1


def oracle_runner(oracle):
    return lambda x1, x2, hyp_end, seed, hyp_begin=0: oracle.lmeds_fundamental(x1, x2, hyp_end, seed, hyp_begin=hyp_begin,
                                                                               nthreads=8)


FIGURES = {"rel": 0.0, "band": 0, "checked": 0}


def check_independent(res, x1, x2, what):
    """Median and mask of one PM_OK result against the fp64 reference; prints the figures it asserts on."""
    rc, F, mask, ninl, best, med = res
    assert rc == PM_OK and best >= 0, (what, rc, best)
    rel, ref = R.check_median(F, x1, x2, med)
    band = R.check_mask(F, x1, x2, mask, ninl)
    FIGURES["rel"] = max(FIGURES["rel"], rel or 0.0)
    FIGURES["band"] = max(FIGURES["band"], band)
    FIGURES["checked"] += 1
    print("lmeds independent %-24s n=%-6d median %.9g fp64 %.9g rel %s band %d inliers %d"
          % (what, x1.shape[0], med, ref, "below floor" if rel is None else "%.3g" % rel, band, ninl))
    return rel, band


def check_tie_side(res, x1, x2, name):
    """The duplicated set really puts the winner's median pair on the side of the tie branch it is meant to cover."""
    ties = DUP_CASES[name][3]
    n = x1.shape[0]
    below = R.strictly_below_upper_median(R.residuals(res[1], x1, x2))
    if ties is None:
        assert n & 1
    elif ties:
        assert below < n // 2, (name, below)
    else:
        assert below == n // 2, (name, below)
    return below


def sweep(run, x1, x2, seed, what, each=None):
    """One call per hypothesis: the answer is the best of at most three models, so every single median shows."""
    found, worst = 0, 0.0
    for h in SWEEP:
        res = run(x1, x2, h + 1, seed, h)
        if each is not None:
            each(h, res)
        assert res[0] in (PM_OK, PM_E_NO_MODEL), (what, h, res[0])
        if res[0] != PM_OK:
            continue
        assert res[4] // 3 == h, (what, h, res[4])
        rel, _ = R.check_median(res[1], x1, x2, res[5])
        worst = max(worst, rel or 0.0)
        found += 1
    FIGURES["rel"] = max(FIGURES["rel"], worst)
    print("lmeds independent sweep %-18s n=%-6d models found %d / %d worst rel %.3g" % (what, x1.shape[0], found, len(SWEEP), worst))
    assert found >= len(SWEEP) // 2, (what, found)
    return found, worst


def check_poisoned(run, sample7):
    x1, x2, iters, seed, rows = poisoned_case()
    drawn = {int(i) for h in range(iters) for i in sample7(seed, h, x1.shape[0])}
    assert drawn & set(rows.tolist())                # some hypothesis of the range samples a poisoned row
    res = run(x1, x2, iters, seed)
    check_independent(res, x1, x2, "poisoned")
    assert not res[2][rows].any() and res[3] > 1000
    return res


def check_mostly_nan(run):
    x1, x2, iters, seed = mostly_nan_case()
    rc, F, mask, ninl, best, med = run(x1, x2, iters, seed)
    assert rc == PM_E_NO_MODEL and (F == 0).all() and not mask.any() and ninl == 0 and best == -1 and med == np.inf
    assert R.median(R.residuals(np.eye(3), x1, x2)) == np.inf      # and so says the reference, for any F


def check_adaptive(res, x1, x2, what):
    """S16 mask of the winner against fp64 residuals at thr = thresh_px^2."""
    rc, F, mask, ninl, best, iters_run = res[0], res[1], res[2], res[3], res[4], res[5]
    assert rc == PM_OK and best >= 0, what
    band = R.check_mask_at(F, x1, x2, mask, ninl, what[1] * what[1])
    FIGURES["band"] = max(FIGURES["band"], band)
    print("adaptive independent %s n=%d band %d inliers %d iters_run %d winner %d" % (what, x1.shape[0], band, ninl, iters_run, best))


# ---- the C oracle standing in for the device ---------------------------------------------------------------------
@pytest.mark.parametrize("n", LDS_SIZES)
def test_oracle_at_the_lds_sizes(oracle, n):
    x1, x2, iters, seed = lds_case(n)
    check_independent(oracle_runner(oracle)(x1, x2, iters, seed), x1, x2, "lds")


@pytest.mark.parametrize("n", DEV_SIZES)
def test_oracle_at_the_device_form_sizes(oracle, n):
    x1, x2, iters, seed = dev_case(n)
    check_independent(oracle_runner(oracle)(x1, x2, iters, seed), x1, x2, "dev")


@pytest.mark.parametrize("name", sorted(DUP_CASES))
def test_oracle_on_ties_at_the_median(oracle, name):
    x1, x2, iters, seed = dup_case(name)
    res = oracle_runner(oracle)(x1, x2, iters, seed)
    check_independent(res, x1, x2, name)
    check_tie_side(res, x1, x2, name)
    sweep(oracle_runner(oracle), x1, x2, seed, name)


def test_oracle_per_hypothesis_at_the_largest_n(oracle):
    x1, x2, iters, seed = lds_case(32768)
    sweep(oracle_runner(oracle), x1, x2, seed, "n32768")


def test_oracle_on_non_finite_rows(oracle):
    check_poisoned(oracle_runner(oracle), oracle.sample7)
    check_mostly_nan(oracle_runner(oracle))


def test_oracle_adaptive_masks(oracle):
    x1, x2, seed = adaptive_case()
    res = oracle.ransac7_adaptive(x1, x2, 512, 0.99, ADAPT_THRESH, seed)
    assert res[5] == 512
    check_adaptive(res, x1, x2, (512, ADAPT_THRESH))
    x1, x2, iters, thr, seed = adaptive_survivor_case()
    res = oracle.ransac7_adaptive(x1, x2, iters, 0.99, thr, seed)
    assert res[4] < 3 * 512 and res[5] > 512, res[4:]
    check_adaptive(res, x1, x2, (iters, thr))
