"""CPU: the references of compaction_ref.py checked against each other, so that the GPU tests built on them are not
vacuous.  On every pattern and size, four statements of each rule agree exactly: the numpy rule, the keep-vector the
generator fixed by construction, the host C filter of the library and (ratio, midpoint) the oracle."""
import numpy as np
import pytest

from points_matching_amd import api
import compaction_ref as cr
from util import assert_matches_equal

SIZES = (1, 255, 257, 65537)
FWD, REV = api.PM_CROSS_RATIO_FWD, api.PM_CROSS_RATIO_REV


def _records(nq, pattern, k=2):
    return cr.make_records(nq, pattern, np.random.default_rng([nq, cr.PATTERNS.index(pattern), k]), k=k)


@pytest.mark.parametrize("pattern", cr.PATTERNS)
@pytest.mark.parametrize("nq", SIZES)
def test_generator_honours_its_contract(nq, pattern):
    r = _records(nq, pattern, k=3)
    i = np.arange(nq)
    want = {"all": np.ones(nq, bool), "none": np.zeros(nq, bool), "checker": (i // 256) % 2 == 0, "last_only": i == nq - 1,
            "first_of_block": i % 256 == 0}.get(pattern)
    if want is None:
        assert r.keep.sum() == nq // 2
    else:
        assert np.array_equal(r.keep, want)
    assert r.fwd.shape == (nq, 3) and r.rev.shape == (r.nt, 2) and r.mid.shape == (nq,) and r.nt == nq
    assert (r.fwd["queryIdx"] == i[:, None]).all() and (r.mid["queryIdx"] == i).all()
    assert (r.rev["queryIdx"] == np.arange(r.nt)[:, None]).all()
    for idx, hi in ((r.fwd["trainIdx"], r.nt), (r.mid["trainIdx"], r.nt), (r.rev["trainIdx"], nq)):
        assert ((idx == -1) | ((idx >= 0) & (idx < hi))).all()
    # every reason the predicate has for a drop is in use as soon as there are enough dropped rows
    n_drop = int((~r.keep).sum())
    assert set(np.unique(r.reason[~r.keep])) == set(range(min(n_drop, cr.N_DROP_REASONS)))
    assert (r.reason[r.keep] == -1).all()
    if n_drop >= cr.N_DROP_REASONS:
        f = r.fwd
        assert (f["distance"][:, 0] == f["distance"][:, 1]).any() and np.isnan(f["distance"][:, 0]).any()
        assert np.isnan(f["distance"][:, 1]).any() and (f["trainIdx"][:, 0] == -1).any()
        assert ((f["trainIdx"][:, 1] == -1) & np.isposinf(f["distance"][:, 1])).any()
        rhs = np.float32(r.ratio) * f["distance"][:, 1]
        with np.errstate(invalid="ignore"):
            assert (f["distance"][:, 0] == np.nextafter(rhs, np.float32(np.inf))).any() and (f["distance"][:, 0] == rhs).any()


@pytest.mark.parametrize("pattern", cr.PATTERNS)
@pytest.mark.parametrize("nq", SIZES)
def test_ratio_rule_four_ways(oracle, nq, pattern):
    for k in (2, 3):
        r = _records(nq, pattern, k)
        assert np.array_equal(cr.ratio_keep(r.fwd, r.ratio), r.keep)
        want = r.fwd[r.keep, 0]
        assert_matches_equal(cr.ratio_rule(r.fwd, r.ratio), want, "numpy")
        assert_matches_equal(api.filter_ratio(r.fwd, r.ratio), want, "host C")
        assert_matches_equal(oracle.filter_ratio(r.fwd, r.ratio), want, "oracle")


@pytest.mark.parametrize("pattern", cr.PATTERNS)
@pytest.mark.parametrize("nq", SIZES)
def test_midpoint_rule_four_ways(oracle, nq, pattern):
    r = _records(nq, pattern)
    want = r.mid[r.keep]
    for name, (good, lo, hi) in (("numpy", cr.midpoint_rule(r.mid)), ("host C", api.filter_midpoint(r.mid)),
                                 ("oracle", oracle.filter_midpoint(r.mid))):
        assert_matches_equal(good, want, name)
        assert [lo, hi] == r.mid_minmax, name


@pytest.mark.parametrize("pattern", cr.PATTERNS)
@pytest.mark.parametrize("nq", SIZES)
def test_cross_rule_three_ways(nq, pattern):
    """(The oracle has no cross rule: cross_ref.py is the independent statement.)"""
    r = _records(nq, pattern)
    want = r.fwd[r.keep, 0]
    for flags in (0, FWD | REV):
        assert_matches_equal(cr.cross_rule(r.fwd, r.rev, flags, r.ratio), want, "numpy flags %d" % flags)
        assert_matches_equal(api.filter_cross(r.fwd, r.rev, flags, r.ratio), want, "host C flags %d" % flags)


def test_gather_is_plain_indexing():
    r = _records(257, "half")
    good = r.fwd[r.keep, 0]
    xy1, xy2 = cr.gather(r.kp1, r.kp2, good)
    assert np.array_equal(xy1, r.kp1[r.keep]) and np.array_equal(xy2, api.gather_points(r.kp2, good["trainIdx"]))
