import numpy as np


def assert_matches_equal(got, want, what=""):
    """Bit-exact comparison of two pm_match arrays (indices AND distance bits)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in ("queryIdx", "trainIdx", "imgIdx"):
        bad = np.nonzero(got[f] != want[f])
        assert bad[0].size == 0, "%s: %s differs at %s: got %s want %s" % (
            what, f, [b[:5] for b in bad], got[f][bad][:5], want[f][bad][:5])
    gb = got["distance"].view(np.uint32)
    wb = want["distance"].view(np.uint32)
    bad = np.nonzero(gb != wb)
    assert bad[0].size == 0, "%s: distance bits differ at %s: got %s want %s" % (
        what, [b[:5] for b in bad], got["distance"][bad][:5], want["distance"][bad][:5])


def assert_lmeds_equal(got, want, what=""):
    """Bit-exact comparison of two (status, F, mask, n_inliers, best_model, median) results of 7-point + LMedS."""
    rc_g, F_g, mask_g, n_g, best_g, med_g = got
    rc_w, F_w, mask_w, n_w, best_w, med_w = want
    assert rc_g == rc_w, what
    assert best_g == best_w, (what, best_g, best_w, med_g, med_w)
    assert np.float64(med_g).view(np.uint64) == np.float64(med_w).view(np.uint64), (what, med_g, med_w)
    assert n_g == n_w and (mask_g == mask_w).all(), what
    assert (F_g.view(np.uint64) == F_w.view(np.uint64)).all(), (what, F_g, F_w)
