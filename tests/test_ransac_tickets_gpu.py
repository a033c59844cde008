"""GPU: the seven families of the one-launch scorer share one block of arrival words per context (csrc/ransac_internal.hpp,
SyncWord).  F-Sampson, H, A-full, A-partial, E, PnP and 3-D alignment run back to back on ONE context and stream, twice
round, 64 correspondences and 256 hypotheses (samples) each: every status, model, mask, count and key must equal, bit for
bit, what the same call gives on a context of its own.  Two families drawing tickets from one word, or a word left
non-zero by a launch, would make a later launch pick its winner early or never, and so change its key, model, count or mask."""
import numpy as np
import pytest

import points_matching_amd as pm
from points_matching_amd import api, synth

pytestmark = pytest.mark.gpu

N, IDS, SEED = 64, 256, 0x71C4E7
KMAT = np.array([[800.0, 0.0, 500.0], [0.0, 850.0, 330.0], [0.0, 0.0, 1.0]])
K = (800.0, 850.0, 500.0, 330.0)

CALLS = {
    "F": (synth.two_view(N, seed=31)[:2], lambda c, a, b: c.ransac_fundamental(a, b, IDS, 1.0, SEED, kind=api.PM_ERR_SAMPSON)),
    "H": (synth.planar_view(N, seed=32)[:2], lambda c, a, b: c.ransac_homography(a, b, IDS, 2.0, SEED)),
    "A-full": (synth.affine_view(N, seed=33)[:2], lambda c, a, b: c.ransac_affine(a, b, IDS, 2.0, SEED, model=api.PM_AFFINE_FULL)),
    "A-partial": (synth.affine_view(N, seed=34, partial=True)[:2],
                  lambda c, a, b: c.ransac_affine(a, b, IDS, 2.0, SEED, model=api.PM_AFFINE_PARTIAL)),
    "E": (synth.calibrated_view(N, seed=35, K=KMAT)[:2], lambda c, a, b: c.ransac_essential(a, b, K, IDS, 1.0, SEED)),
    "P": (synth.pnp_scene(N, seed=36, K=KMAT)[:2], lambda c, a, b: c.ransac_pnp(a, b, K, IDS, 3.0, SEED)),
    "X": (synth.align3d_scene(N, seed=37)[:2], lambda c, a, b: c.ransac_align3d(a, b, IDS, 0.05, SEED)),
}


def _frozen(result):
    return tuple(np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else x for x in result)


def test_seven_families_back_to_back_on_one_context_equal_fresh_contexts():
    want = {}
    for name, ((a, b), call) in CALLS.items():
        c = pm.Context(0)
        try:
            r = call(c, a, b)
        finally:
            c.close()
        assert r[0] == api.PM_OK and r[-1] >> 32 >= 8, (name, r[0], hex(r[-1]))       # a real winner with real inliers
        want[name] = _frozen(r)
    c = pm.Context(0)
    try:
        for rnd in range(2):
            for name, ((a, b), call) in CALLS.items():
                assert _frozen(call(c, a, b)) == want[name], (name, "round", rnd)
    finally:
        c.close()
