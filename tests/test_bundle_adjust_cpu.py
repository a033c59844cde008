"""CPU: local bundle adjustment (docs/SPEC.md S113-S117).  pm_bundle_adjust_workspace is host arithmetic and is tested on the
library itself (no GPU); everything else runs on the plain-C restatement tests/ba_ref.c, the code the GPU tests compare the
kernel with bit for bit: its invariants, its used set against a numpy evaluation, its minimum against a dense numpy solver
that shares nothing with the Schur form, and the recovery of perturbed poses on the scenes the feature was prototyped on."""
import numpy as np
import pytest

import ba_ref as B
from points_matching_amd import api

IDENT = np.r_[np.eye(3).reshape(-1), np.zeros(3)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def test_workspace_is_host_arithmetic():
    W = api.bundle_adjust_workspace
    for V in range(2, 9):
        sizes = [W(V, cap) for cap in (0, 1, 2, 3, 7, 512, 513, 1025, 65535, 65536)]
        assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
        if V > 2:
            assert all(W(V, cap) >= W(V - 1, cap) for cap in (0, 1, 513, 65536)) and W(V, 513) > W(V - 1, 513)
    for V, cap in ((1, 10), (0, 10), (-1, 10), (9, 10), (3, -1), (3, api.PM_BA_MAX_POINTS + 1)):
        assert W(V, cap) == 0
    # every part of the layout fits: X twice, the linearisation twice, Y, the used bytes (SPEC S117)
    assert W(8, 1000) >= 8 * 1000 * (3 + 3 + 2 * (10 + 18 * 7) + 18 * 7) + 1000


@pytest.mark.parametrize("n_views,mask", [(2, 1), (3, 1), (4, 3), (8, 0x7F)])
def test_restatement_invariants(n_views, mask):
    K, uv, Rt, Rt0, xyz0, X = B.perturbed(150, n_views, 20 + n_views, mask)
    xyz0 = xyz0.copy()
    xyz0[3::17] = np.nan
    start = [IDENT if r is None else r for r in Rt0]
    zero = B.run(K, uv, Rt0, xyz0, mask, 0)
    r = B.run(K, uv, Rt0, xyz0, mask, 10)
    # max_iters = 0 moves nothing and reports cost_in and the used set
    assert (zero.status, zero.iters, zero.accepted) == (1, 0, 0) and zero.cost_out == zero.cost_in == r.cost_in
    assert (_bits(zero.xyz) == _bits(xyz0)).all() and (_bits(zero.Rt) == _bits(np.array(start))).all()
    assert (zero.used == r.used).all() and zero.n_points == r.n_points == (r.used != 0).sum()
    assert r.n_obs == sum(bin(int(b)).count("1") for b in r.used)
    # the cost only falls; held poses keep their bits; rows outside the used set keep theirs; used rows are the fp64 state rounded
    assert r.status == 0 and r.accepted >= 1 and r.iters <= 10 and r.cost_out < r.cost_in
    for v in range(n_views):
        assert ((_bits(r.Rt[v]) == _bits(start[v])).all()) == bool((mask >> v) & 1)
    out = r.used == 0
    assert out.sum() >= 8 and (_bits(r.xyz[out]) == _bits(xyz0[out])).all()
    assert (_bits(r.xyz[~out]) == _bits(r.xyz64[~out].astype(np.float32))).all() and not np.isnan(r.xyz[~out]).any()
    # cost_out is the cost of the fp64 state: a numpy evaluation agrees to rounding
    assert abs(B.np_cost(K, uv, list(r.Rt), r.xyz64, r.used) - r.cost_out) <= 1e-9 * r.cost_out
    assert abs(B.np_cost(K, uv, Rt0, xyz0.astype(np.float64), r.used) - r.cost_in) <= 1e-9 * r.cost_in
    # a rotation stays a rotation through ten Cayley updates
    for v in range(n_views):
        Rm = r.Rt[v][:9].reshape(3, 3)
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-13


def test_status_1_returns_every_byte_and_status_2_needs_data():
    K, uv, Rt, Rt0, xyz0, X = B.perturbed(120, 3, 31, 3)
    # status 2: the free view sees 3 used points; outputs are the inputs
    uv3 = [u.copy() for u in uv]
    seen = np.nonzero(B.run(K, uv, Rt0, xyz0, 3, 0).used >> 2 & 1)[0]
    uv3[2][:] = np.nan
    uv3[2][seen[:3]] = uv[2][seen[:3]]
    r = B.run(K, uv3, Rt0, xyz0, 3, 10)
    assert (r.status, r.iters, r.accepted) == (2, 0, 0) and r.cost_out == r.cost_in and (_bits(r.xyz) == _bits(xyz0)).all()
    assert (_bits(r.Rt[2]) == _bits(Rt0[2])).all() and (r.used >> 2 & 1).sum() == 3
    r = B.run(K, [u[:0] for u in uv], Rt0, xyz0[:0], 3, 10)
    assert (r.status, r.n_points, r.n_obs, r.cost_in, r.cost_out) == (2, 0, 0, 0.0, 0.0)
    # status 1 with iterations allowed: a used point on the optical axis of two axis-aligned held views has Vp_22 = 0 exactly
    # (Jc's third column is fa*R_02 - a*R_22 with R_02 = 0 and a = fa*px = 0), so its damped Cholesky fails: S24's "stop"
    Rt1 = [None, np.r_[np.eye(3).reshape(-1), [0.0, 0.0, 1.0]], Rt0[2]]
    uv1 = [u.copy() for u in uv]
    x1 = xyz0.copy()
    x1[10] = (0.0, 0.0, 5.0)
    uv1[0][10] = uv1[1][10] = (np.float32(K[2]), np.float32(K[3]))
    uv1[2][10] = np.nan
    r = B.run(K, uv1, Rt1, x1, 3, 10)
    assert (r.status, r.iters, r.accepted) == (1, 0, 0) and r.used[10] == 3 and r.cost_out == r.cost_in
    assert (_bits(r.xyz) == _bits(x1)).all() and (_bits(r.Rt[2]) == _bits(Rt0[2])).all() and (r.Rt[0] == IDENT).all()


def test_gate_removes_what_numpy_says_it_should():
    K, uv, Rt, Rt0, xyz0, X = B.perturbed(400, 5, 41, 1, swap_every=9)
    xyz0 = xyz0.copy()
    xyz0[7::19] = np.nan
    xyz0[100, 2] = -3.0
    for gate in (0.0, 12.0, 40.0):
        used, e = B.np_used(K, uv, Rt0, xyz0, gate)
        if gate:                                    # no observation so close to the gate that float64 numpy could disagree
            assert np.nanmin(np.abs(e / gate ** 2 - 1)) > 1e-9
        r = B.run(K, uv, Rt0, xyz0, 1, 0, gate)
        assert (r.used == used).all() and r.used[100] == 0 and (r.used[7::19] == 0).all()
    assert B.run(K, uv, Rt0, xyz0, 1, 0, 12.0).n_obs < B.run(K, uv, Rt0, xyz0, 1, 0, 40.0).n_obs < B.run(K, uv, Rt0, xyz0, 1, 0).n_obs


DENSE_CASES = [(2, 40, 1), (2, 120, 1), (3, 100, 1), (3, 60, 3), (4, 120, 3), (4, 200, 1)]
DENSE_GAP = 2.2e-13


@pytest.mark.parametrize("n_views,n,mask", DENSE_CASES)
def test_minimum_equals_a_dense_numpy_solver(n_views, n, mask):
    """The restatement at 30 iterations and the dense numpy solver at convergence (ba_ref.np_dense: the full stacked Jacobian of
    every free pose and point parameter, lstsq steps with additive damping, exact exponential update) minimise the same
    function over the same used set.  Measured here over these cases and seeds 1, 2: the largest relative gap of the two
    costs, either sign, was 2.2e-14 — the rounding of a cost of 5 .. 220 px^2 summed in two different orders, where one
    pixel-noise draw moves the cost by percents.  The bound is ten times that."""
    for seed in (1, 2):
        K, uv, Rt, Rt0, xyz0, X = B.perturbed(n, n_views, seed, mask)
        r = B.run(K, uv, Rt0, xyz0, mask, 30)
        P, Xd, cost = B.np_dense(K, uv, Rt0, xyz0.astype(np.float64), r.used, mask)
        gap = abs(r.cost_out - cost) / cost
        print("dense gap", n_views, n, mask, seed, r.cost_out, cost, gap)
        assert r.status == 0 and gap <= DENSE_GAP


# the four scenes the scheme was prototyped on: views, points, fixed mask (0.5 px noise, 10 % blanked, free poses turned by 0.5
# degrees and shifted by N(0, 0.02), points shifted by N(0, 0.05) and rounded to f32)
PROTOTYPE = [(3, 193, 1), (8, 513, 1), (4, 298, 3), (2, 84, 1)]


@pytest.mark.parametrize("n_views,n,mask", PROTOTYPE)
def test_recovers_perturbed_poses(n_views, n, mask):
    """After 10 iterations every free pose's rotation error is below half of the 0.5 degrees it started with on the scenes of
    three and more views (measured here, seed 100 + views: 0.026, 0.023 and 0.026 degrees, costs 55 164 -> 114.2, 480 380 ->
    1 475.6, 97 906 -> 308.0).  The two-view scene has 63-73 used points and its rotation is held by that many noisy pixels
    alone: over seeds 0 .. 7 the restatement's minimum sits 0.011 .. 0.30 degrees from the truth (0.30 at the seed used here),
    and the dense numpy solver finds the same minimum, so 0.25 degrees is not a property of the solver there.  That scene
    asserts instead that the error falls below its start and that the pose is the dense solver's to 1e-3 degrees."""
    K, uv, Rt, Rt0, xyz0, X = B.perturbed(n, n_views, 100 + n_views, mask)
    r = B.run(K, uv, Rt0, xyz0, mask, 10)
    free = [v for v in range(n_views) if not (mask >> v) & 1]
    err = [B.rot_err_deg(r.Rt[v], Rt[v]) for v in free]
    print("recovery", n_views, n, mask, r.cost_in, r.cost_out, r.iters, r.accepted, err)
    assert r.status == 0 and r.cost_out < 0.02 * r.cost_in
    assert all(abs(B.rot_err_deg(Rt0[v], Rt[v]) - 0.5) < 1e-6 for v in free)
    if n_views > 2:
        assert max(err) < 0.25
    else:
        P, Xd, cost = B.np_dense(K, uv, Rt0, xyz0.astype(np.float64), r.used, mask)
        assert max(err) < 0.5 and all(B.rot_err_deg(r.Rt[v], P[v]) < 1e-3 for v in free)
    if mask == 3:                                   # two held poses fix the scale: the free translations' directions improve
        for v in free:
            assert B.t_dir_err_deg(r.Rt[v], Rt[v]) < 0.5 * B.t_dir_err_deg(Rt0[v], Rt[v])
