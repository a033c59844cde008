"""GPU: pose-graph optimisation (pm_pose_graph_optimize*, pm_pgo_move_points*, docs/SPEC.md S118-S123) against the C restatement
(tests/pgo_ref.c) bit for bit — poses as u64, the used bytes and every field of the info record, with guard values beyond the
count — at the edges of S23's 512 partials in nodes and edges, in both models, with 0, 1 and 10 steps and 1 and 50
conjugate-gradient iterations; the cases named for where the kernel can go wrong (shuffled edge ids, a hub, duplicate edges,
held nodes in the middle, an isolated node, every rule of the used set, a zero weight, a device-side count with poisoned rows
beyond it, poses refined in place); the host form, every refusal with the outputs untouched, capture and replay, the point
move, and the chain RANSAC alignment -> refit into the edge array -> graph -> point move on one stream."""
import numpy as np
import pytest

import pgo_ref as G
import points_matching_amd as pm
from points_matching_amd import api

pytestmark = pytest.mark.gpu

NODES = (2, 3, 511, 512, 513, 1025)          # one node per partial -1 / 0 / +1, and two rounds
GUARD = 7.0
MODELS = (api.PM_PGO_RIGID, api.PM_PGO_SIM3)
_graphs = {}


def _graph(n, n_edges, model, shuffle=False):
    key = (n, n_edges, model, shuffle)
    if key not in _graphs:
        _graphs[key] = G.graph(n, n_edges, model, 11 + n, shuffle=shuffle)[1:]
    return _graphs[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


class _Dev:
    """The device side of one call: the graph, and outputs filled with guard values.  in_place: d_pose_out is d_pose_in."""

    def __init__(self, model, pose, fixed, ab, Z, w, count=None, in_place=False, used=True, work_offset=0):
        import torch
        self.torch, dev = torch, torch.device("cuda", 0)
        self.model, self.N, self.cap = model, len(pose), len(ab)
        up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).to(dev)     # noqa: E731
        self.pose, self.fixed = up(pose, np.float64), up(fixed, np.uint8)
        self.ab, self.Z, self.w = up(ab, np.int32), up(Z, np.float64), up(w, np.float64)
        self.out = self.pose if in_place else torch.full((self.N, 13), GUARD, dtype=torch.float64, device=dev)
        self.count = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
        self.used = torch.full((max(self.cap, 1),), 0xEE, dtype=torch.uint8, device=dev) if used else None
        self.info = torch.full((40,), 0x55, dtype=torch.uint8, device=dev)
        self.work_bytes = api.pose_graph_workspace(self.N, self.cap, model)
        self.work = torch.full((self.work_bytes + 16,), 0xA5, dtype=torch.uint8, device=dev)
        self.work_ptr = self.work.data_ptr() + work_offset
        torch.cuda.synchronize()

    def enqueue(self, ctx, prm, **over):
        a = dict(pose=self.pose.data_ptr(), n_nodes=self.N, fixed=self.fixed.data_ptr(), ab=self.ab.data_ptr(), Z=self.Z.data_ptr(),
                 w=self.w.data_ptr(), count=None if self.count is None else self.count.data_ptr(), cap=self.cap,
                 out=self.out.data_ptr(), used=None if self.used is None else self.used.data_ptr(), work=self.work_ptr,
                 work_bytes=self.work_bytes, info=self.info.data_ptr())
        a.update(over)
        ctx.pose_graph_optimize_dev(a["pose"], a["n_nodes"], a["fixed"], a["ab"], a["Z"], a["w"], a["count"], a["cap"], prm, a["out"],
                                    a["used"], a["work"], a["work_bytes"], a["info"])

    def fetch(self):
        return (self.out.cpu().numpy(), None if self.used is None else self.used.cpu().numpy(),
                self.info.cpu().numpy().view(api.PGO_INFO_DTYPE)[0])

    def run(self, ctx, prm):
        self.enqueue(ctx, prm)
        ctx.synchronize()
        return self.fetch()

    def untouched(self):
        out, used, info = self.out.cpu().numpy(), self.used.cpu().numpy(), self.info.cpu().numpy()
        return (out == GUARD).all() and (used == 0xEE).all() and (info == 0x55).all()


def _assert_parity(got, ref, n):
    out, used, info = got
    assert (_bits(out) == _bits(ref.pose)).all()
    if used is not None:
        assert (used[:n] == ref.used[:n]).all() and (used[n:] == 0xEE).all()
    assert _bits(np.float64(info["cost_in"])) == _bits(np.float64(ref.cost_in))
    assert _bits(np.float64(info["cost_out"])) == _bits(np.float64(ref.cost_out))
    assert (info["n_edges_used"], info["n_nodes_free"], info["iters"], info["accepted"], info["cg_total"], info["status"]) == \
        (ref.n_edges_used, ref.n_nodes_free, ref.iters, ref.accepted, ref.cg_total, ref.status)


def _one(ctx, model, g, max_iters=10, cg_iters=50, cg_tol=1e-6, n=None, in_place=False, used=True, work_offset=0):
    pose, fixed, ab, Z, w = g
    n_eff = len(ab) if n is None else max(0, min(n, len(ab)))
    ref = G.run(model, pose, fixed, ab, Z, w, max_iters, cg_iters, cg_tol, n_edges=n_eff)
    d = _Dev(model, pose, fixed, ab, Z, w, count=n, in_place=in_place, used=used, work_offset=work_offset)
    _assert_parity(d.run(ctx, api.pgo_params(model, max_iters, cg_iters, cg_tol)), ref, n_eff)
    if ref.status != 0:                                          # statuses 1 and 2 return their inputs
        assert (_bits(ref.pose) == _bits(np.ascontiguousarray(pose, np.float64))).all() and ref.cost_out == ref.cost_in
    held = np.asarray(fixed) != 0
    assert (_bits(ref.pose[held]) == _bits(np.ascontiguousarray(pose, np.float64)[held])).all()
    if model == api.PM_PGO_RIGID:
        assert (_bits(ref.pose[:, 12]) == _bits(np.ascontiguousarray(pose, np.float64)[:, 12])).all()
    return ref


@pytest.mark.parametrize("max_iters", [0, 1, 10])
@pytest.mark.parametrize("model", MODELS)
def test_bit_parity_at_the_partial_edges(ctx, model, max_iters):
    k = 0
    for n in NODES:
        for n_edges in (n - 1 + 4, 4 * n):
            for cg_iters in (1, 50):
                k += 1
                ref = _one(ctx, model, _graph(n, n_edges, model), max_iters, cg_iters, in_place=k % 3 == 0)
                assert ref.n_edges_used == n_edges and ref.n_nodes_free == n - 1 and ref.cost_out <= ref.cost_in
                assert ref.status == (1 if max_iters == 0 else 0 if (max_iters, cg_iters) == (10, 50) else ref.status) != 2
                assert ref.iters <= max_iters
                assert ref.cg_total <= cg_iters * ref.iters + cg_iters


@pytest.mark.parametrize("model", MODELS)
def test_shuffled_edge_ids_and_a_hub(ctx, model):
    """Incidence order is ascending edge id whatever order the edges arrive in; node 5 has 200 incident edges."""
    assert _one(ctx, model, _graph(513, 2052, model, shuffle=True)).status == 0
    pose, fixed, ab, Z, w = (v.copy() for v in _graph(210, 450, model))
    rng = np.random.default_rng(5)
    hub = rng.choice(np.arange(209, 450), 200, replace=False)
    for e in hub:
        other = int(rng.integers(6, 210))
        ab[e] = (5, other) if e % 2 else (other, 5)
        Z[e] = G.noisy(G.between(pose[ab[e, 0]], pose[ab[e, 1]]), rng, 0.5, 0.01)
    ref = _one(ctx, model, (pose, fixed, ab, Z, w))
    assert ref.status == 0 and ((ab == 5).any(1)).sum() >= 200


@pytest.mark.parametrize("model", MODELS)
def test_duplicate_edges_and_a_zero_weight(ctx, model):
    pose, fixed, ab, Z, w = (v.copy() for v in _graph(3, 12, model))
    ab[2:8] = (1, 2)                                             # six edges between the same pair, with different measurements
    w[3] = 0.0
    w[4] = (1.0, 0.0, 1.0)
    ref = _one(ctx, model, (pose, fixed, ab, Z, w))
    assert ref.status == 0 and ref.n_edges_used == 12


@pytest.mark.parametrize("model", MODELS)
def test_every_rule_of_the_used_set(ctx, model):
    start, fixed, ab, Z, w, expected = G.rules_graph(model)
    ref = _one(ctx, model, (start, fixed, ab, Z, w), in_place=True)
    assert (ref.used == expected).all() and ref.n_edges_used == expected.sum() and ref.status == 0
    free = ~fixed.astype(bool)
    free[[30, 33, 40]] = False                                   # a NaN pose, a negative scale, no edge: held for the run
    assert ref.n_nodes_free == free.sum()
    assert (_bits(ref.pose[~free]) == _bits(start[~free])).all() and not (_bits(ref.pose[free]) == _bits(start[free])).all(1).any()
    # no fixed node at all, and no used edge at all: status 2
    ref = _one(ctx, model, (start, np.zeros(41, np.uint8), ab, Z, w))
    assert ref.status == 2 and ref.n_edges_used > 0 and ref.iters == 0
    ref = _one(ctx, model, (start, np.ones(41, np.uint8), ab, Z, w))
    assert (ref.status, ref.n_edges_used, ref.n_nodes_free, ref.cost_in) == (2, 0, 0, 0.0)


@pytest.mark.parametrize("model", MODELS)
def test_device_side_count_and_poisoned_rows(ctx, model):
    """Rows at or beyond the count are garbage: node indices far out of range, NaN measurements.  They are neither read into
    the result nor written; a NULL count means cap_edges; a workspace that is not 16-byte aligned; no d_edge_used."""
    pose, fixed, ab, Z, w = (v.copy() for v in _graph(513, 2052, model))
    n = 1500
    ab[n:] = 0x7FFFFFF0
    Z[n:] = np.nan
    w[n:] = -np.inf
    g = (pose, fixed, ab, Z, w)
    assert _one(ctx, model, g, n=n).status == 0
    assert _one(ctx, model, g, n=n, used=False, work_offset=4, in_place=True).status == 0
    for count in (0, -3):
        ref = _one(ctx, model, g, n=count)
        assert (ref.status, ref.n_edges_used, ref.cost_in) == (2, 0, 0.0)
    assert _one(ctx, model, g, n=5000).n_edges_used == n        # a count above cap_edges is clamped; the poisoned rows are unused
    d = _Dev(model, pose, fixed, ab, Z, w, count=n)
    d.run(ctx, api.pgo_params(model))
    assert (d.ab.cpu().numpy() == ab).all() and (_bits(d.Z.cpu().numpy()) == _bits(Z)).all() and (_bits(d.w.cpu().numpy()) == _bits(w)).all()


@pytest.mark.parametrize("model", MODELS)
def test_status_1_at_the_minimum(ctx, model):
    """Measurements that the start satisfies exactly: every residual and the gradient are 0.0, the first conjugate-gradient
    iteration meets p . Ap = 0 and the run stops before any trial."""
    ref = _one(ctx, model, G.exact_graph(model))
    assert (ref.status, ref.iters, ref.accepted, ref.cg_total, ref.cost_in) == (1, 0, 0, 0, 0.0) and ref.n_edges_used == 15


@pytest.mark.parametrize("model", MODELS)
def test_host_form_equals_the_device_form(ctx, model):
    pose, fixed, ab, Z, w = _graph(511, 2044, model)
    ref = G.run(model, pose, fixed, ab, Z, w)
    out, used, info = ctx.pose_graph_optimize(pose, fixed, ab, Z, w, api.pgo_params(model))
    _assert_parity((out, np.r_[used, np.uint8(0xEE)], info), ref, len(ab))
    out, used, info = ctx.pose_graph_optimize(pose, fixed, ab[:0], Z[:0], w[:0], api.pgo_params(model))
    assert info["status"] == 2 and info["n_edges_used"] == 0 and (_bits(out) == _bits(pose)).all()


def test_refusals_leave_the_outputs_untouched(ctx):
    model = api.PM_PGO_SIM3
    pose, fixed, ab, Z, w = _graph(3, 12, model)
    d = _Dev(model, pose, fixed, ab, Z, w)
    good = api.pgo_params()
    inf, nan = float("inf"), float("nan")

    def refused(prm=good, status=api.PM_E_INVALID, **over):
        with pytest.raises(pm.PmError) as e:
            d.enqueue(ctx, prm, **over)
        ctx.synchronize()
        assert e.value.status == status, e.value
        assert d.untouched()
        return True

    for name in ("pose", "fixed", "ab", "Z", "w", "out", "work", "info"):
        assert refused(**{name: None})
    for nn in (-1, 0, 1):
        assert refused(n_nodes=nn)
    assert refused(cap=-1)
    bad = [api.pgo_params(model=v) for v in (-1, 2)] + [api.pgo_params(max_iters=v) for v in (-1, 101)]
    bad += [api.pgo_params(cg_iters=v) for v in (0, -1, 1001)] + [api.pgo_params(cg_tol=v) for v in (-1e-3, 1.0, inf, nan)]
    bad += [api.pgo_params(flags=v) for v in (1, -1)]
    reserved = api.pgo_params()
    reserved.reserved = 1
    for prm in bad + [reserved]:
        assert refused(prm=prm)
        with pytest.raises(pm.PmError) as e:
            ctx.pose_graph_optimize(pose, fixed, ab, Z, w, prm)
        assert e.value.status == api.PM_E_INVALID
    assert refused(work_bytes=d.work_bytes - 1) and refused(work_bytes=0)             # a workspace one byte short
    assert refused(n_nodes=api.PM_PGO_MAX_NODES + 1, status=api.PM_E_UNSUPPORTED)
    assert refused(cap=api.PM_PGO_MAX_EDGES + 1, status=api.PM_E_UNSUPPORTED)
    L = api.lib()
    assert L.pm_pose_graph_optimize_dev(None, None, 3, None, None, None, None, None, 0, None, None, None, None, 0, None) == api.PM_E_INVALID
    assert L.pm_pose_graph_optimize(None, None, 3, None, None, None, None, 0, None, None, None, None) == api.PM_E_INVALID
    assert L.pm_pgo_move_points_dev(None, None, None, 3, None, None, None, 1, None) == api.PM_E_INVALID
    assert L.pm_pgo_move_points(None, None, None, 3, None, None, 1, None) == api.PM_E_INVALID
    with pytest.raises(pm.PmError) as e:
        ctx.pgo_move_points(pose, pose, np.zeros(0, np.int32), np.zeros((0, 3), np.float32))
    assert e.value.status == api.PM_E_UNSUPPORTED
    # and the call still works
    _assert_parity(d.run(ctx, good), G.run(model, pose, fixed, ab, Z, w), len(ab))


def test_capture_and_replay():
    """Recorded once on a stream, replayed after the measurements and the device-side count changed: the restatement each
    time."""
    import gc
    import torch
    dev = torch.device("cuda", 0)
    model = api.PM_PGO_SIM3
    pose, fixed, ab, Z, w = _graph(513, 2052, model)
    st = torch.cuda.Stream(device=dev)
    prev = torch.cuda.current_stream(dev)
    torch.cuda.set_stream(st)
    c = pm.Context(0)
    c.set_stream(st.cuda_stream)
    try:
        d = _Dev(model, pose, fixed, ab, Z, w, count=len(ab))
        prm = api.pgo_params(model, 5, 20)
        gc.collect()                 # no finaliser of an earlier test's context (hipFree) inside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st, capture_error_mode="relaxed"):
            d.enqueue(c, prm)
        torch.cuda.set_stream(st)
        for n, scale in ((2052, 1.0), (1700, 1.001), (0, 1.0)):
            Z2 = Z.copy()
            Z2[:, 9:12] *= scale
            d.Z.copy_(torch.from_numpy(Z2).to(dev))
            d.count.fill_(n)
            d.used.fill_(0xEE)
            d.out.fill_(GUARD)
            g.replay()
            torch.cuda.synchronize()
            _assert_parity(d.fetch(), G.run(model, pose, fixed, ab, Z2, w, 5, 20, n_edges=n), n)
        del g
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)
        c.close()


@pytest.mark.parametrize("in_place", [False, True])
def test_move_points_bit_parity(ctx, in_place):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(9)
    old = G.ring_truth(50, G.SIM3, 2)
    new = np.array([G.compose(G.random_pose(rng, 3.0, (0.9, 1.1), 0.1), p) for p in old])
    new[7, 2], old[9, 12] = np.nan, np.inf
    for n in (1, 63, 64, 65, 4097):
        cap = n + 3
        xyz = rng.normal(0, 5, (cap, 3)).astype(np.float32)
        anchor = rng.integers(10, 50, cap).astype(np.int32)
        if n > 60:
            xyz[5, 1], xyz[11, 0], anchor[20], anchor[21], anchor[22], anchor[23] = np.nan, np.inf, -1, 50, 7, 9
        ref = G.move(old, new, anchor[:n], xyz[:n])
        d_old, d_new, d_anchor, d_xyz = (torch.from_numpy(v).to(dev) for v in (old, new, anchor, xyz))
        d_out = d_xyz if in_place else torch.full((cap, 3), GUARD, dtype=torch.float32, device=dev)
        d_n = torch.tensor([n], dtype=torch.int32, device=dev)
        ctx.pgo_move_points_dev(d_old.data_ptr(), d_new.data_ptr(), 50, d_anchor.data_ptr(), d_xyz.data_ptr(), d_n.data_ptr(), cap,
                                d_out.data_ptr())
        ctx.synchronize()
        out = d_out.cpu().numpy()
        assert (_bits(out[:n]) == _bits(ref)).all()
        assert (_bits(out[n:]) == _bits(xyz[n:] if in_place else np.full((3, 3), GUARD, np.float32))).all()
        assert (_bits(ctx.pgo_move_points(old, new, anchor[:n], xyz[:n])) == _bits(ref)).all()
        if n > 60:
            assert np.isnan(ref[[5, 11, 20, 21, 22, 23]]).all() and np.isfinite(np.delete(ref, [5, 11, 20, 21, 22, 23], 0)).all()
    same = G.move(old, old, anchor[:n], xyz[:n])
    ok = np.isfinite(same).all(1)
    assert np.abs(same[ok] - xyz[:n][ok]).max() <= 4e-6


def test_chain_align_refit_graph_move_on_one_stream(ctx):
    """A drifted ring of 40 keyframes.  Two maps of the same 300 points, one in the frame of keyframe 0 and one in the frame of
    keyframe 39, are aligned (RANSAC + refit) straight into the last row of the edge array; the graph is optimised and the map
    rows anchored to the keyframes move with them, all on one stream with no host read until the end.  The corrected poses
    are those of the restatement fed the same row, and the moved points lie closer to the truth than before."""
    import torch
    dev = torch.device("cuda", 0)
    model, N, npts = api.PM_PGO_SIM3, 40, 300
    rng = np.random.default_rng(21)
    truth = G.ring_truth(N, G.SIM3, 6)
    ab = np.array([(i, i + 1) for i in range(N - 1)] + [(N - 1, 0)], np.int32)
    E = len(ab)
    Z = np.array([G.between(truth[a], truth[b]) for a, b in ab])
    drift = G.pose13(G.rot([0.0, 0.0, np.radians(0.3)]), np.zeros(3), 1.02)
    start = [truth[0]]
    for i in range(N - 1):
        start.append(G.compose(drift, G.compose(Z[i], start[-1])))
    start = np.array(start)
    Z[E - 1] = 0.0                                               # the loop row comes from the device
    w = np.ones((E, 3))
    fixed = np.zeros(N, np.uint8)
    fixed[0] = 1
    X = rng.normal(0, 3, (npts, 3))

    def to_frame(T, P):
        R, t, s = G.parts(T)
        return s * P @ R.T + t
    xyz_a = to_frame(truth[N - 1], X).astype(np.float32)         # frame a = keyframe 39
    xyz_b = (to_frame(truth[0], X) + rng.normal(0, 1e-3, X.shape)).astype(np.float32)
    xyz_b[::10] += 1.0                                           # outliers
    # the map as the drifted keyframes built it: rows anchored to keyframe k were triangulated in k's (true) frame
    anchor = rng.integers(0, N, npts).astype(np.int32)

    def to_world(T, P):
        R, t, s = G.parts(T)
        return ((P - t) / s) @ R
    local = np.array([to_frame(truth[k], x) for k, x in zip(anchor, X)])
    map_rows = np.array([to_world(start[k], p) for k, p in zip(anchor, local)]).astype(np.float32)
    wb = api.pose_graph_workspace(N, E, model)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        ctx.set_stream(s.cuda_stream)
        try:
            d1, d2, d_pose, d_fixed, d_ab, d_Z, d_w, d_anchor, d_rows = (
                torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (xyz_a, xyz_b, start, fixed, ab, Z, w, anchor, map_rows))
            key = torch.zeros(1, dtype=torch.int64, device=dev)
            mask = torch.zeros(npts, dtype=torch.uint8, device=dev)
            ninl = torch.zeros(1, dtype=torch.int32, device=dev)
            out = torch.zeros((N, 13), dtype=torch.float64, device=dev)
            moved = torch.zeros((npts, 3), dtype=torch.float32, device=dev)
            info = torch.zeros(40, dtype=torch.uint8, device=dev)
            work = torch.zeros(wb, dtype=torch.uint8, device=dev)
            s.synchronize()
            view = api.XyzView(d1.data_ptr(), d2.data_ptr(), None, npts, 0)
            row = d_Z.data_ptr() + 104 * (E - 1)
            ctx.ransac_align3d_run_dev(view, 0, 500, 0.05, 3, key.data_ptr(), row, mask.data_ptr(), npts, ninl.data_ptr(),
                                       model=api.PM_ALIGN3D_SIMILARITY)
            ctx.align3d_refine_dev(view, mask.data_ptr(), row, row, None, model=api.PM_ALIGN3D_SIMILARITY)
            ctx.pose_graph_optimize_dev(d_pose.data_ptr(), N, d_fixed.data_ptr(), d_ab.data_ptr(), d_Z.data_ptr(), d_w.data_ptr(), None,
                                        E, api.pgo_params(model, 20, 100), out.data_ptr(), None, work.data_ptr(), wb, info.data_ptr())
            ctx.pgo_move_points_dev(d_pose.data_ptr(), out.data_ptr(), N, d_anchor.data_ptr(), d_rows.data_ptr(), None, npts,
                                    moved.data_ptr())
            ctx.synchronize()
        finally:
            ctx.set_stream(0)
    Zd = d_Z.cpu().numpy()
    assert (_bits(Zd[:E - 1]) == _bits(Z[:E - 1])).all() and G.pose_err(Zd[E - 1], G.between(truth[N - 1], truth[0]))[0] < 0.05
    ref = G.run(model, start, fixed, ab, Zd, w, 20, 100)
    _assert_parity((out.cpu().numpy(), None, info.cpu().numpy().view(api.PGO_INFO_DTYPE)[0]), ref, E)
    assert ref.status == 0 and ref.cost_out < 1e-3 * ref.cost_in
    got = moved.cpu().numpy()
    assert (_bits(got) == _bits(G.move(start, ref.pose, anchor, map_rows))).all()
    rms = lambda P: float(np.sqrt(((P - X) ** 2).sum(1).mean()))     # noqa: E731
    print("chain: rms before %.4g after %.4g, cost %.4g -> %.4g" % (rms(map_rows), rms(got), ref.cost_in, ref.cost_out))
    assert rms(got) < 0.1 * rms(map_rows)
