"""GPU: graph capture of the estimator calls (include/pm.h, "Graph capture of the estimator calls").  The _dev forms of the
six RANSAC families, their refinements, pose recovery, triangulation, the gathers and the 3-D transform are recorded into a
graph on a capturing stream and replayed AFTER the rows and the device-side count in the recorded buffers have changed:
every replay must give what the family's CPU restatement gives for the data then in the buffers.  Also pinned: what a call
does when it finds the stream capturing and would have to allocate (refused before any side effect, with the remedy in the
message), that a scratch block a graph may point into is retired and not freed when the arena grows, and that per-kernel
timing records nothing on a capturing stream.

One recording idiom throughout (_Stage): a stream of the test's own made current, contexts of the test's own bound to it,
gc.collect() before the capture, capture_error_mode="relaxed", the stream made current again after it, graphs dropped
before the contexts are closed.  Every graph is a single chain recorded from that one stream."""
import gc

import numpy as np
import pytest

import affine_ref as AR
import align3d_ref as XR
import essential_ref as ER
import homography_ref as HR
import homography_refine_ref as HRR
import pnp_ref as PR
import points_matching_amd as pm
import triangulate_ref as T
import twoview_refine_ref as TV
from points_matching_amd import api, synth

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")]

CAP = 1024               # rows of every recorded buffer; the count lives on the device
PAD = 64                 # bytes behind a mask that no call may touch
IDS = 300                # model ids of a run: three workgroups of WG_IDS, the last one partial (44 ids)
WG_IDS = 128
U64 = (1 << 64) - 1
KMAT = np.array([[800.0, 0.0, 500.0], [0.0, 850.0, 330.0], [0.0, 0.0, 1.0]])
K = (800.0, 850.0, 500.0, 330.0)
G_F64, G_F32, G_U8, G_I32, G_I64 = 7.0, 7.0, 0xAB, -77, -77
REMEDY = "eager call"    # what the refusal's message must name


def _bits(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)


def _info_ref(i):
    return (int(_bits(i.cost_in)[0]), int(_bits(i.cost_out)[0]), int(i.n_used), int(i.iters), int(i.status))


def _info_dev(raw):
    r = raw.view(api.H_REFINE_INFO_DTYPE)[0]
    return (int(_bits(r["cost_in"])[0]), int(_bits(r["cost_out"])[0]), int(r["n_used"]), int(r["iters"]), int(r["status"]))


class _AInfo:
    """affine_ref.refine's tuple as an info record (the refit runs no iterations)."""

    def __init__(self, st, ci, co, nu):
        self.cost_in, self.cost_out, self.n_used, self.iters, self.status = ci, co, nu, 0, st


# ---- the families: shapes, scenes, the recorded calls and the restatement of the same chain -----------------------------------
class _Fam:
    def __init__(self, name, dim1, dim2, words, min_pts, per_sample, thr, opt=None, model=0):
        self.name, self.dim1, self.dim2, self.words, self.min_pts = name, dim1, dim2, words, min_pts
        self.samples = IDS // per_sample                    # sample ids [0, samples): IDS model ids
        self.thr, self.opt, self.model = thr, opt, model
        self.kind = name.split("-")[0]
        self.extra = {"Rt": 12, "E2": 9} if self.kind == "E" else {}


FAMS = {f.name: f for f in (
    _Fam("F-form1", 2, 2, 9, 8, 1, 1.0, opt=(api.PM_OPT_RANSAC_FORM, 1)),
    _Fam("F-form2", 2, 2, 9, 8, 1, 1.0, opt=(api.PM_OPT_RANSAC_FORM, 2)),
    _Fam("H", 2, 2, 9, 4, 1, 2.0),
    _Fam("A-full", 2, 2, 6, 3, 1, 2.0, model=api.PM_AFFINE_FULL),
    _Fam("A-partial", 2, 2, 6, 2, 1, 2.0, model=api.PM_AFFINE_PARTIAL),
    _Fam("E", 2, 2, 9, 5, 10, 1.0),
    _Fam("P", 3, 2, 12, 4, 4, 3.0),
    _Fam("X-rigid", 3, 3, 13, 3, 1, 0.05, model=api.PM_ALIGN3D_RIGID),
    _Fam("X-similarity", 3, 3, 13, 3, 1, 0.05, model=api.PM_ALIGN3D_SIMILARITY),
)}
SEED = 0xC0FFEE


def _scene(f, seed, n):
    """n rows of the family's two arrays, the camera being K wherever there is one."""
    if f.kind == "F":
        return synth.two_view(n, seed=seed)[:2]
    if f.kind == "H":
        return synth.planar_view(n, seed=seed)[:2]
    if f.kind == "A":
        return synth.affine_view(n, seed=seed, partial=f.model == api.PM_AFFINE_PARTIAL)[:2]
    if f.kind == "E":
        return synth.calibrated_view(n, seed=seed, K=KMAT)[:2]
    if f.kind == "P":
        return synth.pnp_scene(n, seed=seed, K=KMAT)[:2]
    return synth.align3d_scene(n, seed=seed, model=f.model)[:2]


def _want(f, oracle, a1, a2, n):
    """The restatement's result of the recorded chain on rows [0, n): the run, then its refinement (E: pose recovery and the
    refinement of the pose).  Below the family's minimum the run's outputs are the contract's (key 0, zero model, zero mask,
    count 0) and the later steps are the restatement's on exactly those."""
    a1, a2 = np.ascontiguousarray(a1[:n]), np.ascontiguousarray(a2[:n])
    w = {}
    if n < f.min_pts:
        key, model, mask, ninl = 0, np.zeros(f.words), np.zeros(n, np.uint8), 0
    elif f.kind == "F":
        _, model, mask, ninl, key = oracle.ransac_fundamental(a1, a2, f.samples, f.thr, SEED)
    elif f.kind == "H":
        key, model, mask, ninl = HR.run(a1, a2, f.samples, f.thr, SEED)
    elif f.kind == "A":
        key, model, mask, ninl = AR.run(f.model, a1, a2, f.samples, f.thr, SEED)
    elif f.kind == "E":
        key, model, mask, ninl = ER.run(a1, a2, K, f.samples, f.thr, SEED)
    elif f.kind == "P":
        key, model, mask, ninl = PR.run(a1, a2, K, f.samples, f.thr, SEED)
    else:
        key, model, mask, ninl = XR.run(f.model, a1, a2, f.samples, f.thr, SEED)
    model = np.asarray(model, np.float64).reshape(-1)
    if f.kind == "F":
        ref, info = TV.f_refine(a1, a2, mask, model, 10)
    elif f.kind == "H":
        ref, info = HRR.refine(a1, a2, mask, model, 10)
    elif f.kind == "A":
        st, ref, ci, co, nu = AR.refine(f.model, a1, a2, mask, model)
        info = _AInfo(st, ci, co, nu)
    elif f.kind == "E":
        ng, R, t, mo, _, _ = ER.recover_pose(a1, a2, K, model, mask)
        w["Rt"] = np.r_[R.reshape(-1), t]
        w["mo"], w["ng"] = mo, max(ng, 0)
        R2, t2, E2, info = TV.pose_refine(a1, a2, K, mo, R, t, 20)
        ref, w["E2"] = np.r_[R2.reshape(-1), t2], E2.reshape(-1)
    elif f.kind == "P":
        ref, info = PR.refine(a1, a2, K, mask, model, 20)
    else:
        ref, info = XR.refine(f.model, a1, a2, mask, model)
    w.update(key=int(key), model=model, mask=mask, ninl=int(ninl), refined=np.asarray(ref, np.float64).reshape(-1), info=_info_ref(info))
    return w


class _Stage:
    """A stream of the test's own, made current; contexts bound to it; everything released on exit, graphs first."""

    def __enter__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.st = torch.cuda.Stream(device=self.dev)
        self.prev = torch.cuda.current_stream(self.dev)
        torch.cuda.set_stream(self.st)
        self.ctxs, self.graphs = [], []
        return self

    def context(self, opts=()):
        c = pm.Context(0)
        self.ctxs.append(c)
        c.set_stream(self.st.cuda_stream)
        for o, v in opts:
            c.set_option(o, v)
        return c

    def close(self, c):
        self.torch.cuda.synchronize()
        self.ctxs.remove(c)
        c.close()

    def record(self, fn):
        """fn() recorded into a graph; an exception of fn leaves through here after the capture has been ended."""
        gc.collect()                     # no finaliser of an earlier test's context (hipFree) inside the capture
        g = self.torch.cuda.CUDAGraph()
        try:
            with self.torch.cuda.graph(g, stream=self.st, capture_error_mode="relaxed"):
                fn()
        finally:
            self.torch.cuda.set_stream(self.st)
        self.graphs.append(g)
        return g

    def refused(self, fn):
        """fn() under capture must be refused with PM_E_UNSUPPORTED and the remedy in the message."""
        with pytest.raises(pm.api.PmError) as err:
            self.record(fn)
        assert err.value.status == api.PM_E_UNSUPPORTED, err.value
        assert "capturing" in str(err.value) and REMEDY in str(err.value), err.value

    def drop_graphs(self):
        self.torch.cuda.synchronize()
        self.graphs.clear()
        gc.collect()

    def __exit__(self, *a):
        self.drop_graphs()
        self.torch.cuda.set_stream(self.prev)
        for c in self.ctxs:
            c.close()
        return False


class _Rig:
    """The recorded buffers of one family: two row arrays of CAP rows, the count, and every output of the chain."""

    def __init__(self, stage, f):
        t, dev = stage.torch, stage.dev
        self.t, self.f = t, f
        self.d1 = t.zeros((CAP, f.dim1), dtype=t.float32, device=dev)
        self.d2 = t.zeros((CAP, f.dim2), dtype=t.float32, device=dev)
        self.cnt = t.zeros(1, dtype=t.int32, device=dev)
        self.key = t.zeros(1, dtype=t.int64, device=dev)
        self.model = t.zeros(f.words, dtype=t.float64, device=dev)
        self.mask = t.zeros(CAP + PAD, dtype=t.uint8, device=dev)
        self.ninl = t.zeros(1, dtype=t.int32, device=dev)
        self.refined = t.zeros(12 if f.kind == "E" else f.words, dtype=t.float64, device=dev)
        self.info = t.zeros(32, dtype=t.uint8, device=dev)
        self.Rt = t.zeros(12, dtype=t.float64, device=dev)
        self.E2 = t.zeros(9, dtype=t.float64, device=dev)
        self.mo = t.zeros(CAP + PAD, dtype=t.uint8, device=dev)
        self.ng = t.zeros(1, dtype=t.int32, device=dev)
        p = lambda x: x.data_ptr()
        self.view = api.PointsView(p(self.d1), p(self.d2), p(self.cnt), 1, CAP, 0, 1, 0)
        self.pnp = api.PnpView(p(self.d1), p(self.d2), p(self.cnt), CAP, 0)
        self.xyz = api.XyzView(p(self.d1), p(self.d2), p(self.cnt), CAP, 0)

    def load(self, a1, a2, n):
        """Rows [0, n) and the count, on the stream; the rows behind the count hold garbage (finite and not)."""
        rng = np.random.default_rng(n)
        for d, a in ((self.d1, a1), (self.d2, a2)):
            h = rng.uniform(-3e4, 3e4, tuple(d.shape)).astype(np.float32)
            h[n + 1::7] = np.nan
            h[n + 2::11, 0] = np.inf
            h[:n] = a[:n]
            d.copy_(self.t.from_numpy(h))
        self.cnt.fill_(n)

    def guard(self):
        for x, v in ((self.key, G_I64), (self.model, G_F64), (self.mask, G_U8), (self.ninl, G_I32), (self.refined, G_F64),
                     (self.info, G_U8), (self.Rt, G_F64), (self.E2, G_F64), (self.mo, G_U8), (self.ng, G_I32)):
            x.fill_(v)

    def run(self, c, samples=None, refine=True):
        """The chain of the family, enqueued on c's stream: the run, then the second steps."""
        f, p = self.f, (lambda x: x.data_ptr())
        s = f.samples if samples is None else samples
        out = (p(self.key), p(self.model), p(self.mask), CAP, p(self.ninl))
        if f.kind == "F":
            c.ransac_run_dev(p(self.d1), p(self.d2), CAP, p(self.cnt), 0, s, f.thr, SEED, p(self.key), p(self.model), p(self.mask),
                             p(self.ninl))
            if refine:
                c.fundamental_refine_dev(self.view, p(self.mask), p(self.model), 10, p(self.refined), p(self.info))
        elif f.kind == "H":
            c.ransac_homography_run_dev(self.view, 0, s, f.thr, SEED, *out)
            if refine:
                c.homography_refine_dev(self.view, p(self.mask), p(self.model), 10, p(self.refined), p(self.info))
        elif f.kind == "A":
            c.ransac_affine_run_dev(self.view, 0, s, f.thr, SEED, *out, model=f.model)
            if refine:
                c.affine_refine_dev(self.view, p(self.mask), p(self.model), p(self.refined), p(self.info), model=f.model)
        elif f.kind == "E":
            c.ransac_essential_run_dev(self.view, K, 0, s, f.thr, SEED, *out)
            if refine:
                c.recover_pose_dev(self.view, K, p(self.model), p(self.mask), p(self.Rt), p(self.Rt) + 72, p(self.mo), p(self.ng))
                c.pose_refine_dev(self.view, K, p(self.mo), p(self.Rt), 20, p(self.refined), p(self.E2), p(self.info))
        elif f.kind == "P":
            c.ransac_pnp_run_dev(self.pnp, K, 0, s, f.thr, SEED, *out)
            if refine:
                c.pnp_refine_dev(self.pnp, K, p(self.mask), p(self.model), 20, p(self.refined), p(self.info))
        else:
            c.ransac_align3d_run_dev(self.xyz, 0, s, f.thr, SEED, *out, model=f.model)
            if refine:
                c.align3d_refine_dev(self.xyz, p(self.mask), p(self.model), p(self.refined), p(self.info), model=f.model)

    def read(self):
        self.t.cuda.synchronize()
        names = ["key", "model", "mask", "ninl", "refined", "info"] + (["Rt", "E2", "mo", "ng"] if self.f.kind == "E" else [])
        return {k: getattr(self, k).cpu().numpy().copy() for k in names}

    def untouched(self):
        got = self.read()
        return all((v == g).all() for v, g in ((got["key"], G_I64), (got["model"], G_F64), (got["mask"], G_U8),
                                               (got["ninl"], G_I32), (got["refined"], G_F64), (got["info"], G_U8)))


def _assert_is(got, want, n, f, what):
    """Every output of the chain against the restatement: key, count, model bits, mask (zero from the count to CAP, guard
    bytes behind it), the refined model's bits and the info words; E: pose, pose mask, n_good and the refined pose's E."""
    assert int(got["key"][0]) & U64 == want["key"], (what, hex(int(got["key"][0]) & U64), hex(want["key"]))
    assert int(got["ninl"][0]) == want["ninl"], (what, got["ninl"], want["ninl"])
    assert (_bits(got["model"]) == _bits(want["model"])).all(), (what, got["model"], want["model"])
    assert (got["mask"][:n] == want["mask"]).all() and not got["mask"][n:CAP].any(), what
    assert (got["mask"][CAP:] == G_U8).all(), what
    assert (_bits(got["refined"]) == _bits(want["refined"])).all(), (what, got["refined"], want["refined"])
    assert _info_dev(got["info"]) == want["info"], (what, _info_dev(got["info"]), want["info"])
    if f.kind == "E":
        assert (_bits(got["Rt"]) == _bits(want["Rt"])).all() and (_bits(got["E2"]) == _bits(want["E2"])).all(), what
        assert (got["mo"][:n] == want["mo"]).all() and not got["mo"][n:CAP].any() and (got["mo"][CAP:] == G_U8).all(), what
        assert int(got["ng"][0]) == want["ng"], what


def _same_bytes(a, b):
    return a.keys() == b.keys() and all(a[k].tobytes() == b[k].tobytes() for k in a)


def _data(f):
    """Two seeded scenes with different counts, and a count below the family's minimum on the first one's rows."""
    a = _scene(f, 21, 700)
    b = _scene(f, 22, 513)
    return [("recorded data", a, 700), ("second scene", b, 513), ("below the minimum", a, f.min_pts - 1), ("first again", a, 700)]


# ---- 1. record once, replay on changed data and counts -----------------------------------------------------------------------
@pytest.mark.parametrize("fam", list(FAMS))
def test_record_and_replay_on_changed_data(oracle, fam):
    """After one eager call the chain (run, refinement; E: run, pose recovery, pose refinement) is recorded once and replayed
    four times: on the recorded data, on a second scene with another count, on a count below the family's minimum and on
    the first data again.  IDS ids at WG_IDS per workgroup: three workgroups, the last partial, so the arrival ticket, the
    slots and the last workgroup's scan all take part.  Outputs are guard-filled before each replay."""
    f = FAMS[fam]
    sets = _data(f)
    wants = [_want(f, oracle, a[0], a[1], n) for _, a, n in sets]
    assert wants[0]["key"] and wants[1]["key"] and wants[0]["info"][4] == 0              # real models, a real refinement
    assert wants[2]["key"] == 0 and wants[2]["info"][4] == 2                            # "no model"
    with _Stage() as s:
        c = s.context([(api.PM_OPT_RANSAC_WG_IDS, WG_IDS)] + ([f.opt] if f.opt else []))
        rig = _Rig(s, f)
        rig.load(sets[0][1][0], sets[0][1][1], sets[0][2])
        rig.guard()
        rig.run(c)                                           # the eager call the contract asks for
        eager = rig.read()
        _assert_is(eager, wants[0], sets[0][2], f, "eager")
        rig.guard()
        g = s.record(lambda: rig.run(c))
        assert rig.untouched()                               # recording runs nothing
        got = []
        for (what, a, n), want in zip(sets, wants):
            rig.load(a[0], a[1], n)
            rig.guard()
            g.replay()
            got.append(rig.read())
            _assert_is(got[-1], want, n, f, what)
        assert _same_bytes(got[0], eager) and _same_bytes(got[3], got[0])               # nothing carried over
        assert c.scratch_info()[1] == 0


# ---- 2. the chain of test_triangulate_gpu.py::test_chain_pose_map_pnp_on_one_stream, recorded as one graph -------------------
CHAIN_CAP = 1536
CHAIN_SCENES = ((8, 1500), (5, 1200))        # (seed, count); the first is that test's scene


def _chain_scene(seed, n):
    xy0, xy1, _, R01, t01, X, _ = synth.calibrated_view(n, seed=seed, K=KMAT, outlier_frac=0.2, noise_px=0.3)
    a = np.radians(4.0)
    R02 = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t02 = np.array([1.6, 0.1, -0.3])
    Xc = X @ R02.T + t02
    uv2 = (np.c_[K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]] +
           np.random.default_rng(seed).normal(0, 0.3, (n, 2))).astype(np.float32)
    return xy0, xy1, uv2, R02, t02


def chain_ref(xy0, xy1, uv2):
    """The restatements chained as the device chain is: (Rt of view 1, map, status, PnP key, mask, count, refined pose)."""
    n = xy0.shape[0]
    _, E, m, _ = ER.run(xy0, xy1, K, 1000, 1.0, 3)
    _, R, t, mo, _, _ = ER.recover_pose(xy0, xy1, K, E, m)
    R, t, _, _ = TV.pose_refine(xy0, xy1, K, mo, R, t, 20)
    Rt = np.r_[R.reshape(-1), t]
    tri = T.run(K, [xy0, xy1], [None, Rt], 3.0, 0.9998, 50.0, 10)
    k2, Rt2, m2, c2 = PR.run(tri.xyz, uv2, K, 1000, 3.0, 5)
    Rt2r, info = PR.refine(tri.xyz, uv2, K, m2, Rt2, 20)
    return Rt, tri, k2, m2, c2, Rt2r, n


def _rot_deg(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def test_recorded_chain_pose_map_pnp():
    """E run, pose recovery, pose refinement into the 12 doubles that triangulation reads, triangulation, PnP run over the
    map with its NaN rows, PnP refinement: one graph after an eager warm-up, replayed on two scenes that differ in seed and
    count.  Two runs reset and re-carve the same arena inside the graph.  Every output of a replay equals, byte for byte,
    the eager chain of a context that never captured, and the restatements' chain; the final pose meets the tolerances of
    the eager chain test."""
    with _Stage() as s:
        t, dev = s.torch, s.dev
        p = lambda x: x.data_ptr()
        d0, d1, d2 = (t.zeros((CHAIN_CAP, 2), dtype=t.float32, device=dev) for _ in range(3))
        cnt = t.zeros(1, dtype=t.int32, device=dev)
        out = {"k": t.zeros(1, dtype=t.int64, device=dev), "E": t.zeros(9, dtype=t.float64, device=dev),
               "m": t.zeros(CHAIN_CAP, dtype=t.uint8, device=dev), "c": t.zeros(1, dtype=t.int32, device=dev),
               "Rt": t.zeros(12, dtype=t.float64, device=dev), "mo": t.zeros(CHAIN_CAP, dtype=t.uint8, device=dev),
               "ng": t.zeros(1, dtype=t.int32, device=dev), "xyz": t.zeros((CHAIN_CAP, 3), dtype=t.float32, device=dev),
               "st": t.zeros(CHAIN_CAP, dtype=t.uint8, device=dev), "good": t.zeros(1, dtype=t.int32, device=dev),
               "k2": t.zeros(1, dtype=t.int64, device=dev), "Rt2": t.zeros(12, dtype=t.float64, device=dev),
               "m2": t.zeros(CHAIN_CAP, dtype=t.uint8, device=dev), "c2": t.zeros(1, dtype=t.int32, device=dev),
               "Rt2r": t.zeros(12, dtype=t.float64, device=dev), "info": t.zeros(32, dtype=t.uint8, device=dev)}
        view = api.PointsView(p(d0), p(d1), p(cnt), 1, CHAIN_CAP, 0, 1, 0)
        tv = api.tri_views([p(d0), p(d1)], [None, p(out["Rt"])], CHAIN_CAP, p(cnt))
        pv = api.PnpView(p(out["xyz"]), p(d2), p(cnt), CHAIN_CAP, 0)

        def chain(c):
            c.ransac_essential_run_dev(view, K, 0, 1000, 1.0, 3, p(out["k"]), p(out["E"]), p(out["m"]), CHAIN_CAP, p(out["c"]))
            c.recover_pose_dev(view, K, p(out["E"]), p(out["m"]), p(out["Rt"]), p(out["Rt"]) + 72, p(out["mo"]), p(out["ng"]))
            c.pose_refine_dev(view, K, p(out["mo"]), p(out["Rt"]), 20, p(out["Rt"]))
            c.triangulate_dev(tv, K, api.tri_params(3.0, 0.9998, 50.0, 10), p(out["xyz"]), p(out["st"]), None, None, p(out["good"]))
            c.ransac_pnp_run_dev(pv, K, 0, 1000, 3.0, 5, p(out["k2"]), p(out["Rt2"]), p(out["m2"]), CHAIN_CAP, p(out["c2"]))
            c.pnp_refine_dev(pv, K, p(out["m2"]), p(out["Rt2"]), 20, p(out["Rt2r"]), p(out["info"]))

        def load(sc, n):
            for d, a in zip((d0, d1, d2), sc[:3]):
                h = np.full((CHAIN_CAP, 2), 12345.0, np.float32)
                h[:n] = a
                d.copy_(t.from_numpy(h))
            cnt.fill_(n)
            for k, v in out.items():
                v.fill_(G_U8 if v.dtype == t.uint8 else 7)

        def read():
            t.cuda.synchronize()
            return {k: v.cpu().numpy().copy() for k, v in out.items()}

        scenes = [(_chain_scene(seed, n), n) for seed, n in CHAIN_SCENES]
        c = s.context()
        load(*scenes[0])
        chain(c)                                             # eager warm-up: the larger of the two runs' scratch
        t.cuda.synchronize()
        g = s.record(lambda: chain(c))
        fresh = s.context()                                  # never sees a capture
        for sc, n in scenes + scenes[:1]:
            load(sc, n)
            g.replay()
            got = read()
            load(sc, n)
            chain(fresh)
            eager = read()
            assert _same_bytes(got, eager), [k for k in got if got[k].tobytes() != eager[k].tobytes()]
            Rt, tri, k2, m2, c2, Rt2r, _ = chain_ref(*sc[:3])
            assert (_bits(got["Rt"]) == _bits(Rt)).all()
            assert (got["xyz"][:n].view(np.uint32) == tri.xyz.view(np.uint32)).all() and (got["xyz"][n:] == 7.0).all()
            assert (got["st"][:n] == tri.status).all() and (got["st"][n:] == G_U8).all() and int(got["good"][0]) == tri.n_good
            assert int(got["k2"][0]) & U64 == k2 and int(got["c2"][0]) == c2 and (got["m2"][:n] == m2).all() and not got["m2"][n:].any()
            assert (_bits(got["Rt2r"]) == _bits(Rt2r)).all()
            ok = got["st"][:n] == T.OK
            assert ok.sum() > 0.7 * n and not got["m2"][:n][~ok].any() and c2 >= 0.9 * ok.sum()
            R2, t2 = got["Rt2r"][:9].reshape(3, 3), got["Rt2r"][9:]
            assert _rot_deg(R2, sc[3]) < 0.5 and np.linalg.norm(t2 - sc[4]) < 0.05 * np.linalg.norm(sc[4]), (R2, t2)


# ---- 3. the capturable calls that take no scratch: the gathers and the 3-D transform ------------------------------------------
@pytest.mark.parametrize("call", ["gather_pnp", "gather_align3d", "transform_points3"])
def test_gathers_and_transform_record_on_a_fresh_context(call):
    """Recorded on a context that never made an eager call (they allocate nothing), replayed twice with another device count
    and other rows each time.  Reference: numpy indexing with NaN rows for indices out of range; the restatement's transform.
    (pm_transform_points_dev belongs to the image family and refuses capture: tests/test_warp_gpu.py.)"""
    cap, n_a, n_b = 300, 40, 30
    rng = np.random.default_rng(3)
    with _Stage() as s:
        t, dev = s.torch, s.dev
        c = s.context()
        p = lambda x: x.data_ptr()
        cnt = t.zeros(1, dtype=t.int32, device=dev)
        wa, wb = (2, 3) if call == "gather_pnp" else (3, 3)
        o1 = t.zeros((cap, wa), dtype=t.float32, device=dev)
        o2 = t.zeros((cap, wb), dtype=t.float32, device=dev)
        if call == "transform_points3":
            dT = t.zeros(13, dtype=t.float64, device=dev)
            dx = t.zeros((cap, 3), dtype=t.float32, device=dev)
            g = s.record(lambda: c.transform_points3_dev(p(dT), p(dx), p(cnt), cap, p(o1)))
        else:
            dm = t.zeros(cap * 16, dtype=t.uint8, device=dev)
            ta = t.zeros((n_a, wa), dtype=t.float32, device=dev)
            tb = t.zeros((n_b, wb), dtype=t.float32, device=dev)
            fn = c.gather_pnp_dev if call == "gather_pnp" else c.gather_align3d_dev
            g = s.record(lambda: fn(p(dm), p(cnt), cap, p(ta), n_a, p(tb), n_b, p(o1), p(o2)))
        for n in (257, 64):
            o1.fill_(G_F32)
            o2.fill_(G_F32)
            cnt.fill_(n)
            if call == "transform_points3":
                x = rng.uniform(-50, 50, (cap, 3)).astype(np.float32)
                x[5], x[17, 1] = np.nan, np.inf
                _, _, sc, Rg, tg, _ = synth.align3d_scene(3, seed=n, model=XR.SIMILARITY)
                Tm = XR.pack(sc, Rg, tg)
                dT.copy_(t.from_numpy(Tm))
                dx.copy_(t.from_numpy(x))
                g.replay()
                t.cuda.synchronize()
                o = o1.cpu().numpy()
                assert (o[:n].view(np.uint32) == XR.transform(Tm, x[:n]).view(np.uint32)).all() and (o[n:] == G_F32).all()
                continue
            m = np.zeros(cap, api.MATCH_DTYPE)
            m["queryIdx"], m["trainIdx"] = rng.integers(0, n_a, cap), rng.integers(0, n_b, cap)
            m["queryIdx"][3], m["trainIdx"][7], m["trainIdx"][8], m["queryIdx"][9] = n_a, -1, n_b, -5
            a, b = rng.uniform(-5, 5, (n_a, wa)).astype(np.float32), rng.uniform(-5, 5, (n_b, wb)).astype(np.float32)
            dm.copy_(t.from_numpy(m.view(np.uint8)))
            ta.copy_(t.from_numpy(a))
            tb.copy_(t.from_numpy(b))
            g.replay()
            t.cuda.synchronize()
            h1, h2 = o1.cpu().numpy(), o2.cpu().numpy()
            q, tr = m["queryIdx"][:n], m["trainIdx"][:n]
            qok, tok = (q >= 0) & (q < n_a), (tr >= 0) & (tr < n_b)
            assert (h1[:n][qok] == a[q[qok]]).all() and np.isnan(h1[:n][~qok]).all() and (h1[n:] == G_F32).all()
            assert (h2[:n][tok] == b[tr[tok]]).all() and np.isnan(h2[:n][~tok]).all() and (h2[n:] == G_F32).all()
        assert c.scratch_info() == (0, 0)


# ---- 4. the first call under capture, and a call that would have to grow the scratch --------------------------------------------
BIG_SAMPLES = 16384      # with one id per workgroup: at least 2 MiB of slots, above the 1 MiB a small warm-up leaves


@pytest.mark.parametrize("fam", ["F-form2", "H", "A-full", "E", "P", "X-rigid"])
def test_run_under_capture_is_refused_before_any_side_effect_when_it_must_allocate(oracle, fam):
    """A *_run_dev call on a capturing stream that would have to allocate the arrival words or grow the scratch arena returns
    PM_E_UNSUPPORTED with the remedy in its message, before it allocates, synchronises or enqueues anything: the capture ends
    clean and empty, the outputs keep their guard values, the scratch capacity is what it was, and the context then gives
    the bytes of a context that never saw a capture.  Fresh context: refused.  Warmed context, larger shape: refused.
    Warmed context, the same shape: records, and the replay is the restatement's result."""
    f = FAMS[fam]
    _, a, n = _data(f)[0]
    want = _want(f, oracle, a[0], a[1], n)
    opts = [(api.PM_OPT_RANSAC_WG_IDS, WG_IDS)] + ([f.opt] if f.opt else [])
    with _Stage() as s:
        rig = _Rig(s, f)
        rig.load(a[0], a[1], n)
        never = s.context(opts)
        rig.guard()
        rig.run(never)
        base = rig.read()
        _assert_is(base, want, n, f, "never captured")
        c = s.context(opts)
        assert c.scratch_info() == (0, 0)
        rig.guard()
        s.refused(lambda: rig.run(c))                        # first call of the context
        assert rig.untouched() and c.scratch_info() == (0, 0)
        rig.run(c)
        assert _same_bytes(rig.read(), base)
        cap0 = c.scratch_info()[0]
        assert 0 < cap0 < BIG_SAMPLES * 128
        c.set_option(api.PM_OPT_RANSAC_WG_IDS, 1)
        rig.guard()
        s.refused(lambda: rig.run(c, samples=BIG_SAMPLES))   # warmed, but this shape needs more scratch
        assert rig.untouched() and c.scratch_info() == (cap0, 0)
        c.set_option(api.PM_OPT_RANSAC_WG_IDS, WG_IDS)
        g = s.record(lambda: rig.run(c))                     # warmed at this shape: records
        assert rig.untouched() and c.scratch_info() == (cap0, 0)
        g.replay()
        got = rig.read()
        _assert_is(got, want, n, f, "replay")
        assert _same_bytes(got, base)


@pytest.mark.parametrize("call", ["homography_refine", "triangulate"])
def test_calls_without_scratch_record_on_a_fresh_context(call):
    """A refinement and the triangulation take no scratch: their first call on a context may be the recorded one."""
    with _Stage() as s:
        t, dev = s.torch, s.dev
        c = s.context()
        if call == "homography_refine":
            f = FAMS["H"]
            _, a, n = _data(f)[0]
            _, H, mask, _ = HR.run(a[0], a[1], f.samples, f.thr, SEED)
            Hr, info = HRR.refine(a[0], a[1], mask, H, 10)
            rig = _Rig(s, f)
            rig.load(a[0], a[1], n)
            rig.guard()
            rig.model.copy_(t.from_numpy(H.reshape(-1).copy()))
            rig.mask[:n].copy_(t.from_numpy(mask))
            p = lambda x: x.data_ptr()
            g = s.record(lambda: c.homography_refine_dev(rig.view, p(rig.mask), p(rig.model), 10, p(rig.refined), p(rig.info)))
            assert (rig.refined == G_F64).all()
            g.replay()
            got = rig.read()
            assert (_bits(got["refined"]) == _bits(Hr)).all() and _info_dev(got["info"]) == _info_ref(info) and info.status == 0
        else:
            n, cap = 700, 1024
            Kt, uv, Rt, _ = T.scene(cap, 3, 4)[:4]
            Kt = tuple(float(v) for v in Kt)
            ref = T.run(Kt, [u[:n] for u in uv], Rt, 3.0, 0.9998, np.inf, 5)
            duv = [t.from_numpy(np.ascontiguousarray(u)).to(dev) for u in uv]
            dRt = [None if r is None else t.from_numpy(np.ascontiguousarray(r, np.float64).reshape(-1)).to(dev) for r in Rt]
            cnt = t.full((1,), n, dtype=t.int32, device=dev)
            xyz = t.full((cap, 3), G_F32, dtype=t.float32, device=dev)
            st = t.full((cap,), G_U8, dtype=t.uint8, device=dev)
            good = t.full((1,), G_I32, dtype=t.int32, device=dev)
            views = api.tri_views([u.data_ptr() for u in duv], [None if r is None else r.data_ptr() for r in dRt], cap, cnt.data_ptr())
            t.cuda.synchronize()
            g = s.record(lambda: c.triangulate_dev(views, Kt, api.tri_params(3.0, 0.9998, float("inf"), 5), xyz.data_ptr(),
                                                   st.data_ptr(), None, None, good.data_ptr()))
            g.replay()
            t.cuda.synchronize()
            x = xyz.cpu().numpy()
            assert (x[:n].view(np.uint32) == ref.xyz.view(np.uint32)).all() and (x[n:] == G_F32).all()
            assert (st.cpu().numpy()[:n] == ref.status).all() and int(good.item()) == ref.n_good
        assert c.scratch_info() == (0, 0)


# ---- 5. the scratch grows after a graph was recorded ---------------------------------------------------------------------------
def test_scratch_growth_after_recording_retires_the_block(oracle):
    """An E run is recorded at a small capacity; an eager E run of several times the scratch then grows the arena.  The block
    the graph's nodes point into must be retired, not freed: asserted on the host through pm_ctx_scratch_info BEFORE the one
    replay, so that a build without the rule fails here and never replays into freed memory.  Then the replay is the
    restatement's result, and a context created after this one was destroyed starts with nothing retired."""
    f = FAMS["E"]
    _, a, n = _data(f)[0]
    want = _want(f, oracle, a[0], a[1], n)
    with _Stage() as s:
        t, dev = s.torch, s.dev
        c = s.context([(api.PM_OPT_RANSAC_WG_IDS, WG_IDS)])
        rig = _Rig(s, f)
        rig.load(a[0], a[1], n)
        rig.guard()
        rig.run(c)
        cap0, retired0 = c.scratch_info()
        assert cap0 > 0 and retired0 == 0
        g = s.record(lambda: rig.run(c))
        assert c.scratch_info() == (cap0, 0)
        # the same entry point, eager: 32768 rows (300 of them counted) and 4096 samples, 3.2 MiB of candidates alone
        big_cap = 32768
        b1 = t.zeros((big_cap, 2), dtype=t.float32, device=dev)
        b2 = t.zeros((big_cap, 2), dtype=t.float32, device=dev)
        b1[:300].copy_(t.from_numpy(a[0][:300]))
        b2[:300].copy_(t.from_numpy(a[1][:300]))
        bcnt = t.full((1,), 300, dtype=t.int32, device=dev)
        bk, bE = t.zeros(1, dtype=t.int64, device=dev), t.zeros(9, dtype=t.float64, device=dev)
        bm, bc = t.zeros(big_cap, dtype=t.uint8, device=dev), t.zeros(1, dtype=t.int32, device=dev)
        bview = api.PointsView(b1.data_ptr(), b2.data_ptr(), bcnt.data_ptr(), 1, big_cap, 0, 1, 0)
        c.ransac_essential_run_dev(bview, K, 0, 4096, 1.0, SEED, bk.data_ptr(), bE.data_ptr(), bm.data_ptr(), big_cap, bc.data_ptr())
        t.cuda.synchronize()
        kr, Er, mr, cr = ER.run(a[0][:300], a[1][:300], K, 4096, 1.0, SEED)
        assert int(bk.item()) & U64 == kr and (_bits(bE.cpu().numpy()) == _bits(Er)).all() and int(bc.item()) == cr
        # ---- the guard: host-side, before any replay
        cap1, retired1 = c.scratch_info()
        assert cap1 >= 3 * cap0, (cap0, cap1)
        assert retired1 == 1, "the arena grew under a recorded graph and its old block was not retired: no replay"
        # ---- only now
        rig.guard()
        g.replay()
        _assert_is(rig.read(), want, n, f, "replay after the growth")
        # an eager call that fits changes nothing; a second growth, with no capture since the first, frees its block
        rig.run(c)
        assert c.scratch_info() == (cap1, 1)
        c.ransac_essential_run_dev(bview, K, 0, 3 * 4096, 1.0, SEED, bk.data_ptr(), bE.data_ptr(), bm.data_ptr(), big_cap, bc.data_ptr())
        t.cuda.synchronize()
        cap2, retired2 = c.scratch_info()
        assert cap2 > cap1 and retired2 == 1
        s.drop_graphs()
        s.close(c)
        assert s.context().scratch_info() == (0, 0)


# ---- 6. per-kernel timing and a capturing stream --------------------------------------------------------------------------------
def test_timing_records_nothing_on_a_capturing_stream():
    """With pm_ctx_timing_enable(1) a capturable call still records and replays; no event goes into the graph, so the captured
    call and the replays add nothing to pm_ctx_timing_get: the eager warm-up stays the one launch it reports."""
    f = FAMS["H"]
    _, a, n = _data(f)[0]
    key, H, mask, ninl = HR.run(a[0], a[1], f.samples, f.thr, SEED)
    with _Stage() as s:
        c = s.context([(api.PM_OPT_RANSAC_WG_IDS, WG_IDS)])
        c.timing_enable(True)
        rig = _Rig(s, f)
        rig.load(a[0], a[1], n)
        rig.run(c, refine=False)
        ms, launches = c.timing_get("ransac_h_fused")
        assert launches == 1 and ms > 0.0
        rig.guard()
        g = s.record(lambda: rig.run(c, refine=False))
        assert rig.untouched()
        for _ in range(2):
            rig.guard()
            g.replay()
            got = rig.read()
            assert int(got["key"][0]) & U64 == key and int(got["ninl"][0]) == ninl
            assert (_bits(got["model"]) == _bits(H)).all() and (got["mask"][:n] == mask).all() and not got["mask"][n:CAP].any()
        assert c.timing_get("ransac_h_fused") == (ms, 1)
        rig.run(c, refine=False)                             # and eager calls are timed as before
        assert c.timing_get("ransac_h_fused")[1] == 2
        c.timing_enable(False)
