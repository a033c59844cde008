"""CPU: the L2 matcher's route planner (csrc/knn_l2_plan.hpp), through a C shim built with the host compiler.

The golden table tests/golden/knn_l2_plan_cases.json holds requests with the plans that the dispatcher of the commit it
names produced (written by a harness around that commit's decision code, not by the planner); a route change edits the
table in the same diff.  The invariants need no earlier commit: they hold for every plan of a matrix route."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cref
from points_matching_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX, EXACT, WIDEN = 0, 1, 2
ROUTE_U8 = 3
PREP_U8ROWS = 0


@pytest.fixture(scope="module")
def planner():
    L = cref.load("knn_l2_plan_shim", {"knn_plan_fields": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]},
                  {"knn_plan_field_names": C.c_char_p},
                  include=[os.path.join(ROOT, "include"), os.path.join(ROOT, "points_matching_amd", "csrc")])
    names = L.knn_plan_field_names().decode().split(",")
    nopt = L.knn_plan_opt_count()

    def plan(req, opts):
        """req: n x 9 (nq, nt, dim, k, flags, n_cu, u8_rows, aligned, fuse), opts: n x PM_OPT_COUNT_ -> {field: n values}"""
        req = np.ascontiguousarray(req, np.int32)
        opts = np.ascontiguousarray(opts, np.int32)
        assert req.shape[1] == 9 and opts.shape == (req.shape[0], nopt)
        out = np.zeros((req.shape[0], len(names)), np.float64)
        assert L.knn_plan_fields(cref.ptr(req), cref.ptr(opts), req.shape[0], cref.ptr(out)) == len(names)
        return out

    plan.names, plan.nopt, plan.u8_shift = names, nopt, L.knn_plan_u8_shift()
    return plan


def test_plans_equal_the_golden_table(planner):
    with open(os.path.join(ROOT, "tests", "golden", "knn_l2_plan_cases.json")) as f:
        gold = json.load(f)
    assert len(gold["parent"]) == 40 and gold["plan_fields"] == planner.names
    cases = gold["cases"]
    assert len(cases) >= 300
    req = np.array([c["req"] for c in cases], np.int32)
    opts = np.zeros((len(cases), planner.nopt), np.int32)
    for i, c in enumerate(cases):
        for o, v in c["opts"].items():
            opts[i, int(o)] = v
    want = np.array([c["plan"] for c in cases], np.float64)
    got = planner(req, opts)
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(cases[i]["req"], cases[i]["opts"], planner.names[j], got[i, j], want[i, j]) for i, j in bad[:10]]
    # the table is worth something: every verdict, every route, both refinement kernels, every prep kernel
    col = {n: want[:, j] for j, n in enumerate(planner.names)}
    m = col["verdict"] == MATRIX
    assert set(col["verdict"]) == {MATRIX, EXACT, WIDEN} and m.sum() >= 150
    assert set(col["route"][m]) == {0, 1, 2, 3} and set(col["prep"][m]) == set(range(7)) and set(col["refine8"][m]) == {0, 1}
    assert set(col["prep_gen"][m]) == {0, 1, 2} and set(col["dp16"][m]) == {128, 256}


def _random_requests(rng, n, nopt):
    """Shapes on and around the tile, split and id-width boundaries, every flag combination, both pointer classes, u8 rows,
    fused tail, two device sizes, and none / one / two options at a documented value."""
    nq = rng.choice([1, 16, 17, 255, 256, 257, 512, 513, 768, 769, 8192, 32768, 200000], n)
    nt = rng.choice([0, 1, 127, 128, 129, 2048, 2049, 8192, 131072, 131073, 1 << 21, 7456412, 7456413, 1 << 24, (1 << 24) + 1], n)
    nq = np.where(rng.random(n) < 0.3, rng.integers(1, 70000, n), nq)
    nt = np.where(rng.random(n) < 0.3, rng.integers(0, 300000, n), nt)
    dim = rng.choice([1, 3, 4, 6, 20, 64, 128, 129, 132, 256, 257], n)
    k = np.where(rng.random(n) < 0.7, rng.integers(1, 5, n), rng.integers(1, api.PM_MAX_K + 1, n))
    flags = rng.integers(0, 32, n) & np.where(rng.random(n) < 0.6, ~api.PM_KNN_FORCE_EXACT, ~0)
    u8 = rng.random(n) < 0.3
    fuse = rng.random(n) < 0.5
    k = np.where(fuse & (rng.random(n) < 0.8), 2, k)
    req = np.stack([nq, nt, dim, k, np.where(u8, 0, flags), rng.choice([256, 64], n), u8, rng.random(n) < 0.8, fuse], 1)
    documented = {api.PM_OPT_KNN_F16_WAVES: 4, api.PM_OPT_KNN_STAGING: 3, api.PM_OPT_KNN_WG_PER_CU: 3, api.PM_OPT_KNN_XCD_TILE: 3,
                  api.PM_OPT_KNN_GENERAL_F16: 3, api.PM_OPT_KNN_SEEDED: 3, api.PM_OPT_KNN_U8_GROUP: 4, api.PM_OPT_KNN_RING: 7,
                  api.PM_OPT_KNN_U8_REFINE: 3, api.PM_OPT_KNN_RING_PROLOGUE: 9, api.PM_OPT_KNN_WIDE: 3,
                  api.PM_OPT_KNN_PREP_ROWS: 3, api.PM_OPT_KNN_SUPERTILE: 4}
    ids = np.array(sorted(documented))
    opts = np.zeros((n, nopt), np.int32)
    for _ in range(2):
        o = rng.choice(ids, n)
        v = (rng.random(n) * np.array([documented[i] for i in o])).astype(np.int32)
        v[(o == api.PM_OPT_KNN_RING_PROLOGUE) & (v == 1)] = 2
        on = rng.random(n) < 0.5
        opts[np.arange(n)[on], o[on]] = v[on]
    return req.astype(np.int32), opts


def test_invariants_of_every_matrix_plan(planner):
    """What the launcher and the kernels rely on, for 400 000 random requests.

    The 2048-row cap of an f16 / u8 split comes from the (ntiles + 15) / 16 rule and is overridden by the cap of 64
    splits: it holds up to 64 * 2048 = 131072 padded train rows, and always on the u8 route (whose 9 id bits allow no
    longer split; longer train sets leave that route).  Above, a split is as short as 64 splits allow.  The f32 geometry's
    rule is (ntiles + 31) / 32 and gives no such cap."""
    rng = np.random.default_rng(20261018)
    req, opts = _random_requests(rng, 400000, planner.nopt)
    out = planner(req, opts)
    f = {n: out[:, j] for j, n in enumerate(planner.names)}
    nq, nt, u8_rows = req[:, 0].astype(np.int64), req[:, 1].astype(np.int64), req[:, 6] != 0
    verdict = f["verdict"]
    # u8 rows never yield a plan that would read the null f32 pointers
    assert not (u8_rows & (verdict == EXACT)).any()
    m = verdict == MATRIX
    assert m.sum() > 50000 and (u8_rows & m).sum() > 5000
    assert (f["route"][u8_rows & m] == ROUTE_U8).all() and (f["refine8"][u8_rows & m] == 1).all()
    assert ((f["prep"] == PREP_U8ROWS) == u8_rows)[m].all()

    f = {n: v[m].astype(np.int64) if n.split(".")[-1] not in ("eps_coef", "embed_coef", "eps_coef_gen", "abs_gen") else v[m]
         for n, v in f.items()}
    nq, nt = nq[m], nt[m]
    u8r = f["route"] == ROUTE_U8

    def al(x):
        return (x + 255) // 256 * 256
    parts = ["qnorm_bytes", "tnorm_bytes", "c32", "c16", "qh", "th", "sdb", "pkb", "qfb"]
    assert (f["need"] == sum(al(f[p]) for p in parts) + 2048).all()
    assert (f["qnorm_bytes"] == 4 * nq).all() and (f["tnorm_bytes"] == 4 * nt).all()
    assert (f["c32"] == np.where(f["want32"] == 1, 4 * nq * f["g32.slots"], 0)).all()
    assert (f["c16"] == np.where(f["want16"] == 1, 4 * nq * f["g16.slots"], 0)).all()
    assert ((f["want32"] == 1) | (f["want16"] == 1)).all()

    # padding: whole workgroups of queries, whole tiles of train rows
    assert (f["nq_pad"] % 256 == 0).all() and (f["nq_pad"] % f["qb_wg"] == 0).all()
    assert (f["nq_pad"] >= nq).all() and (f["nq_pad"] - nq < np.maximum(f["qb_wg"], 256)).all()
    assert (f["nt_pad"] % 128 == 0).all() and (f["nt_pad"] >= nt).all() and (f["nt_pad"] - nt < 128).all()

    # splits: 1 .. 64, covering every tile, four list entries per split
    for g, sp, tiles in (("g32", "splits32", (nt + 63) // 64), ("g16", "splits16", f["nt_pad"] // 128)):
        s, tps = f[sp], f[g + ".tiles_per_split"]
        assert (s >= 1).all() and (s <= 64).all() and (s * tps >= tiles).all() and ((s - 1) * tps < tiles).all()
        assert (f[g + ".slots"] == 4 * s).all()
    assert (f["g32.rows_per_tile"] == 64).all() and (f["g16.rows_per_tile"] == 128).all()
    rows16 = f["g16.tiles_per_split"] * 128
    small = f["nt_pad"] <= 131072
    assert small.any() and (~small).any()
    assert (rows16[small | u8r] <= 2048).all()
    assert (f["g16.tiles_per_split"][~small] == (f["nt_pad"][~small] // 128 + 63) // 64).all()

    # the id embedded in a candidate: wide enough for a split's row groups, at most 16 bits; the u8 route's integer
    # candidates leave U8_SHIFT bits
    assert (f["lid_bits32"] <= 16).all() and (f["lid_bits16"] <= 16).all()
    assert ((1 << f["lid_bits32"]) >= f["g32.tiles_per_split"] * 16).all()
    assert ((1 << f["lid_bits16"]) >= f["g16.tiles_per_split"] * 32).all()
    assert u8r.sum() > 5000 and (f["lid_bits16"][u8r] <= planner.u8_shift).all()
    assert (f["g16.lid_mask"] == np.where(u8r, (1 << planner.u8_shift) - 1, (1 << f["lid_bits16"]) - 1)).all()
    assert (f["g16.int_shift"] == np.where(u8r, planner.u8_shift, 0)).all()

    # LDS-DMA staged copies are addressed with 32-bit byte offsets
    lim = 2 ** 31 - 1
    assert ((f["nt_pad"][u8r] + 128) * 128 < lim).all()
    wide = f["t_wide"] == 1
    assert wide.any() and ((nt[wide] + 3 * 128) * 144 < lim).all() and (f["th"][wide] == 144 * f["nt_pad"][wide]).all()
    s16 = f["f16s"] == 1
    assert s16.any() and ((f["nt_pad"][s16] + 128) * 256 < lim).all()

    # the refinement instantiation exists: NS covers the lists a lane (row of 16 lanes) has to hold
    r8 = f["refine8"] == 1
    assert (r8 == (u8r & (f["u8_int_refine"] == 1))).all()
    assert (f["refine_ns"][r8] * 16 >= np.minimum(f["g16.slots"][r8], 256)).all() and np.isin(f["refine_ns"][r8], [1, 2, 4, 8, 16]).all()
    slots = np.maximum(np.where(f["want16"] == 1, f["g16.slots"], 0), np.where(f["want32"] == 1, f["g32.slots"], 0))
    assert (f["refine_ns"][~r8] * 64 >= slots[~r8]).all() and np.isin(f["refine_ns"][~r8], [1, 2, 4, 8]).all()
    assert np.isin(f["refine_group"][r8], [4, 8, 16]).all() and np.isin(f["refine_km"], [2, 4]).all()
    assert (f["refine_km"][f["refine_fuse"] == 1] == 2).all()
    assert (f["kf_tile"] == np.where(r8, 16, 32)).all()
