"""GPU: the FlannBasedMatcher-compatible approximate matcher (csrc/flann.hip; main.cpp:44, the reference's active
matcher object; SURVEY.md 8f-4, docs/SPEC.md S17).  Parity against OpenCV's FLANN is unpinned twice over (the library
is absent and its trees come from C rand()), so the tests check what can be checked:
  * the forest is a valid kd-forest of the train set (every tree: each point in exactly one leaf, every leaf on the
    side of each cut its coordinates say) and is reproducible from the seed;
  * the HIP search equals an independently written CPU search (oracle) over the same forest, bit for bit;
  * recall against the exact matcher, with the numbers printed; more checks never hurt recall;
  * with checks >= the train size the search is exhaustive and equals the exact matcher.

Heap overflow (SPEC S17: a heap holds 1024 branches, pushes beyond that are dropped): on 16 trees over 8192 x 128
SIFT-like rows and 512 queries, the CPU search with a heap of 2^20 entries differs from the one with 1024 entries on
57 queries (k = 1) and 317 queries (k = 4) at checks = 2000, so the drop path is reached and decides results there;
at checks = 128 no query differs (0 of 512, both k).  The HIP search equals the 1024-entry CPU search at both."""
import numpy as np
import pytest

import points_matching_amd as pm
from points_matching_amd import synth
from util import assert_matches_equal

pytestmark = pytest.mark.gpu


def _check_forest(nodes, roots, train):
    """Every tree: each point in exactly one leaf, and every leaf on the side of EVERY cut above it that its coordinates
    say (child1: v[dim] <= cut, child2: v[dim] >= cut); 2 nt - 1 nodes per tree, each reached exactly once."""
    nt, dim = train.shape
    reached = np.zeros(nodes.shape[0], bool)
    for root in roots:
        seen = np.zeros(nt, bool)
        stack = [(int(root), [])]            # (node, constraints so far: (dim, value, side))
        while stack:
            i, cons = stack.pop()
            assert 0 <= i < nodes.shape[0] and not reached[i], i
            reached[i] = True
            nd = nodes[i]
            if nd["child1"] < 0:
                assert nd["child2"] < 0
                p = int(nd["divfeat"])
                assert 0 <= p < nt and not seen[p]
                seen[p] = True
                for d, v, side in cons:
                    assert train[p, d] <= v if side == 1 else train[p, d] >= v, (i, p, d, float(train[p, d]), float(v), side)
                continue
            d, v = int(nd["divfeat"]), np.float32(nd["divval"])
            assert 0 <= d < dim and nd["child2"] >= 0
            stack.append((int(nd["child1"]), cons + [(d, v, 1)]))
            stack.append((int(nd["child2"]), cons + [(d, v, 2)]))
        assert seen.all()
    assert nodes.shape[0] == len(roots) * (2 * nt - 1) and reached.all()


def _leaf_sets(nodes, i):
    """points under node i"""
    out, st = [], [int(i)]
    while st:
        j = st.pop()
        nd = nodes[j]
        if nd["child1"] < 0:
            out.append(int(nd["divfeat"]))
        else:
            st += [int(nd["child1"]), int(nd["child2"])]
    return out


def test_forest_is_a_valid_reproducible_kd_forest(ctx):
    w = synth.pair_workload(64, 700, 128, seed=3, kind="surf")
    ix = pm.api.FlannIndex(ctx, w["t"], trees=4, checks=32, seed=11)
    nodes, roots = ix.export()
    _check_forest(nodes, roots, w["t"])
    # cut consistency on the top levels of every tree: left subtree values <= cut <= right subtree values
    for root in roots:
        nd = nodes[root]
        left, right = _leaf_sets(nodes, nd["child1"]), _leaf_sets(nodes, nd["child2"])
        d, v = int(nd["divfeat"]), float(nd["divval"])
        assert (w["t"][left, d] <= v).all() and (w["t"][right, d] >= v).all()
        assert 0.2 < len(left) / 700 < 0.8                      # mean split of a unimodal coordinate: roughly balanced
    again = pm.api.FlannIndex(ctx, w["t"], trees=4, checks=32, seed=11).export()
    other = pm.api.FlannIndex(ctx, w["t"], trees=4, checks=32, seed=12).export()
    assert (again[0] == nodes).all() and (again[1] == roots).all()
    assert not (other[0] == nodes).all()
    assert len({int(nodes[r]["divfeat"]) for r in roots}) >= 1   # trees are drawn independently


@pytest.mark.parametrize("kind,nq,nt,dim,k", [("sift", 1000, 3000, 128, 1), ("surf", 700, 2500, 128, 2), ("surf", 300, 17, 64, 2),
                                              ("sift", 64, 1, 128, 1), ("surf", 513, 4097, 36, 4)])
def test_hip_search_equals_the_cpu_search_over_the_same_forest(ctx, oracle, kind, nq, nt, dim, k):
    w = synth.pair_workload(nq, nt, dim, seed=nq + nt, planted=0.5, kind=kind)
    ix = pm.api.FlannIndex(ctx, w["t"], seed=5)
    got = ix.knn(w["q"], k)
    nodes, roots = ix.export()
    want = oracle.flann_search(nodes, roots, w["t"], w["q"], k, 32)
    assert_matches_equal(got, want, "HIP kd-forest search vs CPU search")


def test_recall_against_the_exact_matcher(ctx, oracle, capsys):
    """The reference's sizes (SURF with hessianThreshold 8000: 10^2..10^3 keypoints) and BASELINE's 8k.  Recall is
    reported for all queries and for the TRUE matches (queries planted as noisy copies of a train row: the ones a
    matcher exists for).  Queries without a counterpart are uniform points in 128-D, where no tree search finds the
    nearest of thousands of equidistant rows in 32 checks — neither does FLANN."""
    rows = []
    for kind, n in (("surf", 300), ("surf", 1000), ("sift", 1000), ("sift", 8192)):
        w = synth.pair_workload(n, n, 128, seed=n, planted=0.5, kind=kind)
        exact = ctx.bf_knn_l2(w["q"], w["t"], 1)[:, 0]
        true = w["truth"] >= 0
        assert (exact["trainIdx"][true] == w["truth"][true]).mean() > 0.97         # the exact matcher finds the planted row
        rec, rec_true = {}, {}
        for checks in (8, 32, 128):
            ix = pm.api.FlannIndex(ctx, w["t"], trees=4, checks=checks, seed=1)
            got = ix.knn(w["q"], 1)[:, 0]
            hit = got["trainIdx"] == exact["trainIdx"]
            rec[checks], rec_true[checks] = float(hit.mean()), float(hit[true].mean())
            assert (got["distance"][hit].view(np.uint32) == exact["distance"][hit].view(np.uint32)).all()   # same bits when found
            assert (got["distance"][~hit] >= exact["distance"][~hit]).all()                                   # never better than exact
            ix.close()
        rows.append((kind, n, rec, rec_true))
        assert rec[8] <= rec[32] + 0.02 and rec[32] <= rec[128] + 0.02
        assert rec_true[32] > 0.4 and rec_true[128] > rec_true[32] - 0.02 and rec_true[128] > 0.7
    with capsys.disabled():
        for kind, n, rec, rt in rows:
            print("\nflann recall@1 %s %dx%d: checks 8/32/128 = %.3f / %.3f / %.3f   true matches only: %.3f / %.3f / %.3f"
                  % (kind, n, n, rec[8], rec[32], rec[128], rt[8], rt[32], rt[128]))


def test_exhaustive_checks_equal_the_exact_matcher(ctx):
    w = synth.pair_workload(400, 350, 128, seed=9, planted=0.5, kind="surf")
    ix = pm.api.FlannIndex(ctx, w["t"], trees=4, checks=100000, seed=2)
    got = ix.knn(w["q"], 2)
    exact = ctx.bf_knn_l2(w["q"], w["t"], 2)
    # exhaustive search examines every point: same neighbours and distances (FLANN keeps an EARLIER-examined point ahead
    # of an equal distance, the exact matcher the lower index: compare as sets of (distance, index) rows where they tie)
    same = (got["trainIdx"] == exact["trainIdx"]).all(axis=1)
    assert same.mean() > 0.99
    assert (got["distance"].view(np.uint32) == exact["distance"].view(np.uint32)).all()


def test_flann_argument_checks(ctx):
    w = synth.pair_workload(16, 40, 32, seed=1, kind="surf")
    with pytest.raises(pm.PmError):
        pm.api.FlannIndex(ctx, w["t"][:0])                          # empty train set
    with pytest.raises(pm.PmError):
        pm.api.FlannIndex(ctx, w["t"], trees=17)
    ix = pm.api.FlannIndex(ctx, w["t"])
    with pytest.raises(pm.PmError):
        ix.knn(w["q"], 5)                                           # k > 4
    assert ix.knn(w["q"][:0], 1).shape == (0, 1)
    one = pm.api.FlannIndex(ctx, w["t"][:1])                        # a single train row: every query matches it, no 2nd neighbour
    r = one.knn(w["q"], 2)
    assert (r["trainIdx"][:, 0] == 0).all() and (r["trainIdx"][:, 1] == -1).all() and np.isinf(r["distance"][:, 1]).all()


# ---- the forest at small, odd and degenerate train sets --------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 2, 3, 101, 102, 700])
def test_forest_is_valid_at_every_size_and_dimension(ctx, nt):
    """1, 2, 3 rows; 101 | 102 rows: all of a node | one more than the mean / variance sample (SPEC S17); 1..128 columns
    (below 5 the cut dimension is drawn among fewer than 5); 1 and 16 trees."""
    for dim in (1, 3, 36, 128):
        for kind in ("surf", "sift"):
            t = synth.pair_workload(8, nt, dim, seed=nt + dim, kind=kind)["t"]
            for trees in (1, 16):
                ix = pm.api.FlannIndex(ctx, t, trees=trees, checks=32, seed=3)
                nodes, roots = ix.export()
                assert roots.shape[0] == trees
                _check_forest(nodes, roots, t)
                ix.close()


def _with_duplicates(t, frac, seed):
    t = t.copy()
    n_dup = int(frac * t.shape[0])
    t[:n_dup] = t[np.random.default_rng(seed).integers(n_dup, t.shape[0], n_dup)]
    return t


@pytest.mark.parametrize("kind", ["surf", "sift"])
@pytest.mark.parametrize("trees", [1, 16])
def test_forest_is_valid_with_duplicate_and_identical_rows(ctx, oracle, kind, trees):
    """40 % exact duplicate rows, and all rows identical: nodes whose values are all equal.  The f32 mean of equal
    general floats is an ulp off them, so every value lies on one side of it (SPEC S17: `lim1 == count or lim2 == 0`);
    integer-valued rows have an exact mean (`lim1 == 0`, `lim2 == count`).  The build terminates with a valid forest,
    and the search over it equals the CPU search."""
    base = synth.pair_workload(64, 700, 36, seed=1, kind=kind)
    for name, t in (("dup40", _with_duplicates(base["t"], 0.4, 0)), ("identical", np.tile(base["t"][:1], (700, 1)))):
        ix = pm.api.FlannIndex(ctx, t, trees=trees, checks=32, seed=3)
        nodes, roots = ix.export()
        _check_forest(nodes, roots, t)
        q = np.concatenate([base["q"], t[:40]])
        assert_matches_equal(ix.knn(q, 4), oracle.flann_search(nodes, roots, t, q, 4, 32), name)
        ix.close()


def test_check_forest_rejects_a_corrupted_export(ctx):
    """The checker itself: a cut moved below the root (where only a walk that carries every constraint looks), a point
    listed twice, and a missing node are all found."""
    t = synth.pair_workload(8, 700, 36, seed=5, kind="surf")["t"]
    ix = pm.api.FlannIndex(ctx, t, trees=4, checks=32, seed=3)
    nodes, roots = ix.export()
    ix.close()
    _check_forest(nodes, roots, t)
    # an inner node three levels below a root: raise its cut above every value (its child2 side now violates >= cut),
    # then lower it below every value (child1 violates <= cut)
    i = int(roots[2])
    for _ in range(3):
        i = int(nodes[i]["child2"] if nodes[int(nodes[i]["child2"])]["child1"] >= 0 else nodes[i]["child1"])
    assert nodes[i]["child1"] >= 0
    for v in (t.max() + 1, t.min() - 1):
        bad = nodes.copy()
        bad[i]["divval"] = v
        with pytest.raises(AssertionError):
            _check_forest(bad, roots, t)
    # the smallest possible slip: one leaf of the child2 side holds a point an ulp below the cut
    leaf = _leaf_sets(nodes, nodes[i]["child2"])[0]
    d = int(nodes[i]["divfeat"])
    t2 = t.copy()
    t2[leaf, d] = np.nextafter(np.float32(nodes[i]["divval"]), np.float32(-np.inf))
    with pytest.raises(AssertionError):
        _check_forest(nodes, roots, t2)
    leaves = np.nonzero(nodes["child1"] < 0)[0]
    bad = nodes.copy()
    bad[leaves[0]]["divfeat"] = bad[leaves[1]]["divfeat"]            # one point twice, another never
    with pytest.raises(AssertionError):
        _check_forest(bad, roots, t)
    with pytest.raises(AssertionError):
        _check_forest(nodes[:-1], roots, t)


# ---- search: heap overflow, shapes, ties, non-finite queries, exhaustive, device form -------------------------------
def _differ(a, b):
    return ((a["trainIdx"] != b["trainIdx"]) | (a["distance"].view(np.uint32) != b["distance"].view(np.uint32))).any(axis=1)


@pytest.mark.parametrize("checks", [128, 2000])
@pytest.mark.parametrize("k", [1, 4])
def test_search_with_a_full_heap_equals_the_cpu_search(ctx, oracle, checks, k, capsys):
    """SPEC S17 "pushes beyond 1024 are dropped".  At checks = 2000 the drop path is reached and matters: the CPU search
    with room for 2^20 branches gives other neighbours for some queries (the counts are in the module docstring)."""
    w = synth.pair_workload(512, 8192, 128, seed=8192, planted=0.5, kind="sift")
    ix = pm.api.FlannIndex(ctx, w["t"], trees=16, checks=checks, seed=5)
    got = ix.knn(w["q"], k)
    nodes, roots = ix.export()
    ix.close()
    want = oracle.flann_search(nodes, roots, w["t"], w["q"], k, checks, heap_cap=1024)
    roomy = oracle.flann_search(nodes, roots, w["t"], w["q"], k, checks, heap_cap=1 << 20)
    n_diff = int(_differ(want, roomy).sum())
    with capsys.disabled():
        print("\nflann heap overflow: trees 16, 8192 x 128, checks %d, k %d: %d of 512 queries differ between heap 1024 and 2^20"
              % (checks, k, n_diff))
    if checks == 2000:
        assert n_diff >= 1
    assert_matches_equal(got, want, "HIP search vs CPU search, heap of 1024")


def test_k_and_query_counts_in_turn_on_one_index(ctx, oracle):
    w = synth.pair_workload(1000, 3000, 128, seed=77, planted=0.5, kind="surf")
    ix = pm.api.FlannIndex(ctx, w["t"], seed=5)
    nodes, roots = ix.export()
    for k in (1, 2, 3, 4, 1):
        assert_matches_equal(ix.knn(w["q"][:300], k), oracle.flann_search(nodes, roots, w["t"], w["q"][:300], k, 32), "k = %d" % k)
    for nq in (64, 1000, 5, 1000):                                   # the examined-point scratch grows and is reused
        assert_matches_equal(ix.knn(w["q"][:nq], 2), oracle.flann_search(nodes, roots, w["t"], w["q"][:nq], 2, 32), "nq = %d" % nq)
    ix.close()


@pytest.mark.parametrize("dim", [3, 7, 8, 9, 36, 100])
def test_dimensions_around_the_cooperative_group_of_eight(ctx, oracle, dim):
    w = synth.pair_workload(200, 1500, dim, seed=dim, planted=0.5, kind="surf")
    ix = pm.api.FlannIndex(ctx, w["t"], seed=5)
    nodes, roots = ix.export()
    _check_forest(nodes, roots, w["t"])
    for k in (1, 4):
        assert_matches_equal(ix.knn(w["q"], k), oracle.flann_search(nodes, roots, w["t"], w["q"], k, 32), "dim %d k %d" % (dim, k))
    ix.close()


def test_equal_distances_keep_the_order_of_examination(ctx, oracle):
    """Runs of identical train rows and queries equal to a train row: an equal distance goes behind the earlier examined
    one (SPEC S17), not to the lower index as in the exact matcher."""
    base = synth.pair_workload(8, 300, 64, seed=13, kind="sift")["t"]
    reps = np.random.default_rng(13).integers(1, 7, 300)
    t = np.repeat(base, reps, axis=0)
    q = np.concatenate([base[:200], t[::5][:100]])
    for checks in (32, 100000):
        ix = pm.api.FlannIndex(ctx, t, checks=checks, seed=5)
        nodes, roots = ix.export()
        got = ix.knn(q, 4)
        ix.close()
        assert_matches_equal(got, oracle.flann_search(nodes, roots, t, q, 4, checks), "runs of identical rows")
        assert (got["distance"][:, 0] == 0).mean() > 0.9             # the query's own row (or a copy) is found
        ties = got["distance"][:, 0] == got["distance"][:, 1]
        assert ties.sum() > 50 and (got["trainIdx"][ties, 0] > got["trainIdx"][ties, 1]).any()   # not the lowest-index rule


def test_non_finite_query_rows(ctx, oracle):
    w = synth.pair_workload(64, 1000, 36, seed=3, planted=0.5, kind="surf")
    q = w["q"].copy()
    q[5, 7] = np.nan
    q[11, 0] = np.inf
    q[12] = np.nan
    q[13, 35] = -np.inf
    ix = pm.api.FlannIndex(ctx, w["t"], seed=5)
    nodes, roots = ix.export()
    for k in (1, 3):
        got, want = ix.knn(q, k), oracle.flann_search(nodes, roots, w["t"], q, k, 32)
        for f in ("queryIdx", "trainIdx", "imgIdx"):
            assert (got[f] == want[f]).all(), f
        gn, wn = np.isnan(got["distance"]), np.isnan(want["distance"])
        assert (gn == wn).all()                                      # NaN distances compare as NaN, not by payload
        assert (got["distance"].view(np.uint32)[~gn] == want["distance"].view(np.uint32)[~wn]).all()
    ix.close()


@pytest.mark.parametrize("nt,k", [(350, 2), (3000, 4)])
def test_exhaustive_search_equals_the_cpu_search_with_its_tie_order(ctx, oracle, nt, k):
    w = synth.pair_workload(400, nt, 128, seed=9, planted=0.5, kind="sift")      # integer rows: equal distances occur
    t = np.concatenate([w["t"], w["t"][:50]])                                      # ... and certainly with copies
    ix = pm.api.FlannIndex(ctx, t, trees=4, checks=100000, seed=2)
    nodes, roots = ix.export()
    got = ix.knn(w["q"], k)
    ix.close()
    assert_matches_equal(got, oracle.flann_search(nodes, roots, t, w["q"], k, 100000), "exhaustive")


def test_device_form_on_torch_buffers_and_streams(ctx, oracle):
    """FlannIndex.knn_dev: query and output owned by torch, 256 sentinel bytes behind the output, equal to the host form;
    on the context's own stream and on a torch stream handed over with set_stream."""
    import torch
    dev = torch.device("cuda", 0)
    w = synth.pair_workload(777, 2500, 128, seed=41, planted=0.5, kind="surf")
    ix = pm.api.FlannIndex(ctx, w["t"], seed=5)
    host = {k: ix.knn(w["q"], k) for k in (1, 2, 4)}
    nodes, roots = ix.export()
    assert_matches_equal(host[2], oracle.flann_search(nodes, roots, w["t"], w["q"], 2, 32), "host form")

    def run(k, nq):
        dq = torch.from_numpy(w["q"][:nq]).to(dev)
        out = torch.full((nq * k * 16 + 256,), 0xA5, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream().synchronize()
        ix.knn_dev(dq.data_ptr(), nq, k, out.data_ptr())
        ctx.synchronize()
        o = out.cpu().numpy()
        assert (o[nq * k * 16:] == 0xA5).all(), "bytes behind the output were written"
        return o[:nq * k * 16].view(pm.api.MATCH_DTYPE).reshape(nq, k)

    for k, nq in ((2, 777), (1, 777), (4, 3), (4, 777), (2, 61)):
        assert_matches_equal(run(k, nq), host[k][:nq], "device form, own stream")
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        ctx.set_stream(s.cuda_stream)
        try:
            for k, nq in ((2, 777), (4, 130)):
                assert_matches_equal(run(k, nq), host[k][:nq], "device form, torch stream")
        finally:
            ctx.set_stream(0)
    assert_matches_equal(ix.knn(w["q"], 2), host[2], "host form afterwards")
    ix.close()
