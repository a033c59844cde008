"""GPU: the image database (docs/SPEC.md S107-S112).  Every comparison is bit for bit with the plain-C restatement
tests/bowdb_ref.c, doubles as u64: the id of every add and the whole dump after it, the weights and norms after both
setters and clear, the score of every image, and ids, scores, count and tails of every selection.  The cases are those of
bowdb_cases.py (the CPU file runs the same lists against an independent model); the device runs them through its _dev forms
with guard elements behind every output.  Shapes cover one word and 2^18, a partial wave and several per stretch in bow_add,
images of 1, 63, 64, 65 and 4097 entries in bow_score, S and Nq * Nd past 2^53, one selection workgroup with and without a
sort of its buffer, and the sliced selection (max_images above 32768)."""
import gc
import itertools
import os

import numpy as np
import pytest

import bowdb_cases as cases
import bowdb_ref as R
import points_matching_amd as pm
from points_matching_amd import api

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G_I32, G_F64 = -77, -5.0
PAD = 16                       # guard elements behind every output


def dev_hist(torch, h):
    return torch.from_numpy(np.ascontiguousarray(h, np.uint32).view(np.int32)).to(torch.device("cuda", 0))


class Dev:
    """api.BowDb behind the adapter interface of bowdb_cases: the _dev forms, guarded outputs, guards checked."""

    def __init__(self, ctx, K, max_images, max_entries):
        import torch
        self.t, self.dev = torch, torch.device("cuda", 0)
        self.ctx, self.K = ctx, K
        self.db = api.BowDb(ctx, K, max_images, max_entries)

    def close(self):
        self.ctx.synchronize()
        self.db.close()

    def add_many(self, hists):
        t = self.t
        n = hists.shape[0]
        d_h = dev_hist(t, hists)
        d_id = t.full((n + PAD,), G_I32, dtype=t.int32, device=self.dev)
        t.cuda.synchronize()
        for i in range(n):
            self.db.add_dev(d_h[i].data_ptr(), d_id.data_ptr() + 4 * i)
        self.ctx.synchronize()
        ids = d_id.cpu().numpy()
        assert (ids[n:] == G_I32).all()
        return ids[:n].copy()

    def set_weights(self, w):
        try:
            self.db.set_weights(w)
            return 0
        except api.PmError as e:
            assert e.status == api.PM_E_INVALID and "8191" in str(e)
            return -1

    def idf(self):
        self.db.idf_dev()

    def clear(self):
        self.db.clear_dev()

    def get(self):
        return self.db.get()

    def query(self, hist, top, lo, hi, want=(1, 1, 1, 1)):
        """want: which of d_ids, d_scores, d_count, d_all are passed; the others are NULL and come back as None."""
        t = self.t
        n = self.db.counts()[0]
        d_h = dev_hist(t, hist)
        d_ids = t.full((top + PAD,), G_I32, dtype=t.int32, device=self.dev)
        d_sc = t.full((top + PAD,), G_F64, dtype=t.float64, device=self.dev)
        d_cnt = t.full((1 + PAD,), G_I32, dtype=t.int32, device=self.dev)
        d_all = t.full((n + PAD,), G_F64, dtype=t.float64, device=self.dev)
        t.cuda.synchronize()
        ptrs = [b.data_ptr() if w else 0 for b, w in zip((d_ids, d_sc, d_cnt, d_all), want)]
        self.db.query_dev(d_h.data_ptr(), top, lo, hi, *ptrs)
        self.ctx.synchronize()
        ids, sc, cnt, every = d_ids.cpu().numpy(), d_sc.cpu().numpy(), d_cnt.cpu().numpy(), d_all.cpu().numpy()
        for a, used, guard, w in ((ids, top, G_I32, want[0]), (sc, top, G_F64, want[1]), (cnt, 1, G_I32, want[2]), (every, n, G_F64, want[3])):
            assert (a[used if w else 0:] == guard).all()
        return (ids[:top].copy() if want[0] else None, sc[:top].copy() if want[1] else None, int(cnt[0]) if want[2] else None,
                every[:n].copy() if want[3] else None)


class Ref:
    def __init__(self, K, max_images, max_entries):
        self.K, self.db = K, R.RefDb(K, max_images, max_entries)

    def add_many(self, hists):
        return np.array([self.db.add(h) for h in hists], np.int32)

    def __getattr__(self, name):
        return getattr(self.db, name)


def both(ctx, K, max_images, max_entries, ops):
    """Runs the list on the device and in the restatement; returns the device's results after comparing every one."""
    d = Dev(ctx, K, max_images, max_entries)
    try:
        got = cases.run(d, ops)
    finally:
        d.close()
    assert cases.same(got, cases.run(Ref(K, max_images, max_entries), ops)) == ""
    return got


# ---- S108 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", cases.ADD_KS)
def test_add(ctx, K):
    mi, me, ops, names = cases.add_case(K)
    res = both(ctx, K, mi, me, ops)
    ids = dict(zip(names, (int(r[0]) for r in res[0::2])))
    dumps = dict(zip(names, res[1::2]))
    assert ids["first_word"] == 0 and ids["T_65535"] >= 0 and ids["T_65536"] == -1 and ids["all_zero"] == -1, ids
    assert R.same_dump(dumps["T_65535"], dumps["T_65536"]) and R.same_dump(dumps["T_65535"], dumps["all_zero"])


@pytest.mark.parametrize("case", cases.limit_cases(), ids=lambda c: c[0])
def test_limits(ctx, case):
    name, K, mi, me, ops = case
    res = both(ctx, K, mi, me, ops)
    if name == "entries_full":
        assert [int(r[0]) for r in res[0:8:2]] == [0, 1, -2, -1] and res[3]["n_entries"] == 10
        assert R.same_dump(res[3], res[5]) and R.same_dump(res[3], res[7])
    else:
        assert res[0][0] == 0 and res[1][0] == 1 and res[3][0] == -2 and R.same_dump(res[2], res[4])


# ---- S109 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 48])
def test_weights(ctx, N):
    K, mi, me, ops = cases.weight_case(N)
    res = both(ctx, K, mi, me, ops)
    assert res[6] == 0 and res[9] == -1 and R.same_dump(res[7], res[10])          # 8192 is refused and changes nothing
    assert (res[12]["weights"] == res[7]["weights"]).all() and res[12]["n_images"] == 0   # clear keeps the weights


# ---- S110 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idf", [False, True], ids=["unit", "idf"])
def test_scene_scores(ctx, idf):
    K, mi, me, ops = cases.scene_case(idf)
    res = both(ctx, K, mi, me, ops)
    ids, scores, count, every = res[-24]
    assert ids[0] == 48 and scores[0] == cases.u64([1.0])[0] and every[48] == cases.u64([1.0])[0]
    for p, r in enumerate(res[-24:]):
        assert sorted(r[0][r[0] != 48][:2].tolist()) == [2 * p, 2 * p + 1]


@pytest.mark.parametrize("make", [cases.shapes_case, cases.range_case], ids=["shapes", "range"])
def test_shapes_and_range(ctx, make):
    K, mi, me, ops = make()
    res = both(ctx, K, mi, me, ops)
    every = res[3][3].view(np.float64)
    if make is cases.shapes_case:
        assert every[7] == 1.0 and every[5] == 0.0 and every[6] == 0.0 and (every[:5] > 0).all()
    else:
        assert every[0] == 1.0 and every[3] == 1.0 and res[3][0][:2].tolist() == [0, 3]


# ---- S111 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,max_images", [(n, None) for n in cases.SELECT_NS] + [(65, 40000), (5000, 70000)])
def test_selection(ctx, N, max_images):
    K, mi, me, ops = cases.selection_case(N, max_images)
    res = both(ctx, K, mi, me, ops)
    assert res[-3][2] == 0 and res[-2][2] == 0 and not res[-3][3].any() and not res[-2][3].any()    # the refused queries
    assert (res[-3][0] == -1).all() and (res[-3][1] == cases.u64([cases.QNAN])[0]).all()


@pytest.mark.parametrize("max_images", [300, 40000])
def test_null_outputs_in_every_combination(ctx, max_images):
    h = cases.tie_histograms(300, seed=5)
    q = np.array([1, 0, 2, 1, 0, 1, 0, 0], np.uint32)
    ref = Ref(8, max_images + 1, 2400)                                   # room for the one more image at the end
    ref.add_many(h)
    want = cases.run(ref, [("query", q, 7, 10, 20)])[0]
    d = Dev(ctx, 8, max_images + 1, 2400)
    try:
        d.add_many(h)
        for combo in itertools.product((0, 1), repeat=4):
            ids, sc, cnt, every = d.query(q, 7, 10, 20, want=combo)
            assert (ids is None) == (not combo[0]) and (sc is None) == (not combo[1]) and (cnt is None) == (not combo[2])
            assert ids is None or (ids == want[0]).all()
            assert sc is None or (cases.u64(sc) == want[1]).all()
            assert cnt is None or cnt == want[2]
            assert every is None or (cases.u64(every) == want[3]).all()
        d.db.add_dev(dev_hist(d.t, h[0]).data_ptr())                      # d_id may be NULL too
        assert d.db.counts()[0] == 301 and ref.add_many(h[:1])[0] == 300 and R.same_dump(d.get(), ref.get())
    finally:
        d.close()


# ---- S112 --------------------------------------------------------------------------------------------------------------------------
def test_host_forms_equal_the_device_forms(ctx):
    dbh, qs = cases.place_scene()
    ref = Ref(512, 48, 8000)
    ref.add_many(dbh)
    ref.idf()
    db = api.BowDb(ctx, 512, 48, 8000)
    try:
        assert [db.add(h) for h in dbh] == list(range(48)) and db.add(np.zeros(512, np.uint32)) == -1 and db.add(dbh[0]) == -2
        db.idf_dev()
        assert (db.get_weights() == ref.get()["weights"]).all() and R.same_dump(db.get(), ref.get())
        for q in qs[:4]:
            ids, scores, every = db.query(q, 6, 2, 4, all_scores=True)
            rid, rsc, rcount, revery = ref.query(q, 6, 2, 4)
            assert ids.size == rcount and (ids == rid[:rcount]).all() and (cases.u64(scores) == cases.u64(rsc[:rcount])).all()
            assert (cases.u64(every) == cases.u64(revery)).all()
            assert len(db.query(q, 1)) == 2
    finally:
        ctx.synchronize()
        db.close()


# ---- the chain on the fixtures -----------------------------------------------------------------------------------------------------
def read_pgm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"P5"
        line = f.readline()
        while line.startswith(b"#"):
            line = f.readline()
        w, h = (int(v) for v in line.split())
        assert int(f.readline()) == 255
        return np.frombuffer(f.read(w * h), np.uint8).reshape(h, w).copy()


def test_chain_describe_encode_add_query_on_the_fixtures(ctx):
    """Image 1 is described and its rows train a vocabulary of 64 words (the one readback is the row count the training call
    takes as a host argument).  Both images are uploaded and every buffer is allocated before that.  From there one stream, no
    readback and no host synchronisation: encode image 1 with its device count, query the empty
    database, add the image, describe and encode image 2, query, and an encoding under a device count of -1 whose add must be
    refused as empty.  Everything is compared on the downloaded histograms afterwards."""
    import torch
    dev = torch.device("cuda", 0)
    max_kp, K, nbytes = 512, 64, 32
    imgs = [read_pgm(os.path.join(GOLD, "img0%d_half.pgm" % i)) for i in (1, 2)]
    voc = api.Vocab(ctx, api.PM_VOCAB_BITS, nbytes, K, max_kp)
    db = api.BowDb(ctx, K, 4, 4 * K)
    try:
        def buffers(img):                                                # uploads and allocations: all before the chain
            return (torch.from_numpy(img).to(dev), torch.zeros((max_kp, 2), dtype=torch.float32, device=dev),
                    torch.full((max_kp, nbytes), 0x5A, dtype=torch.uint8, device=dev), torch.full((1,), -3, dtype=torch.int32, device=dev))

        def describe(img, keep):                                         # enqueues only
            h, w = img.shape
            ctx.detect_describe_bits_dev(keep[0].data_ptr(), w, h, w, max_kp, keep[1].data_ptr(), keep[2].data_ptr(), 0, keep[3].data_ptr())

        keep1, keep2 = buffers(imgs[0]), buffers(imgs[1])
        torch.cuda.synchronize()
        describe(imgs[0], keep1)
        ctx.synchronize()
        n1 = int(keep1[3].cpu().numpy()[0])
        assert 2 * K < n1 <= max_kp
        d_h = torch.full((3, K), 999, dtype=torch.int32, device=dev)
        d_id = torch.full((2 + PAD,), G_I32, dtype=torch.int32, device=dev)
        d_ids = torch.full((2, 3 + PAD), G_I32, dtype=torch.int32, device=dev)
        d_sc = torch.full((2, 3 + PAD), G_F64, dtype=torch.float64, device=dev)
        d_cnt = torch.full((2 + PAD,), G_I32, dtype=torch.int32, device=dev)
        d_neg = torch.full((1,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        voc.init_stride_dev(keep1[2].data_ptr(), n1)
        voc.train_dev(keep1[2].data_ptr(), n1, 5)                        # no readback, no synchronisation from here ...
        voc.assign_dev(keep1[2].data_ptr(), max_kp, keep1[3].data_ptr(), 0, 0, d_h[0].data_ptr())
        db.query_dev(d_h[0].data_ptr(), 3, 0, 0, d_ids[0].data_ptr(), d_sc[0].data_ptr(), d_cnt.data_ptr())
        db.add_dev(d_h[0].data_ptr(), d_id.data_ptr())
        describe(imgs[1], keep2)
        voc.assign_dev(keep2[2].data_ptr(), max_kp, keep2[3].data_ptr(), 0, 0, d_h[1].data_ptr())
        db.query_dev(d_h[1].data_ptr(), 3, 0, 0, d_ids[1].data_ptr(), d_sc[1].data_ptr(), d_cnt.data_ptr() + 4)
        voc.assign_dev(keep2[2].data_ptr(), max_kp, d_neg.data_ptr(), 0, 0, d_h[2].data_ptr())
        db.add_dev(d_h[2].data_ptr(), d_id.data_ptr() + 4)
        ctx.synchronize()                                                # ... to here
        h = d_h.cpu().numpy().view(np.uint32)
        n2 = int(keep2[3].cpu().numpy()[0])
        assert int(h[0].sum()) == n1 and int(h[1].sum()) == n2 and not h[2].any()
        ref = R.RefDb(K, 4, 4 * K)
        assert ref.add(h[0]) == 0
        rid, rsc, rcount, _ = ref.query(h[1], 3)
        assert rcount == 1 and rid[0] == 0 and 0.0 < rsc[0] < 1.0
        ids, sc, cnt, got_id = d_ids.cpu().numpy(), d_sc.cpu().numpy(), d_cnt.cpu().numpy(), d_id.cpu().numpy()
        assert got_id[:2].tolist() == [0, -1] and (got_id[2:] == G_I32).all()
        assert cnt[:2].tolist() == [0, 1] and (cnt[2:] == G_I32).all()
        assert (ids[0, :3] == -1).all() and np.isnan(sc[0, :3]).all()    # the empty database
        assert (ids[1, :3] == rid).all() and (cases.u64(sc[1, :3]) == cases.u64(rsc)).all()
        assert (ids[:, 3:] == G_I32).all() and (sc[:, 3:] == G_F64).all()
        assert R.same_dump(db.get(), ref.get())
    finally:
        ctx.synchronize()
        db.close()
        voc.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_argument_statuses_with_a_device(ctx):
    import torch
    dev = torch.device("cuda", 0)
    d_h = torch.ones(8, dtype=torch.int32, device=dev)
    db = api.BowDb(ctx, 8, 4, 32)
    try:
        bad = np.ones(8, np.uint32)
        bad[3] = 8192
        for call in (lambda: db.add_dev(0), lambda: db.query_dev(0, 4), lambda: db.query_dev(d_h.data_ptr(), 0),
                     lambda: db.query_dev(d_h.data_ptr(), 257), lambda: db.query(np.ones(8, np.uint32), 0), lambda: db.set_weights(bad),
                     lambda: api.BowDb(ctx, 0, 4, 32), lambda: api.BowDb(ctx, 262145, 4, 32), lambda: api.BowDb(ctx, 8, 0, 32),
                     lambda: api.BowDb(ctx, 8, (1 << 22) + 1, 32), lambda: api.BowDb(ctx, 8, 4, 0), lambda: api.BowDb(ctx, 8, 4, (1 << 28) + 1)):
            with pytest.raises(api.PmError) as e:
                call()
            assert e.value.status == api.PM_E_INVALID
        assert (db.get_weights() == 1).all() and db.counts() == (0, 0)
        if torch.cuda.device_count() >= 2:
            other = pm.Context(1)
            try:
                for call in (lambda: api.BowDb.add_dev(_on(db, other), d_h.data_ptr()), lambda: api.BowDb.counts(_on(db, other))):
                    with pytest.raises(api.PmError) as e:
                        call()
                    assert e.value.status == api.PM_E_INVALID and "another device" in str(e.value)
            finally:
                other.close()
    finally:
        ctx.synchronize()
        db.close()


class _on:
    """The database `db` presented with another context (for the other-device refusal)."""

    def __init__(self, db, ctx):
        self._h, self._ctx, self.K = db._h, ctx, db.K


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_capturing_stream_is_refused():
    """Every call finds the stream capturing and returns PM_E_UNSUPPORTED before it allocates or enqueues anything: the outputs
    keep their guard values, the dump stays as it was, and the object then works as one that never saw a capture."""
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    prev = torch.cuda.current_stream(dev)
    torch.cuda.set_stream(st)
    c = pm.Context(0)
    c.set_stream(st.cuda_stream)
    db, bufs = None, None
    try:
        h = cases.tie_histograms(20, seed=9)
        db = api.BowDb(c, 8, 32, 256)
        ref = R.RefDb(8, 32, 256)
        for x in h[:10]:
            assert db.add(x) == ref.add(x)
        before = db.get()
        d_h = dev_hist(torch, h[10])
        d_id = torch.full((1,), G_I32, dtype=torch.int32, device=dev)
        d_ids = torch.full((4,), G_I32, dtype=torch.int32, device=dev)
        d_sc = torch.full((4,), G_F64, dtype=torch.float64, device=dev)
        d_cnt = torch.full((1,), G_I32, dtype=torch.int32, device=dev)
        d_all = torch.full((10,), G_F64, dtype=torch.float64, device=dev)
        bufs = (d_h, d_id, d_ids, d_sc, d_cnt, d_all)
        torch.cuda.synchronize()
        made = []
        calls = [lambda: db.add_dev(d_h.data_ptr(), d_id.data_ptr()),
                 lambda: db.query_dev(d_h.data_ptr(), 4, 0, 0, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(), d_all.data_ptr()),
                 lambda: db.clear_dev(),
                 lambda: db.idf_dev(),
                 lambda: db.set_weights(np.full(8, 5, np.uint32)),
                 lambda: db.get_weights(),
                 lambda: db.get(),
                 lambda: db.add(h[10]),
                 lambda: db.query(h[10], 4),
                 lambda: made.append(api.BowDb(c, 8, 4, 32))]
        gc.collect()
        for call in calls:
            g = torch.cuda.CUDAGraph()
            with pytest.raises(pm.PmError) as err:
                with torch.cuda.graph(g, stream=st, capture_error_mode="relaxed"):
                    call()
            assert err.value.status == api.PM_E_UNSUPPORTED and "capturing" in str(err.value)
            del g, err
            torch.cuda.set_stream(st)
            torch.cuda.synchronize()
        assert not made
        assert (d_id == G_I32).all() and (d_ids == G_I32).all() and (d_sc == G_F64).all() and (d_cnt == G_I32).all() and (d_all == G_F64).all()
        assert R.same_dump(db.get(), before) and R.same_dump(before, ref.get())
        db.add_dev(d_h.data_ptr(), d_id.data_ptr())
        db.query_dev(d_h.data_ptr(), 4, 0, 0, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr())
        torch.cuda.synchronize()
        assert ref.add(h[10]) == 10 == int(d_id.cpu().numpy()[0])
        rid, rsc, rcount, _ = ref.query(h[10], 4)
        assert (d_ids.cpu().numpy() == rid).all() and (cases.u64(d_sc.cpu().numpy()) == cases.u64(rsc)).all() and int(d_cnt.cpu().numpy()[0]) == rcount
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)
        if db is not None:
            db.close()
        c.close()
        del bufs
