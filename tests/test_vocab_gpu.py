"""GPU: visual vocabularies (docs/SPEC.md S102-S106).  Every comparison is bit for bit with the plain-C restatement
tests/vocab_ref.c: the words after every iteration count tested, the labels, every field of every record, and the words,
distances and histogram of the encoding.  Row widths cover every layout of the update kernel (16 rows per wave-instruction,
a lane count per row that does not divide 64, two rows per instruction, a whole wave per row; 1, 4 and 8 bit counters per
lane) and every matcher route behind it; shapes cover one run longer than a wave or workgroup holds, runs of length 1, a
skewed set, a partial wave and a single row.  test_vocab_limits_gpu.py goes on from here: the remaining lane layouts, float-shared
distances, K of 2^16 and more, and 2^24 rows."""
import gc
import os

import numpy as np
import pytest

import points_matching_amd as pm
import vocab_ref as R
from points_matching_amd import api
from vocab_cases import make_rows                   # (moved there unchanged: test_vocab_limits_cpu.py needs it without a device)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G_I32, G_U8 = -77, 0xAB
PAD = 16                       # guard elements behind every output
KIND_NAME = {R.L2_U8: "l2", R.BITS: "bits"}
WIDTHS = [(R.L2_U8, 4), (R.L2_U8, 36), (R.L2_U8, 128), (R.L2_U8, 256), (R.BITS, 8), (R.BITS, 32), (R.BITS, 64)]
BOTH = [(R.L2_U8, 128), (R.BITS, 32)]
_ids = lambda kb: "%s%d" % (KIND_NAME[kb[0]], kb[1])


class Dev:
    """The device side of one training run: rows, guarded outputs, and what came back."""

    def __init__(self, ctx, kind, rows, K, max_rows=None):
        import torch
        self.t, self.dev = torch, torch.device("cuda", 0)
        self.ctx, self.kind, self.rows, self.K = ctx, kind, np.ascontiguousarray(rows, np.uint8), K
        self.n, self.nbytes = self.rows.shape
        self.voc = api.Vocab(ctx, kind, self.nbytes, K, max_rows or self.n)
        self.d_rows = torch.from_numpy(self.rows).to(self.dev)

    def close(self):
        self.ctx.synchronize()
        self.voc.close()

    def train(self, w0, iters, labels=True, info=True):
        """(words, labels, records) after `iters` iterations from w0 (None: stride initialisation on the device); guards checked."""
        t = self.t
        d_lab = t.full((self.n + PAD,), G_I32, dtype=t.int32, device=self.dev)
        d_info = t.full(((iters + 1) * 24 + PAD,), G_U8, dtype=t.uint8, device=self.dev)
        t.cuda.synchronize()
        if w0 is None:
            self.voc.init_stride_dev(self.d_rows.data_ptr(), self.n)
        else:
            self.voc.set(w0)
        self.voc.train_dev(self.d_rows.data_ptr(), self.n, iters, d_lab.data_ptr() if labels else 0, d_info.data_ptr() if info else 0)
        words = self.voc.get()
        lab, raw = d_lab.cpu().numpy(), d_info.cpu().numpy()
        used = self.n if labels and iters > 0 else 0
        assert (lab[used:] == G_I32).all()
        used = iters * 24 if info else 0
        assert (raw[used:] == G_U8).all()
        return words, lab[:self.n].copy(), raw[:iters * 24].copy().view(api.VOCAB_ITER_DTYPE)


def assert_run_equals_ref(got, want, iters, what=""):
    words, lab, info = got
    rw, rl, ri, after = want
    assert (words == after[iters - 1]).all(), what
    assert (lab == rl).all(), what
    for f in R.ITER_DTYPE.names:
        assert (info[f] == ri[f]).all(), (what, f, info[f], ri[f])


def check_training(ctx, kind, rows, K, iters, w0=None, every=False, max_rows=None):
    """Trains on the device and in the restatement and compares everything; `every`: also each shorter run from the same
    start (the words after every iteration).  Returns the device result of the full run and the restatement's."""
    d = Dev(ctx, kind, rows, K, max_rows)
    try:
        start = R.init_stride(rows, K) if w0 is None else np.ascontiguousarray(w0, np.uint8)
        full = R.train(kind, start, rows, iters)
        for it in (range(1, iters + 1) if every else (iters,)):
            got = d.train(w0, it)
            # a run of `it` iterations is a prefix of the full one; its labels are S103 on the words before its last update
            before = start if it == 1 else full[3][it - 2]
            lab = full[1] if it == iters else R.assign(kind, before, rows)[0]
            assert_run_equals_ref(got, (full[3][it - 1], lab, full[2][:it], full[3]), it, "iters=%d" % it)
        return got, full
    finally:
        d.close()


# ---- row widths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kb", WIDTHS, ids=_ids)
def test_every_row_width(ctx, kb):
    kind, nbytes = kb
    rows = make_rows(kind, 3000, nbytes, seed=100 + nbytes)
    got, ref = check_training(ctx, kind, rows, 64, 5, every=True)
    assert ref[2]["n_changed"][0] == 3000 and ref[2]["cost"][0] > ref[2]["cost"][-1]


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kb", BOTH, ids=_ids)
def test_one_word_takes_every_row(ctx, kb):
    """K = 1, n = 5000: one run longer than anything a wave or a workgroup holds, every count on one word."""
    kind, nbytes = kb
    rows = make_rows(kind, 5000, nbytes, seed=7)
    got, ref = check_training(ctx, kind, rows, 1, 3)
    assert got[2]["n_empty"].tolist() == [0, 0, 0] and got[2]["n_changed"].tolist() == [5000, 0, 0] and (got[1] == 0).all()


@pytest.mark.parametrize("kb", BOTH, ids=_ids)
def test_a_word_per_row(ctx, kb):
    """K = n = 500: every run has length 1; the words are the rows and never move."""
    kind, nbytes = kb
    rows = make_rows(kind, 500, nbytes, seed=8, protos=500)
    assert len({r.tobytes() for r in rows}) == 500
    got, ref = check_training(ctx, kind, rows, 500, 3)
    assert (got[0] == rows).all() and (got[1] == np.arange(500)).all()
    assert (got[2]["n_moved"][1:] == 0).all() and (got[2]["cost"] == 0).all() and (got[2]["n_empty"] == 0).all()


@pytest.mark.parametrize("kb", BOTH, ids=_ids)
def test_skewed_set(ctx, kb):
    """90 % identical rows plus a scatter: nearly every wave is one long run with a few strangers."""
    kind, nbytes = kb
    rows = make_rows(kind, 3000, nbytes, seed=9)
    rng = np.random.default_rng(90)
    same = rng.random(3000) < 0.9
    rows[same] = rows[0]
    check_training(ctx, kind, rows, 64, 5)


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("kb", BOTH, ids=_ids)
def test_single_row_and_one_row_past_a_wave(ctx, kb, n):
    kind, nbytes = kb
    rows = make_rows(kind, n, nbytes, seed=10 + n)
    check_training(ctx, kind, rows, min(n, 4), 3, every=True)
    check_training(ctx, kind, rows, 8, 2)                                # more words than rows: the stride rule repeats rows


@pytest.mark.parametrize("kb", BOTH, ids=_ids)
def test_max_rows_larger_than_n_and_guards(ctx, kb):
    """An object made for 5000 rows trained on 777: the guards behind d_labels and d_info (checked in Dev.train) and, in the
    encoding below, behind d_words, d_dist and d_hist stay as they were."""
    import torch
    kind, nbytes = kb
    dev = torch.device("cuda", 0)
    rows = make_rows(kind, 777, nbytes, seed=12)
    d = Dev(ctx, kind, rows, 33, max_rows=5000)
    try:
        got = d.train(None, 4)
        want = R.train(kind, R.init_stride(rows, 33), rows, 4)
        assert_run_equals_ref(got, want, 4)
        d_w = torch.full((777 + PAD,), G_I32, dtype=torch.int32, device=dev)
        d_d = torch.full((777 + PAD,), -5.0, dtype=torch.float32, device=dev)
        d_h = torch.full((33 + PAD,), 12345, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        d.voc.assign_dev(d.d_rows.data_ptr(), 777, 0, d_w.data_ptr(), d_d.data_ptr(), d_h.data_ptr())
        ctx.synchronize()
        w, dist, h = R.encode(kind, want[0], rows)
        assert (d_w.cpu().numpy()[:777] == w).all() and (d_w.cpu().numpy()[777:] == G_I32).all()
        assert (d_d.cpu().numpy()[:777].view(np.uint32) == dist.view(np.uint32)).all() and (d_d.cpu().numpy()[777:] == -5.0).all()
        assert (d_h.cpu().numpy()[:33].view(np.uint32) == h).all() and (d_h.cpu().numpy()[33:] == 12345).all()
    finally:
        d.close()


# ---- rules -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kb", BOTH, ids=_ids)
def test_duplicate_initial_words(ctx, kb):
    kind, nbytes = kb
    rows = make_rows(kind, 1000, nbytes, seed=13)
    w0 = np.stack([rows[0], rows[5], rows[0], rows[9], rows[5]])
    got, ref = check_training(ctx, kind, rows, 5, 3, w0=w0, every=True)
    assert got[2]["n_empty"][0] >= 2
    d = Dev(ctx, kind, rows, 5)
    try:
        words1 = d.train(w0, 1)[0]
        assert (words1[2] == w0[2]).all() and (words1[4] == w0[4]).all()     # the higher duplicates got no row and kept their bytes
    finally:
        d.close()


@pytest.mark.parametrize("kb", BOTH, ids=_ids)
def test_iters_zero_writes_nothing(ctx, kb):
    kind, nbytes = kb
    rows = make_rows(kind, 300, nbytes, seed=14)
    d = Dev(ctx, kind, rows, 6)
    try:
        w0 = R.init_stride(rows, 6)
        words, lab, info = d.train(w0, 0)                                # the guards cover every element of both outputs
        assert (words == w0).all() and info.size == 0
        assert d.voc.train(rows, 0)[1].size == 0 and (d.voc.get() == w0).all()
    finally:
        d.close()


@pytest.mark.parametrize("kb", BOTH, ids=_ids)
def test_converged_runs_stay_put_and_training_twice_is_identical(ctx, kb):
    """After a record with n_changed == 0 nothing moves any more; and a second training on the same object from the same
    start gives identical outputs: the atomic sums do not depend on arrival order and every accumulator was returned to zero."""
    kind, nbytes = kb
    rows = make_rows(kind, 3000, nbytes, seed=15, protos=6, sigma=4.0, flip=0.03)
    d = Dev(ctx, kind, rows, 6)
    try:
        w0 = R.init_stride(rows, 6)
        iters = 12
        a = d.train(w0, iters)
        want = R.train(kind, w0, rows, iters)
        assert_run_equals_ref(a, want, iters)
        still = np.flatnonzero(a[2]["n_changed"] == 0)
        assert still.size, a[2]["n_changed"]
        first = int(still[0])
        assert (a[2]["n_moved"][first:] == 0).all() and (a[2]["n_changed"][first:] == 0).all()
        assert (want[3][first:] == want[3][first]).all()
        b = d.train(w0, iters)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2].tobytes() == b[2].tobytes()
        c = d.train(w0, first + 1)
        assert (c[0] == a[0]).all()                                      # the words of the converged record are the final ones
    finally:
        d.close()


# ---- the label is the matcher's record -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kb", WIDTHS, ids=_ids)
def test_words_and_distances_are_the_matchers_records(ctx, kb):
    import torch
    kind, nbytes = kb
    dev = torch.device("cuda", 0)
    n, K = 1000, 50
    rows = make_rows(kind, n, nbytes, seed=16)
    words = make_rows(kind, K, nbytes, seed=17)
    words[7] = words[3]                                                  # a tie: the lower index wins
    rows[11] = words[3]
    voc = api.Vocab(ctx, kind, nbytes, K, n)
    try:
        d_rows, d_voc = torch.from_numpy(rows).to(dev), torch.from_numpy(words).to(dev)
        d_w = torch.zeros(n, dtype=torch.int32, device=dev)
        d_d = torch.zeros(n, dtype=torch.float32, device=dev)
        d_h = torch.zeros(K, dtype=torch.int32, device=dev)
        d_m = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        voc.set_dev(d_voc.data_ptr())
        voc.assign_dev(d_rows.data_ptr(), n, 0, d_w.data_ptr(), d_d.data_ptr(), d_h.data_ptr())
        if kind == R.L2_U8:
            ctx.bf_knn_l2_u8_dev(d_rows.data_ptr(), n, d_voc.data_ptr(), K, nbytes, 1, d_m.data_ptr())
        else:
            ctx.bf_knn_hamming_dev(d_rows.data_ptr(), n, d_voc.data_ptr(), K, nbytes, 1, d_m.data_ptr())
        ctx.synchronize()
        m = d_m.cpu().numpy().view(api.MATCH_DTYPE)
        w, dist, h = d_w.cpu().numpy(), d_d.cpu().numpy(), d_h.cpu().numpy().view(np.uint32)
        assert (w == m["trainIdx"]).all() and (dist.view(np.uint32) == m["distance"].view(np.uint32)).all()
        rw, rd, rh = R.encode(kind, words, rows)
        assert (w == rw).all() and (dist.view(np.uint32) == rd.view(np.uint32)).all() and (h == rh).all()
        assert w[11] == 3 and dist[11] == 0 and not (w == 7).any()
        assert (voc.get() == words).all()
    finally:
        ctx.synchronize()
        voc.close()


# ---- the device count ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kb", BOTH, ids=_ids)
def test_device_count(ctx, kb):
    import torch
    kind, nbytes = kb
    dev = torch.device("cuda", 0)
    n, K = 333, 20
    rows = make_rows(kind, n, nbytes, seed=18)
    words = R.init_stride(rows, K)
    voc = api.Vocab(ctx, kind, nbytes, K, n)
    try:
        voc.set(words)
        d_rows = torch.from_numpy(rows).to(dev)
        for count in (None, n, n - 1, 0, -1, n + 7):
            m = n if count is None else min(max(count, 0), n)
            d_n = torch.tensor([0 if count is None else count], dtype=torch.int32, device=dev)
            d_w = torch.full((n,), G_I32, dtype=torch.int32, device=dev)
            d_d = torch.full((n,), -5.0, dtype=torch.float32, device=dev)
            d_h = torch.full((K,), 999, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            voc.assign_dev(d_rows.data_ptr(), n, 0 if count is None else d_n.data_ptr(), d_w.data_ptr(), d_d.data_ptr(), d_h.data_ptr())
            ctx.synchronize()
            w, dist, h = d_w.cpu().numpy(), d_d.cpu().numpy(), d_h.cpu().numpy().view(np.uint32)
            rw, rd, rh = R.encode(kind, words, rows, count)
            assert (w == rw).all() and (h == rh).all() and int(h.sum()) == m, count
            assert (dist[:m].view(np.uint32) == rd[:m].view(np.uint32)).all() and np.isnan(dist[m:]).all() and (w[m:] == -1).all(), count
        voc.assign_dev(d_rows.data_ptr(), n)                             # every output is optional
        voc.assign_dev(d_rows.data_ptr(), n, 0, 0, 0, d_h.data_ptr())
        ctx.synchronize()
        assert (d_h.cpu().numpy().view(np.uint32) == R.encode(kind, words, rows)[2]).all()
    finally:
        ctx.synchronize()
        voc.close()


# ---- the host forms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kb", BOTH, ids=_ids)
def test_host_forms_equal_the_device_forms(ctx, kb):
    kind, nbytes = kb
    rows = make_rows(kind, 1200, nbytes, seed=19)
    w0 = R.init_stride(rows, 24)
    d = Dev(ctx, kind, rows, 24)
    try:
        dw, dl, di = d.train(w0, 4)
        d.voc.set(w0)
        hl, hi = d.voc.train(rows, 4)
        hw = d.voc.get()
        assert (hw == dw).all() and (hl == dl).all() and hi.tobytes() == di.tobytes()
        w, dist, h = d.voc.assign(rows[:700])
        rw, rd, rh = R.encode(kind, hw, rows[:700])
        assert (w == rw).all() and (dist.view(np.uint32) == rd.view(np.uint32)).all() and (h == rh).all()
    finally:
        d.close()


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


@pytest.mark.parametrize("kind", [R.L2_U8, R.BITS], ids=["l2", "bits"])
def test_chain_detect_train_encode_on_the_fixtures(ctx, kind):
    """Image 1 is described and its rows train a vocabulary of 32 words (the one readback is the row count the training call
    takes as a host argument).  Image 2 is then described and encoded with n = max_kp and the device count of its describe
    call, on one stream with no readback in between.  Everything is compared on the downloaded rows afterwards."""
    import torch
    dev = torch.device("cuda", 0)
    max_kp, K, nbytes = 512, 32, 128 if kind == R.L2_U8 else 32
    imgs = [read_pgm(os.path.join(GOLD, "img0%d_half.pgm" % i)) for i in (1, 2)]
    voc = api.Vocab(ctx, kind, nbytes, K, max_kp)
    try:
        def describe(img):
            d_img = torch.from_numpy(img).to(dev)
            d_kp = torch.zeros((max_kp, 2), dtype=torch.float32, device=dev)
            d_rows = torch.full((max_kp, nbytes), 0x5A, dtype=torch.uint8, device=dev)
            d_n = torch.full((1,), -3, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            h, w = img.shape
            if kind == R.L2_U8:
                ctx.detect_describe_dev(d_img.data_ptr(), w, h, w, max_kp, d_kp.data_ptr(), d_rows.data_ptr(), 0, 0, d_n.data_ptr())
            else:
                ctx.detect_describe_bits_dev(d_img.data_ptr(), w, h, w, max_kp, d_kp.data_ptr(), d_rows.data_ptr(), 0, d_n.data_ptr())
            return d_img, d_kp, d_rows, d_n

        keep1 = describe(imgs[0])
        ctx.synchronize()
        n1 = int(keep1[3].cpu().numpy()[0])
        assert 2 * K < n1 <= max_kp
        d_info = torch.zeros(5 * 24, dtype=torch.uint8, device=dev)
        d_w = torch.full((max_kp,), G_I32, dtype=torch.int32, device=dev)
        d_h = torch.full((K,), 999, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        voc.init_stride_dev(keep1[2].data_ptr(), n1)
        voc.train_dev(keep1[2].data_ptr(), n1, 5, 0, d_info.data_ptr())
        keep2 = describe(imgs[1])                                        # no readback from here ...
        voc.assign_dev(keep2[2].data_ptr(), max_kp, keep2[3].data_ptr(), d_w.data_ptr(), 0, d_h.data_ptr())
        ctx.synchronize()                                                # ... to here
        rows1, rows2 = keep1[2].cpu().numpy()[:n1], keep2[2].cpu().numpy()
        n2 = int(keep2[3].cpu().numpy()[0])
        assert 2 * K < n2 <= max_kp
        want = R.train(kind, R.init_stride(rows1, K), rows1, 5)
        assert (voc.get() == want[0]).all()
        assert d_info.cpu().numpy().view(api.VOCAB_ITER_DTYPE).tobytes() == want[2].tobytes()
        rw, _, rh = R.encode(kind, want[0], rows2, n2)
        h = d_h.cpu().numpy().view(np.uint32)
        assert (h == rh).all() and int(h.sum()) == n2
        assert (d_w.cpu().numpy() == rw).all()
    finally:
        ctx.synchronize()
        voc.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_argument_statuses_with_a_device(ctx):
    import torch
    dev = torch.device("cuda", 0)
    d_rows = torch.zeros((64, 32), dtype=torch.uint8, device=dev)
    voc = api.Vocab(ctx, R.BITS, 32, 4, 64)
    try:
        for call in (lambda: voc.train_dev(d_rows.data_ptr(), 65, 1), lambda: voc.train_dev(d_rows.data_ptr(), 0, 1),
                     lambda: voc.train_dev(0, 10, 1), lambda: voc.train_dev(d_rows.data_ptr(), 10, 1001),
                     lambda: voc.train_dev(d_rows.data_ptr() + 2, 10, 1), lambda: voc.assign_dev(d_rows.data_ptr(), 65),
                     lambda: voc.assign_dev(d_rows.data_ptr(), 0), lambda: voc.init_stride_dev(d_rows.data_ptr(), 65),
                     lambda: voc.init_stride_dev(0, 10), lambda: voc.set_dev(0)):
            with pytest.raises(api.PmError) as e:
                call()
            assert e.value.status == api.PM_E_INVALID
        with pytest.raises(api.PmError) as e:
            api.Vocab(ctx, R.L2_U8, 128, 8, (1 << 24) + 1)
        assert e.value.status == api.PM_E_UNSUPPORTED
    finally:
        ctx.synchronize()
        voc.close()


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_capturing_stream_is_refused():
    """Every call finds the stream capturing and returns PM_E_UNSUPPORTED before it allocates or enqueues anything: the outputs
    keep their guard values, the words stay as they were, and the object then trains as one that never saw a capture."""
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    prev = torch.cuda.current_stream(dev)
    torch.cuda.set_stream(st)
    c = pm.Context(0)
    c.set_stream(st.cuda_stream)
    voc, bufs = None, None
    try:
        rows = make_rows(R.L2_U8, 500, 128, seed=20)
        w0 = R.init_stride(rows, 8)
        voc = api.Vocab(c, R.L2_U8, 128, 8, 500)
        voc.set(w0)
        d_rows = torch.from_numpy(rows).to(dev)
        d_lab = torch.full((500,), G_I32, dtype=torch.int32, device=dev)
        d_info = torch.full((3 * 24,), G_U8, dtype=torch.uint8, device=dev)
        d_d = torch.full((500,), -5.0, dtype=torch.float32, device=dev)
        d_h = torch.full((8,), 999, dtype=torch.int32, device=dev)
        bufs = (d_rows, d_lab, d_info, d_d, d_h)
        torch.cuda.synchronize()
        made = []
        calls = [lambda: voc.train_dev(d_rows.data_ptr(), 500, 3, d_lab.data_ptr(), d_info.data_ptr()),
                 lambda: voc.assign_dev(d_rows.data_ptr(), 500, 0, d_lab.data_ptr(), d_d.data_ptr(), d_h.data_ptr()),
                 lambda: voc.init_stride_dev(d_rows.data_ptr(), 500),
                 lambda: voc.set_dev(d_rows.data_ptr()),
                 lambda: voc.set(rows[:8]),
                 lambda: voc.get(),
                 lambda: voc.train(rows, 2),
                 lambda: voc.assign(rows),
                 lambda: made.append(api.Vocab(c, R.BITS, 32, 4, 100))]
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
        assert (d_lab == G_I32).all() and (d_info == G_U8).all() and (d_d == -5.0).all() and (d_h == 999).all()
        assert (voc.get() == w0).all()
        voc.train_dev(d_rows.data_ptr(), 500, 3, d_lab.data_ptr(), d_info.data_ptr())
        torch.cuda.synchronize()
        want = R.train(R.L2_U8, w0, rows, 3)
        assert (voc.get() == want[0]).all() and (d_lab.cpu().numpy() == want[1]).all()
        assert d_info.cpu().numpy().view(api.VOCAB_ITER_DTYPE).tobytes() == want[2].tobytes()
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)
        if voc is not None:
            voc.close()
        c.close()
        del bufs
