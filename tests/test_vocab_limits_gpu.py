"""GPU: the vocabulary kernels (docs/SPEC.md S102-S106) at their limits, on the inputs of tests/vocab_cases.py, bit for bit
against the plain-C restatement tests/vocab_ref.c: the words after every iteration, the labels, every field of every record,
and the words, distances and histogram of the encoding, with guards behind every output.

  A  every lane layout of vocab_update: u8 rows of 3, 5, 17, 25, 33, 48 and 63 dwords, bit rows of 1, 3, 5, 9 and 15.
  B  squared distances of 2^22 and more that share a float (S103's tie rule, S105's cost from the bytes), alone and among
     ordinary rows; rows of 132, 192 and 256 bytes take the matcher's widened route.
  C  K = 70 000 and 262 144: labels of 2^16 and more, almost every word empty, a device count in the encoding.
  D  n = max_rows = 2^24 rows on one word: a byte sum of 255 * 2^24.

test_vocab_limits_cpu.py asserts, without a device, that the inputs reach these regimes."""
import gc

import numpy as np
import pytest

import vocab_cases as V
import vocab_ref as R
from test_vocab_gpu import G_I32, KIND_NAME, PAD, Dev, assert_run_equals_ref, check_training

# (the cached inputs are read-only arrays; torch.from_numpy remarks on that, and nothing writes through the tensor)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

G_F32, G_HIST = -5.0, 12345
_ids = lambda kb: "%s%d" % (KIND_NAME[kb[0]], kb[1])


def first_diff(got, want):
    """What an assertion on two arrays says when they differ: the first place, and both values there."""
    bad = np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))
    return "equal" if not bad.size else "%d differ, first at %d: %r != %r" % (bad.size, bad[0], np.asarray(got).reshape(-1)[bad[0]],
                                                                           np.asarray(want).reshape(-1)[bad[0]])


def encode_dev(d, count=None):
    """One assign_dev of the rows of `d` with the words its object holds: (words, distances, histogram), guards checked.
    count: the device count (None: no count is given)."""
    t, n, K = d.t, d.n, d.K
    d_w = t.full((n + PAD,), G_I32, dtype=t.int32, device=d.dev)
    d_d = t.full((n + PAD,), G_F32, dtype=t.float32, device=d.dev)
    d_h = t.full((K + PAD,), G_HIST, dtype=t.int32, device=d.dev)
    d_n = None if count is None else t.tensor([count], dtype=t.int32, device=d.dev)
    t.cuda.synchronize()
    d.voc.assign_dev(d.d_rows.data_ptr(), n, 0 if count is None else d_n.data_ptr(), d_w.data_ptr(), d_d.data_ptr(), d_h.data_ptr())
    d.ctx.synchronize()
    w, dist, h = d_w.cpu().numpy(), d_d.cpu().numpy(), d_h.cpu().numpy()
    assert (w[n:] == G_I32).all() and (dist[n:] == G_F32).all() and (h[K:] == G_HIST).all()
    return w[:n], dist[:n], h[:K].view(np.uint32)


def assert_encoding_equals_ref(got, want, m=None, what=""):
    """Labels, distances (bit for bit below the count m, NaN from there on) and histogram against vocab_ref.encode's."""
    w, dist, h = got
    rw, rd, rh = want
    m = w.size if m is None else m
    assert (w == rw).all(), (what, "words", first_diff(w, rw))
    assert (dist[:m].view(np.uint32) == rd[:m].view(np.uint32)).all(), (what, "dist", first_diff(dist[:m].view(np.uint32), rd[:m].view(np.uint32)))
    assert np.isnan(dist[m:]).all() and (w[m:] == -1).all(), what
    assert (h == rh).all() and int(h.sum(dtype=np.int64)) == m, (what, "hist", first_diff(h, rh))


# ---- A: every lane layout --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kb", V.LAYOUTS, ids=_ids)
def test_every_lane_layout(ctx, kb):
    kind, nbytes = kb
    rows, full, enc = V.layout_case(kind, nbytes)
    got, ref = check_training(ctx, kind, rows, V.LAYOUT_K, V.LAYOUT_ITERS, every=True)
    assert (ref[0] == full[0]).all() and (got[0] == full[0]).all()
    d = Dev(ctx, kind, rows, V.LAYOUT_K)
    try:
        d.voc.set(got[0])
        assert_encoding_equals_ref(encode_dev(d), enc, what="%s %d bytes" % (KIND_NAME[kind], nbytes))
    finally:
        d.close()


# ---- B: float-shared distances ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("embedded", [False, True], ids=["alone", "embedded"])
@pytest.mark.parametrize("nbytes", V.TIE_BYTES)
def test_float_shared_distances(ctx, nbytes, embedded):
    """S103 orders on sqrtf((float)D): of two words whose squared distances share a float the lower index wins, and S105's
    cost is then the integer distance to that word, not the minimum.  `embedded`: the same planted rows among 3000 ordinary
    ones keep their labels, whatever route the matcher takes at that size."""
    rows, words, where, full, enc = V.float_tie_case(nbytes, embedded)
    what = "%d bytes%s" % (nbytes, ", embedded" if embedded else "")
    d = Dev(ctx, R.L2_U8, rows, V.TIE_K)
    try:
        d.voc.set(words)
        got = encode_dev(d)
        assert_encoding_equals_ref(got, enc, what=what)
        alone = V.float_tie_case(nbytes)[4]
        assert (got[0][where] == alone[0]).all(), (what, first_diff(got[0][where], alone[0]))
        assert (got[1][where].view(np.uint32) == alone[1].view(np.uint32)).all(), what
        run = d.train(words, V.TIE_ITERS)
        assert_run_equals_ref(run, full, V.TIE_ITERS, what)
    finally:
        d.close()


# ---- C: K at and above 2^16 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", V.BIG_K, ids=lambda c: "%s%d-K%d" % (KIND_NAME[c[0]], c[1], c[2]))
def test_k_at_and_above_two_to_the_16(ctx, case):
    kind, nbytes, K, n = case
    rows, words, full, enc = V.big_k_case(*case)
    d = Dev(ctx, kind, rows, K)
    try:
        run = d.train(words, V.BIG_K_ITERS)
        assert_run_equals_ref(run, full, V.BIG_K_ITERS, "K = %d" % K)
        assert (run[0] == full[3][-1]).all() and run[1].max() >= 1 << 16
        assert_encoding_equals_ref(encode_dev(d, n - V.BIG_K_SHORT), enc, n - V.BIG_K_SHORT, "K = %d" % K)
    finally:
        d.close()
        del d
        gc.collect()


# ---- D: the row limit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [R.L2_U8, R.BITS], ids=["l2", "bits"])
def test_the_row_limit(ctx, kind):
    """2^24 rows, all on word 0: 2^18 waves flush one accumulator and one histogram bin, and the byte-0 sum is 255 * 2^24.
    One object and one upload serve the training run and the encoding."""
    n = V.ROW_LIMIT_N
    words, info, after, hist, period = V.row_limit_ref(kind)
    d = Dev(ctx, kind, V.row_limit_rows(), 2, max_rows=n)
    try:
        d.rows = None                                        # (the device copy is what the calls read)
        got_words, lab, got_info = d.train(V.ROW_LIMIT_WORDS, V.ROW_LIMIT_ITERS)
        assert (got_words == words).all(), (got_words, words)
        assert not lab.any(), first_diff(lab, np.zeros_like(lab))
        for f in R.ITER_DTYPE.names:
            assert (got_info[f] == info[f]).all(), (f, got_info[f], info[f])
        del lab
        w, dist, h = encode_dev(d)
        assert not w.any(), first_diff(w, np.zeros_like(w))
        want = np.resize(period, n)
        assert (dist.view(np.uint32) == want.view(np.uint32)).all(), first_diff(dist.view(np.uint32), want.view(np.uint32))
        assert (h == hist).all() and h.tolist() == [n, 0]
    finally:
        d.close()
        del d
        gc.collect()
        import torch
        torch.cuda.empty_cache()
