"""CPU: the builders of tests/vocab_cases.py reach the regimes they are named for, measured on the plain-C restatement
tests/vocab_ref.c alone.  test_vocab_limits_gpu.py runs the same inputs on the device; a builder that stops reaching its
regime fails here, before any device run."""
import numpy as np
import pytest

import vocab_cases as V
import vocab_ref as R

KIND_NAME = {R.L2_U8: "l2", R.BITS: "bits"}
_ids = lambda kb: "%s%d" % (KIND_NAME[kb[0]], kb[1])


# ---- A: lane layouts -----------------------------------------------------------------------------------------------------------
def test_the_u8_widths_cover_the_layouts_they_are_listed_for():
    """The arithmetic of vocab_update<0> on the widths of case A: W = bytes / 4 dwords, rpi = 64 / W rows side by side,
    S = ceil(64 / rpi) sorted rows per lane group, walked four at a time."""
    geo = {b: (b // 4,) + V.u8_lane_groups(b) for b in V.LAYOUT_U8}
    assert geo[12] == (3, 21, 4) and geo[20] == (5, 12, 6)
    for b in (12, 20):                                       # W does not divide 64: the last lane groups run past position 63
        W, rpi, S = geo[b]
        assert 64 % W and rpi * S > 64 and rpi * W < 64
    assert geo[20][2] % 4 == 2                               # S = 6: the last step of four has two dead slots
    assert (geo[68][1], geo[100][1]) == (3, 2) and 3 * 17 < 64 and 2 * 25 < 64          # rpi = 3 and 2 with idle lanes
    assert all(geo[b][1] == 1 and geo[b][0] < 64 for b in (132, 192, 252))              # rpi = 1 with idle lanes
    assert all((b // 4) % 2 == 1 for b in V.LAYOUT_BITS)     # bit rows: an odd dword count, the upper half-wave skips a counter


@pytest.mark.parametrize("kb", V.LAYOUTS, ids=_ids)
def test_layout_rows_fill_the_words_and_split_runs_between_lane_groups(kb):
    """Iteration 0 gives rows to at least 30 of the 37 words, and in at least one wave a run of equal labels spans sorted
    positions of different lane groups (u8 rows, rpi >= 2: the run is flushed by two groups, p / S differs).  Where the
    kernel has a single group per wave there is no such pair, and the condition is the one its walk has instead: a run
    that continues across a step of the walk (four sorted rows per step with rpi = 1, two with bit rows) in a wave that
    holds more than one run, so that sums are carried between steps and flushed in the middle of one."""
    kind, nbytes = kb
    rows, full, enc = V.layout_case(kind, nbytes)
    assert full[2]["n_empty"][0] <= V.LAYOUT_K - 30
    assert full[2]["n_changed"][0] == V.LAYOUT_N and V.LAYOUT_N % 64                     # (and a partial last wave)
    lab0 = R.assign(kind, R.init_stride(rows, V.LAYOUT_K), rows)[0]
    rpi, S = V.u8_lane_groups(nbytes) if kind == R.L2_U8 else (1, 64)
    step = S if rpi >= 2 else (4 if kind == R.L2_U8 else 2)
    hits = 0
    for wave in range((V.LAYOUT_N + 63) // 64):
        runs = V.sorted_runs(lab0, wave)
        hits += len(runs) > 1 and any(a // step != b // step for _, a, b in runs)
    assert hits >= 1
    assert (np.bincount(enc[0], minlength=V.LAYOUT_K) == enc[2]).all()


# ---- B: float-shared distances -------------------------------------------------------------------------------------------------
def test_the_tie_words_are_what_the_construction_says():
    for nbytes in V.TIE_BYTES:
        w = V.tie_words(nbytes).astype(np.int64)
        assert (w[:, 4:] == 255).all()
        assert ((w[:, :4] ** 2).sum(1) == V.TIE_H + (63 - np.arange(V.TIE_K)) % 8).all()


@pytest.mark.parametrize("nbytes", V.TIE_BYTES)
def test_float_order_departs_from_the_integer_order(nbytes):
    """Measured: planted rows whose S103 label is not the integer argmin, of 1000: 68 bytes 0, 128 bytes 252, 132 bytes
    261, 192 bytes 375, 256 bytes 466 (asserted: exactly 0, and at least 20 %)."""
    rows, words, where, full, enc = V.float_tie_case(nbytes)
    d = V.np_idist(rows, words)
    assert (d.argmin(1) == 7).all()                          # the integer minimum is at word 7 for every row
    lab0 = R.assign(R.L2_U8, words, rows)
    assert (lab0[0] == enc[0]).all()
    off = int((enc[0] != 7).sum())
    cost_min = int(d.min(1).sum())
    print("bytes %d: %d of %d rows off the integer argmin, cost %d against %d" % (nbytes, off, V.TIE_N, full[2]["cost"][0], cost_min))
    if nbytes == 68:
        assert d.max() < 1 << 22 and off == 0                # the control: the float order is the integer order
        assert int(full[2]["cost"][0]) == cost_min
    else:
        assert d.min() >= 1 << 22
        assert off >= V.TIE_N // 5
        assert (enc[0] <= 7).all() and (enc[0][enc[0] != 7] < 7).all()                   # a float tie goes to the lower index
        assert int(full[2]["cost"][0]) > cost_min            # S105: the cost is the distance to the chosen word
        assert int(full[2]["cost"][0]) == int(d[np.arange(V.TIE_N), enc[0]].sum())


@pytest.mark.parametrize("nbytes", V.TIE_BYTES)
def test_embedded_tie_rows_keep_their_labels(nbytes):
    alone = V.float_tie_case(nbytes)
    rows, words, where, full, enc = V.float_tie_case(nbytes, embedded=True)
    assert rows.shape[0] == V.TIE_HOSTS + V.TIE_N and where.size == V.TIE_N and (np.diff(where) > 0).all()
    assert (rows[where] == alone[0]).all()
    assert (enc[0][where] == alone[4][0]).all() and (enc[1][where].view(np.uint32) == alone[4][1].view(np.uint32)).all()


# ---- C: K at and above 2^16 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", V.BIG_K, ids=lambda c: "%s%d-K%d" % (KIND_NAME[c[0]], c[1], c[2]))
def test_big_k_reaches_high_labels_and_leaves_words_empty(case):
    kind, nbytes, K, n = case
    rows, words, full, enc = V.big_k_case(*case)
    top = 1 << 17 if K == 262144 else 1 << 16
    assert full[1].max() >= top and enc[0].max() >= top
    assert (full[2]["n_empty"] >= K - n).all()
    high = np.bincount(full[1][full[1] >= 1 << 16])
    assert high.max() >= 2                                   # a run of more than one row on such a label
    assert (enc[0][n - V.BIG_K_SHORT:] == -1).all() and int(enc[2].sum()) == n - V.BIG_K_SHORT


# ---- D: the row limit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [R.L2_U8, R.BITS], ids=["l2", "bits"])
def test_row_limit_sums_pass_two_to_the_31(kind):
    n = V.ROW_LIMIT_N
    rows = V.row_limit_rows()
    assert rows.shape == (n, 4) and int(rows[:, 0].sum(dtype=np.uint64)) == 255 * n == 4278190080 >= 1 << 31
    assert int((rows[:, 1] == 254).sum()) == (n + 2) // 3 and int((rows[:, 2] == 0).sum()) == (n - 5 + 6) // 7
    del rows
    words, info, after, hist, period = V.row_limit_ref(kind)
    assert info["n_changed"].tolist() == [n, 0] and info["n_empty"].tolist() == [1, 1]
    assert hist.tolist() == [n, 0] and (words[1] == 0).all()
    if kind == R.L2_U8:
        assert words[0].tolist() == [255, 255, 219, 255] and info["n_moved"].tolist() == [1, 0]
        assert info["cost"].tolist() == [155853936031, 133592969767]
    else:
        # a bit of byte 1 is clear in a third of the rows and all of byte 2 in a seventh: every majority stays 1
        assert words[0].tolist() == [255] * 4 and info["n_moved"].tolist() == [0, 0]
        assert info["cost"].tolist() == [(n + 2) // 3 + 8 * ((n + 1) // 7)] * 2
