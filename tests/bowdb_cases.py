"""The cases of the image-database tests (docs/SPEC.md S107-S112), as lists of operations that any implementation can run:
the plain-C restatement (bowdb_ref.RefDb), the big-integer Python model of test_bowdb_cpu.py, and the device through the
adapter of test_bowdb_gpu.py.  run() executes a list on an adapter and returns one result per operation; same() compares two
such lists bit for bit (doubles as u64).  No device and no library is needed to build the cases.

An adapter has: add_many(hists (n, K) uint32) -> ids int32 (n,);  set_weights(w) -> 0 or -1;  idf();  clear();
query(hist, top, lo, hi) -> (ids int32 (top,), scores float64 (top,), count, every float64 (n_images,));  get() -> the dump
dictionary of BowDb.get()."""
import numpy as np

QNAN = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]
ADD_KS = [1, 63, 64, 65, 1000, 4097, 262144]
SELECT_NS = [1, 63, 64, 65, 1025, 5000]
TOPS = [1, 2, 64, 256]


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def run(db, ops):
    out = []
    for op in ops:
        what = op[0]
        if what == "add":
            out.append(np.asarray(db.add_many(np.ascontiguousarray(op[1], np.uint32).reshape(-1, db.K)), np.int32))
        elif what == "dump":
            out.append(db.get())
        elif what == "set_weights":
            out.append(db.set_weights(np.ascontiguousarray(op[1], np.uint32)))
        elif what == "idf":
            out.append(db.idf())
        elif what == "clear":
            out.append(db.clear())
        elif what == "query":
            ids, scores, count, every = db.query(np.ascontiguousarray(op[1], np.uint32), op[2], op[3], op[4])
            out.append((np.asarray(ids, np.int32), u64(scores), int(count), u64(every)))
        elif what == "query_without_best":                       # the window removes exactly the best image
            ids, _, count, _ = db.query(np.ascontiguousarray(op[1], np.uint32), 1, 0, 0)
            best = int(ids[0]) if count else 0
            ids, scores, count, every = db.query(np.ascontiguousarray(op[1], np.uint32), op[2], best, best + 1)
            out.append((best, np.asarray(ids, np.int32), u64(scores), int(count), u64(every)))
        else:
            raise ValueError(what)
    return out


def same(a, b):
    """Empty string when the two result lists are equal, else where they first differ."""
    if len(a) != len(b):
        return "lengths %d / %d" % (len(a), len(b))
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, dict):
            for k in x:
                if not np.array_equal(np.asarray(x[k]), np.asarray(y[k])):
                    return "op %d: dump field %s" % (i, k)
        elif isinstance(x, tuple):
            for j, (p, q) in enumerate(zip(x, y)):
                if not np.array_equal(np.asarray(p), np.asarray(q)):
                    return "op %d: part %d: %r / %r" % (i, j, p, q)
        elif x is None or y is None:
            if x is not y:
                return "op %d: %r / %r" % (i, x, y)
        elif not np.array_equal(np.asarray(x), np.asarray(y)):
            return "op %d: %r / %r" % (i, x, y)
    return ""


# ---- S108: adding ------------------------------------------------------------------------------------------------------------------
def spread(K, T, seed):
    """T rows over at most 60000 of the K words, every chosen word at least once where T allows."""
    rng = np.random.default_rng(seed)
    h = np.zeros(K, np.uint32)
    words = rng.choice(K, size=min(K, 60000, T), replace=False)
    h[words] = 1
    np.add.at(h, rng.choice(words, size=T - words.size), 1)
    assert int(h.sum()) == T
    return h


def add_histograms(K):
    """The named histograms of the add test, in the order they are added."""
    def one(w, c=3):
        h = np.zeros(K, np.uint32)
        h[w] = c
        return h
    named = [("first_word", one(0)), ("last_word", one(K - 1, 7))]
    if K <= 65535:
        named.append(("every_word", np.arange(K, dtype=np.uint32) % 2 + 1 if 2 * K <= 65535 else np.ones(K, np.uint32)))
    named += [("T_65535", spread(K, 65535, K)), ("T_65536", spread(K, 65536, K + 1)), ("all_zero", np.zeros(K, np.uint32)),
              ("one_more", one(K // 2, 2))]
    return named


def add_case(K):
    """(max_images, max_entries, ops, names): a dump after every add, so that a refusal can be seen to change nothing."""
    named = add_histograms(K)
    ops = []
    for _, h in named:
        ops += [("add", h), ("dump",)]
    entries = sum(int((h != 0).sum()) for _, h in named)
    return 16, entries + 5, ops, [n for n, _ in named]


def limit_cases():
    """K = 65.  Entries: 4 + 6 fill max_entries = 10 exactly, the next image is refused -2, and so is one after it that is
    empty-checked first (-1 beats -2).  Images: max_images = 2 reached, the third refused -2."""
    K = 65
    def h(words):
        a = np.zeros(K, np.uint32)
        a[list(words)] = 2
        return a
    entries = [("add", h(range(4))), ("dump",), ("add", h(range(59, 65))), ("dump",), ("add", h([7])), ("dump",),
               ("add", np.zeros(K, np.uint32)), ("dump",), ("query", h([0, 64]), 4, 0, 0)]
    images = [("add", h([1, 2])), ("add", h([2, 3])), ("dump",), ("add", h([3])), ("dump",), ("query", h([2]), 4, 0, 0)]
    return [("entries_full", K, 8, 10, entries), ("images_full", K, 2, 100, images)]


# ---- S109: weights -----------------------------------------------------------------------------------------------------------------
def weight_case(N):
    """K = 8, N images: word 0 in no image (df 0), word 1 in image 0 alone (df 1), word 2 in every image (df N), the rest at
    random.  idf, then given weights holding 0 and 8191, then 8192 (refused), then clear (the weights stay) and new images."""
    K = 8
    rng = np.random.default_rng(900 + N)
    hists = rng.integers(0, 4, size=(N, K)).astype(np.uint32)
    hists[:, 0] = 0
    hists[:, 1] = 0
    hists[0, 1] = 5
    hists[:, 2] = rng.integers(1, 9, size=N)
    q = np.array([1, 2, 3, 0, 1, 0, 2, 1], np.uint32)
    given = np.array([0, 8191, 1, 8191, 0, 17, 8191, 3], np.uint32)
    bad = given.copy()
    bad[5] = 8192
    ops = [("add", hists), ("dump",), ("query", q, 4, 0, 0), ("idf",), ("dump",), ("query", q, 4, 0, 0),
           ("set_weights", given), ("dump",), ("query", q, 4, 0, 0), ("set_weights", bad), ("dump",),
           ("clear",), ("dump",), ("idf",), ("dump",), ("add", hists[::-1].copy()), ("dump",), ("query", q, 4, 0, 0)]
    return K, N + 2, 8 * (N + 2), ops


# ---- S110: the scene and the score --------------------------------------------------------------------------------------------------
def place_scene(seed=7, K=512, places=24, words_per_place=60, rows=150, own=0.7):
    """(database histograms (2 * places, K): images 2p and 2p + 1 show place p; query histograms (places, K))."""
    rng = np.random.default_rng(seed)
    vocab = [rng.choice(K, size=words_per_place, replace=False) for _ in range(places)]

    def image(p):
        mine = rng.random(rows) < own
        w = np.where(mine, rng.choice(vocab[p], size=rows), rng.integers(0, K, size=rows))
        return np.bincount(w, minlength=K).astype(np.uint32)
    db = np.stack([image(p) for p in range(places) for _ in range(2)])
    qs = np.stack([image(p) for p in range(places)])
    return db, qs


def scene_case(idf):
    """The 48 images, then an image equal to query 0 (its score is exactly 1.0), and every place's query with top = 5."""
    db, qs = place_scene()
    ops = [("add", db), ("add", qs[0])]
    if idf:
        ops += [("idf",)]
    ops += [("dump",)] + [("query", q, 5, 0, 0) for q in qs]
    return 512, 64, int((db != 0).sum()) + 512, ops


def shapes_case():
    """K = 5000: images of 1, 63, 64, 65 and 4097 entries, an image sharing no word with the query, an image all of whose
    words have weight 0, and an image equal to the query; under given weights."""
    K = 5000
    rng = np.random.default_rng(41)
    w = rng.integers(1, 8192, size=K).astype(np.uint32)
    w[4990:] = 0                                                 # the zero-weight words
    def img(n_entries, lo=0, hi=4900):
        h = np.zeros(K, np.uint32)
        h[rng.choice(np.arange(lo, hi), size=n_entries, replace=False)] = rng.integers(1, 6, size=n_entries)
        return h
    q = img(700, 0, 4000)
    imgs = [img(1, 0, 4000), img(63), img(64), img(65), img(4097), img(40, 4000, 4900), img(5, 4990, 5000), q.copy()]
    imgs[0][:] = 0
    imgs[0][np.flatnonzero(q)[3]] = 9                            # the one-entry image shares its word with the query
    ops = [("set_weights", w), ("add", np.stack(imgs)), ("dump",), ("query", q, 8, 0, 0), ("query", imgs[4], 3, 0, 0)]
    return K, 8, int(sum((i != 0).sum() for i in imgs)), ops


def range_case():
    """The top of the range: T = 65535 on one word with weight 8191 on both sides (S = Nq * Nd just under 2^58), and the same
    total over two and three words under odd weights, so that S and Nq * Nd pass 2^32 and 2^53 with low bits set: the three
    counts are all odd; 65535 is odd, so two counts cannot both be, and there one is odd and test_bowdb_cpu.py asserts
    that S and Nq * Nd of that pair are odd."""
    K = 4
    w = np.array([8191, 8189, 8187, 1], np.uint32)
    imgs = np.array([[65535, 0, 0, 0], [40001, 25534, 0, 0], [21845, 21847, 21843, 0], [1, 0, 0, 0], [3, 1, 1, 60001]], np.uint32)
    qs = np.array([[65535, 0, 0, 0], [25535, 40000, 0, 0], [30001, 20003, 15531, 0], [1, 1, 1, 1], [7, 5, 3, 65520]], np.uint32)
    ops = [("set_weights", w), ("add", imgs), ("dump",)] + [("query", q, 5, 0, 0) for q in qs]
    return K, 8, 32, ops


# ---- S111: selection ----------------------------------------------------------------------------------------------------------------
def tie_histograms(N, K=8, seed=0):
    """N images of tiny counts over 8 words: a few dozen distinct histograms, so most scores are shared by many images."""
    rng = np.random.default_rng(3000 + N + seed)
    h = rng.integers(0, 3, size=(N, K)).astype(np.uint32)
    h[h.sum(axis=1) == 0, 0] = 1
    return h


def selection_case(N, max_images=None):
    """max_images above 32768 sends the device through its sliced selection (several workgroups, then one over their keys)."""
    K = 8
    h = tie_histograms(N)
    q = np.array([2, 1, 0, 1, 0, 0, 1, 2], np.uint32)
    narrow = np.array([0, 0, 0, 0, 0, 3, 0, 0], np.uint32)       # many images share no word with it: fewer candidates
    ops = [("add", h)]
    for top in TOPS:
        ops += [("query", q, top, 0, 0), ("query", q, top, 5, 5), ("query", q, top, 0, N), ("query", q, top, -3, N + 9),
                ("query_without_best", q, top), ("query", narrow, top, 0, 0), ("query", q, top, N // 3, N // 3 + max(N // 2, 1))]
    ops += [("query", np.zeros(K, np.uint32), 4, 0, 0), ("query", np.array([65535, 1, 0, 0, 0, 0, 0, 0], np.uint32), 4, 0, 0),
            ("dump",)]
    return K, max_images or N, 8 * N, ops
