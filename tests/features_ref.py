"""What the feature front end's tests share (SPEC S53-S60): the inputs, the numpy restatements of the host file's Gaussian
levels and extrema scan, the descriptor caps, and the host extractor as a program of its own that takes every argument.

tests/features_host_main.cpp is compiled once per process from that file and host/pm_features.cpp alone (no libpm_hip.so)
into a temporary directory; host_features() runs it once per argument tuple.  pm_cli fixes contrast and edge_r, the driver
does not; tests/test_features_limits_cpu.py pins the driver to pm_cli at the defaults."""
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
HOST_DIR = os.path.join(ROOT, "points_matching_amd", "host")


# ---- inputs ------------------------------------------------------------------------------------------------------------

def blobs(w, h, seed, n):
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    im = np.full((h, w), 0.5)
    for _ in range(n):
        cx, cy, s = r.uniform(0, w), r.uniform(0, h), r.uniform(1.2, 3.5)
        a = r.choice([-1, 1]) * r.uniform(0.2, 0.45)
        im += a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
    return np.clip(np.rint(255 * im), 0, 255).astype(np.uint8)


def blobs_windowed(w, h, seed, n):
    """blobs() for the large inputs, where its n full-frame exponentials take tens of seconds: the same draws in the same
    order, each blob added only within 9.2 sigma of its centre.  Beyond that a term is below 0.45 exp(-42) < 2^-61, so the sum
    of the 6066 terms left out of a pixel is below 2^-48 of a grey level: the rounded bytes are blobs()'s unless 255 * im
    lies that close to a half.  tests/test_features_limits_cpu.py pins the bytes of both large inputs by the SHA-256 of
    what blobs() itself gives."""
    r = np.random.default_rng(seed)
    im = np.full((h, w), 0.5)
    for _ in range(n):
        cx, cy, s = r.uniform(0, w), r.uniform(0, h), r.uniform(1.2, 3.5)
        a = r.choice([-1, 1]) * r.uniform(0.2, 0.45)
        rad = int(math.ceil(9.2 * s)) + 1
        x0, x1 = max(0, int(cx) - rad), min(w, int(cx) + rad + 2)
        y0, y1 = max(0, int(cy) - rad), min(h, int(cy) + rad + 2)
        if x0 >= x1 or y0 >= y1:
            continue
        y, x = np.mgrid[y0:y1, x0:x1].astype(np.float64)
        im[y0:y1, x0:x1] += a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
    return np.clip(np.rint(255 * im), 0, 255).astype(np.uint8)


def five_octaves():
    """512x512, five octaves (512 ... 32 pixels a side), one Gaussian blob sized for each: every octave has exactly one
    candidate.  The strongest is octave 4's, which its 32x32 plane cannot keep (border rule); the next is octave 3's, kept."""
    y, x = np.mgrid[0:512, 0:512].astype(np.float64)
    im = np.full((512, 512), 0.5)
    for cx, cy, s, a in ((176.0, 176.0, 40.0, 0.4), (272.0, 272.0, 18.0, -0.35), (400.0, 120.0, 9.0, 0.3), (120.0, 400.0, 4.5, -0.3),
                         (330.0, 420.0, 2.2, 0.3)):
        im += a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
    return np.clip(np.rint(255 * im), 0, 255).astype(np.uint8)


def read_pgm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"P5"
        line = f.readline()
        while line.startswith(b"#"):
            line = f.readline()
        w, h = (int(v) for v in line.split())
        assert int(f.readline()) == 255
        return np.frombuffer(f.read(w * h), np.uint8).reshape(h, w).copy()


_IMG = {}


def image(name):
    """golden1 / golden2: the two 496x330 fixtures; tiled: 3 x 3 copies of one 64x64 blob image; five: five_octaves(); WxH: blobs(W, H, 11, W*H//60)
    (the two LARGE inputs through blobs_windowed, which gives the same bytes).
    Made once per process; the callers leave the array as it is."""
    if name not in _IMG:
        if name == "golden1":
            _IMG[name] = read_pgm(os.path.join(GOLD, "img01_half.pgm"))
        elif name == "golden2":
            _IMG[name] = read_pgm(os.path.join(GOLD, "img02_half.pgm"))
        elif name == "tiled":
            _IMG[name] = np.tile(blobs(64, 64, 5, 40), (3, 3))
        elif name == "five":
            _IMG[name] = five_octaves()
        else:
            w, h = (int(v) for v in name.split("x"))
            _IMG[name] = (blobs_windowed if name in LARGE else blobs)(w, h, 11, w * h // 60)
    return _IMG[name]


# The inputs of the limits tests (tests/test_features_limits_cpu.py pins what the host extractor makes of them,
# tests/test_features_limits_gpu.py runs the device on them).
DEFAULT_MAX_KP = 4000                                   # pm_feat::detect_and_describe's own default
LARGE = ("700x520", "640x480")                          # five / four octaves; more than 2048 / more than 1024 rows at max_kp 4000
LARGE_SHA256 = {"700x520": "404e9d724ce5c7bb3ff068edc162e92fa0aa826da340f3ffce40e5acb64cba09",       # of blobs(w, h, 11, w*h//60)
                "640x480": "715f919faa136d1a9153f016474f987e96e1b949f9315272772ea9785e0d58f0"}
LARGE_CASES = (("700x520", 4000), ("700x520", 1025), ("700x520", 1024), ("700x520", 1023), ("640x480", 4000), ("640x480", 1025))
FIVE_KEPT = ((272.0, 272.0), (330.0, 420.0), (120.0, 400.0), (400.0, 120.0))     # "five": octaves 3, 0, 1, 2 in selection order, behind octave 4's
NO_ROWS = ("32x32", "33x40", "63x64", "64x64", "96x33")     # at least 32 pixels a side, yet no row survives the border rule
FEW_ROWS = (("65x65", 2), ("72x70", 1))                 # the smallest inputs here that keep rows
THRESHOLD_IMAGE = "97x131"
THRESHOLD_PHOTO = "golden1"                              # every pair below changes its count; (0.03, 30) does not change 97x131's
THRESHOLDS = ((0.015, 10.0), (0.06, 10.0), (0.03, 3.0), (0.03, 30.0))       # (contrast, edge_r); the defaults are (0.03, 10)


def plan_octaves(w, h):
    """The octave rule of the host file (and of plan_octaves in csrc/features.hip) restated: [(w, h), ...]."""
    n_oct = max(1, int(math.log2(min(w, h))) - 4)
    out = []
    for _ in range(n_oct):
        out.append((w, h))
        w, h = (w + 1) // 2, (h + 1) // 2
        if w < 20 or h < 20:
            break
    return out


# ---- comparisons ---------------------------------------------------------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def descriptor_shares(dev_f32, host_f32):
    diff = np.abs(dev_f32.astype(np.int32) - host_f32.astype(np.int32)).max(axis=1)
    return int((diff > 0).sum()), int((diff > 1).sum())


def check_descriptors(name, dev_f32, host_f32):
    n = host_f32.shape[0]
    any_diff, big_diff = descriptor_shares(dev_f32, host_f32)
    print("features parity %s: rows %d, rows that differ %d (%.4f), rows off by more than 1: %d (%.4f)" %
          (name, n, any_diff, any_diff / n, big_diff, big_diff / n))
    assert any_diff <= max(1, int(0.02 * n)), (name, any_diff, n)
    assert big_diff <= max(1, int(0.005 * n)), (name, big_diff, n)


def check_bit_rows(name, dev_rows, host_rows):
    """The cap of tests/test_features_bits_gpu.py on rows that differ from the host twin's: 2 % of rows, at least one."""
    n = host_rows.shape[0]
    assert dev_rows.shape == host_rows.shape
    differ = int((dev_rows != host_rows).any(axis=1).sum())
    print("features bits parity %s: rows %d, rows that differ %d (%.4f)" % (name, n, differ, differ / n))
    assert differ <= max(1, int(0.02 * n)), (name, differ, n)


# ---- the extrema scan of the host file in numpy float32 --------------------------------------------------------------------

def candidate_responses(ctx, n_oct, contrast=0.03, edge_r=10.0):
    """The extrema scan of the host file restated in numpy float32 on the Gaussian levels of the last device call (or of any
    object with detect_level(octave, level), such as NumpyLevels): |response| of every candidate in selection order
    (descending, ties in scan order)."""
    contrast, edge_r, two, four = np.float32(contrast), np.float32(edge_r), np.float32(2), np.float32(4)
    out = []
    for o in range(n_oct):
        L = [ctx.detect_level(o, i) for i in range(6)]
        dog = [L[i + 1] - L[i] for i in range(5)]
        h, w = dog[0].shape
        for i in (1, 2, 3):
            def sh(d, dy, dx):
                return d[8 + dy:h - 8 + dy, 8 + dx:w - 8 + dx]
            c = sh(dog[i], 0, 0)
            is_max, is_min = np.ones(c.shape, bool), np.ones(c.shape, bool)
            for d in dog[i - 1:i + 2]:
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        is_max &= ~(sh(d, dy, dx) > c)
                        is_min &= ~(sh(d, dy, dx) < c)
            d = dog[i]
            dxx = sh(d, 0, 1) + sh(d, 0, -1) - two * c
            dyy = sh(d, 1, 0) + sh(d, -1, 0) - two * c
            dxy = (sh(d, 1, 1) - sh(d, 1, -1) - sh(d, -1, 1) + sh(d, -1, -1)) / four
            tr, det = dxx + dyy, dxx * dyy - dxy * dxy
            ok = (np.abs(c) > contrast / np.float32(3)) & (is_max | is_min) & ~((det <= 0) | (tr * tr * edge_r >= (edge_r + 1) * (edge_r + 1) * det))
            ys, xs = np.nonzero(ok)
            out += [(-float(abs(c[y, x])), o, i, y, x) for y, x in zip(ys, xs)]
    out.sort()
    return np.array([-v[0] for v in out], np.float32)


# ---- Gaussian levels: a numpy restatement of gaussian() of the host file, double accumulation in the same order

def reflect_index(i, n):
    i = np.array(i)
    for _ in range(4):
        i = np.where(i < 0, -i - 1, i)
        i = np.where(i >= n, 2 * n - 1 - i, i)
    return i


def gaussian_np(plane, sigma):
    r = int(4.0 * sigma + 0.5)
    k = [math.exp(-0.5 * i * i / (sigma * sigma)) for i in range(-r, r + 1)]        # libm exp, like the host
    s = 0.0
    for v in k:
        s += v
    k = [v / s for v in k]
    h, w = plane.shape
    ys = reflect_index(np.arange(-r, h + r), h)
    a = np.zeros((h, w), np.float64)
    for i in range(-r, r + 1):
        a = a + np.float64(k[i + r]) * plane[ys[r + i:r + i + h], :].astype(np.float64)
    tmp = a.astype(np.float32)
    xs = reflect_index(np.arange(-r, w + r), w)
    a = np.zeros((h, w), np.float64)
    for i in range(-r, r + 1):
        a = a + np.float64(k[i + r]) * tmp[:, xs[r + i:r + i + w]].astype(np.float64)
    return a.astype(np.float32)


def octave_levels_np(base):
    """The six Gaussian levels of an octave from its first one, as the host's scale-space loop makes them."""
    sigma0, kf = 1.6, math.pow(2.0, 1.0 / 3)
    levels = [base]
    for i in range(1, 6):
        sp = sigma0 * math.pow(kf, i - 1)
        st = sp * kf
        levels.append(gaussian_np(levels[-1], math.sqrt(st * st - sp * sp)))
    return levels


def first_level_np(img):
    return gaussian_np(img.astype(np.float32) / np.float32(255.0), math.sqrt(max(1.6 * 1.6 - 0.25, 0.01)))


class NumpyLevels:
    """detect_level(octave, level) of an 8-bit image from the numpy restatement alone (no device): what candidate_responses
    needs to count the candidates of a small input on the CPU."""

    def __init__(self, img):
        self.octaves = []
        base = first_level_np(img)
        for _ in plan_octaves(img.shape[1], img.shape[0]):
            self.octaves.append(octave_levels_np(base))
            base = self.octaves[-1][3][::2, ::2]

    def detect_level(self, octave, level):
        return self.octaves[octave][level]


# ---- the host extractor with every argument -------------------------------------------------------------------------------

_DRIVER = None
_TMP = None
_HOST = {}
_RUNS = 0


def _tmp():
    global _TMP
    if _TMP is None:
        _TMP = tempfile.TemporaryDirectory(prefix="features_host_")       # lives as long as the process
    return _TMP.name


def host_driver():
    """Path of the compiled tests/features_host_main.cpp; compiled on first use."""
    global _DRIVER
    if _DRIVER is None:
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
        assert cxx, "no host compiler"
        exe = os.path.join(_tmp(), "features_host_main")
        r = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I" + HOST_DIR, os.path.join(HERE, "features_host_main.cpp"),
                            os.path.join(HOST_DIR, "pm_features.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        _DRIVER = exe
    return _DRIVER


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())


def run_host_driver(pgm, max_kp, contrast, edge_r, kind):
    """One run of the driver on a PGM file -> (kp (n, 2) f32, rows): rows (n, 128) f32 for kind "grad", (n, 32) u8 for "bits"."""
    assert kind in ("grad", "bits")
    global _RUNS
    _RUNS += 1
    out = os.path.join(_tmp(), "out_%d.bin" % _RUNS)
    # nine significant digits name a float32 exactly: the extractor gets the value that ctypes' c_float hands the library
    r = subprocess.run([host_driver(), pgm, str(int(max_kp)), "%.9g" % np.float32(contrast), "%.9g" % np.float32(edge_r), kind, out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    with open(out, "rb") as f:
        raw = f.read()
    os.remove(out)
    n, k = (int(v) for v in np.frombuffer(raw[:8], "<i4"))
    assert n >= 0 and k == (kind == "bits")
    kp = np.frombuffer(raw[8:8 + 8 * n], "<f4").reshape(n, 2).copy()
    body = raw[8 + 8 * n:]
    if kind == "bits":
        assert len(body) == 32 * n
        return kp, np.frombuffer(body, np.uint8).reshape(n, 32).copy()
    assert len(body) == 512 * n
    return kp, np.frombuffer(body, "<f4").reshape(n, 128).copy()


def host_features(name, max_kp=DEFAULT_MAX_KP, contrast=0.03, edge_r=10.0, kind="grad"):
    """The host extractor on image(name), once per argument tuple; the arrays are shared: leave them as they are."""
    key = (name, int(max_kp), float(np.float32(contrast)), float(np.float32(edge_r)), kind)
    if key not in _HOST:
        pgm = os.path.join(_tmp(), name + ".pgm")
        if not os.path.exists(pgm):
            write_pgm(pgm, image(name))
        _HOST[key] = run_host_driver(pgm, max_kp, contrast, edge_r, kind)
    return _HOST[key]
