"""CPU: the minimal-sample draws of csrc/sample_core.hpp (sample8, and sample_walk at every family's sample size and stream
constants), compiled by the host compiler alone through tests/sampler_shim.cpp, against the references the other tests
already use: the oracle's pmo_sample8 / pmo_sample7, hr_sample4, affine_ref.ar_sample (both models), er_sample,
pr_sample and align3d_ref.ar_sample.  Every index of every case must be equal.

Cases per family (sample size K): n in {K, K + 1, 2K, 97, 2^31 - 1}; h in [0, 20000) at n = K, 200 values elsewhere
(2^32 - 1 and 2^63 among them); three seeds.  The rare branches must really be reached: a numpy restatement of the draws
counts the n = K cases whose 64 draws do not cover all K values (the smallest-unused-integer fill) and the K = 8 cases
with a repeat among the first eight draws (sample8's slow path).  For K <= 4 the fill has probability ~1e-11 per case and is
not looked for.  With seed 20261021 and h in [0, 20000) the counts are 27 (K = 8), 3 (K = 7), 1 (K = 5), 0 (K = 4)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import affine_ref
import align3d_ref
import cref
import essential_ref
import homography_ref
import pnp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "points_matching_amd", "csrc")
SEEDS = (20261021, 0, 0xFFFFFFFFFFFFFFFF)
H_SALT = 0xD1B54A32D192ED03
U64 = np.uint64


@pytest.fixture(scope="module")
def shim():
    return cref.load("sampler_shim", {"sampler_size": [C.c_int], "sampler_salt": [C.c_int, C.c_int],
                                      "sampler_batch": [C.c_int, C.c_uint64, C.c_void_p, C.c_int, C.c_int, C.c_void_p]},
                     {"sampler_salt": C.c_uint64}, include=[CSRC])


def families(oracle):
    """name -> (shim family, K, reference f(seed, h, n, pointer to K int32))"""
    o, hr, af, er, pr, al = oracle.lib(), homography_ref.lib(), affine_ref.lib(), essential_ref.lib(), pnp_ref.lib(), align3d_ref.lib()
    u64, vp = C.c_uint64, C.c_void_p
    return {
        "F": (0, 8, lambda s, h, n, p: o.pmo_sample8(u64(s), u64(h), n, vp(p))),
        "LMedS": (1, 7, lambda s, h, n, p: o.pmo_sample7(u64(s), u64(h), n, vp(p))),
        "H": (2, 4, lambda s, h, n, p: hr.hr_sample4(s, h, n, p)),
        "A-full": (3, 3, lambda s, h, n, p: af.ar_sample(0, s, h, n, p)),
        "A-partial": (4, 2, lambda s, h, n, p: af.ar_sample(1, s, h, n, p)),
        "E": (5, 5, lambda s, h, n, p: er.er_sample(s, h, n, p)),
        "PnP": (6, 3, lambda s, h, n, p: pr.pr_sample(s, h, n, p)),
        "X": (7, 3, lambda s, h, n, p: al.ar_sample(s, h, n, p)),
    }


NAMES = ["F", "LMedS", "H", "A-full", "A-partial", "E", "PnP", "X"]


def mix64(z):
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def draws(seed, hs, n, salt, h_salt, count):
    """cand[i, d] of SPEC S6 for h = hs[i], d < count: this file's own restatement, used only to count the rare cases"""
    with np.errstate(over="ignore"):
        stream = mix64(U64(seed) ^ U64(salt)) ^ mix64(hs + U64(h_salt))
        d = np.arange(1, count + 1, dtype=U64)
        r = mix64(stream[:, None] + d[None, :] * U64(0x9E3779B97F4A7C15))
        return ((r >> U64(32)) * U64(n)) >> U64(32)


def h_values(n, k):
    if n == k:
        return np.arange(20000, dtype=U64)
    rng = np.random.default_rng(n)
    return np.concatenate([rng.integers(0, 2 ** 64, 198, dtype=U64), np.array([2 ** 32 - 1, 2 ** 63], U64)])


@pytest.mark.parametrize("name", NAMES)
def test_every_index_equals_the_reference(shim, oracle, name):
    fam, k, ref = families(oracle)[name]
    assert shim.sampler_size(fam) == k
    salt, h_salt = shim.sampler_salt(fam, 0), shim.sampler_salt(fam, 1)
    fills = {}
    slow8 = 0
    for n in (k, k + 1, 2 * k, 97, 2 ** 31 - 1):
        hs = h_values(n, k)
        for seed in SEEDS:
            got = np.full((len(hs), k), -7, np.int32)
            assert shim.sampler_batch(fam, seed, cref.ptr(hs), len(hs), n, cref.ptr(got)) == k
            want = np.full((len(hs), k), -9, np.int32)
            base = want.ctypes.data
            for i, h in enumerate(hs.tolist()):
                ref(seed, h, n, base + 4 * k * i)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (name, n, seed, int(hs[bad[0]]), got[bad[0]], want[bad[0]])
            assert (np.sort(got, axis=1)[:, 1:] != np.sort(got, axis=1)[:, :-1]).all() and got.min() >= 0 and got.max() < n
            if n == k:
                c = np.sort(draws(seed, hs, n, salt, h_salt, 64), axis=1)
                distinct = 1 + (c[:, 1:] != c[:, :-1]).sum(axis=1)
                fills[seed] = int((distinct < k).sum())
            if k == 8:
                c = np.sort(draws(seed, hs, n, salt, h_salt, 8), axis=1)
                slow8 += int((c[:, 1:] == c[:, :-1]).any(axis=1).sum())
    print(name, "fill cases at n = K per seed:", fills, "sample8 slow-path cases:", slow8)
    if k >= 7:
        assert fills[SEEDS[0]] >= 1          # the smallest-unused-integer fill was compared, not just the draws
    if k == 8:
        assert slow8 >= 1


def test_named_stream_constants_of_the_families(shim):
    """The constants the kernels pass to sample_walk, read from the text next to each family, are the ones checked above."""
    def named(path, name):
        text = open(os.path.join(CSRC, path)).read()
        return [int(v, 16) for v in re.findall(r"\b%s = (0x[0-9A-Fa-f]{16})ULL" % name, text)]
    assert named("lmeds.hip", "LM_STREAM") == [shim.sampler_salt(1, 0)]
    assert named("homography_core.hpp", "STREAM") == [shim.sampler_salt(2, 0)]
    assert named("affine_core.hpp", "STREAM") == [shim.sampler_salt(3, 0), shim.sampler_salt(4, 0)]      # FULL, PARTIAL
    assert named("essential_core.hpp", "STREAM") == [shim.sampler_salt(5, 0)]
    assert named("pnp_core.hpp", "STREAM") == [shim.sampler_salt(6, 0)]
    assert named("align3d_core.hpp", "STREAM") == [shim.sampler_salt(7, 0)]
    assert named("align3d_core.hpp", "STREAM_H") == [shim.sampler_salt(7, 1)]
    assert all(shim.sampler_salt(f, 1) == H_SALT for f in range(7))


def test_the_header_needs_only_a_host_compiler():
    """sample_core.hpp includes <cstdint> and nothing else (the shim above was built with no HIP header in reach)."""
    text = open(os.path.join(CSRC, "sample_core.hpp")).read()
    assert re.findall(r"^\s*#\s*include\s*(\S+)", text, re.M) == ["<cstdint>"]
