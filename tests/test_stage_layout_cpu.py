"""CPU: the layout of the device block that the host-pointer entry points stage through (csrc/stage_layout.hpp), through
a C shim built with the host compiler.  Every part starts on a multiple of 256 bytes, parts do not overlap, a part of
zero bytes still owns an address inside the block, and the block is never empty nor padded by more than 256 bytes a part."""
import ctypes as C
import os

import numpy as np
import pytest

import cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def layout():
    L = cref.load("stage_layout_shim", {"stage_layout": [C.c_void_p, C.c_int, C.c_void_p]}, {"stage_layout": C.c_uint64},
                  include=[os.path.join(ROOT, "points_matching_amd", "csrc")])

    def run(sizes):
        sizes = np.ascontiguousarray(sizes, np.uint64)
        off = np.zeros(len(sizes), np.uint64)
        total = L.stage_layout(cref.ptr(sizes), len(sizes), cref.ptr(off))
        return [int(o) for o in off], int(total)
    return run


def check(sizes, off, total):
    sizes = [int(s) for s in sizes]
    assert total > 0
    assert total <= sum(sizes) + 256 * len(sizes)
    end = 0
    for s, o in zip(sizes, off):
        assert o % 256 == 0
        assert o >= end                      # in order, and past everything before it: no overlap
        assert o < total                     # an address inside the block, also for s == 0
        assert o + s <= total
        end = o + max(s, 1)                  # a part of zero bytes shares its address with no other part


@pytest.mark.parametrize("sizes", [[0], [0, 0], [1, 255, 256, 257, 0, 4096], [3 << 30]], ids=str)
def test_named_layouts(layout, sizes):
    off, total = layout(sizes)
    check(sizes, off, total)


def test_exact_offsets(layout):
    assert layout([0]) == ([0], 256)
    assert layout([0, 0]) == ([0, 256], 512)
    assert layout([1, 255, 256, 257, 0, 4096]) == ([0, 256, 512, 768, 1280, 1536], 5632)
    assert layout([3 << 30]) == ([0], 3 << 30)
    assert layout([(3 << 30) + 1, 7]) == ([0, (3 << 30) + 256], (3 << 30) + 512)


def test_random_layouts(layout):
    rng = np.random.default_rng(20261019)
    for _ in range(400):
        n = int(rng.integers(1, 9))
        kind = rng.integers(0, 4, n)
        sizes = np.where(kind == 0, 0, np.where(kind == 1, rng.integers(1, 600, n),
                         np.where(kind == 2, 256 * rng.integers(1, 64, n), rng.integers(1, 1 << 33, n))))
        off, total = layout(sizes)
        check(sizes, off, total)
