"""CPU: csrc/image_args.hpp through tests/image_args_shim.cpp: the byte range of a strided image, the overlap test, the pixel
cap, the computed columns of the two stereo matchers (SPEC S85, S90) against the Python statements of stereo_ref and sgm_ref,
and the buffer rule of a disparity map on the cases that tests/test_sgm_gpu.py gives the device form.  Addresses are plain
integers here: the rules never follow a pointer."""
import ctypes as C
import os

import cref
import sgm_ref as G
import stereo_ref as S

_L = None
_I, _U = C.c_int, C.c_uint64


def lib():
    global _L
    if _L is None:
        _L = cref.load("image_args_shim",
                       {"ia_span": [_I] * 4, "ia_overlap": [_U] * 4, "ia_pixel_cap": [_I, _I], "ia_computed_columns": [_I] * 5 + [C.POINTER(_I)],
                        "ia_disparity_map_ranges": [_U, _U, _I, _I, _I, _I, _U, _I, _U, C.POINTER(C.c_char_p)], "ia_sizeof_info": []},
                       restypes={"ia_span": _U},
                       include=(os.path.join(S.ROOT, "points_matching_amd", "csrc"), os.path.join(S.ROOT, "include")))
    return _L


def test_span_is_the_last_element_s_end():
    for w, h, stride in ((1, 1, 1), (40, 1, 40), (40, 1, 1000), (40, 12, 40), (40, 12, 47), (1, 9, 5), (10000, 10000, 10000), (3, 100000, 30000)):
        for elem in (1, 2, 8):
            assert lib().ia_span(w, h, stride, elem) == ((h - 1) * stride + w) * elem, (w, h, stride, elem)
    assert lib().ia_span(40, 1, 1000, 2) == 80                        # one row: the stride does not count
    assert lib().ia_span(40, 12, 47, 1) == 11 * 47 + 40 < 12 * 47     # the gap behind the last row is not part of the image


def test_overlap():
    ov = lambda a, ab, b, bb: (lib().ia_overlap(a, ab, b, bb), lib().ia_overlap(b, bb, a, ab))
    assert ov(1000, 100, 1100, 50) == (0, 0)                          # end to start: they touch
    assert ov(1000, 101, 1100, 50) == (1, 1)                          # one byte
    assert ov(1000, 100, 1099, 1) == (1, 1)
    assert ov(1000, 100, 1020, 10) == (1, 1)                          # one inside the other
    assert ov(1000, 100, 1000, 100) == (1, 1)
    assert ov(1000, 100, 5000, 100) == (0, 0)
    # a range of no bytes strictly inside another counts as overlapping; at either end of it, it does not
    assert ov(1000, 100, 1050, 0) == (1, 1)
    assert ov(1000, 100, 1000, 0) == (0, 0) and ov(1000, 100, 1100, 0) == (0, 0)
    assert ov(2 ** 40, 2 ** 33, 2 ** 40 + 2 ** 33 - 1, 1) == (1, 1) and ov(2 ** 40, 2 ** 33, 2 ** 40 + 2 ** 33, 1) == (0, 0)


def test_pixel_cap():
    cap = lib().ia_pixel_cap
    assert cap(10000, 10000) == S.PM_OK and cap(10001, 10000) == S.PM_E_UNSUPPORTED and cap(10000, 10001) == S.PM_E_UNSUPPORTED
    assert cap(1, 1) == S.PM_OK and cap(100000000, 1) == S.PM_OK and cap(1, 100000001) == S.PM_E_UNSUPPORTED
    assert cap(2 ** 31 - 1, 2 ** 31 - 1) == S.PM_E_UNSUPPORTED       # the product is formed in 64 bits


def _columns(from_right, margin, dmin, D, w):
    out = (_I * 2)()
    lib().ia_computed_columns(from_right, margin, dmin, dmin + D - 1, w, out)
    return out[0], out[1]


def test_computed_columns_are_the_references():
    n = 0
    for dmin in (-7, 0, 5):
        for D in (1, 12):
            for flags in (0, S.FROM_RIGHT):
                for w in range(1, 41):
                    for radius in (1, 10):
                        assert _columns(flags, radius, dmin, D, w) == S.computed_columns(w, dmin, D, radius, flags), (dmin, D, flags, w, radius)
                    assert _columns(flags, 4, dmin, D, w) == G.computed_rect(w, 16, dmin, D, flags)[:2], (dmin, D, flags, w)
                    x0, x1 = _columns(flags, 4, dmin, D, w)
                    n += x1 >= x0
    assert 0 < n < 3 * 2 * 2 * 40                                    # images with computed columns and images with none


W, H = 40, 12
LEFT, RIGHT, DISP, INFO, BUF = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000


def _ranges(l=LEFT, r=RIGHT, d=DISP, info=INFO, ls=W, rs=W, ds=W):
    why = C.c_char_p()
    rc = lib().ia_disparity_map_ranges(l, r, W, H, ls, rs, d, ds, info, C.byref(why))
    return rc, why.value.decode()


def test_disparity_map_ranges():
    """The map overlaps neither image, the info record none of the three: the cases of test_sgm_gpu.py's argument test."""
    assert lib().ia_sizeof_info() == 8
    assert _ranges() == (S.PM_OK, "") and _ranges(info=0) == (S.PM_OK, "")
    images = "an input image and the disparity map overlap"
    record = "the info record overlaps an image or the map"
    assert _ranges(l=BUF, d=BUF) == (S.PM_E_INVALID, images)                                   # the map on an image
    assert _ranges(l=BUF, d=BUF + W * H - 1) == (S.PM_E_INVALID, images)                       # one byte into the left image
    assert _ranges(l=BUF, d=BUF + W * H)[0] == S.PM_OK
    assert _ranges(r=BUF + 2 * W * H - 1, d=BUF) == (S.PM_E_INVALID, images)                   # the right image starts on the map's last byte
    assert _ranges(r=BUF + 2 * W * H, d=BUF)[0] == S.PM_OK
    assert _ranges(info=DISP + 128) == (S.PM_E_INVALID, record)                                # inside the map
    assert _ranges(info=LEFT + W * H - 4) == (S.PM_E_INVALID, record)                          # half inside the left image
    assert _ranges(info=RIGHT) == (S.PM_E_INVALID, record)
    assert _ranges(info=LEFT + W * H)[0] == S.PM_OK and _ranges(info=DISP - 8)[0] == S.PM_OK and _ranges(info=DISP - 7)[0] == S.PM_E_INVALID
    # the images may overlap each other (one buffer as both views), and the message of the images comes first
    assert _ranges(l=LEFT, r=LEFT)[0] == S.PM_OK and _ranges(l=BUF, d=BUF, info=BUF) == (S.PM_E_INVALID, images)
    # strides: the ranges are those of the strided images, 2 bytes per element of the map
    assert _ranges(l=BUF, ls=50, d=BUF + 11 * 50 + W)[0] == S.PM_OK and _ranges(l=BUF, ls=50, d=BUF + 11 * 50 + W - 1)[0] == S.PM_E_INVALID
    assert _ranges(d=BUF, ds=50, info=BUF + 2 * (11 * 50 + W))[0] == S.PM_OK and _ranges(d=BUF, ds=50, info=BUF + 2 * (11 * 50 + W) - 1)[0] == S.PM_E_INVALID
