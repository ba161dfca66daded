"""Host side of fmi_conv_transpose2d_pair_bwd_f32 (csrc/convt3x3_bwd.hip): what the entry refuses comes back as a status code before anything
is launched, so this runs on a machine without a GPU."""
import ctypes

import pytest


def test_pair_backward_refusals_without_a_gpu():
    import os

    from face_mask_inpaint_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfmi_hip.so not built")
    c = ctypes.CDLL(_lib.LIB_PATH)
    BAD = 1
    PD, vp, i32, i64 = ctypes.POINTER(_lib.ConvDesc), ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    sup, nbytes, bwd = c.fmi_conv_transpose2d_pair_bwd_supported, c.fmi_conv_transpose2d_pair_bwd_ws_bytes, c.fmi_conv_transpose2d_pair_bwd_f32
    sup.argtypes = nbytes.argtypes = [PD, i32, i32]
    bwd.argtypes = _lib.SIGNATURES["fmi_conv_transpose2d_pair_bwd_f32"]

    def desc(cb, cs1, h=8, w=16):
        return _lib.ConvDesc(N=1, H=2 * h, W=2 * w, C=cb, OH=h, OW=w, K=cs1, x_cstride=cb, y_cstride=cs1, kh=3, kw=3, stride=2, pad=1, pad_mode=0)

    d = desc(32, 32)
    for cs1, cs2 in ((32, 32), (32, 64), (64, 32), (64, 64)):
        dd = desc(32, cs1)
        assert sup(ctypes.byref(dd), cs1, cs2) == 1
        assert nbytes(ctypes.byref(dd), cs1, cs2) == 2 * (9 * 32 * (cs1 + cs2) + 32) * 4  # 2 x 1 tiles of 4 x 16 pixels
    assert sup(None, 32, 32) == 0 and nbytes(None, 32, 32) == 0
    assert sup(ctypes.byref(desc(28, 16)), 16, 48) == 0  # cb = 28
    assert sup(ctypes.byref(desc(32, 16)), 16, 32) == 0  # 16-channel inputs
    assert sup(ctypes.byref(d), 32, 16) == 0
    assert sup(ctypes.byref(desc(64, 64)), 64, 128) == 0  # the second-last block's class
    assert sup(ctypes.byref(d), 64, 32) == 0  # d->K is x1's channel count
    d1 = _lib.ConvDesc(N=1, H=16, W=32, C=32, OH=16, OW=32, K=32, x_cstride=32, y_cstride=32, kh=3, kw=3, stride=1, pad=1, pad_mode=0)
    assert sup(ctypes.byref(d1), 32, 32) == 0  # not the stride-2 geometry
    buf = (ctypes.c_float * 1024)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    row = (9 * 32 * 64 + 32) * 4
    assert bwd(None, a, a, 32, a, a, a, None, None, None, None, None, a, 2 * row, None) == BAD           # null descriptor
    assert bwd(ctypes.byref(d), None, a, 32, a, a, a, None, None, None, None, None, a, 2 * row, None) == BAD  # x1 = NULL
    assert bwd(ctypes.byref(d), a, a, 32, a, a, a, None, None, None, None, None, None, 2 * row, None) == BAD  # no workspace
    assert bwd(ctypes.byref(d), a, a, 32, a, a, a, None, None, None, None, None, a, row - 4, None) == BAD      # shorter than one row
    assert bwd(ctypes.byref(d), a + 4, a, 32, a, a, a, None, None, None, None, None, a, 2 * row, None) == BAD  # misaligned x1
    assert bwd(ctypes.byref(d), a, a, 32, a, a, a, a + 8, None, None, None, None, a, 2 * row, None) == BAD     # misaligned dx1
    assert bwd(ctypes.byref(d), a, a, 16, a, a, a, None, None, None, None, None, a, 2 * row, None) == 2        # K2 = 16: unsupported
