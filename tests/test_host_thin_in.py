"""Host side of the thin-input convolution entries (csrc/thinin.hip): the predicate, the workspace size and what the entries refuse come
back before anything is launched, so this runs on a machine without a GPU."""
import ctypes

import pytest


def _desc(_lib, c, k, ks=3, n=1, h=8, w=64, stride=1, pad=None, pad_mode=0, xcs=None, ycs=None, dil=0):
    pad = ks // 2 if pad is None else pad
    return _lib.ConvDesc(N=n, H=h, W=w, C=c, OH=h, OW=w, K=k, x_cstride=c if xcs is None else xcs, y_cstride=k if ycs is None else ycs,
                         kh=ks, kw=ks, stride=stride, pad=pad, pad_mode=pad_mode, dil=dil)


def test_thin_in_predicate_workspace_and_refusals_without_a_gpu():
    import os

    from face_mask_inpaint_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfmi_hip.so not built")
    c = ctypes.CDLL(_lib.LIB_PATH)
    BAD, UNSUP = 1, 2
    PD = ctypes.POINTER(_lib.ConvDesc)
    sup, nbytes, fwd, wgrad = c.fmi_conv2d_thin_in_supported, c.fmi_conv2d_thin_in_wgrad_ws_bytes, c.fmi_conv2d_thin_in_fwd_f32, c.fmi_conv2d_thin_in_wgrad_f32
    routed = c.fmi_conv2d_thin_in_routed
    sup.argtypes = nbytes.argtypes = routed.argtypes = [PD]
    fwd.argtypes = _lib.SIGNATURES["fmi_conv2d_thin_in_fwd_f32"]
    wgrad.argtypes = _lib.SIGNATURES["fmi_conv2d_thin_in_wgrad_f32"]
    ref = ctypes.byref

    # the workload's classes
    for cc, k, ks in ((3, 32, 3), (3, 64, 3), (3, 32, 1), (1, 8, 3), (4, 64, 1)):
        assert sup(ref(_desc(_lib, cc, k, ks))) == 1, (cc, k, ks)
    assert sup(None) == 0 and nbytes(None) == 0 and routed(None) == 0
    # the dispatch sends the class to these kernels from 131072 pixels on (8 x 128 x 128, the smallest shape timed against the generic path)
    assert routed(ref(_desc(_lib, 3, 32, 1, n=8, h=128, w=128))) == 1 and routed(ref(_desc(_lib, 3, 64, 3, n=24, h=224, w=224))) == 1
    assert routed(ref(_desc(_lib, 3, 32, 3, n=8, h=128, w=127))) == 0 and routed(ref(_desc(_lib, 3, 32, 3))) == 0
    assert routed(ref(_desc(_lib, 5, 32, 3, n=8, h=256, w=256))) == 0 and routed(ref(_desc(_lib, 3, 32, 3, n=8, h=256, w=256, pad_mode=1))) == 0
    refused = {
        "C = 5": _desc(_lib, 5, 32), "K = 12": _desc(_lib, 3, 12), "K = 128": _desc(_lib, 3, 128), "stride 2": _desc(_lib, 3, 32, stride=2),
        "reflect": _desc(_lib, 3, 32, pad_mode=1), "x pitch": _desc(_lib, 3, 32, xcs=4), "y pitch": _desc(_lib, 3, 32, ycs=64),
        "5x5": _desc(_lib, 3, 32, ks=5), "3x3 pad 0": _desc(_lib, 3, 32, pad=0), "dilated": _desc(_lib, 3, 32, dil=2),
    }
    for why, d in refused.items():
        assert sup(ref(d)) == 0 and nbytes(ref(d)) == 0, why

    # rows x (taps*C*K + K) floats; a tile = 256 / P runs of 4 pixels, P = K/4 rounded up to a power of two, at most 1024 rows
    assert nbytes(ref(_desc(_lib, 3, 32, 3, n=1, h=8, w=64))) == 4 * (27 * 32 + 32) * 4          # 128 runs / 32 = 4 tiles
    assert nbytes(ref(_desc(_lib, 3, 32, 3, n=1, h=8, w=63))) == 4 * (27 * 32 + 32) * 4          # ragged rows: still 16 runs each
    assert nbytes(ref(_desc(_lib, 3, 64, 3, n=1, h=8, w=64))) == 8 * (27 * 64 + 64) * 4          # P = 16: 16 runs per tile
    assert nbytes(ref(_desc(_lib, 4, 24, 1, n=1, h=8, w=64))) == 4 * (4 * 24 + 24) * 4           # K/4 = 6 -> P = 8
    assert nbytes(ref(_desc(_lib, 1, 8, 3, n=1, h=1, w=1))) == 1 * (9 * 8 + 8) * 4
    assert nbytes(ref(_desc(_lib, 3, 32, 3, n=8, h=256, w=256))) == 1024 * (27 * 32 + 32) * 4    # 4096 tiles: the cap

    buf = (ctypes.c_float * 8192)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    d = _desc(_lib, 3, 32, 3)
    row = (27 * 32 + 32) * 4
    assert wgrad(None, a, a, a, a, a, 4 * row, None) == BAD            # null descriptor
    assert wgrad(ref(d), None, a, a, a, a, 4 * row, None) == BAD       # x = NULL
    assert wgrad(ref(d), a, None, a, a, a, 4 * row, None) == BAD       # dy = NULL
    assert wgrad(ref(d), a, a, None, a, a, 4 * row, None) == BAD       # dwf = NULL
    assert wgrad(ref(d), a, a, a, a, None, 4 * row, None) == BAD       # no workspace
    assert wgrad(ref(d), a, a, a, a, a, row - 4, None) == BAD          # shorter than one row
    assert wgrad(ref(d), a, a, a, a, a + 4, 4 * row, None) == BAD      # misaligned workspace
    assert wgrad(ref(refused["C = 5"]), a, a, a, a, a, 4 * row, None) == UNSUP
    assert wgrad(ref(d), a, a + 4, a, a, a, 4 * row, None) == UNSUP    # dy rows off 16-byte alignment
    assert fwd(None, a, a, None, None, a, 0, None) == BAD
    assert fwd(ref(d), None, a, None, None, a, 0, None) == BAD         # x = NULL
    assert fwd(ref(d), a, None, None, None, a, 0, None) == BAD         # wf = NULL
    assert fwd(ref(d), a, a, None, None, None, 0, None) == BAD         # y = NULL
    assert fwd(ref(d), a, a, None, None, a, 3, None) == BAD            # activation code
    assert fwd(ref(refused["stride 2"]), a, a, None, None, a, 0, None) == UNSUP
    assert fwd(ref(d), a, a, None, None, a + 4, 0, None) == UNSUP      # y rows off 16-byte alignment
