"""Host side of the bf16 inference form of the map2style heads (csrc/style_heads_bf16.hip, the grouped output stage of csrc/conv_bf16.hip,
psp_encoders.style_level_bf16, GradualStyleEncoder(style_heads_eval_dtype='bf16'), psp_inference --style_heads_dtype): the ABI's
declarations and refusals, the selection switches and the errors that must come before any device call.  No GPU."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from face_mask_inpaint_amd import _lib
from face_mask_inpaint_amd._lib import ConvDesc, FmiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fmi_conv2d_grouped_fwd_bf16", "fmi_fpn_merge_bf16")
BAD, UNSUP = 1, 2


@pytest.fixture(scope="module")
def clib():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        fn = getattr(lib, name)  # AttributeError: the built library lacks the symbol
        fn.argtypes = _lib.SIGNATURES[name]
        fn.restype = ctypes.c_int
    return lib


def test_new_symbols_are_declared_exported_and_bound(clib):
    header = open(os.path.join(ROOT, "include", "fmi_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES
    rows = int(re.search(r"#define FMI_STYLE_SKINNY_ROWS (\d+)\b", header).group(1))
    assert rows in (32, 64, 128)
    # the section names the lines of the reference it replaces
    section = header[header.index("Inference form of the map2style heads"):]
    for cite in ("psp_encoders.py:13-37", "psp_encoders.py:97-98", "psp_encoders.py:140-151", "stylegan2/model.py EqualLinear"):
        assert cite in section, cite
    assert not _lib.Library(_lib.LIB_PATH, strict=True).missing
    from face_mask_inpaint_amd import functional as FF

    assert FF.STYLE_SKINNY_ROWS == rows
    mk = open(os.path.join(ROOT, "face_mask_inpaint_amd", "csrc", "Makefile")).read()
    assert "style_heads_bf16.hip" in mk


def _desc(n, h, w, c, k, kk, stride, pad, g=1, shared=True, x_cs=None, y_cs=None):
    oh, ow = (h + 2 * pad - kk) // stride + 1, (w + 2 * pad - kk) // stride + 1
    return ConvDesc(n, h, w, c, oh, ow, k, x_cs or (c if shared else g * c), y_cs or g * k, kk, kk, stride, pad, 0, 1)


def test_argument_checks_return_before_any_launch(clib):
    """The pointers are host memory: a call that got past its checks would not return a status"""
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    q = ctypes.c_void_p(p.value + 4)  # 4-byte aligned only
    # grouped convolution: (d, G, x_group_off, x, wnk, bias, slope, y16, y32, stream)
    conv = lambda d, g, off, x, w, b, y16, y32: clib.fmi_conv2d_grouped_fwd_bf16(None if d is None else ctypes.byref(d), g, off, x, w, b, 0.01, y16, y32, None)
    d3 = _desc(2, 8, 8, 64, 64, 3, 2, 1, g=3)
    d3g = _desc(2, 8, 8, 64, 64, 3, 2, 1, g=3, shared=False)
    d1 = _desc(2, 1, 1, 64, 64, 1, 1, 0, g=3, shared=False)
    assert conv(None, 3, 0, p, p, p, p, None) == BAD
    assert conv(d3, 3, 0, None, p, p, p, None) == BAD and conv(d3, 3, 0, p, None, p, p, None) == BAD
    assert conv(d3, 3, 0, p, p, p, None, None) == BAD and conv(d3, 3, 0, p, p, p, p, p) == BAD     # neither / both outputs
    assert conv(d1, 3, 64, p, p, p, None, None) == BAD and conv(d1, 3, 64, p, p, p, p, p) == BAD
    assert conv(d3, 0, 0, p, p, p, p, None) == BAD and conv(d3, -2, 0, p, p, p, p, None) == BAD    # G <= 0
    assert conv(d3g, 3, 32, p, p, p, p, None) == BAD and conv(d3g, 3, 128, p, p, p, p, None) == BAD  # x_group_off not in {0, C}
    wrong = _desc(2, 8, 8, 64, 64, 3, 2, 1, g=3)
    wrong.OH = 5
    assert conv(wrong, 3, 0, p, p, p, p, None) == BAD
    wrong = _desc(2, 8, 8, 64, 64, 3, 2, 1, g=3)
    wrong.OW = 3
    assert conv(wrong, 3, 0, p, p, p, p, None) == BAD
    assert conv(_desc(2, 8, 8, 96, 64, 3, 2, 1, g=3), 3, 0, p, p, p, p, None) == UNSUP    # C % 64
    assert conv(_desc(2, 8, 8, 64, 96, 3, 2, 1, g=3), 3, 0, p, p, p, p, None) == UNSUP    # K % 64
    assert conv(_desc(2, 8, 8, 64, 64, 3, 1, 1, g=3), 3, 0, p, p, p, p, None) == UNSUP    # 3x3 stride 1
    assert conv(_desc(2, 8, 8, 64, 64, 5, 2, 2, g=3), 3, 0, p, p, p, p, None) == UNSUP    # 5x5
    assert conv(_desc(2, 8, 8, 64, 64, 3, 2, 0, g=3), 3, 0, p, p, p, p, None) == UNSUP    # 3x3 without its padding
    assert conv(_desc(2, 8, 8, 64, 64, 1, 2, 0, g=3), 3, 0, p, p, p, p, None) == UNSUP    # 1x1 stride 2
    assert conv(d3, 3, 0, p, p, p, None, p) == UNSUP                                      # fp32 output of a 3x3
    for a in range(5):  # x, wnk, bias, y16 / y32 on a 4-byte boundary
        args = [p, p, p, p, None]
        args[a] = q
        if a == 4:
            args[3] = None
        assert conv(d1 if a == 4 else d3, 3, 64 if a == 4 else 0, *args) == UNSUP, a
    assert conv(_desc(2, 8, 8, 64, 64, 3, 2, 1, g=3, x_cs=68), 3, 0, p, p, p, p, None) == UNSUP   # pitches not a multiple of 8
    assert conv(_desc(2, 8, 8, 64, 64, 3, 2, 1, g=3, y_cs=196), 3, 0, p, p, p, p, None) == UNSUP
    assert conv(_desc(2, 8, 8, 64, 64, 3, 2, 1, g=3, y_cs=128), 3, 0, p, p, p, p, None) == BAD    # y narrower than G*K
    assert conv(_desc(2, 8, 8, 64, 64, 3, 2, 1, g=3, shared=False, x_cs=128), 3, 64, p, p, p, p, None) == BAD  # x narrower than G*C
    # merge: (lateral, coarse, p32, p16, N, H, W, CH, CW, C, stream)
    merge = clib.fmi_fpn_merge_bf16
    assert merge(None, p, p, p, 2, 4, 4, 2, 2, 64, None) == BAD and merge(p, p, p, None, 2, 4, 4, 2, 2, 64, None) == BAD
    for i in range(6):
        ext = [2, 4, 4, 2, 2, 64]
        ext[i] = 0
        assert merge(p, p, p, p, *ext, None) == BAD, i
        ext[i] = -1
        assert merge(p, p, p, p, *ext, None) == BAD, i
    assert merge(p, p, p, p, 2, 4, 4, 2, 2, 68, None) == UNSUP                       # C % 8
    for i in range(4):
        a = [p, p, p, p]
        a[i] = q
        assert merge(*a, 2, 4, 4, 2, 2, 64, None) == UNSUP, i
    assert merge(p, None, None, q, 2, 4, 4, 0, 0, 64, None) == UNSUP


def test_psp_inference_flag():
    from face_mask_inpaint_amd.psp_inference import get_args

    assert get_args([]).style_heads_dtype == "fp32"
    assert get_args(["--style_heads_dtype", "bf16"]).style_heads_dtype == "bf16"
    assert get_args(["--style_heads_dtype", "bf16"]).encoder_dtype == "fp32"
    with pytest.raises(SystemExit):
        get_args(["--style_heads_dtype", "fp16"])


def _encoder(heads_dtype, widths=(64, 64, 64, 128, 128)):
    from face_mask_inpaint_amd.modules.psp.encoders.psp_encoders import GradualStyleEncoder

    opts = SimpleNamespace(n_styles=10, use_attention=1)
    if heads_dtype is not None:
        opts.style_heads_eval_dtype = heads_dtype
    torch.manual_seed(0)
    return GradualStyleEncoder(50, "ir_se", opts, _widths=widths, _spatial=(4, 8, 16))


def test_builds_share_one_state_dict():
    a, b, c = _encoder("bf16"), _encoder("fp32"), _encoder(None)
    assert list(a.state_dict()) == list(b.state_dict()) == list(c.state_dict())
    for other in (b, c):
        assert all(torch.equal(v, other.state_dict()[k]) and v.dtype == other.state_dict()[k].dtype for k, v in a.state_dict().items())
    assert a.eval_heads_dtype == torch.bfloat16 and b.eval_heads_dtype == c.eval_heads_dtype == torch.float32
    assert a.eval_body_dtype == torch.float32  # the body is another option
    with pytest.raises(FmiError, match="style_heads_eval_dtype"):
        _encoder("fp16")


def test_bf16_build_refuses_before_any_device_call():
    enc = _encoder("bf16").eval()
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(FmiError, match=r"inference only"):
        enc(x)
    with torch.no_grad():
        with pytest.raises(FmiError, match="no CPU fallback"):
            enc(x)
        odd = _encoder("bf16", widths=(64, 64, 96, 128, 128)).eval()
        with pytest.raises(FmiError, match="multiple of 64"):
            odd(x)
    # training mode is not this option's business: the fp32 path, which meets the CPU tensor first -- grad mode is not refused
    enc.train()
    with pytest.raises(FmiError, match="no CPU fallback"):
        enc(x)
    # the heads' convolutions carry the no-piece-image mark only while the bf16 form is the one that runs
    convs = [m for h in enc.styles for m in h.convs if isinstance(m, torch.nn.Conv2d)]
    assert convs and not any(getattr(m, "_fmi_no_w3", False) for m in convs)
    enc.eval()
    with torch.no_grad(), pytest.raises(FmiError, match="no CPU fallback"):
        enc(x)
    assert all(getattr(m, "_fmi_no_w3", False) for m in convs)
    assert not any(getattr(m, "_fmi_no_w3", False) for m in (enc.latlayer1, enc.latlayer2))
