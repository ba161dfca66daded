"""Host side of the bf16 inference form of the IR-SE body (csrc/irse_infer_bf16.hip, the per-column output stage of csrc/conv_bf16.hip,
helpers._Bottleneck.infer_bf16, GradualStyleEncoder(encoder_eval_dtype='bf16'), psp_inference --encoder_dtype): the ABI's declarations
and refusals, the selection switches and the errors that must come before any device call.  No GPU."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from face_mask_inpaint_amd import _lib
from face_mask_inpaint_amd._lib import ConvDesc, FmiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fmi_conv2d_fwd_chan_bf16", "fmi_se_gate_f32", "fmi_irse_tail_bf16", "fmi_irse_stem_bf16")
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
    assert "#define FMI_CHAN_COLSUM_ROWS 64" in header
    # every entry names the lines of the reference's helpers.py it replaces
    section = header[header.index("Inference form of the IR-SE bottleneck blocks"):]
    assert section.count("helpers.py:") >= 8
    assert not _lib.Library(_lib.LIB_PATH, strict=True).missing
    from face_mask_inpaint_amd import functional as FF

    assert FF.CHAN_COLSUM_ROWS == 64


def _desc(n, h, w, c, k, kk, stride, pad):
    oh, ow = (h + 2 * pad - kk) // stride + 1, (w + 2 * pad - kk) // stride + 1
    return ConvDesc(n, h, w, c, oh, ow, k, c, k, kk, kk, stride, pad, 0, 1)


def test_argument_checks_return_before_any_launch(clib):
    """The pointers are host memory: a call that got past its checks would not return a status"""
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    q = ctypes.c_void_p(p.value + 4)  # 4-byte aligned only
    c = clib
    # convolution: (d, x, wnk, scale, bias, slope, y, colsum, colsum_floats, stream)
    d = _desc(2, 16, 16, 64, 64, 3, 1, 1)
    conv = lambda d, *a: c.fmi_conv2d_fwd_chan_bf16(ctypes.byref(d), *a, None)
    for bad in ((None, p, p), (p, None, p), (p, p, None)):
        assert conv(d, bad[0], bad[1], p, p, p, bad[2], None, 0) == BAD
    assert c.fmi_conv2d_fwd_chan_bf16(None, p, p, p, p, p, p, None, 0, None) == BAD
    assert conv(_desc(2, 16, 16, 96, 64, 3, 1, 1), p, p, None, None, None, p, None, 0) == UNSUP   # C % 64
    assert conv(_desc(2, 16, 16, 64, 96, 3, 1, 1), p, p, None, None, None, p, None, 0) == UNSUP   # K % 64
    assert conv(_desc(2, 16, 16, 64, 64, 3, 3, 1), p, p, None, None, None, p, None, 0) == UNSUP   # stride 3
    assert conv(_desc(2, 16, 16, 64, 64, 1, 3, 0), p, p, None, None, None, p, None, 0) == UNSUP
    assert conv(_desc(2, 16, 16, 64, 64, 3, 1, 0), p, p, None, None, None, p, None, 0) == UNSUP   # 3x3 without its padding
    assert conv(_desc(2, 16, 16, 64, 64, 5, 1, 2), p, p, None, None, None, p, None, 0) == UNSUP   # 5x5
    assert conv(_desc(2, 8, 8, 128, 128, 3, 1, 1), p, p, p, p, None, p, p, 1 << 20) == UNSUP      # column sums on a 64-pixel map
    assert conv(_desc(2, 16, 16, 64, 64, 3, 2, 1), p, p, p, p, None, p, p, 1 << 20) == UNSUP      # ... and on the 8 x 8 output of stride 2
    assert conv(d, p, p, p, p, None, p, p, 8 * 2 * 64 - 1) == BAD                                  # workspace one float short
    assert conv(d, p, p, q, None, None, p, None, 0) == UNSUP and conv(d, p, p, None, None, q, p, None, 0) == UNSUP
    assert conv(d, p, p, None, None, None, p, q, 1 << 20) == UNSUP
    # SE gate: (part, rows_per_part, P, inv_count, fc1, fc2, gates, N, C, stream)
    for bad in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert c.fmi_se_gate_f32(bad[0], 64, 256, 1.0, bad[1], bad[2], bad[3], 2, 64, None) == BAD
    assert c.fmi_se_gate_f32(p, 64, 256, 1.0, p, p, p, 0, 64, None) == BAD
    assert c.fmi_se_gate_f32(p, -1, 256, 1.0, p, p, p, 2, 64, None) == BAD
    assert c.fmi_se_gate_f32(p, 64, 256, 1.0, p, p, p, 2, 72, None) == UNSUP    # C % 16
    assert c.fmi_se_gate_f32(p, 64, 256, 1.0, p, p, p, 2, 1024, None) == UNSUP  # C > 512
    assert c.fmi_se_gate_f32(p, 64, 63, 1.0, p, p, p, 2, 64, None) == UNSUP     # a partial block would touch three samples
    # tail: (r, gate, sc, next_scale, next_shift, y, z, tap, N, OH, OW, C, SH, SW, sc_stride, stream)
    tail = c.fmi_irse_tail_bf16
    for bad in ((None, p, p), (p, None, p), (p, p, None)):
        assert tail(bad[0], p, bad[1], p, p, bad[2], p, p, 1, 4, 4, 64, 4, 4, 1, None) == BAD
    assert tail(p, p, p, None, p, p, p, None, 1, 4, 4, 64, 4, 4, 1, None) == BAD   # z without its scale
    assert tail(p, p, p, p, None, p, p, None, 1, 4, 4, 64, 4, 4, 1, None) == BAD
    assert tail(p, p, p, p, p, p, p, p, 1, 4, 4, 64, 4, 4, 3, None) == UNSUP       # stride 3
    assert tail(p, p, p, p, p, p, p, p, 1, 4, 4, 64, 4, 4, 2, None) == BAD         # a 4 x 4 shortcut at stride 2 gives 2 x 2
    assert tail(p, p, p, p, p, p, p, p, 1, 4, 4, 68, 4, 4, 1, None) == UNSUP       # C % 8
    assert tail(p, q, p, p, p, p, p, p, 1, 4, 4, 64, 4, 4, 1, None) == UNSUP
    assert tail(p, p, p, p, p, p, p, q, 1, 4, 4, 64, 4, 4, 1, None) == UNSUP
    # stem hand-over: (x, scale, shift, y, z, rows, C, stream)
    stem = c.fmi_irse_stem_bf16
    for i in range(5):
        a = [p] * 5
        a[i] = None
        assert stem(*a, 16, 64, None) == BAD
    assert stem(p, p, p, p, p, 0, 64, None) == BAD
    assert stem(p, p, p, p, p, 16, 68, None) == UNSUP and stem(p, p, q, p, p, 16, 64, None) == UNSUP


def test_psp_inference_flag():
    from face_mask_inpaint_amd.psp_inference import get_args

    assert get_args([]).encoder_dtype == "fp32"
    assert get_args(["--encoder_dtype", "bf16"]).encoder_dtype == "bf16"
    with pytest.raises(SystemExit):
        get_args(["--encoder_dtype", "fp16"])


def _encoder(eval_dtype, widths=(64, 64, 64, 128, 128)):
    from face_mask_inpaint_amd.modules.psp.encoders.psp_encoders import GradualStyleEncoder

    opts = SimpleNamespace(n_styles=10, use_attention=1)
    if eval_dtype is not None:
        opts.encoder_eval_dtype = eval_dtype
    torch.manual_seed(0)
    return GradualStyleEncoder(50, "ir_se", opts, _widths=widths, _spatial=(4, 8, 16))


def test_builds_share_one_state_dict():
    a, b, c = _encoder("bf16"), _encoder("fp32"), _encoder(None)
    assert list(a.state_dict()) == list(b.state_dict()) == list(c.state_dict())
    assert all(torch.equal(v, b.state_dict()[k]) and v.dtype == b.state_dict()[k].dtype for k, v in a.state_dict().items())
    assert a.eval_body_dtype == torch.bfloat16 and b.eval_body_dtype == c.eval_body_dtype == torch.float32
    assert a.body_dtype == torch.float32  # the training body is another option
    with pytest.raises(FmiError, match="encoder_eval_dtype"):
        _encoder("fp16")


def test_bf16_build_refuses_before_any_device_call():
    enc = _encoder("bf16").eval()
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(FmiError, match=r"inference only \(no backward\)"):
        enc(x)
    with torch.no_grad():
        with pytest.raises(FmiError, match="no CPU fallback"):
            enc(x)
        odd = _encoder("bf16", widths=(64, 64, 96, 128, 128)).eval()
        with pytest.raises(FmiError, match="multiple of 64"):
            odd(x)
    # training mode is not this option's business: the fp32 body, which meets the CPU tensor first
    enc.train()
    with pytest.raises(FmiError, match="no CPU fallback"):
        enc(x)


def test_kept_constants_join_the_list_a_training_pass_drops():
    """helpers.batch_norm forgets every constant folded from the running statistics when it updates them through raw pointers; the
    inference form's attribute must be on that list (source check: the update itself needs the device)"""
    import inspect

    from face_mask_inpaint_amd.modules.psp.encoders import helpers

    assert '"_fmi_infer"' in inspect.getsource(helpers.batch_norm) and '"_fmi_infer"' in inspect.getsource(helpers.fold_bn_eval)
    bn = torch.nn.BatchNorm2d(8).eval()
    s, t = helpers.fold_bn_eval(bn)
    assert getattr(bn, "_fmi_infer", None) is None  # trainable parameters: nothing is kept
    for p_ in bn.parameters():
        p_.requires_grad_(False)
    s, t = helpers.fold_bn_eval(bn)
    assert helpers.fold_bn_eval(bn)[0] is s
    bn.running_var.mul_(2.0)  # a visible in-place change: the version counter moves
    s2, _ = helpers.fold_bn_eval(bn)
    assert s2 is not s and torch.allclose(s2 * 2 ** 0.5, s)
