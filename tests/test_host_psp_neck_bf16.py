"""Host side of the bf16 stem and neck of the pSp encoder (csrc: fmi_irse_stem_fwd_bf16, fmi_mask_blend_bf16, fmi_fpn_merge_in_bf16, the
guided attention at the pSp shapes; psp_encoders.neck_bf16, GradualStyleEncoder(encoder_neck_eval_dtype='bf16'), psp_inference
--neck_dtype): the ABI's declarations and refusals, the flag, the constructor and forward refusals, and the float64 restatements of
tests/test_gpu_psp_neck_bf16.py against oracle/psp_cpu.py and the reference-generated fixtures -- none of this needs (or touches) a GPU."""
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from face_mask_inpaint_amd import _lib
from face_mask_inpaint_amd._lib import FmiError

NEW = ["fmi_irse_stem_fwd_bf16", "fmi_mask_blend_bf16", "fmi_fpn_merge_in_bf16", "fmi_guided_attention_sliced_fwd_bf16"]
OK, BAD, UNSUP = 0, 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def clib():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        fn = getattr(lib, name)  # AttributeError: the built library lacks the symbol
        fn.argtypes = _lib.SIGNATURES[name]
        fn.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def ptrs():
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 15) & ~15)
    q = ctypes.c_void_p(p.value + 2)  # 2-byte aligned only
    return buf, p, q


def _desc(n=1, h=8, w=16, c=3, k=64, ks=3, stride=1, pad=1, oh=None):
    o = lambda e: (e + 2 * pad - ks) // stride + 1
    return _lib.ConvDesc(n, h, w, c, o(h) if oh is None else oh, o(w), k, c, k, ks, ks, stride, pad, 0, 1)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound(clib):
    header = open(os.path.join(ROOT, "include", "fmi_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and f"int {name}(" in header, name
    assert "(64, 256)" in header and "(128, 512)" in header  # the sliced guided attention's accepted set
    assert not _lib.Library(_lib.LIB_PATH, strict=True).missing
    from face_mask_inpaint_amd import functional as FF

    assert FF.GUIDED_ATTENTION_BF16_SHAPES == ((32, 128), (64, 256), (128, 512))


def test_stem_refusals_return_before_any_launch(clib, ptrs):
    """(d, x, wf, scale, shift, slope, scale0, shift0, y, z, a32, stream).  The pointers are host memory: a call that got past its checks
    would not return a status"""
    _, p, q = ptrs
    f = clib.fmi_irse_stem_fwd_bf16
    d = _desc()
    assert f(None, *[p] * 10, None) == BAD
    for i in range(9):  # every operand but the debug output is required
        a = [p] * 10
        a[i] = None
        assert f(ctypes.byref(d), *a, None) == BAD, i
    assert f(ctypes.byref(_desc(n=0)), *[p] * 10, None) == BAD
    assert f(ctypes.byref(_desc(oh=9)), *[p] * 10, None) == BAD  # an output extent that does not follow
    for bad in (_desc(c=5), _desc(k=60), _desc(k=264), _desc(stride=2), _desc(ks=1, pad=0), _desc(ks=5, pad=2)):
        assert f(ctypes.byref(bad), *[p] * 10, None) == UNSUP
        assert f(ctypes.byref(bad), q, *[p] * 9, None) == UNSUP  # an unsupported shape is refused whatever the pointers are
    for i in (7, 8, 9):  # y, z, a32 off 16-byte alignment
        a = [p] * 10
        a[i] = q
        assert f(ctypes.byref(d), *a, None) == UNSUP, i


def test_blend_and_merge_refusals_return_before_any_launch(clib, ptrs):
    _, p, q = ptrs
    f = clib.fmi_mask_blend_bf16  # (r, c, m, y, rows, C, stream)
    for i in range(4):
        a = [p] * 4
        a[i] = None
        assert f(*a, 35, 64, None) == BAD, i
    assert f(p, p, p, p, 0, 64, None) == BAD and f(p, p, p, p, 35, 0, None) == BAD
    assert f(p, p, p, p, 35, 60, None) == UNSUP  # C % 8
    for i in (0, 1, 3):
        a = [p] * 4
        a[i] = q
        assert f(*a, 35, 64, None) == UNSUP, i
    g = clib.fmi_fpn_merge_in_bf16  # (lateral, coarse, p16, N, H, W, CH, CW, C, stream)
    for i in range(3):
        a = [p] * 3
        a[i] = None
        assert g(*a, 2, 6, 10, 3, 5, 64, None) == BAD, i
    assert g(p, p, p, 0, 6, 10, 3, 5, 64, None) == BAD and g(p, p, p, 2, 6, 10, 0, 5, 64, None) == BAD
    assert g(p, p, p, 2, 6, 10, 3, 5, 60, None) == UNSUP
    for i in range(3):
        a = [p] * 3
        a[i] = q
        assert g(*a, 2, 6, 10, 3, 5, 64, None) == UNSUP, i


def test_guided_attention_refusals_at_the_psp_shapes(clib, ptrs):
    """(q, src, ref, mask, out, N, T, D, C, waves, stream): (64, 256) and (128, 512) get the checks (32, 128) gets at its own entry"""
    _, p, q = ptrs
    f = clib.fmi_guided_attention_sliced_fwd_bf16
    for d, c in ((64, 256), (128, 512)):
        for i in range(5):
            a = [p] * 5
            a[i] = None
            assert f(*a, 1, 128, d, c, 0, None) == BAD, (d, c, i)
            a[i] = q
            assert f(*a, 1, 128, d, c, 0, None) == BAD, (d, c, i)
        assert f(p, p, p, p, p, 1, 192, d, c, 0, None) == UNSUP      # T % 128
        assert f(p, p, p, p, p, 1, 128, d, c, 8, None) == UNSUP      # eight waves own 256 queries
        assert f(p, p, p, p, p, 65536, 128, d, c, 0, None) == UNSUP
    for d, c in ((32, 128), (64, 512), (128, 256), (256, 1024), (32, 256)):
        assert f(p, p, p, p, p, 1, 128, d, c, 0, None) == UNSUP, (d, c)


# ---- the flag, the option, the refusals --------------------------------------------------------------------------------------------------
def test_flag_parsing_and_defaults():
    from face_mask_inpaint_amd.psp_inference import get_args

    assert get_args([]).neck_dtype == "fp32"
    a = get_args(["--neck_dtype", "bf16"])
    assert a.neck_dtype == "bf16" and a.encoder_dtype == "fp32" and a.style_heads_dtype == "fp32"
    with pytest.raises(SystemExit):
        get_args(["--neck_dtype", "fp16"])


def _enc(widths=(64, 64, 64, 128, 128), **opt):
    from face_mask_inpaint_amd.modules.psp.encoders.psp_encoders import GradualStyleEncoder

    torch.manual_seed(5)
    return GradualStyleEncoder(50, "ir_se", SimpleNamespace(n_styles=10, use_attention=True, **opt), _widths=widths, _spatial=(16, 32, 64))


ALL16 = dict(encoder_eval_dtype="bf16", style_heads_eval_dtype="bf16", encoder_neck_eval_dtype="bf16")


def test_option_defaults_and_constructor_refusals():
    assert _enc().eval_neck_dtype == torch.float32 and _enc(encoder_neck_eval_dtype="fp32").eval_neck_dtype == torch.float32
    e = _enc(**ALL16)
    assert e.eval_neck_dtype == torch.bfloat16
    assert e.eval()._neck_bf16() and not e.train()._neck_bf16()  # inference only: training mode is the fp32 path
    plain = _enc()
    assert list(e.state_dict()) == list(plain.state_dict()) and all(torch.equal(v, plain.state_dict()[k]) for k, v in e.state_dict().items())
    with pytest.raises(FmiError, match="encoder_neck_eval_dtype"):
        _enc(encoder_neck_eval_dtype="fp16")
    for missing in ("encoder_eval_dtype", "style_heads_eval_dtype"):
        opt = {k: v for k, v in ALL16.items() if k != missing}
        for kw in (opt, dict(opt, **{missing: "fp32"})):
            with pytest.raises(FmiError) as info:
                _enc(**kw)
            assert "encoder_eval_dtype" in str(info.value) and "style_heads_eval_dtype" in str(info.value), str(info.value)


def test_forward_refusals_come_before_any_library_call(monkeypatch):
    from face_mask_inpaint_amd import functional as FF

    def reached(*a, **k):
        raise AssertionError("a refused forward reached the library")

    monkeypatch.setattr(FF, "_L", reached)
    monkeypatch.setattr(_lib, "lib", reached)
    x, m = torch.zeros(1, 3, 256, 256), torch.zeros(1, 256, 256)
    e = _enc(**ALL16).eval()
    with pytest.raises(FmiError, match="inference only"):  # grad mode is on
        e(x, ref=x, mask=m)
    with pytest.raises(FmiError, match="inference only"):
        e(x)
    with torch.no_grad():
        with pytest.raises(FmiError, match="multiple of 64"):
            _enc(widths=(64, 64, 96, 128, 128), **ALL16).eval()(x, ref=x, mask=m)
        for hw in ((64, 64), (128, 128), (256, 192)):  # 16 / 64, 64 / 256, 192 / 768 tokens at the two attentions
            xs = torch.zeros(1, 3, *hw)
            with pytest.raises(FmiError, match="multiple of 128"):
                e(xs, ref=xs, mask=torch.zeros(1, *hw))
        with pytest.raises(AssertionError, match="reached the library"):  # nothing left to refuse: the call goes on
            e(x, ref=x, mask=m)


def test_example_guided_attention_accepts_out_conv_on_bf16():
    from face_mask_inpaint_amd.modules.example_guided_att import ExampleGuidedAttention

    assert ExampleGuidedAttention(256, out_channels=256).bf16_unfit() is None
    assert ExampleGuidedAttention(512, out_channels=512).bf16_unfit() is None
    assert ExampleGuidedAttention(128).bf16_unfit() is None
    assert "(24, 96)" in ExampleGuidedAttention(96).bf16_unfit()
    assert "multiple of 64" in ExampleGuidedAttention(128, out_channels=96).bf16_unfit()


# ---- the float64 restatements of the GPU tests against the oracle and the reference's fixtures -----------------------------------------
def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def test_guided64_is_the_references_module_with_out_conv(golden):
    import test_gpu_psp_neck_bf16 as G
    from oracle import picnet_cpu as O

    fx = golden("picnet_ops.pt")["ex_guided_att_out"]
    P = {"b." + k: v.double() for k, v in fx["sd0"].items()}
    m, s, r = (t.double() for t in fx["inputs"])
    wq, wo = P["b.conv.weight"].reshape(4, 16), P["b.out_conv.weight"].reshape(16, 32)
    out, _ = G.guided64(wq, wo, P["b.out_conv.bias"], m[:, 0], _nhwc(s), _nhwc(r), G._id)
    torch.testing.assert_close(_nchw(out), fx["out"].double(), rtol=1e-5, atol=1e-6)  # the fixture is the reference's fp32 evaluation
    torch.testing.assert_close(_nchw(out), O.example_guided_attention(P, "b", m, s, r), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("form", ["out_eval", "out_eval_noref", "out_eval_noatt"])
def test_stem64_and_neck64_are_the_references_encoder(golden, form):
    """the oracle's body between the restated stem and the restated neck, the oracle's heads behind it: the codes of the reference's own
    eval-mode encoder in its three forward forms"""
    import test_gpu_psp_neck_bf16 as G
    from oracle import psp_cpu as PO

    fx = golden("psp_ops.pt")["encoder"]
    P = {k: (v.double() if v.is_floating_point() else v) for k, v in {**fx["sd"], **fx["stats_after"]}.items()}
    strides = PO.body_strides(50)

    def fold(pre):
        scale = P[pre + ".weight"] / torch.sqrt(P[pre + ".running_var"] + 1e-5)
        return scale, P[pre + ".bias"] - P[pre + ".running_mean"] * scale

    def taps(img):
        a, z, _ = G.stem64(_nhwc(img.double()), P["input_layer.0.weight"], *fold("input_layer.1"), P["input_layer.2.weight"], *fold("body.0.res_layer.0"))
        torch.testing.assert_close(_nchw(z), PO.batch_norm(P, "body.0.res_layer.0", _nchw(a), False), rtol=1e-12, atol=1e-12)
        x, out = _nchw(a), []
        for i, s in enumerate(strides):
            x = PO.bottleneck(P, "body.%d" % i, x, s, False)
            if i in (6, 20, 23):
                out.append(_nhwc(x))
        return out

    w2 = lambda k: P[k].reshape(P[k].shape[0], P[k].shape[1])
    W = {"l1w": w2("latlayer1.weight"), "l1b": P["latlayer1.bias"], "l2w": w2("latlayer2.weight"), "l2b": P["latlayer2.bias"]}
    for a in ("attention1", "attention2"):
        W["a" + a[-1] + "q"], W["a" + a[-1] + "o"], W["a" + a[-1] + "b"] = w2(a + ".conv.weight"), w2(a + ".out_conv.weight"), P[a + ".out_conv.bias"]
    with torch.no_grad():
        c1, c2, c3 = taps(fx["x"])
        if form == "out_eval_noref":
            maps, _, _ = G.neck64(W, c1, c2, c3, None, None, None, None, False, G._id)
        else:
            r1, r2, r3 = taps(fx["ref"])
            m = fx["mask"].double().unsqueeze(1)
            masks = [F.interpolate(m, size=t.shape[1:3], mode="bilinear", align_corners=True)[:, 0] for t in (r3, r2, r1)]
            maps, _, _ = G.neck64(W, c1, c2, c3, r1, r2, r3, masks, form == "out_eval", G._id)
        oc = P["styles.0.linear.weight"].shape[0]
        level = lambda j: 0 if j < 3 else (1 if j < 7 else 2)
        codes = torch.stack([PO.gradual_style_block(P, "styles.%d" % j, _nchw(maps[level(j)]), oc) for j in range(fx["n_styles"])], dim=1)
    torch.testing.assert_close(codes, fx[form].double(), rtol=1e-4, atol=1e-5)
