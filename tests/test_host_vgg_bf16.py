"""Host side of the bf16 VGG16 trunk of VGGLoss: the float64 reference of tests/vgg_reference.py against CPU autograd, the input condition
of the GPU cases, the plumbing of the argument and of FMI_VGG_DTYPE, the refusals (which happen before any device call and so run
without a GPU) and the exported symbols."""
import copy
import ctypes

import pytest
import torch

import vgg_reference as VR
from face_mask_inpaint_amd import _lib
from face_mask_inpaint_amd import functional as FF
from face_mask_inpaint_amd._lib import FmiError
from face_mask_inpaint_amd.modules.loss import GANOptimizer, VGGLoss

NEW = ["fmi_conv2d_dgrad_relu_bf16", "fmi_vgg_tap_fwd_bf16", "fmi_vgg_tap_bwd_bf16", "fmi_conv2d_thin_input_dgrad_bf16"]
BF = torch.bfloat16


def _convs(v):
    return [m for bl in v.blocks for m in bl if isinstance(m, torch.nn.Conv2d)]


def _module(seed, **kw):
    torch.manual_seed(seed)
    return VGGLoss(**kw)


@pytest.mark.parametrize("rounded", [False, True], ids=["float64", "bf16-hook"])
def test_reference_agrees_with_cpu_autograd(rounded):
    """the module's own nn.Sequential blocks in double, a linear functional of the taps: taps and image gradient.  The hook rounds inside
    the chain, which autograd cannot restate: with it on, the taps are bf16 values and differ from the float64 ones by bf16-sized amounts,
    no more, and the image gradient stays close."""
    v = _module(5, width_div=8)
    n, h, w, seed = 2, 16, 24, 7
    x, gtaps = VR.trunk_inputs(n, h, w, seed, channels=(8, 16, 32, 64))
    convs = _convs(v)
    ws, bs = [c.weight.detach() for c in convs], [c.bias.detach() for c in convs]
    blocks = copy.deepcopy(v.blocks).double()
    xi = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    hmap, taps = xi, []
    for bl in blocks:
        hmap = bl(hmap)
        taps.append(hmap)
    sum((t * g.double().permute(0, 3, 1, 2)).sum() for t, g in zip(taps, gtaps)).backward()
    ref = VR.trunk(x, ws, bs, gtaps)
    for t, r in zip(taps, ref.taps):
        assert torch.allclose(t.detach().permute(0, 2, 3, 1), r, rtol=1e-12, atol=1e-14)
    gx = xi.grad.permute(0, 2, 3, 1)
    assert float((ref.gx - gx).norm() / gx.norm()) < 1e-12
    assert len(ref.acts) == 10
    if rounded:
        emu = VR.trunk(x, ws, bs, gtaps, rnd=VR.rnd_bf16)
        for i, (e, r) in enumerate(zip(emu.taps, ref.taps)):
            rel = float((e - r).norm() / r.norm())
            assert 0 < rel < 10 * 2.0 ** -8, (i, rel)
            assert torch.equal(e, VR.rnd_bf16(e)), "an emulated tap is a bf16 value"
        rel = float((emu.gx - ref.gx).norm() / ref.gx.norm())
        assert 0 < rel < 0.1, rel


@pytest.mark.parametrize("case", VR.TRUNK_CASES, ids=lambda c: "%dx%dx%d" % c[:3])
def test_gpu_cases_exercise_every_mask(case):
    """default-initialised full-width weights on N(0, 1) images: every one of the ten ReLU outputs has 30 % .. 70 % positive entries"""
    n, h, w, seed = case
    v = _module(seed)
    x, _ = VR.trunk_inputs(n, h, w, seed)
    convs = _convs(v)
    out = VR.trunk(x, [c.weight.detach() for c in convs], [c.bias.detach() for c in convs], rnd=VR.rnd_bf16)
    frac = [float((a > 0).double().mean()) for a in out.acts]
    print("positive fractions:", " ".join(f"{f:.3f}" for f in frac))
    assert len(frac) == 10 and all(0.3 <= f <= 0.7 for f in frac), frac


def test_argument_and_environment(monkeypatch):
    monkeypatch.delenv("FMI_VGG_DTYPE", raising=False)
    assert VGGLoss(width_div=8).feature_dtype == torch.float32
    assert VGGLoss(feature_dtype=BF).feature_dtype == BF
    assert VGGLoss(width_div=8, feature_dtype=torch.float32).feature_dtype == torch.float32
    with pytest.raises(FmiError, match="feature_dtype"):
        VGGLoss(feature_dtype=torch.float16)
    monkeypatch.setenv("FMI_VGG_DTYPE", "bf16")
    assert VGGLoss().feature_dtype == BF
    assert GANOptimizer(None, None).vgg_loss.feature_dtype == BF
    assert VGGLoss(width_div=8, feature_dtype=torch.float32).feature_dtype == torch.float32, "the argument wins"
    assert GANOptimizer(None, None, vgg_width_div=8, vgg_dtype=torch.float32).vgg_loss.feature_dtype == torch.float32
    monkeypatch.setenv("FMI_VGG_DTYPE", "fp32")
    assert VGGLoss(width_div=8).feature_dtype == torch.float32
    assert GANOptimizer(None, None, vgg_dtype=BF).vgg_loss.feature_dtype == BF
    monkeypatch.setenv("FMI_VGG_DTYPE", "half")
    with pytest.raises(FmiError, match="FMI_VGG_DTYPE"):
        VGGLoss()
    with pytest.raises(FmiError, match="FMI_VGG_DTYPE"):
        GANOptimizer(None, None)
    assert VGGLoss(feature_dtype=BF).feature_dtype == BF, "the argument wins: the variable is not read"


def test_state_dict_is_the_fp32_one():
    a, b = VGGLoss(), VGGLoss(feature_dtype=BF)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(sa[k].shape == sb[k].shape and sb[k].dtype == torch.float32 for k in sa)
    a.load_state_dict(sb, strict=True)


def test_refusals_come_before_any_device_call(monkeypatch):
    """the widths at construction, naming the layer; the extent at the first forward, naming it -- with every library entry replaced by a
    trap, on CPU tensors"""
    with pytest.raises(FmiError, match=r"convolution 0 is 3 -> 8"):
        VGGLoss(width_div=8, feature_dtype=BF)
    with pytest.raises(FmiError, match=r"convolution 0 is 3 -> 32"):
        VGGLoss(width_div=2, feature_dtype=BF)
    with pytest.raises(FmiError, match=r"convolution 2 is 64 -> 96"):  # a later layer is named by its own index
        FF.vgg_trunk_check_widths([(3, 64, 3, 3), (64, 64, 3, 3), (64, 96, 3, 3)])
    monkeypatch.setenv("FMI_VGG_DTYPE", "bf16")
    with pytest.raises(FmiError, match="convolution 0"):
        GANOptimizer(None, None, vgg_width_div=8)
    monkeypatch.delenv("FMI_VGG_DTYPE")

    def trap(*a, **k):
        raise AssertionError("a library call before the refusal")

    monkeypatch.setattr(_lib, "lib", trap)
    monkeypatch.setattr(FF, "_L", trap)
    v = VGGLoss(feature_dtype=BF)
    for h, w in ((36, 32), (32, 44), (30, 30)):
        x, y = torch.zeros(1, h, w, 3), torch.zeros(1, h, w, 3)
        with pytest.raises(FmiError, match=f"multiples of 8, got {h} x {w}"):
            v.forward_multi_prepared(x, y, ["perceptual"])
        img = torch.zeros(1, 3, h, w)
        with pytest.raises(FmiError, match=f"multiples of 8, got {h} x {w}"):
            v(img, img)
        with pytest.raises(FmiError, match=f"multiples of 8, got {h} x {w}"):
            v.forward_multi([(img, img, "style")])
    with pytest.raises(FmiError, match="multiples of 8, got 36 x 32"):
        FF.vgg_trunk_bf16(torch.zeros(1, 36, 32, 3), [None] * 10)


@pytest.fixture(scope="module")
def clib():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        fn = getattr(lib, name)  # AttributeError: the built library lacks the symbol
        fn.argtypes = _lib.SIGNATURES[name]
        fn.restype = ctypes.c_int
    return lib


def test_new_symbols_are_exported_and_bound(clib):
    assert all(name in _lib.SIGNATURES for name in NEW)
    assert not _lib.Library(_lib.LIB_PATH, strict=True).missing
    header = open(_lib.LIB_PATH.rsplit("/face_mask_inpaint_amd/", 1)[0] + "/include/fmi_hip.h").read()
    assert all(f"int {name}(" in header for name in NEW)
