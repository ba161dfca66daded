"""GPU: the stride-1 ResBlock pair in one launch -- y = act(conv3x3(x1, W1) + conv1x1(x2, W2) + b1 + b2) (fmi_conv2d_pair_fwd_f32) and dW1,
dW2 and the bias gradient from one walk over dy (fmi_conv2d_pair_wgrad_f32), csrc/conv_pair.h -- against the float64 reference with CPU
autograd (tests/resblock_pair_reference.py), against the two launches they replace, and for bit-reproducibility; then ResBlock modules on
the fused route against the same modules forced through the two-launch route.

Tolerances are the ones this project uses for these products: outputs rtol 1e-4 / atol 1e-5; weight and bias gradients rtol 1e-4 / atol
1e-4 * max(1, sqrt(N * H * W / 2048)) (dw_tol of tests/test_gpu_thin_paths.py); against the two-launch composition 1e-5 of the largest
entry (only the summation order differs)."""
import copy
import ctypes as C
import functools

import pytest
import torch
from torch import nn

import resblock_pair_reference as R

pytestmark = pytest.mark.gpu
OK, BAD_ARG, UNSUPPORTED = 0, 1, 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def FF():
    from face_mask_inpaint_amd import functional

    return functional


@functools.lru_cache(maxsize=None)
def case(shape, bias):
    """inputs and float64 reference of one shape, computed once and shared"""
    x1, x2, w1, w2, b1, b2, gy = R.make(*shape)
    if not bias:
        b1 = b2 = None
    return (x1, x2, w1, w2, b1, b2, gy), R.reference(x1, x2, w1, w2, b1, b2, gy)


class OnDevice:
    def __init__(self, FF, dev, shape, bias):
        (x1, x2, w1, w2, b1, b2, gy), self.ref = case(shape, bias)
        self.n, self.h, self.w, self.c1, self.c2, self.k = shape
        to = lambda t: None if t is None else t.to(dev)
        self.x1, self.x2, self.b1, self.b2, self.gy = to(x1), to(x2), to(b1), to(b2), to(gy)
        self.pw1, self.pw2 = FF.prepare_weights([(w1.to(dev), None, None), (w2.to(dev), None, None)])
        self.FF = FF

    def desc(self, pieces):
        d, _, _ = self.FF.conv_desc(self.n, self.h, self.w, self.c1, self.k, 3, 3, 1, 1, w3=self.pw1.w3[0] if pieces else None)
        return d

    def fwd(self, lib, act=0, pieces=True):
        FF = self.FF
        y = torch.full((self.n, self.h, self.w, self.k), float("nan"), device=self.x1.device)
        d = self.desc(pieces)
        w3b = C.c_void_p(self.pw2.w3[0].data_ptr()) if pieces else None
        lib.conv2d_pair_fwd_f32(C.byref(d), FF._p(self.x1), FF._p(self.x2), self.c2, FF._p(self.pw1.wf), FF._p(self.pw2.wf), w3b, FF._p(self.b1),
                                FF._p(self.b2), FF._p(y), act, FF._st())
        torch.cuda.synchronize()
        return y

    def fwd_two_launches(self, lib, act=0):
        FF = self.FF
        s = torch.empty((self.n, self.h, self.w, self.k), device=self.x1.device)
        y = torch.empty_like(s)
        d2, _, _ = FF.conv_desc(self.n, self.h, self.w, self.c2, self.k, 1, 1, 1, 0, w3=self.pw2.w3[0])
        lib.conv2d_fwd_f32(C.byref(d2), FF._p(self.x2), FF._p(self.pw2.wf), FF._p(self.b2), None, FF._p(s), 0, 1, 0, FF._st())
        lib.conv2d_fwd_f32(C.byref(self.desc(True)), FF._p(self.x1), FF._p(self.pw1.wf), FF._p(self.b1), FF._p(s), FF._p(y), act, 1, 0, FF._st())
        torch.cuda.synchronize()
        return y

    def wgrad(self, lib):
        FF = self.FF
        dev = self.x1.device
        g1, g2 = torch.zeros(9, self.c1, self.k, device=dev), torch.zeros(1, self.c2, self.k, device=dev)
        gb = torch.zeros(self.k, device=dev) if self.b1 is not None else None
        lib.conv2d_pair_wgrad_f32(C.byref(self.desc(False)), FF._p(self.x1), FF._p(self.x2), self.c2, FF._p(self.gy), FF._p(g1), FF._p(g2), FF._p(gb), FF._st())
        torch.cuda.synchronize()
        return g1, g2, gb

    def wgrad_two_launches(self, lib):
        FF = self.FF
        dev = self.x1.device
        g1, g2 = torch.zeros(9, self.c1, self.k, device=dev), torch.zeros(1, self.c2, self.k, device=dev)
        gb = torch.zeros(self.k, device=dev)
        d2, _, _ = FF.conv_desc(self.n, self.h, self.w, self.c2, self.k, 1, 1, 1, 0)
        lib.conv2d_wgrad_f32(C.byref(self.desc(False)), FF._p(self.x1), FF._p(self.gy), FF._p(g1), FF._p(gb), 1, 0, FF._st())
        lib.conv2d_wgrad_f32(C.byref(d2), FF._p(self.x2), FF._p(self.gy), FF._p(g2), None, 1, 0, FF._st())
        torch.cuda.synchronize()
        return g1, g2, gb


def lib_():
    from face_mask_inpaint_amd import _lib

    return _lib.lib()


class det_mode:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = lib_().get_deterministic()
        lib_().set_deterministic(1 if self.on else 0)

    def __exit__(self, *exc):
        lib_().set_deterministic(self.old)
        return False


def close_to_largest(a, b, what, scale=None):
    big = float((b if scale is None else scale).abs().max())
    err = float((a - b).abs().max())
    print(f"{what}: max|diff| {err:.3g}, largest entry {big:.3g}, bound {1e-5 * big:.3g}")
    assert err <= 1e-5 * big, what


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("pieces", [True, False])
def test_forward(FF, dev, shape, bias, pieces):
    lib = lib_()
    t = OnDevice(FF, dev, shape, bias)
    y64 = t.ref[0]
    assert lib.conv2d_pair_supported(C.byref(t.desc(pieces)), t.c2) == 1
    with det_mode(False):
        for act in (FF.ACT_NONE, FF.ACT_RELU):  # the fused activation the entry exposes
            y = t.fwd(lib, act, pieces)
            want = y64.clamp_min(0) if act else y64
            print(f"{shape} bias {bias} pieces {pieces} act {act}: max|err| {float((y.cpu().double() - want).abs().max()):.3g}")
            torch.testing.assert_close(y.cpu().double(), want, rtol=1e-4, atol=1e-5)
            close_to_largest(y, t.fwd_two_launches(lib, act), "fused forward against conv1x1 then conv3x3 + residual")
    with det_mode(True):
        assert lib.conv2d_pair_ksplit(C.byref(t.desc(pieces)), t.c2, 0) == 1
        ya, yb = t.fwd(lib, 0, pieces), t.fwd(lib, 0, pieces)
        assert torch.equal(ya, yb), "reproducible mode: two runs must agree bit for bit"
        torch.testing.assert_close(ya.cpu().double(), y64, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("pieces", [True, False])
def test_split_reduction_branch_is_taken(FF, dev, pieces):
    """K = 640 over 2 tiles: the plan query must say the reduction really is split (y starts as b1 + b2, partial sums meet in it); an
    activation or the reproducible mode keeps it whole"""
    lib = lib_()
    t = OnDevice(FF, dev, R.SPLIT_SHAPE, True)
    d = t.desc(pieces)
    with det_mode(False):
        assert lib.conv2d_pair_ksplit(C.byref(d), t.c2, 0) == 2
        assert lib.conv2d_pair_ksplit(C.byref(d), t.c2, FF.ACT_RELU) == 1
        torch.testing.assert_close(t.fwd(lib, 0, pieces).cpu().double(), t.ref[0], rtol=1e-4, atol=1e-5)
    with det_mode(True):
        assert lib.conv2d_pair_ksplit(C.byref(d), t.c2, 0) == 1
    unsplit = [s for s in R.SHAPES if s != R.SPLIT_SHAPE and s[0] * s[1] * s[2] > 128 and 9 * s[3] + s[4] < 512]
    for s in unsplit:
        d2, _, _ = FF.conv_desc(s[0], s[1], s[2], s[3], s[5], 3, 3, 1, 1)
        assert lib.conv2d_pair_ksplit(C.byref(d2), s[4], 0) == 1


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_weight_gradient(FF, dev, shape, bias):
    lib = lib_()
    t = OnDevice(FF, dev, shape, bias)
    _, dw1, dw2, db, _, _ = t.ref
    tol = R.dw_tol(t.n, t.h, t.w)

    def check(g1, g2, gb):
        print(f"{shape} bias {bias}: max|err| dW1 {float((g1.cpu().double() - dw1).abs().max()):.3g} dW2 {float((g2.cpu().double() - dw2).abs().max()):.3g}"
              + (f" dbias {float((gb.cpu().double() - db).abs().max()):.3g}" if gb is not None else "") + f" (atol {tol:.3g})")
        torch.testing.assert_close(g1.cpu().double(), dw1, rtol=1e-4, atol=tol)
        torch.testing.assert_close(g2.cpu().double(), dw2, rtol=1e-4, atol=tol)
        if bias:
            torch.testing.assert_close(gb.cpu().double(), db, rtol=1e-4, atol=tol)
        else:
            assert gb is None

    with det_mode(False):
        g1, g2, gb = t.wgrad(lib)
        check(g1, g2, gb)
        r1, r2, rb = t.wgrad_two_launches(lib)
        close_to_largest(g1, r1, "fused dW1 against the single weight gradient")
        close_to_largest(g2, r2, "fused dW2 against the single weight gradient")
        if bias:
            close_to_largest(gb, rb, "fused bias gradient against the single weight gradient's ones row")
    with det_mode(True):
        a, b = t.wgrad(lib), t.wgrad(lib)
        for u, v in zip(a, b):
            assert (u is None and v is None) or torch.equal(u, v), "reproducible mode: two runs must agree bit for bit"
        check(*a)


def test_refusals_before_any_launch(FF, dev):
    lib = lib_().cdll  # raw status codes
    t = OnDevice(FF, dev, (1, 3, 5, 64, 16, 64), True)
    y = torch.full((t.n, t.h, t.w, t.k), 7.0, device=dev)
    g1, g2 = torch.zeros(9, t.c1, t.k, device=dev), torch.zeros(1, t.c2, t.k, device=dev)
    P = lambda x, off=0: C.c_void_p(x.data_ptr() + off)

    def fwd(d, c2, x2=None, yy=None):
        return lib.fmi_conv2d_pair_fwd_f32(C.byref(d), P(t.x1), x2 or P(t.x2), c2, P(t.pw1.wf), P(t.pw2.wf), None, P(t.b1), P(t.b2), yy or P(y), 0, FF._st())

    def wgrad(d, c2, x2=None):
        return lib.fmi_conv2d_pair_wgrad_f32(C.byref(d), P(t.x1), x2 or P(t.x2), c2, P(t.gy), P(g1), P(g2), None, FF._st())

    mk = lambda **kw: FF.conv_desc(t.n, t.h, t.w, t.c1, t.k, 3, 3, kw.get("stride", 1), 1, kw.get("pad_mode", 0))[0]
    for d, c2 in ((mk(stride=2), t.c2), (mk(pad_mode=1), t.c2), (mk(), 8), (mk(), 24)):
        assert lib.fmi_conv2d_pair_supported(C.byref(d), c2) == 0 and lib.fmi_conv2d_pair_routed(C.byref(d), c2) == 0
        assert fwd(d, c2) == UNSUPPORTED and wgrad(d, c2) == UNSUPPORTED
    assert fwd(mk(), t.c2, x2=P(t.x2, 4)) == BAD_ARG and fwd(mk(), t.c2, yy=P(y, 8)) == BAD_ARG and wgrad(mk(), t.c2, x2=P(t.x2, 4)) == BAD_ARG
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and not bool(g1.any()) and not bool(g2.any()), "a refused call launched"
    assert fwd(mk(), t.c2) == OK
    torch.cuda.synchronize()
    torch.testing.assert_close(y.cpu().double(), t.ref[0], rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------------------------------
# module level: ResBlock on the fused route against the same block forced through the two launches
# ---------------------------------------------------------------------------------------------------
def run_block(FF, blk, x, gy, fused):
    """forward + backward of a copy of blk; returns (out, input gradient, parameter gradients by name, SpectralNorm u / v after the
    forward, the profile tags of the launches)"""
    from face_mask_inpaint_amd.modules.pluralistic_model import base_function as B

    blk = copy.deepcopy(blk)
    x = x.clone().requires_grad_(True)
    old, FF.PAIR_ENABLED, FF.PROFILE = FF.PAIR_ENABLED, fused, []
    try:
        out = blk.nhwc(x)
        uv = {k: v.detach().clone() for k, v in blk.named_parameters() if k.endswith("weight_u") or k.endswith("weight_v")}
        out.backward(gy)
        torch.cuda.synchronize()
        tags = [p[0] for p in FF.PROFILE]
    finally:
        FF.PAIR_ENABLED, FF.PROFILE = old, None
    assert isinstance(blk, B.ResBlock)
    return out.detach(), x.grad, {k: p.grad for k, p in blk.named_parameters() if p.requires_grad}, uv, tags


@pytest.mark.parametrize("form", ["none", "none+spectral", "none+down", "none+spectral+down", "instance", "instance+spectral"])
def test_resblock_fused_route_against_two_launch_route(FF, dev, form):
    from face_mask_inpaint_amd.modules.pluralistic_model.base_function import ResBlock

    torch.manual_seed(11)
    norm = functools.partial(nn.InstanceNorm2d, affine=True) if form.startswith("instance") else None
    blk = ResBlock(64, 64, 64, norm, nn.LeakyReLU(0.1), "down" if "down" in form else "none", "spectral" in form).to(dev)
    with torch.no_grad():
        for name, p in blk.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.5)
            elif norm is not None and name in ("model.0.weight", "model.3.weight"):  # the InstanceNorm scales
                p.copy_(1.0 + torch.randn_like(p) * 0.5)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 8, 8, 64, generator=g).to(dev)
    ho = 4 if "down" in form else 8
    gy = torch.randn(2, ho, ho, 64, generator=g).to(dev)
    with det_mode(False):
        out_f, gx_f, gp_f, uv_f, tags_f = run_block(FF, blk, x, gy, True)
        out_u, gx_u, gp_u, uv_u, tags_u = run_block(FF, blk, x, gy, False)
    assert any("+1x1 64" in t and t.startswith("conv_fwd|") for t in tags_f) and any("+1x1 64" in t and t.startswith("conv_wgrad|") for t in tags_f)
    assert not any("+1x1" in t for t in tags_u) and sum("k1s1" in t and t.startswith("conv_fwd|") for t in tags_u) == 1
    assert not any(t.startswith("conv_fwd|") and "k1s1" in t for t in tags_f), "the routed 1x1 forward launch must be gone"
    close_to_largest(out_f, out_u, "output")
    close_to_largest(gx_f, gx_u, "input gradient")
    assert gp_f.keys() == gp_u.keys() and len(gp_f) >= 6
    for k in gp_f:
        scale = None
        if norm is not None and k in ("conv1.bias", "conv1.module.bias"):
            # InstanceNorm removes the per-channel mean of conv1's output, so this gradient is exactly zero in exact arithmetic and both
            # routes return only the rounding of sum_pixels g (measured ~1e-6): "the largest entry" of such a tensor says nothing.  The
            # same g, summed over the same pixels with activations of order one as weights, is conv1's weight gradient: its largest
            # entry is the scale the 1e-5 rule is applied with here.
            scale = gp_u[k[:-4] + ("weight_bar" if "module" in k else "weight")]
        close_to_largest(gp_f[k], gp_u[k], "gradient of " + k, scale)
    assert uv_f.keys() == uv_u.keys() and len(uv_f) == (6 if "spectral" in form else 0)
    for k in uv_f:
        assert torch.equal(uv_f[k], uv_u[k]), k + " must advance exactly as on the two-launch route"
        assert not torch.equal(uv_f[k], dict(blk.named_parameters())[k]), k + " must advance once per forward"


def test_resblock_mixed_route(FF, dev):
    """8 x 32^2 128 -> 128: the forward tied with the two launches in the measurement and keeps them, the weight gradient is fused
    (fmi_conv2d_pair_routed says 2); same results as the two-launch route"""
    from face_mask_inpaint_amd.modules.pluralistic_model.base_function import ResBlock

    d, _, _ = FF.conv_desc(8, 32, 32, 128, 128, 3, 3, 1, 1)
    assert lib_().conv2d_pair_routed(C.byref(d), 128) == 2
    torch.manual_seed(12)
    blk = ResBlock(128, 128, 128, None, nn.LeakyReLU(0.1), "none", False).to(dev)
    g = torch.Generator().manual_seed(6)
    x, gy = torch.randn(8, 32, 32, 128, generator=g).to(dev), torch.randn(8, 32, 32, 128, generator=g).to(dev)
    with det_mode(False):
        out_f, gx_f, gp_f, _, tags_f = run_block(FF, blk, x, gy, True)
        out_u, gx_u, gp_u, _, tags_u = run_block(FF, blk, x, gy, False)
    assert not any("+1x1" in t for t in tags_f if t.startswith("conv_fwd|")) and sum("k1s1" in t for t in tags_f if t.startswith("conv_fwd|")) == 1
    assert any("+1x1 128" in t for t in tags_f if t.startswith("conv_wgrad|")) and not any("k1s1" in t for t in tags_f if t.startswith("conv_wgrad|"))
    assert not any("+1x1" in t for t in tags_u)
    close_to_largest(out_f, out_u, "output")
    close_to_largest(gx_f, gx_u, "input gradient")
    for k in gp_f:
        close_to_largest(gp_f[k], gp_u[k], "gradient of " + k)
