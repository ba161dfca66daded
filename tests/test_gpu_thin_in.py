"""GPU: the thin-input convolution kernels (csrc/thinin.hip; C <= 4 input channels, 3x3 pad 1 or 1x1 pad 0) against float64
torch.nn.functional.conv2d / autograd on the CPU, through the dedicated entries and through the routes that lead to them."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SIZES = [(1, 1, 1), (2, 3, 5), (1, 17, 33), (2, 9, 130), (2, 80, 260)]  # the last: ragged rows, more tiles than resident workgroups
CHANNELS = [(3, 32), (3, 64), (1, 8), (4, 16)]
TAPS = [9, 1]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def FF():
    from face_mask_inpaint_amd import functional

    return functional


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def pack(w):
    k, c, kh, kw = w.shape
    return (w.permute(2, 3, 1, 0).reshape(kh * kw, c, k).contiguous(), w.permute(2, 3, 0, 1).reshape(kh * kw, k, c).contiguous())


_CASES = {}


def case(n, h, w, c, k, taps):
    """fp32 operands of one geometry and their float64 results (computed once, shared by the tests, never modified)"""
    key = (n, h, w, c, k, taps)
    if key not in _CASES:
        ks = 3 if taps == 9 else 1
        g = torch.Generator().manual_seed(1000 * h + 10 * w + c + k + taps)
        x = torch.randn(n, c, h, w, generator=g)
        wt_ = torch.randn(k, c, ks, ks, generator=g) / (c * taps) ** 0.5
        b = torch.randn(k, generator=g)
        res = torch.randn(n, k, h, w, generator=g)
        gy = torch.randn(n, k, h, w, generator=g)
        x64, w64, b64 = x.double(), wt_.double().requires_grad_(True), b.double().requires_grad_(True)
        pre = F.conv2d(x64, w64, b64, padding=ks // 2)
        pre.backward(gy.double())
        mag = F.conv2d(x64.abs(), w64.detach().abs(), None, padding=ks // 2)  # sum |x| |w| per output value
        _CASES[key] = dict(ks=ks, x=x, w=wt_, b=b, res=res, gy=gy, conv64=(pre.detach() - b64.detach().view(1, k, 1, 1)), mag=mag,
                           gw64=w64.grad.clone(), gb64=b64.grad.clone())
    return _CASES[key]


def act64(v, act):
    return torch.tanh(v) if act == 1 else (torch.relu(v) if act == 2 else v)


@pytest.mark.parametrize("taps", TAPS)
@pytest.mark.parametrize("c,k", CHANNELS)
@pytest.mark.parametrize("n,h,w", SIZES)
def test_thin_in_forward(dev, FF, n, h, w, c, k, taps):
    """y = act(conv + bias + residual): |err| <= (taps*C + 3) 2^-24 (sum |x||w| + |bias| + |residual|) + 1e-30 before the activation (one
    rounding per FMA of the chain, the two additions and the stored value), and the activations are 1-Lipschitz"""
    from face_mask_inpaint_amd import _lib

    lib = _lib.lib()
    cs = case(n, h, w, c, k, taps)
    ks = cs["ks"]
    d, _, _ = FF.conv_desc(n, h, w, c, k, ks, ks, 1, ks // 2, 0)
    assert lib.conv2d_thin_in_supported(C.byref(d)) == 1
    xd, wf = nhwc(cs["x"]).to(dev), pack(cs["w"])[0].to(dev)
    bd, rd = cs["b"].to(dev), nhwc(cs["res"]).to(dev)
    for has_b in (False, True):
        for has_r in (False, True):
            pre = cs["conv64"] + (cs["b"].double().view(1, k, 1, 1) if has_b else 0) + (cs["res"].double() if has_r else 0)
            bound = (taps * c + 3) * 2.0 ** -24 * (cs["mag"] + (cs["b"].double().abs().view(1, k, 1, 1) if has_b else 0)
                                                    + (cs["res"].double().abs() if has_r else 0)) + 1e-30
            for act in (0, 1, 2):
                want = nhwc(act64(pre, act))
                y = torch.full((n, h, w, k), float("nan"), device=dev)
                lib.conv2d_thin_in_fwd_f32(C.byref(d), FF._p(xd), FF._p(wf), FF._p(bd if has_b else None), FF._p(rd if has_r else None), FF._p(y), act,
                                           FF._st())
                for name, got in (("entry", y),):
                    err = (got.cpu().double() - want).abs()
                    assert not torch.isnan(err).any(), f"{name}: unwritten output (bias {has_b} residual {has_r} act {act})"
                    worst = float((err / nhwc(bound)).max())
                    print(f"thin_in fwd {name} {n}x{h}x{w} {c}->{k} taps {taps} bias {has_b} res {has_r} act {act}: err / bound = {worst:.3f}")
                    assert worst <= 1.0, f"{name}: err / bound = {worst:.3f} (bias {has_b} residual {has_r} act {act})"


def _wgrad_new(lib, FF, d, xd, gyd, k, shape, dev, rows=None, want_b=True):
    nb = lib.conv2d_thin_in_wgrad_ws_bytes(C.byref(d))
    width = shape[0] * shape[1] * shape[2] + k
    assert nb > 0 and nb % (4 * width) == 0
    if rows is not None:
        nb = min(nb, rows * width * 4)
    ws = torch.empty(nb // 4, device=dev)
    gw = torch.full(shape, float("nan"), device=dev)
    gb = torch.full((k,), float("nan"), device=dev) if want_b else None
    lib.conv2d_thin_in_wgrad_f32(C.byref(d), FF._p(xd), FF._p(gyd), FF._p(gw), FF._p(gb), FF._p(ws), nb, FF._st())
    return gw, gb


@pytest.mark.parametrize("taps", TAPS)
@pytest.mark.parametrize("c,k", CHANNELS)
@pytest.mark.parametrize("n,h,w", SIZES)
def test_thin_in_wgrad_and_bias_grad(dev, FF, n, h, w, c, k, taps):
    """dW and dbias of one launch pair: against float64 (the project's bound for this quantity), against the generic weight gradient
    plus the bias-gradient pass, bit-identical from call to call and between the reproducible mode and the default one"""
    from face_mask_inpaint_amd import _lib

    lib = _lib.lib()
    cs = case(n, h, w, c, k, taps)
    ks = cs["ks"]
    d, _, _ = FF.conv_desc(n, h, w, c, k, ks, ks, 1, ks // 2, 0)
    xd, gyd = nhwc(cs["x"]).to(dev), nhwc(cs["gy"]).to(dev)
    shape = (taps, c, k)
    want_w, want_b = pack(cs["gw64"])[0], cs["gb64"]
    atol = 1e-4 * max(1.0, math.sqrt(n * h * w / 2048.0))
    gw, gb = _wgrad_new(lib, FF, d, xd, gyd, k, shape, dev)
    assert not torch.isnan(gw).any() and not torch.isnan(gb).any(), "unwritten output"
    print(f"thin_in wgrad {n}x{h}x{w} {c}->{k} taps {taps}: max |dW - dW64| = {float((gw.cpu().double() - want_w).abs().max()):.3e}, "
          f"max |db - db64| = {float((gb.cpu().double() - want_b).abs().max()):.3e}, atol {atol:.3e}")
    torch.testing.assert_close(gw.cpu().double(), want_w, rtol=1e-4, atol=atol)
    torch.testing.assert_close(gb.cpu().double(), want_b, rtol=1e-4, atol=atol)
    # without the bias gradient: the same dW
    gw_nb, _ = _wgrad_new(lib, FF, d, xd, gyd, k, shape, dev, want_b=False)
    assert torch.equal(gw_nb, gw)
    # the parent path on the same inputs
    pw, pb = torch.zeros(shape, device=dev), torch.zeros(k, device=dev)
    lib.conv2d_wgrad_f32(C.byref(d), FF._p(xd), FF._p(gyd), FF._p(pw), None, 1, 0, FF._st())
    lib.bias_grad_f32(FF._p(gyd), gyd.numel() // k, k, k, FF._p(pb), FF._st())
    dw_rel, db_rel = float((gw - pw).abs().max() / pw.abs().max()), float((gb - pb).abs().max() / pb.abs().max())
    print(f"    against the generic path: dW {dw_rel:.3e}, dbias {db_rel:.3e} of the largest entry")
    assert dw_rel <= 1e-5 and db_rel <= 1e-5
    # two calls, and the reproducible mode against the default one: the same bits
    gw2, gb2 = _wgrad_new(lib, FF, d, xd, gyd, k, shape, dev)
    assert torch.equal(gw2, gw) and torch.equal(gb2, gb)
    with FF.deterministic(True):
        gw3, gb3 = _wgrad_new(lib, FF, d, xd, gyd, k, shape, dev)
    assert torch.equal(gw3, gw) and torch.equal(gb3, gb)
    if (n, h, w) == (2, 80, 260):  # a workspace of fewer rows than workgroups only lowers the grid
        gw4, gb4 = _wgrad_new(lib, FF, d, xd, gyd, k, shape, dev, rows=3)
        torch.testing.assert_close(gw4.cpu().double(), want_w, rtol=1e-4, atol=atol)
        torch.testing.assert_close(gb4.cpu().double(), want_b, rtol=1e-4, atol=atol)


# test_thin_input_conv_adjoint's cases, the 1x1 form, the large ragged map, and -- the 3x3 streaming kernel serves maps of at least 131072
# pixels -- maps just above that: ragged segments and bands for every K/4 (segments of 64 .. 512 pixels), two rows, one row
@pytest.mark.parametrize("n,c,k,h,w,ks", [(2, 3, 64, 40, 36, 3), (1, 3, 32, 130, 200, 3), (2, 1, 16, 9, 7, 3), (1, 4, 8, 3, 3, 3), (2, 2, 4, 17, 5, 3),
                                          (2, 3, 32, 9, 130, 1), (1, 4, 8, 1, 1, 1), (2, 3, 64, 80, 260, 3), (2, 3, 32, 80, 260, 1),
                                          (1, 3, 64, 260, 505, 3), (2, 3, 32, 221, 300, 3), (1, 4, 8, 130, 1010, 3), (1, 1, 16, 2, 65536, 3),
                                          (1, 2, 8, 1, 131073, 3), (1, 3, 32, 256, 512, 1)])
def test_thin_in_input_gradient(dev, FF, n, c, k, h, w, ks):
    """input gradient of a thin-input convolution through the dedicated entry and through fmi_conv2d_dgrad_f32, against autograd in
    float64 with test_thin_input_conv_adjoint's tolerance"""
    from face_mask_inpaint_amd import _lib

    lib = _lib.lib()
    g = torch.Generator().manual_seed(h * 7 + c + k + ks)
    x = torch.randn(n, c, h, w, generator=g).double().requires_grad_(True)
    wt_ = torch.randn(k, c, ks, ks, generator=g) / (c * ks * ks) ** 0.5
    gy = torch.randn(n, k, h, w, generator=g)
    F.conv2d(x, wt_.double(), padding=ks // 2).backward(gy.double())
    d, _, _ = FF.conv_desc(n, h, w, c, k, ks, ks, 1, ks // 2, 0)
    wtp = pack(wt_)[1].to(dev)
    gh, st = nhwc(gy).to(dev), FF._st()
    for fn in (lambda dx: lib.conv2d_thin_input_dgrad_f32(C.byref(d), FF._p(gh), FF._p(wtp), FF._p(dx), st),
               lambda dx: lib.conv2d_dgrad_f32(C.byref(d), FF._p(gh), FF._p(wtp), None, None, FF._p(dx), 1, 0, st)):
        dx = torch.full((n, h, w, c), float("nan"), device=dev)
        fn(dx)
        torch.testing.assert_close(dx.cpu().double(), nhwc(x.grad), rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("n,c,k,h,w,ks,act", [(1, 3, 32, 256, 512, 3, 0), (2, 3, 64, 260, 253, 3, 1), (1, 3, 32, 512, 256, 1, 2)])
def test_thin_in_routes(dev, FF, n, c, k, h, w, ks, act):
    """maps of at least 131072 pixels through FF.conv2d and autograd: fmi_conv2d_fwd_f32, the weight-gradient dispatch of
    _Conv2d.backward and fmi_conv2d_dgrad_f32 all lead to the thin-input kernels; the forward within its derived bound, the gradients
    within the bounds of the tests above.  Of the 1x1 form only the weight gradient is routed there: its forward and input gradient
    stay on the generic kernels and are not this file's subject"""
    from face_mask_inpaint_amd import _lib
    from face_mask_inpaint_amd.functional import PackedWeight

    d, _, _ = FF.conv_desc(n, h, w, c, k, ks, ks, 1, ks // 2, 0)
    assert _lib.lib().conv2d_thin_in_routed(C.byref(d)) == 1
    taps = ks * ks
    g = torch.Generator().manual_seed(h + w + k)
    x, b = torch.randn(n, c, h, w, generator=g), torch.randn(k, generator=g)
    wt_ = torch.randn(k, c, ks, ks, generator=g) / (c * taps) ** 0.5
    res, gy = torch.randn(n, k, h, w, generator=g), torch.randn(n, k, h, w, generator=g)
    x64, w64, b64 = x.double().requires_grad_(True), wt_.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = F.conv2d(x64, w64, b64, padding=ks // 2) + res.double()
    y64 = act64(pre, act)
    y64.backward(gy.double())
    bound = (taps * c + 3) * 2.0 ** -24 * (F.conv2d(x.double().abs(), wt_.double().abs(), None, padding=ks // 2) + b.double().abs().view(1, k, 1, 1)
                                           + res.double().abs()) + 1e-30
    wf, wtp = [t.to(dev) for t in pack(wt_)]
    wf.requires_grad_(True)
    xd, bd = nhwc(x).to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    y = FF.conv2d(xd, PackedWeight(wf, wtp, k, c, ks, ks), bd, nhwc(res).to(dev), 1, ks // 2, 0, act)
    worst = float(((y.detach().cpu().double() - nhwc(y64.detach())).abs() / nhwc(bound)).max())
    print(f"thin_in route fwd {n}x{h}x{w} {c}->{k} k{ks} act {act}: err / bound = {worst:.3f}")
    assert ks == 1 or worst <= 1.0
    y.backward(nhwc(gy).to(dev))
    atol = 1e-4 * max(1.0, math.sqrt(n * h * w / 2048.0))
    torch.testing.assert_close(wf.grad.cpu().double(), pack(w64.grad)[0], rtol=1e-4, atol=atol)
    torch.testing.assert_close(bd.grad.cpu().double(), b64.grad, rtol=1e-4, atol=atol)
    if ks == 3:
        torch.testing.assert_close(xd.grad.cpu().double(), nhwc(x64.grad), rtol=1e-5, atol=2e-5)


def test_thin_in_encoder_block_end_to_end(dev, FF):
    """ResBlockEncoderOptimized(3, 32) at 2 x 32 x 40, forward and backward through the module with the input requiring a gradient, against
    the same block evaluated in float64; the tolerances test_blocks_against_reference_golden uses for this block"""
    from torch import nn

    from face_mask_inpaint_amd.modules.pluralistic_model import base_function as bf

    torch.manual_seed(5)
    blk = bf.ResBlockEncoderOptimized(3, 32, None, nn.LeakyReLU(0.1), False, False)
    c1, c2, cb = bf._conv(blk.conv1), bf._conv(blk.conv2), bf._conv(blk.bypass)
    x = torch.randn(2, 3, 32, 40)
    gout = torch.randn(2, 32, 16, 20)
    p64 = [p.detach().double().requires_grad_(True) for p in (c1.weight, c1.bias, c2.weight, c2.bias, cb.weight, cb.bias)]
    x64 = x.double().requires_grad_(True)
    y64 = F.avg_pool2d(F.conv2d(F.leaky_relu(F.conv2d(x64, p64[0], p64[1], padding=1), 0.1), p64[2], p64[3], padding=1), 2) + \
        F.conv2d(F.avg_pool2d(x64, 2), p64[4], p64[5])
    y64.backward(gout.double())
    blk = blk.to(dev)
    xd = x.to(dev).requires_grad_(True)
    y = blk(xd)
    torch.testing.assert_close(y.detach().cpu().double(), y64.detach(), rtol=1e-4, atol=1e-5)
    y.backward(gout.to(dev))
    torch.testing.assert_close(xd.grad.cpu().double(), x64.grad, rtol=2e-4, atol=1e-5)
    for name, p, q in zip(("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "bypass.weight", "bypass.bias"),
                          (c1.weight, c1.bias, c2.weight, c2.bias, cb.weight, cb.bias), p64):
        torch.testing.assert_close(p.grad.cpu().double(), q.grad, rtol=2e-4, atol=2e-5, msg=lambda m, name=name: f"{name}: {m}")
