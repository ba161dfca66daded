"""GPU: the one-pass backward of the generator's Output block (fmi_conv2d_thin_lrelu_bwd_f32: input gradient, weight gradient and
bias gradient of tanh(conv3x3(pad(lrelu(x)))) from one read of x) against autograd on the CPU, against the three separate entries it
replaces at full size, and for bit-reproducibility.  Tolerances are the ones the existing tests of these kernels use
(tests/test_gpu_kernels.py::test_output_block_fused_lrelu_conv_tanh): dx rtol 1e-4 / atol 1e-5, dW and dbias rtol 1e-4 /
atol 1e-4 * max(1, sqrt(N*H*W / 2048)) (fp32 sums over N*H*W pixels)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SLOPE = 0.1


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


def dw_tol(n, h, w):
    return 1e-4 * max(1.0, (n * h * w / 2048.0) ** 0.5)


def fused_bwd(FF, d, x, gy, y, wt, k, with_bias=True):
    """the C entry on device tensors; outputs start as NaN: the entry must write every element and needs nothing zeroed"""
    from face_mask_inpaint_amd import _lib

    lib = _lib.lib()
    dev = x.device
    gx = torch.full_like(x, float("nan"))
    gw = torch.full((9, x.shape[3], k), float("nan"), device=dev)
    gb = torch.full((k,), float("nan"), device=dev) if with_bias else None
    nb = lib.conv2d_thin_lrelu_bwd_ws_bytes(C.byref(d))
    assert nb > 0
    ws = torch.full((nb // 4,), float("nan"), device=dev)
    lib.conv2d_thin_lrelu_bwd_f32(C.byref(d), FF._p(x), SLOPE, FF._p(gy), FF._p(y), FF._p(wt), FF._p(gx), FF._p(gw), FF._p(gb), FF._p(ws), nb, FF._st())
    return gx, gw, gb


# one tile; ragged in both directions; several tiles with a ragged edge; height 3; width 3; N = 3; exact tile multiples; the smallest
# image with an interior tile (26 x 98: exactly one); a 3 x 4 interior with ragged edges
SHAPES = [(1, 8, 32), (1, 70, 33), (2, 130, 70), (2, 3, 40), (2, 37, 3), (3, 20, 24), (1, 3, 3), (2, 16, 64), (1, 9, 34), (1, 26, 98), (2, 41, 200)]


@pytest.mark.parametrize("with_y", [True, False])
@pytest.mark.parametrize("pad_mode", [1, 0])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_fused_backward_against_autograd(dev, FF, n, h, w, pad_mode, with_y):
    """with_y: tanh(conv(...)) with the tanh output handed to the entry; otherwise the plain convolution output"""
    c, k = 32, 3
    g = torch.Generator().manual_seed(h * 131 + w * 7 + n + 2 * pad_mode + with_y)
    x = torch.randn(n, c, h, w, generator=g, requires_grad=True)
    wt_ = (torch.randn(k, c, 3, 3, generator=g) / (c * 9) ** 0.5).requires_grad_(True)
    b = torch.randn(k, generator=g, requires_grad=True)
    a = F.leaky_relu(x, SLOPE)
    ap = F.pad(a, (1, 1, 1, 1), mode="reflect") if pad_mode else F.pad(a, (1, 1, 1, 1))
    y = F.conv2d(ap, wt_, b)
    if with_y:
        y = torch.tanh(y)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    d, _, _ = FF.conv_desc(n, h, w, c, k, 3, 3, 1, 1, pad_mode)
    wtp = pack(wt_.detach())[1].to(dev)
    yd = nhwc(y.detach()).to(dev) if with_y else None
    gx, gw, gb = fused_bwd(FF, d, nhwc(x.detach()).to(dev), nhwc(gy).to(dev), yd, wtp, k)
    err = lambda t, r: float((t.cpu() - r).abs().max())
    print("n%d %dx%d pad_mode %d y %d: max|err| dx %.3g  dW %.3g  dbias %.3g" % (n, h, w, pad_mode, with_y, err(gx, nhwc(x.grad)), err(gw, pack(wt_.grad)[0]), err(gb, b.grad)))
    torch.testing.assert_close(gx.cpu(), nhwc(x.grad), rtol=1e-4, atol=1e-5)
    tol = dw_tol(n, h, w)
    torch.testing.assert_close(gw.cpu(), pack(wt_.grad)[0], rtol=1e-4, atol=tol)
    torch.testing.assert_close(gb.cpu(), b.grad, rtol=1e-4, atol=tol)


def test_fused_backward_without_bias_and_k4(dev, FF):
    """dbias = NULL, and K = 4 (every component of the staged window carries data)"""
    n, c, k, h, w = 2, 32, 4, 21, 45
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, c, h, w, generator=g, requires_grad=True)
    wt_ = (torch.randn(k, c, 3, 3, generator=g) / (c * 9) ** 0.5).requires_grad_(True)
    y = torch.tanh(F.conv2d(F.pad(F.leaky_relu(x, SLOPE), (1, 1, 1, 1), mode="reflect"), wt_))
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    d, _, _ = FF.conv_desc(n, h, w, c, k, 3, 3, 1, 1, 1)
    gx, gw, gb = fused_bwd(FF, d, nhwc(x.detach()).to(dev), nhwc(gy).to(dev), nhwc(y.detach()).to(dev), pack(wt_.detach())[1].to(dev), k, with_bias=False)
    assert gb is None
    torch.testing.assert_close(gx.cpu(), nhwc(x.grad), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(gw.cpu(), pack(wt_.grad)[0], rtol=1e-4, atol=dw_tol(n, h, w))


@pytest.mark.parametrize("rows", [2, 5])
def test_fused_backward_with_a_small_workspace(dev, FF, rows):
    """a workspace smaller than the documented size only lowers the number of workgroups (interior and border launch share its rows)"""
    from face_mask_inpaint_amd import _lib

    lib = _lib.lib()
    n, c, k, h, w = 2, 32, 3, 50, 140
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(n, c, h, w, generator=g, requires_grad=True)
    wt_ = (torch.randn(k, c, 3, 3, generator=g) / (c * 9) ** 0.5).requires_grad_(True)
    b = torch.randn(k, generator=g, requires_grad=True)
    y = torch.tanh(F.conv2d(F.pad(F.leaky_relu(x, SLOPE), (1, 1, 1, 1), mode="reflect"), wt_, b))
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    d, _, _ = FF.conv_desc(n, h, w, c, k, 3, 3, 1, 1, 1)
    xd, gyd, yd, wtp = nhwc(x.detach()).to(dev), nhwc(gy).to(dev), nhwc(y.detach()).to(dev), pack(wt_.detach())[1].to(dev)
    gx, gw, gb = torch.full_like(xd, float("nan")), torch.full((9, c, k), float("nan"), device=dev), torch.full((k,), float("nan"), device=dev)
    nb = rows * (9 * c * k + k) * 4
    assert nb < lib.conv2d_thin_lrelu_bwd_ws_bytes(C.byref(d))
    ws = torch.full((nb // 4,), float("nan"), device=dev)
    lib.conv2d_thin_lrelu_bwd_f32(C.byref(d), FF._p(xd), SLOPE, FF._p(gyd), FF._p(yd), FF._p(wtp), FF._p(gx), FF._p(gw), FF._p(gb), FF._p(ws), nb, FF._st())
    torch.testing.assert_close(gx.cpu(), nhwc(x.grad), rtol=1e-4, atol=1e-5)
    tol = dw_tol(n, h, w)
    torch.testing.assert_close(gw.cpu(), pack(wt_.grad)[0], rtol=1e-4, atol=tol)
    torch.testing.assert_close(gb.cpu(), b.grad, rtol=1e-4, atol=tol)


def test_fused_backward_full_size_against_separate_entries(dev, FF):
    """8 x 1024 x 1024 x 32 -> 3, reflect padding, tanh: the fused launch against tanh-backward + adjoint + weight gradient, and the
    adjointness identities of test_thin_output_conv_adjointness_full_size on its own results"""
    from face_mask_inpaint_amd import _lib

    lib = _lib.lib()
    n, h, c, k = 8, 1024, 32, 3
    torch.manual_seed(11)
    x = torch.randn(n, h, h, c, device=dev)
    w = torch.randn(k, c, 3, 3, device=dev) / (9 * c) ** 0.5
    wf, wt = pack(w)
    b = torch.randn(k, device=dev) * 0.1
    d, _, _ = FF.conv_desc(n, h, h, c, k, 3, 3, 1, 1, 1)
    st = FF._st()
    y = torch.empty(n, h, h, k, device=dev)
    lib.conv2d_thin_lrelu_fwd_f32(C.byref(d), FF._p(x), SLOPE, FF._p(wf), FF._p(b), FF._p(y), FF.ACT_TANH, st)
    gy = torch.randn_like(y)
    # the separate entries
    gt = FF.eltwise(FF.EW_TANH_BWD, gy, y)
    gx0 = torch.empty_like(x)
    lib.conv2d_thin_lrelu_dgrad_f32(C.byref(d), FF._p(gt), FF._p(wt), FF._p(x), SLOPE, FF._p(gx0), st)
    gw0, gb0 = torch.zeros_like(wf), torch.zeros(k, device=dev)
    lib.conv2d_thin_lrelu_wgrad_f32(C.byref(d), FF._p(x), SLOPE, FF._p(gt), FF._p(gw0), FF._p(gb0), st)
    gx, gw, gb = fused_bwd(FF, d, x, gy, y, wt, k)
    tol = dw_tol(n, h, h)
    print("full size: max|diff| dx %.3g  dW %.3g (bound %.3g)  dbias %.3g" % (float((gx - gx0).abs().max()), float((gw - gw0).abs().max()), tol, float((gb - gb0).abs().max())))
    torch.testing.assert_close(gx, gx0, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(gw, gw0, rtol=1e-4, atol=tol)
    torch.testing.assert_close(gb, gb0, rtol=1e-4, atol=tol)
    # <conv(lrelu(x)), gt> = <x, dx> (lrelu(x) = x * lrelu'(x)) = <W, dW>;  dbias = sum gt
    dot = lambda a_, b_: float((a_.double() * b_.double()).sum())
    z = torch.empty_like(y)
    lib.conv2d_thin_lrelu_fwd_f32(C.byref(d), FF._p(x), SLOPE, FF._p(wf), None, FF._p(z), FF.ACT_NONE, st)
    lhs, scale = dot(z, gt), float(z.norm()) * float(gt.norm())
    assert abs(lhs - dot(x, gx)) <= 2e-5 * scale
    assert abs(lhs - dot(wf, gw)) <= 2e-5 * scale
    assert abs(float(gb.double().sum()) - float(gt.double().sum())) <= 1e-5 * float(gt.abs().sum())


@pytest.mark.parametrize("n,h,w", [(2, 130, 70), (4, 512, 512)])
def test_fused_backward_bit_reproducible_in_both_modes(dev, FF, n, h, w):
    """no atomics on this path: two runs on the same inputs are torch.equal in reproducible mode AND in the default mode, and the two
    modes agree (within the dW bound; they run the same launch)"""
    c, k = 32, 3
    torch.manual_seed(h + w)
    x = torch.randn(n, h, w, c, device=dev)
    wt = pack(torch.randn(k, c, 3, 3, device=dev) / (9 * c) ** 0.5)[1]
    y = torch.tanh(torch.randn(n, h, w, k, device=dev))
    gy = torch.randn_like(y)
    d, _, _ = FF.conv_desc(n, h, w, c, k, 3, 3, 1, 1, 1)
    res = {}
    for mode in (True, False):
        with FF.deterministic(mode):
            r1 = fused_bwd(FF, d, x, gy, y, wt, k)
            r2 = fused_bwd(FF, d, x, gy, y, wt, k)
        for a_, b_ in zip(r1, r2):
            assert torch.equal(a_, b_)
        res[mode] = r1
    tol = dw_tol(n, h, w)
    torch.testing.assert_close(res[True][0], res[False][0], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(res[True][1], res[False][1], rtol=1e-4, atol=tol)
    torch.testing.assert_close(res[True][2], res[False][2], rtol=1e-4, atol=tol)


def test_output_block_autograd_takes_the_fused_backward(dev, FF):
    """FF.lrelu_conv2d with both gradients wanted goes through the fused entry (one conv_bwd record) and matches autograd; with only the
    weight gradient wanted it keeps the separate entries"""
    n, c, k, h, w = 2, 32, 3, 40, 50
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, c, h, w, generator=g, requires_grad=True)
    wt_ = (torch.randn(k, c, 3, 3, generator=g) / (c * 9) ** 0.5).requires_grad_(True)
    b = torch.randn(k, generator=g, requires_grad=True)
    y = torch.tanh(F.conv2d(F.pad(F.leaky_relu(x, SLOPE), (1, 1, 1, 1), mode="reflect"), wt_, b))
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    tol = dw_tol(n, h, w)
    for want_gx in (True, False):
        wf, wtp = [t.to(dev) for t in pack(wt_.detach())]
        wf.requires_grad_(True)
        xd, bd = nhwc(x.detach()).to(dev).requires_grad_(want_gx), b.detach().to(dev).requires_grad_(True)
        out = FF.lrelu_conv2d(xd, FF.PackedWeight(wf, wtp, k, c, 3, 3), bd, SLOPE, 1, 1, FF.ACT_TANH)
        FF.PROFILE = []
        try:
            out.backward(nhwc(gy).to(dev))
            tags = [r[0].split("|")[0] for r in FF.PROFILE]
        finally:
            FF.PROFILE = None
        assert tags == (["conv_bwd"] if want_gx else ["conv_wgrad"])
        if want_gx:
            torch.testing.assert_close(xd.grad.cpu(), nhwc(x.grad), rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(wf.grad.cpu(), pack(wt_.grad)[0], rtol=1e-4, atol=tol)
        torch.testing.assert_close(bd.grad.cpu(), b.grad, rtol=1e-4, atol=tol)
