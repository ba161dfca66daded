"""GPU: the one-pass backward of the decoder's ConvTranspose2d pair (fmi_conv_transpose2d_pair_bwd_f32, csrc/convt3x3_bwd.hip: both input
gradients, both weight gradients and the bias gradient of ConvTranspose2d(x1, W1) + ConvTranspose2d(x2, W2) + bias from one read of the
gradient) against float64 autograd on the CPU, against the separate launches it replaces, and for bit-reproducibility.  Tolerances are
the ones this project uses for these products: input gradients rtol 1e-4 / atol 1e-5; weight and bias gradients rtol 1e-4 / atol
1e-4 * max(1, sqrt(N * H_out * W_out / 2048)) (fp32 sums over the output pixels; dw_tol of tests/test_gpu_thin_paths.py)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def FF():
    from face_mask_inpaint_amd import functional

    return functional


def dw_tol(n, hout, wout):
    return 1e-4 * max(1.0, (n * hout * wout / 2048.0) ** 0.5)


def make(n, h, w, c1, c2, cb, seed):
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn(n, h, w, c1, generator=g)
    x2 = torch.randn(n, h, w, c2, generator=g)
    w1 = torch.randn(c1, cb, 3, 3, generator=g) * 0.05  # nn.ConvTranspose2d weight: [in][out][kh][kw]
    w2 = torch.randn(c2, cb, 3, 3, generator=g) * 0.05
    gy = torch.randn(n, 2 * h, 2 * w, cb, generator=g)
    return x1, x2, w1, w2, gy


def reference(x1, x2, w1, w2, gy):
    """float64 autograd on the CPU; weight gradients in the pack's layout [tap][out][in]"""
    t = [v.double().requires_grad_(True) for v in (x1, x2, w1, w2)]
    b = torch.zeros(w1.shape[1], dtype=torch.float64, requires_grad=True)
    y = (F.conv_transpose2d(t[0].permute(0, 3, 1, 2), t[2], None, stride=2, padding=1, output_padding=1) +
         F.conv_transpose2d(t[1].permute(0, 3, 1, 2), t[3], b, stride=2, padding=1, output_padding=1))
    y.backward(gy.double().permute(0, 3, 1, 2))
    packg = lambda gw: gw.permute(2, 3, 1, 0).reshape(9, gw.shape[1], gw.shape[0])
    return t[0].grad, t[1].grad, packg(t[2].grad), packg(t[3].grad), b.grad


def entry(FF, dev, x1, x2, w1, w2, gy, with_bias=True, det=None):
    """the C entry on device tensors; outputs and workspace start as NaN: the entry must write every element and needs nothing zeroed"""
    from face_mask_inpaint_amd import _lib

    lib = _lib.lib()
    n, h, w, c1 = x1.shape
    c2, cb = x2.shape[3], w1.shape[1]
    x1d, x2d, gyd = x1.to(dev), x2.to(dev), gy.to(dev)
    pw1, pw2 = FF.prepare_weights([(w1.to(dev), None, None), (w2.to(dev), None, None)])
    d, _, _ = FF.conv_desc(n, 2 * h, 2 * w, cb, c1, 3, 3, 2, 1)
    assert lib.conv_transpose2d_pair_bwd_supported(C.byref(d), c1, c2) == 1
    nan = float("nan")
    gx1, gx2 = torch.full_like(x1d, nan), torch.full_like(x2d, nan)
    gw1, gw2 = torch.full((9, cb, c1), nan, device=dev), torch.full((9, cb, c2), nan, device=dev)
    gb = torch.full((cb,), nan, device=dev) if with_bias else None
    nb = lib.conv_transpose2d_pair_bwd_ws_bytes(C.byref(d), c1, c2)
    assert nb > 0
    ws = torch.full((nb // 4,), nan, device=dev)
    old = lib.get_deterministic()
    if det is not None:
        lib.set_deterministic(det)
    try:
        lib.conv_transpose2d_pair_bwd_f32(C.byref(d), FF._p(x1d), FF._p(x2d), c2, FF._p(gyd), C.c_void_p(pw1.w3[0].data_ptr()), C.c_void_p(pw2.w3[0].data_ptr()),
                                          FF._p(gx1), FF._p(gx2), FF._p(gw1), FF._p(gw2), FF._p(gb), FF._p(ws), nb, FF._st())
    finally:
        lib.set_deterministic(old)
    torch.cuda.synchronize()
    return gx1, gx2, gw1, gw2, gb


# tile = 4 x 16 input pixels.  Single pixel / single row (every window cell but one outside the image); 3 x 3; ragged strips; image boundaries
# inside a tile row; one column past eight tiles; exact tile multiples; one exact tile, one more and one less in each tile dimension;
# several tiles ragged in both directions; more tiles than resident workgroups (a persistent workgroup walks several, n 2 80x260: 680 tiles)
SHAPES = [(1, 1, 1), (1, 1, 5), (1, 3, 3), (2, 2, 70), (2, 37, 3), (3, 20, 24), (1, 9, 130), (2, 16, 128), (1, 4, 16), (1, 5, 17), (1, 3, 15), (2, 41, 200)]
CHANNELS = [(32, 64, 32), (64, 32, 32), (32, 32, 32), (64, 64, 32)]


def check(FF, dev, n, h, w, c1, c2, cb):
    x1, x2, w1, w2, gy = make(n, h, w, c1, c2, cb, h * 131 + w * 7 + n + c1)
    ref = reference(x1, x2, w1, w2, gy)
    out = entry(FF, dev, x1, x2, w1, w2, gy)
    err = [float((o.cpu().double() - r).abs().max()) for o, r in zip(out, ref)]
    print("n%d %dx%d %d+%d->%d: max|err| gx1 %.3g gx2 %.3g gW1 %.3g gW2 %.3g gb %.3g" % ((n, h, w, c1, c2, cb) + tuple(err)))
    tol = dw_tol(n, 2 * h, 2 * w)
    for o, r in zip(out[:2], ref[:2]):
        torch.testing.assert_close(o.cpu(), r.float(), rtol=1e-4, atol=1e-5)
    for o, r in zip(out[2:], ref[2:]):
        torch.testing.assert_close(o.cpu(), r.float(), rtol=1e-4, atol=tol)


@pytest.mark.parametrize("c1,c2,cb", CHANNELS)
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_pair_backward_against_float64_autograd(dev, FF, n, h, w, c1, c2, cb):
    check(FF, dev, n, h, w, c1, c2, cb)


def test_pair_backward_with_more_tiles_than_workgroups(dev, FF):
    check(FF, dev, 2, 80, 260, 32, 64, 32)


def test_pair_backward_with_null_outputs(dev, FF):
    """every output pointer is nullable: without the bias gradient the other four are unchanged"""
    x1, x2, w1, w2, gy = make(2, 9, 21, 32, 64, 32, 3)
    a = entry(FF, dev, x1, x2, w1, w2, gy)
    b = entry(FF, dev, x1, x2, w1, w2, gy, with_bias=False)
    assert b[4] is None
    for u, v in zip(a[:4], b[:4]):
        assert torch.equal(u, v)


@pytest.mark.parametrize("n,h,w", [(2, 128, 128), (1, 130, 254)])
def test_pair_backward_equals_the_separate_launches(dev, FF, n, h, w):
    """the five gradients against the two single ConvTranspose2d backwards on the shared gradient: 1e-5 of the largest entry, the bound of
    tests/test_gpu_p3.py::test_conv_transpose_pair_equals_two_calls"""
    c1, c2, cb = 32, 64, 32
    x1, x2, w1, w2, gy = make(n, h, w, c1, c2, cb, n + h)
    out = entry(FF, dev, x1, x2, w1, w2, gy)
    t = [v.to(dev).requires_grad_(True) for v in (x1, x2, w1, w2)]
    b = torch.zeros(cb, device=dev, requires_grad=True)
    pw1, pw2 = FF.prepare_weights([(t[2], None, None), (t[3], None, None)])
    y = FF.conv_transpose2d(t[0], pw1, b, residual=FF.conv_transpose2d(t[1], pw2))
    y.backward(gy.to(dev))
    packg = lambda gw: gw.permute(2, 3, 1, 0).reshape(9, gw.shape[1], gw.shape[0])
    sep = (t[0].grad, t[1].grad, packg(t[2].grad), packg(t[3].grad), b.grad)
    for name, o, s in zip(("gx1", "gx2", "gW1", "gW2", "gb"), out, sep):
        m = float(s.abs().max())
        print("n%d %dx%d %s: max|diff| %.3g of max|separate| %.3g" % (n, h, w, name, float((o - s).abs().max()), m))
        torch.testing.assert_close(o, s, rtol=0, atol=1e-5 * m)


def test_pair_backward_is_bit_reproducible(dev, FF):
    """two calls on the same inputs, and reproducible mode on against off: identical bits"""
    x1, x2, w1, w2, gy = make(2, 70, 130, 32, 64, 32, 11)
    a = entry(FF, dev, x1, x2, w1, w2, gy)
    b = entry(FF, dev, x1, x2, w1, w2, gy)
    on = entry(FF, dev, x1, x2, w1, w2, gy, det=1)
    off = entry(FF, dev, x1, x2, w1, w2, gy, det=0)
    for u, v, p, q in zip(a, b, on, off):
        assert torch.equal(u, v) and torch.equal(p, q) and torch.equal(u, p)


def test_pair_backward_refusals_on_the_device(dev, FF):
    """a workspace with fewer rows than workgroups and a misaligned pointer are argument errors, not launches; cb = 28 and 16-channel inputs
    are not supported (and keep the separate launches)"""
    from face_mask_inpaint_amd import _lib

    lib = _lib.lib()
    n, h, w, c1, c2, cb = 1, 16, 64, 32, 64, 32
    d, _, _ = FF.conv_desc(n, 2 * h, 2 * w, cb, c1, 3, 3, 2, 1)
    buf = torch.zeros(1 << 20, device=dev)
    p = lambda off=0: C.c_void_p(buf.data_ptr() + off)
    nb = lib.conv_transpose2d_pair_bwd_ws_bytes(C.byref(d), c1, c2)
    row = (9 * cb * (c1 + c2) + cb) * 4
    assert nb == 16 * row  # 4 x 4 tiles, one workgroup and one row each
    raw = lib.cdll.fmi_conv_transpose2d_pair_bwd_f32
    args = lambda ws_bytes, x1off=0: (C.byref(d), p(x1off), p(), c2, p(), p(), p(), None, None, None, None, None, p(), ws_bytes, FF._st())
    assert raw(*args(3 * row)) == 1
    assert raw(*args(nb, 4)) == 1
    assert raw(*args(nb)) == 0
    d28, _, _ = FF.conv_desc(n, 2 * h, 2 * w, 28, 16, 3, 3, 2, 1)
    assert lib.conv_transpose2d_pair_bwd_supported(C.byref(d28), 16, 48) == 0
    d16, _, _ = FF.conv_desc(n, 2 * h, 2 * w, 32, 16, 3, 3, 2, 1)
    assert lib.conv_transpose2d_pair_bwd_supported(C.byref(d16), 16, 32) == 0
    assert lib.conv_transpose2d_pair_bwd_supported(C.byref(d), 32, 16) == 0
    torch.cuda.synchronize()
