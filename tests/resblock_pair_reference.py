"""Float64 reference of the stride-1 ResBlock pair  y = conv3x3(x1, W1) + conv1x1(x2, W2) + b1 + b2  (fmi_conv2d_pair_fwd_f32 /
fmi_conv2d_pair_wgrad_f32, csrc/conv_pair.h) with CPU autograd, its seeded inputs, and the shapes the tests share.  The reference is
written out as an explicit sum over the nine taps of zero-padded NHWC tensors; tests/test_host_resblock_pair.py checks it against
torch.nn.functional."""
import torch
import torch.nn.functional as F

# (N, H, W, C1, C2, K): the smallest shapes that reach each branch of the kernels
SHAPES = [
    (1, 1, 1, 64, 64, 64),       # every 3x3 tap but the centre outside the image; one partial row tile
    (1, 3, 5, 64, 16, 64),       # C2 != C1 with a single 16-channel extension step: pitch / pointer mix-ups
    (2, 7, 9, 64, 64, 64),       # M = 126: a ragged tile tail
    (1, 16, 16, 64, 64, 64),     # reduction 640 over 2 tiles: the split-reduction branch with the two-bias init
    (2, 12, 12, 128, 128, 256),  # two column tiles
    (1, 6, 6, 16, 16, 32),       # the Nout <= 32 branch of the tap-reuse family
    (2, 9, 9, 32, 32, 64),       # C = 32: the generic implicit-GEMM family
    (2, 8, 8, 16, 16, 16),       # fewer output channels than the narrowest tile has columns (the small networks of the model tests)
]
SPLIT_SHAPE = (1, 16, 16, 64, 64, 64)


def make(n, h, w, c1, c2, k, seed=0):
    """seeded NHWC inputs, torch-layout weights [K][C][kh][kw], biases and an output gradient"""
    g = torch.Generator().manual_seed(1000 * seed + 97 * h + 13 * w + c1 + c2 + k)
    x1 = torch.randn(n, h, w, c1, generator=g)
    x2 = torch.randn(n, h, w, c2, generator=g)
    w1 = torch.randn(k, c1, 3, 3, generator=g) * 0.05
    w2 = torch.randn(k, c2, 1, 1, generator=g) * 0.1
    b1 = torch.randn(k, generator=g)
    b2 = torch.randn(k, generator=g)
    gy = torch.randn(n, h, w, k, generator=g)
    return x1, x2, w1, w2, b1, b2, gy


def pack(w):
    """torch layout [K][C][kh][kw] -> the forward pack [taps][C][K]"""
    k, c, kh, kw = w.shape
    return w.permute(2, 3, 1, 0).reshape(kh * kw, c, k).contiguous()


def pair64(x1, x2, w1, w2, b1, b2):
    """float64  conv3x3(x1, W1) + conv1x1(x2, W2) + b1 + b2  on NHWC tensors, as an explicit sum over the taps (differentiable)"""
    n, h, w, _ = x1.shape
    xp = F.pad(x1, (0, 0, 1, 1, 1, 1))  # zero padding of W and H
    y = torch.einsum("nhwc,kc->nhwk", x2, w2[:, :, 0, 0])
    for ky in range(3):
        for kx in range(3):
            y = y + torch.einsum("nhwc,kc->nhwk", xp[:, ky:ky + h, kx:kx + w, :], w1[:, :, ky, kx])
    if b1 is not None:
        y = y + b1
    if b2 is not None:
        y = y + b2
    return y


def reference(x1, x2, w1, w2, b1, b2, gy):
    """float64 forward and CPU autograd: y, dW1 [9][C1][K], dW2 [1][C2][K], dbias [K] (the gradient of b1 and of b2), dx1, dx2"""
    t = [v.double().requires_grad_(True) for v in (x1, x2, w1, w2)]
    zero = torch.zeros(w1.shape[0], dtype=torch.float64)
    bb1 = (zero if b1 is None else b1.double()).clone().requires_grad_(True)
    bb2 = (zero if b2 is None else b2.double()).clone().requires_grad_(True)
    y = pair64(t[0], t[1], t[2], t[3], bb1, bb2)
    y.backward(gy.double())
    assert torch.equal(bb1.grad, bb2.grad)
    return y.detach(), pack(t[2].grad), pack(t[3].grad), bb1.grad, t[0].grad, t[1].grad


def dw_tol(n, h, w):
    """atol of weight / bias gradients: fp32 sums over the output pixels (dw_tol of tests/test_gpu_thin_paths.py)"""
    return 1e-4 * max(1.0, (n * h * w / 2048.0) ** 0.5)
