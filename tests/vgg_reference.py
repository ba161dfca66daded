"""Float64 restatement of the VGG16 trunk of VGGLoss (modules/loss.py): forward to the four tapped feature maps and, given the gradients
at the taps, the input-gradient chain back to the image.  Plain torch on the CPU, no autograd, no library import.

``rnd`` is an optional rounding hook, called exactly where the bf16 trunk (FF.vgg_trunk_bf16) stores or packs a bf16 value:
  * the weights of the nine convolutions behind conv1_1 (conv1_1 runs on fp32 weights, forward and adjoint),
  * every activated map a16 (so the taps, the pool's winner rule and every ReLU mask see the rounded values),
  * dy16 at the taps: rnd(a16 > 0 ? gtap + unpool(gpool16) : 0),
  * dx16 of every bf16 adjoint: rnd(a_in16 > 0 ? adj(dy16) : 0) inside a block, rnd(adj(dy16)) into a pooled map.
The image gradient (conv1_1's adjoint) is fp32 in the kernels and is not rounded.  With ``rnd`` None this is the float64 reference.

The pool's winner rule is ATen's (F.max_pool2d on the CPU): the first maximum of a window in row-major order wins, which is the rule of
fmi_maxpool2_bf16.  test_host_vgg_bf16.py checks this file against CPU autograd through the module's own blocks in double.

losses() is the float64 form of what VGGLoss.forward_multi_prepared evaluates on the taps, with the gradients at the taps, built from the
closed forms of tests/loss_reference.py."""
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

import loss_reference as LR

F64 = torch.float64
BLOCKS = (2, 2, 3, 3)

# the trunk cases of test_gpu_vgg_bf16.py: (N, H, W, seed).  test_host_vgg_bf16.py establishes for each that every one of the ten ReLU
# outputs has between 30 % and 70 % positive entries, so the masks are exercised.
TRUNK_CASES = [(2, 32, 32, 11), (3, 40, 48, 12)]


def rnd_bf16(t):
    """round-to-nearest-even to bf16, returned as float64"""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def trunk_inputs(n, h, w, seed, channels=(64, 128, 256, 512)):
    """x fp32 [N, H, W, 3] ~ N(0, 1) and the four fp32 tap gradients [N, H/2^i, W/2^i, C_i] ~ N(0, 1) / numel"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, 3, generator=g)
    gtaps = []
    for i, c in enumerate(channels):
        t = torch.randn(n, h >> i, w >> i, c, generator=g)
        gtaps.append(t / t.numel())
    return x, gtaps


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def trunk(x, weights, biases, gtaps=None, rnd=None, blocks=BLOCKS):
    """x [N, H, W, 3], weights [K, C, 3, 3] and biases [K] per convolution, gtaps NHWC per block, a function of the taps that returns
    them (a loss behind the trunk), or None; any dtype, computed in float64.
    Returns taps (NHWC), acts (the ten activated maps, NHWC) and gx (NHWC, the image gradient; None without gtaps)."""
    r = rnd if rnd is not None else (lambda t: t)
    ws = [w.to(F64) if i == 0 else r(w.to(F64)) for i, w in enumerate(weights)]
    bs = [b.to(F64) for b in biases]
    h = _nchw(x.to(F64))
    acts, taps, idxs, li = [], [], [], 0
    for bi, nconv in enumerate(blocks):
        for _ in range(nconv):
            h = r(F.relu(F.conv2d(h, ws[li], bs[li], padding=1)))
            acts.append(h)
            li += 1
        taps.append(h)
        if bi + 1 < len(blocks):
            h, idx = F.max_pool2d(h, 2, 2, return_indices=True)
            idxs.append(idx)
    out = NS(taps=[_nhwc(t) for t in taps], acts=[_nhwc(a) for a in acts], gx=None)
    if gtaps is None:
        return out
    if callable(gtaps):
        gtaps = gtaps(out.taps)
    first = [sum(blocks[:bi]) for bi in range(len(blocks))]
    gpool = None
    for bi in reversed(range(len(blocks))):
        last = first[bi] + blocks[bi] - 1
        a = acts[last]
        g = _nchw(gtaps[bi].to(F64))
        if gpool is not None:
            g = g + F.max_unpool2d(gpool, idxs[bi], 2, 2, output_size=a.shape[2:])
        dy = r(torch.where(a > 0, g, torch.zeros((), dtype=F64)))
        for li in range(last, first[bi] - 1, -1):
            dx = F.conv_transpose2d(dy, ws[li], padding=1)
            if li == 0:
                out.gx = _nhwc(dx)
                return out
            if li > first[bi]:
                dx = torch.where(acts[li - 1] > 0, dx, torch.zeros((), dtype=F64))
            dy = r(dx)
        gpool = dy
    raise AssertionError("unreachable")


def losses(xt, yt, loss_types, want_grad=True):
    """xt, yt: the four NHWC taps of the gradient batch and of the target batch (batch k N for k loss types, stacked as
    forward_multi_prepared stacks them).  Returns ([loss per type], [gradient of sum(weights * losses) at each tap of xt]) in float64;
    the weights are 1."""
    k = len(loss_types)
    vals = [torch.zeros((), dtype=F64) for _ in range(k)]
    grads = []
    for i, (x, y) in enumerate(zip(xt, yt)):
        x, y = x.to(F64), y.to(F64)
        nk, h, w, c = x.shape
        n = nk // k
        dim = c * h * w
        g = torch.zeros_like(x)
        for j, lt in enumerate(loss_types):
            xs, ys = x[j * n:(j + 1) * n], y[j * n:(j + 1) * n]
            if lt == "perceptual":
                r = LR.reduce_loss(0, xs, ys, 0.0, 1.0 / xs.numel(), gscale=1.0 / dim)
                vals[j] = vals[j] + r.out / dim
                g[j * n:(j + 1) * n] = r.ga
            elif lt == "style":
                xm, ym = xs.reshape(n, h * w, c), ys.reshape(n, h * w, c)
                a = 1.0 / (c * h * w)
                gx_, gy_ = a * xm.transpose(1, 2) @ xm, a * ym.transpose(1, 2) @ ym
                r = LR.reduce_loss(0, gx_, gy_, 0.0, 1.0 / gx_.numel(), gscale=1.0 / (c * c * dim))
                vals[j] = vals[j] + r.out / (c * c * dim)
                g[j * n:(j + 1) * n] = (a * xm @ (r.ga + r.ga.transpose(1, 2))).reshape(n, h, w, c)
            elif lt == "contextual" and i == 3:
                ch = LR.cx_chain(xs.reshape(n, h * w, c), ys.reshape(n, h * w, c))
                vals[j] = vals[j] + ch.loss.loss / dim
                if want_grad:
                    g[j * n:(j + 1) * n] = LR.cx_chain_bwd(ch, gscale=1.0 / dim).reshape(n, h, w, c)
        grads.append(g)
    return vals, grads
