"""GPU: the bf16 UNet mask detector -- the kernels of csrc/unet_bf16.hip, the one-launch eval conv + BN + ReLU, the train-mode BN + ReLU
pass, the blocks and the whole model, the trainer and both inference harnesses.

Kernel bounds come from two facts: bf16 round-to-nearest errs by at most 2^-8 |v|, fp32 summation of n terms by at most n 2^-24 sum|terms|.
Every float64 reference is computed here with torch.nn.functional on the CPU from the same bf16-rounded inputs.

Block and model level: a pre-activation rounded across zero flips a ReLU gate, so no bound is derivable.  The reference there is an
emulation written below -- float64 with the weights and every stored activation rounded to bf16, straight-through gradient -- and every
tensor must lie within 3 x the emulation's own relative L2 error against plain float64.  The measured ratios are printed."""
import os

import pytest
import torch
import torch.nn.functional as F

from face_mask_inpaint_amd import functional as FF
from face_mask_inpaint_amd._lib import FmiError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
U8, U24 = 2.0 ** -8, 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _exact_bits(t):
    """bit patterns of an fp32 tensor whose values are all bf16 values (a maximum, a routed gradient): the upper halves, NaN payload
    and sign included -- torch's own fp32 -> bf16 conversion would canonicalise a NaN"""
    t = t.detach().cpu().contiguous()
    assert bool(((t.view(torch.int32) & 0xFFFF) == 0).all())
    return (t.view(torch.int32) >> 16).to(torch.int16)


def _same_bits(name, got, want):
    bad = (got != want).nonzero()
    assert bad.numel() == 0, f"{name}: {bad.shape[0]} entries differ, first at {bad[0].tolist()}: {int(got[tuple(bad[0])])} != {int(want[tuple(bad[0])])}"


def _nchw64(t):
    """bf16 / fp32 NHWC tensor -> float64 NCHW on the CPU (exact)"""
    return t.detach().cpu().double().permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _within(name, got, ref, bound):
    err = (got.detach().cpu().double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"  {name}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert bool((err <= bound).all()), f"{name}: err / bound = {worst}"


# ---------------------------------------------------------------------------------------------------------------------------------
# max pooling
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 6, 10, 72), (1, 2, 2, 8)])
def test_maxpool2_bit_exact(dev, shape):
    """post-ReLU values (about 40 % zeros, so ties at 0 are everywhere) plus planted all-equal non-zero windows; y and gx bit-equal to
    torch.max_pool2d forward / backward on the same values.  72 channels = 9 chunks: a remainder against the 256-thread blocks"""
    n, h, w, c = shape
    x = torch.relu(torch.randn(shape, generator=_gen(1)) + 0.25).to(BF)
    assert x.numel() < 1000 or 0.3 < float((x == 0).float().mean()) < 0.5
    x[0, 0:2, 0:2, : c // 2] = 1.5  # whole window equal: the first pixel takes the gradient
    if h > 2:
        x[-1, 2:4, 4:6, :] = 0.75
        x[0, 4:6, 8:10, 3] = 0.0
        x[1, 1, 6, 5] = float("nan")   # third of its window: a later NaN replaces the running maximum and takes the gradient
        x[1, 2, 0, 7] = float("nan")   # first of its window: larger values after it do not replace it
        x[1, 3, 1, 7] = 9.0
    gy = torch.randn((n, h // 2, w // 2, c), generator=_gen(2)).to(BF)
    xr = x.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    yr = F.max_pool2d(xr, 2)
    yr.backward(gy.float().permute(0, 3, 1, 2))
    xd = x.to(dev).requires_grad_(True)
    y = FF.max_pool(xd, 2, 2)
    assert y.dtype == BF and y.shape == (n, h // 2, w // 2, c)
    y.backward(gy.to(dev))
    assert h == 2 or (int(torch.isnan(yr).sum()) == 2 and int(torch.isnan(y).sum()) == 2 and float(xr.grad[1, 7, 3, 1]) == 0.0)
    _same_bits("y", _bits(y), _exact_bits(_nhwc(yr.detach())))
    _same_bits("gx", _bits(xd.grad), _exact_bits(_nhwc(xr.grad)))
    assert torch.equal(_bits(FF.max_pool2(x.to(dev))), _bits(y))


# ---------------------------------------------------------------------------------------------------------------------------------
# upsample + pad + concat
# ---------------------------------------------------------------------------------------------------------------------------------
def _up_ref(x1, skip):
    """unet_parts.py:59-70 in float64 (NCHW)"""
    u = F.interpolate(x1, scale_factor=2, mode="bilinear", align_corners=True)
    dy, dx = skip.shape[2] - u.shape[2], skip.shape[3] - u.shape[3]
    u = F.pad(u, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])
    return torch.cat([skip, u], dim=1)


@pytest.mark.parametrize("s1,s2", [((2, 3, 5, 16), (2, 6, 10, 8)), ((2, 3, 5, 16), (2, 7, 11, 8)), ((1, 1, 1, 8), (1, 2, 2, 8))],
                         ids=["no_border", "odd_border", "degenerate"])
def test_up2_cat_against_float64(dev, s1, s2):
    x1 = torch.randn(s1, generator=_gen(3)).to(BF)
    sk = torch.randn(s2, generator=_gen(4)).to(BF)
    c1, c2 = s1[3], s2[3]
    g = torch.randn(s2[:3] + (c1 + c2,), generator=_gen(5)).to(BF)
    a = _nchw64(x1).requires_grad_(True)
    b = _nchw64(sk).requires_grad_(True)
    ref = _up_ref(a, b)
    ref.backward(_nchw64(g))
    a_abs = _nchw64(x1).requires_grad_(True)
    _up_ref(a_abs, _nchw64(sk)).backward(_nchw64(g).abs())  # the interpolation weights are non-negative: sum |terms| per input pixel
    x1d, skd = x1.to(dev).requires_grad_(True), sk.to(dev).requires_grad_(True)
    y = FF.up2_cat(x1d, skd)
    assert y.dtype == BF and y.shape == g.shape
    y.backward(g.to(dev))
    ref_y = _nhwc(ref.detach())
    # skip half and border: bit exact
    assert torch.equal(_bits(y[..., :c2]), _bits(sk))
    border = _nhwc(_up_ref(torch.ones_like(a), torch.zeros_like(b)).detach())[..., c2:] == 0
    assert int(border.sum()) == (s2[1] * s2[2] - 4 * s1[1] * s1[2]) * s2[0] * c1
    assert bool((y[..., c2:].detach().cpu().float()[border] == 0).all())
    print(f"\nup2_cat {s1} + {s2}:")
    _within("interpolated half", y[..., c2:], ref_y[..., c2:], U8 * ref_y[..., c2:].abs() + 2.0 ** -20 * float(x1.abs().max()))
    assert torch.equal(_bits(skd.grad), _bits(g[..., :c2]))
    gx1 = _nhwc(a.grad)
    _within("gx1", x1d.grad, gx1, U8 * gx1.abs() + 9 * U24 * _nhwc(a_abs.grad))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1 x 1 head
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead,k", [((2, 16, 16), 2), ((1, 1, 515), 3)], ids=["P512_K2", "P515_K3"])
def test_head1x1_against_float64(dev, lead, k):
    c = 64
    x = torch.randn(lead + (c,), generator=_gen(6)).to(BF)
    w = (torch.randn(k, c, 1, 1, generator=_gen(7)) * 0.2)
    b = torch.randn(k, generator=_gen(8)) * 0.5
    xf = x.view(-1, c)
    xf[5], xf[77], xf[-1] = 0, 0, 0               # planted ties: the logits are the biases there ...
    if k == 2:
        b[1] = b[0]                               # ... which are equal: class 0 wins
    else:
        w[2], b[2] = w[1].clone(), b[1].clone()   # K = 3: the last two classes tie at every pixel: class 2 never wins
    g = torch.randn(lead + (k,), generator=_gen(9))
    p = xf.shape[0]
    x64, w64, b64, g64 = xf.double(), w.view(k, c).double(), b.double(), g.view(-1, k).double()
    ref = x64 @ w64.t() + b64
    mag = x64.abs() @ w64.abs().t() + b64.abs()
    xd, wd, bd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    outs = []
    for _ in range(2):
        with FF.deterministic():
            y = FF.head1x1(xd, wd, bd)
            gx, gw, gb = torch.autograd.grad(y, (xd, wd, bd), g.to(dev))
        outs.append((y.detach().clone(), gx.clone(), gw.clone(), gb.clone()))
    assert all(torch.equal(u, v) for u, v in zip(outs[0], outs[1])), "two runs in reproducible mode differ"
    y2 = FF.head1x1(xd, wd, bd)  # the default mode runs the same code: no atomics
    assert torch.equal(y2.detach(), outs[0][0])
    y, gx, gw, gb = outs[0]
    assert y.dtype == torch.float32 and y.shape == lead + (k,) and gx.dtype == BF and gw.shape == w.shape and gb.shape == b.shape
    print(f"\nhead1x1 P = {p}, K = {k}:")
    _within("logits", y.view(-1, k), ref, c * U24 * mag)
    gx_ref = g64 @ w64
    _within("gx", gx.view(-1, c), gx_ref, U8 * gx_ref.abs() + k * U24 * (g64.abs() @ w64.abs()))
    _within("gw", gw.view(k, c), g64.t() @ x64, p * U24 * (g64.abs().t() @ x64.abs()))
    _within("gb", gb, g64.sum(0), p * U24 * g64.abs().sum(0))
    # argmax form = argmax_channels of the stored logits, ties included
    m = FF.head1x1_argmax(xd, wd, bd)
    want = FF.argmax_channels(y)
    assert m.shape == lead and torch.equal(m, want)
    yc, mc = y.view(-1, k).cpu(), m.view(-1).cpu()
    ties = yc[:, k - 1] == yc[:, k - 2]
    if k == 2:
        assert bool(ties[[5, 77, p - 1]].all()) and bool((mc[ties] == 0).all()) and 0.2 < float(mc.mean()) < 0.8
    else:
        assert bool(ties.all()) and float(mc.max()) == 1.0 and float(mc.min()) == 0.0
    assert torch.equal(mc, yc.argmax(-1).float())


# ---------------------------------------------------------------------------------------------------------------------------------
# eval conv + BN + ReLU in one launch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 8, 8, 64), (1, 4, 4, 128)])
def test_conv_bn_relu_eval_one_launch(dev, shape):
    from face_mask_inpaint_amd.weights import packed, weight_scope

    n, h, w, c = shape
    k = 64
    gen = _gen(10)
    conv = torch.nn.Conv2d(c, k, 3, padding=1)
    bn = torch.nn.BatchNorm2d(k)
    with torch.no_grad():
        conv.bias.copy_(torch.randn(k, generator=gen) * 0.3)
        bn.weight.copy_(torch.rand(k, generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(k, generator=gen) * 0.2)
        bn.running_mean.copy_(torch.randn(k, generator=gen) * 0.3)
        bn.running_var.copy_(torch.rand(k, generator=gen) + 0.5)
    x = torch.randn(shape, generator=gen).to(BF)
    blk = torch.nn.Sequential(conv, bn).to(dev).eval()
    object.__setattr__(blk[0], "_fmi_no_w3", True)
    xd = x.to(dev)
    with weight_scope(blk):
        with pytest.raises(FmiError, match="gradients"):
            FF.conv_bn_relu_eval_bf16(xd, packed(blk[0]), blk[0].bias, blk[1])
        with torch.no_grad():
            y = FF.conv_bn_relu_eval_bf16(xd, packed(blk[0]), blk[0].bias, blk[1])
    assert y.dtype == BF and y.shape == (n, h, w, k)
    w64 = conv.weight.detach().cpu().to(BF).double()
    z = F.conv2d(_nchw64(x), w64, padding=1)
    mag = F.conv2d(_nchw64(x).abs(), w64.abs(), padding=1)
    scale = (bn.weight.detach().cpu().double() / torch.sqrt(bn.running_var.cpu().double() + bn.eps)).view(1, k, 1, 1)
    shift = bn.bias.detach().cpu().double().view(1, k, 1, 1) + (conv.bias.detach().cpu().double() - bn.running_mean.cpu().double()).view(1, k, 1, 1) * scale
    ref = torch.relu(z * scale + shift)
    print(f"\nconv + BN + ReLU (eval) {shape} -> {k}: {float((ref == 0).double().mean()):.2f} of the outputs are gated off")
    _within("y", y, _nhwc(ref), _nhwc(U8 * ref.abs() + 9 * c * U24 * mag * scale.abs()))


# ---------------------------------------------------------------------------------------------------------------------------------
# train-mode BN + ReLU on bf16
# ---------------------------------------------------------------------------------------------------------------------------------
def test_batch_norm_relu_train_bf16(dev):
    """forward 2^-8 |ref| + 2^-18 max|ref|.  Backward, same form per tensor for the bf16 gx (2^-18 of the largest entry = 64 fp32 ulps
    for the fp32 mean / rstd and the handful of fp32 operations per element); g_gamma / g_beta are sums over P = 128 pixels: P 2^-24
    sum|terms|.  Elements whose float64 pre-activation is below 1e-5 in magnitude may legitimately take the other ReLU gate: they are
    left out of gx and their terms are granted to the two sums; at most 0.1 % of the elements may be such."""
    shape = (2, 8, 8, 64)
    c, eps = 64, 1e-5
    gen = _gen(11)
    x = torch.randn(shape, generator=gen).to(BF)
    gamma, beta = torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen) * 0.3
    g = torch.randn(shape, generator=gen).to(BF)
    x64 = _nchw64(x).requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    pre = F.batch_norm(x64, None, None, g64, b64, training=True, eps=eps)
    ref = torch.relu(pre)
    ref.backward(_nchw64(g))
    xd, gd, bd = x.to(dev).requires_grad_(True), gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    y, stats, sums = FF.batch_norm_train(xd, gd, bd, eps, slope=0.0)
    assert y.dtype == BF
    y.backward(g.to(dev))
    print("\nBN + ReLU (train) on bf16:")
    r = _nhwc(ref.detach())
    _within("y", y, r, U8 * r.abs() + 2.0 ** -18 * float(r.abs().max()))
    near = _nhwc(pre.detach().abs() < 1e-5)
    share = float(near.double().mean())
    print(f"  pre-activations within 1e-5 of zero: {int(near.sum())} ({share:.2e})")
    assert share <= 1e-3
    gxr = _nhwc(x64.grad)
    bound = U8 * gxr.abs() + 2.0 ** -18 * float(gxr.abs().max())
    bound[near] = float("inf")
    _within("gx", xd.grad, gxr, bound)
    xhat = _nhwc(((pre.detach() - b64.detach().view(1, c, 1, 1)) / g64.detach().view(1, c, 1, 1)))
    gate = _nhwc((pre.detach() > 0).double())
    gn = _nhwc(_nchw64(g))
    p = shape[0] * shape[1] * shape[2]
    t_gamma, t_beta = (gn * gate * xhat).abs(), (gn * gate).abs()
    slack_g, slack_b = ((gn * xhat).abs() * near).sum((0, 1, 2)), (gn.abs() * near).sum((0, 1, 2))
    _within("g_gamma", gd.grad, g64.grad, p * U24 * t_gamma.sum((0, 1, 2)) + slack_g)
    _within("g_beta", bd.grad, b64.grad, p * U24 * t_beta.sum((0, 1, 2)) + slack_b)


# ---------------------------------------------------------------------------------------------------------------------------------
# blocks and the whole model against the emulation
# ---------------------------------------------------------------------------------------------------------------------------------
def _q(t):
    """round to bf16 with a straight-through gradient"""
    return t + (t.detach().to(BF).double() - t.detach())


def _ident(t):
    return t


_RUNNING = None  # a dict while a test wants the running statistics the train-mode emulation leaves behind (name -> tensor)


def _cbr(P, pre, x, q, train, bf16_conv=True):
    """conv => BN => ReLU of DoubleConv in float64; q rounds what the bf16 path stores: the weights, the convolution's output (batch
    statistics only: with running statistics the launch is fused and stores the activation alone) and the activation.  The bias is
    part of the normalised tensor here, as in torch: the running mean counts it"""
    i, j = pre
    w, b = P[i + ".weight"], P[i + ".bias"]
    z = F.conv2d(x, q(w) if bf16_conv else w, None, padding=1)
    if train and bf16_conv:
        z = q(z)
    z = z + b.view(1, -1, 1, 1)
    rm, rv = P[j + ".running_mean"].clone(), P[j + ".running_var"].clone()
    y = torch.relu(F.batch_norm(z, rm, rv, P[j + ".weight"], P[j + ".bias"], training=train, eps=1e-5))
    if _RUNNING is not None:
        _RUNNING[j + ".running_mean"], _RUNNING[j + ".running_var"] = rm, rv
    return q(y)


def _double_conv(P, pre, x, q, train, stem=False):
    x = _cbr(P, (pre + "double_conv.0", pre + "double_conv.1"), x, q, train, bf16_conv=not stem)
    return _cbr(P, (pre + "double_conv.3", pre + "double_conv.4"), x, q, train)


def _down(P, pre, x, q, train):
    return _double_conv(P, pre + "maxpool_conv.1.", F.max_pool2d(x, 2), q, train)


def _up(P, pre, x1, x2, q, train):
    return _double_conv(P, pre + "conv.", q(_up_ref(x1, x2)), q, train)


def _unet(P, x, q, train):
    x1 = _double_conv(P, "inc.", x, q, train, stem=True)
    x2 = _down(P, "down1.", x1, q, train)
    x3 = _down(P, "down2.", x2, q, train)
    x4 = _down(P, "down3.", x3, q, train)
    x5 = _down(P, "down4.", x4, q, train)
    y = _up(P, "up1.", x5, x4, q, train)
    y = _up(P, "up2.", y, x3, q, train)
    y = _up(P, "up3.", y, x2, q, train)
    y = _up(P, "up4.", y, x1, q, train)
    return F.conv2d(y, P["outc.conv.weight"], P["outc.conv.bias"])


def _params64(module):
    return {k: (v.detach().cpu().double().requires_grad_(v.dtype.is_floating_point and "running" not in k)) for k, v in module.state_dict().items()}


def _rel(a, ref):
    return float((a.double() - ref).norm() / ref.norm().clamp_min(1e-300))


def _adjudicate(title, tensors):
    """tensors: name -> (gpu, emulation, float64).  Each gpu tensor within 3 x the emulation's own relative L2 error against float64"""
    print(f"\n{title}: relative L2 against float64 -- emulation, bf16 kernels, ratio")
    bad = []
    for name, (got, emu, ref) in tensors.items():
        e_emu, e_gpu = _rel(emu.detach(), ref.detach()), _rel(got.detach().cpu(), ref.detach())
        print(f"  {name:44s} {e_emu:.3e} {e_gpu:.3e} {e_gpu / max(e_emu, 1e-300):.2f}")
        if not e_gpu <= 3 * e_emu:
            bad.append(name)
    assert not bad, bad


def _block_case(dev, block, run64, inputs, name):
    """train-mode block on bf16 NHWC inputs: output and every gradient (inputs included) against the emulation"""
    block.to(dev).train()
    xs = [t.to(dev).requires_grad_(True) for t in inputs]
    out = block.nhwc(*xs)
    assert out.dtype == BF
    G = torch.randn(out.shape, generator=_gen(20)).to(BF).float()  # bf16 values: the cotangent the kernels see is the one the references see
    (out.float() * G.to(dev)).sum().backward()
    res = {}
    for tag, q in (("f64", _ident), ("emu", _q)):
        P = _params64(block)
        ins = [_nchw64(t).requires_grad_(True) for t in inputs]
        o = run64(P, ins, q)
        (o * _nchw64(G)).sum().backward()
        res[tag] = (o, ins, P)
    tensors = {"output": (out, _nhwc(res["emu"][0]), _nhwc(res["f64"][0]))}
    for i, x in enumerate(xs):
        tensors[f"grad input {i}"] = (x.grad, _nhwc(res["emu"][1][i].grad), _nhwc(res["f64"][1][i].grad))
    zero_bias = []
    for k, p in block.named_parameters():
        if k.endswith(("double_conv.0.bias", "double_conv.3.bias")):  # in front of a batch-statistics BatchNorm: cancels exactly
            assert p.grad is not None and p.grad.dtype == torch.float32 and not bool(p.grad.any()), k
            zero_bias.append(k)
            continue
        tensors["grad " + k] = (p.grad, res["emu"][2][k].grad, res["f64"][2][k].grad)
    assert len(zero_bias) == 2
    _adjudicate(name, tensors)


def test_down_block_train(dev):
    from face_mask_inpaint_amd.modules.unet.unet_parts import Down

    torch.manual_seed(21)
    x = torch.randn(2, 16, 16, 64, generator=_gen(22)).to(BF)
    _block_case(dev, Down(64, 128, compute_dtype=BF), lambda P, ins, q: _down(P, "", ins[0], q, True), [x], "Down(64, 128) on [2,16,16,64]")


def test_up_block_train(dev):
    from face_mask_inpaint_amd.modules.unet.unet_parts import Up

    torch.manual_seed(23)
    x1 = torch.randn(2, 8, 8, 64, generator=_gen(24)).to(BF)
    x2 = torch.randn(2, 16, 16, 64, generator=_gen(25)).to(BF)
    _block_case(dev, Up(128, 64, compute_dtype=BF), lambda P, ins, q: _up(P, "", ins[0], ins[1], q, True), [x1, x2],
                "Up(128, 64) on x1 [2,8,8,64] + skip [2,16,16,64]")


@pytest.fixture(scope="module")
def detector(dev):
    """one seeded bf16 MaskDetector, its fixed input, and the float64 / emulated logits in eval and train mode (computed once)"""
    from face_mask_inpaint_amd.modules.mask_detector import MaskDetector

    torch.manual_seed(31)
    net = MaskDetector(3, compute_dtype=BF)
    gen = _gen(32)
    with torch.no_grad():  # non-trivial running statistics for the eval path
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) * 0.5 + 0.25)
    x = torch.rand(2, 3, 64, 64, generator=gen)
    ref = {}
    with torch.no_grad():
        for train in (False, True):
            for tag, q in (("f64", _ident), ("emu", _q)):
                ref[(train, tag)] = _unet(_params64(net.model), x.double(), q, train)
    return net.to(dev), x, ref


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_whole_model_logits(dev, detector, train):
    net, x, ref = detector
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net.train(train)
    with torch.no_grad():
        logits = net(x.to(dev), "train")
    net.load_state_dict(sd)  # the train-mode forward moved the running statistics: put the shared fixture back
    assert logits.dtype == torch.float32 and logits.shape == (2, 2, 64, 64)
    _adjudicate(f"MaskDetector logits, {'train' if train else 'eval'} mode, 2x3x64x64",
                {"logits": (logits.contiguous(), ref[(train, "emu")], ref[(train, "f64")])})


def test_running_statistics_count_the_convolution_bias(dev):
    """one train-mode forward from the same initialisation on the fp32 and on the bf16 body: the bf16 path leaves the convolution's bias
    out of the tensor it normalises, yet its running mean must be that of conv(x) + bias -- what the fp32 path, torch and every eval
    consumer use.  Both buffers of all 18 BatchNorms against float64: fp32 at its own accuracy, bf16 within 3 x the emulation's error
    (a missing bias is an error of |b| / |mean|, 10 % and more)"""
    global _RUNNING
    from face_mask_inpaint_amd.modules.mask_detector import MaskDetector

    torch.manual_seed(51)
    init = MaskDetector(3).state_dict()
    with torch.no_grad():  # biases large enough to tell apart from rounding in every layer
        for k, v in init.items():
            if k.endswith(("double_conv.0.bias", "double_conv.3.bias")):
                v.copy_(torch.randn(v.shape, generator=_gen(52)) * 0.2)
    x = torch.rand(2, 3, 64, 64, generator=_gen(53))
    got = {}
    for tag, dt in (("fp32", torch.float32), ("bf16", BF)):
        net = MaskDetector(3, compute_dtype=dt)
        net.load_state_dict(init)
        net.to(dev).train()
        with torch.no_grad():
            net(x.to(dev), "train")
        got[tag] = {k[len("model."):]: v.detach().cpu() for k, v in net.state_dict().items() if "running_" in k}
        assert all(int(v) == 1 for k, v in net.state_dict().items() if k.endswith("num_batches_tracked"))
    ref = {}
    P0 = {k[len("model."):]: v for k, v in init.items()}
    for tag, q in (("f64", _ident), ("emu", _q)):
        _RUNNING = {}
        try:
            with torch.no_grad():
                _unet({k: v.double() for k, v in P0.items()}, x.double(), q, True)
            ref[tag] = _RUNNING
        finally:
            _RUNNING = None
    assert sorted(ref["f64"]) == sorted(got["bf16"]) and len(ref["f64"]) == 36
    worst_fp32 = max(_rel(got["fp32"][k], ref["f64"][k]) for k in ref["f64"])
    print(f"\nfp32 body, running statistics against float64: worst relative L2 {worst_fp32:.2e}")
    assert worst_fp32 <= 1e-4
    stem = [k for k in ref["f64"] if k.startswith("inc.double_conv.1.")]  # behind the fp32 stem convolution: nothing is rounded to bf16
    assert len(stem) == 2 and all(_rel(got["bf16"][k], ref["f64"][k]) <= 1e-4 for k in stem)
    _adjudicate("running statistics after one train-mode forward",
                {k: (got["bf16"][k], ref["emu"][k], ref["f64"][k]) for k in sorted(ref["f64"]) if k not in stem})
    bias_of = lambda k: P0[k.replace("1.running_mean", "0.bias").replace("4.running_mean", "3.bias")].double()
    shift = min(_rel(ref["f64"][k] - 0.1 * bias_of(k), ref["f64"][k]) for k in ref["f64"] if k.endswith("running_mean"))
    print(f"  (a running mean without the bias would be off by at least {shift:.2e} of its norm)")


def test_bf16_checkpoint_evaluates_the_same_in_fp32(dev):
    """three bf16 train steps, then the state_dict loaded into an fp32 MaskDetector: both eval-mode logits against float64 of that
    checkpoint -- fp32 at its own accuracy, bf16 within 3 x the emulation's error"""
    from face_mask_inpaint_amd import train_mask_detector as TM
    from face_mask_inpaint_amd.modules.mask_detector import MaskDetector
    from face_mask_inpaint_amd.optim import FusedAdam

    img, masks = _ellipse_batch()
    torch.manual_seed(54)
    net = MaskDetector(3, compute_dtype=BF).to(dev).train()
    opt = FusedAdam(net.parameters(), lr=1e-3)
    for _ in range(3):
        TM.train_step(net, opt, img.to(dev), masks.to(dev))
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    other = MaskDetector(3)
    other.load_state_dict(sd, strict=True)
    other.to(dev).eval()
    net.eval()
    with torch.no_grad():
        lb, lf = net(img.to(dev), "train"), other(img.to(dev), "train")
        P = {k[len("model."):]: v.double() for k, v in sd.items()}
        f64, emu = _unet(P, img.double(), _ident, False), _unet(P, img.double(), _q, False)
    e32 = _rel(lf.cpu().contiguous(), f64)
    print(f"\nfp32 body on the bf16-trained checkpoint, eval logits against float64: {e32:.2e}")
    assert e32 <= 1e-3
    _adjudicate("bf16-trained checkpoint, eval logits", {"logits": (lb.contiguous(), emu, f64)})
    assert torch.equal(net.predict_mask(img.to(dev)).cpu(), lb.cpu().argmax(1).float())


def test_folded_constants_follow_a_train_mode_pass(dev):
    """a frozen block keeps its folded eval constants; a train-mode pass moves the running statistics through raw pointers and must
    drop them"""
    from face_mask_inpaint_amd.modules.pluralistic_model import base_function
    from face_mask_inpaint_amd.modules.unet.unet_parts import DoubleConv

    torch.manual_seed(55)
    blk = DoubleConv(64, 64, compute_dtype=BF).to(dev)
    base_function._freeze(blk)
    x = torch.randn(2, 8, 8, 64, generator=_gen(56)).to(BF).to(dev)
    with torch.no_grad():
        blk.eval()
        y0 = blk.nhwc(x)
        assert torch.equal(_bits(blk.nhwc(x)), _bits(y0)) and blk.double_conv[1]._fmi_fold is not None
        blk.train()
        blk.nhwc(x)
        blk.eval()
        y1 = blk.nhwc(x)
        for m in blk.modules():
            if hasattr(m, "_fmi_fold"):
                object.__setattr__(m, "_fmi_fold", None)
        y2 = blk.nhwc(x)
    assert not torch.equal(_bits(y1), _bits(y0)) and torch.equal(_bits(y1), _bits(y2))


def test_predict_mask_is_the_argmax_of_its_own_logits(dev, detector):
    net, x, _ = detector
    net.eval()
    with torch.no_grad():
        logits = net.model.nhwc(FF.to_nhwc(x.to(dev)))
    assert logits.dtype == torch.float32
    mask = net.predict_mask(x.to(dev))
    assert mask.shape == (2, 64, 64) and torch.equal(mask, FF.argmax_channels(logits))
    assert torch.equal(mask.cpu(), logits.cpu().argmax(-1).float())
    with pytest.raises(FmiError, match="gradients"):  # eval mode with gradients on has no bf16 path
        net.model.nhwc(FF.to_nhwc(x.to(dev)))


def test_sizes_that_are_no_multiple_of_16_are_refused(dev, detector):
    net, _, _ = detector
    with pytest.raises(FmiError, match="16"):
        net.predict_mask(torch.rand(2, 3, 72, 72, device=dev))
    with pytest.raises(FmiError, match="16"):
        net(torch.rand(2, 3, 64, 72, device=dev), "train")


# ---------------------------------------------------------------------------------------------------------------------------------
# trainer and harnesses
# ---------------------------------------------------------------------------------------------------------------------------------
def _ellipse_batch():
    yy, xx = torch.meshgrid(torch.arange(64.0), torch.arange(64.0), indexing="ij")
    masks = torch.stack([(((yy - 36) / 14) ** 2 + ((xx - 30) / 20) ** 2 <= 1), (((yy - 24) / 18) ** 2 + ((xx - 40) / 11) ** 2 <= 1)]).long()
    img = torch.rand(2, 3, 64, 64, generator=_gen(41)) * 0.5
    img = img + 0.4 * masks.unsqueeze(1).float() * torch.tensor([0.2, 0.6, 1.0]).view(1, 3, 1, 1)
    return img, masks


def test_overfit_one_batch_bf16_against_fp32(dev):
    """20 steps of FusedAdam(lr = 1e-3) on one fixed batch from the same initialisation: the bf16 body must achieve at least three
    quarters of the fp32 run's loss decrease"""
    from face_mask_inpaint_amd import train_mask_detector as TM
    from face_mask_inpaint_amd.modules.mask_detector import MaskDetector
    from face_mask_inpaint_amd.optim import FusedAdam

    img, masks = _ellipse_batch()
    torch.manual_seed(42)
    init = MaskDetector(3).state_dict()
    curves = {}
    for tag, dt in (("fp32", torch.float32), ("bf16", BF)):
        net = MaskDetector(3, compute_dtype=dt)
        net.load_state_dict(init)
        net.to(dev).train()
        opt = FusedAdam(net.parameters(), lr=1e-3)
        losses = [TM.train_step(net, opt, img.to(dev), masks.to(dev)) for _ in range(20)]
        curves[tag] = torch.stack(losses).tolist()
        assert all(p.grad is not None for p in net.parameters()), tag  # the bias in front of a BatchNorm keeps its (zero) gradient
    for tag, c in curves.items():
        print(f"\n{tag}: " + " ".join(f"{v:.4f}" for v in c))
    dec = {tag: c[0] - c[-1] for tag, c in curves.items()}
    print(f"loss decrease: fp32 {dec['fp32']:.4f}, bf16 {dec['bf16']:.4f}, ratio {dec['bf16'] / dec['fp32']:.3f}")
    assert dec["fp32"] > 0 and dec["bf16"] >= 0.75 * dec["fp32"]


def test_train_net_bf16_one_epoch(dev, tmp_path):
    """train_net(dtype='bf16') on the golden image set of the existing trainer test, each 40 x 48 pair cropped to 32 x 48 (the bf16 body
    needs multiples of 16): the checkpoint it writes loads into an fp32 MaskDetector"""
    import numpy as np
    from PIL import Image

    from face_mask_inpaint_amd import train_mask_detector as TM
    from face_mask_inpaint_amd.modules.mask_detector import MaskDetector

    src = os.path.join(ROOT, "tests", "golden", "dataset")
    img, msk, ckpt = tmp_path / "images_masked", tmp_path / "binary_map", tmp_path / "ckpt"
    img.mkdir(), msk.mkdir()
    ids = sorted(f.split("_")[0] for f in os.listdir(os.path.join(src, "images_masked")))
    for i in ids:
        im = Image.open(os.path.join(src, "images_masked", i + "_surgical.jpg")).convert("RGB")
        m = np.load(os.path.join(src, "binary_map", i + ".npy"))
        w16, h16 = im.size[0] // 16 * 16, im.size[1] // 16 * 16
        for r in range(3):  # 24 items as in the fp32 trainer test: 20 to train on, 4 to validate, a validation round after every step
            im.crop((0, 0, w16, h16)).save(img / f"{r + 2}{i}_surgical.jpg", quality=95)
            np.save(msk / f"{r + 2}{i}.npy", np.ascontiguousarray(m[:h16, :w16]))
    torch.manual_seed(43)
    net = MaskDetector(3).to(dev)  # an fp32 model: train_net puts it on the bf16 body
    keys = list(net.state_dict())
    hist = TM.train_net(net, dev, epochs=1, batch_size=2, learning_rate=1e-4, val_percent=1 / 6, save_checkpoint=True, img_scale=1.0,
                        dir_img=img, dir_mask=msk, dir_checkpoint=ckpt, seed=7, dtype="bf16")
    assert net.compute_dtype == BF and net.model.compute_dtype == BF
    assert hist["n_train"] == 20 and hist["n_val"] == 4 and len(hist["val_scores"]) == 10 and all(0.0 <= v <= 1.0 for v in hist["val_scores"])
    assert len(hist["losses"]) == 10 and all(v == v and abs(v) != float("inf") for v in hist["losses"])
    assert [os.path.basename(p) for p in hist["checkpoints"]] == ["checkpoint_epoch1.pth"]
    sd = torch.load(hist["checkpoints"][0], weights_only=True)
    assert list(sd) == keys and all(v.dtype in (torch.float32, torch.int64) for v in sd.values())
    MaskDetector(3).load_state_dict(sd, strict=True)
    print("\ntrain_net(dtype='bf16'): losses " + " ".join(f"{v:.4f}" for v in hist["losses"]) + f"; validation {hist['val_scores']}")


def _count_calls(monkeypatch, name):
    calls = []
    real = getattr(FF, name)

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(FF, name, counted)
    return calls


def test_picnet_harness_with_the_bf16_detector(dev, tmp_path, monkeypatch):
    from face_mask_inpaint_amd import PICNet_inference as PI

    calls = _count_calls(monkeypatch, "head1x1_argmax")
    o = str(tmp_path / "out")
    s = PI.main(["--num_batches", "1", "--batch_size", "1", "--mask_detector_dtype", "bf16", "--out_dir", o])
    assert s == s and -1.0 <= s <= 1.0 and len(calls) == 1
    assert os.listdir(o) == ["metrics.csv"]
    with open(os.path.join(o, "metrics.csv")) as fh:
        rows = [r.strip().split(",") for r in fh if r.strip()]
    assert rows[0] == ["ssim", "ms_ssim"] and float(rows[1][0]) == s


def test_psp_harness_with_the_bf16_detector(dev, tmp_path, monkeypatch):
    from face_mask_inpaint_amd import psp_inference as PI

    calls = _count_calls(monkeypatch, "head1x1_argmax")
    o = str(tmp_path / "out")
    s, m = PI.main(["--batch_size", "1", "--num_batches", "1", "--use_ref", "--output_size", "256", "--mask_detector_dtype", "bf16", "--out_dir", o])
    assert s == s and m == m and len(calls) == 1
    assert sorted(os.listdir(o)) == ["gen_0.jpg", "metrics.csv"]
    _, md = PI.build(PI.get_args(["--output_size", "256", "--mask_detector_dtype", "bf16"]), dev)
    assert md.compute_dtype == BF and not md.training and not any(p.requires_grad for p in md.parameters())
