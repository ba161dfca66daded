"""vgg_bf16_time.py [--batch 24] [--size 224] [--pairs 5] [--layers] [--f32]: the VGG16 trunk of VGGLoss as the reference-fill step runs it --
forward and input-gradient chain of the gradient batch plus the forward of an equal target batch without gradient -- on the fp32 trunk
and on the bf16 trunk (VGGLoss(feature_dtype=torch.bfloat16)), in ONE process, in alternating pairs, timed with device events.  The loss
terms are left out: fixed random gradients enter at the four taps.  Then one profiled pass of each prints the per-launch times and TFLOP/s.
--f32: the three forms of the fp32 trunk instead -- composed (VGGLoss._block: pool, cat, add, un-pool, ReLU mask and split passes of their
own), the one-node trunk FF.vgg_trunk_f32 with x and y in launches of their own, and with both in one launch per layer -- with the tap
gradient as the step delivers it: three batch slices per tap, the third (contextual) only at the last tap.
--layers: every bf16 forward convolution of the trunk on each of its two one-launch entries (fmi_conv2d_fwd_act_bf16,
fmi_conv2d_fwd_chan_bf16), the measurement behind functional._vgg_fwd_entry."""
import argparse
import collections
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from face_mask_inpaint_amd import functional as FF  # noqa: E402
from face_mask_inpaint_amd.modules.loss import VGGLoss  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=24)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--layers", action="store_true")
ap.add_argument("--f32", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(0)
mods = {"fp32": VGGLoss(feature_dtype=torch.float32).to(dev), "bf16": VGGLoss(feature_dtype=torch.bfloat16).to(dev)}
mods["bf16"].load_state_dict(mods["fp32"].state_dict())
n, s = args.batch, args.size
x0 = torch.randn(n, s, s, 3, device=dev)
y0 = torch.randn(n, s, s, 3, device=dev)
gtaps = [torch.randn(n, s >> i, s >> i, c, device=dev) / (n * (s >> i) ** 2 * c) for i, c in enumerate((64, 128, 256, 512))]


def taps_of(v, x):
    if v.feature_dtype == torch.bfloat16:
        return FF.vgg_trunk_bf16(x, v._cache["packs16"])
    out = []
    for i in range(len(v.blocks)):
        x = v._block(i, x)
        out.append(x)
    return out


def step(v):
    v._prepare()
    x = x0.detach().requires_grad_(True)
    torch.autograd.backward(taps_of(v, x), gtaps)
    with torch.no_grad():
        taps_of(v, y0)
    return x.grad


def timed(fn, reps=3):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


if args.layers:
    shapes = [(64, 64, s), (64, 128, s // 2), (128, 128, s // 2), (128, 256, s // 4), (256, 256, s // 4), (256, 512, s // 8), (512, 512, s // 8)]
    print(f"bf16 forward convolution + bias + ReLU, batch {n}: ms (TFLOP/s) per entry, three alternated rounds")
    for c, k, h in shapes:
        xh = torch.randn(n, h, h, c, device=dev).bfloat16()
        wnk = (torch.randn(k, 9, c, device=dev) / (9 * c) ** 0.5).bfloat16()
        bias, zs = torch.randn(k, device=dev), torch.zeros(k, device=dev)
        d, y, _ = FF._conv_fwd_bf16_pre(xh, k, 3, 3, 1, 1)
        L, p, st = FF._L(), FF._p, FF._st()
        fns = {"act": lambda: L.conv2d_fwd_act_bf16(C.byref(d), p(xh), p(wnk), None, None, None, p(bias), 0.0, 1.0, p(y), st),
               "chan": lambda: L.conv2d_fwd_chan_bf16(C.byref(d), p(xh), p(wnk), None, p(bias), p(zs), p(y), None, 0, st)}
        fl = 2.0 * n * h * h * k * c * 9
        for f in fns.values():
            timed(f, 3)
        rounds = [{nm: timed(f, 10) for nm, f in fns.items()} for _ in range(3)]
        print(f"  {c:3d} -> {k:3d} at {h:3d}^2: " + "   ".join(
            f"{nm} " + " ".join(f"{r[nm]:.3f}" for r in rounds) + f" ms ({fl / min(r[nm] for r in rounds) / 1e9:.0f})" for nm in fns)
            + f"   chosen: {FF._vgg_fwd_entry(c, k)}")
    sys.exit(0)

def profiled(nm, fn):
    FF.PROFILE = []
    fn()
    torch.cuda.synchronize()
    agg = collections.OrderedDict()
    for tag, flops, a, b in FF.PROFILE:
        t = agg.setdefault(tag, [0, 0.0, 0.0])
        t[0] += 1
        t[1] += a.elapsed_time(b)
        t[2] += flops
    FF.PROFILE = None
    print(f"{nm}: profiled launches (events around each launch: sums exceed the step time)")
    for tag, (cnt, ms, fl) in agg.items():
        print(f"  {cnt:2d} x {tag:58s} {ms:8.3f} ms" + (f" {fl / ms / 1e9:7.0f} TFLOP/s" if fl else ""))
    print(f"  total {sum(t[1] for t in agg.values()):.3f} ms in {sum(t[0] for t in agg.values())} profiled launches")


if args.f32:
    from torch import nn

    v = mods["fp32"]
    v._prepare()
    convs = [(pw, m.bias) for pw, m in zip(v._cache["pws"], [m for bl in v.blocks for m in bl if isinstance(m, nn.Conv2d)])]
    gsl = [g.split(n // 3, 0) for g in gtaps]
    live = [(i, j) for i in range(4) for j in range(3) if j < 2 or i == 3]  # the contextual slice has a gradient at the last tap only

    def step32(form):
        x = x0.detach().requires_grad_(True)
        if form == "composed":
            xs = [t.split(n // 3, 0) for t in taps_of(v, x)]
        else:
            xs = FF.vgg_trunk_f32(x, y0, convs, nslice=3, merge=form == "merged")[0]
        torch.autograd.backward([xs[i][j] for i, j in live], [gsl[i][j] for i, j in live])
        if form == "composed":
            with torch.no_grad():
                taps_of(v, y0)
        return x.grad

    forms = ("composed", "unmerged", "merged")
    ref = None
    for f in forms:
        for _ in range(2):
            g = step32(f)
        ref = g if ref is None else ref
        print(f"{f}: image gradient against composed: max|diff| {float((g - ref).abs().max()):.3e} of {float(ref.abs().max()):.3e}")
    print(f"fp32 VGG16 trunk, gradient batch {n} x {s} x {s} forward + backward, target batch {n} forward; ms per step, {args.pairs} alternated rounds")
    rows = []
    for i in range(args.pairs):
        rows.append([timed(lambda f=f: step32(f)) for f in forms])
        print(f"  round {i}: " + "   ".join(f"{f} {t:.3f}" for f, t in zip(forms, rows[-1])))
    for k, f in enumerate(forms):
        col = [r[k] for r in rows]
        print(f"  {f}: {min(col):.3f} .. {max(col):.3f} (max - min {max(col) - min(col):.3f})")
    for f in forms:
        profiled(f, lambda f=f: step32(f))
    sys.exit(0)

for nm, v in mods.items():  # warm-up: packs, allocator pools
    for _ in range(2):
        g = step(v)
    assert bool(torch.isfinite(g).all()), nm
print(f"VGG16 trunk, gradient batch {n} x {s} x {s} forward + backward, target batch {n} forward; ms per step, {args.pairs} alternated pairs")
rows = []
for i in range(args.pairs):
    rows.append((timed(lambda: step(mods["fp32"])), timed(lambda: step(mods["bf16"]))))
    print(f"  pair {i}: fp32 {rows[-1][0]:.3f}   bf16 {rows[-1][1]:.3f}   fp32 / bf16 {rows[-1][0] / rows[-1][1]:.2f}")
f32, b16 = [r[0] for r in rows], [r[1] for r in rows]
print(f"  fp32 {min(f32):.3f} .. {max(f32):.3f}   bf16 {min(b16):.3f} .. {max(b16):.3f}   bf16 faster in {sum(a > b for a, b in rows)} of {len(rows)} pairs")
gx32, gx16 = step(mods["fp32"]).double(), step(mods["bf16"]).double()
print(f"  image gradient, bf16 against fp32: relative L2 {float((gx16 - gx32).norm() / gx32.norm()):.3e}")
for nm, v in mods.items():
    profiled(nm, lambda v=v: step(v))
