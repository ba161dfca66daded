"""cmp_chan.py <cand.so> <ref.so>: every entry whose kernels went through csrc/bf16x8.h, chan.hip and sum_parts.h, forward and backward, under
two builds of the library on identical inputs; every output and gradient must be torch.equal.  Entries that accumulate with atomics
run in the reproducible mode only (`det`), the others in both modes.  Exit status 1 on any difference."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from face_mask_inpaint_amd import functional as FF, _lib  # noqa: E402
from face_mask_inpaint_amd.modules.psp.stylegan2.op.fused_act import fused_leaky_relu  # noqa: E402
from face_mask_inpaint_amd.modules.psp.stylegan2.op.upfirdn2d import upfirdn2d  # noqa: E402

dev = torch.device("cuda:0")
libs = [_lib.Library(sys.argv[1]), _lib.Library(sys.argv[2])]
gen = torch.Generator().manual_seed(0)
F32, BF16 = torch.float32, torch.bfloat16
bad = ran = 0


def rn(*shape, dtype=F32, grad=True, scale=1.0):
    t = (torch.randn(*shape, generator=gen) * scale).to(dtype)
    t.want_grad = grad
    return t


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16) if a.dtype == BF16 else a, b.view(torch.int16) if b.dtype == BF16 else b)


def case(name, fn, *xs, det=False):
    """fn(*tensors on the device) -> tensor(s); det: the entry uses atomics outside the reproducible mode"""
    global bad, ran
    for mode in ((True,) if det else (False, True)):
        res = []
        try:
            for lib in libs:
                _lib._LIB = lib
                with FF.deterministic(mode):
                    ins = [x.to(dev).requires_grad_(x.want_grad) for x in xs]
                    out = fn(*ins)
                    outs = [o for o in (out if isinstance(out, (tuple, list)) else [out]) if o is not None]
                    diff = [o for o in outs if o.requires_grad]
                    if diff:
                        cot = [torch.linspace(-1.0, 1.0, o.numel(), device=dev).view(o.shape).to(o.dtype) for o in diff]
                        torch.autograd.backward(diff, cot)
                    torch.cuda.synchronize()
                    res.append([o.detach() for o in outs] + [i.grad for i in ins if i.grad is not None])
        except (FF.FmiError, TypeError, ValueError, ctypes.ArgumentError) as e:  # a refusal is a finding of this tool, not a fault
            bad += 1
            print(f"ERROR {name} det={mode}: {type(e).__name__}: {e}")
            continue
        ok = len(res[0]) == len(res[1]) and all(same(a, b) for a, b in zip(*res))
        ran += 1
        bad += not ok
        print(f"{'ok  ' if ok else 'DIFF'} {name} det={mode}: {len(res[0])} tensors")


def pack(w):
    k, c, kh, kw = w.shape
    wf = w.permute(2, 3, 1, 0).reshape(kh * kw, c, k).contiguous()
    wt = w.permute(2, 3, 0, 1).reshape(kh * kw, k, c).contiguous()
    return wf, wt, c, kh, kw


# ---- the five per-channel families, both types, both kernels of each entry ----
for dt, tag in ((F32, "f32"), (BF16, "bf16")):
    wide = 4 if dt == F32 else 8
    odd = 6 if dt == F32 else 12  # no whole chunks: the one-element kernels
    for n, p, c in [(2, 3, wide), (3, 252, 64), (2, 37, odd), (3, 9000, 8), (16, 64 * 64, 128)]:
        s = f"{tag} N{n} P{p} C{c}"
        case(f"scale_channels {s}", FF.scale_channels, rn(n, p, c, dtype=dt), rn(n, c))
        case(f"scale_channels s-only {s}", FF.scale_channels, rn(n, p, c, dtype=dt, grad=False), rn(n, c))
        case(f"scale_channels_add {s}", FF.scale_channels_add, rn(n, p, c, dtype=dt), rn(n, c), rn(n, p, c, dtype=dt))
    for rows, c in [(3, wide), (300, odd), (7232, 64), (16 * 64 * 64, 128)]:
        if dt == BF16 and c % 8:
            continue  # the bf16 PReLU has no one-element form
        case(f"prelu {tag} rows{rows} C{c}", FF.prelu, rn(rows, c, dtype=dt), rn(c), det=bool(c % 4))
    pool = FF.global_avg_pool_pass if dt == F32 else FF.global_avg_pool_pass_bf16
    for shape in [(2, 16, 16, 64), (3, 8, 8, 512), (16, 64, 64, 128)]:
        case(f"global pool pass {tag} {shape}", pool, rn(*shape, dtype=dt), det=dt == F32)  # pool.hip's fp32 pool adds with atomics
    for shape in [(2, 7, 9, wide), (2, 7, 9, odd), (1, 10, 7, 64), (16, 64, 64, 128)]:
        if dt == BF16 and shape[3] % 8:
            continue
        for stride in (2, 3):
            case(f"subsample {tag} {shape} s{stride}", lambda x, st=stride: FF.subsample(x, st), rn(*shape, dtype=dt))
for shape in [(1, 5, 12), (2, 3, 8), (16, 64, 64, 128)]:
    case(f"add bf16 {shape}", FF.add, rn(*shape, dtype=BF16), rn(*shape, dtype=BF16))

# ---- the norms (sum_parts_kernel<double>, nld4 / nst4) ----
for dt, tag in ((F32, "f32"), (BF16, "bf16")):
    for shape, groups in [((2, 33, 31, 64), 1), ((2, 64, 113, 8), 2), ((16, 64, 64, 128), 1)]:
        for pt in (False, True):
            case(f"batch_norm {tag} {shape} groups{groups} pass{pt}", lambda x, g, b, gr=groups, p=pt: FF.batch_norm_train(x, g, b, 1e-5, gr, p, 0.2),
                 rn(*shape, dtype=dt), rn(shape[3]), rn(shape[3]), det=True)
case("instance_norm_act f32", lambda x, g, b: FF.instance_norm_act(x, g, b, 1e-5, 0.2), rn(2, 33, 31, 64), rn(64), rn(64), det=True)
case("instance_norm_act bf16", lambda x, g, b: FF.instance_norm_act_bf16(x, g, b, 1e-5, 0.2), rn(2, 33, 31, 64, dtype=BF16, grad=False),
     rn(64, grad=False), rn(64, grad=False))

# ---- the entries that take a caller's tensor (bf_st_nan) and the decoder's bandwidth kernels ----
k1 = torch.tensor([1.0, 3.0, 3.0, 1.0])
k2 = (k1[:, None] * k1[None, :]) / k1.sum() ** 2
k2.want_grad = False
for dt, tag in ((F32, "f32"), (BF16, "bf16")):
    for shape in [(2, 8, 9, 9), (2, 16, 16, 16)]:
        case(f"fused_leaky_relu {tag} {shape}", fused_leaky_relu, rn(*shape, dtype=dt), rn(shape[1], dtype=dt), det=True)
    for up, down, pad in [(1, 1, (2, 1)), (2, 1, (2, 1)), (1, 2, (1, 1))]:
        case(f"upfirdn2d {tag} up{up} down{down}", lambda x, k, u=up, d=down, p=pad: upfirdn2d(x, k * u * u, u, d, p), rn(2, 8, 17, 20, dtype=dt), k2)
        if dt == BF16 and (up, down) != (1, 1):
            continue  # the bf16 NHWC filter is the decoder's Blur only
        case(f"upfirdn2d_nhwc {tag} up{up} down{down}", lambda x, k, u=up, d=down, p=pad: FF.upfirdn2d_nhwc(x, k * u * u, u, d, p, True),
             rn(2, 17, 20, 32, dtype=dt), k2)
    case(f"noise_bias_act {tag}", FF.noise_bias_act, rn(2, 16, 16, 32, dtype=dt), rn(32), rn(2, 16, 16, 1, grad=False), rn(1), det=True)
case("blur_act bf16", lambda u, k, d, nz, nw, b: FF.blur_act(u, k, (2, 1), d, nz, nw, b, 0.2, 2 ** 0.5), rn(2, 17, 17, 32, dtype=BF16), k2, rn(2, 32),
     rn(2, 17, 17, 1, grad=False), rn(1), rn(32), det=True)

# ---- the UNet body ----
case("max_pool2 bf16", FF.max_pool2, rn(2, 8, 12, 16, dtype=BF16))
case("up2_cat bf16", FF.up2_cat, rn(2, 4, 5, 16, dtype=BF16), rn(2, 9, 11, 8, dtype=BF16))
case("head1x1 bf16", FF.head1x1, rn(2, 8, 12, 16, dtype=BF16), rn(2, 16), rn(2), det=True)

# ---- the bf16 convolutions, the thin Output forward and the fused attention ----
for n, h, w, c, k, stride in [(2, 16, 16, 32, 64, 1), (2, 17, 19, 64, 32, 2)]:
    wgt = rn(k, c, 3, 3, scale=0.1)

    def conv(x, wg, st=stride):
        wf, wt, cc, kh, kw = pack(wg)
        return FF.conv2d(x, FF.PackedWeight(wf, wt, 9 * cc, cc, kh, kw), stride=st, pad=1)

    case(f"conv2d bf16 {n}x{h}x{w} {c}->{k} s{stride}", conv, rn(n, h, w, c, dtype=BF16), wgt, det=True)
for stride in (1, 2):
    case(f"conv2d_chan bf16 s{stride}", lambda x, wnk, sc, b, sl, st=stride: FF.conv2d_chan_bf16(x, wnk, 3, 3, st, 1, scale=sc, bias=b, slope=sl, colsum=True)[0],
         rn(2, 32, 32, 64, dtype=BF16, grad=False), rn(64, 9, 64, dtype=BF16, grad=False, scale=0.05), rn(64, grad=False), rn(64, grad=False), rn(64, grad=False))
case("thin Output bf16", lambda x, wf, b: FF.lrelu_conv2d_thin_bf16(x, FF.PackedWeight(wf, None, 3, 32, 3, 3), b, 0.1, 1, FF.ACT_TANH),
     rn(2, 9, 35, 32, dtype=BF16, grad=False), rn(9, 32, 3, grad=False, scale=0.08), rn(3, grad=False))
for d, c in ((32, 128), (64, 256)):
    case(f"attention_fwd bf16 d{d} C{c}", FF.self_attention_bf16, rn(2, 256, d, dtype=BF16, grad=False, scale=0.3), rn(2, 256, c, dtype=BF16, grad=False),
         rn(1, grad=False), rn(2, 256, c, dtype=BF16, grad=False))

print(f"{'BAD' if bad else 'OK'}: {ran} runs, {bad} differ or failed")
sys.exit(1 if bad else 0)
