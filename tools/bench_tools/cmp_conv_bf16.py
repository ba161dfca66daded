"""cmp_conv_bf16.py <cand.so> <ref.so>: every entry of the bf16 convolution family (csrc/conv_bf16.hip and the grouped tile path of
style_heads_bf16.hip) and the Python forward wrappers that share _conv_fwd_bf16_pre, under two builds of the library on identical inputs;
every output must be torch.equal on the raw bits.  The shapes take each branch of the host set-up (the tables of csrc/conv_bf16_plan.h, plain and
grouped, the adjoint's phases) and each output stage of conv_bf16_kernel.  The weight gradient and the split reduction accumulate
with atomics outside the reproducible mode: they run in that mode only.  A refusal (FmiError) is reported; where one is expected both
builds must refuse alike.  Exit status 1 on any difference.  Either build may lack entries the other has (an older library next to a newer
one): only the entries the cases call are needed."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from face_mask_inpaint_amd import functional as FF, _lib  # noqa: E402

dev = torch.device("cuda:0")
libs = [_lib.Library(sys.argv[1], strict=False), _lib.Library(sys.argv[2], strict=False)]
gen = torch.Generator().manual_seed(0)
F32, BF16 = torch.float32, torch.bfloat16
bad = ran = 0


def rn(*shape, dtype=F32, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=gen) * scale + shift).to(dtype)


def bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def nan(shape, dtype=BF16):
    return torch.full(shape, float("nan"), device=dev, dtype=dtype)  # a row the kernel leaves unwritten shows


def case(name, fn, *xs, det=False, may_refuse=False, tile=None):
    """fn(lib, *tensors on the device) -> tensor(s).  det: reproducible mode; tile: fmi_debug_bf16_tile mode for the call"""
    global bad, ran
    res = []
    for lib in libs:
        _lib._LIB = lib
        prev = lib.debug_bf16_tile(tile) if tile is not None else None
        try:
            with FF.deterministic(det), torch.no_grad():
                out = fn(lib, *[None if x is None else x.to(dev) for x in xs])
                torch.cuda.synchronize()
            res.append([o for o in (out if isinstance(out, (tuple, list)) else [out]) if o is not None])
        except (FF.FmiError, TypeError, ValueError, C.ArgumentError) as e:
            res.append(f"{type(e).__name__}: {e}")
        finally:
            if prev is not None:
                lib.debug_bf16_tile(prev)
    ran += 1
    tag = f"{name}{' det' if det else ''}{'' if tile is None else f' tile-mode {tile}'}"
    if isinstance(res[0], str) or isinstance(res[1], str):
        ok = may_refuse and res[0] == res[1]
        bad += not ok
        print(f"{'ok  ' if ok else 'ERROR'} {tag}: " + (f"both refuse alike: {res[0]}" if res[0] == res[1] else f"cand: {res[0] if isinstance(res[0], str) else 'ran'} / "
                                                      f"ref: {res[1] if isinstance(res[1], str) else 'ran'}"))
        return
    ok = len(res[0]) == len(res[1]) and all(same(a, b) for a, b in zip(*res))
    bad += not ok
    print(f"{'ok  ' if ok else 'DIFF'} {tag}: {len(res[0])} tensors, {sum(o.numel() // o.shape[-1] for o in res[0])} rows")


def desc(n, h, w, c, k, ks, stride, pad):
    return FF.conv_desc(n, h, w, c, k, ks, ks, stride, pad)


def wpack(k, taps, c):
    return rn(k, taps, c, dtype=BF16, scale=(taps * c) ** -0.5)


p, st = FF._p, FF._st


# ---- fmi_conv2d_fwd_bf16: one case per branch of the plain table of conv_bf16_plan.h ----
def fwd(n, h, w, c, k, ks, stride, pad, colscale=False, split=False):
    def run(lib, x, wnk, cs):
        d, oh, ow = desc(n, h, w, c, k, ks, stride, pad)
        y = nan((n, oh, ow, k))
        ws = torch.zeros(y.numel(), device=dev) if split else None
        lib.conv2d_fwd_bf16(C.byref(d), p(x), p(wnk), p(cs), p(y), p(ws), 0 if ws is None else ws.numel(), st())
        return y
    return run, rn(n, h, w, c, dtype=BF16), wpack(k, ks * ks, c), (rn(n, k, scale=0.2, shift=1.0) if colscale else None)


FWD = [("a 128x32 BK32", (1, 40, 40, 32, 32, 3, 1, 1)), ("b 128x64", (1, 224, 224, 32, 64, 3, 1, 1)), ("c 64x64", (1, 40, 40, 32, 64, 3, 1, 1)),
       ("d 128x128", (1, 256, 256, 64, 128, 1, 1, 0)), ("e 64x128", (1, 128, 128, 64, 128, 3, 1, 1)), ("f 256x256 eight-phase", (1, 256, 256, 64, 256, 1, 1, 0)),
       ("g odd, partial tiles", (2, 9, 7, 64, 128, 3, 2, 1))]
for tag, g in FWD:
    case(f"fwd {tag} {g}", *fwd(*g))
case(f"fwd f 256x256 four-wave {FWD[5][1]}", *fwd(*FWD[5][1]), tile=2)
gh = (1, 40, 40, 64, 40, 3, 1, 1)
for lib in libs:
    print(f"     fmi_conv2d_bf16_supported(64 -> 40) = {lib.conv2d_bf16_supported(C.byref(desc(*gh)[0]))}  [{os.path.basename(os.path.dirname(lib.path)) or lib.path}]")
case(f"fwd h K % 32 != 0 {gh}", *fwd(*gh), may_refuse=True)
case("fwd colscale N=2 64->128 32x32 k3", *fwd(2, 32, 32, 64, 128, 3, 1, 1, colscale=True))
case("fwd split workspace 512->512 8x8 k3", *fwd(2, 8, 8, 512, 512, 3, 1, 1, split=True), det=True)


# ---- fmi_conv2d_fwd_act_bf16 (the eight-phase kernel's output stage) and the eight-phase kernel forced ----
def act(n, h, w, c, k, noise, slope, gain):
    def run(lib, x, wnk, cs, nz, nw, b):
        d, oh, ow = desc(n, h, w, c, k, 3, 1, 1)
        y = nan((n, oh, ow, k))
        lib.conv2d_fwd_act_bf16(C.byref(d), p(x), p(wnk), p(cs), p(nz), p(nw), p(b), slope, gain, p(y), st())
        return y
    return (run, rn(n, h, w, c, dtype=BF16), wpack(k, 9, c), rn(n, k, scale=0.2, shift=1.0), rn(n, h, w, 1) if noise else None,
            rn(1) if noise else None, rn(k))


case("fwd_act UNet form 64->64 2x32x32 bias + colscale", *act(2, 32, 32, 64, 64, False, 0.0, 1.0))
case("fwd_act StyledConv form 64->128 2x32x32 noise", *act(2, 32, 32, 64, 128, True, 0.2, 2 ** 0.5))
case("fwd eight-phase forced 64->128 2x32x32 k3", *fwd(2, 32, 32, 64, 128, 3, 1, 1), tile=8)
case("fwd eight-phase forced + colscale", *fwd(2, 32, 32, 64, 128, 3, 1, 1, colscale=True), tile=8)


# ---- fmi_conv2d_fwd_chan_bf16 ----
def chan(n, h, w, c, k, ks, stride, pad, vecs, colsum):
    def run(lib, x, wnk, sc, b, sl):
        d, oh, ow = desc(n, h, w, c, k, ks, stride, pad)
        y = nan((n, oh, ow, k))
        rows = -(-(n * oh * ow) // FF.CHAN_COLSUM_ROWS)
        part = nan((rows, 2, k), F32) if colsum else None
        lib.conv2d_fwd_chan_bf16(C.byref(d), p(x), p(wnk), p(sc), p(b), p(sl), p(y), p(part), 0 if part is None else part.numel(), st())
        return y, part
    return (run, rn(n, h, w, c, dtype=BF16), wpack(k, ks * ks, c), rn(k, scale=0.2, shift=1.0) if vecs else None, rn(k) if vecs else None,
            rn(k, scale=0.3) if vecs else None)


for k in (64, 128):
    for ks, stride, pad in ((3, 1, 1), (3, 2, 1), (1, 2, 0)):
        for vecs in (False, True):
            case(f"fwd_chan 64->{k} 2x48x48 k{ks}s{stride} {'scale bias slope' if vecs else 'bare'}", *chan(2, 48, 48, 64, k, ks, stride, pad, vecs, False))
    case(f"fwd_chan 64->{k} colsum N=2 12x12 (a tile straddles the samples)", *chan(2, 12, 12, 64, k, 3, 1, 1, True, True))
    case(f"fwd_chan 64->{k} colsum 2x48x48 k3s2", *chan(2, 48, 48, 64, k, 3, 2, 1, True, True))
case("fwd_chan colsum 8x8 (fewer than 128 pixels)", *chan(2, 8, 8, 64, 64, 3, 1, 1, True, True), may_refuse=True)


# ---- fmi_conv2d_grouped_fwd_bf16: one case per branch of the grouped table, shared and per-group maps ----
def grouped(g, n, h, w, c, k, ks, stride, pad, shared):
    def run(lib, x, wnk, b):
        return FF.conv2d_grouped_bf16(x, wnk, b, ks, stride, pad, 0.01, shared)
    return run, rn(n, h, w, c if shared else g * c, dtype=BF16), rn(g, k, ks * ks, c, dtype=BF16, scale=(ks * ks * c) ** -0.5), rn(g, k)


GROUPED = [("256x256", (4, 2, 80, 80, 64, 256, 1, 1, 0)), ("128x128", (2, 2, 128, 128, 64, 128, 1, 1, 0)), ("64x128 / 64x64 by workgroups", (2, 1, 96, 96, 64, 128, 3, 2, 1)),
           ("64x128", (2, 1, 192, 192, 64, 128, 3, 2, 1)), ("64x64", (3, 1, 16, 16, 64, 64, 3, 2, 1))]
for tag, g in GROUPED:
    for shared in (False, True):
        case(f"grouped {tag} G{g[0]} {g[1:]} {'shared' if shared else 'per group'}", *grouped(*g, shared))


def grouped_out(lib, x, wnk, b):
    out = nan((2, 5, 64), F32)
    FF.conv2d_grouped_bf16(x, wnk, b, 1, 1, 0, 1.0, False, out=out, first=1)
    return out[:, 1:4].contiguous()


case("grouped fp32 out= on a 1x1 map G3 64->64", grouped_out, rn(2, 1, 1, 3 * 64, dtype=BF16), rn(3, 64, 1, 64, dtype=BF16, scale=0.125), rn(3, 64))


# ---- fmi_conv2d_dgrad_bf16 ----
def dgrad(n, h, w, c, k, ks, stride, pad, split=False):
    def run(lib, gy, wck):
        d, oh, ow = desc(n, h, w, c, k, ks, stride, pad)
        dx = nan((n, h, w, c))
        ws = torch.zeros(dx.numel(), device=dev) if split else None
        lib.conv2d_dgrad_bf16(C.byref(d), p(gy), p(wck), None, p(dx), p(ws), 0 if ws is None else ws.numel(), st())
        return dx
    oh, ow = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    return run, rn(n, oh, ow, k, dtype=BF16), wpack(c, ks * ks, k)


case("dgrad stride 1 64->128 2x32x32 k3", *dgrad(2, 32, 32, 64, 128, 3, 1, 1))
case("dgrad stride 2, four phases, odd map 9x7", *dgrad(2, 9, 7, 64, 128, 3, 2, 1))
case("dgrad stride 2 2x64x64 k3", *dgrad(2, 64, 64, 64, 128, 3, 2, 1))
case("dgrad 1x1 stride 2 (three tap-less phases write zeros)", *dgrad(2, 16, 16, 64, 128, 1, 2, 0))
case("dgrad 32-deep tiles 64->96 2x20x20 k3", *dgrad(2, 20, 20, 64, 96, 3, 1, 1))
case("dgrad split workspace 512->512 8x8 k3", *dgrad(2, 8, 8, 512, 512, 3, 1, 1, split=True), det=True)


# the shapes of tests/test_gpu_vgg_bf16.py's masked adjoint (the plain adjoint shares its kernels' inner loop) under every tile mode, and the
# decoder's large layers (tools/bench_tools/bf16_time.py) on the eight-phase kernel, forward and adjoint
for g in ((2, 8, 8, 64, 64), (1, 12, 20, 128, 64), (2, 16, 16, 256, 512), (2, 16, 16, 512, 256)):
    for mode in (0, 2, 8):
        case(f"dgrad {g} k3", *dgrad(*g, 3, 1, 1), tile=mode)
        case(f"fwd {g} k3", *fwd(*g, 3, 1, 1), tile=mode)


# ---- fmi_conv2d_dgrad_relu_bf16: the masked output stage on each of its seven kernels (ADJ_CASES of tests/test_gpu_vgg_bf16.py) ----
def dgrad_relu(n, h, w, c, k):
    def run(lib, gy, wck, a):
        d, _, _ = desc(n, h, w, c, k, 3, 1, 1)
        dx = nan((n, h, w, c))
        lib.conv2d_dgrad_relu_bf16(C.byref(d), p(gy), p(wck), p(a), p(dx), st())
        return dx
    return run, rn(n, h, w, k, dtype=BF16), wpack(c, 9, k), rn(n, h, w, c, dtype=BF16)


for g, modes in (((2, 8, 8, 64, 64), (0, 2, 8)), ((1, 12, 20, 128, 64), (0, 2, 8)), ((2, 16, 16, 256, 512), (0, 2, 8)), ((2, 16, 16, 512, 256), (0, 2, 8)),
                 ((1, 192, 256, 64, 64), (0,)), ((1, 128, 128, 128, 64), (2,)), ((1, 128, 128, 512, 64), (2,)), ((1, 160, 160, 512, 64), (2,))):
    for mode in modes:
        case(f"dgrad_relu {g} k3", *dgrad_relu(*g), tile=mode)
for g in ((4, 64, 64, 512, 512), (4, 128, 128, 256, 256), (4, 256, 256, 128, 128)):
    case(f"dgrad decoder layer {g} k3", *dgrad(*g, 3, 1, 1))
    case(f"fwd decoder layer {g} k3", *fwd(*g, 3, 1, 1))
case("fwd_act decoder layer (4, 128, 128, 256, 256) noise + colscale", *act(4, 128, 128, 256, 256, True, 0.2, 2 ** 0.5))
case("fwd_act decoder layer (4, 256, 256, 128, 128) noise + colscale", *act(4, 256, 256, 128, 128, True, 0.2, 2 ** 0.5))


# ---- fmi_conv2d_wgrad_bf16 (reproducible mode: one workgroup per tile walks the whole pixel range) ----
def wgrad(n, h, w, c, k, ks, stride, pad):
    def run(lib, x, gy):
        d, oh, ow = desc(n, h, w, c, k, ks, stride, pad)
        dwf = torch.zeros(ks * ks, c, k, device=dev)
        lib.conv2d_wgrad_bf16(C.byref(d), p(x), p(gy), p(dwf), st())
        return dwf
    oh, ow = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    return run, rn(n, h, w, c, dtype=BF16), rn(n, oh, ow, k, dtype=BF16)


case("wgrad 64->128 2x32x32 k3", *wgrad(2, 32, 32, 64, 128, 3, 1, 1), det=True)
case("wgrad 32->64 2x17x19 k3 s2", *wgrad(2, 17, 19, 32, 64, 3, 2, 1), det=True)


# ---- the Python forward wrappers that share _conv_fwd_bf16_pre, each at its smallest legal shape ----
def pw_of(wf, ks):
    return FF.PackedWeight(wf, None, wf.shape[0] * wf.shape[1], wf.shape[1], ks, ks)


def wf_of(c, k, ks=3):
    return rn(ks * ks, c, k, scale=(ks * ks * c) ** -0.5)


def bn_relu(lib, x, wf, cb, g, b, rv, rm):
    bn = torch.nn.BatchNorm2d(64).to(dev).eval()
    bn.weight.copy_(g), bn.bias.copy_(b), bn.running_var.copy_(rv), bn.running_mean.copy_(rm)
    return FF.conv_bn_relu_eval_bf16(x, pw_of(wf, 3), cb, bn, 1)


case("conv_bn_relu_eval_bf16 64->64 1x8x8", bn_relu, rn(1, 8, 8, 64, dtype=BF16), wf_of(64, 64), rn(64), rn(64, scale=0.2, shift=1.0), rn(64), rn(64).abs() + 0.5,
     rn(64))
case("conv2d_bias_bf16 64->64 1x8x8", lambda lib, x, wf, b: FF.conv2d_bias_bf16(x, pw_of(wf, 3), b, 1), rn(1, 8, 8, 64, dtype=BF16), wf_of(64, 64), rn(64))
case("conv2d_chan_bf16 64->64 1x8x8", lambda lib, x, wnk, sc, b, sl: FF.conv2d_chan_bf16(x, wnk, 3, 3, 1, 1, sc, b, sl), rn(1, 8, 8, 64, dtype=BF16), wpack(64, 9, 64),
     rn(64, scale=0.2, shift=1.0), rn(64), rn(64, scale=0.3))
case("conv2d_chan_bf16 colsum 64->64 1x12x12", lambda lib, x, wnk: FF.conv2d_chan_bf16(x, wnk, 3, 3, 1, 1, colsum=True), rn(1, 12, 12, 64, dtype=BF16), wpack(64, 9, 64))
case("conv2d_enc_bf16 32->32 1x8x8 (c32 kernel)", lambda lib, x, wf, b: FF.conv2d_enc_bf16(x, pw_of(wf, 3), b, 1, 0.1), rn(1, 8, 8, 32, dtype=BF16), wf_of(32, 32), rn(32))
case("conv2d_enc_bf16 64->64 1x8x8 (chan stage)", lambda lib, x, wf, b: FF.conv2d_enc_bf16(x, pw_of(wf, 3), b, 1, 0.1), rn(1, 8, 8, 64, dtype=BF16), wf_of(64, 64), rn(64))
case("conv2d_plain_bf16 32->32 1x8x8", lambda lib, x, wf: FF.conv2d_plain_bf16(x, pw_of(wf, 3), 1), rn(1, 8, 8, 32, dtype=BF16), wf_of(32, 32))
case("conv2d_thin_in_bf16 3->32 1x16x16", lambda lib, x, wf, b: FF.conv2d_thin_in_bf16(x, pw_of(wf, 3), b, 0.1), rn(1, 16, 16, 3), wf_of(3, 32), rn(32))
case("lrelu_conv2d_thin_bf16 32->3 2x9x35", lambda lib, x, wf, b: FF.lrelu_conv2d_thin_bf16(x, pw_of(wf, 3), b, 0.1, 1, FF.ACT_TANH), rn(2, 9, 35, 32, dtype=BF16),
     wf_of(32, 3), rn(3))
case("_Conv2dBF16.forward 32->32 1x8x8 s2", lambda lib, x, wf: FF.conv2d(x, FF.PackedWeight(wf, wf.transpose(1, 2).contiguous(), 9 * 32, 32, 3, 3), stride=2, pad=1),
     rn(1, 8, 8, 32, dtype=BF16), wf_of(32, 32))

print(f"{'BAD' if bad else 'OK'}: {ran} cases, {bad} differ or failed")
sys.exit(1 if bad else 0)
