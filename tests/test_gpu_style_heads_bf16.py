"""GPU: the bf16 inference form of the map2style heads -- the grouped convolution on its two device paths (the tile kernel of
csrc/conv_bf16.hip with the grouped output stage; the weight-streaming kernel of csrc/style_heads_bf16.hip), its linear form into the
latent tensor, the FPN merge, one level of heads, the whole encoder, the launch ledger, the kept packs and the inference harness.

Kernel by kernel the yardstick is float64 computed here from the very operands the kernel read (bf16 values and bf16-rounded weights
widened).  u32 = 2^-24, u16 = 2^-8, mag = the reference with every term replaced by its absolute value, T = kh kw C:
  convolution v   tol_v = (T + 8) u32 mag + 8 u32 (mag + |bias|): T terms accumulated in fp32 in an order the MFMA, the four waves and
                  their fixed-order meeting choose, then the bias
  bf16 output     v sits within tol_v of the kink only where |v| <= tol_v; taking the other side there moves y by |1 - slope| tol_v:
                  (1 + 2 |slope|) tol_v + u16 |y|  (one bf16 rounding)
  fp32 output     slope 1: tol_v
  merge           8 u32 mag for p32 (two weights of one rounding each, three products, three sums per term), + u16 |ref| for p16
Levels and the encoder chain several bf16 roundings; there the criterion is e = max |out - float64 restatement|, e_emul the same for a
restatement that rounds to bf16 where the kernels store bf16 (the map hand-over and every conv + LeakyReLU output), and
e_hip <= 2 e_emul + (9 C + 8) u32 max |ref|."""
import csv
import ctypes
import math
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U32, U16 = 2.0 ** -24, 2.0 ** -8
F64, BF16 = torch.float64, torch.bfloat16
SLOPE = 0.01


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def FF():
    from face_mask_inpaint_amd import functional

    return functional


@pytest.fixture(scope="module")
def lib():
    from face_mask_inpaint_amd import _lib

    return _lib.lib()


def _d(t):
    return t.detach().cpu().double()


def _rd(t):
    return t.to(BF16).double()


def _within(got, ref, tol, what):
    got = _d(got).reshape(ref.shape)
    err = (got - ref).abs()
    ok = err <= tol  # False for NaN: an element the kernel never wrote
    worst = float((err / tol.clamp_min(1e-300)).nan_to_num(float("inf")).max())
    print(f"{what}: worst err / bound = {worst:.3g}")
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} elements beyond the bound; worst err / bound = {worst:.3g}"


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=dev, dtype=dtype)


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _skinny():
    from face_mask_inpaint_amd import functional

    return functional.STYLE_SKINNY_ROWS


# ---- grouped convolution ---------------------------------------------------------------------------------------------------------------
# name: (N, H, W, C, K, G, shared input); the "edge" cases sit on the two sides of FMI_STYLE_SKINNY_ROWS and follow it if it moves.
# a and b have 75 rows: the tile path at the macro's first value 64 (one stacked convolution; a group index above 4 and two reduction
# chunks), the weight-streaming kernel at 128 -- their twins with 150 rows keep both properties on the tile path
def _geom(name):
    s = _skinny()
    return {"a stacked": (3, 10, 10, 64, 64, 3, True),
            "b groups": (3, 10, 10, 128, 64, 5, False),
            "a stacked, tile": (6, 10, 10, 64, 64, 3, True),     # 150 rows: a and b on the tile path whatever the macro (32, 64 or 128)
            "b groups, tile": (6, 10, 10, 128, 64, 5, False),
            "c edge above": (s + 1, 2, 2, 64, 64, 2, False),
            "c edge at": (s, 2, 2, 64, 64, 2, False),
            "d skinny shared": (1, 16, 16, 64, 64, 3, True),
            "e skinny 4x4": (3, 4, 4, 128, 128, 3, False),
            "e skinny 2x2": (3, 2, 2, 128, 128, 3, False),
            "e skinny 1x1": (3, 1, 1, 64, 64, 2, False),
            "f odd": (2, 5, 3, 64, 64, 2, False)}[name]


GEOMS = ["a stacked", "b groups", "a stacked, tile", "b groups, tile", "c edge above", "c edge at", "d skinny shared", "e skinny 4x4", "e skinny 2x2", "e skinny 1x1",
         "f odd"]


def _operands(gen, n, h, w, c, k, g, shared, kk):
    """x bf16 with exact zeros on every seventh element, weights bf16 [G][K][C][kk][kk], biases of both signs"""
    cx = c if shared else g * c
    x = torch.randn(n * h * w * cx, generator=gen)
    x[::7] = 0.0
    x = x.reshape(n, h, w, cx).to(BF16)
    wt = (torch.randn(g, k, c, kk, kk, generator=gen) / (c * kk * kk) ** 0.5).to(BF16)
    bias = torch.rand(g, k, generator=gen) * 2 - 1
    assert bool((bias > 0).any()) and bool((bias < 0).any())
    return x, wt, bias


def _grouped64(x, wt, bias, shared, stride, pad):
    """(v, mag) float64 NHWC [N,OH,OW,G*K]: acc + bias and the sum of the absolute terms"""
    g, k, c = wt.shape[:3]
    vs, ms = [], []
    for i in range(g):
        xi = x.double()[..., :c] if shared else x.double()[..., i * c:(i + 1) * c]
        xi, wi = xi.permute(0, 3, 1, 2), wt[i].double()
        vs.append(F.conv2d(xi, wi, stride=stride, padding=pad).permute(0, 2, 3, 1) + bias[i].double())
        ms.append(F.conv2d(xi.abs(), wi.abs(), stride=stride, padding=pad).permute(0, 2, 3, 1))
    return torch.cat(vs, -1).contiguous(), torch.cat(ms, -1).contiguous()


def _tol_v(mag, bias, terms):
    b = bias.double().reshape(1, 1, 1, -1).abs()
    return (terms + 8) * U32 * mag + 8 * U32 * (mag + b)


def _wnk(wt):
    g, k, c, kh, kw = wt.shape
    return wt.permute(0, 1, 3, 4, 2).reshape(g, k, kh * kw, c).contiguous()


@pytest.mark.parametrize("name", GEOMS)
def test_grouped_conv(dev, lib, name):
    from face_mask_inpaint_amd._lib import ConvDesc

    n, h, w, c, k, g, shared = _geom(name)
    gen = torch.Generator().manual_seed(4100 + GEOMS.index(name))
    x, wt, bias = _operands(gen, n, h, w, c, k, g, shared, 3)
    v, mag = _grouped64(x, wt, bias, shared, 2, 1)
    oh, ow = v.shape[1], v.shape[2]
    rows = n * oh * ow
    print(f"{name}: rows {rows} ({'tile' if rows > _skinny() else 'skinny'} path)")
    ref = torch.where(v > 0, v, SLOPE * v)
    tol = (1 + 2 * SLOPE) * _tol_v(mag, bias, 9 * c) + U16 * ref.abs()
    pitch = g * k + 8  # eight guard columns behind every pixel
    y = _nan((n, oh, ow, pitch), dev, BF16)
    d = ConvDesc(n, h, w, c, oh, ow, k, x.shape[3], pitch, 3, 3, 2, 1, 0, 1)
    xd, wd, bd = x.to(dev), _wnk(wt).to(dev), bias.to(dev)
    lib.conv2d_grouped_fwd_bf16(ctypes.byref(d), g, 0 if shared else c, _vp(xd), _vp(wd), _vp(bd), SLOPE, _vp(y), None,
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[..., g * k:]).all()), "guard columns were written"
    _within(y[..., :g * k], ref, tol, name)


def test_grouped_conv_without_bias_and_activation(dev, FF):
    """bias NULL and slope 1 through the Python entry (dense pitch): both device paths"""
    for n in (6, 1):  # 150 rows: tile path; 25 rows: skinny path
        gen = torch.Generator().manual_seed(4150 + n)
        x, wt, bias = _operands(gen, n, 10, 10, 64, 64, 2, False, 3)
        v, mag = _grouped64(x, wt, torch.zeros_like(bias), False, 2, 1)
        y = FF.conv2d_grouped_bf16(x.to(dev), _wnk(wt).to(dev), None, 3, 2, 1, slope=1.0, shared=False)
        _within(y, v, 3 * _tol_v(mag, torch.zeros_like(bias), 9 * 64) + U16 * v.abs(), f"no bias, slope 1, N={n}")


# ---- linear form -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 70])  # 70: a second 64-row block
def test_linear_into_latent_slots(dev, FF, n):
    c = k = 128
    g = 4
    gen = torch.Generator().manual_seed(4200 + n)
    x, wt, bias = _operands(gen, n, 1, 1, c, k, g, False, 1)
    v, mag = _grouped64(x, wt, bias, False, 1, 0)
    lat = _nan((n, 7, k), dev)
    out = FF.conv2d_grouped_bf16(x.to(dev), _wnk(wt).to(dev), bias.to(dev), 1, 1, 0, slope=1.0, shared=False, out=lat, first=2)
    torch.cuda.synchronize()
    assert out is lat
    assert bool(torch.isnan(lat[:, :2]).all()) and bool(torch.isnan(lat[:, 6:]).all()), "slots 0, 1 or 6 were written"
    _within(lat[:, 2:6], v.reshape(n, g, k), _tol_v(mag, bias, c).reshape(n, g, k), f"linear N={n}")


# ---- merge -----------------------------------------------------------------------------------------------------------------------------
MERGE = {"6x10 from 3x5": ((2, 6, 10, 64), (2, 3, 5, 64), True), "2x2 from 1x1": ((2, 2, 2, 64), (2, 1, 1, 64), True),
         "conversion": ((2, 6, 10, 64), None, True), "no fp32 output": ((2, 6, 10, 64), (2, 3, 5, 64), False)}


@pytest.mark.parametrize("name", list(MERGE))
def test_fpn_merge(dev, FF, name):
    ls, cs, want32 = MERGE[name]
    gen = torch.Generator().manual_seed(4300 + len(name))
    lat = torch.randn(ls, generator=gen)
    coarse = torch.randn(cs, generator=gen) * 1.5 if cs is not None else None
    p32, p16 = FF.fpn_merge_bf16(lat.to(dev), None if coarse is None else coarse.to(dev), want_f32=want32)
    if coarse is None:
        assert torch.equal(p32.cpu(), lat) and torch.equal(p16.cpu(), lat.to(BF16))
        return
    up = lambda t: F.interpolate(t.double().permute(0, 3, 1, 2), size=ls[1:3], mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    ref, mag = up(coarse) + lat.double(), up(coarse.abs()) + lat.double().abs()
    assert (p32 is not None) == want32
    if want32:
        _within(p32, ref, 8 * U32 * mag, name + " p32")
    assert p16.dtype == BF16
    _within(p16, ref, 8 * U32 * mag + U16 * ref.abs(), name + " p16")


# ---- float64 restatement of the heads of one level (plain torch, NCHW) ----------------------------------------------------------------
def _level64(heads, pmap, rd):
    """pmap: float64 NHWC level map; rd rounds where the kernels store bf16 (identity: the float64 yardstick); returns [N, G, K]"""
    out = []
    x0 = rd(pmap).permute(0, 3, 1, 2)
    for h in heads:
        x = x0
        for m in h.convs:
            if isinstance(m, torch.nn.Conv2d):
                x = F.conv2d(x, _rd(m.weight.detach().cpu()), _d(m.bias), stride=2, padding=1)
            else:
                x = rd(torch.where(x > 0, x, m.negative_slope * x))
        wl = _rd(h.linear.weight.detach().cpu() * h.linear.scale)  # the product in fp32, as the pack is made
        out.append(x.reshape(x.shape[0], -1) @ wl.T + _d(h.linear.bias) * h.linear.lr_mul)
    return torch.stack(out, 1)


def _criterion(got, ref, emul, cred, what):
    """e_hip <= 2 e_emul + (9 C + 8) u32 max |ref|"""
    e_hip = float((_d(got) - ref).abs().max())
    e_emul = float((emul - ref).abs().max())
    floor = (9 * cred + 8) * U32 * float(ref.abs().max())
    print(f"{what}: e_hip {e_hip:.4g}  e_emul {e_emul:.4g}  ratio {e_hip / max(e_emul, 1e-300):.3f}  floor {floor:.3g}  max|ref| {float(ref.abs().max()):.4g}")
    assert e_hip == e_hip and e_hip <= 2 * e_emul + floor, f"{what}: e_hip {e_hip:.4g} > 2 x e_emul {e_emul:.4g} + floor {floor:.3g}"


def _random_heads(seed, count, width, spatial):
    from face_mask_inpaint_amd.modules.psp.encoders.psp_encoders import GradualStyleBlock

    torch.manual_seed(seed)
    heads = torch.nn.ModuleList([GradualStyleBlock(width, width, spatial) for _ in range(count)])
    with torch.no_grad():
        for h in heads:
            h.linear.bias.uniform_(-0.5, 0.5)
    return heads


@pytest.mark.parametrize("count,width,spatial", [(3, 64, 8), (2, 128, 4)])
def test_one_level_of_heads(dev, FF, count, width, spatial):
    from face_mask_inpaint_amd.modules.psp.encoders.psp_encoders import style_level_bf16
    from face_mask_inpaint_amd.weights import weight_scope

    heads = _random_heads(4400 + width, count, width, spatial).to(dev).eval()
    gen = torch.Generator().manual_seed(4401 + width)
    pmap = torch.randn(3, spatial, spatial, width, generator=gen) * 1.5
    lat = _nan((3, count + 2, width), dev)
    with torch.no_grad(), weight_scope(heads):
        _, p16 = FF.fpn_merge_bf16(pmap.to(dev), None, want_f32=False)
        style_level_bf16(list(heads), p16, lat, first=1)
    assert bool(torch.isnan(lat[:, 0]).all()) and bool(torch.isnan(lat[:, -1]).all())
    ref, emul = _level64(heads, pmap.double(), lambda v: v), _level64(heads, pmap.double(), _rd)
    _criterion(lat[:, 1:-1], ref, emul, width, f"{count} heads {width} @ {spatial}")


# ---- whole encoder ---------------------------------------------------------------------------------------------------------------------
def _randomise(module, gen):
    """random running statistics (variance in [0.5, 2]), affine parameters of both signs, PReLU weights in [-0.1, 0.5]"""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_((torch.rand(c, generator=gen) * 0.5 + 0.75) * (torch.randint(0, 2, (c,), generator=gen) * 2 - 1))
                m.bias.copy_(torch.rand(c, generator=gen) - 0.5)
                m.running_mean.copy_(torch.randn(c, generator=gen) * 0.3)
                m.running_var.copy_(torch.rand(c, generator=gen) * 1.5 + 0.5)
            elif isinstance(m, torch.nn.PReLU):
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) * 0.6 - 0.1)


SPATIAL = (4, 8, 16)
LEVELS = ((0, 3), (3, 7), (7, 10))


def _encoder(dev, heads_dtype, seed=44, frozen=False):
    from face_mask_inpaint_amd.modules.psp.encoders.psp_encoders import GradualStyleEncoder

    opts = SimpleNamespace(n_styles=10, use_attention=True)
    if heads_dtype is not None:
        opts.style_heads_eval_dtype = heads_dtype
    torch.manual_seed(seed)
    enc = GradualStyleEncoder(50, "ir_se", opts, _widths=(64, 64, 64, 128, 128), _spatial=SPATIAL)
    _randomise(enc.body, torch.Generator().manual_seed(seed + 1))
    if frozen:
        for p_ in enc.parameters():
            p_.requires_grad_(False)
    return enc.to(dev).eval()


def _inputs(dev, seed=46, nb=2):
    gen = torch.Generator().manual_seed(seed)
    xs, rf = torch.rand(nb, 3, 64, 64, generator=gen) * 2 - 1, torch.rand(nb, 3, 64, 64, generator=gen) * 2 - 1
    m = torch.zeros(nb, 64, 64)
    m[:, 20:50, 12:44] = 1
    return xs.to(dev), rf.to(dev), m.to(dev)


def _forward_recording(enc, FF, monkeypatch, inputs):
    """(codes, the three bf16 level maps the heads read)"""
    maps = []
    orig = FF.fpn_merge_bf16
    with monkeypatch.context() as mp:
        mp.setattr(FF, "fpn_merge_bf16", lambda *a, **k: (lambda r: (maps.append(r[1]), r)[1])(orig(*a, **k)))
        with torch.no_grad():
            codes = enc(inputs[0], ref=inputs[1], mask=inputs[2])
    assert len(maps) == 3 and all(m.dtype == BF16 for m in maps)
    return codes, maps


def _check_codes(enc, codes, maps, what):
    for (lo, hi), pm in zip(LEVELS, maps):
        heads = [enc.styles[j] for j in range(lo, hi)]
        ref, emul = _level64(heads, _d(pm), lambda v: v), _level64(heads, _d(pm), _rd)
        _criterion(codes[:, lo:hi], ref, emul, 128, f"{what} heads {lo}..{hi - 1}")


def test_whole_encoder(dev, FF, monkeypatch):
    e16, e32, e0 = _encoder(dev, "bf16"), _encoder(dev, "fp32"), _encoder(dev, None)
    assert list(e16.state_dict()) == list(e32.state_dict()) and all(torch.equal(v, e32.state_dict()[k]) for k, v in e16.state_dict().items())
    inp = _inputs(dev)
    codes, maps = _forward_recording(e16, FF, monkeypatch, inp)
    assert codes.shape == (2, 10, 128) and codes.dtype == torch.float32
    assert [tuple(m.shape) for m in maps] == [(2, 4, 4, 128), (2, 8, 8, 128), (2, 16, 16, 128)]
    _check_codes(e16, codes, maps, "encoder")
    run = lambda e: e(inp[0], ref=inp[1], mask=inp[2])
    with torch.no_grad():
        c32 = run(e32)
    scale, err = float(c32.abs().max()), float((codes - c32).abs().max())
    print(f"whole encoder: bf16 heads vs fp32 heads {err / scale:.3g} of the codes' range")
    with torch.no_grad(), FF.deterministic(True):
        assert torch.equal(run(e16), run(e16)), "two bf16 forwards differ"
        assert torch.equal(run(e32), run(e0)), "option fp32 and the absent option differ"
    e16.train(), e32.train()  # training mode is the fp32 path whatever the eval option says, bit for bit
    with torch.no_grad(), FF.deterministic(True):
        assert torch.equal(run(e16), run(e32))


def test_launches(dev, FF, monkeypatch):
    """frozen weights, second forward: sum over levels of (log2(spatial) + 1) grouped-convolution calls, 3 merges, and nothing else
    between the last lateral convolution and the return"""
    from face_mask_inpaint_amd import _lib
    from face_mask_inpaint_amd.modules.psp.encoders import psp_encoders as PE

    enc, inp = _encoder(dev, "bf16", frozen=True), _inputs(dev)
    with torch.no_grad():
        enc(inp[0], ref=inp[1], mask=inp[2])  # packs are made here
    L = _lib.lib()
    calls = []
    orig_run_conv = PE.run_conv

    def run_conv(m, x):
        y = orig_run_conv(m, x)
        if m is enc.latlayer1 or m is enc.latlayer2:
            calls.append("lateral done")
        return y

    with monkeypatch.context() as mp:
        for name in _lib.SIGNATURES:
            fn = getattr(L, name[4:])
            mp.setattr(L, name[4:], (lambda f, nm: lambda *a: (calls.append(nm), f(*a))[1])(fn, name))
        mp.setattr(PE, "run_conv", run_conv)
        with torch.no_grad():
            enc(inp[0], ref=inp[1], mask=inp[2])
    want = sum(int(math.log2(s)) + 1 for s in SPATIAL)
    assert calls.count("fmi_conv2d_grouped_fwd_bf16") == want == 12 and calls.count("fmi_fpn_merge_bf16") == 3, calls
    assert calls.count("lateral done") == 2
    tail = calls[len(calls) - calls[::-1].index("lateral done"):]
    assert tail == ["fmi_fpn_merge_bf16"] + ["fmi_conv2d_grouped_fwd_bf16"] * (int(math.log2(SPATIAL[2])) + 1), tail


def test_packs_follow_the_weights(dev, FF, monkeypatch):
    from face_mask_inpaint_amd import weights

    enc, inp = _encoder(dev, "bf16", frozen=True), _inputs(dev)
    first, maps = _forward_recording(enc, FF, monkeypatch, inp)
    _check_codes(enc, first, maps, "frozen")
    kept = enc._fmi_head_packs[(3, 4)]
    again, _ = _forward_recording(enc, FF, monkeypatch, inp)
    assert enc._fmi_head_packs[(3, 4)] is kept  # unchanged frozen weights: the stacked packs are the same objects
    _check_codes(enc, again, _, "frozen, kept packs")
    w = enc.styles[4].convs[0].weight
    with torch.no_grad():
        v0 = w._version
        w.mul_(1.5)  # a visible in-place edit: the version counter moves
        assert w._version != v0
    second, maps = _forward_recording(enc, FF, monkeypatch, inp)
    _check_codes(enc, second, maps, "after the in-place edit")
    assert not torch.equal(first[:, 4], second[:, 4])
    v0 = w._version
    w.data.mul_(0.5)  # an edit the version counter does not see
    assert w._version == v0
    weights.invalidate_packs(enc)
    third, maps = _forward_recording(enc, FF, monkeypatch, inp)
    _check_codes(enc, third, maps, "after invalidate_packs")
    assert not torch.equal(second[:, 4], third[:, 4]) and not torch.equal(first[:, 4], third[:, 4])


# ---- harness ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", ["fp32", "bf16"])
def test_psp_inference_bf16_heads(dev, FF, tmp_path, body):
    from face_mask_inpaint_amd import psp_inference as PI

    out = str(tmp_path / "heads")
    flags = ["--style_heads_dtype", "bf16"] + (["--encoder_dtype", "bf16"] if body == "bf16" else [])
    torch.manual_seed(12)
    ssim, ms = PI.main(flags + ["--output_size", "256", "--num_batches", "1", "--batch_size", "2", "--out_dir", out])
    assert ssim == ssim and ms == ms and -1.0 <= ssim <= 1.0 and -1.0 <= ms <= 1.0
    assert sorted(os.listdir(out)) == ["gen_0.jpg", "gen_1.jpg", "metrics.csv"]
    rows = list(csv.reader(open(os.path.join(out, "metrics.csv"))))
    assert rows[0] == ["ssim", "ms_ssim"] and (float(rows[1][0]), float(rows[1][1])) == (ssim, ms)
