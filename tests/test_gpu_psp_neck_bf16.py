"""GPU: the bf16 stem and neck of the pSp encoder for inference -- the fused stem (fmi_irse_stem_fwd_bf16), the guided attention at the pSp
shapes (fmi_guided_attention_sliced_fwd_bf16: (64, 256) and (128, 512)), ExampleGuidedAttention with out_conv on bf16 maps, the mask blend, the
FPN merge from bf16 maps, psp_encoders.neck_bf16 at full widths, the launch ledger, the whole encoder and the inference harness.

Kernel by kernel the yardstick is float64 computed here from the very operands the kernel read.  u32 = 2^-24, u16 = 2^-8, mag = the
reference with every term replaced by its absolute value:
  stem          v = conv3x3(x): 27 fp32 fmas, tol_v = (27 + 8) u32 mag_v; u = v scale + shift: mag_u = mag_v |scale| + |shift| and
                tol_u = (27 + 8) u32 mag_u (the fma and the slope's product are two of the 8); across the PReLU kink (1 + 2 |slope|) tol_u;
                y adds u16 |y|; z = a scale0 + shift0 carries |scale0| tol_a + 2 u32 (|a scale0| + |shift0|) and u16 |z|
  attention     the bound of tests/test_gpu_picnet_enc_bf16.py::test_guided_attention_against_float64 (same kernel scheme, same derivation)
                with d and C of the case
  blend         three fp32 roundings (1 - m, its product, the fma): 3 u32 mag + u16 |y|
  merge         8 u32 mag + u16 |y| (tests/test_gpu_style_heads_bf16.py)
Module and neck level chain several bf16 roundings; there e = max |out - float64 restatement|, e_emul the same for a restatement that
rounds to bf16 exactly where the kernels store bf16 (and the attention probabilities entering P V), and the requirement is
e_hip <= 2 e_emul + (R + 8) u32 max mag, R the reduction length of the last convolution in front of the output (2 for a blend).
The restatements are pinned against oracle/psp_cpu.py and the reference-generated fixtures by tests/test_host_psp_neck_bf16.py."""
import csv
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U32, U16 = 2.0 ** -24, 2.0 ** -8
F64, BF16 = torch.float64, torch.bfloat16
THR = 20.0  # ATT_THR of csrc/attention_bf16.hip


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def FF():
    from face_mask_inpaint_amd import functional

    return functional


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _d(t):
    return t.detach().cpu().double()


def _rd(t):
    return t.to(BF16).double()


def _id(t):
    return t


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _within(got, ref, tol, what):
    got = _d(got).reshape(ref.shape)
    err = (got - ref).abs()
    ok = err <= tol  # False for NaN: an element the kernel never wrote
    worst = float((err / tol.clamp_min(1e-300)).nan_to_num(float("inf")).max())
    print(f"{what}: worst err / bound = {worst:.3g}")
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} elements beyond the bound; worst err / bound = {worst:.3g}"


def _criterion(got, ref, emul, floor, what):
    """e_hip <= 2 e_emul + floor"""
    e_hip = float((_d(got).reshape(ref.shape) - ref).abs().max())
    e_emul = float((emul - ref).abs().max())
    print(f"{what}: e_hip {e_hip:.4g}  e_emul {e_emul:.4g}  ratio {e_hip / max(e_emul, 1e-300):.3f}  floor {floor:.3g}  max|ref| {float(ref.abs().max()):.4g}")
    assert e_hip == e_hip and e_hip <= 2 * e_emul + floor, f"{what}: e_hip {e_hip:.4g} > 2 x e_emul {e_emul:.4g} + floor {floor:.3g}"


# ---- float64 restatements (NHWC; shared with tests/test_host_psp_neck_bf16.py, which pins them) ------------------------------------------
def stem64(x, wt, scale, shift, slope, scale0, shift0):
    """x [N,H,W,C] and wt [K][C][3][3] -> (a, z, mag_u) with a = prelu(conv3x3(x) scale + shift, slope), z = a scale0 + shift0"""
    x64 = x.double().permute(0, 3, 1, 2)
    v = F.conv2d(x64, wt.double(), padding=1).permute(0, 2, 3, 1)
    mag = F.conv2d(x64.abs(), wt.double().abs(), padding=1).permute(0, 2, 3, 1)
    u = v * scale.double() + shift.double()
    a = torch.where(u > 0, u, slope.double() * u)
    return a, a * scale0.double() + shift0.double(), mag * scale.double().abs() + shift.double().abs()


def guided64(wq, wo, bo, m, src, ref, rd):
    """ExampleGuidedAttention (example_guided_att.py:21-41) on NHWC float64 maps: wq [C/4][C], wo [K][2C] / bo [K] or None, m [N,H,W].
    ``rd`` rounds where the bf16 form stores bf16: q, the probabilities entering P V (the row sum adds the unrounded ones), the
    concatenated output and out_conv's output.  Returns (out, mag of the last reduction)"""
    n, h, w, c = src.shape
    t = h * w
    s_, r_, mm = src.reshape(n, t, c), ref.reshape(n, t, c), m.reshape(n, t, 1)
    q = rd(s_ @ wq.T)
    sc = q @ q.transpose(1, 2)
    p = torch.exp(sc - sc.amax(-1, keepdim=True))
    L = p.sum(-1, keepdim=True)
    pr = rd(p)
    cat = rd(torch.cat([(1 - mm) * ((pr @ r_) / L) + mm * r_, (pr @ s_) / L], dim=-1))
    if wo is None:
        mag = torch.cat([(1 - mm) * ((p @ r_.abs()) / L) + mm * r_.abs(), (p @ s_.abs()) / L], dim=-1)
        return cat.reshape(n, h, w, 2 * c), mag.reshape(n, h, w, 2 * c)
    out = rd(cat @ wo.T + bo)
    return out.reshape(n, h, w, -1), (cat.abs() @ wo.abs().T + bo.abs()).reshape(n, h, w, -1)


def blend64(m, r, c):
    mm = m.unsqueeze(-1)
    return mm * r + (1 - mm) * c, mm * r.abs() + (1 - mm) * c.abs()


def merge64(lat, coarse):
    up = lambda t: F.interpolate(t.permute(0, 3, 1, 2), size=lat.shape[1:3], mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    return up(coarse) + lat, up(coarse.abs()) + lat.abs()


def neck64(W, c1, c2, c3, r1, r2, r3, masks, use_att, rd):
    """psp_encoders.py:126-147 on NHWC float64 maps.  W: a1q / a1o / a1b, a2q / a2o / a2b (the attentions' conv and out_conv), l1w / l1b,
    l2w / l2b (latlayer1 / latlayer2, [K][C] and [K]); masks = the three resized masks (coarse, middle, fine) or None without a reference.
    Returns ([coarse, middle, fine], [their last-reduction magnitudes], [their reduction lengths])"""
    red3 = 0
    mag3 = c3.abs()
    if r3 is not None:
        m3, m2, m1 = masks
        if use_att:
            c3, mag3 = guided64(W["a1q"], W["a1o"], W["a1b"], m3, c3, r3, rd)
            c2, _ = guided64(W["a2q"], W["a2o"], W["a2b"], m2, c2, r2, rd)
            red3 = W["a1o"].shape[1]
        else:
            (c3, mag3), (c2, _) = blend64(m3, r3, c3), blend64(m2, r2, c2)
            c3, c2, red3 = rd(c3), rd(c2), 2
        c1 = rd(blend64(m1, r1, c1)[0])
    l2 = rd(c2 @ W["l1w"].T + W["l1b"])
    p2, mag2 = merge64(l2, c3)
    mag2 = mag2 - l2.abs() + (c2.abs() @ W["l1w"].abs().T + W["l1b"].abs())
    p2 = rd(p2)
    l1 = rd(c1 @ W["l2w"].T + W["l2b"])
    p1, mag1 = merge64(l1, p2)
    mag1 = mag1 - l1.abs() + (c1.abs() @ W["l2w"].abs().T + W["l2b"].abs())
    return [c3, p2, rd(p1)], [mag3, mag2, mag1], [red3, W["l1w"].shape[1], W["l2w"].shape[1]]


def neck_weights(att1, att2, lat1, lat2, rw):
    """the float64 weights neck64 reads from the modules; ``rw`` rounds the convolution weights (to bf16: what the kernels read)"""
    w2 = lambda conv: rw(conv.weight.detach().cpu().float()).double().reshape(conv.out_channels, conv.in_channels)
    W = {"l1w": w2(lat1), "l1b": _d(lat1.bias), "l2w": w2(lat2), "l2b": _d(lat2.bias)}
    for name, att in (("a1", att1), ("a2", att2)):
        if att is not None:
            W[name + "q"], W[name + "o"], W[name + "b"] = w2(att.conv), w2(att.out_conv), _d(att.out_conv.bias)
    return W


def _soft_mask(n, t, seed):
    m = torch.rand(n, t, generator=_gen(seed))
    m[:, 10:40] = 0.0
    m[:, t - 50:t - 20] = 1.0
    return m


# ---- fused stem --------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,h,w", [(2, 20, 36), (1, 5, 7)], ids=["2x20x36", "1x5x7"])
def test_fused_stem_against_float64(dev, FF, n, h, w):
    """K = 64 from C = 3; slopes of both signs and exact zeros, a shift that moves the kink off zero; (1, 5, 7): border and tail pixels
    outnumber the interior"""
    g = _gen(7100 + h)
    k = 64
    x = torch.rand(n, h, w, 3, generator=g) * 2 - 1
    wt = torch.randn(k, 3, 3, 3, generator=g) * 0.3
    scale = (torch.rand(k, generator=g) * 0.5 + 0.75) * (torch.randint(0, 2, (k,), generator=g) * 2 - 1)
    shift = torch.rand(k, generator=g) - 0.5
    slope = torch.rand(k, generator=g) * 0.6 - 0.1
    slope[::5] = 0.0
    assert bool((slope > 0).any()) and bool((slope < 0).any()) and bool((shift.abs() > 0.1).any())
    scale0 = (torch.rand(k, generator=g) * 0.5 + 0.75) * (torch.randint(0, 2, (k,), generator=g) * 2 - 1)
    shift0 = torch.rand(k, generator=g) - 0.5
    a64, z64, mag_u = stem64(x, wt, scale, shift, slope, scale0, shift0)
    pw = FF.PackedWeight(wt.permute(2, 3, 1, 0).reshape(9, 3, k).contiguous().to(dev), None, k, 3, 3, 3)
    vec = [t.to(dev) for t in (scale, shift, slope, scale0, shift0)]
    d, _, _ = FF.conv_desc(n, h, w, 3, k, 3, 3, 1, 1)
    xd = x.to(dev)
    y = torch.full((n, h, w, k), float("nan"), device=dev, dtype=BF16)
    z = torch.full((n, h, w, k), float("nan"), device=dev, dtype=BF16)
    a = torch.full((n, h, w, k), float("nan"), device=dev, dtype=torch.float32)
    FF._L().irse_stem_fwd_bf16(ctypes.byref(d), FF._p(xd), FF._p(pw.wf), *[FF._p(t) for t in vec], FF._p(y), FF._p(z), FF._p(a), FF._st())
    torch.cuda.synchronize()
    tol_u = (27 + 8) * U32 * mag_u
    tol_a = (1 + 2 * slope.double().abs()) * tol_u
    _within(a, a64, tol_a, f"stem a (fp32) {n}x{h}x{w}")
    _within(y, a64, tol_a + U16 * (a64.abs() + tol_a), f"stem y {n}x{h}x{w}")
    tol_z = scale0.double().abs() * tol_a + 2 * U32 * ((a64 * scale0.double()).abs() + shift0.double().abs())
    _within(z, z64, tol_z + U16 * (z64.abs() + tol_z), f"stem z {n}x{h}x{w}")
    assert float((a64[:, 0] - a64[:, 1]).abs().max()) > 1e-3  # the zero padding: the border row is not what the interior gives
    # both outputs are roundings of the kernel's own fp32 a: the hand-over kernel applied to it gives the same bits
    y2, z2 = FF.irse_stem_bf16(a, vec[3], vec[4])
    assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(z), _bits(z2))
    # the wrapper, without the debug output
    y3, z3 = FF.irse_stem_fused_bf16(xd, pw, *vec)
    assert torch.equal(_bits(y), _bits(y3)) and torch.equal(_bits(z), _bits(z3))


# ---- guided attention at the pSp shapes -------------------------------------------------------------------------------------------------
GUIDED_CASES = [(128, 0), (384, 0), (256, 4), (256, 8)]  # (T, waves); N = 2


def _guided_call(dev, FF, q, src, ref, m, waves):
    n, t, d = q.shape
    out = FF.guided_attention_bf16(q.to(dev), src.to(dev), ref.to(dev), m.to(dev), waves=waves)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind", ["gauss", "late"])
@pytest.mark.parametrize("tw", GUIDED_CASES, ids=lambda s: "T%d_w%d" % s)
@pytest.mark.parametrize("d,c", [(64, 256), (128, 512)], ids=["d64_C256", "d128_C512"])
def test_guided_attention_against_float64(dev, FF, d, c, tw, kind):
    """out[..., :C] = (1 - m) (A ref) + m ref, out[..., C:] = A src: T = 128 is one query tile, 384 three key stages of 128 and no multiple
    of 256, 256 with four and with eight waves.  "gauss": scores of a few units; "late": a late key tile exceeds the earlier maximum by
    more than 20, so the lazy rescale fires (checked on the float64 scores)."""
    from test_gpu_picnet_bf16 import _attn_data, _branches

    t, waves = tw
    n = 2
    q, ref_v = _attn_data(kind, n, t, d, c, seed=202)
    if kind == "gauss":  # |q|^2 ~ 5: the diagonal holds about half of a row's weight, the other keys share the rest
        q = (torch.randn(n, t, d, generator=_gen(203)) * (5.0 / d) ** 0.5).to(BF16)
    src_v = torch.randn(n, t, c, generator=_gen(201)).to(BF16)
    m = _soft_mask(n, t, 202)
    q64 = q.double()
    s = q64 @ q64.transpose(1, 2)
    pmax = float(torch.softmax(s, -1).amax(-1).mean())
    if kind == "late":
        fired, deferred, margin = _branches(s)
        print(f"\n  late: {fired} rescales after the first tile, {deferred} deferrals, nearest test {margin:.3f}")
        assert fired > 0 and margin > 0.01
    else:
        assert 0.2 < pmax < 0.8, pmax  # neither uniform nor one-hot
    smax = s.amax(-1, keepdim=True)
    p = torch.exp(s - smax)
    L = p.sum(-1, keepdim=True)
    E = (d * U32 * (q64.abs() @ q64.abs().transpose(1, 2))).amax(-1, keepdim=True)
    R = smax - s.amin(-1, keepdim=True) + THR
    eta = E + 3 * U32 * R + 2.0 ** -22
    nT = t + t // 64

    def half(v):
        v64 = v.double()
        o = (p @ v64) / L
        A = (p @ v64.abs()) / L
        return o, 1.001 * (A * (eta + U16 + nT * U32) + o.abs() * (eta + nT * U32 + 3 * U32))

    o_ref, B_ref = half(ref_v)
    o_src, B_src = half(src_v)
    m64 = m.double().unsqueeze(-1)
    y = (1 - m64) * o_ref + m64 * ref_v.double()
    out = _guided_call(dev, FF, q, src_v, ref_v, m, waves)
    assert out.dtype == BF16 and out.shape == (n, t, 2 * c)
    what = f"guided attention d{d} C{c} T{t} w{waves} {kind}"
    _within(out[..., :c], y, (1 - m64) * B_ref + 2 * U32 * y.abs() + U16 * (y.abs() + (1 - m64) * B_ref), what + " blend half")
    _within(out[..., c:], o_src, B_src + U16 * (o_src.abs() + B_src), what + " src half")
    ones = m == 1.0
    assert int(ones.sum()) >= 30 * n and int((m == 0.0).sum()) >= 30 * n
    assert torch.equal(_bits(out[..., :c])[ones], _bits(ref_v)[ones]), "m == 1 must return ref bit for bit"
    out2 = _guided_call(dev, FF, q, src_v, ref_v, m, waves)
    assert torch.equal(_bits(out), _bits(out2)), "two calls differ"


def _att_module(c, seed, dev):
    from face_mask_inpaint_amd.modules.example_guided_att import ExampleGuidedAttention

    torch.manual_seed(seed)
    att = ExampleGuidedAttention(c, out_channels=c)
    with torch.no_grad():
        att.conv.weight.mul_(0.6)  # scores of a few units: neither a uniform nor a one-hot attention
        att.out_conv.bias.uniform_(-0.5, 0.5)
    return att.to(dev).eval()


def test_example_guided_attention_with_out_conv(dev, FF):
    """ExampleGuidedAttention(256, out_channels=256) on bf16 maps at 8 x 16: query convolution, attention, out_conv with its bias"""
    c = 256
    att = _att_module(c, 7200, dev)
    g = _gen(7201)
    src, ref_f = torch.randn(2, 8, 16, c, generator=g).to(BF16), torch.randn(2, 8, 16, c, generator=g).to(BF16)
    m = _soft_mask(2, 128, 7202).view(2, 8, 16)
    with torch.no_grad():
        out = att.nhwc(m.to(dev), src.to(dev), ref_f.to(dev))
    assert out.dtype == BF16 and out.shape == (2, 8, 16, c)
    W = neck_weights(att, None, att.out_conv, att.out_conv, lambda w: w.to(BF16))
    ref, mag = guided64(W["a1q"], W["a1o"], W["a1b"], m.double(), src.double(), ref_f.double(), _id)
    emul, _ = guided64(W["a1q"], W["a1o"], W["a1b"], m.double(), src.double(), ref_f.double(), _rd)
    _criterion(out, ref, emul, (2 * c + 8) * U32 * float(mag.max()), "ExampleGuidedAttention(256, out 256) at 8 x 16")


# ---- mask blend and FPN merge ------------------------------------------------------------------------------------------------------------
def test_mask_blend_against_float64(dev, FF):
    g = _gen(7300)
    r, c = (torch.randn(2, 5, 7, 64, generator=g) * 2).to(BF16), (torch.randn(2, 5, 7, 64, generator=g) * 2).to(BF16)
    r[0, 0, 0, :4] = -0.0
    c[1, 4, 6, :4] = -0.0
    m = torch.rand(2, 5, 7, generator=g)
    m[0, :2] = 1.0
    m[1, 3:] = 0.0
    y = FF.mask_blend_bf16(m.to(dev), r.to(dev), c.to(dev))
    assert y.dtype == BF16 and y.shape == r.shape
    ref, mag = blend64(m.double(), r.double(), c.double())
    _within(y, ref, 3 * U32 * mag + U16 * ref.abs(), "mask blend")
    ones, zeros = m == 1.0, m == 0.0
    assert int(ones.sum()) == 14 and int(zeros.sum()) == 14
    assert torch.equal(_bits(y)[ones], _bits(r)[ones]), "m == 1 must return r bit for bit"
    assert torch.equal(_bits(y)[zeros], _bits(c)[zeros]), "m == 0 must return c bit for bit"


@pytest.mark.parametrize("coarse_hw", [(3, 5), (6, 10)], ids=["up2", "same"])
def test_fpn_merge_from_bf16_maps(dev, FF, coarse_hw):
    g = _gen(7400)
    lat = (torch.randn(2, 6, 10, 64, generator=g) * 1.5).to(BF16)
    coarse = (torch.randn(2, *coarse_hw, 64, generator=g) * 1.5).to(BF16)
    p16 = FF.fpn_merge_in_bf16(lat.to(dev), coarse.to(dev))
    assert p16.dtype == BF16 and p16.shape == lat.shape
    ref, mag = merge64(lat.double(), coarse.double())
    _within(p16, ref, 8 * U32 * mag + U16 * ref.abs(), f"merge from bf16 maps, coarse {coarse_hw}")
    # the fp32-input entry on the same values widened gives the same bits: same weights, same arithmetic, one rounding
    _, q16 = FF.fpn_merge_bf16(lat.float().to(dev), coarse.float().to(dev), want_f32=False)
    assert torch.equal(_bits(p16), _bits(q16))


# ---- the neck at full widths --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def neck_case(dev):
    """modules built directly at the full widths, six random bf16 maps for N = 1, a rectangular mask"""
    att1, att2 = _att_module(512, 7500, dev), _att_module(256, 7501, dev)
    torch.manual_seed(7502)
    lat1, lat2 = torch.nn.Conv2d(256, 512, 1).to(dev).eval(), torch.nn.Conv2d(128, 512, 1).to(dev).eval()
    g = _gen(7503)
    maps = [torch.randn(1, s, s, c, generator=g).to(BF16) for s, c in ((64, 128), (64, 128), (32, 256), (32, 256), (16, 512), (16, 512))]
    mask = torch.zeros(1, 256, 256)
    mask[:, 100:220, 60:200] = 1
    mods = torch.nn.ModuleList([att1, att2, lat1, lat2])
    for p_ in mods.parameters():
        p_.requires_grad_(False)
    return mods, maps, mask


def _run_neck(dev, neck_case, mode):
    from face_mask_inpaint_amd.modules.psp.encoders.psp_encoders import neck_bf16
    from face_mask_inpaint_amd.weights import weight_scope

    mods, maps, mask = neck_case
    att1, att2, lat1, lat2 = mods
    c1, r1, c2, r2, c3, r3 = (t.to(dev) for t in maps)
    with torch.no_grad(), weight_scope(mods):
        if mode == "noref":
            return neck_bf16(None, None, lat1, lat2, c1, c2, c3)
        a1, a2 = (att1, att2) if mode == "attention" else (None, None)
        return neck_bf16(a1, a2, lat1, lat2, c1, c2, c3, r1, r2, r3, mask.to(dev))


@pytest.mark.parametrize("mode", ["attention", "blend", "noref"])
def test_neck_at_full_widths(dev, FF, neck_case, mode):
    mods, maps, mask = neck_case
    att1, att2, lat1, lat2 = mods
    out = _run_neck(dev, neck_case, mode)
    assert [tuple(t.shape) for t in out] == [(1, 16, 16, 512), (1, 32, 32, 512), (1, 64, 64, 512)] and all(t.dtype == BF16 for t in out)
    c1, r1, c2, r2, c3, r3 = (t.double() for t in maps)
    masks = None
    if mode != "noref":  # the masks the kernels read: the library's own fp32 resizes
        md = mask.to(dev).unsqueeze(-1)
        masks = [_d(FF.resize_bilinear(md, s, s)).reshape(1, s, s) for s in (16, 32, 64)]
        assert all(bool((mm == 0).any()) and bool((mm == 1).any()) for mm in masks)
    else:
        r1 = r2 = r3 = None
    W = neck_weights(att1, att2, lat1, lat2, lambda w: w.to(BF16))
    ref, mags, reds = neck64(W, c1, c2, c3, r1, r2, r3, masks, mode == "attention", _id)
    emul, _, _ = neck64(W, c1, c2, c3, r1, r2, r3, masks, mode == "attention", _rd)
    for name, got, rf, em, mag, red in zip(("coarse", "middle", "fine"), out, ref, emul, mags, reds):
        if red == 0:
            assert torch.equal(_bits(got), _bits(maps[4])), "without a reference the coarse map is the tap itself"
            continue
        _criterion(got, rf, em, (red + 8) * U32 * float(mag.max()), f"neck [{mode}] {name}")
    again = _run_neck(dev, neck_case, mode)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(out, again)), "two calls differ"


# ---- whole encoder -----------------------------------------------------------------------------------------------------------------------
WIDTHS, SPATIAL = (64, 64, 64, 128, 128), (16, 32, 64)


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


def _encoder(dev, dtype, neck=None, seed=76, frozen=False, use_attention=True):
    from face_mask_inpaint_amd.modules.psp.encoders.psp_encoders import GradualStyleEncoder

    opts = SimpleNamespace(n_styles=10, use_attention=use_attention, encoder_eval_dtype=dtype, style_heads_eval_dtype=dtype)
    if neck is not None:
        opts.encoder_neck_eval_dtype = neck
    torch.manual_seed(seed)
    enc = GradualStyleEncoder(50, "ir_se", opts, _widths=WIDTHS, _spatial=SPATIAL)
    _randomise(enc, _gen(seed + 1))
    if frozen:
        for p_ in enc.parameters():
            p_.requires_grad_(False)
    return enc.to(dev).eval()


def _inputs(dev, seed=77, nb=1):
    g = _gen(seed)
    xs, rf = torch.rand(nb, 3, 256, 256, generator=g) * 2 - 1, torch.rand(nb, 3, 256, 256, generator=g) * 2 - 1
    m = torch.zeros(nb, 256, 256)
    m[:, 100:220, 60:200] = 1
    return xs.to(dev), rf.to(dev), m.to(dev)


def test_whole_encoder(dev, FF):
    """one source + one reference image at 256^2 (T = 256 and 1024 at the (32, 128) attention): the all-bf16 build against the fp32 eval
    build within 3e-2 of the codes' range (the bound of test_gpu_irse_infer_bf16.py::test_whole_body)"""
    e16, e32 = _encoder(dev, "bf16", "bf16"), _encoder(dev, "fp32", "fp32")
    assert e16.eval_neck_dtype == BF16 and e32.eval_neck_dtype == torch.float32
    assert list(e16.state_dict()) == list(e32.state_dict()) and all(torch.equal(v, e32.state_dict()[k]) for k, v in e16.state_dict().items())
    inp = _inputs(dev)
    forms = {"attention": lambda e: e(inp[0], ref=inp[1], mask=inp[2]), "no reference": lambda e: e(inp[0])}
    for name, run in forms.items():
        with torch.no_grad():
            c16, c32 = run(e16), run(e32)
        assert c16.shape == (1, 10, 128) and c16.dtype == torch.float32 and bool(torch.isfinite(c16).all())
        share = float((c16 - c32).abs().max()) / float(c32.abs().max())
        print(f"whole encoder [{name}]: all-bf16 vs fp32 eval, max |d codes| = {share:.3g} of the codes' range")
        assert share <= 3e-2, share
        with torch.no_grad():
            assert torch.equal(run(e16), c16), "two bf16 forwards differ"
    e16.train(), e32.train()  # training mode is the fp32 path whatever the eval options say, bit for bit
    with torch.no_grad(), FF.deterministic(True):
        assert torch.equal(forms["attention"](e16), forms["attention"](e32))


def test_whole_encoder_without_attention(dev):
    e16, e32 = _encoder(dev, "bf16", "bf16", use_attention=False), _encoder(dev, "fp32", None, use_attention=False)
    inp = _inputs(dev)
    with torch.no_grad():
        c16, c32 = e16(inp[0], ref=inp[1], mask=inp[2]), e32(inp[0], ref=inp[1], mask=inp[2])
    share = float((c16 - c32).abs().max()) / float(c32.abs().max())
    print(f"whole encoder [blends]: all-bf16 vs fp32 eval, max |d codes| = {share:.3g} of the codes' range")
    assert share <= 3e-2, share


# ---- launch ledger -------------------------------------------------------------------------------------------------------------------------
def _ledger(dev, monkeypatch, neck):
    """the library calls of the third forward of a frozen encoder with body and heads bf16: (stem, neck, tap pointers of the tails) --
    stem = the calls in front of the body's first convolution, neck = the calls behind the body's last tail that are not the heads'"""
    from face_mask_inpaint_amd import _lib

    enc, inp = _encoder(dev, "bf16", neck, frozen=True), _inputs(dev)
    with torch.no_grad():
        for _ in range(2):  # packs and folded constants are made here; the body's packs once more when its marks have taken effect
            enc(inp[0], ref=inp[1], mask=inp[2])
    L = _lib.lib()
    calls, taps = [], []
    with monkeypatch.context() as mp:
        for name in _lib.SIGNATURES:
            fn = getattr(L, name[4:])
            mp.setattr(L, name[4:], (lambda f, nm: lambda *a: (calls.append(nm), taps.append(a[7]) if nm == "fmi_irse_tail_bf16" else None, f(*a))[2])(fn, name))
        with torch.no_grad():
            enc(inp[0], ref=inp[1], mask=inp[2])
    first_body = calls.index("fmi_conv2d_fwd_chan_bf16")
    last_tail = len(calls) - 1 - calls[::-1].index("fmi_irse_tail_bf16")
    return calls[:first_body], [c for c in calls[last_tail + 1:] if c != "fmi_conv2d_grouped_fwd_bf16"], taps


STEM_BF16 = ["fmi_irse_stem_fwd_bf16"]
STEM_FP32, NECK_FP32 = 4, 19  # convolution, BatchNorm, PReLU, hand-over; 3 resizes, 4 per attention, 3 for the blend, 2 laterals, 3 merges
NECK_BF16 = (["fmi_resize_bilinear_f32"] * 3 + ["fmi_conv2d_fwd_bf16", "fmi_guided_attention_fwd_bf16", "fmi_conv2d_fwd_chan_bf16"] * 2
             + ["fmi_mask_blend_bf16"] + ["fmi_conv2d_fwd_chan_bf16", "fmi_fpn_merge_in_bf16"] * 2)


def test_launches_of_stem_and_neck(dev, monkeypatch):
    """DESIGN.md "The bf16 stem and neck (inference)", the launch ledger: the stem is 1 library call where the fp32 form takes 4, the neck
    14 where the fp32 form takes NECK_FP32; no tail of the body writes an fp32 tap"""
    stem, neck, taps = _ledger(dev, monkeypatch, "bf16")
    stem32, neck32, taps32 = _ledger(dev, monkeypatch, "fp32")
    print(f"bf16: stem {len(stem)}: {stem}\n      neck {len(neck)}: {neck}")
    print(f"fp32: stem {len(stem32)}: {stem32}\n      neck {len(neck32)}: {neck32}")
    assert stem == STEM_BF16, stem
    assert neck == NECK_BF16 and len(neck) == 14, neck
    assert len(taps) == 24 and all(t is None for t in taps), "a tail wrote an fp32 tap"
    assert len(stem32) == STEM_FP32 and len(neck32) == NECK_FP32, (len(stem32), len(neck32))
    assert sum(t is not None for t in taps32) == 3


# ---- harness -------------------------------------------------------------------------------------------------------------------------------
def test_psp_inference_all_bf16(dev, tmp_path):
    from face_mask_inpaint_amd import psp_inference as PI

    out = str(tmp_path / "neck")
    flags = ["--encoder_dtype", "bf16", "--style_heads_dtype", "bf16", "--neck_dtype", "bf16", "--use_ref", "--use_attention", "1"]
    torch.manual_seed(12)
    ssim, ms = PI.main(flags + ["--output_size", "256", "--num_batches", "1", "--batch_size", "2", "--out_dir", out])
    assert ssim == ssim and ms == ms and -1.0 <= ssim <= 1.0 and -1.0 <= ms <= 1.0
    assert sorted(os.listdir(out)) == ["gen_0.jpg", "gen_1.jpg", "metrics.csv"]
    rows = list(csv.reader(open(os.path.join(out, "metrics.csv"))))
    assert rows[0] == ["ssim", "ms_ssim"] and (float(rows[1][0]), float(rows[1][1])) == (ssim, ms)


def test_psp_inference_default_is_the_build_without_the_option(dev, FF):
    """without --neck_dtype the run builds exactly what an options object WITHOUT the new attribute builds -- the only form before the
    option existed -- and computes the same bits (reproducible mode); body and heads bf16 in both, so that the neck is what differs"""
    from face_mask_inpaint_amd import psp_inference as PI
    from face_mask_inpaint_amd.modules.mask_detector import MaskDetector
    from face_mask_inpaint_amd.modules.pluralistic_model import base_function
    from face_mask_inpaint_amd.modules.psp.psp import pSp

    args = PI.get_args(["--output_size", "256", "--use_ref", "--use_attention", "1", "--encoder_dtype", "bf16", "--style_heads_dtype", "bf16"])
    assert args.neck_dtype == "fp32"
    g = _gen(14)
    src, rf = (torch.rand(2, 3, 256, 256, generator=g) * 2 - 1).to(dev), (torch.rand(2, 3, 256, 256, generator=g) * 2 - 1).to(dev)
    m = torch.zeros(2, 256, 256, device=dev)
    m[:, 100:220, 60:200] = 1
    outs = []
    with FF.deterministic(True):
        for plain in (False, True):
            torch.manual_seed(15)
            if plain:
                MaskDetector(n_channels=3, bilinear=True)  # build() makes the detector first: the same draws from the host generator
                opts = SimpleNamespace(**{k: v for k, v in vars(args).items() if k != "neck_dtype"})
                opts.encoder_eval_dtype, opts.style_heads_eval_dtype, opts.encoder_dtype = "bf16", "bf16", "fp32"
                assert not hasattr(opts, "encoder_neck_eval_dtype")
                G = pSp(opts).to(dev).eval()
                base_function._freeze(G.encoder)
                with torch.no_grad():
                    G.latent_avg = G.decoder.mean_latent(int(1e5))[0].detach()
            else:
                G, _ = PI.build(args, dev)
            assert G.encoder.eval_neck_dtype == torch.float32 and G.encoder.eval_body_dtype == BF16
            out, lat = G.infer(src, ref=rf, src_mask=m, want=("pooled",))
            outs.append((out["pooled"], lat))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
