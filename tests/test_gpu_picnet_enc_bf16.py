"""GPU: the bf16 PICNet encoders and guided attention -- the stem and 32-channel convolutions, the two tails, fmi_guided_attention_fwd_bf16,
ResBlock / ResBlockEncoderOptimized / ResEncoder / ExampleGuidedAttention / ReferenceFill on bf16 activations, the refusals and the
harness flag.  Conventions (and helpers) of tests/test_gpu_picnet_bf16.py.

Kernel bounds come from two facts: bf16 round-to-nearest errs by at most 2^-8 |v|, fp32 summation of n terms by at most n 2^-24 sum|terms|.
Every float64 reference is computed here on the CPU from the same bf16-rounded inputs and bf16-rounded weights.

Block and model level: a rounding across a LeakyReLU gate makes a bound underivable.  The reference there is an emulation written below
-- float64 with the weights the bf16 kernels round, every tensor the bf16 path stores and the attention probabilities entering P V rounded
to bf16 -- and every compared tensor must lie within 3 x the emulation's own relative L2 error against plain float64."""
import copy
import itertools

import pytest
import torch
import torch.nn.functional as F

from face_mask_inpaint_amd import functional as FF
from face_mask_inpaint_amd._lib import FmiError
from test_gpu_picnet_bf16 import (BF, THR, U8, U24, _adjudicate, _attn_data, _bits, _branches, _count_entry, _fill_params, _gen, _generator64,
                                  _ident, _lrelu, _nchw64, _nhwc, _params64, _perturb, _q, _rel, _within)

pytestmark = pytest.mark.gpu

SLOPE = float(torch.tensor(0.1, dtype=torch.float32))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _wf(wt):
    """torch weight [K][C][kh][kw] -> the forward pack wf[tap][C][K]"""
    k, c, kh, kw = wt.shape
    return wt.permute(2, 3, 1, 0).reshape(kh * kw, c, k).contiguous()


def _lr(x, slope):
    return torch.where(x > 0, x, x * slope)


# ---------------------------------------------------------------------------------------------------------------------------------
# the convolutions
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(2, 8, 16), (1, 10, 36)], ids=["2x8x16", "1x10x36"])
def test_stem_conv_against_float64(dev, n, h, w):
    """lrelu(conv3x3(x) + b, 0.1) from the fp32 image and fp32 weights, C = 3, K = 32: 27 fp32 fmas and the bias add, |dz| <= 30 2^-24
    (sum |w| |x| + |b|); LeakyReLU has slope <= 1 (its own multiplication is one of the 30); then the bf16 rounding of the output"""
    x = torch.randn(n, h, w, 3, generator=_gen(50))
    wt = torch.randn(32, 3, 3, 3, generator=_gen(51)) * 0.3
    b = torch.randn(32, generator=_gen(52)) * 0.2
    x64 = x.double().permute(0, 3, 1, 2)
    z = F.conv2d(x64, wt.double(), b.double(), padding=1)
    mag = F.conv2d(x64.abs(), wt.double().abs(), b.double().abs(), padding=1)
    ref = _lr(z, SLOPE).permute(0, 2, 3, 1)
    pw = FF.PackedWeight(_wf(wt).to(dev), None, 32, 3, 3, 3)
    y = FF.conv2d_thin_in_bf16(x.to(dev), pw, b.to(dev), 0.1)
    assert y.dtype == BF and y.shape == (n, h, w, 32)
    B = 30 * U24 * mag.permute(0, 2, 3, 1)
    print(f"\nstem conv {n} x {h} x {w}:")
    _within("lrelu(conv1 + b)", y, ref, B + U8 * (ref.abs() + B))
    assert float((ref[:, 0] - ref[:, 1]).abs().max()) > 1e-3


_C32_REF = {}


def _c32_case(n, h, w, k, ks):
    """float64 z = conv(x) + b and its magnitude sum |w||x| + |b| for bf16 x and bf16-valued weights, computed once per shape"""
    key = (n, h, w, k, ks)
    if key not in _C32_REF:
        x = (torch.randn(n, h, w, 32, generator=_gen(60)) * 1.5).to(BF)
        wt = (torch.randn(k, 32, ks, ks, generator=_gen(61 + k + ks)) * 0.08).to(BF).float()   # bf16 values: the device pack is exact
        b = torch.randn(k, generator=_gen(62)) * 0.2
        x64 = x.double().permute(0, 3, 1, 2)
        z = F.conv2d(x64, wt.double(), b.double(), padding=ks // 2).permute(0, 2, 3, 1).contiguous()
        mag = F.conv2d(x64.abs(), wt.double().abs(), b.double().abs(), padding=ks // 2).permute(0, 2, 3, 1).contiguous()
        _C32_REF[key] = (x, wt, b, z, mag)
    return _C32_REF[key]


# 4137 tiles of 32 pixels: more than the 4096 tiles that 512 workgroups of four waves take at two tiles per wave, the launcher's cap -- the
# smallest map at which a wave's tile loop runs past its share and the grid no longer grows with the map
C32_SHAPES = [(2, 8, 16, 32, 3), (2, 8, 16, 64, 3), (1, 9, 35, 32, 3), (1, 9, 35, 64, 3), (1, 9, 35, 32, 1), (1, 9, 35, 64, 1)]
C32_CASES = [(s, slope) for s in C32_SHAPES for slope in (0.1, 1.0)] + [((1, 257, 515, 32, 3), 0.1)]


@pytest.mark.parametrize("shape,slope", C32_CASES, ids=lambda v: "%dx%dx%d_K%d_k%d" % v if isinstance(v, tuple) else "slope%g" % v)
def test_c32_conv_against_float64(dev, shape, slope):
    """lrelu(conv(x) + b, slope) on 32 channels: 288 fp32 accumulations of exact bf16 products, the bias add and the slope:
    |dz| <= 290 2^-24 (sum |w| |x| + |b|), then the bf16 rounding.  (1, 9, 35): 315 pixels, a ragged last tile and rows that straddle tiles"""
    n, h, w, k, ks = shape
    x, wt, b, z, mag = _c32_case(*shape)
    s32 = float(torch.tensor(slope, dtype=torch.float32))
    ref = _lr(z, s32)
    pw = FF.PackedWeight(_wf(wt).to(dev), None, k, 32, ks, ks)
    y = FF.conv2d_enc_bf16(x.to(dev), pw, b.to(dev), ks // 2, slope)
    assert y.dtype == BF and y.shape == (n, h, w, k)
    B = 290 * U24 * mag
    print(f"\nc32 conv {shape} slope {slope}:")
    _within("lrelu(conv + b)", y, ref, B + U8 * (ref.abs() + B))
    if ks == 3:   # the zero padding: the border rows are not what the interior gives
        assert float((ref[:, 0] - ref[:, 1]).abs().max()) > 1e-3 and float((ref[:, :, 0] - ref[:, :, 1]).abs().max()) > 1e-3
    y2 = FF.conv2d_enc_bf16(x.to(dev), pw, b.to(dev), ks // 2, slope)
    assert torch.equal(_bits(y), _bits(y2))


# ---------------------------------------------------------------------------------------------------------------------------------
# the tails
# ---------------------------------------------------------------------------------------------------------------------------------
def _pool64(t):
    return F.avg_pool2d(t.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)


@pytest.mark.parametrize("pool", [False, True], ids=["none", "down"])
@pytest.mark.parametrize("c", [32, 128])
def test_resblock_tail_against_float64(dev, c, pool):
    """v = main + shortcut [2x2 mean]: a tree of at most three fp32 additions per term (the factor 1/4 is exact) and the slope's
    multiplication: |dv| <= 6 2^-24 sum |terms|; y_raw and y_act add one bf16 rounding, y_f32 none.  Every subset of outputs."""
    a = (torch.randn(2, 8, 16, c, generator=_gen(70)) * 2).to(BF)
    s = (torch.randn(2, 8, 16, c, generator=_gen(71)) * 2).to(BF)
    v = a.double() + s.double()
    mag = a.double().abs() + s.double().abs()
    if pool:
        v, mag = _pool64(v), _pool64(mag)
    B = 6 * U24 * mag
    outs = {}
    print(f"\nresblock tail C = {c}, pool {pool}:")
    for raw, act, f32 in itertools.product([False, True], repeat=3):
        if not (raw or act or f32):
            with pytest.raises(FmiError, match="bad argument"):
                FF.resblock_tail_bf16(a.to(dev), s.to(dev), pool, 0.1, False, False, False)
            continue
        y_raw, y_act, y_f32 = FF.resblock_tail_bf16(a.to(dev), s.to(dev), pool, 0.1, raw, act, f32)
        assert (y_raw is not None, y_act is not None, y_f32 is not None) == (raw, act, f32)
        for name, t in (("raw", y_raw), ("act", y_act), ("f32", y_f32)):
            if t is None:
                continue
            assert t.shape == v.shape and t.dtype == (torch.float32 if name == "f32" else BF)
            if name in outs:     # the same bits whichever other outputs are written
                assert torch.equal(t.cpu(), outs[name]), (name, raw, act, f32)
            else:
                outs[name] = t.cpu()
    _within("y_raw", outs["raw"], v, B + U8 * (v.abs() + B))
    la = _lr(v, SLOPE)
    _within("y_act", outs["act"], la, B + U8 * (la.abs() + B))
    _within("y_f32", outs["f32"], v, B)


def test_stem_tail_against_float64(dev):
    """pool2(h) + sum_c wb[c][k] pool2(img)[c] + bias, C = 3: no term passes more than five fp32 roundings (two in its 2x2 mean), the slope
    is a sixth: |dv| <= 6 2^-24 sum |terms|"""
    n, h, w, k = 2, 8, 16, 32
    hh = (torch.randn(n, h, w, k, generator=_gen(72)) * 2).to(BF)
    img = torch.randn(n, h, w, 3, generator=_gen(73))
    wb = torch.randn(3, k, generator=_gen(74)) * 0.5
    b = torch.randn(k, generator=_gen(75)) * 0.2
    pi, pia = _pool64(img.double()), _pool64(img.double().abs())
    v = _pool64(hh.double()) + pi @ wb.double() + b.double()
    mag = _pool64(hh.double().abs()) + pia @ wb.double().abs() + b.double().abs()
    B = 6 * U24 * mag
    args = (hh.to(dev), img.to(dev), wb.to(dev), b.to(dev), 0.1)
    y_raw, y_act = FF.picnet_stem_tail_bf16(*args)
    assert y_raw.dtype == y_act.dtype == BF and y_raw.shape == y_act.shape == (n, h // 2, w // 2, k)
    print("\nstem tail:")
    _within("y_raw", y_raw, v, B + U8 * (v.abs() + B))
    la = _lr(v, SLOPE)
    _within("y_act", y_act, la, B + U8 * (la.abs() + B))
    r_only, none = FF.picnet_stem_tail_bf16(*args, raw=True, act=False)
    none2, a_only = FF.picnet_stem_tail_bf16(*args, raw=False, act=True)
    assert none is None and none2 is None and torch.equal(_bits(r_only), _bits(y_raw)) and torch.equal(_bits(a_only), _bits(y_act))
    with pytest.raises(FmiError, match="bad argument"):
        FF.picnet_stem_tail_bf16(*args, raw=False, act=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# fmi_guided_attention_fwd_bf16
# ---------------------------------------------------------------------------------------------------------------------------------
def _soft_mask(n, t, seed):
    m = torch.rand(n, t, generator=_gen(seed))
    m[:, 10:40] = 0.0
    m[:, t - 50:t - 20] = 1.0
    return m


def _guided_call(dev, q, src, ref, m, waves=0):
    n, t, d = q.shape
    c = src.shape[2]
    qd, sd, rd, md = q.to(dev), src.to(dev), ref.to(dev), m.to(dev)     # held until the launch has run
    out = torch.empty((n, t, 2 * c), device=dev, dtype=BF)
    FF._L().guided_attention_fwd_bf16(FF._p(qd), FF._p(sd), FF._p(rd), FF._p(md), FF._p(out), n, t, d, c, waves, FF._st())
    torch.cuda.synchronize()
    return out


GUIDED_CASES = [(2, 128, 0), (1, 384, 0), (3, 256, 0), (1, 128, 4), (1, 256, 8)]     # (N, T, waves); D = 32, C = 128


@pytest.mark.parametrize("kind", ["gauss", "late", "onehot", "equal"])
@pytest.mark.parametrize("shape", GUIDED_CASES, ids=lambda s: "N%d_T%d_w%d" % s)
def test_guided_attention_against_float64(dev, shape, kind):
    """out[..., :C] = (1 - m) (A ref) + m ref, out[..., C:] = A src against float64 from the same bf16 q, src, ref and fp32 m.
    Per half the pre-rounding bound B of test_gpu_picnet_bf16.test_attention_against_float64 (same kernel scheme, same derivation) with
    that half's A = sum p |v| / L.  Second half: |err| <= B + 2^-8 (|o| + B).  First half, y = (1 - m) o + m r with 1 - m, m r and the
    fma each rounded once: |err| <= (1 - m) B + 2 2^-24 |y| + 2^-8 (|y| + (1 - m) B); where m == 1 the result is ref bit for bit."""
    n, t, waves = shape
    d, c = 32, 128
    q, ref_v = _attn_data(kind, n, t, d, c, seed=202)    # the seed at which the "late" preconditions below hold for all five shapes
    src_v = torch.randn(n, t, c, generator=_gen(201)).to(BF)
    m = _soft_mask(n, t, 202)
    q64 = q.double()
    s = q64 @ q64.transpose(1, 2)
    if kind == "late":     # float64-only preconditions of the data: the lazy reference maximum defers, fires and grows late
        fired, deferred, margin = _branches(s)
        grow_end = float((s[:, :, t - 32:].amax(-1) > s[:, :, :t - 32].amax(-1)).float().mean())
        print(f"\n  late: {fired} rescales after the first tile, {deferred} deferrals, nearest test {margin:.3f}, late growth {grow_end:.2f}")
        assert margin > 0.05 and deferred > 0 and grow_end > 0.1 and (fired > 0 or t == 128)
    smax = s.amax(-1, keepdim=True)
    p = torch.exp(s - smax)
    L = p.sum(-1, keepdim=True)
    E = (d * U24 * (q64.abs() @ q64.abs().transpose(1, 2))).amax(-1, keepdim=True)
    R = smax - s.amin(-1, keepdim=True) + THR
    eta = E + 3 * U24 * R + 2.0 ** -22
    nT = t + t // 64

    def half(v):
        v64 = v.double()
        o = (p @ v64) / L
        A = (p @ v64.abs()) / L
        return o, 1.001 * (A * (eta + U8 + nT * U24) + o.abs() * (eta + nT * U24 + 3 * U24))

    o_ref, B_ref = half(ref_v)
    o_src, B_src = half(src_v)
    m64 = m.double().unsqueeze(-1)
    y = (1 - m64) * o_ref + m64 * ref_v.double()
    out = _guided_call(dev, q, src_v, ref_v, m, waves)
    assert out.dtype == BF and out.shape == (n, t, 2 * c)
    print(f"guided attention {shape} {kind}: dispatch {FF._L().guided_attention_fwd_bf16_waves(n, t)} waves")
    _within("(1 - m) A ref + m ref", out[..., :c], y, (1 - m64) * B_ref + 2 * U24 * y.abs() + U8 * (y.abs() + (1 - m64) * B_ref))
    _within("A src", out[..., c:], o_src, B_src + U8 * (o_src.abs() + B_src))
    ones = m == 1.0
    assert int(ones.sum()) >= 30 * n and int((m == 0.0).sum()) >= 30 * n
    assert torch.equal(_bits(out[..., :c])[ones], _bits(ref_v)[ones]), "m == 1 must return ref bit for bit"
    out2 = _guided_call(dev, q, src_v, ref_v, m, waves)
    assert torch.equal(_bits(out), _bits(out2)), "two calls differ"


# ---------------------------------------------------------------------------------------------------------------------------------
# block and model level: float64 against its bf16-storage emulation
# ---------------------------------------------------------------------------------------------------------------------------------
def _sn(P, pre, name):
    from oracle import picnet_cpu as O

    return O.sn_weight(P, f"{pre}{name}.module"), P.get(f"{pre}{name}.module.bias")


def _stem64(P, pre, img, q):
    """ResBlockEncoderOptimized as the bf16 path runs it: conv1 and the bypass read the fp32 image with fp32 weights; lrelu(conv1) and conv2
    are stored in bf16, conv2's weights are rounded.  Returns the unrounded tail value v"""
    (w1, b1), (w2, b2), (wb, bb) = (_sn(P, pre, nm) for nm in ("conv1", "conv2", "bypass"))
    h = q(_lrelu(F.conv2d(img, w1, b1, padding=1)))
    h = q(F.conv2d(h, q(w2), b2, padding=1))
    return F.avg_pool2d(h, 2, 2) + F.conv2d(F.avg_pool2d(img, 2, 2), wb, bb)


def _res64(P, pre, raw, act, q, down=False):
    """ResBlock (norm none) as the bf16 path runs it from the stored pair (raw, act = lrelu(raw)); returns the unrounded tail value v"""
    (w1, b1), (w2, b2), (wb, bb) = (_sn(P, pre, nm) for nm in ("conv1", "conv2", "bypass"))
    h = q(_lrelu(F.conv2d(act, q(w1), b1, padding=1)))
    s = q(F.conv2d(raw, q(wb), bb))
    h = q(F.conv2d(h, q(w2), b2, padding=1))
    v = h + s
    return F.avg_pool2d(v, 2, 2) if down else v


def _encoder64(P, pre, img, kind, q, layers=5, L=6):
    """-> (un-split head o, fp32 from the tail; feature, stored in bf16)"""
    v = _stem64(P, pre + "block0.", img, q)
    for i in range(layers - 1):
        v = _res64(P, f"{pre}encoder{i}.", q(v), q(_lrelu(v)), q, down=i % 2 == 1)
    feat = q(v)
    if kind == "src":
        for i in range(L):
            v = _res64(P, f"{pre}infer_prior{i}.", q(v), q(_lrelu(v)), q)
        o = _res64(P, pre + "prior.", q(v), q(_lrelu(v)), q)
    else:
        o = _res64(P, pre + "posterior.", q(v), q(_lrelu(v)), q)
    return o, feat


def _guided64(P, pre, m, src, ref, q):
    """ExampleGuidedAttention as the bf16 path runs it: the query map and the probabilities entering P V rounded, the row sum not"""
    n, c, h, w = src.shape
    qq = q(F.conv2d(src, q(P[pre + "conv.weight"]))).reshape(n, c // 4, h * w)
    s = qq.transpose(1, 2) @ qq
    p = torch.exp(s - s.amax(-1, keepdim=True))
    L = p.sum(-1, keepdim=True)
    pv = lambda v: ((q(p) @ v.reshape(n, c, h * w).transpose(1, 2)) / L).transpose(1, 2).reshape(n, c, h, w)
    return torch.cat([q((1 - m) * pv(ref) + m * ref), q(pv(src))], dim=1)


def _block(kind, *args, **kw):
    from face_mask_inpaint_amd.modules.pluralistic_model import base_function as BFN

    return getattr(BFN, kind)(*args, None, torch.nn.LeakyReLU(0.1), use_spect=True, **kw)


def test_stem_block_bf16(dev):
    from face_mask_inpaint_amd.weights import weight_scope

    torch.manual_seed(20)
    block = _block("ResBlockEncoderOptimized", 3, 32)
    _perturb(block, 21)
    sd = copy.deepcopy(block.state_dict())
    img = torch.rand(2, 16, 32, 3, generator=_gen(22))
    block.to(dev).eval()
    with torch.no_grad(), weight_scope(block):
        raw, act = block.nhwc_bf16(img.to(dev))
    assert raw.dtype == act.dtype == BF and raw.shape == act.shape == (2, 8, 16, 32)
    emu, ref = (_stem64(_params64(sd), "", _nchw64(img), q) for q in (_q, _ident))
    _adjudicate("ResBlockEncoderOptimized(3 -> 32) at 16 x 32", {
        "raw": (raw.float(), _nhwc(_q(emu)), _nhwc(ref)), "act": (act.float(), _nhwc(_q(_lrelu(emu))), _nhwc(_lrelu(ref)))})


@pytest.mark.parametrize("cin,cout,hid,down,h,w", [(32, 64, 32, False, 16, 16), (64, 128, 64, True, 16, 16), (128, 256, 128, False, 8, 16)],
                         ids=["32_64_none", "64_128_down", "128_256_head"])
def test_res_block_bf16(dev, cin, cout, hid, down, h, w):
    """the three forms of the encoder: the 32-channel kernels, the per-column kernel with the pooled tail, and the head that leaves in fp32"""
    from face_mask_inpaint_amd.weights import weight_scope

    torch.manual_seed(23)
    block = _block("ResBlock", cin, cout, hid, sample_type="down" if down else "none")
    _perturb(block, 24)
    sd = copy.deepcopy(block.state_dict())
    x = torch.randn(2, h, w, cin, generator=_gen(25))
    raw_in, act_in = x.to(BF), _lr(x, SLOPE).to(BF)         # the pair a previous tail stores, each rounded once from the fp32 value
    head = cout == 256
    block.to(dev).eval()
    with torch.no_grad(), weight_scope(block):
        raw, act, f32 = block.nhwc_bf16(raw_in.to(dev), act_in.to(dev), raw=not head, act=not head, f32=head)
    emu, ref = (_res64(_params64(sd), "", _nchw64(raw_in), _nchw64(act_in), q, down) for q in (_q, _ident))
    oh, ow = (h // 2, w // 2) if down else (h, w)
    title = f"ResBlock({cin} -> {cout}, hidden {hid}, {'down' if down else 'none'}) at {h} x {w}"
    if head:
        assert raw is None and act is None and f32.dtype == torch.float32 and f32.shape == (2, oh, ow, cout)
        _adjudicate(title, {"fp32 head": (f32, _nhwc(emu), _nhwc(ref))})
    else:
        assert f32 is None and raw.dtype == act.dtype == BF and raw.shape == act.shape == (2, oh, ow, cout)
        _adjudicate(title, {"raw": (raw.float(), _nhwc(_q(emu)), _nhwc(ref)), "act": (act.float(), _nhwc(_q(_lrelu(emu))), _nhwc(_lrelu(ref)))})


def test_example_guided_attention_bf16(dev):
    from face_mask_inpaint_amd.modules.example_guided_att import ExampleGuidedAttention

    torch.manual_seed(26)
    att = ExampleGuidedAttention(128)
    with torch.no_grad():
        att.conv.weight.mul_(0.6)      # scores of a few units: neither a uniform nor a one-hot attention
    sd = copy.deepcopy(att.state_dict())
    g = _gen(27)
    src, ref_f = torch.randn(2, 8, 16, 128, generator=g).to(BF), torch.randn(2, 8, 16, 128, generator=g).to(BF)
    m = _soft_mask(2, 128, 28).view(2, 8, 16)
    att.to(dev).eval()
    with torch.no_grad():
        out = att.nhwc(m.to(dev), src.to(dev), ref_f.to(dev))
    assert out.dtype == BF and out.shape == (2, 8, 16, 256)
    P = {k: v.double() for k, v in sd.items()}
    emu, ref = (_guided64(P, "", m.double().unsqueeze(1), _nchw64(src), _nchw64(ref_f), q) for q in (_q, _ident))
    _adjudicate("ExampleGuidedAttention(128) at 8 x 16", {"blend half": (out[..., :128].float(), _nhwc(emu[:, :128]), _nhwc(ref[:, :128])),
                                                          "src half": (out[..., 128:].float(), _nhwc(emu[:, 128:]), _nhwc(ref[:, 128:]))})


@pytest.mark.parametrize("kind", ["src", "ref"])
def test_res_encoder_bf16(dev, kind):
    from face_mask_inpaint_amd.modules.pluralistic_model import network

    torch.manual_seed(29)
    e = network.define_e(encoder_type=kind, ngf=32, z_nc=128, img_f=128, L=6, layers=5, norm="none", activation="LeakyReLU", compute_dtype=BF)
    _perturb(e, 30)
    sd = copy.deepcopy(e.state_dict())
    img = torch.rand(1, 64, 128, 3, generator=_gen(31))
    e.to(dev).eval()
    with torch.no_grad():
        o, feat = e.nhwc_raw(img.to(dev))
    assert o.dtype == torch.float32 and o.shape == (1, 8, 16, 256) and feat.dtype == BF and feat.shape == (1, 8, 16, 128)
    (eo, ef), (ro, rf) = (_encoder64(_params64(sd), "", _nchw64(img), kind, q) for q in (_q, _ident))
    _adjudicate(f"ResEncoder({kind}) on a 64 x 128 image", {"feature": (feat.float(), _nhwc(ef), _nhwc(rf)), "head": (o, _nhwc(eo), _nhwc(ro))})


@pytest.mark.parametrize("decoder", [torch.float32, BF], ids=["decoder_fp32", "decoder_bf16"])
def test_reference_fill_feature_bf16_end_to_end(dev, decoder):
    from face_mask_inpaint_amd.modules.model import ReferenceFill
    from oracle import picnet_cpu as O

    torch.manual_seed(32)
    enc_p, dec_p = _fill_params()
    G = ReferenceFill(None, enc_p, dec_p, use_att=True, out_size=(64, 128), decoder_dtype=decoder, feature_dtype=BF)
    _perturb(G, 33)
    sd = copy.deepcopy(G.state_dict())
    g = _gen(34)
    src, ref_img = torch.rand(1, 3, 64, 128, generator=g), torch.rand(1, 3, 64, 128, generator=g)
    mask = torch.zeros(1, 64, 128)
    mask[:, 30:56, 12:100] = 1.0
    eps_p, eps_q = torch.randn(1, 128, 8, 16, generator=g), torch.randn(1, 128, 8, 16, generator=g)
    G.to(dev).eval()
    with torch.no_grad():
        img = G(src.to(dev), ref_img.to(dev), src_mask=mask.to(dev), eps=(eps_p.to(dev), eps_q.to(dev)))
    assert img.dtype == torch.float32 and img.shape == (1, 3, 64, 128)

    def run(q):
        P = _params64(sd)
        o_s, f_s = _encoder64(P, "src_encoder.", src.double(), "src", q)
        o_r, f_r = _encoder64(P, "ref_encoder.", ref_img.double(), "ref", q)
        m = O.scale_img(mask.double().unsqueeze(1), f_s.shape[-2:])
        e = _guided64(P, "attention.", m, f_s, f_r, q)
        dist = lambda o: [o[:, :128], F.softplus(o[:, 128:])]
        zz = O.get_z(dist(o_s), dist(o_r), eps_p.double(), eps_q.double())
        qd = q if decoder == BF else _ident
        return F.adaptive_avg_pool2d(_generator64(P, "decoder.", e, zz, qd), (64, 128))

    emu, ref = run(_q), run(_ident)
    whole = O.reference_fill_forward(_params64(sd), src.double(), ref_img.double(), mask.double(), eps_p.double(), eps_q.double(),
                                     out_size=(64, 128))
    # the float64 side here is the oracle's forward, up to the LeakyReLU slope: the kernels hold 0.1 as an fp32 number (relative 1.5e-8)
    assert _rel(ref, whole.detach()) < 1e-7
    _adjudicate(f"ReferenceFill(feature_dtype=bf16, decoder_dtype={decoder}) on a 64 x 128 pair", {"image": (img, emu.detach(), ref.detach())})


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals on the device, launch budget, harness, checkpoints
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(dev):
    from face_mask_inpaint_amd.modules.model import ReferenceFill

    enc_p, dec_p = _fill_params()
    G = ReferenceFill(None, dict(enc_p), dict(dec_p), feature_dtype=BF).to(dev)
    before = copy.deepcopy(G.state_dict())
    x = torch.rand(1, 3, 64, 128, device=dev)
    with pytest.raises(FmiError, match="inference only"):          # grad mode with trainable parameters
        G(x, x, src_mask=torch.zeros(1, 64, 128, device=dev))
    G.eval()
    x72 = torch.rand(1, 3, 72, 72, device=dev)                     # 72 x 72: a 9 x 9 feature map, 81 tokens
    with torch.no_grad():
        with pytest.raises(FmiError, match="81 tokens"):
            G(x72, x72, src_mask=torch.zeros(1, 72, 72, device=dev))
        with pytest.raises(FmiError, match="multiples of 8"):
            G(x72[..., :68], x72[..., :68], src_mask=torch.zeros(1, 72, 68, device=dev))
        with pytest.raises(FmiError, match="no_prior"):
            G(x, x, src_mask=torch.zeros(1, 64, 128, device=dev), no_prior=True)
    after = G.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), "a refused call advanced the SpectralNorm state"


def _count_all(monkeypatch):
    """every entry of the library object, the way test_gpu_irse_infer_bf16.test_launches_per_block counts"""
    from face_mask_inpaint_amd import _lib

    L, calls = _lib.lib(), []
    for name in _lib.SIGNATURES:
        fn = getattr(L, name[4:])
        monkeypatch.setattr(L, name[4:], (lambda f, nm: lambda *a: (calls.append(nm), f(*a))[1])(fn, name))
    return calls


def test_launches_per_block(dev, monkeypatch):
    """a ResBlock is 4 launches (conv1, bypass, conv2, tail), the stem 3, the guided attention 2.  Counted on the second run inside one
    weight_scope: the first cuts the bf16 weight packs, which a prepared weight keeps"""
    from face_mask_inpaint_amd.modules.example_guided_att import ExampleGuidedAttention
    from face_mask_inpaint_amd.weights import weight_scope

    stem, thin, wide = _block("ResBlockEncoderOptimized", 3, 32), _block("ResBlock", 32, 64, 32), _block("ResBlock", 64, 128, 64, sample_type="down")
    att = ExampleGuidedAttention(128)
    for m in (stem, thin, wide, att):
        m.to(dev).eval()
    img = torch.rand(1, 16, 32, 3, device=dev)
    bf = lambda *s: torch.randn(*s, device=dev).to(BF)
    runs = [(stem, lambda: stem.nhwc_bf16(img), 3), (thin, lambda: thin.nhwc_bf16(bf(1, 8, 16, 32), bf(1, 8, 16, 32)), 4),
            (wide, lambda: wide.nhwc_bf16(bf(1, 8, 16, 64), bf(1, 8, 16, 64)), 4),
            (att, lambda: att.nhwc(torch.rand(1, 8, 16, device=dev), bf(1, 8, 16, 128), bf(1, 8, 16, 128)), 2)]
    with monkeypatch.context() as mp:
        calls = _count_all(mp)
        for module, run, want in runs:
            with torch.no_grad(), weight_scope(module):
                run()
                del calls[:]
                run()
            assert len(calls) == want, calls


def test_picnet_harness_feature_dtype(dev, monkeypatch):
    """The issue asks that 'none of the fp32 convolution forward entries' be called with both flags on bf16; the latent ``generator`` block
    (three convolutions on z at 32 x 32) stays fp32 by the same issue, and so does the mask detector without its own flag.  Asserted here:
    inside the generator's forward the fp32 convolution entries see exactly those three calls, 54 + 1 fewer than with the fp32 feature
    path."""
    from face_mask_inpaint_amd import PICNet_inference as PI
    from face_mask_inpaint_amd.modules.model import ReferenceFill

    guided = _count_entry(monkeypatch, "guided_attention_fwd_bf16", lambda a: a[6])        # T
    b16 = _count_entry(monkeypatch, "attention_fwd_bf16", lambda a: a[7])
    f32 = _count_entry(monkeypatch, "attention_fwd_f32", lambda a: a[7])
    f32p = _count_entry(monkeypatch, "attention_fwd_pieces_f32", lambda a: a[9])
    inside = [False]
    shape = lambda a: (inside[0], a[0]._obj.H, a[0]._obj.W, a[0]._obj.C, a[0]._obj.K)
    convs = [_count_entry(monkeypatch, n, shape) for n in ("conv2d_fwd_f32", "conv2d_thin_fwd_f32", "conv2d_thin_lrelu_fwd_f32")]
    real = ReferenceFill.forward

    def forward(self, *a, **kw):
        inside[0] = True
        try:
            return real(self, *a, **kw)
        finally:
            inside[0] = False

    monkeypatch.setattr(ReferenceFill, "forward", forward)
    in_generator = lambda: sorted(c[1:] for cs in convs for c in cs if c[0])
    s = PI.main(["--num_batches", "1", "--batch_size", "1", "--feature_dtype", "bf16", "--generator_dtype", "bf16"])
    assert s == s and -1.0 <= s <= 1.0
    assert guided == [1024] and b16 == [16384] and not f32 and not f32p
    assert in_generator() == sorted([(32, 32, 256, 256)] * 3), in_generator()      # decoder.generator: conv1, conv2, bypass on z
    for c in [guided, b16, f32, f32p] + convs:
        c.clear()
    s2 = PI.main(["--num_batches", "1", "--batch_size", "1", "--feature_dtype", "bf16"])
    assert s2 == s2 and guided == [1024] and not b16 and sorted(f32 + f32p) == [16384]   # the 16384-token attention is the fp32 one
    for c in [guided, b16, f32, f32p] + convs:
        c.clear()
    s3 = PI.main(["--num_batches", "1", "--batch_size", "1", "--generator_dtype", "bf16"])
    # the fp32 feature path: the 54 convolutions of the two encoders and the attention's query convolution on top of the latent three
    assert not guided and b16 == [16384] and f32 + f32p == [1024] and len(in_generator()) == 3 + 54 + 1
    print(f"\nharness SSIM against the random ground truth: both bf16 {s:.6f}, feature bf16 {s2:.6f}, decoder bf16 {s3:.6f}")


def test_fp32_checkpoint_loads_into_the_bf16_build_and_back(dev, tmp_path):
    from face_mask_inpaint_amd.modules.model import ReferenceFill

    enc_p, dec_p = _fill_params()
    a = ReferenceFill(None, dict(enc_p), dict(dec_p)).to(dev)
    b = ReferenceFill(None, dict(enc_p), dict(dec_p), decoder_dtype=BF, feature_dtype=BF).to(dev)
    torch.save(a.state_dict(), tmp_path / "a.pth")
    b.load_state_dict(torch.load(tmp_path / "a.pth", map_location="cpu", weights_only=True), strict=True)
    torch.save(b.state_dict(), tmp_path / "b.pth")
    back = torch.load(tmp_path / "b.pth", map_location="cpu", weights_only=True)
    sa = a.state_dict()
    assert list(back) == list(sa) and all(torch.equal(back[k], sa[k].cpu()) and back[k].dtype == torch.float32 for k in sa)
    a.load_state_dict(back, strict=True)
