"""GPU: the bf16 inference form of the IR-SE body -- the convolution with a per-column output stage (csrc/conv_bf16.hip, EpChanB), the
one-launch SE gate, the block tail and the stem hand-over (csrc/irse_infer_bf16.hip), the four block kinds, the whole body, the kept
constants and the inference harness.

Kernel by kernel the yardstick is float64 computed here from the very operands the kernel read (bf16 values widened, fp32 parameters
widened).  Bounds are derived as in test_gpu_irse_kernels.py, u32 = 2^-24, u16 = 2^-8, mag = the reference with every term replaced by
its absolute value:
  convolution v       (T + 8) u32 mag |scale| + 8 u32 (mag |scale| + |bias|), T = kh kw C terms accumulated in fp32 in an order the MFMA
                      and the reduction loop choose
  activation y        v sits within tol_v of the kink only where |v| <= tol_v; taking the other side there moves y by |1 - slope| tol_v:
                      (1 + 2 |slope|) tol_v + u16 |y|  (one bf16 rounding)
  column sums         the sum of tol_v over the sample's pixels + (11 + 8) u32 sum |v| (8 rows per lane, 3 shuffle steps; the finish of
                      the partial rows is done here in float64)
  gate                the partial rows are operands; pooled (B + 8) u32 mag for B partial rows; through fc1 (C terms), ReLU (1-Lipschitz),
                      fc2 (C / 16 terms) and the sigmoid (1/4-Lipschitz, + 16 u32 for expf and the quotient)
  tail / stem         8 u32 mag + u16 |ref| per bf16 output, 8 u32 mag for the fp32 tap; z is an expression of the fp32 y: 16 u32 mag
Blocks and the whole body chain several bf16 roundings; there the criterion is the issue's: e = max |out - float64 restatement|, e_emul
the same for a float64 restatement that rounds to bf16 where the kernels do (hand-over, conv1 + PReLU, conv2 + BatchNorm, shortcut
convolution, tail y and z), and e_hip <= 2 e_emul + the fp32 accumulation floor (9 C + 8) u32 max |ref| (2: summation order moves ties)."""
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
ROWS = 64  # FMI_CHAN_COLSUM_ROWS


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


def _rd(t):
    return t.to(BF16).double()


# ---- convolution with a per-column output stage ----------------------------------------------------------------------------------
CONV_GEOM = {"3x3s1": (3, 36, 36, 64, 64, 3, 1, 1), "3x3s2": (3, 36, 36, 64, 64, 3, 2, 1), "1x1s2": (3, 36, 36, 64, 128, 1, 2, 0),
             "small": (2, 8, 8, 128, 128, 3, 1, 1)}
_conv_cache = {}


def _conv_case(name):
    """operands and the float64 accumulator, once per geometry (never modified)"""
    if name not in _conv_cache:
        n, h, w, c, k, kk, s, p = CONV_GEOM[name]
        gen = torch.Generator().manual_seed(600 + len(name) + h + k + s)
        x = torch.randn(n, h, w, c, generator=gen).to(BF16)
        wt = (torch.randn(k, c, kk, kk, generator=gen) / (c * kk * kk) ** 0.5).to(BF16)
        sign = (torch.randint(0, 2, (k,), generator=gen) * 2 - 1).float()
        scale = (torch.rand(k, generator=gen) + 0.5) * sign  # both signs
        bias = torch.rand(k, generator=gen) * 2 - 1
        slope = torch.rand(k, generator=gen) * 0.6 - 0.1
        slope[0], slope[1], slope[2], slope[3] = 0.0, -0.25, 1.5, 1.0  # zero, negative, above one, identity
        x64, w64 = x.double().permute(0, 3, 1, 2), wt.double()
        acc = F.conv2d(x64, w64, stride=s, padding=p).permute(0, 2, 3, 1).contiguous()
        mag = F.conv2d(x64.abs(), w64.abs(), stride=s, padding=p).permute(0, 2, 3, 1).contiguous()
        _conv_cache[name] = (x, wt, scale, bias, slope, acc, mag)
    return _conv_cache[name]


def _finish_colsum(part, n, p, k):
    """the documented layout, finished in float64: sample i owns blocks i p / 64 .. ((i + 1) p - 1) / 64, slot = i - (sample of the
    block's first row)"""
    part = _d(part).reshape(-1, 2, k)
    out = torch.zeros(n, k, dtype=F64)
    for i in range(n):
        for b in range(i * p // ROWS, ((i + 1) * p - 1) // ROWS + 1):
            out[i] += part[b, i - (b * ROWS) // p]
    return out


@pytest.mark.parametrize("null", ["none", "scale", "bias", "slope"])
@pytest.mark.parametrize("name", list(CONV_GEOM))
def test_conv_chan(dev, FF, lib, name, null):
    from face_mask_inpaint_amd._lib import FmiError

    n, h, w, c, k, kk, s, p = CONV_GEOM[name]
    x, wt, scale, bias, slope, acc, mag = _conv_case(name)
    scale, bias, slope = (None if null == "scale" else scale), (None if null == "bias" else bias), (None if null == "slope" else slope)
    sc64 = scale.double() if scale is not None else torch.ones(k, dtype=F64)
    bs64 = bias.double() if bias is not None else torch.zeros(k, dtype=F64)
    sl64 = slope.double() if slope is not None else torch.ones(k, dtype=F64)
    v = acc * sc64 + bs64
    v_mag = mag * sc64.abs() + bs64.abs()
    tol_v = (kk * kk * c + 8) * U32 * mag * sc64.abs() + 8 * U32 * v_mag
    y_ref = torch.where(v > 0, v, sl64 * v)
    tol_y = (1 + 2 * sl64.abs()) * tol_v + U16 * y_ref.abs()
    oh, ow = acc.shape[1], acc.shape[2]
    rows, pix = n * oh * ow, oh * ow
    d, _, _ = FF.conv_desc(n, h, w, c, k, kk, kk, s, p)
    xd = x.to(dev)
    wnk = wt.permute(0, 2, 3, 1).reshape(k, kk * kk, c).contiguous().to(dev)
    dv = lambda t: None if t is None else t.to(dev)
    sd, bd, ld = dv(scale), dv(bias), dv(slope)
    what = f"conv+chan {name} null={null}"

    def run(colsum):
        y = _nan((n, oh, ow, k), dev, BF16)
        part = _nan((-(-rows // ROWS) * 2 * k,), dev) if colsum else None
        lib.conv2d_fwd_chan_bf16(ctypes.byref(d), _vp(xd), _vp(wnk), _vp(sd), _vp(bd), _vp(ld), _vp(y), _vp(part),
                                 0 if part is None else part.numel(), FF._st())
        return y, part

    if pix < 128:  # the small-map side: the sums are refused, the convolution itself runs, and the host pools instead
        with pytest.raises(FmiError, match="unsupported"):
            run(True)
        y, _ = run(False)
        _within(y, y_ref, tol_y, what + " y")
        y2, part = FF.conv2d_chan_bf16(xd, wnk, kk, kk, s, p, scale=sd, bias=bd, slope=ld, colsum=True)
        assert part is None and torch.equal(y2, y)
        return
    assert rows % 128 != 0 and pix % 128 != 0  # tiles straddle samples and the last tile is partly empty
    y, part = run(True)
    _within(y, y_ref, tol_y, what + " y")
    assert not bool(torch.isnan(part).any()), what + ": a row of the column-sum workspace was not written"
    sums = _finish_colsum(part, n, pix, k)
    ref = v.reshape(n, pix, k).sum(1)
    tol_s = tol_v.reshape(n, pix, k).sum(1) + (11 + 8) * U32 * v.abs().reshape(n, pix, k).sum(1)
    _within(sums, ref, tol_s, what + " column sums")
    y_again, part_again = run(True)
    assert torch.equal(y, y_again) and torch.equal(part, part_again), what + ": two calls differ"
    y_plain, _ = run(False)
    assert torch.equal(y, y_plain), what + ": the column sums change y"


# ---- SE gate ---------------------------------------------------------------------------------------------------------------------
def _gate_ref(pooled, d_pooled, fc1, fc2):
    """float64 gate and its bound from a pooled vector known to d_pooled"""
    c = pooled.shape[1]
    f1, f2 = fc1.double().reshape(-1, c), fc2.double().reshape(c, -1)
    hpre = pooled @ f1.T
    d_h = d_pooled @ f1.abs().T + (c + 8) * U32 * (pooled.abs() @ f1.abs().T)
    hid = hpre.clamp_min(0)
    s = hid @ f2.T
    d_s = d_h @ f2.abs().T + (f2.shape[1] + 8) * U32 * (hid @ f2.abs().T)
    return torch.sigmoid(s), 0.25 * d_s + 16 * U32


@pytest.mark.parametrize("c", [64, 512])
@pytest.mark.parametrize("p", [64, 1296])  # one partial row per sample; 20.25 of them: blocks straddle samples
def test_se_gate(dev, FF, lib, c, p):
    n = 3
    gen = torch.Generator().manual_seed(700 + c + p)
    v = torch.randn(n * p, c, generator=gen).double() + torch.arange(1, n + 1).repeat_interleave(p).reshape(-1, 1) * 0.5
    nblk = -(-n * p // ROWS)
    part = torch.zeros(nblk, 2, c, dtype=F64)
    for b in range(nblk):
        first = b * ROWS // p
        for r in range(b * ROWS, min((b + 1) * ROWS, n * p)):
            part[b, r // p - first] += v[r]
    part = part.float()  # the operands
    unused = torch.ones(nblk, 2, dtype=torch.bool)
    for i in range(n):
        for b in range(i * p // ROWS, ((i + 1) * p - 1) // ROWS + 1):
            unused[b, i - b * ROWS // p] = False
    part[unused] = float("nan")  # a slot no sample owns must not be read
    fc1 = torch.randn(c // 16, c, 1, 1, generator=gen) / c ** 0.5 * 4
    fc2 = torch.randn(c, c // 16, 1, 1, generator=gen) / (c // 16) ** 0.5 * 2
    p64 = torch.nan_to_num(part.double(), nan=0.0)
    sums = _finish_colsum(p64, n, p, c)
    mags = _finish_colsum(p64.abs(), n, p, c)
    nb = -(-p // ROWS) + 1
    g_ref, tol = _gate_ref(sums / p, (nb + 8) * U32 * mags / p + 4 * U32 * sums.abs() / p, fc1, fc2)
    gates = _nan((n, c), dev)
    part_d, fc1_d, fc2_d = part.to(dev), fc1.to(dev), fc2.to(dev)  # held: the library sees raw pointers
    lib.se_gate_f32(_vp(part_d), ROWS, p, 1.0 / p, _vp(fc1_d), _vp(fc2_d), _vp(gates), n, c, FF._st())
    _within(gates, g_ref, tol, f"SE gate C={c} P={p}")
    assert float((g_ref.max() - g_ref.min())) > 0.2  # the gates are not a constant
    # finished means in place of partial rows (the small-map side)
    pooled = (sums / p).float()
    gates2, pooled_d = _nan((n, c), dev), pooled.to(dev)
    lib.se_gate_f32(_vp(pooled_d), 0, p, 1.0, _vp(fc1_d), _vp(fc2_d), _vp(gates2), n, c, FF._st())
    g2, tol2 = _gate_ref(pooled.double(), 4 * U32 * pooled.double().abs(), fc1, fc2)
    _within(gates2, g2, tol2, f"SE gate from means C={c} P={p}")


def test_se_gate_small_map(dev, FF):
    """FF.se_gate without partial sums: fmi_global_avgpool_bf16 of the rounded map, then the gate launch"""
    n, h, w, c = 2, 8, 8, 128
    gen = torch.Generator().manual_seed(733)
    r = torch.randn(n, h, w, c, generator=gen).to(BF16)
    fc1, fc2 = torch.randn(c // 16, c, 1, 1, generator=gen) / c ** 0.5 * 4, torch.randn(c, c // 16, 1, 1, generator=gen)
    gates = FF.se_gate(r.to(dev), None, fc1.to(dev), fc2.to(dev))
    r64 = r.double().reshape(n, h * w, c)
    g_ref, tol = _gate_ref(r64.mean(1), (h * w + 8) * U32 * r64.abs().mean(1), fc1, fc2)
    _within(gates, g_ref, tol, "SE gate small map")


# ---- block tail and stem hand-over ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", [1, 2])
@pytest.mark.parametrize("gate", [True, False])
@pytest.mark.parametrize("z", [True, False])
@pytest.mark.parametrize("tap", [True, False])
def test_tail(dev, FF, ss, gate, z, tap):
    n, oh, ow, c = 3, 5, 7, 64
    assert (n * oh * ow) % 8 != 0
    sh, sw = (oh, ow) if ss == 1 else (2 * oh - 1, 2 * ow - 1)
    gen = torch.Generator().manual_seed(800)
    r = torch.randn(n, oh, ow, c, generator=gen).to(BF16)
    sc = torch.randn(n, sh, sw, c, generator=gen).to(BF16)
    g = (torch.rand(n, c, generator=gen) + 0.5) * 3.0 ** torch.arange(n).reshape(n, 1)  # a wrong sample index is O(1) wrong
    ns, nsh = torch.randn(c, generator=gen), torch.randn(c, generator=gen)
    g64 = g.double().reshape(n, 1, 1, c) if gate else torch.ones(n, 1, 1, c, dtype=F64)
    s64 = sc.double()[:, ::ss, ::ss]
    y_ref = r.double() * g64 + s64
    y_mag = (r.double() * g64).abs() + s64.abs()
    z_ref = y_ref * ns.double() + nsh.double()
    z_mag = y_mag * ns.double().abs() + nsh.double().abs()
    y, zz, t = FF.irse_tail_bf16(r.to(dev), g.to(dev) if gate else None, sc.to(dev), ns.to(dev) if z else None, nsh.to(dev) if z else None, tap, ss)
    what = f"tail ss={ss} gate={gate} z={z} tap={tap}"
    _within(y, y_ref, 8 * U32 * y_mag + U16 * y_ref.abs(), what + " y")
    assert (zz is not None) == z and (t is not None) == tap
    if z:
        _within(zz, z_ref, 16 * U32 * z_mag + U16 * z_ref.abs(), what + " z")
    if tap:
        assert t.dtype == torch.float32
        _within(t, y_ref, 8 * U32 * y_mag, what + " tap")
        assert torch.equal(t.to(BF16), y), what + ": y is not the tap rounded once"


def test_stem_handover(dev, FF):
    rows, c = 3 * 5 * 7, 64
    gen = torch.Generator().manual_seed(801)
    x = torch.randn(rows, c, generator=gen)
    s, t = torch.randn(c, generator=gen), torch.randn(c, generator=gen)
    y, z = FF.irse_stem_bf16(x.to(dev), s.to(dev), t.to(dev))
    assert torch.equal(y.cpu(), x.to(BF16))
    z_ref = x.double() * s.double() + t.double()
    _within(z, z_ref, 8 * U32 * ((x.double() * s.double()).abs() + t.double().abs()) + U16 * z_ref.abs(), "stem z")


# ---- float64 restatement of the eval block (plain torch, NCHW) ---------------------------------------------------------------------
def _fold64(bn):
    s = _d(bn.weight) / torch.sqrt(_d(bn.running_var) + bn.eps)
    return s.reshape(1, -1, 1, 1), (_d(bn.bias) - _d(bn.running_mean) * s).reshape(1, -1, 1, 1)


def _w64(conv):
    return _rd(conv.weight.detach().cpu())  # the bf16 pack the kernels read


def _block64(blk, x, z, next_bn, rd):
    """eval bottleneck_IR / bottleneck_IR_SE: x the block's input, z = res_layer[0](x) as handed in; rd rounds where the kernels store
    bf16 (identity: the float64 yardstick).  Returns (y stored, z' stored, y before its rounding = the tap)"""
    from torch.nn import MaxPool2d

    res, st = blk.res_layer, blk._stride
    r = F.conv2d(z, _w64(res[1]), stride=1, padding=1)
    a = _d(res[2].weight).reshape(1, -1, 1, 1)
    r = rd(torch.where(r > 0, r, a * r))
    s, t = _fold64(res[4])
    v = F.conv2d(r, _w64(res[3]), stride=st, padding=1) * s + t
    g = 1.0
    if len(res) > 5:
        c = v.shape[1]
        hid = (v.mean((2, 3)) @ _d(res[5].fc1.weight).reshape(-1, c).T).clamp_min(0)
        g = torch.sigmoid(hid @ _d(res[5].fc2.weight).reshape(c, -1).T).reshape(v.shape[0], c, 1, 1)
    if isinstance(blk.shortcut_layer, MaxPool2d):
        sc = x[:, :, ::st, ::st]
    else:
        s, t = _fold64(blk.shortcut_layer[1])
        sc = rd(F.conv2d(x, _w64(blk.shortcut_layer[0]), stride=st) * s + t)
    y = rd(v) * g + sc
    zn = None
    if next_bn is not None:
        s, t = _fold64(next_bn)
        zn = rd(y * s + t)
    return rd(y), zn, y


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


def _nchw(t):
    return _d(t).permute(0, 3, 1, 2)


def _criterion(got_nhwc, ref, emul, cred, what):
    """e_hip <= 2 e_emul + (9 C + 8) u32 max |ref|; returns the ratio for the record"""
    e_hip = float((_nchw(got_nhwc) - ref).abs().max())
    e_emul = float((emul - ref).abs().max())
    floor = (9 * cred + 8) * U32 * float(ref.abs().max())
    print(f"{what}: e_hip {e_hip:.4g}  e_emul {e_emul:.4g}  ratio {e_hip / max(e_emul, 1e-300):.3f}  floor {floor:.3g}  max|ref| {float(ref.abs().max()):.4g}")
    assert e_hip == e_hip and e_hip <= 2 * e_emul + floor, f"{what}: e_hip {e_hip:.4g} > 2 x e_emul {e_emul:.4g} + floor {floor:.3g}"
    return e_hip, e_emul


def _run_block(dev, FF, blk, next_bn, x32, tap=True):
    """the block's inference form on the device from the fp32 map x32 (hand-over, then the block); returns (x, z, y, z', tap)"""
    from face_mask_inpaint_amd.modules.psp.encoders import helpers as H
    from face_mask_inpaint_amd.weights import weight_scope

    with torch.no_grad(), weight_scope(blk):
        x, z = FF.irse_stem_bf16(x32.to(dev), *H.fold_bn_eval(blk.res_layer[0]))
        y, zn, t = blk.infer_bf16(x, z, next_bn, tap=tap)
    return x, z, y, zn, t


def _check_block(dev, FF, blk, next_bn, x32, what):
    x, z, y, zn, t = _run_block(dev, FF, blk, next_bn, x32)
    x64, z64 = _nchw(x), _nchw(z)  # the operands the block read
    cred = blk.res_layer[1].in_channels
    y_ref, z_ref, t_ref = _block64(blk, x64, z64, next_bn, lambda v: v)
    y_em, z_em, t_em = _block64(blk, x64, z64, next_bn, _rd)
    _criterion(t, t_ref, t_em, cred, what + " tap")
    _criterion(y, y_ref, y_em, cred, what + " y")
    _criterion(zn, z_ref, z_em, cred, what + " z")
    assert torch.equal(t.to(BF16), y)


@pytest.mark.parametrize("kind", ["IR_SE(64,64,1)", "IR_SE(64,64,2)", "IR_SE(64,128,2)", "IR(64,128,2)"])
def test_block_kinds(dev, FF, kind):
    from face_mask_inpaint_amd.modules.psp.encoders import helpers as H

    cls, cin, depth, stride = {"IR_SE(64,64,1)": (H.bottleneck_IR_SE, 64, 64, 1), "IR_SE(64,64,2)": (H.bottleneck_IR_SE, 64, 64, 2),
                               "IR_SE(64,128,2)": (H.bottleneck_IR_SE, 64, 128, 2), "IR(64,128,2)": (H.bottleneck_IR, 64, 128, 2)}[kind]
    torch.manual_seed(900 + depth + stride)
    gen = torch.Generator().manual_seed(901 + depth + stride)
    blk, next_bn = cls(cin, depth, stride), torch.nn.BatchNorm2d(depth)
    _randomise(blk, gen), _randomise(next_bn, gen)
    blk, next_bn = blk.to(dev).eval(), next_bn.to(dev).eval()
    x32 = torch.randn(3, 20, 20, cin, generator=gen) * 1.5
    _check_block(dev, FF, blk, next_bn, x32, kind)


def test_block_refuses_widths_the_kernels_do_not_cover(dev, FF):
    from face_mask_inpaint_amd._lib import FmiError
    from face_mask_inpaint_amd.modules.psp.encoders import helpers as H

    blk = H.bottleneck_IR_SE(32, 32, 1).to(dev).eval()
    with pytest.raises(FmiError, match="% 64"):
        _run_block(dev, FF, blk, None, torch.zeros(1, 8, 8, 32))


# ---- kept constants ------------------------------------------------------------------------------------------------------------
def test_kept_constants_follow_a_training_pass(dev, FF):
    """eval bf16 forward (the folded constants are kept: frozen parameters), one training-mode forward that moves the running buffers
    through raw pointers, eval bf16 forward again: the second result is held to the restatement with the NEW statistics"""
    from face_mask_inpaint_amd.modules.psp.encoders import helpers as H
    from face_mask_inpaint_amd.weights import weight_scope

    torch.manual_seed(950)
    gen = torch.Generator().manual_seed(951)
    blk, next_bn = H.bottleneck_IR_SE(64, 64, 1), torch.nn.BatchNorm2d(64)
    _randomise(blk, gen), _randomise(next_bn, gen)
    blk, next_bn = blk.to(dev).eval(), next_bn.to(dev).eval()
    for p_ in list(blk.parameters()) + list(next_bn.parameters()):
        p_.requires_grad_(False)
    x32 = torch.randn(3, 20, 20, 64, generator=gen) * 1.5 + 0.7
    _check_block(dev, FF, blk, next_bn, x32, "before the training pass")
    first = _run_block(dev, FF, blk, next_bn, x32)
    bn0, bn4 = blk.res_layer[0], blk.res_layer[4]
    assert bn0._fmi_infer is not None and bn4._fmi_infer is not None and next_bn._fmi_infer is not None
    old = bn4.running_var.clone()
    blk.train()
    with torch.no_grad(), weight_scope(blk):
        blk.nhwc(x32.to(dev))
    blk.eval()
    assert not torch.equal(old, bn4.running_var) and bn0._fmi_infer is None and bn4._fmi_infer is None
    _check_block(dev, FF, blk, next_bn, x32, "after the training pass")
    second = _run_block(dev, FF, blk, next_bn, x32)
    assert not torch.equal(first[2], second[2])


# ---- whole body ------------------------------------------------------------------------------------------------------------------
def _encoder(dev, eval_dtype, seed=4):
    from face_mask_inpaint_amd.modules.psp.encoders.psp_encoders import GradualStyleEncoder

    torch.manual_seed(seed)
    enc = GradualStyleEncoder(50, "ir_se", SimpleNamespace(n_styles=10, use_attention=True, encoder_eval_dtype=eval_dtype),
                              _widths=(64, 64, 64, 128, 128), _spatial=(4, 8, 16))
    _randomise(enc.body, torch.Generator().manual_seed(seed + 1))
    return enc.to(dev).eval()


def _body64(enc, x_nchw, rd):
    """float64 restatement of input_layer + body from the fp32 image: returns the three taps (the tails' unrounded y)"""
    conv, bn, pr = enc.input_layer
    s, t = _fold64(bn)
    x = F.conv2d(x_nchw, _d(conv.weight), padding=1) * s + t
    a = _d(pr.weight).reshape(1, -1, 1, 1)
    x = torch.where(x > 0, x, a * x)
    s, t = _fold64(enc.body[0].res_layer[0])
    x, z = rd(x), rd(x * s + t)
    taps = {}
    for i, blk in enumerate(enc.body):
        nxt = enc.body[i + 1].res_layer[0] if i + 1 < len(enc.body) else None
        x, z, y = _block64(blk, x, z, nxt, rd)
        if i in (6, 20, 23):
            taps[i] = y
    return taps[6], taps[20], taps[23]


def test_whole_body(dev, FF):
    from face_mask_inpaint_amd.weights import weight_scope

    e16, e32 = _encoder(dev, "bf16"), _encoder(dev, "fp32")
    assert list(e16.state_dict()) == list(e32.state_dict()) and all(torch.equal(v, e32.state_dict()[k]) for k, v in e16.state_dict().items())
    gen = torch.Generator().manual_seed(6)
    nb = 2
    xs, rf = torch.rand(nb, 3, 64, 64, generator=gen) * 2 - 1, torch.rand(nb, 3, 64, 64, generator=gen) * 2 - 1
    m = torch.zeros(nb, 64, 64)
    m[:, 20:50, 12:44] = 1
    both = torch.cat([xs, rf])
    with torch.no_grad(), weight_scope(e16):
        taps = e16._pyramid(FF.to_nhwc(both.to(dev)))
    assert [tuple(t.shape) for t in taps] == [(4, 16, 16, 64), (4, 8, 8, 128), (4, 4, 4, 128)] and all(t.dtype == torch.float32 for t in taps)
    ref = _body64(e16, both.double(), lambda v: v)
    emul = _body64(e16, both.double(), _rd)
    for name, t, r, e in zip(("tap 6", "tap 20", "tap 23"), taps, ref, emul):
        _criterion(t, r, e, 128, "whole body " + name)
    with torch.no_grad():
        c16 = e16(xs.to(dev), ref=rf.to(dev), mask=m.to(dev))
        c32 = e32(xs.to(dev), ref=rf.to(dev), mask=m.to(dev))
    scale, err = float(c32.abs().max()), float((c16 - c32).abs().max())
    print(f"whole body: W+ codes {err / scale:.3g} of their range")
    assert c16.shape == (nb, 10, 128) and err <= 3e-2 * scale, (err, scale)
    # the body has no atomics: with the fp32 parts around it in their reproducible mode, two forwards give the same bits
    with torch.no_grad(), FF.deterministic(True):
        with weight_scope(e16):
            t1, t2 = e16._pyramid(FF.to_nhwc(both.to(dev))), e16._pyramid(FF.to_nhwc(both.to(dev)))
        assert all(torch.equal(a, b) for a, b in zip(t1, t2)), "two bf16 eval passes of the body differ"
        assert torch.equal(e16(xs.to(dev), ref=rf.to(dev), mask=m.to(dev)), e16(xs.to(dev), ref=rf.to(dev), mask=m.to(dev)))
    # training mode is the fp32 body whatever the eval option says, bit for bit
    e16.train(), e32.train()
    with torch.no_grad(), FF.deterministic(True):
        assert torch.equal(e16(xs.to(dev), ref=rf.to(dev), mask=m.to(dev)), e32(xs.to(dev), ref=rf.to(dev), mask=m.to(dev)))


def test_launches_per_block(dev, FF, monkeypatch):
    """4 launches for an identity-shortcut SE block, 5 with a convolution shortcut (frozen weights: the bf16 packs are kept)"""
    from face_mask_inpaint_amd import _lib
    from face_mask_inpaint_amd.modules.psp.encoders import helpers as H
    from face_mask_inpaint_amd.weights import weight_scope

    L = _lib.lib()
    for cin, depth, stride, want in ((64, 64, 1, 4), (64, 64, 2, 4), (64, 128, 2, 5)):
        blk, nxt = H.bottleneck_IR_SE(cin, depth, stride).to(dev).eval(), torch.nn.BatchNorm2d(depth).to(dev).eval()
        for p_ in list(blk.parameters()) + list(nxt.parameters()):
            p_.requires_grad_(False)
        x32 = torch.randn(2, 32, 32, cin)
        _run_block(dev, FF, blk, nxt, x32)  # packs and folded constants are made here
        calls = []
        with monkeypatch.context() as mp:
            for name in _lib.SIGNATURES:
                fn = getattr(L, name[4:])
                mp.setattr(L, name[4:], (lambda f, nm: lambda *a: (calls.append(nm), f(*a))[1])(fn, name))
            with torch.no_grad(), weight_scope(blk):
                x, z = FF.irse_stem_bf16(x32.to(dev), *H.fold_bn_eval(blk.res_layer[0]))
                del calls[:]
                blk.infer_bf16(x, z, nxt)
        assert len(calls) == want, (cin, depth, stride, calls)


# ---- harness -----------------------------------------------------------------------------------------------------------------------
def test_psp_inference_bf16_encoder(dev, FF, tmp_path):
    from face_mask_inpaint_amd import psp_inference as PI

    out = str(tmp_path / "bf16")
    torch.manual_seed(12)
    ssim, ms = PI.main(["--encoder_dtype", "bf16", "--output_size", "256", "--num_batches", "1", "--batch_size", "2", "--out_dir", out])
    assert ssim == ssim and ms == ms and -1.0 <= ssim <= 1.0 and -1.0 <= ms <= 1.0
    assert sorted(os.listdir(out)) == ["gen_0.jpg", "gen_1.jpg", "metrics.csv"]
    rows = list(csv.reader(open(os.path.join(out, "metrics.csv"))))
    assert rows[0] == ["ssim", "ms_ssim"] and (float(rows[1][0]), float(rows[1][1])) == (ssim, ms)
    torch.manual_seed(12)
    G, md = PI.build(PI.get_args(["--encoder_dtype", "bf16", "--output_size", "256", "--use_ref"]), dev)
    assert G.encoder.eval_body_dtype == BF16 and G.encoder.body_dtype == torch.float32
    assert not any(p_.requires_grad for p_ in G.encoder.parameters())
    g = torch.Generator().manual_seed(13)
    src, rf = torch.rand(2, 3, 256, 256, generator=g) * 2 - 1, torch.rand(2, 3, 256, 256, generator=g) * 2 - 1
    res, mask = PI.infer_batch(G, md, (src, rf), dev, want=("pooled", "u8"))
    assert bool(torch.isfinite(res["pooled"]).all()) and res["u8"].shape == (2, 256, 256, 3) and mask.shape == (2, 256, 256)


def test_psp_inference_fp32_default_is_the_build_without_the_option(dev, FF):
    """the default run builds exactly what an options object WITHOUT the new attributes builds -- the only form before the option
    existed -- and computes the same bits (reproducible mode)"""
    from face_mask_inpaint_amd import psp_inference as PI
    from face_mask_inpaint_amd.modules.mask_detector import MaskDetector
    from face_mask_inpaint_amd.modules.psp.psp import pSp

    args = PI.get_args(["--output_size", "256", "--use_ref"])
    assert args.encoder_dtype == "fp32"
    g = torch.Generator().manual_seed(14)
    src, rf = (torch.rand(2, 3, 256, 256, generator=g) * 2 - 1).to(dev), (torch.rand(2, 3, 256, 256, generator=g) * 2 - 1).to(dev)
    m = torch.zeros(2, 256, 256, device=dev)
    m[:, 100:220, 60:200] = 1
    outs = []
    with FF.deterministic(True):
        for plain in (False, True):
            torch.manual_seed(15)
            if plain:
                MaskDetector(n_channels=3, bilinear=True)  # build() makes the detector first: the same draws from the host generator
                opts = SimpleNamespace(**{k: v for k, v in vars(args).items() if k != "encoder_dtype"})
                G = pSp(opts).to(dev).eval()
                with torch.no_grad():
                    G.latent_avg = G.decoder.mean_latent(int(1e5))[0].detach()
            else:
                G, _ = PI.build(args, dev)
            assert G.encoder.eval_body_dtype == torch.float32 and any(p_.requires_grad for p_ in G.encoder.parameters())
            out, lat = G.infer(src, ref=rf, src_mask=m, want=("pooled",))
            outs.append((out["pooled"], lat))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
