"""GPU: the bf16 PICNet decoder -- fmi_attention_fwd_bf16, the Output block from a bf16 input, ResBlockDecoder / Auto_Attn / ResGenerator /
ReferenceFill on bf16 activations, the refusals and the harness flag.  Conventions of tests/test_gpu_unet_bf16.py.

Kernel bounds come from two facts: bf16 round-to-nearest errs by at most 2^-8 |v|, fp32 summation of n terms by at most n 2^-24 sum|terms|.
Every float64 reference is computed here on the CPU from the same bf16-rounded inputs.

Block and model level: a rounding across a LeakyReLU gate or inside InstanceNorm makes a bound underivable.  The reference there is an
emulation written below -- float64 with the weights the bf16 kernels round, every tensor the bf16 path stores and the attention
probabilities entering P V rounded to bf16 -- and every compared tensor must lie within 3 x the emulation's own relative L2 error
against plain float64.  All three numbers are printed."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

from face_mask_inpaint_amd import functional as FF
from face_mask_inpaint_amd._lib import FmiError

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
U8, U24 = 2.0 ** -8, 2.0 ** -24
THR = 20.0      # ATT_THR of csrc/attention_bf16.hip: the deferred-rescale threshold
KEYS = 64       # keys per tile there, 32 queries per wave


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _within(name, got, ref, bound):
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values"
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"  {name}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert bool((err <= bound).all()), f"{name}: err / bound = {worst}"


# ---------------------------------------------------------------------------------------------------------------------------------
# fmi_attention_fwd_bf16
# ---------------------------------------------------------------------------------------------------------------------------------
def _attn_call(dev, q, v, gamma=None, res=None, waves=0, want_lse=True):
    n, t, d = q.shape
    c = v.shape[2]
    qd, vd = q.to(dev), v.to(dev)
    o = torch.empty_like(vd)
    lse = torch.empty((n, t), device=dev, dtype=torch.float32) if want_lse else None
    g = None if gamma is None else torch.tensor([gamma], device=dev, dtype=torch.float32)
    rd = None if res is None else res.to(dev)
    FF._L().attention_fwd_bf16(FF._p(qd), FF._p(vd), FF._p(o), FF._p(lse), FF._p(g), FF._p(rd), n, t, d, c, waves, FF._st())
    torch.cuda.synchronize()
    return o, lse


def _attn_data(kind, n, t, d, c, seed):
    """q [n,t,d], v [n,t,c] as bf16 values"""
    g = _gen(seed)
    v = torch.randn(n, t, c, generator=g)
    if kind == "gauss":        # (a) score spread of a few units: off-diagonal std ~ 1, diagonal ~ 8
        q = torch.randn(n, t, d, generator=g) * math.sqrt(math.sqrt(1.0 / d))
        q = q * math.sqrt(8.0 / float((q * q).sum(-1).mean()))
    elif kind == "late":       # (b) a common direction of weight 3.5 plus noise; one middle 32-block and the last 32 positions x 3
        u = torch.randn(d, generator=g)
        u = u / u.norm()
        q = 3.5 * u + 0.2 * torch.randn(n, t, d, generator=g)
        q[:, 5:8] = 0.2 * torch.randn(n, 3, d, generator=g)      # rows without growth inside the first 32-row block ...
        q[:, t - 60:t - 57] = 0.2 * torch.randn(n, 3, d, generator=g)   # ... and inside a late one
        mid = t // 2 - 32
        q[:, mid:mid + 32] *= 3.0
        q[:, t - 32:] *= 3.0
    elif kind == "onehot":     # (c) |q|^2 ~ 40
        q = torch.randn(n, t, d, generator=g) * math.sqrt(40.0 / d)
    elif kind == "equal":      # (d) all queries equal: uniform attention
        q = (torch.randn(d, generator=g) * 0.5).expand(n, t, d).clone()
    else:
        raise ValueError(kind)
    return q.to(BF), v.to(BF)


def _branches(s):
    """the kernel's reference-maximum schedule replayed on the float64 scores s [n,t,t]: per group of 32 queries and 64-key tile, the
    rescale fires for the whole group when any of its rows has tile max > reference + THR.  Returns (rescales after the first tile,
    deferrals = tiles in which some row's maximum grew and the group did not rescale, smallest distance of any test from its threshold)"""
    n, t, _ = s.shape
    tmax = s.view(n, t // 32, 32, t // KEYS, KEYS).amax(-1)           # [n, groups, 32, tiles]
    mref = torch.full((n, t // 32, 32), -float("inf"), dtype=torch.float64)
    fired = deferred = 0
    margin = float("inf")
    for k in range(t // KEYS):
        tm = tmax[..., k]
        over = (tm - (mref + THR)).amax(-1)                           # [n, groups]: the wave-uniform test
        if k:
            margin = min(margin, float(over.abs().min()))
        fire = over > 0
        grew = (tm > mref).any(-1)
        if k:
            fired += int(fire.sum())
            deferred += int((grew & ~fire).sum())
        mref = torch.where(fire.unsqueeze(-1), torch.maximum(mref, tm), mref)
    return fired, deferred, margin


ATTN_CASES = [
    # (N, T, D, C, waves, gamma)
    (2, 128, 32, 128, 0, None),     # one 128-key span: two tiles
    (1, 384, 64, 256, 0, None),     # not a power of two
    (3, 256, 64, 256, 0, 0.4),      # epilogue, odd N
    (1, 128, 64, 256, 4, None),     # every variant, requested explicitly at the smallest T it accepts ...
    (1, 256, 64, 256, 8, None),
    (1, 128, 32, 128, 4, 0.4),      # ... in both instantiations
    (1, 256, 32, 128, 8, 0.4),
]


@pytest.mark.parametrize("kind", ["gauss", "late", "onehot", "equal"])
@pytest.mark.parametrize("shape", ATTN_CASES, ids=lambda s: "N%d_T%d_D%d_C%d_w%d_%s" % (s[:5] + ("g" if s[5] else "plain",)))
def test_attention_against_float64(dev, shape, kind):
    """o = softmax(q q^T) v [, * gamma + residual] and lse against float64 from the same bf16 q, v.

    Bound, per output (i, c), with s the exact scores, p = exp(s - max), L = sum_j p, o = sum_j p v / L, A = sum_j p |v| / L:
      score error     |ds_ij| <= D 2^-24 sum_d |q_id q_jd|           (D-term fp32 dot product of exact bf16 products);  E_i = max_j
      through exp     relative error of p_ij:  eta_i = E_i + 3 2^-24 R_i + 2^-22, R_i = max_j s - min_j s + THR  (the subtraction, the
                      scaling by log2 e and its constant, one ulp of the hardware exp; the reference maximum lags the true one by at
                      most THR and cancels between numerator and denominator, as does the factor of every rescale)
      P V operand     2^-8 relative on each p entering P V, weighted by A
      fp32 sums       n_T = T + T / 64 terms (T products or addends plus one multiplication per possible rescale): n_T 2^-24 A on the
                      numerator, n_T 2^-24 relative on L; 3 2^-24 for the reciprocal and the final product
      pre-rounding    B = 1.001 (A (eta + 2^-8 + n_T 2^-24) + |o| (eta + n_T 2^-24 + 3 2^-24))   (1.001: the second-order terms)
      plain           |err| <= B + 2^-8 (|o| + B)                                            (the bf16 rounding of o)
      epilogue        y = gamma o + r:  |err| <= |gamma| B + 2^-24 |y| + 2^-8 (|y| + |gamma| B)   (one fma, one bf16 rounding)
      lse             |err| <= 1.001 (eta + n_T 2^-24) + 2^-22 (|max_j s| + |lse| + 1)        (log of L, the sum, their roundings)"""
    n, t, d, c, waves, gamma = shape
    q, v = _attn_data(kind, n, t, d, c, seed=100 + t + d)
    res = v if gamma is not None else None    # Auto_Attn's use: the residual is the value tensor itself
    q64, v64 = q.double(), v.double()
    s = q64 @ q64.transpose(1, 2)
    smax = s.amax(-1, keepdim=True)
    p = torch.exp(s - smax)
    L = p.sum(-1, keepdim=True)
    o_ref = (p @ v64) / L
    A = (p @ v64.abs()) / L
    lse_ref = (smax + L.log()).squeeze(-1)
    E = (d * U24 * (q64.abs() @ q64.abs().transpose(1, 2))).amax(-1, keepdim=True)
    R = smax - s.amin(-1, keepdim=True) + THR
    eta = E + 3 * U24 * R + 2.0 ** -22
    nT = t + t // 64
    B = 1.001 * (A * (eta + U8 + nT * U24) + o_ref.abs() * (eta + nT * U24 + 3 * U24))

    o, lse = _attn_call(dev, q, v, gamma, res, waves)
    assert o.dtype == BF and o.shape == v.shape
    print(f"\nattention {shape} {kind}: dispatch {FF._L().attention_fwd_bf16_waves(n, t)} waves")
    if gamma is None:
        _within("o", o, o_ref, B + U8 * (o_ref.abs() + B))
    else:
        g32 = float(torch.tensor(gamma, dtype=torch.float32))
        y_ref = g32 * o_ref + v64
        _within("gamma * o + residual", o, y_ref, abs(g32) * B + U24 * y_ref.abs() + U8 * (y_ref.abs() + abs(g32) * B))
        # gamma = 0: the residual comes back bit for bit; NULL gamma / residual: the plain result, the same bits on every call
        o0, _ = _attn_call(dev, q, v, 0.0, res, waves)
        assert torch.equal(_bits(o0), _bits(v))
        op, _ = _attn_call(dev, q, v, None, None, waves)
        _within("o (NULL gamma / residual)", op, o_ref, B + U8 * (o_ref.abs() + B))
        op2, _ = _attn_call(dev, q, v, None, None, waves, want_lse=False)
        assert torch.equal(_bits(op), _bits(op2))
    _within("lse", lse, lse_ref, (1.001 * (eta + nT * U24) + 2.0 ** -22 * (smax.abs() + lse_ref.abs().unsqueeze(-1) + 1)).squeeze(-1))
    o2, _ = _attn_call(dev, q, v, gamma, res, waves, want_lse=False)
    assert torch.equal(_bits(o), _bits(o2)), "lse = NULL changes o"

    if kind == "late":
        fired, deferred, margin = _branches(s)
        print(f"  reference maximum: {fired} rescales after the first tile, {deferred} deferrals, nearest test {margin:.3f} from its threshold")
        assert margin > 0.05, "a rescale test too close to its threshold to be decided in float64"
        assert deferred > 0
        assert fired > 0 or t == 128     # T = 128: the scaled blocks lie in tiles 0 and 1, the only rescale is the first tile's
        # growth at a late tile and again at the end: for a good share of the rows the maximum over the last 32 keys exceeds the one over
        # everything before them (the two scaled blocks reach the same level; the noise decides which is higher)
        grow_end = float((s[:, :, t - 32:].amax(-1) > s[:, :, :t - 32].amax(-1)).float().mean())
        print(f"  rows whose maximum grows again in the last 32 keys: {grow_end:.2f}")
        assert grow_end > 0.1
        still = s[:, 5:8, :].amax(-1) - s[:, 5:8, :32].amax(-1)      # rows 5..7: no growth past the first tile
        assert float(still.max()) < THR
    if kind == "onehot":
        diag = torch.diagonal(p / L, dim1=1, dim2=2)
        assert float(diag.median()) > 0.99
    if kind == "equal" and gamma is None:
        _within("o against the mean of V", o, v64.mean(1, keepdim=True).expand_as(v64), B + U8 * (o_ref.abs() + B) + 1e-12)


def test_attention_refusals_on_device_tensors(dev):
    q, v = _attn_data("gauss", 1, 128, 64, 256, 1)
    with pytest.raises(FmiError, match="unsupported"):
        _attn_call(dev, q[:, :, :32].contiguous(), v)                 # (D, C) = (32, 256)
    with pytest.raises(FmiError, match="unsupported"):
        _attn_call(dev, q, v, waves=8)                                # eight waves need T % 256 == 0
    with pytest.raises(FmiError, match="bad argument"):
        _attn_call(dev, q, v, gamma=0.4, res=None)
    with pytest.raises(FmiError, match="multiple of 128"):
        FF.self_attention_bf16(q[:, :96].contiguous().to(dev), v[:, :96].contiguous().to(dev))


# ---------------------------------------------------------------------------------------------------------------------------------
# the Output block from a bf16 input
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(2, 8, 32), (1, 9, 35), (2, 200, 520)], ids=["one_tile", "ragged", "850_tiles"])
def test_output_block_against_float64(dev, n, h, w):
    """tanh(conv3x3(reflect_pad(lrelu(x, 0.1))) + b) from bf16 x, fp32 weights.  z = sum of 288 fp32 fmas of w lrelu(x) (lrelu itself one
    rounding) plus the bias: |dz| <= 290 2^-24 (sum |w| |lrelu(x)| + |b|); tanh has slope <= 1 and |tanh| <= 1: + 2^-21 for tanhf.
    850 tiles of 8 x 32 pixels are more than the workgroups that fit the chip at once (at most three per CU by their LDS): the
    persistent loop that stages the next tile's window during the arithmetic of the current one runs"""
    x = (torch.randn(n, h, w, 32, generator=_gen(40)) * 1.5).to(BF)
    wt = torch.randn(3, 32, 3, 3, generator=_gen(41)) * 0.08
    b = torch.randn(3, generator=_gen(42)) * 0.2
    slope = float(torch.tensor(0.1, dtype=torch.float32))
    x64 = x.double().permute(0, 3, 1, 2)
    a = torch.where(x64 > 0, x64, x64 * slope)
    ap = F.pad(a, (1, 1, 1, 1), mode="reflect")
    z = F.conv2d(ap, wt.double(), b.double())
    mag = F.conv2d(ap.abs(), wt.double().abs(), b.double().abs())
    ref = torch.tanh(z).permute(0, 2, 3, 1)
    wf = wt.permute(2, 3, 1, 0).reshape(9, 32, 3).contiguous().to(dev)       # wf[tap][C][K]
    pw = FF.PackedWeight(wf, None, 3, 32, 3, 3)
    y = FF.lrelu_conv2d_thin_bf16(x.to(dev), pw, b.to(dev), 0.1, 1, FF.ACT_TANH)
    assert y.dtype == torch.float32 and y.shape == (n, h, w, 3)
    print(f"\nOutput block {n} x {h} x {w}:")
    _within("image", y, ref, 290 * U24 * mag.permute(0, 2, 3, 1) + 2.0 ** -21)
    # the reflected border is what the interior of the same map gives: row 0 reads row 1 as its upper neighbour
    assert float((ref[:, 0] - ref[:, 1]).abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# block and model level: float64 against its bf16-storage emulation
# ---------------------------------------------------------------------------------------------------------------------------------
def _q(t):
    return t.to(BF).double()


def _ident(t):
    return t


def _rel(a, ref):
    return float((a.double() - ref).norm() / ref.norm().clamp_min(1e-300))


def _adjudicate(title, tensors):
    """tensors: name -> (gpu, emulation, float64).  Each gpu tensor within 3 x the emulation's own relative L2 error against float64"""
    print(f"\n{title}: relative L2 against float64 -- emulation, bf16 kernels, ratio")
    bad = []
    for name, (got, emu, ref) in tensors.items():
        assert bool(torch.isfinite(got).all()), name
        e_emu, e_gpu = _rel(emu.detach(), ref.detach()), _rel(got.detach().cpu(), ref.detach())
        print(f"  {name:44s} {e_emu:.3e} {e_gpu:.3e} {e_gpu / max(e_emu, 1e-300):.2f}")
        if not e_gpu <= 3 * e_emu:
            bad.append(name)
    assert not bad, bad


def _params64(sd):
    """a fresh float64 copy of a state_dict: every reference run starts from the state the kernels started from"""
    from oracle import picnet_cpu as O

    return O.prepare_params({k: v.detach().cpu() for k, v in sd.items()}, frozen=True, dtype=torch.float64)


def _lrelu(x):
    return F.leaky_relu(x, float(torch.tensor(0.1, dtype=torch.float32)))


def _inorm(P, pre, x):
    return F.instance_norm(x, weight=P[pre + ".weight"], bias=P[pre + ".bias"], eps=1e-5)


def _dec_block64(P, pre, x, q):
    """ResBlockDecoder as the bf16 path runs it (q = _q) or in plain float64 (q = _ident); W / sigma from one power iteration on P's u, v"""
    from oracle import picnet_cpu as O

    w1, w2, wb = (O.sn_weight(P, pre + name + ".module") for name in ("conv1", "conv2", "bypass"))
    h = q(_lrelu(_inorm(P, pre + "model.0", x)))
    h = q(F.conv2d(h, q(w1), P[pre + "conv1.module.bias"], padding=1))
    h = q(_lrelu(_inorm(P, pre + "model.3", h)))
    kw = dict(stride=2, padding=1, output_padding=1)
    y = q(F.conv_transpose2d(h, q(w2), None, **kw) + F.conv_transpose2d(x, q(wb), None, **kw))   # one reduction over cat[h, x]
    return q(y + (P[pre + "conv2.module.bias"] + P[pre + "bypass.module.bias"]).view(1, -1, 1, 1))


def _attn64(P, pre, x, q):
    n, c, h, w = x.shape
    qq = q(F.conv2d(x, q(P[pre + "query_conv.weight"]), P[pre + "query_conv.bias"])).reshape(n, c // 4, h * w)
    v = x.reshape(n, c, h * w)
    s = qq.transpose(1, 2) @ qq
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = (q(p) @ v.transpose(1, 2)) / p.sum(-1, keepdim=True)               # the row sum adds the unrounded p
    return q(P[pre + "gamma"] * o.transpose(1, 2).reshape(n, c, h, w) + x)


def _generator64(P, pre, encoded, z, q, layers=5, L=0):
    from oracle import picnet_cpu as O

    if z is not None:
        f = O.res_block(P, pre + "generator", z)
        for i in range(L):
            f = O.res_block(P, f"{pre}generator{i}", f)
        out = encoded + f
    else:
        out = encoded
    out = q(out)                                                           # the one cast
    for i in range(layers):
        out = _dec_block64(P, f"{pre}decoder{i}.", out, q)
        if i == 1:
            out = _attn64(P, f"{pre}attn{i}.", out, q)
    return O.output_block(P, f"{pre}out{layers - 1}", out)                 # fp32 weights, fp32 image


def _nchw64(t):
    return t.detach().cpu().double().permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _perturb(module, seed):
    """away from the initial values that would hide a term: InstanceNorm weight 1 / bias 0, conv biases 0, gamma 0"""
    g = _gen(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("gamma"):
                p.fill_(0.4)
            elif p.ndim == 1 and not name.endswith(("weight_u", "weight_v", "alpha")):
                p.add_(torch.randn(p.shape, generator=g) * 0.1)


@pytest.mark.parametrize("cin,cout,hw", [(256, 256, 8), (64, 32, 16)], ids=["256_256_at_8", "64_32_at_16"])
def test_res_block_decoder_bf16(dev, cin, cout, hw):
    """the thin end: a 96-wide reduction into 32 channels, conv1 with K = 32"""
    from face_mask_inpaint_amd.modules.pluralistic_model import base_function as BFN

    torch.manual_seed(3)
    block = BFN.ResBlockDecoder(cin, cout, cout, BFN.get_norm_layer("instance"), torch.nn.LeakyReLU(0.1), use_spect=True)
    _perturb(block, 4)
    sd = copy.deepcopy(block.state_dict())
    x = torch.randn(2, hw, hw, cin, generator=_gen(5)).to(BF)
    block.to(dev).eval()
    with torch.no_grad():
        y = block.nhwc(x.to(dev))
    assert y.dtype == BF and y.shape == (2, 2 * hw, 2 * hw, cout)
    emu = _dec_block64(_params64(sd), "", _nchw64(x), _q)
    ref = _dec_block64(_params64(sd), "", _nchw64(x), _ident)
    _adjudicate(f"ResBlockDecoder({cin} -> {cout}) at {hw}^2", {"output": (y.float(), _nhwc(emu), _nhwc(ref))})


def test_auto_attn_bf16(dev):
    from face_mask_inpaint_amd.modules.pluralistic_model import base_function as BFN

    torch.manual_seed(6)
    attn = BFN.Auto_Attn(256, None)
    _perturb(attn, 7)
    with torch.no_grad():
        attn.query_conv.weight.mul_(2.0)      # scores of a few units
    sd = copy.deepcopy(attn.state_dict())
    x = torch.randn(2, 16, 16, 256, generator=_gen(8)).to(BF)
    attn.to(dev).eval()
    with torch.no_grad():
        y = attn.nhwc(x.to(dev))
    assert y.dtype == BF and y.shape == x.shape
    P = _params64(sd)
    emu, ref = _attn64(P, "", _nchw64(x), _q), _attn64(P, "", _nchw64(x), _ident)
    # gamma * out + x is dominated by x, which both sides hold exactly: compare the attention's own contribution too
    x64 = _nchw64(x)
    _adjudicate("Auto_Attn(256) at 16 x 16, gamma 0.4", {"output": (y.float(), _nhwc(emu), _nhwc(ref)),
                                                         "output - x": (y.float().cpu().double() - _nhwc(x64), _nhwc(emu - x64), _nhwc(ref - x64))})


@pytest.fixture(scope="module")
def generator_case(dev):
    """the full-width generator once, with its initial state and one seeded 8 x 8 input"""
    from face_mask_inpaint_amd.modules.pluralistic_model import network

    torch.manual_seed(9)
    g = network.define_g(ngf=32, z_nc=256, img_f=256, L=0, layers=5, norm="instance", activation="LeakyReLU", use_attn=True,
                         compute_dtype=BF)
    _perturb(g, 10)
    sd = copy.deepcopy(g.state_dict())
    enc = torch.randn(1, 256, 8, 8, generator=_gen(11))
    z = torch.randn(1, 256, 8, 8, generator=_gen(12))
    return g.to(dev).eval(), sd, enc, z


@pytest.mark.parametrize("with_z", [True, False], ids=["z", "no_z"])
def test_res_generator_bf16(dev, generator_case, with_z):
    g, sd, enc, z = generator_case
    g.load_state_dict(sd)              # every forward advances the SpectralNorm u / v: each run starts from the same state
    zz = z if with_z else None
    with torch.no_grad():
        img = g(enc.to(dev), None if zz is None else zz.to(dev))
    assert img.dtype == torch.float32 and img.shape == (1, 3, 256, 256)
    z64 = None if zz is None else zz.double()
    emu = _generator64(_params64(sd), "", enc.double(), z64, _q)
    ref = _generator64(_params64(sd), "", enc.double(), z64, _ident)
    _adjudicate("ResGenerator (ngf 32, img_f 256) from 8 x 8, gamma 0.4, " + ("with z" if with_z else "z = None"), {"image": (img, emu, ref)})


def _fill_params():
    from face_mask_inpaint_amd import PICNet_inference as PI

    return PI.process_params(PI.get_args([]))


def test_reference_fill_bf16_end_to_end(dev):
    from face_mask_inpaint_amd.modules.model import ReferenceFill
    from oracle import picnet_cpu as O

    torch.manual_seed(13)
    enc_p, dec_p = _fill_params()
    G = ReferenceFill(None, enc_p, dec_p, use_att=True, out_size=(64, 64), decoder_dtype=BF)
    _perturb(G.decoder, 14)
    sd = copy.deepcopy(G.state_dict())
    g = _gen(15)
    src, ref_img = torch.rand(1, 3, 64, 64, generator=g), torch.rand(1, 3, 64, 64, generator=g)
    mask = torch.zeros(1, 64, 64)
    mask[:, 30:56, 12:52] = 1.0
    eps_p, eps_q = torch.randn(1, 128, 8, 8, generator=g), torch.randn(1, 128, 8, 8, generator=g)
    G.to(dev).eval()
    with torch.no_grad():
        img = G(src.to(dev), ref_img.to(dev), src_mask=mask.to(dev), eps=(eps_p.to(dev), eps_q.to(dev)))
    assert img.dtype == torch.float32 and img.shape == (1, 3, 64, 64)

    def run(q):
        P = _params64(sd)
        s64, r64 = src.double(), ref_img.double()
        src_dist, src_feat = O.res_encoder(P, "src_encoder", s64, "src", 5, 6, 128)
        ref_dist, ref_feat = O.res_encoder(P, "ref_encoder", r64, "ref", 5, 6, 128)
        m = O.scale_img(mask.double().unsqueeze(1), src_feat.shape[-2:])
        e = O.example_guided_attention(P, "attention", m, src_feat, ref_feat)
        zz = O.get_z(src_dist, ref_dist, eps_p.double(), eps_q.double())
        return F.adaptive_avg_pool2d(_generator64(P, "decoder.", e, zz, q), (64, 64))

    emu, ref = run(_q), run(_ident)
    whole = O.reference_fill_forward(_params64(sd), src.double(), ref_img.double(), mask.double(), eps_p.double(), eps_q.double(),
                                     out_size=(64, 64))
    # the float64 side here is the oracle's forward, up to the LeakyReLU slope: the kernels hold 0.1 as an fp32 number (relative 1.5e-8)
    assert _rel(ref, whole.detach()) < 1e-7
    _adjudicate("ReferenceFill(decoder_dtype=bf16) on a 64 x 64 pair", {"image": (img, emu.detach(), ref.detach())})


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals on the device
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(dev, generator_case):
    from face_mask_inpaint_amd.modules.model import ReferenceFill

    g, sd, enc, z = generator_case
    g.load_state_dict(sd)
    before = copy.deepcopy(g.state_dict())
    with pytest.raises(FmiError, match="inference only"):          # grad mode with trainable parameters
        g(enc.to(dev), z.to(dev))
    with torch.no_grad():
        with pytest.raises(FmiError, match="multiple of 128"):     # a 9 x 9 feature map: 1296 tokens at attn1
            g(torch.randn(1, 256, 9, 9, device=dev))
    after = g.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), "a refused call advanced the SpectralNorm state"
    enc_p, dec_p = _fill_params()
    G = ReferenceFill(None, dict(enc_p), dict(dec_p), decoder_dtype=BF).to(dev).eval()
    x = torch.rand(1, 3, 72, 72, device=dev)                       # 72 x 72: a 9 x 9 feature map, T = 1296
    with torch.no_grad():
        with pytest.raises(FmiError, match="1296"):
            G(x, x, src_mask=torch.zeros(1, 72, 72, device=dev))
    dec16 = dict(dec_p, ngf=16)
    with pytest.raises(FmiError, match="fp32 only"):
        ReferenceFill(None, dict(enc_p), dec16, decoder_dtype=BF)


# ---------------------------------------------------------------------------------------------------------------------------------
# harness
# ---------------------------------------------------------------------------------------------------------------------------------
def _count_entry(monkeypatch, name, record=None):
    """count the calls of one library entry (the instance every op goes through)"""
    lib = FF._L()
    calls = []
    real = getattr(lib, name)

    def counted(*a):
        calls.append(record(a) if record else 1)
        return real(*a)

    monkeypatch.setattr(lib, name, counted)
    return calls


def test_picnet_harness_generator_dtype(dev, monkeypatch):
    from face_mask_inpaint_amd import PICNet_inference as PI

    b16 = _count_entry(monkeypatch, "attention_fwd_bf16", lambda a: a[7])                 # T
    out16 = _count_entry(monkeypatch, "conv2d_thin_lrelu_fwd_bf16")
    f32 = _count_entry(monkeypatch, "attention_fwd_f32", lambda a: a[7])
    f32p = _count_entry(monkeypatch, "attention_fwd_pieces_f32", lambda a: a[9])
    out32 = _count_entry(monkeypatch, "conv2d_thin_lrelu_fwd_f32")
    s = PI.main(["--num_batches", "1", "--batch_size", "1", "--generator_dtype", "bf16"])
    assert s == s and -1.0 <= s <= 1.0
    assert b16 == [16384] and len(out16) == 1 and len(out32) == 0
    assert 16384 not in f32 + f32p and f32 + f32p == [1024]        # the guided attention at 32 x 32 stays fp32
    for c in (b16, out16, f32, f32p, out32):
        c.clear()
    s32 = PI.main(["--num_batches", "1", "--batch_size", "1"])
    assert s32 == s32 and not b16 and not out16 and len(out32) == 1 and sorted(f32 + f32p) == [1024, 16384]
    print(f"\nharness SSIM against the random ground truth: bf16 {s:.6f}, fp32 {s32:.6f}")


def test_fp32_checkpoint_loads_into_the_bf16_build_and_back(dev, tmp_path):
    from face_mask_inpaint_amd.modules.model import ReferenceFill

    enc_p, dec_p = _fill_params()
    a = ReferenceFill(None, dict(enc_p), dict(dec_p)).to(dev)
    b = ReferenceFill(None, dict(enc_p), dict(dec_p), decoder_dtype=BF).to(dev)
    torch.save(a.state_dict(), tmp_path / "a.pth")
    b.load_state_dict(torch.load(tmp_path / "a.pth", map_location="cpu", weights_only=True), strict=True)
    torch.save(b.state_dict(), tmp_path / "b.pth")
    back = torch.load(tmp_path / "b.pth", map_location="cpu", weights_only=True)
    sa = a.state_dict()
    assert list(back) == list(sa) and all(torch.equal(back[k], sa[k].cpu()) and back[k].dtype == torch.float32 for k in sa)
    a.load_state_dict(back, strict=True)
