"""GPU: the bf16 VGG16 trunk of VGGLoss -- the masked adjoint fmi_conv2d_dgrad_relu_bf16 on every kernel that carries its output stage,
the tap passes, the bf16-reading thin-input adjoint, every entry's refusals, the trunk with its launch ledger and
VGGLoss(feature_dtype=torch.bfloat16).  Conventions of tests/test_gpu_picnet_bf16.py.

The rule for a tensor the bf16 kernels produce is that file's: it must lie within 3 x the emulation's own relative L2 error against
float64, the emulation being tests/vgg_reference.py with its rounding hook on (float64 arithmetic, bf16 values wherever the kernels
store or pack one).  All three numbers are printed.  The tap passes are exact and are compared bit for bit.  Outputs are pre-filled with
NaN, so an element no thread wrote shows."""
import collections
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import vgg_reference as VR
from face_mask_inpaint_amd import _lib
from face_mask_inpaint_amd import functional as FF
from face_mask_inpaint_amd.modules.loss import VGGLoss

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64
OK, BAD, UNSUP = 0, 1, 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


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


def _nan16(shape, dev):
    return torch.full(shape, float("nan"), device=dev, dtype=BF)


class _tile_mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = FF._L().debug_bf16_tile(self.mode)

    def __exit__(self, *exc):
        FF._L().debug_bf16_tile(self.prev)
        return False


# ---------------------------------------------------------------------------------------------------------------------------------
# fmi_conv2d_dgrad_relu_bf16
# ---------------------------------------------------------------------------------------------------------------------------------
ADJ_SHAPES = [(2, 8, 8, 64, 64), (1, 12, 20, 128, 64), (2, 16, 16, 256, 512), (2, 16, 16, 512, 256)]  # (N, H, W, C -> K)
# fmi_debug_bf16_last_tile's code of the kernel each case must reach: 1000 BM + BN, + 1000000 for the eight-phase kernel.  At the four small
# shapes the row count stays below every threshold of the dispatch, so modes 0 and 2 reach the 64 x 64 tile and mode 8 the two eight-phase
# tiles (64 output columns never take that kernel).  The other four tiles need rows: the smallest maps that cross each threshold --
# 384 tiles of 128 x 64; 256 tiles of 64 x 128; 512 tiles of 128 x 128; 200 tiles of 256 x 256 -- with the smallest reduction (K = 64).
T64, T8P_512, T8P_256 = 64064, 1512128, 1256256
ADJ_CASES = ([(s, m, T64) for s in ADJ_SHAPES for m in (0, 2)]
             + [(ADJ_SHAPES[0], 8, T64), (ADJ_SHAPES[1], 8, T8P_512), (ADJ_SHAPES[2], 8, T8P_256), (ADJ_SHAPES[3], 8, T8P_256)]
             + [((1, 192, 256, 64, 64), 0, 128064), ((1, 128, 128, 128, 64), 2, 64128), ((1, 128, 128, 512, 64), 2, 128128),
                ((1, 160, 160, 512, 64), 2, 256256)])
_ADJ = {}


def _adj_case(shape):
    """bf16 operands of one adjoint and its float64 result, computed once and never modified"""
    if shape not in _ADJ:
        n, h, w, c, k = shape
        g = _gen(sum(shape))
        wt = (torch.randn(k, c, 3, 3, generator=g) / (9 * k) ** 0.5).to(BF)
        dy = torch.randn(n, h, w, k, generator=g).to(BF)
        a = torch.randn(n, h, w, c, generator=g).to(BF)
        a[0, 0, 0, :8] = 0.0   # a zero and a negative zero are not positive
        a[0, 0, 1, :8] = -0.0
        wck = wt.permute(1, 2, 3, 0).reshape(c, 9, k).contiguous()
        adj = F.conv_transpose2d(dy.double().permute(0, 3, 1, 2), wt.double(), padding=1).permute(0, 2, 3, 1).contiguous()
        _ADJ[shape] = dict(dy=dy, a=a, wck=wck, adj=adj, ref=torch.where(a.double() > 0, adj, torch.zeros((), dtype=F64)))
    return _ADJ[shape]


def _run_adj(dev, shape, cs, a_in, masked=True):
    n, h, w, c, k = shape
    d, _, _ = FF.conv_desc(n, h, w, c, k, 3, 3, 1, 1)
    dy, wck = cs["dy"].to(dev), cs["wck"].to(dev)
    dx = _nan16((n, h, w, c), dev)
    if masked:
        FF._L().conv2d_dgrad_relu_bf16(C.byref(d), FF._p(dy), FF._p(wck), FF._p(a_in.to(dev)), FF._p(dx), FF._st())
    else:
        FF._L().conv2d_dgrad_bf16(C.byref(d), FF._p(dy), FF._p(wck), None, FF._p(dx), None, 0, FF._st())
    torch.cuda.synchronize()
    return dx, FF._L().debug_bf16_last_tile()


@pytest.mark.parametrize("shape,mode,tile", ADJ_CASES, ids=lambda v: "N%d_%dx%d_%d-%d" % v if isinstance(v, tuple) else str(v))
def test_masked_adjoint(dev, shape, mode, tile):
    """every kernel that carries the masked output stage -- five tiles of conv_bf16_kernel, two of the eight-phase kernel -- is reached
    (asserted through fmi_debug_bf16_last_tile, for the masked and for the plain launch) and adjudicated"""
    cs = _adj_case(shape)
    with _tile_mode(mode):
        dx, t0 = _run_adj(dev, shape, cs, cs["a"])
        again, t1 = _run_adj(dev, shape, cs, cs["a"])
        ones = torch.ones_like(cs["a"])
        open_, t2 = _run_adj(dev, shape, cs, ones)
        plain, t3 = _run_adj(dev, shape, cs, None, masked=False)
    assert (t0, t1, t2, t3) == (tile,) * 4, f"tile codes {(t0, t1, t2, t3)}, the case is meant for {tile}"
    assert FF._L().get_deterministic() == 0
    assert torch.equal(_bits(dx), _bits(again)), "two runs differ"
    shut = ~(cs["a"].float() > 0)
    assert bool(shut.any()) and bool((~shut).any())
    assert bool((_bits(dx)[shut] == 0).all()), "a masked element is +0, bit for bit"
    assert torch.equal(_bits(open_), _bits(plain)), "with a_in > 0 everywhere: fmi_conv2d_dgrad_bf16's bits in the same tile mode"
    _adjudicate(f"masked adjoint {shape} tile mode {mode}", {"dx16": (dx.float(), VR.rnd_bf16(cs["ref"]), cs["ref"]),
                                                            "dx16, mask open": (open_.float(), VR.rnd_bf16(cs["adj"]), cs["adj"])})


# ---------------------------------------------------------------------------------------------------------------------------------
# fmi_vgg_tap_fwd_bf16 / fmi_vgg_tap_bwd_bf16: exact
# ---------------------------------------------------------------------------------------------------------------------------------
TAP_SHAPES = [(2, 8, 8, 64), (1, 6, 10, 72), (2, 4, 4, 512)]


def _tap_data(shape):
    """a: half of the channels on a grid of half-integers, so that windows with tied positive maxima, all-zero and all-negative windows are
    common; one window is tied by construction"""
    n, h, w, c = shape
    g = _gen(sum(shape))
    a = torch.randn(n, h, w, c, generator=g)
    a[..., ::2] = (a[..., ::2] * 1.5).round() / 2
    a[0, 0:2, 0:2, 0] = 1.25
    a[0, 0:2, 2:4, 0] = torch.tensor([[0.5, 2.0], [2.0, 2.0]])
    a = a.to(BF)
    gtap = torch.randn(n, h, w, c, generator=g)
    gpool = torch.randn(n, h // 2, w // 2, c, generator=g).to(BF)
    return a, gtap, gpool


@pytest.mark.parametrize("pool", [True, False], ids=["pool", "nopool"])
@pytest.mark.parametrize("shape", TAP_SHAPES, ids=lambda s: "N%d_%dx%dx%d" % s)
def test_tap_passes_are_exact(dev, shape, pool):
    n, h, w, c = shape
    a, gtap, gpool = _tap_data(shape)
    an = a.float().permute(0, 3, 1, 2)
    pooled_cpu, idx = F.max_pool2d(an, 2, 2, return_indices=True)
    win = an.unfold(2, 2, 2).unfold(3, 2, 2).reshape(n, c, h // 2, w // 2, 4)
    tied = ((win == pooled_cpu[..., None]).sum(-1) > 1) & (pooled_cpu > 0)
    assert int(tied.sum()) > 10, "windows with tied positive maxima"
    L, st = FF._L(), FF._st()
    ad, gd, gpd = a.to(dev), gtap.to(dev), gpool.to(dev)
    tap = torch.full((n, h, w, c), float("nan"), device=dev)
    pooled = _nan16((n, h // 2, w // 2, c), dev) if pool else None
    L.vgg_tap_fwd_bf16(FF._p(ad), FF._p(tap), FF._p(pooled), n, h, w, c, st)
    dy = _nan16((n, h, w, c), dev)
    L.vgg_tap_bwd_bf16(FF._p(ad), FF._p(gd), FF._p(gpd) if pool else None, FF._p(dy), n, h, w, c, st)
    torch.cuda.synchronize()
    assert torch.equal(tap.cpu().view(torch.int32), a.float().view(torch.int32)), "tap == float(a16), bit for bit"
    g = gtap.permute(0, 3, 1, 2)
    if pool:
        want = _nan16((n, h // 2, w // 2, c), dev)
        L.maxpool2_bf16(FF._p(ad), FF._p(want), n, h, w, c, st)
        torch.cuda.synchronize()
        assert torch.equal(_bits(pooled), _bits(want)), "the pooled map against fmi_maxpool2_bf16"
        assert torch.equal(pooled.float().cpu(), pooled_cpu.permute(0, 2, 3, 1)), "and against ATen's winner rule"
        g = g + F.max_unpool2d(gpool.float().permute(0, 3, 1, 2), idx, 2, 2, output_size=(h, w))  # one fp32 addition
    emu = torch.where(an > 0, g, torch.zeros(())).to(BF).permute(0, 2, 3, 1).contiguous()          # one round-to-nearest-even
    assert torch.equal(_bits(dy), _bits(emu)), "dy16 against the emulation, bit for bit"


# ---------------------------------------------------------------------------------------------------------------------------------
# fmi_conv2d_thin_input_dgrad_bf16
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 16, 16), (1, 10, 24)], ids=lambda s: "N%d_%dx%d" % s)
def test_thin_adjoint_reads_bf16(dev, shape):
    """against fmi_conv2d_thin_input_dgrad_f32 on float(dy16): two fp32 summation orders of the same terms, the tolerance of
    tests/test_gpu_thin_in.py::test_thin_in_input_gradient (rtol 1e-5, atol 2e-5 on operands of the same scale)"""
    n, h, w = shape
    c, k = 3, 64
    g = _gen(h * 7 + w)
    wt_ = torch.randn(k, c, 3, 3, generator=g) / (c * 9) ** 0.5
    dy16 = torch.randn(n, h, w, k, generator=g).to(BF)
    wtp = wt_.permute(2, 3, 0, 1).reshape(9, k, c).contiguous().to(dev)
    d, _, _ = FF.conv_desc(n, h, w, c, k, 3, 3, 1, 1)
    L, st = FF._L(), FF._st()
    dyd, dyf = dy16.to(dev), dy16.float().to(dev)
    got = torch.full((n, h, w, c), float("nan"), device=dev)
    want = torch.full((n, h, w, c), float("nan"), device=dev)
    L.conv2d_thin_input_dgrad_bf16(C.byref(d), FF._p(dyd), FF._p(wtp), FF._p(got), st)
    L.conv2d_thin_input_dgrad_f32(C.byref(d), FF._p(dyf), FF._p(wtp), FF._p(want), st)
    torch.cuda.synchronize()
    ref = F.conv_transpose2d(dy16.double().permute(0, 3, 1, 2), wt_.double(), padding=1).permute(0, 2, 3, 1)
    print(f"\nthin adjoint {shape}: rel L2 against float64 -- bf16-reading {_rel(got.cpu(), ref):.3e}, fp32-reading {_rel(want.cpu(), ref):.3e}")
    torch.testing.assert_close(got, want, rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(got.cpu().double(), ref, rtol=1e-5, atol=2e-5)


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_entry_refuses_before_launching(dev):
    """NULL -> BAD_ARG, a descriptor whose OH / OW do not follow -> BAD_ARG, an unsupported width or a misaligned pointer -> UNSUPPORTED;
    nothing is launched: every buffer keeps its NaN fill"""
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("fmi_conv2d_dgrad_relu_bf16", "fmi_vgg_tap_fwd_bf16", "fmi_vgg_tap_bwd_bf16", "fmi_conv2d_thin_input_dgrad_bf16"):
        getattr(lib, name).argtypes = _lib.SIGNATURES[name]
        getattr(lib, name).restype = C.c_int
    buf = torch.full((1 << 16,), float("nan"), device=dev)
    p = C.c_void_p(buf.data_ptr())
    q = C.c_void_p(buf.data_ptr() + 2)  # 2-byte aligned only
    q8 = C.c_void_p(buf.data_ptr() + 8)  # 8-byte aligned only
    desc = lambda c, k, **kw: FF.conv_desc(1, 8, 8, c, k, kw.get("ks", 3), kw.get("ks", 3), kw.get("stride", 1), kw.get("pad", 1))[0]
    adj = lambda d, *a: lib.fmi_conv2d_dgrad_relu_bf16(C.byref(d), *a, None)
    good = desc(64, 64)
    assert lib.fmi_conv2d_dgrad_relu_bf16(None, p, p, p, p, None) == BAD
    for bad in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert adj(good, *bad) == BAD
    broken = desc(64, 64)
    broken.OH = 7
    assert adj(broken, p, p, p, p) == BAD
    for d in (desc(32, 64), desc(64, 96), desc(64, 64, ks=1, pad=0), desc(64, 64, stride=2), desc(64, 64, pad=2)):
        assert adj(d, p, p, p, p) == UNSUP
    for mis in ((q, p, p, p), (p, q, p, p), (p, p, q8, p), (p, p, p, q8)):
        assert adj(good, *mis) == UNSUP
    fwd = lambda *a: lib.fmi_vgg_tap_fwd_bf16(*a, None)
    assert fwd(None, p, p, 1, 4, 4, 8) == BAD and fwd(p, None, p, 1, 4, 4, 8) == BAD and fwd(p, p, None, 0, 4, 4, 8) == BAD
    assert fwd(p, p, p, 1, 4, 4, 12) == UNSUP and fwd(p, p, p, 1, 5, 4, 8) == UNSUP and fwd(p, p, p, 1, 4, 6 + 1, 8) == UNSUP
    assert fwd(q, p, p, 1, 4, 4, 8) == UNSUP and fwd(p, q8, p, 1, 4, 4, 8) == UNSUP and fwd(p, p, q8, 1, 4, 4, 8) == UNSUP
    bwd = lambda *a: lib.fmi_vgg_tap_bwd_bf16(*a, None)
    for bad in ((None, p, p, p), (p, None, p, p), (p, p, p, None)):
        assert bwd(*bad, 1, 4, 4, 8) == BAD
    assert bwd(p, p, p, p, 1, 4, 0, 8) == BAD
    assert bwd(p, p, p, p, 1, 4, 4, 12) == UNSUP and bwd(p, p, p, p, 1, 3, 4, 8) == UNSUP
    for mis in ((q8, p, p, p), (p, q8, p, p), (p, p, q8, p), (p, p, p, q8)):
        assert bwd(*mis, 1, 4, 4, 8) == UNSUP
    thin = lambda d, *a: lib.fmi_conv2d_thin_input_dgrad_bf16(None if d is None else C.byref(d), *a, None)
    tgood = desc(3, 64)
    assert thin(None, p, p, p) == BAD
    for bad in ((None, p, p), (p, None, p), (p, p, None)):
        assert thin(tgood, *bad) == BAD
    tbroken = desc(3, 64)
    tbroken.OW = 9
    assert thin(tbroken, p, p, p) == BAD
    for d in (desc(8, 64), desc(3, 128), desc(3, 48), desc(3, 64, stride=2)):  # 48 / 4 = 12 lanes per run: not a power of two
        assert thin(d, p, p, p) == UNSUP
    assert thin(tgood, q8, p, p) == UNSUP and thin(tgood, p, p, q) == UNSUP
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()), "a refused call wrote something"


# ---------------------------------------------------------------------------------------------------------------------------------
# the trunk
# ---------------------------------------------------------------------------------------------------------------------------------
LEDGER = {"fwd": {"conv": 10, "fmi_vgg_tap_fwd_bf16": 4},
          "bwd": {"fmi_vgg_tap_bwd_bf16": 4, "fmi_conv2d_dgrad_relu_bf16": 6, "fmi_conv2d_dgrad_bf16": 3, "fmi_conv2d_thin_input_dgrad_bf16": 1}}
FWD_CONVS = ("fmi_conv2d_thin_in_fwd_bf16", "fmi_conv2d_fwd_act_bf16", "fmi_conv2d_fwd_chan_bf16")


def _convs(v):
    return [m for bl in v.blocks for m in bl if isinstance(m, torch.nn.Conv2d)]


def _module(seed, **kw):
    torch.manual_seed(seed)
    return VGGLoss(**kw)


class _count_calls:
    """every library call while the context is open, by entry name"""

    def __init__(self, monkeypatch):
        self.mp, self.calls = monkeypatch, []

    def __enter__(self):
        L = _lib.lib()
        self.ctx = self.mp.context()
        mp = self.ctx.__enter__()
        for name in _lib.SIGNATURES:
            fn = getattr(L, name[4:])
            mp.setattr(L, name[4:], (lambda f, nm: lambda *a: (self.calls.append(nm), f(*a))[1])(fn, name))
        return self

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)

    def ledger(self):
        out = collections.Counter()
        for nm in self.calls:
            out["conv" if nm in FWD_CONVS else nm] += 1
        return dict(out)


_TRUNK = {}


def _trunk_case(case):
    """the module, the inputs and the float64 / emulated results of one trunk case, computed once and never modified"""
    if case not in _TRUNK:
        n, h, w, seed = case
        v = _module(seed, feature_dtype=BF)
        x, gtaps = VR.trunk_inputs(n, h, w, seed)
        y, _ = VR.trunk_inputs(n, h, w, seed + 100)
        ws, bs = [c.weight.detach() for c in _convs(v)], [c.bias.detach() for c in _convs(v)]
        _TRUNK[case] = dict(v=v, x=x, y=y, gtaps=gtaps, ref=VR.trunk(x, ws, bs, gtaps), emu=VR.trunk(x, ws, bs, gtaps, rnd=VR.rnd_bf16),
                            yref=VR.trunk(y, ws, bs), yemu=VR.trunk(y, ws, bs, rnd=VR.rnd_bf16))
    return _TRUNK[case]


@pytest.mark.parametrize("case", VR.TRUNK_CASES, ids=lambda c: "%dx%dx%d" % c[:3])
def test_trunk_against_float64(dev, monkeypatch, case):
    cs = _trunk_case(case)
    v = cs["v"].to(dev)
    v._prepare()
    packs = v._cache["packs16"]
    x = cs["x"].to(dev).requires_grad_(True)
    with _count_calls(monkeypatch) as fwd:
        taps = FF.vgg_trunk_bf16(x, packs)
    with _count_calls(monkeypatch) as bwd:
        torch.autograd.backward(taps, [g.to(dev) for g in cs["gtaps"]])
    with torch.no_grad(), _count_calls(monkeypatch) as tgt:
        ytaps = FF.vgg_trunk_bf16(cs["y"].to(dev), packs)
    torch.cuda.synchronize()
    print(f"\nlaunch ledger: forward {fwd.ledger()}, backward {bwd.ledger()}, target forward {tgt.ledger()}")
    assert fwd.ledger() == LEDGER["fwd"] and bwd.ledger() == LEDGER["bwd"] and tgt.ledger() == LEDGER["fwd"]
    assert all(t.dtype == torch.float32 and t.requires_grad for t in taps) and not any(t.requires_grad for t in ytaps)
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    ts = {f"tap {i + 1} (gradient batch)": (taps[i], cs["emu"].taps[i], cs["ref"].taps[i]) for i in range(4)}
    ts.update({f"tap {i + 1} (target batch)": (ytaps[i], cs["yemu"].taps[i], cs["yref"].taps[i]) for i in range(4)})
    ts["image gradient"] = (x.grad, cs["emu"].gx, cs["ref"].gx)
    _adjudicate(f"bf16 VGG trunk {case[:3]}", ts)


def test_trunk_backward_skips_what_no_gradient_reaches(dev, monkeypatch):
    """taps without a gradient: the blocks behind the last tap that has one are not run; a block in front of it runs with zeros for its own
    tap.  Either way the image gradient has the bits of the run that is given explicit zeros."""
    cs = _trunk_case(VR.TRUNK_CASES[0])
    v = cs["v"].to(dev)
    v._prepare()
    packs = v._cache["packs16"]
    gts = [g.to(dev) for g in cs["gtaps"]]

    def grad(used):
        x = cs["x"].to(dev).requires_grad_(True)
        taps = FF.vgg_trunk_bf16(x, packs)
        with _count_calls(monkeypatch) as bwd:
            torch.autograd.backward([taps[i] for i in used], [gts[i] for i in used])
        return x.grad, bwd.ledger()

    def grad_zeros(used):
        x = cs["x"].to(dev).requires_grad_(True)
        taps = FF.vgg_trunk_bf16(x, packs)
        torch.autograd.backward(taps, [gts[i] if i in used else torch.zeros_like(gts[i]) for i in range(4)])
        return x.grad

    front, ledger = grad([0, 1])
    assert ledger == {"fmi_vgg_tap_bwd_bf16": 2, "fmi_conv2d_dgrad_relu_bf16": 2, "fmi_conv2d_dgrad_bf16": 1, "fmi_conv2d_thin_input_dgrad_bf16": 1}
    assert torch.equal(front.view(torch.int32), grad_zeros([0, 1]).view(torch.int32))
    last, ledger = grad([3])
    assert ledger == LEDGER["bwd"]
    assert torch.equal(last.view(torch.int32), grad_zeros([3]).view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------
# VGGLoss(feature_dtype=torch.bfloat16)
# ---------------------------------------------------------------------------------------------------------------------------------
LOSS_TYPES = ["perceptual", "style", "contextual"]


def _loss_module(seed, **kw):
    """VGGLoss with He-initialised weights (std = sqrt(2 / fan_in), zero biases).  Behind torch's default initialisation the sixteen
    positions of the 4 x 4 map of block 4 are almost parallel (1 - cos < 3e-3), every contextual similarity saturates and the contextual
    loss is -log(1 + 1e-5): a value the fp32 loss kernels cannot hold to 1e-3 -- 1 + 1e-5 itself is rounded by up to 2^-24, 0.6 % of the
    1e-5 that carries the result -- whatever the trunk in front of them.  He initialisation keeps the positions apart (cx = 0.997, the
    loss 3e-3 with a condition number of 1; the float64 chain's selections have row gaps > 0.2 and relative column gaps > 0.9)."""
    v = _module(seed, **kw)
    g = _gen(seed)
    with torch.no_grad():
        for c in _convs(v):
            c.weight.copy_(torch.randn(c.weight.shape, generator=g) * (2.0 / (9 * c.in_channels)) ** 0.5)
            c.bias.zero_()
    return v


def _loss_inputs():
    """x and a target that shares half of it: unrelated images leave the contextual similarities saturated too"""
    n, h, w, seed = VR.TRUNK_CASES[0]
    x, _ = VR.trunk_inputs(3 * n, h, w, seed + 1)
    y, _ = VR.trunk_inputs(3 * n, h, w, seed + 2)
    return x, 0.5 * x + 0.5 * y


def _loss_step(v, xd, yd):
    x = xd.detach().clone().requires_grad_(True)
    losses = v.forward_multi_prepared(x, yd, LOSS_TYPES)
    (gx,) = torch.autograd.grad(losses[0] + losses[1] + losses[2], x)
    return losses, gx


def test_vggloss_bf16(dev, monkeypatch):
    n, h, w, seed = VR.TRUNK_CASES[0]
    v16 = _loss_module(seed, feature_dtype=BF).to(dev)
    v32 = _loss_module(seed, feature_dtype=torch.float32).to(dev)
    x, y = _loss_inputs()
    xd, yd = x.to(dev), y.to(dev)
    seen = []
    real = FF.vgg_trunk_bf16
    monkeypatch.setattr(FF, "vgg_trunk_bf16", lambda *a, **k: (lambda t: (seen.append(t), t)[1])(real(*a, **k)))
    losses, gx = _loss_step(v16, xd, yd)
    monkeypatch.setattr(FF, "vgg_trunk_bf16", real)
    xt, yt = [[t.detach().cpu() for t in s] for s in seen]
    # the unchanged fp32 loss kernels on the GPU's own taps
    want, _ = VR.losses(xt, yt, LOSS_TYPES, want_grad=False)
    for name, got, wv in zip(LOSS_TYPES, losses, want):
        print(f"  {name:11s} loss {float(got.detach()):.8e}, float64 on the GPU's taps {float(wv):.8e}")
        assert abs(float(got.detach()) - float(wv)) <= 1e-3 * abs(float(wv)), name
    # the gradient at the image: float64 losses behind the float64 / the emulated trunk
    ws, bs = [c.weight.detach().cpu() for c in _convs(v16)], [c.bias.detach().cpu() for c in _convs(v16)]
    grads = {}
    for key, rnd in (("ref", None), ("emu", VR.rnd_bf16)):
        ty = VR.trunk(y, ws, bs, rnd=rnd).taps
        grads[key] = VR.trunk(x, ws, bs, lambda tx: VR.losses(tx, ty, LOSS_TYPES)[1], rnd=rnd).gx
    l32, gx32 = _loss_step(v32, xd, yd)
    print("  against the fp32 build (not bounded: a property of bf16 features): " +
          ", ".join(f"{nm} {abs(float(a.detach()) - float(b.detach())) / abs(float(b.detach())):.3e}" for nm, a, b in zip(LOSS_TYPES, losses, l32)) +
          f", image gradient rel L2 {_rel(gx.cpu(), gx32.cpu().double()):.3e}")
    _adjudicate("VGGLoss(feature_dtype=bf16), three losses", {"image gradient": (gx, grads["emu"], grads["ref"])})


def test_default_is_the_fp32_build_bit_for_bit(dev, monkeypatch):
    monkeypatch.delenv("FMI_VGG_DTYPE", raising=False)
    seed = VR.TRUNK_CASES[0][3]
    va, vb = _module(seed, width_div=8).to(dev), _module(seed, width_div=8, feature_dtype=torch.float32).to(dev)
    assert va.feature_dtype == vb.feature_dtype == torch.float32
    x, y = _loss_inputs()
    xd, yd = x.to(dev), y.to(dev)
    with FF.deterministic():
        la, ga = _loss_step(va, xd, yd)
        lb, gb = _loss_step(vb, xd, yd)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(la, lb))
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32))


def test_capture_and_replay_give_the_eager_bits(dev):
    seed = VR.TRUNK_CASES[0][3]
    v = _loss_module(seed, feature_dtype=BF).to(dev)
    x, y = _loss_inputs()
    xd, yd = x.to(dev), y.to(dev)
    with FF.deterministic():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # eager runs on a side stream first, as capture requires
            for _ in range(2):
                eager_l, eager_g = _loss_step(v, xd, yd)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap_l, cap_g = _loss_step(v, xd, yd)
        for _ in range(2):
            graph.replay()
        torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(eager_l, cap_l))
    assert torch.equal(eager_g.view(torch.int32), cap_g.view(torch.int32))
