"""GPU: the trainable bf16 self-attention -- fmi_attention_bwd_prep_bf16 and fmi_attention_bwd_bf16 (csrc/attention_bwd_bf16.hip),
FF.self_attention_bf16_train under autograd and graph capture, Auto_Attn / ResGenerator with attn_dtype = bf16.

The float64 reference and the float64 emulation of the kernels' rounding points are tests/attention_reference.py (checked against
autograd on the CPU by tests/test_host_attention_bf16_train.py, which also asserts that these seeds and scales give a softmax that is
neither uniform nor, in the moderate cases, one-hot).  The rule is that of tests/test_gpu_picnet_bf16.py: a tensor the bf16 kernels
produce must lie within 3 x the emulation's own relative L2 error against float64.  All three numbers are printed."""
import copy

import pytest
import torch

import attention_reference as R

from face_mask_inpaint_amd import functional as FF

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _bits32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _adjudicate(title, tensors):
    """tensors: name -> (gpu, emulation, float64).  Each gpu tensor within 3 x the emulation's own relative L2 error against float64"""
    print(f"\n{title}: relative L2 against float64 -- emulation, bf16 kernels, ratio")
    bad = []
    for name, (got, emu, ref) in tensors.items():
        assert bool(torch.isfinite(got).all()), f"{name}: non-finite (or unwritten) values"
        e_emu, e_gpu = R.rel_l2(emu, ref), R.rel_l2(got, ref)
        print(f"  {name:36s} {e_emu:.3e} {e_gpu:.3e} {e_gpu / max(e_emu, 1e-300):.2f}")
        if not e_gpu <= 3 * e_emu:
            bad.append(name)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------------------
def _forward(dev, q16, v16, waves=0):
    n, t, d = q16.shape
    c = v16.shape[2]
    o = torch.full((n, t, c), float("nan"), device=dev, dtype=BF)
    lse = torch.full((n, t), float("nan"), device=dev, dtype=torch.float32)
    FF._L().attention_fwd_bf16(FF._p(q16), FF._p(v16), FF._p(o), FF._p(lse), None, None, n, t, d, c, waves, FF._st())
    return o, lse


def _prep(dev, go, o16, d):
    n, t, c = go.shape
    go16 = torch.full((n, t, c), float("nan"), device=dev, dtype=BF)
    delta = torch.full((n, t), float("nan"), device=dev, dtype=torch.float32)
    FF._L().attention_bwd_prep_bf16(FF._p(go), FF._p(o16), FF._p(go16), FF._p(delta), n, t, d, c, FF._st())
    return go16, delta


def _backward(dev, q16, v16, go16, lse, delta):
    n, t, d = q16.shape
    c = v16.shape[2]
    gq = torch.full((n, t, d), float("nan"), device=dev, dtype=torch.float32)   # an unwritten element shows
    gv = torch.full((n, t, c), float("nan"), device=dev, dtype=torch.float32)
    FF._L().attention_bwd_bf16(FF._p(q16), FF._p(v16), FF._p(go16), FF._p(lse), FF._p(delta), FF._p(gq), FF._p(gv), n, t, d, c, FF._st())
    torch.cuda.synchronize()
    return gq, gv


KERNEL_CASES = [(s, "moderate", 0) for s in R.KERNEL_SHAPES] + [(s, "moderate", 8) for s in R.KERNEL_SHAPES if s[1] == 512] \
    + [(R.PEAKED_SHAPE, "peaked", 0)]


@pytest.mark.parametrize("shape,kind,waves", KERNEL_CASES, ids=lambda x: "N%d_T%d_D%d_C%d" % x if isinstance(x, tuple) else str(x))
def test_backward_kernels_against_float64(dev, shape, kind, waves):
    """waves: the workgroup form of the FORWARD that wrote o and lse (0: its own dispatch, four waves at these sizes; 8: forced).

    In the peaked case the softmax is one-hot, the exact gq cancels to nearly nothing, and what the emulation and the kernels both
    return for it is the bf16 rounding of the stored o inside delta: both relative errors are huge (9e4 measured) and equal -- the
    ratio is what is asserted.  That case pins gv, delta and the forward's rescale path; gq is pinned by the moderate cases."""
    n, t, d, c = shape
    q, v, go = R.data(kind, n, t, d, c, R.case_seed(n, t, d, c))
    q16, v16, god = q.to(BF).to(dev), v.to(BF).to(dev), go.to(dev)
    o16, lse = _forward(dev, q16, v16, waves)
    go16, delta = _prep(dev, god, o16, d)
    gq, gv = _backward(dev, q16, v16, go16, lse, delta)

    # the prep pass against the operands it read: go16 is round-to-nearest-even of go bit for bit; delta is a C-term fp32 sum of fp32
    # products (C / 8 lanes x 8 fused steps and a shuffle tree: at most C roundings of partial sums bounded by sum |go o|)
    assert torch.equal(_bits16(go16), _bits16(go.to(BF)))
    o64 = o16.cpu().double()
    delta_ref = (go.double() * o64).sum(-1)
    bound = (c + 2) * U24 * (go.double().abs() * o64.abs()).sum(-1)
    err = (delta.cpu().double() - delta_ref).abs()
    print(f"\n{shape} {kind} fwd waves {waves}: delta max err / bound {float((err / bound).max()):.3f}")
    assert bool(torch.isfinite(delta).all()) and bool((err <= bound).all())

    ref = R.attention(q.to(BF), v.to(BF), go)            # float64 on the operands the kernels take
    emu = R.attention(q.to(BF), v.to(BF), go, R.bf16)    # ... with the kernels' rounding points
    _adjudicate(f"backward {shape} {kind}, forward on {waves or 4} waves",
                {"gq": (gq, emu["gq"], ref["gq"]), "gv": (gv, emu["gv"], ref["gv"])})


@pytest.mark.parametrize("shape", [(3, 384, 64, 256), (1, 512, 32, 128)], ids=lambda s: "N%d_T%d_D%d_C%d" % s)
def test_backward_is_reproducible_without_the_deterministic_mode(dev, shape):
    n, t, d, c = shape
    assert FF._L().get_deterministic() == 0
    q, v, go = R.data("moderate", n, t, d, c, R.case_seed(n, t, d, c))
    q16, v16, god = q.to(BF).to(dev), v.to(BF).to(dev), go.to(dev)
    o16, lse = _forward(dev, q16, v16)
    go16, delta = _prep(dev, god, o16, d)
    go16b, deltab = _prep(dev, god, o16, d)
    assert torch.equal(_bits16(go16), _bits16(go16b)) and torch.equal(_bits32(delta), _bits32(deltab))
    a, b = _backward(dev, q16, v16, go16, lse, delta), _backward(dev, q16, v16, go16, lse, delta)
    assert torch.equal(_bits32(a[0]), _bits32(b[0])) and torch.equal(_bits32(a[1]), _bits32(b[1]))


# ---------------------------------------------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------------------------------------------
def _op_run(q, v, go):
    q, v = q.detach().clone().requires_grad_(True), v.detach().clone().requires_grad_(True)
    o = FF.self_attention_bf16_train(q, v)
    o.backward(go)
    return o, q.grad, v.grad


@pytest.mark.parametrize("shape", [(2, 384, 64, 256), (3, 128, 32, 128)], ids=lambda s: "N%d_T%d_D%d_C%d" % s)
def test_op_under_autograd(dev, shape):
    n, t, d, c = shape
    q, v, go = R.data("moderate", n, t, d, c, 77 + t)
    qd, vd = q.to(dev).requires_grad_(True), v.to(dev).requires_grad_(True)
    o = FF.self_attention_bf16_train(qd, vd)
    assert o.dtype == torch.float32 and o.shape == v.shape
    saved = o.grad_fn.saved_tensors
    assert [s.dtype for s in saved] == [BF, BF, BF, torch.float32]   # q16, v16, o16 and lse: not the fp32 operands
    assert sum(s.numel() * s.element_size() for s in saved) == 2 * n * t * (d + 2 * c) + 4 * n * t
    o.backward(go.to(dev))
    ref, emu = R.attention(q, v, go), R.attention(q, v, go, R.bf16)   # the op rounds q and v itself
    _adjudicate(f"self_attention_bf16_train {shape}", {"o": (o, emu["o"], ref["o"]), "q.grad": (qd.grad, emu["gq"], ref["gq"]),
                                                       "v.grad": (vd.grad, emu["gv"], ref["gv"])})


def test_op_graph_capture_replays_the_eager_bits(dev):
    n, t, d, c = 2, 256, 64, 256
    q, v, go = (x.to(dev) for x in R.data("moderate", n, t, d, c, 91))
    eager = _op_run(q, v, go)
    torch.cuda.synchronize()
    qs, vs, gs = torch.zeros_like(q), torch.zeros_like(v), torch.zeros_like(go)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _op_run(qs, vs, gs)                       # warm-up off the capture: allocator pools, the LDS opt-in of each kernel
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _op_run(qs, vs, gs)
    qs.copy_(q), vs.copy_(v), gs.copy_(go)
    graph.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(("o", "q.grad", "v.grad"), eager, captured):
        assert torch.equal(_bits32(a), _bits32(b)), name


# ---------------------------------------------------------------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------------------------------------------------------------
def _count_entry(monkeypatch, name):
    """count the calls of one library entry (the instance every op goes through)"""
    lib = FF._L()
    calls = []
    real = getattr(lib, name)

    def counted(*a):
        calls.append(1)
        return real(*a)

    monkeypatch.setattr(lib, name, counted)
    return calls


def _auto_attn64(w, b, gamma, x, gy, rnd):
    """Auto_Attn on an NHWC map x [n,h,w,c] in float64, forward and backward written out: q = x W^T + b (fp32 on the device: unrounded
    here), o = attention(q, x), y = gamma o + x; the attention's roundings are R.attention's"""
    n, h, wd, c = x.shape
    xt = x.reshape(n, h * wd, c)
    q = xt @ w.t() + b
    go = gamma * gy.reshape(n, h * wd, c)
    a = R.attention(q, xt, go, rnd)
    y = gamma * a["o"] + xt
    gq = a["gq"]
    gx = gy.reshape(n, h * wd, c) + a["gv"] + gq @ w
    return {"output - x": (y - xt).reshape(x.shape), "x.grad - gy": (gx - gy.reshape(n, h * wd, c)).reshape(x.shape),
            "gamma.grad": (gy.reshape(n, h * wd, c) * a["o"]).sum().reshape(1),
            "query_conv.weight.grad": (gq.reshape(-1, gq.shape[-1]).t() @ xt.reshape(-1, c)), "query_conv.bias.grad": gq.sum((0, 1))}


def test_auto_attn_bf16_against_its_emulation_and_launch_ledger(dev, monkeypatch):
    from face_mask_inpaint_amd.modules.pluralistic_model import base_function as BFN

    torch.manual_seed(6)
    attn = BFN.Auto_Attn(256, None, attn_dtype=BF)
    with torch.no_grad():
        attn.gamma.fill_(0.4)
        attn.query_conv.weight.mul_(0.4)      # |q|^2 of a few units: a softmax that is neither uniform nor one-hot
        attn.query_conv.bias.add_(torch.randn(64) * 0.1)
    attn = attn.to(dev)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 256, 8, 16, generator=g)           # T = 128
    gy = torch.randn(2, 256, 8, 16, generator=g)
    counts = {name: _count_entry(monkeypatch, name) for name in (
        "attention_fwd_bf16", "attention_bwd_prep_bf16", "attention_bwd_bf16", "attention_fwd_f32", "attention_fwd_pieces_f32",
        "attention_bwd_f32", "attention_bwd_pieces_f32")}
    xd = x.to(dev).requires_grad_(True)
    y, _ = attn(xd)
    y.backward(gy.to(dev))
    torch.cuda.synchronize()
    assert {k: len(v) for k, v in counts.items()} == {
        "attention_fwd_bf16": 1, "attention_bwd_prep_bf16": 1, "attention_bwd_bf16": 1, "attention_fwd_f32": 0,
        "attention_fwd_pieces_f32": 0, "attention_bwd_f32": 0, "attention_bwd_pieces_f32": 0}

    nhwc = lambda t: t.detach().cpu().double().permute(0, 2, 3, 1).contiguous()
    w64 = attn.query_conv.weight.detach().cpu().double().reshape(64, 256)
    b64 = attn.query_conv.bias.detach().cpu().double()
    args = (w64, b64, float(attn.gamma.detach().cpu()), nhwc(x), nhwc(gy))
    emu, ref = _auto_attn64(*args, R.bf16), _auto_attn64(*args, R.identity)
    # gamma * out + x and its gradient are dominated by x and gy, which both sides hold exactly: compare the attention's own contribution
    got = {"output - x": nhwc(y) - nhwc(x), "x.grad - gy": nhwc(xd.grad) - nhwc(gy), "gamma.grad": attn.gamma.grad.detach().cpu().double(),
           "query_conv.weight.grad": attn.query_conv.weight.grad.detach().cpu().double().reshape(64, 256),
           "query_conv.bias.grad": attn.query_conv.bias.grad.detach().cpu().double()}
    _adjudicate("Auto_Attn(256, attn_dtype=bf16) on 8 x 16, gamma 0.4", {k: (got[k], emu[k], ref[k]) for k in got})


GEN = dict(ngf=16, z_nc=32, img_f=128, L=0, layers=5, norm="instance", activation="LeakyReLU", use_attn=True)   # attn1: (d_qk, C) = (32, 128)


def _generator_step(g, enc, z, gimg):
    for p in g.parameters():
        p.grad = None
    img = g(enc, z)
    img.backward(gimg)
    return img.detach(), {n: p.grad.detach().clone() for n, p in g.named_parameters() if p.grad is not None}


def _generator_pair(dev, **kw):
    from face_mask_inpaint_amd.modules.pluralistic_model import network

    torch.manual_seed(12)
    a = network.define_g(**GEN)
    with torch.no_grad():
        a.attn1.gamma.fill_(0.4)
    b = network.define_g(**GEN, **kw)
    b.load_state_dict(copy.deepcopy(a.state_dict()), strict=True)
    g = torch.Generator().manual_seed(13)
    enc = torch.randn(2, 128, 2, 4, generator=g).to(dev)       # attn1 sees 8 x 16: T = 128, the smallest multiple of 128
    z = torch.randn(2, 32, 2, 4, generator=g).to(dev)
    gimg = torch.randn(2, 3, 64, 128, generator=g).to(dev)
    return a.to(dev), b.to(dev), enc, z, gimg


def test_generator_default_is_the_explicit_fp32_build_bit_for_bit(dev):
    a, b, enc, z, gimg = _generator_pair(dev, attn_dtype=torch.float32)
    with FF.deterministic():     # the fp32 path sums some gradients with atomics: its reproducible mode makes bits comparable
        ia, ga = _generator_step(a, enc, z, gimg)
        ib, gb = _generator_step(b, enc, z, gimg)
    assert torch.equal(_bits32(ia), _bits32(ib))
    assert sorted(ga) == sorted(gb) and len(ga) > 20
    for name in ga:
        assert torch.equal(_bits32(ga[name]), _bits32(gb[name])), name


def test_generator_with_bf16_attention_trains(dev, monkeypatch):
    a, b, enc, z, gimg = _generator_pair(dev, attn_dtype=BF)
    fwd16, bwd16 = _count_entry(monkeypatch, "attention_fwd_bf16"), _count_entry(monkeypatch, "attention_bwd_bf16")
    ib, gb = _generator_step(b, enc, z, gimg)
    assert (len(fwd16), len(bwd16)) == (1, 1)
    ia, ga = _generator_step(a, enc, z, gimg)
    assert (len(fwd16), len(bwd16)) == (1, 1)      # the fp32 build does not touch them
    assert sorted(ga) == sorted(gb)
    for name, grad in gb.items():
        assert bool(torch.isfinite(grad).all()), name
    assert bool(torch.isfinite(ib).all())
    # a property of bf16 attention inside this generator, not of the kernels: recorded, not bounded
    num = sum(float((gb[k].double() - ga[k].double()).pow(2).sum()) for k in ga) ** 0.5
    den = sum(float(ga[k].double().pow(2).sum()) for k in ga) ** 0.5
    print(f"\nResGenerator(attn_dtype=bf16) against the fp32 build, 2 x 4 feature map: image rel L2 {R.rel_l2(ib, ia):.3e}, "
          f"parameter gradients rel L2 {num / den:.3e}")
