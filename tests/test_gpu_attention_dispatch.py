"""GPU: every kernel variant and dispatch branch of csrc/attention.hip against float64, through the C entry points.

Which kernel runs is decided inside the entry points from (N, T, D, C1 + C2) and the reproducible-mode flag:
  forward   fmi_attention_fwd_waves(N, T)      8 if T % 256 == 0 and (T/256) N >= 256, else 2 if (T/128) N < 256, else 4
  backward  fmi_attention_bwd_structure(N, T)  2 if T % 128 == 0 and (T/128) N >= 128, else 1
Every shape below is the smallest that reaches its branch, and every test asserts the predicate for its shape first: a later retune
of a threshold fails here instead of silently moving the cases onto another kernel.

The reference is float64 softmax(q q^T) v, its logsumexp and its autograd, on the device, in chunks of images (no score tensor above
0.5 GB).  Bounds are the suite's existing ones: outputs rtol 1e-4 / atol 2e-5 and lse 1e-5 / 1e-5 (test_fused_attention_forward and
test_forward_on_the_key_tile_image), dQ max|err| <= 2e-5 max|dQ64| + 1e-6 and dV 1e-4 / 2e-5
(test_fused_attention_backward_key_block_structure).

Inputs, each case once per kind:
  randn   q = randn * 0.8 in the forward tests and randn * 2 / sqrt(D) in the backward tests (why: _sigma), v and gO = randn
  edge    image 0: the outlier keys of test_fused_attention_forward (q[0, 5] *= 6, q[0, T - 3] *= 9: scores in the thousands, one-hot
          rows, the lazy-rescale branch); one image with q == 0 (uniform attention, lse = log T); one image whose second upstream
          gradient is all zero (dV2 of that image must be exactly zero).  With N = 2 the last two share image 1; N = 1 has the first."""
import functools
import math

import pytest
import torch

from test_gpu_attention_pieces import _bwd, _fwd_old, _fwd_pieces

pytestmark = pytest.mark.gpu

KINDS = ("randn", "edge")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def FF():
    from face_mask_inpaint_amd import functional

    return functional


def _edge_images(n):
    """(image with q == 0, image with gO2 == 0), None where N has no room"""
    if n == 1:
        return None, None
    return 1, (2 if n >= 3 else 1)


def _make_q(n, t, d, kind, dev, sigma=0.8):
    g = torch.Generator(device=dev).manual_seed(100003 * t + 101 * d + 7)
    q = torch.randn(n, t, d, generator=g, device=dev) * (sigma if kind == "randn" else 0.8)
    if kind == "edge":
        q[0, 5] *= 6.0
        q[0, t - 3] *= 9.0
        zi, _ = _edge_images(n)
        if zi is not None:
            q[zi] = 0.0
    return q


def _make_v(n, t, cs, kind, dev, seed):
    g = torch.Generator(device=dev).manual_seed(100003 * t + 101 * sum(cs) + 13 * len(cs) + seed)
    return [torch.randn(n, t, c, generator=g, device=dev) for c in cs]


def _make_go(n, t, cs, kind, dev):
    gos = _make_v(n, t, cs, kind, dev, 5)
    if kind == "edge" and len(cs) > 1:
        _, gi = _edge_images(n)
        if gi is not None:
            gos[1][gi] = 0.0
    return gos


def _chunk(t):
    return max(1, int(0.5e9 // (t * t * 8)))


@functools.lru_cache(maxsize=2)
def _forward_ref(n, t, d, kind, dev):
    """(q, float64 attention map [N, T, T], float64 lse [N, T]) of one (shape, D, input kind): shared by the cases that differ in the
    value channels only, and left unchanged by them (two entries: the input kind varies fastest)"""
    q = _make_q(n, t, d, kind, dev)
    att, lse = [], []
    for n0 in range(0, n, _chunk(t)):
        q64 = q[n0:n0 + _chunk(t)].double()
        s = q64 @ q64.transpose(1, 2)
        lse.append(torch.logsumexp(s, -1))
        att.append(torch.softmax(s, -1))
    return q, torch.cat(att), torch.cat(lse)


def _backward_ref(q, vs, gos):
    """float64 autograd: (o64 list, lse64, dQ64, dV64 list)"""
    n, t, _ = q.shape
    outs, lses, gq, gvs = [], [], [], []
    for n0 in range(0, n, _chunk(t)):
        sl = slice(n0, n0 + _chunk(t))
        q64 = q[sl].double().requires_grad_(True)
        v64 = [v[sl].double().requires_grad_(True) for v in vs]
        s = q64 @ q64.transpose(1, 2)
        o = [torch.softmax(s, -1) @ v for v in v64]
        torch.autograd.backward(o, [g[sl].double() for g in gos])
        outs.append([x.detach() for x in o])
        lses.append(torch.logsumexp(s.detach(), -1))
        gq.append(q64.grad)
        gvs.append([v.grad for v in v64])
    cat = lambda parts: [torch.cat(p) for p in zip(*parts)]
    return cat(outs), torch.cat(lses), torch.cat(gq), cat(gvs)


def _close(what, got, ref, rtol, atol):
    """|got - ref| <= atol + rtol |ref| everywhere (torch.testing.assert_close's rule), printing the worst figures"""
    got = got.double()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all()), what
    err = (got - ref).abs()
    over = err - rtol * ref.abs()
    excess = float(over.max())
    at = tuple(int(i) for i in torch.unravel_index(over.argmax(), over.shape))
    print(f"{what}: max|err| {float(err.max()):.3g}, worst excess over {rtol:g}|ref| {excess:.3g} at {at} (atol {atol:g})")
    assert excess <= atol, (what, excess, atol, at)


def _check_forward(tag, q, vs, outs, lse, att64, lse64, kind):
    for i, (o, v) in enumerate(zip(outs, vs)):
        _close(f"{tag} o{i + 1}", o, att64 @ v.double(), 1e-4, 2e-5)
    _close(f"{tag} lse", lse, lse64, 1e-5, 1e-5)
    zi, _ = _edge_images(q.shape[0])
    if kind == "edge" and zi is not None:  # q == 0: uniform attention
        assert float((lse[zi].double() - math.log(q.shape[1])).abs().max()) <= 1e-5


def _check_backward(tag, gq, gvs, gq64, gv64, kind, n):
    """the list of misses (empty: within every bound), every figure printed"""
    bad = []
    scale = float(gq64.abs().max())
    err = float((gq.double() - gq64).abs().max())
    print(f"{tag} dQ: max|err| {err:.3g} = {err / scale:.3g} of max|dQ64| {scale:.3g} (bound 2e-5)")
    if not (bool(torch.isfinite(gq).all()) and err <= 2e-5 * scale + 1e-6):
        bad.append((f"{tag} dQ", err, scale))
    for i, (a, b) in enumerate(zip(gvs, gv64)):
        try:
            _close(f"{tag} dV{i + 1}", a, b, 1e-4, 2e-5)
        except AssertionError as e:
            bad.append(e.args[0])
    _, gi = _edge_images(n)
    if kind == "edge" and len(gvs) > 1 and gi is not None and bool(gvs[1][gi].any()):  # gO2 == 0 on that image
        bad.append(f"{tag} dV2 of image {gi} is not zero")
    return bad


# ------------------------------------------------------------------------------------------------
# forward: every wave count x every (D, C / 32) instantiation
FWD_SHAPES = [  # (N, T, waves)
    (256, 128, 4),   # T % 256 != 0, one workgroup per image
    (86, 384, 4),    # three workgroups per image
    (128, 256, 4),   # T % 256 == 0, below the eight-wave threshold
    (256, 256, 8),   # one workgroup per image
    (128, 512, 8),   # two workgroups per image
]
# all six instantiations, C2 = 0, and unequal C1 / C2 splits; with D = 16 the K staging guard f < 8 D is live at 4 and 8 waves
FWD_VARIANTS = [(64, (256,)), (64, (32, 96)), (32, (128, 128)), (32, (96, 32)), (16, (64,)), (16, (32, 32)), (16, (128,)), (16, (96, 32))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d,cs", FWD_VARIANTS)
@pytest.mark.parametrize("n,t,waves", FWD_SHAPES)
def test_forward_wave_count_variants(dev, FF, n, t, waves, d, cs, kind):
    """fmi_attention_fwd_f32 at 4 and 8 waves (attn_fwd_x6_kernel<D, NCT, 4 | 8, false>), o1 / o2 / lse against float64.
    Measured on an MI355X, worst over the cases: randn o max|err| 5.0e-6 (1.7e-6 over 1e-4 |ref|, atol 2e-5), lse 2.9e-5 (inside
    1e-5 |ref| alone); edge o 1.3e-5 (8.4e-6 over), lse 6.7e-4 at |lse| ~ 3300 (inside 1e-5 |ref| alone).  Without the final 1 / l of
    the four-wave kernel exactly the 48 four-wave cases fail, and nothing else in this file."""
    assert FF._L().attention_fwd_waves(n, t) == waves
    q, att64, lse64 = _forward_ref(n, t, d, kind, dev)
    vs = _make_v(n, t, cs, kind, dev, 1)
    outs, lse = _fwd_old(FF, q, vs)
    _check_forward(f"fwd {waves}w N{n} T{t} D{d} C{cs} {kind}", q, vs, outs, lse, att64, lse64, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d,cs", FWD_VARIANTS[:4])
@pytest.mark.parametrize("n,t", [(256, 256), (128, 512)])
def test_image_forward_equals_the_eight_wave_kernel(dev, FF, n, t, d, cs, kind):
    """fmi_attention_fwd_pieces_f32 bit-equal to fmi_attention_fwd_f32 where that IS the eight-wave register-staged kernel (the shapes
    of test_forward_on_the_key_tile_image stay at two waves), and both within the float64 bounds (the figures of the eight-wave cases
    above: o 5.0e-6 / 1.3e-5, lse 2.5e-5 / 6.7e-4 for randn / edge)"""
    lib = FF._L()
    c1, c2 = cs[0], (cs[1] if len(cs) > 1 else 0)
    assert lib.attention_fwd_waves(n, t) == 8 and lib.attention_fwd_uses_pieces(n, t, d, c1, c2) == 1
    q, att64, lse64 = _forward_ref(n, t, d, kind, dev)
    vs = _make_v(n, t, cs, kind, dev, 1)
    outs, lse, _ = _fwd_pieces(FF, q, vs)
    outs0, lse0 = _fwd_old(FF, q, vs)
    assert torch.equal(lse, lse0) and all(torch.equal(a, b) for a, b in zip(outs, outs0))
    _check_forward(f"fwd image N{n} T{t} D{d} C{cs} {kind}", q, vs, outs, lse, att64, lse64, kind)


# ------------------------------------------------------------------------------------------------
# backward
BWD_VARIANTS = [(64, (256,)), (64, (32, 96)), (32, (128, 128)), (32, (128,))]   # the four instantiations, C2 = 0 and C2 > 0


def _sigma(d):
    """The ordinary inputs of the backward tests: q = randn * 2 / sqrt(D), so that |q_i|^2 ~ 4 and a row's own key does not take the
    whole row.  The forward's randn * 0.8 makes |q_i|^2 ~ 41 at D = 64 against cross scores of sigma ~ 5: the softmax is the identity
    to 1e-9, and dQ64 is a residue of 2e-5 .. 3e-2 left by the cancellation of terms of size 16.  A bound relative to max|dQ64| is then
    below what fp32 can give at all: torch's own fp32 autograd on the CPU has 0.15 of max|dQ64| at (T, D, C) = (128, 64, 256) and
    2.7e-4 at (384, 64, 128) there, against 5e-7 .. 1.1e-6 (2e-6 for P = exp(S - lse) evaluated in fp32) on these inputs at every
    shape below."""
    return 2.0 / math.sqrt(d)


def _backward_case(FF, n, t, d, cs, kind, dev):
    """inputs, the forward's results and the float64 reference"""
    q = _make_q(n, t, d, kind, dev, _sigma(d))
    vs, gos = _make_v(n, t, cs, kind, dev, 1), _make_go(n, t, cs, kind, dev)
    _, _, gq64, gv64 = _backward_ref(q, vs, gos)
    outs, lse = _fwd_old(FF, q, vs)
    return q, vs, gos, outs, lse, gq64, gv64


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d,cs", BWD_VARIANTS)
@pytest.mark.parametrize("n,t", [(1, 128), (2, 384), (127, 128)])
def test_backward_first_structure(dev, FF, n, t, d, cs, kind):
    """attn_bwd_kernel<D, NCT> through fmi_attention_bwd_f32, all four instantiations, against float64 autograd with the bounds of the
    second structure's test; reproducible mode: two runs bit-equal, and within the same bounds.
    Measured on an MI355X, worst over the cases: randn dQ 1.1e-6 of max|dQ64|, dV 4.1e-6 (2.4e-7 over 1e-4 |ref|, atol 2e-5); edge dQ
    2.4e-6, dV 5.1e-5 (1.5e-5 over).  With the score tile as a plain fp32 product split over d (before this test existed) the edge
    cases had dV 6.5e-4 over at the outlier keys: see attn_bwd_kernel."""
    lib = FF._L()
    assert lib.attention_bwd_structure(n, t) == 1 and lib.get_deterministic() == 0
    q, vs, gos, outs, lse, gq64, gv64 = _backward_case(FF, n, t, d, cs, kind, dev)
    gq, gvs, _, _ = _bwd(FF, q, vs, outs, gos, lse, False)
    bad = _check_backward(f"bwd1 N{n} T{t} D{d} C{cs} {kind}", gq, gvs, gq64, gv64, kind, n)
    old = lib.set_deterministic(1)
    try:
        a = _bwd(FF, q, vs, outs, gos, lse, False)
        b = _bwd(FF, q, vs, outs, gos, lse, False)
    finally:
        lib.set_deterministic(old)
    bad += _check_backward(f"bwd1 reproducible N{n} T{t} D{d} C{cs} {kind}", a[0], a[1], gq64, gv64, kind, n)
    assert not bad, bad
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("d,cs", BWD_VARIANTS)
@pytest.mark.parametrize("n,t", [(2, 96), (3, 160)])
def test_backward_refuses_a_sequence_the_forward_cannot_produce(dev, FF, n, t, d, cs):
    """T % 128 != 0.  The kernel itself runs any T % 32 == 0, and with o and lse from float64 (rounded; there is no forward for these
    T) it is within the bounds on the randn inputs.  But P = exp(S - lse) is only as good as the agreement of the backward's scores
    with the rounding that lse carries: at the outlier keys of the edge inputs |S| ~ 1650 .. 3300, the kernel's score is 1 - 3 fp32
    ulp (2.4e-4 each) off the float64 one, and so are that row's P and that key's dV -- measured on an MI355X with a build that still
    accepted these T: dV 2.2e-5 .. 1.6e-3 over 1e-4 |dV64| (atol 2e-5) at keys 5 and T - 3 of image 0 in 7 of the 8 edge cases.  Only
    the forward's own lse cancels that rounding.  So the entry point takes what the forward takes, and says so before anything is
    launched: outputs untouched."""
    lib = FF._L()
    assert lib.attention_bwd_structure(n, t) == 1
    q = _make_q(n, t, d, "randn", dev, _sigma(d))
    vs, gos = _make_v(n, t, cs, "randn", dev, 1), _make_go(n, t, cs, "randn", dev)
    o64, lse64, _, _ = _backward_ref(q, vs, gos)
    outs, lse = [o.float() for o in o64], lse64.float()
    gq, gvs, delta = torch.zeros_like(q), [torch.full_like(v, 7.0) for v in vs], torch.full((n, t), 7.0, device=dev)
    two, p = len(cs) > 1, FF._p
    rc = lib.cdll.fmi_attention_bwd_f32(p(q), p(vs[0]), p(vs[1]) if two else None, p(outs[0]), p(outs[1]) if two else None, p(gos[0]),
                                        p(gos[1]) if two else None, p(lse), p(delta), p(gvs[0]), p(gvs[1]) if two else None, p(gq),
                                        n, t, d, cs[0], cs[1] if two else 0, FF._st())
    assert rc == 2   # FMI_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not bool(gq.any()) and all(bool((g == 7.0).all()) for g in gvs) and bool((delta == 7.0).all())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d,cs", BWD_VARIANTS)
def test_backward_across_the_structure_boundary(dev, FF, d, cs, kind):
    """(T/128) N = 127 | 128 on one data pattern: 127 images take the first structure, 128 the second -- once through
    fmi_attention_bwd_f32 in the default mode (the register-staged attn_bwd2_x6_kernel with its atomics, which the library's own dispatch
    leaves to the reproducible mode) and once on the query-tile image; dV has one writer per row: bit-equal between those two.
    Measured on an MI355X, worst over the cases (randn / edge): N = 127 dQ 1.1e-6 / 2.0e-6 of max|dQ64|, dV 2.4e-7 / 7.0e-6 over
    1e-4 |ref| (atol 2e-5); N = 128, both runs alike, dQ 1.3e-6 / 2.3e-6, dV 2.6e-7 / 6.0e-6 over."""
    lib = FF._L()
    t = 128
    c1, c2 = cs[0], (cs[1] if len(cs) > 1 else 0)
    assert lib.attention_bwd_structure(127, t) == 1 and lib.attention_bwd_structure(128, t) == 2
    assert lib.attention_bwd_uses_pieces(127, t, d, c1, c2) == 0 and lib.attention_bwd_uses_pieces(128, t, d, c1, c2) == 1
    assert lib.get_deterministic() == 0
    q, vs, gos, outs, lse, gq64, gv64 = _backward_case(FF, 128, t, d, cs, kind, dev)
    below = [x[:127].contiguous() for x in (q, *vs, *gos, *outs, lse)]
    k = len(cs)
    gq, gvs, _, _ = _bwd(FF, below[0], below[1:1 + k], below[1 + 2 * k:1 + 3 * k], below[1 + k:1 + 2 * k], below[-1], False)
    bad = _check_backward(f"bwd N127 D{d} C{cs} {kind}", gq, gvs, gq64[:127], [g[:127] for g in gv64], kind, 127)
    gq_r, gvs_r, _, _ = _bwd(FF, q, vs, outs, gos, lse, False)
    bad += _check_backward(f"bwd N128 register-staged D{d} C{cs} {kind}", gq_r, gvs_r, gq64, gv64, kind, 128)
    gq_i, gvs_i, _, _ = _bwd(FF, q, vs, outs, gos, lse, True)
    bad += _check_backward(f"bwd N128 image D{d} C{cs} {kind}", gq_i, gvs_i, gq64, gv64, kind, 128)
    assert not bad, bad
    assert all(torch.equal(a, b) for a, b in zip(gvs_r, gvs_i))


# ------------------------------------------------------------------------------------------------
# the autograd glue of functional.self_attention
def _through_autograd(FF, q, vs, gos, used=None):
    qd = q.clone().requires_grad_(True)
    vds = [v.clone().requires_grad_(True) for v in vs]
    res = FF.self_attention(qd, vds)
    used = range(len(vs)) if used is None else used
    torch.autograd.backward([res[i] for i in used], [gos[i] for i in used])
    return [r.detach() for r in res], qd.grad, [v.grad for v in vds]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,t,d,cs", [(256, 256, 32, (128,)), (128, 512, 64, (128, 128))])
def test_self_attention_takes_the_images(dev, FF, n, t, d, cs, kind):
    """the branches of functional.py that allocate the images and call the _pieces entry points, at the smallest shapes that take
    them: outputs bit-equal to the direct call, gradients within the float64 bounds (measured on an MI355X, randn / edge: dQ 1.1e-6 /
    2.7e-6 of max|dQ64|, dV 2.1e-7 / 9.4e-6 over 1e-4 |ref|, atol 2e-5)"""
    lib = FF._L()
    c1, c2 = cs[0], (cs[1] if len(cs) > 1 else 0)
    assert lib.attention_fwd_uses_pieces(n, t, d, c1, c2) == 1 and lib.attention_bwd_uses_pieces(n, t, d, c1, c2) == 1
    assert FF.FUSED_ATTENTION
    q = _make_q(n, t, d, kind, dev, _sigma(d))
    vs, gos = _make_v(n, t, cs, kind, dev, 1), _make_go(n, t, cs, kind, dev)
    res, gq, gvs = _through_autograd(FF, q, vs, gos)
    outs, _, _ = _fwd_pieces(FF, q, vs)
    assert all(torch.equal(a, b) for a, b in zip(res, outs))
    _, _, gq64, gv64 = _backward_ref(q, vs, gos)
    bad = _check_backward(f"glue image N{n} T{t} D{d} C{cs} {kind}", gq, gvs, gq64, gv64, kind, n)
    assert not bad, bad


def _check_composed(tag, q, vs, gos, res, gq, gvs, used):
    o64, _, gq64, gv64 = _backward_ref(q, [vs[i] for i in used], [gos[i] for i in used])
    for i, o in zip(used, o64):
        _close(f"{tag} o{i + 1}", res[i], o, 1e-4, 2e-5)
    _close(f"{tag} dQ", gq, gq64, 1e-3, 3e-4)   # test_self_attention's bounds for this path
    for i, g in zip(used, gv64):
        _close(f"{tag} dV{i + 1}", gvs[i], g, 1e-4, 1e-5)


@pytest.mark.parametrize("n,t,d,cs", [(2, 128, 16, (64,)), (2, 256, 16, (96, 32))])
def test_self_attention_fused_forward_composed_backward(dev, FF, n, t, d, cs):
    """D = 16: the fused forward saves lse and its outputs, the backward has no fused kernel for (16, C / 32) and must take the GEMM
    composition from what the forward saved (measured on an MI355X: dQ max|err| 3.9e-5, 4.0e-6 over 1e-3 |ref| against atol 3e-4;
    dV 2.1e-6, 2.9e-7 over 1e-4 |ref| against atol 1e-5)"""
    assert FF.FUSED_ATTENTION
    q = _make_q(n, t, d, "randn", dev)
    vs, gos = _make_v(n, t, cs, "randn", dev, 1), _make_go(n, t, cs, "randn", dev)
    assert FF._fused_attn_ok(q, vs)
    res, gq, gvs = _through_autograd(FF, q, vs, gos)
    _check_composed(f"glue D16 T{t} C{cs}", q, vs, gos, res, gq, gvs, range(len(cs)))


def test_self_attention_second_output_unused(dev, FF):
    """the loss is taken on o1 only: v2 receives no gradient (None or all zero), dQ and dV1 are those of o1 alone (measured on an
    MI355X: dQ max|err| 1.0e-4, 8.2e-5 over 1e-3 |ref| against atol 3e-4; dV1 8.9e-6, 1.6e-8 over 1e-4 |ref| against atol 1e-5)"""
    n, t, d, cs = 2, 256, 32, (128, 128)
    q = _make_q(n, t, d, "randn", dev)
    vs, gos = _make_v(n, t, cs, "randn", dev, 1), _make_go(n, t, cs, "randn", dev)
    assert FF._fused_attn_ok(q, vs)
    res, gq, gvs = _through_autograd(FF, q, vs, gos, used=[0])
    assert gvs[1] is None or not bool(gvs[1].any())
    _check_composed("glue o1 only", q, vs, gos, res, gq, gvs, [0])
