"""GPU: the attention tile images (csrc/attention.hip: AttKImg, AttQImg), the passes that cut them and the kernels that stream them by
LDS-DMA, through the C entry points (fmi_attention_fwd_pieces_f32 / fmi_attention_bwd_pieces_f32), which take every supported shape --
also those the library's own dispatch leaves to the register-staged kernels.

Layouts undone here (one block per 32 rows of the flattened [N T] axis, padded to whole KiB):
  key tile    K pieces [3][32][2 D + 16 B], V pieces [3][32][2 CT + 64 B]
  query tile  gO pieces [3][32][2 CT B] with the 16-byte chunk c of row r stored at (c & ~15) | ((c ^ swz(r)) & 15),
              swz(r) = ((r & 3) << 2) | ((r >> 2) & 3); Q pieces [3][32][192 B]; lse[32], delta[32] (fp32)
Every image is filled with 0xFF bytes (bf16 / fp32 NaN patterns) before the pass: padding must come back untouched, and a consumer
that read padding as data would produce NaN."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def FF():
    from face_mask_inpaint_amd import functional

    return functional


def _image(FF, which, n, t, d, c1, c2, dev):
    nbytes = C.c_int64(0)
    getattr(FF._L(), f"attention_{which}_image_bytes")(n, t, d, c1, c2, C.byref(nbytes))
    assert nbytes.value > 0 and nbytes.value % (1024 * n * (t // 32)) == 0, nbytes.value  # whole KiB per block
    return torch.full((nbytes.value,), 0xFF, device=dev, dtype=torch.uint8)


def _fwd_old(FF, q, vs):
    n, t, d = q.shape
    outs = [torch.empty_like(v) for v in vs]
    lse = torch.empty(n, t, device=q.device)
    two = len(vs) > 1
    FF._L().attention_fwd_f32(FF._p(q), FF._p(vs[0]), FF._p(vs[1]) if two else None, FF._p(outs[0]), FF._p(outs[1]) if two else None,
                              FF._p(lse), n, t, d, vs[0].shape[2], vs[1].shape[2] if two else 0, FF._st())
    return outs, lse


def _fwd_pieces(FF, q, vs):
    n, t, d = q.shape
    c1, c2 = vs[0].shape[2], (vs[1].shape[2] if len(vs) > 1 else 0)
    img = _image(FF, "fwd", n, t, d, c1, c2, q.device)
    outs = [torch.empty_like(v) for v in vs]
    lse = torch.empty(n, t, device=q.device)
    two = len(vs) > 1
    FF._L().attention_fwd_pieces_f32(FF._p(q), FF._p(vs[0]), FF._p(vs[1]) if two else None, FF._p(img), img.numel(), FF._p(outs[0]),
                                     FF._p(outs[1]) if two else None, FF._p(lse), n, t, d, c1, c2, FF._st())
    return outs, lse, img


def _bwd(FF, q, vs, outs, gos, lse, pieces):
    n, t, d = q.shape
    c1, c2 = vs[0].shape[2], (vs[1].shape[2] if len(vs) > 1 else 0)
    two = len(vs) > 1
    gq = torch.zeros_like(q)
    gvs = [torch.full_like(v, float("nan")) for v in vs]
    delta = torch.empty(n, t, device=q.device)
    p = FF._p
    head = (p(q), p(vs[0]), p(vs[1]) if two else None, p(outs[0]), p(outs[1]) if two else None, p(gos[0]), p(gos[1]) if two else None,
            p(lse), p(delta))
    tail = (p(gvs[0]), p(gvs[1]) if two else None, p(gq), n, t, d, c1, c2, FF._st())
    img = None
    if pieces:
        img = _image(FF, "bwd", n, t, d, c1, c2, q.device)
        FF._L().attention_bwd_pieces_f32(*head, p(img), img.numel(), *tail)
    else:
        FF._L().attention_bwd_f32(*head, *tail)
    return gq, gvs, delta, img


def _split3_ref(FF, x):
    """fmi_split3_f32 of x [rows, C] -> int16 bit patterns [3, rows, C]"""
    rows, c = x.shape
    x3 = torch.empty(rows * c * 3, device=x.device, dtype=torch.int16)
    FF._L().split3_f32(FF._p(x), C.c_void_p(x3.data_ptr()), None, rows, c, 0, 0.0, FF._st())
    return x3.view(rows, c // 16, 3, 16).permute(2, 0, 1, 3).reshape(3, rows, c)


def _as_f32(bits16):
    return (bits16.to(torch.int32) << 16).view(torch.float32)


def _stress(rows, c, g, kinds=("large", "tiny", "below", "zeros", "ordinary")):
    """values that stress the three-way split, one kind per row in turn: +-large; `tiny` = |x| in [2^-109, 2^-107): the third piece is a
    bf16 subnormal (below 2^-126) but x still lies on the subnormal grid of 2^-133; `below` = |x| ~ 1e-36 .. 1e-38, second and third piece
    subnormal and x finer than that grid; zeros and signed zeros among ordinary values; ordinary"""
    x = torch.randn(rows, c, generator=g)
    k = len(kinds)
    for i, kind in enumerate(kinds):
        if kind == "large":
            x[i::2 * k] *= 1e30
            x[i + k::2 * k] *= -3e37
        elif kind == "tiny":
            m = torch.rand(rows, c, generator=g) + 1.0
            x[i::2 * k] = (torch.sign(x) * m)[i::2 * k] * 2.0 ** -108
            x[i + k::2 * k] = (torch.sign(x) * m)[i + k::2 * k] * 2.0 ** -109
        elif kind == "below":
            x[i::2 * k] *= 1e-36
            x[i + k::2 * k] *= 3e-38
        elif kind == "zeros":
            x[i::k, ::3] = 0.0
            x[i::k, 1::5] = -0.0
    return x


def _swz(r):
    return ((r & 3) << 2) | ((r >> 2) & 3)


@pytest.mark.parametrize("d,cs", [(64, (256,)), (32, (96, 32)), (64, (32, 96)), (32, (128, 128))])
def test_cut_pass_pieces_and_padding(dev, FF, d, cs):
    """both images, after undoing the layout: the three pieces of every element are bit for bit those of fmi_split3_f32 (the exactness of
    their sum: test_cut_pass_sum_is_exact); lse / delta ride along unchanged; every padding byte keeps its 0xFF fill"""
    n, t = 2, 256
    ct, c1, c2 = sum(cs), cs[0], (cs[1] if len(cs) > 1 else 0)
    g = torch.Generator().manual_seed(d + ct + c2)
    q = _stress(n * t, d, g).to(dev).view(n, t, d)
    xs = [_stress(n * t, c, g).to(dev) for c in cs]
    if len(xs) > 1:
        xs[1] = xs[1] * 1.5   # the C2 half differs from the C1 half
    xs = [x.view(n, t, -1).contiguous() for x in xs]
    lse = torch.randn(n, t, generator=g).to(dev)
    o = [torch.randn(n, t, c, generator=g).to(dev) for c in cs]
    nblk = n * t // 32
    cat = torch.cat([x.view(n * t, -1) for x in xs], 1).contiguous()
    ref_x, ref_q = _split3_ref(FF, cat), _split3_ref(FF, q.view(n * t, d).contiguous())

    # ---- key-tile image (forward): cut from q and v = xs
    _, _, img = _fwd_pieces(FF, q, xs)
    blk = img.view(nblk, -1)
    kp, vp = 2 * d + 16, 2 * ct + 64
    kimg, vimg = 32 * kp, 32 * vp
    K = blk[:, :3 * kimg].reshape(nblk, 3, 32, kp)
    V = blk[:, 3 * kimg:3 * kimg + 3 * vimg].reshape(nblk, 3, 32, vp)
    gotk = K[..., :2 * d].contiguous().view(torch.int16).permute(1, 0, 2, 3).reshape(3, n * t, d)
    gotv = V[..., :2 * ct].contiguous().view(torch.int16).permute(1, 0, 2, 3).reshape(3, n * t, ct)
    assert torch.equal(gotk, ref_q) and torch.equal(gotv, ref_x)
    assert bool((K[..., 2 * d:] == 0xFF).all()) and bool((V[..., 2 * ct:] == 0xFF).all()) and bool((blk[:, 3 * kimg + 3 * vimg:] == 0xFF).all())

    # ---- query-tile image (backward): cut from q, gO = xs, lse and delta = rowsum(gO o)
    _, _, delta, img = _bwd(FF, q, xs, o, xs, lse, True)
    blk = img.view(nblk, -1)
    gp, qp = 2 * ct, 192
    gimg, qimg = 32 * gp, 32 * qp
    G = blk[:, :3 * gimg].reshape(nblk, 3, 32, ct // 8, 16)
    r = torch.arange(32, device=dev).view(32, 1)
    ch = torch.arange(ct // 8, device=dev).view(1, -1)
    pos = (ch & ~15) | ((ch ^ _swz(r)) & 15)   # [32, ct / 8]: where chunk ch of row r is stored
    G = torch.gather(G, 3, pos.view(1, 1, 32, ct // 8, 1).expand(nblk, 3, 32, ct // 8, 16))
    gotg = G.contiguous().view(torch.int16).permute(1, 0, 2, 3, 4).reshape(3, n * t, ct)
    Q = blk[:, 3 * gimg:3 * gimg + 3 * qimg].reshape(nblk, 3, 32, qp)
    gotq = Q[..., :2 * d].contiguous().view(torch.int16).permute(1, 0, 2, 3).reshape(3, n * t, d)
    assert torch.equal(gotg, ref_x) and torch.equal(gotq, ref_q)
    tail = blk[:, 3 * gimg + 3 * qimg:]
    ld = tail[:, :256].contiguous().view(torch.float32).view(nblk, 2, 32)
    assert torch.equal(ld[:, 0].reshape(n, t), lse)
    assert torch.equal(ld[:, 1].reshape(n, t).view(torch.int32), delta.view(torch.int32))   # bits: the stress values overflow delta to inf / NaN
    assert bool((Q[..., 2 * d:] == 0xFF).all()) and bool((tail[:, 256:] == 0xFF).all())


@pytest.mark.parametrize("kind", ["ordinary", "zeros", "large", "tiny", "below"])
def test_cut_pass_sum_is_exact(dev, FF, kind):
    """the three pieces of every element of both images, added from the smallest up (on the host, in float64: exact), give the input back
    exactly -- also where the third piece is a bf16 subnormal (`tiny`); the C2 half is a different tensor from the C1 half.

    `below`: bf16 keeps fp32's exponent range, so its subnormals lie on a grid of 2^-133 and an fp32 value needs |x| >= 2^-109 for its 24
    bits to fit above that grid: no three bf16 numbers sum to a finer x.  What the format allows is asserted instead: each piece is the
    round-to-nearest of an exact remainder, so the last remainder, and with it |sum - x|, is at most half a grid step, 2^-134.  (Measured
    on an MI355X: e.g. x = -9.414165e-37 -> -9.403955e-37, -1.010190e-39 (a subnormal, correctly rounded), -0.)  The matrix pipe flushes
    subnormal pieces in any case (test_gpu_kernels.py::test_bf16x6_edge_values_on_the_matrix_pipe)."""
    n, t, d, cs = 2, 256, 64, (128, 128)
    g = torch.Generator().manual_seed(len(kind))
    q = _stress(n * t, d, g, (kind,)).to(dev).view(n, t, d)
    xs = [_stress(n * t, c, g, (kind,)).to(dev).view(n, t, c) for c in cs]
    xs[1] = (xs[1] * 1.5).contiguous()
    lse = torch.randn(n, t, generator=g).to(dev)
    nblk = n * t // 32
    cat = torch.cat([x.view(n * t, -1) for x in xs], 1)
    _, _, kimg_ = _fwd_pieces(FF, q, xs)
    _, _, _, qimg_ = _bwd(FF, q, xs, xs, xs, lse, True)
    kp, vp, ct = 2 * d + 16, 2 * sum(cs) + 64, sum(cs)
    kb, qb = kimg_.view(nblk, -1), qimg_.view(nblk, -1)
    K = kb[:, :3 * 32 * kp].reshape(nblk, 3, 32, kp)[..., :2 * d]
    V = kb[:, 3 * 32 * kp:3 * 32 * (kp + vp)].reshape(nblk, 3, 32, vp)[..., :2 * ct]
    G = qb[:, :3 * 32 * 2 * ct].reshape(nblk, 3, 32, ct // 8, 16)
    r = torch.arange(32, device=dev).view(32, 1)
    ch = torch.arange(ct // 8, device=dev).view(1, -1)
    pos = (ch & ~15) | ((ch ^ _swz(r)) & 15)
    G = torch.gather(G, 3, pos.view(1, 1, 32, ct // 8, 1).expand(nblk, 3, 32, ct // 8, 16)).reshape(nblk, 3, 32, 2 * ct)
    Q = qb[:, 3 * 32 * 2 * ct:3 * 32 * (2 * ct + 192)].reshape(nblk, 3, 32, 192)[..., :2 * d]
    worst = []
    for name, img, src in (("K", K, q), ("V", V, cat), ("gO", G, cat), ("Q", Q, q)):
        c = src.shape[-1]
        f = _as_f32(img.contiguous().view(torch.int16).permute(1, 0, 2, 3).reshape(3, n * t, c)).cpu().double()
        x = src.reshape(n * t, c).cpu().double()
        err = float((((f[2] + f[1]) + f[0]) - x).abs().max())
        print(f"{kind} {name}: max |sum - x| = {err:.3g}")
        worst.append(err)
    assert max(worst) <= (2.0 ** -134 if kind == "below" else 0.0), worst


def _inputs(n, t, d, cs, dev):
    g = torch.Generator().manual_seed(t + d + sum(cs) + len(cs))
    q = (torch.randn(n, t, d, generator=g) * 0.5).to(dev)
    vs = [torch.randn(n, t, c, generator=g).to(dev) for c in cs]
    gos = [torch.randn(n, t, c, generator=g).to(dev) for c in cs]
    return q, vs, gos


# one and two key tiles per stage parity (T = 256, 512), every (D, C / 32) instantiation, C2 = 0 and C2 > 0
FWD_CASES = [(2, 256, 64, (256,)), (2, 512, 64, (64, 64)), (2, 512, 32, (128, 128)), (2, 256, 32, (128,))]


@pytest.mark.parametrize("n,t,d,cs", FWD_CASES)
def test_forward_on_the_key_tile_image(dev, FF, n, t, d, cs):
    """o1, o2, lse bit-equal to fmi_attention_fwd_f32 (same pieces, same MFMA order), and within the float64 bounds of the fused
    attention tests (rtol 1e-4, atol 1e-5)"""
    q, vs, _ = _inputs(n, t, d, cs, dev)
    outs, lse, _ = _fwd_pieces(FF, q, vs)
    outs0, lse0 = _fwd_old(FF, q, vs)
    assert torch.equal(lse, lse0)
    for a, b in zip(outs, outs0):
        assert torch.equal(a, b)
    s64 = q.double() @ q.double().transpose(1, 2)
    att = torch.softmax(s64, -1)
    for a, v in zip(outs, vs):
        torch.testing.assert_close(a.double(), att @ v.double(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(lse.double(), torch.logsumexp(s64, -1), rtol=1e-5, atol=1e-5)


# (T / 128) N >= 128 everywhere, so that fmi_attention_bwd_f32 runs the register-staged form of the same kernel; T = 384 = 3 * 128
BWD_CASES = [(64, 256, 64, (256,)), (32, 512, 64, (64, 64)), (32, 512, 32, (128, 128)), (64, 256, 32, (128,)), (48, 384, 64, (128, 128))]


@pytest.mark.parametrize("n,t,d,cs", BWD_CASES)
def test_backward_on_the_query_tile_image(dev, FF, n, t, d, cs):
    """dQ and dV against float64 autograd with the bounds of test_fused_attention_backward_key_block_structure; in the reproducible
    mode two runs are bit-equal, and bit-equal to fmi_attention_bwd_f32 (the register-staged kernel) in that mode"""
    q, vs, gos = _inputs(n, t, d, cs, dev)
    outs, lse = _fwd_old(FF, q, vs)
    q64 = q.double().requires_grad_(True)
    v64 = [v.double().requires_grad_(True) for v in vs]
    att = torch.softmax(q64 @ q64.transpose(1, 2), -1)
    torch.autograd.backward([att @ v for v in v64], [go.double() for go in gos])
    del att
    gq, gvs, _, _ = _bwd(FF, q, vs, outs, gos, lse, True)
    scale = float(q64.grad.abs().max())
    err = float((gq.double() - q64.grad).abs().max())
    print(f"dQ max err {err:.3g} of scale {scale:.3g}")
    assert err <= 2e-5 * scale + 1e-6, (err, scale)
    for gv, v in zip(gvs, v64):
        torch.testing.assert_close(gv.double(), v.grad, rtol=1e-4, atol=2e-5)
    lib = FF._L()
    old = lib.set_deterministic(1)
    try:
        a = _bwd(FF, q, vs, outs, gos, lse, True)
        b = _bwd(FF, q, vs, outs, gos, lse, True)
        c = _bwd(FF, q, vs, outs, gos, lse, False)
    finally:
        lib.set_deterministic(old)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    assert torch.equal(a[0], c[0]) and all(torch.equal(x, y) for x, y in zip(a[1], c[1]))
    for gv, x in zip(gvs, a[1]):  # dV has one writer per row: the same bits in either mode
        assert torch.equal(gv, x)


def test_dispatch_takes_the_images_at_the_decoder_shape(FF):
    """shape dispatch: the long-sequence shapes go through the images, short ones and D = 16 keep the register-staged kernels"""
    lib = FF._L()
    assert lib.attention_fwd_uses_pieces(8, 16384, 64, 128, 128) == 1 and lib.attention_bwd_uses_pieces(8, 16384, 64, 128, 128) == 1
    assert lib.attention_fwd_uses_pieces(8, 1024, 64, 256, 0) == 0 and lib.attention_bwd_uses_pieces(8, 1024, 64, 256, 0) == 0
    assert lib.attention_fwd_uses_pieces(64, 16384, 16, 64, 0) == 0 and lib.attention_bwd_uses_pieces(8, 16384 + 32, 64, 256, 0) == 0
