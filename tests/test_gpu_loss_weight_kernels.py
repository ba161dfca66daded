"""GPU: the kernels of csrc/loss.hip (the seven contextual-loss entries, l2norm_rows, lpips_layer, reduce_loss), dot_f32 / axpy_dev_f32
of csrc/eltwise.hip and csrc/weights.hip (spectral-norm preparation, the packs and their bf16 piece images, the weight gradient,
multi-tensor Adam and Ranger), one by one, against the float64 references of tests/loss_reference.py.

Every kernel is called on operands the test built (through _lib.lib(), or through the thin Python layer where that is the only caller:
FF.prepare_weights, FF.adam_step, Ranger.step); the references get float64 copies of those same fp32 tensors and of the fp32-rounded
scalar arguments.  Optimiser steps are compared one at a time: the reference advances from the KERNEL's fp32 state, not from its own.

Tolerances are derived, none is fitted.  u32 = 2^-24, u64 = 2^-53, mag = the reference's magnitude (the same expression with every
term replaced by its absolute value):
  fp32 element-wise   8 u32 mag
  fp32 reduction      (L + 8) u32 sum|term|, L = the longest chain of fp32 additions the launcher produces for the shape (one thread's
                      run + the wave / workgroup tree + the fp32 atomics); the plan_* helpers restate each launcher's arithmetic and
                      name the source lines.  Where a kernel accumulates in fp64 (reduce_loss beyond 64 terms, dot, the Ranger row
                      means) only the fp32 terms, the fp32 atomics and the final fp32 store count
  expf / logf         4 u32 relative each (EXPLOG).  This is an ASSUMPTION about the device library, not measured here
  exponent            the argument (1 - d / den) / h of cx_rows carries 8 u32 (1 + d / den) / h of rounding (d, den, the quotient, the
                      difference, / h); w = exp(arg) is then off by the factor expm1(that) + 4 u32, as the IR-SE file propagates rstd
  underflow           w = exp(arg) reaches e^-300 in float64 where fp32 ends at 2^-126 (denormals below, which expf may flush): w and
                      cx_ij = w / sum w carry 2^-126 of absolute error each on top
  composite outputs   the element-wise bound plus the propagated bound of the reductions they contain: cx_ij = w / sum w, the dmin
                      correction of cx_bwd, xn = d / ||d||, the l2norm backward's k, and u', v', sigma, W / sigma of the power
                      iteration (first order: products of two error terms are dropped, they are 2^-24 of the terms kept)
  sqrt of a sum       half the sum's relative bound + 1 u32; a quotient by it + 1 u32 more: ((L + 8) / 2 + 4) u32 in all
Bit-exact: colmax / colarg of cx_cols (a maximum of fp32 values rounds nothing), packs without spectral norm and their gradient,
wf against wt of one entry, the piece images' sum against the fp32 pack, iters = 3 against three one-iteration calls, Ranger.step
against the raw entry, FF.contextual_loss / FF.l2norm_rows against the same launches made by hand, L1 gradients.

Indices: arg-min rows are compared where the two smallest float64 d lie more than 2^-20 apart, arg-max columns where the two
largest entries lie more than 1e-5 (relative) apart, at most 1 % excluded; planted exact ties are compared unconditionally (the
smallest index wins).  test_host_loss_reference.py establishes the margins of the seeds used here.

Left out: the 4096-workgroup cap of fmi_bw_grid (common.h) binds from 16.7 M elements (reduce_loss: 4096 x 4096) -- beyond what a
test of a few seconds holds; the grid-stride loops it would exercise run here through the reproducible mode's single workgroup.
The 17 x 17 weights (taps = 289) go through FF.prepare_weights like the others: the Python layer builds that case."""
import ctypes
import functools
import math

import pytest
import torch

import loss_reference as R

pytestmark = pytest.mark.gpu

U32, U64 = 2.0 ** -24, 2.0 ** -53
EXPLOG = 4  # assumed relative error of expf / logf in u32
FMIN32 = 2.0 ** -126  # smallest normal fp32: below it a result is denormal (absolute error up to 2^-149) or flushed to zero
F64 = torch.float64
OMITTED = {
    ("reduce_loss", "fmi_bw_grid cap"): "needs 16.7 M elements (4096 workgroups x 4096); three fp32 tensors of 67 MB and their float64 copies",
}


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


# ---- bounds ------------------------------------------------------------------------------------------------------------------
def _d(t):
    return t.detach().cpu().double()


def _within(got, ref, tol, what):
    got = _d(got).reshape(ref.shape)
    tol = torch.as_tensor(tol, dtype=F64).expand(ref.shape)
    err = (got - ref).abs()
    ok = err <= tol  # False for NaN: an element the kernel never wrote
    if not bool(ok.all()):
        bad = ~ok
        ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.full_like(err, float("inf")))[bad]
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {ok.numel()} elements beyond the bound; worst err / bound = "
                             f"{float(ratio.nan_to_num(float('inf')).max()):.3g}; first at flat index {i}: got {float(got.reshape(-1)[i])!r}, "
                             f"ref {float(ref.reshape(-1)[i])!r}, bound {float(tol.reshape(-1)[i]):.3g}")


def _elem(mag):
    return 8 * U32 * mag


def _red(L, mag):
    return (L + 8) * U32 * mag


def _cdiv(a, b):
    return -(-a // b)


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_KEEP = []


def _up(t, dev):
    """pointer to a device copy of an operand, kept alive until the test ends (a temporary would be freed, and its block handed to
    the next allocation, before the launch that reads it)"""
    _KEEP.append(t.to(dev))
    return _vp(_KEEP[-1])


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    _KEEP.clear()


def _nan(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- the launchers' block arithmetic, restated -----------------------------------------------------------------------------------
def _bw_grid(work, block):
    """common.h fmi_bw_grid(): ceil(work / block), at most 256 x 16 workgroups"""
    return max(1, min(_cdiv(work, block), 4096))


def plan_channel_mean(rows, det=False):
    """loss.hip fmi_cx_channel_mean_f32() (blocks = min(ceil(rows / 64), 1024), 1 in reproducible mode, re-balanced) and
    col_mean_kernel: four row lanes walk rows_per_block, three adds join them, one fp32 atomic per block -> (blocks, L)"""
    blocks = 1 if det else min(_cdiv(rows, 64), 1024)
    rpb = _cdiv(rows, blocks)
    blocks = _cdiv(rows, rpb)
    return blocks, _cdiv(rpb, 4) + 3 + blocks


def plan_wave_row(c):
    """one wave per row (cx_normalise_kernel, cx_normalise_bwd_kernel, l2norm_rows_kernel, l2norm_rows_bwd_kernel of loss.hip,
    wp_wv_kernel of weights.hip): `for (c = lane; c < C; c += 64)` then the six levels of wave_sum (common.h)"""
    return _cdiv(c, 64) + 6


def plan_block_row(p):
    """one 256-thread workgroup per row (cx_rows_kernel, cx_loss_kernel, cx_bwd_kernel of loss.hip, wp_vnorm_kernel, wp_unorm_kernel of
    weights.hip): `for (j = tid; j < P; j += 256)`, then block_sum_256 (common.h): six wave levels and three adds"""
    return _cdiv(p, 256) + 6 + 3


def plan_reduce_loss(n, det=False):
    """loss.hip fmi_reduce_loss_f32(): grid = 1 (reproducible) or fmi_bw_grid(n, 256 * 16); reduce_loss_kernel adds at most 64 terms in
    fp32 before it flushes into fp64 (`++cnt == 64`), block_sum_256_d is fp64, one fp32 atomic per workgroup -> (grid, trips, L)"""
    grid = 1 if det else _bw_grid(n, 256 * 16)
    trips = _cdiv(n, grid * 256)
    return grid, trips, min(trips, 64) + grid


def plan_lpips(total, det=False):
    """loss.hip fmi_lpips_layer_f32(): grid = 1 or fmi_bw_grid(total, 256 * 8); lpips_layer_kernel is fp32 throughout"""
    grid = 1 if det else _bw_grid(total, 256 * 8)
    return grid, _cdiv(total, grid * 256) + 9 + grid


def plan_dot(n, det=False):
    """eltwise.hip fmi_dot_f32(): dot_kernel is fp64 up to the one fp32 atomic per workgroup (grid = 1 or fmi_bw_grid(n, 256 * 8))"""
    grid = 1 if det else _bw_grid(n, 256 * 8)
    return grid, grid


def plan_wg_dot(total, det=False):
    """weights.hip fmi_weight_grad_f32() / wg_dot_kernel: PACK_PER_BLOCK = 2048 elements per workgroup (8 per thread), one fp32 atomic
    each; reproducible mode: grid.x = 1, the one workgroup walks every chunk -> (workgroups of this entry, L)"""
    if det:
        return 1, _cdiv(total, 256) + 9 + 1
    blocks = _cdiv(total, 2048)
    return blocks, 8 + 9 + blocks


def tr_cc(taps):
    """weights.hip tr_cc(): channels per 32-row LDS tile"""
    cc = min(288 // taps, 32)
    if cc >= 8:
        cc &= ~7
    return max(cc, 1)


def pack_path(rows, c, taps):
    """weights.hip wp_pack_kernel / wg_apply_kernel: which wp_tile / wg_tile instantiations a weight reaches"""
    if taps > 288:
        return {"elementwise"}
    cc = tr_cc(taps)
    t = taps if taps in (9, 1) else 0
    kinds = set()
    for r0 in range(0, rows, 32):
        for c0 in range(0, c, cc):
            full = min(c - c0, cc) == cc and min(rows - r0, 32) == 32
            kinds.add((t, full and t != 0))
    return kinds


def test_plans_reach_the_branches_the_cases_are_named_for():
    """a retune of a launcher fails here instead of silently moving a case onto another path"""
    assert [_cdiv(p, 256) for p in (64, 257, 300, 520)] == [1, 2, 2, 3]                       # trips of the 256-stride loops
    assert [plan_wave_row(c) - 6 for c in (7, 64, 24, 96)] == [1, 1, 1, 2] and (2 * 257) % 4 != 0  # rows beyond the last full workgroup of 4
    assert plan_channel_mean(600)[0] > 1 and plan_channel_mean(600, True)[0] == 1
    assert plan_reduce_loss(2 * 16384 + 37, True) == (1, 129, 65)                              # two flushes and a remainder
    assert plan_reduce_loss(5000)[:2] == (2, 10) and plan_lpips(1000 * 192)[0] == 94
    assert pack_path(64, 64, 1) == {(1, True)} and pack_path(40, 24, 1) == {(1, False)}
    assert pack_path(64, 32, 9) == {(9, True)} and pack_path(48, 40, 9) == {(9, True), (9, False)}
    assert tr_cc(16) == 16 and pack_path(32, 16, 16) == {(0, False)} and tr_cc(49) == 5 and pack_path(8, 3, 49) == {(0, False)}
    assert pack_path(5, 3, 289) == {"elementwise"} and 300 > 256
    assert plan_wg_dot(300 * 72)[0] == 11 and plan_wg_dot(300 * 72, True) == (1, 85 + 9 + 1)


# ---- contextual loss -------------------------------------------------------------------------------------------------------------
CX = list(R.CX_SHAPES)
H = R.CX_H
SCALE, GSCALE = R.f32(0.7), R.f32(1.7)
_ids = lambda v: str(v).replace(" ", "")  # noqa: E731


@functools.lru_cache(maxsize=None)
def _cx_case(shape):
    """x, y (fp32, CPU, never modified) and the float64 chain on them, once per shape"""
    n, p, c = shape
    x, y = R.cx_inputs(n, p, c, R.CX_SHAPES[shape])
    return x, y, R.cx_chain(x.double(), y.double(), H, SCALE)


def _norm_factor(c):
    """sqrt of a wave-row sum of squares, and a quotient by it (module docstring)"""
    return ((plan_wave_row(c) + 8) / 2 + 4) * U32


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("shape", CX, ids=_ids)
def test_cx_channel_mean(dev, FF, lib, shape, det):
    n, p, c = shape
    _, y, ch = _cx_case(shape)
    mu = torch.zeros(c, device=dev)
    with FF.deterministic(det):
        lib.cx_channel_mean_f32(_up(y, dev), _vp(mu), n * p, c, FF._st())
    _within(mu, ch.mu.mu, _red(plan_channel_mean(n * p, det)[1], ch.mu.mu_mag), f"cx_channel_mean {shape} det {det}")


@pytest.mark.parametrize("shape", CX, ids=_ids)
def test_cx_normalise_and_backward(dev, FF, lib, shape):
    n, p, c = shape
    x, _, ch = _cx_case(shape)
    rows = n * p
    mu = ch.mu.mu.float()
    ref = R.cx_normalise(x.double().reshape(rows, c), mu.double())
    out, inv = _nan((rows, c), dev), _nan((rows,), dev)
    lib.cx_normalise_f32(_up(x, dev), _up(mu, dev), _vp(out), _vp(inv), rows, c, FF._st())
    k = _norm_factor(c)
    _within(out, ref.xn, k * ref.xn_mag, f"cx_normalise {shape} xn")
    _within(inv, ref.inv, k * ref.inv, f"cx_normalise {shape} inv")
    g, xn32, inv32 = _randn(rows, c, seed=31), ref.xn.float(), ref.inv.float()
    bw = R.cx_normalise_bwd(g.double(), xn32.double(), inv32.double())
    gx = _nan((rows, c), dev)
    lib.cx_normalise_bwd_f32(_up(g, dev), _up(xn32, dev), _up(inv32, dev), _vp(gx), rows, c, FF._st())
    inner = xn32.double().abs() * (inv32.double() * _red(plan_wave_row(c), bw.dot_mag))[:, None]  # the row's own xn . g
    _within(gx, bw.gx, _elem(bw.gx_mag) + inner, f"cx_normalise_bwd {shape}")


def _rows_tols(r, p):
    """(dmin, rowsum, cx_ij) bounds of cx_rows_kernel from the reference r on the same cosine matrix (module docstring: exponent)"""
    darg = 8 * U32 * r.arg_mag
    dw = torch.expm1(darg) + EXPLOG * U32                       # relative error of w = expf(arg)
    ds = (r.w * dw).sum(-1) + _red(plan_block_row(p), r.rowsum) + p * FMIN32
    tol_cx = r.cx * (dw + (ds / r.rowsum)[..., None]) + _elem(r.cx) + FMIN32 * (1 + 1 / r.rowsum[..., None])  # w, then w / s, may underflow
    return _elem(torch.gather(r.d_mag, -1, r.argmin[..., None])[..., 0]), ds, tol_cx


def _check_argmin(got, r, planted, what):
    """planted: [(n, row, expected index)], compared whatever the gap"""
    cmp = r.gap > R.ROW_GAP_BAR
    assert float((~cmp).double().mean()) <= R.EXCLUDED_MAX, what + ": more than 1 % of the rows under the gap bar"
    for n0, i0, _ in planted:
        cmp[n0, i0] = False
    got = got.cpu().long().reshape(r.argmin.shape)
    assert torch.equal(got[cmp], r.argmin[cmp]), f"{what}: arg-min differs on {int((got[cmp] != r.argmin[cmp]).sum())} comparable rows"
    for n0, i0, want in planted:
        assert int(got[n0, i0]) == want, f"{what}: planted tie in row {(n0, i0)}: arg-min {int(got[n0, i0])}, the smallest index is {want}"


def _run_cx_rows(dev, FF, lib, cos32):
    n, p, _ = cos32.shape
    cx, dmin, rsum = _nan((n, p, p), dev), _nan((n, p), dev), _nan((n, p), dev)
    amin = torch.full((n, p), -1, device=dev, dtype=torch.int32)
    lib.cx_rows_f32(_up(cos32, dev), _vp(cx), _vp(dmin), _vp(amin), _vp(rsum), n, p, H, FF._st())
    return cx, dmin, amin, rsum


@pytest.mark.parametrize("shape", CX, ids=_ids)
def test_cx_rows(dev, FF, lib, shape):
    """on the float64 chain's cosine matrix rounded to fp32, with an exact tie planted in row (0, 1): columns 3 and 259 (P - 1 where
    P <= 259; at P = 257 that is the second trip's only column) both hold a value above the row's maximum"""
    n, p, c = shape
    cos32 = _cx_case(shape)[2].cos.float().clone()
    tie = 259 if p > 259 else p - 1
    cos32[0, 1, 3] = cos32[0, 1, tie] = (cos32[0, 1].max() + 1) / 2
    r = R.cx_rows(cos32.double(), H)
    assert int(r.argmin[0, 1]) == 3 and float(r.gap[0, 1]) == 0
    cx, dmin, amin, rsum = _run_cx_rows(dev, FF, lib, cos32)
    what = f"cx_rows {shape}"
    _check_argmin(amin, r, [(0, 1, 3)], what)
    tol_dmin, tol_s, tol_cx = _rows_tols(r, p)
    _within(dmin, r.dmin, tol_dmin, what + " dmin")
    _within(rsum, r.rowsum, tol_s, what + " rowsum")
    _within(cx, r.cx, tol_cx, what + " cx_ij")


@pytest.mark.parametrize("shape", CX, ids=_ids)
def test_cx_cols(dev, FF, lib, shape):
    """the operand is fp32 and a maximum rounds nothing: colmax and colarg are exact, on EVERY column (the 1e-5 bar of the module
    docstring is needed only where the operand itself carries an error, see the end-to-end test); two equal maxima planted in column 2"""
    n, p, c = shape
    cx32 = _cx_case(shape)[2].rows.cx.float().clone()
    cx32[0, 5, 2] = cx32[0, p - 1, 2] = 2.0
    ref = R.cx_cols(cx32.double())
    assert int(ref.colarg[0, 2]) == 5
    cmax, carg = _nan((n, p), dev), torch.full((n, p), -1, device=dev, dtype=torch.int32)
    lib.cx_cols_f32(_up(cx32, dev), _vp(cmax), _vp(carg), n, p, FF._st())
    assert torch.equal(_d(cmax), ref.colmax), f"cx_cols {shape}: colmax is not the exact maximum"
    assert torch.equal(carg.cpu().long(), ref.colarg), f"cx_cols {shape}: colarg is not the first maximum"


def _loss_tols(ls, n, p, scale, dcolmax=None):
    """(cx[n], loss) bounds of cx_loss_kernel; dcolmax [N, P]: a bound the operand itself carries"""
    tol_cx = _red(plan_block_row(p), ls.cx_mag) + (0 if dcolmax is None else dcolmax.mean(1))
    tol_t = EXPLOG * U32 * ls.term.abs() + tol_cx / (ls.cx + R.CX_EPS) + 2 * U32  # logf, its argument, the rounding of cx + 1e-5
    return tol_cx, abs(scale) * tol_t.mean() + _red(n, ls.loss_mag)              # N fp32 atomics (one per sample in both modes)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("shape", CX, ids=_ids)
def test_cx_loss(dev, FF, lib, shape, det):
    n, p, c = shape
    cm32 = _cx_case(shape)[2].cols.colmax.float()
    ls = R.cx_loss(cm32.double(), SCALE)
    cx, loss = _nan((n,), dev), torch.zeros(1, device=dev)
    with FF.deterministic(det):
        lib.cx_loss_f32(_up(cm32, dev), _vp(cx), _vp(loss), n, p, SCALE, FF._st())
    tol_cx, tol_loss = _loss_tols(ls, n, p, SCALE)
    _within(cx, ls.cx, tol_cx, f"cx_loss {shape} det {det} cx")
    _within(loss[0], ls.loss, tol_loss, f"cx_loss {shape} det {det} loss")


def _bwd_tol(bw, p):
    """dcos bound of cx_bwd_kernel: T_i and M_i are workgroup reductions inside an element-wise expression"""
    lb = plan_block_row(p)
    tol_t = _red(lb, bw.t_mag)
    tol_e = _elem(bw.e_mag) + bw.cx.abs() * tol_t[..., None] + FMIN32  # cx_ij reaches the fp32 denormals, and e with it
    tol_m = (tol_e * bw.d.abs()).sum(2) + _red(lb, bw.m_mag)
    tol = _elem(bw.dcos_mag) + tol_e / (abs(H) * bw.den[..., None]) + FMIN32
    return tol.scatter_add(2, bw.idx, (tol_m / (abs(H) * bw.den * bw.den))[..., None])


@pytest.mark.parametrize("shape", CX, ids=_ids)
def test_cx_bwd(dev, FF, lib, shape):
    """operands: the float64 chain's tensors rounded to fp32 and its selections; gscale = 1.7, scale = 0.7.  Where P > 256 some rows'
    arg-min lies at 256 or beyond: thread 0 then corrects an entry of dcos that another thread wrote before the barrier"""
    n, p, c = shape
    ch = _cx_case(shape)[2]
    cx32, dmin32, cos32, cxn32 = ch.rows.cx.float(), ch.rows.dmin.float(), ch.cos.float(), ch.loss.cx.float()
    amin, carg = ch.rows.argmin.int(), ch.cols.colarg.int()
    if p > 256:
        assert int((amin >= 256).sum()) > 0
    bw = R.cx_bwd(cx32.double(), dmin32.double(), amin.long(), cos32.double(), carg.long(), cxn32.double(), GSCALE, H, SCALE)
    bw.cx, bw.idx = cx32.double(), amin.long()[..., None]
    dcos = _nan((n, p, p), dev)
    gs = torch.tensor([GSCALE], device=dev)
    lib.cx_bwd_f32(_up(cx32, dev), _up(dmin32, dev), _up(amin, dev), None, _up(cos32, dev), _up(carg, dev), _up(cxn32, dev),
                   _vp(gs), _vp(dcos), n, p, H, SCALE, FF._st())
    _within(dcos, bw.dcos, _bwd_tol(bw, p), f"cx_bwd {shape}")


@pytest.mark.parametrize("shape", CX, ids=_ids)
def test_contextual_loss_end_to_end(dev, FF, lib, shape):
    """FF.contextual_loss (reproducible mode) = the same launches made here by hand, bit for bit, loss and x.grad -- every link of which
    the tests above hold to float64.  In situ: the cosine matrix (normalise + GEMM) against float64 on the kernel's own mu, with the
    GEMM's bound of test_gpu_kernels.py::test_bf16x6_product_accuracy (1e-6 sum |a| |b|) next to the normalisations'; the kernels'
    selections against the float64 chain's under the gap bars; cx_ij, colmax and the loss against float64 ON the kernel's cosines"""
    n, p, c = shape
    x, y, ch = _cx_case(shape)
    rows, st = n * p, FF._st()
    what = f"contextual_loss {shape}"
    with FF.deterministic(True):
        xd = x.to(dev).requires_grad_(True)
        loss = FF.contextual_loss(xd, y.to(dev), H, SCALE)
        (loss * GSCALE).backward()
        x0, y0 = x.to(dev), y.to(dev)
        mu = torch.zeros(c, device=dev)
        lib.cx_channel_mean_f32(_vp(y0), _vp(mu), rows, c, st)
        xn, yn, xi, yi = torch.empty_like(x0), torch.empty_like(y0), _nan((rows,), dev), _nan((rows,), dev)
        lib.cx_normalise_f32(_vp(x0), _vp(mu), _vp(xn), _vp(xi), rows, c, st)
        lib.cx_normalise_f32(_vp(y0), _vp(mu), _vp(yn), _vp(yi), rows, c, st)
        cosm = _nan((n, p, p), dev)
        FF.gemm_raw(_vp(xn), _vp(yn), _vp(cosm), p, p, c, (c, 1), (1, c), (p, 1), n, (p * c, p * c, p * p))
        cx, dmin, amin, rsum = _run_cx_rows(dev, FF, lib, cosm)
        cmax, carg = _nan((n, p), dev), torch.full((n, p), -1, device=dev, dtype=torch.int32)
        lib.cx_cols_f32(_vp(cx), _vp(cmax), _vp(carg), n, p, st)
        cxn, l2 = _nan((n,), dev), torch.zeros(1, device=dev)
        lib.cx_loss_f32(_vp(cmax), _vp(cxn), _vp(l2), n, p, SCALE, st)
        dcos, gs = _nan((n, p, p), dev), torch.tensor([GSCALE], device=dev)
        lib.cx_bwd_f32(_vp(cx), _vp(dmin), _vp(amin), _vp(rsum), _vp(cosm), _vp(carg), _vp(cxn), _vp(gs), _vp(dcos), n, p, H, SCALE, st)
        gxn, gx = _nan((n, p, c), dev), _nan((n, p, c), dev)
        FF.gemm_raw(_vp(dcos), _vp(yn), _vp(gxn), p, c, p, (p, 1), (c, 1), (c, 1), n, (p * p, p * c, p * c))
        lib.cx_normalise_bwd_f32(_vp(gxn), _vp(xn), _vp(xi), _vp(gx), rows, c, st)
    assert torch.equal(loss.detach().reshape(1), l2), f"{what}: loss {float(loss)!r} != the hand-made chain's {float(l2)!r}"
    assert torch.equal(xd.grad, gx), what + ": x.grad differs from the hand-made chain's"
    # the cosine matrix in situ
    xr, yr = (R.cx_normalise(t.double().reshape(rows, c), _d(mu)) for t in (x, y))
    xr3, yr3 = xr.xn.reshape(n, p, c), yr.xn.reshape(n, p, c)
    _within(cosm, xr3 @ yr3.transpose(1, 2), (1e-6 + 2 * _norm_factor(c)) * (xr3.abs() @ yr3.abs().transpose(1, 2)), what + " cos")
    # selections against the chain on the exact inputs
    _check_argmin(amin, ch.rows, [], what)
    ccmp = ch.cols.relgap > R.COL_GAP_BAR
    assert float((~ccmp).double().mean()) <= R.EXCLUDED_MAX
    assert torch.equal(carg.cpu().long()[ccmp], ch.cols.colarg[ccmp]), what + ": colarg differs on comparable columns"
    # rows -> cols -> loss on the kernel's cosines
    r = R.cx_rows(_d(cosm), H)
    _, _, tol_cx = _rows_tols(r, p)
    _within(cx, r.cx, tol_cx, what + " cx_ij")
    cols = R.cx_cols(r.cx)
    dcm = tol_cx.max(1).values  # |max_i a_i - max_i b_i| <= max_i |a_i - b_i|
    _within(cmax, cols.colmax, dcm, what + " colmax")
    ls = R.cx_loss(cols.colmax, SCALE)
    _within(l2[0], ls.loss, _loss_tols(ls, n, p, SCALE, dcm)[1], what + " loss")


# ---- l2norm_rows -------------------------------------------------------------------------------------------------------------------
L2_SHAPES = [(5, 7), (9, 64), (6, 96), (3, 512), (1030, 130)]


def _l2_inputs(rows, c, eps):
    x, g = _randn(rows, c, seed=rows * 1000 + c), _randn(rows, c, seed=rows * 1000 + c + 1)
    if eps > 0:
        x[rows // 2] = 0  # one all-zero row: y = 0, s = 1 / eps, gradient s g
    return x, g


@pytest.mark.parametrize("eps", [0.0, 1e-10])
@pytest.mark.parametrize("rows,c", L2_SHAPES)
def test_l2norm_rows(dev, FF, lib, rows, c, eps):
    e32 = R.f32(eps)
    x, g = _l2_inputs(rows, c, eps)
    what = f"l2norm_rows {(rows, c)} eps {eps}"
    ref = R.l2norm_rows(x.double(), e32)
    y, inv = _nan((rows, c), dev), _nan((rows,), dev)
    lib.l2norm_rows_f32(_up(x, dev), _vp(y), _vp(inv), rows, c, e32, FF._st())
    k = _norm_factor(c)
    _within(inv, ref.inv, k * ref.inv, what + " inv")
    _within(y, ref.y, k * ref.y.abs(), what + " y")
    # backward on operands built here: y, inv of the reference rounded to fp32
    y32, inv32 = ref.y.float(), ref.inv.float()
    bw = R.l2norm_rows_bwd(g.double(), y32.double(), inv32.double(), e32)
    if eps > 0:
        z = rows // 2
        assert bool(bw.zero[z]) and int(bw.zero.sum()) == 1 and torch.equal(bw.gx[z], inv32.double()[z] * g.double()[z])
    gx = _nan((rows, c), dev)
    lib.l2norm_rows_bwd_f32(_up(g, dev), _up(y32, dev), _up(inv32, dev), _vp(gx), rows, c, e32, FF._st())
    # k = dot (n + eps) / n: the row reduction, then n = 1 / s - eps (two roundings of n + eps) inside the element-wise 8 u32
    tol_k = ((bw.n + e32) / bw.n).abs() * _red(plan_wave_row(c), bw.dot_mag) + _elem(bw.k.abs())
    _within(gx, bw.gx, _elem(bw.gx_mag) + inv32.double()[:, None] * y32.double().abs() * tol_k[:, None], what + " gx")


def test_l2norm_rows_autograd(dev, FF, lib):
    """FF.l2norm_rows: forward and backward are the two launches above, bit for bit (neither kernel has an atomic)"""
    rows, c, eps = 6, 96, 1e-10
    x, g = _l2_inputs(rows, c, eps)
    xd = x.to(dev).requires_grad_(True)
    y = FF.l2norm_rows(xd, eps)
    y.backward(g.to(dev))
    y2, inv, gx = _nan((rows, c), dev), _nan((rows,), dev), _nan((rows, c), dev)
    lib.l2norm_rows_f32(_up(x, dev), _vp(y2), _vp(inv), rows, c, eps, FF._st())
    lib.l2norm_rows_bwd_f32(_up(g, dev), _vp(y2), _vp(inv), _vp(gx), rows, c, eps, FF._st())
    assert torch.equal(y.detach(), y2) and torch.equal(xd.grad, gx)
    assert torch.equal(xd.grad[rows // 2], inv[rows // 2] * g.to(dev)[rows // 2])  # the zero row: s g


# ---- lpips_layer -------------------------------------------------------------------------------------------------------------------
LPIPS_SHAPES = [(35, 64), (1000, 192), (7, 5)]


def _lpips_inputs(pixels, c):
    s = pixels * 100 + c
    return _randn(pixels, c, seed=s), _randn(pixels, c, seed=s + 1), _randn(c, seed=s + 2)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("pixels,c", LPIPS_SHAPES)
def test_lpips_layer_forward(dev, FF, lib, pixels, c, det):
    fx, fy, w = _lpips_inputs(pixels, c)
    scale = R.f32(1.0 / pixels)
    ref = R.lpips_layer(fx.double(), fy.double(), w.double(), scale)
    out = torch.zeros(1, device=dev)
    with FF.deterministic(det):
        lib.lpips_layer_f32(_up(fx, dev), _up(fy, dev), _up(w, dev), _vp(out), pixels, c, scale, FF._st())
    _within(out[0], ref.out, _red(plan_lpips(pixels * c, det)[1], ref.out_mag), f"lpips_layer {(pixels, c)} det {det}")


@pytest.mark.parametrize("form", ["gfx", "gfy", "both"])
@pytest.mark.parametrize("pixels,c", LPIPS_SHAPES)
def test_lpips_layer_backward(dev, FF, lib, pixels, c, form):
    fx, fy, w = _lpips_inputs(pixels, c)
    scale, gout = R.f32(1.0 / pixels), R.f32(-1.3)
    ref = R.lpips_layer(fx.double(), fy.double(), w.double(), scale, gout)
    gfx = _nan((pixels, c), dev) if form != "gfy" else None
    gfy = _nan((pixels, c), dev) if form != "gfx" else None
    lib.lpips_layer_bwd_f32(_up(fx, dev), _up(fy, dev), _up(w, dev), _up(torch.tensor([gout]), dev), _vp(gfx), _vp(gfy),
                            pixels, c, scale, FF._st())
    if gfx is not None:
        _within(gfx, ref.gfx, _elem(ref.g_mag), f"lpips_layer_bwd {(pixels, c)} {form} gfx")
    if gfy is not None:
        _within(gfy, ref.gfy, _elem(ref.g_mag), f"lpips_layer_bwd {(pixels, c)} {form} gfy")
    if form == "both":
        assert torch.equal(gfy, -gfx)


# ---- reduce_loss, dot, axpy ------------------------------------------------------------------------------------------------------
def _ab(n):
    a, b = _randn(n, seed=n), _randn(n, seed=n + 1)
    a[::7] = b[::7]  # elements with a == b: |a - b| has gradient exactly 0 there
    return a, b


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("n,det", [(1, False), (1938, False), (5000, False), (1, True), (1938, True), (5000, True), (2 * 16384 + 37, True)])
def test_reduce_loss(dev, FF, lib, n, det, kind):
    a, b = _ab(n)
    c0, scale, gs = R.f32(0.9), R.f32(1.0 / n), R.f32(1.3)
    ref = R.reduce_loss(kind, a.double(), b.double(), c0, scale, gs)
    ad, bd = a.to(dev), (b.to(dev) if kind != 2 else None)
    out = torch.zeros(1, device=dev)
    with FF.deterministic(det):
        lib.reduce_loss_f32(kind, _vp(ad), _vp(bd), n, c0, scale, _vp(out), FF._st())
    what = f"reduce_loss kind {kind} n {n} det {det}"
    _within(out[0], ref.out, _red(plan_reduce_loss(n, det)[2], ref.out_mag), what)
    ga = _nan((n,), dev)
    lib.reduce_loss_bwd_f32(kind, _vp(ad), _vp(bd), n, c0, scale, _up(torch.tensor([gs]), dev), _vp(ga), FF._st())
    _within(ga, ref.ga, _elem(ref.ga_mag), what + " ga")
    if kind == 0:
        assert bool((ga[::7] == 0).all()) and int((ga == 0).sum()) == _cdiv(n, 7), what + ": sign(0) must be 0"


@pytest.mark.parametrize("n", [1, 5000])
def test_dot_and_axpy(dev, FF, lib, n):
    a, b = _ab(n)
    scale, s = R.f32(0.37), R.f32(-2.5)
    ad, bd = a.to(dev), b.to(dev)
    for det in (False, True):
        out = torch.zeros(1, device=dev)
        with FF.deterministic(det):
            lib.dot_f32(_vp(ad), _vp(bd), n, scale, _vp(out), FF._st())
        ref = R.dot(a.double(), b.double(), scale)
        # fp64 inside: per workgroup the fp32 store of its share, then the fp32 atomics
        _within(out[0], ref.out, _red(plan_dot(n, det)[1], ref.out_mag) + n * U64 * ref.out_mag, f"dot n {n} det {det}")
    sd = torch.tensor([s], device=dev)
    for bb in (None, bd):
        y = _nan((n,), dev)
        lib.axpy_dev_f32(_vp(ad), _vp(sd), _vp(bb), _vp(y), n, FF._st())
        ref = R.axpy(a.double(), s, None if bb is None else b.double())
        _within(y, ref.y, _elem(ref.y_mag), f"axpy n {n} b {'given' if bb is not None else 'null'}")


# ---- weight prepare and gradient ------------------------------------------------------------------------------------------------
# (shape [rows, C, kh, kw], spectral norm, piece images, power iterations)
W_TABLE = [((64, 64, 1, 1), True, False, 1), ((40, 24, 1, 1), False, False, 1), ((64, 32, 3, 3), True, True, 1), ((48, 40, 3, 3), True, False, 1),
           ((32, 16, 4, 4), True, True, 1), ((8, 3, 7, 7), False, False, 1), ((300, 8, 3, 3), True, False, 1), ((24, 16, 3, 3), True, False, 3),
           ((5, 3, 17, 17), True, False, 1), ((5, 3, 17, 17), False, False, 1)]
W_FILL = [(4, 3, 3, 3), (8, 8, 1, 1), (6, 5, 2, 2), (16, 8, 3, 3), (3, 2, 1, 1)]


def _w_specs():
    """35 entries in one call: 12 fillers, the first eight table rows, 13 fillers, the two 17 x 17 weights -- the second launch chunk
    (entries 32 - 34) holds two spectrally normalised entries, whose dots live at scratch + 32 and + 33, and so do entries 0 and 1 of
    the first chunk: dots summed at the wrong offset meet dots that are not zero.  Fillers 0, 1, 4, 5, 8, ... (13 of 25) have
    spectral norm"""
    fill = [(W_FILL[i % 5], i % 4 < 2, True, 1) for i in range(25)]
    specs = fill[:12] + W_TABLE[:8] + fill[12:] + W_TABLE[8:]
    assert len(specs) == 35 and all(specs[i][1] for i in (0, 1, 32, 33))
    return specs


def _unit(n, seed):
    v = _randn(n, seed=seed)
    return v / v.norm()


def _w_operands(specs, dev):
    ops = []
    for i, (shape, sn, w3, iters) in enumerate(specs):
        rows, c, kh, kw = shape
        w = _randn(*shape, seed=500 + i) / math.sqrt(c * kh * kw)
        u, v = (_unit(rows, 600 + i), _unit(c * kh * kw, 700 + i)) if sn else (None, None)
        ops.append((w, u, v))
    return ops


def _pieces_to_float(p3, taps, cred, nout):
    """[3][taps][cred / 8][nout][8] bf16 piece images -> three tensors [taps][cred][nout] (the layout of test_gpu_kernels.py)"""
    return [p3.view(3, taps, cred // 8, nout, 8)[i].permute(0, 1, 3, 2).reshape(taps, cred, nout).double() for i in range(3)]


def _sn_tols(it, w64, rows, width):
    """first-order bounds of one power iteration (weights.hip wp_wtu_kernel: one thread per column, `rows` sequential adds;
    wp_vnorm_kernel / wp_unorm_kernel: a workgroup row; wp_wv_kernel: a wave row) -> (dv, du, dsigma)"""
    def norm_tol(vec, dvec, length):
        n2 = (vec * vec).sum()
        d2 = (2 * vec.abs() * dvec).sum() + _red(plan_block_row(length), n2)
        n = torch.sqrt(n2)
        return torch.maximum(torch.sqrt(n2 + d2) - n, n - torch.sqrt((n2 - d2).clamp_min(0))) + 2 * U32 * n

    aw = w64.abs()
    dv_raw = _red(rows, it.v_raw_mag)
    dv = dv_raw / it.nv + it.v.abs() * norm_tol(it.v_raw, dv_raw, width) / it.nv + 4 * U32 * it.v.abs()
    dt = aw @ dv + _red(plan_wave_row(width), it.t_mag)
    du = dt / it.nt + it.u.abs() * norm_tol(it.t, dt, rows) / it.nt + 4 * U32 * it.u.abs()
    dsig = (it.t.abs() * du + it.u.abs() * dt).sum() + _red(plan_block_row(rows), it.sigma_mag)
    return dv, du, dsig


def _check_prepared(what, spec, w, u0, u1, v1, sigma, pw):
    """one entry after fmi_weight_prepare_f32: u', v', sigma, both packs, the piece images.  All tensors on the CPU"""
    (rows, c, kh, kw), sn, want3, _ = spec
    taps, width = kh * kw, c * kh * kw
    w64 = w.double().reshape(rows, width)
    wf, wt = _d(pw.wf), _d(pw.wt)
    assert wf.shape == (taps, c, rows) and wt.shape == (taps, rows, c)
    assert torch.equal(wf.permute(2, 1, 0), wt.permute(1, 2, 0)), what + ": wf and wt hold different values"
    if not sn:
        assert float(sigma) == 1.0 and torch.equal(wf, R.pack_wf(w64, rows, c, taps)), what + ": a plain pack must be a permutation of w"
    else:
        it = R.spectral_iteration(w64, u0.double())
        dv, du, dsig = _sn_tols(it, w64, rows, width)
        _within(v1, it.v, dv, what + " v'")
        _within(u1, it.u, du, what + " u'")
        _within(sigma, it.sigma, dsig, what + " sigma")
        weff = w64 / it.sigma
        tol = _elem(weff.abs()) + weff.abs() * dsig / it.sigma.abs()
        _within(pw.wf, R.pack_wf(weff, rows, c, taps), R.pack_wf(tol, rows, c, taps), what + " wf")
        _within(pw.wt, R.pack_wt(weff, rows, c, taps), R.pack_wt(tol, rows, c, taps), what + " wt")
    wf3, wt3 = pw.w3
    assert (wf3 is not None) == (want3 and taps <= 36 and c % 16 == 0) and (wt3 is not None) == (want3 and taps <= 36 and rows % 16 == 0), what
    for p3, pack, cred, nout in ((wf3, wf, c, rows), (wt3, wt, rows, c)):
        if p3 is not None:
            x0, x1, x2 = _pieces_to_float(p3.cpu(), taps, cred, nout)
            assert torch.equal(x0 + x1 + x2, pack), what + ": the three pieces do not add up to the fp32 pack exactly"
            assert bool((x1.abs() <= 2.0 ** -8 * pack.abs()).all()) and bool((x2.abs() <= 2.0 ** -16 * pack.abs()).all()), what + ": piece sizes"


@pytest.fixture(scope="module")
def prepared(dev, FF):
    """ONE fmi_weight_prepare_f32 call on the 35 entries, and the gradient of random pack gradients in both modes"""
    specs = _w_specs()
    ops = _w_operands(specs, dev)
    ws = [w.to(dev).requires_grad_(True) for w, _, _ in ops]
    us = [None if u is None else u.to(dev) for _, u, _ in ops]
    vs = [None if v is None else v.to(dev) for _, _, v in ops]
    pws = FF.prepare_weights([(w, u, v, s[2], s[3]) for w, u, v, s in zip(ws, us, vs, specs)])
    sig = pws[0].wf.grad_fn.sig.cpu()  # the autograd node is the ctx _WeightPrepare.forward stored sigma on
    u1 = [None if u is None else u.cpu().clone() for u in us]
    v1 = [None if v is None else v.cpu().clone() for v in vs]
    gwf = [_randn(*pw.wf.shape, seed=800 + i) for i, pw in enumerate(pws)]
    grads = {}
    for det in (False, True):
        for w in ws:
            w.grad = None
        with FF.deterministic(det):
            torch.autograd.backward([pw.wf for pw in pws], [g.to(dev) for g in gwf], retain_graph=True)
        grads[det] = [w.grad.cpu().clone() for w in ws]
    return dict(specs=specs, ops=ops, pws=pws, sig=sig, u1=u1, v1=v1, gwf=gwf, grads=grads)


def test_weight_prepare(prepared):
    """u', v', sigma, wf, wt and the piece images of every one of the 35 entries (iters = 1 here; the three-iteration entry below)"""
    p = prepared
    for i, spec in enumerate(p["specs"]):
        if spec[3] == 1:
            w, u0, _ = p["ops"][i]
            _check_prepared(f"entry {i} {spec}", spec, w, u0, p["u1"][i], p["v1"][i], p["sig"][i], p["pws"][i])


def test_weight_prepare_three_iterations(dev, FF, prepared):
    """the iters = 3 entry of the big call = three one-iteration calls on copies of its operands, bit for bit (no kernel of the
    sequence has an atomic), and each of those three steps against float64 from the state the previous one left"""
    p = prepared
    i = next(j for j, s in enumerate(p["specs"]) if s[3] == 3)
    spec = p["specs"][i]
    w, u0, v0 = p["ops"][i]
    wd, ud, vd = w.to(dev).requires_grad_(True), u0.to(dev), v0.to(dev)
    for step in range(3):
        before = ud.cpu().clone()
        (pw,) = FF.prepare_weights([(wd, ud, vd, False, 1)])
        sig = pw.wf.grad_fn.sig.cpu()
        _check_prepared(f"entry {i} iteration {step}", (spec[0], True, False, 1), w, before, ud.cpu(), vd.cpu(), sig[0], pw)
    assert torch.equal(ud.cpu(), p["u1"][i]) and torch.equal(vd.cpu(), p["v1"][i]), "iters = 3: u / v differ from three single iterations"
    assert torch.equal(sig[0], p["sig"][i]) and torch.equal(pw.wf.detach().cpu(), p["pws"][i].wf.detach().cpu())


@pytest.mark.parametrize("det", [False, True])
def test_weight_grad(prepared, det):
    """dW of every entry against spectral_grad on the u', v', sigma the preparation left (read live by the kernel)"""
    p = prepared
    for i, spec in enumerate(p["specs"]):
        (rows, c, kh, kw), sn = spec[0], spec[1]
        taps, width = kh * kw, c * kh * kw
        what = f"weight_grad det {det} entry {i} {spec}"
        dweff = R.unpack_wf(p["gwf"][i].double(), rows, c, taps)
        got = p["grads"][det][i].reshape(rows, width)
        if not sn:
            assert torch.equal(got.double(), dweff), what + ": a plain pack's gradient must be a permutation of dwf"
            continue
        sg = R.spectral_grad(p["ops"][i][0].double().reshape(rows, width), p["u1"][i].double(), p["v1"][i].double(), p["sig"][i].double(), dweff)
        ddot = _red(plan_wg_dot(rows * width, det)[1], sg.dot_mag)
        _within(got, sg.dw, _elem(sg.dw_mag) + sg.uv.abs() * ddot / (p["sig"][i].double() ** 2), what)


# ---- Adam --------------------------------------------------------------------------------------------------------------------------
ADAM_NS = [1, 255, 4096, 4097, 3 * 4096 + 5]


@pytest.mark.parametrize("form", ["host_step", "device_step"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_step(dev, FF, wd, form):
    """70 tensors (two launch chunks of 64) laid side by side in one buffer, so a write past a tensor's end lands in its neighbour;
    steps 1, 2 and 1000, each from the kernel's own state.  Moments start non-zero"""
    sizes = [ADAM_NS[i % 5] for i in range(70)]
    total = sum(sizes)
    offs = [sum(sizes[:i]) for i in range(70)]
    lr, b1, b2, eps, wd32 = R.f32(1e-2), R.f32(0.9), R.f32(0.999), R.f32(1e-8), R.f32(wd)
    p = _randn(total, seed=41).to(dev)
    m = (_randn(total, seed=42) * 0.1).to(dev)
    v = (_randn(total, seed=43) ** 2 * 0.01).to(dev)
    views = lambda t: [t[o:o + s] for o, s in zip(offs, sizes)]  # noqa: E731
    counter = torch.zeros(1, device=dev, dtype=torch.int32)
    for step in (1, 2, 1000):
        g = _randn(total, seed=50 + step).to(dev)
        p0, m0, v0 = _d(p), _d(m), _d(v)
        if form == "host_step":
            FF.adam_step(views(p), views(g), views(m), views(v), step, lr, b1, b2, eps, wd32)
        else:
            counter.fill_(step - 1)
            FF.adam_step(views(p), views(g), views(m), views(v), counter, lr, b1, b2, eps, wd32)
            assert int(counter) == step
        what = f"adam {form} wd {wd} step {step}"
        ref = R.adam_step(p0, _d(g), m0, v0, step, lr, b1, b2, eps, wd32, mv=(_d(m), _d(v)))
        _within(m, ref.m, _elem(ref.m_mag), what + " m")
        _within(v, ref.v, _elem(ref.v_mag), what + " v")
        _within(p, ref.p, _elem(ref.p_mag), what + " p")  # on the kernel's own m, v (just checked)


# ---- Ranger ------------------------------------------------------------------------------------------------------------------------
RANGER_SHAPES = [(6, 300, 1, 1), (5000, 3), (9000,), (4, 4, 3, 3)] + [((7,), (33, 5), (4, 3, 3, 3), (16,), (2, 9))[i % 5] for i in range(31)]


@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_ranger_step(dev, FF, lib, wd):
    """35 tensors (two launch chunks of 32), 13 steps (unrectified and rectified, two Lookahead syncs).  Each step runs twice from the
    same state: Ranger.step, and the raw entry on copies with a row-mean scratch of the test's own; the two must agree bit for bit,
    and the raw run's row means, m, v, p and slow are held to float64 from the state before the step"""
    from face_mask_inpaint_amd import _lib
    from face_mask_inpaint_amd.modules.psp.ranger import Ranger

    assert len(RANGER_SHAPES) == 35
    cfg = dict(lr=1e-2, alpha=0.5, k=6, betas=(0.95, 0.999), eps=1e-5, weight_decay=wd)
    lr, b1, b2, eps, wd32, alpha = (R.f32(t) for t in (cfg["lr"], 0.95, 0.999, cfg["eps"], wd, cfg["alpha"]))
    ps = [torch.nn.Parameter(_randn(*s, seed=900 + i).to(dev)) for i, s in enumerate(RANGER_SHAPES)]
    opt = Ranger(ps, **cfg)
    gc = [len(s) > 1 for s in RANGER_SHAPES]
    cols = [math.prod(s[1:]) if len(s) > 1 else s[0] for s in RANGER_SHAPES]
    seen = set()
    for step in range(1, 14):
        gs = [_randn(*s, seed=step * 100 + i).to(dev) + 0.3 for i, s in enumerate(RANGER_SHAPES)]  # + 0.3: row means that matter
        if step == 1:
            prev = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p), p.detach().clone()) for p in ps]
        else:
            prev = [tuple(t.clone() for t in (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], opt.state[p]["slow_buffer"])) for p in ps]
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()
        # the raw entry on copies of the state before the step
        rect, step_size = opt._rectification(step, 0.95, 0.999)
        look = step % cfg["k"] == 0
        seen.add((rect, look))
        raw = [tuple(t.clone() for t in st) for st in prev]
        means = [_nan((s[0],), dev) if c else None for s, c in zip(RANGER_SHAPES, gc)]
        entries = (_lib.RangerEntry * 35)()
        for e, (p_, m_, v_, s_), g, mean, s, nc in zip(entries, raw, gs, means, RANGER_SHAPES, cols):
            e.p, e.g, e.m, e.v, e.slow = p_.data_ptr(), g.data_ptr(), m_.data_ptr(), v_.data_ptr(), s_.data_ptr()
            e.n, e.cols, e.row_mean = p_.numel(), nc, (mean.data_ptr() if mean is not None else None)
        lib.ranger_step_f32(entries, 35, cfg["lr"], 0.95, 0.999, cfg["eps"], wd, step_size, 1 if rect else 0, cfg["alpha"], 1 if look else 0, FF._st())
        for i, (p, (p_, m_, v_, s_)) in enumerate(zip(ps, raw)):
            what = f"ranger wd {wd} step {step} tensor {i} {RANGER_SHAPES[i]}"
            st = opt.state[p]
            assert torch.equal(p.detach(), p_) and torch.equal(st["exp_avg"], m_) and torch.equal(st["exp_avg_sq"], v_) and \
                torch.equal(st["slow_buffer"], s_), what + ": Ranger.step and the raw entry disagree"
            g64 = _d(gs[i]).reshape(-1, cols[i])
            mean = None
            if gc[i]:
                rm = R.row_mean(g64, cols[i])
                _within(means[i], rm.mean, 2 * U32 * rm.mean.abs() + (cols[i] + 8) * U64 * rm.mean_mag, what + " row mean")  # fp64 sum, fp32 store
                mean = _d(means[i])
            sh = (-1, cols[i])
            p0, m0, v0, s0 = (_d(t).reshape(sh) for t in prev[i])
            ref = R.ranger_step(p0, g64, m0, v0, s0, mean, lr, b1, b2, eps, wd32, R.f32(step_size), rect, alpha, look,
                                mv=(_d(m_).reshape(sh), _d(v_).reshape(sh)))
            _within(m_, ref.m, _elem(ref.m_mag), what + " m")
            _within(v_, ref.v, _elem(ref.v_mag), what + " v")
            _within(p_, ref.p, _elem(ref.p_mag), what + " p")
            _within(s_, ref.slow, _elem(ref.slow_mag), what + " slow")
            if not look:
                assert torch.equal(s_, prev[i][3]), what + ": slow moved outside a Lookahead step"
    assert {r for r, _ in seen} == {False, True} and {l for _, l in seen} == {False, True}  # both branches; Lookahead at steps 6 and 12
