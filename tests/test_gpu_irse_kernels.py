"""GPU: the bandwidth kernels between the convolutions of the IR-SE50 body (csrc/norm.hip, chan.hip, sg2_bf16.hip, pool.hip),
one by one, against the float64 references of tests/irse_reference.py.

The references get float64 copies of the very operands a kernel read: for bf16 the rounded values; for the BatchNorm apply and backward
kernels the (mean, rstd) the statistics kernel produced (those are checked against float64 on their own first) and the activation mask
the forward kernel decided (y_kernel > 0; that mask may differ from the float64 one only at rounding distance from the kink, which is
asserted -- the condition test_host_irse_reference.py::test_mask_condition establishes for the reference side).

Tolerances are derived, none is fitted.  u32 = 2^-24, u16 = 2^-8 (bf16 round to nearest even), mag = the reference's magnitude (the
same expression with every term replaced by its absolute value):
  fp32 element-wise   8 u32 mag
  bf16 element-wise   u16 |ref| + 8 u32 mag
  fp32 reduction      (L + 8) u32 sum|term|, L = the longest chain of fp32 additions the selected launcher produces for the shape (one
                      thread's run + the lanes combined through LDS + the parts the finishing launch or the atomics add); the plan_*
                      helpers restate each launcher's block arithmetic and name the source lines
  statistics          norm.hip adds in fp32 inside one thread's run only and in fp64 beyond: sum x, sum x^2 to (Lt + 2) u32 sum|term|;
                      propagated to mean (/ count, + 2 u32 |mean| for the fp32 store), to var = E[x^2] - mean^2 and through the monotone
                      1 / sqrt(var + eps) to rstd (+ 2 u32 rstd)
  BatchNorm gx        8 u32 mag (u16 |ref| + ... in bf16) + rstd |gamma| (d1 + |xhat| d2), d1 / d2 = the reduction bound of the kernel's
                      own mean g' and mean g' xhat ((Lt + 8) u32 mean|term|): gx is an element-wise expression OF two reductions
Bit-exact (torch.equal): subsample both ways, gres of scale_channels_add, every pass-through output, num_batches_tracked.

Every cross the cases are built from is run in full (BatchNorm: every shape x groups x slope x pass-through form), except the cells of
OMITTED below: three cells of 55 - 82 million elements, whose float64 host reference alone (six to ten temporaries of 0.4 - 0.7 GB)
takes longer than the few seconds a case may take.  Each is listed there with its size; its channel count and its row count both run
at the neighbouring cells."""
import ctypes
import functools
import itertools
import math

import pytest
import torch

import irse_reference as R

pytestmark = pytest.mark.gpu

U32, U16, U64 = 2.0 ** -24, 2.0 ** -8, 2.0 ** -53
F64, BF16 = torch.float64, torch.bfloat16
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))  # the eps the library sees (a float argument)
# (test, cell) -> why it does not run.  Elements are per tensor; a case holds three to four such tensors on the device and the host, and
# the float64 reference makes six to ten temporaries of 8 bytes per element.
OMITTED = {
    ("se_gate_one_pass", (1024, 9000, 3)): "27.6 M elements (110 MB fp32 per tensor, 221 MB per float64 temporary); N = 1 runs",
    ("se_gate_bf16", (2048, 9000, 3)): "55.3 M elements (111 MB bf16 per tensor, 442 MB per float64 temporary); N = 1 runs",
    ("prelu_bf16", (2048, 40000)): "81.9 M elements (164 MB bf16 per tensor, 655 MB per float64 temporary); C = 2048 runs at 3 and 480 "
                                   "rows, 40000 rows at C = 8 and 64",
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
    err = (got - ref).abs()
    ok = err <= tol  # False for NaN: an element the kernel never wrote
    if not bool(ok.all()):
        bad = ~ok
        ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.full_like(err, float("inf")))[bad]
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {ok.numel()} elements beyond the bound; worst err / bound = "
                             f"{float(ratio.nan_to_num(float('inf')).max()):.3g}; first at flat index {i}: got {float(got.reshape(-1)[i])!r}, "
                             f"ref {float(ref.reshape(-1)[i])!r}, bound {float(tol.reshape(-1)[i]):.3g}")


def _elem_tol(ref, mag, dtype):
    return 8 * U32 * mag + (U16 * ref.abs() if dtype == BF16 else 0)


def _red_tol(L, mag):
    return (L + 8) * U32 * mag


def _cdiv(a, b):
    return -(-a // b)


def _split(total, blocks):
    """rpb = ceil(total / blocks); blocks = ceil(total / rpb): the re-balancing every row-block launcher here ends with"""
    rpb = _cdiv(total, blocks)
    return rpb, _cdiv(total, rpb)


# ---- the launchers' block arithmetic, restated -----------------------------------------------------------------------------------
def _rows_per_block(n, hw, cap, r0):
    """norm.hip rows_per_block()"""
    r = r0
    while n * _cdiv(hw, r) > cap and r < (1 << 20):
        r *= 2
    return r


def plan_norm_reduce(n, hw, c, ws=True, det=False):
    """norm.hip launch_in_reduce(): (rows per block, blocks per sample, Lt = one thread's fp32 run; everything beyond is fp64).
    ws: the partials workspace of FF._norm_ws (max(1024, n) c 2 doubles -> cap 1024)"""
    if ws:
        ws_doubles = max(1024, n) * c * 2  # functional._norm_ws
        rpb = _rows_per_block(n, hw, min(ws_doubles // (c * 2), 1024), 64)  # launch_in_reduce: cap = ws_doubles / (2 C), at most 1024
    else:
        rpb = hw if det else _rows_per_block(n, hw, 2048, 512)
    pl = 256 // (c // 4)  # pixel lanes of in_reduce_kernel
    return rpb, _cdiv(hw, rpb), _cdiv(min(rpb, hw), pl)


def plan_norm_apply(n, hw):
    """norm.hip apply_impl() / in_bwd_apply_impl(): rows per block"""
    return _rows_per_block(n, hw, 16384, 16)


def _sum_parts_chain(nparts):
    """sum_parts_kernel<T> (sum_parts.h): a lane walks ceil(nparts / 16) parts, 3 tree levels, 16 lanes"""
    return _cdiv(nparts, 16) + 3 + 16


def plan_prelu_bwd_f32(rows, c, det=False):
    """chan.hip fmi_prelu_bwd_f32() with FF.prelu's workspace of 1024 c floats: (path, blocks, L)"""
    c4 = c // 4
    if c % 4 == 0 and c4 <= 256 and c4 & (c4 - 1) == 0:
        rpb, blocks = _split(rows, min(_cdiv(rows, 64), 1024))
        rl = 256 // c4
        return "vec", blocks, _cdiv(rpb, rl) + (rl - 1) + _sum_parts_chain(blocks)
    rpb, blocks = _split(rows, 1 if det else min(_cdiv(rows, 128), 2048))
    return "scalar", blocks, _cdiv(rpb, 4) + 3 + blocks  # 4 row lanes, then one fp32 atomic per block and channel


def plan_prelu_bwd_bf16(rows, c):
    """chan.hip fmi_prelu_bwd_bf16() with FF.prelu's workspace of 512 c floats; sum_rows_f32_kernel adds the parts in one chain"""
    rpb, blocks = _split(rows, min(_cdiv(rows, 64), 512))
    rl = 256 // (c // 8)
    return blocks, _cdiv(rpb, rl) + rl + blocks


def _gs_finish_chain(nparts):
    """scale_channels_gs_finish_kernel (chan.hip): four accumulators and their tree"""
    return _cdiv(nparts, 4) + 3 + 2


def plan_scale_bwd_f32(n, p, c):
    """chan.hip fmi_scale_channels_bwd_f32() with FF._scale_channels_bwd's workspace of max(4096, n) c floats"""
    ws_floats = max(4096, n) * c  # functional._scale_channels_bwd
    cap = min(ws_floats // (n * c), _cdiv(4096, n))  # the launcher: what the workspace holds, at most ceil(4096 / N)
    rpb, blocks = _split(p, min(_cdiv(p, 64), cap))
    rl = 256 // (c // 4)
    return blocks, _cdiv(rpb, rl) + (rl - 1) + _gs_finish_chain(blocks)


def plan_scale_gs_f32(n, p, c, ws=True, det=False):
    """chan.hip fmi_scale_channels_gs_f32(); ws: FF's workspace of max(2048, n) c floats, otherwise fp32 atomics"""
    blocks = _cdiv(p, 128)
    ws_floats = max(2048, n) * c  # functional._ScaleChannels.backward
    cap = min(ws_floats // (n * c), _cdiv(2048, n)) if ws else 1024  # the launcher: what the workspace holds, at most ceil(2048 / N)
    blocks = min(blocks, cap)
    if det and not ws:
        blocks = 1
    rpb, blocks = _split(p, blocks)
    return blocks, _cdiv(rpb, 4) + 1 + 3 + (_gs_finish_chain(blocks) if ws else blocks)


def plan_scale_gs_bf16(n, p, c):
    """chan.hip fmi_scale_channels_gs_bf16() / sum_parts.h parts_for() with FF's workspace of max(2048, n) c floats"""
    ws_floats = max(2048, n) * c  # functional._ScaleChannels.backward
    b = min(_cdiv(p, 64), _cdiv(2048, n), ws_floats // (n * c))  # parts_for(): want, then what the workspace holds
    rpb, blocks = _split(p, b)
    rl = 256 // (c // 8)
    return blocks, _cdiv(rpb, rl) + (rl - 1) + _sum_parts_chain(blocks)


def plan_pool_f32(n, h, w, c, det=False):
    """pool.hip fmi_avgpool_f32() with k = H: (kernel, L).  The streaming kernel multiplies by 1 / HW (+1) before its atomics"""
    c4 = c // 4
    if h == w and h >= 8 and c % 4 == 0 and c4 <= 256 and c4 & (c4 - 1) == 0:
        hw = h * w
        blocks = _cdiv(hw, 128)
        if blocks * n > 2048:
            blocks = _cdiv(2048, n)
        if det:
            blocks = 1
        rpb, blocks = _split(hw, blocks)
        rl = 256 // c4
        return "stream", _cdiv(rpb, rl) + (rl - 1) + 1 + blocks
    return "window", h * h + 1


def plan_pool_bf16(n, p, c):
    """chan.hip fmi_global_avgpool_bf16() with FF's workspace of 64 n c floats: (parts, L)"""
    rpb, blocks = _split(p, min(_cdiv(p, 64), 64))
    rl = 256 // (c // 8)
    return blocks, _cdiv(rpb, rl) + rl + blocks + 1


def plan_bias_grad(rows, k):
    """conv.hip fmi_bias_grad_f32(), vector form (K / 4 a power of two): one run, the lanes, one atomic per block"""
    rpb, blocks = _split(rows, min(_cdiv(rows, 256), 256))
    rl = 256 // (k // 4)
    return _cdiv(rpb, rl) + (rl - 1) + blocks


def test_plans_reach_the_branches_the_cases_are_named_for():
    """a retune of a launcher fails here instead of silently moving a case onto another path"""
    assert plan_norm_reduce(1, 30, 12)[2] == 1 and 256 // 3 > 30                     # rows below the pixel lanes, CG = 3
    assert plan_norm_reduce(1, 252, 64)[:2] == (64, 4)                               # four blocks of 64, tail loops only (PL = 16)
    assert plan_norm_reduce(1, 2046, 64)[2] == 4                                     # 64 rows over 16 lanes: the 4-deep loop body
    assert 256 // (1024 // 4) == 1                                                   # CG = 256, one pixel lane
    assert plan_norm_reduce(1, 7232, 8)[1] == 113                                    # > 112 parts: 8-deep loop of sum_parts_kernel<double>
    assert plan_norm_reduce(2, 32896, 8)[0] == 128                                   # rows_per_block doubles in the reduction
    assert plan_norm_apply(1, 262656) == 32                                          # ... and in the apply launches
    assert plan_norm_reduce(1, 4480, 8, ws=False)[:2] == (512, 9)                    # several 512-row chunks of fp64 atomics
    assert plan_prelu_bwd_f32(7232, 64)[:2] == ("vec", 113)                          # 8-deep loop of sum_parts_kernel<float>, one group
    assert plan_scale_gs_bf16(3, 9000, 8)[0] == 141                                  # ... and with three groups (blockIdx.y)
    assert plan_prelu_bwd_f32(300, 132)[:2] == ("scalar", 3) and plan_prelu_bwd_f32(300, 12)[0] == "scalar"
    assert plan_prelu_bwd_bf16(40000, 8)[0] > 500                                    # sum_rows_f32_kernel walks ~512 parts
    assert plan_pool_f32(2, 16, 16, 64)[0] == "stream" and plan_pool_f32(3, 8, 8, 512)[0] == "stream"
    assert plan_pool_f32(2, 4, 4, 64)[0] == "window" and plan_pool_f32(2, 16, 16, 12)[0] == "window"
    assert plan_pool_bf16(2, 6400, 512)[0] == 64                                     # the 64-part cap binds


# ---- BatchNorm -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _bn_case(shape, groups, dtype):
    """inputs (CPU, never modified), their float64 copies and the float64 statistics, once per (shape, groups, dtype)"""
    x, gamma, beta, gy, gpass = R.bn_inputs(shape, groups, R.bn_seed(shape, groups), dtype)
    return (x, gamma, beta, gy, gpass), R.bn_stats(x.double(), EPS32, groups)


def _stat_bounds(st, lt):
    """the statistics bound of the module docstring: (d sum, d sumsq, d mean, d var, d rstd)"""
    d1, d2 = (lt + 2) * U32 * st.s1_mag, (lt + 2) * U32 * st.s2_mag
    e1, e2 = d1 / st.count, d2 / st.count
    dmean = e1 + 2 * U32 * st.mean.abs()
    dvar = e2 + 2 * st.mean.abs() * e1 + e1 * e1
    hi = 1 / torch.sqrt((st.var - dvar).clamp_min(0) + EPS32)
    lo = 1 / torch.sqrt(st.var + dvar + EPS32)
    drstd = torch.maximum(hi - st.rstd, st.rstd - lo) + 2 * U32 * st.rstd
    return d1, d2, dmean, dvar, drstd


def _check_mask(kmask, fw, what):
    bad = kmask != (fw.pre > 0)
    nbad = int(bad.sum())
    assert nbad <= 1e-4 * bad.numel(), f"{what}: the kernel's activation mask differs from float64 on {nbad} of {bad.numel()} elements"
    assert bool((fw.pre.abs()[bad] <= 2.0 ** -20 * fw.pre_mag[bad]).all()), f"{what}: mask differs away from the kink"


def _check_bn_forward(x64, gamma, beta, st, lt, y, stats, sums, slope, groups, dtype, what):
    """statistics against float64, then y against float64 ON the kernel's statistics and mask; returns (mean, rstd, mask) of the kernel"""
    d1, d2, dmean, _, drstd = _stat_bounds(st, lt)
    _within(sums[..., 0], st.s1, d1, what + " sum x")
    _within(sums[..., 1], st.s2, d2, what + " sum x^2")
    _within(stats[..., 0], st.mean, dmean, what + " mean")
    _within(stats[..., 1], st.rstd, drstd, what + " rstd")
    km, kr = _d(stats[..., 0]), _d(stats[..., 1])
    fw = R.bn_apply(x64, km, kr, gamma.double(), beta.double(), slope, groups)
    kmask = _d(y) > 0
    _check_mask(kmask, fw, what)
    y_ref = torch.where(kmask, fw.pre, slope * fw.pre)
    y_mag = torch.where(kmask, fw.pre_mag, abs(slope) * fw.pre_mag)
    _within(y, y_ref, _elem_tol(y_ref, y_mag, dtype), what + " y")
    return km, kr, kmask


def _check_bn_backward(x64, gy64, gadd64, gamma, beta, km, kr, kmask, lt, gx, dgamma, dbeta, slope, groups, dtype, what):
    bw = R.bn_backward(x64, gy64, km, kr, gamma.double(), beta.double(), slope, groups, kmask, gadd64)
    d1, d2 = _red_tol(lt, bw.m1_abs), _red_tol(lt, bw.m2_abs)  # the kernel's own mean g' and mean g' xhat
    inner = (bw.k_abs[:, None] * (d1[:, None] + R._grp(bw.xhat, groups).abs() * d2[:, None])).reshape(x64.shape)
    _within(gx, bw.gx, _elem_tol(bw.gx, bw.gx_mag, dtype) + inner, what + " gx")
    _within(dgamma, bw.dgamma, _red_tol(lt, bw.dgamma_mag), what + " dgamma")
    _within(dbeta, bw.dbeta, _red_tol(lt, bw.dbeta_mag), what + " dbeta")


SLOPES = (1.0, 0.0, 0.2)
PASS = ("off", "both", "pass_only")  # pass_only: a gradient on the pass-through output alone (the `g is None` branch)


def _bn_cases(shapes):
    return [(s, g, sl, pt) for s in shapes for g in R.bn_groups(s) for sl in SLOPES for pt in PASS]


def _run_batch_norm(dev, FF, shape, groups, slope, pt, dtype):
    (x, gamma, beta, gy, gpass), st = _bn_case(shape, groups, dtype)
    what = f"BatchNorm {dtype} {shape} groups {groups} slope {slope} {pt}"
    c = shape[-1]
    rows = x.numel() // c // groups
    _, _, lt = plan_norm_reduce(groups, rows, c)
    xd = x.to(dev).requires_grad_(True)
    gd, bd = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    out = FF.batch_norm_train(xd, gd, bd, EPS, groups, pt != "off", slope)
    y, stats, sums = out[:3]
    assert y.dtype == dtype and stats.shape == (groups, c, 2) and sums.dtype == F64
    x64, gy64, gp64 = x.double(), gy.double(), gpass.double()
    km, kr, kmask = _check_bn_forward(x64, gamma, beta, st, lt, y, stats, sums, slope, groups, dtype, what)
    if pt != "off":
        assert torch.equal(out[3].detach().cpu(), x), what + ": the pass-through output is not x"
    if pt == "pass_only":
        torch.autograd.backward([out[3]], [gpass.to(dev)])
        assert torch.equal(xd.grad.cpu(), gpass) and gd.grad is None and bd.grad is None
        return
    if pt == "both":
        torch.autograd.backward([y, out[3]], [gy.to(dev), gpass.to(dev)])
    else:
        torch.autograd.backward([y], [gy.to(dev)])
    _check_bn_backward(x64, gy64, gp64 if pt == "both" else None, gamma, beta, km, kr, kmask, lt, xd.grad, gd.grad, bd.grad, slope, groups,
                       dtype, what)


@pytest.mark.parametrize("shape,groups,slope,pt", _bn_cases(R.BN_F32_SHAPES), ids=lambda v: str(v).replace(" ", ""))
def test_batch_norm_f32(dev, FF, shape, groups, slope, pt):
    _run_batch_norm(dev, FF, shape, groups, slope, pt, torch.float32)


@pytest.mark.parametrize("shape,groups,slope,pt", _bn_cases(R.BN_BF16_SHAPES), ids=lambda v: str(v).replace(" ", ""))
def test_batch_norm_bf16(dev, FF, shape, groups, slope, pt):
    _run_batch_norm(dev, FF, shape, groups, slope, pt, BF16)


def test_batch_norm_one_row(dev, FF):
    """one row per channel: xhat = 0 exactly, so y = act(beta) and gx = 0 exactly (g' - mean g' = 0), and rstd is within the statistics
    bound of 1 / sqrt(eps) (test_batch_norm_f32 at this shape: the fp32 x x of the one-element run against the fp64 mean^2).  Channel 0
    has beta = 0: pre is an exact zero there, and y = 0 whichever side of the kink takes it, at slope 0 as at 0.2"""
    (x, gamma, beta, gy, _), st = _bn_case((1, 1, 1, 8), 1, torch.float32)
    assert bool((st.var == 0).all())
    beta = beta.clone()
    beta[0] = 0.0
    for slope in (0.0, 0.2):
        xd = x.to(dev).requires_grad_(True)
        y, stats, _ = FF.batch_norm_train(xd, gamma.to(dev), beta.to(dev), EPS, 1, False, slope)
        assert torch.equal(y.detach().cpu().reshape(-1), torch.where(beta > 0, beta, slope * beta))
        y.backward(gy.to(dev))
        assert torch.equal(xd.grad.cpu(), torch.zeros_like(x))


@pytest.mark.parametrize("pt", ["both", "pass_only", "off"])
def test_instance_norm_act_passthrough(dev, FF, lib, pt):
    """FF.instance_norm_act shares the kernels: per-sample statistics = one group per sample.  Its statistics stay inside the op; the
    same launch with the same workspace (partial rows added in a fixed order: bit-reproducible) hands them to the references"""
    shape, slope, dtype = (2, 33, 31, 64), 0.1, torch.float32
    (x, gamma, beta, gy, gpass), _ = _bn_case(shape, 2, dtype)
    n, c = shape[0], shape[-1]
    hw = shape[1] * shape[2]
    st = R.bn_stats(x.double(), EPS32, n)
    _, _, lt = plan_norm_reduce(n, hw, c)
    what = f"instance_norm_act {pt}"
    xd = x.to(dev).requires_grad_(True)
    gd, bd = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    sums, ws = FF._norm_ws(dev, n, c)
    stats = _nan((n, c, 2), dev)
    lib.instnorm_stats_f32(FF._p(xd), _vp(sums), FF._p(stats), n, hw, c, EPS, _vp(ws), ws.numel(), FF._st())
    out = FF.instance_norm_act(xd, gd, bd, EPS, slope, pt != "off")
    y = out[0] if pt != "off" else out
    km, kr, kmask = _check_bn_forward(x.double(), gamma, beta, st, lt, y, stats, sums, slope, n, dtype, what)
    if pt != "off":
        assert torch.equal(out[1].detach().cpu(), x), what + ": the pass-through output is not x"
    if pt == "pass_only":
        torch.autograd.backward([out[1]], [gpass.to(dev)])  # this op gets a zero-filled g: its kernels run, and add exactly nothing
        assert torch.equal(xd.grad.cpu(), gpass)
        assert all(p_.grad is None or not bool(p_.grad.any()) for p_ in (gd, bd))
        return
    if pt == "both":
        torch.autograd.backward([y, out[1]], [gy.to(dev), gpass.to(dev)])
    else:
        y.backward(gy.to(dev))
    _check_bn_backward(x.double(), gy.double(), gpass.double() if pt == "both" else None, gamma, beta, km, kr, kmask, lt, xd.grad, gd.grad,
                       bd.grad, slope, n, dtype, what)


# ---- reductions without a workspace (raw ABI): fp64 / fp32 atomics, and the reproducible mode --------------------------------------
def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=dev, dtype=dtype)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("shape", [(2, 33, 31, 64), (1, 70, 64, 8)])
@pytest.mark.parametrize("det", [False, True])
def test_norm_reductions_without_workspace(dev, FF, lib, shape, det):
    n, h, w, c = shape
    hw, slope = h * w, 0.2
    x, gamma, beta, gy, _ = R.bn_inputs(shape, 1, 77 + c, torch.float32)
    st = R.bn_stats(x.double(), EPS32, n)
    _, blocks, lt = plan_norm_reduce(n, hw, c, ws=False, det=det)
    assert blocks == 1 if det else (blocks == 2 if c == 64 else blocks == 9)
    xd, gyd, gd, bd = x.to(dev), gy.to(dev), gamma.to(dev), beta.to(dev)
    what = f"no-workspace {shape} det={det}"

    def run():
        sums, red = torch.zeros((n, c, 2), device=dev, dtype=F64), torch.zeros((n, c, 2), device=dev, dtype=F64)  # accumulated onto: zeroed
        stats, y = _nan((n, c, 2), dev), _nan(shape, dev)
        lib.instnorm_stats_f32(FF._p(xd), _vp(sums), FF._p(stats), n, hw, c, EPS, None, 0, FF._st())
        lib.instnorm_apply_f32(FF._p(xd), FF._p(stats), FF._p(gd), FF._p(bd), FF._p(y), n, hw, c, slope, FF._st())
        lib.instnorm_bwd_reduce_f32(FF._p(xd), FF._p(gyd), FF._p(stats), FF._p(gd), FF._p(bd), _vp(red), n, hw, c, slope, None, 0, FF._st())
        return sums, stats, y, red

    with FF.deterministic(det):
        sums, stats, y, red = run()
        again = run() if det else None
    km, kr, kmask = _check_bn_forward(x.double(), gamma, beta, st, lt, y, stats, sums, slope, n, torch.float32, what)
    bw = R.bn_backward(x.double(), gy.double(), km, kr, gamma.double(), beta.double(), slope, n, kmask)
    _within(red[..., 0], bw.m1 * hw, _red_tol(lt, bw.m1_abs * hw), what + " sum g'")
    _within(red[..., 1], bw.m2 * hw, _red_tol(lt, bw.m2_abs * hw), what + " sum g' xhat")
    if det:
        for a, b in zip((sums, stats, y, red), again):
            assert torch.equal(a, b), what + ": two reproducible-mode runs differ"


@pytest.mark.parametrize("det", [False, True])
def test_scale_channels_gs_without_workspace(dev, FF, lib, det):
    n, p, c = 2, 33 * 31, 64
    gen = torch.Generator().manual_seed(81)
    x, g = torch.randn(n, p, c, generator=gen), torch.randn(n, p, c, generator=gen)
    ref = R.scale_channels(x.double(), torch.ones(n, c, dtype=F64), g.double())
    blocks, L = plan_scale_gs_f32(n, p, c, ws=False, det=det)
    assert blocks == (1 if det else 8)
    xd, gd = x.to(dev), g.to(dev)

    def run():
        gs = torch.zeros(n, c, device=dev)  # fp32 atomics add onto it
        lib.scale_channels_gs_f32(FF._p(gd), FF._p(xd), FF._p(gs), None, 0, n, p, c, FF._st())
        return gs

    with FF.deterministic(det):
        gs = run()
        again = run() if det else None
    _within(gs, ref.gs, _red_tol(L, ref.gs_mag), f"scale_channels_gs without workspace det={det}")
    if det:
        assert torch.equal(gs, again)


# ---- running statistics --------------------------------------------------------------------------------------------------------
def _momentum_step(r, err, stat, dstat, m):
    """r' = (1 - m) r + m stat in fp32 (1 - m, two products, one sum: within the element-wise 8 u32 mag) with stat known to dstat"""
    mag = (1 - m) * r.abs() + m * stat.abs()
    return (1 - m) * r + m * stat, (1 - m) * err + 8 * U32 * mag + m * dstat


@pytest.mark.parametrize("c", [5, 300])
@pytest.mark.parametrize("form", ["sums", "rstd"])
@pytest.mark.parametrize("offset", [False, True])
def test_running_update(dev, FF, c, form, offset):
    """stats = the float64 statistics rounded to fp32 (1 u32 each), sums = float64: the kernel's own arithmetic is what is measured.
    Channel 1 has variance ~1e-9 at eps 1e-5.  Bounds of the batch variance the kernel forms:
      sums form   var = (s2 / n - m^2) unbias in fp64, stored as fp32: 2 u32 var + the fp64 cancellation (log2 n + 4) 2^-53 2 E[x^2]
      rstd form   var = (1 / rstd^2 - eps) unbias in fp32: rstd carries u32, the square and the quotient one each, so 1 / rstd^2 is
                  (var + eps)(1 +- 4 u32); the difference keeps that ABSOLUTE error: 4 u32 (var + eps) unbias + 2 u32 var.  For
                  var << eps that is 4 u32 eps / var relative -- 0.24% at var = 1e-9 -- which is why the module passes sums"""
    gen = torch.Generator().manual_seed(90 + c)
    n, h, w, mom = 3, 4, 5, 0.1
    cnt = n * h * w
    x = torch.randn(n, h, w, c, generator=gen) * (torch.rand(c, generator=gen) + 0.5) + torch.randn(c, generator=gen)
    x[..., 1] = 0.25 + 10 ** -4.5 * torch.randn(n, h, w, generator=gen)
    x64 = x.double()
    off = torch.randn(c, generator=gen) if offset else None
    bn = torch.nn.BatchNorm2d(c, eps=EPS32, momentum=mom).double()
    bn.running_mean.copy_(torch.randn(c, generator=gen))
    bn.running_var.copy_(torch.rand(c, generator=gen) + 0.5)
    bn.running_var[1] = 0.0  # nothing to hide the tiny batch variance behind
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    st = R.bn_stats(x64, EPS32)
    stats = torch.stack([st.mean[0], st.rstd[0]], -1).float().reshape(1, c, 2).contiguous()
    sums = torch.stack([st.s1[0], st.s2[0]], -1).reshape(1, c, 2).contiguous()
    rm, rv = rm0.float().to(dev), rv0.float().to(dev)
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    unb = cnt / (cnt - 1)
    var_unb = st.var[0] * unb
    dmean = U32 * st.mean[0].abs() + (U32 * (st.mean[0] + off.double()).abs() if offset else 0)
    if form == "sums":
        dvar = 2 * U32 * var_unb + (math.ceil(math.log2(cnt)) + 4) * U64 * 2 * (st.s2[0] / cnt) * unb
    else:
        dvar = 4 * U32 * (st.var[0] + EPS32) * unb + 2 * U32 * var_unb
    r_m, r_v = rm0.float().double(), rv0.float().double()
    e_m, e_v = torch.zeros(c, dtype=F64), torch.zeros(c, dtype=F64)
    bn.running_mean.copy_(r_m)
    bn.running_var.copy_(r_v)
    for k in range(2):
        bn(((x64 + off.double()) if offset else x64).permute(0, 3, 1, 2))  # the offset shifts the mean and leaves the variance
        FF.batch_norm_running_update(stats.to(dev), rm, rv, nbt, cnt, EPS, mom, sums.to(dev) if form == "sums" else None,
                                     off.to(dev) if offset else None)
        assert int(nbt) == k + 1
        r_m, e_m = _momentum_step(r_m, e_m, st.mean[0] + (off.double() if offset else 0), dmean, mom)
        r_v, e_v = _momentum_step(r_v, e_v, var_unb, dvar, mom)
    # the float64 module and the closed form agree; the kernel is held to the closed form's bound around the module's values
    torch.testing.assert_close(r_m, bn.running_mean, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r_v, bn.running_var, rtol=1e-9, atol=1e-12)
    _within(rm, bn.running_mean, e_m, f"running_mean C={c} {form}")
    _within(rv, bn.running_var, e_v, f"running_var C={c} {form}")
    assert torch.equal(nbt.cpu(), bn.num_batches_tracked) and int(nbt) == 2


@pytest.mark.parametrize("form", ["sums", "rstd"])
def test_running_update_count_one(dev, FF, form):
    """count = 1: variance 0, the unbiased factor taken as 1 (torch refuses a one-value batch; the closed form is the reference)"""
    c, mom = 5, 0.3
    gen = torch.Generator().manual_seed(95)
    x = torch.randn(1, 1, 1, c, generator=gen)
    st = R.bn_stats(x.double(), EPS32)
    assert bool((st.var == 0).all())
    stats = torch.stack([st.mean[0], st.rstd[0]], -1).float().reshape(1, c, 2).contiguous()
    sums = torch.stack([st.s1[0], st.s2[0]], -1).reshape(1, c, 2).contiguous()
    rm0, rv0 = torch.randn(c, generator=gen), torch.rand(c, generator=gen) + 0.5
    rm, rv, nbt = rm0.to(dev), rv0.to(dev), torch.full((), 41, dtype=torch.int64, device=dev)
    FF.batch_norm_running_update(stats.to(dev), rm, rv, nbt, 1, EPS, mom, sums.to(dev) if form == "sums" else None)
    ref = R.bn_running_update(rm0.double(), rv0.double(), 41, x.double().reshape(c), st.var[0], 1, mom)
    dvar = 4 * U32 * EPS32 if form == "rstd" else (math.ceil(math.log2(1)) + 4) * U64 * 2 * st.s2[0]
    _, e_m = _momentum_step(rm0.double(), 0.0, x.double().reshape(c), U32 * x.double().reshape(c).abs(), mom)
    _, e_v = _momentum_step(rv0.double(), 0.0, st.var[0], dvar, mom)
    _within(rm, ref.rmean, e_m, "running_mean count 1")
    _within(rv, ref.rvar, e_v, "running_var count 1")
    assert int(nbt) == 42 == ref.nbt


# ---- helpers.batch_norm on an nn.BatchNorm2d ---------------------------------------------------------------------------------------
def _make_bn(c, dev, gen, momentum=0.1):
    bn = torch.nn.BatchNorm2d(c, eps=EPS, momentum=momentum)
    with torch.no_grad():
        bn.weight.copy_((torch.rand(c, generator=gen) + 0.5) * (torch.randint(0, 2, (c,), generator=gen) * 2 - 1))
        bn.bias.copy_(torch.rand(c, generator=gen) * 2 - 1)
        bn.running_mean.copy_(torch.randn(c, generator=gen))
        bn.running_var.copy_(torch.rand(c, generator=gen) + 0.5)
    ref = torch.nn.BatchNorm2d(c, eps=EPS32, momentum=momentum).double()
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in bn.state_dict().items()})
    return bn.to(dev), ref


HELPER_SHAPE = (4, 9, 7, 64)


@pytest.mark.parametrize("mode", ["groups2", "cumulative"])
def test_helpers_batch_norm_training(dev, FF, mode):
    """training: the running buffers after two updates equal two sequential float64 calls -- with BN_GROUPS = [2] the two halves of ONE
    batch, in order; with momentum=None the cumulative average over two calls"""
    from face_mask_inpaint_amd.modules.psp.encoders import helpers as H

    shape = HELPER_SHAPE
    c = shape[-1]
    groups = 2 if mode == "groups2" else 1
    (x, _, _, _, _), st = _bn_case(shape, groups, torch.float32)
    gen = torch.Generator().manual_seed(101)
    bn, ref = _make_bn(c, dev, gen, 0.1 if mode == "groups2" else None)
    bn.train(), ref.train()
    rows = x.numel() // c // groups
    _, _, lt = plan_norm_reduce(groups, rows, c)
    _, _, dmean, dvar, _ = _stat_bounds(st, lt)
    unb = rows / (rows - 1)
    r_m, r_v = ref.running_mean.clone(), ref.running_var.clone()
    e_m, e_v = torch.zeros(c, dtype=F64), torch.zeros(c, dtype=F64)
    old = H.BN_GROUPS[0]
    try:
        H.BN_GROUPS[0] = groups
        with torch.no_grad():
            if mode == "groups2":
                y = H.batch_norm(bn, x.to(dev), slope=0.2)
                steps = [(0, 0.1), (1, 0.1)]
                for part in x.double().chunk(2, 0):
                    ref(part.permute(0, 3, 1, 2))
            else:
                for _ in range(2):
                    y = H.batch_norm(bn, x.to(dev))
                    ref(x.double().permute(0, 3, 1, 2))
                steps = [(0, 1.0), (0, 0.5)]
    finally:
        H.BN_GROUPS[0] = old
    for g, m in steps:
        var_unb = st.var[g] * unb
        r_m, e_m = _momentum_step(r_m, e_m, st.mean[g], dmean[g], m)
        r_v, e_v = _momentum_step(r_v, e_v, var_unb, dvar[g] * unb + 2 * U32 * var_unb, m)
    torch.testing.assert_close(r_m, ref.running_mean, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r_v, ref.running_var, rtol=1e-10, atol=1e-12)
    _within(bn.running_mean, ref.running_mean, e_m, mode + " running_mean")
    _within(bn.running_var, ref.running_var, e_v, mode + " running_var")
    assert torch.equal(bn.num_batches_tracked.cpu(), ref.num_batches_tracked) and int(bn.num_batches_tracked) == 2
    # the helper hands its groups and slope on: its y is, bit for bit, what FF.batch_norm_train gives for them (a partials workspace and
    # a fixed adding order: reproducible), and that entry is held to float64 by test_batch_norm_f32 at this very shape
    want = FF.batch_norm_train(x.to(dev), bn.weight.detach(), bn.bias.detach(), bn.eps, groups, False, 0.2 if mode == "groups2" else 1.0)[0]
    assert torch.equal(y, want), mode + ": helpers.batch_norm does not pass its groups / slope on"


def _affine_bounds(bn, ref):
    """scale = w / sqrt(rv + eps), shift = b - rm scale are [C]-sized torch fp32 expressions (sum, sqrt, quotient; product, difference):
    held to 8 u32 mag.  Returns the float64 (scale, shift) of the fp32 module's own parameters"""
    s = ref.weight / torch.sqrt(ref.running_var + EPS32)
    return s.detach(), (ref.bias - ref.running_mean * s).detach(), (ref.bias.abs() + (ref.running_mean * s).abs()).detach()


@pytest.mark.parametrize("pt", [False, True])
def test_helpers_batch_norm_eval_frozen(dev, FF, pt):
    """eval mode, frozen parameters: FF.channel_affine forward, and gx = g scale (+ the other consumer's gradient, joined in the pass)"""
    from face_mask_inpaint_amd.modules.psp.encoders import helpers as H

    shape = HELPER_SHAPE
    (x, _, _, gy, gpass), _ = _bn_case(shape, 1, torch.float32)
    bn, ref = _make_bn(shape[-1], dev, torch.Generator().manual_seed(102))
    bn.eval()
    for p_ in bn.parameters():
        p_.requires_grad_(False)
    xd = x.to(dev).requires_grad_(True)
    out = H.batch_norm(bn, xd, passthrough=pt)
    y = out[0] if pt else out
    s64, t64, t_mag = _affine_bounds(bn, ref)
    _, ks, kt = bn._fmi_affine  # the operands the kernel read
    _within(ks, s64, 8 * U32 * s64.abs(), "frozen scale")
    _within(kt, t64, 8 * U32 * t_mag + _d(bn.running_mean).abs() * 8 * U32 * s64.abs(), "frozen shift")
    r = R.channel_affine(x.double(), _d(ks), _d(kt), gy.double(), gpass.double() if pt else None)
    _within(y, r.y, _elem_tol(r.y, r.y_mag, torch.float32), "channel_affine y")
    if pt:
        assert torch.equal(out[1].detach().cpu(), x)
        torch.autograd.backward([y, out[1]], [gy.to(dev), gpass.to(dev)])
    else:
        y.backward(gy.to(dev))
    _within(xd.grad, r.gx, _elem_tol(r.gx, r.gx_mag, torch.float32), "channel_affine gx")


def test_helpers_batch_norm_eval_trainable(dev, FF):
    """eval mode, trainable weight and bias: y = scale_channels(x, scale) + shift; d weight = (gs - rm gb) / sqrt(rv + eps), d bias = gb
    with gs = sum g x (the one-pass adjoint, x needs its gradient too) and gb = sum g (fmi_bias_grad_f32)"""
    from face_mask_inpaint_amd.modules.psp.encoders import helpers as H

    shape = HELPER_SHAPE
    c = shape[-1]
    rows = shape[0] * shape[1] * shape[2]
    (x, _, _, gy, _), _ = _bn_case(shape, 1, torch.float32)
    bn, ref = _make_bn(c, dev, torch.Generator().manual_seed(103))
    bn.eval()
    xd = x.to(dev).requires_grad_(True)
    y = H.batch_norm(bn, xd)
    s64, t64, t_mag = _affine_bounds(bn, ref)
    r = R.channel_affine(x.double(), s64, t64, gy.double())
    # scale / shift are torch fp32 here (8 u32 each, as in _affine_bounds), then x scale (1 rounding) + shift (1 rounding)
    y_tol = 8 * U32 * r.y_mag + x.double().abs() * 8 * U32 * s64.abs() + 8 * U32 * t_mag + _d(bn.running_mean).abs() * 8 * U32 * s64.abs()
    _within(y, r.y, y_tol, "eval trainable y")
    y.backward(gy.to(dev))
    _within(xd.grad, r.gx, 8 * U32 * r.gx_mag + gy.double().abs() * 8 * U32 * s64.abs(), "eval trainable gx")
    g2, x2 = gy.double().reshape(-1, c), x.double().reshape(-1, c)
    gs, gs_mag, gb, gb_mag = (g2 * x2).sum(0), (g2 * x2).abs().sum(0), g2.sum(0), g2.abs().sum(0)
    _, L_gs = plan_scale_bwd_f32(1, rows, c)
    L_gb = plan_bias_grad(rows, c)
    d_gs, d_gb = _red_tol(L_gs, gs_mag), _red_tol(L_gb, gb_mag)
    _within(bn.bias.grad, gb, d_gb, "eval trainable d bias")
    inv = 1 / torch.sqrt(ref.running_var + EPS32)
    rm = ref.running_mean
    dw = (gs - rm * gb) * inv
    dw_mag = (gs.abs() + (rm * gb).abs()) * inv
    _within(bn.weight.grad, dw, 8 * U32 * dw_mag + (d_gs + rm.abs() * d_gb) * inv, "eval trainable d weight")


# ---- PReLU ---------------------------------------------------------------------------------------------------------------------
def _prelu_inputs(rows, c, seed, dtype):
    gen = torch.Generator().manual_seed(seed)
    x, g = torch.randn(rows, c, generator=gen), torch.randn(rows, c, generator=gen)
    x.view(-1)[::7] = 0.0  # exact zeros: the x > 0 / x <= 0 sides of the kink
    a = torch.rand(c, generator=gen) * 0.5
    a[0], a[1] = -0.25, 0.0
    return x.to(dtype), a, g.to(dtype)


def _check_prelu(dev, FF, rows, c, dtype, L, what):
    x, a, g = _prelu_inputs(rows, c, 200 + c + rows, dtype)
    r = R.prelu(x.double(), a.double(), g.double())
    xd, ad = x.to(dev).requires_grad_(True), a.to(dev).requires_grad_(True)
    y = FF.prelu(xd, ad)
    _within(y, r.y, _elem_tol(r.y, r.y_mag, dtype), what + " y")
    y.backward(g.to(dev))
    _within(xd.grad, r.gx, _elem_tol(r.gx, r.gx_mag, dtype), what + " gx")
    _within(ad.grad, r.ga, _red_tol(L, r.ga_mag), what + " ga")
    return xd.grad, ad.grad


def _cells(test, *axes):
    """the full cross of the axes, less the cells OMITTED lists for this test"""
    return [cell for cell in itertools.product(*axes) if (test, cell) not in OMITTED]


@pytest.mark.parametrize("c,rows", _cells("prelu_f32_vector", (4, 64, 1024), (3, 252, 7232)))
def test_prelu_f32_vector(dev, FF, c, rows):
    path, _, L = plan_prelu_bwd_f32(rows, c)
    assert path == "vec"
    _check_prelu(dev, FF, rows, c, torch.float32, L, f"PReLU fp32 C={c} rows={rows}")


@pytest.mark.parametrize("c", [6, 12, 132])
@pytest.mark.parametrize("rows", [3, 300])
@pytest.mark.parametrize("det", [False, True])
def test_prelu_f32_scalar_atomic(dev, FF, c, rows, det):
    path, _, L = plan_prelu_bwd_f32(rows, c, det)
    assert path == "scalar"
    with FF.deterministic(det):
        a = _check_prelu(dev, FF, rows, c, torch.float32, L, f"PReLU fp32 scalar C={c} rows={rows} det={det}")
        if det:
            b = _check_prelu(dev, FF, rows, c, torch.float32, L, "second run")
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("c,rows", _cells("prelu_bf16", (8, 64, 2048), (3, 480, 40000)))
def test_prelu_bf16(dev, FF, c, rows):
    _, L = plan_prelu_bwd_bf16(rows, c)
    _check_prelu(dev, FF, rows, c, BF16, L, f"PReLU bf16 C={c} rows={rows}")


def test_prelu_bf16_odd_chunk_count(dev, FF):
    """C = 96 (12 eight-channel chunks, not a power of two): the forward is element-wise and right; the backward kernel's lane layout
    does not cover it and the call raises instead of returning a value"""
    x, a, g = _prelu_inputs(30, 96, 296, BF16)
    r = R.prelu(x.double(), a.double())
    xd, ad = x.to(dev).requires_grad_(True), a.to(dev).requires_grad_(True)
    y = FF.prelu(xd, ad)
    _within(y, r.y, _elem_tol(r.y, r.y_mag, BF16), "PReLU bf16 C=96 y")
    with pytest.raises(FF.FmiError):
        y.backward(g.to(dev))


# ---- SE gate -------------------------------------------------------------------------------------------------------------------
def _gate_inputs(n, p, c, seed, dtype):
    gen = torch.Generator().manual_seed(seed)
    x, res, g = (torch.randn(n, p, c, generator=gen) for _ in range(3))
    s = (torch.rand(n, c, generator=gen) + 0.5) * 3.0 ** torch.arange(n).reshape(n, 1)  # a wrong sample index is O(1) wrong
    return x.to(dtype), s, res.to(dtype), g.to(dtype)


def _check_gate(dev, FF, n, p, c, dtype, add, L, what, x_grad=True):
    x, s, res, g = _gate_inputs(n, p, c, 300 + n + p + c, dtype)
    r = R.scale_channels(x.double(), s.double(), g.double(), res.double() if add else None)
    xd, sd, rd = x.to(dev).requires_grad_(x_grad), s.to(dev).requires_grad_(True), res.to(dev).requires_grad_(add)
    gd = g.to(dev)
    y = FF.scale_channels_add(xd, sd, rd) if add else FF.scale_channels(xd, sd)
    _within(y, r.y, _elem_tol(r.y, r.y_mag, dtype), what + " y")
    y.backward(gd)
    if x_grad:
        _within(xd.grad, r.gx, _elem_tol(r.gx, r.gx_mag, dtype), what + " gx")
    else:
        assert xd.grad is None
    _within(sd.grad, r.gs, _red_tol(L, r.gs_mag), what + " gs")
    if add:
        assert torch.equal(rd.grad, gd), what + ": gres is not g"


@pytest.mark.parametrize("c,p,n", _cells("se_gate_one_pass", (4, 12, 64, 1024), (3, 252, 9000), (1, 3)))
@pytest.mark.parametrize("add", [False, True])
def test_se_gate_one_pass(dev, FF, c, p, n, add):
    _, L = plan_scale_bwd_f32(n, p, c)
    _check_gate(dev, FF, n, p, c, torch.float32, add, L, f"SE gate one-pass N={n} P={p} C={c} add={add}")


@pytest.mark.parametrize("n,p", [(1, 3), (3, 252), (2, 9000)])
def test_se_gate_two_launch(dev, FF, n, p):
    """C = 6: the scalar forward kernel and scale_channels_gs_kernel with its partials workspace; then C = 64 with only s requiring
    a gradient, which takes the same reduction"""
    _, L = plan_scale_gs_f32(n, p, 6)
    _check_gate(dev, FF, n, p, 6, torch.float32, False, L, f"SE gate two-launch N={n} P={p} C=6")
    _, L = plan_scale_gs_f32(n, p, 64)
    _check_gate(dev, FF, n, p, 64, torch.float32, False, L, f"SE gate s-only N={n} P={p} C=64", x_grad=False)
    _check_gate(dev, FF, n, p, 64, torch.float32, True, L, f"SE gate add s-only N={n} P={p} C=64", x_grad=False)


@pytest.mark.parametrize("c,p,n", _cells("se_gate_bf16", (8, 64, 2048), (3, 252, 9000), (1, 3)))
@pytest.mark.parametrize("add", [True, False])
def test_se_gate_bf16(dev, FF, c, p, n, add):
    _, L = plan_scale_gs_bf16(n, p, c)
    _check_gate(dev, FF, n, p, c, BF16, add, L, f"SE gate bf16 N={n} P={p} C={c} add={add}")


@pytest.mark.parametrize("n,p,c", [(2, 10, 12), (1, 5, 12), (3, 252, 12), (2, 37, 100)])
def test_se_gate_bf16_channels_not_a_multiple_of_8(dev, FF, n, p, c):
    """C % 8 != 0: FF.scale_channels_add leaves its fused bf16 kernel for scale_channels + add, whose eight-channel kernels do not cover
    such a C either; the library's one-element-per-thread forms do (chan.hip scale_channels_scalar_kernel<uint16_t> and
    scale_channels_gs_bf16_scalar_kernel: 4 row lanes, then a 2-level tree; add_bf16_scalar_kernel when the element count
    is no multiple of 8, as at (1, 5, 12)).  C = 100 takes two 64-channel stripes of the gs kernel, the second one partly idle.  The
    product is rounded to bf16 before the residual is added: two bf16 roundings"""
    x, s, res, g = _gate_inputs(n, p, c, 399 + p, BF16)
    r = R.scale_channels(x.double(), s.double(), g.double())
    xd, sd, rd = x.to(dev).requires_grad_(True), s.to(dev).requires_grad_(True), res.to(dev).requires_grad_(True)
    y = FF.scale_channels_add(xd, sd, rd)
    prod = _d(FF.scale_channels(x.to(dev), s.to(dev)))  # the rounded product the add kernel read
    _within(prod, r.y, _elem_tol(r.y, r.y_mag, BF16), "bf16 odd C product")
    y_ref = prod + res.double()
    _within(y, y_ref, _elem_tol(y_ref, prod.abs() + res.double().abs(), BF16), "bf16 odd C y")
    y.backward(g.to(dev))
    _within(xd.grad, r.gx, _elem_tol(r.gx, r.gx_mag, BF16), "bf16 odd C gx")
    _within(sd.grad, r.gs, _red_tol(_cdiv(p, 4) + 2, r.gs_mag), "bf16 odd C gs")
    assert torch.equal(rd.grad.cpu(), g)


def test_se_gate_bf16_refuses_what_it_has_no_layout_for(dev, FF, lib):
    """C % 8 == 0 with C / 8 no power of two (C = 96): the gs reduction has neither its chunk layout nor the scalar form (which is for
    odd widths only) and refuses, as fmi_prelu_bwd_bf16 does for the same C; the scalar form needs no workspace"""
    n, p = 2, 20
    x, s, _, g = _gate_inputs(n, p, 96, 398, BF16)
    xd, gd = x.to(dev), g.to(dev)
    ws, out = torch.empty(2048 * 96, device=dev), _nan((n, 96), dev)
    with pytest.raises(FF.FmiError):
        lib.scale_channels_gs_bf16(FF._p(gd), FF._p(xd), FF._p(out), FF._p(ws), ws.numel(), n, p, 96, FF._st())
    x, s, _, g = _gate_inputs(n, p, 12, 397, BF16)
    xd, gd, gs = x.to(dev), g.to(dev), _nan((n, 12), dev)
    lib.scale_channels_gs_bf16(FF._p(gd), FF._p(xd), FF._p(gs), None, 0, n, p, 12, FF._st())
    r = R.scale_channels(x.double(), s.double(), g.double())
    _within(gs, r.gs, _red_tol(_cdiv(p, 4) + 2, r.gs_mag), "bf16 C=12 gs without a workspace")


# ---- global pool with pass-through -------------------------------------------------------------------------------------------------
def _check_pool(dev, FF, shape, dtype, L, what):
    n, h, w, c = shape
    gen = torch.Generator().manual_seed(400 + h + c)
    x = (torch.randn(shape, generator=gen) + 0.5 * torch.arange(1, n + 1).reshape(n, 1, 1, 1)).to(dtype)
    gp, gx_pass = torch.randn(n, c, generator=gen), torch.randn(shape, generator=gen).to(dtype)
    r = R.global_pool_pass(x.double(), gp.double(), gx_pass.double())
    xd = x.to(dev).requires_grad_(True)
    pooled, xp = FF.global_avg_pool_pass_bf16(xd) if dtype == BF16 else FF.global_avg_pool_pass(xd)
    assert pooled.dtype == torch.float32
    _within(pooled, r.pooled, _red_tol(L, r.pooled_mag), what + " pooled")
    assert torch.equal(xp.detach().cpu(), x), what + ": the pass-through output is not x"
    torch.autograd.backward([pooled, xp], [gp.to(dev).reshape(pooled.shape), gx_pass.to(dev)])
    _within(xd.grad, r.gx, _elem_tol(r.gx, r.gx_mag, dtype), what + " joined gx")
    return pooled


@pytest.mark.parametrize("shape,det", [((2, 16, 16, 64), False), ((3, 8, 8, 512), False), ((2, 4, 4, 64), False), ((2, 16, 16, 12), False),
                                       ((2, 16, 16, 64), True)])
def test_global_pool_f32(dev, FF, shape, det):
    _, L = plan_pool_f32(*shape, det=det)
    with FF.deterministic(det):
        a = _check_pool(dev, FF, shape, torch.float32, L, f"global pool fp32 {shape} det={det}")
        if det:
            assert torch.equal(a, _check_pool(dev, FF, shape, torch.float32, L, "second run"))


def test_global_pool_f32_refuses_a_map_that_is_not_square(dev, FF):
    """the fp32 entry pools with a k x k window, k = H: a wider or narrower map is refused instead of being pooled over H x H of it"""
    for shape in [(2, 8, 16, 64), (1, 4, 2, 8)]:
        with pytest.raises(FF.FmiError, match="square"):
            FF.global_avg_pool_pass(torch.zeros(shape, device=dev))


@pytest.mark.parametrize("shape", [(2, 1, 3, 8), (4, 12, 10, 64), (2, 80, 80, 512), (1, 16, 16, 2048)])
def test_global_pool_bf16(dev, FF, shape):
    n, h, w, c = shape
    _, L = plan_pool_bf16(n, h * w, c)
    _check_pool(dev, FF, shape, BF16, L, f"global pool bf16 {shape}")


# ---- subsample -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent,stride", [((2, 7, 9), 2), ((2, 8, 8), 2), ((1, 1, 5), 2), ((1, 10, 7), 3)])
@pytest.mark.parametrize("c,dtype", [(8, torch.float32), (6, torch.float32), (8, BF16)])
def test_subsample(dev, FF, extent, stride, c, dtype):
    gen = torch.Generator().manual_seed(500 + c + stride)
    x = torch.randn(*extent, c, generator=gen).to(dtype)
    xd = x.to(dev).requires_grad_(True)
    y = FF.subsample(xd, stride)
    assert torch.equal(y.detach().cpu(), x[:, ::stride, ::stride])
    g = torch.randn(y.shape, generator=gen).to(dtype)
    y.backward(g.to(dev))
    assert torch.equal(xd.grad.cpu(), R.subsample(x, stride, g).gx)


# ---- which kernel an entry takes, and what it refuses ------------------------------------------------------------------------------
def _off_by_one(t, dev):
    """the values of t on the device as a contiguous view that starts one element into a 16-byte-aligned buffer"""
    buf = torch.empty(t.numel() + 16, device=dev, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def test_f32_forward_chunk_and_scalar_kernels(dev, FF, lib):
    """fmi_scale_channels_f32 reaches its chunk kernel (C % 4 == 0 and x, y, s on 16 bytes) and its one-element kernel two ways: by width
    (C = 6) and by alignment (C = 8, x one float into a buffer); fmi_prelu_f32 likewise by alignment.  Each against float64, and the
    aligned and the misaligned run of the same values bit for bit against each other"""
    for n, p, c in [(2, 3, 8), (2, 5, 6)]:
        x, s, _, _ = _gate_inputs(n, p, c, 600 + c, torch.float32)
        r = R.scale_channels(x.double(), s.double())
        xd, sd = x.to(dev), s.to(dev)
        forms = [xd] if c % 4 else [xd, _off_by_one(x, dev)]
        ys = []
        for xf in forms:
            y = _nan((n, p, c), dev)
            lib.scale_channels_f32(FF._p(xf), FF._p(sd), FF._p(y), n, p, c, FF._st())
            _within(y, r.y, _elem_tol(r.y, r.y_mag, torch.float32), f"scale_channels fp32 C={c} x at {xf.data_ptr() % 16}")
            ys.append(y)
        assert len(ys) == 1 or torch.equal(ys[0], ys[1]), "scale_channels fp32: chunk and scalar kernel differ"
    rows, c = 6, 8
    x, a, _ = _prelu_inputs(rows, c, 608, torch.float32)
    r = R.prelu(x.double(), a.double())
    ad, ys = a.to(dev), []
    for xf in (x.to(dev), _off_by_one(x, dev)):
        y = _nan((rows, c), dev)
        lib.prelu_f32(FF._p(xf), FF._p(ad), FF._p(y), rows, c, FF._st())
        _within(y, r.y, _elem_tol(r.y, r.y_mag, torch.float32), f"PReLU fp32 x at {xf.data_ptr() % 16}")
        ys.append(y)
    assert torch.equal(ys[0], ys[1]), "PReLU fp32: chunk and scalar kernel differ"


def test_bf16_chunk_entries_refuse_a_misaligned_operand(dev, FF, lib):
    """the bf16 entries have no one-element form for C % 8 == 0: a tensor that starts one element into a buffer is refused, and nothing
    is launched (the output keeps its fill)"""
    n, p, c = 1, 2, 8
    x, s, res, _ = _gate_inputs(n, p, c, 620, BF16)
    xd, sd, rd, xo = x.to(dev), s.to(dev), res.to(dev), _off_by_one(x, dev)
    fill = torch.full((n, p, c), 7.0, device=dev, dtype=BF16)
    y = fill.clone()
    calls = {
        "scale_channels_add": lambda: lib.scale_channels_add_bf16(FF._p(xo), FF._p(sd), FF._p(rd), FF._p(y), n, p, c, FF._st()),
        "add_bcast": lambda: lib.add_bcast_bf16(FF._p(xo), FF._p(sd), FF._p(y), n, p, c, FF._st()),
        "prelu": lambda: lib.prelu_bf16(FF._p(xo), FF._p(sd), FF._p(y), n * p, c, FF._st()),
    }
    for name, call in calls.items():
        with pytest.raises(FF.FmiError, match="unsupported"):
            call()
        assert torch.equal(y, fill), name + ": the refused call wrote its output"
    lib.scale_channels_add_bf16(FF._p(xd), FF._p(sd), FF._p(rd), FF._p(y), n, p, c, FF._st())  # the aligned twin of the first call runs
    assert not torch.equal(y, fill)


# ---- the two bf16 roundings stay where they are ------------------------------------------------------------------------------------
def _bf16_bits_host(f32):
    """fp32 tensor -> bf16 bit patterns (int64) by the rule of bf_round_nan (csrc/bf16x8.h) in integer arithmetic: a NaN stays a quiet NaN
    with its sign, everything else -- infinities included -- rounds to nearest even"""
    u = f32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    rne = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return torch.where(nan, (u | 0x00400000) >> 16, rne) & 0xFFFF


def _bits_of(bf):
    return bf.contiguous().view(torch.int16).to(torch.int64).cpu() & 0xFFFF


def _from_bits(bits):
    return (bits - ((bits & 0x8000) << 1)).to(torch.int16).view(BF16)


def test_user_tensor_entries_quiet_a_nan_and_round_to_nearest_even(dev, FF, lib):
    """fmi_fused_bias_act_bf16 and fmi_upfirdn2d_bf16 take a caller's tensor: 1 x 8 channels x 4 x 4 with +-inf, +-NaN, the largest
    finite bf16 and the images of two fp32 ties (0x3f808000: even lower neighbour, 0x3f818000: odd) under the host rule.  With identity
    settings (no bias, slope 1, scale 1; one tap of 1.0) the output bits are the host rule of the input, every element.  A bf16 INPUT
    cannot hold a tie, so a second pass scales by 1.5 (scale, or one tap of 1.5): 1.5 (1 + 2^-7) and 1.5 (1 + 3 2^-7) are ties inside
    the kernel with an odd and an even lower neighbour, 1.5 x 0x7f7f overflows to an infinity; NaN payloads under a multiplication are
    the hardware's, so there the NaN elements are only required to stay NaN"""
    special = torch.tensor([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F7F0000, 0xFF7F0000, 0x3F808000, 0x3F818000, 0xBF808000,
                            0xBF818000, 0x3F810000, 0x3F830000, 0xBF810000, 0xBF830000], dtype=torch.int64)
    f = torch.randn(8 * 16, generator=torch.Generator().manual_seed(640))
    f[:special.numel()] = (special - ((special & 0x80000000) << 1)).to(torch.int32).view(torch.float32)
    x = _from_bits(_bf16_bits_host(f)).reshape(8, 4, 4)  # [major = N C, H, W]
    assert _bits_of(x)[0, 1, 2:4].tolist() == [0x3F80, 0x3F82]  # the ties went to their even neighbours
    xd = x.to(dev)
    wide = x.float()
    nan = torch.isnan(wide)

    def check(out, factor, what):
        got = _bits_of(out)
        want = _bf16_bits_host(wide * factor).reshape(got.shape)
        if factor == 1.0:
            assert torch.equal(got, want), what
        else:
            assert torch.equal(got[~nan], want[~nan]) and bool(torch.isnan(out.float().cpu()[nan]).all()), what
            assert want.reshape(-1)[10:12].tolist() == [0x3FC2, 0x3FC4] and want.reshape(-1)[4] == 0x7F80  # ties up and down, overflow

    for factor in (1.0, 1.5):
        for form, xin in (("16-byte", xd), ("one-element", xd.reshape(-1)[1:])):  # the second starts 2 bytes off: fused_bias_act_kernel
            y = torch.zeros_like(xin)
            lib.fused_bias_act_bf16(FF._p(xin), None, None, FF._p(y), xin.numel(), 1, 1, 3, 0, 1.0, factor, FF._st())
            full = torch.cat([xd.reshape(-1)[:1], y]) if form == "one-element" else y  # element 0, +inf, was not part of that call
            check(full.reshape(8, 4, 4), factor, f"fused_bias_act bf16 {form} x {factor}")
        tap = torch.full((1, 1), factor, device=dev, dtype=BF16)
        y = torch.zeros_like(xd)
        lib.upfirdn2d_bf16(FF._p(xd), FF._p(tap), FF._p(y), 8, 4, 4, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, FF._st())
        check(y, factor, f"upfirdn2d bf16 x {factor}")
