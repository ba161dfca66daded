"""Closed-form float64 references of the operations in csrc/loss.hip (contextual-loss tails, l2norm_rows, lpips_layer, reduce_loss),
of dot / axpy (csrc/eltwise.hip) and of csrc/weights.hip (spectral-norm preparation, the packs, the weight gradient, Adam, Ranger),
and the seeded inputs their tests share.  Plain torch on the CPU; no autograd, no library import.  test_host_loss_reference.py checks
every function here against an independent float64 formulation, test_gpu_loss_weight_kernels.py checks the HIP kernels against them.

Every function takes float64 copies of the operands a kernel sees -- scalars included: a kernel argument declared `float` arrives
rounded to fp32, f32() below gives that value -- and returns a namespace with the outputs and for each of them ``<name>_mag``: the same
expression with every term replaced by its absolute value (for a reduction: the sum of |term|).  The tests build their error bounds
from these magnitudes.  Where a kernel produces an index the margin that decides whether the index is comparable is returned too."""
from types import SimpleNamespace as NS

import torch

F64 = torch.float64


def f32(x):
    """the value a `float` kernel argument holds"""
    return float(torch.tensor(float(x), dtype=torch.float32))


CX_EPS = f32(1e-5)   # the 1e-5f of cx_rows_kernel / cx_loss_kernel / cx_bwd_kernel
SN_EPS = f32(1e-12)  # the 1e-12f of wp_vnorm_kernel / wp_unorm_kernel


# ---------------------------------------------------------------------------------------------------------------------------
# contextual loss (modules/pluralistic_model/external_function.py:231-274), rows = N P
# ---------------------------------------------------------------------------------------------------------------------------
def channel_mean(y):
    """y [rows, C] -> mu[c] = mean over the rows"""
    return NS(mu=y.mean(0), mu_mag=y.abs().mean(0))


def cx_normalise(x, mu):
    """x [rows, C]: xn = (x - mu) / ||x - mu||, inv = 1 / ||x - mu||.  The sum of squares has positive terms only (it is its own
    magnitude), and the difference of two fp32 operands is one rounding of the exact difference: xn_mag = |xn|"""
    d = x - mu
    ss = (d * d).sum(1)
    nrm = torch.sqrt(ss)
    xn = d / nrm[:, None]
    return NS(xn=xn, xn_mag=xn.abs(), inv=1 / nrm, ss=ss)


def cx_normalise_bwd(g, xn, inv):
    """gx = (g - xn (xn . g)) inv"""
    dot = (g * xn).sum(1)
    gx = (g - xn * dot[:, None]) * inv[:, None]
    return NS(gx=gx, gx_mag=(g.abs() + xn.abs() * dot.abs()[:, None]) * inv.abs()[:, None], dot=dot, dot_mag=(g * xn).abs().sum(1))


def first_index_of(t, val, dim):
    """smallest index along dim at which t == val (val keeps dim)"""
    return (t == val).to(torch.uint8).argmax(dim)


def cx_rows(cos, h):
    """cos [..., P]: d = 1 - cos, dmin / argmin (smallest index among equal minima), arg = (1 - d / (dmin + 1e-5)) / h, w = exp(arg),
    rowsum = sum_j w, cx = w / rowsum;  gap = second smallest d - dmin (0 for an exact tie)"""
    d = 1 - cos
    two = torch.topk(d, 2, dim=-1, largest=False).values
    dmin = two[..., 0]
    den = dmin + CX_EPS
    q = d / den[..., None]
    arg = (1 - q) / h
    w = torch.exp(arg)
    rowsum = w.sum(-1)
    return NS(d=d, d_mag=1 + cos.abs(), dmin=dmin, argmin=first_index_of(d, dmin[..., None], -1), gap=two[..., 1] - two[..., 0], den=den,
              arg=arg, arg_mag=(1 + q.abs()) / abs(h), w=w, rowsum=rowsum, cx=w / rowsum[..., None])


def cx_cols(cx):
    """cx [N, P, P] -> colmax[n, j] = max_i cx[n, i, j], colarg = the first i that attains it, relgap = (largest - second) / largest"""
    two = torch.topk(cx, 2, dim=1).values
    colmax = two[:, 0]
    return NS(colmax=colmax, colarg=first_index_of(cx, colmax[:, None], 1), relgap=(two[:, 0] - two[:, 1]) / two[:, 0])


def cx_loss(colmax, scale):
    """colmax [N, P]: cx[n] = mean_j colmax, loss = scale mean_n -log(cx[n] + 1e-5)"""
    cx = colmax.mean(1)
    t = -torch.log(cx + CX_EPS)
    return NS(cx=cx, cx_mag=colmax.abs().mean(1), term=t, loss=scale * t.mean(), loss_mag=abs(scale) * t.abs().mean())


def cx_bwd(cxij, dmin, argmin, cos, colarg, cx, gscale, h, scale):
    """dL / dcos [N, P, P] of loss = scale mean_n -log(cx_n + 1e-5), times the upstream gscale (DESIGN.md "contextual loss, backward").
    argmin [N, P] and colarg [N, P] are INPUTS: the selections the forward made.
      G_ij = dL / dcx_ij = gcol_n where i == colarg[n, j], else 0;  gcol_n = -scale gscale / (N (cx_n + 1e-5) P)
      cx_ij = w_ij / S_i  =>  e_ij = w_ij dL / dw_ij = (G_ij - T_i) cx_ij,  T_i = sum_j G_ij cx_ij
      w_ij = exp((1 - d_ij / den_i) / h), den_i = dmin_i + 1e-5  =>  dL / dd_ij = -e_ij / (h den_i), dL / dden_i = M_i / (h den_i^2),
      M_i = sum_j e_ij d_ij, which reaches d at j = argmin_i;  dcos = -dd"""
    n, p, _ = cxij.shape
    gcol = -scale * gscale / (n * (cx + CX_EPS) * p)                       # [N]
    sel = colarg[:, None, :] == torch.arange(p)[None, :, None]            # [N, i, j]
    G = torch.where(sel, gcol[:, None, None].expand(n, p, p), torch.zeros((), dtype=F64))
    t = (G * cxij).sum(2)
    t_mag = (G * cxij).abs().sum(2)
    e = (G - t[..., None]) * cxij
    e_mag = (G.abs() + t.abs()[..., None]) * cxij.abs()
    d = 1 - cos
    den = dmin + CX_EPS
    m = (e * d).sum(2)
    m_mag = (e * d).abs().sum(2)
    dcos = e / (h * den[..., None])
    dcos_mag = e_mag / (abs(h) * den[..., None])
    corr = m / (h * den * den)
    idx = argmin.long()[..., None]
    dcos = dcos.scatter_add(2, idx, -corr[..., None])
    dcos_mag = dcos_mag.scatter_add(2, idx, corr.abs()[..., None])
    return NS(dcos=dcos, dcos_mag=dcos_mag, gcol=gcol, t=t, t_mag=t_mag, e=e, e_mag=e_mag, d=d, den=den, m=m, m_mag=m_mag, corr=corr)


def cx_inputs(n, p, c, seed):
    """x, y = |randn| [N, P, C] fp32 on the CPU"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, p, c, generator=g).abs(), torch.randn(n, p, c, generator=g).abs()


# (N, P, C) -> seed.  test_host_loss_reference.py establishes for each that the float64 chain excludes no row (two smallest d more than
# 2^-20 apart) and no column (two largest cx more than 1e-5 relative apart), so the kernels' indices are comparable everywhere.
CX_SHAPES = {(3, 64, 7): 3, (2, 257, 64): 2, (2, 300, 24): 0, (1, 520, 96): 1}
CX_H = 0.5
ROW_GAP_BAR, COL_GAP_BAR, EXCLUDED_MAX = 2.0 ** -20, 1e-5, 0.01


def cx_chain(x, y, h=CX_H, scale=1.0):
    """the float64 forward chain on x, y [N, P, C]: every intermediate the seven kernels produce"""
    n, p, c = x.shape
    mu = channel_mean(y.reshape(-1, c))
    xn = cx_normalise(x.reshape(-1, c), mu.mu)
    yn = cx_normalise(y.reshape(-1, c), mu.mu)
    cos = xn.xn.reshape(n, p, c) @ yn.xn.reshape(n, p, c).transpose(1, 2)
    rows = cx_rows(cos, h)
    cols = cx_cols(rows.cx)
    loss = cx_loss(cols.colmax, scale)
    return NS(mu=mu, xn=xn, yn=yn, cos=cos, rows=rows, cols=cols, loss=loss)


def cx_chain_bwd(ch, gscale=1.0, h=CX_H, scale=1.0):
    """x.grad of the chain [N, P, C]"""
    n, p, _ = ch.cos.shape
    c = ch.xn.xn.shape[1]
    bw = cx_bwd(ch.rows.cx, ch.rows.dmin, ch.rows.argmin, ch.cos, ch.cols.colarg, ch.loss.cx, gscale, h, scale)
    gxn = bw.dcos @ ch.yn.xn.reshape(n, p, c)
    return cx_normalise_bwd(gxn.reshape(-1, c), ch.xn.xn, ch.xn.inv).gx.reshape(n, p, c)


# ---------------------------------------------------------------------------------------------------------------------------
# LPIPS / ArcFace pieces, the sum losses, dot / axpy
# ---------------------------------------------------------------------------------------------------------------------------
def l2norm_rows(x, eps):
    """x [rows, C]: s = 1 / (||x|| + eps), y = x s"""
    ss = (x * x).sum(1)
    s = 1 / (torch.sqrt(ss) + eps)
    return NS(y=x * s[:, None], inv=s, ss=ss)


def l2norm_rows_bwd(g, y, inv, eps):
    """of the operands the backward kernel reads: n = 1 / s - eps, gx = s (g - y (g . y) (n + eps) / n); an all-zero row (n = 0,
    where autograd gives 0 / 0) gets s g, as the comment above l2norm_rows_bwd_kernel states"""
    dot = (g * y).sum(1)
    zero = (y == 0).all(1)
    n = torch.where(zero, torch.ones_like(inv), 1 / inv - eps)
    k = torch.where(zero, torch.zeros_like(dot), dot * (n + eps) / n)
    gx = inv[:, None] * (g - y * k[:, None])
    return NS(gx=gx, gx_mag=inv.abs()[:, None] * (g.abs() + y.abs() * k.abs()[:, None]), dot=dot, dot_mag=(g * y).abs().sum(1), k=k, n=n,
              zero=zero)


def lpips_layer(fx, fy, w, scale, gout=None):
    """fx, fy [pixels, C], w [C]: out = scale sum_p sum_c w[c] (fx - fy)^2;  gfx = 2 scale gout w (fx - fy) = -gfy"""
    d = fx - fy
    r = NS(out=scale * (w * d * d).sum(), out_mag=abs(scale) * (w.abs() * d * d).sum())
    if gout is not None:
        r.gfx = 2 * scale * gout * w * d
        r.gfy = -r.gfx
        r.g_mag = r.gfx.abs()
    return r


def reduce_loss(kind, a, b, c0, scale, gscale=None):
    """kind 0: scale sum |a - b|, 1: scale sum (a - b)^2, 2: scale sum (a - c0)^2;  ga = gscale scale sign(a - b) with sign(0) = 0
    (kind 0), 2 gscale scale (a - b or a - c0) (kinds 1, 2)"""
    d = a - (c0 if kind == 2 else b)
    t = d.abs() if kind == 0 else d * d
    r = NS(out=scale * t.sum(), out_mag=abs(scale) * t.sum())
    if gscale is not None:
        g = gscale * scale
        r.ga = torch.sign(d) * g if kind == 0 else 2 * d * g
        r.ga_mag = r.ga.abs()
    return r


def dot(a, b, scale):
    return NS(out=scale * (a * b).sum(), out_mag=abs(scale) * (a * b).abs().sum())


def axpy(a, s, b=None):
    """y = s a (+ b)"""
    y = s * a
    return NS(y=y if b is None else y + b, y_mag=y.abs() if b is None else y.abs() + b.abs())


# ---------------------------------------------------------------------------------------------------------------------------
# weights: spectral norm (external_function.py:30-41), packs, gradient
# ---------------------------------------------------------------------------------------------------------------------------
def spectral_iteration(w, u):
    """one power iteration on w [rows, width]: v_raw = W^T u, v = v_raw / (||v_raw|| + 1e-12), t = W v, u' = t / (||t|| + 1e-12),
    sigma = u' . t.  Every intermediate and its magnitude, for the error propagation of the GPU test"""
    aw = w.abs()
    v_raw = w.t() @ u
    nv = torch.sqrt((v_raw * v_raw).sum())
    v = v_raw / (nv + SN_EPS)
    t = w @ v
    nt = torch.sqrt((t * t).sum())
    un = t / (nt + SN_EPS)
    return NS(v_raw=v_raw, v_raw_mag=aw.t() @ u.abs(), nv=nv, v=v, t=t, t_mag=aw @ v.abs(), nt=nt, u=un, sigma=(un * t).sum(),
              sigma_mag=(un * t).abs().sum())


def spectral_prepare(w, u, v, iters=1):
    """w [rows, width] -> u', v', sigma, W / sigma after max(iters, 1) power iterations (v is overwritten before it is read: an
    argument for symmetry with the kernel's entry only)"""
    it = None
    for _ in range(max(int(iters), 1)):
        it = spectral_iteration(w, u)
        u = it.u
    return NS(u=it.u, v=it.v, sigma=it.sigma, weff=w / it.sigma, weff_mag=(w / it.sigma).abs(), last=it)


def spectral_grad(w, u, v, sigma, dweff):
    """gradient of W / sigma(W), sigma = u . (W v) with u, v constants: dW = dWeff / sigma - (sum dWeff o W) / sigma^2 u v^T; all
    operands [rows, width]"""
    dt = (dweff * w).sum()
    uv = torch.outer(u, v)
    coef = dt / (sigma * sigma)
    return NS(dw=dweff / sigma - coef * uv, dw_mag=(dweff / sigma).abs() + (coef * uv).abs(), dot=dt, dot_mag=(dweff * w).abs().sum(), uv=uv)


def pack_wf(weff, rows, c, taps):
    """[rows][C][taps] -> wf[tap][c][row]"""
    return weff.reshape(rows, c, taps).permute(2, 1, 0).contiguous()


def pack_wt(weff, rows, c, taps):
    """[rows][C][taps] -> wt[tap][row][c]"""
    return weff.reshape(rows, c, taps).permute(2, 0, 1).contiguous()


def unpack_wf(wf, rows, c, taps):
    """wf[tap][c][row] -> [rows, C taps]"""
    return wf.reshape(taps, c, rows).permute(2, 1, 0).reshape(rows, c * taps)


# ---------------------------------------------------------------------------------------------------------------------------
# optimisers
# ---------------------------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, step, lr, b1, b2, eps, wd, mv=None):
    """torch.optim.Adam's single-tensor order: g += wd p; m = lerp(m, g, 1 - b1); v = v b2 + (1 - b2) g g; denom = sqrt(v) / sqrt(1 -
    b2^step) + eps; p -= lr / (1 - b1^step) m / denom.  mv = (m, v): compute p from these moments (the kernel's own, already checked)
    instead of the reference's"""
    if wd != 0:
        g = g + wd * p
    m1 = m + (g - m) * (1 - b1)
    v1 = v * b2 + (1 - b2) * (g * g)
    mm, vv = (m1, v1) if mv is None else mv
    step_size = lr / (1 - b1 ** step)
    upd = step_size * (mm / (torch.sqrt(vv) / (1 - b2 ** step) ** 0.5 + eps))
    return NS(m=m1, m_mag=m.abs() + (g.abs() + m.abs()) * (1 - b1), v=v1, v_mag=v1.abs(), p=p - upd, p_mag=p.abs() + upd.abs())


def ranger_rectification(step, b1, b2, threshold=5):
    """ranger.py:145-162: (rectified, step_size) of a step count"""
    b2t = b2 ** step
    n_max = 2 / (1 - b2) - 1
    n_sma = n_max - 2 * step * b2t / (1 - b2t)
    if n_sma > threshold:
        return True, ((1 - b2t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) ** 0.5 / (1 - b1 ** step)
    return False, 1.0 / (1 - b1 ** step)


def row_mean(g, cols):
    """the gradient-centralisation mean of every row of g viewed as [rows, cols]"""
    g2 = g.reshape(-1, cols)
    return NS(mean=g2.mean(1), mean_mag=g2.abs().mean(1))


def ranger_step(p, g, m, v, slow, mean, lr, b1, b2, eps, wd, step_size, rectified, alpha, lookahead, mv=None):
    """the order written above ranger_kernel: g -= mean[row] (mean = None: no centralisation; otherwise [rows], g [rows, cols]);
    v = v b2 + (1 - b2) g g; m = m b1 + (1 - b1) g; p -= wd lr p; p -= step_size lr m / (sqrt(v) + eps) (rectified) or step_size lr m;
    every k-th step (lookahead) slow += alpha (p - slow), p = slow.  mv as in adam_step"""
    g_mag = g.abs()
    if mean is not None:
        g = g - mean[:, None]
        g_mag = g_mag + mean.abs()[:, None]
    v1 = v * b2 + (1 - b2) * g * g
    m1 = m * b1 + (1 - b1) * g
    mm, vv = (m1, v1) if mv is None else mv
    decay = wd * lr * p if wd != 0 else torch.zeros_like(p)
    upd = step_size * lr * (mm / (torch.sqrt(vv) + eps) if rectified else mm)
    pn = p - decay - upd
    p_mag = p.abs() + decay.abs() + upd.abs()
    r = NS(m=m1, m_mag=m.abs() * b1 + (1 - b1) * g_mag, v=v1, v_mag=v.abs() * b2 + (1 - b2) * g_mag * g_mag, slow=slow, slow_mag=slow.abs())
    if lookahead:
        r.slow = slow + alpha * (pn - slow)
        r.slow_mag = slow.abs() + alpha * (p_mag + slow.abs())
        pn, p_mag = r.slow, r.slow_mag
    r.p, r.p_mag = pn, p_mag
    return r
