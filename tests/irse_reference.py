"""Closed-form float64 references of the IR-SE body operations (pSp encoder, modules/psp/encoders/helpers.py) and the seeded
inputs their tests share.  Plain torch on the CPU; no autograd.  test_host_irse_reference.py checks every function here against
torch autograd in float64, test_gpu_irse_kernels.py checks the HIP kernels against them.

Every function takes float64 copies of the operands a kernel sees (for a bf16 kernel: the bf16-rounded values, widened) and returns
a namespace with the outputs, every gradient, and for each of them ``<name>_mag``: the same expression with every term replaced by
its absolute value (for a reduction: the sum of |term|).  The tests build their error bounds from these magnitudes.

Layout is the library's: activations NHWC, per-channel parameters [C], grouped statistics [G, C]."""
from types import SimpleNamespace as NS

import torch


# ---------------------------------------------------------------------------------------------------------------------------
# grouped batch norm with a fused leaky activation
# ---------------------------------------------------------------------------------------------------------------------------
def _grp(t, groups):
    """[N, H, W, C] -> [G, rows, C]: group g is the g-th of G equal parts of the batch"""
    return t.reshape(groups, -1, t.shape[-1])


def bn_stats(x, eps, groups=1):
    """per group over (N / G, H, W): sums = (sum x, sum x^2), stats = (mean, rstd = 1 / sqrt(biased var + eps))"""
    xg = _grp(x, groups)
    cnt = xg.shape[1]
    s1, s2 = xg.sum(1), (xg * xg).sum(1)
    mean = s1 / cnt
    var = ((xg - mean[:, None]) ** 2).sum(1) / cnt  # centred: no E[x^2] - mean^2 cancellation in the reference itself
    return NS(count=cnt, mean=mean, var=var, rstd=1.0 / torch.sqrt(var + eps), s1=s1, s2=s2, s1_mag=xg.abs().sum(1), s2_mag=s2.clone())


def bn_apply(x, mean, rstd, gamma, beta, slope=1.0, groups=1):
    """pre = xhat gamma + beta, y = pre > 0 ? pre : slope pre, with the given (mean, rstd) [G, C]"""
    xg = _grp(x, groups)
    xh = (xg - mean[:, None]) * rstd[:, None]
    pre = xh * gamma + beta
    pre_mag = (xh * gamma).abs() + beta.abs()
    pos = pre > 0
    y = torch.where(pos, pre, slope * pre)
    y_mag = torch.where(pos, pre_mag, abs(slope) * pre_mag)
    return NS(xhat=xh.reshape(x.shape), pre=pre.reshape(x.shape), pre_mag=pre_mag.reshape(x.shape), y=y.reshape(x.shape),
              y_mag=y_mag.reshape(x.shape))


def bn_backward(x, g, mean, rstd, gamma, beta, slope, groups, mask, gadd=None):
    """the module's backward: g' = mask ? g : slope g;  gx = rstd gamma (g' - mean g' - xhat mean(g' xhat)) [+ gadd], the means per
    group;  dgamma = sum g' xhat, dbeta = sum g' over everything.  ``mask`` is an input (pre > 0 as the forward pass decided it).
    m1_abs / m2_abs [G, C] = mean |g'| and mean |g' xhat|: the magnitudes of the two inner reductions"""
    xg, gg, mk = _grp(x, groups), _grp(g, groups), _grp(mask, groups)
    xh = (xg - mean[:, None]) * rstd[:, None]
    gp = torch.where(mk, gg, slope * gg)
    m1, m2 = gp.mean(1), (gp * xh).mean(1)
    k = (rstd * gamma)[:, None]
    gx = k * (gp - m1[:, None] - xh * m2[:, None])
    gx_mag = k.abs() * (gp.abs() + m1.abs()[:, None] + xh.abs() * m2.abs()[:, None])
    if gadd is not None:
        gx = gx + _grp(gadd, groups)
        gx_mag = gx_mag + _grp(gadd, groups).abs()
    c = x.shape[-1]
    return NS(gx=gx.reshape(x.shape), gx_mag=gx_mag.reshape(x.shape), xhat=xh.reshape(x.shape), k_abs=(rstd * gamma).abs(),
              m1=m1, m2=m2, m1_abs=gp.abs().mean(1), m2_abs=(gp * xh).abs().mean(1),
              dgamma=(gp * xh).reshape(-1, c).sum(0), dgamma_mag=(gp * xh).abs().reshape(-1, c).sum(0),
              dbeta=gp.reshape(-1, c).sum(0), dbeta_mag=gp.abs().reshape(-1, c).sum(0))


def bn_train(x, gamma, beta, eps, groups=1, slope=1.0, g=None, gadd=None):
    """forward and (with g) backward in one call, on the reference's own statistics and its own mask pre > 0"""
    st = bn_stats(x, eps, groups)
    fw = bn_apply(x, st.mean, st.rstd, gamma, beta, slope, groups)
    bw = bn_backward(x, g, st.mean, st.rstd, gamma, beta, slope, groups, fw.pre > 0, gadd) if g is not None else None
    return st, fw, bw


def bn_running_update(rmean, rvar, nbt, mean, var_biased, count, momentum, mean_offset=None):
    """nn.BatchNorm2d bookkeeping of one training forward: momentum average of the mean (plus the optional offset) and of the UNBIASED
    variance; the counter.  count = 1: the unbiased factor is taken as 1 (the library's convention; torch divides by zero there)"""
    m = mean if mean_offset is None else mean + mean_offset
    unb = var_biased * (count / max(count - 1, 1))
    return NS(rmean=(1 - momentum) * rmean + momentum * m, rvar=(1 - momentum) * rvar + momentum * unb, nbt=nbt + 1,
              rmean_mag=(1 - momentum) * rmean.abs() + momentum * m.abs(), rvar_mag=(1 - momentum) * rvar.abs() + momentum * unb.abs(),
              var_unbiased=unb)


# ---------------------------------------------------------------------------------------------------------------------------
# element-wise operations, the SE gate, the global pool, the subsample, the frozen affine
# ---------------------------------------------------------------------------------------------------------------------------
def prelu(x, a, g=None):
    """y = x > 0 ? x : a[c] x;  gx = g (x > 0 ? 1 : a[c]);  ga[c] = sum g x [x <= 0]"""
    pos = x > 0
    r = NS(y=torch.where(pos, x, a * x))
    r.y_mag = r.y.abs()
    if g is not None:
        c = x.shape[-1]
        r.gx = torch.where(pos, g, a * g)
        r.gx_mag = r.gx.abs()
        t = torch.where(pos, torch.zeros_like(x), g * x)
        r.ga, r.ga_mag = t.reshape(-1, c).sum(0), t.abs().reshape(-1, c).sum(0)
    return r


def scale_channels(x, s, g=None, res=None):
    """x [N, P, C], s [N, C]: y = x s[n, c] (+ res);  gx = g s, gs[n, c] = sum_p g x, gres = g"""
    r = NS(y=x * s[:, None])
    r.y_mag = r.y.abs()
    if res is not None:
        r.y = r.y + res
        r.y_mag = r.y_mag + res.abs()
    if g is not None:
        r.gx = g * s[:, None]
        r.gx_mag = r.gx.abs()
        r.gs, r.gs_mag = (g * x).sum(1), (g * x).abs().sum(1)
        r.gres = g.clone()
    return r


def global_pool_pass(x, g_pool=None, g_pass=None):
    """x [N, H, W, C]: pooled [N, C] = mean over (H, W), and x handed on; the joined gradient gx = g_pass + g_pool[n, c] / (H W)"""
    n, h, w, c = x.shape
    r = NS(pooled=x.mean((1, 2)), pooled_mag=x.abs().mean((1, 2)))
    if g_pool is not None:
        b = (g_pool.reshape(n, 1, 1, c) / (h * w)).expand(n, h, w, c)
        r.gx = b.clone() if g_pass is None else g_pass + b
        r.gx_mag = b.abs() if g_pass is None else g_pass.abs() + b.abs()
    return r


def subsample(x, stride, g=None):
    """nn.MaxPool2d(1, stride): y = x[:, ::s, ::s]; the backward scatters g into zeros"""
    r = NS(y=x[:, ::stride, ::stride].contiguous())
    if g is not None:
        r.gx = torch.zeros_like(x)
        r.gx[:, ::stride, ::stride] = g
    return r


def channel_affine(x, scale, shift, g=None, g_pass=None):
    """y = x scale[c] + shift[c] with constant scale / shift; gx = g scale (+ g_pass, the gradient of x's other consumer)"""
    r = NS(y=x * scale + shift, y_mag=(x * scale).abs() + shift.abs())
    if g is not None:
        r.gx = g * scale
        r.gx_mag = r.gx.abs()
        if g_pass is not None:
            r.gx = r.gx + g_pass
            r.gx_mag = r.gx_mag + g_pass.abs()
    return r


# ---------------------------------------------------------------------------------------------------------------------------
# seeded inputs shared by the host and the GPU test
# ---------------------------------------------------------------------------------------------------------------------------
def bn_inputs(shape, groups, seed, dtype=torch.float32):
    """(x, gamma, beta, gy, gpass) on the CPU.  x = randn sigma_c + mu_c with per-channel sigma in [0.5, 2] and mu in [-2, 2]; with two
    groups the second half of the batch gets mu + 3 and 2 sigma, so statistics taken from the wrong group are O(1) wrong.  gamma has
    both signs, beta is O(1): the activation kink crosses every channel.  x / gy / gpass are rounded to ``dtype``"""
    n, h, w, c = shape
    gen = torch.Generator().manual_seed(seed)
    sigma = torch.rand(c, generator=gen) * 1.5 + 0.5
    mu = torch.rand(c, generator=gen) * 4 - 2
    x = torch.randn(shape, generator=gen) * sigma + mu
    if groups == 2:
        x[n // 2:] = x[n // 2:] * 2 - mu + 3  # (r sigma + mu) 2 - mu + 3 = r (2 sigma) + (mu + 3)
    gamma = (torch.rand(c, generator=gen) + 0.5) * (torch.randint(0, 2, (c,), generator=gen) * 2 - 1).float()
    beta = torch.rand(c, generator=gen) * 2 - 1
    gy = torch.randn(shape, generator=gen)
    gpass = torch.randn(shape, generator=gen)
    return x.to(dtype), gamma, beta, gy.to(dtype), gpass.to(dtype)


# Every (shape, groups) the GPU test runs BatchNorm at, fp32 and bf16, with its seed: test_host_irse_reference.py checks the mask
# condition for each of them.  rows = N H W / groups.
BN_F32_SHAPES = [(2, 3, 5, 12), (4, 9, 7, 64), (2, 33, 31, 64), (2, 8, 8, 1024), (1, 1, 1, 8), (1, 113, 64, 8), (2, 257, 128, 8),
                 (1, 512, 513, 4)]
BN_BF16_SHAPES = [(1, 1, 3, c) for c in (8, 64, 512, 1024)] + [(4, 9, 7, c) for c in (8, 64, 512, 1024)] + \
                 [(2, 113, 32, c) for c in (8, 64, 512, 1024)]  # rows 3, 252, 7232


def bn_groups(shape):
    return (1, 2) if shape[0] % 2 == 0 else (1,)


def bn_seed(shape, groups):
    n, h, w, c = shape
    return 1000 + 7 * n + 13 * h + 17 * w + c + 100000 * groups


def bn_kernel_order_pre_f32(x, mean, rstd, gamma, beta, groups):
    """pre in fp32, in the operation order of in_apply_kernel (csrc/norm.hip): ((x - mean) * rstd) * gamma + beta, every operand and
    every intermediate fp32.  The CPU stand-in for the kernel in the mask-condition check"""
    xg = _grp(x.float(), groups)
    pre = (xg - mean.float()[:, None]) * rstd.float()[:, None] * gamma.float() + beta.float()
    return pre.reshape(x.shape)
