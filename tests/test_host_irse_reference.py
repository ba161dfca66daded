"""CPU only: the float64 references of tests/irse_reference.py against torch autograd in float64 (rtol 1e-12), and the mask
condition the GPU test (test_gpu_irse_kernels.py) relies on, for every BatchNorm shape and seed that test uses."""
import pytest
import torch
import torch.nn.functional as F

import irse_reference as R

F64 = torch.float64
RT = dict(rtol=1e-12, atol=1e-12)


def _close(a, b):
    torch.testing.assert_close(a, b, **RT)


def _r(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=F64)


@pytest.mark.parametrize("shape,groups", [((4, 3, 5, 8), 1), ((4, 3, 5, 8), 2), ((2, 7, 2, 12), 1), ((2, 7, 2, 12), 2)])
@pytest.mark.parametrize("slope", [1.0, 0.0, 0.2])
@pytest.mark.parametrize("with_gadd", [False, True])
def test_batch_norm_reference(shape, groups, slope, with_gadd):
    x, gamma, beta, gy, gpass = (t.double() for t in R.bn_inputs(shape, groups, 5))
    eps = 1e-5
    st, fw, bw = R.bn_train(x, gamma, beta, eps, groups, slope, gy, gpass if with_gadd else None)
    xa, ga, ba = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    ys = []
    for xc in xa.chunk(groups, 0):  # F.batch_norm wants NCHW
        yc = F.batch_norm(xc.permute(0, 3, 1, 2), None, None, ga, ba, True, 0.0, eps)
        ys.append(F.leaky_relu(yc, slope).permute(0, 2, 3, 1))
    y = torch.cat(ys, 0)
    out = (y * gy).sum() + ((xa * gpass).sum() if with_gadd else 0)
    out.backward()
    _close(fw.y, y.detach())
    _close(bw.gx, xa.grad)
    _close(bw.dgamma, ga.grad)
    _close(bw.dbeta, ba.grad)
    xg = x.reshape(groups, -1, shape[-1])
    _close(st.mean, xg.mean(1))
    _close(st.rstd, 1 / torch.sqrt(xg.var(1, unbiased=False) + eps))
    _close(st.s1, xg.sum(1))
    _close(st.s2, (xg * xg).sum(1))
    # magnitudes dominate their values
    assert (fw.y_mag >= fw.y.abs() * (1 - 1e-12)).all() and (bw.gx_mag >= bw.gx.abs() * (1 - 1e-12)).all()
    assert (bw.dgamma_mag >= bw.dgamma.abs() * (1 - 1e-12)).all() and (st.s1_mag >= st.s1.abs()).all()


@pytest.mark.parametrize("shape", [(3, 2, 5, 4), (2, 4, 3, 7)])
@pytest.mark.parametrize("momentum", [0.1, 0.37])
def test_running_update_reference(shape, momentum):
    gen = torch.Generator().manual_seed(11)
    c = shape[-1]
    x = _r(gen, *shape) * 1.5 + 0.7
    bn = torch.nn.BatchNorm2d(c, eps=1e-5, momentum=momentum).double()
    bn.running_mean.copy_(_r(gen, c))
    bn.running_var.copy_(torch.rand(c, generator=gen, dtype=F64) + 0.5)
    rm, rv, nbt = bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()
    st = R.bn_stats(x, 1e-5)
    for _ in range(2):
        bn(x.permute(0, 3, 1, 2))
        u = R.bn_running_update(rm, rv, nbt, st.mean[0], st.var[0], st.count, momentum)
        rm, rv, nbt = u.rmean, u.rvar, u.nbt
    _close(rm, bn.running_mean)
    _close(rv, bn.running_var)
    assert int(nbt) == int(bn.num_batches_tracked) == 2
    off = _r(gen, c)
    u = R.bn_running_update(rm, rv, nbt, st.mean[0], st.var[0], st.count, momentum, off)
    _close(u.rmean, (1 - momentum) * rm + momentum * (x.reshape(-1, c) + off).mean(0))
    _close(u.rvar, (1 - momentum) * rv + momentum * x.reshape(-1, c).var(0, unbiased=True))


@pytest.mark.parametrize("shape", [(2, 3, 5, 8), (1, 4, 1, 6)])
def test_prelu_reference(shape):
    gen = torch.Generator().manual_seed(3)
    x, g = _r(gen, *shape), _r(gen, *shape)
    x.view(-1)[::5] = 0.0
    a = torch.rand(shape[-1], generator=gen, dtype=F64) * 0.5
    a[0], a[1] = -0.3, 0.0
    r = R.prelu(x, a, g)
    xa, aa = x.clone().requires_grad_(True), a.clone().requires_grad_(True)
    y = F.prelu(xa.permute(0, 3, 1, 2), aa).permute(0, 2, 3, 1)
    (y * g).sum().backward()
    _close(r.y, y.detach())
    _close(r.gx, xa.grad)
    _close(r.ga, aa.grad)


@pytest.mark.parametrize("n,p,c", [(3, 7, 8), (1, 5, 6)])
def test_scale_channels_reference(n, p, c):
    gen = torch.Generator().manual_seed(4)
    x, s, res, g = _r(gen, n, p, c), _r(gen, n, c), _r(gen, n, p, c), _r(gen, n, p, c)
    for with_res in (False, True):
        r = R.scale_channels(x, s, g, res if with_res else None)
        xa, sa, ra = (t.clone().requires_grad_(True) for t in (x, s, res))
        y = xa * sa[:, None] + (ra if with_res else 0)
        (y * g).sum().backward()
        _close(r.y, y.detach())
        _close(r.gx, xa.grad)
        _close(r.gs, sa.grad)
        if with_res:
            assert torch.equal(r.gres, ra.grad)


@pytest.mark.parametrize("shape", [(2, 4, 4, 8), (3, 3, 5, 6)])
def test_global_pool_reference(shape):
    gen = torch.Generator().manual_seed(5)
    n, h, w, c = shape
    x, gp, gx_pass = _r(gen, *shape), _r(gen, n, c), _r(gen, *shape)
    r = R.global_pool_pass(x, gp, gx_pass)
    xa = x.clone().requires_grad_(True)
    pooled = xa.mean((1, 2))
    ((pooled * gp).sum() + (xa * gx_pass).sum()).backward()
    _close(r.pooled, pooled.detach())
    _close(r.gx, xa.grad)
    xb = x.clone().requires_grad_(True)
    (xb.mean((1, 2)) * gp).sum().backward()
    _close(R.global_pool_pass(x, gp).gx, xb.grad)


@pytest.mark.parametrize("shape,stride", [((2, 7, 9, 4), 2), ((1, 10, 7, 3), 3)])
def test_subsample_reference(shape, stride):
    gen = torch.Generator().manual_seed(6)
    x = _r(gen, *shape)
    xa = x.clone().requires_grad_(True)
    y = xa[:, ::stride, ::stride]
    g = _r(gen, *y.shape)
    (y * g).sum().backward()
    r = R.subsample(x, stride, g)
    assert torch.equal(r.y, y.detach()) and torch.equal(r.gx, xa.grad)
    assert torch.equal(r.y, F.max_pool2d(x.permute(0, 3, 1, 2), 1, stride).permute(0, 2, 3, 1))


@pytest.mark.parametrize("shape", [(2, 3, 5, 8), (1, 4, 1, 6)])
def test_channel_affine_reference(shape):
    gen = torch.Generator().manual_seed(7)
    c = shape[-1]
    x, g, gpass, scale, shift = _r(gen, *shape), _r(gen, *shape), _r(gen, *shape), _r(gen, c), _r(gen, c)
    xa = x.clone().requires_grad_(True)
    y = xa * scale + shift
    ((y * g).sum() + (xa * gpass).sum()).backward()
    r = R.channel_affine(x, scale, shift, g, gpass)
    _close(r.y, y.detach())
    _close(r.gx, xa.grad)
    _close(R.channel_affine(x, scale, shift, g).gx, g * scale)


# ---- the mask condition --------------------------------------------------------------------------------------------------
# The GPU test hands the backward reference the kernel's own activation mask (y_kernel > 0).  That is sound as long as the kernel's
# fp32 pre and the float64 pre can differ in sign only where the float64 pre is at rounding distance from 0.  Here an fp32 CPU
# evaluation in the kernel's operation order stands in for the kernel; statistics are the float64 ones rounded to fp32, which is what the
# apply kernel reads.  Observed on this reference side, over all cases below: 0 disagreeing elements of 26 791 536 (the inputs are
# continuous; the fp32 pre is within 4 u32 (|xhat gamma| + |beta|) of the float64 one, so a sign can differ only that close to 0).
_MASK_CASES = [(s, g, torch.float32) for s in R.BN_F32_SHAPES for g in R.bn_groups(s)] + \
              [(s, g, torch.bfloat16) for s in R.BN_BF16_SHAPES for g in R.bn_groups(s)]


@pytest.mark.parametrize("shape,groups,dtype", _MASK_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_mask_condition(shape, groups, dtype):
    x, gamma, beta, _, _ = R.bn_inputs(shape, groups, R.bn_seed(shape, groups), dtype)
    eps = float(torch.tensor(1e-5, dtype=torch.float32))
    st = R.bn_stats(x.double(), eps, groups)
    mean32, rstd32 = st.mean.float(), st.rstd.float()
    pre32 = R.bn_kernel_order_pre_f32(x, mean32, rstd32, gamma, beta, groups)
    fw = R.bn_apply(x.double(), mean32.double(), rstd32.double(), gamma.double(), beta.double(), 1.0, groups)
    bad = (pre32 > 0) != (fw.pre > 0)
    assert int(bad.sum()) <= 1e-4 * x.numel()
    assert (fw.pre.abs()[bad] <= 2.0 ** -20 * fw.pre_mag[bad]).all()
