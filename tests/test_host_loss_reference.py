"""CPU: every float64 reference of tests/loss_reference.py against an independent float64 formulation (autograd, torch.optim.Adam,
the oracle's contextual loss, the Ranger fixture), and the index conditions test_gpu_loss_weight_kernels.py relies on for its seeds."""
import os

import pytest
import torch

import loss_reference as R

F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _close(a, b, rtol=1e-11, atol=1e-13):
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol)


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


# ---- contextual loss ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 64, 7), (2, 300, 24)], ids=str)
def test_contextual_chain_against_the_oracle_in_double(shape):
    """loss and x.grad of the chained references = oracle.picnet_cpu.contextual_loss run in double (the oracle takes [N, C, H, W];
    P = P x 1).  R.CX_EPS is 1e-5 rounded to fp32 (what the kernels add), the oracle adds the double 1e-5: 2.5e-13 apart in absolute
    terms, on dmin = O(0.1) through the exponent's 1 / dmin^2 / h sensitivity -- hence 1e-8, not 1e-11"""
    from oracle import picnet_cpu as O

    n, p, c = shape
    x, y = (t.double() for t in R.cx_inputs(n, p, c, R.CX_SHAPES[shape]))
    xo = x.transpose(1, 2).reshape(n, c, p, 1).clone().requires_grad_(True)
    lo = O.contextual_loss(xo, y.transpose(1, 2).reshape(n, c, p, 1), R.CX_H)
    lo.backward()
    ch = R.cx_chain(x, y, R.CX_H, 1.0)
    _close(ch.loss.loss, lo.detach(), rtol=1e-8)
    gx = R.cx_chain_bwd(ch, 1.0, R.CX_H, 1.0)
    _close(gx, xo.grad.reshape(n, c, p).transpose(1, 2), rtol=1e-7, atol=1e-9 * float(xo.grad.abs().max()))
    # scale and the upstream gradient are linear factors
    _close(R.cx_chain_bwd(ch, 0.75, R.CX_H, 3.0), gx * 2.25, rtol=1e-12)


def test_cx_bwd_against_autograd_with_the_selections_held():
    """cx_bwd alone: autograd through rows -> cols -> loss as functions of cos, on a small random cosine matrix"""
    cos = (torch.rand(2, 9, 9, generator=torch.Generator().manual_seed(4), dtype=F64) * 1.6 - 0.8).requires_grad_(True)
    d = 1 - cos
    dmin = d.min(2).values
    w = torch.exp((1 - d / (dmin[..., None] + R.CX_EPS)) / 0.3)
    cx = w / w.sum(2, keepdim=True)
    cxn = cx.max(1).values.mean(1)
    loss = 1.7 * (-torch.log(cxn + R.CX_EPS)).mean()
    loss.backward()
    rows = R.cx_rows(cos.detach(), 0.3)
    cols = R.cx_cols(rows.cx)
    ls = R.cx_loss(cols.colmax, 1.7)
    _close(ls.loss, loss.detach())
    _close(rows.cx, cx.detach())
    bw = R.cx_bwd(rows.cx, rows.dmin, rows.argmin, cos.detach(), cols.colarg, ls.cx, 1.0, 0.3, 1.7)
    _close(bw.dcos, cos.grad, rtol=1e-10, atol=1e-13)
    assert bool((bw.dcos.abs() <= bw.dcos_mag * (1 + 1e-12)).all())


def test_ties_take_the_smallest_index():
    cos = torch.zeros(1, 2, 300, dtype=F64)
    cos[0, 0, 259] = cos[0, 0, 3] = 0.5
    cos[0, 1, 7] = 0.25
    r = R.cx_rows(cos, 0.5)
    assert r.argmin.tolist() == [[3, 7]] and r.gap[0, 0] == 0 and r.gap[0, 1] == 0.25
    cx = torch.rand(1, 5, 4, generator=torch.Generator().manual_seed(1), dtype=F64)
    cx[0, 1, 2] = cx[0, 4, 2] = 2.0
    c = R.cx_cols(cx)
    assert int(c.colarg[0, 2]) == 1 and c.relgap[0, 2] == 0 and bool((c.relgap[0, [0, 1, 3]] > 0).all())


def _margins(shape, seed):
    n, p, c = shape
    x, y = (t.double() for t in R.cx_inputs(n, p, c, seed))
    ch = R.cx_chain(x, y)
    return ch, ch.rows.gap, ch.cols.relgap


@pytest.mark.parametrize("shape", list(R.CX_SHAPES), ids=str)
def test_index_conditions_of_the_chosen_seeds(shape):
    """for the reference alone: at most 1 % of the rows / columns fall under the bars below which the GPU test does not compare an
    index -- for the chosen seeds none at all, with the smallest margins recorded here; and some row's arg-min lies at 256 or beyond
    wherever P > 256 (cx_bwd's fix-up then corrects an entry another thread wrote)"""
    ch, gap, relgap = _margins(shape, R.CX_SHAPES[shape])
    assert float((gap <= R.ROW_GAP_BAR).double().mean()) <= R.EXCLUDED_MAX and float((relgap <= R.COL_GAP_BAR).double().mean()) <= R.EXCLUDED_MAX
    floor = {(3, 64, 7): (7.0e-4, 1.0e-3), (2, 257, 64): (6.0e-5, 2.0e-4), (2, 300, 24): (4.0e-5, 2.5e-4), (1, 520, 96): (8.0e-5, 8.0e-5)}[shape]
    assert float(gap.min()) > floor[0] and float(relgap.min()) > floor[1], (float(gap.min()), float(relgap.min()))
    if shape[1] > 256:
        assert int((ch.rows.argmin >= 256).sum()) > 0


def test_index_condition_at_the_production_shape():
    _, gap, relgap = _margins((1, 784, 96), 1)
    assert float((gap <= R.ROW_GAP_BAR).double().mean()) <= R.EXCLUDED_MAX and float(relgap.min()) > 2.0e-5


def test_cx_normalise_backward_against_autograd():
    x = _rand(11, 70, seed=5).requires_grad_(True)
    mu, g = _rand(70, seed=6), _rand(11, 70, seed=7)
    d = x - mu
    xn = d / d.norm(dim=1, keepdim=True)
    xn.backward(g)
    f = R.cx_normalise(x.detach(), mu)
    _close(f.xn, xn.detach())
    _close(f.inv, 1 / d.detach().norm(dim=1))
    _close(R.cx_normalise_bwd(g, f.xn, f.inv).gx, x.grad)
    _close(R.channel_mean(x.detach()).mu, x.detach().sum(0) / 11)


# ---- l2norm, lpips, reduce_loss, dot, axpy -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 1e-10])
def test_l2norm_rows_against_autograd(eps):
    x = _rand(6, 96, seed=8)
    if eps:
        x[2] = 0
    g = _rand(6, 96, seed=9)
    xa = x.clone().requires_grad_(True)
    y = xa / (xa.norm(dim=1, keepdim=True) + eps)
    y.backward(g)
    f = R.l2norm_rows(x, eps)
    _close(f.y, y.detach())
    b = R.l2norm_rows_bwd(g, f.y, f.inv, eps)
    live = torch.ones(6, dtype=torch.bool)
    if eps:
        live[2] = False
        assert bool(b.zero[2]) and not bool(b.zero[live].any())
        _close(b.gx[2], g[2] / eps)  # s g with s = 1 / eps ...
        _close(b.gx[2], xa.grad[2])  # ... which is also what torch's norm (subgradient 0 at the origin) hands back
    _close(b.gx[live], xa.grad[live], rtol=1e-6 if eps else 1e-11)  # n = 1 / s - eps recovers ||x|| to eps u64 / ||x||^2 only


def test_lpips_layer_against_autograd():
    fx, fy = _rand(35, 20, seed=10).requires_grad_(True), _rand(35, 20, seed=11).requires_grad_(True)
    w = _rand(20, seed=12)
    out = 0.37 * (w * (fx - fy) ** 2).sum()
    (out * 1.9).backward()
    r = R.lpips_layer(fx.detach(), fy.detach(), w, 0.37, 1.9)
    _close(r.out, out.detach())
    _close(r.gfx, fx.grad)
    _close(r.gfy, fy.grad)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_reduce_loss_against_autograd(kind):
    a, b = _rand(1938, seed=13), _rand(1938, seed=14)
    a[:5] = b[:5]
    aa = a.clone().requires_grad_(True)
    d = aa - (0.9 if kind == 2 else b)
    out = 0.01 * (d.abs() if kind == 0 else d * d).sum()
    (out * 1.3).backward()
    r = R.reduce_loss(kind, a, b, 0.9, 0.01, 1.3)
    _close(r.out, out.detach())
    _close(r.ga, aa.grad)
    if kind == 0:
        assert bool((r.ga[:5] == 0).all())
    _close(R.dot(a, b, 0.5).out, 0.5 * torch.dot(a, b))
    _close(R.axpy(a, 0.3, b).y, torch.add(b, a, alpha=0.3))
    _close(R.axpy(a, 0.3).y, a * 0.3)


# ---- weights -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 3])
def test_spectral_prepare_and_grad_against_autograd(iters):
    """the written-out power iteration of external_function.py:30-41 (state under no_grad, sigma = u . W v differentiable through W
    only) and autograd through W / sigma"""
    rows, c, taps = 12, 5, 4
    w = _rand(rows, c * taps, seed=15).requires_grad_(True)
    u0, v0 = _rand(rows, seed=16), _rand(c * taps, seed=17)
    u, v = u0 / u0.norm(), v0 / v0.norm()
    with torch.no_grad():
        for _ in range(iters):
            v = torch.mv(w.t(), u)
            v = v / (v.norm() + 1e-12)
            u = torch.mv(w, v)
            u = u / (u.norm() + 1e-12)
    sigma = u.dot(w.mv(v))
    weff = w / sigma
    dweff = _rand(rows, c * taps, seed=18)
    weff.backward(dweff)
    sp = R.spectral_prepare(w.detach(), u0 / u0.norm(), v0 / v0.norm(), iters)
    _close(sp.u, u)
    _close(sp.v, v)
    _close(sp.sigma, sigma.detach())
    _close(sp.weff, weff.detach())
    _close(R.spectral_grad(w.detach(), sp.u, sp.v, sp.sigma, dweff).dw, w.grad)
    wf, wt = R.pack_wf(sp.weff, rows, c, taps), R.pack_wt(sp.weff, rows, c, taps)
    w4 = sp.weff.reshape(rows, c, taps)
    assert wf.shape == (taps, c, rows) and wt.shape == (taps, rows, c)
    assert wf[3, 2, 7] == w4[7, 2, 3] and wt[3, 7, 2] == w4[7, 2, 3]
    assert torch.equal(R.unpack_wf(wf, rows, c, taps), sp.weff)


# ---- optimisers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_step_against_torch_optim(wd):
    p0 = _rand(257, seed=19)
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, foreach=False)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for step in range(1, 6):
        g = _rand(257, seed=20 + step)
        pt.grad = g.clone()
        opt.step()
        r = R.adam_step(p, g, m, v, step, 1e-2, 0.9, 0.999, 1e-8, wd)
        p, m, v = r.p, r.m, r.v
        _close(p, pt.detach(), rtol=1e-12, atol=1e-15)
        _close(m, opt.state[pt]["exp_avg"], rtol=1e-12, atol=1e-15)
        _close(v, opt.state[pt]["exp_avg_sq"], rtol=1e-12, atol=1e-18)
        assert bool(((r.p - r.p_mag).abs() <= 2 * r.p_mag).all())


def test_ranger_step_against_the_fixture():
    """13 steps on the gradients of tests/golden/ranger.pt in double, against the parameters the reference's (fp32) optimiser
    produced, at the tolerance test_gpu_kernels.py::test_ranger_against_reference holds the kernel to"""
    fx = torch.load(os.path.join(GOLDEN, "ranger.pt"), map_location="cpu", weights_only=False)
    cfg = dict(lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=0)
    cfg.update(fx["cfg"])
    b1, b2 = cfg["betas"]
    ps = [p.double() for p in fx["p0"]]
    ms, vs, slows = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps], [p.clone() for p in ps]
    seen = set()
    for step, (gs, want) in enumerate(zip(fx["grads"], fx["params"]), 1):
        rect, ss = R.ranger_rectification(step, b1, b2, cfg["N_sma_threshhold"])
        look = step % cfg["k"] == 0
        seen.add((rect, look))
        for i, g in enumerate(gs):
            g = g.double()
            gc = g.dim() > 1
            cols = g.numel() // g.shape[0] if gc else g.numel()
            g2 = g.reshape(-1, cols)
            mean = R.row_mean(g, cols).mean if gc else None
            r = R.ranger_step(ps[i].reshape(-1, cols), g2, ms[i].reshape(-1, cols), vs[i].reshape(-1, cols), slows[i].reshape(-1, cols), mean,
                              cfg["lr"], b1, b2, cfg["eps"], cfg["weight_decay"], ss, rect, cfg["alpha"], look)
            ps[i], ms[i], vs[i], slows[i] = (t.reshape(g.shape) for t in (r.p, r.m, r.v, r.slow))
            torch.testing.assert_close(ps[i].float(), want[i], rtol=2e-5, atol=2e-6, msg=lambda s, i=i, step=step: f"step {step} tensor {i}: {s}")
    assert {r for r, _ in seen} == {False, True} and {l for _, l in seen} == {False, True}  # both branches, and a Lookahead sync
