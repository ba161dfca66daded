"""float64 references of the bf16 self-attention with K = Q and no scaling (csrc/attention_bf16.hip, csrc/attention_bwd_bf16.hip), written
out from the formulas and not taken from autograd:

    S = q q^T,  lse_i = log sum_j exp S_ij,  P = exp(S - lse),  o = P v
    delta_i = sum_c go_ic o_ic,  dP = go v^T,  dS = P o (dP - delta)
    gv = P^T go,  gq = dS q + dS^T q

``attention(q, v, go, rnd)`` takes a rounding function: with the identity it is the plain reference; with ``bf16`` it is the kernels'
arithmetic in float64 -- q, v, go and, as matrix operands only, P and dS are rounded once each; scores, exp, dP - delta, delta (from the
unrounded go and the o the forward STORED, which is itself rounded) and all sums are exact.  Shared by the host and the GPU tests."""
import torch

BF = torch.bfloat16


def identity(t):
    return t


def bf16(t):
    """round to nearest even onto the bf16 grid, result in float64 (the values here are far inside the fp32 range)"""
    return t.float().to(BF).double()


def attention(q, v, go, rnd=identity, lse=None, o_stored=None):
    """q [N,T,d], v / go [N,T,C] (any float dtype; computed in float64) -> dict of o, lse, delta, gq, gv (and go16 = rnd(go)).
    ``lse`` / ``o_stored``: use these instead of the ones computed here (a kernel-level check of the backward alone passes what the
    forward kernel wrote, so that the backward is compared on the operands it read)."""
    q, v, go = rnd(q.double()), rnd(v.double()), go.double()
    s = q @ q.transpose(1, 2)
    lse_own = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - (lse_own if lse is None else lse.double()).unsqueeze(-1))
    o = rnd(p) @ v                      # P is rounded as the operand of P v only
    o_st = rnd(o) if o_stored is None else o_stored.double()
    delta = (go * o_st).sum(-1)         # from the unrounded go
    go_r = rnd(go)
    dp = go_r @ v.transpose(1, 2) - delta.unsqueeze(-1)
    ds = p * dp                         # the unrounded P
    gv = rnd(p).transpose(1, 2) @ go_r
    gq = rnd(ds) @ q + rnd(ds).transpose(1, 2) @ q
    return dict(o=o_st, lse=lse_own, delta=delta, gq=gq, gv=gv, go16=go_r)


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def data(kind, n, t, d, c, seed):
    """fp32 q [n,t,d], v and go [n,t,c].  'moderate': q ~ 0.25 N(0,1) at d = 64 (0.35 at d = 32: the same |q|^2 ~ 4, so that the
    diagonal keeps 5 % .. 50 % of the mass against up to 511 other keys), a softmax that is neither uniform nor one-hot; 'peaked':
    q ~ N(0,1), so |q_i|^2 ~ d exceeds the forward's deferred-rescale threshold of 20 and the diagonal takes almost all of the mass."""
    g = torch.Generator().manual_seed(seed)
    scale = {"moderate": 0.25 * (64.0 / d) ** 0.5, "peaked": 1.0}[kind]
    q = torch.randn(n, t, d, generator=g) * scale
    v = torch.randn(n, t, c, generator=g)
    go = torch.randn(n, t, c, generator=g)
    return q, v, go


def mean_diagonal_probability(q):
    q = q.double()
    p = torch.softmax(q @ q.transpose(1, 2), dim=-1)
    return float(torch.diagonal(p, dim1=1, dim2=2).mean())


# the kernel-level cases of tests/test_gpu_attention_bf16_train.py, named here so that the host test can assert their input condition
KERNEL_SHAPES = [(n, t, d, c) for (d, c) in ((32, 128), (64, 256)) for t in (128, 384, 512) for n in (1, 3)]
PEAKED_SHAPE = (1, 384, 64, 256)


def case_seed(n, t, d, c):
    return 1000 + 7 * t + d + n
