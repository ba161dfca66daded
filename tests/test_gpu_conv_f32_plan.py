"""GPU: the launchers of the fp32 convolution family follow the plan (csrc/conv_f32_plan.h).  One case per route and tile family the
training step uses: the entry is called through the C ABI, fmi_debug_f32_last_plan() must equal what fmi_conv2d_f32_plan planned for
the same descriptor and flags, and the result is compared with torch fp32 on the CPU within the bound of tests/test_gpu_p3.py (1e-5
relative, 1e-5 of the largest entry).  Each case's shape is the smallest of a fixed ladder that the query maps to the case's target --
searched on the host, not guessed.  The pinned table of tests/test_host_conv_f32_plan.py holds the instantiations; this file proves that
what is planned is what runs."""
import contextlib
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tools.golden import gen_conv_f32_plan as G

pytestmark = pytest.mark.gpu
NOUT = len(G.OUT_COLS)
LADDER = [(1, 4), (1, 8), (2, 8), (2, 16), (2, 32), (2, 64), (8, 64), (8, 128), (2, 256), (8, 256)]  # (N, H = W)
BASE = G.X_AL16 | G.W_AL16 | G.OUT_AL16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def FF():
    from face_mask_inpaint_amd import functional

    return functional


def _lib():
    from face_mask_inpaint_amd import _lib

    return _lib.lib()


def query(d, pass_, flags, lib=None):
    """lib: the library to ask (a tool that holds several); the process's otherwise"""
    out = (C.c_int * NOUT)()
    rc = (lib or _lib()).conv2d_f32_plan(C.byref(d), pass_, flags, C.cast(out, C.c_void_p))
    o = list(out)
    return rc, o, [dict(zip(G.LAUNCH_COLS, o[4 + 10 * p:14 + 10 * p])) for p in range(min(o[1], 4))]


def smallest(FF, pass_, flags, c, k, ksz, stride, want, hw=None, lib=None):
    """the smallest shape of the ladder whose plan satisfies want(out, launches)"""
    for n, h in LADDER:
        h, w = hw or (h, h)
        d, _, _ = FF.conv_desc(n, h, w, c, k, ksz, ksz, stride, ksz // 2)
        rc, o, ls = query(d, pass_, flags, lib)
        if rc == 0 and want(o, ls):
            return n, h, w
    raise AssertionError(f"no shape of the ladder reaches the target: pass {pass_} {c} -> {k} k{ksz} s{stride}")


def _split(FF, x):
    x3 = torch.full((x.numel() * 3,), float("nan"), device=x.device, dtype=torch.bfloat16)
    _lib().split3_f32(FF._p(x), C.c_void_p(x3.data_ptr()), None, x.numel() // x.shape[-1], x.shape[-1], 0, 0.0, FF._st())
    return x3


def close(got, ref):
    torch.testing.assert_close(got.cpu(), ref, rtol=1e-5, atol=1e-5 * float(ref.abs().max()))


def run_case(FF, dev, pass_, c, k, ksz, stride, want, w3=False, x3=False, y3=False, bias=False, det=False, hw=None):
    """plan on the host, run the entry, compare the record and the values"""
    lib = _lib()
    flags = BASE | (G.P3W if w3 else 0) | (G.P3X if x3 else 0) | (G.P3Y if y3 else 0) | (G.BIAS if bias else 0)
    ctx = FF.deterministic() if det else contextlib.nullcontext()
    with ctx:
        n, h, w = smallest(FF, pass_, flags, c, k, ksz, stride, want, hw)
        pad = ksz // 2
        g = torch.Generator().manual_seed(11 * c + k + h + pass_)
        wt_ = torch.randn(k, c, ksz, ksz, generator=g) / (c * ksz * ksz) ** 0.5
        (pw,) = FF.prepare_weights([(wt_.to(dev), None, None)])
        x = torch.randn(n, h, w, c, generator=g)
        xd = x.to(dev)
        b = torch.randn(k, generator=g) if bias else None
        d, oh, ow = FF.conv_desc(n, h, w, c, k, ksz, ksz, stride, pad)
        gy = torch.randn(n, oh, ow, k, generator=g)
        gyd = gy.to(dev)
        keep = []
        if w3:
            d.w3 = pw.w3[0 if pass_ == 0 else 1].data_ptr()
        if x3:
            keep.append(_split(FF, xd if pass_ != 1 else gyd))
            d.x3 = keep[-1].data_ptr()
        if y3:  # the weight gradient's second piece image: dy
            keep.append(_split(FF, gyd))
            d.y3 = keep[-1].data_ptr()
        rc, o, ls = query(d, pass_, flags)
        assert rc == 0 and want(o, ls), (o[:4], ls)
        before = lib.debug_f32_last_plan()
        xr, wr = x.permute(0, 3, 1, 2).clone().requires_grad_(True), wt_.clone().requires_grad_(True)
        yref = F.conv2d(xr, wr, b, stride=stride, padding=pad)
        if pass_ == 0:
            y = torch.full((n, oh, ow, k), float("nan"), device=dev)
            lib.conv2d_fwd_f32(C.byref(d), FF._p(xd), FF._p(pw.wf.detach()), FF._p(b.to(dev)) if bias else None, None, FF._p(y), 0, 1, 0, FF._st())
            got, ref = y, yref.detach().permute(0, 2, 3, 1)
        elif pass_ == 1:
            dx = torch.full((n, h, w, c), float("nan"), device=dev)
            lib.conv2d_dgrad_f32(C.byref(d), FF._p(gyd), FF._p(pw.wt), None, None, FF._p(dx), 1, 0, FF._st())
            yref.backward(gy.permute(0, 3, 1, 2))
            got, ref = dx, xr.grad.permute(0, 2, 3, 1)
        else:
            dw = torch.zeros(ksz * ksz, c, k, device=dev)
            db = torch.zeros(k, device=dev) if bias else None
            lib.conv2d_wgrad_f32(C.byref(d), FF._p(xd), FF._p(gyd), FF._p(dw), FF._p(db), 1, 0, FF._st())
            yref.backward(gy.permute(0, 3, 1, 2))
            got, ref = dw, wr.grad.permute(2, 3, 1, 0).reshape(ksz * ksz, c, k)
            if bias:
                close(db, gy.sum((0, 1, 2)))
        torch.cuda.synchronize()
        after = lib.debug_f32_last_plan()
        if o[2]:  # an early exit to the thin kernels: taken, and the record is left untouched
            assert not ls and after == before, (o[:4], before, after)
        else:
            assert after == ls[-1]["code"], (hex(after), hex(ls[-1]["code"]), ls)
        close(got, ref)
        return o, ls


def route_is(route, **kw):
    return lambda o, ls: bool(ls) and all(l["route"] == route for l in ls) and all(ls[-1][key] == v for key, v in kw.items())


FWD = [
    ("gemm_register_kernel", dict(c=3, k=8, ksz=1, want=route_is(G.GEMM, dma=0))),
    ("gemm_dma", dict(c=16, k=16, ksz=1, want=route_is(G.GEMM, dma=1))),
    ("gemm_w3", dict(c=16, k=16, ksz=1, w3=True, want=route_is(G.GEMM_W3))),
    ("gemm_p3", dict(c=16, k=16, ksz=1, w3=True, x3=True, want=route_is(G.GEMM_P3))),
    ("c3", dict(c=64, k=32, ksz=3, hw=(8, 8), want=route_is(G.C3))),
    ("c3_w3", dict(c=64, k=64, ksz=3, w3=True, want=route_is(G.C3_W3, tile=128064))),
    ("c3_p3_four_waves", dict(c=64, k=64, ksz=3, w3=True, x3=True, want=route_is(G.C3_P3, tile=128064))),
    ("c3_p3_eight_waves", dict(c=64, k=64, ksz=3, w3=True, x3=True, want=route_is(G.C3_P3, tile=256064))),
    ("split_with_init", dict(c=128, k=128, ksz=3, w3=True, want=lambda o, ls: ls and ls[0]["init"] == 1 and ls[0]["ksplit"] > 1)),
    ("thin_output_exit", dict(c=32, k=3, ksz=3, want=lambda o, ls: o[2] == G.THIN_OUT_ROUTE)),
    ("thin_input_exit", dict(c=3, k=32, ksz=3, want=lambda o, ls: o[2] == G.THIN_IN_ROUTE)),
]


@pytest.mark.parametrize("name,case", FWD, ids=[n for n, _ in FWD])
def test_forward_follows_the_plan(dev, FF, name, case):
    run_case(FF, dev, 0, stride=1, bias=True, **case)


ADJ = [
    ("c3", dict(c=32, k=64, ksz=3, stride=1, want=route_is(G.C3))),
    ("gemm_p3", dict(c=16, k=16, ksz=1, stride=1, w3=True, x3=True, want=route_is(G.GEMM_P3))),
    ("convt3x3_at_its_floor", dict(c=8, k=16, ksz=3, stride=2, w3=True, want=lambda o, ls: len(ls) == 1 and ls[0]["route"] == G.CONVT3X3)),
    ("stride2_shared_init", dict(c=512, k=512, ksz=3, stride=2, hw=(4, 4), want=lambda o, ls: o[3] & 1 and len(ls) == 4)),
    ("stride2_phases", dict(c=16, k=16, ksz=3, stride=2, want=lambda o, ls: not o[3] & 1 and len(ls) == 4 and ls[0]["route"] == G.GEMM)),
]


@pytest.mark.parametrize("name,case", ADJ, ids=[n for n, _ in ADJ])
def test_adjoint_follows_the_plan(dev, FF, name, case):
    o, ls = run_case(FF, dev, 1, **case)
    if name == "convt3x3_at_its_floor":
        assert ls[0]["grid_x"] == 32768 // 128  # N OH OW = 32768, the smallest map the route takes


WGRAD = [
    ("gemm_fused_bias", dict(c=16, k=16, ksz=3, bias=True, want=lambda o, ls: ls[0]["route"] == G.WGRAD_GEMM and o[3] & 2)),
    ("p3", dict(c=32, k=16, ksz=1, x3=True, y3=True, want=route_is(G.WGRAD_P3))),
    ("p3_3x3_narrow", dict(c=64, k=64, ksz=3, x3=True, y3=True, want=route_is(G.WGRAD_P3_3X3, tile=192064))),
    ("p3_3x3_wide", dict(c=64, k=128, ksz=3, x3=True, y3=True, want=route_is(G.WGRAD_P3_3X3, tile=192128))),
    ("reproducible_long_reduction", dict(c=16, k=16, ksz=3, det=True, want=lambda o, ls: ls[0]["route"] == G.WGRAD_GEMM and ls[0]["fl"] == 1 and ls[0]["chunk"] > 640)),
]


@pytest.mark.parametrize("name,case", WGRAD, ids=[n for n, _ in WGRAD])
def test_weight_gradient_follows_the_plan(dev, FF, name, case):
    run_case(FF, dev, 2, stride=1, **case)
