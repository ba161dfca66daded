"""CPU: the stride-1 ResBlock pair  conv3x3(x1, W1) + conv1x1(x2, W2) + b1 + b2  (csrc/conv_pair.h) without a GPU.

* the float64 reference the GPU tests use (tests/resblock_pair_reference.py) against torch.nn.functional;
* the eligibility and plan queries (fmi_conv2d_pair_supported / _ksplit) and the refusals of the entries, on the g++ -DFMI_HOST_EMU build
  of csrc/conv.hip, where the second-source loaders and the two-destination epilogue are the code the GPU kernels run
  (tests/test_host_geometry.py), and the forward / weight gradient of that build against the float64 reference;
* the Python wrapper's wiring: FF.conv2d_pair takes the fused Function only where conv2d_pair_ok says so and otherwise issues the 1x1
  convolution and the 3x3 one with its result as residual."""
import ctypes as C
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

import resblock_pair_reference as R
from face_mask_inpaint_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face_mask_inpaint_amd", "csrc")
OK, BAD_ARG, UNSUPPORTED = 0, 1, 2


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(ROOT, "oracle", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libfmi_emu_pair.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-DFMI_HOST_EMU", "-x", "c++",
                           os.path.join(CSRC, "conv.hip"), os.path.join(CSRC, "gemm.hip"), "-o", so])
    lib = C.CDLL(so)
    for name in ("fmi_conv2d_pair_fwd_f32", "fmi_conv2d_pair_wgrad_f32"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = _lib.SIGNATURES[name], C.c_int
    for name in ("fmi_conv2d_pair_supported", "fmi_conv2d_pair_routed", "fmi_conv2d_pair_ksplit"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = _lib.PREDICATES[name], C.c_int
    return lib


def ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else None


def desc(n, h, w, c, k, kh=3, stride=1, pad=1, pad_mode=0):
    oh = (h + 2 * pad - kh) // stride + 1
    ow = (w + 2 * pad - kh) // stride + 1
    return _lib.ConvDesc(n, h, w, c, oh, ow, k, c, k, kh, kh, stride, pad, pad_mode, 1)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_reference_matches_torch_functional(shape):
    x1, x2, w1, w2, b1, b2, _ = R.make(*shape)
    d = [v.double() for v in (x1, x2, w1, w2, b1, b2)]
    y = R.pair64(*d)
    ref = (F.conv2d(d[0].permute(0, 3, 1, 2), d[2], d[4], padding=1) + F.conv2d(d[1].permute(0, 3, 1, 2), d[3], d[5])).permute(0, 2, 3, 1)
    torch.testing.assert_close(y, ref, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.pair64(d[0], d[1], d[2], d[3], None, None), ref - d[4] - d[5], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_emu_forward_and_weight_gradient(emu, shape, bias):
    n, h, w, c1, c2, k = shape
    x1, x2, w1, w2, b1, b2, gy = R.make(*shape)
    if not bias:
        b1 = b2 = None
    y64, dw1, dw2, db, _, _ = R.reference(x1, x2, w1, w2, b1, b2, gy)
    d = desc(n, h, w, c1, k)
    assert emu.fmi_conv2d_pair_supported(C.byref(d), c2) == 1
    wf1, wf2 = R.pack(w1), R.pack(w2)
    for act in (0, 2):
        y = torch.full((n, h, w, k), float("nan"))
        assert emu.fmi_conv2d_pair_fwd_f32(C.byref(d), ptr(x1), ptr(x2), c2, ptr(wf1), ptr(wf2), None, ptr(b1), ptr(b2), ptr(y), act, None) == OK
        torch.testing.assert_close(y.double(), y64.clamp_min(0) if act else y64, rtol=1e-4, atol=1e-5)
    g1, g2 = torch.zeros(9, c1, k), torch.zeros(1, c2, k)
    gb = torch.zeros(k) if bias else None
    assert emu.fmi_conv2d_pair_wgrad_f32(C.byref(d), ptr(x1), ptr(x2), c2, ptr(gy), ptr(g1), ptr(g2), ptr(gb), None) == OK
    tol = R.dw_tol(n, h, w)
    torch.testing.assert_close(g1.double(), dw1, rtol=1e-4, atol=tol)
    torch.testing.assert_close(g2.double(), dw2, rtol=1e-4, atol=tol)
    if bias:
        torch.testing.assert_close(gb.double(), db, rtol=1e-4, atol=tol)


def test_eligibility_and_refusals(emu):
    n, h, w, c1, c2, k = 1, 4, 4, 32, 16, 32
    x1, x2, w1, w2, b1, b2, gy = R.make(n, h, w, c1, c2, k)
    wf1, wf2 = R.pack(w1), R.pack(w2)
    y = torch.zeros(n, h, w, k)
    g1, g2 = torch.zeros(9, c1, k), torch.zeros(1, c2, k)

    def fwd(d, c2_=c2, x1_=None, x2_=None, y_=None):
        return emu.fmi_conv2d_pair_fwd_f32(C.byref(d), x1_ or ptr(x1), x2_ or ptr(x2), c2_, ptr(wf1), ptr(wf2), None, ptr(b1), ptr(b2), y_ or ptr(y), 0, None)

    def wgrad(d, c2_=c2, x2_=None):
        return emu.fmi_conv2d_pair_wgrad_f32(C.byref(d), ptr(x1), x2_ or ptr(x2), c2_, ptr(gy), ptr(g1), ptr(g2), None, None)

    good = desc(n, h, w, c1, k)
    assert emu.fmi_conv2d_pair_supported(C.byref(good), c2) == 1 and fwd(good) == OK and wgrad(good) == OK
    assert emu.fmi_conv2d_pair_ksplit(C.byref(good), c2, 0) == 1  # the emulation never splits
    y.fill_(7.0)
    for d, cc in ((desc(n, h, w, c1, k, stride=2), c2),             # stride 2
                  (desc(n, h, w, c1, k, pad_mode=1), c2),           # reflect padding
                  (good, 8), (good, 24),                            # C2 % 16 != 0
                  (desc(n, h, w, 24, k), c2),                       # C1 % 16 != 0
                  (desc(n, h, w, c1, k, kh=1, pad=0), c2)):         # not a 3x3
        assert emu.fmi_conv2d_pair_supported(C.byref(d), cc) == 0
        assert emu.fmi_conv2d_pair_routed(C.byref(d), cc) == 0
        assert emu.fmi_conv2d_pair_ksplit(C.byref(d), cc, 0) == 0
        assert fwd(d, cc) == UNSUPPORTED and wgrad(d, cc) == UNSUPPORTED
    # a pointer off 16-byte alignment, a missing pointer, a null descriptor
    assert fwd(good, x2_=ptr(x2, 4)) == BAD_ARG and fwd(good, x1_=ptr(x1, 8)) == BAD_ARG and fwd(good, y_=ptr(y, 4)) == BAD_ARG
    assert wgrad(good, x2_=ptr(x2, 4)) == BAD_ARG
    assert emu.fmi_conv2d_pair_fwd_f32(C.byref(good), ptr(x1), None, c2, ptr(wf1), ptr(wf2), None, None, None, ptr(y), 0, None) == BAD_ARG
    assert emu.fmi_conv2d_pair_fwd_f32(None, ptr(x1), ptr(x2), c2, ptr(wf1), ptr(wf2), None, None, None, ptr(y), 0, None) == BAD_ARG
    assert emu.fmi_conv2d_pair_fwd_f32(C.byref(good), ptr(x1), ptr(x2), c2, ptr(wf1), ptr(wf2), None, None, None, ptr(y), 3, None) == BAD_ARG
    assert bool((y == 7.0).all()), "a refused call wrote to its output"


class _FakeLib:
    def __init__(self, routed):
        self.routed, self.asked = routed, []

    def conv2d_pair_routed(self, d, c2):
        self.asked.append((d._obj.C, d._obj.K, d._obj.kh, c2))
        return self.routed


def test_routing_follows_the_measured_table(emu):
    """profiles/resblock_pair.txt: bit 0 forward, bit 1 weight gradient; shapes of the step at 256^2, batch 8, and the tests' small ones"""
    want = {(8, 32, 128, 128): 2, (8, 32, 128, 256): 3, (8, 16, 128, 128): 3, (8, 8, 128, 128): 3, (8, 128, 32, 64): 3, (8, 64, 64, 128): 3,
            (8, 64, 128, 128): 0, (8, 128, 64, 128): 0, (2, 8, 64, 64): 3, (1, 1, 64, 64): 3, (2, 8, 16, 16): 0, (8, 128, 16, 32): 0}
    for (n, h, c, k), bits in want.items():
        assert emu.fmi_conv2d_pair_routed(C.byref(desc(n, h, h, c, k)), c) == bits, (n, h, c, k)


def test_wrapper_fallback_wiring(monkeypatch):
    """conv2d_pair: the fused Function where conv2d_pair_ok says so, else conv2d(x2) and then conv2d(x1, residual = that)"""
    from face_mask_inpaint_amd import functional as FF

    class PW:
        def __init__(self, taps, c, k, kh):
            self.wf, self.wt, self.kh, self.kw, self.w3 = torch.zeros(taps, c, k), torch.zeros(taps, k, c), kh, kh, (None, None)

    x1, x2 = torch.zeros(1, 4, 4, 32), torch.zeros(1, 4, 4, 16)
    pw1, pw2 = PW(9, 32, 64, 3), PW(1, 16, 64, 1)
    calls = []

    def fake_conv2d(x, pw, bias=None, residual=None, stride=1, pad=0, pad_mode=0, act=0, in_act=None, *a, **kw):
        calls.append((pw, bias, residual, stride, pad, pad_mode, act, in_act))
        return "s" if pw is pw2 else "out"

    monkeypatch.setattr(FF, "conv2d", fake_conv2d)
    # host tensors: never the fused launch, whatever the library would say
    assert not FF.conv2d_pair_ok(x1, pw1, x2, pw2)
    assert FF.conv2d_pair(x1, pw1, "b1", x2, pw2, "b2", in_act=("apply", 0.1)) == "out"
    assert calls == [(pw2, "b2", None, 1, 0, 0, 0, None), (pw1, "b1", "s", 1, 1, 0, 0, ("apply", 0.1))]
    # the decision on device tensors: every precondition, then the library's routing query
    fake = _FakeLib(1)
    monkeypatch.setattr(FF, "_L", lambda: fake)

    class Dev:
        """just enough of a device tensor for conv2d_pair_ok"""

        def __init__(self, t, addr=256, cuda=True, dtype=torch.float32, contiguous=True):
            self.shape, self.is_cuda, self.dtype, self._a, self._c = t.shape, cuda, dtype, addr, contiguous

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return self._c

        def data_ptr(self):
            return self._a

    assert FF.conv2d_pair_ok(Dev(x1), pw1, Dev(x2), pw2) == 1 and fake.asked == [(32, 64, 3, 16)]
    assert not FF.conv2d_pair_ok(Dev(x1, addr=260), pw1, Dev(x2), pw2)
    assert not FF.conv2d_pair_ok(Dev(x1), pw1, Dev(x2, contiguous=False), pw2)
    assert not FF.conv2d_pair_ok(Dev(x1), pw1, Dev(x2, dtype=torch.bfloat16), pw2)
    assert not FF.conv2d_pair_ok(Dev(x1), pw1, Dev(torch.zeros(1, 4, 5, 16)), pw2)      # another map
    assert not FF.conv2d_pair_ok(Dev(x1), pw1, Dev(x2), PW(1, 16, 32, 1))               # another width
    assert not FF.conv2d_pair_ok(Dev(x1), pw2, Dev(x2), pw2)                            # not a 3x3 + 1x1
    monkeypatch.setattr(FF, "PAIR_ENABLED", False)
    assert not FF.conv2d_pair_ok(Dev(x1), pw1, Dev(x2), pw2)
    monkeypatch.setattr(FF, "PAIR_ENABLED", True)
    with torch.no_grad():  # inference keeps its launch sequence
        assert not FF.conv2d_pair_ok(Dev(x1), pw1, Dev(x2), pw2)
    monkeypatch.setattr(FF, "PAIR_ENABLED", True)
    fake.routed = 0
    assert not FF.conv2d_pair_ok(Dev(x1), pw1, Dev(x2), pw2)
    for bits in (1, 2, 3):  # the library's routing bits are handed on as they are
        fake.routed = bits
        assert FF.conv2d_pair_ok(Dev(x1), pw1, Dev(x2), pw2) == bits
