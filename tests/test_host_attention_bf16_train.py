"""Host side of the trainable bf16 self-attention (csrc/attention_bwd_bf16.hip, FF.self_attention_bf16_train, Auto_Attn(attn_dtype=),
FMI_ATTENTION_DTYPE): the float64 reference against autograd, the input condition of the GPU cases, every refusal before any device
call, the option through the three constructors, and the new symbols -- none of this needs (or touches) a GPU."""
import ctypes
import os

import pytest
import torch

import attention_reference as R

from face_mask_inpaint_amd import _lib
from face_mask_inpaint_amd import functional as FF
from face_mask_inpaint_amd._lib import FmiError

BF = torch.bfloat16
NEW = ["fmi_attention_bwd_prep_bf16", "fmi_attention_bwd_bf16"]
OK, BAD, UNSUP = 0, 1, 2


# ---- the reference ----
@pytest.mark.parametrize("shape", [(2, 48, 16, 24), (1, 128, 32, 128)])
def test_identity_reference_equals_float64_autograd(shape):
    n, t, d, c = shape
    q, v, go = (x.double() for x in R.data("moderate", n, t, d, c, seed=5))
    qa, va = q.clone().requires_grad_(True), v.clone().requires_grad_(True)
    o = torch.softmax(qa @ qa.transpose(1, 2), dim=-1) @ va
    o.backward(go)
    ref = R.attention(q, v, go)
    for name, want in (("o", o.detach()), ("gq", qa.grad), ("gv", va.grad)):
        assert R.rel_l2(ref[name], want) < 1e-12, name
    assert R.rel_l2(ref["delta"], (go * o.detach()).sum(-1)) < 1e-12
    assert R.rel_l2(ref["lse"], torch.logsumexp(q @ q.transpose(1, 2), -1)) < 1e-12


def test_bf16_emulation_rounds_where_the_kernels_do():
    q, v, go = R.data("moderate", 1, 128, 32, 128, seed=6)
    emu, ref = R.attention(q, v, go, R.bf16), R.attention(q.to(BF), v.to(BF), go)
    assert torch.equal(emu["go16"], go.to(BF).double())
    for name in ("o", "gq", "gv"):   # a bf16-sized distance from float64 on the same rounded operands: neither exact nor wrong
        e = R.rel_l2(emu[name], ref[name])
        assert 1e-4 < e < 2e-2, (name, e)
    assert R.rel_l2(emu["lse"], ref["lse"]) == 0.0   # q is rounded once, before the scores: the same lse


def test_gpu_cases_meet_their_input_condition():
    """K = Q: the diagonal score |q_i|^2 dominates when q is large.  Moderate: a softmax that is neither uniform nor one-hot; peaked: |q|^2
    beyond the forward's deferred-rescale threshold of 20, the diagonal holds nearly all of the mass"""
    for n, t, d, c in R.KERNEL_SHAPES:
        q, _, _ = R.data("moderate", n, t, d, c, R.case_seed(n, t, d, c))
        m = R.mean_diagonal_probability(q.to(BF))
        assert 0.05 < m < 0.5, ((n, t, d, c), m)
    n, t, d, c = R.PEAKED_SHAPE
    q, _, _ = R.data("peaked", n, t, d, c, R.case_seed(n, t, d, c))
    assert R.mean_diagonal_probability(q.to(BF)) > 0.9
    assert float((q.to(BF).double() ** 2).sum(-1).min()) > 20.0


# ---- the C entries ----
@pytest.fixture(scope="module")
def clib():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        fn = getattr(lib, name)  # AttributeError: the built library lacks the symbol
        fn.argtypes = _lib.SIGNATURES[name]
        fn.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def ptrs():
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 15) & ~15)
    return buf, p, ctypes.c_void_p(p.value + 4)  # the second: 4-byte aligned only


def test_new_symbols_are_declared_and_exported(clib):
    assert all(name in _lib.SIGNATURES for name in NEW)
    assert not _lib.Library(_lib.LIB_PATH, strict=True).missing
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "fmi_hip.h")).read()
    assert all(f"int {name}(" in header for name in NEW)


BAD_SHAPES = [(1, 192, 64, 256), (1, 64, 64, 256), (1, 128, 64, 128), (1, 128, 32, 256), (1, 128, 16, 64), (65536, 128, 64, 256)]


def test_backward_entries_refuse_before_any_launch(clib, ptrs):
    """the pointers are host memory: a call that got past its checks would not return a status"""
    _, p, off = ptrs
    good = (1, 128, 64, 256)
    prep, bwd = clib.fmi_attention_bwd_prep_bf16, clib.fmi_attention_bwd_bf16
    for i in range(4):
        a = [p] * 4
        a[i] = None
        assert prep(*a, *good, None) == BAD, i
        a[i] = off
        assert prep(*a, *good, None) == BAD, i
    for i in range(7):
        a = [p] * 7
        a[i] = None
        assert bwd(*a, *good, None) == BAD, i
        a[i] = off
        assert bwd(*a, *good, None) == BAD, i
    assert prep(p, p, p, p, 0, 128, 64, 256, None) == BAD and bwd(*[p] * 7, 1, 0, 64, 256, None) == BAD
    for shape in BAD_SHAPES:
        assert prep(p, p, p, p, *shape, None) == UNSUP, shape
        assert bwd(*[p] * 7, *shape, None) == UNSUP, shape
        assert bwd(off, *[p] * 6, *shape, None) == UNSUP, shape   # whatever the pointers are


# ---- the Python entries: refused before the library is touched ----
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was used ({name}) before the refusal")


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "_LIB", _NoLibrary())


@pytest.mark.parametrize("shape", [(1, 192, 64, 256), (1, 128, 64, 128), (1, 128, 32, 256), (2, 100, 32, 128)])
def test_op_refuses_unsupported_shapes(no_library, shape):
    n, t, d, c = shape
    q, v = torch.zeros(n, t, d, requires_grad=True), torch.zeros(n, t, c, requires_grad=True)
    with pytest.raises(FmiError, match=rf"T = {t}, \(d_qk, C\) = \({d}, {c}\)"):
        FF.self_attention_bf16_train(q, v)
    with torch.no_grad(), pytest.raises(FmiError, match=rf"T = {t}"):
        FF.self_attention_bf16_train(q, v)


def test_op_needs_device_tensors_for_a_supported_shape(no_library):
    with pytest.raises(FmiError, match="device tensors"):
        FF.self_attention_bf16_train(torch.zeros(1, 128, 64), torch.zeros(1, 128, 256))


def _fill(**kw):
    from face_mask_inpaint_amd import PICNet_inference as PI
    from face_mask_inpaint_amd.modules.model import ReferenceFill

    enc, dec = PI.process_params(PI.get_args([]))
    dec.update(kw.pop("dec", {}))
    return ReferenceFill(None, enc, dec, **kw)


def test_modules_refuse_unsupported_shapes_naming_the_layer(no_library):
    from face_mask_inpaint_amd.modules.pluralistic_model import base_function as BFN
    from face_mask_inpaint_amd.modules.pluralistic_model import network

    a = BFN.Auto_Attn(256, None, attn_dtype=BF)
    with pytest.raises(FmiError, match=r"Auto_Attn.*T = 81, \(d_qk, C\) = \(64, 256\).*9 x 9"):
        a(torch.zeros(1, 256, 9, 9, requires_grad=True))
    with pytest.raises(FmiError, match=r"\(d_qk, C\) = \(16, 64\)"):
        BFN.Auto_Attn(64, None, attn_dtype=BF)(torch.zeros(1, 64, 16, 8))
    with pytest.raises(FmiError, match="attn_dtype"):
        BFN.Auto_Attn(256, None, attn_dtype=torch.float16)
    with pytest.raises(FmiError, match=r"attn1.*\(16, 64\)"):          # a width the kernels do not take: at construction
        network.define_g(ngf=8, z_nc=16, img_f=64, L=0, layers=5, norm="instance", activation="LeakyReLU", use_attn=True, attn_dtype=BF)
    with pytest.raises(FmiError, match="attn_dtype"):
        network.define_g(ngf=32, z_nc=256, img_f=256, L=0, layers=5, attn_dtype=torch.float16)
    g = network.define_g(ngf=32, z_nc=256, img_f=256, L=0, layers=5, norm="instance", activation="LeakyReLU", use_attn=True, attn_dtype=BF)
    with pytest.raises(FmiError, match=r"attn1.*multiple of 128.*3 x 3.*144 tokens"):   # a token count: at the first forward
        g(torch.zeros(1, 256, 3, 3, requires_grad=True))
    with pytest.raises(FmiError, match="attention_dtype"):
        _fill(attention_dtype=torch.float16)


# ---- the option ----
def test_constructors_accept_and_store_the_option(monkeypatch):
    from face_mask_inpaint_amd.modules.pluralistic_model import base_function as BFN
    from face_mask_inpaint_amd.modules.pluralistic_model import network

    monkeypatch.delenv("FMI_ATTENTION_DTYPE", raising=False)
    assert BFN.Auto_Attn(256, None).attn_dtype == torch.float32
    assert BFN.Auto_Attn(256, None, attn_dtype=BF).attn_dtype == BF
    kw = dict(ngf=32, z_nc=256, img_f=256, L=0, layers=5, norm="instance", activation="LeakyReLU", use_attn=True)
    g32, g16 = network.define_g(**kw), network.define_g(**kw, attn_dtype=BF)
    assert (g32.attn_dtype, g32.attn1.attn_dtype) == (torch.float32, torch.float32)
    assert (g16.attn_dtype, g16.attn1.attn_dtype, g16.compute_dtype) == (BF, BF, torch.float32)
    assert list(g32.state_dict()) == list(g16.state_dict())
    a, b = _fill(), _fill(attention_dtype=BF)
    assert a.attention_dtype == torch.float32 and a.decoder.attn1.attn_dtype == torch.float32
    assert b.attention_dtype == BF and b.decoder.attn1.attn_dtype == BF and b.decoder.compute_dtype == torch.float32
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(sa[k].shape == sb[k].shape and sa[k].dtype == sb[k].dtype for k in sa)
    b.load_state_dict(sa, strict=True)
    # the discriminator's attention is out of scope and has no switch to inherit
    d = network.define_d(ndf=32, img_f=128, layers=5, norm="none", activation="LeakyReLU")
    assert all(m.attn_dtype == torch.float32 for m in d.modules() if isinstance(m, BFN.Auto_Attn))
    # the fp32 packs of the query convolution are kept: it runs in fp32 either way
    assert not any(getattr(m, "_fmi_no_w3", False) for m in b.modules())


def test_environment_variable_selects_the_dtype_where_the_argument_is_absent(monkeypatch):
    monkeypatch.setenv("FMI_ATTENTION_DTYPE", "bf16")
    assert _fill().decoder.attn1.attn_dtype == BF
    assert _fill(attention_dtype=torch.float32).decoder.attn1.attn_dtype == torch.float32   # the argument wins
    monkeypatch.setenv("FMI_ATTENTION_DTYPE", "fp32")
    assert _fill().decoder.attn1.attn_dtype == torch.float32
    for bad in ("half", "BF16", ""):
        monkeypatch.setenv("FMI_ATTENTION_DTYPE", bad)
        with pytest.raises(FmiError, match="FMI_ATTENTION_DTYPE"):
            _fill()
        _fill(attention_dtype=BF)   # not read when the argument is given
