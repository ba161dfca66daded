"""Host side of the bf16 PICNet encoders and guided attention: the new C entries are exported and their refusals come back before any HIP
call, the guided attention's shape dispatch, the harness flag, checkpoint compatibility of the bf16 build, the constructor refusals and
the inference-only refusal -- none of this needs (or touches) a GPU."""
import ctypes

import pytest
import torch

from face_mask_inpaint_amd import _lib
from face_mask_inpaint_amd._lib import FmiError

NEW = ["fmi_conv2d_thin_in_fwd_bf16", "fmi_conv2d_c32_fwd_bf16", "fmi_resblock_tail_bf16", "fmi_picnet_stem_tail_bf16",
       "fmi_guided_attention_fwd_bf16"]
WAVES = "fmi_guided_attention_fwd_bf16_waves"
OK, BAD, UNSUP = 0, 1, 2
BF = torch.bfloat16


@pytest.fixture(scope="module")
def clib():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        fn = getattr(lib, name)  # AttributeError: the built library lacks the symbol
        fn.argtypes = _lib.SIGNATURES[name]
        fn.restype = ctypes.c_int
    fn = getattr(lib, WAVES)
    fn.argtypes = _lib.PREDICATES[WAVES]
    fn.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def ptrs():
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 15) & ~15)
    q = ctypes.c_void_p(p.value + 2)  # 2-byte aligned only
    return buf, p, q


def _desc(n=1, h=8, w=16, c=32, k=32, ks=3, stride=1, pad=1, oh=None, ow=None):
    oh = (h + 2 * pad - ks) // stride + 1 if oh is None else oh
    ow = (w + 2 * pad - ks) // stride + 1 if ow is None else ow
    return _lib.ConvDesc(n, h, w, c, oh, ow, k, c, k, ks, ks, stride, pad, 0, 1)


def test_new_symbols_are_exported_and_bound(clib):
    assert all(name in _lib.SIGNATURES for name in NEW) and WAVES in _lib.PREDICATES
    assert not _lib.Library(_lib.LIB_PATH, strict=True).missing


def test_conv_refusals_return_before_any_launch(clib, ptrs):
    """(d, x, w, bias, slope, y, stream) for both convolutions.  The pointers are host memory: a call that got past its checks would not
    return a status"""
    _, p, q = ptrs
    for f, c in ((clib.fmi_conv2d_thin_in_fwd_bf16, 3), (clib.fmi_conv2d_c32_fwd_bf16, 32)):
        d = _desc(c=c)
        assert f(None, p, p, p, 0.1, p, None) == BAD
        for bad in ((None, p, p), (p, None, p), (p, p, None)):
            assert f(ctypes.byref(d), bad[0], bad[1], p, 0.1, bad[2], None) == BAD
        assert f(ctypes.byref(_desc(n=0, c=c)), p, p, p, 0.1, p, None) == BAD
        assert f(ctypes.byref(_desc(c=c, oh=9)), p, p, p, 0.1, p, None) == BAD            # an output extent that does not follow
        assert f(ctypes.byref(d), p, p, p, 0.1, q, None) == UNSUP                          # y off 16-byte alignment
        assert f(ctypes.byref(_desc(c=c, k=48)), p, p, p, 0.1, p, None) == UNSUP           # K in {32, 64}
        assert f(ctypes.byref(_desc(c=c, k=128)), p, p, p, 0.1, p, None) == UNSUP
        assert f(ctypes.byref(_desc(c=c, stride=2)), p, p, p, 0.1, p, None) == UNSUP
        assert f(ctypes.byref(_desc(c=c, pad=0)), p, p, p, 0.1, p, None) in (BAD, UNSUP)   # 3x3 without padding shrinks the map
        d5 = _desc(c=c, ks=5, pad=2)
        assert f(ctypes.byref(d5), p, p, p, 0.1, p, None) == UNSUP
        dp = _desc(c=c)
        dp.x_cstride = c + 8
        assert f(ctypes.byref(dp), p, p, p, 0.1, p, None) == UNSUP                         # dense pixel pitches only
        dm = _desc(c=c)
        dm.pad_mode = 1
        assert f(ctypes.byref(dm), p, p, p, 0.1, p, None) == UNSUP                         # zero padding only
        # an unsupported shape is refused whatever the pointers are
        assert f(ctypes.byref(_desc(c=c, k=48)), q, p, p, 0.1, p, None) == UNSUP
    thin, c32 = clib.fmi_conv2d_thin_in_fwd_bf16, clib.fmi_conv2d_c32_fwd_bf16
    assert thin(ctypes.byref(_desc(c=5)), p, p, p, 0.1, p, None) == UNSUP                   # C <= 4
    assert thin(ctypes.byref(_desc(c=3, ks=1, pad=0)), p, p, p, 0.1, p, None) == UNSUP      # the stem's conv1 is 3 x 3
    assert c32(ctypes.byref(_desc(c=64, k=64)), p, p, p, 0.1, p, None) == UNSUP             # C = 64 belongs to fmi_conv2d_fwd_chan_bf16
    assert c32(ctypes.byref(_desc(c=16)), p, p, p, 0.1, p, None) == UNSUP
    for i in range(3):                                                                      # x, wnk, bias off 16-byte alignment
        a = [p, p, p]
        a[i] = q
        assert c32(ctypes.byref(_desc()), *a, 0.1, p, None) == UNSUP, i


def test_tail_refusals_return_before_any_launch(clib, ptrs):
    _, p, q = ptrs
    f = clib.fmi_resblock_tail_bf16  # (main, shortcut, y_raw, y_act, y_f32, N, H, W, C, pool, slope, stream)
    shape = (1, 8, 16, 32)
    assert f(None, p, p, p, p, *shape, 0, 0.1, None) == BAD and f(p, None, p, p, p, *shape, 0, 0.1, None) == BAD
    assert f(p, p, None, None, None, *shape, 0, 0.1, None) == BAD                            # all three outputs NULL
    assert f(p, p, p, None, None, 0, 8, 16, 32, 0, 0.1, None) == BAD
    assert f(p, p, p, None, None, *shape, 2, 0.1, None) == BAD                               # pool is 0 or 1
    assert f(p, p, p, None, None, 1, 8, 16, 36, 0, 0.1, None) == UNSUP                       # C % 8
    assert f(p, p, p, None, None, 1, 9, 16, 32, 1, 0.1, None) == UNSUP                       # odd H with pool
    assert f(p, p, p, None, None, 1, 8, 15, 32, 1, 0.1, None) == UNSUP
    for i in range(5):                                                                       # any pointer off 16-byte alignment
        a = [p, p, p, p, p]
        a[i] = q
        assert f(*a, *shape, 0, 0.1, None) == UNSUP, i
    g = clib.fmi_picnet_stem_tail_bf16  # (h, img, wb, bias, y_raw, y_act, N, H, W, C, K, slope, stream)
    shape = (1, 8, 16, 3, 32)
    for i in range(3):
        a = [p, p, p]
        a[i] = None
        assert g(*a, p, p, p, *shape, 0.1, None) == BAD, i
    assert g(p, p, p, p, None, None, *shape, 0.1, None) == BAD                               # both outputs NULL
    assert g(p, p, p, p, p, p, 1, 8, 16, 5, 32, 0.1, None) == UNSUP                          # C <= 4
    assert g(p, p, p, p, p, p, 1, 8, 16, 3, 36, 0.1, None) == UNSUP                          # K % 8
    assert g(p, p, p, p, p, p, 1, 7, 16, 3, 32, 0.1, None) == UNSUP                          # odd H
    for i in (0, 1, 2, 3, 4, 5):
        a = [p, p, p, p, p, p]
        a[i] = q
        assert g(*a, *shape, 0.1, None) == UNSUP, i


def test_guided_attention_refusals_return_before_any_launch(clib, ptrs):
    """(q, src, ref, mask, out, N, T, D, C, waves, stream)"""
    _, p, q = ptrs
    f = clib.fmi_guided_attention_fwd_bf16
    shape = (1, 128, 32, 128, 0, None)
    for i in range(5):
        a = [p, p, p, p, p]
        a[i] = None
        assert f(*a, *shape) == BAD, i
    for i in range(5):                                    # q, src, ref, out off 16-byte alignment; the mask off 4
        a = [p, p, p, p, p]
        a[i] = q
        assert f(*a, *shape) == BAD, i
    assert f(p, p, p, p, p, 0, 128, 32, 128, 0, None) == BAD
    assert f(p, p, p, p, p, 1, 192, 32, 128, 0, None) == UNSUP        # T % 128
    assert f(p, p, p, p, p, 1, 128, 64, 128, 0, None) == UNSUP        # (D, C) = (64, 128)
    assert f(p, p, p, p, p, 1, 128, 64, 256, 0, None) == UNSUP        # the plain attention's other shape: a V tile 512 wide does not fit
    assert f(p, p, p, p, p, 1, 128, 32, 64, 0, None) == UNSUP
    assert f(p, p, p, p, p, 65536, 128, 32, 128, 0, None) == UNSUP
    assert f(p, p, p, p, p, 1, 128, 32, 128, 8, None) == UNSUP        # eight waves own 256 queries
    assert f(p, p, p, p, p, 1, 256, 32, 128, 2, None) == UNSUP        # no two-wave form
    assert f(q, p, p, p, p, 1, 192, 32, 128, 0, None) == UNSUP        # an unsupported shape is refused whatever the pointers are


def test_guided_attention_dispatch_at_its_thresholds(clib):
    """eight waves if T % 256 == 0 and (T / 256) N >= 256, else four: the plain bf16 forward's rule"""
    w = getattr(clib, WAVES)
    want = lambda n, t: 8 if t % 256 == 0 and (t // 256) * n >= 256 else 4
    for t in (128, 256, 384, 512, 1024, 16384):
        per = t // 256
        ns = {1, 2, 8, 65535}
        if per:
            edge = -(-256 // per)
            ns.update((edge - 1, edge, edge + 1))
        for n in sorted(x for x in ns if x >= 1):
            assert w(n, t) == want(n, t), (n, t)
    assert [w(n, t) for n, t in ((255, 256), (256, 256), (64, 1024), (63, 1024), (8, 1024), (65535, 384))] == [4, 8, 8, 4, 4, 4]


# ---------------------------------------------------------------------------------------------------------------------------------
# the flag, the builds, the refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_harness_flag_and_build_refusal():
    from face_mask_inpaint_amd import PICNet_inference as PI

    assert PI.get_args([]).feature_dtype == "fp32"
    assert PI.get_args(["--feature_dtype", "bf16"]).feature_dtype == "bf16"
    with pytest.raises(SystemExit):
        PI.get_args(["--feature_dtype", "fp16"])
    # the flag stays out of define_e's and define_g's keywords
    enc, dec = PI.process_params(PI.get_args(["--feature_dtype", "bf16", "--generator_dtype", "bf16"]))
    assert not any("dtype" in k for k in list(enc) + list(dec))
    with pytest.raises(FmiError, match="old_model"):
        PI.build(PI.get_args(["--old_model", "--feature_dtype", "bf16"]), torch.device("cpu"))
    args = PI.get_args([])
    args.feature_dtype = "half"
    with pytest.raises(FmiError, match="feature_dtype"):
        PI.build(args, torch.device("cpu"))


def _fill(decoder=None, feature=None, use_att=True, enc_over=None, **dec_over):
    from face_mask_inpaint_amd import PICNet_inference as PI
    from face_mask_inpaint_amd.modules.model import ReferenceFill

    enc, dec = PI.process_params(PI.get_args([]))
    enc.update(enc_over or {})
    dec.update(dec_over)
    kw = {}
    if decoder is not None:
        kw["decoder_dtype"] = decoder
    if feature is not None:
        kw["feature_dtype"] = feature
    return ReferenceFill(None, enc, dec, use_att=use_att, **kw)


def _marked(model):
    return sorted(n for n, m in model.named_modules() if getattr(m, "_fmi_no_w3", False))


def test_all_four_builds_share_the_fp32_state_dict(tmp_path):
    a = _fill()
    sa = a.state_dict()
    assert a.feature_dtype == torch.float32 and len(sa) > 100
    torch.save(sa, tmp_path / "a.pth")
    for dec_dt, feat_dt in ((None, BF), (BF, BF), (BF, None)):
        b = _fill(dec_dt, feat_dt)
        assert b.feature_dtype == (feat_dt or torch.float32) and b.decoder.compute_dtype == (dec_dt or torch.float32)
        assert b.src_encoder.compute_dtype == b.ref_encoder.compute_dtype == b.feature_dtype
        sb = b.state_dict()
        assert list(sa) == list(sb)
        for k in sa:
            assert sa[k].shape == sb[k].shape and sa[k].dtype == sb[k].dtype == torch.float32, k
        b.load_state_dict(torch.load(tmp_path / "a.pth", weights_only=True), strict=True)
        torch.save(b.state_dict(), tmp_path / "b.pth")
        back = torch.load(tmp_path / "b.pth", weights_only=True)
        assert all(torch.equal(back[k], sa[k]) for k in sa)
        a.load_state_dict(back, strict=True)


def test_no_w3_marks_sit_on_the_encoders_and_the_attention_conv():
    feat = _fill(None, BF)
    convs = sorted(n for n, m in feat.named_modules() if isinstance(m, torch.nn.Conv2d) and n.startswith(("src_encoder.", "ref_encoder.")))
    # block0 + four encoder blocks + (six infer_prior blocks) + the head, three convolutions each: 54 with the default widths
    assert len(convs) == 3 * (1 + 4 + 6 + 1) + 3 * (1 + 4 + 1) == 54
    assert _marked(feat) == sorted(convs + ["attention.conv"])
    dec_only = _marked(_fill(BF))
    assert len(dec_only) == 5 * 3 + 1 + 1 and all(n.startswith(("decoder.decoder", "decoder.out4", "decoder.attn1.query_conv")) for n in dec_only)
    assert _marked(_fill(BF, BF)) == sorted(dec_only + convs + ["attention.conv"])
    assert not _marked(_fill())


def test_constructor_refusals():
    from face_mask_inpaint_amd.modules.pluralistic_model import network

    with pytest.raises(FmiError, match="feature_dtype"):
        _fill(None, torch.float16)
    with pytest.raises(FmiError, match="compute_dtype"):
        network.define_e(ngf=32, z_nc=128, img_f=128, layers=5, L=6, activation="LeakyReLU", compute_dtype=torch.float16)
    cases = [
        (dict(enc_over=dict(type="drn")), "drn"),
        (dict(use_att=False), "use_att"),
        (dict(enc_over=dict(norm="instance")), "norm 'none'"),
        (dict(enc_over=dict(ngf=16)), "ngf == 32"),
        (dict(enc_over=dict(ngf=64)), "ngf == 32"),
        (dict(enc_over=dict(z_nc=48)), "prior.conv2"),          # a head of 96 channels: not a multiple of 64
        (dict(enc_over=dict(img_f=96)), "encoder1"),            # 32 -> 64 -> 96: a wider layer that is no multiple of 64
        (dict(enc_over=dict(img_f=256)), r"\(64, 256\)"),       # the attention's accepted set is (32, 128)
        (dict(enc_over=dict(img_f=64)), r"\(16, 64\)"),
    ]
    for kw, pattern in cases:
        with pytest.raises(FmiError, match=pattern) as info:
            _fill(None, BF, **kw)
        assert "these run in fp32 only" in str(info.value), kw
    # fp32 takes what it took before
    _fill(enc_over=dict(ngf=16))
    _fill(use_att=False)
    _fill(enc_over=dict(img_f=256))
    e = network.define_e(ngf=32, z_nc=128, img_f=128, layers=5, L=6, activation="LeakyReLU")
    assert e.compute_dtype == torch.float32


def test_grad_mode_and_extents_are_refused_before_the_library_is_reached():
    """CPU tensors: an op that reached the library would raise 'need device tensors', not the refusal under test"""
    from face_mask_inpaint_amd.modules.pluralistic_model import network

    b = _fill(None, BF)
    x = torch.zeros(1, 3, 256, 256)
    m = torch.zeros(1, 256, 256)
    before = {k: v.clone() for k, v in b.state_dict().items()}
    with pytest.raises(FmiError, match="inference only"):
        b(x, x, src_mask=m)
    e = network.define_e(ngf=32, z_nc=128, img_f=128, layers=5, L=6, activation="LeakyReLU", compute_dtype=BF)
    with pytest.raises(FmiError, match="inference only"):
        e(torch.zeros(1, 3, 64, 128))
    for p in e.parameters():
        p.requires_grad_(False)
    with pytest.raises(FmiError, match="inference only"):      # a frozen encoder, an input that carries a gradient
        e(torch.zeros(1, 3, 64, 128, requires_grad=True))
    with torch.no_grad():
        with pytest.raises(FmiError, match="device tensors|not found"):   # gradients off: the call goes on to the library
            e(torch.zeros(1, 3, 64, 128))
        with pytest.raises(FmiError, match="multiples of 8"):
            e(torch.zeros(1, 3, 64, 100))
        with pytest.raises(FmiError, match="multiples of 8"):
            b(torch.zeros(1, 3, 252, 256), torch.zeros(1, 3, 252, 256), src_mask=torch.zeros(1, 252, 256))
        with pytest.raises(FmiError, match="64 tokens"):        # an 8 x 8-token feature map
            b(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64), src_mask=torch.zeros(1, 64, 64))
        with pytest.raises(FmiError, match="no_prior"):
            b(x, x, src_mask=m, no_prior=True)
        with pytest.raises(FmiError, match="device tensors|not found"):
            b(x, x, src_mask=m)
    after = b.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), "a refused call advanced the SpectralNorm state"
