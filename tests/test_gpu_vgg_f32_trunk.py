"""The fp32 VGG16 trunk of VGGLoss as one autograd node (FF.vgg_trunk_f32) and its two tap passes (csrc/vgg_f32.hip).

The tap passes add no rounding of their own: every output is compared BIT FOR BIT with the composition of the entries they replace
(fmi_maxpool2_f32 / fmi_split3_f32; zeros / cat, add, fmi_maxpool2_bwd_f32, FMI_EW_RELU_BWD_OUT, fmi_split3_f32).  The trunk is compared
with the same module run through ``VGGLoss._block`` (called from here): bit-equal where it makes the same launches (x and y unmerged,
the tap gradient as one tensor), to 1e-5 of the largest entry where x and y share one launch per layer -- the 2N-image launch may
take another tile than the N-image one."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

FF = pytest.importorskip("face_mask_inpaint_amd.functional")

SHAPES = [(3, 4, 6, 16), (2, 5, 7, 64), (3, 8, 8, 128)]  # odd extents (floor mode) included
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _split3(t):
    x3 = torch.empty(t.numel() * 3, device=t.device, dtype=torch.bfloat16)
    FF._L().split3_f32(FF._p(t), _vp(x3), None, t.numel() // t.shape[-1], t.shape[-1], 0, 0.0, FF._st())
    return x3


def _act_map(n, h, w, c, seed):
    """a ReLU output with exact ties inside windows (equal positive values placed by hand) and all-zero windows"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.relu(torch.randn(n, h, w, c, generator=g))
    a[:, 0:2, 0:2, :] = 1.5  # all four equal: the first wins
    a[:, 0, 2, :] = 2.0  # positions 0 and 3 of the window tie above the other two
    a[:, 1, 3, :] = 2.0
    a[:, 0, 3, :] = 0.25
    a[:, 1, 2, :] = 0.0
    if h >= 4:
        a[:, 2:4, 0:2, :] = 0.0  # an all-zero window
        a[:, 2, 2, : c // 2] = 0.75  # positions 1 and 2 tie in half of the channels
        a[:, 2, 3, :] = 0.75
        a[:, 3, 2, :] = 0.75
        a[:, 3, 3, :] = 0.5
    return a.to(DEV)


@pytest.mark.parametrize("shape", SHAPES)
def test_tap_forward_bit_equal(shape):
    n, h, w, c = shape
    lib = FF._L()
    a = _act_map(n, h, w, c, 1)
    ref = torch.empty(n, h // 2, w // 2, c, device=DEV)
    lib.maxpool2_f32(FF._p(a), FF._p(ref), n, h, w, c, FF._st())
    ref3 = _split3(ref)
    for pieces in (False, True):
        pooled = torch.full_like(ref, -7.0)
        p3 = torch.full_like(ref3, -7.0)
        lib.vgg_tap_fwd_f32(FF._p(a), FF._p(pooled), _vp(p3) if pieces else None, n, h, w, c, FF._st())
        assert _same(pooled, ref)
        assert _same(p3, ref3 if pieces else torch.full_like(ref3, -7.0))


def _composed_bwd(a, slices, gpool):
    n, h, w, c = a.shape
    per = n // len(slices)
    gt = torch.cat([torch.zeros(per, h, w, c, device=DEV) if s is None else s for s in slices], 0)
    if gpool is not None:
        un = torch.empty_like(a)
        FF._L().maxpool2_bwd_f32(FF._p(a), FF._p(gpool), FF._p(un), n, h, w, c, FF._st())
        gt = gt + un
    dy = FF.eltwise(FF.EW_RELU_BWD_OUT, gt, a)
    return dy, _split3(dy) if c % 16 == 0 else None


@pytest.mark.parametrize("with_pool", [True, False])
@pytest.mark.parametrize("given", [(1, 1, 1), (1, 0, 1), (0, 1, 0)])
@pytest.mark.parametrize("shape", SHAPES)
def test_tap_backward_bit_equal(shape, given, with_pool):
    _, h, w, c = shape
    n = 3  # a multiple of the slice count
    lib = FF._L()
    a = _act_map(n, h, w, c, 2)
    g = torch.Generator(device="cpu").manual_seed(3)
    slices = [(torch.randn(1, h, w, c, generator=g) - 0.0).to(DEV) if on else None for on in given]
    if slices[1] is not None:
        slices[1][:, :, :, 0] = -0.0  # the composed add turns -0 + 0 into +0
    gpool = torch.randn(n, h // 2, w // 2, c, generator=g).to(DEV) if with_pool else None
    ref, ref3 = _composed_bwd(a, slices, gpool)
    ptrs = (C.c_void_p * 3)(*[None if s is None else s.data_ptr() for s in slices])
    for want_dy, want_3 in ((True, True), (True, False), (False, True)):
        dy = torch.full_like(ref, -7.0)
        dy3 = torch.full_like(ref3, -7.0)
        lib.vgg_tap_bwd_f32(FF._p(a), ptrs, 3, 1, FF._p(gpool), FF._p(dy) if want_dy else None, _vp(dy3) if want_3 else None, n, h, w, c, FF._st())
        assert _same(dy, ref if want_dy else torch.full_like(ref, -7.0))  # a null output leaves its buffer untouched
        assert _same(dy3, ref3 if want_3 else torch.full_like(ref3, -7.0))
    # the same gradient as ONE slice (the cat'ed form)
    whole = torch.cat([torch.zeros(1, h, w, c, device=DEV) if s is None else s for s in slices], 0)
    dy = torch.empty_like(ref)
    lib.vgg_tap_bwd_f32(FF._p(a), (C.c_void_p * 1)(whole.data_ptr()), 1, n, FF._p(gpool), FF._p(dy), None, n, h, w, c, FF._st())
    assert _same(dy, ref)


def test_tap_widths():
    """C % 4 == 0 without pieces; anything else is refused before a launch"""
    lib = FF._L()
    n, h, w = 2, 4, 4
    for c in (4, 8):
        a = _act_map(n, h, w, c, 4)
        gt = torch.randn(n, h, w, c, device=DEV)
        gpool = torch.randn(n, h // 2, w // 2, c, device=DEV)
        ref, _ = _composed_bwd(a, [gt], gpool)
        dy = torch.empty_like(ref)
        lib.vgg_tap_bwd_f32(FF._p(a), (C.c_void_p * 1)(gt.data_ptr()), 1, n, FF._p(gpool), FF._p(dy), None, n, h, w, c, FF._st())
        assert _same(dy, ref)
        pooled, refp = torch.empty_like(gpool), torch.empty_like(gpool)
        lib.vgg_tap_fwd_f32(FF._p(a), FF._p(pooled), None, n, h, w, c, FF._st())
        lib.maxpool2_f32(FF._p(a), FF._p(refp), n, h, w, c, FF._st())
        assert _same(pooled, refp)
        junk = torch.empty(a.numel() * 3, device=DEV, dtype=torch.bfloat16)
        with pytest.raises(FF.FmiError, match="unsupported"):
            lib.vgg_tap_fwd_f32(FF._p(a), FF._p(pooled), _vp(junk), n, h, w, c, FF._st())
        with pytest.raises(FF.FmiError, match="unsupported"):
            lib.vgg_tap_bwd_f32(FF._p(a), (C.c_void_p * 1)(gt.data_ptr()), 1, n, None, None, _vp(junk), n, h, w, c, FF._st())
    a = torch.rand(n, h, w, 6, device=DEV)
    with pytest.raises(FF.FmiError, match="unsupported"):
        lib.vgg_tap_fwd_f32(FF._p(a), FF._p(torch.empty(n, 2, 2, 6, device=DEV)), None, n, h, w, 6, FF._st())


# ---------------------------------------------------------------------------------------------------
# the trunk
# ---------------------------------------------------------------------------------------------------
LOSSES = ("perceptual", "style", "contextual")
WIDTH_DIV = 16  # 4 .. 32 channels: the smallest widths the tap passes accept


@pytest.fixture(scope="module")
def vgg():
    from face_mask_inpaint_amd.modules.loss import VGGLoss

    torch.manual_seed(0)
    v = VGGLoss(width_div=WIDTH_DIV, feature_dtype=torch.float32).to(DEV)
    v._prepare()
    return v


@pytest.fixture(scope="module")
def images():
    g = torch.Generator(device="cpu").manual_seed(5)
    return torch.randn(9, 32, 32, 3, generator=g).to(DEV), torch.randn(9, 32, 32, 3, generator=g).to(DEV)


def _convs(v):
    from torch import nn

    mods = [m for bl in v.blocks for m in bl if isinstance(m, nn.Conv2d)]
    blocks = tuple(sum(isinstance(m, nn.Conv2d) for m in bl) for bl in v.blocks)
    return [(pw, m.bias) for pw, m in zip(v._cache["pws"], mods)], blocks


def _losses(xt, yt, loss_types, n, sliced, last_tap=3):
    """forward_multi_prepared's loss terms on given taps (taps behind last_tap are left out)"""
    out = [0.0] * len(loss_types)
    for i in range(last_tap + 1):
        xparts = xt[i] if sliced else xt[i].split(n, 0)
        yparts = yt[i].split(n, 0)
        _, h, w, c = yt[i].shape
        dim = c * h * w
        for j, kind in enumerate(loss_types):
            xs, ys = xparts[j], yparts[j]
            if kind == "perceptual":
                out[j] = out[j] + FF.l1_loss(xs, ys) / dim
            elif kind == "style":
                out[j] = out[j] + FF.l1_loss(FF.gram_matrix(xs.reshape(n, h * w, c)), FF.gram_matrix(ys.reshape(n, h * w, c))) / (c * c * dim)
            elif kind == "contextual" and i == 3:
                out[j] = out[j] + FF.contextual_loss(xs.reshape(n, h * w, c), ys.reshape(n, h * w, c)) / dim
    return out


def _block_taps(v, x, y):
    xt, yt = [], []
    for i in range(len(v.blocks)):
        x = v._block(i, x)
        with torch.no_grad():
            y = v._block(i, y)
        xt.append(x)
        yt.append(y)
    return xt, yt


@pytest.fixture(scope="module")
def composed(vgg, images):
    """the module through ``_block``: taps, the three losses and the image gradient (computed once, left unchanged)"""
    x = images[0].clone().requires_grad_(True)
    xt, yt = _block_taps(vgg, x, images[1])
    losses = _losses(xt, yt, LOSSES, 3, False)
    (losses[0] * 0.1 + losses[1] * 250 + losses[2]).backward()
    return [t.detach() for t in xt], yt, [float(l.detach()) for l in losses], x.grad


def _close(a, b, what):
    err, top = float((a - b).abs().max()), float(b.abs().max())
    print(f"{what}: max|diff| {err:.3e} of max|ref| {top:.3e}")
    assert err <= 1e-5 * top, what


def test_trunk_module_matches_block(vgg, images, composed):
    """VGGLoss.forward_multi_prepared (the shipped form: slices, x and y in one launch per layer) against ``_block``"""
    xt0, yt0, losses0, gx0 = composed
    x = images[0].clone().requires_grad_(True)
    convs, blocks = _convs(vgg)
    xt, yt = FF.vgg_trunk_f32(x, images[1], convs, blocks, nslice=3)
    for i in range(4):
        _close(torch.cat(xt[i], 0).detach(), xt0[i], f"x tap {i}")
        _close(yt[i], yt0[i], f"y tap {i}")
    x = images[0].clone().requires_grad_(True)
    losses = vgg.forward_multi_prepared(x, images[1], LOSSES)
    for l, l0, kind in zip(losses, losses0, LOSSES):
        print(f"{kind}: {float(l.detach()):.8e} against {l0:.8e}")
        assert abs(float(l.detach()) - l0) <= 1e-5 * abs(l0)
    (losses[0] * 0.1 + losses[1] * 250 + losses[2]).backward()
    _close(x.grad, gx0, "image gradient")


@pytest.mark.parametrize("merge", [False, True])
def test_trunk_forms_match_block(vgg, images, composed, merge):
    xt0, yt0, _, gx0 = composed
    x = images[0].clone().requires_grad_(True)
    convs, blocks = _convs(vgg)
    xt, yt = FF.vgg_trunk_f32(x, images[1], convs, blocks, nslice=3, merge=merge)
    losses = _losses(xt, yt, LOSSES, 3, True)
    (losses[0] * 0.1 + losses[1] * 250 + losses[2]).backward()
    for i in range(4):
        _close(torch.cat(xt[i], 0).detach(), xt0[i], f"x tap {i}")
        _close(yt[i], yt0[i], f"y tap {i}")
    _close(x.grad, gx0, "image gradient")


def test_trunk_unmerged_cat_bit_equal(vgg, images):
    """x and y in launches of their own and the tap gradient as one tensor: the launches of ``_block``, so its bits.  Fixed gradients
    enter at the four taps (the loss kernels' atomics stay out of the comparison)."""
    g = torch.Generator(device="cpu").manual_seed(7)
    convs, blocks = _convs(vgg)
    x0 = images[0].clone().requires_grad_(True)
    xt0, yt0 = _block_taps(vgg, x0, images[1])
    gts = [torch.randn(t.shape, generator=g).to(DEV) for t in xt0]
    torch.autograd.backward([t.split(3, 0)[j] for t in xt0 for j in range(3)], [gt.split(3, 0)[j] for gt in gts for j in range(3)])  # cat
    x = images[0].clone().requires_grad_(True)
    xt, yt = FF.vgg_trunk_f32(x, images[1], convs, blocks, nslice=1, merge=False)
    torch.autograd.backward([t.split(3, 0)[j] for t in xt for j in range(3)], [gt.split(3, 0)[j] for gt in gts for j in range(3)])
    for i in range(4):
        assert _same(xt[i].detach(), xt0[i].detach()), f"x tap {i}"
        assert _same(yt[i], yt0[i]), f"y tap {i}"
    assert _same(x.grad, x0.grad)


def test_trunk_tap_without_gradient(vgg, images):
    """perceptual only on taps 0-1: blocks 3 and 4 receive no gradient and are skipped; the image gradient is the composed path's"""
    x0 = images[0].clone().requires_grad_(True)
    xt0, yt0 = _block_taps(vgg, x0, images[1])
    _losses(xt0, yt0, ("perceptual",) * 3, 3, False, last_tap=1)[0].backward()
    x = images[0].clone().requires_grad_(True)
    convs, blocks = _convs(vgg)
    xt, yt = FF.vgg_trunk_f32(x, images[1], convs, blocks, nslice=3)
    _losses(xt, yt, ("perceptual",) * 3, 3, True, last_tap=1)[0].backward()  # only slice 0 of taps 0 and 1 carries a gradient
    _close(x.grad, x0.grad, "image gradient")
    assert bool((x.grad[3:] == 0).all()) and bool((x0.grad[3:] == 0).all())


def test_trunk_reproducible(vgg, images):
    grads = []
    with FF.deterministic():
        for _ in range(2):
            x = images[0].clone().requires_grad_(True)
            losses = vgg.forward_multi_prepared(x, images[1], LOSSES)
            (losses[0] * 0.1 + losses[1] * 250 + losses[2]).backward()
            grads.append((x.grad, [l.detach() for l in losses]))
    assert _same(grads[0][0], grads[1][0])
    for a, b in zip(grads[0][1], grads[1][1]):
        assert _same(a.reshape(1), b.reshape(1))
