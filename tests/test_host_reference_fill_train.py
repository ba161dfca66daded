"""Host side of the PICNet trainer (face_mask_inpaint_amd/train_reference_fill.py): the command line and the checkpoints' key lists against
the reference's (tests/golden/ref_train.pt, tools/golden/gen_reference_fill_train.py), the refusals that need no GPU, the C boundary of the
image-head kernels, a guard on the fixture itself (a float64 restatement of loss.py:48-51,84-95,115 written here reproduces what the
reference recorded), and the kernels' own source compiled for the host (g++ -DFMI_HOST_THREADS, csrc/host_threads.h) held to the GPU
test's bounds."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from face_mask_inpaint_amd import train_reference_fill as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fmi_gan_image_head_fwd_f32", "fmi_gan_image_head_bwd_f32")
SMALL = ("a", "b", "c", "d")
CASES = SMALL + ("e",)
U = 2.0 ** -24
get_args = TR.get_args  # every test here fails at import without the feature


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and the float64 restatement
def head_inputs(fx, name):
    """(gen, gt, src, ref, mask) fp32 of a fixture case: images uniform in [0, 1] from the stored seed, the stored mask"""
    cfg = fx["head_inputs"][name]
    n, h, w = cfg["shape"]
    g = torch.Generator().manual_seed(cfg["seed"])
    gen, gt, src, ref = (torch.rand((n, 3, h, w), generator=g) for _ in range(4))
    return gen, gt, src, ref, fx["head"][name]["mask"].float()


def upstream(fx, name):
    """the stored-seed upstream gradient Gx [3N, OH, OW, 3] and g_l1"""
    cfg = fx["head_inputs"][name]
    n, h, w = cfg["shape"]
    oh, ow = out_size(h, w, cfg["vgg_size"])
    return torch.randn((3 * n, oh, ow, 3), generator=torch.Generator().manual_seed(cfg["gx_seed"])), cfg["g_l1"]


def out_size(h, w, size):
    return (size, size) if w > size else (h, w)  # loss.py:48


def axis_weights(n_in, n_out, kind):
    """(i0, i1, l0, l1) of every output index of one axis, align_corners=True.  kind 'f32': exactly as lerp_of (csrc/common.h) forms them,
    every operation in numpy float32; 'f64': the same arithmetic in double (what ATen's upsample_bilinear2d does for double tensors)"""
    f = np.float32 if kind == "f32" else np.float64
    scale = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
    r = (scale * np.arange(n_out).astype(f)).astype(f)
    i0 = r.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (r - i0.astype(f)).astype(f)
    l0 = (f(1) - l1).astype(f)
    return i0, i1, l0, l1


def axis_matrix(n_in, n_out, kind):
    """the [n_out, n_in] float64 matrix of one axis of R, and per input index the number of (output, corner) pairs that read it"""
    i0, i1, l0, l1 = axis_weights(n_in, n_out, kind)
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    reads = np.zeros(n_in, dtype=np.int64)
    for o in range(n_out):
        m[o, i0[o]] += float(l0[o])
        m[o, i1[o]] += float(l1[o])
        reads[i0[o]] += 1
        reads[i1[o]] += 1
    return m, int(reads.max())


def restated(gen, gt, src, ref, mask, mean, std, size, gx=None, g_l1=0.0, kind="f32"):
    """float64 from the definitions (loss.py:48-51,84-95,115) on fp32 inputs, the interpolation weights of ``kind``:
    x_in, y_in [3N, OH, OW, 3]; x_mag, y_mag = (sum |w_i| |v_i| + |mean|) / std per element; l1; grad = d (g_l1 l1 + <gx, x_in>) / d gen;
    grad_mag = the sum of the magnitudes of that gradient's terms (one per contributing output pixel and stream, and the L1 term);
    contributors = the largest number of (output pixel, corner) pairs of one stream that reach one entry"""
    n, _, h, w = gen.shape
    oh, ow = out_size(h, w, size)
    my, cy = axis_matrix(h, oh, kind)
    mx, cx = axis_matrix(w, ow, kind)
    R = lambda v: torch.einsum("oh,nchw,pw->ncop", my, v, mx)
    Rt = lambda g: torch.einsum("oh,ncop,pw->nchw", my, g, mx)
    mean, std = mean.double().view(1, 3, 1, 1), std.double().view(1, 3, 1, 1)
    m = mask.double().unsqueeze(1)
    im = 1 - m
    gd = gen.double()
    norm = lambda v: ((R(v) - mean) / std).permute(0, 2, 3, 1)
    mag = lambda v: ((R(v.abs()) + mean.abs()) / std).permute(0, 2, 3, 1)
    xs, ys = [gd, gd * im, gd * m], [gt.double(), src.double(), ref.double() * m]
    out = dict(x_in=torch.cat([norm(v) for v in xs]), y_in=torch.cat([norm(v) for v in ys]), x_mag=torch.cat([mag(v) for v in xs]),
               y_mag=torch.cat([mag(v) for v in ys]), contributors=cy * cx)
    cnt = float(gd.numel())
    out["l1"] = float((gd - gt.double()).abs().sum() / cnt)
    g = gx.double().permute(0, 3, 1, 2) / std if gx is not None else torch.zeros(3 * n, 3, oh, ow, dtype=torch.float64)
    g0, g1, g2 = g[:n], g[n:2 * n], g[2 * n:]
    t_l1 = g_l1 * torch.sign(gd - gt.double()) / cnt
    out["grad"] = t_l1 + Rt(g0) + im * Rt(g1) + m * Rt(g2)
    out["grad_mag"] = t_l1.abs() + Rt(g0.abs()) + im.abs() * Rt(g1.abs()) + m.abs() * Rt(g2.abs())
    return out


def backward_k(contributors):
    """the rounded operations of the longest chain behind one entry of d_gen (csrc/ganhead.hip): per contributing (output pixel, corner)
    the division by std, the product of the two weights and its product with the quotient (3); their accumulation (contributors - 1
    additions after the first); 1 - m and the product with the mask (2); the quotient g_l1 / count and the three final additions (4)"""
    return 3 + (contributors - 1) + 2 + 4


def check_forward(got_x, got_y, got_l1, want, rec, pick=lambda t: t):
    """the forward bounds: every element of x_in / y_in within 8 U (sum |w_i| |v_i| + |mean|) / std of the restatement with fp32 weights
    -- the eight rounded operations are the product with the mask (1), two per lerp level over two levels (4), l0 = 1 - l1 (1), the
    subtraction of the mean (1) and the division by std (1); per tensor the worst error against the reference's float64 record at most
    twice the worst error of the reference's own fp32 run; l1 within max(4 |ref32 - ref64|, 4 U |ref64|) of float64.
    ``pick`` subsamples a full tensor to the record's grid (case e).  Returns the worst observed multiples, for the record."""
    worst = {}
    for key, got in (("x_in", got_x), ("y_in", got_y)):
        got = got.double()
        assert not bool(torch.isnan(got).any()), key
        err, lim = (got - want[key]).abs(), 8 * U * want[key[0] + "_mag"]
        assert bool((err <= lim).all()), (key, float((err / want[key[0] + "_mag"]).max() / U))
        worst[key] = float((err / want[key[0] + "_mag"]).max() / U)
        e64 = float((pick(got) - rec[key + "64"]).abs().max())
        r64 = float((rec[key].double() - rec[key + "64"]).abs().max())
        assert e64 <= 2 * r64, (key, e64, r64)
        worst[key + "_vs_ref64"] = (e64, r64)
    r64, r32 = float(rec["l164"]), float(rec["l1"])
    assert abs(float(got_l1) - r64) <= max(4 * abs(r32 - r64), 4 * U * abs(r64)), (float(got_l1), r64, r32)
    return worst


def check_backward(got, want, k):
    """every entry within k U sum |terms| of float64; returns the worst observed multiple of U sum |terms|"""
    got = got.double()
    assert not bool(torch.isnan(got).any())
    err = (got - want["grad"]).abs()
    ratio = float(torch.where(want["grad_mag"] > 0, err / want["grad_mag"], err * float("inf")).nan_to_num(0.0).max() / U)
    assert bool((err <= k * U * want["grad_mag"]).all()), (ratio, k)
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------------
def test_get_args_has_the_reference_flags_and_defaults(golden):
    ref = dict((k, v) for k, v in golden("ref_train.pt")["args"])
    assert ref["learning_rate"] == 1e-5 and ref["batch_size"] == 8 and ref["encoder_type"] == "pluralistic" and ref["use_att"] == 1
    ours = vars(TR.get_args([]))
    assert set(ours) == set(ref)
    for k, v in ref.items():
        if k == "eval_options":
            assert isinstance(ours[k], set) and sorted(ours[k]) == v
        else:
            assert ours[k] == v and type(ours[k]) is type(v), (k, ours[k], v)
    a = TR.get_args("--epochs 2 --batch_size 4 --learning_rate 0.001 --eval_options ssim ms_ssim --debug 1 --img_scale 0.5 --run_name r "
                    "--checkpoint_path ck --mask_detector_path md.pth --data_root /d --src_img_path s --ref_img_path rf --mask_path m "
                    "--identity_file_path id.txt --use_best_reference 1 --pt_ckpt_path pic --encoder_type drn --encoder_ngf 8 --encoder_z_nc 16 "
                    "--encoder_img_f 24 --encoder_layers 4 --encoder_norm instance --encoder_activation ReLU --encoder_init_type normal "
                    "--decoder_ngf 12 --decoder_z_nc 20 --decoder_img_f 28 --decoder_L 1 --decoder_layers 3 --decoder_norm none "
                    "--decoder_activation SELU --decoder_init_type xavier --disc_ndf 6 --disc_layers 2 --disc_model_type PatchDis "
                    "--disc_init_type kaiming --use_att 0".split())
    want = dict(epochs=2, batch_size=4, learning_rate=1e-3, eval_options=["ssim", "ms_ssim"], debug=1, img_scale=0.5, run_name="r", checkpoint_path="ck",
                mask_detector_path="md.pth", data_root="/d", src_img_path="/d/s", ref_img_path="/d/rf", mask_path="/d/m", identity_file_path="/d/id.txt",
                use_best_reference=1, pt_ckpt_path="",  # cleared: the encoder is not 'pluralistic' (train_reference_fill.py:82-83)
                encoder_type="drn", encoder_ngf=8, encoder_z_nc=16, encoder_img_f=24, encoder_layers=4, encoder_norm="instance", encoder_activation="ReLU",
                encoder_init_type="normal", decoder_ngf=12, decoder_z_nc=20, decoder_img_f=28, decoder_L=1, decoder_layers=3, decoder_norm="none",
                decoder_activation="SELU", decoder_init_type="xavier", disc_ndf=6, disc_layers=2, disc_model_type="PatchDis", disc_init_type="kaiming",
                use_att=0)
    assert vars(a) == want
    assert TR.get_args(["--pt_ckpt_path", "pic"]).pt_ckpt_path == "pic"


def test_default_models_have_the_reference_checkpoint_keys(golden):
    fx = golden("ref_train.pt")
    G, D = TR.build_models(TR.get_args([]))
    assert list(G.state_dict().keys()) == fx["keys_G"]
    assert list(D.state_dict().keys()) == fx["keys_D"]
    assert len(set(fx["keys_G"])) == len(fx["keys_G"]) and any(k.startswith("mask_detector.") for k in fx["keys_G"])


def test_trainer_refusals(monkeypatch, tmp_path):
    from face_mask_inpaint_amd._lib import FmiError

    kw = dict(epochs=1, batch_size=1, learning_rate=1e-3, save_checkpoint=False, dir_checkpoint=str(tmp_path), run_name="", debug=False)
    with pytest.raises(FmiError, match="fid"):
        TR.train_net(None, None, "cuda", [], [], eval_options={"fid", "ssim"}, **kw)
    with pytest.raises(FmiError, match="fid"):
        TR.evaluate(None, None, [], None, "cuda", 1, options={"fid"})
    with pytest.raises(FmiError, match="fid"):
        TR.main(["--eval_options", "fid"])
    with pytest.raises(FmiError, match="GPU"):
        TR.train_net(None, None, "cpu", [], [], eval_options={"ssim"}, **kw)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(FmiError, match="GPU"):
        TR.train_net(None, None, "cuda", [], [], eval_options={"ssim"}, **kw)
    with pytest.raises(FmiError, match="GPU"):
        TR.main([])


def test_image_head_refuses_cpu_tensors_and_bad_shapes():
    from face_mask_inpaint_amd import functional as FF
    from face_mask_inpaint_amd._lib import FmiError

    a, m, v = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4), torch.ones(3)
    with pytest.raises(FmiError, match="device tensors"):
        FF.gan_image_head(a, a, a, a, m, v, v)
    with pytest.raises(FmiError, match=r"gen is \[N, 3, H, W\]"):
        FF.gan_image_head(torch.zeros(1, 4, 4, 3), a, a, a, m, v, v)
    with pytest.raises(FmiError, match="src .* does not match"):
        FF.gan_image_head(a, a, torch.zeros(1, 3, 4, 5), a, m, v, v)
    with pytest.raises(FmiError, match="mask is"):
        FF.gan_image_head(a, a, a, a, torch.zeros(1, 1, 4, 4), v, v)
    with pytest.raises(FmiError, match="three entries"):
        FF.gan_image_head(a, a, a, a, m, torch.ones(4), v)
    with pytest.raises(FmiError, match="fp32"):
        FF.gan_image_head(a.double(), a, a, a, m, v, v)
    with pytest.raises(FmiError, match="tensor"):
        FF.gan_image_head(a, None, a, a, m, v, v)


def test_image_head_refuses_stream_capture(monkeypatch):
    """the head is not offered inside a captured stream: refused before anything else is looked at"""
    from face_mask_inpaint_amd import functional as FF
    from face_mask_inpaint_amd._lib import FmiError

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    a = torch.zeros(1, 3, 4, 4)
    with pytest.raises(FmiError, match="stream capture"):
        FF.gan_image_head(a, a, a, a, torch.zeros(1, 4, 4), torch.ones(3), torch.ones(3))


def test_image_head_entries_are_declared():
    hdr = open(os.path.join(ROOT, "include", "fmi_hip.h")).read()
    assert "loss.py:48-51,84-95,115" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    from face_mask_inpaint_amd import _lib

    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
    mk = open(os.path.join(ROOT, "face_mask_inpaint_amd", "csrc", "Makefile")).read()
    assert "ganhead.hip" in mk


def test_image_head_argument_validation_without_a_gpu():
    """bad arguments come back as status codes before anything is launched"""
    from face_mask_inpaint_amd import _lib

    c = ctypes.CDLL(_lib.LIB_PATH)
    BAD = 1
    for name in ENTRIES:
        getattr(c, name).argtypes = _lib.SIGNATURES[name]
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p((ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 2)
    big = 1 << 20
    fwd, bwd = c.fmi_gan_image_head_fwd_f32, c.fmi_gan_image_head_bwd_f32
    ptrs = [p] * 10
    for i in range(10):  # every required pointer: null, then not even float-aligned
        for bad in (None, odd):
            q = list(ptrs)
            q[i] = bad
            assert fwd(*q, 1, 4, 4, 4, 4, 0, p, big, None) == BAD, (i, bad)
    for dims in ((0, 4, 4, 4, 4), (1, 0, 4, 4, 4), (1, 4, -1, 4, 4), (1, 4, 4, 0, 4), (1, 4, 4, 4, 0)):
        assert fwd(*ptrs, *dims, 0, p, big, None) == BAD, dims
    assert fwd(*ptrs, 1, 4, 4, 4, 4, 2, p, big, None) == BAD      # layout flag is 0 or 1
    assert fwd(*ptrs, 1, 4, 4, 4, 4, -1, p, big, None) == BAD
    assert fwd(*ptrs, 1, 4, 4, 4, 4, 0, None, big, None) == BAD   # no scratch
    assert fwd(*ptrs, 1, 4, 4, 4, 4, 0, ctypes.c_void_p(p.value + 4), big, None) == BAD  # scratch not 8-byte aligned
    assert fwd(*ptrs, 1, 4, 4, 4, 4, 0, p, 0, None) == BAD        # scratch smaller than one row
    assert fwd(*ptrs, 3, 4, 4, 4, 4, 0, p, 2, None) == BAD        # one row per workgroup: three samples need three
    bp = [p] * 7
    for i in (0, 1, 2, 3, 6):  # gen, gt, mask, stdv, d_gen are required; gx and g_l1 may be null
        q = list(bp)
        q[i] = None
        assert bwd(*q, 1, 4, 4, 4, 4, 0, None) == BAD, i
    for i in range(7):
        q = list(bp)
        q[i] = odd
        assert bwd(*q, 1, 4, 4, 4, 4, 0, None) == BAD, i
    for dims in ((0, 4, 4, 4, 4), (1, 0, 4, 4, 4), (1, 4, 0, 4, 4), (1, 4, 4, -3, 4), (1, 4, 4, 4, 0)):
        assert bwd(*bp, *dims, 0, None) == BAD, dims
    assert bwd(*bp, 1, 4, 4, 4, 4, 2, None) == BAD


def test_fixture_follows_from_the_definitions(golden):
    """guards the fixture: the float64 values the reference recorded equal the restatement above with DOUBLE weights to 4 U relative to
    the tensor's largest entry, the restatement with lerp_of's fp32 weights is as close to them as the forward bound allows the kernel to
    be (twice the reference's own fp32 error), the masks and shapes are what the issue's table names"""
    fx = golden("ref_train.pt")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_train.pt")) <= 1 << 20
    assert set(fx["head"]) == set(CASES) and set(fx["head_inputs"]) == set(CASES)
    shapes = {k: tuple(fx["head_inputs"][k]["shape"]) + (fx["head_inputs"][k]["vgg_size"],) for k in CASES}
    assert shapes == dict(a=(2, 5, 7, 4), b=(2, 4, 9, 6), c=(1, 6, 8, 8), d=(2, 8, 12, 8), e=(1, 230, 226, 224))
    assert torch.equal(fx["mean"], torch.tensor([0.485, 0.456, 0.406])) and torch.equal(fx["std"], torch.tensor([0.229, 0.224, 0.225]))
    for name in CASES:
        c, cfg = fx["head"][name], fx["head_inputs"][name]
        gen, gt, src, ref, mask = head_inputs(fx, name)
        assert gen.dtype == torch.float32 and 0 <= float(gen.min()) and float(gen.max()) <= 1
        gx, g_l1 = upstream(fx, name)
        n, h, w = cfg["shape"]
        oh, ow = out_size(h, w, cfg["vgg_size"])
        pick = (lambda t: t[:, c["rows"]][:, :, c["cols"]]) if name == "e" else (lambda t: t)
        r64 = restated(gen, gt, src, ref, mask, fx["mean"], fx["std"], cfg["vgg_size"], gx, g_l1, kind="f64")
        r32 = restated(gen, gt, src, ref, mask, fx["mean"], fx["std"], cfg["vgg_size"], gx, g_l1, kind="f32")
        for key in ("x_in", "y_in"):
            rec = c[key + "64"]
            assert rec.dtype == torch.float64 and tuple(pick(r64[key]).shape) == tuple(rec.shape)
            assert float((pick(r64[key]) - rec).abs().max()) <= 4 * U * float(rec.abs().max()), (name, key)
            own = float((c[key].double() - rec).abs().max())
            assert float((pick(r32[key]) - rec).abs().max()) <= 2 * own, (name, key)
        assert abs(r64["l1"] - float(c["l164"])) <= 4 * U * r64["l1"]
        assert abs(float(c["l1"]) - r64["l1"]) <= 4 * U * r64["l1"]  # the reference's own fp32 run is inside the kernel's bound
        if name != "e":
            assert float((r64["grad"] - c["grad64"]).abs().max()) <= 4 * U * float(c["grad64"].abs().max()), name
            assert tuple(c["x_in64"].shape) == (3 * n, oh, ow, 3)
    m = {k: fx["head"][k]["mask"] for k in CASES}
    assert (5 * 7) % 4 and 7 % 4 and 4 % 4 == 0                                                     # (a) scalar backward, odd sizes
    assert shapes["b"][0:3] == (2, 4, 9) and 6 > 4 and 6 < 9                                        # (b) H enlarged, W shrunk
    assert out_size(6, 8, 8) == (6, 8)                                                              # (c) W equal to the size: no resize
    assert set(m["d"][0].unique().tolist()) == {0.0, 0.25, 0.5, 1.0} and float(m["d"][1].min()) == 1  # (d) fractional values; all one
    assert float(m["a"][1].abs().max()) == 0 and set(m["a"][0].unique().tolist()) == {0.0, 1.0}     # the all-zero sample sits in (a)
    assert m["e"].dtype == torch.uint8 and set(m["e"].unique().tolist()) == {0, 1}
    assert 224 * 224 // 4 > 256 * 4                                                                 # (e) several workgroups
    rows = fx["head"]["e"]["rows"].tolist()
    assert rows[0] == 0 and rows[-1] == 223 and set(range(0, 224, 7)) <= set(rows) and rows == fx["head"]["e"]["cols"].tolist()
    assert any(k.startswith("decoder.") for k in fx["keys_G"]) and any(k.startswith("src_encoder.") for k in fx["keys_G"])


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """csrc/ganhead.hip compiled for the host with g++ -DFMI_HOST_THREADS (one OS thread per work-item): the kernels' own source"""
    from face_mask_inpaint_amd import _lib

    csrc = os.path.join(ROOT, "face_mask_inpaint_amd", "csrc")
    so = str(tmp_path_factory.mktemp("ganhead_host") / "libganhead_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wno-unknown-pragmas", "-DFMI_HOST_THREADS",
                           "-x", "c++", os.path.join(csrc, "ganhead.hip"), "-o", so])
    lib = ctypes.CDLL(so)
    for name in ENTRIES:
        getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    return lib


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("name,hwc,misalign", [(n, h, False) for n in SMALL for h in (0, 1)] + [("d", 0, True)])
def test_kernel_source_on_the_host(emu, golden, name, hwc, misalign):
    """the GPU test's checks on cases a-d, met by the kernels' source run on the host; outputs and scratch start as NaN, so anything left
    unwritten shows.  hwc: gen and its gradient in channels-last memory (what ReferenceFill.forward hands over).  misalign: gen starts 4
    bytes past a 16-byte boundary, which sends the four-pixel shape (d) down the one-pixel paths of the L1 sum and of the backward.
    The backward bound's K is backward_k(contributors) -- see there; the worst observed multiples are printed"""
    fx = golden("ref_train.pt")
    c, cfg = fx["head"][name], fx["head_inputs"][name]
    gen, gt, src, ref, mask = head_inputs(fx, name)
    n, h, w = cfg["shape"]
    oh, ow = out_size(h, w, cfg["vgg_size"])
    flat = gen.permute(0, 2, 3, 1).flatten() if hwc else gen.flatten()
    gen_mem = torch.cat([torch.zeros(1), flat])[1:] if misalign else flat.contiguous()  # what the kernel reads
    assert gen_mem.data_ptr() % 16 == (4 if misalign else 0)
    nan = float("nan")
    mean, std = fx["mean"].clone(), fx["std"].clone()
    x_in, y_in = torch.full((3 * n, oh, ow, 3), nan), torch.full((3 * n, oh, ow, 3), nan)
    l1, part = torch.full((1,), nan), torch.full((n * 64,), nan, dtype=torch.float64)
    assert emu.fmi_gan_image_head_fwd_f32(_ptr(gen_mem), _ptr(gt), _ptr(src), _ptr(ref), _ptr(mask), _ptr(mean), _ptr(std), _ptr(x_in), _ptr(y_in), _ptr(l1),
                                          n, h, w, oh, ow, hwc, _ptr(part), part.numel(), None) == 0
    gx, g_l1 = upstream(fx, name)
    g1 = torch.tensor([g_l1], dtype=torch.float32)
    want = restated(gen, gt, src, ref, mask, mean, std, cfg["vgg_size"], gx, float(g1[0]))
    worst = check_forward(x_in, y_in, l1[0], want, c)
    if (oh, ow) == (h, w):  # no resize: the operands are torch's own, bit for bit
        assert torch.equal(x_in[:n], ((gen - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)).permute(0, 2, 3, 1))
    k = backward_k(want["contributors"])
    d_mem = torch.full((gen.numel(),), nan)
    logical = (lambda: d_mem.view(n, h, w, 3).permute(0, 3, 1, 2)) if hwc else (lambda: d_mem.view(n, 3, h, w))
    bwd = lambda g, s: emu.fmi_gan_image_head_bwd_f32(_ptr(gen_mem), _ptr(gt), _ptr(mask), _ptr(std), _ptr(g), _ptr(s), _ptr(d_mem), n, h, w, oh, ow, hwc, None)
    assert bwd(gx, g1) == 0
    worst["grad"] = check_backward(logical(), want, k)
    first = logical().clone()
    # absent upstream gradients equal zero ones
    d_mem.fill_(nan)
    assert bwd(None, g1) == 0
    a = logical().clone()
    d_mem.fill_(nan)
    assert bwd(torch.zeros_like(gx), g1) == 0
    assert torch.equal(a, logical())
    check_backward(a, restated(gen, gt, src, ref, mask, mean, std, cfg["vgg_size"], None, float(g1[0])), k)
    d_mem.fill_(nan)
    assert bwd(gx, None) == 0
    a = logical().clone()
    d_mem.fill_(nan)
    assert bwd(gx, torch.zeros(1)) == 0
    assert torch.equal(a, logical())
    d_mem.fill_(nan)
    assert bwd(gx, g1) == 0 and torch.equal(first, logical())  # and the same bits on a second run
    print(name, "hwc" if hwc else "planar", "K", k, {kk: (vv if isinstance(vv, tuple) else round(vv, 2)) for kk, vv in worst.items()})
