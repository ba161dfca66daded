"""GPU: the pSp inference path -- the fused image-tail kernel against torch / numpy, the 1024^2 model (n_styles 18, BASELINE configs[4]'s
network) against the imported reference in fp32 and float64 (tests/golden/psp_infer.pt + psp_infer_parts/, tools/golden/gen_psp_infer.py),
psp_inference.infer_batch / main and the single-pair ModelInterface."""
import csv
import itertools
import os
import shutil
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx(golden):
    """psp_infer.pt with its parts (one file per full image: no committed file exceeds 1 MiB) put back under ``parts``"""
    f = dict(golden("psp_infer.pt"))
    f["parts"] = {n: golden(os.path.join("psp_infer_parts", n + ".pt")) for n in f["parts"]}
    return f


def _inputs(cfg, dev):
    x = (torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(cfg["x_seed"])) * 2 - 1).to(dev)
    ref = (torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(cfg["ref_seed"])) * 2 - 1).to(dev)
    mask = torch.zeros(1, 256, 256)
    a, b, c, d = cfg["rect"]
    mask[0, a:b, c:d] = 1
    return x, ref, mask.to(dev)


_NETS = {}


def _net(cfg, use_attention, dtype, dev):
    """pSp(output_size=1024) with the fixture's seeded parameters; the bf16-decoder model takes the fp32 model's state_dict"""
    from face_mask_inpaint_amd.modules.psp.psp import pSp
    from oracle.seeded import seeded_fill_, seeded_tensor  # checker

    key = (use_attention, dtype)
    if key not in _NETS:
        opts = types.SimpleNamespace(output_size=cfg["output_size"], encoder_type="GradualStyleEncoder", use_attention=use_attention, train_decoder=False,
                                     start_from_latent_avg=True, learn_in_w=False, pt_ckpt_path=None, stylegan_weights=None, decoder_dtype=dtype)
        net = pSp(opts)
        assert opts.n_styles == 18 and len(net.encoder.styles) == 18 and net.decoder.n_latent == 18
        if dtype == "fp32":
            seeded_fill_(net, cfg["seed"])
        else:
            net.load_state_dict(_net(cfg, use_attention, "fp32", dev).state_dict())
        net.latent_avg = seeded_tensor((18, 512), cfg["latent_avg_seed"], 0.5)
        _NETS[key] = net.to(dev).eval()
    return _NETS[key]


def _rel(got, want, scale=None):
    want = want.to(got.device) if torch.is_tensor(want) else want
    return float((got.double() - want.double()).abs().max()) / (float(want.abs().max()) if scale is None else scale)


def _host_u8(pooled_cpu, form):
    from face_mask_inpaint_amd.psp_inference import tensor2im, tensor2im_unit

    f = (lambda t: np.array(tensor2im(t))) if form == (1.0, 0.5) else tensor2im_unit
    return torch.from_numpy(np.stack([f(p) for p in pooled_cpu]))


def test_image_tail_kernel_against_torch(dev, fx):
    """fmi_image_tail_f32 / fmi_planes_to_u8_f32: pooled at the existing pool's bound, everything downstream of ``pooled`` bit exact"""
    from face_mask_inpaint_amd import functional as FF
    from face_mask_inpaint_amd.psp_inference import tensor2im, tensor2im_unit

    edge = fx["tensor2im"]["input"].flatten()
    edge = edge[torch.randperm(edge.numel(), generator=torch.Generator().manual_seed(1))[:4096]]
    g = torch.Generator().manual_seed(0)
    for s, n in itertools.product((256, 512, 1024), (1, 3)):
        f = s // 256
        x = torch.rand(n, s, s, 3, generator=g) * 3 - 1.5
        # the edge values planted as whole f x f windows, so that the POOLED value sits on / next to tensor2im's decision points
        pos = torch.randperm(n * 256 * 256 * 3, generator=g)[:edge.numel()]
        xw = x.view(n, 256, f, 256, f, 3).permute(0, 1, 3, 5, 2, 4).reshape(-1, f, f).clone()
        xw[pos] = edge.view(-1, 1, 1).expand(-1, f, f)
        x = xw.view(n, 256, 256, 3, f, f).permute(0, 1, 4, 2, 5, 3).reshape(n, s, s, 3).contiguous()
        xd = x.to(dev)
        full = FF.image_tail(xd)
        assert set(full) == {"pooled", "unit", "u8"}
        pooled = full["pooled"].cpu()
        assert pooled.shape == (n, 3, 256, 256) and full["u8"].shape == (n, 256, 256, 3) and full["u8"].dtype == torch.uint8
        want = torch.nn.functional.adaptive_avg_pool2d(x.permute(0, 3, 1, 2), (256, 256))
        torch.testing.assert_close(pooled, want, rtol=1e-5, atol=1e-6)
        if f == 1:
            assert torch.equal(pooled, want)  # a plain transposition
        assert torch.equal(full["unit"].cpu(), (pooled + 1) / 2)
        assert torch.equal(full["u8"].cpu(), _host_u8(pooled, (1.0, 0.5)))
        alt = FF.image_tail(xd, want=("pooled", "u8"), shift=0.0, scale=1.0)
        assert torch.equal(alt["pooled"].cpu(), pooled) and torch.equal(alt["u8"].cpu(), _host_u8(pooled, (0.0, 1.0)))
        assert len(torch.unique(full["u8"])) == 256
        for k in (1, 2):
            for sub in itertools.combinations(("pooled", "unit", "u8"), k):
                part = FF.image_tail(xd, want=sub)
                assert set(part) == set(sub) and all(torch.equal(part[w], full[w]) for w in sub), sub
        again = FF.image_tail(xd)
        assert all(torch.equal(again[w], full[w]) for w in full)
    # ---- the detected mask and the planar form (vector path: H * W % 4 == 0; one pixel per thread otherwise)
    for shape in ((2, 256, 256), (3, 37, 53)):
        m = (torch.rand(shape, generator=g) < 0.4).float()
        got = FF.mask_to_u8(m.to(dev)).cpu()
        assert got.shape == shape + (3,) and sorted(torch.unique(got).tolist()) == [127, 255]  # the (x + 1) / 2 inside tensor2im: 0 -> 127
        assert torch.equal(got, torch.from_numpy(np.stack([np.array(tensor2im(v.repeat(3, 1, 1))) for v in m])))
        assert torch.equal(got[..., 0] == 255, m == 1)
        got = FF.mask_to_u8(m.to(dev), 0.0, 1.0).cpu()
        assert sorted(torch.unique(got).tolist()) == [0, 255] and torch.equal(got, torch.from_numpy(np.stack([tensor2im_unit(v.repeat(3, 1, 1)) for v in m])))
        t = torch.rand((shape[0], 3) + shape[1:], generator=g) * 3 - 1.5
        t.view(-1)[torch.randperm(t.numel(), generator=g)[:1500]] = edge[:1500]
        for form in ((0.0, 1.0), (1.0, 0.5)):
            got = FF.planes_to_u8(t.to(dev), *form)
            assert torch.equal(got.cpu(), _host_u8(t, form)) and torch.equal(got, FF.planes_to_u8(t.to(dev), *form))
    with pytest.raises(FF.FmiError):
        FF.image_tail(torch.zeros(1, 256, 256, 3, device=dev, requires_grad=True))  # inference only
    with pytest.raises(FF.FmiError):
        FF.image_tail(torch.zeros(1, 384, 384, 3, device=dev))  # other sizes keep the existing pool


@pytest.mark.parametrize("use_attention", (0, 1))
def test_c5_model_against_the_reference(dev, fx, use_attention):
    """pSp(output_size=1024), n_styles 18, eval, fixed noise, ref + rectangular mask -- through forward(resize=True), forward(resize=False)
    and the new infer path, against the reference's fp32 run at the project's bounds (encoder codes 1e-3 of their own largest entry, W+
    codes 1e-4, images 1e-3); the error against the reference's FLOAT64 run is printed next to the reference's own fp32 error."""
    from face_mask_inpaint_amd import functional as FF
    from oracle.seeded import check_digest, digest_error  # checker

    cfg, case, P = fx["config"], fx[f"att{use_attention}"], fx["parts"]
    net = _net(cfg, use_attention, "fp32", dev)
    x, ref, mask = _inputs(cfg, dev)
    img_ref, img64 = P[f"image_att{use_attention}"], P[f"image_att{use_attention}64"]
    rng = float(img64.max() - img64.min())
    with torch.no_grad():
        codes = net.encoder(x, ref=ref, mask=mask)
        img, lat = net(x, ref=ref, src_mask=mask, resize=True, randomize_noise=False, return_latents=True)
        raw = net(x, ref=ref, src_mask=mask, resize=False, randomize_noise=False)
        out, lat_i = net.infer(x, ref=ref, src_mask=mask)
    assert lat.shape == (1, 18, 512) and img.shape == (1, 3, 256, 256) and raw.shape == (1, 3, 1024, 1024)
    print("\nC5 model, use_attention %d, error / reference's own fp32 error, both against float64:" % use_attention)
    print("  encoder codes (of max)  %.2e / %.2e" % (_rel(codes, case["codes64"]), _rel(case["codes"], case["codes64"])))
    print("  W+ codes (of max)       %.2e / %.2e" % (_rel(lat, case["latent64"]), _rel(case["latent"], case["latent64"])))
    print("  pooled image (of range) forward %.2e, infer %.2e / %.2e" % (_rel(img, img64, rng), _rel(out["pooled"], img64, rng), _rel(img_ref, img64, rng)))
    print("  1024^2 image (sampled, of max) %.2e / %.2e" % (digest_error(raw, case["raw64"]), digest_error(case["raw"]["sample"], dict(case["raw64"], step=torch.tensor(1)))))
    assert _rel(codes, case["codes"]) <= 1e-3
    for l in (lat, lat_i):
        assert _rel(l, case["latent"]) <= 1e-4
    for im in (img, out["pooled"]):
        assert _rel(im, img_ref) <= 1e-3
    check_digest(raw, case["raw"], 1e-3, "1024^2 image")
    with FF.deterministic(True), torch.no_grad():  # two forwards are bit-identical up to the tail: the two tails against each other
        a = net(x, ref=ref, src_mask=mask, resize=True, randomize_noise=False)
        b, _ = net.infer(x, ref=ref, src_mask=mask)
        torch.testing.assert_close(b["pooled"], a.contiguous(), rtol=1e-5, atol=1e-6)
        if use_attention == 0:
            an, latn = net(x, resize=True, randomize_noise=False, return_latents=True)
            bn, _ = net.infer(x)
            torch.testing.assert_close(bn["pooled"], an.contiguous(), rtol=1e-5, atol=1e-6)
    if use_attention == 0:  # the call without ref / mask (psp_inference.py:84-87)
        nr = fx["noref"]
        print("  no ref: pooled image (of range) %.2e / %.2e" % (_rel(bn["pooled"], P["image_noref64"], rng), _rel(P["image_noref"], P["image_noref64"], rng)))
        assert _rel(latn, nr["latent"]) <= 1e-4
        for im in (an, bn["pooled"]):
            assert _rel(im, P["image_noref"]) <= 1e-3


@pytest.mark.parametrize("use_attention", (0, 1))
def test_c5_model_with_the_bf16_decoder(dev, fx, use_attention):
    """decoder_dtype='bf16' (the C5 configuration) on the same inputs against the reference's float64 pooled image.  No reference bf16
    run exists; the bound is the one the project holds its 1024^2 bf16 decoder to against its own fp32 form (5e-2 of the image range,
    tests/test_gpu_fullsize.py::test_bf16_decoder_1024_tracks_fp32)."""
    cfg, P = fx["config"], fx["parts"]
    net = _net(cfg, use_attention, "bf16", dev)
    assert net.decoder.compute_dtype == torch.bfloat16
    x, ref, mask = _inputs(cfg, dev)
    img64 = P[f"image_att{use_attention}64"]
    rng = float(img64.max() - img64.min())
    out, lat = net.infer(x, ref=ref, src_mask=mask)
    with torch.no_grad():
        img = net(x, ref=ref, src_mask=mask, resize=True, randomize_noise=False)
    err = _rel(out["pooled"], img64, rng)
    print("\nC5 model, bf16 decoder, use_attention %d: pooled image error against float64 %.2e of the range (forward path %.2e)" % (use_attention, err, _rel(img, img64, rng)))
    assert _rel(lat, fx[f"att{use_attention}"]["latent"]) <= 1e-4  # the encoder stays fp32
    assert err <= 5e-2 and _rel(img, img64, rng) <= 5e-2


class GoldenMask:
    """stands in for the detector with the reference's own argmax, so that a tied pixel does not decide whether the image is compared"""

    def __init__(self, mask):
        self.mask = mask

    def predict_mask(self, src):
        return self.mask.to(src.device)


def test_mask_detector_and_infer_batch(dev, fx):
    """psp_inference.infer_batch: MaskDetector((src + 1) / 2).argmax -> pSp(src, ref, src_mask).  A seeded UNet's two logits differ by
    4e-3 (std), so the margin outside which the masks must agree is not fixed in advance: it is four times the measured error of the HIP
    logits against the reference's float64 logits, and at most 5 % of the pixels may fall inside it."""
    from face_mask_inpaint_amd.modules.mask_detector import MaskDetector
    from face_mask_inpaint_amd.psp_inference import infer_batch
    from oracle.seeded import seeded_fill_  # checker

    cfg, d, P = fx["config"], fx["detector"], fx["parts"]
    md = MaskDetector(n_channels=3, bilinear=True)
    seeded_fill_(md, d["seed"])
    with torch.no_grad():
        md.model.outc.conv.bias.copy_(d["outc_bias"])
    md = md.to(dev).eval()
    x, ref, _ = _inputs(cfg, dev)
    with torch.no_grad():
        logits = md((x + 1) / 2, mode="train").cpu()
        am = md.predict_mask((x + 1) / 2).cpu()
    l64 = P["logits64_hi"].double() + P["logits64_lo"].double()
    e = float((logits.double() - l64).abs().max())
    e_ref = float((P["logits"].double() - l64).abs().max())
    m = 4 * e
    gap = (l64[:, 0] - l64[:, 1]).abs()
    inside = float((gap <= m).float().mean())
    print("\nmask detector: HIP logits against float64 max %.2e (the reference's fp32 run: %.2e); margin %.2e holds %.4f of the pixels" % (e, e_ref, m, inside))
    assert e <= 1e-3  # the project's bound on the UNet logits, here only a sanity check
    want = d["argmax"].float()
    sure = gap > m
    assert torch.equal(am[sure], want[sure])
    assert inside <= 0.05
    for cls in (0.0, 1.0):
        assert float((want == cls).float().mean()) >= 0.2 and float((want[sure] == cls).float().mean()) >= 0.2
    net = _net(cfg, 0, "fp32", dev)
    gen, mask = infer_batch(net, md, (x.cpu(), ref.cpu()), dev)
    assert gen.is_cuda and not mask.is_cuda and mask.shape == (1, 256, 256) and torch.equal(mask[sure], want[sure])
    golden_mask = fx["infer_batch"]["mask"].float()
    gen, mask = infer_batch(net, GoldenMask(golden_mask), (x.cpu(), ref.cpu()), dev)
    assert torch.equal(mask, golden_mask)
    assert _rel(gen, P["infer_gen"]) <= 1e-3
    out, _ = infer_batch(net, GoldenMask(golden_mask), (x.cpu(), ref.cpu()), dev, want=("pooled", "unit", "u8"))
    assert _rel(out["pooled"], P["infer_gen"]) <= 1e-3 and torch.equal(out["unit"], (out["pooled"] + 1) / 2)
    assert torch.equal(out["u8"].cpu(), _host_u8(out["pooled"].cpu(), (1.0, 0.5)))
    gen, mask = infer_batch(net, md, (x.cpu(),), dev)  # no ref: no mask is computed
    assert mask is None and _rel(gen, P["image_noref"]) <= 1e-3


def _enlarged_dataset(tmp_path):
    """a copy of tests/golden/dataset under tmp_path (use_ssim=True writes best_reference_map.json next to the source directory: nothing
    may be written into the repository).  The harness reads CelebA-HQ files and scales them by the reference's fixed 0.25 to the encoder's
    256 x 256 input; the golden files are 40 x 48, so the copies are enlarged to 1024 x 1024."""
    from PIL import Image

    root = str(tmp_path / "dataset")
    shutil.copytree(os.path.join(ROOT, "tests", "golden", "dataset"), root)
    for sub in ("images", "images_masked"):
        for f in os.listdir(os.path.join(root, sub)):
            p = os.path.join(root, sub, f)
            Image.open(p).convert("RGB").resize((1024, 1024), Image.BICUBIC).save(p, quality=95)
    for f in os.listdir(os.path.join(root, "binary_map")):
        p = os.path.join(root, "binary_map", f)
        np.save(p, np.asarray(Image.fromarray(np.load(p)).resize((1024, 1024), Image.NEAREST)))
    return root


def test_harness_end_to_end(dev, tmp_path):
    """psp_inference.main on the (enlarged) golden dataset with a ragged last batch: one picture and one mask per id, metrics.csv, and the
    returned SSIM / MS-SSIM against the CPU restatements of the valid-window definition (oracle/msssim_cpu.py: ``ssim`` and ``ms_ssim``;
    oracle/ssim_cpu.py is the zero-padded in-repo SSIM, a different metric) at the bounds of test_c1_harness_runs_at_full_size.  Then
    the synthetic mode at the default 1024^2 for both decoder types."""
    from PIL import Image

    from face_mask_inpaint_amd import functional as FF
    from face_mask_inpaint_amd import psp_inference as PI
    from face_mask_inpaint_amd.dataloader import DeviceLoader, ReferenceDataset
    from oracle import msssim_cpu  # checker

    root, out_dir = _enlarged_dataset(tmp_path), str(tmp_path / "out")
    argv = ["--data_root", root, "--src_img_path", "images_masked", "--identity_file_path", "identity.txt", "--output_size", "256", "--batch_size", "3",
            "--use_ref", "--save_src_mask", "1", "--out_dir", out_dir]
    with FF.deterministic(True):  # the recomputation below then sees the same bits
        torch.manual_seed(3)
        ssim, ms = PI.main(argv)
        torch.manual_seed(3)
        args = PI.get_args(argv)
        G, md = PI.build(args, dev)
        j = lambda p: os.path.join(root, p)
        ds = ReferenceDataset(j("images_masked"), j("images"), j("binary_map"), j("identity.txt"), apply_transform=True, scale=0.25, use_ssim=True, device=dev, return_id=True)
        assert len(ds) % 3 != 0  # the last batch is ragged
        ids, per_batch = [], []
        for batch in DeviceLoader(ds, range(len(ds)), 3, shuffle=False, drop_last=False):
            out, mask = PI.infer_batch(G, md, (batch["src_img"], batch["ref_img"]), dev, want=("pooled", "unit"))
            assert out["unit"].shape[1:] == (3, 256, 256) and mask.shape[1:] == (256, 256)
            gt, unit = batch["raw_gt_img"].cpu().double(), out["unit"].cpu().double()
            per_batch.append((float(msssim_cpu.ssim(gt, unit)), float(msssim_cpu.ms_ssim(gt, unit))))
            ids += batch["id"].view(-1).tolist()
    assert len(per_batch) == 3 and len(ids) == len(ds)
    want = np.array(per_batch).mean(0)  # over batches, as the reference does
    print("\nharness: ssim %.6f (oracle %.6f), ms_ssim %.6f (oracle %.6f)" % (ssim, want[0], ms, want[1]))
    assert abs(ssim - want[0]) <= 1e-5 and abs(ms - want[1]) <= 2e-5
    assert sorted(os.listdir(out_dir)) == sorted(["metrics.csv"] + [f"gen_{i}.jpg" for i in ids] + [f"mask_{i}.jpg" for i in ids])
    for f in os.listdir(out_dir):
        if f.endswith(".jpg"):
            im = Image.open(os.path.join(out_dir, f))
            assert im.size == (256, 256) and im.mode == "RGB", f
    rows = list(csv.reader(open(os.path.join(out_dir, "metrics.csv"))))
    assert rows[0] == ["ssim", "ms_ssim"] and len(rows) == 2 and (float(rows[1][0]), float(rows[1][1])) == (ssim, ms)
    assert not os.path.exists(os.path.join(ROOT, "tests", "golden", "best_reference_map.json"))
    for dt in ("fp32", "bf16"):
        o = str(tmp_path / ("syn_" + dt))
        s, m = PI.main(["--batch_size", "1", "--num_batches", "1", "--decoder_dtype", dt, "--out_dir", o])  # output_size 1024, no ref
        assert s == s and m == m and -1.0 <= s <= 1.0 and -1.0 <= m <= 1.0
        assert sorted(os.listdir(o)) == ["gen_0.jpg", "metrics.csv"]


def test_mean_latent_default(dev):
    """without a stored latent_avg ``build`` takes the mean of 1e5 mapped latents (psp_inference.py:139-140), a [512] vector that the
    codes' addition broadcasts over the styles"""
    from face_mask_inpaint_amd import psp_inference as PI

    torch.manual_seed(11)
    G, _ = PI.build(PI.get_args(["--output_size", "256"]), dev)
    assert G.latent_avg.shape == (512,) and not G.latent_avg.requires_grad
    torch.manual_seed(11)  # the device generator restarts: the same draw of z (building the modules draws from the host generator only)
    z = torch.randn(int(1e5), 512, device=dev)
    with torch.no_grad():
        want = G.decoder.get_latent(z).mean(0)
    torch.testing.assert_close(G.latent_avg, want, rtol=1e-5, atol=1e-5)
    x = torch.rand(2, 3, 256, 256, device=dev) * 2 - 1
    out, lat = G.infer(x)
    with torch.no_grad():
        codes = G.encoder(x)
    torch.testing.assert_close(lat, codes + G.latent_avg.view(1, 1, 512), rtol=1e-5, atol=1e-5)
    assert lat.shape == (2, 14, 512) and bool(torch.isfinite(out["pooled"]).all())


def test_model_interface(dev):
    """gradio_serve.ModelInterface without gradio: Pillow-exact preprocessing to 256 x 256 from any aspect ratio, and ``infer`` equal to
    the composition of its parts with the host tensor2im"""
    from PIL import Image

    from face_mask_inpaint_amd import functional as FF
    from face_mask_inpaint_amd import psp_inference as PI
    from face_mask_inpaint_amd.modules.model import scale_img

    torch.manual_seed(5)
    mi = PI.ModelInterface(PI.get_args([]), dev)
    assert mi.generator.opts.output_size == 1024 and mi.generator.latent_avg.shape == (512,)
    d = os.path.join(ROOT, "tests", "golden", "dataset")
    crop = Image.open(os.path.join(d, "images", "103.jpg")).convert("RGB").crop((3, 5, 40, 44))  # 37 x 39
    assert crop.size == (37, 39)
    for pil in (crop, crop.resize((301, 77), Image.BICUBIC)):  # enlarged on both axes / reduced on one
        t, size = mi.preprocess_img(pil)
        a = np.asarray(pil.resize((256, 256), resample=Image.BICUBIC)).transpose((2, 0, 1)) / 255
        want = (torch.as_tensor(a.copy()).float() - 0.5) / 0.5
        assert size == (pil.size[1], pil.size[0]) and t.shape == (1, 3, 256, 256) and torch.equal(t.cpu()[0], want)
    src = Image.open(os.path.join(d, "images_masked", "103_surgical.jpg")).convert("RGB").resize((150, 203), Image.BICUBIC)
    ref = Image.open(os.path.join(d, "images", "104.jpg")).convert("RGB").resize((97, 61), Image.BICUBIC)
    s, size = mi.preprocess_img(src)
    with torch.no_grad():  # a random detector predicts one class nearly everywhere: shift its output bias so that both occur on this image
        l = mi.mask_detector((s + 1) / 2, mode="train")
        mi.mask_detector.model.outc.conv.bias[1] += torch.quantile((l[:, 0] - l[:, 1]).flatten(), 0.5)
    with FF.deterministic(True), torch.no_grad():
        gen, mask = mi.infer(src, ref)
        r, _ = mi.preprocess_img(ref)
        g, m = mi.infer_image(s, r)
        g = scale_img((g + 1) / 2, size)
        m3 = scale_img(m.repeat(3, 1, 1).unsqueeze(0).contiguous(), size)
    assert size == (203, 150)
    for got in (gen, mask):
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (203, 150, 3)
    assert np.array_equal(gen, PI.tensor2im_unit(g[0].cpu())) and np.array_equal(mask, PI.tensor2im_unit(m3[0].cpu()))
    assert mask.min() == 0 and mask.max() == 255 and np.array_equal(mask[..., 0], mask[..., 1]) and np.array_equal(mask[..., 0], mask[..., 2])
