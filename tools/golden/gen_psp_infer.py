"""Generator of tests/golden/psp_infer.pt (+ tests/golden/psp_infer_parts/*.pt): the reference's pSp at output_size 1024 (n_styles 18)
in eval mode and its inference harness, run on the CPU from the imported reference.  Run from the repository root:

    python -m tools.golden.gen_psp_infer

Parameters are not stored: both sides fill them with oracle/seeded.py::seeded_fill_.  Everything stored is a plain tensor / number /
string, so the ``golden`` test fixture loads it with ``weights_only=True``.  No committed file may exceed 1 MiB and one pooled image is
768 KiB, so every full image / logit tensor is a file of its own under psp_infer_parts/ and psp_infer.pt holds the rest plus the list
of part names (tests/test_gpu_psp_inference.py::_fixture puts them together again).

Contents
  config      seeds, output_size, mask rectangle, latent_avg seed, detector seed
  att0 / att1 use_attention 0 / 1, batch 1, eval, randomize_noise False, start_from_latent_avg, ref + rectangular src_mask:
              ``codes`` (the encoder's output, latent - latent_avg), ``latent`` (W+ [1, 18, 512]), ``raw`` (digest of the 1024^2 image),
              part ``image_<case>`` (pooled [1, 3, 256, 256]); the same from the reference's float64 run with suffix 64.  One forward
              per run: the 1024^2 image is taken with resize=False and pooled with the model's own ``face_pool``, which is what
              resize=True does to the same tensor (psp.py:113-114).
  noref       use_attention 0 called without ref / mask (psp_inference.py:84-87), through resize=True
  detector    seeded MaskDetector on (src + 1) / 2: output bias (shifted so that both classes occur), argmax mask (uint8), parts
              ``logits`` (fp32 run) and ``logits64_hi`` / ``logits64_lo`` (float64 run split into two float32 tensors, hi + lo)
  infer_batch the reference's own psp_inference.infer_batch on that pair: mask (uint8, equals the detector's argmax), part ``infer_gen``
  tensor2im   a [3, 64, 64] tensor with the edge values and the uint8 results of psp_inference.tensor2im and gradio_serve's
  args        names and defaults of the reference's get_args() with an empty command line
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

from oracle import gen_golden as G
from oracle.seeded import grad_digest, seeded_fill_, seeded_tensor

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests", "golden")
PARTS = "psp_infer_parts"
SEED, AVG_SEED, X_SEED, REF_SEED, MD_SEED = 777, 778, 31, 32, 55
RECT = (120, 230, 60, 200)


def _stub_modules():
    """psp_inference.py / gradio_serve.py / dataloader.py import packages that are absent here and irrelevant to the functions used"""
    def mod(name, **attrs):
        m = sys.modules.get(name) or types.ModuleType(name)
        for k, v in attrs.items():
            if not hasattr(m, k):
                setattr(m, k, v)
        sys.modules[name] = m
        return m

    blank = lambda n: type(n, (), {"__init__": lambda self, *a, **k: None})
    mod("pytorch_msssim", SSIM=blank("SSIM"), MS_SSIM=blank("MS_SSIM"))
    tvt = mod("torchvision.transforms", Normalize=blank("Normalize"))
    mod("torchvision").transforms = tvt
    mod("gradio")


def edge_tensor():
    """[3, 64, 64] fp32: values below -1 / above 1, exactly -1 / 0 / 1, 2k/255 - 1 and k/255 with their fp32 neighbours for every k
    (the points where ``* 255`` followed by truncation changes its result), the rest uniform in [-1.5, 1.5]"""
    k = torch.arange(256, dtype=torch.float64)
    a = (2 * k / 255 - 1).float()
    b = (k / 255).float()
    inf = torch.tensor(float("inf"))
    vals = torch.cat([a, torch.nextafter(a, inf), torch.nextafter(a, -inf), b, torch.nextafter(b, inf), torch.nextafter(b, -inf),
                      torch.tensor([-1.0, 1.0, 0.0, -0.0, -1.5, 1.5, 2.0, -3.0, 1e-8, -1e-8, 0.5, -0.5])])
    t = torch.rand(3 * 64 * 64, generator=torch.Generator().manual_seed(5)) * 3 - 1.5
    pos = torch.randperm(t.numel(), generator=torch.Generator().manual_seed(6))[:vals.numel()]
    t[pos] = vals
    return t.view(3, 64, 64)


def main():
    sg = G._import_stylegan2()  # noqa: F841  (re-binds the native ops of the reference's StyleGAN2 to their own CPU forms)
    _stub_modules()
    from modules.psp import psp as P
    from modules.mask_detector import MaskDetector
    import gradio_serve as GS
    import psp_inference as PI

    P.pSp.load_weights = lambda self: setattr(self, "latent_avg", None)  # the checkpoint files are absent (as in psp_whole_fixture)
    os.makedirs(os.path.join(OUT, PARTS), exist_ok=True)
    parts = {}
    fx = dict(config=dict(seed=SEED, latent_avg_seed=AVG_SEED, output_size=1024, x_seed=X_SEED, ref_seed=REF_SEED, rect=RECT, detector_seed=MD_SEED))
    x = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(X_SEED)) * 2 - 1
    ref = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(REF_SEED)) * 2 - 1
    mask = torch.zeros(1, 256, 256)
    mask[0, RECT[0]:RECT[1], RECT[2]:RECT[3]] = 1

    def make(use_attention, dt):
        opts = types.SimpleNamespace(output_size=1024, encoder_type="GradualStyleEncoder", use_attention=use_attention, train_decoder=False,
                                     start_from_latent_avg=True, learn_in_w=False, pt_ckpt_path=None, stylegan_weights=None)
        net = P.pSp(opts)
        assert opts.n_styles == 18
        seeded_fill_(net, SEED)
        net = net.to(dt).eval()
        net.latent_avg = seeded_tensor((18, 512), AVG_SEED, 0.5).to(dt)
        return net

    net32 = None
    for ua in (0, 1):
        case = fx.setdefault(f"att{ua}", {})
        for dt, sfx in ((torch.float32, ""), (torch.float64, "64")):
            net = make(ua, dt)
            with torch.no_grad():
                codes = net.encoder(x.to(dt), ref=ref.to(dt), mask=mask.to(dt))
                raw, lat = net(x.to(dt), ref=ref.to(dt), src_mask=mask.to(dt), resize=False, randomize_noise=False, return_latents=True)
                img = net.face_pool(raw)
                assert float((lat - (codes + net.latent_avg)).abs().max()) <= 1e-6
                case["codes" + sfx], case["latent" + sfx] = codes.float(), lat.float()
                case["raw" + sfx] = grad_digest(raw.float(), 16384)
                parts[f"image_att{ua}{sfx}"] = img.float().clone()
                if ua == 0:
                    img_n, lat_n = net(x.to(dt), resize=True, randomize_noise=False, return_latents=True)
                    nr = fx.setdefault("noref", {})
                    nr["latent" + sfx] = lat_n.float()
                    parts["image_noref" + sfx] = img_n.float().clone()
            if sfx:
                i32, l32 = parts[f"image_att{ua}"], case["latent"]
                rng = float(img.max() - img.min())
                print(f"att{ua}: pooled range {float(img.min()):.3f} .. {float(img.max()):.3f}; outside [-1, 1] {float((img.abs() > 1).float().mean()):.3f}; "
                      f"W+ std {float(lat.std()):.3f}; fp32 vs fp64 / range: pooled {float((i32.double() - img).abs().max()) / rng:.2e}, "
                      f"1024^2 sample {float((case['raw']['sample'] - case['raw64']['sample']).abs().max()) / float(raw.max() - raw.min()):.2e}, "
                      f"W+ {float((l32.double() - lat).abs().max()) / float(lat.max() - lat.min()):.2e}")
            elif ua == 0:
                net32 = net
            del raw, img
    # ---- mask detector and the reference's infer_batch
    md = MaskDetector(n_channels=3, bilinear=True)
    seeded_fill_(md, MD_SEED)
    md.eval()
    u = (x + 1) / 2
    with torch.no_grad():
        l0 = md(u, mode="train")
        md.model.outc.conv.bias[1] += torch.quantile((l0[:, 0] - l0[:, 1]).flatten(), 0.6)  # both classes occur (as picnet_infer.pt's detector)
        logits = md(u, mode="train")
        md64 = MaskDetector(n_channels=3, bilinear=True)
        md64.load_state_dict(md.state_dict())
        md64 = md64.double().eval()
        logits64 = md64((x.double() + 1) / 2, mode="train")
    am = logits.argmax(1)
    d = (logits64[:, 0] - logits64[:, 1]).abs()
    print("detector: class 1 on %.3f of the pixels; logit0 - logit1 std %.2e; share with |diff| <= 1e-2 / 1e-3 / 1e-4 / 1e-5 = %s; fp32 vs fp64 logits max %.2e"
          % (float(am.float().mean()), float((logits64[:, 0] - logits64[:, 1]).std()), " / ".join("%.4f" % float((d <= t).float().mean()) for t in (1e-2, 1e-3, 1e-4, 1e-5)),
             float((logits.double() - logits64).abs().max())))
    hi = logits64.float()
    parts["logits"], parts["logits64_hi"], parts["logits64_lo"] = logits.clone(), hi, (logits64 - hi.double()).float()
    fx["detector"] = dict(seed=MD_SEED, outc_bias=md.model.outc.conv.bias.detach().clone(), argmax=am.to(torch.uint8))
    gen, m_out = PI.infer_batch(net32, md, (x, ref), torch.device("cpu"))
    assert torch.equal(m_out, am.float())
    fx["infer_batch"] = dict(mask=m_out.to(torch.uint8))
    parts["infer_gen"] = gen.clone()
    # ---- tensor2im, both forms (gradio_serve's writes into its argument: it gets a copy)
    t = edge_tensor()
    fx["tensor2im"] = dict(input=t, psp_inference=torch.from_numpy(np.array(PI.tensor2im(t.clone()))),
                           gradio_serve=torch.from_numpy(np.array(GS.ModelInterface.tensor2im(None, t.clone()))))
    # ---- the reference's command line
    argv, sys.argv = sys.argv, ["psp_inference.py"]
    try:
        a = PI.get_args()
    finally:
        sys.argv = argv
    fx["args"] = [[k, v] for k, v in sorted(vars(a).items())]
    fx["parts"] = sorted(parts)
    total = 0
    for name, tens in parts.items():
        p = os.path.join(OUT, PARTS, name + ".pt")
        torch.save(tens.contiguous(), p)
        total += os.path.getsize(p)
        assert os.path.getsize(p) <= (1 << 20), name
    p = os.path.join(OUT, "psp_infer.pt")
    torch.save(fx, p)
    assert os.path.getsize(p) <= (1 << 20)
    print("psp_infer.pt %.2f MB + %d parts %.2f MB" % (os.path.getsize(p) / 1e6, len(parts), total / 1e6))


if __name__ == "__main__":
    main()
