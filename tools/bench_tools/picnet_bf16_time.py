"""The bf16 PICNet decoder against the fp32 one, both builds in ONE process, alternating (DESIGN.md "The bf16 PICNet decoder
(inference)", raw output in profiles/picnet_bf16.txt):
  generator   ReferenceFill forward of PICNet_inference.py's default model at 256^2 input, batch 1 and 8, by device events; SSIM
              between the two builds' images on the harness's synthetic batch (same weights, same eps)
  attention   fmi_attention_fwd_bf16 (with the gamma / residual epilogue) against the fp32 forward at (8, 16384, 64, 256)
  output      the Output block at (8, 1024, 1024, 32): bf16 input against fp32 input
--profile: three bf16 generator forwards at batch 8 and nothing else (the command to put behind rocprofv3 --kernel-trace --stats)."""
import argparse
import copy
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from face_mask_inpaint_amd import PICNet_inference as PI  # noqa: E402
from face_mask_inpaint_amd import functional as FF  # noqa: E402
from face_mask_inpaint_amd.modules.evaluations.ssim import ssim  # noqa: E402

dev = torch.device("cuda:0")
PAIRS, WARM, TIMED = 5, 2, 6


def timed(fn):
    """(median, min) ms of TIMED calls after WARM, each between its own pair of events"""
    for _ in range(WARM):
        fn()
    ms = []
    for _ in range(TIMED):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms), min(ms)


def alternate(title, a, b, names=("fp32", "bf16"), rate=None):
    print(f"\n== {title}: {PAIRS} alternating pairs, {TIMED} timed calls after {WARM}, ms (median min) ==")
    meds = {names[0]: [], names[1]: []}
    for _ in range(PAIRS):
        for name, fn in zip(names, (a, b)):
            med, lo = timed(fn)
            meds[name].append(med)
            print(f"{name:6s} {med:8.3f} {lo:8.3f}" + (f"   {rate[name](med)}" if rate else ""))
    m0, m1 = statistics.median(meds[names[0]]), statistics.median(meds[names[1]])
    sp0, sp1 = max(meds[names[0]]) - min(meds[names[0]]), max(meds[names[1]]) - min(meds[names[1]])
    print(f"median of medians: {names[0]} {m0:.3f} (spread {sp0:.3f}), {names[1]} {m1:.3f} (spread {sp1:.3f}); ratio {m0 / m1:.2f}; "
          f"every {names[1]} run below every {names[0]} run: {max(meds[names[1]]) < min(meds[names[0]])}")
    return m0, m1


def generators():
    gens = {}
    for dt in ("fp32", "bf16"):
        torch.manual_seed(0)
        g, _ = PI.build(PI.get_args(["--generator_dtype", dt]), dev)
        gens[dt] = g
    gens["bf16"].load_state_dict(gens["fp32"].state_dict())
    return gens


def batch(bs):
    g = torch.Generator().manual_seed(0)   # PICNet_inference.main's synthetic batch
    src, ref = torch.rand(bs, 3, 256, 256, generator=g).to(dev), torch.rand(bs, 3, 256, 256, generator=g).to(dev)
    mask = torch.zeros(bs, 256, 256, device=dev)
    mask[:, 120:230, 48:208] = 1.0
    eps = (torch.randn(bs, 128, 32, 32, generator=g).to(dev), torch.randn(bs, 128, 32, 32, generator=g).to(dev))
    return src, ref, mask, eps


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    gens = generators()
    if args.profile:
        src, ref, mask, eps = batch(8)
        for _ in range(3):
            gens["bf16"](src, ref, src_mask=mask, eps=eps)
        torch.cuda.synchronize()
        return
    for bs in (1, 8):
        src, ref, mask, eps = batch(bs)
        run = {dt: (lambda g=g: g(src, ref, src_mask=mask, eps=eps)) for dt, g in gens.items()}
        alternate(f"generator forward, 256^2 input, batch {bs}", run["fp32"], run["bf16"])
        for gamma in (0.0, 0.4):
            sd = copy.deepcopy(gens["fp32"].state_dict())
            for g in gens.values():
                g.decoder.attn1.gamma.fill_(gamma)
            imgs = {}
            for dt, g in gens.items():
                g.load_state_dict(sd)          # the same SpectralNorm state on both sides
                g.decoder.attn1.gamma.fill_(gamma)
                imgs[dt] = g(src, ref, src_mask=mask, eps=eps)
            a, b = imgs["fp32"].clamp(0, 1).contiguous(), imgs["bf16"].clamp(0, 1).contiguous()
            print(f"batch {bs}, attn1.gamma {gamma}: SSIM(fp32 image, bf16 image) = {float(ssim(a, b)):.6f}, max |diff| = "
                  f"{float((imgs['fp32'] - imgs['bf16']).abs().max()):.4f}, rel L2 = "
                  f"{float((imgs['fp32'] - imgs['bf16']).norm() / imgs['fp32'].norm()):.4e}")
        for g in gens.values():
            g.decoder.attn1.gamma.fill_(0.0)

    n, t, d, c = 8, 16384, 64, 256
    q = torch.randn(n, t, d, device=dev) * 0.3
    v = torch.randn(n, t, c, device=dev)
    qb, vb = q.to(torch.bfloat16), v.to(torch.bfloat16)
    gamma = torch.full((1,), 0.4, device=dev)
    fl = 2.0 * n * t * t * (d + c)
    rate = {k: (lambda ms: f"{fl / ms / 1e9:7.1f} TFLOP/s") for k in ("fp32", "bf16")}
    m32, m16 = alternate(f"attention forward at ({n}, {t}, {d}, {c}): FF.self_attention (fp32, key-tile image cut inside) against "
                         "fmi_attention_fwd_bf16 with gamma / residual", lambda: FF.self_attention(q, [v]),
                         lambda: FF.self_attention_bf16(qb, vb, gamma, vb), rate=rate)
    print(f"bf16: {fl / m16 / 1e9:.1f} TFLOP/s = {100 * fl / m16 / 1e9 / 2500:.1f} % of the 2.5 PFLOP/s dense bf16 MFMA peak; fp32: "
          f"{fl / m32 / 1e9:.1f} TFLOP/s of useful work")
    o32 = FF.self_attention(q, [v])[0][0, :256].double()
    o16 = FF.self_attention_bf16(qb, vb)[0, :256].double()
    print(f"bf16 against fp32 on 256 queries: max |diff| {float((o32 - o16).abs().max()):.3e} of max |o| {float(o32.abs().max()):.3e}")
    del q, v, qb, vb

    from face_mask_inpaint_amd.weights import packed, weight_scope

    out = gens["fp32"].decoder.out4
    n, h, w = 8, 1024, 1024
    x = torch.randn(n, h, w, 32, device=dev)
    xb = x.to(torch.bfloat16)
    with weight_scope(out):
        conv = out.conv1.module
        pw = packed(conv)
        by = {"fp32": n * h * w * (32 * 4 + 12), "bf16": n * h * w * (32 * 2 + 12)}
        rate = {k: (lambda ms, k=k: f"{by[k] / ms / 1e9:6.2f} TB/s of {by[k] / 1e6:.0f} MB") for k in by}
        m32, m16 = alternate(f"Output block at ({n}, {h}, {w}, 32)", lambda: FF.lrelu_conv2d(x, pw, conv.bias, 0.1, 1, 1, FF.ACT_TANH),
                             lambda: FF.lrelu_conv2d_thin_bf16(xb, pw, conv.bias, 0.1, 1, FF.ACT_TANH), rate=rate)
    print(f"bf16: {by['bf16'] / m16 / 1e9:.2f} TB/s = {100 * by['bf16'] / m16 / 1e9 / 8.0:.0f} % of the 8.0 TB/s HBM peak "
          f"({100 * by['bf16'] / m16 / 1e9 / 6.29:.0f} % of the 6.29 TB/s a copy reaches); fp32: {by['fp32'] / m32 / 1e9:.2f} TB/s")


if __name__ == "__main__":
    main()
