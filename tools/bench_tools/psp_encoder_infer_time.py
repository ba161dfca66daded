"""Eval-mode GradualStyleEncoder(50, "ir_se") forward at 256^2 on source + reference, 8 + 8 images: the fp32 body against the bf16
inference body (opts.encoder_eval_dtype), both builds in ONE process on the same weights, alternating (DESIGN.md "The bf16 IR-SE
encoder body (inference)").  Per build: WARM untimed forwards, TIMED forwards each between its own pair of device events, the median;
then one forward with functional.PROFILE on and the per-call-site table of the MFMA launches (functional._prof)."""
import collections
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from face_mask_inpaint_amd import functional as FF  # noqa: E402
from face_mask_inpaint_amd.modules.psp.encoders.psp_encoders import GradualStyleEncoder  # noqa: E402

dev = torch.device("cuda:0")
PAIRS, WARM, TIMED = 3, 3, 25


def timed(fn):
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


def table(fn, title):
    FF.PROFILE = []
    fn()
    torch.cuda.synchronize()
    recs, FF.PROFILE = FF.PROFILE, None
    by = collections.OrderedDict()
    for tag, flops, s, e in recs:
        ms = s.elapsed_time(e)
        n, t, f = by.get(tag, (0, 0.0, 0.0))
        by[tag] = (n + 1, t + ms, f + flops)
    total = sum(t for _, t, _ in by.values())
    print(f"\n-- {title}: {len(recs)} profiled launches, {total:.3f} ms inside them (events around every launch: eager, serialised) --")
    for tag, (n, t, f) in sorted(by.items(), key=lambda kv: -kv[1][1]):
        print(f"{t:8.3f} ms  x{n:<3d} {f / t / 1e9 if t > 0 else 0:8.1f} TFLOP/s  {tag}")


@torch.no_grad()
def main():
    encs = {}
    for dt in ("fp32", "bf16"):
        torch.manual_seed(0)
        enc = GradualStyleEncoder(50, "ir_se", types.SimpleNamespace(n_styles=18, use_attention=True, encoder_eval_dtype=dt)).to(dev).eval()
        for p in enc.parameters():  # the inference harness's state: frozen weights keep their packs and folded constants
            p.requires_grad_(False)
        encs[dt] = enc
    encs["bf16"].load_state_dict(encs["fp32"].state_dict())
    g = torch.Generator().manual_seed(0)
    nb = 8
    src, ref = (torch.rand(nb, 3, 256, 256, generator=g) * 2 - 1).to(dev), (torch.rand(nb, 3, 256, 256, generator=g) * 2 - 1).to(dev)
    mask = torch.zeros(nb, 256, 256, device=dev)
    mask[:, 100:220, 60:200] = 1
    run = {dt: (lambda e=e: e(src, ref=ref, mask=mask)) for dt, e in encs.items()}
    meds = {"fp32": [], "bf16": []}
    print(f"== encoder forward, eval, {nb} + {nb} images at 256^2: {PAIRS} alternating pairs, {TIMED} timed calls after {WARM}, ms (median min) ==")
    for _ in range(PAIRS):
        for dt in ("fp32", "bf16"):
            med, lo = timed(run[dt])
            meds[dt].append(med)
            print(f"{dt:5s} {med:8.3f} {lo:8.3f}")
    m32, m16 = statistics.median(meds["fp32"]), statistics.median(meds["bf16"])
    print(f"median of medians: fp32 body {m32:.3f} ms, bf16 body {m16:.3f} ms, ratio {m32 / m16:.2f}")
    c32, c16 = run["fp32"](), run["bf16"]()
    print(f"W+ codes: max |bf16 - fp32| = {float((c16 - c32).abs().max()):.4g} of range {float(c32.abs().max()):.4g}")
    for dt in ("fp32", "bf16"):
        table(run[dt], f"{dt} body")


if __name__ == "__main__":
    main()
