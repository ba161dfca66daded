"""Forward + backward of the decoder's attention at (batch 8, T 16384, d 64, C 256): FF.self_attention (fp32 operands, six bf16 MFMAs
per product, dQ by atomics) against FF.self_attention_bf16_train (one bf16 MFMA per product, two-launch backward without atomics), both
in ONE process, alternating (DESIGN.md "bf16 attention for training"; raw output in profiles/attn_bwd_bf16.txt).
  whole      forward + backward between one pair of device events, PAIRS alternating rounds of TIMED calls after WARM
  per launch each library launch between its own pair of events (functional.PROFILE), median of TIMED passes, with the algorithmic
             TFLOP/s of that launch; casts and other eager glue are the difference to the whole"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from face_mask_inpaint_amd import functional as FF  # noqa: E402

dev = torch.device("cuda:0")
PAIRS, WARM, TIMED = 5, 2, 6
N, T, D, C = 8, 16384, 64, 256


def step(fn, q, v, go):
    q.grad = v.grad = None
    o = fn(q, v)
    o.backward(go)


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


def per_launch(fn):
    rows = {}
    for _ in range(TIMED):
        FF.PROFILE = []
        fn()
        torch.cuda.synchronize()
        for tag, flops, s, e in FF.PROFILE:
            rows.setdefault(tag, (flops, []))[1].append(s.elapsed_time(e))
        FF.PROFILE = None
    for tag, (flops, ms) in rows.items():
        med = statistics.median(ms)
        print(f"  {tag:44s} {med:8.3f} ms  {flops / med / 1e9:8.1f} TFLOP/s")
    return sum(statistics.median(ms) for _, ms in rows.values())


def main():
    g = torch.Generator().manual_seed(0)
    q = (torch.randn(N, T, D, generator=g) * 0.25).to(dev).requires_grad_(True)
    v = torch.randn(N, T, C, generator=g).to(dev).requires_grad_(True)
    go = torch.randn(N, T, C, generator=g).to(dev)
    forms = {"fp32": lambda: step(lambda a, b: FF.self_attention(a, [b])[0], q, v, go),
             "bf16": lambda: step(FF.self_attention_bf16_train, q, v, go)}
    print(f"attention forward + backward at (N, T, d, C) = ({N}, {T}, {D}, {C}) on {torch.cuda.get_device_name(0)}")
    print(f"\n== whole step: {PAIRS} alternating pairs, {TIMED} timed calls after {WARM}, ms (median min) ==")
    meds = {k: [] for k in forms}
    for _ in range(PAIRS):
        for name, fn in forms.items():
            med, lo = timed(fn)
            meds[name].append(med)
            print(f"{name:6s} {med:8.3f} {lo:8.3f}")
    m = {k: statistics.median(x) for k, x in meds.items()}
    print(f"median of medians: fp32 {m['fp32']:.3f} (spread {max(meds['fp32']) - min(meds['fp32']):.3f}), bf16 {m['bf16']:.3f} "
          f"(spread {max(meds['bf16']) - min(meds['bf16']):.3f}); ratio {m['fp32'] / m['bf16']:.2f}; every bf16 run below every fp32 run: "
          f"{max(meds['bf16']) < min(meds['fp32'])}")
    for name, fn in forms.items():
        print(f"\n== per launch, {name}: median of {TIMED} passes ==")
        total = per_launch(fn)
        print(f"  sum of the launches {total:.3f} ms of {m[name]:.3f}")
    # the two forms on the same operands: a sanity line, not a test (tests/test_gpu_attention_bf16_train.py holds the bounds)
    forms["fp32"]()
    g32 = (q.grad.clone(), v.grad.clone())
    forms["bf16"]()
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    print(f"\nbf16 against fp32 gradients, relative L2: q.grad {rel(q.grad, g32[0]):.3e}, v.grad {rel(v.grad, g32[1]):.3e}")


if __name__ == "__main__":
    main()
