"""ReferenceFill forward at 256^2, batch 1 and 8, feature_dtype fp32 against bf16 with the bf16 decoder in both: median of three runs of 50
event-timed iterations after warm-up, the two builds alternating in one process; then fmi_conv2d_c32_fwd_bf16 alone on the encoder's
32-channel layers next to a device copy.  Run from the repository root: python tools/bench_tools/time_picnet_feature.py
(profiles/picnet_enc_bf16.txt holds a recorded run)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from face_mask_inpaint_amd import PICNet_inference as PI
from face_mask_inpaint_amd import functional as FF
from face_mask_inpaint_amd.modules.model import ReferenceFill

dev = torch.device("cuda:0")
BF = torch.bfloat16


def say(s):
    print(s, flush=True)


def timed(fn, iters=50, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


enc, dec = PI.process_params(PI.get_args([]))
torch.manual_seed(0)
models = {}
for name, fdt in (("fp32", torch.float32), ("bf16", BF)):
    models[name] = ReferenceFill(None, dict(enc), dict(dec), decoder_dtype=BF, feature_dtype=fdt).to(dev).eval()
models["bf16"].load_state_dict(models["fp32"].state_dict())
for n in (1, 8):
    g = torch.Generator().manual_seed(1)
    src, ref = torch.rand(n, 3, 256, 256, generator=g).to(dev), torch.rand(n, 3, 256, 256, generator=g).to(dev)
    mask = torch.zeros(n, 256, 256, device=dev)
    mask[:, 100:200, 60:200] = 1
    eps = (torch.randn(n, 128, 32, 32, device=dev), torch.randn(n, 128, 32, 32, device=dev))
    res = {k: [] for k in models}
    with torch.no_grad():
        for rep in range(3):          # alternating builds, three runs each
            for name, G in models.items():
                res[name].append(timed(lambda: G(src, ref, src_mask=mask, eps=eps)))
    for name in models:
        r = res[name]
        say(f"ReferenceFill 256^2 batch {n} feature {name} (decoder bf16): median {statistics.median(r):.3f} ms, runs {['%.3f' % t for t in r]}, "
            f"spread {max(r) - min(r):.3f}")

# the c32 kernel alone: 32 -> 32 and 32 -> 64 at 256^2 and 128^2, batch 8
for (n, h, k) in ((8, 256, 32), (8, 128, 32), (8, 128, 64), (1, 256, 32)):
    x = torch.randn(n, h, h, 32, device=dev).to(BF)
    wf = (torch.randn(9, 32, k, device=dev) * 0.05)
    b = torch.randn(k, device=dev)
    pw = FF.PackedWeight(wf, None, k, 32, 3, 3)
    FF.conv2d_enc_bf16(x, pw, b, 1, 0.1)      # cuts the pack
    r = [timed(lambda: FF.conv2d_enc_bf16(x, pw, b, 1, 0.1)) for _ in range(3)]
    byts = n * h * h * (32 + k) * 2
    say(f"c32 conv 32->{k} at {h}^2 batch {n}: median {statistics.median(r) * 1e3:.1f} us (runs {['%.1f' % (t * 1e3) for t in r]}), "
        f"{byts / 1e6:.1f} MB moved once = {byts / (statistics.median(r) * 1e-3) / 1e12:.2f} TB/s (event-timed, includes launch)")
# a plain device copy of the same bytes for scale
for mb in (67, 201):
    a = torch.empty(mb * 1000 * 1000 // 4, device=dev, dtype=torch.float32)
    c = torch.empty_like(a)
    r = [timed(lambda: c.copy_(a)) for _ in range(3)]
    say(f"torch copy of {mb} MB (read + write {2 * mb} MB): median {statistics.median(r) * 1e3:.1f} us = {2 * mb * 1e6 / (statistics.median(r) * 1e-3) / 1e12:.2f} TB/s")
