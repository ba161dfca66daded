"""Per-entry time of the per-channel kernels of csrc/chan.hip at the IR-SE body's shapes (16 x 128 x 128 x 64 and 16 x 16 x 16 x 512), fp32 and
bf16, raw entries on preallocated tensors: median over REPS windows of LOOP launches between device events, in us per launch.  The
library is the one FMI_LIB_PATH names (tools/bench_tools/ab.sh alternates builds).  Prints one line: entry=us ..."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from face_mask_inpaint_amd import functional as FF, _lib  # noqa: E402

dev = torch.device("cuda:0")
WARM, REPS, LOOP = 3, 15, 50
lib, P, st = _lib.lib(), FF._p, FF._st


def time_us(call):
    for _ in range(WARM * LOOP):
        call()
    ms = []
    for _ in range(REPS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(LOOP):
            call()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms) * 1000.0 / LOOP


out = []
for n, h, c in ((16, 128, 64), (16, 16, 512)):
    p = h * h
    for dt, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        x, r = torch.randn(n, p, c, device=dev).to(dt), torch.randn(n, p, c, device=dev).to(dt)
        y, g = torch.empty_like(x), torch.empty_like(x)
        s, a = torch.rand(n, c, device=dev) + 0.5, torch.rand(c, device=dev) * 0.5
        sub = torch.empty(n, (h // 2) ** 2, c, device=dev, dtype=dt)
        ws = torch.empty(1024 * c, device=dev)
        ga = torch.empty(c, device=dev)
        entries = {
            "scale": lambda: getattr(lib, "scale_channels_" + tag)(P(x), P(s), P(y), n, p, c, st()),
            "scale_add": lambda: getattr(lib, "scale_channels_add_" + tag)(P(x), P(s), P(r), P(y), n, p, c, st()),
            "prelu": lambda: getattr(lib, "prelu_" + tag)(P(x), P(a), P(y), n * p, c, st()),
            "add_bcast": lambda: getattr(lib, "add_bcast_" + tag)(P(x), P(s), P(y), n, p, c, st()),
            "subsample": lambda: getattr(lib, "subsample_" + tag)(P(x), P(sub), n, h, h, c, 2, 0, st()),
            "subsample_bwd": lambda: getattr(lib, "subsample_" + tag)(P(sub), P(y), n, h, h, c, 2, 1, st()),
            "prelu_bwd": lambda: getattr(lib, "prelu_bwd_" + tag)(P(g), P(x), P(a), P(y), P(ga), P(ws), 512 * c, n * p, c, st()),  # + sum_parts / sum_rows
        }
        for name, call in entries.items():
            out.append(f"{name}_{tag}_{h}x{c}={time_us(call):.2f}")
print(" ".join(out))
