"""Time of the pSp encoder's head section -- FPN merges + map2style heads from given level maps c1, c2, c3 -- at full widths, batch 8,
n_styles 18 and 14, for style_heads_eval_dtype fp32 and bf16.  Both options run in ONE process, alternating call by call, frozen weights
(as psp_inference.build leaves them), each call between two device events: WARM warm-up and REPS timed repetitions per option.  Prints per
n_styles the medians, the spread (min .. max), the ratio and the library calls of one head section.  The library is the one FMI_LIB_PATH
names (an experimental build with another FMI_STYLE_SKINNY_ROWS, say)."""
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from face_mask_inpaint_amd import functional as FF, _lib  # noqa: E402
from face_mask_inpaint_amd.modules.psp.encoders.psp_encoders import GradualStyleEncoder  # noqa: E402
from face_mask_inpaint_amd.weights import weight_scope  # noqa: E402

dev = torch.device("cuda:0")
WARM, REPS, BATCH = 5, 20, 8


def build(n_styles, dtype):
    torch.manual_seed(0)
    enc = GradualStyleEncoder(50, "ir_se", SimpleNamespace(n_styles=n_styles, use_attention=0, style_heads_eval_dtype=dtype))
    for p in enc.parameters():
        p.requires_grad_(False)
    return enc.to(dev).eval()


def section(enc, maps):
    with torch.no_grad(), weight_scope(enc):
        return enc._latents(*maps)


def count_calls(enc, maps):
    L, calls, saved = _lib.lib(), [], {}
    for name in _lib.SIGNATURES:
        saved[name] = getattr(L, name[4:])
        setattr(L, name[4:], (lambda f, nm: lambda *a: (calls.append(nm), f(*a))[1])(saved[name], name))
    try:
        section(enc, maps)
    finally:
        for name, fn in saved.items():
            setattr(L, name[4:], fn)
    return calls


gen = torch.Generator().manual_seed(1)
maps = tuple(torch.randn(BATCH, s, s, c, generator=gen).to(dev) for s, c in ((64, 128), (32, 256), (16, 512)))
for n_styles in (18, 14):
    encs = {"fp32": build(n_styles, "fp32"), "bf16": build(n_styles, "bf16")}
    out = {k: section(e, maps) for k, e in encs.items()}  # packs are made here
    torch.cuda.synchronize()
    diff = float((out["bf16"] - out["fp32"]).abs().max()) / float(out["fp32"].abs().max())
    calls = {k: count_calls(e, maps) for k, e in encs.items()}
    ms = {"fp32": [], "bf16": []}
    for rep in range(WARM + REPS):
        for k, e in encs.items():
            s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            section(e, maps)
            t.record()
            torch.cuda.synchronize()
            if rep >= WARM:
                ms[k].append(s.elapsed_time(t))
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k in ("fp32", "bf16"):
        grouped = calls[k].count("fmi_conv2d_grouped_fwd_bf16")
        print(f"n_styles {n_styles} batch {BATCH} heads {k}: median {med[k]:.3f} ms  min {min(ms[k]):.3f}  max {max(ms[k]):.3f}  "
              f"library calls {len(calls[k])} (grouped convolutions {grouped}, merges {calls[k].count('fmi_fpn_merge_bf16')})")
    print(f"n_styles {n_styles}: fp32 / bf16 = {med['fp32'] / med['bf16']:.2f}  max |bf16 - fp32| = {diff:.3g} of the codes' range  "
          f"FMI_STYLE_SKINNY_ROWS as built, Python side {FF.STYLE_SKINNY_ROWS}")
    del encs, out
    torch.cuda.empty_cache()
