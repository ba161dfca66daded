"""Eval-mode GradualStyleEncoder(50, "ir_se") forward at full widths, 256^2 on source + reference, 8 + 8 images, body and heads bf16 in
both legs: the fp32 stem and neck (opts.encoder_neck_eval_dtype absent: the form before the option) against the bf16 stem and neck, both
builds in ONE process on the same frozen weights, alternating (DESIGN.md "The bf16 stem and neck (inference)").  Per leg and pair: WARM
untimed forwards, TIMED forwards each between its own pair of device events, the median and the minimum.  Then, per leg, one forward with
a pair of events around every library call: the per-launch table of the stem (the calls in front of the body's first convolution) and of
the neck (the calls behind the body's last tail that are not the heads'), the fused stem's write rate, and the distance of the codes."""
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from face_mask_inpaint_amd import _lib  # noqa: E402
from face_mask_inpaint_amd.modules.psp.encoders.psp_encoders import GradualStyleEncoder  # noqa: E402

dev = torch.device("cuda:0")
PAIRS, WARM, TIMED, REPS = 3, 3, 25, 20
COPY_TBS = 6.29  # the copy figure the project measures bandwidth kernels against (profiles/README.md)


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
    """[(entry, ms)] of one forward, a pair of events around every library call (eager, serialised)"""
    L = _lib.lib()
    recs, saved = [], {}
    for name in _lib.SIGNATURES:
        f = getattr(L, name[4:])
        saved[name[4:]] = f

        def wrapped(*a, _f=f, _n=name):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = _f(*a)
            e.record()
            recs.append((_n, s, e))
            return r

        setattr(L, name[4:], wrapped)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        for k, f in saved.items():
            setattr(L, k, f)
    return [(n, s.elapsed_time(e)) for n, s, e in recs]


def stem_and_neck(recs):
    names = [n for n, _ in recs]
    first_body = names.index("fmi_conv2d_fwd_chan_bf16")
    last_tail = len(names) - 1 - names[::-1].index("fmi_irse_tail_bf16")
    return recs[:first_body], [r for r in recs[last_tail + 1:] if r[0] != "fmi_conv2d_grouped_fwd_bf16"], recs[first_body:last_tail + 1]


def table(title, recs):
    print(f"\n-- {title}: {len(recs)} launches, {sum(ms for _, ms in recs):.3f} ms inside them --")
    for name, ms in recs:
        print(f"{ms:8.3f} ms  {name}")


@torch.no_grad()
def main():
    base = dict(n_styles=18, use_attention=True, encoder_eval_dtype="bf16", style_heads_eval_dtype="bf16")
    opts = {"neck fp32": base, "neck bf16": dict(base, encoder_neck_eval_dtype="bf16"),
            "all fp32": dict(n_styles=18, use_attention=True)}
    encs = {}
    for leg, o in opts.items():
        torch.manual_seed(0)
        enc = GradualStyleEncoder(50, "ir_se", types.SimpleNamespace(**o)).to(dev).eval()
        for p in enc.parameters():  # the inference harness's state: frozen weights keep their packs and folded constants
            p.requires_grad_(False)
        if encs:
            enc.load_state_dict(encs["neck fp32"].state_dict())
        encs[leg] = enc
    g = torch.Generator().manual_seed(0)
    nb = 8
    src, ref = (torch.rand(nb, 3, 256, 256, generator=g) * 2 - 1).to(dev), (torch.rand(nb, 3, 256, 256, generator=g) * 2 - 1).to(dev)
    mask = torch.zeros(nb, 256, 256, device=dev)
    mask[:, 100:220, 60:200] = 1
    run = {leg: (lambda e=e: e(src, ref=ref, mask=mask)) for leg, e in encs.items()}
    legs = ("neck fp32", "neck bf16")
    meds = {leg: [] for leg in legs}
    print(f"== encoder forward, eval, body and heads bf16, {nb} + {nb} images at 256^2: {PAIRS} alternating pairs, {TIMED} timed calls after {WARM}, "
          "ms (median min) ==")
    for _ in range(PAIRS):
        for leg in legs:
            med, lo = timed(run[leg])
            meds[leg].append(med)
            print(f"{leg:10s} {med:8.3f} {lo:8.3f}")
    off, on = meds["neck fp32"], meds["neck bf16"]
    print(f"median of medians: fp32 stem and neck {statistics.median(off):.3f} ms, bf16 stem and neck {statistics.median(on):.3f} ms, "
          f"ratio {statistics.median(off) / statistics.median(on):.2f}")
    print(f"every bf16 run below every fp32 run: {'yes' if max(on) < min(off) else 'NO'} (slowest bf16 {max(on):.3f}, fastest fp32 {min(off):.3f})")
    c_off, c_on, c_32 = run["neck fp32"](), run["neck bf16"](), run["all fp32"]()
    rng = float(c_32.abs().max())
    print(f"W+ codes, range {rng:.4g} (the all-fp32 eval build): max |all-bf16 - all-fp32| = {float((c_on - c_32).abs().max()) / rng:.4g} of it, "
          f"max |body+heads bf16 - all-fp32| = {float((c_off - c_32).abs().max()) / rng:.4g}, "
          f"max |all-bf16 - body+heads bf16| = {float((c_on - c_off).abs().max()) / rng:.4g}")
    for leg in legs:
        run[leg]()
        stem, neck, body = stem_and_neck(per_launch(run[leg]))
        table(f"{leg}: stem", stem)
        table(f"{leg}: neck", neck)
        taps = sum(ms for n, ms in body if n == "fmi_irse_tail_bf16")
        print(f"   (the body's 24 tails, which write the three fp32 taps in the fp32 leg: {taps:.3f} ms)")
    # the fused stem alone, REPS launches back to back between one pair of events: no host gap inside the measurement
    from face_mask_inpaint_amd import functional as FF
    from face_mask_inpaint_amd.modules.psp.encoders import helpers
    from face_mask_inpaint_amd.weights import packed, weight_scope

    enc = encs["neck bf16"]
    x = torch.cat([FF.to_nhwc(src), FF.to_nhwc(ref)], dim=0)
    with weight_scope(enc):
        stem = enc.input_layer
        args = (x, packed(stem[0]), *helpers.fold_bn_eval(stem[1]), stem[2].weight.detach(), *helpers.fold_bn_eval(enc.body[0].res_layer[0]))
        FF.irse_stem_fused_bf16(*args)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(REPS):
            FF.irse_stem_fused_bf16(*args)
        e.record()
        torch.cuda.synchronize()
    ms = s.elapsed_time(e) / REPS
    out_bytes = 2 * (2 * nb) * 256 * 256 * 64 * 2
    print(f"\nfused stem alone, {REPS} launches back to back: {ms:.4f} ms each; {out_bytes / 1e6:.0f} MB written = {out_bytes / ms / 1e9:.2f} TB/s, "
          f"{out_bytes / ms / 1e9 / COPY_TBS:.2f} of the {COPY_TBS} TB/s copy figure")


if __name__ == "__main__":
    main()
