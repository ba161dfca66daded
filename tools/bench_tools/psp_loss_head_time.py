"""pSpLoss.__call__ + backward with and without the fused pixel head (device events; one JSON line, optionally appended to argv[1]).

At 16 x 256^2 and 4 x 256^2 (bench_psp.synth's images and elliptical masks; y_hat a leaf that requires a gradient, in channels-last
memory as pSp.forward's pool hands it over -- "nhwc" -- and, at 16 images, also contiguous -- "planar"), for three sets of lambdas --
    pixel    l2 + l2_ref only: the head by itself
    lpips    l2, l2_ref, LPIPS and LPIPS_ref in the backward
    trainer  train_psp.py's defaults with --use_ref (l2 1, LPIPS 0.8 in the backward; VGG style / contextual evaluated for the log)
-- the two forms ``fused_head = False`` (the composition of to_nhwc / mask_mul / mse_loss / cat) and ``fused_head = True``
(FF.psp_pixel_head) are warmed up separately and then ALTERNATED inside one timed loop, in two blocks: per form the median of all
samples, and the two block medians, whose difference is the run-to-run spread the comparison has to clear.  The launch counts of one
call + backward of each form come from a separate, untimed pass under torch.profiler (device-side events).  The two forms' losses and
gradients are compared (the gradient to 1e-4 of the largest entry: reductions in the LPIPS backward use fp32 atomics, whose order differs
from call to call).  No speed threshold is asserted."""
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bench_psp import synth  # noqa: E402
from face_mask_inpaint_amd.modules.psp.criteria import pSpLoss  # noqa: E402

BASE = dict(id_lambda=0, lpips_lambda=0, l2_lambda=0, style_lambda=0, lpips_lambda_ref=0, l2_lambda_ref=0, cx_lambda=0, w_norm_lambda=0,
            start_from_latent_avg=True)
CONFIGS = {"pixel": dict(l2_lambda=1.0, l2_lambda_ref=1.0),
           "lpips": dict(l2_lambda=1.0, l2_lambda_ref=0.7, lpips_lambda=0.8, lpips_lambda_ref=0.4),
           "trainer": dict(l2_lambda=1.0, lpips_lambda=0.8, style_lambda=250.0, cx_lambda=1.0)}
BLOCKS, PER_BLOCK = 2, 12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def device_ops(fn):
    """device-side events (kernels, fills, copies) of one call, from an untimed profiler pass; None when the profiler gives none"""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if getattr(e.device_type, "name", "") in ("CUDA", "PrivateUse1"))
    return n or None


def main():
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {}
    for cfg_name, lam in CONFIGS.items():
        crit = pSpLoss(types.SimpleNamespace(**{**BASE, **lam})).to(dev)
        crit.defer_logs = True
        for n, layout in ((16, "nhwc"), (4, "nhwc"), (16, "planar")):
            x, ref, y, m = synth(n, dev)
            yh = (y + 0.3 * torch.randn_like(y)).clamp(-1, 1)
            if layout == "nhwc":
                yh = yh.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            yh = yh.detach().requires_grad_(True)
            lat = torch.zeros(n, 14, 512, device=dev)

            def run(fused):
                crit.fused_head = fused
                yh.grad = None
                loss, _, _ = crit(x, y, yh, lat, latent_avg=None, ref=ref, mask=m)
                loss.backward()
                return loss

            vals = {}
            for fused in (False, True):
                for _ in range(3):  # warm-up of every shape, outside the timed window
                    loss = run(fused)
                vals[fused] = (float(loss), yh.grad.clone())
            gdiff = float((vals[True][1] - vals[False][1]).abs().max() / vals[False][1].abs().max())
            ldiff = abs(vals[True][0] - vals[False][0]) / abs(vals[False][0])
            assert gdiff <= 1e-4 and ldiff <= 1e-5, (cfg_name, n, gdiff, ldiff)
            ms = {False: [[] for _ in range(BLOCKS)], True: [[] for _ in range(BLOCKS)]}
            for blk in range(BLOCKS):
                for _ in range(PER_BLOCK):
                    for fused in (False, True):
                        ms[fused][blk].append(event_ms(lambda: run(fused)))
            entry = {}
            for fused, key in ((False, "unfused"), (True, "fused")):
                allv = [v for b in ms[fused] for v in b]
                entry[key + "_ms"] = round(statistics.median(allv), 4)
                entry[key + "_block_medians_ms"] = [round(statistics.median(b), 4) for b in ms[fused]]
                entry[key + "_min_ms"] = round(min(allv), 4)
            try:
                entry["device_ops"] = {"unfused": device_ops(lambda: run(False)), "fused": device_ops(lambda: run(True))}
            except Exception as e:  # the count is a report, not a condition of the timing
                entry["device_ops"] = "not measured: %s" % type(e).__name__
            entry["grad_diff_rel"], entry["loss_diff_rel"] = gdiff, ldiff
            res[f"{cfg_name}_N{n}_{layout}"] = entry
        del crit
        torch.cuda.empty_cache()
    line = json.dumps(dict(psp_loss_head_time=res, samples_per_form=BLOCKS * PER_BLOCK))
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
