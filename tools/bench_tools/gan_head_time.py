"""The image head of GANOptimizer with and without FF.gan_image_head: device time from a kernel trace, and eager wall time.

At the workload's shape, 8 x 3 x 256^2 resized to 224^2 (gen a leaf in channels-last memory, as ReferenceFill.forward hands it over, and,
in the eager mode, once contiguous), the two forms --
    composed  three mask_mul (with their layout round trips), six resize_bilinear, two cat and l1_loss; backwards the three
              resize_bilinear_bwd into zero-filled buffers, the mask adjoints and the adds into gen.grad
    fused     FF.gan_image_head (csrc/ganhead.hip)

  gan_head_time.py [out.json]            eager: the forms are warmed up and ALTERNATED inside one timed loop; a sample is REPS back-to-back
      calls of the forward, or of the forward and the backward (torch.autograd.grad with a fixed upstream gradient of x_in and of l1: no
      op besides the head's own), between two events, divided by REPS.  A bracket holds whatever launch gaps the host leaves: this is
      the time a training step pays, not the kernels' own.  The two forms' values are compared.
  gan_head_time.py steps FORM fwd|fwdbwd   TRACE_STEPS identical calls of one form (the first of them cold) and nothing else of the other: the program to put
      behind ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR --``.
  gan_head_time.py sum STATS.csv          the device time of one call from that run's kernel_stats csv: the total duration of every
      kernel launched at least TRACE_STEPS times (the input set-up launches a handful), divided by TRACE_STEPS, and the launches per
      call -- the kernels' own time, with no host gap in it.  Fills and copies that run as kernels are counted; memset / memcpy
      commands, which the kernel trace does not list, are not.

No speed threshold is asserted."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from face_mask_inpaint_amd import functional as FF  # noqa: E402
from face_mask_inpaint_amd.modules.loss import GANOptimizer  # noqa: E402

REPS, REPLAYS = 20, 30
TRACE_STEPS = 50
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summarise(path):
    import csv

    total, launches = 0.0, 0
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            if int(row["Calls"]) >= TRACE_STEPS:
                total += float(row["TotalDurationNs"])
                launches += int(row["Calls"])
    print(json.dumps(dict(file=os.path.basename(path), device_us_per_call=round(total / TRACE_STEPS / 1e3, 2),
                          launches_per_call=round(launches / TRACE_STEPS, 2), calls=TRACE_STEPS)))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "sum":
        return summarise(sys.argv[2])
    trace = tuple(sys.argv[2:4]) if len(sys.argv) > 3 and sys.argv[1] == "steps" else None
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    n, h, w, size = 8, 256, 256, 224
    mean, std = torch.tensor(MEAN, device=dev), torch.tensor(STD, device=dev)
    gt, src, ref = (torch.rand(n, 3, h, w, device=dev) for _ in range(3))
    mask = torch.zeros(n, h, w, device=dev)
    mask[:, 90:200, 60:190] = 1.0
    gx, g1 = torch.randn(3 * n, size, size, 3, device=dev), torch.tensor(0.7, device=dev)
    res = {}
    for layout in ("nhwc",) if trace else ("nhwc", "planar"):
        gen = torch.rand(n, 3, h, w, device=dev)
        if layout == "nhwc":
            gen = gen.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        gen = gen.detach().requires_grad_(True)
        inp = lambda img: FF.resize_bilinear(FF.to_nhwc(img), size, size, mean, std)

        def composed():
            x = torch.cat([inp(gen), inp(GANOptimizer._masked(gen, mask, True)), inp(GANOptimizer._masked(gen, mask, False))], 0)
            with torch.no_grad():
                y = torch.cat([inp(gt), inp(src), inp(GANOptimizer._masked(ref, mask, False))], 0)
            return x, y, FF.l1_loss(FF.to_nhwc(gen), FF.to_nhwc(gt))

        def fused():
            return FF.gan_image_head(gen, gt, src, ref, mask, mean, std, vgg_size=size)

        forms = {"composed": composed, "fused": fused}

        def step(form, backward):
            x, y, l1 = forms[form]()
            if not backward:
                return x, y, l1, None
            (d,) = torch.autograd.grad([x, l1], [gen], [gx, g1])
            return x, y, l1, d

        if trace:
            for _ in range(TRACE_STEPS):
                step(trace[0], trace[1] == "fwdbwd")
            torch.cuda.synchronize()
            return
        vals = {k: step(k, True) for k in forms}
        diffs = [float((a - b).abs().max()) for a, b in zip(vals["fused"], vals["composed"])]
        assert diffs[0] <= 1e-5 and diffs[1] <= 1e-5 and diffs[2] <= 1e-6 and diffs[3] <= 1e-5 * float(vals["composed"][3].abs().max()) + 1e-7, diffs
        keys = [(form, backward) for form in forms for backward in (False, True)]
        for k in keys:
            for _ in range(3):
                step(*k)
        torch.cuda.synchronize()

        def many(k):
            for _ in range(REPS):
                step(*k)

        ms = {k: [] for k in keys}
        for _ in range(REPLAYS):
            for k in keys:
                ms[k].append(event_ms(lambda: many(k)) / REPS)
        entry = {}
        for form in forms:
            f, fb = ms[(form, False)], ms[(form, True)]
            half = REPLAYS // 2
            entry[form] = dict(fwd_ms=round(statistics.median(f), 5), fwd_bwd_ms=round(statistics.median(fb), 5),
                               bwd_ms=round(statistics.median(fb) - statistics.median(f), 5),
                               fwd_half_medians_ms=[round(statistics.median(f[:half]), 5), round(statistics.median(f[half:]), 5)],
                               fwd_bwd_half_medians_ms=[round(statistics.median(fb[:half]), 5), round(statistics.median(fb[half:]), 5)])
        entry["max_abs_diff_x_y_l1_grad"] = diffs
        res[f"N{n}_{h}to{size}_{layout}"] = entry
    line = json.dumps(dict(gan_head_time=res, reps_per_sample=REPS, samples=REPLAYS))
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
