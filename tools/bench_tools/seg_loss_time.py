"""The mask-detector trainer's loss and step (device events; one JSON line, optionally appended to the file given as argv[1]).

(1) loss forward + backward on the same NHWC logits at 1 x 1024^2 and 8 x 1024^2, two forms alternated inside ONE timed loop after a
    separate warm-up of both (so that clock state and allocator state are shared):
      fused  FF.seg_ce_dice_loss + backward (3 launches; 8 B of logits + 8 B of int64 map read per pixel and direction, 8 B written)
      aten   the reference's lines (train_mask_detector.py:127-134 with modules/loss.py:148-186, including dice_coeff's .item()) on the
             NCHW view of the same logits
    ms per form (median), the fused form's bytes / s against the 6.29 TB/s measured-copy figure, and the largest
    difference of the two forms' gradients relative to the largest entry.
(2) one train_step of MaskDetector(3, bilinear=True) at 1 x 1024^2 (median of 5 after 2 warm-up steps), and the share of it that (1)'s
    fused form is.  No speed threshold is asserted; the two forms' gradients must agree within 1e-3 of the largest entry."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from face_mask_inpaint_amd import functional as FF  # noqa: E402
from face_mask_inpaint_amd import train_mask_detector as TM  # noqa: E402
from face_mask_inpaint_amd.modules.mask_detector import MaskDetector  # noqa: E402
from face_mask_inpaint_amd.optim import FusedAdam  # noqa: E402

COPY_TBS = 6.29


def aten_form(logits_nhwc, mask, eps=1e-6):
    """the launches the reference's objective makes, on the NCHW view UNet.forward would hand its trainer: cross_entropy, softmax, one_hot,
    permute, .float(), and per class a dot, two sums and the host read of the empty-set test"""
    masks_pred = FF.to_nchw(logits_nhwc)
    true_masks = (mask > 0).to(dtype=torch.long)
    classes = masks_pred.shape[1]
    probs = F.softmax(masks_pred, dim=1).float()
    onehot = F.one_hot(true_masks, classes).permute(0, 3, 1, 2).float()
    coeffs = []
    for k in range(classes):
        a, b = probs[:, k].reshape(-1), onehot[:, k].reshape(-1)
        inter, total = torch.dot(a, b), a.sum() + b.sum()
        denom = 2 * inter if total.item() == 0 else total  # the host synchronisation of the reference's form
        coeffs.append((2 * inter + eps) / (denom + eps))
    return F.cross_entropy(masks_pred, true_masks) + (1 - sum(coeffs) / classes)


def fused_form(logits_nhwc, mask):
    return FF.seg_ce_dice_loss(logits_nhwc, mask)[0]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    dev = torch.device("cuda:0")
    res = {}
    for n in (1, 8):
        x = (torch.randn(n, 1024, 1024, 2, device=dev) * 2).requires_grad_(True)
        mask = torch.zeros(n, 1024, 1024, dtype=torch.int64, device=dev)
        mask[:, 200:700, 300:900] = 255

        def run(form):
            x.grad = None
            form(x, mask).backward()

        grads = {}
        for name, form in (("fused", fused_form), ("aten", aten_form)):
            for _ in range(3):  # warm-up, outside the timed window
                run(form)
            grads[name] = x.grad.clone()
        ms = {"fused": [], "aten": []}
        for _ in range(15):  # alternate the two forms
            for name, form in (("fused", fused_form), ("aten", aten_form)):
                ms[name].append(event_ms(lambda: run(form)))
        p = n * 1024 * 1024
        nbytes = p * (8 + 8) * 2 + p * 8  # logits + int64 map read in both directions, dlogits written
        tf, ta = statistics.median(ms["fused"]), statistics.median(ms["aten"])
        res[f"N{n}"] = dict(fused_ms=round(tf, 4), aten_ms=round(ta, 4), fused_TBs=round(nbytes / tf / 1e9, 3),
                            share_of_copy_rate=round(nbytes / tf / 1e9 / COPY_TBS, 3),
                            grad_diff_rel=float((grads["fused"] - grads["aten"]).abs().max() / grads["aten"].abs().max()))
        assert res[f"N{n}"]["grad_diff_rel"] <= 1e-3, res  # the two forms compute the same gradient
    torch.manual_seed(0)
    net = MaskDetector(n_channels=3, bilinear=True).to(dev).train()
    opt = FusedAdam(net.parameters(), lr=1e-5)
    img = torch.rand(1, 3, 1024, 1024, device=dev)
    mask = torch.zeros(1, 1024, 1024, dtype=torch.int64, device=dev)
    mask[:, 200:700, 300:900] = 255
    for _ in range(2):
        TM.train_step(net, opt, img, mask)
    step = statistics.median(event_ms(lambda: TM.train_step(net, opt, img, mask)) for _ in range(5))
    res["train_step_N1_ms"] = round(step, 3)
    res["loss_share_of_step"] = round(res["N1"]["fused_ms"] / step, 5)
    line = json.dumps(dict(seg_loss_time=res, copy_TBs=COPY_TBS))
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
