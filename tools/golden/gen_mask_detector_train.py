"""Generator of tests/golden/md_train.pt (+ tests/golden/md_train_parts/*.pt): the reference's mask-detector training objective, its
validation metric and one training step / four Adam steps of its MaskDetector, run on the CPU from the imported reference in fp32 and
in float64.  Run from the repository root:

    python -m tools.golden.gen_mask_detector_train

Parameters are not stored: both sides fill them with oracle/seeded.py::seeded_fill_.  Gradients are stored as digests
(oracle/seeded.py::grad_digest).  Everything stored is a plain tensor / number / string (``weights_only=True`` loads it) and no file
exceeds 1 MiB: the step's logits are files of their own under md_train_parts/.

Contents (suffix 64 = the float64 run; the float64 run of the objective drops the reference's ``.float()`` cast, which would round the
probabilities to fp32 -- ``dice64_cast`` keeps it, for the record)
  config      seeds and shapes
  step        MaskDetector(3, bilinear=True), seeded, .train(), batch 2 at 100 x 84 (odd intermediate sizes: the pad branch of Up),
              rectangular targets (uint8, non-zero = mask): ce / dice / loss, the 18 BatchNorms' running statistics after the forward, the
              reference's fp32-vs-float64 gradient error over whole tensors (median, p90, worst); parts ``step_logits`` / ``step_logits64``
              (NCHW) and ``step_gparams`` / ``step_gparams64`` (digests of the 74 parameter gradients, GRAD_KEEP entries each)
  trajectory  4 x (forward, loss, backward, torch.optim.Adam(lr=1e-5).step()) on that batch: the 4 losses
  ops         cases of (logits NHWC, target): ce, dice (= dice_loss), dlogits of ce + dice (NCHW; a digest for the 1 x 1024^2 case,
              whose logits are a seed) and the evaluate()-style Dice score; ``helpers``: dice_coeff / multiclass_dice_coeff / dice_loss
              on softmax probabilities and one-hot targets for reduce_batch_first False / True
  args        names and defaults of the reference's get_args() with an empty command line;  keys: MaskDetector's state_dict keys
"""
from __future__ import annotations

import os
import sys
import types

import torch
import torch.nn.functional as F

from oracle import gen_golden as G
from oracle.seeded import grad_digest, seeded_fill_, seeded_tensor

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests", "golden")
PARTS = "md_train_parts"
MD_SEED, X_SEED = 91, 92
STEP_SHAPE = (2, 3, 100, 84)
STEP_RECTS = ((20, 70, 10, 60, 255), (35, 90, 30, 80, 1))  # y0, y1, x0, x1, the map's non-zero value
LR, STEPS = 1e-5, 4
# entries kept per gradient tensor.  The worst entry of an fp32 gradient sits where a ReLU mask element differs from float64's (one such
# element in the reference's own fp32 run: 576 entries of one 64 x 64 x 3 x 3 weight gradient); 512 samples per tensor saw 1.26e-3 where
# the whole tensors have 3.39e-3, so the digests are as dense as the 1 MiB file limit allows
GRAD_KEEP = 8192
BIG_SEED, BIG_RECT = 97, (200, 700, 300, 900)


def _stub_modules():
    """train_mask_detector.py / dataloader.py import packages that are absent here and irrelevant to the functions used"""
    def mod(name, **attrs):
        m = sys.modules.get(name) or types.ModuleType(name)
        for k, v in attrs.items():
            if not hasattr(m, k):
                setattr(m, k, v)
        sys.modules[name] = m
        return m

    blank = lambda n: type(n, (), {"__init__": lambda self, *a, **k: None})
    mod("pytorch_msssim", SSIM=blank("SSIM"), MS_SSIM=blank("MS_SSIM"))
    tvt = mod("torchvision.transforms", Normalize=blank("Normalize"))
    mod("torchvision").transforms = tvt
    mod("wandb")
    mod("tqdm", tqdm=lambda it=None, *a, **k: it)


def step_targets():
    t = torch.zeros(STEP_SHAPE[0], STEP_SHAPE[2], STEP_SHAPE[3], dtype=torch.uint8)
    for i, (y0, y1, x0, x1, v) in enumerate(STEP_RECTS):
        t[i, y0:y1, x0:x1] = v
    return t


def op_cases():
    """name -> (logits NHWC fp32, target uint8 [N, H, W]); the big case is built by big_case() on both sides"""
    g = torch.Generator().manual_seed(95)
    cases = {}

    def rect(n, h, w):
        t = torch.zeros(n, h, w, dtype=torch.uint8)
        for i in range(n):
            t[i, h // 4 + i:h // 4 + i + h // 2, w // 5:w // 5 + w // 2 + i] = 1 if i % 2 else 200
        return t

    # C = 2, 2 x 13 x 9: pixel count 234 is not a multiple of the vector width and 117 pixels per sample is odd; exact ties
    x = torch.randn(2, 13, 9, 2, generator=g) * 2
    x[0, 3, :, 1] = x[0, 3, :, 0]
    x[1, 5:7, 2:6, 0] = x[1, 5:7, 2:6, 1]
    cases["c2_odd"] = (x, rect(2, 13, 9))
    # C = 2, 3 x 16 x 20: sample 1 has an empty target AND an empty prediction, sample 2 an empty target but a non-empty prediction
    x = torch.randn(3, 16, 20, 2, generator=g) * 3
    x[0, 2, 4:12, 1] = x[0, 2, 4:12, 0]
    x[1, ..., 0] = x[1, ..., 1].abs() + 0.5 + x[1, ..., 1]
    x[1, 4, 5, 1] = x[1, 4, 5, 0]  # a tie: the first class (background) wins, the prediction stays empty
    t = rect(3, 16, 20)
    t[1] = 0
    t[2] = 0
    cases["c2_empty"] = (x, t)
    # C = 3 (targets stay in {0, 1}: the trainer binarises the map), ties between the two foreground classes and with the background
    x = torch.randn(2, 12, 10, 3, generator=g) * 2
    x[0, 1, :, 2] = x[0, 1, :, 1] = x[0, 1, :, 0].abs() + x[0, 1, :, 0] + 1.0
    x[1, 6, 2:8, 2] = x[1, 6, 2:8, 0] = x[1, 6, 2:8, 1].abs() + x[1, 6, 2:8, 1] + 0.25
    cases["c3"] = (x, rect(2, 12, 10))
    x = torch.randn(2, 7, 9, 3, generator=g) * 4
    cases["c3_odd"] = (x, rect(2, 7, 9))
    return cases


def big_case():
    x = seeded_tensor((1, 1024, 1024, 2), BIG_SEED, 2.0)
    t = torch.zeros(1, 1024, 1024, dtype=torch.uint8)
    t[0, BIG_RECT[0]:BIG_RECT[1], BIG_RECT[2]:BIG_RECT[3]] = 1
    return x, t


def main():
    torch.set_num_threads(8)
    G.import_reference()
    _stub_modules()
    import train_mask_detector as T
    from modules import loss as RL
    from modules.mask_detector import MaskDetector

    os.makedirs(os.path.join(OUT, PARTS), exist_ok=True)
    parts = {}
    fx = dict(config=dict(md_seed=MD_SEED, x_seed=X_SEED, step_shape=STEP_SHAPE, step_rects=STEP_RECTS, lr=LR, steps=STEPS, big_seed=BIG_SEED,
                          big_scale=2.0, big_rect=BIG_RECT))

    def objective(masks_pred, true_masks, n_classes, cast=True):
        """train_mask_detector.py:131-134, literally; cast=False drops the .float() of the probabilities (the float64 run)"""
        probs = F.softmax(masks_pred, dim=1)
        onehot = F.one_hot(true_masks, n_classes).permute(0, 3, 1, 2)
        ce = torch.nn.CrossEntropyLoss()(masks_pred, true_masks)
        dice = RL.dice_loss(probs.float() if cast else probs, onehot.float() if cast else onehot.to(probs.dtype), multiclass=True)
        return ce, dice

    def score(masks_pred, true_masks, n_classes):
        """train_mask_detector.py:34-35,47-49 for one batch"""
        dt = masks_pred.dtype
        mask_true = F.one_hot(true_masks, n_classes).permute(0, 3, 1, 2).to(dt)
        mask_pred = F.one_hot(masks_pred.argmax(dim=1), n_classes).permute(0, 3, 1, 2).to(dt)
        return RL.multiclass_dice_coeff(mask_pred[:, 1:, ...], mask_true[:, 1:, ...], reduce_batch_first=False)

    # ---- one training step and the 4-step trajectory
    x = torch.rand(STEP_SHAPE, generator=torch.Generator().manual_seed(X_SEED))
    tmap = step_targets()
    true_masks = (tmap > 0).to(torch.long)  # train_mask_detector.py:127
    step, traj, full = {"target": tmap}, {}, {}
    for dt, sfx in ((torch.float32, ""), (torch.float64, "64")):
        net = MaskDetector(n_channels=3, bilinear=True)
        seeded_fill_(net, MD_SEED)
        net = net.to(dt).train()
        opt = torch.optim.Adam(net.parameters(), lr=LR)
        losses = []
        for i in range(STEPS):
            logits = net(x.to(dt))
            ce, dice = objective(logits, true_masks, net.n_classes, cast=not sfx)
            loss = ce + dice
            opt.zero_grad(set_to_none=True)
            loss.backward()
            if i == 0:
                parts["step_logits" + sfx] = logits.detach().float().clone()
                step["ce" + sfx], step["dice" + sfx], step["loss" + sfx] = (torch.tensor(float(v.detach()), dtype=torch.float64) for v in (ce, dice, loss))
                parts["step_gparams" + sfx] = {n: grad_digest(p.grad.float(), GRAD_KEEP) for n, p in net.named_parameters()}
                full[sfx] = {n: p.grad.detach().double().clone() for n, p in net.named_parameters()}
                step["no_grad" + sfx] = sorted(n for n, p in net.named_parameters() if p.grad is None)
                step["bn" + sfx] = {k: v.detach().clone().to(torch.float32 if v.is_floating_point() else v.dtype)
                                    for k, v in net.state_dict().items() if k.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked")}
            opt.step()
            losses.append(float(loss.detach()))
        traj["losses" + sfx] = torch.tensor(losses, dtype=torch.float64)
    fx["step"], fx["trajectory"] = step, traj
    g32, g64 = parts["step_gparams"], parts["step_gparams64"]
    big = [n for n in g64 if float(g64[n]["max"]) > 1e-9]
    whole = sorted(float((full[""][n] - full["64"][n]).abs().max() / full["64"][n].abs().max()) for n in big)
    step["ref_error_whole_tensors"] = torch.tensor([whole[len(whole) // 2], whole[int(.9 * len(whole))], whole[-1]], dtype=torch.float64)
    print("fp32 vs float64 gradients over WHOLE tensors: median %.2e p90 %.2e worst %.2e (the digests below sample %d entries per tensor)" % (
        whole[len(whole) // 2], whole[int(.9 * len(whole))], whole[-1], GRAD_KEEP))
    rel = sorted(float((g32[n]["sample"] - g64[n]["sample"]).abs().max()) / float(g64[n]["max"]) for n in g64 if float(g64[n]["max"]) > 1e-9)
    print("step: %d parameters, %d with a gradient above 1e-9; fp32 vs float64 gradients median %.2e p90 %.2e worst %.2e; logits %.2e; loss %.2e; "
          "trajectory %.2e" % (len(g64), len(rel), rel[len(rel) // 2], rel[int(.9 * len(rel))], rel[-1],
                                float((parts["step_logits"] - parts["step_logits64"]).abs().max()), abs(float(step["loss"] - step["loss64"])),
                                float((traj["losses"] - traj["losses64"]).abs().max())))
    print("zero-gradient biases: largest float64 |g| %.2e" % max(float(d["max"]) for n, d in g64.items() if float(d["max"]) <= 1e-9))

    # ---- the objective, its gradient and the metric on given logits
    ops = {}
    cases = op_cases()
    cases["c2_big"] = big_case()
    for name, (x_nhwc, t8) in cases.items():
        c = dict() if name == "c2_big" else dict(logits=x_nhwc.clone(), target=t8)  # the big case is rebuilt from config
        n_classes = x_nhwc.shape[-1]
        t = (t8 > 0).to(torch.long)
        for dt, sfx in ((torch.float32, ""), (torch.float64, "64")):
            lg = x_nhwc.permute(0, 3, 1, 2).contiguous().to(dt).requires_grad_(True)
            ce, dice = objective(lg, t, n_classes, cast=not sfx)
            (ce + dice).backward()
            c["ce" + sfx], c["dice" + sfx] = torch.tensor(float(ce.detach()), dtype=torch.float64), torch.tensor(float(dice.detach()), dtype=torch.float64)
            c["dlogits" + sfx] = grad_digest(lg.grad.float(), 4096) if name == "c2_big" else lg.grad.clone()
            with torch.no_grad():
                c["score" + sfx] = torch.tensor(float(score(lg, t, n_classes)), dtype=torch.float64)
                if sfx:
                    c["dice64_cast"] = torch.tensor(float(objective(lg, t, n_classes, cast=True)[1]), dtype=torch.float64)
                if name in ("c2_empty", "c3"):
                    probs = F.softmax(lg, dim=1)
                    onehot = F.one_hot(t, n_classes).permute(0, 3, 1, 2).to(dt)
                    h = {}
                    for rbf in (False, True):
                        h[f"dice_coeff_{int(rbf)}"] = RL.dice_coeff(probs[:, 1], onehot[:, 1], reduce_batch_first=rbf)
                        h[f"multiclass_{int(rbf)}"] = RL.multiclass_dice_coeff(probs, onehot, reduce_batch_first=rbf)
                    h["dice_coeff_2d"] = RL.dice_coeff(probs[0, 1], onehot[0, 1])
                    h["dice_loss"] = RL.dice_loss(probs[:, 1], onehot[:, 1], multiclass=False)
                    h["dice_loss_multiclass"] = RL.dice_loss(probs, onehot, multiclass=True)
                    c["helpers" + sfx] = {k: torch.tensor(float(v), dtype=torch.float64) for k, v in h.items()}
        ops[name] = c
        print("%-9s ce %.9f (fp32 %+.1e)  dice %.9f (fp32 %+.1e, cast %+.1e)  score %.9f (fp32 %+.1e)" % (
            name, float(c["ce64"]), float(c["ce"] - c["ce64"]), float(c["dice64"]), float(c["dice"] - c["dice64"]),
            float(c["dice64_cast"] - c["dice64"]), float(c["score64"]), float(c["score"] - c["score64"])))
    fx["ops"] = ops

    # ---- the reference's command line and the checkpoint's key list
    argv, sys.argv = sys.argv, ["train_mask_detector.py"]
    try:
        a = T.get_args()
    finally:
        sys.argv = argv
    fx["args"] = [[k, v] for k, v in sorted(vars(a).items())]
    fx["keys"] = list(MaskDetector(n_channels=3, bilinear=True).state_dict().keys())
    fx["parts"] = sorted(parts)
    total = 0
    for name, tens in parts.items():
        p = os.path.join(OUT, PARTS, name + ".pt")
        torch.save(tens.contiguous() if torch.is_tensor(tens) else tens, p)
        total += os.path.getsize(p)
        assert os.path.getsize(p) <= (1 << 20), name
    p = os.path.join(OUT, "md_train.pt")
    torch.save(fx, p)
    assert os.path.getsize(p) <= (1 << 20), os.path.getsize(p)
    print("md_train.pt %.2f MB + %d parts %.2f MB" % (os.path.getsize(p) / 1e6, len(parts), total / 1e6))


if __name__ == "__main__":
    main()
