"""Generator of tests/golden/ref_train.pt: the reference's PICNet trainer command line, the key lists of its two checkpoints and the image
head of its GANOptimizer (modules/loss.py:48-51,84-95,115), run on the CPU from the imported reference in fp32 and in float64.  Run from
the repository root:

    python -m tools.golden.gen_reference_fill_train

Everything stored is a plain tensor / number / string (``weights_only=True`` loads it); the file stays below 1 MiB.

Contents
  args            names and values of the reference's train_reference_fill.get_args() with an empty command line, after its post-processing
                  (``eval_options``, a set there, is stored as a sorted list)
  keys_G, keys_D  state_dict keys of the reference's ReferenceFill (with its frozen MaskDetector) / define_d built as its main() builds
                  them from those arguments -- G_checkpoint_epoch{n}.pth / D_checkpoint_epoch{n}.pth hold exactly these
  mean, std       the buffers of the reference's VGGLoss
  head_inputs     per case: shape (N, H, W), vgg_size, the seed of the images (gen, gt, src, ref uniform in [0, 1], drawn in that order),
                  the seed of the upstream gradient Gx ([3N, OH, OW, 3] standard normal) and g_l1
  head            cases (a) .. (d) with the reference's own scale_img and the mask expressions of loss.py:87-95, resized when W > vgg_size
                  (loss.py:48): ``x_in`` / ``y_in`` ([3N, OH, OW, 3]: the three operands of each side, channels last), ``l1``
                  (nn.L1Loss, loss.py:115) and ``grad`` = d (g_l1 l1 + <Gx, x_in>) / d gen, from the fp32 run and (suffix 64) the
                  float64 run on the same fp32 inputs; ``mask`` is stored.
                  case (e): what the reference's VGGLoss.forward hands its first block for the three losses through
                  GANOptimizer.perceptual_loss / style_loss / contextual_loss, captured with a forward-pre-hook on a stand-in block (the
                  VGG itself is not run), subsampled at ``rows`` x ``cols`` (the borders plus every 7th), and ``l1``; mask as uint8.
"""
from __future__ import annotations

import os
import sys

import torch

from oracle import gen_golden as G
from tools.golden.gen_psp_train import _stub_modules

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests", "golden")
# name -> ((N, H, W), vgg_size, image seed, Gx seed)
HEAD_CASES = {"a": ((2, 5, 7), 4, 201, 301), "b": ((2, 4, 9), 6, 202, 302), "c": ((1, 6, 8), 8, 203, 303), "d": ((2, 8, 12), 8, 204, 304),
              "e": ((1, 230, 226), 224, 205, 305)}
G_L1 = 0.7


def out_size(h, w, size):
    return (size, size) if w > size else (h, w)


def head_inputs(name):
    """(gen, gt, src, ref, mask) fp32 of a case.  The tests rebuild the images from the shapes and seeds stored under ``head_inputs``
    and take the masks from the fixture."""
    (n, h, w), _, seed, _ = HEAD_CASES[name]
    g = torch.Generator().manual_seed(seed)
    gen, gt, src, ref = (torch.rand((n, 3, h, w), generator=g) for _ in range(4))
    m = torch.zeros(n, h, w)
    if name == "d":  # values {0, 0.25, 0.5, 1} in sample 0; sample 1 all one
        m[0] = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (h, w), generator=g)]
        m[1] = 1.0
    elif name == "e":  # binary: a rectangle plus scattered pixels
        m[0, 60:170, 40:190] = 1.0
        m[0] = torch.maximum(m[0], (torch.rand((h, w), generator=g) < 0.05).float())
    else:  # binary, random; the second sample of (a) all zero
        m[0] = (torch.rand((h, w), generator=g) < 0.5).float()
        if n > 1 and name == "b":
            m[1] = (torch.rand((h, w), generator=g) < 0.5).float()
    return gen, gt, src, ref, m


def upstream(name):
    (n, h, w), size, _, gseed = HEAD_CASES[name]
    oh, ow = out_size(h, w, size)
    return torch.randn((3 * n, oh, ow, 3), generator=torch.Generator().manual_seed(gseed))


def main():
    torch.set_num_threads(8)
    ref_model, ref_loss, ref_network = G.import_reference()
    _stub_modules()
    import train_reference_fill as T
    from modules.mask_detector import MaskDetector

    fx = {}

    # ---- the reference's command line
    argv, sys.argv = sys.argv, ["train_reference_fill.py"]
    try:
        a = T.get_args()
    finally:
        sys.argv = argv
    fx["args"] = [[k, sorted(v) if isinstance(v, (set, frozenset)) else v] for k, v in sorted(vars(a).items())]

    # ---- the checkpoints' key lists (main() :149-163)
    enc, dec, disc = T.process_params(a)
    gen_net = ref_model.ReferenceFill(MaskDetector(n_channels=3, bilinear=True), enc, dec, use_att=a.use_att)
    fx["keys_G"] = list(gen_net.state_dict().keys())
    fx["keys_D"] = list(ref_network.define_d(**disc).state_dict().keys())

    # ---- the image head
    gan = ref_loss.GANOptimizer(None, None)
    vgg = gan.vgg_loss
    fx["mean"], fx["std"] = vgg.mean.view(3).clone(), vgg.std.view(3).clone()
    fx["head_inputs"] = {k: dict(shape=list(v[0]), vgg_size=v[1], seed=v[2], gx_seed=v[3], g_l1=G_L1) for k, v in HEAD_CASES.items()}
    head = {}
    for name in "abcd":
        gen, gt, src, ref, m = head_inputs(name)
        size = HEAD_CASES[name][1]
        gx = upstream(name)
        c = dict(mask=m.clone())
        for dt, sfx in ((torch.float32, ""), (torch.float64, "64")):
            mean, std = vgg.mean.to(dt), vgg.std.to(dt)

            def inp(t):
                if t.shape[-1] > size:  # loss.py:48 at this case's size
                    t = ref_model.scale_img(t, [size, size])
                return (t - mean) / std  # loss.py:50-51

            gd = gen.to(dt).clone().requires_grad_(True)
            md = m.to(dt)
            inv, fwd = (1 - md).unsqueeze(1), md.unsqueeze(1)  # loss.py:88,92
            x = torch.cat([inp(gd), inp(gd * inv), inp(gd * fwd)]).permute(0, 2, 3, 1)
            y = torch.cat([inp(gt.to(dt)), inp(src.to(dt)), inp(ref.to(dt) * fwd)]).permute(0, 2, 3, 1)
            l1 = gan.l1_loss(gd, gt.to(dt))  # loss.py:115
            (G_L1 * l1 + (gx.to(dt) * x).sum()).backward()
            c["x_in" + sfx], c["y_in" + sfx] = x.detach().contiguous().clone(), y.detach().contiguous().clone()
            c["l1" + sfx] = l1.detach().double().clone()
            c["grad" + sfx] = gd.grad.clone()
        head[name] = c
        print("%s x_in fp32 vs 64 %.2e  y_in %.2e  l1 %.12f (fp32 %+.1e)  grad %.2e" % (
            name, float((c["x_in"].double() - c["x_in64"]).abs().max()), float((c["y_in"].double() - c["y_in64"]).abs().max()),
            float(c["l164"]), float(c["l1"] - c["l164"]), float((c["grad"].double() - c["grad64"]).abs().max())))

    # ---- case (e): the operands the reference's VGGLoss.forward hands its first block, through GANOptimizer's three loss methods
    class Tiny(torch.nn.Module):  # stands in for every VGG block: the losses behind it run on a 2 x 2 corner
        def forward(self, x):
            return x[..., :2, :2].contiguous()

    vgg.blocks = torch.nn.ModuleList([Tiny() for _ in range(4)])
    seen = []
    vgg.blocks[0].register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
    gen, gt, src, ref, m = head_inputs("e")
    (n, h, w), size, _, _ = HEAD_CASES["e"]
    assert w > size and out_size(h, w, size) == (224, 224)
    rows = sorted(set(range(0, 224, 7)) | {223})
    cols = sorted(set(range(0, 224, 7)) | {223})
    c = dict(mask=m.to(torch.uint8), rows=torch.tensor(rows), cols=torch.tensor(cols))
    for dt, sfx in ((torch.float32, ""), (torch.float64, "64")):
        gan.to(dt)
        del seen[:]
        gd, md = gen.to(dt), m.to(dt)
        gan.perceptual_loss(gt.to(dt), gd)
        gan.style_loss(gd, src.to(dt), md)
        gan.contextual_loss(gd, ref.to(dt), md)
        assert len(seen) == 6 and all(t.shape == (n, 3, 224, 224) and t.dtype == dt for t in seen)
        sub = lambda ts: torch.cat(ts).permute(0, 2, 3, 1)[:, rows][:, :, cols].contiguous().clone()
        c["x_in" + sfx], c["y_in" + sfx] = sub(seen[0::2]), sub(seen[1::2])  # (input, target) per loss
        c["l1" + sfx] = gan.l1_loss(gd, gt.to(dt)).detach().double().clone()
    head["e"] = c
    print("e x_in fp32 vs 64 %.2e  y_in %.2e  l1 %.12f (fp32 %+.1e)" % (
        float((c["x_in"].double() - c["x_in64"]).abs().max()), float((c["y_in"].double() - c["y_in64"]).abs().max()), float(c["l164"]),
        float(c["l1"] - c["l164"])))
    fx["head"] = head
    p = os.path.join(OUT, "ref_train.pt")
    torch.save(fx, p)
    assert os.path.getsize(p) <= (1 << 20), os.path.getsize(p)
    torch.load(p, weights_only=True)
    print("ref_train.pt %.3f MB, %d + %d keys, %d args" % (os.path.getsize(p) / 1e6, len(fx["keys_G"]), len(fx["keys_D"]), len(fx["args"])))


if __name__ == "__main__":
    main()
