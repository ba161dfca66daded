"""Generator of tests/golden/psp_train.pt: the reference's pSp trainer command line, the key list of its checkpoints and the pixel head
of its pSpLoss.__call__ (modules/psp/criteria/__init__.py:58-65,80-87), run on the CPU from the imported reference in fp32 and in
float64.  Run from the repository root:

    python -m tools.golden.gen_psp_train

Everything stored is a plain tensor / number / string (``weights_only=True`` loads it); the file stays far below 1 MiB.

Contents
  args    names and values of the reference's train_psp.get_args() with an empty command line, after its post-processing (``eval_options``,
          a set there, is stored as a sorted list)
  keys    state_dict keys of the reference's pSp at output_size 256 with attention (``config.keys_opts``), weight loading stubbed out
          as in oracle/gen_golden.py:psp_whole_fixture -- the checkpoint G_checkpoint_epoch{n}.pth holds exactly these
  head    cases (a) .. (e) through the reference's own pSpLoss.__call__ with l2_lambda = l2_lambda_ref = 1 and every other lambda 0 (no
          network is constructed): ``loss_l2``, ``loss_l2_ref``, ``loss`` and d loss / d y_hat, from the fp32 run and (suffix 64) the
          float64 run on the same fp32 inputs.  Inputs are uniform in [-1, 1] from the stored seeds (``head_inputs``); every mask value
          is 0, 1 or a power of two, so each product y_hat * m is exact in fp32 and the float64 run is the exact value of what a kernel
          with one fp32 multiply per product computes.  Masks are stored; images are regenerated from the seeds.
"""
from __future__ import annotations

import os
import sys
import types

import torch

from oracle import gen_golden as G

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests", "golden")
KEYS_OPTS = dict(output_size=256, encoder_type="GradualStyleEncoder", use_attention=True, train_decoder=True, start_from_latent_avg=True,
                 learn_in_w=False, pt_ckpt_path=None, stylegan_weights=None)
# name -> (shape, seed, with ref and mask)
HEAD_CASES = {"a": ((2, 3, 5, 7), 101, True), "b": ((2, 3, 6, 6), 102, True), "c": ((3, 3, 16, 16), 103, True), "d": ((2, 3, 64, 64), 104, True),
              "e": ((2, 3, 6, 6), 102, False)}


def _stub_modules():
    """train_psp.py / dataloader.py import packages that are absent here and irrelevant to the functions used"""
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
    try:
        import modules.evaluations.fid  # noqa: F401
    except Exception:  # its scipy / inception imports are absent: the trainer's functions used here never call it
        sys.modules.pop("modules.evaluations.fid", None)
        mod("modules.evaluations.fid", calculate_fid=None)


def head_inputs(name):
    """(y_hat, y, ref, mask) fp32 of a case; ref / mask None for case e.  The tests rebuild the images from the shapes and seeds stored
    under ``head_inputs`` (tests/test_host_psp_train.py:head_inputs) and take the masks from the fixture."""
    shape, seed, full = HEAD_CASES[name]
    g = torch.Generator().manual_seed(seed)
    y_hat, y, ref = (torch.rand(shape, generator=g) * 2 - 1 for _ in range(3))
    if not full:
        return y_hat, y, None, None
    n, _, h, w = shape
    m = torch.zeros(n, h, w)
    if name == "c":  # values {0, 0.25, 0.5, 1}; sample 1 all zero, sample 2 all one
        m[0] = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (h, w), generator=g)]
        m[2] = 1.0
    else:  # binary rectangles, different per sample, touching a border in sample 1
        for i in range(n):
            m[i, h // 4 + i:h // 4 + i + h // 2, (w // 5) * (1 - i):w // 5 + w // 2 + i] = 1.0
    return y_hat, y, ref, m


def main():
    torch.set_num_threads(8)
    G.import_reference()
    G._import_stylegan2()
    _stub_modules()
    import train_psp as T
    from modules.psp import psp as P
    from modules.psp.criteria import pSpLoss

    fx = dict(config=dict(keys_opts=[[k, v] for k, v in sorted(KEYS_OPTS.items())]))

    # ---- the reference's command line
    argv, sys.argv = sys.argv, ["train_psp.py"]
    try:
        a = T.get_args()
    finally:
        sys.argv = argv
    fx["args"] = [[k, sorted(v) if isinstance(v, (set, frozenset)) else v] for k, v in sorted(vars(a).items())]

    # ---- the checkpoint's key list
    P.pSp.load_weights = lambda self: setattr(self, "latent_avg", None)  # the checkpoint files are absent (as in psp_whole_fixture)
    fx["keys"] = list(P.pSp(types.SimpleNamespace(**KEYS_OPTS)).state_dict().keys())

    # ---- the pixel head through the reference's pSpLoss.__call__
    lam = types.SimpleNamespace(id_lambda=0, lpips_lambda=0, l2_lambda=1.0, style_lambda=0, lpips_lambda_ref=0, l2_lambda_ref=1.0, cx_lambda=0,
                                w_norm_lambda=0, start_from_latent_avg=False)
    crit = pSpLoss(lam)
    fx["head_inputs"] = {k: dict(shape=list(v[0]), seed=v[1], full=v[2]) for k, v in HEAD_CASES.items()}
    head = {}
    for name in HEAD_CASES:
        y_hat, y, ref, m = head_inputs(name)
        c = dict() if m is None else dict(mask=m.clone())
        for dt, sfx in ((torch.float32, ""), (torch.float64, "64")):
            yh = y_hat.to(dt).clone().requires_grad_(True)
            loss, d, _ = crit(None, y.to(dt), yh, None, latent_avg=None, ref=None if ref is None else ref.to(dt), mask=None if m is None else m.to(dt))
            loss.backward()
            for k in ("loss_l2", "loss_l2_ref", "loss"):
                if k in d:
                    c[k + sfx] = torch.tensor(d[k], dtype=torch.float64)
            c["loss_tensor" + sfx] = loss.detach().double().clone()
            c["grad" + sfx] = yh.grad.clone()
        head[name] = c
        print("%s %-14s l2 %.12f (fp32 %+.1e)  l2_ref %s  grad fp32 vs 64 %.1e" % (
            name, tuple(y_hat.shape), float(c["loss_l264"]), float(c["loss_l2"] - c["loss_l264"]),
            "%.12f (fp32 %+.1e)" % (float(c["loss_l2_ref64"]), float(c["loss_l2_ref"] - c["loss_l2_ref64"])) if "loss_l2_ref64" in c else "-",
            float((c["grad"].double() - c["grad64"]).abs().max())))
    fx["head"] = head
    p = os.path.join(OUT, "psp_train.pt")
    torch.save(fx, p)
    assert os.path.getsize(p) <= (1 << 20), os.path.getsize(p)
    torch.load(p, weights_only=True)
    print("psp_train.pt %.3f MB, %d keys, %d args" % (os.path.getsize(p) / 1e6, len(fx["keys"]), len(fx["args"])))


if __name__ == "__main__":
    main()
