"""Host-side mirror of the reference's two entry points of the pSp model: psp_inference.py (``get_args`` :19-77, ``infer_batch`` :80-103,
``tensor2im`` :106-112, ``evaluate`` :115-119, ``main`` :122-202: dataset -> mask detector -> pSp(ref, src_mask) -> SSIM / MS-SSIM ->
gen_<id>.jpg + metrics.csv) and gradio_serve.py's ``ModelInterface`` (:14-77, one PIL pair in, the unmasked face and the detected mask
out at the source's own size) without the web part.  Encoder, decoder and detector run on the HIP kernels; the image tail
(face_pool, the (x + 1) / 2 operand of the metrics, tensor2im's uint8 picture) is one kernel (functional.image_tail).  There is no
CPU path.

    python -m face_mask_inpaint_amd.psp_inference --data_root DIR --pt_ckpt_path CKPT --mask_detector_path UNET --use_ref

SSIM / MS-SSIM: the reference imports pytorch_msssim (absent offline, **parity unpinned** -- SURVEY.md 8c); ``main`` uses this build's
valid-window kernels of the published definition (modules/evaluations/msssim.py)."""
from __future__ import annotations

import argparse
import csv
import os

import numpy as np
import torch

from . import functional as FF
from .modules.mask_detector import MaskDetector
from .modules.model import scale_img
from .modules.pluralistic_model import base_function
from .modules.psp.psp import pSp


MASK_DETECTOR_DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def get_args(argv=None):
    """the reference's flags with the reference's defaults (psp_inference.py:19-77).  Differences, all about paths: no default points
    outside the working directory (``--data_root`` absent = synthetic batches; ``--pt_ckpt_path`` / ``--mask_detector_path`` absent =
    random initialisation), and the data sub-paths are joined with ``data_root`` where they are used, not here."""
    p = argparse.ArgumentParser()
    p.add_argument("--data_root", type=str, default=None, help="directory with the src / ref / mask sub-directories; synthetic batches when absent")
    p.add_argument("--identity_file_path", type=str, default="CelebA-HQ-identity.txt")
    p.add_argument("--mask_path", type=str, default="binary_map")
    p.add_argument("--src_img_path", type=str, default="images_masked_test")
    p.add_argument("--ref_img_path", type=str, default="images")
    p.add_argument("--mask_detector_path", type=str, default=None)
    p.add_argument("--batch_size", default=8, type=int)
    p.add_argument("--pt_ckpt_path", default=None, type=str, help="Path to pretrained pSp model checkpoint")
    p.add_argument("--save_src_mask", type=int, default=0)
    p.add_argument("--use_ref", action="store_true", help="use reference image")
    p.add_argument("--use_attention", default=0, type=int, help="use attention")
    p.add_argument("--encoder_type", type=str, default="GradualStyleEncoder")
    p.add_argument("--output_size", default=1024, type=int, help="Output size of generator")
    p.add_argument("--train_decoder", default=0, type=int, help="Whether to train the decoder model")
    p.add_argument("--start_from_latent_avg", type=int, default=1, help="Whether to add average latent vector to generate codes from encoder.")
    p.add_argument("--learn_in_w", type=int, default=0, help="Whether to learn in w space instead of w+")
    p.add_argument("--randomize_noise", type=int, default=0, help="whether to randomize noise in stylegan")
    p.add_argument("--stylegan_weights", default=None, type=str, help="Path to StyleGAN model weights")
    # this build's extras
    p.add_argument("--decoder_dtype", type=str, default="fp32", choices=("fp32", "bf16"), help="activation type of the synthesis network")
    p.add_argument("--mask_detector_dtype", type=str, default="fp32", choices=("fp32", "bf16"),
                   help="activation type of the mask detector's UNet body (bf16 needs H and W to be multiples of 16)")
    p.add_argument("--encoder_dtype", type=str, default="fp32", choices=("fp32", "bf16"),
                   help="activation type of the encoder's IR-SE body (bf16: the fused inference form of its 24 blocks)")
    p.add_argument("--style_heads_dtype", type=str, default="fp32", choices=("fp32", "bf16"),
                   help="activation type of the encoder's map2style heads (bf16: the heads of a pyramid level run together, one launch per layer)")
    p.add_argument("--neck_dtype", type=str, default="fp32", choices=("fp32", "bf16"),
                   help="activation type of the encoder's stem and neck (bf16: fused stem, guided attention, blends, laterals and merges on bf16 maps; "
                        "needs --encoder_dtype bf16 and --style_heads_dtype bf16)")
    p.add_argument("--out_dir", type=str, default=None, help="where gen_<id>.jpg / metrics.csv go (default: test_results/<run name>)")
    p.add_argument("--num_batches", type=int, default=2, help="synthetic mode: batches to run")
    return p.parse_args(argv)


def run_name(args):
    """psp_inference.py:163: the directory the checkpoint lies in names the run"""
    return os.path.split(os.path.split(args.pt_ckpt_path)[0])[1] if args.pt_ckpt_path else "random_init"


@torch.no_grad()
def infer_batch(generator, mask_detector, batch_images, device, want=None):
    """psp_inference.py:80-103.  The detector sees (src + 1) / 2.  Returns (pooled image on the device, mask on the CPU or None);
    with ``want`` (a subset of 'pooled', 'unit', 'u8') the first element is the dictionary of those outputs of the fused tail."""
    generator.eval()
    if len(batch_images) == 1:
        src_img = batch_images[0].to(device)
        ref_img = src_mask = None
    else:
        src_img, ref_img = batch_images
        src_img = src_img.to(device)
        ref_img = ref_img.to(device)
        unit_src = (src_img + 1) / 2
        if hasattr(mask_detector, "predict_mask"):
            src_mask = mask_detector.predict_mask(unit_src)                      # argmax as one index kernel, bit exact
        else:
            src_mask = mask_detector(unit_src, mode="train").argmax(1).float()   # [N, H, W]
    out, _ = generator.infer(src_img, ref=ref_img, src_mask=src_mask, want=("pooled",) if want is None else want)
    mask_cpu = src_mask.detach().cpu() if src_mask is not None else None
    return (out["pooled"] if want is None else out), mask_cpu


def tensor2im(var):
    """psp_inference.py:106-112 on a CPU tensor [3, H, W] in [-1, 1], in numpy float32 -- kept for parity of the interface and as the
    checker of the device kernel (functional.image_tail / planes_to_u8 compute exactly this)"""
    from PIL import Image

    var = var.permute(1, 2, 0).numpy()
    var = ((var + 1) / 2)
    var[var < 0] = 0
    var[var > 1] = 1
    var = var * 255
    return Image.fromarray(var.astype("uint8"))


def tensor2im_unit(img):
    """gradio_serve.py:45-51: the same for an image that is already in [0, 1]; returns the uint8 array"""
    img = img.permute(1, 2, 0).numpy().copy()
    img[img < 0] = 0
    img[img > 1] = 1
    img = img * 255
    return img.astype("uint8")


def evaluate(gt_img, gen_img, ssim_func, ms_ssim_func, unit=None):
    """psp_inference.py:115-119; ``unit`` (this build's extra) is (gen_img + 1) / 2 when the fused tail has already produced it"""
    if unit is None:
        unit = (gen_img + 1) / 2
    return float(ssim_func(gt_img, unit)), float(ms_ssim_func(gt_img, unit))


def build(args, device):
    """frozen eval mask detector + pSp(args); without a stored latent_avg the mean of 1e5 mapped latents (psp_inference.py:131-143)"""
    dt = getattr(args, "mask_detector_dtype", "fp32")
    if dt not in MASK_DETECTOR_DTYPES:
        raise FF.FmiError(f"mask_detector_dtype must be one of {sorted(MASK_DETECTOR_DTYPES)}, got {dt!r}")
    mask_detector = MaskDetector(n_channels=3, bilinear=True, compute_dtype=MASK_DETECTOR_DTYPES[dt])
    if args.mask_detector_path:
        mask_detector.load_state_dict(torch.load(args.mask_detector_path, map_location="cpu", weights_only=True))
    base_function._freeze(mask_detector)
    mask_detector = mask_detector.to(device).eval()
    # --encoder_dtype is this harness's name for the encoder's EVAL-mode body (pSp / GradualStyleEncoder: opts.encoder_eval_dtype); their
    # opts.encoder_dtype is the training body, which an inference run never enters
    opts = argparse.Namespace(**vars(args))
    opts.encoder_eval_dtype = getattr(args, "encoder_dtype", "fp32")
    opts.encoder_dtype = "fp32"
    opts.style_heads_eval_dtype = getattr(args, "style_heads_dtype", "fp32")  # likewise: the heads of an EVAL-mode forward
    opts.encoder_neck_eval_dtype = getattr(args, "neck_dtype", "fp32")  # likewise: the stem and the neck of an EVAL-mode forward
    generator = pSp(opts).to(device).eval()
    if "bf16" in (opts.encoder_eval_dtype, opts.style_heads_eval_dtype, opts.encoder_neck_eval_dtype):  # a frozen encoder keeps its folded BatchNorm constants and bf16 weight packs between calls
        base_function._freeze(generator.encoder)
    if generator.latent_avg is None:
        with torch.no_grad():
            generator.latent_avg = generator.decoder.mean_latent(int(1e5))[0].detach()
    return generator, mask_detector


def _metric_funcs():
    from .modules.evaluations.msssim import MS_SSIM, SSIM

    return SSIM(data_range=1, size_average=True, channel=3), MS_SSIM(data_range=1, size_average=True, channel=3)


def main(argv=None):
    from PIL import Image

    args = get_args(argv)
    if not torch.cuda.is_available():
        raise FF.FmiError("psp_inference needs the MI355X (the HIP path has no CPU fallback)")
    device = torch.device("cuda:0")
    ssim_func, ms_ssim_func = _metric_funcs()
    generator, mask_detector = build(args, device)
    if args.data_root:
        from .dataloader import DeviceLoader, ReferenceDataset

        j = lambda p: os.path.join(args.data_root, p)
        ds = ReferenceDataset(j(args.src_img_path), j(args.ref_img_path), j(args.mask_path), j(args.identity_file_path), apply_transform=True,
                              scale=0.25, use_ssim=True, device=device, return_id=True)
        batches = DeviceLoader(ds, range(len(ds)), args.batch_size, shuffle=False, drop_last=False)
    else:
        g = torch.Generator().manual_seed(0)
        r = lambda: torch.rand(args.batch_size, 3, 256, 256, generator=g)
        batches = [{"src_img": r() * 2 - 1, "ref_img": r() * 2 - 1, "raw_gt_img": r(),
                    "id": torch.arange(b * args.batch_size, (b + 1) * args.batch_size).view(-1, 1)} for b in range(args.num_batches)]
    out_dir = args.out_dir or os.path.join("test_results", run_name(args))
    os.makedirs(out_dir, exist_ok=True)
    results = []
    for batch in batches:
        images = (batch["src_img"], batch["ref_img"]) if args.use_ref else (batch["src_img"],)
        out, src_mask = infer_batch(generator, mask_detector, images, device, want=("pooled", "unit", "u8"))
        results.append(list(evaluate(batch["raw_gt_img"].to(device).contiguous(), out["pooled"], ssim_func, ms_ssim_func, unit=out["unit"])))
        pictures = out["u8"].cpu().numpy()  # the one device -> host copy of the generated batch
        masks = FF.mask_to_u8(src_mask.to(device)).cpu().numpy() if src_mask is not None and args.save_src_mask else None
        for i, key in enumerate(batch["id"].view(-1).tolist()):
            Image.fromarray(pictures[i]).save(os.path.join(out_dir, f"gen_{key}.jpg"))
            if masks is not None:
                Image.fromarray(masks[i]).save(os.path.join(out_dir, f"mask_{key}.jpg"))
    mean = np.array(results, dtype=np.float64).mean(0) if results else np.array([float("nan")] * 2)  # over batches, as the reference does
    print({"ssim": float(mean[0]), "ms_ssim": float(mean[1]), "batches": len(results), "out_dir": out_dir})
    with open(os.path.join(out_dir, "metrics.csv"), "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["ssim", "ms_ssim"])
        w.writerow([repr(float(mean[0])), repr(float(mean[1]))])
    return float(mean[0]), float(mean[1])


class ModelInterface:
    """gradio_serve.py:14-77 without gradio: ``infer(src_pil, ref_pil)`` -> (generated image, detected mask), uint8 [H, W, 3] arrays at
    the source image's own size.

        iface = ModelInterface(get_args(["--pt_ckpt_path", CKPT, "--mask_detector_path", UNET]), "cuda:0")
        face, mask = iface.infer(PIL.Image.open("masked.jpg"), PIL.Image.open("same_person.jpg"))
    """

    def __init__(self, args, device="cuda:0"):
        from .preprocess import DevicePreprocessor

        if not torch.cuda.is_available():
            raise FF.FmiError("ModelInterface needs the MI355X (the HIP path has no CPU fallback)")
        self.device = torch.device(device)
        self.generator, self.mask_detector = build(args, self.device)
        self.pre = DevicePreprocessor(self.device)

    def preprocess_img(self, img):
        """PIL image -> (float32 [1, 3, 256, 256] on the device, (H, W) of the original): Pillow-exact BICUBIC to 256 x 256, / 255,
        Normalize(0.5, 0.5) (gradio_serve.py:31-43)"""
        arr = np.asarray(img.convert("RGB") if img.mode != "RGB" else img)
        return self.pre.images([arr], normalise=True, size=(256, 256)), (arr.shape[0], arr.shape[1])

    @torch.no_grad()
    def _run(self, src_img, ref_img, want):
        src_mask = self.mask_detector.predict_mask((src_img + 1) / 2)
        out, _ = self.generator.infer(src_img, ref=ref_img, src_mask=src_mask, want=want)
        return out, src_mask

    def infer_image(self, src_img, ref_img):
        """gradio_serve.py:66-77: (pooled image [1, 3, 256, 256] in [-1, 1], mask [1, 256, 256]); both stay on the device here (the
        reference moves them to the CPU, where its resize then runs)"""
        out, src_mask = self._run(src_img, ref_img, ("pooled",))
        return out["pooled"], src_mask

    @torch.no_grad()
    def infer(self, src_img, ref_img):
        """gradio_serve.py:53-64"""
        src, size = self.preprocess_img(src_img)
        ref, _ = self.preprocess_img(ref_img)
        out, mask = self._run(src, ref, ("unit",))
        gen = scale_img(out["unit"], size)                       # (gen + 1) / 2, then bilinear (align_corners) to the source's size
        mask = scale_img(mask.unsqueeze(1).contiguous(), size)   # one channel resized; the conversion kernel replicates it
        return FF.planes_to_u8(gen, 0.0, 1.0)[0].cpu().numpy(), FF.planes_to_u8(mask, 0.0, 1.0)[0].cpu().numpy()


if __name__ == "__main__":
    main()
