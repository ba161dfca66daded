"""Trainer of the pSp generator -- the counterpart of the reference's train_psp.py (the entry point scripts/train_psp.sh runs), whose
checkpoints psp_inference.py loads through ``--pt_ckpt_path``.

Same command line (``get_args`` :24-116, with the path joins onto ``--data_root`` and ``train_decoder`` -> bool), same step
(``train_step`` :308-335: forward, pSpLoss, the non-finite skip, zero_grad / backward / step), same validation (``evaluate`` :162-242)
on the reference's cadence (``n_train // (10 * batch_size)``, tested after EVERY batch, a skipped one included, :347-351),
``ReduceLROnPlateau('max', patience=2, factor=0.8)`` stepped with the validation LOSS (:294-297,382 -- the reference's literal choice,
kept) and one ``G_checkpoint_epoch{n}.pth`` state_dict per epoch (:388-391).  What differs:

  * the pixel side of the loss is FF.psp_pixel_head (``pSpLoss.fused_head``): one pass forward, one backward;
  * Adam is optim.FusedAdam; batches arrive as device tensors from dataloader.get_reference_dataloader / to_device_batch;
  * two options of this build, ``--decoder_dtype`` / ``--encoder_dtype`` (default fp32), are passed through to pSp;
  * logging goes through ``logging`` and an optional ``callback(event: dict)``: no wandb, no tqdm, no histograms or images;
  * the one host read of a step is ``torch.isfinite(loss)`` (the loop's control flow depends on it); loss values and validation metrics
    stay device scalars until the end of an evaluation round or of the epoch;
  * an ``--optimizer`` other than adam / ranger is refused (the reference would fail on an unbound name).

Out of scope: replaying the step as a HIP graph (a captured FusedAdam bakes ``lr`` into its launches, optim.py, which
ReduceLROnPlateau would silently defeat -- that needs a device-side ``lr`` first), multi-GPU ranks, wandb, and FID (``'fid'`` in
``--eval_options`` is refused: its InceptionV3 is a download).
"""
from __future__ import annotations

import argparse
import logging
import os
from pathlib import Path

import torch

from ._lib import FmiError
from .dataloader import get_reference_dataloader, to_device_batch
from .modules.mask_detector import MaskDetector
from .modules.pluralistic_model import base_function
from .modules.psp.criteria import pSpLoss
from .modules.psp.psp import pSp
from .modules.psp.ranger import Ranger
from .optim import FusedAdam


def get_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--epochs', type=int, default=5, help='Number of epochs')
    parser.add_argument('--batch_size', dest='batch_size', type=int, default=8)
    parser.add_argument('--learning_rate', type=float, default=1e-5)
    parser.add_argument('--eval_options', nargs="+", default={'ssim'})
    parser.add_argument('--debug', type=int, default=0, help='debug with turning off not implemented parts')
    parser.add_argument('--img_scale', type=float, default=1.)
    parser.add_argument('--optimizer', type=str, default='adam')
    parser.add_argument('--use_ref', action='store_true', help='use reference image')
    parser.add_argument('--use_attention', action='store_true', help='use attention')

    # path args
    parser.add_argument('--run_name', type=str, default='', help='exp name')
    parser.add_argument('--checkpoint_path', type=str, default='saved_model')
    parser.add_argument('--mask_detector_path', type=str, default='')
    parser.add_argument('--data_root', type=str, default='/data/mohaa/project1/CelebA')
    parser.add_argument('--src_img_path', type=str, default='img_align_celeba_masked1')
    parser.add_argument('--ref_img_path', type=str, default='img_align_celeba')
    parser.add_argument('--mask_path', type=str, default='binary_map')
    parser.add_argument('--identity_file_path', type=str, default='identity_CelebA.txt')

    # pSp args
    parser.add_argument('--encoder_type', type=str, default='GradualStyleEncoder')
    parser.add_argument('--output_size', default=1024, type=int, help='Output size of generator')
    parser.add_argument('--train_decoder', default=0, type=int, help='Whether to train the decoder model')
    parser.add_argument('--start_from_latent_avg', action='store_true',
                        help='Whether to add average latent vector to generate codes from encoder.')
    parser.add_argument('--learn_in_w', action='store_true', help='Whether to learn in w space instead of w+')
    parser.add_argument('--randomize_noise', action='store_true', help='whether to randomize noise in stylegan')

    # loss weights
    parser.add_argument('--lpips_lambda', default=0.8, type=float, help='LPIPS loss multiplier factor')
    parser.add_argument('--id_lambda', default=0, type=float, help='ID loss multiplier factor')
    parser.add_argument('--l2_lambda', default=1.0, type=float, help='L2 loss multiplier factor')
    parser.add_argument('--w_norm_lambda', default=0, type=float, help='W-norm loss multiplier factor')
    parser.add_argument('--lpips_lambda_ref', default=0, type=float, help='LPIPS loss multiplier factor for inner image region')
    parser.add_argument('--l2_lambda_ref', default=0, type=float, help='L2 loss multiplier factor for inner image region')
    parser.add_argument('--style_lambda', default=250, type=float)
    parser.add_argument('--cx_lambda', default=1, type=float)

    # pretrained weight paths
    parser.add_argument('--stylegan_weights', default=None, type=str, help='Path to StyleGAN model weights')
    parser.add_argument('--pt_ckpt_path', default=None, type=str, help='Path to pretrained pSp model checkpoint')

    # this build's options, passed through to pSp
    parser.add_argument('--decoder_dtype', type=str, default='fp32', choices=('fp32', 'bf16'), help='activation type of the synthesis network')
    parser.add_argument('--encoder_dtype', type=str, default='fp32', choices=('fp32', 'bf16'), help="activation type of the encoder's IR-SE body")
    args = parser.parse_args(argv)

    # process data path args here
    args.src_img_path = os.path.join(args.data_root, args.src_img_path)
    args.ref_img_path = os.path.join(args.data_root, args.ref_img_path)
    args.mask_path = os.path.join(args.data_root, args.mask_path)
    args.identity_file_path = os.path.join(args.data_root, args.identity_file_path)

    args.train_decoder = bool(args.train_decoder)
    return args


def _need_gpu(device=None):
    if not torch.cuda.is_available() or (device is not None and torch.device(device).type != 'cuda'):
        raise FmiError("train_psp needs the GPU (there is no CPU path)")


def _check_eval_options(options):
    if 'fid' in options:
        raise FmiError("eval option 'fid' is not built (its InceptionV3 weights are a download); use 'ssim' / 'ms_ssim'")


def _operands(batch, use_ref):
    """(src, gt, ref | None, mask | None) of a batch from to_device_batch (train_psp.py:308-315)"""
    if use_ref:
        return batch['src_img'], batch['gt_img'], batch['ref_img'], batch['true_masks']
    return batch['src_img'], batch['gt_img'], None, None


def train_step(generator, psp_loss, optimizer, batch, args):
    """one optimisation step on a batch from to_device_batch (train_psp.py:308-335).  Returns ``(loss, loss_dict, stepped)``: the loss as
    a detached 0-dim device tensor, the loss terms as device tensors (``defer_logs``), and whether the step was taken -- a non-finite
    loss skips zero_grad / backward / step, as the reference does.  That test is the one host read of the step."""
    src_images, gt_images, ref_images, true_masks = _operands(batch, args.use_ref)
    gen_images, latent = generator(src_images, ref=ref_images, src_mask=true_masks, return_latents=True, randomize_noise=args.randomize_noise)
    psp_loss.defer_logs = True
    loss, loss_dict, _id_logs = psp_loss(src_images, gt_images, gen_images, latent, latent_avg=generator.latent_avg, ref=ref_images, mask=true_masks)
    stepped = bool(torch.isfinite(loss))
    if stepped:
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
    return loss.detach(), loss_dict, stepped


def evaluate(generator, val_loader, psp_loss, device, batch_size, latent_avg=None, use_ref=True, options={'ssim'}):
    """the reference's evaluate (:162-242): mean over the validation batches of the loss and of SSIM / MS-SSIM of ``(gen + 1) / 2``
    against ``raw_gt_img`` (this build's valid-window kernels, constructed as in psp_inference.py), with the reference's forward call
    (its default ``randomize_noise``).  The values are 0-dim device tensors: the caller reads them once, at the end of the round."""
    _check_eval_options(options)
    from .modules.evaluations.msssim import MS_SSIM, SSIM

    generator.eval()
    num_val_batches = len(val_loader)
    metrics = {'val loss': 0}
    if 'ssim' in options:
        ssim_func = SSIM(data_range=1, size_average=True, channel=3)
    if 'ms_ssim' in options:
        ms_ssim_func = MS_SSIM(data_range=1, size_average=True, channel=3)
    defer = getattr(psp_loss, 'defer_logs', None)
    if defer is not None:
        psp_loss.defer_logs = True
    with torch.no_grad():
        for batch in val_loader:
            batch = to_device_batch(batch, device)
            src_images, gt_images, ref_images, true_masks = _operands(batch, use_ref)
            raw_gt_img = batch['raw_gt_img'].contiguous()  # [0 ~ 1]
            gen_images, latent = generator(src_images, ref=ref_images, src_mask=true_masks, return_latents=True)  # [-1 ~ 1]
            loss, _, _ = psp_loss(src_images, gt_images, gen_images, latent, latent_avg=latent_avg, ref=ref_images, mask=true_masks)
            metrics['val loss'] = metrics['val loss'] + loss.detach()
            gen_images = ((gen_images + 1) / 2).contiguous()  # [-1 ~ 1] -> [0 ~ 1]
            if 'ssim' in options:
                metrics['ssim'] = metrics.get('ssim', 0) + ssim_func(gen_images, raw_gt_img)
            if 'ms_ssim' in options:
                metrics['ms_ssim'] = metrics.get('ms_ssim', 0) + ms_ssim_func(gen_images, raw_gt_img)
    if defer is not None:
        psp_loss.defer_logs = defer
    generator.train()
    return {k: v / num_val_batches for k, v in metrics.items()}


def train_net(generator,
              device,
              train_loader,
              val_loader,
              args,
              epochs=5,
              batch_size=1,
              learning_rate=0.001,
              save_checkpoint=True,
              dir_checkpoint=None,
              run_name='',
              eval_options={'ssim'},
              debug=False,
              callback=None,
              history=None,
              psp_loss=None):
    """the reference's train_net (:245-391).  Returns the history: ``losses`` (one float per step taken), ``skipped`` (the 0-based
    batch counts of the steps a non-finite loss skipped), ``val`` (one metrics dict of floats per evaluation round) / ``val_steps`` /
    ``lrs`` (the learning rate after the scheduler saw the round's ``val loss``), ``checkpoints`` (paths).  A dict passed as ``history``
    is filled in place.  ``psp_loss``: the criterion to use instead of ``pSpLoss(args)`` with the fused pixel head."""
    eval_options = set(eval_options)
    _check_eval_options(eval_options)
    if args.optimizer not in ('adam', 'ranger'):
        raise FmiError(f"--optimizer {args.optimizer!r}: 'adam' or 'ranger'")
    _need_gpu(device)
    device = torch.device(device)

    n_train, n_val = _n_items(train_loader), _n_items(val_loader)

    logging.info(f'''Starting training:
        Epochs:          {epochs}
        Batch size:      {batch_size}
        Learning rate:   {learning_rate}
        Training size:   {n_train}
        Validation size: {n_val}
        Checkpoints:     {save_checkpoint}
        Device:          {device}
    ''')

    dir_checkpoint = Path(dir_checkpoint) / Path(run_name)
    dir_checkpoint.mkdir(parents=True, exist_ok=True)

    params = list(generator.encoder.parameters())
    if args.train_decoder:
        params += list(generator.decoder.parameters())
    params = [p for p in params if p.requires_grad]
    if args.optimizer == 'adam':
        optimizer = FusedAdam(params, lr=learning_rate)
    else:
        optimizer = Ranger(params, lr=learning_rate)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, 'max', patience=2, factor=0.8)

    global_step = 0
    seen = 0
    if psp_loss is None:
        psp_loss = pSpLoss(args).to(device)
        psp_loss.fused_head = True
    pending = []  # device scalars of the steps since the last flush
    history = {} if history is None else history
    history.update(losses=[], skipped=[], val=[], val_steps=[], lrs=[], checkpoints=[], n_train=n_train, n_val=n_val)

    def flush():
        if pending:
            history['losses'].extend(torch.stack(pending).tolist())
            pending.clear()

    # 5. Begin training
    for epoch in range(epochs):
        generator.train()
        for batch in train_loader:
            batch = to_device_batch(batch, device)
            loss, loss_dict, stepped = train_step(generator, psp_loss, optimizer, batch, args)
            if stepped:
                global_step += 1
                pending.append(loss)
                if callback is not None:
                    callback({**loss_dict, 'step': global_step, 'epoch': epoch})
            else:
                history['skipped'].append(seen)
                logging.info('batch %d: non-finite loss, step skipped', seen)
            seen += 1

            # Evaluation round
            division_step = (n_train // (10 * batch_size))
            if division_step == 0:
                continue
            if global_step % division_step == 0:
                event = {'learning rate': optimizer.param_groups[0]['lr'], 'step': global_step, 'epoch': epoch}
                if len(eval_options) > 0:
                    metrics = evaluate(generator, val_loader, psp_loss, device, batch_size, use_ref=args.use_ref,
                                       latent_avg=generator.latent_avg, options=eval_options)
                    metrics = {k: float(v) for k, v in metrics.items()}  # the host reads of a round
                    flush()
                    scheduler.step(metrics['val loss'])
                    history['val'].append(metrics)
                    history['val_steps'].append(global_step)
                    history['lrs'].append(optimizer.param_groups[0]['lr'])
                    for k, v in metrics.items():
                        logging.info(f'{k}: {v}')
                        event[k] = v
                if callback is not None:
                    callback(event)

        flush()
        if save_checkpoint:
            path = str(dir_checkpoint / Path(f'G_checkpoint_epoch{epoch + 1}.pth'))
            torch.save(generator.state_dict(), path)
            history['checkpoints'].append(path)
            logging.info(f'Checkpoint {epoch + 1} saved!')

    return history


def _n_items(loader):
    """items behind a loader (train_psp.py:259-260 reads ``len(loader.dataset)`` of a torch Subset): a DeviceLoader's subset, a torch
    DataLoader's dataset, or the batches of a plain sequence"""
    if hasattr(loader, 'indices'):
        return len(loader.indices)
    if hasattr(loader, 'dataset'):
        return len(loader.dataset)
    return sum(int(next(iter(b.values())).shape[0]) for b in loader)


def main(argv=None):
    args = get_args(argv)
    logging.basicConfig(level=logging.INFO, format='%(levelname)s: %(message)s')
    _check_eval_options(set(args.eval_options))
    if args.optimizer not in ('adam', 'ranger'):
        raise FmiError(f"--optimizer {args.optimizer!r}: 'adam' or 'ranger'")
    _need_gpu()
    device = torch.device('cuda')

    # load saved mask detector (frozen; the training loop does not use it, as in the reference)
    mask_detector = MaskDetector(n_channels=3, bilinear=True)
    if args.mask_detector_path:
        mask_detector.load_state_dict(torch.load(args.mask_detector_path, map_location='cpu', weights_only=True))
    base_function._freeze(mask_detector)  # freeze

    # define models
    generator = pSp(args).to(device)
    if generator.latent_avg is None:
        generator.latent_avg = generator.decoder.mean_latent(int(1e5))[0].detach()

    train_loader, val_loader = get_reference_dataloader(args.src_img_path,
                                                        args.ref_img_path,
                                                        args.mask_path,
                                                        args.identity_file_path,
                                                        args.batch_size,
                                                        apply_transform=True,
                                                        val_amount=0.1,
                                                        num_workers=4,
                                                        img_scale=args.img_scale,
                                                        use_ssim=True,
                                                        device=device)

    return train_net(generator,
                     device,
                     train_loader,
                     val_loader,
                     args,
                     epochs=args.epochs,
                     batch_size=args.batch_size,
                     learning_rate=args.learning_rate,
                     save_checkpoint=True,
                     dir_checkpoint=args.checkpoint_path,
                     run_name=args.run_name,
                     eval_options=set(args.eval_options),
                     debug=bool(args.debug))


if __name__ == '__main__':
    main()
