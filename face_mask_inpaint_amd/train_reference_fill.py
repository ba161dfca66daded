"""Trainer of the PICNet reference-fill generator -- the counterpart of the reference's train_reference_fill.py (the workload bench.py
measures one step of), whose checkpoints PICNet_inference.py loads.

Same command line (``get_args`` :20-85, with the path joins onto ``--data_root`` and ``pt_ckpt_path`` cleared for a non-pluralistic
encoder), same construction (``process_params`` :88-104, ``load_networks`` :107-140, ReferenceFill / define_d :159-165), same step
(generator forward, ``GANOptimizer.__call__`` :342-346), same validation (``evaluate`` :193-263: both nets in ``eval()``, ``calc_loss``,
SSIM / MS-SSIM of ``(gt, gen)``) on the reference's cadence (``n_train // (10 * batch_size)`` :368-371), two
``ReduceLROnPlateau('max', patience=2, factor=0.8)`` stepped with the D and G validation LOSSES (:310-319,403-404 -- the reference's
literal choice, kept) and ``G_checkpoint_epoch{n}.pth`` / ``D_checkpoint_epoch{n}.pth`` state_dicts per epoch (:410-415).  What differs:

  * the image side of the loss is FF.gan_image_head (``GANOptimizer.fused_head``): one pass forward, one launch backward;
  * Adam is optim.FusedAdam; batches arrive as device tensors from dataloader.get_reference_dataloader / to_device_batch, whose
    ``true_masks`` is the reference's ``(mask > 0).float()``;
  * logging goes through ``logging`` and an optional ``callback(event: dict)``: no wandb, no tqdm, no histograms or images;
  * loss values and validation metrics stay device scalars until the end of an evaluation round or of the epoch;
  * the environment variable ``FMI_ATTENTION_DTYPE=bf16`` (``fp32`` is the default; ``get_args`` keeps exactly the reference's flags)
    runs the generator's ``attn1`` on the bf16 attention kernels, forward and backward, in the otherwise fp32 model -- read by
    ``ReferenceFill`` where it is built, same parameters and checkpoints.

``load_networks`` reproduces the reference literally -- including that for G and E it collects the MODEL'S OWN tensors for
every key whose shape matches the checkpoint (``matches[k] = v`` at :123-126 takes ``v`` from ``generator.decoder.state_dict()``,
not from the file), so those two loads are value-preserving, and a key missing from the file raises KeyError exactly as there;
only D is really loaded (strict).  ``copy_pretrained=True`` is this build's fix: the matching tensors are taken from the file.

Out of scope: multi-GPU ranks, replaying the step as a HIP graph, FID (``'fid'`` in ``--eval_options`` is refused: its InceptionV3 is a
download) and the DRN encoder's pretrained download."""
from __future__ import annotations

import argparse
import logging
import os
from pathlib import Path

import torch

from ._lib import FmiError


# the reference trainer's command line (train_reference_fill.py:20-74): flag -> (type, default)
_FLAGS = {
    'epochs': (int, 5), 'batch_size': (int, 8), 'learning_rate': (float, 1e-5), 'debug': (int, 0), 'img_scale': (float, 1.),
    'run_name': (str, ''), 'checkpoint_path': (str, 'saved_model'), 'mask_detector_path': (str, ''),
    'data_root': (str, '/data/mohaa/project1/CelebA'), 'src_img_path': (str, 'img_align_celeba_masked1'),
    'ref_img_path': (str, 'img_align_celeba'), 'mask_path': (str, 'binary_map'), 'identity_file_path': (str, 'identity_CelebA.txt'),
    'use_best_reference': (int, 0), 'pt_ckpt_path': (str, ''),
    'encoder_ngf': (int, 32), 'encoder_z_nc': (int, 128), 'encoder_img_f': (int, 128), 'encoder_layers': (int, 5),
    'encoder_norm': (str, 'none'), 'encoder_activation': (str, 'LeakyReLU'), 'encoder_init_type': (str, 'orthogonal'),
    'decoder_ngf': (int, 32), 'decoder_z_nc': (int, 128), 'decoder_img_f': (int, 128), 'decoder_L': (int, 0), 'decoder_layers': (int, 5),
    'decoder_norm': (str, 'instance'), 'decoder_activation': (str, 'LeakyReLU'), 'decoder_init_type': (str, 'orthogonal'),
    'disc_ndf': (int, 32), 'disc_layers': (int, 5), 'disc_model_type': (str, 'ResDis'), 'disc_init_type': (str, 'orthogonal'),
    'use_att': (int, 1),
}
_DATA_PATHS = ('src_img_path', 'ref_img_path', 'mask_path', 'identity_file_path')


def get_args(argv=None):
    """the reference's flags and defaults; the four data paths are joined onto ``--data_root`` and ``--pt_ckpt_path`` only applies to the
    'pluralistic' encoder (:76-83)"""
    parser = argparse.ArgumentParser(description='train the PICNet reference-fill generator')
    for name, (kind, default) in _FLAGS.items():
        parser.add_argument('--' + name, type=kind, default=default)
    parser.add_argument('--eval_options', nargs='+', default={'ssim'}, help="any of 'ssim', 'ms_ssim'")
    parser.add_argument('--encoder_type', type=str, default='pluralistic', choices=['pluralistic', 'drn'])
    args = parser.parse_args(argv)
    for name in _DATA_PATHS:
        setattr(args, name, os.path.join(args.data_root, getattr(args, name)))
    if args.encoder_type != 'pluralistic':
        args.pt_ckpt_path = ''
    return args


def process_params(args):
    encoder_params = {k.replace("encoder_", ""): v for k, v in args._get_kwargs() if k.startswith("encoder")}
    decoder_params = {k.replace("decoder_", ""): v for k, v in args._get_kwargs() if k.startswith("decoder")}
    disc_params = {k.replace("disc_", ""): v for k, v in args._get_kwargs() if k.startswith("disc")}
    disc_params["img_f"] = encoder_params["img_f"]
    return encoder_params, decoder_params, disc_params


def _matches(module, pretrained_dict, copy_pretrained):
    out = {}
    for k, v in module.state_dict().items():
        if v.shape == pretrained_dict[k].shape:  # KeyError for a key the checkpoint lacks, as in the reference
            out[k] = pretrained_dict[k] if copy_pretrained else v
    return out


def load_networks(generator, discriminator, path, copy_pretrained=False):
    """Load all the networks from the disk (train_reference_fill.py:107-140).  Checkpoints are read with
    ``weights_only=True`` (tensor-only state_dicts; nothing from the file is executed)."""
    if not path:
        return
    for name in ["G", "E", "D"]:
        ckpt_path = os.path.join(path, f"latest_net_{name}.pth")
        if not os.path.isfile(ckpt_path):
            continue
        pretrained_dict = {k.replace("module.", "", 1): v for k, v in torch.load(ckpt_path, map_location="cpu", weights_only=True).items()}
        if name == "G":
            generator.decoder.load_state_dict(_matches(generator.decoder, pretrained_dict, copy_pretrained), strict=False)
        elif name == "E":
            generator.src_encoder.load_state_dict(_matches(generator.src_encoder, pretrained_dict, copy_pretrained), strict=False)
            generator.ref_encoder.load_state_dict(_matches(generator.ref_encoder, pretrained_dict, copy_pretrained), strict=False)
        elif name == "D":
            discriminator.load_state_dict(pretrained_dict, strict=True)  # discriminator did not change: strict loading


def _need_gpu(device=None):
    if not torch.cuda.is_available() or (device is not None and torch.device(device).type != 'cuda'):
        raise FmiError("train_reference_fill needs the GPU (there is no CPU path)")


def _check_eval_options(options):
    if 'fid' in options:
        raise FmiError("eval option 'fid' is not built (its InceptionV3 weights are a download); use 'ssim' / 'ms_ssim'")


def build_models(args, device=None):
    """(generator, discriminator) as the reference's main constructs them (:149-165): the frozen mask detector, ReferenceFill and
    define_d from ``process_params``, then ``load_networks``"""
    from .modules.mask_detector import MaskDetector
    from .modules.model import ReferenceFill
    from .modules.pluralistic_model import base_function, network

    # load saved mask detector
    mask_detector = MaskDetector(n_channels=3, bilinear=True)
    if args.mask_detector_path:
        mask_detector.load_state_dict(torch.load(args.mask_detector_path, map_location='cpu', weights_only=True))
    base_function._freeze(mask_detector)  # freeze

    # process encoder, decoder, discriminator args
    encoder_params, decoder_params, disc_params = process_params(args)

    # define models
    generator = ReferenceFill(mask_detector, encoder_params, decoder_params, use_att=args.use_att)
    discriminator = network.define_d(**disc_params)
    if device is not None:
        generator, discriminator = generator.to(device), discriminator.to(device)
    load_networks(generator, discriminator, args.pt_ckpt_path)
    return generator, discriminator


def evaluate(generator, discriminator, val_loader, calc_loss, device, batch_size, options={'ssim'}):
    """the reference's evaluate (:193-263): both nets in ``eval()``, under no_grad the mean over the validation batches of the two
    ``calc_loss`` values and of SSIM / MS-SSIM of ``(gt, gen)`` (this build's valid-window kernels), then both nets back in ``train()``.
    The values are 0-dim device tensors: the caller reads them once, at the end of the round."""
    _check_eval_options(options)
    from .dataloader import to_device_batch
    from .modules.evaluations.msssim import MS_SSIM, SSIM

    generator.eval()
    discriminator.eval()
    num_val_batches = len(val_loader)
    metrics = {'D validation loss': 0, 'G validation loss': 0}
    if 'ssim' in options:
        ssim_loss = SSIM(data_range=1, size_average=True, channel=3)
    if 'ms_ssim' in options:
        ms_ssim_loss = MS_SSIM(data_range=1, size_average=True, channel=3)
    with torch.no_grad():
        for batch in val_loader:
            batch = to_device_batch(batch, device)
            src_images, ref_images, gt_images, true_masks = batch['src_img'], batch['ref_img'], batch['gt_img'], batch['true_masks']
            gen_images = generator(src_images, ref_images, src_mask=true_masks)  # [N, 3, H, W]
            loss_D, loss_G = calc_loss(discriminator, src_images, gt_images, ref_images, gen_images, true_masks)
            metrics['D validation loss'] = metrics['D validation loss'] + loss_D.detach()
            metrics['G validation loss'] = metrics['G validation loss'] + loss_G.detach()
            if 'ssim' in options:
                metrics['ssim'] = metrics.get('ssim', 0) + ssim_loss(gt_images.contiguous(), gen_images.contiguous())
            if 'ms_ssim' in options:
                metrics['ms_ssim'] = metrics.get('ms_ssim', 0) + ms_ssim_loss(gt_images.contiguous(), gen_images.contiguous())
    generator.train()
    discriminator.train()
    return {k: v / num_val_batches for k, v in metrics.items()}


def train_net(generator,
              discriminator,
              device,
              train_loader,
              val_loader,
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
              gan_optimizer=None):
    """the reference's train_net (:266-415).  Returns the history: ``losses_G`` / ``losses_D`` (one float per step), ``val`` (one metrics
    dict of floats per evaluation round) / ``val_steps`` / ``lrs_G`` / ``lrs_D`` (the learning rates after the schedulers saw the round's
    validation losses), ``checkpoints`` (paths), ``n_train`` / ``n_val``.  A dict passed as ``history`` is filled in place.
    ``gan_optimizer``: the GANOptimizer to use (it is handed this run's two optimisers) instead of
    ``GANOptimizer(optimizer_D, optimizer_G, debug=debug)`` with the fused image head."""
    eval_options = set(eval_options)
    _check_eval_options(eval_options)
    _need_gpu(device)
    device = torch.device(device)
    from .dataloader import to_device_batch
    from .modules.loss import GANOptimizer
    from .optim import FusedAdam

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

    # 4. Set up the optimizers, the loss and the learning rate schedulers
    optimizer_G = FusedAdam([p for p in generator.parameters() if p.requires_grad], lr=learning_rate)
    scheduler_G = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer_G, 'max', patience=2, factor=0.8)
    optimizer_D = FusedAdam([p for p in discriminator.parameters() if p.requires_grad], lr=learning_rate)
    scheduler_D = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer_D, 'max', patience=2, factor=0.8)

    if gan_optimizer is None:
        gan_optimizer = GANOptimizer(optimizer_D, optimizer_G, debug=debug).to(device)
        gan_optimizer.fused_head = True
    else:  # the caller's criterion (its VGG, lambdas, fused_head) on this run's optimisers
        gan_optimizer.optimizer_D, gan_optimizer.optimizer_G = optimizer_D, optimizer_G
    global_step = 0
    pending_G, pending_D = [], []  # device scalars of the steps since the last flush
    history = {} if history is None else history
    history.update(losses_G=[], losses_D=[], val=[], val_steps=[], lrs_G=[], lrs_D=[], checkpoints=[], n_train=n_train, n_val=n_val)

    def flush():
        for pending, key in ((pending_G, 'losses_G'), (pending_D, 'losses_D')):
            if pending:
                history[key].extend(torch.stack(pending).tolist())
                pending.clear()

    # 5. Begin training
    for epoch in range(epochs):
        generator.train()
        discriminator.train()
        for batch in train_loader:
            batch = to_device_batch(batch, device)
            src_images, ref_images, gt_images, true_masks = batch['src_img'], batch['ref_img'], batch['gt_img'], batch['true_masks']

            gen_images = generator(src_images, ref_images, src_mask=true_masks)

            loss_D, loss_G, perc_loss, style_loss, cx_loss = gan_optimizer(discriminator, src_images, gt_images, ref_images, gen_images, true_masks)

            global_step += 1
            pending_G.append(loss_G.detach())
            pending_D.append(loss_D.detach())
            if callback is not None:
                callback({'G train loss': loss_G.detach(), 'D train loss': loss_D.detach(), 'perc': perc_loss.detach(), 'style': style_loss.detach(),
                          'context': cx_loss.detach(), 'step': global_step, 'epoch': epoch})

            # Evaluation round
            division_step = (n_train // (10 * batch_size))
            if division_step == 0:
                continue
            if global_step % division_step == 0:
                event = {'[G] learning rate': optimizer_G.param_groups[0]['lr'], '[D] learning rate': optimizer_D.param_groups[0]['lr'],
                         'step': global_step, 'epoch': epoch}
                if len(eval_options) > 0:
                    metrics = evaluate(generator, discriminator, val_loader, gan_optimizer.calc_loss, device, batch_size, eval_options)
                    metrics = {k: float(v) for k, v in metrics.items()}  # the host reads of a round
                    flush()
                    scheduler_D.step(metrics['D validation loss'])
                    scheduler_G.step(metrics['G validation loss'])
                    history['val'].append(metrics)
                    history['val_steps'].append(global_step)
                    history['lrs_G'].append(optimizer_G.param_groups[0]['lr'])
                    history['lrs_D'].append(optimizer_D.param_groups[0]['lr'])
                    for k, v in metrics.items():
                        logging.info(f'{k}: {v}')
                        event[k] = v
                if callback is not None:
                    callback(event)

        flush()
        if save_checkpoint:
            for net, tag in ((generator, 'G'), (discriminator, 'D')):
                path = str(dir_checkpoint / Path(f'{tag}_checkpoint_epoch{epoch + 1}.pth'))
                torch.save(net.state_dict(), path)
                history['checkpoints'].append(path)
            logging.info(f'Checkpoint {epoch + 1} saved!')

    return history


def _n_items(loader):
    """items behind a loader (train_reference_fill.py:280-281 reads ``len(loader.dataset)`` of a torch Subset): a DeviceLoader's subset,
    a torch DataLoader's dataset, or the batches of a plain sequence"""
    if hasattr(loader, 'indices'):
        return len(loader.indices)
    if hasattr(loader, 'dataset'):
        return len(loader.dataset)
    return sum(int(next(iter(b.values())).shape[0]) for b in loader)


def main(argv=None):
    args = get_args(argv)
    logging.basicConfig(level=logging.INFO, format='%(levelname)s: %(message)s')
    _check_eval_options(set(args.eval_options))
    _need_gpu()
    device = torch.device('cuda')
    from .dataloader import get_reference_dataloader

    generator, discriminator = build_models(args, device)

    train_loader, val_loader = get_reference_dataloader(args.src_img_path,
                                                        args.ref_img_path,
                                                        args.mask_path,
                                                        args.identity_file_path,
                                                        args.batch_size,
                                                        apply_transform=False,
                                                        val_amount=0.1,
                                                        num_workers=4,
                                                        img_scale=args.img_scale,
                                                        use_ssim=args.use_best_reference,
                                                        device=device)

    return train_net(generator,
                     discriminator,
                     device,
                     train_loader,
                     val_loader,
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
