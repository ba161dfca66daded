"""Trainer of the UNet mask detector -- the counterpart of the reference's train_mask_detector.py, whose checkpoints both inference
harnesses load from ``--mask_detector_path``.

Same command line (``get_args``), same objective (CrossEntropyLoss + multiclass Dice loss on ``mask > 0``, :127-134), same validation
metric and cadence (``evaluate`` :24-58, ten rounds per epoch :152-154), ``ReduceLROnPlateau('max', patience=2)`` on the validation
Dice score (:107,162) and one ``checkpoint_epoch{n}.pth`` state_dict per epoch (:178-181) with the reference's key names.  What differs:

  * the logits stay NHWC and the whole loss is FF.seg_ce_dice_loss (2 launches forward, 1 backward, no NCHW copy, no ``.item()``);
    the metric is FF.seg_dice_score (the reference's dice_coeff reads ``sets_sum.item()`` per sample and class);
  * Adam is optim.FusedAdam; batches arrive as device tensors from dataloader.BasicDataset;
  * logging goes through ``logging`` and an optional ``callback(event: dict)`` -- no wandb, no tqdm;
  * ``train_step`` never synchronises with the host.  The one synchronisation per evaluation round is the ``float()`` that
    ReduceLROnPlateau needs; per-step losses stay device scalars until that read (or the end of the epoch);
  * ``--amp`` is refused: fp16 autocast with a GradScaler is not built.  What is built is the bf16 UNet body (fp32 master weights,
    statistics and parameter gradients; no loss scaling needed): ``train_net(..., dtype="bf16")``, or on the command line the
    environment variable ``FMI_MASK_DETECTOR_DTYPE=bf16`` (``fp32`` is the default; ``get_args`` keeps exactly the reference's flags).
    The bf16 body needs image sizes that are multiples of 16; checkpoints are the same in either dtype.
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
from pathlib import Path

import torch
from torch.utils.data import DataLoader, random_split

from . import functional as FF
from ._lib import FmiError
from .dataloader import BasicDataset
from .modules.mask_detector import MaskDetector
from .optim import FusedAdam

DIR_IMG = Path('../CelebAHQ/images_masked')
DIR_MASK = Path('../CelebAHQ/binary_map')
DIR_CHECKPOINT = Path('./checkpoints256_mask_detector/')


DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def set_compute_dtype(net, compute_dtype):
    """put ``net`` (a MaskDetector) on the fp32 or the bf16 UNet body in place: parameters, buffers and the state_dict do not change"""
    from .modules.unet.unet_parts import _mark_bf16

    for m in net.modules():
        if hasattr(m, "compute_dtype"):
            m.compute_dtype = compute_dtype
    _mark_bf16(net, compute_dtype)
    return net


def train_step(net, optimizer, images, true_masks):
    """one optimisation step on a device batch (train_mask_detector.py:126-139): images [N, 3, H, W] fp32, true_masks [N, H, W] as the
    dataset yields them (int64; ``> 0`` is applied inside the loss kernel).  Returns the loss as a 0-dim device tensor; no host sync."""
    logits = net.model.nhwc(FF.to_nhwc(images))
    loss, _ce, _dice = FF.seg_ce_dice_loss(logits, true_masks)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    return loss.detach()


def evaluate(net, dataloader, device):
    """mean over the validation batches of the Dice score of the argmax prediction, background ignored (train_mask_detector.py:24-58);
    0 when there are no batches.  A 0-dim device tensor (or the int 0): the caller decides when to read it."""
    net.eval()
    num_val_batches = len(dataloader)
    dice_score = 0
    with torch.no_grad():
        for batch in dataloader:
            image = batch['image'].to(device=device, dtype=torch.float32)
            dice_score = dice_score + FF.seg_dice_score(net.model.nhwc(FF.to_nhwc(image)), batch['mask'].to(device))
    net.train()
    if num_val_batches == 0:
        return dice_score
    return dice_score / num_val_batches


def train_net(net,
              device,
              epochs: int = 5,
              batch_size: int = 1,
              learning_rate: float = 0.001,
              val_percent: float = 0.1,
              save_checkpoint: bool = True,
              img_scale: float = 0.5,
              amp: bool = False,
              dir_img=DIR_IMG,
              dir_mask=DIR_MASK,
              dir_checkpoint=DIR_CHECKPOINT,
              seed=None,
              callback=None,
              history=None,
              dtype: str = "fp32"):
    """the reference's train_net (:61-181).  Returns the history: ``losses`` (one float per step), ``val_scores`` / ``val_steps`` /
    ``lrs`` (one entry per evaluation round; the learning rate after the scheduler saw the score), ``checkpoints`` (paths).  A dict
    passed as ``history`` is filled in place, so a caller that catches an exception (``main`` on Ctrl-C) still holds what was recorded.
    Per-step losses wait on the device until the next point that synchronises anyway (a validation round, the end of an epoch)."""
    if dtype not in DTYPES:
        raise FmiError(f"dtype must be one of {sorted(DTYPES)}, got {dtype!r}")
    if amp:
        raise FmiError('--amp: fp16 autocast with a GradScaler is not built; run without --amp and use dtype="bf16" '
                       '(FMI_MASK_DETECTOR_DTYPE=bf16 on the command line) for the bf16 UNet body')
    device = torch.device(device)
    if device.type != 'cuda':
        raise FmiError("train_mask_detector needs the GPU (there is no CPU path)")

    have = getattr(net, "compute_dtype", torch.float32)
    if have != DTYPES[dtype]:
        if dtype == "fp32":  # never take a net that was built for bf16 off its body behind the caller's back
            raise FmiError('dtype="fp32" (the default) but the net was built with compute_dtype=torch.bfloat16: pass dtype="bf16", '
                           'or set_compute_dtype(net, torch.float32) first')
        net = set_compute_dtype(net, DTYPES[dtype])

    # 1. Create dataset
    dataset = BasicDataset(dir_img, dir_mask, img_scale, device=device)

    # 2. Split into train / validation partitions
    n_val = int(len(dataset) * val_percent)
    n_train = len(dataset) - n_val
    seeded = dict(generator=torch.Generator().manual_seed(seed)) if seed is not None else {}  # one stream: the split, then the shuffles
    train_set, val_set = random_split(dataset, [n_train, n_val], **seeded)

    # 3. Create data loaders (items are device tensors: batches are stacked on the calling process)
    train_loader = DataLoader(train_set, shuffle=True, batch_size=batch_size, num_workers=0, **seeded)
    val_loader = DataLoader(val_set, shuffle=False, drop_last=True, batch_size=batch_size, num_workers=0)

    logging.info(f'''Starting training:
        Epochs:          {epochs}
        Batch size:      {batch_size}
        Learning rate:   {learning_rate}
        Training size:   {n_train}
        Validation size: {n_val}
        Checkpoints:     {save_checkpoint}
        Device:          {device}
        Images scaling:  {img_scale}
        Mixed Precision: {amp}
    ''')

    # 4. Set up the optimizer and the learning rate scheduler
    optimizer = FusedAdam(net.parameters(), lr=learning_rate)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, 'max', patience=2)  # goal: maximize Dice score
    global_step = 0
    pending = []  # device scalars of the steps since the last flush
    history = {} if history is None else history
    history.update(losses=[], val_scores=[], val_steps=[], lrs=[], checkpoints=[], n_train=n_train, n_val=n_val)

    def flush():
        if pending:
            history['losses'].extend(torch.stack(pending).tolist())
            pending.clear()

    # 5. Begin training
    for epoch in range(epochs):
        net.train()
        for batch in train_loader:
            images, true_masks = batch['image'], batch['mask']
            assert images.shape[1] == net.n_channels, \
                f'Network has been defined with {net.n_channels} input channels, ' \
                f'but loaded images have {images.shape[1]} channels. Please check that ' \
                'the images are loaded correctly.'
            images = images.to(device=device, dtype=torch.float32)
            loss = train_step(net, optimizer, images, true_masks.to(device))
            pending.append(loss)
            global_step += 1
            if callback is not None:
                callback({'train loss': loss, 'step': global_step, 'epoch': epoch})

            # Evaluation round
            division_step = (n_train // (10 * batch_size))
            if division_step > 0 and global_step % division_step == 0:
                val_score = float(evaluate(net, val_loader, device))  # the one host read of a round
                flush()
                scheduler.step(val_score)
                lr = optimizer.param_groups[0]['lr']
                history['val_scores'].append(val_score)
                history['val_steps'].append(global_step)
                history['lrs'].append(lr)
                logging.info('Validation Dice score: {}'.format(val_score))
                if callback is not None:
                    callback({'learning rate': lr, 'validation Dice': val_score, 'step': global_step, 'epoch': epoch})

        flush()
        if save_checkpoint:
            Path(dir_checkpoint).mkdir(parents=True, exist_ok=True)
            path = str(Path(dir_checkpoint) / 'checkpoint_epoch{}.pth'.format(epoch + 1))
            torch.save(net.state_dict(), path)
            history['checkpoints'].append(path)
            logging.info(f'Checkpoint {epoch + 1} saved!')

    return history


def get_args(argv=None):
    parser = argparse.ArgumentParser(description='Train the UNet on images and target masks')
    parser.add_argument('--epochs', '-e', metavar='E', type=int, default=5, help='Number of epochs')
    parser.add_argument('--batch-size', '-b', dest='batch_size', metavar='B', type=int, default=1, help='Batch size')
    parser.add_argument('--learning-rate', '-l', metavar='LR', type=float, default=0.00001,
                        help='Learning rate', dest='lr')
    parser.add_argument('--load', '-f', type=str, default=False, help='Load model from a .pth file')
    parser.add_argument('--scale', '-s', type=float, default=1, help='Downscaling factor of the images')
    parser.add_argument('--validation', '-v', dest='val', type=float, default=10.0,
                        help='Percent of the data that is used as validation (0-100)')
    parser.add_argument('--amp', action='store_true', default=False, help='Use mixed precision (refused: fp16 autocast is not built; FMI_MASK_DETECTOR_DTYPE=bf16 selects the bf16 body)')
    parser.add_argument('--threshold', '-t', type=float, default=0.5, help='Threshold for deciding mask')

    return parser.parse_args(argv)


def main(argv=None):
    args = get_args(argv)

    logging.basicConfig(level=logging.INFO, format='%(levelname)s: %(message)s')
    if not torch.cuda.is_available():
        raise FmiError("train_mask_detector needs the GPU (there is no CPU path)")
    device = torch.device('cuda')
    logging.info(f'Using device {device}')

    # n_channels=3 for RGB images; two classes (mask / no mask)
    dtype = os.environ.get("FMI_MASK_DETECTOR_DTYPE", "fp32")
    if dtype not in DTYPES:
        raise FmiError(f"FMI_MASK_DETECTOR_DTYPE: dtype must be one of {sorted(DTYPES)}, got {dtype!r}")
    net = MaskDetector(n_channels=3, bilinear=True, threshold=args.threshold, compute_dtype=DTYPES[dtype])

    logging.info(f'Network:\n'
                 f'\t{net.n_channels} input channels\n'
                 f'\t2 output channels (classes)\n'
                 f'\t{"Bilinear" if net.bilinear else "Transposed conv"} upscaling')

    if args.load:
        net.load_state_dict(torch.load(args.load, map_location=device, weights_only=True))
        logging.info(f'Model loaded from {args.load}')

    net.to(device=device)
    history = {}
    try:
        return train_net(net=net,
                         history=history,
                         epochs=args.epochs,
                         batch_size=args.batch_size,
                         learning_rate=args.lr,
                         device=device,
                         img_scale=args.scale,
                         val_percent=args.val / 100,
                         amp=args.amp,
                         dtype=dtype)
    except KeyboardInterrupt:
        torch.save(net.state_dict(), 'INTERRUPTED.pth')
        logging.info('Saved interrupt after %d recorded steps, %d validation rounds',
                     len(history.get('losses', [])), len(history.get('val_scores', [])))
        sys.exit(0)


if __name__ == '__main__':
    main()
