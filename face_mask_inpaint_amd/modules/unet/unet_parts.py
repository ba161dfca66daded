"""Host-side mirror of modules/unet/unet_parts.py (DoubleConv, Down, Up, OutConv) with the reference's parameter names
(``double_conv.N``, ``maxpool_conv.1``, ``up`` / ``conv``); forward on the HIP kernels in NHWC."""
from __future__ import annotations

import torch
import torch.nn as nn

from ... import functional as FF
from ...weights import packed, weight_scope
from ..pluralistic_model.external_function import run_conv
from ..psp.encoders.helpers import batch_norm

BF16 = torch.bfloat16


def _bf16_conv(conv) -> bool:
    """the bf16 convolution family takes this layer (C and K multiples of 32): everything but the 3 -> 64 stem and the head"""
    return conv.in_channels % 32 == 0 and conv.out_channels % 32 == 0


def _mark_bf16(module: nn.Module, compute_dtype):
    """convolutions that run on bf16 activations are packed without fp32 piece images (weights.weight_scope reads the mark)"""
    if compute_dtype not in (torch.float32, BF16):
        raise FF.FmiError(f"compute_dtype must be torch.float32 or torch.bfloat16, got {compute_dtype}")
    for m in module.modules():
        if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3):
            object.__setattr__(m, "_fmi_no_w3", compute_dtype == BF16 and _bf16_conv(m))


def _conv_bn_relu_bf16(conv, bn, x):
    """relu(bn(conv(x))) on bf16 NHWC.  Batch statistics: the bf16 convolution, then BatchNorm + ReLU as one pass each way; the
    convolution's bias cancels in the mean subtraction, so it is not applied and receives an exact zero gradient (the running mean still includes it).  Running statistics
    (eval): one launch, gradients off."""
    pw = packed(conv)
    if bn.training or not bn.track_running_stats:
        y = FF.conv2d(x, pw, stride=1, pad=conv.padding[0])
        if conv.bias is not None and conv.bias.requires_grad:
            y = FF.zero_grad_of(y, conv.bias)
        return batch_norm(bn, y, slope=0.0, mean_offset=conv.bias)  # the running mean is that of conv(x) + bias
    return FF.conv_bn_relu_eval_bf16(x, pw, conv.bias, bn, pad=conv.padding[0])


class _Nhwc(nn.Module):
    compute_dtype = torch.float32

    def forward(self, *xs):
        """fp32 NCHW-shaped tensors in and out in either compute dtype"""
        if self.compute_dtype == BF16:
            xs = [FF.to_nhwc(x) for x in xs]
            xs = [x.to(BF16) if x.shape[-1] % 32 == 0 else x for x in xs]
            return FF.to_nchw(self.nhwc(*xs).float())
        return FF.to_nchw(self.nhwc(*[FF.to_nhwc(x) for x in xs]))


class DoubleConv(_Nhwc):
    """(convolution => [BN] => ReLU) * 2   (unet_parts.py:8-27)"""

    def __init__(self, in_channels, out_channels, mid_channels=None, compute_dtype=torch.float32):
        super().__init__()
        self.compute_dtype = compute_dtype
        if not mid_channels:
            mid_channels = out_channels
        self.double_conv = nn.Sequential(
            nn.Conv2d(in_channels, mid_channels, kernel_size=3, padding=1), nn.BatchNorm2d(mid_channels), nn.ReLU(inplace=True),
            nn.Conv2d(mid_channels, out_channels, kernel_size=3, padding=1), nn.BatchNorm2d(out_channels), nn.ReLU(inplace=True))
        _mark_bf16(self, compute_dtype)

    def nhwc(self, x):
        with weight_scope(self):
            for conv, bn in ((self.double_conv[0], self.double_conv[1]), (self.double_conv[3], self.double_conv[4])):
                if self.compute_dtype == BF16 and _bf16_conv(conv):
                    if x.dtype != BF16:  # the stem's result enters the bf16 body after its BN + ReLU
                        x = x.to(BF16)
                    x = _conv_bn_relu_bf16(conv, bn, x)
                    continue
                x = FF.leaky_relu(batch_norm(bn, run_conv(conv, x)), 0.0)
            return x


class Down(_Nhwc):
    """MaxPool2d(2) then DoubleConv (unet_parts.py:30-42)"""

    def __init__(self, in_channels, out_channels, compute_dtype=torch.float32):
        super().__init__()
        self.compute_dtype = compute_dtype
        self.maxpool_conv = nn.Sequential(nn.MaxPool2d(2), DoubleConv(in_channels, out_channels, compute_dtype=compute_dtype))

    def nhwc(self, x):
        with weight_scope(self):
            return self.maxpool_conv[1].nhwc(FF.max_pool(x, 2, 2))


class Up(_Nhwc):
    """bilinear x2 (align_corners=True) or ConvTranspose2d(k2, s2), pad to the skip's size, concat [skip, up], DoubleConv
    (unet_parts.py:45-72)"""

    def __init__(self, in_channels, out_channels, bilinear=True, compute_dtype=torch.float32):
        super().__init__()
        self.compute_dtype = compute_dtype
        if bilinear:
            self.up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)
            self.conv = DoubleConv(in_channels, out_channels, in_channels // 2, compute_dtype=compute_dtype)
        else:
            self.up = nn.ConvTranspose2d(in_channels, in_channels // 2, kernel_size=2, stride=2)
            self.conv = DoubleConv(in_channels, out_channels, compute_dtype=compute_dtype)

    def nhwc(self, x1, x2):
        with weight_scope(self):
            if self.compute_dtype == BF16:
                if not isinstance(self.up, nn.Upsample):
                    raise NotImplementedError("Up(bilinear=False): every caller of the reference builds MaskDetector(bilinear=True)")
                return self.conv.nhwc(FF.up2_cat(x1, x2))  # upsample, zero border and concat in one pass
            if isinstance(self.up, nn.Upsample):
                x1 = FF.resize_bilinear(x1, 2 * x1.shape[1], 2 * x1.shape[2])
            else:
                raise NotImplementedError("Up(bilinear=False): every caller of the reference builds MaskDetector(bilinear=True)")
            dy, dx = x2.shape[1] - x1.shape[1], x2.shape[2] - x1.shape[2]
            if dy or dx:  # odd input sizes only: zero border (torch plumbing, copies a few rows)
                x1 = torch.nn.functional.pad(x1, [0, 0, dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])
            return self.conv.nhwc(FF.cat_channels(x2, x1))


class OutConv(_Nhwc):
    def __init__(self, in_channels, out_channels, compute_dtype=torch.float32):
        super().__init__()
        self.compute_dtype = compute_dtype
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size=1)
        if compute_dtype not in (torch.float32, BF16):
            raise FF.FmiError(f"compute_dtype must be torch.float32 or torch.bfloat16, got {compute_dtype}")

    def nhwc(self, x):
        """fp32 logits in either compute dtype"""
        if x.dtype == BF16:
            return FF.head1x1(x, self.conv.weight, self.conv.bias)
        with weight_scope(self):
            return run_conv(self.conv, x)

    def argmax_nhwc(self, x):
        """argmax over the classes as a float mask [N, H, W]; on bf16 activations the logits are never stored"""
        if x.dtype == BF16:
            return FF.head1x1_argmax(x, self.conv.weight, self.conv.bias)
        return FF.argmax_channels(self.nhwc(x))

    def forward(self, x):
        if self.compute_dtype == BF16:
            return FF.to_nchw(self.nhwc(FF.to_nhwc(x).to(BF16)))
        return super().forward(x)
