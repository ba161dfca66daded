"""Host-side mirror of modules/unet/unet_model.py: UNet(n_channels, n_classes, bilinear) -- the mask detector's network."""
from __future__ import annotations

import torch
from torch import nn

from ... import functional as FF
from ...weights import weight_scope
from .unet_parts import DoubleConv, Down, OutConv, Up


class UNet(nn.Module):
    def __init__(self, n_channels, n_classes, bilinear=True, compute_dtype=torch.float32):
        """compute_dtype = torch.bfloat16: the 3 -> 64 stem convolution (with its BN + ReLU) stays fp32, everything from there to the
        head keeps bf16 NHWC activations (fp32 accumulation, fp32 parameters, statistics and parameter gradients); the logits are fp32.
        The state_dict is the same in either dtype."""
        super().__init__()
        self.n_channels, self.n_classes, self.bilinear = n_channels, n_classes, bilinear
        self.compute_dtype = dt = compute_dtype
        if dt == torch.bfloat16 and n_classes > 4:
            raise FF.FmiError("the bf16 head takes at most 4 classes")
        self.inc = DoubleConv(n_channels, 64, compute_dtype=dt)
        self.down1 = Down(64, 128, compute_dtype=dt)
        self.down2 = Down(128, 256, compute_dtype=dt)
        self.down3 = Down(256, 512, compute_dtype=dt)
        factor = 2 if bilinear else 1
        self.down4 = Down(512, 1024 // factor, compute_dtype=dt)
        self.up1 = Up(1024, 512 // factor, bilinear, compute_dtype=dt)
        self.up2 = Up(512, 256 // factor, bilinear, compute_dtype=dt)
        self.up3 = Up(256, 128 // factor, bilinear, compute_dtype=dt)
        self.up4 = Up(128, 64, bilinear, compute_dtype=dt)
        self.outc = OutConv(64, n_classes, compute_dtype=dt)

    def features_nhwc(self, x):
        """everything in front of the head: fp32 NHWC image -> [N, H, W, 64] in the compute dtype"""
        if self.compute_dtype == torch.bfloat16 and (x.shape[1] % 16 or x.shape[2] % 16):
            raise FF.FmiError(f"the bf16 UNet body needs H and W to be multiples of 16 (four 2 x 2 poolings), got {x.shape[1]} x {x.shape[2]}; "
                              "odd sizes run on compute_dtype=torch.float32")
        with weight_scope(self):
            x1 = self.inc.nhwc(x)
            x2 = self.down1.nhwc(x1)
            x3 = self.down2.nhwc(x2)
            x4 = self.down3.nhwc(x3)
            x5 = self.down4.nhwc(x4)
            x = self.up1.nhwc(x5, x4)
            x = self.up2.nhwc(x, x3)
            x = self.up3.nhwc(x, x2)
            return self.up4.nhwc(x, x1)

    def nhwc(self, x):
        with weight_scope(self):
            return self.outc.nhwc(self.features_nhwc(x))

    def argmax_nhwc(self, x):
        """float mask [N, H, W] = argmax over the classes of nhwc(x), first maximum wins"""
        with weight_scope(self):
            return self.outc.argmax_nhwc(self.features_nhwc(x))

    def forward(self, x):
        return FF.to_nchw(self.nhwc(FF.to_nhwc(x)))
