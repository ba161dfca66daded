"""Host-side mirror of modules/example_guided_att.py (example_guided_att.py:5-41): same constructor, parameter
names (``conv.weight``, ``out_conv.weight/bias``) and forward(src_mask, src_feature, ref_feature).  The
[N, HW, HW] attention map is produced chunk-wise inside the Infinity Cache and applied to BOTH value maps from
one softmax pass; the mask blend and the channel concat are one kernel."""
from __future__ import annotations

import torch
from torch import nn

from .. import functional as FF
from ..weights import packed, weight_scope
from .pluralistic_model.external_function import run_conv


class ExampleGuidedAttention(nn.Module):
    def __init__(self, in_channels, out_channels=None):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, in_channels // 4, 1, bias=False)
        self.out_channels = out_channels
        if out_channels is not None:
            self.out_conv = nn.Conv2d(in_channels * 2, out_channels, 1)

    def bf16_unfit(self, shapes=None):
        """why the bf16 form cannot run this module (None: it can); ``shapes``: a caller's narrower set of (img_f // 4, img_f)"""
        c = self.conv.in_channels
        shapes = FF.GUIDED_ATTENTION_BF16_SHAPES if shapes is None else shapes
        if (c // 4, c) not in shapes:
            return f"(img_f // 4, img_f) in {set(shapes)} at the guided attention (got ({c // 4}, {c}))"
        if self.out_channels is not None and self.out_channels % 64:
            return f"an out_conv whose width is a multiple of 64 (got {self.out_channels})"
        return None

    def _nhwc_bf16(self, mask_nhw, src, ref):
        """inference on bf16 feature maps, two launches: the query convolution, then both attentions from one softmax with the mask blend
        in the epilogue (fmi_guided_attention_fwd_bf16, at the pSp widths fmi_guided_attention_sliced_fwd_bf16); the result is bf16 [N,H,W,2C] -- or, with out_conv, a third launch (the 1x1
        convolution with its bias on fmi_conv2d_fwd_chan_bf16) and bf16 [N,H,W,out_channels]"""
        n, h, w, c = src.shape
        unfit = self.bf16_unfit()
        if unfit or ref.dtype != torch.bfloat16 or (h * w) % 128:
            raise FF.FmiError(f"the bf16 guided attention needs {unfit or 'bf16 src and ref maps with a token count that is a multiple of 128'}"
                              f" (got {h} x {w} = {h * w} tokens); these run in fp32 only")
        q = FF.conv2d_plain_bf16(src, packed(self.conv), 0)
        out = FF.guided_attention_bf16(q.view(n, h * w, -1), src.view(n, h * w, c), ref.view(n, h * w, c), mask_nhw.contiguous().view(n, h * w))
        out = out.view(n, h, w, 2 * c)
        if self.out_channels is not None:
            out = FF.conv2d_chan_bf16(out, FF._wnk_of(packed(self.out_conv)), 1, 1, 1, 0, bias=self.out_conv.bias.detach())
        return out

    def nhwc(self, mask_nhw, src, ref):
        """mask [N,H,W] (soft), src / ref [N,H,W,C] -> [N,H,W,2C] (or out_channels)."""
        with weight_scope(self):
            n, h, w, c = src.shape
            if src.dtype == torch.bfloat16:
                return self._nhwc_bf16(mask_nhw, src, ref)
            q = run_conv(self.conv, src)
            src_att, ref_att = FF.self_attention(q.view(n, h * w, -1), [src.view(n, h * w, c), ref.view(n, h * w, c)])
            out = FF.guide_blend_cat(ref_att.view(n, h, w, c), ref, src_att.view(n, h, w, c), mask_nhw)
            if self.out_channels is not None:
                out = run_conv(self.out_conv, out)
            return out

    def forward(self, src_mask, src_feature, ref_feature):
        """src_mask [N,1,H,W]; src_feature, ref_feature [N,C,H,W] -> [N, 2C | out_channels, H, W]"""
        m = src_mask.reshape(src_mask.shape[0], src_mask.shape[2], src_mask.shape[3]).contiguous()
        return FF.to_nchw(self.nhwc(m, FF.to_nhwc(src_feature), FF.to_nhwc(ref_feature)))
