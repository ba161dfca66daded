"""Host-side mirror of modules/psp/encoders/psp_encoders.py:13-152 (GradualStyleBlock, GradualStyleEncoder): IR-SE50
feature pyramid on source and reference, example-guided attention at 16^2 / 32^2, mask blend at 64^2, 14-18 map2style heads.
BackboneEncoderUsingLastLayerIntoW(Plus) are not the default encoder and are absent."""
from __future__ import annotations

import numpy as np
import torch
from torch import nn
from torch.nn import BatchNorm2d, Conv2d, Module, PReLU, Sequential

from .... import functional as FF
from ....weights import packed, weight_scope
from ...example_guided_att import ExampleGuidedAttention
from ...pluralistic_model.external_function import run_conv
from ..stylegan2.model import EqualLinear
from . import helpers
from .helpers import batch_norm, bottleneck_IR, bottleneck_IR_SE, get_blocks


class GradualStyleBlock(Module):
    def __init__(self, in_c, out_c, spatial):
        super().__init__()
        self.out_c = out_c
        self.spatial = spatial
        num_pools = int(np.log2(spatial))
        modules = [Conv2d(in_c, out_c, kernel_size=3, stride=2, padding=1), nn.LeakyReLU()]
        for _ in range(num_pools - 1):
            modules += [Conv2d(out_c, out_c, kernel_size=3, stride=2, padding=1), nn.LeakyReLU()]
        self.convs = nn.Sequential(*modules)
        self.linear = EqualLinear(out_c, out_c, lr_mul=1)

    def nhwc(self, x):
        with weight_scope(self):
            for m in self.convs:
                x = run_conv(m, x) if isinstance(m, Conv2d) else FF.leaky_relu(x, m.negative_slope)
            return self.linear(x.reshape(-1, self.out_c))

    def forward(self, x):
        return self.nhwc(FF.to_nhwc(x))


def _level_packs(heads, holder=None, key=None):
    """The operands of ``style_level_bf16`` for the heads of one level: per layer the stacked bf16 weights [G][K][9][C] (concatenated from
    the per-convolution packs, helpers._wnk) and fp32 biases [G][K], the EqualLinears as bf16(weight * scale) [G][K][1][C] and
    bias * lr_mul [G][K], and the LeakyReLU slope.  The caller holds weight_scope.  With ``holder`` (the encoder) they are kept under
    ``key`` while every source pack is the same object as when they were stacked -- helpers._wnk's rule: a frozen weight's pack lives
    while the weight is unchanged (weights.invalidate_packs forgets it), a trainable one is new every forward -- and no bias or linear
    weight is trainable or has changed (storage + version counter)."""
    depth = len(heads[0].convs) // 2
    layers = [[h.convs[2 * i] for h in heads] for i in range(depth)]
    src = [packed(c).wf for layer in layers for c in layer]
    small = [t for h in heads for t in ([c.bias for c in h.convs if isinstance(c, Conv2d)] + [h.linear.weight, h.linear.bias]) if t is not None]
    ver = None if any(t.requires_grad for t in small) else tuple((t.data_ptr(), t._version) for t in small)
    store = getattr(holder, "_fmi_head_packs", None) if holder is not None else None
    kept = store.get(key) if store is not None else None
    if kept is not None and ver is not None and kept[1] == ver and len(kept[0]) == len(src) and all(a is b for a, b in zip(kept[0], src)):
        return kept[2]
    with torch.no_grad():
        conv_w, conv_b = [], []
        for layer in layers:
            conv_w.append(torch.stack([helpers._wnk(c) for c in layer]))
            conv_b.append(torch.stack([c.bias.detach() for c in layer]).contiguous() if layer[0].bias is not None else None)
            for c in layer:  # the stacked copy is the one that is read from now on
                object.__setattr__(c, "_fmi_wnk", None)
        lin_w = torch.stack([(h.linear.weight.detach() * h.linear.scale).to(torch.bfloat16) for h in heads]).unsqueeze(2).contiguous()
        lin_b = torch.stack([h.linear.bias.detach() * h.linear.lr_mul for h in heads]).contiguous() if heads[0].linear.bias is not None else None
    ops = (conv_w, conv_b, lin_w, lin_b, float(heads[0].convs[1].negative_slope))
    if holder is not None:
        if store is None:
            store = {}
            object.__setattr__(holder, "_fmi_head_packs", store)
        store[key] = (src, ver, ops) if ver is not None else None
    return ops


def style_level_bf16(heads, p16, latents, first=0, holder=None):
    """The map2style heads of ONE pyramid level (psp_encoders.py:13-37 for each of them, the loops of :140-151) on the bf16 NHWC map
    ``p16``, one launch per layer for all of them: layer 1 on the shared map, every deeper layer on the stacked outputs, and the
    EqualLinears straight into slots first .. first + len(heads) - 1 of ``latents`` (fp32 [N, n_styles, K]).  Inference only; the caller
    holds weight_scope over the heads."""
    conv_w, conv_b, lin_w, lin_b, slope = _level_packs(heads, holder, (first, len(heads)))
    x = p16
    for i, (w, b) in enumerate(zip(conv_w, conv_b)):
        x = FF.conv2d_grouped_bf16(x, w, b, 3, 2, 1, slope=slope, shared=(i == 0))
    if x.shape[1] != 1 or x.shape[2] != 1:
        raise FF.FmiError(f"a level map of {tuple(p16.shape[1:3])} does not reduce to 1 x 1 in {len(conv_w)} stride-2 layers")
    return FF.conv2d_grouped_bf16(x, lin_w, lin_b, 1, 1, 0, shared=False, out=latents, first=first)


def neck_bf16(attention1, attention2, latlayer1, latlayer2, c1, c2, c3, r1=None, r2=None, r3=None, mask=None):
    """The neck of the pSp encoder (psp_encoders.py:126-147: mask resizes, guided attention or mask blend at the three levels, lateral
    1x1 convolutions, _upsample_add) on bf16 NHWC maps, inference only: c1 / c2 / c3 are the source taps ([N,64,64,128], [N,32,32,256],
    [N,16,16,512] at full widths), r1 / r2 / r3 the reference taps and ``mask`` the fp32 [N,H,W] soft mask -- all four None for a forward
    without a reference.  ``attention1`` / ``attention2`` (ExampleGuidedAttention with out_conv) work on c3 / c2; None: the plain blend
    there, as with use_attention off.  Returns the three bf16 level maps the heads read (coarse, middle, fine).  No fp32 activation map
    is written: 3 launches per attention, 1 per blend, 2 per lateral level.  The caller holds weight_scope over the modules and has
    refused grad mode."""
    if r3 is not None:
        m = mask.contiguous().unsqueeze(-1)  # [N,H,W,1]
        n = m.shape[0]
        mask_3 = FF.resize_bilinear(m, r3.shape[1], r3.shape[2]).view(n, r3.shape[1], r3.shape[2])
        mask_2 = FF.resize_bilinear(m, r2.shape[1], r2.shape[2]).view(n, r2.shape[1], r2.shape[2])
        mask_1 = FF.resize_bilinear(m, r1.shape[1], r1.shape[2]).view(n, r1.shape[1], r1.shape[2])
        c3 = attention1.nhwc(mask_3, c3, r3) if attention1 is not None else FF.mask_blend_bf16(mask_3, r3, c3)
        c2 = attention2.nhwc(mask_2, c2, r2) if attention2 is not None else FF.mask_blend_bf16(mask_2, r2, c2)
        c1 = FF.mask_blend_bf16(mask_1, r1, c1)

    def lateral(conv, x):
        return FF.conv2d_chan_bf16(x, helpers._wnk(conv), 1, 1, 1, 0, bias=None if conv.bias is None else conv.bias.detach())

    p2 = FF.fpn_merge_in_bf16(lateral(latlayer1, c2), c3)
    p1 = FF.fpn_merge_in_bf16(lateral(latlayer2, c1), p2)
    return c3, p2, p1


class GradualStyleEncoder(Module):
    def __init__(self, num_layers, mode="ir", opts=None, *, _widths=(64, 64, 128, 256, 512), _spatial=(16, 32, 64)):
        """``_widths`` (stem + the four stage depths) and ``_spatial`` (map sizes feeding the coarse / middle / fine heads)
        default to the reference's hard-coded IR-50 / 256x256 geometry; tests shrink them to keep fixtures small."""
        super().__init__()
        assert num_layers in [50, 100, 152], "num_layers should be 50,100, or 152"
        assert mode in ["ir", "ir_se"], "mode should be ir or ir_se"
        unit_module = bottleneck_IR if mode == "ir" else bottleneck_IR_SE
        w0, w1, w2, w3, w4 = _widths
        self.input_layer = Sequential(Conv2d(3, w0, (3, 3), 1, 1, bias=False), BatchNorm2d(w0), PReLU(w0))
        scale = {64: w1, 128: w2, 256: w3, 512: w4}
        self.body = Sequential(*[unit_module(w0 if i == 0 and j == 0 else scale[b.in_channel], scale[b.depth], b.stride)
                                 for i, block in enumerate(get_blocks(num_layers)) for j, b in enumerate(block)])
        self.styles = nn.ModuleList()
        self.style_count = opts.n_styles
        self.coarse_ind = 3
        self.middle_ind = 7
        for i in range(self.style_count):
            self.styles.append(GradualStyleBlock(w4, w4, _spatial[0] if i < self.coarse_ind else (_spatial[1] if i < self.middle_ind else _spatial[2])))
        self.latlayer1 = nn.Conv2d(w3, w4, kernel_size=1, stride=1, padding=0)
        self.latlayer2 = nn.Conv2d(w2, w4, kernel_size=1, stride=1, padding=0)
        # opts.encoder_dtype ("fp32" default / "bf16", this build's option like opts.decoder_dtype): the 24 IR-SE blocks keep bf16 NHWC
        # activations between the bf16 MFMA convolutions (fp32 accumulation, fp32 parameters / BatchNorm statistics / SE gates and all
        # parameter gradients); the C = 3 stem, the attention blocks, the FPN and the style heads stay fp32
        dt = getattr(opts, "encoder_dtype", "fp32")
        self.body_dtype = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp32": torch.float32, "float32": torch.float32}.get(dt, dt)
        # opts.encoder_eval_dtype ("fp32" default / "bf16"): the body of an EVAL-mode forward -- bf16 selects the inference form of the
        # blocks (helpers._Bottleneck.infer_bf16: BatchNorms folded, 4-5 launches per block, no backward).  Independent of
        # opts.encoder_dtype, which is the training body; parameters, running statistics and the state_dict are the same in every build
        edt = getattr(opts, "encoder_eval_dtype", "fp32")
        if edt not in ("fp32", "bf16"):
            raise FF.FmiError(f"encoder_eval_dtype must be 'fp32' or 'bf16', got {edt!r}")
        self.eval_body_dtype = torch.bfloat16 if edt == "bf16" else torch.float32
        # opts.style_heads_eval_dtype ("fp32" default / "bf16"): the map2style heads of an EVAL-mode forward -- bf16 runs the heads of a
        # pyramid level together on bf16 activations, one launch per layer (style_level_bf16; no backward).  Independent of the two
        # options above: the level maps arrive in fp32 either way, and the lateral convolutions and the attention blocks stay fp32
        sdt = getattr(opts, "style_heads_eval_dtype", "fp32")
        if sdt not in ("fp32", "bf16"):
            raise FF.FmiError(f"style_heads_eval_dtype must be 'fp32' or 'bf16', got {sdt!r}")
        self.eval_heads_dtype = torch.bfloat16 if sdt == "bf16" else torch.float32
        # opts.encoder_neck_eval_dtype ("fp32" default / "bf16"): the stem and the neck of an EVAL-mode forward -- bf16 runs the stem as one
        # launch that writes the body's two bf16 inputs, takes the body's bf16 outputs as the taps and keeps the attention blocks, the
        # blends, the lateral convolutions and the merges on bf16 maps (neck_bf16; no backward).  It consumes bf16 taps and produces bf16
        # level maps, so it needs both options above to be bf16: there is no mixed form
        ndt = getattr(opts, "encoder_neck_eval_dtype", "fp32")
        if ndt not in ("fp32", "bf16"):
            raise FF.FmiError(f"encoder_neck_eval_dtype must be 'fp32' or 'bf16', got {ndt!r}")
        if ndt == "bf16" and (edt != "bf16" or sdt != "bf16"):
            raise FF.FmiError("encoder_neck_eval_dtype='bf16' needs encoder_eval_dtype='bf16' and style_heads_eval_dtype='bf16' (got "
                              f"{edt!r} and {sdt!r}): the neck reads the body's bf16 taps and writes the heads' bf16 level maps")
        self.eval_neck_dtype = torch.bfloat16 if ndt == "bf16" else torch.float32
        self._widths = tuple(_widths)
        self.use_attention = opts.use_attention
        if opts.use_attention:
            self.attention1 = ExampleGuidedAttention(w4, out_channels=w4)
            self.attention2 = ExampleGuidedAttention(w3, out_channels=w3)

    def _pyramid(self, x):
        neck16 = self._neck_bf16()
        if not neck16:
            x = run_conv(self.input_layer[0], x)
            x = FF.prelu(batch_norm(self.input_layer[1], x), self.input_layer[2].weight)
        b16 = self.body_dtype == torch.bfloat16 and self.training
        infer16 = self._infer_bf16()
        if getattr(self, "_fmi_body_b16", None) != (b16 or infer16):  # the body's convolutions need no fp32 piece images while they run on bf16 activations
            for m in self.body.modules():
                if isinstance(m, nn.Conv2d):
                    object.__setattr__(m, "_fmi_no_w3", b16 or infer16)
            object.__setattr__(self, "_fmi_body_b16", b16 or infer16)
        if neck16:  # the stem in one launch; the tails of blocks 6, 20 and 23 write no fp32 copy: their bf16 y is the tap
            taps = {}
            stem = self.input_layer
            x, z = FF.irse_stem_fused_bf16(x, packed(stem[0]), *helpers.fold_bn_eval(stem[1]), stem[2].weight.detach(),
                                           *helpers.fold_bn_eval(self.body[0].res_layer[0]))
            for i, l in enumerate(self.body):
                nxt = self.body[i + 1].res_layer[0] if i + 1 < len(self.body) else None
                x, z, _ = l.infer_bf16(x, z, nxt, tap=False)
                if i in (6, 20, 23):
                    taps[i] = x
            return taps[6], taps[20], taps[23]
        if infer16:
            taps = {}
            x, z = FF.irse_stem_bf16(x, *helpers.fold_bn_eval(self.body[0].res_layer[0]))
            for i, l in enumerate(self.body):
                nxt = self.body[i + 1].res_layer[0] if i + 1 < len(self.body) else None
                x, z, t = l.infer_bf16(x, z, nxt, tap=i in (6, 20, 23))
                if t is not None:
                    taps[i] = t
            return taps[6], taps[20], taps[23]
        if b16:
            x = x.to(torch.bfloat16)
        taps = {}
        for i, l in enumerate(self.body):
            x = l.nhwc(x)
            if i in (6, 20, 23):
                taps[i] = x.float() if b16 else x
        return taps[6], taps[20], taps[23]  # [N,64,64,128], [N,32,32,256], [N,16,16,512]

    @staticmethod
    def _upsample_add(x, y):
        return FF.add(FF.resize_bilinear(x, y.shape[1], y.shape[2]), y)

    @staticmethod
    def _blend(m, r, c):
        """m*r + (1-m)*c with m [N,H,W] (psp_encoders.py:135-138)"""
        return FF.add(FF.mask_mul(r, m, False), FF.mask_mul(c, m, True))

    def _infer_bf16(self):
        return self.eval_body_dtype == torch.bfloat16 and not self.training

    def _heads_bf16(self):
        return self.eval_heads_dtype == torch.bfloat16 and not self.training

    def _neck_bf16(self):
        return self.eval_neck_dtype == torch.bfloat16 and not self.training

    def _latents_from_maps(self, maps):
        """the heads on the three bf16 level maps of neck_bf16 (coarse, middle, fine): log2(spatial) + 1 launches per level"""
        latents = torch.empty((maps[0].shape[0], self.style_count, maps[0].shape[3]), device=maps[0].device, dtype=torch.float32)
        bounds = [0, min(self.coarse_ind, self.style_count), min(self.middle_ind, self.style_count), self.style_count]
        for lvl, p16 in enumerate(maps):
            lo, hi = bounds[lvl], bounds[lvl + 1]
            if hi > lo:
                style_level_bf16([self.styles[j] for j in range(lo, hi)], p16, latents, lo, holder=self)
        return latents

    def _neck_check(self, x, ref):
        """the refusals of the bf16 stem and neck, before any device call; there is no fp32 detour"""
        if torch.is_grad_enabled():
            raise FF.FmiError("GradualStyleEncoder with encoder_neck_eval_dtype='bf16' is inference only (no backward): call it under "
                              "torch.no_grad() or detach the input")
        if any(w % 64 for w in self._widths):
            raise FF.FmiError(f"the bf16 stem and neck need every width to be a multiple of 64, got {self._widths}")
        if ref is not None and self.use_attention:
            h, w = x.shape[2], x.shape[3]
            for lvl in range(4):  # the body's four stride-2 stages; the attentions sit behind the third (32^2) and the fourth (16^2)
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
                if lvl >= 2 and (h * w) % 128:
                    raise FF.FmiError(f"the bf16 guided attention needs a token count that is a multiple of 128, got {h} x {w} = {h * w} "
                                      f"tokens at attention{4 - lvl} for a {x.shape[2]} x {x.shape[3]} image")
            for att in (self.attention1, self.attention2):
                unfit = att.bf16_unfit()
                if unfit:
                    raise FF.FmiError(f"the bf16 neck needs {unfit}")

    def _latents_bf16(self, c1, c2, c3):
        """FPN + heads of the bf16 inference form: three map hand-overs and log2(spatial) + 1 launches per level, written straight into
        the [N, n_styles, K] tensor (the fp32 form: psp_encoders.py:140-151, 2 depth + 1 launches per head and a torch.stack)"""
        latents = torch.empty((c3.shape[0], self.style_count, c3.shape[3]), device=c3.device, dtype=torch.float32)
        bounds = [0, min(self.coarse_ind, self.style_count), min(self.middle_ind, self.style_count), self.style_count]
        p = None
        for lvl, lateral in enumerate((None, self.latlayer1, self.latlayer2)):
            if lateral is None:
                p, p16 = c3, FF.fpn_merge_bf16(c3, None, want_f32=False)[1]
            else:
                p, p16 = FF.fpn_merge_bf16(run_conv(lateral, c2 if lvl == 1 else c1), p, want_f32=lvl == 1)
            lo, hi = bounds[lvl], bounds[lvl + 1]
            if hi > lo:
                style_level_bf16([self.styles[j] for j in range(lo, hi)], p16, latents, lo, holder=self)
        return latents

    def _latents(self, c1, c2, c3):
        """the head section: FPN merges + map2style heads from the three level maps (fp32 NHWC); the caller holds weight_scope"""
        if self._heads_bf16():
            return self._latents_bf16(c1, c2, c3)
        latents = [self.styles[j].nhwc(c3) for j in range(self.coarse_ind)]
        p2 = self._upsample_add(c3, run_conv(self.latlayer1, c2))
        latents += [self.styles[j].nhwc(p2) for j in range(self.coarse_ind, self.middle_ind)]
        p1 = self._upsample_add(p2, run_conv(self.latlayer2, c1))
        latents += [self.styles[j].nhwc(p1) for j in range(self.middle_ind, self.style_count)]
        return torch.stack(latents, dim=1)

    def forward(self, x, ref=None, mask=None):
        heads16 = self._heads_bf16()
        if heads16:  # refused before any device call, like the body's inference form
            if torch.is_grad_enabled():
                raise FF.FmiError("GradualStyleEncoder with style_heads_eval_dtype='bf16' is inference only (no backward): call it under "
                                  "torch.no_grad() or detach the input")
            if any(w % 64 for w in self._widths):
                raise FF.FmiError(f"the bf16 style heads need every width to be a multiple of 64, got {self._widths}")
        if getattr(self, "_fmi_heads_b16", None) != heads16:  # the heads' convolutions need no fp32 piece images while they run on bf16 activations
            for h in self.styles:
                for m in h.convs:
                    if isinstance(m, nn.Conv2d):
                        object.__setattr__(m, "_fmi_no_w3", heads16)
            object.__setattr__(self, "_fmi_heads_b16", heads16)
        neck16 = self._neck_bf16()
        if neck16:
            self._neck_check(x, ref)
        if getattr(self, "_fmi_neck_b16", None) != neck16:  # the stem's, the attentions' and the lateral convolutions need no fp32 piece images either
            convs = [self.input_layer[0], self.latlayer1, self.latlayer2]
            if self.use_attention:
                convs += [self.attention1.conv, self.attention1.out_conv, self.attention2.conv, self.attention2.out_conv]
            for m in convs:
                object.__setattr__(m, "_fmi_no_w3", neck16)
            object.__setattr__(self, "_fmi_neck_b16", neck16)
        if self._infer_bf16():  # refused before any device call; there is no fp32 detour
            if torch.is_grad_enabled():
                raise FF.FmiError("GradualStyleEncoder with encoder_eval_dtype='bf16' is inference only (no backward): call it under "
                                  "torch.no_grad() or detach the input")
            if any(w % 64 for w in self._widths):
                raise FF.FmiError(f"the bf16 inference body needs every width to be a multiple of 64, got {self._widths}")
        with weight_scope(self):
            if ref is not None:
                assert mask is not None, "ref and mask should both be provided"
                # psp_encoders.py:101-125 runs input_layer + body on x and then AGAIN on ref (shared weights).  Here both go through
                # as ONE batch of 2N -- every convolution launch has twice the rows (the 256-channel 32^2 stage is 256 tiles = one
                # workgroup per CU at N = 16) and half the launches -- while training-mode BatchNorm keeps per-part statistics and
                # updates its running buffers part by part (helpers.BN_GROUPS), so every value equals the two-pass form
                nb = x.shape[0]
                helpers.BN_GROUPS[0] = 2
                try:
                    t1, t2, t3 = self._pyramid(torch.cat([FF.to_nhwc(x), FF.to_nhwc(ref)], dim=0))
                finally:
                    helpers.BN_GROUPS[0] = 1
                if neck16:
                    (c1, r1), (c2, r2), (c3, r3) = ((t[:nb], t[nb:]) for t in (t1, t2, t3))
                    att1, att2 = (self.attention1, self.attention2) if self.use_attention else (None, None)
                    return self._latents_from_maps(neck_bf16(att1, att2, self.latlayer1, self.latlayer2, c1, c2, c3, r1, r2, r3, mask))
                (c1, r1), (c2, r2), (c3, r3) = FF.split_batch(t1, nb), FF.split_batch(t2, nb), FF.split_batch(t3, nb)
                m = mask.contiguous().unsqueeze(-1)  # [N,H,W,1]
                n = m.shape[0]
                mask_3 = FF.resize_bilinear(m, r3.shape[1], r3.shape[2]).view(n, r3.shape[1], r3.shape[2])
                mask_2 = FF.resize_bilinear(m, r2.shape[1], r2.shape[2]).view(n, r2.shape[1], r2.shape[2])
                mask_1 = FF.resize_bilinear(m, r1.shape[1], r1.shape[2]).view(n, r1.shape[1], r1.shape[2])
                if self.use_attention:
                    c3 = self.attention1.nhwc(mask_3, c3, r3)
                    c2 = self.attention2.nhwc(mask_2, c2, r2)
                else:
                    c3 = self._blend(mask_3, r3, c3)
                    c2 = self._blend(mask_2, r2, c2)
                c1 = self._blend(mask_1, r1, c1)
            else:
                c1, c2, c3 = self._pyramid(FF.to_nhwc(x))
                if neck16:
                    return self._latents_from_maps(neck_bf16(None, None, self.latlayer1, self.latlayer2, c1, c2, c3))
            return self._latents(c1, c2, c3)
