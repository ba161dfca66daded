"""Host-side mirror of modules/loss.py: VGGLoss (loss.py:16-65), GANOptimizer (loss.py:68-144) and the UNet losses dice_coeff /
multiclass_dice_coeff / dice_loss (loss.py:148-186) with the reference's signatures and return values.  The dice_* helpers are the
general form (any two equal-shaped fp32 device tensors, values only): the sums come from one kernel (FF.plane_sums) and the rest is
[planes]-sized bookkeeping on the device.  The mask-detector trainer does not go through them: its objective and its gradient are
FF.seg_ce_dice_loss, its validation metric FF.seg_dice_score.
"""
from __future__ import annotations

import os

import torch
from torch import nn

from .. import functional as FF
from ..weights import packed
from .pluralistic_model import base_function
from .pluralistic_model.external_function import GANLoss, run_conv

VGG_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M"]  # vgg16.features[:23] has no 5th stage


VGG_DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def vgg_dtype_from_env():
    """FMI_VGG_DTYPE={fp32,bf16} (default fp32): the dtype of VGGLoss's feature trunk where it is built without the argument -- how pSpLoss,
    a trainer whose flags are the reference's, or a fixed benchmark selects the bf16 trunk"""
    name = os.environ.get("FMI_VGG_DTYPE", "fp32")
    if name not in VGG_DTYPES:
        raise FF.FmiError(f"FMI_VGG_DTYPE must be one of {sorted(VGG_DTYPES)}, got {name!r}")
    return VGG_DTYPES[name]


def _vgg16_features(width_div: int = 1) -> nn.Sequential:
    """Architecture of torchvision.models.vgg16().features[:24] (cfg 'D'); used when torchvision is absent.
    Weights are then random (no network access for the ImageNet checkpoint): SURVEY.md section 8c."""
    layers, c_in = [], 3
    for v in VGG_CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(c_in, v // width_div, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            c_in = v // width_div
    return nn.Sequential(*layers)


class VGGLoss(torch.nn.Module):
    def __init__(self, width_div: int = 1, feature_dtype=None):
        """feature_dtype=torch.bfloat16 (this build's extra, TRAINABLE THROUGH): the trunk between the image and the four tapped feature
        maps on the bf16 kernels, forward and input-gradient chain (FF.vgg_trunk_bf16); the parameters, the taps the loss kernels read and
        the image gradient stay fp32.  Needs width_div = 1 and an input whose H and W are multiples of 8.  None (the default) reads
        FMI_VGG_DTYPE, which defaults to fp32."""
        super().__init__()
        if feature_dtype is None:
            feature_dtype = vgg_dtype_from_env()
        if feature_dtype not in (torch.float32, torch.bfloat16):
            raise FF.FmiError(f"feature_dtype must be torch.float32 or torch.bfloat16, got {feature_dtype}")
        self.feature_dtype = feature_dtype
        try:  # the reference's source of weights (loss.py:21)
            import torchvision  # type: ignore

            features = torchvision.models.vgg16(pretrained=True).features
        except Exception:
            features = _vgg16_features(width_div)
        blocks = [features[:4].eval(), features[4:9].eval(), features[9:16].eval(), features[16:23].eval()]
        for bl in blocks:
            for p in bl.parameters():
                p.requires_grad = False
        self.blocks = torch.nn.ModuleList(blocks)
        if feature_dtype == torch.bfloat16:
            FF.vgg_trunk_check_widths([(m.in_channels, m.out_channels) + tuple(m.kernel_size) for bl in blocks for m in bl if isinstance(m, nn.Conv2d)])
        self.register_buffer("mean", torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
        self.register_buffer("std", torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))
        self._cache = {}

    def _prepare(self):
        """frozen weights: pack once, re-pack when a weight tensor is replaced or modified in place"""
        convs = [m for bl in self.blocks for m in bl if isinstance(m, nn.Conv2d)]
        key = tuple((c.weight.data_ptr(), c.weight._version) for c in convs)
        if self._cache.get("key") != key:
            with torch.no_grad():
                pws = FF.prepare_weights([(c.weight, None, None) for c in convs])
                # the bf16 trunk's packs live and die with the fp32 packs they are cut from: no pack launch per call
                packs16 = FF.vgg_trunk_packs(pws, [c.bias for c in convs]) if self.feature_dtype == torch.bfloat16 else None
            self._cache = {"key": key, "pws": pws, "packs16": packs16}
        for c, pw in zip(convs, self._cache["pws"]):
            object.__setattr__(c, "_fmi_packed", pw)

    def _block(self, bi, x):
        mods = [m for m in self.blocks[bi] if isinstance(m, (nn.MaxPool2d, nn.Conv2d))]
        prev_conv = False
        for i, m in enumerate(mods):
            if isinstance(m, nn.MaxPool2d):
                x = FF.max_pool2(x)
                prev_conv = False
            else:
                # ReLU fused into the GEMM epilogue.  Between two convolutions of a block the ReLU's backward runs in the NEXT
                # convolution's adjoint epilogue (its input is this ReLU's output and it is the only consumer), not as a pass of its own
                next_conv = i + 1 < len(mods) and isinstance(mods[i + 1], nn.Conv2d)
                x = run_conv(m, x, act=FF.ACT_RELU, in_act=("mask", 0.0) if prev_conv else None, skip_act_bwd=next_conv)
                prev_conv = True
        return x

    def _taps16(self, x, y, nslice=1):
        """the one-node trunks: (taps of x with gradient, taps of y without), four fp32 NHWC maps each -- the bf16 trunk, or the fp32 trunk
        (FF.vgg_trunk_f32; with nslice > 1 every tap of x is a tuple of nslice batch slices) -- or (None, None) where the fp32 tap passes
        refuse the widths and the composed ``_block`` runs"""
        blocks = tuple(sum(isinstance(m, nn.Conv2d) for m in bl) for bl in self.blocks)
        if self.feature_dtype != torch.bfloat16:
            convs = [m for bl in self.blocks for m in bl if isinstance(m, nn.Conv2d)]
            pws = self._cache["pws"]
            if not (x.is_cuda and x.dtype == torch.float32 and FF.vgg_trunk_f32_ok(pws, blocks)) or x.shape[0] % nslice or nslice > 4:
                return None, None
            return FF.vgg_trunk_f32(x, y, [(pw, c.bias) for pw, c in zip(pws, convs)], blocks, nslice=nslice)
        xt = FF.vgg_trunk_bf16(x, self._cache["packs16"], blocks)
        with torch.no_grad():
            yt = FF.vgg_trunk_bf16(y, self._cache["packs16"], blocks)
        return xt, yt

    @staticmethod
    def _input_extent(h, w):
        return (224, 224) if w > 224 else (h, w)  # loss.py:48-49 "Filter HQ"

    def _check16(self, h, w):
        """the bf16 trunk's refusal of a VGG input extent, before any device call of the forward that asks"""
        if self.feature_dtype == torch.bfloat16:
            FF.vgg_trunk_check_extent(h, w)

    def _input(self, img):
        x = FF.to_nhwc(img)
        n, h, w, c = x.shape
        oh, ow = self._input_extent(h, w)
        return FF.resize_bilinear(x, oh, ow, self.mean.view(3).contiguous(), self.std.view(3).contiguous())

    def forward(self, input, target, lossType="perceptual"):
        self._check16(*self._input_extent(input.shape[2], input.shape[3]))
        self._prepare()
        x = self._input(input)
        with torch.no_grad():
            y = self._input(target)
        loss = 0.0
        xt, yt = self._taps16(x, y)
        for i in range(len(self.blocks)):
            if xt is not None:
                x, y = xt[i], yt[i]
            else:
                x = self._block(i, x)
                with torch.no_grad():
                    y = self._block(i, y)
            n, h, w, c = x.shape
            dim = c * h * w
            if lossType == "perceptual":
                loss = loss + FF.l1_loss(x, y) / dim
            elif lossType == "style":
                gx = FF.gram_matrix(x.view(n, h * w, c))
                gy = FF.gram_matrix(y.view(n, h * w, c))
                loss = loss + FF.l1_loss(gx, gy) / (c * c * dim)
            elif lossType == "contextual" and i == 3:
                loss = loss + FF.contextual_loss(x.view(n, h * w, c), y.view(n, h * w, c)) / dim
        return loss


    def forward_multi(self, triples):
        """[(input, target, lossType), ...] -> [loss, ...], identical values to calling ``forward`` per triple, but the
        inputs share ONE VGG pass with gradient (batch k*N) and the targets ONE pass without (the three losses of
        GANOptimizer are 6 VGG passes of batch N in the reference, loss.py:84-95): larger GEMM M fills the GPU at the
        28x28 / 56x56 layers, and the launch count drops 3x."""
        for t in triples:
            self._check16(*self._input_extent(t[0].shape[2], t[0].shape[3]))
        x = torch.cat([self._input(t[0]) for t in triples], 0)
        with torch.no_grad():
            y = torch.cat([self._input(t[1]) for t in triples], 0)
        return self.forward_multi_prepared(x, y, [t[2] for t in triples])

    def forward_multi_prepared(self, x, y, loss_types):
        """``forward_multi`` from its block loop onward: x, y [k*N, H, W, 3] NHWC are the resized and normalised operands of the k
        losses stacked along the batch (what ``forward_multi`` builds, or FF.gan_image_head in one pass); y carries no gradient"""
        self._check16(x.shape[1], x.shape[2])
        self._prepare()
        k = len(loss_types)
        n = x.shape[0] // k
        losses = [0.0] * k
        xt, yt = self._taps16(x, y, nslice=k)
        sliced = xt is not None and k > 1 and isinstance(xt[0], tuple)  # the fp32 trunk hands out the k slices of a tap themselves
        for i in range(len(self.blocks)):
            if xt is not None:
                x, y = xt[i], yt[i]
            else:
                x = self._block(i, x)
                with torch.no_grad():
                    y = self._block(i, y)
            # contiguous batch slices; the backward of split is one cat, the fp32 trunk's slices go back as they are
            xparts, yparts = x if sliced else x.split(n, 0), y.split(n, 0)
            _, h, w, c = y.shape
            dim = c * h * w
            for j, lossType in enumerate(loss_types):
                xs, ys = xparts[j], yparts[j]
                if lossType == "perceptual":
                    losses[j] = losses[j] + FF.l1_loss(xs, ys) / dim
                elif lossType == "style":
                    gx = FF.gram_matrix(xs.reshape(n, h * w, c))
                    gy = FF.gram_matrix(ys.reshape(n, h * w, c))
                    losses[j] = losses[j] + FF.l1_loss(gx, gy) / (c * c * dim)
                elif lossType == "contextual" and i == 3:
                    losses[j] = losses[j] + FF.contextual_loss(xs.reshape(n, h * w, c), ys.reshape(n, h * w, c)) / dim
        return losses


class GANOptimizer(nn.Module):
    """loss.py:68-144.  ``__call__`` performs the generator step then the discriminator step and returns
    (D_loss, G_loss, perc_loss, style_loss, cx_loss) exactly like the reference."""

    def __init__(self, optimizer_D, optimizer_G, lambda_g=0.01, debug=False, vgg_width_div: int = 1, vgg_dtype=None):
        super().__init__()
        self.gan_loss = GANLoss("lsgan")
        self.vgg_loss = VGGLoss(vgg_width_div, feature_dtype=vgg_dtype)  # vgg_dtype None: FMI_VGG_DTYPE (VGGLoss)
        self.debug = debug
        self.optimizer_D = optimizer_D
        self.optimizer_G = optimizer_G
        self.lambda_perc = 0.1
        self.lambda_style = 250
        self.lambda_cx = 1
        self.lambda_g = lambda_g
        self.early_d = None  # None: automatic (on when the optimisers are DataParallelOptimizer); True / False force it
        self.fused_head = False  # True: the VGG operands and the L1 term come from FF.gan_image_head (one pass) instead of composed ops

    LOSS_TYPES = ("perceptual", "style", "contextual")  # the row blocks of FF.gan_image_head's x_in / y_in

    @staticmethod
    def _masked(img, mask, invert):
        return FF.to_nchw(FF.mask_mul(FF.to_nhwc(img), mask.contiguous(), invert))

    def perceptual_loss(self, gt_img, gen_img):
        return self.vgg_loss(gen_img, gt_img, lossType="perceptual")

    def style_loss(self, gen_img, src_img, src_mask):
        return self.vgg_loss(self._masked(gen_img, src_mask, True), src_img, lossType="style")  # "Yes inverse"

    def contextual_loss(self, gen_img, ref_img, src_mask):
        return self.vgg_loss(self._masked(gen_img, src_mask, False), self._masked(ref_img, src_mask, False), lossType="contextual")

    def discriminator_loss(self, netD, real, fake):
        D_real_loss = self.gan_loss(netD(real), True, True)
        D_fake_loss = self.gan_loss(netD(fake.detach()), False, True)
        return (D_real_loss + D_fake_loss) * 0.5

    def generator_loss(self, netD, real, fake, freeze=True, l1=None):
        """``l1``: the L1 term already computed (FF.gan_image_head) instead of FF.l1_loss here"""
        if freeze:
            base_function._freeze(netD)
        D_fake = netD(fake)
        loss_ad_g = self.gan_loss(D_fake, True, False) * self.lambda_g
        loss_l1_g = FF.l1_loss(FF.to_nhwc(fake), FF.to_nhwc(real)) if l1 is None else l1
        return loss_ad_g + loss_l1_g

    def _head(self, src_img, gt_img, ref_img, gen_img, src_mask):
        """(x_in, y_in, l1) of the three VGG losses and the L1 term in one pass over the images (csrc/ganhead.hip)"""
        return FF.gan_image_head(gen_img, gt_img, src_img, ref_img, src_mask, self.vgg_loss.mean, self.vgg_loss.std)

    def __call__(self, discriminator, src_img, gt_img, ref_img, gen_img, src_mask):
        # The reference leaves D trainable here (freeze=False) and then discards the D gradients this backward
        # produces (optimizer_D.zero_grad() at loss.py:130).  They are not computed at all: D's parameters are
        # switched to requires_grad=False for the generator pass only -- same values everywhere, less work.
        d_params = [p for p in discriminator.parameters() if p.requires_grad]
        for p in d_params:
            p.requires_grad_(False)
        head = self._head(src_img, gt_img, ref_img, gen_img, src_mask) if self.fused_head else None
        try:
            if head is None:
                G_loss = self.generator_loss(discriminator, gt_img, gen_img, freeze=False)
            else:
                G_loss = self.generator_loss(discriminator, gt_img, gen_img, freeze=False, l1=head[2])
        finally:
            for p in d_params:
                p.requires_grad_(True)
        if head is not None:
            perc, sty, cx = self.vgg_loss.forward_multi_prepared(head[0], head[1], self.LOSS_TYPES)
        else:
            perc, sty, cx = self.vgg_loss.forward_multi([
                (gen_img, gt_img, "perceptual"),                                                     # loss.py:84-85
                (self._masked(gen_img, src_mask, True), src_img, "style"),                           # loss.py:87-89 "Yes inverse"
                (self._masked(gen_img, src_mask, False), self._masked(ref_img, src_mask, False), "contextual")])  # loss.py:91-95
        perc_loss, style_loss, cx_loss = perc * self.lambda_perc, sty * self.lambda_style, cx * self.lambda_cx
        G_loss = G_loss + perc_loss + style_loss + cx_loss
        early_d = self.early_d if self.early_d is not None else hasattr(self.optimizer_D, "launch")
        if early_d:
            # Data-parallel schedule: the discriminator loss depends only on gen_img and on the pre-update D
            # weights, so its forward (same D call order gen -> gt -> gen.detach(), hence the same SpectralNorm u/v
            # sequence) and backward run BEFORE the generator backward; the D gradients then travel over xGMI while the
            # VGG dgrad at the head of G_loss.backward() runs, and the G buckets follow as the decoder/encoder gradients
            # complete.  Every tensor has the value it has in the reference order (loss.py:120-134).
            D_loss = self.discriminator_loss(discriminator, gt_img, gen_img)
            self.optimizer_D.zero_grad()
            D_loss.backward()
            launch = getattr(self.optimizer_D, "launch", None)
            if launch is not None:
                launch()
            self.optimizer_G.zero_grad()
            G_loss.backward()
            self.optimizer_G.step()
            self.optimizer_D.step()
            return D_loss, G_loss, perc_loss, style_loss, cx_loss
        self.optimizer_G.zero_grad()
        G_loss.backward()
        self.optimizer_G.step()
        D_loss = self.discriminator_loss(discriminator, gt_img, gen_img)
        self.optimizer_D.zero_grad()
        D_loss.backward()
        self.optimizer_D.step()
        return D_loss, G_loss, perc_loss, style_loss, cx_loss

    def calc_loss(self, discriminator, src_img, gt_img, ref_img, gen_img, src_mask):
        D_loss = self.discriminator_loss(discriminator, gt_img, gen_img)
        if self.fused_head:
            x_in, y_in, l1 = self._head(src_img, gt_img, ref_img, gen_img, src_mask)
            G_loss = self.generator_loss(discriminator, gt_img, gen_img, freeze=False, l1=l1)
            perc, sty, cx = self.vgg_loss.forward_multi_prepared(x_in, y_in, self.LOSS_TYPES)
            return D_loss, G_loss + perc * self.lambda_perc + sty * self.lambda_style + cx * self.lambda_cx
        G_loss = self.generator_loss(discriminator, gt_img, gen_img, freeze=False)
        perc_loss = self.perceptual_loss(gt_img, gen_img) * self.lambda_perc
        style_loss = self.style_loss(gen_img, src_img, src_mask) * self.lambda_style
        cx_loss = self.contextual_loss(gen_img, ref_img, src_mask) * self.lambda_cx
        return D_loss, G_loss + perc_loss + style_loss + cx_loss


######################## Unet Losses #########################################
def _dice_from_sums(sums, epsilon):
    """[..., 3] fp64 (inter, sum input, sum target) -> dice_coeff's value per entry (loss.py:157-162); the `sets_sum == 0` branch is a
    torch.where on the device instead of the reference's .item()"""
    inter, sets_sum = sums[..., 0], sums[..., 1] + sums[..., 2]
    sets_sum = torch.where(sets_sum == 0, 2 * inter, sets_sum)
    return (2 * inter + epsilon) / (sets_sum + epsilon)


def dice_coeff(input, target, reduce_batch_first=False, epsilon=1e-6):
    """Average of Dice coefficient for all batches, or for a single mask (loss.py:148-168) -> 0-dim fp32 device tensor"""
    assert input.size() == target.size()
    if input.dim() == 2 and reduce_batch_first:
        raise ValueError(f'Dice: asked to reduce batch but got tensor without batch dimension (shape {input.shape})')
    if input.dim() == 2 or reduce_batch_first:
        return _dice_from_sums(FF.plane_sums(input, target, 1)[0], epsilon).float()
    # the reference recurses over the leading dimensions down to single [H, W] masks and calls itself there with the DEFAULT epsilon
    # (loss.py:167); nested means over equal-sized groups are the mean over all masks
    planes = input.numel() // (input.shape[-1] * input.shape[-2])
    return _dice_from_sums(FF.plane_sums(input, target, planes), 1e-6).mean().float()


def multiclass_dice_coeff(input, target, reduce_batch_first=False, epsilon=1e-6):
    """Average of Dice coefficient for all classes (loss.py:171-179): dice_coeff(input[:, c], target[:, c], ...) averaged over c, for
    input / target [N, C, ...] of any rank the reference's recursion takes"""
    assert input.size() == target.size()
    n, c = input.shape[0], input.shape[1]
    if input.dim() == 3 or reduce_batch_first:
        if input.dim() == 3 and reduce_batch_first:  # input[:, c] is 2-D: a single mask without a batch dimension (loss.py:151-154)
            raise ValueError(f'Dice: asked to reduce batch but got tensor without batch dimension (shape {input[:, 0].shape})')
        sums = FF.plane_sums(input, target, n * c).view(n, c, 3).sum(0)  # one mask per class over everything else
        return _dice_from_sums(sums, epsilon).mean().float()
    # per class the mean over single [H, W] masks with the default epsilon (loss.py:164-168); equal-sized groups: the mean over all
    planes = input.numel() // (input.shape[-1] * input.shape[-2])
    return _dice_from_sums(FF.plane_sums(input, target, planes), 1e-6).mean().float()


def dice_loss(input, target, multiclass=False):
    """Dice loss (objective to minimize) between 0 and 1 (loss.py:182-186)"""
    assert input.size() == target.size()
    fn = multiclass_dice_coeff if multiclass else dice_coeff
    return 1 - fn(input, target, reduce_batch_first=True)
