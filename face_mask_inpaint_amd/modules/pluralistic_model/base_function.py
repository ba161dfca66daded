"""Host-side mirror of modules/pluralistic_model/base_function.py (hot-path subset): same class names,
constructor arguments, sub-module names and therefore ``state_dict`` keys (``conv1.module.weight_bar``,
``model.N.module.*`` aliases, ``shortcut.0.module.*`` ...), with every forward running on the HIP kernels.

Public ``forward`` methods take / return NCHW-shaped tensors like the reference; internally activations are NHWC
contiguous (``nhwc`` methods), so chained blocks never transpose.  CoordConv / AddCoords, get_scheduler,
print_network and the DataParallel branch of init_net are not on the hot path and are absent.
"""
from __future__ import annotations

import functools

import torch
import torch.nn as nn
from torch.nn import init

from ... import functional as FF
from ...weights import packed, weight_scope
from .external_function import SpectralNorm, run_conv


# ----------------------------------------------------------------------------------------------
# init / factories (base_function.py:14-146)
# ----------------------------------------------------------------------------------------------
def init_weights(net, init_type="normal", gain=0.02):
    """Same rule as the reference: only modules that (still) own a ``weight`` and whose class name contains
    Conv / Linear are re-initialised -- SpectralNorm-wrapped convs lost ``weight`` and keep the default init."""

    def init_func(m):
        classname = m.__class__.__name__
        if hasattr(m, "weight") and (classname.find("Conv") != -1 or classname.find("Linear") != -1):
            if init_type == "normal":
                init.normal_(m.weight.data, 0.0, gain)
            elif init_type == "xavier":
                init.xavier_normal_(m.weight.data, gain=gain)
            elif init_type == "kaiming":
                init.kaiming_normal_(m.weight.data, a=0, mode="fan_in")
            elif init_type == "orthogonal":
                init.orthogonal_(m.weight.data, gain=gain)
            else:
                raise NotImplementedError("initialization method [%s] is not implemented" % init_type)
            if hasattr(m, "bias") and m.bias is not None:
                init.constant_(m.bias.data, 0.0)
        elif classname.find("BatchNorm2d") != -1:
            init.normal_(m.weight.data, 1.0, 0.02)
            init.constant_(m.bias.data, 0.0)

    net.apply(init_func)


def get_norm_layer(norm_type="batch"):
    if norm_type == "instance":
        return functools.partial(nn.InstanceNorm2d, affine=True)
    if norm_type == "none":
        return None
    if norm_type == "batch":
        raise NotImplementedError("BatchNorm2d is not on the PICNet hot path (encoder norm=none, decoder norm=instance)")
    raise NotImplementedError("normalization layer [%s] is not found" % norm_type)


def get_nonlinearity_layer(activation_type="PReLU"):
    if activation_type == "ReLU":
        return nn.ReLU()
    if activation_type == "LeakyReLU":
        return nn.LeakyReLU(0.1)
    raise NotImplementedError("activation layer [%s] is not on the hot path" % activation_type)


def init_net(net, init_type="normal", activation="relu", gpu_ids=[]):
    if len(gpu_ids) > 0:
        raise NotImplementedError("multi-GPU runs use one process per GPU (face_mask_inpaint_amd.distributed), not nn.DataParallel")
    init_weights(net, init_type)
    return net


def _freeze(*args):
    for module in args:
        if module:
            for p in module.parameters():
                p.requires_grad = False


def _unfreeze(*args):
    for module in args:
        if module:
            for p in module.parameters():
                p.requires_grad = True


def spectral_norm(module, use_spect=True):
    return SpectralNorm(module) if use_spect else module


def coord_conv(input_nc, output_nc, use_spect=False, use_coord=False, with_r=False, **kwargs):
    if use_coord:
        raise NotImplementedError("CoordConv is dead code in the reference's hot path")
    return spectral_norm(nn.Conv2d(input_nc, output_nc, **kwargs), use_spect)


def _slope(nonlinearity) -> float:
    if isinstance(nonlinearity, nn.LeakyReLU):
        return float(nonlinearity.negative_slope)
    if isinstance(nonlinearity, nn.ReLU):
        return 0.0
    raise NotImplementedError(type(nonlinearity))


def _conv(m):
    """the nn.Conv2d / nn.ConvTranspose2d parameter holder behind an (optionally) spectral-normed layer"""
    return m.module if isinstance(m, SpectralNorm) else m


def _norm_act(norm: nn.Module, x, slope, passthrough=False):
    if not isinstance(norm, nn.InstanceNorm2d) or not norm.affine or norm.track_running_stats:
        raise NotImplementedError("only InstanceNorm2d(affine=True) is on the hot path")
    return FF.instance_norm_act(x, norm.weight, norm.bias, norm.eps, slope, passthrough)


def _norm_act_bf16(norm: nn.Module, x, slope):
    if not isinstance(norm, nn.InstanceNorm2d) or not norm.affine or norm.track_running_stats:
        raise NotImplementedError("only InstanceNorm2d(affine=True) is on the hot path")
    return FF.instance_norm_act_bf16(x, norm.weight, norm.bias, norm.eps, slope)


class _NhwcBlock(nn.Module):
    """public forward = NCHW-shaped tensors, like the reference; ``nhwc`` = channels-last fast path"""

    def forward(self, x):
        return FF.to_nchw(self.nhwc(FF.to_nhwc(x)))


# ----------------------------------------------------------------------------------------------
# blocks (base_function.py:207-398)
# ----------------------------------------------------------------------------------------------
class ResBlock(_NhwcBlock):
    def __init__(self, input_nc, output_nc, hidden_nc=None, norm_layer=nn.BatchNorm2d, nonlinearity=nn.LeakyReLU(),
                 sample_type="none", use_spect=False, use_coord=False):
        super().__init__()
        hidden_nc = output_nc if hidden_nc is None else hidden_nc
        self.sample = sample_type != "none"
        if sample_type == "down":
            self.pool = nn.AvgPool2d(kernel_size=2, stride=2)
        elif sample_type != "none":
            raise NotImplementedError("sample type [%s] is not on the hot path" % sample_type)
        self.conv1 = coord_conv(input_nc, hidden_nc, use_spect, use_coord, kernel_size=3, stride=1, padding=1)
        self.conv2 = coord_conv(hidden_nc, output_nc, use_spect, use_coord, kernel_size=3, stride=1, padding=1)
        self.bypass = coord_conv(input_nc, output_nc, use_spect, use_coord, kernel_size=1, stride=1, padding=0)
        if norm_layer is None:
            self.model = nn.Sequential(nonlinearity, self.conv1, nonlinearity, self.conv2)
            self._norms = None
        else:
            self.model = nn.Sequential(norm_layer(input_nc), nonlinearity, self.conv1, norm_layer(hidden_nc), nonlinearity, self.conv2)
            self._norms = (0, 3)
        self.shortcut = nn.Sequential(self.bypass)
        self._slope = _slope(nonlinearity)

    def bf16_unfit(self):
        """why the bf16 form cannot run this block (None: it can) -- checked at construction by ResEncoder(compute_dtype=torch.bfloat16)"""
        if self._norms is not None:
            return "norm 'none'"
        for name in ("conv1", "conv2", "bypass"):
            c = _conv(getattr(self, name))
            ci, co = c.in_channels, c.out_channels
            if not ((ci == 32 and co in (32, 64)) or (ci % 64 == 0 and co % 64 == 0)):
                return f"{name} with 32 -> 32 / 64 channels or widths that are multiples of 64 (got {ci} -> {co})"
        return None

    def nhwc_bf16(self, x_raw, x_act, raw=True, act=True, f32=False):
        """inference on bf16 activations (ResEncoder(compute_dtype=torch.bfloat16)), norm 'none': x_raw = the block's input, x_act =
        lrelu(x_raw) as the previous tail stored it.  conv1 with bias and LeakyReLU in its output stage, the 1x1 bypass, conv2 with its
        bias, then one tail pass: main + shortcut [2x2 mean] written raw (the next bypass, the feature), activated (the next conv1) and /
        or in fp32 (the distribution head).  Four launches; returns (raw, act, f32), None where not asked for."""
        if self._norms is not None:
            raise FF.FmiError("the bf16 ResBlock is the norm 'none' form (encoder norm 'none'); these run in fp32 only")
        c1, c2, cb = _conv(self.conv1), _conv(self.conv2), _conv(self.bypass)
        h = FF.conv2d_enc_bf16(x_act, packed(c1), c1.bias, 1, self._slope)
        s = FF.conv2d_enc_bf16(x_raw, packed(cb), cb.bias, 0)
        h = FF.conv2d_enc_bf16(h, packed(c2), c2.bias, 1)
        return FF.resblock_tail_bf16(h, s, self.sample, self._slope, raw, act, f32)

    def _conv2_plus_bypass(self, h, xp, in_act):
        """model(x) + shortcut(x): conv2 and the 1x1 bypass as one reduction where the fused launches take the shape (FF.conv2d_pair), else
        the bypass launch and conv2 with its result as the residual of the epilogue"""
        c2, cb = _conv(self.conv2), _conv(self.bypass)
        for c in (c2, cb):
            if c.stride != (1, 1) or c.dilation != (1, 1) or c.groups != 1:
                raise NotImplementedError("Conv2d geometry outside the hot path")
        if c2.padding == (1, 1) and cb.padding == (0, 0):
            return FF.conv2d_pair(h, packed(c2), c2.bias, xp, packed(cb), cb.bias, in_act=in_act)
        s = run_conv(cb, xp)
        return run_conv(c2, h, residual=s, in_act=in_act)

    def nhwc(self, x):
        with weight_scope(self):
            # x has two consumers (the main path and the 1x1 bypass): the bypass reads the pass-through copy the main path's first op
            # hands on, so its gradient re-enters that op's backward kernel instead of an accumulation pass of its own
            if self._norms is None:
                # LeakyReLU -> conv pairs: the activation is applied on the way in and differentiated in the adjoint's epilogue
                act_in = ("apply", self._slope)
                h, xp = run_conv(_conv(self.conv1), x, in_act=act_in, passthrough=True)
                out = self._conv2_plus_bypass(h, xp, act_in)
            else:
                h, xp = _norm_act(self.model[0], x, self._slope, passthrough=True)
                h = run_conv(_conv(self.conv1), h)
                h = _norm_act(self.model[3], h, self._slope)
                out = self._conv2_plus_bypass(h, xp, None)
            if self.sample:  # pool(a) + pool(b) == pool(a + b)
                out = FF.avg_pool(out, 2)
            return out


class ResBlockEncoderOptimized(_NhwcBlock):
    def __init__(self, input_nc, output_nc, norm_layer=nn.BatchNorm2d, nonlinearity=nn.LeakyReLU(), use_spect=False, use_coord=False):
        super().__init__()
        if norm_layer is not None:
            raise NotImplementedError("ResBlockEncoderOptimized runs with norm='none' on the hot path")
        self.conv1 = coord_conv(input_nc, output_nc, use_spect, use_coord, kernel_size=3, stride=1, padding=1)
        self.conv2 = coord_conv(output_nc, output_nc, use_spect, use_coord, kernel_size=3, stride=1, padding=1)
        self.bypass = coord_conv(input_nc, output_nc, use_spect, use_coord, kernel_size=1, stride=1, padding=0)
        self.model = nn.Sequential(self.conv1, nonlinearity, self.conv2, nn.AvgPool2d(kernel_size=2, stride=2))
        self.shortcut = nn.Sequential(nn.AvgPool2d(kernel_size=2, stride=2), self.bypass)
        self._slope = _slope(nonlinearity)

    def nhwc_bf16(self, img):
        """inference from the fp32 image to bf16 activations (ResEncoder(compute_dtype=torch.bfloat16)) in three launches: conv1 reads the
        fp32 image and stores lrelu(conv1 + bias) in bf16, conv2 with its bias, and the tail -- pool2(h) + bypass(pool2(img)) + bias with
        the three-term 1x1 convolution evaluated in the tail itself.  Returns (raw, lrelu(raw)) for the next block's bypass and conv1."""
        c1, c2, cb = _conv(self.conv1), _conv(self.conv2), _conv(self.bypass)
        h = FF.conv2d_thin_in_bf16(img, packed(c1), c1.bias, self._slope)
        h = FF.conv2d_enc_bf16(h, packed(c2), c2.bias, 1)
        return FF.picnet_stem_tail_bf16(h, img, packed(cb).wf[0], cb.bias, self._slope)

    def nhwc(self, x):
        with weight_scope(self):
            h, xp = run_conv(_conv(self.conv1), x, passthrough=True)
            s = run_conv(_conv(self.bypass), FF.avg_pool(xp, 2))
            h = run_conv(_conv(self.conv2), h, in_act=("apply", self._slope))
            return FF.add(FF.avg_pool(h, 2), s)


class ResBlockDecoder(_NhwcBlock):
    def __init__(self, input_nc, output_nc, hidden_nc=None, norm_layer=nn.BatchNorm2d, nonlinearity=nn.LeakyReLU(),
                 use_spect=False, use_coord=False):
        super().__init__()
        hidden_nc = output_nc if hidden_nc is None else hidden_nc
        self.conv1 = spectral_norm(nn.Conv2d(input_nc, hidden_nc, kernel_size=3, stride=1, padding=1), use_spect)
        self.conv2 = spectral_norm(nn.ConvTranspose2d(hidden_nc, output_nc, kernel_size=3, stride=2, padding=1, output_padding=1), use_spect)
        self.bypass = spectral_norm(nn.ConvTranspose2d(input_nc, output_nc, kernel_size=3, stride=2, padding=1, output_padding=1), use_spect)
        if norm_layer is None:
            self.model = nn.Sequential(nonlinearity, self.conv1, nonlinearity, self.conv2)
            self._norms = None
        else:
            self.model = nn.Sequential(norm_layer(input_nc), nonlinearity, self.conv1, norm_layer(hidden_nc), nonlinearity, self.conv2)
            self._norms = (0, 3)
        self.shortcut = nn.Sequential(self.bypass)
        self._slope = _slope(nonlinearity)
        self._pair_geometry = True  # both ConvTranspose2d are kernel 3 / stride 2 / padding 1 / output_padding 1 by construction

    def _nhwc_bf16(self, x):
        """inference on bf16 activations (ResGenerator(compute_dtype=torch.bfloat16)): IN + lrelu, conv1 with its bias in the output stage,
        IN + lrelu, then conv2(h) + bypass(x) as ONE ConvTranspose2d of cat[h, x] and one bias pass -- no fp32 intermediate"""
        if self._norms is None:
            raise FF.FmiError("the bf16 ResBlockDecoder is the InstanceNorm form (decoder norm 'instance')")
        c1, c2, cb = _conv(self.conv1), _conv(self.conv2), _conv(self.bypass)
        h = _norm_act_bf16(self.model[0], x, self._slope)
        h = FF.conv2d_bias_bf16(h, packed(c1), c1.bias, c1.padding[0])
        h = _norm_act_bf16(self.model[3], h, self._slope)
        bias = c2.bias if cb.bias is None else (cb.bias if c2.bias is None else FF.add(c2.bias, cb.bias))
        return FF.conv_transpose2d_cat_bf16(h, packed(c2), x, packed(cb), bias)

    def nhwc(self, x):
        with weight_scope(self):
            if x.dtype == torch.bfloat16:
                return self._nhwc_bf16(x)
            c2, cb = _conv(self.conv2), _conv(self.bypass)
            if self._norms is None:
                h, xp = run_conv(_conv(self.conv1), x, in_act=("apply", self._slope), passthrough=True)
                h = FF.leaky_relu(h, self._slope)
            else:
                h, xp = _norm_act(self.model[0], x, self._slope, passthrough=True)  # the bypass ConvTranspose2d's gradient joins in the IN backward
                h = run_conv(_conv(self.conv1), h)
                h = _norm_act(self.model[3], h, self._slope)
            # main path + bypass: thin outputs on a large map go out as ONE launch (the reduction continues over the bypass input's
            # channels: the intermediate is neither written nor re-read), otherwise the bypass result is the main convolution's residual
            pw2, pwb = packed(c2), packed(cb)
            if self._pair_geometry and FF.conv_transpose2d_pair_ok(h, pw2, xp, pwb):
                bias = c2.bias if cb.bias is None else (cb.bias if c2.bias is None else FF.add(c2.bias, cb.bias))
                return FF.conv_transpose2d_pair(h, pw2, xp, pwb, bias)
            s = run_conv(cb, xp)
            return run_conv(c2, h, residual=s)


class Output(_NhwcBlock):
    def __init__(self, input_nc, output_nc, kernel_size=3, norm_layer=nn.BatchNorm2d, nonlinearity=nn.LeakyReLU(),
                 use_spect=False, use_coord=False):
        super().__init__()
        if norm_layer is not None:
            raise NotImplementedError("Output runs without a norm layer on the hot path (network.py:233-236)")
        self.conv1 = coord_conv(input_nc, output_nc, use_spect, use_coord, kernel_size=kernel_size, padding=0, bias=True)
        self._pad = int(kernel_size / 2)
        self.model = nn.Sequential(nonlinearity, nn.ReflectionPad2d(self._pad), self.conv1, nn.Tanh())
        self._slope = _slope(nonlinearity)

    def nhwc(self, x):
        with weight_scope(self):
            conv = _conv(self.conv1)
            if x.dtype == torch.bfloat16:  # bf16 decoder (inference): the fused pass or nothing, the image leaves in fp32
                if not (self._pad == 1 and conv.stride == (1, 1) and conv.groups == 1 and conv.dilation == (1, 1)):
                    raise FF.FmiError("the bf16 Output block takes the 3 x 3 stride-1 reflect-padded convolution only")
                return FF.lrelu_conv2d_thin_bf16(x, packed(conv), conv.bias, self._slope, 1, FF.ACT_TANH)
            if self._pad == 1 and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.groups == 1 and conv.dilation == (1, 1):
                # LeakyReLU, ReflectionPad2d, the convolution and tanh in one kernel (thin-output path); falls back to
                # LeakyReLU + convolution by itself for shapes that path does not take
                return FF.lrelu_conv2d(x, packed(conv), conv.bias, self._slope, 1, 1, FF.ACT_TANH)
            h = FF.leaky_relu(x, self._slope)
            # ReflectionPad2d is folded into the gather of the implicit GEMM, tanh into its epilogue
            return run_conv(conv, h, act=FF.ACT_TANH, pad_mode=1, pad=self._pad)


class Auto_Attn(nn.Module):
    """Short+Long attention (base_function.py:401-448).  Only the ``pre is None`` form is on the hot path; the
    attention map itself is never materialised, so the second return value is None (every caller discards it:
    network.py:265-268, 364-366).

    ``attn_dtype=torch.bfloat16`` (this build's extra, an opt-in for training an otherwise fp32 model): on an fp32 input the query
    convolution and ``gamma * out + x`` stay fp32, and softmax(q q^T) x runs on the bf16 attention kernels, forward and backward
    (FF.self_attention_bf16_train).  Parameters and state_dict keys are those of the default."""

    def __init__(self, input_nc, norm_layer=nn.BatchNorm2d, attn_dtype=torch.float32):
        super().__init__()
        if attn_dtype not in (torch.float32, torch.bfloat16):
            raise FF.FmiError(f"attn_dtype must be torch.float32 or torch.bfloat16, got {attn_dtype}")
        self.attn_dtype = attn_dtype
        self.input_nc = input_nc
        self.query_conv = nn.Conv2d(input_nc, input_nc // 4, kernel_size=1)
        self.gamma = nn.Parameter(torch.zeros(1))
        self.alpha = nn.Parameter(torch.zeros(1))
        self.softmax = nn.Softmax(dim=-1)
        self.model = ResBlock(int(input_nc * 2), input_nc, input_nc, norm_layer=norm_layer, use_spect=True)
        self.model._fmi_never_runs = True  # the reference never executes it when pre is None; its u/v must not advance

    def check_bf16(self, h, w, c):
        """attn_dtype=torch.bfloat16 on an h x w map of c channels: refused before any device work where the bf16 attention does not
        take the shape -- there is no fp32 detour"""
        why = FF.attention_bf16_unfit(h * w, self.query_conv.out_channels, c) if self.attn_dtype == torch.bfloat16 else None
        if why:
            raise FF.FmiError(f"Auto_Attn(attn_dtype=torch.bfloat16) needs {why} from a {h} x {w} map; these run in fp32 only")

    def nhwc(self, x):
        with weight_scope(self):
            n, h, w, c = x.shape
            if x.dtype == torch.bfloat16:  # bf16 decoder (inference): gamma * out + x is the attention kernel's epilogue
                q = FF.conv2d_bias_bf16(x, packed(self.query_conv), self.query_conv.bias, 0)
                xv = x.view(n, h * w, c)
                return FF.self_attention_bf16(q.view(n, h * w, -1), xv, self.gamma, xv).view(n, h, w, c)
            self.check_bf16(h, w, c)
            q = run_conv(self.query_conv, x)
            if self.attn_dtype == torch.bfloat16:
                o = FF.self_attention_bf16_train(q.view(n, h * w, -1), x.view(n, h * w, c))
            else:
                (o,) = FF.self_attention(q.view(n, h * w, -1), [x.view(n, h * w, c)])
            return FF.scale_add_param(o.view(n, h, w, c), self.gamma, x)

    def forward(self, x, pre=None, mask=None):
        if pre is not None:
            raise NotImplementedError("the long-term (pre/mask) branch of Auto_Attn is never taken by the reference's callers")
        if x.dtype != torch.bfloat16:
            self.check_bf16(x.shape[2], x.shape[3], x.shape[1])
        return FF.to_nchw(self.nhwc(FF.to_nhwc(x))), None
