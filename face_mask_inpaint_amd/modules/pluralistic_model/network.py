"""Host-side mirror of modules/pluralistic_model/network.py: define_e / define_g / define_d and the
ResEncoder / ResGenerator / ResDiscriminator networks with the reference's constructor arguments, attribute
names (``block0``, ``encoder{i}``, ``infer_prior{i}``, ``prior`` / ``posterior``, ``generator``, ``decoder{i}``,
``out{i}``, ``attn{i}``, ``block1``, ``conv``) and forward signatures; all arithmetic runs in the HIP kernels.
PatchDiscriminator (``--disc_model_type PatchDis``, network.py:373-430) is mirrored too.
"""
from __future__ import annotations

import torch
from torch import nn

from ... import functional as FF
from ...weights import weight_scope
from .base_function import (Auto_Attn, Output, ResBlock, ResBlockDecoder, ResBlockEncoderOptimized, _conv, get_nonlinearity_layer,
                            get_norm_layer, init_net, _slope)
from .external_function import SpectralNorm, run_conv


def define_e(encoder_type="src", input_nc=3, ngf=64, z_nc=512, img_f=512, L=6, layers=5, norm="none", activation="ReLU",
             use_spect=True, use_coord=False, init_type="orthogonal", gpu_ids=[], compute_dtype=torch.float32):
    net = ResEncoder(input_nc, ngf, z_nc, img_f, L, layers, norm, activation, use_spect, use_coord, encoder_type, compute_dtype=compute_dtype)
    return init_net(net, init_type, activation, gpu_ids)


def define_g(output_nc=3, ngf=64, z_nc=512, img_f=512, L=1, layers=5, norm="instance", activation="ReLU", use_spect=True,
             use_coord=False, use_attn=True, init_type="orthogonal", gpu_ids=[], compute_dtype=torch.float32, attn_dtype=torch.float32):
    net = ResGenerator(output_nc, ngf, z_nc, img_f, L, layers, norm, activation, use_spect, use_coord, use_attn, compute_dtype=compute_dtype,
                       attn_dtype=attn_dtype)
    return init_net(net, init_type, activation, gpu_ids)


def define_d(input_nc=3, ndf=64, img_f=512, layers=6, norm="none", activation="LeakyReLU", use_spect=True, use_coord=False,
             use_attn=True, model_type="ResDis", init_type="orthogonal", gpu_ids=[]):
    if model_type == "ResDis":
        net = ResDiscriminator(input_nc, ndf, img_f, layers, norm, activation, use_spect, use_coord, use_attn)
    elif model_type == "PatchDis":
        net = PatchDiscriminator(input_nc, ndf, img_f, layers, norm, activation, use_spect, use_coord, use_attn)
    else:
        raise NotImplementedError("model_type %s" % model_type)
    return init_net(net, init_type, activation, gpu_ids)


class ResEncoder(nn.Module):
    """network.py:76-178.  forward(img) -> ([mu, softplus(std)], feature); the fused training path uses
    ``nhwc_raw`` which returns the un-split distribution head so that split/softplus/rsample happen in one kernel.
    ``compute_dtype=torch.bfloat16`` (this build's extra, inference only): the stem's first convolution reads the fp32 image, every
    activation stored after it is bf16, the feature map comes back in bf16 and the un-split distribution head in fp32, written by the last
    block's tail.  Parameters, state_dict keys and SpectralNorm state are those of the fp32 build."""

    def __init__(self, input_nc=3, ngf=64, z_nc=128, img_f=1024, L=6, layers=6, norm="none", activation="ReLU",
                 use_spect=True, use_coord=False, encoder_type="src", compute_dtype=torch.float32):
        super().__init__()
        if compute_dtype not in (torch.float32, torch.bfloat16):
            raise FF.FmiError(f"compute_dtype must be torch.float32 or torch.bfloat16, got {compute_dtype}")
        self.compute_dtype = compute_dtype
        if compute_dtype == torch.bfloat16:
            self._check_bf16(input_nc, ngf, norm)
        self.layers, self.z_nc, self.L = layers, z_nc, L
        self.ecnoder_type = encoder_type  # (sic) attribute name of the reference
        norm_layer = get_norm_layer(norm_type=norm)
        nonlinearity = get_nonlinearity_layer(activation_type=activation)
        self.block0 = ResBlockEncoderOptimized(input_nc, ngf, norm_layer, nonlinearity, use_spect, use_coord)
        mult = 1
        for i in range(layers - 1):
            mult_prev = mult
            mult = min(2 ** (i + 1), img_f // ngf)
            block = ResBlock(ngf * mult_prev, ngf * mult, ngf * mult_prev, norm_layer, nonlinearity,
                             "none" if i % 2 == 0 else "down", use_spect, use_coord)
            setattr(self, "encoder" + str(i), block)
        if encoder_type == "src":
            for i in range(self.L):
                setattr(self, "infer_prior" + str(i),
                        ResBlock(ngf * mult, ngf * mult, ngf * mult, norm_layer, nonlinearity, "none", use_spect, use_coord))
            self.prior = ResBlock(ngf * mult, 2 * z_nc, ngf * mult, norm_layer, nonlinearity, "none", use_spect, use_coord)
        elif encoder_type == "ref":
            self.posterior = ResBlock(ngf * mult, 2 * z_nc, ngf * mult, norm_layer, nonlinearity, "none", use_spect, use_coord)
        else:
            raise NotImplementedError(encoder_type)
        self._down = 2 ** (1 + (layers - 1) // 2)  # the stem and every second encoder block halve the map
        if compute_dtype == torch.bfloat16:
            self._check_bf16(input_nc, ngf, norm, blocks=True)
            for m in self.modules():
                if isinstance(m, nn.Conv2d):
                    object.__setattr__(m, "_fmi_no_w3", True)  # these run on bf16 activations: no fp32 piece images of their packs

    def _check_bf16(self, input_nc, ngf, norm, blocks=False):
        """the shapes the bf16 kernels take, refused at construction (the arguments before any block is built, the blocks' widths after):
        there is no fp32 detour for a block that does not fit"""
        why = None
        if norm != "none":
            why = f"encoder norm 'none' (got {norm!r})"
        elif ngf != 32:
            why = f"ngf == 32, the width of the stem's kernels (got {ngf})"
        elif input_nc > 4:
            why = f"an image of at most 4 channels (got {input_nc})"
        elif blocks:
            for name, block in self.named_children():
                unfit = block.bf16_unfit() if isinstance(block, ResBlock) else None
                if unfit:
                    why = f"{name}.{unfit}"
                    break
        if why:
            raise FF.FmiError(f"ResEncoder(compute_dtype=torch.bfloat16) needs {why}; these run in fp32 only")

    def check_inference(self, *inputs):
        """the bf16 encoder has no backward: refuse, before any device work, a call that autograd would record"""
        if self.compute_dtype == torch.bfloat16 and torch.is_grad_enabled() and (
                any(t is not None and t.requires_grad for t in inputs) or any(p.requires_grad for p in self.parameters())):
            raise FF.FmiError("the bf16 encoder (compute_dtype=torch.bfloat16) is inference only -- no bf16 backward exists: call it under "
                              "torch.no_grad(), or build the encoder with compute_dtype=torch.float32 to train")

    def check_extent(self, h, w):
        """the bf16 path halves the map log2(_down) times with 2x2 means: refused on the host where H or W does not divide"""
        if self.compute_dtype == torch.bfloat16 and (h % self._down or w % self._down):
            raise FF.FmiError(f"the bf16 encoder needs H and W to be multiples of {self._down}, got {h} x {w}; these run in fp32 only")

    def _nhwc_raw_bf16(self, img):
        raw, act = self.block0.nhwc_bf16(img)
        for i in range(self.layers - 1):
            raw, act, _ = getattr(self, "encoder" + str(i)).nhwc_bf16(raw, act)
        feat = raw
        if self.ecnoder_type == "src":
            for i in range(self.L):
                raw, act, _ = getattr(self, "infer_prior" + str(i)).nhwc_bf16(raw, act)
            head = self.prior
        else:
            head = self.posterior
        _, _, o = head.nhwc_bf16(raw, act, raw=False, act=False, f32=True)  # the fp32 head leaves the tail itself: no cast afterwards
        return o, feat

    def nhwc_raw(self, img):
        """returns (o [N,h,w,2*z_nc] = un-split (mu, raw std), feature [N,h,w,C])"""
        self.check_inference(img)
        self.check_extent(img.shape[1], img.shape[2])
        with weight_scope(self):
            if self.compute_dtype == torch.bfloat16:
                return self._nhwc_raw_bf16(img)
            out = self.block0.nhwc(img)
            for i in range(self.layers - 1):
                out = getattr(self, "encoder" + str(i)).nhwc(out)
            enc = out
            if self.ecnoder_type == "src":
                for i in range(self.L):
                    enc = getattr(self, "infer_prior" + str(i)).nhwc(enc)
                o = self.prior.nhwc(enc)
            else:
                o = self.posterior.nhwc(enc)
            return o, out

    def forward(self, img):
        o, feat = self.nhwc_raw(FF.to_nhwc(img))
        mu = o[..., : self.z_nc].contiguous()
        std = FF._Softplus.apply(o[..., self.z_nc:].contiguous())
        return [FF.to_nchw(mu), FF.to_nchw(std)], FF.to_nchw(feat)


class ResGenerator(nn.Module):
    """network.py:181-307.  ``compute_dtype=torch.bfloat16`` (this build's extra, inference only): the latent ResBlocks stay fp32,
    ``encoded + f`` is cast to bf16 once, and decoder0.., attn1 and the Output block run on the bf16 kernels; the image leaves the
    Output block in fp32.  Parameters, state_dict keys and SpectralNorm state are those of the fp32 build.
    ``attn_dtype=torch.bfloat16`` (likewise an extra, and trainable): the fp32 generator with attn1's softmax(q q^T) x alone on the bf16
    attention kernels, forward and backward (Auto_Attn); everything else, and every default, is the fp32 build's."""

    def __init__(self, output_nc=3, ngf=64, z_nc=128, img_f=1024, L=1, layers=6, norm="batch", activation="ReLU",
                 use_spect=True, use_coord=False, use_attn=False, compute_dtype=torch.float32, attn_dtype=torch.float32):
        super().__init__()
        if compute_dtype not in (torch.float32, torch.bfloat16):
            raise FF.FmiError(f"compute_dtype must be torch.float32 or torch.bfloat16, got {compute_dtype}")
        if attn_dtype not in (torch.float32, torch.bfloat16):
            raise FF.FmiError(f"attn_dtype must be torch.float32 or torch.bfloat16, got {attn_dtype}")
        self.compute_dtype = compute_dtype
        self.attn_dtype = attn_dtype
        self.layers, self.L, self.use_attn = layers, L, use_attn
        norm_layer = get_norm_layer(norm_type=norm)
        nonlinearity = get_nonlinearity_layer(activation_type=activation)
        mult = min(2 ** (layers - 1), img_f // ngf)
        ch = int(ngf * mult)
        self.generator = ResBlock(z_nc, ch, ch, None, nonlinearity, "none", use_spect, use_coord)
        for i in range(self.L):
            setattr(self, "generator" + str(i), ResBlock(ch, ch, ch, None, nonlinearity, "none", use_spect, use_coord))
        for i in range(layers):
            mult_prev = mult
            mult = min(2 ** (layers - i - 1), img_f // ngf)
            prev_ch, ch = int(ngf * mult_prev), int(ngf * mult)
            setattr(self, "decoder" + str(i), ResBlockDecoder(prev_ch, ch, ch, norm_layer, nonlinearity, use_spect, use_coord))
            if i > layers - 2:
                setattr(self, "out" + str(i), Output(ch, output_nc, 3, None, nonlinearity, use_spect, use_coord))
            if i == 1 and use_attn:
                setattr(self, "attn" + str(i), Auto_Attn(ch, None, attn_dtype=attn_dtype))
                if attn_dtype == torch.bfloat16 and (ch // 4, ch) not in FF.ATTN_BF16_SHAPES:
                    raise FF.FmiError(f"ResGenerator(attn_dtype=torch.bfloat16) needs (d_qk, C) in {{(64, 256), (32, 128)}} at attn{i} "
                                      f"(got ({ch // 4}, {ch})); these channel counts run in fp32 only")
            if compute_dtype == torch.bfloat16:
                self._check_bf16_block(i, prev_ch, ch, norm, use_attn)
        if compute_dtype == torch.bfloat16:
            for name, block in self.named_children():
                if name.startswith(("decoder", "out")):
                    for m in block.modules():
                        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                            object.__setattr__(m, "_fmi_no_w3", True)  # these run on bf16 activations: no fp32 piece images of their packs
                elif name.startswith("attn"):  # Auto_Attn.model never runs
                    object.__setattr__(block.query_conv, "_fmi_no_w3", True)

    def _check_bf16_block(self, i, prev_ch, ch, norm, use_attn):
        """the widths the bf16 kernels take, refused at construction: there is no fp32 detour for a block that does not fit"""
        why = None
        if norm != "instance":
            why = f"decoder norm 'instance' (got {norm!r})"
        elif prev_ch % 64:
            why = f"decoder{i}.conv1 input channels % 64 == 0 (got {prev_ch})"
        elif ch % 8 or (ch + prev_ch) % 32:
            why = f"decoder{i} widths with hidden % 8 == 0 and (hidden + input) % 32 == 0 (got {ch} + {prev_ch})"
        elif i > self.layers - 2 and ch != 32:
            why = f"32 channels into out{i} (got {ch})"
        elif i == 1 and use_attn and (ch // 4, ch) not in ((64, 256), (32, 128)):
            why = f"(d_qk, C) in {{(64, 256), (32, 128)}} at attn{i} (got ({ch // 4}, {ch}))"
        if why:
            raise FF.FmiError(f"ResGenerator(compute_dtype=torch.bfloat16) needs {why}; these channel counts run in fp32 only")

    def check_inference(self, *inputs):
        """the bf16 decoder has no backward: refuse, before any device work, a call that autograd would record"""
        if self.compute_dtype == torch.bfloat16 and torch.is_grad_enabled() and (
                any(t is not None and t.requires_grad for t in inputs) or any(p.requires_grad for p in self.parameters())):
            raise FF.FmiError("the bf16 decoder (compute_dtype=torch.bfloat16) is inference only -- no bf16 backward exists: call it under "
                              "torch.no_grad(), or build the generator with compute_dtype=torch.float32 to train")

    def nhwc(self, encoded, z=None):
        bf16 = self.compute_dtype == torch.bfloat16
        self.check_inference(encoded, z)
        if bf16 and self.use_attn and self.layers > 1 and (16 * encoded.shape[1] * encoded.shape[2]) % 128:
            raise FF.FmiError(f"the bf16 attention at attn1 needs a token count that is a multiple of 128: a {encoded.shape[1]} x "
                              f"{encoded.shape[2]} feature map gives {16 * encoded.shape[1] * encoded.shape[2]} tokens")
        if not bf16 and self.attn_dtype == torch.bfloat16 and self.use_attn and self.layers > 1 and (
                16 * encoded.shape[1] * encoded.shape[2]) % 128:
            raise FF.FmiError(f"ResGenerator(attn_dtype=torch.bfloat16): the bf16 attention at attn1 needs a token count that is a multiple "
                              f"of 128: a {encoded.shape[1]} x {encoded.shape[2]} feature map gives "
                              f"{16 * encoded.shape[1] * encoded.shape[2]} tokens; these run in fp32 only")
        with weight_scope(self):
            if z is not None:
                f = self.generator.nhwc(z)
                for i in range(self.L):
                    f = getattr(self, "generator" + str(i)).nhwc(f)
                out = FF.add(encoded, f)
            else:
                out = encoded
            if bf16:
                out = out.to(torch.bfloat16)  # the one cast: everything from decoder0 to the Output block's input is bf16
            output = None
            for i in range(self.layers):
                out = getattr(self, "decoder" + str(i)).nhwc(out)
                if i == 1 and self.use_attn:
                    out = getattr(self, "attn" + str(i)).nhwc(out)
                if i > self.layers - 2:
                    # the reference also builds cat([out, output]) here, which nothing reads (network.py:272)
                    output = getattr(self, "out" + str(i)).nhwc(out)
            return output

    def forward(self, encoded, z=None, f_e=None, mask=None):
        if f_e is not None or mask is not None:
            raise NotImplementedError("f_e / mask are never passed by the reference's callers")
        return FF.to_nchw(self.nhwc(FF.to_nhwc(encoded), None if z is None else FF.to_nhwc(z)))

    def get_z(self, src_distribution, ref_distribution, return_zq=False, mask=None, eps=None):
        """network.py:275-307 on NCHW-shaped (mu, sigma) pairs.  ``eps = (eps_p, eps_q)`` injects the two
        standard-normal draws (posterior first, as rsample is called in the reference); default: fresh draws."""
        p_mu, p_sigma = ref_distribution
        q_mu, q_sigma = src_distribution
        if eps is None:
            eps = (torch.randn_like(p_mu), torch.randn_like(q_mu))
        z_p = FF._MulAdd.apply(p_sigma.contiguous(), eps[0].contiguous(), p_mu.contiguous())
        z_q = FF._MulAdd.apply(q_sigma.contiguous(), eps[1].contiguous(), q_mu.contiguous())
        if return_zq:
            return z_q
        return torch.cat([z_q, z_p], dim=1)


class ResDiscriminator(nn.Module):
    """network.py:310-370."""

    def __init__(self, input_nc=3, ndf=64, img_f=1024, layers=6, norm="none", activation="LeakyReLU", use_spect=True,
                 use_coord=False, use_attn=True):
        super().__init__()
        self.layers, self.use_attn = layers, use_attn
        norm_layer = get_norm_layer(norm_type=norm)
        nonlinearity = get_nonlinearity_layer(activation_type=activation)
        self.nonlinearity = nonlinearity
        self.block0 = ResBlockEncoderOptimized(input_nc, ndf, norm_layer, nonlinearity, use_spect, use_coord)
        mult = 1
        for i in range(layers - 1):
            mult_prev = mult
            mult = min(2 ** (i + 1), img_f // ndf)
            if i == 2 and use_attn:
                setattr(self, "attn" + str(i), Auto_Attn(ndf * mult_prev, norm_layer))
            setattr(self, "encoder" + str(i),
                    ResBlock(ndf * mult_prev, ndf * mult, ndf * mult_prev, norm_layer, nonlinearity, "down", use_spect, use_coord))
        self.block1 = ResBlock(ndf * mult, ndf * mult, ndf * mult, norm_layer, nonlinearity, "none", use_spect, use_coord)
        self.conv = SpectralNorm(nn.Conv2d(ndf * mult, 1, 3))
        self._slope = _slope(nonlinearity)

    def nhwc(self, x):
        with weight_scope(self):
            out = self.block0.nhwc(x)
            for i in range(self.layers - 1):
                if i == 2 and self.use_attn:
                    out = getattr(self, "attn" + str(i)).nhwc(out)
                out = getattr(self, "encoder" + str(i)).nhwc(out)
            out = self.block1.nhwc(out)
            return run_conv(_conv(self.conv), FF.leaky_relu(out, self._slope))

    def forward(self, x):
        return FF.to_nchw(self.nhwc(FF.to_nhwc(x)))


class PatchDiscriminator(nn.Module):
    """network.py:373-430 (``--disc_model_type PatchDis``): ``layers`` 4x4 stride-2 SpectralNorm convs + two 4x4 stride-1 ones,
    LeakyReLU in between, no bias, no norm layer (the reference builds ``norm_layer`` and never uses it).  ``model.N`` keys as in
    the reference's nn.Sequential."""

    def __init__(self, input_nc=3, ndf=64, img_f=512, layers=3, norm="batch", activation="LeakyReLU", use_spect=True, use_coord=False,
                 use_attn=False):
        super().__init__()
        from .base_function import coord_conv

        nonlinearity = get_nonlinearity_layer(activation_type=activation)
        self._slope = _slope(nonlinearity)
        kwargs = {"kernel_size": 4, "stride": 2, "padding": 1, "bias": False}
        sequence = [coord_conv(input_nc, ndf, use_spect, use_coord, **kwargs), nonlinearity]
        mult, i = 1, 0
        for i in range(1, layers):
            mult_prev = mult
            mult = min(2 ** i, img_f // ndf)
            sequence += [coord_conv(ndf * mult_prev, ndf * mult, use_spect, use_coord, **kwargs), nonlinearity]
        mult_prev = mult
        mult = min(2 ** i, img_f // ndf)
        kwargs = {"kernel_size": 4, "stride": 1, "padding": 1, "bias": False}
        sequence += [coord_conv(ndf * mult_prev, ndf * mult, use_spect, use_coord, **kwargs), nonlinearity,
                     coord_conv(ndf * mult, 1, use_spect, use_coord, **kwargs)]
        self.model = nn.Sequential(*sequence)

    def nhwc(self, x):
        with weight_scope(self):
            for m in self.model:
                x = FF.leaky_relu(x, self._slope) if isinstance(m, (nn.LeakyReLU, nn.ReLU)) else run_conv(_conv(m), x)
            return x

    def forward(self, x):
        return FF.to_nchw(self.nhwc(FF.to_nhwc(x)))
