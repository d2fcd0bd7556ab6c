"""GauGAN under GAN Compression: the pruned "sub-mobile" SPADE generator built on sige_amd.nn.

The network of gaugan/models/sub_mobile_spade_generators/sige_fused_sub_mobile_spade_generator.py (the reference's
`SIGEFusedSubMobileSPADEGenerator`, `--netG sige_fused_sub_mobile_spade --config_str 32_32_32_48_32_24_24_32`).  It differs from
gaugan_spade.py's generator in two ways:
  * pruned widths: every block has its own input width `ic`, width `channel` and label-branch width `hidden`, from the config string;
  * gamma and beta of a SPADE layer each come from a separable conv (mobile_modules.py:65-119 SIGESeparableConv2d): depthwise 3x3
    with bias -> InstanceNorm -> pointwise 1x1 with bias.  The full pass remembers the InstanceNorm of every TILED layer as a
    per-channel affine (scale = 1 / sqrt(var + eps), shift = -mean * scale); sparse mode applies that affine to the edited tiles.
    The blocks below `num_sparse_layers` are recomputed densely in sparse mode, InstanceNorm statistics included, as in the reference.
Parameter and buffer names are the reference's (`up_1.norm_s.mlp_gamma.conv.0.weight`, `....conv.2.bias`,
`....param_free_norm.running_mean`, `conv_s`, `fc`, `conv_img`): its state dict loads with strict=True.

Everything else -- the label-branch split, the one-pass SPADE modulation, the dense layers' convs, the resizes, the image tail -- is
gaugan_spade.py's code: gamma | beta are concatenated and go through ONE ScatterGather (or Scatter + Gather), so the cache is the
[1, 2 oc, H, W] tensor hip.spade_modulate_cl expects.

Sparse mode computes gamma | beta of a layer in one of two forms with the same arithmetic:
  * SEPARABLE_NATIVE: ONE launch of hip.spade_separable_cl (csrc/spade_separable.hip) on channels-last GPU tensors -- tile slabs for
    the tiled layers, the full tensor for the dense ones, behind its InstanceNorm statistics: a torch prologue, or ONE more launch
    (hip.spade_separable_stats_cl; SEPARABLE_STATS_NATIVE, and always in a stacked forward, where every edit has its own affine);
  * the reference's chain: depthwise SIGEConv2d(groups=Ch), affine, 1x1 SIGEConv2d, per branch, then torch.cat.  Whatever the
    kernel refuses takes the chain.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch import nn
from torch.nn import functional as F

from ..nn import Gather, SIGEConv2d, SIGEModel, SIGEModule
from ..nn import deferred
from .gaugan_spade import SPADEConfig, SpadeGenerator, SpadeNorm, SpadeResBlock, _cl_gpu, _refuse_in_stacked_mode

# One hip.spade_separable_cl launch per SPADE layer in sparse mode.  False: the reference's module chain.  The default follows the
# measurement in DESIGN.md 5.18 (tools/sub_mobile_bench.py).
SEPARABLE_NATIVE = True
# The InstanceNorm statistics of a dense SPADE layer from ONE hip.spade_separable_stats_cl launch in a single-edit forward too (a
# stacked forward always takes it).  False: the torch prologue -- a grouped conv, var_mean and four elementwise kernels per layer.
# The default follows the A/B in DESIGN.md 5.23 (tools/sub_mobile_bench.py --stacked): on, 0.24 - 0.26 ms of a 0.79 - 1.09 ms forward.
SEPARABLE_STATS_NATIVE = True


@dataclass
class SubMobileSPADEConfig(SPADEConfig):
    channels: Tuple[int, ...] = (32, 32, 32, 48, 32, 24, 24, 32)  # --config_str 32_32_32_48_32_24_24_32
    num_sparse_layers: int = 4                                    # (the value of the reference's README)

    @staticmethod
    def decode(config_str: str, **kw) -> "SubMobileSPADEConfig":
        return SubMobileSPADEConfig(channels=tuple(int(c) for c in config_str.split("_")), **kw)


def _instance_norm_affine(d: torch.Tensor, eps: float):
    """(scale, shift) [C] of InstanceNorm over one image: biased variance (mobile_modules.py:7-25 my_instance_norm)."""
    var, mean = torch.var_mean(d, unbiased=False, dim=[2, 3])
    std = torch.sqrt(var[0] + eps)
    return 1 / std, -(mean[0] / std)


class SeparableConv(SIGEModule):
    """depthwise 3x3 + bias -> InstanceNorm -> pointwise 1x1 + bias (SIGESeparableConv2d)."""

    def __init__(self, in_channels: int, out_channels: int, tiled: bool):
        super().__init__()
        self.tiled = tiled
        Conv = SIGEConv2d if tiled else nn.Conv2d
        self.conv = nn.Sequential(Conv(in_channels, in_channels, 3, padding=1, groups=in_channels), nn.InstanceNorm2d(in_channels),
                                  Conv(in_channels, out_channels, 1))
        self.scale = self.shift = None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.mode == "full":
            if x.shape[0] != 1:
                raise RuntimeError("SeparableConv: the cached InstanceNorm affine is that of ONE image (batch %d)" % x.shape[0])
            d = self.conv[0](x)
            self.scale, self.shift = _instance_norm_affine(d, self.conv[1].eps)
            return self.conv[2](d * self.scale.view(1, -1, 1, 1) + self.shift.view(1, -1, 1, 1))
        if self.mode in ("sparse", "profile"):
            if self.tiled:
                d = deferred.resolve(self.conv[0](x))
                return self.conv[2](d * self.scale.view(1, -1, 1, 1) + self.shift.view(1, -1, 1, 1))
            _refuse_in_stacked_mode(x, "a dense separable conv")
            return self.conv(x)
        raise NotImplementedError("Unknown mode [%s]!!!" % self.mode)


class SubMobileSpadeNorm(SpadeNorm):
    """One sub-mobile SPADE layer (sige_normalization.py:91-170 SIGEFusedSubMobileSPADE): param-free BatchNorm (running statistics)
    over `oc` channels, modulated by gamma = mlp_gamma(label features), beta = mlp_beta(label features), two separable convs."""

    def __init__(self, cfg: SPADEConfig, nhidden: int, oc: int, seg_gather: Optional[Gather], shortcut_conv: Optional[nn.Conv2d] = None):
        SIGEModule.__init__(self)
        from ..nn import Scatter, ScatterGather

        self.channels = oc
        self.nhidden = nhidden
        self.role = "shortcut" if shortcut_conv is not None else "main"
        self.tiled = seg_gather is not None
        self.param_free_norm = nn.BatchNorm2d(oc, affine=False, eps=cfg.bn_eps)
        self.mlp_gamma = SeparableConv(nhidden, oc, self.tiled)
        self.mlp_beta = SeparableConv(nhidden, oc, self.tiled)
        if self.tiled and self.role == "shortcut":
            self.scatter = Scatter(seg_gather)
            self.gather = Gather(shortcut_conv, cfg.shortcut_block_size)
        elif self.tiled:
            self.scatter_gather = ScatterGather(seg_gather)
        self.scale = self.shift = None
        self._sep_affine = None               # [2, Ch] scale and shift of (gamma, beta): restacked by every full pass
        self._sep_weights = self._sep_key = None

    # -- operands of the one-launch form -----------------------------------------------------------------------------------------
    def _stacked_weights(self):
        """(dw_w [2,Ch,3,3], dw_b [2,Ch], pw_w [2,oc,Ch], pw_b [2,oc]) of (gamma, beta), rebuilt when a weight changes or moves."""
        g, b = self.mlp_gamma.conv, self.mlp_beta.conv
        params = (g[0].weight, g[0].bias, g[2].weight, g[2].bias, b[0].weight, b[0].bias, b[2].weight, b[2].bias)
        key = tuple((p.data_ptr(), p._version, p.device) for p in params)
        if self._sep_key != key:
            with torch.no_grad():
                Ch, oc = self.nhidden, self.channels
                self._sep_weights = (torch.stack([g[0].weight.reshape(Ch, 3, 3), b[0].weight.reshape(Ch, 3, 3)]).contiguous(),
                                     torch.stack([g[0].bias, b[0].bias]).contiguous(),
                                     torch.stack([g[2].weight.reshape(oc, Ch), b[2].weight.reshape(oc, Ch)]).contiguous(),
                                     torch.stack([g[2].bias, b[2].bias]).contiguous())
            self._sep_key = key
        return self._sep_weights

    def _native(self, actv: torch.Tensor) -> Optional[torch.Tensor]:
        """gamma | beta in one launch, or None where the kernel does not apply."""
        if not (SEPARABLE_NATIVE and self.mode == "sparse" and _cl_gpu(actv)):
            return None
        from .. import hip

        dw_w, dw_b, pw_w, pw_b = self._stacked_weights()
        if self.tiled:
            if self._sep_affine is None or tuple(actv.shape[2:]) != (6, 6):
                return None
            sc, sh = self._sep_affine
        else:
            # the reference recomputes a dense layer's InstanceNorm on the edited label features, so in a stacked forward every edit
            # has its own: one statistics launch ([E,2,Ch], hip.spade_separable_stats_cl), then the launch applies them per image
            stacked = hip.get_edit_batch() > 1
            stats = None
            if stacked or SEPARABLE_STATS_NATIVE:
                stats = hip.spade_separable_stats_cl(actv, dw_w, dw_b, self.mlp_gamma.conv[1].eps)
            if stats is not None:
                sc, sh = stats
            else:
                # ... or its statistics from ONE grouped conv (output channel 2 c + b = branch b of channel c) and torch kernels
                _refuse_in_stacked_mode(actv, "the InstanceNorm statistics of a dense separable conv")
                Ch = self.nhidden
                d = F.conv2d(actv, dw_w.transpose(0, 1).reshape(2 * Ch, 1, 3, 3), dw_b.t().reshape(-1), padding=1, groups=Ch)
                sc, sh = _instance_norm_affine(d, self.mlp_gamma.conv[1].eps)
                sc, sh = sc.view(Ch, 2).t().contiguous(), sh.view(Ch, 2).t().contiguous()
            out = hip.spade_separable_cl(actv, dw_w, dw_b, sc, sh, pw_w, pw_b, tiled=False)
            if out is None:
                _refuse_in_stacked_mode(actv, "a dense separable conv")  # (the module chain is torch: no seam-aware form)
            return out
        return hip.spade_separable_cl(actv, dw_w, dw_b, sc, sh, pw_w, pw_b, tiled=self.tiled)

    def mlp_gamma_beta(self, actv: torch.Tensor) -> torch.Tensor:
        """gamma | beta [*, 2 oc, h, w]: what gaugan_spade.SpadeNorm's one 3x3 conv of the same name returns."""
        actv = deferred.resolve(actv)
        out = self._native(actv)
        if out is not None:
            return out
        gb = torch.cat([self.mlp_gamma(actv), self.mlp_beta(actv)], dim=1)
        if self.mode == "full":
            with torch.no_grad():
                self._sep_affine = (torch.stack([self.mlp_gamma.scale, self.mlp_beta.scale]).contiguous(),
                                    torch.stack([self.mlp_gamma.shift, self.mlp_beta.shift]).contiguous())
        return gb

    def _gamma_beta(self, actv: torch.Tensor) -> torch.Tensor:
        return self.mlp_gamma_beta(actv)


class SubMobileSpadeResBlock(SpadeResBlock):
    """SIGEFusedSubMobileSPADEResnetBlock: x has `ic` channels; conv_0 ic -> channel, conv_1 channel -> channel (learned shortcut,
    conv_s ic -> channel) or channel -> ic; `learned` is decided by the UNPRUNED widths (fin != fout), as in the reference."""

    def __init__(self, cfg: SPADEConfig, learned: bool, ic: int, channel: int, hidden: int, tiled: bool):
        super().__init__(cfg, ic, channel if learned else ic, tiled, fmid=channel, nhidden=hidden, learned_shortcut=learned,
                         make_norm=lambda oc, seg_gather, shortcut_conv=None: SubMobileSpadeNorm(cfg, hidden, oc, seg_gather, shortcut_conv))
        self.ic = ic


class SubMobileSpadeGenerator(SpadeGenerator):
    def __init__(self, cfg: SubMobileSPADEConfig = SubMobileSPADEConfig()):
        SIGEModel.__init__(self)
        if cfg.num_upsampling_layers == "most":
            raise NotImplementedError("the sub-mobile generator has no 'most' form (sige_fused_sub_mobile_spade_generator.py:283)")
        if len(cfg.channels) != 8:
            raise ValueError("SubMobileSPADEConfig.channels: eight widths (fc, head_0, G_middle_0, G_middle_1, up_0 .. up_3)")
        self.cfg = cfg
        ups = {"normal": 5, "more": 6}[cfg.num_upsampling_layers]
        self.sw = cfg.crop_size // (2 ** ups)
        self.sh = round(self.sw / cfg.aspect_ratio)
        c, k = cfg.channels, cfg.num_sparse_layers
        ic = 16 * c[0]
        self.fc = nn.Conv2d(cfg.semantic_nc, ic, 3, padding=1)
        self.head_0 = SubMobileSpadeResBlock(cfg, False, ic, 16 * c[1], 2 * c[1], k >= 7)
        self.G_middle_0 = SubMobileSpadeResBlock(cfg, False, ic, 16 * c[2], 2 * c[2], k >= 6)
        self.G_middle_1 = SubMobileSpadeResBlock(cfg, False, ic, 16 * c[3], 2 * c[3], k >= 5)
        self.up_0 = SubMobileSpadeResBlock(cfg, True, ic, 8 * c[4], 2 * c[4], k >= 4)
        self.up_1 = SubMobileSpadeResBlock(cfg, True, 8 * c[4], 4 * c[5], 2 * c[5], k >= 3)
        self.up_2 = SubMobileSpadeResBlock(cfg, True, 4 * c[5], 2 * c[6], 2 * c[6], k >= 2)
        self.up_3 = SubMobileSpadeResBlock(cfg, True, 2 * c[6], c[7], 2 * c[7], k >= 1)
        self.conv_img = nn.Conv2d(c[7], 3, 3, padding=1)
        self.edit_batch = 1

    def _forward(self, seg: torch.Tensor) -> torch.Tensor:
        if self.edit_batch > 1:
            # stacked edits (sige_amd/stacked.py) are SpadeGenerator's path: E label maps, one per edit, on the tall tensor; the dense
            # SPADE layers take one InstanceNorm affine per edit (SubMobileSpadeNorm._native).  The library finds the seams by a shift
            if self.sh < 4 or self.sh & (self.sh - 1):
                raise RuntimeError("SubMobileSpadeGenerator: stacked edits need a power-of-two height of at least 4 rows at the smallest "
                                   "level (this configuration has %d x %d)" % (self.sh, self.sw))
            return super()._forward(seg)
        _refuse_in_stacked_mode(seg, "the sub-mobile generator")
        if seg.shape[0] != 1:
            raise RuntimeError("SubMobileSpadeGenerator: batch 1 only -- the InstanceNorm of the separable convs is cached as ONE "
                               "image's per-channel affine (mobile_modules.py:10), got batch %d" % seg.shape[0])
        return super()._forward(seg)
