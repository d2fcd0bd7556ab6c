"""Stable Diffusion's VAE decoder as a sparse workload (the reference's SIGEDecoder: stable-diffusion/ldm/modules/
diffusionmodules/sige_model.py:279, built by ldm/models/sige_autoencoder.py with the `ddconfig` of configs/sige.yaml) on sige_amd.nn.

Module tree and state-dict keys are the reference's (`conv_in`, `mid.{block_1,attn_1,block_2}`, `up.L.block.B.{norm1,conv1,norm2,
conv2,nin_shortcut}`, `up.L.upsample.conv`, `norm_out`, `conv_out`; `mid.attn_1.{norm,q,k,v,proj_out}`), so a checkpoint's
`first_stage_model.decoder.*` loads strictly.  Every level is tiled: residual blocks with cached GroupNorm affines and no timestep
embedding (6x6 tiles for the 3x3 convs, 4x4 for the 1x1 shortcuts), Upsample = Gather(upsample2x) in front of a 3x3 tile conv,
norm_out as a TRUE GroupNorm of the edited activation in front of conv_out.

The attention block (model.py:180-252, SIGEAttnBlock) is single-head attention over ALL channels of the middle block -- 512 in
the real configuration: queries = the tokens of the active 4x4 tiles, keys / values = every position of the scattered K / V
tensors.  In sparse mode on channels-last fp32 GPU tensors:
    gather (cached affine) -> q on the tiles                                      1 launch
    gather -> (k | v), ONE C -> 2C conv whose weight is the derived concatenation of `k` and `v`, written into the persistent
              [B,2C,H,W] tensor that holds the original's K | V outside the active tiles          1 launch
    attention: hip.attention_tokens (C <= 160) or hip.attention_wide (above), q / k / v read in place    1 launch
    proj_out on the tiles, then the scatter with the residual x                   2 launches
`NATIVE_ATTENTION = False` -- and any backend without the fused path: CPU, NCHW -- runs the reference's module chain (bmm, softmax
over a [B,Nq,HW] score tensor, bmm, with its reshapes and copies); a shape the attention entry refuses runs that bmm chain on the
fused q and K | V.  With in-place scatters (SIGEModel.set_scatter_inplace) the persistent K | V tensor and the attention's output rows
are allocated by set_masks() / set_mode(), never inside a forward; without, every Scatter returns a fresh tensor as the reference's does.  Batch 1 (the reference's sparse mode calls scale.view(1, -1, 1, 1): one cached original).

Stacked edits (sige_amd/stacked.py): under `stacked.edit_batch(model, E)` both models take [E, ...] inputs in sparse
mode -- the first conv at batch E, every block on the tall image [1,C,E*H,W], the tail per image at batch E again -- and the
attention is hip.attention_wide(tiles=...): the queries of an edit's tiles against THAT edit's H * W keys, one launch for all E
edits.  What has no per-image form (C <= 160, NATIVE_ATTENTION off, NCHW, CPU, sparse_update, a shape the entry refuses) raises a
RuntimeError that names stacked edits: the chain would softmax over the keys of all E images.

The f16 compute mode (SIGEModel.set_compute_dtype("f16")): both models run it on channels-last GPU tensors, sparse
and full.  Every SIGEConv2d on tiles runs the fp16 tile kernels, the derived K | V conv takes its compute dtype from `k` and `v`
(folded_kv()), and the attention launch follows `ATTENTION_COMPUTE` below (hip.attention_wide / attention_tokens, compute="f16").
What has no fp16 form keeps its exact-fp32 kernel in that mode: `conv_in` / `conv_out` with the decoder's conv3x3_small_cout_cl
head, the encoder's latent head (conv_latent_head.hip), the stride-2 Downsample conv (hip.conv_pack_weights packs that geometry for
the exact-fp32 tile conv; the full pass runs it as the torch conv), the GroupNorm statistics, and the torch chain (`_chain`: CPU, NCHW, NATIVE_ATTENTION off,
and the full-mode attention).  The Upsample conv runs as the 9-tap fp16 tile conv: SIGEConv2d.phase_kernels() is None outside f32
(the four-phase form on fp16 operands exists behind Gather.PHASE_UPSAMPLE_TILE3, off by default: DESIGN.md 5.29).
"f16x3" has no attention or tile form of its own: both run exact fp32.

The encoder (SIGEEncoder, sige_model.py:177) is built from the same blocks: SparseVAEEncoder, at the end of the file."""
from dataclasses import dataclass
from typing import Tuple

import torch
from torch import nn
from torch.nn import functional as F

from ..nn import Gather, Scatter, ScatterGather, ScatterWithBlockResidual, SIGEConv2d, SIGEModel, SIGEModule, paired_convs
from ..nn.dense import group_norm_affine, input_conv2d
from .ddpm_unet import Downsample, Upsample, norm_affine
from .pd_unet import _as4, _fused_layout

# The attention launch of the library in the tiled attention block.  False: the reference's bmm / softmax / bmm chain (A/B runs:
# tools/vae_bench.py; tests).
NATIVE_ATTENTION = True
# The latent-head launch of the library (hip.conv3x3_latent_head_cl) as the encoder's tail in sparse mode.  False: the reference's
# chain, conv_out(silu(norm_out(h))) -> quant_conv -> the posterior in torch (A/B runs: tools/vae_encoder_bench.py; tests).
NATIVE_HEAD = True
# The arithmetic of the attention launch: "f32" exact fp32 products, "f16" fp16 operands with fp32 accumulation on the same fp32
# tensors (sige_hip_attention_wide_f16c / sige_hip_attention_tokens_f16c), None: the model's compute policy -- "f16" where the block's
# `q` conv has compute dtype "f16" (set_compute_dtype("f16") without a `keep` prefix naming it), "f32" otherwise ("f16x3" included).
ATTENTION_COMPUTE = None
# precision order of the compute dtypes: the derived K | V conv takes the higher one of `k` and `v`
_PRECISION = {"f16": 0, "f16x3": 1, "f32": 2}


@dataclass
class VAEDecoderConfig:
    """Defaults: configs/sige.yaml, first_stage_config.params.ddconfig."""
    ch: int = 128
    out_ch: int = 3
    ch_mult: Tuple[int, ...] = (1, 2, 4, 4)
    num_res_blocks: int = 2
    attn_resolutions: Tuple[int, ...] = ()
    in_channels: int = 3
    resolution: int = 256
    z_channels: int = 4
    main_block: int = 6      # tile edge of the 3x3 convs
    shortcut_block: int = 4  # tile edge of the 1x1 shortcuts
    attn_block: int = 4      # tile edge of the attention block's 1x1 convs
    groups: int = 32
    eps: float = 1e-6


class VAEResBlock(SIGEModule):
    """SIGEResnetBlock with temb_channels = 0 (sige_model.py:10-139): no temb_proj."""

    def __init__(self, cfg: VAEDecoderConfig, cin: int, cout: int):
        super().__init__()
        self.cin, self.cout = cin, cout
        self.norm1 = nn.GroupNorm(cfg.groups, cin, eps=cfg.eps)
        self.conv1 = SIGEConv2d(cin, cout, 3, 1, 1)
        self.norm2 = nn.GroupNorm(cfg.groups, cout, eps=cfg.eps)
        self.conv2 = SIGEConv2d(cout, cout, 3, 1, 1)
        self.main_gather = Gather(self.conv1, cfg.main_block, activation_name="swish")
        self.scatter_gather = ScatterGather(self.main_gather, activation_name="swish")
        if cin != cout:
            self.nin_shortcut = SIGEConv2d(cin, cout, 1, 1, 0)
            self.shortcut_gather = Gather(self.nin_shortcut, cfg.shortcut_block)
            self.scatter = ScatterWithBlockResidual(self.main_gather, self.shortcut_gather)
        else:
            self.scatter = Scatter(self.main_gather)
        self.affine = {}  # cache_id -> (scale1, shift1, scale2, shift2) as [1,C,1,1]
        self.plain = False

    def clear_cache(self):
        self.affine = {}

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.mode == "full" and self.plain:
            # the stock dense block (model.py:119-139): F.group_norm, no cache bookkeeping
            h = self.conv1(F.silu(self.norm1(x)))
            h = self.conv2(F.silu(self.norm2(h)))
            return (x if self.cin == self.cout else self.nin_shortcut(x)) + h
        if self.mode == "full":
            skip = x if self.cin == self.cout else self.nin_shortcut(self.shortcut_gather(x))
            h = self.main_gather(x)  # records the input resolution
            s1, t1 = norm_affine(h, self.norm1)
            h = self.scatter_gather(self.conv1(F.silu(h * _as4(s1) + _as4(t1))))
            s2, t2 = norm_affine(h, self.norm2)
            self.affine[self.cache_id] = tuple(_as4(v).contiguous() for v in (s1, t1, s2, t2))
            return self.scatter(self.conv2(F.silu(h * _as4(s2) + _as4(t2))), skip)
        if self.mode in ("sparse", "profile"):
            s1, t1, s2, t2 = self.affine[self.cache_id]
            # (channels-last GPU tensors: the 1x1 shortcut rides in conv1's launch, conv2 + scatter + residual are one launch)
            with paired_convs(x, enabled=self.cin != self.cout and self.mode == "sparse", main=getattr(self, "main_gather", None)):
                skip = x if self.cin == self.cout else self.nin_shortcut(self.shortcut_gather(x))
                h = self.conv1(self.main_gather(x, s1, t1))
            tiles = self.scatter_gather(h, s2, t2)
            if self.mode == "sparse":
                return self.scatter.forward_fused(self.conv2, tiles, skip)
            return self.scatter(self.conv2(tiles), skip)
        raise NotImplementedError("Unknown mode [%s]!!!" % self.mode)


class VAEAttnBlock(SIGEModule):
    """SIGEAttnBlock (model.py:180-252)."""

    def __init__(self, cfg: VAEDecoderConfig, ch: int):
        super().__init__()
        self.ch, self.block = ch, cfg.attn_block
        self.norm = nn.GroupNorm(cfg.groups, ch, eps=cfg.eps)
        self.q = SIGEConv2d(ch, ch, 1, 1, 0)
        self.k = SIGEConv2d(ch, ch, 1, 1, 0)
        self.v = SIGEConv2d(ch, ch, 1, 1, 0)
        self.proj_out = SIGEConv2d(ch, ch, 1, 1, 0)
        self.gather = Gather(self.q, cfg.attn_block)
        self.k_scatter = Scatter(self.gather)
        self.v_scatter = Scatter(self.gather)
        self.out_scatter = Scatter(self.gather)
        # (not in the reference; no parameters: the state dict keeps its keys) K | V as ONE [B,2C,H,W] tensor: cache + persistent output
        self.kv_scatter = Scatter(self.gather)
        self.affine = {}      # cache_id -> (scale, shift) as [1,C,1,1]
        self._attn_out = None  # [1, 16 * active tiles, C]: the attention launch's output rows (alloc_buffers)
        self.plain = False
        self.edit_batch = 1    # stacked edits (sige_amd/stacked.py: `with stacked.edit_batch(model, E)`)

    def clear_cache(self):
        self.affine = {}
        self._attn_out = None
        self.__dict__.pop("_kv_conv", None)

    # ---- derived: the C -> 2C conv (k | v) ------------------------------------------------------------------------------------
    def folded_kv(self) -> SIGEConv2d:
        """The 1x1 conv with outputs (k(x) | v(x)): the weights and biases of `k` and `v` concatenated.  Not a Parameter, a buffer or
        a submodule -- the state dict keeps the reference's keys; rebuilt when a parameter of `k` / `v` has been replaced, moved or
        edited in place (address, version counter, shape, device, dtype: the key of ddpm_unet.AttnBlock.folded_qv) and after
        clear_cache()."""
        params = (self.k.weight, self.k.bias, self.v.weight, self.v.bias)
        key = tuple(None if p is None else (p.data_ptr(), p._version, tuple(p.shape), p.device, p.dtype) for p in params)
        # the compute dtype of `k` and `v` (set_compute_dtype never reaches the derived conv: it is no submodule); where a `keep`
        # prefix names one of the two, the higher precision
        dtype = max((getattr(c, "compute_dtype", "f32") for c in (self.k, self.v)), key=_PRECISION.__getitem__)
        key += (dtype,)
        entry = self.__dict__.get("_kv_conv")
        if entry is not None and entry[0] != key and entry[0][:-1] == key[:-1]:
            # the same weights under another compute dtype: re-labelled (SIGEConv2d keeps one pack per compute form, each keyed
            # on the weight, so no pack of the other form is ever read)
            entry[1].compute_dtype = dtype
            entry = self.__dict__["_kv_conv"] = (key, entry[1])
        if entry is None or entry[0] != key:
            C = self.ch
            with torch.device("meta"):
                conv = SIGEConv2d(C, 2 * C, 1, 1, 0)
            conv.weight = nn.Parameter(torch.cat([self.k.weight.detach(), self.v.weight.detach()]).contiguous(), requires_grad=False)
            conv.bias = nn.Parameter(torch.cat([self.k.bias.detach(), self.v.bias.detach()]).contiguous(), requires_grad=False)
            conv.set_mode("sparse")
            conv.compute_dtype = dtype
            entry = (key, conv)
            self.__dict__["_kv_conv"] = entry  # (not through nn.Module.__setattr__: that would register the conv as a submodule)
        return entry[1]

    # ---- persistent buffers: SparseVAEDecoder.set_masks / set_mode -----------------------------------------------------------------
    def _fused_cache(self):
        kv = self.kv_scatter.original_outputs.get(self.cache_id)
        return kv if kv is not None and _fused_layout(kv) else None

    def alloc_buffers(self):
        """Outside any forward (a forward may run under a graph capture): the persistent K | V tensor of the current cache id --
        the original's K | V, restored in place when only the mask changed -- and the attention's output rows for the current
        mask's tile count."""
        kv = self._fused_cache()
        g = self.gather
        if kv is None or g.active_indices is None:
            return
        if self.kv_scatter.inplace:
            self.kv_scatter._out_bufs.get(self.cache_id, kv, g.timestamp)
        self.folded_kv()
        rows = 16 * int(g.active_indices.shape[0]) * kv.shape[0]
        buf = self._attn_out
        if buf is None or buf.shape[1] != rows or buf.device != kv.device:
            self._attn_out = torch.empty((1, rows, self.ch), dtype=torch.float32, device=kv.device)

    def persistent_buffers(self):
        """(tests) [(name, tensor, rewritten)]: `rewritten` = the forward writes every element it later reads -- K | V is rewritten
        on the active tiles only; everywhere else it carries the original's values (a cache)."""
        out = []
        entry = self.kv_scatter._out_bufs.bufs.get(self.cache_id)
        if entry is not None:
            out.append(("kv", entry[1], False))
        if self._attn_out is not None:
            out.append(("attn_out", self._attn_out, True))
        return out

    # ---- the reference's attention (model.py:218-247) ---------------------------------------------------------------------------
    def _chain(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        """q [b,nq,c] tokens, k / v [b,c,h,w] -> [b,c,nq]."""
        b, c, h, w = k.shape
        w_ = torch.bmm(q, k.reshape(b, c, h * w)) * (int(c) ** (-0.5))
        w_ = F.softmax(w_, dim=2)
        return torch.bmm(v.reshape(b, c, h * w), w_.permute(0, 2, 1))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.mode == "full" and self.plain:
            # the stock dense block (model.py:153-177)
            h = self.norm(x)
            q, k, v = self.q(h), self.k(h), self.v(h)
            b, c, hh, ww = q.shape
            h = self._chain(q.reshape(b, c, hh * ww).permute(0, 2, 1), k, v).reshape(b, c, hh, ww)
            return x + self.proj_out(h)
        if self.mode == "full":
            h = self.gather(x)
            s, t = norm_affine(h, self.norm)
            self.affine[self.cache_id] = (_as4(s).contiguous(), _as4(t).contiguous())
            h = h * _as4(s) + _as4(t)
            q = self.q(h)
            k, v = self.k_scatter(self.k(h)), self.v_scatter(self.v(h))
            if _fused_layout(x):
                self.kv_scatter(torch.cat([k, v], dim=1).contiguous(memory_format=torch.channels_last))
            b, c, hh, ww = q.shape
            h = self._chain(q.reshape(b, c, hh * ww).permute(0, 2, 1), k, v).reshape(b, c, hh, ww)
            if _fused_layout(x) and getattr(self.proj_out, "compute_dtype", "f32") != "f32":
                # the chain's output is NCHW; the library's full-pass conv (f16 / f16x3) keeps its input's layout, and an NCHW
                # cache behind out_scatter would send every later block down the exact-fp32 NCHW route, in both passes
                h = h.contiguous(memory_format=torch.channels_last)
            return self.out_scatter(self.proj_out(h), x)
        if self.mode not in ("sparse", "profile"):
            raise NotImplementedError("Unknown mode [%s]!!!" % self.mode)
        s, t = self.affine[self.cache_id]
        stacked = self._stacked(x)
        if stacked and not (self.mode == "sparse" and NATIVE_ATTENTION and _fused_layout(x) and x.shape[0] == 1):
            # (the chain below would softmax over the keys of all E images: a wrong answer, not an error)
            self._refuse_stacked("sparse mode with NATIVE_ATTENTION on the channels-last fp32 GPU tall tensor [1,C,E*H,W]")
        if self.mode == "sparse" and NATIVE_ATTENTION and _fused_layout(x) and x.shape[0] == 1:
            out = self._sparse_fused(x, s, t, stacked)
            if out is not None:
                return out
        # the reference's module chain: CPU, NCHW, NATIVE_ATTENTION off
        tiles = self.gather(x, s, t)
        q = self.q(tiles)  # [b * nb, c, bh, bw]
        k, v = self.k_scatter(self.k(tiles)), self.v_scatter(self.v(tiles))
        b, c, bs = x.size(0), q.shape[1], self.block
        q = q.reshape(b, -1, c, bs * bs).permute(0, 1, 3, 2).reshape(b, -1, c)  # [b, nb * hw, c]
        h = self._chain(q, k, v)  # [b, c, nb * hw]
        h = h.reshape(b, c, -1, bs, bs).permute(0, 2, 1, 3, 4).reshape(-1, c, bs, bs)
        return self.out_scatter(self.proj_out(h), x)

    # ---- stacked edits (sige_amd/stacked.py) ---------------------------------------------------------------------------------------
    def _stacked(self, x) -> bool:
        if self.edit_batch > 1:
            return True
        if not x.is_cuda:
            return False
        from .. import hip

        return hip.get_edit_batch() > 1

    def _refuse_stacked(self, needs: str):
        raise RuntimeError("VAEAttnBlock: stacked edits attend per image -- the queries of an edit's tiles against that edit's own "
                           "keys --, which only hip.attention_wide(tiles=...) does: %s (this block has %d channels)" % (needs, self.ch))

    def attention_compute(self) -> str:
        """ "f32" | "f16": `ATTENTION_COMPUTE`, or under None the compute policy as it reached `q`."""
        compute = ATTENTION_COMPUTE
        if compute is None:
            compute = "f16" if getattr(self.q, "compute_dtype", "f32") == "f16" else "f32"
        if compute not in ("f32", "f16"):
            raise ValueError("sd_vae.ATTENTION_COMPUTE must be None, 'f32' or 'f16', got %r" % (compute,))
        return compute

    def _sparse_fused(self, x, s, t, stacked=False):
        """None: no fused form as things stand (the caller runs the module chain).  `stacked`: x is the tall image of E edits
        (hip.set_edit_batch) and there is no chain to fall back to -- whatever has no per-image form raises."""
        from .. import hip

        kv_cache = self._fused_cache()
        C, g = self.ch, self.gather
        if stacked:
            if C <= 160:
                self._refuse_stacked("more than 160 channels (hip.attention_tokens has no per-image form)")
            if kv_cache is None or C % 4 or self.sparse_update:
                self._refuse_stacked("a channels-last K | V cache of the full pass, channels a multiple of 4, no sparse_update")
        if kv_cache is None or C % 4 or self.sparse_update:
            return None
        T = int(g.active_indices.shape[0])
        if T == 0:
            return None  # (no query: the chain has nothing to attend with, under stacked edits too)
        q = self.q(self.gather(x, s, t))  # [T,C,4,4] channels-last tiles = the token matrix [16 T, C]
        kv = self.kv_scatter.forward_fused(self.folded_kv(), self.gather(x, s, t))  # persistent [1,2C,H,W]: new K | V on the tiles
        if not (hip.is_cl(q) and hip.is_cl(kv)):
            if stacked:
                self._refuse_stacked("channels-last tiles and K | V")
            return None
        _, _, H, W = kv.shape
        qt = q.permute(0, 2, 3, 1).reshape(1, 16 * T, C)            # (views: no copy on either side)
        tok = kv.permute(0, 2, 3, 1).reshape(1, H * W, 2 * C)
        scale = int(C) ** (-0.5)
        compute = self.attention_compute()
        if C <= 160:
            o = hip.attention_tokens(qt, tok[:, :, :C], tok[:, :, C:], 1, scale, compute=compute)
        else:
            buf = self._attn_out
            if buf is None or buf.shape[1] != 16 * T or buf.device != x.device:
                # (not reached after set_masks() / set_mode(): only a block driven module by module allocates here)
                buf = self._attn_out = torch.empty((1, 16 * T, C), dtype=torch.float32, device=x.device)
            # stacked edits: kv is the tall image; tile t's keys are the rows of the image its origin row lies in, found inside the launch
            o = hip.attention_wide(qt, tok[:, :, :C], tok[:, :, C:], 1, scale, out=buf,
                                   tiles=(g.active_indices, H, W) if stacked else None, compute=compute)
        if o is None and stacked:
            self._refuse_stacked("a shape sige_hip_attention_wide_tiles_f32 / _f16c takes (one image's height a power of two >= 4; K | V is "
                                 "%d x %d for the whole edit batch)" % (H, W))
        if o is None:
            # a shape the entry does not take: the reference's bmm chain on the fused q and K | V (fp32 in every compute mode)
            o = self._chain(qt, kv[:, :C], kv[:, C:]).permute(0, 2, 1)
        h = o.reshape(T, 4, 4, C).permute(0, 3, 1, 2)  # channels-last tiles again
        return self.out_scatter(self.proj_out(h), x)


def _enter_stacked(model, x, h, E: int):
    """Stacked edits (sige_amd/stacked.py): x is [E,c,H,W], h = conv_in(x) a whole-image op at batch E; from here to the output norm
    every tensor is the tall image [1,C,E*H,W] -- the same bytes -- and every sparse module works on it unchanged."""
    if model.mode != "sparse" or x.shape[0] != E:
        raise RuntimeError("stacked edits: sparse mode, one input image per edit (edit batch %d, mode %r, input batch %d)"
                           % (E, model.mode, x.shape[0]))
    if not _fused_layout(h):
        raise RuntimeError("stacked edits: channels-last fp32 GPU tensors only")
    from ..stacked import tall

    return tall(h)


def _leave_stacked(h, E: int):
    """The tall image back as [E,C,H,W] (the same bytes) for the per-image tail."""
    from ..stacked import untall

    return untall(h, E)


class SparseVAEDecoder(SIGEModel):
    # set_compute_dtype("f16"): no conv stays at the higher precision, at any edit size.  tests/vae_f16.py's per-layer trace on
    # name-initialised weights (profiles/sd_vae_f16_error_trace.json): the worst element is at 0.012 of the f16
    # criterion's allowance with every conv and the attention in plain fp16 (1.2 - 15 % edits, both sizes).
    F16_KEEP = ()
    F16_KEEP_ABOVE = 0.0

    def __init__(self, cfg: VAEDecoderConfig = VAEDecoderConfig()):
        super().__init__()
        self.cfg = cfg
        self.edit_batch = 1  # stacked edits (sige_amd/stacked.py: `with stacked.edit_batch(model, E)`)
        ch, mult = cfg.ch, tuple(cfg.ch_mult)
        self.num_resolutions, self.num_res_blocks = len(mult), cfg.num_res_blocks
        cur = ch * mult[-1]
        res = cfg.resolution // 2 ** (self.num_resolutions - 1)
        self.z_shape = (1, cfg.z_channels, res, res)

        self.conv_in = nn.Conv2d(cfg.z_channels, cur, 3, 1, 1)
        self.mid = nn.Module()
        self.mid.block_1 = VAEResBlock(cfg, cur, cur)
        self.mid.attn_1 = VAEAttnBlock(cfg, cur)
        self.mid.block_2 = VAEResBlock(cfg, cur, cur)

        ups = []
        for lvl in reversed(range(self.num_resolutions)):
            stage = nn.Module()
            stage.block, stage.attn = nn.ModuleList(), nn.ModuleList()
            cout = ch * mult[lvl]
            for _ in range(cfg.num_res_blocks + 1):
                stage.block.append(VAEResBlock(cfg, cur, cout))
                cur = cout
                if res in cfg.attn_resolutions:
                    stage.attn.append(VAEAttnBlock(cfg, cur))
            if lvl != 0:
                stage.upsample = Upsample(cfg, cur)
                res *= 2
            ups.insert(0, stage)
        self.up = nn.ModuleList(ups)

        self.norm_out = nn.GroupNorm(cfg.groups, cur, eps=cfg.eps)
        self.conv_out = nn.Conv2d(cur, cfg.out_ch, 3, 1, 1)

    # ---- bookkeeping -------------------------------------------------------------------------------------------------------------
    def _attn_blocks(self):
        return [m for m in self.modules() if isinstance(m, VAEAttnBlock)]

    def _alloc_buffers(self):
        for m in self._attn_blocks():
            m.alloc_buffers()

    def persistent_buffers(self):
        """(tests) every persistent buffer the attention blocks own: [(name, tensor, rewritten)], see VAEAttnBlock."""
        return [(name, buf, rw) for m in self._attn_blocks() for name, buf, rw in m.persistent_buffers()]

    def set_plain_dense(self, plain: bool):
        """full mode = the stock dense decoder (F.group_norm, no cache bookkeeping): what a speedup is quoted against."""
        for m in self.modules():
            if isinstance(m, (VAEResBlock, VAEAttnBlock, Upsample)):
                m.plain = plain

    def set_masks(self, masks):
        super().set_masks(masks)
        self._alloc_buffers()

    def set_mode(self, mode: str):
        super().set_mode(mode)
        if mode == "sparse":
            self._alloc_buffers()

    def set_cache_id(self, cache_id: int):
        super().set_cache_id(cache_id)
        if self.mode == "sparse":
            self._alloc_buffers()

    # ---- forward -----------------------------------------------------------------------------------------------------------------
    def _head(self, h):
        """norm_out is a TRUE GroupNorm of the edited activation (sige_model.py:386-388)."""
        if self.mode == "sparse" and _fused_layout(h) and h.shape[1] % 4 == 0:
            from .. import hip

            so, to = group_norm_affine(h, self.norm_out)
            out = hip.conv3x3_small_cout_cl(h, self.conv_out.weight, self.conv_out.bias, so, to, "swish")
            if out is not None:
                return out
        return self.conv_out(F.silu(self.norm_out(h)))

    def forward(self, z: torch.Tensor) -> torch.Tensor:
        h = self.conv_in(z)
        if z.is_contiguous(memory_format=torch.channels_last) and not z.is_contiguous():
            h = h.contiguous(memory_format=torch.channels_last)  # (MIOpen may hand back NCHW for 4 input channels)
        E = self.edit_batch
        if E > 1:
            h = _enter_stacked(self, z, h, E)
        h = self.mid.block_1(h)
        h = self.mid.attn_1(h)
        h = self.mid.block_2(h)
        for lvl in reversed(range(self.num_resolutions)):
            stage = self.up[lvl]
            for i, block in enumerate(stage.block):
                h = block(h)
                if len(stage.attn):
                    h = stage.attn[i](h)
            if lvl != 0:
                h = stage.upsample(h)
        if E > 1:
            h = _leave_stacked(h, E)  # (norm_out and conv_out are per image: [E,C,1,1] affines at B = E)
        return self._head(h)


# ---- the encoder (sige_model.py:177-276, SIGEEncoder) ------------------------------------------------------------------------------
@dataclass
class VAEEncoderConfig:
    """Defaults: configs/sige.yaml, first_stage_config.params.ddconfig (with its double_z)."""
    ch: int = 128
    out_ch: int = 3
    ch_mult: Tuple[int, ...] = (1, 2, 4, 4)
    num_res_blocks: int = 2
    attn_resolutions: Tuple[int, ...] = ()
    in_channels: int = 3
    resolution: int = 256
    z_channels: int = 4
    double_z: bool = True
    main_block: int = 6
    shortcut_block: int = 4
    attn_block: int = 4
    groups: int = 32
    eps: float = 1e-6


class SparseVAEEncoder(SIGEModel):
    """Stable Diffusion's VAE encoder as a sparse workload: the SDEdit runner encodes the original image in full mode once and every
    edited image in sparse mode under the edit's masks (runners/sdedit_runner.py:54-62).  Module tree and state-dict keys are the
    reference's (`conv_in`, `down.L.block.B.*`, `down.L.attn.*`, `down.L.downsample.conv`, `mid.{block_1,attn_1,block_2}`,
    `norm_out`, `conv_out`): a checkpoint's `first_stage_model.encoder.*` loads strictly.  Every level is tiled -- the decoder's
    residual and attention blocks, Downsample = Gather in front of a stride-2 tile conv whose zero fill is the (0,1,0,1) padding.

    The tail, norm_out -> SiLU -> conv_out and the autoencoder's 1x1 `quant_conv` behind it, is dense in every mode (norm_out is a
    TRUE GroupNorm of the edited activation).  In sparse mode on channels-last fp32 GPU tensors it is group_norm_affine + ONE
    launch of hip.conv3x3_latent_head_cl: quant_conv is folded into conv_out's weights (no nonlinearity between them) and the
    posterior sample rides in the launch's epilogue.  `NATIVE_HEAD = False`, CPU, NCHW and shapes the entry refuses run the
    reference's chain.  Batch 1 in sparse mode, as the decoder."""

    # set_compute_dtype("f16"): no conv stays at the higher precision, at any edit size.  tests/vae_f16.py's per-layer trace on
    # name-initialised weights (profiles/sd_vae_f16_error_trace.json): the worst element is at 0.005 of the f16
    # criterion's allowance with every conv and the attention in plain fp16 (1.2 - 15 % edits, both sizes).
    F16_KEEP = ()
    F16_KEEP_ABOVE = 0.0

    def __init__(self, cfg: VAEEncoderConfig = VAEEncoderConfig()):
        super().__init__()
        self.cfg = cfg
        ch, mult = cfg.ch, tuple(cfg.ch_mult)
        self.num_resolutions, self.num_res_blocks = len(mult), cfg.num_res_blocks
        self.conv_in = nn.Conv2d(cfg.in_channels, ch, 3, 1, 1)
        in_mult = (1,) + mult
        res, cur = cfg.resolution, ch
        self.down = nn.ModuleList()
        for lvl in range(self.num_resolutions):
            stage = nn.Module()
            stage.block, stage.attn = nn.ModuleList(), nn.ModuleList()
            cur, cout = ch * in_mult[lvl], ch * mult[lvl]
            for _ in range(cfg.num_res_blocks):
                stage.block.append(VAEResBlock(cfg, cur, cout))
                cur = cout
                if res in cfg.attn_resolutions:
                    stage.attn.append(VAEAttnBlock(cfg, cur))
            if lvl != self.num_resolutions - 1:
                stage.downsample = Downsample(cfg, cur, sparse=True)
                res //= 2
            self.down.append(stage)
        self.mid = nn.Module()
        self.mid.block_1 = VAEResBlock(cfg, cur, cur)
        self.mid.attn_1 = VAEAttnBlock(cfg, cur)
        self.mid.block_2 = VAEResBlock(cfg, cur, cur)
        self.norm_out = nn.GroupNorm(cfg.groups, cur, eps=cfg.eps)
        self.conv_out = nn.Conv2d(cur, 2 * cfg.z_channels if cfg.double_z else cfg.z_channels, 3, 1, 1)
        self._h0_buf = None  # conv_in's output on the active windows (alloc_buffers)
        self.edit_batch = 1  # stacked edits (sige_amd/stacked.py: `with stacked.edit_batch(model, E)`)

    # ---- bookkeeping: as SparseVAEDecoder ----------------------------------------------------------------------------------------
    def _attn_blocks(self):
        return [m for m in self.modules() if isinstance(m, VAEAttnBlock)]

    def _conv_in_windows(self):
        """The Gather whose windows are all a sparse forward reads of hs[0] = conv_in(x), or None (conv_in runs densely).  The
        encoder has no skip connections (sige_model.py:256-264): hs[0] goes to down[0].block[0] alone.  With cin == cout that block
        reads it through `main_gather` and, as the residual, through `scatter` = Scatter(main_gather) -- one index list, the
        residual inside the windows' 4x4 output blocks.  With cin != cout `shortcut_gather` reads it under a second index list:
        dense then."""
        first = self.down[0].block[0]
        g = first.main_gather
        if first.cin != first.cout or not isinstance(first.scatter, Scatter) or first.scatter.gather.module is not g:
            return None
        if g.active_indices is None or g.input_res is None or tuple(g.model_stride) != (1, 1):
            return None
        return g

    def _alloc_buffers(self):
        for m in self._attn_blocks():
            m.alloc_buffers()
        g = self._conv_in_windows()
        if self.__dict__.get("_sige_stacked"):
            g = None  # (stacked caches: conv_in is a whole-image op at batch E, the window form is for single edits)
        if g is not None and g.active_indices.is_cuda:
            shape = (1, self.conv_in.out_channels) + tuple(g.input_res)
            buf = self._h0_buf
            if buf is None or tuple(buf.shape) != shape or buf.device != g.active_indices.device:
                self._h0_buf = torch.zeros(shape, dtype=torch.float32, device=g.active_indices.device).contiguous(memory_format=torch.channels_last)

    def persistent_buffers(self):
        """(tests) [(name, tensor, rewritten)], see VAEAttnBlock; `conv_in`: the first conv's output, written on the active windows
        of down[0].block[0] and read nowhere else."""
        out = [(name, buf, rw) for m in self._attn_blocks() for name, buf, rw in m.persistent_buffers()]
        if self._h0_buf is not None:
            out.append(("conv_in", self._h0_buf, True))
        return out

    def clear_cache(self):
        super().clear_cache()
        self._h0_buf = None
        self.__dict__.pop("_head_fold", None)

    def set_plain_dense(self, plain: bool):
        """full mode = the stock dense encoder (F.group_norm, no cache bookkeeping): what a speedup is quoted against."""
        for m in self.modules():
            if isinstance(m, (VAEResBlock, VAEAttnBlock, Downsample)):
                m.plain = plain

    def set_masks(self, masks):
        super().set_masks(masks)
        self._alloc_buffers()

    def set_mode(self, mode: str):
        super().set_mode(mode)
        if mode == "sparse":
            self._alloc_buffers()

    def set_cache_id(self, cache_id: int):
        super().set_cache_id(cache_id)
        if self.mode == "sparse":
            self._alloc_buffers()

    # ---- derived: conv_out with quant_conv folded in ----------------------------------------------------------------------------
    def folded_head(self, quant_conv: nn.Conv2d):
        """(weight [2z,C,3,3], bias [2z]) of quant_conv(conv_out(.)): W' = Wq Wc, b' = Wq bc + bq, products in fp64.  Not a
        Parameter or a buffer -- the state dict keeps the reference's keys; rebuilt when one of the four parameters has been
        replaced, moved or edited in place (the key of VAEAttnBlock.folded_kv) and after clear_cache()."""
        params = (self.conv_out.weight, self.conv_out.bias, quant_conv.weight, quant_conv.bias)
        key = tuple(None if p is None else (p.data_ptr(), p._version, tuple(p.shape), p.device, p.dtype) for p in params)
        entry = self.__dict__.get("_head_fold")
        if entry is None or entry[0] != key:
            with torch.no_grad():
                wq = quant_conv.weight.detach().double().flatten(1)  # [2z, 2z]
                wc, bc = self.conv_out.weight.detach().double(), self.conv_out.bias.detach().double()
                w = torch.einsum("oi,ichw->ochw", wq, wc)
                b = wq @ bc
                if quant_conv.bias is not None:
                    b = b + quant_conv.bias.detach().double()
                entry = (key, w.float().contiguous(), b.float().contiguous())
            self.__dict__["_head_fold"] = entry
        return entry[1], entry[2]

    # ---- forward -----------------------------------------------------------------------------------------------------------------
    def _conv_in(self, x):
        if self.mode != "sparse":
            h = self.conv_in(x)
        else:
            g, buf = self._conv_in_windows(), self._h0_buf
            if (g is not None and buf is not None and x.is_cuda and x.shape[0] == 1 and tuple(buf.shape[2:]) == tuple(x.shape[2:])
                    and buf.device == x.device):
                h = input_conv2d(self.conv_in, x, tiles=(g.active_indices, tuple(g.block_size)), out=buf)
            else:
                h = input_conv2d(self.conv_in, x)
        if x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous():
            h = h.contiguous(memory_format=torch.channels_last)  # (MIOpen may hand back NCHW for 3 input channels)
        return h

    def _body(self, x):
        h = self._conv_in(x)
        E = self.edit_batch
        if E > 1:
            h = _enter_stacked(self, x, h, E)
        for lvl in range(self.num_resolutions):
            stage = self.down[lvl]
            for i, block in enumerate(stage.block):
                h = block(h)
                if len(stage.attn):
                    h = stage.attn[i](h)
            if lvl != self.num_resolutions - 1:
                h = stage.downsample(h)
        h = self.mid.block_1(h)
        h = self.mid.attn_1(h)
        h = self.mid.block_2(h)
        return _leave_stacked(h, E) if E > 1 else h  # (the tail is per image: [E,C,1,1] affines, [E,z,h,w] noise, at B = E)

    def _tail(self, h, quant_conv=None, posterior=False, noise=None, scale_factor=1.0):
        """norm_out (a TRUE GroupNorm of the edited activation, sige_model.py:272-275) -> SiLU -> conv_out [-> quant_conv [-> the
        posterior]].  Returns the moments, or (moments, z)."""
        if (NATIVE_HEAD and self.mode == "sparse" and _fused_layout(h) and (quant_conv is None or
                (tuple(quant_conv.kernel_size) == (1, 1) and quant_conv.groups == 1 and quant_conv.in_channels == self.conv_out.out_channels))):
            from .. import hip

            w, b = (self.conv_out.weight, self.conv_out.bias) if quant_conv is None else self.folded_head(quant_conv)
            if noise is not None:
                noise = noise.to(h.device, torch.float32)
            so, to = group_norm_affine(h, self.norm_out)
            out = hip.conv3x3_latent_head_cl(h, w, b, so, to, "swish", noise=noise, latent_scale=scale_factor if posterior else None)
            if out is not None:
                return out
        m = self.conv_out(F.silu(self.norm_out(h)))
        if quant_conv is not None:
            m = quant_conv(m)
        if not posterior:
            return m
        # DiagonalGaussianDistribution (ldm/modules/distributions/distributions.py:24-44): sample() or, without noise, mode()
        mean, logvar = torch.chunk(m, 2, dim=1)
        z = mean if noise is None else mean + torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * noise.to(m.device, m.dtype)
        return m, scale_factor * z

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """[B, 2z, H/8, W/8]: the reference encoder's output."""
        return self._tail(self._body(x))

    def moments(self, x: torch.Tensor, quant_conv: nn.Conv2d) -> torch.Tensor:
        """quant_conv(forward(x)): the parameters of the posterior (SIGEAutoencoderKL.encode up to the distribution)."""
        return self._tail(self._body(x), quant_conv)

    def encode(self, x: torch.Tensor, quant_conv: nn.Conv2d, noise=None, scale_factor: float = 0.18215):
        """(moments, z): z = scale_factor * posterior.sample() with the caller's `noise` [B,z,H/8,W/8] (get_first_stage_encoding),
        or scale_factor * posterior.mode() with noise=None."""
        return self._tail(self._body(x), quant_conv, True, noise, scale_factor)
