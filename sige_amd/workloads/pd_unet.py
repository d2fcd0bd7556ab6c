"""Progressive Distillation U-Net workload (LSUN-Church configurations church_pd128-sige.yml / church_pd256-sige.yml of the
reference: diffusion/models/pd_arch/sige_unet.py) built on sige_amd.nn.

Module tree and state-dict keys are those of the reference's SIGEUNet (`temb.dense.{0,1}`, `conv_in`,
`down.L.block.B.{norm1,conv1,temb_proj,norm2,conv2,nin_shortcut}`, `down.L.attn.B.{norm,qkv,proj_out}`, `down.L.downsample.*`,
`mid.{block_1,attn_1,block_2}`, `up.L.{block,attn,upsample}`, `norm_out`, `conv_out`), so a reference checkpoint loads as it
stands.  What differs from the DDPM workload:

  * the residual blocks RESAMPLE INSIDE the block (`resample="down" | "up"`): the activated norm-1 output is average-pooled or
    nearest-upsampled before conv1, and the shortcut is the resampled raw input.  Average pooling does not commute with SiLU,
    so in a sparse pass each gathered pixel of a "down" block needs four activated source pixels -- one launch of
    hip.resample_tiles gives conv1's pre-activated input tiles AND the pooled shortcut on the active cells ("up": the
    activation commutes with nearest x2, conv1 reads the half-resolution tensor through Gather(upsample2x=True), the kernel
    writes the shortcut cells).  The shortcut lives in a persistent buffer per block: outside the active cells of the current
    mask it is STALE, and the fused conv2 + scatter + residual launch never reads it there;
  * the timestep embedding enters as a scale-shift AFTER norm-2, folded into the cached affine:
    scale2 = (1 + emb_scale) * scale, shift2 = (1 + emb_scale) * shift + emb_shift (sige_unet.py:113-120);
  * multi-head attention (head_dim 64) at the dense levels: the cached affine in the qkv 1x1 conv, then ONE
    hip.attention_tokens launch over the token view of the channels-last tensor, then proj_out with the residual.

On the CPU, in NCHW and on any backend without the fused channels-last path every block runs the reference's expression order
(affine -> swish -> avg_pool2d / interpolate -> gather).

Stacked edits (sige_amd/stacked.py): under `stacked.edit_batch(model, E)` the model takes [E,3,H,W] in sparse mode.
conv_in (image by image, see forward), norm_out and conv_out are whole-image ops on [E,C,H,W]; in between every tensor is the tall image [1,C,E*H,W] and every block runs its fused
launches on it (hip.resample_tiles with the tiles of all E images; attention over the same bytes seen as [E, tokens, 3c], one launch).
There is no chain to fall back to: NCHW, the CPU, FUSED_RESAMPLE = False, a block without a fused form and a shape the attention entry
does not take raise a RuntimeError that names stacked edits."""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch import nn
from torch.nn import functional as F

from ..nn import Gather, Scatter, ScatterGather, ScatterWithBlockResidual, SIGEConv2d, SIGEModel, SIGEModule, paired_convs
from ..nn.deferred import lazy_cat
from ..nn.dense import full_conv2d, fused_conv2d, group_norm_affine, input_conv2d
from .ddpm_unet import norm_affine, timestep_embedding

# The resampling blocks on hip.resample_tiles (sparse levels: tiles + shortcut cells in one launch; dense levels: the shortcut in
# its whole-tensor form).  False: the torch-op chain of the reference in front of the same convs (A/B runs: tools/pd_bench.py).
FUSED_RESAMPLE = True


@dataclass
class PDConfig:
    """Defaults: church_pd128-sige.yml."""
    image_size: int = 128
    ch: int = 64
    ch_mult: Tuple[int, ...] = (1, 2, 4, 6, 8)
    num_res_blocks: int = 3
    attn_resolutions: Tuple[int, ...] = (8, 16, 32)
    head_dim: Optional[int] = 64
    num_heads: Optional[int] = None
    in_ch: int = 3
    out_ch: int = 6
    temb_ch: int = 768
    logsnr_input_type: str = "inv_cos"
    sparse_resolution_threshold: int = 64
    main_block: Optional[int] = 6       # sige_block_size.normal: tile edge of the 3x3 convs
    shortcut_block: Optional[int] = 4   # sige_block_size.instance: tile edge of the 1x1 shortcuts
    groups: int = 32
    eps: float = 1e-6

    @classmethod
    def pd256(cls) -> "PDConfig":
        """church_pd256-sige.yml."""
        return cls(image_size=256, ch=128, ch_mult=(1, 1, 2, 2, 4, 4), num_res_blocks=3, attn_resolutions=(8, 16, 32),
                   head_dim=64, temb_ch=1024, sparse_resolution_threshold=64)


def _as4(v: torch.Tensor) -> torch.Tensor:
    return v.reshape(1, -1, 1, 1)


def _fused_layout(*ts) -> bool:
    """Channels-last fp32 GPU tensors: where the library's fused launches run."""
    from .. import hip

    return all(t.is_cuda and t.dtype == torch.float32 and hip.is_cl(t) for t in ts)


def _refuse_stacked(who: str, needs: str):
    """Stacked edits (sige_amd/stacked.py) have no chain to fall back to: the torch ops would pool, pad and attend across the seams
    of the tall image.  Whatever has no seam-aware launch raises."""
    raise RuntimeError("%s: stacked edits run on the library's seam-aware launches only -- %s" % (who, needs))


class _per_image:
    """Around the whole-image ops at batch E (norm_out, conv_out): the library sees E separate images, no seams inside them."""

    def __enter__(self):
        from .. import hip

        self.prev = hip.get_edit_batch()
        hip.set_edit_batch(1)

    def __exit__(self, *exc):
        from .. import hip

        hip.set_edit_batch(self.prev)
        return False


class PDResBlock(SIGEModule):
    def __init__(self, cfg: PDConfig, cin: int, cout: int, sparse: bool, resample: Optional[str] = None):
        super().__init__()
        assert resample in (None, "down", "up")
        self.cin, self.cout, self.resample = cin, cout, resample
        self.sparse_main = sparse and cfg.main_block is not None
        Conv = SIGEConv2d if self.sparse_main else nn.Conv2d
        self.norm1 = nn.GroupNorm(cfg.groups, cin, eps=cfg.eps)
        self.conv1 = Conv(cin, cout, 3, 1, 1)
        self.temb_proj = nn.Linear(cfg.temb_ch, 2 * cout)
        self.norm2 = nn.GroupNorm(cfg.groups, cout, eps=cfg.eps)
        self.conv2 = Conv(cout, cout, 3, 1, 1)
        self.sparse_shortcut = False
        if self.sparse_main:
            # (a resampling block gathers the ALREADY activated, resampled tensor: sige_unet.py:54-56)
            self.main_gather = Gather(self.conv1, cfg.main_block, activation_name="swish" if resample is None else "identity")
            self.scatter_gather = ScatterGather(self.main_gather, activation_name="swish")
            if resample == "up":
                # the same windows with the activation in the gather: SiLU commutes with nearest x2, so the fused path reads the
                # half-resolution tensor (upsample2x) and activates what it reads
                self.act_gather = Gather(self.conv1, cfg.main_block, activation_name="swish")
        if cin != cout:
            self.sparse_shortcut = self.sparse_main and cfg.shortcut_block is not None
            self.nin_shortcut = (SIGEConv2d if self.sparse_shortcut else nn.Conv2d)(cin, cout, 1, 1, 0)
            if self.sparse_shortcut:
                self.shortcut_gather = Gather(self.nin_shortcut, cfg.shortcut_block)
                self.scatter = ScatterWithBlockResidual(self.main_gather, self.shortcut_gather)
        if self.sparse_main and not self.sparse_shortcut:
            self.scatter = Scatter(self.main_gather)
        self.affine = {}       # cache_id -> (scale1, shift1, scale2, shift2) as [1,C,1,1]
        self.plain = False
        self.edit_batch = 1    # stacked edits (sige_amd/stacked.py: `with stacked.edit_batch(model, E)`)
        self._res_like = None  # (shape of ONE image, device) of the shortcut buffer of a sparse resampling block, from the full pass
        self._res_buf = None

    def clear_cache(self):
        self.affine = {}

    # ---- the persistent shortcut buffer of a sparse resampling block -----------------------------------------------------------
    def alloc_buffers(self):
        """(PDSparseUNet.set_masks / set_mode) the shortcut buffer of a sparse resampling block, allocated OUTSIDE any forward: a
        forward may run under a graph capture.  Zero-filled once; afterwards stale outside the current mask's cells.  Under
        stacked edits (stacked.set_masks: hip.get_edit_batch() is E) the buffer is the tall image, E times the rows."""
        if self._res_like is None:
            return
        shape, device = self._res_like
        if device.type == "cuda":
            from .. import hip

            shape = (shape[0], shape[1], shape[2] * hip.get_edit_batch(), shape[3])
        buf = self._res_buf
        if buf is None or tuple(buf.shape) != tuple(shape) or buf.device != device:
            self._res_buf = torch.zeros(shape, dtype=torch.float32, device=device).contiguous(memory_format=torch.channels_last)

    def _resample(self, t: torch.Tensor) -> torch.Tensor:
        if self.resample == "down":
            return F.avg_pool2d(t, 2)
        if self.resample == "up":
            return F.interpolate(t, scale_factor=2)
        return t

    def forward(self, x, temb: Optional[torch.Tensor]) -> torch.Tensor:
        """`x` may be a pair (h, skip): the up path's torch.cat."""
        pair = x if isinstance(x, (tuple, list)) else None
        if self.mode == "full":
            if self.edit_batch > 1:
                _refuse_stacked("PDResBlock", "sparse mode (the full pass is one original)")
            return self._full(torch.cat(pair, dim=1) if pair else x, temb)
        if self.mode in ("sparse", "profile"):
            parts = list(pair) if pair else [x]
            if self.mode == "sparse" and _fused_layout(*parts):
                out = self._sparse_fused(parts)
                if out is not None:
                    return out
            if self.edit_batch > 1:
                _refuse_stacked("PDResBlock", "sparse mode on channels-last fp32 GPU tensors, and a fused form of this block "
                                "(resample %r, %d -> %d channels, FUSED_RESAMPLE %s)" % (self.resample, self.cin, self.cout, FUSED_RESAMPLE))
            return self._sparse_chain(torch.cat(pair, dim=1) if pair else x)
        raise NotImplementedError("Unknown mode [%s]!!!" % self.mode)

    # ---- full mode: the cache-producing pass (sige_unet.py:88-129) ---------------------------------------------------------
    def _plain(self, x, temb):
        """Dense forward with stock GroupNorm and no caching (the "original model" a speedup is quoted against)."""
        skip = self._resample(x)
        if self.cin != self.cout:
            skip = nn.Conv2d.forward(self.nin_shortcut, skip)
        h = nn.Conv2d.forward(self.conv1, self._resample(F.silu(self.norm1(x))))
        emb = self.temb_proj(F.silu(temb))
        h = self.norm2(h) * (1 + _as4(emb[0, :self.cout])) + _as4(emb[0, self.cout:])
        return nn.Conv2d.forward(self.conv2, F.silu(h)) + skip

    def _full(self, x, temb):
        if self.plain:
            return self._plain(x, temb)
        skip = self._resample(x)
        if self.cin != self.cout:
            if self.sparse_shortcut:
                skip = self.shortcut_gather(skip)
            skip = full_conv2d(self.nin_shortcut, skip)
        s1, t1 = norm_affine(x, self.norm1)
        h = self._resample(F.silu(x * _as4(s1) + _as4(t1)))
        if self.sparse_main:
            h = self.main_gather(h)  # records the input resolution
            if self.resample == "up":
                self.act_gather.note_full_input(h.shape[2:])
        h = full_conv2d(self.conv1, h)
        if self.sparse_main:
            h = self.scatter_gather(h)
        s2, t2 = norm_affine(h, self.norm2)
        emb = self.temb_proj(F.silu(temb))
        es, eh = emb[0, :self.cout], emb[0, self.cout:]
        s2, t2 = (1 + es) * s2, (1 + es) * t2 + eh  # the scale-shift of the embedding, folded into the cached affine
        self.affine[self.cache_id] = tuple(_as4(v).contiguous() for v in (s1, t1, s2, t2))
        if self.sparse_main:
            if self.resample != "down":
                self.scatter_gather.cache_activated(_as4(s2), _as4(t2))
            if self.resample is not None and _fused_layout(x):
                self._res_like = (tuple(skip.shape), x.device)
        if self.sparse_main and self.sparse_shortcut:
            h = full_conv2d(self.conv2, h, _as4(s2), _as4(t2), "swish")
            return self.scatter(h, skip)
        h = full_conv2d(self.conv2, h, _as4(s2), _as4(t2), "swish", residual=skip)
        return self.scatter(h) if self.sparse_main else h

    # ---- sparse mode, the reference's expression order (sige_unet.py:131-174): CPU, NCHW, FUSED_RESAMPLE off ------------------
    def _sparse_chain(self, x):
        s1, t1, s2, t2 = self.affine[self.cache_id]
        skip = self._resample(x)
        if self.cin != self.cout:
            if self.sparse_shortcut:
                skip = self.shortcut_gather(skip)
            skip = self.nin_shortcut(skip)
        if self.sparse_main and self.resample is None:
            h = self.main_gather(x, s1, t1)
        else:
            h = self._resample(F.silu(x * s1 + t1))
            if self.sparse_main:
                h = self.main_gather(h)
        h = self.conv1(h)
        if not self.sparse_main:
            return self.conv2(F.silu(h * s2 + t2)) + skip
        return self.scatter.forward_fused(self.conv2, self.scatter_gather(h, s2, t2), skip)

    # ---- sparse mode on channels-last GPU tensors ------------------------------------------------------------------------------
    def _sparse_fused(self, parts):
        """None: no fused form for this block as it stands (the caller runs the chain)."""
        from .. import hip

        s1, t1, s2, t2 = self.affine[self.cache_id]
        x = parts[0]
        if self.resample is not None:
            if not FUSED_RESAMPLE or len(parts) != 1 or self.cin != self.cout or x.shape[1] % 4:
                return None
            if not self.sparse_main:
                return self._dense_resample(x, s1, t1, s2, t2)
            g = self.main_gather
            res = self._res_buf
            B, C, H, W = x.shape
            want = (B, C, H // 2, W // 2) if self.resample == "down" else (B, C, 2 * H, 2 * W)
            if self.resample == "down" and (H % 2 or W % 2):
                return None
            if res is None or tuple(res.shape) != want or res.device != x.device:
                # (not reached after set_masks() / set_mode(): only a model driven module by module allocates here)
                self._res_like = ((want[0], want[1], want[2] // hip.get_edit_batch(), want[3]), x.device)
                self.alloc_buffers()
                res = self._res_buf
            idx = g.indices_on(x.device)
            geo = dict(res=res, offset=tuple(g.offset), stride=tuple(g.model_stride), cells=tuple(g.out_tile))
            if self.resample == "down":
                # conv1's tiles, activated then pooled, and the pooled shortcut cells: one launch; conv1 takes plain tiles
                tiles = hip.resample_tiles(x, "down", idx, tuple(g.block_size), s1, t1, **geo)
                h = self.conv1(tiles)
                return self.scatter.forward_fused(self.conv2, self.scatter_gather(h, s2, t2), res)
            if not self.act_gather.fuses_upsample(x, s1, t1):
                return None
            hip.resample_tiles(x, "up", idx, None, **geo)
            h = self.conv1(self.act_gather(x, s1, t1, upsample2x=True), out_affine=(s2, t2, "swish"))
            return self.scatter.forward_fused(self.conv2, self.scatter_gather(h, preactivated=True), res)
        if not self.sparse_main:
            return self._dense(x, parts[1] if len(parts) > 1 else None, s1, t1, s2, t2)
        # a plain tiled block, as the DDPM workload runs it: fused gather (affine + SiLU) -> conv1 with the consumer's affine in its
        # epilogue, scatter_gather of finished values, conv2 + scatter + residual in one launch
        xin = x if len(parts) == 1 else (lazy_cat(parts[0], parts[1]) if self.cin != self.cout else torch.cat(parts, dim=1))
        with paired_convs(x, enabled=self.cin != self.cout and self.sparse_shortcut, main=getattr(self, "main_gather", None)):
            if self.cin == self.cout:
                skip = xin
            elif self.sparse_shortcut:
                skip = self.nin_shortcut(self.shortcut_gather(xin))
            else:
                skip = fused_conv2d(self.nin_shortcut, parts[0], x2=parts[1] if len(parts) > 1 else None)
            h = self.conv1(self.main_gather(xin, s1, t1), out_affine=(s2, t2, "swish"))
        return self.scatter.forward_fused(self.conv2, self.scatter_gather(h, preactivated=True), skip)

    def _dense(self, x, x2, s1, t1, s2, t2):
        """Dense block on the cached affines: 2-3 fused launches (shortcut 1x1, conv1, conv2 + skip)."""
        if self.cin == self.cout:
            skip = x if x2 is None else torch.cat([x, x2], dim=1)
        else:
            skip = fused_conv2d(self.nin_shortcut, x, x2=x2)
        h = fused_conv2d(self.conv1, x, s1, t1, "swish", x2=x2, out_affine=(s2, t2, "swish"))
        return fused_conv2d(self.conv2, h, residual=skip)

    def _dense_resample(self, x, s1, t1, s2, t2):
        """A dense resampling block: the shortcut from the whole-tensor form of the kernel.  "up": the upsampled raw tensor is
        conv1's input as well (the activation commutes: affine + SiLU in the conv's staging path); "down": the pooled
        activation has no fused form at a dense level -- torch's SiLU and pooling over this level's small tensor."""
        from .. import hip

        B, C, H, W = x.shape
        if self.resample == "down":
            if H % 2 or W % 2:
                return None
            res = torch.empty((B, C, H // 2, W // 2), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
            hip.resample_tiles(x, "down", res=res)
            hp = F.avg_pool2d(F.silu(x * s1 + t1), 2)
            h = fused_conv2d(self.conv1, hp, out_affine=(s2, t2, "swish"))
        else:
            res = torch.empty((B, C, 2 * H, 2 * W), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
            hip.resample_tiles(x, "up", res=res)
            h = fused_conv2d(self.conv1, res, s1, t1, "swish", out_affine=(s2, t2, "swish"))
        return fused_conv2d(self.conv2, h, residual=res)


class PDAttnBlock(SIGEModule):
    """Multi-head self-attention over all pixels of a dense level (sige_unet.py:177-266, built without support_sparse)."""

    def __init__(self, cfg: PDConfig, ch: int):
        super().__init__()
        head_dim, heads = cfg.head_dim, cfg.num_heads
        if head_dim is None:
            assert heads is not None and ch % heads == 0
            head_dim = ch // heads
        else:
            assert heads is None and ch % head_dim == 0
            heads = ch // head_dim
        self.ch, self.heads, self.head_dim = ch, heads, head_dim
        self.norm = nn.GroupNorm(cfg.groups, ch, eps=cfg.eps)
        self.qkv = nn.Conv2d(ch, 3 * heads * head_dim, 1, 1, 0)
        self.proj_out = nn.Conv2d(heads * head_dim, ch, 1, 1, 0)
        self.affine = {}
        self.plain = False
        self.edit_batch = 1  # stacked edits (sige_amd/stacked.py): E images stacked along H, attention is per image

    def clear_cache(self):
        self.affine = {}

    def _attention(self, qkv: torch.Tensor) -> torch.Tensor:
        """The reference's chain (sige_unet.py:236-256): qkv[:, :c] are the queries, a head is `head_dim` consecutive channels."""
        nh, hd = self.heads, self.head_dim
        c = nh * hd
        b, _, hh, ww = qkv.shape
        q = qkv[:, :c].reshape(b * nh, hd, hh * ww).permute(0, 2, 1)
        k = qkv[:, c:2 * c].reshape(b * nh, hd, hh * ww)
        v = qkv[:, 2 * c:].reshape(b * nh, hd, hh * ww)
        w_ = F.softmax(torch.bmm(q, k) * (hd ** -0.5), dim=2)
        return torch.bmm(v, w_.permute(0, 2, 1)).reshape(b, c, hh, ww)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.mode == "full":
            if self.plain:
                h = self.norm(x)
            else:
                s, t = norm_affine(x, self.norm)
                self.affine[self.cache_id] = (_as4(s).contiguous(), _as4(t).contiguous())
                h = x * _as4(s) + _as4(t)
            return self.proj_out(self._attention(self.qkv(h))) + x
        if self.mode not in ("sparse", "profile"):
            raise NotImplementedError("Unknown mode [%s]!!!" % self.mode)
        s, t = self.affine[self.cache_id]
        E = self.edit_batch
        if self.mode == "sparse" and _fused_layout(x):
            from .. import hip

            qkv = fused_conv2d(self.qkv, x, s, t, "identity")
            b, _, hh, ww = qkv.shape
            c = self.heads * self.head_dim
            if E > 1 and (b != 1 or hh % E):
                _refuse_stacked("PDAttnBlock", "the tall image of %d edits, got %s" % (E, tuple(x.shape)))
            # stacked edits: the tall image is E images -- tokens attend within their own image: the same bytes as [E, hp W, 3c],
            # the one launch at batch E
            tb, tn = (E, (hh // E) * ww) if E > 1 else (b, hh * ww)
            out = None
            if hip.is_cl(qkv):
                tok = qkv.permute(0, 2, 3, 1).reshape(tb, tn, 3 * c)  # (a view: the channels-last tensor IS the token matrix)
                out = hip.attention_tokens(tok[:, :, :c], tok[:, :, c:2 * c], tok[:, :, 2 * c:], self.heads, self.head_dim ** -0.5)
            if out is not None:
                h = out.reshape(b, hh, ww, c).permute(0, 3, 1, 2)  # (channels-last again, no copy)
            elif E > 1:
                _refuse_stacked("PDAttnBlock", "a shape hip.attention_tokens takes (%d heads of %d, %d tokens per image): the chain "
                                "would attend over the keys of all %d images" % (self.heads, self.head_dim, tn, E))
            else:
                h = self._attention(qkv).contiguous(memory_format=torch.channels_last)
            return fused_conv2d(self.proj_out, h, residual=x)
        if E > 1:
            _refuse_stacked("PDAttnBlock", "sparse mode on channels-last fp32 GPU tensors")
        return self.proj_out(self._attention(self.qkv(x * s + t))) + x


class PDSparseUNet(SIGEModel):
    def __init__(self, cfg: PDConfig = PDConfig()):
        super().__init__()
        self.cfg = cfg
        self.edit_batch = 1  # stacked edits (sige_amd/stacked.py: `with stacked.edit_batch(model, E)`)
        ch, mult = cfg.ch, tuple(cfg.ch_mult)
        self.ch, self.temb_ch = ch, cfg.temb_ch
        self.num_resolutions, self.num_res_blocks = len(mult), cfg.num_res_blocks
        self.resolution = cfg.image_size
        thr = cfg.sparse_resolution_threshold

        self.temb = nn.Module()
        self.temb.dense = nn.ModuleList([nn.Linear(ch, cfg.temb_ch), nn.Linear(cfg.temb_ch, cfg.temb_ch)])
        self.conv_in = nn.Conv2d(cfg.in_ch, ch, 3, 1, 1)

        res = cfg.image_size
        in_mult = (1,) + mult
        self.down = nn.ModuleList()
        cur = ch
        for lvl in range(self.num_resolutions):
            stage = nn.Module()
            stage.block, stage.attn = nn.ModuleList(), nn.ModuleList()
            cur, cout = ch * in_mult[lvl], ch * mult[lvl]
            for _ in range(cfg.num_res_blocks):
                stage.block.append(PDResBlock(cfg, cur, cout, res >= thr))
                cur = cout
                if res in cfg.attn_resolutions:
                    stage.attn.append(PDAttnBlock(cfg, cur))
            if lvl != self.num_resolutions - 1:
                stage.downsample = PDResBlock(cfg, cur, cur, res >= thr, resample="down")
                res //= 2
            self.down.append(stage)

        self.mid = nn.Module()
        self.mid.block_1 = PDResBlock(cfg, cur, cur, res >= thr)
        self.mid.attn_1 = PDAttnBlock(cfg, cur)
        self.mid.block_2 = PDResBlock(cfg, cur, cur, res >= thr)

        ups = []
        for lvl in reversed(range(self.num_resolutions)):
            stage = nn.Module()
            stage.block, stage.attn = nn.ModuleList(), nn.ModuleList()
            cout = ch * mult[lvl]
            for i in range(cfg.num_res_blocks + 1):
                skip = ch * (in_mult[lvl] if i == cfg.num_res_blocks else mult[lvl])
                stage.block.append(PDResBlock(cfg, cur + skip, cout, res >= thr))
                cur = cout
                if res in cfg.attn_resolutions:
                    stage.attn.append(PDAttnBlock(cfg, cur))
            if lvl != 0:
                stage.upsample = PDResBlock(cfg, cur, cout, res >= thr, resample="up")
                res *= 2
            ups.insert(0, stage)
        self.up = nn.ModuleList(ups)

        self.norm_out = nn.GroupNorm(cfg.groups, cur, eps=cfg.eps)
        self.conv_out = nn.Conv2d(cur, cfg.out_ch, 3, 1, 1)

    # ---- bookkeeping -------------------------------------------------------------------------------------------------------------
    def _blocks(self):
        return (m for m in self.modules() if isinstance(m, PDResBlock))

    def _alloc_buffers(self):
        for b in self._blocks():
            b.alloc_buffers()

    def res_buffers(self):
        """The persistent shortcut buffers of the sparse resampling blocks (tests poison them)."""
        return [b._res_buf for b in self._blocks() if b._res_buf is not None]

    def set_masks(self, masks):
        super().set_masks(masks)
        self._alloc_buffers()

    def set_mode(self, mode: str):
        super().set_mode(mode)
        if mode == "sparse":
            self._alloc_buffers()

    def set_plain_dense(self, plain: bool):
        """full mode = the stock dense U-Net (F.group_norm, no cache bookkeeping)."""
        for m in self.modules():
            if isinstance(m, (PDResBlock, PDAttnBlock)):
                m.plain = plain

    # ---- forward -----------------------------------------------------------------------------------------------------------------
    def _temb(self, logsnr: torch.Tensor):
        if self.mode != "full":
            return None  # folded into the cached affines
        kind = self.cfg.logsnr_input_type
        if kind == "sigmoid":
            v = torch.sigmoid(logsnr)
        elif kind == "inv_cos":
            v = torch.arctan(torch.exp(-0.5 * torch.clip(logsnr, -20.0, 20.0))) / (0.5 * math.pi)
        else:
            raise NotImplementedError(kind)
        e = timestep_embedding(v * 1000, self.ch)
        return self.temb.dense[1](F.silu(self.temb.dense[0](e)))

    def _padded_conv_out(self):
        """conv_out with its output channels padded to a multiple of 4 (zero rows): the channels-last launches write 16 bytes
        along C.  Derived, not a Parameter or a submodule; rebuilt when conv_out's weights change."""
        conv = self.conv_out
        key = tuple(None if p is None else (p.data_ptr(), p._version, tuple(p.shape), p.device, p.dtype) for p in (conv.weight, conv.bias))
        entry = self.__dict__.get("_conv_out4")
        if entry is None or entry[0] != key:
            co, pad = conv.out_channels, (-conv.out_channels) % 4
            wide = nn.Conv2d(conv.in_channels, co + pad, 3, 1, 1, bias=conv.bias is not None, device="meta")
            w = torch.cat([conv.weight.detach(), conv.weight.new_zeros((pad,) + tuple(conv.weight.shape[1:]))])
            wide.weight = nn.Parameter(w.contiguous(), requires_grad=False)
            if conv.bias is not None:
                wide.bias = nn.Parameter(torch.cat([conv.bias.detach(), conv.bias.new_zeros(pad)]), requires_grad=False)
            entry = (key, wide)
            self.__dict__["_conv_out4"] = entry
        return entry[1]

    def _head(self, h):
        """norm_out is a TRUE GroupNorm of the edited activation (sige_unet.py:469-471)."""
        if self.mode == "sparse" and _fused_layout(h) and h.shape[1] % 4 == 0:
            so, to = group_norm_affine(h, self.norm_out)
            co = self.conv_out.out_channels
            if co % 4 == 0:
                return fused_conv2d(self.conv_out, h, so, to, "swish")
            return fused_conv2d(self._padded_conv_out(), h, so, to, "swish")[:, :co]
        return self.conv_out(F.silu(self.norm_out(h)))

    def _enter_stacked(self, x, h0, E: int):
        if self.mode != "sparse" or x.shape[0] != E:
            raise RuntimeError("stacked edits: sparse mode, one input image per edit (edit batch %d, mode %r, input batch %d)"
                               % (E, self.mode, x.shape[0]))
        if not _fused_layout(x, h0):
            raise RuntimeError("stacked edits: channels-last fp32 GPU tensors only")
        low = self.resolution >> (self.num_resolutions - 1)
        if self.resolution & (self.resolution - 1) or low < 4:
            # (the seam test of every launch is a shift: sige_hip_set_edit_batch)
            raise RuntimeError("stacked edits: every level's height must be a power of two of at least 4 rows (%d ... %d)"
                               % (self.resolution, low))
        from ..stacked import tall

        return tall(h0)

    def forward(self, x: torch.Tensor, logsnr: torch.Tensor) -> torch.Tensor:
        assert x.shape[2] == x.shape[3] == self.resolution
        temb = self._temb(logsnr)
        if self.mode == "sparse" and self.edit_batch > 1 and x.shape[0] > 1 and x.is_cuda:
            # stacked edits: the first conv image by image.  ONE launch of the library's first conv at batch 8 (64 output channels,
            # 128 x 128) returned wrong pixels in some images, differently from run to run, while its launches on one image each
            # are right (found with tools/pd_bench.py --stacked, cause not found)
            h0 = torch.cat([input_conv2d(self.conv_in, x[e:e + 1]) for e in range(x.shape[0])])
        else:
            h0 = input_conv2d(self.conv_in, x) if self.mode == "sparse" else self.conv_in(x)
        if x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous():
            h0 = h0.contiguous(memory_format=torch.channels_last)  # (MIOpen may hand back NCHW for 3 input channels)
        E = self.edit_batch
        if E > 1:
            # stacked edits (sige_amd/stacked.py): x is [E,3,H,W], conv_in a whole-image op at batch E; from here to the output norm
            # every tensor is the tall image [1,C,E*H,W] -- the same bytes -- and every block works on it unchanged
            h0 = self._enter_stacked(x, h0, E)
        hs = [h0]
        for lvl, stage in enumerate(self.down):
            for i, block in enumerate(stage.block):
                h = block(hs[-1], temb)
                if len(stage.attn):
                    h = stage.attn[i](h)
                hs.append(h)
            if lvl != self.num_resolutions - 1:
                hs.append(stage.downsample(hs[-1], temb))

        h = self.mid.block_1(hs[-1], temb)
        h = self.mid.attn_1(h)
        h = self.mid.block_2(h, temb)

        for lvl in reversed(range(self.num_resolutions)):
            stage = self.up[lvl]
            for i, block in enumerate(stage.block):
                h = block((h, hs.pop()), temb)
                if len(stage.attn):
                    h = stage.attn[i](h)
            if lvl != 0:
                h = stage.upsample(h, temb)
        if E > 1:
            from ..stacked import untall

            with _per_image():  # (norm_out and conv_out are per image: [E,C,1,1] affines at B = E)
                return self._head(untall(h, E))
        return self._head(h)
