"""DDPM 256x256 U-Net workload (LSUN-Church configuration) built on sige_amd.nn.

This is the benchmark harness for BASELINE.json configs[1]/[4]: the network the
reference's headline numbers are quoted on (diffusion/configs/
church_ddpm256-sige.yml: ch 128, mult 1,1,2,2,4,4, 2 res-blocks per level,
attention at 16x16, SIGE tiles 6/4, sparse at resolutions >= 64).  It follows
the public DDPM checkpoint layout (parameter names `down.{l}.block.{i}.conv1`,
`mid.block_1`, `up.{l}.upsample.conv`, `temb.dense.{k}`, ...), so a state dict of
the reference's SIGEFusedUNet (diffusion/models/ddpm_arch/sige_fused_unet.py:
251-434) loads into it -- tests/test_reference_models.py checks that both
produce the same full and sparse outputs.

Sparse-mode contract (what SIGE caches):
  * GroupNorm statistics are NOT recomputed: the full pass stores per-channel
    (scale, shift) = (gamma/sigma, beta - mu*gamma/sigma) of the original image,
    with the timestep-embedding add folded into the second shift; the sparse
    pass feeds them to Gather / ScatterGather as the fused affine + SiLU.
  * resolutions below `sparse_threshold` run dense convs on the cached affine.
"""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch import nn
from torch.nn import functional as F

from ..nn import Gather, Scatter, ScatterGather, ScatterWithBlockResidual, SIGEConv2d, SIGEModel, SIGEModule, paired_convs
from ..nn.deferred import lazy_cat
from ..nn.dense import demand_buffer, fast_full_pass, full_conv2d, fused_conv2d, group_norm_affine, input_conv2d
from ..nn.twins import BufferName, TwinConsumer, TwinProducer, cache_id_of, tag, twin_of


@dataclass
class DDPMConfig:
    ch: int = 128
    ch_mult: Tuple[int, ...] = (1, 1, 2, 2, 4, 4)
    num_res_blocks: int = 2
    attn_resolutions: Tuple[int, ...] = (16,)
    in_ch: int = 3
    out_ch: int = 3
    resolution: int = 256
    main_block: Optional[int] = 6       # tile edge for 3x3 convs
    shortcut_block: Optional[int] = 4   # tile edge for 1x1 convs
    sparse_threshold: int = 64
    groups: int = 32
    eps: float = 1e-6
    # The reference's SIGEFusedAttnBlock stores its cached (scale, shift) un-keyed
    # (sige_fused_unet.py:170) and then indexes them with cache_id, so its sparse
    # pass normalises every channel with channel 0's statistics.  True reproduces
    # that (bit-for-bit model-level parity tests); False is the intended math.
    reference_attn_quirk: bool = False
    # conv1's epilogue applies the cached affine-2 + SiLU (and the ScatterGather cache keeps an activated copy),
    # so conv2 stages raw values: the activation is computed once per element, not once per output-channel block
    preactivate: bool = True
    # launch the shortcut 1x1 of a ResBlock inside the kernel of its conv1 (sige_amd.hip.conv_pair: horizontal fusion)
    pair_shortcut: bool = True
    # conv1 inputs activated by their PRODUCERS: every module whose output feeds a ResBlock's conv1 also writes
    # SiLU(scale1 * out + shift1) (an "activated twin"), so conv1 stages raw values -- the cached affine + SiLU is computed once
    # per element instead of once per output-channel block (8-16 per layer).  Consumers register on their first sparse
    # forward and activate for themselves until the twin exists.  The protocol: sige_amd/nn/twins.py.
    conv1_twins: bool = True
    # run the shortcut branch of a ResBlock (1x1 conv on the block input) on a second stream (it is independent of
    # conv1 -> conv2).  Measured on MI355X / ROCm 7.2: the cross-stream graph edges cost more than the overlap gains
    # (2.05 ms vs 1.82 ms per forward), so it is off by default.
    overlap_shortcut: bool = False


def timestep_embedding(t: torch.Tensor, dim: int) -> torch.Tensor:
    half = dim // 2
    freq = torch.exp(torch.arange(half, dtype=torch.float32, device=t.device) * (-math.log(10000) / (half - 1)))
    arg = t.float()[:, None] * freq[None, :]
    emb = torch.cat([arg.sin(), arg.cos()], dim=1)
    return F.pad(emb, (0, 1)) if dim % 2 else emb


def norm_affine(x: torch.Tensor, norm: nn.GroupNorm, fast: bool = False, cbias: Optional[torch.Tensor] = None,
                x2: Optional[torch.Tensor] = None):
    """Per-channel (scale, shift) with GroupNorm(x) == x * scale + shift, batch 1.  `fast` (the full pass on the fp16 matrix
    cores): the library's split reduction (fp64 combine) instead of torch's var_mean + five elementwise kernels.
    `cbias` [C]: the statistics are those of x + cbias (the timestep embedding); with `fast` the returned affine is for x itself
    (GroupNorm(x + cbias) == x * scale + shift), otherwise for x + cbias as before -- the caller folds the bias."""
    if fast and x.is_cuda:
        assert x.shape[0] == 1, "SIGE caches one original image"
        # (`x2`: the norm of torch.cat([x, x2], 1); tensors that carry their producer's per-channel statistics are not read)
        sc, sh = group_norm_affine(x, norm, cbias, x2=x2, make_stats=True)
        return sc.reshape(-1), sh.reshape(-1)
    if x2 is not None:
        x = torch.cat([x, x2], dim=1)
    n, c, h, w = x.shape
    assert n == 1, "SIGE caches one original image"
    if cbias is not None:
        x = x + cbias.reshape(1, -1, 1, 1)
    g = norm.num_groups
    var, mean = torch.var_mean(x.reshape(g, -1), dim=1, unbiased=False)
    inv = torch.rsqrt(var + norm.eps).repeat_interleave(c // g)
    mu = mean.repeat_interleave(c // g)
    scale = inv * norm.weight
    shift = norm.bias - mu * scale
    return scale, shift


def _as4(v: torch.Tensor) -> torch.Tensor:
    return v.reshape(1, -1, 1, 1)


# Dense attention blocks in sparse mode: run proj_out inside the value projection (AttnBlock.folded_proj) and its bias, residual
# and twins in the epilogue of the attention's second kernel -- three launches per block instead of four.
# False: the chain as it was, qkv conv -> attention -> proj_out conv (A/B runs, tests).
FOLD_ATTN_PROJ = True


def fold_proj_into_qkv(w_qkv: torch.Tensor, b_qkv: Optional[torch.Tensor], w_p: torch.Tensor, b_p: Optional[torch.Tensor]):
    """proj_out folded into the value rows of a single-head attention block's qkv conv.  The softmax rows P sum to 1, so

        W_p (P v) + b_p = P (W_p W_v x + W_p b_v) + b_p = P (W_vp x) + b'     W_vp = W_p W_v,  b' = W_p b_v + b_p

    Returns (weight [3C,C,1,1] = cat(W_q, W_k, W_vp), bias [3C] = cat(b_q, b_k, 0), b' [C]) in the dtype of `w_qkv`; the
    products are formed in fp64 and rounded once."""
    C = w_p.shape[0]
    wq = w_qkv.detach().reshape(3 * C, C)
    wp = w_p.detach().reshape(C, C).double()
    bq = torch.zeros(3 * C, dtype=wq.dtype, device=wq.device) if b_qkv is None else b_qkv.detach()
    w = torch.cat([wq[:2 * C], (wp @ wq[2 * C:].double()).to(wq.dtype)]).reshape(3 * C, C, 1, 1)
    b = torch.cat([bq[:2 * C], torch.zeros_like(bq[2 * C:])])
    bp = wp @ bq[2 * C:].double()
    if b_p is not None:
        bp = bp + b_p.detach().double()
    return w.contiguous(), b, bp.to(wq.dtype)


# ... and the key projection as well (fold_keys_into_query, AttnBlock.folded_qv): the qkv conv becomes C -> 2C with outputs
# (M x_n + m | v') and the keys are the block input itself.  Active where FOLD_ATTN_PROJ is; False: the C -> 3C conv
# of 5.9 (A/B runs, tests).
FOLD_ATTN_QK = True


def fold_keys_into_query(w_qkv: torch.Tensor, b_qkv: Optional[torch.Tensor]):
    """The key projection of a single-head attention block folded into its query projection.  With x_n = s*x + t the
    normalised input, q = W_q x_n + b_q and k = W_k x_n + b_k, a term of q_i . k_j that does not depend on the key j cancels
    in the softmax over j:

        q_i . k_j          = (W_k^T q_i) . x_n,j + q_i . b_k              (second term constant in j)
        (W_k^T q_i) . x_n,j = (s * W_k^T q_i) . x_j + (W_k^T q_i) . t      (second term constant in j)

        softmax_j(scale q_i . k_j) = softmax_j(scale q''_i . x_j),   q'' = s * (M x_n + m),   M = W_k^T W_q,  m = W_k^T b_q

    Returns (M [C,C], m [C]) in the dtype of `w_qkv`; the products are formed in fp64 and rounded once.  The factor s is the
    cached GroupNorm scale: not a weight, so it stays with the caller (the conv's out-affine, or the score kernel's query scale)."""
    C = w_qkv.shape[0] // 3
    wq = w_qkv.detach().reshape(3 * C, C)
    wk_t = wq[C:2 * C].double().t()
    M = wk_t @ wq[:C].double()
    m = torch.zeros(C, dtype=torch.float64, device=wq.device) if b_qkv is None else wk_t @ b_qkv.detach()[:C].double()
    return M.to(wq.dtype).contiguous(), m.to(wq.dtype)


class ResBlock(SIGEModule, TwinProducer, TwinConsumer):
    def __init__(self, cfg: DDPMConfig, cin: int, cout: int, sparse: bool):
        super().__init__()
        self.cin, self.cout = cin, cout
        self.sparse_main = sparse and cfg.main_block is not None
        Conv = SIGEConv2d if self.sparse_main else nn.Conv2d
        self.norm1 = nn.GroupNorm(cfg.groups, cin, eps=cfg.eps)
        self.conv1 = Conv(cin, cout, 3, 1, 1)
        self.norm2 = nn.GroupNorm(cfg.groups, cout, eps=cfg.eps)
        self.conv2 = Conv(cout, cout, 3, 1, 1)
        self.sparse_shortcut = False
        if self.sparse_main:
            self.main_gather = Gather(self.conv1, cfg.main_block, activation_name="swish")
            self.scatter_gather = ScatterGather(self.main_gather, activation_name="swish")
        if cin != cout:
            self.sparse_shortcut = self.sparse_main and cfg.shortcut_block is not None
            self.nin_shortcut = (SIGEConv2d if self.sparse_shortcut else nn.Conv2d)(cin, cout, 1, 1, 0)
            if self.sparse_shortcut:
                self.shortcut_gather = Gather(self.nin_shortcut, cfg.shortcut_block)
                self.scatter = ScatterWithBlockResidual(self.main_gather, self.shortcut_gather)
        if self.sparse_main and not self.sparse_shortcut:
            self.scatter = Scatter(self.main_gather)
        self.affine = {}  # cache_id -> (scale1, shift1, scale2, shift2) as [1,C,1,1]
        self.plain = False
        self.preactivate = cfg.preactivate
        self.overlap = cfg.overlap_shortcut
        self.pair = cfg.pair_shortcut
        self._init_twin_consumer(cfg.conv1_twins)
        self._side = None

    def clear_cache(self):
        self.affine = {}
        self._drop_twin_links()
        self.__dict__.pop("_split1", None)
        self.__dict__.pop("_side_product", None)

    # ---- conv1 of an up block split at the torch.cat (DDPMSparseUNet.SIDE_SKIP_PRODUCTS) ----
    def split_conv1(self, ch: int):
        """(conv_h, conv_s): conv1 over cat(h, skip) as two convs, W[:, :ch] with the bias and W[:, ch:] without, so that
        conv1(cat(a, b)) = conv_h(a) + conv_s(b).  Derived nn.Conv2d objects like AttnBlock.folded_proj(): neither a Parameter, a
        buffer nor a submodule (the state dict keeps the reference's keys); rebuilt when conv1's weight or bias has been replaced,
        moved or edited in place (address, version counter, shape, device, dtype), when its compute dtype changes, and after
        clear_cache()."""
        params = (self.conv1.weight, self.conv1.bias)
        key = tuple(None if p is None else (p.data_ptr(), p._version, tuple(p.shape), p.device, p.dtype) for p in params)
        key += (getattr(self.conv1, "compute_dtype", "f32"), ch)
        entry = self.__dict__.get("_split1")
        if entry is None or entry[0] != key:
            w, b = (None if p is None else p.detach() for p in params)
            cin, cout = w.shape[1], w.shape[0]
            conv_h = nn.Conv2d(ch, cout, 3, 1, 1, bias=b is not None, device="meta")
            conv_s = nn.Conv2d(cin - ch, cout, 3, 1, 1, bias=False, device="meta")
            conv_h.weight = nn.Parameter(w[:, :ch].contiguous(), requires_grad=False)
            conv_s.weight = nn.Parameter(w[:, ch:].contiguous(), requires_grad=False)
            if b is not None:
                conv_h.bias = nn.Parameter(b.clone(), requires_grad=False)
            conv_h.compute_dtype = conv_s.compute_dtype = key[-2]
            entry = (key, conv_h, conv_s)
            self.__dict__["_split1"] = entry  # (not through nn.Module.__setattr__: that would register the convs as submodules)
        return entry[1], entry[2]

    def side_product_ready(self, skip: torch.Tensor):
        """The activated twin of `skip` if this block can take conv1's skip half as a precomputed product in this forward -- a
        dense up block in sparse mode on channels-last fp32 GPU tensors, one image, exact-fp32 conv1, the skip's twin written and
        the twin of h promised by its producer -- else None (conv1 runs unsplit, as without the flag)."""
        from .. import hip

        if self.sparse_main or self.mode != "sparse" or not (self.use_twins and self.preactivate) or self.overlap:
            return None
        if hip.TILE3:  # (every eligible launch forced onto the tile conv v3: no launch is left that could host a product)
            return None
        if not (isinstance(skip, torch.Tensor) and skip.is_cuda and skip.dtype == torch.float32 and skip.shape[0] == 1 and hip.is_cl(skip)):
            return None
        if getattr(self.conv1, "compute_dtype", "f32") != "f32" or hip.get_edit_batch() != 1 or self.cache_id not in self.affine:
            return None
        ch = self.cin - skip.shape[1]
        if ch <= 0 or not hip.cl_supported(ch, skip.shape[1], self.cout) or self.affine[self.cache_id][0].shape[0] != 1:
            return None
        # (the derived convs are built and packed as soon as the block qualifies by shape -- in the first sparse forward, next
        #  to every other weight -- so that no later forward launches pack kernels)
        from ..nn.dense import _packed

        for conv in self.split_conv1(ch):
            _packed(conv, (6, 6))
        if self._twin_key(0) not in self._twin_links:
            return None
        return twin_of(skip, self._twin_key(1))

    def submit_side_product(self, skip: torch.Tensor) -> bool:
        """Queue W[:, ch:] * act(skip) as a side conv (hip.conv_side_begin) into a persistent buffer; _sparse_dense picks it up."""
        from .. import hip

        tw = self.side_product_ready(skip)
        if tw is None:
            return False
        _, conv_s = self.split_conv1(self.cin - skip.shape[1])
        B, _, H, W = skip.shape
        buf = demand_buffer(conv_s, ("side", self.cache_id), (B, self.cout, H, W), skip.device)
        tiles = hip.all_tiles(H, W, (4, 4), (1, 1), (1, 1), skip.device)
        hip.conv_side_begin()
        fused_conv2d(conv_s, tw, tiles=tiles, out=buf)
        self.__dict__["_side_product"] = (buf, tw)
        return True

    # ---- activated twins (cfg.conv1_twins): producer and consumer, sige_amd/nn/twins.py ----
    def _twin_scatter(self):
        return self.scatter if self.sparse_main else None

    def rebuild_derived_caches(self):
        """(sige_amd.parallel) the cache tensors were rewritten in place: recompute the activated ScatterGather copy."""
        if self.sparse_main and self.preactivate:
            for cid, (_, _, s2, t2) in self.affine.items():
                if cid in self.scatter_gather.original_outputs:
                    keep, self.scatter_gather.cache_id = self.scatter_gather.cache_id, cid
                    self.scatter_gather.cache_activated(s2, t2)
                    self.scatter_gather.cache_id = keep

    def _shortcut_async(self, fn, x_ready: torch.Tensor):
        """Run `fn()` (the shortcut branch) on a side stream forked from the current one; returns (result, join).
        `join()` must be called on the current stream before the result is consumed.  hipGraph capture records the
        fork / join as graph edges, so the two branches run concurrently in a replay."""
        if not (self.overlap and x_ready.is_cuda and self.mode == "sparse"):
            return fn(), (lambda: None)
        cur = torch.cuda.current_stream(x_ready.device)
        if self._side is None:
            self._side = torch.cuda.Stream(device=x_ready.device)
        side = self._side
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            out = fn()

        def join():
            cur.wait_stream(side)
            out.record_stream(cur)  # (allocated on the side stream, consumed on the current one)

        return out, join

    def _pairing(self, t: torch.Tensor):
        """Context for [shortcut conv, conv1] of a sparse-mode block: on the GPU the two share one launch."""
        return paired_convs(t, enabled=self.pair and self.cin != self.cout and self.mode == "sparse", main=getattr(self, "main_gather", None))

    def forward(self, x, temb: Optional[torch.Tensor], demand=None) -> torch.Tensor:
        """`x` may be a pair (h, skip): the up path's torch.cat, which the dense
        sparse-mode blocks fold into their convs' two-pointer input.
        `demand` = (hip.DemandTiles, depth of this block's conv2) for a dense block of a stage that runs on its demand regions
        (DDPMSparseUNet.DENSE_ON_DEMAND): conv2 and the shortcut compute the cells of that depth, conv1 those one deeper -- or on
        its change regions (DDPMSparseUNet.DENSE_ON_CHANGE: the lists of this block, conv2's first, and depth 0)."""
        pair = x if isinstance(x, (tuple, list)) else None
        if self.mode == "full":
            if pair and not self.plain and self._fast_full() and pair[0].is_cuda:
                return self._full(pair[0], temb, x2=pair[1])  # (the cat never exists: two-pointer convs, statistics per part)
            return self._full(torch.cat(pair, dim=1) if pair else x, temb)
        if self.mode in ("sparse", "profile"):
            if pair and not self.sparse_main and self.mode == "sparse":
                return self._sparse_dense(pair[0], pair[1], demand)
            if pair and self.mode == "sparse" and self.cin != self.cout:
                return self._sparse(lazy_cat(pair[0], pair[1]))  # consumed by the block's two Gathers only
            return self._sparse(torch.cat(pair, dim=1) if pair else x, demand)
        raise NotImplementedError("Unknown mode [%s]!!!" % self.mode)

    def _fast_full(self) -> bool:
        """The full pass on the library's kernels (dense.full_conv2d) rather than torch's: compute dtype "f16" / "f16x3", or
        dense.FULL_PASS_F32_NATIVE for exact fp32."""
        from ..nn import dense as _dense

        return _dense.fast_full_pass(self.conv1)

    def _shortcut(self, x, x2=None):
        if self.cin == self.cout:
            return x if x2 is None else torch.cat([x, x2], dim=1)  # (identity shortcut of a concatenated input: both halves)
        if x2 is not None:  # (full mode, fast: the cat is read through two pointers)
            if self.sparse_shortcut:
                self.shortcut_gather.note_full_input(x.shape[2:])
            return full_conv2d(self.nin_shortcut, x, x2=x2)
        if self.sparse_shortcut:
            x = self.shortcut_gather(x)
        return full_conv2d(self.nin_shortcut, x) if self.mode == "full" else self.nin_shortcut(x)

    def _plain(self, x, temb):
        """Dense forward with stock GroupNorm and no caching (the "original model"
        baseline the speedup is quoted against)."""
        skip = x if self.cin == self.cout else self.nin_shortcut(x)
        h = self.conv1(F.silu(self.norm1(x)))
        h = self.conv2(F.silu(self.norm2(h + temb.reshape(1, -1, 1, 1))))
        return h + skip

    def _full(self, x, temb, x2=None):
        if self.plain:
            return self._plain(x, temb)
        # (the full pass on the library's kernels -- dense.full_conv2d -- also takes the library's GroupNorm statistics; its
        #  convs leave the per-channel sums of their outputs, so that a norm never reads a tensor its producer just wrote)
        fast = self._fast_full()
        skip = self._shortcut(x, x2)
        if x2 is not None:
            if self.sparse_main:
                self.main_gather.note_full_input(x.shape[2:])
            h = x
        else:
            h = self.main_gather(x) if self.sparse_main else x  # records the input resolution
        s1, t1 = norm_affine(h, self.norm1, fast, x2=x2)
        h = full_conv2d(self.conv1, h, _as4(s1), _as4(t1), "swish", x2=x2, stats=fast)  # conv1(silu(cat(h, x2) * s1 + t1))
        if self.sparse_main:
            h = self.scatter_gather(h)
        te = temb.reshape(-1)
        if fast and h.is_cuda:
            # statistics of h + temb and the embedding folded into the shift in ONE launch (no h + temb tensor)
            s2, t2 = norm_affine(h, self.norm2, True, cbias=te.contiguous())
        else:
            s2, t2 = norm_affine(h + _as4(te), self.norm2, fast)
            t2 = t2 + te * s2  # fold the timestep-embedding add into the cached shift
        self._drop_twin_links()  # (twins written for the previous affine are stale)
        self.affine[self.cache_id] = tuple(_as4(v).contiguous() for v in (s1, t1, s2, t2))
        if self.sparse_main and self.preactivate:
            self.scatter_gather.cache_activated(_as4(s2), _as4(t2))
        # conv2(silu(h * s2 + t2)) + skip in one launch: a plain Scatter caches the SUM (sige/nn/scatter.py:31-37), and so does
        # ScatterWithBlockResidual (sige/nn/scatter.py:89-93), next to the shortcut
        if self.sparse_main and self.sparse_shortcut:
            if fast and h.is_cuda:
                h = full_conv2d(self.conv2, h, _as4(s2), _as4(t2), "swish", residual=skip, stats=True)
                return self.scatter(h, skip, x_is_sum=True)
            h = full_conv2d(self.conv2, h, _as4(s2), _as4(t2), "swish")  # conv2(silu(h * s2 + t2))
            return self.scatter(h, skip)
        h = full_conv2d(self.conv2, h, _as4(s2), _as4(t2), "swish", residual=skip, stats=fast)
        return self.scatter(h) if self.sparse_main else h

    def _sparse(self, x, demand=None):
        s1, t1, s2, t2 = self.affine[self.cache_id]
        if self.sparse_main and self.preactivate and self.mode == "sparse":
            parts = list(x.parts) if hasattr(x, "parts") else [x]
            first = parts[0]
            tw = self._twin_inputs(parts, s1, t1)
            # an accepted edit (`sparse_update`): conv1's RAW tiles are what the ScatterGather cache takes (SiLU cannot be inverted), so
            # conv1 runs without its out-affine and conv2 stages SiLU(s2 * . + t2) itself -- the same launches, the activation moved
            # to conv2's staging
            oa = {} if self.sparse_update else dict(out_affine=(s2, t2, "swish"))
            with self._pairing(first):
                skip, join = (self._shortcut_async(lambda: self._shortcut(x), first) if self.cin != self.cout
                              else (x, lambda: None))
                if tw is not None:  # the producers wrote SiLU(s1 * x + t1): conv1 stages raw values
                    xa = tw[0] if len(tw) == 1 else lazy_cat(tw[0], tw[1])
                    h = self.conv1(self.main_gather(xa, preactivated=True), **oa)
                else:
                    h = self.conv1(self.main_gather(x, s1, t1), **oa)
            tiles = self.scatter_gather(h, s2, t2) if self.sparse_update else self.scatter_gather(h, preactivated=True)
            join()
            return self._produced(self.scatter.forward_fused(self.conv2, tiles, skip))
        if not self.sparse_main:
            return self._sparse_dense(x, None, demand)
        skip = self._shortcut(x)
        h = self.conv1(self.main_gather(x, s1, t1))
        if self.mode == "sparse":
            return self.scatter.forward_fused(self.conv2, self.scatter_gather(h, s2, t2), skip)
        return self.scatter(self.conv2(self.scatter_gather(h, s2, t2)), skip)

    def _demand_args(self, conv, demand, deeper: int, x) -> dict:
        """fused_conv2d's `tiles` / `out` for `conv` of a block that runs on its demand regions ({}: the all-tiles call).
        Outside a launch plan a list that holds every cell takes the all-tiles call, so a large edit runs exactly the launches
        it always ran; a plan follows any later mask and therefore always takes the list."""
        if demand is None:
            return {}
        from .. import hip

        region, depth = demand
        lists = region.flat if tuple(conv.kernel_size) == (1, 1) else region.main
        tiles = lists[depth + deeper]
        # (change regions: `tag` = the cache id the persistent buffers belong to -- what they hold outside the lists is READ;
        #  `keep` = the launch that establishes it: every cell, into those buffers)
        tag, keep = getattr(region, "tag", None), getattr(region, "keep", False)
        if tiles.shape[0] == region.cells and hip.plan_recorder() is None and not keep:
            return {}
        shape = (x.shape[0], conv.out_channels, x.shape[2], x.shape[3])
        return dict(tiles=tiles, out=demand_buffer(conv, "out" if tag is None else ("out", tag), shape, x.device))

    def _sparse_dense(self, x, x2, demand=None):
        """Dense block on the cached affine: 2-3 fused launches (shortcut 1x1, conv1, conv2+skip)."""
        s1, t1, s2, t2 = self.affine[self.cache_id]
        join = lambda: None  # noqa: E731
        if self.preactivate:
            tw = self._twin_inputs([x] if x2 is None else [x, x2], s1, t1)
            side = self.__dict__.pop("_side_product", None)
            if side is not None:
                from .. import hip

                hip.conv_side_flush(x)  # (what no host has taken runs now: the product is complete behind this)
                if tw is None or demand is not None or tw[1] is not side[1]:
                    side = None  # (no twin of h after all: the unsplit conv1, as without the flag)
            with self._pairing(x):
                if self.cin == self.cout:
                    skip = x if x2 is None else torch.cat([x, x2], dim=1)
                else:
                    # (the shortcut is needed where conv2 adds it: on conv2's cells)
                    skip, join = self._shortcut_async(lambda: fused_conv2d(self.nin_shortcut, x, x2=x2,
                                                                           **self._demand_args(self.nin_shortcut, demand, 0, x)), x)
                if side is not None:  # conv1 = W[:, :ch] * act(h) + b + the skip product computed behind earlier launches
                    conv_h, _ = self.split_conv1(x.shape[1])
                    h = fused_conv2d(conv_h, tw[0], None, None, "identity", residual=side[0], out_affine=(s2, t2, "swish"))
                elif tw is not None:  # the producers wrote SiLU(s1 * x + t1): conv1 stages raw values
                    h = fused_conv2d(self.conv1, tw[0], None, None, "identity", x2=(tw[1] if len(tw) > 1 else None),
                                     out_affine=(s2, t2, "swish"), **self._demand_args(self.conv1, demand, 1, x))
                else:
                    h = fused_conv2d(self.conv1, x, s1, t1, "swish", x2=x2, out_affine=(s2, t2, "swish"),
                                     **self._demand_args(self.conv1, demand, 1, x))
            join()
            return self._produced(fused_conv2d(self.conv2, h, residual=skip, twins=self._my_twins(),
                                               **self._demand_args(self.conv2, demand, 0, x)))
        if self.cin == self.cout:
            skip = x if x2 is None else torch.cat([x, x2], dim=1)
        else:
            skip, join = self._shortcut_async(lambda: fused_conv2d(self.nin_shortcut, x, x2=x2), x)
        join()
        h = fused_conv2d(self.conv1, x, s1, t1, "swish", x2=x2)
        return fused_conv2d(self.conv2, h, s2, t2, "swish", residual=skip)


class AttnBlock(SIGEModule, TwinProducer):
    def __init__(self, cfg: DDPMConfig, ch: int, sparse: bool):
        super().__init__()
        self.ch = ch
        self.edit_batch = 1  # (sige_amd.stacked: E images stacked along H; attention is per image)
        self.quirk = cfg.reference_attn_quirk
        self.sparse = sparse and cfg.shortcut_block is not None
        Conv = SIGEConv2d if self.sparse else nn.Conv2d
        self.norm = nn.GroupNorm(cfg.groups, ch, eps=cfg.eps)
        self.qkv = Conv(ch, 3 * ch, 1, 1, 0)
        self.proj_out = Conv(ch, ch, 1, 1, 0)
        if self.sparse:
            self.gather1 = Gather(self.qkv, cfg.shortcut_block)
            self.scatter1 = Scatter(self.gather1)
            self.gather2 = Gather(self.proj_out, cfg.shortcut_block)
            self.scatter2 = Scatter(self.gather2)
        self.affine = {}
        self.plain = False

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.mode == "full" and self.plain:
            h = self.norm(x)
        elif self.mode == "full":
            h = self.gather1(x) if self.sparse else x
            s, t = norm_affine(h, self.norm, fast_full_pass(self.qkv))
            self.affine[self.cache_id] = (_as4(s).contiguous(), _as4(t).contiguous())
            if not self.sparse:  # dense block: qkv(h * s + t) in one launch where the conv's compute dtype allows, then the rest
                qkv = full_conv2d(self.qkv, h, _as4(s), _as4(t), "identity")
                return full_conv2d(self.proj_out, self._attention(qkv), residual=x)
            h = h * _as4(s) + _as4(t)
        else:
            s, t = self.affine[self.cache_id]
            if self.quirk:
                s, t = s[:, :1].expand_as(s).contiguous(), t[:, :1].expand_as(t).contiguous()
            if not self.sparse and self.mode == "sparse":
                return self._dense_sparse(x, s, t)
            h = self.gather1(x, s, t) if self.sparse else x * s + t
        plain = self.mode == "full" and self.plain
        qkv = self.qkv(h)
        if self.sparse and not plain:
            qkv = self.scatter1(qkv)
        b, _, hh, ww = qkv.shape
        q, k, v = qkv.reshape(b, 3, self.ch, hh * ww).unbind(1)
        attn = torch.softmax(torch.bmm(q.transpose(1, 2), k) * (self.ch ** -0.5), dim=2)  # [b, hw(q), hw(k)]
        h = torch.bmm(v, attn.transpose(1, 2)).reshape(b, self.ch, hh, ww)
        if self.sparse and not plain:
            h = self.gather2(h)
        h = self.proj_out(h)
        return self.scatter2(h, x) if (self.sparse and not plain) else h + x


    def _attention(self, qkv):
        if self.edit_batch > 1 and qkv.shape[0] == 1:
            # stacked edits: the tall image is E images -- tokens attend within their own image (the same bytes seen as batch E)
            from ..stacked import tall, untall

            return tall(self._attention(untall(qkv, self.edit_batch)))
        b, _, hh, ww = qkv.shape
        if qkv.is_cuda and qkv.dtype == torch.float32:
            from .. import hip

            if hip.is_cl(qkv):
                out = hip.attention_cl(qkv, self.ch ** -0.5)
                if out is not None:
                    return out
            if hip.attention_supported(self.ch, hh * ww):
                return hip.attention(qkv, self.ch ** -0.5)
        q, k, v = qkv.reshape(b, 3, self.ch, hh * ww).unbind(1)
        attn = torch.softmax(torch.bmm(q.transpose(1, 2), k) * (self.ch ** -0.5), dim=2)
        return torch.bmm(v, attn.transpose(1, 2)).reshape(b, self.ch, hh, ww)

    def _twins_ok(self) -> bool:
        return not self.sparse  # (the tiled form ends in a plain Scatter with a residual: not wired for twins)

    def clear_cache(self):
        self.affine = {}
        self.__dict__.pop("_fold", None)
        self.__dict__.pop("_fold_qv", None)
        self.__dict__.pop("_qv_oaffine", None)

    def folded_proj(self):
        """(conv, b'): the qkv conv with proj_out folded into its value rows (fold_proj_into_qkv) as a derived nn.Conv2d that the
        dense-layer launches pack like any other, and the bias left for the attention's epilogue.  Neither is a Parameter, a
        buffer or a submodule -- the state dict keeps the reference's keys.  Rebuilt when a parameter of `qkv` / `proj_out` has
        been replaced, moved or edited in place (address, version counter, shape, device, dtype: what the packed-weight caches
        key on, sige_amd/nn/base.py), and after clear_cache() -- an edit through `.data` moves no version counter."""
        params = (self.qkv.weight, self.qkv.bias, self.proj_out.weight, self.proj_out.bias)
        key = tuple(None if p is None else (p.data_ptr(), p._version, tuple(p.shape), p.device, p.dtype) for p in params)
        key += (getattr(self.qkv, "compute_dtype", "f32"),)
        entry = self.__dict__.get("_fold")
        if entry is None or entry[0] != key:
            w, b, bp = fold_proj_into_qkv(*params)
            conv = nn.Conv2d(self.ch, 3 * self.ch, 1, 1, 0, device="meta")
            conv.weight, conv.bias = nn.Parameter(w, requires_grad=False), nn.Parameter(b, requires_grad=False)
            conv.compute_dtype = key[-1]
            entry = (key, conv, bp)
            self.__dict__["_fold"] = entry  # (not through nn.Module.__setattr__: that would register the conv as a submodule)
        return entry[1], entry[2]

    def folded_qv(self):
        """(conv, b'): the C -> 2C conv with outputs (M x_n + m | v') -- the key projection folded into the query rows
        (fold_keys_into_query) next to the value rows of folded_proj(), bias (m | 0).  Derived, keyed and rebuilt exactly as
        folded_proj(); the factor s of q'' is not in it: the caller applies it (the conv's out-affine, or the score kernel's qscale)."""
        conv3, bp = self.folded_proj()
        key = self.__dict__["_fold"][0]
        entry = self.__dict__.get("_fold_qv")
        if entry is None or entry[0] != key or entry[3] is not conv3:
            C = self.ch
            M, m = fold_keys_into_query(self.qkv.weight, self.qkv.bias)
            conv = nn.Conv2d(C, 2 * C, 1, 1, 0, device="meta")
            w = torch.cat([M.reshape(C, C, 1, 1), conv3.weight.detach()[2 * C:]]).contiguous()
            conv.weight = nn.Parameter(w, requires_grad=False)
            conv.bias = nn.Parameter(torch.cat([m, torch.zeros_like(m)]), requires_grad=False)
            conv.compute_dtype = key[-1]
            entry = (key, conv, bp, conv3)
            self.__dict__["_fold_qv"] = entry
        return entry[1], entry[2]

    def _qv_out_affine(self, s):
        """Out-affine of the key-folded conv for a cache with one affine: scale (s | 1), shift 0, identity.  (s | 1) is a COPY of the
        cached scale, kept per cache id at a fixed address (launch plans and captured graphs replay pointers; no per-forward
        temporaries).  It is rebuilt when the cached affine is another tensor, and re-copied IN PLACE by rebuild_derived_caches()
        when the cache was rewritten behind the module's back (parallel.refresh_derived)."""
        src = self.affine[self.cache_id][0]
        kept = self.__dict__.setdefault("_qv_oaffine", {})
        entry = kept.get(self.cache_id)
        if entry is None or entry[0] is not src or entry[1] != self.quirk:
            sv = s.reshape(-1)
            entry = (src, self.quirk, torch.cat([sv, torch.ones_like(sv)]), torch.zeros(2 * sv.numel(), dtype=s.dtype, device=s.device))
            kept[self.cache_id] = entry
        return entry[2], entry[3], "identity"

    def rebuild_derived_caches(self):
        # (parallel.refresh_derived: the cached affines were overwritten in place -- the kept (s | 1) vectors follow, at their addresses)
        for cid, (src, quirk, vec, _) in list(self.__dict__.get("_qv_oaffine", {}).items()):
            cur = self.affine.get(cid)
            if cur is None or cur[0] is not src:
                del self.__dict__["_qv_oaffine"][cid]  # (re-pointed: rebuilt at the next forward)
                continue
            sv = src.reshape(-1)
            vec[:sv.numel()].copy_(sv[:1].expand_as(sv) if quirk else sv)

    def _fold_ok(self, x) -> bool:
        # where hip.attention_residual_cl runs, and in exact fp32 only ("f16" / "f16x3" layers keep the chain their sweeps pin)
        if not (FOLD_ATTN_PROJ and x.is_cuda and x.dtype == torch.float32):
            return False
        if getattr(self.qkv, "compute_dtype", "f32") != "f32" or getattr(self.proj_out, "compute_dtype", "f32") != "f32":
            return False
        from .. import hip

        return hip.is_cl(x) and not hip.FUSED_ATTENTION

    def _dense_sparse(self, x, s, t):
        refused = self.__dict__.setdefault("_fold_refused", set())  # (shapes the attention kernels do not take: asked once)
        if tuple(x.shape) not in refused and self._fold_ok(x):
            from .. import hip

            if FOLD_ATTN_QK:
                # the factor s of q'': one affine for the whole batch -> the conv's out-affine (s | 1) (measured 3 us per forward
                # faster than the score kernel's query scale); one affine per image -> the score kernel reads it
                conv, bp = self.folded_qv()
                one = s.shape[0] == 1
                qv = fused_conv2d(conv, x, s, t, "identity", out_affine=self._qv_out_affine(s) if one else None)
                qs = None if one else s
                if hip.is_cl(qv):
                    E = self.edit_batch if qv.shape[0] == 1 else 1
                    if E > 1:  # (stacked edits, as below: queries, values, keys, residual and twins per image)
                        from ..stacked import tall, untall

                        res = hip.attention_residual_qv_cl(untall(qv, E), untall(x, E), self.ch ** -0.5, bp, residual=untall(x, E),
                                                           twins=self._my_twins(), qscale=qs)
                        if res is not None:
                            res = (tall(res[0]), {k: tall(v) for k, v in res[1].items()})
                    else:
                        res = hip.attention_residual_qv_cl(qv, x, self.ch ** -0.5, bp, residual=x, twins=self._my_twins(), qscale=qs)
                    if res is not None:
                        return tag(res[0], res[1], self)
            conv, bp = self.folded_proj()
            qkv = fused_conv2d(conv, x, s, t, "identity")
            if hip.is_cl(qkv):
                E = self.edit_batch if qkv.shape[0] == 1 else 1
                if E > 1:
                    # stacked edits: the tall image is E images -- tokens attend within their own image (the same bytes seen as
                    # batch E, residual and twins alike)
                    from ..stacked import tall, untall

                    res = hip.attention_residual_cl(untall(qkv, E), self.ch ** -0.5, bp, residual=untall(x, E), twins=self._my_twins())
                    if res is not None:
                        res = (tall(res[0]), {k: tall(v) for k, v in res[1].items()})
                else:
                    res = hip.attention_residual_cl(qkv, self.ch ** -0.5, bp, residual=x, twins=self._my_twins())
                if res is not None:
                    return tag(res[0], res[1], self)
            refused.add(tuple(x.shape))
        qkv = fused_conv2d(self.qkv, x, s, t, "identity")
        return self._produced(fused_conv2d(self.proj_out, self._attention(qkv), residual=x, twins=self._my_twins()))


class Upsample(SIGEModule, TwinProducer):
    """nearest x2 then a tiled 3x3 conv (always tiled, as in the reference)."""

    def _twin_scatter(self):
        return self.scatter

    def __init__(self, cfg: DDPMConfig, ch: int):
        super().__init__()
        self.conv = SIGEConv2d(ch, ch, 3, 1, 1)
        self.gather = Gather(self.conv, cfg.main_block)
        self.scatter = Scatter(self.gather)
        self.plain = False

    def forward(self, x):
        if self.mode == "sparse" and self.gather.fuses_upsample(x):
            # the upsampled tensor only feeds the gather: read the half-resolution one at (h/2, w/2) instead
            return self._produced(self.scatter.forward_fused(self.conv, self.gather(x, upsample2x=True)))
        if self.mode == "full" and not self.plain and x.is_cuda:
            from ..nn import dense as _dense

            if _dense.fast_full_pass(self.conv):
                # the full pass on the library's kernels: the conv reads the half-resolution tensor at (h/2, w/2) as well
                self.gather.note_full_input((2 * x.shape[2], 2 * x.shape[3]))
                return self.scatter(full_conv2d(self.conv, x, upsample2x=True, stats=True))
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
        if self.mode == "sparse":
            return self._produced(self.scatter.forward_fused(self.conv, self.gather(x)))
        if self.plain and self.mode == "full":
            return self.conv(x)
        return self.scatter(self.conv(self.gather(x)))


class Downsample(SIGEModule, TwinProducer):
    """3x3 stride-2 conv with (0,1,0,1) zero padding; tiled when `sparse` (the
    gather's zero fill past the bottom/right border IS the padding then)."""

    def _twin_scatter(self):
        return self.scatter if self.sparse else None

    def __init__(self, cfg: DDPMConfig, ch: int, sparse: bool):
        super().__init__()
        self.sparse = sparse
        self.plain = False
        self.conv = (SIGEConv2d if sparse else nn.Conv2d)(ch, ch, 3, 2, 0)
        if sparse:
            self.gather = Gather(self.conv, cfg.main_block)
            self.scatter = Scatter(self.gather)

    def forward(self, x):
        if not self.sparse and self.mode == "sparse":
            return self._produced(fused_conv2d(self.conv, x, pad_bottom_right=True, twins=self._my_twins()))
        if self.mode == "full" and not self.plain and x.is_cuda:
            from ..nn import dense as _dense

            if _dense.fast_full_pass(self.conv):
                # the full pass on the library's kernels: the padding is the tile kernel's zero fill, as in the sparse pass
                if not self.sparse:
                    return fused_conv2d(self.conv, x, pad_bottom_right=True)
                return self.scatter(fused_conv2d(self.conv, self.gather(x), pad_bottom_right=True))
        if not self.sparse or (self.plain and self.mode == "full"):
            return self.conv(F.pad(x, (0, 1, 0, 1)))
        x = self.gather(x)
        if self.mode == "full":
            x = F.pad(x, (0, 1, 0, 1))
        if self.mode == "sparse":
            return self._produced(self.scatter.forward_fused(self.conv, x))
        return self.scatter(self.conv(x))


class DDPMSparseUNet(SIGEModel):
    # an accepted edit (`set_sparse_update(True)`) stays on the fused kernels and is committed by one tile-copy launch per
    # hip.COMMIT_CAPACITY records at the end of the forward (sige_amd/nn/commit.py)
    COMMIT_TILES = True

    # set_compute_dtype("f16"): the convs that stay at fp32-level precision (split fp16 operands, "f16x3") so that the f16
    # path meets sige_amd.tolerance.F16_CRITERION at every edit ratio of BASELINE.json configs[4] (1 ... 20 %).  From the
    # per-layer error trace (tests/f16_error_trace.py, profiles/r3a_f16_error_trace.json): fp16 rounding errors made on
    # the down path and at the 16x16 / 8x8 levels are amplified by everything downstream; with them kept the worst
    # element is at 0.34 of the allowed error at 20 % edit (2.5x over it with every conv in plain fp16).
    F16_KEEP = ("down", "up.4", "up.5")
    # ... for edits above this fraction of the image; below it every conv in plain fp16 meets the criterion (worst element at
    # 0.11 / 0.15 / 0.24 of the allowed error at 1 / 2 / 5 % edit, 0.98 at 10 %: the same trace)
    F16_KEEP_ABOVE = 0.05

    def __init__(self, cfg: DDPMConfig = DDPMConfig()):
        super().__init__()
        self.cfg = cfg
        self.edit_batch = 1  # (sige_amd.stacked.edit_batch: E edits of one original stacked along H in every sparse-mode tensor)
        ch, mult = cfg.ch, tuple(cfg.ch_mult)
        self.ch, self.temb_ch = ch, 4 * ch
        self.num_levels = len(mult)
        self.resolution = cfg.resolution
        self.conv_in = nn.Conv2d(cfg.in_ch, ch, 3, 1, 1)
        temb_slices = []

        res = cfg.resolution
        in_mult = (1,) + mult
        self.down = nn.ModuleList()
        cur = ch
        for lvl in range(self.num_levels):
            stage = nn.Module()
            stage.block, stage.attn = nn.ModuleList(), nn.ModuleList()
            cur, cout = ch * in_mult[lvl], ch * mult[lvl]
            sparse = res >= cfg.sparse_threshold
            for _ in range(cfg.num_res_blocks):
                stage.block.append(ResBlock(cfg, cur, cout, sparse))
                temb_slices.append(cout)
                cur = cout
                if res in cfg.attn_resolutions:
                    stage.attn.append(AttnBlock(cfg, cur, sparse))
            if lvl != self.num_levels - 1:
                stage.downsample = Downsample(cfg, cur, sparse)
                res //= 2
            self.down.append(stage)

        self.mid = nn.Module()
        self.mid.block_1 = ResBlock(cfg, cur, cur, False)
        self.mid.attn_1 = AttnBlock(cfg, cur, False)
        self.mid.block_2 = ResBlock(cfg, cur, cur, False)
        temb_slices += [cur, cur]

        ups = []
        for lvl in reversed(range(self.num_levels)):
            stage = nn.Module()
            stage.block, stage.attn = nn.ModuleList(), nn.ModuleList()
            cout = ch * mult[lvl]
            sparse = res >= cfg.sparse_threshold
            for i in range(cfg.num_res_blocks + 1):
                skip = ch * (in_mult[lvl] if i == cfg.num_res_blocks else mult[lvl])
                stage.block.append(ResBlock(cfg, cur + skip, cout, sparse))
                temb_slices.append(cout)
                cur = cout
                if res in cfg.attn_resolutions:
                    stage.attn.append(AttnBlock(cfg, cur, sparse))
            if lvl != 0:
                stage.upsample = Upsample(cfg, cur)
                res *= 2
            ups.insert(0, stage)
        self.up = nn.ModuleList(ups)

        self.temb_slices = temb_slices
        self.temb = nn.Module()
        self.temb.dense = nn.ModuleList([nn.Linear(ch, self.temb_ch), nn.Linear(self.temb_ch, self.temb_ch),
                                         nn.Linear(self.temb_ch, sum(temb_slices))])
        self.norm_out = nn.GroupNorm(cfg.groups, cur, eps=cfg.eps)
        self.conv_out = nn.Conv2d(cur, cfg.out_ch, 3, 1, 1)

    def set_plain_dense(self, plain: bool):
        """full mode = stock dense U-Net (F.group_norm, no cache bookkeeping)."""
        for m in self.modules():
            if isinstance(m, (ResBlock, AttnBlock, Upsample, Downsample)):
                m.plain = plain
        self.conv_in._plain_model = plain  # (the stock baseline keeps torch's first / last conv and GroupNorm)

    def _temb(self, t):
        if self.mode != "full":
            return None  # folded into the cached shifts
        e = timestep_embedding(t, self.ch)
        e = F.silu(self.temb.dense[0](e))
        e = F.silu(self.temb.dense[1](e))
        return list(torch.split(self.temb.dense[2](e), self.temb_slices, dim=1))

    # ---- the first conv of a sparse pass, on the active windows only (round 6) ------------------------------------------------------
    # hs[0] = conv_in(x) is read by down[0].block[0] and, as a skip, by the last block of up[0] (sige_fused_unet.py:395-400, 419-424):
    # both are tiled at this resolution with the same index list, so a sparse forward only ever looks at conv_in's output through
    # those 6x6 Gather windows (which contain the 4x4 shortcut windows).  The reference computes it densely because it is cheap there;
    # here it is 33.5 MB written per forward (17 us, write-bandwidth-bound) for a 1.2 % edit that reads 6 % of them.  The output
    # buffer is persistent; what lies outside the active windows is stale and unread.
    SPARSE_CONV_IN = True

    def _conv_in(self, x, native_full):
        if self.mode != "sparse" and not native_full:
            return self.conv_in(x)
        if self.mode == "sparse" and self.SPARSE_CONV_IN and self.edit_batch == 1 and x.is_cuda:
            first, last = self.down[0].block[0], self.up[0].block[-1]
            g0, g1 = getattr(first, "main_gather", None), getattr(last, "main_gather", None)
            if (g0 is not None and g1 is not None and g0.active_indices is not None and g1.active_indices is not None
                    and tuple(g0.block_size) == tuple(g1.block_size) and tuple(g0.offset) == tuple(g1.offset)
                    and tuple(g0.model_stride) == (1, 1) and tuple(g1.model_stride) == (1, 1)
                    # (one index list for both: set_masks memoises the lists per (resolution, block, stride, offset) key -- no comparison
                    #  of contents here: that would be a device -> host sync inside a capture)
                    and g0.active_indices.data_ptr() == g1.active_indices.data_ptr()):
                buf = getattr(self, "_h0_buf", None)
                shape = (x.shape[0], self.conv_in.out_channels, x.shape[2], x.shape[3])
                if buf is None or tuple(buf.shape) != shape or buf.device != x.device:
                    buf = self._h0_buf = torch.zeros(shape, dtype=torch.float32, device=x.device).contiguous(memory_format=torch.channels_last)
                return input_conv2d(self.conv_in, x, tiles=(g0.active_indices, tuple(g0.block_size)), out=buf)
        return input_conv2d(self.conv_in, x)

    # ---- a dense up level in front of a tiled Upsample, on the cells that Upsample reads ---------------------------
    # `Upsample` is always a SIGE layer; where its gather fuses the upsampling, a sparse pass reads the half-resolution output of
    # the level below it ONLY through that gather's 6x6 windows, and backwards through the level's 3x3 convs the needed region
    # grows by one pixel per conv.  A level that is dense, has no attention (keys and values need every pixel) and feeds nothing
    # else therefore computes, conv by conv, only the 4x4 cells that intersect its region (hip.DemandTiles: built on the device
    # behind the index compactions of set_masks).  The outputs and twins of its convs are persistent buffers; outside the cells
    # of the current mask they are stale and unread.  False: every tile, as before (A/B runs, tests).
    DENSE_ON_DEMAND = True

    def _demand_stages(self):
        """[(name, stage)]: the up levels that can run on their demand regions whatever the mask -- dense, no attention, output
        to a tiled Upsample only, and wider than the region of the level's first conv can grow (2 pixels per ResBlock on each
        side of a window: a level no wider than that is covered by any edit -- the 8x8 level of DDPM-256)."""
        out = []
        for lvl, stage in enumerate(self.up):
            up = getattr(stage, "upsample", None)
            if up is None or len(stage.attn) or up.gather.input_res is None:
                continue
            if any(b.sparse_main or not b.preactivate or b.overlap for b in stage.block):
                continue
            if min(up.gather.input_res) // 2 <= 4 * len(stage.block):
                continue
            out.append(("up.%d" % lvl, stage))
        return out

    def _demand_requests(self, masks):
        if not self.DENSE_ON_DEMAND or self.edit_batch != 1:
            return []
        reqs = []
        for name, stage in self._demand_stages():
            g = stage.upsample.gather
            res = tuple(g.input_res)
            mask = masks.get(res)
            if mask is None or not mask.is_cuda or mask.dim() != 2 or res[0] % 2 or res[1] % 2 or tuple(g.model_stride) != (1, 1):
                continue
            reqs.append((name, g, True, (res[0] // 2, res[1] // 2), 2 * len(stage.block)))
        if reqs:
            from .. import hip

            if hip.get_edit_batch() != 1:  # (sige_amd.stacked.set_masks: masks E images tall -- stacked edits run every tile)
                return []
        return reqs

    def _stage_demand(self, lvl: int, stage, h):
        """The demand regions the dense level `stage` runs on in this forward, or None (every tile): sparse mode, channels-last
        fp32 tensors on the GPU, one edit, exact-fp32 convs, and the Upsample above it reading `h`-like tensors through its
        fused gather."""
        if not (self.DENSE_ON_DEMAND and self.mode == "sparse" and self.edit_batch == 1 and isinstance(h, torch.Tensor) and h.is_cuda):
            return None
        region = getattr(self, "_demand_lists", {}).get("up.%d" % lvl)
        if region is None or h.shape[0] != 1:
            return None
        from .. import hip

        convs = [c for b in stage.block for c in (b.conv1, b.conv2, getattr(b, "nin_shortcut", None)) if c is not None]
        if not hip.is_cl(h) or any(getattr(c, "compute_dtype", "f32") != "f32" for c in convs):
            return None
        g = stage.upsample.gather
        if not g.fuses_upsample(h) or tuple(g.input_res) != (2 * h.shape[2], 2 * h.shape[3]):
            return None
        return region

    # ---- a dense down level behind a tiled Downsample, on the cells an edit can change ----------------------------
    # A sparse pass runs the dense blocks on the CACHED GroupNorm affines, so each of their convs is a local operator, and the
    # level's input -- the persistent output of the tiled Downsample above it -- equals the original's outside the tiles S0 that
    # Downsample's Scatter writes.  The k-th 3x3 conv of the level can therefore differ from the original's values only on S_k =
    # S0 dilated k times by one pixel (hip.ChangeTiles: built on the device behind the index compactions of set_masks): conv1 of
    # block i runs the cells of S_{2i+1}, conv2 and a shortcut those of S_{2i+2}.  Unlike the demand regions above, what lies
    # outside the lists IS read (the level's Downsample, the up path's skips, the 6x6 windows of the next conv): outputs and twins
    # are persistent buffers per cache id that hold the values derived from the current original there.  That is established by
    # running the level on EVERY cell into those buffers -- in front of the lists in the first forward after anything they derive
    # from has changed (`_change_signature`), `refresh_change_stages()` behind a launch plan's restore of the Scatter outputs, and
    # `rebuild_derived_caches()` after an in-place rewrite of the cache.  False: every tile, fresh tensors (A/B runs, tests).
    DENSE_ON_CHANGE = True

    # ---- the skip half of a dense up level's conv1, computed behind the small launches of the levels below ---------
    # conv1 of an up block reads cat(h, skip); on the cached affine with activated twins it splits into W[:, :ch] * act(h) + b and
    # W[:, ch:] * act(skip), and the second depends on the down path only.  Once the down blocks of such a level are done, its skip
    # products are queued as side convs (hip.conv_side_begin) in the order the up path consumes them; the single 3x3 launches of
    # the levels below -- half a chip of workgroups each -- take their blocks along, and the up block's conv1 runs over half the K
    # with the product as its residual.  False: today's launches exactly.
    SIDE_SKIP_PRODUCTS = True

    def _side_levels(self):
        """The up levels whose skip products are submitted: dense, with a level below them (its launches are the hosts), and no
        demand stage -- whether or not DENSE_ON_DEMAND is on: with the flag off such a level runs every tile, but its products would
        take the hosts of the levels below it first and leave the others' to launches of their own."""
        demand = {name for name, _ in self._demand_stages()}
        out = []
        for lvl, stage in enumerate(self.up):
            if lvl >= self.num_levels - 1 or any(b.sparse_main for b in stage.block):
                continue
            if ("up.%d" % lvl) in demand or ("up.%d" % lvl) in (getattr(self, "_demand_lists", None) or {}):
                continue
            out.append(lvl)
        return out

    def _submit_side_products(self, lvl: int, hs):
        """Behind the blocks of down[lvl]: hs[-1], hs[-2], ... are the skips of up[lvl].block[0], [1], ..."""
        blocks = self.up[lvl].block
        for block in blocks:
            block.__dict__.pop("_side_product", None)  # (nothing of an earlier forward survives)
        if not (self.SIDE_SKIP_PRODUCTS and self.mode == "sparse" and self.edit_batch == 1 and lvl in self._side_levels()):
            return
        if len(hs) < len(blocks) or not all(isinstance(h, torch.Tensor) and h.is_cuda for h in hs[-len(blocks):]):
            return
        for i, block in enumerate(blocks):
            block.submit_side_product(hs[-1 - i])

    def _change_stages(self):
        """[(level, stage, the Downsample that feeds it)]: dense, no attention, input from a tiled Downsample, and wider than
        its region can grow (2 pixels per ResBlock on each side of a written tile)."""
        out = []
        for lvl in range(1, len(self.down)):
            stage, prev = self.down[lvl], getattr(self.down[lvl - 1], "downsample", None)
            if prev is None or not prev.sparse or len(stage.attn) or prev.gather.input_res is None:
                continue
            if any(b.sparse_main or not b.preactivate or b.overlap for b in stage.block):
                continue
            if min(prev.gather.input_res) // 2 <= 4 * len(stage.block):
                continue
            out.append((lvl, stage, prev))
        return out

    def _change_requests(self, masks):
        if not self.DENSE_ON_CHANGE or self.edit_batch != 1:
            return []
        reqs = []
        for lvl, stage, prev in self._change_stages():
            g = prev.gather
            res = tuple(g.input_res)
            mask = masks.get(res)
            if mask is None or not mask.is_cuda or mask.dim() != 2 or res[0] % 2 or res[1] % 2 or tuple(g.model_stride) != (2, 2):
                continue
            reqs.append(("down.%d" % lvl, g, (res[0] // 2, res[1] // 2), 2 * len(stage.block)))
        if reqs:
            from .. import hip

            if hip.get_edit_batch() != 1:  # (stacked edits run every tile)
                return []
        return reqs

    def _change_signature(self, lvl: int, stage, h):
        """Everything the level's persistent buffers are derived from, the current edit aside: the mask, the producer's
        persistent output and the generation of its cache, the cached affines (tensors and generation: a full pass, clear_cache,
        pack_caches) and the registered twins of every block.  A forward whose signature differs from the one the buffers were
        built under runs every cell."""
        cid = stage.block[0].cache_id
        sct = self.down[lvl - 1].downsample.scatter
        blocks = tuple((b._aff_gen, tuple(v.data_ptr() for v in b.affine[cid]), tuple(b._my_twins())) for b in stage.block)
        return (self.timestamp, h.data_ptr(), tuple(h.shape), str(h.device), sct._out_bufs.gen.get(cid, 0), blocks)

    @staticmethod
    def _change_buffers(stage, cid):
        """The persistent outputs and twins of the level's convs for cache id `cid`, by name and address: a buffer that is new
        (or gone) holds nothing outside the lists yet."""
        out = []
        for b in stage.block:
            for conv in (b.conv1, b.conv2, getattr(b, "nin_shortcut", None)):
                for name, buf in (conv.__dict__.get("_sige_demand_bufs", {}) if conv is not None else {}).items():
                    if name == ("out", cid) or (isinstance(name, BufferName) and cache_id_of(name.key) == cid):
                        out.append((id(conv), repr(name), buf.data_ptr()))
        return tuple(out)

    def _stage_change(self, lvl: int, stage, h, refresh: bool = False):
        """For the dense down level `stage` in this forward: (per-block lists, None) where its buffers are built, (per-block
        every-cell lists, (state key, signature)) where they have to be built first (`refresh`: in any case), or None (every
        tile, fresh tensors): sparse mode, channels-last fp32 on the GPU, one edit, exact-fp32 convs, batch 1."""
        if not (self.DENSE_ON_CHANGE and self.mode == "sparse" and self.edit_batch == 1 and isinstance(h, torch.Tensor) and h.is_cuda):
            return None
        region = getattr(self, "_change_lists", {}).get("down.%d" % lvl)
        if region is None or h.shape[0] != 1 or len(region.main) != 2 * len(stage.block):
            return None
        from .. import hip

        convs = [c for b in stage.block for c in (b.conv1, b.conv2, getattr(b, "nin_shortcut", None)) if c is not None]
        if not hip.is_cl(h) or h.dtype != torch.float32 or any(getattr(c, "compute_dtype", "f32") != "f32" for c in convs):
            return None
        # (`sparse_update` on the reference's route rewrites the producer's cache mid-forward; where the model commits through the
        #  queue -- nn/commit.py -- the level's buffers simply are the new base: original values outside the region, the accepted
        #  edit's inside, and the signature below does not move)
        if any((b.sparse_update and b.commit_queue is None) or b.mode != "sparse" for b in stage.block):
            return None
        g = self.down[lvl - 1].downsample.gather
        if tuple(g.input_res) != (2 * h.shape[2], 2 * h.shape[3]) or region.cells != -(-h.shape[2] // 4) * -(-h.shape[3] // 4):
            return None
        cid = stage.block[0].cache_id
        self.__dict__.setdefault("_change_inputs", {})[(lvl, cid)] = h  # (persistent: the producer Scatter's output buffer)
        planned = hip.plan_recorder() is not None
        counts = region.counts
        if not planned and not refresh and (counts[0] == 0 or counts[0] == region.cells):
            return None  # (nothing written, or every list holds every cell: the launches of the all-tiles forward exactly)
        sig = self._change_signature(lvl, stage, h)
        state = self.__dict__.setdefault("_change_state", {})
        if refresh or state.get((lvl, cid)) != (sig, self._change_buffers(stage, cid)):
            every = (hip.all_tiles(h.shape[2], h.shape[3], (4, 4), (1, 1), (1, 1), h.device),
                     hip.all_tiles(h.shape[2], h.shape[3], (4, 4), (1, 1), (0, 0), h.device))
            per_block = []
            for _ in stage.block:
                r = hip.DemandTiles([every[0]] * 2, [every[1]] * 2, region.cells)
                r.tag, r.keep = cid, True
                per_block.append(r)
            state.pop((lvl, cid), None)
            return per_block, ((lvl, cid), sig)
        return self._change_steady(stage, region, cid), None

    @staticmethod
    def _change_steady(stage, region, cid):
        """The lists of each block of a level whose buffers are built (S_k = main[k - 1]): conv2 / shortcut of block i on
        S_{2i+2}, conv1 on S_{2i+1}."""
        from .. import hip

        per_block = []
        for i in range(len(stage.block)):
            r = hip.DemandTiles([region.main[2 * i + 1], region.main[2 * i]], [region.flat[2 * i + 1], region.flat[2 * i]], region.cells)
            r.tag, r.keep = cid, False
            per_block.append(r)
        return per_block

    def refresh_change_stages(self):
        """Run every change-region level on all cells, into its persistent buffers, from the input its last forward had: the
        Scatter outputs it derives from were restored to the original's (LaunchPlan: recorded behind `refresh_outputs`, so that
        `bind_mask` replays it) or re-copied from a cache rewritten in place (`rebuild_derived_caches`).  Same addresses: graphs
        and plans captured earlier stay valid."""
        inputs = self.__dict__.get("_change_inputs", {})
        state = self.__dict__.setdefault("_change_state", {})
        for (lvl, cid), h in list(inputs.items()):
            stage = self.down[lvl]
            state.pop((lvl, cid), None)
            if stage.block[0].cache_id != cid or cid not in stage.block[0].affine:
                continue  # (another cache id is current: that one's buffers are rebuilt by its next forward)
            found = self._stage_change(lvl, stage, h, refresh=True)
            if found is None:
                continue
            per_block, (key, sig) = found
            with torch.no_grad():
                built = self._change_build(lvl, stage, h, per_block, sig)
            if built is not None:
                state[key] = (built, self._change_buffers(stage, cid))

    def _change_build(self, lvl: int, stage, h, per_block, sig):
        """Every cell of the level into its persistent buffers.  A block that meets its input for the first time registers its
        activated twin with the block in front of it WHILE this runs, and the twin's buffer then exists only from the next launch of
        that block on: the run is repeated until the signature stands.  Returns the signature the buffers are built under, or None
        (it did not settle)."""
        for _ in range(3):
            x = h
            for i, block in enumerate(stage.block):
                x = block(x, None, demand=(per_block[i], 0))
            after = self._change_signature(lvl, stage, h)
            if after == sig:
                return sig
            sig = after
        return None

    def rebuild_derived_caches(self):
        # (parallel.refresh_derived: caches rewritten in place, Scatter outputs re-copied -- the levels' buffers follow)
        self.refresh_change_stages()

    def clear_cache(self):
        super().clear_cache()
        self.__dict__.pop("_change_inputs", None)
        self.__dict__.pop("_change_state", None)

    def forward(self, x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        assert x.shape[2] == x.shape[3] == self.resolution
        temb = self._temb(t)
        nxt = (lambda: temb.pop(0)) if temb is not None else (lambda: None)

        from ..nn import dense as _dense

        # the full pass on the library's kernels (compute dtype "f16" / "f16x3", or dense.FULL_PASS_F32_NATIVE) also takes the
        # library's first / last conv and output norm -- the same launches the sparse pass uses
        native_full = self.mode == "full" and x.is_cuda and not getattr(self.conv_in, "_plain_model", False) and (
            getattr(self.conv_out, "compute_dtype", "f32") != "f32" or _dense.FULL_PASS_F32_NATIVE)
        h0 = self._conv_in(x, native_full)
        if x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous():
            h0 = h0.contiguous(memory_format=torch.channels_last)  # (MIOpen may hand back NCHW for 3 input channels)
        E = self.edit_batch
        if E > 1:
            # stacked edits (sige_amd/stacked.py): x is [E,3,H,W]; from here to the output norm every tensor is the tall image
            # [1,C,E*H,W] -- the same bytes -- and every sparse module works on it unchanged
            if self.mode != "sparse" or x.shape[0] != E:
                raise RuntimeError("stacked edits: sparse mode, one input image per edit")
            if self.__dict__.get("_commit_queue") is not None:
                raise RuntimeError("stacked edits: sparse_update is not supported -- E edits of one original cannot all become the original")
            from ..stacked import tall, untall

            h0 = tall(h0)
        hs = [h0]
        for lvl, stage in enumerate(self.down):
            change = self._stage_change(lvl, stage, hs[-1]) if lvl else None
            if change is not None and change[0][0].keep:
                # the level's buffers are not built for this signature: every cell first, then the lists like any later forward --
                # so that this forward's result is, bit for bit, what the steady forwards (and a graph of one) compute
                # (a capture in this state records the every-cell launches in front of the lists: its replays are right under any
                #  later state of the buffers, and nothing has run yet, so the buffers do not count as built)
                key, sig = change[1]
                built = self._change_build(lvl, stage, hs[-1], change[0], sig)
                if built is not None:
                    if not torch.cuda.is_current_stream_capturing():
                        self._change_state[key] = (built, self._change_buffers(stage, key[1]))
                    change = (self._change_steady(stage, self._change_lists["down.%d" % lvl], key[1]), None)
            for i, block in enumerate(stage.block):
                h = block(hs[-1], nxt()) if change is None else block(hs[-1], nxt(), demand=(change[0][i], 0))
                if len(stage.attn):
                    h = stage.attn[i](h)
                hs.append(h)
            self._submit_side_products(lvl, hs)
            if lvl != self.num_levels - 1:
                hs.append(stage.downsample(hs[-1]))

        h = self.mid.block_1(hs[-1], nxt())
        h = self.mid.attn_1(h)
        h = self.mid.block_2(h, nxt())

        for lvl in reversed(range(self.num_levels)):
            stage = self.up[lvl]
            region = self._stage_demand(lvl, stage, h)
            for i, block in enumerate(stage.block):
                if region is not None:  # (conv2 of block i is 2 * (blocks after it) convs in front of the level's output)
                    h = block((h, hs.pop()), nxt(), demand=(region, 2 * (len(stage.block) - 1 - i)))
                else:
                    h = block((h, hs.pop()), nxt())
                if len(stage.attn):
                    h = stage.attn[i](h)
            if lvl != 0:
                h = stage.upsample(h)
        if self.mode == "sparse" or native_full:
            if E > 1:
                h = untall(h, E)  # (the output norm and the last conv are per image)
            # the output norm is a TRUE GroupNorm of the edited activation (sige_fused_unet.py:430-432)
            so, to = group_norm_affine(h, self.norm_out)
            out = fused_conv2d(self.conv_out, h, so, to, "swish")
            self.flush_commit()  # (an accepted edit: behind every reader of a cache in stream order)
            return out
        return self.conv_out(F.silu(self.norm_out(h)))

