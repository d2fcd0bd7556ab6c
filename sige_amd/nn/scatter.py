"""Scatter / ScatterWithBlockResidual: conv-output tiles back into the cached
full activation.

API parity with sige/nn/scatter.py:9-136 (same attributes: `gather`,
`original_outputs`, `original_residuals`, `output_res`; same full / sparse /
profile behaviour; `sparse_update` refreshes the cache in place).

On the GPU the sparse mode uses the fused single-pass kernels of
libsige_hip.so (tile table + one streaming pass) -- results are bit-identical
to the reference's clone-then-overwrite.
"""
from typing import Optional

import torch

from . import commit, deferred, twins
from .base import SIGEModule, SIGEModuleWrapper
from .gather import Gather


def _fused_ok(x: torch.Tensor) -> bool:
    return x.is_cuda


def hip_is_cl(t: torch.Tensor) -> bool:
    from .. import hip

    return hip.is_cl(t)


def _cl_ok(cached: torch.Tensor, *others) -> bool:
    """Channels-last kernels: a channels-last cache with C % 4 == 0 and full-size operands."""
    if not cached.is_cuda or cached.dtype not in (torch.float32, torch.float16):  # (fp16: SIGEModel.set_cache_dtype)
        return False
    from .. import hip

    if not (hip.is_cl(cached) and cached.shape[1] % 4 == 0):
        return False
    return all(o is None or tuple(o.shape) == tuple(cached.shape) for o in others)


def _fill(buf: torch.Tensor, cached: torch.Tensor, build=None) -> torch.Tensor:
    """buf <- cached (build None) or SiLU(scale * cached + shift) (build = (scale [C], shift [C])).  On the GPU, channels-last:
    ONE library launch (sige_hip_copy_f32 / sige_hip_affine_act_nhwc_f32), which a launch plan records -- a torch copy would
    be invisible to it."""
    if cached.is_cuda and cached.dtype in (torch.float32, torch.float16) and buf.stride() == cached.stride():
        from .. import hip

        if (build is None and (cached.is_contiguous() or cached.is_contiguous(memory_format=torch.channels_last))
                and (cached.dtype == torch.float32 or cached.numel() % 4 == 0)):
            return hip.copy_dense_(buf, cached)  # (an fp16-stored cache is widened on the way)
        if build is not None and hip.is_cl(cached):
            sc, sh = build
            done = hip.affine_act_cl(cached, sc.reshape(1, -1, 1, 1), sh.reshape(1, -1, 1, 1), "swish", out=buf)
            if done is not None:
                return buf
    if build is None:
        buf.copy_(cached)
    else:
        sc, sh = build
        buf.copy_(torch.nn.functional.silu(cached.float() * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)))
    return buf


class _OutputBuffers:
    """Persistent outputs of a Scatter module for the in-place mode (SIGEModel.set_scatter_inplace).

    The reference returns `y.clone()` with the tiles written over it (sige/cpu/scatter.cpp:83):
    two full-tensor passes per call although only the tiles change.  With 288 GB of HBM the
    module keeps, per cache id, one buffer that already equals the cached tensor outside the
    current mask's tiles; a forward then writes the covered pixels only.  The buffer is rebuilt
    (one copy) whenever the cache or the mask changes.  The caller must not modify the returned
    tensor in place, and it is only valid until the module's next forward.

    "The cache changed" is an explicit per-cache-id generation counter, bumped by whoever writes the
    cache (a full-mode forward, `sparse_update`, `parallel.pack_caches` / `broadcast_cache`) --
    not the tensor's address or version: the caching allocator recycles addresses, a fresh tensor
    starts at version 0 and a collective may write a buffer without touching its version."""

    def __init__(self):
        self.bufs = {}
        self.gen = {}

    def get(self, cache_id, cached: torch.Tensor, stamp, build=None):
        """`build`: what a fresh buffer holds -- None: a copy of the cache; (scale [C], shift [C]): SiLU(scale * cache + shift),
        an activated twin."""
        entry = self.bufs.get(cache_id)
        key = (stamp, self.gen.get(cache_id, 0), tuple(cached.shape), cached.stride())
        if entry is None or entry[0] != key:
            if entry is not None and entry[0][1:] == key[1:] and entry[1].device == cached.device:
                # only the MASK changed: restore the buffer in place -- same address, so a launch plan or a captured hipGraph
                # that points at it stays valid, and nothing is allocated.  CONSEQUENCE: a hipGraph captured under an
                # EARLIER mask shares this buffer and does not contain the restore -- after set_masks() graphs of earlier masks
                # are invalid (alternating replays of two masks' graphs would leave the other mask's tiles in the buffer):
                # re-capture per mask (GraphPool / LaunchPlan.capture do), and clone() a model output that must outlive set_masks
                buf = _fill(entry[1], cached, build)
            else:
                # (persistent outputs and twins are fp32 whatever the cache is stored as: they hold this edit's RESULTS)
                buf = _fill(torch.empty_like(cached, dtype=torch.float32, memory_format=torch.preserve_format), cached, build)
            entry = (key, buf, build)
            self.bufs[cache_id] = entry
        return entry[1]

    def invalidate(self, cache_id=None):
        """The cached tensor of `cache_id` (None: of every id) was replaced or rewritten."""
        for k in ([cache_id] if cache_id is not None else set(self.bufs) | set(self.gen)):
            self.gen[k] = self.gen.get(k, 0) + 1
            self.bufs.pop(k, None)

    def refresh(self, caches: dict, stamp=None):
        """The cached tensors were rewritten IN PLACE (same tensors, new values -- e.g. a collective into the packed
        cache), or (`stamp`) the mask changed: rebuild the existing buffers from them, addresses kept -- a captured hipGraph
        or a launch plan may hold them.  `stamp`: the buffers then count as built for that mask."""
        for cid, (key, buf, build) in list(self.bufs.items()):
            cached = caches.get(cid)
            if cached is not None and tuple(cached.shape) == tuple(buf.shape) and cached.stride() == buf.stride():
                _fill(buf, cached, build)
                if stamp is not None:
                    self.bufs[cid] = ((stamp,) + tuple(key[1:]), buf, build)
            else:
                self.bufs.pop(cid)

    def clear(self):
        self.bufs = {}


class _TwinBuffers(twins.Registry):
    """Activated twins of a Scatter module's persistent output (not in the reference; the protocol: sige_amd/nn/twins.py).

    For every registration the fused conv -> scatter launch also writes SiLU(scale * value + shift) for every pixel it writes
    into a second persistent buffer that equals SiLU(scale * cache + shift) elsewhere."""

    def __init__(self):
        super().__init__()   # regs: key -> (scale [C], shift [C])
        self.bufs = {}       # key -> _OutputBuffers

    def register(self, key, scale: torch.Tensor, shift: torch.Tensor) -> bool:
        ok = super().register(key, scale, shift)
        if ok:
            self.bufs.pop(key, None)
        return ok

    def unregister(self, key):
        super().unregister(key)
        self.bufs.pop(key, None)

    def launch_args(self, cache_id, cached: torch.Tensor, stamp) -> twins.LaunchSet:
        """[(key, buffer, scale, shift)] for the fused launch; buffers are (re)built from the cache when stale."""
        return twins.LaunchSet(self.serving(cache_id), lambda key, sc, sh: self.bufs.setdefault(key, _OutputBuffers()).get(
            cache_id, cached, stamp, build=(sc, sh)))

    def invalidate(self, cache_id=None):
        for b in self.bufs.values():
            b.invalidate(cache_id)

    def refresh(self, caches: dict, stamp=None):
        for b in self.bufs.values():
            b.refresh(caches, stamp)

    def clear(self):
        self.bufs = {}

    def unwritten(self, output: torch.Tensor, cache_id) -> torch.Tensor:
        """Tag the output of a launch that wrote no twin: consumers activate for themselves (tests: twins.EMULATE_TWINS)."""
        return twins.tag(output, twins.emulated_twins(output, self.serving(cache_id)) if twins.EMULATE_TWINS else {})


class Scatter(SIGEModule):
    def __init__(self, gather: Gather):
        super(Scatter, self).__init__()
        self.gather = SIGEModuleWrapper(gather)

        self.load_runtime("scatter")
        self.output_res = None
        self.original_outputs = {}
        self.inplace = False
        self._out_bufs = _OutputBuffers()
        self.twins = _TwinBuffers()

    def clear_cache(self):
        self.original_outputs = {}
        self._out_bufs.clear()
        self.twins.clear()

    def refresh_outputs(self, new_mask: bool = False):
        """(sige_amd.parallel) the cache tensors were rewritten in place -- or (`new_mask`, sige_amd.plan) the mask changed:
        persistent outputs follow, addresses kept."""
        stamp = self.gather.module.timestamp if new_mask else None
        self._out_bufs.refresh(self.original_outputs, stamp)
        self.twins.refresh(self.original_outputs, stamp)

    def plan_tables(self):
        """(sige_amd.plan) build, now, the per-mask lookup tables this module's sparse forward would build lazily."""
        g: Gather = self.gather.module
        for cached in self.original_outputs.values():
            if cached.is_cuda and g.active_indices is not None:
                g.tile_table(cached.shape[2:], cached.device)

    def forward_fused(self, conv, tiles: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(not in the reference) `self(conv(tiles), residual)` in ONE launch when the in-place mode is on and `tiles`
        are pending (deferred) channels-last tiles: the conv's epilogue writes into this module's persistent output.
        Falls back to the two-module form otherwise; values are identical."""
        if self.mode == "sparse" and self.inplace and (not self.sparse_update or commit.active(self, self.original_outputs[self.cache_id])):
            g: Gather = self.gather.module
            cached = self.original_outputs[self.cache_id]
            if _cl_ok(cached, residual) and isinstance(tiles, deferred.DeferredTiles) and tiles.spec is not None:
                out = self._out_bufs.get(self.cache_id, cached, g.timestamp)
                tw = self.twins.launch_args(self.cache_id, cached, g.timestamp)
                done = _fused_conv_into(conv, tiles, out, g, residual=residual, twins=tw.args())
                if done is not None:
                    if self.sparse_update:
                        self._queue_commit(done, cached, g)
                    return twins.tag(done, tw.written())
        return self.forward(conv(tiles), residual)

    def _queue_commit(self, out: torch.Tensor, cached: torch.Tensor, g: Gather):
        """(commit.py) an accepted edit: the persistent output's pixels under this mask's tiles become the cache at the end of the
        forward.  Nothing is invalidated -- output and twins then equal the new cache everywhere."""
        self.commit_queue.add(out, cached, g.indices_on(out.device), g.offset, g.model_stride, g.out_tile)

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        self.check_dtype(x, residual)
        self.check_dim(x, residual)
        if self.mode == "sparse":
            x = deferred.resolve(x)
            g: Gather = self.gather.module
            cached = self.original_outputs[self.cache_id]
            if _cl_ok(cached, residual):
                from .. import hip

                queue = self.inplace and commit.active(self, cached)
                out = self._out_bufs.get(self.cache_id, cached, g.timestamp) if (self.inplace and (not self.sparse_update or queue)) else None
                output = hip.scatter_cl(x, cached, g.offset, g.model_stride, g.indices_on(x.device),
                                        g.tile_table(cached.shape[2:], x.device), residual, out=out)
                if queue:
                    self._queue_commit(output, cached, g)
                    return self.twins.unwritten(output, self.cache_id)
            elif _fused_ok(x):
                from .. import hip

                output = hip.scatter_fused(
                    x.contiguous(), deferred.from_cache(cached), g.tile_table(cached.shape[2:], x.device), g.active_indices.size(0),
                    None if residual is None else residual.contiguous())
            else:
                fn = self.native(self.runtime, x)
                output = fn(x.contiguous(), deferred.from_cache(cached).contiguous(), g.offset[0], g.offset[1],
                            g.model_stride[0], g.model_stride[1], g.indices_on(x.device),
                            None if residual is None else residual.contiguous())
            if self.sparse_update and self.inplace and commit.active(self, cached) and deferred.FORCE_ON_CPU:
                # (tests: the protocol without a device -- the persistent output is the result, as the in-place kernels leave it)
                output = self._out_bufs.get(self.cache_id, cached, g.timestamp).copy_(output)
                self._queue_commit(output, cached, g)
            elif self.sparse_update:
                cached.copy_(output)
                self._out_bufs.invalidate(self.cache_id)
                self.twins.invalidate(self.cache_id)
            return self.twins.unwritten(output, self.cache_id)
        if self.mode == "full":
            output = x if residual is None else x + residual
            self.output_res = output.shape[2:]
            self.original_outputs[self.cache_id] = deferred.to_cache(output, self.cache_dtype)
            self._out_bufs.invalidate(self.cache_id)
            self.twins.invalidate(self.cache_id)
            return output
        if self.mode == "profile":
            c = x.shape[1]
            output = torch.full((self.original_outputs[self.cache_id].size(0), c, *self.output_res),
                                fill_value=x[0, 0, 0, 0], dtype=x.dtype, device=x.device)
            if residual is not None:
                output = output + residual
            return output
        raise NotImplementedError("Unknown mode: [%s]!!!" % self.mode)


def _fused_conv_into(conv, tiles, out, g: Gather, residual=None, x1=None, table1=None, twins=None):
    """Run `conv` on the pending (deferred) tiles with its output written straight into `out` at the tile positions of
    gather `g`.  Returns `out`, or None when the combination has no fused kernel."""
    from .. import hip

    spec = tiles.spec if isinstance(tiles, deferred.DeferredTiles) else None
    if spec is None or not spec.get("cl", False) or conv.groups != 1 or tuple(conv.dilation) != (1, 1):
        return None
    if conv.out_channels % 4 or tuple(conv.stride) != tuple(g.model_stride):
        return None
    packed = conv._packed_weights(tiles, True)
    if packed is None:
        return None
    if spec["kind"] == "gather":
        if x1 is not None:
            return None
        phase = None
        if (spec.get("phase") and spec.get("x2") is None and spec["scale"] is None and spec["shift"] is None and spec["act"] == "identity"
                and getattr(packed, "compute", "f32") == "f32" and spec["x"].is_cuda and hip.get_edit_batch() == 1):
            phase = conv.phase_packed()  # (None: not a 3x3 / stride-1 conv)
        more = {}
        if (spec.get("phase3") and spec.get("x2") is None and spec["scale"] is None and spec["shift"] is None and spec["act"] == "identity"
                and spec["x"].is_cuda and getattr(packed, "compute", "f32") == conv.compute_dtype):
            # (Gather.PHASE_UPSAMPLE_TILE3: the keyword exists only on this path, so that off is today's call, argument for argument)
            more["phase3"] = conv.phase_tile3_packed()  # (None: no such kernel for this conv)
        return hip.gather_conv_cl(spec["x"], spec.get("x2"), spec["block"], spec["idx"], spec["scale"], spec["shift"], spec["act"],
                                  packed, conv.bias, conv.out_channels, conv.kernel_size, conv.stride,
                                  full=dict(offset=g.offset, out_res=tuple(out.shape[2:]), residual=residual),
                                  upsample2x=spec.get("up", False), out=out, twins=twins, phase=phase, **more)
    if tuple(conv.kernel_size) != (3, 3) or tuple(conv.stride) != (1, 1):
        return None
    return hip.scatter_gather_conv_scatter_cl(spec["x"], spec["y"], spec["block"], spec["idx"], spec["map"], spec["scale"],
                                              spec["shift"], spec["act"], packed, conv.bias, conv.out_channels,
                                              conv.kernel_size, g.offset, out, residual=residual, x1=x1, table1=table1,
                                              twins=twins)


class ScatterWithBlockResidual(SIGEModule):
    """scatter(main tiles, residual = cached shortcut) + `x1 - y1` correction on the
    shortcut branch's own tiles (sige/nn/scatter.py:66-136)."""

    def __init__(self, main_gather: Gather, shortcut_gather: Gather):
        super(ScatterWithBlockResidual, self).__init__()
        self.main_gather = SIGEModuleWrapper(main_gather)
        self.shortcut_gather = SIGEModuleWrapper(shortcut_gather)

        self.load_runtime("scatter_with_block_residual")
        self.scatter_runtime = None
        self.output_res = None
        self.original_outputs = {}
        self.original_residuals = {}
        self.inplace = False
        self._out_bufs = _OutputBuffers()
        self.twins = _TwinBuffers()

    def clear_cache(self):
        self.original_outputs = {}
        self.original_residuals = {}
        self._out_bufs.clear()
        self.twins.clear()

    def refresh_outputs(self, new_mask: bool = False):
        """(sige_amd.parallel) the cache tensors were rewritten in place -- or (`new_mask`, sige_amd.plan) the mask changed:
        persistent outputs follow, addresses kept."""
        stamp = (self.main_gather.module.timestamp, self.shortcut_gather.module.timestamp) if new_mask else None
        self._out_bufs.refresh(self.original_outputs, stamp)
        self.twins.refresh(self.original_outputs, stamp)

    def plan_tables(self):
        """(sige_amd.plan) build, now, the per-mask lookup tables this module's sparse forward would build lazily."""
        for cached in self.original_outputs.values():
            if cached.is_cuda:
                for g in (self.main_gather.module, self.shortcut_gather.module):
                    if g.active_indices is not None:
                        g.tile_table(cached.shape[2:], cached.device)

    def forward_fused(self, conv, tiles: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
        """(not in the reference) `self(conv(tiles), residual)` in ONE launch (see Scatter.forward_fused): `residual` are
        the shortcut conv's tiles; the block-residual correction runs in the conv's epilogue."""
        if self.mode == "sparse" and self.inplace and (not self.sparse_update or commit.active(
                self, self.original_outputs[self.cache_id], self.original_residuals[self.cache_id])):
            mg: Gather = self.main_gather.module
            sg: Gather = self.shortcut_gather.module
            y0 = self.original_outputs[self.cache_id]
            y1 = self.original_residuals[self.cache_id]
            if (_cl_ok(y0, y1) and hip_is_cl(y1) and isinstance(tiles, deferred.DeferredTiles) and tiles.spec is not None
                    and sg.active_indices.size(0) <= mg.active_indices.size(0)):
                out = self._out_bufs.get(self.cache_id, y0, (mg.timestamp, sg.timestamp))
                x1 = deferred.resolve(residual)
                tw = self.twins.launch_args(self.cache_id, y0, (mg.timestamp, sg.timestamp))
                done = _fused_conv_into(conv, tiles, out, mg, residual=y1, x1=x1, table1=sg.tile_table(y0.shape[2:], y0.device),
                                        twins=tw.args())
                if done is not None:
                    if self.sparse_update:
                        self._queue_commit(done, x1, y0, y1, mg, sg)
                    return twins.tag(done, tw.written())
        return self.forward(conv(tiles), residual)

    def _queue_commit(self, out: torch.Tensor, x1: torch.Tensor, y0: torch.Tensor, y1: torch.Tensor, mg: Gather, sg: Gather):
        """(commit.py) an accepted edit, at the end of the forward: the persistent output over the MAIN list and over the SHORTCUT list
        (it differs from the cache on both: out += x1 - y1) becomes the output cache, the shortcut tiles go to the residual cache
        (sige/nn/scatter.py:118-129).  Nothing is invalidated."""
        q, dev = self.commit_queue, out.device
        if x1.is_cuda:
            x1 = x1.contiguous(memory_format=torch.channels_last)  # (what the tile convs write: no copy)
        q.add(out, y0, mg.indices_on(dev), mg.offset, mg.model_stride, mg.out_tile)
        q.add(out, y0, sg.indices_on(dev), sg.offset, sg.model_stride, sg.out_tile)
        q.add(x1, y1, sg.indices_on(dev), sg.offset, sg.model_stride, tuple(x1.shape[2:]), tile_source=True)

    def forward(self, x: torch.Tensor, residual: torch.Tensor, x_is_sum: bool = False) -> torch.Tensor:
        """`x_is_sum` (full mode only, not in the reference): `x` already is main + residual."""
        self.check_dtype(x, residual)
        self.check_dim(x, residual)
        assert not x_is_sum or self.mode == "full"
        if self.mode == "sparse":
            x, residual = deferred.resolve(x), deferred.resolve(residual)
            mg: Gather = self.main_gather.module
            sg: Gather = self.shortcut_gather.module
            y0 = self.original_outputs[self.cache_id]
            y1 = self.original_residuals[self.cache_id]
            res = y0.shape[2:]
            if _cl_ok(y0, y1) and hip_is_cl(y1):
                from .. import hip

                queue = self.inplace and commit.active(self, y0, y1)
                out = self._out_bufs.get(self.cache_id, y0, (mg.timestamp, sg.timestamp)) \
                    if (self.inplace and (not self.sparse_update or queue)) else None
                output = hip.scatter_with_block_residual_cl(
                    x, y0, residual, y1, mg.offset, mg.model_stride, mg.indices_on(x.device), mg.tile_table(res, x.device),
                    sg.indices_on(x.device), sg.tile_table(res, x.device), out=out)
                if queue:
                    self._queue_commit(output, residual, y0, y1, mg, sg)
                    return self.twins.unwritten(output, self.cache_id)
            elif _fused_ok(x):
                from .. import hip

                output = hip.scatter_with_block_residual_fused(
                    x.contiguous(), deferred.from_cache(y0), residual.contiguous(), deferred.from_cache(y1),
                    mg.tile_table(res, x.device), mg.active_indices.size(0),
                    sg.tile_table(res, x.device), sg.active_indices.size(0))
            else:
                fn = self.native(self.runtime, x)
                output = fn(x.contiguous(), deferred.from_cache(y0).contiguous(), residual.contiguous(), deferred.from_cache(y1).contiguous(),
                            mg.offset[0], mg.offset[1], mg.model_stride[0], mg.model_stride[1],
                            mg.indices_on(x.device), sg.indices_on(x.device))
            if self.sparse_update and self.inplace and commit.active(self, y0, y1) and deferred.FORCE_ON_CPU:
                # (tests: the protocol without a device -- the persistent output is the result, as the in-place kernels leave it)
                output = self._out_bufs.get(self.cache_id, y0, (mg.timestamp, sg.timestamp)).copy_(output)
                self._queue_commit(output, residual, y0, y1, mg, sg)
            elif self.sparse_update:
                if self.scatter_runtime is None:
                    self.scatter_runtime = self.load_runtime("scatter", {})
                y0.copy_(output)
                self._out_bufs.invalidate(self.cache_id)
                self.twins.invalidate(self.cache_id)
                if _fused_ok(x):
                    from .. import hip

                    y1.copy_(hip.scatter_fused(residual.contiguous(), deferred.from_cache(y1), sg.tile_table(res, x.device),
                                               sg.active_indices.size(0), None))
                else:
                    fn = self.native(self.scatter_runtime, x)
                    y1.copy_(fn(residual.contiguous(), deferred.from_cache(y1).contiguous(), sg.offset[0], sg.offset[1],
                                sg.model_stride[0], sg.model_stride[1], sg.indices_on(x.device), None))
            return self.twins.unwritten(output, self.cache_id)
        if self.mode == "full":
            # (x_is_sum: the caller's conv already added the residual in its epilogue -- one launch less, one pass less)
            output = x if x_is_sum else x + residual
            self.output_res = output.shape[2:]
            self.original_outputs[self.cache_id] = deferred.to_cache(output, self.cache_dtype)
            cl = self.original_outputs[self.cache_id].is_contiguous(memory_format=torch.channels_last)
            self.original_residuals[self.cache_id] = deferred.to_cache(
                residual.contiguous(memory_format=torch.channels_last) if cl and not residual.is_contiguous() else residual,
                self.cache_dtype)
            self._out_bufs.invalidate(self.cache_id)
            self.twins.invalidate(self.cache_id)
            return output
        if self.mode == "profile":
            c = x.shape[1]
            return torch.full((self.original_outputs[self.cache_id].size(0), c, *self.output_res),
                              fill_value=x[0, 0, 0, 0] + residual[0, 0, 0, 0], dtype=x.dtype, device=x.device)
        raise NotImplementedError("Unknown mode: [%s]!!!" % self.mode)
