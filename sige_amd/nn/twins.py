"""Activated twins of the conv1 inputs: the whole protocol (not in the reference).

A CONSUMER (a residual block) whose conv1 applies a cached GroupNorm affine + SiLU to the output of a PRODUCER registers
(scale, shift) with that producer under a key; every launch of the producer whose epilogue writes the full output tensor
then also writes SiLU(scale * out + shift) -- the "activated twin" -- and the consumer's conv1 stages raw values: the
activation is computed once per element by the producer instead of once per output-channel block by the consumer.  A
consumer that finds no twin activates for itself, so a refused or dropped registration costs time, never correctness.

    TwinKey                    what a registration is made for: consumer, input part, affine generation, cache id
    Registry                   the registrations of one producer: at most MAX per cache id, `serving(cache_id)`
    LaunchSet                  what ONE launch writes: (key, buffer, scale, shift) rows -> the bindings' list, the {key: twin} tag
    tag / twin_of / producer_of   the marks on an output tensor
    TwinProducer, TwinConsumer the two halves, as mixins of the modules
    invalidate(model)          every persistent output, twin and link of a model, after its caches moved

The pointer-level marshalling and validation of a launch's twins is hip._twin_args; the kernels' side is csrc/conv_call.hpp.
"""
from typing import NamedTuple

import torch

MAX = 2  # twins per launch (include/sige_hip.h: two pointer triples) -- a skip tensor has two consumers


class TwinKey(NamedTuple):
    """The registered (scale, shift) is the consumer's cached affine of THAT cache id (one cache per denoising step,
    sige/nn/scatter.py:59-60) and of THAT generation (TwinConsumer._aff_gen)."""
    consumer: int   # id() of the consuming module
    part: int       # which part of its (possibly concatenated) conv1 input
    affine_gen: int
    cache_id: int


def cache_id_of(key):
    """The cache id `key` was registered for.  None -- any key that is not a TwinKey -- applies to every cache id."""
    return key.cache_id if isinstance(key, TwinKey) else None


class Registry:
    """key -> (scale [C], shift [C]) of one producer.  At most MAX registrations per cache id (a key without a cache id counts
    against every id); further ones are refused and those consumers keep activating."""

    def __init__(self):
        self.regs = {}

    def serving(self, cache_id) -> dict:
        """The registrations a launch under `cache_id` serves, in registration order."""
        return {k: v for k, v in self.regs.items() if cache_id_of(k) in (None, cache_id)}

    def register(self, key, scale: torch.Tensor, shift: torch.Tensor) -> bool:
        if key not in self.regs and len(self.serving(cache_id_of(key))) >= MAX:
            return False
        self.regs[key] = (scale, shift)
        return True

    def unregister(self, key):
        self.regs.pop(key, None)


class LaunchSet(list):
    """The twins of ONE launch: rows (key, buffer, scale, shift) for the first MAX of `served` = {key: (scale, shift)}, with
    `buffer(key, scale, shift)` the tensor the launch writes that twin into (persistent, demand buffer or fresh).  Empty when
    the launch has an `out_affine`: a twin is a function of the RAW result, so the primary output must be it."""

    def __init__(self, served, buffer, out_affine=None):
        if served and out_affine is None:  # (most launches serve nobody: that path stays a bare, empty list)
            for key, (sc, sh) in list(served.items())[:MAX]:
                self.append((key, buffer(key, sc, sh), sc, sh))

    @classmethod
    def fresh(cls, served, shape, device, out_affine=None):
        """... into a new channels-last fp32 tensor per twin (dense producers: a fresh twin per forward)."""
        return cls(served, lambda *_: torch.empty(shape, dtype=torch.float32, device=device, memory_format=torch.channels_last),
                   out_affine)

    def args(self):
        """What the bindings take as `twins` (hip._twin_args): [(buffer, scale, shift)] or None."""
        return [(b, sc, sh) for _, b, sc, sh in self] or None

    def written(self) -> dict:
        """{key: twin} once the launch is out: what `tag` attaches to the output."""
        return {key: b for key, b, _, _ in self}


class BufferName(NamedTuple):
    """Name of the persistent twin of a dense conv that runs over partial tile lists (dense.demand_buffer)."""
    key: object


# Tests only (tests/test_host_logic.py, tests/test_twins.py): where a launch cannot write twins itself (no GPU: the CPU path goes
# through the plain Scatter kernels), compute them from the finished output with torch -- the registration / invalidation
# logic of the twins can then be exercised end to end on the oracle backend.  Never set in the product.
EMULATE_TWINS = False


def emulated_twins(out: torch.Tensor, regs: dict) -> dict:
    return {k: torch.nn.functional.silu(out * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) for k, (sc, sh) in list(regs.items())[:MAX]}


def tag(out: torch.Tensor, twins=None, producer=None) -> torch.Tensor:
    """Attach {consumer key: activated twin} and / or the producing module (consumers find their producer through it) to an
    output tensor.  `twins` may be empty: persistent outputs keep their Python object, and a stale entry must not survive a
    launch that did not write it; None leaves the tensor's twins as they are ({} if it has none)."""
    if twins is not None or not hasattr(out, "_sige_twins"):
        out._sige_twins = twins or {}
    if producer is not None:
        out._sige_producer = producer
    return out


def twin_of(t, key):
    """The activated twin written next to `t` for `key`, or None."""
    return getattr(t, "_sige_twins", {}).get(key)


def producer_of(t):
    return getattr(t, "_sige_producer", None)


class TwinProducer:
    """Mixin of the modules whose output is written by a full-tensor conv epilogue and can therefore carry activated twins
    for the conv1 of a consumer (cfg.conv1_twins).  `_twin_scatter()`: the Scatter module that owns the persistent in-place
    output (SIGE layers: persistent twins live next to it, scatter._TwinBuffers), or None (dense layers: a fresh twin per
    forward, from the module's own registry)."""

    def _twin_scatter(self):
        return None

    def _twins_ok(self) -> bool:
        return True

    def _twin_registry(self) -> Registry:
        sct = self._twin_scatter()
        return sct.twins if sct is not None else self.__dict__.setdefault("_twin_regs", Registry())

    def register_twin(self, key, scale: torch.Tensor, shift: torch.Tensor) -> bool:
        return self._twins_ok() and self._twin_registry().register(key, scale, shift)

    def unregister_twin(self, key):
        self._twin_registry().unregister(key)

    def _my_twins(self) -> dict:
        """(dense producers) the registrations this forward serves: those of the current cache id."""
        own = self.__dict__.get("_twin_regs")
        return {} if own is None else own.serving(getattr(self, "cache_id", 0))

    def _produced(self, out: torch.Tensor) -> torch.Tensor:
        """Mark `out` as this module's output of the current sparse forward."""
        return tag(out, producer=self)


class TwinConsumer:
    """Mixin of the module whose conv1 takes activated twins.  The host class provides `mode`, `cache_id` and `preactivate`
    (conv1's input is act(x * scale1 + shift1) of the CACHED affine) and calls `_drop_twin_links()` whenever that affine is
    recomputed or dropped."""

    def _init_twin_consumer(self, use_twins: bool):
        self.use_twins = use_twins
        self._twin_links = {}   # key -> (the producer it registered with, the addresses of the affine it registered)
        self._aff_gen = 0       # bumped when the cached affine is recomputed: old twins are for the old affine

    def _twin_key(self, part: int) -> TwinKey:
        return TwinKey(id(self), part, self._aff_gen, self.cache_id)  # (the registered affine is this cache id's)

    def _drop_twin_links(self):
        for key, (prod, _) in self._twin_links.items():
            prod.unregister_twin(key)
        self._twin_links = {}
        self._aff_gen += 1

    def _twin_inputs(self, parts, s1, t1):
        """The activated twins of this block's conv1 inputs, one per part of the (possibly concatenated) input -- or None
        (then conv1 activates in its staging path, as without twins).  A missing twin is requested from the module that
        produced the part; it exists from the next forward on."""
        if not (self.use_twins and self.preactivate and self.mode == "sparse" and (parts[0].is_cuda or EMULATE_TWINS)):
            return None
        if s1.shape[0] != 1:
            return None  # (per-sample affine: the epilogue's twin vectors are per channel)
        # A registration holds VIEWS of the affine tensors it was made with.  If the cached affine has been re-pointed since
        # (sige_amd.parallel.pack_caches moves every cache tensor into one flat buffer; anything that assigns `affine[cid]`
        # without going through _full), the producers would keep activating with the old tensors: drop every link and start
        # over with the current ones (sparse -> pack_caches -> broadcast gave stale twins, max error 0.18).
        anchor = (s1.data_ptr(), t1.data_ptr())
        if any(a != anchor for k, (_, a) in self._twin_links.items() if k.cache_id == self.cache_id):
            self._drop_twin_links()
        twins, off, complete = [], 0, True
        for i, p in enumerate(parts):
            c = p.shape[1]
            # (the key carries the cache id: a twin registered with cache 1's affine must never serve a forward under cache 0 --
            #  found on the GPU in round 3, max error 1.37)
            key = self._twin_key(i)
            t = twin_of(p, key)
            if t is None:
                complete = False
                prod = producer_of(p)
                if prod is not None and key not in self._twin_links:
                    sc = s1.reshape(-1)[off:off + c].contiguous()
                    sh = t1.reshape(-1)[off:off + c].contiguous()
                    if prod.register_twin(key, sc, sh):
                        self._twin_links[key] = (prod, anchor)
            twins.append(t)
            off += c
        return twins if complete else None


def invalidate(model: torch.nn.Module, drop_links: bool = True) -> None:
    """The cached tensors of `model` were replaced or moved (sige_amd.stacked, parallel.pack_caches): persistent outputs and
    their twins are rebuilt on next use.  `drop_links`: the cached affines moved too -- twins were registered with VIEWS of
    the old affine tensors (a consumer's conv1 affine, held by its producers), so the registrations go; the consumers register
    again, with the current tensors, on their next sparse forward (sparse -> pack -> broadcast otherwise serves
    twins of the OLD affine -- 0.18 max error on the oracle backend)."""
    for m in model.modules():
        for bufs in (getattr(m, "_out_bufs", None), getattr(m, "twins", None)):
            if hasattr(bufs, "invalidate"):
                bufs.invalidate()
        if drop_links and isinstance(m, TwinConsumer):
            m._drop_twin_links()
