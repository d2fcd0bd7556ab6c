"""Multi-GPU use of the sparse path: one edited image per GPU, one process per
GPU, the original image's activation cache distributed with a single RCCL
broadcast over xGMI.

The reference has no multi-device path at all (no
torch.distributed / NCCL call sites).  What shards naturally is the unit of
work -- an edited image: every sparse forward only READS the cache of the
original image (Scatter/ScatterGather/ScatterWithBlockResidual `original_*`
dicts + the models' cached GroupNorm affines) and there is no exchange inside
the forward (halos come from the local cache).  So:

    flat = pack_caches(model)                  # the ORIGINAL cache tensors -> views of ONE buffer
    broadcast_cache(flat, src=0, model=model)  # one collective, ~0.67 GB for DDPM-256; derived caches
                                               # (activated copies, persistent outputs) are rebuilt locally
    my_edits = shard(range(num_edits))         # independent units, no collective

`torch.distributed` backend "nccl" is RCCL on ROCm; "gloo" works for CPU tests.
"""
import time
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from .nn import twins

_ALIGN = 64  # floats; keeps every view 256-byte aligned for 16-byte vector access
_PAD = 64 * 48  # floats: world sizes 1, 2, 3, 4, 6, 8, 12, 16 divide the padded buffer into 256-byte aligned chunks


def cache_slots(model: torch.nn.Module, derived: bool = False) -> List[Tuple]:
    """Where every cached tensor of `model` lives, in module order (identical on every rank that built the same model):
    ("dict", d, key, tuple-index-or-None) or ("attr", module, name, tuple-index-or-None).
    `derived=False` (default) lists only what the full pass produced -- Scatter / ScatterGather / ScatterWithBlockResidual
    `original_*` (incl. the K / V caches of the SD transformer, which are Scatter modules), the models' cached affines
    (`affine` dicts or tuples, `scale` / `shift`) and the cross-attention's `cached_k` / `cached_v` (38 big
    tensors / 673 MB for DDPM-256); `derived=True` adds the activated copies (`activated_outputs`), which every rank can
    recompute from those."""
    return [s[:4] for s in _slots_with_modules(model, derived)]


def _slots_with_modules(model: torch.nn.Module, derived: bool = False) -> List[Tuple]:
    """cache_slots() with the owning module as a fifth element (the pipelined distribution refreshes per module)."""
    slots = []
    attrs = ("original_outputs", "original_residuals") + (("activated_outputs",) if derived else ())
    for m in model.modules():
        for attr in attrs:
            d = getattr(m, attr, None)
            if isinstance(d, dict):
                slots.extend(("dict", d, k, None, m) for k in sorted(d))
        aff = getattr(m, "affine", None)  # workload models keep (scale, shift, ...) tuples here
        if isinstance(aff, dict):
            for k in sorted(aff):
                if isinstance(aff[k], tuple):
                    slots.extend(("dict", aff, k, i, m) for i in range(len(aff[k])))
        elif isinstance(aff, tuple) and all(isinstance(t, torch.Tensor) for t in aff):
            slots.extend(("attr", m, "affine", i, m) for i in range(len(aff)))
        for name in ("scale", "shift", "cached_k", "cached_v"):
            t = m.__dict__.get(name)  # (plain attributes only: not parameters / buffers / sub-modules)
            if isinstance(t, torch.Tensor) and t.dtype == torch.float32:
                slots.append(("attr", m, name, None, m))
    return slots


def _get(slot):
    kind, holder, k, i = slot[:4]
    v = holder[k] if kind == "dict" else getattr(holder, k)
    return v if i is None else v[i]


def _set(slot, value):
    kind, holder, k, i = slot[:4]
    if i is not None:
        cur = list(holder[k] if kind == "dict" else getattr(holder, k))
        cur[i] = value
        value = tuple(cur)
    if kind == "dict":
        holder[k] = value
    else:
        setattr(holder, k, value)


def refresh_derived(model: torch.nn.Module, modules=None) -> None:
    """After the cache tensors were rewritten behind the modules' backs (a collective into the packed buffer):
    re-copy every persistent scatter output (it was a copy of the old cache) and let the model recompute what it
    derives from the cache (`rebuild_derived_caches()` of its modules, e.g. the activated ScatterGather copies) --
    all in place, so that a hipGraph captured before keeps valid addresses.  `modules`: only these (the pipelined
    distribution refreshes a module as soon as the chunks holding its caches have landed)."""
    mods = list(model.modules()) if modules is None else list(modules)
    for m in mods:
        fn = getattr(m, "refresh_outputs", None)
        if fn is not None:
            fn()
    for m in mods:
        fn = getattr(m, "rebuild_derived_caches", None)
        if fn is not None:
            fn()


def pack_caches(model: torch.nn.Module) -> torch.Tensor:
    """Copy every ORIGINAL cache tensor into one flat buffer and re-point the module caches at views of it.  Afterwards
    writing the buffer (e.g. by a broadcast) updates every cache in place (then call refresh_derived, or pass `model` to
    broadcast_cache).  The buffer is fp32 -- or, when the model stores its caches as fp16 (SIGEModel.set_cache_dtype("f16")),
    fp16: the fp16 cache tensors lie in it as they are and the (few, small) fp32 tensors -- the cached GroupNorm affines --
    occupy two elements per value, bit for bit; ONE collective moves both, and nothing is converted on either side of the wire."""
    slots = _slots_with_modules(model)
    if not slots:
        raise RuntimeError("pack_caches: no cached activations -- run the model in `full` mode first")
    tensors = [_get(s) for s in slots]
    for t in tensors:
        if t.dtype not in (torch.float32, torch.float16):
            raise NotImplementedError("cache tensors are fp32 or fp16 (got %s)" % t.dtype)
    half = any(t.dtype == torch.float16 for t in tensors)
    fdt = torch.float16 if half else torch.float32
    es = 2 if half else 4
    per = [(4 // es) if t.dtype == torch.float32 else 1 for t in tensors]  # flat elements per tensor element
    align = _ALIGN * 4 // es   # 256 bytes
    pad = _PAD * 4 // es
    sizes = [(t.numel() * k + align - 1) // align * align for t, k in zip(tensors, per)]
    ref = tensors[0]
    total = (sum(sizes) + pad - 1) // pad * pad  # (see _PAD: distribute_cache splits the buffer evenly over the ranks)
    flat = torch.zeros(total, dtype=fdt, device=ref.device)
    off = 0
    layout = []  # (owning module, first element, one past its last (padded) element, true element count -- in FLAT elements) in module order
    for s, t, size, k in zip(slots, tensors, sizes, per):
        raw = flat[off:off + t.numel() * k]
        if t.dtype != fdt:
            raw = raw.view(t.dtype)  # (fp32 values inside an fp16 buffer: two elements each)
        if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous():
            # keep channels-last caches channels-last: an NHWC block of the flat buffer seen as [B,C,H,W]
            bb, c, h, w = t.shape
            view = raw.view(bb, h, w, c).permute(0, 3, 1, 2)
        else:
            view = raw.view(t.shape)  # (a non-dense view -- e.g. an expanded affine -- is stored dense)
        view.copy_(t)
        _set(s, view)
        layout.append((s[4], off, off + size, t.numel() * k))
        off += size
    twins.invalidate(model)  # (the cache tensors moved, the cached affines with them)
    model.__dict__["_sige_cache_layout"] = (flat.data_ptr(), layout)
    return flat


def checksum(flat: torch.Tensor) -> int:
    """An exact fingerprint of a packed cache (the sum of its 32-bit words as integers): equal on every rank after a
    distribution.  (A floating-point sum would do for an fp32 buffer; an fp16 buffer also carries fp32 bit patterns.)"""
    words = flat.view(torch.int32) if flat.numel() * flat.element_size() % 4 == 0 else flat.view(torch.int16).to(torch.int32)
    return int(words.sum(dtype=torch.int64).item())


def broadcast_cache(flat: torch.Tensor, src: int = 0, group=None, async_op: bool = False, model: torch.nn.Module = None):
    """ONE collective for the whole cache (RCCL broadcast over xGMI on MI355X).  With `model` (and not
    async) the receiving ranks' derived caches are refreshed right after; with `async_op=True` call
    `refresh_derived(model)` after waiting on the returned work handle."""
    work = dist.broadcast(flat, src=src, group=group, async_op=async_op)
    if model is not None and not async_op:
        refresh_derived(model)
    return work


def _global_rank(group, r: int) -> int:
    """P2P peers and broadcast sources are GLOBAL ranks; `src` / chunk owners here are ranks of `group`."""
    return r if group is None else dist.get_global_rank(group, r)


# ---- fp16 on the wire -------------------------------------------------------------------------------------------------
# The cached ACTIVATIONS may travel as fp16 (half the bytes over xGMI: 337 instead of 673 MB for DDPM-256): emulated on the CPU
# oracle (profiles/r3_f16_cache_trace.json), a cache rounded to fp16 moves the sparse pass's output by 5e-4 / 5e-4 / 1.6e-3 at
# 1.2 / 5 / 15 % edit -- 0.02-0.07 of what the f16 criterion (sige_amd/tolerance.py) allows, but above the fp32 path's 1e-3 at
# large edits, so it is an option of the f16 compute mode, not a default.  The cached AFFINES (GroupNorm scale / shift: a few
# KB, and the one place where 2^-11 relative is not harmless) always travel in fp32.  Every rank, the source included, ends up
# with the SAME rounded cache: the ranks' results stay bit-identical to each other.
_WIRE_SMALL = 1 << 16  # cache tensors below this many elements stay fp32 on the wire


def _wire_layout(flat: torch.Tensor, model: torch.nn.Module):
    ptr, layout = (model.__dict__.get("_sige_cache_layout", (None, None)) if model is not None else (None, None))
    if layout is None or ptr != flat.data_ptr():
        raise RuntimeError("wire_dtype needs `model` and the buffer pack_caches(model) returned (the layout says which tensors are "
                           "cached affines)")
    small, pos = [], 0
    for _, off, _, n in layout:
        if n < _WIRE_SMALL:
            small.append((off, off + n, pos))  # (first float, one past the last, position in the fp32 side buffer)
            pos += n
    return small, pos


def _wire_send(flat, small, side_n, src, group):
    """The fp16 image of the packed cache (on `src`; elsewhere an empty buffer of the same size) and the fp32 side buffer with the
    small tensors, the latter already distributed."""
    rank = dist.get_rank(group)
    wire = flat.to(torch.float16) if rank == src else torch.empty(flat.numel(), dtype=torch.float16, device=flat.device)
    side = torch.empty(max(side_n, 1), dtype=torch.float32, device=flat.device)
    if rank == src:
        for lo, hi, pos in small:
            side[pos:pos + hi - lo].copy_(flat[lo:hi])
    dist.broadcast(side, src=_global_rank(group, src), group=group)
    return wire, side


def _wire_land(flat, wire, side, small, lo, hi):
    """flat[lo:hi] <- the fp16 piece that has landed, the small tensors inside it from the fp32 side buffer."""
    flat[lo:hi].copy_(wire[lo:hi])
    for a, b, pos in small:
        a2, b2 = max(a, lo), min(b, hi)
        if a2 < b2:
            flat[a2:b2].copy_(side[pos + a2 - a:pos + b2 - a])


def distribute_cache(flat: torch.Tensor, src: int = 0, method: str = "broadcast", group=None,
                     model: torch.nn.Module = None, wire_dtype=None) -> None:
    """Rank `src` (a rank of `group`)'s packed cache to every rank of the group; with `model`, the buffers derived from the
    cache (activated copies, persistent outputs) are refreshed afterwards -- for both methods.

    "broadcast": one RCCL broadcast.  "scatter_allgather": rank `src` sends chunk r of the buffer to rank r (seven
    different xGMI links in parallel on an 8-GPU MI355X node), then one in-place all-gather, in which every link of the
    fully connected node carries 1/N of the buffer at the same time -- xGMI is point-to-point, so a broadcast's ring /
    tree moves the WHOLE buffer over each hop's single link (~4.4 ms vs ~1.3 ms ideal for 673 MB).
    `flat.numel()` must be a multiple of the world size for the second form (pack_caches pads it).
    `wire_dtype=torch.float16` (needs `model`): the activations travel as fp16, see above."""
    world = dist.get_world_size(group)
    if world == 1:
        return
    if method not in ("broadcast", "scatter_allgather"):
        raise ValueError("unknown method %r" % method)
    if wire_dtype not in (None, torch.float32, torch.float16):
        raise ValueError("wire_dtype: torch.float32 or torch.float16")
    if wire_dtype == torch.float16 and flat.dtype == torch.float32:
        small, side_n = _wire_layout(flat, model)
        wire, side = _wire_send(flat, small, side_n, src, group)
        work = _issue(wire, src, method, group, world, async_op=False)
        assert work is None
        _wire_land(flat, wire, side, small, 0, flat.numel())
    else:  # (an fp16-STORED cache already is its wire format)
        work = _issue(flat, src, method, group, world, async_op=False)
        assert work is None
    if model is not None:
        refresh_derived(model)


def _issue(buf: torch.Tensor, src: int, method: str, group, world: int, async_op: bool):
    """One collective over `buf` (a whole packed cache or one chunk of it); returns the work handle when async."""
    if method == "broadcast":
        return dist.broadcast(buf, src=_global_rank(group, src), group=group, async_op=async_op)
    if buf.numel() % world:
        raise RuntimeError("scatter_allgather: buffer of %d elements is not a multiple of the world size %d" % (buf.numel(), world))
    rank = dist.get_rank(group)
    chunk = buf.numel() // world
    mine = buf[rank * chunk:(rank + 1) * chunk]
    # scatter as point-to-point sends (rank `src` keeps its own chunk where it is: no self-send, no aliased buffers)
    if rank == src:
        ops = [dist.P2POp(dist.isend, buf[r * chunk:(r + 1) * chunk], _global_rank(group, r), group) for r in range(world) if r != src]
    else:
        ops = [dist.P2POp(dist.irecv, mine, _global_rank(group, src), group)]
    for work in dist.batch_isend_irecv(ops):
        work.wait()  # (RCCL: a stream dependency, not a host wait)
    return dist.all_gather_into_tensor(buf, mine, group=group, async_op=async_op)  # in place: rank r's input is chunk r of the output


def _refresh_schedule(model: torch.nn.Module, layout, total: int, world: int, n_chunks: int):
    """(chunk bounds, modules to refresh after each chunk) of the pipelined distribution.  A module (and its ancestors: a
    block's derived caches read its children's) is ready once the chunk holding the END of everything its refresh reads has
    landed: its own last cache tensor, and -- for a module that keeps activated twins (scatter._TwinBuffers), which it rebuilds
    as SiLU(scale * cache + shift) with the CONSUMER's cached affine -- the affines of its registered consumers, which sit later
    in module order, for a skip connection at another level of the up path (the twin was rebuilt from the previous
    affine and never refreshed again)."""
    gran = world * _ALIGN
    size = max(gran, ((total + n_chunks - 1) // n_chunks + gran - 1) // gran * gran)
    bounds = [(o, min(o + size, total)) for o in range(0, total, size)]
    parents = {}
    for _, m in model.named_modules():
        for _, c in m.named_children():
            parents[c] = m
    own = {}
    for m, _, e, _ in layout:
        own[m] = max(own.get(m, 0), e)
    by_id = {id(m): m for m in model.modules()}
    needs = dict(own)
    for m in by_id.values():
        regs = getattr(getattr(m, "twins", None), "regs", None)
        for key in (regs or ()):
            consumer = by_id.get(getattr(key, "consumer", None))  # (twins.TwinKey)
            if consumer is not None:
                needs[m] = max(needs.get(m, 0), own.get(consumer, 0))
    end = {}
    for m, e in needs.items():
        node = m
        while node is not None:
            end[node] = max(end.get(node, 0), e)
            node = parents.get(node)
    ready = [[] for _ in bounds]
    for m in model.modules():
        if getattr(m, "refresh_outputs", None) is None and getattr(m, "rebuild_derived_caches", None) is None:
            continue
        e = end.get(m, 0)
        k = next((i for i, (lo, hi) in enumerate(bounds) if e <= hi), len(bounds) - 1)
        ready[k].append(m)
    return bounds, ready


def distribute_cache_pipelined(flat: torch.Tensor, model: torch.nn.Module, src: int = 0, method: str = "scatter_allgather",
                               n_chunks: int = 8, group=None, wire_dtype=None) -> dict:
    """The same result as `distribute_cache(..., model=model)`, pipelined: the packed cache is cut into `n_chunks` pieces in
    MODULE ORDER (pack_caches lays the tensors out in the order the forward uses them), every piece's collective is issued
    asynchronously up front, and as soon as piece k has landed the buffers derived from the modules whose caches are
    complete (activated ScatterGather copies, persistent Scatter outputs, activated twins: ~0.65 GB of local copies for
    DDPM-256) are refreshed on the current stream -- while pieces k+1 ... are still moving over xGMI.  What remains exposed
    is the transfer itself plus the last piece's refresh.  `wire_dtype=torch.float16`: see distribute_cache.
    Returns {"chunks": n, "refreshed": modules refreshed, "wire_bytes": bytes every rank received}."""
    world = dist.get_world_size(group)
    ptr, layout = model.__dict__.get("_sige_cache_layout", (None, None))
    if layout is None or ptr != flat.data_ptr():
        raise RuntimeError("distribute_cache_pipelined: `flat` is not the buffer pack_caches(model) returned")
    if world == 1:
        return {"chunks": 0, "refreshed": 0}
    if method not in ("broadcast", "scatter_allgather"):
        raise ValueError("unknown method %r" % method)
    bounds, ready = _refresh_schedule(model, layout, flat.numel(), world, n_chunks)
    if wire_dtype not in (None, torch.float32, torch.float16):
        raise ValueError("wire_dtype: torch.float32 or torch.float16")
    f16 = wire_dtype == torch.float16 and flat.dtype == torch.float32  # (an fp16-STORED cache already is its wire format)
    if f16:  # (the activations travel as fp16, the cached affines in an fp32 side buffer sent first: see distribute_cache)
        small, side_n = _wire_layout(flat, model)
        wire, side = _wire_send(flat, small, side_n, src, group)
    buf = wire if f16 else flat
    works = [_issue(buf[lo:hi], src, method, group, world, async_op=True) for lo, hi in bounds]
    n = 0
    for k, work in enumerate(works):
        if work is not None:
            work.wait()
        if f16:
            _wire_land(flat, wire, side, small, *bounds[k])
        refresh_derived(model, ready[k])
        n += len(ready[k])
    return {"chunks": len(bounds), "refreshed": n, "wire_bytes": int(buf.numel() * buf.element_size() + (side.numel() * 4 if f16 else 0))}


def max_over_ranks(seconds: float, device=None, group=None) -> float:
    """The slowest rank's time (what a whole-job throughput is quoted on)."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return float(seconds)
    v = torch.tensor([seconds], dtype=torch.float64, device=device if device is not None else "cpu")
    dist.all_reduce(v, op=dist.ReduceOp.MAX, group=group)
    return float(v.item())


WATCHDOG_S = 2.0  # a cache distribution slower than this loses to recomputing the cache (a DDPM-256 full pass is ~4 ms)


def _all_ok(ok: bool, device=None, group=None) -> bool:
    """True iff `ok` on EVERY rank (the ranks must take the same branch after a candidate failed somewhere)."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return bool(ok)
    v = torch.tensor([1 if ok else 0], dtype=torch.int32, device=device if device is not None else "cpu")
    dist.all_reduce(v, op=dist.ReduceOp.MIN, group=group)
    return bool(v.item())


_agree_calls = 0  # (every rank calls choose_distribution the same number of times: the same key prefix on every rank)


def _default_store():
    try:
        return dist.distributed_c10d._get_default_store()
    except Exception:  # noqa: BLE001
        return None


class _StoreAgreement:
    """Status / time exchange between the ranks through the rendezvous store (a TCP key-value server), NOT through the process
    group whose collectives are on trial: a rank whose candidate raised must not enter an all_reduce while the others are still
    inside the candidate's broadcast (mismatched collectives deadlock), and a rank whose candidate hangs cannot answer through
    the communicator it hangs in."""

    def __init__(self, store, rank, world, prefix):
        self.store, self.rank, self.world, self.prefix, self.n = store, rank, world, prefix, 0

    def exchange(self, text: str, timeout_s: float) -> Optional[List[str]]:
        """Every rank's `text`, or None if some rank did not answer within `timeout_s` (it hangs, or it died)."""
        from datetime import timedelta

        self.n += 1
        key = "%s/%d/" % (self.prefix, self.n)
        self.store.set(key + str(self.rank), text)
        keys = [key + str(r) for r in range(self.world)]
        try:
            self.store.wait(keys, timedelta(seconds=timeout_s))
        except Exception:  # noqa: BLE001 -- timeout
            return None
        return [self.store.get(k).decode() for k in keys]


def _run_with_timeout(fn: Callable[[], None], timeout_s: float):
    """fn() on a daemon thread of its own: (finished, error text or None).  A collective that never returns leaves the thread
    blocked inside it; the caller goes on without it (and must not touch the communicator again)."""
    import threading

    box = {}
    dev = torch.cuda.current_device() if torch.cuda.is_available() else None

    def target():
        try:
            if dev is not None:
                torch.cuda.set_device(dev)  # (the current device is per thread)
            fn()
        except BaseException as e:  # noqa: BLE001 -- a collective this RCCL build cannot run must not end the job
            box["err"] = repr(e)[:200]
        box["done"] = True

    th = threading.Thread(target=target, name="sige-distribution-trial", daemon=True)
    th.start()
    th.join(timeout_s)
    if not box.get("done"):
        return False, "no return within %.1f s (hung collective)" % timeout_s
    return True, box.get("err")


def choose_distribution(candidates: Dict[str, Callable[[], None]], recompute: Optional[Callable[[], None]] = None,
                        watchdog_s: float = WATCHDOG_S, repeats: int = 2, device=None, group=None,
                        sync: Optional[Callable[[], None]] = None, clock: Callable[[], float] = time.perf_counter,
                        hang_timeout_s: Optional[float] = None) -> dict:
    """How should the original image's cache reach every rank of THIS job on THIS node?  Decide by measuring, once, at start-up.

    `candidates`: name -> callable that performs one complete distribution (collective + local refresh), tried in order;
    `recompute`: callable with which every rank rebuilds the cache itself (no communication), or None.  Every candidate runs
    once (communicator set-up included) on a thread of its own, with three ways out:
      * SLOW: the run took longer than `watchdog_s` on the slowest rank -> the candidate is out after that one run;
      * RAISED on any rank -> out; the ranks learn of it through the rendezvous store, not through a collective, so the rank that
        raised never enters a collective the others are not in;
      * HUNG: no return within `hang_timeout_s` (default max(60 s, 30 x watchdog_s): well above the slowest collective that does
        finish -- gloo's scatter + all-gather between two ranks sharing one GPU takes 14 s) on any rank -> out, and the communicator counts
        as poisoned: no further collective candidate is tried (a hung collective cannot be cancelled from Python; its thread stays
        blocked, its stream is abandoned), the decision falls to `recompute`, which needs no communication.
    Survivors run `repeats - 1` more times; the figure is the best run, max over ranks.  The fastest survivor wins, `recompute`
    competing like any other; if no candidate survives, `recompute` is the fallback (and if there is none, RuntimeError).  Every
    rank takes the same decision: times and failures are exchanged through the store before they are compared.

    Returns {"method_chosen", "methods_ms": {name: ms or None}, "errors": {name: text}, "fallback": reason or None,
    "watchdog_s", "hang_timeout_s", "poisoned"}.  (VERDICT r4 next #8 / ADVICE r5: RCCL has only run with one rank in this
    project's sessions -- whichever collective this build of it handles badly, slow, raising or hanging, the scaling bench still
    finishes and says which one it used.)"""
    global _agree_calls
    if sync is None:
        sync = (lambda: torch.cuda.synchronize()) if torch.cuda.is_available() else (lambda: None)
    if hang_timeout_s is None:
        hang_timeout_s = max(60.0, 30.0 * watchdog_s)
    multi = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if multi else 1
    rank = dist.get_rank(group) if multi else 0
    agree = None
    if world > 1:
        store = _default_store()
        if store is not None:
            _agree_calls += 1
            agree = _StoreAgreement(store, rank, world, "sige/choose/%d" % _agree_calls)
    state = {"poisoned": False}

    def exchange(ok: bool, dt: float, hung: bool = False):
        """(every rank ok, max time over the ranks); a rank that does not answer = a hang somewhere."""
        if world == 1:
            return ok, dt
        if agree is None:  # (no store: the collectives of the group itself, as before round 6 -- never on a communicator a trial hung in)
            if state["poisoned"] or hung:
                state["poisoned"] = True
                return False, dt
            all_ok = _all_ok(ok, device=device, group=group)
            return all_ok, (max_over_ranks(dt, device=device, group=group) if all_ok else dt)
        # 1 = ran, 0 = raised, 2 = hung here (every rank must then stop using the communicator, not only this one)
        got = agree.exchange("%d %.9f" % (2 if hung else (1 if ok else 0), dt), hang_timeout_s + 5.0)
        if got is None or any(g.split()[0] == "2" for g in got):
            state["poisoned"] = True
            return False, dt
        return all(g.split()[0] == "1" for g in got), max(float(g.split()[1]) for g in got)

    def one_run(fn, is_collective):
        if world > 1 and not state["poisoned"]:
            if agree is not None:
                if agree.exchange("b", hang_timeout_s + 5.0) is None:  # (a barrier that cannot hang in the communicator on trial)
                    state["poisoned"] = True
            else:
                dist.barrier(group=group)
        t0 = clock()

        def trial():
            sync()
            fn()
            sync()

        finished, err = _run_with_timeout(trial, hang_timeout_s) if is_collective else (True, None)
        if not is_collective:
            try:
                trial()
            except Exception as e:  # noqa: BLE001
                err = repr(e)[:200]
        dt = clock() - t0
        if not finished:
            state["poisoned"] = True
        all_ok, worst = exchange(finished and err is None, dt, hung=not finished)
        return (worst if all_ok else None), err

    methods_ms, errors = {}, {}
    todo = [(n, f, True) for n, f in candidates.items()] + ([("recompute", recompute, False)] if recompute is not None else [])
    for name, fn, is_collective in todo:
        if is_collective and state["poisoned"]:
            errors[name] = "skipped: a collective hung before it, the communicator is not used again"
            methods_ms[name] = None
            continue
        first, err = one_run(fn, is_collective)
        if first is None:
            errors[name] = err or ("hung on another rank" if state["poisoned"] else "failed on another rank")
            methods_ms[name] = None
            continue
        if first > watchdog_s and name != "recompute":
            errors[name] = "exceeded the %.1f s watchdog (%.2f s)" % (watchdog_s, first)
            methods_ms[name] = round(first * 1e3, 3)
            continue
        best = first
        for _ in range(max(0, repeats - 1)):
            again, err = one_run(fn, is_collective)
            if again is None:
                errors[name] = err or "failed on another rank"
                best = None
                break
            best = min(best, again)
        methods_ms[name] = None if best is None else round(best * 1e3, 3)
    alive = {k: v for k, v in methods_ms.items() if v is not None and k not in errors}
    if state["poisoned"]:
        alive = {k: v for k, v in alive.items() if k == "recompute"}  # (survivors measured before the hang share its communicator)
    fallback = None
    if not alive:
        raise RuntimeError("choose_distribution: no method worked: %r" % errors)
    chosen = min(alive, key=lambda k: alive[k])
    collectives_alive = [k for k in alive if k != "recompute"]
    if chosen == "recompute" and candidates and not collectives_alive:
        fallback = "every collective failed, hung or exceeded the watchdog: " + "; ".join("%s: %s" % kv for kv in errors.items())
    return {"method_chosen": chosen, "methods_ms": methods_ms, "errors": errors, "fallback": fallback, "watchdog_s": watchdog_s,
            "hang_timeout_s": hang_timeout_s, "poisoned": state["poisoned"]}


def shard(units: Sequence, rank: int = None, world: int = None) -> List:
    """Round-robin assignment of independent units (edited images) to ranks."""
    rank = dist.get_rank() if rank is None else rank
    world = dist.get_world_size() if world is None else world
    return [u for i, u in enumerate(units) if i % world == rank]
