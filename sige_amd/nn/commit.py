"""Committing an edit on the fused path (not in the reference): the queue behind `set_sparse_update(True)`.

The reference accepts an edit by running the sparse forward once more with `sparse_update` set; every Scatter,
ScatterWithBlockResidual and ScatterGather then copies its whole result over its cache (sige/nn/scatter.py:59-60,114-129,
scatter_gather.py:65-77).  A model class that opts in (`SIGEModel.COMMIT_TILES`) keeps that forward on the fused kernels instead:
each module QUEUES what has to reach its cache -- the tiles of its persistent output, conv1's raw tiles, the shortcut tiles -- and
the model flushes the queue once, at the end of `forward`, through sige_hip_commit_tiles (csrc/commit_tiles.hip: every record of
the forward in one launch per hip.COMMIT_CAPACITY records).  Within a forward a cache is read only by its own module, and stream
order puts the commit behind every reader, so the caches end up exactly as the reference's module-by-module refresh leaves them.

Persistent outputs and activated twins are NOT invalidated on this path: after the commit they equal the new cache everywhere
(outside the mask's tiles they always did, inside them they hold what was just committed); buffers, addresses and generation stay.

    CommitQueue          the records of one forward; holds the tile tensors until the flush
    active(module, ...)  does this module queue (instead of copying) in this forward?
"""
import torch

from . import deferred


class CommitQueue:
    def __init__(self):
        self.records = []
        self.launches = 0   # of the last flush
        self.flushed = 0    # records of the last flush

    def __len__(self):
        return len(self.records)

    def add(self, src, dst, idx, offset, stride, tile, tile_source=False, scale=None, shift=None):
        from .. import hip

        self.records.append(hip.CommitRecord(src, dst, idx, offset=tuple(offset), stride=tuple(stride), tile=tuple(tile),
                                             tile_source=tile_source, scale=scale, shift=shift))

    def flush(self) -> int:
        """Execute the queued records; returns the number of launches.  The modules checked every record against what the kernel
        takes before queueing it (`active`), so a refusal here is a bug, and the caches were not touched."""
        from .. import hip

        records, self.records = self.records, []
        n = hip.commit_tiles(records) if records else 0
        if n is None:
            raise RuntimeError("sige_amd: the commit of a sparse_update forward was refused by sige_hip_commit_tiles (%d records, "
                               "first: %r); no cache was updated" % (len(records), records[0]))
        self.launches, self.flushed = n, len(records)
        return n

    def require_empty(self, what: str):
        if self.records:
            raise RuntimeError("sige_amd: %s with %d queued cache updates of a sparse_update forward that was never flushed "
                               "(the model's forward ends with flush_commit())" % (what, len(self.records)))


def lifted(module) -> bool:
    """`module` belongs to a model that commits through the queue: its `sparse_update` no longer forbids deferral / fusion."""
    return module.commit_queue is not None


def active(module, *caches) -> bool:
    """Does `module` queue its cache updates in this forward?  The model opted in, sparse mode with `sparse_update` set, and every
    destination is something sige_hip_commit_tiles writes: a channels-last fp32 / fp16 GPU tensor of ONE image with C % 4 == 0, at
    one edit.  (deferred.FORCE_ON_CPU: the tests' stand-in, as for deferral -- the protocol without a device.)"""
    if module.commit_queue is None or not module.sparse_update or module.mode != "sparse":
        return False
    if deferred.FORCE_ON_CPU:
        return True
    from .. import hip

    for c in caches:
        if c is None:
            continue
        if not (c.is_cuda and c.dim() == 4 and c.shape[0] == 1 and c.shape[1] % 4 == 0 and c.dtype in (torch.float32, torch.float16)
                and hip.is_cl(c)):
            return False
    return hip.get_edit_batch() == 1
