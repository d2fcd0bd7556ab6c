"""The activated-twin protocol (sige_amd/nn/twins.py) on the CPU: what a registry answers, what a launch serves, and the
model-wide invalidation.

The expected answers were recorded on the commit BEFORE the protocol moved into twins.py, through that commit's own classes
(scatter._TwinBuffers / scatter.twins_for, _TwinProducer.register_twin / _my_twins, fused_conv2d with emulated twins, the
invalidation loop of stacked.unstack_caches), with the keys as bare 4-tuples -- a TwinKey compares equal to one.  They pin the
behaviour; they do not restate the new code.
"""
import contextlib
import warnings

import pytest
import torch

from sige_amd.nn import Gather, Scatter, SIGEConv2d, twins
from sige_amd.nn.dense import fused_conv2d
from sige_amd.nn.twins import TwinKey
from sige_amd.workloads.ddpm_unet import AttnBlock, DDPMConfig, DDPMSparseUNet, Downsample, ResBlock

# (the small model of test_host_logic.py::test_conv1_twins_host_logic_on_the_oracle_backend)
CFG = DDPMConfig(ch=32, ch_mult=(1, 2, 2, 4), num_res_blocks=2, attn_resolutions=(16,), resolution=64, sparse_threshold=32, groups=8)
SC, SH = torch.arange(8.0) / 8 + 0.5, torch.arange(8.0) / 4 - 1


def K(part, cache_id):
    return TwinKey(1234, part, 0, cache_id)


class _Owner:
    """One face for the two owners of a registry: a Scatter's `twins`, and a dense producer module."""

    def __init__(self, kind):
        if kind == "scatter":
            with _quiet():
                self.mod = Scatter(Gather(SIGEConv2d(8, 8, 3, 1, 1), 6))
            self.register, self.unregister = self.mod.twins.register, self.mod.twins.unregister
        else:
            self.mod = AttnBlock(CFG, 32, sparse=False) if kind == "attn" else Downsample(CFG, 32, sparse=False)
            self.register, self.unregister = self.mod.register_twin, self.mod.unregister_twin

    def serving(self, cache_id):
        if isinstance(self.mod, Scatter):
            return list(self.mod.twins.serving(cache_id))
        self.mod.cache_id = cache_id
        return list(self.mod._my_twins())


@contextlib.contextmanager
def _quiet():
    with warnings.catch_warnings():  # (Gather: "Change the block size from (6, 6) to (5, 5)")
        warnings.simplefilter("ignore")
        yield


@pytest.fixture(params=["scatter", "attn", "down"])
def owner(request):
    return _Owner(request.param)


def test_registry_limit_is_per_cache_id(owner):
    assert owner.register(K(0, 0), SC, SH) and owner.register(K(1, 0), SC, SH)
    assert not owner.register(K(2, 0), SC, SH)        # a third key for the same cache id is refused
    assert owner.register(K(0, 1), SC, SH)            # a third key for another cache id is accepted
    assert owner.register(K(1, 0), SC * 2, SH)        # re-registering an existing key is accepted
    assert owner.serving(0) == [K(0, 0), K(1, 0)] and owner.serving(1) == [K(0, 1)] and owner.serving(2) == []
    assert owner.serving(0) == [(1234, 0, 0, 0), (1234, 1, 0, 0)]  # (positional access and tuple equality stand)
    owner.unregister(TwinKey(99, 9, 9, 9))            # unregister of an unknown key is a no-op
    owner.unregister("nobody")
    assert owner.serving(0) == [K(0, 0), K(1, 0)] and owner.serving(1) == [K(0, 1)]


def test_a_key_without_a_cache_id_counts_against_every_id(owner):
    for key in (K(1, 0), K(0, 1)):
        assert owner.register(key, SC, SH)
    got = [owner.register(key, SC, SH) for key in ("plain", K(5, 0), K(1, 1), K(2, 1), K(0, 7), K(1, 7))]
    assert got == [True, False, False, False, True, False]
    assert owner.serving(0) == [K(1, 0), "plain"] and owner.serving(1) == [K(0, 1), "plain"] and owner.serving(7) == ["plain", K(0, 7)]
    # (a bare tuple is not a TwinKey: like "plain", it serves every id)
    owner.unregister("plain")
    assert owner.register((1234, 3, 0, 5), SC, SH) and owner.serving(0) == [K(1, 0), (1234, 3, 0, 5)]


def test_scatter_owner_drops_the_buffer_of_a_re_registered_key():
    tb = _Owner("scatter").mod.twins
    cache = torch.randn(1, 8, 4, 4).contiguous(memory_format=torch.channels_last)
    assert tb.register(K(0, 0), SC, SH) and tb.register(K(1, 0), SC, SH)
    first = tb.launch_args(0, cache, stamp=1)
    assert sorted(tb.bufs) == [K(0, 0), K(1, 0)]
    assert tb.register(K(0, 0), SC * 3, SH)
    assert sorted(tb.bufs) == [K(1, 0)]
    again = tb.launch_args(0, cache, stamp=1)
    assert [k for k, *_ in again] == [K(0, 0), K(1, 0)]  # (registration order)
    assert again[0][1] is not first[0][1] and again[1][1] is first[1][1]
    torch.testing.assert_close(again[0][1], torch.nn.functional.silu(cache * (SC * 3).view(1, -1, 1, 1) + SH.view(1, -1, 1, 1)))
    # with a third key of another cache id present, only the current id's are served
    assert tb.register(K(0, 1), SC, SH)
    assert [k for k, *_ in tb.launch_args(0, cache, stamp=1)] == [K(0, 0), K(1, 0)]
    under1 = tb.launch_args(1, cache, stamp=1)
    assert [k for k, *_ in under1] == [K(0, 1)]
    assert len(under1.args()) == 1 and under1.args()[0][0] is under1[0][1] and list(under1.written()) == [K(0, 1)]


def test_launch_set_of_a_dense_producer():
    """Through fused_conv2d on the CPU, the twins emulated: what the launch serves is what the output is tagged with."""
    torch.manual_seed(0)
    d = Downsample(CFG, 8, sparse=False)
    assert d.register_twin(K(0, 0), SC, SH) and d.register_twin(K(1, 0), SC * 2, SH) and d.register_twin(K(0, 1), SC * 3, SH)
    x = torch.randn(1, 8, 8, 8)
    twins.EMULATE_TWINS = True
    try:
        d.cache_id = 0
        out = fused_conv2d(d.conv, x, pad_bottom_right=True, twins=d._my_twins())
        assert list(out._sige_twins) == [K(0, 0), K(1, 0)]  # two registrations, in registration order; cache id 1's is not served
        assert twins.twin_of(out, K(1, 0)) is out._sige_twins[K(1, 0)] and twins.twin_of(out, K(0, 1)) is None
        assert torch.equal(out._sige_twins[K(1, 0)], torch.nn.functional.silu(out * (SC * 2).view(1, -1, 1, 1) + SH.view(1, -1, 1, 1)))
        d.cache_id = 1
        assert list(fused_conv2d(d.conv, x, pad_bottom_right=True, twins=d._my_twins())._sige_twins) == [K(0, 1)]
        # with an out_affine the set is empty and the tag is {}, not absent: a twin is a function of the raw result
        d.cache_id = 0
        out = fused_conv2d(d.conv, x, pad_bottom_right=True, twins=d._my_twins(), out_affine=(torch.ones(8), torch.zeros(8), "identity"))
        assert hasattr(out, "_sige_twins") and out._sige_twins == {}
        assert fused_conv2d(d.conv, x, pad_bottom_right=True)._sige_twins == {}
    finally:
        twins.EMULATE_TWINS = False


def test_launch_set_rules():
    served = {K(0, 0): (SC, SH), K(1, 0): (SC * 2, SH), "third": (SC, SH)}
    made = []
    tw = twins.LaunchSet(served, lambda key, sc, sh: made.append(key) or torch.zeros(1))
    assert made == [K(0, 0), K(1, 0)] and [k for k, *_ in tw] == made  # (at most two, in order; no buffer for a key not served)
    assert [(sc is a, sh is b) for (_, _, sc, sh), (a, b) in zip(tw, served.values())] == [(True, True)] * 2
    assert list(tw.written()) == made and len(tw.args()) == 2
    empty = twins.LaunchSet(served, lambda *_: made.append("no"), out_affine=(SC, SH, "swish"))
    assert list(empty) == [] and empty.args() is None and empty.written() == {} and "no" not in made
    assert twins.LaunchSet(None, None).args() is None and twins.LaunchSet({}, None).written() == {}
    fresh = twins.LaunchSet.fresh(served, (1, 8, 4, 4), "cpu")
    assert all(b.shape == (1, 8, 4, 4) and b.dtype == torch.float32 and b.is_contiguous(memory_format=torch.channels_last)
               for _, b, _, _ in fresh) and fresh[0][1] is not fresh[1][1]
    # the tag: an empty set REPLACES what a persistent output carried from an earlier launch
    out = twins.tag(torch.zeros(1), {"old": torch.ones(1)}, producer="p")
    assert twins.twin_of(out, "old") is not None and twins.producer_of(out) == "p"
    assert twins.tag(out, empty.written())._sige_twins == {} and twins.producer_of(out) == "p"
    assert twins.twin_of(torch.zeros(1), "old") is None and twins.producer_of(torch.zeros(1)) is None


def test_model_wide_invalidation():
    from oracle import oracle
    from sige_amd import runtime
    from sige_amd.utils import dilate_mask, downsample_mask

    torch.manual_seed(0)
    with _quiet():
        model = DDPMSparseUNet(CFG).eval()
    model.set_scatter_inplace(True)
    blocks = [m for m in model.modules() if isinstance(m, ResBlock)]
    g = torch.Generator().manual_seed(1)
    x0, noise, t = torch.randn(1, 3, 64, 64, generator=g), torch.randn(1, 3, 64, 64, generator=g), torch.zeros(1)
    m = torch.zeros(64, 64, dtype=torch.bool)
    m[10:22, 14:30] = True

    def registrations():
        return sum(len(mod.twins.regs) for mod in model.modules() if isinstance(getattr(mod, "twins", None), twins.Registry)) + \
            sum(len(mod._twin_registry().regs) for mod in model.modules() if isinstance(mod, twins.TwinProducer) and mod._twin_scatter() is None)

    runtime.register_backend("cpu", oracle)
    twins.EMULATE_TWINS = True
    try:
        with torch.no_grad():
            model.set_mode("full")
            model(x0, t)
            model.set_masks(downsample_mask(dilate_mask(m, 5), 8))
            model.set_mode("sparse")
            for _ in range(3):
                out = model(x0 + noise * m, t)
            assert sum(len(b._twin_links) for b in blocks) == 21 and registrations() == 21  # (recorded: 22 blocks)
            gens = [b._aff_gen for b in blocks]
            twins.invalidate(model)
            assert sum(len(b._twin_links) for b in blocks) == 0 and registrations() == 0
            assert all(b._aff_gen == g0 + 1 for b, g0 in zip(blocks, gens))  # every consumer's affine generation has moved
            assert not any(mod.twins.bufs for mod in model.modules() if isinstance(getattr(mod, "twins", None), twins.Registry))
            for _ in range(3):
                again = model(x0 + noise * m, t)
            assert sum(len(b._twin_links) for b in blocks) == 21 and registrations() == 21
            assert torch.equal(again, out)
            # drop_links=False: the caches moved, the affines did not -- links and generations stay
            gens = [b._aff_gen for b in blocks]
            twins.invalidate(model, drop_links=False)
            assert sum(len(b._twin_links) for b in blocks) == 21 and [b._aff_gen for b in blocks] == gens
    finally:
        twins.EMULATE_TWINS = False
        runtime.unregister_backend("cpu")
