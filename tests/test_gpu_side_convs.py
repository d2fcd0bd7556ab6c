"""On the MI355X: deferred "side" convs (sige_hip_conv_side_begin / _flush) -- a queued 3x3 conv whose blocks run
inside later 3x3 launches.  Host conv: 8x8 image, 64 -> 32 channels (4 tiles, 8 workgroups); side conv: 16x16 image, 32 -> 64
channels (16 tiles: 64 blocks of 16 x 16, 32 of 16 x 32).  Every result is compared bit for bit with the same conv launched
alone; every uninitialised allocation is NaN."""
import pytest
import torch
from torch import nn

from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    from sige_amd import hip as h

    h.lib()
    return h


def _cl(t):
    return t.to(DEV).contiguous(memory_format=CL)


def _conv(cin, cout, k=3, seed=0, bias=True):
    gen = torch.Generator().manual_seed(100 * cin + cout + seed)
    conv = nn.Conv2d(cin, cout, k, 1, k // 2, bias=bias)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) / (cin * k * k) ** 0.5)
        if bias:
            conv.bias.copy_(torch.randn(cout, generator=gen))
    return conv.to(DEV).eval()


def _x(c, hw, seed):
    return _cl(torch.randn(1, c, hw, hw, generator=torch.Generator().manual_seed(seed)))


def _run(conv, x, **kw):
    from sige_amd.nn.dense import fused_conv2d

    with torch.no_grad():
        return fused_conv2d(conv, x, **kw)


def _side_call(hip, conv, x):
    """The side conv's call: every tile, into a (poisoned) buffer of the caller's."""
    out = torch.empty((1, conv.out_channels, x.shape[2], x.shape[3]), device=DEV, memory_format=CL)
    tiles = hip.all_tiles(x.shape[2], x.shape[3], (4, 4), (1, 1), (1, 1), x.device)
    _run(conv, x, tiles=tiles, out=out)
    return out


def _side_alone(hip, conv, x, nb):
    """The side conv in a launch of its own with 16 x (16 * nb) blocks -- the plan it is queued with (the two block shapes add
    the K steps up in different orders: 16 x 16 blocks alternate between two accumulators)."""
    with hip.tuning_build():
        hip.conv_force_tile(16, nb)
        try:
            return _side_call(hip, conv, x).clone()
        finally:
            hip.conv_force_tile(0, 0)


SIDE_NB = 2  # the library's choice for the side conv of these tests (K = 288: 16 x 32 blocks)


def _queue(hip, conv, x, budget, force_nb=None, packs=0):
    """side_begin + the call: nothing is launched (`packs`: but the kernels that pack a conv's weights at its first use).
    `force_nb` (measurement build): the side conv's plan, 16 x (16 * nb) blocks."""
    if force_nb:
        hip.conv_force_tile(16, force_nb)
    try:
        hip.conv_side_begin(budget)
        n0 = hip.launch_count()
        out = _side_call(hip, conv, x)
        assert hip.launch_count() == n0 + packs, "the armed call launched"
    finally:
        if force_nb:
            hip.conv_force_tile(0, 0)
    return out


def _hosted(hip, fn):
    """(result of fn(), side workgroups it hosted, side workgroups flushed meanwhile, launches counted)"""
    h0, f0 = hip.conv_side_workgroups()
    n0 = hip.launch_count()
    out = fn()
    h1, f1 = hip.conv_side_workgroups()
    return out, h1 - h0, f1 - f0, hip.launch_count() - n0


@pytest.fixture(scope="module")
def case(hip):
    """(host conv, three host inputs, side conv, side input) and the results of each launched alone (computed once)."""
    host, side = _conv(64, 32), _conv(32, 64, bias=False)
    xh = [_x(64, 8, s) for s in (1, 2, 3, 4)]
    xs = _x(32, 16, 9)
    with util.poisoned(NAN):
        want_h = [_run(host, x).clone() for x in xh]
        want_s = {nb: _side_alone(hip, side, xs, nb) for nb in (1, 2)}
    torch.cuda.synchronize()
    util.assert_finite(want_s[1], "side conv alone")
    assert float((want_s[1] - want_s[2]).abs().max()) <= 1e-5  # (rounding apart)
    return host, xh, side, xs, want_h, want_s


@pytest.mark.parametrize("nb,slices", [(1, [24, 24, 16]), (2, [24, 8, 0])])
def test_three_hosts_take_the_side_conv(hip, case, nb, slices):
    """(a) budget 24: the hosts take 24 + 24 + 16 of the 64 blocks (16 x 32 blocks: 24 + 8 of the 32, the third host runs alone)."""
    host, xh, side, xs, want_h, want_s = case
    with hip.tuning_build(), util.poisoned(NAN):
        out = _queue(hip, side, xs, 24, force_nb=nb)
        for i, take in enumerate(slices):
            got, hosted, flushed, launches = _hosted(hip, lambda: _run(host, xh[i]))
            assert (hosted, flushed, launches) == (take, 0, 1), (i, hosted, flushed, launches)
            assert torch.equal(got, want_h[i]), i
        _, hosted, flushed, launches = _hosted(hip, lambda: hip.conv_side_flush(xs))
        assert (hosted, flushed, launches) == (0, 0, 0)
        torch.cuda.synchronize()
        assert torch.equal(out, want_s[nb])


@pytest.mark.parametrize("nb,hosts,rest", [(1, 2, 16), (2, 1, 8)])
def test_flush_runs_the_remainder(hip, case, nb, hosts, rest):
    """(b) budget 24, two hosts, then flush: the last 16 blocks run as ONE launch of their own (16 x 32 blocks: one host, 8 left)."""
    host, xh, side, xs, want_h, want_s = case
    with hip.tuning_build(), util.poisoned(NAN):
        out = _queue(hip, side, xs, 24, force_nb=nb)
        for i in range(hosts):
            got, hosted, _, _ = _hosted(hip, lambda: _run(host, xh[i]))
            assert hosted == 24 and torch.equal(got, want_h[i])
        _, hosted, flushed, launches = _hosted(hip, lambda: hip.conv_side_flush(xs))
        assert (hosted, flushed, launches) == (0, rest, 1)
        torch.cuda.synchronize()
        assert torch.equal(out, want_s[nb])


def test_flush_without_a_host(hip, case):
    """(c) no host at all: the flush is the conv's own launch."""
    _, _, side, xs, _, want_s = case
    with util.poisoned(NAN):
        out = _queue(hip, side, xs, 24)
        _, hosted, flushed, launches = _hosted(hip, lambda: hip.conv_side_flush(xs))
        assert (hosted, flushed, launches) == (0, 64 // SIDE_NB, 1)
        torch.cuda.synchronize()
        assert torch.equal(out, want_s[SIDE_NB])
        # a side_begin whose conv never comes is disarmed by the flush: the next call launches
        hip.conv_side_begin(24)
        hip.conv_side_flush(xs)
        got, _, _, launches = _hosted(hip, lambda: _side_call(hip, side, xs))
        assert launches == 1 and torch.equal(got, want_s[1])  # (its own plan: 16 x 16 blocks)
        # a call that is not eligible (affine + SiLU staging) launches as ever and spends the side_begin: the next one launches too
        host, xh = case[0], case[1]
        sc, sh = torch.rand(1, 64, 1, 1, device=DEV) + 0.5, torch.randn(1, 64, 1, 1, device=DEV)
        want_a = _run(host, xh[0], scale=sc, shift=sh, activation_name="swish").clone()
        hip.conv_side_begin(24)
        got_a, hosted, flushed, launches = _hosted(hip, lambda: _run(host, xh[0], scale=sc, shift=sh, activation_name="swish"))
        assert (hosted, flushed, launches) == (0, 0, 1) and torch.equal(got_a, want_a)
        got, _, _, launches = _hosted(hip, lambda: _side_call(hip, side, xs))
        assert launches == 1 and torch.equal(got, want_s[1])
        assert _hosted(hip, lambda: hip.conv_side_flush(xs))[1:] == (0, 0, 0)


def test_two_side_convs_are_served_in_order(hip, case):
    """(d) the second queued conv gets its first block only when the first has none left; a host serves one conv."""
    host, xh, side, xs, want_h, want_s = case
    side2, xs2 = _conv(32, 64, seed=5), _x(32, 16, 11)
    with util.poisoned(NAN):
        want_2 = _side_alone(hip, side2, xs2, SIDE_NB)
        out1 = _queue(hip, side, xs, 24)
        out2 = _queue(hip, side2, xs2, 24)
        total = sum(hip.conv_side_workgroups())
        taken = []
        for i in range(4):
            got, hosted, flushed, _ = _hosted(hip, lambda: _run(host, xh[i]))
            assert flushed == 0 and torch.equal(got, want_h[i])
            taken.append(hosted)
        assert taken == [24, 8, 24, 8], taken  # (32 blocks each)
        hip.conv_side_flush(xs)
        assert sum(hip.conv_side_workgroups()) - total == 64
        torch.cuda.synchronize()
        assert torch.equal(out1, want_s[SIDE_NB]) and torch.equal(out2, want_2)


def test_launches_that_are_no_hosts(hip, case):
    """(e) a K-split launch and a launch that carries a held 1x1 shortcut leave the queue alone; a launch on another stream flushes
    it first.  All exact."""
    host, xh, side, xs, want_h, want_s = case
    deep, xd = _conv(256, 32), _x(256, 8, 21)          # 8 blocks over 4 chunks: K-split over gridDim.y = 2
    short, conv1 = _conv(64, 32, k=1, seed=3), _conv(64, 32, seed=4)
    sc = torch.rand(1, 64, 1, 1, device=DEV) + 0.5
    sh = torch.randn(1, 64, 1, 1, device=DEV)
    with util.poisoned(NAN):
        want_d = _run(deep, xd).clone()
        want_short, want_c1 = _run(short, xh[0]).clone(), _run(conv1, xh[0], scale=sc, shift=sh, activation_name="swish").clone()
        out = _queue(hip, side, xs, 24)
        got_d, hosted, flushed, _ = _hosted(hip, lambda: _run(deep, xd))
        assert (hosted, flushed) == (0, 0)
        pairs = hip.conv_pairs_fused()

        def block():
            with hip.conv_pair(xh[0]):
                a = _run(short, xh[0])
                return a, _run(conv1, xh[0], scale=sc, shift=sh, activation_name="swish")

        (got_short, got_c1), hosted, flushed, _ = _hosted(hip, block)
        assert (hosted, flushed) == (0, 0) and hip.conv_pairs_fused() == pairs + 1
        other = torch.cuda.Stream()
        other.wait_stream(torch.cuda.current_stream())

        def elsewhere():
            with torch.cuda.stream(other):
                return _run(host, xh[1])

        got_h, hosted, flushed, launches = _hosted(hip, elsewhere)
        assert (hosted, flushed, launches) == (0, 64 // SIDE_NB, 2)
        torch.cuda.current_stream().wait_stream(other)
        torch.cuda.synchronize()
        assert torch.equal(got_d, want_d) and torch.equal(got_short, want_short) and torch.equal(got_c1, want_c1)
        assert torch.equal(got_h, want_h[1]) and torch.equal(out, want_s[SIDE_NB])
        assert _hosted(hip, lambda: hip.conv_side_flush(xs))[1:] == (0, 0, 0)


def test_graph_replays_equal_eager(hip, case):
    """(f) the queued conv, three hosts and the flush captured once; three replays over the same buffers, alternating two inputs."""
    host, xh, side, xs, _, _ = case
    ins = {"A": ([x.clone() for x in xh[:3]], xs.clone()), "B": ([_x(64, 8, 30 + i) for i in range(3)], _x(32, 16, 40))}
    with util.poisoned(NAN):
        want = {k: ([_run(host, x).clone() for x in h], _side_alone(hip, side, s, SIDE_NB)) for k, (h, s) in ins.items()}
        bh, bs = [x.clone() for x in xh[:3]], xs.clone()

        def run():
            out = _queue(hip, side, bs, 24)
            outs = [_run(host, b) for b in bh]
            hip.conv_side_flush(bs)
            return outs, out

        g, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            run()
            torch.cuda.synchronize()
            h0 = hip.conv_side_workgroups()[0]
            with torch.cuda.graph(g, stream=st):
                outs, out = run()
            assert hip.conv_side_workgroups()[0] > h0
        torch.cuda.current_stream().wait_stream(st)
        for k in ("A", "B", "A"):
            for b, x in zip(bh, ins[k][0]):
                b.copy_(x)
            bs.copy_(ins[k][1])
            g.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(o, w) for o, w in zip(outs, want[k][0])), k
            assert torch.equal(out, want[k][1]), k
        del g


@pytest.mark.parametrize("ch_h,ch_s", [(32, 32), (32, 16)])
def test_partitioned_conv_vs_fp64(hip, case, ch_h, ch_s):
    """(g) conv1(cat(a, b)) as conv_h(a) + residual P, P = conv_s(b) computed as a side conv behind two hosts, against an fp64 conv
    of the cat on the CPU: the conv parity bound 2e-5 (1 + max |ref|)."""
    from sige_amd.workloads.ddpm_unet import DDPMConfig, ResBlock

    host, xh, _, _, want_h, _ = case
    torch.manual_seed(7)
    block = ResBlock(DDPMConfig(groups=8), ch_h + ch_s, 64, sparse=False).eval()
    a, b = torch.randn(1, ch_h, 16, 16), torch.randn(1, ch_s, 16, 16)
    with torch.no_grad():
        ref = torch.nn.functional.conv2d(torch.cat([a, b], 1).double(), block.conv1.weight.double(), block.conv1.bias.double(), 1, 1)
    block = block.to(DEV)
    conv_h, conv_s = block.split_conv1(ch_h)
    with util.poisoned(NAN):
        P = _queue(hip, conv_s, _cl(b), 24, packs=2)
        for i in range(2):
            assert torch.equal(_run(host, xh[i]), want_h[i])
        hip.conv_side_flush(P)
        got = _run(conv_h, _cl(a), residual=P)
    err, tol = float((got.double().cpu() - ref).abs().max()), 2e-5 * (1 + float(ref.abs().max()))
    print("side_convs partitioned %d+%d: %.3e (tol %.3e)" % (ch_h, ch_s, err, tol), flush=True)
    assert err <= tol, (err, tol)
