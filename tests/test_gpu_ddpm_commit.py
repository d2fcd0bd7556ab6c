"""An accepted edit on the fused path: DDPMSparseUNet(ch=32) in the benchmarked configuration (channels-last, persistent in-place
scatter outputs, twins warmed) runs full(x0), a `sparse_update` forward on x1 under the mask m1, a plain sparse forward on x2
under m1 and one on x3 under m2 (m2 overlaps m1 and extends past it), and is compared with the same network on the CPU with the
oracle as native backend -- the reference's module-by-module refresh -- after every step.  The sequence runs ONCE per process
(`run`); the tests look at what it recorded."""
import os

import pytest
import torch

from tests import commit_common as K
from tests import util

pytestmark = [pytest.mark.gpu, pytest.mark.oracle_parity]
DEV = torch.device("cuda")
CL = torch.channels_last
TEST = "test_gpu_ddpm_commit"


def _cl(a):
    return a.to(DEV).contiguous(memory_format=CL)


def _inputs():
    import bench

    x0, noise = bench.make_inputs()
    g = torch.Generator().manual_seed(7)
    n2, n3 = torch.randn(x0.shape, generator=g), torch.randn(x0.shape, generator=g)
    m1 = torch.zeros(256, 256, dtype=torch.bool)
    m1[96:128, 96:128] = True
    m2 = torch.zeros(256, 256, dtype=torch.bool)
    m2[112:160, 112:160] = True
    x1 = x0 + noise * m1
    return dict(x0=x0, x1=x1, x2=x1 + n2 * m1, x3=x1 + n3 * m2, m1=m1, m2=m2, t=torch.zeros(1))


def _pyramid(m):
    from sige_amd.utils import dilate_mask, downsample_mask

    return downsample_mask(dilate_mask(m, 5), 8)


def _caches(model, clone=False):
    out = {}
    for name, mod in model.named_modules():
        for attr in ("original_outputs", "original_residuals", "activated_outputs"):
            for cid, t in getattr(mod, attr, {}).items():
                out[(name, attr, cid)] = t.detach().clone() if clone else t
    return out


def _buffers(model):
    """Every persistent output and twin buffer by name: (object id, address), and every generation counter."""
    out = {}
    for name, mod in model.named_modules():
        ob = getattr(mod, "_out_bufs", None)
        if ob is None:
            continue
        for cid, (_, buf, _) in ob.bufs.items():
            out[(name, "out", cid)] = (id(buf), buf.data_ptr())
        out[(name, "gen")] = dict(ob.gen)
        for key, tb in mod.twins.bufs.items():
            for cid, (_, buf, _) in tb.bufs.items():
                out[(name, "twin", key, cid)] = (id(buf), buf.data_ptr())
            out[(name, "twin gen", key)] = dict(tb.gen)
    return out


def _new_model():
    from sige_amd.workloads.ddpm_unet import DDPMConfig, DDPMSparseUNet

    torch.manual_seed(0)
    return DDPMSparseUNet(DDPMConfig(ch=32)).eval()


def _oracle(d):
    """The reference semantics: outputs of the four steps and the caches right after the sparse_update forward."""
    from oracle import oracle
    from sige_amd import runtime

    model = _new_model()
    n_thr = min(32, os.cpu_count() or 1)
    torch.set_num_threads(n_thr)
    oracle.set_num_threads(n_thr)
    backend, _ = util.cpu_backend()
    runtime.register_backend("cpu", backend)
    try:
        with torch.no_grad():
            model.set_mode("full")
            full = model(d["x0"], d["t"]).clone()
            model.set_masks(_pyramid(d["m1"]))
            model.set_mode("sparse")
            model.set_sparse_update(True)
            out1 = model(d["x1"], d["t"]).clone()
            model.set_sparse_update(False)
            caches = _caches(model, clone=True)
            out2 = model(d["x2"], d["t"]).clone()
            model.set_masks(_pyramid(d["m2"]))
            out3 = model(d["x3"], d["t"]).clone()
    finally:
        runtime.unregister_backend("cpu")
    return dict(full=full, out1=out1, out2=out2, out3=out3, caches=caches)


def _gpu_sequence(hip, d, opt_in=True, cache_dtype="f32", change=True):
    model = _new_model().to(DEV).to(memory_format=CL)
    if not opt_in:
        model.COMMIT_TILES = False
    model.DENSE_ON_CHANGE = change
    model.set_scatter_inplace(True)
    model.set_cache_dtype(cache_dtype)
    t = d["t"].to(DEV)
    r = dict(model=model)
    builds = []
    inner = model._change_build
    model._change_build = lambda *a, **k: (builds.append(a[0]), inner(*a, **k))[1]  # (counts the every-cell builds per level)
    with torch.no_grad(), util.native_full_pass():
        model.set_mode("full")
        r["full"] = model(_cl(d["x0"]), t).clone()
        model.set_masks(_pyramid(d["m1"].to(DEV)))
        model.set_mode("sparse")
        for _ in range(2):  # (the activated twins of the conv1 inputs exist from the second forward on)
            model(_cl(d["x1"]), t)
        n0 = hip.launch_count()
        model(_cl(d["x1"]), t)
        r["plain_launches"] = hip.launch_count() - n0
        r["before"] = _buffers(model)
        r["cache_ids"] = {k: (id(v), v.data_ptr()) for k, v in _caches(model).items()}
        r["state0"] = dict(model.__dict__.get("_change_state", {}))
        r["builds0"] = list(builds)
        model.set_sparse_update(True)
        n0 = hip.launch_count()
        r["out1"] = model(_cl(d["x1"]), t).clone()
        r["commit_forward_launches"] = hip.launch_count() - n0
        q = model.__dict__.get("_commit_queue")
        r["commit_launches"], r["records"] = (q.launches, q.flushed) if q is not None else (0, 0)
        model.set_sparse_update(False)
        r["after"] = _buffers(model)
        r["cache_ids_after"] = {k: (id(v), v.data_ptr()) for k, v in _caches(model).items()}
        r["caches"] = _caches(model, clone=True)
        r["outs"] = {name: mod._out_bufs.bufs[0][1].clone() for name, mod in model.named_modules()
                     if hasattr(mod, "_out_bufs") and 0 in mod._out_bufs.bufs}
        r["affines"] = {name: mod.affine[0] for name, mod in model.named_modules() if hasattr(mod, "scatter_gather") and 0 in mod.affine}
        r["state1"] = dict(model.__dict__.get("_change_state", {}))
        r["out2"] = model(_cl(d["x2"]), t).clone()
        r["state2"] = dict(model.__dict__.get("_change_state", {}))
        r["builds2"] = list(builds)
        model.set_masks(_pyramid(d["m2"].to(DEV)))
        r["out3"] = model(_cl(d["x3"]), t).clone()
        r["state3"] = dict(model.__dict__.get("_change_state", {}))
        r["builds3"] = list(builds)
        torch.cuda.synchronize()
    return r


_RUN = {}


@pytest.fixture(scope="module")
def run():
    from sige_amd import hip

    hip.lib()
    if not _RUN:
        d = _inputs()
        _RUN.update(d=d, hip=hip, oracle=_oracle(d), new=_gpu_sequence(hip, d))
    return _RUN


def _worst(a, b):
    return float((a.float().cpu() - b.float().cpu()).abs().max())


def test_every_output_is_the_oracles(run):
    o, n = run["oracle"], run["new"]
    for key in ("full", "out1", "out2", "out3"):
        m = util.record_margin(TEST, key, _worst(n[key], o[key]), util.CONV_ATOL)
        print("%s: %.3g (bound %.3g)" % (key, m, util.CONV_ATOL))
        assert m <= util.CONV_ATOL, (key, m)
    # the steps are different images: an out2 computed on the ORIGINAL's caches would be x2's edit without x1's -- far off
    assert _worst(o["out1"], o["full"]) > 1e-2 and _worst(o["out2"], o["out1"]) > 1e-2 and _worst(o["out3"], o["out1"]) > 1e-2


def test_the_committed_caches_are_the_oracles(run):
    o, n = run["oracle"]["caches"], run["new"]["caches"]
    raw = {k: v for k, v in n.items() if k[1] != "activated_outputs"}
    assert sorted(raw) == sorted(k for k in o if k[1] != "activated_outputs") and len(raw) >= 20
    worst = max(_worst(raw[k], o[k]) for k in raw)
    util.record_margin(TEST, "caches after the commit", worst, util.CONV_ATOL)
    print("caches: %d tensors, worst %.3g (bound %.3g)" % (len(raw), worst, util.CONV_ATOL))
    for k in raw:
        assert _worst(raw[k], o[k]) <= util.CONV_ATOL, k
    # ... and they moved: the sparse_update forward did change them (the full pass's caches are x0's)
    assert run["new"]["records"] >= len(raw)


def test_every_scatter_cache_is_its_persistent_output(run):
    n = run["new"]
    assert n["outs"]
    for name, out in n["outs"].items():
        assert torch.equal(n["caches"][(name, "original_outputs", 0)], out), name


def test_the_activated_copy_follows_the_committed_raw_cache(run):
    n = run["new"]
    acts = [k for k in n["caches"] if k[1] == "activated_outputs"]
    assert acts
    worst = 0.0
    for name, attr, cid in acts:
        s2, t2 = n["affines"][name.rsplit(".", 1)[0]][2:]
        want = K.affine_swish(n["caches"][(name, "original_outputs", cid)].cpu(), s2.cpu(), t2.cpu())
        got = n["caches"][(name, attr, cid)].cpu()
        worst = max(worst, float(((got - want).abs() / (want.abs() + util.SWISH_ATOL / util.SWISH_RTOL)).max()))
    util.record_margin(TEST, "activated copies", worst, util.SWISH_RTOL)
    print("activated copies: %d tensors, worst %.3g (bound %.3g)" % (len(acts), worst, util.SWISH_RTOL))
    assert worst <= util.SWISH_RTOL


def test_launch_count_and_nothing_reallocated(run):
    n = run["new"]
    print("plain %d launches, sparse_update forward %d, of which commit %d (%d records)" % (
        n["plain_launches"], n["commit_forward_launches"], n["commit_launches"], n["records"]))
    assert n["commit_launches"] >= 1 and n["records"] > 0
    assert n["commit_forward_launches"] == n["plain_launches"] + n["commit_launches"]
    # every cache tensor, persistent output and twin buffer: the same object at the same address, no generation bumped
    assert n["before"] and any(k[1] == "twin" for k in n["before"])
    assert n["after"] == n["before"]
    assert n["cache_ids_after"] == n["cache_ids"]


def test_the_change_region_level_keeps_its_buffers(run):
    """Derived expectation: the level's buffers hold the original's values outside the region and the accepted
    edit's inside -- after the commit that IS the new base, and nothing in `_change_signature` moved (no generation, no affine, no
    mask), so neither the sparse_update forward nor the plain forward behind it rebuilds; the new mask m2 moves the signature's
    timestamp: exactly one every-cell build per level, from the producer output that set_masks restored from the committed cache."""
    n = run["new"]
    assert n["state0"], "no change-region level in this network: the test has nothing to say"
    assert n["state1"] == n["state0"] and n["state2"] == n["state0"]
    assert n["builds2"] == n["builds0"]
    levels = sorted(k[0] for k in n["state0"])
    assert sorted(n["builds3"][len(n["builds0"]):]) == levels
    for key, (sig, _) in n["state3"].items():
        sig0 = n["state0"][key][0]
        assert sig[0] == sig0[0] + 1 and sig[1:] == sig0[1:], key  # the mask's timestamp, and nothing else


def test_the_reference_route_gives_the_same_caches(run):
    """Opt-in off: the forward leaves the fused path and every module copies its whole tensor, as before."""
    old = _gpu_sequence(run["hip"], run["d"], opt_in=False)
    n = run["new"]
    assert old["commit_launches"] == 0 and old["records"] == 0
    assert sorted(old["caches"]) == sorted(n["caches"])
    worst = max(_worst(old["caches"][k], n["caches"][k]) for k in n["caches"])
    util.record_margin(TEST, "caches, reference route", worst, util.CONV_ATOL)
    print("reference route: caches worst %.3g, forward %d launches against %d" % (
        worst, old["commit_forward_launches"], n["commit_forward_launches"]))
    assert worst <= util.CONV_ATOL
    for key in ("out1", "out2", "out3"):
        assert _worst(old[key], run["oracle"][key]) <= util.CONV_ATOL, key
    assert old["after"] != old["before"]  # (that route drops the persistent outputs)


def test_a_commit_under_cache_id_1_leaves_cache_id_0_alone(run):
    d, hip = run["d"], run["hip"]
    model = _new_model().to(DEV).to(memory_format=CL)
    model.set_scatter_inplace(True)
    t = d["t"].to(DEV)
    with torch.no_grad(), util.native_full_pass():
        model.set_mode("full")
        model.set_cache_id(0)
        model(_cl(d["x0"]), t)
        model.set_cache_id(1)
        model(_cl(d["x0"].flip(-1)), t)
        model.set_masks(_pyramid(d["m1"].to(DEV)))
        model.set_mode("sparse")
        model(_cl(d["x0"].flip(-1) + (d["x1"] - d["x0"])), t)
        keep = {k: v for k, v in _caches(model, clone=True).items()}
        model.set_sparse_update(True)
        model(_cl(d["x0"].flip(-1) + (d["x1"] - d["x0"])), t)
        model.set_sparse_update(False)
        torch.cuda.synchronize()
    now = _caches(model)
    assert sorted(now) == sorted(keep)
    for k in now:
        if k[2] == 0:
            assert torch.equal(now[k], keep[k]), k
    assert any(k[2] == 1 and k[1] == "original_outputs" and not torch.equal(now[k], keep[k]) for k in now)


def test_stacked_edits_raise(run):
    from sige_amd import stacked

    model, d = run["new"]["model"], run["d"]
    with stacked.edit_batch(model, 2):
        with pytest.raises(RuntimeError, match="stacked"):
            model.set_sparse_update(True)
    model.set_sparse_update(True)
    try:
        with stacked.edit_batch(model, 2), torch.no_grad():
            with pytest.raises(RuntimeError, match="stacked"):
                model(_cl(torch.cat([d["x1"], d["x2"]])), d["t"].to(DEV))
    finally:
        model.set_sparse_update(False)


def test_fp16_stored_caches(run):
    """set_cache_dtype("f16"): the commit rounds to fp16 where the reference route's `cached.copy_(output)` does.  Bounds: the two
    routes' fp32 values lie within CONV_ATOL of each other and each is rounded to fp16 once -- one more fp16 ulp, 2^-10 relative;
    the activated copy is SiLU(s2 * v + t2) of the fp32 tile value v rounded once, against the formula on the STORED cache
    half(v): the input moved by 2^-11 |v|, SiLU's slope is at most 1.1, plus the two roundings of the results (2^-10 |want|)."""
    new = _gpu_sequence(run["hip"], run["d"], cache_dtype="f16")
    old = _gpu_sequence(run["hip"], run["d"], opt_in=False, cache_dtype="f16")
    assert all(v.dtype == torch.float16 for v in new["caches"].values())
    assert new["commit_forward_launches"] == new["plain_launches"] + new["commit_launches"] and new["after"] == new["before"]
    for name, out in new["outs"].items():
        assert torch.equal(new["caches"][(name, "original_outputs", 0)], out.half()), name
    worst = 0.0
    for k, v in new["caches"].items():
        a, b = v.float().cpu(), old["caches"][k].float().cpu()
        if k[1] == "activated_outputs":
            s2, t2 = (x.cpu() for x in new["affines"][k[0].rsplit(".", 1)[0]][2:])
            raw = new["caches"][(k[0], "original_outputs", k[2])].float().cpu()
            want = K.affine_swish(raw, s2, t2)
            bound = 2.0 ** -10 * want.abs() + 1.1 * 2.0 ** -11 * (s2.abs() * raw.abs()) + 1e-6
            assert bool(((a - want).abs() <= bound).all()), k
        else:
            m = float(((a - b).abs() / (util.CONV_ATOL + 2.0 ** -10 * b.abs())).max())
            worst = max(worst, m)
            assert m <= 1.0, (k, m)
    util.record_margin(TEST, "caches, fp16 storage, against the reference route (in units of the bound)", worst, 1.0)
    print("fp16 caches: worst %.3g of the bound against the reference route" % worst)
