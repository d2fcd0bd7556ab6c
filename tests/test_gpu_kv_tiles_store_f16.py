"""hip.kv_tiles_store_f16 = sige_hip_kv_tiles_store_f16 (csrc/kv_rows_f16.hip) on the GPU, and the SD VAE decoder under
sd_vae.ATTENTION_COMPUTE = "f16kv", whose fp16 twin of the persistent K | V that launch keeps current.

The launch: the 4x4 tiles of the index list of a channels-last fp32 image, rounded into the same cells of an fp16 image -- bit for bit
what torch indexing plus .half() gives, every other cell left as it was (a sentinel pattern).  The decoder: after every sparse
forward the output meets the f16 criterion against the all-fp32 model and the twin equals persistent_kv.half() over the WHOLE tensor --
a twin that missed a restore or a tile is stale somewhere."""
import pytest
import torch

from sige_amd.tolerance import f16_check
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
H, W = 18, 26  # ragged: the tiles at row 16 and column 24 hang off the image
TILES = [(0, 0), (4, 8), (16, 4), (8, 24), (16, 24)]


@pytest.mark.parametrize("C", [8, 1024])
def test_tiles_land_rounded_and_nothing_else_moves(C):
    from sige_amd import hip

    g = torch.Generator().manual_seed(H * W + C)
    # values that need rounding in every binade fp16 has between 2^-16 (subnormal) and 2^8
    src = (torch.randn(1, C, H, W, generator=g) * 2.0 ** torch.randint(-16, 8, (1, C, H, W), generator=g).float()).to(DEV).contiguous(memory_format=CL)
    sentinel = (torch.arange(C * H * W, dtype=torch.float32) % 2039.0 - 1000.0).reshape(1, C, H, W).half().to(DEV).contiguous(memory_format=CL)
    got, want = sentinel.clone(memory_format=CL), sentinel.clone(memory_format=CL)
    for y0, x0 in TILES:
        want[:, :, y0:y0 + 4, x0:x0 + 4] = src[:, :, y0:y0 + 4, x0:x0 + 4].half()
    idx = torch.tensor(TILES, dtype=torch.int32, device=DEV)
    n0 = hip.launch_count()
    hip.kv_tiles_store_f16(src, got, idx)
    assert hip.launch_count() == n0 + 1
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    hip.kv_tiles_store_f16(src, got, idx[:0])  # T = 0: nothing launched
    assert hip.launch_count() == n0 + 1


def test_decoder_with_the_switch_on_keeps_its_twin_current():
    """full pass -> sparse under mask A -> mask B -> mask A again, then one stacked forward at E = 2.  (A forward that fell back to the
    "f16" launch would leave its tiles out of the twin: the twin check fails then, too.)"""
    from sige_amd import stacked
    from sige_amd.workloads import sd_vae
    from tests import test_gpu_sd_vae_stacked as S

    E, keep, models = 2, sd_vae.ATTENTION_COMPUTE, {}
    sd_vae.ATTENTION_COMPUTE = "f16kv"
    try:
        models = {dtype: S.build("decoder", DEV, True, True)[0] for dtype in ("f32", "f16")}
        models["f16"].set_compute_dtype("f16")
        model, attn = models["f16"], models["f16"].mid.attn_1
        assert attn.ch > 160 and attn.attention_compute() == "f16kv"
        pyrs = S.pyramids("decoder", DEV)[:E]
        x0, edits, _ = S.edit_inputs("decoder", pyrs, DEV)
        x0, edits = S._fmt(x0, True), [S._fmt(x, True) for x in edits[:E]]

        def both(x):
            sd_vae.ATTENTION_COMPUTE = "f32"  # (the all-fp32 model's attention is the exact one)
            want = models["f32"](x).clone()
            sd_vae.ATTENTION_COMPUTE = "f16kv"
            with util.poisoned():
                got = model(x).clone()
            util.assert_finite(got, "decoder output, attention f16kv")
            chk = f16_check(got, want)
            util.record_margin("test_gpu_kv_tiles_store_f16 decoder", "worst / allowed", chk["worst_over_allowed"], 1.0)
            assert chk["ok"], chk
            bufs = dict((name, buf) for name, buf, _ in attn.persistent_buffers())
            assert "kv16" in bufs and torch.equal(bufs["kv16"], bufs["kv"].half()), "no twin, or a stale one"

        with torch.no_grad():
            for m in models.values():
                m.set_mode("full")
                m(x0)
                m.set_mode("sparse")
            for e in (0, 1, 0):
                for m in models.values():
                    m.set_masks(pyrs[e])
                both(edits[e])
            for m in models.values():
                stacked.stack_caches(m, E)
                stacked.set_masks(m, pyrs)
            with stacked.edit_batch(models["f32"], E), stacked.edit_batch(model, E):
                both(S._fmt(torch.cat(edits, 0), True))
    finally:
        sd_vae.ATTENTION_COMPUTE = keep
        for m in models.values():
            stacked.unstack_caches(m)
