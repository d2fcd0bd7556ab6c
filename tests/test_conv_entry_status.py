"""What the tile-conv entry points ANSWER, pinned without a launch.

Every case below is answered by the host code before anything is launched: SIGE_HIP_OK through an empty tile list, SIGE_HIP_EINVAL
or SIGE_HIP_EUNSUPPORTED.  The table was recorded on the commit before the host path moved onto the call record
(csrc/conv_call.hpp) and pins the checks AND their order: a case that breaks two rules with different codes says which one is
asked first.  The calls go through the raw ctypes functions with made-up pointers (0x1000; 0x1004 = not 16-byte aligned) that the
host code never dereferences.  A case the code under test wrongly accepted would launch on them, so the module skips itself
where a device is present (without one such a launch fails cleanly with SIGE_HIP_ELAUNCH and shows up as a mismatch).
"""
import pytest
import torch

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
P, Q = 0x1000, 0x1004  # a well-aligned made-up pointer, a misaligned one

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up pointers: never where a wrongly accepted case could launch")

_BLOCK = "x T Cin R S packed bias Cout kH kW strideH strideW out stream"
_TILE3_HEAD = "compute source x x2 y_f16 B C1 C2 H W"
_TILE3_TAIL = ("upsample2x active_indices N scatter_map Rx Sx scale shift affineB activation packed bias Cout to_full offsetH offsetW Ho Wo "
               "residual residual_f16 x1 table1 gH1 gW1 N1 R1 S1 out_scale out_shift out_activation "
               "twin0 twin_scale0 twin_shift0 twin1 twin_scale1 twin_shift1 out stream")
_BC = "%s %sB %sC %sH %sW"

# entry point -> (its parameters in the order of include/sige_hip.h, the baseline: every parameter not named here is 0 / NULL)
ENTRIES = {
    "sige_hip_block_conv_nhwc": (
        "compute " + _BLOCK,
        dict(x=P, T=4, Cin=64, R=6, S=6, packed=P, Cout=64, kH=3, kW=3, strideH=1, strideW=1, out=P)),
    "sige_hip_block_conv_nhwc_keyed": (
        "compute x count_key B N Cin R S packed bias Cout kH kW strideH strideW out stream",
        dict(x=P, count_key=P, B=1, N=4, Cin=64, R=6, S=6, packed=P, Cout=64, kH=3, kW=3, strideH=1, strideW=1, out=P)),
    "sige_hip_gather_conv_nhwc": (
        "compute x x2 B C1 C2 H W bH bW active_indices N scale scaleB scaleC shift shiftB shiftC activation packed bias Cout kH kW "
        "strideH strideW to_full offsetH offsetW residual Ho Wo workspace workspace_floats out_scale out_shift out_activation upsample2x "
        "twin0 twin0_scale twin0_shift twin1 twin1_scale twin1_shift packed_tile3 min_blocks out stream",
        dict(x=P, B=1, C1=64, H=16, W=16, bH=6, bW=6, active_indices=P, N=4, packed=P, Cout=64, kH=3, kW=3, strideH=1, strideW=1, out=P)),
    "sige_hip_scatter_gather_conv_nhwc": (
        "compute x y y_f16 B Cin H W Rx Sx bH bW active_indices N scatter_map scale scaleB scaleC shift shiftB shiftC activation "
        "packed bias Cout kH kW strideH strideW out stream",
        dict(x=P, y=P, B=1, Cin=64, H=16, W=16, Rx=4, Sx=4, bH=6, bW=6, active_indices=P, N=4, scatter_map=P, packed=P, Cout=64,
             kH=3, kW=3, strideH=1, strideW=1, out=P)),
    "sige_hip_scatter_gather_conv_scatter_nhwc": (
        "compute x y y_f16 B Cin H W Rx Sx bH bW active_indices N scatter_map scale scaleB scaleC shift shiftB shiftC activation "
        "packed bias Cout kH kW offsetH offsetW residual residual_f16 x1 table1 gH1 gW1 N1 R1 S1 "
        "twin0 twin0_scale twin0_shift twin1 twin1_scale twin1_shift packed_tile3 min_blocks out stream",
        dict(x=P, y=P, B=1, Cin=64, H=16, W=16, Rx=4, Sx=4, bH=6, bW=6, active_indices=P, N=4, scatter_map=P, packed=P, Cout=64,
             kH=3, kW=3, offsetH=1, offsetW=1, out=P)),
    "sige_hip_tile_conv3_nhwc": (
        _TILE3_HEAD + " " + _TILE3_TAIL,
        dict(source=1, x=P, B=1, C1=64, H=16, W=16, active_indices=P, N=4, packed=P, Cout=64, out=P)),
    "sige_hip_tile_conv3_block_nhwc": (
        _TILE3_HEAD + " bH bW " + _TILE3_TAIL,
        dict(source=1, x=P, B=1, C1=64, H=16, W=16, bH=10, bW=10, active_indices=P, N=4, packed=P, Cout=64, out=P)),
    "sige_hip_wide_conv_nhwc": (
        "x x2 B C1 C2 H W upsample2x scale shift affineB activation packed prec wshift bias Cout kH kW residual out_scale out_shift "
        "out_activation twin0 twin_scale0 twin_shift0 twin1 twin_scale1 twin_shift1 workspace workspace_floats out stats stream",
        dict(x=P, B=1, C1=64, H=16, W=16, packed=P, prec=2, Cout=64, kH=3, kW=3, out=P)),
    "sige_hip_gather_conv_f32": (
        "x B Cin H W bH bW active_indices N " + _BC % (("scale",) * 5) + " " + _BC % (("shift",) * 5) + " activation packed bias Cout "
        "kH kW strideH strideW out stream",
        dict(x=P, B=1, Cin=64, H=16, W=16, bH=6, bW=6, active_indices=P, N=4, packed=P, Cout=64, kH=3, kW=3, strideH=1, strideW=1, out=P)),
    "sige_hip_gather_conv_nchw_f32": (
        "x x2 B C1 C2 H W bH bW active_indices N scale scaleB scaleC shift shiftB shiftC activation packed bias Cout kH kW "
        "strideH strideW offsetH offsetW residual Ho Wo out stream",
        dict(x=P, B=1, C1=64, H=16, W=16, bH=6, bW=6, active_indices=P, N=4, packed=P, Cout=64, kH=3, kW=3, strideH=1, strideW=1,
             Ho=16, Wo=16, out=P)),
    "sige_hip_scatter_gather_conv_f32": (
        "x y B Cin H W Rx Sx bH bW active_indices N scatter_map " + _BC % (("scale",) * 5) + " " + _BC % (("shift",) * 5) +
        " activation packed bias Cout kH kW strideH strideW out stream",
        dict(x=P, y=P, B=1, Cin=64, H=16, W=16, Rx=4, Sx=4, bH=6, bW=6, active_indices=P, N=4, scatter_map=P, packed=P, Cout=64,
             kH=3, kW=3, strideH=1, strideW=1, out=P)),
}

# groups of arguments that several cases share
FULL = dict(to_full=1, Ho=16, Wo=16)                                                 # full-tensor destination
AFF = dict(scale=P, scaleB=1, scaleC=64, shift=P, shiftB=1, shiftC=64)               # staging affine [1, C, 1, 1]
AFF4 = dict(scale=P, scaleB=1, scaleC=64, scaleH=1, scaleW=1, shift=P, shiftB=1, shiftC=64, shiftH=1, shiftW=1)
AFF3 = dict(scale=P, shift=P, affineB=1)                                             # ... of the v3 / wide entry points
BIG = dict(B=8, H=512, W=512)                                                        # with 1024 channels: past the 2^29 offset limit
B10 = dict(bH=10, bW=10, packed_tile3=P)                                             # 10x10 windows with v3 weights
ROUTED = dict(packed_tile3=P, min_blocks=1)                                          # the router sends the call to the v3 kernel
SG3 = dict(source=2, x2=P, scatter_map=P, Rx=4, Sx=4)                                # scatter_gather source of the v3 entry points
BRES = dict(residual=P, x1=P, table1=P, gH1=4, gW1=4, N1=4, R1=4, S1=4)              # block residual
TWIN0 = dict(twin0=P, twin0_scale=P, twin0_shift=P)
EDIT2 = dict(edit_batch=2)                                                           # sige_hip_set_edit_batch(2) around the call


def mix(*groups, **change):
    """One case: the groups above, then single arguments, later ones overriding earlier ones."""
    out = {}
    for g in groups:
        out.update(g)
    out.update(change)
    return out


# (entry point, what the case changes against the baseline, the status recorded on the parent commit)
CASES = [
    # ---- sige_hip_block_conv_nhwc
    ("sige_hip_block_conv_nhwc", mix(T=0), OK),
    ("sige_hip_block_conv_nhwc", mix(T=0, x=None, packed=None, out=None), OK),
    ("sige_hip_block_conv_nhwc", mix(T=-1), EINVAL),
    ("sige_hip_block_conv_nhwc", mix(Cin=0), EINVAL),
    ("sige_hip_block_conv_nhwc", mix(Cout=0), EINVAL),
    ("sige_hip_block_conv_nhwc", mix(compute=3), EINVAL),
    ("sige_hip_block_conv_nhwc", mix(compute=-1), EINVAL),
    ("sige_hip_block_conv_nhwc", mix(compute=3, T=0), EINVAL),
    ("sige_hip_block_conv_nhwc", mix(x=None), EINVAL),
    ("sige_hip_block_conv_nhwc", mix(packed=None), EINVAL),
    ("sige_hip_block_conv_nhwc", mix(out=None), EINVAL),
    ("sige_hip_block_conv_nhwc", mix(Cin=6), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc", mix(Cout=6), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc", mix(x=Q), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc", mix(packed=Q), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc", mix(out=Q), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc", mix(bias=Q), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc", mix(T=2 ** 20, Cin=1024), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc", mix(kH=5, kW=5), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc", mix(kH=3, kW=1), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc", mix(R=7, S=7), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc", mix(strideH=2, strideW=2), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc", mix(compute=1, R=5, S=5, strideH=2, strideW=2), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc", mix(Cin=6, x=None), EINVAL),
    ("sige_hip_block_conv_nhwc", mix(T=-1, x=Q), EINVAL),
    ("sige_hip_block_conv_nhwc", mix(compute=2, Cin=6), EUNSUPPORTED),
    # ---- sige_hip_block_conv_nhwc_keyed
    ("sige_hip_block_conv_nhwc_keyed", mix(N=0), OK),
    ("sige_hip_block_conv_nhwc_keyed", mix(B=0), OK),
    ("sige_hip_block_conv_nhwc_keyed", mix(count_key=None), EINVAL),
    ("sige_hip_block_conv_nhwc_keyed", mix(count_key=None, N=0), EINVAL),
    ("sige_hip_block_conv_nhwc_keyed", mix(B=-1), EINVAL),
    ("sige_hip_block_conv_nhwc_keyed", mix(N=-1), EINVAL),
    ("sige_hip_block_conv_nhwc_keyed", mix(B=65536, N=65536), EINVAL),
    ("sige_hip_block_conv_nhwc_keyed", mix(compute=3), EINVAL),
    ("sige_hip_block_conv_nhwc_keyed", mix(compute=3, N=0), EINVAL),
    ("sige_hip_block_conv_nhwc_keyed", mix(x=None), EINVAL),
    ("sige_hip_block_conv_nhwc_keyed", mix(packed=None), EINVAL),
    ("sige_hip_block_conv_nhwc_keyed", mix(out=None), EINVAL),
    ("sige_hip_block_conv_nhwc_keyed", mix(Cin=0), EINVAL),
    ("sige_hip_block_conv_nhwc_keyed", mix(Cin=0, N=0), EINVAL),
    ("sige_hip_block_conv_nhwc_keyed", mix(Cin=6), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc_keyed", mix(Cout=6), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc_keyed", mix(x=Q), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc_keyed", mix(bias=Q), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc_keyed", mix(kH=5, kW=5), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc_keyed", mix(B=32768, N=32768, Cin=1024), EUNSUPPORTED),
    ("sige_hip_block_conv_nhwc_keyed", mix(Cin=6, out=None), EINVAL),
    ("sige_hip_block_conv_nhwc_keyed", mix(Cin=6, count_key=None), EINVAL),
    # ---- sige_hip_gather_conv_nhwc
    ("sige_hip_gather_conv_nhwc", mix(N=0), OK),
    ("sige_hip_gather_conv_nhwc", mix(B=0), OK),
    ("sige_hip_gather_conv_nhwc", mix(compute=3), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(compute=3, N=0), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(x=None), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(active_indices=None), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(N=-1), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(Cout=0), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(activation=7), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(activation=7, x=None), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(activation=1), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(C1=6), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(C1=6, x=None), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(out=Q), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(packed=Q), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(FULL, residual=Q), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(upsample2x=3), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(upsample2x=1, H=15), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(twin0=P), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(TWIN0), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(FULL, twin0=P), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(FULL, twin1=P, twin1_scale=P), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(FULL, twin0=P, twin0_scale=P, twin0_shift=Q), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(out_scale=P), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(out_activation=7), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(out_scale=P, out_shift=Q), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(scale=P, scaleB=1, scaleC=64), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(AFF, scaleB=3, shiftB=3), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(AFF, shiftC=1), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(to_full=1), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(C2=64), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(C2=64, x2=P, B=2), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(BIG, C1=1024), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(FULL, upsample2x=2, compute=1), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(FULL, upsample2x=2, compute=2), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(upsample2x=2), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(FULL, AFF, upsample2x=2), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(FULL, upsample2x=2, C2=64, x2=P), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(FULL, upsample2x=2, H=15), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(FULL, EDIT2, upsample2x=2), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(EDIT2, H=24), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(EDIT2, B=2), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(bH=10, bW=10), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(B10, compute=1), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(B10, FULL, upsample2x=2), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(B10, AFF, scaleC=32, shiftC=32), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(B10, N=0), OK),
    ("sige_hip_gather_conv_nhwc", mix(B10, x=None), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(B10, C1=32), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(B10, twin0=P), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(B10, packed_tile3=Q), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(B10, out_scale=P), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(B10, EDIT2), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(B10, compute=3), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(kH=5, kW=5), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(ROUTED, x=Q), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(ROUTED, activation=1), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(ROUTED, twin0=P), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(ROUTED, upsample2x=1, H=15), EINVAL),
    ("sige_hip_gather_conv_nhwc", mix(twin0=P, out_activation=7), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(out_scale=P, activation=7), EUNSUPPORTED),
    ("sige_hip_gather_conv_nhwc", mix(to_full=1, activation=7), EINVAL),
    # ---- sige_hip_scatter_gather_conv_nhwc
    ("sige_hip_scatter_gather_conv_nhwc", mix(N=0), OK),
    ("sige_hip_scatter_gather_conv_nhwc", mix(B=0), OK),
    ("sige_hip_scatter_gather_conv_nhwc", mix(compute=3), EINVAL),
    ("sige_hip_scatter_gather_conv_nhwc", mix(compute=3, N=0), EINVAL),
    ("sige_hip_scatter_gather_conv_nhwc", mix(B=-1), EINVAL),
    ("sige_hip_scatter_gather_conv_nhwc", mix(Cin=0), EINVAL),
    ("sige_hip_scatter_gather_conv_nhwc", mix(Rx=0), EINVAL),
    ("sige_hip_scatter_gather_conv_nhwc", mix(activation=7), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(activation=7, x=None), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(activation=7, B=-1), EINVAL),
    ("sige_hip_scatter_gather_conv_nhwc", mix(BIG, Cin=1024), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(N=2 ** 16, Cin=1024), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(x=None), EINVAL),
    ("sige_hip_scatter_gather_conv_nhwc", mix(y=None), EINVAL),
    ("sige_hip_scatter_gather_conv_nhwc", mix(packed=None), EINVAL),
    ("sige_hip_scatter_gather_conv_nhwc", mix(out=None), EINVAL),
    ("sige_hip_scatter_gather_conv_nhwc", mix(active_indices=None), EINVAL),
    ("sige_hip_scatter_gather_conv_nhwc", mix(scatter_map=None), EINVAL),
    ("sige_hip_scatter_gather_conv_nhwc", mix(Cin=6), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(Cin=6, y=None), EINVAL),
    ("sige_hip_scatter_gather_conv_nhwc", mix(x=Q), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(y=Q), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(out=Q), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(bias=Q), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(packed=Q), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(y_f16=1, kH=1, kW=1), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(y_f16=1, strideH=2, strideW=2), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(EDIT2, H=24), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(EDIT2, B=2), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(scale=P, scaleB=1, scaleC=64), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(AFF, scaleB=3, shiftB=3), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(activation=1), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(kH=5, kW=5), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_nhwc", mix(bH=10, bW=10), EUNSUPPORTED),
    # ---- sige_hip_scatter_gather_conv_scatter_nhwc
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(N=0), OK),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(compute=3), EINVAL),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(compute=3, N=0), EINVAL),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(Sx=0), EINVAL),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(kH=1, kW=1), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(kH=1, kW=1, N=0), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(bH=4, bW=4), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(bH=10, bW=10), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(activation=7), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(BIG, Cin=1024), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(x=None), EINVAL),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(scatter_map=None), EINVAL),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(x1=P), EINVAL),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(BRES, table1=None), EINVAL),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(BRES, gH1=3), EINVAL),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(BRES, R1=0), EINVAL),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(BRES, x1=Q), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(residual=Q), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(residual_f16=1), EINVAL),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(residual_f16=1, Cin=6), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(x1=P, Cin=6), EINVAL),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(Cin=6), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(EDIT2, H=24), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(scale=P, scaleB=1, scaleC=64), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(twin0=P), EINVAL),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(twin0=P, twin0_scale=P, twin0_shift=Q), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(twin0=P, scale=P, scaleB=1, scaleC=64), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(B10), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(B10, Rx=8, Sx=8, y_f16=1), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(B10, Rx=8, Sx=8, N=0), OK),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(B10, Rx=8, Sx=8, x=None), EINVAL),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(B10, AFF, Rx=8, Sx=8), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(B10, Rx=8, Sx=8, compute=1), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(B10, Rx=8, Sx=8, compute=3), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(B10, Rx=8, Sx=8, scatter_map=None), EINVAL),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(B10, Rx=8, Sx=8, Cin=32), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(B10, Rx=8, Sx=8, x1=P), EINVAL),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(B10, EDIT2, Rx=8, Sx=8), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(ROUTED, x=Q), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(ROUTED, twin0=P), EINVAL),
    ("sige_hip_scatter_gather_conv_scatter_nhwc", mix(ROUTED, activation=1), EUNSUPPORTED),
    # ---- sige_hip_tile_conv3_nhwc
    ("sige_hip_tile_conv3_nhwc", mix(N=0), OK),
    ("sige_hip_tile_conv3_nhwc", mix(compute=3), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(compute=-1), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(compute=2), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(compute=2, N=0), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(compute=2, source=0), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(source=0), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(source=3), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(y_f16=1), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(y_f16=1, residual_f16=1), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(SG3, y_f16=1), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(residual_f16=1), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(B=-1), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(C1=0), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(x=None), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(C2=64), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(SG3, x2=None), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(SG3, scatter_map=None), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(SG3, Rx=0), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(SG3, C2=64), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(SG3, upsample2x=1), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(C1=32), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(C1=32, x=None), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(Cout=32), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(scale=P), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(scale=P, x=Q), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(AFF3, affineB=3), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(activation=1), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(AFF3, activation=7), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(out_scale=P), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(out_scale=P, out_shift=P, out_activation=7), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(upsample2x=1, H=15), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(to_full=1), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(residual=P), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(twin0=P, twin_scale0=P, twin_shift0=P), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(FULL, x1=P), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(FULL, twin0=P), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(FULL, twin1=P, twin_shift1=P), EINVAL),
    ("sige_hip_tile_conv3_nhwc", mix(BIG, C1=1024), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(N=2 ** 16, C1=1024), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(x=Q), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(bias=Q), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(AFF3, scale=Q), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(AFF3, affineB=2, B=2, N=3), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(EDIT2, H=24), EUNSUPPORTED),
    ("sige_hip_tile_conv3_nhwc", mix(EDIT2, B=2), EUNSUPPORTED),
    # ---- sige_hip_tile_conv3_block_nhwc
    ("sige_hip_tile_conv3_block_nhwc", mix(N=0), OK),
    ("sige_hip_tile_conv3_block_nhwc", mix(compute=3), EINVAL),
    ("sige_hip_tile_conv3_block_nhwc", mix(bH=8, bW=8), EUNSUPPORTED),
    ("sige_hip_tile_conv3_block_nhwc", mix(bW=6), EUNSUPPORTED),
    ("sige_hip_tile_conv3_block_nhwc", mix(compute=3, bH=8, bW=8), EINVAL),
    ("sige_hip_tile_conv3_block_nhwc", mix(bH=6, bW=6, N=0), OK),
    ("sige_hip_tile_conv3_block_nhwc", mix(bH=6, bW=6, compute=2), EUNSUPPORTED),
    ("sige_hip_tile_conv3_block_nhwc", mix(bH=6, bW=6, source=0), EINVAL),
    ("sige_hip_tile_conv3_block_nhwc", mix(SG3, bH=6, bW=6, y_f16=1), EUNSUPPORTED),
    ("sige_hip_tile_conv3_block_nhwc", mix(compute=1), EUNSUPPORTED),
    ("sige_hip_tile_conv3_block_nhwc", mix(compute=2), EUNSUPPORTED),
    ("sige_hip_tile_conv3_block_nhwc", mix(compute=1, x=None), EUNSUPPORTED),
    ("sige_hip_tile_conv3_block_nhwc", mix(y_f16=1), EUNSUPPORTED),
    ("sige_hip_tile_conv3_block_nhwc", mix(y_f16=1, N=0), EUNSUPPORTED),
    ("sige_hip_tile_conv3_block_nhwc", mix(residual_f16=1), EUNSUPPORTED),
    ("sige_hip_tile_conv3_block_nhwc", mix(SG3), EUNSUPPORTED),
    ("sige_hip_tile_conv3_block_nhwc", mix(SG3, AFF3, Rx=8, Sx=8), EUNSUPPORTED),
    ("sige_hip_tile_conv3_block_nhwc", mix(SG3, Rx=8, Sx=8, x2=None), EINVAL),
    ("sige_hip_tile_conv3_block_nhwc", mix(SG3, Rx=8, Sx=8, N=0), OK),
    ("sige_hip_tile_conv3_block_nhwc", mix(x=None), EINVAL),
    ("sige_hip_tile_conv3_block_nhwc", mix(source=0), EINVAL),
    ("sige_hip_tile_conv3_block_nhwc", mix(C1=32), EUNSUPPORTED),
    ("sige_hip_tile_conv3_block_nhwc", mix(EDIT2), EUNSUPPORTED),
    ("sige_hip_tile_conv3_block_nhwc", mix(scale=P), EINVAL),
    ("sige_hip_tile_conv3_block_nhwc", mix(twin0=P), EINVAL),
    ("sige_hip_tile_conv3_block_nhwc", mix(x=Q), EUNSUPPORTED),
    ("sige_hip_tile_conv3_block_nhwc", mix(upsample2x=1, H=15), EINVAL),
    ("sige_hip_tile_conv3_block_nhwc", mix(to_full=1), EINVAL),
    ("sige_hip_tile_conv3_block_nhwc", mix(N=2 ** 16, C1=1024), EUNSUPPORTED),
    # ---- sige_hip_wide_conv_nhwc
    ("sige_hip_wide_conv_nhwc", mix(B=0), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(H=0), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(C1=0), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(C2=-1), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(Cout=0), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(prec=-1), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(prec=3), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(x=None), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(packed=None), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(out=None), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(C2=64), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(C1=32), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(C1=32, x=None), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(Cout=32), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(kH=5, kW=5), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(scale=P), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(scale=P, C1=32), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(AFF3, affineB=3), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(activation=1), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(AFF3, activation=7), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(out_scale=P, out_shift=P, out_activation=7), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(out_scale=P), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(out_scale=P, out_activation=7), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(upsample2x=1, H=15), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(BIG, C1=1024), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(x=Q), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(residual=Q), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(workspace=Q, workspace_floats=64), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(stats=Q), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(twin0=P), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(twin0=Q), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(twin1=P, twin_scale1=P), EINVAL),
    ("sige_hip_wide_conv_nhwc", mix(EDIT2, H=24), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(EDIT2, H=8), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(EDIT2, B=2), EUNSUPPORTED),
    ("sige_hip_wide_conv_nhwc", mix(EDIT2, stats=P), EUNSUPPORTED),
    # ---- sige_hip_gather_conv_f32
    ("sige_hip_gather_conv_f32", mix(N=0), OK),
    ("sige_hip_gather_conv_f32", mix(B=0), OK),
    ("sige_hip_gather_conv_f32", mix(N=0, x=None), OK),
    ("sige_hip_gather_conv_f32", mix(B=-1), EINVAL),
    ("sige_hip_gather_conv_f32", mix(Cin=0), EINVAL),
    ("sige_hip_gather_conv_f32", mix(H=0), EINVAL),
    ("sige_hip_gather_conv_f32", mix(N=-1), EINVAL),
    ("sige_hip_gather_conv_f32", mix(activation=7), EUNSUPPORTED),
    ("sige_hip_gather_conv_f32", mix(activation=7, B=-1), EINVAL),
    ("sige_hip_gather_conv_f32", mix(activation=7, N=0), EUNSUPPORTED),
    ("sige_hip_gather_conv_f32", mix(AFF4, scaleH=2), EUNSUPPORTED),
    ("sige_hip_gather_conv_f32", mix(AFF4, scaleH=2, N=0), EUNSUPPORTED),
    ("sige_hip_gather_conv_f32", mix(AFF4, scaleB=3, shiftB=3), EUNSUPPORTED),
    ("sige_hip_gather_conv_f32", mix(scale=P, scaleB=1, scaleC=64, scaleH=1, scaleW=1), EUNSUPPORTED),
    ("sige_hip_gather_conv_f32", mix(AFF4, shiftC=1), EUNSUPPORTED),
    ("sige_hip_gather_conv_f32", mix(activation=1), EUNSUPPORTED),
    ("sige_hip_gather_conv_f32", mix(BIG, Cin=1024), EUNSUPPORTED),
    ("sige_hip_gather_conv_f32", mix(x=None), EINVAL),
    ("sige_hip_gather_conv_f32", mix(packed=None), EINVAL),
    ("sige_hip_gather_conv_f32", mix(active_indices=None), EINVAL),
    ("sige_hip_gather_conv_f32", mix(out=Q), EINVAL),
    ("sige_hip_gather_conv_f32", mix(packed=Q), EINVAL),
    ("sige_hip_gather_conv_f32", mix(EDIT2), EUNSUPPORTED),
    ("sige_hip_gather_conv_f32", mix(EDIT2, out=Q), EINVAL),
    ("sige_hip_gather_conv_f32", mix(kH=5, kW=5), EUNSUPPORTED),
    # ---- sige_hip_gather_conv_nchw_f32
    ("sige_hip_gather_conv_nchw_f32", mix(N=0), OK),
    ("sige_hip_gather_conv_nchw_f32", mix(B=0), OK),
    ("sige_hip_gather_conv_nchw_f32", mix(Ho=0), EINVAL),
    ("sige_hip_gather_conv_nchw_f32", mix(B=-1), EINVAL),
    ("sige_hip_gather_conv_nchw_f32", mix(C2=-1), EINVAL),
    ("sige_hip_gather_conv_nchw_f32", mix(activation=7), EUNSUPPORTED),
    ("sige_hip_gather_conv_nchw_f32", mix(AFF, scaleB=3), EINVAL),
    ("sige_hip_gather_conv_nchw_f32", mix(AFF, scaleC=32), EINVAL),
    ("sige_hip_gather_conv_nchw_f32", mix(AFF, shiftB=3), EINVAL),
    ("sige_hip_gather_conv_nchw_f32", mix(AFF, scaleB=3, activation=7), EUNSUPPORTED),
    ("sige_hip_gather_conv_nchw_f32", mix(AFF, scaleB=3, N=0), EINVAL),
    ("sige_hip_gather_conv_nchw_f32", mix(shift=P, shiftB=1, shiftC=64), EUNSUPPORTED),
    ("sige_hip_gather_conv_nchw_f32", mix(AFF, shiftC=1), EUNSUPPORTED),
    ("sige_hip_gather_conv_nchw_f32", mix(activation=1), EUNSUPPORTED),
    ("sige_hip_gather_conv_nchw_f32", mix(BIG, C1=1024), EUNSUPPORTED),
    ("sige_hip_gather_conv_nchw_f32", mix(x=None), EINVAL),
    ("sige_hip_gather_conv_nchw_f32", mix(out=None), EINVAL),
    ("sige_hip_gather_conv_nchw_f32", mix(C2=64), EINVAL),
    ("sige_hip_gather_conv_nchw_f32", mix(packed=Q), EINVAL),
    ("sige_hip_gather_conv_nchw_f32", mix(C2=64, x2=P, B=2), EUNSUPPORTED),
    ("sige_hip_gather_conv_nchw_f32", mix(EDIT2), EUNSUPPORTED),
    ("sige_hip_gather_conv_nchw_f32", mix(EDIT2, packed=Q), EINVAL),
    ("sige_hip_gather_conv_nchw_f32", mix(kH=5, kW=5), EUNSUPPORTED),
    # ---- sige_hip_scatter_gather_conv_f32
    ("sige_hip_scatter_gather_conv_f32", mix(N=0), OK),
    ("sige_hip_scatter_gather_conv_f32", mix(B=0), OK),
    ("sige_hip_scatter_gather_conv_f32", mix(Rx=0), EINVAL),
    ("sige_hip_scatter_gather_conv_f32", mix(Cout=0), EINVAL),
    ("sige_hip_scatter_gather_conv_f32", mix(W=0), EINVAL),
    ("sige_hip_scatter_gather_conv_f32", mix(activation=7), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_f32", mix(activation=7, Rx=0), EINVAL),
    ("sige_hip_scatter_gather_conv_f32", mix(AFF4, shiftW=2), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_f32", mix(AFF4, scaleC=32), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_f32", mix(shift=P, shiftB=1, shiftC=64, shiftH=1, shiftW=1), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_f32", mix(activation=1), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_f32", mix(BIG, Cin=1024), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_f32", mix(N=2 ** 16, Cin=1024), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_f32", mix(BIG, Cin=1024, N=0), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_f32", mix(x=None), EINVAL),
    ("sige_hip_scatter_gather_conv_f32", mix(y=None), EINVAL),
    ("sige_hip_scatter_gather_conv_f32", mix(scatter_map=None), EINVAL),
    ("sige_hip_scatter_gather_conv_f32", mix(out=Q), EINVAL),
    ("sige_hip_scatter_gather_conv_f32", mix(packed=Q), EINVAL),
    ("sige_hip_scatter_gather_conv_f32", mix(EDIT2), EUNSUPPORTED),
    ("sige_hip_scatter_gather_conv_f32", mix(EDIT2, out=Q), EINVAL),
    ("sige_hip_scatter_gather_conv_f32", mix(kH=5, kW=5), EUNSUPPORTED),
]


@pytest.fixture(scope="module")
def L():
    from sige_amd import build, hip

    build.build(verbose=False)
    return hip.lib()


def answer(L, entry, change):
    """The status of `entry` called with its baseline changed by `change` (EDIT2's pseudo-argument stacks two edits around the call)."""
    names, base = ENTRIES[entry]
    args = dict.fromkeys(names.split())
    for k in args:
        args[k] = None if k in ("stream", "bias") else 0
    args.update(base)
    change = dict(change)
    edits = change.pop("edit_batch", 1)
    assert set(change) <= set(args), (entry, sorted(set(change) - set(args)))
    args.update(change)
    fn = getattr(L, entry).fn  # (the raw ctypes function: no device guard)
    assert len(fn.argtypes) == len(args), entry
    vals = [None if (t.__name__ == "c_void_p" and not v) else v for t, v in zip(fn.argtypes, args.values())]
    L.sige_hip_set_edit_batch(edits)
    try:
        return fn(*vals)
    finally:
        L.sige_hip_set_edit_batch(1)


def test_the_table_covers_every_entry_point():
    assert len(CASES) >= 150
    for entry in ENTRIES:
        mine = [c for e, c, _ in CASES if e == entry]
        assert len(mine) >= 15, entry
        assert len({repr(sorted(c.items())) for c in mine}) == len(mine), entry  # (no case twice)
    assert all(s in (OK, EINVAL, EUNSUPPORTED) for _, _, s in CASES)  # (nothing that the parent answered after a launch)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_entry_status_table(L, entry):
    wrong = []
    for e, change, want in CASES:
        if e == entry:
            got = answer(L, entry, change)
            if got != want:
                wrong.append((change, "recorded %d" % want, "answers %d" % got))
    assert not wrong, wrong
