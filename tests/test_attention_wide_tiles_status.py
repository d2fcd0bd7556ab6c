"""What sige_hip_attention_wide_tiles_f32 ANSWERS, pinned without a launch (the way of tests/test_conv_entry_status.py).

Every case is answered by the host code before any device use: SIGE_HIP_OK through an empty tile list, SIGE_HIP_EINVAL or
SIGE_HIP_EUNSUPPORTED, in the order include/sige_hip.h states -- sizes and row strides, the empty list, null pointers, the
power-of-two rule of stacked edits, then everything the batched entry refuses at Nq = 16 T, Nk = (H / E) W.  The calls go through
the raw ctypes function with made-up pointers (0x1000; 0x1004 = not 16-byte aligned) that the host code never dereferences.  A case
the code wrongly accepted would launch on them, so the module skips itself where a device is present.

The last test pins that the existing entry answers the same questions as before the two entries shared a launcher."""
import pytest
import torch

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
P, Q = 0x1000, 0x1004

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up pointers: never where a wrongly accepted case could launch")

NAMES = "q ldq k ldk v ldv active_indices T H W C heads scale out ldo stream".split()
BASE = dict(q=P, ldq=192, k=P, ldk=384, v=P, ldv=384, active_indices=P, T=3, H=32, W=16, C=192, heads=1, scale=0.07, out=P, ldo=192,
            stream=None)

# (the edit batch around the call, what the case changes against BASE, the status)
CASES = [
    (2, dict(T=0), OK),
    (2, dict(T=0, q=None, k=None, v=None, out=None, active_indices=None), OK),
    (2, dict(T=0, H=12), OK),                       # (the empty list is answered before the height is judged)
    (2, dict(T=-1), EINVAL),
    (2, dict(H=0), EINVAL),
    (2, dict(W=0), EINVAL),
    (2, dict(C=0), EINVAL),
    (2, dict(heads=0), EINVAL),
    (2, dict(ldq=188), EINVAL),
    (2, dict(ldk=188), EINVAL),
    (2, dict(ldv=188), EINVAL),
    (2, dict(ldo=188), EINVAL),
    (2, dict(T=0, ldo=188), EINVAL),
    (2, dict(q=None), EINVAL),
    (2, dict(k=None), EINVAL),
    (2, dict(v=None), EINVAL),
    (2, dict(out=None), EINVAL),
    (2, dict(active_indices=None), EINVAL),
    (2, dict(H=12), EUNSUPPORTED),                  # 6 rows per image: not a power of two
    (2, dict(H=4), EUNSUPPORTED),                   # 2 rows per image: below 4
    (2, dict(H=33), EUNSUPPORTED),                  # E does not divide H
    (4, dict(H=24), EUNSUPPORTED),
    (2, dict(H=12, q=None), EINVAL),                # (null pointers are asked first)
    (1, dict(H=12, C=160, ldq=160, ldo=160), EUNSUPPORTED),  # (E = 1: any height passes; refused for its channels)
    (2, dict(C=160, ldq=160, ldo=160), EUNSUPPORTED),   # attention_tokens' range
    (2, dict(C=528, ldq=528, ldk=1056, ldv=1056, ldo=528), EUNSUPPORTED),
    (2, dict(C=200, ldq=200, ldk=400, ldv=400, ldo=200), EUNSUPPORTED),  # d % 16
    (2, dict(C=384, heads=3, ldq=384, ldk=768, ldv=768, ldo=384), EUNSUPPORTED),  # d = 128 per head
    (2, dict(C=192, heads=5), EUNSUPPORTED),        # C % heads
    (2, dict(q=Q), EUNSUPPORTED),
    (2, dict(k=Q), EUNSUPPORTED),
    (2, dict(v=Q), EUNSUPPORTED),
    (2, dict(out=Q), EUNSUPPORTED),
    (2, dict(ldk=386), EUNSUPPORTED),               # a row stride that is no multiple of 4
    (2, dict(T=65536), EUNSUPPORTED),               # grid y
    (2, dict(H=2 ** 15, W=2 ** 14, ldk=512, ldv=512), EUNSUPPORTED),  # ONE image's K: 2^14 * 2^14 rows of 2 KiB
]


@pytest.fixture(scope="module")
def L():
    from sige_amd import build, hip

    build.build(verbose=False)
    return hip.lib()


def answer(L, entry, names, args, edits=1):
    fn = getattr(L, entry).fn  # (the raw ctypes function: no device guard)
    assert len(fn.argtypes) == len(names), entry
    vals = [None if (t.__name__ == "c_void_p" and not args[n]) else args[n] for t, n in zip(fn.argtypes, names)]
    L.sige_hip_set_edit_batch(edits)
    try:
        return fn(*vals)
    finally:
        L.sige_hip_set_edit_batch(1)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_tiles_entry_status(L, i):
    edits, change, want = CASES[i]
    assert set(change) <= set(BASE)
    got = answer(L, "sige_hip_attention_wide_tiles_f32", NAMES, dict(BASE, **change), edits)
    assert got == want, (edits, change, got, want)


def test_every_refusal_is_answered_before_a_launch(L):
    before = L.sige_hip_launch_count()
    for edits, change, want in CASES:
        if want in (OK, EINVAL, EUNSUPPORTED):
            answer(L, "sige_hip_attention_wide_tiles_f32", NAMES, dict(BASE, **change), edits)
    assert L.sige_hip_launch_count() == before


def test_the_batched_entry_answers_as_before(L):
    names = "q ldq k ldk v ldv B Nq Nk C heads scale out ldo stream".split()
    base = dict(q=P, ldq=192, k=P, ldk=384, v=P, ldv=384, B=1, Nq=48, Nk=100, C=192, heads=1, scale=0.07, out=P, ldo=192, stream=None)
    table = [
        (dict(Nq=0), OK), (dict(B=0), OK), (dict(B=0, q=None), OK), (dict(B=-1), EINVAL), (dict(Nk=0), EINVAL), (dict(C=0), EINVAL),
        (dict(ldv=100), EINVAL), (dict(Nq=0, ldv=100), EINVAL), (dict(q=None), EINVAL), (dict(out=None), EINVAL),
        (dict(Nq=24), EUNSUPPORTED), (dict(Nq=24, q=None), EINVAL), (dict(C=160, ldq=160, ldo=160), EUNSUPPORTED),
        (dict(k=Q), EUNSUPPORTED), (dict(ldq=194), EUNSUPPORTED), (dict(Nk=2 ** 22, ldk=512), EUNSUPPORTED),
        (dict(B=65536), EUNSUPPORTED), (dict(Nq=16 * 65536), EUNSUPPORTED),
        (dict(Nk=2 ** 22, ldk=512, k=Q), EUNSUPPORTED),
    ]
    for edits in (1, 2):  # (the batched entry does not look at the edit batch)
        for change, want in table:
            assert answer(L, "sige_hip_attention_wide_f32", names, dict(base, **change), edits) == want, (edits, change)
