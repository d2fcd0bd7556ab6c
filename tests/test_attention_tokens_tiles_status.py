"""What sige_hip_attention_tokens_tiles_f32 and sige_hip_attention_tokens_tiles_f16c ANSWER, pinned without a launch (the way of
tests/test_attention_wide_tiles_status.py).

Every case is answered by the host code before any device use: SIGE_HIP_OK through an empty tile list, SIGE_HIP_EINVAL or
SIGE_HIP_EUNSUPPORTED, in the order include/sige_hip.h states -- sizes, the empty list, null pointers (the index list among them),
the power-of-two rule of stacked edits, then everything sige_hip_attention_tokens_f32 refuses at Nq = 16 T, Nk = (H / E) W.  The
calls go through the raw ctypes function with made-up pointers (0x1000; 0x1004 = not 16-byte aligned) that the host code never
dereferences.  A case the code wrongly accepted would launch on them, so the module skips itself where a device is present.

The last test pins that the batched entries answer the same questions as before they shared a launcher with these."""
import pytest
import torch

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
P, Q = 0x1000, 0x1004

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up pointers: never where a wrongly accepted case could launch")

ENTRIES = ("sige_hip_attention_tokens_tiles_f32", "sige_hip_attention_tokens_tiles_f16c")
NAMES = "q k v active_indices T H W C heads scale out stream".split()
BASE = dict(q=P, k=P, v=P, active_indices=P, T=3, H=32, W=16, C=160, heads=4, scale=0.15, out=P, stream=None)

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
    (2, dict(T=0, heads=0), EINVAL),                # (sizes before the empty list)
    (2, dict(q=None), EINVAL),
    (2, dict(k=None), EINVAL),
    (2, dict(v=None), EINVAL),
    (2, dict(out=None), EINVAL),
    (2, dict(active_indices=None), EINVAL),
    (1, dict(active_indices=None), EINVAL),         # (with one edit too: the argument is not optional)
    (2, dict(H=12), EUNSUPPORTED),                  # 6 rows per image: not a power of two
    (5, dict(H=24), EUNSUPPORTED),                  # E does not divide H
    (2, dict(H=4), EUNSUPPORTED),                   # 2 rows per image: below 4
    (2, dict(H=33), EUNSUPPORTED),
    (2, dict(H=12, q=None), EINVAL),                # (null pointers are asked first)
    (1, dict(H=12, C=164, heads=1), EUNSUPPORTED),  # (E = 1: any height passes; refused for its head size)
    (2, dict(C=164, heads=1), EUNSUPPORTED),        # d = 164 > 160
    (2, dict(C=168, heads=4), EUNSUPPORTED),        # d = 42: d % 4
    (2, dict(C=160, heads=3), EUNSUPPORTED),        # C % heads
    (2, dict(C=176, heads=1), EUNSUPPORTED),        # d = 176: past the widest unit count
    (2, dict(q=Q), EUNSUPPORTED),
    (2, dict(k=Q), EUNSUPPORTED),
    (2, dict(v=Q), EUNSUPPORTED),
    (2, dict(out=Q), EUNSUPPORTED),
    (2, dict(H=2 ** 15, W=2 ** 15), EUNSUPPORTED),  # ONE image's K: 2^14 * 2^15 rows of 640 bytes
    (2, dict(T=2 ** 27), EUNSUPPORTED),             # 16 T past 2^31
    (2, dict(T=2 ** 26, heads=40), EUNSUPPORTED),   # the grid: 40 heads x 2^26 tiles
]
ACCEPTED_SHAPES = [  # (what the refusals above are NOT about: the same calls would be launched -- judged by the shape predicate alone)
    (16 * 3, 16 * 16, 160, 4),
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


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("i", range(len(CASES)))
def test_tiles_entry_status(L, i, entry):
    edits, change, want = CASES[i]
    assert set(change) <= set(BASE)
    got = answer(L, entry, NAMES, dict(BASE, **change), edits)
    assert got == want, (entry, edits, change, got, want)
    assert L.sige_hip_get_edit_batch() == 1


def test_the_base_case_is_a_shape_the_library_takes(L):
    for Nq, Nk, C, heads in ACCEPTED_SHAPES:
        assert L.sige_hip_attention_tokens_supported(Nq, Nk, C, heads) == 1


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_refusal_is_answered_before_a_launch(L, entry):
    before = L.sige_hip_launch_count()
    for edits, change, want in CASES:
        answer(L, entry, NAMES, dict(BASE, **change), edits)
    assert L.sige_hip_launch_count() == before


@pytest.mark.parametrize("entry", ("sige_hip_attention_tokens_f32", "sige_hip_attention_tokens_f16c"))
def test_the_batched_entries_answer_as_before(L, entry):
    names = "q k v B Nq Nk C heads scale out stream".split()
    base = dict(q=P, k=P, v=P, B=1, Nq=48, Nk=100, C=160, heads=4, scale=0.15, out=P, stream=None)
    table = [
        (dict(Nq=0), OK), (dict(B=0), OK), (dict(B=0, q=None), OK), (dict(B=-1), EINVAL), (dict(Nk=0), EINVAL), (dict(C=0), EINVAL),
        (dict(q=None), EINVAL), (dict(out=None), EINVAL), (dict(Nq=24), EUNSUPPORTED), (dict(Nq=24, q=None), EINVAL),
        (dict(C=164, heads=1), EUNSUPPORTED), (dict(k=Q), EUNSUPPORTED), (dict(Nk=2 ** 22), EUNSUPPORTED),
        (dict(Nk=2 ** 22, k=Q), EUNSUPPORTED), (dict(B=2 ** 20, Nq=16 * 2 ** 10), EUNSUPPORTED),
    ]
    for edits in (1, 2):  # (the batched entries do not look at the edit batch)
        for change, want in table:
            assert answer(L, entry, names, dict(base, **change), edits) == want, (edits, change)
