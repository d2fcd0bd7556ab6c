"""What sige_hip_attention_tokens_f16kv and sige_hip_attention_tokens_tiles_f16kv ANSWER where a call breaks TWO rules at once: which
status wins, pinned without a launch (the way of tests/test_attention_tokens_tiles_status.py, whose made-up pointers and `answer`
these cases use; tests/test_kv16_abi.py pins the single rules).  The order is the one include/sige_hip.h states for the f32 / f16c
entries -- sizes, the empty call, null pointers, (tiles) the power-of-two rule of stacked edits, the shape predicate with
d % 8 == 0, alignment and the 2 GiB of ONE image's K / V counted in halves, the grid -- and every code below is what the library
answered before the three token units shared one launcher and one argument check (csrc/attention_tokens_image.hpp)."""
import pytest
import torch

from tests.test_attention_tokens_tiles_status import BASE, EINVAL, EUNSUPPORTED, NAMES, OK, P, Q, answer

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up pointers: never where a wrongly accepted case could launch")

BATCHED = "sige_hip_attention_tokens_f16kv"
BATCHED_NAMES = "q k v B Nq Nk C heads scale out stream".split()
BATCHED_BASE = dict(q=P, k=P, v=P, B=1, Nq=48, Nk=100, C=160, heads=4, scale=0.15, out=P, stream=None)
BATCHED_CASES = [
    (dict(B=0, Nk=0), EINVAL),                            # sizes before the empty call
    (dict(B=-1, Nq=0), EINVAL),
    (dict(B=0, q=None, out=None), OK),                    # the empty call before null pointers
    (dict(Nq=0, C=176), OK),                              # ... and before the shape (d = 44)
    (dict(Nq=24, q=None), EINVAL),                        # null pointers before the shape
    (dict(C=176, v=None), EINVAL),                        # ... before d % 8
    (dict(Nk=2 ** 23, k=None), EINVAL),                   # ... before the 2 GiB of halves
    (dict(B=2 ** 20, Nq=16 * 2 ** 10, out=None), EINVAL),  # ... before the grid
    (dict(C=176, k=Q), EUNSUPPORTED),                     # d % 8 and alignment
    (dict(Nq=24, Nk=2 ** 23), EUNSUPPORTED),
    (dict(Nk=2 ** 23, v=Q), EUNSUPPORTED),
    (dict(B=2 ** 20, Nq=16 * 2 ** 10, q=Q), EUNSUPPORTED),
    (dict(C=176), EUNSUPPORTED),                          # (the single rules these pairs are made of)
    (dict(Nk=2 ** 23), EUNSUPPORTED),
    (dict(B=2 ** 20, Nq=16 * 2 ** 10), EUNSUPPORTED),
]

TILES = "sige_hip_attention_tokens_tiles_f16kv"
TILES_CASES = [  # (the edit batch around the call, what the case changes against BASE, the status)
    (2, dict(T=0, heads=0), EINVAL),                      # sizes before the empty list
    (2, dict(T=-1, q=None), EINVAL),
    (2, dict(T=0, H=12, C=176, q=None, active_indices=None), OK),  # the empty list before everything else
    (2, dict(H=12, q=None), EINVAL),                      # null pointers before the power-of-two rule
    (2, dict(C=176, active_indices=None), EINVAL),        # ... before d % 8
    (2, dict(T=2 ** 27, out=None), EINVAL),               # ... before 16 T past 2^31
    (2, dict(H=2 ** 15, W=2 ** 15, k=None), EINVAL),      # ... before the 2 GiB of halves
    (2, dict(H=12, C=176), EUNSUPPORTED),                 # the power-of-two rule and d % 8
    (2, dict(H=12, k=Q), EUNSUPPORTED),
    (1, dict(H=12, C=176), EUNSUPPORTED),                 # (E = 1: any height passes; refused for d = 44)
    (2, dict(C=176, v=Q), EUNSUPPORTED),
    (2, dict(H=2 ** 15, W=2 ** 15, out=Q), EUNSUPPORTED),
    (2, dict(T=2 ** 26, C=320, heads=40, q=Q), EUNSUPPORTED),  # the grid (40 heads x 2^26 tiles) and alignment
    (2, dict(C=176), EUNSUPPORTED),                       # (the single rules these pairs are made of)
    (2, dict(H=2 ** 15, W=2 ** 15), EUNSUPPORTED),
    (2, dict(T=2 ** 27), EUNSUPPORTED),
    (2, dict(T=2 ** 26, C=320, heads=40), EUNSUPPORTED),
]


@pytest.fixture(scope="module")
def L():
    from sige_amd import build, hip

    build.build(verbose=False)
    return hip.lib()


def test_which_status_wins_where_two_rules_are_broken(L):
    before = L.sige_hip_launch_count()
    for edits in (1, 2):  # (the batched entry does not look at the edit batch)
        for change, want in BATCHED_CASES:
            assert set(change) <= set(BATCHED_BASE)
            got = answer(L, BATCHED, BATCHED_NAMES, dict(BATCHED_BASE, **change), edits)
            assert got == want, (BATCHED, edits, change, got, want)
    for edits, change, want in TILES_CASES:
        assert set(change) <= set(BASE)
        got = answer(L, TILES, NAMES, dict(BASE, **change), edits)
        assert got == want, (TILES, edits, change, got, want)
    assert L.sige_hip_launch_count() == before and L.sige_hip_get_edit_batch() == 1


def test_the_base_cases_are_shapes_the_library_takes(L):
    assert L.sige_hip_attention_tokens_f16kv_supported(48, 100, 160, 4) == 1
    assert L.sige_hip_attention_tokens_f16kv_supported(16 * 3, 16 * 16, 160, 4) == 1
    assert L.sige_hip_attention_tokens_f16kv_supported(16 * 2 ** 26, 16 * 16, 320, 40) == 1
