"""GPU parity of the FP6 screen where its staging can go wrong: the LDS stages are filled by LDS-DMA through buffer
resources over the train image's padded rows and keys, with the stage advance in the scalar offset
(Screen6Stage in csrc/match_kernels.hip), and the lanes read them at bases computed once.  The matcher must give
the oracle's arrays byte for byte (matches, offsets, keep) for

  * train images of 1, 2, 127, 128, 129, 255, 256, 257 and 385 rows: 1, 2, 3 and 4 stages of 128 rows, odd and
    even counts for the double buffer, a partial last stage,
  * query images of 1, 511, 512 and 513 rows: partial tiles and a second work item,
  * images that are third and fourth in a set of four, and a longer set in which no image of a pair is first,
    so that the bases of the buffer resources are not the base of the allocation,
  * one empty train image,
  * the ratios 0.7 and 1.5,

on the product library, and on one case in the 32 x 32 x 64 form (SFMX_SIFT_VARIANT=112 of the diagnostic library),
which shares the staging.
Fails without the feature only if the staging is wrong: the arrays are the parent's."""
import numpy as np
import pytest

import sfmx
from sfmx import synth
from diag import diagnostic

pytestmark = pytest.mark.gpu

TRAIN_ROWS = (1, 2, 127, 128, 129, 255, 256, 257, 385)
QUERY_ROWS = (1, 511, 512, 513)
RATIOS = (0.7, 1.5)


def _near(rng, rows, amp=6):
    return np.clip(rows + rng.integers(-amp, amp + 1, rows.shape), 0, 255).astype(np.float32)


def run(imgs, pairs, ratio):
    m = sfmx.BFMatcher(sfmx.NORM_L2)
    try:
        m.set_images(imgs)
        m.run(pairs, ratio, False, 0)
        out = m.fetch()
        slow, f32 = m.stats()
    finally:
        m.close()
    assert f32 == 0                                            # every pair took the FP6 screen
    return out


def reference(imgs, pairs, ratio):
    from oracle import oracle
    em, eoff = oracle.match_pairs(imgs, pairs, ratio)
    return oracle.filter_matches(em, eoff, False, 0)


def assert_same(got, exp):
    (m, off, keep), (em, eoff, ekeep) = got[:3], exp
    assert np.array_equal(off, eoff), (off, eoff)
    if m.tobytes() != em.tobytes():
        bad = np.nonzero(m != em)[0][:5]
        raise AssertionError(f"mismatch at {bad}: got {m[bad]} exp {em[bad]}")
    assert np.array_equal(keep, ekeep)


@pytest.fixture(scope="module")
def grid():
    """Two leading images that no pair uses, the query images, the train images, an empty image; every query image
    against every train image and against the empty one.  The references of both ratios, computed once."""
    rng = np.random.default_rng(5101)
    pool = synth.sift_images(1, 400, seed=5102, shared=0.0)[0]
    lead = [synth.sift_images(1, 77, seed=5103, shared=0.0)[0], pool[:130].copy()]
    # queries near rows spread over the whole pool: their neighbours lie in every stage of the longer train images
    queries = [_near(rng, pool[(np.arange(nq) * 7) % 385]) for nq in QUERY_ROWS]
    trains = [pool[:nt].copy() for nt in TRAIN_ROWS]
    imgs = lead + queries + trains + [np.zeros((0, 128), np.float32)]
    q0, t0 = len(lead), len(lead) + len(queries)
    pairs = np.array([[q0 + qi, t0 + ti] for qi in range(len(queries)) for ti in range(len(trains) + 1)], np.int32)
    return imgs, pairs, {r: reference(imgs, pairs, r) for r in RATIOS}


@pytest.mark.parametrize("ratio", RATIOS)
def test_stage_counts_query_counts_and_bases(grid, ratio):
    imgs, pairs, exp = grid
    e = exp[ratio]
    per_pair = np.diff(e[1]).reshape(len(QUERY_ROWS), len(TRAIN_ROWS) + 1)
    assert (per_pair[:, -1] == 0).all()                        # the empty train image: no match
    assert (per_pair[1:, 3:-1] > 50).all(), "vacuous: few matches"   # every longer pair has matches to lose
    assert_same(run(imgs, pairs, ratio), e)


def test_third_and_fourth_of_four():
    rng = np.random.default_rng(5111)
    base = synth.sift_images(3, 300, seed=5112, shared=0.0)
    T = base[2][:257].copy()
    Q = _near(rng, T[(np.arange(513) * 5) % 257])
    imgs = [base[0][:65].copy(), base[1][:129].copy(), Q, T]
    pairs = np.array([[2, 3], [3, 2]], np.int32)
    for ratio in RATIOS:
        exp = reference(imgs, pairs, ratio)
        assert exp[1][-1] > 300
        assert_same(run(imgs, pairs, ratio), exp)


def test_wide_form_shares_the_staging(grid):
    imgs, pairs, exp = grid
    with diagnostic(SFMX_SIFT_VARIANT="112"):
        assert_same(run(imgs, pairs, 0.7), exp[0.7])
