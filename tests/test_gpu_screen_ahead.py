"""GPU parity of the FP6 screen where a row loop that runs one 32-row block ahead can go wrong: at the seams
between blocks and between 128-row stages, in the last (partial) block of an image, and when the ring of stage
buffers wraps (sift_screen6_kernel in csrc/match_device.hpp).  The matcher must give the oracle's arrays byte for
byte (matches, offsets, keep) and take the FP6 screen for every pair (stats()[1] == 0) for

  * train images of 1, 16, 17, 31, 32, 33, 97, 127, 128, 129, 160, 161, 256, 257, 385, 513, 641 and 769 rows:
    every position of the last real row within a block and within a stage, and 1 to 7 stages,
  * query images of 1, 17, 512 and 513 rows,
  * the ratios 0.7 and 1.5,
  * planted neighbours: the train images are prefixes of one pool in which row j2 of each planted pair (j1, j2) is
    a noisy copy of row j1, and the queries are closer copies of row j1, so a query's best row is j1 and its
    second-best j2.  The pairs lie at the first and the last row of a 32-row block, in the last block of one stage
    and the first block of the next, in the last (partial) block of every train image, and inside one block; each
    in two strengths, one whose second neighbour is far enough for Lowe's test at 0.7 to keep the match and one
    whose second neighbour is so close that it rejects it (a screen that loses that row keeps a match the oracle
    does not have),
  * one empty train image, and no image of a pair first in the set,
  * one case in the 32 x 32 x 64 form (SFMX_SIFT_VARIANT=112 of the diagnostic library), which shares the staging.

A case must be able to fail: on the reference, every pair of a 512- or 513-row query image with a train image of at
least 128 rows holds more than 50 matches at ratio 0.7 (a query image of 1 or 17 rows cannot hold 50), and the planted
queries match their row j1 exactly where the construction says so.
Fails without the feature only if the row loop is wrong: the arrays are the parent's."""
import numpy as np
import pytest

import sfmx
from sfmx import synth
from diag import diagnostic

pytestmark = pytest.mark.gpu

TRAIN_ROWS = (1, 16, 17, 31, 32, 33, 97, 127, 128, 129, 160, 161, 256, 257, 385, 513, 641, 769)
QUERY_ROWS = (1, 17, 512, 513)
RATIOS = (0.7, 1.5)
POOL = max(TRAIN_ROWS)
FAR, CLOSE = 14, 1   # noise of the planted second neighbour: Lowe's test at 0.7 keeps / rejects the match


def _near(rng, rows, amp=6):
    return np.clip(rows + rng.integers(-amp, amp + 1, rows.shape), 0, 255).astype(np.float32)


def planted_pairs():
    """(j1, j2, amp, kind): row j2 becomes a copy of row j1 with noise amp.  No row is used twice; the strengths
    alternate within a kind."""
    want = []
    for nt in TRAIN_ROWS:                                        # the last (partial) block of every train image;
        last, first = nt - 1, 32 * ((nt - 1) // 32)              # a block of one row: the row before it
        if last >= 1:
            want.append((last, first + (last - first) // 2 if last > first else last - 1, "last"))
    for b in (2, 6, 9, 14, 21):                                  # first and last row of a 32-row block, both orders
        want += [(32 * b, 32 * b + 31, "block"), (32 * b + 31 - 1, 32 * b + 1, "block")]
    for s in (0, 1, 2, 4, 5):                                    # last block of a stage, first block of the next
        want += [(128 * s + 100 + s, 128 * (s + 1) + 7 + s, "stage"), (128 * (s + 1) + 20 + s, 128 * s + 120 + s, "stage")]
    for b in (1, 5, 10, 13, 17, 23):                             # inside one block
        want.append((32 * b + 5, 32 * b + 9, "inside"))
    used, out, n = set(), [], {}
    for j1, j2, kind in want:
        if j1 in used or j2 in used or j1 == j2 or max(j1, j2) >= POOL:
            continue
        used |= {j1, j2}
        n[kind] = n.get(kind, 0) + 1
        out.append((j1, j2, FAR if n[kind] % 2 else CLOSE, kind))
    return out


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
    """Two leading images that no pair uses, the query images, the train images (prefixes of the planted pool), an
    empty image; every query image against every train image and against the empty one.  Query row i is a copy of
    pool row target[i]: the planted rows j1 first, then rows spread over the pool.  The references of both ratios,
    computed once."""
    rng = np.random.default_rng(6101)
    pool = synth.sift_images(1, POOL, seed=6102, shared=0.0)[0].copy()
    plant = planted_pairs()
    for j1, j2, amp, _ in plant:
        pool[j2] = _near(rng, pool[j1], amp)
    free = np.setdiff1d(np.arange(POOL), [j for p in plant for j in p[:2]])
    target = np.concatenate([[p[0] for p in plant], free[(np.arange(600) * 7) % len(free)]])
    lead = [synth.sift_images(1, 77, seed=6103, shared=0.0)[0], pool[:130].copy()]
    queries = [_near(rng, pool[target[:nq]], 3) for nq in QUERY_ROWS]
    trains = [pool[:nt].copy() for nt in TRAIN_ROWS]
    imgs = lead + queries + trains + [np.zeros((0, 128), np.float32)]
    q0, t0 = len(lead), len(lead) + len(queries)
    pairs = np.array([[q0 + qi, t0 + ti] for qi in range(len(queries)) for ti in range(len(trains) + 1)], np.int32)
    return imgs, pairs, {r: reference(imgs, pairs, r) for r in RATIOS}, plant


def test_reference_has_matches_to_lose_at_the_planted_rows(grid):
    """The construction, on the reference alone: enough matches per pair, the empty image none, and the planted
    queries matched to j1 (far second neighbour) or rejected (close one) wherever the train image holds both rows."""
    imgs, pairs, exp, plant = grid
    m, off, _ = exp[0.7]
    per_pair = np.diff(off).reshape(len(QUERY_ROWS), len(TRAIN_ROWS) + 1)
    assert (per_pair[:, -1] == 0).all()                        # the empty train image: no match
    big = [i for i, nt in enumerate(TRAIN_ROWS) if nt >= 128]
    assert (per_pair[2:, big] > 50).all(), f"vacuous: few matches {per_pair[2:, big]}"
    for kind in ("last", "block", "stage", "inside"):          # every kind of seam in both strengths
        for amp in (FAR, CLOSE):
            assert sum(1 for p in plant if p[2:] == (amp, kind)) >= 3, (kind, amp)
    for ti, nt in enumerate(TRAIN_ROWS):
        p = 3 * (len(TRAIN_ROWS) + 1) + ti                     # the 513-row query image against train image ti
        mm = m[off[p]:off[p + 1]]
        got = dict(zip(mm["queryIdx"].tolist(), mm["trainIdx"].tolist()))
        for qi, (j1, j2, amp, _) in enumerate(plant):
            if max(j1, j2) < nt:
                assert got.get(qi) == (j1 if amp == FAR else None), (nt, qi, j1, j2, amp, got.get(qi))
            elif j1 < nt:
                assert got.get(qi) == j1                       # the second neighbour is not in this image: a match


@pytest.mark.parametrize("ratio", RATIOS)
def test_block_seams_stage_seams_and_ring_wrap(grid, ratio):
    imgs, pairs, exp, _ = grid
    assert_same(run(imgs, pairs, ratio), exp[ratio])


def test_wide_form_keeps_its_two_buffers(grid):
    imgs, pairs, exp, _ = grid
    with diagnostic(SFMX_SIFT_VARIANT="112"):
        assert_same(run(imgs, pairs, 0.7), exp[0.7])
