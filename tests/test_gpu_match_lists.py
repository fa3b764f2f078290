"""GPU parity of the list path of the product SIFT matcher: the forwarded queries are settled
(sift_finish_kernel) and assembled (assemble_lists_kernel) from their list slots, never through the
dense per-query arrays.  Everything is compared, bytes and offsets, with the oracle's exact matcher
followed by its restatement of the match-graph filters."""
import numpy as np
import pytest

import sfmx
from sfmx import synth
import fixtures
import kat

pytestmark = pytest.mark.gpu


def run(imgs, pairs, ratio=0.7, distinct=False, min_count=0):
    m = sfmx.BFMatcher(sfmx.NORM_L2)
    try:
        m.set_images(imgs)
        m.run(pairs, ratio, distinct, min_count)
        out = m.fetch()
        stats = m.stats()
    finally:
        m.close()
    return out + (stats,)


def assert_same(got, off, exp, exp_off):
    assert np.array_equal(off, exp_off), (off, exp_off)
    if got.tobytes() != exp.tobytes():
        bad = np.nonzero(got != exp)[0][:5] if len(got) == len(exp) else []
        raise AssertionError(f"mismatch at {bad}: got {got[bad] if len(bad) else got[:5]} exp {exp[bad] if len(bad) else exp[:5]}")


def per_pair(m, off):
    return [m[off[p]:off[p + 1]].tobytes() for p in range(len(off) - 1)]


# --- filters ------------------------------------------------------------------------------------
def _filter_case():
    """Ragged images; image 4's rows are copies of rows of image 1 moved by 1 in one component: three
    of each of the first 150, so three queries of pair (4, 1) accept the same train row, and one of
    each of the next 200, which the distinct filter keeps; image 3 is tiny."""
    base = synth.sift_images(4, 1300, seed=301)
    imgs = [base[0], base[1][:900], base[2][:513], base[3][:40]]
    dup = np.concatenate([np.repeat(imgs[1][:150], 3, axis=0), imgs[1][150:350]])   # 150 x 3 copies, 200 single ones
    comp = np.arange(len(dup)) % 128
    cur = dup[np.arange(len(dup)), comp]
    dup[np.arange(len(dup)), comp] = np.where(cur >= 255, cur - 1, cur + 1)
    imgs.append(np.ascontiguousarray(dup[np.random.default_rng(302).permutation(len(dup))]))
    pairs = np.array([[0, 1], [4, 1], [0, 2], [3, 0], [1, 2], [2, 0], [4, 0], [1, 4]], np.int32)
    return imgs, pairs


@pytest.fixture(scope="module")
def filter_ref():
    from oracle import oracle
    imgs, pairs = _filter_case()
    em, eoff = oracle.match_pairs(imgs, pairs)
    refs = {(d, mc): oracle.filter_matches(em, eoff, bool(d), mc) for d in (0, 1) for mc in (0, 20)}
    # the oracle alone: the case really exercises both filters
    assert refs[(1, 0)][1][-1] < refs[(0, 0)][1][-1], "distinct = 1 drops no match"
    assert (refs[(0, 20)][2] == 0).any() and (refs[(0, 20)][2] == 1).any(), "min_count = 20 clears no pair"
    return imgs, pairs, refs


@pytest.mark.parametrize("min_count", [0, 20])
@pytest.mark.parametrize("distinct", [0, 1])
def test_filters_vs_oracle(filter_ref, distinct, min_count):
    imgs, pairs, refs = filter_ref
    fm, foff, fkeep = refs[(distinct, min_count)]
    m, off, keep, stats = run(imgs, pairs, 0.7, distinct, min_count)
    assert_same(m, off, fm, foff)
    assert np.array_equal(keep, fkeep)
    assert stats == (0, 0)


# --- list-path and dense-path pairs in one run -----------------------------------------------------
def test_mixed_list_and_dense_pairs():
    """Integral and non-integral images in one run: pair 1 (fp32, dense path) sits between list-path
    pairs, pair 3 has an empty left image, pair 5 is dense again; offsets run over both kinds."""
    from oracle import oracle
    base = synth.sift_images(3, 1300, seed=311)
    rng = np.random.default_rng(312)
    A, C, D = base[0], base[1][:700], base[2][:513]
    B = np.ascontiguousarray(C[:300] + rng.random((300, 128), dtype=np.float32) * 0.25)   # non-integral, near C's rows
    E = np.zeros((0, 128), np.float32)
    imgs = [A, B, C, D, E]
    pairs = np.array([[0, 2], [0, 1], [2, 3], [4, 0], [3, 0], [1, 2], [2, 0]], np.int32)
    for distinct, min_count in ((0, 0), (1, 20)):
        m, off, keep, stats = run(imgs, pairs, 0.7, distinct, min_count)
        em, eoff = oracle.match_pairs(imgs, pairs)
        fm, foff, fkeep = oracle.filter_matches(em, eoff, bool(distinct), min_count)
        assert_same(m, off, fm, foff)
        assert np.array_equal(keep, fkeep)
        assert stats[1] == 2                       # the two pairs that touch the non-integral image
        cnt = np.diff(off)
        assert cnt[3] == 0 and cnt[1] > 0 and cnt[5] > 0 and cnt[0] > 0 and cnt[2] > 0


# --- order and bitmap edges ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_case():
    nqs, nts = [1, 33, 1025, 1300], [0, 1, 2, 17, 700]
    base = synth.sift_images(len(nqs) + len(nts), 1300, seed=321)
    imgs = [b[:n] for b, n in zip(base, nqs + nts)]
    pairs = np.array([[q, len(nqs) + t] for q in range(len(nqs)) for t in range(len(nts))], np.int32)
    return imgs, pairs


def test_every_query_accepted_in_query_order(edge_case):
    """Ratio 1.5 forwards and accepts every query: lists longer than the gather window, nq not a
    multiple of 32, nt = 0 / 1 / 2 / 17; the output is in ascending query order whatever order the
    screen's atomics filled the lists in."""
    from oracle import oracle
    imgs, pairs = edge_case
    m, off, _, stats = run(imgs, pairs, 1.5)
    em, eoff = oracle.match_pairs(imgs, pairs, 1.5)
    assert_same(m, off, em, eoff)
    for p, (l, r) in enumerate(pairs):
        seg = m[off[p]:off[p + 1]]
        if len(imgs[r]) > 0:
            assert np.array_equal(seg["queryIdx"], np.arange(len(imgs[l])))
        else:
            assert len(seg) == 0
    assert stats == (0, 0)


def test_nothing_forwarded(edge_case):
    from oracle import oracle
    imgs, pairs = edge_case
    m, off, keep, stats = run(imgs, pairs, 0.0)
    em, eoff = oracle.match_pairs(imgs, pairs, 0.0)
    assert_same(m, off, em, eoff)
    nt = np.array([len(imgs[r]) for _, r in pairs])
    assert (np.diff(off)[nt >= 2] == 0).all()      # (a single neighbour is accepted at any ratio)
    assert keep.all()                              # min_count 0


# --- determinism ------------------------------------------------------------------------------------
def test_deterministic_across_runs_and_pair_order():
    base = synth.sift_images(4, 1300, seed=331)
    imgs = [base[0], base[1][:1111], base[2][:700], base[3][:257]]
    pairs = sfmx.pairs_unordered(4)
    rev = np.ascontiguousarray(pairs[::-1])
    m = sfmx.BFMatcher(sfmx.NORM_L2)
    try:
        m.set_images(imgs)
        m.run(pairs, 0.8, True, 0)
        a = m.fetch()
        m.run(pairs, 0.8, True, 0)
        b = m.fetch()
        m.set_images(imgs)
        m.run(pairs, 0.8, True, 0)
        c = m.fetch()
        m.run(rev, 0.8, True, 0)
        d = m.fetch()
    finally:
        m.close()
    for x in (b, c):
        assert np.array_equal(a[1], x[1]) and a[0].tobytes() == x[0].tobytes() and np.array_equal(a[2], x[2])
    assert a[1][-1] > 0
    assert per_pair(d[0], d[1]) == per_pair(a[0], a[1])[::-1]


# --- slow path inside the finish kernel ---------------------------------------------------------------
# stats()[0] of the commit before the list path (settle + sift_slow_kernel), read from a run of that
# commit's library on kat.sift_extreme() at the two goldens' ratios.
# 0.7: 0 (the screen rejects the far queries, test_gpu_match.py::test_golden); 1.5: every query is
# forwarded and 250 of the 500 are re-ranked.
PARENT_SLOW = {"sift_extreme": 0, "sift_extreme_r15": 250}


@pytest.mark.parametrize("name", sorted(PARENT_SLOW))
def test_slow_path_count_as_before(name):
    from oracle import oracle
    ratio = fixtures.load(name)["ratio"]
    q, t = kat.sift_extreme()
    pairs = np.array([[0, 1], [1, 0]], np.int32)   # as the goldens
    m, off, _, stats = run([q, t], pairs, ratio)
    em, eoff = oracle.match_pairs([q, t], pairs, ratio)
    assert_same(m, off, em, eoff)
    assert stats[0] == PARENT_SLOW[name]
