"""GPU: the product SIFT run with two launches folded into their neighbours.  Workgroup 0 of sift_rows_kernel builds
the full-row work list before its own item (also when its own pair has no forwarded query and it returns), and the
last workgroup of sift_finish_kernel to finish scans the pairs' counts into the offsets and leaves its ticket at zero.

Every comparison is byte for byte with the oracle (matches, offsets, keep).  The cases sit where the folds can go
wrong: pair counts around the 256 threads of the list builder and the 1024 of the scan (1, 2, 255, 256, 257, 1023,
1024, 1035), pairs without a forwarded query at both ends of the pair order, empty images, no pair at all, an
fp32-fallback pair among list pairs (one scan over both kinds), pairs with 32 and 33 full-route queries (the work
list empty and not) several at once behind an empty first pair, three runs on one matcher (the ticket is back at
zero), and the match-graph filters.
Fails without the feature only where the parent would: the results do not change with the number of launches."""
import ctypes as C

import numpy as np
import pytest

import sfmx
import sift_fp6_cert_ref as cert
from sfmx import synth
from diag import diagnostic
from test_gpu_match_onesubset import _ride_case, assert_same, reference

pytestmark = pytest.mark.gpu

N_IMG = 46                                   # 46 * 45 / 2 = 1035 pairs
COUNTS = (1, 2, 255, 256, 257, 1023, 1024, 1035)


@pytest.fixture(scope="module")
def small_set():
    """46 images of 16 to 64 rows on synth's ring of shared landmarks, all pairs, and the oracle's result per pair."""
    base = synth.sift_images(N_IMG, 64, seed=7401, shared=0.5)
    imgs = [np.ascontiguousarray(a[:16 + (5 * i) % 49]) for i, a in enumerate(base)]
    assert min(map(len, imgs)) == 16 and max(map(len, imgs)) == 64
    pairs = sfmx.pairs_unordered(N_IMG)
    assert len(pairs) == 1035
    from oracle import oracle
    em, eoff = oracle.match_pairs(imgs, pairs, 0.7)
    assert eoff[-1] > 1000
    return imgs, pairs, em, eoff


@pytest.fixture(scope="module")
def matcher(small_set):
    m = sfmx.BFMatcher(sfmx.NORM_L2)
    m.set_images(small_set[0])
    yield m
    m.close()


def _go(m, pairs, ratio=0.7, distinct=False, min_count=0):
    m.run(pairs, ratio, distinct, min_count)
    return m.fetch()


def _totals(dl, m):
    fn = dl.sfmx_diag_matcher_route_totals
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    a, b = C.c_int64(-1), C.c_int64(-1)
    assert fn(m._h, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


@pytest.mark.parametrize("k", COUNTS)
def test_pair_counts(small_set, matcher, k):
    imgs, pairs, em, eoff = small_set
    from oracle import oracle
    # without filters a pair's matches do not depend on the other pairs: the first k pairs are the oracle's prefix
    exp = oracle.filter_matches(em[:eoff[k]], eoff[:k + 1], False, 0)
    assert_same(_go(matcher, pairs[:k]), exp)


def test_rerun_without_set_images(small_set, matcher):
    """Two pair lists, then the first again: the third result equals the first only if the ticket went back to zero."""
    imgs, pairs, _, _ = small_set
    a, b = pairs[100:400], pairs[::-1][:257]
    first = _go(matcher, a)
    assert_same(first, reference(imgs, a))
    assert_same(_go(matcher, b), reference(imgs, b))
    assert_same(_go(matcher, a), first)


def test_filters_on_a_multi_pair_run(small_set, matcher):
    imgs, pairs, _, _ = small_set
    p = pairs[:257]
    exp = reference(imgs, p, 0.97, True, 8)      # (at 0.97 several queries share a train row)
    assert (exp[2] == 0).any() and (exp[2] == 1).any(), "min_count clears no pair, or every pair"
    assert exp[1][-1] < reference(imgs, p, 0.97)[1][-1], "distinct drops no match"
    assert_same(_go(matcher, p, 0.97, True, 8), exp)


def test_no_pair(matcher):
    m, off, keep = _go(matcher, np.zeros((0, 2), np.int32))
    assert len(m) == 0 and np.array_equal(off, [0]) and len(keep) == 0


def _flat(seed, rows=40):
    """A train image of identical rows: d1 == d2 for every query, so Lowe's test fails and the screen forwards nothing."""
    row = synth.sift_images(1, 1, seed=seed, shared=0.0)[0]
    return np.repeat(row, rows, axis=0).copy()


def test_pairs_without_a_forwarded_query_at_both_ends_of_the_pair_order():
    """The pair order is by train image: train image 0 and the last one are flat, so the first and the last pair of
    the order (the designated workgroup's own pair among them) have no forwarded query; so has the pair of an empty
    left image, and the pair of an empty right image has no neighbour at all."""
    base = synth.sift_images(4, 48, seed=7411, shared=0.5)
    empty = np.zeros((0, 128), np.float32)
    imgs = [_flat(7412), base[0], base[1], base[2][:33], empty, base[3][:17], _flat(7413)]
    for q in (1, 2):
        for t in (0, 6):
            assert not cert.screen(imgs[q], imgs[t], 0.7)["forward"].any()
    pairs = np.array([[1, 2], [2, 6], [1, 6], [2, 1], [3, 1], [4, 2], [2, 4], [5, 3], [1, 0], [2, 0], [3, 5]], np.int32)
    exp = reference(imgs, pairs)
    assert exp[1][-1] > 10
    with diagnostic() as dl:
        m = sfmx.BFMatcher(sfmx.NORM_L2)
        try:
            m.set_images(imgs)
            assert_same(_go(m, pairs), exp)
            only_empty = np.array([[4, 1], [4, 2]], np.int32)   # no work item at all: nothing is launched behind the fill
            assert_same(_go(m, only_empty), reference(imgs, only_empty))
            assert _totals(dl, m) == (0, 0)
            assert_same(_go(m, pairs), exp)
        finally:
            m.close()
    m = sfmx.BFMatcher(sfmx.NORM_L2)                            # the product library
    try:
        m.set_images(imgs)
        assert_same(_go(m, pairs), exp)
    finally:
        m.close()


def test_fp32_fallback_pair_among_list_pairs():
    """Host sources, one image with a non-integral value: its pairs go through the dense arrays, the others through
    the lists, and the offsets are one scan over both kinds."""
    imgs = [a.copy() for a in synth.sift_images(4, 60, seed=7421, shared=0.5)]
    imgs[2][5, 5] += np.float32(0.5)
    pairs = np.array([[0, 1], [2, 1], [1, 3], [3, 2], [0, 3], [1, 0]], np.int32)
    for distinct, min_count in ((False, 0), (True, 3)):
        exp = reference(imgs, pairs, 0.7, distinct, min_count)
        m = sfmx.BFMatcher(sfmx.NORM_L2)
        try:
            m.set_images(imgs)
            got = _go(m, pairs, 0.7, distinct, min_count)
            assert m.stats() == (0, 2)
        finally:
            m.close()
        assert_same(got, exp)
        assert 0 < exp[1][2] - exp[1][1] and 0 < exp[1][1]      # the fallback pair and a list pair both have matches


def test_full_route_items_behind_an_empty_first_pair():
    """tests/test_gpu_match_onesubset.py's construction: 32 full-route queries ride the rows kernel (no item), 33 get
    a full-row item.  Several such pairs at once; the first pair of the order, the list builder's own, is empty."""
    imgs, _ = _ride_case()                       # [R, 32 full-route queries + 60 certified, 33 + 60]
    imgs = imgs + [np.zeros((0, 128), np.float32)]
    cases = ((np.array([[3, 0], [1, 0], [1, 0]], np.int32), (2 * 92, 2 * 32)),                       # the list stays empty
             (np.array([[3, 0], [2, 0], [1, 0], [2, 0], [1, 0]], np.int32), (2 * 185, 2 * 65)))     # two items, two riders
    with diagnostic() as dl:
        m = sfmx.BFMatcher(sfmx.NORM_L2)
        try:
            m.set_images(imgs)
            for pairs, totals in cases:
                got = _go(m, pairs)
                assert m.stats() == (0, 0)
                assert _totals(dl, m) == totals
                assert_same(got, reference(imgs, pairs))
        finally:
            m.close()
    m = sfmx.BFMatcher(sfmx.NORM_L2)             # the product library
    try:
        m.set_images(imgs)
        for pairs, _ in cases:
            assert_same(_go(m, pairs), reference(imgs, pairs))
    finally:
        m.close()
