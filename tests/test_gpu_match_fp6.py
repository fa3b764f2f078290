"""GPU parity of the product SIFT path with the conservative FP6 screen (sift_screen6_kernel) and the exact
pass 2 over every train row: every output array (matches, offsets, keep) equals the oracle's exact matcher
followed by its restatement of the match-graph filters.  The screen may forward more than the exact int8
screen did, never less (tests/test_sift_fp6_bound.py), so any difference here is a lost or invented match.

Ratio test near its threshold: descriptors are integers, so the closest a query can sit to the ratio is
one unit of s1 on either side of (ratio * d2)^2; the planted queries have exactly those (s1, s2), accepted
and rejected, for the s2 where that gap is narrowest.  d1 <= d2 always, so at ratio 1.5 no query can sit
near the threshold: there the same planted queries are all accepted, and the only rejection left is an
exact duplicate pair of train rows at the query (d1 = d2 = 0), which is planted too."""
import math

import numpy as np
import pytest

import sfmx
from sfmx import synth
from diag import diagnostic

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 15, 16, 17, 33, 65, 513, 600]


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


def assert_same(got, exp):
    (m, off, keep), (em, eoff, ekeep) = got[:3], exp
    assert np.array_equal(off, eoff), (off, eoff)
    if m.tobytes() != em.tobytes():
        bad = np.nonzero(m != em)[0][:5]
        raise AssertionError(f"mismatch at {bad}: got {m[bad]} exp {em[bad]}")
    assert np.array_equal(keep, ekeep)


def reference(imgs, pairs, ratio=0.7, distinct=False, min_count=0):
    from oracle import oracle
    em, eoff = oracle.match_pairs(imgs, pairs, ratio)
    return oracle.filter_matches(em, eoff, bool(distinct), min_count)


# --- every (nq, nt) ---------------------------------------------------------------------------------
def _size_case(uniform):
    base = synth.sift_images(2 * len(SIZES), 600, seed=411, uniform=uniform)
    imgs = [b[:n] for b, n in zip(base, SIZES + SIZES)]
    pairs = np.array([[q, len(SIZES) + t] for q in range(len(SIZES)) for t in range(len(SIZES))], np.int32)
    return imgs, pairs


@pytest.fixture(scope="module", params=["synth", "uniform"])
def size_case(request):
    imgs, pairs = _size_case(request.param == "uniform")
    return imgs, pairs, {r: reference(imgs, pairs, r) for r in (0.7, 1.5)}


@pytest.mark.parametrize("ratio", [0.7, 1.5])
def test_every_size_pair(size_case, ratio):
    imgs, pairs, refs = size_case
    got = run(imgs, pairs, ratio)
    assert_same(got, refs[ratio])
    assert got[3] == (got[3][0], 0)           # no fp32 pair
    assert refs[ratio][1][-1] > 0


# --- one unit of s1 on either side of the ratio -------------------------------------------------------
def _four_squares(s):
    for a in range(math.isqrt(s), -1, -1):
        r1 = s - a * a
        for b in range(math.isqrt(r1), -1, -1):
            r2 = r1 - b * b
            for c in range(math.isqrt(r2), -1, -1):
                d = math.isqrt(r2 - c * c)
                if d * d == r2 - c * c:
                    return a, b, c, d
    raise AssertionError(s)


def _threshold_pairs(ratio=0.7, n=4):
    """-> n x (s1 accepted, s1 rejected, s2): s1 rejected = s1 accepted + 1, for the s2 in [30000, 48000) where
    (ratio * sqrtf(s2))^2 lies closest to an integer boundary."""
    out = []
    for s2 in range(30000, 48000):
        x = float(np.float32(math.sqrt(s2))) * ratio
        s1 = int(x * x)
        while float(np.float32(math.sqrt(s1))) < x:
            s1 += 1
        while not float(np.float32(math.sqrt(s1 - 1))) < x:
            s1 -= 1
        out.append((abs(x * x - s1), s1 - 1, s1, s2))       # s1 - 1 accepted, s1 rejected
    out.sort()
    return [o[1:] for o in out[:n]]


def _planted_case():
    rng = np.random.default_rng(421)
    base = synth.sift_images(2, 600, seed=422)
    q_rows, t_rows, expect = [], [], []
    for acc, rej, s2 in _threshold_pairs():
        for s1, accepted in ((acc, True), (rej, False)):
            q = rng.integers(0, 31, 128).astype(np.float32)
            q[8 + 8 * len(q_rows):16 + 8 * len(q_rows)] = 150      # far from every other planted query
            t1, t2 = q.copy(), q.copy()
            t1[0:4] += _four_squares(s1)
            t2[4:8] += _four_squares(s2)
            q_rows.append(q); t_rows += [t1, t2]; expect.append(accepted)
    dup = rng.integers(0, 31, 128).astype(np.float32)       # d1 = d2 = 0: rejected at every ratio
    dup[8 + 8 * len(q_rows):16 + 8 * len(q_rows)] = 150
    q_rows.append(dup); t_rows += [dup, dup]; expect.append(False)
    nq0 = len(base[0])
    L = np.concatenate([base[0], np.array(q_rows)])
    R = np.concatenate([np.array(t_rows), base[1]])
    assert L.max() <= 255 and R.max() <= 255 and L.min() >= 0
    return [L, R], np.array([[0, 1]], np.int32), nq0, np.array(expect)


@pytest.fixture(scope="module")
def planted():
    imgs, pairs, nq0, expect = _planted_case()
    # the planted rows are the queries' two nearest, at the planted distances (numpy, not the oracle)
    d = ((imgs[0][nq0:, None, :] - imgs[1][None, :, :]) ** 2).sum(-1)
    order = np.argsort(d, axis=1, kind="stable")[:, :2]
    assert np.array_equal(order, np.arange(2 * len(expect)).reshape(-1, 2))
    return imgs, pairs, nq0, expect, {r: reference(imgs, pairs, r) for r in (0.7, 1.5)}


@pytest.mark.parametrize("ratio", [0.7, 1.5])
def test_one_unit_either_side_of_the_ratio(planted, ratio):
    imgs, pairs, nq0, expect, refs = planted
    got = run(imgs, pairs, ratio)
    assert_same(got, refs[ratio])
    accepted = np.isin(np.arange(nq0, len(imgs[0])), got[0]["queryIdx"])
    want = expect if ratio == 0.7 else np.append(np.ones(len(expect) - 1, bool), False)
    assert np.array_equal(accepted, want)


# --- extreme rows -----------------------------------------------------------------------------------
def _extreme_case():
    import sift_fp6_ref
    c = sift_fp6_ref.cases()
    imgs = [c["extreme"][0], c["extreme"][1], c["midpoints"][0], c["midpoints"][1]]
    return imgs, np.array([[0, 1], [1, 0], [2, 3], [3, 2], [0, 3], [2, 1]], np.int32)


@pytest.mark.parametrize("ratio", [0.7, 1.5])
def test_extreme_and_midpoint_rows(ratio):
    imgs, pairs = _extreme_case()
    assert_same(run(imgs, pairs, ratio), reference(imgs, pairs, ratio))


# --- fp32 fallback beside FP6 pairs, filters, the int8 list variant ---------------------------------
def _mixed_case():
    base = synth.sift_images(3, 700, seed=431)
    rng = np.random.default_rng(432)
    A, C, D = base[0], base[1][:600], base[2][:513]
    B = np.ascontiguousarray(C[:300] + rng.random((300, 128), dtype=np.float32) * 0.25)   # non-integral, near C's rows
    dup = np.repeat(C[:120], 3, axis=0)                                                   # three queries per train row
    dup[np.arange(len(dup)), np.arange(len(dup)) % 128] += 1
    imgs = [A, B, C, D, np.clip(dup, 0, 255)]
    pairs = np.array([[0, 2], [0, 1], [2, 3], [4, 2], [1, 2], [2, 0], [3, 4]], np.int32)
    return imgs, pairs


@pytest.fixture(scope="module")
def mixed():
    imgs, pairs = _mixed_case()
    refs = {(d, mc): reference(imgs, pairs, 0.7, d, mc) for d, mc in ((0, 0), (1, 0), (1, 20))}
    assert refs[(1, 0)][1][-1] < refs[(0, 0)][1][-1], "distinct = 1 drops no match"
    assert (refs[(1, 20)][2] == 0).any() and (refs[(1, 20)][2] == 1).any(), "min_count = 20 clears no pair"
    return imgs, pairs, refs


@pytest.mark.parametrize("distinct,min_count", [(0, 0), (1, 0), (1, 20)])
def test_fp32_pairs_beside_fp6_pairs_with_filters(mixed, distinct, min_count):
    imgs, pairs, refs = mixed
    got = run(imgs, pairs, 0.7, distinct, min_count)
    assert_same(got, refs[(distinct, min_count)])
    assert got[3][1] == 2                      # the two pairs that touch the non-integral image


def test_int8_list_variant_gives_the_same_arrays(mixed, size_case):
    """SFMX_SIFT_VARIANT=110 (diagnostic library): the exact int8 screen with subset masks and the subset pass 2."""
    imgs, pairs, refs = mixed
    with diagnostic(SFMX_SIFT_VARIANT="110"):
        got = run(imgs, pairs, 0.7, 1, 20)
        simgs, spairs, srefs = size_case
        got_s = run(simgs, spairs, 0.7)
    assert_same(got, refs[(1, 20)])
    assert_same(got_s, srefs[0.7])
