"""GPU parity of the FP6 screen in both MFMA shapes: the product path (lib/libsfmx.so) and the other shape
(SFMX_SIFT_VARIANT=112 in the diagnostic library) must both give the oracle's arrays byte for byte (matches,
offsets, keep), as tests/test_gpu_match_onesubset.py asks of the product path.

The cases sit where the 32 x 32 x 64 form (sift_screen6w_kernel: 32-query tiles, 32-row blocks, two K-halves
per lane pair, 8 chains per lane) can go wrong: partial query tiles and a second work item, pad rows inside a
row block and a second LDS stage, a planted neighbour at every row residue mod 32 (every accumulator register
of both lane halves; the certificate must name subset j mod 16), neighbours that differ from the other rows
inside one 32-element K fragment only, the ratio sweep, the filters and an fp32-fallback pair.
Fails without the feature: the diagnostic library rejects variant 112."""
import ctypes as C

import numpy as np
import pytest

import sfmx
import sift_fp6_cert_ref as cert
from sfmx import synth
from diag import diagnostic

pytestmark = pytest.mark.gpu

OTHER = {"SFMX_SIFT_VARIANT": "112"}


def run(imgs, pairs, ratio=0.7, distinct=False, min_count=0, totals=None):
    m = sfmx.BFMatcher(sfmx.NORM_L2)
    try:
        m.set_images(imgs)
        m.run(pairs, ratio, distinct, min_count)
        out = m.fetch()
        stats = m.stats()
        if totals is not None:   # the diagnostic library's reader of the two route counters
            fn = totals.sfmx_diag_matcher_route_totals
            fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
            a, b = C.c_int64(-1), C.c_int64(-1)
            assert fn(m._h, C.byref(a), C.byref(b)) == 0
            stats = stats + (a.value, b.value)
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


def both_shapes(imgs, pairs, ratio=0.7, distinct=False, min_count=0):
    """-> (product library, product path of the diagnostic library, its other shape); the last two with route totals."""
    prod = run(imgs, pairs, ratio, distinct, min_count)
    with diagnostic() as dl:
        same = run(imgs, pairs, ratio, distinct, min_count, totals=dl)
    with diagnostic(**OTHER) as dl:
        other = run(imgs, pairs, ratio, distinct, min_count, totals=dl)
    return prod, same, other


def _near(rng, rows, amp=6):
    return np.clip(rows + rng.integers(-amp, amp + 1, rows.shape), 0, 255).astype(np.float32)


# --- train sizes around the row block and the stage, query counts around the tile and the work item ----
TRAIN_SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 129)
QUERY_COUNTS = (1, 31, 33, 513)


@pytest.fixture(scope="module")
def sizes_case():
    rng = np.random.default_rng(3201)
    pool = synth.sift_images(1, 700, seed=3202, shared=0.0)[0]
    trains = [pool[:nt].copy() for nt in TRAIN_SIZES]
    # queries near rows spread over the pool (many beyond a short train image: rejected or far matches there)
    queries = [_near(rng, pool[(np.arange(nq) * 7) % 140]) for nq in QUERY_COUNTS]
    imgs = queries + trains
    pairs = np.array([[qi, len(queries) + ti] for qi in range(len(queries)) for ti in range(len(trains))], np.int32)
    return imgs, pairs, reference(imgs, pairs)


def test_partial_tiles_second_item_pad_rows_second_stage(sizes_case):
    imgs, pairs, exp = sizes_case
    assert exp[1][-1] > 300, "vacuous: few matches"
    prod, same, other = both_shapes(imgs, pairs)
    for got in (prod, same, other):
        assert_same(got, exp)
    assert same[3][2] > 0 and other[3][2] > 0                 # both forward (the forwarded sets may differ in a few queries)


# --- a planted neighbour at every residue j mod 32 of a 64-row train image ---------------------------
def _residue32_case():
    rng = np.random.default_rng(3211)
    T = synth.sift_images(1, 64, seed=3212, shared=0.0)[0].copy()
    Q = synth.sift_images(1, 32, seed=3213, shared=0.0)[0].copy()
    rows = [j + 32 * (j & 1) for j in range(32)]              # residue j, both row blocks
    for j, r in enumerate(rows):
        T[r] = _near(rng, Q[j], 3)                            # the neighbour; every other row is a distant runner-up
    return [Q, T], np.array([[0, 1]], np.int32), rows


def test_every_residue_mod_32():
    imgs, pairs, rows = _residue32_case()
    s = cert.screen(imgs[0], imgs[1], 0.7)
    assert s["forward"].all() and s["certified"].all()
    assert np.array_equal(s["r1"], np.arange(32) % 16)
    exp = reference(imgs, pairs)
    prod, same, other = both_shapes(imgs, pairs)
    for got in (prod, same, other):
        assert_same(got, exp)
        assert np.array_equal(got[0]["queryIdx"], np.arange(32)) and np.array_equal(got[0]["trainIdx"], rows)
    for got in (same, other):                                 # every query took the subset route: r1 = j mod 16
        slow, f32, forwarded, full = got[3]
        assert (slow, f32) == (0, 0) and forwarded == 32 and full == 0 and forwarded > full


# --- neighbours that differ from every other row inside one 32-element K fragment only ---------------
def _fragment_case():
    rng = np.random.default_rng(3221)
    base = synth.sift_images(1, 1, seed=3222, shared=0.0)[0][0]
    imgs, pairs = [], []
    for f in range(4):
        T = np.tile(base, (48, 1)).astype(np.float32)
        T[:, 32 * f:32 * f + 32] = rng.integers(0, 120, (48, 32))
        Q = T[rng.permutation(48)[:20]].copy()
        Q[:, 32 * f:32 * f + 32] = _near(rng, Q[:, 32 * f:32 * f + 32], 2)
        imgs += [Q, T]
        pairs.append([2 * f, 2 * f + 1])
    return imgs, np.array(pairs, np.int32)


def test_one_fragment_decides():
    imgs, pairs = _fragment_case()
    exp = reference(imgs, pairs)
    assert (np.diff(exp[1]) >= 15).all(), "vacuous: the planted neighbours do not match"
    prod, same, other = both_shapes(imgs, pairs)
    for got in (prod, same, other):
        assert_same(got, exp)


# --- the ratio sweep, the filters and an fp32-fallback pair in one run ------------------------------
@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(3231)
    base = synth.sift_images(3, 700, seed=3232, shared=0.0)
    R = base[0].copy()
    R[1:200:2] = _near(rng, R[0:200:2])                       # near-duplicate train rows in neighbouring subsets
    L = np.concatenate([_near(rng, R[200:600]), _near(rng, R[0:200:2]), _near(rng, np.repeat(R[600:640], 3, axis=0)),
                        base[1][:150]])
    L = L[rng.permutation(len(L))]
    A = np.concatenate([_near(rng, R[640:660]), base[2][:200]])   # few matches: min_count clears its pairs
    F = _near(rng, R[300:420]) + np.float32(0.25)                  # non-integer values: the fp32 fallback
    imgs = [L, R, np.ascontiguousarray(A), np.ascontiguousarray(F)]
    pairs = np.array([[0, 1], [2, 1], [1, 0], [3, 1]], np.int32)
    return imgs, pairs


@pytest.mark.parametrize("ratio,distinct,min_count", [(0.7, 0, 0), (1.0, 0, 0), (1.5, 0, 0), (0.7, 1, 0), (0.7, 1, 100)])
def test_ratios_filters_and_fp32_pair(mixed, ratio, distinct, min_count):
    imgs, pairs = mixed
    exp = reference(imgs, pairs, ratio, distinct, min_count)
    assert exp[1][-1] > 400
    if min_count:
        assert (exp[2] == 0).any() and (exp[2] == 1).any(), "min_count clears no pair"
    prod, same, other = both_shapes(imgs, pairs, ratio, distinct, min_count)
    for got in (prod, same, other):
        assert_same(got, exp)
    for got in (same, other):
        slow, f32, forwarded, full = got[3]
        assert f32 == 1 and forwarded > 400
        if ratio == 0.7:
            assert 0 < full < forwarded                       # both routes ran
