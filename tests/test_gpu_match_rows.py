"""GPU parity of the product SIFT path with the row-form pass 2 (sift_rows_kernel: one wave per (pair, row subset),
the subset's rows streamed from global memory into the MFMA operand, four subsets and one gather per workgroup)
and with the full-row launch on a fixed grid whose workgroups loop over the item list.  Every output array
(matches, offsets, keep) must equal the oracle's exact matcher followed by its restatement of the match-graph
filters, byte for byte.

  1. train images whose subsets have 0, 1, 2 and 3 rows (16, 17, 32, 33, 48), one 32-row tile short, exact and over
     (511, 512, 513) and more than one 256-row chunk (4096 + 16, 8192); query images of 1, 31, 32, 33, 64, 65 and 97
     rows whose hits fall in ONE subset (one tile, two, the limit of a pass, a second pass over the rows) and spread ones,
  2. planted winners and runner-ups (tests/sift_rows_cases.py, whose key fold tests/test_sift_rows_keys.py pins),
  3. lists longer than the 1024-entry window, riders either side of their threshold, a pair with nothing forwarded,
  4. a job with more full-row items than the launch's grid, and one with none,
  5. images that are not first in the pool, with the filters on,
  6. the parent's pass 2 (SFMX_SIFT_VARIANT=113 of the diagnostic library) and the other screen shape (112).
Fails without the feature: variant 113 is unknown to the parent (the run fails), and SFMX_FULL_ROW_GRID is ignored."""
import ctypes as C

import numpy as np
import pytest

import sfmx
import sift_fp6_cert_ref as cert
import sift_rows_cases as cases
from sfmx import synth
from diag import diagnostic

pytestmark = pytest.mark.gpu

TRAIN_ROWS = (16, 17, 32, 33, 48, 511, 512, 513, 4096 + 16, 8192)
QUERY_ROWS = (1, 31, 32, 33, 64, 65, 97)
RATIOS = (0.7, 1.5)


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


def reference(imgs, pairs, ratio=0.7, distinct=False, min_count=0):
    from oracle import oracle
    em, eoff = oracle.match_pairs(imgs, pairs, ratio)
    return oracle.filter_matches(em, eoff, bool(distinct), min_count)


def assert_same(got, exp):
    (m, off, keep), (em, eoff, ekeep) = got[:3], exp
    assert np.array_equal(off, eoff), (off, eoff)
    if m.tobytes() != em.tobytes():
        bad = np.nonzero(m != em)[0][:5]
        raise AssertionError(f"mismatch at {bad}: got {m[bad]} exp {em[bad]}")
    assert np.array_equal(keep, ekeep)


# --- 1. train image sizes x hits per subset -----------------------------------------------------------
@pytest.fixture(scope="module")
def grid():
    """Two leading images no pair uses; per query size one image whose queries lie near train rows of subset 5 only
    (rows 5 + 16 k, k < 31: inside every train image of 511 rows and more) and one whose queries are spread over
    the 8192 rows; the train images are prefixes of one pool.  Every query image against every train image."""
    rng = np.random.default_rng(7201)
    pool = synth.sift_images(1, 8192, seed=7202, shared=0.0)[0]
    lead = [synth.sift_images(1, 77, seed=7203, shared=0.0)[0], pool[:130].copy()]
    one = [cases.near(rng, pool[5 + 16 * (np.arange(nq) % 31)]) for nq in QUERY_ROWS]
    spread = [cases.near(rng, pool[(np.arange(nq) * 83 + 7 * nq) % 8192]) for nq in QUERY_ROWS]
    trains = [pool[:nt].copy() for nt in TRAIN_ROWS]
    imgs = lead + one + spread + trains
    q0, t0 = len(lead), len(lead) + 2 * len(QUERY_ROWS)
    pairs = np.array([[q0 + qi, t0 + ti] for qi in range(2 * len(QUERY_ROWS)) for ti in range(len(trains))], np.int32)
    return imgs, pairs, {r: reference(imgs, pairs, r) for r in RATIOS}


def test_grid_is_not_vacuous(grid):
    """The restatement of the screen: the 97-query image puts more than 64 certified queries (a second pass over the
    rows) into subset 5 of every train image from 511 rows on, and the short images certify some and refuse some."""
    imgs, pairs, _ = grid
    q97 = imgs[2 + len(QUERY_ROWS) - 1]
    for nt in (511, 513, 8192):
        s = cert.screen(q97, imgs[2 + 2 * len(QUERY_ROWS) + TRAIN_ROWS.index(nt)], 0.7)
        assert (s["forward"] & s["certified"] & (s["r1"] == 5)).sum() > 64
    kinds = set()
    for nt in (16, 17, 32, 33, 48):
        s = cert.screen(q97, imgs[2 + 2 * len(QUERY_ROWS) + TRAIN_ROWS.index(nt)], 1.5)
        kinds |= set((s["certified"][s["forward"]]).tolist())
    assert kinds == {True, False}


@pytest.mark.parametrize("ratio", RATIOS)
def test_train_sizes_and_tiles_per_subset(grid, ratio):
    imgs, pairs, exp = grid
    per_pair = np.diff(exp[ratio][1]).reshape(2 * len(QUERY_ROWS), len(TRAIN_ROWS))
    assert (per_pair[1:len(QUERY_ROWS), 5:] > 20).all(), "vacuous: few matches"
    with diagnostic() as dl:
        got = run(imgs, pairs, ratio, totals=dl)
    assert_same(got, exp[ratio])
    slow, f32, forwarded, full = got[3]
    assert f32 == 0 and forwarded - full > 2000 and full > 0       # both routes ran
    assert_same(run(imgs, pairs, ratio), exp[ratio])               # the product library


# --- 2. planted winners and runner-ups ---------------------------------------------------------------
def test_every_residue_writes():
    imgs, pairs, rows = cases.residue_case()
    s = cert.screen(imgs[0], imgs[1], 0.7)
    assert s["forward"].all() and s["certified"].all() and np.array_equal(s["r1"], np.arange(16))
    with diagnostic() as dl:
        got = run(imgs, pairs, totals=dl)
    assert_same(got, reference(imgs, pairs))
    assert np.array_equal(got[0]["trainIdx"], rows)
    assert got[3] == (0, 0, 16, 0)                 # 16 forwarded, none on the full route: the full-row launch has no item
    assert_same(run(imgs, pairs), reference(imgs, pairs))


@pytest.mark.parametrize("ratio,accepted", [(0.7, [False, True, False, False]), (1.5, [True, True, False, True])])
def test_runner_up_inside_the_subset(ratio, accepted):
    imgs, pairs, rows = cases.runner_up_case()
    s = cert.screen(imgs[0], imgs[1], ratio)
    assert s["forward"].all() and s["certified"].all() and np.array_equal(s["r1"], [1, 4, 7, 10])
    with diagnostic() as dl:
        got = run(imgs, pairs, ratio, totals=dl)
    assert_same(got, reference(imgs, pairs, ratio))
    assert np.array_equal(np.isin(np.arange(4), got[0]["queryIdx"]), accepted)
    if ratio == 1.5:    # the tie at distance 1: the lower index wins
        assert got[0]["trainIdx"][-1] == rows[3] and got[0]["distance"][-1] == 1.0
    assert got[3] == (0, 0, 4, 0)
    assert_same(run(imgs, pairs, ratio), reference(imgs, pairs, ratio))


@pytest.mark.parametrize("ratio", RATIOS)
def test_neighbours_in_different_chunks(ratio):
    imgs, pairs, plan = cases.chunk_case()
    s = cert.screen(imgs[0], imgs[1], ratio)
    assert s["forward"].all() and s["certified"].all() and np.array_equal(s["r1"], [p[0] % 16 for p in plan])
    with diagnostic() as dl:
        got = run(imgs, pairs, ratio, totals=dl)
    exp = reference(imgs, pairs, ratio)
    assert_same(got, exp)
    if ratio == 1.5:    # every query accepted; equal distances: the lower index, in the earlier chunk or the same one
        assert np.array_equal(got[0]["trainIdx"], [min((s1, j1), (s2, j2))[1] for j1, j2, s1, s2 in plan])
    assert got[3] == (0, 0, 6, 0)
    assert_same(run(imgs, pairs, ratio), exp)


# --- 3. lists ----------------------------------------------------------------------------------------
def _mixed_case():
    """More than 1024 certified and more than 32 uncertified queries in one pair, in random list order (hits of every
    subset in every window); three queries per train row for the distinct filter; a pair with few matches."""
    rng = np.random.default_rng(7301)
    base = synth.sift_images(3, 2600, seed=7302, shared=0.0)
    R = base[0].copy()
    R[1:600:2] = cases.near(rng, R[0:600:2])             # 300 near-duplicate train rows in neighbouring subsets
    one = cases.near(rng, R[600:2000])                   # one near neighbour: the certified route
    two = cases.near(rng, R[0:600:2])                    # two near neighbours in two subsets: the full route
    dup = cases.near(rng, np.repeat(R[2000:2100], 3, axis=0))
    L = np.concatenate([one, two, dup, base[1][:300]])
    L = L[rng.permutation(len(L))]
    A = np.concatenate([cases.near(rng, R[2100:2130]), base[2][:400]])
    return [L, R, np.ascontiguousarray(A)], np.array([[0, 1], [2, 1], [1, 0], [2, 0]], np.int32)


@pytest.fixture(scope="module")
def mixed():
    imgs, pairs = _mixed_case()
    refs = {(d, mc): reference(imgs, pairs, 0.7, d, mc) for d, mc in ((0, 0), (1, 100))}
    assert refs[(1, 100)][1][-1] < refs[(0, 0)][1][-1], "distinct = 1 drops no match"
    assert (refs[(1, 100)][2] == 0).any() and (refs[(1, 100)][2] == 1).any(), "min_count clears no pair"
    s = cert.screen(imgs[0], imgs[1], 0.7)
    ok = s["forward"] & s["certified"]
    assert ok.sum() > 1100 and (s["forward"] & ~s["certified"]).sum() > 250
    assert np.bincount(s["r1"][ok], minlength=16).min() > 40      # every subset, more than one tile each
    return imgs, pairs, refs


def test_lists_longer_than_the_window(mixed):
    imgs, pairs, refs = mixed
    with diagnostic() as dl:
        got = run(imgs, pairs, totals=dl)
    assert_same(got, refs[(0, 0)])
    slow, f32, forwarded, full = got[3]
    assert (slow, f32) == (0, 0) and forwarded > 4000 and 250 < full < forwarded - 2000
    assert_same(run(imgs, pairs), refs[(0, 0)])


def _ride_case():
    """Pairs with 32 and with 33 full-route queries (at most 32 ride the row kernel, all 16 subsets and the atomic
    merge, in tiles they share with the ~4 certified queries of each subset; 33 get a full-row item), and between
    them a pair whose train image is empty: nothing forwarded."""
    rng = np.random.default_rng(7311)
    base = synth.sift_images(2, 600, seed=7312, shared=0.0)
    R = base[0].copy()
    R[1:80:2] = cases.near(rng, R[0:80:2])
    imgs = [R, np.zeros((0, 128), np.float32)]
    for k in (32, 33):
        imgs.append(np.concatenate([cases.near(rng, R[200:230]), cases.near(rng, R[0:2 * k:2]), cases.near(rng, R[230:260])]))
    return imgs, np.array([[2, 0], [2, 1], [3, 0], [3, 1], [0, 1]], np.int32)


def test_riders_either_side_of_the_threshold_and_an_empty_pair():
    imgs, pairs = _ride_case()
    for k, n in ((2, 32), (3, 33)):
        s = cert.screen(imgs[k], imgs[0], 0.7)
        assert s["forward"].all() and (~s["certified"]).sum() == n and s["certified"].sum() == 60
    exp = reference(imgs, pairs)
    assert np.array_equal(np.diff(exp[1]) == 0, [False, True, False, True, True])
    with diagnostic() as dl:
        got = run(imgs, pairs, totals=dl)
    assert_same(got, exp)
    assert got[3] == (0, 0, 92 + 93, 65)
    assert_same(run(imgs, pairs), exp)


# --- 4. the full-row launch --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_small():
    """50 images of 64 uniform rows, every ordered pair, at ratio 1.5: every query is forwarded and all but a handful
    go the full route, so each of the 2450 pairs has one full-row item: more than two resident rounds of workgroups."""
    imgs = [np.ascontiguousarray(x) for x in synth.sift_images(50, 64, uniform=True)]
    pairs = np.array([[a, b] for a in range(50) for b in range(50) if a != b], np.int32)
    return imgs, pairs, reference(imgs, pairs, 1.5)


@pytest.mark.parametrize("grid2", [None, 8, 7, 1])
def test_more_full_row_items_than_workgroups(many_small, grid2):
    """grid2: SFMX_FULL_ROW_GRID of the diagnostic library, the full-row launch's grid: each workgroup takes 307, 350
    or all 2450 items; None: the product's grid on both libraries."""
    imgs, pairs, exp = many_small
    assert exp[1][-1] > 10000
    env = {} if grid2 is None else {"SFMX_FULL_ROW_GRID": str(grid2)}
    with diagnostic(**env) as dl:
        got = run(imgs, pairs, 1.5, totals=dl)
    assert_same(got, exp)
    slow, f32, forwarded, full = got[3]
    # fewer than 32 of the 156800 forwarded queries off the full route: every pair keeps more than 32 of its 64, so
    # every pair has its full-row item (the screen certifies a handful of uniform queries)
    assert (slow, f32, forwarded) == (0, 0, 2450 * 64) and full > 2450 * 64 - 32
    if grid2 is None:
        assert_same(run(imgs, pairs, 1.5), exp)


# --- 5. images that are not first in the pool, filters on ---------------------------------------------
def test_not_first_in_the_pool_with_filters(mixed):
    imgs, pairs, refs = mixed
    lead = [synth.sift_images(1, 77, seed=7501, shared=0.0)[0], synth.sift_images(1, 513, seed=7502, shared=0.0)[0]]
    with diagnostic() as dl:
        got = run(lead + imgs, pairs + 2, 0.7, 1, 100, totals=dl)
    assert_same(got, refs[(1, 100)])
    assert got[3][2] > 4000
    assert_same(run(lead + imgs, pairs + 2, 0.7, 1, 100), refs[(1, 100)])


# --- 6. the parent's pass 2 and the other screen shape ------------------------------------------------
@pytest.mark.parametrize("variant", ["113", "112"])
def test_diagnostic_variants_give_the_same_arrays(grid, variant):
    imgs, pairs, exp = grid
    planted = [cases.residue_case()[:2], cases.runner_up_case()[:2], cases.chunk_case()[:2]]
    with diagnostic(SFMX_SIFT_VARIANT=variant) as dl:
        got = run(imgs, pairs, 0.7, totals=dl)
        got_p = [run(i, p, 1.5, totals=dl) for i, p in planted]
    assert_same(got, exp[0.7])
    assert got[3][2] - got[3][3] > 2000                                # the certified route ran
    for (i, p), g in zip(planted, got_p):
        assert_same(g, reference(i, p, 1.5))
        assert g[3][3] == 0
