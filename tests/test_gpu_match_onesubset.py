"""GPU parity of the product SIFT path with the one-subset pass 2: a forwarded query the FP6 screen certifies
(fp6::certified) is settled by the exact top-2 of one row subset (train rows j = r1 mod 16), every other one by
the exact pass 2 over every train row.  Every output array (matches, offsets, keep) must equal the oracle's
exact matcher followed by its restatement of the match-graph filters, byte for byte, with stats() unchanged.

The planted cases put a query's neighbours where the one-subset route can go wrong: every residue, a subset
of one or two rows, a runner-up inside the subset that decides Lowe's test either way, ties, the two
neighbours in different 256-row chunks of the subset, a subset whose second row lies in the float-sqrt
collision range, lists longer than the subset kernel's 1024-entry window with both kinds of slot, and the
filters.  tests/sift_fp6_cert_ref.py says which planted queries are certified, and the diagnostic library's
route totals (forwarded, full-route) say which route ran.
Fails without the feature: no query takes the subset route (full-route total == forwarded)."""
import ctypes as C
import math

import numpy as np
import pytest

import sfmx
import sift_fp6_cert_ref as cert
from sfmx import synth
from diag import diagnostic

pytestmark = pytest.mark.gpu


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


def _at(q, s, where=0):
    """A copy of q at squared distance s: four squares added to elements where .. where + 3 (q is small there)."""
    t = q.copy()
    t[where:where + 4] += _four_squares(s)
    assert t.max() <= 255
    return t


def _queries(n, seed):
    """n SIFT-like rows, far from each other and from every other image, elements 0..15 small."""
    q = synth.sift_images(1, n, seed=seed, shared=0.0)[0].copy()
    q[:, :16] = np.minimum(q[:, :16], 20)
    return q


def _certified(q, t, ratio=0.7):
    s = cert.screen(q, t, ratio)
    return s["forward"], s["certified"], s["r1"]


# --- an isolated planted neighbour in each of the 16 residues ----------------------------------------
def _residue_case():
    T = synth.sift_images(1, 600, seed=511, shared=0.0)[0].copy()
    Q = _queries(16, 512)
    rows = [16 * (3 + 2 * r) + r for r in range(16)]            # residue r, different blocks of 16
    for r, j in enumerate(rows):
        T[j] = _at(Q[r], 900 + r)
    return [Q, T], np.array([[0, 1]], np.int32), rows


def test_every_residue():
    imgs, pairs, rows = _residue_case()
    fwd, c, r1 = _certified(imgs[0], imgs[1])
    assert fwd.all() and c.all() and np.array_equal(r1, np.arange(16))
    with diagnostic() as dl:
        got = run(imgs, pairs, totals=dl)
    assert_same(got, reference(imgs, pairs))
    assert np.array_equal(got[0]["trainIdx"], rows)
    assert got[3] == (0, 0, 16, 0)                # no slow query, no fp32 pair; 16 forwarded, none on the full route
    assert_same(run(imgs, pairs), reference(imgs, pairs))          # the product library


# --- a subset of one row (the full route) and of two --------------------------------------------------
def _short_subset_case():
    base = synth.sift_images(1, 40, seed=521, shared=0.0)[0]
    Q = _queries(1, 522)
    imgs = [Q]
    for j, nt in ((5, 21), (5, 22), (0, 16), (0, 17), (15, 31), (15, 32)):   # nt = r1 + 16, r1 + 17
        T = base[:nt].copy()
        T[j] = _at(Q[0], 400)
        imgs.append(T)
    pairs = np.array([[0, k] for k in range(1, 7)], np.int32)
    return imgs, pairs


def test_subset_of_one_row_and_of_two():
    imgs, pairs = _short_subset_case()
    want = []
    for k in range(1, 7):
        fwd, c, r1 = _certified(imgs[0], imgs[k])
        assert fwd.all()
        want.append(bool(c[0]))
    assert want == [False, True, False, True, False, True]
    with diagnostic() as dl:
        got = run(imgs, pairs, totals=dl)
    assert_same(got, reference(imgs, pairs))
    assert got[1][-1] == 6
    assert got[3] == (0, 0, 6, 3)


# --- a runner-up at j + 16: Lowe fails, passes, identical rows, a distance-1 tie ---------------------
def _runner_up_case():
    T = synth.sift_images(1, 300, seed=531, shared=0.0)[0].copy()
    Q = _queries(4, 532)
    # (s1, s2): Lowe at 0.7 fails (sqrt 4000 = 63.2 >= 0.7 * 70.7), passes (31.6 < 49.5), identical rows, tie at 1
    for k, (s1, s2) in enumerate(((4000, 5000), (1000, 5000), (0, 0), (1, 1))):
        j = 16 * (2 + 3 * k) + (3 * k + 1)
        T[j] = _at(Q[k], s1, 0)
        T[j + 16] = _at(Q[k], s2, 4)
    return [Q, T], np.array([[0, 1]], np.int32)


@pytest.mark.parametrize("ratio,accepted", [(0.7, [False, True, False, False]), (1.5, [True, True, False, True])])
def test_runner_up_inside_the_subset(ratio, accepted):
    imgs, pairs = _runner_up_case()
    fwd, c, r1 = _certified(imgs[0], imgs[1], ratio)
    assert fwd.all() and c.all() and np.array_equal(r1, [1, 4, 7, 10])
    with diagnostic() as dl:
        got = run(imgs, pairs, ratio, totals=dl)
    assert_same(got, reference(imgs, pairs, ratio))
    assert np.array_equal(np.isin(np.arange(4), got[0]["queryIdx"]), accepted)
    if ratio == 1.5:    # the tie: the lower index wins
        assert got[0]["trainIdx"][-1] == 16 * 11 + 10 and got[0]["distance"][-1] == 1.0
    assert got[3] == (0, 0, 4, 0)


# --- winner and runner-up in different 256-row chunks of the subset ----------------------------------
def _chunk_case():
    T = synth.sift_images(1, 8193, seed=541, shared=0.0)[0].copy()
    Q = _queries(3, 542)
    # subset rows i = j // 16: chunk 0 is i < 256, chunk 1 is i < 512, the last holds the 513th row (j = 8192)
    for k, (j1, j2, s1, s2) in enumerate(((16 * 10 + 2, 16 * 300 + 2, 900, 1500),      # Lowe fails
                                          (16 * 400 + 9, 16 * 20 + 9, 500, 1500),       # passes, winner in chunk 1
                                          (8192, 16 * 100, 400, 1000))):                # winner is the last row
        T[j1] = _at(Q[k], s1, 0)
        T[j2] = _at(Q[k], s2, 4)
    return [Q, T], np.array([[0, 1]], np.int32)


def test_neighbours_in_different_chunks_of_the_subset():
    imgs, pairs = _chunk_case()
    fwd, c, r1 = _certified(imgs[0], imgs[1])
    assert fwd.all() and c.all() and np.array_equal(r1, [2, 9, 0])
    with diagnostic() as dl:
        got = run(imgs, pairs, totals=dl)
    assert_same(got, reference(imgs, pairs))
    assert np.array_equal(got[0]["queryIdx"], [1, 2]) and np.array_equal(got[0]["trainIdx"], [16 * 400 + 9, 8192])
    assert got[3] == (0, 0, 3, 0)


# --- a two-row subset whose second row lies in the float-sqrt collision range -------------------------
def _far_second_row_case():
    rng = np.random.default_rng(551)
    q = (4 * rng.integers(2, 14, 128)).astype(np.float32)        # u - 32 = 4 m exactly: no quantisation error
    T = np.zeros((30, 128), np.float32)
    for j in range(30):                                           # the other subsets: s about 1e6, far below 2^22
        T[j] = np.clip(q + rng.choice([-90, 90], 128), 0, 255)
    T[3] = _at(q, 100)
    T[19] = 255                                                   # subset 3 = rows 3, 19: s(q, row 19) >= 2^22
    return [q[None, :].copy(), T], np.array([[0, 1]], np.int32)


def test_second_row_of_the_subset_in_the_collision_range():
    imgs, pairs = _far_second_row_case()
    S = cert.exact_s(imgs[0], imgs[1])[0]
    assert S[19] >= cert.SQRT_SAFE and np.delete(S, 19).max() < cert.SQRT_SAFE
    fwd, c, r1 = _certified(imgs[0], imgs[1])
    assert fwd[0] and c[0] and r1[0] == 3
    with diagnostic() as dl:
        got = run(imgs, pairs, totals=dl)
    assert_same(got, reference(imgs, pairs))
    assert got[1][-1] == 1 and got[0]["trainIdx"][0] == 3
    assert got[3] == (0, 0, 1, 0)                 # stats()[0] == 0: no slow query
    assert run(imgs, pairs)[3] == (0, 0)          # the product library


# --- both kinds of slot in lists longer than the 1024-entry window; the filters; the parent's path --
def _mixed_case():
    rng = np.random.default_rng(561)
    base = synth.sift_images(3, 2600, seed=562, shared=0.0)
    R = base[0].copy()
    near = lambda rows: np.clip(rows + rng.integers(-6, 7, rows.shape), 0, 255).astype(np.float32)
    R[1:600:2] = near(R[0:600:2])                 # 300 near-duplicate train rows in neighbouring subsets
    one = near(R[600:2000])                       # one near neighbour: the subset route
    two = near(R[0:600:2])                        # two near neighbours in two subsets: forwarded, the full route
    dup = near(np.repeat(R[2000:2100], 3, axis=0))   # three queries per train row (distinct drops them)
    L = np.concatenate([one, two, dup, base[1][:300]])
    L = L[rng.permutation(len(L))]
    A = np.concatenate([near(R[2100:2130]), base[2][:400]])      # a pair with few matches (min_count clears it)
    return [L, R, np.ascontiguousarray(A)], np.array([[0, 1], [2, 1], [1, 0], [2, 0]], np.int32)


@pytest.fixture(scope="module")
def mixed():
    imgs, pairs = _mixed_case()
    refs = {(d, mc): reference(imgs, pairs, 0.7, d, mc) for d, mc in ((0, 0), (1, 0), (1, 100))}
    assert refs[(1, 0)][1][-1] < refs[(0, 0)][1][-1], "distinct = 1 drops no match"
    assert (refs[(1, 100)][2] == 0).any() and (refs[(1, 100)][2] == 1).any(), "min_count clears no pair"
    fwd, c, _ = _certified(imgs[0], imgs[1])
    assert (fwd & c).sum() > 1100 and (fwd & ~c).sum() > 250     # both kinds, more than one window
    return imgs, pairs, refs


@pytest.mark.parametrize("distinct,min_count", [(0, 0), (1, 0), (1, 100)])
def test_both_kinds_of_slot_past_the_window_with_filters(mixed, distinct, min_count):
    imgs, pairs, refs = mixed
    with diagnostic() as dl:
        got = run(imgs, pairs, 0.7, distinct, min_count, totals=dl)
    assert_same(got, refs[(distinct, min_count)])
    slow, f32, forwarded, full = got[3]
    assert (slow, f32) == (0, 0)
    assert forwarded > 4000 and 350 < full < 450     # (the restatement: 4131 forwarded, 400 of them uncertified)
    assert_same(run(imgs, pairs, 0.7, distinct, min_count), refs[(distinct, min_count)])   # the product library


# --- few full-route queries ride the subset kernel: either side of the threshold ----------------------
def _ride_case():
    rng = np.random.default_rng(571)
    base = synth.sift_images(2, 600, seed=572, shared=0.0)
    R = base[0].copy()
    near = lambda rows: np.clip(rows + rng.integers(-6, 7, rows.shape), 0, 255).astype(np.float32)
    R[1:80:2] = near(R[0:80:2])                                   # near-duplicate train rows in neighbouring subsets
    imgs = [R]
    for k in (32, 33):                                            # k queries with two near neighbours, 60 with one
        imgs.append(np.concatenate([near(R[200:230]), near(R[0:2 * k:2]), near(R[230:260])]))
    return imgs, np.array([[1, 0], [2, 0]], np.int32)


def test_either_side_of_the_ride_threshold():
    """At most 32 full-route queries of a pair ride the subset kernel (all 16 subsets, the atomic merge), 33 get
    a full-row item."""
    imgs, pairs = _ride_case()
    for k, n in ((1, 32), (2, 33)):
        fwd, c, _ = _certified(imgs[k], imgs[0])
        assert fwd.all() and (~c).sum() == n and c.sum() == 60
    with diagnostic() as dl:
        got = run(imgs, pairs, totals=dl)
    assert_same(got, reference(imgs, pairs))
    assert got[3] == (0, 0, 92 + 93, 65)
    assert_same(run(imgs, pairs), reference(imgs, pairs))         # the product library


def test_full_row_variant_gives_the_same_arrays(mixed):
    """SFMX_SIFT_VARIANT=111 (diagnostic library): the FP6 screen with the full-row pass 2 for every forwarded query."""
    imgs, pairs, refs = mixed
    rimgs, rpairs, _ = _residue_case()
    with diagnostic(SFMX_SIFT_VARIANT="111") as dl:
        got = run(imgs, pairs, 0.7, 1, 100, totals=dl)
        got_r = run(rimgs, rpairs, totals=dl)
    assert_same(got, refs[(1, 100)])
    assert_same(got_r, reference(rimgs, rpairs))
    assert got[3][3] == 0 and got_r[3] == (0, 0, 16, 0)      # (the second counters are not used on that path)


def test_uniform_data_takes_only_the_full_route():
    imgs = synth.sift_images(2, 1024, uniform=True)
    pairs = np.array([[0, 1], [1, 0]], np.int32)
    with diagnostic() as dl:
        got = run(imgs, pairs, 1.5, totals=dl)
    assert_same(got, reference(imgs, pairs, 1.5))
    assert got[3][2] == 2048 and got[3][3] == 2048
