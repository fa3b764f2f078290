"""The key fold of the row-form pass 2 (sift_rows_kernel, csrc/match_kernels.hip), restated in numpy and checked
against brute force; no GPU.  For a query and the row subset r (train rows j = r + 16 i) the kernel

  * forms, per 32-row tile, the packed keys (dot << 9) + (-nb << 8) + 255 - (i & 255) (INT_MIN for pad rows and rows
    past the image), dot and nb over the int8 rows u - 128,
  * keeps the two largest per lane half in accumulator order, two keys per step (b2 takes the medians, b1 the maxima),
    over the eight tiles of a 256-row chunk, and combines the halves at the chunk's end,
  * folds the chunk's two keys into the running (T, J) pairs with strict <, so an equal distance in a later chunk
    never displaces an earlier one,
  * writes k = ((na + T) << 32) | (r + 16 J).

The two keys must be the two smallest (squared distance, train index) pairs of the subset, in that order: the
order sift_subset_kernel produces and sift_finish_kernel expects.  The planted cases are those of
tests/test_gpu_match_rows.py: every residue, a runner-up either side of Lowe's test, identical rows, equal distances
inside a chunk and across two, the winner and the runner-up in different chunks in both orders, and a 513th row."""
import numpy as np
import pytest

import sift_rows_cases as cases

INT_MIN = -(1 << 31)
NONE = (1 << 64) - 1


def _med3(a, b, c):
    return max(min(a, b), min(max(a, b), c))


def fold_top2(q, T, r):
    """The kernel's (k1, k2) of query row q (128 values 0..255) over subset r of the train image T."""
    nt = len(T)
    rows_pad = -(-nt // 512) * 512
    aq = q.astype(np.int64) - 128
    na = int((aq * aq).sum())
    A = np.zeros((rows_pad, 128), np.int64)                   # pad rows are zero bytes
    A[:nt] = T.astype(np.int64) - 128
    T1 = T2 = None
    J1 = J2 = -1
    ntile = rows_pad // 512
    c1, c2 = [INT_MIN, INT_MIN], [INT_MIN, INT_MIN]           # per lane half
    for t in range(ntile):
        i = 32 * t + np.arange(32)
        rows = A[r + 16 * i]
        dot = rows @ aq
        nb = (rows * rows).sum(1)
        key = (dot << 9) - (nb << 8) + 255 - (i & 255)
        assert key.min() > INT_MIN and key.max() < (1 << 31)
        key = np.where(r + 16 * i < nt, key, INT_MIN)
        for h in range(2):                                    # accumulator element 4 g + u of half h: tile row 8 g + 4 h + u
            acc = [int(key[8 * g + 4 * h + u]) for g in range(4) for u in range(4)]
            for e in range(0, 16, 2):
                m = _med3(c1[h], acc[e], acc[e + 1])
                c1[h] = max(c1[h], acc[e], acc[e + 1])
                c2[h] = max(c2[h], m)
        if t % 8 == 7 or t + 1 == ntile:                      # end of a 256-row chunk
            cb = (t // 8) * 256
            m1 = max(c1)
            m2 = max(min(c1), max(c2))
            for k in (m1, m2):
                if k != INT_MIN:
                    t_, i_ = -(k >> 8), cb + 255 - (k & 255)
                    if T2 is None or t_ < T2:
                        if T1 is None or t_ < T1:
                            T2, J2, T1, J1 = T1, J1, t_, i_
                        else:
                            T2, J2 = t_, i_
            c1, c2 = [INT_MIN, INT_MIN], [INT_MIN, INT_MIN]
    k1 = ((na + T1) << 32) | (r + 16 * J1) if T1 is not None else NONE
    k2 = ((na + T2) << 32) | (r + 16 * J2) if T2 is not None else NONE
    return k1, k2


def brute_top2(q, T, r):
    j = np.arange(r, len(T), 16)
    d = T[j].astype(np.int64) - q.astype(np.int64)
    s = (d * d).sum(1)
    keys = sorted((int(a) << 32) | int(b) for a, b in zip(s, j))
    return tuple(keys[:2] + [NONE] * (2 - len(keys[:2])))


def _planted():
    out = []
    imgs, _, rows = cases.residue_case()
    out += [("residue", imgs, k, j % 16, j, j + 16) for k, j in enumerate(rows)]
    imgs, _, rows = cases.runner_up_case()
    out += [("runner-up", imgs, k, j % 16, j, j + 16) for k, j in enumerate(rows)]
    imgs, _, plan = cases.chunk_case()
    for k, (j1, j2, s1, s2) in enumerate(plan):
        first, second = (j1, j2) if (s1, j1) < (s2, j2) else (j2, j1)
        out.append(("chunk", imgs, k, j1 % 16, first, second))
    return out


PLANTED = _planted()


@pytest.mark.parametrize("case", PLANTED, ids=[f"{c[0]}-{c[2]}" for c in PLANTED])
def test_planted_top2_in_distance_index_order(case):
    _, imgs, k, r, first, second = case
    Q, T = imgs
    got = fold_top2(Q[k], T, r)
    assert got == brute_top2(Q[k], T, r)
    assert (got[0] & 0xFFFFFFFF, got[1] & 0xFFFFFFFF) == (first, second)      # the planted rows, the lower index first on a tie
    assert got[0] <= got[1]


def test_every_subset_of_the_chunk_case_and_short_images():
    """Unplanted subsets (random rows) of the 513-row subsets, and images whose subsets have 0, 1 or 2 rows."""
    Q, T = cases.chunk_case()[0]
    for r in range(16):
        assert fold_top2(Q[0], T, r) == brute_top2(Q[0], T, r)
    for nt in (1, 16, 17, 32, 33, 48, 511, 512, 513):
        for r in (0, 1, 15):
            got = fold_top2(Q[1], T[:nt], r)
            assert got == brute_top2(Q[1], T[:nt], r)
            assert (got[0] == NONE) == (r >= nt) and (got[1] == NONE) == (r + 16 >= nt)
