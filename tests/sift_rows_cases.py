"""Planted inputs for the tests of the row-form pass 2 (sift_rows_kernel, csrc/match_kernels.hip): one wave per
(pair, row subset r = j mod 16), the subset's rows streamed in 32-row tiles, keys packed per 256-row chunk,
later chunks folded with strict <.  Shared by tests/test_gpu_match_rows.py (the GPU against the oracle) and
tests/test_sift_rows_keys.py (a numpy restatement of the key fold against brute force); test infrastructure."""
import math

import numpy as np

from sfmx import synth


def four_squares(s):
    for a in range(math.isqrt(s), -1, -1):
        r1 = s - a * a
        for b in range(math.isqrt(r1), -1, -1):
            r2 = r1 - b * b
            for c in range(math.isqrt(r2), -1, -1):
                d = math.isqrt(r2 - c * c)
                if d * d == r2 - c * c:
                    return a, b, c, d
    raise AssertionError(s)


def at(q, s, where=0):
    """A copy of q at squared distance s: four squares added to elements where .. where + 3 (q is small there)."""
    t = q.copy()
    t[where:where + 4] += four_squares(s)
    assert t.max() <= 255
    return t


def queries(n, seed):
    """n SIFT-like rows, far from each other and from every other image, elements 0..15 small."""
    q = synth.sift_images(1, n, seed=seed, shared=0.0)[0].copy()
    q[:, :16] = np.minimum(q[:, :16], 20)
    return q


def near(rng, rows, amp=6):
    return np.clip(rows + rng.integers(-amp, amp + 1, rows.shape), 0, 255).astype(np.float32)


def residue_case():
    """An isolated neighbour in each residue r = 0..15 (every wave of every group writes), a runner-up 16 rows on."""
    T = synth.sift_images(1, 600, seed=7111, shared=0.0)[0].copy()
    Q = queries(16, 7112)
    rows = [16 * (3 + 2 * r) + r for r in range(16)]
    for r, j in enumerate(rows):
        T[j] = at(Q[r], 900 + r)
        T[j + 16] = at(Q[r], 4000 + r, 4)
    return [Q, T], np.array([[0, 1]], np.int32), rows


def runner_up_case():
    """(s1, s2) in one subset: Lowe at 0.7 fails, passes, two identical rows (the index decides), a tie at distance 1."""
    T = synth.sift_images(1, 300, seed=7121, shared=0.0)[0].copy()
    Q = queries(4, 7122)
    rows = []
    for k, (s1, s2) in enumerate(((4000, 5000), (1000, 5000), (0, 0), (1, 1))):
        j = 16 * (2 + 3 * k) + (3 * k + 1)
        T[j] = at(Q[k], s1, 0)
        T[j + 16] = at(Q[k], s2, 4)
        rows.append(j)
    return [Q, T], np.array([[0, 1]], np.int32), rows


def chunk_case():
    """Winner and runner-up in different 256-row chunks of the subset (subset row i = j // 16, chunk i // 256), in both
    orders; equal distances in two chunks, where the strict < of the later chunk keeps the lower index; a winner
    in the last row of a 513-row subset; a winner at local index 255 and a runner-up at local index 0 of the next chunk."""
    T = synth.sift_images(1, 8193, seed=7131, shared=0.0)[0].copy()
    Q = queries(6, 7132)
    plan = ((16 * 10 + 2, 16 * 300 + 2, 900, 1500),        # winner in chunk 0, runner-up in chunk 1: Lowe at 0.7 fails
            (16 * 400 + 9, 16 * 20 + 9, 500, 1500),        # winner in chunk 1, runner-up in chunk 0: passes
            (16 * 30 + 4, 16 * 290 + 4, 700, 700),         # equal distances in chunks 0 and 1
            (16 * 500 + 7, 16 * 270 + 7, 800, 800),        # equal distances, both in chunk 1, planted in descending order
            (8192, 16 * 100, 400, 1000),                   # the winner is the subset's 513th row
            (16 * 255 + 12, 16 * 256 + 12, 600, 650))      # either side of the chunk boundary
    for k, (j1, j2, s1, s2) in enumerate(plan):
        T[j1] = at(Q[k], s1, 0)
        T[j2] = at(Q[k], s2, 4)
    return [Q, T], np.array([[0, 1]], np.int32), plan
