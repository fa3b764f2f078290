"""GPU parity of the SIFT pass 2 (sift_subset_kernel: staging at entry, keys from the norms loaded
with the rows, two-slot merge of two-subset queries, three-atomic merge of the rest), the
one-read assembly count, the ballot rank of the write pass and the single per-run fill, byte for
byte against the oracle.

Every case compares pair offsets and packed matches with oracle.match_pairs and asserts that no
query took the slow path or the fp32 path (stats() == (0, 0))."""
import functools

import numpy as np
import pytest

import sfmx
from sfmx import synth

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def base_images():
    """Six 8193-row SIFT-like images; every case slices them (never modified)."""
    imgs = synth.sift_images(6, 8193, seed=20611)
    for im in imgs:
        im.setflags(write=False)
    return imgs


def assert_same(got, off, exp, exp_off):
    assert np.array_equal(off, exp_off), (off, exp_off)
    if got.tobytes() != exp.tobytes():
        bad = np.nonzero(got != exp)[0][:5] if len(got) == len(exp) else []
        raise AssertionError(f"mismatch at {bad}: got {got[bad] if len(bad) else got[:5]} exp {exp[bad] if len(bad) else exp[:5]}")


def gpu_run(m, pairs, ratio):
    m.run(pairs, ratio)
    got, off, _ = m.fetch()
    assert m.stats() == (0, 0)
    return got, off


def check_against_oracle(imgs, pairs, ratio):
    from oracle import oracle
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    m = sfmx.BFMatcher(sfmx.NORM_L2)
    try:
        m.set_images(imgs)
        got, off = gpu_run(m, pairs, ratio)
    finally:
        m.close()
    exp, eoff = oracle.match_pairs(imgs, pairs, ratio)
    assert_same(got, off, exp, eoff)
    return got, off


def test_short_train_images():
    """Train images of 0, 1, 2, 15, 16, 17 and 33 rows: subsets with r >= nt, one-row subsets and
    fewer than two valid subsets, under a 40-row and a 600-row query image."""
    b = base_images()
    sizes = [0, 1, 2, 15, 16, 17, 33]
    imgs = [b[0][:40], b[1][:600]] + [b[2][100:100 + n] for n in sizes]
    pairs = [(q, 2 + t) for t in range(len(sizes)) for q in (0, 1)]
    check_against_oracle(imgs, pairs, 0.7)


CHUNK_SIZES = [4096, 4097, 8192, 8193]   # 1, 2, 2 and 3 chunks of 256 subset rows


def chunk_case():
    b = base_images()
    imgs = [b[0][:1300]] + [b[1 + i][:n] for i, n in enumerate(CHUNK_SIZES)]
    pairs = np.array([(0, 1 + i) for i in range(len(CHUNK_SIZES))], np.int32)
    return imgs, pairs


@pytest.mark.parametrize("ratio", [0.0, 0.7, 1.0, 1.5])
def test_chunk_boundaries(ratio):
    """Ratio 1.5 forwards every query (lists longer than the 1024-entry window, subsets with more
    than 128 queries); ratio 0.0 forwards none (every workgroup sees cnt == 0)."""
    imgs, pairs = chunk_case()
    check_against_oracle(imgs, pairs, ratio)


def test_ties_lower_index_wins():
    """Row j copied to j + 1 (another subset), j + 16 (same subset, same chunk), j + 4096 and
    j + 8192 (same subset, later chunks).  Exact-copy queries tie at distance 0 (rejected by the
    ratio test, as in the oracle); the same rows moved by 1 in one component tie at distance 1 and
    are accepted at ratio 1.5, where the reported neighbour must be the lowest tied index."""
    b = base_images()
    t = b[3].copy()
    t[101] = t[100]
    t[216] = t[200]
    t[4096] = t[0]
    t[8192] = t[0]
    t[300 + 4096] = t[300]
    src = [100, 200, 0, 300]
    near = t[src].copy()
    for row in near:
        row[5] += 1.0 if row[5] < 255.0 else -1.0
    q = np.ascontiguousarray(np.concatenate([t[src], near]))
    for ratio in (0.7, 1.5):
        got, off = check_against_oracle([q, t], [(0, 1)], ratio)
        if ratio == 1.5:
            by_query = {int(g["queryIdx"]): int(g["trainIdx"]) for g in got}
            for i, j in enumerate(src):
                assert by_query.get(len(src) + i) == j, (i, j, by_query)


def test_grouping_across_train_images():
    """Six images, one empty.  Image 5 is the train image of pairs whose left images have 1, 33,
    511 and 1300 rows and of an empty-left pair; sorted by train image the list puts changes of
    train image inside any group of 2 to 8 consecutive pairs (pass 2 takes one pair per workgroup;
    a grouped form must get this right).  The reversed list gives the same matches."""
    from oracle import oracle
    b = base_images()
    imgs = [b[0][:1], b[1][:33], b[2][:511], b[3][:1300], b[4][:0], b[5][:2100]]
    pairs = np.array([(0, 2), (1, 2), (0, 5), (1, 5), (2, 5), (3, 5), (4, 5), (0, 3), (1, 3), (2, 3), (3, 4),
                      (5, 3), (3, 2)], np.int32)
    rev = np.ascontiguousarray(pairs[::-1])
    m = sfmx.BFMatcher(sfmx.NORM_L2)
    try:
        m.set_images(imgs)
        got, off = gpu_run(m, pairs, 0.7)
        rgot, roff = gpu_run(m, rev, 0.7)
    finally:
        m.close()
    exp, eoff = oracle.match_pairs(imgs, pairs, 0.7)
    assert_same(got, off, exp, eoff)
    rexp, reoff = oracle.match_pairs(imgs, rev, 0.7)
    assert_same(rgot, roff, rexp, reoff)
    n = len(pairs)
    for p in range(n):
        a = got[off[p]:off[p + 1]]
        c = rgot[roff[n - 1 - p]:roff[n - p]]
        assert a.tobytes() == c.tobytes(), p


def test_determinism_across_runs_and_set_images():
    """Two runs on one matcher without a new set_images, then one after it: byte-equal (counters
    of the per-run arena that were not zeroed again would show here)."""
    from oracle import oracle
    imgs, pairs = chunk_case()
    outs = []
    m = sfmx.BFMatcher(sfmx.NORM_L2)
    try:
        m.set_images(imgs)
        outs.append(gpu_run(m, pairs, 0.7))
        outs.append(gpu_run(m, pairs, 0.7))
        m.set_images(imgs)
        outs.append(gpu_run(m, pairs, 0.7))
    finally:
        m.close()
    exp, eoff = oracle.match_pairs(imgs, pairs, 0.7)
    for got, off in outs:
        assert_same(got, off, exp, eoff)
