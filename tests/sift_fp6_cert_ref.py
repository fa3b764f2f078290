"""numpy restatement of the one-subset certificate of the FP6 SIFT screen (csrc/sift_fp6.hpp, fp6::certified),
written from its definition.

With M = E + SLACK and K1 > K2 the two largest of the 16 row-subset maxima of the quantised key (units of
1 / 1024 in the float32 accumulator), r1 the subset (train row mod 16) of K1:
    s1hi = ceil(max(na - 2 (1024 K1 - M), 0))   every row of r1's maximum has s <= s1hi
    lo   = floor(max(na - 2 (1024 K2 + M), 0))  every row outside r1 has s >= lo
    hi   = ceil(max(na - 2 (1024 K2 - M), 0))   some row outside r1 has s <= hi
A forwarded query is certified for r1 iff the bound is usable, s1hi < lo, Lowe's test passes at (s1hi, lo),
hi < 2^22 and r1 + 16 < nt."""
import numpy as np

import sift_fp6_ref as ref

SQRT_SAFE = 1 << 22


def subset_maxima(q, t):
    """-> (k1, k2, r1, usable): float32 accumulator values of the two largest subset maxima, the subset of the
    largest, and whether two subsets hold a row."""
    mq, _ = ref.quantise(q)
    mt, _ = ref.quantise(t)
    at = t.astype(np.int64) - ref.OFFSET
    nb = (at * at).sum(1)
    acc = ((mq @ mt.T) / 64.0 - nb / 2048.0).astype(np.float32).astype(np.float64)
    sub = np.full((len(q), 16), -np.inf)
    for r in range(min(16, len(t))):
        sub[:, r] = acc[:, r::16].max(axis=1)
    r1 = sub.argmax(axis=1)
    srt = np.sort(sub, axis=1)
    k1, k2 = srt[:, -1], srt[:, -2]
    usable = (len(t) >= 2) & np.isfinite(k2)
    return (np.where(usable, k1, 0).astype(np.float32), np.where(usable, k2, 0).astype(np.float32), r1.astype(np.int32),
            usable)


def bounds(k1, k2, na, e2q, emax2, amax2):
    f64 = lambda x: np.asarray(x, np.float64)
    na, k1, k2 = f64(na), f64(k1), f64(k2)
    E = np.sqrt(na * f64(emax2)) + np.sqrt(f64(e2q)) * (np.sqrt(f64(amax2)) + np.sqrt(f64(emax2)))
    M = E + ref.SLACK
    clamp = lambda x: np.minimum(np.maximum(x, 0.0), 1.0e12)
    s1hi = np.ceil(clamp(na - 2.0 * (k1 * 1024.0 - M))).astype(np.int64)
    lo = np.floor(clamp(na - 2.0 * (k2 * 1024.0 + M))).astype(np.int64)
    hi = np.ceil(clamp(na - 2.0 * (k2 * 1024.0 - M))).astype(np.int64)
    return s1hi, lo, hi


def lowe(s1, s2, ratio):
    return ref.sqrt_rn(s1).astype(np.float64) < ref.sqrt_rn(s2).astype(np.float64) * ratio


def certified(k1, k2, r1, usable, nt, na, e2q, emax2, amax2, ratio):
    s1hi, lo, hi = bounds(k1, k2, na, e2q, emax2, amax2)
    return usable & (s1hi < lo) & lowe(s1hi, lo, ratio) & (hi < SQRT_SAFE) & (r1 + 16 < nt)


def screen(q, t, ratio):
    """-> dict: per query forwarded, certified (a subset of forwarded), r1 and the certificate's inputs."""
    c = ref.conservative(q, t, ratio)
    k1, k2, r1, usable = subset_maxima(q, t)
    assert np.array_equal(k1, c["k1"]) and np.array_equal(k2, c["k2"]) and np.array_equal(usable, c["usable"])
    cert = certified(k1, k2, r1, usable, len(t), c["na"], c["e2q"], c["emax2"], c["amax2"], ratio) & c["forward"]
    return {"forward": c["forward"], "certified": cert, "r1": r1, "k1": k1, "k2": k2, "usable": usable, "na": c["na"],
            "e2q": c["e2q"], "emax2": c["emax2"], "amax2": c["amax2"]}


def exact_s(q, t):
    """Exact squared distances (nq x nt, int64)."""
    a, b = q.astype(np.int64), t.astype(np.int64)
    return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)
