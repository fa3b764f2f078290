"""numpy restatement of the conservative FP6 (e2m3) SIFT screen (csrc/sift_fp6.hpp), written from the
format's definition rather than from the header's arithmetic.

e2m3: 1 sign, 2 exponent (bias 1), 3 mantissa bits, subnormals, no infinities.  In units of 1/8 the
magnitudes are 0..15, 16..30 step 2, 32..60 step 4.  A descriptor value u is written
u - OFFSET = SCALE * m + e with m the nearest of those (ties away from zero)."""
import numpy as np

from sfmx import synth

OFFSET, SCALE = 32, 4
SLACK = 1025.0
PAD_KEY = np.float32(-1.0e30)


def decode(code: int) -> int:
    """Value of a 6-bit e2m3 code in units of 1/8."""
    man, ex, sign = code & 7, (code >> 3) & 3, code >> 5
    mag = man if ex == 0 else (8 + man) * 2 ** (ex - 1)
    return -mag if sign else mag


MAGS = np.array(sorted({abs(decode(c)) for c in range(64)}))
CODE_OF = {decode(c): c for c in range(63, -1, -1) if not (c == 0x20)}   # (-0 is never produced)


def quantise(u):
    """u (integers 0..255, any shape) -> (m, e): nearest representable magnitude, ties away from zero."""
    a = np.asarray(u, np.int64) - OFFSET
    dist = np.abs(np.abs(a)[..., None] - SCALE * MAGS)            # to every magnitude
    pick = dist.shape[-1] - 1 - np.argmin(dist[..., ::-1], axis=-1)   # the last (largest) of the nearest
    m = np.sign(a) * MAGS[pick]
    return m, a - SCALE * m


def pack_rows(m):
    """m (n x 128) -> n x 24 uint32: lane group g takes elements 32 g .. 32 g + 31 as 192 bits, element i at
    bits [6 i, 6 i + 6); a group's words 0..3 go to word 4 g of the row, words 4, 5 to word 16 + 2 g."""
    m = np.asarray(m)
    codes = np.vectorize(CODE_OF.__getitem__)(m).astype(np.uint64)
    out = np.zeros((len(m), 24), np.uint32)
    for g in range(4):
        bits = np.zeros((len(m), 192), np.uint8)
        for i in range(32):
            for b in range(6):
                bits[:, 6 * i + b] = (codes[:, 32 * g + i] >> np.uint64(b)) & np.uint64(1)
        words = (bits.reshape(len(m), 6, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
        out[:, 4 * g:4 * g + 4] = words[:, :4]
        out[:, 16 + 2 * g:18 + 2 * g] = words[:, 4:]
    return out


def sqrt_rn(s):
    return np.sqrt(np.asarray(s, np.float64)).astype(np.float32)


def top2_of_subsets(keys):
    """keys (nq x nt) -> the two largest of the 16 row-subset maxima (subset = train row mod 16); -inf where
    fewer subsets have a row."""
    nq, nt = keys.shape
    sub = np.full((nq, 16), -np.inf)
    for r in range(min(16, nt)):
        sub[:, r] = keys[:, r::16].max(axis=1)
    sub.sort(axis=1)
    return sub[:, -1], sub[:, -2]


def exact_forward(q, t, ratio):
    """The exact int8 screen (sift_screen16_kernel): forwarded unless Lowe's test fails at
    (na - 2 K1 - 1, na - 2 K2), K = dot - ceil(nb / 2) on u - 128."""
    a, b = q.astype(np.int64) - 128, t.astype(np.int64) - 128
    na, nb = (a * a).sum(1), (b * b).sum(1)
    K = a @ b.T - (nb + 1) // 2
    k1, k2 = top2_of_subsets(K.astype(np.float64))
    usable = (len(t) >= 2) & np.isfinite(k2)
    k1f, k2f = np.where(usable, k1, 0), np.where(usable, k2, 0)
    s1, s2 = np.maximum(na - 2 * k1f - 1, 0), na - 2 * k2f
    rej = usable & ~(sqrt_rn(s1).astype(np.float64) < sqrt_rn(s2).astype(np.float64) * ratio)
    return ~rej


def certainly_rejected(k1, k2, na, e2q, emax2, amax2, ratio):
    """The header's decision, operation by operation in float64 (k1, k2: float32 accumulators)."""
    E = np.sqrt(np.float64(na) * np.float64(emax2)) + \
        np.sqrt(np.float64(e2q)) * (np.sqrt(np.float64(amax2)) + np.sqrt(np.float64(emax2)))
    M = E + SLACK
    lo = np.float64(na) - 2.0 * (np.float64(k1) * 1024.0 + M)
    hi = np.float64(na) - 2.0 * (np.float64(k2) * 1024.0 - M)
    lo = np.minimum(np.maximum(lo, 0.0), 1.0e12)
    hi = np.minimum(np.maximum(hi, 0.0), 1.0e12)
    s1, s2 = np.floor(lo), np.ceil(hi)
    return ~(sqrt_rn(s1).astype(np.float64) < sqrt_rn(s2).astype(np.float64) * ratio)


def conservative(q, t, ratio):
    """-> dict: forwarded mask, the keys' exact and quantised values and the bound E per query."""
    mq, eq = quantise(q)
    mt, et = quantise(t)
    aq, at = q.astype(np.int64) - OFFSET, t.astype(np.int64) - OFFSET
    na, nb = (aq * aq).sum(1), (at * at).sum(1)
    e2q = (eq * eq).sum(1)
    emax2 = int((et * et).sum(1).max()) if len(t) else 0
    amax2 = int(nb.max()) if len(t) else 0
    kappa = aq @ at.T - nb / 2.0                                   # exact (halves)
    acc = ((mq @ mt.T) / 64.0 - nb / 2048.0).astype(np.float32)    # one rounding of the exact value
    E = np.sqrt(na.astype(np.float64) * emax2) + np.sqrt(e2q.astype(np.float64)) * (np.sqrt(float(amax2)) + np.sqrt(float(emax2)))
    k1, k2 = top2_of_subsets(acc.astype(np.float64))
    usable = (len(t) >= 2) & np.isfinite(k2)
    k1f = np.where(usable, k1, 0).astype(np.float32)
    k2f = np.where(usable, k2, 0).astype(np.float32)
    rej = usable & certainly_rejected(k1f, k2f, na, e2q, emax2, amax2, ratio)
    return {"forward": ~rej, "kappa": kappa, "kappa_q": acc.astype(np.float64) * 1024.0, "E": E, "na": na, "e2q": e2q,
            "emax2": emax2, "amax2": amax2, "k1": k1f, "k2": k2f, "usable": usable}


# --- inputs shared by the CPU and the GPU tests ---
def extreme_rows():
    """All 0, all 255, half and half, and 0 / 255 alternating."""
    r = np.zeros((6, 128), np.float32)
    r[1] = 255
    r[2, :64] = 255
    r[3, ::2] = 255
    r[4] = 254
    r[5] = 1
    return r


def midpoint_rows():
    """Every value whose u - 32 lies halfway between two representable values (times SCALE), and its neighbours."""
    mids = []
    for lo, hi in zip(MAGS[:-1], MAGS[1:]):
        if (SCALE * (lo + hi)) % 2 == 0:
            for sign in (1, -1):
                u = OFFSET + sign * SCALE * (lo + hi) // 2
                mids += [v for v in (u - 1, u, u + 1) if 0 <= v <= 255]
    mids = np.array(sorted(set(mids)), np.float32)
    assert len(mids) > 40
    rng = np.random.default_rng(5)
    rows = np.stack([rng.choice(mids, 128) for _ in range(62)] + [np.resize(mids, 128), np.resize(mids[::-1], 128)])
    return rows.astype(np.float32)


def cases():
    s = synth.sift_images(2, 1024)
    u = synth.sift_images(2, 1024, uniform=True)
    ext, mid = extreme_rows(), midpoint_rows()
    rng = np.random.default_rng(11)
    near = np.clip(np.concatenate([ext, mid])[:, None, :] + rng.integers(-2, 3, (1, 3, 128)), 0, 255).reshape(-1, 128)
    return {
        "synth": (s[0], s[1]),
        "uniform": (u[0], u[1]),
        "extreme": (np.concatenate([ext, near]).astype(np.float32), np.concatenate([near, ext, s[0][:64]]).astype(np.float32)),
        "midpoints": (mid, np.concatenate([mid[::-1], near]).astype(np.float32)),
    }
