"""GPU: the unscaled f8f6f4 MFMA (v_mfma_f32_*_f8f6f4, what fp6::mfma16 / mfma32 issue with SCALED = false) against
the block-scaled one with unit E8M0 scales, through the diagnostic library's sfmx_diag_mfma_forms: one wave per
case runs both forms on the same operand fragments and C values, and the raw bits of D must be equal.

256 cases per format (e2m3 of the SIFT screens, e2m1 of the ORB kernels), each as one 16 x 16 x 128 MFMA and as the
chained 32 x 32 x 64 pair of the wide screen: rows that hold every code of the format, rows quantised from
synth.sift_images (e2m3) or +-1 rows (e2m1), and all-extreme rows; the C operand of a train row is 0, a SIFT key
-|a|^2 / 2048, fp6::PAD_KEY or the ORB key 767 + i / 16384, in turn.

Beyond the equality of the two forms: for e2m3, 1024 D lies within the header's accumulation bound (258 key units,
260 for the chained pair) of the exact integer kappa~ = 16 <m_a, m_b> + 1024 C; for e2m1 +-1 operands D is the
integer sum exactly (C = 0 or the ORB key, where every partial sum is a float).
Fails without the feature: the diagnostic library has no such export."""
import ctypes as C

import numpy as np
import pytest

import sift_fp6_ref as ref
from sfmx import synth
from diag import diag_lib

pytestmark = pytest.mark.gpu

N = 256
PAD_KEY = np.float32(-1.0e30)
E2M3, E2M1 = 2, 4
BITS = {E2M3: 6, E2M1: 4}
DECODE3 = np.array([ref.decode(c) for c in range(64)], np.int64)                        # units of 1 / 8
DECODE1 = np.array([s * v for s in (1, -1) for v in (0, 1, 2, 3, 4, 6, 8, 12)], np.int64)  # units of 1 / 2
C_ZERO, C_KEYF, C_PAD, C_ORB = 0, 1, 2, 3


def _pack(codes, nbits):
    """codes (..., 32) -> (..., 8) uint32: element i at bits [nbits i, nbits i + nbits), the rest zero."""
    bits = ((codes[..., None] >> np.arange(nbits)) & 1).astype(np.uint8).reshape(*codes.shape[:-1], 32 * nbits)
    words = np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little")).view("<u4")
    out = np.zeros((*codes.shape[:-1], 8), np.uint32)
    out[..., :nbits] = words
    return out


def _cases(fmt):
    """-> codes of the A rows and of the B rows (N x 32 x 128), the C value of every A row (N x 32), the C kind per
    case and the mask of the cases whose operands are all +-1 (e2m1)."""
    rng = np.random.default_rng(900 + fmt)
    ncode = 1 << BITS[fmt]
    rows = np.zeros((2, N, 32, 128), np.int64)
    # 0..63: every code in every row
    every = np.tile(np.arange(ncode), 128 // ncode)
    rows[:, :64] = rng.permuted(np.broadcast_to(every, (2, 64, 32, 128)), axis=-1)
    sift = synth.sift_images(1, 2048, seed=901, shared=0.0)[0]
    m, _ = ref.quantise(sift)
    a2 = ((sift.astype(np.int64) - ref.OFFSET) ** 2).sum(1)
    if fmt == E2M3:   # 64..191: rows of the quantiser
        codes = np.vectorize(ref.CODE_OF.__getitem__)(m)
        rows[:, 64:192] = codes[rng.integers(0, len(codes), (2, 128, 32))]
        lo, hi = 0x1F, 0x3F            # +-7.5
    else:             # 64..191: +-1 (codes 2 and 10), the ORB operands
        rows[:, 64:192] = np.where(rng.integers(0, 2, (2, 128, 32, 128)) == 1, 2, 10)
        lo, hi = 0x7, 0xF              # +-6
    # 192..255: all-extreme rows: one sign, the other, alternating, random signs
    ext = np.where(rng.integers(0, 2, (2, 64, 32, 128)) == 1, lo, hi)
    ext[:, 0:16] = lo
    ext[1, 8:16] = hi
    ext[:, 16:24] = hi
    ext[0, 24:32, :, ::2] = lo
    ext[0, 24:32, :, 1::2] = hi
    rows[:, 192:] = ext
    kind = np.arange(N) % 4
    crow = np.zeros((N, 32), np.float32)
    keyf = (-a2.astype(np.float32) / np.float32(2048.0)).astype(np.float32)
    crow[kind == C_KEYF] = keyf[rng.integers(0, len(keyf), ((kind == C_KEYF).sum(), 32))]
    crow[kind == C_PAD] = PAD_KEY
    orb = (767.0 + rng.integers(0, 16384, ((kind == C_ORB).sum(), 32)) / 16384.0).astype(np.float32)
    crow[kind == C_ORB] = orb
    pm1 = np.zeros(N, bool)
    pm1[64:192] = fmt == E2M1
    return rows[0], rows[1], crow, kind, pm1


def _operands16(ra, rb, crow, nbits):
    """Lane l of a case: A row / B column l & 15, elements 32 g .. 32 g + 31 with g = l >> 4; C and D register i:
    row 4 g + i of column l & 15."""
    def frag(r):
        p = _pack(r[:, :16].reshape(N, 16, 4, 32), nbits)                   # [case, row, g]
        return np.ascontiguousarray(p.transpose(0, 2, 1, 3).reshape(N, 64, 8))
    c = np.broadcast_to(crow[:, :16].reshape(N, 4, 1, 4), (N, 4, 16, 4))
    return frag(ra), frag(rb), np.ascontiguousarray(c.reshape(N, 64, 4), np.float32)


def _matrix16(d):
    return d.reshape(N, 4, 16, 4).transpose(0, 1, 3, 2).reshape(N, 16, 16)   # [case, row, column]


def _operands32(ra, rb, crow, nbits):
    """Lane l: row / column l & 31, K-half h = l >> 5; MFMA m takes fragment 2 m + h (fp6::frag32); register i is
    row (i & 3) + 8 (i >> 2) + 4 h (fp6::acc_row32)."""
    def frag(r):
        p = _pack(r.reshape(N, 32, 4, 32), nbits)                           # [case, row, f]
        return np.ascontiguousarray(p.transpose(0, 2, 1, 3).reshape(N, 2, 64, 8))   # f = 2 m + h -> [m][h * 32 + row]
    c = crow.reshape(N, 4, 2, 4).transpose(0, 2, 1, 3)[:, :, None]          # [case, h, 1, i >> 2, i & 3]
    c = np.broadcast_to(c, (N, 2, 32, 4, 4))
    return frag(ra), frag(rb), np.ascontiguousarray(c.reshape(N, 64, 16), np.float32)


def _matrix32(d):
    # [case, h, column, k, j] -> row 8 k + 4 h + j
    return d.reshape(N, 2, 32, 4, 4).transpose(0, 3, 1, 4, 2).reshape(N, 32, 32)


def _run(shape, fmt, a, b, c):
    fn = diag_lib().sfmx_diag_mfma_forms
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 4 + [C.c_void_p] * 5
    ds, du = np.full_like(c, np.nan), np.full_like(c, np.nan)
    assert fn(0, shape, fmt, N, *(x.ctypes.data for x in (a, b, c, ds, du))) == 0
    return ds, du


@pytest.fixture(scope="module", params=[E2M3, E2M1], ids=["e2m3", "e2m1"])
def cases(request):
    return (request.param,) + _cases(request.param)


@pytest.mark.parametrize("shape", [16, 32])
def test_unscaled_equals_unit_scaled(cases, shape):
    fmt, ra, rb, crow, kind, pm1 = cases
    for r in (ra, rb):   # every code of the format is present
        assert len(np.unique(r)) == 1 << BITS[fmt]
    ops, matrix, rows = (_operands16, _matrix16, 16) if shape == 16 else (_operands32, _matrix32, 32)
    a, b, c = ops(ra, rb, crow, BITS[fmt])
    ds, du = _run(shape, fmt, a, b, c)
    diff = ds.view(np.uint32) != du.view(np.uint32)
    print(f"shape {shape} fmt {fmt}: {int(diff.sum())} of {diff.size} D words differ between the forms")
    assert not diff.any(), np.argwhere(diff)[:8]

    d = matrix(du).astype(np.float64)
    cm = crow[:, :rows, None].astype(np.float64)
    if fmt == E2M3:
        ma, mb = DECODE3[ra[:, :rows]], DECODE3[rb[:, :rows]]
        kappa = 16.0 * np.einsum("nik,njk->nij", ma, mb) + 1024.0 * cm      # exact: integers and halves below 2^27
        use = kind != C_PAD
        err = np.abs(1024.0 * d - kappa)[use]
        bound = 258.0 if shape == 16 else 260.0
        print(f"shape {shape} e2m3: max |1024 D - kappa~| = {err.max()} key units (bound {bound})")
        assert (err < bound).all()
        assert (d[kind == C_PAD] < -9.0e29).all()
    else:
        ma, mb = DECODE1[ra[:, :rows]], DECODE1[rb[:, :rows]]
        use = pm1 & ((kind == C_ZERO) | (kind == C_ORB))
        assert use.sum() >= 32
        exact = np.einsum("nik,njk->nij", ma, mb) / 4.0 + cm                # +-1 operands: an integer plus C
        assert np.array_equal(d[use], exact[use])
