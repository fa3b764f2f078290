// SPDX-License-Identifier: MIT
// Conservative FP6 (e2m3) first pass of the exact SIFT matcher: the quantiser, the packed row layout
// and the bound arithmetic, for the device (match_device.hpp) and for the host (tests/cpp/sift_fp6_main.cpp,
// tests/test_sift_fp6_bound.py restates it in numpy; the one-subset certificate: tests/cpp/sift_fp6_cert_main.cpp,
// tests/test_sift_fp6_cert.py).  No HIP header is needed to compile it for the host.
//
// Quantiser.  A descriptor value u (integer 0..255) is written  a = u - OFFSET = SCALE * m + e  with m the
// nearest value an e2m3 element can hold, in units of 1/8:  +-{0..15, 16..30 step 2, 32..60 step 4}.  With
// OFFSET = 32 and SCALE = 4, a lies in [-32, 223] and m in [-8, 56]: nothing saturates, and
// |e| <= 2 (|a| < 64), <= 4 (|a| < 128), <= 8 otherwise.
//
// Keys.  For a query q and a train row t, with integer vectors a_q, a_t, the exact squared distance is
//     s = |a_q|^2 - 2 kappa,   kappa = <a_q, a_t> - |a_t|^2 / 2
// (the offset cancels in a_q - a_t).  The screen's MFMA computes, unscaled, i.e. with unit block scales (an e2m3
// element m stands for m / 8) and the f32 C operand keyf_t = -|a_t|^2 / 2048,
//     acc = <m_q, m_t> / 64 + keyf_t,   kappa~ = 1024 acc = 16 <m_q, m_t> - |a_t|^2 / 2.
//
// Bound.  <a_q, a_t> - 16 <m_q, m_t> = <a_q, e_t> + <e_q, SCALE m_t>, so by Cauchy-Schwarz
//     |kappa - kappa~| <= |a_q| max_t |e_t| + |e_q| max_t |SCALE m_t|
//                      <= E = |a_q| max_t |e_t| + |e_q| (max_t |a_t| + max_t |e_t|)
// (|SCALE m_t| = |a_t - e_t| <= |a_t| + |e_t|), with the maxima over the rows of the train image.  The
// squared norms are kept as integers, so their products are exact in a double.
// Accumulation.  Every product <= 60 * 60 / 64 and |keyf| <= 128 * 223^2 / 2048, so every partial sum of the
// 128 products and C, in any order, is below 2^14 in magnitude.  If each of the <= 129 additions loses at
// most one f32 ulp at that magnitude (2^-9: round-to-nearest loses half of the 2^-10 ulp, truncation all
// of it, and another factor 2 is left for alignment that keeps fewer bits), acc is off by < 129 * 2^-9
// < 0.26, i.e. kappa~ by < 258 (the 32 x 32 x 64 form below: <= 130 additions, < 260).  SLACK = 1025 is four
// times that, plus 1 for the rounding of this header's own double arithmetic (values < 2^27, a handful of
// roundings of 2^-26 each).
//
// Screen.  Let K1 >= K2 be the two largest of the 16 row-subset maxima of kappa~: the maxima of two
// different rows, both with kappa >= K2 - E - SLACK, and no row has kappa > K1 + E + SLACK.  Hence
//     s1 >= na - 2 (K1 + E + SLACK),   s2 <= na - 2 (K2 - E - SLACK)
// for the true best and second-best squared distances, and Lowe's test, monotone in both, fails for
// the true pair when it fails for (floor of the first bound clamped at 0, ceil of the second).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SFMX_FP6_HD __host__ __device__ __forceinline__
#else
#define SFMX_FP6_HD inline
#endif

namespace sfmx {
namespace fp6 {

constexpr int OFFSET = 32;
constexpr int SCALE = 4;
constexpr int ROW_BYTES = 96;          // 128 elements x 6 bits
constexpr int ROW_WORDS = 24;
constexpr float PAD_KEY = -1.0e30f;    // C operand of a pad row: never a subset maximum that counts
constexpr float KEY_VALID = -1.0e29f;  // real keys are > -2^14
constexpr float KEY_INIT = -3.0e38f;   // running maximum before any row
constexpr double SLACK = 1025.0;       // kappa~ units (see above)

// m (units of 1/8 of an e2m3 element, i.e. a ~ SCALE * m) nearest to a / SCALE, for -32 <= a <= 223.
// Branch-free: with the step 2^s of the magnitudes around |a| / SCALE (s = 0 below 16, 1 below 32, else 2),
// |m| = t << s, t = (|a| + (2 << s)) >> (2 + s)  (round half up: integers 0..16, even 16..32, multiples of 4).
SFMX_FP6_HD int quant_m(int a) {
    const int mag = a < 0 ? -a : a, s = (mag >> 6) < 2 ? (mag >> 6) : 2;
    const int m = ((mag + (2 << s)) >> (2 + s)) << s;
    return a < 0 ? -m : m;
}
// The 6-bit e2m3 code (sign, 2 exponent bits, 3 mantissa bits; bias 1, subnormals) of m / 8: magnitudes
// 0..15 are their own code (exponent 0: subnormal 0..7; exponent 1: 8..15), 16 + 2 k is 16 + k, 32 + 4 k is 24 + k.
SFMX_FP6_HD unsigned code_of_m(int m) {
    const unsigned mag = (unsigned)(m < 0 ? -m : m), s = (mag >= 16u) + (mag >= 32u);
    return (8u * s + (mag >> s)) | (m < 0 ? 0x20u : 0u);
}
// The value (units of 1/8) an e2m3 code stands for: the inverse of code_of_m.
SFMX_FP6_HD int m_of_code(unsigned c) {
    const int man = (int)(c & 7u), ex = (int)((c >> 3) & 3u);
    const int mag = ex == 0 ? man : (8 + man) << (ex - 1);
    return (c & 0x20u) ? -mag : mag;
}

// Packed row.  The MFMA lane group g = 0..3 of a row takes elements 32 g .. 32 g + 31 as one 192-bit
// fragment, element i at bits [6 i, 6 i + 6).  A fragment's 6 words are stored as 4 words at word 4 g
// of the row (one 16-B read) and 2 words at word 16 + 2 g (one 8-B read): words 0..15 of a row are its
// "plane A" part, 16..23 its "plane B" part.
SFMX_FP6_HD int word_index(int g, int w) { return w < 4 ? 4 * g + w : 16 + 2 * g + (w - 4); }

// Host-side packing of one row (the device packs with lane shuffles, prep_l2_row).
inline void pack_row(const unsigned* codes /*128*/, uint32_t* out /*24*/) {
    for (int i = 0; i < ROW_WORDS; ++i) out[i] = 0;
    for (int k = 0; k < 128; ++k) {
        const int g = k >> 5, bit = 6 * (k & 31);
        const uint64_t v = (uint64_t)(codes[k] & 63u) << (bit & 31);
        out[word_index(g, bit >> 5)] |= (uint32_t)v;
        if ((bit & 31) > 26) out[word_index(g, (bit >> 5) + 1)] |= (uint32_t)(v >> 32);
    }
}

// Swizzled position of a row's 16-B pieces inside an LDS stage (speed only: query and train rows share
// the fragment order through word_index alone).
//   plane A: 64 B per row, piece c = g at slot c ^ swz_a(row); plane B: 32 B per row, piece c = g >> 1
//   at slot c ^ swz_b(row).  tests/test_sift_fp6_bound.py enumerates the banks of every read group.
SFMX_FP6_HD constexpr int swz_a(int row) { return (0 - (row >> 2)) & 3; }
SFMX_FP6_HD constexpr int swz_b(int row) { return (row >> 3) & 1; }

// The 32 x 32 x 64 form of the screen (sift_screen6w_kernel): v_mfma_f32_32x32x64_f8f6f4, two chained
// MFMAs per tile of 32 train rows x 32 queries.  Lane l owns column l & 31 and K-half h = l >> 5; MFMA
// m = 0, 1 of a tile takes fragment frag32(m, h) of the train row (A) and of the query (B): any bijection
// onto the row's four fragments is correct as long as both operands use the same one.
//   Accumulator register i = 0..15 of a lane with half h is train row acc_row32(i, h) of the 32-row block.
//   Registers i and i + 8 are rows 16 apart, the same row subset j mod 16, so a lane folds them into 8
//   chains, chain c = max3(chain c, acc[c], acc[c + 8]), and chain c of half h is row subset
//   chain_subset32(c, h); the two halves of a column hold all 16 between them.
//   Accumulation: the chained form rounds the intermediate accumulator once more, 130 additions instead
//   of 129: acc is off by < 130 * 2^-9 < 0.26, kappa~ by < 2 * 130 = 260 key units, against SLACK = 1025.
SFMX_FP6_HD constexpr int frag32(int m, int h) { return 2 * m + h; }
SFMX_FP6_HD constexpr int acc_row32(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }
SFMX_FP6_HD constexpr int chain_subset32(int c, int h) { return (c & 3) + 4 * h + 8 * (c >> 2); }
// Byte offsets of that form's LDS reads inside a stage of STAGE rows (plane A | plane B | keys, the layout
// and the swizzles of the 16 x 16 form).  Lane (row, h) reads fragment f = frag32(m, h): 16 B of plane A,
// conflict-free in the ds_read_b128 lane groups, and 8 B of plane B.  The lanes of a 32-lane half all read
// the same 8-B half of a 16-B piece, 32 banks for 64 words: a 2-way conflict under any swizzle of 16-B
// pieces (two 8-B reads against six 16-B reads per row block).  The keys of registers 4 k .. 4 k + 3 are
// four consecutive rows, one 16-B read per k, the same address in every lane of a half (broadcast).
// tests/test_sift_fp6_screen32.py enumerates the banks.
SFMX_FP6_HD constexpr int lds_a32(int row, int f) { return row * 64 + 16 * (f ^ swz_a(row)); }
SFMX_FP6_HD constexpr int lds_b32(int stage, int row, int f) {
    return stage * 64 + row * 32 + 16 * ((f >> 1) ^ swz_b(row)) + 8 * (f & 1);
}
SFMX_FP6_HD constexpr int lds_key32(int stage, int row0, int k, int h) { return stage * 96 + 4 * (row0 + 8 * k + 4 * h); }

#if defined(__HIPCC__)
// The f8f6f4 MFMAs of the matcher (device only).  FMT is the element format code of both operands: 2 = e2m3
// (the FP6 SIFT screens), 4 = e2m1 (the FP4 ORB kernels).  SCALED issues v_mfma_scale_f32_*_f8f6f4 with unit
// E8M0 block scales (the 16-byte paired encoding: a scale load, then the MFMA, and one more VGPR read twice);
// !SCALED passes constant zero scale arguments, for which the compiler selects the plain 8-byte
// v_mfma_f32_*_f8f6f4: the unscaled instruction is the unit-scale product (tests/test_gpu_mfma_unscaled.py
// compares the raw bits of D of both forms).
constexpr int FMT_E2M3 = 2, FMT_E2M1 = 4;
typedef int mfma_i32x8 __attribute__((ext_vector_type(8)));
typedef float mfma_f32x4 __attribute__((ext_vector_type(4)));
typedef float mfma_f32x16 __attribute__((ext_vector_type(16)));
template <int FMT, bool SCALED>
__device__ __forceinline__ mfma_f32x4 mfma16(mfma_i32x8 a, mfma_i32x8 b, mfma_f32x4 c) {
    if constexpr (SCALED) return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, FMT, FMT, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
    else return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, FMT, FMT, 0, 0, 0, 0);
}
template <int FMT, bool SCALED>
__device__ __forceinline__ mfma_f32x16 mfma32(mfma_i32x8 a, mfma_i32x8 b, mfma_f32x16 c) {
    if constexpr (SCALED) return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, FMT, FMT, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
    else return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, FMT, FMT, 0, 0, 0, 0);
}
#endif

SFMX_FP6_HD float sqrt_rn(int64_t s) { return (float)__builtin_sqrt((double)s); }

// 1: the query is certainly rejected by Lowe's test.  k1 >= k2: the two largest subset maxima of acc;
// na = |a_q|^2, e2q = |e_q|^2, emax2 / amax2 = max over the train image's rows of |e_t|^2 / |a_t|^2.
SFMX_FP6_HD int certainly_rejected(float k1, float k2, int na, int e2q, int emax2, int amax2, double ratio) {
    const double E = __builtin_sqrt((double)na * (double)emax2) +
                     __builtin_sqrt((double)e2q) * (__builtin_sqrt((double)amax2) + __builtin_sqrt((double)emax2));
    const double M = E + SLACK;
    double lo = (double)na - 2.0 * ((double)k1 * 1024.0 + M);
    double hi = (double)na - 2.0 * ((double)k2 * 1024.0 - M);
    lo = lo < 0.0 ? 0.0 : lo;
    hi = hi < 0.0 ? 0.0 : (hi > 1.0e12 ? 1.0e12 : hi);
    lo = lo > 1.0e12 ? 1.0e12 : lo;
    const int64_t s1 = (int64_t)__builtin_floor(lo), s2 = (int64_t)__builtin_ceil(hi);
    return (int)!((double)sqrt_rn(s1) < (double)sqrt_rn(s2) * ratio);
}

// One-subset certificate.  k1 > k2 as above, r1 the row subset (j mod 16) of k1's row, nt the train rows.
// With M = E + SLACK every row of subset r1's maximum has s <= s1hi and every row outside r1 has s >= lo,
// some row outside it s <= hi:
//     s1hi = ceil(max(na - 2 (1024 k1 - M), 0)),  lo = floor(max(na - 2 (1024 k2 + M), 0)),
//     hi = ceil(max(na - 2 (1024 k2 - M), 0)).
// 1: the query's best row lies in subset r1 strictly ahead of every row outside it (s1hi < lo: no index
// tie across subsets), Lowe's test passes against every row outside it (at (s1hi, lo), monotone), the
// exact s2 <= hi is below the float-sqrt collision range (SQRT_SAFE_S, the matcher's SQRT_SAFE), and the
// subset holds two real rows (r1 + 16 < nt).  The exact top-2 (a1, a2) of subset r1 alone then settles the
// query: s1 = a1, s2 = min(a2, s_other) with s_other in [lo, hi], and Lowe's test, which passes at every
// s2 >= lo, fails at the true s2 exactly when it fails at a2 (sift_finish_kernel).
constexpr int64_t SQRT_SAFE_S = 1 << 22;
SFMX_FP6_HD int certified(float k1, float k2, int r1, int nt, int na, int e2q, int emax2, int amax2, double ratio) {
    const double E = __builtin_sqrt((double)na * (double)emax2) +
                     __builtin_sqrt((double)e2q) * (__builtin_sqrt((double)amax2) + __builtin_sqrt((double)emax2));
    const double M = E + SLACK;
    double s1 = (double)na - 2.0 * ((double)k1 * 1024.0 - M);
    double lo = (double)na - 2.0 * ((double)k2 * 1024.0 + M);
    double hi = (double)na - 2.0 * ((double)k2 * 1024.0 - M);
    s1 = s1 < 0.0 ? 0.0 : (s1 > 1.0e12 ? 1.0e12 : s1);
    lo = lo < 0.0 ? 0.0 : (lo > 1.0e12 ? 1.0e12 : lo);
    hi = hi < 0.0 ? 0.0 : (hi > 1.0e12 ? 1.0e12 : hi);
    // integers <= 10^12, exact in a double: compared and rooted as doubles (sqrt_rn of the same integers)
    const double s1hi = __builtin_ceil(s1), slo = __builtin_floor(lo), shi = __builtin_ceil(hi);
    const int usable = (int)(nt >= 2) & (int)(k2 > KEY_VALID);
    const int lowe = (int)((double)(float)__builtin_sqrt(s1hi) < (double)(float)__builtin_sqrt(slo) * ratio);
    return usable & (int)(s1hi < slo) & lowe & (int)(shi < (double)SQRT_SAFE_S) & (int)(r1 + 16 < nt);
}

}  // namespace fp6
}  // namespace sfmx
