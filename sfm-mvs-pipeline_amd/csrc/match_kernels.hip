// SPDX-License-Identifier: MIT
// sfmx matcher kernels for gfx950 (MI355X / CDNA4).
//
// Replaces, per image pair, cv::BFMatcher(NORM_L2|NORM_HAMMING)::knnMatch(L, R, m, 2)
// + Lowe's ratio test as called at
//   src/photogrammetrie/sfm/UnorderedFeatureMatchingStrategy.cpp:50-64
//   (same code: VideoFeatureMatchingStrategy.cpp:61-75, GridFeatureMatchingStrategy.cpp:104-118)
// and the match-graph filters of SfM::calculateShotMatches (sfm/SfM.cpp:547-570).
//
// Semantics reproduced bit for bit (see oracle/match_oracle.cpp):
//   L2:      d = sqrtf(sum (a-b)^2), top-2 ranked on (float bits of d, train index)
//   Hamming: d = popcount(a xor b),  top-2 ranked on (d, train index)
//   ratio:   accept m0 iff (double)d0 < (double)d1 * ratio; a single neighbour is accepted.
//
// SIFT kernel design (sift_knn2_kernel):
//   * descriptors are integer 0..255, stored as int8 a' = a - 128, so the
//     distance contraction is an exact int8 MFMA: v_mfma_i32_32x32x32_i8,
//     K = 128 = 4 MFMAs per 32x32 tile.
//   * D = A * B with A = 32 train rows (from LDS), B = 32 queries (registers):
//     each lane's accumulator column is ONE query, its 16 registers are 16
//     train rows, so the 2-NN reduction is lane-local (no shuffles per tile).
//   * ranking key per element, one VALU op (v_lshl_add_u32):
//         key = (dot << 9) + keyc[j],  keyc[j] = -(nb_j << 8) + 255 - (j & 255)
//             = 256 * (2 dot - nb_j) + (255 - (j & 255))
//     Larger key <=> smaller s = na + nb - 2 dot, ties -> smaller j (within a
//     256-row chunk); fits int32 because s < 2^23.  Top-2 by max: two VALU ops
//     (v_med3_i32, v_max_i32).  Every 256 rows the chunk's top-2 is merged with
//     the partner half-wave and folded into the running (t, j) top-2; later
//     chunks only win on strictly smaller t (OpenCV's strict '<' insertion).
//   * integer s ranks like sqrtf(s) bits while s < SQRT_SAFE; a query whose
//     2nd-best s reaches it is handed to sift_slow_kernel (exact float sqrt
//     ranking, 64-bit keys).  Real SIFT distances never get there.
//   * train rows stream through a double-buffered LDS stage (64 rows, 8 KiB)
//     filled by global_load_lds_dwordx4 with an XOR-swizzled source address
//     (conflict-free ds_read_b128 fragment reads).
//   * one work item = 512 queries of one pair (8 waves x 2 query tiles x 32);
//     work items are sorted by train image and mapped XCD-contiguously so the
//     blocks streaming one train image share an XCD's L2.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <climits>
#include <cstdlib>
#include "match_common.hpp"
#include "diag.hpp"
#include "sift_fp6.hpp"

namespace sfmx {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define GLOBAL_AS __attribute__((address_space(1)))
#define LDS_AS __attribute__((address_space(3)))

__device__ __forceinline__ int med3i(int a, int b, int c) { return max(min(a, b), min(max(a, b), c)); }
// Explicit v_med3_i32 / v_max3_i32: hipcc only pattern-matches med3 from some
// min/max shapes; in the pairwise top-2 update it otherwise emits 4 ops.
__device__ __forceinline__ int v_med3(int a, int b, int c) {
    int d;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ int v_max3(int a, int b, int c) {
    int d;
    asm("v_max3_i32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ unsigned med3u(unsigned a, unsigned b, unsigned c) { return max(min(a, b), min(max(a, b), c)); }

// Correctly rounded sqrtf of an exact integer < 2^24: the double sqrt is
// correctly rounded and 53 >= 2*24+2, so rounding it to float is the
// correctly rounded float sqrt (no double-rounding error).  Exhaustively
// checked against host sqrtf by tests/test_gpu_match.py.
__device__ __forceinline__ float sqrt_rn_int(int64_t s) { return (float)__builtin_sqrt((double)s); }

// Pad-row key of the screening pass (C2 operand): 0xC0C0C0C0 + dot never reaches
// KEY_VALID, real keys are >= -(2^21 + 2^20).
constexpr int PAD_KEY = (int)0xC0C0C0C0;
constexpr int KEY_VALID = -(1 << 29);
// dense_idx of a query pass 1 forwarded to pass 2; assemble_kernel counts any left over
// (a pass-2 grid that did not cover its item's queries) and the run fails loudly.
constexpr int UNSETTLED = -3;
static_assert(PAD_KEY < KEY_VALID - (1 << 22), "pad keys must never look valid");

// Lowe's acceptance applied to the best index as an all-ones mask, with no bool PHI.
// ROCm 7.2 (clang 22) miscompiled `acc = nt >= 2 ? (d1 < d2 * ratio) : true; out = acc ? J1 : -1`
// in some register allocations (MINW = 1 / other tilings): the divergent select became an
// exec-masked PHI whose -1 default was written with the full exec mask into the VGPR that also
// held J1, which the same block had already reused as a temporary, so every query of a pair with
// nt >= 2 came out rejected.  Integer arithmetic keeps it a straight-line select.
__device__ __forceinline__ int lowe_select(int j1, float d1, float d2, int nt, double ratio) {
    const int rej = (int)(nt >= 2) & (int)!((double)d1 < (double)d2 * ratio);
    return j1 | -rej;
}

// Bijective XCD-contiguous remap: blocks b, b+8, ... share an XCD (observed
// round-robin dispatch; speed only, never correctness).
__device__ __forceinline__ int xcd_remap(int b, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = b & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}

// ---------------------------------------------------------------------------
// prep: float SIFT rows -> int8 a' = a - 128, ||a'||^2, chunk keys, integrality.
// 32 threads per row (float4 each); pad rows are written as zeros.
// The FP6 screen's per-row operands (sift_fp6.hpp), written by the batched prep beside the int8 ones.
struct Fp6Rows {
    uint32_t* desc6;   // [row][24]  packed e2m3 row
    float* keyf;       // [row]      C operand -|a|^2 / 2048 (pad rows: fp6::PAD_KEY)
    int2* ne;          // [row]      (|a|^2, |e|^2), a = u - 32
};
__device__ __forceinline__ int2 prep_l2_row(const float* __restrict__ src, int r, int rows, int cols,
                                            int8_t* __restrict__ dst, int32_t* __restrict__ norm,
                                            int32_t* __restrict__ keyc, int32_t* __restrict__ keyc2,
                                            int32_t* __restrict__ nonintegral, const Fp6Rows* f6 = nullptr);
__global__ void prep_l2_kernel(const float* __restrict__ src, int rows, int cols, int rows_pad,
                               int8_t* __restrict__ dst, int32_t* __restrict__ norm,
                               int32_t* __restrict__ keyc, int32_t* __restrict__ keyc2,
                               int32_t* __restrict__ nonintegral) {
    const int r = blockIdx.x * (blockDim.x >> 5) + (threadIdx.x >> 5);
    if (r >= rows_pad) return;
    prep_l2_row(src, r, rows, cols, dst, norm, keyc, keyc2, nonintegral);
}
// All images of a set_images call in one launch: blockIdx.y = image (table in HBM).
constexpr int PREP_ROWS = 64;   // rows per workgroup of the batched prep
static_assert(ROW_ALIGN % PREP_ROWS == 0 && PREP_ROWS % 8 == 0, "whole 8-row steps, no partial workgroup");
__global__ void prep_l2_batch_kernel(const PrepImg* __restrict__ tab, int8_t* __restrict__ desc8,
                                     int32_t* __restrict__ norm, int32_t* __restrict__ keyc,
                                     int32_t* __restrict__ keyc2, int32_t* __restrict__ flags, Fp6Rows f6,
                                     int32_t* __restrict__ imax) {
    const PrepImg t = tab[blockIdx.y];
    const Fp6Rows f6i{f6.desc6 + t.row0 * fp6::ROW_WORDS, f6.keyf + t.row0, f6.ne + t.row0};
    int emax = 0, amax = 0;   // the image's largest |e|^2 and |a|^2 over this workgroup's rows
    // PREP_ROWS rows per workgroup, 8 at a time (rows_pad is a multiple of PREP_ROWS)
    for (int r = blockIdx.x * PREP_ROWS + (threadIdx.x >> 5); r < min((int)(blockIdx.x + 1) * PREP_ROWS, t.rows_pad);
         r += blockDim.x >> 5) {
        const int2 em = prep_l2_row(t.src, r, t.rows, t.cols, desc8 + t.row0 * SIFT_DIM, norm + t.row0, keyc + t.row0,
                                    keyc2 + t.row0, flags + blockIdx.y, &f6i);
        emax = max(emax, em.x);
        amax = max(amax, em.y);
    }
    // One pair of atomics per workgroup at most, and only where it raises the image's maximum (imax is zero
    // before the launch): every image's words share a few cache lines, and unconditional atomics from each
    // wave serialised there (prep 283 -> 158 us on 50 x 8192 rows with this guard).
    __shared__ int wmax[2][PREP_ROWS / 8];
    for (int o = 32; o > 0; o >>= 1) {
        emax = max(emax, __shfl_xor(emax, o));
        amax = max(amax, __shfl_xor(amax, o));
    }
    if ((threadIdx.x & 63) == 0) { wmax[0][threadIdx.x >> 6] = emax; wmax[1][threadIdx.x >> 6] = amax; }
    __syncthreads();
    if (threadIdx.x < 2) {
        int v = 0;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) v = max(v, wmax[threadIdx.x][i]);
        int32_t* p = imax + 2 * blockIdx.y + threadIdx.x;
        if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, v);
    }
}
// -> (|e|^2, |a|^2) of the row's FP6 form (0, 0 for a pad row or without f6).
__device__ __forceinline__ int2 prep_l2_row(const float* __restrict__ src, int r, int rows, int cols,
                                            int8_t* __restrict__ dst, int32_t* __restrict__ norm,
                                            int32_t* __restrict__ keyc, int32_t* __restrict__ keyc2,
                                            int32_t* __restrict__ nonintegral, const Fp6Rows* f6) {
    const int c4 = threadIdx.x & 31;   // 4 columns each
    int v[4] = {0, 0, 0, 0};
    bool bad = false;
    if (r < rows) {
        float f4[4] = {0.f, 0.f, 0.f, 0.f};
        if (cols == SIFT_DIM && ((uintptr_t)src & 15) == 0) {   // full 512-B rows: one 16-B load per lane
            const float4 q = reinterpret_cast<const float4*>(src + (int64_t)r * SIFT_DIM)[c4];
            f4[0] = q.x; f4[1] = q.y; f4[2] = q.z; f4[3] = q.w;
        } else {
            for (int e = 0; e < 4; ++e)
                if (c4 * 4 + e < cols) f4[e] = src[(int64_t)r * cols + c4 * 4 + e];
        }
        for (int e = 0; e < 4; ++e) {
            if (c4 * 4 + e < cols) {
                const float f = f4[e];
                const bool ok = (f >= 0.f) && (f <= 255.f) && (f == __builtin_floorf(f));
                bad |= !ok;
                v[e] = ok ? (int)f - 128 : 0;
            }
        }
    }
    const unsigned packed = (unsigned)(v[0] & 255) | ((unsigned)(v[1] & 255) << 8) |
                            ((unsigned)(v[2] & 255) << 16) | ((unsigned)(v[3] & 255) << 24);
    reinterpret_cast<unsigned*>(dst + (int64_t)r * SIFT_DIM)[c4] = packed;
    int n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    for (int o = 16; o > 0; o >>= 1) n2 += __shfl_xor(n2, o, 32);
    if (__any(bad) && c4 == 0) atomicOr(nonintegral, 1);
    if (c4 == 0) {
        norm[r] = n2;
        keyc[r] = (r < rows) ? (-(n2 << 8) + 255 - (r & 255)) : INT_MIN;
        keyc2[r] = (r < rows) ? -((n2 + 1) >> 1) : PAD_KEY;     // screening pass: -ceil(nb / 2)
    }
    if (!f6) return make_int2(0, 0);
    // FP6 form of u = v + 128: a = u - 32 = v + 96 = SCALE m + e; 4 elements = 24 bits per lane, 8 lanes per
    // 192-bit fragment, whose word w is cut from the 48 bits of lanes (4 w) / 3 and (4 w) / 3 + 1.
    // One reduction for both sums: |e|^2 <= 2^13 above sum (v + 128) < 2^15; |a|^2 = n2 + 192 sum v + 128 * 96^2.
    unsigned chunk = 0;
    int red = 0;
    if (r < rows) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int a = v[e] + 128 - fp6::OFFSET, m = fp6::quant_m(a), er = a - fp6::SCALE * m;
            chunk |= fp6::code_of_m(m) << (6 * e);
            red += ((er * er) << 16) + v[e] + 128;
        }
    }
    for (int o = 16; o > 0; o >>= 1) red += __shfl_xor(red, o, 32);
    const int e2 = red >> 16, a2 = r < rows ? n2 + 192 * ((red & 0xFFFF) - 128 * 128) + 128 * 96 * 96 : 0;
    const int w = c4 & 7, g = c4 >> 3, j0 = min((4 * w) / 3, 6);
    const unsigned lo = __shfl(chunk, (c4 & ~7) + j0, 32), hi = __shfl(chunk, (c4 & ~7) + j0 + 1, 32);
    const unsigned word = (unsigned)((((unsigned long long)hi << 24) | lo) >> (w < 6 ? 32 * w - 24 * j0 : 0));
    if (w < 6) f6->desc6[(int64_t)r * fp6::ROW_WORDS + fp6::word_index(g, w)] = word;
    if (c4 == 0) {
        f6->keyf[r] = (r < rows) ? -(float)a2 * (1.0f / 2048.0f) : fp6::PAD_KEY;   // exact: a2 < 2^23
        f6->ne[r] = make_int2(a2, e2);
    }
    return make_int2(e2, a2);
}

// Copy of the raw float rows for the fp32 fallback (non-integer SIFT values).
__global__ void prep_f32_kernel(const float* __restrict__ src, int rows, int cols, int rows_pad,
                                float* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)rows_pad * SIFT_DIM;
    if (i >= total) return;
    const int r = (int)(i / SIFT_DIM), c = (int)(i % SIFT_DIM);
    dst[i] = (r < rows && c < cols) ? src[(int64_t)r * cols + c] : 0.f;
}

// ORB rows (cols <= 32 bytes) -> zero-padded 32-byte rows.
__global__ void prep_hamming_kernel(const uint8_t* __restrict__ src, int rows, int cols, int rows_pad,
                                    uint8_t* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)rows_pad * ORB_BYTES;
    if (i >= total) return;
    const int r = (int)(i / ORB_BYTES), c = (int)(i % ORB_BYTES);
    dst[i] = (r < rows && c < cols) ? src[(int64_t)r * cols + c] : 0;
}

// ORB rows -> +-1 FP4 (e2m1) rows for the MFMA Hamming path: bit 1 -> +1.0
// (0x2), bit 0 -> -1.0 (0xA), so for two 256-bit rows dot = 256 - 2 * popcount(a ^ b).
// Missing bytes (cols < 32) encode as zero bytes, as the VALU path pads them.
// Pad rows are all +0.0 nibbles (contribute 0).  keyc[r] = float bits of the
// row's MFMA C-operand: 767 + (16383 - (r & 16383)) / 16384 (exact in f32),
// pad rows 0.0 (see orb_mfma_kernel).  32 threads per row, one u32 each.
__global__ void prep_hamming_fp4_kernel(const uint8_t* __restrict__ src, int rows, int cols, int rows_pad,
                                        uint32_t* __restrict__ dst, int32_t* __restrict__ keyc) {
    const int r = blockIdx.x * (blockDim.x >> 5) + (threadIdx.x >> 5);
    const int c = threadIdx.x & 31;
    if (r >= rows_pad) return;
    uint32_t w = 0;
    if (r < rows) {
        const unsigned byte = c < cols ? src[(int64_t)r * cols + c] : 0u;
#pragma unroll
        for (int b = 0; b < 8; ++b) w |= (((byte >> b) & 1u) ? 0x2u : 0xAu) << (4 * b);
    }
    dst[(int64_t)r * 32 + c] = w;
    if (c == 0) {
        const int jj = 16383 - (r & 16383);
        keyc[r] = r < rows ? __float_as_int((float)(767 * 16384 + jj) * (1.0f / 16384.0f)) : 0;
    }
}

// ---------------------------------------------------------------------------
// SIFT 2-NN, int8 MFMA.
// GATHER (pass 2 of the two-pass path): `work` is the compacted list of
// *work2_n items built by compact_work_kernel; an item's queries are entries
// [q0, q0 + 512) of its pair's list of unresolved queries (qlist at the pair's
// dense_base, qcount[pair] entries) written by sift_screen_kernel.
// LISTS (with GATHER; the product path behind sift_screen6_kernel): the query's exact top-2 goes to its list
// slot of `top2` as the two (s << 32) | j keys sift_finish_kernel merges for a mask of other than two bits.
// VIA (with LISTS): the item's entries are those of the pair's second list (`qcount` = its counters): entry
// e names the list slot `via[dense_base + e]`, whose query is gathered and whose two keys are written.
// The VIA launch is a fixed grid sized by the device, not by the job: workgroup b takes items b, b + gridDim.x,
// ... < *work2_n (the XCD remap applies to the item index), each with the body of a one-item workgroup.
//
// One work item, `item` of `nwork` (workgroup-uniform).  Every wave leaves behind the barrier that follows the
// last stage's reads (or, with no stage, the one before the loop), so the next item may restage the buffers.
template <int QT, int WAVES, int MINW, int STAGE, bool MFMA_FIRST, int PROBE, int PIPE, bool GATHER, bool LISTS, bool VIA>
__device__ __forceinline__
void sift_knn2_item(const int item, const int nwork, const WorkItem* __restrict__ work, const PairDev* __restrict__ pairs,
                    const ImgDev* __restrict__ imgs, const int8_t* __restrict__ desc8,
                    const int32_t* __restrict__ norm, const int32_t* __restrict__ keyc,
                    int32_t* __restrict__ out_idx, float* __restrict__ out_dist,
                    int2* __restrict__ slow_list, int32_t* __restrict__ slow_count, double ratio,
                    const int32_t* __restrict__ qlist, const int32_t* __restrict__ qcount,
                    unsigned long long* __restrict__ top2, const int32_t* __restrict__ via) {
    static_assert(!LISTS || GATHER, "the list slots are the gathered entries");
    static_assert(!VIA || LISTS, "the second list names list slots");
    constexpr int GLDS = STAGE * SIFT_DIM / (WAVES * 64 * 16);   // 16-B LDS-DMA pieces per thread per stage
    static_assert(GLDS * WAVES * 64 * 16 == STAGE * SIFT_DIM, "stage must split into whole 16-B pieces");
    static_assert(256 % STAGE == 0, "stages tile the 256-row key chunk");
    constexpr int DESC_BYTES = STAGE * SIFT_DIM;
    constexpr int BUF_BYTES = DESC_BYTES + STAGE * 4;      // + keys
    constexpr int SPC = 256 / STAGE;                       // stages per key chunk
    __shared__ __attribute__((aligned(16))) char lds[2 * BUF_BYTES];

    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    const WorkItem w = work[xcd_remap(item, nwork)];
    const PairDev P = pairs[w.pair];
    const ImgDev L = imgs[P.left], R = imgs[P.right];
    const int nq = L.rows, nt = R.rows;
    const int qbase = w.q0 + wid * (QT * 32);
    int qrow[QT];                     // query row of this lane's column in each query tile (-1: none)
    int qslot[QT];                    // LISTS: its list slot
    if constexpr (GATHER) {
        const int cnt = qcount[w.pair];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            const int e = qbase + qt * 32 + l32;
            qslot[qt] = e;
            if constexpr (VIA) qslot[qt] = e < cnt ? via[P.dense_base + e] : 0;
            qrow[qt] = e < cnt ? qlist[P.dense_base + qslot[qt]] : -1;
        }
    } else {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            const int qi = qbase + qt * 32 + l32;
            qrow[qt] = qi < nq ? qi : -1;
        }
    }

    // Query fragments (B operand): lane holds 16 bytes of k-block (2m + h).
    i32x4 bq[QT][4];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const int lr = GATHER ? (qrow[qt] < 0 ? 0 : qrow[qt]) : qbase + qt * 32 + l32;   // rows < rows_pad
        const i32x4* src = reinterpret_cast<const i32x4*>(desc8 + (L.row0 + lr) * SIFT_DIM);
#pragma unroll
        for (int m = 0; m < 4; ++m) bq[qt][m] = src[2 * m + h];
    }

    int T1[QT], J1[QT], T2[QT], J2[QT], c1[QT], c2[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        T1[qt] = T2[qt] = INT_MAX; J1[qt] = J2[qt] = -1; c1[qt] = c2[qt] = INT_MIN;
    }

    const int nstages = (nt + STAGE - 1) / STAGE;
    const int8_t* tbase = desc8 + R.row0 * SIFT_DIM;
    const int32_t* kbase = keyc + R.row0;

    auto stage = [&](int s, int buf) {
        char* base = lds + buf * BUF_BYTES;
#pragma unroll
        for (int i = 0; i < GLDS; ++i) {
            const int p = i * WAVES * 64 + threadIdx.x;  // 16-byte unit index in the stage
            const int rr = p >> 3, slot = p & 7, c = slot ^ ((rr >> 1) & 7);
            const int8_t* g = tbase + (int64_t)(s * STAGE + rr) * SIFT_DIM + 16 * c;
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)g,
                                             (LDS_AS void*)(base + (i * WAVES + wid) * 1024), 16, 0, 0);
        }
        if (wid < STAGE / 64)
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(kbase + s * STAGE + wid * 64 + lane),
                                             (LDS_AS void*)(base + DESC_BYTES + wid * 256), 4, 0, 0);
    };

    // Top-2 by max over packed keys, two new keys per step:
    //   m_i = med3(b1, ka, kb),  b1' = max3(b1, ka, kb)
    // and b2' = max(b2, m_1 .. m_8) as a max3 tree once per 16 keys, since
    // max(med3(b1, ka, kb), b2) chained over the steps equals that maximum
    // (1.25 VALU per element for the selection, + 1 for the key).
    auto select = [&](const i32x16& acc, const i32x4 (&kv)[4], int& b1, int& b2) {
        int m[8];
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const int ka = (int)(((unsigned)acc[r] << 9) + (unsigned)kv[r >> 2][r & 3]);
            const int kb = (int)(((unsigned)acc[r + 1] << 9) + (unsigned)kv[r >> 2][(r + 1) & 3]);
            m[r >> 1] = v_med3(b1, ka, kb);
            b1 = v_max3(b1, ka, kb);
        }
        b2 = v_max3(v_max3(m[0], m[1], m[2]), v_max3(m[3], m[4], m[5]), v_max3(m[6], m[7], b2));
    };

    if (nstages > 0) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int s = 0; s < nstages; ++s) {
        const int buf = s & 1;
        if (s + 1 < nstages) stage(s + 1, buf ^ 1);
        const char* base = lds + buf * BUF_BYTES;
        if constexpr (PIPE > 0) {
            // Software pipeline over the stage's (tile, query-tile) steps: the MFMA chain
            // of step k is issued first, the selection of step k-1 (independent of it)
            // runs under it; sched_group_barrier interleaves 1 MFMA with PIPE VALU ops.
            i32x16 prev = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            i32x4 kvp[4];
#pragma unroll
            for (int t = 0; t < STAGE / 32; ++t) {
                const int row = t * 32 + l32;
                i32x4 a[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int slot = (2 * m + h) ^ ((row >> 1) & 7);
                    a[m] = *reinterpret_cast<const i32x4*>(base + row * SIFT_DIM + 16 * slot);
                }
                i32x4 kv[4];
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    kv[g] = *reinterpret_cast<const i32x4*>(base + DESC_BYTES + 4 * (t * 32 + 8 * g + 4 * h));
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                    for (int m = 0; m < 4; ++m) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[m], bq[qt][m], acc, 0, 0, 0);
                    if (t > 0 || qt > 0) {
                        const int pq = qt > 0 ? qt - 1 : QT - 1;
                        select(prev, qt > 0 ? kv : kvp, c1[pq], c2[pq]);
#pragma unroll
                        for (int m = 0; m < 4; ++m) {
                            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // 1 MFMA
                            __builtin_amdgcn_sched_group_barrier(0x002, PIPE, 0);   // PIPE VALU
                        }
                    }
                    prev = acc;
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) kvp[g] = kv[g];
            }
            select(prev, kvp, c1[QT - 1], c2[QT - 1]);
        } else
#pragma unroll
        for (int t = 0; t < STAGE / 32; ++t) {
            const int row = t * 32 + l32;
            i32x4 a[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int slot = (2 * m + h) ^ ((row >> 1) & 7);
                a[m] = *reinterpret_cast<const i32x4*>(base + row * SIFT_DIM + 16 * slot);
            }
            i32x4 kv[4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
                kv[g] = *reinterpret_cast<const i32x4*>(base + DESC_BYTES + 4 * (t * 32 + 8 * g + 4 * h));
            if constexpr (MFMA_FIRST) {
                i32x16 acc[QT];
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    acc[qt] = i32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                    for (int m = 0; m < 4; ++m) acc[qt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[m], bq[qt][m], acc[qt], 0, 0, 0);
                }
                if constexpr (PROBE == 1) {   // timing probe only: MFMA + staging skeleton, no selection
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt) c1[qt] = v_max3(c1[qt], acc[qt][0], acc[qt][15]);
                } else {
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt) select(acc[qt], kv, c1[qt], c2[qt]);
                }
            } else {
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                    for (int m = 0; m < 4; ++m) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[m], bq[qt][m], acc, 0, 0, 0);
                    select(acc, kv, c1[qt], c2[qt]);
                }
            }
        }
        if ((s % SPC) == SPC - 1 || s + 1 == nstages) {      // end of a 256-row chunk
            const int cb = (s / SPC) * 256;
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                const int p1 = __shfl_xor(c1[qt], 32), p2 = __shfl_xor(c2[qt], 32);
                const int m1 = max(c1[qt], p1), m2 = max(min(c1[qt], p1), max(c2[qt], p2));
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int key = e == 0 ? m1 : m2;
                    if (key != INT_MIN) {
                        const int t_ = -(key >> 8), j_ = cb + 255 - (key & 255);
                        if (t_ < T2[qt]) {
                            if (t_ < T1[qt]) { T2[qt] = T1[qt]; J2[qt] = J1[qt]; T1[qt] = t_; J1[qt] = j_; }
                            else { T2[qt] = t_; J2[qt] = j_; }
                        }
                    }
                }
                c1[qt] = c2[qt] = INT_MIN;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // Epilogue: lanes of half 0 own query column l32 of each tile.
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const int qi = qrow[qt];
        if (h != 0 || qi < 0) continue;
        if constexpr (LISTS) {   // (an empty train image forwards nothing; a missing key stays ~0: unsettled)
            const long long na = norm[L.row0 + qi];
            const unsigned long long k1 = T1[qt] != INT_MAX ? ((unsigned long long)(na + T1[qt]) << 32) | (unsigned)J1[qt] : ~0ull;
            const unsigned long long k2 = T2[qt] != INT_MAX ? ((unsigned long long)(na + T2[qt]) << 32) | (unsigned)J2[qt] : ~0ull;
            *reinterpret_cast<ulonglong2*>(top2 + 2 * (P.dense_base + qslot[qt])) = make_ulonglong2(k1, k2);
            continue;
        }
        const int64_t o = P.dense_base + qi;
        if (nt == 0) { out_idx[o] = -1; out_dist[o] = 0.f; continue; }
        const int64_t na = norm[L.row0 + qi];
        const int64_t s1 = (int64_t)T1[qt] + na, s2 = (int64_t)T2[qt] + na;
        if (nt >= 2 && s2 >= SQRT_SAFE) {
            const int slot = atomicAdd(slow_count, 1);
            slow_list[slot] = make_int2(w.pair, qi);
            out_idx[o] = -2;
            continue;
        }
        const float d1 = sqrt_rn_int(s1);
        out_idx[o] = lowe_select(J1[qt], d1, nt >= 2 ? sqrt_rn_int(s2) : 0.f, nt, ratio);
        out_dist[o] = d1;
    }
}

template <int QT, int WAVES, int MINW, int STAGE, bool MFMA_FIRST, int PROBE = 0, int PIPE = 0, bool GATHER = false,
          bool LISTS = false, bool VIA = false>
__global__ __launch_bounds__(WAVES * 64, MINW)
void sift_knn2_kernel(const WorkItem* __restrict__ work, const PairDev* __restrict__ pairs,
                      const ImgDev* __restrict__ imgs, const int8_t* __restrict__ desc8,
                      const int32_t* __restrict__ norm, const int32_t* __restrict__ keyc,
                      int32_t* __restrict__ out_idx, float* __restrict__ out_dist,
                      int2* __restrict__ slow_list, int32_t* __restrict__ slow_count, double ratio,
                      const int32_t* __restrict__ qlist = nullptr, const int32_t* __restrict__ qcount = nullptr,
                      const int32_t* __restrict__ work2_n = nullptr, unsigned long long* __restrict__ top2 = nullptr,
                      const int32_t* __restrict__ via = nullptr) {
#define SIFT_KNN2_ITEM(item, nwork)                                                                                    \
    sift_knn2_item<QT, WAVES, MINW, STAGE, MFMA_FIRST, PROBE, PIPE, GATHER, LISTS, VIA>(                               \
        item, nwork, work, pairs, imgs, desc8, norm, keyc, out_idx, out_dist, slow_list, slow_count, ratio, qlist, qcount, \
        top2, via)
    if constexpr (VIA) {              // a fixed grid over the compacted list of *work2_n items
        const int nwork = *work2_n;
        for (int item = blockIdx.x; item < nwork; item += gridDim.x) SIFT_KNN2_ITEM(item, nwork);
    } else if constexpr (GATHER) {    // compacted list of *work2_n work items; the grid is an upper bound
        const int nwork = *work2_n;
        if ((int)blockIdx.x < nwork) SIFT_KNN2_ITEM((int)blockIdx.x, nwork);
    } else {
        SIFT_KNN2_ITEM((int)blockIdx.x, (int)gridDim.x);
    }
#undef SIFT_KNN2_ITEM
}

// ---------------------------------------------------------------------------
// Two-pass ratio test, pass 1 (default SIFT path): sift_screen_kernel settles
// every query whose ratio test certainly fails, with 0.5 VALU per element.
//
//   The C operand of train row j is  C2_j = -ceil(nb_j / 2),  so the MFMA leaves
//       K = dot + C2_j = floor(X / 2),   X = 2 dot - nb_j,   s = na - X,
//   i.e. s in [na - 2K - 1, na - 2K].  Each lane keeps, per query tile, the max of
//   K over 8 disjoint row subsets (chain c takes accumulator rows 2c and 2c+1 of
//   every tile: one v_max3 per two elements); with the partner half-wave that is
//   16 subsets per query.  The best elements of two different subsets are two
//   different rows, so with K1 >= K2 the two largest subset maxima,
//       s1 >= na - 2 K1 - 1   and   s2 <= na - 2 K2.
//   Lowe's test (double)sqrtf(s1) < (double)sqrtf(s2) * ratio is monotone
//   (non-increasing in s1, non-decreasing in s2 for ratio >= 0; never true for
//   ratio <= 0), so if it fails at (s1_lb, s2_ub) it fails for the true (s1, s2):
//   the query is rejected, exactly as the exact path would reject it.  Every
//   other query (accepted or undecided, fewer than 2 train rows, fewer than 2
//   non-empty subsets) goes to its pair's list for pass 2, the exact kernel in
//   GATHER mode.  Only accepted matches leave the matcher (sfmx_matcher_run /
//   device_results), so a rejected query's distance is never observed.
template <int QT, int WAVES, int MINW, int STAGE>
__global__ __launch_bounds__(WAVES * 64, MINW)
void sift_screen_kernel(const WorkItem* __restrict__ work, const PairDev* __restrict__ pairs,
                        const ImgDev* __restrict__ imgs, const int8_t* __restrict__ desc8,
                        const int32_t* __restrict__ norm, const int32_t* __restrict__ keyc2,
                        int32_t* __restrict__ out_idx, float* __restrict__ out_dist,
                        int32_t* __restrict__ qlist, int32_t* __restrict__ qcount, double ratio) {
    constexpr int GLDS = STAGE * SIFT_DIM / (WAVES * 64 * 16);
    static_assert(GLDS * WAVES * 64 * 16 == STAGE * SIFT_DIM, "stage must split into whole 16-B pieces");
    constexpr int DESC_BYTES = STAGE * SIFT_DIM;
    constexpr int BUF_BYTES = DESC_BYTES + STAGE * 4;
    __shared__ __attribute__((aligned(16))) char lds[2 * BUF_BYTES];

    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    const WorkItem w = work[xcd_remap(blockIdx.x, gridDim.x)];
    const PairDev P = pairs[w.pair];
    const ImgDev L = imgs[P.left], R = imgs[P.right];
    const int nq = L.rows, nt = R.rows;
    const int qbase = w.q0 + wid * (QT * 32);

    i32x4 bq[QT][4];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const i32x4* src = reinterpret_cast<const i32x4*>(desc8 + (L.row0 + qbase + qt * 32 + l32) * SIFT_DIM);
#pragma unroll
        for (int m = 0; m < 4; ++m) bq[qt][m] = src[2 * m + h];
    }
    int ch[QT][8];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int c = 0; c < 8; ++c) ch[qt][c] = INT_MIN;

    const int nstages = (nt + STAGE - 1) / STAGE;
    const int8_t* tbase = desc8 + R.row0 * SIFT_DIM;
    const int32_t* kbase = keyc2 + R.row0;
    auto stage = [&](int s, int buf) {
        char* base = lds + buf * BUF_BYTES;
#pragma unroll
        for (int i = 0; i < GLDS; ++i) {
            const int p = i * WAVES * 64 + threadIdx.x;
            const int rr = p >> 3, slot = p & 7, c = slot ^ ((rr >> 1) & 7);
            const int8_t* g = tbase + (int64_t)(s * STAGE + rr) * SIFT_DIM + 16 * c;
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)g,
                                             (LDS_AS void*)(base + (i * WAVES + wid) * 1024), 16, 0, 0);
        }
        if (wid < STAGE / 64)
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(kbase + s * STAGE + wid * 64 + lane),
                                             (LDS_AS void*)(base + DESC_BYTES + wid * 256), 4, 0, 0);
    };

    if (nstages > 0) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int s = 0; s < nstages; ++s) {
        const int buf = s & 1;
        if (s + 1 < nstages) stage(s + 1, buf ^ 1);
        const char* base = lds + buf * BUF_BYTES;
#pragma unroll
        for (int t = 0; t < STAGE / 32; ++t) {
            const int row = t * 32 + l32;
            i32x4 a[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int slot = (2 * m + h) ^ ((row >> 1) & 7);
                a[m] = *reinterpret_cast<const i32x4*>(base + row * SIFT_DIM + 16 * slot);
            }
            // C operand: keys of rows t*32 + 8g + 4h + (0..3) = accumulator rows 4g..4g+3.
            i32x16 cv;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const i32x4 k4 = *reinterpret_cast<const i32x4*>(base + DESC_BYTES + 4 * (t * 32 + 8 * g + 4 * h));
                cv[4 * g + 0] = k4[0]; cv[4 * g + 1] = k4[1]; cv[4 * g + 2] = k4[2]; cv[4 * g + 3] = k4[3];
            }
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                i32x16 acc = cv;
#pragma unroll
                for (int m = 0; m < 4; ++m) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[m], bq[qt][m], acc, 0, 0, 0);
#pragma unroll
                for (int c = 0; c < 8; ++c) ch[qt][c] = max(max(ch[qt][c], acc[2 * c]), acc[2 * c + 1]);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // Per query: the two largest of the 16 subset maxima (8 per half-wave).
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        int k1 = INT_MIN, k2 = INT_MIN;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int v = ch[qt][c];
            k2 = max(k2, min(k1, v));
            k1 = max(k1, v);
        }
        const int p1 = __shfl_xor(k1, 32), p2 = __shfl_xor(k2, 32);
        const int K2 = max(min(k1, p1), max(k2, p2)), K1 = max(k1, p1);
        const int qi = qbase + qt * 32 + l32;
        if (h != 0 || qi >= nq) continue;
        const int64_t o = P.dense_base + qi;
        if (nt == 0) { out_idx[o] = -1; out_dist[o] = 0.f; continue; }
        bool reject = false;
        if (nt >= 2 && K2 >= KEY_VALID) {
            const int64_t na = norm[L.row0 + qi];
            const int64_t s1 = max<int64_t>(na - 2 * (int64_t)K1 - 1, 0), s2 = na - 2 * (int64_t)K2;
            reject = !((double)sqrt_rn_int(s1) < (double)sqrt_rn_int(s2) * ratio);
        }
        if (reject) {
            out_idx[o] = -1;
            out_dist[o] = 0.f;
        } else {
            const int slot = atomicAdd(&qcount[w.pair], 1);
            qlist[P.dense_base + slot] = qi;
            out_idx[o] = UNSETTLED;   // pass 2 must overwrite it (assemble counts survivors)
        }
    }
}

// Screening pass on v_mfma_i32_16x16x64_i8 (same bounds, same outputs as
// sift_screen_kernel; a second MFMA shape for the clock the chip holds under it).
//   D = A * B, A = 16 train rows (LDS), B = 16 queries (registers), K = 128 = 2 MFMAs.
//   Lane l: A row / B column l & 15, 16 operand bytes of chunk 4m + (l >> 4) (any
//   chunk order is a dot product as long as A and B agree); accumulator rows
//   4 (l >> 4) + i, i = 0..3, of column l & 15.  Two row blocks per step feed one
//   v_max3 per accumulator row i: 4 chains per lane x 4 lanes = 16 disjoint row
//   subsets per query, the same bound as the 32x32 form.
// The persistent screens' item source: XCD x (HW_REG_XCC_ID) owns the contiguous item range
// [x n / 8, (x + 1) n / 8) -- the train-image locality of xcd_remap -- and takes from its own ticket
// counter; an XCD whose range is done steals from the next ones (only the tail leaves its L2).
// ticket[0..8) is zero at launch.  -> item, or -1 when every range is done.
__device__ __forceinline__ int xcd_ticket(int32_t* ticket, int n) {
    const int x0 = (int)(__builtin_amdgcn_s_getreg(0x1814) & 7);   // hwreg(HW_REG_XCC_ID, 0, 4)
    for (int k = 0; k < 8; ++k) {
        const int x = (x0 + k) & 7, b0 = (int)((int64_t)n * x / 8), b1 = (int)((int64_t)n * (x + 1) / 8);
        if (b1 <= b0) continue;
        if (__hip_atomic_load(&ticket[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= b1 - b0) continue;
        const int t = atomicAdd(&ticket[x], 1);
        if (t < b1 - b0) return b0 + t;
    }
    return -1;
}
// PERSIST (r04, diagnostic build only, see persist_screens): a grid of resident workgroup slots takes work items
// from a ticket counter in list order (the last partial round of a one-item-per-workgroup grid --
// C2: 19 600 items on 512 slots, 38.3 rounds -- becomes a ragged end of single items).
// LISTS (with SUBSET; the product path until sift_screen6_kernel, now SIFT_VARIANT_INT8_LISTS): nothing goes to the dense
// per-query arrays.  A rejected query
// leaves no trace, a forwarded one is its list entry alone, and its pass-2 state (top2 / slot1) lives at
// its list slot (dense_base + slot), where sift_subset_kernel<_, true> and sift_finish_kernel find it.
template <int QT, int WAVES, int MINW, int STAGE, bool SUBSET = false, bool PERSIST = false, bool LISTS = false>
__global__ __launch_bounds__(WAVES * 64, MINW)
void sift_screen16_kernel(const WorkItem* __restrict__ work, const PairDev* __restrict__ pairs,
                          const ImgDev* __restrict__ imgs, const int8_t* __restrict__ desc8,
                          const int32_t* __restrict__ norm, const int32_t* __restrict__ keyc2,
                          int32_t* __restrict__ out_idx, float* __restrict__ out_dist,
                          int32_t* __restrict__ qlist, int32_t* __restrict__ qcount, double ratio,
                          int32_t* __restrict__ qmask = nullptr, unsigned long long* __restrict__ top2 = nullptr,
                          int32_t* __restrict__ ticket = nullptr, int n_work = 0) {
    constexpr int GLDS = STAGE * SIFT_DIM / (WAVES * 64 * 16);
    static_assert(GLDS * WAVES * 64 * 16 == STAGE * SIFT_DIM, "stage must split into whole 16-B pieces");
    static_assert(QT * WAVES * 16 == 512, "work items are 512 queries");
    constexpr int DESC_BYTES = STAGE * SIFT_DIM;
    constexpr int BUF_BYTES = DESC_BYTES + STAGE * 4;
    __shared__ __attribute__((aligned(16))) char lds[2 * BUF_BYTES];

    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
    __shared__ int item_sh;
    for (int round = 0;; ++round) {
    int wi;
    if constexpr (PERSIST) {
        if (threadIdx.x == 0) item_sh = xcd_ticket(ticket, n_work);
        __syncthreads();
        wi = item_sh;
        if (wi < 0) break;
    } else {
        if (round > 0) break;
        wi = xcd_remap(blockIdx.x, gridDim.x);
    }
    const WorkItem w = work[wi];
    const PairDev P = pairs[w.pair];
    const ImgDev L = imgs[P.left], R = imgs[P.right];
    const int nq = L.rows, nt = R.rows;
    const int qbase = w.q0 + wid * (QT * 16);

    i32x4 bq[QT][2];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const i32x4* src = reinterpret_cast<const i32x4*>(desc8 + (L.row0 + qbase + qt * 16 + l16) * SIFT_DIM);
#pragma unroll
        for (int m = 0; m < 2; ++m) bq[qt][m] = src[4 * m + g];
    }
    int ch[QT][4];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int i = 0; i < 4; ++i) ch[qt][i] = INT_MIN;

    const int nstages = (nt + STAGE - 1) / STAGE;
    const int8_t* tbase = desc8 + R.row0 * SIFT_DIM;
    const int32_t* kbase = keyc2 + R.row0;
    auto stage = [&](int s, int buf) {
        char* base = lds + buf * BUF_BYTES;
#pragma unroll
        for (int i = 0; i < GLDS; ++i) {
            const int p = i * WAVES * 64 + threadIdx.x;
            const int rr = p >> 3, slot = p & 7, c = slot ^ ((rr >> 1) & 7);
            const int8_t* gp = tbase + (int64_t)(s * STAGE + rr) * SIFT_DIM + 16 * c;
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)gp,
                                             (LDS_AS void*)(base + (i * WAVES + wid) * 1024), 16, 0, 0);
        }
        if (wid < STAGE / 64)
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(kbase + s * STAGE + wid * 64 + lane),
                                             (LDS_AS void*)(base + DESC_BYTES + wid * 256), 4, 0, 0);
    };

    if (nstages > 0) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int s = 0; s < nstages; ++s) {
        const int buf = s & 1;
        if (s + 1 < nstages) stage(s + 1, buf ^ 1);
        const char* base = lds + buf * BUF_BYTES;
#pragma unroll
        for (int t = 0; t < STAGE / 32; ++t) {
            i32x4 a[2][2], cv[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int row = t * 32 + b * 16 + l16;
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int slot = (4 * m + g) ^ ((row >> 1) & 7);
                    a[b][m] = *reinterpret_cast<const i32x4*>(base + row * SIFT_DIM + 16 * slot);
                }
                cv[b] = *reinterpret_cast<const i32x4*>(base + DESC_BYTES + 4 * (t * 32 + b * 16 + 4 * g));
            }
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                i32x4 acc0 = cv[0], acc1 = cv[1];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    acc0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[0][m], bq[qt][m], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[1][m], bq[qt][m], acc1, 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) ch[qt][i] = max(max(ch[qt][i], acc0[i]), acc1[i]);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        int k1 = INT_MIN, k2 = INT_MIN;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = ch[qt][i];
            k2 = max(k2, min(k1, v));
            k1 = max(k1, v);
        }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const int p1 = __shfl_xor(k1, o), p2 = __shfl_xor(k2, o);
            k2 = max(min(k1, p1), max(k2, p2));
            k1 = max(k1, p1);
        }
        // SUBSET: the row subsets (j mod 16 = 4g + i) whose maximum reaches k2; only they can hold
        // the first or second neighbour (a row of a subset with K <= k2 - 1 has s >= na - 2 k2 + 1 > s2)
        int mask = 0xFFFF;
        if constexpr (SUBSET) {
            int nib = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) nib |= (ch[qt][i] >= k2 ? 1 : 0) << i;
            int mk = nib << (4 * g);
            mk |= __shfl_xor(mk, 16);
            mk |= __shfl_xor(mk, 32);
            if (nt >= 2 && k2 >= KEY_VALID) mask = mk;
        }
        const int qi = qbase + qt * 16 + l16;
        if (g != 0 || qi >= nq) continue;
        const int64_t o = P.dense_base + qi;
        if (nt == 0) {
            if constexpr (!LISTS) { out_idx[o] = -1; out_dist[o] = 0.f; }
            continue;
        }
        bool reject = false;
        if (nt >= 2 && k2 >= KEY_VALID) {
            const int64_t na = norm[L.row0 + qi];
            const int64_t s1 = max<int64_t>(na - 2 * (int64_t)k1 - 1, 0), s2 = na - 2 * (int64_t)k2;
            reject = !((double)sqrt_rn_int(s1) < (double)sqrt_rn_int(s2) * ratio);
        }
        if (reject) {
            if constexpr (!LISTS) { out_idx[o] = -1; out_dist[o] = 0.f; }
        } else {
            const int slot = atomicAdd(&qcount[w.pair], 1);
            qlist[P.dense_base + slot] = qi;
            if constexpr (SUBSET) {
                qmask[P.dense_base + slot] = mask;
                // a two-subset mask: both 16-B words are written whole by plain stores (sift_subset_kernel)
                const int64_t t = LISTS ? P.dense_base + slot : o;
                if (!LISTS || __popc(mask) != 2) {
                    top2[2 * t] = ~0ull;
                    top2[2 * t + 1] = ~0ull;
                }
            }
            if constexpr (!LISTS) out_idx[o] = UNSETTLED;   // pass 2 must overwrite it (assemble counts survivors)
        }
    }
    __syncthreads();   // the next item restages the LDS buffers and rewrites item_sh
    }
}

// The screen's decision for one query from its two largest subset maxima k1 >= k2 and k1's row subset r1
// (both forms of the FP6 screen): rejected, or appended to the pair's list with its pass-2 route.
template <bool CERT>
__device__ __forceinline__ void screen6_forward(float k1, float k2, int r1, int qi, int nt, int2 q2, int emax2, int amax2,
                                                double ratio, int pair, int64_t dense_base, int32_t* __restrict__ qlist,
                                                int32_t* __restrict__ qcount, int32_t* __restrict__ qmask,
                                                unsigned long long* __restrict__ top2, int32_t* __restrict__ qlist2,
                                                int32_t* __restrict__ qcount2) {
    // straight-line integer arithmetic decides (lowe_select: no bool PHI): the bound is usable with two
    // train rows in two different subsets, every other query is forwarded
    const int usable = (int)(nt >= 2) & (int)(k2 > fp6::KEY_VALID);
    const int rej = usable & fp6::certainly_rejected(k1, k2, q2.x, q2.y, emax2, amax2, ratio);
    if (rej == 0) {
        const int64_t slot = dense_base + atomicAdd(&qcount[pair], 1);
        qlist[slot] = qi;
        if constexpr (CERT) {
            const int cert = fp6::certified(k1, k2, r1, nt, q2.x, q2.y, emax2, amax2, ratio);
            qmask[slot] = cert ? 1 << r1 : QMASK_FULL_ROUTE;
            if (!cert) qlist2[dense_base + atomicAdd(&qcount2[pair], 1)] = (int32_t)(slot - dense_base);
        } else {
            qmask[slot] = 0xFFFF;   // not a two-bit mask: sift_finish_kernel reads the slot's own two keys
        }
        top2[2 * slot] = ~0ull;   // pass 2 overwrites both (a slot it misses counts as unsettled)
        top2[2 * slot + 1] = ~0ull;
    }
}

// LDS stage of the FP6 screens (STAGE train rows: plane A | plane B | keys, the layout described at
// sift_screen6_kernel) filled by 16-B LDS-DMA through two buffer resources, one over the train image's padded
// packed rows and one over its keys.  Everything that changes from stage to stage is wave-uniform, so a lane's
// byte offsets (swizzle included: a stage is a multiple of 16 rows, the period of fp6::swz_a / swz_b) are
// computed once, and the stage advance goes into the instruction's scalar offset: no vector instruction per
// stage.  The range check of the resources ends at the image's padded rows.
template <int STAGE>
struct Screen6Stage {
    static constexpr int WAVES = 4;
    static constexpr int A_BYTES = STAGE * 64, B_BYTES = STAGE * 32;
    static constexpr int GA = A_BYTES / (WAVES * 64 * 16), GB = B_BYTES / (WAVES * 64 * 16), GK = STAGE / 64;
    static constexpr int BUF_BYTES = A_BYTES + B_BYTES + STAGE * 4;
    static_assert(STAGE % 128 == 0 && ROW_ALIGN % STAGE == 0, "whole DMA instructions per wave; stages inside the padded rows");
    __amdgpu_buffer_rsrc_t rows, keys;
    int va, vb, vk;   // per-lane byte offsets of the lane's plane-A piece, plane-B piece and key inside a stage
    int wid;          // wave of the workgroup, in a scalar register

    __device__ __forceinline__ Screen6Stage(const uint32_t* __restrict__ desc6, const float* __restrict__ keyf, const ImgDev& R) {
        const int tid = threadIdx.x;
        wid = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int ra = tid >> 2, rb = tid >> 1;   // instruction i adds 64 (A) / 128 (B) rows: the swizzles do not change
        va = ra * fp6::ROW_BYTES + 16 * ((tid & 3) ^ fp6::swz_a(ra));
        vb = rb * fp6::ROW_BYTES + 64 + 16 * ((tid & 1) ^ fp6::swz_b(rb));
        vk = (tid & 63) * 4;
        rows = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(desc6 + R.row0 * fp6::ROW_WORDS), 0,
                                                 R.rows_pad * fp6::ROW_BYTES, 0x00020000);
        keys = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(keyf + R.row0), 0, R.rows_pad * 4, 0x00020000);
    }
    // stage s of the image into buffer `buf` of `lds` (2 x BUF_BYTES)
    __device__ __forceinline__ void issue(char* lds, int s, int buf) const {
        char* base = lds + buf * BUF_BYTES;
        const int row0 = s * STAGE;
#pragma unroll
        for (int i = 0; i < GA; ++i)   // plane A: 4 pieces per row, 64 rows per instruction
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rows, (LDS_AS void*)(base + (i * WAVES + wid) * 1024), 16, va,
                                                     (row0 + i * 64) * fp6::ROW_BYTES, 0, 0);
#pragma unroll
        for (int i = 0; i < GB; ++i)   // plane B: 2 pieces per row, 128 rows per instruction
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rows, (LDS_AS void*)(base + A_BYTES + (i * WAVES + wid) * 1024), 16, vb,
                                                     (row0 + i * 128) * fp6::ROW_BYTES, 0, 0);
        if (wid < GK)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(keys, (LDS_AS void*)(base + A_BYTES + B_BYTES + wid * 256), 4, vk,
                                                     (row0 + wid * 64) * 4, 0, 0);
    }
};

// ---------------------------------------------------------------------------
// Screening pass of the product path on the FP6 matrix pipe: v_mfma_f32_16x16x128_f8f6f4 (unscaled, fp6::mfma16) with e2m3
// operands, one MFMA (K = 128) per 16 x 16 tile, twice the MACs per clock of the int8 screens.  The
// operands are quantised, so the screen is conservative rather than exact (sift_fp6.hpp: quantiser, key,
// bound and its proof): it rejects a query only when Lowe's test fails at a lower bound of s1 and an upper
// bound of s2, and forwards every other one -- a superset of what sift_screen16_kernel forwards -- to the
// exact pass 2 (sift_knn2_kernel<GATHER, LISTS>), whose results do not depend on which rejected queries
// were forwarded as well.  The bound is too wide to name the subsets that can hold the second neighbour,
// but for most forwarded queries it does name the subset of the first one and shows that no row outside
// it can decide Lowe's test (fp6::certified).  CERT: such a query gets the one-bit mask of that subset,
// and the exact top-2 of the subset alone settles it (sift_subset_kernel<_, true>, sift_finish_kernel);
// every other forwarded query gets QMASK_FULL_ROUTE and its slot is appended to the pair's second list
// (`qlist2`, counted in `qcount2`), which the full-row pass 2 gathers through (sift_knn2_kernel<VIA>).
// Without CERT (SIFT_VARIANT_FP6_FULL) every forwarded query carries the full mask and pass 2 scans
// every train row for it.
//   Loop structure of orb_screen16_kernel: A = 16 train rows (LDS), B = 16 queries (registers), the f32 C
//   operand is the row's key, v_max3_f32 folds two row blocks into 4 chains per lane (16 row subsets per
//   query with the other three lanes of the column).
//   LDS stage: plane A (64 B per row: the first 16 B of each lane group's 24-B fragment) | plane B (32 B
//   per row: the last 8 B) | keys, filled by 16-B LDS-DMA from the 96-B rows with the swizzle on the
//   source address (fp6::swz_a / swz_b keep ds_read_b128 / ds_read_b64 conflict-free in their lane groups).
template <int QT, int WAVES, int MINW, int STAGE, bool CERT>
__global__ __launch_bounds__(WAVES * 64, MINW)
void sift_screen6_kernel(const WorkItem* __restrict__ work, const PairDev* __restrict__ pairs,
                         const ImgDev* __restrict__ imgs, const uint32_t* __restrict__ desc6,
                         const float* __restrict__ keyf, const int2* __restrict__ ne,
                         const int32_t* __restrict__ imax,
                         int32_t* __restrict__ qlist, int32_t* __restrict__ qcount, double ratio,
                         int32_t* __restrict__ qmask, unsigned long long* __restrict__ top2,
                         int32_t* __restrict__ qlist2, int32_t* __restrict__ qcount2) {
    static_assert(QT * WAVES * 16 == 512, "work items are 512 queries");
    using Stage = Screen6Stage<STAGE>;
    static_assert(WAVES == Stage::WAVES, "whole DMA instructions per wave");
    constexpr int A_BYTES = Stage::A_BYTES, B_BYTES = Stage::B_BYTES, BUF_BYTES = Stage::BUF_BYTES;
    __shared__ __attribute__((aligned(16))) char lds[2 * BUF_BYTES];

    const int lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
    const WorkItem w = work[xcd_remap(blockIdx.x, gridDim.x)];
    const PairDev P = pairs[w.pair];
    const ImgDev L = imgs[P.left], R = imgs[P.right];
    const int nq = L.rows, nt = R.rows;
    const Stage stager(desc6, keyf, R);
    const int wid = stager.wid;
    const int qbase = w.q0 + wid * (QT * 16);

    // Query fragments (B operand): lane group g's 192 bits of the row (fp6::word_index)
    i32x8 bq[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const uint32_t* src = desc6 + (L.row0 + qbase + qt * 16 + l16) * fp6::ROW_WORDS;   // rows < rows_pad
        const i32x4 lo = *reinterpret_cast<const i32x4*>(src + 4 * g);
        const int2 hi = *reinterpret_cast<const int2*>(src + 16 + 2 * g);
        bq[qt] = i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, 0, 0};
    }
    float ch[QT][4];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int i = 0; i < 4; ++i) ch[qt][i] = fp6::KEY_INIT;

    const int nstages = (nt + STAGE - 1) / STAGE;
    // The lane's LDS reads: row block (t, b) is rows 16 (2 t + b) + l16, and the swizzles have a period of 16 rows,
    // so a lane reads at three bases computed once (plane A, plane B, keys) plus a compile-time offset per
    // buffer and row block, which goes into the ds_read offset field.
    const char* ra = lds + l16 * 64 + 16 * (g ^ fp6::swz_a(l16));
    const char* rb = lds + A_BYTES + l16 * 32 + 16 * ((g >> 1) ^ fp6::swz_b(l16)) + 8 * (g & 1);
    const char* rk = lds + A_BYTES + B_BYTES + 16 * g;
    static_assert(fp6::swz_a(16) == fp6::swz_a(0) && fp6::swz_b(16) == fp6::swz_b(0), "swizzle period of 16 rows");

    if (nstages > 0) stager.issue(lds, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int s = 0; s < nstages; ++s) {
        const int buf = s & 1;
        if (s + 1 < nstages) stager.issue(lds, s + 1, buf ^ 1);
        // the buffer select is wave-uniform: one add per base and stage
        const char *pa = ra + buf * BUF_BYTES, *pb = rb + buf * BUF_BYTES, *pk = rk + buf * BUF_BYTES;
#pragma unroll
        for (int t = 0; t < STAGE / 32; ++t) {
            i32x8 a[2];
            f32x4 cinit[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int blk = 2 * t + b;   // 16-row block of the stage
                const i32x4 lo = *reinterpret_cast<const i32x4*>(pa + blk * 16 * 64);
                // (volatile: one ds_read_b64 per fragment.  Merged into ds_read2st64_b64, the two row blocks' halves
                // land in one register quad and cost four v_mov_b32 per 32 rows to reach their fragments.)
                const long long hi = *(const volatile LDS_AS long long*)(pb + blk * 16 * 32);
                a[b] = i32x8{lo.x, lo.y, lo.z, lo.w, (int)hi, (int)(hi >> 32), 0, 0};
                cinit[b] = *reinterpret_cast<const f32x4*>(pk + blk * 16 * 4);
            }
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                // e2m3 for both operands, the unit-scale product (fp6::mfma16)
                const f32x4 acc0 = fp6::mfma16<fp6::FMT_E2M3, false>(a[0], bq[qt], cinit[0]);
                const f32x4 acc1 = fp6::mfma16<fp6::FMT_E2M3, false>(a[1], bq[qt], cinit[1]);
                // (folding one tile behind, the folds pinned under the next tile's MFMAs, measured slower: DESIGN 5)
#pragma unroll
                for (int i = 0; i < 4; ++i) ch[qt][i] = fmaxf(fmaxf(ch[qt][i], acc0[i]), acc1[i]);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    const int emax2 = imax[2 * P.right], amax2 = imax[2 * P.right + 1];
    // After the two shuffle rounds every lane group holds a tile's (k1, k2, r1), so lane group g decides tile
    // 4 p + g: two passes of the decision (square roots in double, the certificate, the list atomics) with 64
    // queries each instead of eight passes with 16 active lanes.
    static_assert(QT % 4 == 0, "four tiles per decision pass");
    float kk1[4] = {}, kk2[4] = {};
    int rr1[4] = {};
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        float k1 = fp6::KEY_INIT, k2 = fp6::KEY_INIT;
        int r1 = 4 * g;   // the row subset of k1: chain i of lane group g holds rows j = 4 g + i (mod 16)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float v = ch[qt][i];
            if constexpr (CERT) r1 = v > k1 ? 4 * g + i : r1;
            k2 = fmaxf(k2, fminf(k1, v));
            k1 = fmaxf(k1, v);
        }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float p1 = __shfl_xor(k1, o), p2 = __shfl_xor(k2, o);
            if constexpr (CERT) {   // (equal maxima: either subset; k1 == k2 is never certified)
                const int pr = __shfl_xor(r1, o);
                r1 = p1 > k1 ? pr : r1;
            }
            k2 = fmaxf(fminf(k1, p1), fmaxf(k2, p2));
            k1 = fmaxf(k1, p1);
        }
        kk1[qt & 3] = k1; kk2[qt & 3] = k2; rr1[qt & 3] = r1;
        if ((qt & 3) != 3) continue;
        k1 = kk1[0]; k2 = kk2[0]; r1 = rr1[0];
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            k1 = g == j ? kk1[j] : k1;
            k2 = g == j ? kk2[j] : k2;
            r1 = g == j ? rr1[j] : r1;
        }
        const int qi = qbase + ((qt & ~3) + g) * 16 + l16;
        if (qi >= nq || nt == 0) continue;   // an empty train image: no neighbour, nothing to forward
        screen6_forward<CERT>(k1, k2, r1, qi, nt, ne[L.row0 + qi], emax2, amax2, ratio, w.pair, P.dense_base, qlist, qcount,
                              qmask, top2, qlist2, qcount2);
    }
}

// The same screen on v_mfma_f32_32x32x64_f8f6f4: two chained MFMAs (K = 64 each, the second takes the
// first one's result as its C operand) per tile of 32 train rows x 32 queries, half the MFMA instructions
// of the 16 x 16 form for the same products and the same 8 v_max3_f32 per tile.  Lane l owns query column
// l & 31 and K-half h = l >> 5 (sift_fp6.hpp: fragments, accumulator rows, chains and LDS reads of this
// form).  The 16 accumulator registers of a lane fold into 8 chains per query tile; the row subsets stay
// "train row j mod 16", so everything behind the screen is the same.  A work item is 4 waves x 4 query
// tiles of 32; the stage, its LDS-DMA fill and the rows in HBM are those of sift_screen6_kernel.
// Fewer issue cycles but a lower held clock: 2.6 % slower on the step than the 16 x 16 form, which
// stays the product; this one is SFMX_SIFT_VARIANT=112 of the diagnostic build.
template <int WAVES, int MINW, int STAGE, bool CERT>
__global__ __launch_bounds__(WAVES * 64, MINW)
void sift_screen6w_kernel(const WorkItem* __restrict__ work, const PairDev* __restrict__ pairs,
                          const ImgDev* __restrict__ imgs, const uint32_t* __restrict__ desc6,
                          const float* __restrict__ keyf, const int2* __restrict__ ne,
                          const int32_t* __restrict__ imax,
                          int32_t* __restrict__ qlist, int32_t* __restrict__ qcount, double ratio,
                          int32_t* __restrict__ qmask, unsigned long long* __restrict__ top2,
                          int32_t* __restrict__ qlist2, int32_t* __restrict__ qcount2) {
    constexpr int QT = 4;
    static_assert(QT * WAVES * 32 == 512, "work items are 512 queries");
    using Stage = Screen6Stage<STAGE>;   // the stage and its fill of sift_screen6_kernel
    static_assert(WAVES == Stage::WAVES, "whole DMA instructions per wave");
    constexpr int BUF_BYTES = Stage::BUF_BYTES;
    __shared__ __attribute__((aligned(16))) char lds[2 * BUF_BYTES];

    const int lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    const WorkItem w = work[xcd_remap(blockIdx.x, gridDim.x)];
    const PairDev P = pairs[w.pair];
    const ImgDev L = imgs[P.left], R = imgs[P.right];
    const int nq = L.rows, nt = R.rows;
    const Stage stager(desc6, keyf, R);
    const int wid = stager.wid;
    const int qbase = w.q0 + wid * (QT * 32);

    // Query fragments (B operand): fragment frag32(m, h) of the row for MFMA m
    i32x8 bq[QT][2];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const uint32_t* src = desc6 + (L.row0 + qbase + qt * 32 + l32) * fp6::ROW_WORDS;   // rows < rows_pad
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int f = fp6::frag32(m, h);
            const i32x4 lo = *reinterpret_cast<const i32x4*>(src + fp6::word_index(f, 0));
            const int2 hi = *reinterpret_cast<const int2*>(src + fp6::word_index(f, 4));
            bq[qt][m] = i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, 0, 0};
        }
    }
    float ch[QT][8];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int c = 0; c < 8; ++c) ch[qt][c] = fp6::KEY_INIT;

    const int nstages = (nt + STAGE - 1) / STAGE;
    if (nstages > 0) stager.issue(lds, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int s = 0; s < nstages; ++s) {
        const int buf = s & 1;
        if (s + 1 < nstages) stager.issue(lds, s + 1, buf ^ 1);
        const char* base = lds + buf * BUF_BYTES;
#pragma unroll
        for (int t = 0; t < STAGE / 32; ++t) {
            i32x8 a[2];
            f32x16 key;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int f = fp6::frag32(m, h), row = t * 32 + l32;
                const i32x4 lo = *reinterpret_cast<const i32x4*>(base + fp6::lds_a32(row, f));
                const int2 hi = *reinterpret_cast<const int2*>(base + fp6::lds_b32(STAGE, row, f));
                a[m] = i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, 0, 0};
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {   // registers 4 k .. 4 k + 3: rows 8 k + 4 h .. + 3 of the block (fp6::acc_row32)
                const f32x4 kv = *reinterpret_cast<const f32x4*>(base + fp6::lds_key32(STAGE, t * 32, k, h));
                key[4 * k + 0] = kv.x; key[4 * k + 1] = kv.y; key[4 * k + 2] = kv.z; key[4 * k + 3] = kv.w;
            }
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                // e2m3 for both operands, the unit-scale product (fp6::mfma32)
                f32x16 acc = fp6::mfma32<fp6::FMT_E2M3, false>(a[0], bq[qt][0], key);
                acc = fp6::mfma32<fp6::FMT_E2M3, false>(a[1], bq[qt][1], acc);
#pragma unroll
                for (int c = 0; c < 8; ++c) ch[qt][c] = fmaxf(fmaxf(ch[qt][c], acc[c]), acc[c + 8]);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    const int emax2 = imax[2 * P.right], amax2 = imax[2 * P.right + 1];
    float kk1[2] = {}, kk2[2] = {};
    int rr1[2] = {};
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        float k1 = fp6::KEY_INIT, k2 = fp6::KEY_INIT;
        int r1 = fp6::chain_subset32(0, h);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float v = ch[qt][c];
            if constexpr (CERT) r1 = v > k1 ? fp6::chain_subset32(c, h) : r1;
            k2 = fmaxf(k2, fminf(k1, v));
            k1 = fmaxf(k1, v);
        }
        {   // the other K-half's 8 subsets (equal maxima: either subset; k1 == k2 is never certified)
            const float p1 = __shfl_xor(k1, 32), p2 = __shfl_xor(k2, 32);
            if constexpr (CERT) {
                const int pr = __shfl_xor(r1, 32);
                r1 = p1 > k1 ? pr : r1;
            }
            k2 = fmaxf(fminf(k1, p1), fmaxf(k2, p2));
            k1 = fmaxf(k1, p1);
        }
        // after the shuffle both halves hold the tile's (k1, k2, r1): half h decides tile 2 p + h, 64 queries a pass
        kk1[qt & 1] = k1; kk2[qt & 1] = k2; rr1[qt & 1] = r1;
        if ((qt & 1) != 1) continue;
        k1 = h ? k1 : kk1[0]; k2 = h ? k2 : kk2[0]; r1 = h ? r1 : rr1[0];
        const int qi = qbase + ((qt & ~1) + h) * 32 + l32;
        if (qi >= nq || nt == 0) continue;   // an empty train image: no neighbour, nothing to forward
        screen6_forward<CERT>(k1, k2, r1, qi, nt, ne[L.row0 + qi], emax2, amax2, ratio, w.pair, P.dense_base, qlist, qcount,
                              qmask, top2, qlist2, qcount2);
    }
}

// ---------------------------------------------------------------------------
// Pass 2, subset form (SFMX_SIFT_P2 = 10): one workgroup per (pair, row subset r), r = j mod 16.
// The screen forwarded each unsettled query with the mask of the subsets whose maximum reaches
// its second-largest subset maximum; only rows of those subsets can be the first or second
// neighbour (sift_screen16_kernel), typically 2 of 16.  The workgroup gathers the pair's forwarded
// queries with bit r, stages subset r's rows (j = r + 16 i, 256 per LDS chunk, the 8-bit local
// index i & 255 in the packed key) and runs the exact top-2 of sift_knn2_kernel on them
// (v_mfma_i32_32x32x32_i8, packed keys, 32 queries per wave).
//
// The kernel is bound by its chain of memory round trips and by its atomics, not by its MFMAs.
// Nothing in the staging depends on the query list, so chunk 0's LDS-DMA and the norms of its rows
// are issued at entry: the gather and the query-row loads run under them, and the chunk's keys are
// formed from norms that arrived with the rows (no second, dependent load).
//
// Merge: each (query, subset) top-2 k1 <= k2, key = (s << 32) | j, i.e. (distance, train index)
// order, goes into the query's global pair (b0, b1), both ~0 before pass 2:
//       old = atomicMin(b0, k1);  atomicMin(b1, max(old, k1));  atomicMin(b1, k2).
// Invariant: b0 and b1 end as the two smallest keys inserted, in any arrival order.  b0 is the
// minimum of every k1, hence of every key, since each k2 has its own k1 <= k2 below it.  The
// atomics on b0 are serialised: every k1 but the smallest either finds b0 <= k1 and sends itself to
// b1, or displaces an `old` that goes to b1, and the smallest k1 is never sent to b1 (it is never
// displaced and displaces whatever it finds), so the k1 steps alone leave b1 = the second smallest
// k1.  The second smallest key overall is the smaller of that and the smallest k2 (the k2 of
// another insertion has its own k1 at or below it among the other k1), which is what reaches b1.
// A k2 never needs the exchange on b0: k2 >= k1 >= b0 from the moment k1 is inserted, and the
// minimum on b1 commutes with everything else, so it need not wait for k1's atomics either.
// sift_settle_kernel reads (b0, b1).
//
// Most forwarded queries have exactly two flagged subsets.  Those need no atomics at all: the
// lower subset's workgroup stores its (k1, k2) as one 16-B word over the query's pair in `top2`,
// the upper one's into the same place of `slot1` (the matcher's packed output buffer, idle until
// assembly), ~0 for a missing key, and sift_settle_kernel, which sees the same mask, merges the
// two top-2.  Both workgroups exist and write: a mask of two bits comes from two subset maxima
// that are real rows (r < nt), and the query is in its pair's list (cnt > 0).  The workgroup then
// ends on plain stores instead of waiting for a returning atomic.  Every other mask (3+ subsets,
// or all 16 when the screen's bound was not usable) takes the atomics above.
//
// LISTS (the list path of SIFT_VARIANT_INT8_LISTS): the query's pass-2 state lives at its list slot, dense_base + e, not at
// its row: the gather carries e (16 bits, relative to the window) beside the packed row | mode, and
// sift_finish_kernel walks the same slots in order instead of two scattered 16-B reads per query.
template <int WAVES, bool LISTS = false>
__global__ __launch_bounds__(WAVES * 64, 2)
void sift_subset_kernel(const PairDev* __restrict__ pairs, const ImgDev* __restrict__ imgs,
                        const int8_t* __restrict__ desc8, const int32_t* __restrict__ norm,
                        const int32_t* __restrict__ qlist, const int32_t* __restrict__ qmask,
                        const int32_t* __restrict__ qcount, const int32_t* __restrict__ porder,
                        unsigned long long* __restrict__ top2, unsigned long long* __restrict__ slot1,
                        const int32_t* __restrict__ qcount2 = nullptr, int ride = 0) {
    constexpr int CH = 256;                   // rows per LDS chunk
    constexpr int QC = WAVES * 32;            // queries per tile group (one 32-query tile per wave)
    constexpr int WIN = 1024;                 // forwarded-query window scanned per round
    constexpr int GLDS = CH * SIFT_DIM / (WAVES * 64 * 16);
    static_assert(GLDS * WAVES * 64 * 16 == CH * SIFT_DIM, "chunk must split into whole 16-B pieces");
    static_assert(WAVES * 64 == CH, "one thread per chunk row loads its norm");
    __shared__ __attribute__((aligned(16))) char rows_lds[CH * SIFT_DIM];
    __shared__ int keys_lds[CH];
    __shared__ int ql[WIN];
    __shared__ unsigned short qs[LISTS ? WIN : 2];   // LISTS: the entry's list slot, relative to the window
    __shared__ int s_n;
    // four workgroups per CU (160 KB of LDS), as the 128-VGPR bound of four waves per SIMD allows
    static_assert(sizeof(rows_lds) + sizeof(keys_lds) + sizeof(ql) + sizeof(qs) + sizeof(s_n) <= 160 * 1024 / 4,
                  "pass-2 LDS must leave four workgroups resident per CU");

    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63, h = lane >> 5, l32 = lane & 31;
    const int item = xcd_remap(blockIdx.x, gridDim.x);
    const int pi = porder[item >> 4], r = item & 15;
    const int cnt = qcount[pi];
    const PairDev P = pairs[pi];
    const ImgDev L = imgs[P.left], R = imgs[P.right];
    const int nt = R.rows;
    const int nr = R.rows_pad >> 4;           // rows j = r + 16 i < rows_pad (pad rows are zero)
    if (cnt == 0 || r >= nt) return;
    const int32_t* qls = qlist + P.dense_base;
    const int32_t* qms = qmask + P.dense_base;
    // FP6 product path: a pair with at most `ride` queries on the full-row route gets no full-row item
    // (compact_work_kernel); every subset's workgroup takes them as if their mask had all 16 bits
    const bool riders = LISTS && qcount2 != nullptr && qcount2[pi] <= ride;

    // Chunk c0's rows (XOR-swizzled 16-B pieces; rows past the subset's end are clamped to the
    // chunk's first row, so every address lies in the image's padded rows) -> LDS by DMA;
    // returns the norm of this thread's row of the chunk.
    auto stage = [&](int c0, int rows) -> int {
#pragma unroll
        for (int u = 0; u < GLDS; ++u) {
            const int p = u * WAVES * 64 + tid;
            const int rr = p >> 3, slot = p & 7, c = slot ^ ((rr >> 1) & 7);
            const int j = r + 16 * (c0 + (rr < rows ? rr : 0));
            const int8_t* gp = desc8 + (R.row0 + j) * SIFT_DIM + 16 * c;
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)gp,
                                             (LDS_AS void*)(rows_lds + (u * WAVES + wid) * 1024), 16, 0, 0);
        }
        return norm[R.row0 + r + 16 * (c0 + (tid < rows ? tid : 0))];
    };
    int nv = stage(0, min(CH, nr));           // nr >= 32: r < nt
    int cur = 0;                              // the chunk in (or on its way into) the LDS
    bool fresh = true;                        // its keys are not written yet

    for (int e0 = 0; e0 < cnt; e0 += WIN) {
        if (tid == 0) s_n = 0;
        __syncthreads();
        for (int e = e0 + tid; e < min(cnt, e0 + WIN); e += WAVES * 64) {
            int mk = qms[e];
            if constexpr (LISTS) mk = riders && mk == QMASK_FULL_ROUTE ? 0xFFFF : mk;
            if ((mk >> r) & 1) {   // query row (< 2^18) | merge mode << 20: 0 atomics, 1 / 2 the lower / upper of two subsets
                // (a one-bit mask, the FP6 screen's certified subset, takes the atomics too: its single writer
                // could store plainly, which measured no faster)
                const int mode = __popc(mk) == 2 ? ((mk & ((1 << r) - 1)) ? 2 : 1) : 0;
                const int at = atomicAdd(&s_n, 1);
                ql[at] = qls[e] | (mode << 20);
                if constexpr (LISTS) qs[at] = (unsigned short)(e - e0);
            }
        }
        __syncthreads();
        const int n = s_n;
        for (int g0 = 0; g0 < n; g0 += QC) {
            const int qe = g0 + wid * 32 + l32;
            const int qpk = qe < n ? ql[qe] : -1;
            const int qrow = qpk < 0 ? -1 : (qpk & 0xFFFFF), mode = qpk < 0 ? 0 : (qpk >> 20);
            int qslot = qrow;          // where the query's pass-2 state lives: its row, or (LISTS) its list slot
            if constexpr (LISTS) qslot = qe < n ? e0 + qs[qe] : 0;
            const bool active = g0 + wid * 32 < n;   // wave-uniform
            const int64_t lrow = L.row0 + (qrow < 0 ? 0 : qrow);
            i32x4 bq[4];
            {
                const i32x4* src = reinterpret_cast<const i32x4*>(desc8 + lrow * SIFT_DIM);
#pragma unroll
                for (int m = 0; m < 4; ++m) bq[m] = src[2 * m + h];
            }
            const long long na = norm[lrow];
            int T1 = INT_MAX, J1 = -1, T2 = INT_MAX, J2 = -1;
            for (int c0 = 0; c0 < nr; c0 += CH) {
                const int rows = min(CH, nr - c0);   // a multiple of 32
                if (cur != c0) {                     // (a one-chunk subset stays staged for every group)
                    __syncthreads();                 // the previous chunk's readers are done
                    nv = stage(c0, rows);
                    cur = c0;
                    fresh = true;
                }
                if (fresh) keys_lds[tid] = (tid < rows && r + 16 * (c0 + tid) < nt) ? (-(nv << 8) + 255 - tid) : INT_MIN;
                fresh = false;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (active) {
                    int c1 = INT_MIN, c2 = INT_MIN;
                    for (int t = 0; t < rows / 32; ++t) {
                        const int row = t * 32 + l32;
                        i32x4 a[4];
#pragma unroll
                        for (int m = 0; m < 4; ++m) {
                            const int slot = (2 * m + h) ^ ((row >> 1) & 7);
                            a[m] = *reinterpret_cast<const i32x4*>(rows_lds + row * SIFT_DIM + 16 * slot);
                        }
                        i32x4 kv[4];
#pragma unroll
                        for (int g = 0; g < 4; ++g) kv[g] = *reinterpret_cast<const i32x4*>(keys_lds + t * 32 + 8 * g + 4 * h);
                        i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                        for (int m = 0; m < 4; ++m) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[m], bq[m], acc, 0, 0, 0);
                        int mm[8];
#pragma unroll
                        for (int q = 0; q < 16; q += 2) {
                            const int ka = (int)(((unsigned)acc[q] << 9) + (unsigned)kv[q >> 2][q & 3]);
                            const int kb = (int)(((unsigned)acc[q + 1] << 9) + (unsigned)kv[q >> 2][(q + 1) & 3]);
                            mm[q >> 1] = v_med3(c1, ka, kb);
                            c1 = v_max3(c1, ka, kb);
                        }
                        c2 = v_max3(v_max3(mm[0], mm[1], mm[2]), v_max3(mm[3], mm[4], mm[5]), v_max3(mm[6], mm[7], c2));
                    }
                    const int p1 = __shfl_xor(c1, 32), p2 = __shfl_xor(c2, 32);
                    const int m1 = max(c1, p1), m2 = max(min(c1, p1), max(c2, p2));
#pragma unroll
                    for (int e = 0; e < 2; ++e) {   // chunk top-2 into the running top-2 (later chunks: strict <)
                        const int key = e == 0 ? m1 : m2;
                        if (key != INT_MIN) {
                            const int t_ = -(key >> 8), i_ = c0 + 255 - (key & 255);
                            if (t_ < T2) {
                                if (t_ < T1) { T2 = T1; J2 = J1; T1 = t_; J1 = i_; }
                                else { T2 = t_; J2 = i_; }
                            }
                        }
                    }
                }
            }
            // (T1, J1) <= (T2, J2) in (distance, index) order: k1 <= k2 (see the merge above)
            if (active && h == 0 && qrow >= 0) {
                const unsigned long long k1 = T1 != INT_MAX ? ((unsigned long long)(na + T1) << 32) | (unsigned)(r + 16 * J1) : ~0ull;
                const unsigned long long k2 = T2 != INT_MAX ? ((unsigned long long)(na + T2) << 32) | (unsigned)(r + 16 * J2) : ~0ull;
                if (mode != 0) {          // one of exactly two subsets: its own 16-B slot, no atomics
                    unsigned long long* b = (mode == 1 ? top2 : slot1) + 2 * (P.dense_base + qslot);
                    *reinterpret_cast<ulonglong2*>(b) = make_ulonglong2(k1, k2);
                } else if (T1 != INT_MAX) {
                    unsigned long long* b = top2 + 2 * (P.dense_base + qslot);
                    if (T2 != INT_MAX) atomicMin(b + 1, k2);
                    const unsigned long long old = atomicMin(b, k1);
                    atomicMin(b + 1, old > k1 ? old : k1);
                }
            }
        }
        __syncthreads();   // ql / s_n are rewritten by the next window
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // a staged chunk no group read: its LDS-DMA ends before the LDS is freed
}

// FP6 product path: the most full-route queries of a pair that ride the subset pass 2 (16 visits and the
// atomic merge each) in place of one nearly empty 128-query full-row item (measured).
constexpr int SIFT_RIDE_MAX = 32;

// Pass 2, row form (the FP6 product path's certified route): one wave per (pair, row subset), one 256-thread
// workgroup per (pair, group of four subsets); wave w of group G owns subset r = 4 G + w.  The FP6 screen's
// masks have one bit (fp6::certified) or are QMASK_FULL_ROUTE, so a certified query belongs to exactly one
// subset and the subset's unit is a wave: nothing but the gather is shared between the four waves.
//
// Gather, once per workgroup and 1024-entry window of the pair's forwarded list: every entry goes to at most
// one of five lists in LDS, the four subsets' and the riders' (full-route entries of a pair with at most
// SIFT_RIDE_MAX of them, which every wave takes behind its own list as if appended to all four), ranked by a
// returning LDS atomic and placed after a barrier, so the lists share one pool of a window's size.  An entry
// is query row | slot in the window << 20 | rider << 30.
//
// Rows: the wave streams its subset's rows j = r + 16 i in 32-row tiles through two 4-KB buffers of its own
// (LDS-DMA, sift_subset_kernel's swizzle, the tile's norms beside it): the next tile lands under the one
// being multiplied, tile 0 is issued at entry, under the gather, and the only wait is the wave's own counted
// vmcnt: no workgroup barrier in the row loop.  (Loading the A operand straight from global memory, lane
// (l32, h) the pieces 2 m + h of row l32, measured slower than sift_subset_kernel: each such instruction
// touches 32 rows, 32 B of each, where eight lanes of a DMA fetch one whole row)
// Every row r + 16 i, i < rows_pad / 16, lies in the image's padded rows (pad rows are zero; their keys are
// INT_MIN, as those of the rows past nt).
// Rows are the outer loop, the wave's up to QTMAX 32-query tiles the inner one (B fragments and the running
// chunk top-2 in registers); more tiles take another pass over the rows.  The tile's 32 keys reach the
// accumulator layout through a 128-B strip of LDS private to the wave (DS instructions of one wave execute
// in order: no barrier).  Keys, 256-row chunks, the strict < of later chunks and the (s << 32) | j keys are
// sift_subset_kernel's: both give the same top-2 of a (query, subset).
//
// Result: a certified slot has one writer, which stores (k1, k2) as one 16-B word over the slot's `top2`
// pair (sift_finish_kernel clamps s2 for a one-bit mask); a rider takes sift_subset_kernel's three atomics.
template <int QTMAX>
__global__ __launch_bounds__(256, 4)
void sift_rows_kernel(const PairDev* __restrict__ pairs, const ImgDev* __restrict__ imgs,
                      const int8_t* __restrict__ desc8, const int32_t* __restrict__ norm,
                      const int32_t* __restrict__ qlist, const int32_t* __restrict__ qmask,
                      const int32_t* __restrict__ qcount, const int32_t* __restrict__ qcount2,
                      const int32_t* __restrict__ porder, unsigned long long* __restrict__ top2) {
    constexpr int WIN = 1024;                 // forwarded-query window scanned per round
    constexpr int EPT = WIN / 256;            // window entries per thread
    constexpr int RIDER = 1 << 30;
    constexpr int TILE = 32 * SIFT_DIM;       // bytes of a 32-row tile
    __shared__ __attribute__((aligned(16))) char rows_lds[4][2][TILE];   // per wave: the tile being read, the one landing
    __shared__ int nrm_lds[4][2][64];         // their norms (lanes 32..63 land a copy)
    __shared__ int pool[WIN];                 // the five lists, back to back
    __shared__ __attribute__((aligned(16))) int strip[4][32];
    __shared__ int s_cnt[5];
    // four workgroups per CU (160 KB of LDS), every wave working (128 VGPRs)
    static_assert(sizeof(rows_lds) + sizeof(nrm_lds) + sizeof(pool) + sizeof(strip) + sizeof(s_cnt) <= 160 * 1024 / 4,
                  "pass-2 LDS must leave four workgroups resident per CU");

    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, l32 = lane & 31;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: the subset and all that follows from it
    const int item = xcd_remap(blockIdx.x, gridDim.x);
    const int pi = porder[item >> 2], G = item & 3, r = 4 * G + wid;
    const int cnt = qcount[pi];
    if (cnt == 0) return;
    const PairDev P = pairs[pi];
    const ImgDev L = imgs[P.left], R = imgs[P.right];
    const int nt = R.rows;
    if (4 * G >= nt) return;                  // no subset of the group has a row
    const bool live = r < nt;                 // wave-uniform: an empty subset's wave only joins the barriers
    const int ntile = R.rows_pad >> 9;        // 32-row tiles of a subset (rows_pad / 16 rows, a multiple of 32); >= 1
    const int32_t* qls = qlist + P.dense_base;
    const int32_t* qms = qmask + P.dense_base;
    const bool riders = qcount2[pi] <= SIFT_RIDE_MAX;

    const int8_t* rbase = desc8 + (R.row0 + r) * SIFT_DIM;   // scalar bases, one 32-bit lane offset each
    const int32_t* nbase = norm + R.row0 + r;
    // Tile t (< ntile: rows r + 16 i < rows_pad, i = 32 t + row) -> the wave's buffer b by LDS-DMA, five
    // instructions: 16-B piece p = 64 u + lane of the tile is row p >> 3, slot p & 7, which holds the row's piece
    // slot ^ ((row >> 1) & 7) (eight lanes fetch one whole 128-B row), and the norm of row l32.
    auto stage = [&](int t, int b) {
        const int8_t* src = rbase + (int64_t)t * (32 * 16 * SIFT_DIM);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int rr = 8 * u + (lane >> 3), c = (lane & 7) ^ ((rr >> 1) & 7);
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(src + (unsigned)(rr * (16 * SIFT_DIM) + 16 * c)),
                                             (LDS_AS void*)(&rows_lds[wid][b][u * 1024]), 16, 0, 0);
        }
        __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(nbase + t * (32 * 16) + 16 * l32),
                                         (LDS_AS void*)(&nrm_lds[wid][b][0]), 4, 0, 0);
    };
    int cur = 0;                              // the buffer of the next tile to read (tile 0 of the next pass)
    if (live) stage(0, 0);

    for (int e0 = 0; e0 < cnt; e0 += WIN) {
        if (tid < 5) s_cnt[tid] = 0;
        __syncthreads();
        int ent[EPT], at[EPT], li[EPT];
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int e = e0 + k * 256 + tid;
            li[k] = -1;
            ent[k] = at[k] = 0;
            if (e < cnt) {
                const int mk = qms[e];
                if (mk & QMASK_FULL_ROUTE) li[k] = riders ? 4 : -1;
                else if (mk != 0 && ((__ffs(mk) - 1) >> 2) == G) li[k] = (__ffs(mk) - 1) & 3;
                if (li[k] >= 0) {
                    ent[k] = qls[e] | ((e - e0) << 20) | (li[k] == 4 ? RIDER : 0);
                    at[k] = atomicAdd(&s_cnt[li[k]], 1);
                }
            }
        }
        __syncthreads();
        int base[5], n_l[5];
        base[0] = 0;
#pragma unroll
        for (int l = 0; l < 5; ++l) {
            n_l[l] = __builtin_amdgcn_readfirstlane(s_cnt[l]);   // scalar, as everything sized by it
            if (l < 4) base[l + 1] = base[l] + n_l[l];
        }
#pragma unroll
        for (int k = 0; k < EPT; ++k)
            if (li[k] >= 0) pool[base[li[k]] + at[k]] = ent[k];
        __syncthreads();
        const int n_own = n_l[wid], b_own = base[wid], n = live ? n_own + n_l[4] : 0;
        for (int g0 = 0; g0 < n; g0 += 32 * QTMAX) {
            const int nqt = min(QTMAX, (n - g0 + 31) >> 5);   // wave-uniform
            // this lane's entry of tile qt (-1: none); read again in the epilogue, not kept across the row loop
            auto entry = [&](int qt) {
                const int qe = g0 + qt * 32 + l32;
                return qe < n ? (qe < n_own ? pool[b_own + qe] : pool[base[4] + qe - n_own]) : -1;
            };
            i32x4 bq[QTMAX][4];
#pragma unroll
            for (int qt = 0; qt < QTMAX; ++qt) {
#pragma unroll
                for (int m = 0; m < 4; ++m) bq[qt][m] = i32x4{0, 0, 0, 0};
                if (qt < nqt) {
                    const int qpk = entry(qt);
                    const int64_t lrow = L.row0 + (qpk < 0 ? 0 : (qpk & 0xFFFFF));
                    const i32x4* src = reinterpret_cast<const i32x4*>(desc8 + lrow * SIFT_DIM);
#pragma unroll
                    for (int m = 0; m < 4; ++m) bq[qt][m] = src[2 * m + h];
                }
            }
            int T1[QTMAX], T2[QTMAX], c1[QTMAX], c2[QTMAX];
            unsigned JJ[QTMAX];   // J1 | J2 << 16: subset rows i < rows_pad / 16 <= 2^14 (an image has fewer than 2^18 rows)
#pragma unroll
            for (int qt = 0; qt < QTMAX; ++qt) {
                T1[qt] = T2[qt] = INT_MAX; JJ[qt] = 0; c1[qt] = c2[qt] = INT_MIN;
            }
            for (int t = 0; t < ntile; ++t) {
                stage(t + 1 < ntile ? t + 1 : 0, cur ^ 1);   // (tile 0 again: the next pass's or window's first)
                // tile t has landed once at most the five instructions above are outstanding (vector memory
                // instructions retire in order; whatever else was issued since only tightens the wait)
                // The reads are written out: before a ds_read the compiler has seen, it waits for every LDS-DMA in
                // flight (vmcnt(0)), the tile just issued included, which would undo the overlap.
                int nv;
                i32x4 a[4];
                {
                    const unsigned rb = (unsigned)(size_t)(LDS_AS const void*)&rows_lds[wid][cur][l32 * SIFT_DIM];
                    const unsigned sw = (l32 >> 1) & 7;
                    asm volatile("s_waitcnt vmcnt(5)\n\t"
                                 "ds_read_b32 %0, %5\n\t"
                                 "ds_read_b128 %1, %6\n\t"
                                 "ds_read_b128 %2, %7\n\t"
                                 "ds_read_b128 %3, %8\n\t"
                                 "ds_read_b128 %4, %9\n\t"
                                 "s_waitcnt lgkmcnt(0)"
                                 : "=&v"(nv), "=&v"(a[0]), "=&v"(a[1]), "=&v"(a[2]), "=&v"(a[3])
                                 : "v"((unsigned)(size_t)(LDS_AS const void*)&nrm_lds[wid][cur][l32]),
                                   "v"(rb + 16 * ((0 + h) ^ sw)), "v"(rb + 16 * ((2 + h) ^ sw)),
                                   "v"(rb + 16 * ((4 + h) ^ sw)), "v"(rb + 16 * ((6 + h) ^ sw))
                                 : "memory");
                }
                cur ^= 1;
                const int i = t * 32 + l32;
                strip[wid][l32] = r + 16 * i < nt ? -(nv << 8) + 255 - (i & 255) : INT_MIN;   // (both halves: the same word)
                asm volatile("" ::: "memory");   // the strip is the wave's own: its DS instructions execute in order
                i32x4 kv[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) kv[g] = *reinterpret_cast<const i32x4*>(&strip[wid][8 * g + 4 * h]);
                asm volatile("" ::: "memory");
#pragma unroll
                for (int qt = 0; qt < QTMAX; ++qt) {
                    if (qt >= nqt) continue;
                    i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                    for (int m = 0; m < 4; ++m) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[m], bq[qt][m], acc, 0, 0, 0);
#pragma unroll
                    for (int q = 0; q < 16; q += 4) {   // (c2 every four keys: two medians live, not eight)
                        int mm[2];
#pragma unroll
                        for (int u = 0; u < 4; u += 2) {
                            const int ka = (int)(((unsigned)acc[q + u] << 9) + (unsigned)kv[q >> 2][u]);
                            const int kb = (int)(((unsigned)acc[q + u + 1] << 9) + (unsigned)kv[q >> 2][u + 1]);
                            mm[u >> 1] = v_med3(c1[qt], ka, kb);
                            c1[qt] = v_max3(c1[qt], ka, kb);
                        }
                        c2[qt] = v_max3(mm[0], mm[1], c2[qt]);
                    }
                }
                if ((t & 7) == 7 || t + 1 == ntile) {   // end of a 256-row chunk
                    const int cb = (t >> 3) * 256;
#pragma unroll
                    for (int qt = 0; qt < QTMAX; ++qt) {
                        const int p1 = __shfl_xor(c1[qt], 32), p2 = __shfl_xor(c2[qt], 32);
                        const int m1 = max(c1[qt], p1), m2 = max(min(c1[qt], p1), max(c2[qt], p2));
#pragma unroll
                        for (int e = 0; e < 2; ++e) {   // chunk top-2 into the running top-2 (later chunks: strict <)
                            const int key = e == 0 ? m1 : m2;
                            if (key != INT_MIN) {
                                const int t_ = -(key >> 8), i_ = cb + 255 - (key & 255);
                                if (t_ < T2[qt]) {
                                    if (t_ < T1[qt]) { T2[qt] = T1[qt]; T1[qt] = t_; JJ[qt] = (JJ[qt] << 16) | (unsigned)i_; }
                                    else { T2[qt] = t_; JJ[qt] = (JJ[qt] & 0xFFFFu) | ((unsigned)i_ << 16); }
                                }
                            }
                        }
                        c1[qt] = c2[qt] = INT_MIN;
                    }
                }
            }
            // (T1, J1) <= (T2, J2) in (distance, index) order: k1 <= k2 (the merge at sift_subset_kernel)
#pragma unroll
            for (int qt = 0; qt < QTMAX; ++qt) {
                const int qpk = qt < nqt ? entry(qt) : -1;
                if (h != 0 || qpk < 0) continue;
                const long long nq = norm[L.row0 + (qpk & 0xFFFFF)];
                const unsigned long long k1 = T1[qt] != INT_MAX ? ((unsigned long long)(nq + T1[qt]) << 32) | (unsigned)(r + 16 * (JJ[qt] & 0xFFFFu)) : ~0ull;
                const unsigned long long k2 = T2[qt] != INT_MAX ? ((unsigned long long)(nq + T2[qt]) << 32) | (unsigned)(r + 16 * (JJ[qt] >> 16)) : ~0ull;
                unsigned long long* b = top2 + 2 * (P.dense_base + e0 + ((qpk >> 20) & (WIN - 1)));
                if (!(qpk & RIDER)) {   // certified: this wave is the slot's only writer
                    *reinterpret_cast<ulonglong2*>(b) = make_ulonglong2(k1, k2);
                } else if (T1[qt] != INT_MAX) {
                    if (T2[qt] != INT_MAX) atomicMin(b + 1, k2);
                    const unsigned long long old = atomicMin(b, k1);
                    atomicMin(b + 1, old > k1 ? old : k1);
                }
            }
        }
        __syncthreads();   // pool / s_cnt are rewritten by the next window
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the tile still landing: its LDS-DMA ends before the LDS is freed
}

// Pass 2, subset form: the forwarded queries' merged top-2 -> dense results (one workgroup per pair).
__global__ __launch_bounds__(256)
void sift_settle_kernel(const PairDev* __restrict__ pairs, const ImgDev* __restrict__ imgs,
                        const int32_t* __restrict__ qlist, const int32_t* __restrict__ qcount,
                        const unsigned long long* __restrict__ top2, int32_t* __restrict__ out_idx,
                        float* __restrict__ out_dist, int2* __restrict__ slow_list, int32_t* __restrict__ slow_count,
                        double ratio, const int32_t* __restrict__ qmask, const unsigned long long* __restrict__ slot1,
                        const int32_t* __restrict__ porder = nullptr) {
    const int pi = porder ? porder[blockIdx.x] : (int)blockIdx.x;   // porder: one batch's pairs (overlapped pass 2)
    const int cnt = qcount[pi];
    if (cnt == 0) return;
    const PairDev P = pairs[pi];
    const int nt = imgs[P.right].rows;
    for (int e = threadIdx.x; e < cnt; e += 256) {
        const int qi = qlist[P.dense_base + e];
        const int64_t o = P.dense_base + qi;
        unsigned long long b0 = top2[2 * o], b1 = top2[2 * o + 1];
        if (__popc(qmask[P.dense_base + e]) == 2) {   // two subsets, one slot each (sift_subset_kernel): merge the two top-2
            const unsigned long long c0 = slot1[2 * o], c1 = slot1[2 * o + 1];
            const unsigned long long lo = b0 < c0 ? b0 : c0, hi = b0 < c0 ? c0 : b0, m2 = b1 < c1 ? b1 : c1;
            b0 = lo;
            b1 = hi < m2 ? hi : m2;
        }
        if (b0 == ~0ull || (nt >= 2 && b1 == ~0ull)) {
            if (nt == 0) { out_idx[o] = -1; out_dist[o] = 0.f; }   // an empty train image: no neighbour
            // otherwise pass 2 left a flagged subset unscanned: the UNSETTLED stamp stays, so
            // assemble_kernel counts the query and the run fails (SFMX_EINTERNAL), never a lost match
            continue;
        }
        const int64_t s1 = (int64_t)(b0 >> 32), s2 = (int64_t)(b1 >> 32);
        if (nt >= 2 && s2 >= SQRT_SAFE) {
            const int slot = atomicAdd(slow_count, 1);
            slow_list[slot] = make_int2(pi, qi);
            out_idx[o] = -2;
            continue;
        }
        const float d1 = sqrt_rn_int(s1);
        out_idx[o] = lowe_select((int)(b0 & 0xffffffffu), d1, nt >= 2 ? sqrt_rn_int(s2) : 0.f, nt, ratio);
        out_dist[o] = d1;
    }
}

#ifdef SFMX_DIAG
// Timing probe only (wrong results; diagnostic build only): flips the sign bit of every int8
// operand byte, i.e. the unshifted byte a instead of a - 128, to measure how operand
// bit patterns move the clock the chip holds under the screening MFMAs.
__global__ void probe_xor80_kernel(uint32_t* __restrict__ p, int64_t n_words) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_words) p[i] ^= 0x80808080u;
}
#endif
// imax[2 i], imax[2 i + 1]: image i's largest |e|^2 and |a|^2 (zero before the launch).
hipError_t launch_prep_l2_batch(const PrepImg* tab, int n, int max_rows_pad, int8_t* desc8, int32_t* norm,
                                int32_t* keyc, int32_t* keyc2, int32_t* flags, uint32_t* desc6, float* keyf,
                                int2* ne, int32_t* imax, hipStream_t st) {
    if (n == 0 || max_rows_pad == 0) return hipSuccess;
    prep_l2_batch_kernel<<<dim3((unsigned)((max_rows_pad + PREP_ROWS - 1) / PREP_ROWS), (unsigned)n), 256, 0, st>>>(
        tab, desc8, norm, keyc, keyc2, flags, Fp6Rows{desc6, keyf, ne}, imax);
    return hipGetLastError();
}
// The per-image integrality flags into pinned, host-coherent memory, then a sequence word with
// system-scope release: set_images spins on the word instead of a D2H copy + hipStreamSynchronize
// (whose interrupt-driven wake-up the host would pay once per matching call).
__global__ __launch_bounds__(256)
void publish_flags_kernel(const int32_t* __restrict__ flags, int n, int32_t* __restrict__ dst, unsigned* __restrict__ seq,
                          unsigned v) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = flags[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(seq, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
hipError_t launch_publish_flags(const int32_t* flags, int n, int32_t* dst, unsigned* seq, unsigned v, hipStream_t st) {
    publish_flags_kernel<<<1, 256, 0, st>>>(flags, n, dst, seq, v);
    return hipGetLastError();
}
#ifdef SFMX_DIAG
// Diagnostic build only: both forms of the f8f6f4 MFMA (fp6::mfma16 / mfma32: block-scaled with unit scales,
// and unscaled) on caller-supplied fragments, one wave per case (tests/test_gpu_mfma_unscaled.py).
//   16 x 16 x 128: a, b [case][lane] fragments, c, d [case][lane] 4 floats
//   32 x 32 x 64, the chained pair of the wide screen: a, b [case][m = 0, 1][lane], c, d [case][lane] 16 floats
template <int FMT>
__global__ __launch_bounds__(64)
void mfma_forms16_kernel(const i32x8* __restrict__ a, const i32x8* __restrict__ b, const f32x4* __restrict__ c,
                         f32x4* __restrict__ d_scaled, f32x4* __restrict__ d_unscaled) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    d_scaled[i] = fp6::mfma16<FMT, true>(a[i], b[i], c[i]);
    d_unscaled[i] = fp6::mfma16<FMT, false>(a[i], b[i], c[i]);
}
template <int FMT>
__global__ __launch_bounds__(64)
void mfma_forms32_kernel(const i32x8* __restrict__ a, const i32x8* __restrict__ b, const f32x16* __restrict__ c,
                         f32x16* __restrict__ d_scaled, f32x16* __restrict__ d_unscaled) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x, j = (int64_t)blockIdx.x * 128 + threadIdx.x;
    d_scaled[i] = fp6::mfma32<FMT, true>(a[j + 64], b[j + 64], fp6::mfma32<FMT, true>(a[j], b[j], c[i]));
    d_unscaled[i] = fp6::mfma32<FMT, false>(a[j + 64], b[j + 64], fp6::mfma32<FMT, false>(a[j], b[j], c[i]));
}
hipError_t launch_mfma_forms(int shape, int fmt, int n, const int32_t* a, const int32_t* b, const float* c, float* d_scaled,
                             float* d_unscaled, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if ((shape != 16 && shape != 32) || (fmt != fp6::FMT_E2M3 && fmt != fp6::FMT_E2M1)) return hipErrorInvalidValue;
    const i32x8 *pa = reinterpret_cast<const i32x8*>(a), *pb = reinterpret_cast<const i32x8*>(b);
    if (shape == 16) {
        const f32x4* pc = reinterpret_cast<const f32x4*>(c);
        f32x4 *ds = reinterpret_cast<f32x4*>(d_scaled), *du = reinterpret_cast<f32x4*>(d_unscaled);
        if (fmt == fp6::FMT_E2M3) mfma_forms16_kernel<fp6::FMT_E2M3><<<n, 64, 0, st>>>(pa, pb, pc, ds, du);
        else mfma_forms16_kernel<fp6::FMT_E2M1><<<n, 64, 0, st>>>(pa, pb, pc, ds, du);
    } else {
        const f32x16* pc = reinterpret_cast<const f32x16*>(c);
        f32x16 *ds = reinterpret_cast<f32x16*>(d_scaled), *du = reinterpret_cast<f32x16*>(d_unscaled);
        if (fmt == fp6::FMT_E2M3) mfma_forms32_kernel<fp6::FMT_E2M3><<<n, 64, 0, st>>>(pa, pb, pc, ds, du);
        else mfma_forms32_kernel<fp6::FMT_E2M1><<<n, 64, 0, st>>>(pa, pb, pc, ds, du);
    }
    return hipGetLastError();
}
hipError_t launch_probe_xor80(int8_t* p, int64_t bytes, hipStream_t st) {
    const int64_t n = bytes / 4;
    if (n == 0) return hipSuccess;
    probe_xor80_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(reinterpret_cast<uint32_t*>(p), n);
    return hipGetLastError();
}
#endif

// Pass-2 work list: ceil(qcount[p] / 512) items per pair, pairs in the host's
// order (sorted by train image, so XCD-contiguous items share train rows).
// One 1024-thread block; each thread owns a contiguous run of pairs.
// A pair with at most `ride` queries gets no item (its queries ride the subset kernel; 0: every pair with a query).
template <int ISH>   // queries per pass-2 item = 1 << ISH
__global__ __launch_bounds__(1024)
void compact_work_kernel(const int32_t* __restrict__ porder, int n_pairs, const int32_t* __restrict__ qcount,
                         WorkItem* __restrict__ work2, int32_t* __restrict__ work2_n, int ride = 0) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int per = (n_pairs + 1023) / 1024, p0 = min(tid * per, n_pairs), p1 = min(p0 + per, n_pairs);
    int mine = 0;
    auto items = [&](int c) { return c > ride ? (c + (1 << ISH) - 1) >> ISH : 0; };
    for (int i = p0; i < p1; ++i) mine += items(qcount[porder[i]]);
    int incl = mine;                                  // inclusive scan: wave, then across waves
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int base = 0;
    for (int i = 0; i < wv; ++i) base += wsum[i];
    int at = base + incl - mine;
    for (int i = p0; i < p1; ++i) {
        const int p = porder[i], n = items(qcount[p]);
        for (int k = 0; k < n; ++k) work2[at++] = WorkItem{p, k << ISH};
    }
    if (tid == 1023) *work2_n = base + incl;
}

// Exact path for queries whose best-2 falls in the float-sqrt collision range:
// one wave per query, s exact via v_dot4_i32_i8, ranked on (sqrtf bits, j).
__device__ __forceinline__ void top2_u64(unsigned long long k, unsigned long long& b1, unsigned long long& b2) {
    if (k < b2) { if (k < b1) { b2 = b1; b1 = k; } else b2 = k; }
}

// One wave: query row `lrow` of the pool against train rows [rrow0, rrow0 + nt); every lane ends with
// the two smallest (sqrtf bits << 32 | j) keys.
__device__ __forceinline__ void slow_top2(const int8_t* __restrict__ desc8, const int32_t* __restrict__ norm,
                                          int64_t lrow, int64_t rrow0, int nt, int lane,
                                          unsigned long long& b1, unsigned long long& b2) {
    const int* q = reinterpret_cast<const int*>(desc8 + lrow * SIFT_DIM);
    int qw[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) qw[k] = q[k];
    const int na = norm[lrow];
    b1 = ~0ull;
    b2 = ~0ull;
    for (int j = lane; j < nt; j += 64) {
        const int* t = reinterpret_cast<const int*>(desc8 + (rrow0 + j) * SIFT_DIM);
        int dot = 0;
#pragma unroll
        for (int k = 0; k < 32; ++k) dot = __builtin_amdgcn_sdot4(qw[k], t[k], dot, false);
        const int64_t s = (int64_t)na + norm[rrow0 + j] - 2 * (int64_t)dot;
        const float d = sqrt_rn_int(s);
        top2_u64(((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j, b1, b2);
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long p1 = __shfl_xor(b1, o), p2 = __shfl_xor(b2, o);
        top2_u64(p1, b1, b2);
        top2_u64(p2, b1, b2);
    }
}

__global__ __launch_bounds__(256)
void sift_slow_kernel(const int2* __restrict__ slow_list, const int32_t* __restrict__ slow_count,
                      const PairDev* __restrict__ pairs, const ImgDev* __restrict__ imgs,
                      const int8_t* __restrict__ desc8, const int32_t* __restrict__ norm,
                      int32_t* __restrict__ out_idx, float* __restrict__ out_dist, double ratio) {
    const int lane = threadIdx.x & 63;
    const int nwave = gridDim.x * (blockDim.x >> 6);
    const int n = *slow_count;
    for (int e = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); e < n; e += nwave) {
        const int2 it = slow_list[e];
        const PairDev P = pairs[it.x];
        const ImgDev L = imgs[P.left], R = imgs[P.right];
        unsigned long long b1, b2;
        slow_top2(desc8, norm, L.row0 + it.y, R.row0, R.rows, lane, b1, b2);
        if (lane == 0) {
            const float d1 = __uint_as_float((unsigned)(b1 >> 32)), d2 = __uint_as_float((unsigned)(b2 >> 32));
            const int64_t o = P.dense_base + it.y;
            out_idx[o] = lowe_select((int)(b1 & 0xffffffffu), d1, d2, 2, ratio);   // slow path implies nt >= 2
            out_dist[o] = d1;
        }
    }
}

// fp32 fallback (non-integer SIFT rows): one thread per query, the oracle's
// 8-partial-sum order, train rows staged through LDS.  Not MFMA: this path
// exists for correctness on out-of-contract input only.
__global__ __launch_bounds__(512)
void sift_f32_kernel(const WorkItem* __restrict__ work, const int32_t* __restrict__ pair_sel,
                     const PairDev* __restrict__ pairs, const ImgDev* __restrict__ imgs,
                     const float* __restrict__ f32, int32_t* __restrict__ out_idx,
                     float* __restrict__ out_dist, double ratio) {
    // the default -ffp-contract=fast-honor-pragmas fused the d * d + acc below into v_pk_fma_f32 (r03 wrote
    // them as __fadd_rn / __fmul_rn, which are inlined plain + / * outside this pragma's reach): 1-ulp
    // distances vs the oracle's -ffp-contract=off sums, found in r04 on an integral x non-integral pair
#pragma clang fp contract(off)
    constexpr int STAGE = 32;
    __shared__ float tl[STAGE * SIFT_DIM];
    const WorkItem w = work[blockIdx.x];
    (void)pair_sel;
    const PairDev P = pairs[w.pair];
    const ImgDev L = imgs[P.left], R = imgs[P.right];
    const int qi = w.q0 + threadIdx.x;
    const float* qrow = f32 + (L.row0 + (qi < L.rows_pad ? qi : 0)) * SIFT_DIM;
    unsigned b1 = 0x7f7fffffu, b2 = 0x7f7fffffu;
    int j1 = -1, j2 = -1;
    for (int s0 = 0; s0 < R.rows; s0 += STAGE) {
        __syncthreads();
        for (int i = threadIdx.x; i < STAGE * SIFT_DIM; i += blockDim.x)
            tl[i] = f32[(R.row0 + s0) * SIFT_DIM + i];
        __syncthreads();
        const int lim = min(STAGE, R.rows - s0);
        for (int jj = 0; jj < lim; ++jj) {
            float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int k = 0; k < SIFT_DIM; k += 8)
#pragma unroll
                for (int l = 0; l < 8; ++l) {
                    const float d = qrow[k + l] - tl[jj * SIFT_DIM + k + l];
                    acc[l] = acc[l] + d * d;   // no FMA contraction (the pragma above; oracle: -ffp-contract=off)
                }
            float ssum = acc[0];
#pragma unroll
            for (int l = 1; l < 8; ++l) ssum += acc[l];
            const unsigned key = __float_as_uint(__builtin_sqrtf(ssum));
            const int j = s0 + jj;
            if (key < b2) { if (b1 > key) { b2 = b1; j2 = j1; b1 = key; j1 = j; } else { b2 = key; j2 = j; } }
        }
    }
    (void)j2;
    if (qi >= L.rows) return;
    const int64_t o = P.dense_base + qi;
    if (R.rows == 0) { out_idx[o] = -1; out_dist[o] = 0.f; return; }
    const float d1 = __uint_as_float(b1), d2 = __uint_as_float(b2);
    out_idx[o] = lowe_select(j1, d1, d2, R.rows, ratio);
    out_dist[o] = d1;
}

// ---------------------------------------------------------------------------
// ORB Hamming 2-NN on the matrix cores (FP4 e2m1, +-1 encoding).
//
//   With bits mapped to +-1, dot(a, b) = 256 - 2 * hamming(a, b): an exact
//   contraction of 256 products of +-1, i.e. 4 x v_mfma_f32_32x32x64_f8f6f4
//   (FP4 operands, unscaled: fp6::mfma32) per 32x32 tile — the same 128-byte rows
//   and LDS stage as the SIFT kernel, at the FP4 rate (2x int8 per clock).
//   The key needs no VALU: the MFMA's C operand is a per-train-row constant
//       C_j = 767 + (16383 - (j & 16383)) / 16384
//   so acc = C_j + dot lies in [511, 1024) where the f32 ulp is <= 2^-14: the
//   sum is exact, its integer part is 767 + dot and its fraction carries the
//   row's tie-break index, so the top-2 runs on the raw accumulators with
//   v_med3_f32 / v_max3_f32 (larger key = smaller hamming, then lower index:
//   OpenCV's order).  Every
//   16384 rows the chunk's top-2 is decoded and folded into the running
//   (hamming, j) top-2 with strict '<' (earlier chunks keep ties).
//   Pad rows have C = 0 and all-zero nibbles: key 0.0 never wins.
template <int QT, int WAVES, int MINW, int STAGE>
__global__ __launch_bounds__(WAVES * 64, MINW)
void orb_mfma_kernel(const WorkItem* __restrict__ work, const PairDev* __restrict__ pairs,
                     const ImgDev* __restrict__ imgs, const uint8_t* __restrict__ desc4,
                     const int32_t* __restrict__ keyc, int32_t* __restrict__ out_idx,
                     float* __restrict__ out_dist, double ratio) {
    constexpr int ROWB = 128;                               // 256 fp4 nibbles per row
    constexpr int GLDS = STAGE * ROWB / (WAVES * 64 * 16);
    static_assert(GLDS * WAVES * 64 * 16 == STAGE * ROWB, "stage must split into whole 16-B pieces");
    constexpr int CHUNK = 16384;                            // rows per key chunk (14 index bits)
    static_assert(CHUNK % STAGE == 0, "stages tile the key chunk");
    constexpr int DESC_BYTES = STAGE * ROWB;
    constexpr int BUF_BYTES = DESC_BYTES + STAGE * 4;
    constexpr int SPC = CHUNK / STAGE;
    constexpr float KEY_FLOOR = 256.f;                      // real keys are >= 511, pad rows 0
    __shared__ __attribute__((aligned(16))) char lds[2 * BUF_BYTES];

    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    const WorkItem w = work[xcd_remap(blockIdx.x, gridDim.x)];
    const PairDev P = pairs[w.pair];
    const ImgDev L = imgs[P.left], R = imgs[P.right];
    const int nq = L.rows, nt = R.rows;
    const int qbase = w.q0 + wid * (QT * 32);

    i32x4 bq[QT][4];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const i32x4* src = reinterpret_cast<const i32x4*>(desc4 + (L.row0 + qbase + qt * 32 + l32) * ROWB);
#pragma unroll
        for (int m = 0; m < 4; ++m) bq[qt][m] = src[2 * m + h];
    }
    int T1[QT], J1[QT], T2[QT], J2[QT];
    float c1[QT], c2[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        T1[qt] = T2[qt] = INT_MAX; J1[qt] = J2[qt] = -1; c1[qt] = c2[qt] = 0.f;
    }
    const int nstages = (nt + STAGE - 1) / STAGE;
    const uint8_t* tbase = desc4 + R.row0 * ROWB;
    const int32_t* kbase = keyc + R.row0;

    auto stage = [&](int s, int buf) {
        char* base = lds + buf * BUF_BYTES;
#pragma unroll
        for (int i = 0; i < GLDS; ++i) {
            const int p = i * WAVES * 64 + threadIdx.x;
            const int rr = p >> 3, slot = p & 7, c = slot ^ ((rr >> 1) & 7);
            const uint8_t* g = tbase + (int64_t)(s * STAGE + rr) * ROWB + 16 * c;
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)g,
                                             (LDS_AS void*)(base + (i * WAVES + wid) * 1024), 16, 0, 0);
        }
        if (wid < STAGE / 64)
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(kbase + s * STAGE + wid * 64 + lane),
                                             (LDS_AS void*)(base + DESC_BYTES + wid * 256), 4, 0, 0);
    };
    // Top-2 by max on the f32 accumulators (v_med3_f32 / v_max3_f32; compiler
    // builtins, not inline asm, so the MFMA->VALU read hazards are resolved).
    auto select = [&](const f32x16& acc, float& b1, float& b2) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const float ka = acc[r], kb = acc[r + 1];
            b2 = fmaxf(__builtin_amdgcn_fmed3f(b1, ka, kb), b2);
            b1 = fmaxf(b1, fmaxf(ka, kb));
        }
    };
    auto i8of = [](const i32x4& v) { return i32x8{v.x, v.y, v.z, v.w, 0, 0, 0, 0}; };

    if (nstages > 0) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int s = 0; s < nstages; ++s) {
        const int buf = s & 1;
        if (s + 1 < nstages) stage(s + 1, buf ^ 1);
        const char* base = lds + buf * BUF_BYTES;
#pragma unroll
        for (int t = 0; t < STAGE / 32; ++t) {
            const int row = t * 32 + l32;
            i32x4 a[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int slot = (2 * m + h) ^ ((row >> 1) & 7);
                a[m] = *reinterpret_cast<const i32x4*>(base + row * ROWB + 16 * slot);
            }
            f32x16 cinit;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 kv = *reinterpret_cast<const f32x4*>(base + DESC_BYTES + 4 * (t * 32 + 8 * g + 4 * h));
                cinit[4 * g + 0] = kv.x; cinit[4 * g + 1] = kv.y; cinit[4 * g + 2] = kv.z; cinit[4 * g + 3] = kv.w;
            }
            f32x16 acc[QT];
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                acc[qt] = fp6::mfma32<fp6::FMT_E2M1, false>(i8of(a[0]), i8of(bq[qt][0]), cinit);
#pragma unroll
                for (int m = 1; m < 4; ++m)
                    acc[qt] = fp6::mfma32<fp6::FMT_E2M1, false>(i8of(a[m]), i8of(bq[qt][m]), acc[qt]);
            }
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) select(acc[qt], c1[qt], c2[qt]);
        }
        if ((s % SPC) == SPC - 1 || s + 1 == nstages) {      // end of a key chunk
            const int cb = (s / SPC) * CHUNK;
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                const float p1 = __shfl_xor(c1[qt], 32), p2 = __shfl_xor(c2[qt], 32);
                const float m1 = fmaxf(c1[qt], p1), m2 = fmaxf(fminf(c1[qt], p1), fmaxf(c2[qt], p2));
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const float v = e == 0 ? m1 : m2;
                    if (v >= KEY_FLOOR) {
                        const float ip = __builtin_floorf(v);
                        const int dot = (int)ip - 767;
                        const int t_ = (256 - dot) >> 1;                       // hamming distance
                        const int j_ = cb + 16383 - (int)((v - ip) * 16384.0f);
                        if (t_ < T2[qt]) {
                            if (t_ < T1[qt]) { T2[qt] = T1[qt]; J2[qt] = J1[qt]; T1[qt] = t_; J1[qt] = j_; }
                            else { T2[qt] = t_; J2[qt] = j_; }
                        }
                    }
                }
                c1[qt] = c2[qt] = 0.f;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const int qi = qbase + qt * 32 + l32;
        if (h != 0 || qi >= nq) continue;
        const int64_t o = P.dense_base + qi;
        if (nt == 0) { out_idx[o] = -1; out_dist[o] = 0.f; continue; }
        const float d1 = (float)T1[qt], d2 = (float)T2[qt];
        out_idx[o] = lowe_select(J1[qt], d1, d2, nt, ratio);
        out_dist[o] = d1;
    }
}

// ORB FP4 2-NN on v_mfma_f32_16x16x128_f8f6f4: the same +-1 encoding,
// C-operand keys and chunked top-2 as orb_mfma_kernel, in the 16x16 shape (the
// shape the SIFT screening pass holds a higher clock on).  K = 256 = 2 MFMAs per
// 16x16 tile; lane l: A row / B column l & 15, operand chunk 4m + (l >> 4)
// (A and B agree, so the chunk order is irrelevant to the dot product);
// accumulator rows 4 (l >> 4) + i of column l & 15.  Each query's 16 rows of a
// block are spread over 4 lanes, merged (shfl 16, 32) at each key chunk's end.
//   GATHER (pass 2 of the two-pass ORB path): as sift_knn2_kernel<GATHER>, the
//   item's queries are entries [q0, q0 + QT * WAVES * 16) of its pair's qlist.
template <int QT, int WAVES, int MINW, int STAGE, bool GATHER = false>
__global__ __launch_bounds__(WAVES * 64, MINW)
void orb_mfma16_kernel(const WorkItem* __restrict__ work, const PairDev* __restrict__ pairs,
                       const ImgDev* __restrict__ imgs, const uint8_t* __restrict__ desc4,
                       const int32_t* __restrict__ keyc, int32_t* __restrict__ out_idx,
                       float* __restrict__ out_dist, double ratio,
                       const int32_t* __restrict__ qlist = nullptr, const int32_t* __restrict__ qcount = nullptr,
                       const int32_t* __restrict__ work2_n = nullptr) {
    constexpr int ROWB = 128;
    constexpr int GLDS = STAGE * ROWB / (WAVES * 64 * 16);
    static_assert(GLDS * WAVES * 64 * 16 == STAGE * ROWB, "stage must split into whole 16-B pieces");
    static_assert(GATHER || QT * WAVES * 16 == 512, "pass-1 work items are 512 queries");
    constexpr int CHUNK = 16384;
    static_assert(CHUNK % STAGE == 0, "stages tile the key chunk");
    constexpr int DESC_BYTES = STAGE * ROWB;
    constexpr int BUF_BYTES = DESC_BYTES + STAGE * 4;
    constexpr int SPC = CHUNK / STAGE;
    constexpr float KEY_FLOOR = 256.f;
    __shared__ __attribute__((aligned(16))) char lds[2 * BUF_BYTES];

    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
    int nwork = gridDim.x;
    if constexpr (GATHER) {           // compacted list; the grid is an upper bound
        nwork = *work2_n;
        if ((int)blockIdx.x >= nwork) return;
    }
    const WorkItem w = work[xcd_remap(blockIdx.x, nwork)];
    const PairDev P = pairs[w.pair];
    const ImgDev L = imgs[P.left], R = imgs[P.right];
    const int nq = L.rows, nt = R.rows;
    const int qbase = w.q0 + wid * (QT * 16);
    int qrow[QT];                     // query row of this lane's column in each tile (-1: none)
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const int e = qbase + qt * 16 + l16;
        if constexpr (GATHER) qrow[qt] = e < qcount[w.pair] ? qlist[P.dense_base + e] : -1;
        else qrow[qt] = e < nq ? e : -1;
    }

    i32x4 bq[QT][2];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const int lr = GATHER ? (qrow[qt] < 0 ? 0 : qrow[qt]) : qbase + qt * 16 + l16;   // rows < rows_pad
        const i32x4* src = reinterpret_cast<const i32x4*>(desc4 + (L.row0 + lr) * ROWB);
#pragma unroll
        for (int m = 0; m < 2; ++m) bq[qt][m] = src[4 * m + g];
    }
    int T1[QT], J1[QT], T2[QT], J2[QT];
    float c1[QT], c2[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        T1[qt] = T2[qt] = INT_MAX; J1[qt] = J2[qt] = -1; c1[qt] = c2[qt] = 0.f;
    }
    const int nstages = (nt + STAGE - 1) / STAGE;
    const uint8_t* tbase = desc4 + R.row0 * ROWB;
    const int32_t* kbase = keyc + R.row0;
    auto stage = [&](int s, int buf) {
        char* base = lds + buf * BUF_BYTES;
#pragma unroll
        for (int i = 0; i < GLDS; ++i) {
            const int p = i * WAVES * 64 + threadIdx.x;
            const int rr = p >> 3, slot = p & 7, c = slot ^ ((rr >> 1) & 7);
            const uint8_t* gp = tbase + (int64_t)(s * STAGE + rr) * ROWB + 16 * c;
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)gp,
                                             (LDS_AS void*)(base + (i * WAVES + wid) * 1024), 16, 0, 0);
        }
        if (wid < STAGE / 64)
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(kbase + s * STAGE + wid * 64 + lane),
                                             (LDS_AS void*)(base + DESC_BYTES + wid * 256), 4, 0, 0);
    };
    auto i8of = [](const i32x4& v) { return i32x8{v.x, v.y, v.z, v.w, 0, 0, 0, 0}; };

    if (nstages > 0) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int s = 0; s < nstages; ++s) {
        const int buf = s & 1;
        if (s + 1 < nstages) stage(s + 1, buf ^ 1);
        const char* base = lds + buf * BUF_BYTES;
#pragma unroll
        for (int t = 0; t < STAGE / 32; ++t) {
            i32x4 a[2][2];
            f32x4 cinit[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int row = t * 32 + b * 16 + l16;
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int slot = (4 * m + g) ^ ((row >> 1) & 7);
                    a[b][m] = *reinterpret_cast<const i32x4*>(base + row * ROWB + 16 * slot);
                }
                cinit[b] = *reinterpret_cast<const f32x4*>(base + DESC_BYTES + 4 * (t * 32 + b * 16 + 4 * g));
            }
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                f32x4 acc[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    acc[b] = fp6::mfma16<fp6::FMT_E2M1, false>(i8of(a[b][0]), i8of(bq[qt][0]), cinit[b]);
                    acc[b] = fp6::mfma16<fp6::FMT_E2M1, false>(i8of(a[b][1]), i8of(bq[qt][1]), acc[b]);
                }
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int r = 0; r < 4; r += 2) {
                        const float ka = acc[b][r], kb = acc[b][r + 1];
                        c2[qt] = fmaxf(__builtin_amdgcn_fmed3f(c1[qt], ka, kb), c2[qt]);
                        c1[qt] = fmaxf(c1[qt], fmaxf(ka, kb));
                    }
            }
        }
        if ((s % SPC) == SPC - 1 || s + 1 == nstages) {      // end of a key chunk
            const int cb = (s / SPC) * CHUNK;
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                float m1 = c1[qt], m2 = c2[qt];
#pragma unroll
                for (int o = 16; o <= 32; o <<= 1) {
                    const float p1 = __shfl_xor(m1, o), p2 = __shfl_xor(m2, o);
                    m2 = fmaxf(fminf(m1, p1), fmaxf(m2, p2));
                    m1 = fmaxf(m1, p1);
                }
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const float v = e == 0 ? m1 : m2;
                    if (v >= KEY_FLOOR) {
                        const float ip = __builtin_floorf(v);
                        const int dot = (int)ip - 767;
                        const int t_ = (256 - dot) >> 1;
                        const int j_ = cb + 16383 - (int)((v - ip) * 16384.0f);
                        if (t_ < T2[qt]) {
                            if (t_ < T1[qt]) { T2[qt] = T1[qt]; J2[qt] = J1[qt]; T1[qt] = t_; J1[qt] = j_; }
                            else { T2[qt] = t_; J2[qt] = j_; }
                        }
                    }
                }
                c1[qt] = c2[qt] = 0.f;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const int qi = qrow[qt];
        if (g != 0 || qi < 0) continue;
        const int64_t o = P.dense_base + qi;
        if (nt == 0) { out_idx[o] = -1; out_dist[o] = 0.f; continue; }
        const float d1 = (float)T1[qt], d2 = (float)T2[qt];
        out_idx[o] = lowe_select(J1[qt], d1, d2, nt, ratio);
        out_dist[o] = d1;
    }
}

// Two-pass ORB ratio test, pass 1: the SIFT screening argument on the FP4 path.
// The accumulator acc = keyc_j + dot (orb_mfma_kernel) is exact, floor(acc) - 767
// = dot = 256 - 2 hamming; each lane keeps the max over 4 disjoint row subsets
// per query tile (one v_max3_f32 per two elements), 16 subsets per query with the
// other 3 lanes of its column.  The best two subset maxima K1 >= K2 are two
// different rows, so hamming d1 (of K1) is the true best and d2' (of K2) >= the
// true second best; Lowe's test is non-decreasing in d2, so when it fails at
// (d1, d2') it fails for the true pair and the query is rejected exactly.  Every
// other query goes to its pair's qlist for orb_mfma16_kernel<GATHER>.
template <int QT, int WAVES, int MINW, int STAGE, bool SUBSET = false, bool PERSIST = false>
__global__ __launch_bounds__(WAVES * 64, MINW)
void orb_screen16_kernel(const WorkItem* __restrict__ work, const PairDev* __restrict__ pairs,
                         const ImgDev* __restrict__ imgs, const uint8_t* __restrict__ desc4,
                         const int32_t* __restrict__ keyc, int32_t* __restrict__ out_idx,
                         float* __restrict__ out_dist, int32_t* __restrict__ qlist, int32_t* __restrict__ qcount,
                         double ratio, int32_t* __restrict__ qmask = nullptr,
                         unsigned long long* __restrict__ top2 = nullptr, int32_t* __restrict__ ticket = nullptr,
                         int n_work = 0) {
    constexpr int ROWB = 128;
    constexpr int GLDS = STAGE * ROWB / (WAVES * 64 * 16);
    static_assert(GLDS * WAVES * 64 * 16 == STAGE * ROWB, "stage must split into whole 16-B pieces");
    static_assert(QT * WAVES * 16 == 512, "work items are 512 queries");
    constexpr int DESC_BYTES = STAGE * ROWB;
    constexpr int BUF_BYTES = DESC_BYTES + STAGE * 4;
    constexpr float KEY_FLOOR = 256.f;                      // real keys >= 511, pad rows 0
    __shared__ __attribute__((aligned(16))) char lds[2 * BUF_BYTES];

    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
    __shared__ int item_sh;
    for (int round = 0;; ++round) {
    int wi;
    if constexpr (PERSIST) {
        if (threadIdx.x == 0) item_sh = xcd_ticket(ticket, n_work);
        __syncthreads();
        wi = item_sh;
        if (wi < 0) break;
    } else {
        if (round > 0) break;
        wi = xcd_remap(blockIdx.x, gridDim.x);
    }
    const WorkItem w = work[wi];
    const PairDev P = pairs[w.pair];
    const ImgDev L = imgs[P.left], R = imgs[P.right];
    const int nq = L.rows, nt = R.rows;
    const int qbase = w.q0 + wid * (QT * 16);

    i32x4 bq[QT][2];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const i32x4* src = reinterpret_cast<const i32x4*>(desc4 + (L.row0 + qbase + qt * 16 + l16) * ROWB);
#pragma unroll
        for (int m = 0; m < 2; ++m) bq[qt][m] = src[4 * m + g];
    }
    float ch[QT][4];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int i = 0; i < 4; ++i) ch[qt][i] = 0.f;

    const int nstages = (nt + STAGE - 1) / STAGE;
    const uint8_t* tbase = desc4 + R.row0 * ROWB;
    const int32_t* kbase = keyc + R.row0;
    auto stage = [&](int s, int buf) {
        char* base = lds + buf * BUF_BYTES;
#pragma unroll
        for (int i = 0; i < GLDS; ++i) {
            const int p = i * WAVES * 64 + threadIdx.x;
            const int rr = p >> 3, slot = p & 7, c = slot ^ ((rr >> 1) & 7);
            const uint8_t* gp = tbase + (int64_t)(s * STAGE + rr) * ROWB + 16 * c;
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)gp,
                                             (LDS_AS void*)(base + (i * WAVES + wid) * 1024), 16, 0, 0);
        }
        if (wid < STAGE / 64)
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(kbase + s * STAGE + wid * 64 + lane),
                                             (LDS_AS void*)(base + DESC_BYTES + wid * 256), 4, 0, 0);
    };
    auto i8of = [](const i32x4& v) { return i32x8{v.x, v.y, v.z, v.w, 0, 0, 0, 0}; };

    if (nstages > 0) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int s = 0; s < nstages; ++s) {
        const int buf = s & 1;
        if (s + 1 < nstages) stage(s + 1, buf ^ 1);
        const char* base = lds + buf * BUF_BYTES;
#pragma unroll
        for (int t = 0; t < STAGE / 32; ++t) {
            i32x4 a[2][2];
            f32x4 cinit[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int row = t * 32 + b * 16 + l16;
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int slot = (4 * m + g) ^ ((row >> 1) & 7);
                    a[b][m] = *reinterpret_cast<const i32x4*>(base + row * ROWB + 16 * slot);
                }
                cinit[b] = *reinterpret_cast<const f32x4*>(base + DESC_BYTES + 4 * (t * 32 + b * 16 + 4 * g));
            }
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                f32x4 acc[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    acc[b] = fp6::mfma16<fp6::FMT_E2M1, false>(i8of(a[b][0]), i8of(bq[qt][0]), cinit[b]);
                    acc[b] = fp6::mfma16<fp6::FMT_E2M1, false>(i8of(a[b][1]), i8of(bq[qt][1]), acc[b]);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) ch[qt][i] = fmaxf(fmaxf(ch[qt][i], acc[0][i]), acc[1][i]);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        float k1 = 0.f, k2 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float v = ch[qt][i];
            k2 = fmaxf(k2, fminf(k1, v));
            k1 = fmaxf(k1, v);
        }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float p1 = __shfl_xor(k1, o), p2 = __shfl_xor(k2, o);
            k2 = fmaxf(fminf(k1, p1), fmaxf(k2, p2));
            k1 = fmaxf(k1, p1);
        }
        // SUBSET: subsets whose best Hamming distance is <= the second subset's (integer part of
        // the key): a row of any other subset is strictly farther than two distinct rows
        int mask = 0xFFFF;
        if constexpr (SUBSET) {
            const float f2 = __builtin_floorf(k2);
            int nib = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) nib |= (__builtin_floorf(ch[qt][i]) >= f2 ? 1 : 0) << i;
            int mk = nib << (4 * g);
            mk |= __shfl_xor(mk, 16);
            mk |= __shfl_xor(mk, 32);
            if (nt >= 2 && k2 >= KEY_FLOOR) mask = mk;
        }
        const int qi = qbase + qt * 16 + l16;
        if (g != 0 || qi >= nq) continue;
        const int64_t o = P.dense_base + qi;
        if (nt == 0) { out_idx[o] = -1; out_dist[o] = 0.f; continue; }
        bool reject = false;
        if (nt >= 2 && k2 >= KEY_FLOOR) {
            const int d1 = (256 - ((int)__builtin_floorf(k1) - 767)) >> 1;
            const int d2 = (256 - ((int)__builtin_floorf(k2) - 767)) >> 1;
            reject = !((double)(float)d1 < (double)(float)d2 * ratio);
        }
        if (reject) {
            out_idx[o] = -1;
            out_dist[o] = 0.f;
        } else {
            const int slot = atomicAdd(&qcount[w.pair], 1);
            qlist[P.dense_base + slot] = qi;
            if constexpr (SUBSET) {
                qmask[P.dense_base + slot] = mask;
                top2[2 * o] = ~0ull;
                top2[2 * o + 1] = ~0ull;
            }
            out_idx[o] = UNSETTLED;   // pass 2 must overwrite it (assemble counts survivors)
        }
    }
    __syncthreads();   // the next item restages the LDS buffers and rewrites item_sh
    }
}

// ORB pass 2, subset form (default): as sift_subset_kernel, on the FP4 +-1 rows with
// v_mfma_f32_16x16x128_f8f6f4.  Subset r's rows j = r + 16 i get the C-operand key
// 767 + (16383 - i) / 16384 (the local index keeps j's order), so a lane's float top-2 (v_med3_f32 /
// v_max_f32) ranks (Hamming distance, j) exactly; one 16-query tile per wave pair of blocks.  The
// (query, subset) top-2 is merged into the query's pair of 64-bit keys (d << 32) | j with atomicMin
// (sift_subset_kernel); orb_settle_kernel writes the results.
template <int WAVES, int QT>
__global__ __launch_bounds__(WAVES * 64, 2)
void orb_subset_kernel(const PairDev* __restrict__ pairs, const ImgDev* __restrict__ imgs,
                       const uint8_t* __restrict__ desc4, const int32_t* __restrict__ qlist,
                       const int32_t* __restrict__ qmask, const int32_t* __restrict__ qcount,
                       const int32_t* __restrict__ porder, unsigned long long* __restrict__ top2) {
    constexpr int ROWB = 128;
    constexpr int CH = 256;                   // rows per LDS chunk
    constexpr int QC = WAVES * QT * 16;       // queries per tile group
    constexpr int WIN = 1024;
    constexpr int GLDS = CH * ROWB / (WAVES * 64 * 16);
    static_assert(GLDS * WAVES * 64 * 16 == CH * ROWB, "chunk must split into whole 16-B pieces");
    constexpr float KEY_FLOOR = 256.f;
    __shared__ __attribute__((aligned(16))) char rows_lds[CH * ROWB];
    __shared__ float keys_lds[CH];
    __shared__ int ql[WIN];
    __shared__ int s_n;

    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63, g = lane >> 4, l16 = lane & 15;
    const int item = xcd_remap(blockIdx.x, gridDim.x);
    const int pi = porder[item >> 4], r = item & 15;
    const int cnt = qcount[pi];
    const PairDev P = pairs[pi];
    const ImgDev L = imgs[P.left], R = imgs[P.right];
    const int nt = R.rows;
    const int nr = R.rows_pad >> 4;
    if (cnt == 0 || r >= nt) return;
    const int32_t* qls = qlist + P.dense_base;
    const int32_t* qms = qmask + P.dense_base;
    auto i8of = [](const i32x4& v) { return i32x8{v.x, v.y, v.z, v.w, 0, 0, 0, 0}; };

    for (int e0 = 0; e0 < cnt; e0 += WIN) {
        if (tid == 0) s_n = 0;
        __syncthreads();
        for (int e = e0 + tid; e < min(cnt, e0 + WIN); e += WAVES * 64)
            if ((qms[e] >> r) & 1) ql[atomicAdd(&s_n, 1)] = qls[e];
        __syncthreads();
        const int n = s_n;
        for (int g0 = 0; g0 < n; g0 += QC) {
            int qrow[QT];
            i32x4 bq[QT][2];
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                const int qe = g0 + (wid * QT + qt) * 16 + l16;
                qrow[qt] = qe < n ? ql[qe] : -1;
                const i32x4* src = reinterpret_cast<const i32x4*>(desc4 + (L.row0 + (qrow[qt] < 0 ? 0 : qrow[qt])) * ROWB);
#pragma unroll
                for (int m = 0; m < 2; ++m) bq[qt][m] = src[4 * m + g];
            }
            const bool active = g0 + wid * QT * 16 < n;   // wave-uniform
            float c1[QT], c2[QT];
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) c1[qt] = c2[qt] = 0.f;
            for (int c0 = 0; c0 < nr; c0 += CH) {
                const int rows = min(CH, nr - c0);   // a multiple of 32
                __syncthreads();
#pragma unroll
                for (int u = 0; u < GLDS; ++u) {
                    const int p = u * WAVES * 64 + tid;
                    const int rr = p >> 3, slot = p & 7, c = slot ^ ((rr >> 1) & 7);
                    const int j = r + 16 * (c0 + (rr < rows ? rr : 0));
                    const uint8_t* gp = desc4 + (R.row0 + j) * ROWB + 16 * c;
                    __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)gp,
                                                     (LDS_AS void*)(rows_lds + (u * WAVES + wid) * 1024), 16, 0, 0);
                }
                for (int i = tid; i < CH; i += WAVES * 64) {
                    const int li = c0 + i, j = r + 16 * li;
                    keys_lds[i] = (i < rows && j < nt) ? (float)(767 * 16384 + 16383 - li) * (1.0f / 16384.0f) : 0.f;
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (active) {
                    for (int t = 0; t < rows / 32; ++t) {
                        i32x4 a[2][2];
                        f32x4 cinit[2];
#pragma unroll
                        for (int b = 0; b < 2; ++b) {
                            const int row = t * 32 + b * 16 + l16;
#pragma unroll
                            for (int m = 0; m < 2; ++m) {
                                const int slot = (4 * m + g) ^ ((row >> 1) & 7);
                                a[b][m] = *reinterpret_cast<const i32x4*>(rows_lds + row * ROWB + 16 * slot);
                            }
                            cinit[b] = *reinterpret_cast<const f32x4*>(keys_lds + t * 32 + b * 16 + 4 * g);
                        }
#pragma unroll
                        for (int qt = 0; qt < QT; ++qt) {
                            f32x4 acc[2];
#pragma unroll
                            for (int b = 0; b < 2; ++b) {
                                acc[b] = fp6::mfma16<fp6::FMT_E2M1, false>(i8of(a[b][0]), i8of(bq[qt][0]), cinit[b]);
                                acc[b] = fp6::mfma16<fp6::FMT_E2M1, false>(i8of(a[b][1]), i8of(bq[qt][1]), acc[b]);
                            }
#pragma unroll
                            for (int b = 0; b < 2; ++b)
#pragma unroll
                                for (int q = 0; q < 4; q += 2) {
                                    const float ka = acc[b][q], kb = acc[b][q + 1];
                                    c2[qt] = fmaxf(__builtin_amdgcn_fmed3f(c1[qt], ka, kb), c2[qt]);
                                    c1[qt] = fmaxf(c1[qt], fmaxf(ka, kb));
                                }
                        }
                    }
                }
            }
            if (active) {
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    float m1 = c1[qt], m2 = c2[qt];
#pragma unroll
                    for (int o = 16; o <= 32; o <<= 1) {
                        const float p1 = __shfl_xor(m1, o), p2 = __shfl_xor(m2, o);
                        m2 = fmaxf(fminf(m1, p1), fmaxf(m2, p2));
                        m1 = fmaxf(m1, p1);
                    }
                    if (g != 0 || qrow[qt] < 0) continue;
                    unsigned long long* bp = top2 + 2 * (P.dense_base + qrow[qt]);
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const float v = e == 0 ? m1 : m2;
                        if (v < KEY_FLOOR) continue;
                        const float ip = __builtin_floorf(v);
                        const int d = (256 - ((int)ip - 767)) >> 1;
                        const int li = 16383 - (int)((v - ip) * 16384.0f);
                        const unsigned long long k = ((unsigned long long)d << 32) | (unsigned)(r + 16 * li);
                        const unsigned long long old = atomicMin(bp, k);
                        atomicMin(bp + 1, old > k ? old : k);
                    }
                }
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256)
void orb_settle_kernel(const PairDev* __restrict__ pairs, const ImgDev* __restrict__ imgs,
                       const int32_t* __restrict__ qlist, const int32_t* __restrict__ qcount,
                       const unsigned long long* __restrict__ top2, int32_t* __restrict__ out_idx,
                       float* __restrict__ out_dist, double ratio, const int32_t* __restrict__ porder = nullptr) {
    const int pi = porder ? porder[blockIdx.x] : (int)blockIdx.x;   // porder: one batch's pairs (overlapped pass 2)
    const int cnt = qcount[pi];
    if (cnt == 0) return;
    const PairDev P = pairs[pi];
    const int nt = imgs[P.right].rows;
    for (int e = threadIdx.x; e < cnt; e += 256) {
        const int qi = qlist[P.dense_base + e];
        const int64_t o = P.dense_base + qi;
        const unsigned long long b0 = top2[2 * o], b1 = top2[2 * o + 1];
        if (b0 == ~0ull || (nt >= 2 && b1 == ~0ull)) {
            if (nt == 0) { out_idx[o] = -1; out_dist[o] = 0.f; }   // an empty train image: no neighbour
            // otherwise pass 2 left a flagged subset unscanned: the UNSETTLED stamp stays, so
            // assemble_kernel counts the query and the run fails (SFMX_EINTERNAL), never a lost match
            continue;
        }
        const float d1 = (float)(int)(b0 >> 32), d2 = nt >= 2 ? (float)(int)(b1 >> 32) : 0.f;
        out_idx[o] = lowe_select((int)(b0 & 0xffffffffu), d1, d2, nt, ratio);
        out_dist[o] = d1;
    }
}

// ---------------------------------------------------------------------------
// ORB Hamming 2-NN on the VALU (8 x v_xor + 8 x v_bcnt per pair, no MFMA).
// 4 waves x 2 queries per lane = 512 queries per block; train rows stream
// through LDS (256 rows = 8 KiB per stage, broadcast ds_read_b128).
// key = (d << 23) | j (unsigned), top-2 by min: v_med3_u32 + v_min_u32.
template <int QPL>
__global__ __launch_bounds__(256, 2)
void orb_knn2_kernel(const WorkItem* __restrict__ work, const PairDev* __restrict__ pairs,
                     const ImgDev* __restrict__ imgs, const uint8_t* __restrict__ desc8,
                     int32_t* __restrict__ out_idx, float* __restrict__ out_dist, double ratio) {
    constexpr int STAGE = 256;
    constexpr int BUF = STAGE * ORB_BYTES;   // 8 KiB
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * BUF];
    const int wid = threadIdx.x >> 6;
    const WorkItem w = work[xcd_remap(blockIdx.x, gridDim.x)];
    const PairDev P = pairs[w.pair];
    const ImgDev L = imgs[P.left], R = imgs[P.right];
    const int nq = L.rows, nt = R.rows;

    u32x4 q[QPL][2];
#pragma unroll
    for (int e = 0; e < QPL; ++e) {
        const int qi = w.q0 + e * 256 + threadIdx.x;
        const u32x4* src = reinterpret_cast<const u32x4*>(desc8 + (L.row0 + qi) * ORB_BYTES);
        q[e][0] = src[0]; q[e][1] = src[1];
    }
    unsigned b1[QPL], b2[QPL];
#pragma unroll
    for (int e = 0; e < QPL; ++e) b1[e] = b2[e] = 0xffffffffu;

    const uint8_t* tbase = desc8 + R.row0 * ORB_BYTES;
    const int nstages = (nt + STAGE - 1) / STAGE;
    auto stage = [&](int s, int buf) {
        uint8_t* base = lds + buf * BUF;
#pragma unroll
        for (int i = 0; i < 2; ++i) {   // 2 x (256 threads x 16 B) = 8 KiB
            const uint8_t* g = tbase + (int64_t)s * BUF + i * 4096 + threadIdx.x * 16;
            __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)g, (LDS_AS void*)(base + i * 4096 + wid * 1024), 16, 0, 0);
        }
    };
    if (nstages > 0) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int s = 0; s < nstages; ++s) {
        const int buf = s & 1;
        if (s + 1 < nstages) stage(s + 1, buf ^ 1);
        const u32x4* tl = reinterpret_cast<const u32x4*>(lds + buf * BUF);
        const int lim = min(STAGE, nt - s * STAGE);
        const unsigned j0 = (unsigned)(s * STAGE);
        for (int jj = 0; jj < lim; ++jj) {
            const u32x4 t0 = tl[2 * jj], t1 = tl[2 * jj + 1];
#pragma unroll
            for (int e = 0; e < QPL; ++e) {
                unsigned d = __builtin_popcount(q[e][0].x ^ t0.x);
                d += __builtin_popcount(q[e][0].y ^ t0.y);
                d += __builtin_popcount(q[e][0].z ^ t0.z);
                d += __builtin_popcount(q[e][0].w ^ t0.w);
                d += __builtin_popcount(q[e][1].x ^ t1.x);
                d += __builtin_popcount(q[e][1].y ^ t1.y);
                d += __builtin_popcount(q[e][1].z ^ t1.z);
                d += __builtin_popcount(q[e][1].w ^ t1.w);
                const unsigned key = (d << 23) | (j0 + jj);
                b2[e] = med3u(b1[e], b2[e], key);
                b1[e] = min(b1[e], key);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < QPL; ++e) {
        const int qi = w.q0 + e * 256 + threadIdx.x;
        if (qi >= nq) continue;
        const int64_t o = P.dense_base + qi;
        if (nt == 0) { out_idx[o] = -1; out_dist[o] = 0.f; continue; }
        const float d1 = (float)(b1[e] >> 23), d2 = (float)(b2[e] >> 23);
        out_idx[o] = lowe_select((int)(b1[e] & 0x7fffffu), d1, d2, nt, ratio);
        out_dist[o] = d1;
    }
}

// ---------------------------------------------------------------------------
// Match-graph assembly: per pair (one 1024-thread block), optional distinct
// filter (trainIdx seen/dup bitsets in LDS, SfM.cpp:547-564), count, min_count
// keep flag (SfM.cpp:566-570), then a second launch writes packed DMatch in
// query order at the scanned pair offset.
// mode 0: count -> counts[p], keep[p];  mode 1: write packed matches.
// The pieces are device functions (blocks of 1024 threads = 16 waves) shared with the list-path
// kernels below, which run them for the pairs that go through the dense arrays.
__device__ __forceinline__ void mark_seen(unsigned* bits, int words, int j) {   // seen | dup bitsets
    const unsigned bit = 1u << (j & 31);
    const unsigned old = atomicOr(&bits[j >> 5], bit);
    if (old & bit) atomicOr(&bits[words + (j >> 5)], bit);
}
__device__ __forceinline__ void dense_dup_bits(unsigned* bits, const int32_t* __restrict__ ix, int nq, int words) {
    for (int i = threadIdx.x; i < 2 * words; i += blockDim.x) bits[i] = 0;
    __syncthreads();
    for (int q = threadIdx.x; q < nq; q += blockDim.x) {
        const int j = ix[q];
        if (j >= 0) mark_seen(bits, words, j);
    }
    __syncthreads();
}
// one read of the pair's results: per-thread counts, one block reduction
__device__ __forceinline__ void dense_count(const unsigned* bits, int* sh, const int32_t* __restrict__ ix, int nq, int words,
                                            int distinct, int min_count, int p, int64_t* __restrict__ counts,
                                            int32_t* __restrict__ keep, int32_t* __restrict__ unsettled) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int cnt = 0, bad = 0;
    for (int q = threadIdx.x; q < nq; q += blockDim.x) {
        int j = ix[q];
        bad += j == UNSETTLED;
        if (j >= 0 && distinct && (bits[words + (j >> 5)] >> (j & 31)) & 1u) j = -1;
        cnt += j >= 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o); bad += __shfl_xor(bad, o); }
    if (lane == 0) { sh[wid] = cnt; sh[16 + wid] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0, b = 0;
        for (int i = 0; i < 16; ++i) { run += sh[i]; b += sh[16 + i]; }
        if (b) atomicAdd(unsettled, b);
        counts[p] = run;
        keep[p] = run < min_count ? 0 : 1;
    }
}
// rank within the wave by ballot, wave totals through LDS (two sets, by the round's
// parity: a wave is at most one round ahead of the slowest one, so one barrier per round)
__device__ __forceinline__ void dense_write(const unsigned* bits, int* sh, const int32_t* __restrict__ ix,
                                            const float* __restrict__ dx, int nq, int words, int distinct, int64_t run,
                                            DMatchDev* __restrict__ out) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int q0 = 0, it = 0; q0 < nq; q0 += blockDim.x, it ^= 1) {
        const int q = q0 + threadIdx.x;
        int j = q < nq ? ix[q] : -1;
        if (j >= 0 && distinct && (bits[words + (j >> 5)] >> (j & 31)) & 1u) j = -1;
        const unsigned long long bal = __ballot(j >= 0);
        if (lane == 0) sh[16 * it + wid] = __popcll(bal);
        __syncthreads();
        int wbase = 0, total = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int v = sh[16 * it + i];
            wbase += i < wid ? v : 0;
            total += v;
        }
        if (j >= 0) out[run + wbase + __popcll(bal & ((1ull << lane) - 1ull))] = DMatchDev{q, j, 0, dx[q]};
        run += total;
    }
}

template <int MODE>
__global__ __launch_bounds__(1024)
void assemble_kernel(const PairDev* __restrict__ pairs, const ImgDev* __restrict__ imgs,
                     const int32_t* __restrict__ out_idx, const float* __restrict__ out_dist,
                     int distinct, int min_count, int64_t* __restrict__ counts, int32_t* __restrict__ keep,
                     const int64_t* __restrict__ offsets, DMatchDev* __restrict__ out, int32_t* __restrict__ unsettled) {
    extern __shared__ __attribute__((aligned(16))) unsigned bits[];   // seen | dup bitsets (distinct only)
    __shared__ int sh[32];
    const int p = blockIdx.x;
    const PairDev P = pairs[p];
    const int nq = imgs[P.left].rows, nt = imgs[P.right].rows;
    const int words = (nt + 31) >> 5;
    const int32_t* ix = out_idx + P.dense_base;
    if (distinct) dense_dup_bits(bits, ix, nq, words);
    if (MODE == 0) dense_count(bits, sh, ix, nq, words, distinct, min_count, p, counts, keep, unsettled);
    else dense_write(bits, sh, ix, out_dist + P.dense_base, nq, words, distinct, offsets[p], out);
}

// ---------------------------------------------------------------------------
// List path (product SIFT): settle and assemble from the forwarded lists.  Only a query the screen
// forwarded can become a match, and its whole state sits at its list slot e (qlist, qmask, top2,
// slot1 at dense_base + e), so nothing below touches a per-row array.  One 1024-thread workgroup per
// pair, from the pair's flat record; a pair whose record says lists = 0 (fp32 fallback) is counted
// and written from the dense arrays by the functions above, so one run can hold both kinds.
//
// sift_finish_kernel, per slot: merge the two-slot or atomic top-2 (see sift_subset_kernel), Lowe's
// test, and the result (j or -1, distance bits) over the first 8 B of the slot's top2 word.  Queries
// in the float-sqrt collision range are listed (in the pair's part of slow_list) and re-ranked after
// a barrier, one wave each.  Then the distinct filter and the count: with the seen / dup bitsets a
// train row is matched exactly once iff seen and not dup, so the count is a popcount over the words.
// A slot pass 2 never wrote counts as unsettled (the run fails in fetch / stats).
__global__ __launch_bounds__(1024)
void sift_finish_kernel(const PairRec* __restrict__ recs, const int32_t* __restrict__ qlist,
                        const int32_t* __restrict__ qmask, const int32_t* __restrict__ qcount,
                        unsigned long long* __restrict__ top2, const unsigned long long* __restrict__ slot1,
                        int2* __restrict__ slow_list, int32_t* __restrict__ slow_count,
                        const int8_t* __restrict__ desc8, const int32_t* __restrict__ norm,
                        const int32_t* __restrict__ out_idx, double ratio, int distinct, int min_count,
                        int64_t* __restrict__ counts, int32_t* __restrict__ keep, int32_t* __restrict__ unsettled) {
    extern __shared__ __attribute__((aligned(16))) unsigned bits[];   // seen | dup bitsets (distinct only)
    __shared__ int sh[32];
    __shared__ int s_slow;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const PairRec R = recs[blockIdx.x];
    const int nt = R.nt, words = (nt + 31) >> 5;
    if (!R.lists) {
        const int32_t* ix = out_idx + R.dense_base;
        if (distinct) dense_dup_bits(bits, ix, R.nq, words);
        dense_count(bits, sh, ix, R.nq, words, distinct, min_count, R.pair, counts, keep, unsettled);
        return;
    }
    const int cnt = qcount[R.pair];
    if (cnt == 0) {
        if (tid == 0) { counts[R.pair] = 0; keep[R.pair] = 0 < min_count ? 0 : 1; }
        return;
    }
    if (tid == 0) s_slow = 0;
    if (distinct)
        for (int i = tid; i < 2 * words; i += 1024) bits[i] = 0;
    __syncthreads();
    const int32_t* qls = qlist + R.dense_base;
    const int32_t* qms = qmask + R.dense_base;
    unsigned long long* t2 = top2 + 2 * R.dense_base;
    const unsigned long long* s1p = slot1 + 2 * R.dense_base;
    int2* sl = slow_list + R.dense_base;
    int acc = 0, bad = 0;
    for (int e = tid; e < cnt; e += 1024) {
        const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(t2 + 2 * e);
        unsigned long long b0 = a.x, b1 = a.y;
        const int mk = qms[e];
        if (__popc(mk) == 2) {   // two subsets, one 16-B word each: merge the two top-2
            const ulonglong2 c = *reinterpret_cast<const ulonglong2*>(s1p + 2 * e);
            const unsigned long long lo = b0 < c.x ? b0 : c.x, hi = b0 < c.x ? c.x : b0, m2 = b1 < c.y ? b1 : c.y;
            b0 = lo;
            b1 = hi < m2 ? hi : m2;
        }
        int j = -1;
        float d1 = 0.f;
        if (b0 == ~0ull || (nt >= 2 && b1 == ~0ull)) {
            bad += nt != 0;   // pass 2 left a flagged subset unscanned
        } else {
            const int64_t s1 = (int64_t)(b0 >> 32);
            int64_t s2 = (int64_t)(b1 >> 32);
            // one bit (a subset bit): certified by fp6::certified, (b0, b1) the exact top-2 of that subset alone.
            // Some row outside it has s in [lo, hi], hi < SQRT_SAFE, and Lowe's test passes at every s2 >= lo:
            // at the true s2 = min(b1's, s_other) it fails exactly when it fails at b1's clamped below SQRT_SAFE.
            if (__popc(mk) == 1 && mk < QMASK_FULL_ROUTE) s2 = s2 < SQRT_SAFE ? s2 : SQRT_SAFE - 1;
            if (nt >= 2 && s2 >= SQRT_SAFE) {
                sl[atomicAdd(&s_slow, 1)] = make_int2(e, qls[e]);
                continue;
            }
            d1 = sqrt_rn_int(s1);
            j = lowe_select((int)(b0 & 0xffffffffu), d1, nt >= 2 ? sqrt_rn_int(s2) : 0.f, nt, ratio);
        }
        *reinterpret_cast<int2*>(t2 + 2 * e) = make_int2(j, __float_as_int(d1));
        if (j >= 0) {
            if (distinct) mark_seen(bits, words, j);
            else ++acc;
        }
    }
    __syncthreads();
    const int n_slow = s_slow;
    for (int k = wid; k < n_slow; k += 16) {   // exact float-sqrt ranking, one wave per query
        const int2 it = sl[k];
        unsigned long long b1, b2;
        slow_top2(desc8, norm, R.lrow0 + it.y, R.rrow0, nt, lane, b1, b2);
        if (lane == 0) {
            const float d1 = __uint_as_float((unsigned)(b1 >> 32)), d2 = __uint_as_float((unsigned)(b2 >> 32));
            const int j = lowe_select((int)(b1 & 0xffffffffu), d1, d2, 2, ratio);   // slow path implies nt >= 2
            *reinterpret_cast<int2*>(t2 + 2 * it.x) = make_int2(j, __float_as_int(d1));
            if (j >= 0) {
                if (distinct) mark_seen(bits, words, j);
                else ++acc;
            }
        }
    }
    if (distinct) {
        __syncthreads();
        for (int i = tid; i < words; i += 1024) acc += __popc(bits[i] & ~bits[words + i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { acc += __shfl_xor(acc, o); bad += __shfl_xor(bad, o); }
    if (lane == 0) { sh[wid] = acc; sh[16 + wid] = bad; }
    __syncthreads();
    if (tid == 0) {
        int run = 0, b = 0;
        for (int i = 0; i < 16; ++i) { run += sh[i]; b += sh[16 + i]; }
        if (b) atomicAdd(unsettled, b);
        if (n_slow) atomicAdd(slow_count, n_slow);
        counts[R.pair] = run;
        keep[R.pair] = run < min_count ? 0 : 1;
    }
}

// assemble_lists_kernel: the pair's accepted slots -> packed DMatch at offsets[pair], in ascending
// query order whatever order the screen's atomics filled the list in: a bitmap of the accepted
// query rows in LDS (nq bits) with per-word prefix counts ranks each slot's query.
// LDS: bitmap[W] | prefix[W] | seen[words] | dup[words] (the last two with distinct only).
__global__ __launch_bounds__(1024)
void assemble_lists_kernel(const PairRec* __restrict__ recs, const int32_t* __restrict__ qlist,
                           const int32_t* __restrict__ qcount, const unsigned long long* __restrict__ top2,
                           const int32_t* __restrict__ out_idx, const float* __restrict__ out_dist, int distinct,
                           const int64_t* __restrict__ counts, const int64_t* __restrict__ offsets,
                           DMatchDev* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned bits[];
    __shared__ int sh[32];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const PairRec R = recs[blockIdx.x];
    const int words = (R.nt + 31) >> 5;
    if (!R.lists) {
        const int32_t* ix = out_idx + R.dense_base;
        if (distinct) dense_dup_bits(bits, ix, R.nq, words);
        dense_write(bits, sh, ix, out_dist + R.dense_base, R.nq, words, distinct, offsets[R.pair], out);
        return;
    }
    const int cnt = qcount[R.pair];
    if (cnt == 0 || counts[R.pair] == 0) return;
    const int W = (R.nq + 31) >> 5;
    unsigned* bm = bits;
    unsigned* pre = bits + W;
    unsigned* seen = bits + 2 * W;
    for (int i = tid; i < W; i += 1024) bm[i] = 0;
    if (distinct)
        for (int i = tid; i < 2 * words; i += 1024) seen[i] = 0;
    __syncthreads();
    const int32_t* qls = qlist + R.dense_base;
    const int2* res = reinterpret_cast<const int2*>(top2 + 2 * R.dense_base);   // slot e: res[2 e] = (j, distance bits)
    if (distinct) {
        for (int e = tid; e < cnt; e += 1024) {
            const int j = res[2 * e].x;
            if (j >= 0) mark_seen(seen, words, j);
        }
        __syncthreads();
    }
    for (int e = tid; e < cnt; e += 1024) {
        const int j = res[2 * e].x;
        if (j >= 0 && !(distinct && ((seen[words + (j >> 5)] >> (j & 31)) & 1u))) {
            const int qi = qls[e];
            atomicOr(&bm[qi >> 5], 1u << (qi & 31));
        }
    }
    __syncthreads();
    {   // exclusive prefix of the words' popcounts: each thread a contiguous run of words
        const int per = (W + 1023) / 1024, w0 = min(tid * per, W), w1 = min(w0 + per, W);
        int mine = 0;
        for (int w = w0; w < w1; ++w) mine += __popc(bm[w]);
        int incl = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        if (lane == 63) sh[wid] = incl;
        __syncthreads();
        int at = incl - mine;
        for (int i = 0; i < wid; ++i) at += sh[i];
        for (int w = w0; w < w1; ++w) { pre[w] = at; at += __popc(bm[w]); }
    }
    __syncthreads();
    DMatchDev* o = out + offsets[R.pair];
    for (int e = tid; e < cnt; e += 1024) {
        const int2 r = res[2 * e];
        if (r.x >= 0 && !(distinct && ((seen[words + (r.x >> 5)] >> (r.x & 31)) & 1u))) {
            const int qi = qls[e];
            const unsigned below = bm[qi >> 5] & ((1u << (qi & 31)) - 1u);
            o[pre[qi >> 5] + __popc(below)] = DMatchDev{qi, r.x, 0, __int_as_float(r.y)};
        }
    }
}

// offsets[0..n] = exclusive scan of counts (single block, 1024 threads).
__global__ __launch_bounds__(1024)
void scan_offsets_kernel(const int64_t* __restrict__ counts, int n, int64_t* __restrict__ offsets) {
    __shared__ long long sh[1024];
    long long run = 0;
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int i = c0 + threadIdx.x;
        const long long v = i < n ? counts[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const long long y = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += y;
            __syncthreads();
        }
        if (i < n) offsets[i] = run + sh[threadIdx.x] - v;
        run += sh[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[n] = run;
}

__global__ void selftest_sqrt_kernel(int64_t n, uint32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = __float_as_uint(sqrt_rn_int(i));
}

// ---------------------------------------------------------------------------
// Launch wrappers (host side, called by matcher.cpp).
hipError_t launch_selftest_sqrt(int64_t n, uint32_t* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    selftest_sqrt_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, out);
    return hipGetLastError();
}
hipError_t launch_prep_l2(const float* src, int rows, int cols, int rows_pad, int8_t* dst, int32_t* norm,
                          int32_t* keyc, int32_t* keyc2, int32_t* nonintegral, hipStream_t st) {
    if (rows_pad == 0) return hipSuccess;
    const int rows_per_block = 8;   // 256 threads
    prep_l2_kernel<<<(rows_pad + rows_per_block - 1) / rows_per_block, 256, 0, st>>>(src, rows, cols, rows_pad, dst, norm,
                                                                                      keyc, keyc2, nonintegral);
    return hipGetLastError();
}
hipError_t launch_prep_f32(const float* src, int rows, int cols, int rows_pad, float* dst, hipStream_t st) {
    const int64_t total = (int64_t)rows_pad * SIFT_DIM;
    if (total == 0) return hipSuccess;
    prep_f32_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(src, rows, cols, rows_pad, dst);
    return hipGetLastError();
}
hipError_t launch_prep_hamming(const uint8_t* src, int rows, int cols, int rows_pad, uint8_t* dst, hipStream_t st) {
    const int64_t total = (int64_t)rows_pad * ORB_BYTES;
    if (total == 0) return hipSuccess;
    prep_hamming_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(src, rows, cols, rows_pad, dst);
    return hipGetLastError();
}

// Kernel variants (queries per block = QT * WAVES * 32, must divide ROW_ALIGN).
// The product library runs only the default two-pass forms (variant 0: the FP6 screen with the exact pass 2
// over the certified row subset, or over every row where there is none, for SIFT; the FP4 screen with the
// subset pass 2 for ORB);
// the diagnostic build (diag.hpp) selects the others with SFMX_SIFT_VARIANT / SFMX_SIFT_P2,
// read per run so tests switch paths within one process.
int sift_variant() {
    const char* e = SFMX_DIAG_ENV("SFMX_SIFT_VARIANT");
    return e ? atoi(e) : 0;
}
int match_batches() {   // overlapped two-pass batches (1: one screen launch, then pass 2)
    const char* e = SFMX_DIAG_ENV("SFMX_MATCH_BATCHES");
    return e ? std::max(1, std::min(64, atoi(e))) : MATCH_BATCHES;
}
int pass2_variant() {   // 10 = subset pass 2 (default), else the full-row GATHER pass 2
    const char* e = SFMX_DIAG_ENV("SFMX_SIFT_P2");   // with that item size (0 / 2 = 128 queries)
    return e ? atoi(e) : 10;
}
// FP6 product path: the screen on 32 x 32 x 64 MFMAs (sift_screen6w_kernel) or on 16 x 16 x 128 ones
// (sift_screen6_kernel); SIFT_VARIANT_FP6_OTHER_SHAPE runs the one that is not the product (measured).
constexpr bool SIFT_SCREEN6_WIDE = false;
// FP6 product path: 32-query tiles a wave of sift_rows_kernel carries per pass over its subset's rows.  Two fit
// the 128 VGPRs of four waves per SIMD without scratch (126); three spill 13 registers.
constexpr int SIFT_ROWS_QT = 2;
// FP6 product path: resident workgroups assumed for the full-row launch where the occupancy query fails
// (256 CUs x 4), and (diagnostic build) SFMX_FULL_ROW_GRID, which sets that launch's grid (tests: several items
// per workgroup on a small job).
constexpr int SIFT_FULL_ROW_SLOTS = 1024;
int full_row_grid(int dflt) {
    const char* e = SFMX_DIAG_ENV("SFMX_FULL_ROW_GRID");
    return e ? std::max(1, atoi(e)) : dflt;
}
int sift_block_queries(int v) { return v == 2 || v == 4 || v == 23 ? 256 : 512; }

#define SIFT_LAUNCH(QT, W, MINW, ST, MF, ...)                                                             \
    sift_knn2_kernel<QT, W, MINW, ST, MF __VA_OPT__(,) __VA_ARGS__><<<n_work, W * 64, 0, st>>>(work, pairs, imgs, desc8, norm, keyc, \
                                                                     out_idx, out_dist, slow_list, slow_count, ratio)

// Resident workgroups of a kernel on the current device (the persistent screens' grid); 0 = unknown.
template <class F>
int resident_slots(F kernel, int threads) {
    int dev = 0, nb = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, threads, 0) != hipSuccess) return 0;
    return nb * prop.multiProcessorCount;
}
// SFMX_SCREEN_PERSIST=1 (diagnostic build only): the ticket-fed persistent screens.  A single global
// ticket measured slower in r04d (C2 6.85 vs 6.40 ms, C4 18.96 vs 17.44 ms per launch,
// profiles/r04d_ab.txt): items taken in list order landed on every XCD, so each XCD's L2 streamed every
// active train image, where the one-item-per-workgroup grid's XCD-contiguous mapping keeps a train image
// on one XCD.  Hence the per-XCD ranges and tickets of xcd_ticket (r04e A/B).
bool persist_screens() {
    const char* e = SFMX_DIAG_ENV("SFMX_SCREEN_PERSIST");
    return e && e[0] == '1';
}

hipError_t launch_sift_knn2(const WorkItem* work, int n_work, const PairDev* pairs, const ImgDev* imgs,
                            const int8_t* desc8, const int32_t* norm, const int32_t* keyc, const int32_t* keyc2,
                            int32_t* qlist, int32_t* qcount, int n_pairs, const int32_t* porder, WorkItem* work2,
                            int32_t* work2_n, int32_t* out_idx,
                            float* out_dist, int2* slow_list, int32_t* slow_count, double ratio, hipStream_t st,
                            hipEvent_t ev_screen, int32_t* qmask, unsigned long long* top2, unsigned long long* slot1,
                            bool lists, const uint32_t* desc6, const float* keyf, const int2* ne, const int32_t* imax) {
    if (n_work == 0) return hipSuccess;
    const int v = sift_variant();
    if (v == 0 || v >= 101) {   // two-pass ratio test: screen every query, exact kernel on the rest
        hipError_t e = hipSuccess;   // qcount and the screen's XCD tickets behind it: zeroed by the caller's one fill
        if (lists) {   // product path: pass-2 state at the list slots; the caller settles with launch_finish_lists
            if ((v != 0 && v != SIFT_VARIANT_INT8_LISTS && v != SIFT_VARIANT_FP6_FULL && v != SIFT_VARIANT_FP6_OTHER_SHAPE &&
                 v != SIFT_VARIANT_FP6_SUBSET_WG) ||
                pass2_variant() != 10 || !qmask || !top2)
                return hipErrorInvalidValue;
            if (v == 0 || v == SIFT_VARIANT_FP6_OTHER_SHAPE || v == SIFT_VARIANT_FP6_SUBSET_WG) {
                // conservative FP6 screen; exact pass 2 over the one certified row subset (one wave per pair
                // and subset: sift_rows_kernel; diagnostic build, SIFT_VARIANT_FP6_SUBSET_WG: one workgroup,
                // sift_subset_kernel), and over every train row for the queries of the second list (128-query
                // items).  The second list sits in `slot1`, idle here: no mask of this path has two bits.
                if (!desc6 || !keyf || !ne || !imax || !slot1) return hipErrorInvalidValue;
                int32_t* qlist2 = reinterpret_cast<int32_t*>(slot1);
                int32_t* qcount2 = qcount + arena_qcount2(n_pairs);
                // the screen's MFMA shape: the product's, or (diagnostic build) the other one
                if (SIFT_SCREEN6_WIDE != (v == SIFT_VARIANT_FP6_OTHER_SHAPE))
                    sift_screen6w_kernel<4, 2, 128, true><<<n_work, 256, 0, st>>>(work, pairs, imgs, desc6, keyf, ne, imax, qlist,
                                                                                 qcount, ratio, qmask, top2, qlist2, qcount2);
                else
                    sift_screen6_kernel<8, 4, 2, 128, true><<<n_work, 256, 0, st>>>(work, pairs, imgs, desc6, keyf, ne, imax, qlist,
                                                                                   qcount, ratio, qmask, top2, qlist2, qcount2);
                if (ev_screen) {
                    e = hipEventRecord(ev_screen, st);
                    if (e != hipSuccess) return e;
                }
                if (v == SIFT_VARIANT_FP6_SUBSET_WG)
                    sift_subset_kernel<4, true><<<n_pairs * 16, 256, 0, st>>>(pairs, imgs, desc8, norm, qlist, qmask, qcount, porder,
                                                                              top2, slot1, qcount2, SIFT_RIDE_MAX);
                else
                    sift_rows_kernel<SIFT_ROWS_QT><<<n_pairs * 4, 256, 0, st>>>(pairs, imgs, desc8, norm, qlist, qmask, qcount,
                                                                                 qcount2, porder, top2);
                compact_work_kernel<7><<<1, 1024, 0, st>>>(porder, n_pairs, qcount2, work2, work2_n, SIFT_RIDE_MAX);
                // the full-row items (work2 holds up to n_work << 2 of them; the count stays on the device): a
                // grid of two resident rounds, each workgroup looping over the list
                static const int slots = resident_slots(sift_knn2_kernel<1, 4, 2, 128, false, 0, 0, true, true, true>, 256);
                const int grid2 = std::min(n_work << 2, full_row_grid(2 * (slots > 0 ? slots : SIFT_FULL_ROW_SLOTS)));
                sift_knn2_kernel<1, 4, 2, 128, false, 0, 0, true, true, true><<<grid2, 256, 0, st>>>(
                    work2, pairs, imgs, desc8, norm, keyc, nullptr, nullptr, nullptr, nullptr, ratio, qlist, qcount2, work2_n,
                    top2, qlist2);
                return hipGetLastError();
            }
            if (v == SIFT_VARIANT_FP6_FULL) {   // (diagnostic build) FP6 screen, exact pass 2 over every train row for every forwarded query
                if (!desc6 || !keyf || !ne || !imax) return hipErrorInvalidValue;
                sift_screen6_kernel<8, 4, 2, 128, false><<<n_work, 256, 0, st>>>(work, pairs, imgs, desc6, keyf, ne, imax, qlist,
                                                                                qcount, ratio, qmask, top2, nullptr, nullptr);
                if (ev_screen) {
                    e = hipEventRecord(ev_screen, st);
                    if (e != hipSuccess) return e;
                }
                compact_work_kernel<7><<<1, 1024, 0, st>>>(porder, n_pairs, qcount, work2, work2_n);
                sift_knn2_kernel<1, 4, 2, 128, false, 0, 0, true, true><<<n_work << 2, 256, 0, st>>>(   // work2 holds n_work << 2 items
                    work2, pairs, imgs, desc8, norm, keyc, nullptr, nullptr, nullptr, nullptr, ratio, qlist, qcount, work2_n,
                    top2);
                return hipGetLastError();
            }
            // SIFT_VARIANT_INT8_LISTS (diagnostic build): the exact int8 screen with subset masks, subset pass 2
            sift_screen16_kernel<8, 4, 2, 64, true, false, true><<<n_work, 256, 0, st>>>(
                work, pairs, imgs, desc8, norm, keyc2, out_idx, out_dist, qlist, qcount, ratio, qmask, top2);
            if (ev_screen) {
                e = hipEventRecord(ev_screen, st);
                if (e != hipSuccess) return e;
            }
            sift_subset_kernel<4, true><<<n_pairs * 16, 256, 0, st>>>(pairs, imgs, desc8, norm, qlist, qmask, qcount, porder,
                                                                      top2, slot1);
            return hipGetLastError();
        }
        if (pass2_variant() == 10 && qmask && top2) {   // subset-restricted pass 2
            static const int slots = resident_slots(sift_screen16_kernel<8, 4, 2, 64, true, true>, 256);
            if (slots > 0 && persist_screens())
                sift_screen16_kernel<8, 4, 2, 64, true, true><<<std::min(n_work, slots), 256, 0, st>>>(
                    work, pairs, imgs, desc8, norm, keyc2, out_idx, out_dist, qlist, qcount, ratio, qmask, top2,
                    qcount + n_pairs, n_work);
            else
                sift_screen16_kernel<8, 4, 2, 64, true><<<n_work, 256, 0, st>>>(work, pairs, imgs, desc8, norm, keyc2, out_idx,
                                                                               out_dist, qlist, qcount, ratio, qmask, top2);
            if (ev_screen) {
                e = hipEventRecord(ev_screen, st);
                if (e != hipSuccess) return e;
            }
            sift_subset_kernel<4><<<n_pairs * 16, 256, 0, st>>>(pairs, imgs, desc8, norm, qlist, qmask, qcount, porder, top2, slot1);
            sift_settle_kernel<<<n_pairs, 256, 0, st>>>(pairs, imgs, qlist, qcount, top2, out_idx, out_dist, slow_list,
                                                        slow_count, ratio, qmask, slot1);
            return hipGetLastError();
        }
#ifndef SFMX_DIAG
        return hipErrorInvalidValue;   // the product path always has the subset buffers
    }
    return hipErrorInvalidValue;
#else
#define SCREEN_LAUNCH(QT, W, MINW, ST) \
    sift_screen_kernel<QT, W, MINW, ST><<<n_work, W * 64, 0, st>>>(work, pairs, imgs, desc8, norm, keyc2, out_idx, \
                                                                   out_dist, qlist, qcount, ratio)
#define SCREEN16_LAUNCH(QT, W, MINW, ST, ...) \
    sift_screen16_kernel<QT, W, MINW, ST __VA_OPT__(,) __VA_ARGS__><<<n_work, W * 64, 0, st>>>(work, pairs, imgs, desc8, norm, keyc2, out_idx, \
                                                                     out_dist, qlist, qcount, ratio)
        switch (v) {
        // every variant: 512 queries per work item (pass 2's).  r01f A/B on config 2 (kernel ms, both
        // passes): 64-row stages 8.31-8.41, 128-row 8.50-8.57, MINW 3 8.37-8.41, 2 x 8 waves 9.60-9.66
        case 101: SCREEN_LAUNCH(4, 4, 2, 128); break;
        case 102: SCREEN_LAUNCH(2, 8, 2, 128); break;
        case 104: SCREEN_LAUNCH(2, 8, 2, 64); break;
        case 105: SCREEN_LAUNCH(4, 4, 3, 64); break;
        case 103: SCREEN_LAUNCH(4, 4, 2, 64); break;       // r01f default (32x32x32 screen)
        // r01g A/B on config 2 (kernel ms, both passes, 2 runs): 103 8.24-8.27, 106 7.43-7.50,
        // 107 7.43-7.44, 108 8.60-8.61
        case 107: SCREEN16_LAUNCH(8, 4, 2, 128); break;
        case 108: SCREEN16_LAUNCH(4, 8, 2, 64); break;
        default: SCREEN16_LAUNCH(8, 4, 2, 64);             // 0 / 106
        }
#undef SCREEN_LAUNCH
#undef SCREEN16_LAUNCH
        if (ev_screen) {   // pass-1 / pass-2 split of the launch (sfmx_matcher_pass_timing)
            e = hipEventRecord(ev_screen, st);
            if (e != hipSuccess) return e;
        }
#define PASS2_LAUNCH(ISH, QT, W, MINW, ST)                                                                   \
    static_assert((1 << (ISH)) == (QT) * (W) * 32, "pass-2 item size must equal the queries one block covers"); \
    static_assert((ISH) >= 7 && (ISH) <= 9, "work2 holds n_work << 2 items: items of 128..512 queries");       \
    compact_work_kernel<ISH><<<1, 1024, 0, st>>>(porder, n_pairs, qcount, work2, work2_n);                  \
    sift_knn2_kernel<QT, W, MINW, ST, false, 0, 0, true><<<n_work << (9 - ISH), W * 64, 0, st>>>(             \
        work2, pairs, imgs, desc8, norm, keyc, out_idx, out_dist, slow_list, slow_count, ratio, qlist, qcount, \
        work2_n)
        // pass-2 item size (queries); the work2 list holds up to n_work << 2 items (host sizes it)
        switch (pass2_variant()) {
        // r01g A/B on config 2 (kernel ms, both passes, 2 runs): 512-query items (r01f) 7.40-7.43,
        // 256 (QT 2 x 4 waves) 7.19-7.22, 256 (QT 4 x 2 waves) 7.24-7.28, 128 (QT 1 x 4 waves) 7.16-7.21:
        // a config-2 pair leaves ~500 queries for pass 2, so smaller items fill the chip's last round
        case 1: PASS2_LAUNCH(8, 2, 4, 2, 128); break;
        case 3: PASS2_LAUNCH(8, 4, 2, 2, 128); break;
        case 4: PASS2_LAUNCH(9, 4, 4, 2, 128); break;   // r01f
        default: PASS2_LAUNCH(7, 1, 4, 2, 128);         // 0 / 2
        }
#undef PASS2_LAUNCH
        return hipGetLastError();
    }
    switch (v) {    // single pass (tuning / A-B only)
    case 1: SIFT_LAUNCH(2, 8, 2, 128, false); break;
    case 2: SIFT_LAUNCH(2, 4, 3, 64, true); break;
    case 3: SIFT_LAUNCH(2, 8, 2, 64, false); break;
    case 4: SIFT_LAUNCH(2, 4, 4, 128, false); break;
    case 5: SIFT_LAUNCH(4, 4, 2, 64, true); break;
    case 6: SIFT_LAUNCH(4, 4, 2, 128, true); break;
    case 7: SIFT_LAUNCH(4, 4, 2, 256, true); break;
    case 11: SIFT_LAUNCH(2, 8, 2, 64, true); break;    // r01 default
    case 90: SIFT_LAUNCH(2, 8, 2, 64, true, 1); break;   // timing probe (wrong results): no selection
    case 95: SIFT_LAUNCH(4, 4, 2, 64, true, 1); break;   // timing probe (wrong results): no selection
    case 20: SIFT_LAUNCH(4, 4, 2, 128, false, 0, 9); break;   // software-pipelined selection
    case 21: SIFT_LAUNCH(2, 8, 2, 128, false, 0, 9); break;
    case 22: SIFT_LAUNCH(4, 4, 2, 128, false, 0, 8); break;
    case 23: SIFT_LAUNCH(2, 4, 4, 128, false, 0, 9); break;
    case 30: SIFT_LAUNCH(4, 4, 1, 128, false); break;   // MINW = 1 (r01: failed kat_sift_nt1_nt0)
    case 31: SIFT_LAUNCH(2, 8, 1, 64, true); break;     // MINW = 1, the r01 default's tiling
    default: SIFT_LAUNCH(4, 4, 2, 128, false);   // 100: the r01d single-pass default (9.57-9.67 ms on config 2)
    }
    return hipGetLastError();
#endif   // SFMX_DIAG
}
// Pass 2 overlapped with pass 1 (product SIFT / ORB paths).  One screen launch
// leaves its last partial round of workgroups idle and pass 2 (subset + settle) waits behind it.
// Here the work list (pairs in train-image order, each pair's items contiguous) is cut into batches
// at pair boundaries; the screens of consecutive batches alternate between the caller's stream and a
// second one, so one batch's tail overlaps the next batch's workgroups, and each batch's pass 2 runs
// on a third stream behind an event on its screen, beside the later screens (its latency-bound
// staging fills MFMA idle time).  Batches touch disjoint pairs (dense rows, qlist, qcount, top2); the
// slow list is appended atomically.  Dependencies are events only: no in-kernel waits.  The caller's
// stream ends after every batch (ev_screen: after the last screen; the join before returning).
hipError_t launch_two_pass_overlap(bool sift, const MatchBatch* b, int nb, const WorkItem* work, const PairDev* pairs,
                                   const ImgDev* imgs, const int8_t* desc, const int32_t* norm, const int32_t* keyc,
                                   int32_t* qlist, int32_t* qcount, int n_pairs, const int32_t* porder, int32_t* out_idx,
                                   float* out_dist, int2* slow_list, int32_t* slow_count, double ratio, hipStream_t st,
                                   hipEvent_t ev_screen, int32_t* qmask, unsigned long long* top2,
                                   unsigned long long* slot1, const OverlapStreams& os) {
    hipError_t e;
#define OCHK(x) do { if ((e = (x)) != hipSuccess) return e; } while (0)
    OCHK(hipEventRecord(os.start, st));
    OCHK(hipStreamWaitEvent(os.sx, os.start, 0));
    OCHK(hipStreamWaitEvent(os.sp, os.start, 0));
    for (int i = 0; i < nb; ++i) {
        const MatchBatch& B = b[i];
        hipStream_t s = (i & 1) ? os.sx : st;
        if (B.nw == 0) {}   // no screen items (fp32 / empty-left pairs only): pass 2 finds qcount 0
        else if (sift)
            sift_screen16_kernel<8, 4, 2, 64, true><<<B.nw, 256, 0, s>>>(work + B.w0, pairs, imgs, desc, norm, keyc,
                                                                         out_idx, out_dist, qlist, qcount, ratio, qmask, top2);
        else
            orb_screen16_kernel<8, 4, 2, 64, true><<<B.nw, 256, 0, s>>>(work + B.w0, pairs, imgs, (const uint8_t*)desc, keyc,
                                                                        out_idx, out_dist, qlist, qcount, ratio, qmask, top2);
        OCHK(hipGetLastError());
        OCHK(hipEventRecord(os.screen[i], s));
        OCHK(hipStreamWaitEvent(os.sp, os.screen[i], 0));
        if (sift) {
            sift_subset_kernel<4><<<B.np * 16, 256, 0, os.sp>>>(pairs, imgs, desc, norm, qlist, qmask, qcount, porder + B.p0, top2, slot1);
            sift_settle_kernel<<<B.np, 256, 0, os.sp>>>(pairs, imgs, qlist, qcount, top2, out_idx, out_dist, slow_list,
                                                        slow_count, ratio, qmask, slot1, porder + B.p0);
        } else {
            orb_subset_kernel<4, 2><<<B.np * 16, 256, 0, os.sp>>>(pairs, imgs, (const uint8_t*)desc, qlist, qmask, qcount,
                                                                  porder + B.p0, top2);
            orb_settle_kernel<<<B.np, 256, 0, os.sp>>>(pairs, imgs, qlist, qcount, top2, out_idx, out_dist, ratio,
                                                       porder + B.p0);
        }
        OCHK(hipGetLastError());
    }
    OCHK(hipEventRecord(os.sx_done, os.sx));
    OCHK(hipStreamWaitEvent(st, os.sx_done, 0));
    if (ev_screen) OCHK(hipEventRecord(ev_screen, st));   // every screen done (pass-1 / pass-2 split, approximate)
    OCHK(hipEventRecord(os.sp_done, os.sp));
    OCHK(hipStreamWaitEvent(st, os.sp_done, 0));
#undef OCHK
    return hipSuccess;
}

hipError_t launch_sift_slow(const int2* slow_list, const int32_t* slow_count, const PairDev* pairs,
                            const ImgDev* imgs, const int8_t* desc8, const int32_t* norm, int32_t* out_idx,
                            float* out_dist, double ratio, hipStream_t st) {
    sift_slow_kernel<<<256, 256, 0, st>>>(slow_list, slow_count, pairs, imgs, desc8, norm, out_idx, out_dist, ratio);
    return hipGetLastError();
}
hipError_t launch_sift_f32(const WorkItem* work, int n_work, const PairDev* pairs, const ImgDev* imgs,
                           const float* f32, int32_t* out_idx, float* out_dist, double ratio, hipStream_t st) {
    if (n_work == 0) return hipSuccess;
    sift_f32_kernel<<<n_work, 512, 0, st>>>(work, nullptr, pairs, imgs, f32, out_idx, out_dist, ratio);
    return hipGetLastError();
}
hipError_t launch_orb_knn2(const WorkItem* work, int n_work, const PairDev* pairs, const ImgDev* imgs,
                           const uint8_t* desc8, int32_t* out_idx, float* out_dist, double ratio, hipStream_t st) {
    if (n_work == 0) return hipSuccess;
    orb_knn2_kernel<2><<<n_work, 256, 0, st>>>(work, pairs, imgs, desc8, out_idx, out_dist, ratio);
    return hipGetLastError();
}
// ORB kernel selection: 0 (default, the only form in the product library) = FP4 MFMA path on
// 128-byte +-1 rows; in the diagnostic build SFMX_ORB_VARIANT selects 1 = VALU xor/popcount path
// on 32-byte rows, 2.. = FP4 MFMA tiling variants (tuning only).
int orb_variant() {   // read per run, as sift_variant(): tests switch variants within one process
    const char* e = SFMX_DIAG_ENV("SFMX_ORB_VARIANT");
    return e ? atoi(e) : 0;
}
hipError_t launch_prep_hamming_fp4(const uint8_t* src, int rows, int cols, int rows_pad, uint8_t* dst, int32_t* keyc,
                                   hipStream_t st) {
    if (rows_pad == 0) return hipSuccess;
    prep_hamming_fp4_kernel<<<(rows_pad + 7) / 8, 256, 0, st>>>(src, rows, cols, rows_pad,
                                                               reinterpret_cast<uint32_t*>(dst), keyc);
    return hipGetLastError();
}
hipError_t launch_orb_mfma(const WorkItem* work, int n_work, const PairDev* pairs, const ImgDev* imgs,
                           const uint8_t* desc4, const int32_t* keyc, int32_t* qlist, int32_t* qcount, int n_pairs,
                           const int32_t* porder, WorkItem* work2, int32_t* work2_n, int32_t* out_idx, float* out_dist,
                           double ratio, hipStream_t st, hipEvent_t ev_screen, int32_t* qmask,
                           unsigned long long* top2) {
    if (n_work == 0) return hipSuccess;
    if (orb_variant() == 0 || orb_variant() >= 10) {   // two-pass ratio test (default)
        hipError_t e = hipSuccess;   // qcount and the screen's XCD tickets behind it: zeroed by the caller's one fill
        if (orb_variant() == 0 && qmask && top2) {   // subset-restricted pass 2 (default)
            static const int slots = resident_slots(orb_screen16_kernel<8, 4, 2, 64, true, true>, 256);
            if (slots > 0 && persist_screens())
                orb_screen16_kernel<8, 4, 2, 64, true, true><<<std::min(n_work, slots), 256, 0, st>>>(
                    work, pairs, imgs, desc4, keyc, out_idx, out_dist, qlist, qcount, ratio, qmask, top2,
                    qcount + n_pairs, n_work);
            else
                orb_screen16_kernel<8, 4, 2, 64, true><<<n_work, 256, 0, st>>>(work, pairs, imgs, desc4, keyc, out_idx,
                                                                              out_dist, qlist, qcount, ratio, qmask, top2);
            if (ev_screen) {
                e = hipEventRecord(ev_screen, st);
                if (e != hipSuccess) return e;
            }
            orb_subset_kernel<4, 2><<<n_pairs * 16, 256, 0, st>>>(pairs, imgs, desc4, qlist, qmask, qcount, porder, top2);
            orb_settle_kernel<<<n_pairs, 256, 0, st>>>(pairs, imgs, qlist, qcount, top2, out_idx, out_dist, ratio);
            return hipGetLastError();
        }
#ifndef SFMX_DIAG
        return hipErrorInvalidValue;   // the product path always has the subset buffers
    }
    return hipErrorInvalidValue;
#else
        orb_screen16_kernel<8, 4, 2, 64><<<n_work, 256, 0, st>>>(work, pairs, imgs, desc4, keyc, out_idx, out_dist,
                                                                  qlist, qcount, ratio);
        if (ev_screen) {
            e = hipEventRecord(ev_screen, st);
            if (e != hipSuccess) return e;
        }
#define ORB_PASS2(ISH, QT, W)                                                                                   \
    static_assert((1 << (ISH)) == (QT) * (W) * 16, "pass-2 item size must equal the queries one block covers"); \
    static_assert((ISH) >= 7 && (ISH) <= 9, "work2 holds n_work << 2 items: items of 128..512 queries");       \
    compact_work_kernel<ISH><<<1, 1024, 0, st>>>(porder, n_pairs, qcount, work2, work2_n);                      \
    orb_mfma16_kernel<QT, W, 2, 64, true><<<n_work << (9 - ISH), W * 64, 0, st>>>(work2, pairs, imgs, desc4, keyc, \
                                                                                  out_idx, out_dist, ratio, qlist, \
                                                                                  qcount, work2_n)
        switch (orb_variant()) {
        // Pass-2 builds with 2 or 4 query tiles per wave (128- / 256-query items) lost about half
        // the accepted matches in the GPU parity tests, also with 16 extra wait states after each
        // tile's MFMAs and with the key added on the VALU instead of the C operand; the 8-tile build
        // is exact on every test.  Not understood; only the 8-tile form is built.
        // r01g config 4: 18.68-18.73 ms (two-pass) vs 20.19-20.24 (single pass, variant 5).
        case 13: ORB_PASS2(7, 2, 4); break;   // 128-query items (2 tiles per wave)
        case 14: ORB_PASS2(8, 4, 4); break;   // 256-query items (4 tiles per wave)
        default: ORB_PASS2(9, 8, 4);       // 12: 512-query items (the r01 pass 2)
        }
#undef ORB_PASS2
        return hipGetLastError();
    }
#define ORB_LAUNCH(QT, W, MINW, ST) \
    orb_mfma_kernel<QT, W, MINW, ST><<<n_work, W * 64, 0, st>>>(work, pairs, imgs, desc4, keyc, out_idx, out_dist, ratio)
#define ORB16_LAUNCH(QT, W, MINW, ST) \
    orb_mfma16_kernel<QT, W, MINW, ST><<<n_work, W * 64, 0, st>>>(work, pairs, imgs, desc4, keyc, out_idx, out_dist, ratio)
    switch (orb_variant()) {      // every variant: 512 queries per work item
    // r01g A/B on config 4 (kernel ms, 2 runs): 32x32x64 4 x 4 waves (r01 default, now 8) 21.1-21.5,
    // 16x16x128 8 x 4 waves / 64-row stages 20.16-20.21, 128-row stages 20.78-20.85.  A 16x16x128
    // build with 4 tiles x 8 waves failed kat_orb_ties (one accepted match lost) and is not kept;
    // like the MINW = 1 builds the cause is not understood.
    case 6: ORB16_LAUNCH(8, 4, 2, 128); break;
    case 7: ORB16_LAUNCH(4, 8, 2, 64); break;    // 4 tiles x 8 waves (r01g: lost a kat_orb_ties match)
    case 9: ORB_LAUNCH(4, 4, 1, 64); break;      // 32x32x64 with MINW = 1
    case 8: ORB_LAUNCH(4, 4, 2, 64); break;
    case 2: ORB_LAUNCH(2, 8, 2, 64); break;
    case 3: ORB_LAUNCH(2, 8, 2, 128); break;
    case 4: ORB_LAUNCH(1, 16, 1, 128); break;
    default: ORB16_LAUNCH(8, 4, 2, 64);   // 5: single pass, 16x16x128
    }
#undef ORB_LAUNCH
#undef ORB16_LAUNCH
    return hipGetLastError();
#endif   // SFMX_DIAG
}
hipError_t launch_assemble(const PairDev* pairs, int n_pairs, const ImgDev* imgs, const int32_t* out_idx,
                           const float* out_dist, int distinct, int min_count, int max_nt, int64_t* counts,
                           int32_t* keep, int64_t* offsets, DMatchDev* out, int32_t* unsettled, hipStream_t st) {
    if (n_pairs == 0) {
        (void)hipMemsetAsync(offsets, 0, sizeof(int64_t), st);
        return hipGetLastError();
    }
    const size_t shmem = distinct ? (size_t)2 * ((max_nt + 31) / 32) * 4 : 0;
    if (shmem > 150 * 1024) return hipErrorInvalidValue;
    assemble_kernel<0><<<n_pairs, 1024, shmem, st>>>(pairs, imgs, out_idx, out_dist, distinct, min_count, counts, keep, nullptr,
                                                     nullptr, unsettled);
    scan_offsets_kernel<<<1, 1024, 0, st>>>(counts, n_pairs, offsets);
    assemble_kernel<1><<<n_pairs, 1024, shmem, st>>>(pairs, imgs, out_idx, out_dist, distinct, min_count, counts, keep, offsets,
                                                     out, unsettled);
    return hipGetLastError();
}
// The list path's settle + assembly (after the LISTS screen and subset kernels, and after the fp32
// kernel of a mixed run): finish (ev_main is recorded behind it), one scan over every pair's count,
// write.  recs: the run's pairs in any order, one workgroup each.
hipError_t launch_finish_lists(const PairRec* recs, int n_pairs, const int32_t* qlist, const int32_t* qmask,
                               const int32_t* qcount, unsigned long long* top2, const unsigned long long* slot1,
                               int2* slow_list, int32_t* slow_count, const int8_t* desc8, const int32_t* norm,
                               const int32_t* out_idx, const float* out_dist, double ratio, int distinct, int min_count,
                               int max_nq, int max_nt, int64_t* counts, int32_t* keep, int64_t* offsets, DMatchDev* out,
                               int32_t* unsettled, hipStream_t st, hipEvent_t ev_main) {
    hipError_t e;
    if (n_pairs == 0) {
        (void)hipMemsetAsync(offsets, 0, sizeof(int64_t), st);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        return ev_main ? hipEventRecord(ev_main, st) : hipSuccess;
    }
    const size_t dup = distinct ? (size_t)2 * ((max_nt + 31) / 32) * 4 : 0;
    const size_t shmem = (size_t)2 * ((max_nq + 31) / 32) * 4 + dup;
    if (shmem > 150 * 1024) return hipErrorInvalidValue;
    sift_finish_kernel<<<n_pairs, 1024, dup, st>>>(recs, qlist, qmask, qcount, top2, slot1, slow_list, slow_count, desc8, norm,
                                                   out_idx, ratio, distinct, min_count, counts, keep, unsettled);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev_main && (e = hipEventRecord(ev_main, st)) != hipSuccess) return e;
    scan_offsets_kernel<<<1, 1024, 0, st>>>(counts, n_pairs, offsets);
    assemble_lists_kernel<<<n_pairs, 1024, shmem, st>>>(recs, qlist, qcount, top2, out_idx, out_dist, distinct, counts, offsets,
                                                        out);
    return hipGetLastError();
}

}  // namespace sfmx
