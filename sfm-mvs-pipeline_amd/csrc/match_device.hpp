// SPDX-License-Identifier: MIT
// sfmx matcher device code that both translation units instantiate: the product kernels of
// match_kernels.hip and the diagnostic routes of match_diag.hip (which replace one kernel of a product
// sequence, or run the product sequence on other streams).  Kernel templates and device helpers, and the
// occupancy query their launchers share.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <climits>
#include <cstdlib>
#include "match_common.hpp"
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
template <int QT, int WAVES, int MINW, int STAGE, bool MFMA_FIRST, bool GATHER, bool LISTS, bool VIA>
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
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) select(acc[qt], kv, c1[qt], c2[qt]);
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

template <int QT, int WAVES, int MINW, int STAGE, bool MFMA_FIRST, bool GATHER = false, bool LISTS = false, bool VIA = false>
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
    sift_knn2_item<QT, WAVES, MINW, STAGE, MFMA_FIRST, GATHER, LISTS, VIA>(                                            \
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

// The read-ahead of sift_screen6_kernel's row loop.  A 32-row block of a stage in registers: per 16-row block the
// lane's plane-A piece (16 B: lo), its plane-B piece (8 B: hi) and the four keys of its accumulator rows (k).
// Two such sets take turns, each in registers of its own named here: lo and hi of a 16-row block are adjacent (the
// MFMA takes them as one 192-bit operand), and a set that the allocator places itself costs copies at the stage
// seam, where the first block of the next stage is requested while the other set is still to be multiplied.
typedef int i32x2 __attribute__((ext_vector_type(2)));
#define SCREEN6_REGS_0(C) C "{v[120:123]}"(lo0), C "{v[124:125]}"(hi0), C "{v[132:135]}"(k0), C "{v[126:129]}"(lo1), C "{v[130:131]}"(hi1), C "{v[136:139]}"(k1)
#define SCREEN6_REGS_1(C) C "{v[140:143]}"(lo0), C "{v[144:145]}"(hi0), C "{v[152:155]}"(k0), C "{v[146:149]}"(lo1), C "{v[150:151]}"(hi1), C "{v[156:159]}"(k1)
// Requests block T of the stage at the lane's bases (plane A, plane B, keys; LDS byte addresses) into set SET: six
// reads the compiler does not count and does not drain the LDS-DMA in front of.  The registers hold the block
// only after screen6_arrived.
template <int SET, int T>
__device__ __forceinline__ void screen6_request(i32x4& lo0, i32x2& hi0, f32x4& k0, i32x4& lo1, i32x2& hi1, f32x4& k1,
                                                unsigned pa, unsigned pb, unsigned pk) {
#define SCREEN6_REQUEST(REGS)                                                                                           \
    asm volatile("ds_read_b128 %0, %6 offset:%9\n\t"                                                                    \
                 "ds_read_b64 %1, %7 offset:%10\n\t"                                                                    \
                 "ds_read_b128 %2, %8 offset:%11\n\t"                                                                   \
                 "ds_read_b128 %3, %6 offset:%12\n\t"                                                                   \
                 "ds_read_b64 %4, %7 offset:%13\n\t"                                                                    \
                 "ds_read_b128 %5, %8 offset:%14"                                                                        \
                 : REGS("=")                                                                                            \
                 : "v"(pa), "v"(pb), "v"(pk), "n"(2 * T * 1024), "n"(2 * T * 512), "n"(2 * T * 64),                      \
                   "n"((2 * T + 1) * 1024), "n"((2 * T + 1) * 512), "n"((2 * T + 1) * 64)                                \
                 : "memory")
    if constexpr (SET == 0) SCREEN6_REQUEST(SCREEN6_REGS_0);
    else SCREEN6_REQUEST(SCREEN6_REGS_1);
#undef SCREEN6_REQUEST
}
// Waits until at most N LDS reads are in flight (they return in order) and hands set SET to the compiler: nothing
// that reads it is scheduled above the wait.
template <int SET, int N>
__device__ __forceinline__ void screen6_arrived(i32x4& lo0, i32x2& hi0, f32x4& k0, i32x4& lo1, i32x2& hi1, f32x4& k1) {
    if constexpr (SET == 0) asm volatile("s_waitcnt lgkmcnt(%6)" : SCREEN6_REGS_0("+") : "n"(N));
    else asm volatile("s_waitcnt lgkmcnt(%6)" : SCREEN6_REGS_1("+") : "n"(N));
}
// A block's MFMAs and folds over the wave's QT query tiles: e2m3 for both operands, the unit-scale product
// (fp6::mfma16), the keys as C, v_max3_f32 into the four chains of a tile.  A fence on both sides keeps them
// between the request in front and the wait behind; inside, a tile's four folds follow the next tile's two MFMAs,
// so two result pairs are live at a time.  (In the compiler's own order four pairs are, and the second register
// set does not fit beside them at three waves per SIMD.)
template <int QT>
__device__ __forceinline__ void screen6_mul(const i32x8 (&bq)[QT], float (&ch)[QT][4], i32x4 lo0, i32x2 hi0, f32x4 k0,
                                            i32x4 lo1, i32x2 hi1, f32x4 k1) {
    __builtin_amdgcn_sched_barrier(0);
    const i32x8 a0 = i32x8{lo0.x, lo0.y, lo0.z, lo0.w, hi0.x, hi0.y, 0, 0};
    const i32x8 a1 = i32x8{lo1.x, lo1.y, lo1.z, lo1.w, hi1.x, hi1.y, 0, 0};
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const f32x4 acc0 = fp6::mfma16<fp6::FMT_E2M3, false>(a0, bq[qt], k0);
        const f32x4 acc1 = fp6::mfma16<fp6::FMT_E2M3, false>(a1, bq[qt], k1);
#pragma unroll
        for (int i = 0; i < 4; ++i) ch[qt][i] = fmaxf(fmaxf(ch[qt][i], acc0[i]), acc1[i]);
    }
    __builtin_amdgcn_sched_group_barrier(0x8, 2, 0);
#pragma unroll
    for (int qt = 1; qt < QT; ++qt) {
        __builtin_amdgcn_sched_group_barrier(0x8, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x2, 4, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x2, 4, 0);
    __builtin_amdgcn_sched_barrier(0);
}

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
    const unsigned lds0 = (unsigned)(size_t)(LDS_AS const void*)lds;
    const unsigned ra = lds0 + l16 * 64 + 16 * (g ^ fp6::swz_a(l16));
    const unsigned rb = lds0 + A_BYTES + l16 * 32 + 16 * ((g >> 1) ^ fp6::swz_b(l16)) + 8 * (g & 1);
    const unsigned rk = lds0 + A_BYTES + B_BYTES + 16 * g;
    static_assert(fp6::swz_a(16) == fp6::swz_a(0) && fp6::swz_b(16) == fp6::swz_b(0), "swizzle period of 16 rows");
    static_assert(STAGE == 128, "the row loop is written out for four 32-row blocks per stage");

    // The row loop runs one 32-row block ahead: block n + 1's six reads are requested into the other register
    // set before block n's sixteen MFMAs, and the wait in front of a block's MFMAs is counted (LDS reads return
    // in order, so lgkmcnt(6) with the next block's six in flight means this block's have landed).
#define SCREEN6_SET0 lo00, hi00, k00, lo01, hi01, k01
#define SCREEN6_SET1 lo10, hi10, k10, lo11, hi11, k11

    if (nstages > 0) stager.issue(lds, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    i32x4 lo00, lo01, lo10, lo11;
    i32x2 hi00, hi01, hi10, hi11;
    f32x4 k00, k01, k10, k11;
    unsigned pa = ra, pb = rb, pk = rk;
    screen6_request<0, 0>(SCREEN6_SET0, pa, pb, pk);
    for (int s = 0; s < nstages; ++s) {
        // every wave has read stage s - 1 (the barrier below), so stage s + 1 may land in its buffer; the branch
        // stands at the top so that the body below is one basic block
        if (s + 1 < nstages) stager.issue(lds, s + 1, (s + 1) & 1);
        screen6_request<1, 1>(SCREEN6_SET1, pa, pb, pk);
        screen6_arrived<0, 6>(SCREEN6_SET0);
        screen6_mul<QT>(bq, ch, SCREEN6_SET0);
        screen6_request<0, 2>(SCREEN6_SET0, pa, pb, pk);
        screen6_arrived<1, 6>(SCREEN6_SET1);
        screen6_mul<QT>(bq, ch, SCREEN6_SET1);
        screen6_request<1, 3>(SCREEN6_SET1, pa, pb, pk);
        screen6_arrived<0, 6>(SCREEN6_SET0);
        screen6_mul<QT>(bq, ch, SCREEN6_SET0);
        // Stage end: the last block's operands are in registers before the barrier, the next stage's first block
        // is requested from the other buffer straight after it, and the last block's MFMAs run under that read.
        screen6_arrived<1, 0>(SCREEN6_SET1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // the buffer select is wave-uniform: one add per base and stage
        const int nb = s & 1 ? -BUF_BYTES : BUF_BYTES;
        pa += nb; pb += nb; pk += nb;
        screen6_request<0, 0>(SCREEN6_SET0, pa, pb, pk);   // (behind the last stage: the other buffer's old rows, never multiplied)
        screen6_mul<QT>(bq, ch, SCREEN6_SET1);
    }
    screen6_arrived<0, 0>(SCREEN6_SET0);   // no read in flight into registers the epilogue reuses
#undef SCREEN6_SET0
#undef SCREEN6_SET1

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
//
// Work list of the full-row launch behind this kernel (work2 not null): workgroup 0 builds it from qcount2 before
// its own item (compact_work_block, the body of compact_work_kernel), whatever that item turns out to be.  The
// screen has finished, so the counts are final, and the list's only reader is the next kernel on the stream.
template <int ISH, int THREADS>
__device__ __forceinline__ void compact_work_block(const int32_t* __restrict__ porder, int n_pairs,
                                                   const int32_t* __restrict__ qcount, WorkItem* __restrict__ work2,
                                                   int32_t* __restrict__ work2_n, int ride, int* wsum);
template <int QTMAX>
__global__ __launch_bounds__(256, 4)
void sift_rows_kernel(const PairDev* __restrict__ pairs, const ImgDev* __restrict__ imgs,
                      const int8_t* __restrict__ desc8, const int32_t* __restrict__ norm,
                      const int32_t* __restrict__ qlist, const int32_t* __restrict__ qmask,
                      const int32_t* __restrict__ qcount, const int32_t* __restrict__ qcount2,
                      const int32_t* __restrict__ porder, unsigned long long* __restrict__ top2,
                      WorkItem* __restrict__ work2 = nullptr, int32_t* __restrict__ work2_n = nullptr, int n_pairs = 0) {
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
    if (work2 && blockIdx.x == 0)             // (pool: free until the first window; the function ends with a barrier)
        compact_work_block<7, 256>(porder, n_pairs, qcount2, work2, work2_n, SIFT_RIDE_MAX, pool);
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

// Pass-2 work list: ceil(qcount[p] / 512) items per pair, pairs in the host's
// order (sorted by train image, so XCD-contiguous items share train rows).
// One workgroup of THREADS threads; each thread owns a contiguous run of pairs.
// A pair with at most `ride` queries gets no item (its queries ride the subset kernel; 0: every pair with a query).
// wsum: THREADS / 64 words of the caller's LDS, free again on return.
template <int ISH, int THREADS>   // queries per pass-2 item = 1 << ISH
__device__ __forceinline__ void compact_work_block(const int32_t* __restrict__ porder, int n_pairs,
                                                   const int32_t* __restrict__ qcount, WorkItem* __restrict__ work2,
                                                   int32_t* __restrict__ work2_n, int ride, int* wsum) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int per = (n_pairs + THREADS - 1) / THREADS, p0 = min(tid * per, n_pairs), p1 = min(p0 + per, n_pairs);
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
    if (tid == THREADS - 1) *work2_n = base + incl;
    __syncthreads();
}
template <int ISH>
__global__ __launch_bounds__(1024)
void compact_work_kernel(const int32_t* __restrict__ porder, int n_pairs, const int32_t* __restrict__ qcount,
                         WorkItem* __restrict__ work2, int32_t* __restrict__ work2_n, int ride = 0) {
    __shared__ int wsum[16];
    compact_work_block<ISH, 1024>(porder, n_pairs, qcount, work2, work2_n, ride, wsum);
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

// Resident workgroups of a kernel on the current device (host side: the grids of the full-row launch and of the
// persistent screens); 0 = unknown.
template <class F>
int resident_slots(F kernel, int threads) {
    int dev = 0, nb = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, threads, 0) != hipSuccess) return 0;
    return nb * prop.multiProcessorCount;
}

}  // namespace sfmx
