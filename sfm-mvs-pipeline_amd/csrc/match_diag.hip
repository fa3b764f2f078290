// SPDX-License-Identifier: MIT
// sfmx matcher: the diagnostic library's kernels and routes (lib/libsfmx_diag.so, -DSFMX_DIAG; diag.hpp).
//
// Everything only a non-product MatchRoute reaches: the superseded kernel forms kept for A/B timing and the
// variant parity tests, their launch sequences, the overlapped two-pass launcher and the MFMA form probe.
// The file is empty in the product build, so the product library carries none of these kernels.  Kernel
// templates that the product instantiates as well are in match_device.hpp; for the product route the two
// dispatchers below call the product's own launch_sift_product / launch_orb_product (match_kernels.hip).
#ifdef SFMX_DIAG
#include "match_device.hpp"
#include "diag.hpp"

namespace sfmx {

// ORB rows (cols <= 32 bytes) -> zero-padded 32-byte rows.
__global__ void prep_hamming_kernel(const uint8_t* __restrict__ src, int rows, int cols, int rows_pad,
                                    uint8_t* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)rows_pad * ORB_BYTES;
    if (i >= total) return;
    const int r = (int)(i / ORB_BYTES), c = (int)(i % ORB_BYTES);
    dst[i] = (r < rows && c < cols) ? src[(int64_t)r * cols + c] : 0;
}

// ---------------------------------------------------------------------------
// Two-pass ratio test, pass 1 (the r01f SIFT path, MatchRoute::INT8_32): sift_screen_kernel settles
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
// PERSIST (r04, MatchRoute::persist): a grid of resident workgroup slots takes work items
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
// Launch wrappers (host side, called by matcher.cpp).
hipError_t launch_prep_hamming(const uint8_t* src, int rows, int cols, int rows_pad, uint8_t* dst, hipStream_t st) {
    const int64_t total = (int64_t)rows_pad * ORB_BYTES;
    if (total == 0) return hipSuccess;
    prep_hamming_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(src, rows, cols, rows_pad, dst);
    return hipGetLastError();
}
#define RECORD_SCREEN()                                              \
    if (ev_screen) {   /* pass-1 / pass-2 split of the launch (sfmx_matcher_pass_timing) */ \
        const hipError_t e_ = hipEventRecord(ev_screen, st);         \
        if (e_ != hipSuccess) return e_;                             \
    }

// SIFT, every route (MatchRoute; resolve_route of matcher.cpp names the switch values).  qcount, the screens' XCD
// tickets behind it and qcount2: zeroed by the caller's one fill.  On the list routes the pass-2 state lives at the
// list slots and the caller settles with launch_finish_lists; on the others the results go to the dense arrays.
// SFMX_SCREEN_PERSIST=1: the ticket-fed persistent screens.  A single global ticket measured slower in r04d (C2 6.85
// vs 6.40 ms, C4 18.96 vs 17.44 ms per launch, profiles/r04d_ab.txt): items taken in list order landed on every XCD,
// so each XCD's L2 streamed every active train image, where the one-item-per-workgroup grid's XCD-contiguous mapping
// keeps a train image on one XCD.  Hence the per-XCD ranges and tickets of xcd_ticket (r04e A/B).
hipError_t launch_sift_diag(const MatchRoute& r, const MatchBufs& b, int n_work, int n_pairs, double ratio, hipStream_t st,
                            hipEvent_t ev_screen) {
    if (r.sift_product()) return launch_sift_product(b, n_work, n_pairs, ratio, r.full_row_grid, st, ev_screen);
    if (n_work == 0) return hipSuccess;
    using R = MatchRoute;
    int32_t* qlist2 = reinterpret_cast<int32_t*>(b.slot1);
    int32_t* qcount2 = b.qcount + arena_qcount2(n_pairs);
    if (r.sift_lists) {
        switch (r.pass2) {
        case R::ROWS:          // the product sequence behind the screen's other MFMA shape (SIFT_VARIANT_FP6_OTHER_SHAPE)
        case R::SUBSET_CERT:   // the product sequence with the certified route on sift_subset_kernel (SIFT_VARIANT_FP6_SUBSET_WG)
            if (r.screen == R::FP6_32)
                sift_screen6w_kernel<4, 2, 128, true><<<n_work, 256, 0, st>>>(b.work, b.pairs, b.imgs, b.desc6, b.keyf, b.ne, b.imax,
                                                                             b.qlist, b.qcount, ratio, b.qmask, b.top2, qlist2, qcount2);
            else
                sift_screen6_kernel<8, 4, 3, 128, true><<<n_work, 256, 0, st>>>(b.work, b.pairs, b.imgs, b.desc6, b.keyf, b.ne, b.imax,
                                                                               b.qlist, b.qcount, ratio, b.qmask, b.top2, qlist2, qcount2);
            RECORD_SCREEN();
            if (r.pass2 == R::SUBSET_CERT)
                sift_subset_kernel<4, true><<<n_pairs * 16, 256, 0, st>>>(b.pairs, b.imgs, b.desc8, b.norm, b.qlist, b.qmask, b.qcount,
                                                                          b.porder, b.top2, b.slot1, qcount2, SIFT_RIDE_MAX);
            else
                sift_rows_kernel<2><<<n_pairs * 4, 256, 0, st>>>(b.pairs, b.imgs, b.desc8, b.norm, b.qlist, b.qmask, b.qcount, qcount2,
                                                                 b.porder, b.top2);
            return launch_sift_full_rows(b, n_work, n_pairs, ratio, r.full_row_grid, st);
        case R::FULL_ROWS:     // FP6 screen, exact pass 2 over every train row for every forwarded query (SIFT_VARIANT_FP6_FULL)
            sift_screen6_kernel<8, 4, 3, 128, false><<<n_work, 256, 0, st>>>(b.work, b.pairs, b.imgs, b.desc6, b.keyf, b.ne, b.imax,
                                                                            b.qlist, b.qcount, ratio, b.qmask, b.top2, nullptr, nullptr);
            RECORD_SCREEN();
            compact_work_kernel<7><<<1, 1024, 0, st>>>(b.porder, n_pairs, b.qcount, b.work2, b.work2_n);
            sift_knn2_kernel<1, 4, 2, 128, false, true, true><<<n_work << 2, 256, 0, st>>>(   // work2 holds n_work << 2 items
                b.work2, b.pairs, b.imgs, b.desc8, b.norm, b.keyc, nullptr, nullptr, nullptr, nullptr, ratio, b.qlist, b.qcount,
                b.work2_n, b.top2);
            return hipGetLastError();
        case R::SUBSET:        // the exact int8 screen with subset masks, subset pass 2 (SIFT_VARIANT_INT8_LISTS)
            sift_screen16_kernel<8, 4, 2, 64, true, false, true><<<n_work, 256, 0, st>>>(
                b.work, b.pairs, b.imgs, b.desc8, b.norm, b.keyc2, b.dense_idx, b.dense_dist, b.qlist, b.qcount, ratio, b.qmask, b.top2);
            RECORD_SCREEN();
            sift_subset_kernel<4, true><<<n_pairs * 16, 256, 0, st>>>(b.pairs, b.imgs, b.desc8, b.norm, b.qlist, b.qmask, b.qcount,
                                                                      b.porder, b.top2, b.slot1);
            return hipGetLastError();
        default: return hipErrorInvalidValue;
        }
    }
    if (r.pass2 == R::SUBSET) {   // int8 screen with subset masks, subset pass 2, settle into the dense arrays (the r02 default)
        static const int slots = resident_slots(sift_screen16_kernel<8, 4, 2, 64, true, true>, 256);
        if (slots > 0 && r.persist)
            sift_screen16_kernel<8, 4, 2, 64, true, true><<<std::min(n_work, slots), 256, 0, st>>>(
                b.work, b.pairs, b.imgs, b.desc8, b.norm, b.keyc2, b.dense_idx, b.dense_dist, b.qlist, b.qcount, ratio, b.qmask,
                b.top2, b.qcount + n_pairs, n_work);
        else
            sift_screen16_kernel<8, 4, 2, 64, true><<<n_work, 256, 0, st>>>(b.work, b.pairs, b.imgs, b.desc8, b.norm, b.keyc2,
                                                                           b.dense_idx, b.dense_dist, b.qlist, b.qcount, ratio,
                                                                           b.qmask, b.top2);
        RECORD_SCREEN();
        sift_subset_kernel<4><<<n_pairs * 16, 256, 0, st>>>(b.pairs, b.imgs, b.desc8, b.norm, b.qlist, b.qmask, b.qcount, b.porder,
                                                            b.top2, b.slot1);
        sift_settle_kernel<<<n_pairs, 256, 0, st>>>(b.pairs, b.imgs, b.qlist, b.qcount, b.top2, b.dense_idx, b.dense_dist,
                                                    b.slow_list, b.slow_count, ratio, b.qmask, b.slot1);
        return hipGetLastError();
    }
    if (r.pass2 == R::GATHER) {   // screen, then the exact kernel on the compacted list of forwarded queries
#define SCREEN_ARGS b.work, b.pairs, b.imgs, b.desc8, b.norm, b.keyc2, b.dense_idx, b.dense_dist, b.qlist, b.qcount, ratio
        switch (r.screen) {
        case R::INT8_32: sift_screen_kernel<4, 4, 2, 64><<<n_work, 256, 0, st>>>(SCREEN_ARGS); break;
        case R::INT8_16: sift_screen16_kernel<8, 4, 2, 64><<<n_work, 256, 0, st>>>(SCREEN_ARGS); break;
        case R::INT8_16_S128: sift_screen16_kernel<8, 4, 2, 128><<<n_work, 256, 0, st>>>(SCREEN_ARGS); break;
        case R::INT8_16_W8: sift_screen16_kernel<4, 8, 2, 64><<<n_work, 512, 0, st>>>(SCREEN_ARGS); break;
        default: return hipErrorInvalidValue;
        }
#undef SCREEN_ARGS
        RECORD_SCREEN();
#define PASS2_LAUNCH(ISH, QT, W)                                                                                 \
    static_assert((1 << (ISH)) == (QT) * (W) * 32, "pass-2 item size must equal the queries one block covers");  \
    static_assert((ISH) >= 7 && (ISH) <= 9, "work2 holds n_work << 2 items: items of 128..512 queries");         \
    compact_work_kernel<ISH><<<1, 1024, 0, st>>>(b.porder, n_pairs, b.qcount, b.work2, b.work2_n);               \
    sift_knn2_kernel<QT, W, 2, 128, false, true><<<n_work << (9 - ISH), W * 64, 0, st>>>(                         \
        b.work2, b.pairs, b.imgs, b.desc8, b.norm, b.keyc, b.dense_idx, b.dense_dist, b.slow_list, b.slow_count, ratio, \
        b.qlist, b.qcount, b.work2_n)
        switch (r.p2_qt * r.p2_waves) {   // the work2 list holds up to n_work << 2 items (the host sizes it)
        case 4: PASS2_LAUNCH(7, 1, 4); break;    // SFMX_SIFT_P2 = 0
        case 8:
            if (r.p2_waves == 4) { PASS2_LAUNCH(8, 2, 4); }   // 1
            else { PASS2_LAUNCH(8, 4, 2); }                   // 3
            break;
        case 16: PASS2_LAUNCH(9, 4, 4); break;   // 4 (r01f)
        default: return hipErrorInvalidValue;
        }
#undef PASS2_LAUNCH
        return hipGetLastError();
    }
#define SIFT_LAUNCH(QT, W, MINW, ST, MF)                                                                       \
    sift_knn2_kernel<QT, W, MINW, ST, MF><<<n_work, W * 64, 0, st>>>(b.work, b.pairs, b.imgs, b.desc8, b.norm, b.keyc, \
                                                                     b.dense_idx, b.dense_dist, b.slow_list, b.slow_count, ratio)
    switch (r.pass2) {    // single pass (tuning / A-B only)
    case R::SINGLE: SIFT_LAUNCH(4, 4, 2, 128, false); break;         // the r01d default (9.57-9.67 ms on config 2)
    case R::SINGLE_MINW1: SIFT_LAUNCH(4, 4, 1, 128, false); break;   // MINW = 1 (r01: failed kat_sift_nt1_nt0)
    case R::SINGLE_R01: SIFT_LAUNCH(2, 8, 1, 64, true); break;       // MINW = 1, the r01 default's tiling
    default: return hipErrorInvalidValue;
    }
#undef SIFT_LAUNCH
    return hipGetLastError();
}

// Pass 2 overlapped with pass 1 (the int8 SIFT screen / the ORB product kernels).  One screen
// launch leaves its last partial round of workgroups idle and pass 2 (subset + settle) waits behind it.
// Here the work list (pairs in train-image order, each pair's items contiguous) is cut into batches
// at pair boundaries; the screens of consecutive batches alternate between the caller's stream and a
// second one, so one batch's tail overlaps the next batch's workgroups, and each batch's pass 2 runs
// on a third stream behind an event on its screen, beside the later screens (its latency-bound
// staging fills MFMA idle time).  Batches touch disjoint pairs (dense rows, qlist, qcount, top2); the
// slow list is appended atomically.  Dependencies are events only: no in-kernel waits.  The caller's
// stream ends after every batch (ev_screen: after the last screen; the join before returning).
hipError_t launch_two_pass_overlap(bool sift, const MatchBatch* batches, int nb, const MatchBufs& b, int n_pairs, double ratio,
                                   hipStream_t st, hipEvent_t ev_screen, const OverlapStreams& os) {
    hipError_t e;
    const uint8_t* desc4 = reinterpret_cast<const uint8_t*>(b.desc8);
#define OCHK(x) do { if ((e = (x)) != hipSuccess) return e; } while (0)
    OCHK(hipEventRecord(os.start, st));
    OCHK(hipStreamWaitEvent(os.sx, os.start, 0));
    OCHK(hipStreamWaitEvent(os.sp, os.start, 0));
    for (int i = 0; i < nb; ++i) {
        const MatchBatch& B = batches[i];
        hipStream_t s = (i & 1) ? os.sx : st;
        if (B.nw == 0) {}   // no screen items (fp32 / empty-left pairs only): pass 2 finds qcount 0
        else if (sift)
            sift_screen16_kernel<8, 4, 2, 64, true><<<B.nw, 256, 0, s>>>(b.work + B.w0, b.pairs, b.imgs, b.desc8, b.norm, b.keyc2,
                                                                         b.dense_idx, b.dense_dist, b.qlist, b.qcount, ratio,
                                                                         b.qmask, b.top2);
        else
            orb_screen16_kernel<8, 4, 2, 64, true><<<B.nw, 256, 0, s>>>(b.work + B.w0, b.pairs, b.imgs, desc4, b.keyc, b.dense_idx,
                                                                        b.dense_dist, b.qlist, b.qcount, ratio, b.qmask, b.top2);
        OCHK(hipGetLastError());
        OCHK(hipEventRecord(os.screen[i], s));
        OCHK(hipStreamWaitEvent(os.sp, os.screen[i], 0));
        if (sift) {
            sift_subset_kernel<4><<<B.np * 16, 256, 0, os.sp>>>(b.pairs, b.imgs, b.desc8, b.norm, b.qlist, b.qmask, b.qcount,
                                                                b.porder + B.p0, b.top2, b.slot1);
            sift_settle_kernel<<<B.np, 256, 0, os.sp>>>(b.pairs, b.imgs, b.qlist, b.qcount, b.top2, b.dense_idx, b.dense_dist,
                                                        b.slow_list, b.slow_count, ratio, b.qmask, b.slot1, b.porder + B.p0);
        } else {
            OCHK(launch_orb_pass2(b, b.porder + B.p0, B.np, b.porder + B.p0, ratio, os.sp));
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

hipError_t launch_sift_slow(const MatchBufs& b, double ratio, hipStream_t st) {
    sift_slow_kernel<<<256, 256, 0, st>>>(b.slow_list, b.slow_count, b.pairs, b.imgs, b.desc8, b.norm, b.dense_idx, b.dense_dist,
                                          ratio);
    return hipGetLastError();
}

// ORB, every route: the FP4 MFMA forms on 128-byte +-1 rows, and ORB_VALU (xor / popcount on 32-byte rows; the
// row layout is fixed by set_images).
hipError_t launch_orb_diag(const MatchRoute& r, const MatchBufs& b, int n_work, int n_pairs, double ratio, hipStream_t st,
                           hipEvent_t ev_screen) {
    if (r.orb_product()) return launch_orb_product(b, n_work, n_pairs, ratio, st, ev_screen);
    if (n_work == 0) return hipSuccess;
    using R = MatchRoute;
    const uint8_t* desc = reinterpret_cast<const uint8_t*>(b.desc8);
    if (r.orb == R::ORB_VALU) {
        orb_knn2_kernel<2><<<n_work, 256, 0, st>>>(b.work, b.pairs, b.imgs, desc, b.dense_idx, b.dense_dist, ratio);
        return hipGetLastError();
    }
    if (r.orb == R::ORB_SUBSET) {   // the product kernels; the screen persistent (SFMX_SCREEN_PERSIST=1) where the occupancy is known
        static const int slots = resident_slots(orb_screen16_kernel<8, 4, 2, 64, true, true>, 256);
        if (slots > 0 && r.persist)
            orb_screen16_kernel<8, 4, 2, 64, true, true><<<std::min(n_work, slots), 256, 0, st>>>(
                b.work, b.pairs, b.imgs, desc, b.keyc, b.dense_idx, b.dense_dist, b.qlist, b.qcount, ratio, b.qmask, b.top2,
                b.qcount + n_pairs, n_work);
        else
            orb_screen16_kernel<8, 4, 2, 64, true><<<n_work, 256, 0, st>>>(b.work, b.pairs, b.imgs, desc, b.keyc, b.dense_idx,
                                                                          b.dense_dist, b.qlist, b.qcount, ratio, b.qmask, b.top2);
        RECORD_SCREEN();
        return launch_orb_pass2(b, b.porder, n_pairs, nullptr, ratio, st);
    }
#define ORB_PASS2(ISH, QT, W)                                                                                   \
    static_assert((1 << (ISH)) == (QT) * (W) * 16, "pass-2 item size must equal the queries one block covers"); \
    static_assert((ISH) >= 7 && (ISH) <= 9, "work2 holds n_work << 2 items: items of 128..512 queries");       \
    orb_screen16_kernel<8, 4, 2, 64><<<n_work, 256, 0, st>>>(b.work, b.pairs, b.imgs, desc, b.keyc, b.dense_idx, b.dense_dist, \
                                                              b.qlist, b.qcount, ratio);                        \
    RECORD_SCREEN();                                                                                            \
    compact_work_kernel<ISH><<<1, 1024, 0, st>>>(b.porder, n_pairs, b.qcount, b.work2, b.work2_n);              \
    orb_mfma16_kernel<QT, W, 2, 64, true><<<n_work << (9 - ISH), W * 64, 0, st>>>(b.work2, b.pairs, b.imgs, desc, b.keyc, \
                                                                                  b.dense_idx, b.dense_dist, ratio, b.qlist, \
                                                                                  b.qcount, b.work2_n)
#define ORB_LAUNCH(QT, W, MINW, ST) \
    orb_mfma_kernel<QT, W, MINW, ST><<<n_work, W * 64, 0, st>>>(b.work, b.pairs, b.imgs, desc, b.keyc, b.dense_idx, b.dense_dist, ratio)
#define ORB16_LAUNCH(QT, W, MINW, ST) \
    orb_mfma16_kernel<QT, W, MINW, ST><<<n_work, W * 64, 0, st>>>(b.work, b.pairs, b.imgs, desc, b.keyc, b.dense_idx, b.dense_dist, ratio)
    switch (r.orb) {      // every form: 512 queries per work item
    // Two-pass with the full-row pass 2.  Pass-2 builds with 2 or 4 query tiles per wave (128- / 256-query items)
    // lost about half the accepted matches in the GPU parity tests, also with 16 extra wait states after each
    // tile's MFMAs and with the key added on the VALU instead of the C operand; the 8-tile build was exact on
    // every test.  Both causes are found and fixed (the item size, and the select behind lowe_select).
    // r01g config 4: 18.68-18.73 ms (two-pass) vs 20.19-20.24 (single pass, ORB_SINGLE_16).
    case R::ORB_GATHER_128: ORB_PASS2(7, 2, 4); break;   // 2 tiles per wave
    case R::ORB_GATHER_256: ORB_PASS2(8, 4, 4); break;   // 4 tiles per wave
    case R::ORB_GATHER_512: ORB_PASS2(9, 8, 4); break;   // the r01 pass 2
    // Single pass.  r01g A/B on config 4 (kernel ms, 2 runs): 32x32x64 4 x 4 waves 21.1-21.5, 16x16x128 8 x 4 waves /
    // 64-row stages 20.16-20.21 (the other tilings' numbers: DESIGN.md 5).
    case R::ORB_SINGLE_16_W8: ORB16_LAUNCH(4, 8, 2, 64); break;    // 4 tiles x 8 waves (r01g: lost a kat_orb_ties match)
    case R::ORB_SINGLE_32_MINW1: ORB_LAUNCH(4, 4, 1, 64); break;   // 32x32x64 with MINW = 1
    case R::ORB_SINGLE_32_W16: ORB_LAUNCH(1, 16, 1, 128); break;
    case R::ORB_SINGLE_16: ORB16_LAUNCH(8, 4, 2, 64); break;       // 16x16x128
    default: return hipErrorInvalidValue;
    }
#undef ORB_PASS2
#undef ORB_LAUNCH
#undef ORB16_LAUNCH
    return hipGetLastError();
}
#undef RECORD_SCREEN

}  // namespace sfmx
#endif   // SFMX_DIAG
