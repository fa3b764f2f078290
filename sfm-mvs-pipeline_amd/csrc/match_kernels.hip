// SPDX-License-Identifier: MIT
// sfmx matcher kernels for gfx950 (MI355X / CDNA4): the product library's kernels and launchers.
// Kernel templates the diagnostic library instantiates as well are in match_device.hpp; what only a
// diagnostic route (MatchRoute, match_common.hpp) launches is in match_diag.hip.
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
//     2nd-best s reaches it takes the exact float-sqrt ranking on 64-bit keys
//     (slow_top2: in sift_finish_kernel on the list path, sift_slow_kernel on the
//     diagnostic library's dense routes).  Real SIFT distances never get there.
//   * train rows stream through a double-buffered LDS stage (64 rows, 8 KiB)
//     filled by global_load_lds_dwordx4 with an XOR-swizzled source address
//     (conflict-free ds_read_b128 fragment reads).
//   * one work item = 512 queries of one pair (8 waves x 2 query tiles x 32);
//     work items are sorted by train image and mapped XCD-contiguously so the
//     blocks streaming one train image share an XCD's L2.
#include "match_device.hpp"

namespace sfmx {

// ---------------------------------------------------------------------------
// Last arrivers: a workgroup hands a few words to whichever workgroup of the grid finishes last.
// A device-scope release fence in front of the ticket writes the XCD's whole L2 back, once per workgroup
// (prep_l2_batch_kernel 140 -> 460-490 us, sift_finish_kernel 17 -> 46 us with it, profiles/folds_ab_step.txt).
// So the handed-over words, and only they, move as device-scope atomics, which are performed at the point that is
// coherent for every XCD: the writer's returning atomics have been performed when their values are back
// (handed_over waits for them), its ticket is issued after that, and the last arriver issues its device-scope
// atomic loads after its own ticket has returned.  Nothing else a workgroup wrote is read before the kernel ends.
__device__ __forceinline__ void hand_over(unsigned long long* p, unsigned long long v) {
    const unsigned long long old = atomicExch(p, v);
    asm volatile("" ::"v"(old));   // the returning form: complete when the value is back
}
__device__ __forceinline__ void handed_over() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

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
// All images of a set_images call in one launch: blockIdx.y = image (table in HBM).
constexpr int PREP_ROWS = 64;   // rows per workgroup of the batched prep
static_assert(ROW_ALIGN % PREP_ROWS == 0 && PREP_ROWS % 8 == 0, "whole 8-row steps, no partial workgroup");
//
// The kernel finishes its own job (no fill in front, no publishing kernel behind): last arrivers, DESIGN 5.
// One thread of a workgroup hands its (emax, amax) over in its own slot of `part` and its integrality finding in
// the image's flag (hand_over above), and then takes the image's ticket.  Whoever draws the image's last ticket
// reduces the image's slots into imax[2 i], imax[2 i + 1] (plain stores: no zeroed word, no atomicMax), puts the
// ticket back to 0 and takes the global ticket; whoever draws the last of those copies the n flags to the host
// words, release-stores the sequence word at system scope and leaves flags and the ticket at 0 for the next call.
// Nothing waits.  Image i's ticket counts max(rows_pad / PREP_ROWS, 1) workgroups, computed here from rows_pad:
// a workgroup past its image's rows_pad leaves at once and takes no ticket, except workgroup 0 of an image
// without rows, which carries that image's zeros.  What a last arriver reads of other workgroups (slots, flags)
// it reads with device-scope atomics issued behind its own ticket, never through its L2's cached lines.
__global__ void prep_l2_batch_kernel(const PrepImg* __restrict__ tab, int8_t* __restrict__ desc8,
                                     int32_t* __restrict__ norm, int32_t* __restrict__ keyc,
                                     int32_t* __restrict__ keyc2, int32_t* __restrict__ flags, Fp6Rows f6,
                                     int32_t* __restrict__ imax, int32_t* __restrict__ scratch, int n_flags,
                                     FlagHandoff pub) {
    const PrepImg t = tab[blockIdx.y];
    if (blockIdx.x != 0 && (int)blockIdx.x * PREP_ROWS >= t.rows_pad) return;
    __shared__ int wmax[2][PREP_ROWS / 8];
    __shared__ int s_bad, s_last;
    const int tid = threadIdx.x;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    const Fp6Rows f6i{f6.desc6 + t.row0 * fp6::ROW_WORDS, f6.keyf + t.row0, f6.ne + t.row0};
    int emax = 0, amax = 0;   // the image's largest |e|^2 and |a|^2 over this workgroup's rows
    // PREP_ROWS rows per workgroup, 8 at a time (rows_pad is a multiple of PREP_ROWS)
    for (int r = blockIdx.x * PREP_ROWS + (tid >> 5); r < min((int)(blockIdx.x + 1) * PREP_ROWS, t.rows_pad);
         r += blockDim.x >> 5) {
        const int2 em = prep_l2_row(t.src, r, t.rows, t.cols, desc8 + t.row0 * SIFT_DIM, norm + t.row0, keyc + t.row0,
                                    keyc2 + t.row0, &s_bad, &f6i);
        emax = max(emax, em.x);
        amax = max(amax, em.y);
    }
    for (int o = 32; o > 0; o >>= 1) {
        emax = max(emax, __shfl_xor(emax, o));
        amax = max(amax, __shfl_xor(amax, o));
    }
    if ((tid & 63) == 0) { wmax[0][tid >> 6] = emax; wmax[1][tid >> 6] = amax; }
    __syncthreads();
    const int need = max(t.rows_pad / PREP_ROWS, 1);
    unsigned long long* part = reinterpret_cast<unsigned long long*>(scratch + SCRATCH_IMG + n_flags) +
                               (int64_t)blockIdx.y * gridDim.x;
    if (tid == 0) {
        int e = 0, a = 0;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) { e = max(e, wmax[0][i]); a = max(a, wmax[1][i]); }
        hand_over(part + blockIdx.x, (unsigned long long)(unsigned)e | ((unsigned long long)(unsigned)a << 32));
        if (s_bad) {
            const int old = atomicOr(flags + blockIdx.y, 1);
            asm volatile("" ::"v"(old));
        }
        handed_over();
        s_last = atomicAdd(scratch + SCRATCH_IMG + blockIdx.y, 1) == need - 1;
    }
    __syncthreads();
    if (!s_last) return;
    // the image's last workgroup: every slot of the image has been performed
    emax = amax = 0;
    for (int i = tid; i < need; i += blockDim.x) {
        const unsigned long long p = __hip_atomic_load(part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        emax = max(emax, (int)(unsigned)p);
        amax = max(amax, (int)(unsigned)(p >> 32));
    }
    for (int o = 32; o > 0; o >>= 1) {
        emax = max(emax, __shfl_xor(emax, o));
        amax = max(amax, __shfl_xor(amax, o));
    }
    if ((tid & 63) == 0) { wmax[0][tid >> 6] = emax; wmax[1][tid >> 6] = amax; }
    __syncthreads();
    if (tid == 0) {
        int e = 0, a = 0;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) { e = max(e, wmax[0][i]); a = max(a, wmax[1][i]); }
        imax[2 * blockIdx.y] = e;
        imax[2 * blockIdx.y + 1] = a;
        __hip_atomic_store(scratch + SCRATCH_IMG + blockIdx.y, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // (the image's flag was performed before any of its tickets; imax and the ticket's reset wait for no reader here)
        s_last = atomicAdd(scratch + SCRATCH_PREP, 1) == (int)gridDim.y - 1;
    }
    __syncthreads();
    if (!s_last) return;
    // the last image's last workgroup: every flag is final
    for (int i = tid; i < (int)gridDim.y; i += blockDim.x) pub.dst[i] = atomicExch(flags + i, 0);
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        __hip_atomic_store(scratch + SCRATCH_PREP, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(pub.seq, pub.value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
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

// imax[2 i], imax[2 i + 1]: image i's largest |e|^2 and |a|^2.  flags[n] and the tickets of `scratch` (n_flags image
// tickets; scratch_words(n_flags, n, prep_l2_grid_x(max_rows_pad)) words) are zero before the launch and after it.
// The per-image integrality flags go to pinned, host-coherent memory, then a sequence word with system-scope
// release: set_images spins on the word instead of a D2H copy + hipStreamSynchronize (whose interrupt-driven
// wake-up the host would pay once per matching call).  A set of empty images still runs one workgroup per image.
int prep_l2_grid_x(int max_rows_pad) { return std::max((max_rows_pad + PREP_ROWS - 1) / PREP_ROWS, 1); }
hipError_t launch_prep_l2_batch(const PrepImg* tab, int n, int max_rows_pad, int8_t* desc8, int32_t* norm,
                                int32_t* keyc, int32_t* keyc2, int32_t* flags, uint32_t* desc6, float* keyf,
                                int2* ne, int32_t* imax, int32_t* scratch, int n_flags, const FlagHandoff& pub,
                                hipStream_t st) {
    if (n == 0) return hipSuccess;
    prep_l2_batch_kernel<<<dim3((unsigned)prep_l2_grid_x(max_rows_pad), (unsigned)n), 256, 0, st>>>(
        tab, desc8, norm, keyc, keyc2, flags, Fp6Rows{desc6, keyf, ne}, imax, scratch, n_flags, pub);
    return hipGetLastError();
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
        hand_over(reinterpret_cast<unsigned long long*>(counts + p), (unsigned long long)run);   // (read by sift_finish_kernel's last workgroup)
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
// finish_pair: the workgroup's pair (every path stores counts[pair] from thread 0; the returns are uniform).
__device__ __forceinline__ void finish_pair(unsigned* bits, int* sh, int& s_slow, const PairRec* __restrict__ recs,
                                            const int32_t* __restrict__ qlist,
                                            const int32_t* __restrict__ qmask, const int32_t* __restrict__ qcount,
                                            unsigned long long* __restrict__ top2, const unsigned long long* __restrict__ slot1,
                                            int2* __restrict__ slow_list, int32_t* __restrict__ slow_count,
                                            const int8_t* __restrict__ desc8, const int32_t* __restrict__ norm,
                                            const int32_t* __restrict__ out_idx, double ratio, int distinct, int min_count,
                                            int64_t* __restrict__ counts, int32_t* __restrict__ keep,
                                            int32_t* __restrict__ unsettled) {
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
        if (tid == 0) { hand_over(reinterpret_cast<unsigned long long*>(counts + R.pair), 0); keep[R.pair] = 0 < min_count ? 0 : 1; }
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
        hand_over(reinterpret_cast<unsigned long long*>(counts + R.pair), (unsigned long long)run);
        keep[R.pair] = run < min_count ? 0 : 1;
    }
}
// One workgroup per pair record, then the offsets: thread 0, which handed the pair's count over (hand_over), waits for it
// and takes a ticket; the workgroup that draws the last one (every count is stored and released) scans
// counts[0, n_pairs) into offsets[0, n_pairs] (scan_offsets_kernel's result) and puts the ticket back to 0.  The
// counts come from workgroups on other XCDs: device-scope atomic loads issued behind the ticket.  Nothing waits.
__global__ __launch_bounds__(1024)
void sift_finish_kernel(const PairRec* __restrict__ recs, const int32_t* __restrict__ qlist,
                        const int32_t* __restrict__ qmask, const int32_t* __restrict__ qcount,
                        unsigned long long* __restrict__ top2, const unsigned long long* __restrict__ slot1,
                        int2* __restrict__ slow_list, int32_t* __restrict__ slow_count,
                        const int8_t* __restrict__ desc8, const int32_t* __restrict__ norm,
                        const int32_t* __restrict__ out_idx, double ratio, int distinct, int min_count,
                        int64_t* __restrict__ counts, int32_t* __restrict__ keep, int32_t* __restrict__ unsettled,
                        int n_pairs, int64_t* __restrict__ offsets, int32_t* __restrict__ ticket) {
    extern __shared__ __attribute__((aligned(16))) unsigned bits[];   // seen | dup bitsets (distinct only)
    __shared__ int sh[32];
    __shared__ int s_slow, s_last;
    __shared__ long long wsum[16];
    finish_pair(bits, sh, s_slow, recs, qlist, qmask, qcount, top2, slot1, slow_list, slow_count, desc8, norm, out_idx, ratio,
                distinct, min_count, counts, keep, unsettled);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid == 0) {
        handed_over();
        s_last = atomicAdd(ticket, 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    long long run = 0;
    for (int c0 = 0; c0 < n_pairs; c0 += 1024) {
        const int i = c0 + tid;
        const long long v = i < n_pairs ? (long long)__hip_atomic_load(counts + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        long long incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const long long y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (lane == 63) wsum[wid] = incl;
        __syncthreads();
        long long base = 0, total = 0;
        for (int k = 0; k < 16; ++k) {
            const long long w = wsum[k];
            base += k < wid ? w : 0;
            total += w;
        }
        if (i < n_pairs) offsets[i] = run + base + incl - v;
        run += total;
        __syncthreads();
    }
    if (tid == 0) {
        offsets[n_pairs] = run;
        __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
hipError_t launch_prep_f32(const float* src, int rows, int cols, int rows_pad, float* dst, hipStream_t st) {
    const int64_t total = (int64_t)rows_pad * SIFT_DIM;
    if (total == 0) return hipSuccess;
    prep_f32_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(src, rows, cols, rows_pad, dst);
    return hipGetLastError();
}

hipError_t launch_prep_hamming_fp4(const uint8_t* src, int rows, int cols, int rows_pad, uint8_t* dst, int32_t* keyc,
                                   hipStream_t st) {
    if (rows_pad == 0) return hipSuccess;
    prep_hamming_fp4_kernel<<<(rows_pad + 7) / 8, 256, 0, st>>>(src, rows, cols, rows_pad,
                                                               reinterpret_cast<uint32_t*>(dst), keyc);
    return hipGetLastError();
}

// The product routes (MatchRoute's default value; queries per block = QT * WAVES * 32 divides ROW_ALIGN): for SIFT
// the FP6 screen with the exact pass 2 over the certified row subset, or over every row where there is none; for
// ORB the FP4 screen with the subset pass 2.  The diagnostic library's other routes are in match_diag.hip, whose
// dispatchers call these two functions for the product route.
//
// FP6 product path: 32-query tiles a wave of sift_rows_kernel carries per pass over its subset's rows.  Two fit
// the 128 VGPRs of four waves per SIMD without scratch (126); three spill 13 registers.
constexpr int SIFT_ROWS_QT = 2;
// FP6 product path: resident workgroups assumed for the full-row launch where the occupancy query fails (256 CUs x 4).
constexpr int SIFT_FULL_ROW_SLOTS = 1024;

// The full-row items of the pairs' second lists (`slot1`, counted behind the arena's qcount2): work2 holds up to
// n_work << 2 of them and the count stays on the device, so the grid is two resident rounds (or full_row_grid
// workgroups when that is not 0: MatchRoute), each workgroup looping over the list.
// compact: build the list here (compact_work_kernel); false where the kernel in front has built it (sift_rows_kernel).
hipError_t launch_sift_full_rows(const MatchBufs& b, int n_work, int n_pairs, double ratio, int full_row_grid, hipStream_t st,
                                 bool compact) {
    const int32_t* qlist2 = reinterpret_cast<const int32_t*>(b.slot1);
    const int32_t* qcount2 = b.qcount + arena_qcount2(n_pairs);
    if (compact) compact_work_kernel<7><<<1, 1024, 0, st>>>(b.porder, n_pairs, qcount2, b.work2, b.work2_n, SIFT_RIDE_MAX);
    static const int slots = resident_slots(sift_knn2_kernel<1, 4, 2, 128, false, true, true, true>, 256);
    const int grid = std::min(n_work << 2, full_row_grid > 0 ? full_row_grid : 2 * (slots > 0 ? slots : SIFT_FULL_ROW_SLOTS));
    sift_knn2_kernel<1, 4, 2, 128, false, true, true, true><<<grid, 256, 0, st>>>(
        b.work2, b.pairs, b.imgs, b.desc8, b.norm, b.keyc, nullptr, nullptr, nullptr, nullptr, ratio, b.qlist, qcount2,
        b.work2_n, b.top2, qlist2);
    return hipGetLastError();
}
// Conservative FP6 screen; exact pass 2 over the one certified row subset (one wave per pair and subset), and over
// every train row for the queries of the second list (128-query items).  The second list sits in `slot1`, idle
// here: no mask of this path has two bits.  qcount and qcount2: zeroed by the caller's one fill.  The caller
// settles with launch_finish_lists.  ev_screen: recorded behind the screen (pass-1 / pass-2 split of the timing).
hipError_t launch_sift_product(const MatchBufs& b, int n_work, int n_pairs, double ratio, int full_row_grid, hipStream_t st,
                               hipEvent_t ev_screen) {
    if (n_work == 0) return hipSuccess;
    int32_t* qlist2 = reinterpret_cast<int32_t*>(b.slot1);
    int32_t* qcount2 = b.qcount + arena_qcount2(n_pairs);
    sift_screen6_kernel<8, 4, 3, 128, true><<<n_work, 256, 0, st>>>(b.work, b.pairs, b.imgs, b.desc6, b.keyf, b.ne, b.imax,
                                                                   b.qlist, b.qcount, ratio, b.qmask, b.top2, qlist2, qcount2);
    if (ev_screen) {
        const hipError_t e = hipEventRecord(ev_screen, st);
        if (e != hipSuccess) return e;
    }
    sift_rows_kernel<SIFT_ROWS_QT><<<n_pairs * 4, 256, 0, st>>>(b.pairs, b.imgs, b.desc8, b.norm, b.qlist, b.qmask, b.qcount,
                                                                 qcount2, b.porder, b.top2, b.work2, b.work2_n, n_pairs);
    return launch_sift_full_rows(b, n_work, n_pairs, ratio, full_row_grid, st, false);   // workgroup 0 above built the list
}
// ORB pass 2 of np pairs: the subset kernel over the pairs porder[0, np), then the settle, one workgroup per pair
// (workgroup i: pair settle_order[i], or pair i of the run where settle_order is null).
hipError_t launch_orb_pass2(const MatchBufs& b, const int32_t* porder, int np, const int32_t* settle_order, double ratio,
                            hipStream_t st) {
    const uint8_t* desc4 = reinterpret_cast<const uint8_t*>(b.desc8);
    orb_subset_kernel<4, 2><<<np * 16, 256, 0, st>>>(b.pairs, b.imgs, desc4, b.qlist, b.qmask, b.qcount, porder, b.top2);
    orb_settle_kernel<<<np, 256, 0, st>>>(b.pairs, b.imgs, b.qlist, b.qcount, b.top2, b.dense_idx, b.dense_dist, ratio,
                                          settle_order);
    return hipGetLastError();
}
// FP4 screen, subset pass 2, settle into the dense arrays.
hipError_t launch_orb_product(const MatchBufs& b, int n_work, int n_pairs, double ratio, hipStream_t st, hipEvent_t ev_screen) {
    if (n_work == 0) return hipSuccess;
    const uint8_t* desc4 = reinterpret_cast<const uint8_t*>(b.desc8);
    orb_screen16_kernel<8, 4, 2, 64, true><<<n_work, 256, 0, st>>>(b.work, b.pairs, b.imgs, desc4, b.keyc, b.dense_idx,
                                                                  b.dense_dist, b.qlist, b.qcount, ratio, b.qmask, b.top2);
    if (ev_screen) {
        const hipError_t e = hipEventRecord(ev_screen, st);
        if (e != hipSuccess) return e;
    }
    return launch_orb_pass2(b, b.porder, n_pairs, nullptr, ratio, st);
}
hipError_t launch_sift_f32(const MatchBufs& b, int n_work32, double ratio, hipStream_t st) {
    if (n_work32 == 0) return hipSuccess;
    sift_f32_kernel<<<n_work32, 512, 0, st>>>(b.work32, nullptr, b.pairs, b.imgs, b.f32, b.dense_idx, b.dense_dist, ratio);
    return hipGetLastError();
}
hipError_t launch_assemble(const MatchBufs& b, int n_pairs, int distinct, int min_count, int max_nt, hipStream_t st) {
    if (n_pairs == 0) {
        (void)hipMemsetAsync(b.offsets, 0, sizeof(int64_t), st);
        return hipGetLastError();
    }
    const size_t shmem = distinct ? (size_t)2 * ((max_nt + 31) / 32) * 4 : 0;
    if (shmem > 150 * 1024) return hipErrorInvalidValue;
    assemble_kernel<0><<<n_pairs, 1024, shmem, st>>>(b.pairs, b.imgs, b.dense_idx, b.dense_dist, distinct, min_count, b.counts,
                                                     b.keep, nullptr, nullptr, b.unsettled);
    scan_offsets_kernel<<<1, 1024, 0, st>>>(b.counts, n_pairs, b.offsets);
    assemble_kernel<1><<<n_pairs, 1024, shmem, st>>>(b.pairs, b.imgs, b.dense_idx, b.dense_dist, distinct, min_count, b.counts,
                                                     b.keep, b.offsets, b.out, b.unsettled);
    return hipGetLastError();
}
// The list path's settle + assembly (after the screen and pass 2, and after the fp32 kernel of a mixed run):
// finish, whose last workgroup scans every pair's count into the offsets (ev_main is recorded behind it), write.
// One workgroup per record.
hipError_t launch_finish_lists(const MatchBufs& b, int n_pairs, double ratio, int distinct, int min_count, int max_nq,
                               int max_nt, hipStream_t st, hipEvent_t ev_main) {
    hipError_t e;
    if (n_pairs == 0) {
        (void)hipMemsetAsync(b.offsets, 0, sizeof(int64_t), st);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        return ev_main ? hipEventRecord(ev_main, st) : hipSuccess;
    }
    const size_t dup = distinct ? (size_t)2 * ((max_nt + 31) / 32) * 4 : 0;
    const size_t shmem = (size_t)2 * ((max_nq + 31) / 32) * 4 + dup;
    if (shmem > 150 * 1024) return hipErrorInvalidValue;
    sift_finish_kernel<<<n_pairs, 1024, dup, st>>>(b.recs, b.qlist, b.qmask, b.qcount, b.top2, b.slot1, b.slow_list,
                                                   b.slow_count, b.desc8, b.norm, b.dense_idx, ratio, distinct, min_count,
                                                   b.counts, b.keep, b.unsettled, n_pairs, b.offsets,
                                                   b.scratch + SCRATCH_FINISH);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev_main && (e = hipEventRecord(ev_main, st)) != hipSuccess) return e;
    assemble_lists_kernel<<<n_pairs, 1024, shmem, st>>>(b.recs, b.qlist, b.qcount, b.top2, b.dense_idx, b.dense_dist, distinct,
                                                        b.counts, b.offsets, b.out);
    return hipGetLastError();
}

}  // namespace sfmx
