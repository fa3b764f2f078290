// Vector-issue cost of the FP6 MFMA, block-scaled with unit scales and unscaled (fp6::mfma16 / mfma32: SHAPE 16 / 32
// against 16u / 32u, printed as 16x16x128u / 32x32x64u), under the SIFT screen's fold density: register-resident
// loops (no LDS, no global traffic inside the loop) on all 256 CUs, e2m3 operands quantised from SIFT-like
// rows (fp6::quant_m / code_of_m of v ~ Exp(20): the held clock depends on operand bits).
//   shape 16: v_mfma_scale_f32_16x16x128_f8f6f4, fresh C per MFMA, 0 / 1 / 2 v_max3_f32 per MFMA
//   shape 32: v_mfma_scale_f32_32x32x64_f8f6f4 as two chained MFMAs, 0 / 4 / 8 v_max3_f32 per chained pair
//             (the 8 are max3(ch[c], acc[c], acc[c + 8]))
// each at 1 and at 3 waves per SIMD (dynamic LDS sets how many 256-thread workgroups share a CU).
// Two more arms of shape 16u with 2 folds price the screen's LDS feed: the A fragments and keys of every 16-row block
// come from one LDS stage in sift_screen6_kernel's layout (plane A | plane B | keys, fp6::swz_a / swz_b), filled once
// before the loop; no LDS-DMA and no barrier inside it.
//   16u-lds:   a block's six reads, then the wait, then its MFMAs (the kernel's loop before the read-ahead)
//   16u-ahead: block n + 1's reads requested before block n's MFMAs, counted lgkmcnt (the kernel's loop:
//              screen6_request / screen6_arrived of match_device.hpp)
// One arm per process:  mfma_fp6_issue SHAPE[u][-lds|-ahead] FOLDS WAVES  -> one line: wall time per MFMA (per SIMD), the
// held clock (d s_memtime / d s_memrealtime x 100 MHz, median over workgroups), cycles per MFMA and ops/s
// as a fraction of the 10.07 PF FP6 peak.  Measurement only, never in the product.
//   hipcc --offload-arch=gfx950 -O3 -o tools/micro/mfma_fp6_issue tools/micro/mfma_fp6_issue.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../../sfm-mvs-pipeline_amd/csrc/match_device.hpp"   // (sift_fp6.hpp, the vector types, the read-ahead statements)

using namespace sfmx;

constexpr int NROWS = 1 << 14;   // host-filled rows, a power of two
constexpr int CUS = 256;

// lane group g's 192-bit fragment of a packed row
__device__ __forceinline__ i32x8 frag(const uint32_t* __restrict__ rows, int row, int g) {
    const uint32_t* p = rows + (row & (NROWS - 1)) * fp6::ROW_WORDS;
    return i32x8{(int)p[fp6::word_index(g, 0)], (int)p[fp6::word_index(g, 1)], (int)p[fp6::word_index(g, 2)],
                 (int)p[fp6::word_index(g, 3)], (int)p[fp6::word_index(g, 4)], (int)p[fp6::word_index(g, 5)], 0, 0};
}

struct Stamp { long long cyc, real; };

// 16 x 16 x 128: per iteration 8 query tiles x 2 row blocks = 16 MFMAs, FOLDS v_max3_f32 per MFMA
template <int FOLDS, bool SCALED>
__global__ __launch_bounds__(256, 3) void arm16(const uint32_t* __restrict__ rows, int iters, float* __restrict__ out,
                                                Stamp* __restrict__ st) {
    extern __shared__ char occupancy_lds[];
    const int lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
    const int base = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 160;
    i32x8 a[2], b[8];
    for (int k = 0; k < 2; ++k) a[k] = frag(rows, base + 16 * k + l16, g);
    for (int k = 0; k < 8; ++k) b[k] = frag(rows, base + 32 + 16 * k + l16, g);
    f32x4 key[2], acc[8][2];
    float ch[8][4];
    for (int k = 0; k < 2; ++k) key[k] = f32x4{-(float)(lane + k), -2.f, -3.f, -4.f};
    for (int q = 0; q < 8; ++q) {
        for (int k = 0; k < 2; ++k) acc[q][k] = key[k];
        for (int i = 0; i < 4; ++i) ch[q][i] = fp6::KEY_INIT;
    }
    const long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    // Folds run one tile behind their MFMAs (two result sets in turn, the order pinned), so that a lone wave
    // can issue them under the next tile's MFMAs.
    auto pair = [&](int q, f32x4& x, f32x4& y) {
        x = fp6::mfma16<fp6::FMT_E2M3, SCALED>(a[0], b[q], FOLDS == 0 ? acc[q][0] : key[0]);
        y = fp6::mfma16<fp6::FMT_E2M3, SCALED>(a[1], b[q], FOLDS == 0 ? acc[q][1] : key[1]);
    };
    if constexpr (FOLDS == 0) {
        for (int it = 0; it < iters; ++it) {
            asm volatile("" : "+v"(a[0]), "+v"(a[1]));   // new rows each iteration as far as the compiler knows
#pragma unroll
            for (int q = 0; q < 8; ++q) pair(q, acc[q][0], acc[q][1]);
        }
    } else {
        f32x4 x[2], y[2];
        pair(0, x[0], y[0]);
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (q == 7) asm volatile("" : "+v"(a[0]), "+v"(a[1]));
                pair((q + 1) & 7, x[(q + 1) & 1], y[(q + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 2 * FOLDS; ++i) ch[q][i] = fmaxf(fmaxf(ch[q][i], x[q & 1][i]), y[q & 1][i]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        acc[0][0] = x[0];   // the tile issued ahead of the last fold
        acc[0][1] = y[0];
    }
    const long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    float s = 0.f;
    for (int q = 0; q < 8; ++q)
        for (int i = 0; i < 4; ++i) s += ch[q][i] * 1e-30f + acc[q][0][i] + acc[q][1][i];
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if (threadIdx.x == 0) st[blockIdx.x] = Stamp{c1 - c0, r1 - r0};
}

// 16 x 16 x 128 unscaled, 2 folds per MFMA, operands of the row blocks from an LDS stage of 128 rows in the screen's
// layout: per iteration one stage = four 32-row blocks = 64 MFMAs (`iters` counts 32-row blocks, a multiple of 4).
template <bool AHEAD>
__global__ __launch_bounds__(256, 3) void arm16lds(const uint32_t* __restrict__ rows, int iters, float* __restrict__ out,
                                                   Stamp* __restrict__ st) {
    extern __shared__ __attribute__((aligned(16))) char occupancy_lds[];   // the stage is its first 12 800 B
    constexpr int STAGE = 128, A_BYTES = STAGE * 64, B_BYTES = STAGE * 32;
    char* lds = occupancy_lds;
    const int lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
    const int base = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 160;
    // the fill: what the kernel's LDS-DMA leaves (slot ^ swizzle of the row is the piece a slot holds)
    for (int i = threadIdx.x; i < STAGE * 4; i += 256) {
        const int r = i >> 2, slot = i & 3;
        const uint32_t* src = rows + ((blockIdx.x * STAGE + r) & (NROWS - 1)) * fp6::ROW_WORDS + 4 * (slot ^ fp6::swz_a(r));
        *reinterpret_cast<i32x4*>(lds + r * 64 + 16 * slot) = i32x4{(int)src[0], (int)src[1], (int)src[2], (int)src[3]};
    }
    for (int i = threadIdx.x; i < STAGE * 2; i += 256) {
        const int r = i >> 1, slot = i & 1;
        const uint32_t* src = rows + ((blockIdx.x * STAGE + r) & (NROWS - 1)) * fp6::ROW_WORDS + 16 + 4 * (slot ^ fp6::swz_b(r));
        *reinterpret_cast<i32x4*>(lds + A_BYTES + r * 32 + 16 * slot) = i32x4{(int)src[0], (int)src[1], (int)src[2], (int)src[3]};
    }
    for (int r = threadIdx.x; r < STAGE; r += 256) *reinterpret_cast<float*>(lds + A_BYTES + B_BYTES + 4 * r) = -(float)(r + 1);
    __syncthreads();
    i32x8 b[8];
    for (int k = 0; k < 8; ++k) b[k] = frag(rows, base + 32 + 16 * k + l16, g);
    float ch[8][4];
    for (int q = 0; q < 8; ++q)
        for (int i = 0; i < 4; ++i) ch[q][i] = fp6::KEY_INIT;
    const unsigned lds0 = (unsigned)(size_t)(LDS_AS const void*)lds;
    const unsigned pa = lds0 + l16 * 64 + 16 * (g ^ fp6::swz_a(l16));
    const unsigned pb = lds0 + A_BYTES + l16 * 32 + 16 * ((g >> 1) ^ fp6::swz_b(l16)) + 8 * (g & 1);
    const unsigned pk = lds0 + A_BYTES + B_BYTES + 16 * g;
    const long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    if constexpr (!AHEAD) {
        const char *qa = lds + (pa - lds0), *qb = lds + (pb - lds0), *qk = lds + (pk - lds0);
        for (int it = 0; it < iters; it += 4) {
            asm volatile("" ::: "memory");   // the stage may have changed as far as the compiler knows
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                i32x8 a[2];
                f32x4 cinit[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int blk = 2 * t + k;
                    const i32x4 lo = *reinterpret_cast<const i32x4*>(qa + blk * 16 * 64);
                    const long long hi = *(const volatile LDS_AS long long*)(qb + blk * 16 * 32);
                    a[k] = i32x8{lo.x, lo.y, lo.z, lo.w, (int)hi, (int)(hi >> 32), 0, 0};
                    cinit[k] = *reinterpret_cast<const f32x4*>(qk + blk * 16 * 4);
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const f32x4 x = fp6::mfma16<fp6::FMT_E2M3, false>(a[0], b[q], cinit[0]);
                    const f32x4 y = fp6::mfma16<fp6::FMT_E2M3, false>(a[1], b[q], cinit[1]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) ch[q][i] = fmaxf(fmaxf(ch[q][i], x[i]), y[i]);
                }
            }
        }
    } else {
#define SCREEN6_SET0 lo00, hi00, k00, lo01, hi01, k01
#define SCREEN6_SET1 lo10, hi10, k10, lo11, hi11, k11
        i32x4 lo00, lo01, lo10, lo11;
        i32x2 hi00, hi01, hi10, hi11;
        f32x4 k00, k01, k10, k11;
        screen6_request<0, 0>(SCREEN6_SET0, pa, pb, pk);
        for (int it = 0; it < iters; it += 4) {
            screen6_request<1, 1>(SCREEN6_SET1, pa, pb, pk);
            screen6_arrived<0, 6>(SCREEN6_SET0);
            screen6_mul<8>(b, ch, SCREEN6_SET0);
            screen6_request<0, 2>(SCREEN6_SET0, pa, pb, pk);
            screen6_arrived<1, 6>(SCREEN6_SET1);
            screen6_mul<8>(b, ch, SCREEN6_SET1);
            screen6_request<1, 3>(SCREEN6_SET1, pa, pb, pk);
            screen6_arrived<0, 6>(SCREEN6_SET0);
            screen6_mul<8>(b, ch, SCREEN6_SET0);
            screen6_request<0, 0>(SCREEN6_SET0, pa, pb, pk);
            screen6_arrived<1, 6>(SCREEN6_SET1);
            screen6_mul<8>(b, ch, SCREEN6_SET1);
        }
        screen6_arrived<0, 0>(SCREEN6_SET0);
#undef SCREEN6_SET0
#undef SCREEN6_SET1
    }
    const long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    float s = 0.f;
    for (int q = 0; q < 8; ++q)
        for (int i = 0; i < 4; ++i) s += ch[q][i];
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if (threadIdx.x == 0) st[blockIdx.x] = Stamp{c1 - c0, r1 - r0};
}

// 32 x 32 x 64: per iteration 4 query tiles x 2 chained MFMAs = 8 MFMAs, FOLDS v_max3_f32 per chained pair
template <int FOLDS, bool SCALED>
__global__ __launch_bounds__(256, 3) void arm32(const uint32_t* __restrict__ rows, int iters, float* __restrict__ out,
                                                Stamp* __restrict__ st) {
    extern __shared__ char occupancy_lds[];
    const int lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    const int base = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 160;
    i32x8 a[2], b[4][2];
    for (int m = 0; m < 2; ++m) a[m] = frag(rows, base + l32, 2 * m + h);
    for (int q = 0; q < 4; ++q)
        for (int m = 0; m < 2; ++m) b[q][m] = frag(rows, base + 32 + 32 * q + l32, 2 * m + h);
    f32x16 key, acc[4];
    float ch[4][8];
    for (int i = 0; i < 16; ++i) key[i] = -(float)(lane + i);
    for (int q = 0; q < 4; ++q) {
        acc[q] = key;
        for (int c = 0; c < 8; ++c) ch[q][c] = fp6::KEY_INIT;
    }
    const long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    auto pair = [&](int q, f32x16& x) {
        x = fp6::mfma32<fp6::FMT_E2M3, SCALED>(a[0], b[q][0], FOLDS == 0 ? acc[q] : key);
        x = fp6::mfma32<fp6::FMT_E2M3, SCALED>(a[1], b[q][1], x);
    };
    if constexpr (FOLDS == 0) {
        for (int it = 0; it < iters; ++it) {
            asm volatile("" : "+v"(a[0]), "+v"(a[1]));
#pragma unroll
            for (int q = 0; q < 4; ++q) pair(q, acc[q]);
        }
    } else {
        f32x16 x[2];   // folds one tile behind, as in arm16
        pair(0, x[0]);
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q == 3) asm volatile("" : "+v"(a[0]), "+v"(a[1]));
                pair((q + 1) & 3, x[(q + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int c = 0; c < FOLDS; ++c) ch[q][c] = fmaxf(fmaxf(ch[q][c], x[q & 1][c]), x[q & 1][c + 8]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        acc[0] = x[0];
    }
    const long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    float s = 0.f;
    for (int q = 0; q < 4; ++q) {
        for (int c = 0; c < 8; ++c) s += ch[q][c] * 1e-30f;
        for (int i = 0; i < 16; ++i) s += acc[q][i];
    }
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if (threadIdx.x == 0) st[blockIdx.x] = Stamp{c1 - c0, r1 - r0};
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

typedef void (*Arm)(const uint32_t*, int, float*, Stamp*);

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s SHAPE(16|32|16u|32u|16u-lds|16u-ahead) FOLDS WAVES(1|3) [seconds]\n", argv[0]); return 2; }
    const int shape = atoi(argv[1]), folds = atoi(argv[2]), waves = atoi(argv[3]);
    const bool unscaled = strchr(argv[1], 'u') != nullptr;   // 16u / 32u: the plain v_mfma_f32_*_f8f6f4
    const double seconds = argc > 4 ? atof(argv[4]) : 2.0;
    Arm k = nullptr;
    if (shape == 16 && !unscaled) k = folds == 0 ? arm16<0, true> : folds == 1 ? arm16<1, true> : folds == 2 ? arm16<2, true> : nullptr;
    if (shape == 32 && !unscaled) k = folds == 0 ? arm32<0, true> : folds == 4 ? arm32<4, true> : folds == 8 ? arm32<8, true> : nullptr;
    if (shape == 16 && unscaled) k = folds == 0 ? arm16<0, false> : folds == 1 ? arm16<1, false> : folds == 2 ? arm16<2, false> : nullptr;
    if (shape == 32 && unscaled) k = folds == 0 ? arm32<0, false> : folds == 4 ? arm32<4, false> : folds == 8 ? arm32<8, false> : nullptr;
    const bool from_lds = strstr(argv[1], "-lds") != nullptr, ahead = strstr(argv[1], "-ahead") != nullptr;
    if (from_lds || ahead) k = shape == 16 && unscaled && folds == 2 ? (ahead ? arm16lds<true> : arm16lds<false>) : nullptr;
    if (!k || (waves != 1 && waves != 3)) { fprintf(stderr, "no such arm\n"); return 2; }
    const int mfma_per_iter = shape == 16 ? 16 : 8;
    const double ops_per_mfma = shape == 16 ? 16.0 * 16 * 128 * 2 : 32.0 * 32 * 64 * 2;
    // 160 KB of LDS per CU: 96 KB lets one workgroup (one wave per SIMD) in, 48 KB three
    const int lds = waves == 1 ? 96 * 1024 : 48 * 1024, blocks = CUS * waves;

    std::vector<uint32_t> h((size_t)NROWS * fp6::ROW_WORDS);
    std::mt19937 rng(7);
    std::exponential_distribution<double> ex(1.0 / 20.0);
    for (int r = 0; r < NROWS; ++r) {
        unsigned codes[128];
        for (int i = 0; i < 128; ++i)
            codes[i] = fp6::code_of_m(fp6::quant_m((int)std::min(255.0, ex(rng)) - fp6::OFFSET));
        fp6::pack_row(codes, h.data() + (size_t)r * fp6::ROW_WORDS);
    }
    uint32_t* d_rows;
    float* d_out;
    Stamp* d_st;
    CHECK(hipMalloc(&d_rows, h.size() * 4));
    CHECK(hipMalloc(&d_out, (size_t)blocks * 256 * 4));
    CHECK(hipMalloc(&d_st, (size_t)blocks * sizeof(Stamp)));
    CHECK(hipMemcpy(d_rows, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    int occ = 0;
    CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)k, 256, lds));
    if (occ != waves) { fprintf(stderr, "occupancy %d workgroups per CU, wanted %d\n", occ, waves); return 3; }

    // launches of ~20 ms, back to back for `seconds`; the last five are timed
    int iters = 20000;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    float ms = 0.f;
    CHECK(hipEventRecord(e0));
    k<<<blocks, 256, lds>>>(d_rows, iters, d_out, d_st);
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    iters = std::max(1000, (int)(iters * 20.0 / std::max(ms, 0.01f))) & ~3;   // (the LDS arms run whole stages of four blocks)
    const auto t0 = std::chrono::steady_clock::now();
    while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < seconds) {
        for (int i = 0; i < 4; ++i) k<<<blocks, 256, lds>>>(d_rows, iters, d_out, d_st);
        CHECK(hipDeviceSynchronize());
    }
    std::vector<float> t(5);
    std::vector<double> ghz;
    for (int r = 0; r < 5; ++r) {
        CHECK(hipEventRecord(e0));
        k<<<blocks, 256, lds>>>(d_rows, iters, d_out, d_st);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&t[r], e0, e1));
    }
    std::vector<Stamp> st(blocks);
    CHECK(hipMemcpy(st.data(), d_st, (size_t)blocks * sizeof(Stamp), hipMemcpyDeviceToHost));
    for (const Stamp& s : st)
        if (s.real > 0) ghz.push_back((double)s.cyc / (double)s.real * 0.1);
    std::sort(ghz.begin(), ghz.end());
    std::sort(t.begin(), t.end());
    const double clock = ghz.empty() ? 0.0 : ghz[ghz.size() / 2], wall = t[2] * 1e-3;
    // every SIMD runs `waves` waves of iters * mfma_per_iter MFMAs each
    const double per_simd = (double)waves * iters * mfma_per_iter;
    const double ns = wall / per_simd * 1e9, cyc = ns * clock;
    const double frac = per_simd * CUS * 4 * ops_per_mfma / wall / 10.07e15;
    printf("%dx%dx%d%s%s  %d v_max3 per %s  %d wave/SIMD  %7.3f ns/MFMA  clock %.3f GHz  %6.2f cyc/MFMA  %.3f of 10.07 PF  "
           "(%.2f ms, min %.2f max %.2f)\n",
           shape, shape, shape == 16 ? 128 : 64, unscaled ? "u" : " ", from_lds ? "-lds  " : ahead ? "-ahead" : "", folds, shape == 16 ? "MFMA" : "pair", waves, ns, clock, cyc, frac, t[2],
           t[0], t[4]);
    return 0;
}
