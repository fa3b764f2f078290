// SPDX-License-Identifier: MIT
// sfmx — point-cloud neighbour statistics (include/sfmx_cloud.h).
//
// sfmx_cloud_neighbor_distances: for every point i of a cloud, over all points j (i included), with FLANN's
// float distance d = (dx*dx + dy*dy) + dz*dz (no FMA: this file is built with -ffp-contract=off; f32
// subnormals are kept, hipcc's default),
//     z = #{ j : d == 0 }      m = min{ d : d > 0 }      neighbour = smallest j attaining m
// and the distance is 0 if z >= Ke or no positive d exists, else sqrt((double)m).
//
// Exact search on a uniform grid, all on the caller's stream, no host round trip before the results:
//   cloud_minmax_kernel      min / max of the finite points per axis
//   cloud_hist_kernel x 3    per-axis histogram of the current interval (LDS, then one flush per block)
//   cloud_pick_kernel  x 4   inner-quantile interval of each round; the last one fixes the grid: origin, cell
//                            edge h (cubic cells, about one cell per point), cells per axis, the stop bounds
//   cloud_count_kernel       cell of every point (double: monotone in the coordinate), its rank in the cell
//   cloud_refine_kernel      more than 4 points per occupied cell (sheets, clusters): a finer grid, counted again
//   cloud_scan_* (3)         exclusive scan of the cell counts
//   cloud_scatter_kernel     (x, y, z, original index) into cell order
//   cloud_search_kernel      one thread per point in cell order: rings r = 0, 1, 2 of cells by Chebyshev index
//                            distance; stops after ring r when z >= Ke, when the rings cover the grid, or when
//                            m < bound[r] <= the float d of every unvisited point (derivation: DESIGN.md §8j)
//   cloud_brute_kernel       the queries the rings did not finish against all points: one wave per (4 queries,
//                            4096 points), a wave reduction, one 64-bit atomic min per query; then _emit
// Cell indices are clamped to the grid, so the border cells are half-spaces and the result does not depend
// on the box; the box only decides how many queries end in the brute-force kernel.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/sfmx_cloud.h"
#include "cloud_host.hpp"
#include "device_call.hpp"
#include "match_common.hpp"

namespace sfmx {
namespace cloud {

constexpr int BLOCK = 256;
constexpr int BINS = 1024;        // histogram bins per axis and round
static_assert(BINS == 1024, "cloud_pick_kernel runs one thread per bin in one block");
constexpr int ROUNDS = 3;         // each round narrows an axis interval by up to BINS / 2
constexpr int RMAX = 2;           // rings 0 .. RMAX (125 cells) before a query goes to the brute-force kernel
constexpr int GMAX = 4096;        // cells per axis (the stop-rule margin assumes it)
constexpr int SCAN_PER_THREAD = 16;
constexpr int SCAN_TILE = BLOCK * SCAN_PER_THREAD;
constexpr unsigned NONE = 0xffffffffu;
constexpr unsigned long long KEY_NONE = ((unsigned long long)0x7f800000u << 32) | NONE;   // (+inf, no index)

struct Plan {                      // device resident, zeroed at the start of a call
    unsigned enc_max[3];           // ordered encodings of max(x) and max(-x) per axis; 0 = no finite point
    unsigned enc_negmax[3];
    unsigned n_finite;
    unsigned n_brute;              // queries handed to the brute-force kernel
    unsigned error;                // a scatter position outside [0, n): self check
    unsigned refined;              // the second, finer grid is in use
    unsigned long long evals;      // evaluations of d
    double lo[3], hi[3];           // the interval of the current histogram round, then the grid box
    double inv;                    // 1 / h
    int G[3];
    int n_cells;
    float bound[RMAX + 1];
    unsigned occupied;             // cells of the first grid that hold a point
    double ext[3];                 // extents of the box (0: a flat axis)
    unsigned hist[3 * BINS];
};

__device__ inline unsigned enc_order(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float dec_order(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e ^ 0x80000000u) : ~e); }
__device__ inline bool finite3(float x, float y, float z) {
    return fabsf(x) <= 3.402823466e38f && fabsf(y) <= 3.402823466e38f && fabsf(z) <= 3.402823466e38f;   // false for NaN
}
__device__ inline unsigned wave_max(unsigned v) {
    for (int o = 32; o; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
    return v;
}
__device__ inline unsigned long long wave_sum(unsigned long long v) {
    for (int o = 32; o; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

__global__ __launch_bounds__(BLOCK)
void cloud_minmax_kernel(const float* __restrict__ xyz, int64_t n, Plan* __restrict__ P) {
    unsigned mx[3] = {0, 0, 0}, ng[3] = {0, 0, 0}, cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if (!finite3(x, y, z)) continue;
        ++cnt;
        mx[0] = max(mx[0], enc_order(x)); ng[0] = max(ng[0], enc_order(-x));
        mx[1] = max(mx[1], enc_order(y)); ng[1] = max(ng[1], enc_order(-y));
        mx[2] = max(mx[2], enc_order(z)); ng[2] = max(ng[2], enc_order(-z));
    }
    // per wave, then per block through LDS, then one atomic per block and word -- and none where the word already
    // holds as much (a stale read only costs an atomic: the maximum never decreases)
    __shared__ unsigned sh[BLOCK / 64][7];
    const unsigned long long total = wave_sum(cnt);
    for (int a = 0; a < 3; ++a) { mx[a] = wave_max(mx[a]); ng[a] = wave_max(ng[a]); }
    if ((threadIdx.x & 63) == 0) {
        unsigned* w = sh[threadIdx.x >> 6];
        for (int a = 0; a < 3; ++a) { w[a] = mx[a]; w[3 + a] = ng[a]; }
        w[6] = (unsigned)total;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        unsigned v = 0;
        for (int k = 0; k < BLOCK / 64; ++k) v = threadIdx.x < 6 ? max(v, sh[k][threadIdx.x]) : v + sh[k][6];
        if (threadIdx.x == 6) { if (v) atomicAdd(&P->n_finite, v); }
        else {
            unsigned* dst = threadIdx.x < 3 ? &P->enc_max[threadIdx.x] : &P->enc_negmax[threadIdx.x - 3];
            if (v > *dst) atomicMax(dst, v);
        }
    }
}

// Cells per axis for cubic cells of edge h over the extents e (0: a flat axis, one cell): h grows until every axis
// has at most GMAX cells and the grid at most `limit`.  false: no such grid within 96 steps.
__device__ inline bool fit_grid(const double e[3], double& h, int64_t limit, int G[3]) {
    for (int it = 0; it < 96; ++it) {
        double prod = 1.0;
        bool ok = true;
        for (int a = 0; a < 3; ++a) {
            const double g = e[a] > 0.0 ? fmax(1.0, ceil(e[a] / h)) : 1.0;
            if (!(g <= (double)GMAX)) ok = false;
            prod *= g;
            G[a] = ok ? (int)g : 1;
        }
        if (ok && prod <= (double)limit) return true;
        h *= 1.2599210498948732;
    }
    return false;
}

struct Plan;
__device__ inline void set_grid(Plan* P, double h, const int G[3]);

__device__ inline int hist_bin(float x, double lo, double scale) {
    const double u = ((double)x - lo) * scale;
    return !(u >= 0.0) ? 0 : (u >= (double)(BINS - 1) ? BINS - 1 : (int)u);
}

__global__ __launch_bounds__(BLOCK)
void cloud_hist_kernel(const float* __restrict__ xyz, int64_t n, Plan* __restrict__ P) {
    __shared__ unsigned h[3 * BINS];
    for (int k = threadIdx.x; k < 3 * BINS; k += BLOCK) h[k] = 0;
    __syncthreads();
    double lo[3], sc[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = P->lo[a];
        const double w = P->hi[a] - lo[a];
        sc[a] = w > 0.0 ? (double)BINS / w : 0.0;
    }
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if (!finite3(x, y, z)) continue;
        atomicAdd(&h[hist_bin(x, lo[0], sc[0])], 1u);
        atomicAdd(&h[BINS + hist_bin(y, lo[1], sc[1])], 1u);
        atomicAdd(&h[2 * BINS + hist_bin(z, lo[2], sc[2])], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 3 * BINS; k += BLOCK)
        if (h[k]) atomicAdd(&P->hist[k], h[k]);
}

// One block of BINS threads.  round 0: the interval is the bounding box.  round 1 .. ROUNDS: the bins holding the
// inner 96 % of the last histogram become the interval (a prefix sum per axis in LDS).  After the last round
// thread 0 fixes the grid.
__global__ __launch_bounds__(BINS)
void cloud_pick_kernel(Plan* __restrict__ P, int round, int64_t cells_target) {
    __shared__ unsigned cum[BINS];
    __shared__ int sb0, sb1;
    const int t = threadIdx.x;
    const unsigned nf = P->n_finite;
    if (round == 0) {
        if (t < 3) {
            P->lo[t] = nf ? -(double)dec_order(P->enc_negmax[t]) : 0.0;
            P->hi[t] = nf ? (double)dec_order(P->enc_max[t]) : 0.0;
        }
        return;
    }
    const unsigned q = max(1u, nf / 50u);
    for (int a = 0; a < 3; ++a) {
        cum[t] = P->hist[a * BINS + t];
        P->hist[a * BINS + t] = 0;
        if (t == 0) sb0 = sb1 = BINS - 1;
        __syncthreads();
        for (int o = 1; o < BINS; o <<= 1) {
            const unsigned add = t >= o ? cum[t - o] : 0u;
            __syncthreads();
            cum[t] += add;
            __syncthreads();
        }
        if (cum[t] >= q) atomicMin(&sb0, t);                // the first bin that reaches the lower cut
        if (cum[t] + q >= nf + 1u) atomicMin(&sb1, t);      // the first bin that reaches the upper cut
        __syncthreads();
        if (t == 0) {
            const int b0 = sb0, b1 = max(sb1, sb0);
            const double lo = P->lo[a], w = (P->hi[a] - lo) / (double)BINS;
            if (w > 0.0 && nf) {
                P->lo[a] = lo + (double)b0 * w;
                P->hi[a] = lo + (double)(b1 + 1) * w;
            }
        }
        __syncthreads();
    }
    if (round < ROUNDS || t) return;
    // the grid: the interval widened by 5 % on each side; cubic cells of edge h, about cells_target of them
    double e[3], vol = 1.0, emax = 0.0;
    int k = 0;
    for (int a = 0; a < 3; ++a) {
        const double w = P->hi[a] - P->lo[a];
        if (w > 0.0 && w < 1e300) {
            P->lo[a] -= 0.05 * w;
            P->hi[a] += 0.05 * w;
        }
        e[a] = P->hi[a] - P->lo[a];
        if (!(e[a] > 0.0) || !(e[a] < 1e300)) e[a] = 0.0;
        if (e[a] > 0.0) { vol *= e[a]; ++k; emax = fmax(emax, e[a]); }
    }
    double h = 1.0;
    int G[3] = {1, 1, 1};
    if (k > 0) {
        h = pow(vol / (double)cells_target, 1.0 / (double)k);
        if (!(h > 0.0) || !(h < 1e300)) h = emax;
        if (!fit_grid(e, h, 2 * cells_target, G)) { h = emax; G[0] = G[1] = G[2] = 1; }
    }
    for (int a = 0; a < 3; ++a) P->ext[a] = e[a];
    set_grid(P, h, G);
}

__device__ inline void set_grid(Plan* P, double h, const int G[3]) {
    P->inv = 1.0 / h;
    for (int a = 0; a < 3; ++a) P->G[a] = G[a];
    P->n_cells = G[0] * G[1] * G[2];
    P->bound[0] = 0.f;
    for (int r = 1; r <= RMAX; ++r) {
        const double B = ((double)r * h) * ((double)r * h) * (1.0 - 9.5367431640625e-07);   // 1 - 2^-20
        P->bound[r] = !(B >= 4.8e-38) ? 0.f : (B > 3.0e38 ? __uint_as_float(0x7f800000u) : (float)B);
    }
}

// One thread, after the first count: a cloud of sheets or clusters leaves most cells of the first grid empty
// and tens of points in the others.  With more than 4 points per occupied cell the edge shrinks by
// sqrt(occupancy / 2) (a sheet then holds about 2 per cell), at most 4 times and within cells_limit cells;
// the points are then counted again on the finer grid.
__global__ void cloud_refine_kernel(Plan* __restrict__ P, int64_t cells_limit) {
    if (threadIdx.x || blockIdx.x) return;
    const unsigned occ = P->occupied, nf = P->n_finite;
    if (!occ || (double)nf <= 4.0 * (double)occ) return;
    const double f = fmin(4.0, sqrt((double)nf / (2.0 * (double)occ)));
    double h = (1.0 / P->inv) / f;
    double e[3] = {P->ext[0], P->ext[1], P->ext[2]};
    int G[3];
    if (!(h > 0.0) || !fit_grid(e, h, cells_limit, G)) return;
    if (G[0] * G[1] * G[2] <= P->n_cells) return;
    set_grid(P, h, G);
    P->refined = 1u;
}

__device__ inline int cell_axis(float x, double lo, double inv, int G) {   // monotone non-decreasing in x
    double u = floor(((double)x - lo) * inv);
    u = fmin(fmax(u, 0.0), (double)(G - 1));
    return (int)u;
}

__global__ __launch_bounds__(BLOCK)
void cloud_count_kernel(const float* __restrict__ xyz, int64_t n, const Plan* __restrict__ P, unsigned* __restrict__ count,
                        int* __restrict__ cell, unsigned* __restrict__ rank, int pass) {
    if (pass && !P->refined) return;   // the second pass runs only on a refined grid
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = i < n;
    int c = 0;
    if (valid) {
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if (finite3(x, y, z)) {
            const double inv = P->inv;
            const int cx = cell_axis(x, P->lo[0], inv, P->G[0]), cy = cell_axis(y, P->lo[1], inv, P->G[1]),
                      cz = cell_axis(z, P->lo[2], inv, P->G[2]);
            c = (cz * P->G[1] + cy) * P->G[0] + cx;
        } else {
            c = P->n_cells;   // the bucket after the grid: never a candidate
        }
    }
    // lanes that share a cell add once (up to four distinct cells per wave; the rest add one by one)
    unsigned r = 0;
    bool done = !valid;
    for (int it = 0; it < 4; ++it) {
        const unsigned long long rem = __ballot(!done);
        if (!rem) break;
        const int leader = __ffsll((long long)rem) - 1;
        const int lc = __shfl(c, leader);
        const bool same = !done && c == lc;
        const unsigned long long mask = __ballot(same);
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(&count[lc], (unsigned)__popcll(mask));
        base = (unsigned)__shfl((int)base, leader);
        if (same) {
            r = base + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
            done = true;
        }
    }
    if (!done) r = atomicAdd(&count[c], 1u);
    if (valid) { cell[i] = c; rank[i] = r; }
}

__device__ inline unsigned block_exclusive_scan(unsigned v, unsigned* sh, unsigned& total) {   // BLOCK threads
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < BLOCK; o <<= 1) {
        const unsigned add = t >= o ? sh[t - o] : 0u;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    total = sh[BLOCK - 1];
    const unsigned ex = sh[t] - v;
    __syncthreads();
    return ex;
}

__global__ __launch_bounds__(BLOCK)
void cloud_scan_reduce_kernel(const unsigned* __restrict__ a, int64_t m, unsigned* __restrict__ bsum, Plan* __restrict__ P, int pass) {
    __shared__ unsigned sh[BLOCK];
    if (pass && !P->refined) return;
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_PER_THREAD;
    const int64_t grid_cells = P->n_cells;   // the bucket after the grid is not a cell
    if ((int64_t)blockIdx.x * SCAN_TILE > grid_cells + 1) {   // past the grid, its extra bucket and the end: all zero
        if (threadIdx.x == 0) bsum[blockIdx.x] = 0u;
        return;
    }
    unsigned s = 0, nz = 0;
    for (int k = 0; k < SCAN_PER_THREAD; ++k)
        if (base + k < m) {
            const unsigned v = a[base + k];
            s += v;
            nz += v != 0u && base + k < grid_cells;
        }
    unsigned total;
    (void)block_exclusive_scan(s, sh, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
    if (!pass) {   // occupied cells of the first grid
        const unsigned long long w = wave_sum(nz);
        if ((threadIdx.x & 63) == 0 && w) atomicAdd(&P->occupied, (unsigned)w);
    }
}

__global__ __launch_bounds__(BLOCK)
void cloud_rezero_kernel(unsigned* __restrict__ a, int64_t m, const Plan* __restrict__ P) {   // before the second count
    if (!P->refined) return;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * BLOCK) a[i] = 0u;
}

__global__ __launch_bounds__(BLOCK)
void cloud_scan_top_kernel(unsigned* __restrict__ bsum, int nb) {   // one block: exclusive scan of the block sums
    __shared__ unsigned sh[BLOCK];
    const int per = (nb + BLOCK - 1) / BLOCK, b0 = threadIdx.x * per, b1 = min(nb, b0 + per);
    unsigned s = 0;
    for (int b = b0; b < b1; ++b) s += bsum[b];
    unsigned total;
    unsigned run = block_exclusive_scan(s, sh, total);
    for (int b = b0; b < b1; ++b) {
        const unsigned v = bsum[b];
        bsum[b] = run;
        run += v;
    }
}

__global__ __launch_bounds__(BLOCK)
void cloud_scan_apply_kernel(unsigned* __restrict__ a, int64_t m, const unsigned* __restrict__ bsum, const Plan* __restrict__ P) {
    __shared__ unsigned sh[BLOCK];
    if ((int64_t)blockIdx.x * SCAN_TILE > (int64_t)P->n_cells + 1) return;   // nothing reads the offsets past the grid's end
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_PER_THREAD;
    unsigned v[SCAN_PER_THREAD], s = 0;
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
        v[k] = base + k < m ? a[base + k] : 0u;
        s += v[k];
    }
    unsigned total;
    unsigned run = block_exclusive_scan(s, sh, total) + bsum[blockIdx.x];
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
        if (base + k < m) a[base + k] = run;
        run += v[k];
    }
}

__global__ __launch_bounds__(BLOCK)
void cloud_scatter_kernel(const float* __restrict__ xyz, int64_t n, const unsigned* __restrict__ start, const int* __restrict__ cell,
                          const unsigned* __restrict__ rank, float4* __restrict__ sorted, Plan* __restrict__ P) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t pos = (uint64_t)start[cell[i]] + rank[i];
    if (pos >= (uint64_t)n) { P->error = 1u; return; }
    sorted[pos] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], __uint_as_float((unsigned)i));
}

struct Best {
    float m;          // smallest positive d, +inf before any
    unsigned idx;     // the smallest original index attaining it
    unsigned z;       // points at d == 0 (the query itself included)
    unsigned ev;
};

__device__ inline void eval(const float4 q, const float4 p, Best& b) {
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    const float d = (dx * dx + dy * dy) + dz * dz;   // FLANN L2_Simple<float>; uncontracted
    const unsigned j = __float_as_uint(p.w);
    ++b.ev;
    if (d == 0.f) ++b.z;
    else if (d < b.m || (d == b.m && j < b.idx)) { b.m = d; b.idx = j; }
}

__device__ inline void emit(const Best& b, unsigned ke, unsigned orig, int64_t n, Plan* __restrict__ P,
                            double* __restrict__ out_distance, int64_t* __restrict__ out_neighbor) {
    if ((int64_t)orig >= n) { P->error = 1u; return; }   // self check: never writes outside the outputs
    const bool zero = b.z >= ke || b.idx == NONE;
    out_distance[orig] = zero ? 0.0 : __dsqrt_rn((double)b.m);
    if (out_neighbor) out_neighbor[orig] = zero ? (int64_t)-1 : (int64_t)b.idx;
}

__global__ __launch_bounds__(BLOCK)
void cloud_search_kernel(const float4* __restrict__ sorted, int64_t n, const unsigned* __restrict__ start, Plan* __restrict__ P,
                         unsigned ke, unsigned* __restrict__ brute, unsigned long long* __restrict__ bkey, unsigned* __restrict__ bz,
                         double* __restrict__ out_distance, int64_t* __restrict__ out_neighbor) {
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    Best b{__uint_as_float(0x7f800000u), NONE, 0u, 0u};
    if (t < n) {
        const float4 q = sorted[t];
        const unsigned orig = __float_as_uint(q.w);
        if (t >= (int64_t)P->n_finite) {            // a non-finite point
            emit(b, 0u, orig, n, P, out_distance, out_neighbor);   // z >= 0: distance 0, neighbour -1
        } else {
            const int Gx = P->G[0], Gy = P->G[1], Gz = P->G[2];
            const double inv = P->inv;
            const int cx = cell_axis(q.x, P->lo[0], inv, Gx), cy = cell_axis(q.y, P->lo[1], inv, Gy),
                      cz = cell_axis(q.z, P->lo[2], inv, Gz);
            bool done = false;
            for (int r = 0; r <= RMAX && !done; ++r) {
                const int x0 = max(cx - r, 0), x1 = min(cx + r, Gx - 1), y0 = max(cy - r, 0), y1 = min(cy + r, Gy - 1),
                          z0 = max(cz - r, 0), z1 = min(cz + r, Gz - 1);
                for (int zz = z0; zz <= z1; ++zz)
                    for (int yy = y0; yy <= y1; ++yy) {
                        const int row = (zz * Gy + yy) * Gx;
                        const bool shell = abs(zz - cz) == r || abs(yy - cy) == r;
                        // the cells of a row are contiguous in the sorted order: a shell row is one run,
                        // an inner row contributes its two end cells
                        for (int part = 0; part < 2; ++part) {
                            int xa, xb;
                            if (shell) { if (part) break; xa = x0; xb = x1; }
                            else if (part == 0) { xa = xb = cx - r; if (xa < 0) continue; }
                            else { xa = xb = cx + r; if (xa > Gx - 1 || r == 0) continue; }
                            const unsigned s = start[row + xa], e = start[row + xb + 1];
                            for (unsigned j = s; j < e; ++j) eval(q, sorted[j], b);
                        }
                    }
                const bool covered = cx - r <= 0 && cx + r >= Gx - 1 && cy - r <= 0 && cy + r >= Gy - 1 && cz - r <= 0 &&
                                     cz + r >= Gz - 1;
                done = b.z >= ke || covered || b.m < P->bound[r];
            }
            if (done) emit(b, ke, orig, n, P, out_distance, out_neighbor);
            else {   // to the brute-force kernel, with its accumulators cleared
                const unsigned slot = atomicAdd(&P->n_brute, 1u);
                brute[slot] = (unsigned)t;
                bkey[slot] = KEY_NONE;
                bz[slot] = 0u;
            }
        }
    }
    const unsigned long long ev = wave_sum(b.ev);
    if ((threadIdx.x & 63) == 0 && ev) atomicAdd(&P->evals, ev);
}

constexpr int QB = 4;          // queries one wave resolves together: a point is loaded once for all of them
constexpr int BRUTE_CHUNK = 4096;   // points of one wave task

// One wave per (group of QB queries, chunk of BRUTE_CHUNK points): coalesced over the chunk, a wave reduction,
// then per query one 64-bit atomic min on (float bits of m, index) -- for d > 0 the bits order like the values,
// so the minimum is the smallest m and, among equals, the smallest index -- and one atomic add on z.
__global__ __launch_bounds__(BLOCK)
void cloud_brute_kernel(const float4* __restrict__ sorted, int64_t n, Plan* __restrict__ P, const unsigned* __restrict__ brute,
                        unsigned long long* __restrict__ bkey, unsigned* __restrict__ bz) {
    const unsigned nq = min(P->n_brute, (unsigned)n), nf = min(P->n_finite, (unsigned)n);
    const int lane = threadIdx.x & 63;
    const unsigned wave = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), n_waves = gridDim.x * (BLOCK / 64);
    const unsigned groups = (nq + QB - 1) / QB, chunks = (nf + BRUTE_CHUNK - 1) / BRUTE_CHUNK;
    const unsigned long long tasks = (unsigned long long)groups * chunks;
    unsigned long long ev = 0;
    for (unsigned long long task = wave; task < tasks; task += n_waves) {
        const unsigned g = (unsigned)(task % groups), c = (unsigned)(task / groups);   // neighbouring waves share a chunk
        float4 q[QB];
        Best b[QB];
        bool live[QB];
        for (int u = 0; u < QB; ++u) {
            const unsigned k = g * QB + u;
            live[u] = k < nq;
            const unsigned t = live[u] ? brute[k] : 0u;
            if ((int64_t)t >= n) { live[u] = false; if (lane == 0) P->error = 1u; }
            q[u] = live[u] ? sorted[t] : make_float4(0.f, 0.f, 0.f, 0.f);
            b[u] = Best{__uint_as_float(0x7f800000u), NONE, 0u, 0u};
        }
        const unsigned j1 = min(nf, (c + 1u) * BRUTE_CHUNK);
        for (unsigned j = c * BRUTE_CHUNK + lane; j < j1; j += 64) {
            const float4 p = sorted[j];
            for (int u = 0; u < QB; ++u)
                if (live[u]) eval(q[u], p, b[u]);
        }
        for (int u = 0; u < QB; ++u) {
            if (!live[u]) continue;   // wave-uniform
            ev += b[u].ev;
            for (int o = 32; o; o >>= 1) {
                const float om = __shfl_xor(b[u].m, o);
                const unsigned oi = (unsigned)__shfl_xor((int)b[u].idx, o), oz = (unsigned)__shfl_xor((int)b[u].z, o);
                b[u].z += oz;
                if (om < b[u].m || (om == b[u].m && oi < b[u].idx)) { b[u].m = om; b[u].idx = oi; }
            }
            if (lane == 0) {
                const unsigned k = g * QB + u;
                if (b[u].idx != NONE) atomicMin(&bkey[k], ((unsigned long long)__float_as_uint(b[u].m) << 32) | b[u].idx);
                if (b[u].z) atomicAdd(&bz[k], b[u].z);
            }
        }
    }
    ev = wave_sum(ev);
    if (lane == 0 && ev) atomicAdd(&P->evals, ev);
}

__global__ __launch_bounds__(BLOCK)
void cloud_brute_emit_kernel(const float4* __restrict__ sorted, int64_t n, Plan* __restrict__ P, unsigned ke, const unsigned* __restrict__ brute,
                             const unsigned long long* __restrict__ bkey, const unsigned* __restrict__ bz,
                             double* __restrict__ out_distance, int64_t* __restrict__ out_neighbor) {
    const unsigned nq = min(P->n_brute, (unsigned)n);
    for (unsigned k = blockIdx.x * BLOCK + threadIdx.x; k < nq; k += gridDim.x * BLOCK) {
        const unsigned t = brute[k];
        if ((int64_t)t >= n) { P->error = 1u; continue; }
        const unsigned long long key = bkey[k];
        const Best b{__uint_as_float((unsigned)(key >> 32)), (unsigned)key, bz[k], 0u};
        emit(b, ke, __float_as_uint(sorted[t].w), n, P, out_distance, out_neighbor);
    }
}

thread_local float g_last_ms = -1.f;
thread_local int64_t g_last_evals = 0, g_last_brute = 0;

Slot g_slot[64];   // csrc/device_call.hpp

int fail(int code, const std::string& msg) {
    set_last_error(msg.c_str());
    return code;
}

}  // namespace cloud
}  // namespace sfmx

using namespace sfmx;
using namespace sfmx::cloud;

extern "C" {

int sfmx_cloud_last_stats(float* kernel_ms, int64_t* evaluations, int64_t* brute_queries) {
    if (kernel_ms) *kernel_ms = g_last_ms;
    if (evaluations) *evaluations = g_last_evals;
    if (brute_queries) *brute_queries = g_last_brute;
    return SFMX_OK;
}

int sfmx_cloud_neighbor_distances(const float* xyz, int64_t n, int32_t max_equal, int32_t inputs_on_device, int32_t device,
                                  void* stream, double* out_distance, int64_t* out_neighbor) {
    if (n < 0) return fail(SFMX_EINVAL, "negative point count");
    if (n > 0 && (!xyz || !out_distance)) return fail(SFMX_EINVAL, "null argument");
    if (n > (int64_t)INT32_MAX - 64) return fail(SFMX_ECAPACITY, "more than 2^31 - 65 points in one call");
    DeviceCall F(stream, !inputs_on_device);
    const hipStream_t st = F.st;
    const int64_t K = 2 + (int64_t)std::max<int32_t>(0, max_equal);
    const unsigned ke = (unsigned)std::min<int64_t>(K, n);
    if (n <= 1 && !inputs_on_device) {   // nothing to search, nothing launched
        if (n == 1) { out_distance[0] = 0.0; if (out_neighbor) out_neighbor[0] = -1; }
        g_last_ms = 0.f;
        g_last_evals = g_last_brute = 0;
        return SFMX_OK;
    }
    const int orc = F.open(g_slot, device);
    if (orc != SFMX_OK) return orc;
    Slot* const S = F.S;
    int rc = SFMX_OK;
    {
        if (n <= 1) {   // device outputs of an empty or one-point cloud
            if (n == 1) {
                SFMX_HIP_CHK(hipMemsetAsync(out_distance, 0, sizeof(double), st));
                if (out_neighbor) SFMX_HIP_CHK(hipMemsetAsync(out_neighbor, 0xff, sizeof(int64_t), st));
                SFMX_HIP_CHK(hipStreamSynchronize(st));
            }
            g_last_ms = 0.f;
            g_last_evals = g_last_brute = 0;
            goto done;
        }
        {
            const bool H = !inputs_on_device;
            // about one cell per point, at most 2^23: the pick kernel keeps the first grid within twice that, the
            // refinement for sheets and clusters within 16 times
            const int64_t cells_target = std::min<int64_t>(std::max<int64_t>(n, 64), (int64_t)1 << 23), cells_limit = 16 * cells_target;
            const int64_t m_scan = cells_limit + 2;   // counts of the grid cells, the non-finite bucket, the end
            const int64_t nb_scan = (m_scan + SCAN_TILE - 1) / SCAN_TILE;
            BlockLayout L;
            Plan* plan;
            unsigned *cnt, *bsum, *rank;
            int* cell;
            float4* sorted;
            unsigned long long* bkey;
            float* xd;
            double* odd;
            int64_t* ond;
            L.want(plan, 1);
            L.want(cnt, m_scan);
            L.want(bsum, nb_scan);
            L.want(cell, n);     // after the scatter: the brute-force list
            L.want(rank, n);     // after the scatter: z of the brute-force queries
            L.want(sorted, n);
            L.want(bkey, n);
            L.want(xd, 3 * n, H);
            L.want(odd, n, H);
            L.want(ond, n, H && out_neighbor);
            rc = F.reserve(L, 256);   // pinned words for the counters
            if (rc != SFMX_OK) goto done;
            const float* px = F.in(xyz, xd, 3 * n);
            SFMX_HIP_CHK(F.err);
            double* pod = F.out(out_distance, odd);
            int64_t* pon = F.out(out_neighbor, ond);
            const unsigned blocks = (unsigned)((n + BLOCK - 1) / BLOCK), stride_blocks = std::min<unsigned>(blocks, 2048u);
            (void)hipEventRecord(S->e0, st);
            SFMX_HIP_CHK(hipMemsetAsync(plan, 0, sizeof(Plan), st));
            SFMX_HIP_CHK(hipMemsetAsync(cnt, 0, sizeof(unsigned) * m_scan, st));
            cloud_minmax_kernel<<<std::min<unsigned>(blocks, 1024u), BLOCK, 0, st>>>(px, n, plan);
            cloud_pick_kernel<<<1, BINS, 0, st>>>(plan, 0, cells_target);
            for (int round = 1; round <= ROUNDS; ++round) {
                cloud_hist_kernel<<<stride_blocks, BLOCK, 0, st>>>(px, n, plan);
                cloud_pick_kernel<<<1, BINS, 0, st>>>(plan, round, cells_target);
            }
            cloud_count_kernel<<<blocks, BLOCK, 0, st>>>(px, n, plan, cnt, cell, rank, 0);
            cloud_scan_reduce_kernel<<<(unsigned)nb_scan, BLOCK, 0, st>>>(cnt, m_scan, bsum, plan, 0);
            cloud_refine_kernel<<<1, 64, 0, st>>>(plan, cells_limit);
            cloud_rezero_kernel<<<(unsigned)std::min<int64_t>(nb_scan * SCAN_PER_THREAD, 2048), BLOCK, 0, st>>>(cnt, m_scan, plan);
            cloud_count_kernel<<<blocks, BLOCK, 0, st>>>(px, n, plan, cnt, cell, rank, 1);
            cloud_scan_reduce_kernel<<<(unsigned)nb_scan, BLOCK, 0, st>>>(cnt, m_scan, bsum, plan, 1);
            cloud_scan_top_kernel<<<1, BLOCK, 0, st>>>(bsum, (int)nb_scan);
            cloud_scan_apply_kernel<<<(unsigned)nb_scan, BLOCK, 0, st>>>(cnt, m_scan, bsum, plan);
            cloud_scatter_kernel<<<blocks, BLOCK, 0, st>>>(px, n, cnt, cell, rank, sorted, plan);
            unsigned* brute = reinterpret_cast<unsigned*>(cell);
            cloud_search_kernel<<<blocks, BLOCK, 0, st>>>(sorted, n, cnt, plan, ke, brute, bkey, rank, pod, pon);
            cloud_brute_kernel<<<2048, BLOCK, 0, st>>>(sorted, n, plan, brute, bkey, rank);
            cloud_brute_emit_kernel<<<std::min<unsigned>(blocks, 1024u), BLOCK, 0, st>>>(sorted, n, plan, ke, brute, bkey, rank, pod, pon);
            (void)hipEventRecord(S->e1, st);
            SFMX_HIP_CHK(hipGetLastError());
            SFMX_HIP_CHK(hipMemcpyAsync(S->pin, plan, offsetof(Plan, lo), hipMemcpyDeviceToHost, st));
            SFMX_HIP_CHK(F.back(out_distance, odd, n));
            if (out_neighbor) SFMX_HIP_CHK(F.back(out_neighbor, ond, n));
            SFMX_HIP_CHK(hipStreamSynchronize(st));
            const Plan* hp = reinterpret_cast<const Plan*>(S->pin);   // only the words before `lo` were copied
            if (hp->error || (int64_t)hp->n_brute > n || (int64_t)hp->n_finite > n) {
                set_last_error("cloud grid self check failed");
                rc = SFMX_EINTERNAL;
                goto done;
            }
            float ms = -1.f;
            (void)hipEventElapsedTime(&ms, S->e0, S->e1);
            g_last_ms = ms;
            g_last_evals = (int64_t)hp->evals;
            g_last_brute = (int64_t)hp->n_brute;
        }
    done:;
        rc = F.finish(rc, "sfmx_cloud_neighbor_distances");
    }
    return rc;
}

// ---- host layer: csrc/cloud_host.hpp behind the C ABI ---------------------------------------------------

int sfmx_cloud_statistics(const double* distances, int64_t n_distances, int64_t n_points, sfmx_cloud_stats* out) {
    if (!out || n_distances < 0 || (n_distances && !distances)) return fail(SFMX_EINVAL, "null argument or negative count");
    try {
        const cloudhost::Stats s = cloudhost::statistics(distances, n_distances, n_points);
        *out = sfmx_cloud_stats{s.n_points, s.max, s.min, s.mean, s.median, s.variance, s.deviation};
    } catch (const std::bad_alloc&) {
        return fail(SFMX_ENOMEM, "host allocation failed");
    }
    return SFMX_OK;
}

int sfmx_cloud_histogram(const double* distances, int64_t n_distances, double resolution, double* out_key, uint64_t* out_count,
                         int64_t cap, int64_t* required) {
    if (!required || n_distances < 0 || cap < 0 || (n_distances && !distances) || (cap && (!out_key || !out_count)))
        return fail(SFMX_EINVAL, "null argument or negative count");
    try {
        std::vector<double> key;
        std::vector<uint64_t> count;
        cloudhost::histogram(distances, n_distances, resolution, key, count);
        *required = (int64_t)key.size();
        if ((int64_t)key.size() > cap) return fail(SFMX_ECAPACITY, "histogram buffers too small");
        if (!key.empty()) {
            std::memcpy(out_key, key.data(), sizeof(double) * key.size());
            std::memcpy(out_count, count.data(), sizeof(uint64_t) * count.size());
        }
    } catch (const std::bad_alloc&) {
        return fail(SFMX_ENOMEM, "host allocation failed");
    }
    return SFMX_OK;
}

int sfmx_ply_read(const char* path, float* xyz, int64_t cap_points, int64_t* n_points, int32_t* face_sizes, int64_t cap_faces,
                  int64_t* n_faces, int32_t* face_indices, int64_t cap_indices, int64_t* n_indices) {
    if (!path || !n_points || !n_faces || !n_indices || cap_points < 0 || cap_faces < 0 || cap_indices < 0)
        return fail(SFMX_EINVAL, "null argument or negative capacity");
    try {
        cloudhost::Ply ply;
        std::string err;
        const bool fill = xyz || face_sizes || face_indices;
        const int rc = cloudhost::read_ply(path, fill, ply, err);
        if (rc != cloudhost::OK) return fail(rc, err);
        *n_points = ply.n_points;
        *n_faces = ply.n_faces;
        *n_indices = ply.n_indices;
        if ((xyz && cap_points < ply.n_points) || (face_sizes && cap_faces < ply.n_faces) ||
            (face_indices && cap_indices < ply.n_indices))
            return fail(SFMX_ECAPACITY, "PLY output buffer too small");
        if (xyz && ply.n_points) std::memcpy(xyz, ply.xyz.data(), sizeof(float) * 3 * (size_t)ply.n_points);
        if (face_sizes && ply.n_faces) std::memcpy(face_sizes, ply.face_sizes.data(), sizeof(int32_t) * (size_t)ply.n_faces);
        if (face_indices && ply.n_indices) std::memcpy(face_indices, ply.face_indices.data(), sizeof(int32_t) * (size_t)ply.n_indices);
    } catch (const std::bad_alloc&) {
        return fail(SFMX_ENOMEM, "host allocation failed");
    }
    return SFMX_OK;
}

int sfmx_cloud_write_stats_csv(const char* path, const sfmx_cloud_stats* s) {
    if (!path || !s) return fail(SFMX_EINVAL, "null argument");
    std::string err;
    const cloudhost::Stats hs{s->n_points, s->max, s->min, s->mean, s->median, s->variance, s->deviation};
    const int rc = cloudhost::write_file(path, cloudhost::stats_csv(hs), err);
    return rc == cloudhost::OK ? SFMX_OK : fail(rc, err);
}

int sfmx_cloud_write_neighbors_csv(const char* path, const double* key, const uint64_t* count, int64_t n) {
    if (!path || n < 0 || (n && (!key || !count))) return fail(SFMX_EINVAL, "null argument or negative count");
    std::string err;
    const int rc = cloudhost::write_file(path, cloudhost::neighbors_csv(key, count, n), err);
    return rc == cloudhost::OK ? SFMX_OK : fail(rc, err);
}

int sfmx_cloud_write_quality_ply(const char* path, const float* xyz, const double* distances, int64_t n_distances,
                                 const int32_t* face_sizes, int64_t n_faces, const int32_t* face_indices, double distance_cutoff) {
    if (!path || n_distances < 0 || n_faces < 0 || (n_distances && (!xyz || !distances)) || (n_faces && !face_sizes))
        return fail(SFMX_EINVAL, "null argument or negative count");
    int64_t total = 0;
    for (int64_t f = 0; f < n_faces; ++f) {
        if (face_sizes[f] < 0) return fail(SFMX_EINVAL, "negative face size");
        total += face_sizes[f];
    }
    if (total && !face_indices) return fail(SFMX_EINVAL, "null face indices");
    try {
        std::string err;
        const int rc = cloudhost::write_file(
            path, cloudhost::quality_ply(xyz, distances, n_distances, face_sizes, n_faces, face_indices, distance_cutoff), err);
        return rc == cloudhost::OK ? SFMX_OK : fail(rc, err);
    } catch (const std::bad_alloc&) {
        return fail(SFMX_ENOMEM, "host allocation failed");
    }
}

}  // extern "C"
