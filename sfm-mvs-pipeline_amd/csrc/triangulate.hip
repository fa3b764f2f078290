// SPDX-License-Identifier: MIT
// sfmx triangulation of shot matches for gfx950: SfM::triangulateMatch (sfm/SfM.cpp:383-451) for every
// pair of a match graph in one call (include/sfmx_triangulate.h; DESIGN.md has the algorithm).
//
// Three kernels over the packed match list, one thread per match, all pairs in one launch:
//   1. tri_solve_kernel    undistortPoints -> the 4x4 DLT system -> its null vector by the one-sided Jacobi
//                          of OpenCV's JacobiSVDImpl_ -> convertPointsFromHomogeneous -> projectPoints into
//                          both views -> reprojection errors and the keep flag.  Writes float X, Y, Z and
//                          the two keypoints of kept matches, one keep mask per wave, one count per block.
//   2. tri_scan_kernel     exclusive scan of the block counts (one block, looped, any number of blocks) and
//                          the point offsets at the pair boundaries.
//   3. tri_compact_kernel  stable compaction by mask popcount prefix into the caller's arrays.
// All arithmetic is fp64 (float where OpenCV's arrays are float), one correctly rounded IEEE operation per
// step in the order of tests/tri_ref.py; the file is compiled with -ffp-contract=off and calls no libm
// function but sqrt.  At, V and W of the Jacobi live in registers: every loop over them is fully unrolled
// and the row sort is compare / select, so nothing is indexed dynamically (no scratch).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/sfmx_triangulate.h"
#include "device_call.hpp"
#include "match_common.hpp"
#include "project_device.hpp"

namespace sfmx {
namespace tri {

struct ShotT {            // one shot: its pose, its camera, its keypoints
    double P[12];         // 3x4 [R|t] row-major
    double fx, fy, cx, cy, ifx, ify, k1, k2, p1, p2, k3;
    const float2* kp;
    int32_t nkp, _pad;
};

constexpr int BLOCK = 256;
constexpr int MAX_SWEEPS = 30;

// largest p in [lo, hi] with off[p] <= g: the pair whose list holds match g (empty pairs are passed over)
__device__ __forceinline__ int search_pair(int64_t g, const int64_t* __restrict__ off, int lo, int hi) {
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The pair of match g (g < n).  One search per wave for its first match; `uniform` tells whether the whole
// wave lies inside that pair, else every lane searches on from there.
__device__ __forceinline__ int pair_of(int64_t g, int64_t n, const int64_t* __restrict__ off, int n_pairs, bool& uniform) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t g0 = min((int64_t)blockIdx.x * BLOCK + wave * 64, n - 1);
    const int p0 = search_pair(g0, off, 0, n_pairs - 1);
    uniform = min(g0 + 63, n - 1) < off[p0 + 1];
    return uniform ? p0 : search_pair(g, off, p0, n_pairs - 1);
}

// cv::undistortPoints, TermCriteria(COUNT, 5); the result is rounded to float
__device__ __forceinline__ void undistort(const float2 pt, const ShotT* __restrict__ S, float& ox, float& oy) {
    const double k1 = S->k1, k2 = S->k2, p1 = S->p1, p2 = S->p2, k3 = S->k3;
    double x = ((double)pt.x - S->cx) * S->ifx;
    double y = ((double)pt.y - S->cy) * S->ify;
    const double x0 = x, y0 = y;
#pragma unroll 1
    for (int it = 0; it < 5; ++it) {
        const double r2 = x * x + y * y;
        const double icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
        if (icdist < 0) { x = x0; y = y0; break; }
        const double dX = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
        const double dY = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
        x = (x0 - dX) * icdist;
        y = (y0 - dY) * icdist;
    }
    ox = (float)x;
    oy = (float)y;
}

// two rows of the DLT system of one view, stored transposed: At[k][row] = A[row][k]
__device__ __forceinline__ void dlt_rows(const ShotT* __restrict__ S, float xf, float yf, int row, double (&At)[4][4]) {
    const double x = (double)xf, y = (double)yf;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double p0 = S->P[k], p1 = S->P[4 + k], p2 = S->P[8 + k];
        if (row == 0) { At[k][0] = x * p2 - p0; At[k][1] = y * p2 - p1; }
        else          { At[k][2] = x * p2 - p0; At[k][3] = y * p2 - p1; }
    }
}

__device__ __forceinline__ double sum4(double a, double b, double c, double d) { return ((a + b) + c) + d; }

// one Jacobi rotation of rows I, J (JacobiSVDImpl_); false when the pair is already orthogonal
template <int I, int J>
__device__ __forceinline__ bool rotate(double (&At)[4][4], double (&V)[4][4], double (&W)[4]) {
    const double eps = 10.0 * 2.220446049250313e-16;   // 10 * DBL_EPSILON
    double p = sum4(At[I][0] * At[J][0], At[I][1] * At[J][1], At[I][2] * At[J][2], At[I][3] * At[J][3]);
    if (fabs(p) <= eps * sqrt(W[I] * W[J])) return false;
    p = 2.0 * p;
    const double beta = W[I] - W[J];
    const double gamma = sqrt(p * p + beta * beta);   // OpenCV: hypot(p, beta)
    double c, s;
    if (beta < 0) {
        s = sqrt(((gamma - beta) * 0.5) / gamma);
        c = p / (gamma * s * 2.0);
    } else {
        c = sqrt((gamma + beta) / (gamma * 2.0));
        s = p / (gamma * c * 2.0);
    }
    double t0[4], t1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        t0[k] = c * At[I][k] + s * At[J][k];
        t1[k] = c * At[J][k] - s * At[I][k];
        At[I][k] = t0[k];
        At[J][k] = t1[k];
    }
    W[I] = sum4(t0[0] * t0[0], t0[1] * t0[1], t0[2] * t0[2], t0[3] * t0[3]);
    W[J] = sum4(t1[0] * t1[0], t1[1] * t1[1], t1[2] * t1[2], t1[3] * t1[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double v0 = c * V[I][k] + s * V[J][k];
        const double v1 = c * V[J][k] - s * V[I][k];
        V[I][k] = v0;
        V[J][k] = v1;
    }
    return true;
}

// the right singular vector of the smallest singular value: row 3 of V after the descending sort, as float
__device__ __forceinline__ void jacobi_null(double (&At)[4][4], float (&h)[4]) {
    double V[4][4], W[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) V[i][k] = i == k ? 1.0 : 0.0;
        W[i] = sum4(At[i][0] * At[i][0], At[i][1] * At[i][1], At[i][2] * At[i][2], At[i][3] * At[i][3]);
    }
#pragma unroll 1
    for (int sweep = 0; sweep < MAX_SWEEPS; ++sweep) {
        bool changed = rotate<0, 1>(At, V, W);
        changed |= rotate<0, 2>(At, V, W);
        changed |= rotate<0, 3>(At, V, W);
        changed |= rotate<1, 2>(At, V, W);
        changed |= rotate<1, 3>(At, V, W);
        changed |= rotate<2, 3>(At, V, W);
        if (!changed) break;
    }
    int idx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        W[i] = sqrt(sum4(At[i][0] * At[i][0], At[i][1] * At[i][1], At[i][2] * At[i][2], At[i][3] * At[i][3]));
        idx[i] = i;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {   // selection sort, descending; the rows follow through idx
        int j = i;
        double wj = W[i];
#pragma unroll
        for (int k = i + 1; k < 4; ++k) {
            const bool lt = wj < W[k];
            j = lt ? k : j;
            wj = lt ? W[k] : wj;
        }
#pragma unroll
        for (int m = i + 1; m < 4; ++m) {
            const bool sw = j == m;
            const double wi = W[i], wm = W[m];
            const int ii = idx[i], im = idx[m];
            W[i] = sw ? wm : wi;
            W[m] = sw ? wi : wm;
            idx[i] = sw ? im : ii;
            idx[m] = sw ? ii : im;
        }
    }
    const int r = idx[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k] = (float)(r == 0 ? V[0][k] : (r == 1 ? V[1][k] : (r == 2 ? V[2][k] : V[3][k])));
}

// cv::projectPoints with R, t of the pose (project_device.hpp), then the reprojection error against the keypoint
__device__ __forceinline__ double reproject_error(const ShotT* __restrict__ S, float Xf, float Yf, float Zf, const float2 pt) {
    float u, v;
    project_point(S, Xf, Yf, Zf, u, v);
    const float du = u - pt.x, dv = v - pt.y;
    const double e = sqrt((double)du * (double)du + (double)dv * (double)dv);
    return canon(e);
}

// steps a and b up to the DLT system (transposed)
__device__ __forceinline__ void build_system(const ShotT* __restrict__ SL, const ShotT* __restrict__ SR, const float2 l,
                                             const float2 r, double (&At)[4][4]) {
    float xl, yl, xr, yr;
    undistort(l, SL, xl, yl);
    undistort(r, SR, xr, yr);
    dlt_rows(SL, xl, yl, 0, At);
    dlt_rows(SR, xr, yr, 1, At);
}

__global__ __launch_bounds__(BLOCK)
void tri_solve_kernel(const ShotT* __restrict__ shots, const int32_t* __restrict__ pairs, int n_pairs,
                      const DMatchDev* __restrict__ matches, const int64_t* __restrict__ off, int64_t n, double max_err,
                      float4* __restrict__ sxyz, float4* __restrict__ slr, unsigned long long* __restrict__ keepmask,
                      int32_t* __restrict__ block_count, double* __restrict__ out_err, int64_t* __restrict__ res) {
    __shared__ int s_cnt[BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t g = (int64_t)blockIdx.x * BLOCK + tid;
    const bool in = g < n;
    const int64_t gc = in ? g : n - 1;
    bool uniform;
    const int p = pair_of(gc, n, off, n_pairs, uniform);
    // The two table rows of the pair: every lane of a wave inside one pair reads the same addresses, which the
    // vector memory path serves as one broadcast cache line per load (duplicating the body behind wave-uniform
    // pointers does not survive the compiler: it merges the two copies back into one with a selected pointer).
    const ShotT* SL = shots + pairs[2 * p];
    const ShotT* SR = shots + pairs[2 * p + 1];
    const DMatchDev d = matches[gc];
    const bool valid = in && d.queryIdx >= 0 && d.queryIdx < SL->nkp && d.trainIdx >= 0 && d.trainIdx < SR->nkp;
    if (in && !valid) res[1] = 1;   // a match index outside its image's keypoints: the call fails
    bool keep = false;
    if (valid) {
        const float2 l = SL->kp[d.queryIdx], r = SR->kp[d.trainIdx];
        double At[4][4];
        build_system(SL, SR, l, r, At);
        float h[4];
        jacobi_null(At, h);
        const float scale = h[3] != 0.f ? 1.f / h[3] : 1.f;   // convertPointsFromHomogeneous, in float
        const float X = h[0] * scale, Y = h[1] * scale, Z = h[2] * scale;
        // the poses and cameras are read again here, not held in ~90 registers across the Jacobi sweeps
        // (116 instead of 192 VGPRs): the empty asm keeps the compiler from merging the two reads
        const ShotT *PL = SL, *PR = SR;
        asm volatile("" : "+v"(PL), "+v"(PR));
        const double eL = reproject_error(PL, X, Y, Z, l);
        const double eR = reproject_error(PR, X, Y, Z, r);
        keep = !(eL > max_err || eR > max_err);   // a NaN error keeps the point (SfM.cpp:434)
        if (out_err) {
            out_err[2 * g] = eL;
            out_err[2 * g + 1] = eR;
        }
        if (keep) {
            sxyz[g] = make_float4(canon(X), canon(Y), canon(Z), 0.f);
            slr[g] = make_float4(l.x, l.y, r.x, r.y);
        }
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) {
        keepmask[g >> 6] = mask;
        s_cnt[wave] = __popcll(mask);
    }
    __syncthreads();
    if (tid == 0) block_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// One block: block_off = exclusive scan of block_count (chunks of 1024 with a carry), then the number of
// points before every pair boundary and the total.
__global__ __launch_bounds__(1024)
void tri_scan_kernel(const int32_t* __restrict__ block_count, int64_t n_blocks, int64_t* __restrict__ block_off,
                     const unsigned long long* __restrict__ keepmask, const int64_t* __restrict__ off, int n_pairs,
                     int64_t n, int64_t* __restrict__ out_point_offsets, int64_t* __restrict__ res) {
    __shared__ long long s_wave[16];
    __shared__ long long s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < n_blocks; base += 1024) {
        const int64_t i = base + tid;
        const long long v = i < n_blocks ? block_count[i] : 0;
        long long x = v;
#pragma unroll
        for (int dlt = 1; dlt < 64; dlt <<= 1) {
            const long long t = __shfl_up(x, dlt);
            if (lane >= dlt) x += t;
        }
        if (lane == 63) s_wave[wave] = x;
        __syncthreads();
        long long woff = 0;
        for (int w = 0; w < wave; ++w) woff += s_wave[w];
        const long long carry = s_carry;
        if (i < n_blocks) block_off[i] = carry + woff + x - v;
        __syncthreads();
        if (tid == 1023) s_carry = carry + woff + x;
        __syncthreads();
    }
    const long long total = s_carry;
    for (int p = tid; p <= n_pairs; p += 1024) {
        const int64_t g = min(max(off[p], (int64_t)0), n);
        long long v = total;
        if (g < n) {
            const int64_t blk = g >> 8, wq = g >> 6;
            v = block_off[blk];
            for (int64_t w = blk * 4; w < wq; ++w) v += __popcll(keepmask[w]);
            v += __popcll(keepmask[wq] & ((1ull << (g & 63)) - 1ull));
        }
        out_point_offsets[p] = v;
    }
    if (tid == 0) res[0] = total;
}

__global__ __launch_bounds__(BLOCK)
void tri_compact_kernel(const int32_t* __restrict__ pairs, int n_pairs, const int64_t* __restrict__ off, int64_t n,
                        const float4* __restrict__ sxyz, const float4* __restrict__ slr,
                        const unsigned long long* __restrict__ keepmask, const int64_t* __restrict__ block_off,
                        double* __restrict__ out_xyz, int64_t* __restrict__ out_match,
                        int32_t* __restrict__ out_origin_shot, double* __restrict__ out_origin_xy) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t g = (int64_t)blockIdx.x * BLOCK + tid;
    const int64_t gc = g < n ? g : n - 1;
    bool uniform;
    const int p = pair_of(gc, n, off, n_pairs, uniform);
    if (g >= n) return;
    const unsigned long long mask = keepmask[g >> 6];
    if (!((mask >> lane) & 1ull)) return;
    int64_t pos = block_off[blockIdx.x];
    for (int w = 0; w < wave; ++w) pos += __popcll(keepmask[(int64_t)blockIdx.x * 4 + w]);
    pos += __popcll(mask & ((1ull << lane) - 1ull));
    const float4 a = sxyz[g], b = slr[g];
    out_xyz[3 * pos] = (double)a.x;
    out_xyz[3 * pos + 1] = (double)a.y;
    out_xyz[3 * pos + 2] = (double)a.z;
    out_match[pos] = g;
    out_origin_shot[2 * pos] = pairs[2 * p];
    out_origin_shot[2 * pos + 1] = pairs[2 * p + 1];
    out_origin_xy[4 * pos] = (double)b.x;
    out_origin_xy[4 * pos + 1] = (double)b.y;
    out_origin_xy[4 * pos + 2] = (double)b.z;
    out_origin_xy[4 * pos + 3] = (double)b.w;
}

thread_local float g_last_ms = -1.f;

Slot g_slot[64];   // csrc/device_call.hpp

}  // namespace tri
}  // namespace sfmx

using namespace sfmx;
using namespace sfmx::tri;

extern "C" {

float sfmx_triangulate_last_kernel_ms(void) { return g_last_ms; }

int sfmx_triangulate_matches(const sfmx_point2f* const* keypoints, const int32_t* n_keypoints, int32_t n_shots,
                             const sfmx_tri_camera* cameras, int32_t n_cameras, const int32_t* shot_camera,
                             const double* shot_pose, const int32_t* pairs, int32_t n_pairs,
                             const sfmx_dmatch* matches, const int64_t* pair_offsets, double max_reprojection_error,
                             int32_t inputs_on_device, int32_t device, void* stream, int64_t* out_point_offsets,
                             double* out_xyz, int64_t* out_match, int32_t* out_origin_shot, double* out_origin_xy,
                             double* out_err, int64_t* out_n_points) {
    if (n_shots < 0 || n_cameras < 0 || n_pairs < 0) { set_last_error("negative count"); return SFMX_EINVAL; }
    if (!out_n_points || !out_point_offsets || !pair_offsets || (n_pairs && !pairs) ||
        (n_shots && (!keypoints || !n_keypoints || !shot_camera || !shot_pose)) || (n_cameras && !cameras)) {
        set_last_error("null argument");
        return SFMX_EINVAL;
    }
    *out_n_points = 0;
    for (int c = 0; c < n_cameras; ++c)
        if (cameras[c].K[0] == 0.0 || cameras[c].K[4] == 0.0) { set_last_error("camera with zero focal length"); return SFMX_EINVAL; }
    for (int s = 0; s < n_shots; ++s) {
        if (shot_camera[s] < 0 || shot_camera[s] >= n_cameras) { set_last_error("shot camera index out of range"); return SFMX_EINVAL; }
        if (n_keypoints[s] < 0) { set_last_error("negative keypoint count"); return SFMX_EINVAL; }
    }
    for (int p = 0; p < n_pairs; ++p)
        if (pairs[2 * p] < 0 || pairs[2 * p] >= n_shots || pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= n_shots) {
            set_last_error("pair shot index out of range");
            return SFMX_EINVAL;
        }
    DeviceCall F(stream, !inputs_on_device);
    const hipStream_t st = F.st;
    if (inputs_on_device || pair_offsets[n_pairs] != 0) {   // anything but an empty host call needs the device
        const int orc = F.open(g_slot, device);
        if (orc != SFMX_OK) return orc;
    }
    Slot* const S = F.S;
    int rc = SFMX_OK;
    {
        // the pair offsets on the host: they size the launch
        std::vector<int64_t> hoff(n_pairs + 1);
        int64_t n = 0, n_blocks = 0, nk = 0;
        if (inputs_on_device) {
            SFMX_HIP_CHK(hipMemcpyAsync(hoff.data(), pair_offsets, sizeof(int64_t) * (n_pairs + 1), hipMemcpyDeviceToHost, st));
            SFMX_HIP_CHK(hipStreamSynchronize(st));
        } else {
            std::memcpy(hoff.data(), pair_offsets, sizeof(int64_t) * (n_pairs + 1));
        }
        if (hoff[0] != 0) { set_last_error("pair offsets do not start at 0"); rc = SFMX_EINVAL; goto done; }
        for (int p = 0; p < n_pairs; ++p)
            if (hoff[p + 1] < hoff[p]) { set_last_error("pair offsets not ascending"); rc = SFMX_EINVAL; goto done; }
        n = hoff[n_pairs];
        if (n == 0) {   // no match: nothing is launched
            if (inputs_on_device) {
                SFMX_HIP_CHK(hipMemsetAsync(out_point_offsets, 0, sizeof(int64_t) * (n_pairs + 1), st));
                SFMX_HIP_CHK(hipStreamSynchronize(st));
            } else {
                std::memset(out_point_offsets, 0, sizeof(int64_t) * (n_pairs + 1));
            }
            g_last_ms = 0.f;
            goto done;
        }
        if (!matches || !out_xyz || !out_match || !out_origin_shot || !out_origin_xy) {
            set_last_error("null argument");
            rc = SFMX_EINVAL;
            goto done;
        }
        n_blocks = (n + BLOCK - 1) / BLOCK;
        if (n_blocks > INT32_MAX) { set_last_error("too many matches"); rc = SFMX_EINVAL; goto done; }
        if (!inputs_on_device) {
            for (int p = 0; p < n_pairs; ++p) {
                const int L = pairs[2 * p], R = pairs[2 * p + 1];
                for (int64_t i = hoff[p]; i < hoff[p + 1]; ++i)
                    if (matches[i].queryIdx < 0 || matches[i].queryIdx >= n_keypoints[L] || matches[i].trainIdx < 0 ||
                        matches[i].trainIdx >= n_keypoints[R]) {
                        set_last_error("match index outside its image's keypoints");
                        rc = SFMX_EINVAL;
                        goto done;
                    }
            }
            for (int i = 0; i < n_shots; ++i) nk += n_keypoints[i];
        }
        {
            // device block: [shot table | pairs | result words | block counts | block offsets | keep masks |
            // xyz scratch | keypoint scratch | (host inputs: keypoints, matches, offsets, every output)]
            const bool H = F.host;
            BlockLayout L;
            ShotT* shd;
            int32_t *prd, *bcd, *osd;
            int64_t *resd, *bod, *od, *pod, *omd;
            unsigned long long* kmd;
            float4 *s1, *s2;
            float2* kd;
            sfmx_dmatch* md;
            double *oxd, *oyd, *oed;
            L.want(shd, n_shots);
            L.want(prd, 2 * (size_t)n_pairs);
            L.want(resd, 2);
            const size_t b_tab = L.need;   // up to here: staged in pinned memory, one upload
            L.want(bcd, n_blocks);
            L.want(bod, n_blocks);
            L.want(kmd, n_blocks * (BLOCK / 64));
            L.want(s1, n);
            L.want(s2, n);
            L.want(kd, nk, H);
            L.want(md, n, H);
            L.want(od, n_pairs + 1, H);
            L.want(pod, n_pairs + 1, H);
            L.want(oxd, 3 * n, H);
            L.want(omd, n, H);
            L.want(osd, 2 * n, H);
            L.want(oyd, 4 * n, H);
            L.want(oed, 2 * n, H && out_err);
            rc = F.reserve(L, b_tab);
            if (rc != SFMX_OK) goto done;
            // shot table: pose, camera and keypoint pointer of every shot
            ShotT* hs = F.pinned(shd);
            int64_t o = 0;
            for (int i = 0; i < n_shots; ++i) {
                const sfmx_tri_camera& c = cameras[shot_camera[i]];
                ShotT& t = hs[i];
                std::memcpy(t.P, shot_pose + 12 * i, sizeof(double) * 12);
                t.fx = c.K[0]; t.fy = c.K[4]; t.cx = c.K[2]; t.cy = c.K[5];
                t.ifx = 1.0 / c.K[0]; t.ify = 1.0 / c.K[4];
                t.k1 = c.dist[0]; t.k2 = c.dist[1]; t.p1 = c.dist[2]; t.p2 = c.dist[3]; t.k3 = c.dist[4];
                t.nkp = n_keypoints[i];
                t._pad = 0;
                if (H) {
                    if (n_keypoints[i]) SFMX_HIP_CHK(hipMemcpyAsync(kd + o, keypoints[i], sizeof(float2) * n_keypoints[i], hipMemcpyHostToDevice, st));
                    t.kp = kd + o;
                    o += n_keypoints[i];
                } else {
                    t.kp = reinterpret_cast<const float2*>(keypoints[i]);
                }
            }
            std::memcpy(F.pinned(prd), pairs, sizeof(int32_t) * 2 * n_pairs);
            int64_t* hres = F.pinned(resd);
            hres[0] = hres[1] = 0;
            SFMX_HIP_CHK(F.upload(b_tab));   // tables, result words = 0
            const DMatchDev* dm = reinterpret_cast<const DMatchDev*>(F.in(matches, md, n));
            const int64_t* doff = F.in(pair_offsets, od, n_pairs + 1);
            SFMX_HIP_CHK(F.err);
            int64_t *dpo = F.out(out_point_offsets, pod), *dom = F.out(out_match, omd);
            double *dox = F.out(out_xyz, oxd), *doy = F.out(out_origin_xy, oyd), *doe = F.out(out_err, oed);
            int32_t* dos = F.out(out_origin_shot, osd);
            (void)hipEventRecord(S->e0, st);
            tri_solve_kernel<<<(unsigned)n_blocks, BLOCK, 0, st>>>(shd, prd, n_pairs, dm, doff, n, max_reprojection_error, s1, s2,
                                                                   kmd, bcd, doe, resd);
            tri_scan_kernel<<<1, 1024, 0, st>>>(bcd, n_blocks, bod, kmd, doff, n_pairs, n, dpo, resd);
            tri_compact_kernel<<<(unsigned)n_blocks, BLOCK, 0, st>>>(prd, n_pairs, doff, n, s1, s2, kmd, bod, dox, dom, dos, doy);
            (void)hipEventRecord(S->e1, st);
            SFMX_HIP_CHK(hipGetLastError());
            SFMX_HIP_CHK(hipMemcpyAsync(hres, resd, sizeof(int64_t) * 2, hipMemcpyDeviceToHost, st));   // total and the index flag
            SFMX_HIP_CHK(hipStreamSynchronize(st));
            if (hres[1] != 0) { set_last_error("match index outside its image's keypoints"); rc = SFMX_EINVAL; goto done; }
            const int64_t total = hres[0];
            if (total < 0 || total > n) { set_last_error("point count self check failed"); rc = SFMX_EINTERNAL; goto done; }
            SFMX_HIP_CHK(F.back(out_point_offsets, pod, n_pairs + 1));
            if (total) {
                SFMX_HIP_CHK(F.back(out_xyz, oxd, 3 * total));
                SFMX_HIP_CHK(F.back(out_match, omd, total));
                SFMX_HIP_CHK(F.back(out_origin_shot, osd, 2 * total));
                SFMX_HIP_CHK(F.back(out_origin_xy, oyd, 4 * total));
            }
            if (out_err) SFMX_HIP_CHK(F.back(out_err, oed, 2 * n));
            if (H) SFMX_HIP_CHK(hipStreamSynchronize(st));
            *out_n_points = total;
            float ms = -1.f;
            (void)hipEventElapsedTime(&ms, S->e0, S->e1);
            g_last_ms = ms;
        }
    done:;
        rc = F.finish(rc, "sfmx_triangulate_matches");
    }
    return rc;
}

}  // extern "C"
