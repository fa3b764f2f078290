// SPDX-License-Identifier: MIT
// sfmx registration pose of a new shot for gfx950 (row f8): SfM::findCameraPoseFrom3d2dMatch
// (sfm/SfM.cpp:453-489) for any number of candidate sets in one call, and ShotMatches3d2d::getDistinct3d2dPoints
// (include/sfmx_pnp.h; DESIGN.md §8i has the algorithm).
//
// Kernels:
//   1. pnp_set_kernel       one 256-thread workgroup per candidate set.  RANSAC runs in rounds of BATCH iterations in
//                           iteration order: thread 0 draws the round's subsets from the cv::RNG stream; lanes
//                           0..BATCH-1 solve one 5-point sample each (undistortPoints + epnp5 of pnp_math.hpp, its
//                           workspace in LDS, element-major); the four waves count the inliers of the round's
//                           models (float reprojection error, ballot + popcount); thread 0 replays the round in
//                           iteration order (strict >, at least 5 inliers, RANSACUpdateNumIters), so the result is
//                           the serial loop's.  Then the mask of the best model, its count and the ratio.  The
//                           set's points stay in global memory (the solver's workspace takes the LDS) and are
//                           rounded to float where they are read.
//   2. pnp_refit_kernel     one workgroup per set, after the first: solvePnP(SOLVEPNP_ITERATIVE) on the inliers.  The
//                           planarity test on the inliers' covariance; the DLT start from the 12 x 12 L^T L (three
//                           passes of 26 sums) or, for a planar set, the RANSAC's EPnP model; CvLevMarq on (rvec,
//                           tvec), every evaluation one pass over the set (cvProjectPoints2 with its Jacobian,
//                           refit_terms of pnp_math.hpp) and one reduction of 28 sums.  Every sum over the set has
//                           the fixed order of tests/pnp_ref.py tree_sum: thread t adds points t, t + 256, ... into
//                           its LDS slot, the slots are folded in halves.  Thread 0 runs the eigen-solver, the 6 x 6
//                           solve and the LM decisions.  sin, cos and acos come from the device's libm.
//   3. distinct_*           mark the records with a match (one thread per cloud point), stable compaction by a
//                           one-block scan, brute-force test of every matched record against the earlier ones,
//                           second scan and gather.
// All arithmetic is pnp_math.hpp's, one correctly rounded IEEE operation per step in the order of tests/pnp_ref.py;
// the file is compiled with -ffp-contract=off; the RANSAC stage calls no libm function but sqrt and the log of
// RANSACUpdateNumIters (as pose.hip), the refit also sin, cos and acos.  No floating-point atomics; every loop is bounded.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/sfmx_pnp.h"
#include "device_call.hpp"
#include "match_common.hpp"
#include "pnp_math.hpp"

namespace sfmx {
namespace pnp {

using pnpm::CamP;
using pnpm::PN_PW;
using pnpm::PN_RES;
using pnpm::PN_UV;
using pnpm::PN_WS;

struct SetP {             // one candidate set: the camera of its shot, the squared threshold as the float compared
    CamP cam;
    float thr2;
    int32_t _pad;
};

constexpr int BLOCK = 256;
constexpr int BATCH = 32;    // RANSAC iterations per round: BATCH * PN_WS doubles of solver workspace in LDS
constexpr int MAX_DRAWS = 10000;
static_assert((size_t)BATCH * PN_WS * sizeof(double) <= 112 * 1024, "solver workspace must leave LDS for the rest");

// cv::RNG::next
__device__ __forceinline__ uint32_t rng_next(unsigned long long& st) {
    st = (unsigned long long)(uint32_t)st * 4164903690ull + (uint32_t)(st >> 32);
    return (uint32_t)st;
}

// RANSACUpdateNumIters, modelPoints = 5
__device__ int update_num_iters(double p, double ep, int max_iters) {
    p = fmax(p, 0.); p = fmin(p, 1.);
    ep = fmax(ep, 0.); ep = fmin(ep, 1.);
    double num = fmax(1. - p, DBL_MIN);
    const double q = 1. - ep, q2 = q * q;
    double denom = 1. - q2 * q2 * q;
    if (denom < DBL_MIN) return 0;
    num = log(num);
    denom = log(denom);
    return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)rint(num / denom);
}

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7FF8000000000000ll); }

// a set without a pose: the status, NaN pose, zero mask and count, ratio -1
__device__ void write_failure(int sidx, int status, int64_t o0, int n, int32_t* __restrict__ out_status,
                              double* __restrict__ out_pose, uint8_t* __restrict__ out_mask, int32_t* __restrict__ out_ni,
                              double* __restrict__ out_ratio) {
    const int tid = threadIdx.x;
    if (tid == 0) { out_status[sidx] = status; out_ni[sidx] = 0; out_ratio[sidx] = -1.0; }
    if (tid < 12) out_pose[12 * (int64_t)sidx + tid] = qnan();
    for (int i = tid; i < n; i += BLOCK) out_mask[o0 + i] = 0;
}

__global__ __launch_bounds__(BLOCK)
void pnp_set_kernel(const SetP* __restrict__ sets, const double* __restrict__ p3, const double* __restrict__ p2,
                    const int64_t* __restrict__ off, int max_iters, double confidence, int32_t* __restrict__ out_status,
                    double* __restrict__ out_pose, uint8_t* __restrict__ out_mask, int32_t* __restrict__ out_ni,
                    double* __restrict__ out_ratio) {
    __shared__ double ws[PN_WS * BATCH];
    __shared__ int sub[BATCH][5];
    __shared__ int nmod[BATCH];
    __shared__ int good[BATCH];
    __shared__ double s_best[12];
    __shared__ int s_cnt[BLOCK / 64];
    __shared__ int s_nb, s_fail_at, s_done, s_niters, s_maxgood, s_it;
    __shared__ unsigned long long s_rng;
    const int sidx = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t o0 = off[sidx];
    const int n = (int)(off[sidx + 1] - o0);
    if (n < 5) {   // fewer than 4: the reference throws; exactly 4: P3P, the host's
        write_failure(sidx, n == 4 ? 2 : 0, o0, n, out_status, out_pose, out_mask, out_ni, out_ratio);
        return;
    }
    const CamP cam = sets[sidx].cam;
    const float thr2 = sets[sidx].thr2;
    const double* X = p3 + 3 * o0;
    const double* x = p2 + 2 * o0;
    if (tid == 0) {
        s_niters = n == 5 ? 1 : max(max_iters, 1);   // 5 points: EPnP on the list itself, nothing is drawn
        s_maxgood = 0; s_it = 0; s_done = 0;
        s_rng = ~0ull;                                // cv::RNG((uint64)-1)
    }
    __syncthreads();
#pragma unroll 1
    for (int round = 0; round < INT_MAX; ++round) {   // (ends by s_done: every round adds at least one iteration)
        if (tid == 0) {   // 1. the next subsets, in iteration order (getSubset, default checkSubset)
            const int want = min(BATCH, s_niters - s_it);
            unsigned long long rng = s_rng;
            int b = 0, fail_at = -1;
            for (; b < want; ++b) {
                int i0 = 0, i1 = 1, i2 = 2, i3 = 3, i4 = 4, cnt = n == 5 ? 5 : 0;
                for (int draws = 0; draws < MAX_DRAWS && cnt < 5; ++draws) {
                    const int v = (int)(rng_next(rng) % (uint32_t)n);
                    if ((cnt > 0 && v == i0) || (cnt > 1 && v == i1) || (cnt > 2 && v == i2) || (cnt > 3 && v == i3)) continue;
                    if (cnt == 0) i0 = v;
                    else if (cnt == 1) i1 = v;
                    else if (cnt == 2) i2 = v;
                    else if (cnt == 3) i3 = v;
                    else i4 = v;
                    ++cnt;
                }
                if (cnt < 5) { fail_at = s_it + b; break; }
                sub[b][0] = i0; sub[b][1] = i1; sub[b][2] = i2; sub[b][3] = i3; sub[b][4] = i4;
            }
            s_rng = rng;
            s_nb = b;
            s_fail_at = fail_at;
        }
        __syncthreads();
        const int nb = s_nb;
        if (tid < nb) {   // 2. one 5-point sample per lane: undistortPoints, then EPnP with the identity camera matrix
            double* w = ws + tid;
#pragma unroll 1
            for (int r = 0; r < 5; ++r) {
                const int i = sub[tid][r];
                w[(PN_PW + 3 * r) * BATCH] = (double)(float)X[3 * i];
                w[(PN_PW + 3 * r + 1) * BATCH] = (double)(float)X[3 * i + 1];
                w[(PN_PW + 3 * r + 2) * BATCH] = (double)(float)X[3 * i + 2];
                float ux, uy;
                pnpm::undistort_f((float)x[2 * i], (float)x[2 * i + 1], cam, ux, uy);
                w[(PN_UV + 2 * r) * BATCH] = (double)ux;
                w[(PN_UV + 2 * r + 1) * BATCH] = (double)uy;
            }
            nmod[tid] = pnpm::epnp5(w, BATCH);
        }
        __syncthreads();
        // 3. inlier counts (computeError + findInliers): wave w takes samples w, w + 4, ... whole
        for (int b = wid; b < nb; b += BLOCK / 64) {
            const int N = nmod[b];
            if (N == 0) continue;
            double P[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) P[e] = ws[(PN_RES + 13 * (N - 1) + e) * BATCH + b];
            int cnt = 0;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = min(i0 + lane, n - 1);
                const float err = pnpm::reprojection_error(P, (float)X[3 * i], (float)X[3 * i + 1], (float)X[3 * i + 2],
                                                           (float)x[2 * i], (float)x[2 * i + 1], cam);
                cnt += __popcll(__ballot(i0 + lane < n && err <= thr2));   // a NaN error is no inlier
            }
            if (lane == 0) good[b] = cnt;
        }
        __syncthreads();
        if (tid == 0) {   // 4. replay in iteration order
            for (int b = 0; b < nb; ++b) {
                if (s_it + b >= s_niters) { s_done = 1; break; }
                const int N = nmod[b];
                if (N == 0) continue;
                const int g = n == 5 ? 5 : good[b];   // 5 points: all five are inliers
                if (g > max(s_maxgood, 4)) {
                    s_maxgood = g;
                    for (int e = 0; e < 12; ++e) s_best[e] = ws[(PN_RES + 13 * (N - 1) + e) * BATCH + b];
                    s_niters = update_num_iters(confidence, (double)(n - g) / n, s_niters);
                }
            }
            s_it += nb;
            if (s_fail_at >= 0) {
                if (s_fail_at == 0) s_maxgood = 0;   // getSubset failed in iteration 0: RANSAC fails
                s_done = 1;
            }
            if (s_it >= s_niters || nb == 0) s_done = 1;
        }
        __syncthreads();
        if (s_done) break;
    }
    if (s_maxgood <= 0) {
        write_failure(sidx, 0, o0, n, out_status, out_pose, out_mask, out_ni, out_ratio);
        return;
    }
    // ---- the mask of the best model, its count, and the ratio of SfM.cpp:479 (index 0 is never counted)
    double P[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) P[e] = s_best[e];
    int cnt = 0;
    for (int i0 = 0; i0 < n; i0 += BLOCK) {
        const int i = i0 + tid;
        const int ic = min(i, n - 1);
        const float err = pnpm::reprojection_error(P, (float)X[3 * ic], (float)X[3 * ic + 1], (float)X[3 * ic + 2],
                                                   (float)x[2 * ic], (float)x[2 * ic + 1], cam);
        const bool inl = i < n && (n == 5 || err <= thr2);
        if (i < n) out_mask[o0 + i] = inl ? 1 : 0;
        cnt += __popcll(__ballot(inl));
    }
    if (lane == 0) s_cnt[wid] = cnt;
    __syncthreads();
    if (tid == 0) {
        const int ni = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        const float e0 = pnpm::reprojection_error(P, (float)X[0], (float)X[1], (float)X[2], (float)x[0], (float)x[1], cam);
        const int m0 = (n == 5 || e0 <= thr2) ? 1 : 0;
        out_status[sidx] = 1;
        out_ni[sidx] = ni;
        out_ratio[sidx] = (double)(ni - m0) / (double)n;
    }
    if (tid < 12) out_pose[12 * (int64_t)sidx + tid] = s_best[tid];
}

// ---- the refit: solvePnP(SOLVEPNP_ITERATIVE) on the inliers of every posed set

constexpr int NSUM = 28;     // sums per reduction: JtJ upper triangle (21), JtErr (6), |err|^2

// red[k][tid] -> red[k][0]: the slots folded in halves, the order of tests/pnp_ref.py tree_sum
__device__ void fold_slots(double (*red)[BLOCK], int nk) {
    const int tid = threadIdx.x;
    __syncthreads();
    for (int s = BLOCK / 2; s >= 1; s >>= 1) {
        if (tid < s)
            for (int k = 0; k < nk; ++k) red[k][tid] = red[k][tid] + red[k][tid + s];
        __syncthreads();
    }
}

// one third (26 entries) of the packed 12 x 12 L^T L of the DLT: both rows of every inlier
template <int G>
__device__ void ltl_pass(double (*red)[BLOCK], const double* X, const double* x, const uint8_t* mk, int n, const CamP& cam) {
    const int tid = threadIdx.x;
    for (int k = 0; k < 26; ++k) red[k][tid] = 0.0;
    for (int i = tid; i < n; i += BLOCK) {
        const bool inl = mk[i] != 0;
        double xn, yn;
        pnpm::undistort_d((float)x[2 * i], (float)x[2 * i + 1], cam, xn, yn);
        const double M0 = (double)(float)X[3 * i], M1 = (double)(float)X[3 * i + 1], M2 = (double)(float)X[3 * i + 2];
        const double r1[12] = {M0, M1, M2, 1.0, 0.0, 0.0, 0.0, 0.0, -xn * M0, -xn * M1, -xn * M2, -xn};
        const double r2[12] = {0.0, 0.0, 0.0, 0.0, M0, M1, M2, 1.0, -yn * M0, -yn * M1, -yn * M2, -yn};
        int idx = 0;
#pragma unroll
        for (int a = 0; a < 12; ++a) {
#pragma unroll
            for (int b = a; b < 12; ++b) {
                if (idx / 26 == G) {
                    const double v = r1[a] * r1[b] + r2[a] * r2[b];
                    red[idx % 26][tid] = red[idx % 26][tid] + (inl ? v : 0.0);
                }
                ++idx;
            }
        }
    }
    fold_slots(red, 26);
}

__global__ __launch_bounds__(BLOCK)
void pnp_refit_kernel(const SetP* __restrict__ sets, const double* __restrict__ p3, const double* __restrict__ p2,
                      const int64_t* __restrict__ off, int32_t* __restrict__ status, double* __restrict__ ransac_pose,
                      uint8_t* __restrict__ mask, int32_t* __restrict__ n_inl, double* __restrict__ ratio,
                      double* __restrict__ out_pose, int32_t* __restrict__ out_start) {
    __shared__ double red[NSUM][BLOCK];
    __shared__ double ws[PN_WS];          // thread 0's eigen-solver and SVD workspace (stride 1)
    __shared__ double sR[9], sdR[27], sPar[6], sPrev[6], sJtJ[36], sJtE[6], sA[42], sX[6], sMc[3];
    __shared__ int s_go, s_fail, s_planar;
    const int sidx = blockIdx.x, tid = threadIdx.x;
    const int64_t o0 = off[sidx];
    const int n = (int)(off[sidx + 1] - o0);
    const int st = status[sidx];
    if (st != 1 || n == 5) {   // no pose: NaN; 5 points: EPnP on the list is the result, no refit
        if (tid < 12) out_pose[12 * (int64_t)sidx + tid] = st == 1 ? ransac_pose[12 * (int64_t)sidx + tid] : qnan();
        if (tid == 0) out_start[sidx] = -1;
        return;
    }
    const CamP cam = sets[sidx].cam;
    const double* X = p3 + 3 * o0;
    const double* x = p2 + 2 * o0;
    const uint8_t* mk = mask + o0;
    const int m = n_inl[sidx];
    // ---- the planarity test of cvFindExtrinsicCameraParams2 on the inliers' covariance
    for (int k = 0; k < 6; ++k) red[k][tid] = 0.0;
    for (int i = tid; i < n; i += BLOCK) {
        const bool inl = mk[i] != 0;
        for (int k = 0; k < 3; ++k) red[k][tid] = red[k][tid] + (inl ? (double)(float)X[3 * i + k] : 0.0);
    }
    fold_slots(red, 3);
    if (tid < 3) sMc[tid] = red[tid][0] / (double)m;
    __syncthreads();
    for (int k = 0; k < 6; ++k) red[k][tid] = 0.0;
    for (int i = tid; i < n; i += BLOCK) {
        const bool inl = mk[i] != 0;
        const double d0 = (double)(float)X[3 * i] - sMc[0], d1 = (double)(float)X[3 * i + 1] - sMc[1], d2 = (double)(float)X[3 * i + 2] - sMc[2];
        red[0][tid] = red[0][tid] + (inl ? d0 * d0 : 0.0);
        red[1][tid] = red[1][tid] + (inl ? d0 * d1 : 0.0);
        red[2][tid] = red[2][tid] + (inl ? d0 * d2 : 0.0);
        red[3][tid] = red[3][tid] + (inl ? d1 * d1 : 0.0);
        red[4][tid] = red[4][tid] + (inl ? d1 * d2 : 0.0);
        red[5][tid] = red[5][tid] + (inl ? d2 * d2 : 0.0);
    }
    fold_slots(red, 6);
    if (tid == 0) {
        for (int k = 0; k < 6; ++k) ws[pnpm::PN_S3 + k] = red[k][0];
        const bool planar = pnpm::planar_cov(ws, 1);
        s_planar = planar ? 1 : 0;
        s_fail = (!planar && m < 6) ? 1 : 0;   // OpenCV's DLT needs 6 points
    }
    __syncthreads();
    const bool planar = s_planar != 0, few = s_fail != 0;
    if (!planar && !few) {   // ---- the DLT start: the eigenvector of L^T L's smallest eigenvalue
        ltl_pass<0>(red, X, x, mk, n, cam);
        if (tid < 26) ws[pnpm::PN_MTM + tid] = red[tid][0];
        __syncthreads();
        ltl_pass<1>(red, X, x, mk, n, cam);
        if (tid < 26) ws[pnpm::PN_MTM + 26 + tid] = red[tid][0];
        __syncthreads();
        ltl_pass<2>(red, X, x, mk, n, cam);
        if (tid < 26) ws[pnpm::PN_MTM + 52 + tid] = red[tid][0];
        __syncthreads();
    }
    if (tid == 0 && !few) {
        bool ok = true;
        double t3[3];
        if (planar) {   // documented deviation: the RANSAC's best EPnP model instead of the homography decomposition
            const double* P = ransac_pose + 12 * (int64_t)sidx;
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) sR[3 * i + j] = P[4 * i + j];
                t3[i] = P[4 * i + 3];
            }
        } else {
            ok = pnpm::dlt_start(ws, 1, sR, t3);
        }
        if (ok) {
            for (int k = 0; k < 9; ++k) ok = ok && pnpm::finite_d(sR[k]);
            for (int k = 0; k < 3; ++k) ok = ok && pnpm::finite_d(t3[k]);
        }
        if (ok) {
            pnpm::rodrigues_inv(sR, sPar);
            sPar[3] = t3[0]; sPar[4] = t3[1]; sPar[5] = t3[2];
        }
        s_fail = ok ? 0 : 1;
    }
    __syncthreads();
    // ---- CvLevMarq on (rvec, tvec): every evaluation is one pass over the set and one fixed-tree reduction
    if (!s_fail) {
        if (tid == 0) s_go = 1;
        int lg = -3, iters = 0, mode = 0;   // thread 0's; mode 0: the sums are J, err at a new centre; 1: err at a trial
        double prev_norm = 0.0;
#pragma unroll 1
        for (int ev = 0; ev < 1024; ++ev) {   // (at most 20 iterations and 20 steps of lambda)
            if (tid == 0) pnpm::rodrigues(sPar[0], sPar[1], sPar[2], sR, sdR);
            for (int k = 0; k < NSUM; ++k) red[k][tid] = 0.0;
            __syncthreads();
            for (int i = tid; i < n; i += BLOCK)
                if (mk[i]) pnpm::refit_terms(sR, sdR, sPar + 3, (double)(float)X[3 * i], (double)(float)X[3 * i + 1], (double)(float)X[3 * i + 2],
                                             (double)(float)x[2 * i], (double)(float)x[2 * i + 1], cam, &red[0][tid], BLOCK);
            fold_slots(red, NSUM);
            if (tid == 0) {
                bool step = false, done = false, fail = false;
                if (mode == 1) {
                    const double norm = sqrt(red[27][0]);
                    bool accept = true;
                    if (norm > prev_norm) {
                        ++lg;
                        if (lg <= 16) { step = true; accept = false; }
                    }
                    if (accept) {
                        lg = max(lg - 1, -16);
                        ++iters;
                        double num = 0.0, den = 0.0;
                        for (int i = 0; i < 6; ++i) { const double d = sPar[i] - sPrev[i]; num = num + d * d; }
                        for (int i = 0; i < 6; ++i) den = den + sPrev[i] * sPrev[i];
                        if (iters >= 20 || sqrt(num) / sqrt(den) < (double)FLT_EPSILON) done = true;
                        prev_norm = norm;
                        mode = 0;   // the same sums are J and err at the new centre
                    }
                }
                if (mode == 0 && !done) {
                    int k = 0;
                    for (int a = 0; a < 6; ++a)
                        for (int b = a; b < 6; ++b) { sJtJ[6 * a + b] = red[k][0]; sJtJ[6 * b + a] = red[k][0]; ++k; }
                    for (int a = 0; a < 6; ++a) { sJtE[a] = red[21 + a][0]; sPrev[a] = sPar[a]; }
                    if (iters == 0) prev_norm = sqrt(red[27][0]);
                    step = true;
                    mode = 1;
                }
                if (step) {
                    const double lam = pnpm::pow10i(lg);
                    for (int a = 0; a < 6; ++a) {
                        for (int b = 0; b < 6; ++b) sA[7 * a + b] = a == b ? sJtJ[6 * a + b] * (1.0 + lam) : sJtJ[6 * a + b];
                        sA[7 * a + 6] = sJtE[a];
                    }
                    if (pnpm::solve6(sA, sX)) for (int i = 0; i < 6; ++i) sPar[i] = sPrev[i] - sX[i];
                    else fail = true;
                }
                if (fail) s_fail = 1;
                if (done || fail) s_go = 0;
            }
            __syncthreads();
            if (!s_go) break;
        }
        if (tid == 0 && !s_fail) {
            pnpm::rodrigues(sPar[0], sPar[1], sPar[2], sR, sdR);
            bool ok = true;
            for (int k = 0; k < 9; ++k) ok = ok && pnpm::finite_d(sR[k]);
            for (int k = 3; k < 6; ++k) ok = ok && pnpm::finite_d(sPar[k]);
            s_fail = ok ? 0 : 1;
        }
        __syncthreads();
    }
    if (s_fail) {   // a failing refit: no pose
        write_failure(sidx, 0, o0, n, status, ransac_pose, mask, n_inl, ratio);
        if (tid < 12) out_pose[12 * (int64_t)sidx + tid] = qnan();
        if (tid == 0) out_start[sidx] = -1;
        return;
    }
    if (tid < 12) out_pose[12 * (int64_t)sidx + tid] = (tid & 3) == 3 ? sPar[3 + (tid >> 2)] : sR[3 * (tid >> 2) + (tid & 3)];
    if (tid == 0) out_start[sidx] = planar ? 1 : 0;
}

// ---- getDistinct3d2dPoints

__global__ __launch_bounds__(BLOCK)
void distinct_mark_kernel(const int64_t* __restrict__ off, int n_points, const int32_t* __restrict__ kp,
                          int32_t* __restrict__ rec_point, uint8_t* __restrict__ flag) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n_points) return;
    for (int64_t r = off[p]; r < off[p + 1]; ++r) {
        rec_point[r] = p;
        flag[r] = kp[r] >= 0 ? 1 : 0;
    }
}

// One block: pos = exclusive scan of the flags (chunks of 1024 with a carry), total last.
__global__ __launch_bounds__(1024)
void distinct_scan_kernel(const uint8_t* __restrict__ flag, int64_t n, int64_t* __restrict__ pos) {
    __shared__ long long s_wave[16];
    __shared__ long long s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + tid;
        const long long v = i < n ? flag[i] : 0;
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
        if (i < n) pos[i] = carry + woff + x - v;
        __syncthreads();
        if (tid == 1023) s_carry = carry + woff + x;
        __syncthreads();
    }
    if (tid == 0) pos[n] = s_carry;
}

// the matched records' five doubles, in record order
__global__ __launch_bounds__(BLOCK)
void distinct_gather_kernel(const double* __restrict__ xyz, const float* __restrict__ fxy, const int32_t* __restrict__ rec_point,
                            const uint8_t* __restrict__ flag, const int64_t* __restrict__ pos, int64_t n_rec,
                            double* __restrict__ c5) {
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n_rec || !flag[r]) return;
    const int64_t i = pos[r];
    const int p = rec_point[r];
    c5[5 * i] = xyz[3 * (int64_t)p]; c5[5 * i + 1] = xyz[3 * (int64_t)p + 1]; c5[5 * i + 2] = xyz[3 * (int64_t)p + 2];
    c5[5 * i + 3] = (double)fxy[2 * r]; c5[5 * i + 4] = (double)fxy[2 * r + 1];   // cv::Point2d(kp.pt)
}

// keep[i] = no earlier matched record has == coordinates in all five doubles (i >= m: 0)
__global__ __launch_bounds__(BLOCK)
void distinct_test_kernel(const double* __restrict__ c5, const int64_t* __restrict__ pos, int64_t n_rec, uint8_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_rec) return;
    const int64_t m = pos[n_rec];
    if (i >= m) { keep[i] = 0; return; }
    const double a = c5[5 * i], b = c5[5 * i + 1], c = c5[5 * i + 2], d = c5[5 * i + 3], e = c5[5 * i + 4];
    bool dup = false;
    for (int64_t j = 0; j < i && !dup; ++j)
        dup = c5[5 * j] == a && c5[5 * j + 1] == b && c5[5 * j + 2] == c && c5[5 * j + 3] == d && c5[5 * j + 4] == e;
    keep[i] = dup ? 0 : 1;
}

__global__ __launch_bounds__(BLOCK)
void distinct_write_kernel(const double* __restrict__ c5, const uint8_t* __restrict__ keep, const int64_t* __restrict__ pos2,
                           int64_t n_rec, double* __restrict__ out_xyz, double* __restrict__ out_xy) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_rec || !keep[i]) return;
    const int64_t o = pos2[i];
    out_xyz[3 * o] = c5[5 * i]; out_xyz[3 * o + 1] = c5[5 * i + 1]; out_xyz[3 * o + 2] = c5[5 * i + 2];
    out_xy[2 * o] = c5[5 * i + 3]; out_xy[2 * o + 1] = c5[5 * i + 4];
}

thread_local float g_last_ms = -1.f;
thread_local float g_distinct_ms = -1.f;

Slot g_slot[64];   // csrc/device_call.hpp

}  // namespace pnp
}  // namespace sfmx

using namespace sfmx;
using namespace sfmx::pnp;

extern "C" {

float sfmx_register_poses_last_kernel_ms(void) { return g_last_ms; }
float sfmx_distinct_3d2d_last_kernel_ms(void) { return g_distinct_ms; }

int sfmx_register_poses(const double* points3d, const double* points2d, const int64_t* set_offsets,
                        const int32_t* set_shot, int32_t n_sets, const sfmx_tri_camera* cameras, int32_t n_cameras,
                        const int32_t* shot_camera, const int32_t* shot_size, int32_t n_shots, double threshold,
                        double confidence, int32_t max_iters, int32_t inputs_on_device, int32_t device, void* stream,
                        int32_t* out_status, double* out_pose, double* out_ransac_pose, uint8_t* out_mask,
                        int32_t* out_n_inliers, double* out_inlier_ratio, int32_t* out_refit_start) {
    if (n_sets < 0 || n_cameras < 0 || n_shots < 0) { set_last_error("negative count"); return SFMX_EINVAL; }
    if (!set_offsets || (n_sets && (!set_shot || !out_status || !out_pose || !out_ransac_pose || !out_n_inliers || !out_inlier_ratio || !out_refit_start)) ||
        (n_shots && (!shot_camera || !shot_size)) || (n_cameras && !cameras)) {
        set_last_error("null argument");
        return SFMX_EINVAL;
    }
    if (!(threshold < 0.0 || threshold > 0.0)) { set_last_error("threshold must be negative (pixels) or positive (fraction)"); return SFMX_EINVAL; }
    if (!(confidence > 0.0 && confidence < 1.0)) { set_last_error("confidence must be in (0, 1)"); return SFMX_EINVAL; }
    if (max_iters < 1) { set_last_error("max_iters must be at least 1"); return SFMX_EINVAL; }
    for (int c = 0; c < n_cameras; ++c)
        if (cameras[c].K[0] == 0.0 || cameras[c].K[4] == 0.0) { set_last_error("camera with zero focal length"); return SFMX_EINVAL; }
    for (int s = 0; s < n_shots; ++s)
        if (shot_camera[s] < 0 || shot_camera[s] >= n_cameras) { set_last_error("shot camera index out of range"); return SFMX_EINVAL; }
    for (int s = 0; s < n_sets; ++s)
        if (set_shot[s] < 0 || set_shot[s] >= n_shots) { set_last_error("set shot index out of range"); return SFMX_EINVAL; }
    DeviceCall F(stream, !inputs_on_device);
    const hipStream_t st = F.st;
    if (inputs_on_device ? n_sets > 0 : set_offsets[n_sets] != 0) {   // anything but an empty call needs the device
        const int orc = F.open(g_slot, device);
        if (orc != SFMX_OK) return orc;
    }
    Slot* const S = F.S;
    int rc = SFMX_OK;
    {
        std::vector<int64_t> hoff(n_sets + 1);
        std::vector<double> nanv;
        int64_t n = 0, longest = 0;
        if (inputs_on_device && n_sets > 0) {
            SFMX_HIP_CHK(hipMemcpyAsync(hoff.data(), set_offsets, sizeof(int64_t) * (n_sets + 1), hipMemcpyDeviceToHost, st));
            SFMX_HIP_CHK(hipStreamSynchronize(st));
        } else if (!inputs_on_device) {
            std::memcpy(hoff.data(), set_offsets, sizeof(int64_t) * (n_sets + 1));
        } else {
            hoff[0] = 0;
        }
        if (hoff[0] != 0) { set_last_error("set offsets do not start at 0"); rc = SFMX_EINVAL; goto done; }
        for (int s = 0; s < n_sets; ++s) {
            if (hoff[s + 1] < hoff[s]) { set_last_error("set offsets not ascending"); rc = SFMX_EINVAL; goto done; }
            longest = std::max(longest, hoff[s + 1] - hoff[s]);
        }
        if (longest > INT32_MAX / 3) { set_last_error("too many points in one set"); rc = SFMX_EINVAL; goto done; }   // 3 * i is an int
        n = hoff[n_sets];
        if (n == 0) {   // no point: nothing is launched; every set has status 0
            const uint64_t qb = 0x7FF8000000000000ull;
            nanv.assign((size_t)12 * n_sets, 0.0);
            for (double& v : nanv) std::memcpy(&v, &qb, 8);
            std::vector<double> neg((size_t)n_sets, -1.0);
            std::vector<int32_t> negi((size_t)n_sets, -1);
            if (inputs_on_device && n_sets) {
                SFMX_HIP_CHK(hipMemsetAsync(out_status, 0, sizeof(int32_t) * n_sets, st));
                SFMX_HIP_CHK(hipMemsetAsync(out_n_inliers, 0, sizeof(int32_t) * n_sets, st));
                SFMX_HIP_CHK(hipMemcpyAsync(out_ransac_pose, nanv.data(), sizeof(double) * 12 * n_sets, hipMemcpyHostToDevice, st));
                SFMX_HIP_CHK(hipMemcpyAsync(out_pose, nanv.data(), sizeof(double) * 12 * n_sets, hipMemcpyHostToDevice, st));
                SFMX_HIP_CHK(hipMemcpyAsync(out_refit_start, negi.data(), sizeof(int32_t) * n_sets, hipMemcpyHostToDevice, st));
                SFMX_HIP_CHK(hipMemcpyAsync(out_inlier_ratio, neg.data(), sizeof(double) * n_sets, hipMemcpyHostToDevice, st));
                SFMX_HIP_CHK(hipStreamSynchronize(st));
            } else if (n_sets) {
                std::memset(out_status, 0, sizeof(int32_t) * n_sets);
                std::memset(out_n_inliers, 0, sizeof(int32_t) * n_sets);
                std::memcpy(out_ransac_pose, nanv.data(), sizeof(double) * 12 * n_sets);
                std::memcpy(out_pose, nanv.data(), sizeof(double) * 12 * n_sets);
                std::memcpy(out_refit_start, negi.data(), sizeof(int32_t) * n_sets);
                std::memcpy(out_inlier_ratio, neg.data(), sizeof(double) * n_sets);
            }
            g_last_ms = 0.f;
            goto done;
        }
        if (!points3d || !points2d || !out_mask) { set_last_error("null argument"); rc = SFMX_EINVAL; goto done; }
        {
            // device block: [set table | (host inputs: points, offsets, every output)]
            const size_t ns = (size_t)n_sets;
            BlockLayout L;
            SetP* std_;
            double *p3d, *p2d, *opd, *ord_, *ofd;
            int64_t* od;
            int32_t *osd, *oid, *obd;
            uint8_t* okd;
            L.want(std_, n_sets);
            L.want(p3d, 3 * n, F.host);
            L.want(p2d, 2 * n, F.host);
            L.want(od, n_sets + 1, F.host);
            L.want(osd, n_sets, F.host);
            L.want(opd, 12 * ns, F.host);
            L.want(okd, n, F.host);
            L.want(oid, n_sets, F.host);
            L.want(ord_, n_sets, F.host);
            L.want(ofd, 12 * ns, F.host);
            L.want(obd, n_sets, F.host);
            rc = F.reserve(L, r256(sizeof(SetP) * n_sets));
            if (rc != SFMX_OK) goto done;
            SetP* hs = F.pinned(std_);
            for (int s = 0; s < n_sets; ++s) {
                const int sh = set_shot[s];
                const sfmx_tri_camera& c = cameras[shot_camera[sh]];
                // SfM.cpp:469-473, then solvePnPRansac's float parameter and the registrator's (float)(thr * thr)
                const double thr = threshold < 0 ? -threshold : (double)std::max(shot_size[2 * sh], shot_size[2 * sh + 1]) * threshold;
                const double tf = (double)(float)thr;
                hs[s].cam = CamP{c.K[0], c.K[4], c.K[2], c.K[5], c.dist[0], c.dist[1], c.dist[2], c.dist[3], c.dist[4]};
                hs[s].thr2 = (float)(tf * tf);
                hs[s]._pad = 0;
            }
            SFMX_HIP_CHK(F.upload(sizeof(SetP) * n_sets));
            const double *d3 = F.in(points3d, p3d, 3 * n), *d2 = F.in(points2d, p2d, 2 * n);
            const int64_t* doff = F.in(set_offsets, od, n_sets + 1);
            SFMX_HIP_CHK(F.err);
            int32_t *dst = F.out(out_status, osd), *dni = F.out(out_n_inliers, oid), *dB = F.out(out_refit_start, obd);
            double *dP = F.out(out_ransac_pose, opd), *dr = F.out(out_inlier_ratio, ord_), *dF = F.out(out_pose, ofd);
            uint8_t* dk = F.out(out_mask, okd);
            (void)hipEventRecord(S->e0, st);
            pnp_set_kernel<<<(unsigned)n_sets, BLOCK, 0, st>>>(std_, d3, d2, doff, max_iters, confidence, dst, dP, dk, dni, dr);
            pnp_refit_kernel<<<(unsigned)n_sets, BLOCK, 0, st>>>(std_, d3, d2, doff, dst, dP, dk, dni, dr, dF, dB);
            (void)hipEventRecord(S->e1, st);
            SFMX_HIP_CHK(hipGetLastError());
            SFMX_HIP_CHK(F.back(out_status, osd, n_sets));
            SFMX_HIP_CHK(F.back(out_ransac_pose, opd, 12 * ns));
            SFMX_HIP_CHK(F.back(out_mask, okd, n));
            SFMX_HIP_CHK(F.back(out_n_inliers, oid, n_sets));
            SFMX_HIP_CHK(F.back(out_inlier_ratio, ord_, n_sets));
            SFMX_HIP_CHK(F.back(out_pose, ofd, 12 * ns));
            SFMX_HIP_CHK(F.back(out_refit_start, obd, n_sets));
            SFMX_HIP_CHK(hipStreamSynchronize(st));   // the pinned set table is reused by the next call
            float ms = -1.f;
            (void)hipEventElapsedTime(&ms, S->e0, S->e1);
            g_last_ms = ms;
        }
    done:;
        rc = F.finish(rc, "sfmx_register_poses");
    }
    return rc;
}

int sfmx_distinct_3d2d_points(const double* cloud_xyz, int32_t n_points, const int64_t* origin_offsets,
                              const int32_t* found_keypoint, const float* found_xy, int32_t inputs_on_device,
                              int32_t device, void* stream, double* out_xyz, double* out_xy, int64_t* out_n) {
    if (n_points < 0) { set_last_error("negative count"); return SFMX_EINVAL; }
    if (!origin_offsets || !out_n) { set_last_error("null argument"); return SFMX_EINVAL; }
    DeviceCall F(stream, !inputs_on_device);
    const hipStream_t st = F.st;
    if (inputs_on_device ? n_points > 0 : origin_offsets[n_points] != 0) {
        const int orc = F.open(g_slot, device);
        if (orc != SFMX_OK) return orc;
    }
    Slot* const S = F.S;
    int rc = SFMX_OK;
    {
        std::vector<int64_t> hoff((size_t)n_points + 1);
        int64_t nr = 0;
        if (inputs_on_device && n_points > 0) {
            SFMX_HIP_CHK(hipMemcpyAsync(hoff.data(), origin_offsets, sizeof(int64_t) * ((size_t)n_points + 1), hipMemcpyDeviceToHost, st));
            SFMX_HIP_CHK(hipStreamSynchronize(st));
        } else if (!inputs_on_device) {
            std::memcpy(hoff.data(), origin_offsets, sizeof(int64_t) * ((size_t)n_points + 1));
        } else {
            hoff[0] = 0;
        }
        if (hoff[0] != 0) { set_last_error("origin offsets do not start at 0"); rc = SFMX_EINVAL; goto done; }
        for (int p = 0; p < n_points; ++p)
            if (hoff[p + 1] < hoff[p]) { set_last_error("origin offsets not ascending"); rc = SFMX_EINVAL; goto done; }
        nr = hoff[n_points];
        *out_n = 0;
        if (nr == 0) { g_distinct_ms = 0.f; goto done; }
        if (!cloud_xyz || !found_keypoint || !found_xy || !out_xyz || !out_xy) { set_last_error("null argument"); rc = SFMX_EINVAL; goto done; }
        {
            // device block: [record -> point | flags | positions | five doubles per matched record | keep | positions
            // | (host inputs: cloud, offsets, found_*, outputs)]
            BlockLayout L;
            int32_t *rp, *fkd;
            uint8_t *fl, *kp;
            int64_t *ps, *ps2, *ofd;
            double *c5, *xyzd, *o3d, *o2d;
            float* fxd;
            L.want(rp, nr);
            L.want(fl, nr);
            L.want(ps, nr + 1);
            L.want(c5, 5 * nr);
            L.want(kp, nr);
            L.want(ps2, nr + 1);
            L.want(xyzd, 3 * (size_t)n_points, F.host);
            L.want(ofd, (size_t)n_points + 1, F.host);
            L.want(fkd, nr, F.host);
            L.want(fxd, 2 * nr, F.host);
            L.want(o3d, 3 * nr, F.host);
            L.want(o2d, 2 * nr, F.host);
            rc = F.reserve(L, 256);
            if (rc != SFMX_OK) goto done;
            const double* dxyz = F.in(cloud_xyz, xyzd, 3 * (size_t)n_points);
            const int64_t* dof = F.in(origin_offsets, ofd, (size_t)n_points + 1);
            const int32_t* dfk = F.in(found_keypoint, fkd, nr);
            const float* dfx = F.in(found_xy, fxd, 2 * nr);
            SFMX_HIP_CHK(F.err);
            double *do3 = F.out(out_xyz, o3d), *do2 = F.out(out_xy, o2d);
            const unsigned gp = (unsigned)((n_points + BLOCK - 1) / BLOCK), gr = (unsigned)((nr + BLOCK - 1) / BLOCK);
            (void)hipEventRecord(S->e0, st);
            distinct_mark_kernel<<<gp, BLOCK, 0, st>>>(dof, n_points, dfk, rp, fl);
            distinct_scan_kernel<<<1, 1024, 0, st>>>(fl, nr, ps);
            distinct_gather_kernel<<<gr, BLOCK, 0, st>>>(dxyz, dfx, rp, fl, ps, nr, c5);
            distinct_test_kernel<<<gr, BLOCK, 0, st>>>(c5, ps, nr, kp);
            distinct_scan_kernel<<<1, 1024, 0, st>>>(kp, nr, ps2);
            distinct_write_kernel<<<gr, BLOCK, 0, st>>>(c5, kp, ps2, nr, do3, do2);
            (void)hipEventRecord(S->e1, st);
            SFMX_HIP_CHK(hipGetLastError());
            int64_t* htot = reinterpret_cast<int64_t*>(S->pin);
            SFMX_HIP_CHK(hipMemcpyAsync(htot, ps2 + nr, sizeof(int64_t), hipMemcpyDeviceToHost, st));
            SFMX_HIP_CHK(hipStreamSynchronize(st));
            const int64_t total = *htot;
            if (total < 0 || total > nr) { set_last_error("distinct count self check failed"); rc = SFMX_EINTERNAL; goto done; }
            if (F.host && total) {
                SFMX_HIP_CHK(F.back(out_xyz, o3d, 3 * total));
                SFMX_HIP_CHK(F.back(out_xy, o2d, 2 * total));
                SFMX_HIP_CHK(hipStreamSynchronize(st));
            }
            *out_n = total;
            float ms = -1.f;
            (void)hipEventElapsedTime(&ms, S->e0, S->e1);
            g_distinct_ms = ms;
        }
    done:;
        rc = F.finish(rc, "sfmx_distinct_3d2d_points");
    }
    return rc;
}

}  // extern "C"
