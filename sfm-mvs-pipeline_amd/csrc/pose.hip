// SPDX-License-Identifier: MIT
// sfmx relative pose of shot matches for gfx950 (row f7): SfM::findCameraPoseFromMatch (sfm/SfM.cpp:491-540) for
// every pair of a match graph in one call (include/sfmx_pose.h; DESIGN.md §8h has the algorithm).
//
// Three kernels:
//   1. pose_pair_kernel     one 256-thread workgroup per pair.  The correspondences are prepared once
//                           (undistortPoints per side, the mean camera matrix) into LDS, lists over CAP into a
//                           global scratch.  RANSAC runs in batches of BATCH iterations in iteration order:
//                           thread 0 draws the batch's subsets from the cv::RNG stream; lanes 0..BATCH-1 solve one
//                           minimal sample each (five_point of pose_math.hpp, its workspace in LDS, element-major);
//                           the four waves count the inliers of the batch's models (Sampson error, ballot +
//                           popcount); thread 0 replays the batch in iteration order and root order (strict >, at
//                           least 5 inliers, RANSACUpdateNumIters), so the result is the serial loop's.  Then
//                           recoverPose: thread 0 decomposes the best E into the four candidates, every thread
//                           takes the pair's matches 256 at a time (the four DLT triangulations and cheirality
//                           tests of an inlier), the four counts come by popcount and the >= cascade picks the
//                           winner, whose mask, pose and counts are written.
//   2. pose_scan_kernel     exclusive scan of the pairs' inlier counts: the output offsets.
//   3. pose_compact_kernel  one workgroup per pair: stable compaction of the DMatches by mask popcount prefix.
// All arithmetic is pose_math.hpp's, one correctly rounded IEEE operation per step in the order of
// tests/pose_ref.py; the file is compiled with -ffp-contract=off and calls no libm function but sqrt and the log
// of RANSACUpdateNumIters (as homography.hip).  No floating-point atomics; every loop is bounded.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/sfmx_pose.h"
#include "device_call.hpp"
#include "match_common.hpp"
#include "pose_math.hpp"

namespace sfmx {
namespace pose {

using posem::CamP;
using posem::PM_MODELS;
using posem::PM_WS;

struct ShotP {            // one shot: its camera, its keypoints
    CamP cam;
    const float2* kp;
    int32_t nkp, _pad;
};
struct PairP {
    int32_t left, right;
    double thr;           // the threshold in pixels (SfM.cpp:515-521)
};

constexpr int BLOCK = 256;
constexpr int CAP = 1024;    // correspondences kept in LDS (larger lists use the global scratch)
constexpr int BATCH = 32;    // RANSAC iterations per round: BATCH * PM_WS doubles of solver workspace in LDS
constexpr int MAX_DRAWS = 10000;

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

// a pair without a pose: status 0, NaN E and pose, zero mask and counts
__device__ void write_failure(int p, int64_t o0, int n, int32_t* __restrict__ out_status, double* __restrict__ out_E,
                              double* __restrict__ out_pose, uint8_t* __restrict__ out_mask,
                              int32_t* __restrict__ out_nr, int32_t* __restrict__ out_ni) {
    const int tid = threadIdx.x;
    if (tid == 0) { out_status[p] = 0; out_nr[p] = 0; out_ni[p] = 0; }
    if (tid < 9) out_E[9 * (int64_t)p + tid] = qnan();
    if (tid < 12) out_pose[12 * (int64_t)p + tid] = qnan();
    for (int i = tid; i < n; i += BLOCK) out_mask[o0 + i] = 0;
}

__global__ __launch_bounds__(BLOCK)
void pose_pair_kernel(const ShotP* __restrict__ shots, const PairP* __restrict__ pairs, const DMatchDev* __restrict__ matches,
                      const int64_t* __restrict__ off, double* __restrict__ scratch, int64_t scratch_n,
                      uint8_t* __restrict__ cbits, int max_iters, double confidence, int32_t* __restrict__ out_status,
                      double* __restrict__ out_E, double* __restrict__ out_pose, uint8_t* __restrict__ out_mask,
                      int32_t* __restrict__ out_nr, int32_t* __restrict__ out_ni, int64_t* __restrict__ res) {
    __shared__ double pts[CAP * 4];
    __shared__ double ws[PM_WS * BATCH];
    __shared__ int sub[BATCH][5];
    __shared__ int nmod[BATCH];
    __shared__ int good[BATCH][10];
    __shared__ double s_best[9];
    __shared__ double s_cand[4][12];
    __shared__ int s_cnt[BLOCK / 64][5];
    __shared__ int s_nb, s_fail_at, s_done, s_niters, s_maxgood, s_it;
    __shared__ unsigned long long s_rng;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t o0 = off[p];
    const int n = (int)(off[p + 1] - o0);
    if (n < 5 || (n > CAP && (scratch == nullptr || o0 < 0 || o0 + n > scratch_n))) {
        write_failure(p, o0, n, out_status, out_E, out_pose, out_mask, out_nr, out_ni);
        return;
    }
    const PairP P = pairs[p];
    const ShotP* SL = shots + P.left;
    const ShotP* SR = shots + P.right;
    const CamP camL = SL->cam, camR = SR->cam;
    const float2* kl = SL->kp;
    const float2* kr = SR->kp;
    const int nl = SL->nkp, nr = SR->nkp;
    // the mean camera matrix of the two-camera findEssentialMat overload
    const double fx = (camL.fx + camR.fx) * 0.5, fy = (camL.fy + camR.fy) * 0.5;
    const double cx = (camL.cx + camR.cx) * 0.5, cy = (camL.cy + camR.cy) * 0.5;
    double* C = n <= CAP ? pts : scratch + 4 * o0;
    bool bad = false;
    for (int i = tid; i < n; i += BLOCK) {
        const DMatchDev d = matches[o0 + i];
        double x1 = 0, y1 = 0, x2 = 0, y2 = 0;
        if (d.queryIdx < 0 || d.queryIdx >= nl || d.trainIdx < 0 || d.trainIdx >= nr) bad = true;
        else {
            const float2 a = kl[d.queryIdx], b = kr[d.trainIdx];
            posem::prepare_point(a.x, a.y, camL, fx, fy, cx, cy, x1, y1);
            posem::prepare_point(b.x, b.y, camR, fx, fy, cx, cy, x2, y2);
        }
        C[4 * i] = x1; C[4 * i + 1] = y1; C[4 * i + 2] = x2; C[4 * i + 3] = y2;
    }
    if (tid == 0) {
        s_niters = n == 5 ? 1 : max(max_iters, 1);   // 5 matches: the sample is the list, every iteration the same
        s_maxgood = 0; s_it = 0; s_done = 0;
        s_rng = ~0ull;                                // cv::RNG((uint64)-1)
    }
    if (__syncthreads_or(bad)) {   // a match index outside its image's keypoints: the call fails
        if (tid == 0) res[1] = 1;
        write_failure(p, o0, n, out_status, out_E, out_pose, out_mask, out_nr, out_ni);
        return;
    }
    const double thr_n = P.thr / ((fx + fy) / 2.0);
    const float thr2 = (float)(thr_n * thr_n);
#pragma unroll 1
    for (int round = 0; round < INT_MAX; ++round) {   // (ends by s_done: every round adds at least one iteration)
        if (tid == 0) {   // 1. the next subsets, in iteration order (getSubset without checkSubset)
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
        if (tid < nb) {   // 2. one minimal sample per lane
            double q[5][4];
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                const int i = sub[tid][r];
#pragma unroll
                for (int c = 0; c < 4; ++c) q[r][c] = C[4 * i + c];
            }
            nmod[tid] = posem::five_point(q, ws + tid, BATCH);
        }
        __syncthreads();
        // 3. inlier counts (computeError + findInliers): wave w takes samples w, w + 4, ... whole
        for (int b = wid; b < nb; b += BLOCK / 64) {
            const int nm = nmod[b];
            for (int m = 0; m < nm; ++m) {
                double E[9];
#pragma unroll
                for (int e = 0; e < 9; ++e) E[e] = ws[(PM_MODELS + 9 * m + e) * BATCH + b];
                int cnt = 0;
                for (int i0 = 0; i0 < n; i0 += 64) {
                    const int i = min(i0 + lane, n - 1);
                    const float err = posem::sampson_error(E, C[4 * i], C[4 * i + 1], C[4 * i + 2], C[4 * i + 3]);
                    cnt += __popcll(__ballot(i0 + lane < n && err <= thr2));   // a NaN error is no inlier
                }
                if (lane == 0) good[b][m] = cnt;
            }
        }
        __syncthreads();
        if (tid == 0) {   // 4. replay in iteration order, models in root order
            for (int b = 0; b < nb; ++b) {
                if (s_it + b >= s_niters) { s_done = 1; break; }
                for (int m = 0; m < nmod[b]; ++m) {
                    const int g = good[b][m];
                    if (g > max(s_maxgood, 4)) {
                        s_maxgood = g;
                        for (int e = 0; e < 9; ++e) s_best[e] = ws[(PM_MODELS + 9 * m + e) * BATCH + b];
                        s_niters = update_num_iters(confidence, (double)(n - g) / n, s_niters);
                    }
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
        write_failure(p, o0, n, out_status, out_E, out_pose, out_mask, out_nr, out_ni);
        return;
    }
    // ---- recoverPose(E, left, right, K_L, R, t, mask): the raw keypoints, both sides with the left camera
    if (tid == 0) {
        double cand[4][12];
        posem::pose_candidates(s_best, cand);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int e = 0; e < 12; ++e) s_cand[c][e] = cand[c][e];
    }
    __syncthreads();
    double E[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) E[e] = s_best[e];
    int c_r = 0, c_0 = 0, c_1 = 0, c_2 = 0, c_3 = 0;
    for (int i0 = 0; i0 < n; i0 += BLOCK) {
        const int i = i0 + tid;
        const bool in = i < n;
        const int ic = in ? i : n - 1;
        const bool inl = in && posem::sampson_error(E, C[4 * ic], C[4 * ic + 1], C[4 * ic + 2], C[4 * ic + 3]) <= thr2;
        int bits = 0;
        if (inl) {
            const DMatchDev d = matches[o0 + i];
            const float2 a = kl[d.queryIdx], b = kr[d.trainIdx];
            const double x1 = ((double)a.x - camL.cx) / camL.fx, y1 = ((double)a.y - camL.cy) / camL.fy;
            const double x2 = ((double)b.x - camL.cx) / camL.fx, y2 = ((double)b.y - camL.cy) / camL.fy;
#pragma unroll 1
            for (int c = 0; c < 4; ++c)
                if (posem::cheirality(&s_cand[c][0], x1, y1, x2, y2)) bits |= 1 << c;
        }
        if (in) cbits[o0 + i] = (uint8_t)bits;
        c_r += __popcll(__ballot(inl));
        c_0 += __popcll(__ballot(bits & 1));
        c_1 += __popcll(__ballot(bits & 2));
        c_2 += __popcll(__ballot(bits & 4));
        c_3 += __popcll(__ballot(bits & 8));
    }
    if (lane == 0) { s_cnt[wid][0] = c_r; s_cnt[wid][1] = c_0; s_cnt[wid][2] = c_1; s_cnt[wid][3] = c_2; s_cnt[wid][4] = c_3; }
    __syncthreads();
    int tot[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) tot[k] = s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k];
    const int win = posem::choose_candidate(tot[1], tot[2], tot[3], tot[4]);
    if (tid == 0) {
        out_status[p] = 1;
        out_nr[p] = tot[0];
        out_ni[p] = win == 0 ? tot[1] : (win == 1 ? tot[2] : (win == 2 ? tot[3] : tot[4]));
    }
    if (tid < 9) out_E[9 * (int64_t)p + tid] = s_best[tid];
    if (tid < 12) out_pose[12 * (int64_t)p + tid] = s_cand[win][tid];
    for (int i = tid; i < n; i += BLOCK) out_mask[o0 + i] = (uint8_t)((cbits[o0 + i] >> win) & 1);   // (own writes)
}

// One block: out_off = exclusive scan of the pairs' inlier counts (chunks of 1024 with a carry), total last.
__global__ __launch_bounds__(1024)
void pose_scan_kernel(const int32_t* __restrict__ count, int n_pairs, int64_t* __restrict__ out_off, int64_t* __restrict__ res) {
    __shared__ long long s_wave[16];
    __shared__ long long s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < n_pairs; base += 1024) {
        const int i = base + tid;
        const long long v = i < n_pairs ? count[i] : 0;
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
        if (i < n_pairs) out_off[i] = carry + woff + x - v;
        __syncthreads();
        if (tid == 1023) s_carry = carry + woff + x;
        __syncthreads();
    }
    if (tid == 0) { out_off[n_pairs] = s_carry; res[0] = s_carry; }
}

__global__ __launch_bounds__(BLOCK)
void pose_compact_kernel(const DMatchDev* __restrict__ matches, const int64_t* __restrict__ off, const uint8_t* __restrict__ mask,
                         const int64_t* __restrict__ out_off, DMatchDev* __restrict__ out_matches) {
    __shared__ int s_w[BLOCK / 64];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t o0 = off[p];
    const int n = (int)(off[p + 1] - o0);
    int64_t base = out_off[p];
    for (int i0 = 0; i0 < n; i0 += BLOCK) {
        const int i = i0 + tid;
        const bool keep = i < n && mask[o0 + i] != 0;
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_w[wid] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) {
            before += w < wid ? s_w[w] : 0;
            total += s_w[w];
        }
        if (keep) out_matches[base + before + __popcll(m & ((1ull << lane) - 1ull))] = matches[o0 + i];
        base += total;
        __syncthreads();
    }
}

thread_local float g_last_ms = -1.f;

Slot g_slot[64];   // csrc/device_call.hpp

}  // namespace pose
}  // namespace sfmx

using namespace sfmx;
using namespace sfmx::pose;

extern "C" {

float sfmx_relative_poses_last_kernel_ms(void) { return g_last_ms; }

int sfmx_relative_poses(const sfmx_point2f* const* keypoints, const int32_t* n_keypoints, int32_t n_shots,
                        const sfmx_tri_camera* cameras, int32_t n_cameras, const int32_t* shot_camera,
                        const int32_t* shot_size, const int32_t* pairs, int32_t n_pairs, const sfmx_dmatch* matches,
                        const int64_t* pair_offsets, double threshold, double confidence, int32_t max_iters,
                        int32_t inputs_on_device, int32_t device, void* stream, int32_t* out_status, double* out_E,
                        double* out_pose, uint8_t* out_mask, int32_t* out_n_ransac_inliers, int32_t* out_n_inliers,
                        sfmx_dmatch* out_matches, int64_t* out_pair_offsets) {
    if (n_shots < 0 || n_cameras < 0 || n_pairs < 0) { set_last_error("negative count"); return SFMX_EINVAL; }
    if (!out_pair_offsets || !pair_offsets ||
        (n_pairs && (!pairs || !out_status || !out_E || !out_pose || !out_n_ransac_inliers || !out_n_inliers)) ||
        (n_shots && (!keypoints || !n_keypoints || !shot_camera || !shot_size)) || (n_cameras && !cameras)) {
        set_last_error("null argument");
        return SFMX_EINVAL;
    }
    if (!(threshold < 0.0 || threshold > 0.0)) { set_last_error("threshold must be negative (pixels) or positive (fraction)"); return SFMX_EINVAL; }
    if (!(confidence > 0.0 && confidence < 1.0)) { set_last_error("confidence must be in (0, 1)"); return SFMX_EINVAL; }
    if (max_iters < 1) { set_last_error("max_iters must be at least 1"); return SFMX_EINVAL; }
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
        // the pair offsets on the host: they size the scratch
        std::vector<int64_t> hoff(n_pairs + 1);
        std::vector<double> nanv;
        int64_t n = 0, nk = 0, longest = 0;
        if (inputs_on_device) {
            SFMX_HIP_CHK(hipMemcpyAsync(hoff.data(), pair_offsets, sizeof(int64_t) * (n_pairs + 1), hipMemcpyDeviceToHost, st));
            SFMX_HIP_CHK(hipStreamSynchronize(st));
        } else {
            std::memcpy(hoff.data(), pair_offsets, sizeof(int64_t) * (n_pairs + 1));
        }
        if (hoff[0] != 0) { set_last_error("pair offsets do not start at 0"); rc = SFMX_EINVAL; goto done; }
        for (int p = 0; p < n_pairs; ++p) {
            if (hoff[p + 1] < hoff[p]) { set_last_error("pair offsets not ascending"); rc = SFMX_EINVAL; goto done; }
            longest = std::max(longest, hoff[p + 1] - hoff[p]);
        }
        if (longest > INT32_MAX) { set_last_error("too many matches in one pair"); rc = SFMX_EINVAL; goto done; }
        n = hoff[n_pairs];
        if (n == 0) {   // no match: nothing is launched; every pair has status 0
            nanv.assign((size_t)21 * n_pairs, std::nan(""));
            for (double& v : nanv) { const uint64_t b = 0x7FF8000000000000ull; std::memcpy(&v, &b, 8); }
            if (inputs_on_device) {
                SFMX_HIP_CHK(hipMemsetAsync(out_pair_offsets, 0, sizeof(int64_t) * (n_pairs + 1), st));
                if (n_pairs) {
                    SFMX_HIP_CHK(hipMemsetAsync(out_status, 0, sizeof(int32_t) * n_pairs, st));
                    SFMX_HIP_CHK(hipMemsetAsync(out_n_ransac_inliers, 0, sizeof(int32_t) * n_pairs, st));
                    SFMX_HIP_CHK(hipMemsetAsync(out_n_inliers, 0, sizeof(int32_t) * n_pairs, st));
                    SFMX_HIP_CHK(hipMemcpyAsync(out_E, nanv.data(), sizeof(double) * 9 * n_pairs, hipMemcpyHostToDevice, st));
                    SFMX_HIP_CHK(hipMemcpyAsync(out_pose, nanv.data(), sizeof(double) * 12 * n_pairs, hipMemcpyHostToDevice, st));
                }
                SFMX_HIP_CHK(hipStreamSynchronize(st));
            } else {
                std::memset(out_pair_offsets, 0, sizeof(int64_t) * (n_pairs + 1));
                if (n_pairs) {
                    std::memset(out_status, 0, sizeof(int32_t) * n_pairs);
                    std::memset(out_n_ransac_inliers, 0, sizeof(int32_t) * n_pairs);
                    std::memset(out_n_inliers, 0, sizeof(int32_t) * n_pairs);
                    std::memcpy(out_E, nanv.data(), sizeof(double) * 9 * n_pairs);
                    std::memcpy(out_pose, nanv.data(), sizeof(double) * 12 * n_pairs);
                }
            }
            g_last_ms = 0.f;
            goto done;
        }
        if (!matches || !out_mask || !out_matches) { set_last_error("null argument"); rc = SFMX_EINVAL; goto done; }
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
            // device block: [shot table | pair table | result words | correspondence scratch (only with a list over
            // CAP) | candidate bits | (host inputs: keypoints, matches, offsets, every output)]
            const bool H = F.host;
            const size_t np = (size_t)n_pairs;
            BlockLayout L;
            ShotP* shd;
            PairP* prd;
            int64_t *resd, *od, *ood;
            double *scr, *oed, *opd;
            uint8_t *cbd, *okd;
            float2* kd;
            sfmx_dmatch *md, *omd;
            int32_t *osd, *ord_, *oid;
            L.want(shd, n_shots);
            L.want(prd, np);
            L.want(resd, 2);
            const size_t b_tab = L.need;   // up to here: staged in pinned memory, one upload
            L.want(scr, 4 * n, longest > CAP);
            L.want(cbd, n);
            L.want(kd, nk, H);
            L.want(md, n, H);
            L.want(od, np + 1, H);
            L.want(osd, np, H);
            L.want(oed, 9 * np, H);
            L.want(opd, 12 * np, H);
            L.want(okd, n, H);
            L.want(ord_, np, H);
            L.want(oid, np, H);
            L.want(omd, n, H);
            L.want(ood, np + 1, H);
            rc = F.reserve(L, b_tab);
            if (rc != SFMX_OK) goto done;
            // shot table: camera and keypoint pointer of every shot
            ShotP* hs = F.pinned(shd);
            int64_t o = 0;
            for (int i = 0; i < n_shots; ++i) {
                const sfmx_tri_camera& c = cameras[shot_camera[i]];
                ShotP& t = hs[i];
                t.cam = CamP{c.K[0], c.K[4], c.K[2], c.K[5], c.dist[0], c.dist[1], c.dist[2], c.dist[3], c.dist[4]};
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
            PairP* hp = F.pinned(prd);
            for (int p = 0; p < n_pairs; ++p) {
                const int L = pairs[2 * p], R = pairs[2 * p + 1];
                // SfM.cpp:515-521; the right width is never looked at (:519)
                const double thr = threshold < 0 ? -threshold
                                                 : std::max({shot_size[2 * L], shot_size[2 * L + 1], shot_size[2 * R + 1],
                                                             shot_size[2 * R + 1]}) * threshold;
                hp[p] = PairP{L, R, thr};
            }
            int64_t* hres = F.pinned(resd);
            hres[0] = hres[1] = 0;
            SFMX_HIP_CHK(F.upload(b_tab));   // tables, result words = 0
            const DMatchDev* dm = reinterpret_cast<const DMatchDev*>(F.in(matches, md, n));
            const int64_t* doff = F.in(pair_offsets, od, np + 1);
            SFMX_HIP_CHK(F.err);
            int32_t *dst = F.out(out_status, osd), *dnr = F.out(out_n_ransac_inliers, ord_), *dni = F.out(out_n_inliers, oid);
            double *dE = F.out(out_E, oed), *dP = F.out(out_pose, opd);
            uint8_t* dk = F.out(out_mask, okd);
            DMatchDev* dom = reinterpret_cast<DMatchDev*>(F.out(out_matches, omd));
            int64_t* doo = F.out(out_pair_offsets, ood);
            (void)hipEventRecord(S->e0, st);
            pose_pair_kernel<<<(unsigned)n_pairs, BLOCK, 0, st>>>(shd, prd, dm, doff, scr, n, cbd, max_iters, confidence, dst, dE,
                                                                  dP, dk, dnr, dni, resd);
            pose_scan_kernel<<<1, 1024, 0, st>>>(dni, n_pairs, doo, resd);
            pose_compact_kernel<<<(unsigned)n_pairs, BLOCK, 0, st>>>(dm, doff, dk, doo, dom);
            (void)hipEventRecord(S->e1, st);
            SFMX_HIP_CHK(hipGetLastError());
            SFMX_HIP_CHK(hipMemcpyAsync(hres, resd, sizeof(int64_t) * 2, hipMemcpyDeviceToHost, st));   // total and the index flag
            SFMX_HIP_CHK(hipStreamSynchronize(st));
            if (hres[1] != 0) { set_last_error("match index outside its image's keypoints"); rc = SFMX_EINVAL; goto done; }
            const int64_t total = hres[0];
            if (total < 0 || total > n) { set_last_error("inlier count self check failed"); rc = SFMX_EINTERNAL; goto done; }
            SFMX_HIP_CHK(F.back(out_status, osd, np));
            SFMX_HIP_CHK(F.back(out_E, oed, 9 * np));
            SFMX_HIP_CHK(F.back(out_pose, opd, 12 * np));
            SFMX_HIP_CHK(F.back(out_mask, okd, n));
            SFMX_HIP_CHK(F.back(out_n_ransac_inliers, ord_, np));
            SFMX_HIP_CHK(F.back(out_n_inliers, oid, np));
            if (total) SFMX_HIP_CHK(F.back(out_matches, omd, total));
            SFMX_HIP_CHK(F.back(out_pair_offsets, ood, np + 1));
            if (H) SFMX_HIP_CHK(hipStreamSynchronize(st));
            float ms = -1.f;
            (void)hipEventElapsedTime(&ms, S->e0, S->e1);
            g_last_ms = ms;
        }
    done:;
        rc = F.finish(rc, "sfmx_relative_poses");
    }
    return rc;
}

}  // extern "C"
