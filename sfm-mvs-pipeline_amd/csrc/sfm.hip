// SPDX-License-Identifier: MIT
// sfmx incremental reconstruction: the ABI of include/sfmx_sfm.h over the control flow of
// csrc/sfm_host.hpp.  The argument checks run before any step is called.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/sfmx_sfm.h"
#include "../../include/sfmx_pnp.h"
#include "../../include/sfmx_pose.h"
#include "../../include/sfmx_scene.h"
#include "match_common.hpp"
#include "sfm_host.hpp"

using namespace sfmx;

namespace {

// getDistinctShotMatches on the device: the first origin record (point-major order) through which each pair gave
// the shot a 3D-2D match.  A keypoint or pair index out of range sets the flag.
__global__ __launch_bounds__(256)
void first_record_of_pair_kernel(int64_t n_rec, const int32_t* __restrict__ found_kp, const int32_t* __restrict__ found_pair,
                                 int32_t n_pairs, int32_t n_kp_shot, int32_t* __restrict__ first, int32_t* __restrict__ flag) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rec) return;
    const int32_t k = found_kp[r];
    if (k < 0) return;
    const int32_t p = found_pair[r];
    if (k >= n_kp_shot || p < 0 || p >= n_pairs) { atomicOr(flag, 1); return; }
    atomicMin(first + p, (int32_t)r);
}

#define ROW_HIP(expr) do { if ((expr) != hipSuccess) { set_last_error("HIP error in " #expr); return SFMX_EDEVICE; } } while (0)

// The scene of sfmx_sfm_triangulate and the library's rows as the steps of the loop.  The scene lives on the device
// between the rows: the keypoints go up once, the packed match lists, the cloud (coordinates and origin CSR) and what
// one row hands the next stay there, and every row is called with inputs_on_device = 1.  A list that shrinks to its
// inliers is repacked on the device.  The host sees the pair offsets, the counts, statuses and poses, and for the
// adjustment the cloud (sfmx_ba_solve takes host arrays); the merge reads the pair offsets and a few words and stages
// the cloud only when its resolution falls back to the host (sfmx_scene.h).
struct Rows {
    const sfmx_point2f* const* kp;
    const int32_t* nkp;
    int32_t n_shots;
    const int32_t* shot_size;
    sfmx_tri_camera cam;
    int32_t cam_model;
    const int32_t* pairs;
    int32_t n_pairs;
    sfmx_sfm_params prm;
    int32_t device;
    int64_t M = 0, max_list = 0;       // matches of the graph on entry, the longest list
    std::vector<int32_t> shot_camera;  // all 0
    std::vector<int64_t> off;          // pair offsets of the packed lists as they are now
    std::vector<double> pose;          // 12 * n_shots
    int64_t n_points = 0, n_rec = 0;   // the cloud's sizes
    int32_t cur = 0;                   // which of the two cloud buffers holds the cloud (the merge writes the other)
    int64_t n_new = 0;                 // elements of the last triangulate_pair, on the device
    int32_t pend_pair = -1, pend_shot = -1;
    int64_t pend_inliers = 0;
    double pend_pair_pose[12], pend_shot_pose[12];
    sfmx_sfm_timing tm{};
    int row_error = 0;   // the first negative value a row returned (the loop's own SFMX_ECAPACITY means a short trace)
    int note(int r) { if (r < 0 && !row_error) row_error = r; return r; }

    // device memory
    std::vector<void*> owned;
    std::vector<const sfmx_point2f*> d_kp;
    sfmx_dmatch *d_m = nullptr, *d_tmp = nullptr, *d_inl = nullptr;
    int64_t *d_off = nullptr, *d_off2 = nullptr, *d_ooff = nullptr, *d_po = nullptr, *d_nmatch = nullptr, *d_noff = nullptr;
    int32_t *d_status = nullptr, *d_nr = nullptr, *d_ni = nullptr, *d_nosh = nullptr, *d_target = nullptr, *d_cnt = nullptr;
    int32_t *d_fk = nullptr, *d_fp = nullptr, *d_first = nullptr, *d_flag = nullptr, *d_start = nullptr;
    double *d_E = nullptr, *d_pose = nullptr, *d_rpose = nullptr, *d_nxyz = nullptr, *d_noxy = nullptr, *d_dist = nullptr;
    double *d_p3 = nullptr, *d_p2 = nullptr, *d_ratio = nullptr;
    float* d_fxy = nullptr;
    uint8_t* d_mask = nullptr;
    double *c_xyz[2] = {nullptr, nullptr}, *c_oxy[2] = {nullptr, nullptr};
    int64_t* c_oo[2] = {nullptr, nullptr};
    int32_t* c_osh[2] = {nullptr, nullptr};
    int prev_device = -1;

    ~Rows() {
        for (void* q : owned) (void)hipFree(q);
        if (prev_device >= 0) (void)hipSetDevice(prev_device);
    }
    template <class T> bool alloc(T*& p, int64_t count) {
        void* q = nullptr;
        if (hipMalloc(&q, sizeof(T) * (size_t)std::max<int64_t>(count, 1)) != hipSuccess) { (void)hipGetLastError(); return false; }
        owned.push_back(q);
        p = static_cast<T*>(q);
        return true;
    }

    struct Clock {
        Rows& r;
        const int row;
        const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        Clock(Rows& rows, int which) : r(rows), row(which) {}
        ~Clock() {
            r.tm.wall_ms[row] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            ++r.tm.calls[row];
        }
    };
    void device_ms(int row, float ms) { if (ms > 0.f) tm.device_ms[row] += ms; }

    // the device and the scene's first upload: keypoints, match lists, offsets, 2 * arange for the new elements' CSR
    int open(const sfmx_dmatch* matches, const int64_t* pair_offsets) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_last_error("no HIP device visible"); return SFMX_EDEVICE; }
        if (device < 0 || device >= ndev) { set_last_error("device index out of range"); return SFMX_EINVAL; }
        (void)hipGetDevice(&prev_device);
        ROW_HIP(hipSetDevice(device));
        off.assign(pair_offsets, pair_offsets + n_pairs + 1);
        M = off[n_pairs];
        for (int p = 0; p < n_pairs; ++p) max_list = std::max(max_list, off[p + 1] - off[p]);
        if (M > (int64_t)1 << 29) { set_last_error("more than 2^29 matches"); return SFMX_ECAPACITY; }
        int64_t nk = 0;
        for (int s = 0; s < n_shots; ++s) nk += nkp[s];
        sfmx_point2f* kblock = nullptr;
        bool ok = alloc(kblock, nk) && alloc(d_m, M) && alloc(d_tmp, M) && alloc(d_inl, max_list) && alloc(d_off, n_pairs + 1) &&
                  alloc(d_off2, 2) && alloc(d_ooff, 2) && alloc(d_po, 2) && alloc(d_nmatch, max_list) && alloc(d_noff, max_list + 1) &&
                  alloc(d_status, 1) && alloc(d_nr, 1) && alloc(d_ni, 1) && alloc(d_nosh, 2 * max_list) && alloc(d_target, max_list) &&
                  alloc(d_cnt, n_shots) && alloc(d_fk, 2 * M) && alloc(d_fp, 2 * M) && alloc(d_first, n_pairs) && alloc(d_flag, 1) &&
                  alloc(d_start, 1) && alloc(d_E, 9) && alloc(d_pose, 12) && alloc(d_rpose, 12) && alloc(d_nxyz, 3 * max_list) &&
                  alloc(d_noxy, 4 * max_list) && alloc(d_dist, max_list) && alloc(d_p3, 6 * M) && alloc(d_p2, 4 * M) &&
                  alloc(d_ratio, 1) && alloc(d_fxy, 4 * M) && alloc(d_mask, 2 * M);
        for (int b = 0; ok && b < 2; ++b)
            ok = alloc(c_xyz[b], 3 * M) && alloc(c_oo[b], M + 1) && alloc(c_osh[b], 2 * M) && alloc(c_oxy[b], 4 * M);
        if (!ok) { set_last_error("device allocation failed"); return SFMX_ENOMEM; }
        Clock c(*this, SFMX_SFM_ROW_HANDOFF);
        d_kp.assign((size_t)std::max(n_shots, 1), nullptr);
        int64_t o = 0;
        for (int s = 0; s < n_shots; ++s) {
            d_kp[s] = kblock + o;
            if (nkp[s]) ROW_HIP(hipMemcpy(kblock + o, kp[s], sizeof(sfmx_point2f) * nkp[s], hipMemcpyHostToDevice));
            o += nkp[s];
        }
        if (M) ROW_HIP(hipMemcpy(d_m, matches, sizeof(sfmx_dmatch) * M, hipMemcpyHostToDevice));
        ROW_HIP(hipMemcpy(d_off, off.data(), sizeof(int64_t) * (n_pairs + 1), hipMemcpyHostToDevice));
        std::vector<int64_t> noff((size_t)max_list + 1);
        for (int64_t i = 0; i <= max_list; ++i) noff[i] = 2 * i;
        ROW_HIP(hipMemcpy(d_noff, noff.data(), sizeof(int64_t) * (max_list + 1), hipMemcpyHostToDevice));
        const int64_t zero = 0;
        ROW_HIP(hipMemcpy(c_oo[0], &zero, sizeof zero, hipMemcpyHostToDevice));
        tm.handoff_bytes[SFMX_SFM_ROW_HANDOFF] += nk * 8 + M * 16 + (n_pairs + 1) * 8 + (max_list + 1) * 8;
        return SFMX_OK;
    }

    int single_offsets(int64_t m) {   // {0, m}: the offsets of a call on one pair or one set
        const int64_t o[2] = {0, m};
        ROW_HIP(hipMemcpy(d_off2, o, sizeof o, hipMemcpyHostToDevice));
        return SFMX_OK;
    }

    int relative_pose(int32_t p, int32_t* n_inliers) {
        const int64_t m = off[p + 1] - off[p];
        pend_pair = -1;
        *n_inliers = 0;
        if (m == 0) return 0;   // an empty list: findEssentialMat throws
        int rc = single_offsets(m);
        if (rc < 0) return rc;
        {
            Clock c(*this, SFMX_SFM_ROW_POSE);
            rc = sfmx_relative_poses(d_kp.data(), nkp, n_shots, &cam, 1, shot_camera.data(), shot_size, pairs + 2 * p, 1,
                                     d_m + off[p], d_off2, prm.ransac_baseline_threshold, SFMX_POSE_CONFIDENCE, SFMX_POSE_MAX_ITERS,
                                     1, device, nullptr, d_status, d_E, d_pose, d_mask, d_nr, d_ni, d_inl, d_ooff);
        }
        if (rc < 0) return rc;
        device_ms(SFMX_SFM_ROW_POSE, sfmx_relative_poses_last_kernel_ms());
        int32_t status = 0, ni = 0;
        int64_t ooff[2] = {0, 0};
        ROW_HIP(hipMemcpy(&status, d_status, sizeof status, hipMemcpyDeviceToHost));
        ROW_HIP(hipMemcpy(&ni, d_ni, sizeof ni, hipMemcpyDeviceToHost));
        ROW_HIP(hipMemcpy(ooff, d_ooff, sizeof ooff, hipMemcpyDeviceToHost));
        ROW_HIP(hipMemcpy(pend_pair_pose, d_pose, sizeof pend_pair_pose, hipMemcpyDeviceToHost));
        tm.handoff_bytes[SFMX_SFM_ROW_POSE] += 16 + 4 + 4 + 16 + 96;
        if (status != 1) return 0;
        if (ooff[1] < 0 || ooff[1] > m || ooff[1] != ni) { set_last_error("relative pose: inlier count self check failed"); return SFMX_EINTERNAL; }
        pend_inliers = ooff[1];
        pend_pair = p;
        *n_inliers = ni;
        return 1;
    }

    // setMatches(inlierMatches) on the packed lists: the inliers take the head of the pair's slot, the tail moves up
    int replace_list(int32_t p) {
        Clock c(*this, SFMX_SFM_ROW_HANDOFF);
        const int64_t m = off[p + 1] - off[p], k = pend_inliers, tail = off[n_pairs] - off[p + 1];
        if (k) ROW_HIP(hipMemcpy(d_m + off[p], d_inl, sizeof(sfmx_dmatch) * k, hipMemcpyDeviceToDevice));
        if (k != m && tail) {   // through the spare buffer: source and destination overlap
            ROW_HIP(hipMemcpy(d_tmp, d_m + off[p + 1], sizeof(sfmx_dmatch) * tail, hipMemcpyDeviceToDevice));
            ROW_HIP(hipMemcpy(d_m + off[p] + k, d_tmp, sizeof(sfmx_dmatch) * tail, hipMemcpyDeviceToDevice));
        }
        for (int q = p + 1; q <= n_pairs; ++q) off[q] -= m - k;
        ROW_HIP(hipMemcpy(d_off, off.data(), sizeof(int64_t) * (n_pairs + 1), hipMemcpyHostToDevice));
        tm.handoff_bytes[SFMX_SFM_ROW_HANDOFF] += (n_pairs + 1) * 8;
        return SFMX_OK;
    }

    int triangulate_pair(int32_t p, int32_t initial, int32_t* n_points_out) {
        if (pend_pair != p) { set_last_error("triangulation without the pair's relative pose"); return SFMX_ESTATE; }
        int rc = replace_list(p);
        if (rc < 0) return rc;
        pend_pair = -1;
        if (initial) {
            const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
            std::memcpy(&pose[12 * (size_t)pairs[2 * p]], eye, sizeof eye);
            std::memcpy(&pose[12 * (size_t)pairs[2 * p + 1]], pend_pair_pose, sizeof pend_pair_pose);
        }
        const int64_t m = off[p + 1] - off[p];
        n_new = 0;
        *n_points_out = 0;
        if (m == 0) return 0;   // triangulateMatch returns at once (SfM.cpp:385-387)
        rc = single_offsets(m);
        if (rc < 0) return rc;
        int64_t total = 0;
        {
            Clock c(*this, SFMX_SFM_ROW_TRIANGULATE);
            rc = sfmx_triangulate_matches(d_kp.data(), nkp, n_shots, &cam, 1, shot_camera.data(), pose.data(), pairs + 2 * p, 1,
                                          d_m + off[p], d_off2, prm.max_reprojection_error, 1, device, nullptr, d_po, d_nxyz,
                                          d_nmatch, d_nosh, d_noxy, nullptr, &total);
        }
        if (rc < 0) return rc;
        device_ms(SFMX_SFM_ROW_TRIANGULATE, sfmx_triangulate_last_kernel_ms());
        tm.handoff_bytes[SFMX_SFM_ROW_TRIANGULATE] += 16 + 8;
        if (total < 0 || total > m) { set_last_error("triangulation: point count self check failed"); return SFMX_EINTERNAL; }
        n_new = total;
        *n_points_out = (int32_t)total;
        return 0;
    }

    int add_elements(int32_t, int32_t merge) {
        if (n_new == 0) return 0;
        if (n_points + n_new > M || n_rec + 2 * n_new > 2 * M) { set_last_error("cloud beyond its bound"); return SFMX_EINTERNAL; }
        if (!merge) {   // scene.addPointcloudElement for each: the elements go behind the cloud as they are
            Clock c(*this, SFMX_SFM_ROW_HANDOFF);
            ROW_HIP(hipMemcpy(c_xyz[cur] + 3 * n_points, d_nxyz, sizeof(double) * 3 * n_new, hipMemcpyDeviceToDevice));
            ROW_HIP(hipMemcpy(c_osh[cur] + n_rec, d_nosh, sizeof(int32_t) * 2 * n_new, hipMemcpyDeviceToDevice));
            ROW_HIP(hipMemcpy(c_oxy[cur] + 2 * n_rec, d_noxy, sizeof(double) * 4 * n_new, hipMemcpyDeviceToDevice));
            std::vector<int64_t> o((size_t)n_new);
            for (int64_t i = 0; i < n_new; ++i) o[i] = n_rec + 2 * (i + 1);
            ROW_HIP(hipMemcpy(c_oo[cur] + n_points + 1, o.data(), sizeof(int64_t) * n_new, hipMemcpyHostToDevice));
            tm.handoff_bytes[SFMX_SFM_ROW_HANDOFF] += n_new * 8;
            n_points += n_new;
            n_rec += 2 * n_new;
            n_new = 0;
            return 0;
        }
        const int nxt = cur ^ 1;
        int32_t k = 0;
        int64_t r = 0;
        int rc;
        {
            Clock c(*this, SFMX_SFM_ROW_MERGE);
            rc = sfmx_merge_pointcloud_3d2d(d_kp.data(), nkp, n_shots, pairs, n_pairs, d_m, d_off, c_xyz[cur], (int32_t)n_points,
                                            c_oo[cur], c_osh[cur], c_oxy[cur], d_nxyz, (int32_t)n_new, d_noff, d_nosh, d_noxy,
                                            prm.point_merge_distance, prm.feature_merge_distance, 1, device, nullptr, d_target, d_dist,
                                            c_xyz[nxt], c_oo[nxt], c_osh[nxt], c_oxy[nxt], &k, &r);
        }
        if (rc < 0) return rc;
        device_ms(SFMX_SFM_ROW_MERGE, sfmx_merge_pointcloud_last_kernel_ms());
        {   // every byte the call copied between host and device, the two counts included
            int64_t bytes = 0;
            (void)sfmx_merge_pointcloud_last_path(nullptr, nullptr, &bytes);
            tm.handoff_bytes[SFMX_SFM_ROW_MERGE] += bytes;
        }
        if (k < n_points || k > n_points + n_new || r < n_rec || r > n_rec + 2 * n_new) {
            set_last_error("merge: cloud size self check failed");
            return SFMX_EINTERNAL;
        }
        cur = nxt;
        n_points = k;
        n_rec = r;
        n_new = 0;
        return 0;
    }

    int count_candidates(const int32_t* shots, int32_t n, int32_t* counts) {
        int rc;
        {
            Clock c(*this, SFMX_SFM_ROW_COUNT);
            rc = sfmx_count_3d2d_matches(d_kp.data(), nkp, n_shots, pairs, n_pairs, nullptr, d_m, d_off, c_oo[cur], (int32_t)n_points,
                                         c_osh[cur], c_oxy[cur], shots, n, 1, device, nullptr, d_cnt);
        }
        if (rc < 0) return rc;
        device_ms(SFMX_SFM_ROW_COUNT, sfmx_count_3d2d_last_kernel_ms());
        ROW_HIP(hipMemcpy(counts, d_cnt, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
        tm.handoff_bytes[SFMX_SFM_ROW_COUNT] += 4 * (int64_t)n + 8;
        return 0;
    }

    int register_shot(int32_t shot, double* ratio, int32_t* distinct, int32_t capacity, int32_t* n_distinct) {
        *n_distinct = 0;
        *ratio = -1.0;
        pend_shot = -1;
        if (n_rec == 0) return 0;   // an empty cloud has no 3D-2D match: solvePnPRansac throws
        int64_t n_set = 0;
        int rc;
        {
            Clock c(*this, SFMX_SFM_ROW_FIND);
            rc = sfmx_find_3d2d_matches(d_kp.data(), nkp, n_shots, pairs, n_pairs, d_m, d_off, c_oo[cur], (int32_t)n_points, c_osh[cur],
                                        c_oxy[cur], shot, 1, device, nullptr, d_fk, d_fp, d_fxy);
            if (rc >= 0) {
                device_ms(SFMX_SFM_ROW_FIND, sfmx_find_3d2d_last_kernel_ms());
                rc = sfmx_distinct_3d2d_points(c_xyz[cur], (int32_t)n_points, c_oo[cur], d_fk, d_fxy, 1, device, nullptr, d_p3, d_p2, &n_set);
                if (rc >= 0) device_ms(SFMX_SFM_ROW_FIND, sfmx_distinct_3d2d_last_kernel_ms());
            }
        }
        if (rc < 0) return rc;
        if (n_set < 0 || n_set > n_rec) { set_last_error("registration: distinct point count self check failed"); return SFMX_EINTERNAL; }
        // getDistinctShotMatches: the pairs of the 3D-2D matches, first appearance over the point-major records
        std::vector<int32_t> first((size_t)std::max(n_pairs, 1));
        int32_t flag = 0;
        ROW_HIP(hipMemset(d_first, 0x7f, sizeof(int32_t) * std::max(n_pairs, 1)));
        ROW_HIP(hipMemset(d_flag, 0, sizeof(int32_t)));
        first_record_of_pair_kernel<<<(unsigned)((n_rec + 255) / 256), 256>>>(n_rec, d_fk, d_fp, n_pairs, nkp[shot], d_first, d_flag);
        ROW_HIP(hipGetLastError());
        ROW_HIP(hipMemcpy(first.data(), d_first, sizeof(int32_t) * std::max(n_pairs, 1), hipMemcpyDeviceToHost));
        ROW_HIP(hipMemcpy(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost));
        tm.handoff_bytes[SFMX_SFM_ROW_FIND] += 4 * (int64_t)n_pairs + 4 + 8;
        if (flag) { set_last_error("registration: 3D-2D match out of range"); return SFMX_EINTERNAL; }
        std::vector<std::pair<int32_t, int32_t>> order;
        for (int32_t p = 0; p < n_pairs; ++p)
            if (first[p] != 0x7f7f7f7f) {
                if (first[p] < 0 || first[p] >= n_rec) { set_last_error("registration: record index out of range"); return SFMX_EINTERNAL; }
                order.push_back({first[p], p});
            }
        std::sort(order.begin(), order.end());
        if ((int64_t)order.size() > capacity) { set_last_error("registration: more distinct pairs than pairs"); return SFMX_EINTERNAL; }
        for (const auto& e : order) distinct[(*n_distinct)++] = e.second;
        if (n_set == 0) return 0;   // no 3D-2D match: solvePnPRansac throws
        rc = single_offsets(n_set);
        if (rc < 0) return rc;
        {
            Clock c(*this, SFMX_SFM_ROW_REGISTER);
            rc = sfmx_register_poses(d_p3, d_p2, d_off2, &shot, 1, &cam, 1, shot_camera.data(), shot_size, n_shots,
                                     prm.ransac_pose_threshold, SFMX_PNP_CONFIDENCE, SFMX_PNP_MAX_ITERS, 1, device, nullptr, d_status,
                                     d_pose, d_rpose, d_mask, d_ni, d_ratio, d_start);
        }
        if (rc < 0) return rc;
        device_ms(SFMX_SFM_ROW_REGISTER, sfmx_register_poses_last_kernel_ms());
        int32_t status = 0;
        double r = -1.0;
        ROW_HIP(hipMemcpy(&status, d_status, sizeof status, hipMemcpyDeviceToHost));
        ROW_HIP(hipMemcpy(&r, d_ratio, sizeof r, hipMemcpyDeviceToHost));
        ROW_HIP(hipMemcpy(pend_shot_pose, d_pose, sizeof pend_shot_pose, hipMemcpyDeviceToHost));
        tm.handoff_bytes[SFMX_SFM_ROW_REGISTER] += 16 + 4 + 8 + 96;
        if (status == 1) { *ratio = r; pend_shot = shot; }
        return status;
    }

    int accept_shot(int32_t shot) {
        if (pend_shot != shot) { set_last_error("a pose accepted without its registration"); return SFMX_ESTATE; }
        std::memcpy(&pose[12 * (size_t)shot], pend_shot_pose, sizeof pend_shot_pose);
        pend_shot = -1;
        return 0;
    }

    // the cloud on the host: for the adjustment and for the caller's buffers
    int fetch_cloud(double* xyz, int64_t* oo, int32_t* osh, double* oxy) {
        if (n_points) ROW_HIP(hipMemcpy(xyz, c_xyz[cur], sizeof(double) * 3 * n_points, hipMemcpyDeviceToHost));
        ROW_HIP(hipMemcpy(oo, c_oo[cur], sizeof(int64_t) * (n_points + 1), hipMemcpyDeviceToHost));
        if (n_rec) {
            ROW_HIP(hipMemcpy(osh, c_osh[cur], sizeof(int32_t) * n_rec, hipMemcpyDeviceToHost));
            ROW_HIP(hipMemcpy(oxy, c_oxy[cur], sizeof(double) * 2 * n_rec, hipMemcpyDeviceToHost));
        }
        return SFMX_OK;
    }

    int bundle_adjust(int32_t* iterations, int32_t* termination) {
        *iterations = 0;
        *termination = -1;
        if (n_points == 0 || n_rec == 0) return 0;   // an empty cloud: nothing to adjust
        std::vector<int32_t> op((size_t)n_rec), oc((size_t)n_rec), osh((size_t)n_rec), pose_of_shot((size_t)n_shots), shot_of_pose((size_t)n_shots);
        std::vector<double> ox(2 * (size_t)n_rec), oxy(2 * (size_t)n_rec), pts(3 * (size_t)n_points), poses6;
        std::vector<int64_t> oo((size_t)n_points + 1);
        double intr[7];
        int32_t n_poses = 0;
        sfmx_ba_problem pb{};
        {
            Clock c(*this, SFMX_SFM_ROW_HANDOFF);
            int rc = fetch_cloud(pts.data(), oo.data(), osh.data(), oxy.data());   // CeresPCE::read
            if (rc < 0) return rc;
            tm.handoff_bytes[SFMX_SFM_ROW_BA] += n_points * 24 + (n_points + 1) * 8 + n_rec * (4 + 16);
            rc = sfmx_ba_observations_from_origins(oo.data(), (int32_t)n_points, osh.data(), oxy.data(), n_shots, op.data(), oc.data(),
                                                   ox.data(), pose_of_shot.data(), shot_of_pose.data(), &n_poses);
            if (rc < 0) return rc;
            if (n_poses < 0 || n_poses > n_shots) { set_last_error("adjustment: pose count self check failed"); return SFMX_EINTERNAL; }
            poses6.resize(6 * (size_t)n_poses);
            for (int i = 0; i < n_poses; ++i) {
                const int32_t s = shot_of_pose[i];
                if (s < 0 || s >= n_shots) { set_last_error("adjustment: shot of a pose out of range"); return SFMX_EINTERNAL; }
                sfmx_pose_to_ceres(&pose[12 * (size_t)s], &poses6[6 * (size_t)i]);   // CeresCameraShot::read
            }
            // ceresCameraParameters(true): getFocalLength is fx, or the mean where fx != fy (ICamera.cpp:62-66)
            const double f = cam.K[0] == cam.K[4] ? cam.K[0] : (cam.K[0] + cam.K[4]) / 2.0;
            intr[0] = f;
            if (cam_model == SFMX_CAM_SIMPLE_RADIAL) { intr[1] = cam.dist[0]; intr[2] = cam.dist[1]; }
            if (cam_model == SFMX_CAM_DISTORTION) {
                intr[1] = cam.K[2]; intr[2] = cam.K[5];
                intr[3] = cam.dist[0]; intr[4] = cam.dist[1]; intr[5] = cam.dist[2]; intr[6] = cam.dist[3];
            }
            pb.n_points = (int32_t)n_points; pb.n_cams = n_poses; pb.n_obs = (int32_t)n_rec; pb.cam_model = cam_model;
            pb.points = pts.data(); pb.poses = poses6.data(); pb.intr = intr;
            pb.obs_point = op.data(); pb.obs_cam = oc.data(); pb.obs_xy = ox.data();
            pb.cx = cam.K[2]; pb.cy = cam.K[5];
        }
        sfmx_ba_options opt;
        sfmx_ba_default_options(&opt);
        opt.device = device;
        sfmx_ba_summary sm{};
        int rc;
        {
            Clock c(*this, SFMX_SFM_ROW_BA);
            rc = sfmx_ba_solve(&pb, &opt, &sm, nullptr, 0);
        }
        if (rc < 0) return rc;
        tm.device_ms[SFMX_SFM_ROW_BA] += sm.total_ms;
        {
            Clock c(*this, SFMX_SFM_ROW_HANDOFF);
            ROW_HIP(hipSetDevice(device));
            ROW_HIP(hipMemcpy(c_xyz[cur], pts.data(), sizeof(double) * 3 * n_points, hipMemcpyHostToDevice));   // CeresPCE::write
            tm.handoff_bytes[SFMX_SFM_ROW_BA] += n_points * 24;
            for (int i = 0; i < n_poses; ++i) sfmx_pose_from_ceres(&poses6[6 * (size_t)i], &pose[12 * (size_t)shot_of_pose[i]]);
            cam.K[0] = cam.K[4] = intr[0];   // ceresApplyParameters
            if (cam_model == SFMX_CAM_SIMPLE_RADIAL) { cam.dist[0] = intr[1]; cam.dist[1] = intr[2]; }
            if (cam_model == SFMX_CAM_DISTORTION) {
                cam.K[2] = intr[1]; cam.K[5] = intr[2];
                cam.dist[0] = intr[3]; cam.dist[1] = intr[4]; cam.dist[2] = intr[5]; cam.dist[3] = intr[6];
            }
        }
        *iterations = sm.num_successful_steps + sm.num_unsuccessful_steps;
        *termination = sm.termination_type;
        return 0;
    }
};

int row_relative_pose(void* u, int32_t p, int32_t* n) { Rows* r = static_cast<Rows*>(u); return r->note(r->relative_pose(p, n)); }
int row_triangulate_pair(void* u, int32_t p, int32_t initial, int32_t* n) { Rows* r = static_cast<Rows*>(u); return r->note(r->triangulate_pair(p, initial, n)); }
int row_add_elements(void* u, int32_t p, int32_t merge) { Rows* r = static_cast<Rows*>(u); return r->note(r->add_elements(p, merge)); }
int row_count_candidates(void* u, const int32_t* s, int32_t n, int32_t* c) { Rows* r = static_cast<Rows*>(u); return r->note(r->count_candidates(s, n, c)); }
int row_register_shot(void* u, int32_t s, double* r, int32_t* d, int32_t cap, int32_t* n) {
    Rows* rows = static_cast<Rows*>(u);
    return rows->note(rows->register_shot(s, r, d, cap, n));
}
int row_accept_shot(void* u, int32_t s) { Rows* r = static_cast<Rows*>(u); return r->note(r->accept_shot(s)); }
int row_bundle_adjust(void* u, int32_t* it, int32_t* term) { Rows* r = static_cast<Rows*>(u); return r->note(r->bundle_adjust(it, term)); }

}  // namespace

extern "C" {

int sfmx_sfm_default_params(sfmx_sfm_params* params) {
    if (!params) { set_last_error("null argument"); return SFMX_EINVAL; }
    sfm_host::default_params(*params);
    return SFMX_OK;
}

int sfmx_sfm_triangulate_steps(const sfmx_sfm_steps* steps, void* user, const sfmx_sfm_params* params, int32_t n_shots,
                               const int32_t* pairs, int32_t n_pairs, const int32_t* pair_n_matches,
                               const double* homography_ratio, int32_t* out_recovered, int32_t* out_pair_state,
                               int32_t* out_pair_n_matches, sfmx_sfm_event* trace, int64_t trace_capacity,
                               int64_t* out_n_events, sfmx_sfm_summary* summary) {
    if (!steps || !steps->relative_pose || !steps->triangulate_pair || !steps->add_elements || !steps->count_candidates ||
        !steps->register_shot || !steps->accept_shot || !steps->bundle_adjust) {
        set_last_error("null step");
        return SFMX_EINVAL;
    }
    if (const char* why = sfm_host::check_params(params)) { set_last_error(why); return SFMX_EINVAL; }
    if (const char* why = sfm_host::check_graph(n_shots, pairs, n_pairs, pair_n_matches, homography_ratio)) {
        set_last_error(why);
        return SFMX_EINVAL;
    }
    if ((n_shots && !out_recovered) || (n_pairs && !out_pair_state) || trace_capacity < 0 || (trace_capacity && !trace)) {
        set_last_error("null argument");
        return SFMX_EINVAL;
    }
    const int rc = sfm_host::triangulate_steps(*steps, user, *params, n_shots, pairs, n_pairs, pair_n_matches, homography_ratio,
                                               out_recovered, out_pair_state, out_pair_n_matches, trace, trace_capacity,
                                               out_n_events, summary);
    if (rc == SFMX_ECAPACITY) set_last_error("trace capacity too small");
    else if (rc == SFMX_EINTERNAL) set_last_error("a step returned a pair index or count out of range");
    else if (rc < 0) set_last_error("a step aborted the loop");
    return rc;
}

int sfmx_sfm_triangulate(const sfmx_point2f* const* keypoints, const int32_t* n_keypoints, int32_t n_shots,
                         const int32_t* shot_size, const sfmx_tri_camera* cameras, int32_t n_cameras,
                         int32_t camera_model, const int32_t* pairs, int32_t n_pairs, const sfmx_dmatch* matches,
                         const int64_t* pair_offsets, const double* homography_ratio, const sfmx_sfm_params* params,
                         int32_t device, int32_t* out_recovered, double* out_pose, sfmx_tri_camera* out_camera,
                         double* out_xyz, int64_t point_capacity, int64_t* out_origin_offsets,
                         int32_t* out_origin_shot, double* out_origin_xy, int64_t record_capacity,
                         int64_t* out_n_points, int64_t* out_n_records, sfmx_dmatch* out_matches,
                         int64_t* out_pair_offsets, int32_t* out_pair_state, sfmx_sfm_event* trace,
                         int64_t trace_capacity, int64_t* out_n_events, sfmx_sfm_summary* summary,
                         sfmx_sfm_timing* timing) {
    if (n_shots < 0 || n_pairs < 0 || n_cameras < 0) { set_last_error("negative count"); return SFMX_EINVAL; }
    if (n_cameras > 1) { set_last_error("more than one camera: the reconstruction loop adjusts a single intrinsics block"); return SFMX_ECAPACITY; }
    if (n_cameras == 0 || !cameras) { set_last_error("no camera"); return SFMX_EINVAL; }
    if (const char* why = sfm_host::check_params(params)) { set_last_error(why); return SFMX_EINVAL; }
    if (!pair_offsets || !out_n_points || !out_n_records || !out_origin_offsets || !out_pair_offsets || !out_camera ||
        (n_shots && (!keypoints || !n_keypoints || !shot_size || !out_recovered || !out_pose)) ||
        (n_pairs && (!pairs || !homography_ratio || !out_pair_state)) || trace_capacity < 0 || (trace_capacity && !trace)) {
        set_last_error("null argument");
        return SFMX_EINVAL;
    }
    if (camera_model != SFMX_CAM_SIMPLE && camera_model != SFMX_CAM_SIMPLE_RADIAL && camera_model != SFMX_CAM_DISTORTION) {
        set_last_error("unknown camera model");
        return SFMX_EINVAL;
    }
    if (cameras[0].K[0] == 0.0 || cameras[0].K[4] == 0.0) { set_last_error("camera with zero focal length"); return SFMX_EINVAL; }
    for (int s = 0; s < n_shots; ++s)
        if (n_keypoints[s] < 0 || (n_keypoints[s] && !keypoints[s])) { set_last_error("bad keypoint array"); return SFMX_EINVAL; }
    if (pair_offsets[0] != 0) { set_last_error("pair offsets do not start at 0"); return SFMX_EINVAL; }
    for (int p = 0; p < n_pairs; ++p)
        if (pair_offsets[p + 1] < pair_offsets[p] || pair_offsets[p + 1] - pair_offsets[p] > INT32_MAX) {
            set_last_error("pair offsets not ascending");
            return SFMX_EINVAL;
        }
    const int64_t M = pair_offsets[n_pairs];
    std::vector<int32_t> n_matches((size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) n_matches[p] = (int32_t)(pair_offsets[p + 1] - pair_offsets[p]);
    if (const char* why = sfm_host::check_graph(n_shots, pairs, n_pairs, n_matches.data(), homography_ratio)) {
        set_last_error(why);
        return SFMX_EINVAL;
    }
    if (M && (!matches || !out_matches || !out_xyz || !out_origin_shot || !out_origin_xy)) { set_last_error("null argument"); return SFMX_EINVAL; }
    if (point_capacity < M || record_capacity < 2 * M) { set_last_error("cloud capacity below the bound"); return SFMX_EINVAL; }
    for (int p = 0; p < n_pairs; ++p)
        for (int64_t i = pair_offsets[p]; i < pair_offsets[p + 1]; ++i)
            if (matches[i].queryIdx < 0 || matches[i].queryIdx >= n_keypoints[pairs[2 * p]] || matches[i].trainIdx < 0 ||
                matches[i].trainIdx >= n_keypoints[pairs[2 * p + 1]]) {
                set_last_error("match index outside its image's keypoints");
                return SFMX_EINVAL;
            }

    Rows R;
    R.kp = keypoints; R.nkp = n_keypoints; R.n_shots = n_shots; R.shot_size = shot_size;
    R.cam = cameras[0]; R.cam_model = camera_model; R.pairs = pairs; R.n_pairs = n_pairs; R.prm = *params; R.device = device;
    R.shot_camera.assign((size_t)std::max(n_shots, 1), 0);
    R.pose.assign(12 * (size_t)n_shots, std::numeric_limits<double>::quiet_NaN());
    {
        const int orc = R.open(matches, pair_offsets);
        if (orc != SFMX_OK) return orc;
    }
    const sfmx_sfm_steps steps = {row_relative_pose, row_triangulate_pair, row_add_elements, row_count_candidates,
                                  row_register_shot, row_accept_shot, row_bundle_adjust};
    const int rc = sfm_host::triangulate_steps(steps, &R, *params, n_shots, pairs, n_pairs, n_matches.data(), homography_ratio,
                                               out_recovered, out_pair_state, nullptr, trace, trace_capacity, out_n_events, summary);
    if (timing) *timing = R.tm;
    if (R.row_error || (rc < 0 && rc != SFMX_ECAPACITY)) return rc;   // a row's error, whatever its code: its text stands
    if (rc == SFMX_ECAPACITY) set_last_error("trace capacity too small");   // the loop finished: the outputs are complete
    if (R.n_points > point_capacity || R.n_rec > record_capacity || R.off[n_pairs] > M) { set_last_error("scene beyond its bound"); return SFMX_EINTERNAL; }
    std::copy(R.pose.begin(), R.pose.end(), out_pose);
    for (int s = 0; s < n_shots; ++s)
        if (!out_recovered[s]) std::fill(out_pose + 12 * (size_t)s, out_pose + 12 * (size_t)s + 12, std::numeric_limits<double>::quiet_NaN());
    *out_camera = R.cam;
    {
        const int frc = R.fetch_cloud(out_xyz, out_origin_offsets, out_origin_shot, out_origin_xy);
        if (frc < 0) return frc;
    }
    *out_n_points = R.n_points;
    *out_n_records = R.n_rec;
    if (R.off[n_pairs] && hipMemcpy(out_matches, R.d_m, sizeof(sfmx_dmatch) * R.off[n_pairs], hipMemcpyDeviceToHost) != hipSuccess) {
        set_last_error("HIP error fetching the match lists");
        return SFMX_EDEVICE;
    }
    std::copy(R.off.begin(), R.off.end(), out_pair_offsets);
    return rc;
}

}  // extern "C"
