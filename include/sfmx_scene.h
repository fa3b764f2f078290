/* SPDX-License-Identifier: MIT
 *
 * sfmx — scene bookkeeping around bundle adjustment:
 * the 3D-2D correspondence search for a new shot and the construction of the
 * Ceres problem's observation arrays from the point cloud.
 *
 * Point-cloud origins are passed flattened, one record per distinct (shot,
 * 2-D point) of PointcloudElement::getOriginPoints (common/Scene.cpp:162-185,
 * first-appearance order, left point before right point of every origin),
 * as a CSR over points:
 *     origin_offsets[n_points + 1], origin_shot[n_origins], origin_xy[2 * n_origins] (double, cv::Point2d)
 * Shot matches are the packed lists of sfmx.h (pairs[2 * n_pairs] = (left,
 * right) shot indices in Scene::getShotMatches() order, matches, pair_offsets).
 *
 * Status codes and threading as in sfmx.h.
 */
#ifndef SFMX_SCENE_H
#define SFMX_SCENE_H

#include <stdint.h>
#include "sfmx.h"
#include "sfmx_homography.h"   /* sfmx_point2f */

#ifdef __cplusplus
extern "C" {
#endif

/* Scene::find3d2dMatches(ShotMatches3d2d&) (common/Scene.cpp:369-424) for the
 * new shot `shot`: for every origin record (point p, origin shot o, 2-D point q)
 * with o != shot, the FIRST shot-match pair in list order joining {shot, o}
 * (:389-394), then the FIRST DMatch in that pair's list whose keypoint on o's
 * side has cv::Point2d(kp.pt) == q (:396-405); the 3D-2D match is the keypoint
 * on `shot`'s side (:407-411).
 *   out_keypoint[i]  keypoint index in `shot` matched through origin record i, -1 if none
 *   out_pair[i]      index of the shot-match pair used, -1 if none
 *   out_xy[2i]       that keypoint's position (cv::KeyPoint::pt), NaN if none (may be NULL)
 * The reference appends matches under `omp critical` in a nondeterministic
 * order; here they are reported per origin record (point-major), which keys
 * parity by (point, origin).
 * SFMX_EINVAL: `shot` or a pair shot outside [0, n_shots), a negative keypoint count,
 * pair offsets that do not ascend from 0, an origin record count that is negative or
 * beyond 2^39, matches NULL with a non-empty list, (host) a match index outside its
 * image's keypoints in a pair that is read (the pairs and checks of
 * sfmx_count_3d2d_matches for the one candidate `shot`), 2^31 matches or more in the
 * pairs that are read or one list of more than 2^29.
 * The device block of a call is kept for the next one; calls of this function and of
 * sfmx_count_3d2d_matches on one device take turns.
 * inputs_on_device = 1: keypoints[i], matches, pair_offsets, origin_* and the
 * out_* arrays are device pointers on `device`; pairs is host memory always;
 * 0: host memory. */
int sfmx_find_3d2d_matches(const sfmx_point2f* const* keypoints, const int32_t* n_keypoints, int32_t n_shots,
                           const int32_t* pairs, int32_t n_pairs, const sfmx_dmatch* matches,
                           const int64_t* pair_offsets, const int64_t* origin_offsets, int32_t n_points,
                           const int32_t* origin_shot, const double* origin_xy, int32_t shot,
                           int32_t inputs_on_device, int32_t device, void* stream, int32_t* out_keypoint,
                           int32_t* out_pair, float* out_xy);

/* Device time (ms) of the last sfmx_find_3d2d_matches call on this thread
 * (table build + lookup kernels, HIP events on its stream); -1 before any call. */
float sfmx_find_3d2d_last_kernel_ms(void);

/* The candidate ranking of SfM::triangulate (sfm/SfM.cpp:276-300): the reference runs
 * Scene::find3d2dMatches for every remaining shot and keeps the list sizes.  Here all
 * candidates are counted in one call: one table build and one probe pass over the
 * origin records.
 *   pair_active[n_pairs]      a pair with 0 is invisible to the search; NULL: all visible
 *   candidates[n_candidates]  shot indices, each at most once
 *   out_count[c]              the number of origin records for which
 *                             sfmx_find_3d2d_matches(shot = candidates[c]) over the visible
 *                             pairs reports out_keypoint >= 0
 * The tables are those of sfmx_find_3d2d_matches: for a candidate s and another shot o,
 * the FIRST visible pair in list order joining {s, o}, keyed on the exact float bits of
 * the keypoint position on o's side (-0 keyed as +0, NaN never matches), value the
 * smallest match index.
 * SFMX_EINVAL: a candidate or pair shot outside [0, n_shots), a candidate listed twice,
 * pair or (host) origin offsets that do not ascend from 0, (host) a match index outside
 * its image's keypoints in a pair that is read.  SFMX_ECAPACITY: 2^31 matches or more
 * in the tables of one call (count the candidates in several calls), or one list of
 * more than 2^29 matches.
 * n_candidates == 0 writes nothing and touches no device.
 * inputs_on_device = 1: keypoints[i], matches, pair_offsets, origin_* and out_count are
 * device pointers on `device`; pairs, pair_active and candidates are host memory always. */
int sfmx_count_3d2d_matches(const sfmx_point2f* const* keypoints, const int32_t* n_keypoints, int32_t n_shots,
                            const int32_t* pairs, int32_t n_pairs, const int32_t* pair_active,
                            const sfmx_dmatch* matches, const int64_t* pair_offsets, const int64_t* origin_offsets,
                            int32_t n_points, const int32_t* origin_shot, const double* origin_xy,
                            const int32_t* candidates, int32_t n_candidates, int32_t inputs_on_device, int32_t device,
                            void* stream, int32_t* out_count);

/* Device time (ms) of the last sfmx_count_3d2d_matches call on this thread (table
 * build + count kernels, HIP events on its stream); 0 for n_candidates == 0, -1 before any call. */
float sfmx_count_3d2d_last_kernel_ms(void);

/* BundleAdjustment::doBundleAdjustment(const Scene&, ...)'s problem assembly
 * (common/BundleAdjustment.cpp:50-91) as flat sfmx_ba_problem arrays: one
 * observation per origin record, in point order then origin order (the
 * AddResidualBlock order); the camera-pose block of a shot is created on its
 * first appearance (the OpenMpUtils::find_if over ceresShots, :64-79, made
 * O(1) by a shot -> pose table).  The observation is the cv::Point2f the
 * cost function receives (ICamera::ceresCostFunction(const cv::Point2f&),
 * ICamera.h:161), stored as double.
 *   obs_point[n_origins], obs_cam[n_origins], obs_xy[2 * n_origins]
 *   pose_of_shot[n_shots]  pose index of each shot (-1: not observed)
 *   shot_of_pose[n_shots]  inverse (first *n_poses entries valid)
 * Host memory only (O(n_origins) host work). */
int sfmx_ba_observations_from_origins(const int64_t* origin_offsets, int32_t n_points, const int32_t* origin_shot,
                                      const double* origin_xy, int32_t n_shots, int32_t* obs_point, int32_t* obs_cam,
                                      double* obs_xy, int32_t* pose_of_shot, int32_t* shot_of_pose, int32_t* n_poses);

#define SFMX_POINT_MERGE_DISTANCE   0.01   /* SfM.h:56 */
#define SFMX_FEATURE_MERGE_DISTANCE 20.0   /* SfM.h:57 */

/* The merge loop of SfM.cpp:354-363: Scene::mergePointcloudElement3d2d(element,
 * pointMergeDistance, featureMergeDistance) (common/Scene.cpp:470-567) for the
 * n_new elements in index order, the cloud growing as it goes.  Cloud and new
 * elements are origin CSRs as above (sfmx_triangulate_matches' output is the
 * case new_origin_offsets = 2 * arange).  For element e:
 *   near    (:482-485)  cloud point c is a candidate iff !(d > point_merge_distance),
 *                       d = cv::norm(c - e) = sqrt((dx*dx + dy*dy) + dz*dz) in double,
 *                       so a NaN distance is a candidate; points appended earlier
 *                       in the call are cloud points;
 *   linked  (:498-545)  c qualifies iff for a record (s_e, q_e) of e and a record
 *                       (s_c, q_c) c holds at that moment, s_e != s_c, the FIRST pair
 *                       in list order joining {s_e, s_c} in either orientation has a
 *                       DMatch with cv::Point2d(kp_left[queryIdx]) == the left shot's
 *                       record, cv::Point2d(kp_right[trainIdx]) == the right shot's
 *                       record and fabsf(distance) <= feature_merge_distance
 *                       (match indices out of range never match);
 *   best    (:532-538)  fold over the qualifying candidates in ascending index with
 *                       `best == -1 || best > d` (the reference's single-thread order;
 *                       its OpenMP order leaves ties open);
 *   apply   (:552-567)  no winner: e is appended as given; winner c: each record of e,
 *                       in order, is appended to c's list unless c already holds an
 *                       equal (shot, xy) record (double ==; a NaN record is always
 *                       appended) — PointcloudElement::addOrigin (:205-214) restated
 *                       on origin points.
 * Outputs: old points keep their indices and their records come first, merged-in
 * records follow in merge order, appended elements follow in element order; the
 * result is again an origin CSR for sfmx_find_3d2d_matches,
 * sfmx_ba_observations_from_origins and the next merge.
 *   out_target[e]          cloud index the element ended in
 *   out_merge_distance[e]  distance to the point merged into (a NaN distance is the
 *                          canonical quiet NaN), -1.0 if appended
 *   out_xyz                capacity 3 * (n_cloud + n_new)
 *   out_origin_offsets     capacity n_cloud + n_new + 1 (first *out_n_points + 1 valid)
 *   out_origin_shot/_xy    capacity: cloud records + new records
 *   out_n_points, out_n_origins   host memory, always
 * The out_* arrays must not overlap the inputs (old records move within the CSR).
 * SFMX_EINVAL: a NaN merge distance, offsets that do not ascend from 0, an origin
 * or pair shot outside [0, n_shots), n_cloud + n_new beyond int32.  With host inputs
 * all of these are found on the host before any launch; with device inputs the two
 * origin offset arrays and the origin shots are checked by a kernel, the error is
 * returned after it and the outputs are unspecified.  n_new == 0 copies the cloud
 * through and, with host inputs, touches no device.  A hash table that fills up:
 * SFMX_EINTERNAL; more than 2^31 links among the new elements, 2^30 records in a
 * cloud or 2^29 matches: SFMX_ECAPACITY (merge the elements in several calls).
 * inputs_on_device = 1: keypoints[i], matches, pair_offsets, both clouds' arrays
 * and the out_* arrays except the two counts are device pointers on `device`;
 * 0: host memory.
 * The merge-or-append decisions and the record dedupe run on the device: the
 * decisions in rounds (an element is decided in the first round after all the
 * earlier elements it is linked to), one word read by the host per round.  In
 * device mode the host reads pair_offsets, the last entry of both origin offset
 * arrays and a few result words, and uploads its per-shot and per-pair tables:
 * nothing of either cloud, of the matches or of the links crosses.  A call that
 * still has undecided elements after the cap of
 * sfmx_merge_pointcloud_set_max_rounds finishes on the host instead, with the same
 * result: it then stages the per-element summaries, the link lists and, in device
 * mode, both clouds' coordinates and origin records. */
int sfmx_merge_pointcloud_3d2d(const sfmx_point2f* const* keypoints, const int32_t* n_keypoints, int32_t n_shots,
                               const int32_t* pairs, int32_t n_pairs, const sfmx_dmatch* matches,
                               const int64_t* pair_offsets, const double* cloud_xyz, int32_t n_cloud,
                               const int64_t* cloud_origin_offsets, const int32_t* cloud_origin_shot,
                               const double* cloud_origin_xy, const double* new_xyz, int32_t n_new,
                               const int64_t* new_origin_offsets, const int32_t* new_origin_shot,
                               const double* new_origin_xy, double point_merge_distance, double feature_merge_distance,
                               int32_t inputs_on_device, int32_t device, void* stream, int32_t* out_target,
                               double* out_merge_distance, double* out_xyz, int64_t* out_origin_offsets,
                               int32_t* out_origin_shot, double* out_origin_xy, int32_t* out_n_points,
                               int64_t* out_n_origins);

/* Device time (ms) of the last sfmx_merge_pointcloud_3d2d call on this thread
 * (validation, table build + probe, link fill, scans, resolve rounds, dedupe and
 * scatter kernels, HIP events on its stream; the copies and, after a fallback, the
 * host resolution between them are not in it); 0 for n_new == 0, -1 before any call. */
float sfmx_merge_pointcloud_last_kernel_ms(void);

/* The cap on the resolve rounds of this thread's later sfmx_merge_pointcloud_3d2d
 * calls: 0 the library default, > 0 that cap, < 0 no device
 * resolution: the host resolution always.  The results do not depend on it. */
int sfmx_merge_pointcloud_set_max_rounds(int32_t max_rounds);

/* About the last sfmx_merge_pointcloud_3d2d call on this thread (any pointer may be
 * NULL; zeros before any call): the resolve rounds it launched, 1 if the host
 * resolution decided its result (the cap was reached, or a negative setting), and
 * every byte it copied host to device or device to host, the pinned table upload
 * included. */
int sfmx_merge_pointcloud_last_path(int32_t* rounds, int32_t* host_fallback, int64_t* host_bytes);

/* Counts of the last sfmx_merge_pointcloud_3d2d call on this thread (any pointer
 * may be NULL): merges whose winner qualifies through a record it held when the
 * call started (static), merges whose winner qualifies only through a record merged
 * in earlier in the call or is a point appended in it (dynamic), and the links
 * found among the new elements. */
int sfmx_merge_pointcloud_last_stats(int64_t* merged_static, int64_t* merged_dynamic, int64_t* links);

#ifdef __cplusplus
}
#endif

#endif /* SFMX_SCENE_H */
