/* SPDX-License-Identifier: MIT
 *
 * sfmx — triangulation of shot matches into 3D points (the row between the
 * match graph and the 3D-2D search / bundle adjustment).
 *
 * Replaces SfM::triangulateMatch(match, points)     src/photogrammetrie/sfm/SfM.cpp:383-451
 *   for one ShotMatches of two posed shots (called once per newly connected
 *   pair, SfM.cpp:220,356):
 *     aligned keypoints      left[queryIdx], right[trainIdx]                (:389-391, :407-408)
 *     cv::undistortPoints    per side, with the shot's camera K, distortion (:410-412)
 *     cv::triangulatePoints  with the two shots' 3x4 poses                  (:414-416)
 *     convertPointsFromHomogeneous                                          (:418-419)
 *     projectPoints          into both views                                (:422-426)
 *     keep rule              drop iff left or right reprojection error
 *                            > maxReprojectionError                         (:429-436)
 *     -> PointcloudElement(cv::Point3d(float X, Y, Z)) with one origin
 *        (left point, right point as cv::Point2d)                           (:438-445)
 * Here every pair of a match graph is triangulated in one call.  The
 * arithmetic is the project's operation-by-operation restatement of the
 * OpenCV 4.5.1 functions above (tests/tri_ref.py; DESIGN.md has the
 * algorithm).  Deviations from the reference, all documented in DESIGN.md:
 *   - the Jacobi SVD's hypot(p, beta) is sqrt(p*p + beta*beta) (no libm);
 *   - the reprojection uses the rotation R of `shot_pose` itself; the reference
 *     reprojects with Rodrigues(Rodrigues(R)) (CameraShot.cpp:96-100), a host
 *     libm round trip.  A caller that wants that round trip applies it to the
 *     pose it passes;
 *   - a NaN coordinate or error is emitted as the canonical quiet NaN.
 *
 * Status codes and threading as in sfmx.h.  Calls on one device are serialised
 * inside the library (they share that device's cached scratch); calls on
 * different devices run concurrently.  sfmx_triangulate_last_kernel_ms is per
 * calling thread.
 */
#ifndef SFMX_TRIANGULATE_H
#define SFMX_TRIANGULATE_H

#include <stdint.h>
#include "sfmx.h"
#include "sfmx_homography.h"   /* sfmx_point2f */

#ifdef __cplusplus
extern "C" {
#endif

/* ICamera::getK / ICamera::getDistortion of one camera. */
typedef struct sfmx_tri_camera {
    double K[9];      /* row-major; fx = K[0], fy = K[4], cx = K[2], cy = K[5] */
    double dist[5];   /* k1 k2 p1 p2 k3, the convention of sfmx_undistort_images */
} sfmx_tri_camera;

/* SfM.h:55: maxReprojectionError. */
#define SFMX_MAX_REPROJECTION_ERROR 10.0

/* Triangulate every match of a match graph between posed shots.
 *   keypoints     n_shots pointers; shot i has n_keypoints[i] points
 *   cameras       n_cameras cameras; shot i uses cameras[shot_camera[i]]
 *   shot_pose     12 * n_shots doubles: CameraShot::getPose, 3x4 [R|t] row-major
 *   pairs         2 * n_pairs (left, right) shot indices
 *   matches       packed DMatch lists, pair p at [pair_offsets[p], pair_offsets[p+1])
 *                 (the layout sfmx_matcher_fetch / sfmx_matcher_device_results return);
 *                 n_matches = pair_offsets[n_pairs]
 *   max_reprojection_error   a match is dropped iff its left or right error is
 *                 greater; a NaN error therefore keeps the point (the reference's
 *                 comparison)
 * Outputs (capacities in elements; n_points = *out_n_points are written):
 *   out_point_offsets  n_pairs + 1: the points of pair p are [off[p], off[p+1])
 *   out_xyz            3 * n_matches: cv::Point3d(float X, float Y, float Z)
 *   out_match          n_matches: index into `matches` of each kept point
 *   out_origin_shot    2 * n_matches: left, right shot of each point
 *   out_origin_xy      4 * n_matches: left point, right point as cv::Point2d
 *   out_err            optional (NULL ok), 2 * n_matches: left, right reprojection
 *                      error of every MATCH (uncompacted, dropped ones included)
 *   out_n_points       host memory, always: number of points kept
 * Points come out pair-major in `pairs` order and in match-list order within a
 * pair (the reference's push_back order).  Every point has one origin of two
 * records, left then right, at records 2i and 2i + 1: with origin_offsets[i] =
 * 2 * i (i = 0 .. n_points) out_origin_shot / out_origin_xy are the origin CSR
 * of sfmx_scene.h and go into sfmx_find_3d2d_matches and
 * sfmx_ba_observations_from_origins unchanged.
 * inputs_on_device = 0: every pointer is host memory.  1: keypoints[i], matches,
 * pair_offsets and every out_* array except out_n_points are device pointers on
 * `device`, and the caller guarantees the capacities above; the small arrays
 * (n_keypoints, cameras, shot_camera, shot_pose, pairs) are always host memory.
 * SFMX_EINVAL: a shot_camera outside [0, n_cameras), fx == 0 or fy == 0, a pair
 * shot outside [0, n_shots), offsets that do not ascend from 0, a queryIdx /
 * trainIdx outside its image's keypoints.  With device inputs the match indices
 * are checked in the kernel and reported after it ran: the out_* arrays are then
 * unspecified.
 * Replaces: SfM::triangulateMatch, SfM.cpp:383-451. */
int sfmx_triangulate_matches(const sfmx_point2f* const* keypoints, const int32_t* n_keypoints, int32_t n_shots,
                             const sfmx_tri_camera* cameras, int32_t n_cameras, const int32_t* shot_camera,
                             const double* shot_pose, const int32_t* pairs, int32_t n_pairs,
                             const sfmx_dmatch* matches, const int64_t* pair_offsets, double max_reprojection_error,
                             int32_t inputs_on_device, int32_t device, void* stream, int64_t* out_point_offsets,
                             double* out_xyz, int64_t* out_match, int32_t* out_origin_shot, double* out_origin_xy,
                             double* out_err, int64_t* out_n_points);

/* Device time (ms) of the kernels of the last sfmx_triangulate_matches call on
 * this thread (HIP events on its stream); 0 when the call had no match and
 * launched nothing, -1 before any call. */
float sfmx_triangulate_last_kernel_ms(void);

#ifdef __cplusplus
}
#endif

#endif /* SFMX_TRIANGULATE_H */
