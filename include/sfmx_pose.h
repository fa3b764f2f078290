/* SPDX-License-Identifier: MIT
 *
 * sfmx — relative pose of shot matches (row f7: between the homography ratio
 * and the triangulation of a posed pair).
 *
 * Replaces SfM::findCameraPoseFromMatch(match)       src/photogrammetrie/sfm/SfM.cpp:491-540
 *   for one ShotMatches (called for every candidate initial pair, SfM.cpp:202,
 *   and for every pair that connects a newly registered shot, SfM.cpp:345):
 *     aligned keypoints      left[queryIdx], right[trainIdx]                 (:497-512)
 *     threshold              < 0: -t pixels; > 0: t * max(leftW, leftH,
 *                            rightH, rightH) — never the right width         (:515-521)
 *     cv::findEssentialMat   (left, right, K_L, dist_L, K_R, dist_R,
 *                            cv::RANSAC, 0.999, thr, mask)                   (:523-525)
 *     cv::recoverPose        (E, left, right, K_L, R, t, mask)               (:527-528)
 *     inlier DMatches        the matches whose mask byte survived both       (:530-537)
 *   and the caller's setMatches(inlierMatches)                               (:213, :350)
 * Here every pair of a match graph is posed in one call.  The arithmetic is the
 * project's operation-by-operation restatement of the OpenCV 4.5.1 functions
 * above (tests/pose_ref.py; DESIGN.md §8h has the algorithm).  Deviations from
 * the reference, all documented in DESIGN.md §8h:
 *   - the five-point solver's null space comes from Gauss-Jordan elimination
 *     with complete pivoting (OpenCV: full-UV Jacobi SVD, completed with random
 *     vectors), its real roots from derivative bracketing and bisection
 *     (OpenCV: solvePoly, Durand-Kerner), x and y from a cross product of two
 *     rows of B(z); E is divided by its Frobenius norm.  The solutions are the
 *     same up to rounding, so an inlier at the threshold's edge can differ;
 *   - the two-camera overload's points return to float pixels through the mean
 *     camera matrix in one rounding per coordinate;
 *   - decomposeEssentialMat's SVD is the one-sided Jacobi of the triangulation
 *     with hypot restated as sqrt(p*p + beta*beta); U's third column is the
 *     cross product of the first two;
 *   - getSubset's redraw loop is bounded by 10000 values;
 *   - with 5 matches the sample is the list itself and nothing is drawn;
 *   - the log of RANSACUpdateNumIters is the device's (as in sfmx_homography.h);
 *   - a pair the reference would throw cv::Exception for (fewer than 5
 *     matches, no model) has status 0, and its E and pose are the canonical
 *     quiet NaN.
 * solvePnPRansac (findCameraPoseFrom3d2dMatch, SfM.cpp:453-489) is row f8:
 * sfmx_register_poses in sfmx_pnp.h.
 *
 * Status codes and threading as in sfmx.h.  Calls on one device are serialised
 * inside the library; sfmx_relative_poses_last_kernel_ms is per calling thread.
 */
#ifndef SFMX_POSE_H
#define SFMX_POSE_H

#include <stdint.h>
#include "sfmx.h"
#include "sfmx_homography.h"    /* sfmx_point2f */
#include "sfmx_triangulate.h"   /* sfmx_tri_camera */

#ifdef __cplusplus
extern "C" {
#endif

/* SfM.cpp:524 and RANSACPointSetRegistrator's default. */
#define SFMX_POSE_CONFIDENCE 0.999
#define SFMX_POSE_MAX_ITERS 1000

/* findCameraPoseFromMatch for every pair of a match graph.
 *   keypoints, n_keypoints, n_shots, cameras, n_cameras, shot_camera
 *                 as in sfmx_triangulate_matches
 *   shot_size     2 * n_shots: width, height of every shot's image
 *   pairs, n_pairs, matches, pair_offsets
 *                 the packed match graph, as in sfmx_triangulate_matches
 *   threshold     ransacReprojectionBaselineThreshold: < 0 means -threshold
 *                 pixels, > 0 that fraction of max(leftW, leftH, rightH, rightH)
 *   confidence    in (0, 1); SFMX_POSE_CONFIDENCE
 *   max_iters     >= 1; SFMX_POSE_MAX_ITERS
 * Outputs (n_matches = pair_offsets[n_pairs]):
 *   out_status            n_pairs: 1 the pose was found, 0 the reference would
 *                         throw (the caller `continue`s)
 *   out_E                 9 * n_pairs: the essential matrix, row-major
 *   out_pose              12 * n_pairs: hconcat(R, t), 3x4 row-major (the layout
 *                         of shot_pose)
 *   out_mask              n_matches bytes: the mask after recoverPose
 *   out_n_ransac_inliers  n_pairs: the mask count after findEssentialMat
 *   out_n_inliers         n_pairs: the count after recoverPose (its ratio to the
 *                         list length is poseInliersRatio, SfM.cpp:207)
 *   out_matches           n_matches capacity: the inlier DMatches, pair-major,
 *                         in list order within a pair
 *   out_pair_offsets      n_pairs + 1: pair p's inliers are [off[p], off[p+1]);
 *                         out_matches / out_pair_offsets go into
 *                         sfmx_triangulate_matches unchanged
 * A status-0 pair has an all-zero mask, an empty list and NaN E / pose.
 * inputs_on_device = 0: every pointer is host memory.  1: keypoints[i], matches,
 * pair_offsets and every out_* array are device pointers on `device`; the small
 * arrays (n_keypoints, cameras, shot_camera, shot_size, pairs) are host memory.
 * A host call without a match touches no device.
 * SFMX_EINVAL: a null argument, a negative count, a shot_camera outside
 * [0, n_cameras), fx == 0 or fy == 0, a pair shot outside [0, n_shots), offsets
 * that do not ascend from 0, threshold 0 or NaN, confidence outside (0, 1),
 * max_iters < 1, a queryIdx / trainIdx outside its image's keypoints.  With
 * device inputs the match indices are checked in the kernel and reported after
 * it ran: the out_* arrays are then unspecified.
 * Replaces: SfM::findCameraPoseFromMatch, SfM.cpp:491-540. */
int sfmx_relative_poses(const sfmx_point2f* const* keypoints, const int32_t* n_keypoints, int32_t n_shots,
                        const sfmx_tri_camera* cameras, int32_t n_cameras, const int32_t* shot_camera,
                        const int32_t* shot_size, const int32_t* pairs, int32_t n_pairs,
                        const sfmx_dmatch* matches, const int64_t* pair_offsets, double threshold,
                        double confidence, int32_t max_iters, int32_t inputs_on_device, int32_t device,
                        void* stream, int32_t* out_status, double* out_E, double* out_pose, uint8_t* out_mask,
                        int32_t* out_n_ransac_inliers, int32_t* out_n_inliers, sfmx_dmatch* out_matches,
                        int64_t* out_pair_offsets);

/* Device time (ms) of the kernels of the last sfmx_relative_poses call on this
 * thread (HIP events on its stream); 0 when the call launched nothing, -1
 * before any call. */
float sfmx_relative_poses_last_kernel_ms(void);

#ifdef __cplusplus
}
#endif

#endif /* SFMX_POSE_H */
