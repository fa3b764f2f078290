/* SPDX-License-Identifier: MIT
 *
 * sfmx — registration pose of a new shot (row f8: between the 3D-2D search and
 * the relative poses of the pairs that connect the registered shot).
 *
 * Replaces
 * SfM::findCameraPoseFrom3d2dMatch(match, inlierRatio)  src/photogrammetrie/sfm/SfM.cpp:453-489
 *     distinct points      ShotMatches3d2d::getDistinct3d2dPoints   (:459)   common/Scene.cpp:264-278
 *     threshold            ransacReprojectionPoseThreshold: < 0: -t pixels;
 *                          > 0: t * max(width, height) of the shot           (:469-473)
 *     cv::solvePnPRansac   (points3d, points2d, K, dist, rvec, tvec, false,
 *                          100, thr, 0.99, inliers)                          (:477)
 *     inlier ratio         cv::countNonZero(inliers) / points                (:479)
 * for any number of candidate sets in one call (the reference finds the 3D-2D
 * matches of all remaining shots, SfM.cpp:278-282, and poses the best one).
 * The arithmetic is the project's operation-by-operation restatement of the
 * OpenCV 4.5.1 functions above (tests/pnp_ref.py; DESIGN.md §8i has the
 * algorithm).  What is built and what is not, all documented in DESIGN.md §8i:
 *   - built: both conversions to float, the threshold through its float
 *     parameter, RANSACPointSetRegistrator on 5-point samples (cv::RNG stream,
 *     getSubset, strict acceptance, RANSACUpdateNumIters), undistortPoints +
 *     EPnP with the identity camera matrix per sample, the float reprojection
 *     error, the final inlier mask, and the ratio with the reference's quirk
 *     (`inliers` is an index list, so an inlier with index 0 is not counted);
 *   - built: the final solvePnP(SOLVEPNP_ITERATIVE) refit on the inliers
 *     (cvFindExtrinsicCameraParams2): the planarity test on the inliers'
 *     covariance, the DLT start from the 12x12 L^T L, CvLevMarq on (rvec, tvec)
 *     (at most 20 iterations, FLT_EPSILON on the relative step, lambda from 1e-3
 *     by factors of 10 inside [1e-16, 1e16]) with cvProjectPoints2's analytic
 *     Jacobian.  It needs sin, cos and acos, so out_pose agrees with the
 *     restatement within a tolerance, not as bits; everything else is bit-exact;
 *   - NOT built: P3P for exactly 4 points.  Such a set has status 2: "fall back
 *     to the host".
 * Deviations from OpenCV inside the built part:
 *   - EPnP's cvSVD / cvInvert / cvSolve are replaced by deterministic, libm-free
 *     routines: cyclic Jacobi rotations for the symmetric 3x3 and 12x12, the
 *     pseudo-inverse of the 3x3 control matrix through its eigenpairs (OpenCV:
 *     cvInvert(CV_SVD)), epnp's own Householder qr_solve
 *     for every 6 x k least-squares system (OpenCV: cvSolve(CV_SVD) for the three
 *     approximations), the one-sided Jacobi of the triangulation for the 3x3
 *     SVD of the absolute orientation.  A coplanar sample (eigenvalue ratio
 *     under 1e-12) is solved with three control points (EPnP's case N = 1);  The solutions agree up to rounding, so
 *     an inlier at the threshold's edge can differ;
 *   - the model keeps R between EPnP and the projection (OpenCV:
 *     Rodrigues(Rodrigues(R))), as in DESIGN.md §8f: the stage needs no
 *     trigonometry;
 *   - the refit of a planar inlier set starts from the RANSAC's best EPnP model
 *     (OpenCV: a homography decomposition); out_refit_start says which start was
 *     used.  The augmented normal equations are solved by pivoted elimination
 *     (OpenCV: SVD), lambda's powers of ten are exact literals (OpenCV: exp), the
 *     matrix -> vector Rodrigues skips OpenCV's re-orthonormalisation, and every
 *     sum over the inliers has a fixed tree order;
 *   - getSubset's redraw loop is bounded by 10000 values; with 5 points the
 *     sample is the list itself and nothing is drawn;
 *   - the log of RANSACUpdateNumIters is the device's (as in sfmx_homography.h);
 *   - a set the reference would throw cv::Exception for (fewer than 4 points,
 *     no model, a failing refit: OpenCV's DLT needs 6 points) has status 0; the
 *     reference's Rodrigues / hconcat of the result (:481-485) is out_pose.
 *
 * Status codes and threading as in sfmx.h.  Calls on one device are serialised
 * inside the library; the *_last_kernel_ms values are per calling thread.
 */
#ifndef SFMX_PNP_H
#define SFMX_PNP_H

#include <stdint.h>
#include "sfmx.h"
#include "sfmx_triangulate.h"   /* sfmx_tri_camera */

#ifdef __cplusplus
extern "C" {
#endif

/* What SfM.cpp:477 passes (solvePnPRansac's defaults). */
#define SFMX_PNP_CONFIDENCE 0.99
#define SFMX_PNP_MAX_ITERS 100

/* ShotMatches3d2d::getDistinct3d2dPoints on the output of
 * sfmx_find_3d2d_matches: the distinct (cv::Point3d, cv::Point2d) list.
 *   cloud_xyz        3 * n_points doubles
 *   origin_offsets   n_points + 1: the origin CSR sfmx_find_3d2d_matches was given
 *   found_keypoint   its out_keypoint (one per origin record, -1: no match)
 *   found_xy         its out_xy (2 floats per record)
 * A record with a match is dropped iff an earlier record with a match has ==
 * coordinates in all five doubles (on coordinates, not on point indices;
 * -0 == +0, a NaN never equals anything).  The order is first-appearance order
 * over the point-major records (the reference's order comes from an
 * `omp critical` push and is open).
 *   out_xyz, out_xy  capacity 3 * / 2 * origin_offsets[n_points] doubles
 *   out_n            host memory, always: the number of distinct points
 * inputs_on_device = 1: cloud_xyz, origin_offsets, found_* and out_xyz / out_xy
 * are device pointers on `device`.  A host call without records touches no device.
 * SFMX_EINVAL: a null argument, a negative count, offsets that do not ascend
 * from 0. */
int sfmx_distinct_3d2d_points(const double* cloud_xyz, int32_t n_points, const int64_t* origin_offsets,
                              const int32_t* found_keypoint, const float* found_xy, int32_t inputs_on_device,
                              int32_t device, void* stream, double* out_xyz, double* out_xy, int64_t* out_n);

/* findCameraPoseFrom3d2dMatch for n_sets candidate sets.
 *   points3d, points2d   3 * / 2 * set_offsets[n_sets] doubles (Point3d / Point2d,
 *                        as sfmx_distinct_3d2d_points delivers them)
 *   set_offsets          n_sets + 1: set s is [off[s], off[s+1])
 *   set_shot             n_sets: the shot each set would register (host memory)
 *   cameras, n_cameras, shot_camera, shot_size, n_shots
 *                        as in sfmx_relative_poses (host memory)
 *   threshold            ransacReprojectionPoseThreshold (sfmx_cli_config.
 *                        ransac_pose_threshold, default -8): < 0 means -threshold
 *                        pixels, > 0 that fraction of max(width, height)
 *   confidence           in (0, 1); SFMX_PNP_CONFIDENCE
 *   max_iters            >= 1; SFMX_PNP_MAX_ITERS
 * Outputs (n = set_offsets[n_sets]):
 *   out_status        n_sets: 1 a pose was found; 0 the reference would throw or
 *                     finds no model; 2 exactly 4 points (P3P, not built)
 *   out_pose          12 * n_sets: hconcat(R, t) after the refit, 3x4 row-major
 *                     (the layout of shot_pose); with exactly 5 points the EPnP
 *                     pose of the list
 *   out_ransac_pose   12 * n_sets: the RANSAC's best EPnP model, same layout
 *   out_refit_start   n_sets: 0 the refit started from the DLT, 1 from the EPnP
 *                     model (planar inliers), -1 no refit (5 points, status 0 / 2)
 *   out_mask          n bytes: the RANSAC inlier mask
 *   out_n_inliers     n_sets: the honest mask count
 *   out_inlier_ratio  n_sets: (n_inliers - mask[0]) / points, the value
 *                     SfM.cpp:311 tests; -1 for status 0 and 2
 * A status-0 or status-2 set has a zero mask and canonical quiet NaN poses.
 * inputs_on_device = 0: every pointer is host memory.  1: points3d, points2d,
 * set_offsets and every out_* array are device pointers on `device`.  An empty
 * call (no set, or no point in any set) launches nothing and with host inputs
 * touches no device.
 * SFMX_EINVAL: a null argument, a negative count, offsets that do not ascend
 * from 0, a set_shot outside [0, n_shots), a shot_camera outside [0, n_cameras),
 * fx == 0 or fy == 0, threshold 0 or NaN, confidence outside (0, 1),
 * max_iters < 1.
 * Replaces: SfM::findCameraPoseFrom3d2dMatch, SfM.cpp:453-489. */
int sfmx_register_poses(const double* points3d, const double* points2d, const int64_t* set_offsets,
                        const int32_t* set_shot, int32_t n_sets, const sfmx_tri_camera* cameras, int32_t n_cameras,
                        const int32_t* shot_camera, const int32_t* shot_size, int32_t n_shots, double threshold,
                        double confidence, int32_t max_iters, int32_t inputs_on_device, int32_t device, void* stream,
                        int32_t* out_status, double* out_pose, double* out_ransac_pose, uint8_t* out_mask,
                        int32_t* out_n_inliers, double* out_inlier_ratio, int32_t* out_refit_start);

/* Device time (ms) of the kernels of the last call on this thread (HIP events on
 * its stream); 0 when the call launched nothing, -1 before any call. */
float sfmx_register_poses_last_kernel_ms(void);
float sfmx_distinct_3d2d_last_kernel_ms(void);

#ifdef __cplusplus
}
#endif

#endif /* SFMX_PNP_H */
