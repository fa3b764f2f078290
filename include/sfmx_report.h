/* SPDX-License-Identifier: MIT
 *
 * sfmx — the outputs of a sparse reconstruction (row f10): what
 * PhotogrammetrieCli::runSfM does after reconstructScene,
 * src/cli/PhotogrammetrieCli.cpp:115-132.
 *
 * Replaces Scene::colorizePointcloud                          src/photogrammetrie/common/Scene.cpp:569-617
 *          PclUtils::writeToPLY (cloud)                       src/photogrammetrie/util/PclUtils.cpp:401-460
 *          PclUtils::writeToPLY (cameras)                     PclUtils.cpp:466-590
 *          SceneUtils::writeToReprojectionErrorStatisticsCSV  src/photogrammetrie/util/SceneUtils.cpp:28-80
 *          SceneUtils::writeToReprojectionErrorHistogramCSV   SceneUtils.cpp:82-144
 *
 * The cloud is passed as the arrays the rows in front leave on the device: the
 * coordinates (xyz, doubles), the origin CSR of sfmx_scene.h
 * (origin_offsets[n_points + 1], origin_shot[n_origins], origin_xy[2 * n_origins]
 * as double), the cameras (sfmx_tri_camera), shot_camera and shot_pose (12
 * doubles per shot, CameraShot::getPose, 3x4 [R|t] row-major).
 *
 * The per-record and per-point work runs on the GPU (csrc/report.hip); the
 * statistics of the error list are sfmx_cloud_statistics (n_points = n_errors)
 * and sfmx_cloud_histogram (resolution = -1) of sfmx_cloud.h, which move NaN
 * errors behind the ordered ones before they sort; the writers are host code
 * (csrc/report_host.hpp).  Parity is with the project's restatement
 * (tests/report_ref.py).  Deviations from the reference, all in DESIGN.md §8k / §9:
 *   - the reprojection uses the rotation R of `shot_pose` itself; the reference
 *     projects with Rodrigues(Rodrigues(R)) (CameraShot.cpp:96-100), a host
 *     libm round trip (as sfmx_triangulate_matches);
 *   - a NaN error is emitted as the canonical quiet NaN;
 *   - a colour whose origin position is not finite, or rounds outside the
 *     image, is the default colour (the reference reads out of bounds);
 *   - Scene::colorizePointcloud's overwrite = true and writeToPLY's ascii cloud
 *     branch are not built: no reference call path reaches them;
 *   - the cloud PLY is written in cloud order (the reference: the order its
 *     threads reach an `omp critical`).
 *
 * Status codes and threading as in sfmx.h.  Calls on one device are serialised
 * inside the library (they share that device's cached scratch); the
 * *_last_kernel_ms values are per calling thread.
 */
#ifndef SFMX_REPORT_H
#define SFMX_REPORT_H

#include <stdint.h>
#include "sfmx.h"
#include "sfmx_cloud.h"         /* sfmx_cloud_stats */
#include "sfmx_mvs.h"           /* sfmx_mvs_camera, sfmx_mvs_shot */
#include "sfmx_triangulate.h"   /* sfmx_tri_camera */

#ifdef __cplusplus
extern "C" {
#endif

/* The reprojection error of every origin record (SceneUtils.cpp:43-62, the
 * loop both CSV writers run): for record i of point p in shot s at q,
 *   X = cv::Point3f(xyz[p])                                        (:56)
 *   (u, v) = cv::projectPoints(X, R, t, K, distortion) as float    (:57-58)
 *   out_err[i] = cv::norm(q - cv::Point2d(u, v)) = sqrt(du*du + dv*dv), in double (:62)
 * in record order (the reference appends under `omp critical` in no fixed
 * order; statistics and histogram do not depend on it).
 *   xyz             3 * n_points doubles
 *   origin_offsets  n_points + 1, ascending from 0 to n_origins
 *   cameras         n_cameras cameras; shot i uses cameras[shot_camera[i]]
 *   shot_pose       12 * n_shots doubles
 *   out_err         n_origins doubles
 * n_origins == 0 launches nothing.
 * inputs_on_device = 0: every pointer is host memory.  1: xyz, origin_offsets,
 * origin_shot, origin_xy and out_err are device pointers on `device`; the small
 * arrays (cameras, shot_camera, shot_pose) are always host memory.  The work
 * runs on `stream` and has completed when the call returns.
 * SFMX_EINVAL: a negative count, a NULL array, a shot_camera outside
 * [0, n_cameras), fx == 0 or fy == 0, offsets that do not ascend from 0 to
 * n_origins, an origin_shot outside [0, n_shots).  With device inputs the
 * kernel checks every shot and that every record lies inside the row its search
 * over the offsets finds, and the call reports it after the kernel ran: out_err
 * is then unspecified.  Every index is checked before it is used.
 * Replaces: SceneUtils.cpp:43-69 and :91-117. */
int sfmx_reprojection_errors(const double* xyz, int64_t n_points, const int64_t* origin_offsets,
                             const int32_t* origin_shot, const double* origin_xy, int64_t n_origins,
                             const sfmx_tri_camera* cameras, int32_t n_cameras, const int32_t* shot_camera,
                             const double* shot_pose, int32_t n_shots, int32_t inputs_on_device, int32_t device,
                             void* stream, double* out_err);

/* Device time (ms) of the kernel of the last sfmx_reprojection_errors call on
 * this thread (HIP events on its stream); 0 when the call had no record and
 * launched nothing, -1 before any call. */
float sfmx_reprojection_last_kernel_ms(void);

/* Scene::colorizePointcloud(defaultColor, overwrite = false) (Scene.cpp:569-617).
 * The reference visits the shots in scene order and gives every point that has
 * no colour yet the pixel under its first origin record in that shot
 * (:580-607): the colour of a point comes from the record with the lowest shot
 * index, the first such record in CSR order.  The pixel is image.at<Vec3b>(q)
 * (:601): column cvRound(q.x), row cvRound(q.y), round half to even; the colour
 * is (pixel[2], pixel[1], pixel[0]) of the 8-bit BGR image (:605).  A point with
 * no record keeps the default colour (:610-616).
 *   images          n_shots pointers: 8-bit BGR, image_height[s] rows of
 *                   image_pitch[s] bytes, image_width[s] pixels each
 *   default_rgb     3 bytes; NULL: 0, 0, 0 (cv::Scalar(0, 0, 0, 255), Scene.h:484)
 *   out_rgb         3 * n_points bytes: r, g, b
 *   out_record      optional (NULL ok), n_points: the origin record the colour
 *                   came from; -1 for a point with no record.  A record whose
 *                   position is not finite or rounds outside [0, width) x
 *                   [0, height) is still named, and the colour is the default.
 * inputs_on_device = 0: every pointer is host memory; only the CSR goes to the
 * device, which selects the record and rounds the position, and the pixels are
 * gathered from the host images.  1: origin_*, images[s] and out_* are device
 * pointers on `device` (the pointer table and the sizes are host memory) and
 * one kernel selects and gathers.  Both give the same bytes.
 * SFMX_EINVAL as sfmx_reprojection_errors, and an image with a negative size,
 * a pitch below 3 * width or a NULL pointer with width * height > 0.
 * Replaces: Scene::colorizePointcloud, Scene.cpp:569-617. */
int sfmx_colorize_pointcloud(int64_t n_points, const int64_t* origin_offsets, const int32_t* origin_shot,
                             const double* origin_xy, int64_t n_origins, const uint8_t* const* images,
                             const int32_t* image_width, const int32_t* image_height, const int64_t* image_pitch,
                             int32_t n_shots, const uint8_t* default_rgb, int32_t inputs_on_device, int32_t device,
                             void* stream, uint8_t* out_rgb, int64_t* out_record);

/* As sfmx_reprojection_last_kernel_ms, for sfmx_colorize_pointcloud; 0 when
 * n_points == 0. */
float sfmx_colorize_last_kernel_ms(void);

/* reprojectionerror.stat.csv (SceneUtils.cpp:30-33, :75-77): the header
 * N_Points,Max_Error,Min_Error,Avg_Error,Median_Error,Variance_Error,Deviation_Error
 * and one row, doubles as %.6f.  `s` is sfmx_cloud_statistics of the error
 * list with n_points = n_errors.  The reference has no `size > 1` guard here: an
 * empty list writes the zero row, one error writes what 0.0 / 0.0 prints. */
int sfmx_reprojection_write_stats_csv(const char* path, const sfmx_cloud_stats* s);

/* reprojectionerror.hist.csv (SceneUtils.cpp:136-141): the header Error,Count
 * and one row per key of sfmx_cloud_histogram(errors, n, -1, ...). */
int sfmx_reprojection_write_hist_csv(const char* path, const double* key, const uint64_t* count, int64_t n);

/* pointcloud_sparse.ply (PclUtils.cpp:401-460, binary = true on a little-endian
 * host): the header of :409-421, then 15 bytes per point in cloud order:
 * (float)x, (float)y, (float)z, r, g, b.
 *   xyz   3 * n_points doubles
 *   rgb   3 * n_points bytes (the --colored run, color[0] == -1); NULL: every
 *         point 0, 0, 0 (cv::Scalar(0, 0, 0, 255), PhotogrammetrieCli.cpp:123) */
int sfmx_write_pointcloud_ply(const char* path, const double* xyz, int64_t n_points, const uint8_t* rgb);

/* cameras_recovered.ply (PclUtils.cpp:466-590), ascii: the coordinate system
 * (4 vertices, 3 edges) and per written shot a frustum of 5 vertices (focal
 * point, top left, top right, bottom left, bottom right) and 8 edges.  With
 * norm = 1.0 / max(width, height) of the shot's camera, f = fx == fy ? fx :
 * (fx + fy) / 2 (ICamera.cpp:62-66), the corners are (-cx * norm | width *
 * norm - cx * norm, -cy * norm | height * norm - cy * norm, f * norm),
 * transformed by the pose as cv::Affine3d(pose) * point computes it:
 * ((m0 * x + m1 * y) + m2 * z) + m3 per row; doubles as %.6f.
 *   color           3 bytes; NULL: 255, 255, 0 (PclUtils.h:125)
 *   only_recovered  != 0: shots with recovered == 0 are left out (:470-476)
 * SFMX_EINVAL: a written shot whose camera is outside [0, n_cameras). */
int sfmx_write_cameras_ply(const char* path, const sfmx_mvs_camera* cameras, int32_t n_cameras,
                           const sfmx_mvs_shot* shots, int32_t n_shots, const uint8_t* color,
                           int32_t only_recovered);

#ifdef __cplusplus
}
#endif

#endif /* SFMX_REPORT_H */
