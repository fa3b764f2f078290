/* SPDX-License-Identifier: MIT
 *
 * sfmx — the incremental reconstruction loop, SfM::triangulate (sfm/SfM.cpp:164-381),
 * as control flow over a table of steps.
 *
 * sfmx_sfm_triangulate_steps owns the loop's bookkeeping: the to-triangulate,
 * triangulated and failed pair lists, the recovered flags, the pairs' match counts and
 * homography ratios.  Everything that touches keypoints, poses or the cloud is a step the
 * caller supplies.  The library's own rows behind the steps are: relative pose
 * sfmx_relative_poses, triangulation sfmx_triangulate_matches, merge
 * sfmx_merge_pointcloud_3d2d, ranking sfmx_count_3d2d_matches, registration
 * sfmx_find_3d2d_matches + sfmx_distinct_3d2d_points + sfmx_register_poses, adjustment
 * sfmx_ba_observations_from_origins + sfmx_ba_solve.  A reference-side adapter replaces
 * SfM::triangulate by a call with steps over its own Scene.
 *
 * No GPU is needed to call it.  Status codes as in sfmx.h.
 */
#ifndef SFMX_SFM_H
#define SFMX_SFM_H

#include <stdint.h>
#include "sfmx.h"
#include "sfmx_homography.h"    /* sfmx_point2f */
#include "sfmx_triangulate.h"   /* sfmx_tri_camera */
#include "sfmx_ba.h"            /* SFMX_CAM_*, SFMX_BA_* */

#ifdef __cplusplus
extern "C" {
#endif

/* The values of SfM.h:48-57 the loop and its steps read. */
typedef struct sfmx_sfm_params {
    int32_t min_match_count_for_baseline;   /* SfM.h:49   100; >= 4                          */
    int32_t _reserved;                      /* 0                                             */
    double ransac_baseline_threshold;       /* SfM.h:51   -1.0 (for the relative pose step)  */
    double ransac_pose_threshold;           /* SfM.h:52   -8.0 (for the registration step)   */
    double min_homography_inlier_ratio;     /* SfM.h:53   0.5; in [0, 1]                     */
    double min_pose_inlier_ratio;           /* SfM.h:54   0.5; in [0, 1]                     */
    double max_reprojection_error;          /* SfM.h:55   10.0 (for the triangulation step)  */
    double point_merge_distance;            /* SfM.h:56   0.01; not NaN (for the merge step) */
    double feature_merge_distance;          /* SfM.h:57   20.0; not NaN                      */
} sfmx_sfm_params;

int sfmx_sfm_default_params(sfmx_sfm_params* params);

/* The steps.  `user` is passed through.  A step returns a value < 0 to abort the loop;
 * sfmx_sfm_triangulate_steps then returns that value at once.
 *
 * relative_pose     findCameraPoseFromMatch (SfM.cpp:202, :345) of a pair.  Returns 1 and
 *                   the number of inliers, or 0 where the reference throws.  It changes
 *                   nothing in the scene.
 * triangulate_pair  what follows an accepted relative pose: the pair's match list becomes
 *                   the inliers of the last relative_pose of this pair (:213, :350); with
 *                   initial = 1 the left shot's pose becomes [I|0] and the right shot's the
 *                   relative pose (:214-215); then triangulateMatch (:220, :356).
 *                   *n_points: the elements it made, held by the step until add_elements.
 * add_elements      the elements of the last triangulate_pair go into the cloud: merge = 0
 *                   appended as they are (:221-223), merge = 1 through
 *                   mergePointcloudElement3d2d with the two merge distances (:358-362).
 * count_candidates  counts[i] = size of the list Scene::find3d2dMatches gives for shots[i]
 *                   (:276-282), over every pair of the scene.
 * register_shot     find3d2dMatches and findCameraPoseFrom3d2dMatch (:305) for the shot.
 *                   Returns 1 with *ratio, or another value >= 0 where the reference throws
 *                   (the loop then takes the ratio as -1).  The pose is kept by the step
 *                   and not applied.  distinct_pairs receives getDistinctShotMatches
 *                   (:333) of the shot's 3D-2D matches, at most `capacity` = n_pairs.
 * accept_shot       the pose of the last register_shot becomes the shot's pose (:329).
 * bundle_adjust     BundleAdjustment::doBundleAdjustment(scene) (:235, :371); iterations
 *                   and termination type go into the summary and the trace. */
typedef struct sfmx_sfm_steps {
    int (*relative_pose)(void* user, int32_t pair, int32_t* n_inliers);
    int (*triangulate_pair)(void* user, int32_t pair, int32_t initial, int32_t* n_points);
    int (*add_elements)(void* user, int32_t pair, int32_t merge);
    int (*count_candidates)(void* user, const int32_t* shots, int32_t n_shots, int32_t* counts);
    int (*register_shot)(void* user, int32_t shot, double* ratio, int32_t* distinct_pairs, int32_t capacity,
                         int32_t* n_distinct_pairs);
    int (*accept_shot)(void* user, int32_t shot);
    int (*bundle_adjust)(void* user, int32_t* iterations, int32_t* termination_type);
} sfmx_sfm_steps;

/* One record of the trace: what the loop decided, in order.              a      b              value          */
enum {
    SFMX_SFM_NO_CANDIDATE_PAIR = 1,   /* no pair passes the homography filter    -1     -1             0              */
    SFMX_SFM_INITIAL_TRY = 2,         /* :197                                    pair   match count    homography r.  */
    SFMX_SFM_INITIAL_THROWS = 3,      /* :203-206 relative_pose returned 0       pair   -1             0              */
    SFMX_SFM_INITIAL_LOW_RATIO = 4,   /* :209-212                                pair   inliers        inlier ratio   */
    SFMX_SFM_INITIAL_PAIR = 5,        /* :213-233                                pair   points         inlier ratio   */
    SFMX_SFM_NO_INITIAL_PAIR = 6,     /* :239-242                                -1     -1             0              */
    SFMX_SFM_BUNDLE_ADJUST = 7,       /* :235, :371                              iter.  termination    0              */
    SFMX_SFM_SHOT_CHOSEN = 8,         /* :300                                    shot   its count      candidates     */
    SFMX_SFM_SHOT_FAILED = 9,         /* :311                                    shot   step's status  ratio (or -1)  */
    SFMX_SFM_PAIR_FAILED = 10,        /* :320-325                                pair   the shot       0              */
    SFMX_SFM_SHOT_REGISTERED = 11,    /* :329-330                                shot   distinct pairs ratio          */
    SFMX_SFM_PAIR_SKIPPED = 12,       /* :335-337 a shot of it is not recovered  pair   -1             0              */
    SFMX_SFM_PAIR_THROWS = 13,        /* :346-349 the pair stays open            pair   -1             0              */
    SFMX_SFM_PAIR_TRIANGULATED = 14,  /* :350-368                                pair   points         inliers        */
    SFMX_SFM_NO_REMAINING_SHOT = 15,  /* :272-274                                open pairs  -1        0              */
    SFMX_SFM_DONE = 16                /* :378                                    triangulated  failed  open pairs     */
};

typedef struct sfmx_sfm_event {
    int32_t event, a, b, _pad;
    double value;
} sfmx_sfm_event;

enum { SFMX_SFM_PAIR_OPEN = 0, SFMX_SFM_PAIR_DONE = 1, SFMX_SFM_PAIR_LOST = 2 };

#define SFMX_SFM_N_STEPS 7   /* in the order of sfmx_sfm_steps */

typedef struct sfmx_sfm_summary {
    int32_t ba_calls, ba_iterations, last_termination_type;   /* -1 before any BA */
    int32_t shots_recovered, pairs_triangulated, pairs_failed, pairs_open, initial_pair;   /* -1: none */
    int64_t step_calls[SFMX_SFM_N_STEPS];
    double step_wall_ms[SFMX_SFM_N_STEPS];   /* host wall time spent inside each kind of step */
} sfmx_sfm_summary;

/* SfM::triangulate over `steps`.
 *   pairs[2 * n_pairs]         (left, right) shot indices in Scene::getShotMatches() order
 *   pair_n_matches[n_pairs]    length of every pair's match list on entry
 *   homography_ratio[n_pairs]  ShotMatches::getHomographyInlierRatio (sfmx_homography_ratios)
 *   out_recovered[n_shots]     1: the shot has a pose
 *   out_pair_state[n_pairs]    SFMX_SFM_PAIR_*: the list the pair was moved to last
 *   out_pair_n_matches[n_pairs]  lengths at the end: inliers where a list was replaced (may be NULL)
 *   trace[trace_capacity]      the first trace_capacity events; *out_n_events counts all of them
 *   summary                    may be NULL
 * Where the reference leaves an order open: the initial candidates are the
 * pairs with at least min_match_count_for_baseline matches in ascending homography ratio,
 * then the others in ascending ratio, equal ratios in list order; the remaining shots are
 * in ascending index; among equal counts the lowest shot index is chosen; no pair passing
 * the homography filter is an empty reconstruction, not an error.
 * Checked before any step is called, SFMX_EINVAL: a null pointer, a negative count,
 * min_match_count_for_baseline < 4, a ratio threshold outside [0, 1], a NaN threshold or
 * merge distance, a pair shot outside [0, n_shots), a negative match count, a NaN
 * homography ratio.  SFMX_ECAPACITY after the loop has finished: the trace was too short
 * (every output but the trace's tail is complete). */
int sfmx_sfm_triangulate_steps(const sfmx_sfm_steps* steps, void* user, const sfmx_sfm_params* params, int32_t n_shots,
                               const int32_t* pairs, int32_t n_pairs, const int32_t* pair_n_matches,
                               const double* homography_ratio, int32_t* out_recovered, int32_t* out_pair_state,
                               int32_t* out_pair_n_matches, sfmx_sfm_event* trace, int64_t trace_capacity,
                               int64_t* out_n_events, sfmx_sfm_summary* summary);

/* The rows behind the steps of sfmx_sfm_triangulate, for its timing. */
enum {
    SFMX_SFM_ROW_COUNT = 0,       /* sfmx_count_3d2d_matches                                   */
    SFMX_SFM_ROW_FIND = 1,        /* sfmx_find_3d2d_matches + sfmx_distinct_3d2d_points        */
    SFMX_SFM_ROW_REGISTER = 2,    /* sfmx_register_poses                                       */
    SFMX_SFM_ROW_POSE = 3,        /* sfmx_relative_poses                                       */
    SFMX_SFM_ROW_TRIANGULATE = 4, /* sfmx_triangulate_matches                                  */
    SFMX_SFM_ROW_MERGE = 5,       /* sfmx_merge_pointcloud_3d2d                                */
    SFMX_SFM_ROW_BA = 6,          /* sfmx_ba_solve (device_ms: the minimizer's total_ms)       */
    SFMX_SFM_ROW_HANDOFF = 7,     /* work between the rows: the scene's first upload, the
                                     repack of a shrunk list, appending the first elements,
                                     the BA problem's arrays and write-back (device_ms 0)      */
    SFMX_SFM_N_ROWS = 8
};

typedef struct sfmx_sfm_timing {
    int64_t calls[SFMX_SFM_N_ROWS];
    double device_ms[SFMX_SFM_N_ROWS];     /* the rows' *_last_kernel_ms, summed                */
    double wall_ms[SFMX_SFM_N_ROWS];       /* host wall time inside the rows' calls, summed     */
    int64_t handoff_bytes[SFMX_SFM_N_ROWS]; /* bytes that cross between host and device for each row     */
} sfmx_sfm_timing;

/* SfM::triangulate with the library's own rows as steps: the reconstruction of a scene
 * from its keypoints, its match graph and the pairs' homography ratios.
 *   keypoints, n_keypoints, n_shots   as in sfmx_triangulate_matches (host memory)
 *   shot_size                 2 * n_shots: width, height of every shot's image
 *   cameras, n_cameras        ONE camera (SfM's command line builds one); more is
 *                             SFMX_ECAPACITY, none SFMX_EINVAL
 *   camera_model              SFMX_CAM_*: its bundle-adjustment model
 *   pairs, n_pairs, matches, pair_offsets   the packed match graph (sfmx.h), host memory
 *   homography_ratio          n_pairs (sfmx_homography_ratios' output)
 * Outputs, all caller's host buffers; M = pair_offsets[n_pairs]:
 *   out_recovered             n_shots
 *   out_pose                  12 * n_shots, [R|t] row-major; an unrecovered shot's is NaN
 *   out_camera                the camera after the last adjustment
 *   out_xyz                   3 * point_capacity; the cloud never has more than M points
 *   out_origin_offsets        point_capacity + 1
 *   out_origin_shot / _xy     record_capacity / 2 * record_capacity; never more than 2 * M records
 *   out_n_points, out_n_records
 *   out_matches               M: the final lists, packed (a list that was posed holds its inliers)
 *   out_pair_offsets          n_pairs + 1
 *   out_pair_state            n_pairs, SFMX_SFM_PAIR_*
 *   trace, trace_capacity, out_n_events, summary   as in sfmx_sfm_triangulate_steps
 *   timing                    may be NULL
 * The steps: relative pose = sfmx_relative_poses on the pair alone with
 * params->ransac_baseline_threshold; triangulation = sfmx_triangulate_matches on the pair
 * alone with params->max_reprojection_error; the initial pair's elements are appended, the
 * others go through sfmx_merge_pointcloud_3d2d over the whole match graph as it is at that
 * moment; ranking = sfmx_count_3d2d_matches over every pair; registration =
 * sfmx_find_3d2d_matches, sfmx_distinct_3d2d_points, sfmx_register_poses (one set,
 * params->ransac_pose_threshold; a shot without a 3D-2D match and status 0 or 2 count as
 * "throws"); getDistinctShotMatches = the pairs of the 3D-2D matches in first-appearance
 * order over the point-major origin records; adjustment =
 * sfmx_ba_observations_from_origins, sfmx_pose_to_ceres, sfmx_ba_solve with default
 * options on `device`, and the write-back of points, poses and intrinsics
 * (ceresApplyParameters: f -> fx = fy, and the model's distortion / centre entries).  An
 * empty cloud is not adjusted (iterations 0, termination type -1 in the trace).
 * The scene stays on `device` between the rows: the keypoints go up once, the packed match
 * lists, the cloud and what one row hands the next live there, every row runs with
 * inputs_on_device = 1, and a list that shrinks to its inliers is repacked on the device.
 * The host sees offsets, counts, statuses and poses; the cloud comes to the host for
 * sfmx_ba_solve, and the merge stages its own resolution.  DESIGN.md §8l lists the hand-offs.
 * Checked before any step runs, SFMX_EINVAL: what sfmx_sfm_triangulate_steps checks, a
 * null argument, offsets that do not ascend from 0, a match index outside its image's
 * keypoints, an unknown camera model, fx == 0 or fy == 0, capacities below the bounds
 * above.  Any row's error ends the loop and is returned. */
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
                         sfmx_sfm_timing* timing);

#ifdef __cplusplus
}
#endif

#endif /* SFMX_SFM_H */
