/* SPDX-License-Identifier: MIT
 *
 * sfmx — point-cloud neighbour statistics (the -Prun=pcl-stats sub-program).
 *
 * Replaces PclUtils::getNearestNeighbors       src/photogrammetrie/util/PclUtils.cpp:75-89
 *          PclUtils::writeToNeighborPLY        PclUtils.cpp:91-265   (quality PLY)
 *          PclUtils::writeToNeighborCSV        PclUtils.cpp:267-339  (neighbour histogram)
 *          PclUtils::writeToStatisticsCSV      PclUtils.cpp:341-399
 *          MathUtils::calculateStatistics      src/photogrammetrie/util/MathUtils.h:53-90
 *          PclStatsCli::main                   src/cli/PclStatsCli.cpp:30-79
 *
 * The reference builds a PCL KdTreeFLANN three times and asks it, per point, for
 * the K = 2 + maxEqual nearest points of the cloud itself; the point's distance
 * is the first returned sqrt((double)d) that is > 0, or 0.  d is FLANN's
 * L2_Simple<float>: dx = xi - xj (dy, dz alike), d = (dx*dx + dy*dy) + dz*dz in
 * float without FMA.  The tree search is exact, so with, over all j (i included),
 *     z = #{ j : d == 0 }        m = min{ d : d > 0 }        Ke = min(K, n)
 * the distance is 0 if z >= Ke or no positive d exists, and sqrt((double)m)
 * otherwise.  sfmx_cloud_neighbor_distances computes exactly that on the GPU: a
 * counting sort into a uniform grid, a ring-by-ring search with a proven stop
 * rule, and a brute-force kernel for the queries the rings do not finish
 * (DESIGN.md §8j).  The search runs once and feeds all three outputs.
 *
 * Parity is with the project's restatement (tests/cloud_ref.py); PCL, FLANN and
 * their PLY reader are not pinned.  Points the reference leaves open, all in
 * DESIGN.md §8j:
 *   - a point with a non-finite coordinate is never a candidate; its own
 *     distance is 0 and its neighbour -1 (PCL leaves it out of the tree and
 *     asserts on it as a query);
 *   - maxDistance == 0 in the quality PLY writes r = b = 0 (the reference
 *     converts a NaN to u_char);
 *   - a double above 255 becomes a u_char by truncation to int32, low 8 bits
 *     (undefined in C++; what the reference's x86-64 build does);
 *   - a face with an index outside [0, vertex count), with more than 255
 *     vertices or with none is not written (the reference reads out of bounds /
 *     skips / divides by zero); `element face` still counts it;
 *   - faces are written in input order (the reference: unspecified order).
 *
 * Status codes and threading as in sfmx.h.  Calls on one device are serialised
 * inside the library (they share that device's cached scratch).
 * sfmx_cloud_last_stats is per calling thread.
 */
#ifndef SFMX_CLOUD_H
#define SFMX_CLOUD_H

#include <stdint.h>
#include "sfmx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Nearest-neighbour distance of every point of a cloud to the cloud itself.
 *   xyz            3 * n floats
 *   max_equal      PclUtils' maxEqual; negative values count as 0
 * Outputs:
 *   out_distance   n doubles: 0 or sqrt((double)m) as above
 *   out_neighbor   optional (NULL ok), n: the smallest index among the points
 *                  attaining m; -1 where the distance is 0
 * n <= 1 writes 0 / -1 and launches nothing (the reference's `size > 1` guard
 * belongs to the statistics layer: pass n_distances = 0 there).
 * inputs_on_device = 0: every pointer is host memory.  1: xyz and the outputs
 * are device pointers on `device`; the work runs on `stream` and has completed
 * when the call returns.
 * SFMX_EINVAL: n < 0, a NULL xyz (n > 0) or out_distance (n > 0), a device
 * index out of range.  SFMX_ECAPACITY: n > 2^31 - 65.
 * Replaces: PclUtils::getNearestNeighbors and the three per-point loops around
 * it, PclUtils.cpp:75-89, :109-136, :285-309, :358-382. */
int sfmx_cloud_neighbor_distances(const float* xyz, int64_t n, int32_t max_equal, int32_t inputs_on_device,
                                  int32_t device, void* stream, double* out_distance, int64_t* out_neighbor);

/* Of the last sfmx_cloud_neighbor_distances call on this thread (any NULL ok):
 *   kernel_ms      device time of its kernels (HIP events on its stream); 0 when
 *                  nothing was launched, -1 before any call
 *   evaluations    number of squared distances d evaluated by the search and the
 *                  brute-force kernel together
 *   brute_queries  points resolved by the brute-force kernel */
int sfmx_cloud_last_stats(float* kernel_ms, int64_t* evaluations, int64_t* brute_queries);

/* MathUtils::calculateStatistics of a distance list, bug for bug: the list is
 * sorted ascending; min = min(0, all) and max = max(0, all) (both start at 0);
 * mean and variance are sequential double sums in sorted order, the variance
 * over (size - 1) with (x - mean) * (x - mean) for pow(x - mean, 2); the median
 * is the middle element or the mean of the two middle ones; an empty list gives
 * zeros.  n_points is carried into the record (the N_Points column).  NaN
 * elements (reprojection errors, sfmx_report.h; distances have none) stand
 * behind the ordered ones: the reference's sort is undefined on them. */
typedef struct sfmx_cloud_stats {
    int64_t n_points;
    double max, min, mean, median, variance, deviation;
} sfmx_cloud_stats;
int sfmx_cloud_statistics(const double* distances, int64_t n_distances, int64_t n_points, sfmx_cloud_stats* out);

/* PclUtils.cpp:313-328: resolution < 0 -> the variance of the list; key =
 * (resolution <= 0) ? distance : ceil(distance / resolution) * resolution;
 * counts per distinct double key, keys ascending (NaN keys: one last row).
 * *required = number of rows; with cap < *required nothing is written and the
 * call returns SFMX_ECAPACITY (out_key / out_count NULL with cap = 0: sizes only). */
int sfmx_cloud_histogram(const double* distances, int64_t n_distances, double resolution, double* out_key,
                         uint64_t* out_count, int64_t cap, int64_t* required);

/* Reads the vertex positions and the faces of a PLY file (ascii or
 * binary_little_endian): a `vertex` element with float x, y, z among scalar
 * properties of any type, an optional `face` element with one list property
 * vertex_indices / vertex_index (uchar counts, int or uint indices) among
 * scalar properties, any other element with scalar properties only.  Everything
 * else, a truncated body or a count that overruns the file is SFMX_EINVAL with a
 * sfmx_last_error text.  The three counts are always written; a NULL buffer is
 * skipped, a non-NULL one with a capacity below its count is SFMX_ECAPACITY.
 *   xyz 3 * n_points floats, face_sizes n_faces, face_indices n_indices (concatenated) */
int sfmx_ply_read(const char* path, float* xyz, int64_t cap_points, int64_t* n_points, int32_t* face_sizes,
                  int64_t cap_faces, int64_t* n_faces, int32_t* face_indices, int64_t cap_indices, int64_t* n_indices);

/* The three files of PclStatsCli (byte layouts: DESIGN.md §8j).  The quality
 * PLY takes the cloud, its distances (n_distances = n_points, or 0 when
 * n_points <= 1) and the faces as sfmx_ply_read returns them; distance_cutoff
 * > 0 clamps a distance before it is used (the CLI passes -1). */
int sfmx_cloud_write_stats_csv(const char* path, const sfmx_cloud_stats* s);
int sfmx_cloud_write_neighbors_csv(const char* path, const double* key, const uint64_t* count, int64_t n);
int sfmx_cloud_write_quality_ply(const char* path, const float* xyz, const double* distances, int64_t n_distances,
                                 const int32_t* face_sizes, int64_t n_faces, const int32_t* face_indices,
                                 double distance_cutoff);

#ifdef __cplusplus
}
#endif

#endif /* SFMX_CLOUD_H */
