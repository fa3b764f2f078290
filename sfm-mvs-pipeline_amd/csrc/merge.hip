// SPDX-License-Identifier: MIT
// sfmx point-cloud merge for gfx950.
//
//   sfmx_merge_pointcloud_3d2d   Scene::mergePointcloudElement3d2d (common/Scene.cpp:470-567), called
//                                once per triangulated element by SfM.cpp:354-363
//
// The reference scans the whole cloud per new element for points within pointMergeDistance and then,
// per (element origin point x candidate origin point), walks the shot-match list and that pair's DMatch
// list comparing keypoint positions.  A candidate can only qualify through a DMatch that joins one of
// the element's keypoints to one of the candidate's, so the qualifying candidates are reachable through
// the match graph — a hash join, as in scene.hip:
//   1. (host, O(pairs)) the first pair in list order per unordered shot pair — the only pair the
//      reference's search loop can stop at (Scene.cpp:505-520);
//   2. link table: every admissible DMatch of a first pair (valid indices, non-NaN positions,
//      |distance| <= F) as two entries keyed by (shot, position bits), the partner entry is the other side;
//   3. record tables: the cloud's records at call start and the new elements' records, keyed the same
//      way, value = record index (its point / element index in a side array);
//      all three tables are multi-valued: every entry claims a slot of its own (one 32-bit CAS, no key
//      in the slot), a lookup walks the probe sequence to the first empty slot and compares the key of
//      every entry it meets (cv::Point2d(kp.pt) == record, in double, as the reference);
//   4. one thread per new element: records -> link entries -> partners -> cloud points holding the
//      partner record, the fp64 near test, and the two values the fold rule needs (lowest-index
//      qualifier with its distance; lowest-index minimum over non-NaN distances); the same walk against
//      the new-record table counts, then fills, the earlier elements linked to this one (the list
//      offsets are a device scan of the counts);
//   5. the resolution, for e in order: static summary + the targets of its linked earlier elements, the
//      fold (Scene.cpp:532-538), merge or append.  A record added during the call always comes from an
//      earlier new element, so "qualifies through a record added in this call" is exactly "linked to an
//      earlier element and near that element's target": the only sequential dependence is the DAG of
//      links among the new elements.  resolve_kernel runs in rounds, one thread per element: an element
//      is decided in the first launch after the one that decided the last of its linked elements (a
//      per-element round stamp, so a value written in the same launch is never used); the host reads one
//      word per round, the number still undecided.  A point appended in the call is known as
//      n_cloud + its element until a scan of the appended flags gives the final indices;
//   5b. record-level dedupe and every output record's destination: the merged elements grouped by
//      target (count, scan, fill, each group sorted by element index), one thread per output point that
//      walks its group in merge order, a scan of the points' sizes, the destinations;
//   5'. (host, sequential, O(n_new + links)) the same resolution and dedupe on the host: the path of a
//      call whose link DAG is deeper than the round cap, or with the device resolution switched off; it
//      stages the summaries, the link lists and (device inputs) both clouds;
//   6. one scatter kernel writes the output xyz and origin CSR.
// Integer / byte work with one fp64 distance per candidate: latency- and HBM-bound, no MFMA, no
// floating-point atomics (one thread owns one element; the counters are integer).  No workgroup waits
// for another inside a launch; every scan is three launches.  Built with -ffp-contract=off (host and
// device evaluate the same uncontracted distance).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/sfmx_scene.h"
#include "device_call.hpp"
#include "match_common.hpp"
#include "scene_plan.hpp"

namespace sfmx {
namespace merge {

// every NaN as the one quiet NaN 0x7ff8000000000000 (on the bits: a select on d != d may be folded away)
__host__ __device__ __forceinline__ double canonical(double d) {
    unsigned long long u;
    memcpy(&u, &d, sizeof u);
    if ((u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) u = 0x7ff8000000000000ull;
    memcpy(&d, &u, sizeof u);
    return d;
}

// cv::norm(candidate - element) (Scene.cpp:482-485): sqrt(x*x + y*y + z*z) in double
__host__ __device__ __forceinline__ double point_distance(const double* c, const double* e) {
    const double dx = c[0] - e[0], dy = c[1] - e[1], dz = c[2] - e[2];
    return canonical(sqrt((dx * dx + dy * dy) + dz * dz));
}

__device__ __forceinline__ unsigned long long pos_key(float x, float y) {
    x = x == 0.f ? 0.f : x;   // -0 == +0 under cv::Point2d ==
    y = y == 0.f ? 0.f : y;
    return ((unsigned long long)__float_as_uint(x) << 32) | __float_as_uint(y);
}
__device__ __forceinline__ uint32_t mix(unsigned long long k, int shot) {
    k ^= (unsigned long long)(uint32_t)(shot + 1) * 0x9e3779b97f4a7c15ull;
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (uint32_t)k;
}

// The words of a call the host reads back, or the kernels hand to each other.
struct Words {
    int32_t full;         // a hash table filled up
    int32_t bad;          // device inputs: which check of validate_kernel failed, 0 if none
    int32_t unresolved;   // elements the last resolve round left undecided
    int32_t pad;
    unsigned long long merged_static, merged_dynamic;
};

// claim an empty slot for entry `id`; the loop is bounded by the capacity, a full table raises the flag
__device__ __forceinline__ void insert(int32_t* __restrict__ slot, uint32_t cap, uint32_t h, int32_t id,
                                       int32_t* __restrict__ full) {
    h &= cap - 1;
    for (uint32_t probe = 0; probe < cap; ++probe) {
        if (atomicCAS(slot + h, -1, id) == -1) return;
        h = (h + 1) & (cap - 1);
    }
    *full = 1;
}

// the record (x, y) as the float position it can equal, if any (NaN and non-representable doubles: none)
__device__ __forceinline__ bool as_float_pos(double x, double y, float* fx, float* fy) {
    *fx = (float)x;
    *fy = (float)y;
    return (double)*fx == x && (double)*fy == y;
}

// Device inputs: what the host checks of host arrays.  One thread per offset of the two origin offset arrays
// (off[0] == 0, off[i] >= off[i - 1]) and per origin record (its shot in [0, n_shots)); n_crec / n_nrec are the
// arrays' last entries as the host read them.  A thread whose check fails raises the flag and touches nothing
// else; the kernels that walk the offsets (build_records_kernel, probe_kernel) return at once under the flag.
// The flag names the check that failed, the one the host would have met first if several did (an integer max).
enum : int32_t { BAD_NEW_SHOT = 1, BAD_CLOUD_SHOT = 2, BAD_NEW_OFFSETS = 3, BAD_CLOUD_OFFSETS = 4 };
__global__ __launch_bounds__(256)
void validate_kernel(int n_cloud, int n_new, int64_t n_crec, int64_t n_nrec, int n_shots,
                     const int64_t* __restrict__ cloud_off, const int64_t* __restrict__ new_off,
                     const int32_t* __restrict__ cloud_shot, const int32_t* __restrict__ new_shot, int32_t* __restrict__ bad) {
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = true;
    int32_t what = 0;
    if (g <= n_cloud) {
        ok = g == 0 ? cloud_off[0] == 0 : cloud_off[g] >= cloud_off[g - 1];
        what = BAD_CLOUD_OFFSETS;
    } else if ((g -= (int64_t)n_cloud + 1) <= n_new) {
        ok = g == 0 ? new_off[0] == 0 : new_off[g] >= new_off[g - 1];
        what = BAD_NEW_OFFSETS;
    } else if ((g -= (int64_t)n_new + 1) < n_crec) {
        ok = cloud_shot[g] >= 0 && cloud_shot[g] < n_shots;
        what = BAD_CLOUD_SHOT;
    } else if ((g -= n_crec) < n_nrec) {
        ok = new_shot[g] >= 0 && new_shot[g] < n_shots;
        what = BAD_NEW_SHOT;
    }
    if (!ok) atomicMax(bad, what);
}

// the message of a raised flag, as the host checks word it
inline const char* bad_input(int32_t what) {
    return what == BAD_CLOUD_OFFSETS ? "cloud origin offsets do not ascend from 0"
         : what == BAD_NEW_OFFSETS   ? "new origin offsets do not ascend from 0"
         : what == BAD_CLOUD_SHOT    ? "cloud origin shot out of range"
                                     : "new origin shot out of range";
}

// one thread per DMatch: the two link entries 2g (left side) and 2g + 1 (right side)
__global__ __launch_bounds__(256)
void build_links_kernel(int64_t n_matches, int n_pairs, const int64_t* __restrict__ off,
                        const int32_t* __restrict__ pair_first, const int32_t* __restrict__ pairs,
                        const DMatchDev* __restrict__ matches, const float2* const* __restrict__ kp,
                        const int32_t* __restrict__ nkp, double F, int32_t* __restrict__ slot, uint32_t cap,
                        int32_t* __restrict__ ent_shot, unsigned long long* __restrict__ ent_pos,
                        int32_t* __restrict__ full) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_matches) return;
    int lo = 0, hi = n_pairs - 1;   // the pair whose list holds match g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    if (!pair_first[lo]) return;   // a later duplicate of the unordered pair is never consulted
    const DMatchDev d = matches[g];
    const int L = pairs[2 * lo], R = pairs[2 * lo + 1];
    if (d.queryIdx < 0 || d.queryIdx >= nkp[L] || d.trainIdx < 0 || d.trainIdx >= nkp[R]) return;
    if (!((double)fabsf(d.distance) <= F)) return;   // NaN fails
    const float2 a = kp[L][d.queryIdx], b = kp[R][d.trainIdx];
    if (a.x != a.x || a.y != a.y || b.x != b.x || b.y != b.y) return;
    const unsigned long long ka = pos_key(a.x, a.y), kb = pos_key(b.x, b.y);
    ent_shot[2 * g] = L;
    ent_pos[2 * g] = ka;
    ent_shot[2 * g + 1] = R;
    ent_pos[2 * g + 1] = kb;
    insert(slot, cap, mix(ka, L), (int32_t)(2 * g), full);
    insert(slot, cap, mix(kb, R), (int32_t)(2 * g + 1), full);
}

// one thread per origin record: its point and, if a keypoint position can equal it, its table entry
__global__ __launch_bounds__(256)
void build_records_kernel(int64_t n_rec, int n_pts, const int64_t* __restrict__ off,
                          const int32_t* __restrict__ shot, const double* __restrict__ xy,
                          int32_t* __restrict__ slot, uint32_t cap, int32_t* __restrict__ rec_point,
                          int32_t* __restrict__ full, const int32_t* __restrict__ bad) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rec || *bad) return;
    int lo = 0, hi = n_pts - 1;   // the last point whose range starts at or before r (skips empty points)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    rec_point[r] = lo;
    float fx, fy;
    if (!as_float_pos(xy[2 * r], xy[2 * r + 1], &fx, &fy)) return;
    insert(slot, cap, mix(pos_key(fx, fy), shot[r]), (int32_t)r, full);
}

struct Table {             // a multi-valued record table
    const int32_t* slot;
    uint32_t cap;
    const int32_t* shot;   // the records it indexes
    const double* xy;
    const int32_t* owner;  // record -> point / element
};

struct Summary {           // what the fold rule needs of an element's static candidates
    int32_t first_idx;     // lowest-index qualifying cloud point, -1: none
    int32_t min_idx;       // lowest-index point among the smallest non-NaN distances, -1: none
    double first_d, min_d;
};

// one thread per new element.  FILL = false: the static summary and the number of earlier linked
// elements; FILL = true: the list of those elements at link_off[e].
template <bool FILL>
__global__ __launch_bounds__(256)
void probe_kernel(int n_new, const int64_t* __restrict__ new_off, const int32_t* __restrict__ new_shot,
                  const double* __restrict__ new_xy, const double* __restrict__ new_xyz,
                  const double* __restrict__ cloud_xyz, double D, const int32_t* __restrict__ lslot, uint32_t lcap,
                  const int32_t* __restrict__ ent_shot, const unsigned long long* __restrict__ ent_pos, Table cloud,
                  Table fresh, Summary* __restrict__ summary, int32_t* __restrict__ link_count,
                  const int64_t* __restrict__ link_off, int32_t* __restrict__ link_list, const int32_t* __restrict__ bad) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_new || *bad) return;
    Summary s{-1, -1, 0.0, 0.0};
    const double ex[3] = {new_xyz[3 * (int64_t)e], new_xyz[3 * (int64_t)e + 1], new_xyz[3 * (int64_t)e + 2]};
    int32_t links = 0;
    const int64_t out0 = FILL ? link_off[e] : 0;
    const int32_t out_n = FILL ? (int32_t)(link_off[e + 1] - out0) : 0;
    for (int64_t r = new_off[e]; r < new_off[e + 1]; ++r) {
        float fx, fy;
        if (!as_float_pos(new_xy[2 * r], new_xy[2 * r + 1], &fx, &fy)) continue;   // no keypoint can equal it
        const int se = new_shot[r];
        const unsigned long long key = pos_key(fx, fy);
        uint32_t h = mix(key, se) & (lcap - 1);
        for (uint32_t probe = 0; probe < lcap; ++probe, h = (h + 1) & (lcap - 1)) {
            const int32_t i = lslot[h];
            if (i < 0) break;
            if (ent_shot[i] != se || ent_pos[i] != key) continue;
            // a DMatch of the first pair joining {se, sc} with this record on se's side: its other side
            const int sc = ent_shot[i ^ 1];
            const unsigned long long pk = ent_pos[i ^ 1];
            const double px = (double)__uint_as_float((uint32_t)(pk >> 32)), py = (double)__uint_as_float((uint32_t)pk);
            const uint32_t ph = mix(pk, sc);
            if (!FILL) {
                uint32_t g = ph & (cloud.cap - 1);
                for (uint32_t q = 0; q < cloud.cap; ++q, g = (g + 1) & (cloud.cap - 1)) {
                    const int32_t j = cloud.slot[g];
                    if (j < 0) break;
                    if (cloud.shot[j] != sc || cloud.xy[2 * (int64_t)j] != px || cloud.xy[2 * (int64_t)j + 1] != py) continue;
                    const int32_t c = cloud.owner[j];
                    const double d = point_distance(cloud_xyz + 3 * (int64_t)c, ex);
                    if (d > D) continue;   // Scene.cpp:483: a NaN distance stays a candidate
                    if (s.first_idx < 0 || c < s.first_idx) { s.first_idx = c; s.first_d = d; }
                    if (d == d && (s.min_idx < 0 || d < s.min_d || (d == s.min_d && c < s.min_idx))) { s.min_idx = c; s.min_d = d; }
                }
            }
            uint32_t g = ph & (fresh.cap - 1);
            for (uint32_t q = 0; q < fresh.cap; ++q, g = (g + 1) & (fresh.cap - 1)) {
                const int32_t j = fresh.slot[g];
                if (j < 0) break;
                if (fresh.shot[j] != sc || fresh.xy[2 * (int64_t)j] != px || fresh.xy[2 * (int64_t)j + 1] != py) continue;
                const int32_t e2 = fresh.owner[j];
                if (e2 >= e) continue;
                if (FILL) { if (links < out_n) link_list[out0 + links] = e2; }
                if (links < INT32_MAX) ++links;   // saturates: the host refuses a total beyond int32
            }
        }
    }
    if (!FILL) {
        summary[e] = s;
        link_count[e] = links;
    }
}

// ---- exclusive scan in three launches: block sums, the scan of the sums, the add -------------------------------
// dst[i] = sum of (src[j] & mask) over j < i for i < n, dst[n] = the total; src may be dst (T = int64_t).  A block
// scans SCAN_BLOCK values; scan_top_kernel is one block whose threads each take a contiguous run of the block sums,
// of more than one sum from SCAN_BLOCK * SCAN_BLOCK values on.
constexpr int SCAN_BLOCK = 256;

// exclusive scan of one value per thread over the block; *total: the block's sum (every thread)
__device__ __forceinline__ int64_t block_exclusive(int64_t v, int64_t* total) {
    __shared__ int64_t sh[SCAN_BLOCK];
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < SCAN_BLOCK; d <<= 1) {
        const int64_t add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const int64_t incl = sh[t];
    *total = sh[SCAN_BLOCK - 1];
    __syncthreads();   // sh is free for the next call
    return incl - v;
}

template <class T>
__global__ __launch_bounds__(SCAN_BLOCK)
void scan_sums_kernel(const T* src, T mask, int64_t n, int64_t* __restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    int64_t total;
    (void)block_exclusive(i < n ? (int64_t)(src[i] & mask) : 0, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[0 .. nb) -> their exclusive scan, sums[nb] = the total
__global__ __launch_bounds__(SCAN_BLOCK)
void scan_top_kernel(int64_t* __restrict__ sums, int64_t nb) {
    const int64_t per = (nb + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const int64_t b0 = threadIdx.x * per < nb ? threadIdx.x * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
    int64_t mine = 0;
    for (int64_t b = b0; b < b1; ++b) mine += sums[b];
    int64_t total;
    int64_t run = block_exclusive(mine, &total);
    for (int64_t b = b0; b < b1; ++b) {
        const int64_t v = sums[b];
        sums[b] = run;
        run += v;
    }
    if (threadIdx.x == 0) sums[nb] = total;
}

template <class T>
__global__ __launch_bounds__(SCAN_BLOCK)
void scan_add_kernel(const T* src, T mask, int64_t* dst, int64_t n, const int64_t* __restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    int64_t total;
    const int64_t ex = block_exclusive(i < n ? (int64_t)(src[i] & mask) : 0, &total);
    if (i < n) dst[i] = ex + sums[blockIdx.x];
    if (i == 0) dst[n] = sums[gridDim.x];   // no thread reads or writes dst[n] as a value: n is beyond every i
}

template <class T>
hipError_t exclusive_scan(const T* src, T mask, int64_t* dst, int64_t n, int64_t* sums, hipStream_t st) {
    const int64_t nb = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;   // n >= 1
    scan_sums_kernel<T><<<(unsigned)nb, SCAN_BLOCK, 0, st>>>(src, mask, n, sums);
    scan_top_kernel<<<1, SCAN_BLOCK, 0, st>>>(sums, nb);
    scan_add_kernel<T><<<(unsigned)nb, SCAN_BLOCK, 0, st>>>(src, mask, dst, n, sums);
    return hipGetLastError();
}

// ---- the resolution in rounds ----------------------------------------------------------------------------------
enum : int32_t { KIND_STATIC = 0, KIND_APPENDED = 1, KIND_DYNAMIC = 2 };   // bit 0: the appended flag the rank scan sums

// One thread per new element, launch `round` = 1, 2, ...: stamp[e] is 0 while e is undecided, else the round that
// decided it.  e is decided now iff every element of its link list carries a stamp of an earlier round; a stamp
// written by this launch is `round`, one not yet written is 0, and either keeps e waiting, visible or not.  The
// decision is the host loop's (5' in the head comment), statement for statement; a point appended in this call is
// n_cloud + its element, which orders as the final indices do, and has that element's coordinates.
__global__ __launch_bounds__(256)
void resolve_kernel(int n_new, int n_cloud, int32_t round, const Summary* __restrict__ summary,
                    const int64_t* __restrict__ link_off, const int32_t* __restrict__ link_list,
                    const double* __restrict__ cloud_xyz, const double* __restrict__ new_xyz, double D, int32_t* stamp,
                    int32_t* target, double* __restrict__ dist, int32_t* __restrict__ kind, int32_t* __restrict__ unresolved) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    bool left = false;
    if (e < n_new && stamp[e] == 0) {
        const int64_t k0 = link_off[e], k1 = link_off[e + 1];
        bool ready = true;
        for (int64_t k = k0; k < k1 && ready; ++k) {
            const int32_t s = *(const volatile int32_t*)(stamp + link_list[k]);
            ready = s != 0 && s < round;
        }
        if (ready) {
            Summary s = summary[e];
            const double ex[3] = {new_xyz[3 * (int64_t)e], new_xyz[3 * (int64_t)e + 1], new_xyz[3 * (int64_t)e + 2]};
            bool first_dynamic = false, min_dynamic = false;   // the slot holds a candidate only this call made
            for (int64_t k = k0; k < k1; ++k) {
                const int32_t c = target[link_list[k]];
                const double* pc = c < n_cloud ? cloud_xyz + 3 * (int64_t)c : new_xyz + 3 * (int64_t)(c - n_cloud);
                const double d = point_distance(pc, ex);
                if (d > D) continue;
                // a point that also qualifies statically never displaces the static slots: it is behind or in them
                if (s.first_idx < 0 || c < s.first_idx) { s.first_idx = c; s.first_d = d; first_dynamic = true; }
                if (d == d && (s.min_idx < 0 || d < s.min_d || (d == s.min_d && c < s.min_idx))) { s.min_idx = c; s.min_d = d; min_dynamic = true; }
            }
            if (s.first_idx < 0) {
                target[e] = n_cloud + e;
                dist[e] = -1.0;
                kind[e] = KIND_APPENDED;
            } else if (s.first_d != s.first_d) {   // best stays NaN: `best > d` is never true again
                target[e] = s.first_idx;
                dist[e] = s.first_d;
                kind[e] = first_dynamic ? KIND_DYNAMIC : KIND_STATIC;
            } else {
                target[e] = s.min_idx;
                dist[e] = s.min_d;
                kind[e] = min_dynamic ? KIND_DYNAMIC : KIND_STATIC;
            }
            stamp[e] = round;
        } else {
            left = true;
        }
    }
    const int n = __syncthreads_count(left);
    if (threadIdx.x == 0 && n) atomicAdd(unresolved, n);
}

// After the last round, rank = the exclusive scan of the appended flags: the final target of every element, the
// appended elements in rank order for scatter_kernel, the number of elements merged into each output point and the
// two statistics (block counts, one integer atomic each per block).
__global__ __launch_bounds__(256)
void finalize_kernel(int n_new, int n_cloud, const int64_t* __restrict__ rank, const int32_t* __restrict__ kind,
                     const int32_t* __restrict__ provisional, int32_t* __restrict__ out_target, int32_t* __restrict__ appended,
                     int32_t* __restrict__ group_count, Words* __restrict__ w) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    int32_t k = -1;
    if (e < n_new) {
        k = kind[e];
        int32_t t = provisional[e];
        if (t >= n_cloud) t = n_cloud + (int32_t)rank[t - n_cloud];
        out_target[e] = t;
        if (k == KIND_APPENDED) appended[rank[e]] = e;
        else atomicAdd(group_count + t, 1);
    }
    const int ns = __syncthreads_count(k == KIND_STATIC), nd = __syncthreads_count(k == KIND_DYNAMIC);
    if (threadIdx.x == 0) {
        if (ns) atomicAdd(&w->merged_static, (unsigned long long)ns);
        if (nd) atomicAdd(&w->merged_dynamic, (unsigned long long)nd);
    }
}

// every merged element into its target's group, in any order (walk_kernel sorts the group)
__global__ __launch_bounds__(256)
void group_fill_kernel(int n_new, const int32_t* __restrict__ kind, const int32_t* __restrict__ target,
                       const int64_t* __restrict__ group_start, int32_t* __restrict__ cursor, int32_t* __restrict__ group_elem) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_new || kind[e] == KIND_APPENDED) return;
    const int32_t t = target[e];
    group_elem[group_start[t] + atomicAdd(cursor + t, 1)] = e;
}

// One thread per output point (of at most n_cloud + n_new; rank[n_new] is the number appended): its group sorted by
// element index, which is merge order, then the walk of 5b: a new record is held iff it equals one of the point's
// initial records or a record accepted earlier in this walk (shot ==, x ==, y == in double).  local[r]: the record's
// position in the point's output list, -1 if held; an appended element's own records open its point's list.
// size[c]: the point's output records.
__global__ __launch_bounds__(256)
void walk_kernel(int n_total, int n_cloud, int n_new, const int64_t* __restrict__ rank, const int32_t* __restrict__ appended,
                 const int64_t* __restrict__ group_start, int32_t* group_elem, const int64_t* __restrict__ cloud_off,
                 const int32_t* __restrict__ cloud_shot, const double* __restrict__ cloud_xy,
                 const int64_t* __restrict__ new_off, const int32_t* __restrict__ new_shot,
                 const double* __restrict__ new_xy, int64_t* local, int64_t* __restrict__ size) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_total) return;
    if (c >= n_cloud + (int)rank[n_new]) { size[c] = 0; return; }
    const int e0 = c < n_cloud ? -1 : appended[c - n_cloud];
    const int64_t i0 = e0 < 0 ? cloud_off[c] : new_off[e0], ni = (e0 < 0 ? cloud_off[c + 1] : new_off[e0 + 1]) - i0;
    const int32_t* is = (e0 < 0 ? cloud_shot : new_shot) + i0;
    const double* ixy = (e0 < 0 ? cloud_xy : new_xy) + 2 * i0;
    if (e0 >= 0)
        for (int64_t k = 0; k < ni; ++k) local[i0 + k] = k;   // appended as given
    const int64_t g0 = group_start[c], g1 = group_start[c + 1];
    for (int64_t a = g0 + 1; a < g1; ++a) {   // insertion sort: the groups are short
        const int32_t v = group_elem[a];
        int64_t b = a;
        for (; b > g0 && group_elem[b - 1] > v; --b) group_elem[b] = group_elem[b - 1];
        group_elem[b] = v;
    }
    int64_t added = 0;
    for (int64_t g = g0; g < g1; ++g) {
        const int e = group_elem[g];
        for (int64_t r = new_off[e]; r < new_off[e + 1]; ++r) {
            const int32_t rs = new_shot[r];
            const double rx = new_xy[2 * r], ry = new_xy[2 * r + 1];
            bool held = false;
            for (int64_t k = 0; k < ni && !held; ++k) held = is[k] == rs && ixy[2 * k] == rx && ixy[2 * k + 1] == ry;
            for (int64_t g2 = g0; g2 <= g && !held; ++g2) {   // the records accepted so far, in walk order
                const int e2 = group_elem[g2];
                const int64_t q1 = g2 == g ? r : new_off[e2 + 1];
                for (int64_t q = new_off[e2]; q < q1 && !held; ++q)
                    held = local[q] >= 0 && new_shot[q] == rs && new_xy[2 * q] == rx && new_xy[2 * q + 1] == ry;
            }
            local[r] = held ? -1 : ni + added++;
        }
    }
    size[c] = ni + added;
}

// one thread per new record: its local position -> its place in the output CSR
__global__ __launch_bounds__(256)
void dest_kernel(int64_t n_nrec, const int32_t* __restrict__ rec_elem, const int32_t* __restrict__ target,
                 const int64_t* __restrict__ out_off, int64_t* __restrict__ dest) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_nrec) return;
    const int64_t p = dest[r];
    if (p >= 0) dest[r] = out_off[target[rec_elem[r]]] + p;
}

// one thread per cloud record, new record and output point
__global__ __launch_bounds__(256)
void scatter_kernel(int64_t n_crec, int64_t n_nrec, int n_cloud, int n_out, const int64_t* __restrict__ cloud_off,
                    const int32_t* __restrict__ crec_point, const int32_t* __restrict__ cloud_shot,
                    const double* __restrict__ cloud_xy, const double* __restrict__ cloud_xyz,
                    const int32_t* __restrict__ new_shot, const double* __restrict__ new_xy,
                    const double* __restrict__ new_xyz, const int64_t* __restrict__ new_dest,
                    const int32_t* __restrict__ appended, const int64_t* __restrict__ out_off,
                    int32_t* __restrict__ out_shot, double* __restrict__ out_xy, double* __restrict__ out_xyz) {
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n_crec) {   // old records keep their place at the head of their point's list
        const int p = crec_point[g];
        const int64_t dst = out_off[p] + (g - cloud_off[p]);
        out_shot[dst] = cloud_shot[g];
        out_xy[2 * dst] = cloud_xy[2 * g];
        out_xy[2 * dst + 1] = cloud_xy[2 * g + 1];
        return;
    }
    g -= n_crec;
    if (g < n_nrec) {
        const int64_t dst = new_dest[g];
        if (dst < 0) return;   // a record its target already held
        out_shot[dst] = new_shot[g];
        out_xy[2 * dst] = new_xy[2 * g];
        out_xy[2 * dst + 1] = new_xy[2 * g + 1];
        return;
    }
    g -= n_nrec;
    if (g < n_out) {
        const double* src = g < n_cloud ? cloud_xyz + 3 * g : new_xyz + 3 * (int64_t)appended[g - n_cloud];
        out_xyz[3 * g] = src[0];
        out_xyz[3 * g + 1] = src[1];
        out_xyz[3 * g + 2] = src[2];
    }
}

// The default cap on the resolve rounds (measured): a round is one launch and one word read, about
// 0.1 ms at 556 207 elements and less for a pair's worth; the host path it gives way to costs as much as some
// 2300 such rounds on that batch and 50 on a call of the reconstruction loop, and the batch needs 102.  The cap is
// for chains as long as the batch itself: it bounds what such a call spends before it falls back at about 0.1 s.
constexpr int32_t DEFAULT_MAX_ROUNDS = 1024;

thread_local float g_last_ms = -1.f;
thread_local int64_t g_last_stats[3] = {0, 0, 0};   // merges decided statically, dynamically; new-new links
thread_local int32_t g_max_rounds = 0;              // sfmx_merge_pointcloud_set_max_rounds
thread_local int32_t g_last_rounds = 0, g_last_fallback = 0;
thread_local int64_t g_last_bytes = 0;
Slot g_slot[64];        // csrc/device_call.hpp: the block of a call
Slot g_link_slot[64];   // the link list, whose length only the first probe gives: a block of its own, taken after g_slot's

}  // namespace merge
}  // namespace sfmx

using namespace sfmx;
using namespace sfmx::merge;

extern "C" {

float sfmx_merge_pointcloud_last_kernel_ms(void) { return g_last_ms; }

int sfmx_merge_pointcloud_last_stats(int64_t* merged_static, int64_t* merged_dynamic, int64_t* links) {
    if (merged_static) *merged_static = g_last_stats[0];
    if (merged_dynamic) *merged_dynamic = g_last_stats[1];
    if (links) *links = g_last_stats[2];
    return SFMX_OK;
}

int sfmx_merge_pointcloud_set_max_rounds(int32_t max_rounds) {
    g_max_rounds = max_rounds;
    return SFMX_OK;
}

int sfmx_merge_pointcloud_last_path(int32_t* rounds, int32_t* host_fallback, int64_t* host_bytes) {
    if (rounds) *rounds = g_last_rounds;
    if (host_fallback) *host_fallback = g_last_fallback;
    if (host_bytes) *host_bytes = g_last_bytes;
    return SFMX_OK;
}

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
                               int64_t* out_n_origins) {
    g_last_rounds = g_last_fallback = 0;
    g_last_bytes = 0;
    if (n_shots < 0 || n_pairs < 0 || n_cloud < 0 || n_new < 0) { set_last_error("negative count"); return SFMX_EINVAL; }
    if ((int64_t)n_cloud + n_new > INT32_MAX) { set_last_error("cloud and new points together exceed the int32 range"); return SFMX_EINVAL; }
    if (point_merge_distance != point_merge_distance || feature_merge_distance != feature_merge_distance) {
        set_last_error("a merge distance is NaN");
        return SFMX_EINVAL;
    }
    if ((n_shots && (!keypoints || !n_keypoints)) || (n_pairs && (!pairs || !pair_offsets)) || !cloud_origin_offsets ||
        !new_origin_offsets || (n_cloud && !cloud_xyz) || (n_new && (!new_xyz || !out_target || !out_merge_distance)) ||
        !out_origin_offsets || !out_n_points || !out_n_origins || (n_cloud + n_new && !out_xyz)) {
        set_last_error("null argument");
        return SFMX_EINVAL;
    }
    if (!plan::shots_in_range(pairs, n_pairs, n_shots)) { set_last_error("pair shot index out of range"); return SFMX_EINVAL; }
    const double D = point_merge_distance, F = feature_merge_distance;
    DeviceCall call(stream, !inputs_on_device);   // opened where a device is first needed: a host call with nothing new opens none
    DeviceCall link_call(stream, false);          // the link list's block
    const hipStream_t st = call.st;
    const bool H = call.host;
    int rc = SFMX_OK;
    int64_t xfer = 0;   // bytes copied host -> device and device -> host
    try {
        // host copies of what the host reads: the pair offsets always; the rest only on the host resolution's path
        // (staged from the device when inputs_on_device)
        std::vector<int64_t> hoff(n_pairs + 1, 0), hco, hno;
        std::vector<int32_t> hcs, hns;
        std::vector<double> hcxy, hnxy, hcx, hnx;
        // and of what comes back from the kernels or goes up to them; all alive until the frame's tail has drained the stream
        std::vector<Summary> hs;
        std::vector<int32_t> hlist, htarget, happ;
        std::vector<int64_t> hloff, hdest, hout;
        std::vector<double> hdist;
        int32_t hflags[2] = {0, 0}, hleft = 0;   // Words::full, Words::bad; Words::unresolved
        int64_t hlast[2] = {0, 0}, hlinks = 0, hcounts[2] = {0, 0};
        unsigned long long hstat[2] = {0, 0};
        const int64_t *co = cloud_origin_offsets, *no = new_origin_offsets;
        const int32_t *cs = cloud_origin_shot, *ns = new_origin_shot;
        const double *cxy = cloud_origin_xy, *nxy = new_origin_xy, *cx = cloud_xyz, *nx = new_xyz;
        int64_t n_crec = 0, n_nrec = 0, n_matches = 0;
        if (!H) {   // of the inputs the host reads the pair offsets and the two record counts
            const int orc = call.open(g_slot, device);
            if (orc != SFMX_OK) return orc;
            if (n_pairs) {
                SFMX_HIP_CHK(hipMemcpyAsync(hoff.data(), pair_offsets, sizeof(int64_t) * (n_pairs + 1), hipMemcpyDeviceToHost, st));
                xfer += sizeof(int64_t) * (n_pairs + 1);
            }
            SFMX_HIP_CHK(hipMemcpyAsync(&hlast[0], cloud_origin_offsets + n_cloud, sizeof(int64_t), hipMemcpyDeviceToHost, st));
            SFMX_HIP_CHK(hipMemcpyAsync(&hlast[1], new_origin_offsets + n_new, sizeof(int64_t), hipMemcpyDeviceToHost, st));
            xfer += 2 * sizeof(int64_t);
            SFMX_HIP_CHK(hipStreamSynchronize(st));
            n_crec = hlast[0];
            n_nrec = hlast[1];
        } else {
            if (n_pairs) std::memcpy(hoff.data(), pair_offsets, sizeof(int64_t) * (n_pairs + 1));
            if (!plan::offsets_ascend(co, n_cloud)) { set_last_error("cloud origin offsets do not ascend from 0"); rc = SFMX_EINVAL; goto done; }
            if (!plan::offsets_ascend(no, n_new)) { set_last_error("new origin offsets do not ascend from 0"); rc = SFMX_EINVAL; goto done; }
            n_crec = co[n_cloud];
            n_nrec = no[n_new];
        }
        if (!plan::offsets_ascend(hoff.data(), n_pairs)) { set_last_error("pair offsets do not ascend from 0"); rc = SFMX_EINVAL; goto done; }
        if (n_crec < 0) { set_last_error("cloud origin offsets do not ascend from 0"); rc = SFMX_EINVAL; goto done; }
        if (n_nrec < 0) { set_last_error("new origin offsets do not ascend from 0"); rc = SFMX_EINVAL; goto done; }
        n_matches = hoff[n_pairs];
        // table capacities (2 x entries, rounded up to a power of two) and entry indices stay within 32 bits
        if (n_crec > (1 << 30) || n_nrec > (1 << 30) || n_matches > (1 << 29)) {
            set_last_error("too many origin records or matches for one call");
            rc = SFMX_ECAPACITY;
            goto done;
        }
        if ((n_crec && (!cloud_origin_shot || !cloud_origin_xy)) || (n_nrec && (!new_origin_shot || !new_origin_xy)) ||
            (n_crec + n_nrec && (!out_origin_shot || !out_origin_xy)) || (n_matches && !matches)) {
            set_last_error("null argument");
            rc = SFMX_EINVAL;
            goto done;
        }
        if (H) {
            for (int64_t r = 0; r < n_crec; ++r)
                if (cs[r] < 0 || cs[r] >= n_shots) { set_last_error("cloud origin shot out of range"); rc = SFMX_EINVAL; goto done; }
            for (int64_t r = 0; r < n_nrec; ++r)
                if (ns[r] < 0 || ns[r] >= n_shots) { set_last_error("new origin shot out of range"); rc = SFMX_EINVAL; goto done; }
        }

        if (n_new == 0) {   // nothing to merge: the cloud goes through unchanged, with device inputs after their check
            if (!H) {
                BlockLayout L0;
                Words* w0;
                L0.want(w0, 1);
                if ((rc = call.reserve(L0, 0)) != SFMX_OK) goto done;
                SFMX_HIP_CHK(hipMemsetAsync(w0, 0, sizeof(Words), st));
                {
                    const int64_t items = (int64_t)n_cloud + 2 + n_crec;
                    validate_kernel<<<(unsigned)((items + 255) / 256), 256, 0, st>>>(n_cloud, 0, n_crec, 0, n_shots, cloud_origin_offsets,
                                                                                    new_origin_offsets, cloud_origin_shot, new_origin_shot,
                                                                                    &w0->bad);
                }
                SFMX_HIP_CHK(hipGetLastError());
                SFMX_HIP_CHK(hipMemcpyAsync(&hflags[1], &w0->bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
                xfer += sizeof(int32_t);
                if (n_cloud) SFMX_HIP_CHK(hipMemcpyAsync(out_xyz, cloud_xyz, sizeof(double) * 3 * n_cloud, hipMemcpyDeviceToDevice, st));
                SFMX_HIP_CHK(hipMemcpyAsync(out_origin_offsets, cloud_origin_offsets, sizeof(int64_t) * (n_cloud + 1), hipMemcpyDeviceToDevice, st));
                if (n_crec) {
                    SFMX_HIP_CHK(hipMemcpyAsync(out_origin_shot, cloud_origin_shot, sizeof(int32_t) * n_crec, hipMemcpyDeviceToDevice, st));
                    SFMX_HIP_CHK(hipMemcpyAsync(out_origin_xy, cloud_origin_xy, sizeof(double) * 2 * n_crec, hipMemcpyDeviceToDevice, st));
                }
                SFMX_HIP_CHK(hipStreamSynchronize(st));
                if (hflags[1]) { set_last_error(bad_input(hflags[1])); rc = SFMX_EINVAL; goto done; }
            } else {
                if (n_cloud) std::memcpy(out_xyz, cloud_xyz, sizeof(double) * 3 * n_cloud);
                std::memcpy(out_origin_offsets, cloud_origin_offsets, sizeof(int64_t) * (n_cloud + 1));
                if (n_crec) {
                    std::memcpy(out_origin_shot, cloud_origin_shot, sizeof(int32_t) * n_crec);
                    std::memcpy(out_origin_xy, cloud_origin_xy, sizeof(double) * 2 * n_crec);
                }
            }
            *out_n_points = n_cloud;
            *out_n_origins = n_crec;
            g_last_ms = 0.f;
            g_last_stats[0] = g_last_stats[1] = g_last_stats[2] = 0;
            goto done;
        }

        if (H) {
            const int orc = call.open(g_slot, device);
            if (orc != SFMX_OK) return orc;
        }
        if (H && !plan::counts_non_negative(n_keypoints, n_shots)) { set_last_error("negative keypoint count"); rc = SFMX_EINVAL; goto done; }
        {
            Slot* const S = call.S;
            // 1. first pair per unordered shot pair: the only one whose matches link anything
            std::vector<int32_t> pair_first;
            const int64_t link_matches = plan::first_pairs(pairs, n_pairs, n_shots, hoff.data(), pair_first);
            const uint32_t lcap = (uint32_t)plan::capacity_for(2 * link_matches), ccap = (uint32_t)plan::capacity_for(n_crec),
                           ncap = (uint32_t)plan::capacity_for(n_nrec);
            const int n_total = n_cloud + n_new;
            const unsigned eb = (unsigned)((n_new + 255) / 256);
            const int32_t cap = g_max_rounds < 0 ? 0 : g_max_rounds == 0 ? DEFAULT_MAX_ROUNDS : g_max_rounds;
            int n_app = 0, n_out = 0;
            int64_t n_orec = 0;
            float ms = 0.f, part = 0.f;
            int64_t nk = 0;
            for (int i = 0; H && i < n_shots; ++i) nk += n_keypoints[i];

            // device block: [tables of the call | work buffers | (host inputs: graph, both clouds, the output cloud)]
            BlockLayout L;
            const float2** kpd;
            int32_t *nkd, *prd, *pfd, *lslot, *cslot, *nslot, *ent_shot, *crec_point, *nrec_elem, *lcount, *appd, *csd, *nsd, *osd;
            int32_t *stamp, *ptarget, *kind, *gcount, *gcursor, *gelem, *tgd;
            int64_t *loff, *ndest, *od, *cod, *nod, *ood, *rank, *gstart, *sums;
            unsigned long long* ent_pos;
            Summary* summ;
            Words* wd;
            float2* kd;
            sfmx_dmatch* md;
            double *cxyd, *nxyd, *cxd, *nxd, *oxyd, *oxd, *dsd;
            L.want(kpd, n_shots);
            L.want(nkd, n_shots);
            L.want(prd, 2 * (size_t)n_pairs);
            L.want(pfd, n_pairs);
            const size_t b_tab = L.need;   // up to here: staged in pinned memory, one upload
            L.want(lslot, lcap);
            L.want(cslot, ccap);
            L.want(nslot, ncap);
            L.want(ent_shot, 2 * (size_t)n_matches);
            L.want(ent_pos, 2 * (size_t)n_matches);
            L.want(crec_point, n_crec);
            L.want(nrec_elem, n_nrec);
            L.want(wd, 1);
            L.want(summ, n_new);
            L.want(lcount, n_new);
            L.want(loff, (size_t)n_new + 1);
            L.want(ndest, n_nrec);
            L.want(appd, n_new);
            L.want(stamp, n_new);
            L.want(ptarget, n_new);
            L.want(kind, n_new);
            L.want(rank, (size_t)n_new + 1);
            L.want(gcount, n_total);
            L.want(gcursor, n_total);
            L.want(gstart, (size_t)n_total + 1);
            L.want(gelem, n_new);
            L.want(sums, (size_t)n_total / SCAN_BLOCK + 2);
            L.want(kd, nk, H);
            L.want(md, n_matches, H);
            L.want(od, (size_t)n_pairs + 1, H);
            L.want(cod, (size_t)n_cloud + 1, H);
            L.want(nod, (size_t)n_new + 1, H);
            L.want(csd, n_crec, H);
            L.want(nsd, n_nrec, H);
            L.want(cxyd, 2 * (size_t)n_crec, H);
            L.want(nxyd, 2 * (size_t)n_nrec, H);
            L.want(cxd, 3 * (size_t)n_cloud, H);
            L.want(nxd, 3 * (size_t)n_new, H);
            L.want(osd, (size_t)(n_crec + n_nrec), H);
            L.want(oxyd, 2 * (size_t)(n_crec + n_nrec), H);
            L.want(oxd, 3 * (size_t)n_total, H);
            L.want(ood, (size_t)n_total + 1, H);
            L.want(tgd, n_new, H);
            L.want(dsd, n_new, H);
            rc = call.reserve(L, b_tab);
            if (rc != SFMX_OK) goto done;
            if (n_shots) std::memcpy(call.pinned(nkd), n_keypoints, sizeof(int32_t) * n_shots);
            if (n_pairs) {
                std::memcpy(call.pinned(prd), pairs, sizeof(int32_t) * 2 * n_pairs);
                std::memcpy(call.pinned(pfd), pair_first.data(), sizeof(int32_t) * n_pairs);
            }
            const float2** hk = call.pinned(kpd);
            int64_t o = 0;
            for (int i = 0; i < n_shots; ++i) {
                if (H) {
                    if (n_keypoints[i]) SFMX_HIP_CHK(hipMemcpyAsync(kd + o, keypoints[i], sizeof(float2) * n_keypoints[i], hipMemcpyHostToDevice, st));
                    hk[i] = kd + o;
                    o += n_keypoints[i];
                } else {
                    hk[i] = reinterpret_cast<const float2*>(keypoints[i]);
                }
            }
            SFMX_HIP_CHK(call.upload(b_tab));
            xfer += (int64_t)b_tab;
            if (H)   // the uploads of call.in below
                xfer += (int64_t)(sizeof(float2) * nk + sizeof(sfmx_dmatch) * n_matches + sizeof(int64_t) * (n_pairs ? n_pairs + 1 : 0) +
                                  sizeof(int64_t) * ((size_t)n_total + 2) + (sizeof(int32_t) + 2 * sizeof(double)) * (n_crec + n_nrec) +
                                  sizeof(double) * 3 * (size_t)n_total);
            // what the kernels read and write: the caller's device arrays or the staging copies
            const DMatchDev* dm = reinterpret_cast<const DMatchDev*>(n_matches ? call.in(matches, md, n_matches) : matches);
            const int64_t* doff = n_pairs ? call.in(pair_offsets, od, (size_t)n_pairs + 1) : pair_offsets;
            const int64_t* dco = call.in(cloud_origin_offsets, cod, (size_t)n_cloud + 1);
            const int64_t* dno = call.in(new_origin_offsets, nod, (size_t)n_new + 1);
            const int32_t* dcs = n_crec ? call.in(cloud_origin_shot, csd, n_crec) : cloud_origin_shot;
            const int32_t* dns = n_nrec ? call.in(new_origin_shot, nsd, n_nrec) : new_origin_shot;
            const double* dcxy = n_crec ? call.in(cloud_origin_xy, cxyd, 2 * (size_t)n_crec) : cloud_origin_xy;
            const double* dnxy = n_nrec ? call.in(new_origin_xy, nxyd, 2 * (size_t)n_nrec) : new_origin_xy;
            const double* dcx = n_cloud ? call.in(cloud_xyz, cxd, 3 * (size_t)n_cloud) : cloud_xyz;
            const double* dnx = call.in(new_xyz, nxd, 3 * (size_t)n_new);
            SFMX_HIP_CHK(call.err);
            int32_t *do_shot = call.out(out_origin_shot, osd), *do_target = call.out(out_target, tgd);
            double *do_xy = call.out(out_origin_xy, oxyd), *do_xyz = call.out(out_xyz, oxd), *do_dist = call.out(out_merge_distance, dsd);
            int64_t* do_off = call.out(out_origin_offsets, ood);
            const Table tc{cslot, ccap, dcs, dcxy, crec_point}, tn{nslot, ncap, dns, dnxy, nrec_elem};
            int32_t* const full = &wd->full;
            const int32_t* const bad = &wd->bad;

            // 2-4. input check (device inputs), tables, static probe, link counts and their scan.  A timed span runs
            //      from S->e0 to S->e1 and ends in a stream synchronisation, after which its time is read and the
            //      slot's two events are free for the next.
            SFMX_HIP_CHK(hipEventRecord(S->e0, st));
            SFMX_HIP_CHK(hipMemsetAsync(lslot, 0xff, sizeof(int32_t) * lcap, st));
            SFMX_HIP_CHK(hipMemsetAsync(cslot, 0xff, sizeof(int32_t) * ccap, st));
            SFMX_HIP_CHK(hipMemsetAsync(nslot, 0xff, sizeof(int32_t) * ncap, st));
            SFMX_HIP_CHK(hipMemsetAsync(wd, 0, sizeof(Words), st));
            if (!H) {
                const int64_t items = (int64_t)n_total + 2 + n_crec + n_nrec;
                validate_kernel<<<(unsigned)((items + 255) / 256), 256, 0, st>>>(n_cloud, n_new, n_crec, n_nrec, n_shots, dco, dno, dcs, dns,
                                                                                &wd->bad);
            }
            if (n_matches && link_matches)
                build_links_kernel<<<(unsigned)((n_matches + 255) / 256), 256, 0, st>>>(n_matches, n_pairs, doff, pfd, prd, dm, kpd, nkd,
                                                                                       F, lslot, lcap, ent_shot, ent_pos, full);
            if (n_crec)
                build_records_kernel<<<(unsigned)((n_crec + 255) / 256), 256, 0, st>>>(n_crec, n_cloud, dco, dcs, dcxy, cslot, ccap,
                                                                                     crec_point, full, bad);
            if (n_nrec)
                build_records_kernel<<<(unsigned)((n_nrec + 255) / 256), 256, 0, st>>>(n_nrec, n_new, dno, dns, dnxy, nslot, ncap,
                                                                                     nrec_elem, full, bad);
            probe_kernel<false><<<eb, 256, 0, st>>>(n_new, dno, dns, dnxy, dnx, dcx, D, lslot, lcap, ent_shot, ent_pos, tc, tn, summ,
                                                    lcount, nullptr, nullptr, bad);
            SFMX_HIP_CHK(hipGetLastError());
            SFMX_HIP_CHK(exclusive_scan<int32_t>(lcount, -1, loff, n_new, sums, st));
            SFMX_HIP_CHK(hipEventRecord(S->e1, st));
            SFMX_HIP_CHK(hipMemcpyAsync(hflags, wd, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            SFMX_HIP_CHK(hipMemcpyAsync(&hlinks, loff + n_new, sizeof(int64_t), hipMemcpyDeviceToHost, st));
            xfer += 2 * sizeof(int32_t) + sizeof(int64_t);
            SFMX_HIP_CHK(hipStreamSynchronize(st));
            if (hipEventElapsedTime(&part, S->e0, S->e1) == hipSuccess) ms += part;
            if (hflags[1]) { set_last_error(bad_input(hflags[1])); rc = SFMX_EINVAL; goto done; }   // before the link count, which then means nothing
            if (hflags[0]) { set_last_error("a merge hash table filled up"); rc = SFMX_EINTERNAL; goto done; }
            if (hlinks >= INT32_MAX) {
                set_last_error("more than 2^31 links between the new elements: merge them in several calls");
                rc = SFMX_ECAPACITY;
                goto done;
            }
            int32_t* llist = nullptr;
            SFMX_HIP_CHK(hipEventRecord(S->e0, st));   // the span of the link fill and, if any, the first round
            if (hlinks) {
                BlockLayout LL;
                LL.want(llist, (size_t)hlinks);
                const int orc = link_call.open(g_link_slot, device);   // the stream is idle here
                if (orc != SFMX_OK) return orc;
                if ((rc = link_call.reserve(LL, 0)) != SFMX_OK) goto done;
                probe_kernel<true><<<eb, 256, 0, st>>>(n_new, dno, dns, dnxy, dnx, dcx, D, lslot, lcap, ent_shot, ent_pos, tc, tn,
                                                       nullptr, nullptr, loff, llist, bad);
                SFMX_HIP_CHK(hipGetLastError());
            }
            g_last_stats[2] = hlinks;

            // 5. the resolution in rounds: one word back per round, until none is left or the cap is reached
            bool decided = false;
            if (cap > 0) {
                int32_t rounds = 0;
                SFMX_HIP_CHK(hipMemsetAsync(stamp, 0, sizeof(int32_t) * n_new, st));
                hleft = n_new;
                while (hleft && rounds < cap) {
                    ++rounds;
                    if (rounds > 1) SFMX_HIP_CHK(hipEventRecord(S->e0, st));
                    SFMX_HIP_CHK(hipMemsetAsync(&wd->unresolved, 0, sizeof(int32_t), st));
                    resolve_kernel<<<eb, 256, 0, st>>>(n_new, n_cloud, rounds, summ, loff, llist, dcx, dnx, D, stamp, ptarget, do_dist,
                                                       kind, &wd->unresolved);
                    SFMX_HIP_CHK(hipGetLastError());
                    SFMX_HIP_CHK(hipEventRecord(S->e1, st));
                    SFMX_HIP_CHK(hipMemcpyAsync(&hleft, &wd->unresolved, sizeof(int32_t), hipMemcpyDeviceToHost, st));
                    xfer += sizeof(int32_t);
                    SFMX_HIP_CHK(hipStreamSynchronize(st));
                    if (hipEventElapsedTime(&part, S->e0, S->e1) == hipSuccess) ms += part;
                    g_last_rounds = rounds;
                }
                decided = hleft == 0;
                if (!decided) SFMX_HIP_CHK(hipEventRecord(S->e0, st));   // the fallback closes a span: an empty one here, the link fill went with round 1
            }

            if (decided) {
                // 5b. final targets, groups, walk, offsets, destinations (one timed span)
                SFMX_HIP_CHK(hipEventRecord(S->e0, st));
                SFMX_HIP_CHK(hipMemsetAsync(gcount, 0, sizeof(int32_t) * n_total, st));
                SFMX_HIP_CHK(hipMemsetAsync(gcursor, 0, sizeof(int32_t) * n_total, st));
                SFMX_HIP_CHK(exclusive_scan<int32_t>(kind, KIND_APPENDED, rank, n_new, sums, st));
                finalize_kernel<<<eb, 256, 0, st>>>(n_new, n_cloud, rank, kind, ptarget, do_target, appd, gcount, wd);
                SFMX_HIP_CHK(hipGetLastError());
                SFMX_HIP_CHK(exclusive_scan<int32_t>(gcount, -1, gstart, n_total, sums, st));
                group_fill_kernel<<<eb, 256, 0, st>>>(n_new, kind, do_target, gstart, gcursor, gelem);
                walk_kernel<<<(unsigned)((n_total + 255) / 256), 256, 0, st>>>(n_total, n_cloud, n_new, rank, appd, gstart, gelem, dco, dcs,
                                                                              dcxy, dno, dns, dnxy, ndest, do_off);
                SFMX_HIP_CHK(hipGetLastError());
                SFMX_HIP_CHK(exclusive_scan<int64_t>(do_off, -1, do_off, n_total, sums, st));
                if (n_nrec) dest_kernel<<<(unsigned)((n_nrec + 255) / 256), 256, 0, st>>>(n_nrec, nrec_elem, do_target, do_off, ndest);
                SFMX_HIP_CHK(hipGetLastError());
                SFMX_HIP_CHK(hipEventRecord(S->e1, st));
                SFMX_HIP_CHK(hipMemcpyAsync(&hcounts[0], rank + n_new, sizeof(int64_t), hipMemcpyDeviceToHost, st));
                SFMX_HIP_CHK(hipMemcpyAsync(&hcounts[1], do_off + n_total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
                SFMX_HIP_CHK(hipMemcpyAsync(hstat, &wd->merged_static, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
                xfer += 4 * sizeof(int64_t);
                SFMX_HIP_CHK(hipStreamSynchronize(st));
                if (hipEventElapsedTime(&part, S->e0, S->e1) == hipSuccess) ms += part;
                n_app = (int)hcounts[0];
                n_out = n_cloud + n_app;
                n_orec = hcounts[1];
                g_last_stats[0] = (int64_t)hstat[0];
                g_last_stats[1] = (int64_t)hstat[1];
            } else {
                // 5'. the host resolution, from element 0: the summaries, the link lists and, with device inputs, both clouds
                g_last_fallback = 1;
                hs.resize(n_new); htarget.resize(n_new); hdist.resize(n_new); happ.reserve(n_new);
                hloff.assign((size_t)n_new + 1, 0); hlist.resize(hlinks); hdest.assign(n_nrec, -1); hout.assign((size_t)n_total + 1, 0);
                if (!H) {
                    hco.resize((size_t)n_cloud + 1); hno.resize((size_t)n_new + 1);
                    hcs.resize(n_crec); hcxy.resize(2 * n_crec); hcx.resize(3 * (size_t)n_cloud);
                    hns.resize(n_nrec); hnxy.resize(2 * n_nrec); hnx.resize(3 * (size_t)n_new);
                }
                SFMX_HIP_CHK(hipEventRecord(S->e1, st));
                SFMX_HIP_CHK(hipMemcpyAsync(hs.data(), summ, sizeof(Summary) * n_new, hipMemcpyDeviceToHost, st));
                SFMX_HIP_CHK(hipMemcpyAsync(hloff.data(), loff, sizeof(int64_t) * (n_new + 1), hipMemcpyDeviceToHost, st));
                xfer += (int64_t)(sizeof(Summary) * n_new + sizeof(int64_t) * (n_new + 1));
                if (hlinks) {
                    SFMX_HIP_CHK(hipMemcpyAsync(hlist.data(), llist, sizeof(int32_t) * hlinks, hipMemcpyDeviceToHost, st));
                    xfer += (int64_t)sizeof(int32_t) * hlinks;
                }
                if (!H) {
                    SFMX_HIP_CHK(hipMemcpyAsync(hco.data(), cloud_origin_offsets, sizeof(int64_t) * (n_cloud + 1), hipMemcpyDeviceToHost, st));
                    SFMX_HIP_CHK(hipMemcpyAsync(hno.data(), new_origin_offsets, sizeof(int64_t) * (n_new + 1), hipMemcpyDeviceToHost, st));
                    if (n_crec) {
                        SFMX_HIP_CHK(hipMemcpyAsync(hcs.data(), cloud_origin_shot, sizeof(int32_t) * n_crec, hipMemcpyDeviceToHost, st));
                        SFMX_HIP_CHK(hipMemcpyAsync(hcxy.data(), cloud_origin_xy, sizeof(double) * 2 * n_crec, hipMemcpyDeviceToHost, st));
                    }
                    if (n_nrec) {
                        SFMX_HIP_CHK(hipMemcpyAsync(hns.data(), new_origin_shot, sizeof(int32_t) * n_nrec, hipMemcpyDeviceToHost, st));
                        SFMX_HIP_CHK(hipMemcpyAsync(hnxy.data(), new_origin_xy, sizeof(double) * 2 * n_nrec, hipMemcpyDeviceToHost, st));
                    }
                    if (n_cloud) SFMX_HIP_CHK(hipMemcpyAsync(hcx.data(), cloud_xyz, sizeof(double) * 3 * n_cloud, hipMemcpyDeviceToHost, st));
                    SFMX_HIP_CHK(hipMemcpyAsync(hnx.data(), new_xyz, sizeof(double) * 3 * n_new, hipMemcpyDeviceToHost, st));
                    xfer += (int64_t)(sizeof(int64_t) * ((size_t)n_total + 2) + (sizeof(int32_t) + 2 * sizeof(double)) * (n_crec + n_nrec) +
                                      sizeof(double) * 3 * (size_t)n_total);
                    co = hco.data(); no = hno.data();
                    cs = hcs.data(); cxy = hcxy.data(); cx = hcx.data();
                    ns = hns.data(); nxy = hnxy.data(); nx = hnx.data();
                }
                SFMX_HIP_CHK(hipStreamSynchronize(st));
                if (hipEventElapsedTime(&part, S->e0, S->e1) == hipSuccess) ms += part;

                // 5'a. targets, in element order (Scene.cpp:532-538 fold, :552-567 merge or append)
                int64_t n_static = 0, n_dynamic = 0;
                for (int e = 0; e < n_new; ++e) {
                    Summary s = hs[e];
                    bool first_dynamic = false, min_dynamic = false;   // the slot holds a candidate only this call made
                    for (int64_t k = hloff[e]; k < hloff[e + 1]; ++k) {
                        const int32_t c = htarget[hlist[k]];
                        const double* pc = c < n_cloud ? cx + 3 * (int64_t)c : nx + 3 * (int64_t)happ[c - n_cloud];
                        const double d = point_distance(pc, nx + 3 * (int64_t)e);
                        if (d > D) continue;
                        // a point that also qualifies statically never displaces the static slots: it is behind or in them
                        if (s.first_idx < 0 || c < s.first_idx) { s.first_idx = c; s.first_d = d; first_dynamic = true; }
                        if (d == d && (s.min_idx < 0 || d < s.min_d || (d == s.min_d && c < s.min_idx))) { s.min_idx = c; s.min_d = d; min_dynamic = true; }
                    }
                    if (s.first_idx < 0) {
                        htarget[e] = n_cloud + n_app++;
                        hdist[e] = -1.0;
                        happ.push_back(e);
                    } else if (s.first_d != s.first_d) {   // best stays NaN: `best > d` is never true again
                        htarget[e] = s.first_idx;
                        hdist[e] = s.first_d;
                        ++(first_dynamic ? n_dynamic : n_static);
                    } else {
                        htarget[e] = s.min_idx;
                        hdist[e] = s.min_d;
                        ++(min_dynamic ? n_dynamic : n_static);
                    }
                }
                g_last_stats[0] = n_static;
                g_last_stats[1] = n_dynamic;
                // 5'b. record-level dedupe and destinations: old records, then merged-in records in merge order.
                //     The merged elements are grouped by target (stable, so in merge order); one pass over the
                //     output points in index order then knows every list's start as it goes.
                n_out = n_cloud + n_app;
                {
                    std::vector<int64_t> gs((size_t)n_out + 2, 0);
                    for (int e = 0; e < n_new; ++e)
                        if (hdist[e] != -1.0) ++gs[htarget[e] + 2];
                    for (int c = 0; c < n_out; ++c) gs[c + 2] += gs[c + 1];
                    std::vector<int32_t> ge(gs[n_out + 1]);
                    for (int e = 0; e < n_new; ++e)
                        if (hdist[e] != -1.0) ge[gs[htarget[e] + 1]++] = e;   // gs[c + 1] ends as the end of c's group
                    std::vector<int64_t> cur;   // new-record indices merged into the current point
                    for (int c = 0; c < n_out; ++c) {
                        const int e0 = c < n_cloud ? -1 : happ[c - n_cloud];
                        const int64_t i0 = e0 < 0 ? co[c] : no[e0], ni = (e0 < 0 ? co[c + 1] : no[e0 + 1]) - i0;
                        const int32_t* is = (e0 < 0 ? cs : ns) + i0;
                        const double* ixy = (e0 < 0 ? cxy : nxy) + 2 * i0;
                        if (e0 >= 0)
                            for (int64_t k = 0; k < ni; ++k) hdest[i0 + k] = hout[c] + k;   // appended as given
                        cur.clear();
                        for (int64_t g = gs[c]; g < gs[c + 1]; ++g) {
                            const int e = ge[g];
                            for (int64_t r = no[e]; r < no[e + 1]; ++r) {
                                bool held = false;
                                for (int64_t k = 0; k < ni && !held; ++k)
                                    held = is[k] == ns[r] && ixy[2 * k] == nxy[2 * r] && ixy[2 * k + 1] == nxy[2 * r + 1];
                                for (size_t k = 0; k < cur.size() && !held; ++k) {
                                    const int64_t q = cur[k];
                                    held = ns[q] == ns[r] && nxy[2 * q] == nxy[2 * r] && nxy[2 * q + 1] == nxy[2 * r + 1];
                                }
                                if (!held) {
                                    hdest[r] = hout[c] + ni + (int64_t)cur.size();
                                    cur.push_back(r);
                                }
                            }
                        }
                        hout[c + 1] = hout[c] + ni + (int64_t)cur.size();
                    }
                }
                n_orec = hout[n_out];
                if (n_nrec) SFMX_HIP_CHK(hipMemcpyAsync(ndest, hdest.data(), sizeof(int64_t) * n_nrec, hipMemcpyHostToDevice, st));
                if (n_app) SFMX_HIP_CHK(hipMemcpyAsync(appd, happ.data(), sizeof(int32_t) * n_app, hipMemcpyHostToDevice, st));
                SFMX_HIP_CHK(hipMemcpyAsync(do_off, hout.data(), sizeof(int64_t) * (n_out + 1), hipMemcpyHostToDevice, st));
                xfer += (int64_t)(sizeof(int64_t) * n_nrec + sizeof(int32_t) * n_app + sizeof(int64_t) * (n_out + 1));
            }

            // 6. scatter (the last timed span)
            SFMX_HIP_CHK(hipEventRecord(S->e0, st));
            {
                const int64_t items = n_crec + n_nrec + n_out;
                scatter_kernel<<<(unsigned)((items + 255) / 256), 256, 0, st>>>(n_crec, n_nrec, n_cloud, n_out, dco, crec_point, dcs, dcxy,
                                                                               dcx, dns, dnxy, dnx, ndest, appd, do_off, do_shot, do_xy,
                                                                               do_xyz);
            }
            SFMX_HIP_CHK(hipGetLastError());
            SFMX_HIP_CHK(hipEventRecord(S->e1, st));
            if (!decided) {   // the host's decisions
                if (!H) {
                    SFMX_HIP_CHK(hipMemcpyAsync(out_target, htarget.data(), sizeof(int32_t) * n_new, hipMemcpyHostToDevice, st));
                    SFMX_HIP_CHK(hipMemcpyAsync(out_merge_distance, hdist.data(), sizeof(double) * n_new, hipMemcpyHostToDevice, st));
                    xfer += (int64_t)((sizeof(int32_t) + sizeof(double)) * n_new);
                } else {
                    std::memcpy(out_target, htarget.data(), sizeof(int32_t) * n_new);
                    std::memcpy(out_merge_distance, hdist.data(), sizeof(double) * n_new);
                    std::memcpy(out_origin_offsets, hout.data(), sizeof(int64_t) * (n_out + 1));
                }
            } else if (H) {
                SFMX_HIP_CHK(call.back(out_target, tgd, n_new));
                SFMX_HIP_CHK(call.back(out_merge_distance, dsd, n_new));
                SFMX_HIP_CHK(call.back(out_origin_offsets, ood, (size_t)n_out + 1));
                xfer += (int64_t)((sizeof(int32_t) + sizeof(double)) * n_new + sizeof(int64_t) * (n_out + 1));
            }
            if (H) {
                SFMX_HIP_CHK(call.back(out_xyz, oxd, 3 * (size_t)n_out));
                xfer += (int64_t)sizeof(double) * 3 * n_out;
                if (n_orec) {
                    SFMX_HIP_CHK(call.back(out_origin_shot, osd, n_orec));
                    SFMX_HIP_CHK(call.back(out_origin_xy, oxyd, 2 * (size_t)n_orec));
                    xfer += (int64_t)(sizeof(int32_t) + 2 * sizeof(double)) * n_orec;
                }
            }
            SFMX_HIP_CHK(hipStreamSynchronize(st));
            if (hipEventElapsedTime(&part, S->e0, S->e1) == hipSuccess) ms += part;
            *out_n_points = n_out;
            *out_n_origins = n_orec;
            g_last_ms = ms;
        }
    done:;
        g_last_bytes = xfer;
        rc = call.finish(rc, "sfmx_merge_pointcloud_3d2d");   // drains the stream after an error: the host buffers are alive
    } catch (const std::bad_alloc&) {   // the host buffers: none is allocated with a copy to or from one in flight; no exception crosses the ABI
        if (call.S) (void)hipStreamSynchronize(st);   // the copies up from the caller's arrays
        rc = SFMX_ENOMEM;
        set_last_error("host allocation failed");
    }
    return rc;
}

}  // extern "C"
