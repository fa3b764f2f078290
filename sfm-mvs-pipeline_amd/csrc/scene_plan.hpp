// SPDX-License-Identifier: MIT
// What the entry points over the match graph (keypoints, n_keypoints, n_shots, pairs, n_pairs, matches, pair_offsets)
// decide on the host before they lay out a device block: sfmx_find_3d2d_matches and sfmx_count_3d2d_matches
// (csrc/scene.hip), sfmx_merge_pointcloud_3d2d (csrc/merge.hip).  The checks of the graph's host arrays, the capacity
// of a hash table, the pairs the reference's find_if loops can stop at.  Plain C++, no HIP:
// tests/cpp/scene_plan_main.cpp runs it under the host sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/sfmx.h"

namespace sfmx {
namespace plan {

// ---- checks of the graph's host arrays ---------------------------------------------------------------------------

inline bool shots_in_range(const int32_t* pairs, int32_t n_pairs, int32_t n_shots) {
    for (int64_t i = 0; i < 2 * (int64_t)n_pairs; ++i)
        if (pairs[i] < 0 || pairs[i] >= n_shots) return false;
    return true;
}

inline bool counts_non_negative(const int32_t* n_keypoints, int32_t n_shots) {
    for (int32_t s = 0; s < n_shots; ++s)
        if (n_keypoints[s] < 0) return false;
    return true;
}

// off[0 .. n]: a CSR's offsets start at 0 and never descend
inline bool offsets_ascend(const int64_t* off, int64_t n) {
    if (off[0] != 0) return false;
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

// matches[begin .. end) of a pair whose images hold n_left and n_right keypoints
inline bool match_indices_ok(const sfmx_dmatch* matches, int64_t begin, int64_t end, int32_t n_left, int32_t n_right) {
    for (int64_t k = begin; k < end; ++k)
        if (matches[k].queryIdx < 0 || matches[k].queryIdx >= n_left || matches[k].trainIdx < 0 || matches[k].trainIdx >= n_right)
            return false;
    return true;
}

// ---- hash tables -------------------------------------------------------------------------------------------------

constexpr int64_t MAX_LIST = (int64_t)1 << 29;   // entries of one table of the 3D-2D search: its capacity is an int32

// power of two, at least 16, load factor <= 1/2
inline int64_t capacity_for(int64_t entries) {
    int64_t cap = 16;
    while (cap < 2 * entries) cap <<= 1;
    return cap;
}

// ---- the 3D-2D search: one table per (other shot, candidate) -----------------------------------------------------

struct Table {
    int32_t other, cand;      // the table joins candidate `cand` (an index into the caller's list) to shot `other`
    int32_t pair;             // through the first visible pair in list order joining the two (Scene.cpp:389-394)
    int32_t other_is_left;    // 1: `other` is that pair's left image (queryIdx side)
    int64_t matches;          // the pair's list length, > 0
    int64_t item0, slot0;     // exclusive scans of `matches` and `cap` over the tables before this one
    int64_t cap;
};

struct Tables {
    std::vector<Table> tables;   // ascending in (other, cand)
    int64_t items = 0, slots = 0;
    const char* why = "";        // what was wrong, after a status other than SFMX_OK
};

// cand_of_shot[n_shots]: a shot's index among the candidates, -1 for the others.  active: null, or a pair with 0 is
// invisible.  off[n_pairs + 1] ascends from 0.  host_matches: null (device inputs), or the indices of every list that
// is read are checked against n_keypoints.  A pair of a shot with itself joins nothing; a first pair with an empty
// list has no table and no later pair takes its place.
// SFMX_OK, SFMX_EINVAL (a match index) or SFMX_ECAPACITY (a list beyond MAX_LIST, 2^31 items or tables).
inline int plan_tables(const int32_t* pairs, int32_t n_pairs, const int32_t* active, const int64_t* off,
                       const int32_t* cand_of_shot, const sfmx_dmatch* host_matches, const int32_t* n_keypoints, Tables& out) {
    std::vector<Table>& t = out.tables;
    t.clear();
    out.items = out.slots = 0;
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int32_t L = pairs[2 * p], R = pairs[2 * p + 1];
        if (L == R || (active && !active[p])) continue;
        if (cand_of_shot[L] >= 0) t.push_back(Table{R, cand_of_shot[L], p, 0, 0, 0, 0, 0});
        if (cand_of_shot[R] >= 0) t.push_back(Table{L, cand_of_shot[R], p, 1, 0, 0, 0, 0});
    }
    std::stable_sort(t.begin(), t.end(), [](const Table& a, const Table& b) {
        return a.other != b.other ? a.other < b.other : a.cand < b.cand;
    });
    size_t n = 0;
    for (size_t i = 0; i < t.size(); ++i) {
        if (i && t[i].other == t[i - 1].other && t[i].cand == t[i - 1].cand) continue;   // only the first of a run counts
        Table u = t[i];
        u.matches = off[u.pair + 1] - off[u.pair];
        if (u.matches <= 0) continue;
        if (host_matches && !match_indices_ok(host_matches, off[u.pair], off[u.pair + 1], n_keypoints[pairs[2 * u.pair]],
                                              n_keypoints[pairs[2 * u.pair + 1]])) {
            out.why = "match index outside its image's keypoints";
            return SFMX_EINVAL;
        }
        if (u.matches > MAX_LIST) { out.why = "a match list beyond 2^29 entries"; return SFMX_ECAPACITY; }
        u.cap = capacity_for(u.matches);
        u.item0 = out.items;
        u.slot0 = out.slots;
        out.items += u.matches;
        out.slots += u.cap;
        t[n++] = u;
    }
    t.resize(n);
    if (out.items >= INT32_MAX || n >= (size_t)INT32_MAX) { out.why = "too many matches"; return SFMX_ECAPACITY; }
    return SFMX_OK;
}

// ---- the merge: one link list per unordered shot pair ------------------------------------------------------------

// first[p] = 1 iff p is the lowest-index pair joining its two shots in either orientation (Scene.cpp:505-520: the
// loop breaks at the first such pair); a pair of a shot with itself joins nothing.  -> the matches of those pairs
inline int64_t first_pairs(const int32_t* pairs, int32_t n_pairs, int32_t n_shots, const int64_t* off, std::vector<int32_t>& first) {
    first.assign(n_pairs, 0);
    std::vector<std::pair<int64_t, int32_t>> keyed(n_pairs);
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int64_t a = std::min(pairs[2 * p], pairs[2 * p + 1]), c = std::max(pairs[2 * p], pairs[2 * p + 1]);
        keyed[p] = {a * n_shots + c, p};
    }
    std::sort(keyed.begin(), keyed.end());
    int64_t matches = 0;
    for (int32_t i = 0; i < n_pairs; ++i) {
        const int32_t p = keyed[i].second;
        if (pairs[2 * p] == pairs[2 * p + 1]) continue;
        if (i == 0 || keyed[i - 1].first != keyed[i].first) {
            first[p] = 1;
            matches += off[p + 1] - off[p];
        }
    }
    return matches;
}

}  // namespace plan
}  // namespace sfmx
