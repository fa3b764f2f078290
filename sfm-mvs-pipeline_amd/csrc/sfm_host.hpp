// SPDX-License-Identifier: MIT
// The control flow of SfM::triangulate (sfm/SfM.cpp:164-381) over a table of steps (include/sfmx_sfm.h).
// Plain C++: no HIP, no library state; tests/cpp/sfm_host_main.cpp includes it and runs under the sanitizers.
//
// The loop is the reference's, statement by statement, on pair and shot indices instead of shared_ptrs.  The
// three pair lists are vectors that are erased from and pushed to as the reference does.  Where the reference
// leaves an order open:
//   1. the initial candidates' std::sort comparator (:184-188) is no strict weak order once a pair has fewer
//      than min_match_count_for_baseline matches: here the pairs with enough matches come first in ascending
//      ratio, then the others in ascending ratio, both stable in list order;
//   2. remainingShots comes from a std::set of pointers (:261-270): here ascending shot index;
//   3. the candidates' std::sort by count (:284-287) is unstable: here ties go to the lower shot index;
//   5. no pair passes the homography filter (:189-194 index an empty vector): here nothing is recovered.
// (4, the order of getDistinctShotMatches, belongs to the register_shot step.)
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/sfmx_sfm.h"

namespace sfmx {
namespace sfm_host {

inline void default_params(sfmx_sfm_params& p) {
    p.min_match_count_for_baseline = 100;
    p._reserved = 0;
    p.ransac_baseline_threshold = -1.0;
    p.ransac_pose_threshold = -8.0;
    p.min_homography_inlier_ratio = 0.5;
    p.min_pose_inlier_ratio = 0.5;
    p.max_reprojection_error = 10.0;
    p.point_merge_distance = 0.01;
    p.feature_merge_distance = 20.0;
}

// nullptr, or what is wrong with the parameters
inline const char* check_params(const sfmx_sfm_params* p) {
    if (!p) return "null parameters";
    if (p->min_match_count_for_baseline < 4) return "min_match_count_for_baseline below 4";
    if (!(p->min_homography_inlier_ratio >= 0.0 && p->min_homography_inlier_ratio <= 1.0)) return "min_homography_inlier_ratio outside [0, 1]";
    if (!(p->min_pose_inlier_ratio >= 0.0 && p->min_pose_inlier_ratio <= 1.0)) return "min_pose_inlier_ratio outside [0, 1]";
    if (std::isnan(p->point_merge_distance) || std::isnan(p->feature_merge_distance)) return "NaN merge distance";
    if (std::isnan(p->max_reprojection_error) || std::isnan(p->ransac_baseline_threshold) || std::isnan(p->ransac_pose_threshold))
        return "NaN threshold";
    return nullptr;
}

// nullptr, or what is wrong with the scene arguments
inline const char* check_graph(int32_t n_shots, const int32_t* pairs, int32_t n_pairs, const int32_t* pair_n_matches,
                               const double* homography_ratio) {
    if (n_shots < 0 || n_pairs < 0) return "negative count";
    if (n_pairs && (!pairs || !pair_n_matches || !homography_ratio)) return "null argument";
    for (int p = 0; p < n_pairs; ++p) {
        if (pairs[2 * p] < 0 || pairs[2 * p] >= n_shots || pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= n_shots)
            return "pair shot index out of range";
        if (pair_n_matches[p] < 0) return "negative match count";
        if (std::isnan(homography_ratio[p])) return "NaN homography ratio";
    }
    return nullptr;
}

struct Trace {
    sfmx_sfm_event* ev;
    int64_t cap;
    int64_t n = 0;
    void add(int32_t event, int32_t a, int32_t b, double value) {
        if (n < cap) ev[n] = sfmx_sfm_event{event, a, b, 0, value};
        ++n;
    }
};

struct Timed {   // wall time and call count of one kind of step
    sfmx_sfm_summary& s;
    const int k;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    Timed(sfmx_sfm_summary& sum, int kind) : s(sum), k(kind) {}
    ~Timed() {
        s.step_wall_ms[k] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        ++s.step_calls[k];
    }
};

inline void erase_value(std::vector<int32_t>& v, int32_t x) { v.erase(std::remove(v.begin(), v.end(), x), v.end()); }

// The arguments are valid (check_params, check_graph) and no output pointer is null except those that may be.
// SFMX_OK, SFMX_ECAPACITY (trace too short) or the negative value a step returned.
inline int triangulate_steps(const sfmx_sfm_steps& st, void* user, const sfmx_sfm_params& prm, int32_t n_shots,
                             const int32_t* pairs, int32_t n_pairs, const int32_t* pair_n_matches,
                             const double* homography_ratio, int32_t* recovered, int32_t* pair_state,
                             int32_t* out_pair_n_matches, sfmx_sfm_event* trace, int64_t trace_capacity,
                             int64_t* out_n_events, sfmx_sfm_summary* summary) {
    sfmx_sfm_summary sum{};
    sum.last_termination_type = -1;
    sum.initial_pair = -1;
    Trace tr{trace, trace ? trace_capacity : 0};
    std::vector<int32_t> count(pair_n_matches, pair_n_matches + n_pairs);   // ShotMatches::getMatches().size()
    std::vector<int32_t> to_triangulate(n_pairs), triangulated, failed;      // :166-168
    for (int p = 0; p < n_pairs; ++p) to_triangulate[p] = p;
    for (int s = 0; s < n_shots; ++s) recovered[s] = 0;
    for (int p = 0; p < n_pairs; ++p) pair_state[p] = SFMX_SFM_PAIR_OPEN;
    int rc = SFMX_OK;

    auto bundle_adjust = [&]() -> int {
        int32_t it = 0, term = -1;
        int r;
        {
            Timed t(sum, 6);
            r = st.bundle_adjust(user, &it, &term);
        }
        if (r < 0) return r;
        ++sum.ba_calls;
        sum.ba_iterations += it;
        sum.last_termination_type = term;
        tr.add(SFMX_SFM_BUNDLE_ADJUST, it, term, 0.0);
        return 0;
    };
    auto finish = [&]() {
        for (int s = 0; s < n_shots; ++s) sum.shots_recovered += recovered[s] != 0;
        sum.pairs_triangulated = (int32_t)triangulated.size();
        sum.pairs_failed = (int32_t)failed.size();
        sum.pairs_open = (int32_t)to_triangulate.size();
        if (out_pair_n_matches) std::copy(count.begin(), count.end(), out_pair_n_matches);
        if (out_n_events) *out_n_events = tr.n;
        if (summary) *summary = sum;
    };

    if (to_triangulate.empty()) {   // :171-173
        finish();
        return SFMX_OK;
    }

    // the initial pair from the homographies (:176-236)
    {
        std::vector<int32_t> ordered;
        for (int32_t p : to_triangulate)
            if (!(homography_ratio[p] < prm.min_homography_inlier_ratio)) ordered.push_back(p);   // :178-183
        std::stable_sort(ordered.begin(), ordered.end(),
                         [&](int32_t a, int32_t b) { return homography_ratio[a] < homography_ratio[b]; });
        std::stable_partition(ordered.begin(), ordered.end(),
                              [&](int32_t a) { return count[a] >= prm.min_match_count_for_baseline; });
        if (ordered.empty()) tr.add(SFMX_SFM_NO_CANDIDATE_PAIR, -1, -1, 0.0);
        bool found = false;
        for (int32_t p : ordered) {
            tr.add(SFMX_SFM_INITIAL_TRY, p, count[p], homography_ratio[p]);
            int32_t n_inliers = 0;
            int r;
            {
                Timed t(sum, 0);
                r = st.relative_pose(user, p, &n_inliers);
            }
            if (r < 0) { rc = r; goto out; }
            if (r != 1) {   // :203-206
                tr.add(SFMX_SFM_INITIAL_THROWS, p, -1, 0.0);
                continue;
            }
            const double ratio = (double)n_inliers / (double)count[p];   // :207
            if (ratio < prm.min_pose_inlier_ratio) {                     // :209-212
                tr.add(SFMX_SFM_INITIAL_LOW_RATIO, p, n_inliers, ratio);
                continue;
            }
            count[p] = n_inliers;   // :213
            int32_t n_points = 0;
            {
                Timed t(sum, 1);
                r = st.triangulate_pair(user, p, 1, &n_points);   // :214-220
            }
            if (r < 0) { rc = r; goto out; }
            {
                Timed t(sum, 2);
                r = st.add_elements(user, p, 0);   // :221-223
            }
            if (r < 0) { rc = r; goto out; }
            recovered[pairs[2 * p]] = 1;       // :226-227
            recovered[pairs[2 * p + 1]] = 1;
            erase_value(to_triangulate, p);    // :228-231
            triangulated.push_back(p);
            pair_state[p] = SFMX_SFM_PAIR_DONE;
            sum.initial_pair = p;
            tr.add(SFMX_SFM_INITIAL_PAIR, p, n_points, ratio);
            found = true;
            break;   // :233
        }
        if (found) {   // :235; without a pair the cloud is empty and the reference's call adjusts nothing
            const int r = bundle_adjust();
            if (r < 0) { rc = r; goto out; }
        }
    }

    if (triangulated.empty()) {   // :239-242
        tr.add(SFMX_SFM_NO_INITIAL_PAIR, -1, -1, 0.0);
        goto out;
    }

    // further shots (:245-376)
    while (!to_triangulate.empty()) {
        std::vector<int32_t> remaining;   // :259-271, ascending shot index
        {
            std::vector<char> in(n_shots, 0);
            for (int32_t p : to_triangulate) {
                const int32_t l = pairs[2 * p], r = pairs[2 * p + 1];
                if (!recovered[l]) in[l] = 1;
                if (!recovered[r]) in[r] = 1;
            }
            for (int32_t s = 0; s < n_shots; ++s)
                if (in[s]) remaining.push_back(s);
        }
        if (remaining.empty()) {   // :272-274
            tr.add(SFMX_SFM_NO_REMAINING_SHOT, (int32_t)to_triangulate.size(), -1, 0.0);
            break;
        }
        std::vector<int32_t> counts(remaining.size(), 0);   // :276-282
        {
            int r;
            {
                Timed t(sum, 3);
                r = st.count_candidates(user, remaining.data(), (int32_t)remaining.size(), counts.data());
            }
            if (r < 0) { rc = r; goto out; }
        }
        size_t best = 0;   // :284-300: the largest list, ties to the lower shot index
        for (size_t i = 1; i < remaining.size(); ++i)
            if (counts[i] > counts[best]) best = i;
        const int32_t shot = remaining[best];
        tr.add(SFMX_SFM_SHOT_CHOSEN, shot, counts[best], (double)remaining.size());

        double ratio = -1.0;
        std::vector<int32_t> distinct(std::max(n_pairs, 1));
        int32_t n_distinct = 0;
        int status;
        {
            Timed t(sum, 4);
            status = st.register_shot(user, shot, &ratio, distinct.data(), n_pairs, &n_distinct);   // :305
        }
        if (status < 0) { rc = status; goto out; }
        if (status != 1) ratio = -1.0;   // :306-309
        if (ratio < prm.min_pose_inlier_ratio) {   // :311-328
            tr.add(SFMX_SFM_SHOT_FAILED, shot, status, ratio);
            std::vector<int32_t> failed_now;
            for (int32_t p : to_triangulate)
                if (pairs[2 * p] == shot || pairs[2 * p + 1] == shot) failed_now.push_back(p);
            for (int32_t p : failed_now) {
                erase_value(to_triangulate, p);
                failed.push_back(p);
                pair_state[p] = SFMX_SFM_PAIR_LOST;
                tr.add(SFMX_SFM_PAIR_FAILED, p, shot, 0.0);
            }
            continue;
        }
        if (n_distinct < 0 || n_distinct > n_pairs) { rc = SFMX_EINTERNAL; goto out; }
        {
            Timed t(sum, 5);
            status = st.accept_shot(user, shot);   // :329
        }
        if (status < 0) { rc = status; goto out; }
        recovered[shot] = 1;   // :330
        tr.add(SFMX_SFM_SHOT_REGISTERED, shot, n_distinct, ratio);

        for (int32_t k = 0; k < n_distinct; ++k) {   // :334-369, one pair at a time
            const int32_t p = distinct[k];
            if (p < 0 || p >= n_pairs) { rc = SFMX_EINTERNAL; goto out; }
            if (!recovered[pairs[2 * p]] || !recovered[pairs[2 * p + 1]]) {   // :335-337
                tr.add(SFMX_SFM_PAIR_SKIPPED, p, -1, 0.0);
                continue;
            }
            int32_t n_inliers = 0, n_points = 0;
            int r;
            {
                Timed t(sum, 0);
                r = st.relative_pose(user, p, &n_inliers);   // :345
            }
            if (r < 0) { rc = r; goto out; }
            if (r != 1) {   // :346-349
                tr.add(SFMX_SFM_PAIR_THROWS, p, -1, 0.0);
                continue;
            }
            count[p] = n_inliers;   // :350
            {
                Timed t(sum, 1);
                r = st.triangulate_pair(user, p, 0, &n_points);   // :356
            }
            if (r < 0) { rc = r; goto out; }
            {
                Timed t(sum, 2);
                r = st.add_elements(user, p, 1);   // :358-362
            }
            if (r < 0) { rc = r; goto out; }
            erase_value(to_triangulate, p);   // :365-368
            triangulated.push_back(p);
            pair_state[p] = SFMX_SFM_PAIR_DONE;
            tr.add(SFMX_SFM_PAIR_TRIANGULATED, p, n_points, (double)n_inliers);
        }
        const int r = bundle_adjust();   // :371
        if (r < 0) { rc = r; goto out; }
    }
    tr.add(SFMX_SFM_DONE, (int32_t)triangulated.size(), (int32_t)failed.size(), (double)to_triangulate.size());

out:
    finish();
    if (rc == SFMX_OK && trace && tr.n > tr.cap) rc = SFMX_ECAPACITY;
    return rc;
}

}  // namespace sfm_host
}  // namespace sfmx
