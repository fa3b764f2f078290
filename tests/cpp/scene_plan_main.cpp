// SPDX-License-Identifier: MIT
// Stand-alone driver of csrc/scene_plan.hpp for tests/test_scene_plan_san.py (built with the host sanitizers; no
// device, no HIP).  The plan of the 3D-2D search and the merge's first pairs are checked against a brute-force
// restatement written here: for a candidate and another shot, the lowest-index visible pair joining the two in
// either orientation, dropped if its list is empty.  Then the capacity function and the accept and reject cases of
// every graph check.  Prints "ok <cases>" and exits 0, or names the first failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sfm-mvs-pipeline_amd/csrc/scene_plan.hpp"

using namespace sfmx::plan;

static int g_cases = 0;

struct GraphCase {
    const char* name;
    int32_t n_shots;
    std::vector<int32_t> pairs;     // 2 per pair
    std::vector<int64_t> lengths;   // one per pair
    std::vector<int32_t> active;    // empty: no mask
};

// the lowest-index visible pair joining {a, b} (a != b) in either orientation, -1: none
static int32_t first_joining(const GraphCase& g, int32_t a, int32_t b, bool masked) {
    for (size_t p = 0; p < g.lengths.size(); ++p) {
        if (masked && !g.active.empty() && !g.active[p]) continue;
        const int32_t L = g.pairs[2 * p], R = g.pairs[2 * p + 1];
        if (L != R && ((L == a && R == b) || (L == b && R == a))) return (int32_t)p;
    }
    return -1;
}

static bool check_plan(const GraphCase& g, const std::vector<int32_t>& candidates) {
    ++g_cases;
    const int32_t n_pairs = (int32_t)g.lengths.size();
    std::vector<int64_t> off(n_pairs + 1, 0);
    for (int32_t p = 0; p < n_pairs; ++p) off[p + 1] = off[p] + g.lengths[p];
    std::vector<int32_t> cand_of_shot(g.n_shots, -1);
    for (size_t c = 0; c < candidates.size(); ++c) cand_of_shot[candidates[c]] = (int32_t)c;
    std::vector<Table> expect;   // ascending in (other, cand)
    int64_t items = 0, slots = 0;
    for (int32_t o = 0; o < g.n_shots; ++o)
        for (size_t c = 0; c < candidates.size(); ++c) {
            const int32_t p = candidates[c] == o ? -1 : first_joining(g, candidates[c], o, true);
            if (p < 0 || g.lengths[p] == 0) continue;   // an empty first pair: no table, and no later pair instead
            int64_t cap = 16;
            while (cap < 2 * g.lengths[p]) cap *= 2;
            expect.push_back(Table{o, (int32_t)c, p, g.pairs[2 * p] == o ? 1 : 0, g.lengths[p], items, slots, cap});
            items += g.lengths[p];
            slots += cap;
        }
    Tables T;
    T.tables.resize(3);   // plan_tables must start from nothing
    T.items = T.slots = 99;
    const int rc = plan_tables(g.pairs.data(), n_pairs, g.active.empty() ? nullptr : g.active.data(), off.data(), cand_of_shot.data(),
                               nullptr, nullptr, T);
    if (rc != SFMX_OK) { std::printf("%s: status %d (%s)\n", g.name, rc, T.why); return false; }
    if (T.tables.size() != expect.size() || T.items != items || T.slots != slots) {
        std::printf("%s (%zu candidates): %zu tables, %lld items, %lld slots; the restatement gives %zu, %lld, %lld\n", g.name,
                    candidates.size(), T.tables.size(), (long long)T.items, (long long)T.slots, expect.size(), (long long)items,
                    (long long)slots);
        return false;
    }
    for (size_t i = 0; i < expect.size(); ++i) {
        const Table &a = T.tables[i], &b = expect[i];
        if (a.other != b.other || a.cand != b.cand || a.pair != b.pair || a.other_is_left != b.other_is_left || a.matches != b.matches ||
            a.item0 != b.item0 || a.slot0 != b.slot0 || a.cap != b.cap) {
            std::printf("%s (%zu candidates): table %zu is (other %d, cand %d, pair %d, left %d), the restatement gives (%d, %d, %d, %d)\n",
                        g.name, candidates.size(), i, a.other, a.cand, a.pair, a.other_is_left, b.other, b.cand, b.pair, b.other_is_left);
            return false;
        }
    }
    return true;
}

static bool check_first_pairs(const GraphCase& g) {
    ++g_cases;
    const int32_t n_pairs = (int32_t)g.lengths.size();
    std::vector<int64_t> off(n_pairs + 1, 0);
    for (int32_t p = 0; p < n_pairs; ++p) off[p + 1] = off[p] + g.lengths[p];
    std::vector<int32_t> first(7, 5);   // first_pairs must size and clear it
    const int64_t matches = first_pairs(g.pairs.data(), n_pairs, g.n_shots, off.data(), first);
    if ((int32_t)first.size() != n_pairs) { std::printf("%s: %zu flags for %d pairs\n", g.name, first.size(), n_pairs); return false; }
    int64_t expect_matches = 0;
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int32_t L = g.pairs[2 * p], R = g.pairs[2 * p + 1];
        const int32_t e = (L != R && first_joining(g, L, R, false) == p) ? 1 : 0;   // the merge knows no mask
        if (first[p] != e) { std::printf("%s: pair %d flagged %d, the restatement gives %d\n", g.name, p, first[p], e); return false; }
        if (e) expect_matches += g.lengths[p];
    }
    if (matches != expect_matches) { std::printf("%s: %lld link matches, expected %lld\n", g.name, (long long)matches, (long long)expect_matches); return false; }
    return true;
}

static bool expect(bool cond, const char* what) {
    ++g_cases;
    if (!cond) std::printf("%s\n", what);
    return cond;
}

int main() {
    bool ok = true;
    const std::vector<GraphCase> graphs = {
        {"no-pairs", 3, {}, {}, {}},
        {"self-pair", 3, {1, 1, 0, 1, 2, 2}, {4, 3, 2}, {}},
        {"both-orientations", 3, {0, 1, 1, 0, 2, 1, 1, 2}, {10, 25, 20, 40}, {}},
        {"mask-hides-the-first", 3, {0, 1, 1, 0, 2, 1, 1, 2}, {10, 25, 20, 40}, {0, 1, 1, 1}},
        {"mask-hides-all", 3, {0, 1, 1, 0}, {10, 25}, {0, 0}},
        {"empty-first-then-duplicate", 4, {0, 1, 1, 0, 0, 1, 2, 3}, {0, 7, 9, 1}, {}},
        {"candidate-without-a-pair", 5, {0, 1, 2, 1, 1, 3, 3, 0, 2, 0, 3, 2}, {5, 6, 7, 8, 9, 17}, {}},   // shot 4: no pair
        {"edge-case", 4, {0, 1, 2, 0, 0, 1, 1, 2, 3, 1}, {3, 3, 2, 1, 0}, {}},                            // tests/scene_cases.py
    };
    for (const GraphCase& g : graphs) {
        std::vector<int32_t> all;
        for (int32_t s = 0; s < g.n_shots; ++s) {
            ok = ok && check_plan(g, {s});   // n_candidates of 1: sfmx_find_3d2d_matches
            all.insert(all.begin(), s);      // every shot, in descending order: candidate index != shot index
        }
        ok = ok && check_plan(g, all);
        ok = ok && check_plan(g, {});
        if (g.n_shots >= 3) ok = ok && check_plan(g, {2, 0});
        ok = ok && check_first_pairs(g);
    }
    // the table capacity: a power of two, at least 16, at least twice the entries
    ok = ok && expect(capacity_for(0) == 16 && capacity_for(1) == 16 && capacity_for(8) == 16, "capacity of 0, 1, 8 entries is not 16");
    ok = ok && expect(capacity_for(9) == 32, "capacity of 9 entries is not 32");
    ok = ok && expect(capacity_for(MAX_LIST) == (int64_t)1 << 30, "capacity of 2^29 entries is not 2^30");
    ok = ok && expect(capacity_for(((int64_t)1 << 29) + 1) == (int64_t)1 << 31, "capacity of 2^29 + 1 entries is not 2^31");
    // the graph checks
    {
        const int32_t pairs[] = {0, 2, 2, 1}, low[] = {0, -1}, high[] = {0, 3}, counts[] = {5, 0, 7}, neg[] = {5, -1, 7};
        ok = ok && expect(shots_in_range(pairs, 2, 3) && shots_in_range(pairs, 0, 0), "shots_in_range refuses a valid list");
        ok = ok && expect(!shots_in_range(pairs, 2, 2) && !shots_in_range(low, 1, 3) && !shots_in_range(high, 1, 3),
                          "shots_in_range accepts a shot outside [0, n_shots)");
        ok = ok && expect(counts_non_negative(counts, 3) && counts_non_negative(neg, 1) && counts_non_negative(nullptr, 0),
                          "counts_non_negative refuses valid counts");
        ok = ok && expect(!counts_non_negative(neg, 3), "counts_non_negative accepts -1");
        const int64_t asc[] = {0, 0, 3, 3, 9}, from1[] = {1, 2}, desc[] = {0, 5, 3}, zero[] = {0};
        ok = ok && expect(offsets_ascend(asc, 4) && offsets_ascend(zero, 0), "offsets_ascend refuses valid offsets");
        ok = ok && expect(!offsets_ascend(from1, 1) && !offsets_ascend(desc, 2) && !offsets_ascend(from1, 0),
                          "offsets_ascend accepts offsets that do not ascend from 0");
        const sfmx_dmatch m[] = {{0, 0, 0, 1.f}, {4, 6, 0, 1.f}, {5, 0, 0, 1.f}, {0, 7, 0, 1.f}, {-1, 0, 0, 1.f}, {0, -1, 0, 1.f}};
        ok = ok && expect(match_indices_ok(m, 0, 2, 5, 7) && match_indices_ok(m, 2, 2, 0, 0), "match_indices_ok refuses valid indices");
        ok = ok && expect(!match_indices_ok(m, 0, 3, 5, 7) && !match_indices_ok(m, 3, 4, 5, 7) && !match_indices_ok(m, 4, 5, 5, 7) &&
                              !match_indices_ok(m, 5, 6, 5, 7) && !match_indices_ok(m, 0, 2, 4, 7) && !match_indices_ok(m, 0, 2, 5, 6),
                          "match_indices_ok accepts an index outside its image's keypoints");
        // through the plan: only the lists that are read are checked (pair 1 duplicates pair 0 and holds the bad index)
        const int32_t p2[] = {0, 1, 1, 0}, cand[] = {0, -1}, nkp[] = {5, 7};
        const int64_t off2[] = {0, 2, 3}, off3[] = {0, 0, 3};
        const sfmx_dmatch bad[] = {{0, 0, 0, 1.f}, {4, 6, 0, 1.f}, {7, 0, 0, 1.f}};
        Tables T;
        ok = ok && expect(plan_tables(p2, 2, nullptr, off2, cand, bad, nkp, T) == SFMX_OK && T.tables.size() == 1,
                          "a bad index in a pair that is not read refuses the call");
        const int32_t hide0[] = {0, 1};
        ok = ok && expect(plan_tables(p2, 2, hide0, off2, cand, bad, nkp, T) == SFMX_EINVAL && std::strstr(T.why, "keypoints"),
                          "a bad index in a pair that is read is accepted");
        ok = ok && expect(plan_tables(p2, 2, nullptr, off3, cand, bad, nkp, T) == SFMX_OK && T.tables.empty(),
                          "an empty first pair lets the later duplicate in");
        const int64_t huge[] = {0, MAX_LIST + 1, MAX_LIST + 2};
        ok = ok && expect(plan_tables(p2, 2, nullptr, huge, cand, nullptr, nkp, T) == SFMX_ECAPACITY, "a list beyond 2^29 entries is accepted");
        const int32_t p5[] = {0, 1, 0, 2, 0, 3, 0, 4}, cand5[] = {0, -1, -1, -1, -1};
        const int64_t many[] = {0, MAX_LIST, 2 * MAX_LIST, 3 * MAX_LIST, 4 * MAX_LIST};   // 2^31 items in four tables
        ok = ok && expect(plan_tables(p5, 4, nullptr, many, cand5, nullptr, nkp, T) == SFMX_ECAPACITY, "2^31 items in one call are accepted");
        ok = ok && expect(plan_tables(p5, 3, nullptr, many, cand5, nullptr, nkp, T) == SFMX_OK && T.items == 3 * MAX_LIST && T.slots == (int64_t)3 << 30,
                          "three lists of 2^29 entries are refused");
    }
    if (!ok) return 1;
    std::printf("ok %d\n", g_cases);
    return 0;
}
