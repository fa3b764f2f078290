// SPDX-License-Identifier: MIT
// sfmx scene bookkeeping for gfx950.
//
//   sfmx_find_3d2d_matches            Scene::find3d2dMatches   (common/Scene.cpp:369-424)
//   sfmx_count_3d2d_matches           the sizes of find3d2dMatches' lists for many shots at once (SfM.cpp:276-300)
//   sfmx_ba_observations_from_origins BundleAdjustment.cpp:50-91 problem assembly (host, O(n))
//
// The reference's 3D-2D search is a nested linear scan: for every point
// origin it walks the shot-match list (find_if) and then the pair's DMatch
// list comparing keypoint positions, O(P * origins * (pairs + matches)).  Here
// it is a hash join on the GPU:
//   1. (host, O(pairs)) for every other shot o, the first pair joining
//      {shot, o} in list order — the only pair find_if can return;
//   2. one open-addressing table per such pair, keyed by the exact float bits
//      of the keypoint position on o's side, value = the smallest match index
//      with that position (atomicMin: the first DMatch in list order, which is
//      what find_if returns);
//   3. one thread per origin record probes its pair's table with the origin's
//      cv::Point2d — equal to a float keypoint position iff both coordinates
//      are exactly representable as float and equal (NaN never matches; -0 and
//      +0 compare equal, so both are keyed as +0).
// Integer / byte work: HBM- and latency-bound, no MFMA.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/sfmx_scene.h"
#include "device_call.hpp"
#include "match_common.hpp"
#include "scene_plan.hpp"

namespace sfmx {
namespace scene {

constexpr unsigned long long EMPTY = ~0ull;

struct UsedPair {          // a pair that is the first one joining {shot, other}
    int32_t pair;
    int32_t other_is_left;  // 1: the other shot is the pair's left image (queryIdx side)
    int64_t table0;         // first slot of its table
    int32_t cap;            // table capacity (power of two)
    int32_t cand;           // sfmx_count_3d2d_matches: index of the candidate the table serves
};

__device__ __forceinline__ unsigned long long pos_key(float x, float y) {
    x = x == 0.f ? 0.f : x;   // -0 == +0 under cv::Point2d ==
    y = y == 0.f ? 0.f : y;
    return ((unsigned long long)__float_as_uint(x) << 32) | __float_as_uint(y);
}
__device__ __forceinline__ uint32_t mix(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (uint32_t)k;
}

// one thread per match of a used pair: table[pos] = min match index
__global__ __launch_bounds__(256)
void build_tables_kernel(const UsedPair* __restrict__ used, const int32_t* __restrict__ used_first_match,
                         int n_used, int64_t n_items, const int64_t* __restrict__ off,
                         const DMatchDev* __restrict__ matches, const float2* const* __restrict__ kp,
                         const int32_t* __restrict__ nkp, const int32_t* __restrict__ pairs,
                         unsigned long long* __restrict__ tkey, int32_t* __restrict__ tval) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_items) return;
    // locate the used pair (used_first_match is the exclusive scan of match counts)
    int lo = 0, hi = n_used - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (used_first_match[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const UsedPair u = used[lo];
    const int i = (int)(g - used_first_match[lo]);
    const DMatchDev d = matches[off[u.pair] + i];
    const int oshot = u.other_is_left ? pairs[2 * u.pair] : pairs[2 * u.pair + 1];
    const int kidx = u.other_is_left ? d.queryIdx : d.trainIdx;
    if (kidx < 0 || kidx >= nkp[oshot]) return;
    const float2 q = kp[oshot][kidx];
    if (q.x != q.x || q.y != q.y) return;   // NaN never compares equal
    const unsigned long long key = pos_key(q.x, q.y);
    uint32_t h = mix(key) & (uint32_t)(u.cap - 1);
    for (int probe = 0; probe < u.cap; ++probe) {
        unsigned long long* slot = tkey + u.table0 + h;
        const unsigned long long prev = atomicCAS(slot, EMPTY, key);
        if (prev == EMPTY || prev == key) {
            atomicMin(tval + u.table0 + h, i);
            return;
        }
        h = (h + 1) & (uint32_t)(u.cap - 1);
    }
}

// one thread per origin record
__global__ __launch_bounds__(256)
void lookup_kernel(int64_t n_origins, const int32_t* __restrict__ origin_shot, const double* __restrict__ origin_xy,
                   int shot, int n_shots, const int32_t* __restrict__ used_of_shot, const UsedPair* __restrict__ used,
                   const unsigned long long* __restrict__ tkey, const int32_t* __restrict__ tval,
                   const int64_t* __restrict__ off, const DMatchDev* __restrict__ matches,
                   const float2* const* __restrict__ kp, const int32_t* __restrict__ nkp,
                   int32_t* __restrict__ out_kp, int32_t* __restrict__ out_pair, float* __restrict__ out_xy) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_origins) return;
    int res_kp = -1, res_pair = -1;
    float2 res_xy = make_float2(__builtin_nanf(""), __builtin_nanf(""));
    const int o = origin_shot[r];
    const int ui = (o >= 0 && o < n_shots && o != shot) ? used_of_shot[o] : -1;
    if (ui >= 0) {
        const double qx = origin_xy[2 * r], qy = origin_xy[2 * r + 1];
        const float fx = (float)qx, fy = (float)qy;
        if ((double)fx == qx && (double)fy == qy) {   // else no float keypoint position can equal it
            const UsedPair u = used[ui];
            const unsigned long long key = pos_key(fx, fy);
            uint32_t h = mix(key) & (uint32_t)(u.cap - 1);
            for (int probe = 0; probe < u.cap; ++probe) {
                const unsigned long long k = tkey[u.table0 + h];
                if (k == EMPTY) break;
                if (k == key) {
                    const int i = tval[u.table0 + h];
                    const DMatchDev d = matches[off[u.pair] + i];
                    const int sidx = u.other_is_left ? d.trainIdx : d.queryIdx;   // `shot`'s side
                    if (sidx >= 0 && sidx < nkp[shot]) {
                        res_kp = sidx;
                        res_pair = u.pair;
                        res_xy = kp[shot][sidx];
                    }
                    break;
                }
                h = (h + 1) & (uint32_t)(u.cap - 1);
            }
        }
    }
    out_kp[r] = res_kp;
    out_pair[r] = res_pair;
    if (out_xy) { out_xy[2 * r] = res_xy.x; out_xy[2 * r + 1] = res_xy.y; }
}

// sfmx_count_3d2d_matches: one thread per origin record.  The tables of the candidates that have a pair with the
// record's origin shot lie in used[tab_first[o] .. tab_first[o + 1]), ascending in candidate index; the thread
// probes each of them with the record's position.  Hits are summed per wave in LDS (one row per wave, COUNT_TILE
// candidates per pass; the walk of a lane stops at the pass's last candidate and goes on in the next pass), then
// one global atomic per (wave, candidate with a hit).  16 KiB of LDS per block.
constexpr int COUNT_TILE = 1024;

__global__ __launch_bounds__(256)
void count_kernel(int64_t n_origins, const int32_t* __restrict__ origin_shot, const double* __restrict__ origin_xy,
                  int n_shots, const int32_t* __restrict__ tab_first, const UsedPair* __restrict__ used,
                  const unsigned long long* __restrict__ tkey, const int32_t* __restrict__ tval,
                  const int64_t* __restrict__ off, const DMatchDev* __restrict__ matches,
                  const int32_t* __restrict__ nkp_cand, int n_candidates, int32_t* __restrict__ out_count) {
    __shared__ int32_t cnt[4][COUNT_TILE];
    const int lane = threadIdx.x & 63;
    int32_t* const row = cnt[threadIdx.x >> 6];
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int e = 0, end = 0;
    unsigned long long key = 0;
    if (r < n_origins) {
        const int o = origin_shot[r];
        if (o >= 0 && o < n_shots) {
            const double qx = origin_xy[2 * r], qy = origin_xy[2 * r + 1];
            const float fx = (float)qx, fy = (float)qy;
            if ((double)fx == qx && (double)fy == qy) {   // else no float keypoint position can equal it
                e = tab_first[o];
                end = tab_first[o + 1];
                key = pos_key(fx, fy);
            }
        }
    }
    const uint32_t hash = mix(key);
    for (int t0 = 0; t0 < n_candidates; t0 += COUNT_TILE) {
        const int t1 = min(t0 + COUNT_TILE, n_candidates);
        for (int j = lane; j < t1 - t0; j += 64) row[j] = 0;
        __syncthreads();
        while (e < end) {
            const UsedPair u = used[e];
            if (u.cand >= t1) break;
            ++e;
            uint32_t h = hash & (uint32_t)(u.cap - 1);
            for (int probe = 0; probe < u.cap; ++probe) {
                const unsigned long long k = tkey[u.table0 + h];
                if (k == EMPTY) break;
                if (k == key) {
                    const int i = tval[u.table0 + h];
                    const int64_t m0 = off[u.pair];
                    if (i >= 0 && i < off[u.pair + 1] - m0) {
                        const DMatchDev d = matches[m0 + i];
                        const int sidx = u.other_is_left ? d.trainIdx : d.queryIdx;   // the candidate's side
                        if (sidx >= 0 && sidx < nkp_cand[u.cand]) atomicAdd(&row[u.cand - t0], 1);
                    }
                    break;
                }
                h = (h + 1) & (uint32_t)(u.cap - 1);
            }
        }
        __syncthreads();
        for (int j = lane; j < t1 - t0; j += 64) {
            const int v = row[j];
            if (v) atomicAdd(out_count + t0 + j, v);
        }
        __syncthreads();
    }
}

thread_local float g_last_ms = -1.f;
thread_local float g_count_ms = -1.f;
Slot g_slot[64];   // csrc/device_call.hpp; both entry points share it

// ---- what both entry points do around their launches (the call frame: csrc/device_call.hpp) -----------------------

// the checks of the graph's host arrays that need no device
static int check_graph(const int32_t* n_keypoints, int32_t n_shots, const int32_t* pairs, int32_t n_pairs) {
    if (!plan::counts_non_negative(n_keypoints, n_shots)) { set_last_error("negative keypoint count"); return SFMX_EINVAL; }
    if (!plan::shots_in_range(pairs, n_pairs, n_shots)) { set_last_error("pair shot index out of range"); return SFMX_EINVAL; }
    return SFMX_OK;
}

// After F.open: the pair offsets and the origin record count on the host, their checks, the tables of the call
// (cand_of_shot[s]: the index of shot s among the candidates, -1 for the others).  SFMX_OK, or the status with the
// error text set (the frame's tail names a HIP error).
static int plan_call(const DeviceCall& F, const int32_t* n_keypoints, const int32_t* pairs, int32_t n_pairs,
                     const int32_t* pair_active, const sfmx_dmatch* matches, const int64_t* pair_offsets,
                     const int64_t* origin_offsets, int32_t n_points, const std::vector<int32_t>& cand_of_shot,
                     std::vector<int64_t>& hoff, int64_t& n_origins, plan::Tables& T) {
    hoff.assign((size_t)n_pairs + 1, 0);
    if (F.host) {
        if (n_pairs) std::memcpy(hoff.data(), pair_offsets, sizeof(int64_t) * (n_pairs + 1));
        n_origins = origin_offsets[n_points];
    } else if ((n_pairs && hipMemcpyAsync(hoff.data(), pair_offsets, sizeof(int64_t) * (n_pairs + 1), hipMemcpyDeviceToHost, F.st) != hipSuccess) ||
               hipMemcpyAsync(&n_origins, origin_offsets + n_points, sizeof(int64_t), hipMemcpyDeviceToHost, F.st) != hipSuccess ||
               hipStreamSynchronize(F.st) != hipSuccess) {
        return SFMX_EDEVICE;
    }
    if (!plan::offsets_ascend(hoff.data(), n_pairs)) { set_last_error("pair offsets do not ascend from 0"); return SFMX_EINVAL; }
    if (n_origins < 0 || (n_origins + 255) / 256 > INT32_MAX) { set_last_error("origin record count out of range"); return SFMX_EINVAL; }
    if (hoff[n_pairs] && !matches) { set_last_error("null argument"); return SFMX_EINVAL; }
    const int rc = plan::plan_tables(pairs, n_pairs, pair_active, hoff.data(), cand_of_shot.data(), F.host ? matches : nullptr,
                                     n_keypoints, T);
    if (rc != SFMX_OK) set_last_error(T.why);
    return rc;
}

// The parts of the device block that both entry points have: the graph's small tables, which lie among the block's
// pinned leading tables, and with host inputs the staging copies of the graph and of the origin records.
struct Graph {
    int32_t *nkd, *prd, *sd;
    const float2** kpd;
    float2* kd;
    sfmx_dmatch* md;
    int64_t* od;
    double* xd;
    // what the kernels read: the caller's device arrays or the staging copies, set by stage()
    const DMatchDev* dm;
    const int64_t* doff;
    const int32_t* dshot;
    const double* dxy;

    void want_tables(BlockLayout& L, int32_t n_shots, int32_t n_pairs) {
        L.want(nkd, n_shots);
        L.want(prd, 2 * (size_t)n_pairs);
        L.want(kpd, n_shots);
    }
    void want_staging(BlockLayout& L, bool H, const int32_t* n_keypoints, int32_t n_shots, int32_t n_pairs, int64_t n_matches,
                      int64_t n_origins) {
        int64_t nk = 0;
        for (int i = 0; H && i < n_shots; ++i) nk += n_keypoints[i];
        L.want(kd, nk, H);
        L.want(md, n_matches, H);
        L.want(od, (size_t)n_pairs + 1, H);
        L.want(sd, n_origins, H);
        L.want(xd, 2 * (size_t)n_origins, H);
    }
    // after F.reserve: fills the pinned twins of the tables and sends the host inputs on their way up
    hipError_t stage(DeviceCall& F, const sfmx_point2f* const* keypoints, const int32_t* n_keypoints, int32_t n_shots,
                     const int32_t* pairs, int32_t n_pairs, const sfmx_dmatch* matches, int64_t n_matches,
                     const int64_t* pair_offsets, const int32_t* origin_shot, const double* origin_xy, int64_t n_origins) {
        std::memcpy(F.pinned(nkd), n_keypoints, sizeof(int32_t) * n_shots);
        if (n_pairs) std::memcpy(F.pinned(prd), pairs, sizeof(int32_t) * 2 * n_pairs);
        const float2** hk = F.pinned(kpd);
        int64_t o = 0;
        for (int i = 0; i < n_shots; ++i) {
            if (F.host) {
                if (n_keypoints[i] && F.err == hipSuccess)
                    F.err = hipMemcpyAsync(kd + o, keypoints[i], sizeof(float2) * n_keypoints[i], hipMemcpyHostToDevice, F.st);
                hk[i] = kd + o;
                o += n_keypoints[i];
            } else {
                hk[i] = reinterpret_cast<const float2*>(keypoints[i]);
            }
        }
        dm = reinterpret_cast<const DMatchDev*>(n_matches ? F.in(matches, md, n_matches) : matches);
        doff = n_pairs ? F.in(pair_offsets, od, (size_t)n_pairs + 1) : pair_offsets;
        dshot = n_origins ? F.in(origin_shot, sd, n_origins) : origin_shot;
        dxy = n_origins ? F.in(origin_xy, xd, 2 * (size_t)n_origins) : origin_xy;
        return F.err;
    }
};

// the pinned twins of the table list (used) and of the exclusive scan of its match counts (first)
static void fill_used(const plan::Tables& T, UsedPair* used, int32_t* first) {
    for (size_t u = 0; u < T.tables.size(); ++u) {
        const plan::Table& t = T.tables[u];
        used[u] = UsedPair{t.pair, t.other_is_left, t.slot0, (int32_t)t.cap, t.cand};
        first[u] = (int32_t)t.item0;
    }
}

}  // namespace scene
}  // namespace sfmx

using namespace sfmx;
using namespace sfmx::scene;

extern "C" {

float sfmx_find_3d2d_last_kernel_ms(void) { return g_last_ms; }

int sfmx_find_3d2d_matches(const sfmx_point2f* const* keypoints, const int32_t* n_keypoints, int32_t n_shots,
                           const int32_t* pairs, int32_t n_pairs, const sfmx_dmatch* matches,
                           const int64_t* pair_offsets, const int64_t* origin_offsets, int32_t n_points,
                           const int32_t* origin_shot, const double* origin_xy, int32_t shot,
                           int32_t inputs_on_device, int32_t device, void* stream, int32_t* out_keypoint,
                           int32_t* out_pair, float* out_xy) {
    if (n_shots < 0 || n_pairs < 0 || n_points < 0) { set_last_error("negative count"); return SFMX_EINVAL; }
    if (!keypoints || !n_keypoints || (n_pairs && (!pairs || !pair_offsets)) || !origin_offsets ||
        !out_keypoint || !out_pair) {
        set_last_error("null argument");
        return SFMX_EINVAL;
    }
    if (shot < 0 || shot >= n_shots) { set_last_error("shot index out of range"); return SFMX_EINVAL; }
    {
        const int grc = check_graph(n_keypoints, n_shots, pairs, n_pairs);
        if (grc != SFMX_OK) return grc;
    }
    if (!inputs_on_device && origin_offsets[n_points] && (!origin_shot || !origin_xy)) { set_last_error("null origin arrays"); return SFMX_EINVAL; }
    DeviceCall F(stream, !inputs_on_device);
    const hipStream_t st = F.st;
    {
        const int orc = F.open(g_slot, device);
        if (orc != SFMX_OK) return orc;
    }
    Slot* const S = F.S;
    int rc = SFMX_OK;
    {
        std::vector<int64_t> hoff;
        std::vector<int32_t> cand_of_shot(n_shots, -1);
        plan::Tables T;
        int64_t n_origins = 0;
        cand_of_shot[shot] = 0;   // the count's plan for one candidate and no mask (Scene.cpp:389-394)
        rc = plan_call(F, n_keypoints, pairs, n_pairs, nullptr, matches, pair_offsets, origin_offsets, n_points, cand_of_shot, hoff,
                       n_origins, T);
        if (rc == SFMX_ECAPACITY) rc = SFMX_EINVAL;   // this entry point's code for too many matches
        if (rc != SFMX_OK) goto done;
        {
            // device block: [tables of the call | hash tables | (host inputs: graph, origins, outputs)]
            const bool H = F.host;
            const size_t n_used = T.tables.size();
            const int64_t n_matches = hoff[n_pairs];
            BlockLayout L;
            Graph G;
            UsedPair* usd;
            int32_t *ufd, *uos, *tv, *kpo, *pro;
            unsigned long long* tk;
            float* xyo;
            L.want(usd, n_used);
            L.want(ufd, n_used);
            L.want(uos, n_shots);
            G.want_tables(L, n_shots, n_pairs);
            const size_t b_tab = L.need;   // up to here: staged in pinned memory, one upload
            L.want(tk, T.slots);
            L.want(tv, T.slots);
            G.want_staging(L, H, n_keypoints, n_shots, n_pairs, n_matches, n_origins);
            L.want(kpo, n_origins, H);
            L.want(pro, n_origins, H);
            L.want(xyo, 2 * (size_t)n_origins, H && out_xy);
            rc = F.reserve(L, b_tab);
            if (rc != SFMX_OK) goto done;
            fill_used(T, F.pinned(usd), F.pinned(ufd));
            int32_t* const used_of_shot = F.pinned(uos);
            for (int s = 0; s < n_shots; ++s) used_of_shot[s] = -1;
            for (size_t u = 0; u < n_used; ++u) used_of_shot[T.tables[u].other] = (int32_t)u;
            SFMX_HIP_CHK(G.stage(F, keypoints, n_keypoints, n_shots, pairs, n_pairs, matches, n_matches, pair_offsets, origin_shot,
                                 origin_xy, n_origins));
            SFMX_HIP_CHK(F.upload(b_tab));
            int32_t *dokp = F.out(out_keypoint, kpo), *dopair = F.out(out_pair, pro);
            float* doxy = out_xy ? F.out(out_xy, xyo) : nullptr;
            (void)hipEventRecord(S->e0, st);
            if (T.slots) {
                SFMX_HIP_CHK(hipMemsetAsync(tk, 0xff, sizeof(unsigned long long) * T.slots, st));
                SFMX_HIP_CHK(hipMemsetAsync(tv, 0x7f, sizeof(int32_t) * T.slots, st));
            }
            if (T.items)
                build_tables_kernel<<<(unsigned)((T.items + 255) / 256), 256, 0, st>>>(usd, ufd, (int)n_used, T.items, G.doff, G.dm,
                                                                                      G.kpd, G.nkd, G.prd, tk, tv);
            if (n_origins)
                lookup_kernel<<<(unsigned)((n_origins + 255) / 256), 256, 0, st>>>(n_origins, G.dshot, G.dxy, shot, n_shots, uos, usd,
                                                                                 tk, tv, G.doff, G.dm, G.kpd, G.nkd, dokp, dopair, doxy);
            (void)hipEventRecord(S->e1, st);
            SFMX_HIP_CHK(hipGetLastError());
            if (n_origins) {
                SFMX_HIP_CHK(F.back(out_keypoint, kpo, n_origins));
                SFMX_HIP_CHK(F.back(out_pair, pro, n_origins));
                if (out_xy) SFMX_HIP_CHK(F.back(out_xy, xyo, 2 * (size_t)n_origins));
            }
            SFMX_HIP_CHK(hipStreamSynchronize(st));
            float ms = -1.f;
            (void)hipEventElapsedTime(&ms, S->e0, S->e1);
            g_last_ms = ms;
        }
    done:;
        rc = F.finish(rc, "sfmx_find_3d2d_matches");
    }
    return rc;
}

float sfmx_count_3d2d_last_kernel_ms(void) { return g_count_ms; }

int sfmx_count_3d2d_matches(const sfmx_point2f* const* keypoints, const int32_t* n_keypoints, int32_t n_shots,
                            const int32_t* pairs, int32_t n_pairs, const int32_t* pair_active,
                            const sfmx_dmatch* matches, const int64_t* pair_offsets, const int64_t* origin_offsets,
                            int32_t n_points, const int32_t* origin_shot, const double* origin_xy,
                            const int32_t* candidates, int32_t n_candidates, int32_t inputs_on_device, int32_t device,
                            void* stream, int32_t* out_count) {
    if (n_shots < 0 || n_pairs < 0 || n_points < 0 || n_candidates < 0) { set_last_error("negative count"); return SFMX_EINVAL; }
    if (!keypoints || !n_keypoints || (n_pairs && (!pairs || !pair_offsets)) || !origin_offsets ||
        (n_candidates && (!candidates || !out_count))) {
        set_last_error("null argument");
        return SFMX_EINVAL;
    }
    {
        const int grc = check_graph(n_keypoints, n_shots, pairs, n_pairs);
        if (grc != SFMX_OK) return grc;
    }
    std::vector<int32_t> cand_of_shot(n_shots, -1);
    for (int c = 0; c < n_candidates; ++c) {
        const int s = candidates[c];
        if (s < 0 || s >= n_shots) { set_last_error("candidate shot index out of range"); return SFMX_EINVAL; }
        if (cand_of_shot[s] >= 0) { set_last_error("candidate shot listed twice"); return SFMX_EINVAL; }
        cand_of_shot[s] = c;
    }
    if (!inputs_on_device) {
        if (!plan::offsets_ascend(origin_offsets, n_points)) { set_last_error("origin offsets do not ascend from 0"); return SFMX_EINVAL; }
        if (origin_offsets[n_points] && (!origin_shot || !origin_xy)) { set_last_error("null origin arrays"); return SFMX_EINVAL; }
    }
    if (n_candidates == 0) { g_count_ms = 0.f; return SFMX_OK; }   // nothing to write
    DeviceCall F(stream, !inputs_on_device);
    const hipStream_t st = F.st;
    {
        const int orc = F.open(g_slot, device);
        if (orc != SFMX_OK) return orc;
    }
    Slot* const S = F.S;
    int rc = SFMX_OK;
    {
        std::vector<int64_t> hoff;
        plan::Tables T;
        int64_t n_origins = 0;
        // per (origin shot o, candidate s): the first visible pair in list order joining {s, o} (Scene.cpp:389-394)
        rc = plan_call(F, n_keypoints, pairs, n_pairs, pair_active, matches, pair_offsets, origin_offsets, n_points, cand_of_shot, hoff,
                       n_origins, T);
        if (rc != SFMX_OK) goto done;
        {
            // device block: [tables of the call | hash tables | (host inputs: graph, origins, counts)]
            const bool H = F.host;
            const size_t n_used = T.tables.size();
            const int64_t n_matches = hoff[n_pairs];
            BlockLayout L;
            Graph G;
            UsedPair* usd;
            int32_t *ufd, *tfd, *ncd, *tv, *cd;
            unsigned long long* tk;
            L.want(usd, n_used);
            L.want(ufd, n_used);
            L.want(tfd, (size_t)n_shots + 1);
            L.want(ncd, n_candidates);
            G.want_tables(L, n_shots, n_pairs);
            const size_t b_tab = L.need;   // up to here: staged in pinned memory, one upload
            L.want(tk, T.slots);
            L.want(tv, T.slots);
            G.want_staging(L, H, n_keypoints, n_shots, n_pairs, n_matches, n_origins);
            L.want(cd, n_candidates, H);
            rc = F.reserve(L, b_tab);
            if (rc != SFMX_OK) goto done;
            fill_used(T, F.pinned(usd), F.pinned(ufd));
            int32_t* const htf = F.pinned(tfd);   // the tables of origin shot o: used[htf[o] .. htf[o + 1])
            for (int o = 0; o <= n_shots; ++o) htf[o] = 0;
            for (const plan::Table& t : T.tables) ++htf[t.other + 1];
            for (int o = 0; o < n_shots; ++o) htf[o + 1] += htf[o];
            for (int c = 0; c < n_candidates; ++c) F.pinned(ncd)[c] = n_keypoints[candidates[c]];
            SFMX_HIP_CHK(G.stage(F, keypoints, n_keypoints, n_shots, pairs, n_pairs, matches, n_matches, pair_offsets, origin_shot,
                                 origin_xy, n_origins));
            SFMX_HIP_CHK(F.upload(b_tab));
            int32_t* dcount = F.out(out_count, cd);
            (void)hipEventRecord(S->e0, st);
            SFMX_HIP_CHK(hipMemsetAsync(dcount, 0, sizeof(int32_t) * n_candidates, st));
            if (T.slots) {
                SFMX_HIP_CHK(hipMemsetAsync(tk, 0xff, sizeof(unsigned long long) * T.slots, st));
                SFMX_HIP_CHK(hipMemsetAsync(tv, 0x7f, sizeof(int32_t) * T.slots, st));
            }
            if (T.items)
                build_tables_kernel<<<(unsigned)((T.items + 255) / 256), 256, 0, st>>>(usd, ufd, (int)n_used, T.items, G.doff, G.dm,
                                                                                      G.kpd, G.nkd, G.prd, tk, tv);
            if (T.items && n_origins)
                count_kernel<<<(unsigned)((n_origins + 255) / 256), 256, 0, st>>>(n_origins, G.dshot, G.dxy, n_shots, tfd, usd, tk, tv,
                                                                                G.doff, G.dm, ncd, n_candidates, dcount);
            (void)hipEventRecord(S->e1, st);
            SFMX_HIP_CHK(hipGetLastError());
            SFMX_HIP_CHK(F.back(out_count, cd, n_candidates));
            SFMX_HIP_CHK(hipStreamSynchronize(st));
            float ms = -1.f;
            (void)hipEventElapsedTime(&ms, S->e0, S->e1);
            g_count_ms = ms;
        }
    done:;
        rc = F.finish(rc, "sfmx_count_3d2d_matches");
    }
    return rc;
}

int sfmx_ba_observations_from_origins(const int64_t* origin_offsets, int32_t n_points, const int32_t* origin_shot,
                                      const double* origin_xy, int32_t n_shots, int32_t* obs_point, int32_t* obs_cam,
                                      double* obs_xy, int32_t* pose_of_shot, int32_t* shot_of_pose, int32_t* n_poses) {
    if (n_points < 0 || n_shots < 0 || !origin_offsets || !pose_of_shot || !shot_of_pose || !n_poses) {
        set_last_error("bad argument");
        return SFMX_EINVAL;
    }
    const int64_t n = origin_offsets[n_points];
    if (n && (!origin_shot || !origin_xy || !obs_point || !obs_cam || !obs_xy)) { set_last_error("null array"); return SFMX_EINVAL; }
    for (int s = 0; s < n_shots; ++s) pose_of_shot[s] = -1;
    int32_t np = 0;
    for (int p = 0; p < n_points; ++p) {
        if (origin_offsets[p + 1] < origin_offsets[p]) { set_last_error("origin offsets not ascending"); return SFMX_EINVAL; }
        for (int64_t r = origin_offsets[p]; r < origin_offsets[p + 1]; ++r) {
            const int s = origin_shot[r];
            if (s < 0 || s >= n_shots) { set_last_error("origin shot out of range"); return SFMX_EINVAL; }
            if (pose_of_shot[s] < 0) { pose_of_shot[s] = np; shot_of_pose[np] = s; ++np; }   // BundleAdjustment.cpp:64-79
            obs_point[r] = p;
            obs_cam[r] = pose_of_shot[s];
            obs_xy[2 * r] = (double)(float)origin_xy[2 * r];           // cv::Point2d -> cv::Point2f (ICamera.h:161)
            obs_xy[2 * r + 1] = (double)(float)origin_xy[2 * r + 1];
        }
    }
    *n_poses = np;
    return SFMX_OK;
}

}  // extern "C"
