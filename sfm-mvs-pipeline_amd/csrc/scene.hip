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
Slot g_count_slot[64];   // csrc/device_call.hpp

struct Bufs {
    std::vector<void*> ptrs;
    ~Bufs() { for (void* q : ptrs) (void)hipFree(q); }
    void* alloc(size_t bytes) {
        void* q = nullptr;
        if (hipMalloc(&q, std::max<size_t>(bytes, 16)) != hipSuccess) return nullptr;
        ptrs.push_back(q);
        return q;
    }
};

}  // namespace scene
}  // namespace sfmx

using namespace sfmx;
using namespace sfmx::scene;

#define SCHK(expr) do { if ((expr) != hipSuccess) { rc = SFMX_EDEVICE; set_last_error("HIP error in " #expr); goto done; } } while (0)

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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_last_error("no HIP device visible"); return SFMX_EDEVICE; }
    if (device < 0 || device >= ndev) { set_last_error("device index out of range"); return SFMX_EINVAL; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_last_error("sfmx kernels are built for gfx950 only");
        return SFMX_EDEVICE;
    }
    for (int p = 0; p < n_pairs; ++p)
        if (pairs[2 * p] < 0 || pairs[2 * p] >= n_shots || pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= n_shots) {
            set_last_error("pair shot index out of range");
            return SFMX_EINVAL;
        }
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(device);
    const hipStream_t st = (hipStream_t)stream;
    int rc = SFMX_OK;
    {
        Bufs b;
        std::vector<int64_t> hoff(n_pairs + 1, 0), hoo;
        int64_t n_origins = 0;
        // 1. first pair per other shot (Scene.cpp:389-394: find_if over the pair list)
        std::vector<int32_t> first(n_shots, -1);
        std::vector<UsedPair> used;
        std::vector<int32_t> used_of_shot(n_shots, -1), used_first;
        int64_t items = 0, slots = 0;
        if (inputs_on_device) {
            if (n_pairs) SCHK(hipMemcpyAsync(hoff.data(), pair_offsets, sizeof(int64_t) * (n_pairs + 1), hipMemcpyDeviceToHost, st));
            SCHK(hipMemcpyAsync(&n_origins, origin_offsets + n_points, sizeof(int64_t), hipMemcpyDeviceToHost, st));
            SCHK(hipStreamSynchronize(st));
        } else {
            if (n_pairs) std::memcpy(hoff.data(), pair_offsets, sizeof(int64_t) * (n_pairs + 1));
            n_origins = origin_offsets[n_points];
            if (n_origins && (!origin_shot || !origin_xy)) { set_last_error("null origin arrays"); rc = SFMX_EINVAL; goto done; }
        }
        for (int p = 0; p < n_pairs; ++p) {
            const int L = pairs[2 * p], R = pairs[2 * p + 1];
            if (L == R) continue;
            const int o = L == shot ? R : (R == shot ? L : -1);
            if (o >= 0 && first[o] < 0) first[o] = p;
        }
        for (int o = 0; o < n_shots; ++o) {
            const int p = first[o];
            if (p < 0) continue;
            const int64_t m = hoff[p + 1] - hoff[p];
            if (m <= 0) continue;
            int cap = 16;
            while (cap < 2 * m) cap <<= 1;
            used_of_shot[o] = (int32_t)used.size();
            used.push_back(UsedPair{p, pairs[2 * p] == o ? 1 : 0, slots, cap, 0});
            used_first.push_back((int32_t)items);
            items += m;
            slots += cap;
        }
        if (items >= INT32_MAX) { set_last_error("too many matches"); rc = SFMX_EINVAL; goto done; }
        if (!inputs_on_device) {   // host validation of keypoint indices of the used pairs
            for (const UsedPair& u : used)
                for (int64_t i = hoff[u.pair]; i < hoff[u.pair + 1]; ++i) {
                    const int L = pairs[2 * u.pair], R = pairs[2 * u.pair + 1];
                    if (matches[i].queryIdx < 0 || matches[i].queryIdx >= n_keypoints[L] || matches[i].trainIdx < 0 ||
                        matches[i].trainIdx >= n_keypoints[R]) {
                        set_last_error("match index outside its image's keypoints");
                        rc = SFMX_EINVAL;
                        goto done;
                    }
                }
        }
        {
            // device copies of the inputs
            std::vector<const float2*> kptr(std::max(n_shots, 1));
            const DMatchDev* dm = reinterpret_cast<const DMatchDev*>(matches);
            const int64_t* doff = pair_offsets;
            const int32_t* dshot = origin_shot;
            const double* dxy = origin_xy;
            int32_t *dokp = out_keypoint, *dopair = out_pair;
            float* doxy = out_xy;
            if (inputs_on_device) {
                for (int i = 0; i < n_shots; ++i) kptr[i] = reinterpret_cast<const float2*>(keypoints[i]);
            } else {
                int64_t nk = 0;
                for (int i = 0; i < n_shots; ++i) nk += n_keypoints[i];
                auto* kd = static_cast<float2*>(b.alloc(sizeof(float2) * nk));
                auto* md = static_cast<DMatchDev*>(b.alloc(sizeof(DMatchDev) * std::max<int64_t>(hoff[n_pairs], 1)));
                auto* od = static_cast<int64_t*>(b.alloc(sizeof(int64_t) * (n_pairs + 1)));
                auto* sd = static_cast<int32_t*>(b.alloc(sizeof(int32_t) * std::max<int64_t>(n_origins, 1)));
                auto* xd = static_cast<double*>(b.alloc(sizeof(double) * 2 * std::max<int64_t>(n_origins, 1)));
                dokp = static_cast<int32_t*>(b.alloc(sizeof(int32_t) * std::max<int64_t>(n_origins, 1)));
                dopair = static_cast<int32_t*>(b.alloc(sizeof(int32_t) * std::max<int64_t>(n_origins, 1)));
                doxy = out_xy ? static_cast<float*>(b.alloc(sizeof(float) * 2 * std::max<int64_t>(n_origins, 1))) : nullptr;
                if (!kd || !md || !od || !sd || !xd || !dokp || !dopair || (out_xy && !doxy)) { rc = SFMX_ENOMEM; goto done; }
                int64_t o = 0;
                for (int i = 0; i < n_shots; ++i) {
                    if (n_keypoints[i]) SCHK(hipMemcpyAsync(kd + o, keypoints[i], sizeof(float2) * n_keypoints[i], hipMemcpyHostToDevice, st));
                    kptr[i] = kd + o;
                    o += n_keypoints[i];
                }
                if (hoff[n_pairs]) SCHK(hipMemcpyAsync(md, matches, sizeof(DMatchDev) * hoff[n_pairs], hipMemcpyHostToDevice, st));
                SCHK(hipMemcpyAsync(od, pair_offsets, sizeof(int64_t) * (n_pairs + 1), hipMemcpyHostToDevice, st));
                if (n_origins) {
                    SCHK(hipMemcpyAsync(sd, origin_shot, sizeof(int32_t) * n_origins, hipMemcpyHostToDevice, st));
                    SCHK(hipMemcpyAsync(xd, origin_xy, sizeof(double) * 2 * n_origins, hipMemcpyHostToDevice, st));
                }
                dm = md; doff = od; dshot = sd; dxy = xd;
            }
            auto* kpd = static_cast<const float2**>(b.alloc(sizeof(float2*) * kptr.size()));
            auto* nkd = static_cast<int32_t*>(b.alloc(sizeof(int32_t) * std::max(n_shots, 1)));
            auto* prd = static_cast<int32_t*>(b.alloc(sizeof(int32_t) * 2 * std::max(n_pairs, 1)));
            auto* usd = static_cast<UsedPair*>(b.alloc(sizeof(UsedPair) * std::max<size_t>(used.size(), 1)));
            auto* ufd = static_cast<int32_t*>(b.alloc(sizeof(int32_t) * std::max<size_t>(used_first.size(), 1)));
            auto* uos = static_cast<int32_t*>(b.alloc(sizeof(int32_t) * std::max(n_shots, 1)));
            auto* tk = static_cast<unsigned long long*>(b.alloc(sizeof(unsigned long long) * std::max<int64_t>(slots, 1)));
            auto* tv = static_cast<int32_t*>(b.alloc(sizeof(int32_t) * std::max<int64_t>(slots, 1)));
            if (!kpd || !nkd || !prd || !usd || !ufd || !uos || !tk || !tv) { rc = SFMX_ENOMEM; goto done; }
            SCHK(hipMemcpyAsync(kpd, kptr.data(), sizeof(float2*) * kptr.size(), hipMemcpyHostToDevice, st));
            SCHK(hipMemcpyAsync(nkd, n_keypoints, sizeof(int32_t) * n_shots, hipMemcpyHostToDevice, st));
            if (n_pairs) SCHK(hipMemcpyAsync(prd, pairs, sizeof(int32_t) * 2 * n_pairs, hipMemcpyHostToDevice, st));
            if (!used.empty()) {
                SCHK(hipMemcpyAsync(usd, used.data(), sizeof(UsedPair) * used.size(), hipMemcpyHostToDevice, st));
                SCHK(hipMemcpyAsync(ufd, used_first.data(), sizeof(int32_t) * used_first.size(), hipMemcpyHostToDevice, st));
            }
            SCHK(hipMemcpyAsync(uos, used_of_shot.data(), sizeof(int32_t) * n_shots, hipMemcpyHostToDevice, st));
            hipEvent_t e0 = nullptr, e1 = nullptr;
            SCHK(hipEventCreate(&e0));
            SCHK(hipEventCreate(&e1));
            SCHK(hipEventRecord(e0, st));
            if (slots) {
                SCHK(hipMemsetAsync(tk, 0xff, sizeof(unsigned long long) * slots, st));
                SCHK(hipMemsetAsync(tv, 0x7f, sizeof(int32_t) * slots, st));
            }
            if (items)
                build_tables_kernel<<<(unsigned)((items + 255) / 256), 256, 0, st>>>(usd, ufd, (int)used.size(), items, doff, dm,
                                                                                    kpd, nkd, prd, tk, tv);
            if (n_origins)
                lookup_kernel<<<(unsigned)((n_origins + 255) / 256), 256, 0, st>>>(n_origins, dshot, dxy, shot, n_shots, uos, usd,
                                                                                 tk, tv, doff, dm, kpd, nkd, dokp, dopair, doxy);
            SCHK(hipGetLastError());
            SCHK(hipEventRecord(e1, st));
            if (!inputs_on_device && n_origins) {
                SCHK(hipMemcpyAsync(out_keypoint, dokp, sizeof(int32_t) * n_origins, hipMemcpyDeviceToHost, st));
                SCHK(hipMemcpyAsync(out_pair, dopair, sizeof(int32_t) * n_origins, hipMemcpyDeviceToHost, st));
                if (out_xy) SCHK(hipMemcpyAsync(out_xy, doxy, sizeof(float) * 2 * n_origins, hipMemcpyDeviceToHost, st));
            }
            SCHK(hipStreamSynchronize(st));
            float ms = -1.f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            g_last_ms = ms;
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
        }
    done:;
    }
    if (rc == SFMX_ENOMEM) set_last_error("device allocation failed");
    if (prev >= 0) (void)hipSetDevice(prev);
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
    for (int s = 0; s < n_shots; ++s)
        if (n_keypoints[s] < 0) { set_last_error("negative keypoint count"); return SFMX_EINVAL; }
    for (int p = 0; p < n_pairs; ++p)
        if (pairs[2 * p] < 0 || pairs[2 * p] >= n_shots || pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= n_shots) {
            set_last_error("pair shot index out of range");
            return SFMX_EINVAL;
        }
    std::vector<int32_t> cand_of_shot(n_shots, -1);
    for (int c = 0; c < n_candidates; ++c) {
        const int s = candidates[c];
        if (s < 0 || s >= n_shots) { set_last_error("candidate shot index out of range"); return SFMX_EINVAL; }
        if (cand_of_shot[s] >= 0) { set_last_error("candidate shot listed twice"); return SFMX_EINVAL; }
        cand_of_shot[s] = c;
    }
    if (!inputs_on_device) {
        if (origin_offsets[0] != 0) { set_last_error("origin offsets do not start at 0"); return SFMX_EINVAL; }
        for (int p = 0; p < n_points; ++p)
            if (origin_offsets[p + 1] < origin_offsets[p]) { set_last_error("origin offsets not ascending"); return SFMX_EINVAL; }
        if (origin_offsets[n_points] && (!origin_shot || !origin_xy)) { set_last_error("null origin arrays"); return SFMX_EINVAL; }
    }
    if (n_candidates == 0) { g_count_ms = 0.f; return SFMX_OK; }   // nothing to write
    DeviceCall F(stream, !inputs_on_device);
    const hipStream_t st = F.st;
    {
        const int orc = F.open(g_count_slot, device);
        if (orc != SFMX_OK) return orc;
    }
    Slot* const S = F.S;
    int rc = SFMX_OK;
    {
        struct Entry { int32_t other, cand, pair; };
        std::vector<int64_t> hoff(n_pairs + 1, 0);
        std::vector<Entry> ent;
        int64_t n_origins = 0, items = 0, slots = 0, nk = 0, n_matches = 0;
        size_t n_used = 0;
        if (inputs_on_device) {
            if (n_pairs) SFMX_HIP_CHK(hipMemcpyAsync(hoff.data(), pair_offsets, sizeof(int64_t) * (n_pairs + 1), hipMemcpyDeviceToHost, st));
            SFMX_HIP_CHK(hipMemcpyAsync(&n_origins, origin_offsets + n_points, sizeof(int64_t), hipMemcpyDeviceToHost, st));
            SFMX_HIP_CHK(hipStreamSynchronize(st));
        } else {
            if (n_pairs) std::memcpy(hoff.data(), pair_offsets, sizeof(int64_t) * (n_pairs + 1));
            n_origins = origin_offsets[n_points];
        }
        if (hoff[0] != 0) { set_last_error("pair offsets do not start at 0"); rc = SFMX_EINVAL; goto done; }
        for (int p = 0; p < n_pairs; ++p)
            if (hoff[p + 1] < hoff[p]) { set_last_error("pair offsets not ascending"); rc = SFMX_EINVAL; goto done; }
        n_matches = hoff[n_pairs];
        if (n_origins < 0 || (n_origins + 255) / 256 > INT32_MAX) { set_last_error("origin record count out of range"); rc = SFMX_EINVAL; goto done; }
        if (n_matches && !matches) { set_last_error("null argument"); rc = SFMX_EINVAL; goto done; }
        // per (origin shot o, candidate s): the first visible pair in list order joining {s, o} (Scene.cpp:389-394)
        for (int p = 0; p < n_pairs; ++p) {
            const int L = pairs[2 * p], R = pairs[2 * p + 1];
            if (L == R || (pair_active && !pair_active[p])) continue;
            if (cand_of_shot[L] >= 0) ent.push_back(Entry{R, cand_of_shot[L], p});
            if (cand_of_shot[R] >= 0) ent.push_back(Entry{L, cand_of_shot[R], p});
        }
        std::stable_sort(ent.begin(), ent.end(), [](const Entry& a, const Entry& b) {
            return a.other != b.other ? a.other < b.other : a.cand < b.cand;
        });
        for (size_t i = ent.size(); i-- > 1;)   // only the first of every (o, s) run counts
            if (ent[i].other == ent[i - 1].other && ent[i].cand == ent[i - 1].cand) ent[i].pair = -1;
        for (size_t i = 0; i < ent.size(); ++i) {   // a first pair without matches has no table: no match through it
            const int p = ent[i].pair;
            if (p < 0) continue;
            const int64_t m = hoff[p + 1] - hoff[p];
            if (m <= 0) { ent[i].pair = -1; continue; }
            if (!inputs_on_device) {   // host validation of the keypoint indices of the pairs that are read
                const int L = pairs[2 * p], R = pairs[2 * p + 1];
                for (int64_t k = hoff[p]; k < hoff[p + 1]; ++k)
                    if (matches[k].queryIdx < 0 || matches[k].queryIdx >= n_keypoints[L] || matches[k].trainIdx < 0 ||
                        matches[k].trainIdx >= n_keypoints[R]) {
                        set_last_error("match index outside its image's keypoints");
                        rc = SFMX_EINVAL;
                        goto done;
                    }
            }
            if (m > ((int64_t)1 << 29)) { set_last_error("a match list beyond 2^29 entries"); rc = SFMX_ECAPACITY; goto done; }   // its table's capacity is an int32
            ++n_used;
            items += m;
        }
        if (items >= INT32_MAX || n_used >= (size_t)INT32_MAX) { set_last_error("too many matches"); rc = SFMX_ECAPACITY; goto done; }
        if (!inputs_on_device)
            for (int i = 0; i < n_shots; ++i) nk += n_keypoints[i];
        {
            // device block: [tables of the call | hash tables | (host inputs: keypoints, matches, offsets, origins, counts)]
            const bool H = F.host;
            BlockLayout L;
            UsedPair* usd;
            int32_t *ufd, *tfd, *nkd, *ncd, *prd, *tv, *sd, *cd;
            const float2** kpd;
            unsigned long long* tk;
            float2* kd;
            sfmx_dmatch* md;
            int64_t* od;
            double* xd;
            L.want(usd, n_used);
            L.want(ufd, n_used);
            L.want(tfd, (size_t)n_shots + 1);
            L.want(nkd, n_shots);
            L.want(ncd, n_candidates);
            L.want(prd, 2 * (size_t)n_pairs);
            L.want(kpd, n_shots);
            const size_t b_tab = L.need;   // up to here: staged in pinned memory, one upload
            for (const Entry& en : ent) {
                if (en.pair < 0) continue;
                const int64_t m = hoff[en.pair + 1] - hoff[en.pair];
                int64_t cap = 16;
                while (cap < 2 * m) cap <<= 1;
                slots += cap;
            }
            L.want(tk, slots);
            L.want(tv, slots);
            L.want(kd, nk, H);
            L.want(md, n_matches, H);
            L.want(od, (size_t)n_pairs + 1, H);
            L.want(sd, n_origins, H);
            L.want(xd, 2 * (size_t)n_origins, H);
            L.want(cd, n_candidates, H);
            rc = F.reserve(L, b_tab);
            if (rc != SFMX_OK) goto done;
            UsedPair* hu = F.pinned(usd);
            int32_t *huf = F.pinned(ufd), *htf = F.pinned(tfd);
            size_t u = 0;
            int64_t it = 0, sl = 0;
            for (int o = 0; o <= n_shots; ++o) htf[o] = 0;
            for (const Entry& en : ent) {
                if (en.pair < 0) continue;
                const int64_t m = hoff[en.pair + 1] - hoff[en.pair];
                int64_t cap = 16;
                while (cap < 2 * m) cap <<= 1;
                hu[u] = UsedPair{en.pair, pairs[2 * en.pair] == en.other ? 1 : 0, sl, (int32_t)cap, en.cand};
                huf[u] = (int32_t)it;
                ++htf[en.other + 1];
                ++u;
                it += m;
                sl += cap;
            }
            for (int o = 0; o < n_shots; ++o) htf[o + 1] += htf[o];
            std::memcpy(F.pinned(nkd), n_keypoints, sizeof(int32_t) * n_shots);
            for (int c = 0; c < n_candidates; ++c) F.pinned(ncd)[c] = n_keypoints[candidates[c]];
            if (n_pairs) std::memcpy(F.pinned(prd), pairs, sizeof(int32_t) * 2 * n_pairs);
            const float2** hk = F.pinned(kpd);
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
            SFMX_HIP_CHK(F.upload(b_tab));
            const DMatchDev* dm = reinterpret_cast<const DMatchDev*>(n_matches ? F.in(matches, md, n_matches) : matches);
            const int64_t* doff = n_pairs ? F.in(pair_offsets, od, (size_t)n_pairs + 1) : pair_offsets;
            const int32_t* dshot = n_origins ? F.in(origin_shot, sd, n_origins) : origin_shot;
            const double* dxy = n_origins ? F.in(origin_xy, xd, 2 * (size_t)n_origins) : origin_xy;
            SFMX_HIP_CHK(F.err);
            int32_t* dcount = F.out(out_count, cd);
            (void)hipEventRecord(S->e0, st);
            SFMX_HIP_CHK(hipMemsetAsync(dcount, 0, sizeof(int32_t) * n_candidates, st));
            if (slots) {
                SFMX_HIP_CHK(hipMemsetAsync(tk, 0xff, sizeof(unsigned long long) * slots, st));
                SFMX_HIP_CHK(hipMemsetAsync(tv, 0x7f, sizeof(int32_t) * slots, st));
            }
            if (items)
                build_tables_kernel<<<(unsigned)((items + 255) / 256), 256, 0, st>>>(usd, ufd, (int)n_used, items, doff, dm, kpd,
                                                                                    nkd, prd, tk, tv);
            if (items && n_origins)
                count_kernel<<<(unsigned)((n_origins + 255) / 256), 256, 0, st>>>(n_origins, dshot, dxy, n_shots, tfd, usd, tk, tv,
                                                                                doff, dm, ncd, n_candidates, dcount);
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
