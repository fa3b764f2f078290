// SPDX-License-Identifier: MIT
// sfmx matcher — host driver behind the C ABI (include/sfmx.h).
//
// Mirrors the reference's strategy call
//   IFeatureMatchingStrategy::calculateShotMatches(scene, matcher, out)
//   (src/photogrammetrie/sfm/IFeatureMatchingStrategy.h:45-46, e.g.
//    UnorderedFeatureMatchingStrategy.cpp:27-90)
// followed by SfM::calculateShotMatches' filters (sfm/SfM.cpp:542-575):
//   set_images  = the descriptor matrices the Scene's shots own (CameraShot.h:39-42),
//                 uploaded once into an HBM pool and prepared (int8 + norms)
//   run         = the OpenMP pair loop (:40-88) as one batched launch sequence
//   fetch       = the vector<ShotMatches> hand-back, as packed DMatch lists
// No CPU fallback: every numeric step runs in the HIP kernels of
// match_kernels.hip (the diagnostic library's other routes: match_diag.hip); a
// missing/unsupported device returns SFMX_EDEVICE.
#include <hip/hip_runtime.h>
#include "diag.hpp"
#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sfmx.h"
#include "match_common.hpp"
#include "sift_fp6.hpp"

using namespace sfmx;

namespace {

thread_local std::string g_last_error;
}  // namespace
void sfmx::set_last_error(const char* msg) { g_last_error = msg ? msg : ""; }
namespace {

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(e_ == hipErrorOutOfMemory ? SFMX_ENOMEM : SFMX_EDEVICE,               \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                   \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return SFMX_OK;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        const size_t want = std::max<size_t>(bytes, 256);
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return fail(SFMX_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e)); }
        cap = want;
        return SFMX_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
// A typed view of memory another DevBuf owns.
struct DevView {
    void* p = nullptr;
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// Pinned host staging for small H2D uploads (prep table, pair/work lists): truly
// asynchronous copies.  `busy` is recorded after the copies that read the buffer;
// a writer waits for it first, so a copy still in flight is never overwritten.
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipEvent_t busy = nullptr;
    bool pending = false;
    int ensure(size_t bytes) {
        if (pending) { (void)hipEventSynchronize(busy); pending = false; }
        if (bytes <= cap) return SFMX_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        const size_t want = std::max<size_t>(bytes, 4096);
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return fail(SFMX_ENOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
        cap = want;
        return SFMX_OK;
    }
    int copied(hipStream_t st) {     // call after enqueueing the copies that read the buffer
        if (!busy && hipEventCreateWithFlags(&busy, hipEventDisableTiming) != hipSuccess) return fail(SFMX_EDEVICE, "hipEventCreate");
        if (hipEventRecord(busy, st) != hipSuccess) return fail(SFMX_EDEVICE, "hipEventRecord");
        pending = true;
        return SFMX_OK;
    }
    void release() {
        if (pending) (void)hipEventSynchronize(busy);
        if (busy) (void)hipEventDestroy(busy);
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0; busy = nullptr; pending = false;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// Device guard: set the matcher's device for the duration of a call.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) { (void)hipGetDevice(&prev); (void)hipSetDevice(dev); }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace

struct sfmx_matcher {
    int device = 0;
    int norm = 0;
    bool orb_fp4 = false;   // ORB rows expanded to +-1 FP4 (MFMA forms), else 32-byte rows (MatchRoute::ORB_VALU): set_images' route
    int n_imgs = 0;
    std::vector<ImgDev> imgs;
    int64_t total_rows = 0;
    int max_rows = 0;
    bool any_nonintegral = false;
    DevBuf raw, desc8, normv, keyc, keyc2, f32, flags;
    // One allocation, PrepImg[n] | ImgDev[n], so that set_images_device uploads both tables with one copy
    DevBuf tabs;
    DevView prep_tab, imgs_d;        // batched SIFT prep: one PrepImg per image; the kernels' image table
    // Last-arriver tickets and the prepare kernel's partial maxima (match_common.hpp SCRATCH_*).  The kernels
    // leave the tickets, and the prepare kernel the integrality flags, at zero.  scratch_clean says that they are:
    // set_images and run clear it on entry and set it on success, so after an error return (a failed launch, a
    // stream error, a call stopped half-way) the next call zeroes flags and scratch with one explicit fill each.
    DevBuf scratch;
    bool scratch_clean = false;
    int64_t flags_split = 0;         // n_flags of the last set_images: flags[n_flags] | imax[2 n_flags]
    // FP6 screen (sift_fp6.hpp): packed e2m3 rows, f32 C-operand keys, (|u - 32|^2, |e|^2) per row; the
    // per-image maxima of |e|^2 and |u - 32|^2 live behind the integrality flags (imax: one fill for both)
    DevBuf desc6, keyf, ne;
    DevView imax;
    // run state
    int n_pairs = 0;
    int64_t dense_total = 0;
    int64_t fp32_pairs = 0;
    DevBuf pairs_d, work_d, work32_d, dense_idx, dense_dist, slow_list, counts, keep, offsets, out;
    DevBuf qlist, qcount;   // two-pass SIFT path: per pair, the queries the screening pass could not settle
    // One zeroed arena per run, a single fill: qcount[n_pairs] | the persistent screens' 8 XCD tickets |
    // slow_count | unsettled | qcount2[n_pairs] (match_common.hpp; views into qcount's allocation, set by every run)
    DevView slow_count;              // int32: length of slow_list
    DevBuf qmask, top2;     // subset pass 2: per forwarded query its row-subset mask; per query the merged top-2 keys
    DevBuf porder, work2, work2_n;   // pair order (by train image) and the compacted pass-2 work list
    DevBuf recs;                     // list path: one flat PairRec per pair, in porder order
    DevView unsettled;               // int32: pass-1 forwarded queries pass 2 never wrote (must stay 0)
    PinnedBuf stage_prep, stage_run, stage_imgs, stage_flags; // pinned staging of the small uploads / flag readback
    int32_t* hflags = nullptr;   // host-coherent mapped: integrality flags [hflags_cap] + sequence word (prep_l2_batch_kernel's last workgroup)
    int hflags_cap = 0;
    unsigned flag_seq = 0;
    // Run plan cache: the device pair/work lists of the last run stay valid while the
    // pair list, the images' row counts and integrality and the run's route are unchanged.
    std::vector<int32_t> plan_pairs;
    std::vector<int64_t> plan_imgs;
    MatchRoute plan_route;
    bool plan_valid = false;
    int64_t plan_dense = 0;
    size_t plan_nwork = 0, plan_nwork32 = 0;
    int plan_max_nt = 0, plan_max_nq = 0;
    bool has_run = false;
    // per run: start, main kernel end, run end, pass-1 end; a ring of EV_RING sets (r06) so the timing
    // of every run of a loop is readable afterwards (sfmx_matcher_timing_history) without a host sync
    // inside it; ev points at the current run's set
    static constexpr int EV_RING = 32;
    hipEvent_t evr[EV_RING][4] = {};
    hipEvent_t* ev = evr[0];
    long long runs = 0;
    bool ev_recorded = false;
    // overlapped two-pass matching (a route of more than one batch): the plan's batches, two more streams
    std::vector<MatchBatch> batches;
    hipStream_t sx = nullptr, sp = nullptr;
    hipEvent_t ov_ev[3] = {nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> bev;
    // r05: device-resident descriptors (set_images_device) are not waited on for their integrality:
    // the run assumes every image integral (SIFT descriptors always are) and the assumption is checked
    // when results are read (fetch / stats / device_results); a non-integral image then gets its fp32
    // rows and the last run is re-run on the exact paths.  The host no longer waits mid-step.
    bool flags_pending = false;
    unsigned flags_want = 0;
    hipStream_t flags_stream = nullptr;
    std::vector<const void*> last_src;     // the device descriptors of the last set_images_device
    hipStream_t run_stream = nullptr;      // the stream of the last run (the re-run is ordered behind it)
    hipEvent_t fix_ev[2] = {nullptr, nullptr};   // set-stream point / re-run end (resolve_flags)
    std::vector<int> last_cols;
    bool run_spec = false;                 // the last run assumed integrality not yet confirmed
    std::vector<int32_t> last_pairs;
    double last_ratio = 0.0;
    int last_distinct = 0, last_min_count = 0;
};

namespace {

int check_device(int dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(SFMX_EDEVICE, "no HIP device visible");
    if (dev < 0 || dev >= n) return fail(SFMX_EINVAL, "device index out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return fail(SFMX_EDEVICE, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SFMX_EDEVICE, std::string("sfmx kernels are built for gfx950 only, device is ") + prop.gcnArchName);
    return SFMX_OK;
}

// The route of a run (MatchRoute).  The product library has one, from constants.  The diagnostic library reads
// the matcher's switches here and nowhere else, per run (tests switch routes within one process):
//   SFMX_SIFT_VARIANT   0 (product), SIFT_VARIANT_* of diag.hpp (110-113), 103 / 106 / 107 / 108 (int8 screens:
//                       32x32x32, and 16x16x64 in three tilings), 100 / 30 / 31 (single pass)
//   SFMX_SIFT_P2        10 (the route's own pass 2), or full-row GATHER items into the dense arrays behind an
//                       int8 screen: 0 = 128 queries, 1 / 3 = 256 (2 x 4 and 4 x 2 waves), 4 = 512
//   SFMX_ORB_VARIANT    0 (product), 1 (VALU, 32-byte rows), 4 / 5 / 7 / 9 (single pass), 12 / 13 / 14 (full-row pass 2)
//   SFMX_MATCH_BATCHES  1..64 overlapped batches of the int8 SIFT / the ORB product kernels
//   SFMX_SCREEN_PERSIST 1 = ticket-fed persistent screens
//   SFMX_FULL_ROW_GRID  grid of the product path's full-row launch
// A value not listed fails the run (SFMX_EINVAL) instead of timing some other kernel.
#ifndef SFMX_DIAG
int resolve_route(int, MatchRoute& r) {
    r = MatchRoute{};
    return SFMX_OK;
}
#else
int resolve_route(int norm, MatchRoute& r) {
    using R = MatchRoute;
    r = R{};
    const auto value = [](const char* name, int dflt, std::string& text) {
        const char* e = SFMX_DIAG_ENV(name);
        text = std::string(name) + "=" + (e ? e : "");
        return e ? atoi(e) : dflt;
    };
    std::string t_sv, t_p2, t_ov, t_nb, t_grid, t_persist;
    const int sv = value("SFMX_SIFT_VARIANT", 0, t_sv), p2 = value("SFMX_SIFT_P2", 10, t_p2);
    const int ov = value("SFMX_ORB_VARIANT", 0, t_ov);
    const int nb = std::max(1, std::min(64, value("SFMX_MATCH_BATCHES", 1, t_nb)));
    const int grid = value("SFMX_FULL_ROW_GRID", INT_MIN, t_grid);
    r.persist = value("SFMX_SCREEN_PERSIST", 0, t_persist) == 1;
    const auto unknown = [](const std::string& text) { return fail(SFMX_EINVAL, "unknown or removed switch value " + text); };
    if (norm != SFMX_NORM_L2) {
        switch (ov) {
        case 0: r.orb = R::ORB_SUBSET; break;
        case 1: r.orb = R::ORB_VALU; break;
        case 4: r.orb = R::ORB_SINGLE_32_W16; break;
        case 5: r.orb = R::ORB_SINGLE_16; break;
        case 7: r.orb = R::ORB_SINGLE_16_W8; break;
        case 9: r.orb = R::ORB_SINGLE_32_MINW1; break;
        case 12: r.orb = R::ORB_GATHER_512; break;
        case 13: r.orb = R::ORB_GATHER_128; break;
        case 14: r.orb = R::ORB_GATHER_256; break;
        default: return unknown(t_ov);
        }
        r.batches = ov == 0 ? nb : 1;   // the overlapped form exists for the product kernels
        return SFMX_OK;
    }
    r.full_row_grid = grid == INT_MIN ? 0 : std::max(1, grid);
    bool fp6 = false;   // a route with a list form
    switch (sv) {
    case 0: fp6 = true; break;
    case SIFT_VARIANT_INT8_LISTS: fp6 = true; r.screen = R::INT8_16; r.pass2 = R::SUBSET; break;
    case SIFT_VARIANT_FP6_FULL: fp6 = true; r.pass2 = R::FULL_ROWS; break;
    case SIFT_VARIANT_FP6_OTHER_SHAPE: fp6 = true; r.screen = R::FP6_32; break;
    case SIFT_VARIANT_FP6_SUBSET_WG: fp6 = true; r.pass2 = R::SUBSET_CERT; break;
    case 103: r.screen = R::INT8_32; break;
    case 106: r.screen = R::INT8_16; break;
    case 107: r.screen = R::INT8_16_S128; break;
    case 108: r.screen = R::INT8_16_W8; break;
    case 100: r.screen = R::NO_SCREEN; r.pass2 = R::SINGLE; break;
    case 30: r.screen = R::NO_SCREEN; r.pass2 = R::SINGLE_MINW1; break;
    case 31: r.screen = R::NO_SCREEN; r.pass2 = R::SINGLE_R01; break;
    default: return unknown(t_sv);
    }
    if (p2 != 10 && p2 != 0 && p2 != 1 && p2 != 3 && p2 != 4) return unknown(t_p2);
    r.sift_lists = fp6 && p2 == 10 && nb == 1 && !r.persist;
    if (r.screen == R::NO_SCREEN || r.sift_lists) return SFMX_OK;
    // two passes into the dense arrays: the list routes' screens give way to the int8 one
    if (fp6) r.screen = R::INT8_16;
    if (p2 == 10) {   // subset pass 2 behind the int8 screen with subset masks; overlapped batches for the r02 default
        r.screen = R::INT8_16;
        r.pass2 = R::SUBSET;
        r.batches = sv == 0 ? nb : 1;
    } else {
        r.pass2 = R::GATHER;
        r.p2_qt = p2 == 0 ? 1 : p2 == 1 ? 2 : 4;
        r.p2_waves = p2 == 3 ? 2 : 4;
    }
    return SFMX_OK;
}

// Batches of the overlapped two-pass path: whole pairs in `order`, about n_work / nb items each.
int plan_batches(sfmx_matcher* m, int nb, const std::vector<PairDev>& pd, const std::vector<int>& order,
                 const std::vector<WorkItem>& work) {
    m->batches.clear();
    const int n_pairs = (int)order.size();
    const int64_t per = ((int64_t)work.size() + nb - 1) / nb;
    MatchBatch cur{0, 0, 0, 0};
    size_t w = 0;
    for (int i = 0; i < n_pairs; ++i) {
        const int p = order[i];
        const bool f32path = m->norm == SFMX_NORM_L2 && !(m->imgs[pd[p].left].integral && m->imgs[pd[p].right].integral);
        int items = 0;
        while (!f32path && w + items < work.size() && work[w + items].pair == p) ++items;
        cur.nw += items;
        cur.np += 1;
        w += items;
        if (cur.nw >= per && i + 1 < n_pairs && w < work.size()) {   // (trailing no-work pairs join the last batch)
            m->batches.push_back(cur);
            cur = MatchBatch{(int32_t)w, 0, i + 1, 0};
        }
    }
    if (cur.np > 0) m->batches.push_back(cur);
    if (w != work.size()) return fail(SFMX_EINTERNAL, "match batches do not cover the work list");
    return SFMX_OK;
}

// The screen and pass 2 of any route: overlapped on the matcher's extra streams where the route has more than
// one batch (and the plan cut the work into at least two), else the route's dispatcher.
int launch_route_diag(sfmx_matcher* m, const MatchRoute& route, const MatchBufs& B, int n_work, int n_pairs, double ratio,
                      hipStream_t st) {
    const bool sift = m->norm == SFMX_NORM_L2;
    if (route.batches > 1 && m->batches.size() >= 2 && n_work > 0) {
        if (!m->sx) {
            HIPCHK(hipStreamCreateWithFlags(&m->sx, hipStreamNonBlocking));
            HIPCHK(hipStreamCreateWithFlags(&m->sp, hipStreamNonBlocking));
            for (auto& e : m->ov_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        while (m->bev.size() < m->batches.size()) {
            hipEvent_t e = nullptr;
            HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            m->bev.push_back(e);
        }
        const OverlapStreams os{m->sx, m->sp, m->ov_ev[0], m->ov_ev[1], m->ov_ev[2], m->bev.data()};
        HIPCHK(launch_two_pass_overlap(sift, m->batches.data(), (int)m->batches.size(), B, n_pairs, ratio, st, m->ev[3], os));
        return SFMX_OK;
    }
    HIPCHK(sift ? launch_sift_diag(route, B, n_work, n_pairs, ratio, st, m->ev[3])
                : launch_orb_diag(route, B, n_work, n_pairs, ratio, st, m->ev[3]));
    return SFMX_OK;
}
#endif

// The tickets' buffer, at least `words` long; zeroed whole when it is allocated or grown, and when the last call
// may have left a ticket behind (dirty: sfmx_matcher::scratch_clean was false).
int ensure_scratch(sfmx_matcher* m, int64_t words, bool dirty, hipStream_t st) {
    const size_t bytes = sizeof(int32_t) * (size_t)align_up(words, 64);
    const bool grown = bytes > m->scratch.cap;
    if (int rc = m->scratch.ensure(bytes)) return rc;
    if (grown || dirty) HIPCHK(hipMemsetAsync(m->scratch.p, 0, m->scratch.cap, st));
    return SFMX_OK;
}

int set_images_impl(sfmx_matcher* m, const sfmx_desc* imgs, int n, int norm, hipStream_t st, bool device_src) {
    if (m) m->flags_pending = m->run_spec = false;   // (a pending check of earlier images is moot now)
    if (!m || (n > 0 && !imgs) || n < 0) return fail(SFMX_EINVAL, "null matcher/images");
    if (norm != SFMX_NORM_L2 && norm != SFMX_NORM_HAMMING) return fail(SFMX_EINVAL, "norm must be SFMX_NORM_L2 or SFMX_NORM_HAMMING");
    const int want_type = norm == SFMX_NORM_L2 ? SFMX_32F : SFMX_8U;
    const int max_cols = norm == SFMX_NORM_L2 ? SIFT_DIM : ORB_BYTES;
    for (int i = 0; i < n; ++i) {
        if (imgs[i].rows < 0 || imgs[i].cols < 0) return fail(SFMX_EINVAL, "negative descriptor shape");
        if (imgs[i].rows > 0 && imgs[i].type != want_type)
            return fail(SFMX_EINVAL, "descriptor type does not match norm (L2 needs CV_32F, HAMMING needs CV_8U)");
        if (imgs[i].rows > 0 && (imgs[i].cols < 1 || imgs[i].cols > max_cols))
            return fail(SFMX_EINVAL, "descriptor width unsupported (SIFT <= 128 floats, ORB <= 32 bytes)");
        if (imgs[i].rows >= (1 << 18))   // cv::BFMatcher asserts train rows < IMGIDX_ONE = 2^18 [ext]
            return fail(SFMX_EINVAL, "more than 2^18 - 1 descriptors in one image");
        if (imgs[i].rows > 0 && !imgs[i].data) return fail(SFMX_EINVAL, "null descriptor data");
    }
    MatchRoute route;   // ORB: the row layout follows the route; run_impl checks its own route against it
    if (int rc_ = resolve_route(norm, route)) return rc_;
    DeviceGuard g(m->device);
    const bool dirty = !m->scratch_clean;   // (see scratch_clean: every return but the last leaves it false)
    m->scratch_clean = false;
    m->norm = norm;
    m->orb_fp4 = norm == SFMX_NORM_HAMMING && route.orb != MatchRoute::ORB_VALU;
    m->n_imgs = n;
    m->imgs.assign(n, ImgDev{});
    m->has_run = false;
    int64_t row = 0, raw_bytes = 0;
    std::vector<int64_t> raw_off(n);
    m->max_rows = 0;
    for (int i = 0; i < n; ++i) {
        ImgDev& d = m->imgs[i];
        d.rows = imgs[i].rows;
        d.rows_pad = (int32_t)align_up(d.rows, ROW_ALIGN);
        d.row0 = row;
        d.integral = 1;
        row += d.rows_pad;
        m->max_rows = std::max(m->max_rows, d.rows);
        const int64_t esz = norm == SFMX_NORM_L2 ? 4 : 1;
        raw_off[i] = raw_bytes;
        raw_bytes += align_up((int64_t)imgs[i].rows * imgs[i].cols * esz, 256);
    }
    m->total_rows = row;
    const int row_bytes = (norm == SFMX_NORM_L2 || m->orb_fp4) ? SIFT_DIM : ORB_BYTES;
    int rc;
    if ((rc = m->desc8.ensure((size_t)row * row_bytes))) return rc;
    const int64_t n_flags = align_up(std::max(n, 1), 64);   // flags[n_flags] | imax[2 n_flags]
    // (a new allocation, or another split of it: imax words of the last call where this call's flags lie)
    const bool relayout = n_flags != m->flags_split;   // (the same for the tickets and partial maxima of `scratch`)
    const bool flags_grown = sizeof(int32_t) * 3 * n_flags > m->flags.cap || relayout;
    if ((rc = m->flags.ensure(sizeof(int32_t) * 3 * n_flags))) return rc;
    m->flags_split = n_flags;
    m->imax.p = m->flags.as<int32_t>() + n_flags;
    if ((rc = m->tabs.ensure((sizeof(PrepImg) + sizeof(ImgDev)) * std::max(n, 1)))) return rc;
    m->prep_tab.p = m->tabs.p;
    m->imgs_d.p = m->tabs.as<PrepImg>() + n;
    if (norm == SFMX_NORM_L2 && (rc = m->normv.ensure((size_t)row * 4))) return rc;
    if ((norm == SFMX_NORM_L2 || m->orb_fp4) && (rc = m->keyc.ensure((size_t)row * 4))) return rc;
    if (norm == SFMX_NORM_L2 && (rc = m->keyc2.ensure((size_t)row * 4))) return rc;
    if (norm == SFMX_NORM_L2) {
        if ((rc = m->desc6.ensure((size_t)row * fp6::ROW_BYTES))) return rc;
        if ((rc = m->keyf.ensure((size_t)row * 4))) return rc;
        if ((rc = m->ne.ensure((size_t)row * sizeof(int2)))) return rc;
    }
    if (!device_src && (rc = m->raw.ensure((size_t)raw_bytes))) return rc;
    // L2: the prepare kernel leaves the flags at zero and stores every imax word it owns, so the fill is for a new
    // allocation or a call that failed half-way.  Hamming: the fill of every call, as before (nothing reads it).
    if (norm != SFMX_NORM_L2 || flags_grown || dirty)
        HIPCHK(hipMemsetAsync(m->flags.p, 0, sizeof(int32_t) * 3 * n_flags, st));   // whole 256-B units: one dispatch
    std::vector<const void*> src(n);
    for (int i = 0; i < n; ++i) {
        const int64_t esz = norm == SFMX_NORM_L2 ? 4 : 1;
        const size_t bytes = (size_t)imgs[i].rows * imgs[i].cols * esz;
        if (device_src) src[i] = imgs[i].data;
        else {
            src[i] = m->raw.as<char>() + raw_off[i];
            if (bytes) HIPCHK(hipMemcpyAsync((void*)src[i], imgs[i].data, bytes, hipMemcpyHostToDevice, st));
        }
    }
    unsigned* hseq = nullptr;
    unsigned want = 0;
    if (norm == SFMX_NORM_L2 && n > 0) {      // one launch for every image
        if ((rc = m->stage_prep.ensure((sizeof(PrepImg) + sizeof(ImgDev)) * n))) return rc;
        PrepImg* tab = m->stage_prep.as<PrepImg>();
        int max_pad = 0;
        for (int i = 0; i < n; ++i) {
            const ImgDev& d = m->imgs[i];
            tab[i] = PrepImg{(const float*)src[i], d.rows, imgs[i].cols, d.rows_pad, 0, d.row0};
            max_pad = std::max(max_pad, d.rows_pad);
        }
        // Device sources: every image counts as integral until the flags say otherwise (flags_pending), so the
        // image table depends on nothing the kernel finds and goes up with the prepare table, in one copy.
        if (device_src) std::memcpy(tab + n, m->imgs.data(), sizeof(ImgDev) * n);
        HIPCHK(hipMemcpyAsync(m->tabs.p, tab, (sizeof(PrepImg) + (device_src ? sizeof(ImgDev) : 0)) * n, hipMemcpyHostToDevice, st));
        if ((rc = m->stage_prep.copied(st))) return rc;
        if ((rc = ensure_scratch(m, scratch_words(n_flags, n, prep_l2_grid_x(max_pad)), dirty || relayout, st))) return rc;
        if (n > m->hflags_cap) {
            if (m->hflags) (void)hipHostFree(m->hflags);
            m->hflags = nullptr;
            m->hflags_cap = 0;
            if (hipHostMalloc(reinterpret_cast<void**>(&m->hflags), sizeof(int32_t) * (n + 4),
                              hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
                return fail(SFMX_ENOMEM, "hipHostMalloc (integrality flags)");
            m->hflags_cap = n;
            m->hflags[n] = 0;
        }
        hseq = reinterpret_cast<unsigned*>(m->hflags + m->hflags_cap);
        want = ++m->flag_seq;
        // the kernel's last workgroup publishes the flags to hflags and release-stores `want` to the sequence word
        HIPCHK(launch_prep_l2_batch(m->prep_tab.as<PrepImg>(), n, max_pad, m->desc8.as<int8_t>(), m->normv.as<int32_t>(),
                                    m->keyc.as<int32_t>(), m->keyc2.as<int32_t>(), m->flags.as<int32_t>(),
                                    m->desc6.as<uint32_t>(), m->keyf.as<float>(), m->ne.as<int2>(), m->imax.as<int32_t>(),
                                    m->scratch.as<int32_t>(), (int)n_flags, FlagHandoff{m->hflags, hseq, want}, st));
    }
    for (int i = 0; i < n && norm != SFMX_NORM_L2; ++i) {
        const ImgDev& d = m->imgs[i];
#ifdef SFMX_DIAG
        if (!m->orb_fp4) {
            HIPCHK(launch_prep_hamming((const uint8_t*)src[i], d.rows, imgs[i].cols, d.rows_pad,
                                       m->desc8.as<uint8_t>() + d.row0 * ORB_BYTES, st));
            continue;
        }
#endif
        HIPCHK(launch_prep_hamming_fp4((const uint8_t*)src[i], d.rows, imgs[i].cols, d.rows_pad,
                                       m->desc8.as<uint8_t>() + d.row0 * SIFT_DIM, m->keyc.as<int32_t>() + d.row0, st));
    }
    m->any_nonintegral = false;
    if (norm == SFMX_NORM_L2 && n > 0) {
        if (device_src) {   // (see flags_pending) every image integral until the flags say otherwise
            m->flags_pending = true;
            m->flags_want = want;
            m->flags_stream = st;
            m->last_src = src;
            m->last_cols.resize(n);
            for (int i = 0; i < n; ++i) m->last_cols[i] = imgs[i].cols;
        }
        for (unsigned spins = 1; !device_src; ++spins) {   // host buffers: the flags before the run is planned
            if (__atomic_load_n(hseq, __ATOMIC_ACQUIRE) == want) break;
            if ((spins & 255) == 0) {
                const hipError_t e = hipStreamQuery(st);
                if (e != hipSuccess && e != hipErrorNotReady) return fail(SFMX_EDEVICE, std::string("set_images: ") + hipGetErrorString(e));
                if (e == hipSuccess && __atomic_load_n(hseq, __ATOMIC_ACQUIRE) != want)
                    return fail(SFMX_EINTERNAL, "set_images: stream drained without the flag handoff");
            }
            __builtin_ia32_pause();
        }
        const int32_t* fl = m->hflags;
        for (int i = 0; i < n && !device_src; ++i) {
            m->imgs[i].integral = fl[i] ? 0 : 1;
            m->any_nonintegral |= fl[i] != 0;
        }
        if (m->any_nonintegral) {
            // every image gets its fp32 rows: a pair takes the fp32 path when EITHER side is
            // non-integral, and then reads both sides from this buffer (an integral partner's rows
            // were left unwritten before r03: stale memory, caught by test_non_integral_fp32_fallback)
            if ((rc = m->f32.ensure((size_t)row * SIFT_DIM * 4))) return rc;
            for (int i = 0; i < n; ++i) {
                const ImgDev& d = m->imgs[i];
                HIPCHK(launch_prep_f32((const float*)src[i], d.rows, imgs[i].cols, d.rows_pad,
                                       m->f32.as<float>() + d.row0 * SIFT_DIM, st));
            }
        }
    }
    if (n > 0 && !(norm == SFMX_NORM_L2 && device_src)) {   // (L2 device sources: went up with the prepare table)
        if ((rc = m->stage_imgs.ensure(sizeof(ImgDev) * n))) return rc;
        std::memcpy(m->stage_imgs.p, m->imgs.data(), sizeof(ImgDev) * n);
        HIPCHK(hipMemcpyAsync(m->imgs_d.p, m->stage_imgs.p, sizeof(ImgDev) * n, hipMemcpyHostToDevice, st));
        if ((rc = m->stage_imgs.copied(st))) return rc;
    }
    if (!device_src) HIPCHK(hipStreamSynchronize(st));   // host buffers may be released by the caller
    m->scratch_clean = true;
    return SFMX_OK;
}

int run_impl(sfmx_matcher* m, const int32_t* pairs, int n_pairs, double ratio, int distinct, int min_count,
             hipStream_t st) {
    if (!m) return fail(SFMX_EINVAL, "null matcher");
    if (m->norm == 0) return fail(SFMX_ESTATE, "run before set_images");
    if (n_pairs < 0 || (n_pairs > 0 && !pairs)) return fail(SFMX_EINVAL, "bad pair list");
    if (!(ratio == ratio)) return fail(SFMX_EINVAL, "ratio is NaN");
    DeviceGuard g(m->device);
    MatchRoute route;
    if (int rc_ = resolve_route(m->norm, route)) return rc_;
    const bool sift = m->norm == SFMX_NORM_L2;
#ifdef SFMX_DIAG
    if (!sift && m->orb_fp4 != (route.orb != MatchRoute::ORB_VALU))   // the layout is set_images' decision
        return fail(SFMX_EINVAL, "SFMX_ORB_VARIANT selects the other descriptor row layout than at set_images");
#endif
    // List path: the product SIFT path and its predecessors (resolve_route).  ORB and every other diagnostic
    // route keep the dense per-query arrays; fp32-fallback pairs of a list run do too, per pair.
    const bool lists = sift && route.sift_lists;
    // Run plan: per-pair dense offsets, the pair order by train image and the work
    // items.  Reused (no host work, no uploads) while the pair list, the images'
    // row counts / integrality and the route are those of the last run.
    std::vector<int64_t> img_key(2 * (size_t)m->n_imgs);
    for (int i = 0; i < m->n_imgs; ++i) { img_key[2 * i] = m->imgs[i].rows; img_key[2 * i + 1] = m->imgs[i].integral; }
    const bool reuse = m->plan_valid && m->plan_route == route && m->plan_imgs == img_key &&
                       m->plan_pairs.size() == 2 * (size_t)n_pairs &&
                       (n_pairs == 0 || std::memcmp(m->plan_pairs.data(), pairs, sizeof(int32_t) * 2 * n_pairs) == 0);
    int rc;
    if (!reuse) {
        m->plan_valid = false;
        std::vector<PairDev> pd(n_pairs);
        int64_t dense = 0;
        for (int p = 0; p < n_pairs; ++p) {
            const int L = pairs[2 * p], R = pairs[2 * p + 1];
            if (L < 0 || L >= m->n_imgs || R < 0 || R >= m->n_imgs) return fail(SFMX_EINVAL, "pair image index out of range");
            pd[p] = PairDev{L, R, dense};
            dense += m->imgs[L].rows;
        }
        // Work items: 512-query blocks, sorted by train image so XCD-contiguous
        // blocks stream the same train rows (L2 reuse); fp32 pairs separately.
        std::vector<WorkItem> work, work32;
        std::vector<int> order(n_pairs);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return pd[a].right < pd[b].right; });
        m->fp32_pairs = 0;
        int max_nt = 0, max_nq = 0;
        std::vector<PairRec> recs;
        if (lists) recs.reserve(n_pairs);
        for (int p : order) {
            const ImgDev& L = m->imgs[pd[p].left];
            const ImgDev& R = m->imgs[pd[p].right];
            max_nt = std::max(max_nt, R.rows);
            max_nq = std::max(max_nq, L.rows);
            const bool f32path = sift && !(L.integral && R.integral);
            m->fp32_pairs += f32path;
            if (lists) recs.push_back(PairRec{L.row0, R.row0, pd[p].dense_base, L.rows, R.rows, R.rows_pad, p, f32path ? 0 : 1, 0});
            const int bq = f32path ? 512 : route.block_queries;
            for (int q0 = 0; q0 < L.rows; q0 += bq) (f32path ? work32 : work).push_back(WorkItem{p, q0});
        }
        if ((rc = m->pairs_d.ensure(sizeof(PairDev) * std::max(n_pairs, 1)))) return rc;
        if ((rc = m->work_d.ensure(sizeof(WorkItem) * std::max<size_t>(work.size(), 1)))) return rc;
        if ((rc = m->work32_d.ensure(sizeof(WorkItem) * std::max<size_t>(work32.size(), 1)))) return rc;
        if (!lists || m->fp32_pairs) {   // the dense per-query results: not touched by a run of list pairs only
            if ((rc = m->dense_idx.ensure(sizeof(int32_t) * std::max<int64_t>(dense, 1)))) return rc;
            if ((rc = m->dense_dist.ensure(sizeof(float) * std::max<int64_t>(dense, 1)))) return rc;
        }
        if (lists && (rc = m->recs.ensure(sizeof(PairRec) * std::max(n_pairs, 1)))) return rc;
        if ((rc = m->slow_list.ensure(sizeof(int2) * std::max<int64_t>(dense, 1)))) return rc;
        if ((rc = m->qlist.ensure(sizeof(int32_t) * std::max<int64_t>(dense, 1)))) return rc;
        if (m->norm == SFMX_NORM_L2 || m->orb_fp4) {
            if ((rc = m->qmask.ensure(sizeof(int32_t) * std::max<int64_t>(dense, 1)))) return rc;
            if ((rc = m->top2.ensure(2 * sizeof(uint64_t) * std::max<int64_t>(dense, 1)))) return rc;
        }
        if ((rc = m->qcount.ensure(sizeof(int32_t) * align_up(arena_words(n_pairs), 64)))) return rc;   // the run's zeroed arena (see qcount)
        m->slow_count.p = m->unsettled.p = nullptr;   // views of the old allocation; set again below
        if ((rc = m->porder.ensure(sizeof(int32_t) * std::max(n_pairs, 1)))) return rc;
        if ((rc = m->work2.ensure(sizeof(WorkItem) * std::max<size_t>(4 * work.size(), 1)))) return rc;   // pass-2 items >= 128 queries
        if ((rc = m->work2_n.ensure(sizeof(int32_t)))) return rc;
        if ((rc = m->counts.ensure(sizeof(int64_t) * std::max(n_pairs, 1)))) return rc;
        if ((rc = m->keep.ensure(sizeof(int32_t) * std::max(n_pairs, 1)))) return rc;
        if ((rc = m->offsets.ensure(sizeof(int64_t) * (n_pairs + 1)))) return rc;
        if ((rc = m->out.ensure(sizeof(DMatchDev) * std::max<int64_t>(dense, 1)))) return rc;
        // uploads from pinned staging: [pairs | order | work | work32 | recs], 256-B aligned parts
        const size_t b_pd = align_up(sizeof(PairDev) * n_pairs, 256), b_or = align_up(sizeof(int32_t) * n_pairs, 256),
                     b_w = align_up(sizeof(WorkItem) * work.size(), 256), b_w32 = align_up(sizeof(WorkItem) * work32.size(), 256),
                     b_rc = sizeof(PairRec) * recs.size();
        if ((rc = m->stage_run.ensure(b_pd + b_or + b_w + b_w32 + b_rc))) return rc;
        char* hs = m->stage_run.as<char>();
        std::memcpy(hs, pd.data(), sizeof(PairDev) * n_pairs);
        std::memcpy(hs + b_pd, order.data(), sizeof(int32_t) * n_pairs);
        std::memcpy(hs + b_pd + b_or, work.data(), sizeof(WorkItem) * work.size());
        std::memcpy(hs + b_pd + b_or + b_w, work32.data(), sizeof(WorkItem) * work32.size());
        std::memcpy(hs + b_pd + b_or + b_w + b_w32, recs.data(), b_rc);
        if (n_pairs) HIPCHK(hipMemcpyAsync(m->pairs_d.p, hs, sizeof(PairDev) * n_pairs, hipMemcpyHostToDevice, st));
        if (n_pairs) HIPCHK(hipMemcpyAsync(m->porder.p, hs + b_pd, sizeof(int32_t) * n_pairs, hipMemcpyHostToDevice, st));
        if (!work.empty()) HIPCHK(hipMemcpyAsync(m->work_d.p, hs + b_pd + b_or, sizeof(WorkItem) * work.size(), hipMemcpyHostToDevice, st));
        if (!work32.empty()) HIPCHK(hipMemcpyAsync(m->work32_d.p, hs + b_pd + b_or + b_w, sizeof(WorkItem) * work32.size(), hipMemcpyHostToDevice, st));
        if (!recs.empty()) HIPCHK(hipMemcpyAsync(m->recs.p, hs + b_pd + b_or + b_w + b_w32, b_rc, hipMemcpyHostToDevice, st));
        if ((rc = m->stage_run.copied(st))) return rc;
#ifdef SFMX_DIAG
        if (route.batches > 1 && (rc = plan_batches(m, route.batches, pd, order, work))) return rc;
#endif
        m->plan_pairs.assign(pairs, pairs + 2 * (size_t)n_pairs);
        m->plan_imgs = img_key;
        m->plan_route = route;
        m->plan_dense = dense;
        m->plan_nwork = work.size();
        m->plan_nwork32 = work32.size();
        m->plan_max_nt = max_nt;
        m->plan_max_nq = max_nq;
        m->plan_valid = true;
    }
    const int64_t dense = m->plan_dense;
    const size_t n_work = m->plan_nwork, n_work32 = m->plan_nwork32;
    if (!m->evr[0][0])
        for (auto& set : m->evr)
            for (auto& e : set) HIPCHK(hipEventCreate(&e));
    m->ev = m->evr[m->runs % sfmx_matcher::EV_RING];
    ++m->runs;
    m->slow_count.p = m->qcount.as<int32_t>() + n_pairs + 8;
    m->unsettled.p = m->qcount.as<int32_t>() + n_pairs + 9;
    // the run's only fill; whole 256-B units, which the runtime clears in one dispatch (no unaligned tail)
    HIPCHK(hipMemsetAsync(m->qcount.p, 0, sizeof(int32_t) * align_up(arena_words(n_pairs), 64), st));
    const bool dirty = !m->scratch_clean;   // (see scratch_clean: every return but the last leaves it false)
    m->scratch_clean = false;
    if ((rc = ensure_scratch(m, SCRATCH_IMG, dirty, st))) return rc;
    HIPCHK(hipEventRecord(m->ev[0], st));
    // ev[3]: the product launchers record it behind the screen whenever there is a work item, and nothing reads it
    // in between (timing, timing_history and pass_timing wait for ev[2] first).  Every other route, and a run
    // without work, keeps the record here (the two-pass launchers of the diagnostic routes record it again).
    const bool product = route.batches == 1 && (sift ? route.sift_product() : route.orb_product());
    if (!(product && n_work > 0)) HIPCHK(hipEventRecord(m->ev[3], st));
    // Pairs with an empty left image have no work item; pairs with an empty
    // right image are handled in-kernel (every query: no neighbour).
    MatchBufs B{};
    B.work = m->work_d.as<WorkItem>();
    B.work32 = m->work32_d.as<WorkItem>();
    B.pairs = m->pairs_d.as<PairDev>();
    B.imgs = m->imgs_d.as<ImgDev>();
    B.porder = m->porder.as<int32_t>();
    B.recs = m->recs.as<PairRec>();
    B.desc8 = m->desc8.as<int8_t>();
    B.norm = m->normv.as<int32_t>();
    B.keyc = m->keyc.as<int32_t>();
    B.keyc2 = m->keyc2.as<int32_t>();
    B.desc6 = m->desc6.as<uint32_t>();
    B.keyf = m->keyf.as<float>();
    B.ne = m->ne.as<int2>();
    B.imax = m->imax.as<int32_t>();
    B.f32 = m->f32.as<float>();
    B.qlist = m->qlist.as<int32_t>();
    B.qcount = m->qcount.as<int32_t>();
    B.qmask = m->qmask.as<int32_t>();
    B.top2 = m->top2.as<unsigned long long>();
    B.slot1 = m->out.as<unsigned long long>();   // pass 2's second slot: `out` is idle until assembly
    B.work2 = m->work2.as<WorkItem>();
    B.work2_n = m->work2_n.as<int32_t>();
    B.dense_idx = m->dense_idx.as<int32_t>();
    B.dense_dist = m->dense_dist.as<float>();
    B.slow_list = m->slow_list.as<int2>();
    B.slow_count = m->slow_count.as<int32_t>();
    B.unsettled = m->unsettled.as<int32_t>();
    B.counts = m->counts.as<int64_t>();
    B.keep = m->keep.as<int32_t>();
    B.offsets = m->offsets.as<int64_t>();
    B.out = m->out.as<DMatchDev>();
    B.scratch = m->scratch.as<int32_t>();
#ifdef SFMX_DIAG
    if ((rc = launch_route_diag(m, route, B, (int)n_work, n_pairs, ratio, st))) return rc;
#else
    HIPCHK(sift ? launch_sift_product(B, (int)n_work, n_pairs, ratio, route.full_row_grid, st, m->ev[3])
                : launch_orb_product(B, (int)n_work, n_pairs, ratio, st, m->ev[3]));
#endif
    if (!lists) HIPCHK(hipEventRecord(m->ev[1], st));
#ifdef SFMX_DIAG
    if (sift && !lists) HIPCHK(launch_sift_slow(B, ratio, st));
#endif
    if (n_work32) HIPCHK(launch_sift_f32(B, (int)n_work32, ratio, st));
    if (lists)   // settle + count (ev[1] behind it), scan, write: the writer of `out` runs after slot1's last reader
        HIPCHK(launch_finish_lists(B, n_pairs, ratio, distinct ? 1 : 0, min_count, m->plan_max_nq, m->plan_max_nt, st, m->ev[1]));
    else
        HIPCHK(launch_assemble(B, n_pairs, distinct ? 1 : 0, min_count, m->plan_max_nt, st));
    HIPCHK(hipEventRecord(m->ev[2], st));
    m->ev_recorded = true;
    m->n_pairs = n_pairs;
    m->dense_total = dense;
    m->has_run = true;
    m->run_stream = st;
    m->run_spec = m->flags_pending;
    if (m->run_spec) {   // what a re-run on the exact paths needs (resolve_flags)
        m->last_pairs.assign(pairs, pairs + 2 * (size_t)n_pairs);
        m->last_ratio = ratio;
        m->last_distinct = distinct;
        m->last_min_count = min_count;
    }
    m->scratch_clean = true;
    return SFMX_OK;
}

// The integrality check of set_images_device, deferred to the first read of results (flags_pending):
// wait for the published flags (long since written); if an image is not integral, give every image
// its fp32 rows, mark the images, and re-run the last run, whose int8 results assumed integrality.
// Ordering: the fp32 prep and the re-run go on the last run's stream, after an event of
// the set stream (the images' prep), so they can neither overlap the original run nor the set; the
// reader's stream then waits on the re-run's end (fetch / stats), or the host does (device_results,
// whose pointers may be used on any stream).  The caller's device descriptors are re-read here:
// sfmx.h requires them to stay valid and unchanged until the run's results are read.
int resolve_flags(sfmx_matcher* m, hipStream_t reader, bool host_wait) {
    if (!m->flags_pending) return SFMX_OK;
    const hipStream_t st = m->flags_stream;
    const int n = m->n_imgs;
    unsigned* hseq = reinterpret_cast<unsigned*>(m->hflags + m->hflags_cap);
    for (unsigned spins = 1;; ++spins) {
        if (__atomic_load_n(hseq, __ATOMIC_ACQUIRE) == m->flags_want) break;
        if ((spins & 255) == 0) {
            const hipError_t e = hipStreamQuery(st);
            if (e != hipSuccess && e != hipErrorNotReady) return fail(SFMX_EDEVICE, std::string("integrality flags: ") + hipGetErrorString(e));
            if (e == hipSuccess && __atomic_load_n(hseq, __ATOMIC_ACQUIRE) != m->flags_want)
                return fail(SFMX_EINTERNAL, "integrality flags: stream drained without the flag handoff");
        }
        __builtin_ia32_pause();
    }
    m->flags_pending = false;
    const int32_t* fl = m->hflags;
    bool any = false;
    for (int i = 0; i < n; ++i) any |= fl[i] != 0;
    if (!any) { m->run_spec = false; return SFMX_OK; }   // the assumption held
    m->any_nonintegral = true;
    for (int i = 0; i < n; ++i) m->imgs[i].integral = fl[i] ? 0 : 1;
    if (!m->fix_ev[0])
        for (auto& e : m->fix_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const hipStream_t rs = m->has_run ? m->run_stream : st;
    if (rs != st) {
        HIPCHK(hipEventRecord(m->fix_ev[0], st));
        HIPCHK(hipStreamWaitEvent(rs, m->fix_ev[0], 0));
    }
    int rc;
    if ((rc = m->f32.ensure((size_t)m->total_rows * SIFT_DIM * 4))) return rc;
    for (int i = 0; i < n; ++i) {
        const ImgDev& d = m->imgs[i];
        HIPCHK(launch_prep_f32((const float*)m->last_src[i], d.rows, m->last_cols[i], d.rows_pad,
                               m->f32.as<float>() + d.row0 * SIFT_DIM, rs));
    }
    if ((rc = m->stage_imgs.ensure(sizeof(ImgDev) * n))) return rc;
    std::memcpy(m->stage_imgs.p, m->imgs.data(), sizeof(ImgDev) * n);
    HIPCHK(hipMemcpyAsync(m->imgs_d.p, m->stage_imgs.p, sizeof(ImgDev) * n, hipMemcpyHostToDevice, rs));
    if ((rc = m->stage_imgs.copied(rs))) return rc;
    m->plan_valid = false;
    if (m->run_spec) {
        m->run_spec = false;
        const std::vector<int32_t> pairs = m->last_pairs;
        if ((rc = run_impl(m, pairs.data(), (int)(pairs.size() / 2), m->last_ratio, m->last_distinct,
                           m->last_min_count, rs))) return rc;
    }
    if (host_wait) HIPCHK(hipStreamSynchronize(rs));
    else if (reader != rs) {
        HIPCHK(hipEventRecord(m->fix_ev[1], rs));
        HIPCHK(hipStreamWaitEvent(reader, m->fix_ev[1], 0));
    }
    return SFMX_OK;
}

int fetch_impl(sfmx_matcher* m, sfmx_dmatch* out, int64_t cap, int64_t* required, int64_t* pair_offsets,
               int32_t* keep, hipStream_t st) {
    if (!m) return fail(SFMX_EINVAL, "null matcher");
    if (!m->has_run) return fail(SFMX_ESTATE, "fetch before run");
    DeviceGuard g(m->device);
    { const int rc_ = resolve_flags(m, st, false); if (rc_) return rc_; }
    std::vector<int64_t> off(m->n_pairs + 1);
    int32_t unsettled = 0;
    HIPCHK(hipMemcpyAsync(off.data(), m->offsets.p, sizeof(int64_t) * (m->n_pairs + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&unsettled, m->unsettled.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (unsettled) return fail(SFMX_EINTERNAL, std::to_string(unsettled) + " forwarded queries were not settled by pass 2");
    const int64_t total = off[m->n_pairs];
    if (required) *required = total;
    if (pair_offsets) std::memcpy(pair_offsets, off.data(), sizeof(int64_t) * (m->n_pairs + 1));
    if (keep && m->n_pairs) HIPCHK(hipMemcpyAsync(keep, m->keep.p, sizeof(int32_t) * m->n_pairs, hipMemcpyDeviceToHost, st));
    if (out) {
        if (cap < total) { HIPCHK(hipStreamSynchronize(st)); return fail(SFMX_ECAPACITY, "output capacity too small"); }
        if (total) HIPCHK(hipMemcpyAsync(out, m->out.p, sizeof(sfmx_dmatch) * total, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return SFMX_OK;
}

}  // namespace

static_assert(sizeof(sfmx_dmatch) == 16 && sizeof(DMatchDev) == 16, "DMatch layout");

extern "C" {

const char* sfmx_version(void) { return "sfmx 0.1 (gfx950)"; }
const char* sfmx_last_error(void) { return g_last_error.c_str(); }

int sfmx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return fail(SFMX_EDEVICE, "hipGetDeviceCount failed");
    int good = 0;
    for (int d = 0; d < n; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++good;
    }
    return good;
}

int sfmx_selftest_sqrt(int32_t device, int64_t n, uint32_t* out_bits) {
    if (n < 0 || n > (int64_t)1 << 24 || (n > 0 && !out_bits)) return fail(SFMX_EINVAL, "n must be in [0, 2^24]");
    int rc = check_device(device);
    if (rc) return rc;
    DeviceGuard g(device);
    DevBuf b;
    if ((rc = b.ensure(sizeof(uint32_t) * std::max<int64_t>(n, 1)))) return rc;
    hipError_t e = launch_selftest_sqrt(n, b.as<uint32_t>(), nullptr);
    if (e == hipSuccess) e = hipMemcpy(out_bits, b.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost);
    b.release();
    if (e != hipSuccess) return fail(SFMX_EDEVICE, hipGetErrorString(e));
    return SFMX_OK;
}

int sfmx_matcher_create(int32_t device, sfmx_matcher** out) {
    if (!out) return fail(SFMX_EINVAL, "null out");
    *out = nullptr;
    int rc = check_device(device);
    if (rc) return rc;
    auto* m = new (std::nothrow) sfmx_matcher();
    if (!m) return fail(SFMX_ENOMEM, "host allocation");
    m->device = device;
    *out = m;
    return SFMX_OK;
}

int sfmx_matcher_destroy(sfmx_matcher* m) {
    if (!m) return SFMX_OK;
    {
        DeviceGuard g(m->device);
        m->stage_prep.release();
        m->stage_run.release();
        m->stage_imgs.release();
        m->stage_flags.release();
        if (m->hflags) (void)hipHostFree(m->hflags);
        m->hflags = nullptr;
        DevBuf* bufs[] = {&m->raw, &m->desc8, &m->normv, &m->keyc, &m->keyc2, &m->desc6, &m->keyf, &m->ne, &m->qlist, &m->qcount, &m->porder, &m->work2, &m->work2_n, &m->f32, &m->flags, &m->tabs, &m->pairs_d, &m->scratch,
                          &m->work_d, &m->work32_d, &m->dense_idx, &m->dense_dist, &m->slow_list,
                          &m->counts, &m->keep, &m->offsets, &m->out, &m->qmask, &m->top2, &m->recs};
        for (DevBuf* b : bufs) b->release();
        for (auto& set : m->evr)
            for (auto& e : set) if (e) (void)hipEventDestroy(e);
        for (auto& e : m->ov_ev) if (e) (void)hipEventDestroy(e);
        for (auto& e : m->fix_ev) if (e) (void)hipEventDestroy(e);
        for (auto& e : m->bev) if (e) (void)hipEventDestroy(e);
        if (m->sx) (void)hipStreamDestroy(m->sx);
        if (m->sp) (void)hipStreamDestroy(m->sp);
    }
    delete m;
    return SFMX_OK;
}

int sfmx_matcher_set_images(sfmx_matcher* m, const sfmx_desc* imgs, int32_t n, int32_t norm, void* stream) {
    return set_images_impl(m, imgs, n, norm, (hipStream_t)stream, false);
}

int sfmx_matcher_set_images_device(sfmx_matcher* m, const sfmx_desc* imgs, int32_t n, int32_t norm, void* stream) {
    return set_images_impl(m, imgs, n, norm, (hipStream_t)stream, true);
}

int sfmx_matcher_run(sfmx_matcher* m, const int32_t* pairs, int32_t n_pairs, double ratio, int32_t distinct,
                     int32_t min_count, void* stream) {
    return run_impl(m, pairs, n_pairs, ratio, distinct, min_count, (hipStream_t)stream);
}

int sfmx_matcher_fetch(sfmx_matcher* m, sfmx_dmatch* out, int64_t cap, int64_t* required, int64_t* pair_offsets,
                       int32_t* keep, void* stream) {
    const int rc = fetch_impl(m, out, cap, required, pair_offsets, keep, (hipStream_t)stream);
    if (m && (rc == SFMX_EDEVICE || rc == SFMX_EINTERNAL)) m->scratch_clean = false;   // a stream error: a kernel may have stopped half-way
    return rc;
}

int sfmx_matcher_device_results(sfmx_matcher* m, const sfmx_dmatch** matches, const int64_t** pair_offsets,
                                const int32_t** keep) {
    if (!m) return fail(SFMX_EINVAL, "null matcher");
    if (!m->has_run) return fail(SFMX_ESTATE, "no results before run");
    {
        DeviceGuard g(m->device);
        { const int rc_ = resolve_flags(m, nullptr, true); if (rc_) return rc_; }
    }
    if (matches) *matches = m->out.as<const sfmx_dmatch>();
    if (pair_offsets) *pair_offsets = m->offsets.as<const int64_t>();
    if (keep) *keep = m->keep.as<const int32_t>();
    return SFMX_OK;
}

int sfmx_matcher_stats(sfmx_matcher* m, int64_t* slow_queries, int64_t* fp32_pairs, void* stream) {
    if (!m) return fail(SFMX_EINVAL, "null matcher");
    if (!m->has_run) return fail(SFMX_ESTATE, "no stats before run");
    DeviceGuard g(m->device);
    { const int rc_ = resolve_flags(m, (hipStream_t)stream, false); if (rc_) return rc_; }
    int32_t sc = 0, unsettled = 0;
    HIPCHK(hipMemcpyAsync(&sc, m->slow_count.p, sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipMemcpyAsync(&unsettled, m->unsettled.p, sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    if (const hipError_t e = hipStreamSynchronize((hipStream_t)stream); e != hipSuccess) {
        m->scratch_clean = false;   // a stream error: a kernel may have stopped half-way
        return fail(SFMX_EDEVICE, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    }
    if (unsettled) return fail(SFMX_EINTERNAL, std::to_string(unsettled) + " forwarded queries were not settled by pass 2");
    if (slow_queries) *slow_queries = sc;
    if (fp32_pairs) *fp32_pairs = m->fp32_pairs;
    return SFMX_OK;
}

#ifdef SFMX_DIAG
// Diagnostic build only (not part of the public interface): the last run's totals over the pairs of the
// screen's two counters, forwarded queries and those of them on the full-row route of the FP6 product
// path (0 on every other path, whose second counters stay zero).  Summed on the host.
int sfmx_diag_matcher_route_totals(sfmx_matcher* m, int64_t* forwarded, int64_t* full_route) {
    if (!m) return fail(SFMX_EINVAL, "null matcher");
    if (!m->has_run) return fail(SFMX_ESTATE, "no totals before run");
    DeviceGuard g(m->device);
    std::vector<int32_t> h((size_t)arena_words(m->n_pairs));
    HIPCHK(hipStreamSynchronize(m->run_stream));
    HIPCHK(hipMemcpy(h.data(), m->qcount.p, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost));
    int64_t a = 0, b = 0;
    for (int p = 0; p < m->n_pairs; ++p) { a += h[p]; b += h[arena_qcount2(m->n_pairs) + p]; }
    if (forwarded) *forwarded = a;
    if (full_route) *full_route = b;
    return SFMX_OK;
}
// Diagnostic build only: what the batched prep wrote for the padded rows of image `img` of an L2 matcher:
// desc6[rows_pad][24], keyf[rows_pad], ne[rows_pad][2], norm[rows_pad] and the image's imax[2]; any pointer
// may be null.  -> rows_pad, or a (negative) SFMX_E* code.
int sfmx_diag_matcher_prep_rows(sfmx_matcher* m, int img, uint32_t* desc6, float* keyf, int32_t* ne, int32_t* norm,
                                int32_t* imax) {
    if (!m) return fail(SFMX_EINVAL, "null matcher");
    if (m->norm != SFMX_NORM_L2 || img < 0 || img >= m->n_imgs) return fail(SFMX_EINVAL, "no such L2 image");
    DeviceGuard g(m->device);
    if (hipDeviceSynchronize() != hipSuccess) return fail(SFMX_EINTERNAL, "device synchronize failed");
    const ImgDev& d = m->imgs[img];
    const size_t n = (size_t)d.rows_pad;
    hipError_t e = hipSuccess;
    if (desc6 && e == hipSuccess)
        e = hipMemcpy(desc6, m->desc6.as<uint32_t>() + d.row0 * fp6::ROW_WORDS, n * fp6::ROW_BYTES, hipMemcpyDeviceToHost);
    if (keyf && e == hipSuccess) e = hipMemcpy(keyf, m->keyf.as<float>() + d.row0, n * 4, hipMemcpyDeviceToHost);
    if (ne && e == hipSuccess) e = hipMemcpy(ne, m->ne.as<int2>() + d.row0, n * sizeof(int2), hipMemcpyDeviceToHost);
    if (norm && e == hipSuccess) e = hipMemcpy(norm, m->normv.as<int32_t>() + d.row0, n * 4, hipMemcpyDeviceToHost);
    if (imax && e == hipSuccess) e = hipMemcpy(imax, m->imax.as<int32_t>() + 2 * img, 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(SFMX_EINTERNAL, hipGetErrorString(e));
    return d.rows_pad;
}
// Diagnostic build only: the int8 side of the same rows: desc8[rows_pad][128], keyc[rows_pad], keyc2[rows_pad]; any
// pointer may be null.  -> rows_pad, or a (negative) SFMX_E* code.
int sfmx_diag_matcher_prep_rows8(sfmx_matcher* m, int img, int8_t* desc8, int32_t* keyc, int32_t* keyc2) {
    if (!m) return fail(SFMX_EINVAL, "null matcher");
    if (m->norm != SFMX_NORM_L2 || img < 0 || img >= m->n_imgs) return fail(SFMX_EINVAL, "no such L2 image");
    DeviceGuard g(m->device);
    if (hipDeviceSynchronize() != hipSuccess) return fail(SFMX_EINTERNAL, "device synchronize failed");
    const ImgDev& d = m->imgs[img];
    const size_t n = (size_t)d.rows_pad;
    hipError_t e = hipSuccess;
    if (desc8 && e == hipSuccess)
        e = hipMemcpy(desc8, m->desc8.as<int8_t>() + d.row0 * SIFT_DIM, n * SIFT_DIM, hipMemcpyDeviceToHost);
    if (keyc && e == hipSuccess) e = hipMemcpy(keyc, m->keyc.as<int32_t>() + d.row0, n * 4, hipMemcpyDeviceToHost);
    if (keyc2 && e == hipSuccess) e = hipMemcpy(keyc2, m->keyc2.as<int32_t>() + d.row0, n * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(SFMX_EINTERNAL, hipGetErrorString(e));
    return d.rows_pad;
}
// Diagnostic build only: the f8f6f4 MFMA in both forms (fp6::mfma16 / mfma32, block-scaled with unit scales and
// unscaled) on the caller's operand fragments and C values, one wave per case, D of each form back to the host.
// shape 16: a, b [n][64][8] words, c, d [n][64][4] floats; shape 32 (the chained pair): a, b [n][2][64][8] words,
// c, d [n][64][16] floats.  fmt: 2 = e2m3, 4 = e2m1.
int sfmx_diag_mfma_forms(int device, int shape, int fmt, int n, const int32_t* a, const int32_t* b, const float* c,
                         float* d_scaled, float* d_unscaled) {
    if (n < 0 || (shape != 16 && shape != 32) || (fmt != 2 && fmt != 4) || !a || !b || !c || !d_scaled || !d_unscaled)
        return fail(SFMX_EINVAL, "mfma forms: shape 16 | 32, fmt 2 | 4, no null array");
    if (n == 0) return SFMX_OK;
    DeviceGuard g(device);
    const size_t ab = (size_t)n * (shape == 16 ? 1 : 2) * 64 * 8 * 4, cd = (size_t)n * 64 * (shape == 16 ? 4 : 16) * 4;
    DevBuf da, db, dc, ds, du;
    auto run = [&]() -> int {
        for (DevBuf* buf : {&da, &db})
            if (const int rc = buf->ensure(ab)) return rc;
        for (DevBuf* buf : {&dc, &ds, &du})
            if (const int rc = buf->ensure(cd)) return rc;
        HIPCHK(hipMemcpy(da.p, a, ab, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(db.p, b, ab, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dc.p, c, cd, hipMemcpyHostToDevice));
        HIPCHK(launch_mfma_forms(shape, fmt, n, da.as<int32_t>(), db.as<int32_t>(), dc.as<float>(), ds.as<float>(),
                                 du.as<float>(), nullptr));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(d_scaled, ds.p, cd, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(d_unscaled, du.p, cd, hipMemcpyDeviceToHost));
        return SFMX_OK;
    };
    const int rc = run();
    for (DevBuf* buf : {&da, &db, &dc, &ds, &du}) buf->release();
    return rc;
}
#endif

int sfmx_matcher_timing(sfmx_matcher* m, float* main_kernel_ms, float* total_ms) {
    if (!m) return fail(SFMX_EINVAL, "null matcher");
    if (!m->ev_recorded) return fail(SFMX_ESTATE, "no timing before run");
    DeviceGuard g(m->device);
    HIPCHK(hipEventSynchronize(m->ev[2]));
    float a = 0.f, b = 0.f;
    HIPCHK(hipEventElapsedTime(&a, m->ev[0], m->ev[1]));
    HIPCHK(hipEventElapsedTime(&b, m->ev[0], m->ev[2]));
    if (main_kernel_ms) *main_kernel_ms = a;
    if (total_ms) *total_ms = b;
    return SFMX_OK;
}

int sfmx_matcher_timing_history(sfmx_matcher* m, float* main_kernel_ms, float* screen_ms, int32_t n) {
    if (!m) return fail(SFMX_EINVAL, "null matcher");
    if (!m->ev_recorded) return fail(SFMX_ESTATE, "no timing before run");
    if (n < 0) return fail(SFMX_EINVAL, "negative count");
    DeviceGuard g(m->device);
    HIPCHK(hipEventSynchronize(m->ev[2]));
    const long long k = std::min<long long>({(long long)n, m->runs, (long long)sfmx_matcher::EV_RING});
    for (long long i = 0; i < k; ++i) {   // oldest first: runs (runs - k) .. (runs - 1)
        hipEvent_t* e = m->evr[(m->runs - k + i) % sfmx_matcher::EV_RING];
        float a = 0.f, b = 0.f;
        HIPCHK(hipEventElapsedTime(&a, e[0], e[1]));
        HIPCHK(hipEventElapsedTime(&b, e[0], e[3]));
        if (main_kernel_ms) main_kernel_ms[i] = a;
        if (screen_ms) screen_ms[i] = b;
    }
    return (int)k;
}

int sfmx_matcher_pass_timing(sfmx_matcher* m, float* screen_ms, float* pass2_ms) {
    if (!m) return fail(SFMX_EINVAL, "null matcher");
    if (!m->ev_recorded) return fail(SFMX_ESTATE, "no timing before run");
    DeviceGuard g(m->device);
    HIPCHK(hipEventSynchronize(m->ev[2]));
    float a = 0.f, b = 0.f;
    HIPCHK(hipEventElapsedTime(&a, m->ev[0], m->ev[3]));
    HIPCHK(hipEventElapsedTime(&b, m->ev[3], m->ev[1]));
    if (screen_ms) *screen_ms = a;
    if (pass2_ms) *pass2_ms = b;
    return SFMX_OK;
}

int sfmx_match_pairs(const sfmx_desc* imgs, int32_t n_imgs, const int32_t* pairs, int32_t n_pairs, int32_t norm,
                     double ratio, int32_t distinct, int32_t min_count, int32_t n_gpus, sfmx_dmatch* out,
                     int64_t cap, int64_t* required, int64_t* pair_offsets, int32_t* keep) {
    if (n_pairs < 0 || (n_pairs > 0 && !pairs)) return fail(SFMX_EINVAL, "bad pair list");
    int ndev = sfmx_device_count();
    if (ndev <= 0) return fail(SFMX_EDEVICE, "no gfx950 device");
    const int G = std::max(1, std::min<int>(n_gpus <= 0 ? ndev : n_gpus, ndev));
    // Split the pair list into G contiguous slices balanced by sum Nq*Nt.
    std::vector<double> cost(n_pairs);
    double tot = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const int L = pairs[2 * p], R = pairs[2 * p + 1];
        if (L < 0 || L >= n_imgs || R < 0 || R >= n_imgs) return fail(SFMX_EINVAL, "pair image index out of range");
        cost[p] = (double)imgs[L].rows * imgs[R].rows + 1.0;
        tot += cost[p];
    }
    std::vector<int> cut(G + 1, n_pairs);
    cut[0] = 0;
    {
        double acc = 0; int g = 1;
        for (int p = 0; p < n_pairs && g < G; ++p) {
            acc += cost[p];
            if (acc >= tot * g / G) cut[g++] = p + 1;
        }
    }
    struct Slice { std::vector<sfmx_dmatch> m; std::vector<int64_t> off; std::vector<int32_t> keep; int rc = 0; std::string err; };
    std::vector<Slice> sl(G);
    auto work = [&](int g) {
        Slice& s = sl[g];
        const int np = cut[g + 1] - cut[g];
        sfmx_matcher* m = nullptr;
        if ((s.rc = sfmx_matcher_create(g, &m))) { s.err = g_last_error; return; }
        hipStream_t st = nullptr;
        {
            DeviceGuard dg(g);
            if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { s.rc = SFMX_EDEVICE; s.err = "stream"; sfmx_matcher_destroy(m); return; }
        }
        s.off.assign(np + 1, 0); s.keep.assign(np, 0);
        // upload only the images this GPU's slice references (remapped to a dense local table)
        std::vector<int32_t> local_of(n_imgs, -1), lpairs(2 * (size_t)np);
        std::vector<sfmx_desc> limgs;
        for (int q = 0; q < 2 * np; ++q) {
            const int im = pairs[2 * cut[g] + q];
            if (local_of[im] < 0) { local_of[im] = (int32_t)limgs.size(); limgs.push_back(imgs[im]); }
            lpairs[q] = local_of[im];
        }
        int64_t req = 0;
        if (!(s.rc = sfmx_matcher_set_images(m, limgs.data(), (int32_t)limgs.size(), norm, st)) &&
            !(s.rc = sfmx_matcher_run(m, lpairs.data(), np, ratio, distinct, min_count, st)) &&
            !(s.rc = sfmx_matcher_fetch(m, nullptr, 0, &req, s.off.data(), s.keep.data(), st))) {
            s.m.resize(req);
            s.rc = sfmx_matcher_fetch(m, s.m.data(), req, &req, nullptr, nullptr, st);
        }
        if (s.rc) s.err = g_last_error;
        { DeviceGuard dg(g); (void)hipStreamDestroy(st); }
        sfmx_matcher_destroy(m);
    };
    if (G == 1) work(0);
    else {
        std::vector<std::thread> th;
        for (int g = 0; g < G; ++g) th.emplace_back(work, g);
        for (auto& t : th) t.join();
    }
    int64_t total = 0;
    for (int g = 0; g < G; ++g) {
        if (sl[g].rc) return fail(sl[g].rc, sl[g].err);
        total += (int64_t)sl[g].m.size();
    }
    if (required) *required = total;
    if (out && cap < total) return fail(SFMX_ECAPACITY, "output capacity too small");
    int64_t base = 0;
    for (int g = 0; g < G; ++g) {
        const int np = cut[g + 1] - cut[g];
        for (int p = 0; p < np; ++p) {
            if (pair_offsets) pair_offsets[cut[g] + p] = base + sl[g].off[p];
            if (keep) keep[cut[g] + p] = sl[g].keep[p];
        }
        if (out && !sl[g].m.empty()) std::memcpy(out + base, sl[g].m.data(), sizeof(sfmx_dmatch) * sl[g].m.size());
        base += (int64_t)sl[g].m.size();
    }
    if (pair_offsets) pair_offsets[n_pairs] = base;
    return SFMX_OK;
}

}  // extern "C"
