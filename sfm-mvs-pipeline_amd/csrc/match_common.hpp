// SPDX-License-Identifier: MIT
// sfmx matcher — device data layout shared by the host driver and the kernels.
//
// HBM layout (one matcher context, one device):
//   SIFT (NORM_L2):  desc8[row][128]  int8   a' = a - 128   (exact: SIFT values are integers 0..255)
//                    norm [row]       int32  ||a'||^2        (<= 2^21)
//                    keyc [row]       int32  -(||a'||^2 << 8) + 255 - (row & 255)   (see match_device.hpp)
//                    desc6[row][96 B] e2m3   a = u - 32 quantised for the FP6 screen (sift_fp6.hpp: layout, bound)
//                    keyf [row]       float  -||a||^2 / 2048, the FP6 screen's C operand
//                    ne   [row]       int2   (||a||^2, ||e||^2), e the quantisation error; per-image maxima in imax
//                    f32  [row][128]  float  only when an image is not integer-valued (fp32 fallback)
//   ORB (NORM_HAMMING): desc8[row][32] uint8 (rows padded with zeros)
// Images are concatenated; each starts at a row offset that is a multiple of
// ROW_ALIGN and is padded to a multiple of ROW_ALIGN rows with zero rows
// (int8 0 == descriptor value 128: contributes 0 to every dot product).
#pragma once
#include <cstdint>
#include <string>

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

namespace sfmx {

constexpr int ROW_ALIGN = 512;       // = query rows per work item = 2 x key chunk (256)
constexpr int SIFT_DIM = 128;
constexpr int ORB_BYTES = 32;
// Queries whose best-2 squared distance reaches this value take the exact
// float-sqrt slow path: below it sqrtf is injective on integers (first
// collision is at s = 4,197,201), so ranking on the integer
// s equals ranking on sqrtf(s) bits.
constexpr int64_t SQRT_SAFE = 1 << 22;

// A run's zeroed arena of int32 (one fill): qcount[n_pairs] | the persistent screens' 8 XCD tickets |
// slow_count | unsettled | qcount2[n_pairs], the per-pair count of forwarded queries on the full-row route
// of the FP6 product path (sift_screen6_kernel).
constexpr int ARENA_FIXED = 8 + 2;
inline int arena_qcount2(int n_pairs) { return n_pairs + ARENA_FIXED; }
inline int arena_words(int n_pairs) { return 2 * n_pairs + ARENA_FIXED; }
// qmask of a forwarded query of the FP6 product path that is not certified for one subset: no subset bit
// (sift_subset_kernel does not gather it) and not two bits (sift_finish_kernel reads the slot's own two keys).
constexpr int32_t QMASK_FULL_ROUTE = 1 << 16;

// The matcher's last-arriver scratch, int32 words (matcher.cpp ensure_scratch; DESIGN 5 "last arriver"): tickets
// that are zero between kernels (zeroed when the buffer is allocated, set back to zero by the workgroup that reads
// the last value), and the prepare kernel's per-workgroup maxima, which are written before they are read.
//   [SCRATCH_FINISH]            sift_finish_kernel: workgroups done (the last one scans the counts)
//   [SCRATCH_PREP]              prep_l2_batch_kernel: images done (the last one publishes the flags)
//   [SCRATCH_IMG + i]           prep_l2_batch_kernel: workgroups of image i done, i < n_flags (a multiple of 64)
//   [SCRATCH_IMG + n_flags ..)  int2 (emax, amax) of workgroup (image, blockIdx.x): [n][grid x]
constexpr int SCRATCH_FINISH = 0, SCRATCH_PREP = 1, SCRATCH_IMG = 64;
inline int64_t scratch_words(int64_t n_flags, int64_t n, int64_t grid_x) { return SCRATCH_IMG + n_flags + 2 * n * grid_x; }

struct ImgDev {
    int32_t rows;       // real descriptor rows (Nq or Nt)
    int32_t rows_pad;   // multiple of ROW_ALIGN
    int64_t row0;       // first row in the pool
    int32_t integral;   // SIFT: 1 if all values are integers in [0,255]
    int32_t _pad;
};

struct PairDev {
    int32_t left, right;   // image indices: left = query, right = train
    int64_t dense_base;    // offset of this pair's per-query results (sum of previous Nq)
};

// One pair of a run as a flat record, in `porder` order (built by the host with the plan): what the
// list-path kernels would otherwise chain through porder -> pairs -> imgs (three dependent loads).
struct PairRec {
    int64_t lrow0, rrow0;  // first pool row of the left (query) / right (train) image
    int64_t dense_base;    // as PairDev
    int32_t nq, nt;        // real rows of the left / right image
    int32_t rows_pad;      // padded rows of the right image
    int32_t pair;          // index in the caller's pair list
    int32_t lists;         // 1: settled and assembled from the forwarded lists; 0: through the dense arrays
    int32_t _pad;
};

struct WorkItem {          // one 512-query block of one pair
    int32_t pair;
    int32_t q0;
};

struct DMatchDev { int32_t queryIdx, trainIdx, imgIdx; float distance; };

struct PrepImg {           // one image of a batched prep launch
    const float* src;
    int32_t rows, cols, rows_pad, _pad;
    int64_t row0;
};

// The route of one run: which kernels a run launches and where its results settle.  matcher.cpp resolves it
// once per run (resolve_route: constants in the product library, the SFMX_* switches of diag.hpp in the
// diagnostic one), keeps it in the run plan as the route part of the reuse key, and hands it to the
// launchers; nothing below run_impl reads a switch.  The default-constructed value is the product route.
struct MatchRoute {
    enum SiftScreen : int32_t {
        FP6_16,         // sift_screen6_kernel, 16 x 16 x 128 (product)
        FP6_32,         // sift_screen6w_kernel, 32 x 32 x 64 (SIFT_VARIANT_FP6_OTHER_SHAPE)
        INT8_16,        // sift_screen16_kernel, 16 x 16 x 64: 8 tiles x 4 waves, 64-row stages (106; the int8 routes' default)
        INT8_16_S128,   //   128-row stages (107)
        INT8_16_W8,     //   4 tiles x 8 waves (108)
        INT8_32,        // sift_screen_kernel, 32 x 32 x 32 (103)
        NO_SCREEN       // single pass (100, 30, 31)
    };
    enum SiftPass2 : int32_t {
        ROWS,           // sift_rows_kernel on the certified subset, full-row items for the rest (product)
        SUBSET_CERT,    // the same with sift_subset_kernel on the certified subset (SIFT_VARIANT_FP6_SUBSET_WG)
        FULL_ROWS,      // full-row items for every forwarded query (SIFT_VARIANT_FP6_FULL)
        SUBSET,         // sift_subset_kernel over the flagged subsets (SFMX_SIFT_P2 = 10 behind an int8 screen)
        GATHER,         // sift_knn2_kernel<GATHER> items of p2_qt x p2_waves x 32 queries into the dense arrays
        SINGLE,         // no pass 2: the r01d single-pass kernel (100)
        SINGLE_MINW1,   //   with one wave per SIMD (30)
        SINGLE_R01      //   the r01 tiling with one wave per SIMD (31)
    };
    enum OrbForm : int32_t {
        ORB_SUBSET,        // orb_screen16_kernel + orb_subset_kernel + orb_settle_kernel (product)
        ORB_VALU,          // orb_knn2_kernel on 32-byte rows (1): the other row layout, fixed by set_images
        ORB_SINGLE_32_W16, // orb_mfma_kernel<1, 16, 1, 128> (4)
        ORB_SINGLE_16,     // orb_mfma16_kernel<8, 4, 2, 64> (5)
        ORB_SINGLE_16_W8,  // orb_mfma16_kernel<4, 8, 2, 64> (7)
        ORB_SINGLE_32_MINW1, // orb_mfma_kernel<4, 4, 1, 64> (9)
        ORB_GATHER_512,    // orb_screen16_kernel + orb_mfma16_kernel<GATHER>, 512-query items (12)
        ORB_GATHER_128,    //   128-query items (13)
        ORB_GATHER_256     //   256-query items (14)
    };
    SiftScreen screen = FP6_16;
    SiftPass2 pass2 = ROWS;
    int32_t p2_qt = 1, p2_waves = 4;   // pass-2 item: p2_qt x p2_waves x 32 queries (GATHER: 128, 256 or 512; the full-row items: 128)
    bool sift_lists = true;            // SIFT pairs settle and assemble from the forwarded lists; else from the dense arrays
    int32_t block_queries = ROW_ALIGN; // queries per work item
    OrbForm orb = ORB_SUBSET;
    // 1 = one screen launch, then pass 2.  The overlapped form (8 batches, screens on two streams, pass 2 on a
    // third) measured slower on C2 in r04a (launch span 6.94 vs 6.20 ms: concurrent screens and subset kernels
    // contend for the CUs; the subset dispatches stretch to 0.67 ms each, profiles/r04a_c2_span.txt); kept
    // selectable (SFMX_MATCH_BATCHES) and tested in the diagnostic build.
    int32_t batches = 1;
    bool persist = false;              // ticket-fed persistent screens (SFMX_SCREEN_PERSIST)
    int32_t full_row_grid = 0;         // grid of the product path's full-row launch; 0 = two resident rounds (SFMX_FULL_ROW_GRID)

    bool operator==(const MatchRoute& o) const {
        return screen == o.screen && pass2 == o.pass2 && p2_qt == o.p2_qt && p2_waves == o.p2_waves &&
               sift_lists == o.sift_lists && block_queries == o.block_queries && orb == o.orb && batches == o.batches &&
               persist == o.persist && full_row_grid == o.full_row_grid;
    }
    bool operator!=(const MatchRoute& o) const { return !(*this == o); }
    // the launch sequences of launch_sift_product / launch_orb_product (the full-row grid is an argument of the former)
    bool sift_product() const { return screen == FP6_16 && pass2 == ROWS && sift_lists; }
    bool orb_product() const { return orb == ORB_SUBSET && batches == 1 && !persist; }
};

// The device pointers of one run, filled once per run by run_impl from the matcher's buffers.
struct MatchBufs {
    const WorkItem* work;          // the run's work items (integer pairs), n_work of them
    const WorkItem* work32;        // those of the fp32-fallback pairs
    const PairDev* pairs;
    const ImgDev* imgs;
    const int32_t* porder;         // pairs ordered by train image
    const PairRec* recs;           // list path: one record per pair, in porder order
    const int8_t* desc8;           // SIFT int8 rows; ORB rows (FP4 +-1 rows, or 32-byte rows for ORB_VALU)
    const int32_t* norm;
    const int32_t* keyc;
    const int32_t* keyc2;
    const uint32_t* desc6;         // FP6 screen operands (sift_fp6.hpp)
    const float* keyf;
    const int2* ne;
    const int32_t* imax;
    const float* f32;              // fp32 rows (only with a non-integral image)
    int32_t* qlist;                // per pair at dense_base: the forwarded queries
    int32_t* qcount;               // the run's zeroed arena (ARENA_FIXED above): qcount | tickets | ... | qcount2
    int32_t* qmask;
    unsigned long long* top2;
    unsigned long long* slot1;     // the packed output buffer, idle until assembly: second top-2 slot / second list
    WorkItem* work2;               // compacted pass-2 items (up to 4 per work item) and their count
    int32_t* work2_n;
    int32_t* dense_idx;            // dense per-query results
    float* dense_dist;
    int2* slow_list;
    int32_t* slow_count;
    int32_t* unsettled;
    int64_t* counts;               // assembly: per-pair counts, keep flags, offsets, packed matches
    int32_t* keep;
    int64_t* offsets;
    DMatchDev* out;
    int32_t* scratch;              // the last-arriver tickets (SCRATCH_* above)
};

// Launchers of match_kernels.hip (both libraries).
struct FlagHandoff {               // where the prepare kernel's last workgroup publishes the integrality flags
    int32_t* dst;                  // host-coherent: one word per image
    unsigned* seq;                 // host-coherent sequence word, release-stored behind the flags
    unsigned value;                // the value the host waits for
};
int prep_l2_grid_x(int max_rows_pad);
hipError_t launch_prep_l2_batch(const PrepImg*, int, int, int8_t*, int32_t*, int32_t*, int32_t*, int32_t*, uint32_t*, float*,
                                int2*, int32_t*, int32_t* scratch, int n_flags, const FlagHandoff&, hipStream_t);
hipError_t launch_prep_f32(const float*, int, int, int, float*, hipStream_t);
hipError_t launch_prep_hamming_fp4(const uint8_t*, int, int, int, uint8_t*, int32_t*, hipStream_t);
hipError_t launch_selftest_sqrt(int64_t, uint32_t*, hipStream_t);
hipError_t launch_sift_product(const MatchBufs& b, int n_work, int n_pairs, double ratio, int full_row_grid, hipStream_t st,
                               hipEvent_t ev_screen);
hipError_t launch_sift_full_rows(const MatchBufs& b, int n_work, int n_pairs, double ratio, int full_row_grid, hipStream_t st,
                                 bool compact = true);
hipError_t launch_orb_product(const MatchBufs& b, int n_work, int n_pairs, double ratio, hipStream_t st, hipEvent_t ev_screen);
hipError_t launch_orb_pass2(const MatchBufs& b, const int32_t* porder, int np, const int32_t* settle_order, double ratio,
                            hipStream_t st);
hipError_t launch_sift_f32(const MatchBufs& b, int n_work32, double ratio, hipStream_t st);
hipError_t launch_assemble(const MatchBufs& b, int n_pairs, int distinct, int min_count, int max_nt, hipStream_t st);
hipError_t launch_finish_lists(const MatchBufs& b, int n_pairs, double ratio, int distinct, int min_count, int max_nq,
                               int max_nt, hipStream_t st, hipEvent_t ev_main);

// Overlapped two-pass matching (a route of more than one batch; match_diag.hip launch_two_pass_overlap): a
// batch of the work list, and the matcher's extra streams / events.
struct MatchBatch { int32_t w0, nw, p0, np; };   // work items [w0, w0 + nw), pair-order slots [p0, p0 + np)
struct OverlapStreams {
    hipStream_t sx, sp;                          // second screen stream, pass-2 stream
    hipEvent_t start, sx_done, sp_done;          // after the qcount clear; the two joins
    hipEvent_t* screen;                          // one per batch
};
#ifdef SFMX_DIAG
// Launchers of match_diag.hip (diagnostic library only).  The two dispatchers run any route; for the product
// route they call launch_sift_product / launch_orb_product.
hipError_t launch_sift_diag(const MatchRoute& r, const MatchBufs& b, int n_work, int n_pairs, double ratio, hipStream_t st,
                            hipEvent_t ev_screen);
hipError_t launch_orb_diag(const MatchRoute& r, const MatchBufs& b, int n_work, int n_pairs, double ratio, hipStream_t st,
                           hipEvent_t ev_screen);
hipError_t launch_two_pass_overlap(bool sift, const MatchBatch* batches, int nb, const MatchBufs& b, int n_pairs, double ratio,
                                   hipStream_t st, hipEvent_t ev_screen, const OverlapStreams& os);
hipError_t launch_sift_slow(const MatchBufs& b, double ratio, hipStream_t st);
hipError_t launch_prep_hamming(const uint8_t*, int, int, int, uint8_t*, hipStream_t);
hipError_t launch_mfma_forms(int, int, int, const int32_t*, const int32_t*, const float*, float*, float*, hipStream_t);
#endif

// Thread-local last-error text shared by every C-ABI entry point (sfmx_last_error).
void set_last_error(const char* msg);

}  // namespace sfmx
