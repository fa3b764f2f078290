// SPDX-License-Identifier: MIT
// Stand-alone driver of csrc/device_call.hpp's BlockLayout for tests/test_device_call_san.py (built with the host
// sanitizers; no device, no HIP).  Every request list is laid out over a malloc'ed block of exactly `need` bytes
// and checked against the size list that the entry points kept by hand before the header existed (ref256 below
// restates their r256): need, every offset, null pointers of the parts not needed, 256-byte alignment relative
// to the base, parts disjoint and inside the block.  Every byte of every part is written, so an overlap or an
// overrun is also an AddressSanitizer report.  Prints "ok <cases>" and exits 0, or names the first failure.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sfm-mvs-pipeline_amd/csrc/device_call.hpp"

static size_t ref256(size_t b) { return ((b > 1 ? b : 1) + 255) & ~(size_t)255; }

struct alignas(16) E16 { unsigned char b[16]; };          // float4 / sfmx_dmatch
struct E88 { double d[11]; };                             // ShotP: CamP (9 doubles), a pointer, two int32
struct E200 { double d[25]; };                            // ShotT: 12 + 11 doubles, a pointer, two int32
static_assert(sizeof(E16) == 16 && sizeof(E88) == 88 && sizeof(E200) == 200, "element sizes");

struct Req { size_t esize, count; bool needed; };

static int g_cases = 0;

template <class T> static void want_as(sfmx::BlockLayout& L, void*& slot, const Req& r) {
    L.want(reinterpret_cast<T*&>(slot), r.count, r.needed);
}

// lays `reqs` out, checks it against the hand-kept list, writes and reads back every byte; `expect_need`: the sum
// written out from literal counts (0: only the per-part sum is checked)
static bool run(const char* name, const std::vector<Req>& reqs, size_t expect_need) {
    ++g_cases;
    sfmx::BlockLayout L;
    std::vector<void*> ptr(reqs.size(), reinterpret_cast<void*>(1));   // want() must clear them
    size_t sum = 0;
    for (size_t i = 0; i < reqs.size(); ++i) {
        const Req& r = reqs[i];
        switch (r.esize) {
            case 1: want_as<uint8_t>(L, ptr[i], r); break;
            case 4: want_as<uint32_t>(L, ptr[i], r); break;
            case 8: want_as<uint64_t>(L, ptr[i], r); break;
            case 16: want_as<E16>(L, ptr[i], r); break;
            case 88: want_as<E88>(L, ptr[i], r); break;
            case 200: want_as<E200>(L, ptr[i], r); break;
            default: std::printf("%s: no element type of %zu bytes\n", name, r.esize); return false;
        }
        if (ptr[i] != nullptr) { std::printf("%s: part %zu not cleared by want()\n", name, i); return false; }
        sum += r.needed ? ref256(r.esize * r.count) : 0;
        if (L.need != sum) { std::printf("%s: need %zu after part %zu, the size list gives %zu\n", name, L.need, i, sum); return false; }
    }
    if (expect_need && L.need != expect_need) { std::printf("%s: need %zu, expected %zu\n", name, L.need, expect_need); return false; }
    char* base = static_cast<char*>(std::malloc(L.need ? L.need : 1));
    if (!base) return false;
    L.commit(base);
    bool ok = true;
    size_t off = 0;
    for (size_t i = 0; i < reqs.size() && ok; ++i) {
        const Req& r = reqs[i];
        char* p = static_cast<char*>(ptr[i]);
        if (!r.needed) {
            if (p) { std::printf("%s: part %zu is not needed but not null\n", name, i); ok = false; }
            continue;
        }
        const size_t bytes = r.esize * r.count;
        if (p != base + off) { std::printf("%s: part %zu at %td, the size list gives %zu\n", name, i, p - base, off); ok = false; break; }
        if ((p - base) % 256 != 0 || off + bytes > L.need) { std::printf("%s: part %zu misaligned or outside the block\n", name, i); ok = false; break; }
        std::memset(p, (int)(i + 1), bytes);
        off += ref256(bytes);
    }
    if (ok && off != L.need) { std::printf("%s: parts end at %zu, need %zu\n", name, off, L.need); ok = false; }
    for (size_t i = 0; i < reqs.size() && ok; ++i) {   // no later part wrote into an earlier one
        if (!reqs[i].needed) continue;
        const unsigned char* p = static_cast<const unsigned char*>(ptr[i]);
        for (size_t b = 0; b < reqs[i].esize * reqs[i].count; ++b)
            if (p[b] != (unsigned char)(i + 1)) { std::printf("%s: part %zu overwritten at byte %zu\n", name, i, b); ok = false; break; }
    }
    std::free(base);
    return ok;
}

// sfmx_triangulate_matches: tables | block counts, offsets, keep masks | two float4 scratches | host staging
static std::vector<Req> triangulate_list(size_t n_shots, size_t n_pairs, size_t n, size_t nk, bool H, bool err) {
    const size_t nb = (n + 255) / 256;
    return {{200, n_shots, true}, {4, 2 * n_pairs, true}, {8, 2, true}, {4, nb, true}, {8, nb, true}, {8, nb * 4, true},
            {16, n, true}, {16, n, true}, {8, nk, H}, {16, n, H}, {8, n_pairs + 1, H}, {8, n_pairs + 1, H}, {8, 3 * n, H},
            {8, n, H}, {4, 2 * n, H}, {8, 4 * n, H}, {8, 2 * n, H && err}};
}

// sfmx_relative_poses: tables | scratch (only with a list over CAP) | candidate bits | host staging
static std::vector<Req> pose_list(size_t n_shots, size_t n_pairs, size_t n, size_t nk, bool H, bool scratch) {
    return {{88, n_shots, true}, {16, n_pairs, true}, {8, 2, true}, {8, 4 * n, scratch}, {1, n, true}, {8, nk, H}, {16, n, H},
            {8, n_pairs + 1, H}, {4, n_pairs, H}, {8, 9 * n_pairs, H}, {8, 12 * n_pairs, H}, {1, n, H}, {4, n_pairs, H},
            {4, n_pairs, H}, {16, n, H}, {8, n_pairs + 1, H}};
}

int main() {
    bool ok = true;
    // parts of 0, 1, 255, 256 and 257 bytes: an empty part still takes 256
    ok = ok && run("bytes", {{1, 0, true}, {1, 1, true}, {1, 255, true}, {1, 256, true}, {1, 257, true}}, 256 + 256 + 256 + 256 + 512);
    // a part that is not needed between two that are: null, no bytes, the neighbours adjacent
    ok = ok && run("disabled", {{4, 10, true}, {8, 1000, false}, {4, 10, true}}, 512);
    ok = ok && run("disabled-first-last", {{8, 3, false}, {1, 300, true}, {16, 5, false}}, 512);
    ok = ok && run("all-disabled", {{8, 3, false}, {4, 0, false}}, 0);
    ok = ok && run("nothing", {}, 0);
    // element types of 1, 4, 8 and 16 bytes, counts that are no multiple of anything
    ok = ok && run("types", {{1, 77, true}, {4, 65, true}, {8, 33, true}, {16, 17, true}, {16, 16, true}, {4, 0, true}},
                   256 + 512 + 512 + 512 + 256 + 256);
    // 5 shots, 3 pairs, 1000 matches (4 blocks), 7000 keypoints, as the entry point's size list gave them:
    // tables 1024 + 256 + 256 | block parts 3 * 256 | scratch 2 * 16128 = 34560; host staging 56064 + 16128 + 256 +
    // 256 + 24064 + 8192 + 8192 + 32000 = 145152, and 16128 more with out_err
    ok = ok && run("triangulate-device", triangulate_list(5, 3, 1000, 0, false, true), 34560);
    ok = ok && run("triangulate-host", triangulate_list(5, 3, 1000, 7000, true, false), 34560 + 145152);
    ok = ok && run("triangulate-host-err", triangulate_list(5, 3, 1000, 7000, true, true), 34560 + 145152 + 16128);
    // the same counts for the pose: tables 512 + 256 + 256 | bits 1024 = 2048, scratch 32000; host staging 56064 +
    // 16128 + 256 + 256 + 256 + 512 + 1024 + 256 + 256 + 16128 + 256 = 91392
    ok = ok && run("pose-device", pose_list(5, 3, 1000, 0, false, false), 2048);
    ok = ok && run("pose-device-scratch", pose_list(5, 3, 1000, 0, false, true), 2048 + 32000);
    ok = ok && run("pose-host", pose_list(5, 3, 1000, 7000, true, false), 2048 + 91392);
    ok = ok && run("pose-host-scratch", pose_list(5, 3, 1000, 7000, true, true), 2048 + 32000 + 91392);
    if (!ok) return 1;
    std::printf("ok %d\n", g_cases);
    return 0;
}
