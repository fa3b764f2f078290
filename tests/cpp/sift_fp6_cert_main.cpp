// SPDX-License-Identifier: MIT
// Host driver of fp6::certified (csrc/sift_fp6.hpp) for tests/test_sift_fp6_cert.py (its own main;
// g++ -O2 -ffp-contract=off).
//
//   sift_fp6_cert_main <in.bin> <out.bin>
// in:  int32 n; n records of (float k1, float k2, int32 r1, int32 nt, int32 na, int32 e2q, int32 emax2,
//      int32 amax2, double ratio)
// out: int32 certified[n]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../sfm-mvs-pipeline_amd/csrc/sift_fp6.hpp"

using namespace sfmx;

#pragma pack(push, 1)
struct Rec { float k1, k2; int32_t r1, nt, na, e2q, emax2, amax2; double ratio; };
#pragma pack(pop)
static_assert(sizeof(Rec) == 40, "record layout");

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t n = 0;
    if (std::fread(&n, 4, 1, f) != 1 || n < 0) return 4;
    std::vector<Rec> rec((size_t)n);
    if (std::fread(rec.data(), sizeof(Rec), rec.size(), f) != rec.size()) return 4;
    std::fclose(f);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 5;
    for (const Rec& d : rec) {
        const int32_t c = fp6::certified(d.k1, d.k2, d.r1, d.nt, d.na, d.e2q, d.emax2, d.amax2, d.ratio);
        std::fwrite(&c, 4, 1, o);
    }
    std::fclose(o);
    return 0;
}
