// SPDX-License-Identifier: MIT
// Host driver of csrc/sift_fp6.hpp for tests/test_sift_fp6_bound.py (its own main; g++ -O2 -ffp-contract=off).
//
//   sift_fp6_main <in.bin> <out.bin>
// in:  int32 n_rows, n_dec; uint8 rows[n_rows][128];
//      n_dec records of (float k1, float k2, int32 na, int32 e2q, int32 emax2, int32 amax2, double ratio)
// out: per row int32 m[128], uint32 packed[24], int32 a2, e2; then int32 rejected[n_dec];
//      then the 64 code -> m values and the swizzles of rows 0..15 (swz_a, swz_b).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sfm-mvs-pipeline_amd/csrc/sift_fp6.hpp"

using namespace sfmx;

#pragma pack(push, 1)
struct Dec { float k1, k2; int32_t na, e2q, emax2, amax2; double ratio; };
#pragma pack(pop)
static_assert(sizeof(Dec) == 32, "record layout");

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[2];
    if (std::fread(hdr, 4, 2, f) != 2) return 4;
    std::vector<uint8_t> rows((size_t)hdr[0] * 128);
    std::vector<Dec> dec(hdr[1]);
    if (std::fread(rows.data(), 1, rows.size(), f) != rows.size()) return 4;
    if (std::fread(dec.data(), sizeof(Dec), dec.size(), f) != dec.size()) return 4;
    std::fclose(f);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 5;
    for (int r = 0; r < hdr[0]; ++r) {
        int32_t m[128], sums[2] = {0, 0};
        unsigned codes[128];
        uint32_t packed[fp6::ROW_WORDS];
        for (int k = 0; k < 128; ++k) {
            const int a = (int)rows[(size_t)r * 128 + k] - fp6::OFFSET;
            m[k] = fp6::quant_m(a);
            codes[k] = fp6::code_of_m(m[k]);
            const int e = a - fp6::SCALE * m[k];
            sums[0] += a * a;
            sums[1] += e * e;
        }
        fp6::pack_row(codes, packed);
        std::fwrite(m, 4, 128, o);
        std::fwrite(packed, 4, fp6::ROW_WORDS, o);
        std::fwrite(sums, 4, 2, o);
    }
    for (const Dec& d : dec) {
        const int32_t rej = fp6::certainly_rejected(d.k1, d.k2, d.na, d.e2q, d.emax2, d.amax2, d.ratio);
        std::fwrite(&rej, 4, 1, o);
    }
    for (unsigned c = 0; c < 64; ++c) {
        const int32_t m = fp6::m_of_code(c);
        std::fwrite(&m, 4, 1, o);
    }
    for (int r = 0; r < 16; ++r) {
        const int32_t s[2] = {fp6::swz_a(r), fp6::swz_b(r)};
        std::fwrite(s, 4, 2, o);
    }
    std::fclose(o);
    return 0;
}
