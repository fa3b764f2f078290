// SPDX-License-Identifier: MIT
// Host driver of the 32 x 32 x 64 maps of csrc/sift_fp6.hpp for tests/test_sift_fp6_screen32.py (its own main).
//
//   sift_fp6_screen32_main      prints one record per line:
//     frag m h f          fragment of MFMA m for K-half h
//     accrow i h row      train row (of the 32-row block) of accumulator register i
//     chain c h subset    row subset (j mod 16) of chain c
//     a row f off         byte offset of the plane-A read of fragment f of stage row `row` (stage of 128 rows)
//     b row f off         ... of the plane-B read
//     key row0 k h off    ... of the 16-B key read of registers 4 k .. 4 k + 3 for the row block at row0
#include <cstdio>

#include "../../sfm-mvs-pipeline_amd/csrc/sift_fp6.hpp"

using namespace sfmx;

int main() {
    constexpr int STAGE = 128;
    for (int m = 0; m < 2; ++m)
        for (int h = 0; h < 2; ++h) std::printf("frag %d %d %d\n", m, h, fp6::frag32(m, h));
    for (int i = 0; i < 16; ++i)
        for (int h = 0; h < 2; ++h) std::printf("accrow %d %d %d\n", i, h, fp6::acc_row32(i, h));
    for (int c = 0; c < 8; ++c)
        for (int h = 0; h < 2; ++h) std::printf("chain %d %d %d\n", c, h, fp6::chain_subset32(c, h));
    for (int row = 0; row < STAGE; ++row)
        for (int f = 0; f < 4; ++f) {
            std::printf("a %d %d %d\n", row, f, fp6::lds_a32(row, f));
            std::printf("b %d %d %d\n", row, f, fp6::lds_b32(STAGE, row, f));
        }
    for (int row0 = 0; row0 < STAGE; row0 += 32)
        for (int k = 0; k < 4; ++k)
            for (int h = 0; h < 2; ++h) std::printf("key %d %d %d %d\n", row0, k, h, fp6::lds_key32(STAGE, row0, k, h));
    return 0;
}
