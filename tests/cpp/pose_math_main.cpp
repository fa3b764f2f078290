// SPDX-License-Identifier: MIT
// Stand-alone host driver of csrc/pose_math.hpp for tests/test_pose_math_host.py: reads samples, runs the
// five-point solver, the Sampson error, the pose candidates and the cheirality test, writes every result as
// doubles.  Build: g++ -O2 -std=c++17 -ffp-contract=off pose_math_main.cpp -o pose_math_main
//   input : int32 n5, ns, nd, nc; then n5 x 20, ns x 13 (E, x1 y1 x2 y2), nd x 9, nc x 16 (P1, x1 y1 x2 y2) doubles
//   output: n5 x 91 (count, 10 models), ns (float error), nd x 48, nc (0 / 1) doubles
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../sfm-mvs-pipeline_amd/csrc/pose_math.hpp"

using namespace sfmx::posem;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    int32_t cnt[4];
    if (std::fread(cnt, sizeof(int32_t), 4, in) != 4) return 4;
    const size_t n_in = (size_t)cnt[0] * 20 + (size_t)cnt[1] * 13 + (size_t)cnt[2] * 9 + (size_t)cnt[3] * 16;
    std::vector<double> d(n_in);
    if (n_in && std::fread(d.data(), sizeof(double), n_in, in) != n_in) return 4;
    std::fclose(in);
    std::vector<double> out;
    const double* p = d.data();
    for (int i = 0; i < cnt[0]; ++i, p += 20) {
        double q[5][4], w[PM_WS];
        for (int r = 0; r < 5; ++r)
            for (int c = 0; c < 4; ++c) q[r][c] = p[4 * r + c];
        const int nm = five_point(q, w, 1);
        out.push_back((double)nm);
        for (int e = 0; e < 90; ++e) out.push_back(e < 9 * nm ? w[PM_MODELS + e] : 0.0);
    }
    for (int i = 0; i < cnt[1]; ++i, p += 13) out.push_back((double)sampson_error(p, p[9], p[10], p[11], p[12]));
    for (int i = 0; i < cnt[2]; ++i, p += 9) {
        double cand[4][12];
        pose_candidates(p, cand);
        for (int c = 0; c < 4; ++c)
            for (int e = 0; e < 12; ++e) out.push_back(cand[c][e]);
    }
    for (int i = 0; i < cnt[3]; ++i, p += 16) out.push_back(cheirality(p, p[12], p[13], p[14], p[15]) ? 1.0 : 0.0);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 5;
    if (!out.empty() && std::fwrite(out.data(), sizeof(double), out.size(), o) != out.size()) return 6;
    std::fclose(o);
    return 0;
}
