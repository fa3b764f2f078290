// SPDX-License-Identifier: MIT
// cv::projectPoints for one point, as tests/tri_ref.py's project() restates it, shared by the rows that
// reproject a float 3-D point into a posed shot: triangulate.hip (the keep rule of SfM::triangulateMatch) and
// report.hip (the reprojection error of SceneUtils.cpp:43-62).  Both compile this one text with
// -ffp-contract=off: every step is one correctly rounded IEEE operation in the written association.
// Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace sfmx {

// A NaN result leaves as the canonical quiet NaN: IEEE 754 leaves the sign and payload of a NaN open, and
// x86 and gfx950 produce different ones.  On the bit patterns: the compiler folds `v != v ? NaN : v` to v.
__device__ __forceinline__ float canon(float v) {
    const uint32_t b = __float_as_uint(v);
    return __uint_as_float((b & 0x7FFFFFFFu) > 0x7F800000u ? 0x7FC00000u : b);
}
__device__ __forceinline__ double canon(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return __longlong_as_double((long long)((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull ? 0x7FF8000000000000ull : b));
}

// The float pixel position of the float point (Xf, Yf, Zf) in a shot.  ShotT holds the 3x4 pose [R|t] row-major
// as P[12] and the camera as fx, fy, cx, cy, k1, k2, p1, p2, k3.  Rows are ((r0*X + r1*Y) + r2*Z) + t; a point on
// the camera plane (z == 0) is divided by 1.
template <class ShotT>
__device__ __forceinline__ void project_point(const ShotT* __restrict__ S, float Xf, float Yf, float Zf, float& u, float& v) {
    const double X = (double)Xf, Y = (double)Yf, Z = (double)Zf;
    double x = S->P[0] * X + S->P[1] * Y + S->P[2] * Z + S->P[3];
    double y = S->P[4] * X + S->P[5] * Y + S->P[6] * Z + S->P[7];
    double z = S->P[8] * X + S->P[9] * Y + S->P[10] * Z + S->P[11];
    z = z != 0 ? 1.0 / z : 1.0;
    x = x * z;
    y = y * z;
    const double r2 = x * x + y * y;
    const double r4 = r2 * r2;
    const double r6 = r4 * r2;
    const double a1 = 2.0 * x * y;
    const double a2 = r2 + 2.0 * x * x;
    const double a3 = r2 + 2.0 * y * y;
    const double cdist = 1.0 + S->k1 * r2 + S->k2 * r4 + S->k3 * r6;
    const double xd = x * cdist + S->p1 * a1 + S->p2 * a2;
    const double yd = y * cdist + S->p1 * a3 + S->p2 * a1;
    u = (float)(xd * S->fx + S->cx);
    v = (float)(yd * S->fy + S->cy);
}

}  // namespace sfmx
