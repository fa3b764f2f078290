// SPDX-License-Identifier: MIT
// The arithmetic of sfmx_relative_poses (SfM::findCameraPoseFromMatch, sfm/SfM.cpp:491-540), host and device:
// the five-point solver, the Sampson error, decomposeEssentialMat and recoverPose's cheirality test, operation
// by operation in the order of tests/pose_ref.py.  One correctly rounded IEEE + - * / sqrt per
// step: every translation unit that includes this header is compiled with -ffp-contract=off, and nothing here
// calls libm but sqrt and fabs.
//
// The solver works in a caller-provided workspace of PM_WS doubles that it addresses as w[i * s]: s = 1 on the
// host, s = the batch size in the kernel, where w points into LDS at the lane's own column (element-major, so
// the lanes of a wave touch consecutive banks).  Nothing in it is an array in registers, so nothing can spill.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PM_HD __host__ __device__ inline
#define PM_UNROLL _Pragma("unroll")       // the register arrays below are indexed statically only when unrolled
#define PM_UNROLL1 _Pragma("unroll 1")
#else
#define PM_HD inline
#define PM_UNROLL
#define PM_UNROLL1
#endif

namespace sfmx {
namespace posem {

constexpr int PM_WS = 316;         // doubles of workspace per sample
constexpr int PM_A = 0;            // 10 x 20 constraint matrix; before it the 5 x 9 epipolar system; after it:
constexpr int PM_DP = 0;           //   the derivatives dp[d] (d = 1..10) at d (d + 1) / 2 - 1
constexpr int PM_R0 = 70;          //   root lists of two consecutive levels
constexpr int PM_R1 = 80;
constexpr int PM_MODELS = 100;     //   the models, 9 doubles each (at most 10)
constexpr int PM_N = 200;          // null-space basis X, Y, Z, W (4 x 9)
constexpr int PM_T = 236;          // E E^T (6 x 10), its trace (10), a minor (10); after the reduction:
constexpr int PM_B = 236;          //   B(z): row r at 13 r: bx[4], by[4], bc[5]
constexpr int PM_P1 = PM_B + 39;   //   2 x 2 minors of B (8, 8, 7 coefficients)
constexpr int PM_P2 = PM_P1 + 8;
constexpr int PM_P3 = PM_P2 + 8;
constexpr int PM_C = PM_P3 + 7;    //   det B(z), 11 coefficients
constexpr int MAX_HALVINGS = 128;
constexpr int SVD_SWEEPS = 30;

#define PW(i) w[(i) * s]

// products of the monomials of tests/pose_ref.py (M1 x M1 -> M2, M2 x M1 -> M3), packed 4 / 5 bits per entry
PM_HD int mul11(int i, int j) { return (int)((0x9876825475136430ull >> (4 * (4 * i + j))) & 15ull); }
PM_HD int mul21(int i, int j) {
    const unsigned long long t = j == 0 ? 0x18b4950412860ull : j == 1 ? 0x1ee3a4c81b422ull : j == 2 ? 0x25172daa440c4ull : 0x2727b1cb4c4e5ull;
    return (int)((t >> (5 * i)) & 31ull);
}

PM_HD bool finite_d(double v) { return fabs(v) < HUGE_VAL; }   // false for a NaN

// out (10) +-= a (4, stride sa) * b (4, stride sb): all three in the workspace
PM_HD void pmul11(double* w, int s, int out, int a, int sa, int b, int sb, bool sub) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const int k = out + mul11(i, j);
            const double v = PW(a + i * sa) * PW(b + j * sb);
            PW(k) = sub ? PW(k) - v : PW(k) + v;
        }
}
// out (20) +-= a (10) * b (4, stride sb)
PM_HD void pmul21(double* w, int s, int out, int a, int b, int sb, bool sub) {
    for (int i = 0; i < 10; ++i)
        for (int j = 0; j < 4; ++j) {
            const int k = out + mul21(i, j);
            const double v = PW(a + i) * PW(b + j * sb);
            PW(k) = sub ? PW(k) - v : PW(k) + v;
        }
}
// out[i + j] +-= a[i] * b[j]
PM_HD void pconv(double* w, int s, int out, int a, int na, int b, int nb, bool sub) {
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j) {
            const double v = PW(a + i) * PW(b + j);
            PW(out + i + j) = sub ? PW(out + i + j) - v : PW(out + i + j) + v;
        }
}
PM_HD double phorner(const double* w, int s, int c, int d, double z) {
    double v = PW(c + d);
    for (int i = d - 1; i >= 0; --i) v = v * z + PW(c + i);
    return v;
}

// EMEstimatorCallback::runKernel on 5 correspondences q[i] = (x1, y1, x2, y2): the number of models (0..10);
// model m is w[(PM_MODELS + 9 m + e) * s], row-major with unit Frobenius norm, in ascending order of the root z.
PM_HD int five_point(const double (&q)[5][4], double* w, int s) {
    // ---- the null space of the 5 x 9 epipolar system: Gauss-Jordan elimination, complete pivoting
PM_UNROLL
    for (int r = 0; r < 5; ++r) {
        const double x1 = q[r][0], y1 = q[r][1], x2 = q[r][2], y2 = q[r][3];
        PW(9 * r + 0) = x2 * x1; PW(9 * r + 1) = x2 * y1; PW(9 * r + 2) = x2;
        PW(9 * r + 3) = y2 * x1; PW(9 * r + 4) = y2 * y1; PW(9 * r + 5) = y2;
        PW(9 * r + 6) = x1;      PW(9 * r + 7) = y1;      PW(9 * r + 8) = 1.0;
    }
    unsigned long long perm = 0x876543210ull;   // column permutation, 4 bits per entry
    for (int k = 0; k < 5; ++k) {
        double best = 0.0;
        int pr = -1, pc = -1;
        for (int r = k; r < 5; ++r)
            for (int c = k; c < 9; ++c) {
                const double v = fabs(PW(9 * r + c));
                if (v > best) { best = v; pr = r; pc = c; }   // strict: the first largest wins, a NaN never does
            }
        if (!(best > 0.0)) return 0;
        for (int c = 0; c < 9; ++c) { const double t = PW(9 * k + c); PW(9 * k + c) = PW(9 * pr + c); PW(9 * pr + c) = t; }
        for (int r = 0; r < 5; ++r) { const double t = PW(9 * r + k); PW(9 * r + k) = PW(9 * r + pc); PW(9 * r + pc) = t; }
        {
            const unsigned long long a = (perm >> (4 * k)) & 15ull, b = (perm >> (4 * pc)) & 15ull;
            perm &= ~((15ull << (4 * k)) | (15ull << (4 * pc)));
            perm |= (b << (4 * k));
            perm |= (a << (4 * pc));   // (k == pc: a == b, both writes restore the entry)
        }
        const double p = PW(9 * k + k);
        for (int c = k + 1; c < 9; ++c) PW(9 * k + c) = PW(9 * k + c) / p;
        for (int r = 0; r < 5; ++r) {
            if (r == k) continue;
            const double f = PW(9 * r + k);
            for (int c = k + 1; c < 9; ++c) PW(9 * r + c) = PW(9 * r + c) - f * PW(9 * k + c);
        }
    }
    for (int j = 0; j < 4; ++j) {
        for (int e = 0; e < 9; ++e) PW(PM_N + 9 * j + e) = 0.0;
        for (int i = 0; i < 5; ++i) PW(PM_N + 9 * j + (int)((perm >> (4 * i)) & 15ull)) = -PW(9 * i + 5 + j);
        PW(PM_N + 9 * j + (int)((perm >> (4 * (5 + j))) & 15ull)) = 1.0;
    }
    // ---- the 10 x 20 constraint matrix.  Entry e of E is the polynomial (N[0][e], N[1][e], N[2][e], N[3][e])
    // over (x, y, z, 1): offset PM_N + e, stride 9.
    {
        int o = PM_T;
        for (int i = 0; i < 3; ++i)
            for (int k = i; k < 3; ++k) {
                for (int m = 0; m < 10; ++m) PW(o + m) = 0.0;
                for (int m = 0; m < 3; ++m) pmul11(w, s, o, PM_N + 3 * i + m, 9, PM_N + 3 * k + m, 9, false);
                o += 10;
            }
        for (int m = 0; m < 10; ++m) PW(PM_T + 60 + m) = (PW(PM_T + m) + PW(PM_T + 30 + m)) + PW(PM_T + 50 + m);
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int row = PM_A + 20 * (3 * i + j);
            for (int m = 0; m < 20; ++m) PW(row + m) = 0.0;
            for (int k = 0; k < 3; ++k) {
                const int lo = i < k ? i : k, hi = i < k ? k : i;
                const int sym = lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);   // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
                pmul21(w, s, row, PM_T + 10 * sym, PM_N + 3 * k + j, 9, false);
            }
            for (int m = 0; m < 20; ++m) PW(row + m) = 2.0 * PW(row + m);
            pmul21(w, s, row, PM_T + 60, PM_N + 3 * i + j, 9, true);
        }
    {
        const int row = PM_A + 180, minor = PM_T + 70;
        for (int m = 0; m < 20; ++m) PW(row + m) = 0.0;
        for (int c = 0; c < 3; ++c) {
            const int a0 = c == 0 ? 4 : 3, a1 = c == 2 ? 7 : 8, b0 = c == 2 ? 4 : 5, b1 = c == 0 ? 7 : 6;
            for (int m = 0; m < 10; ++m) PW(minor + m) = 0.0;
            pmul11(w, s, minor, PM_N + a0, 9, PM_N + a1, 9, false);
            pmul11(w, s, minor, PM_N + b0, 9, PM_N + b1, 9, true);
            pmul21(w, s, row, minor, PM_N + c, 9, c == 1);
        }
    }
    // ---- Gauss-Jordan elimination of the first 10 columns, partial pivoting
    for (int k = 0; k < 10; ++k) {
        double best = 0.0;
        int pr = -1;
        for (int r = k; r < 10; ++r) {
            const double v = fabs(PW(PM_A + 20 * r + k));
            if (v > best) { best = v; pr = r; }
        }
        if (!(best > 0.0)) return 0;
        if (pr != k)
            for (int c = 0; c < 20; ++c) { const double t = PW(PM_A + 20 * k + c); PW(PM_A + 20 * k + c) = PW(PM_A + 20 * pr + c); PW(PM_A + 20 * pr + c) = t; }
        const double p = PW(PM_A + 20 * k + k);
        for (int c = k + 1; c < 20; ++c) PW(PM_A + 20 * k + c) = PW(PM_A + 20 * k + c) / p;
        for (int r = 0; r < 10; ++r) {
            if (r == k) continue;
            const double f = PW(PM_A + 20 * r + k);
            for (int c = k + 1; c < 20; ++c) PW(PM_A + 20 * r + c) = PW(PM_A + 20 * r + c) - f * PW(PM_A + 20 * k + c);
        }
    }
    // ---- B(z) (x, y, 1)^T = 0 from rows (4 - z 5), (6 - z 7), (8 - z 9); coefficients ascending in z
    for (int r = 0; r < 3; ++r) {
        const int p = PM_A + 20 * (4 + 2 * r), q2 = p + 20, b = PM_B + 13 * r;
        for (int v = 0; v < 2; ++v) {   // x: columns 10-12, y: columns 13-15
            const int c = 10 + 3 * v, o = b + 4 * v;
            PW(o) = PW(p + c + 2);
            PW(o + 1) = PW(p + c + 1) - PW(q2 + c + 2);
            PW(o + 2) = PW(p + c) - PW(q2 + c + 1);
            PW(o + 3) = -PW(q2 + c);
        }
        PW(b + 8) = PW(p + 19);
        PW(b + 9) = PW(p + 18) - PW(q2 + 19);
        PW(b + 10) = PW(p + 17) - PW(q2 + 18);
        PW(b + 11) = PW(p + 16) - PW(q2 + 17);
        PW(b + 12) = -PW(q2 + 16);
    }
    // ---- det B(z): bx0 (by1 bc2 - by2 bc1) - by0 (bx1 bc2 - bx2 bc1) + bc0 (bx1 by2 - bx2 by1)
    {
        const int b0 = PM_B, b1 = PM_B + 13, b2 = PM_B + 26;
        for (int m = 0; m < 8 + 8 + 7 + 11; ++m) PW(PM_P1 + m) = 0.0;
        pconv(w, s, PM_P1, b1 + 4, 4, b2 + 8, 5, false);
        pconv(w, s, PM_P1, b2 + 4, 4, b1 + 8, 5, true);
        pconv(w, s, PM_P2, b1, 4, b2 + 8, 5, false);
        pconv(w, s, PM_P2, b2, 4, b1 + 8, 5, true);
        pconv(w, s, PM_P3, b1, 4, b2 + 4, 4, false);
        pconv(w, s, PM_P3, b2, 4, b1 + 4, 4, true);
        pconv(w, s, PM_C, b0, 4, PM_P1, 8, false);
        pconv(w, s, PM_C, b0 + 4, 4, PM_P2, 8, true);
        pconv(w, s, PM_C, b0 + 8, 5, PM_P3, 7, false);
    }
    // ---- the real roots: each level's roots are bracketed by the previous level's (the derivative's) inside
    // the Cauchy bound, then bisected until the interval is two neighbouring doubles
    for (int i = 0; i <= 10; ++i)
        if (!finite_d(PW(PM_C + i))) return 0;
    const double lead = PW(PM_C + 10);
    if (lead == 0.0) return 0;
    double R = 0.0;
    for (int i = 0; i < 10; ++i) {
        const double v = fabs(PW(PM_C + i) / lead);
        if (v > R) R = v;
    }
    R = 1.0 + R;
    if (!(R < 1e300)) return 0;
    for (int i = 0; i <= 10; ++i) PW(PM_DP + 54 + i) = PW(PM_C + i);
    for (int d = 10; d > 1; --d) {
        const int src = PM_DP + d * (d + 1) / 2 - 1, dst = PM_DP + (d - 1) * d / 2 - 1;
        for (int i = 0; i < d; ++i) PW(dst + i) = PW(src + i + 1) * (double)(i + 1);
    }
    int nroots = 0, cur = PM_R0, nxt = PM_R1;
    for (int d = 1; d <= 10; ++d) {
        const int c = PM_DP + d * (d + 1) / 2 - 1;
        int nnew = 0;
        double lo0 = -R, fa = phorner(w, s, c, d, lo0);
        for (int sgm = 0; sgm <= nroots; ++sgm) {
            double lo = lo0, hi = sgm < nroots ? PW(cur + sgm) : R;
            const double hi0 = hi, fb = phorner(w, s, c, d, hi);
            const bool neg = fa < 0.0;
            if (neg != (fb < 0.0)) {
                for (int it = 0; it < MAX_HALVINGS; ++it) {
                    const double mid = 0.5 * (lo + hi);
                    if (!(lo < mid && mid < hi)) break;
                    const double fm = phorner(w, s, c, d, mid);
                    if ((fm < 0.0) == neg) lo = mid; else hi = mid;
                }
                PW(nxt + nnew) = 0.5 * (lo + hi);
                ++nnew;
            }
            lo0 = hi0;
            fa = fb;
        }
        nroots = nnew;
        const int t = cur; cur = nxt; nxt = t;
    }
    // ---- per root: (x, y, 1) ~ the cross product of two rows of B(z) with the largest third component
    int nm = 0;
    for (int k = 0; k < nroots; ++k) {
        const double z = PW(cur + k);
        double best = -1.0, cx = 0.0, cy = 0.0, cz = 0.0;
        for (int pq = 0; pq < 3; ++pq) {
            const int a = PM_B + 13 * (pq == 2 ? 1 : 0), b = PM_B + 13 * (pq == 0 ? 1 : 2);
            const double a0 = phorner(w, s, a, 3, z), a1 = phorner(w, s, a + 4, 3, z), a2 = phorner(w, s, a + 8, 4, z);
            const double b0 = phorner(w, s, b, 3, z), b1 = phorner(w, s, b + 4, 3, z), b2 = phorner(w, s, b + 8, 4, z);
            const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
            if (fabs(c2) > best) { best = fabs(c2); cx = c0; cy = c1; cz = c2; }
        }
        const double x = cx / cz, y = cy / cz;
        const int m = PM_MODELS + 9 * nm;
        double ss = 0.0;
        for (int e = 0; e < 9; ++e) {
            const double v = ((x * PW(PM_N + e) + y * PW(PM_N + 9 + e)) + z * PW(PM_N + 18 + e)) + PW(PM_N + 27 + e);
            PW(m + e) = v;
            ss = ss + v * v;
        }
        const double nrm = sqrt(ss);
        bool ok = true;
        for (int e = 0; e < 9; ++e) {
            const double v = PW(m + e) / nrm;
            PW(m + e) = v;
            ok = ok && finite_d(v);
        }
        if (ok) ++nm;
    }
    return nm;
}
#undef PW

// EMEstimatorCallback::computeError: the Sampson error of (x1, y1) -> (x2, y2) under E, rounded to float
PM_HD float sampson_error(const double* E, double x1, double y1, double x2, double y2) {
    const double e0 = (E[0] * x1 + E[1] * y1) + E[2];
    const double e1 = (E[3] * x1 + E[4] * y1) + E[5];
    const double e2 = (E[6] * x1 + E[7] * y1) + E[8];
    const double t0 = (E[0] * x2 + E[3] * y2) + E[6];
    const double t1 = (E[1] * x2 + E[4] * y2) + E[7];
    const double sv = (x2 * e0 + y2 * e1) + e2;
    return (float)((sv * sv) / (((e0 * e0 + e1 * e1) + t0 * t0) + t1 * t1));
}

PM_HD double sum3(double a, double b, double c) { return (a + b) + c; }
PM_HD double sum4(double a, double b, double c, double d) { return ((a + b) + c) + d; }

// one Jacobi rotation of rows I, J of an N x N system (JacobiSVDImpl_; the rotation of csrc/triangulate.hip)
template <int N, int I, int J>
PM_HD bool jrotate(double (&At)[N][N], double (&V)[N][N], double (&W)[N]) {
    const double eps = 10.0 * 2.220446049250313e-16;   // 10 * DBL_EPSILON
    double p;
    if (N == 3) p = sum3(At[I][0] * At[J][0], At[I][1] * At[J][1], At[I][2] * At[J][2]);
    else p = sum4(At[I][0] * At[J][0], At[I][1] * At[J][1], At[I][2] * At[J][2], At[I][N - 1] * At[J][N - 1]);
    if (fabs(p) <= eps * sqrt(W[I] * W[J])) return false;
    p = 2.0 * p;
    const double beta = W[I] - W[J];
    const double gamma = sqrt(p * p + beta * beta);   // OpenCV: hypot(p, beta)
    double c, s;
    if (beta < 0) {
        s = sqrt(((gamma - beta) * 0.5) / gamma);
        c = p / (gamma * s * 2.0);
    } else {
        c = sqrt((gamma + beta) / (gamma * 2.0));
        s = p / (gamma * c * 2.0);
    }
    double t0[N], t1[N];
PM_UNROLL
    for (int k = 0; k < N; ++k) {
        t0[k] = c * At[I][k] + s * At[J][k];
        t1[k] = c * At[J][k] - s * At[I][k];
        At[I][k] = t0[k];
        At[J][k] = t1[k];
    }
    if (N == 3) {
        W[I] = sum3(t0[0] * t0[0], t0[1] * t0[1], t0[2] * t0[2]);
        W[J] = sum3(t1[0] * t1[0], t1[1] * t1[1], t1[2] * t1[2]);
    } else {
        W[I] = sum4(t0[0] * t0[0], t0[1] * t0[1], t0[2] * t0[2], t0[N - 1] * t0[N - 1]);
        W[J] = sum4(t1[0] * t1[0], t1[1] * t1[1], t1[2] * t1[2], t1[N - 1] * t1[N - 1]);
    }
PM_UNROLL
    for (int k = 0; k < N; ++k) {
        const double v0 = c * V[I][k] + s * V[J][k];
        const double v1 = c * V[J][k] - s * V[I][k];
        V[I][k] = v0;
        V[J][k] = v1;
    }
    return true;
}

// the right singular vector of the smallest singular value of the 4 x 4 system (At = its transpose): the
// jacobi_null of csrc/triangulate.hip without the rounding to float
PM_HD void jacobi_null4(double (&At)[4][4], double (&h)[4]) {
    double V[4][4], W[4];
PM_UNROLL
    for (int i = 0; i < 4; ++i) {
PM_UNROLL
        for (int k = 0; k < 4; ++k) V[i][k] = i == k ? 1.0 : 0.0;
        W[i] = sum4(At[i][0] * At[i][0], At[i][1] * At[i][1], At[i][2] * At[i][2], At[i][3] * At[i][3]);
    }
PM_UNROLL1
    for (int sweep = 0; sweep < SVD_SWEEPS; ++sweep) {
        bool changed = jrotate<4, 0, 1>(At, V, W);
        changed |= jrotate<4, 0, 2>(At, V, W);
        changed |= jrotate<4, 0, 3>(At, V, W);
        changed |= jrotate<4, 1, 2>(At, V, W);
        changed |= jrotate<4, 1, 3>(At, V, W);
        changed |= jrotate<4, 2, 3>(At, V, W);
        if (!changed) break;
    }
    int idx[4];
PM_UNROLL
    for (int i = 0; i < 4; ++i) {
        W[i] = sqrt(sum4(At[i][0] * At[i][0], At[i][1] * At[i][1], At[i][2] * At[i][2], At[i][3] * At[i][3]));
        idx[i] = i;
    }
PM_UNROLL
    for (int i = 0; i < 3; ++i) {   // selection sort, descending; the rows follow through idx
        int j = i;
        double wj = W[i];
PM_UNROLL
        for (int k = i + 1; k < 4; ++k) {
            const bool lt = wj < W[k];
            j = lt ? k : j;
            wj = lt ? W[k] : wj;
        }
PM_UNROLL
        for (int m = i + 1; m < 4; ++m) {
            const bool sw = j == m;
            const double wi = W[i], wm = W[m];
            const int ii = idx[i], im = idx[m];
            W[i] = sw ? wm : wi;
            W[m] = sw ? wi : wm;
            idx[i] = sw ? im : ii;
            idx[m] = sw ? ii : im;
        }
    }
    const int r = idx[3];
PM_UNROLL
    for (int k = 0; k < 4; ++k) h[k] = r == 0 ? V[0][k] : (r == 1 ? V[1][k] : (r == 2 ? V[2][k] : V[3][k]));
}

PM_HD double det3(const double (&M)[3][3]) {
    return (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])) +
           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

// rows A, B of At, V and W exchanged when sw
template <int A, int B>
PM_HD void cswap3(bool sw, double (&At)[3][3], double (&V)[3][3], double (&W)[3]) {
PM_UNROLL
    for (int k = 0; k < 3; ++k) {
        const double a = At[A][k], b = At[B][k], c = V[A][k], d = V[B][k];
        At[A][k] = sw ? b : a; At[B][k] = sw ? a : b;
        V[A][k] = sw ? d : c;  V[B][k] = sw ? c : d;
    }
    const double a = W[A], b = W[B];
    W[A] = sw ? b : a;
    W[B] = sw ? a : b;
}

// cv::decomposeEssentialMat + recoverPose's four candidates: cand[c] = [R1|t], [R2|t], [R1|-t], [R2|-t]
// (3 x 4 row-major).  The SVD is the one-sided Jacobi on the rows of At = E^T; U's third column is the cross
// product of the first two (E has rank 2).
PM_HD void pose_candidates(const double* E, double (&cand)[4][12]) {
    double At[3][3], V[3][3], W[3];
PM_UNROLL
    for (int i = 0; i < 3; ++i) {
PM_UNROLL
        for (int k = 0; k < 3; ++k) { At[i][k] = E[3 * k + i]; V[i][k] = i == k ? 1.0 : 0.0; }
    }
PM_UNROLL
    for (int i = 0; i < 3; ++i) W[i] = sum3(At[i][0] * At[i][0], At[i][1] * At[i][1], At[i][2] * At[i][2]);
PM_UNROLL1
    for (int sweep = 0; sweep < SVD_SWEEPS; ++sweep) {
        bool changed = jrotate<3, 0, 1>(At, V, W);
        changed |= jrotate<3, 0, 2>(At, V, W);
        changed |= jrotate<3, 1, 2>(At, V, W);
        if (!changed) break;
    }
PM_UNROLL
    for (int i = 0; i < 3; ++i) W[i] = sqrt(sum3(At[i][0] * At[i][0], At[i][1] * At[i][1], At[i][2] * At[i][2]));
    {   // selection sort, descending
        int j = 0;
        if (W[j] < W[1]) j = 1;
        if ((j == 0 ? W[0] : W[1]) < W[2]) j = 2;
        cswap3<0, 1>(j == 1, At, V, W);
        cswap3<0, 2>(j == 2, At, V, W);
        cswap3<1, 2>(W[1] < W[2], At, V, W);
    }
    double U[3][3];
    const double u00 = At[0][0] / W[0], u01 = At[0][1] / W[0], u02 = At[0][2] / W[0];
    const double u10 = At[1][0] / W[1], u11 = At[1][1] / W[1], u12 = At[1][2] / W[1];
    U[0][0] = u00; U[1][0] = u01; U[2][0] = u02;
    U[0][1] = u10; U[1][1] = u11; U[2][1] = u12;
    U[0][2] = u01 * u12 - u02 * u11;
    U[1][2] = u02 * u10 - u00 * u12;
    U[2][2] = u00 * u11 - u01 * u10;
    const bool nu = det3(U) < 0, nv = det3(V) < 0;
PM_UNROLL
    for (int r = 0; r < 3; ++r) {
PM_UNROLL
        for (int c = 0; c < 3; ++c) {
            U[r][c] = nu ? -U[r][c] : U[r][c];
            V[r][c] = nv ? -V[r][c] : V[r][c];
        }
    }
PM_UNROLL
    for (int r = 0; r < 3; ++r) {
PM_UNROLL
        for (int c = 0; c < 3; ++c) {
            const double r1 = ((-U[r][1]) * V[0][c] + U[r][0] * V[1][c]) + U[r][2] * V[2][c];
            const double r2 = (U[r][1] * V[0][c] + (-U[r][0]) * V[1][c]) + U[r][2] * V[2][c];
            cand[0][4 * r + c] = r1; cand[2][4 * r + c] = r1;
            cand[1][4 * r + c] = r2; cand[3][4 * r + c] = r2;
        }
        cand[0][4 * r + 3] = U[r][2];  cand[1][4 * r + 3] = U[r][2];
        cand[2][4 * r + 3] = -U[r][2]; cand[3][4 * r + 3] = -U[r][2];
    }
}

// recoverPose's test of one correspondence under P1 (3 x 4): cv::triangulatePoints([I|0], P1) by the DLT of
// csrc/triangulate.hip on double points, then Z > 0 and Z < 50 in both views.
PM_HD bool cheirality(const double* P1, double x1, double y1, double x2, double y2) {
    double At[4][4], h[4];
PM_UNROLL
    for (int k = 0; k < 4; ++k) {
        const double i0 = k == 0 ? 1.0 : 0.0, i1 = k == 1 ? 1.0 : 0.0, i2 = k == 2 ? 1.0 : 0.0;
        At[k][0] = x1 * i2 - i0;
        At[k][1] = y1 * i2 - i1;
        At[k][2] = x2 * P1[8 + k] - P1[k];
        At[k][3] = y2 * P1[8 + k] - P1[4 + k];
    }
    jacobi_null4(At, h);
    bool m = (h[2] * h[3]) > 0;
    const double X = h[0] / h[3], Y = h[1] / h[3], Z = h[2] / h[3];
    m = m && Z < 50.0;
    const double Z2 = ((P1[8] * X + P1[9] * Y) + P1[10] * Z) + P1[11];
    m = m && Z2 > 0;
    m = m && Z2 < 50.0;
    return m;
}

// recoverPose's >= cascade over the four counts
PM_HD int choose_candidate(int g0, int g1, int g2, int g3) {
    if (g0 >= g1 && g0 >= g2 && g0 >= g3) return 0;
    if (g1 >= g0 && g1 >= g2 && g1 >= g3) return 1;
    if (g2 >= g0 && g2 >= g1 && g2 >= g3) return 2;
    return 3;
}

struct CamP {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

// cv::undistortPoints, TermCriteria(COUNT, 5), result rounded to float (the undistort of csrc/triangulate.hip)
PM_HD void undistort_f(float px, float py, const CamP& S, float& ox, float& oy) {
    const double ifx = 1.0 / S.fx, ify = 1.0 / S.fy;
    double x = ((double)px - S.cx) * ifx;
    double y = ((double)py - S.cy) * ify;
    const double x0 = x, y0 = y;
    for (int it = 0; it < 5; ++it) {
        const double r2 = x * x + y * y;
        const double icdist = 1.0 / (1.0 + ((S.k3 * r2 + S.k2) * r2 + S.k1) * r2);
        if (icdist < 0) { x = x0; y = y0; break; }
        const double dX = 2.0 * S.p1 * x * y + S.p2 * (r2 + 2.0 * x * x);
        const double dY = S.p1 * (r2 + 2.0 * y * y) + 2.0 * S.p2 * x * y;
        x = (x0 - dX) * icdist;
        y = (y0 - dY) * icdist;
    }
    ox = (float)x;
    oy = (float)y;
}

// The two-camera findEssentialMat overload up to the RANSAC's points: undistort with the side's own camera,
// back to float pixels with the mean camera matrix (fx, fy, cx, cy), then (p - c) / f in double.
PM_HD void prepare_point(float px, float py, const CamP& S, double fx, double fy, double cx, double cy, double& ox, double& oy) {
    float x, y;
    undistort_f(px, py, S, x, y);
    const float u = (float)(fx * (double)x + cx);
    const float v = (float)(fy * (double)y + cy);
    ox = ((double)u - cx) / fx;
    oy = ((double)v - cy) / fy;
}

}  // namespace posem
}  // namespace sfmx
