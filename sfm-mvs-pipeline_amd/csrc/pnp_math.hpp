// SPDX-License-Identifier: MIT
// The arithmetic of sfmx_register_poses (SfM::findCameraPoseFrom3d2dMatch, sfm/SfM.cpp:453-489), host and device:
// EPnP on five points, the reprojection error of PnPRansacCallback and the pieces of the solvePnP(ITERATIVE) refit,
// operation by operation in the order of tests/pnp_ref.py.  One correctly rounded IEEE + - * / sqrt
// per step: every translation unit that includes this header is compiled with -ffp-contract=off.  The RANSAC stage
// calls nothing from libm but sqrt and fabs; the refit's rodrigues / rodrigues_inv also call sin, cos and acos.
//
// The solver works in a caller-provided workspace of PN_WS doubles that it addresses as w[i * s]: s = 1 on the
// host, s = the batch size in the kernel, where w points into LDS at the lane's own column (element-major, so
// the lanes of a wave touch consecutive banks).  Every array of the solver lives there; nothing is an array in
// registers, so nothing can spill.  (CamP and undistort_f are copies of pose_math.hpp's, so that pose.hip and
// triangulate.hip keep their code objects: §8h.)
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PN_HD __host__ __device__ inline
#else
#define PN_HD inline
#endif

namespace sfmx {
namespace pnpm {

// ---- workspace layout (doubles).  Kept through the whole solve:
constexpr int PN_PW = 0;              // 5 x 3 the 3-D points
constexpr int PN_UV = 15;             // 5 x 2 the normalised image points
constexpr int PN_CWS = 25;            // 4 x 3 control points
constexpr int PN_D = 37;              // 5 x 3 points - centroid
constexpr int PN_AL = 52;             // 5 x 4 barycentric coordinates
constexpr int PN_RHO = 72;            // 6
constexpr int PN_V = 78;              // 4 x 12 eigenvectors of the four smallest eigenvalues, ascending
constexpr int PN_RES = 126;           // 3 x 13: pose and rep_error of the three approximations
constexpr int PN_T = 165;             // phase regions start here
// phase 1 (up to the eigenvectors)
constexpr int PN_S3 = PN_T;           // packed 3 x 3 (6) and its eigenvectors (9); the cofactor inverse (9)
constexpr int PN_V3 = PN_T + 6;
constexpr int PN_CI = PN_T + 15;
constexpr int PN_MTM = PN_T + 24;     // packed 12 x 12 (78)
constexpr int PN_VT = PN_MTM + 78;    // 12 x 12 eigenvectors (144); before them the 10 x 12 M (120)
constexpr int PN_END1 = PN_VT + 144;
// phase 2 (betas and poses)
constexpr int PN_L = PN_T;            // 6 x 10
constexpr int PN_QA = PN_L + 60;      // qr_solve: A (6 x 5 at most), b (6), A1, A2, x (5 each)
constexpr int PN_QB = PN_QA + 30;
constexpr int PN_A1 = PN_QB + 6;
constexpr int PN_A2 = PN_A1 + 5;
constexpr int PN_X = PN_A2 + 5;
constexpr int PN_BETA = PN_X + 5;     // 4
constexpr int PN_CCS = PN_BETA + 4;   // 4 x 3
constexpr int PN_PCS = PN_CCS + 12;   // 5 x 3
constexpr int PN_ABT = PN_PCS + 15;   // 9
constexpr int PN_SAT = PN_ABT + 9;    // svd: At (9), V (9), W (3), U (9)
constexpr int PN_SV = PN_SAT + 9;
constexpr int PN_SW = PN_SV + 9;
constexpr int PN_SU = PN_SW + 3;
constexpr int PN_R = PN_SU + 9;       // R (9), t (3), pc0 (3)
constexpr int PN_TT = PN_R + 9;
constexpr int PN_PC0 = PN_TT + 3;
constexpr int PN_END2 = PN_PC0 + 3;
constexpr int PN_WS = PN_END1 > PN_END2 ? PN_END1 : PN_END2;   // doubles of workspace per sample
static_assert(PN_WS == 411, "workspace size is part of the kernel's LDS budget (DESIGN.md 8i)");

constexpr int EIG_SWEEPS = 30;
constexpr int SVD_SWEEPS = 30;
constexpr int GN_STEPS = 5;
constexpr double JEPS = 10.0 * 2.220446049250313e-16;   // 10 * DBL_EPSILON
constexpr double PLANE_EPS = 1e-12;   // eigenvalue ratio under which a sample has no extent (float inputs: 2^-48)

#define PW(i) w[(i) * s]

PN_HD bool finite_d(double v) { return fabs(v) < HUGE_VAL; }   // false for a NaN
PN_HD int si(int n, int i, int j) {                           // (i, j) in the packed upper triangle
    if (i > j) { const int t = i; i = j; j = t; }
    return i * n - (i * (i - 1)) / 2 + (j - i);
}
PN_HD double wdot3(const double* w, int s, int a, int b) { return (PW(a) * PW(b) + PW(a + 1) * PW(b + 1)) + PW(a + 2) * PW(b + 2); }

// cyclic Jacobi on the packed symmetric n x n at A (its diagonal becomes the eigenvalues); row j of Vt is the
// eigenvector of the j-th diagonal entry
PN_HD void jacobi_eig(double* w, int s, int A, int Vt, int n) {
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < n; ++k) PW(Vt + n * i + k) = i == k ? 1.0 : 0.0;
    double big = 0.0;
    for (int i = 0; i < n; ++i) {
        const double v = fabs(PW(A + si(n, i, i)));
        if (v > big) big = v;
    }
    const double tol = JEPS * big;
    for (int sweep = 0; sweep < EIG_SWEEPS; ++sweep) {
        bool changed = false;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const int ipq = A + si(n, p, q);
                const double apq = PW(ipq);
                if (fabs(apq) <= tol) continue;
                const int ipp = A + si(n, p, p), iqq = A + si(n, q, q);
                const double app = PW(ipp), aqq = PW(iqq);
                const double theta = (aqq - app) / (2.0 * apq);
                double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(t * t + 1.0);
                const double sn = t * c;
                for (int k = 0; k < n; ++k) {
                    if (k == p || k == q) continue;
                    const int ikp = A + si(n, k, p), ikq = A + si(n, k, q);
                    const double akp = PW(ikp), akq = PW(ikq);
                    PW(ikp) = c * akp - sn * akq;
                    PW(ikq) = sn * akp + c * akq;
                }
                PW(ipp) = app - t * apq;
                PW(iqq) = aqq + t * apq;
                PW(ipq) = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double vp = PW(Vt + n * p + k), vq = PW(Vt + n * q + k);
                    PW(Vt + n * p + k) = c * vp - sn * vq;
                    PW(Vt + n * q + k) = sn * vp + c * vq;
                }
                changed = true;
            }
        if (!changed) break;
    }
}

// epnp::qr_solve: least squares of the nr x nc system at PN_QA (row-major), right side at PN_QB -> PN_X;
// false when a column is zero
PN_HD bool qr_solve(double* w, int s, int nr, int nc) {
    for (int k = 0; k < nc; ++k) {
        double eta = fabs(PW(PN_QA + k * nc + k));
        for (int i = k + 1; i < nr; ++i) {
            const double v = fabs(PW(PN_QA + i * nc + k));
            if (v > eta) eta = v;
        }
        if (!(eta > 0.0)) return false;
        const double inv_eta = 1.0 / eta;
        double sm = 0.0;
        for (int i = k; i < nr; ++i) {
            const double v = PW(PN_QA + i * nc + k) * inv_eta;
            PW(PN_QA + i * nc + k) = v;
            sm = sm + v * v;
        }
        double sigma = sqrt(sm);
        if (PW(PN_QA + k * nc + k) < 0.0) sigma = -sigma;
        const double akk = PW(PN_QA + k * nc + k) + sigma;
        PW(PN_QA + k * nc + k) = akk;
        PW(PN_A1 + k) = sigma * akk;
        PW(PN_A2 + k) = -eta * sigma;
        for (int j = k + 1; j < nc; ++j) {
            sm = 0.0;
            for (int i = k; i < nr; ++i) sm = sm + PW(PN_QA + i * nc + k) * PW(PN_QA + i * nc + j);
            const double tau = sm / PW(PN_A1 + k);
            for (int i = k; i < nr; ++i) PW(PN_QA + i * nc + j) = PW(PN_QA + i * nc + j) - tau * PW(PN_QA + i * nc + k);
        }
    }
    for (int j = 0; j < nc; ++j) {
        double tau = 0.0;
        for (int i = j; i < nr; ++i) tau = tau + PW(PN_QA + i * nc + j) * PW(PN_QB + i);
        tau = tau / PW(PN_A1 + j);
        for (int i = j; i < nr; ++i) PW(PN_QB + i) = PW(PN_QB + i) - tau * PW(PN_QA + i * nc + j);
    }
    PW(PN_X + nc - 1) = PW(PN_QB + nc - 1) / PW(PN_A2 + nc - 1);
    for (int i = nc - 2; i >= 0; --i) {
        double sm = 0.0;
        for (int j = i + 1; j < nc; ++j) sm = sm + PW(PN_QA + i * nc + j) * PW(PN_X + j);
        PW(PN_X + i) = (PW(PN_QB + i) - sm) / PW(PN_A2 + i);
    }
    return true;
}

// M (9, row-major, at PN_ABT) = U diag(w) Vt: U at PN_SU, Vt at PN_SV.  The one-sided Jacobi of pose_math.hpp on
// the rows of M^T, rows sorted by descending norm, the columns of U the normalised rows (the third a cross product
// when its singular value is not above JEPS times the largest).
PN_HD void svd3_full(double* w, int s) {
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) {
            PW(PN_SAT + 3 * i + k) = PW(PN_ABT + 3 * k + i);
            PW(PN_SV + 3 * i + k) = i == k ? 1.0 : 0.0;
        }
    for (int i = 0; i < 3; ++i) PW(PN_SW + i) = wdot3(w, s, PN_SAT + 3 * i, PN_SAT + 3 * i);
    for (int sweep = 0; sweep < SVD_SWEEPS; ++sweep) {
        bool changed = false;
        for (int pr = 0; pr < 3; ++pr) {
            const int i = pr == 2 ? 1 : 0, j = pr == 0 ? 1 : 2;
            double p = wdot3(w, s, PN_SAT + 3 * i, PN_SAT + 3 * j);
            if (fabs(p) <= JEPS * sqrt(PW(PN_SW + i) * PW(PN_SW + j))) continue;
            p = 2.0 * p;
            const double beta = PW(PN_SW + i) - PW(PN_SW + j);
            const double gamma = sqrt(p * p + beta * beta);
            double c, sn;
            if (beta < 0) {
                sn = sqrt(((gamma - beta) * 0.5) / gamma);
                c = p / (gamma * sn * 2.0);
            } else {
                c = sqrt((gamma + beta) / (gamma * 2.0));
                sn = p / (gamma * c * 2.0);
            }
            for (int m = 0; m < 2; ++m) {
                const int base = m == 0 ? PN_SAT : PN_SV;
                for (int k = 0; k < 3; ++k) {
                    const double a = PW(base + 3 * i + k), b = PW(base + 3 * j + k);
                    PW(base + 3 * i + k) = c * a + sn * b;
                    PW(base + 3 * j + k) = c * b - sn * a;
                }
            }
            PW(PN_SW + i) = wdot3(w, s, PN_SAT + 3 * i, PN_SAT + 3 * i);
            PW(PN_SW + j) = wdot3(w, s, PN_SAT + 3 * j, PN_SAT + 3 * j);
            changed = true;
        }
        if (!changed) break;
    }
    for (int i = 0; i < 3; ++i) PW(PN_SW + i) = sqrt(wdot3(w, s, PN_SAT + 3 * i, PN_SAT + 3 * i));
    for (int i = 0; i < 2; ++i) {   // selection sort, descending
        int j = i;
        for (int k = i + 1; k < 3; ++k)
            if (PW(PN_SW + j) < PW(PN_SW + k)) j = k;
        if (j != i) {
            double t = PW(PN_SW + i); PW(PN_SW + i) = PW(PN_SW + j); PW(PN_SW + j) = t;
            for (int k = 0; k < 3; ++k) {
                t = PW(PN_SAT + 3 * i + k); PW(PN_SAT + 3 * i + k) = PW(PN_SAT + 3 * j + k); PW(PN_SAT + 3 * j + k) = t;
                t = PW(PN_SV + 3 * i + k); PW(PN_SV + 3 * i + k) = PW(PN_SV + 3 * j + k); PW(PN_SV + 3 * j + k) = t;
            }
        }
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 2; ++c) PW(PN_SU + 3 * r + c) = PW(PN_SAT + 3 * c + r) / PW(PN_SW + c);
    if (PW(PN_SW + 2) > JEPS * PW(PN_SW)) {
        for (int r = 0; r < 3; ++r) PW(PN_SU + 3 * r + 2) = PW(PN_SAT + 6 + r) / PW(PN_SW + 2);
    } else {   // rank 2 (coplanar points): completed by the cross product
        const double a0 = PW(PN_SU), a1 = PW(PN_SU + 3), a2 = PW(PN_SU + 6), b0 = PW(PN_SU + 1), b1 = PW(PN_SU + 4), b2 = PW(PN_SU + 7);
        PW(PN_SU + 2) = a1 * b2 - a2 * b1;
        PW(PN_SU + 5) = a2 * b0 - a0 * b2;
        PW(PN_SU + 8) = a0 * b1 - a1 * b0;
    }
}

PN_HD double wdet3(const double* w, int s, int M) {
    return (PW(M) * (PW(M + 4) * PW(M + 8) - PW(M + 5) * PW(M + 7)) - PW(M + 1) * (PW(M + 3) * PW(M + 8) - PW(M + 5) * PW(M + 6))) +
           PW(M + 2) * (PW(M + 3) * PW(M + 7) - PW(M + 4) * PW(M + 6));
}

// find_betas_approx_1 / _2 / _3 (which = 0, 1, 2) -> PN_BETA; false when the system has a zero column
PN_HD bool betas_approx(double* w, int s, int which) {
    const int nc = which == 0 ? 4 : (which == 1 ? 3 : 5);
    for (int r = 0; r < 6; ++r) {
        for (int c = 0; c < nc; ++c) {
            const int col = which == 0 ? (c == 2 ? 3 : (c == 3 ? 6 : c)) : c;   // {0,1,3,6}, {0,1,2}, {0..4}
            PW(PN_QA + r * nc + c) = PW(PN_L + 10 * r + col);
        }
        PW(PN_QB + r) = PW(PN_RHO + r);
    }
    if (!qr_solve(w, s, 6, nc)) return false;
    const double x0 = PW(PN_X), x1 = PW(PN_X + 1), x2 = PW(PN_X + 2), x3 = PW(PN_X + 3);
    if (which == 0) {
        if (x0 < 0) {
            const double b0 = sqrt(-x0);
            PW(PN_BETA) = b0; PW(PN_BETA + 1) = -x1 / b0; PW(PN_BETA + 2) = -x2 / b0; PW(PN_BETA + 3) = -x3 / b0;
        } else {
            const double b0 = sqrt(x0);
            PW(PN_BETA) = b0; PW(PN_BETA + 1) = x1 / b0; PW(PN_BETA + 2) = x2 / b0; PW(PN_BETA + 3) = x3 / b0;
        }
        return true;
    }
    double b0, b1;
    if (x0 < 0) {
        b0 = sqrt(-x0);
        b1 = x2 < 0 ? sqrt(-x2) : 0.0;
    } else {
        b0 = sqrt(x0);
        b1 = x2 > 0 ? sqrt(x2) : 0.0;
    }
    if (x1 < 0) b0 = -b0;
    PW(PN_BETA) = b0; PW(PN_BETA + 1) = b1;
    PW(PN_BETA + 2) = which == 1 ? 0.0 : x3 / b0;
    PW(PN_BETA + 3) = 0.0;
    return true;
}

PN_HD bool gauss_newton(double* w, int s) {
    for (int it = 0; it < GN_STEPS; ++it) {
        const double b0 = PW(PN_BETA), b1 = PW(PN_BETA + 1), b2 = PW(PN_BETA + 2), b3 = PW(PN_BETA + 3);
        for (int i = 0; i < 6; ++i) {
            const int l = PN_L + 10 * i;
            const double l0 = PW(l), l1 = PW(l + 1), l2 = PW(l + 2), l3 = PW(l + 3), l4 = PW(l + 4), l5 = PW(l + 5),
                         l6 = PW(l + 6), l7 = PW(l + 7), l8 = PW(l + 8), l9 = PW(l + 9);
            PW(PN_QA + 4 * i + 0) = ((2.0 * l0 * b0 + l1 * b1) + l3 * b2) + l6 * b3;
            PW(PN_QA + 4 * i + 1) = ((l1 * b0 + 2.0 * l2 * b1) + l4 * b2) + l7 * b3;
            PW(PN_QA + 4 * i + 2) = ((l3 * b0 + l4 * b1) + 2.0 * l5 * b2) + l8 * b3;
            PW(PN_QA + 4 * i + 3) = ((l6 * b0 + l7 * b1) + l8 * b2) + 2.0 * l9 * b3;
            PW(PN_QB + i) = PW(PN_RHO + i) - (((((((((l0 * b0 * b0 + l1 * b0 * b1) + l2 * b1 * b1) + l3 * b0 * b2) + l4 * b1 * b2) +
                                                  l5 * b2 * b2) + l6 * b0 * b3) + l7 * b1 * b3) + l8 * b2 * b3) + l9 * b3 * b3);
        }
        if (!qr_solve(w, s, 6, 4)) return false;
        for (int k = 0; k < 4; ++k) PW(PN_BETA + k) = PW(PN_BETA + k) + PW(PN_X + k);
    }
    return true;
}

// compute_R_and_t from PN_BETA -> pose (12) and rep_error at PN_RES + 13 * which; the error is +inf when a value
// of the result is not finite
PN_HD void r_and_t(double* w, int s, int which) {
    const double b0 = PW(PN_BETA), b1 = PW(PN_BETA + 1), b2 = PW(PN_BETA + 2), b3 = PW(PN_BETA + 3);
    for (int j = 0; j < 4; ++j)
        for (int k = 0; k < 3; ++k) {
            const int e = 3 * j + k;
            PW(PN_CCS + e) = ((b0 * PW(PN_V + e) + b1 * PW(PN_V + 12 + e)) + b2 * PW(PN_V + 24 + e)) + b3 * PW(PN_V + 36 + e);
        }
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 3; ++j)
            PW(PN_PCS + 3 * i + j) = ((PW(PN_AL + 4 * i) * PW(PN_CCS + j) + PW(PN_AL + 4 * i + 1) * PW(PN_CCS + 3 + j)) +
                                      PW(PN_AL + 4 * i + 2) * PW(PN_CCS + 6 + j)) + PW(PN_AL + 4 * i + 3) * PW(PN_CCS + 9 + j);
    if (PW(PN_PCS + 2) < 0.0)
        for (int e = 0; e < 15; ++e) PW(PN_PCS + e) = -PW(PN_PCS + e);
    for (int j = 0; j < 3; ++j)
        PW(PN_PC0 + j) = ((((PW(PN_PCS + j) + PW(PN_PCS + 3 + j)) + PW(PN_PCS + 6 + j)) + PW(PN_PCS + 9 + j)) + PW(PN_PCS + 12 + j)) / 5.0;
    for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k) {
            double sm = 0.0;
            for (int i = 0; i < 5; ++i) sm = sm + (PW(PN_PCS + 3 * i + j) - PW(PN_PC0 + j)) * PW(PN_D + 3 * i + k);
            PW(PN_ABT + 3 * j + k) = sm;
        }
    svd3_full(w, s);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            PW(PN_R + 3 * i + j) = (PW(PN_SU + 3 * i) * PW(PN_SV + j) + PW(PN_SU + 3 * i + 1) * PW(PN_SV + 3 + j)) +
                                   PW(PN_SU + 3 * i + 2) * PW(PN_SV + 6 + j);
    if (wdet3(w, s, PN_R) < 0)
        for (int j = 0; j < 3; ++j) PW(PN_R + 6 + j) = -PW(PN_R + 6 + j);
    for (int i = 0; i < 3; ++i) PW(PN_TT + i) = PW(PN_PC0 + i) - wdot3(w, s, PN_R + 3 * i, PN_CWS);
    double sm = 0.0;
    for (int i = 0; i < 5; ++i) {
        const double iz = 1.0 / (wdot3(w, s, PN_R + 6, PN_PW + 3 * i) + PW(PN_TT + 2));
        const double du = PW(PN_UV + 2 * i) - (wdot3(w, s, PN_R, PN_PW + 3 * i) + PW(PN_TT)) * iz;
        const double dv = PW(PN_UV + 2 * i + 1) - (wdot3(w, s, PN_R + 3, PN_PW + 3 * i) + PW(PN_TT + 1)) * iz;
        sm = sm + sqrt(du * du + dv * dv);
    }
    const double err = sm / 5.0;
    const int o = PN_RES + 13 * which;
    bool ok = finite_d(err);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            const double v = PW(PN_R + 3 * i + j);
            PW(o + 4 * i + j) = v;
            ok = ok && finite_d(v);
        }
        const double v = PW(PN_TT + i);
        PW(o + 4 * i + 3) = v;
        ok = ok && finite_d(v);
    }
    PW(o + 12) = ok ? err : HUGE_VAL;
}

// epnp::compute_pose on the five points at PN_PW (5 x 3) and PN_UV (5 x 2, normalised): 0 when there is no
// model, else N = 1, 2, 3, the chosen approximation, whose pose (hconcat(R, t), row-major) is at
// w[(PN_RES + 13 (N - 1) + e) * s], e < 12, followed by its rep_error.
PN_HD int epnp5(double* w, int s) {
    bool full = true;   // the sample has extent in all three directions
    // ---- control points: the centroid and the principal directions of PW0^T PW0
    for (int j = 0; j < 3; ++j)
        PW(PN_CWS + j) = ((((PW(PN_PW + j) + PW(PN_PW + 3 + j)) + PW(PN_PW + 6 + j)) + PW(PN_PW + 9 + j)) + PW(PN_PW + 12 + j)) / 5.0;
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 3; ++j) PW(PN_D + 3 * i + j) = PW(PN_PW + 3 * i + j) - PW(PN_CWS + j);
    {
        int o = PN_S3;
        for (int a = 0; a < 3; ++a)
            for (int b = a; b < 3; ++b) {
                double sm = 0.0;
                for (int i = 0; i < 5; ++i) sm = sm + PW(PN_D + 3 * i + a) * PW(PN_D + 3 * i + b);
                PW(o++) = sm;
            }
    }
    jacobi_eig(w, s, PN_S3, PN_V3, 3);
    // The control matrix has the columns k_m v_m with orthonormal v_m, so row m of its (pseudo-)inverse is v_m / k_m;
    // a direction whose eigenvalue is not above PLANE_EPS times the largest (a coplanar or collinear sample) is
    // truncated: its control point is the centroid and its row is zero.
    {
        int used = 0;
        double lam0 = 0.0;
        for (int m = 0; m < 3; ++m) {   // descending; the first largest wins, a NaN never does
            double best = -HUGE_VAL;
            int bi = -1;
            for (int i = 0; i < 3; ++i) {
                const double lam = PW(PN_S3 + si(3, i, i));
                if (!((used >> i) & 1) && lam > best) { best = lam; bi = i; }
            }
            if (bi < 0) return 0;
            used |= 1 << bi;
            if (m == 0) lam0 = best;
            const double k = sqrt(best / 5.0);
            const bool keep = best > PLANE_EPS * lam0;
            if (m == 2) full = keep;
            for (int j = 0; j < 3; ++j) {
                const double v = PW(PN_V3 + 3 * bi + j);
                PW(PN_CWS + 3 * (m + 1) + j) = keep ? PW(PN_CWS + j) + k * v : PW(PN_CWS + j);
                PW(PN_CI + 3 * m + j) = keep ? v / k : 0.0;
            }
        }
        for (int i = 0; i < 5; ++i) {
            const double a0 = wdot3(w, s, PN_CI, PN_D + 3 * i), a1 = wdot3(w, s, PN_CI + 3, PN_D + 3 * i),
                         a2 = wdot3(w, s, PN_CI + 6, PN_D + 3 * i);
            PW(PN_AL + 4 * i) = ((1.0 - a0) - a1) - a2;
            PW(PN_AL + 4 * i + 1) = a0; PW(PN_AL + 4 * i + 2) = a1; PW(PN_AL + 4 * i + 3) = a2;
        }
    }
    // ---- M (fill_M with fu = fv = 1, uc = vc = 0), M^T M and its four eigenvectors of smallest eigenvalue
    {
        const int M = PN_VT;
        for (int i = 0; i < 5; ++i)
            for (int k = 0; k < 4; ++k) {
                const double a = PW(PN_AL + 4 * i + k);
                PW(M + 24 * i + 3 * k) = a;      PW(M + 24 * i + 3 * k + 1) = 0.0; PW(M + 24 * i + 3 * k + 2) = a * (0.0 - PW(PN_UV + 2 * i));
                PW(M + 24 * i + 12 + 3 * k) = 0.0; PW(M + 24 * i + 12 + 3 * k + 1) = a; PW(M + 24 * i + 12 + 3 * k + 2) = a * (0.0 - PW(PN_UV + 2 * i + 1));
            }
        int o = PN_MTM;
        for (int a = 0; a < 12; ++a)
            for (int b = a; b < 12; ++b) {
                double sm = 0.0;
                for (int r = 0; r < 10; ++r) sm = sm + PW(M + 12 * r + a) * PW(M + 12 * r + b);
                PW(o++) = sm;
            }
    }
    jacobi_eig(w, s, PN_MTM, PN_VT, 12);
    {
        int used = 0;
        // A coplanar sample has three control points: the fourth's columns of M are exactly zero, the rotations never
        // touch them, and its unit eigenvectors (indices 9-11) are left out.
        for (int m = 0; m < 4; ++m) {   // ascending; the first smallest wins
            double best = HUGE_VAL;
            int bi = -1;
            for (int i = 0; i < (full ? 12 : 9); ++i) {
                const double lam = PW(PN_MTM + si(12, i, i));
                if (!((used >> i) & 1) && lam < best) { best = lam; bi = i; }
            }
            if (bi < 0) return 0;
            used |= 1 << bi;
            for (int k = 0; k < 12; ++k) PW(PN_V + 12 * m + k) = PW(PN_VT + 12 * bi + k);
        }
    }
    // ---- rho and L_6x10 (phase 2: the eigen-solver's space is free)
    for (int r = 0; r < 6; ++r) {
        const int a = r < 3 ? 0 : (r < 5 ? 1 : 2), b = r < 3 ? r + 1 : (r < 5 ? r - 1 : 3);
        const double x = PW(PN_CWS + 3 * a) - PW(PN_CWS + 3 * b), y = PW(PN_CWS + 3 * a + 1) - PW(PN_CWS + 3 * b + 1),
                     z = PW(PN_CWS + 3 * a + 2) - PW(PN_CWS + 3 * b + 2);
        PW(PN_RHO + r) = (x * x + y * y) + z * z;
        // dv[i] = v[i][3a..] - v[i][3b..] at PN_QA (4 x 3)
        for (int i = 0; i < 4; ++i)
            for (int k = 0; k < 3; ++k) PW(PN_QA + 3 * i + k) = PW(PN_V + 12 * i + 3 * a + k) - PW(PN_V + 12 * i + 3 * b + k);
        const int d0 = PN_QA, d1 = PN_QA + 3, d2 = PN_QA + 6, d3 = PN_QA + 9, l = PN_L + 10 * r;
        PW(l + 0) = wdot3(w, s, d0, d0);
        PW(l + 1) = 2.0 * wdot3(w, s, d0, d1);
        PW(l + 2) = wdot3(w, s, d1, d1);
        PW(l + 3) = 2.0 * wdot3(w, s, d0, d2);
        PW(l + 4) = 2.0 * wdot3(w, s, d1, d2);
        PW(l + 5) = wdot3(w, s, d2, d2);
        PW(l + 6) = 2.0 * wdot3(w, s, d0, d3);
        PW(l + 7) = 2.0 * wdot3(w, s, d1, d3);
        PW(l + 8) = 2.0 * wdot3(w, s, d2, d3);
        PW(l + 9) = wdot3(w, s, d3, d3);
    }
    // ---- the three approximations, five Gauss-Newton steps each, and the rep_errors cascade
    for (int which = 0; which < 3; ++which) {
        bool ok;
        if (full) ok = betas_approx(w, s, which) && gauss_newton(w, s);
        else {
            ok = which == 0;
            if (ok) {   // EPnP's case N = 1 on the three control points that span the plane
                double num = 0.0, den = 0.0;
                for (int r = 0; r < 4; ++r) {
                    if (r == 2) continue;   // pairs (0, 1), (0, 2), (1, 2)
                    const int a = r < 3 ? 0 : 1, b = r < 3 ? r + 1 : 2;
                    const double x = PW(PN_V + 3 * a) - PW(PN_V + 3 * b), y = PW(PN_V + 3 * a + 1) - PW(PN_V + 3 * b + 1),
                                 z = PW(PN_V + 3 * a + 2) - PW(PN_V + 3 * b + 2);
                    const double q = (x * x + y * y) + z * z;
                    num = num + sqrt(q) * sqrt(PW(PN_RHO + r));
                    den = den + q;
                }
                PW(PN_BETA) = num / den; PW(PN_BETA + 1) = 0.0; PW(PN_BETA + 2) = 0.0; PW(PN_BETA + 3) = 0.0;
            }
        }
        if (ok) r_and_t(w, s, which);
        else PW(PN_RES + 13 * which + 12) = HUGE_VAL;
    }
    int N = 0;
    if (PW(PN_RES + 13 + 12) < PW(PN_RES + 12)) N = 1;
    if (PW(PN_RES + 26 + 12) < PW(PN_RES + 13 * N + 12)) N = 2;
    if (!(PW(PN_RES + 13 * N + 12) < HUGE_VAL)) return 0;
    return N + 1;
}
#undef PW

struct CamP {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

// cv::undistortPoints, TermCriteria(COUNT, 5), result rounded to float (the undistort of csrc/triangulate.hip)
PN_HD void undistort_f(float px, float py, const CamP& S, float& ox, float& oy) {
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

// PnPRansacCallback::computeError of one point: cv::projectPoints of the float 3-D point under P = hconcat(R, t)
// (double, rounded to float; the projection of csrc/triangulate.hip), then the float squared distance to the float
// image point.
PN_HD float reprojection_error(const double* P, float Xf, float Yf, float Zf, float u0, float v0, const CamP& S) {
    const double X = (double)Xf, Y = (double)Yf, Z = (double)Zf;
    double x = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3];
    double y = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7];
    double z = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11];
    z = z != 0 ? 1.0 / z : 1.0;
    x = x * z;
    y = y * z;
    const double r2 = x * x + y * y;
    const double r4 = r2 * r2;
    const double r6 = r4 * r2;
    const double a1 = 2.0 * x * y;
    const double a2 = r2 + 2.0 * x * x;
    const double a3 = r2 + 2.0 * y * y;
    const double cdist = ((1.0 + S.k1 * r2) + S.k2 * r4) + S.k3 * r6;
    const double xd = (x * cdist + S.p1 * a1) + S.p2 * a2;
    const double yd = (y * cdist + S.p1 * a3) + S.p2 * a1;
    const float u = (float)(xd * S.fx + S.cx);
    const float v = (float)(yd * S.fy + S.cy);
    const float du = u - u0, dv = v - v0;
    return du * du + dv * dv;
}


// ---- the refit: solvePnP(SOLVEPNP_ITERATIVE) on the inliers (tests/pnp_ref.py, last section).  sin, cos and acos
// come from libm here, so the refit's pose is compared within a tolerance and not as bits.

// cvUndistortPoints into CV_64F: undistort_f without the rounding to float
PN_HD void undistort_d(float px, float py, const CamP& S, double& ox, double& oy) {
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
    ox = x;
    oy = y;
}

PN_HD double eye9(int k) { return (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0; }
// d [r]x / d r_i, row-major
PN_HD double gen9(int i, int k) {
    if (i == 0) return k == 5 ? -1.0 : (k == 7 ? 1.0 : 0.0);
    if (i == 1) return k == 2 ? 1.0 : (k == 6 ? -1.0 : 0.0);
    return k == 1 ? -1.0 : (k == 3 ? 1.0 : 0.0);
}

// cvRodrigues2, vector -> matrix with its Jacobian: R (9) and dR (3 x 9) are written through the pointers
PN_HD void rodrigues(double r0, double r1, double r2, double* R, double* dR) {
    const double theta = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
    if (!(theta >= 2.220446049250313e-16)) {
        for (int k = 0; k < 9; ++k) {
            R[k] = eye9(k);
            for (int i = 0; i < 3; ++i) dR[9 * i + k] = gen9(i, k);
        }
        return;
    }
    const double c = cos(theta), sn = sin(theta);
    const double c1 = 1.0 - c, it = 1.0 / theta;
    const double x = r0 * it, y = r1 * it, z = r2 * it;
    for (int k = 0; k < 9; ++k) {
        const int a = k / 3, b = k % 3;
        const double va = a == 0 ? x : (a == 1 ? y : z), vb = b == 0 ? x : (b == 1 ? y : z);
        const double rrt = a <= b ? va * vb : vb * va;
        const double rx = x * gen9(0, k) + y * gen9(1, k) + z * gen9(2, k);   // one non-zero term: exact
        R[k] = (c * eye9(k) + c1 * rrt) + sn * rx;
        for (int i = 0; i < 3; ++i) {
            const double ri = i == 0 ? x : (i == 1 ? y : z);
            // d (r r^T)[a][b] / d r_i = (a == i) r_b + (b == i) r_a
            const double drrt = (a == i && b == i) ? ri + ri : (a == i ? vb : (b == i ? va : 0.0));
            const double a0 = -sn * ri, a1 = (sn - 2.0 * c1 * it) * ri, a2 = c1 * it, a3 = (c - sn * it) * ri, a4 = sn * it;
            dR[9 * i + k] = (((a0 * eye9(k) + a1 * rrt) + a2 * drrt) + a3 * rx) + a4 * gen9(i, k);
        }
    }
}

// cvRodrigues2, matrix -> vector (without its re-orthonormalisation)
PN_HD void rodrigues_inv(const double* R, double* r) {
    double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    const double sn = sqrt(((rx * rx + ry * ry) + rz * rz) * 0.25);
    double c = ((R[0] + R[4]) + R[8] - 1.0) * 0.5;
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    double theta = acos(c);
    if (sn < 1e-5) {
        if (c > 0) { r[0] = 0.0; r[1] = 0.0; r[2] = 0.0; return; }
        double t = (R[0] + 1.0) * 0.5;
        rx = sqrt(t > 0.0 ? t : 0.0);
        t = (R[4] + 1.0) * 0.5;
        ry = sqrt(t > 0.0 ? t : 0.0) * (R[1] < 0 ? -1.0 : 1.0);
        t = (R[8] + 1.0) * 0.5;
        rz = sqrt(t > 0.0 ? t : 0.0) * (R[2] < 0 ? -1.0 : 1.0);
        if (fabs(rx) < fabs(ry) && fabs(rx) < fabs(rz) && (R[5] > 0) != (ry * rz > 0)) rz = -rz;
        theta = theta / sqrt((rx * rx + ry * ry) + rz * rz);
        r[0] = rx * theta; r[1] = ry * theta; r[2] = rz * theta;
        return;
    }
    const double vth = (1.0 / (2.0 * sn)) * theta;
    r[0] = rx * vth; r[1] = ry * vth; r[2] = rz * vth;
}

// One point's terms of cvProjectPoints2 with dp/dr, dp/dt: the 28 sums' addends (JtJ upper triangle 21, JtErr 6,
// |err|^2) are added into acc[k * stride].  R (9), dR (27), t (3); the point as float-rounded doubles, the image
// point as the float's double.
PN_HD void refit_terms(const double* R, const double* dR, const double* t, double X0, double X1, double X2, double pu,
                       double pv, const CamP& S, double* acc, int stride) {
    const double X = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + t[0];
    const double Y = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + t[1];
    const double Z = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + t[2];
    const double z = Z != 0 ? 1.0 / Z : 1.0;
    const double x = X * z, y = Y * z;
    const double r2 = x * x + y * y;
    const double r4 = r2 * r2;
    const double r6 = r4 * r2;
    const double a1 = 2.0 * x * y;
    const double a2 = r2 + 2.0 * x * x;
    const double a3 = r2 + 2.0 * y * y;
    const double cdist = ((1.0 + S.k1 * r2) + S.k2 * r4) + S.k3 * r6;
    const double xd = (x * cdist + S.p1 * a1) + S.p2 * a2;
    const double yd = (y * cdist + S.p1 * a3) + S.p2 * a1;
    const double eu = (xd * S.fx + S.cx) - pu;
    const double ev = (yd * S.fy + S.cy) - pv;
    const double dcd = (S.k1 + 2.0 * S.k2 * r2) + 3.0 * S.k3 * r4;
    const double xdx = ((cdist + 2.0 * x * x * dcd) + 2.0 * S.p1 * y) + 6.0 * S.p2 * x;
    const double xdy = (2.0 * x * y * dcd + 2.0 * S.p1 * x) + 2.0 * S.p2 * y;
    const double ydx = (2.0 * x * y * dcd + 2.0 * S.p1 * x) + 2.0 * S.p2 * y;
    const double ydy = ((cdist + 2.0 * y * y * dcd) + 6.0 * S.p1 * y) + 2.0 * S.p2 * x;
    const double xz = -(x * z), yz = -(y * z);
    double Ju[6], Jv[6];
    Ju[3] = S.fx * (xdx * z); Ju[4] = S.fx * (xdy * z); Ju[5] = S.fx * (xdx * xz + xdy * yz);
    Jv[3] = S.fy * (ydx * z); Jv[4] = S.fy * (ydy * z); Jv[5] = S.fy * (ydx * xz + ydy * yz);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 3; ++i) {
        const double* D = dR + 9 * i;
        const double q0 = (D[0] * X0 + D[1] * X1) + D[2] * X2;
        const double q1 = (D[3] * X0 + D[4] * X1) + D[5] * X2;
        const double q2 = (D[6] * X0 + D[7] * X1) + D[8] * X2;
        Ju[i] = (Ju[3] * q0 + Ju[4] * q1) + Ju[5] * q2;
        Jv[i] = (Jv[3] * q0 + Jv[4] * q1) + Jv[5] * q2;
    }
    int k = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int a = 0; a < 6; ++a) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int b = a; b < 6; ++b) {
            acc[k * stride] = acc[k * stride] + (Ju[a] * Ju[b] + Jv[a] * Jv[b]);
            ++k;
        }
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int a = 0; a < 6; ++a) acc[(21 + a) * stride] = acc[(21 + a) * stride] + (Ju[a] * eu + Jv[a] * ev);
    acc[27 * stride] = acc[27 * stride] + (eu * eu + ev * ev);
}

#define PW(i) w[(i) * s]
// The planarity test of cvFindExtrinsicCameraParams2 on the packed 3 x 3 covariance at PN_S3 (overwritten): its
// eigenvalues descending, W[2] / W[1] < 1e-3; a NaN eigenvalue is not planar.
PN_HD bool planar_cov(double* w, int s) {
    jacobi_eig(w, s, PN_S3, PN_V3, 3);
    double w0 = PW(PN_S3), w1 = PW(PN_S3 + 3), w2 = PW(PN_S3 + 5);
    if (!(w0 == w0 && w1 == w1 && w2 == w2)) return false;
    double t;
    if (w0 < w1) { t = w0; w0 = w1; w1 = t; }
    if (w1 < w2) { t = w1; w1 = w2; w2 = t; }
    if (w0 < w1) { t = w0; w0 = w1; w1 = t; }
    return w2 / w1 < 1e-3;
}

// The DLT start of cvFindExtrinsicCameraParams2 from the packed 12 x 12 L^T L at PN_MTM (overwritten): the
// eigenvector of the smallest eigenvalue (the first smallest, a NaN never) as 3 x 4, negated when the determinant
// of its 3 x 3 part is negative, R = U V^T of that part's SVD, t scaled by |R|_F / |RR|_F.  R (9) and t (3) are
// written through the pointers; false when there is no eigenvalue or a value is not finite.  No libm but sqrt.
PN_HD bool dlt_start(double* w, int s, double* R, double* t) {
    jacobi_eig(w, s, PN_MTM, PN_VT, 12);
    double best = HUGE_VAL;
    int bi = -1;
    for (int i = 0; i < 12; ++i) {
        const double lam = PW(PN_MTM + si(12, i, i));
        if (lam < best) { best = lam; bi = i; }
    }
    if (bi < 0) return false;
    for (int k = 0; k < 12; ++k) PW(PN_V + k) = PW(PN_VT + 12 * bi + k);   // (PN_V is outside the SVD's space)
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) PW(PN_ABT + 3 * i + j) = PW(PN_V + 4 * i + j);
    if (wdet3(w, s, PN_ABT) < 0) {
        for (int k = 0; k < 12; ++k) PW(PN_V + k) = -PW(PN_V + k);
        for (int k = 0; k < 9; ++k) PW(PN_ABT + k) = -PW(PN_ABT + k);
    }
    double nrr = 0.0;
    for (int k = 0; k < 9; ++k) nrr = nrr + PW(PN_ABT + k) * PW(PN_ABT + k);
    svd3_full(w, s);
    double nr = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double v = (PW(PN_SU + 3 * i) * PW(PN_SV + j) + PW(PN_SU + 3 * i + 1) * PW(PN_SV + 3 + j)) +
                             PW(PN_SU + 3 * i + 2) * PW(PN_SV + 6 + j);
            R[3 * i + j] = v;
            nr = nr + v * v;
        }
    const double sc = sqrt(nr) / sqrt(nrr);
    bool ok = true;
    for (int i = 0; i < 3; ++i) t[i] = PW(PN_V + 4 * i + 3) * sc;
    for (int k = 0; k < 9; ++k) ok = ok && finite_d(R[k]);
    for (int k = 0; k < 3; ++k) ok = ok && finite_d(t[k]);
    return ok;
}
#undef PW

// Gaussian elimination with partial pivoting of the 6 x 6 system in A (6 rows of 7: the right side last) -> x;
// false on a zero pivot
PN_HD bool solve6(double* A, double* x) {
    for (int k = 0; k < 6; ++k) {
        double best = 0.0;
        int pr = -1;
        for (int r = k; r < 6; ++r) {
            const double v = fabs(A[7 * r + k]);
            if (v > best) { best = v; pr = r; }
        }
        if (pr < 0) return false;
        if (pr != k)
            for (int c = 0; c < 7; ++c) { const double t = A[7 * k + c]; A[7 * k + c] = A[7 * pr + c]; A[7 * pr + c] = t; }
        for (int r = k + 1; r < 6; ++r) {
            const double f = A[7 * r + k] / A[7 * k + k];
            for (int c = k + 1; c < 7; ++c) A[7 * r + c] = A[7 * r + c] - f * A[7 * k + c];
        }
    }
    for (int i = 5; i >= 0; --i) {
        double sm = A[7 * i + 6];
        for (int j = i + 1; j < 6; ++j) sm = sm - A[7 * i + j] * x[j];
        x[i] = sm / A[7 * i + i];
    }
    return true;
}

// 10^k, k in [-16, 16], as the literals' doubles
PN_HD double pow10i(int k) {
    switch (k) {
        case -16: return 1e-16; case -15: return 1e-15; case -14: return 1e-14; case -13: return 1e-13;
        case -12: return 1e-12; case -11: return 1e-11; case -10: return 1e-10; case -9: return 1e-9;
        case -8: return 1e-8; case -7: return 1e-7; case -6: return 1e-6; case -5: return 1e-5;
        case -4: return 1e-4; case -3: return 1e-3; case -2: return 1e-2; case -1: return 1e-1;
        case 0: return 1e0; case 1: return 1e1; case 2: return 1e2; case 3: return 1e3; case 4: return 1e4;
        case 5: return 1e5; case 6: return 1e6; case 7: return 1e7; case 8: return 1e8; case 9: return 1e9;
        case 10: return 1e10; case 11: return 1e11; case 12: return 1e12; case 13: return 1e13;
        case 14: return 1e14; case 15: return 1e15; default: return 1e16;
    }
}

}  // namespace pnpm
}  // namespace sfmx
