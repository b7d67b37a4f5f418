// nsc_gauss_newton.h -- the end of a Gauss-Newton round over a rigid transform that the finalize kernels of
// nsc_geometry.hip (GICP) and nsc_localize.hip (scan to map) share: the 6x6 system by Cholesky and T <- dT T with dT from
// three small angles (rotation first) and a translation.  Included at file scope; the namespace below gives each file its
// own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace {

__device__ void rot_zyx(double a, double b, double g, double R[3][3])
{
    const double ca = cos(a), sa = sin(a), cb = cos(b), sb = sin(b), cg = cos(g), sg = sin(g);
    // Rz(g) Ry(b) Rx(a)
    R[0][0] = cg * cb; R[0][1] = cg * sb * sa - sg * ca; R[0][2] = cg * sb * ca + sg * sa;
    R[1][0] = sg * cb; R[1][1] = sg * sb * sa + cg * ca; R[1][2] = sg * sb * ca - cg * sa;
    R[2][0] = -sb;     R[2][1] = cb * sa;                R[2][2] = cb * ca;
}

// A pivot d_j of the factorisation below counts as positive only above GN_PIVOT_TAU times H[j][j], the original diagonal
// term.  For a rank-deficient H (one or two source rows, collinear rows: a rotation the data says nothing about) d_j is
// zero in exact arithmetic and rounding alone decides d_j > 0.  Measured in float64 in this pivot order
// (tests/test_registration_degenerate_cpu.py, test_thresholds, which measures again and asserts both margins):
//   (a) 4.7e-12  the largest |d_j| / H[j][j] at the rejecting or last pivot over the systems that are singular by
//                construction (tests/registration_degenerate_cases.py) and the singular ones of many_small
//   (b) 3.2e-6   the smallest d_j / H[j][j] over every regular system the suite has, at every round (a 40-row line and
//                one row 0.1 m off it)
// and GN_PIVOT_TAU is their geometric mean: (a) < tau / 100, (b) > 100 tau.
constexpr double GN_PIVOT_TAU = 3.9e-9;

// H x = -g by Cholesky, H the 21 upper-triangle terms sys[0..20] (row by row) and g = sys[21..26]; false, and x
// untouched, without an H that is positive definite by the pivot test above
__device__ bool gn_solve6(const double *sys, double x[6])
{
    double L[6][6];
    {
        int t = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) { L[b][a] = sys[t]; ++t; }         // lower triangle of the symmetric H
    }
    for (int j = 0; j < 6; ++j) {
        const double hjj = L[j][j];                                       // still H[j][j]
        double dj = hjj;
        for (int k = 0; k < j; ++k) dj -= L[j][k] * L[j][k];
        if (!(dj > GN_PIVOT_TAU * hjj) || !isfinite(dj)) return false;
        L[j][j] = sqrt(dj);
        for (int i = j + 1; i < 6; ++i) {
            double v = L[i][j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    for (int i = 0; i < 6; ++i) {                                         // L y = -g
        double v = -sys[21 + i];
        for (int k = 0; k < i; ++k) v -= L[i][k] * x[k];
        x[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {                                        // L^T x = y
        double v = x[i];
        for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
        x[i] = v / L[i][i];
    }
    return true;
}

// rows 0..2 of the row-major 4x4 T <- dT T, dT = [rot_zyx(x[0], x[1], x[2]) | x[3..5]]
__device__ void gn_apply(const double x[6], double *T)
{
    double dR[3][3], N[12];
    rot_zyx(x[0], x[1], x[2], dR);
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 4; ++b)
            N[4 * a + b] = dR[a][0] * T[b] + dR[a][1] * T[4 + b] + dR[a][2] * T[8 + b] + (b == 3 ? x[3 + a] : 0.0);
    for (int e = 0; e < 12; ++e) T[e] = N[e];
}

}  // namespace
