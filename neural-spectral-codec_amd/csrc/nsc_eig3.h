// nsc_eig3.h -- the eigendecomposition of a symmetric 3x3 that the covariances of nsc_geometry.hip (the normal of a
// neighbourhood) and the voxel distributions of nsc_map.hip (the information matrix of a voxel) share: cyclic Jacobi in
// float64.  Included at file scope; the namespace below gives each file its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace {

// C = (xx xy xz yy yz zz)  ->  A with the eigenvalues on its diagonal, V with the eigenvectors in its columns
__device__ __forceinline__ void jacobi_eig3(const double C[6], double A[3][3], double V[3][3])
{
    A[0][0] = C[0]; A[0][1] = C[1]; A[0][2] = C[2];
    A[1][0] = C[1]; A[1][1] = C[3]; A[1][2] = C[4];
    A[2][0] = C[2]; A[2][1] = C[4]; A[2][2] = C[5];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) V[a][b] = a == b ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        const double diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (!(off > 1e-30 * diag)) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                for (int r = 0; r < 3; ++r) {            // A <- A J
                    const double arp = A[r][p], arq = A[r][q];
                    A[r][p] = cs * arp - sn * arq; A[r][q] = sn * arp + cs * arq;
                }
                for (int r = 0; r < 3; ++r) {            // A <- J^T A
                    const double apr = A[p][r], aqr = A[q][r];
                    A[p][r] = cs * apr - sn * aqr; A[q][r] = sn * apr + cs * aqr;
                }
                for (int r = 0; r < 3; ++r) {
                    const double vrp = V[r][p], vrq = V[r][q];
                    V[r][p] = cs * vrp - sn * vrq; V[r][q] = sn * vrp + cs * vrq;
                }
            }
    }
}

}  // namespace
