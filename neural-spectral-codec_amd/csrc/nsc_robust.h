// nsc_robust.h -- the scalar robust kernel that nsc_posegraph.hip (per edge) and nsc_localize.hip (per row and voxel)
// share: (kernel, width c, s = r^T Omega r) -> rho(s) and the IRLS weight w = rho'(s).  include/nsc.h has the table; the
// kernel numbers are NSC_POSEGRAPH_KERNEL_* = NSC_MAP_KERNEL_*.  Included at file scope; the namespace below gives each
// file its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/nsc.h"

namespace {

struct Robust {
    double rho, w;
};

// The term is quadratic, rho = s and w = 1 exactly, for kernel NONE, for a width c that is not finite and positive or
// whose square is not, and for s <= 0 or NaN.
__device__ __forceinline__ Robust robust_rho_w(int kernel, double c, double s)
{
    Robust out{s, 1.0};
    if (kernel == NSC_POSEGRAPH_KERNEL_NONE) return out;
    const double c2 = c * c;
    if (!(c > 0.0) || !(c2 > 0.0) || !isfinite(c2) || !(s > 0.0)) return out;
    if (kernel == NSC_POSEGRAPH_KERNEL_HUBER) {
        if (s > c2) {
            const double q = sqrt(s);
            out.rho = 2.0 * c * q - c2;
            out.w = c / q;
        }
    } else if (kernel == NSC_POSEGRAPH_KERNEL_CAUCHY) {
        const double u = s / c2;
        out.rho = c2 * log1p(u);
        out.w = 1.0 / (1.0 + u);
    } else {                                 // Geman-McClure
        const double t = c2 / (c2 + s);
        out.rho = t * s;
        out.w = t * t;
    }
    return out;
}

}  // namespace
