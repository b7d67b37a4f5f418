"""The end of a Gauss-Newton round (csrc/nsc_gauss_newton.h) restated for the references: the one written rule by which
gicp_restatement, map_localize_restatement and map_robust_restatement decide "no step", and a float64 emulation of
gn_solve6's factorisation in its own pivot order, with which tests/test_registration_degenerate_cpu.py measures the
kernel's pivot threshold.  Nothing here calls the library.

The rule does not factorise: no step when lambda_min(H) <= TAU_REF * lambda_max(H), the eigenvalues by numpy's eigvalsh.
TAU_REF is the geometric mean of two figures that tests/test_registration_degenerate_cpu.py measures again and asserts
(test_thresholds): the largest lambda_min / lambda_max of a system that is singular by construction, 1.7e-16 in magnitude
(eigvalsh's own rounding, a unit of 2^-53 of lambda_max), and the smallest of any regular system the suite has, at every
round of the references' iterations, 1.3e-13 (gicp_clouds' far-v0.5-k20: a cloud 2 km from the origin, whose rotation
terms dwarf its translation terms).  The ratio of eigenvalues depends on where the origin is, so the rule has a decade
and a half on either side and no more; gn_solve6's own test, relative to each pivot's diagonal term, does not depend on
it and has almost three (TAU_KERNEL)."""
import numpy as np

TAU_REF = 4.6e-15
# gn_solve6's relative pivot bound, the figure in the comment above it (csrc/nsc_gauss_newton.h)
TAU_KERNEL = 3.9e-9


def eig_ratio(H):
    """lambda_min / lambda_max of the symmetric H (0 for H = 0)"""
    lam = np.linalg.eigvalsh(np.asarray(H, np.float64))
    return float(lam[0] / lam[-1]) if lam[-1] > 0.0 else 0.0


def regular(H):
    """the references' rule: a step is taken exactly when this holds"""
    H = np.asarray(H, np.float64)
    if not np.isfinite(H).all():
        return False
    lam = np.linalg.eigvalsh(H)
    return bool(lam[-1] > 0.0 and lam[0] > TAU_REF * lam[-1])


def kernel_order_cholesky(H, tau=0.0):
    """gn_solve6's factorisation written out in float64, pivot by pivot in its order (rotation first, no pivoting), every
    product and difference rounded on its own.  A pivot is taken when d_j > tau * H[j][j], H[j][j] the original diagonal
    term; tau = 0 is the absolute test.  -> (accepted, j, d_j / H[j][j] there, the smallest ratio over the pivots taken):
    j is the rejecting pivot, or 5 when all six are taken."""
    H = np.asarray(H, np.float64)
    L = np.tril(H).copy()
    smallest = np.inf
    for j in range(6):
        dj = L[j, j]
        for k in range(j):
            dj -= L[j, k] * L[j, k]
        ratio = dj / H[j, j] if H[j, j] != 0.0 else 0.0
        if not (dj > tau * H[j, j]) or not np.isfinite(dj):
            return False, j, float(ratio), float(smallest)
        smallest = min(smallest, ratio)
        L[j, j] = np.sqrt(dj)
        for i in range(j + 1, 6):
            v = L[i, j]
            for k in range(j):
                v -= L[i, k] * L[j, k]
            L[i, j] = v / L[j, j]
    return True, 5, float(ratio), float(smallest)
