"""Float64 restatement of the marginal covariances of csrc/nsc_posegraph.hip (contract: include/nsc.h,
nsc_posegraph_covariance), on top of the optimiser's restatements: the same H (robust weights included), lambda = 0, the
same free poses.

    Sigma           the inverse of H restricted to the free poses, zero elsewhere: the covariance of the right
                    perturbations delta_k in X_k Exp(delta_k), rotation first, in the gauge the fixed poses set
    joint[a, b]     the block (nodes[a], nodes[b]) of Sigma, from the six columns H x = e_{6 nodes[b] + c}
    columns         each one a PCG of its own: posegraph_restatement.pcg_step (block-Jacobi) or
                    posegraph_coarse_restatement.pcg_step (two-level) with g = -e and lambda = 0
    relative        A = X_i^-1 X_j moves by delta_A = delta_j - Ad(A^-1) delta_i:  Sigma_rel = G Sigma G^T, G = [-Ad(A^-1), I]
    gate            d^2 = r^T (Omega^-1 + Sigma_rel)^-1 r, r the residual of the closure
"""
import numpy as np

import posegraph_coarse_restatement as Cr
import posegraph_restatement as P
import posegraph_robust_restatement as R

TAU = 1e-10                                  # the tolerance the device is held to
BAR = 10.0                                   # |joint - Sigma| <= BAR * TAU * |Sigma|_2 for converged columns


def first_fixed(n):
    fixed = np.zeros(n, bool)
    fixed[:1] = True
    return fixed


def system(poses, edge_ij, Z, Om, fixed=None, kernel=R.NONE, scale=None):
    """-> the weighted linearisation at ``poses`` (H sparse) and the free poses at lambda = 0"""
    n = len(poses)
    lin = Cr.linearize(poses, edge_ij, Z, Om, kernel, scale)
    free = Cr.free_nodes(n, edge_ij, first_fixed(n) if fixed is None else np.asarray(fixed, bool), lin["blocks"], 0.0)
    return lin, free


def dense_sigma(H, free):
    """Sigma (6N,6N): the inverse of the free submatrix of H, zero elsewhere"""
    m = np.repeat(np.asarray(free, bool), 6)
    S = np.zeros((len(m), len(m)))
    if m.any():
        A = H.toarray() if hasattr(H, "toarray") else np.asarray(H)
        S[np.ix_(m, m)] = np.linalg.inv(A[np.ix_(m, m)])
    return S


def joint_of(Sigma, nodes):
    """(Q,Q,6,6): the blocks of the selected poses; zero rows and columns for an index outside [0, N)"""
    n = Sigma.shape[0] // 6
    q = len(nodes)
    out = np.zeros((q, q, 6, 6))
    for a, na in enumerate(nodes):
        for b, nb in enumerate(nodes):
            if 0 <= na < n and 0 <= nb < n:
                out[a, b] = Sigma[6 * na:6 * na + 6, 6 * nb:6 * nb + 6]
    return out


def pcg_columns(lin, free, nodes, poses=None, L=None, max_pcg_iterations=1000, pcg_tolerance=TAU):
    """-> joint (Q,Q,6,6), iterations (Q,6): column by column, the optimiser's PCG with g = -e and lambda = 0"""
    n = len(free)
    q = len(nodes)
    joint, its = np.zeros((q, q, 6, 6)), np.zeros((q, 6), np.int64)
    Hd = lin["H"].toarray() if L is None else None
    for b, nb in enumerate(nodes):
        for c in range(6):
            g = np.zeros((n, 6))
            if 0 <= nb < n and free[nb]:
                g[nb, c] = -1.0
            if L is None:
                x, its[b, c] = P.pcg_step(Hd, g, 0.0, free, max_pcg_iterations, pcg_tolerance)
            else:
                x, its[b, c], failed = Cr.pcg_step(lin["H"], g, lin["blocks"], 0.0, free, max_pcg_iterations,
                                                   pcg_tolerance, poses, L)
                assert not failed
            for a, na in enumerate(nodes):
                if 0 <= na < n:
                    joint[a, b][:, c] = x[na]
    return joint, its


def local(X, Y):
    """delta with Y = retract(X, delta)"""
    return np.concatenate([P.log_so3(X[:3, :3].T @ Y[:3, :3]), X[:3, :3].T @ (Y[:3, 3] - X[:3, 3])])


def relative_jacobian(X_i, X_j):
    """G (6,12) = [-Ad(A^-1), I], A = X_i^-1 X_j"""
    A = P.inv_se3(X_i) @ X_j
    return np.concatenate([-P.adjoint(P.inv_se3(A)), np.eye(6)], axis=1)


def relative_jacobian_fd(X_i, X_j, h=1e-6):
    """the same by central differences of ``retract``: d local(A, A(delta)) / d (delta_i, delta_j)"""
    A = P.inv_se3(X_i) @ X_j
    G = np.zeros((6, 12))
    for k in range(12):
        d = np.zeros(12)
        d[k] = h
        plus = local(A, P.inv_se3(P.retract(X_i, d[:6])) @ P.retract(X_j, d[6:]))
        minus = local(A, P.inv_se3(P.retract(X_i, -d[:6])) @ P.retract(X_j, -d[6:]))
        G[:, k] = (plus - minus) / (2.0 * h)
    return G


def relative_covariance(joint_pair, X_i, X_j):
    S = np.asarray(joint_pair, np.float64).reshape(2, 2, 6, 6).transpose(0, 2, 1, 3).reshape(12, 12)
    S = 0.5 * (S + S.T)
    G = relative_jacobian(X_i, X_j)
    return G @ S @ G.T


def closure_mahalanobis(Z, Omega, X_i, X_j, sigma_rel):
    r = P.residual(X_i, X_j, Z)
    W = np.asarray(Omega, np.float64)
    return float(r @ np.linalg.solve(np.linalg.inv(0.5 * (W + W.T)) + sigma_rel, r))


# ---- graphs the tests share ------------------------------------------------------------------------------------------

def open_chain(n=257):
    """drift_ring(n) without its closure -> initial poses, edge_ij, Z, Om"""
    _, init, e, Z, Om = P.drift_ring(n)
    return init, e[:-1], Z[:-1], Om[:-1]


def two_components(n=12, m=5):
    """drift_ring(n), anchored by pose 0, and a chain of m more poses that no edge ties to it and no pose fixes: H is
    singular on that chain -> initial poses (n + m), edge_ij, Z, Om"""
    _, init, e, Z, Om = P.drift_ring(n)
    rng = np.random.default_rng(5)
    tail = P.integrate(P.noisy(P.relative(P.ring_poses(m + 1, 6.0), P.chain_edges(m + 1)), rng)[:m - 1],
                       P.make_pose([0.1, 0.0, 0.3], [40.0, 2.0, 0.0]))
    e2 = P.chain_edges(m) + n
    Z2 = P.noisy(P.relative(tail, P.chain_edges(m)), rng)
    return (np.concatenate([init, tail]), np.concatenate([e, e2]), np.concatenate([Z, Z2]),
            np.concatenate([Om, P.random_information(rng, m - 1) * 50.0]))
