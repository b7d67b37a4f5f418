"""Float64 restatement of the two-level preconditioner of csrc/nsc_posegraph.hip (contract: include/nsc.h,
nsc_posegraph_optimize_coarse), on top of posegraph_restatement and posegraph_robust_restatement: the same residuals,
Jacobians, robust weights, Levenberg-Marquardt and PCG rules, with H kept sparse (scipy.sparse) so that graphs of a
thousand poses can be restated.

    aggregates      pose k belongs to a(k) = k // L;  n_a = ceil(N / L)
    prolongation    P (6N, 6 n_a): block (k, a(k)) = Ad(X_k^-1 X_ref) for a free pose k, X_ref = X_{a(k) L}; zero rows for
                    poses that are not free (fixed, without a counted edge, or with a block that is not positive definite)
    coarse matrix   A_c = P^T (H + lambda diag H) P, the identity block for an aggregate without a free pose
    preconditioner  M^-1 r = B^-1 r + P A_c^-1 P^T r,  B^-1 the per-node solve with the damped 6 x 6 diagonal block
    failure         a Cholesky factor of A_c that does not exist leaves the outer step with B^-1 alone, and is counted

``L=None`` everywhere is block-Jacobi alone: posegraph_restatement.pcg_step on a sparse H.
"""
import numpy as np
import scipy.sparse as sp

import posegraph_restatement as P
import posegraph_robust_restatement as R


def linearize(poses, edge_ij, Z, Om, kernel=R.NONE, scale=None):
    """-> dict(H (6N,6N) csr, gradient (N,6), blocks (N,6,6), cost, weights (E,)) of the weighted system"""
    poses = np.asarray(poses, np.float64)
    n = len(poses)
    e = np.asarray(edge_ij, np.int64).reshape(-1, 2)
    ok = P.valid_edges(n, e)
    g = np.zeros((n, 6))
    blocks = np.zeros((n, 6, 6))
    wts = np.zeros(len(e))
    data, rows, cols = [], [], []
    F = 0.0
    for k in np.nonzero(ok)[0]:
        i, j = e[k]
        r, Ji, Jj = P.edge_terms(poses[i], poses[j], Z[k])
        W = P.sym_upper(Om[k])
        rho, w = R.rho_w(kernel, None if scale is None else scale[k], r @ W @ r)
        wts[k] = w
        W = w * W
        F += rho
        g[i] += Ji.T @ W @ r
        g[j] += Jj.T @ W @ r
        blocks[i] += Ji.T @ W @ Ji
        blocks[j] += Jj.T @ W @ Jj
        Hij = Ji.T @ W @ Jj
        data += [Hij, Hij.T]
        rows += [i, j]
        cols += [j, i]
    data += list(blocks)
    rows += list(range(n))
    cols += list(range(n))
    idx = np.arange(6)
    rr = np.concatenate([np.repeat(6 * a + idx, 6) for a in rows]) if rows else np.zeros(0, np.int64)
    cc = np.concatenate([np.tile(6 * b + idx, 6) for b in cols]) if cols else np.zeros(0, np.int64)
    vv = np.concatenate([d.reshape(-1) for d in data]) if data else np.zeros(0)
    H = sp.coo_matrix((vv, (rr, cc)), shape=(6 * n, 6 * n)).tocsr()            # duplicate entries are summed
    return dict(H=H, gradient=g, blocks=blocks, cost=F, weights=wts)


def free_nodes(n, edge_ij, fixed, blocks=None, lam=0.0):
    """posegraph_restatement.free_nodes, and with ``blocks`` also: the damped diagonal block is positive definite"""
    free = P.free_nodes(n, edge_ij, fixed)
    if blocks is not None:
        for k in np.nonzero(free)[0]:
            D = blocks[k] + lam * np.diag(np.diag(blocks[k]))
            try:
                np.linalg.cholesky(D)
            except np.linalg.LinAlgError:
                free[k] = False
    return free


def aggregates(n, L):
    return -(-n // L)


def prolongation(poses, free, L):
    """P (6N, 6 n_a) csr"""
    n = len(poses)
    idx = np.arange(6)
    rows, cols, vals = [], [], []
    for k in np.nonzero(free)[0]:
        a = k // L
        T = P.adjoint(P.inv_se3(poses[k]) @ poses[a * L])
        rows.append(np.repeat(6 * k + idx, 6))
        cols.append(np.tile(6 * a + idx, 6))
        vals.append(T.reshape(-1))
    if not rows:
        return sp.csr_matrix((6 * n, 6 * aggregates(n, L)))
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                         shape=(6 * n, 6 * aggregates(n, L))).tocsr()


def coarse_matrix(H, lam, Pm, free, L):
    """A_c = P^T (H + lambda diag H) P as a dense matrix, the identity block for an aggregate without a free pose"""
    A = H + lam * sp.diags(H.diagonal())
    Ac = (Pm.T @ (A @ Pm)).toarray()
    n_a = Ac.shape[0] // 6
    for a in range(n_a):
        if not free[a * L:(a + 1) * L].any():
            Ac[6 * a:6 * a + 6, 6 * a:6 * a + 6] = np.eye(6)
    return Ac


class Preconditioner:
    """M^-1 of the damped system at ``poses``; ``L=None``: B^-1 alone.  ``failed``: the coarse factor did not exist."""

    def __init__(self, H, blocks, lam, free, poses=None, L=None):
        n = len(free)
        inv = np.zeros((n, 6, 6))
        for k in np.nonzero(free)[0]:
            inv[k] = np.linalg.inv(blocks[k] + lam * np.diag(np.diag(blocks[k])))
        self.Binv = sp.bsr_matrix((inv, np.arange(n), np.arange(n + 1)), shape=(6 * n, 6 * n)).tocsr()
        self.Pm = self.Ac_inv = None
        self.failed = False
        if L is not None:
            self.Pm = prolongation(poses, free, L)
            self.Ac = coarse_matrix(H, lam, self.Pm, free, L)
            try:
                if not np.isfinite(self.Ac).all():
                    raise np.linalg.LinAlgError
                np.linalg.cholesky(self.Ac)
                self.Ac_inv = np.linalg.inv(self.Ac)
            except np.linalg.LinAlgError:
                self.failed = True

    def __call__(self, v):
        z = self.Binv @ v
        if self.Ac_inv is not None:
            z = z + self.Pm @ (self.Ac_inv @ (self.Pm.T @ v))
        return z

    def dense(self):
        """M^-1 as a dense matrix"""
        M = self.Binv.toarray()
        if self.Ac_inv is not None:
            Pd = self.Pm.toarray()
            M = M + Pd @ self.Ac_inv @ Pd.T
        return M


def pcg_step(H, g, blocks, lam, free, max_pcg_iterations, pcg_tolerance, poses=None, L=None):
    """posegraph_restatement.pcg_step with a sparse H and the preconditioner above -> delta (N,6), iterations, failed"""
    m = np.repeat(free, 6)
    n = len(free)
    dH = H.diagonal()
    Minv = Preconditioner(H, blocks, lam, free, poses, L)

    def A(v):
        return np.where(m, H @ v + lam * dH * v, 0.0)

    x = np.zeros(6 * n)
    r = np.where(m, -g.reshape(-1), 0.0)
    bb = r @ r
    its = 0
    if bb == 0.0:
        return x.reshape(-1, 6), 0, Minv.failed
    z = Minv(r)
    p = z.copy()
    rz = r @ z
    for _ in range(max_pcg_iterations):
        Ap = A(p)
        pAp = p @ Ap
        its += 1
        if not pAp > 0.0:
            break
        alpha = rz / pAp
        x += alpha * p
        r -= alpha * Ap
        if r @ r <= pcg_tolerance * pcg_tolerance * bb:
            break
        z = Minv(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x.reshape(-1, 6), its, Minv.failed


def dense_step(H, g, lam, free):
    return P.dense_step(H.toarray(), g, lam, free)


def optimize(poses, edge_ij, Z, Om, L=None, kernel=R.NONE, scale=None, fixed=None, **params):
    """posegraph_robust_restatement.optimize with a sparse H and the two-level preconditioner; also -> coarse_aggregates,
    coarse_failed"""
    p = dict(P.DEFAULTS, **params)
    X = np.array(poses, np.float64)
    n = len(X)
    fx = np.zeros(n, bool)
    if fixed is None:
        fx[:1] = True
    else:
        fx[:] = np.asarray(fixed, bool)
    F = R.cost(X, edge_ij, Z, Om, kernel, scale)
    out = dict(cost0=F, iterations=0, accepted=0, rejected=0, pcg_iterations=0, converged=False, step0=None,
               coarse_aggregates=0 if L is None else aggregates(n, L), coarse_failed=0, inner=[])
    hist = [F]
    lam = p["lambda0"]
    for _ in range(p["max_iteration"]):
        lin = linearize(X, edge_ij, Z, Om, kernel, scale)
        free = free_nodes(n, edge_ij, fx, lin["blocks"], lam)
        d, its, failed = pcg_step(lin["H"], lin["gradient"], lin["blocks"], lam, free, p["max_pcg_iterations"],
                                  p["pcg_tolerance"], X, L)
        if out["step0"] is None:
            out["step0"] = d.copy()
        out["pcg_iterations"] += its
        out["inner"].append(its)
        out["coarse_failed"] += int(failed)
        step = float(np.sqrt((d * d).sum()))
        cand = np.stack([P.retract(X[k], d[k]) if free[k] else X[k] for k in range(n)]) if n else X
        Fc = R.cost(cand, edge_ij, Z, Om, kernel, scale)
        out["iterations"] += 1
        stop = False
        if Fc < F:
            out["accepted"] += 1
            stop = (F - Fc) < p["relative_cost"] * F
            X, F = cand, Fc
            lam = max(lam / p["lambda_factor"], p["lambda_min"])
        else:
            out["rejected"] += 1
            lam = lam * p["lambda_factor"]
        hist.append(F)
        if stop or step < p["min_step"]:
            out["converged"] = True
            break
    hist += [F] * (p["max_iteration"] + 1 - len(hist))
    out.update(poses=X, cost=F, cost_history=np.array(hist), lam=lam)
    return out
