"""Float64 numpy restatement of the pose-graph optimiser of csrc/nsc_posegraph.hip (contract: include/nsc.h,
nsc_posegraph_optimize).  Dense H, the same Levenberg-Marquardt and PCG rules; ``dense_step`` solves the damped
system with np.linalg.solve for comparison.

    D = Z^-1 X_i^-1 X_j,  r = [Log_SO3(R_D); t_D],  F = sum r^T Omega r
    update  X_k <- [R_k Exp(phi_k) | t_k + R_k rho_k]
    J_j = B = blockdiag(Jr^-1(r_phi), R_D),  J_i = -B Ad(A^-1),  A = X_i^-1 X_j
    g = sum J^T Omega r,  H = sum J^T Omega J,  (H + lambda diag H) delta = -g
"""
import numpy as np

DEFAULTS = dict(max_iteration=20, max_pcg_iterations=100, pcg_tolerance=1e-6, lambda0=1e-4, lambda_min=1e-9,
                lambda_factor=10.0, relative_cost=1e-9, min_step=1e-9)
TRIU = np.triu_indices(6)


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def exp_so3(phi):
    phi = np.asarray(phi, np.float64)
    t2 = float(phi @ phi)
    if t2 < 1e-8:
        a, b = 1.0 - t2 / 6.0 + t2 * t2 / 120.0, 0.5 - t2 / 24.0 + t2 * t2 / 720.0
    else:
        t = np.sqrt(t2)
        a, b = np.sin(t) / t, (1.0 - np.cos(t)) / t2
    K = hat(phi)
    return np.eye(3) + a * K + b * (K @ K)


def log_so3(R):
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = float(np.linalg.norm(v))
    if s < 1e-12:
        return v
    return v * (np.arctan2(s, 0.5 * (np.trace(R) - 1.0)) / s)


def jr_inv(phi):
    t2 = float(phi @ phi)
    t = np.sqrt(t2)
    c = 1.0 / 12.0 + t2 / 720.0 if t < 1e-4 else 1.0 / t2 - (1.0 + np.cos(t)) / (2.0 * t * np.sin(t))
    K = hat(phi)
    return np.eye(3) + 0.5 * K + c * (K @ K)


def inv_se3(X):
    R, t = X[:3, :3], X[:3, 3]
    Y = np.eye(4)
    Y[:3, :3] = R.T
    Y[:3, 3] = -R.T @ t
    return Y


def adjoint(X):
    R, t = X[:3, :3], X[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = hat(t) @ R
    return A


def make_pose(phi, t):
    X = np.eye(4)
    X[:3, :3] = exp_so3(phi)
    X[:3, 3] = t
    return X


def retract(X, d):
    Y = X.copy()
    Y[:3, :3] = X[:3, :3] @ exp_so3(d[:3])
    Y[:3, 3] = X[:3, 3] + X[:3, :3] @ d[3:]
    return Y


def residual(Xi, Xj, Z):
    D = inv_se3(Z) @ inv_se3(Xi) @ Xj
    return np.concatenate([log_so3(D[:3, :3]), D[:3, 3]])


def edge_terms(Xi, Xj, Z):
    """-> r (6), J_i (6,6), J_j (6,6)"""
    A = inv_se3(Xi) @ Xj
    D = inv_se3(Z) @ A
    r = np.concatenate([log_so3(D[:3, :3]), D[:3, 3]])
    B = np.zeros((6, 6))
    B[:3, :3] = jr_inv(r[:3])
    B[3:, 3:] = D[:3, :3]
    return r, -B @ adjoint(inv_se3(A)), B


def sym_upper(Om):
    """the matrix whose upper triangle is Om's (only that is read)"""
    U = np.triu(np.asarray(Om, np.float64))
    return U + np.triu(U, 1).T


def valid_edges(n, edge_ij):
    e = np.asarray(edge_ij, np.int64).reshape(-1, 2)
    return (e[:, 0] != e[:, 1]) & (e >= 0).all(1) & (e < n).all(1)


def cost(poses, edge_ij, Z, Om):
    e = np.asarray(edge_ij, np.int64).reshape(-1, 2)
    ok = valid_edges(len(poses), e)
    F = 0.0
    for k in np.nonzero(ok)[0]:
        r = residual(poses[e[k, 0]], poses[e[k, 1]], Z[k])
        F += r @ sym_upper(Om[k]) @ r
    return F


def linearize(poses, edge_ij, Z, Om, dense=False):
    """-> dict(residuals (E,6), cost, gradient (N,6), blocks (N,21), skipped[, H (6N,6N)])"""
    poses = np.asarray(poses, np.float64)
    n = len(poses)
    e = np.asarray(edge_ij, np.int64).reshape(-1, 2)
    ok = valid_edges(n, e)
    res = np.zeros((len(e), 6))
    g = np.zeros((n, 6))
    blocks = np.zeros((n, 6, 6))
    H = np.zeros((6 * n, 6 * n)) if dense else None
    F = 0.0
    for k in np.nonzero(ok)[0]:
        i, j = e[k]
        r, Ji, Jj = edge_terms(poses[i], poses[j], Z[k])
        W = sym_upper(Om[k])
        res[k] = r
        F += r @ W @ r
        g[i] += Ji.T @ W @ r
        g[j] += Jj.T @ W @ r
        blocks[i] += Ji.T @ W @ Ji
        blocks[j] += Jj.T @ W @ Jj
        if dense:
            si, sj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
            H[si, si] += Ji.T @ W @ Ji
            H[sj, sj] += Jj.T @ W @ Jj
            H[si, sj] += Ji.T @ W @ Jj
            H[sj, si] += Jj.T @ W @ Ji
    out = dict(residuals=res, cost=F, gradient=g, blocks=blocks[:, TRIU[0], TRIU[1]], skipped=int((~ok).sum()))
    if dense:
        out["H"] = H
    return out


def free_nodes(n, edge_ij, fixed):
    """poses the solver moves: not fixed and with at least one counted edge"""
    e = np.asarray(edge_ij, np.int64).reshape(-1, 2)
    deg = np.zeros(n, np.int64)
    for i, j in e[valid_edges(n, e)]:
        deg[i] += 1
        deg[j] += 1
    return (~np.asarray(fixed, bool)) & (deg > 0)


def _mask(free):
    return np.repeat(free, 6)


def dense_step(H, g, lam, free):
    m = _mask(free)
    A = H + lam * np.diag(np.diag(H))
    d = np.zeros(len(m))
    if m.any():
        d[m] = np.linalg.solve(A[np.ix_(m, m)], -g.reshape(-1)[m])
    return d.reshape(-1, 6)


def pcg_step(H, g, lam, free, max_pcg_iterations, pcg_tolerance):
    """-> delta (N,6), iterations"""
    m = _mask(free)
    n = len(free)
    dH = np.diag(H).copy()
    chol = {}
    for k in np.nonzero(free)[0]:
        s = slice(6 * k, 6 * k + 6)
        chol[k] = np.linalg.cholesky(H[s, s] + lam * np.diag(dH[s]))

    def A(v):
        return np.where(m, H @ v + lam * dH * v, 0.0)

    def Minv(v):
        z = np.zeros_like(v)
        for k, L in chol.items():
            s = slice(6 * k, 6 * k + 6)
            z[s] = np.linalg.solve(L.T, np.linalg.solve(L, v[s]))
        return z

    x = np.zeros(6 * n)
    r = np.where(m, -g.reshape(-1), 0.0)
    bb = r @ r
    its = 0
    if bb == 0.0:
        return x.reshape(-1, 6), 0
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
    return x.reshape(-1, 6), its


def optimize(poses, edge_ij, Z, Om, fixed=None, solver="pcg", **params):
    p = dict(DEFAULTS, **params)
    X = np.array(poses, np.float64)
    n = len(X)
    fx = np.zeros(n, bool)
    if fixed is None:
        fx[:1] = True
    else:
        fx[:] = np.asarray(fixed, bool)
    free = free_nodes(n, edge_ij, fx)
    F = cost(X, edge_ij, Z, Om)
    out = dict(cost0=F, iterations=0, accepted=0, rejected=0, pcg_iterations=0, converged=False, step0=None)
    hist = [F]
    lam = p["lambda0"]
    for _ in range(p["max_iteration"]):
        lin = linearize(X, edge_ij, Z, Om, dense=True)
        if solver == "pcg":
            d, its = pcg_step(lin["H"], lin["gradient"], lam, free, p["max_pcg_iterations"], p["pcg_tolerance"])
        else:
            d, its = dense_step(lin["H"], lin["gradient"], lam, free), 0
        if out["step0"] is None:
            out["step0"] = d.copy()
        out["pcg_iterations"] += its
        step = float(np.sqrt((d * d).sum()))
        cand = np.stack([retract(X[k], d[k]) if free[k] else X[k] for k in range(n)]) if n else X
        Fc = cost(cand, edge_ij, Z, Om)
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


# ---- graphs the tests share -------------------------------------------------------------------------------

def ring_poses(n, radius=20.0):
    """n poses on a circle of `radius` metres, heading along the tangent, with a gentle roll / pitch / height wave"""
    out = []
    for k in range(n):
        a = 2.0 * np.pi * k / n
        X = np.eye(4)
        X[:3, :3] = exp_so3(np.array([0.0, 0.0, a + np.pi / 2])) @ exp_so3(np.array([0.03 * np.sin(3 * a),
                                                                                     0.02 * np.cos(2 * a), 0.0]))
        X[:3, 3] = [radius * np.cos(a), radius * np.sin(a), 0.3 * np.sin(2 * a)]
        out.append(X)
    return np.stack(out)


def relative(poses, edge_ij):
    return np.stack([inv_se3(poses[i]) @ poses[j] for i, j in np.asarray(edge_ij).reshape(-1, 2)]) \
        if len(edge_ij) else np.zeros((0, 4, 4))


def chain_edges(n):
    return np.stack([np.arange(n - 1), np.arange(1, n)], 1).astype(np.int64)


def noisy(Z, rng, rot=0.002, trans=0.02):
    return np.stack([z @ make_pose(rot * rng.standard_normal(3), trans * rng.standard_normal(3)) for z in Z])


def integrate(Z, X0=None):
    """poses of a chain from its relative measurements"""
    X = [np.eye(4) if X0 is None else X0]
    for z in Z:
        X.append(X[-1] @ z)
    return np.stack(X)


def random_information(rng, m):
    out = []
    for _ in range(m):
        A = rng.standard_normal((6, 6))
        out.append(A @ A.T + 6.0 * np.eye(6))
    return np.stack(out) if m else np.zeros((0, 6, 6))


def drift_ring(n=64, seed=0, rot=0.004, trans=0.03):
    """A ring with accumulated odometry drift and one closure (last pose -> first):
    -> truth (n,4,4), initial (n,4,4), edge_ij, Z, Om"""
    rng = np.random.default_rng(seed)
    truth = ring_poses(n)
    truth = np.stack([inv_se3(truth[0]) @ x for x in truth])        # pose 0 at the origin: it is the fixed one
    e = chain_edges(n)
    Zo = noisy(relative(truth, e), rng, rot, trans)
    init = integrate(Zo)
    loop = np.array([[n - 1, 0]], np.int64)
    Zl = noisy(relative(truth, loop), rng, rot / 4, trans / 4)
    Om_o = np.tile(np.diag([1e4, 1e4, 1e4, 4e2, 4e2, 4e2]), (n - 1, 1, 1))
    Om_l = np.tile(np.diag([4e4, 4e4, 4e4, 2e3, 2e3, 2e3]), (1, 1, 1))
    return truth, init, np.concatenate([e, loop]), np.concatenate([Zo, Zl]), np.concatenate([Om_o, Om_l])


def far_start(n=12, seed=3):
    """The rejected-step case: a ring with two loop edges, started far from the optimum; run with lambda0 = 1e-12.
    -> truth, initial, edge_ij, Z, Om"""
    rng = np.random.default_rng(seed)
    truth = ring_poses(n, radius=8.0)
    e = np.concatenate([chain_edges(n), np.array([[n - 1, 0], [n // 2, 1]], np.int64)])
    Z = noisy(relative(truth, e), rng)
    Om = random_information(rng, len(e)) * 50.0
    init = np.stack([x @ make_pose(0.9 * rng.standard_normal(3), 4.0 * rng.standard_normal(3)) for x in truth])
    init[0] = truth[0]
    return truth, init, e, Z, Om


def trajectory_error(poses, truth):
    return float(np.sqrt(np.mean(np.sum((poses[:, :3, 3] - truth[:, :3, 3]) ** 2, axis=1))))
