"""Float64 numpy restatement of the robust kernels of csrc/nsc_posegraph.hip (contract: include/nsc.h,
nsc_posegraph_optimize_robust), on top of posegraph_restatement: the same residuals, Jacobians, Levenberg-Marquardt and
PCG rules, with

    s = r^T Omega r,  F = sum rho(s),  g = sum w J^T Omega r,  H = sum w J^T Omega J,  w = rho'(s)

    huber          rho = s for s <= c^2, else 2 c sqrt(s) - c^2     w = 1 for s <= c^2, else c / sqrt(s)
    cauchy         rho = c^2 log1p(s / c^2)                         w = 1 / (1 + s / c^2)
    geman_mcclure  rho = c^2 s / (c^2 + s)                          w = (c^2 / (c^2 + s))^2

An edge is quadratic (rho = s, w = 1) with kernel NONE, without widths, for a width that is not finite and positive (or
whose square is not), and for s <= 0.
"""
import numpy as np

import posegraph_restatement as P

NONE, HUBER, CAUCHY, GEMAN_MCCLURE = 0, 1, 2, 3
KERNELS = {"huber": HUBER, "cauchy": CAUCHY, "geman_mcclure": GEMAN_MCCLURE}


def is_robust(kernel, c, s):
    """whether the edge leaves the quadratic cost"""
    if kernel == NONE or c is None:
        return False
    c = float(c)
    with np.errstate(over="ignore", under="ignore"):
        c2 = c * c
    return bool(c > 0.0 and np.isfinite(c2) and c2 > 0.0 and s > 0.0)


def rho_w(kernel, c, s):
    """-> rho(s), w(s) of one edge of width c"""
    if not is_robust(kernel, c, s):
        return s, 1.0
    c = float(c)
    c2 = c * c
    if kernel == HUBER:
        if s <= c2:
            return s, 1.0
        q = np.sqrt(s)
        return 2.0 * c * q - c2, c / q
    if kernel == CAUCHY:
        return c2 * np.log1p(s / c2), 1.0 / (1.0 + s / c2)
    if kernel == GEMAN_MCCLURE:
        return c2 * s / (c2 + s), (c2 / (c2 + s)) ** 2
    raise ValueError(kernel)


def _width(scale, k):
    return None if scale is None else scale[k]


def edge_chi2(poses, edge_ij, Z, Om):
    """r^T Omega r of every edge, 0 for a skipped one"""
    e = np.asarray(edge_ij, np.int64).reshape(-1, 2)
    s = np.zeros(len(e))
    for k in np.nonzero(P.valid_edges(len(poses), e))[0]:
        r = P.residual(poses[e[k, 0]], poses[e[k, 1]], Z[k])
        s[k] = r @ P.sym_upper(Om[k]) @ r
    return s


def edge_weights(poses, edge_ij, Z, Om, kernel, scale):
    """-> chi2 (E,), weights (E,): zeros for skipped edges"""
    e = np.asarray(edge_ij, np.int64).reshape(-1, 2)
    ok = P.valid_edges(len(poses), e)
    s = edge_chi2(poses, e, Z, Om)
    return s, np.array([rho_w(kernel, _width(scale, k), s[k])[1] if ok[k] else 0.0 for k in range(len(e))])


def cost(poses, edge_ij, Z, Om, kernel=NONE, scale=None):
    e = np.asarray(edge_ij, np.int64).reshape(-1, 2)
    ok = P.valid_edges(len(poses), e)
    s = edge_chi2(poses, e, Z, Om)
    return float(sum(rho_w(kernel, _width(scale, k), s[k])[0] for k in np.nonzero(ok)[0]))


def linearize(poses, edge_ij, Z, Om, kernel=NONE, scale=None, dense=False):
    """-> dict(residuals (E,6) unweighted, chi2 (E,), weights (E,), cost, gradient (N,6), blocks (N,21), skipped
    [, H (6N,6N)])"""
    poses = np.asarray(poses, np.float64)
    n = len(poses)
    e = np.asarray(edge_ij, np.int64).reshape(-1, 2)
    ok = P.valid_edges(n, e)
    res, chi2, wts = np.zeros((len(e), 6)), np.zeros(len(e)), np.zeros(len(e))
    g = np.zeros((n, 6))
    blocks = np.zeros((n, 6, 6))
    H = np.zeros((6 * n, 6 * n)) if dense else None
    F = 0.0
    for k in np.nonzero(ok)[0]:
        i, j = e[k]
        r, Ji, Jj = P.edge_terms(poses[i], poses[j], Z[k])
        W = P.sym_upper(Om[k])
        s = r @ W @ r
        rho, w = rho_w(kernel, _width(scale, k), s)
        res[k], chi2[k], wts[k] = r, s, w
        W = w * W
        F += rho
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
    out = dict(residuals=res, chi2=chi2, weights=wts, cost=F, gradient=g, blocks=blocks[:, P.TRIU[0], P.TRIU[1]],
               skipped=int((~ok).sum()))
    if dense:
        out["H"] = H
    return out


def optimize(poses, edge_ij, Z, Om, kernel=NONE, scale=None, fixed=None, solver="pcg", **params):
    """posegraph_restatement.optimize with the robust cost and the weighted system; also -> chi2, weights at the end"""
    p = dict(P.DEFAULTS, **params)
    X = np.array(poses, np.float64)
    n = len(X)
    fx = np.zeros(n, bool)
    if fixed is None:
        fx[:1] = True
    else:
        fx[:] = np.asarray(fixed, bool)
    free = P.free_nodes(n, edge_ij, fx)
    F = cost(X, edge_ij, Z, Om, kernel, scale)
    out = dict(cost0=F, iterations=0, accepted=0, rejected=0, pcg_iterations=0, converged=False, step0=None)
    hist = [F]
    lam = p["lambda0"]
    for _ in range(p["max_iteration"]):
        lin = linearize(X, edge_ij, Z, Om, kernel, scale, dense=True)
        if solver == "pcg":
            d, its = P.pcg_step(lin["H"], lin["gradient"], lam, free, p["max_pcg_iterations"], p["pcg_tolerance"])
        else:
            d, its = P.dense_step(lin["H"], lin["gradient"], lam, free), 0
        if out["step0"] is None:
            out["step0"] = d.copy()
        out["pcg_iterations"] += its
        step = float(np.sqrt((d * d).sum()))
        cand = np.stack([P.retract(X[k], d[k]) if free[k] else X[k] for k in range(n)]) if n else X
        Fc = cost(cand, edge_ij, Z, Om, kernel, scale)
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
    chi2, wts = edge_weights(X, edge_ij, Z, Om, kernel, scale)
    out.update(poses=X, cost=F, cost_history=np.array(hist), lam=lam, chi2=chi2, weights=wts)
    return out


# ---- the outlier ring ---------------------------------------------------------------------------------------------

TRUE_CLOSURES = ((60, 2), (58, 4), (62, 1))
FALSE_CLOSURES = ((40, 8), (50, 20))


def outlier_ring(seed=0, false_closures=True):
    """drift_ring(64, seed) plus three true closures (noisy, rng seed 100) and, on request, two false ones, all with
    Omega = diag(4e4 x 3, 2e3 x 3).  The closure edges are the last `closures` ones.
    -> truth, initial, edge_ij, Z, Om, closures"""
    truth, init, e, Z, Om = P.drift_ring(64, seed)
    te = np.asarray(TRUE_CLOSURES, np.int64)
    tZ = P.noisy(P.relative(truth, te), np.random.default_rng(100), 0.001, 0.0075)
    fe = np.asarray(FALSE_CLOSURES if false_closures else (), np.int64).reshape(-1, 2)
    fZ = np.tile(P.make_pose([0.0, 0.0, 0.1], [0.5, -0.3, 0.0]), (len(fe), 1, 1))
    m = len(te) + len(fe)
    om = np.tile(np.diag([4e4, 4e4, 4e4, 2e3, 2e3, 2e3]), (m, 1, 1))
    return (truth, init, np.concatenate([e, te, fe]), np.concatenate([Z, tZ, fZ]), np.concatenate([Om, om]),
            1 + m)


def closure_scale(n_edges, closures, c):
    """zero on the odometry edges, c on the last `closures` edges"""
    s = np.zeros(n_edges)
    s[n_edges - closures:] = c
    return s
