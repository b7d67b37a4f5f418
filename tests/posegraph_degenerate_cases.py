"""Constructed pose graphs on which the optimiser's system is not well posed, shared by test_posegraph_degenerate_cpu.py
and test_posegraph_degenerate_gpu.py: information matrices that are zero, negative, indefinite, rank-deficient or not
finite, so that the paths of csrc/nsc_posegraph.hip that a healthy graph never takes do run -- a damped diagonal block
that is not positive definite, a coarse factor that fails, the PCG exit on p.Ap <= 0.

Every case returns ``(X, edge_ij, Z, Om, fixed, extras)``; ``extras`` holds the parameters the case is run with
(``params``, ``L`` values, ``kernel`` and ``scale``) and what it claims (``not_free``: poses whose block fails).

``traced_optimize`` is posegraph_coarse_restatement.optimize, step for step and bit for bit, that also records every
decision it takes with the scale the decision is formed on, and that can be run as a mutant (one rule broken).
"""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import posegraph_coarse_restatement as Cr
import posegraph_restatement as P
import posegraph_robust_restatement as R

BAR = 1e-6                                   # close() of test_posegraph_gpu.py: the margin every decision must have

BRANCHES = ("block not PD", "identity aggregate from non-PD blocks", "coarse factor failed",
            "factor OK on an indefinite A", "p.Ap <= 0 exit", "fail-then-succeed", "succeed-then-fail")
MUTANTS = ("block-free", "stale-inverse", "breakdown-steps", "breakdown-uncounted", "no-lambda-coarse")


def first_fixed(n):
    fixed = np.zeros(n, bool)
    fixed[:1] = True
    return fixed


# ---- the decidable cases ------------------------------------------------------------------------------------------------

def _ring(n, seed, radius=20.0):
    """a noisy ring with unit information: poses perturbed about the truth, chain edges and the closure (n - 1, 0)"""
    rng = np.random.default_rng(seed)
    truth = P.ring_poses(n, radius)
    truth = np.stack([P.inv_se3(truth[0]) @ x for x in truth])
    e = np.concatenate([P.chain_edges(n), [[n - 1, 0]]]).astype(np.int64)
    Z = P.noisy(P.relative(truth, e), rng)
    X = np.stack([x @ P.make_pose(0.02 * rng.standard_normal(3), 0.1 * rng.standard_normal(3)) for x in truth])
    X[0] = truth[0]
    return truth, X, e, Z, np.tile(np.eye(6), (len(e), 1, 1)), rng


def chords(n=9, weight=0.75, seed=0, also=(), radius=20.0, **params):
    """The family of the issue: a noisy ring with unit information plus chords (k, k + 2) for odd k (and for the k of
    ``also``), each with information -weight I.  The chord's lever arm makes the block of its first end indefinite, so the
    odd poses are not free; the free system stays indefinite at small lambda and positive definite from lambda ~ 1 on."""
    truth, X, e, Z, Om, rng = _ring(n, seed, radius)
    ks = sorted(set(range(1, n - 2, 2)) | set(also))
    ce = np.array([[k, k + 2] for k in ks], np.int64).reshape(-1, 2)
    cZ = P.noisy(P.relative(truth, ce), rng)
    cOm = np.tile(-weight * np.eye(6), (len(ce), 1, 1))
    extras = dict(params=dict(max_iteration=8, max_pcg_iterations=100, **params), chords=len(ce), not_free=ks)
    return X, np.concatenate([e, ce]), np.concatenate([Z, cZ]), np.concatenate([Om, cOm]), first_fixed(n), extras


def chords65():
    """n = 65, L = 8: the ragged last aggregate of one pose, and aggregate 3 (poses 24..31) with a chord from every one
    of its poses, so that none of them is free and its block of A_c is the identity"""
    return chords(65, 0.75, 0, also=range(24, 32))


def leaf(weight, n=6, seed=1):
    """a closed chain 0 .. n - 1 with random information and a leaf pose n tied to pose 2 by an edge with information
    weight I: 0 -> the leaf's block is exactly zero, -1 -> negative definite; pose 2 keeps a positive definite block.
    Three outer steps: the later ones decide on gains at rounding level.  The poses lie within a metre or so: with lever
    arms of 4 m the system's condition number is 2e4, PCG needs 25 of its 30 possible iterations and two float64
    implementations of it differ by 5e-7 in the step, half the bar; here they differ by 1e-13."""
    rng = np.random.default_rng(seed)
    truth = np.stack([P.make_pose(0.3 * rng.standard_normal(3), rng.standard_normal(3)) for _ in range(n + 1)])
    e = np.concatenate([P.chain_edges(n), [[n - 1, 0], [n, 2]]]).astype(np.int64)     # pose 2 is the second end: J_j = B
    Z = P.noisy(P.relative(truth, e), rng, 0.01, 0.05)
    Om = np.concatenate([P.random_information(rng, n), weight * np.eye(6)[None]])
    X = np.stack([x @ P.make_pose(0.05 * rng.standard_normal(3), 0.2 * rng.standard_normal(3)) for x in truth])
    X[0] = truth[0]
    return X, e, Z, Om, first_fixed(n + 1), dict(params=dict(max_iteration=3, max_pcg_iterations=100), not_free=[n])


def robust_indefinite(n=9, seed=0):
    """``chords`` with Cauchy widths on the chords, and with the information of every second chord turned to
    diag(-w, -w, -w, 3, 3, 3): there chi^2 > 0, so the Cauchy weight is below 1 and scales an indefinite block; a chord
    with -w I has chi^2 <= 0 and stays quadratic, as the contract has it"""
    X, e, Z, Om, fixed, extras = chords(n, 0.75, seed)
    m = extras["chords"]
    first = len(e) - m
    for k in range(first, len(e), 2):
        Om[k] = np.diag([-0.75, -0.75, -0.75, 3.0, 3.0, 3.0])
    extras.update(kernel=R.CAUCHY, scale=R.closure_scale(len(e), m, 0.05))
    return X, e, Z, Om, fixed, extras


# name -> (maker, coarse blocks to run it with)
DECIDABLE = {
    "zero-leaf": (lambda: leaf(0.0), (None, 2)),
    "negative-leaf": (lambda: leaf(-1.0), (None, 2)),
    "chords-4": (lambda: chords(4), (None, 2)),
    "chords-9": (lambda: chords(9), (None, 2, 4)),
    # radius 6, seed 1: at lambda0 the factor of A_c fails for L = 2 and exists for L = 4 while A is indefinite
    "chords-17": (lambda: chords(17, 0.9, 1, radius=6.0), (None, 2, 4)),
    "chords-65": (chords65, (8,)),
    # eight outer steps are the cap of the device tests: a factor of 100 takes lambda from 1e-4 past 1 within them
    "lambda-walk-up": (lambda: chords(9, lambda_factor=100.0), (2,)),
    "lambda-walk-down": (lambda: chords(9, lambda0=10.0, lambda_factor=1e3), (2,)),
    "robust-indefinite": (robust_indefinite, (None, 2)),
}


def decidable(name):
    return DECIDABLE[name][0]()


def instances():
    """(case, L) of every decidable run"""
    return [(name, L) for name, (_, Ls) in DECIDABLE.items() for L in Ls]


# ---- the undecidable cases ----------------------------------------------------------------------------------------------

def _conjugated(W, T):
    """Ad(T)^T sym(W) Ad(T): what pose_graph.closure_edges hands the optimiser"""
    A = P.adjoint(T)
    return A.T @ (0.5 * (W + W.T)) @ A


def planar_information(n=9, seed=2):
    """every edge carries diag(0, 0, 1, 1, 1, 0) (yaw, x, y: what a planar registration observes) conjugated by its
    measurement, on a ring whose poses, measurements and noise are planar too: every block of H has rank 3 with roll, pitch
    and height in its null space, so three of its pivots are rounding errors of either sign"""
    rng = np.random.default_rng(seed)

    def planar(a, x, y):                                      # and 1e-8 of roll, pitch and height: their squares are roundings
        return P.make_pose([0.0, 0.0, a], [x, y, 0.0]) @ P.make_pose(1e-8 * rng.standard_normal(3) * [1, 1, 0],
                                                                      1e-8 * rng.standard_normal(3) * [0, 0, 1])
    ang = 2.0 * np.pi * np.arange(n) / n
    truth = np.stack([planar(a + np.pi / 2, 6.0 * np.cos(a) - 6.0, 6.0 * np.sin(a)) for a in ang])
    e = np.concatenate([P.chain_edges(n), [[n - 1, 0]]]).astype(np.int64)
    Z = np.stack([z @ planar(*(s * rng.standard_normal() for s in (0.002, 0.02, 0.02))) for z in P.relative(truth, e)])
    X = np.stack([x @ planar(*(s * rng.standard_normal() for s in (0.02, 0.1, 0.1))) for x in truth])
    X[0] = truth[0]
    W = np.diag([0.0, 0.0, 1.0, 1.0, 1.0, 0.0])
    Om = np.stack([_conjugated(W, z) for z in Z])
    return X, e, Z, Om, first_fixed(n), dict(params=dict(max_iteration=8, max_pcg_iterations=100))


def corridor_candidate(n=12, seed=3):
    """a chain with identity odometry information and the stand-in of one verified LoopClosureCandidate (database 1, query
    n - 1) whose GICP information has rank 5: nothing constrains the motion along the corridor's axis
    -> X, edge_ij, Z, Om of the odometry, and the candidate"""
    rng = np.random.default_rng(seed)
    truth = P.integrate([P.make_pose([0.0, 0.0, 0.02], [1.0, 0.0, 0.0])] * (n - 1))
    e = P.chain_edges(n)
    Z = P.noisy(P.relative(truth, e), rng, 0.004, 0.03)
    X = P.integrate(Z)
    T = P.noisy(P.relative(truth, np.array([[1, n - 1]])), rng, 0.001, 0.01)[0]
    B = rng.standard_normal((6, 5))
    B[3] = 0.0                                                # no row for x: the corridor's axis
    cand = SimpleNamespace(verified=True, transform=T, information_matrix=100.0 * (B @ B.T), database_idx=1)
    return X, e, Z, np.tile(np.eye(6), (n - 1, 1, 1)), cand


NON_FINITE = ("nan-in-Z", "nan-in-Om", "inf-in-Om", "nan-in-pose")


def non_finite(kind, apart=False):
    """``chain5``-like ring of 6 poses (anchored by pose 0) and a loose chain of 4 more that no edge ties to it, with one
    bad entry: in the anchored ring, or with ``apart`` in the loose chain.  extras: ``clean`` = the same graph without the
    bad entry, ``edges`` / ``poses`` = what the bad entry touches"""
    rng = np.random.default_rng(11)
    truth, X, e, Z, _, _ = _ring(6, 4, radius=5.0)
    tail = np.stack([P.make_pose(0.2 * rng.standard_normal(3), [30.0 + 2.0 * k, 1.0, 0.0]) for k in range(4)])
    e2 = P.chain_edges(4) + 6
    Z2 = P.noisy(P.relative(tail, P.chain_edges(4)), rng)
    X = np.concatenate([X, np.stack([x @ P.make_pose(0.02 * rng.standard_normal(3), 0.1 * rng.standard_normal(3))
                                     for x in tail])])
    e, Z = np.concatenate([e, e2]), np.concatenate([Z, Z2])
    Om = P.random_information(rng, len(e))
    clean = (X.copy(), e.copy(), Z.copy(), Om.copy())
    k = len(e) - 2 if apart else 2                            # the edge (7, 8) or (2, 3)
    touched_edges, touched_poses = [k], [int(e[k, 0]), int(e[k, 1])]
    if kind == "nan-in-Z":
        Z[k, 1, 3] = np.nan
    elif kind == "nan-in-Om":
        Om[k, 1, 4] = np.nan
    elif kind == "inf-in-Om":
        Om[k, 2, 2] = np.inf
    elif kind == "nan-in-pose":
        p = 8 if apart else 3
        X[p, 0, 1] = np.nan
        touched_edges = [int(a) for a in np.nonzero((e == p).any(1))[0]]
        touched_poses = sorted({int(v) for a in touched_edges for v in e[a]})
    else:
        raise ValueError(kind)
    extras = dict(params=dict(max_iteration=4, max_pcg_iterations=30), clean=clean, edges=touched_edges,
                  poses=touched_poses)
    return X, e, Z, Om, first_fixed(len(X)), extras


# ---- the restatement with its decisions recorded, and its mutants -------------------------------------------------------

def pivots(M):
    """The pivots d_r = M_rr - sum_k U_kr^2 of the Cholesky factor in the order the device takes them, up to and including
    the first that is not positive and finite, each with the scale it is formed on, |M_rr| + sum_k U_kr^2.
    -> [(d, scale)], ok"""
    n = len(M)
    U = np.zeros((n, n))
    out = []
    for r in range(n):
        q = float(U[:r, r] @ U[:r, r])
        d = M[r, r] - q
        out.append((d, abs(M[r, r]) + q))
        if not (d > 0.0 and np.isfinite(d)):
            return out, False
        U[r, r] = np.sqrt(d)
        U[r, r + 1:] = (M[r, r + 1:] - U[:r, r] @ U[:r, r + 1:]) / U[r, r]
    return out, True


def _margin(trace, what, value, scale):
    trace["margins"].append((what, float(abs(value) / scale) if scale > 0.0 else np.inf))


def _cost_terms(X, e, Z, Om, kernel, scale):
    s = R.edge_chi2(X, e, Z, Om)
    ok = P.valid_edges(len(X), e)
    return np.array([R.rho_w(kernel, None if scale is None else scale[k], s[k])[0] for k in np.nonzero(ok)[0]])


def traced_pcg(H, g, lam, free, Minv, max_pcg_iterations, pcg_tolerance, trace, mutant=None):
    """posegraph_coarse_restatement.pcg_step with the preconditioner given, its decisions recorded -> x (6N,), iterations"""
    m = np.repeat(free, 6)
    dH = H.diagonal()
    tol2 = pcg_tolerance * pcg_tolerance

    def A(v):
        return np.where(m, H @ v + lam * dH * v, 0.0)

    x = np.zeros(len(m))
    r = np.where(m, -g.reshape(-1), 0.0)
    bb = r @ r
    its = 0
    trace["exit"] = 0.0                                       # r.r / b.b at the exit
    if bb == 0.0:
        return x, 0
    rr = bb
    z = Minv(r)
    pd = z.copy()
    rz = r @ z
    for _ in range(max_pcg_iterations):
        trace["exit"] = rr / bb
        Ap = A(pd)
        pAp = pd @ Ap
        _margin(trace, "p.Ap", pAp, float(np.abs(pd * Ap).sum()))
        broke = not pAp > 0.0
        if not (broke and mutant == "breakdown-uncounted"):
            its += 1
        if broke:
            trace["branches"].add("p.Ap <= 0 exit")
            if mutant == "breakdown-steps":
                x += (rz / pAp) * pd
            break
        alpha = rz / pAp
        x += alpha * pd
        r -= alpha * Ap
        rr = r @ r
        trace["exit"] = rr / bb
        _margin(trace, "r.r against the tolerance", rr - tol2 * bb, max(rr, tol2 * bb))
        if rr <= tol2 * bb:
            break
        z = Minv(r)
        rz_new = r @ z
        _margin(trace, "r.z", rz_new, float(np.abs(r * z).sum()))
        if not rz_new > 0.0:                                  # the device ends the loop here; the restatement has no such
            trace["branches"].add("r.z <= 0")                 # rule, so no decidable case may reach it
        pd = z + (rz_new / rz) * pd
        rz = rz_new
    return x, its


def traced_optimize(poses, edge_ij, Z, Om, L=None, kernel=R.NONE, scale=None, fixed=None, mutant=None, **params):
    """posegraph_coarse_restatement.optimize (the same calls in the same order: without a mutant every output has its
    bits) -> its result with ``trace``: ``branches`` (the set reached), ``margins`` [(decision, |value| / scale)],
    ``free`` (the mask of every outer step), ``failed`` (per outer step)."""
    assert mutant is None or mutant in MUTANTS
    p = dict(P.DEFAULTS, **params)
    X = np.array(poses, np.float64)
    n = len(X)
    fx = first_fixed(n) if fixed is None else np.asarray(fixed, bool)
    graph_free = P.free_nodes(n, edge_ij, fx)
    F = R.cost(X, edge_ij, Z, Om, kernel, scale)
    out = dict(cost0=F, iterations=0, accepted=0, rejected=0, pcg_iterations=0, converged=False, step0=None,
               coarse_aggregates=0 if L is None else Cr.aggregates(n, L), coarse_failed=0, inner=[])
    trace = dict(branches=set(), margins=[], free=[], failed=[])
    hist = [F]
    lam = p["lambda0"]
    stale = None
    for _ in range(p["max_iteration"]):
        lin = Cr.linearize(X, edge_ij, Z, Om, kernel, scale)
        H, g, blocks = lin["H"], lin["gradient"], lin["blocks"]
        free = Cr.free_nodes(n, edge_ij, fx, blocks, lam)
        for k in np.nonzero(graph_free)[0]:
            pv, ok = pivots(blocks[k] + lam * np.diag(np.diag(blocks[k])))
            assert ok == bool(free[k])
            if ok:
                d, s = min(pv, key=lambda t: t[0] / t[1])
            else:
                d, s = pv[-1]
                trace["branches"].add("block not PD")
            if s > 0.0:                                       # an exactly zero block fails on d = 0 with nothing summed
                _margin(trace, f"block pivot of pose {k}", d, s)
        if mutant == "block-free":
            free = graph_free & (np.abs(blocks).reshape(n, -1).max(1) > 0.0)      # a zero block has no inverse at all
        trace["free"].append(free.copy())
        m = np.repeat(free, 6)
        Minv = Cr.Preconditioner(H, blocks, lam, free, X, L)
        failed = Minv.failed
        if L is not None:
            if mutant == "no-lambda-coarse":
                Minv.Ac = Cr.coarse_matrix(H, 0.0, Minv.Pm, free, L)
                _, ok = pivots(Minv.Ac)
                failed = Minv.failed = not ok
                Minv.Ac_inv = np.linalg.inv(Minv.Ac) if ok else None
            pv, ok = pivots(Minv.Ac)
            assert ok == (not failed)
            for j, (d, s) in enumerate(pv):
                _margin(trace, f"coarse pivot {j}", d, s)
            for a in range(Cr.aggregates(n, L)):
                sl = slice(a * L, (a + 1) * L)
                if not free[sl].any() and (graph_free[sl] & ~free[sl]).all():
                    trace["branches"].add("identity aggregate from non-PD blocks")
            Af = (H + lam * sp.diags(H.diagonal())).toarray()[np.ix_(m, m)]
            indefinite = m.any() and np.linalg.eigvalsh(Af)[0] < 0.0
            if failed:
                trace["branches"].add("coarse factor failed")
                if trace["failed"] and not trace["failed"][-1]:
                    trace["branches"].add("succeed-then-fail")
                if mutant == "stale-inverse" and stale is not None:
                    Minv.Ac_inv = stale                       # what ignoring the flag would read
            else:
                if indefinite:
                    trace["branches"].add("factor OK on an indefinite A")
                if trace["failed"] and trace["failed"][-1]:
                    trace["branches"].add("fail-then-succeed")
                stale = Minv.Ac_inv
            trace["failed"].append(failed)

        x, its = traced_pcg(H, g, lam, free, Minv, p["max_pcg_iterations"], p["pcg_tolerance"], trace, mutant)
        d = x.reshape(-1, 6)
        if out["step0"] is None:
            out["step0"] = d.copy()
        out["pcg_iterations"] += its
        out["inner"].append(its)
        out["coarse_failed"] += int(failed)
        step = float(np.sqrt((d * d).sum()))
        cand = np.stack([P.retract(X[k], d[k]) if free[k] else X[k] for k in range(n)]) if n else X
        Fc = R.cost(cand, edge_ij, Z, Om, kernel, scale)
        terms = np.abs(_cost_terms(X, edge_ij, Z, Om, kernel, scale)).sum() + \
            np.abs(_cost_terms(cand, edge_ij, Z, Om, kernel, scale)).sum()
        if step > 0.0:                                        # delta = 0 exactly: the candidate is X and F_c = F bit for bit
            _margin(trace, "F - F_c", F - Fc, terms)
        else:
            assert Fc == F
        _margin(trace, "step against min_step", step - p["min_step"], max(step, p["min_step"]))
        out["iterations"] += 1
        stop = False
        if Fc < F:
            out["accepted"] += 1
            stop = (F - Fc) < p["relative_cost"] * F
            _margin(trace, "gain against relative_cost", (F - Fc) - p["relative_cost"] * F, terms)
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
    out.update(poses=X, cost=F, cost_history=np.array(hist), lam=lam, trace=trace)
    return out


def run(name, L, mutant=None, **override):
    """the traced restatement on a decidable case with the case's own parameters"""
    X, e, Z, Om, fixed, extras = decidable(name)
    prm = dict(extras["params"], **override)
    return traced_optimize(X, e, Z, Om, L=L, kernel=extras.get("kernel", R.NONE), scale=extras.get("scale"),
                           fixed=fixed, mutant=mutant, **prm)


def reference(name, L, **override):
    """posegraph_coarse_restatement.optimize on a decidable case: what the device is compared with"""
    X, e, Z, Om, fixed, extras = decidable(name)
    prm = dict(extras["params"], **override)
    return Cr.optimize(X, e, Z, Om, L=L, kernel=extras.get("kernel", R.NONE), scale=extras.get("scale"), fixed=fixed,
                       **prm)


# ---- the covariance call on the same graphs -----------------------------------------------------------------------------

def cov_two_components():
    """drift_ring(12), anchored by pose 0, and the ``chords`` ring of 9 as poses 12..20, which no edge ties to it and no
    pose fixes -> X, edge_ij, Z, Om, fixed, extras (``healthy`` and ``degenerate``: poses to select in either component)"""
    _, X1, e1, Z1, Om1 = P.drift_ring(12)
    X2, e2, Z2, Om2, _, _ = chords(9)
    X2 = np.stack([P.make_pose([0.0, 0.0, 0.4], [90.0, -5.0, 1.0]) @ x for x in X2])
    return (np.concatenate([X1, X2]), np.concatenate([e1, e2 + 12]), np.concatenate([Z1, Z2]),
            np.concatenate([Om1, Om2]), first_fixed(21), dict(healthy=[3, 7, 11], degenerate=[12, 14, 15, 20]))


def traced_columns(X, e, Z, Om, fixed, nodes, L=None, max_pcg_iterations=100, pcg_tolerance=1e-10):
    """posegraph_cov_restatement.pcg_columns (lambda = 0) with the decisions of every column recorded
    -> joint (Q,Q,6,6), iterations (Q,6), free, trace (``failed``: whether the coarse factor failed; ``converged`` (Q,6):
    the column ended at r.r <= pcg_tolerance^2 b.b)"""
    n = len(X)
    lin = Cr.linearize(X, e, Z, Om)
    free = Cr.free_nodes(n, e, fixed, lin["blocks"], 0.0)
    trace = dict(branches=set(), margins=[], failed=False)
    for k in np.nonzero(P.free_nodes(n, e, fixed))[0]:
        pv, ok = pivots(lin["blocks"][k])
        assert ok == bool(free[k])
        d, s = min(pv, key=lambda t: t[0] / t[1]) if ok else pv[-1]
        _margin(trace, f"block pivot of pose {k}", d, s)
    Minv = Cr.Preconditioner(lin["H"], lin["blocks"], 0.0, free, X, L)
    if L is not None:
        trace["failed"] = Minv.failed
        for j, (d, s) in enumerate(pivots(Minv.Ac)[0]):
            _margin(trace, f"coarse pivot {j}", d, s)
    q = len(nodes)
    joint, its = np.zeros((q, q, 6, 6)), np.zeros((q, 6), np.int64)
    trace["converged"] = np.zeros((q, 6), bool)
    for b, nb in enumerate(nodes):
        for c in range(6):
            g = np.zeros((n, 6))
            if free[nb]:
                g[nb, c] = -1.0
            x, its[b, c] = traced_pcg(lin["H"], g, 0.0, free, Minv, max_pcg_iterations, pcg_tolerance, trace)
            trace["converged"][b, c] = trace["exit"] <= pcg_tolerance * pcg_tolerance
            joint[:, b, :, c] = x.reshape(-1, 6)[nodes]
    return joint, its, free, trace
