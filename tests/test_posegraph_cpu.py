"""Pose-graph optimisation without a device: the float64 restatement (tests/posegraph_restatement.py) against central
differences and an independent least-squares solver, the host helpers of retrieval/pose_graph.py, and the argument
checks of the C ABI."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import posegraph_restatement as P

ANGLES = (0.0, 1e-9, 1e-3, np.pi / 2, np.deg2rad(170.0))

# Distance between the restatement's optimum and scipy.optimize.least_squares' (xtol = ftol = gtol = 1e-14, 3-point
# Jacobians) on the noisy 12-pose ring below, measured: 3.6e-10 over the pose entries (the
# restatement's |g| there is 4e-12, scipy's 2e-11; with scipy's default 2-point Jacobians the distance is 2.8e-8).
# The bar is ten times that, for scipy's own stopping slack.
SCIPY_DISTANCE = 3.6e-10


def edge_with_residual_angle(rng, angle):
    """Xi, Xj, Z whose residual rotation is `angle` about a random axis (and a residual translation of about 1 m)"""
    Xi = P.make_pose(rng.standard_normal(3), 5.0 * rng.standard_normal(3))
    A = P.make_pose(0.5 * rng.standard_normal(3), 3.0 * rng.standard_normal(3))
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    D = P.make_pose(axis * angle, rng.standard_normal(3))
    return Xi, Xi @ A, A @ P.inv_se3(D)


@pytest.mark.parametrize("angle", ANGLES)
def test_jacobians_against_central_differences(angle):
    rng = np.random.default_rng(11)
    h = 1e-6
    for _ in range(4):
        Xi, Xj, Z = edge_with_residual_angle(rng, angle)
        r, Ji, Jj = P.edge_terms(Xi, Xj, Z)
        assert abs(np.linalg.norm(r[:3]) - angle) <= 1e-9
        Ni, Nj = np.zeros((6, 6)), np.zeros((6, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            Ni[:, k] = (P.residual(P.retract(Xi, d), Xj, Z) - P.residual(P.retract(Xi, -d), Xj, Z)) / (2 * h)
            Nj[:, k] = (P.residual(Xi, P.retract(Xj, d), Z) - P.residual(Xi, P.retract(Xj, -d), Z)) / (2 * h)
        # central differences: h^2 times the third derivative, plus rounding 1e-16 / h of residuals of size <= 10
        bar = 1e-7 * max(1.0, np.abs(Ji).max())
        assert np.abs(Ni - Ji).max() <= bar and np.abs(Nj - Jj).max() <= bar


def noisy_ring12():
    rng = np.random.default_rng(5)
    truth = P.ring_poses(12, radius=6.0)
    e = np.concatenate([P.chain_edges(12), np.array([[11, 0], [7, 2]], np.int64)])
    Z = P.noisy(P.relative(truth, e), rng, rot=0.01, trans=0.05)
    Om = P.random_information(rng, len(e))
    init = np.stack([x @ P.make_pose(0.02 * rng.standard_normal(3), 0.1 * rng.standard_normal(3)) for x in truth])
    init[0] = truth[0]
    return truth, init, e, Z, Om


def test_optimum_against_scipy_least_squares():
    from scipy.optimize import least_squares
    truth, init, e, Z, Om = noisy_ring12()
    ours = P.optimize(init, e, Z, Om, max_iteration=50, max_pcg_iterations=500, pcg_tolerance=1e-14,
                      relative_cost=0.0, min_step=1e-13)
    Ls = [np.linalg.cholesky(P.sym_upper(w)).T for w in Om]               # Omega = L^T L

    def poses_of(x):
        return np.stack([init[0]] + [P.retract(init[k], x[6 * (k - 1):6 * k]) for k in range(1, 12)])

    def whitened(x):
        X = poses_of(x)
        return np.concatenate([Ls[k] @ P.residual(X[i], X[j], Z[k]) for k, (i, j) in enumerate(e)])

    sol = least_squares(whitened, np.zeros(66), xtol=1e-14, ftol=1e-14, gtol=1e-14, method="trf", jac="3-point")
    ref = poses_of(sol.x)
    dist = np.abs(ours["poses"] - ref).max()
    print("distance to scipy's optimum:", dist, "costs:", ours["cost"], 2 * sol.cost)
    assert dist <= 10 * SCIPY_DISTANCE
    assert abs(ours["cost"] - 2 * sol.cost) <= 1e-9 * ours["cost"]


def test_exact_recovery_from_noise_free_edges():
    rng = np.random.default_rng(2)
    truth = P.ring_poses(10, radius=5.0)
    e = np.concatenate([P.chain_edges(10), np.array([[9, 0], [6, 1]], np.int64)])
    Z = P.relative(truth, e)
    Om = P.random_information(rng, len(e))
    init = np.stack([x @ P.make_pose(0.1 * rng.standard_normal(3), 0.3 * rng.standard_normal(3)) for x in truth])
    init[0] = truth[0]
    out = P.optimize(init, e, Z, Om, max_iteration=30, pcg_tolerance=1e-10, max_pcg_iterations=200)
    assert out["converged"] and out["cost"] <= 1e-16 * out["cost0"]
    assert np.abs(out["poses"] - truth).max() <= 1e-8


def test_rejected_step_case_rejects_and_converges():
    truth, init, e, Z, Om = P.far_start()
    out = P.optimize(init, e, Z, Om, lambda0=1e-12, max_iteration=60)
    assert out["rejected"] >= 1 and out["converged"]
    h = out["cost_history"]
    assert np.all(np.diff(h) <= 0) and out["cost"] < 1e-2 * out["cost0"]


def test_closure_edges_converts_the_information_frame():
    """GICP's information weighs a left perturbation xi of the measurement, T = Exp(xi) Z; the residual of that
    measurement against Z is r = Ad(Z^-1) xi to first order.  chi^2 must agree: r^T Omega_r r = xi^T Omega xi up to
    O(|xi|) relative.  The lever arm (8 m) makes the [t]x term matter: without it the two differ by far more."""
    from neural_spectral_codec_amd.retrieval.pose_graph import closure_edges
    rng = np.random.default_rng(4)
    Zt = P.make_pose(np.array([0.02, -0.01, 2.9]), np.array([3.5, -8.0, 0.2]))
    W = P.random_information(rng, 1)[0]
    cands = [SimpleNamespace(database_idx=3, verified=True, transform=Zt, information_matrix=W),
             SimpleNamespace(database_idx=5, verified=False, transform=Zt, information_matrix=W),
             SimpleNamespace(database_idx=6, verified=False, transform=None, information_matrix=None)]
    e, Z, Om = closure_edges(9, cands)
    assert e.tolist() == [[3, 9]] and np.array_equal(Z[0], Zt) and Om.shape == (1, 6, 6)
    for scale in (1e-3, 1e-5):
        xi = scale * rng.standard_normal(6)
        T = P.make_pose(xi[:3], xi[3:]) @ Zt                   # the true relative pose X_i^-1 X_j
        r = P.residual(np.eye(4), T, Zt)
        chi_r, chi_xi = r @ Om[0] @ r, xi @ W @ xi
        assert abs(chi_r - chi_xi) <= 20 * scale * chi_xi, (scale, chi_r, chi_xi)
        R = Zt[:3, :3]
        naive = np.zeros((6, 6))
        naive[:3, :3] = naive[3:, 3:] = R                       # rotation only, no [t]x
        assert abs(r @ (naive.T @ W @ naive) @ r - chi_xi) > 0.05 * chi_xi


def test_g2o_information_order_round_trip():
    from neural_spectral_codec_amd.retrieval.pose_graph import information_from_g2o, information_to_g2o
    rng = np.random.default_rng(0)
    W = P.random_information(rng, 3)
    G = information_to_g2o(W)
    assert np.array_equal(G[:, :3, :3], W[:, 3:, 3:]) and np.array_equal(G[:, 3:, :3], W[:, :3, 3:])
    assert np.array_equal(information_from_g2o(G), W)
    assert np.array_equal(information_from_g2o(information_to_g2o(W[0])), W[0])


def test_odometry_edges():
    from neural_spectral_codec_amd.retrieval.pose_graph import odometry_edges
    X = P.ring_poses(5)
    e, Z, Om = odometry_edges(X, information=2.0 * np.eye(6))
    assert e.tolist() == [[0, 1], [1, 2], [2, 3], [3, 4]] and Om.shape == (4, 6, 6) and Om[2, 1, 1] == 2.0
    assert np.abs(Z - P.relative(X, e)).max() <= 1e-14
    e, Z, Om = odometry_edges(X[:1])
    assert e.shape == (0, 2) and Z.shape == (0, 4, 4) and Om.shape == (0, 6, 6)


@pytest.fixture(scope="module")
def lib():
    from neural_spectral_codec_amd import build, _lib
    build.build_hip()
    return _lib.lib()


def test_argument_checks_without_a_device(lib):
    from neural_spectral_codec_amd import _lib
    p = _lib.PoseGraphParams()
    lib.nsc_posegraph_default_params(C.byref(p))
    assert (p.max_iteration, p.max_pcg_iterations) == (P.DEFAULTS["max_iteration"], P.DEFAULTS["max_pcg_iterations"])
    for k in ("pcg_tolerance", "lambda0", "lambda_min", "lambda_factor", "relative_cost", "min_step"):
        assert getattr(p, k) == P.DEFAULTS[k]
    d = 256                                                   # non-null dummy pointer: nothing may be dereferenced
    need = lib.nsc_posegraph_workspace_bytes(100, 120, C.byref(p))
    assert need > 0 and lib.nsc_posegraph_workspace_bytes(100, 120, None) == need
    assert lib.nsc_posegraph_workspace_bytes(-1, 0, None) == 0

    def opt(poses=d, n=100, e=d, z=d, om=d, m=120, fixed=d, prm=p, out=d, stats=d, hist=d, ws=d, nbytes=need):
        return lib.nsc_posegraph_optimize(poses, n, e, z, om, m, fixed, C.byref(prm) if prm is not None else None, out,
                                          stats, hist, None, ws, nbytes, None)

    def lin(poses=d, n=100, e=d, z=d, om=d, m=120, res=d, cost=d, g=d, blocks=d, skipped=d, ws=d, nbytes=need):
        return lib.nsc_posegraph_linearize(poses, n, e, z, om, m, res, cost, g, blocks, skipped, ws, nbytes, None)

    for name in ("poses", "e", "z", "om", "fixed", "prm", "out", "stats", "hist"):
        assert opt(**{name: None}) == -1, name
    for name in ("poses", "e", "z", "om", "res", "cost", "g", "blocks", "skipped"):
        assert lin(**{name: None}) == -1, name
    assert opt(n=-1) == -1 and opt(m=-1) == -1 and lin(n=-1) == -1 and lin(m=-1) == -1
    assert opt(nbytes=need - 1) == -3 and lin(nbytes=need - 1) == -3 and opt(ws=None) == -3 and lin(ws=None) == -3
    for field, bad in (("max_iteration", -1), ("max_pcg_iterations", -1), ("pcg_tolerance", -1.0), ("lambda0", 0.0),
                       ("lambda_min", 0.0), ("lambda_factor", 1.0), ("relative_cost", -1.0), ("min_step", float("nan"))):
        q = _lib.PoseGraphParams()
        lib.nsc_posegraph_default_params(C.byref(q))
        setattr(q, field, bad)
        assert opt(prm=q) == -1, field
    q = _lib.PoseGraphParams()
    lib.nsc_posegraph_default_params(C.byref(q))
    q.max_iteration, q.max_pcg_iterations = 1000, 1000         # 4 million launches in one call
    assert opt(prm=q) == -2
