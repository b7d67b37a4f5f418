"""Robust kernels of the pose-graph optimiser without a device: the restatement (tests/posegraph_robust_restatement.py)
against central differences -- w = rho' for every kernel, the gradient of the robust cost on a graph -- and the argument
checks of the two robust entry points of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import posegraph_restatement as P
import posegraph_robust_restatement as R

WIDTH = 3.0
ROBUST = (R.HUBER, R.CAUCHY, R.GEMAN_MCCLURE)


def chain5():
    """the 5-chain with a loop of tests/test_posegraph_gpu.py"""
    rng = np.random.default_rng(7)
    truth = P.ring_poses(5, 4.0)
    e = np.concatenate([P.chain_edges(5), [[4, 0]]]).astype(np.int64)
    Z = P.noisy(P.relative(truth, e), rng)
    init = np.stack([x @ P.make_pose(0.05 * rng.standard_normal(3), 0.2 * rng.standard_normal(3)) for x in truth])
    init[0] = truth[0]
    return init, e, Z, P.random_information(rng, len(e))


@pytest.mark.parametrize("kernel", (R.NONE,) + ROBUST)
def test_weight_is_the_derivative_of_rho(kernel):
    c2 = WIDTH * WIDTH
    for s in (0.0, 1e-12, c2 * (1 - 1e-3), c2 * (1 + 1e-3), 1e6):
        rho, w = R.rho_w(kernel, WIDTH, s)
        if s == 0.0:                                          # s <= 0 is the quadratic rule: rho = s, w = 1 exactly
            assert (rho, w) == (0.0, 1.0)
            continue
        # central differences with h = 1e-4 s: the truncation is h^2 rho''' / 6 <= 1e-8 w (rho''' s^2 is of the order of
        # w for these kernels), the rounding 1e-16 rho / h <= 1e-12 rho / s; rho / s <= 1.  h stays on one side of c^2.
        h = 1e-4 * s
        num = (R.rho_w(kernel, WIDTH, s + h)[0] - R.rho_w(kernel, WIDTH, s - h)[0]) / (2 * h)
        assert abs(num - w) <= 1e-7 * max(w, 1e-3), (kernel, s, num, w)
        assert 0.0 < w <= 1.0 and 0.0 < rho <= s
    if kernel == R.NONE:
        assert R.rho_w(kernel, WIDTH, 1e6) == (1e6, 1.0)


def test_huber_is_continuous_at_the_width():
    c2 = WIDTH * WIDTH
    below, at, above = (R.rho_w(R.HUBER, WIDTH, s) for s in (np.nextafter(c2, 0.0), c2, np.nextafter(c2, np.inf)))
    assert at == (c2, 1.0) and below[1] == 1.0
    assert abs(above[0] - at[0]) <= 4 * np.spacing(c2) and abs(above[1] - 1.0) <= 4 * np.spacing(1.0)
    assert below[0] < at[0] <= above[0]


@pytest.mark.parametrize("kernel", ROBUST)
def test_quadratic_rules(kernel):
    for c in (None, 0.0, -1.0, np.nan, np.inf, -np.inf, 1e200, 1e-200):
        assert R.rho_w(kernel, c, 5.0) == (5.0, 1.0), c
    assert R.rho_w(kernel, WIDTH, -1.0) == (-1.0, 1.0)
    assert R.rho_w(R.HUBER, 1e150, 1e6) == (1e6, 1.0)          # c^2 = 1e300 is finite: the quadratic zone of Huber
    # Geman-McClure is the closed form of a switchable constraint: min over sigma of sigma^2 s + c^2 (1 - sigma)^2
    s, c2 = 40.0, WIDTH * WIDTH
    sigma = c2 / (c2 + s)
    assert abs(R.rho_w(R.GEMAN_MCCLURE, WIDTH, s)[0] - (sigma ** 2 * s + c2 * (1 - sigma) ** 2)) <= 1e-12
    assert abs(R.rho_w(R.GEMAN_MCCLURE, WIDTH, s)[1] - sigma ** 2) <= 1e-15


@pytest.mark.parametrize("kernel", ROBUST)
def test_gradient_against_central_differences_of_the_robust_cost(kernel):
    X, e, Z, Om = chain5()
    chi2 = R.edge_chi2(X, e, Z, Om)
    c = float(np.sqrt(np.median(chi2)))                       # edges on both sides of c^2
    scale = np.full(len(e), c)
    scale[0] = 0.0                                            # one edge stays quadratic
    assert (chi2[1:] > c * c).any() and (chi2[1:] < c * c).any()
    lin = R.linearize(X, e, Z, Om, kernel, scale)
    assert lin["weights"][0] == 1.0 and (lin["weights"][1:] < 1.0).any()
    assert abs(lin["cost"] - R.cost(X, e, Z, Om, kernel, scale)) <= 1e-12 * lin["cost"]
    h = 1e-6
    num = np.zeros((len(X), 6))
    for k in range(len(X)):
        for a in range(6):
            d = np.zeros(6)
            d[a] = h
            Xp, Xm = X.copy(), X.copy()
            Xp[k], Xm[k] = P.retract(X[k], d), P.retract(X[k], -d)
            num[k, a] = (R.cost(Xp, e, Z, Om, kernel, scale) - R.cost(Xm, e, Z, Om, kernel, scale)) / (2 * h)
    # h^2 times the third derivative plus the rounding 1e-16 F / h, as for the Jacobians in test_posegraph_cpu.py
    g2 = 2.0 * lin["gradient"]
    assert np.abs(num - g2).max() <= 1e-6 * np.abs(g2).max(), (np.abs(num - g2).max(), np.abs(g2).max())


@pytest.fixture(scope="module")
def lib():
    from neural_spectral_codec_amd import build, _lib
    build.build_hip()
    return _lib.lib()


def test_argument_checks_of_the_robust_entry_points(lib):
    from neural_spectral_codec_amd import _lib
    p = _lib.PoseGraphParams()
    lib.nsc_posegraph_default_params(C.byref(p))
    d = 256                                                   # non-null dummy pointer: nothing may be dereferenced
    need = lib.nsc_posegraph_workspace_bytes(100, 120, C.byref(p))
    assert need > 0 and lib.nsc_posegraph_workspace_bytes(100, 120, None) == need

    def opt(poses=d, n=100, e=d, z=d, om=d, m=120, fixed=d, prm=p, out=d, stats=d, hist=d, ws=d, nbytes=need,
            kernel=R.CAUCHY, scale=d, chi2=d, weight=d):
        return lib.nsc_posegraph_optimize_robust(poses, n, e, z, om, m, fixed, C.byref(prm) if prm is not None else None,
                                                 out, stats, hist, None, ws, nbytes, None, kernel, scale, chi2, weight)

    def lin(poses=d, n=100, e=d, z=d, om=d, m=120, res=d, cost=d, g=d, blocks=d, skipped=d, ws=d, nbytes=need,
            kernel=R.CAUCHY, scale=d, weights=d):
        return lib.nsc_posegraph_linearize_robust(poses, n, e, z, om, m, res, cost, g, blocks, skipped, ws, nbytes, None,
                                                  kernel, scale, weights)

    for bad in (-1, 4, 2 ** 31 - 1, -2 ** 31):
        assert opt(kernel=bad) == -1 and lin(kernel=bad) == -1, bad
        assert opt(kernel=bad, nbytes=need - 1) == -1             # the id is checked before the workspace
    for name in ("poses", "e", "z", "om", "fixed", "prm", "out", "stats", "hist"):
        assert opt(**{name: None}) == -1, name
    for name in ("poses", "e", "z", "om", "res", "cost", "g", "blocks", "skipped"):
        assert lin(**{name: None}) == -1, name
    assert opt(n=-1) == -1 and opt(m=-1) == -1 and lin(n=-1) == -1 and lin(m=-1) == -1
    # the robust arguments are nullable: with every one of them NULL the call gets as far as the workspace check
    for kernel in (R.NONE, R.HUBER, R.CAUCHY, R.GEMAN_MCCLURE):
        assert opt(kernel=kernel, nbytes=need - 1) == -3 and lin(kernel=kernel, nbytes=need - 1) == -3
        assert opt(kernel=kernel, scale=None, chi2=None, weight=None, nbytes=need - 1) == -3
        assert lin(kernel=kernel, scale=None, weights=None, nbytes=need - 1) == -3
        assert opt(kernel=kernel, scale=None, ws=None) == -3 and lin(kernel=kernel, weights=None, ws=None) == -3
    q = _lib.PoseGraphParams()
    lib.nsc_posegraph_default_params(C.byref(q))
    q.lambda0 = 0.0
    assert opt(prm=q) == -1
    q.lambda0, q.max_iteration, q.max_pcg_iterations = 1e-4, 1000, 1000
    assert opt(prm=q) == -2


def test_python_layer_rejects_a_scalar_width_and_an_unknown_kernel(lib):
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval.pose_graph import PoseGraphOptimizer
    with pytest.raises(_lib.NscError):
        PoseGraphOptimizer(kernel="tukey")
    assert PoseGraphOptimizer(kernel="cauchy").kernel == R.CAUCHY and PoseGraphOptimizer().kernel == R.NONE
    for bad in (3.0, np.float64(3.0), np.zeros((4, 1))):
        with pytest.raises(_lib.NscError):
            PoseGraphOptimizer._scale(bad, "cpu", 4)
    with pytest.raises(_lib.NscError):
        PoseGraphOptimizer._scale(np.zeros(3), "cpu", 4)
    assert PoseGraphOptimizer._scale(None, "cpu", 4) is None
