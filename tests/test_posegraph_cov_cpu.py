"""Marginal covariances of the pose graph without a device: the restatement (tests/posegraph_cov_restatement.py) against
itself -- column-wise PCG against the dense inverse, G against finite differences of ``retract`` -- the two host helpers
of retrieval/pose_graph.py against it, the argument checks of nsc_posegraph_covariance and of the Python layer, and the
exports."""
import ctypes as C

import numpy as np
import pytest

import posegraph_cov_restatement as V
import posegraph_restatement as P


# ---- the restatement ----------------------------------------------------------------------------------------------------

def test_restated_columns_reach_the_dense_inverse():
    """drift_ring(12), nodes [1, 6, 11]: block-Jacobi PCG to 1e-10 lands far inside the device's bar"""
    _, X, e, Z, Om = P.drift_ring(12)
    lin, free = V.system(X, e, Z, Om)
    assert np.array_equal(free, ~V.first_fixed(12))
    Sigma = V.dense_sigma(lin["H"], free)
    nodes = [1, 6, 11]
    joint, its = V.pcg_columns(lin, free, nodes)
    ratio = np.abs(joint - V.joint_of(Sigma, nodes)).max() / (V.TAU * np.linalg.norm(Sigma, 2))
    print("12-ring: iterations", its.min(), "..", its.max(), "worst error over tau |Sigma|_2", ratio)
    assert ratio <= 1e-2 and its.max() < 200
    assert not Sigma[:6].any() and not Sigma[:, :6].any()      # the fixed pose
    # Sigma is what it claims to be: H Sigma = I on the free poses
    m = np.repeat(free, 6)
    assert np.abs((lin["H"].toarray() @ Sigma)[np.ix_(m, m)] - np.eye(m.sum())).max() <= 1e-9


def test_two_level_columns_on_the_open_chain():
    """257-pose open chain, aggregates of 8: the columns of the far end converge in under 100 iterations"""
    X, e, Z, Om = V.open_chain(257)
    lin, free = V.system(X, e, Z, Om)
    Sigma = V.dense_sigma(lin["H"], free)
    nodes = [256]
    joint, its = V.pcg_columns(lin, free, nodes, X, 8, 300)
    ratio = np.abs(joint - V.joint_of(Sigma, nodes)).max() / (V.TAU * np.linalg.norm(Sigma, 2))
    print("257-chain, L = 8: iterations", its.min(), "..", its.max(), "worst error over tau |Sigma|_2", ratio)
    assert ratio <= 1e-1 and its.max() < 100


@pytest.mark.parametrize("seed", [0, 1])
def test_relative_jacobian_is_the_derivative_of_retract(seed):
    rng = np.random.default_rng(seed)
    Xi = P.make_pose(0.8 * rng.standard_normal(3), 10.0 * rng.standard_normal(3))
    Xj = P.make_pose(0.8 * rng.standard_normal(3), 10.0 * rng.standard_normal(3))
    G, fd = V.relative_jacobian(Xi, Xj), V.relative_jacobian_fd(Xi, Xj)
    # central differences at h = 1e-6 on entries of size <= 30 (the lever arm): truncation h^2, rounding 1e-16 * 30 / h
    assert np.abs(G - fd).max() <= 1e-7, np.abs(G - fd).max()
    assert np.abs(G[:, :6]).max() > 3.0                          # the lever arm is in it


# ---- the host helpers -----------------------------------------------------------------------------------------------------

def _pair(rng, lever):
    """two poses `lever` metres apart sideways (an other-lane closure) with a random SPD joint covariance"""
    Xi = P.make_pose(0.3 * rng.standard_normal(3), 5.0 * rng.standard_normal(3))
    Xj = Xi @ P.make_pose([0.02, -0.01, np.pi - 0.1], [0.4, lever, 0.05])
    A = rng.standard_normal((12, 12))
    S = 1e-3 * (A @ A.T + 12.0 * np.eye(12))
    return Xi, Xj, S.reshape(2, 6, 2, 6).transpose(0, 2, 1, 3)


@pytest.mark.parametrize("lever", [0.0, 3.5])
def test_helpers_match_the_restatement(lever):
    from neural_spectral_codec_amd.retrieval import closure_mahalanobis, relative_covariance
    rng = np.random.default_rng(11)
    Xi, Xj, pair = _pair(rng, lever)
    want = V.relative_covariance(pair, Xi, Xj)
    got = relative_covariance(pair, Xi, Xj)
    assert got.shape == (6, 6) and np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    assert np.abs(got - got.T).max() <= 1e-15 * np.abs(got).max() and np.linalg.eigvalsh(0.5 * (got + got.T)).min() > 0
    # against sampling-free first principles: the covariance of G (delta_i, delta_j)
    G = V.relative_jacobian_fd(Xi, Xj)
    S = pair.transpose(0, 2, 1, 3).reshape(12, 12)
    assert np.abs(got - G @ S @ G.T).max() <= 1e-6 * np.abs(got).max()
    if lever:
        # the rotation of pose i reaches the translation of A through the lever arm: |[t]x R|_F = sqrt(2) |t|, |t| >= lever
        assert np.linalg.norm(V.relative_jacobian(Xi, Xj)[3:, :3]) >= np.sqrt(2.0) * lever
    Z = P.inv_se3(Xi) @ Xj @ P.make_pose([0.01, 0.02, -0.015], [0.1, -0.2, 0.05])
    Om = P.random_information(rng, 1)[0] * 20.0
    d2, ref = closure_mahalanobis(Z, Om, Xi, Xj, got), V.closure_mahalanobis(Z, Om, Xi, Xj, want)
    assert abs(d2 - ref) <= 1e-12 * ref and d2 > 0.0
    # no prior uncertainty: the plain chi^2 of the edge; more uncertainty: a smaller distance
    r = P.residual(Xi, Xj, Z)
    assert abs(closure_mahalanobis(Z, Om, Xi, Xj, np.zeros((6, 6))) - r @ Om @ r) <= 1e-10 * (r @ Om @ r)
    assert closure_mahalanobis(Z, Om, Xi, Xj, 4.0 * got) < d2 < r @ Om @ r


def test_exports():
    import neural_spectral_codec_amd.retrieval as Rt
    from neural_spectral_codec_amd import _lib
    for name in ("relative_covariance", "closure_mahalanobis", "PoseGraphOptimizer"):
        assert name in Rt.__all__ and callable(getattr(Rt, name))
    assert callable(Rt.PoseGraphOptimizer.covariance) and callable(Rt.PoseGraphOptimizer.covariance_device)
    assert _lib.POSEGRAPH_MAX_COV_NODES == 64 and _lib.POSEGRAPH_COV_STATS == len(_lib.POSEGRAPH_COV_STAT_NAMES) == 4
    assert "nsc_posegraph_covariance" in _lib.SYMBOLS and "nsc_posegraph_covariance_workspace_bytes" in _lib.SYMBOLS
    for text in (Rt.pose_graph.__doc__, Rt.PoseGraphOptimizer.covariance.__doc__):
        assert "relative_covariance" in text and "closure_mahalanobis" in text
    assert "chi^2" in Rt.closure_mahalanobis.__doc__ and "6 degrees" in Rt.closure_mahalanobis.__doc__


# ---- the C ABI ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from neural_spectral_codec_amd import build, _lib
    build.build_hip()
    return _lib.lib()


def test_argument_checks_without_a_device(lib):
    from neural_spectral_codec_amd import _lib
    p = _lib.PoseGraphParams()
    lib.nsc_posegraph_default_params(C.byref(p))
    d = 256                                                   # non-null dummy pointer: nothing may be dereferenced
    size = lib.nsc_posegraph_covariance_workspace_bytes
    plain, coarse = lib.nsc_posegraph_workspace_bytes(100, 120, None), lib.nsc_posegraph_coarse_workspace_bytes(100, 120, 8)
    need, need8 = size(100, 120, 11, 0), size(100, 120, 11, 8)
    # five vectors (N,6,R_pad) with R_pad = 128 for the 66 columns of 11 poses, behind the optimiser's layout
    assert need - plain >= 8 * 5 * 100 * 6 * 128 and need8 - coarse >= 8 * (5 * 100 * 6 * 128 + 78 * 128)
    assert size(100, 120, 10, 0) < need == size(100, 120, 21, 0) < size(100, 120, 22, 0)      # chunks of 64 columns
    assert size(100, 120, 0, 0) >= plain and size(100, 120, 64, 0) > 0 and size(100, 120, 65, 0) == 0
    assert size(-1, 0, 1, 0) == 0 and size(1, -1, 1, 0) == 0 and size(1, 1, -1, 0) == 0
    assert size(100, 120, 1, 1) == 0 and size(100, 120, 1, -1) == 0 and size(1025, 1200, 1, 8) == 0

    def cov(poses=d, n=100, e=d, z=d, om=d, m=120, fixed=d, prm=p, nodes=d, q=11, joint=d, res=d, its=d, stats=d, ws=d,
            nbytes=need8, kernel=0, block=8):
        return lib.nsc_posegraph_covariance(poses, n, e, z, om, m, fixed, C.byref(prm) if prm is not None else None,
                                            nodes, q, joint, res, its, stats, ws, nbytes, None, kernel, None, block, None)

    for name in ("poses", "e", "z", "om", "fixed", "prm", "nodes", "joint", "res", "its", "stats"):
        assert cov(**{name: None}) == -1, name
    assert cov(n=-1) == -1 and cov(m=-1) == -1 and cov(q=-1) == -1
    assert cov(block=-1) == -1 and cov(block=1) == -1 and cov(kernel=4) == -1
    assert cov(q=65) == -2 and cov(n=1025) == -2              # the cap on selected poses; too many aggregates
    assert cov(nbytes=need8 - 1) == -3 and cov(ws=None) == -3
    assert cov(block=0, nbytes=need - 1) == -3 and cov(block=8, nbytes=need) == -3
    q = _lib.PoseGraphParams()
    lib.nsc_posegraph_default_params(C.byref(q))
    q.lambda0 = 0.0                                           # not used here, but params_ok still applies
    assert cov(prm=q) == -1
    # the launch cap follows the header's formula: 18 + 4 max_pcg_iterations with the coarse space, 3 without
    lib.nsc_posegraph_default_params(C.byref(q))
    q.max_pcg_iterations = (_lib.POSEGRAPH_MAX_LAUNCHES - 18) // 4 + 1
    assert cov(prm=q) == -2 and cov(prm=q, block=0, nbytes=need - 1) == -3
    q.max_pcg_iterations -= 1
    assert cov(prm=q, nbytes=need8 - 1) == -3                 # past the cap check, stopped by the next one


def test_python_refuses_what_the_host_can_see(lib):
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import PoseGraphOptimizer
    _, X, e, Z, Om = P.drift_ring(12)
    opt = PoseGraphOptimizer()
    for bad in ([12], [-1], [0, 3, 99], np.arange(65) % 12):
        with pytest.raises(_lib.NscError):
            opt.covariance(X, e, Z, Om, bad)
    with pytest.raises(_lib.NscError):
        import torch
        opt.covariance(torch.from_numpy(X), e, Z, Om, [1])     # host tensors: there is no CPU fallback
