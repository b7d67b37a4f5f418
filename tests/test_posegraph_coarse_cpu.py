"""The two-level preconditioner of the pose-graph optimiser without a device: the sparse float64 restatement
(tests/posegraph_coarse_restatement.py) -- the basis, the preconditioner's symmetry and definiteness, its PCG against the
dense solve with the iteration counts it was chosen by, the 1 025-pose ring that block-Jacobi cannot close within the
default caps -- and the argument checks of nsc_posegraph_optimize_coarse and of the Python layer."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import posegraph_coarse_restatement as Cr
import posegraph_restatement as P
from _posegraph import first_fixed

LAMBDA = P.DEFAULTS["lambda0"]
# inner iterations to |r| <= 1e-12 |g| at lambda = 1e-4 on drift_ring(n): block-Jacobi, and with aggregates of 8 poses
TABLE = {64: (341, 97), 65: (344, 85), 257: (1210, 79)}


# ---- the basis ------------------------------------------------------------------------------------------------------

def test_the_basis_is_rigid_motions():
    """A rigid motion of a whole aggregate changes no residual of an edge inside it, so H of those edges annihilates P:
    J_i Ad(X_i^-1 X_ref) + J_j Ad(X_j^-1 X_ref) = 0.  With the adjoint inverted, or the two frames swapped, it does not."""
    rng = np.random.default_rng(1)
    n = 8
    X = np.stack([P.make_pose(0.6 * rng.standard_normal(3), 5.0 * rng.standard_normal(3)) for _ in range(n)])
    e = P.chain_edges(n)
    Z = P.relative(X, e)                                       # noise-free
    H = Cr.linearize(X, e, Z, P.random_information(rng, len(e)))["H"]
    free = np.ones(n, bool)
    Pm = Cr.prolongation(X, free, n)                           # one aggregate, X_ref = X_0
    assert Pm.shape == (6 * n, 6)
    scale = np.abs(H).max() * np.abs(Pm).max()
    assert np.abs((H @ Pm).toarray()).max() <= 1e-11 * scale   # sums of 12 products, each to 1e-16 of `scale`
    inverted = np.concatenate([np.linalg.inv(P.adjoint(P.inv_se3(X[k]) @ X[0])) for k in range(n)])
    swapped = np.concatenate([P.adjoint(X[k] @ P.inv_se3(X[0])) for k in range(n)])
    for wrong in (inverted, swapped):
        assert np.abs(H @ wrong).max() > 1e-3 * scale
    # the block of the reference pose itself is the identity (R^T R, to rounding), and a pose that is not free has a zero row
    assert np.abs(Pm[:6].toarray() - np.eye(6)).max() <= 1e-15
    free[3] = False
    assert not Cr.prolongation(X, free, n)[18:24].toarray().any()


def test_preconditioner_is_symmetric_positive_definite():
    """65-ring, aggregates of 8 (the last one a single pose), poses 8..15 fixed: aggregate 1 has no free pose and gets
    the identity block, decoupled from the others"""
    n, L = 65, 8
    _, X, e, Z, Om = P.drift_ring(n)
    fixed = np.zeros(n, bool)
    fixed[8:16] = True
    lin = Cr.linearize(X, e, Z, Om)
    free = Cr.free_nodes(n, e, fixed, lin["blocks"], LAMBDA)
    assert np.array_equal(free, ~fixed)
    M = Cr.Preconditioner(lin["H"], lin["blocks"], LAMBDA, free, X, L)
    assert not M.failed and M.Ac.shape == (54, 54)
    assert np.array_equal(M.Ac[6:12, 6:12], np.eye(6))
    assert not M.Ac[6:12, :6].any() and not M.Ac[6:12, 12:].any() and not M.Ac[:6, 6:12].any()
    D = M.dense()
    m = np.repeat(free, 6)
    assert not D[~m].any() and not D[:, ~m].any()              # nothing reaches a pose that is not free
    D = D[np.ix_(m, m)]
    assert np.abs(D - D.T).max() <= 1e-12 * np.abs(D).max()
    w = np.linalg.eigvalsh(0.5 * (D + D.T))
    assert w.min() > 0.0
    # and it is an approximate inverse: the spectrum of M^-1 A is far narrower than that of B^-1 A
    A = (lin["H"] + LAMBDA * sp.diags(lin["H"].diagonal())).toarray()[np.ix_(m, m)]
    B = Cr.Preconditioner(lin["H"], lin["blocks"], LAMBDA, free).dense()[np.ix_(m, m)]

    def condition(Minv):
        Lc = np.linalg.cholesky(A)
        ev = np.linalg.eigvalsh(Lc.T @ Minv @ Lc)
        return ev.max() / ev.min()
    assert condition(D) < 0.1 * condition(B)


# ---- PCG against the dense solve ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", list(TABLE))
def test_restated_pcg_reaches_the_dense_solve(n):
    _, X, e, Z, Om = P.drift_ring(n)
    lin = Cr.linearize(X, e, Z, Om)
    free = Cr.free_nodes(n, e, first_fixed(n), lin["blocks"], LAMBDA)
    dense = Cr.dense_step(lin["H"], lin["gradient"], LAMBDA, free)
    its = {}
    for L in (None, 8):
        d, its[L], failed = Cr.pcg_step(lin["H"], lin["gradient"], lin["blocks"], LAMBDA, free, 5000, 1e-12, X, L)
        dist = np.abs(d - dense).max() / np.abs(dense).max()
        print(n, "L", L, "iterations", its[L], "relative distance from the dense solve", dist)
        assert not failed
        if L is not None:
            assert dist <= 1e-11
    assert (its[None], its[8]) == TABLE[n]
    assert 2 * its[8] < its[None]


def test_sparse_restatement_is_the_dense_one():
    """on the 64-ring the sparse linearisation and block-Jacobi PCG are posegraph_restatement's"""
    _, X, e, Z, Om = P.drift_ring()
    a, b = Cr.linearize(X, e, Z, Om), P.linearize(X, e, Z, Om, dense=True)
    assert np.abs(a["H"].toarray() - b["H"]).max() <= 1e-12 * np.abs(b["H"]).max()
    assert np.abs(a["gradient"] - b["gradient"]).max() <= 1e-12 * np.abs(b["gradient"]).max()
    free = P.free_nodes(64, e, first_fixed(64))
    da, ia, _ = Cr.pcg_step(a["H"], a["gradient"], a["blocks"], LAMBDA, free, 100, 1e-6)
    db, ib = P.pcg_step(b["H"], b["gradient"], LAMBDA, free, 100, 1e-6)
    assert ia == ib and np.abs(da - db).max() <= 1e-9 * np.abs(db).max()


# ---- the ring that block-Jacobi does not close within the caps ------------------------------------------------------

@pytest.fixture(scope="module")
def ring1025():
    truth, X, e, Z, Om = P.drift_ring(1025, 0)
    return truth, X, Cr.optimize(X, e, Z, Om), Cr.optimize(X, e, Z, Om, max_pcg_iterations=100000), \
        Cr.optimize(X, e, Z, Om, L=16)


def test_ring_of_1025_converges_within_the_default_caps(ring1025):
    truth, X, capped, uncapped, coarse = ring1025
    for name, o in (("block-Jacobi, default caps", capped), ("block-Jacobi, inner cap 100 000", uncapped),
                    ("aggregates of 16, default caps", coarse)):
        print(name, "converged", o["converged"], "cost", repr(o["cost"]), "accepted", o["accepted"], "inner iterations",
              o["pcg_iterations"], "trajectory error (m)", P.trajectory_error(o["poses"], truth))
    assert not capped["converged"] and capped["cost"] > 2.0 * uncapped["cost"]
    assert uncapped["converged"] and coarse["converged"] and coarse["coarse_failed"] == 0
    assert coarse["coarse_aggregates"] == 65 and coarse["rejected"] == 0
    # both runs stop once an accepted step gains less than relative_cost = 1e-9 of F, a step at which Levenberg-Marquardt
    # gains at least as much as all later steps together: each cost is within 1e-9 F of the minimum; the bar is 1e-8
    assert abs(coarse["cost"] - uncapped["cost"]) <= 1e-8 * uncapped["cost"]
    assert np.all(np.diff(coarse["cost_history"]) <= 0)


# ---- the C ABI --------------------------------------------------------------------------------------------------------

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
    size = lib.nsc_posegraph_coarse_workspace_bytes
    plain = lib.nsc_posegraph_workspace_bytes(100, 120, None)
    need = size(100, 120, 8)
    assert size(100, 120, 0) == plain and need > plain and size(100, 120, 200) > plain
    # T (36 N), three (6 n_a)^2 matrices, r_c and the partials: the 13 aggregates of 100 poses
    assert need - plain >= 8 * (36 * 100 + 3 * 78 * 78 + 78 + 2 * 13)
    assert size(100, 120, 1) == 0 and size(100, 120, -1) == 0 and size(-1, 0, 8) == 0 and size(0, -1, 8) == 0
    assert size(1000, 1200, 2) == 0 and size(1024, 1200, 8) > 0 and size(1025, 1200, 8) == 0    # 128 aggregates at most
    assert _lib.POSEGRAPH_MAX_AGGREGATES == 128

    def opt(poses=d, n=100, e=d, z=d, om=d, m=120, fixed=d, prm=p, out=d, stats=d, hist=d, ws=d, nbytes=need, block=8,
            cstats=d):
        return lib.nsc_posegraph_optimize_coarse(poses, n, e, z, om, m, fixed, C.byref(prm) if prm is not None else None,
                                                 out, stats, hist, None, ws, nbytes, None, 0, None, None, None, block,
                                                 cstats)

    for name in ("poses", "e", "z", "om", "fixed", "prm", "out", "stats", "hist"):
        assert opt(**{name: None}) == -1, name
    assert opt(n=-1) == -1 and opt(m=-1) == -1
    assert opt(block=-1) == -1 and opt(block=1) == -1 and opt(block=-2 ** 31) == -1
    assert opt(n=1000, block=2) == -2 and opt(n=1025, block=8) == -2                # too many aggregates
    assert opt(nbytes=need - 1) == -3 and opt(ws=None) == -3
    assert opt(block=0, nbytes=plain - 1) == -3 and opt(block=8, nbytes=plain) == -3
    assert lib.nsc_posegraph_optimize_coarse(d, 100, d, d, d, 120, d, C.byref(p), d, d, d, None, d, need, None, 7, None,
                                             None, None, 8, d) == -1                # kernel id
    q = _lib.PoseGraphParams()
    lib.nsc_posegraph_default_params(C.byref(q))
    q.lambda0 = 0.0
    assert opt(prm=q) == -1
    # the launch cap follows the header's formula: max_iteration (14 + 5 max_pcg_iterations) with the coarse space
    lib.nsc_posegraph_default_params(C.byref(q))
    q.max_iteration, q.max_pcg_iterations = 20, 9998
    assert 20 * (14 + 5 * 9998) > _lib.POSEGRAPH_MAX_LAUNCHES >= 20 * (8 + 4 * 9998)
    assert opt(prm=q) == -2
    q.max_pcg_iterations = 9997
    assert 20 * (14 + 5 * 9997) <= _lib.POSEGRAPH_MAX_LAUNCHES
    assert opt(prm=q, nbytes=need - 1) == -3                  # past the cap check, stopped by the next one


def test_python_refuses_an_unknown_coarse_block(lib):
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import PoseGraphOptimizer
    for bad in ("foo", "Auto", 1, 0, -3, 2.5, True, (8,)):
        with pytest.raises(_lib.NscError):
            PoseGraphOptimizer(coarse_block=bad)
    for good, n, want in ((None, 4541, 0), (8, 4541, 8), (np.int64(16), 100, 16), ("auto", 4541, 71), ("auto", 100, 8),
                          ("auto", 513, 9)):
        assert PoseGraphOptimizer(coarse_block=good)._coarse(n) == want
