"""Marginal covariances of the pose graph on the MI355X: nsc_posegraph_covariance against the dense inverse of the
restatement (tests/posegraph_cov_restatement.py).  The bar, for columns that report convergence at tau = 1e-10, is
max |joint - Sigma| <= 10 tau |Sigma|_2: b.b = 1, so |x - x*| <= |H^-1| |r| <= |Sigma|_2 tau, and the factor 10 covers the
gap between the recursive and the true residual and a different summation order.  The asymmetry |joint[a,b] -
joint[b,a]^T| is held to the same bar.  Sizes, chunk edges, independence of the columns, determinism, capture,
per-column control on a singular component, robust weights, the coarse space, and the error codes."""
import ctypes as C

import numpy as np
import pytest
import torch

import posegraph_cov_restatement as V
import posegraph_restatement as P
import posegraph_robust_restatement as R
from _posegraph import host, optimizer
from test_posegraph_gpu import chain5

pytestmark = pytest.mark.gpu

CAP = 1000                                   # inner iterations where block-Jacobi runs alone


def tile():
    from neural_spectral_codec_amd import _lib
    return _lib.POSEGRAPH_COV_TILE


def covariance(X, e, Z, Om, nodes, fixed=None, scale=None, kernel=None, L=None, cap=CAP, device=False):
    opt = optimizer(kernel=kernel, coarse_block=L, max_pcg_iterations=cap, pcg_tolerance=V.TAU)
    if device:
        out = host(opt.covariance_device(X, e, Z, Om, nodes, fixed, robust_scale=scale))
        out["converged"] = out["residual"] <= V.TAU
        return out
    return opt.covariance(X, e, Z, Om, nodes, fixed, robust_scale=scale)


def check(what, out, Sigma, nodes, expect_all=True):
    """converged columns against the dense Sigma, and the asymmetry, at the bar; -> worst error / (tau |Sigma|_2)"""
    norm = np.linalg.norm(Sigma, 2)
    ref = V.joint_of(Sigma, nodes)
    conv = out["converged"]                                   # (Q,6): column c of selected pose b
    assert out["joint"].shape == ref.shape and conv.shape == (len(nodes), 6)
    if expect_all:
        assert conv.all(), (what, out["residual"].max(), out["iterations"])
    col = np.broadcast_to(conv[None, :, None, :], ref.shape)
    err = np.abs(out["joint"] - ref)[col].max(initial=0.0) / (V.TAU * norm)
    both = col & np.broadcast_to(conv[:, None, :, None], ref.shape)      # entry (a,b,r,c) and its mirror (b,a,c,r)
    asym = np.abs(out["joint"] - out["joint"].transpose(1, 0, 3, 2))[both].max(initial=0.0) / (V.TAU * norm)
    print(f"{what}: iterations {out['iterations'].min()} .. {out['iterations'].max()}, worst residual "
          f"{np.nanmax(out['residual']):.3g}, error / (tau |Sigma|_2) {err:.3g}, asymmetry / (tau |Sigma|_2) {asym:.3g}, "
          f"|Sigma|_2 {norm:.3g}")
    assert err <= V.BAR and asym <= V.BAR, (what, err, asym)
    return err


def reference(X, e, Z, Om, fixed=None, kernel=R.NONE, scale=None):
    lin, free = V.system(X, e, Z, Om, fixed, kernel, scale)
    return V.dense_sigma(lin["H"], free), free


# ---- 1. the smallest graphs ---------------------------------------------------------------------------------------------

def test_one_pose_two_poses_and_no_edges():
    none = (np.zeros((0, 2), np.int64), np.zeros((0, 4, 4)), np.zeros((0, 6, 6)))
    out = covariance(np.eye(4)[None], *none, [0])
    assert not out["joint"].any() and not out["residual"].any() and not out["iterations"].any()
    assert (out["skipped"], out["outside"], out["not_free"], out["not_converged"]) == (0, 0, 1, 0)
    # two poses, one edge: Sigma_11 = (B^T Omega B)^-1 with B = J_j of the edge
    rng = np.random.default_rng(2)
    X = np.stack([P.make_pose(0.3 * rng.standard_normal(3), rng.standard_normal(3)) for _ in range(2)])
    e = np.array([[0, 1]], np.int64)
    Z = P.noisy(P.relative(X, e), rng, 0.05, 0.2)
    Om = P.random_information(rng, 1)
    B = P.edge_terms(X[0], X[1], Z[0])[2]
    S11 = np.linalg.inv(B.T @ Om[0] @ B)
    out = covariance(X, e, Z, Om, [1, 0])
    assert out["converged"].all() and out["not_free"] == 1 and out["iterations"][1].tolist() == [0] * 6
    assert np.abs(out["joint"][0, 0] - S11).max() <= V.BAR * V.TAU * np.linalg.norm(S11, 2)
    assert not out["joint"][1].any() and not out["joint"][:, 1].any()
    # five poses, no edge: nothing is free
    out = covariance(np.tile(np.eye(4), (5, 1, 1)), *none, [1, 4])
    assert not out["joint"].any() and out["not_free"] == 2 and not out["iterations"].any()


# ---- 2. against the dense inverse -----------------------------------------------------------------------------------------

def _far_start():
    _, init, e, Z, Om = P.far_start()
    return init, e, Z, Om


def _ring(n):
    return lambda: P.drift_ring(n)[1:]


DENSE = {"chain5": (chain5, [1, 2, 4]), "12-ring": (_ring(12), [1, 6, 11]), "far start": (_far_start, [3, 7, 11]),
         "63-ring": (_ring(63), [1, 31, 62]), "64-ring": (_ring(64), [1, 32, 63]), "65-ring": (_ring(65), [1, 32, 64]),
         "tile - 1": (lambda: _ring(tile() - 1)(), [1, -1]), "tile": (lambda: _ring(tile())(), [1, -1]),
         "tile + 1": (lambda: _ring(tile() + 1)(), [1, -1])}


@pytest.mark.parametrize("name", list(DENSE))
def test_dense_comparison(name):
    make, nodes = DENSE[name]
    X, e, Z, Om = make()
    nodes = [n % len(X) for n in nodes]                        # -1: the last pose
    Sigma, free = reference(X, e, Z, Om)
    out = covariance(X, e, Z, Om, nodes)
    check(name, out, Sigma, nodes)
    assert (out["skipped"], out["outside"], out["not_free"], out["not_converged"]) == (0, 0, 0, 0)


# ---- 3. chunks of 64 columns, and what is selected ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ring65():
    X, e, Z, Om = P.drift_ring(65)[1:]
    return X, e, Z, Om, reference(X, e, Z, Om)[0]


@pytest.mark.parametrize("Q", [10, 11, 22, 64])
def test_chunks_of_columns(ring65, Q):
    """60, 66 and 132 columns: one chunk, a second nearly empty, a third; and the cap of 64 poses"""
    X, e, Z, Om, Sigma = ring65
    nodes = list(range(1, 65)) if Q == 64 else [1 + (7 * k) % 64 for k in range(Q)]
    assert len(set(nodes)) == Q
    check(f"65-ring, Q = {Q}", covariance(X, e, Z, Om, nodes), Sigma, nodes)


def test_duplicate_outside_fixed_and_isolated_poses():
    _, X, e, Z, Om = P.drift_ring(12)
    X = np.concatenate([X, X[5:6]])                           # pose 12: no edge touches it
    Sigma, free = reference(X, e, Z, Om)
    assert not free[0] and not free[12] and free[1:12].all()
    nodes = [3, 3, 40, 0, 12, 7, -1]
    out = covariance(X, e, Z, Om, torch.tensor(nodes).cuda(), device=True)
    check("duplicate, outside, fixed, isolated", out, Sigma, nodes)
    assert out["stats"].tolist() == [0, 2, 2, 0]              # skipped, outside, not free, not converged
    j = out["joint"]
    assert j[0].tobytes() == j[1].tobytes() and j[:, 0].tobytes() == j[:, 1].tobytes()      # the duplicate
    for q in (2, 3, 4, 6):
        assert not j[q].any() and not j[:, q].any() and not out["iterations"][q].any() and not out["residual"][q].any()
    alone = covariance(X, e, Z, Om, [3, 7])
    assert j[np.ix_([0, 5], [0, 5])].tobytes() == alone["joint"].tobytes()
    assert out["iterations"][[0, 5]].tolist() == alone["iterations"].tolist()


# ---- 4. the columns are independent ---------------------------------------------------------------------------------------

def test_columns_do_not_depend_on_their_neighbours(ring65):
    X, e, Z, Om, _ = ring65
    abc, ca, b = (covariance(X, e, Z, Om, n) for n in ([5, 33, 64], [64, 5], [33]))
    again = covariance(X, e, Z, Om, [5, 33, 64])
    for k in ("joint", "residual", "iterations"):
        assert abc[k].tobytes() == again[k].tobytes(), k      # two runs agree bitwise
        assert np.ascontiguousarray(abc[k][[2, 0]][:, [2, 0]] if k == "joint" else abc[k][[2, 0]]).tobytes() == \
            ca[k].tobytes(), k
        assert np.ascontiguousarray(abc[k][1:2, 1:2] if k == "joint" else abc[k][1:2]).tobytes() == b[k].tobytes(), k
    assert abc["converged"].all() and len({int(i) for i in abc["iterations"].ravel()}) > 1    # columns stop on their own


def test_captured_replay_equals_eager(ring65):
    from _hipgraph import capture_replay
    X, e, Z, Om, _ = ring65
    cap = 60
    opt = optimizer(coarse_block=8, max_pcg_iterations=cap, pcg_tolerance=V.TAU)
    dev = [torch.from_numpy(a).cuda() for a in (X, e, Z, Om)]
    fixed = torch.zeros(len(X), dtype=torch.uint8, device="cuda")
    fixed[0] = 1
    nodes = torch.tensor([5, 33, 64]).cuda()

    def step():
        return opt.covariance_device(*dev, nodes, fixed=fixed)
    eager, captured, types = capture_replay(step)
    assert set(eager) == {"joint", "residual", "iterations", "stats", "coarse_stats"}
    for k in eager:
        assert torch.equal(eager[k], captured[k]), k
    assert eager["iterations"].min().item() >= 1 and eager["coarse_stats"].tolist() == [9.0, 0.0]
    launches = 5 + 2 + 1 + 5 + 4 + 4 * cap + 1               # include/nsc.h
    kernels = types.pop("kernel", 0)
    assert types.get("memset", 0) == 0 and types.get("memcpy", 0) == 0, types
    assert kernels == launches, (kernels, launches)          # the Python layer adds none


# ---- 5. a column stops on its own -----------------------------------------------------------------------------------------

def test_singular_component_does_not_touch_the_anchored_columns():
    X, e, Z, Om = V.two_components(12, 5)
    lin, free = V.system(X, e, Z, Om)
    assert free[1:].all()                                     # the loose chain is free: nothing fixes it
    Sigma = V.dense_sigma(lin["H"], free & (np.arange(17) < 12))         # H is block diagonal over the components
    out = covariance(X, e, Z, Om, [14, 6], cap=200)
    print("singular columns: iterations", out["iterations"][0], "residual", out["residual"][0])
    assert out["converged"][1].all() and not out["converged"][0].any() and out["not_converged"] == 6
    assert (out["iterations"][0] >= 1).all() and (out["iterations"] <= 200).all()
    check("anchored beside singular", out, Sigma, [14, 6], expect_all=False)
    assert not out["joint"][0, 1].any() and not out["joint"][1, 0].any()      # the components do not meet
    alone = covariance(X, e, Z, Om, [6], cap=200)
    assert out["joint"][1, 1].tobytes() == alone["joint"][0, 0].tobytes()
    assert out["iterations"][1].tolist() == alone["iterations"][0].tolist()


# ---- 6. robust weights ----------------------------------------------------------------------------------------------------

def test_covariance_of_the_weighted_system():
    _, X, e, Z, Om, closures = R.outlier_ring(0)
    scale = R.closure_scale(len(e), closures, 3.0)
    nodes = [10, 40, 63]
    weighted, _ = reference(X, e, Z, Om, kernel=R.CAUCHY, scale=scale)
    quadratic, _ = reference(X, e, Z, Om)
    out = covariance(X, e, Z, Om, nodes, scale=scale, kernel="cauchy")
    check("outlier ring, Cauchy c = 3", out, weighted, nodes)
    gap = np.abs(out["joint"] - V.joint_of(quadratic, nodes)).max() / (V.TAU * np.linalg.norm(quadratic, 2))
    print("distance from the quadratic system's covariance / (tau |Sigma|_2)", gap)
    assert gap > V.BAR
    check("outlier ring, quadratic", covariance(X, e, Z, Om, nodes), quadratic, nodes)


# ---- 7. the coarse space --------------------------------------------------------------------------------------------------

def test_open_chain_needs_the_coarse_space():
    X, e, Z, Om = V.open_chain(257)
    Sigma, _ = reference(X, e, Z, Om)
    nodes = [256, 100]
    out = covariance(X, e, Z, Om, nodes, L=8, cap=300)
    check("257-chain, L = 8", out, Sigma, nodes)
    assert (out["coarse_aggregates"], out["coarse_failed"]) == (33, 0) and out["iterations"].max() < 150
    plain = covariance(X, e, Z, Om, nodes, cap=300)
    norm = np.linalg.norm(Sigma, 2)
    print("257-chain, block-Jacobi alone, 300 iterations: residual of pose 256", plain["residual"][0], "error / (tau "
          "|Sigma|_2)", np.abs(plain["joint"] - V.joint_of(Sigma, nodes)).max() / (V.TAU * norm))
    assert not plain["converged"][0].any() and (plain["iterations"][0] == 300).all() and plain["not_converged"] >= 6


def test_ring_of_65_with_the_coarse_space(ring65):
    X, e, Z, Om, Sigma = ring65
    nodes = [1, 32, 64]
    out = covariance(X, e, Z, Om, nodes, L=8)
    check("65-ring, L = 8", out, Sigma, nodes)
    assert (out["coarse_aggregates"], out["coarse_failed"]) == (9, 0)
    assert out["iterations"].max() < covariance(X, e, Z, Om, nodes)["iterations"].max()


# ---- 8. the C ABI ---------------------------------------------------------------------------------------------------------

def test_error_codes_come_before_any_launch(ring65):
    from neural_spectral_codec_amd import _lib
    L, ptr = _lib.lib(), _lib.ptr
    X, e, Z, Om, _ = ring65
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (X, e, Z, Om)]
    N, E, Q = len(X), len(e), 3
    fixed = torch.zeros(N, dtype=torch.uint8, device="cuda")
    fixed[0] = 1
    nodes = torch.tensor([5, 33, 64]).cuda()
    prm = optimizer(max_pcg_iterations=50).params
    f64 = dict(dtype=torch.float64, device="cuda")
    outs = [torch.full((65, 65, 6, 6), -7.0, **f64), torch.full((65, 6), -7.0, **f64),
            torch.full((65, 6), -7, dtype=torch.int32, device="cuda"), torch.full((4,), -7, dtype=torch.int64, device="cuda")]
    need = int(L.nsc_posegraph_covariance_workspace_bytes(N, E, Q, 0))
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")

    def call(nodes=ptr(nodes), q=Q, nbytes=need):
        return L.nsc_posegraph_covariance(ptr(dev[0]), N, ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), E, ptr(fixed),
                                          C.byref(prm), nodes, q, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]),
                                          ptr(ws), nbytes, _lib.stream_ptr(ws.device), 0, None, 0, None)
    assert call(nbytes=need - 1) == -3 and call(q=65) == -2 and call(nodes=None) == -1
    torch.cuda.synchronize()
    assert all(bool((o == -7).all()) for o in outs) and bool((ws == 0x5A).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((outs[3] == -7).any()) and bool((outs[2].reshape(-1)[:18] >= 1).all())
