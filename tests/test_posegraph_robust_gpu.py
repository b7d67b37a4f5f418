"""Robust kernels of the pose-graph optimiser on the MI355X: nsc_posegraph_linearize_robust and
nsc_posegraph_optimize_robust against the float64 restatement (tests/posegraph_robust_restatement.py), bitwise against
the plain entry points wherever every edge is quadratic, and on a ring with two false closures."""
import numpy as np
import pytest
import torch

import posegraph_restatement as P
import posegraph_robust_restatement as R
from _posegraph import first_fixed, host, optimizer, plain_linearize, plain_optimize, same_bits
from test_posegraph_gpu import assert_poses, chain5, close, graph

pytestmark = pytest.mark.gpu

KERNELS = ("huber", "cauchy", "geman_mcclure")


# ---- 1. linearize against the restatement -------------------------------------------------------------------------

def mixed_scales(X, e, Z, Om):
    """edge k gets [a width that puts it in the tail, one that leaves it in the quadratic zone, 0, NaN][k % 4]: the tail
    width is half the smallest sqrt(chi^2) of the graph, the other twice the largest"""
    chi = np.sqrt(R.edge_chi2(X, e, Z, Om))
    assert chi.min() > 0.0
    return np.array([0.5 * chi.min(), 2.0 * chi.max(), 0.0, np.nan])[np.arange(len(e)) % 4]


@pytest.fixture(scope="module")
def linearize_graphs():
    out = {}
    for name, g in (("5-chain", chain5()), ("N=65", graph(65, 40, 31))):
        out[name] = g + (mixed_scales(*g),)
    return out


@pytest.mark.parametrize("name", ["5-chain", "N=65"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_linearize_matches_restatement(kernel, name, linearize_graphs):
    X, e, Z, Om, scale = linearize_graphs[name]
    ref = R.linearize(X, e, Z, Om, R.KERNELS[kernel], scale)
    robust = np.array([R.is_robust(R.KERNELS[kernel], c, s) for c, s in zip(scale, ref["chi2"])])
    with np.errstate(invalid="ignore"):
        tail = robust & (ref["chi2"] > scale * scale)
    assert tail.any() and (robust & ~tail).any() and (~robust).any()      # both sides of c^2, and quadratic edges
    assert (ref["weights"][tail] < 0.6).all() and (ref["weights"][~robust] == 1.0).all()
    got = host(optimizer(kernel=kernel).linearize(X, e, Z, Om, robust_scale=scale))
    assert got["skipped"][0] == ref["skipped"] == 0
    for k in ("residuals", "gradient", "blocks", "weights"):
        close(got[k], ref[k], (kernel, name, k))
    assert abs(got["cost"][0] - ref["cost"]) <= 1e-6 * ref["cost"], (kernel, name, got["cost"], ref["cost"])
    plain = P.linearize(X, e, Z, Om)
    assert ref["cost"] < 0.9 * plain["cost"]                              # the weighted system is another system
    if kernel == "huber":
        assert (got["weights"][robust & ~tail] == 1.0).all()


# ---- 2. bitwise the plain entry points where every edge is quadratic ------------------------------------------------

QUADRATIC_CASES = [(k, s) for k in KERNELS for s in ("none", "zeros", "not finite or positive")] + [
    (None, "positive"), ("huber", "1e150")]


def quadratic_scale(kind, m):
    if kind == "none":
        return None
    if kind == "zeros":
        return np.zeros(m)
    if kind == "not finite or positive":
        return np.array([-1.0, np.nan, np.inf, -np.inf, -0.0])[np.arange(m) % 5]
    return np.full(m, 1e150 if kind == "1e150" else 2.0)


@pytest.fixture(scope="module")
def plain65():
    X, e, Z, Om = graph(65, 40, 32)
    prm = dict(max_iteration=4, max_pcg_iterations=30)
    return (X, e, Z, Om), prm, plain_linearize(X, e, Z, Om), plain_optimize(X, e, Z, Om, **prm)


@pytest.mark.parametrize("kernel,kind", QUADRATIC_CASES)
def test_quadratic_edges_give_the_bits_of_the_plain_entry_points(kernel, kind, plain65):
    (X, e, Z, Om), prm, lin, opt = plain65
    scale = quadratic_scale(kind, len(e))
    got = host(optimizer(kernel=kernel).linearize(X, e, Z, Om, robust_scale=scale))
    same_bits(lin, got)
    out = host(optimizer(kernel=kernel, **prm).optimize_device(X, e, Z, Om, first_fixed(len(X)), step0=True,
                                                               robust_scale=scale))
    same_bits(opt, out)                                                   # poses, stats, cost_history, step0
    assert opt["stats"][1] >= 1 and opt["stats"][3] >= 1                  # steps were taken
    if scale is not None:
        assert (got["weights"] == 1.0).all() and (out["weights"] == 1.0).all()
        close(out["chi2"], R.edge_chi2(out["poses"], e, Z, Om), "chi2")


# ---- 3. a noise-free chain: every s is 0 ----------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_zero_residuals(kernel):
    """quarter turns and whole-number translations: every product is exact, so every residual is 0 and not 1e-17"""
    turn = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    X = np.tile(np.eye(4), (70, 1, 1))
    for k in range(1, 70):
        X[k, :3, :3] = X[k - 1, :3, :3] @ (turn if k % 3 == 0 else np.eye(3))
        X[k, :3, 3] = X[k - 1, :3, 3] + X[k - 1, :3, :3] @ np.array([2.0, k % 2, 0.0])
    e = np.concatenate([P.chain_edges(70), [[69, 0], [40, 3]]]).astype(np.int64)
    Z = P.relative(X, e)
    Om = P.random_information(np.random.default_rng(1), len(e))
    assert not R.edge_chi2(X, e, Z, Om).any()
    scale = np.full(len(e), 3.0)
    lin = host(optimizer(kernel=kernel).linearize(X, e, Z, Om, robust_scale=scale))
    assert (lin["weights"] == 1.0).all() and lin["cost"][0] == 0.0
    assert not lin["residuals"].any() and not lin["gradient"].any() and np.isfinite(lin["blocks"]).all()
    out = optimizer(kernel=kernel).optimize(X, e, Z, Om, robust_scale=scale)
    assert out["poses"].tobytes() == X.tobytes()
    assert (out["weights"] == 1.0).all() and not out["chi2"].any()
    assert out["cost0"] == out["cost"] == 0.0 and out["converged"] and out["pcg_iterations"] == 0
    assert np.isfinite(out["cost_history"]).all() and np.isfinite(out["step"]) and np.isfinite(out["lambda"])


# ---- 4. the first step ---------------------------------------------------------------------------------------------

def test_first_step_matches_dense_solve_of_the_weighted_system():
    _, X, e, Z, Om = P.drift_ring()
    scale = R.closure_scale(len(e), 1, 3.0)
    lam = P.DEFAULTS["lambda0"]
    lin = R.linearize(X, e, Z, Om, R.CAUCHY, scale, dense=True)
    assert lin["weights"][-1] < 0.1 and (lin["weights"][:-1] == 1.0).all()    # the drift is in the closure's residual
    fixed = first_fixed(len(X))
    free = P.free_nodes(len(X), e, fixed)
    dense = P.dense_step(lin["H"], lin["gradient"], lam, free)
    pcg, its = P.pcg_step(lin["H"], lin["gradient"], lam, free, 1000, 1e-12)
    bar = 10.0 * np.abs(pcg - dense).max()          # the restatement's own PCG against its dense solve, times ten
    out = host(optimizer(kernel="cauchy", max_iteration=1, max_pcg_iterations=1000, pcg_tolerance=1e-12).optimize_device(
        X, e, Z, Om, fixed, step0=True, robust_scale=scale))
    err = np.abs(out["step0"] - dense).max()
    print("restatement PCG iterations", its, "device", out["stats"][3], "bar", bar, "device error", err,
          "largest step entry", np.abs(dense).max())
    assert err <= bar
    assert not out["step0"][0].any()
    unweighted = P.dense_step(P.linearize(X, e, Z, Om, dense=True)["H"], P.linearize(X, e, Z, Om)["gradient"], lam, free)
    assert np.abs(unweighted - dense).max() > 1e3 * bar                     # the quadratic step is another step


# ---- 5. the outlier ring ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def outlier_ring():
    """the graph, and the two quadratic device runs: without the false closures, and with them"""
    g = R.outlier_ring(0)
    truth, init, e, Z, Om, closures = g
    _, ic, ec, Zc, Omc, _ = R.outlier_ring(0, false_closures=False)
    clean = optimizer().optimize(ic, ec, Zc, Omc)
    bent = optimizer().optimize(init, e, Z, Om)
    return g, P.trajectory_error(clean["poses"], truth), P.trajectory_error(bent["poses"], truth)


@pytest.mark.parametrize("kernel,c", [("cauchy", 3.0), ("geman_mcclure", 10.0)])
def test_outlier_ring(kernel, c, outlier_ring):
    (truth, init, e, Z, Om, closures), clean, bent = outlier_ring
    scale = R.closure_scale(len(e), closures, c)
    assert np.count_nonzero(scale) == 6
    ref = R.optimize(init, e, Z, Om, R.KERNELS[kernel], scale)
    # the restatement with PCG rules: 11 (Cauchy, c = 3) and 13 (Geman-McClure, c = 10) accepted steps, none rejected
    assert ref["converged"] and ref["rejected"] == 0 and 11 <= ref["accepted"] <= 13
    out = optimizer(kernel=kernel).optimize(init, e, Z, Om, robust_scale=scale)
    after = P.trajectory_error(out["poses"], truth)
    print(kernel, c, {k: out[k] for k in ("cost0", "cost", "iterations", "accepted", "rejected", "pcg_iterations")},
          "weights on the closures", out["weights"][-closures:], "trajectory error (m): robust", after, "clean quadratic",
          clean, "quadratic with the false closures", bent, "restatement", P.trajectory_error(ref["poses"], truth))
    assert_poses(out["poses"], ref["poses"])
    h = out["cost_history"]
    assert out["converged"] and np.all(np.diff(h) <= 0) and h[0] == out["cost0"] and h[-1] == out["cost"]
    assert abs(out["cost0"] - ref["cost0"]) <= 1e-6 * ref["cost0"] and abs(out["cost"] - ref["cost"]) <= 1e-6 * ref["cost"]
    w = out["weights"]
    assert (w[:len(e) - closures] == 1.0).all()                           # odometry stays quadratic
    assert (w[-closures:-2] > 0.9).all() and (w[-2:] < 0.01).all()        # the ring's and the true closures; the false ones
    close(out["chi2"], R.edge_chi2(out["poses"], e, Z, Om), "chi2")
    close(w, R.edge_weights(out["poses"], e, Z, Om, R.KERNELS[kernel], scale)[1], "weights")
    assert abs(after - clean) <= 0.02
    assert bent > 10.0


# ---- 6. skipped edges -----------------------------------------------------------------------------------------------

def test_skipped_edges_carrying_robust_scales():
    X, e, Z, Om = graph(70, 50, 21)
    n, m = len(X), len(e)
    rng = np.random.default_rng(3)
    scale = np.full(m, float(np.sqrt(np.median(R.edge_chi2(X, e, Z, Om)))))
    scale[::5] = 0.0
    bad = np.array([[3, 3], [-1, 2], [2, n], [n + 5, -7], [0, 2 ** 40], [69, 69], [-2 ** 40, 1]], np.int64)
    at = np.sort(rng.integers(0, m + 1, len(bad)))
    at[0], at[-1] = 0, m                                      # one in front of every edge, one behind, the rest among them
    e2 = np.insert(e, at, bad, axis=0)
    Z2 = np.insert(Z, at, np.tile(np.eye(4) * np.nan, (len(bad), 1, 1)), axis=0)
    Om2 = np.insert(Om, at, np.tile(np.eye(6) * np.nan, (len(bad), 1, 1)), axis=0)
    scale2 = np.insert(scale, at, np.array([1.0, 3.0, np.nan, 0.0, 1e150, 2.0, -1.0]))
    keep = P.valid_edges(n, e2)
    assert keep.sum() == m and np.array_equal(e2[keep], e)
    opt = optimizer(kernel="cauchy", max_iteration=3)
    a, b = host(opt.linearize(X, e, Z, Om, robust_scale=scale)), host(opt.linearize(X, e2, Z2, Om2, robust_scale=scale2))
    assert a["skipped"][0] == 0 and b["skipped"][0] == len(bad)
    assert (a["weights"] < 0.9).any() and (a["weights"][::5] == 1.0).all()
    assert not b["residuals"][~keep].any() and not b["weights"][~keep].any()
    assert b["residuals"][keep].tobytes() == a["residuals"].tobytes()
    assert b["weights"][keep].tobytes() == a["weights"].tobytes()
    same_bits(a, b, ("cost", "gradient", "blocks"))
    fixed = first_fixed(n)
    oa = host(opt.optimize_device(X, e, Z, Om, fixed, robust_scale=scale))
    ob = host(opt.optimize_device(X, e2, Z2, Om2, fixed, robust_scale=scale2))
    assert ob["stats"][7] == len(bad) and oa["stats"][7] == 0 and oa["stats"][1] >= 1
    same_bits(oa, ob, ("poses", "cost_history"))
    assert np.array_equal(np.delete(oa["stats"], 7), np.delete(ob["stats"], 7))
    for k in ("chi2", "weights"):
        assert not ob[k][~keep].any() and ob[k][keep].tobytes() == oa[k].tobytes(), k
    assert (oa["chi2"] > 0.0).all() and (oa["weights"] > 0.0).all()


# ---- 7. repeatability, capture, aliasing, sizes ----------------------------------------------------------------------

def test_two_runs_agree_bitwise(outlier_ring):
    (_, init, e, Z, Om, closures), _, _ = outlier_ring
    scale = R.closure_scale(len(e), closures, 3.0)
    opt = optimizer(kernel="cauchy", max_iteration=6)
    a = host(opt.optimize_device(init, e, Z, Om, step0=True, robust_scale=scale))
    b = host(opt.optimize_device(init, e, Z, Om, step0=True, robust_scale=scale))
    same_bits(a, b)
    assert set(a) == {"poses", "stats", "cost_history", "step0", "chi2", "weights"} and a["stats"][1] >= 1
    a, b = host(opt.linearize(init, e, Z, Om, robust_scale=scale)), host(opt.linearize(init, e, Z, Om, robust_scale=scale))
    same_bits(a, b)


def test_alias_of_input_and_output(outlier_ring):
    (_, init, e, Z, Om, closures), _, _ = outlier_ring
    scale = R.closure_scale(len(e), closures, 3.0)
    opt = optimizer(kernel="cauchy", max_iteration=5)
    separate = host(opt.optimize_device(init, e, Z, Om, robust_scale=scale))
    X = torch.from_numpy(init).cuda()
    aliased = opt.optimize_device(X, e, Z, Om, poses_out=X, robust_scale=scale)
    assert aliased["poses"].data_ptr() == X.data_ptr()
    same_bits(separate, host(aliased))
    assert separate["stats"][1] >= 1 and (separate["weights"][-2:] < 1.0).all()


def test_captured_replay_equals_eager(outlier_ring):
    from _hipgraph import capture_replay
    (_, init, e, Z, Om, closures), _, _ = outlier_ring
    prm = dict(max_iteration=4, max_pcg_iterations=30)
    opt = optimizer(kernel="geman_mcclure", **prm)
    dev = [torch.from_numpy(a).cuda() for a in (init, e, Z, Om)]
    scale = torch.from_numpy(R.closure_scale(len(e), closures, 10.0)).cuda()
    fixed = torch.zeros(len(init), dtype=torch.uint8, device="cuda")
    fixed[0] = 1

    def step():
        return opt.optimize_device(*dev, fixed=fixed, step0=True, robust_scale=scale)
    eager, cap, types = capture_replay(step)
    assert set(eager) == {"poses", "stats", "cost_history", "step0", "chi2", "weights"}
    for k in eager:
        assert torch.equal(eager[k], cap[k]), k
    assert eager["stats"][1].item() >= 1 and (eager["weights"][-2:] < 1.0).all()
    launches = 5 + 1 + 3 + prm["max_iteration"] * (8 + 4 * prm["max_pcg_iterations"]) + 1 + 1    # include/nsc.h
    kernels = types.pop("kernel", 0)
    assert types.get("memset", 0) == 0 and types.get("memcpy", 0) == 0, types
    assert kernels == launches, (kernels, launches)          # the Python layer adds none


SIZES = {"N=1": lambda: graph(1, 0, 4), "N=2": lambda: graph(2, 0, 5, reverse=True), "N=63": lambda: graph(63, 40, 6),
         "N=64": lambda: graph(64, 40, 7), "N=65": lambda: graph(65, 40, 8),
         "E=0": lambda: (graph(5, 0, 10)[0], np.zeros((0, 2), np.int64), np.zeros((0, 4, 4)), np.zeros((0, 6, 6)))}


@pytest.mark.parametrize("name", list(SIZES))
def test_sizes(name):
    X, e, Z, Om = SIZES[name]()
    chi = np.sqrt(R.edge_chi2(X, e, Z, Om))
    scale = np.full(len(e), float(np.median(chi))) if len(e) else np.zeros(0)
    opt = optimizer(kernel="cauchy", max_iteration=3)
    ref = R.linearize(X, e, Z, Om, R.CAUCHY, scale)
    got = host(opt.linearize(X, e, Z, Om, robust_scale=scale))
    for k in ("residuals", "gradient", "blocks", "weights"):
        close(got[k], ref[k], (name, k))
    assert abs(got["cost"][0] - ref["cost"]) <= 1e-6 * max(ref["cost"], 1e-300)
    out = optimizer(kernel="cauchy", max_iteration=3).optimize(X, e, Z, Om, robust_scale=scale)
    assert out["chi2"].shape == out["weights"].shape == (len(e),)
    assert np.isfinite(out["poses"]).all() and np.isfinite(out["cost_history"]).all()
    assert np.isfinite(out["chi2"]).all() and ((out["weights"] > 0.0) & (out["weights"] <= 1.0)).all()
    assert out["cost"] <= out["cost0"] and out["skipped"] == 0
    if len(e) == 0 or len(X) == 1:
        assert out["poses"].tobytes() == np.asarray(X).tobytes() and out["cost"] == 0.0
    else:
        assert out["accepted"] >= 1
        close(out["weights"], R.edge_weights(out["poses"], e, Z, Om, R.CAUCHY, scale)[1], (name, "final weights"))


# ---- 8. one evaluation of an edge --------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_one_edge_evaluation(kernel):
    """Every kernel takes an edge's s = r^T Omega r, rho and w from one device function, so what linearize and optimize
    say about the same edges at the same poses is the same bits: the weights, and the cost in the three places it comes
    out.  65 poses and 106 edges: two workgroups of edges and of nodes, two skipped edges among the counted ones, a width
    on every second edge."""
    X, e, Z, Om = graph(65, 40, 8)
    n = len(X)
    at = np.array([20, 70])
    e = np.insert(e, at, np.array([[7, 7], [3, n]], np.int64), axis=0)
    Z = np.insert(Z, at, np.tile(np.eye(4) * np.nan, (2, 1, 1)), axis=0)
    Om = np.insert(Om, at, np.tile(np.eye(6) * np.nan, (2, 1, 1)), axis=0)
    keep = P.valid_edges(n, e)
    assert keep.sum() == len(e) - 2 and len(e) > 64 and n > 64
    widths = np.arange(len(e)) % 2 == 0
    chi2 = R.edge_chi2(X, e, Z, Om)
    scale = np.where(widths, np.sqrt(np.median(chi2[keep & widths])), 0.0)     # half the edges with a width in Huber's tail
    ref = R.edge_weights(X, e, Z, Om, R.KERNELS[kernel], scale)[1]
    assert (ref[keep] < 1.0).sum() >= 10 and (ref[keep] == 1.0).sum() >= 10

    lin = host(optimizer(kernel=kernel).linearize(X, e, Z, Om, robust_scale=scale))
    out = host(optimizer(kernel=kernel, max_iteration=0).optimize_device(X, e, Z, Om, first_fixed(n), robust_scale=scale))
    assert lin["skipped"][0] == out["stats"][7] == 2
    print(kernel, "cost", lin["cost"][0], out["stats"][4], out["cost_history"][0], "weights < 1:",
          (lin["weights"] < 1.0).sum(), "differing weights:", (lin["weights"] != out["weights"]).sum())
    assert lin["weights"].tobytes() == out["weights"].tobytes()
    assert lin["cost"][:1].tobytes() == out["stats"][4:5].tobytes() == out["cost_history"][:1].tobytes()
    r = lin["residuals"]
    want = np.array([r[k] @ P.sym_upper(Om[k]) @ r[k] if keep[k] else 0.0 for k in range(len(e))])
    close(out["chi2"], want, "chi2")
    assert not out["chi2"][~keep].any() and not out["weights"][~keep].any()
    close(out["weights"], ref, "weights")
