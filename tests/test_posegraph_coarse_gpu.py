"""The two-level preconditioner of the pose-graph optimiser on the MI355X: nsc_posegraph_optimize_coarse against the sparse
float64 restatement (tests/posegraph_coarse_restatement.py) -- the first step against the dense solve for every shape of
aggregate, the inner iterations it saves, full optimisations (the 1 025-pose ring that block-Jacobi does not close within
the default caps among them), bitwise equivalence with the robust entry point at coarse_block = 0, determinism, capture,
aliasing, fixed / skipped / degenerate inputs and a robust kernel."""
import numpy as np
import pytest
import torch

import posegraph_coarse_restatement as Cr
import posegraph_restatement as P
import posegraph_robust_restatement as R
from _posegraph import abi_optimize, first_fixed, host, optimizer, same_bits
from test_posegraph_gpu import assert_poses, chain5, graph

pytestmark = pytest.mark.gpu

LAMBDA = P.DEFAULTS["lambda0"]
BLOCK_JACOBI = {64: 341, 257: 1210}          # the restatement's inner iterations to 1e-12 (test_posegraph_coarse_cpu.py)


# ---- the first step -----------------------------------------------------------------------------------------------

_SYSTEMS = {}


def system(name):
    """graph, fixed mask, the restatement's linearisation at the start, free poses and the dense step; made once"""
    if name not in _SYSTEMS:
        if name == "5-chain":
            X, e, Z, Om = chain5()
        else:
            _, X, e, Z, Om = P.drift_ring(int(name.split("-")[0]))
        fixed = first_fixed(len(X))
        lin = Cr.linearize(X, e, Z, Om)
        free = Cr.free_nodes(len(X), e, fixed, lin["blocks"], LAMBDA)
        _SYSTEMS[name] = (X, e, Z, Om, fixed, lin, free, Cr.dense_step(lin["H"], lin["gradient"], LAMBDA, free))
    return _SYSTEMS[name]


def first_step(X, e, Z, Om, fixed, L, **kw):
    return host(optimizer(coarse_block=L, max_iteration=1, max_pcg_iterations=1000, pcg_tolerance=1e-12, **kw)
                .optimize_device(X, e, Z, Om, fixed, step0=True))


def check_first_step(what, X, e, Z, Om, fixed, lin, free, dense, L, out):
    """the device's first step against the dense solve of the damped system: the bar is ten times the distance of the
    restatement's own two-level PCG from that solve"""
    pcg, its, failed = Cr.pcg_step(lin["H"], lin["gradient"], lin["blocks"], LAMBDA, free, 1000, 1e-12, X, L)
    assert not failed
    bar = 10.0 * np.abs(pcg - dense).max()
    err = np.abs(out["step0"] - dense).max()
    print(what, "L", L, "restatement PCG iterations", its, "device", out["stats"][3], "bar", bar, "device error", err,
          "largest step entry", np.abs(dense).max(), "coarse stats", out["coarse_stats"])
    assert err <= bar
    assert not out["step0"][~free].any()
    assert out["coarse_stats"][0] == Cr.aggregates(len(X), L) and out["coarse_stats"][1] == 0
    return its


FIRST_STEPS = [("5-chain", 2), ("64-ring", 8), ("65-ring", 8), ("257-ring", 8), ("257-ring", 64), ("257-ring", 128),
               ("65-ring", 1000)]


@pytest.mark.parametrize("name,L", FIRST_STEPS)
def test_first_step_matches_dense_solve(name, L):
    X, e, Z, Om, fixed, lin, free, dense = system(name)
    out = first_step(X, e, Z, Om, fixed, L)
    its = check_first_step(name, X, e, Z, Om, fixed, lin, free, dense, L, out)
    n = len(X)
    if L == 8 and n in BLOCK_JACOBI:
        # the inner iterations the coarse space saves: the device's count is below half of block-Jacobi's
        assert 2 * out["stats"][3] < BLOCK_JACOBI[n], (out["stats"][3], BLOCK_JACOBI[n], its)


# ---- the full optimisation ------------------------------------------------------------------------------------------

def test_ring_of_64():
    truth, init, e, Z, Om = P.drift_ring()
    ref = Cr.optimize(init, e, Z, Om, L=8)
    out = optimizer(coarse_block=8).optimize(init, e, Z, Om)
    plain = optimizer().optimize(init, e, Z, Om)
    print("64-ring, L = 8:", {k: out[k] for k in ("cost0", "cost", "iterations", "accepted", "rejected", "pcg_iterations",
                                                   "coarse_aggregates", "coarse_failed")},
          "block-Jacobi:", {k: plain[k] for k in ("cost", "iterations", "pcg_iterations")},
          "restatement:", {k: ref[k] for k in ("cost", "iterations", "pcg_iterations")})
    assert out["converged"] and ref["converged"] and out["rejected"] == 0
    assert out["coarse_aggregates"] == 8 and out["coarse_failed"] == 0
    assert_poses(out["poses"], ref["poses"])
    assert_poses(out["poses"], plain["poses"])
    assert abs(out["cost"] - ref["cost"]) <= 1e-6 * ref["cost"]
    h = out["cost_history"]
    assert len(h) == out["iterations"] + 1 and h[0] == out["cost0"] and h[-1] == out["cost"]
    assert np.all(np.diff(h) <= 0)


def test_ring_of_1025_converges_where_block_jacobi_is_capped():
    truth, init, e, Z, Om = P.drift_ring(1025, 0)
    ref = Cr.optimize(init, e, Z, Om, L=16)
    out = optimizer(coarse_block=16).optimize(init, e, Z, Om)
    plain = optimizer().optimize(init, e, Z, Om)
    for name, o in (("L = 16", out), ("block-Jacobi", plain), ("restatement, L = 16", ref)):
        print("1025-ring,", name, {k: o[k] for k in ("converged", "cost", "iterations", "accepted", "pcg_iterations")},
              "trajectory error (m)", P.trajectory_error(o["poses"], truth))
    assert ref["converged"] and out["converged"] and out["coarse_failed"] == 0 and out["coarse_aggregates"] == 65
    assert abs(out["cost"] - ref["cost"]) <= 1e-6 * ref["cost"]
    assert not plain["converged"]


# ---- equivalence and determinism --------------------------------------------------------------------------------------

def test_coarse_block_zero_is_the_robust_entry_point():
    truth, init, e, Z, Om, closures = R.outlier_ring(0)
    scale = R.closure_scale(len(e), closures, 3.0)
    prm = dict(max_iteration=6, max_pcg_iterations=40)
    a = abi_optimize("nsc_posegraph_optimize_robust", init, e, Z, Om, scale, R.CAUCHY, **prm)
    b = abi_optimize("nsc_posegraph_optimize_coarse", init, e, Z, Om, scale, R.CAUCHY, coarse_block=0, **prm)
    assert a["stats"][1] >= 1 and a["stats"][3] >= 1 and (a["weights"] < 1.0).any()
    assert b["coarse_stats"].tolist() == [0.0, 0.0]
    same_bits(a, b, list(a))                                   # poses, stats, cost_history, step0, chi2, weights


@pytest.fixture(scope="module")
def ring64():
    return P.drift_ring()


def test_two_runs_agree_bitwise(ring64):
    _, init, e, Z, Om = ring64
    opt = optimizer(coarse_block=8)
    a = host(opt.optimize_device(init, e, Z, Om, step0=True))
    b = host(opt.optimize_device(init, e, Z, Om, step0=True))
    assert set(a) == {"poses", "stats", "cost_history", "step0", "coarse_stats"} and a["stats"][1] >= 1
    same_bits(a, b)


def test_alias_of_input_and_output(ring64):
    _, init, e, Z, Om = ring64
    opt = optimizer(coarse_block=8, max_iteration=5)
    separate = host(opt.optimize_device(init, e, Z, Om))
    X = torch.from_numpy(init).cuda()
    aliased = opt.optimize_device(X, e, Z, Om, poses_out=X)
    assert aliased["poses"].data_ptr() == X.data_ptr()
    same_bits(separate, host(aliased))
    assert separate["stats"][1] >= 1


def test_captured_replay_equals_eager(ring64):
    from _hipgraph import capture_replay
    _, init, e, Z, Om = ring64
    prm = dict(max_iteration=4, max_pcg_iterations=30)
    opt = optimizer(coarse_block=8, **prm)
    dev = [torch.from_numpy(a).cuda() for a in (init, e, Z, Om)]
    fixed = torch.zeros(len(init), dtype=torch.uint8, device="cuda")
    fixed[0] = 1

    def step():
        return opt.optimize_device(*dev, fixed=fixed, step0=True)
    eager, cap, types = capture_replay(step)
    assert set(eager) == {"poses", "stats", "cost_history", "step0", "coarse_stats"}
    for k in eager:
        assert torch.equal(eager[k], cap[k]), k
    assert eager["stats"][1].item() >= 1 and eager["coarse_stats"].tolist() == [8.0, 0.0]
    launches = 5 + 1 + 3 + prm["max_iteration"] * (14 + 5 * prm["max_pcg_iterations"]) + 1      # include/nsc.h
    kernels = types.pop("kernel", 0)
    assert types.get("memset", 0) == 0 and types.get("memcpy", 0) == 0, types
    assert kernels == launches, (kernels, launches)          # the Python layer adds none


# ---- fixed, skipped and degenerate inputs -----------------------------------------------------------------------------

def test_fixed_aggregate_fixed_poses_and_a_pose_without_edges(ring64):
    """aggregate 1 (poses 8..15) wholly fixed, poses 0, 17, 18 and 40 fixed, and a 65th pose that no edge touches: the
    ragged last aggregate has no free pose either.  They stay bitwise; the step is still the dense solve's."""
    from test_posegraph_gpu import perturbed
    _, init, e, Z, Om = ring64
    init = perturbed(init, np.random.default_rng(23), 0.01, 0.05)     # every edge has a residual: every free pose moves
    X = np.concatenate([init, init[5:6]])
    fixed = np.zeros(65, bool)
    fixed[[0, 17, 18, 40]] = True
    fixed[8:16] = True
    lin = Cr.linearize(X, e, Z, Om)
    free = Cr.free_nodes(65, e, fixed, lin["blocks"], LAMBDA)
    assert np.array_equal(free, ~fixed & (np.arange(65) < 64))
    dense = Cr.dense_step(lin["H"], lin["gradient"], LAMBDA, free)
    check_first_step("fixed", X, e, Z, Om, fixed, lin, free, dense, 8, first_step(X, e, Z, Om, fixed, 8))
    out = optimizer(coarse_block=8, max_iteration=6).optimize(X, e, Z, Om, fixed=fixed)
    assert out["accepted"] >= 1 and out["coarse_aggregates"] == 9 and out["coarse_failed"] == 0
    assert out["poses"][~free].tobytes() == X[~free].tobytes()
    moved = np.abs(out["poses"] - X).reshape(65, -1).max(1) > 0
    assert np.array_equal(moved, free)
    ref = Cr.optimize(X, e, Z, Om, L=8, fixed=fixed, max_iteration=6)
    assert_poses(out["poses"], ref["poses"])


def test_skipped_edges_are_counted_and_change_nothing_else():
    X, e, Z, Om = graph(70, 50, 21)
    n, m = len(X), len(e)
    rng = np.random.default_rng(3)
    bad = np.array([[3, 3], [-1, 2], [2, n], [n + 5, -7], [0, 2 ** 40], [69, 69], [-2 ** 40, 1]], np.int64)
    at = np.sort(rng.integers(0, m + 1, len(bad)))
    at[0], at[-1] = 0, m                                      # one in front of every edge, one behind, the rest among them
    e2 = np.insert(e, at, bad, axis=0)
    Z2 = np.insert(Z, at, np.tile(np.eye(4) * np.nan, (len(bad), 1, 1)), axis=0)
    Om2 = np.insert(Om, at, np.tile(np.eye(6) * np.nan, (len(bad), 1, 1)), axis=0)
    keep = P.valid_edges(n, e2)
    assert keep.sum() == m and np.array_equal(e2[keep], e)
    opt = optimizer(coarse_block=8, max_iteration=3)
    oa = host(opt.optimize_device(X, e, Z, Om, first_fixed(n), step0=True))
    ob = host(opt.optimize_device(X, e2, Z2, Om2, first_fixed(n), step0=True))
    assert ob["stats"][7] == len(bad) and oa["stats"][7] == 0 and oa["stats"][1] >= 1
    same_bits(oa, ob, ("poses", "cost_history", "step0", "coarse_stats"))
    assert np.array_equal(np.delete(oa["stats"], 7), np.delete(ob["stats"], 7))


SIZES = {"N=1": lambda: graph(1, 0, 4), "N=2": lambda: graph(2, 0, 5, reverse=True), "N=63": lambda: graph(63, 40, 6),
         "N=64": lambda: graph(64, 40, 7), "N=65": lambda: graph(65, 40, 8),
         "E=0": lambda: (graph(5, 0, 10)[0], np.zeros((0, 2), np.int64), np.zeros((0, 4, 4)), np.zeros((0, 6, 6)))}


@pytest.mark.parametrize("name", list(SIZES))
def test_sizes(name):
    X, e, Z, Om = SIZES[name]()
    n, L = len(X), 2 if len(X) <= 2 else 8
    fixed = first_fixed(n)
    out = optimizer(coarse_block=L, max_iteration=3).optimize(X, e, Z, Om)
    assert np.isfinite(out["poses"]).all() and np.isfinite(out["cost_history"]).all()
    assert out["cost"] <= out["cost0"] and out["skipped"] == 0
    assert out["coarse_aggregates"] == Cr.aggregates(n, L) and out["coarse_failed"] == 0
    if len(e) == 0 or n == 1:
        assert out["poses"].tobytes() == np.asarray(X).tobytes() and out["cost"] == 0.0 and out["pcg_iterations"] == 0
        return
    assert out["accepted"] >= 1
    lin = Cr.linearize(X, e, Z, Om)
    free = Cr.free_nodes(n, e, fixed, lin["blocks"], LAMBDA)
    dense = Cr.dense_step(lin["H"], lin["gradient"], LAMBDA, free)
    check_first_step(name, X, e, Z, Om, fixed, lin, free, dense, L, first_step(X, e, Z, Om, fixed, L))


# ---- a robust kernel --------------------------------------------------------------------------------------------------

def test_outlier_ring_with_cauchy():
    truth, init, e, Z, Om, closures = R.outlier_ring(0)
    scale = R.closure_scale(len(e), closures, 3.0)
    ref = Cr.optimize(init, e, Z, Om, L=8, kernel=R.CAUCHY, scale=scale)
    out = optimizer(kernel="cauchy", coarse_block=8).optimize(init, e, Z, Om, robust_scale=scale)
    plain = optimizer(kernel="cauchy").optimize(init, e, Z, Om, robust_scale=scale)
    print("outlier ring, Cauchy c = 3, L = 8:",
          {k: out[k] for k in ("cost0", "cost", "iterations", "accepted", "rejected", "pcg_iterations")},
          "block-Jacobi:", {k: plain[k] for k in ("cost", "iterations", "pcg_iterations")},
          "weights on the closures", out["weights"][-closures:], "without the coarse space", plain["weights"][-closures:])
    assert ref["converged"] and out["converged"] and out["coarse_failed"] == 0
    w, wp = out["weights"], plain["weights"]
    assert (w[:len(e) - closures] == 1.0).all()                           # odometry stays quadratic
    assert (w[-closures:-2] > 0.9).all() and (w[-2:] < 0.01).all()        # the ring's and the true closures; the false ones
    assert np.array_equal(w > 0.5, wp > 0.5)                              # the same sides as without the coarse space
    assert_poses(out["poses"], ref["poses"])
    assert abs(out["cost"] - ref["cost"]) <= 1e-6 * ref["cost"]
