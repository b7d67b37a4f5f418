"""Pose-graph optimisation on the MI355X: nsc_posegraph_linearize and nsc_posegraph_optimize against the float64
restatement (tests/posegraph_restatement.py) -- the system, the first step, the full optimisation, every stopping and
rejection path, determinism, capture, aliasing, and the loop from TwoStageRetrieval.query to corrected poses."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import posegraph_restatement as P
from _posegraph import host, optimizer

pytestmark = pytest.mark.gpu

ANGLES = (0.0, 1e-9, 1e-3, np.pi / 2, np.deg2rad(170.0))


def _pg():
    from neural_spectral_codec_amd.retrieval import pose_graph as pg
    return pg


def close(got, want, what):
    """the project's bar for float64 sums against a float64 restatement: 1e-6 of the array's largest magnitude"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.size:
        scale = np.abs(want).max()
        assert np.abs(got - want).max() <= 1e-6 * scale, (what, np.abs(got - want).max(), scale)


# ---- graphs -----------------------------------------------------------------------------------------------------

def perturbed(truth, rng, rot=0.05, trans=0.2):
    return np.stack([x @ P.make_pose(rot * rng.standard_normal(3), trans * rng.standard_normal(3)) for x in truth])


def graph(n, extra, seed, reverse=False, duplicate=False):
    """n poses, a chain plus `extra` random edges; measurements with noise, random information"""
    rng = np.random.default_rng(seed)
    truth = np.stack([P.make_pose(0.4 * rng.standard_normal(3), 6.0 * rng.standard_normal(3)) for _ in range(n)])
    e = P.chain_edges(n)
    if extra and n > 2:
        a = rng.integers(0, n, (extra, 2))
        e = np.concatenate([e, a[a[:, 0] != a[:, 1]]])
    if reverse:
        e = np.where((np.arange(len(e)) % 2 == 0)[:, None], e[:, ::-1], e)
    if duplicate:
        e = np.concatenate([e, e[::2], e[:1]])
    e = e.astype(np.int64).reshape(-1, 2)
    Z = P.noisy(P.relative(truth, e), rng, 0.01, 0.05) if len(e) else np.zeros((0, 4, 4))
    return perturbed(truth, rng), e, Z, P.random_information(rng, len(e))


def chain5():
    rng = np.random.default_rng(7)
    truth = P.ring_poses(5, 4.0)
    e = np.concatenate([P.chain_edges(5), [[4, 0]]]).astype(np.int64)
    Z = P.noisy(P.relative(truth, e), rng)
    init = perturbed(truth, rng)
    init[0] = truth[0]
    return init, e, Z, P.random_information(rng, len(e))


def angle_graph():
    """ten poses, one edge per residual angle of ANGLES"""
    rng = np.random.default_rng(13)
    X, e, Z = [], [], []
    for k, a in enumerate(ANGLES):
        Xi = P.make_pose(rng.standard_normal(3), 5.0 * rng.standard_normal(3))
        A = P.make_pose(0.5 * rng.standard_normal(3), 3.0 * rng.standard_normal(3))
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        X += [Xi, Xi @ A]
        e.append((2 * k, 2 * k + 1))
        Z.append(A @ P.inv_se3(P.make_pose(axis * a, rng.standard_normal(3))))
    return np.stack(X), np.asarray(e, np.int64), np.stack(Z), P.random_information(rng, len(e))


def star(hub_edges=300):
    rng = np.random.default_rng(17)
    n = hub_edges + 1
    truth = np.stack([P.make_pose(0.4 * rng.standard_normal(3), 6.0 * rng.standard_normal(3)) for _ in range(n)])
    k = np.arange(1, n)
    e = np.where((k % 2 == 0)[:, None], np.stack([np.zeros_like(k), k], 1), np.stack([k, np.zeros_like(k)], 1))
    e = e.astype(np.int64)
    return perturbed(truth, rng), e, P.noisy(P.relative(truth, e), rng, 0.01, 0.05), P.random_information(rng, len(e))


LINEARIZE_CASES = {
    "two poses, one edge": lambda: graph(2, 0, 1),
    "5-chain with a loop": chain5,
    "edges with i > j": lambda: graph(9, 6, 2, reverse=True),
    "duplicate edges": lambda: graph(7, 4, 3, duplicate=True),
    "residual angles": angle_graph,
    "hub of 300": star,
    "N=1": lambda: graph(1, 0, 4),
    "N=2": lambda: graph(2, 0, 5, reverse=True),
    "N=63": lambda: graph(63, 40, 6),
    "N=64": lambda: graph(64, 40, 7),
    "N=65": lambda: graph(65, 40, 8),
    "N=257": lambda: graph(257, 200, 9, reverse=True),
    "E=0": lambda: (graph(5, 0, 10)[0], np.zeros((0, 2), np.int64), np.zeros((0, 4, 4)), np.zeros((0, 6, 6))),
}


@pytest.mark.parametrize("name", list(LINEARIZE_CASES))
def test_linearize_matches_restatement(name):
    X, e, Z, Om = LINEARIZE_CASES[name]()
    got = host(optimizer().linearize(X, e, Z, Om))
    ref = P.linearize(X, e, Z, Om)
    assert got["skipped"][0] == ref["skipped"] == 0
    for k in ("residuals", "gradient", "blocks"):
        close(got[k], ref[k], (name, k))
    assert abs(got["cost"][0] - ref["cost"]) <= 1e-6 * max(ref["cost"], 1e-300), (name, got["cost"], ref["cost"])
    if name == "residual angles":
        assert np.abs(np.linalg.norm(got["residuals"][:, :3], axis=1) - np.array(ANGLES)).max() <= 1e-9


def test_linearize_reads_the_upper_triangle_only():
    X, e, Z, Om = chain5()
    junk = Om + np.tril(np.full((6, 6), 1e9), -1)
    a, b = host(optimizer().linearize(X, e, Z, Om)), host(optimizer().linearize(X, e, Z, junk))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


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
    a, b = host(optimizer().linearize(X, e, Z, Om)), host(optimizer().linearize(X, e2, Z2, Om2))
    assert a["skipped"][0] == 0 and b["skipped"][0] == len(bad)
    assert not b["residuals"][~keep].any()
    assert b["residuals"][keep].tobytes() == a["residuals"].tobytes()
    for k in ("cost", "gradient", "blocks"):
        assert a[k].tobytes() == b[k].tobytes(), k
    fixed = np.zeros(n, bool)
    fixed[0] = True
    oa = host(optimizer(max_iteration=3).optimize_device(X, e, Z, Om, fixed))
    ob = host(optimizer(max_iteration=3).optimize_device(X, e2, Z2, Om2, fixed))
    assert ob["stats"][7] == len(bad) and oa["stats"][7] == 0
    assert oa["poses"].tobytes() == ob["poses"].tobytes() and oa["cost_history"].tobytes() == ob["cost_history"].tobytes()


# ---- the first step -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ring64():
    return P.drift_ring()


@pytest.mark.parametrize("name", ["5-chain", "64-ring"])
def test_first_step_matches_dense_solve(name, ring64):
    if name == "5-chain":
        X, e, Z, Om = chain5()
    else:
        _, X, e, Z, Om = ring64
    lam = P.DEFAULTS["lambda0"]
    lin = P.linearize(X, e, Z, Om, dense=True)
    fixed = np.zeros(len(X), bool)
    fixed[0] = True
    free = P.free_nodes(len(X), e, fixed)
    dense = P.dense_step(lin["H"], lin["gradient"], lam, free)
    pcg, its = P.pcg_step(lin["H"], lin["gradient"], lam, free, 1000, 1e-12)
    bar = 10.0 * np.abs(pcg - dense).max()          # the restatement's own PCG against its dense solve, times ten
    out = host(optimizer(max_iteration=1, max_pcg_iterations=1000, pcg_tolerance=1e-12).optimize_device(
        X, e, Z, Om, fixed, step0=True))
    err = np.abs(out["step0"] - dense).max()
    print(name, "restatement PCG iterations", its, "device", out["stats"][3], "bar", bar, "device error", err,
          "largest step entry", np.abs(dense).max())
    assert err <= bar
    assert not out["step0"][0].any()                          # the fixed pose


# ---- the full optimisation ----------------------------------------------------------------------------------------

def assert_poses(got, want):
    """the project's bars for converged registrations: 1e-3 on translations, 1e-4 on rotation entries"""
    assert np.abs(got[:, :3, 3] - want[:, :3, 3]).max() <= 1e-3
    assert np.abs(got[:, :3, :3] - want[:, :3, :3]).max() <= 1e-4
    assert np.array_equal(got[:, 3], want[:, 3])


def test_ring_with_drift_and_one_closure(ring64):
    truth, init, e, Z, Om = ring64
    ref = P.optimize(init, e, Z, Om)
    out = optimizer().optimize(init, e, Z, Om)
    print("64-ring:", {k: out[k] for k in ("cost0", "cost", "iterations", "accepted", "rejected", "pcg_iterations")},
          "restatement:", {k: ref[k] for k in ("cost", "iterations", "pcg_iterations")})
    assert_poses(out["poses"], ref["poses"])
    assert out["converged"] and ref["converged"] and out["rejected"] == 0
    assert abs(out["cost0"] - ref["cost0"]) <= 1e-6 * ref["cost0"] and abs(out["cost"] - ref["cost"]) <= 1e-6 * ref["cost"]
    h = out["cost_history"]
    assert len(h) == out["iterations"] + 1 and h[0] == out["cost0"] and h[-1] == out["cost"]
    assert np.all(np.diff(h) <= 0) and out["accepted"] == np.count_nonzero(np.diff(h) < 0)
    before, after = P.trajectory_error(init, truth), P.trajectory_error(out["poses"], truth)
    print("trajectory error (m): before", before, "after", after)
    assert after < before


def test_rejected_steps():
    truth, init, e, Z, Om = P.far_start()
    kw = dict(lambda0=1e-12, max_iteration=60)
    ref = P.optimize(init, e, Z, Om, **kw)
    out = optimizer(**kw).optimize(init, e, Z, Om)
    print("rejected-step case:", {k: out[k] for k in ("cost0", "cost", "iterations", "accepted", "rejected")})
    assert out["rejected"] >= 1 and out["converged"] and ref["rejected"] >= 1
    assert_poses(out["poses"], ref["poses"])
    h = out["cost_history"]
    assert np.all(np.diff(h) <= 0) and np.count_nonzero(np.diff(h) == 0) == out["rejected"]


def test_capped_inner_iterations(ring64):
    _, init, e, Z, Om = ring64
    kw = dict(max_pcg_iterations=2, max_iteration=8)
    ref = P.optimize(init, e, Z, Om, **kw)
    out = optimizer(**kw).optimize(init, e, Z, Om)
    assert out["pcg_iterations"] == ref["pcg_iterations"] == 16 and out["iterations"] == 8 and not out["converged"]
    assert_poses(out["poses"], ref["poses"])
    assert np.abs(out["cost_history"] - ref["cost_history"]).max() <= 1e-6 * ref["cost0"]


def test_no_outer_iteration(ring64):
    _, init, e, Z, Om = ring64
    out = host(optimizer(max_iteration=0).optimize_device(init, e, Z, Om))
    assert out["poses"].tobytes() == init.tobytes()
    s = out["stats"]
    assert s[0] == s[1] == s[2] == s[3] == 0 and s[4] == s[5] == out["cost_history"][0] and s[8] == 0
    assert abs(s[4] - P.cost(init, e, Z, Om)) <= 1e-6 * s[4] and len(out["cost_history"]) == 1


# ---- invariants -----------------------------------------------------------------------------------------------------

def test_fixed_poses_stay_bitwise(ring64):
    _, init, e, Z, Om = ring64
    init = perturbed(init, np.random.default_rng(23), 0.01, 0.05)     # every edge has a residual: every free pose moves
    fixed = np.zeros(len(init), bool)
    fixed[[0, 17, 18, 40, 63]] = True
    out = optimizer(max_iteration=6).optimize(init, e, Z, Om, fixed=fixed)
    assert out["accepted"] >= 1
    assert out["poses"][fixed].tobytes() == init[fixed].tobytes()
    moved = np.abs(out["poses"] - init).reshape(len(init), -1).max(1) > 0
    assert np.array_equal(moved, ~fixed)
    ref = P.optimize(init, e, Z, Om, fixed=fixed, max_iteration=6)
    assert_poses(out["poses"], ref["poses"])
    # a pose no edge touches is not moved either, and nothing else notices it
    lonely = np.concatenate([init, init[5:6]])
    alone = optimizer(max_iteration=6).optimize(lonely, e, Z, Om, fixed=np.append(fixed, False))
    assert alone["poses"][-1].tobytes() == init[5].tobytes() and alone["poses"][:-1].tobytes() == out["poses"].tobytes()


def test_two_runs_agree_bitwise(ring64):
    _, init, e, Z, Om = ring64
    a = host(optimizer().optimize_device(init, e, Z, Om, step0=True))
    b = host(optimizer().optimize_device(init, e, Z, Om, step0=True))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    X, e, Z, Om = star()
    a, b = host(optimizer().linearize(X, e, Z, Om)), host(optimizer().linearize(X, e, Z, Om))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_alias_of_input_and_output(ring64):
    _, init, e, Z, Om = ring64
    opt = optimizer(max_iteration=5)
    separate = host(opt.optimize_device(init, e, Z, Om))
    X = torch.from_numpy(init).cuda()
    aliased = opt.optimize_device(X, e, Z, Om, poses_out=X)
    assert aliased["poses"].data_ptr() == X.data_ptr()
    aliased = host(aliased)
    for k in separate:
        assert separate[k].tobytes() == aliased[k].tobytes(), k
    assert separate["stats"][1] >= 1


def test_captured_replay_equals_eager(ring64):
    from _hipgraph import capture_replay
    _, init, e, Z, Om = ring64
    prm = dict(max_iteration=4, max_pcg_iterations=30)
    opt = optimizer(**prm)
    dev = [torch.from_numpy(a).cuda() for a in (init, e, Z, Om)]
    fixed = torch.zeros(len(init), dtype=torch.uint8, device="cuda")
    fixed[0] = 1

    def step():
        return opt.optimize_device(*dev, fixed=fixed, step0=True)
    eager, cap, types = capture_replay(step)
    for k in eager:
        assert torch.equal(eager[k], cap[k]), k
    assert eager["stats"][1].item() >= 1
    launches = 5 + 1 + 3 + prm["max_iteration"] * (8 + 4 * prm["max_pcg_iterations"]) + 1     # include/nsc.h
    kernels = types.pop("kernel", 0)
    assert types.get("memset", 0) == 0 and types.get("memcpy", 0) == 0, types
    assert kernels == launches, (kernels, launches)          # the Python layer adds none


# ---- from the retrieval to corrected poses --------------------------------------------------------------------------

def test_query_to_corrected_poses():
    """A short trajectory through world 3 that ends where it can see its first three keyframes again: stage 1 and stage 2
    (prepared stores, planar guess) verify the revisits, closure_edges + odometry_edges build the graph from the drifted
    odometry, and the optimiser pulls the end point back: its error falls below the drift that was injected."""
    from neural_spectral_codec_amd import synth
    from neural_spectral_codec_amd.retrieval import GeometricVerifier, create_two_stage_retrieval
    pg = _pg()
    world = synth.make_world(3)
    truth = np.stack([synth.pose_xyz_yaw(4.0, -3.0, 0.0, 17.5), synth.pose_xyz_yaw(10.0, -2.0, 0.0, 30.0),
                      synth.pose_xyz_yaw(8.0, 8.0, 0.0, -93.2), synth.pose_xyz_yaw(0.0, 0.0)])
    scans = [synth.scan_world(world, X, seed=2 + k) for k, X in enumerate(truth[:3])] + [
        synth.scan_world(world, truth[3], seed=1)]
    rng = np.random.default_rng(0)
    desc = rng.random((4, 800)).astype(np.float32)
    desc /= desc.sum(1, keepdims=True)
    kfs = [SimpleNamespace(keyframe_id=100 + k, scan_id=k, points=scans[k], descriptor=desc[k], pose=None)
           for k in range(3)]
    r = create_two_stage_retrieval(top_k=3, verifier=GeometricVerifier(), prepare_geometry=True, planar_init=True)
    r.add_keyframes(kfs)
    query = SimpleNamespace(keyframe_id=7, scan_id=3, points=scans[3], descriptor=desc[3], pose=None)
    candidates = r.query(query)
    ce, cZ, cOm = pg.closure_edges(3, candidates)
    assert len(ce) >= 1 and set(ce[:, 1]) == {3} and set(ce[:, 0]) <= {0, 1, 2}
    for (i, j), z in zip(ce, cZ):
        assert np.abs(z[:3, 3] - (P.inv_se3(truth[i]) @ truth[j])[:3, 3]).max() <= 0.1

    drift = P.make_pose(np.array([0.0, 0.0, 0.03]), np.array([0.4, -0.3, 0.05]))
    _, oZ, _ = pg.odometry_edges(truth)
    odometry = P.integrate(np.stack([z @ drift for z in oZ]), truth[0])
    oe, oZ, oOm = pg.odometry_edges(odometry, information=np.diag([400.0, 400.0, 400.0, 25.0, 25.0, 25.0]))
    injected = np.linalg.norm(odometry[3, :3, 3] - truth[3, :3, 3])
    out = pg.PoseGraphOptimizer().optimize(odometry, np.concatenate([oe, ce]), np.concatenate([oZ, cZ]),
                                           np.concatenate([oOm, cOm]))
    closed = np.linalg.norm(out["poses"][3, :3, 3] - truth[3, :3, 3])
    print("end-point error (m): injected", injected, "after closing", closed, "closures", ce.tolist(),
          {k: out[k] for k in ("cost0", "cost", "iterations", "accepted", "rejected")})
    assert injected > 0.5 and closed < injected and out["accepted"] >= 1
