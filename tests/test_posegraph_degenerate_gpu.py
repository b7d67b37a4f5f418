"""The pose-graph kernels on systems that are not well posed (tests/posegraph_degenerate_cases.py): damped blocks that are
not positive definite, a coarse factor that fails, the PCG exit on p.Ap <= 0, information that is rank-deficient or not
finite.  On the decidable cases every decision of the restatement has a relative margin of 1e-6 or more
(test_posegraph_degenerate_cpu.py), so the device has to take the same branches: counts are compared exactly, vectors at
the project's bar (close() of test_posegraph_gpu.py).  On the undecidable cases pivots sit at rounding level and only
properties are asserted."""
import numpy as np
import pytest
import torch

import posegraph_coarse_restatement as Cr
import posegraph_cov_restatement as V
import posegraph_degenerate_cases as D
import posegraph_restatement as P
import posegraph_robust_restatement as R
from _posegraph import abi_optimize, host, optimizer, plain_linearize, plain_optimize, same_bits
from test_posegraph_gpu import close

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678                         # what every output holds before a call
IDS = [f"{name}-L{L}" for name, L in D.instances()]
ITERATIONS, ACCEPTED, REJECTED, PCG_ITERATIONS, INITIAL_COST, FINAL_COST, LAMBDA, SKIPPED, CONVERGED, STEP = range(10)

_REF = {}


def reference(name, L, **override):
    """the traced restatement (bitwise posegraph_coarse_restatement.optimize: test_posegraph_degenerate_cpu.py), once"""
    key = (name, L, tuple(sorted(override.items())))
    if key not in _REF:
        _REF[key] = D.run(name, L, **override)
    return _REF[key]


def device(name, L, ws=None, graph=None, **override):
    """a decidable case through the entry point that fits it: nsc_posegraph_optimize (no coarse space, no kernel),
    nsc_posegraph_optimize_robust (a kernel) or nsc_posegraph_optimize_coarse"""
    X, e, Z, Om, fixed, extras = graph or D.decidable(name)
    prm = dict(extras["params"], **override)
    kernel, scale = extras.get("kernel"), extras.get("scale")
    common = dict(fixed=fixed, ws=ws, fill=SENTINEL, **prm)
    if L is None and kernel is None:
        return plain_optimize(X, e, Z, Om, **common)
    scale = np.zeros(len(e)) if scale is None else scale
    if L is None:
        return abi_optimize("nsc_posegraph_optimize_robust", X, e, Z, Om, scale, kernel, **common)
    return abi_optimize("nsc_posegraph_optimize_coarse", X, e, Z, Om, scale, R.NONE if kernel is None else kernel,
                        coarse_block=L, **common)


def written(out, keys=("poses", "stats", "cost_history", "coarse_stats")):
    for k in keys:
        if k in out:
            assert not (out[k] == SENTINEL).any(), k


# ---- decidable cases: the first step ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,L", D.instances(), ids=IDS)
def test_first_step(name, L):
    ref = reference(name, L, max_iteration=1)
    out = device(name, L, max_iteration=1)
    free = ref["trace"]["free"][0]
    err = np.abs(out["step0"] - ref["step0"]).max() / np.abs(ref["step0"]).max()
    print(f"{name}, L = {L}: free {int(free.sum())} of {len(free)}, inner iterations {ref['inner']}, device "
          f"{out['stats'][PCG_ITERATIONS]}, coarse stats {out.get('coarse_stats')}, step0 error / largest entry {err:.3g}")
    written(out, ("poses", "stats", "cost_history", "coarse_stats", "step0"))
    assert out["stats"][PCG_ITERATIONS] == ref["pcg_iterations"]
    assert not out["step0"][~free].any()                      # exactly zero where the pose is not free
    close(out["step0"], ref["step0"], (name, L, "step0"))
    if L is not None:
        assert out["coarse_stats"].tolist() == [Cr.aggregates(len(free), L), ref["coarse_failed"]]


def test_first_step_sees_a_failed_factor_and_blocks_that_are_not_positive_definite():
    """what the table above relies on, spelt out on one case: the counts are not those of a healthy graph"""
    ref = reference("chords-9", 2, max_iteration=1)
    out = device("chords-9", 2, max_iteration=1)
    X, e, Z, Om, fixed, extras = D.decidable("chords-9")
    free = ref["trace"]["free"][0]
    not_free_by_block = ~free & ~fixed
    assert not_free_by_block.sum() == 3 and np.array_equal(np.nonzero(not_free_by_block)[0], extras["not_free"])
    assert out["coarse_stats"][1] == 1 and out["coarse_stats"][1] > 0
    assert out["stats"][PCG_ITERATIONS] == 3                  # two steps and the iteration that meets p.Ap <= 0
    assert out["step0"][free].any(1).all() and not out["step0"][not_free_by_block].any()


# ---- decidable cases: the full run --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,L", D.instances(), ids=IDS)
def test_full_run(name, L):
    X = D.decidable(name)[0]
    ref = reference(name, L)
    out = device(name, L)
    s = out["stats"]
    got = dict(accepted=s[ACCEPTED], rejected=s[REJECTED], pcg_iterations=s[PCG_ITERATIONS], converged=s[CONVERGED],
               coarse_failed=out["coarse_stats"][1] if L is not None else 0)
    ever_free = np.any(ref["trace"]["free"], axis=0)
    print(f"{name}, L = {L}: device {got}, restatement inner {ref['inner']} failed {ref['trace']['failed']}, cost "
          f"{ref['cost0']:.6g} -> {ref['cost']:.6g}, poses error "
          f"{np.abs(out['poses'] - ref['poses']).max() / np.abs(ref['poses']).max():.3g}, cost history error "
          f"{np.abs(out['cost_history'] - ref['cost_history']).max() / np.abs(ref['cost_history']).max():.3g}")
    written(out)
    for k, v in got.items():
        assert v == ref[k], (k, v, ref[k])
    assert s[ITERATIONS] == ref["iterations"] == s[ACCEPTED] + s[REJECTED]
    close(out["cost_history"], ref["cost_history"], (name, L, "cost_history"))
    close(out["poses"], ref["poses"], (name, L, "poses"))
    assert out["poses"][~ever_free].tobytes() == X[~ever_free].tobytes()
    if L is not None and ref["coarse_failed"]:
        assert out["coarse_stats"][1] > 0


def test_entry_points_agree_bitwise_on_degenerate_input():
    """coarse_block = 0 is the robust call and kernel NONE is the plain call, also where blocks fail and PCG breaks down"""
    X, e, Z, Om, fixed, extras = D.decidable("robust-indefinite")
    prm = dict(extras["params"], fixed=fixed)
    a = abi_optimize("nsc_posegraph_optimize_robust", X, e, Z, Om, extras["scale"], extras["kernel"], **prm)
    b = abi_optimize("nsc_posegraph_optimize_coarse", X, e, Z, Om, extras["scale"], extras["kernel"], coarse_block=0,
                     **prm)
    assert a["stats"][ACCEPTED] >= 1 and a["stats"][REJECTED] >= 1 and (a["weights"] < 1.0).any()
    assert b["coarse_stats"].tolist() == [0.0, 0.0]
    same_bits(a, b, list(a))
    X, e, Z, Om, fixed, extras = D.decidable("chords-9")
    prm = dict(extras["params"], fixed=fixed)
    plain = plain_optimize(X, e, Z, Om, **prm)
    none = abi_optimize("nsc_posegraph_optimize_robust", X, e, Z, Om, np.full(len(e), 3.0), R.NONE, **prm)
    zero = abi_optimize("nsc_posegraph_optimize_coarse", X, e, Z, Om, np.full(len(e), 3.0), R.NONE, coarse_block=0, **prm)
    assert plain["stats"][REJECTED] >= 1 and plain["stats"][PCG_ITERATIONS] == reference("chords-9", None)["pcg_iterations"]
    same_bits(plain, none, list(plain))
    same_bits(plain, zero, list(plain))


# ---- determinism, capture, workspace reuse ------------------------------------------------------------------------------

def test_lambda_walk_is_deterministic_and_can_be_captured():
    from _hipgraph import capture_replay
    X, e, Z, Om, fixed, extras = D.decidable("lambda-walk-up")
    ref = reference("lambda-walk-up", 2)
    opt = optimizer(coarse_block=2, **extras["params"])
    dev = [torch.from_numpy(a).cuda() for a in (X, e, Z, Om)]
    fx = torch.from_numpy(fixed.astype(np.uint8)).cuda()

    def step():
        return opt.optimize_device(*dev, fixed=fx, step0=True)
    a, b = host(step()), host(step())
    same_bits(a, b)
    assert a["coarse_stats"].tolist() == [5.0, float(ref["coarse_failed"])] and 0 < a["coarse_stats"][1] < a["stats"][0]
    eager, cap, types = capture_replay(step)
    assert set(eager) == {"poses", "stats", "cost_history", "step0", "coarse_stats"}
    for k in eager:
        assert torch.equal(eager[k], cap[k]), k
        assert eager[k].cpu().numpy().tobytes() == a[k].tobytes(), k
    assert types.get("memset", 0) == 0 and types.get("memcpy", 0) == 0, types


@pytest.mark.parametrize("order", ["degenerate first", "healthy first"])
def test_no_failure_state_survives_in_the_workspace(order):
    """chords (the factor fails on every step) and a healthy ring share one workspace buffer: the second call's outputs
    are those of a call on a fresh buffer, whichever comes second"""
    from neural_spectral_codec_amd import _lib
    _, init, e, Z, Om = P.drift_ring(17)
    healthy = (init, e, Z, Om, D.first_fixed(17), dict(params=dict(max_iteration=4, max_pcg_iterations=60)))
    sick = D.decidable("chords-17")
    lib = _lib.lib()
    need = max(int(lib.nsc_posegraph_coarse_workspace_bytes(len(g[0]), len(g[1]), 2)) for g in (healthy, sick))
    pair = [("chords-17", sick), ("ring", healthy)]
    first, second = pair if order == "degenerate first" else pair[::-1]
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    one = device(first[0], 2, ws=ws, graph=first[1])
    two = device(second[0], 2, ws=ws, graph=second[1])
    fresh = device(second[0], 2, ws=torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda"), graph=second[1])
    same_bits(two, fresh)
    sick_out, healthy_out = (one, two) if order == "degenerate first" else (two, one)
    assert sick_out["coarse_stats"][1] == sick_out["stats"][ITERATIONS] > 0      # every step of chords-17, L = 2 fails
    assert healthy_out["coarse_stats"].tolist() == [9.0, 0.0] and healthy_out["stats"][ACCEPTED] >= 1


# ---- the covariance call ------------------------------------------------------------------------------------------------

CAP = 100


def covariance(X, e, Z, Om, nodes, fixed, L=None):
    return optimizer(coarse_block=L, max_pcg_iterations=CAP, pcg_tolerance=V.TAU).covariance(X, e, Z, Om, nodes, fixed)


@pytest.fixture(scope="module")
def chords9_columns():
    X, e, Z, Om, fixed, _ = D.decidable("chords-9")
    nodes = list(range(1, 9))
    joint, its, free, trace = D.traced_columns(X, e, Z, Om, fixed, nodes, None, CAP, V.TAU)
    return X, e, Z, Om, fixed, nodes, joint, its, free, trace["converged"]


def test_covariance_counts_blocks_that_fail(chords9_columns):
    X, e, Z, Om, fixed, nodes, joint, its, free, conv = chords9_columns
    out = covariance(X, e, Z, Om, nodes, fixed)
    sel = free[nodes]
    print("chords-9 covariance: iterations", out["iterations"].tolist(), "not free", out["not_free"], "not converged",
          out["not_converged"])
    assert not fixed[nodes].any() and out["not_free"] == (~sel).sum() == 3 and out["not_free"] > 0
    for q in np.nonzero(~sel)[0]:
        assert not out["joint"][q].any() and not out["joint"][:, q].any() and not out["iterations"][q].any()
    # poses 2 and 4 lie between poses that are not free: their columns are solved by B^-1 in one iteration; the columns of
    # poses 6, 7 and 8 end on p.Ap <= 0 and are counted
    assert np.array_equal(out["iterations"], its) and np.array_equal(out["converged"], conv)
    assert out["not_converged"] == (~conv).sum() == 18 and out["not_converged"] > 0
    close(out["joint"], joint, "joint at the breakdown")


@pytest.mark.parametrize("L", [2, 4])
def test_covariance_with_a_failed_coarse_factor_is_block_jacobi(chords9_columns, L):
    X, e, Z, Om, fixed, nodes, joint, its, free, conv = chords9_columns
    assert D.traced_columns(X, e, Z, Om, fixed, nodes, L, CAP, V.TAU)[3]["failed"]
    out = covariance(X, e, Z, Om, nodes, fixed, L)
    plain = covariance(X, e, Z, Om, nodes, fixed)
    assert (out["coarse_aggregates"], out["coarse_failed"]) == (Cr.aggregates(9, L), 1)
    assert np.array_equal(out["iterations"], plain["iterations"]) and np.array_equal(out["iterations"], its)
    assert (out["not_free"], out["not_converged"]) == (plain["not_free"], plain["not_converged"])
    close(out["joint"], plain["joint"], "joint, B^-1 alone")


def test_covariance_of_the_healthy_component_beside_a_degenerate_one():
    X, e, Z, Om, fixed, extras = D.cov_two_components()
    healthy, sick = extras["healthy"], extras["degenerate"]
    _, its, free, trace = D.traced_columns(X, e, Z, Om, fixed, healthy + sick, None, CAP, V.TAU)
    both = covariance(X, e, Z, Om, healthy + sick, fixed)
    alone = covariance(X, e, Z, Om, healthy, fixed)
    h = len(healthy)
    assert np.ascontiguousarray(both["joint"][:h, :h]).tobytes() == alone["joint"].tobytes()
    assert both["iterations"][:h].tobytes() == alone["iterations"].tobytes()
    assert np.array_equal(both["iterations"], its)
    assert both["converged"][:h].all() and np.array_equal(both["converged"], trace["converged"])
    assert both["not_free"] == 1 and both["not_converged"] == 12 and alone["not_converged"] == 0      # poses 12 and 20
    lin, _ = V.system(X, e, Z, Om, fixed)
    Sigma = V.dense_sigma(lin["H"], free & (np.arange(len(X)) < 12))              # H is block diagonal over the components
    err = np.abs(alone["joint"] - V.joint_of(Sigma, healthy)).max() / (V.TAU * np.linalg.norm(Sigma, 2))
    print("healthy columns beside the degenerate component: error / (tau |Sigma|_2)", err)
    assert err <= V.BAR
    assert not both["joint"][:h, h:].any() and not both["joint"][h:, :h].any()   # the components do not meet
    coarse = covariance(X, e, Z, Om, healthy + sick, fixed, 4)
    assert (coarse["coarse_aggregates"], coarse["coarse_failed"]) == (6, 1)
    assert np.array_equal(coarse["iterations"], both["iterations"])


def test_covariance_counts_a_block_that_is_not_finite():
    """+inf on the diagonal of one information matrix: both poses of that edge have a block that is not finite, which is
    not positive definite: they are not free, and the columns of the others are those of the graph without them"""
    X, e, Z, Om, fixed, extras = D.non_finite("inf-in-Om", apart=True)
    out = covariance(X, e, Z, Om, [7, 8, 2], fixed)
    assert (out["not_free"], out["skipped"], out["outside"]) == (2, 0, 0)
    assert not out["joint"][:2].any() and not out["joint"][:, :2].any() and not out["iterations"][:2].any()
    cX, ce, cZ, cOm = extras["clean"]
    clean = covariance(cX, ce, cZ, cOm, [2], fixed)
    assert out["converged"][2].all() and out["joint"][2, 2].tobytes() == clean["joint"][0, 0].tobytes()


def test_covariance_counts_a_block_whose_pivot_overflows():
    """two edges of information 1e308 I have pose 1 as their second end (J_j = B, no lever arm): its block sums to +inf on
    the diagonal with finite entries beside it, so every pivot is positive and none is finite.  The pose is not free."""
    rng = np.random.default_rng(5)
    X = P.integrate([P.make_pose(0.1 * rng.standard_normal(3), rng.standard_normal(3)) for _ in range(2)])
    e = np.array([[0, 1], [2, 1]], np.int64)
    Z = P.noisy(P.relative(X, e), rng)
    Om = np.tile(1e308 * np.eye(6), (2, 1, 1))
    with np.errstate(all="ignore"):
        block = Cr.linearize(X, e, Z, Om)["blocks"][1]
    assert (np.diag(block) == np.inf).all() and np.isfinite(block[~np.eye(6, dtype=bool)]).all()
    out = covariance(X, e, Z, Om, [1], D.first_fixed(3))
    print("overflowing block: not free", out["not_free"], "iterations", out["iterations"].tolist())
    assert out["not_free"] == 1 and out["not_free"] > 0
    assert not out["joint"].any() and not out["iterations"].any() and not out["residual"].any()


# ---- undecidable cases: properties ----------------------------------------------------------------------------------------

def check_properties(what, out, X, fixed, max_iteration):
    written(out)
    s, h = out["stats"], out["cost_history"]
    print(what, "stats", s.tolist(), "coarse", out.get("coarse_stats"), "history", h.tolist())
    finite = np.isfinite(X)
    assert np.isfinite(out["poses"][finite]).all()
    assert out["poses"][fixed].tobytes() == X[fixed].tobytes()
    assert s[ACCEPTED] + s[REJECTED] == s[ITERATIONS] <= max_iteration
    if np.isfinite(s[INITIAL_COST]):
        assert np.isfinite(h).all() and np.all(np.diff(h) <= 0) and s[FINAL_COST] <= s[INITIAL_COST]
        assert h[0] == s[INITIAL_COST] and h[-1] == s[FINAL_COST]
    else:
        assert out["poses"].tobytes() == X.tobytes() and s[ACCEPTED] == 0


@pytest.mark.parametrize("L", [None, 2, 4])
def test_planar_information(L):
    X, e, Z, Om, fixed, extras = D.planar_information()
    out = device("planar-information", L, graph=(X, e, Z, Om, fixed, extras))
    check_properties(f"planar information, L = {L}", out, X, fixed, extras["params"]["max_iteration"])
    if L is not None:
        assert out["coarse_stats"][0] == Cr.aggregates(len(X), L) and 0 <= out["coarse_stats"][1] <= out["stats"][0]


@pytest.mark.parametrize("apart", [False, True], ids=["anchored", "apart"])
@pytest.mark.parametrize("kind", D.NON_FINITE)
@pytest.mark.parametrize("L", [None, 2])
def test_non_finite_input(kind, apart, L):
    X, e, Z, Om, fixed, extras = D.non_finite(kind, apart)
    out = device(kind, L, graph=(X, e, Z, Om, fixed, extras))
    check_properties(f"{kind}, apart {apart}, L = {L}", out, X, fixed, extras["params"]["max_iteration"])
    assert not np.isfinite(out["stats"][INITIAL_COST])
    assert out["poses"].tobytes() == X.tobytes() and out["stats"][ACCEPTED] == 0
    if L is not None:
        return
    # the system: what the bad entry does not touch has the bits of the graph without it
    got, clean = plain_linearize(X, e, Z, Om), plain_linearize(*extras["clean"])
    edges = np.setdiff1d(np.arange(len(e)), extras["edges"])
    poses = np.setdiff1d(np.arange(len(X)), extras["poses"])
    assert got["residuals"][edges].tobytes() == clean["residuals"][edges].tobytes()
    for k in ("gradient", "blocks"):
        assert got[k][poses].tobytes() == clean[k][poses].tobytes(), k
    assert got["skipped"][0] == 0 and not np.isfinite(got["cost"][0])
    if apart:
        assert set(range(6)) <= set(poses.tolist())           # the whole component of the fixed pose


def test_corridor_closure_through_the_python_layer():
    from neural_spectral_codec_amd.retrieval import pose_graph as pg
    X, e, Z, Om, cand = D.corridor_candidate()
    q = len(X) - 1
    ce, cZ, cOm = pg.closure_edges(q, [cand])
    assert ce.tolist() == [[1, q]] and np.linalg.matrix_rank(cOm[0]) == 5
    for L in (None, 4):
        opt = pg.PoseGraphOptimizer(coarse_block=L, max_iteration=8, pcg_tolerance=1e-10, max_pcg_iterations=200)
        out = opt.optimize(X, np.concatenate([e, ce]), np.concatenate([Z, cZ]), np.concatenate([Om, cOm]))
        before = P.residual(X[1], X[q], cZ[0])
        after = P.residual(out["poses"][1], out["poses"][q], cZ[0])
        print(f"corridor closure, L = {L}: chi2 of the closure {before @ cOm[0] @ before:.6g} -> "
              f"{after @ cOm[0] @ after:.6g}, cost {out['cost0']:.6g} -> {out['cost']:.6g}, accepted {out['accepted']}")
        assert np.isfinite(out["poses"]).all() and out["accepted"] >= 1 and out["cost"] < out["cost0"]
        assert after @ cOm[0] @ after < before @ cOm[0] @ before
        assert np.all(np.diff(out["cost_history"]) <= 0)
        cov = opt.covariance(X, e, Z, Om, [1, q])                 # the graph without the closure gates it
        assert cov["converged"].all() and cov["not_free"] == 0
        rel = pg.relative_covariance(cov["joint"], X[1], X[q])
        assert np.isfinite(rel).all() and np.array_equal(rel, rel.T) or np.abs(rel - rel.T).max() <= 1e-12 * np.abs(rel).max()
        assert np.linalg.eigvalsh(0.5 * (rel + rel.T))[0] > 0.0
        d2 = pg.closure_mahalanobis(cZ[0], cOm[0], X[1], X[q], rel)
        print("closure_mahalanobis", d2)
        assert np.isfinite(d2) and d2 >= 0.0
