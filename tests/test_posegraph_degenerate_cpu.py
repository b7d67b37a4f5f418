"""The constructed graphs of tests/posegraph_degenerate_cases.py against the restatement alone, no device: that every case
reaches the branches it claims, that every decision the restatement takes on a decidable case has a relative margin of at
least 1e-6 -- the bar the device is compared at (close() in test_posegraph_gpu.py), so a device result inside the bar takes
the same branch -- and that a restatement with one rule broken is told apart by the quantities test_posegraph_degenerate_gpu.py
compares.  The margins are a condition on the inputs, met by the choice of weights, seeds and lambda0."""
import numpy as np
import pytest

import posegraph_coarse_restatement as Cr
import posegraph_cov_restatement as V
import posegraph_degenerate_cases as D
import posegraph_restatement as P
import posegraph_robust_restatement as R

B = dict(zip(("block", "identity", "failed", "ok-indefinite", "pap", "fail-succeed", "succeed-fail"), D.BRANCHES))

# (case, L) -> the branches its run reaches
FAMILIES = {
    ("zero-leaf", None): {"block"},
    ("zero-leaf", 2): {"block", "identity"},
    ("negative-leaf", None): {"block"},
    ("negative-leaf", 2): {"block", "identity"},
    ("chords-4", None): {"block", "pap"},
    ("chords-4", 2): {"block", "failed", "pap"},
    ("chords-9", None): {"block", "pap"},
    ("chords-9", 2): {"block", "failed", "pap"},
    ("chords-9", 4): {"block", "failed", "pap"},
    ("chords-17", None): {"block", "pap"},
    ("chords-17", 2): {"block", "failed", "pap"},
    ("chords-17", 4): {"block", "ok-indefinite", "pap"},
    ("chords-65", 8): {"block", "identity", "ok-indefinite", "pap"},
    ("lambda-walk-up", 2): {"block", "failed", "fail-succeed", "succeed-fail", "pap"},
    ("lambda-walk-down", 2): {"block", "failed", "succeed-fail", "pap"},
    ("robust-indefinite", None): {"block", "pap"},
    ("robust-indefinite", 2): {"block", "failed", "pap"},
}

# mutant -> decidable runs that must tell it from the restatement
CAUGHT_BY = {
    "block-free": [("negative-leaf", None), ("chords-9", 2), ("chords-65", 8)],
    "stale-inverse": [("lambda-walk-up", 2), ("lambda-walk-down", 2)],
    "breakdown-steps": [("chords-4", None), ("chords-17", 4), ("lambda-walk-down", 2)],
    "breakdown-uncounted": [("chords-9", None), ("lambda-walk-up", 2)],
    "no-lambda-coarse": [("chords-17", 4), ("lambda-walk-down", 2)],
}
COUNTS = ("accepted", "rejected", "pcg_iterations", "coarse_failed", "converged")

_RUNS = {}


def run(name, L):
    if (name, L) not in _RUNS:
        _RUNS[name, L] = D.run(name, L)
    return _RUNS[name, L]


def test_the_table_lists_every_run():
    assert list(FAMILIES) == D.instances()
    assert set(CAUGHT_BY) == set(D.MUTANTS)


@pytest.mark.parametrize("name,L", D.instances())
def test_traced_restatement_is_the_restatement(name, L):
    """bit for bit, so that what the trace says holds for the run the device is compared with"""
    got, ref = run(name, L), D.reference(name, L)
    for k in ("poses", "cost_history", "step0"):
        assert got[k].tobytes() == ref[k].tobytes(), k
    for k in COUNTS + ("iterations", "inner", "coarse_aggregates", "cost0", "cost"):
        assert got[k] == ref[k], k


@pytest.mark.parametrize("name,L", D.instances())
def test_every_decision_has_a_margin(name, L):
    tr = run(name, L)["trace"]
    what, worst = min(tr["margins"], key=lambda t: t[1])
    print(f"{name}, L = {L}: {len(tr['margins'])} decisions, the smallest margin {worst:.3g} ({what})")
    assert worst >= D.BAR, (what, worst)
    assert "r.z <= 0" not in tr["branches"]                   # a rule of the device that the restatement does not have


@pytest.mark.parametrize("name", list(D.DECIDABLE))
def test_first_step_does_not_depend_on_the_form_of_the_block_solve(name):
    """The margins bound what rounding may do to one decision, not what many inner iterations do to the step.  Two float64
    forms of block-Jacobi PCG, the explicit inverses of posegraph_coarse_restatement and the triangular solves of
    posegraph_restatement (what the device does), agree in the count and to a thousandth of the bar in the step."""
    X, e, Z, Om, fixed, extras = D.decidable(name)
    prm = dict(P.DEFAULTS, **extras["params"])
    lin = Cr.linearize(X, e, Z, Om, extras.get("kernel", R.NONE), extras.get("scale"))
    free = Cr.free_nodes(len(X), e, fixed, lin["blocks"], prm["lambda0"])
    a, its_a, _ = Cr.pcg_step(lin["H"], lin["gradient"], lin["blocks"], prm["lambda0"], free, prm["max_pcg_iterations"],
                              prm["pcg_tolerance"])
    b, its_b = P.pcg_step(lin["H"].toarray(), lin["gradient"], prm["lambda0"], free, prm["max_pcg_iterations"],
                          prm["pcg_tolerance"])
    gap = np.abs(a - b).max() / np.abs(a).max()
    print(name, "inner iterations", its_a, its_b, "distance of the two steps / largest entry", gap)
    assert its_a == its_b and gap <= 1e-3 * D.BAR


@pytest.mark.parametrize("name,L", D.instances())
def test_branches_reached(name, L):
    assert run(name, L)["trace"]["branches"] == {B[k] for k in FAMILIES[name, L]}


def test_every_branch_is_reached_by_some_case():
    assert {B[k] for s in FAMILIES.values() for k in s} == set(D.BRANCHES)


def test_the_chord_family_is_what_it_says():
    """at lambda0 = 1e-4: 2 of 3, 5 of 8 and 9 of 16 poses free, an indefinite free system, a failed factor for L = 2, and
    at n = 17, L = 4 a factor that exists although A is indefinite; from lambda = 1 on everything is positive definite"""
    for name, n_free in (("chords-4", 2), ("chords-9", 5), ("chords-17", 9)):
        X, e, Z, Om, fixed, extras = D.decidable(name)
        n = len(X)
        lin = Cr.linearize(X, e, Z, Om)
        free = Cr.free_nodes(n, e, fixed, lin["blocks"], 1e-4)
        assert free.sum() == n_free and not free[extras["not_free"]].any()
        m = np.repeat(free, 6)
        H = lin["H"].toarray()
        A = (H + 1e-4 * np.diag(np.diag(H)))[np.ix_(m, m)]
        ev = np.linalg.eigvalsh(A)
        print(name, "eigenvalues of the free system", ev[0], "..", ev[-1])
        assert ev[0] < -1e-4 * ev[-1]                         # indefinite by a hundred times the bar
        assert Cr.Preconditioner(lin["H"], lin["blocks"], 1e-4, free, X, 2).failed
        assert Cr.Preconditioner(lin["H"], lin["blocks"], 1e-4, free, X, 4).failed == (name != "chords-17")
        for lam in (1.0, 10.0):
            free = Cr.free_nodes(n, e, fixed, lin["blocks"], lam)
            m = np.repeat(free, 6)
            assert free.sum() >= n_free and np.linalg.eigvalsh((H + lam * np.diag(np.diag(H)))[np.ix_(m, m)])[0] > 0.0
            assert not Cr.Preconditioner(lin["H"], lin["blocks"], lam, free, X, 2).failed


def test_chords_65_has_an_aggregate_without_a_free_pose():
    X, e, Z, Om, fixed, _ = D.decidable("chords-65")
    free = run("chords-65", 8)["trace"]["free"][0]
    assert not free[24:32].any() and not fixed[24:32].any() and free[64] and Cr.aggregates(65, 8) == 9
    assert all(free[8 * a:8 * a + 8].any() for a in (1, 2, 4, 5, 6, 7, 8))


def test_leaf_cases():
    X, e, Z, Om, fixed, _ = D.decidable("zero-leaf")
    lin = Cr.linearize(X, e, Z, Om)
    assert not lin["blocks"][6].any() and not lin["gradient"][6].any()           # exactly zero
    without = Cr.linearize(X[:6], e[:-1], Z[:-1], Om[:-1])
    assert lin["blocks"][:6].tobytes() == without["blocks"].tobytes()            # the edge changes no other pose
    X, e, Z, Om, fixed, _ = D.decidable("negative-leaf")
    lin = Cr.linearize(X, e, Z, Om)
    assert np.linalg.eigvalsh(lin["blocks"][6])[-1] < 0.0 and np.linalg.eigvalsh(lin["blocks"][2])[0] > 0.0


def test_robust_weights_scale_indefinite_blocks():
    X, e, Z, Om, fixed, extras = D.decidable("robust-indefinite")
    chi2, w = R.edge_weights(X, e, Z, Om, extras["kernel"], extras["scale"])
    chord = np.arange(len(e)) >= len(e) - extras["chords"]
    assert (w[~chord] == 1.0).all()
    assert ((w[chord] < 0.01) == (chi2[chord] > 0.0)).all() and (w[chord] < 0.01).sum() == 2 and (chi2[chord] < 0).any()
    for k in np.nonzero(chord & (w < 1.0))[0]:
        assert np.linalg.eigvalsh(Om[k])[0] < 0.0 < np.linalg.eigvalsh(Om[k])[-1]


@pytest.mark.parametrize("mutant", D.MUTANTS)
def test_mutant_is_caught(mutant):
    """every listed run moves outside the bar (poses or first step) or changes a count"""
    for name, L in CAUGHT_BY[mutant]:
        ref, got = run(name, L), D.run(name, L, mutant=mutant)
        counts = [k for k in COUNTS if got[k] != ref[k]]
        moved = max(np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max() for k in ("poses", "step0", "cost_history"))
        print(mutant, name, L, "counts that change:", counts, "largest relative move", moved)
        assert counts or moved > 10.0 * D.BAR, (mutant, name, L)


# ---- the covariance call ------------------------------------------------------------------------------------------------

def test_covariance_columns_on_the_chords():
    X, e, Z, Om, fixed, extras = D.decidable("chords-9")
    nodes = list(range(1, 9))
    lin, free = V.system(X, e, Z, Om, fixed)
    assert np.array_equal(np.nonzero(~free)[0], [0, 1, 3, 5])                     # lambda = 0: the odd poses with a chord
    ref_its = V.pcg_columns(lin, free, nodes, max_pcg_iterations=100)[1]
    for L in (None, 2, 4):
        joint, its, free2, tr = D.traced_columns(X, e, Z, Om, fixed, nodes, L)
        what, worst = min(tr["margins"], key=lambda t: t[1])
        print("chords-9 covariance, L =", L, "iterations", its.tolist(), "smallest margin", worst, what)
        assert np.array_equal(free, free2) and np.array_equal(its, ref_its)
        assert worst >= D.BAR and tr["failed"] == (L is not None) and "r.z <= 0" not in tr["branches"]
        assert tr["branches"] == {B["pap"]} and (its[free[nodes]] >= 1).all() and not its[~free[nodes]].any()


def test_covariance_two_components():
    X, e, Z, Om, fixed, extras = D.cov_two_components()
    nodes = extras["healthy"] + extras["degenerate"]
    for L in (None, 4):
        joint, its, free, tr = D.traced_columns(X, e, Z, Om, fixed, nodes, L)
        what, worst = min(tr["margins"], key=lambda t: t[1])
        print("two components, L =", L, "iterations", its.tolist(), "smallest margin", worst, what)
        assert worst >= D.BAR and tr["failed"] == (L is not None)
        assert free[extras["healthy"]].all() and free[extras["degenerate"]].tolist() == [True, True, False, True]
        assert (its[:3] > its[3:].max()).all()                 # the healthy columns converge; the others break down early


# ---- the undecidable cases ----------------------------------------------------------------------------------------------

def test_planar_information_has_pivots_at_rounding_level():
    X, e, Z, Om, fixed, _ = D.planar_information()
    assert all(np.linalg.matrix_rank(W, tol=1e-9) == 3 for W in Om)
    lin = Cr.linearize(X, e, Z, Om)
    ev = np.linalg.eigvalsh(lin["blocks"][1:])
    print("planar information: eigenvalues of the blocks", ev.min(0), ev.max(0))
    assert (np.abs(ev[:, :3]) < 1e-12 * ev[:, -1:]).all() and (ev[:, 3] > 1e-3 * ev[:, -1]).all()


def test_corridor_closure_has_rank_five():
    from types import SimpleNamespace
    X, e, Z, Om, cand = D.corridor_candidate()
    assert isinstance(cand, SimpleNamespace) and np.linalg.matrix_rank(cand.information_matrix) == 5
    W = D._conjugated(np.asarray(cand.information_matrix), cand.transform)       # as pose_graph.closure_edges forms it
    ev = np.linalg.eigvalsh(W)
    assert abs(ev[0]) < 1e-9 * ev[-1] and ev[1] > 1e-9 * ev[-1]


@pytest.mark.parametrize("kind", D.NON_FINITE)
@pytest.mark.parametrize("apart", [False, True])
def test_non_finite_cases(kind, apart):
    X, e, Z, Om, fixed, extras = D.non_finite(kind, apart)
    cX, ce, cZ, cOm = extras["clean"]
    assert sum(int((~np.isfinite(a)).sum()) for a in (X, Z, Om)) == 1 and np.array_equal(e, ce)
    assert all(np.isfinite(a).all() for a in (cX, cZ, cOm)) and P.valid_edges(len(X), e).all()
    assert not np.isfinite(R.cost(X, e, Z, Om)) and np.isfinite(R.cost(cX, ce, cZ, cOm))
    anchored = set(range(6))
    assert set(extras["poses"]).isdisjoint(anchored) == apart  # apart: the fixed pose's component is untouched
