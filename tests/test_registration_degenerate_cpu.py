"""The singular and barely regular registration inputs (tests/registration_degenerate_cases.py) without a GPU: from the
float64 restatements alone, every input is what its name claims, and the two thresholds -- TAU_REF of the references'
no-step rule and gn_solve6's relative pivot bound TAU_KERNEL (tests/gauss_newton_restatement.py,
csrc/nsc_gauss_newton.h) -- are measured again and asserted with their margins.

Run with -s to see, per family, the rank evidence (|H n| / (||H|| |n|) or lambda_min / lambda_max), whether gn_solve6's
factorisation order with the absolute test d_j > 0 would have stepped, and the measured figures."""
import numpy as np
import pytest

import gauss_newton_restatement as GN
import gicp_clouds as F
import gicp_restatement as G
import map_localize_cases as K
import map_localize_restatement as R
import map_robust_restatement as RR
import registration_degenerate_cases as D
from test_gicp_families_cpu import MANY_SMALL_SEED, MIN_GAP

NULL_BAR = 1e-9                          # |H n| <= NULL_BAR ||H|| |n| for a singular case's analytic null vectors
# lambda_min / lambda_max of the reference H of a regular family stays above this at every round of the reference's
# iteration; measured: plane_far 3.9e-9, line_plus_one-1.0 1.9e-7, line_plus_one-0.1 2.1e-9
REGULAR_FLOOR = 1e-9
# The largest |u . d| over the rows of the eight 40-row lines, u the epsilon-eigenvector of the reference's covariance
# (numpy's eigh of the rank-1 neighbourhood covariance, read back from the (epsilon, 1, 1) matrix by ``normal_of``) and
# d the line's direction: measured 2.5e-16.  The GPU test bounds the kernel's by ten times this figure (its own largest
# on the MI355X: 2.2e-16).
U_DOT_D_REF = 3e-16
SCAN_CONFIGS = {"plain": dict(), "robust": dict(kernel=D.ROBUST[0], scale=D.ROBUST[1], neighbours=D.ROBUST[2])}


def numerical_rank(H):
    lam = np.linalg.eigvalsh(H)
    return int((lam > 1e-9 * lam[-1]).sum())


@pytest.fixture
def systems(monkeypatch):
    """every H the references hand to their no-step rule while the test runs"""
    seen, rule = [], GN.regular
    monkeypatch.setattr(GN, "regular", lambda H: (seen.append(np.array(H, np.float64)), rule(H))[1])
    return seen


# ---- GICP ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", D.SINGULAR + D.REGULAR)
def test_gicp_case_is_what_it_claims(name, systems):
    c = D.gicp_cases()[name]
    assert D.own_voxels(c["source"]) and (len(c["target"]) > 100 or D.own_voxels(c["target"])), name
    assert len(c["source"]) <= 310 and len(c["target"]) <= 310
    src, tgt, cov, lin = D.gicp_reference(c)
    assert lin["n_corr"] == len(src) and F.radius_margin(src, tgt, c["init"], 1.0) > 1e-3
    if name in ("one_row", "two_rows"):                          # a sampled surface: its covariances must be determined
        r = F.cloud_reference(c["target"], D.PARAMS)
        assert r["sep"].all() and r["gap"] > MIN_GAP and 150 <= len(tgt) <= 250
        assert np.abs(c["target"][:, :3]).min() >= 0.5          # exact in units of 2^-24 m
    H = lin["H"]
    ref = G.register(c["source"], c["target"], init=c["init"], exact=True)
    if c["singular"]:
        res, taken = D.null_residual(H, c["null"]), GN.kernel_order_cholesky(H)
        print(f"{name}: |H n| / (||H|| |n|) = {res:.3g}, lambda_min / lambda_max = {GN.eig_ratio(H):.3g}, rank "
              f"{numerical_rank(H)}; d_j > 0 in gn_solve6's order would {'step' if taken[0] else 'not step'} "
              f"(pivot {taken[1]}, d_j / H_jj = {taken[2]:.3g})")
        assert res <= NULL_BAR and numerical_rank(H) == c["rank"] and not GN.regular(H)
        assert np.array_equal(ref["transform"], c["init"]) and ref["iterations"] == 1
        assert ref["n_corr"] == lin["n_corr"] and ref["fitness"] == 1.0 and ref["rmse"] == lin["rmse"] > 0.01
    else:
        ratios = [GN.eig_ratio(h) for h in systems]
        print(f"{name}: lambda_min / lambda_max over the reference's {len(ratios)} rounds >= {min(ratios):.3g} "
              f"(floor {REGULAR_FLOOR:.3g}), {ref['iterations']} iterations, rmse {lin['rmse']:.3g} -> {ref['rmse']:.3g}")
        assert min(ratios) > REGULAR_FLOOR > 100 * GN.TAU_REF and numerical_rank(H) == 6
        assert 1 < ref["iterations"] < 30 and ref["rmse"] < 1e-4 * lin["rmse"]           # the step is taken and lands
        truth = c.get("truth")
        if truth is None:
            truth = np.eye(4)
            truth[:3, 3] = D.SHIFT
        te, re = G.pose_error(ref["transform"], truth)
        assert te <= 1e-4 and re <= 1e-5, (name, te, re)


def test_line_covariances_have_a_free_normal():
    """A collinear neighbourhood has a rank-1 covariance: the normal is any unit vector across the line, so the
    reference's matrix is U diag(epsilon, 1, 1) U^T with u perpendicular to d, and nothing more can be asked of the
    kernel's."""
    worst = 0.0
    for name in D.LINES_40:
        c = D.gicp_cases()[name]
        src, _, cov, _ = D.gicp_reference(c)
        idx, _ = G.knn_exact(src, 20)
        lam = G.neighbour_eigenvalues(src, idx)
        assert np.abs(lam[:, :2]).max() <= 1e-12 * lam[:, 2].min()                       # rank 1, every row
        w, u = D.normal_of(cov[0])
        assert np.abs(w - np.array([1e-3, 1.0, 1.0])).max() <= 1e-9
        worst = max(worst, float(np.abs(u @ c["line"][1]).max()))
    print(f"40-row lines: the reference's largest |u . d| = {worst:.3g} (U_DOT_D_REF {U_DOT_D_REF:.3g})")
    assert worst <= U_DOT_D_REF


# ---- scan to map --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("config", list(SCAN_CONFIGS))
@pytest.mark.parametrize("name", D.SCAN_BATCH)
def test_scan_case_is_what_it_claims(name, config):
    c, m, kw = D.scan_cases()[name], K.scene_reference()["map"], SCAN_CONFIGS[config]
    s0 = RR.linearize(m, c["scan"], c["init"], **kw)
    H = R.full(s0)
    ref = RR.register_one(m, c["scan"], c["init"], **kw)
    if not c["singular"]:
        print(f"{name} {config}: lambda_min / lambda_max = {GN.eig_ratio(H):.3g}")
        assert GN.eig_ratio(H) > 1e-3 and ref["iterations"] > 1 and not np.array_equal(ref["transform"], c["init"])
        return
    n = len(c["scan"])
    assert R.keep_off_faces(m, c["scan"], c["init"], K.FACE_MARGIN).all()
    assert s0[27] >= min(n, 5) and (s0[27] == n or n == 40), (name, s0[27])
    res, taken = D.null_residual(H, c["null"]), GN.kernel_order_cholesky(H)
    print(f"{name} {config}: {int(s0[27])} of {n} rows, {int(s0[31])} pairs, |H n| / (||H|| |n|) = {res:.3g}, "
          f"lambda_min / lambda_max = {GN.eig_ratio(H):.3g}; d_j > 0 in gn_solve6's order would "
          f"{'step' if taken[0] else 'not step'} (pivot {taken[1]}, d_j / H_jj = {taken[2]:.3g})")
    assert res <= NULL_BAR and numerical_rank(H) == c["rank"] and not GN.regular(H)
    assert np.array_equal(ref["transform"], c["init"]) and ref["iterations"] == 1
    assert np.array_equal(ref["system0"], s0) and np.array_equal(ref["information"], H)


def test_plain_options_are_the_plain_restatement():
    m = K.scene_reference()["map"]
    for name in D.SCAN_SINGULAR:
        c = D.scan_cases()[name]
        a, b = R.register_one(m, c["scan"], c["init"]), RR.register_one(m, c["scan"], c["init"])
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])[..., :30] if k == "system0" else np.asarray(b[k])), k


# ---- the thresholds -----------------------------------------------------------------------------------------------------

def singular_systems():
    """(name, H) of every singular family at its initial transform, GICP and scan to map (both configurations)"""
    out = [(n, D.gicp_reference(D.gicp_cases()[n])[3]["H"]) for n in D.SINGULAR]
    m = K.scene_reference()["map"]
    for n in D.SCAN_SINGULAR:
        c = D.scan_cases()[n]
        out += [(f"{n} {cfg}", R.full(RR.linearize(m, c["scan"], c["init"], **kw))) for cfg, kw in SCAN_CONFIGS.items()]
    return out


def test_thresholds(systems):
    """(a) the largest |d_j| / H_jj at the rejecting or last pivot of gn_solve6's factorisation order (float64, absolute
    test) over every singular family, and over the systems of many_small that the rule calls singular; (b) the smallest
    pivot ratio over every regular system the suite has, at every round of the references' iterations: END_TO_END,
    STAGE_CASES from their fixed transforms, the rank-6 pairs of many_small, the scene's eight scans (plain and
    robust), plane_far and line_plus_one.  TAU_KERNEL is their geometric mean; TAU_REF the same of the eigenvalue
    ratios."""
    singular = singular_systems()
    fam = [GN.kernel_order_cholesky(H) for _, H in singular]
    stepped = [n for (n, _), f in zip(singular, fam) if f[0]]
    print(f"singular families: d_j > 0 in gn_solve6's order would step on {len(stepped)} of {len(singular)}: {stepped}")
    assert len(singular) // 5 <= len(stepped) <= len(singular) * 3 // 5                 # the gap was real
    a_fam = max(abs(f[2]) for f in fam)
    e_fam = max(abs(GN.eig_ratio(H)) for _, H in singular)

    groups = {}

    def ran(what):
        groups[what] = list(systems)
        del systems[:]
    for name, (build, params, _) in F.END_TO_END.items():
        A, B, _ = build()
        G.register(A, B, exact=True, **params)
    ran("END_TO_END")
    for name in F.STAGE_CASES:
        A, B, T_fix, params, _ = F.stage_case(name)
        G.register(A, B, init=T_fix, **params)
    ran("STAGE_CASES")
    for a, b in zip(*F.many_small(MANY_SMALL_SEED)):
        G.register(a, b)
    ran("many_small")
    s, m = K.scene(), K.scene_reference()["map"]
    R.register(m, s["scans"], s["scan_offsets"], s["init"])
    RR.register(m, s["scans"], s["scan_offsets"], s["init"], **SCAN_CONFIGS["robust"])
    ran("scene")
    for name in D.REGULAR:
        c = D.gicp_cases()[name]
        G.register(c["source"], c["target"], init=c["init"], exact=True)
    ran("families 4 and 5")

    small = groups["many_small"]
    small_singular = [H for H in small if abs(GN.eig_ratio(H)) <= 1e-12]
    groups["many_small"] = [H for H in small if GN.eig_ratio(H) > 1e-12]
    assert len(small_singular) >= 20 and len(groups["many_small"]) >= 2000
    a_small = max(abs(GN.kernel_order_cholesky(H)[2]) for H in small_singular)
    e_small = max(abs(GN.eig_ratio(H)) for H in small_singular)
    a, e_sing = max(a_fam, a_small), max(e_fam, e_small)
    print(f"(a) largest |d_j| / H_jj at the rejecting or last pivot: families {a_fam:.3g}, many_small's {len(small_singular)} "
          f"singular systems {a_small:.3g}; largest |lambda_min / lambda_max|: {e_fam:.3g}, {e_small:.3g}")
    b, e_reg = np.inf, np.inf
    for what, Hs in groups.items():
        facts = [GN.kernel_order_cholesky(H) for H in Hs]
        assert all(f[0] for f in facts), what
        pb, eb = min(f[3] for f in facts), min(GN.eig_ratio(H) for H in Hs)
        print(f"(b) {what}: {len(Hs)} systems, smallest pivot ratio {pb:.3g}, smallest lambda_min / lambda_max {eb:.3g}")
        b, e_reg = min(b, pb), min(e_reg, eb)
    tau, tau_ref = np.sqrt(a * b), np.sqrt(e_sing * e_reg)
    print(f"(a) {a:.3g}  (b) {b:.3g}  gap {b / a:.3g}  tau {tau:.3g} (TAU_KERNEL {GN.TAU_KERNEL:.3g}); eigenvalue ratios "
          f"{e_sing:.3g} / {e_reg:.3g}, tau_ref {tau_ref:.3g} (TAU_REF {GN.TAU_REF:.3g})")
    assert b / a >= 1e4
    assert a < GN.TAU_KERNEL / 100 and b > 100 * GN.TAU_KERNEL
    assert 0.5 <= GN.TAU_KERNEL / tau <= 2.0                                           # the written figure is this mean
    # eigvalsh's error is a few units of 2^-53 of lambda_max, and a far-away cloud (STAGE_CASES far-v0.5-k20, 2 km from
    # the origin) is regular at 1.3e-13: the reference's rule has a decade on either side, not two
    assert e_sing < GN.TAU_REF / 10 and e_reg > 10 * GN.TAU_REF
    assert 0.5 <= GN.TAU_REF / tau_ref <= 2.0
    # with the relative test every decision is the rule's
    for _, H in singular:
        assert not GN.kernel_order_cholesky(H, GN.TAU_KERNEL)[0]
    for H in small_singular:
        assert not GN.kernel_order_cholesky(H, GN.TAU_KERNEL)[0]
    for Hs in groups.values():
        assert all(GN.kernel_order_cholesky(H, GN.TAU_KERNEL)[0] for H in Hs)
