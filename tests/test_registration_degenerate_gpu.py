"""Singular and barely regular Gauss-Newton systems on the MI355X: GICP (register_packed on raw clouds and
register_prepared on a PreparedClouds store) and scan-to-map registration (MapLocalizer.register, plain and with a robust
kernel and face neighbours) on the inputs of tests/registration_degenerate_cases.py, whose claims
tests/test_registration_degenerate_cpu.py asserts from the restatements alone.

The contract.  Where the reference system is singular -- by construction: the case carries its null vectors -- the step
is the identity: the transform comes back as the initial one bit for bit, iterations == 1, and every other output is the
reference's linearisation at the initial transform.  Where it is regular, however badly conditioned, the step is taken
and the result is the reference's.

Tolerances are the project's: system terms 1e-6 relative (test_gicp_paths_gpu.check_system,
test_map_localize_gpu.test_system0_against_restatement), end to end 1e-3 m / 1e-4 on rotation entries / 1e-3 on fitness
and on the information matrix (test_gicp_paths_gpu.test_end_to_end); null vectors |H n| <= 1e-9 ||H|| |n|.

The covariance of a row whose neighbours are collinear is U diag(epsilon, 1, 1) U^T with any u across the line, so the
reference's own choice of u says nothing about the kernel's.  For the collinear clouds the kernel's covariances are
checked for what is determined (the eigenvalues, and u . d = 0 within ten times the reference's own figure,
test_registration_degenerate_cpu.U_DOT_D_REF) and then handed to the reference's linearisation in place of its own."""
import numpy as np
import pytest

import gicp_restatement as G
import map_localize_cases as K
import map_localize_restatement as R
import map_robust_restatement as RR
import registration_degenerate_cases as D
from test_gicp_gpu import run
from test_gicp_paths_gpu import full3
from test_gicp_store_gpu import assert_bitwise, prepared, raw, store_of
from test_map_robust_gpu import host, localizer, options, with_options
from test_registration_degenerate_cpu import NULL_BAR, SCAN_CONFIGS, U_DOT_D_REF

pytestmark = pytest.mark.gpu


def close(got, ref):
    return np.allclose(got, ref, rtol=1e-6, atol=1e-6 * max(np.abs(ref).max(), 1e-300))


# ---- GICP ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed():
    """families 1 .. 5 in one call (``mixed_batch``): singular pairs at both ends and in the middle"""
    cases = list(D.gicp_cases().values())
    S, T = [c["source"] for c in cases], [c["target"] for c in cases]
    out = run(S, T, [c["init"] for c in cases], stages=True)
    so = np.concatenate([[0], np.cumsum([len(c) for c in S])])
    to = so[-1] + np.concatenate([[0], np.cumsum([len(c) for c in T])])
    return cases, out, so, to


def stage_clouds(mixed, p):
    """pair p's down-sampled clouds and covariances as the kernels left them: (points, (n,3,3)) of source and target"""
    cases, out, so, to = mixed
    P = len(cases)
    got = []
    for at, c in ((so[p], p), (to[p], P + p)):
        n = int(out["counts"][c])
        got.append((out["points"][at:at + n], full3(out["covariances"][at:at + n])))
    return got


@pytest.mark.parametrize("name", D.SINGULAR)
def test_gicp_singular_system_takes_no_step(mixed, name):
    cases, out, _, _ = mixed
    p = [c["name"] for c in cases].index(name)
    c = cases[p]
    (ps, cs), (pt, ct) = stage_clouds(mixed, p)
    src, tgt, cov, lin = D.gicp_reference(c)
    assert np.array_equal(ps, src) and len(ps) == len(c["source"])   # every source row its own voxel on the device too
    assert np.array_equal(pt, tgt) if c["line"] else np.abs(pt - tgt).max() <= 1e-6
    for C in (cs, ct):
        assert np.abs(np.linalg.eigvalsh(C) - np.array([1e-3, 1.0, 1.0])).max() <= 1e-9, name
    if c["line"]:                                                    # a free normal: take the kernel's (module docstring)
        for C in (cs, ct):
            dot = float(np.abs(D.normal_of(C)[1] @ c["line"][1]).max())
            print(f"{name}: largest |u . d| = {dot:.3g} (bar {10 * U_DOT_D_REF:.3g})")
            assert dot <= 10 * U_DOT_D_REF, name
        lin = D.gicp_reference(c, cov=(cs, ct))[3]
    s0 = out["system0"][p]
    H = D.hessian(s0)
    print(f"{name}: iterations {out['iterations'][p]}, |H n| / (||H|| |n|) = {D.null_residual(H, c['null']):.3g}, "
          f"moved {np.abs(out['transform'][p] - c['init']).max():.3g}")
    assert out["transform"][p].tobytes() == c["init"].tobytes(), (name, out["transform"][p])
    assert out["iterations"][p] == 1
    assert D.null_residual(H, c["null"]) <= NULL_BAR
    assert s0[27] == lin["n_corr"] == out["n_correspondences"][p] == len(src)
    assert close(H, lin["H"]) and close(s0[21:27], lin["g"]), name
    assert abs(s0[28] - lin["sse"]) <= 1e-6 * lin["sse"]
    assert abs(out["fitness"][p] - lin["fitness"]) <= 1e-6 * lin["fitness"]
    assert abs(out["rmse"][p] - lin["rmse"]) <= 1e-6 * lin["rmse"]
    assert close(out["information"][p], lin["info"]), name


@pytest.mark.parametrize("name", D.REGULAR)
def test_gicp_regular_system_takes_its_step(mixed, name):
    cases, out, _, _ = mixed
    p = [c["name"] for c in cases].index(name)
    c = cases[p]
    ref = G.register(c["source"], c["target"], init=c["init"], exact=True)
    T = out["transform"][p]
    print(f"{name}: iterations {out['iterations'][p]} / {ref['iterations']}, "
          f"dt {np.abs(T[:3, 3] - ref['transform'][:3, 3]).max():.3g}, "
          f"dR {np.abs(T[:3, :3] - ref['transform'][:3, :3]).max():.3g}, rmse {out['rmse'][p]:.3g}")
    assert out["iterations"][p] > 1 and not np.array_equal(T, c["init"])
    assert np.abs(T[:3, 3] - ref["transform"][:3, 3]).max() <= 1e-3
    assert np.abs(T[:3, :3] - ref["transform"][:3, :3]).max() <= 1e-4
    assert abs(out["fitness"][p] - ref["fitness"]) <= 1e-3 and out["n_correspondences"][p] == ref["n_corr"]
    info = ref["information"]
    assert np.abs(out["information"][p] - info).max() <= 1e-3 * np.abs(info).max()


def test_gicp_mixed_batch_store_and_independence(mixed):
    """raw against prepared bit for bit, and every pair alone equals itself in the batch"""
    cases, out, _, _ = mixed
    P = len(cases)
    S, T = [c["source"] for c in cases], [c["target"] for c in cases]
    store, ids = store_of(S + T)
    got = prepared(store, ids[:P], store, ids[P:])
    for i in range(P):
        assert_bitwise(got, i, out, i, cases[i]["name"])
        assert_bitwise(raw([S[i]], [T[i]]), 0, out, i, cases[i]["name"] + " alone")
    singular = [i for i, c in enumerate(cases) if c["singular"]]
    assert singular[0] == 0 and singular[-1] == P - 1 and len(singular) == len(D.SINGULAR) == P - len(D.REGULAR)


# ---- scan to map --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene_map():
    s = K.scene()
    m = localizer(voxel_size=1.0)
    assert m.build(list(np.split(s["points"], 6)), s["poses"])["complete"]
    return m


def configured(scene_map, config):
    return scene_map if config == "plain" else with_options(scene_map, **options(*D.ROBUST))


@pytest.mark.parametrize("config", list(SCAN_CONFIGS))
def test_scan_mixed_batch(scene_map, config):
    """``scan_one_row``, ``scan_line`` (5 and 40 rows) beside two of the scene's scans in one call: the singular ones
    keep their initial pose by bits after one iteration and return the reference's sums there; every scan alone equals
    itself in the batch"""
    m, ref_map, kw = configured(scene_map, config), K.scene_reference()["map"], SCAN_CONFIGS[config]
    cases = [D.scan_cases()[n] for n in D.SCAN_BATCH]
    scans, init = [c["scan"] for c in cases], np.stack([c["init"] for c in cases])
    out = host(m.register(scans, init, system0=True))
    for i, (name, c) in enumerate(zip(D.SCAN_BATCH, cases)):
        alone = host(m.register([c["scan"]], c["init"][None], system0=True))
        for k in out:
            assert alone[k][0].tobytes() == out[k][i].tobytes(), (name, k)
        if not c["singular"]:
            assert out["iterations"][i] > 1 and not np.array_equal(out["transform"][i], c["init"])
            assert out["n_correspondences"][i] > 1000
            continue
        want = RR.linearize(ref_map, c["scan"], c["init"], **kw)
        got = out["system0"][i]
        H = R.full(got)
        print(f"{name} {config}: iterations {out['iterations'][i]}, {int(got[27])} rows, |H n| / (||H|| |n|) = "
              f"{D.null_residual(H, c['null']):.3g}, moved {np.abs(out['transform'][i] - c['init']).max():.3g}")
        assert out["transform"][i].tobytes() == c["init"].tobytes(), (name, out["transform"][i])
        assert out["iterations"][i] == 1
        assert D.null_residual(H, c["null"]) <= NULL_BAR
        assert got[27] == want[27] == out["n_correspondences"][i] and want[27] >= min(len(c["scan"]), 5)
        assert close(got[:21], want[:21]) and close(got[21:27], want[21:27])
        assert abs(got[28] - want[28]) <= 1e-6 * want[28] and abs(got[29] - want[29]) <= 1e-6 * want[29]
        assert abs(out["cost"][i] - want[29]) <= 1e-6 * want[29]
        assert close(out["information"][i], R.full(want))
        assert abs(out["fitness"][i] - want[27] / len(c["scan"])) <= 1e-12
        ws = want[30] if config == "robust" else want[27]
        assert abs(out["rmse"][i] - np.sqrt(want[28] / ws)) <= 1e-6 * out["rmse"][i]
        if config == "robust":
            assert got[31] == want[31] == out["n_pairs"][i] and want[31] > want[27]
            assert abs(got[30] - want[30]) <= 1e-6 * want[30] and abs(out["weight_sum"][i] - want[30]) <= 1e-6 * want[30]
