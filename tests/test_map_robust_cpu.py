"""Robust weights and face-neighbour voxels in map localisation, without a GPU: the C ABI's and ``MapLocalizer``'s
refusals, the restatement (tests/map_robust_restatement.py) against map_localize_restatement and against central
differences, and the claims of the constructed inputs (tests/map_robust_cases.py) that tests/test_map_robust_gpu.py relies
on."""
import ctypes as C

import numpy as np
import pytest

import kernel_budget as KB
import map_localize_cases as K
import map_localize_restatement as R
import map_robust_cases as KR
import map_robust_restatement as RR


@pytest.fixture(scope="module")
def lib():
    from neural_spectral_codec_amd import build, _lib
    build.build_hip()
    return _lib.lib()


# ---- the C ABI without a device ---------------------------------------------------------------------------------------

def test_abi_defaults_workspace_and_refusals(lib):
    from neural_spectral_codec_amd import _lib
    p = _lib.MapRobustParams(kernel=9, neighbours=9, scale=9.0)
    lib.nsc_map_robust_default_params(C.byref(p))
    assert (p.kernel, p.neighbours, p.scale) == (0, 1, 0.0)
    assert _lib.MAP_KERNELS == _lib.POSEGRAPH_KERNELS and _lib.MAP_REGISTER_ROBUST_SYSTEM == 32
    # per scan 64 slabs of 32 float64, a 32-byte state and a count, each region rounded up to 256 bytes
    up = lambda v: (v + 255) // 256 * 256
    sizes = [lib.nsc_map_register_robust_workspace_bytes(n) for n in (0, 1, 2, 8, 1000, 65535)]
    assert sizes == sorted(sizes) and sizes[1] > 0
    for n, got in zip((0, 1, 2, 8, 1000, 65535), sizes):
        assert got == up(n * 64 * 32 * 8) + up(n * 32) + up(n * 8)
        assert got >= lib.nsc_map_register_workspace_bytes(n)
    assert lib.nsc_map_register_robust_workspace_bytes(-1) == 0
    g, r = _lib.MapParams(), _lib.MapRegisterParams()
    lib.nsc_map_default_params(C.byref(g))
    lib.nsc_map_register_default_params(C.byref(r))
    none = [None] * 8

    def call(rob, n_scans=0):
        return lib.nsc_map_register_robust(None, 0, 3, None, n_scans, 0, None, None, 0, C.byref(g), C.byref(r), rob,
                                           *none, None, 0, None)
    ok = lambda **kw: C.byref(_lib.MapRobustParams(**{**dict(kernel=0, neighbours=1, scale=0.0), **kw}))
    assert call(ok()) == 0 and call(ok(neighbours=7)) == 0 and call(ok(kernel=3, scale=2.0, neighbours=7)) == 0
    assert call(ok(scale=float("nan"))) == 0                            # without a kernel the width is not read
    assert call(None) == -1
    for bad in (dict(kernel=-1), dict(kernel=4, scale=1.0), dict(neighbours=0), dict(neighbours=6), dict(neighbours=27),
                dict(kernel=1), dict(kernel=2, scale=-1.0), dict(kernel=3, scale=float("inf")),
                dict(kernel=1, scale=float("nan"))):
        assert call(ok(**bad)) == -1, bad
        assert call(ok(**bad), _lib.MAP_REGISTER_MAX_SCANS + 1) == -1, bad       # before every other refusal
    # then nsc_map_register's own refusals
    assert call(ok(kernel=2, scale=3.0), _lib.MAP_REGISTER_MAX_SCANS + 1) == -2
    assert call(ok(kernel=2, scale=3.0), 1) == -1


def test_localizer_refusals():
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import MapLocalizer
    for kw in (dict(kernel="tukey"), dict(kernel=2), dict(neighbours=0), dict(neighbours=27), dict(neighbours=7.5),
               dict(kernel="cauchy"), dict(kernel="huber", robust_scale=0.0), dict(kernel="huber", robust_scale=-1.0),
               dict(kernel="geman_mcclure", robust_scale=np.inf), dict(kernel="cauchy", robust_scale=np.nan),
               dict(robust_scale=2.0)):
        with pytest.raises(_lib.NscError):
            MapLocalizer(**kw)
    m = MapLocalizer()
    assert (m.robust.kernel, m.robust.neighbours, m.robust.scale) == (0, 1, 0.0)
    m = MapLocalizer(kernel="geman_mcclure", robust_scale=2.0, neighbours=7)
    assert (m.robust.kernel, m.robust.neighbours, m.robust.scale) == (3, 7, 2.0)
    assert MapLocalizer(neighbours=7).robust.neighbours == 7


def test_new_linearize_kernels_use_no_scratch(lib, tmp_path):
    """the six instantiations of loc_linearize_robust_kernel (float32 and float64 rows x {kernel over one voxel, seven
    voxels without a kernel, kernel over seven voxels}) keep their 32 sums in registers; read from the gfx950 code object"""
    assert KB.binutils(), f"no llvm binutils in {KB.LLVM}"
    found = KB.kernels("loc_linearize_robust_kernel")
    assert len(found) == 6, sorted(found)
    for k, (vg, sc) in found.items():
        print(f"{k}: {vg} VGPRs, {sc} B scratch")
        assert sc == 0 and vg <= 256, f"{k}: {vg} VGPRs, {sc} B scratch"        # 256: two waves per SIMD still fit


# ---- the restatement --------------------------------------------------------------------------------------------------

def test_restatement_without_options_is_the_plain_restatement():
    s, ref = K.scene(), K.scene_reference()
    got = RR.register(ref["map"], s["scans"], s["scan_offsets"], s["init"])
    for k, want in ref["ref"].items():
        a = got[k][:, :30] if k == "system0" else got[k]
        assert np.array_equal(a, want), (k, np.abs(a - want).max())
    assert np.array_equal(got["weight_sum"], got["n_pairs"]) and np.array_equal(got["n_pairs"], got["n_correspondences"])
    assert np.array_equal(got["system0"][:, 30], got["system0"][:, 27])
    assert np.array_equal(got["system0"][:, 31], got["system0"][:, 27])


def test_kernel_weights_are_the_derivative_of_rho():
    s = np.concatenate([[0.0, -1.0], np.geomspace(1e-3, 1e4, 200)])
    for kernel in RR.KERNELS[1:]:
        for c in (0.5, 2.0, 3.0):
            rho, w = RR.rho_w(kernel, c, s)
            assert (rho[:2] == s[:2]).all() and (w[:2] == 1.0).all()
            h = 1e-6 * s[2:]
            num = (RR.rho_w(kernel, c, s[2:] + h)[0] - RR.rho_w(kernel, c, s[2:] - h)[0]) / (2 * h)
            assert np.allclose(num, w[2:], rtol=1e-6, atol=1e-9)
            assert (w[2:] <= 1.0).all() and (w[2:] > 0.0).all() and (rho[2:] <= s[2:] * (1 + 1e-15)).all()
    rho, w = RR.rho_w(None, None, s)
    assert np.array_equal(rho, s) and (w == 1.0).all()
    assert RR.rho_w("huber", 2.0, np.array([4.0, 9.0]))[1].tolist() == [1.0, 2.0 / 3.0]
    assert RR.rho_w("cauchy", 2.0, np.array([4.0]))[1].tolist() == [0.5]
    assert RR.rho_w("geman_mcclure", 2.0, np.array([4.0]))[1].tolist() == [0.25]


@pytest.mark.parametrize("neighbours", [1, 7])
@pytest.mark.parametrize("kernel", ["huber", "cauchy", "geman_mcclure"])
def test_system_against_central_differences(kernel, neighbours):
    """sum w J^T O d is half the gradient of sum rho(s) along the update's six unknowns, and sum w J^T O J the
    Gauss-Newton matrix of the residuals weighted by w, built from the central-difference Jacobian of the residuals, at
    fixed pairs (rows are kept 1e-3 voxel from faces, the steps move them by less): test_map_localize_cpu's method and
    bars"""
    s, m = K.scene(), K.scene_reference()["map"]
    pts, T, c = s["scans"][:2000].astype(np.float64), s["init"][0], 2.0
    pts = pts[R.keep_off_faces(m, pts, T, 1e-3)]
    sums = RR.linearize(m, pts, T, kernel, c, neighbours)
    _, row, place = RR.pairs(m, pts, T, neighbours)
    assert len(row) > 1000 and sums[31] == len(row) and sums[27] == len(np.unique(row))
    assert (len(row) > sums[27]) == (neighbours == 7)
    rec = m["voxels"][place]
    O = R.sym3(rec[:, 9:15])

    def residuals(x):
        return R.transform_rows(pts, R.update(x) @ T)[row] - rec[:, :3]

    def chi2(x):
        d = residuals(x)
        return np.einsum("nr,nrs,ns->n", d, O, d)

    def energy(x):
        return RR.rho_w(kernel, c, chi2(x))[0].sum()
    wt = RR.rho_w(kernel, c, chi2(np.zeros(6)))[1]
    assert wt.min() < 0.5 and wt.max() > 0.9                              # the kernel is at work on this scan
    h = 1e-6
    g = np.array([(energy(h * e) - energy(-h * e)) / (2 * h) for e in np.eye(6)]) / 2.0
    assert np.allclose(g, sums[21:27], rtol=1e-6, atol=1e-6 * np.abs(sums[21:27]).max())
    J = np.stack([(residuals(h * e) - residuals(-h * e)) / (2 * h) for e in np.eye(6)], 2)        # (n,3,6)
    H = np.einsum("nra,nrs,nsb->ab", J, O * wt[:, None, None], J)
    assert np.allclose(H, R.full(sums), rtol=1e-6, atol=1e-6 * np.abs(H).max())
    assert abs(energy(np.zeros(6)) - sums[29]) <= 1e-12 * sums[29]
    assert abs(wt.sum() - sums[30]) <= 1e-12 * sums[30]


# ---- the claims of the constructed inputs -----------------------------------------------------------------------------

def test_clutter_bends_the_quadratic_pose_and_not_the_robust_one():
    """(a): the quadratic restatement's worst translation error to the truth is at least 5 x that of Geman-McClure c = 2
    over one voxel; both bars of the GPU test are computed here"""
    s = K.scene()
    scans = KR.clutter_scans()
    moved = (scans != s["scans"]).any(1)
    assert scans.dtype == np.float32 and all(moved[a:b].sum() == 400 for a, b in zip(s["scan_offsets"][:-1],
                                                                                      s["scan_offsets"][1:]))
    clean = K.scene_reference()["to_truth"]
    quad, rob = KR.clutter_reference(False), KR.clutter_reference(True)
    for name, r in (("quadratic", quad), ("geman_mcclure c=2", rob)):
        print(f"{name}: to truth {r['to_truth'][:, 0].max() * 1e3:.2f} mm, {r['to_truth'][:, 1].max() * 1e3:.3f} mrad; "
              f"rounds {r['ref']['iterations'].tolist()}; under +-2^-24 m: {r['change'][0]:.3g} m, {r['change'][1]:.3g} rad "
              f"over {int(r['finished'].sum())} finished scans")
    print(f"clean scans, quadratic: {clean[0] * 1e3:.2f} mm, {clean[1] * 1e3:.3f} mrad")
    assert quad["to_truth"][:, 0].max() >= 5.0 * rob["to_truth"][:, 0].max()
    assert rob["to_truth"][:, 0].max() < 0.01
    assert quad["finished"].sum() >= 7 and rob["finished"].sum() >= 7
    assert rob["change"][0] > 0 and quad["change"][0] > 0


def test_wide_start_needs_neighbours():
    """(b): at 0.5 m voxels and 1.0 m off, round-0 fitness is below 0.2 over one voxel and above 0.5 over seven, and Cauchy
    c = 3 over seven voxels ends all eight scans within 1 cm of the truth"""
    s, ws = K.scene(), KR.wide_scene()
    off = s["scan_offsets"]
    off_by = KR.errors(ws["init"], s["truth"])
    assert (off_by[:, 0] > 0.9).all() and (off_by[:, 0] < 1.2).all()         # 1.0 m, and what 3 degrees move the origin by
    f = {nb: np.array([RR.linearize(ws["map"], s["scans"][a:b], T, neighbours=nb)[27] / (b - a)
                       for a, b, T in zip(off[:-1], off[1:], ws["init"])]) for nb in (1, 7)}
    r = KR.wide_reference()
    print(f"round-0 fitness over one voxel {f[1].min():.3f} .. {f[1].max():.3f}, over seven {f[7].min():.3f} .. "
          f"{f[7].max():.3f}; cauchy c=3 over seven: to truth {r['to_truth'][:, 0].max() * 1e3:.2f} mm, rounds "
          f"{r['ref']['iterations'].tolist()}; under +-2^-24 m: {r['change'][0]:.3g} m, {r['change'][1]:.3g} rad over "
          f"{int(r['finished'].sum())} finished scans")
    assert (f[1] < 0.2).all() and (f[7] > 0.5).all()
    assert (r["to_truth"][:, 0] < 0.01).all()
    assert r["finished"].sum() >= 7 and r["change"][0] > 0
    assert (r["ref"]["n_pairs"] >= r["ref"]["n_correspondences"]).all() and (r["ref"]["fitness"] <= 1.0).all()


def test_off_face_scans_leave_out_at_most_one_percent():
    """(c)"""
    s, m = K.scene(), K.scene_reference()["map"]
    pts, off, left = KR.off_face()
    print(f"off-face scans leave out {left:.4%} of the rows")
    assert left <= 0.01 and off[-1] == len(pts)
    for i in range(8):
        assert R.keep_off_faces(m, pts[off[i]:off[i + 1]], s["init"][i], K.FACE_MARGIN).all()


def test_neighbour_scan_has_every_kind_of_row():
    pts, off, poses, vox = K.ten_voxels()
    m = R.build_dist(pts, off, poses, max_voxels=6)
    scan = KR.neighbour_scan(vox)
    I = np.eye(4)
    _, row1, _ = RR.pairs(m, scan, I, 1)
    _, row7, place7 = RR.pairs(m, scan, I, 7)
    own = np.isin(np.arange(len(scan)), row1)
    any7 = np.isin(np.arange(len(scan)), row7)
    assert own.sum() == 35 and not (own & ~any7).any()
    assert (any7 & ~own).sum() >= 40            # rows in an absent own voxel with a usable neighbour: pairs only over seven
    assert (~any7).sum() >= 60                  # next to the unusable voxel, next to voxels past the capacity, absent, ...
    assert set(place7.tolist()) == {0, 1, 2, 3, 5}
    assert not np.isfinite(scan).all() and (np.abs(scan[np.isfinite(scan).all(1)]) > 1e6).any()


@pytest.mark.parametrize("shift", [0, 1 << 20, -(1 << 20)])
def test_edge_map_sits_on_the_grids_first_and_last_coordinate(shift):
    pts, off, poses, origin, scan = KR.edge_map(shift)
    m = R.build_dist(pts, off, poses, origin=origin)
    keys = sorted(int(v[0]) | (int(v[1]) << 21) | (int(v[2]) << 42) for v in KR.EDGE_VOXELS)
    assert sorted(m["keys"].tolist()) == keys and (m["voxels"][:, 15] == 1.0).all()
    a, b, c, d = (int(v[0]) | (int(v[1]) << 21) | (int(v[2]) << 42) for v in KR.EDGE_VOXELS)
    assert a - 1 == b and c + 1 == d            # what a borrowing or carrying key would find
    I = np.eye(4)
    _, row1, _ = RR.pairs(m, scan, I, 1)
    _, row7, _ = RR.pairs(m, scan, I, 7)
    # three rows in each voxel (own), three one step inside (the map voxel is their x neighbour), three outside the grid
    assert len(row1) == 12 and len(row7) == 24 and len(np.unique(row7)) == 24
