"""Map localisation without a GPU: the restatement (tests/map_localize_restatement.py) against independent arithmetic, the
claims of the constructed inputs (tests/map_localize_cases.py) that tests/test_map_localize_gpu.py relies on, the host-side
refusals of ``MapLocalizer`` and the argument checks of the C ABI."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import kernel_budget as KB
import map_localize_cases as K
import map_localize_restatement as R
import map_restatement as M


@pytest.fixture(scope="module")
def lib():
    from neural_spectral_codec_amd import build, _lib
    build.build_hip()
    return _lib.lib()


# ---- the restatement against independent arithmetic -------------------------------------------------------------------

def test_moments_give_the_covariance_of_exact_rationals():
    pts, off, poses = K.exact_case(1, 3500)
    m = R.build_dist(pts, off, poses)
    assert m["rows_used"] == 3500 and m["info"][:, 0].max() >= 6
    assert M.face_distance(m["world"], m["used"], voxel_size=1.0) >= 1.0 / 64
    w = m["world"]                                                   # exact: lattice points under rot90 poses
    key_of = np.floor(w).astype(np.int64)
    for i in np.argsort(-m["info"][:, 0])[:20]:                       # the twenty fullest voxels
        k = (int(m["keys"][i]) & 0x1FFFFF, (int(m["keys"][i]) >> 21) & 0x1FFFFF, int(m["keys"][i]) >> 42)
        rows = np.all(key_of + (1 << 20) == np.array(k), 1)
        n = int(rows.sum())
        assert n == m["info"][i, 0]
        # q from the coordinates as exact rationals: (w - k) 2^16 - 2^15, an integer on this lattice
        q = [[Fraction(float(x)) * 65536 - (Fraction(kk - (1 << 20))) * 65536 - 32768 for x, kk in zip(row, k)]
             for row in w[rows]]
        assert all(v.denominator == 1 for row in q for v in row)
        q = np.array([[int(v) for v in row] for row in q], np.float64)
        assert m["moments"][i][:3].tolist() == q.sum(0).astype(np.int64).tolist()
        cov = np.cov(q.T, bias=True) * (1.0 / 65536) ** 2             # voxel_size 1
        got = R.sym3(m["voxels"][i:i + 1, 3:9])[0]
        assert np.abs(got - cov).max() <= 1e-12 * max(np.abs(cov).max(), 1e-300)
        mean = w[rows].mean(0)
        assert np.abs(m["voxels"][i, :3] - mean).max() <= 1e-14


@pytest.mark.parametrize("shape", ["full", "planar", "linear", "one point", "min_points - 1"])
def test_information_rule_against_eigh(shape):
    rng = np.random.default_rng(3)
    n = {"one point": 1, "min_points - 1": 5}.get(shape, 40)
    u = rng.uniform(0.1, 0.9, (n, 3))
    if shape == "planar":
        u[:, 2] = 0.5 + 0.2 * (u[:, 0] - 0.5)
    if shape == "linear":
        u[:, 1] = 0.5 + 0.3 * (u[:, 0] - 0.5)
        u[:, 2] = 0.5 - 0.1 * (u[:, 0] - 0.5)
    q = np.rint(u * 65536) - 32768
    pts = (q + 32768) / 65536 + np.array([2.0, -3.0, 1.0])            # exact: voxel (2, -3, 1) of 1 m
    m = R.build_dist(pts, np.array([0, n]), np.eye(4)[None], min_points=6, eigen_ratio=1e-2, sigma_floor=1e-3)
    assert m["voxels_found"] == 1
    rec = m["voxels"][0]
    assert rec[15] == (1.0 if n >= 6 else 0.0)
    C3 = np.cov(q.T, bias=True) / 65536.0 ** 2 if n > 1 else np.zeros((3, 3))
    lam, U = np.linalg.eigh(C3)
    rank = {"full": 3, "planar": 2, "linear": 1, "one point": 0, "min_points - 1": 3}[shape]
    assert int((lam > 1e-9).sum()) == rank, lam
    kept = np.maximum(np.maximum(lam, 1e-2 * lam.max()), 1e-6)
    O = R.sym3(rec[None, 9:15])[0]
    got = np.sort(1.0 / np.linalg.eigvalsh(O))
    assert np.abs(got - np.sort(kept)).max() <= 1e-9 * kept.max(), (got, kept)
    # Omega and C share eigenvectors where the rule keeps an eigenvalue as it is
    for i in range(3):
        if lam[i] == kept[i] and rank == 3:
            assert np.abs(O @ U[:, i] - U[:, i] / lam[i]).max() <= 1e-6 / lam[i]
    if shape == "one point":
        assert np.abs(O - np.eye(3) * 1e6).max() <= 1e-6


def _small_map_and_scan():
    s = K.scene()
    m = K.scene_reference()["map"]
    pts = s["scans"][:2000].astype(np.float64)
    return m, pts, s["init"][0]


def test_system_against_central_differences():
    """J^T O d is half the gradient of E along the update's six unknowns and J^T O J the Gauss-Newton matrix built from
    the central-difference Jacobian of the residuals, at fixed correspondences (rows are kept 1e-3 voxel from faces, the
    steps move them by less)."""
    m, pts, T = _small_map_and_scan()
    pts = pts[R.keep_off_faces(m, pts, T, 1e-3)]
    s = R.linearize(m, pts, T)
    _, place = R.lookup(m, pts, T)
    sel = place >= 0
    assert sel.sum() > 1000 and s[27] == sel.sum()
    rec = m["voxels"][place[sel]]
    O = R.sym3(rec[:, 9:15])

    def residuals(x):
        w = R.transform_rows(pts[sel], R.update(x) @ T)
        return w - rec[:, :3]

    def energy(x):
        d = residuals(x)
        return np.einsum("nr,nrs,ns->", d, O, d)
    h = 1e-6
    g = np.array([(energy(h * e) - energy(-h * e)) / (2 * h) for e in np.eye(6)]) / 2.0
    assert np.allclose(g, s[21:27], rtol=1e-6, atol=1e-6 * np.abs(s[21:27]).max())
    J = np.stack([(residuals(h * e) - residuals(-h * e)) / (2 * h) for e in np.eye(6)], 2)        # (n,3,6)
    H = np.einsum("nra,nrs,nsb->ab", J, O, J)
    assert np.allclose(H, R.full(s), rtol=1e-6, atol=1e-6 * np.abs(H).max())
    assert abs(energy(np.zeros(6)) - s[29]) <= 1e-12 * s[29]


# ---- the claims of the constructed inputs -----------------------------------------------------------------------------

@pytest.mark.parametrize("voxel", [0.5, 1.0])
def test_exact_case_is_exact(voxel):
    pts, off, poses = K.exact_case(1, 3500, voxel)
    m = R.build_dist(pts, off, poses, voxel_size=voxel)
    assert m["rows_used"] == 3500 and 200 < m["voxels_found"] < 3000 and m["info"][:, 0].max() > 3
    assert M.face_distance(m["world"], m["used"], voxel_size=voxel) >= 1.0 / 64
    assert np.array_equal(m["world"] * 64, np.rint(m["world"] * 64))              # on the lattice: no rounding anywhere
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_general_case_keeps_off_faces(dtype):
    sensor, off, poses = K.general_case(dtype)
    m = R.build_dist(sensor, off, poses)
    assert m["rows_used"] == len(sensor) and M.face_distance(m["world"], m["used"], voxel_size=1.0) >= K.FACE_MARGIN
    assert (m["voxels"][:, 15] == 1.0).sum() > 300


def test_ten_voxels_and_lookup_scan():
    pts, off, poses, vox = K.ten_voxels()
    m = R.build_dist(pts, off, poses, max_voxels=6)
    assert m["stats"][:2].tolist() == [10, 6] and m["capacity"] == 6
    assert m["info"][:, 0].tolist() == [8, 8, 8, 6, 5, 8, 8, 8, 8, 8]
    assert m["voxels"][:, 15].tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1, 1]
    scan, cat = K.lookup_scan(vox)
    _, place = R.lookup(m, scan, np.eye(4))
    assert set(cat) == {"usable", "unusable", "overflow", "absent", "outside", "not finite"}
    assert np.array_equal(place >= 0, cat == "usable") and (place >= 0).sum() == 35
    full = R.build_dist(pts, off, poses)                         # without the capacity the overflow voxels are found
    _, place = R.lookup(full, scan, np.eye(4))
    assert np.array_equal(place >= 0, (cat == "usable") | (cat == "overflow"))


def test_scene_and_its_bars():
    """The end-to-end scene: the restatement converges on it, and the two bars of the GPU test are computed here."""
    s, ref = K.scene(), K.scene_reference()
    m, r = ref["map"], ref["ref"]
    usable = int((m["voxels"][:, 15] == 1.0).sum())
    f0 = np.array([R.linearize(m, s["scans"][a:b], T)[27] / (b - a)
                   for a, b, T in zip(s["scan_offsets"][:-1], s["scan_offsets"][1:], s["init"])])
    print(f"scene: {usable} usable voxels of {m['voxels_found']}; fitness {f0.mean():.3f} -> {r['fitness'].mean():.3f}; "
          f"rounds {r['iterations'].tolist()}")
    print(f"restatement to truth: {ref['to_truth'][0] * 1e3:.2f} mm, {ref['to_truth'][1] * 1e3:.2f} mrad; "
          f"bar to truth (2x): {2e3 * ref['to_truth'][0]:.2f} mm, {2e3 * ref['to_truth'][1]:.2f} mrad")
    print(f"restatement under +-2^-24 m: {ref['change'][0]:.3g} m, {ref['change'][1]:.3g} rad; bar (10x): "
          f"{10 * ref['change'][0]:.3g} m, {10 * ref['change'][1]:.3g} rad")
    assert m["rows_used"] == 24000 and usable > 300
    assert (r["fitness"] > f0).all()
    assert ref["to_truth"][0] < 0.03 and ref["to_truth"][1] < 0.005          # the initial poses are 0.3 m and 3 degrees off
    assert ref["change"][0] > 0 and ref["change"][1] >= 0


def test_off_face_scans_leave_out_at_most_one_percent():
    s, m = K.scene(), K.scene_reference()["map"]
    pts, off, left = K.off_face_scans(m, s["scans"].astype(np.float64), s["scan_offsets"], s["init"])
    assert left <= 0.01 and len(off) == 9 and off[-1] == len(pts)
    for i in range(8):
        assert R.keep_off_faces(m, pts[off[i]:off[i + 1]], s["init"][i]).all()
    # and after the restatement's first update, for the one-update comparison
    one = R.register(m, pts, off, s["init"], max_iteration=1)
    pts1, off1, left1 = K.off_face_scans(m, pts, off, one["transform"])
    assert left1 <= 0.01


# ---- host-side refusals: nothing here touches a device ----------------------------------------------------------------

def test_constructor_refusals():
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import MapLocalizer
    for kw in (dict(voxel_size=0.0), dict(voxel_size=np.nan), dict(origin=(0, 0)), dict(origin=(0, np.inf, 0)),
               dict(max_voxels=-1), dict(min_points=0), dict(eigen_ratio=0.0), dict(eigen_ratio=1.5),
               dict(sigma_floor=0.0), dict(sigma_floor=np.nan), dict(max_iteration=-1), dict(relative_fitness=-1.0),
               dict(relative_rmse=np.nan), dict(device="cpu")):
        with pytest.raises(_lib.NscError):
            MapLocalizer(**kw)
    m = MapLocalizer()
    assert m.params.voxel_size == 1.0 and m.dist.min_points == 6 and m.reg.max_iteration == 30


def test_build_and_register_refusals():
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import MapLocalizer
    m = MapLocalizer()
    cloud = np.zeros((5, 3), np.float32)
    with pytest.raises(_lib.NscError):
        m.build([cloud, cloud], np.eye(4)[None], pose_ids=[0])                       # one id per cloud
    with pytest.raises(_lib.NscError):
        m.build([cloud], np.eye(4)[None], pose_ids=[1])                              # an id past the poses
    with pytest.raises(_lib.NscError):
        m.build([np.zeros((5, 2), np.float32)], np.eye(4)[None])
    with pytest.raises(_lib.NscError):
        m.build([cloud], np.zeros((3, 5)))
    with pytest.raises(_lib.NscError, match="build a map first"):
        m.register([cloud], np.eye(4)[None])
    import torch
    with pytest.raises(_lib.NscError):                                                # host tensors: no CPU fallback
        m.build_device(torch.zeros(5, 3), torch.tensor([0, 5]), torch.eye(4)[None])
    m.voxels = torch.zeros(0, 16)                                                     # as if a map were there
    with pytest.raises(_lib.NscError, match="one .* pose per scan"):
        m.register([cloud, cloud], np.eye(4)[None])
    with pytest.raises(_lib.NscError):
        m.register([np.zeros((5, 5), np.float32)], np.eye(4)[None])


# ---- the C ABI without a device ---------------------------------------------------------------------------------------

def test_abi_defaults_workspace_and_guards(lib):
    from neural_spectral_codec_amd import _lib
    d, r, g = _lib.MapDistParams(), _lib.MapRegisterParams(), _lib.MapParams()
    lib.nsc_map_dist_default_params(C.byref(d))
    lib.nsc_map_register_default_params(C.byref(r))
    lib.nsc_map_default_params(C.byref(g))
    assert (d.min_points, d.eigen_ratio, d.sigma_floor) == (6, 1e-2, 1e-3)
    assert (r.max_iteration, r.relative_fitness, r.relative_rmse) == (30, 1e-6, 1e-6)
    assert g.voxel_size == 0.5                                          # the map's own default stays
    assert lib.nsc_abi_version() == 4
    # the build's table has 128-byte slots, the rest of the layout is nsc_map_build's
    for rows, vox in ((0, 0), (1, 1), (5000, 100), (100000, 4096)):
        assert lib.nsc_map_dist_workspace_bytes(rows, vox) - lib.nsc_map_workspace_bytes(rows, vox) == \
            (2 * vox * 128 + 255) // 256 * 256 - (2 * vox * 64 + 255) // 256 * 256
    assert lib.nsc_map_dist_workspace_bytes(-1, 1) == 0 and lib.nsc_map_dist_workspace_bytes(1, _lib.MAP_MAX_VOXELS + 1) == 0
    # registration: per scan 64 slabs of 30 float64, a 32-byte state and a count, each region rounded up to 256 bytes
    up = lambda v: (v + 255) // 256 * 256
    for n in (0, 1, 8, 65535):
        assert lib.nsc_map_register_workspace_bytes(n) == up(n * 64 * 30 * 8) + up(n * 32) + up(n * 8)
    assert lib.nsc_map_register_workspace_bytes(-1) == 0
    assert _lib.MAP_REGISTER_BLOCKS == 64 and _lib.MAP_REGISTER_SYSTEM == 30
    # more than 65 535 scans: refused before any launch, whatever else is passed
    none = [None] * 8
    assert lib.nsc_map_register(None, 0, 3, None, _lib.MAP_REGISTER_MAX_SCANS + 1, 0, None, None, 0, None, None,
                                *none, 0, None) == -2
    assert lib.nsc_map_register(None, 0, 3, None, _lib.MAP_REGISTER_MAX_SCANS + 1, 0, None, None, 0, C.byref(g),
                                C.byref(r), *none, 0, None) == -2
    assert lib.nsc_map_register(None, 0, 3, None, 0, 0, None, None, 0, C.byref(g), C.byref(r), *none, 0, None) == 0
    assert lib.nsc_map_register(None, 0, 3, None, 1, 0, None, None, 0, C.byref(g), C.byref(r), *none, 0, None) == -1
    assert lib.nsc_map_register(None, 2, 3, None, 0, 0, None, None, 0, C.byref(g), C.byref(r), *none, 0, None) == -1
    assert lib.nsc_map_register(None, 1, 4, None, 0, 0, None, None, 0, C.byref(g), C.byref(r), *none, 0, None) == -1
    r.max_iteration = -1
    assert lib.nsc_map_register(None, 0, 3, None, 0, 0, None, None, 0, C.byref(g), C.byref(r), *none, 0, None) == -1
    # the build: nsc_map_build's refusals, and the new parameters
    stats = (C.c_int64 * 7)()
    off = (C.c_int64 * 1)(0)
    args = lambda dist, vox=0: (None, 0, 3, off, 0, 0, None, 0, None, C.byref(g), dist, vox, None, None, None, None, None,
                                stats, None, 0, None)
    assert lib.nsc_map_build_dist(*args(None)) == -1
    assert lib.nsc_map_build_dist(*args(C.byref(d), 4)) == -1           # outputs missing
    assert lib.nsc_map_build_dist(*args(C.byref(d), _lib.MAP_MAX_VOXELS + 1)) in (-1, -2)
    for name, bad in (("min_points", 0), ("eigen_ratio", 0.0), ("eigen_ratio", 2.0), ("sigma_floor", 0.0),
                      ("sigma_floor", float("inf"))):
        e = _lib.MapDistParams(min_points=6, reserved=0, eigen_ratio=1e-2, sigma_floor=1e-3)
        setattr(e, name, bad)
        assert lib.nsc_map_build_dist(*args(C.byref(e))) == -1, name


def test_linearize_keeps_its_sums_in_registers(lib, tmp_path):
    """loc_linearize_kernel adds 30 float64 terms per row into per-lane accumulators: they must stay in registers (no
    scratch) and leave room for four waves per SIMD (at most 128 VGPRs), read from the gfx950 code object."""
    if not KB.binutils():
        pytest.skip("llvm binutils of the ROCm image not found")
    found = KB.kernels("loc_linearize_kernel")
    assert len(found) == 2, sorted(found)                        # float32 and float64 rows
    for k, (vg, sc) in found.items():
        assert vg <= 128 and sc == 0, f"{k}: {vg} VGPRs, {sc} B scratch"
