"""Map localisation on the MI355X: MapLocalizer / nsc_map_build_dist / nsc_map_register against the restatement
(tests/map_localize_restatement.py) on the constructed inputs of tests/map_localize_cases.py, whose claims
tests/test_map_localize_cpu.py asserts.

Exact comparisons: keys, info and stats against GlobalMap on the same input; the integer moments against the restatement
on input that is exact in any evaluation order; correspondence counts.

Bars that are not exact:
  mean      a fused and an unfused R p + t can differ by one unit of q = 2^-16 voxel in a row, so a voxel's mean by at most
            one unit, plus the rounding of a handful of float64 operations on coordinates below 16 m (2^-49 m each):
            MEAN_BAR = 2^-16 voxel + 1e-12 m
  C, Omega  worst relative error in the Frobenius norm measured on the general-pose inputs (test_build_general_poses)
            against the exact-rational restatement, times 10 because Omega amplifies by up to 1 / eigen_ratio
            (DESIGN 4.13): C 6.08e-16 -> C_BAR 6.1e-15, Omega 2.56e-14 -> OMEGA_BAR 2.6e-13
  systems   the project's 1e-6 relative bar for system terms (tests/test_gicp_paths_gpu.py check_system)
  end to end  to the truth twice the restatement's own worst error, to the restatement ten times what +-2^-24 m on every
            scan coordinate changes in the restatement's result; both computed by map_localize_cases.scene_reference
"""
import numpy as np
import pytest
import torch

import map_localize_cases as K
import map_localize_restatement as R

pytestmark = pytest.mark.gpu

C_BAR, OMEGA_BAR = 6.1e-15, 2.6e-13      # 10 x the measured figures


def _lib():
    from neural_spectral_codec_amd import _lib
    return _lib


def localizer(**kw):
    from neural_spectral_codec_amd.retrieval import MapLocalizer
    return MapLocalizer(**kw)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def built(points, off, poses, ids=None, **kw):
    """-> (the localizer, build_device's full buffers on the host, moments included)"""
    m = localizer(**kw)
    return m, host(m.build_device(dev(points), dev(off), dev(poses), ids, moments=True))


def moments_of(ref, n):
    return np.array(ref["moments"][:n].tolist(), np.int64).reshape(n, 9)


def assert_build_exact(out, ref, what=""):
    """stats, and the written voxels' info, keys and moments, equal the restatement's bit for bit; usable flags too"""
    assert out["stats"].tolist() == ref["stats"].tolist(), (what, out["stats"], ref["stats"])
    n = int(ref["stats"][1])
    assert np.array_equal(out["info"][:n], ref["info"][:n]) and np.array_equal(out["keys"][:n], ref["keys"][:n]), what
    assert np.array_equal(out["moments"][:n], moments_of(ref, n)), what
    assert np.array_equal(out["voxels"][:n, 15], ref["voxels"][:n, 15]), what


def frobenius_error(got6, ref6):
    a, b = R.sym3(got6), R.sym3(ref6)
    return np.linalg.norm(a - b, axis=(1, 2)) / np.maximum(np.linalg.norm(b, axis=(1, 2)), 1e-300)


def assert_records_close(out, ref, voxel, what=""):
    n = int(ref["stats"][1])
    got, want = out["voxels"][:n], ref["voxels"][:n]
    if n == 0:
        return
    mean = np.abs(got[:, :3] - want[:, :3]).max()
    many = ref["info"][:n, 0] >= 2                                # a voxel of one row has C = 0: compared absolutely
    ec = frobenius_error(got[many, 3:9], want[many, 3:9]).max() if many.any() else 0.0
    eo = frobenius_error(got[:, 9:15], want[:, 9:15]).max()
    print(f"{what}: {n} voxels, mean error {mean:.3g} m (bar {2.0 ** -16 * voxel + 1e-12:.3g}), C {ec:.3g} "
          f"(bar {C_BAR:.3g}), Omega {eo:.3g} (bar {OMEGA_BAR:.3g})")
    assert mean <= 2.0 ** -16 * voxel + 1e-12, what
    assert np.abs(got[~many, 3:9]).max(initial=0.0) == 0.0, what
    assert ec <= C_BAR and eo <= OMEGA_BAR, what


def index_of(out):
    """the index as {key: place or -1} and the number of its occupied slots"""
    idx = out["index"].view(np.uint64)
    used = idx[:, 0] != 0
    return {int(k) - 1: (-1 if p == np.uint64(2 ** 64 - 1) else int(p)) for k, p in idx[used]}, int(used.sum())


# ---- 1. the build: exact comparisons ----------------------------------------------------------------------------------

@pytest.mark.parametrize("voxel", [0.5, 1.0])
def test_build_equals_global_map_and_restatement_on_exact_input(voxel):
    from neural_spectral_codec_amd.retrieval import GlobalMap
    pts, off, poses = K.exact_case(1, 3500, voxel)
    ref = R.build_dist(pts, off, poses, voxel_size=voxel)
    rows4 = np.concatenate([pts, np.full((len(pts), 1), np.nan)], 1).astype(np.float32)      # the 4th column is not read
    for rows, what in ((pts.astype(np.float32), "float32 x 3"), (rows4, "float32 x 4"), (pts, "float64")):
        m, out = built(rows, off, poses, voxel_size=voxel)
        g = host(GlobalMap(voxel_size=voxel).build_device(dev(rows), dev(off), dev(poses)))
        n = int(g["stats"][1])
        assert out["stats"].tobytes() == g["stats"].tobytes(), what
        assert out["keys"][:n].tobytes() == g["keys"][:n].tobytes() and out["info"][:n].tobytes() == g["info"][:n].tobytes()
        assert_build_exact(out, ref, what)
        assert_records_close(out, ref, voxel, what)
        places, occupied = index_of(out)
        assert occupied == n and places == {int(k): i for i, k in enumerate(ref["keys"].tolist())}, what


# ---- 2. the build: general poses --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_build_general_poses(dtype):
    sensor, off, poses = K.general_case(dtype)
    ref = R.build_dist(sensor, off, poses)
    m, out = built(sensor, off, poses)
    n = ref["voxels_found"]
    assert out["stats"].tolist() == ref["stats"].tolist()
    assert np.array_equal(out["keys"][:n], ref["keys"]) and np.array_equal(out["info"][:n], ref["info"])
    flips = np.abs(out["moments"][:n, :3] - moments_of(ref, n)[:, :3]).max()
    print(f"{np.dtype(dtype).name}: largest difference of a sum of q: {flips} units")
    assert flips <= ref["info"][:, 0].max()
    assert np.array_equal(out["voxels"][:n, 15], ref["voxels"][:, 15])
    assert_records_close(out, ref, 1.0, np.dtype(dtype).name)


# ---- 3. the build: sizes ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["0", "1", "64", "65", "T-1", "T", "T+1"])
def test_build_small_sizes_and_empty_clouds(which):
    T = _lib().MAP_TILE_ROWS
    n = {"0": 0, "1": 1, "64": 64, "65": 65, "T-1": T - 1, "T": T, "T+1": T + 1}[which]
    pts, off, poses = K.exact_case(40 + n % 7, n)
    ref = R.build_dist(pts, off, poses)
    assert ref["rows_used"] == n
    for rows in (pts.astype(np.float32), pts):
        m, out = built(rows, off, poses)
        assert_build_exact(out, ref, which)
        assert_records_close(out, ref, 1.0, which)
        places, occupied = index_of(out)
        assert occupied == ref["voxels_found"] and all(places[int(k)] == i for i, k in enumerate(ref["keys"].tolist()))


def test_min_points_boundary():
    pts, off, poses, _ = K.ten_voxels()
    m, out = built(pts, off, poses)
    assert out["info"][:10, 0].tolist() == [8, 8, 8, 6, 5, 8, 8, 8, 8, 8]
    assert out["voxels"][:10, 15].tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1, 1]
    assert_build_exact(out, R.build_dist(pts, off, poses))


@pytest.mark.parametrize("max_voxels", [1, 2, 3])
def test_capacity_table_short(max_voxels):
    """Ten voxels, 2 max_voxels slots: probes wrap, rows go unplaced, which voxels get in depends on arrival.  What is
    written are voxels of the complete map with all of their rows, in its order; the index holds every voxel of the
    table, those past the outputs with place ~0; nothing is written outside the buffers."""
    pts, off, poses, _ = K.ten_voxels()
    ref = R.build_dist(pts, off, poses)
    M, guard, sentinel = max_voxels, 8, -77
    shapes = dict(voxels=(M, 16), index=(2 * M, 2), info=(M, 4), keys=(M,), moments=(M, 9), stats=(7,))
    big = {k: torch.full((s[0] + guard,) + s[1:], sentinel, dtype=torch.float64 if k == "voxels" else torch.int64,
                         device="cuda") for k, s in shapes.items()}
    views = {k: big[k][:shapes[k][0]] for k in shapes}
    out = host(localizer(max_voxels=M).build_device(dev(pts), dev(off), dev(poses), out=views))
    found, written, used, _, _, _, unplaced = out["stats"].tolist()
    assert unplaced > 0 and found == 2 * M and written == M and used + unplaced == len(pts)
    for k, s in shapes.items():
        assert bool((big[k][s[0]:] == sentinel).all()), k
    place = {int(k): i for i, k in enumerate(ref["keys"].tolist())}
    at = [place[int(k)] for k in out["keys"][:written]]
    assert at == sorted(at)
    assert np.array_equal(out["info"][:written], ref["info"][at])
    assert np.array_equal(out["moments"][:written], moments_of(ref, 10)[at])
    places, occupied = index_of(out)
    assert occupied == found and set(places) <= set(place)
    assert sorted(p for p in places.values() if p >= 0) == list(range(written))
    assert all(int(out["keys"][p]) == k for k, p in places.items() if p >= 0)
    assert sum(p < 0 for p in places.values()) == found - written


# ---- 4. the lookup ----------------------------------------------------------------------------------------------------

def test_lookup_counts_every_kind_of_row():
    pts, off, poses, vox = K.ten_voxels()
    ref = R.build_dist(pts, off, poses, max_voxels=6)
    scan, cat = K.lookup_scan(vox)
    m = localizer(max_voxels=6, max_iteration=0)
    m.build_device(dev(pts), dev(off), dev(poses))
    per_kind = {c: scan[cat == c] for c in sorted(set(cat))}
    scans = [scan] + list(per_kind.values())
    out = host(m.register(scans, np.tile(np.eye(4), (len(scans), 1, 1))))
    want = [int((R.lookup(ref, s, np.eye(4))[1] >= 0).sum()) for s in scans]
    assert out["n_correspondences"].tolist() == want and want[0] == 35
    assert dict(zip(per_kind, want[1:])) == {"absent": 0, "not finite": 0, "outside": 0, "overflow": 0, "unusable": 0,
                                             "usable": 35}
    assert out["iterations"].tolist() == [0] * len(scans)
    assert np.array_equal(out["transform"], np.tile(np.eye(4), (len(scans), 1, 1)))
    assert out["fitness"][0] == 35 / len(scan)


# ---- 5. one linearisation, one update ---------------------------------------------------------------------------------

def close(got, ref):
    return np.allclose(got, ref, rtol=1e-6, atol=1e-6 * max(np.abs(ref).max(), 1e-300))


@pytest.fixture(scope="module")
def scene_map():
    s = K.scene()
    m = localizer(voxel_size=1.0)
    res = m.build(list(np.split(s["points"], 6)), s["poses"])
    assert res["complete"] and res["rows_used"] == 24000
    return m


def test_scene_map_equals_restatement(scene_map):
    ref = K.scene_reference()["map"]
    n = ref["voxels_found"]
    assert np.array_equal(scene_map.keys[:n].cpu().numpy(), ref["keys"])
    assert np.array_equal(scene_map.info[:n].cpu().numpy(), ref["info"])
    out = dict(voxels=scene_map.voxels.cpu().numpy())
    assert np.array_equal(out["voxels"][:n, 15], ref["voxels"][:, 15])
    assert_records_close(out, ref, 1.0, "scene")


def test_system0_against_restatement(scene_map):
    s, ref = K.scene(), K.scene_reference()["map"]
    pts, off, _ = K.off_face_scans(ref, s["scans"].astype(np.float64), s["scan_offsets"], s["init"])
    scene_map.reg.max_iteration = 0
    try:
        out = host(scene_map.register((dev(pts), dev(off)), s["init"], system0=True))
    finally:
        scene_map.reg.max_iteration = 30
    for i in range(8):
        want = R.linearize(ref, pts[off[i]:off[i + 1]], s["init"][i])
        got = out["system0"][i]
        assert got[27] == want[27] == out["n_correspondences"][i] and want[27] > 1000
        assert close(got[:21], want[:21]) and close(got[21:27], want[21:27])
        assert abs(got[28] - want[28]) <= 1e-6 * want[28] and abs(got[29] - want[29]) <= 1e-6 * want[29]
        assert abs(out["cost"][i] - want[29]) <= 1e-6 * want[29]
        assert close(out["information"][i], R.full(want))
        assert abs(out["fitness"][i] - want[27] / (off[i + 1] - off[i])) <= 1e-12
        assert abs(out["rmse"][i] - np.sqrt(want[28] / want[27])) <= 1e-6 * out["rmse"][i]
        assert np.array_equal(out["transform"][i], s["init"][i])


def test_one_update_against_restatement(scene_map):
    s, ref = K.scene(), K.scene_reference()["map"]
    pts, off, _ = K.off_face_scans(ref, s["scans"].astype(np.float64), s["scan_offsets"], s["init"])
    want = R.register(ref, pts, off, s["init"], max_iteration=1)
    pts, off, _ = K.off_face_scans(ref, pts, off, want["transform"])         # off the faces after the update as well
    want = R.register(ref, pts, off, s["init"], max_iteration=1)
    scene_map.reg.max_iteration = 1
    try:
        out = host(scene_map.register((dev(pts), dev(off)), s["init"]))
    finally:
        scene_map.reg.max_iteration = 30
    assert out["iterations"].tolist() == [1] * 8
    assert out["n_correspondences"].tolist() == want["n_correspondences"].tolist()
    for i in range(8):
        assert close(out["transform"][i], want["transform"][i])
        assert not np.array_equal(out["transform"][i], s["init"][i])
        assert abs(out["cost"][i] - want["cost"][i]) <= 1e-6 * want["cost"][i]


# ---- 6. end to end ----------------------------------------------------------------------------------------------------

def test_scans_find_their_place_in_the_map(scene_map):
    s, ref = K.scene(), K.scene_reference()
    scene_map.reg.max_iteration = 0
    try:
        before = host(scene_map.register((dev(s["scans"]), dev(s["scan_offsets"])), s["init"]))
    finally:
        scene_map.reg.max_iteration = 30
    out = host(scene_map.register(list(np.split(s["scans"], 8)), s["init"]))
    assert (out["fitness"] > before["fitness"]).all()
    to_truth = np.array([K.pose_error(a, b) for a, b in zip(out["transform"], s["truth"])])
    to_ref = np.array([K.pose_error(a, b) for a, b in zip(out["transform"], ref["ref"]["transform"])])
    print(f"fitness {before['fitness'].mean():.3f} -> {out['fitness'].mean():.3f}, rounds {out['iterations'].tolist()}")
    print(f"to truth {to_truth[:, 0].max() * 1e3:.3f} mm, {to_truth[:, 1].max() * 1e3:.3f} mrad "
          f"(bars {2e3 * ref['to_truth'][0]:.3f}, {2e3 * ref['to_truth'][1]:.3f}); to the restatement "
          f"{to_ref[:, 0].max():.3g} m, {to_ref[:, 1].max():.3g} rad (bars {10 * ref['change'][0]:.3g}, "
          f"{10 * ref['change'][1]:.3g})")
    assert (to_truth.max(0) <= 2.0 * ref["to_truth"]).all()
    assert (to_ref.max(0) <= 10.0 * ref["change"]).all()
    assert (out["iterations"] <= 30).all() and (out["n_correspondences"] > 1000).all()
    lam = np.linalg.eigvalsh(out["information"])
    assert (lam > 0).all()                                               # the scene constrains all six unknowns


# ---- 7. edges ---------------------------------------------------------------------------------------------------------

def test_edges_in_one_batch(scene_map):
    """scans of 0 and 1 rows mid-batch, a scan with no usable voxel, a NaN initial pose"""
    s = K.scene()
    a, b = s["scans"][:2000], s["scans"][2000:4000]
    far = a + np.array([500.0, 500.0, 50.0], np.float32)                 # inside the grid, nowhere near the map
    nan_pose = s["init"][1].copy()
    nan_pose[1, 2] = np.nan
    scans = [a, a[:0], b[:1], far, b, b]
    init = np.stack([s["init"][0], s["init"][0], s["init"][1], s["init"][0], nan_pose, s["init"][1]])
    out = host(scene_map.register(scans, init, system0=True))
    alone = host(scene_map.register([a, b], s["init"][:2]))
    for i, j in ((0, 0), (5, 1)):
        for k in alone:
            assert out[k][i].tobytes() == alone[k][j].tobytes(), (i, k)
    assert out["n_correspondences"][1] == 0 and out["fitness"][1] == 0 and out["rmse"][1] == 0
    assert np.array_equal(out["transform"][1], init[1]) and not out["information"][1].any()
    one = R.lookup(K.scene_reference()["map"], b[:1], init[2])[1]       # its voxel is usable, 0.14 voxels from a face
    assert out["n_correspondences"][2] == int((one >= 0).sum()) == 1
    assert np.array_equal(out["transform"][2], init[2]) and out["iterations"][2] == 1    # rank 3: no step
    assert out["n_correspondences"][3] == 0 and np.array_equal(out["transform"][3], init[3]) and out["cost"][3] == 0
    assert out["n_correspondences"][4] == -1 and out["iterations"][4] == 0
    for k in ("transform", "fitness", "rmse", "cost", "information", "system0"):
        assert np.isnan(out[k][4]).all(), k


@pytest.mark.parametrize("n", [16383, 16384, 16385])
def test_rows_at_the_sweep_boundary(scene_map, n):
    """64 workgroups x 256 lanes take 16 384 rows per sweep"""
    assert _lib().MAP_REGISTER_BLOCKS * 256 == 16384
    s, ref = K.scene(), K.scene_reference()["map"]
    rows = np.concatenate([s["scans"][:2000]] * 9)[:n].astype(np.float64)
    rows += np.random.default_rng(n).normal(0, 0.01, rows.shape)
    T0 = s["init"][0]
    pts, off, _ = K.off_face_scans(ref, rows, np.array([0, n]), T0[None])
    pad = rows[:n - len(pts)]                                             # back to n rows, with rows that contribute nowhere
    pts = np.concatenate([pts, np.full_like(pad, np.nan)])
    assert len(pts) == n
    scene_map.reg.max_iteration = 1
    try:
        out = host(scene_map.register([pts], T0[None], system0=True))
    finally:
        scene_map.reg.max_iteration = 30
    want = R.linearize(ref, pts, T0)
    assert out["system0"][0, 27] == want[27] and want[27] > 10000
    assert close(out["system0"][0, :21], want[:21]) and close(out["system0"][0, 21:27], want[21:27])
    assert out["iterations"][0] == 1


def test_formats_agree(scene_map):
    s = K.scene()
    a = s["scans"][:2000]                                                 # float32 values
    off = dev(np.array([0, 2000], np.int64))
    rows4 = np.concatenate([a, np.full((2000, 1), np.nan, np.float32)], 1)
    outs = [host(scene_map.register((dev(r), off), s["init"][:1])) for r in (a, rows4, a.astype(np.float64))]
    for other in outs[1:]:
        for k in outs[0]:
            assert other[k].tobytes() == outs[0][k].tobytes(), k
    assert outs[0]["n_correspondences"][0] > 1000


# ---- 8. independence and determinism ----------------------------------------------------------------------------------

def test_alone_and_in_a_batch_and_twice(scene_map):
    s = K.scene()
    scans = list(np.split(s["scans"], 8))
    batch = host(scene_map.register(scans, s["init"]))
    again = host(scene_map.register(scans, s["init"]))
    for k in batch:
        assert batch[k].tobytes() == again[k].tobytes(), k
    for i in (0, 5):
        alone = host(scene_map.register(scans[i:i + 1], s["init"][i:i + 1]))
        for k in batch:
            assert alone[k][0].tobytes() == batch[k][i].tobytes(), (i, k)
    pts, off, poses = K.exact_case(1, 3500)
    a, b = built(pts, off, poses)[1], built(pts, off, poses)[1]
    n = int(a["stats"][1])
    for k in ("voxels", "info", "keys", "moments"):
        assert a[k][:n].tobytes() == b[k][:n].tobytes(), k
    # which of two colliding keys claims a slot first is free, so the index may differ in where a key sits, not in what
    # a lookup finds
    assert index_of(a) == index_of(b) and a["stats"].tobytes() == b["stats"].tobytes()


# ---- 9. capture -------------------------------------------------------------------------------------------------------

def test_captured_replay_equals_eager():
    from _hipgraph import capture_replay
    s = K.scene()
    m = localizer(max_voxels=2048, max_iteration=3)
    d_pts, d_off, d_poses = dev(s["points"]), dev(s["offsets"]), dev(s["poses"])
    eager, cap, types = capture_replay(lambda: m.build_device(d_pts, d_off, d_poses))
    assert types == {"kernel": 6}, types
    n = int(eager["stats"][1].item())
    assert n == K.scene_reference()["map"]["voxels_found"]
    assert index_of(host(eager)) == index_of(host(cap))           # where a key sits may differ, what a lookup finds not
    for k in set(eager) - {"index"}:
        rows = slice(None) if k == "stats" else slice(0, n)
        assert torch.equal(eager[k][rows], cap[k][rows]), k
    m.build_device(d_pts, d_off, d_poses)                         # the map the scans are registered against: not a graph's
    d_scans, d_soff, d_init = dev(s["scans"]), dev(s["scan_offsets"]), dev(s["init"])
    eager, cap, types = capture_replay(lambda: m.register_device(d_scans, d_soff, d_init))
    assert types == {"kernel": 1 + 2 * (3 + 1)}, types
    for k in eager:
        assert torch.equal(eager[k], cap[k]), k
    assert bool((eager["iterations"] == 3).all()) and bool((eager["n_correspondences"] > 1000).all())
