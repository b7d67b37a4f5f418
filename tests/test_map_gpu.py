"""The global voxel map on the MI355X: GlobalMap / nsc_map_build against the restatement (tests/map_restatement.py).

Bitwise comparisons use input that is exact in any evaluation order: points on the lattice of 2^-6 m strictly inside
voxels, rotations by multiples of 90 degrees about the axes, translations that are multiples of the voxel.  Every w, every
fixed-point value, every sum and every centroid is then exact, so points, info, keys and stats equal the restatement's bit
for bit.  General poses (test_general_poses) hold keys, counts, first rows, clouds, order and stats exactly, on input whose
world coordinates are asserted to stay 1e-6 voxel from every face, and centroids within 2^-23 m: a row's fixed-point value
can differ by one unit of 2^-24 m between a fused and an unfused R p + t, the mean of such values by at most one unit, plus
the rounding of the division."""
import numpy as np
import pytest
import torch

import map_restatement as M

pytestmark = pytest.mark.gpu

VOXEL = 0.5


def _lib():
    from neural_spectral_codec_amd import _lib
    return _lib


def global_map(**kw):
    from neural_spectral_codec_amd.retrieval import GlobalMap
    return GlobalMap(**kw)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def run(points, off, poses, ids=None, max_voxels=None, **kw):
    """build_device on host arrays -> the full buffers on the host"""
    return host(global_map(max_voxels=max_voxels, **kw).build_device(dev(points), dev(off), dev(poses), ids))


def assert_bitwise(out, ref, what=""):
    """stats, and the written voxels' points, info and keys, equal bit for bit"""
    assert out["stats"].tolist() == ref["stats"].tolist(), (what, out["stats"], ref["stats"])
    n = int(ref["stats"][1])
    for k in ("info", "keys", "points"):
        assert out[k][:n].tobytes() == np.ascontiguousarray(ref[k][:n]).tobytes(), (what, k)


def lattice_points(rng, n, half=3.0):
    """n points on the 2^-6 m lattice, 1 .. 31 steps inside a voxel of 0.5 m on every axis, within +-half"""
    v = rng.integers(-int(half / VOXEL), int(half / VOXEL), (n, 3))
    return (v * 32 + rng.integers(1, 32, (n, 3))) / 64.0


def rot90_pose(rng):
    """a rotation by multiples of 90 degrees about each axis and a translation of whole voxels: entries 0, +-1 and k / 2"""
    R = np.eye(3)
    for axis in range(3):
        c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][int(rng.integers(0, 4))]
        Q = np.eye(3)
        i, j = [(1, 2), (2, 0), (0, 1)][axis]
        Q[i, i], Q[i, j], Q[j, i], Q[j, j] = c, -s, s, c
        R = R @ Q
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = rng.integers(-8, 9, 3) * VOXEL
    return T


def general_pose(yaw, tilt, t):
    cz, sz, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(tilt), np.sin(tilt)
    T = np.eye(4)
    T[:3, :3] = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    T[:3, 3] = t
    return T


def offsets_with_empty_clouds(n):
    """six clouds over n rows: none at the start, in the middle and at the end"""
    return np.array([0, 0, n // 3, n // 3, 2 * n // 3, n, n], np.int64)


def exact_case(seed, n, half=3.0):
    rng = np.random.default_rng(seed)
    off = offsets_with_empty_clouds(n)
    return lattice_points(rng, n, half), off, np.stack([rot90_pose(rng) for _ in range(len(off) - 1)])


# ---- 1. bitwise on exactly representable input, all three formats -----------------------------------------------------

def test_bitwise_on_exact_input_all_formats():
    pts, off, poses = exact_case(1, 3500)
    ref = M.build_map(pts, off, poses)
    assert ref["rows_used"] == 3500 and 500 < ref["voxels_found"] < 3000 and ref["info"][:, 0].max() > 3
    assert M.face_distance(ref["world"], ref["used"]) >= 1.0 / 32
    rows4 = np.concatenate([pts, np.full((len(pts), 1), np.nan)], 1).astype(np.float32)      # the 4th column is not read
    outs = [run(pts.astype(np.float32), off, poses), run(rows4, off, poses), run(pts, off, poses)]
    for out, what in zip(outs, ("float32 x 3", "float32 x 4", "float64")):
        assert_bitwise(out, ref, what)
    n = ref["voxels_found"]
    for other in outs[1:]:
        for k in ("points", "info", "keys"):
            assert other[k][:n].tobytes() == outs[0][k][:n].tobytes(), k


# ---- 2. general poses: exact membership, centroids within 2^-23 m -----------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_general_poses(dtype):
    rng = np.random.default_rng(2)
    n = 3000
    world = (rng.integers(-40, 40, (n, 3)) + rng.uniform(1e-3, 1.0 - 1e-3, (n, 3))) * VOXEL          # +-20 m
    poses = np.stack([general_pose(0.3, 0.02, [1.0, -2.0, 0.3]), general_pose(-2.1, -0.03, [-7.5, 4.0, -0.2])])
    sensor = np.concatenate([(world - T[:3, 3]) @ T[:3, :3] for T in poses]).astype(dtype)          # R^T (w - t)
    off = np.array([0, n, 2 * n], np.int64)
    ref = M.build_map(sensor, off, poses)
    # the condition on the input: from the rounded rows, every w at least 1e-6 voxel from a face, no row left out
    assert ref["rows_used"] == 2 * n and M.face_distance(ref["world"], ref["used"]) >= 1e-6
    assert ref["info"][:, 0].min() >= 2                                                           # both views, every voxel
    out = run(sensor, off, poses)
    assert out["stats"].tolist() == ref["stats"].tolist()
    v = ref["voxels_found"]
    assert np.array_equal(out["keys"][:v], ref["keys"]) and np.array_equal(out["info"][:v], ref["info"])
    err = np.abs(out["points"][:v] - ref["points"]).max()
    print(f"{np.dtype(dtype).name}: {v} voxels, centroid error {err:.3g} m (bar {2.0 ** -23:.3g})")
    assert err <= 2.0 ** -23


# ---- 3. the purpose: a consistent map has fewer voxels than a bent one ------------------------------------------------

def test_wrong_pose_occupies_more_voxels():
    from neural_spectral_codec_amd.retrieval import revisited
    g = np.arange(-8.0, 8.0, 0.25) + 0.125                                  # 0.125 m from every voxel face
    floor = np.stack(np.meshgrid(g, g, [-1.7], indexing="ij"), -1).reshape(-1, 3)
    wall = np.stack(np.meshgrid([8.2], g, np.arange(-1.5, 2.5, 0.25) + 0.125, indexing="ij"), -1).reshape(-1, 3)
    world = np.concatenate([floor, wall])
    true = [np.eye(4), general_pose(np.deg2rad(30.0), 0.0, [2.0, 1.0, 0.0])]
    views = [((world - T[:3, 3]) @ T[:3, :3]).astype(np.float32) for T in true]
    m = global_map()
    one = m.build(views[:1], true[:1])
    two = m.build(views, true)
    assert one["complete"] and two["complete"] and two["rows_used"] == 2 * len(world)
    assert two["voxels_found"] == one["voxels_found"] and torch.equal(two["keys"], one["keys"])
    assert bool(revisited(two["first_cloud"], two["last_cloud"], 1).all())
    assert not bool(revisited(one["first_cloud"], one["last_cloud"], 1).any())
    off = general_pose(np.deg2rad(2.0), 0.0, [0.7, 0.0, 0.0]) @ true[1]       # 0.7 m and 2 degrees off
    bent = m.build(views, [true[0], off])
    print(f"voxels: one view {one['voxels_found']}, two views {two['voxels_found']}, second pose off {bent['voxels_found']}")
    assert bent["voxels_found"] > two["voxels_found"]


# ---- 4. sizes where the compaction and the grid-stride loops can go wrong ---------------------------------------------

def _boundaries():
    L = _lib()
    scan = L.MAP_SCAN_THREADS * L.MAP_TILE_ROWS             # above it a scan thread takes two tiles
    wrap = L.MAP_INSERT_BLOCKS * L.MAP_INSERT_ROWS          # above it the insert pass's workgroups take a second sweep
    return L.MAP_TILE_ROWS, sorted({scan + 1, wrap + 1})


@pytest.mark.parametrize("which", ["0", "1", "T-1", "T", "T+1", "64", "65"])
def test_small_sizes_and_empty_clouds(which):
    T, _ = _boundaries()
    n = {"0": 0, "1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "64": 64, "65": 65}[which]
    pts, off, poses = exact_case(40 + n % 7, n)
    ref = M.build_map(pts, off, poses)
    assert ref["rows_used"] == n
    assert_bitwise(run(pts.astype(np.float32), off, poses), ref, which)
    assert_bitwise(run(pts, off, poses), ref, which)


def test_sizes_above_the_scan_and_insert_boundaries():
    _, sizes = _boundaries()
    for n in sizes:
        pts, off, poses = exact_case(5, n, half=20.0)
        ref = M.build_map(pts, off, poses)
        assert ref["rows_used"] == n and ref["voxels_found"] > 400000
        assert ref["info"][:, 1].max() > 0.9 * n              # first rows up to the input's end: every tile holds some
        assert_bitwise(run(pts.astype(np.float32), off, poses), ref, str(n))


def test_no_clouds():
    poses = np.eye(4)[None]
    out = run(np.zeros((0, 3), np.float32), np.zeros(1, np.int64), poses)
    assert out["stats"].tolist() == [0] * 7
    pts = lattice_points(np.random.default_rng(0), 3)
    out = run(pts, np.zeros(1, np.int64), poses)                # rows, but no cloud holds them
    ref = M.build_map(pts, np.zeros(1, np.int64), poses)
    assert ref["rows_without_pose"] == 3
    assert_bitwise(out, ref)
    out = run(pts, np.array([0, 3], np.int64), np.zeros((0, 4, 4)))              # a cloud, but no pose
    assert out["stats"].tolist() == [0, 0, 0, 0, 0, 3, 0]


def test_voxel_across_tiles_and_clouds():
    T, _ = _boundaries()
    n = 2 * T + 3
    i = np.arange(n)
    pts = (np.stack([i % 64, (i // 64) % 64, i // 4096], 1) * 32 + 7) / 64.0        # a voxel per row ...
    shared = [0, T + 1, 2 * T + 2]                                                  # ... but these three share one
    pts[shared] = (np.array([[-3, -3, -3]]) * 32 + np.array([[1, 5, 9], [30, 2, 17], [16, 16, 31]])) / 64.0
    off = np.array([0, T, 2 * T + 1, n], np.int64)
    poses = np.tile(np.eye(4), (3, 1, 1))
    ref = M.build_map(pts, off, poses)
    assert ref["voxels_found"] == n - 2 and ref["info"][0].tolist() == [3, 0, 0, 2]
    out = run(pts, off, poses)
    assert_bitwise(out, ref)
    assert out["info"][0].tolist() == [3, 0, 0, 2]


# ---- 5. dropped rows are counted and change nothing else --------------------------------------------------------------

def test_dropped_rows_are_counted():
    rng = np.random.default_rng(6)
    n = 2400
    pts = lattice_points(rng, n)
    off = np.array([0, 600, 1200, 1800, n], np.int64)
    poses = np.stack([rot90_pose(rng) for _ in range(4)])
    pts[[3, 700, 2399]] = np.nan
    pts[[10, 1500], [0, 2]] = [np.inf, -np.inf]
    bad_pose = poses.copy()
    bad_pose[2, 1, 3] = np.nan                                  # every row of the cloud that uses pose 2
    ids = np.array([1, -1, 2, 0])
    ref = M.build_map(pts, off, bad_pose, ids)
    assert ref["rows_without_pose"] == 600 and ref["rows_not_finite"] == 600 + 3 and ref["rows_used"] == 1200 - 3
    for rows in (pts.astype(np.float32), pts):
        assert_bitwise(run(rows, off, bad_pose, ids), ref, "nan, inf, nan pose, -1")
    # an id past the poses, on a device tensor (the host refuses it): the cloud is left out like -1
    past = torch.tensor([1, 4, 2, 0], device="cuda")
    assert_bitwise(run(pts, off, bad_pose, past), ref, "device id past the poses")
    # outside the grid: with a far origin the 2^21 bound runs through the cloud, low on x and high on y
    far = (524288.0, -524288.0, 0.0)
    ref = M.build_map(pts, off, poses, origin=far)
    w = ref["world"]
    expect = np.isfinite(w).all(1) & ((w[:, 0] < 0) | (w[:, 1] >= 0))
    assert ref["rows_outside"] == expect.sum() and 0 < ref["rows_used"] < n - 5
    assert_bitwise(run(pts, off, poses, origin=far), ref, "far origin")
    # and with a tiny voxel: +-2^20 x 2^-22 m = +-0.25 m is all the grid covers
    tiny = 2.0 ** -22
    ref = M.build_map(pts, off, poses, voxel_size=tiny)
    assert ref["rows_outside"] > 0 and ref["rows_used"] + ref["rows_outside"] == n - 5
    assert_bitwise(run(pts, off, poses, voxel_size=tiny), ref, "tiny voxel")


# ---- 6. capacity ------------------------------------------------------------------------------------------------------

def _ten_voxels():
    rng = np.random.default_rng(7)
    vox = np.stack([np.arange(10) - 5, (np.arange(10) * 3) % 7 - 3, np.arange(10) % 2], 1)
    which = np.concatenate([np.arange(10), rng.integers(0, 10, 15)])
    pts = (vox[which] * 32 + rng.integers(1, 32, (25, 3))) / 64.0
    return pts, np.array([0, 12, 25], np.int64), np.tile(np.eye(4), (2, 1, 1))


def test_capacity_outputs_short():
    pts, off, poses = _ten_voxels()
    ref = M.build_map(pts, off, poses, max_voxels=6)
    assert ref["stats"][:2].tolist() == [10, 6]
    out = run(pts, off, poses, max_voxels=6)                   # 12 slots hold the 10 keys
    assert out["stats"].tolist() == [10, 6, 25, 0, 0, 0, 0]
    assert_bitwise(out, ref)
    res = global_map(max_voxels=6).build((dev(pts), dev(off)), poses)
    assert res["complete"] is False and res["voxels_found"] == 10 and len(res["points"]) == 6


def test_capacity_table_short():
    pts, off, poses = _ten_voxels()
    ref = M.build_map(pts, off, poses)
    m = global_map(max_voxels=4)                                # 8 slots for 10 keys
    guard, sentinel = 8, -77
    big = dict(points=torch.full((4 + guard, 3), float(sentinel), dtype=torch.float64, device="cuda"),
               info=torch.full((4 + guard, 4), sentinel, dtype=torch.int64, device="cuda"),
               keys=torch.full((4 + guard,), sentinel, dtype=torch.int64, device="cuda"),
               stats=torch.full((7 + guard,), sentinel, dtype=torch.int64, device="cuda"))
    views = dict(points=big["points"][:4], info=big["info"][:4], keys=big["keys"][:4], stats=big["stats"][:7])
    out = host(m.build_device(dev(pts), dev(off), dev(poses), out=views))          # returns: NSC_OK
    found, written, used, _, _, _, unplaced = out["stats"].tolist()
    assert unplaced > 0 and written <= 4 and found <= 8 and used + unplaced == 25
    assert written == min(found, 4)
    for k, at in (("points", 4), ("info", 4), ("keys", 4), ("stats", 7)):
        assert bool((big[k][at:] == sentinel).all()), k                            # nothing past the buffers
    # a voxel that is in the table has all of its rows: what was written are voxels of the complete map, in its order
    place = {int(k): i for i, k in enumerate(ref["keys"])}
    at = [place[int(k)] for k in out["keys"][:written]]
    assert at == sorted(at)
    assert out["info"][:written].tobytes() == ref["info"][at].tobytes()
    assert out["points"][:written].tobytes() == ref["points"][at].tobytes()
    assert m.build((dev(pts), dev(off)), poses)["complete"] is False


# ---- 7. determinism ---------------------------------------------------------------------------------------------------

def test_two_calls_agree_and_cloud_order_is_free():
    rng = np.random.default_rng(8)
    sizes = np.array([900, 0, 1300, 700, 1100])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    world = lattice_points(rng, int(off[-1]), half=2.5)
    poses = np.stack([general_pose(0.4 * c, 0.01 * c, [c, -c, 0.1 * c]) for c in range(5)])
    pts = np.concatenate([(world[off[c]:off[c + 1]] - poses[c][:3, 3]) @ poses[c][:3, :3] for c in range(5)])
    a, b = run(pts, off, poses), run(pts, off, poses)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    v = int(a["stats"][0])
    assert a["info"][:v, 0].max() > 3

    def permuted(perm):                                             # new cloud i is old cloud perm[i]
        p2 = np.concatenate([pts[off[c]:off[c + 1]] for c in perm])
        o2 = np.concatenate([[0], np.cumsum(sizes[perm])]).astype(np.int64)
        return run(p2, o2, poses, np.asarray(perm))

    def voxels(out, clouds=None):
        return {(int(k), int(i[0]), p.tobytes()) + (clouds(i) if clouds else ())
                for k, i, p in zip(out["keys"][:v], out["info"][:v], out["points"][:v])}
    other = permuted([3, 0, 4, 2, 1])
    assert other["stats"].tolist() == a["stats"].tolist() and voxels(other) == voxels(a)
    rev = permuted([4, 3, 2, 1, 0])                                 # the reversal maps min to max
    assert voxels(rev, lambda i: (4 - int(i[3]), 4 - int(i[2]))) == voxels(a, lambda i: (int(i[2]), int(i[3])))


# ---- 8. capture -------------------------------------------------------------------------------------------------------

def test_captured_replay_equals_eager():
    from _hipgraph import keep_graphs, node_types
    pts, off, poses = exact_case(9, 5000)
    other, _, other_poses = exact_case(10, 5000)
    m = global_map(max_voxels=4096)
    d_pts, d_off, d_poses = dev(pts.astype(np.float32)), dev(off), dev(poses)

    def step():
        return m.build_device(d_pts, d_off, d_poses)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                               # warm the allocator outside the capture
    torch.cuda.current_stream().wait_stream(s)
    with keep_graphs() as made:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cap = step()
    d_pts.copy_(dev(other.astype(np.float32)))               # other values, the same shapes
    d_poses.copy_(dev(other_poses))
    eager = host(step())
    for t in cap.values():
        t.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    replayed = host(cap)
    ref = M.build_map(other.astype(np.float32), off, other_poses, max_voxels=4096)
    assert_bitwise(eager, ref)
    assert_bitwise(replayed, ref)
    types = node_types(made[0])
    assert types == {"kernel": 6}, types                      # include/nsc.h: six launches, the Python layer adds none


# ---- 9. the clouds stage 2 keeps are the map's input ------------------------------------------------------------------

def test_build_prepared_equals_build_on_the_stored_clouds():
    import gicp_clouds as GC
    from neural_spectral_codec_amd.retrieval import PreparedClouds
    store = PreparedClouds(voxel_size=0.5)
    store.add([GC.surface(s, n=600, ext=6.0) for s in (1, 2, 3)])
    poses = np.stack([general_pose(0.2 * c, 0.01, [0.4 * c, -0.3 * c, 0.0]) for c in range(3)])
    m = global_map(voxel_size=1.0)
    clouds = [store.cloud(i)["points"] for i in range(3)]
    assert all(c.dtype == torch.float64 and len(c) > 50 for c in clouds)
    for ids in (None, [0, -1, 2]):
        a, b = m.build_prepared(store, poses, ids), m.build(clouds, poses, ids)
        assert a["complete"] and a["rows_used"] == sum(len(c) for i, c in enumerate(clouds) if ids is None or ids[i] >= 0)
        assert a["rows_without_pose"] == (0 if ids is None else len(clouds[1]))
        for k in a:
            same = torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]
            assert same, k
        ref = M.build_map(torch.cat(clouds).cpu().numpy(), np.cumsum([0] + [len(c) for c in clouds]), poses, ids,
                          voxel_size=1.0)
        assert a["voxels_found"] == ref["voxels_found"] and np.array_equal(a["keys"].cpu().numpy(), ref["keys"])
        assert np.array_equal(a["first_cloud"].cpu().numpy(), ref["info"][:, 2])
    left_out = m.build_prepared(store, poses, [0, -1, 2])             # the map of the two other clouds
    rest = m.build([clouds[0], clouds[2]], poses[[0, 2]])
    assert torch.equal(left_out["keys"], rest["keys"]) and torch.equal(left_out["points"], rest["points"])
