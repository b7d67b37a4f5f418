"""Constructed inputs of tests/test_map_localize_cpu.py and tests/test_map_localize_gpu.py.  The CPU file asserts what each
case claims about itself (exactness, distance from voxel faces, which voxels are usable or past the capacity); the GPU file
relies on those claims."""
import functools

import numpy as np

import map_localize_restatement as R
import map_restatement as M

FACE_MARGIN = 1e-6                      # voxels: the distance transformed rows keep from every voxel face


def rot90_pose(rng, voxel):
    """a rotation by multiples of 90 degrees about each axis and a translation of whole voxels"""
    Rm = np.eye(3)
    for axis in range(3):
        c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][int(rng.integers(0, 4))]
        Q = np.eye(3)
        i, j = [(1, 2), (2, 0), (0, 1)][axis]
        Q[i, i], Q[i, j], Q[j, i], Q[j, j] = c, -s, s, c
        Rm = Rm @ Q
    T = np.eye(4)
    T[:3, :3] = Rm
    T[:3, 3] = rng.integers(-8, 9, 3) * voxel
    return T


def general_pose(yaw, tilt, t, roll=0.0):
    cz, sz, cx, sx, cy, sy = np.cos(yaw), np.sin(yaw), np.cos(tilt), np.sin(tilt), np.cos(roll), np.sin(roll)
    T = np.eye(4)
    T[:3, :3] = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
        np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    T[:3, 3] = t
    return T


def offsets_with_empty_clouds(n):
    """six clouds over n rows: none at the start, in the middle and at the end"""
    return np.array([0, 0, n // 3, n // 3, 2 * n // 3, n, n], np.int64)


def exact_case(seed, n, voxel=1.0, half=3.0):
    """n points on the 2^-6 m lattice strictly inside voxels of ``voxel`` (0.5 or 1.0) m within +-half, six clouds under
    rot90 poses: every world coordinate, q and moment is exact in any evaluation order"""
    rng = np.random.default_rng(seed)
    steps = int(round(voxel * 64))
    v = rng.integers(-int(half / voxel), int(half / voxel), (n, 3))
    pts = (v * steps + rng.integers(1, steps, (n, 3))) / 64.0
    off = offsets_with_empty_clouds(n)
    return pts, off, np.stack([rot90_pose(rng, voxel) for _ in range(len(off) - 1)])


def general_case(dtype, voxel=1.0):
    """two views of 3000 world points within +-4 voxels under general poses, about twelve rows per voxel"""
    rng = np.random.default_rng(2)
    n = 3000
    world = (rng.integers(-4, 4, (n, 3)) + rng.uniform(1e-3, 1.0 - 1e-3, (n, 3))) * voxel
    poses = np.stack([general_pose(0.3, 0.02, [1.0, -2.0, 0.3]), general_pose(-2.1, -0.03, [-7.5, 4.0, -0.2])])
    sensor = np.concatenate([(world - T[:3, 3]) @ T[:3, :3] for T in poses]).astype(dtype)
    return sensor, np.array([0, n, 2 * n], np.int64), poses


def ten_voxels(min_points=6):
    """ten voxels of 1.0 m in first-row order: voxel i has min_points + 2 rows, but voxel 3 has exactly min_points and
    voxel 4 exactly min_points - 1 (not usable); two clouds, identity poses, lattice points"""
    rng = np.random.default_rng(7)
    vox = np.stack([np.arange(10) - 5, (np.arange(10) * 3) % 7 - 3, np.arange(10) % 2], 1)
    per = np.full(10, min_points + 2)
    per[3], per[4] = min_points, min_points - 1
    which = np.concatenate([np.arange(10), np.repeat(np.arange(10), per - 1)])
    pts = (vox[which] * 64 + rng.integers(1, 64, (len(which), 3))) / 64.0
    n = len(pts)
    return pts, np.array([0, n // 2, n], np.int64), np.tile(np.eye(4), (2, 1, 1)), vox


def lookup_scan(vox):
    """rows for a map of ten_voxels with max_voxels = 6 -> (points, category of each row): in a present and usable voxel
    (0, 1, 2, 3, 5), in the voxel that is not usable (4), in voxels past the capacity (6 .. 9), in absent voxels, outside
    the grid, and not finite"""
    rng = np.random.default_rng(11)
    rows, cat = [], []

    def inside(v, k):
        return (np.asarray(v) * 64 + rng.integers(1, 64, (k, 3))) / 64.0
    for i in (0, 1, 2, 3, 5):
        rows.append(inside(vox[i], 7)); cat += ["usable"] * 7
    rows.append(inside(vox[4], 5)); cat += ["unusable"] * 5
    for i in (6, 7, 8, 9):
        rows.append(inside(vox[i], 3)); cat += ["overflow"] * 3
    rows.append(inside([20, 20, 20], 4)); cat += ["absent"] * 4
    rows.append(inside([-30, 2, 1], 4)); cat += ["absent"] * 4
    rows.append(np.array([[2.0e6, 0.5, 0.5], [0.5, -3.0e6, 0.5], [0.5, 0.5, 1.0e300]])); cat += ["outside"] * 3
    rows.append(np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5]])); cat += ["not finite"] * 2
    pts, cat = np.concatenate(rows), np.array(cat)
    perm = rng.permutation(len(pts))
    return pts[perm], cat[perm]


# ---- the end-to-end scene: a floor, three walls (one of them tilted) and a slanted panel -----------------------------

def _surfaces():
    """(origin, u, v) of each rectangle: points origin + a u + b v, a and b in [0, 1]"""
    tilt = np.deg2rad(8.0)
    return [
        (np.array([-10.0, -10.0, -1.6]), np.array([20.0, 0, 0]), np.array([0, 20.0, 0])),                     # floor
        (np.array([9.3, -10.0, -1.6]), np.array([0, 20.0, 0]), np.array([0, 0, 5.0])),                        # wall x
        (np.array([-10.0, 8.7, -1.6]), np.array([20.0, 0, 0]), np.array([0, 0, 5.0])),                        # wall y
        (np.array([-9.4, -10.0, -1.6]), np.array([0, 20.0, 0]), 5.0 * np.array([np.sin(tilt), 0, np.cos(tilt)])),   # tilted
        (np.array([-3.0, -8.2, -1.6]), np.array([6.0, 1.5, 0]), np.array([0, 1.2, 3.0])),                     # slanted panel
    ]


def scene_points(rng, n, noise=0.01):
    """n world points on the scene's surfaces (by area), with ``noise`` m of Gaussian noise"""
    surf = _surfaces()
    area = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v in surf])
    which = rng.choice(len(surf), n, p=area / area.sum())
    ab = rng.uniform(0, 1, (n, 2))
    o = np.stack([s[0] for s in surf])[which]
    u = np.stack([s[1] for s in surf])[which]
    v = np.stack([s[2] for s in surf])[which]
    return o + ab[:, :1] * u + ab[:, 1:] * v + rng.normal(0, noise, (n, 3))


def _view(world, T, dtype=np.float32):
    return ((world - T[:3, 3]) @ T[:3, :3]).astype(dtype)


@functools.lru_cache(maxsize=None)
def scene():
    """-> dict: the map's input (six clouds of 4 000 rows under their true poses), eight scans of 2 000 rows with their
    true poses and their initial poses (+-0.3 m, +-3 degrees yaw, +-1 degree roll and pitch off)"""
    rng = np.random.default_rng(2024)
    map_poses = np.stack([general_pose(0.5 * c, 0.01 * c, [1.5 * c - 4.0, 0.8 * c - 2.0, 0.05 * c]) for c in range(6)])
    clouds = [_view(scene_points(rng, 4000), T) for T in map_poses]
    off = np.arange(7, dtype=np.int64) * 4000
    truth = np.stack([general_pose(0.7 * s - 2.0, 0.0, [0.9 * s - 3.0, 2.0 - 0.6 * s, 0.1]) for s in range(8)])
    scans = [_view(scene_points(rng, 2000), T) for T in truth]
    init = []
    for T in truth:
        sg = rng.choice([-1.0, 1.0], 6)
        dT = general_pose(sg[0] * np.deg2rad(3.0), sg[1] * np.deg2rad(1.0), sg[3:6] * 0.3 / np.sqrt(3.0),
                          roll=sg[2] * np.deg2rad(1.0))
        init.append(dT @ T)
    return dict(points=np.concatenate(clouds), offsets=off, poses=map_poses, scans=np.concatenate(scans),
                scan_offsets=np.arange(9, dtype=np.int64) * 2000, truth=truth, init=np.stack(init))


def pose_error(A, B):
    """-> (translation distance in m, rotation angle in rad) between two (4,4) poses"""
    dR = A[:3, :3] @ B[:3, :3].T
    axis = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])     # sin(angle) x axis
    return float(np.linalg.norm(A[:3, 3] - B[:3, 3])), float(np.arctan2(np.linalg.norm(axis), (np.trace(dR) - 1.0) / 2.0))


@functools.lru_cache(maxsize=None)
def scene_reference():
    """the restatement on the scene, once: its map, its registration of the eight scans, its own worst error to the truth
    and the largest change of its result when every scan coordinate moves by +-2^-24 m"""
    s = scene()
    m = R.build_dist(s["points"], s["offsets"], s["poses"], voxel_size=1.0)
    ref = R.register(m, s["scans"], s["scan_offsets"], s["init"])
    to_truth = np.array([pose_error(a, b) for a, b in zip(ref["transform"], s["truth"])]).max(0)
    rng = np.random.default_rng(5)
    moved = s["scans"].astype(np.float64) + rng.choice([-1.0, 1.0], s["scans"].shape) * 2.0 ** -24
    alt = R.register(m, moved, s["scan_offsets"], s["init"])
    change = np.array([pose_error(a, b) for a, b in zip(ref["transform"], alt["transform"])]).max(0)
    return dict(map=m, ref=ref, to_truth=to_truth, change=change)


def off_face_scans(m, points, offsets, poses, margin=FACE_MARGIN):
    """the scans with the rows left out whose transformed point comes within ``margin`` voxels of a face
    -> (points, offsets, share of rows left out)"""
    off = np.asarray(offsets, np.int64)
    keep = np.concatenate([R.keep_off_faces(m, points[off[i]:off[i + 1]], poses[i], margin) for i in range(len(off) - 1)])
    sizes = [int(keep[off[i]:off[i + 1]].sum()) for i in range(len(off) - 1)]
    return points[keep], np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), 1.0 - keep.mean()
