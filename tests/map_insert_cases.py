"""Constructed inputs of tests/test_map_insert_cpu.py and tests/test_map_insert_gpu.py, beside those of
tests/map_localize_cases.py.  The CPU file asserts what each case claims about itself; the GPU file relies on it."""
import numpy as np

import map_localize_cases as K

MASK = (1 << 64) - 1
FAR = np.array([20, 21, 22])                 # a voxel no exact_case reaches (they stay within +-3 and +-8 of translation)


def pack(clouds):
    """a list of (n,c) arrays -> (points, offsets)"""
    off = np.zeros(len(clouds) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    return np.concatenate(clouds), off


def mix64(x):
    """the hash of csrc/nsc_voxel_hash.h"""
    x ^= x >> 33; x = (x * 0xff51afd7ed558ccd) & MASK
    x ^= x >> 33; x = (x * 0xc4ceb9fe1a85ec53) & MASK
    return x ^ (x >> 33)


def general_split(dtype=np.float32, cols=3):
    """eight clouds of 400 rows under general poses, about thirteen rows per voxel, every row 1e-3 voxel off the faces.
    -> dict: clouds, poses (8,4,4) and the groups A (three clouds, x voxels -4 .. 0), B (three clouds, x voxels -1 .. 3:
    partly A's voxels, partly new ones), C_old (one cloud, in voxels of A alone) and C_new (one cloud, x voxels 6 and 7:
    new voxels alone)"""
    rng = np.random.default_rng(31)
    n = 400
    poses = np.stack([K.general_pose(0.4 * i - 1.2, 0.01 * i - 0.03, [1.1 * i - 3.0, 0.7 * i - 2.0, 0.1 * i], roll=0.02)
                      for i in range(8)])

    def voxels(lo, hi):
        return np.stack([rng.integers(lo, hi, n), rng.integers(-3, 3, n), rng.integers(-1, 1, n)], 1)
    vox = [voxels(-4, 1) for _ in range(3)] + [voxels(-1, 4) for _ in range(3)]
    vox.append(vox[0][rng.integers(0, n, n)])                    # voxels the first cloud of A occupies
    vox.append(voxels(6, 8))
    clouds = []
    for v, T in zip(vox, poses):
        world = v + rng.uniform(1e-3, 1.0 - 1e-3, (n, 3))
        sensor = ((world - T[:3, 3]) @ T[:3, :3]).astype(dtype)
        clouds.append(sensor if cols == 3 else np.concatenate([sensor, np.full((n, 1), np.nan, dtype)], 1))
    return dict(clouds=clouds, poses=poses, A=[0, 1, 2], B=[3, 4, 5], C_old=[6], C_new=[7])


def sized_insert(n):
    """A: exact_case of 600 rows.  B: exact_case of n rows in six clouds, three of them empty.  With n > 3000 the rows
    700, 1500 and 3000 of B lie in the voxel FAR, which nothing else reaches: a new voxel whose rows fall to the workgroups
    1, 2 and 5 of the row passes (512 rows each), the smallest of them not to the first"""
    pa, oa, Ta = K.exact_case(90, 600)
    pb, ob, Tb = K.exact_case(91 + n % 5, n)
    rows = [700, 1500, 3000] if n > 3000 else []
    for r, frac in zip(rows, ([5, 9, 33], [17, 2, 60], [40, 40, 1])):
        c = int(np.searchsorted(ob[:-1], r, side="right") - 1)
        world = FAR + np.array(frac) / 64.0
        pb[r] = Tb[c][:3, :3].T @ (world - Tb[c][:3, 3])          # exact: a rot90 pose and lattice coordinates
    return (pa, oa, Ta), (pb, ob, Tb), rows


def twelve_voxels(min_points=6):
    """twelve voxels of 1.0 m, lattice points, identity poses.  A (one cloud) fills voxels 0 .. 6, B (two clouds) voxels
    4 .. 11 -> (A, B, vox): with max_voxels = 8 voxel 7 takes the last place and voxels 8 .. 11 are past the outputs"""
    rng = np.random.default_rng(17)
    vox = np.stack([np.arange(12) - 6, (np.arange(12) * 5) % 7 - 3, np.arange(12) % 3 - 1], 1)

    def rows(which):
        return (vox[which] * 64 + rng.integers(1, 64, (len(which), 3))) / 64.0
    a = rows(np.concatenate([np.arange(7), np.repeat(np.arange(7), min_points)]))
    b = rows(np.concatenate([np.arange(4, 12), np.repeat(np.arange(4, 12), min_points)]))
    A = (a, np.array([0, len(a)], np.int64), np.eye(4)[None])
    B = (b, np.array([0, len(b) // 2, len(b)], np.int64), np.tile(np.eye(4), (2, 1, 1)))
    return A, B, vox


def voxel_key(v):
    k = np.asarray(v, np.int64) + (1 << 20)
    return int(k[0]) | (int(k[1]) << 21) | (int(k[2]) << 42)


def ten_voxels_split():
    """K.ten_voxels, its first cloud as A and its second as B -> (A, B, vox)"""
    pts, off, poses, vox = K.ten_voxels()
    h = int(off[1])
    return (pts[:h], np.array([0, h], np.int64), poses[:1]), (pts[h:], np.array([0, len(pts) - h], np.int64), poses[1:]), vox


def every_kind_of_row():
    """B for a map of K.ten_voxels: five clouds of four rows inside voxels of the map, with pose ids [0, -1, 2, 0, 0]
    of one pose: clouds 1 and 2 have no pose.  Cloud 0 is usable as it stands; cloud 3 holds NaN and inf rows and cloud 4
    rows outside the grid -> (points, offsets, poses, pose_ids, the counts used, not finite, outside, without pose)"""
    _, _, _, vox = K.ten_voxels()
    rng = np.random.default_rng(23)
    inside = lambda i, k: (vox[i] * 64 + rng.integers(1, 64, (k, 3))) / 64.0
    clouds = [inside(0, 4), inside(1, 4), inside(2, 4),
              np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan]]),
              np.array([[2.0e6, 0.5, 0.5], [0.5, -3.0e6, 0.5], [0.5, 0.5, 1.0e300], [-1.5e6, 0.5, 0.5]])]
    pts, off = pack(clouds)
    return pts, off, np.eye(4)[None], np.array([0, -1, 2, 0, 0], np.int64), (4, 4, 4, 8)


def one_row_in_the_unusable_voxel():
    """one row inside voxel 4 of K.ten_voxels, the voxel of min_points - 1 rows"""
    _, _, _, vox = K.ten_voxels()
    return (vox[4] * 64 + np.array([[11, 29, 47]])) / 64.0


def scene_far_scan():
    """the first scan of K.scene moved 500 m away: inside the grid, in no voxel of the map"""
    return K.scene()["scans"][:2000] + np.array([500.0, 500.0, 50.0], np.float32)
