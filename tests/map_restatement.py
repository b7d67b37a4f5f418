"""The global voxel map of include/nsc.h (nsc_map_build) restated in float64 numpy: the reference of tests/test_map_gpu.py.

Rows are visited in packed order and grouped by a plain dict from voxel key to the voxel's place, so the voxels come out in
the order of their first rows by construction.  Every operation is rounded on its own, in the order the header states:
w_a = ((R_a0 x + R_a1 y) + R_a2 z) + t_a, k_a = floor((w_a - origin_a) / voxel_size) + 2^20, sums of rint(w_a 2^24) in
int64, centroid_a = (sum_a / 2^24) / count."""
import numpy as np

STAT_NAMES = ("voxels_found", "voxels_written", "rows_used", "rows_not_finite", "rows_outside", "rows_without_pose",
              "rows_unplaced")
KEY_BITS = 21
FIX = float(1 << 24)


def world_rows(points, offsets, poses, pose_ids=None):
    """-> w (N,3) float64 (NaN where no pose applies), cloud (N,) of each packed row (-1: in no cloud), has_pose (N,)"""
    pts = np.asarray(points)
    p = pts[:, :3].astype(np.float64)
    off = np.asarray(offsets, np.int64)
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    rows = np.arange(len(p), dtype=np.int64)
    # the largest c with off[c] <= row: clouds of no rows are never it
    cloud = np.searchsorted(off[:-1], rows, side="right") - 1
    if len(off) > 1:
        cloud[(cloud >= 0) & (rows >= off[np.maximum(cloud, 0) + 1])] = -1
    ids = cloud.copy() if pose_ids is None else np.where(cloud >= 0, np.asarray(pose_ids, np.int64)[np.maximum(cloud, 0)], -1)
    has_pose = (cloud >= 0) & (ids >= 0) & (ids < len(poses))
    w = np.full((len(p), 3), np.nan)
    if has_pose.any():
        T = poses[ids[has_pose]]
        x, y, z = p[has_pose].T
        with np.errstate(all="ignore"):
            for a in range(3):
                w[has_pose, a] = ((T[:, a, 0] * x + T[:, a, 1] * y) + T[:, a, 2] * z) + T[:, a, 3]
    return w, cloud, has_pose


def build_map(points, offsets, poses, pose_ids=None, voxel_size=0.5, origin=(0.0, 0.0, 0.0), max_voxels=None):
    """-> dict of points (V,3) float64, info (V,4) int64 = [count, first_row, first_cloud, last_cloud], keys (V,) int64,
    stats (7,) int64 and the stats by name; ``used`` (N,) bool and ``world`` (N,3) for the tests' conditions on the input.
    All V voxels are returned (the table is never short here); voxels_written = min(V, max_voxels)."""
    pts = np.asarray(points)
    p = pts[:, :3].astype(np.float64)
    origin = np.asarray(origin, np.float64)
    w, cloud, has_pose = world_rows(points, offsets, poses, pose_ids)
    finite = has_pose & np.isfinite(p).all(1) & np.isfinite(w).all(1)
    with np.errstate(all="ignore"):
        k = np.floor((w - origin) / float(voxel_size)) + float(1 << 20)
    inside = finite & ((k >= 0) & (k < float(1 << KEY_BITS))).all(1)
    rows = np.nonzero(inside)[0]
    ki = k[rows].astype(np.int64)
    keys = ki[:, 0] | (ki[:, 1] << KEY_BITS) | (ki[:, 2] << (2 * KEY_BITS))
    place = {}
    g = np.fromiter((place.setdefault(key, len(place)) for key in keys.tolist()), np.int64, count=len(keys))
    V = len(place)
    fixed = np.rint(w[rows] * FIX).astype(np.int64)
    sums = np.zeros((V, 3), np.int64)
    np.add.at(sums, g, fixed)
    count = np.bincount(g, minlength=V).astype(np.int64)
    first_row = np.full(V, np.iinfo(np.int64).max)
    np.minimum.at(first_row, g, rows)
    first_cloud = np.full(V, np.iinfo(np.int64).max)
    np.minimum.at(first_cloud, g, cloud[rows])
    last_cloud = np.full(V, -1, np.int64)
    np.maximum.at(last_cloud, g, cloud[rows])
    assert np.all(np.diff(first_row) > 0)                    # row order: a voxel's place is the order of its first row
    out_keys = np.fromiter(place.keys(), np.int64, count=V)
    stats = np.array([V, V if max_voxels is None else min(V, int(max_voxels)), len(rows), int((has_pose & ~finite).sum()),
                      int((finite & ~inside).sum()), int((~has_pose).sum()), 0], np.int64)
    out = dict(points=(sums.astype(np.float64) / FIX) / count[:, None].astype(np.float64),
               info=np.stack([count, first_row, first_cloud, last_cloud], 1).reshape(V, 4), keys=out_keys, stats=stats,
               used=inside, world=w)
    out.update(zip(STAT_NAMES, stats.tolist()))
    return out


def face_distance(world, used, voxel_size=0.5, origin=(0.0, 0.0, 0.0)):
    """the smallest distance, in voxels, of a used row's world coordinate from a voxel face"""
    q = (world[used] - np.asarray(origin, np.float64)) / float(voxel_size)
    f = q - np.floor(q)
    return float(np.minimum(f, 1.0 - f).min()) if len(q) else 1.0
