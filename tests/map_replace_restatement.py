"""Removal from and replacement in a kept map of include/nsc.h (nsc_map_remove_dist, nsc_map_replace_dist) restated
directly: the reference of tests/test_map_replace_cpu.py and tests/test_map_replace_gpu.py.

The state is map_insert_restatement's.  A removal is its insertion with the signs turned: a row is placed and keyed as
then, the dict gives the place of its key (a key the dict does not hold, or a place past the capacity, makes the row
missing), and the row's count of one and its nine Python integers are subtracted.  The record of a place a row was taken
from is map_localize_restatement.record of what is left, or sixteen zeros when nothing is left (count 0 and nine zero
moments: emptied) or when what is left is not a voxel (count below 0, or 0 with a moment: inconsistent).  Keys, places,
first rows and cloud bounds stay.  A replacement is a removal under the old poses and map_insert_restatement.insert under
the new ones, numbered from the caller's bases, with the cursor and the stats of dropped rows put back."""
import numpy as np

import map_insert_restatement as IR
import map_localize_restatement as R
import map_restatement as M

REMOVE_STAT_NAMES = ("rows_removed", "removed_not_finite", "removed_outside", "removed_without_pose", "rows_missing",
                     "voxels_touched", "voxels_emptied", "voxels_inconsistent")
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def remove(s, points, offsets, poses, pose_ids=None):
    """take packed clouds out of the state in place -> (the eight counts of ``removed``, the places touched in the order
    they were first reached, the places emptied, the places inconsistent)"""
    voxel, origin = s["grid"]
    p = np.asarray(points)[:, :3].astype(np.float64)
    w, cloud, has_pose = M.world_rows(points, offsets, poses, pose_ids)
    finite = has_pose & np.isfinite(p).all(1) & np.isfinite(w).all(1)
    k, q = R.inside_voxel(w, voxel, origin)
    with np.errstate(invalid="ignore"):
        kk = k + float(1 << 20)
        inside = finite & ((kk >= 0) & (kk < float(1 << M.KEY_BITS))).all(1)
    touched, missing, taken = [], 0, 0
    for r in np.nonzero(inside)[0].tolist():
        ki = [int(v) for v in kk[r]]
        key = ki[0] | (ki[1] << M.KEY_BITS) | (ki[2] << (2 * M.KEY_BITS))
        at = s["place"].get(key)
        if at is None or at >= s["capacity"]:
            missing += 1
            continue
        taken += 1
        if at not in touched:
            touched.append(at)
        mo, qq = s["moments"][at], [int(v) for v in q[r]]
        s["info"][at][0] -= 1
        for a in range(3):
            mo[a] -= qq[a]
        for t, (a, b) in enumerate(PAIRS):
            mo[3 + t] -= qq[a] * qq[b]
    emptied, inconsistent = [], []
    for at in touched:
        n = s["info"][at][0]
        if n > 0:
            s["voxels"][at] = R.record(s["moments"][at], n, IR.key_voxel(s["keys"][at]), voxel, origin, *s["rule"])
            continue
        s["voxels"][at] = np.zeros(16)
        (emptied if n == 0 and not any(s["moments"][at]) else inconsistent).append(at)
    s["stats"][2] -= taken
    counts = [taken, int((has_pose & ~finite).sum()), int((finite & ~inside).sum()), int((~has_pose).sum()), missing,
              len(touched), len(emptied), len(inconsistent)]
    return counts, touched, emptied, inconsistent


def replace(s, points, offsets, old_poses, new_poses, pose_ids=None, first_row=0, first_cloud=0):
    """move packed clouds of the state from old_poses to new_poses in place -> (removed (8), placed (7))"""
    counts = remove(s, points, offsets, old_poses, pose_ids)[0]
    cursor, before = list(s["cursor"]), list(s["stats"])
    s["cursor"] = [int(first_row), int(first_cloud)]
    IR.insert(s, points, offsets, new_poses, pose_ids)
    s["cursor"] = cursor
    st = s["stats"]
    placed = [st[0] - before[0], st[1]] + [st[i] - before[i] for i in range(2, 7)]
    st[3], st[4], st[5] = before[3], before[4], before[5]       # dropped rows of a replacement are not the map's
    return counts, placed


def mapping(m):
    """a map of the restatement (``arrays``, or build_dist's dict) -> {key: (count, the nine moments, the record's bytes)}"""
    return {int(key): (int(m["info"][i, 0]), tuple(int(v) for v in m["moments"][i]), m["voxels"][i].tobytes())
            for i, key in enumerate(m["keys"].tolist())}


EMPTIED = (0, (0,) * 9, np.zeros(16).tobytes())


def assert_follows(got, want, what=""):
    """``got`` (a kept map after removals) holds every voxel of ``want`` (the build over what remains) with the same
    count, moments and record bits, and every other keyed voxel of it is emptied -> the number of emptied voxels"""
    g, w = mapping(got), mapping(want)
    assert set(w) <= set(g), (what, len(set(w) - set(g)))
    for key, v in w.items():
        assert g[key] == v, (what, key, g[key][:2], v[:2])
    rest = set(g) - set(w)
    for key in rest:
        assert g[key] == EMPTIED, (what, key, g[key][:2])
    return len(rest)
