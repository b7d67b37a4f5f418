"""Insertion into a kept map of include/nsc.h (nsc_map_insert_dist) restated directly: the reference of
tests/test_map_insert_cpu.py and tests/test_map_insert_gpu.py.

The state is map_localize_restatement.build_dist's dict and a cursor.  An insertion visits its rows in order: a row is
placed, keyed and counted as map_restatement does it, a key the dict does not hold takes the next place, and the row's
nine Python integers are added to the moments of its place.  Rows and clouds are numbered on from the cursor.  The record
of every place a row reached is map_localize_restatement.record of its integers: the same function of the same integers
as a build over all clouds, so the two agree to the last bit."""
import numpy as np

import map_localize_restatement as R
import map_restatement as M

BIG = np.iinfo(np.int64).max


def start(m, n_rows, n_clouds, min_points=6, eigen_ratio=1e-2, sigma_floor=1e-3):
    """build_dist's dict over n_clouds clouds of n_rows rows (built with these parameters) -> a state ``insert`` adds to"""
    s = dict(grid=m["grid"], capacity=m["capacity"], place=dict(m["place"]), keys=m["keys"].tolist(),
             info=m["info"].tolist(), moments=[list(r) for r in m["moments"].tolist()],
             voxels=[r.copy() for r in m["voxels"]], stats=m["stats"].tolist(), cursor=[int(n_rows), int(n_clouds)],
             rule=(int(min_points), float(eigen_ratio), float(sigma_floor)))
    return s


def key_voxel(key):
    """packed key -> the voxel coordinate relative to the origin voxel"""
    mask = (1 << M.KEY_BITS) - 1
    return [((key >> (a * M.KEY_BITS)) & mask) - (1 << 20) for a in range(3)]


def insert(s, points, offsets, poses, pose_ids=None):
    """add packed clouds to the state in place -> the places the rows reached, in the order they were first reached"""
    voxel, origin = s["grid"]
    pts = np.asarray(points)
    p = pts[:, :3].astype(np.float64)
    w, cloud, has_pose = M.world_rows(points, offsets, poses, pose_ids)
    finite = has_pose & np.isfinite(p).all(1) & np.isfinite(w).all(1)
    k, q = R.inside_voxel(w, voxel, origin)
    with np.errstate(invalid="ignore"):
        kk = k + float(1 << 20)
        inside = finite & ((kk >= 0) & (kk < float(1 << M.KEY_BITS))).all(1)
    row0, cloud0 = s["cursor"]
    touched = []
    for r in np.nonzero(inside)[0].tolist():
        ki = [int(v) for v in kk[r]]
        key = ki[0] | (ki[1] << M.KEY_BITS) | (ki[2] << (2 * M.KEY_BITS))
        at = s["place"].get(key)
        if at is None:
            at = s["place"][key] = len(s["keys"])
            s["keys"].append(key)
            s["info"].append([0, row0 + r, BIG, -1])
            s["moments"].append([0] * 9)
            s["voxels"].append(np.zeros(16))
        if at not in touched:
            touched.append(at)
        info, mo, qq, c = s["info"][at], s["moments"][at], [int(v) for v in q[r]], cloud0 + int(cloud[r])
        info[0] += 1
        info[2], info[3] = min(info[2], c), max(info[3], c)
        for a in range(3):
            mo[a] += qq[a]
        for t, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            mo[3 + t] += qq[a] * qq[b]
    for at in touched:                   # a place an unmatched removal left below one row keeps the zero record until it has one
        s["voxels"][at] = R.record(s["moments"][at], s["info"][at][0], key_voxel(s["keys"][at]), voxel, origin, *s["rule"]) \
            if s["info"][at][0] > 0 else np.zeros(16)
    st = s["stats"]
    st[0] = len(s["keys"])
    st[1] = min(st[0], s["capacity"])
    st[2] += int(inside.sum())
    st[3] += int((has_pose & ~finite).sum())
    st[4] += int((finite & ~inside).sum())
    st[5] += int((~has_pose).sum())
    s["cursor"] = [row0 + len(p), cloud0 + len(np.asarray(offsets)) - 1]
    return touched


def arrays(s):
    """the state as build_dist returns a map: keys (V,), info (V,4), stats (7,) int64, moments (V,9) object,
    voxels (V,16) float64, place, grid, capacity, and the stats by name"""
    V = len(s["keys"])
    moments = np.zeros((V, 9), object)
    for i, r in enumerate(s["moments"]):
        moments[i] = r
    out = dict(keys=np.array(s["keys"], np.int64), info=np.array(s["info"], np.int64).reshape(V, 4),
               stats=np.array(s["stats"], np.int64), moments=moments,
               voxels=np.stack(s["voxels"]) if V else np.zeros((0, 16)), place=dict(s["place"]), grid=s["grid"],
               capacity=s["capacity"], cursor=list(s["cursor"]))
    out.update(zip(M.STAT_NAMES, s["stats"]))
    return out
