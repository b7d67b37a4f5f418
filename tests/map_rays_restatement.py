"""Seen-through voxels of include/nsc.h (nsc_map_cast_rays, nsc_map_flag_rows) restated in float64: the reference of
tests/test_map_rays_cpu.py and tests/test_map_rays_gpu.py.

Rows are placed by map_restatement.world_rows, the quantities of a ray (fo, d, D, L, t0, t1) are numpy float64 arrays made
one operation at a time, and every ray is then walked in Python floats (IEEE doubles, nothing fused).  The index is a plain
dict from key to place, ``crossed`` and the counters are Python integers.  The map is an argument -- ``voxels`` (V,16),
``place``, ``capacity`` and ``grid`` as map_localize_restatement.build_dist returns them -- so that the GPU tests can hand
in the device's own records: the restatement's come from numpy.linalg.eigh and the kernel's from Jacobi sweeps, and the
decision s <= gate^2 has to be made on the same bits.

``walk`` is generic in its number type: with fractions.Fraction it is the same walk in exact arithmetic."""
import math

import numpy as np

import map_insert_restatement as IR
import map_replace_restatement as RP
import map_restatement as M

RAY_STAT_NAMES = ("rays_cast", "rays_not_finite", "rays_outside", "rays_without_pose", "rays_short", "voxels_visited",
                  "crossings", "rays_truncated")
FLAG_STAT_NAMES = ("rows_flagged", "rows_kept", "rows_dropped", "rows_without_voxel")
MAX_REACH = 65536
HALF = 1 << 20


def key_of(k):
    """voxel coordinates relative to the origin voxel -> the packed key, or None outside the grid"""
    kk = [int(v) + HALF for v in k]
    if any(v < 0 or v >= (1 << M.KEY_BITS) for v in kk):
        return None
    return kk[0] | (kk[1] << M.KEY_BITS) | (kk[2] << (2 * M.KEY_BITS))


def max_steps(max_range, voxel):
    return 3 * (math.floor(max_range / voxel) + 2)


def walk(fo, d, t0, t1, steps):
    """the voxels of one ray -> a list of (k, ta, tb, tn of the step axis), and whether the ray ended before ``steps``"""
    k = [math.floor(fo[a] + t0 * d[a]) for a in range(3)]
    ta, out = t0, []
    for _ in range(steps):
        tn = [((k[a] + 1) - fo[a]) / d[a] if d[a] > 0 else (k[a] - fo[a]) / d[a] if d[a] < 0 else math.inf
              for a in range(3)]
        axis, tx = 0, tn[0]
        if tn[1] < tx:
            axis, tx = 1, tn[1]
        if tn[2] < tx:
            axis, tx = 2, tn[2]
        out.append((tuple(k), ta, min(tx, t1), tx))
        if not tx < t1:
            return out, True
        k[axis] += 1 if d[axis] > 0 else -1
        ta = tx
    return out, False


def rays(points, offsets, poses, pose_ids, grid, min_range=0.0, max_range=60.0, end_margin=None):
    """-> dict of the per-ray arrays: kind (0 cast, 1 not finite, 2 outside, 3 without pose, 4 short), o, w, fo, d, D, t0,
    t1, and end_key (Python integers, None where the row has no voxel)"""
    voxel, origin = float(grid[0]), np.asarray(grid[1], np.float64)
    p = np.asarray(points)[:, :3].astype(np.float64)
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    w, cloud, has_pose = M.world_rows(points, offsets, poses, pose_ids)
    ids = cloud if pose_ids is None else np.where(cloud >= 0, np.asarray(pose_ids, np.int64)[np.maximum(cloud, 0)], -1)
    o = np.full((len(p), 3), np.nan)
    o[has_pose] = poses[ids[has_pose]][:, :3, 3]
    em = voxel if end_margin is None or end_margin < 0 else float(end_margin)
    with np.errstate(all="ignore"):
        finite = has_pose & np.isfinite(p).all(1) & np.isfinite(w).all(1)
        fo, fw = (o - origin) / voxel, (w - origin) / voxel
        ko, kw = np.floor(fo) + float(HALF), np.floor(fw) + float(HALF)
        inside = finite & ((ko >= 0) & (ko < float(1 << M.KEY_BITS)) & (kw >= 0) & (kw < float(1 << M.KEY_BITS))).all(1)
        d, D = fw - fo, w - o
        L = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) * voxel
        t0 = float(min_range) / L
        t1 = np.minimum(1.0 - em / L, float(max_range) / L)
        long_enough = (L > 0.0) & (t0 < t1)
    kind = np.where(~has_pose, 3, np.where(~finite, 1, np.where(~inside, 2, np.where(~long_enough, 4, 0))))
    has_voxel = finite & ((kw >= 0) & (kw < float(1 << M.KEY_BITS))).all(1)             # the row's own voxel: o plays no part
    end_key = [key_of([v - HALF for v in k]) if ok else None for k, ok in zip(kw.tolist(), has_voxel.tolist())]
    return dict(kind=kind, o=o, w=w, fo=fo, d=d, D=D, t0=t0, t1=t1, end_key=end_key)


def examine(rec, o, D, ta, tb):
    """s = the smallest x^T Omega x of the segment [ta, tb] against the record (16 Python floats), as the header forms it"""
    O = ((rec[9], rec[10], rec[11]), (rec[10], rec[12], rec[13]), (rec[11], rec[13], rec[14]))
    a = (o[0] - rec[0], o[1] - rec[1], o[2] - rec[2])
    ea = [(O[r][0] * a[0] + O[r][1] * a[1]) + O[r][2] * a[2] for r in range(3)]
    eD = [(O[r][0] * D[0] + O[r][1] * D[1]) + O[r][2] * D[2] for r in range(3)]
    num = (D[0] * ea[0] + D[1] * ea[1]) + D[2] * ea[2]
    den = (D[0] * eD[0] + D[1] * eD[1]) + D[2] * eD[2]
    t = -num / den if den > 0.0 else ta
    t = min(max(t, ta), tb)
    x = (a[0] + t * D[0], a[1] + t * D[1], a[2] + t * D[2])
    ex = [(O[r][0] * x[0] + O[r][1] * x[1]) + O[r][2] * x[2] for r in range(3)]
    return (x[0] * ex[0] + x[1] * ex[1]) + x[2] * ex[2]


def walks(points, offsets, poses, pose_ids, grid, min_range=0.0, max_range=60.0, end_margin=None):
    """the rays of packed clouds and the walk of each ray that is cast -> (rays' dict, {row: walk's result}).  Nothing
    here depends on the map's records: a caller who casts the same rays into several maps on one grid walks them once"""
    voxel = float(grid[0])
    assert max_range / voxel <= MAX_REACH
    r = rays(points, offsets, poses, pose_ids, grid, min_range, max_range, end_margin)
    steps = max_steps(max_range, voxel)
    fo, d, t0, t1 = r["fo"].tolist(), r["d"].tolist(), r["t0"].tolist(), r["t1"].tolist()
    return r, {i: walk(fo[i], d[i], t0[i], t1[i], steps) for i in np.nonzero(r["kind"] == 0)[0].tolist()}


def cast(points, offsets, poses, pose_ids, m, min_range=0.0, max_range=60.0, end_margin=None, gate=3.0, crossed=None,
         walked=None):
    """cast the rows of packed clouds into the map ``m`` -> dict: crossed (capacity Python integers; ``crossed`` is added
    to, if given), stats (8), the stats by name, per_ray (the closest gate decision, relative, and the closest stop
    decision |tn - t1| of each row; inf where it made none), closest_gate and closest_stop (their minima).  ``walked``:
    what ``walks`` returned for the same rays, grid and ranges"""
    r, walked = walked or walks(points, offsets, poses, pose_ids, m["grid"], min_range, max_range, end_margin)
    g2 = float(gate) * float(gate)
    recs, place, cap = np.asarray(m["voxels"]).tolist(), m["place"], int(m["capacity"])
    crossed = [0] * cap if crossed is None else crossed
    stats = [int((r["kind"] == k).sum()) for k in range(5)] + [0, 0, 0]
    n = len(r["kind"])
    near_gate, near_stop = np.full(n, np.inf), np.full(n, np.inf)
    os_, Ds, t1s = r["o"].tolist(), r["D"].tolist(), r["t1"].tolist()
    for i, (visits, ended) in walked.items():
        o, D = os_[i], Ds[i]
        stats[5] += len(visits)
        stats[7] += not ended
        for k, ta, tb, tx in visits:
            near_stop[i] = min(near_stop[i], abs(tx - t1s[i]))
            key = key_of(k)
            if key is None or key == r["end_key"][i]:
                continue
            at = place.get(key, -1)
            if at < 0 or at >= cap or recs[at][15] != 1.0:
                continue
            s = examine(recs[at], o, D, ta, tb)
            near_gate[i] = min(near_gate[i], abs(s - g2) / g2)
            if s <= g2:
                crossed[at] += 1
                stats[6] += 1
    out = dict(crossed=crossed, stats=stats, per_ray=(near_gate, near_stop), closest_gate=float(near_gate.min(initial=np.inf)),
               closest_stop=float(near_stop.min(initial=np.inf)))
    out.update(zip(RAY_STAT_NAMES, stats))
    return out


def seen_through(count, crossed, min_crossings=3, ratio=0.5):
    """-> (places,) bool: count > 0, crossed >= min_crossings and (double)crossed >= ratio (double)count"""
    return np.array([n > 0 and c >= min_crossings and float(c) >= ratio * float(n) for n, c in zip(count, crossed)], bool)


def flag_rows(points, offsets, poses, pose_ids, m, count, crossed, min_crossings=3, ratio=0.5):
    """-> (flags (N,) bool: the row's own voxel is seen through; [rows flagged, kept, dropped, missing]).  ``count`` is
    the count of each place"""
    r = rays(points, offsets, poses, pose_ids, m["grid"])
    seen = seen_through(count, crossed, min_crossings, ratio)
    flags, stats = np.zeros(len(r["kind"]), bool), [0, 0, 0, 0]
    for i, key in enumerate(r["end_key"]):
        if key is None:
            stats[2] += 1
            continue
        at = m["place"].get(key, -1)
        if at < 0 or at >= m["capacity"]:
            stats[3] += 1
            continue
        flags[i] = bool(seen[at])
        stats[0 if seen[at] else 1] += 1
    return flags, stats


def without(points, mask):
    """the rows of ``mask`` made NaN"""
    p = np.array(points, copy=True)
    p[np.asarray(mask, bool)] = np.nan
    return p


def carve(s, points, offsets, poses, pose_ids, crossed, min_crossings=3, ratio=0.5):
    """flag the rows of the clouds against the state ``s`` (map_insert_restatement) and remove the flagged ones in place
    -> (carved (N,) bool, map_replace_restatement.remove's eight counts, flag_rows' four)"""
    m = IR.arrays(s)
    flags, fstats = flag_rows(points, offsets, poses, pose_ids, m, [r[0] for r in s["info"]], crossed, min_crossings, ratio)
    removed = RP.remove(s, without(points, ~flags), offsets, poses, pose_ids)[0]
    return flags, removed, fstats
