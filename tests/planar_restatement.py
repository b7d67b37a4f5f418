"""Float64 numpy restatement of the planar initial guess (retrieval/planar_alignment.py's definition; the kernels
are csrc/nsc_planar.hip).  Independent of the library: nothing here calls it.  ``votes`` is the vectorised form,
``votes_loop`` the same definition as three nested Python loops."""
import math

import numpy as np

DEFAULTS = dict(cell=0.5, half_bins=24, z_window=0.5, normal_z2_max=0.25, source_stride=2, guard=5)
EPSILON = 1e-3           # the plane regularisation the clouds were prepared with (PreparedClouds' default)


def yaw_table(step_deg=2.0):
    """((H,2) (cos, sin) of theta_h = -180 + h step, the (H,) angles in degrees)"""
    H = int(round(360.0 / step_deg))
    deg = [-180.0 + h * step_deg for h in range(H)]
    return table_of(deg), np.array(deg)


def table_of(degrees):
    return np.array([[math.cos(math.radians(d)), math.sin(math.radians(d))] for d in degrees], np.float64).reshape(-1, 2)


def structure(cov6, normal_z2_max=0.25, epsilon=EPSILON):
    """(m,) bool: (1 - C_zz) < normal_z2_max (1 - epsilon); zz is the last of xx xy xz yy yz zz"""
    cov6 = np.asarray(cov6, np.float64).reshape(-1, 6)
    return (1.0 - cov6[:, 5]) < normal_z2_max * (1.0 - epsilon)


def rows_taken(sp, sc, tp, tc, P, epsilon=EPSILON):
    """-> (source rows taken (a,3), target structure rows (b,3))"""
    sp, tp = np.asarray(sp, np.float64).reshape(-1, 3), np.asarray(tp, np.float64).reshape(-1, 3)
    s_ok = structure(sc, P["normal_z2_max"], epsilon) & (np.arange(len(sp)) % P["source_stride"] == 0)
    return sp[s_ok], tp[structure(tc, P["normal_z2_max"], epsilon)]


def votes(sp, sc, tp, tc, yaw_cs, epsilon=EPSILON, near=None, **params):
    """(H, n, n) int32 vote counts, n = 2 half_bins + 1, of source (points, covariances) against target.  ``near``: a
    dict that receives ``edge`` = pre-floor values within 1e-9 of a bin edge but not on it (over the pairs that pass
    the z test) and ``z`` = |dz| within 1e-9 of z_window but not equal to it."""
    P = dict(DEFAULTS, **params)
    S, T = rows_taken(sp, sc, tp, tc, P, epsilon)
    hb, n = P["half_bins"], 2 * P["half_bins"] + 1
    inv_cell = 1.0 / P["cell"]
    yaw_cs = np.asarray(yaw_cs, np.float64).reshape(-1, 2)
    out = np.zeros((len(yaw_cs), n * n), np.int64)
    if near is not None:
        near.update(edge=0, z=0)
    if len(S) == 0 or len(T) == 0:
        return out.reshape(-1, n, n).astype(np.int32)
    dz = np.abs(T[None, :, 2] - S[:, None, 2])
    z_ok = dz <= P["z_window"]
    if near is not None:
        near["z"] = int(((np.abs(dz - P["z_window"]) < 1e-9) & (dz != P["z_window"])).sum())
    for h, (c, s) in enumerate(yaw_cs):
        xr = c * S[:, 0] - s * S[:, 1]
        yr = s * S[:, 0] + c * S[:, 1]
        ux = (T[None, :, 0] - xr[:, None]) * inv_cell + 0.5
        uy = (T[None, :, 1] - yr[:, None]) * inv_cell + 0.5
        bx, by = np.floor(ux), np.floor(uy)
        ok = (np.abs(bx) <= hb) & (np.abs(by) <= hb) & z_ok
        flat = ((bx[ok] + hb) * n + (by[ok] + hb)).astype(np.int64)
        out[h] = np.bincount(flat, minlength=n * n)
        if near is not None:
            for u in (ux, uy):
                w = u[z_ok & (np.abs(u) <= hb + 2)]
                d = np.abs(w - np.rint(w))
                near["edge"] += int(((d < 1e-9) & (d != 0.0)).sum())
    return out.reshape(-1, n, n).astype(np.int32)


def votes_loop(sp, sc, tp, tc, yaw_cs, epsilon=EPSILON, **params):
    """``votes`` by brute force: one Python iteration per (hypothesis, source row, target row)."""
    P = dict(DEFAULTS, **params)
    hb, n = P["half_bins"], 2 * P["half_bins"] + 1
    inv_cell = 1.0 / P["cell"]
    thr = P["normal_z2_max"] * (1.0 - epsilon)
    out = np.zeros((len(yaw_cs), n, n), np.int32)
    for h, (c, s) in enumerate(np.asarray(yaw_cs, np.float64)):
        for i, (a, ca) in enumerate(zip(np.asarray(sp, np.float64), np.asarray(sc, np.float64))):
            if i % P["source_stride"] != 0 or not (1.0 - ca[5]) < thr:
                continue
            xr = np.float64(c * a[0]) - np.float64(s * a[1])
            yr = np.float64(s * a[0]) + np.float64(c * a[1])
            for b, cb in zip(np.asarray(tp, np.float64), np.asarray(tc, np.float64)):
                if not (1.0 - cb[5]) < thr:
                    continue
                bx = math.floor((b[0] - xr) * inv_cell + 0.5)
                by = math.floor((b[1] - yr) * inv_cell + 0.5)
                if abs(bx) <= hb and abs(by) <= hb and abs(b[2] - a[2]) <= P["z_window"]:
                    out[h, bx + hb, by + hb] += 1
    return out


def reduce(v, yaw_cs, cell=0.5, guard=5):
    """(H, n, n) votes -> dict(yaw_peaks (H,2) int32 = [peak_h, flat bin_h], best (3,) int32 = [h, bx, by], scores
    (2,) int32 = [peak, runner_up], init (4,4))"""
    v = np.asarray(v)
    H, n = v.shape[0], v.shape[1]
    hb = (n - 1) // 2
    flat = v.reshape(H, n * n)
    bins = flat.argmax(1)                                     # the first of equal maxima: the smaller flat index
    peaks = flat[np.arange(H), bins]
    yaw_peaks = np.stack([peaks, bins], 1).astype(np.int32)
    best = int(peaks.argmax())                                # ... the smaller h
    peak = int(peaks[best])
    init = np.eye(4)
    if peak == 0:
        return dict(yaw_peaks=yaw_peaks, best=np.array([-1, 0, 0], np.int32), scores=np.array([0, 0], np.int32),
                    init=init)
    d = np.abs(np.arange(H) - best)
    far = np.minimum(d, H - d) > guard
    runner = int(peaks[far].max()) if far.any() else 0
    bx, by = int(bins[best]) // n - hb, int(bins[best]) % n - hb
    c, s = np.asarray(yaw_cs, np.float64)[best]
    init[:2, :2] = [[c, -s], [s, c]]
    init[0, 3], init[1, 3] = bx * cell, by * cell
    return dict(yaw_peaks=yaw_peaks, best=np.array([best, bx, by], np.int32),
                scores=np.array([peak, runner], np.int32), init=init)


def align(sp, sc, tp, tc, yaw_cs, epsilon=EPSILON, near=None, **params):
    """-> reduce's dict + votes (H,n,n) and counts (2,) int32 = [source rows taken, target structure rows]"""
    P = dict(DEFAULTS, **params)
    v = votes(sp, sc, tp, tc, yaw_cs, epsilon, near, **params)
    out = reduce(v, yaw_cs, P["cell"], P["guard"])
    S, T = rows_taken(sp, sc, tp, tc, P, epsilon)
    out.update(votes=v, counts=np.array([len(S), len(T)], np.int32))
    return out


def info(r):
    """planar_info's numbers of an ``align`` result"""
    peak, runner = int(r["scores"][0]), int(r["scores"][1])
    T = r["init"]
    return dict(init_yaw_deg=float(np.degrees(np.arctan2(T[1, 0], T[0, 0]))), init_translation=T[:3, 3].copy(),
                planar_peak=peak, planar_peak_ratio=peak / runner if runner > 0 else float("inf"),
                planar_support=peak / int(r["counts"][0]) if r["counts"][0] > 0 and peak > 0 else 0.0)
