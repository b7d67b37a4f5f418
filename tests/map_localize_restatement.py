"""Map localisation of include/nsc.h (nsc_map_build_dist, nsc_map_register) restated in float64 numpy with Python-integer
moment sums: the reference of tests/test_map_localize_cpu.py and tests/test_map_localize_gpu.py.

The build takes placement, keys, order, info and stats from map_restatement.build_map.  A voxel's moments are sums of
Python integers, its mean and covariance exact rationals (fractions.Fraction) rounded once to float64, its information from
numpy.linalg.eigh of that covariance.  The lookup is a plain dict from key to place.  One linearisation and the round loop
follow the header's definition with numpy's own solver."""
from fractions import Fraction

import numpy as np

import gauss_newton_restatement as GN
import map_restatement as M

Q = 1 << 16
SYSTEM = 30                              # 21 JtOJ + 6 JtOd + n_corr + sum |d|^2 + sum dtOd


def inside_voxel(world, voxel_size, origin):
    """-> k (N,3) float64 voxel coordinates and q (N,3) int64 positions inside the voxel, in [-2^15, 2^15]"""
    with np.errstate(all="ignore"):
        f = (world - np.asarray(origin, np.float64)) / float(voxel_size)
        k = np.floor(f)
        q = np.rint((f - k) * float(Q)) - float(Q // 2)
    return k, q


def information(C6, eigen_ratio, sigma_floor):
    """(6,) xx xy xz yy yz zz -> the (6,) information U diag(1 / max(l, eigen_ratio l_max, sigma_floor^2)) U^T"""
    C = np.array([[C6[0], C6[1], C6[2]], [C6[1], C6[3], C6[4]], [C6[2], C6[4], C6[5]]])
    lam, U = np.linalg.eigh(C)
    lam = np.maximum(np.maximum(lam, eigen_ratio * lam.max()), sigma_floor ** 2)
    O = (U / lam) @ U.T
    return np.array([O[0, 0], O[0, 1], O[0, 2], O[1, 1], O[1, 2], O[2, 2]])


def record(moments, n, k, voxel_size, origin, min_points, eigen_ratio, sigma_floor):
    """nine Python-integer sums, the count and the voxel coordinate (relative to the origin voxel) -> the (16,) record;
    mean and covariance are exact rationals rounded once"""
    s, ss = moments[:3], moments[3:]
    v = Fraction(float(voxel_size))
    mean = [float(Fraction(float(origin[a])) + (Fraction(int(k[a])) + Fraction(1, 2) + Fraction(s[a], n * Q)) * v)
            for a in range(3)]
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    C6 = [float((Fraction(ss[t], n) - Fraction(s[a], n) * Fraction(s[b], n)) * (v / Q) ** 2)
          for t, (a, b) in enumerate(pairs)]
    O6 = information(C6, eigen_ratio, sigma_floor)
    rec = np.array(mean + C6 + O6.tolist() + [0.0])
    rec[15] = 1.0 if n >= min_points and np.isfinite(rec[:15]).all() else 0.0
    return rec


def build_dist(points, offsets, poses, pose_ids=None, voxel_size=1.0, origin=(0.0, 0.0, 0.0), max_voxels=None,
               min_points=6, eigen_ratio=1e-2, sigma_floor=1e-3):
    """-> map_restatement.build_map's dict (keys, info, stats, used, world; all V voxels), and moments (V,9) Python
    integers as an object array, voxels (V,16) float64, place {key: place} and the grid and capacity for the lookup"""
    out = M.build_map(points, offsets, poses, pose_ids, voxel_size=voxel_size, origin=origin, max_voxels=max_voxels)
    rows = np.nonzero(out["used"])[0]
    k, q = inside_voxel(out["world"][rows], voxel_size, origin)
    place = {int(key): i for i, key in enumerate(out["keys"].tolist())}
    ki = (k + float(1 << 20)).astype(np.int64)
    keys = ki[:, 0] | (ki[:, 1] << M.KEY_BITS) | (ki[:, 2] << (2 * M.KEY_BITS))
    V = len(place)
    moments = np.zeros((V, 9), object)
    kv = np.zeros((V, 3))
    for key, kk, qq in zip(keys.tolist(), k.tolist(), q.astype(np.int64).tolist()):
        m = moments[place[key]]
        kv[place[key]] = kk
        m[0] += qq[0]; m[1] += qq[1]; m[2] += qq[2]
        m[3] += qq[0] * qq[0]; m[4] += qq[0] * qq[1]; m[5] += qq[0] * qq[2]
        m[6] += qq[1] * qq[1]; m[7] += qq[1] * qq[2]; m[8] += qq[2] * qq[2]
    count = out["info"][:, 0]
    out["moments"] = moments
    out["voxels"] = np.stack([record(moments[i].tolist(), int(count[i]), kv[i], voxel_size, origin, min_points,
                                     eigen_ratio, sigma_floor) for i in range(V)]) if V else np.zeros((0, 16))
    out["place"] = place
    out["grid"] = (float(voxel_size), np.asarray(origin, np.float64))
    out["capacity"] = V if max_voxels is None else int(max_voxels)
    return out


def transform_rows(points, T):
    """w = ((R_a0 x + R_a1 y) + R_a2 z) + t_a, every operation rounded on its own"""
    p = np.asarray(points)[:, :3].astype(np.float64)
    T = np.asarray(T, np.float64)
    with np.errstate(all="ignore"):
        return np.stack([((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)], 1)


def lookup(m, points, T):
    """-> w (N,3) and place (N,) of the usable voxel each row falls into under T, -1 for a row that does not contribute:
    not finite, outside the grid, voxel absent, past the capacity or not usable"""
    p = np.asarray(points)[:, :3].astype(np.float64)
    w = transform_rows(points, T)
    voxel, origin = m["grid"]
    k, _ = inside_voxel(w, voxel, origin)
    k = k + float(1 << 20)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(p).all(1) & np.isfinite(w).all(1) & ((k >= 0) & (k < float(1 << M.KEY_BITS))).all(1)
    place = np.full(len(p), -1, np.int64)
    ki = k[ok].astype(np.int64)
    keys = ki[:, 0] | (ki[:, 1] << M.KEY_BITS) | (ki[:, 2] << (2 * M.KEY_BITS))
    at = np.array([m["place"].get(key, -1) for key in keys.tolist()], np.int64)
    at[at >= m["capacity"]] = -1
    usable = m["voxels"][:, 15] == 1.0
    at[(at >= 0) & ~usable[np.maximum(at, 0)]] = -1
    place[ok] = at
    return w, place


def sym3(s6):
    """(n,6) xx xy xz yy yz zz -> (n,3,3)"""
    return s6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def linearize(m, points, T):
    """the 30 sums of one scan at T: the upper triangle of sum J^T O J row by row, sum J^T O d, n_corr, sum |d|^2,
    sum d^T O d, with J = [-[w]x | I]"""
    w, place = lookup(m, points, T)
    sel = place >= 0
    w, rec = w[sel], m["voxels"][place[sel]]
    d = w - rec[:, 0:3]
    O = sym3(rec[:, 9:15])
    J = np.zeros((len(w), 3, 6))
    J[:, 0, 1], J[:, 0, 2] = w[:, 2], -w[:, 1]
    J[:, 1, 0], J[:, 1, 2] = -w[:, 2], w[:, 0]
    J[:, 2, 0], J[:, 2, 1] = w[:, 1], -w[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
    H = np.einsum("nra,nrs,nsb->ab", J, O, J)
    g = np.einsum("nra,nrs,ns->a", J, O, d)
    out = np.zeros(SYSTEM)
    out[:21] = H[np.triu_indices(6)]
    out[21:27] = g
    out[27], out[28], out[29] = len(w), (d * d).sum(), np.einsum("nr,nrs,ns->", d, O, d)
    return out


def rot_zyx(a, b, g):
    ca, sa, cb, sb, cg, sg = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(g), np.sin(g)
    return np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                     [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                     [-sb, cb * sa, cb * ca]])


def update(x):
    """the six unknowns, rotation first -> dT (4,4)"""
    dT = np.eye(4)
    dT[:3, :3] = rot_zyx(x[0], x[1], x[2])
    dT[:3, 3] = x[3:6]
    return dT


def full(system):
    """the 21 upper-triangle terms -> the symmetric (6,6)"""
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = system[:21]
    return H + np.triu(H, 1).T


def register_one(m, points, T0, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """-> dict of transform, fitness, rmse, cost, n_correspondences, iterations, information, system0 of one scan"""
    T = np.array(T0, np.float64)
    n = len(points)
    if not np.isfinite(T).all():
        nan = np.nan
        return dict(transform=np.full((4, 4), nan), fitness=nan, rmse=nan, cost=nan, n_correspondences=-1, iterations=0,
                    information=np.full((6, 6), nan), system0=np.full(SYSTEM, nan))
    prev, system0 = None, None
    for rnd in range(max_iteration + 1):
        s = linearize(m, points, T)
        if rnd == 0:
            system0 = s
        nc = s[27]
        fitness = nc / n if n > 0 else 0.0
        rmse = np.sqrt(s[28] / nc) if nc > 0 else 0.0
        done = rnd == max_iteration
        if prev is not None and abs(prev[0] - fitness) < relative_fitness and abs(prev[1] - rmse) < relative_rmse:
            done = True
        if done:
            return dict(transform=T, fitness=fitness, rmse=rmse, cost=s[29], n_correspondences=int(nc), iterations=rnd,
                        information=full(s), system0=system0)
        prev = (fitness, rmse)
        if nc > 0:
            H = full(s)
            if not GN.regular(H):                                 # no step on a singular system: the written rule
                continue
            T = update(np.linalg.solve(H, -s[21:27])) @ T


def register(m, points, offsets, init, **kw):
    """register_one over packed scans -> a dict of stacked arrays"""
    off = np.asarray(offsets, np.int64)
    res = [register_one(m, np.asarray(points)[off[i]:off[i + 1]], init[i], **kw) for i in range(len(off) - 1)]
    return {k: np.stack([np.asarray(r[k]) for r in res]) for k in res[0]} if res else {}


def keep_off_faces(m, points, T, margin=1e-6):
    """the mask of rows whose transformed point stays at least ``margin`` voxels from every voxel face (rows that are
    not finite count as kept: they contribute nowhere)"""
    w = transform_rows(points, T)
    voxel, origin = m["grid"]
    with np.errstate(invalid="ignore"):
        f = (w - origin) / voxel
        u = f - np.floor(f)
        near = (np.minimum(u, 1.0 - u) < margin).any(1)
    return ~near
