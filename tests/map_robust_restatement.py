"""nsc_map_register_robust of include/nsc.h restated in float64 numpy on top of map_localize_restatement: robust weights on
s = d^T Omega d and, with ``neighbours=7``, the six face neighbours of a row's voxel.  The reference of
tests/test_map_robust_cpu.py and tests/test_map_robust_gpu.py.

With ``kernel=None`` and ``neighbours=1`` every array handed to numpy is the one map_localize_restatement hands to it, so
the results are equal exactly."""
import numpy as np

import gauss_newton_restatement as GN
import map_localize_restatement as R
import map_restatement as M

SYSTEM = 32                              # map_localize_restatement's 30 sums, then sum w and n_pairs
W_SUM, N_PAIRS = 30, 31
KERNELS = (None, "huber", "cauchy", "geman_mcclure")
# the fixed order of a row's candidate voxels
OFFSETS = np.array([(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], np.float64)


def rho_w(kernel, c, s):
    """(n,) s -> rho(s) and w = rho'(s); quadratic (rho = s, w = 1) without a kernel and where s <= 0"""
    s = np.asarray(s, np.float64)
    rho, w = s.copy(), np.ones_like(s)
    if kernel is None:
        return rho, w
    assert kernel in KERNELS and np.isfinite(c) and c > 0
    c2 = c * c
    pos = s > 0
    sp = s[pos]
    if kernel == "huber":
        q = np.sqrt(sp)
        far = sp > c2
        rho[pos] = np.where(far, 2.0 * c * q - c2, sp)
        w[pos] = np.where(far, c / q, 1.0)
    elif kernel == "cauchy":
        rho[pos] = c2 * np.log1p(sp / c2)
        w[pos] = 1.0 / (1.0 + sp / c2)
    else:
        t = c2 / (c2 + sp)
        rho[pos] = t * sp
        w[pos] = t * t
    return rho, w


def pairs(m, points, T, neighbours=1):
    """-> w (N,3), row (P,) and place (P,) of every pair (row, usable voxel) under T: a row's pairs stand together, in the
    fixed order of OFFSETS"""
    assert neighbours in (1, 7)
    p = np.asarray(points)[:, :3].astype(np.float64)
    w = R.transform_rows(points, T)
    voxel, origin = m["grid"]
    k, _ = R.inside_voxel(w, voxel, origin)
    k = k + float(1 << 20)
    top = float(1 << M.KEY_BITS)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(p).all(1) & np.isfinite(w).all(1) & ((k >= 0) & (k < top)).all(1)
    usable = m["voxels"][:, 15] == 1.0
    row, order, place = [], [], []
    for j in range(neighbours):
        kj = k + OFFSETS[j]
        with np.errstate(invalid="ignore"):
            sel = np.nonzero(ok & ((kj >= 0) & (kj < top)).all(1))[0]         # a neighbour outside the grid is skipped
        ki = kj[sel].astype(np.int64)
        keys = ki[:, 0] | (ki[:, 1] << M.KEY_BITS) | (ki[:, 2] << (2 * M.KEY_BITS))
        at = np.array([m["place"].get(key, -1) for key in keys.tolist()], np.int64)
        at[at >= m["capacity"]] = -1
        at[(at >= 0) & ~usable[np.maximum(at, 0)]] = -1
        row.append(sel[at >= 0]); place.append(at[at >= 0]); order.append(np.full(int((at >= 0).sum()), j))
    row, place, order = np.concatenate(row), np.concatenate(place), np.concatenate(order)
    by = np.lexsort((order, row))
    return w, row[by], place[by]


def terms(m, w, row, place):
    """-> d (P,3), Omega (P,3,3), J (P,3,6) of the pairs"""
    w = w[row]
    rec = m["voxels"][place]
    d = w - rec[:, 0:3]
    O = R.sym3(rec[:, 9:15])
    J = np.zeros((len(w), 3, 6))
    J[:, 0, 1], J[:, 0, 2] = w[:, 2], -w[:, 1]
    J[:, 1, 0], J[:, 1, 2] = -w[:, 2], w[:, 0]
    J[:, 2, 0], J[:, 2, 1] = w[:, 1], -w[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
    return d, O, J


def linearize(m, points, T, kernel=None, scale=None, neighbours=1):
    """the 32 sums of one scan at T: the upper triangle of sum w J^T O J, sum w J^T O d, n_corr (rows with a pair),
    sum w |d|^2, sum rho(s), sum w, n_pairs"""
    w, row, place = pairs(m, points, T, neighbours)
    d, O, J = terms(m, w, row, place)
    s = np.einsum("nr,nrs,ns->n", d, O, d)
    rho, wt = rho_w(kernel, scale, s)
    Ow = O * wt[:, None, None]
    H = np.einsum("nra,nrs,nsb->ab", J, Ow, J)
    g = np.einsum("nra,nrs,ns->a", J, Ow, d)
    out = np.zeros(SYSTEM)
    out[:21] = H[np.triu_indices(6)]
    out[21:27] = g
    out[27] = len(np.unique(row))
    out[28] = (d * d * wt[:, None]).sum()
    out[29] = np.einsum("nr,nrs,ns->", d, O, d) if kernel is None else rho.sum()
    out[W_SUM], out[N_PAIRS] = wt.sum(), len(row)
    return out


def register_one(m, points, T0, kernel=None, scale=None, neighbours=1, max_iteration=30, relative_fitness=1e-6,
                 relative_rmse=1e-6):
    """map_localize_restatement.register_one with the sums above; also weight_sum and n_pairs at the result"""
    T = np.array(T0, np.float64)
    n = len(points)
    if not np.isfinite(T).all():
        nan = np.nan
        return dict(transform=np.full((4, 4), nan), fitness=nan, rmse=nan, cost=nan, n_correspondences=-1, iterations=0,
                    information=np.full((6, 6), nan), system0=np.full(SYSTEM, nan), weight_sum=nan, n_pairs=-1)
    prev, system0 = None, None
    for rnd in range(max_iteration + 1):
        s = linearize(m, points, T, kernel, scale, neighbours)
        if rnd == 0:
            system0 = s
        nc, ws = s[27], s[W_SUM]
        fitness = nc / n if n > 0 else 0.0
        rmse = np.sqrt(s[28] / ws) if ws > 0 else 0.0
        done = rnd == max_iteration
        if prev is not None and abs(prev[0] - fitness) < relative_fitness and abs(prev[1] - rmse) < relative_rmse:
            done = True
        if done:
            return dict(transform=T, fitness=fitness, rmse=rmse, cost=s[29], n_correspondences=int(nc), iterations=rnd,
                        information=R.full(s), system0=system0, weight_sum=ws, n_pairs=int(s[N_PAIRS]))
        prev = (fitness, rmse)
        if nc > 0:
            H = R.full(s)
            if not GN.regular(H):                                 # no step on a singular system: the written rule
                continue
            T = R.update(np.linalg.solve(H, -s[21:27])) @ T


def register(m, points, offsets, init, **kw):
    """register_one over packed scans -> a dict of stacked arrays"""
    off = np.asarray(offsets, np.int64)
    res = [register_one(m, np.asarray(points)[off[i]:off[i + 1]], init[i], **kw) for i in range(len(off) - 1)]
    return {k: np.stack([np.asarray(r[k]) for r in res]) for k in res[0]} if res else {}
