"""Float64 numpy / scipy restatement of the stage-2 verifier (retrieval/geometric_verification.py's definitions).

Independent of the kernels: searches go through scipy.spatial.cKDTree, sums through numpy."""
import numpy as np
from scipy.spatial import cKDTree

DEFAULTS = dict(voxel_size=0.5, max_correspondence_distance=1.0, max_iteration=30, relative_fitness=1e-6,
                relative_rmse=1e-6, covariance_knn=20, epsilon=1e-3)


def finite_xyz(points):
    p = np.asarray(points, np.float32).reshape(-1, np.asarray(points).shape[-1] if np.asarray(points).size else 3)
    p = p[:, :3].astype(np.float64)
    return p[np.all(np.isfinite(p), 1)]


def voxel_down_sample(points, voxel):
    """Centroid per voxel, voxels in the order of their first row."""
    p = finite_xyz(points)
    if len(p) == 0:
        return np.zeros((0, 3))
    lo = p.min(0) - voxel / 2
    key = np.floor((p - lo) / voxel).astype(np.int64)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    row = rank[inv]
    out = np.zeros((len(first), 3))
    np.add.at(out, row, p)
    return out / np.bincount(row, minlength=len(first))[:, None]


def knn(points, k):
    """(n, min(k, n)) neighbour indices and (n, min(k+1, n)) distances (the (k+1)-th shows ties at the edge)."""
    n = len(points)
    kk = min(k + 1, n)
    d, i = cKDTree(points).query(points, k=kk)
    d, i = d.reshape(n, kk), i.reshape(n, kk)
    return i[:, :min(k, n)], d


def covariances(points, k=20, eps=1e-3):
    n = len(points)
    if n == 0:
        return np.zeros((0, 3, 3))
    idx, _ = knn(points, k)
    nb = points[idx]                                             # (n, k, 3)
    if idx.shape[1] < 3:
        C = np.tile(np.eye(3), (n, 1, 1))
    else:
        c = nb - nb.mean(1, keepdims=True)
        C = np.einsum("nki,nkj->nij", c, c) / idx.shape[1]
    w, U = np.linalg.eigh(C)                                     # ascending: column 0 = smallest
    u = U[:, :, 0]
    return np.eye(3)[None] - (1 - eps) * np.einsum("ni,nj->nij", u, u)


def skew_neg(v):
    """-[v]x for rows of v."""
    z = np.zeros(len(v))
    return np.stack([np.stack([z, v[:, 2], -v[:, 1]], 1), np.stack([-v[:, 2], z, v[:, 0]], 1),
                     np.stack([v[:, 1], -v[:, 0], z], 1)], 1)


def correspondences(src, tgt, T, radius):
    q = src @ T[:3, :3].T + T[:3, 3]
    if len(tgt) == 0 or len(src) == 0:
        return q, np.zeros(0, np.int64), np.zeros(0, np.int64)
    d, j = cKDTree(tgt).query(q, k=1, distance_upper_bound=radius * (1 + 1e-9))
    ok = np.isfinite(d) & (d <= radius)
    return q, np.nonzero(ok)[0], j[ok]


def linearize(src, tgt, Cs, Ct, T, radius):
    """-> dict(H (6,6), g (6), n_corr, sse, info (6,6), fitness, rmse)"""
    q, i, j = correspondences(src, tgt, T, radius)
    R = T[:3, :3]
    n = len(i)
    out = dict(n_corr=n, H=np.zeros((6, 6)), g=np.zeros(6), sse=0.0, info=np.zeros((6, 6)))
    if n:
        d = q[i] - tgt[j]
        M = Ct[j] + np.einsum("ab,nbc,dc->nad", R, Cs[i], R)
        W = np.linalg.inv(M)
        J = np.concatenate([skew_neg(q[i]), np.tile(np.eye(3), (n, 1, 1))], 2)      # (n, 3, 6)
        WJ = W @ J
        out["H"] = np.einsum("nka,nkb->ab", J, WJ)
        out["g"] = np.einsum("nka,nk->a", WJ, d)
        out["sse"] = float((d * d).sum())
        G = np.concatenate([skew_neg(tgt[j]), np.tile(np.eye(3), (n, 1, 1))], 2)
        out["info"] = np.einsum("nka,nkb->ab", G, G)
    out["fitness"] = n / len(src) if len(src) else 0.0
    out["rmse"] = float(np.sqrt(out["sse"] / n)) if n else 0.0
    return out


def delta_transform(x):
    a, b, g = x[:3]
    ca, sa, cb, sb, cg, sg = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(g), np.sin(g)
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    D = np.eye(4)
    D[:3, :3] = Rz @ Ry @ Rx
    D[:3, 3] = x[3:]
    return D


def prepare(points, voxel_size, covariance_knn, epsilon):
    p = voxel_down_sample(points, voxel_size)
    return p, covariances(p, covariance_knn, epsilon)


def register(source, target, init=None, **params):
    """-> dict(transform, fitness, rmse, n_corr, iterations, information, source_ds, target_ds)"""
    P = dict(DEFAULTS, **params)
    src, Cs = prepare(source, P["voxel_size"], P["covariance_knn"], P["epsilon"])
    tgt, Ct = prepare(target, P["voxel_size"], P["covariance_knn"], P["epsilon"])
    T = np.eye(4) if init is None else np.asarray(init, np.float64).copy()
    radius = P["max_correspondence_distance"]
    lin = linearize(src, tgt, Cs, Ct, T, radius)
    it = 0
    for it in range(1, P["max_iteration"] + 1):
        ok = lin["n_corr"] > 0
        x = np.zeros(6)
        if ok:
            try:
                L = np.linalg.cholesky(lin["H"])
                x = np.linalg.solve(L.T, np.linalg.solve(L, -lin["g"]))
            except np.linalg.LinAlgError:
                x = np.zeros(6)
        T = delta_transform(x) @ T
        prev = lin
        lin = linearize(src, tgt, Cs, Ct, T, radius)
        if abs(prev["fitness"] - lin["fitness"]) < P["relative_fitness"] and \
                abs(prev["rmse"] - lin["rmse"]) < P["relative_rmse"]:
            break
    return dict(transform=T, fitness=lin["fitness"], rmse=lin["rmse"], n_corr=lin["n_corr"], iterations=it,
                information=lin["info"], source_ds=src, target_ds=tgt)


def pose_error(T, T_true):
    """(translation error m, rotation error rad)"""
    E = np.linalg.inv(T_true) @ T
    return float(np.linalg.norm(E[:3, 3])), float(np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1)))
