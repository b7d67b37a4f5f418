"""Float64 numpy / scipy restatement of the stage-2 verifier (retrieval/geometric_verification.py's definitions).

Independent of the kernels: searches go through scipy.spatial.cKDTree or a brute-force distance matrix, sums through
numpy.  ``knn_exact`` and ``path_census`` write out again, in Python, rules and branch conditions that
csrc/nsc_geometry.hip documents; nothing here calls the library."""
import numpy as np
from scipy.spatial import cKDTree

import gauss_newton_restatement as GN

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


def knn_exact(points, k, reverse_ties=False):
    """The kernel's documented rule (TopK: "k smallest (d2, index), ascending; ties to the smaller index"): float64
    squared distances ``x*x + y*y + z*z`` to every row, neighbours ordered by (distance, index).  -> (n, min(k, n))
    indices and (n, min(k+1, n)) squared distances.  ``reverse_ties`` orders equal distances by the larger index
    (the opposite rule; the CPU tests use it to show that an input's ties matter)."""
    p = np.asarray(points, np.float64)
    n = len(p)
    kk = min(k + 1, n)
    idx, d2 = np.zeros((n, kk), np.int64), np.zeros((n, kk))
    order = np.arange(n)[::-1] if reverse_ties else np.arange(n)
    q = p[order]                                                 # a stable sort keeps equal distances in this order
    for a in range(0, n, 512):
        d = p[a:a + 512, None, :] - q[None, :, :]
        dd = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        o = np.argsort(dd, axis=1, kind="stable")[:, :kk]
        idx[a:a + 512], d2[a:a + 512] = order[o], np.take_along_axis(dd, o, 1)
    return idx[:, :min(k, n)], d2


def neighbour_eigenvalues(points, idx):
    """(n, 3) ascending eigenvalues of the neighbourhood covariances of index sets idx (n, k >= 3)"""
    nb = points[idx]
    c = nb - nb.mean(1, keepdims=True)
    return np.linalg.eigvalsh(np.einsum("nki,nkj->nij", c, c) / idx.shape[1])


def separated(points, idx):
    """Rows whose plane normal is defined: the two smallest eigenvalues of the neighbourhood covariance differ by
    more than 1e-3 of the largest.  With fewer than 3 neighbours the covariance is the identity and the normal is
    the x axis by definition (see ``covariances``), so every row counts as separated."""
    if idx.shape[1] < 3:
        return np.ones(len(points), bool)
    w = neighbour_eigenvalues(points, idx)
    return (w[:, 1] - w[:, 0]) > 1e-3 * np.maximum(w[:, 2], 1e-12)


def covariances(points, k=20, eps=1e-3, exact=False, reverse_ties=False, idx=None):
    """``exact``: neighbours by ``knn_exact`` (the kernel's tie rule) instead of the cKDTree.  With fewer than 3
    neighbours the covariance is the identity, whose eigenvectors are the coordinate axes in order: the normal is
    the x axis and the result diag(eps, 1, 1).  ``idx``: neighbour sets already computed."""
    n = len(points)
    if n == 0:
        return np.zeros((0, 3, 3))
    if idx is None:
        idx, _ = knn_exact(points, k, reverse_ties) if exact or reverse_ties else knn(points, k)
    nb = points[idx]                                             # (n, k, 3)
    if idx.shape[1] < 3:
        u = np.tile(np.array([1.0, 0.0, 0.0]), (n, 1))
    else:
        c = nb - nb.mean(1, keepdims=True)
        C = np.einsum("nki,nkj->nij", c, c) / idx.shape[1]
        w, U = np.linalg.eigh(C)                                 # ascending: column 0 = smallest
        u = U[:, :, 0]
    return np.eye(3)[None] - (1 - eps) * np.einsum("ni,nj->nij", u, u)


def ring_census(ds, voxel, k, d2=None):
    """Which search covariance_kernel must run for each row of a down-sampled cloud, from the cloud alone.
    ``small``: m <= knn, one full scan for every row.  Otherwise rings r = 0, 1, .. of voxels are searched while
    (2r+1)^3 <= 2m (``r_max`` is the last such r); after ring r every unseen row is farther than r * voxel, and the
    search stops once the k-th distance found is below that reach (minus the kernel's slack 1e-9 relative + 1e-6 m).
    ``falls_back``: the exact k-th distance is at least r_max * voxel, so no ring can stop the search and the row
    ends in the full scan.  ``stops``: it is below the slackened reach of ring r_max (>= 1), by which ring every
    one of the k nearest has been seen, so the search surely stops in the rings.  Rows in neither set lie within
    the slack of the bound.  ``d2``: knn_exact's squared distances, if already computed."""
    m = len(ds)
    out = dict(m=m, small=m <= k, r_max=-1, falls_back=np.zeros(m, bool), stops=np.zeros(m, bool))
    if m == 0 or out["small"]:
        return out
    r = 0
    while (2 * (r + 1) + 1) ** 3 <= 2 * m:
        r += 1
    out["r_max"] = r
    if d2 is None:
        _, d2 = knn_exact(ds, k)
    dk = np.sqrt(d2[:, k - 1])
    out["falls_back"] = dk >= r * voxel
    reach = r * voxel * (1.0 - 1e-9) - 1e-6
    out["stops"] = (dk < reach) if reach > 0.0 else np.zeros(m, bool)
    return out


def path_census(source_ds, target_ds, params=None, source_d2=None, target_d2=None):
    """The branch each kernel must take on a pair of down-sampled reference clouds: ``source`` / ``target`` =
    ``ring_census`` of each cloud; ``span`` = floor(2 radius / voxel) + 2, the cells per axis the radius can reach;
    ``linearize_brute`` = span^3 > mt, linearize_kernel scans the whole target instead of walking cells."""
    P = dict(DEFAULTS, **(params or {}))
    v, k = P["voxel_size"], P["covariance_knn"]
    span = int(np.floor(2.0 * P["max_correspondence_distance"] / v)) + 2 if len(target_ds) else 1
    return dict(source=ring_census(source_ds, v, k, source_d2), target=ring_census(target_ds, v, k, target_d2),
                span=span, mt=len(target_ds), linearize_brute=span ** 3 > len(target_ds))


def _mix64(x):
    x = np.asarray(x, np.uint64)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xff51afd7ed558ccd)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xc4ceb9fe1a85ec53)
    return x ^ (x >> np.uint64(33))


def table_surely_wraps(points, voxel):
    """The cloud's voxel table (open addressing, 2 slots per input row, home slot mix64(packed key) % capacity,
    linear probing that wraps from the last slot to slot 0) has more keys at home in its last t slots than t, for
    some t: whatever the insertion order, one of them wraps.  -> (wraps, capacity)"""
    raw = np.asarray(points, np.float32)
    cap = 2 * len(raw)
    p = finite_xyz(points)
    if len(p) == 0:
        return False, cap
    lo = p.min(0) - voxel / 2
    key = np.unique(np.floor((p - lo) / voxel).astype(np.int64), axis=0).astype(np.uint64)
    packed = key[:, 0] | (key[:, 1] << np.uint64(21)) | (key[:, 2] << np.uint64(42))
    with np.errstate(over="ignore"):
        home = (_mix64(packed) % np.uint64(cap)).astype(np.int64)
    tail = np.bincount(cap - 1 - home, minlength=cap)           # keys at home t slots before the end
    return bool(np.any(np.cumsum(tail) > np.arange(1, cap + 1))), cap


def skew_neg(v):
    """-[v]x for rows of v."""
    z = np.zeros(len(v))
    return np.stack([np.stack([z, v[:, 2], -v[:, 1]], 1), np.stack([-v[:, 2], z, v[:, 0]], 1),
                     np.stack([v[:, 1], -v[:, 0], z], 1)], 1)


def correspondences(src, tgt, T, radius, exact=False):
    """``exact``: the documented rule written out -- brute-force squared distances, the nearest target row with
    d2 <= radius^2, equal distances to the smaller target index -- instead of the cKDTree (ties arbitrary)."""
    q = src @ T[:3, :3].T + T[:3, 3]
    if len(tgt) == 0 or len(src) == 0:
        return q, np.zeros(0, np.int64), np.zeros(0, np.int64)
    if exact:
        d = q[:, None, :] - tgt[None, :, :]
        dd = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        j = np.argmin(dd, axis=1)                                # the first of equal minima
        ok = dd[np.arange(len(q)), j] <= radius * radius
        return q, np.nonzero(ok)[0], j[ok]
    d, j = cKDTree(tgt).query(q, k=1, distance_upper_bound=radius * (1 + 1e-9))
    ok = np.isfinite(d) & (d <= radius)
    return q, np.nonzero(ok)[0], j[ok]


def linearize(src, tgt, Cs, Ct, T, radius, exact=False):
    """-> dict(H (6,6), g (6), n_corr, sse, info (6,6), fitness, rmse)"""
    q, i, j = correspondences(src, tgt, T, radius, exact)
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


def prepare(points, voxel_size, covariance_knn, epsilon, exact=False):
    p = voxel_down_sample(points, voxel_size)
    return p, covariances(p, covariance_knn, epsilon, exact=exact)


def register(source, target, init=None, exact=False, **params):
    """-> dict(transform, fitness, rmse, n_corr, iterations, information, source_ds, target_ds)"""
    P = dict(DEFAULTS, **params)
    src, Cs = prepare(source, P["voxel_size"], P["covariance_knn"], P["epsilon"], exact)
    tgt, Ct = prepare(target, P["voxel_size"], P["covariance_knn"], P["epsilon"], exact)
    T = np.eye(4) if init is None else np.asarray(init, np.float64).copy()
    radius = P["max_correspondence_distance"]
    lin = linearize(src, tgt, Cs, Ct, T, radius)
    it = 0
    for it in range(1, P["max_iteration"] + 1):
        x = np.zeros(6)
        if lin["n_corr"] > 0 and GN.regular(lin["H"]):           # no step on a singular system: the written rule
            L = np.linalg.cholesky(lin["H"])
            x = np.linalg.solve(L.T, np.linalg.solve(L, -lin["g"]))
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
