"""Seeded input families for the GICP kernels (csrc/nsc_geometry.hip): small clouds, each built to reach one search
path, parameter range or batch shape, so that the brute-force float64 restatement (tests/gicp_restatement.py) stays
cheap.  CPU only; every cloud is an (n, 4) float32 array (xyz + a column the kernels ignore).

tests/test_gicp_families_cpu.py checks, without a GPU, that every family with every seed used reaches the branch it
is named after (``gicp_restatement.path_census``); tests/test_gicp_paths_gpu.py runs them on the device."""
import numpy as np

import gicp_restatement as G

MOTION = np.array([0.01, -0.015, 0.03, 0.25, -0.2, 0.05])       # a small known motion: 0.03 rad, about 0.3 m


def _rows(xyz):
    xyz = np.asarray(xyz, np.float64)
    return np.concatenate([xyz, np.zeros((len(xyz), 1))], 1).astype(np.float32)


def moved(cloud, T):
    """rows of ``cloud`` under the rigid transform T (float64, then rounded to float32)"""
    c = np.asarray(cloud, np.float64)
    return _rows(c[:, :3] @ T[:3, :3].T + T[:3, 3])


def _height(x, y, ext=20.0):
    return 0.8 * np.sin(0.5 * x) + 0.6 * np.cos(0.4 * y) + 0.05 * x * y / ext


def surface(seed, n=4000, ext=20.0, noise=0.02, shift=(0.0, 0.0, 0.0), relief=0.0):
    """Rows on a smooth height field over ext x ext metres with ``noise`` m of noise, then shifted.  Dense: the ring
    search stops early, linearize walks cells.  ``relief`` adds metre-scale bumps, which pin a small patch in place."""
    rng = np.random.default_rng([seed, 1])
    xy = rng.uniform(-ext / 2, ext / 2, (n, 2))
    z = _height(xy[:, 0], xy[:, 1]) + relief * np.sin(2.1 * xy[:, 0]) * np.cos(1.7 * xy[:, 1]) + rng.normal(0, noise, n)
    return _rows(np.c_[xy, z] + np.asarray(shift, np.float64))


def surface_pair(seed, n=4000, shift=(0.0, 0.0, 0.0)):
    """(A, B, T): two samplings of one surface, B moved by T = delta_transform(MOTION) about the shifted origin's
    frame; registering A onto B recovers T."""
    A = surface(seed, n, shift=shift)
    B0 = surface(seed + 1000, n, shift=shift)
    T = G.delta_transform(MOTION)
    return A, moved(B0, T), T


SHIFT_FAR = (1000.0, -2000.0, 50.0)
SHIFT_NEGATIVE = (-500.0, -700.0, -300.0)                         # every coordinate negative


def sparse(seed, n=400, extent=200.0):
    """Uniform in a cube: at voxel 0.5 every row's 20th neighbour is tens of metres away, so every row's ring
    search falls back to the full scan."""
    rng = np.random.default_rng([seed, 2])
    return _rows(rng.uniform(-extent / 2, extent / 2, (n, 3)))


FAR_ROW = 4.0e5        # metres: 2.0e6 voxels of 0.2 m from the surface, under the 21-bit key range (2 097 151)


def mixed(seed, n=2000):
    """A surface plus six isolated rows 150 m .. 4e5 m away: rows of both ring-search kinds in one cloud, and a
    voxel coordinate just inside the key range.  The far rows sit in the middle of the row order."""
    rng = np.random.default_rng([seed, 3])
    s = surface(seed, n)
    far = np.array([[150.0, 0, 0], [0, -300.0, 20.0], [-600.0, 600.0, 5.0], [900.0, 40.0, -3.0], [30.0, 1500.0, 0],
                    [FAR_ROW, 0.5 * FAR_ROW, 10.0]]) + rng.uniform(0, 1, (6, 3))
    at = n // 2
    return np.concatenate([s[:at], _rows(far), s[at:]])


def small_target(seed, side=4.0, n_target=600, n_source=3000, relief=0.5):
    """(A, B, T): the target is a side x side patch of the surface, which keeps fewer voxels than the span^3 cells a
    correspondence search can reach (linearize's full-scan branch) but more than knn; the source covers it."""
    T = G.delta_transform(MOTION)
    A = surface(seed, n_source, ext=10.0, relief=relief)
    B0 = surface(seed + 1000, n_target, ext=side, relief=relief)
    return A, moved(B0, T), T


def lattice(seed, n=40, voxel=0.5):
    """n x n rows at multiples of ``voxel``, one per voxel, on a stepped sheet (heights 0, 1, 2 voxels) in a seeded
    row order.  Squared distances are small integers times voxel^2: equal distances at the k-th place are the rule,
    and which of the equal rows is taken changes the covariance.  All arithmetic on these rows is exact in float32
    and float64."""
    rng = np.random.default_rng([seed, 4])
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    h = np.round(1.0 + np.sin(0.45 * i + 0.2) * np.cos(0.35 * j)).astype(np.int64)      # 0, 1, 2
    h = np.where(rng.random((n, n)) < 0.15, (h + 1) % 3, h)
    xyz = np.stack([i, j, h], -1).reshape(-1, 3) * voxel + np.array([2.0, -3.0, 1.0])
    return _rows(xyz[rng.permutation(n * n)])


def faces_and_duplicates(seed, voxel=0.5, crowd=30000):
    """Rows exactly on voxel faces (min + voxel / 2 + j * voxel: the key is floor of an exact integer), each
    repeated, rows strictly inside voxels, and one voxel holding ``crowd`` rows.  The first row is the cloud's
    minimum in every axis, so the min bound is known: -3 - voxel / 2."""
    rng = np.random.default_rng([seed, 5])
    lo = -3.0
    corner = np.array([[lo, lo, lo]])
    faces = lo + voxel / 2 + rng.integers(0, 12, (300, 3)) * voxel
    faces = np.concatenate([faces, faces[rng.integers(0, 300, 200)]])                   # repeated rows
    inside = lo + rng.uniform(0.01, 6.0, (500, 3))
    cell = lo + voxel / 2 + np.array([3, 7, 5]) * voxel
    crowded = cell + rng.uniform(0.01, voxel - 0.01, (crowd, 3))
    body = np.concatenate([faces, inside, crowded])
    return _rows(np.concatenate([corner, body[rng.permutation(len(body))], faces[:50]]))


def many_small(seed, P=300):
    """-> (sources, targets): P pairs of 0 .. 300 rows each.  Three in ten clouds have 1 .. 8 rows (tables of 2 .. 16
    slots); an empty, an all-NaN, a one-row and a two-row cloud sit in the middle of each list.  A pair's clouds
    sample one 3 m patch of the surface, the target moved by a few centimetres.  Every coordinate is at least 0.5 m
    in magnitude, where float32 is exact in the kernel's fixed-point unit of 2^-24 m: in pairs this small the
    gradient terms are sums that cancel, and the rounding of smaller coordinates (up to 2^-25 m) would show in them
    at 1e-5 relative."""
    rng = np.random.default_rng([seed, 6])
    T = G.delta_transform(0.2 * MOTION)

    def cloud(n, centre):
        xy = rng.uniform(-1.5, 1.5, (n, 2)) + centre
        return _rows(np.c_[xy, 3.0 + _height(xy[:, 0], xy[:, 1]) + rng.normal(0, 0.02, n)])

    def size():
        return int(rng.integers(1, 9)) if rng.random() < 0.3 else int(rng.integers(9, 301))
    sources, targets = [], []
    for p in range(P):
        centre = rng.uniform(2.5, 14.0, 2)
        sources.append(cloud(size(), centre))
        targets.append(moved(cloud(size(), centre), T))
    mid = P // 2
    nan = np.full((5, 4), np.nan, np.float32)
    empty = np.zeros((0, 4), np.float32)
    sources[mid], targets[mid + 1] = empty, empty
    sources[mid + 2], targets[mid + 3] = nan, nan
    sources[mid + 4], targets[mid + 5] = sources[mid + 4][:1], targets[mid + 5][:1]
    sources[mid + 6], targets[mid + 7] = sources[mid + 6][:2], targets[mid + 7][:2]
    return sources, targets


def tiny_clouds(seed, n=1100):
    """n clouds of one to five rows"""
    rng = np.random.default_rng([seed, 7])
    return [_rows(rng.uniform(-2, 2, (int(rng.integers(1, 6)), 3))) for _ in range(n)]


# ----------------------------------------------------------------------------------------------------------------
# the cases both test files run: (family, seed, parameters, stride), and their float64 reference
# ----------------------------------------------------------------------------------------------------------------
def _pair_of(cloud_fn, seed, **kw):
    """(A, B, T) from a one-cloud family: B is another seed's cloud, moved"""
    T = G.delta_transform(MOTION)
    return cloud_fn(seed, **kw), moved(cloud_fn(seed + 1000, **kw), T), T


def _sparse_pair(seed, **kw):
    """the target is the source itself, moved: uniform rows of two seeds would share no correspondence"""
    T = G.delta_transform(MOTION)
    A = sparse(seed, **kw)
    return A, moved(A, T), T


def _p(voxel, knn, eps, radius):
    return dict(voxel_size=voxel, covariance_knn=knn, epsilon=eps, max_correspondence_distance=radius)


# id -> (builder of (A, B, T_true), parameters, stride of the packed rows).  span = floor(2 radius / voxel) + 2.
STAGE_CASES = {
    "surface-v0.5-k20":  (lambda: surface_pair(0, n=3000), _p(0.5, 20, 1e-3, 1.0), 4),              # span 6: the defaults
    "surface-v0.2-k32":  (lambda: surface_pair(1, n=2000), _p(0.2, 32, 1e-3, 1.0), 3),      # span 12
    "surface-v1.0-k5":   (lambda: surface_pair(2), _p(1.0, 5, 1e-2, 2.5), 4),               # span 7
    "surface-v2.0-k3":   (lambda: surface_pair(3), _p(2.0, 3, 1e-3, 2.5), 3),               # span 4
    "surface-v0.5-k1":   (lambda: surface_pair(4), _p(0.5, 1, 1e-3, 0.3), 4),               # span 3, identity C
    "surface-v0.5-k2":   (lambda: surface_pair(5), _p(0.5, 2, 1e-2, 0.3), 3),               # span 3, identity C
    "surface-v0.2-r3":   (lambda: surface_pair(6, n=2000), _p(0.2, 20, 1e-3, 3.0), 4),      # span 32
    "sparse-400":        (lambda: _sparse_pair(0), _p(0.5, 20, 1e-3, 1.0), 4),
    "sparse-1200":       (lambda: _sparse_pair(1, n=1200, extent=50.0), _p(0.5, 20, 1e-3, 1.0), 3),
    "far-v0.5-k20":      (lambda: surface_pair(7, shift=SHIFT_FAR), _p(0.5, 20, 1e-3, 1.0), 4),
    "negative-v1.0-k20": (lambda: surface_pair(8, shift=SHIFT_NEGATIVE), _p(1.0, 20, 1e-2, 2.5), 3),
    "mixed-v0.5-k20":    (lambda: _pair_of(mixed, 0), _p(0.5, 20, 1e-3, 1.0), 4),
    "mixed-v0.2-k12":    (lambda: _pair_of(mixed, 1), _p(0.2, 12, 1e-3, 0.6), 3),            # key range, span 8
    "small-target":      (lambda: small_target(0), _p(0.5, 20, 1e-3, 1.0), 4),
}

# what path_census must say of each case: every row of both clouds "falls_back" / "stops", both kinds, or the
# linearize branch
CLAIMS = {"sparse-400": "falls_back", "sparse-1200": "falls_back", "mixed-v0.5-k20": "both",
          "mixed-v0.2-k12": "both", "surface-v0.2-k32": "both", "small-target": "linearize_brute",
          "surface-v0.2-r3": "linearize_brute"}

# id -> (builder, parameters, (translation bar m, rotation bar rad) on the recovered motion).  The 20 m surfaces
# take the project's bars for revisits (tests/test_gicp_cpu.py); a 4 m patch pins the rotation weakly -- the float64
# restatement itself ends 1.5 cm and 1.26 degrees from the truth -- so its rotation bar is 2 degrees.
_BARS = (0.05, np.deg2rad(0.25))
END_TO_END = {
    "surface-default":  (lambda: surface_pair(0), {}, _BARS),
    "surface-fine":     (lambda: surface_pair(0), dict(voxel_size=0.25, max_correspondence_distance=0.6,
                                                       covariance_knn=12), _BARS),
    "surface-coarse":   (lambda: surface_pair(0), dict(voxel_size=1.0, max_correspondence_distance=2.5,
                                                       covariance_knn=32, epsilon=1e-2), _BARS),
    "small-target":     (lambda: small_target(0), {}, (0.05, np.deg2rad(2.0))),
}

T_FIX_OFFSET = np.array([0.004, -0.003, 0.005, 0.05, -0.03, 0.02])     # the fixed transform: near the truth, not at it


def stage_case(name):
    build, params, stride = STAGE_CASES[name]
    A, B, T = build()
    c = np.eye(4)
    c[:3, 3] = np.median(A[:, :3].astype(np.float64), 0)         # the offset turns about the cloud, not the origin
    return A, B, T @ c @ G.delta_transform(T_FIX_OFFSET) @ np.linalg.inv(c), params, stride


def cloud_reference(cloud, params):
    """-> dict(ds, idx, d2, gap, cov (n,3,3), sep): the down-sampled cloud, its exact neighbour sets, the smallest
    distance (m) between a row's k-th and (k+1)-th neighbour, the exact-rule covariances and the rows whose normal
    is defined"""
    k = params["covariance_knn"]
    ds = G.voxel_down_sample(cloud, params["voxel_size"])
    idx, d2 = G.knn_exact(ds, k)
    gap = np.inf
    if d2.shape[1] > idx.shape[1]:
        d = np.sqrt(d2)
        gap = float((d[:, -1] - d[:, -2]).min())
    return dict(ds=ds, idx=idx, d2=d2, gap=gap, cov=G.covariances(ds, k, params["epsilon"], idx=idx),
                sep=G.separated(ds, idx))


def radius_margin(src, tgt, T, radius):
    """smallest | |T s - t| - radius | over rows s and their nearest target row t, however far"""
    from scipy.spatial import cKDTree
    if len(src) == 0 or len(tgt) == 0:
        return np.inf
    d, _ = cKDTree(tgt).query(src @ T[:3, :3].T + T[:3, 3], k=1)
    return float(np.abs(d - radius).min())
