"""Constructed inputs on which the 6x6 Gauss-Newton system of a registration round is singular, or regular but badly
conditioned, for GICP (csrc/nsc_geometry.hip) and scan-to-map registration (csrc/nsc_localize.hip), whose rounds both
end in gn_solve6 (csrc/nsc_gauss_newton.h).  tests/test_registration_degenerate_cpu.py proves from the restatements
alone that each input is what its name claims; tests/test_registration_degenerate_gpu.py runs the kernels on them.

The contract: at a round whose reference system H = sum J^T W J is singular the step is the identity, so the transform
that comes back is the initial one bit for bit and, with max_iteration >= 1, iterations == 1.  A regular system's step
is taken.  "Singular" is decided here, by construction: a singular case carries analytic null vectors n with J n = 0 for
every row, whatever the weights W are.  With J = [-[q]x | I] at a transformed source row q and n = (a, b),
J n = a x q + b:
  rows q on the line o + t d    n = (d, o x d)                      a x q + b = d x (q - o) = 0
  one row q                     n = (e, q x e), e over a basis      e x q + q x e = 0
  two rows                      the line through them

Every GICP cloud that has to be exactly collinear lies on the lattice of 2^-6 m: its rows are exact in float32, in the
kernel's fixed-point unit of 2^-24 m and in float64, and so are their differences.  Rows are 0.7 m apart (45 lattice
steps), the voxel is 0.5 m, and each case asserts that every row is its own voxel (``own_voxels``)."""
import functools

import numpy as np

import gicp_clouds as F
import gicp_restatement as G
import map_localize_cases as K
import map_localize_restatement as R

UNIT = 2.0 ** -6                         # m: the lattice of the collinear clouds
STEP_NORM = (44.2, 45.8)                 # lattice steps between two rows of a line: 0.69 .. 0.716 m
SHIFT = np.array([2.0, -1.0, 3.0]) * UNIT            # the target of a line is the line moved by this: 5.8 cm
LINE_SEEDS = tuple(range(8))
REACH = 20.0                             # m: a line's middle row is up to this far from the origin on each axis
PARAMS = dict(G.DEFAULTS)                # voxel 0.5 m, 20 neighbours, epsilon 1e-3, radius 1.0 m


def _rows(xyz):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    return np.concatenate([xyz, np.zeros((len(xyz), 1))], 1).astype(np.float32)


def own_voxels(cloud, voxel=0.5):
    """every row of the cloud survives down-sampling as its own voxel, in its place"""
    ds = G.voxel_down_sample(cloud, voxel)
    return len(ds) == len(cloud) and np.array_equal(ds, np.asarray(cloud)[:, :3].astype(np.float64))


def lattice_line(seed, n):
    """n rows o + i s (i = -(n // 2) ..) on the 2^-6 m lattice, s in a general direction (no component under 8 steps)
    -> (xyz (n,3) float64, a point o of the line, its unit direction d).  Candidates are drawn until every row of the
    line and of the line moved by SHIFT is its own 0.5 m voxel."""
    rng = np.random.default_rng([seed, 11])
    while True:
        s = rng.integers(-45, 46, 3).astype(np.float64)
        o = rng.integers(-int(REACH / UNIT), int(REACH / UNIT) + 1, 3).astype(np.float64) * UNIT
        if not (STEP_NORM[0] <= np.linalg.norm(s) <= STEP_NORM[1]) or np.abs(s).min() < 8:
            continue
        xyz = o + np.arange(-(n // 2), n - n // 2)[:, None] * (s * UNIT)
        if own_voxels(_rows(xyz)) and own_voxels(_rows(xyz + SHIFT)):
            return xyz, o, s / np.linalg.norm(s)


def line_null(o, d):
    return np.concatenate([d, np.cross(o, d)])[None]


def point_null(q):
    return np.stack([np.concatenate([e, np.cross(q, e)]) for e in np.eye(3)])


def _case(name, source, target, singular, null=None, line=None, init=None, rank=None):
    return dict(name=name, source=source, target=target, singular=singular, null=null, line=line, rank=rank,
                init=np.eye(4) if init is None else init)


@functools.lru_cache(maxsize=None)
def spread_target():
    """about 200 rows of a 6 m patch of gicp_clouds' surface with metre-scale relief, every coordinate above 0.5 m (exact
    in the fixed-point unit)"""
    return F.surface(21, 260, ext=6.0, relief=0.5, shift=(6.0, 5.0, 4.0))


def few_rows(n):
    """``one_row`` / ``two_rows``: n of the spread target's rows, moved by 3 cm, against the whole target"""
    tgt = spread_target()
    pick = tgt[[17, 140][:n], :3].astype(np.float64) + np.array([0.02, -0.02, 0.01])
    src = _rows(pick)
    q = src[:, :3].astype(np.float64)
    if n == 1:
        null = point_null(q[0])
    else:
        d = (q[1] - q[0]) / np.linalg.norm(q[1] - q[0])
        null = line_null(q[0], d)
    return _case(("one_row", "two_rows")[n - 1], src, tgt, True, null, rank=(3, 5)[n - 1])


def line_axis():
    """40 rows on the x axis through the origin: the first rotation column of every J is exactly zero"""
    xyz = np.arange(-20, 20)[:, None] * np.array([45.0, 0.0, 0.0]) * UNIT
    return _case("line_axis", _rows(xyz), _rows(xyz + SHIFT), True, line_null(np.zeros(3), np.array([1.0, 0, 0])),
                 line=(np.zeros(3), np.array([1.0, 0, 0])), rank=5)


def line_general(seed, n):
    xyz, o, d = lattice_line(seed, n)
    return _case(f"line_general-{n}-{seed}", _rows(xyz), _rows(xyz + SHIFT), True, line_null(o, d), line=(o, d), rank=5)


def line_plus_one(off, seed=0, n=40):
    """line_general and one row past the line's end, ``off`` m to its side: rank 6, barely"""
    xyz, o, d = lattice_line(seed, n)
    side = np.cross(d, [0.0, 0.0, 1.0])
    extra = np.round((xyz[-1] + (xyz[-1] - xyz[-2]) + off * side / np.linalg.norm(side)) / UNIT) * UNIT
    xyz = np.concatenate([xyz, extra[None]])
    return _case(f"line_plus_one-{off}", _rows(xyz), _rows(xyz + SHIFT), False)


PLANE_CENTRE = np.array([30.0, -40.0, 3.0])                      # 50 m from the origin


def plane_far():
    """17 x 18 rows of the plane z = 3, 0.7 m apart with +-0.05 m of in-plane jitter (axis gaps of 0.6 m: one row per
    voxel), 50 m from the origin, against itself turned by 0.34 degrees about its centre and moved by 6 cm"""
    rng = np.random.default_rng(31)
    i, j = np.meshgrid(np.arange(17) - 8.0, np.arange(18) - 8.5, indexing="ij")
    xy = np.stack([i, j], -1).reshape(-1, 2) * 0.7 + rng.uniform(-0.05, 0.05, (17 * 18, 2))
    src = _rows(np.c_[xy, np.zeros(len(xy))] + PLANE_CENTRE)
    c = np.eye(4)
    c[:3, 3] = PLANE_CENTRE
    T = c @ G.delta_transform(0.2 * F.MOTION) @ np.linalg.inv(c)
    out = _case("plane_far", src, F.moved(src, T), False)
    out["truth"] = T
    return out


@functools.lru_cache(maxsize=None)
def gicp_cases():
    """name -> case, in the order of the mixed batch: singular pairs at both ends and in the middle"""
    lines = [line_general(s, n) for n in (5, 40) for s in LINE_SEEDS]
    order = ([few_rows(1), lines[0], plane_far(), line_plus_one(1.0)] + lines[1:8] + [line_axis(), few_rows(2)] +
             lines[8:15] + [line_plus_one(0.1), lines[15]])
    return {c["name"]: c for c in order}


SINGULAR = ("one_row", "two_rows", "line_axis") + tuple(f"line_general-{n}-{s}" for n in (5, 40) for s in LINE_SEEDS)
REGULAR = ("plane_far", "line_plus_one-1.0", "line_plus_one-0.1")
LINES_40 = tuple(f"line_general-40-{s}" for s in LINE_SEEDS)


def hessian(s21):
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = np.asarray(s21)[:21]
    return H + np.triu(H, 1).T


def null_residual(H, null):
    """max over the case's null vectors of |H n| / (||H||_2 |n|)"""
    return max(float(np.linalg.norm(H @ n) / (np.linalg.norm(H, 2) * np.linalg.norm(n))) for n in null)


def gicp_reference(case, cov=None):
    """the restatement's down-sampled clouds, covariances (``cov`` = (source, target) to take them from elsewhere) and
    linearisation at the case's initial transform"""
    src, tgt = G.voxel_down_sample(case["source"], 0.5), G.voxel_down_sample(case["target"], 0.5)
    if cov is None:
        cov = (G.covariances(src, 20, 1e-3, exact=True), G.covariances(tgt, 20, 1e-3, exact=True))
    return src, tgt, cov, G.linearize(src, tgt, cov[0], cov[1], case["init"], 1.0, exact=True)


def normal_of(C, eps=1e-3):
    """(n,3,3) matrices U diag(eps, 1, 1) U^T -> their eigenvalues (n,3) ascending and the eps-eigenvectors (n,3)"""
    w, U = np.linalg.eigh(C)
    return w, U[:, :, 0]


# ---- scan to map: on map_localize_cases.scene() and its map ------------------------------------------------------------

WALL_START = np.array([9.13, -9.63, 0.27])                       # on the scene's wall x = 9.3 (1.0 m voxels x in [9, 10))
WALL_STEP = np.array([0.028, 0.6953, 0.071])                     # 0.7 m a row, 0.8 m of x over the wall's 20 m
ROBUST = ("cauchy", 3.0, 7)                                      # map_robust_cases.WIDE_ROBUST: a kernel and face neighbours


def _scan_of(world, T):
    """float64 scan rows whose points under T are ``world`` to rounding"""
    return (world - T[:3, 3]) @ T[:3, :3]


@functools.lru_cache(maxsize=None)
def scan_cases():
    """name -> dict(scan (n,3) float64, init, singular, null, rank): ``scan_one_row``, ``scan_line-5`` / ``-40`` along
    the wall x = 9.3 (40 rows run 28 m: the last ones leave the map), and two of the scene's scans.  The null vectors
    are about the transformed rows as the restatement computes them."""
    s = K.scene()
    m = K.scene_reference()["map"]
    out = {}
    T1 = s["init"][1]
    b = s["scans"][2000:4000].astype(np.float64)
    ok = (R.lookup(m, b, T1)[1] >= 0) & R.keep_off_faces(m, b, T1, 1e-3)
    row = b[np.nonzero(ok)[0][:1]]
    out["scan_one_row"] = dict(scan=row, init=T1, singular=True, null=point_null(R.transform_rows(row, T1)[0]), rank=3)
    d = WALL_STEP / np.linalg.norm(WALL_STEP)
    for n, T in ((5, s["init"][2]), (40, s["init"][5])):
        world = WALL_START + np.arange(n)[:, None] * WALL_STEP
        scan = _scan_of(world, T)
        out[f"scan_line-{n}"] = dict(scan=scan, init=T, singular=True, rank=5,
                                     null=line_null(R.transform_rows(scan, T)[0], d))
    for i in (0, 1):
        out[f"scene-{i}"] = dict(scan=s["scans"][2000 * i:2000 * (i + 1)].astype(np.float64), init=s["init"][i],
                                 singular=False, null=None, rank=6)
    return out


SCAN_BATCH = ("scan_one_row", "scene-0", "scan_line-5", "scene-1", "scan_line-40")
SCAN_SINGULAR = ("scan_one_row", "scan_line-5", "scan_line-40")
