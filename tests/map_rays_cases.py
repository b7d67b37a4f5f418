"""Constructed inputs of tests/test_map_rays_cpu.py and tests/test_map_rays_gpu.py.

(a) ``hand_map`` and ``hand_cases``: a map of a few voxels whose Gaussians are known -- thin planes and wide blobs on a
    lattice of 1/64 m -- and rays whose voxels and crossings are derived by hand in the comments beside them.  Every
    decision of a case is far from its threshold (s below 5 or above 25 against gate^2 = 9) or exact (coordinates are
    dyadic, so every face time is exact), so the counts hold for the restatement's records and for the device's alike.
(b) ``scene``: map_localize_cases' surfaces and a box that stands in clouds 0-2 and has left in clouds 3-5, seen from the
    six map poses, sampled WITH occlusion: a sample is kept only if the segment from the sensor to it meets no rectangle
    and not the box before its end.  Without that the scene contradicts itself (every wall is looked through by the samples
    behind it).  ``scene_result`` runs the restatement on it once per voxel size."""
import functools

import numpy as np

import map_insert_restatement as IR
import map_localize_cases as K
import map_localize_restatement as R
import map_rays_restatement as RR

LAT = np.array([-28, -9, 9, 28]) / 64.0                 # offsets of a lattice point from the voxel's centre
VAR = (28 ** 2 + 9 ** 2) / 2.0 / 64.0 ** 2              # the variance along an axis the lattice spans: 0.1056 m^2
THIN = float(np.sqrt(1e-2 * VAR))                       # sigma across a plane, from eigen_ratio = 1e-2: 0.0325 m


def plane(v):
    """16 rows in voxel v on the plane x = v_x + 0.5: sigma THIN along x, sqrt(VAR) along y and z"""
    y, z = np.meshgrid(LAT, LAT, indexing="ij")
    return np.stack([np.full(16, v[0] + 0.5), v[1] + 0.5 + y.ravel(), v[2] + 0.5 + z.ravel()], 1)


def blob(v):
    """64 rows in voxel v on the lattice: sigma sqrt(VAR) = 0.325 m along every axis, so a ray crosses iff it comes within
    0.975 m of the centre -- every ray through the voxel does"""
    x, y, z = np.meshgrid(LAT, LAT, LAT, indexing="ij")
    return np.stack([v[0] + 0.5 + x.ravel(), v[1] + 0.5 + y.ravel(), v[2] + 0.5 + z.ravel()], 1)


PLANES = [(i, 0, 0) for i in range(2, 9)] + [(2, 0, 16)]
BLOBS = [(2, 1, 4), (3, 1, 4), (1, 1, 4), (3, 0, 4),            # one zero component: the first two are on the path
         (1, 0, 8), (2, 1, 8), (0, 1, 8), (1, 2, 8),            # diagonal ties: the first two are on the path
         (2, 1, 13), (2, 0, 13), (2, 1, 12), (2, 0, 12)]        # a ray along an edge: the first is on the path


def hand_map():
    """-> (points (N,3) float64, offsets, poses) of the map of voxel 1.0 m: one cloud under the identity"""
    pts = np.concatenate([plane(v) for v in PLANES] + [blob(v) for v in BLOBS])
    return pts, np.array([0, len(pts)], np.int64), np.eye(4)[None]


def _sensor(o):
    T = np.eye(4)
    T[:3, 3] = o
    return T


def _case(name, sensors, rows, crossed, stats, pose_ids=None, **ray):
    """``rows``: per sensor the rows relative to it (the rotation is the identity)"""
    pts = np.concatenate([np.asarray(r, np.float64).reshape(-1, 3) for r in rows])
    off = np.concatenate([[0], np.cumsum([len(np.asarray(r).reshape(-1, 3)) for r in rows])]).astype(np.int64)
    return dict(name=name, points=pts, offsets=off, poses=np.stack([_sensor(o) for o in sensors]), pose_ids=pose_ids,
                ray=ray, crossed=crossed, stats=stats)


def hand_cases():
    """-> list of dicts: name, points, offsets, poses, pose_ids, ray (keywords of the cast), crossed {voxel: count} (every
    other voxel 0) and the eight stats"""
    on = lambda vs: {v: 1 for v in vs}                   # noqa: E731
    row = [(i, 0, 0) for i in range(9)]
    c = []
    # x runs from 0.5 to 8.5 - 1.25 = 7.25 through the planes at 2.5 .. 6.5; voxel 7 is examined over [7, 7.25], 0.25 m =
    # 7.7 sigma in front of its plane; voxel 8, the row's own, is never reached: voxels 0 .. 7
    c.append(_case("perpendicular", [(0.5, 0.5, 0.5)], [[(8, 0, 0)]], on(row[2:7]), [1, 0, 0, 0, 0, 8, 5, 0], end_margin=1.25))
    # without a margin the ray runs into its own voxel and onto plane 8 (s = 0 there): the end voxel is not counted
    c.append(_case("end voxel", [(0.5, 0.5, 0.5)], [[(8, 0, 0)]], on(row[2:8]), [1, 0, 0, 0, 0, 9, 6, 0], end_margin=0.0))
    # from x = 0.5 + 3.25 = 3.75 (behind plane 3 by 7.7 sigma) to x = 0.5 + 5.25 = 5.75 (in front of plane 6): voxels 3, 4, 5
    c.append(_case("clipped", [(0.5, 0.5, 0.5)], [[(8, 0, 0)]], on(row[4:6]), [1, 0, 0, 0, 0, 3, 2, 0], min_range=3.25,
                   max_range=5.25, end_margin=0.0))
    # along y beside the plane x = 2.5 of voxel (2, 0, 16), through y = -2.5 .. 3.5: voxels (2, -3 .. 3, 16); s = 1 and 25
    for name, k, hit in (("parallel at 1 sigma", 1.0, {(2, 0, 16): 1}), ("parallel at 5 sigma", 5.0, {})):
        c.append(_case(name, [(2.5 + k * THIN, -2.5, 16.5)], [[(0, 6, 0)]], hit, [1, 0, 0, 0, 0, 7, len(hit), 0],
                       end_margin=0.0))
    # x = 0.5 + 4 t, y = 0.125 + 2 t, z fixed: faces x=1 (t .125), x=2 (.375), y=1 (.4375), x=3 (.625), x=4 (.875),
    # y=2 (.9375): voxels (0,0) (1,0) (2,0) (2,1) (3,1) (4,1) (4,2); (1,1) and (3,0) hold blobs and are not on the path
    c.append(_case("one zero component", [(0.5, 0.125, 4.5)], [[(4, 2, 0)]], on([(2, 1, 4), (3, 1, 4)]),
                   [1, 0, 0, 0, 0, 7, 2, 0], end_margin=0.0))
    # through the corners (1,1), (2,2), ...: x wins every tie, so (1,0) is entered (over one point, 0.707 m from its centre:
    # s = 4.7) and (0,1) never: voxels (0,0) (1,0) (1,1) (2,1) (2,2) (3,2) (3,3) (4,3) (4,4)
    c.append(_case("diagonal ties", [(0.5, 0.5, 8.5)], [[(4, 4, 0)]], on([(1, 0, 8), (2, 1, 8)]), [1, 0, 0, 0, 0, 9, 2, 0],
                   end_margin=0.0))
    # along the edge y = 1, z = 13 (two zero components of d): floor puts it into the voxels (0 .. 5, 1, 13) and not into
    # their three neighbours around the edge, which hold blobs as near to the ray
    c.append(_case("along an edge", [(0.5, 1.0, 13.0)], [[(5, 0, 0)]], on([(2, 1, 13)]), [1, 0, 0, 0, 0, 6, 1, 0],
                   end_margin=0.0))
    # no ray is walked: length 0 and length 0.5 < the margin of one voxel are short; a NaN; a row outside the grid; a cloud
    # with pose_id -1; a sensor outside the grid whose row is inside
    c.append(_case("dropped", [(0.5, 0.5, 20.5), (3.0e6, 0.5, 0.5)],
                   [[(0, 0, 0), (0.5, 0, 0), (np.nan, 1, 1), (3.0e6, 0, 0)], [(1, 2, 3), (4, 5, 6)], [(1.5 - 3.0e6, 0, 0)]], {},
                   [0, 1, 2, 2, 2, 0, 0, 0], pose_ids=np.array([0, -1, 1], np.int64)))
    return c


def crossed_by_voxel(crossed, keys):
    """crossed per place and the key of each place -> {voxel: count} of the places with a count"""
    return {tuple(IR.key_voxel(int(k))): int(n) for k, n in zip(keys, crossed) if n}


# ---- (b) the scene ----------------------------------------------------------------------------------------------------

BOX = (np.array([3.2, 3.1, -1.6]), np.array([5.4, 5.0, 0.1]))
SURFACE_ROWS, BOX_ROWS, EPS = 6000, 1200, 1e-6


def _box_faces():
    """the four sides and the top of the box as (origin, u, v)"""
    lo, hi = BOX
    e = hi - lo
    ex, ey, ez = np.array([e[0], 0, 0]), np.array([0, e[1], 0]), np.array([0, 0, e[2]])
    return [(lo, ex, ez), (lo + ey, ex, ez), (lo, ey, ez), (lo + ex, ey, ez), (lo + ez, ex, ey)]


def _samples(rng, rects, n):
    area = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v in rects])
    which = rng.choice(len(rects), n, p=area / area.sum())
    ab = rng.uniform(0, 1, (n, 2))
    o, u, v = (np.stack([r[i] for r in rects])[which] for i in range(3))
    return o + ab[:, :1] * u + ab[:, 1:] * v


def _visible(o, pts, rects, box):
    """the points the sensor at o sees: the segment meets no rectangle and not the box at a parameter in (EPS, 1 - EPS)"""
    seg = pts - o
    seen = np.ones(len(pts), bool)
    with np.errstate(all="ignore"):
        for r0, u, v in rects:
            n = np.cross(u, v)
            t = ((r0 - o) @ n) / (seg @ n)
            h = o + t[:, None] * seg - r0
            G = np.array([[u @ u, u @ v], [u @ v, v @ v]])
            ab = np.linalg.solve(G, np.stack([h @ u, h @ v]))
            seen &= ~((t > EPS) & (t < 1.0 - EPS) & (ab >= 0).all(0) & (ab <= 1).all(0))
        if box is not None:
            ta, tb = (box[0] - o) / seg, (box[1] - o) / seg
            enter, leave = np.minimum(ta, tb).max(1), np.maximum(ta, tb).min(1)
            seen &= ~((enter < leave) & (enter < 1.0 - EPS) & (leave > EPS))
    return seen


@functools.lru_cache(maxsize=None)
def scene():
    """-> dict: points (float32, sensor frame), offsets, poses (map_localize_cases.scene's six), is_box (N,) bool"""
    rng = np.random.default_rng(77)
    poses = K.scene()["poses"]
    static = K._surfaces()
    clouds, box_rows = [], []
    for c, T in enumerate(poses):
        present = c < 3
        world = _samples(rng, static, SURFACE_ROWS)
        mark = np.zeros(SURFACE_ROWS, bool)
        if present:
            world = np.concatenate([world, _samples(rng, _box_faces(), BOX_ROWS)])
            mark = np.concatenate([mark, np.ones(BOX_ROWS, bool)])
        keep = _visible(T[:3, 3], world, static, BOX if present else None)
        world = world[keep] + rng.normal(0, 0.01, (int(keep.sum()), 3))
        clouds.append(K._view(world, T))
        box_rows.append(mark[keep])
    off = np.concatenate([[0], np.cumsum([len(x) for x in clouds])]).astype(np.int64)
    return dict(points=np.concatenate(clouds), offsets=off, poses=poses, is_box=np.concatenate(box_rows))


@functools.lru_cache(maxsize=None)
def scene_walks(voxel):
    s = scene()
    return RR.walks(s["points"], s["offsets"], s["poses"], None, (voxel, np.zeros(3)))


@functools.lru_cache(maxsize=None)
def scene_result(voxel):
    """the restatement on the scene at one voxel size, once: its map ``m``, the cast of all six clouds into it (``cast``),
    the flags and their four counts, and the shares the issue bounds: of box rows flagged, and of static rows flagged among
    those in voxels that hold no box row"""
    s = scene()
    m = R.build_dist(s["points"], s["offsets"], s["poses"], voxel_size=voxel)
    cast = RR.cast(s["points"], s["offsets"], s["poses"], None, m, walked=scene_walks(voxel))
    flags, fstats = RR.flag_rows(s["points"], s["offsets"], s["poses"], None, m, m["info"][:, 0].tolist(), cast["crossed"])
    place = rows_place(m, s)
    box_voxels = np.unique(place[s["is_box"]])
    clean = ~s["is_box"] & ~np.isin(place, box_voxels)
    return dict(m=m, cast=cast, flags=flags, flag_stats=fstats, box_share=float(flags[s["is_box"]].mean()),
                static_share=float(flags[clean].mean()))


def rows_place(m, s):
    """the place of each row's own voxel in the map m (-1: none)"""
    r = RR.rays(s["points"], s["offsets"], s["poses"], None, m["grid"])
    return np.array([m["place"].get(k, -1) if k is not None else -1 for k in r["end_key"]], np.int64)
