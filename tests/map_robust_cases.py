"""Constructed inputs of tests/test_map_robust_cpu.py and tests/test_map_robust_gpu.py, on top of map_localize_cases.  The
CPU file asserts what each case claims about itself; the GPU file relies on those claims.  Every reference is computed once
(functools.lru_cache) and shared."""
import functools

import numpy as np

import map_localize_cases as K
import map_localize_restatement as R
import map_robust_restatement as RR

# the configurations compared end to end: (kernel, width, neighbours)
CLUTTER_ROBUST = ("geman_mcclure", 2.0, 1)
WIDE_ROBUST = ("cauchy", 3.0, 7)
# the configurations whose sums at the initial poses are compared
SYSTEM_CONFIGS = [(k, 2.0, nb) for k in ("huber", "cauchy", "geman_mcclure") for nb in (1, 7)]


@functools.lru_cache(maxsize=None)
def clutter_scans():
    """the scene's eight scans with 20 % of each scan's rows moved 0.15 .. 0.45 m off their surface toward the room's
    centre (0, 0, 0.9): objects in front of walls -> (8 x 2000, 3) float32"""
    s = K.scene()
    rng = np.random.default_rng(77)
    scans = s["scans"].copy()
    off = s["scan_offsets"]
    for i, T in enumerate(s["truth"]):
        rows = scans[off[i]:off[i + 1]]
        n = len(rows)
        pick = rng.choice(n, n // 5, replace=False)
        world = rows[pick].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        to = np.array([0.0, 0.0, 0.9]) - world
        world = world + to / np.linalg.norm(to, axis=1, keepdims=True) * rng.uniform(0.15, 0.45, (len(pick), 1))
        rows[pick] = ((world - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    return scans


@functools.lru_cache(maxsize=None)
def wide_scene():
    """-> the restatement's map of the scene at 0.5 m voxels and initial poses 1.0 m and 3 / 1 / 1 degrees off the truth,
    drawn as map_localize_cases.scene draws its own"""
    s = K.scene()
    rng = np.random.default_rng(9)
    init = []
    for T in s["truth"]:
        sg = rng.choice([-1.0, 1.0], 6)
        dT = K.general_pose(sg[0] * np.deg2rad(3.0), sg[1] * np.deg2rad(1.0), sg[3:6] * 1.0 / np.sqrt(3.0),
                            roll=sg[2] * np.deg2rad(1.0))
        init.append(dT @ T)
    m = R.build_dist(s["points"], s["offsets"], s["poses"], voxel_size=0.5)
    return dict(map=m, init=np.stack(init))


def errors(got, want):
    """(S,2): translation (m) and rotation (rad) between two stacks of poses"""
    return np.array([K.pose_error(a, b) for a, b in zip(got, want)])


def reference(m, scans, offsets, init, truth, kernel, scale, neighbours):
    """the restatement on one configuration: its result, its errors to the truth, the scans it finishes before
    max_iteration and, over those, the largest change of its result when every scan coordinate moves by +-2^-24 m"""
    kw = dict(kernel=kernel, scale=scale, neighbours=neighbours)
    ref = RR.register(m, scans, offsets, init, **kw)
    rng = np.random.default_rng(5)
    moved = scans.astype(np.float64) + rng.choice([-1.0, 1.0], scans.shape) * 2.0 ** -24
    alt = RR.register(m, moved, offsets, init, **kw)
    finished = (ref["iterations"] < 30) & (alt["iterations"] < 30)
    change = errors(ref["transform"], alt["transform"])[finished].max(0)
    return dict(ref=ref, to_truth=errors(ref["transform"], truth), finished=finished, change=change)


@functools.lru_cache(maxsize=None)
def clutter_reference(robust):
    """the clutter scans against the scene's 1.0 m map from the scene's own initial poses: quadratic (robust=False) or
    CLUTTER_ROBUST"""
    s, m = K.scene(), K.scene_reference()["map"]
    kernel, scale, nb = CLUTTER_ROBUST if robust else (None, None, 1)
    return reference(m, clutter_scans(), s["scan_offsets"], s["init"], s["truth"], kernel, scale, nb)


@functools.lru_cache(maxsize=None)
def wide_reference():
    """the scene's scans against the 0.5 m map from the wide starts with WIDE_ROBUST"""
    s, ws = K.scene(), wide_scene()
    return reference(ws["map"], s["scans"], s["scan_offsets"], ws["init"], s["truth"], *WIDE_ROBUST)


@functools.lru_cache(maxsize=None)
def off_face():
    """the scene's scans without the rows that come within FACE_MARGIN voxels of a face under the scene's initial poses
    -> (points float64, offsets, share left out)"""
    s, m = K.scene(), K.scene_reference()["map"]
    return K.off_face_scans(m, s["scans"].astype(np.float64), s["scan_offsets"], s["init"])


# ---- pair counting on map_localize_cases.ten_voxels with max_voxels = 6 -----------------------------------------------

def neighbour_scan(vox):
    """rows for a map of ten_voxels with max_voxels = 6: lookup_scan's rows (own voxel usable, unusable, past the capacity,
    absent, outside the grid, not finite) and, per map voxel v and face direction, rows in the voxel next to v -- an
    absent own voxel whose neighbour v is usable (0, 1, 2, 3, 5), unusable (4) or past the capacity (6 .. 9)"""
    rng = np.random.default_rng(13)
    base, _ = K.lookup_scan(vox)
    rows = [base]
    for v in vox:
        for off in RR.OFFSETS[1:]:
            rows.append(((np.asarray(v) + off) * 64 + rng.integers(1, 64, (2, 3))) / 64.0)
    pts = np.concatenate(rows)
    return pts[rng.permutation(len(pts))]


TOP = (1 << 21) - 1
# key coordinates of four map voxels at the grid's first and last coordinate on x.  A packed key that borrowed or carried
# would take A's -x neighbour for B (key(A) - 1 == key(B)) and C's +x neighbour for D (key(C) + 1 == key(D))
EDGE_VOXELS = np.array([(0, 1, 0), (TOP, 0, 0), (TOP, 5, 5), (0, 6, 5)], np.int64)


def edge_map(origin_shift=0):
    """a map of EDGE_VOXELS (eight rows each, 1.0 m voxels, float64 lattice points about 2^20 m from the origin, exact),
    with the grid's origin and every point shifted by ``origin_shift`` whole voxels
    -> (points, offsets, poses, origin, scan): the scan has three rows in each map voxel, in each voxel one step further
    inside the grid on x (whose x neighbour is a map voxel) and one step outside the grid on x (no voxel at all)"""
    rng = np.random.default_rng(17)

    def inside(coord, k):
        return (np.asarray(coord, np.float64) - float(1 << 20) + origin_shift) + rng.integers(1, 64, (k, 3)) / 64.0
    pts = np.concatenate([inside(v, 8) for v in EDGE_VOXELS])
    rows = []
    for v in EDGE_VOXELS:
        step = np.array([1 if v[0] == 0 else -1, 0, 0])
        rows += [inside(v, 3), inside(v + step, 3), inside(v - step, 3)]
    return pts, np.array([0, len(pts)], np.int64), np.eye(4)[None], (float(origin_shift),) * 3, np.concatenate(rows)
