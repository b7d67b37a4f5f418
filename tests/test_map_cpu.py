"""The global voxel map without a GPU: the restatement (tests/map_restatement.py) against an independent grouping, its
own invariances, the host-side refusals of GlobalMap and nsc_map_build, and the workspace query."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import map_restatement as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def yaw_pose(deg, t):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = t
    return T


def scene(seed=0, sizes=(300, 0, 500, 200), extent=6.0):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-extent, extent, (sum(sizes), 3))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    poses = np.stack([yaw_pose(20.0 * i, rng.uniform(-3, 3, 3)) for i in range(len(sizes))])
    return pts, off, poses


def test_restatement_against_unique_grouping():
    """np.unique over the world-voxel coordinates of the same rows groups them without a dict and without keys; sums in
    Python integers."""
    pts, off, poses = scene()
    pts[7] = np.nan
    pts[400, 1] = np.inf
    ids = np.array([2, 0, -1, 1])
    voxel, origin = 0.5, (0.25, -1.0, 3.0)
    out = M.build_map(pts, off, poses, ids, voxel, origin)
    w, cloud, has_pose = M.world_rows(pts, off, poses, ids)
    assert not has_pose[300:800].any() and has_pose[:300].all() and has_pose[800:].all()
    ok = has_pose & np.isfinite(w).all(1)
    assert out["rows_without_pose"] == 500 and out["rows_not_finite"] == 1 and out["rows_used"] == ok.sum() == 499
    rows = np.nonzero(ok)[0]
    vox = np.floor((w[rows] - np.asarray(origin)) / voxel).astype(np.int64)
    uniq, inv = np.unique(vox, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    assert out["voxels_found"] == len(uniq)
    firsts = np.array([rows[inv == g][0] for g in range(len(uniq))])
    order = np.argsort(firsts)
    assert np.array_equal(out["info"][:, 1], firsts[order])
    for place, g in enumerate(order):
        member = rows[inv == g]
        assert out["info"][place].tolist() == [len(member), member[0], cloud[member].min(), cloud[member].max()]
        k = uniq[g] + (1 << 20)
        assert out["keys"][place] == int(k[0]) | int(k[1]) << 21 | int(k[2]) << 42
        for a in range(3):
            total = sum(int(np.rint(v * 2.0 ** 24)) for v in w[member, a])
            assert out["points"][place, a] == (float(total) / 2.0 ** 24) / float(len(member))
        assert np.abs(out["points"][place] - w[member].mean(0)).max() < 1e-6


def test_restatement_invariances():
    pts, off, poses = scene(1)
    base = M.build_map(pts, off, poses)
    # a permutation of the clouds: the same voxels, first and last cloud mapped through it
    sizes = np.diff(off)

    def permuted(perm):                                             # new cloud i is old cloud perm[i]
        p2 = np.concatenate([pts[off[c]:off[c + 1]] for c in perm])
        return M.build_map(p2, np.concatenate([[0], np.cumsum(sizes[perm])]), poses, pose_ids=perm)

    def by_key(out, clouds=None):
        return {int(k): (int(i[0]), p.tobytes()) + (clouds(i) if clouds else ())
                for k, i, p in zip(out["keys"], out["info"], out["points"])}
    other = permuted(np.array([2, 3, 0, 1]))
    assert other["rows_used"] == base["rows_used"] and by_key(base) == by_key(other)
    # the reversal maps min to max: first and last cloud follow exactly
    rev = permuted(np.array([3, 2, 1, 0]))
    assert by_key(base, lambda i: (int(i[2]), int(i[3]))) == by_key(rev, lambda i: (3 - int(i[3]), 3 - int(i[2])))
    # a dropped cloud: the map of the other clouds, whatever stands in its rows
    ids = np.array([0, 1, -1, 3])
    dropped = M.build_map(pts, off, poses, pose_ids=ids)
    keep = np.r_[0:off[2], off[3]:off[4]]
    rest = M.build_map(pts[keep], np.array([0, sizes[0], sizes[0], sizes[0] + sizes[3]]), poses[[0, 1, 3]])
    assert dropped["rows_without_pose"] == sizes[2] and rest["rows_without_pose"] == 0
    assert np.array_equal(dropped["keys"], rest["keys"]) and dropped["points"].tobytes() == rest["points"].tobytes()
    assert np.array_equal(dropped["info"][:, 0], rest["info"][:, 0])
    # rows outside the grid are counted and dropped, not clamped
    tiny = M.build_map(pts, off, poses, voxel_size=1e-6)
    w, _, _ = M.world_rows(pts, off, poses)
    inside = (np.abs(np.floor(w / 1e-6) + 0.5) < 2 ** 20).all(1)
    assert tiny["rows_outside"] == (~inside).sum() > 0 and tiny["rows_used"] == inside.sum()


def test_globalmap_refusals_on_the_host():
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import GlobalMap, revisited
    with pytest.raises(_lib.NscError):
        GlobalMap(device="cpu")
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(_lib.NscError):
            GlobalMap(voxel_size=bad)
    with pytest.raises(_lib.NscError):
        GlobalMap(origin=(0.0, float("nan"), 0.0))
    with pytest.raises(_lib.NscError):
        GlobalMap(max_voxels=-1)
    m = GlobalMap()                                                   # nothing touches the device yet
    clouds, poses = [np.zeros((2, 3), np.float32)] * 2, np.tile(np.eye(4), (2, 1, 1))
    for ids in ([0, 2], [-2, 0], [0], [0, 1, 1]):
        with pytest.raises(_lib.NscError):
            m.build(clouds, poses, pose_ids=ids)
    with pytest.raises(_lib.NscError):
        m.build([np.zeros((2, 5), np.float32)], poses)
    mask = revisited(np.array([0, 3, 5]), np.array([0, 4, 9]), 2)
    assert mask.tolist() == [False, False, True]


def test_header_constants_match_the_binding():
    from neural_spectral_codec_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nsc.h")).read()
    val = {m.group(1): m.group(2) for m in re.finditer(r"#define NSC_MAP_(\w+)\s+(\(1LL << \d+\)|\d+)", hdr)}
    assert [int(val[k]) for k in ("DTYPE_F32", "DTYPE_F64", "STATS", "TILE_ROWS", "SCAN_THREADS", "INSERT_ROWS",
                                  "INSERT_BLOCKS")] == [
        _lib.MAP_DTYPE_F32, _lib.MAP_DTYPE_F64, _lib.MAP_STATS, _lib.MAP_TILE_ROWS, _lib.MAP_SCAN_THREADS,
        _lib.MAP_INSERT_ROWS, _lib.MAP_INSERT_BLOCKS]
    assert val["MAX_VOXELS"] == "(1LL << 36)" and _lib.MAP_MAX_VOXELS == 1 << 36
    assert val["MAX_ROWS"] == "(1LL << 46)" and _lib.MAP_MAX_ROWS == 1 << 46
    names = ("FOUND", "WRITTEN", "USED", "NOT_FINITE", "OUTSIDE", "NO_POSE", "UNPLACED")
    assert [int(val["STAT_" + n]) for n in names] == list(range(_lib.MAP_STATS)) and len(_lib.MAP_STAT_NAMES) == _lib.MAP_STATS
    assert _lib.MAP_STAT_NAMES == M.STAT_NAMES


def test_workspace_bytes_and_refusals():
    from neural_spectral_codec_amd import _lib
    L = _lib.lib()
    ws = L.nsc_map_workspace_bytes
    assert ws(-1, 10) == 0 and ws(10, -1) == 0 and ws(10, _lib.MAP_MAX_VOXELS + 1) == 0 and ws(_lib.MAP_MAX_ROWS + 1, 10) == 0
    assert ws(_lib.MAP_MAX_ROWS, _lib.MAP_MAX_VOXELS) > 128 << 36
    sizes = (0, 1, 63, 64, 65, _lib.MAP_TILE_ROWS, _lib.MAP_TILE_ROWS + 1, 10 ** 6, 10 ** 8)
    grid = [[ws(n, v) for v in sizes] for n in sizes]
    assert all(a <= b for row in grid for a, b in zip(row, row[1:]))           # monotone in max_voxels
    assert all(a <= b for col in zip(*grid) for a, b in zip(col, col[1:]))     # and in total_rows
    assert ws(0, 0) == 0 and ws(1, 0) > 0 and ws(0, 1) >= 128
    assert ws(10 ** 8, 1 << 24) >= 128 << 24                                   # the table: 2 x 64 bytes per voxel
    p = _lib.MapParams()
    L.nsc_map_default_params(C.byref(p))
    assert p.voxel_size == 0.5 and list(p.origin) == [0.0, 0.0, 0.0]
    d = 256                                                                    # non-null: nothing may be dereferenced

    def build(points=d, dtype=0, stride=3, off=d, B=1, N=5, poses=d, P=1, prm=p, V=4, out=d, stats=d, ws_ptr=None,
              ws_bytes=0):
        return L.nsc_map_build(points, dtype, stride, off, B, N, poses, P, None, C.byref(prm) if prm else None, V, out,
                               out, out, stats, ws_ptr, ws_bytes, None)
    need = ws(5, 4)
    assert build() == -3 and build(ws_ptr=d, ws_bytes=need - 1) == -3            # NSC_EWORKSPACE
    for kw in (dict(B=-1), dict(N=-1), dict(P=-1), dict(V=-1), dict(dtype=2), dict(stride=2), dict(stride=5),
               dict(dtype=1, stride=4), dict(prm=None), dict(stats=None), dict(off=None), dict(points=None),
               dict(poses=None), dict(out=None)):
        assert build(ws_ptr=d, ws_bytes=need, **kw) == -1, kw                   # NSC_EINVAL
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        q = _lib.MapParams(voxel_size=bad)
        assert build(prm=q, ws_ptr=d, ws_bytes=need) == -1
    q = _lib.MapParams(voxel_size=0.5, origin=(C.c_double * 3)(0.0, float("inf"), 0.0))
    assert build(prm=q, ws_ptr=d, ws_bytes=need) == -1
    assert build(V=_lib.MAP_MAX_VOXELS + 1, ws_ptr=d, ws_bytes=need) == -2       # NSC_EUNSUPPORTED
    assert build(N=_lib.MAP_MAX_ROWS + 1, ws_ptr=d, ws_bytes=need) == -2
