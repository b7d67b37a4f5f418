"""Removal from and replacement in a kept map without a GPU: the restated removal and replacement
(tests/map_replace_restatement.py) against the restated build over what remains, the claims of the constructed inputs
(tests/map_replace_cases.py) that tests/test_map_replace_gpu.py relies on, the host-side refusals of
``MapLocalizer.remove*`` / ``replace*`` / ``update_prepared``, the argument checks of the C ABI and the registers of the
new kernels."""
import ctypes as C

import numpy as np
import pytest

import map_insert_cases as IK
import map_insert_restatement as IR
import map_localize_cases as K
import map_localize_restatement as R
import map_replace_cases as PK
import map_replace_restatement as PR
from test_map_insert_cpu import group, joined


@pytest.fixture(scope="module")
def lib():
    from neural_spectral_codec_amd import build, _lib
    build.build_hip()
    return _lib.lib()


def state(parts, max_voxels, **kw):
    """the restated build over all parts -> a state of the restatement"""
    p, o, T = joined(parts)
    return IR.start(R.build_dist(p, o, T, max_voxels=max_voxels, **kw), len(p), len(o) - 1, **kw)


# ---- 1. the restatement against itself --------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restated_removal_and_replacement_equal_the_restated_build(dtype):
    g = IK.general_split(dtype)
    A, B, Co, Cn = (group(g, [n]) for n in ("A", "B", "C_old", "C_new"))
    s = state([A, B, Co, Cn], 512)
    before = IR.arrays(s)
    counts, touched, emptied, bad = PR.remove(s, *B)
    rest = R.build_dist(*joined([A, Co, Cn]), max_voxels=512)
    got = IR.arrays(s)
    assert PR.assert_follows(got, rest, "B removed") == len(emptied)
    assert counts == [1200, 0, 0, 0, 0, len(touched), len(emptied), 0] and not bad
    if dtype == np.float32:
        assert (len(touched), len(emptied), rest["voxels_found"]) == (60, 36, 84)
    assert got["stats"].tolist() == [before["stats"][0], before["stats"][1], 3200 - 1200, 0, 0, 0, 0]
    # keys, places, first rows and cloud bounds stay; untouched places keep every bit
    assert np.array_equal(got["keys"], before["keys"]) and got["place"] == before["place"]
    assert np.array_equal(got["info"][:, 1:], before["info"][:, 1:])
    same = np.setdiff1d(np.arange(len(got["keys"])), touched)
    assert got["voxels"][same].tobytes() == before["voxels"][same].tobytes()
    # B put back under poses 0.37 / -0.21 / 0.05 m away: the build over the moved input
    s = state([A, B, Co, Cn], 512)
    moved = PK.shifted(B[2], PK.B_SHIFT)
    counts, placed = PR.replace(s, B[0], B[1], B[2], moved, first_row=1200, first_cloud=3)
    want = R.build_dist(*joined([A, (B[0], B[1], moved), Co, Cn]), max_voxels=512)
    got = IR.arrays(s)
    emptied = PR.assert_follows(got, want, "B re-placed")
    assert counts[0] == 1200 and placed[2:] == [1200, 0, 0, 0, 0] and placed[0] == got["stats"][0] - before["stats"][0]
    assert got["stats"][2:].tolist() == [3200, 0, 0, 0, 0] and got["cursor"] == [3200, 8]
    if dtype == np.float32:
        assert want["voxels_found"] == 170
    assert len(got["keys"]) == want["voxels_found"] + emptied <= 512
    # removal followed by insertion at the same bases is the replacement
    s2 = state([A, B, Co, Cn], 512)
    PR.remove(s2, *B)
    s2["cursor"] = [1200, 3]
    IR.insert(s2, B[0], B[1], moved)
    two = IR.arrays(s2)
    for k in ("keys", "info", "stats"):
        assert np.array_equal(two[k], got[k]), k
    assert two["moments"].tolist() == got["moments"].tolist() and two["voxels"].tobytes() == got["voxels"].tobytes()
    # everything removed, one group after the other: every voxel is emptied
    for part in (Cn, A, Co, B):
        PR.remove(s2, part[0], part[1], moved if part is B else part[2])
    assert PR.assert_follows(IR.arrays(s2), R.build_dist(A[0][:0], np.zeros(1, np.int64), A[2][:0]), "all removed") == len(two["keys"])
    assert s2["stats"][2] == 0


def test_restated_removal_with_ids_missing_rows_and_twice():
    A, B, vox = IK.twelve_voxels()
    s = state([A, B], 8)
    before = IR.arrays(s)
    # cloud 0 of B is left out; cloud 1 has rows in voxels 8 .. 11, which are past the outputs: missing
    counts, touched, emptied, bad = PR.remove(s, B[0], B[1], B[2], np.array([-1, 1]))
    half = len(B[0]) // 2
    w = B[0][half:]
    past = int((np.floor(w)[:, None, :] == vox[None, 8:, :]).all(2).any(1).sum())
    assert counts[3] == half and counts[4] == past > 0 and counts[0] == half - past and not bad
    assert s["stats"][2] == before["stats"][2] - counts[0]
    # the same rows again: their voxels end below zero, or at zero with nothing left only if they held these rows twice
    counts2, touched2, emptied2, bad2 = PR.remove(s, B[0], B[1], B[2], np.array([-1, 1]))
    assert counts2[:5] == counts[:5] and touched2 == touched and bad2
    after = IR.arrays(s)
    assert all(after["voxels"][at].tobytes() == np.zeros(16).tobytes() for at in bad2)
    # adding them back twice restores the integers
    for _ in range(2):
        s["cursor"] = [0, 0]
        IR.insert(s, B[0][half:], np.array([0, len(w)]), np.eye(4)[None])
    again = IR.arrays(s)
    n = 8
    assert np.array_equal(again["info"][:n, 0], before["info"][:n, 0])
    assert again["moments"][:n].tolist() == before["moments"][:n].tolist()
    assert again["voxels"][:n].tobytes() == before["voxels"][:n].tobytes()


# ---- 2. the claims of the constructed inputs --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,cols", [(np.float32, 3), (np.float32, 4), (np.float64, 3)])
def test_general_split_removal_claims(dtype, cols):
    """removing C_new empties every voxel of C_new and touches nothing else; removing C_old empties none; removing B
    empties some of its voxels and keeps others"""
    g = IK.general_split(dtype, cols)
    A, B, Co, Cn = (group(g, [n]) for n in ("A", "B", "C_old", "C_new"))
    s = state([A, B, Co, Cn], 512)
    place = dict(s["place"])
    counts, touched, emptied, bad = PR.remove(s, *Co)
    assert counts[0] == 400 and len(touched) > 10 and not emptied and not bad
    counts, touched, emptied, bad = PR.remove(s, *Cn)
    own = sorted(place[k] for k in R.build_dist(*Cn)["place"])
    assert counts[0] == 400 and sorted(touched) == sorted(emptied) == own and len(own) > 10 and not bad
    counts, touched, emptied, bad = PR.remove(s, *B)
    assert counts[0] == 1200 and 10 < len(emptied) < len(touched) - 10 and not bad
    PR.assert_follows(IR.arrays(s), R.build_dist(*A, max_voxels=512), "A is left")


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097])
def test_sized_removal_claims(n):
    """B of IK.sized_insert removed again leaves A; FAR is emptied; B's poses moved by one voxel keep the input exact"""
    A, B, rows = IK.sized_insert(n)
    s = state([A, B], 8192)
    counts, touched, emptied, bad = PR.remove(s, *B)
    assert counts[0] == n and counts[1:5] == [0, 0, 0, 0] and not bad
    PR.assert_follows(IR.arrays(s), R.build_dist(*A, max_voxels=8192), n)
    if rows:
        assert s["place"][IK.voxel_key(IK.FAR)] in emptied
    moved = PK.one_voxel_on(B[2])
    w = R.build_dist(B[0], B[1], moved, max_voxels=8192)
    assert w["rows_used"] == n and np.array_equal(w["world"][w["used"]] * 64, np.rint(w["world"][w["used"]] * 64))
    if rows:
        assert IK.voxel_key(IK.FAR + np.array([1, 0, 0])) in w["place"]
    whole = R.build_dist(*joined([A, (B[0], B[1], moved)]), max_voxels=8192)
    assert whole["voxels_found"] + len(emptied) <= 8192


def test_twelve_voxels_and_ten_voxels_removal_claims():
    A, B, vox = IK.twelve_voxels()
    whole = R.build_dist(*joined([A, B]), max_voxels=8)
    assert IK.voxel_key([40, 40, 40]) not in whole["place"]
    # seven rows per voxel in A's voxels 0 .. 6 and in B's 4 .. 11: with A twice in a map, B removed twice leaves 7 rows in
    # the shared voxels 4 .. 6 and -7 in B's own
    a, b = R.build_dist(*A), R.build_dist(*B)
    assert a["info"][:, 0].tolist() == [7] * 7 and b["info"][:, 0].tolist() == [7] * 8
    assert a["keys"].tolist() == [IK.voxel_key(v) for v in vox[:7]] and b["keys"].tolist() == [IK.voxel_key(v) for v in vox[4:]]
    assert np.array_equal(np.floor(PK.twelve_voxels_absent_rows()), np.full((2, 3), 40.0))
    r, row = PK.one_row_of_voxel_three()
    pts, off, poses, vox = K.ten_voxels()
    m = R.build_dist(pts, off, poses)
    assert m["info"][3, 0] == 6 and m["voxels"][3, 15] == 1.0 and np.array_equal(np.floor(row[0]), vox[3])
    s = IR.start(m, len(pts), 2)
    counts, touched, emptied, bad = PR.remove(s, row, np.array([0, 1]), np.eye(4)[None])
    assert counts == [1, 0, 0, 0, 0, 1, 0, 0] and touched == [3]
    after = IR.arrays(s)
    assert after["info"][3, 0] == 5 and after["voxels"][3, 15] == 0.0
    scan, cat = K.lookup_scan(vox)
    assert int((np.floor(scan[cat == "usable"]) == vox[3]).all(1).sum()) == 7


def test_scene_replacement_claims():
    """the scene's clouds 2 and 3 moved 0.6 m and 2 degrees: the map stays below 8192 voxels on both sides, voxels are
    emptied, and at least one emptied voxel is a face neighbour of an occupied one"""
    s = K.scene()
    new, small = PK.scene_new_poses()
    for c in PK.SCENE_MOVED:
        dt, dr = K.pose_error(new[c], s["poses"][c])
        assert abs(dr - np.deg2rad(2.0)) < 1e-9 and dt >= 0.59
    dt, dr = K.pose_error(small[1], s["poses"][1])
    assert 0 < dt < PK.MIN_TRANSLATION and dr < PK.MIN_ROTATION
    assert all(dt >= PK.MIN_TRANSLATION and dr >= PK.MIN_ROTATION
               for dt, dr in (K.pose_error(new[c], s["poses"][c]) for c in PK.SCENE_MOVED))
    old_keys, new_keys = PK.scene_keys(s["poses"]), PK.scene_keys(new)
    emptied = old_keys - new_keys
    # every cloud samples the same surfaces, so only the few voxels that the moved clouds held alone are emptied
    assert len(old_keys | new_keys) <= 8192 and len(emptied) >= 1 and len(new_keys - old_keys) > 10
    assert any(n in new_keys for k in emptied for n in PK.face_neighbours(k))


# ---- 3. refusals ------------------------------------------------------------------------------------------------------

def test_remove_and_replace_refusals_on_the_host():
    import torch
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import MapLocalizer
    cloud, eye = np.zeros((5, 3), np.float32), np.eye(4)[None]
    dpts, doff, deye = torch.zeros(5, 3), torch.tensor([0, 5]), torch.eye(4)[None]

    class ThreeClouds:                                                      # a store of three clouds
        def __len__(self):
            return 3
    m = MapLocalizer(insertable=True, max_voxels=16)
    calls = (lambda m: m.remove([cloud], eye), lambda m: m.remove_device(dpts, doff, deye),
             lambda m: m.remove_prepared(ThreeClouds(), eye), lambda m: m.replace([cloud], eye, eye),
             lambda m: m.replace_device(dpts, doff, deye, deye), lambda m: m.update_prepared(ThreeClouds(), eye, eye))
    for call in calls:
        with pytest.raises(_lib.NscError, match="build a map first"):
            call(m)
    plain = MapLocalizer(max_voxels=16)
    plain.voxels = torch.zeros(0, 16)                                       # as if a map were there
    for call in calls:
        with pytest.raises(_lib.NscError, match="not built insertable"):
            call(plain)
    m.voxels, m.moments, m.cursor = torch.zeros(0, 16), torch.zeros(0, 9), torch.zeros(2)
    for call in (lambda ids: m.remove([cloud, cloud], eye, pose_ids=ids),
                 lambda ids: m.replace([cloud, cloud], eye, eye, pose_ids=ids)):
        with pytest.raises(_lib.NscError, match="one entry per cloud"):
            call([0])                                                       # one id per cloud
        with pytest.raises(_lib.NscError, match="pose_ids must be -1 or lie in"):
            call([0, 1])                                                    # an id past the poses
    with pytest.raises(_lib.NscError):
        m.remove([np.zeros((5, 2), np.float32)], eye)
    with pytest.raises(_lib.NscError):
        m.remove([cloud], np.zeros((3, 5)))
    with pytest.raises(_lib.NscError, match="one pose each per id"):
        m.replace([cloud], eye, np.tile(eye, (2, 1, 1)))
    for bases in (dict(first_row=-1), dict(first_cloud=-1)):
        with pytest.raises(_lib.NscError, match="must not be negative"):
            m.replace([cloud], eye, eye, **bases)
        with pytest.raises(_lib.NscError, match="must not be negative"):
            m.replace_device(dpts, doff, deye, deye, **bases)
    for call in (lambda: m.remove_device(dpts, doff, deye), lambda: m.replace_device(dpts, doff, deye, deye)):
        with pytest.raises(_lib.NscError):                                  # host tensors: no CPU fallback
            call()
    for start, stop in ((-1, None), (4, None), (2, 1), (0, 4)):
        with pytest.raises(_lib.NscError, match="start and stop must satisfy"):
            m.remove_prepared(ThreeClouds(), eye, start=start, stop=stop)
    with pytest.raises(_lib.NscError, match="one entry per cloud"):         # one id per removed cloud: two in [1, 3)
        m.remove_prepared(ThreeClouds(), eye, pose_ids=[0], start=1)
    with pytest.raises(_lib.NscError, match="one .* pose per cloud of the store"):
        m.update_prepared(ThreeClouds(), eye, eye)
    three = np.tile(eye, (3, 1, 1))
    with pytest.raises(_lib.NscError, match="one .* pose per cloud of the store"):
        m.update_prepared(ThreeClouds(), three, eye)
    for kw in (dict(min_translation=-1.0), dict(min_rotation=float("nan"))):
        with pytest.raises(_lib.NscError, match="must not be negative"):
            m.update_prepared(ThreeClouds(), three, three, **kw)
    m.voxels = torch.zeros(0, 16, device=torch.device("meta"))              # a map on another device than the clouds
    for call in (lambda: m.remove_device(dpts, doff, deye), lambda: m.replace_device(dpts, doff, deye, deye)):
        with pytest.raises(_lib.NscError, match="map's device"):
            call()


def test_abi_refusals_workspace_and_launch_constants(lib):
    import re
    from neural_spectral_codec_amd import _lib
    up = lambda v: (v + 255) // 256 * 256
    rem, rep, ins = lib.nsc_map_remove_workspace_bytes, lib.nsc_map_replace_workspace_bytes, lib.nsc_map_insert_workspace_bytes
    assert rem.argtypes == [C.c_int64] and rep.argtypes == [C.c_int64]      # no capacity argument
    for n in (0, 1, 64, 65, 4096, 4097, 120000, 64 * 120000):
        assert rem(n) == up(8 * n) + up(8 * 7)                              # the touched list and the call's counters
        assert rep(n) == ins(n) + rem(n) + up(8 * 2)                        # both, and the bases as a cursor of its own
    for size in (rem, rep):
        sizes = [size(n) for n in (0, 1, 255, 256, 257, 4096, 4097, 10 ** 6, 10 ** 9)]
        assert sizes == sorted(sizes) and sizes[0] > 0
        assert size(-1) == 0 and size(_lib.MAP_MAX_ROWS + 1) == 0 and size(_lib.MAP_MAX_ROWS) > 0
    # the launch constants, here and in the header
    assert (_lib.MAP_REMOVE_LAUNCHES, _lib.MAP_REPLACE_LAUNCHES) == (3, 10)
    assert _lib.MAP_REPLACE_LAUNCHES <= _lib.MAP_REMOVE_LAUNCHES + _lib.MAP_INSERT_LAUNCHES
    import os
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "nsc.h")).read()
    for name, value in (("NSC_MAP_REMOVE_LAUNCHES", _lib.MAP_REMOVE_LAUNCHES), ("NSC_MAP_REPLACE_LAUNCHES", _lib.MAP_REPLACE_LAUNCHES),
                        ("NSC_MAP_REMOVE_STATS", _lib.MAP_REMOVE_STATS)):
        assert int(re.search(rf"#define {name}\s+(\d+)", header).group(1)) == value, name
    assert len(_lib.MAP_REMOVE_STAT_NAMES) == _lib.MAP_REMOVE_STATS == 8
    g, d = _lib.MapParams(), _lib.MapDistParams()
    lib.nsc_map_default_params(C.byref(g))
    lib.nsc_map_dist_default_params(C.byref(d))
    stats, removed, placed, off = (C.c_int64 * 7)(), (C.c_int64 * 8)(), (C.c_int64 * 7)(), (C.c_int64 * 1)(0)
    mom, ws = (C.c_int64 * 9)(), (C.c_uint8 * 8192)()
    some = (C.c_int64 * 64)()
    pose = (C.c_double * 16)()

    def remove(dist=C.byref(d), vox=0, outputs=None, moments=mom, rm=removed, st=stats, work=ws, nbytes=8192, dtype=0,
               stride=3, rows=0, grid=C.byref(g), offsets=off, **_):
        return lib.nsc_map_remove_dist(None, dtype, stride, offsets, 0, rows, None, 0, None, grid, dist, vox, outputs,
                                       outputs, outputs, outputs, moments, st, rm, work, nbytes, None)

    def replace(dist=C.byref(d), vox=0, outputs=None, moments=mom, rm=removed, pl=placed, st=stats, work=ws, nbytes=8192,
                dtype=0, stride=3, rows=0, grid=C.byref(g), offsets=off, row0=0, cloud0=0, poses=0, old=None, new=None):
        return lib.nsc_map_replace_dist(None, dtype, stride, offsets, 0, rows, old, new, poses, None, grid, dist, vox,
                                        outputs, outputs, outputs, outputs, moments, st, row0, cloud0, rm, pl, work, nbytes,
                                        None)
    for call, size in ((remove, rem), (replace, rep)):
        # nsc_map_build_dist's refusals
        assert call(dist=None) == -1 and call(grid=None) == -1 and call(st=None) == -1 and call(offsets=None) == -1
        assert call(vox=4) == -1                                            # outputs missing
        assert call(vox=-1) == -1 and call(rows=-1) == -1 and call(rows=1) == -1    # rows without points
        assert call(dtype=2) == -1 and call(stride=5) == -1 and call(dtype=1, stride=4) == -1
        assert call(vox=_lib.MAP_MAX_VOXELS + 1, outputs=some) == -2
        for name, bad in (("min_points", 0), ("eigen_ratio", 0.0), ("eigen_ratio", 2.0), ("sigma_floor", 0.0),
                          ("sigma_floor", float("inf"))):
            e = _lib.MapDistParams(min_points=6, reserved=0, eigen_ratio=1e-2, sigma_floor=1e-3)
            setattr(e, name, bad)
            assert call(dist=C.byref(e)) == -1, name
        bad_grid = _lib.MapParams(voxel_size=0.0, origin=(C.c_double * 3)(0, 0, 0))
        assert call(grid=C.byref(bad_grid)) == -1
        # the insertion's: the moments are needed, and a workspace even for no rows
        assert call(moments=None) == -1
        assert call(work=None) == -3 and call(nbytes=size(0) - 1) == -3
        # their own
        assert call(rm=None) == -1
    assert replace(pl=None) == -1 and replace(row0=-1) == -1 and replace(cloud0=-1) == -1
    assert replace(poses=1, old=pose, new=None) == -1 and replace(poses=1, old=None, new=pose) == -1


def test_remove_and_replace_kernels_use_no_scratch(lib, tmp_path):
    """the five new kernels (the clear, the removal's row pass for float32 and float64 rows, its refresh) and the
    insertion's refresh, whose loop body the removal's shares, keep everything in registers (no scratch) and leave room
    for four waves per SIMD (at most 128 VGPRs); read from the gfx950 code object as test_insert_kernels_use_no_scratch
    does"""
    import kernel_budget as KB
    # the binutils stand beside the hipcc that built the library: their absence is a failure, not a reason to skip
    assert KB.binutils(), f"no llvm binutils in {KB.LLVM}"
    found = KB.kernels(r"call_clear_kernel|rem_(rows|refresh)_kernel|ins_refresh_kernel")
    assert len(found) == 5, sorted(found)
    for k, (vg, sc) in found.items():
        print(f"{k}: {vg} VGPRs, {sc} B scratch")
        assert sc == 0 and vg <= 128, f"{k}: {vg} VGPRs, {sc} B scratch"
