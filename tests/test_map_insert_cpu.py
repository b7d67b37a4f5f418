"""Insertion into a kept map without a GPU: the restated insertion (tests/map_insert_restatement.py) against the restated
build over all clouds, the claims of the constructed inputs (tests/map_insert_cases.py) that tests/test_map_insert_gpu.py
relies on, the host-side refusals of ``MapLocalizer.insert*`` and the argument checks of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import map_insert_cases as IK
import map_insert_restatement as IR
import map_localize_cases as K
import map_localize_restatement as R


@pytest.fixture(scope="module")
def lib():
    from neural_spectral_codec_amd import build, _lib
    build.build_hip()
    return _lib.lib()


def assert_same_map(got, want, what=""):
    """two maps of the restatement agree exactly: integers as integers, records to the last bit"""
    assert got["stats"].tolist() == want["stats"].tolist(), (what, got["stats"], want["stats"])
    assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["info"], want["info"]), what
    assert got["moments"].tolist() == want["moments"].tolist(), what
    assert got["voxels"].tobytes() == want["voxels"].tobytes(), what
    assert got["place"] == want["place"], what


def inserted(parts, max_voxels, **kw):
    """build the first part, insert the others one by one -> the state as arrays"""
    p, o, T = parts[0]
    s = IR.start(R.build_dist(p, o, T, max_voxels=max_voxels, **kw), len(p), len(o) - 1, **kw)
    for p, o, T in parts[1:]:
        IR.insert(s, p, o, T)
    return IR.arrays(s)


def joined(parts):
    pts = np.concatenate([p for p, _, _ in parts])
    off, at = [np.zeros(1, np.int64)], 0
    for p, o, _ in parts:
        off.append(np.asarray(o[1:], np.int64) + at)
        at += len(p)
    return pts, np.concatenate(off), np.concatenate([T for _, _, T in parts])


# ---- 1. the restatement against itself --------------------------------------------------------------------------------

def group(g, names):
    ids = [i for n in names for i in g[n]]
    pts, off = IK.pack([g["clouds"][i] for i in ids])
    return pts, off, g["poses"][ids]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restated_insertion_equals_restated_build(dtype):
    g = IK.general_split(dtype)
    A, B, Co, Cn = (group(g, [n]) for n in ("A", "B", "C_old", "C_new"))
    whole = R.build_dist(*joined([A, B, Co, Cn]), max_voxels=512)
    assert_same_map(inserted([A, B, Co, Cn], 512), whole, "one by one")
    assert_same_map(inserted([A, joined([B, Co, Cn])], 512), whole, "one insert")
    empty = (A[0][:0], np.zeros(1, np.int64), A[2][:0])
    assert_same_map(inserted([A, empty], 512), R.build_dist(*A, max_voxels=512), "an empty insert")
    assert_same_map(inserted([A, empty, B], 512), R.build_dist(*joined([A, B]), max_voxels=512), "an empty insert first")
    # other parameters reach the records of the voxels an insertion touches
    kw = dict(min_points=3, eigen_ratio=0.1, sigma_floor=0.05)
    assert_same_map(inserted([A, B], 512, **kw), R.build_dist(*joined([A, B]), max_voxels=512, **kw), "parameters")


def test_restated_insertion_numbers_rows_and_clouds_from_the_cursor():
    (pa, oa, Ta), (pb, ob, Tb), _ = IK.sized_insert(513)
    s = IR.start(R.build_dist(pa, oa, Ta, max_voxels=4096), len(pa), len(oa) - 1)
    before = len(s["keys"])
    IR.insert(s, pb, ob, Tb)
    m = IR.arrays(s)
    assert m["cursor"] == [600 + 513, 12] and len(m["keys"]) > before
    new = m["info"][before:]
    assert new[:, 1].min() >= 600 and (np.diff(new[:, 1]) > 0).all()       # first rows count on from the cursor, ascending
    assert new[:, 2].min() >= 6 and new[:, 3].max() <= 11                  # clouds too; B's last cloud is empty
    assert_same_map(m, R.build_dist(*joined([(pa, oa, Ta), (pb, ob, Tb)]), max_voxels=4096))


# ---- 3. the claims of the constructed inputs --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,cols", [(np.float32, 3), (np.float32, 4), (np.float64, 3)])
def test_general_split_claims(dtype, cols):
    g = IK.general_split(dtype, cols)
    A, B, Co, Cn = (group(g, [n]) for n in ("A", "B", "C_old", "C_new"))
    a = R.build_dist(*A, max_voxels=512)
    ab = R.build_dist(*joined([A, B]), max_voxels=512)
    abo = R.build_dist(*joined([A, B, Co]), max_voxels=512)
    whole = R.build_dist(*joined([A, B, Co, Cn]), max_voxels=512)
    assert a["rows_used"] == 1200 and whole["rows_used"] == 3200
    shared = len(set(R.build_dist(*B)["place"]) & set(a["place"]))
    assert shared > 10 and ab["voxels_found"] - a["voxels_found"] > 10     # B: partly A's voxels, partly new ones
    assert abo["voxels_found"] == ab["voxels_found"]                       # C_old: existing voxels alone
    cn = R.build_dist(*Cn)
    assert not set(cn["place"]) & set(abo["place"]) and cn["voxels_found"] > 10   # C_new: new voxels alone
    assert whole["voxels_found"] <= 512                                    # far below the 1024 slots
    for part in (A, B, Co, Cn):
        m = R.build_dist(*part)
        assert K.M.face_distance(m["world"], m["used"], voxel_size=1.0) >= 1e-4


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097])
def test_sized_insert_claims(n):
    from neural_spectral_codec_amd import _lib
    assert (_lib.MAP_INSERT_ROWS, _lib.MAP_TILE_ROWS) == (512, 4096)      # the sizes walk these boundaries and the sweep of 256
    A, B, rows = IK.sized_insert(n)
    assert len(B[0]) == n and B[1].tolist() == K.offsets_with_empty_clouds(n).tolist()
    b = R.build_dist(*B, max_voxels=8192)
    assert b["rows_used"] == n and np.array_equal(B[0] * 64, np.rint(B[0] * 64))
    whole = R.build_dist(*joined([A, B]), max_voxels=8192)
    assert whole["voxels_found"] <= 8192 and whole["rows_used"] == 600 + n
    if n > 1:
        a = R.build_dist(*A, max_voxels=8192)
        assert whole["voxels_found"] > a["voxels_found"] or n < 255       # new voxels beside A's
    if n > 3000:
        far = IK.voxel_key(IK.FAR)
        at = whole["place"][far]
        assert whole["info"][at].tolist() == [3, 600 + 700, 6 + 1, 6 + 4] and far not in R.build_dist(*A)["place"]
        assert [r // 512 for r in rows] == [1, 2, 5]
    else:
        assert rows == []


def test_twelve_voxels_claims():
    A, B, vox = IK.twelve_voxels()
    a, whole = R.build_dist(*A, max_voxels=8), R.build_dist(*joined([A, B]), max_voxels=8)
    assert a["stats"][:2].tolist() == [7, 7] and whole["stats"][:2].tolist() == [12, 8]
    keys = [IK.voxel_key(v) for v in vox]
    assert whole["keys"].tolist() == keys                                  # in first-row order: 7 takes the last place
    assert [whole["place"][k] for k in keys[8:]] == [8, 9, 10, 11]          # four voxels past the outputs
    # probe chains: in 16 slots a new key's first slot is a slot an old key's probe sequence holds
    home = [IK.mix64(k) % 16 for k in keys]
    table = {}
    for k, h in zip(keys[:7], home[:7]):
        while h in table:
            h = (h + 1) % 16
        table[h] = k
    assert any(h in table for h in home[7:]), (home, sorted(table))


def test_ten_voxels_split_claims():
    A, B, vox = IK.ten_voxels_split()
    pts, off, poses, _ = K.ten_voxels()
    assert np.array_equal(np.concatenate([A[0], B[0]]), pts) and len(A[0]) == int(off[1])
    a = R.build_dist(*A)
    assert a["voxels_found"] == 10                                         # the first row of every voxel is in A
    whole = R.build_dist(*joined([A, B]))
    assert whole["info"][:, 0].tolist() == [8, 8, 8, 6, 5, 8, 8, 8, 8, 8]   # min_points - 1 rows in voxel 4
    assert whole["voxels"][4, 15] == 0.0
    s = IR.start(whole, len(pts), 2)
    IR.insert(s, IK.one_row_in_the_unusable_voxel(), np.array([0, 1]), np.eye(4)[None])
    m = IR.arrays(s)
    assert m["info"][4].tolist() == [6, int(whole["info"][4, 1]), 0, 2] and m["voxels"][4, 15] == 1.0
    others = np.arange(10) != 4
    assert m["voxels"][others].tobytes() == whole["voxels"][others].tobytes()


def test_every_kind_of_row_claims():
    pts, off, poses, ids, (used, not_finite, outside, no_pose) = IK.every_kind_of_row()
    m = R.build_dist(pts, off, poses, ids)
    assert m["stats"][2:].tolist() == [used, not_finite, outside, no_pose, 0] and used + not_finite + outside + no_pose == len(pts)
    base = R.build_dist(*K.ten_voxels()[:3])
    assert set(m["place"]) <= set(base["place"])


# ---- 2. refusals ------------------------------------------------------------------------------------------------------

def test_insert_refusals_on_the_host():
    import torch
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import MapLocalizer
    cloud = np.zeros((5, 3), np.float32)
    m = MapLocalizer(insertable=True, max_voxels=16)
    assert m.insertable and m.cursor is None and not MapLocalizer().insertable
    for call in (lambda: m.insert([cloud], np.eye(4)[None]), lambda: m.extend([cloud], np.eye(4)[None], 0.5),
                 lambda: m.insert_device(torch.zeros(5, 3), torch.tensor([0, 5]), torch.eye(4)[None])):
        with pytest.raises(_lib.NscError, match="build a map first"):
            call()
    plain = MapLocalizer(max_voxels=16)
    plain.voxels = torch.zeros(0, 16)                                       # as if a map were there
    with pytest.raises(_lib.NscError, match="not built insertable"):
        plain.insert([cloud], np.eye(4)[None])
    with pytest.raises(_lib.NscError, match="not built insertable"):
        plain.extend([cloud], np.eye(4)[None], 0.5)
    m.voxels, m.moments, m.cursor = torch.zeros(0, 16), torch.zeros(0, 9), torch.zeros(2)
    with pytest.raises(_lib.NscError):
        m.insert([cloud, cloud], np.eye(4)[None], pose_ids=[0])             # one id per cloud
    with pytest.raises(_lib.NscError):
        m.insert([cloud], np.eye(4)[None], pose_ids=[1])                    # an id past the poses
    with pytest.raises(_lib.NscError):
        m.insert([np.zeros((5, 2), np.float32)], np.eye(4)[None])
    with pytest.raises(_lib.NscError):
        m.insert([cloud], np.zeros((3, 5)))
    with pytest.raises(_lib.NscError, match="one .* pose per scan"):
        m.extend([cloud, cloud], np.eye(4)[None], 0.5)
    with pytest.raises(_lib.NscError):                                      # host tensors: no CPU fallback
        m.insert_device(torch.zeros(5, 3), torch.tensor([0, 5]), torch.eye(4)[None])
    class ThreeClouds:                                                      # a store of three clouds, for the range of start
        def __len__(self):
            return 3
    for start in (-1, 4):
        with pytest.raises(_lib.NscError, match="start must lie in"):
            m.insert_prepared(ThreeClouds(), np.eye(4)[None], start=start)
    with pytest.raises(_lib.NscError):                                      # one id per inserted cloud: two from start=1
        m.insert_prepared(ThreeClouds(), np.eye(4)[None], pose_ids=[0], start=1)
    with pytest.raises(_lib.NscError, match="build a map first"):
        MapLocalizer(insertable=True).insert_prepared(ThreeClouds(), np.eye(4)[None])
    dev = torch.device("meta")
    m.voxels = torch.zeros(0, 16, device=dev)                               # a map on another device than the scans
    with pytest.raises(_lib.NscError, match="map's device"):
        m.insert_device(torch.zeros(5, 3), torch.tensor([0, 5]), torch.eye(4)[None])


def test_insert_kernels_use_no_scratch(lib, tmp_path):
    """the seven kernels of the insertion (claim and accumulate for float32 and float64 rows, mark, assign, refresh) keep
    everything in registers, the record's Jacobi sweep included (no scratch), and leave room for four waves per SIMD (at
    most 128 VGPRs, the bar of test_linearize_keeps_its_sums_in_registers); read from the gfx950 code object"""
    import kernel_budget as KB
    # the binutils stand beside the hipcc that built the library: their absence is a failure, not a reason to skip
    assert KB.binutils(), f"no llvm binutils in {KB.LLVM}"
    found = KB.kernels(r"ins_(claim|mark|assign|accumulate|refresh)_kernel")
    assert len(found) == 7, sorted(found)
    for k, (vg, sc) in found.items():
        print(f"{k}: {vg} VGPRs, {sc} B scratch")
        assert sc == 0 and vg <= 128, f"{k}: {vg} VGPRs, {sc} B scratch"


def test_abi_refusals_and_workspace(lib):
    from neural_spectral_codec_amd import _lib
    up = lambda v: (v + 255) // 256 * 256
    size = lib.nsc_map_insert_workspace_bytes
    assert lib.nsc_map_insert_workspace_bytes.argtypes == [C.c_int64]       # no capacity argument
    for n in (0, 1, 64, 65, 4096, 4097, 120000, 64 * 120000):
        words, tiles = (n + 63) // 64, (n + 4095) // 4096
        assert size(n) == up(8 * words) + up(4 * words) + up(8 * tiles) + 2 * up(8 * n) + up(8 * 7)
    sizes = [size(n) for n in (0, 1, 255, 256, 257, 4096, 4097, 10 ** 6, 10 ** 9)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert size(-1) == 0 and size(_lib.MAP_MAX_ROWS + 1) == 0 and size(_lib.MAP_MAX_ROWS) > 0
    assert _lib.MAP_INSERT_LAUNCHES == 8
    g, d = _lib.MapParams(), _lib.MapDistParams()
    lib.nsc_map_default_params(C.byref(g))
    lib.nsc_map_dist_default_params(C.byref(d))
    stats, cursor, off = (C.c_int64 * 7)(), (C.c_int64 * 2)(), (C.c_int64 * 1)(0)
    mom, ws = (C.c_int64 * 9)(), (C.c_uint8 * 4096)()
    some = (C.c_int64 * 64)()

    def call(dist=C.byref(d), vox=0, outputs=None, moments=mom, cur=cursor, st=stats, work=ws, nbytes=4096, dtype=0,
             stride=3, rows=0, grid=C.byref(g), offsets=off):
        return lib.nsc_map_insert_dist(None, dtype, stride, offsets, 0, rows, None, 0, None, grid, dist, vox, outputs,
                                       outputs, outputs, outputs, moments, st, cur, work, nbytes, None)
    # nsc_map_build_dist's refusals
    assert call(dist=None) == -1 and call(grid=None) == -1 and call(st=None) == -1 and call(offsets=None) == -1
    assert call(vox=4) == -1                                                # outputs missing
    assert call(vox=-1) == -1 and call(rows=-1) == -1 and call(rows=1) == -1        # rows without points
    assert call(dtype=2) == -1 and call(stride=5) == -1 and call(dtype=1, stride=4) == -1
    assert call(vox=_lib.MAP_MAX_VOXELS + 1, outputs=some) == -2
    for name, bad in (("min_points", 0), ("eigen_ratio", 0.0), ("eigen_ratio", 2.0), ("sigma_floor", 0.0),
                      ("sigma_floor", float("inf"))):
        e = _lib.MapDistParams(min_points=6, reserved=0, eigen_ratio=1e-2, sigma_floor=1e-3)
        setattr(e, name, bad)
        assert call(dist=C.byref(e)) == -1, name
    bad_grid = _lib.MapParams(voxel_size=0.0, origin=(C.c_double * 3)(0, 0, 0))
    assert call(grid=C.byref(bad_grid)) == -1
    # its own: the moments and the cursor are needed, and a workspace even for no rows
    assert call(moments=None) == -1 and call(cur=None) == -1
    assert call(work=None) == -3 and call(nbytes=size(0) - 1) == -3
    assert b"workspace" in lib.nsc_status_string(-3)
