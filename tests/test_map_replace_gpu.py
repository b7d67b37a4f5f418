"""Removal from and replacement in a kept map on the MI355X: MapLocalizer.remove* / replace* / update_prepared and
nsc_map_remove_dist / nsc_map_replace_dist against a fresh build over the rows that remain, on the constructed inputs of
tests/map_replace_cases.py, tests/map_insert_cases.py and tests/map_localize_cases.py, whose claims
tests/test_map_replace_cpu.py and tests/test_map_insert_cpu.py assert.

Every comparison is by bits.  With the rebuild it is a comparison of mappings key -> (count, moments, record): the kept
map keeps its places and its emptied voxels, the rebuild has places of its own.  Between two kept maps it is torch.equal
on voxels, info, keys, moments and stats, the index as a mapping key -> place."""
import numpy as np
import pytest
import torch

import map_insert_cases as IK
import map_localize_cases as K
import map_replace_cases as PK
from test_map_insert_cpu import group, joined
from test_map_insert_gpu import (KEPT, assert_guards, assert_same_bits, build_then_insert, captured, guarded, kept, rebuilt,
                                 scene_parts)
from test_map_localize_gpu import dev, index_of, localizer

pytestmark = pytest.mark.gpu

ZEROS = (0, np.zeros(9, np.int64).tobytes(), np.zeros(16).tobytes())


def mapping(k):
    """kept tensors on the host -> {key: (count, the moments' bytes, the record's bytes)} of the voxels with a place"""
    return {key: (int(k["info"][p, 0]), k["moments"][p].tobytes(), k["voxels"][p].tobytes())
            for key, p in index_of(k)[0].items() if p >= 0}


def assert_follows(got, want, what=""):
    """the kept map ``got`` holds every voxel of the rebuild ``want`` with its count, moments and record by bits, and
    every other voxel of it is emptied -> the keys of the emptied voxels"""
    g, w = mapping(got), mapping(want)
    assert int(want["stats"][0]) == int(want["stats"][1]) == len(w), (what, want["stats"])      # found <= max_voxels
    assert set(w) <= set(g), (what, len(set(w) - set(g)))
    for key, v in w.items():
        assert g[key] == v, (what, key, g[key][0], v[0])
    rest = set(g) - set(w)
    for key in rest:
        assert g[key] == ZEROS, (what, key, g[key][0])
    return rest


def assert_only_touched_places_changed(before, after, removed, what=""):
    """places whose count stayed keep every bit; keys, first rows and cloud bounds stay everywhere; emptied places hold
    zeros; the counts of ``removed`` agree with what changed"""
    n = int(before["stats"][1])
    changed = before["info"][:n, 0] != after["info"][:n, 0]
    assert int(changed.sum()) == removed[5], (what, int(changed.sum()), removed)
    for k in KEPT:
        assert after[k][:n][~changed].tobytes() == before[k][:n][~changed].tobytes(), (what, k)
    assert np.array_equal(after["keys"][:n], before["keys"][:n]) and np.array_equal(after["info"][:n, 1:], before["info"][:n, 1:])
    assert index_of(after) == index_of(before), what
    empty = changed & (after["info"][:n, 0] == 0)
    assert int(empty.sum()) == removed[6] and removed[7] == 0, (what, removed)
    assert not after["moments"][:n][empty].any() and after["voxels"][:n][empty].tobytes() == bytes(128 * int(empty.sum()))
    assert after["stats"].tolist() == [before["stats"][0], before["stats"][1], before["stats"][2] - removed[0]] + \
        before["stats"][3:].tolist(), what


def devs(part):
    return tuple(dev(x) for x in part)


# ---- 1. removal against the rebuild -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,cols", [(np.float32, 3), (np.float32, 4), (np.float64, 3)])
def test_removal_equals_the_rebuild(dtype, cols):
    g = IK.general_split(dtype, cols)
    A, B, Co, Cn = (group(g, [n]) for n in ("A", "B", "C_old", "C_new"))
    m = build_then_insert([joined([A, B, Co, Cn])], max_voxels=512)
    left = [A, B, Co, Cn]
    for name, part, rows in (("C_old", Co, 400), ("C_new", Cn, 400), ("B", B, 1200)):
        before = kept(m)
        removed = m.remove_device(*devs(part))["removed"].tolist()
        after = kept(m)
        left = [p for p in left if p is not part]
        emptied = assert_follows(after, rebuilt(left, max_voxels=512), name)
        assert removed[:5] == [rows, 0, 0, 0, 0] and removed[5] > 10, (name, removed)
        assert_only_touched_places_changed(before, after, removed, name)
        assert (name != "C_old" or removed[6] == 0) and (name != "C_new" or removed[6] == removed[5])
        assert (name != "B" or 10 < removed[6] < removed[5] - 10), (name, removed)
    assert after["stats"][2] == 1200 and len(emptied) == int(after["stats"][0]) - int(rebuilt([A], max_voxels=512)["stats"][0])
    # in one call, through the host form
    one = build_then_insert([joined([A, B, Co, Cn])], max_voxels=512)
    p, o, T = joined([Co, Cn, B])
    res = one.remove([p[o[i]:o[i + 1]] for i in range(5)], T)
    assert (res["rows_removed"], res["rows_missing"], res["voxels_inconsistent"], res["rows_used"]) == (2000, 0, 0, 1200)
    assert res["voxels_emptied"] == len(emptied) and int((res["count"] == 0).sum()) == len(emptied)
    assert not bool(res["usable"][res["count"] == 0].any())
    assert_same_bits(kept(one), after, "one call")
    assert one.cursor.tolist() == m.cursor.tolist() == [3200, 8]          # a removal leaves the cursor alone


# ---- 2. sizes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097])
def test_removed_and_replaced_sizes(n):
    """the sweep of 256 rows, the 512 rows of a workgroup and the bitmap tile of 4096 rows; B's clouds 0, 2 and 5 are
    empty; from 4095 rows on the voxel FAR has its rows in the workgroups 1, 2 and 5"""
    A, B, rows = IK.sized_insert(n)
    moved = PK.one_voxel_on(B[2])
    for cast in (np.float32, np.float64):
        a, b = (A[0].astype(cast), A[1], A[2]), (B[0].astype(cast), B[1], B[2])
        m = build_then_insert([a, b], max_voxels=8192)
        removed = m.remove_device(*devs(b))["removed"].tolist()
        got = kept(m)
        emptied = assert_follows(got, rebuilt([a], max_voxels=8192), n)
        assert removed[:5] == [n, 0, 0, 0, 0] and removed[6] == len(emptied) and removed[7] == 0 and got["stats"][2] == 600
        assert (IK.voxel_key(IK.FAR) in emptied) == bool(rows)
        m = build_then_insert([a, b], max_voxels=8192)
        out = m.replace_device(dev(b[0]), dev(b[1]), dev(b[2]), dev(moved), first_row=600, first_cloud=6)
        got = kept(m)
        emptied = assert_follows(got, rebuilt([a, (b[0], b[1], moved)], max_voxels=8192), f"{n} re-placed")
        assert out["removed"].tolist()[:5] == [n, 0, 0, 0, 0] and out["placed"].tolist()[2:] == [n, 0, 0, 0, 0]
        assert got["stats"][2] == 600 + n and got["cursor"].tolist() == [600 + n, 12]
        if rows:
            at = index_of(got)[0][IK.voxel_key(IK.FAR + np.array([1, 0, 0]))]
            assert IK.voxel_key(IK.FAR) in emptied and got["info"][at].tolist() == [3, 600 + rows[0], 7, 10]


# ---- 3. missing rows --------------------------------------------------------------------------------------------------

def test_missing_rows_change_nothing():
    A, B, vox = IK.twelve_voxels()
    views, big, shapes = guarded(8)
    m = build_then_insert([A, B], out=views, max_voxels=8)
    before = kept(m)
    past = (np.floor(B[0])[:, None, :] == vox[None, 8:, :]).all(2).any(1)
    rows = np.concatenate([B[0][past], PK.twelve_voxels_absent_rows()])
    assert int(past.sum()) == 4 * 7
    removed = m.remove_device(dev(rows), dev(np.array([0, 5, len(rows)])), dev(np.tile(np.eye(4), (2, 1, 1))))["removed"]
    assert removed.tolist() == [0, 0, 0, 0, len(rows), 0, 0, 0]
    after = kept(m)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k
    assert_guards(big, shapes)
    # all of B: the rows of the voxels 8 .. 11 are missing, voxel 7 is emptied, A's voxels are those of a build of A
    removed = m.remove_device(*devs(B))["removed"].tolist()
    after = kept(m)
    assert removed == [len(B[0]) - 28, 0, 0, 0, 28, 4, 1, 0]
    assert assert_follows(after, rebuilt([A], max_voxels=8)) == {IK.voxel_key(vox[7])}
    assert index_of(after) == index_of(before) and after["stats"][:2].tolist() == [12, 8]
    assert_guards(big, shapes)


# ---- 4. every kind of row ---------------------------------------------------------------------------------------------

def test_every_kind_of_row_is_counted():
    pts, off, poses, _ = K.ten_voxels()
    m = build_then_insert([(pts, off, poses)], max_voxels=16)
    before = kept(m)
    bp, bo, bT, ids, (used, not_finite, outside, no_pose) = IK.every_kind_of_row()
    m.insert_device(dev(bp), dev(bo), dev(bT), dev(ids))
    between = kept(m)
    removed = m.remove_device(dev(bp), dev(bo), dev(bT), dev(ids))["removed"].tolist()
    assert removed == [used, not_finite, outside, no_pose, 0, 1, 0, 0] == [4, 4, 4, 8, 0, 1, 0, 0]
    after = kept(m)
    assert after["stats"].tolist() == [10, 10, len(pts), not_finite, outside, no_pose, 0]    # a removal takes only its rows back
    assert after["cursor"].tolist() == between["cursor"].tolist()
    assert mapping(after) == mapping(before)


# ---- 5. usable flips --------------------------------------------------------------------------------------------------

def test_one_row_less_makes_a_voxel_unusable():
    pts, off, poses, vox = K.ten_voxels()
    scan, cat = K.lookup_scan(vox)
    r, row = PK.one_row_of_voxel_three()
    m = localizer(insertable=True, max_voxels=6, max_iteration=0)
    m.build_device(dev(pts), dev(off), dev(poses))
    before = kept(m)
    n0 = int(m.register([scan], np.eye(4)[None])["n_correspondences"][0])
    res = m.remove([row], np.eye(4)[None])
    after = kept(m)
    assert (res["rows_removed"], res["voxels_touched"], res["voxels_emptied"]) == (1, 1, 0)
    assert before["voxels"][3, 15] == 1.0 and after["voxels"][3, 15] == 0.0 and not bool(res["usable"][3])
    assert after["info"][3].tolist() == [5] + before["info"][3, 1:].tolist()
    others = np.arange(6) != 3
    for k in KEPT:
        assert after[k][:6][others].tobytes() == before[k][:6][others].tobytes(), k
    n1 = int(m.register([scan], np.eye(4)[None])["n_correspondences"][0])
    assert (n0, n1) == (35, 28)
    m.insert([row], np.eye(4)[None])
    again = kept(m)
    assert mapping(again) == mapping(before) and index_of(again) == index_of(before)
    assert np.array_equal(again["keys"][:6], before["keys"][:6]) and np.array_equal(again["info"][:6, :2], before["info"][:6, :2])
    assert int(m.register([scan], np.eye(4)[None])["n_correspondences"][0]) == 35


# ---- 6. the same cloud removed twice ----------------------------------------------------------------------------------

def test_a_cloud_removed_twice_leaves_zero_records():
    """IK.twelve_voxels with A in the map twice: every voxel of A holds 14 rows, B adds 7 to the voxels 4 .. 11.  B removed
    twice leaves 7 rows in the voxels 4 .. 6 (a positive count: not detectable) and -7 in its own voxels 7 .. 11"""
    A, B, vox = IK.twelve_voxels()
    views, big, shapes = guarded(16)
    m = build_then_insert([A, A, B], out=views, max_voxels=16, max_iteration=0)
    first = m.remove_device(*devs(B))["removed"].tolist()
    assert first == [len(B[0]), 0, 0, 0, 0, 8, 5, 0]
    second = m.remove_device(*devs(B))["removed"].tolist()
    assert second == [len(B[0]), 0, 0, 0, 0, 8, 0, 5]
    got = kept(m)
    at = [index_of(got)[0][IK.voxel_key(v)] for v in vox]
    assert got["info"][at, 0].tolist() == [14] * 4 + [7] * 3 + [-7] * 5
    assert got["voxels"][at[7:]].tobytes() == bytes(128 * 5) and (got["voxels"][at[:4], 15] == 1.0).all()
    assert got["moments"][at[7:]].any(1).all()                          # the integers stay: adding B twice restores the map
    assert_guards(big, shapes)
    own = (np.floor(B[0])[:, None, :] == vox[None, 7:, :]).all(2).any(1)
    untouched = A[0][(np.floor(A[0])[:, None, :] == vox[None, :4, :]).all(2).any(1)]
    out = m.register([B[0][own], untouched], np.tile(np.eye(4), (2, 1, 1)))
    assert int(own.sum()) == 5 * 7 and out["n_correspondences"].tolist() == [0, 4 * 7]
    for _ in range(2):
        m.insert_device(*devs(B))
    assert mapping(kept(m)) == mapping(kept(build_then_insert([A, A, B], max_voxels=16)))
    assert_guards(big, shapes)


# ---- 7. registration against the re-placed map ------------------------------------------------------------------------

@pytest.mark.parametrize("options", [dict(), dict(kernel="cauchy", robust_scale=3.0, neighbours=7)],
                         ids=["plain", "cauchy-7"])
def test_registration_after_replacement_equals_registration_against_the_rebuild(options):
    s = K.scene()
    new, _ = PK.scene_new_poses()
    m = build_then_insert([scene_parts(0, 6)], max_voxels=8192, **options)
    pts, off = PK.scene_cloud_group(PK.SCENE_MOVED)
    ids = list(PK.SCENE_MOVED)
    out = m.replace_device(dev(pts), dev(off), dev(s["poses"][ids]), dev(new[ids]), first_row=8000, first_cloud=2)
    assert out["removed"].tolist()[:5] == [8000, 0, 0, 0, 0] and out["placed"].tolist()[2:] == [8000, 0, 0, 0, 0]
    whole = localizer(max_voxels=8192, **options)
    whole.build_device(dev(s["points"]), dev(s["offsets"]), dev(new), moments=True)
    got, want = kept(m), kept(whole)
    assert got["stats"][0] <= 8192 and want["stats"][0] <= 8192
    emptied = assert_follows(got, want)
    occupied = set(mapping(want))
    # `removed` is the removal half's: a voxel it emptied may have been filled again by the insertion half
    assert int(out["removed"][6]) >= len(emptied) >= 1 and any(n in occupied for k in emptied for n in PK.face_neighbours(k))
    scans = (dev(s["scans"]), dev(s["scan_offsets"]))
    a, b = m.register(scans, s["init"], system0=True), whole.register(scans, s["init"], system0=True)
    assert set(a) == set(b) and ("n_pairs" in b) == bool(options)
    for k in b:
        assert torch.equal(a[k], b[k]), k
    assert bool((b["n_correspondences"] > 1000).all())


# ---- 8. two replacement identities ------------------------------------------------------------------------------------

def test_replacement_is_removal_then_insertion_and_the_identity_for_equal_poses():
    g = IK.general_split(np.float32)
    parts = [group(g, [n]) for n in ("A", "B", "C_old", "C_new")]
    B = parts[1]
    moved = PK.shifted(B[2], PK.B_SHIFT)
    a, b = (build_then_insert([joined(parts)], max_voxels=512) for _ in range(2))
    out = a.replace_device(dev(B[0]), dev(B[1]), dev(B[2]), dev(moved), first_row=3200, first_cloud=8)
    removed = b.remove_device(*devs(B))["removed"]
    before = b.stats.clone()
    b.insert_device(dev(B[0]), dev(B[1]), dev(moved))
    assert_same_bits(kept(a), {**kept(b), "cursor": kept(a)["cursor"]}, "replace against remove, insert")
    assert torch.equal(out["removed"], removed)
    assert out["placed"].tolist() == [int(b.stats[0] - before[0]), int(b.stats[1]), 1200, 0, 0, 0, 0]
    assert a.cursor.tolist() == [3200, 8] and b.cursor.tolist() == [4400, 11]
    assert_follows(kept(a), rebuilt([parts[0], (B[0], B[1], moved), parts[2], parts[3]], max_voxels=512))
    # the same poses on both sides: every voxel is taken apart and made again
    before = kept(a)
    out = a.replace_device(dev(B[0]), dev(B[1]), dev(moved), dev(moved), first_row=1200, first_cloud=3)
    after = kept(a)
    assert out["removed"].tolist()[:5] == [1200, 0, 0, 0, 0] and out["placed"].tolist() == [0, int(before["stats"][1]), 1200, 0, 0, 0, 0]
    assert mapping(after) == mapping(before) and index_of(after) == index_of(before)
    assert after["stats"].tobytes() == before["stats"].tobytes() and after["cursor"].tobytes() == before["cursor"].tobytes()
    assert np.array_equal(after["keys"], before["keys"])


# ---- 9. update_prepared -----------------------------------------------------------------------------------------------

def prepared_scene():
    from neural_spectral_codec_amd.retrieval import PreparedClouds
    s = K.scene()
    store = PreparedClouds(voxel_size=0.25)
    store.add([s["points"][4000 * i:4000 * (i + 1)] for i in range(6)])
    return store


def test_update_prepared_replaces_the_clouds_that_moved():
    s = K.scene()
    new, small = PK.scene_new_poses()
    store = prepared_scene()
    m = localizer(insertable=True, max_voxels=8192)
    res = m.build_prepared(store, s["poses"])
    assert res["complete"]
    n0 = res["voxels_written"]
    out = m.update_prepared(store, s["poses"], small, min_translation=PK.MIN_TRANSLATION, min_rotation=PK.MIN_ROTATION)
    assert out["moved"].tolist() == [-1, -1, 2, 3, -1, -1]
    mixed = s["poses"].copy()
    mixed[list(PK.SCENE_MOVED)] = new[list(PK.SCENE_MOVED)]                 # cloud 1 stays where the map has it
    whole = localizer(insertable=True, max_voxels=8192)
    whole.build_prepared(store, mixed)
    got = kept(m)
    emptied = assert_follows(got, kept(whole))
    rows = store._row_host
    moved_rows = int(rows[4] - rows[2])
    assert out["removed"].tolist()[:5] == [moved_rows, 0, 0, store.n_rows - moved_rows, 0]
    assert int(out["removed"][5]) > int(out["removed"][6]) >= len(emptied) and int(out["removed"][7]) == 0
    assert out["placed"].tolist()[2:] == [moved_rows, 0, 0, store.n_rows - moved_rows, 0]
    assert got["stats"][2:].tolist() == [store.n_rows, 0, 0, 0, 0] and got["cursor"].tolist() == [store.n_rows, 6]
    n1 = int(got["stats"][1])
    assert n1 - n0 == int(out["placed"][0]) > 10
    made = got["info"][n0:n1]                                              # the store's numbering, not the call's
    assert made[:, 1].min() >= rows[2] and made[:, 1].max() < rows[4] and (np.diff(made[:, 1]) > 0).all()
    assert made[:, 2].min() >= 2 and made[:, 3].max() <= 3 and got["info"][:n1, 3].max() == 5
    # with no thresholds the small move counts too, and poses that did not change never do
    out = m.update_prepared(store, mixed, small)
    assert out["moved"].tolist() == [-1, 1, -1, -1, -1, -1]
    whole.build_prepared(store, small)
    assert_follows(kept(m), kept(whole))
    bad = small.copy()
    bad[4, 0, 3] = np.nan                                                   # a pose that is not finite is left alone
    assert m.update_prepared(store, small, bad)["moved"].tolist() == [-1] * 6


# ---- 10. capture ------------------------------------------------------------------------------------------------------

def test_captured_remove_and_replace_replay_on_new_contents():
    from neural_spectral_codec_amd import _lib
    g = IK.general_split(np.float32)
    A, B = group(g, ["A"]), group(g, ["B"])
    C = joined([group(g, ["C_old"]), group(g, ["C_new"]), group(g, ["C_old"])])          # 1200 rows in three clouds, as B
    assert B[0].shape == C[0].shape and B[1].shape == C[1].shape
    eager = build_then_insert([A, B, C], max_voxels=512)
    eager.remove_device(*devs(B))
    eager.remove_device(*devs(C))
    m = build_then_insert([A, B, C], max_voxels=512)
    before = kept(m)
    pts, off, poses = devs(B)
    out = {}
    graph, types = captured(lambda: out.update(m.remove_device(pts, off, poses)))
    assert types == {"kernel": _lib.MAP_REMOVE_LAUNCHES}, types
    assert kept(m)["stats"].tobytes() == before["stats"].tobytes()        # a capture removes nothing
    graph.replay()
    for t, new in zip((pts, off, poses), C):
        t.copy_(dev(new))
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits(kept(m), kept(eager), "captured removal")
    assert out["removed"].tolist()[:5] == [1200, 0, 0, 0, 0]
    assert_follows(kept(m), rebuilt([A], max_voxels=512))
    # replacement: B and then C moved by B_SHIFT
    eager = build_then_insert([A, B, C], max_voxels=512)
    m = build_then_insert([A, B, C], max_voxels=512)
    for p, o, T in (B, C):
        eager.replace_device(dev(p), dev(o), dev(T), dev(PK.shifted(T, PK.B_SHIFT)), first_row=1200, first_cloud=3)
    pts, off, old = devs(B)
    new = dev(PK.shifted(B[2], PK.B_SHIFT))
    graph, types = captured(lambda: out.update(m.replace_device(pts, off, old, new, first_row=1200, first_cloud=3)))
    assert types == {"kernel": _lib.MAP_REPLACE_LAUNCHES}, types
    graph.replay()
    for t, value in zip((pts, off, old, new), C + (PK.shifted(C[2], PK.B_SHIFT),)):
        t.copy_(dev(value))
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits(kept(m), kept(eager), "captured replacement")
    assert out["placed"].tolist()[2:] == [1200, 0, 0, 0, 0] and m.cursor.tolist() == [3600, 9]
    assert_follows(kept(m), rebuilt([A, (B[0], B[1], PK.shifted(B[2], PK.B_SHIFT)), (C[0], C[1], PK.shifted(C[2], PK.B_SHIFT))],
                                    max_voxels=512))


def test_captured_update_prepared_is_kernels_only():
    from neural_spectral_codec_amd import _lib
    s = K.scene()
    new, small = PK.scene_new_poses()
    store = prepared_scene()
    eager, m = (localizer(insertable=True, max_voxels=8192) for _ in range(2))
    for x in (eager, m):
        x.build_prepared(store, s["poses"])
    old, to = dev(s["poses"]), dev(small)
    want = eager.update_prepared(store, old, to, min_translation=PK.MIN_TRANSLATION, min_rotation=PK.MIN_ROTATION)
    out = {}
    graph, types = captured(lambda: out.update(m.update_prepared(store, old, to, min_translation=PK.MIN_TRANSLATION,
                                                                 min_rotation=PK.MIN_ROTATION)))
    assert set(types) == {"kernel"} and types["kernel"] > _lib.MAP_REPLACE_LAUNCHES, types     # the choice, then the replacement
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits(kept(m), kept(eager), "captured update")
    for k in ("moved", "removed", "placed"):
        assert torch.equal(out[k], want[k]), k


# ---- 11. alone and twice ----------------------------------------------------------------------------------------------

def test_the_same_sequence_twice_and_a_cloud_alone_or_in_a_batch():
    g = IK.general_split(np.float32)
    A, B, Co, Cn = (group(g, [n]) for n in ("A", "B", "C_old", "C_new"))
    moved = PK.shifted(Co[2], PK.B_SHIFT)

    def sequence():
        m = build_then_insert([A, B, Co, Cn], max_voxels=512)
        m.remove_device(*devs(B))
        m.replace_device(dev(Co[0]), dev(Co[1]), dev(Co[2]), dev(moved), first_row=2400, first_cloud=6)
        m.insert_device(*devs(B))
        m.remove_device(*devs(Cn))
        return kept(m)
    a, b = sequence(), sequence()
    assert_same_bits(a, b)
    assert a["cursor"].tobytes() == b["cursor"].tobytes()
    assert_follows(a, rebuilt([A, B, (Co[0], Co[1], moved)], max_voxels=512))
    # B and C_new removed one by one and in one call; C_old re-placed alone and in a call that also re-places C_new to
    # where it is
    one, both = (build_then_insert([A, B, Co, Cn], max_voxels=512) for _ in range(2))
    one.remove_device(*devs(B))
    one.remove_device(*devs(Cn))
    both.remove_device(*devs(joined([B, Cn])))
    assert_same_bits(kept(one), kept(both), "removal alone and in a batch")
    one, both = (build_then_insert([A, B, Co, Cn], max_voxels=512) for _ in range(2))
    one.replace_device(dev(Co[0]), dev(Co[1]), dev(Co[2]), dev(moved), first_row=2400, first_cloud=6)
    p, o, T = joined([Co, Cn])
    both.replace_device(dev(p), dev(o), dev(T), dev(np.concatenate([moved, Cn[2]])), first_row=2400, first_cloud=6)
    x, y = kept(one), kept(both)
    assert mapping(x) == mapping(y) and index_of(x) == index_of(y) and x["stats"].tobytes() == y["stats"].tobytes()
