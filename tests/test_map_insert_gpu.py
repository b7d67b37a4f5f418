"""Insertion into a kept map on the MI355X: MapLocalizer.insert* / extend / nsc_map_insert_dist against a fresh build over
all clouds (by bits) and against the restated insertion (tests/map_insert_restatement.py), on the constructed inputs of
tests/map_insert_cases.py and tests/map_localize_cases.py, whose claims tests/test_map_insert_cpu.py asserts.

Comparisons with the rebuild are by bits: torch.equal on voxels[:n], info[:n], keys[:n], moments[:n] and stats, the index
as a mapping key -> place (which of two keys that meet in a slot claims it is free, so a key may sit in different slots).
The bars of the one comparison that is not exact (records against the exact-rational restatement) are those of
tests/test_map_localize_gpu.py."""
import numpy as np
import pytest
import torch

import map_insert_cases as IK
import map_insert_restatement as IR
import map_localize_cases as K
import map_localize_restatement as R
from test_map_insert_cpu import group, joined
from test_map_localize_gpu import assert_build_exact, assert_records_close, dev, host, index_of, localizer

pytestmark = pytest.mark.gpu

KEPT = ("voxels", "info", "keys", "moments")
EXTEND_CHOICE_KERNELS = 4               # torch operators by which ``extend`` turns fitness into pose_ids on the device
GUARD, SENTINEL = 8, -77


def kept(m):
    """the kept tensors on the host"""
    return {k: getattr(m, k).cpu().numpy() for k in KEPT + ("index", "stats", "cursor") if getattr(m, k) is not None}


def assert_same_bits(got, want, what=""):
    """two maps on the host agree by bits where they are defined, and a lookup finds the same in both"""
    assert got["stats"].tobytes() == want["stats"].tobytes(), (what, got["stats"], want["stats"])
    n = int(want["stats"][1])
    for k in KEPT:
        assert got[k][:n].tobytes() == want[k][:n].tobytes(), (what, k)
    assert index_of(got) == index_of(want), what


def guarded(M):
    """the kept tensors of capacity M with GUARD sentinel elements behind each -> (the views to build into, the whole)"""
    shapes = dict(voxels=(M, 16), index=(2 * M, 2), info=(M, 4), keys=(M,), moments=(M, 9), stats=(7,), cursor=(2,))
    big = {k: torch.full((s[0] + GUARD,) + s[1:], SENTINEL, dtype=torch.float64 if k == "voxels" else torch.int64,
                         device="cuda") for k, s in shapes.items()}
    return {k: big[k][:shapes[k][0]] for k in shapes}, big, shapes


def assert_guards(big, shapes):
    for k, s in shapes.items():
        assert bool((big[k][s[0]:] == SENTINEL).all()), k


def build_then_insert(parts, out=None, **kw):
    """an insertable map of the first part, the others inserted one by one -> the localizer"""
    m = localizer(insertable=True, **kw)
    p, o, T = parts[0]
    m.build_device(dev(p), dev(o), dev(T), out=out)
    for p, o, T in parts[1:]:
        m.insert_device(dev(p), dev(o), dev(T))
    return m


def rebuilt(parts, **kw):
    """a fresh build over all parts, moments kept -> its buffers on the host"""
    p, o, T = joined(parts)
    return host(localizer(**kw).build_device(dev(p), dev(o), dev(T), moments=True))


# ---- 1. equality with the rebuild -------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,cols", [(np.float32, 3), (np.float32, 4), (np.float64, 3)])
def test_insertion_equals_the_rebuild(dtype, cols):
    g = IK.general_split(dtype, cols)
    A, B, Co, Cn = (group(g, [n]) for n in ("A", "B", "C_old", "C_new"))
    want = rebuilt([A, B, Co, Cn], max_voxels=512)
    m = build_then_insert([A, B], max_voxels=512)
    ab = kept(m)
    assert_same_bits(ab, rebuilt([A, B], max_voxels=512), "A then B")
    assert ab["stats"][0] > rebuilt([A], max_voxels=512)["stats"][0]
    res = m.insert((dev(Co[0]), dev(Co[1])), Co[2])                      # existing voxels alone
    abo = kept(m)
    assert res["voxels_found"] == ab["stats"][0] and res["rows_used"] == ab["stats"][2] + 400 and res["complete"]
    assert_same_bits(abo, rebuilt([A, B, Co], max_voxels=512), "then C_old")
    res = m.insert(list(np.split(Cn[0], 1)), Cn[2])                      # new voxels alone, through the host form
    n = int(abo["stats"][1])
    assert res["voxels_found"] > n and res["count"].shape[0] == res["voxels_found"]
    for k in KEPT:                                                       # nothing that was there has moved
        assert getattr(m, k)[:n].cpu().numpy().tobytes() == abo[k][:n].tobytes(), k
    assert_same_bits(kept(m), want, "one by one")
    assert m.cursor.tolist() == [3200, 8]
    assert_same_bits(kept(build_then_insert([A, joined([B, Co, Cn])], max_voxels=512)), want, "one insert")
    assert_same_bits(kept(build_then_insert([A, B, joined([Co, Cn])], max_voxels=512)), want, "two inserts")


# ---- 2. sizes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097])
def test_inserted_sizes_and_empty_clouds(n):
    """the sweep of 256 rows, the 512 rows of a workgroup and the bitmap tile of 4096 rows; B's clouds 0, 2 and 5 are
    empty; from 4095 rows on a new voxel has its rows in the workgroups 1, 2 and 5"""
    A, B, rows = IK.sized_insert(n)
    for cast in (np.float32, np.float64):
        a, b = (A[0].astype(cast), A[1], A[2]), (B[0].astype(cast), B[1], B[2])
        m = build_then_insert([a, b], max_voxels=8192)
        got = kept(m)
        assert_same_bits(got, rebuilt([a, b], max_voxels=8192), n)
        assert got["cursor"].tolist() == [600 + n, 12] and got["stats"][2] == 600 + n
        if rows:
            at = index_of(got)[0][IK.voxel_key(IK.FAR)]
            assert got["info"][at].tolist() == [3, 600 + rows[0], 7, 10]


# ---- 3. probe chains, and voxels past the outputs ---------------------------------------------------------------------

def test_probe_chains_and_overflow():
    A, B, vox = IK.twelve_voxels()
    views, big, shapes = guarded(8)
    m = build_then_insert([A, B], out=views, max_voxels=8)
    got, want = kept(m), rebuilt([A, B], max_voxels=8)
    assert_same_bits(got, want)
    assert got["stats"][:2].tolist() == [12, 8] and got["stats"][2] == len(A[0]) + len(B[0]) and got["stats"][6] == 0
    places, occupied = index_of(got)
    assert occupied == 12 and [places[IK.voxel_key(v)] for v in vox] == list(range(8)) + [-1] * 4
    assert_guards(big, shapes)
    # a further insertion into the full outputs: the voxels past them keep their keys, a new one is found and not written
    extra = ((np.array([30, 30, 30]) * 64 + np.array([[3, 5, 7], [9, 11, 13]])) / 64.0, np.array([0, 2]), np.eye(4)[None])
    m.insert_device(dev(B[0]), dev(B[1]), dev(B[2]))
    m.insert_device(*(dev(x) for x in extra))
    assert_same_bits(kept(m), rebuilt([A, B, B, extra], max_voxels=8), "into full outputs")
    assert m.stats[:2].tolist() == [13, 8]
    assert_guards(big, shapes)


# ---- 4. a full table --------------------------------------------------------------------------------------------------

def test_full_table_keeps_its_invariants():
    """ten voxels, six slots: which voxels get in depends on arrival, so only invariants hold (as
    test_map_localize_gpu.test_capacity_table_short)"""
    A, B, _ = IK.ten_voxels_split()
    ref = R.build_dist(*joined([A, B]))
    views, big, shapes = guarded(3)
    m = build_then_insert([A, B], out=views, max_voxels=3)
    out = kept(m)
    found, written, used, not_finite, outside, no_pose, unplaced = out["stats"].tolist()
    assert used + not_finite + outside + no_pose + unplaced == len(A[0]) + len(B[0]) and unplaced > 0
    assert (found, written, not_finite, outside, no_pose) == (6, 3, 0, 0, 0)
    assert_guards(big, shapes)
    place = {int(k): i for i, k in enumerate(ref["keys"].tolist())}
    at = [place[int(k)] for k in out["keys"][:3]]
    assert at == sorted(at)
    # a voxel in the table takes every one of its rows, A's and B's: the first three records are the complete map's
    assert np.array_equal(out["info"][:3], ref["info"][at])
    assert np.array_equal(out["moments"][:3], np.array(ref["moments"][at].tolist(), np.int64))
    whole = rebuilt([A, B], max_voxels=16)
    assert out["voxels"][:3].tobytes() == whole["voxels"][at].tobytes()
    places, occupied = index_of(out)
    assert occupied == 6 and sorted(p for p in places.values() if p >= 0) == [0, 1, 2]
    assert all(int(out["keys"][p]) == k for k, p in places.items() if p >= 0)


# ---- 5. every kind of row ---------------------------------------------------------------------------------------------

def test_every_kind_of_row_is_counted():
    pts, off, poses, _ = K.ten_voxels()
    m = build_then_insert([(pts, off, poses)], max_voxels=16)
    before = kept(m)
    bp, bo, bT, ids, (used, not_finite, outside, no_pose) = IK.every_kind_of_row()
    # the ids as a device tensor: the host does not read them, and the library counts the cloud whose id is past the poses
    # (the same ids as a host sequence are refused before anything goes to the device)
    m.insert_device(dev(bp), dev(bo), dev(bT), dev(ids))
    after = kept(m)
    assert (after["stats"] - before["stats"]).tolist() == [0, 0, used, not_finite, outside, no_pose, 0]
    assert after["cursor"].tolist() == [len(pts) + len(bp), 2 + 5]
    touched = [0]                                                        # cloud 0's rows are in voxel 0: the one used cloud
    same = np.setdiff1d(np.arange(10), touched)
    for k in KEPT:
        assert after[k][same].tobytes() == before[k][same].tobytes(), k
    assert after["info"][0].tolist() == [before["info"][0, 0] + 4, before["info"][0, 1], 0, 2]
    assert index_of(after) == index_of(before)
    want = R.build_dist(pts, off, poses, max_voxels=16)
    s = IR.start(want, len(pts), 2)
    IR.insert(s, bp, bo, bT, ids)
    assert_build_exact(after, IR.arrays(s))


# ---- 6. usable flips --------------------------------------------------------------------------------------------------

def test_one_row_makes_a_voxel_usable():
    pts, off, poses, vox = K.ten_voxels()
    scan, cat = K.lookup_scan(vox)
    m = localizer(insertable=True, max_voxels=6, max_iteration=0)
    m.build_device(dev(pts), dev(off), dev(poses))
    before = kept(m)
    n0 = int(m.register([scan], np.eye(4)[None])["n_correspondences"][0])
    res = m.insert([IK.one_row_in_the_unusable_voxel()], np.eye(4)[None])
    after = kept(m)
    assert before["voxels"][4, 15] == 0.0 and after["voxels"][4, 15] == 1.0 and bool(res["usable"][4])
    assert after["info"][4].tolist() == [6, before["info"][4, 1], 0, 2]
    others = np.arange(6) != 4
    for k in KEPT:
        assert after[k][:6][others].tobytes() == before[k][:6][others].tobytes(), k
    n1 = int(m.register([scan], np.eye(4)[None])["n_correspondences"][0])
    assert (n0, n1) == (35, 35 + int((cat == "unusable").sum())) and n1 == 40
    only = host(m.register([scan[cat == "unusable"]], np.eye(4)[None]))
    assert only["n_correspondences"].tolist() == [5]


# ---- 7. registration after insertion ----------------------------------------------------------------------------------

def scene_parts(a, b):
    s = K.scene()
    return s["points"][4000 * a:4000 * b], s["offsets"][a:b + 1] - 4000 * a, s["poses"][a:b]


def test_registration_after_insertion_equals_registration_against_the_rebuild():
    s = K.scene()
    m = build_then_insert([scene_parts(0, 4), scene_parts(4, 6)], max_voxels=4096)
    whole = localizer(max_voxels=4096)
    whole.build_device(dev(s["points"]), dev(s["offsets"]), dev(s["poses"]), moments=True)
    assert_same_bits(kept(m), kept(whole))
    scans = (dev(s["scans"]), dev(s["scan_offsets"]))
    got, want = m.register(scans, s["init"], system0=True), whole.register(scans, s["init"], system0=True)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert bool((want["n_correspondences"] > 1000).all())


# ---- 7b. the clouds of a store ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_ids", [False, True])
def test_insert_prepared_equals_the_rebuild_and_insert(with_ids):
    """three clouds of a PreparedClouds built, three more added to the store and inserted from ``start=3``: the map is
    the build over the whole store and the map ``insert`` gives on the same rows, by bits; with ``pose_ids`` the poses
    come permuted and the middle cloud is left out; ``start=len(store)`` inserts nothing"""
    from neural_spectral_codec_amd.retrieval import PreparedClouds
    s = K.scene()
    clouds = [s["points"][4000 * i:4000 * (i + 1)] for i in range(6)]
    store = PreparedClouds(voxel_size=0.25)
    store.add(clouds[:3])
    m, by_insert = (localizer(insertable=True, max_voxels=4096) for _ in range(2))
    assert m.build_prepared(store, s["poses"][:3])["complete"] and by_insert.build_prepared(store, s["poses"][:3])["complete"]
    rows3 = store.n_rows
    assert m.cursor.tolist() == [rows3, 3]
    store.add(clouds[3:])
    assert len(store) == 6 and store.n_rows > rows3 + 300
    if with_ids:
        poses, ids, all_ids = s["poses"][[5, 0, 3]], [2, -1, 0], [0, 1, 2, 3, -1, 5]
    else:
        poses, ids, all_ids = s["poses"][3:], None, None
    res = m.insert_prepared(store, poses, pose_ids=ids, start=3)
    left_out = int(store.cloud(4)["points"].shape[0]) if with_ids else 0
    assert res["rows_without_pose"] == left_out and res["rows_used"] == store.n_rows - left_out and res["complete"]
    whole = localizer(insertable=True, max_voxels=4096)
    whole.build_prepared(store, s["poses"], pose_ids=all_ids)
    assert_same_bits(kept(m), kept(whole), "against the build over the store")
    assert m.cursor.tolist() == whole.cursor.tolist() == [store.n_rows, 6]
    assert int(m.info[:res["voxels_written"], 3].max()) == 5              # the store's cloud numbers, not the call's
    by_insert.insert([store.cloud(i)["points"] for i in (3, 4, 5)], poses, pose_ids=ids)
    assert_same_bits(kept(m), kept(by_insert), "against insert of the same rows")
    before = kept(m)
    res = m.insert_prepared(store, s["poses"][:0], start=len(store))
    after = kept(m)
    assert after["cursor"].tolist() == [store.n_rows, 6] and res["voxels_found"] == int(before["stats"][0])
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k


# ---- 8. the restatement on exact input --------------------------------------------------------------------------------

@pytest.mark.parametrize("voxel", [0.5, 1.0])
def test_insertion_equals_the_restatement_on_exact_input(voxel):
    pts, off, poses = K.exact_case(1, 3500, voxel)
    cut = int(off[4])                                                    # four clouds built, two inserted
    A, B = (pts[:cut], off[:5], poses[:4]), (pts[cut:], off[4:] - cut, poses[4:])
    s = IR.start(R.build_dist(*A, voxel_size=voxel, max_voxels=4096), cut, 4)
    touched = IR.insert(s, *B)
    ref = IR.arrays(s)
    assert len(touched) > 100 and ref["voxels_found"] > len(touched)
    for cast in (np.float32, np.float64):
        m = build_then_insert([(A[0].astype(cast), A[1], A[2]), (B[0].astype(cast), B[1], B[2])], voxel_size=voxel,
                              max_voxels=4096)
        out = kept(m)
        assert_build_exact(out, ref, np.dtype(cast).name)
        assert_records_close(out, ref, voxel, f"inserted, {np.dtype(cast).name}")
        assert index_of(out)[0] == ref["place"] and out["cursor"].tolist() == ref["cursor"]


# ---- 9. extend --------------------------------------------------------------------------------------------------------

def test_extend_inserts_the_scans_that_registered():
    s = K.scene()
    scans = list(np.split(s["scans"], 8)) + [IK.scene_far_scan()]
    init = np.concatenate([s["init"], s["init"][:1]])
    a = build_then_insert([scene_parts(0, 6)], max_voxels=8192)
    b = build_then_insert([scene_parts(0, 6)], max_voxels=8192)
    out = a.extend(scans, init, min_fitness=0.3)
    fitness = out["fitness"].cpu().numpy()
    assert (fitness[:8] > 0.3).all() and fitness[8] == 0.0
    assert a.complete is None
    reg = b.register(scans, init)
    for k in reg:
        assert torch.equal(out[k], reg[k]), k
    res = b.insert(scans, reg["transform"], pose_ids=list(range(8)) + [-1])
    assert res["rows_without_pose"] == 2000 and res["rows_used"] == 24000 + 16000 and res["complete"]
    assert_same_bits(kept(a), kept(b))
    assert a.cursor.tolist() == b.cursor.tolist() == [24000 + 18000, 6 + 9]


# ---- 10. capture ------------------------------------------------------------------------------------------------------

def captured(step):
    """``step`` captured into a hipGraph (not run) -> (the graph, its node types)"""
    from _hipgraph import keep_graphs, node_types
    torch.cuda.synchronize()
    with keep_graphs() as made:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
    return g, node_types(made[0])


def test_captured_insert_replays_as_further_insertions():
    from neural_spectral_codec_amd import _lib
    g = IK.general_split(np.float32)
    A, B = group(g, ["A"]), group(g, ["B"])
    C = joined([group(g, ["C_old"]), group(g, ["C_new"]), group(g, ["C_old"])])          # 1200 rows in three clouds, as B
    assert B[0].shape == C[0].shape and B[1].shape == C[1].shape
    eager = build_then_insert([A, B, C], max_voxels=512)
    m = build_then_insert([A], max_voxels=512)
    pts, off, poses = dev(B[0]), dev(B[1]), dev(B[2])
    graph, types = captured(lambda: m.insert_device(pts, off, poses))
    assert types == {"kernel": _lib.MAP_INSERT_LAUNCHES}, types
    assert m.cursor.tolist() == [1200, 3]                                # a capture inserts nothing
    graph.replay()
    for t, new in zip((pts, off, poses), C):
        t.copy_(dev(new))
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits(kept(m), kept(eager))
    assert m.cursor.tolist() == eager.cursor.tolist() == [3600, 9]


def test_captured_extend_replays_as_further_insertions():
    from neural_spectral_codec_amd import _lib
    s = K.scene()
    first, second = (s["scans"][:8000], s["init"][:4]), (s["scans"][8000:], s["init"][4:])
    off = dev(s["scan_offsets"][:5])
    eager = build_then_insert([scene_parts(0, 6)], max_voxels=8192, max_iteration=3)
    for rows, init in (first, second):
        eager.extend((dev(rows), off), init, min_fitness=0.3)
    m = build_then_insert([scene_parts(0, 6)], max_voxels=8192, max_iteration=3)
    pts, init = dev(first[0]), dev(first[1])
    out = {}
    graph, types = captured(lambda: out.update(m.extend((pts, off), init, min_fitness=0.3)))
    # register_device's launches, the four launches of the choice (arange, fitness >= min_fitness, the -1 as a device
    # scalar, where) and the
    # insertion's launches; nothing else, and no memset or memcpy node
    assert types == {"kernel": 1 + 2 * (3 + 1) + EXTEND_CHOICE_KERNELS + _lib.MAP_INSERT_LAUNCHES}, types
    graph.replay()
    pts.copy_(dev(second[0]))
    init.copy_(dev(second[1]))
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits(kept(m), kept(eager))
    assert m.cursor.tolist() == eager.cursor.tolist() == [24000 + 16000, 6 + 8]
    assert bool((out["fitness"] > 0.3).all()) and bool((out["iterations"] == 3).all())


# ---- 11. alone and twice ----------------------------------------------------------------------------------------------

def test_the_same_insertion_twice_gives_the_same_bits():
    g = IK.general_split(np.float32)
    A, B, Cn = group(g, ["A"]), group(g, ["B"]), group(g, ["C_new"])
    a, b = kept(build_then_insert([A, B, Cn], max_voxels=512)), kept(build_then_insert([A, B, Cn], max_voxels=512))
    assert_same_bits(a, b)
    assert a["cursor"].tobytes() == b["cursor"].tobytes()
    # B alone, and B in one insertion with C_new: B's part of the map does not depend on what else is in the call
    both = kept(build_then_insert([A, joined([B, Cn])], max_voxels=512))
    assert_same_bits(both, a)
