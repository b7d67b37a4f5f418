"""Resizing and compacting a kept map on the MI355X: MapLocalizer.resize_device / resize / fit and nsc_map_rehash_dist
against a fresh build at the new capacity, against the restated move (tests/map_rehash_restatement.py) and against the
source map, on the constructed inputs of tests/map_insert_cases.py, tests/map_replace_cases.py and
tests/map_localize_cases.py, whose claims tests/test_map_rehash_cpu.py and the CPU files of those cases assert.

Every comparison is by bits: nothing is computed by the move, so there are no tolerances.  With a rebuild over the same
rows it is ``assert_same_bits``; after a compaction, whose places are not the rebuild's, it is a comparison of mappings
key -> (count, moments, record); the index is always read as a mapping key -> place."""
import numpy as np
import pytest
import torch

import map_insert_cases as IK
import map_localize_cases as K
import map_rehash_restatement as HR
import workspace_contract as W
from test_map_insert_cpu import group, joined
from test_map_insert_gpu import (GUARD, KEPT, SENTINEL, assert_guards, assert_same_bits, build_then_insert, captured, guarded,
                                 kept, rebuilt, scene_parts)
from test_map_localize_gpu import dev, index_of, localizer
from test_map_replace_gpu import assert_follows, mapping

pytestmark = pytest.mark.gpu

FORMATS = [(np.float32, 3), (np.float32, 4), (np.float64, 3)]
OUTS = ("new_place", "tile_base", "rehashed")
REGISTERED = ("transform", "fitness", "rmse", "cost", "n_correspondences", "iterations", "information")
EMPTY = np.uint64(2 ** 64 - 1)


def devs(part):
    return tuple(dev(x) for x in part)


def four_groups(dtype=np.float32, cols=3):
    g = IK.general_split(dtype, cols)
    return [group(g, [n]) for n in ("A", "B", "C_old", "C_new")]


def resized(m, *args, **kw):
    """resize_device -> (the kept tensors on the host, the three typed outputs on the host)"""
    out = m.resize_device(*args, **kw)
    for k in KEPT + ("index", "stats", "cursor"):
        assert out[k] is getattr(m, k), k
    return kept(m), {k: out[k].cpu().numpy() for k in OUTS}


def assert_restated(got, outs, ref, what=""):
    """the kept tensors and typed outputs of a move equal the restatement's: every entry where every entry is defined
    (stats, cursor, new_place, tile_base, rehashed, the index), the first stats[1] entries elsewhere"""
    assert got["stats"].tolist() == ref["stats"].tolist(), (what, got["stats"], ref["stats"])
    for k in OUTS:
        assert np.array_equal(outs[k], ref[k]), (what, k, outs[k], ref[k])
    n = int(ref["stats"][1])
    for k in KEPT:
        assert got[k][:n].tobytes() == ref[k][:n].tobytes(), (what, k)
    if "cursor" in ref:
        assert got["cursor"].tolist() == ref["cursor"].tolist(), what
    idx = got["index"].view(np.uint64)
    assert (idx[idx[:, 0] == 0, 1] == EMPTY).all(), what                 # an empty slot is (0, ~0)
    assert not (idx[idx[:, 1] != EMPTY, 1] >> np.uint64(36)).any(), what  # a place, no flag bits
    places, occupied = index_of(got)
    if ref["place"] is not None:
        assert places == ref["place"] and occupied == len(ref["place"]), what


# ---- 1. growth equals the build ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,cols", FORMATS)
def test_growth_equals_the_build(dtype, cols):
    parts = four_groups(dtype, cols)
    m = build_then_insert(parts, max_voxels=512)
    src = kept(m)
    found = int(src["stats"][0])
    got, outs = resized(m, 2048)
    assert_same_bits(got, rebuilt(parts, max_voxels=2048), "grown")
    assert got["cursor"].tolist() == src["cursor"].tolist() == [3200, 8]
    assert (m.capacity, m.max_voxels, m.complete) == (2048, 2048, None) and tuple(m.index.shape) == (4096, 2)
    assert_restated(got, outs, HR.rehash(src, False, 2048), "grown")
    assert outs["rehashed"].tolist() == [found, 0, 0, 0, 0, 0]
    # the same capacity: the source again
    m = build_then_insert(parts, max_voxels=512)
    got, outs = resized(m)
    assert_same_bits(got, src, "same capacity")
    assert got["cursor"].tobytes() == src["cursor"].tobytes() and m.capacity == 512
    assert outs["new_place"].tolist() == list(range(found)) + [-1] * (512 - found)
    assert outs["tile_base"].tolist() == [0, found]
    # the tightest fit
    m = build_then_insert(parts, max_voxels=512)
    got, outs = resized(m, found)
    assert_same_bits(got, rebuilt(parts, max_voxels=found), "tightest")
    assert got["stats"][:2].tolist() == [found, found] and outs["rehashed"].tolist() == [found, 0, 0, 0, 0, 0]


# ---- 2. insertion after growth ----------------------------------------------------------------------------------------

def test_insertion_after_growth_equals_the_build_and_fails_without_it():
    A, B = four_groups()[:2]
    own = int(rebuilt([A], max_voxels=512)["stats"][0])
    m = build_then_insert([A], max_voxels=own)
    m.resize_device(2048)
    m.insert_device(*devs(B))
    got = kept(m)
    assert_same_bits(got, rebuilt([A, B], max_voxels=2048), "resized, then B")
    assert got["stats"][0] == got["stats"][1] > own
    # the same insertion into the map as it was built: the new voxels are found and have no place
    short = kept(build_then_insert([A, B], max_voxels=own))
    assert short["stats"][0] == got["stats"][0] > short["stats"][1] == own


# ---- 3. compaction ----------------------------------------------------------------------------------------------------

def removed_map(parts, gone, **kw):
    m = build_then_insert([joined(parts)], max_voxels=512, **kw)
    for part in gone:
        m.remove_device(*devs(part))
    return m


@pytest.mark.parametrize("dtype,cols", FORMATS)
def test_compaction_equals_the_rebuild_over_what_remains(dtype, cols):
    A, B, Co, Cn = parts = four_groups(dtype, cols)
    src = kept(removed_map(parts, [Cn, B]))
    emptied, bad = HR.kinds(src)
    n_emptied, written = int(emptied.sum()), int(src["stats"][1])
    assert n_emptied > 10 and not bad.any()
    left = int(rebuilt([A, Co], max_voxels=512)["stats"][0])
    assert left == written - n_emptied
    for size in (left, 512):                                              # the fitted size, then the source's
        m = removed_map(parts, [Cn, B])
        got, outs = resized(m, size, compact=True)
        want = rebuilt([A, Co], max_voxels=size)
        assert mapping(got) == mapping(want) and len(mapping(got)) == left, size
        assert got["stats"][:2].tolist() == want["stats"][:2].tolist() == [left, left]
        assert got["stats"][2:].tolist() == src["stats"][2:].tolist() and got["cursor"].tolist() == src["cursor"].tolist()
        old = np.nonzero(~emptied)[0]
        assert outs["new_place"][old].tolist() == list(range(left))      # strictly increasing on the kept places
        assert (outs["new_place"][np.nonzero(emptied)[0]] == -1).all() and (outs["new_place"][written:] == -1).all()
        assert np.array_equal(got["info"][:left, 1:], src["info"][old, 1:]) and (np.diff(got["info"][:left, 1]) > 0).all()
        assert outs["rehashed"].tolist() == [left, n_emptied, 0, 0, 0, 0]
        assert_restated(got, outs, HR.rehash(src, False, size), size)
    # the removed clouds inserted again into the compacted map of 512: the map over all four
    m.insert_device(*devs(Cn))
    m.insert_device(*devs(B))
    again, whole = kept(m), rebuilt(parts, max_voxels=512)
    assert mapping(again) == mapping(whole) and again["stats"][0] == again["stats"][1] == whole["stats"][0]
    assert again["stats"][2:].tolist() == whole["stats"][2:].tolist()
    # without compaction the places stay
    m = removed_map(parts, [Cn, B])
    got, outs = resized(m, compact=False)
    assert got["stats"].tobytes() == src["stats"].tobytes() and outs["rehashed"].tolist() == [written, 0, 0, 0, 0, 0]
    assert len(assert_follows(got, rebuilt([A, Co], max_voxels=512), "kept emptied")) == n_emptied
    assert_same_bits(got, src, "kept emptied")


# ---- 4. registration --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("options", [dict(), dict(kernel="cauchy", robust_scale=3.0, neighbours=7)],
                         ids=["plain", "cauchy-7"])
def test_registration_is_the_same_before_and_after_a_resize(options):
    s = K.scene()
    scans = (dev(s["scans"]), dev(s["scan_offsets"]))

    def registered(m):
        out = m.register(scans, s["init"])
        return {k: out[k] for k in REGISTERED}

    def same(a, b, what):
        for k in REGISTERED:
            assert torch.equal(a[k], b[k]), (what, k)
    m = build_then_insert([scene_parts(0, 6)], max_voxels=8192, **options)
    before = registered(m)
    assert bool((before["n_correspondences"] > 1000).all())
    m.resize_device(16384)
    same(registered(m), before, "grown")
    whole = localizer(max_voxels=16384, **options)
    whole.build_device(*devs(scene_parts(0, 6)))
    same(registered(whole), before, "grown, against the rebuild")
    # two clouds removed, then compacted to the source's first capacity
    m.remove_device(*devs(scene_parts(4, 6)))
    removed = registered(m)
    out = m.resize_device(8192, compact=True)
    assert int(out["rehashed"][1]) >= 1 and int(out["rehashed"][4]) == 0
    same(registered(m), removed, "compacted")
    rest = localizer(max_voxels=8192, **options)
    rest.build_device(*devs(scene_parts(0, 4)))
    same(registered(rest), removed, "compacted, against the rebuild")


# ---- 5. sizes ---------------------------------------------------------------------------------------------------------

def lattice_map(n):
    """n clouds of one row, each alone in a voxel of 1 m, every third cloud removed again -> the localizer"""
    i = np.arange(n)
    pts = np.stack([i % 64, (i // 64) % 64, i // 4096], 1) + 0.5
    off, poses = np.arange(n + 1, dtype=np.int64), np.tile(np.eye(4), (n, 1, 1))
    m = localizer(insertable=True, max_voxels=max(n, 1), min_points=1)
    m.build_device(dev(pts), dev(off), dev(poses))
    m.remove_device(dev(pts), dev(off), dev(poses), dev(np.where(i % 3 == 0, i, -1)))
    return m


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_sizes_equal_the_restatement(n):
    """the wave of 64 places, the sweep of 256 and the tile of 4096; every third place is emptied, so the tiles' counts
    differ"""
    gone = (n + 2) // 3
    for size in (max(n, 1), max(n - gone, 1)):
        m = lattice_map(n)
        src = kept(m)
        assert src["stats"][:3].tolist() == [n, n, n - gone]
        got, outs = resized(m, size)
        assert outs["rehashed"].tolist() == [n - gone, gone, 0, 0, 0, 0]
        assert outs["tile_base"].shape == (-(-max(n, 1) // 4096) + 1,) and outs["tile_base"][-1] == n - gone
        assert_restated(got, outs, HR.rehash(src, False, size), (n, size))


# ---- 6. a destination that is too small -------------------------------------------------------------------------------

def test_destination_too_small_is_the_build_overflow():
    parts = four_groups()
    m = build_then_insert(parts, max_voxels=512)
    src = kept(m)
    found = int(src["stats"][0])
    size = (3 * found) // 5
    assert size < found <= 2 * size
    got, outs = resized(m, size)
    assert got["stats"][:2].tolist() == [found, size] and outs["rehashed"].tolist() == [found, 0, 0, 0, found - size, 0]
    assert_same_bits(got, rebuilt(parts, max_voxels=size), "against the build that overflows")
    places, occupied = index_of(got)
    assert occupied == found and [places[int(k)] for k in src["keys"][:found]] == list(range(size)) + [-1] * (found - size)
    assert outs["new_place"].tolist() == list(range(size)) + [-1] * (512 - size)
    assert_restated(got, outs, HR.rehash(src, False, size))
    # after a removal: the kept voxels in front take the places
    m = removed_map(parts, [parts[3]])
    src = kept(m)
    ref = HR.rehash(src, False, size)
    assert size < ref["rehashed"][0] <= 2 * size and ref["rehashed"][1] > 10
    got, outs = resized(m, size)
    assert_restated(got, outs, ref, "removed, then too small")
    assert outs["rehashed"][4] == ref["rehashed"][0] - size == got["stats"][0] - got["stats"][1]


def rehash_views(M, N, with_cursor=True):
    """``guarded``'s scheme for a move from capacity M to N: the destination tensors and the three typed outputs, each
    with GUARD sentinel elements behind it -> (the views to move into, the whole, the shapes)"""
    views, big, shapes = guarded(N)
    extra = dict(new_place=(M,), tile_base=(-(-M // 4096) + 1,), rehashed=(6,))
    for k, s in extra.items():
        big[k] = torch.full((s[0] + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
        views[k] = big[k][:s[0]]
    shapes.update(extra)
    if not with_cursor:
        for d in (views, big, shapes):
            del d["cursor"]
    return views, big, shapes


def test_more_kept_voxels_than_slots_keeps_its_counts_and_its_bounds():
    parts = four_groups()
    m = build_then_insert(parts, max_voxels=512)
    found = int(m.stats[0])
    size = found // 3
    assert found > 2 * size
    views, big, shapes = rehash_views(512, size)
    got, outs = resized(m, size, out=views)
    r = outs["rehashed"].tolist()
    assert r == [found, 0, 0, 0, found - size, found - 2 * size] and got["stats"][:2].tolist() == [found, size]
    assert index_of(got)[1] == 2 * size                                 # every slot keyed
    assert outs["new_place"].tolist() == list(range(size)) + [-1] * (512 - size)
    assert_guards(big, shapes)


# ---- 7. an inconsistent voxel -----------------------------------------------------------------------------------------

def test_an_inconsistent_voxel_survives_a_compaction_with_its_integers():
    """test_map_replace_gpu.test_a_cloud_removed_twice_leaves_zero_records: B removed twice leaves -7 rows in its own five
    voxels"""
    A, B, vox = IK.twelve_voxels()
    m = build_then_insert([A, A, B], max_voxels=16, max_iteration=0)
    for _ in range(2):
        m.remove_device(*devs(B))
    src = kept(m)
    got, outs = resized(m, 12, compact=True)
    assert outs["rehashed"].tolist() == [12, 0, 0, 5, 0, 0]
    assert_restated(got, outs, HR.rehash(src, False, 12))
    at = [index_of(got)[0][IK.voxel_key(v)] for v in vox]
    assert got["info"][at, 0].tolist() == [14] * 4 + [7] * 3 + [-7] * 5
    assert got["voxels"][at[7:]].tobytes() == bytes(128 * 5) and got["moments"][at[7:]].any(1).all()
    for _ in range(2):
        m.insert_device(*devs(B))
    assert mapping(kept(m)) == mapping(kept(build_then_insert([A, A, B], max_voxels=16)))


# ---- 8. poisoned, exact-size outputs ----------------------------------------------------------------------------------

@pytest.mark.parametrize("insertable", [True, False])
def test_poisoned_exact_size_outputs(insertable):
    """every output between sentinel guards and filled with each pattern before the call: nothing is read before it is
    written, nothing is written past its end, and what is defined in every entry equals the restatement in every entry.
    A map that is not insertable is moved without moments and cursor"""
    A, B, Co, Cn = parts = four_groups()
    results = []
    for pattern in W.PATTERNS:
        if insertable:
            m = removed_map(parts, [Cn])
        else:
            m = localizer(max_voxels=512)
            m.build_device(*devs(joined(parts)))
        src = kept(m)
        views, big, shapes = rehash_views(512, 300, with_cursor=insertable)
        if not insertable:
            for d in (views, big, shapes):
                del d["moments"]
        for t in views.values():
            t.view(torch.uint8).fill_(pattern)
        out = m.resize_device(300, out=views)
        assert all(out[k] is views[k] for k in views)
        got = {k: v.cpu().numpy() for k, v in views.items()}
        outs = {k: got[k] for k in OUTS}
        ref = HR.rehash(src, False, 300)
        n = int(ref["stats"][1])
        assert got["stats"].tolist() == ref["stats"].tolist() and n == (int(src["stats"][1]) - int(ref["rehashed"][1]))
        for k in OUTS:
            assert np.array_equal(outs[k], ref[k]), (pattern, k)
        for k in KEPT:
            assert (k in got) == (k in ref) and (k not in got or got[k][:n].tobytes() == ref[k][:n].tobytes()), (pattern, k)
        idx = got["index"].view(np.uint64)
        assert (idx[idx[:, 0] == 0, 1] == EMPTY).all() and index_of(got) == (ref["place"], n)
        assert_guards(big, shapes)
        results.append(got)
    assert (int(ref["rehashed"][1]) > 10) == insertable
    for other in results[1:]:
        for k in ("stats",) + OUTS + (("cursor",) if insertable else ()):
            assert other[k].tobytes() == results[0][k].tobytes(), k
        for k in KEPT:
            assert k not in other or other[k][:n].tobytes() == results[0][k][:n].tobytes(), k
        assert index_of(other) == index_of(results[0])


# ---- 9. capture and repeatability -------------------------------------------------------------------------------------

def test_captured_resize_replays_to_the_same_bits():
    from neural_spectral_codec_amd import _lib
    parts = four_groups()
    eager = removed_map(parts, [parts[3]])
    want, want_outs = resized(eager, 1024)
    m = removed_map(parts, [parts[3]])
    source = m._kept()                                                   # the graph reads these: they stay alive
    views, big, shapes = rehash_views(512, 1024)
    graph, types = captured(lambda: m.resize_device(1024, out=views))
    assert types == {"kernel": _lib.MAP_REHASH_LAUNCHES}, types
    assert m.voxels is views["voxels"] and m.capacity == 1024
    for _ in range(2):
        for t in views.values():
            t.view(torch.uint8).fill_(0x3C)
        graph.replay()
        torch.cuda.synchronize()
        got = kept(m)
        assert_same_bits(got, want, "replayed")
        assert got["cursor"].tobytes() == want["cursor"].tobytes()
        for k in OUTS:
            assert np.array_equal(views[k].cpu().numpy(), want_outs[k]), k
    assert_guards(big, shapes)
    assert len(source) == 7


def test_the_same_sequence_twice_gives_the_same_bits():
    A, B, Co, Cn = four_groups()

    def sequence():
        m = build_then_insert([A, B, Co], max_voxels=256)
        m.insert_device(*devs(Cn))
        m.remove_device(*devs(B))
        out = m.resize_device(384)
        return kept(m), {k: out[k].cpu().numpy() for k in OUTS}
    (a, oa), (b, ob) = sequence(), sequence()
    assert_same_bits(a, b)
    assert a["cursor"].tobytes() == b["cursor"].tobytes()
    for k in OUTS:
        assert oa[k].tobytes() == ob[k].tobytes(), k
    assert mapping(a) == mapping(rebuilt([A, Co, Cn], max_voxels=384))


# ---- 10. the host forms -----------------------------------------------------------------------------------------------

def test_resize_and_fit_on_the_host():
    from neural_spectral_codec_amd import _lib
    parts = four_groups()
    m = localizer(insertable=True)                                       # max_voxels=None: one voxel of capacity per row
    p, o, T = joined(parts)
    res = m.build((dev(p), dev(o)), T)
    found = res["voxels_found"]
    assert m.capacity == 3200 and res["complete"]
    res = m.fit(headroom=1.5)
    assert m.capacity == m.max_voxels == -(-3 * found // 2) and res["complete"] and m.complete
    assert [res[k] for k in _lib.MAP_REHASH_STAT_NAMES] == [found, 0, 0, 0, 0, 0]
    assert res["count"].shape[0] == found and tuple(m.voxels.shape) == (m.capacity, 16)
    assert_same_bits(kept(m), rebuilt(parts, max_voxels=m.capacity), "fitted")
    m.remove((dev(parts[3][0]), dev(parts[3][1])), parts[3][2])
    res = m.resize(compact=True)
    assert res["voxels_dropped"] > 10 and res["voxels_found"] == res["voxels_kept"] == found - res["voxels_dropped"]
    assert not bool((res["count"] == 0).any())
    res = m.fit()
    assert m.capacity == res["voxels_written"] == res["voxels_kept"] and res["complete"]
