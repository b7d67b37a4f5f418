"""Seen-through voxels on the MI355X: nsc_map_cast_rays, nsc_map_flag_rows and MapLocalizer.observe* / flag_rows_device /
carve* / resize_device against counts derived by hand (tests/map_rays_cases.py) and against the restatement
(tests/map_rays_restatement.py) run on the DEVICE's own records, so that every gate decision is made on the same bits.

Every comparison is exact: integers by torch.equal or ==, maps by bits (test_map_replace_gpu.assert_follows)."""
import numpy as np
import pytest
import torch

import map_rays_cases as RC
import map_rays_restatement as RR
from test_map_insert_gpu import assert_same_bits, captured, kept
from test_map_localize_gpu import dev, host, index_of, localizer
from test_map_replace_gpu import assert_follows

pytestmark = pytest.mark.gpu

CASES = RC.hand_cases()
CARVE_TORCH_KERNELS = 3                 # torch's part of carve_device: the NaN (a fill), the where, and crossed := 0 (a fill)


def _lib():
    from neural_spectral_codec_amd import _lib
    return _lib


def built(points, off, poses, **kw):
    m = localizer(**kw)
    m.build_device(dev(points), dev(off), dev(poses))
    return m


def device_map(m):
    """the kept map of a localizer as the restatement takes a map: the device's records, the index as a dict"""
    place = {k: p for k, p in index_of(dict(index=m.index.cpu().numpy()))[0].items() if p >= 0}
    return dict(voxels=m.voxels.cpu().numpy(), place=place, capacity=m.capacity,
                grid=(m.params.voxel_size, np.array(list(m.params.origin))))


def cast_abi(m, points, off, poses, ids=None, crossed=None, min_range=0.0, max_range=60.0, end_margin=None, gate=3.0,
             max_voxels=None):
    """nsc_map_cast_rays on host arrays -> (crossed, ray_stats) on the device; the stats start from a sentinel"""
    L = _lib()
    pts, o, T = dev(points), dev(np.asarray(off, np.int64)), dev(np.asarray(poses, np.float64))
    M = m.capacity if max_voxels is None else max_voxels
    crossed = torch.zeros(M, dtype=torch.int64, device="cuda") if crossed is None else crossed
    stats = torch.full((L.MAP_RAY_STATS,), -7, dtype=torch.int64, device="cuda")
    ray = L.MapRayParams(min_range, max_range, -1.0 if end_margin is None else end_margin, gate)
    L.call("nsc_map_cast_rays", pts.device, pts, L.MAP_DTYPE_F64 if pts.dtype == torch.float64 else L.MAP_DTYPE_F32,
           int(pts.shape[1]), o, len(off) - 1, len(points), T, len(poses), None if ids is None else dev(ids), m.params,
           m.voxels if M else None, m.index if M else None, M, ray, crossed, stats, L.STREAM)
    return crossed, stats


def formatted(points, dtype, cols):
    p = np.asarray(points).astype(dtype)
    return p if cols == 3 else np.concatenate([p, np.full((len(p), 1), np.nan, dtype)], 1)


@pytest.fixture(scope="module")
def hand():
    return built(*RC.hand_map(), voxel_size=1.0, max_voxels=64)


@pytest.fixture(scope="module", params=[1.0, 0.5])
def scene_map(request):
    """(voxel size, an insertable localizer with the scene's six clouds, the scene's tensors on the device)"""
    s = RC.scene()
    m = localizer(voxel_size=request.param, max_voxels=16384, insertable=True)
    d = (dev(s["points"]), dev(s["offsets"]), dev(s["poses"]))
    m.build_device(*d)
    assert m.stats[0].item() == m.stats[1].item() < 16384
    return request.param, m, d


# ---- 1. the hand-derived cases through the C ABI ----------------------------------------------------------------------

@pytest.mark.parametrize("dtype,cols", [(np.float32, 3), (np.float32, 4), (np.float64, 3)])
def test_hand_cases_through_the_abi(hand, dtype, cols):
    n = int(hand.stats[1])
    keys = hand.keys[:n].cpu().numpy()
    assert n == len(RC.PLANES) + len(RC.BLOBS) and bool((hand.voxels[:n, 15] == 1.0).all())
    for c in CASES:
        crossed, stats = cast_abi(hand, formatted(c["points"], dtype, cols), c["offsets"], c["poses"], c["pose_ids"], **c["ray"])
        assert RC.crossed_by_voxel(crossed[:n].tolist(), keys) == c["crossed"], c["name"]
        assert stats.tolist() == c["stats"] and not bool(crossed[n:].any()), (c["name"], stats.tolist())


# ---- 2. the scene against the restatement on the device's records -----------------------------------------------------

def test_scene_equals_the_restatement(scene_map):
    voxel, m, _ = scene_map
    s = RC.scene()
    crossed, stats = cast_abi(m, s["points"], s["offsets"], s["poses"])
    ref = RR.cast(s["points"], s["offsets"], s["poses"], None, device_map(m), walked=RC.scene_walks(voxel))
    print(f"voxel {voxel}: stats {stats.tolist()}, closest gate decision {ref['closest_gate']:.3g} (relative), closest "
          f"stop {ref['closest_stop']:.3g}; no ray is left out")
    assert stats.tolist() == ref["stats"] and ref["rays_truncated"] == 0 and ref["crossings"] > 1000
    assert torch.equal(crossed.cpu(), torch.tensor(ref["crossed"], dtype=torch.int64))


# ---- 3. shapes --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_ray_counts_and_an_empty_cloud(scene_map, n):
    """the sweep of 256 lanes; the n rays come as three clouds of which the middle one has no rows"""
    voxel, m, _ = scene_map
    s = RC.scene()
    a, b = int(s["offsets"][3]), int(s["offsets"][4])
    rows = np.concatenate([s["points"][a:a + n // 2], s["points"][b:b + n - n // 2]])
    off, ids = np.array([0, n // 2, n // 2, n]), np.array([3, 0, 4])
    crossed, stats = cast_abi(m, rows, off, s["poses"], ids)
    ref = RR.cast(rows, off, s["poses"], ids, device_map(m))
    assert stats.tolist() == ref["stats"] and ref["rays_cast"] == n
    assert crossed.tolist() == ref["crossed"]


def test_a_map_of_no_voxels(hand):
    c = CASES[0]
    crossed, stats = cast_abi(hand, c["points"], c["offsets"], c["poses"], max_voxels=0, **c["ray"])
    assert stats.tolist() == [1, 0, 0, 0, 0, 8, 0, 0] and crossed.numel() == 0
    L = _lib()
    flags = torch.full((1,), True, device="cuda")
    fstats = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    L.call("nsc_map_flag_rows", flags.device, dev(c["points"]), L.MAP_DTYPE_F64, 3, dev(c["offsets"]), 1, 1, dev(c["poses"]), 1,
           None, hand.params, None, None, None, 0, 3, 0.5, flags, fstats, L.STREAM)
    assert fstats.tolist() == [0, 0, 0, 1] and not bool(flags.any())


def test_grid_wrap_and_accumulation(hand):
    """more rays than the cast's grid holds at once (NSC_MAP_INSERT_BLOCKS workgroups of NSC_MAP_INSERT_ROWS rays), each of
    three steps: from x = 1.75 through the plane of voxel 2 into voxel 3, and from x = 4.75 through the plane of voxel 5
    into voxel 6, within 0.15 m of the planes' centres (s < 0.5).  One call equals two halves into one ``crossed``"""
    L = _lib()
    n = L.MAP_INSERT_ROWS * L.MAP_INSERT_BLOCKS + 50_001
    rng = np.random.default_rng(3)
    rows = (np.array([2.0, 0, 0]) + rng.uniform(-0.3, 0.3, (n, 3))).astype(np.float32)
    rows[:, 0] = np.clip(rows[:, 0], 1.8, 2.2)                            # the end stays inside voxel 3 or 6
    n1 = n // 3
    off, poses = np.array([0, n1, n]), np.stack([np.eye(4), np.eye(4)])
    poses[0, :3, 3], poses[1, :3, 3] = (1.75, 0.5, 0.5), (4.75, 0.5, 0.5)
    crossed, stats = cast_abi(hand, rows, off, poses, end_margin=0.0)
    keys = hand.keys[:int(hand.stats[1])].cpu().numpy()
    assert RC.crossed_by_voxel(crossed.tolist(), keys) == {(2, 0, 0): n1, (5, 0, 0): n - n1}
    assert stats.tolist() == [n, 0, 0, 0, 0, 3 * n, n, 0]
    h = n // 2 + 7
    half, st1 = cast_abi(hand, rows[:h], np.array([0, n1, h]), poses, end_margin=0.0)
    half, st2 = cast_abi(hand, rows[h:], np.array([0, n - h]), poses[1:], crossed=half, end_margin=0.0)
    assert torch.equal(half, crossed) and (st1 + st2).tolist() == stats.tolist()


# ---- 4. determinism ---------------------------------------------------------------------------------------------------

def test_two_calls_cloud_order_and_batches_agree(scene_map):
    voxel, m, _ = scene_map
    s = RC.scene()
    off = s["offsets"]
    whole, stats = cast_abi(m, s["points"], off, s["poses"])
    again, stats2 = cast_abi(m, s["points"], off, s["poses"])
    assert torch.equal(whole, again) and torch.equal(stats, stats2)
    parts = [s["points"][off[c]:off[c + 1]] for c in range(6)]
    back = np.concatenate(parts[::-1])
    boff = np.concatenate([[0], np.cumsum([len(p) for p in parts[::-1]])])
    rev, rstats = cast_abi(m, back, boff, s["poses"][::-1].copy())
    assert torch.equal(rev, whole) and torch.equal(rstats, stats)
    # a cloud alone contributes what it contributes inside the batch: the clouds one by one add up to the batch
    total, visited = None, 0
    for c in range(6):
        total, st = cast_abi(m, parts[c], np.array([0, len(parts[c])]), s["poses"][c:c + 1], crossed=total)
        visited += int(st[5])
    assert torch.equal(total, whole) and visited == int(stats[5])


# ---- 5. flags ---------------------------------------------------------------------------------------------------------

def test_flag_rows_equal_the_restatement_and_seen_through(scene_map):
    voxel, m, d = scene_map
    s = RC.scene()
    m.crossed = None
    out = m.observe_device(*d)
    assert out["crossed"] is m.crossed and int(out["ray_stats"][0]) == len(s["points"])
    got = m.flag_rows_device(*d)
    dm = device_map(m)
    flags, fstats = RR.flag_rows(s["points"], s["offsets"], s["poses"], None, dm, m.info[:, 0].tolist(), m.crossed.tolist())
    assert got["row_flags"].dtype == torch.bool and np.array_equal(got["row_flags"].cpu().numpy(), flags)
    assert got["flag_stats"].tolist() == fstats and fstats[0] > 500 and fstats[2:] == [0, 0]
    place = RC.rows_place(dm, s)
    seen = m.seen_through().cpu().numpy()
    assert bool((place >= 0).all()) and np.array_equal(seen[place], flags)
    assert np.array_equal(seen, RR.seen_through(m.info[:, 0].tolist(), m.crossed.tolist()))
    # a second observation accumulates; the host form reads the counts
    named = m.observe((d[0], d[1]), s["poses"])
    assert named["rays_cast"] == len(s["points"]) and named["rays_truncated"] == 0
    assert torch.equal(m.crossed, 2 * cast_abi(m, s["points"], s["offsets"], s["poses"])[0])
    m.crossed = None


# ---- 6. carving -------------------------------------------------------------------------------------------------------

def rebuilt_without(s, carved, clouds, voxel):
    """a fresh build over ``clouds`` of the scene with their carved rows NaN -> its buffers on the host"""
    a, b = int(s["offsets"][clouds[0]]), int(s["offsets"][clouds[-1] + 1])
    pts = RR.without(s["points"], carved)[a:b]
    off = s["offsets"][clouds[0]:clouds[-1] + 2] - a
    return host(localizer(voxel_size=voxel, max_voxels=16384).build_device(dev(pts), dev(off), dev(s["poses"][clouds]),
                                                                           moments=True))


def test_carve_leaves_the_rebuild_over_the_rows_kept():
    voxel, s = 1.0, RC.scene()
    n = len(s["points"])
    m = localizer(voxel_size=voxel, max_voxels=16384, insertable=True)
    d = (dev(s["points"]), dev(s["offsets"]), dev(s["poses"]))
    m.build_device(*d)
    m.observe_device(*d)
    flags, _ = RR.flag_rows(s["points"], s["offsets"], s["poses"], None, device_map(m), m.info[:, 0].tolist(),
                            m.crossed.tolist())
    res = m.carve((d[0], d[1]), s["poses"])
    carved = res["carved"].cpu().numpy()
    k = int(carved.sum())
    assert np.array_equal(carved, flags) and k > 500
    assert (res["rows_removed"], res["removed_not_finite"], res["removed_outside"], res["removed_without_pose"],
            res["rows_missing"], res["voxels_inconsistent"]) == (k, n - k, 0, 0, 0, 0)
    assert (res["rows_flagged"], res["rows_kept"], res["rows_dropped"], res["rows_without_voxel"]) == (k, n - k, 0, 0)
    assert res["voxels_emptied"] > 0 and res["rows_used"] == n - k and not bool(m.crossed.any())
    emptied = assert_follows(kept(m), rebuilt_without(s, carved, list(range(6)), voxel), "carved")
    assert len(emptied) == res["voxels_emptied"]
    box = s["is_box"]
    print(f"carved {k} rows: {carved[box].mean():.3f} of the box rows, {carved[~box].mean():.4f} of the others")
    # the documented way to move or remove a carved cloud: its carved rows NaN
    a = int(s["offsets"][1])
    out = m.remove_device(m.without(d[0][:a], res["carved"][:a]), d[1][:2], d[2][:1])
    k0 = int(carved[:a].sum())
    assert out["removed"].tolist()[:5] == [a - k0, k0, 0, 0, 0] and int(out["removed"][7]) == 0
    assert_follows(kept(m), rebuilt_without(s, carved, [1, 2, 3, 4, 5], voxel), "cloud 0 removed")


# ---- 7. resizing with counts ------------------------------------------------------------------------------------------

def by_key(m):
    """{key: crossed} of the voxels with a place"""
    crossed = m.crossed.tolist()
    return {k: crossed[p] for k, p in index_of(dict(index=m.index.cpu().numpy()))[0].items() if p >= 0}


@pytest.mark.parametrize("new", [4096, 40000])
def test_resize_carries_the_counts(new):
    s = RC.scene()
    d = (dev(s["points"]), dev(s["offsets"]), dev(s["poses"]))
    m, plain = (localizer(voxel_size=1.0, max_voxels=16384, insertable=True) for _ in range(2))
    for x in (m, plain):
        x.build_device(*d)
    m.observe_device(*d)
    before = by_key(m)
    assert sum(before.values()) > 1000
    out, want = m.resize_device(new), plain.resize_device(new)
    assert plain.crossed is None and set(out) == set(want)
    # what the method returns is what it returns without counts: the maps by bits where they are defined, the rest whole
    assert_same_bits(kept(m), kept(plain), "resized")
    for k in ("new_place", "tile_base", "rehashed", "stats", "cursor"):
        assert torch.equal(out[k], want[k]), k
    written = int(m.stats[1])
    assert m.crossed.shape == (new,) and by_key(m) == before and not bool(m.crossed[written:].any())
    again, _ = cast_abi(m, s["points"], s["offsets"], s["poses"])       # the counts stand where a cast into the new map puts them
    assert torch.equal(again, m.crossed)


# ---- 8. one graph -----------------------------------------------------------------------------------------------------

def test_observe_and_carve_captured_as_one_graph():
    L = _lib()
    s = RC.scene()
    d = (dev(s["points"]), dev(s["offsets"]), dev(s["poses"]))
    eager, m = (localizer(voxel_size=1.0, max_voxels=16384, insertable=True) for _ in range(2))
    for x in (eager, m):
        x.build_device(*d)
    eager.observe_device(*d)
    want = eager.carve_device(*d)
    m.observe_device(*d)                                     # ``crossed`` exists before the capture, and is zero again
    m.crossed.fill_(0)
    outs = {}

    def step():
        outs.update(m.observe_device(*d))
        outs.update(m.carve_device(*d))
    graph, types = captured(step)
    assert types == {"kernel": L.MAP_RAY_LAUNCHES + L.MAP_FLAG_LAUNCHES + CARVE_TORCH_KERNELS + L.MAP_REMOVE_LAUNCHES}, types
    assert int(m.stats[2]) == len(s["points"])              # a capture carves nothing
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits(kept(m), kept(eager), "replayed")
    for k in ("carved", "removed", "flag_stats"):
        assert torch.equal(outs[k], want[k]), k
    assert int(outs["carved"].sum()) > 500 and not bool(m.crossed.any())
    assert int(outs["ray_stats"][0]) == len(s["points"])


# ---- 9. the store forms -----------------------------------------------------------------------------------------------

def test_store_forms_equal_the_device_forms():
    """observe_prepared over two ranges of a PreparedClouds and carve_prepared against observe_device and carve_device on
    the store's packed rows"""
    from neural_spectral_codec_amd.retrieval import PreparedClouds
    s = RC.scene()
    off = s["offsets"]
    store = PreparedClouds(voxel_size=0.25)
    store.add([s["points"][off[i]:off[i + 1]] for i in range(6)])
    a, b = (localizer(voxel_size=1.0, max_voxels=16384, insertable=True) for _ in range(2))
    pts, o = store.packed()
    poses = dev(s["poses"])
    a.build_prepared(store, s["poses"])
    b.build_device(pts, o, poses)
    first = a.observe_prepared(store, s["poses"][:3], stop=3)
    second = a.observe_prepared(store, s["poses"][3:], start=3)
    whole = b.observe_device(pts, o, poses)
    assert torch.equal(a.crossed, b.crossed) and int(a.crossed.sum()) > 1000
    assert first["rays_cast"] + second["rays_cast"] == int(whole["ray_stats"][0]) == store.n_rows
    assert first["crossings"] + second["crossings"] == int(whole["ray_stats"][6]) and first["rays_truncated"] == 0
    ra, rb = a.carve_prepared(store, s["poses"]), b.carve_device(pts, o, poses)
    assert torch.equal(ra["carved"], rb["carved"]) and ra["rows_removed"] == ra["rows_flagged"] == int(rb["removed"][0]) > 0
    assert ra["voxels_inconsistent"] == 0 and not bool(a.crossed.any())
    assert_same_bits(kept(a), kept(b), "store forms")
    for call in (lambda: a.observe_prepared(store, s["poses"], start=4, stop=3), lambda: a.carve_prepared(store, s["poses"], stop=7)):
        with pytest.raises(_lib().NscError, match="start and stop"):
            call()
