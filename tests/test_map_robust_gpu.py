"""Robust weights and face-neighbour voxels in map localisation on the MI355X: nsc_map_register_robust and ``MapLocalizer``
with ``kernel`` / ``robust_scale`` / ``neighbours`` against nsc_map_register (by bits, without options) and against the
restatement (tests/map_robust_restatement.py) on the inputs of tests/map_robust_cases.py, whose claims
tests/test_map_robust_cpu.py asserts.

Bars that are not exact:
  systems     the project's 1e-6 relative bar for system terms (tests/test_map_localize_gpu.py)
  end to end  to the restatement ten times what +-2^-24 m on every scan coordinate changes in the restatement's own
              result for that configuration, over the scans the restatement finishes before max_iteration (at least 7 of
              8); to the truth twice the restatement's own worst error.  Both come from map_robust_cases.reference
"""
import ctypes as C

import numpy as np
import pytest
import torch

import map_localize_cases as K
import map_localize_restatement as R
import map_robust_cases as KR
import map_robust_restatement as RR

pytestmark = pytest.mark.gpu

PLAIN_KEYS = {"transform", "fitness", "rmse", "cost", "n_correspondences", "iterations", "information"}


def localizer(**kw):
    from neural_spectral_codec_amd.retrieval import MapLocalizer
    return MapLocalizer(**kw)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def options(kernel, scale, neighbours):
    return dict(kernel=kernel, robust_scale=scale, neighbours=neighbours)


def with_options(m, **kw):
    """a localizer with ``m``'s kept map and the given registration options"""
    o = localizer(voxel_size=m.params.voxel_size, origin=tuple(m.params.origin), max_voxels=m.max_voxels,
                  max_iteration=m.reg.max_iteration, **kw)
    o.voxels, o.index, o.keys, o.info, o.stats, o.capacity = m.voxels, m.index, m.keys, m.info, m.stats, m.capacity
    return o


def robust_entry(m, points, offsets, init, kernel=0, neighbours=1, scale=0.0):
    """nsc_map_register_robust itself on device tensors, system0 included -> register_device's dict and weight_pairs: the
    way to the new entry with NONE and one voxel, which ``MapLocalizer`` sends to nsc_map_register"""
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval.geometric_verification import _workspace
    S, N = int(offsets.numel()) - 1, int(points.shape[0])
    f64 = dict(dtype=torch.float64, device=points.device)
    T, fr, cost = torch.empty((S, 4, 4), **f64), torch.empty((S, 2), **f64), torch.empty((S,), **f64)
    ci = torch.empty((S, 2), dtype=torch.int64, device=points.device)
    info, sys0, wp = torch.empty((S, 6, 6), **f64), torch.empty((S, 32), **f64), torch.empty((S, 2), **f64)
    L = _lib.lib()
    ws = _workspace(L.nsc_map_register_robust_workspace_bytes(S), points.device)
    rob = _lib.MapRobustParams(kernel=kernel, neighbours=neighbours, scale=scale)
    status = L.nsc_map_register_robust(
        _lib.ptr(points), _lib.MAP_DTYPE_F64 if points.dtype == torch.float64 else _lib.MAP_DTYPE_F32,
        int(points.shape[1]), _lib.ptr(offsets), S, N, _lib.ptr(m.voxels), _lib.ptr(m.index), m.capacity,
        C.byref(m.params), C.byref(m.reg), C.byref(rob), _lib.ptr(init), _lib.ptr(T), _lib.ptr(fr), _lib.ptr(cost),
        _lib.ptr(ci), _lib.ptr(info), _lib.ptr(sys0), _lib.ptr(wp), _lib.ptr(ws), int(ws.numel()),
        _lib.stream_ptr(points.device))
    _lib.check(status, "nsc_map_register_robust")
    return dict(transform=T, fitness=fr[:, 0], rmse=fr[:, 1], cost=cost, n_correspondences=ci[:, 0], iterations=ci[:, 1],
                information=info, system0=sys0, weight_pairs=wp)


def close(got, ref):
    return np.allclose(got, ref, rtol=1e-6, atol=1e-6 * max(np.abs(ref).max(), 1e-300))


@pytest.fixture(scope="module")
def scene_map():
    s = K.scene()
    m = localizer(voxel_size=1.0)
    assert m.build(list(np.split(s["points"], 6)), s["poses"])["complete"]
    return m


@pytest.fixture(scope="module")
def wide_map():
    s = K.scene()
    m = localizer(voxel_size=0.5)
    assert m.build(list(np.split(s["points"], 6)), s["poses"])["complete"]
    return m


@pytest.fixture(scope="module")
def ten_map():
    pts, off, poses, vox = K.ten_voxels()
    m = localizer(max_voxels=6, max_iteration=0)
    m.build_device(dev(pts), dev(off), dev(poses))
    return m, R.build_dist(pts, off, poses, max_voxels=6), vox


# ---- 1. without options: nsc_map_register, by bits --------------------------------------------------------------------

def test_none_and_one_voxel_is_nsc_map_register_by_bits(scene_map, ten_map):
    s = K.scene()
    m10, _, vox = ten_map
    scan, _ = K.lookup_scan(vox)
    cases = [(scene_map, dev(s["scans"]), dev(s["scan_offsets"]), dev(s["init"])),
             (m10, dev(scan), dev(np.array([0, len(scan)], np.int64)), dev(np.eye(4)[None]))]
    for m, pts, off, init in cases:
        old = host(m.register_device(pts, off, init, system0=True))
        new = host(robust_entry(m, pts, off, init))
        assert set(old) == PLAIN_KEYS | {"system0"}
        for k in PLAIN_KEYS:
            assert new[k].tobytes() == old[k].tobytes(), k
        assert new["system0"][:, :30].tobytes() == old["system0"].tobytes()
        nc = old["n_correspondences"].astype(np.float64)
        assert np.array_equal(new["weight_pairs"][:, 0], nc) and np.array_equal(new["weight_pairs"][:, 1], nc)
        # system0 is the first round's: its two new sums are the first round's n_corr
        assert np.array_equal(new["system0"][:, 30], new["system0"][:, 27])
        assert np.array_equal(new["system0"][:, 31], new["system0"][:, 27])
    assert old["n_correspondences"].tolist() == [35]


def test_defaults_return_todays_keys(scene_map):
    s = K.scene()
    out = scene_map.register(list(np.split(s["scans"], 8))[:2], s["init"][:2])
    assert set(out) == PLAIN_KEYS
    out = scene_map.register(list(np.split(s["scans"], 8))[:2], s["init"][:2], system0=True)
    assert set(out) == PLAIN_KEYS | {"system0"} and tuple(out["system0"].shape) == (2, 30)


# ---- 2. one linearisation ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel,scale,neighbours", KR.SYSTEM_CONFIGS)
def test_system0_against_restatement(scene_map, kernel, scale, neighbours):
    s, ref = K.scene(), K.scene_reference()["map"]
    pts, off, _ = KR.off_face()
    m = with_options(scene_map, **options(kernel, scale, neighbours))
    m.reg.max_iteration = 0
    out = host(m.register((dev(pts), dev(off)), s["init"], system0=True))
    assert out["system0"].shape == (8, 32) and out["n_pairs"].dtype == np.int64
    for i in range(8):
        want = RR.linearize(ref, pts[off[i]:off[i + 1]], s["init"][i], kernel, scale, neighbours)
        got = out["system0"][i]
        assert got[27] == want[27] == out["n_correspondences"][i] and want[27] > 1000
        assert got[31] == want[31] == out["n_pairs"][i] and (want[31] > want[27]) == (neighbours == 7)
        assert close(got[:21], want[:21]) and close(got[21:27], want[21:27])
        for t in (28, 29, 30):
            assert abs(got[t] - want[t]) <= 1e-6 * want[t], t
        assert 0.0 < want[30] < want[31]                                   # the kernel is at work
        assert out["weight_sum"][i] == got[30] and abs(out["cost"][i] - want[29]) <= 1e-6 * want[29]
        assert close(out["information"][i], R.full(want))
        assert out["fitness"][i] == want[27] / (off[i + 1] - off[i]) <= 1.0
        assert abs(out["rmse"][i] - np.sqrt(want[28] / want[30])) <= 1e-6 * out["rmse"][i]
        assert np.array_equal(out["transform"][i], s["init"][i])


def test_seven_voxels_without_a_kernel(scene_map):
    s, ref = K.scene(), K.scene_reference()["map"]
    pts, off, _ = KR.off_face()
    m = with_options(scene_map, neighbours=7)
    m.reg.max_iteration = 0
    out = host(m.register((dev(pts), dev(off)), s["init"], system0=True))
    for i in range(8):
        want = RR.linearize(ref, pts[off[i]:off[i + 1]], s["init"][i], None, None, 7)
        got = out["system0"][i]
        assert got[27] == want[27] and got[31] == want[31] == got[30] and want[31] > want[27]
        assert close(got[:21], want[:21]) and close(got[21:27], want[21:27])
        assert abs(got[28] - want[28]) <= 1e-6 * want[28] and abs(got[29] - want[29]) <= 1e-6 * want[29]


# ---- 3. which pairs exist ---------------------------------------------------------------------------------------------

def counts(m, scan, init=None, **kw):
    o = with_options(m, **kw)
    o.reg.max_iteration = 0
    out = host(o.register([scan], np.eye(4)[None] if init is None else init))
    return int(out["n_correspondences"][0]), int(out["n_pairs"][0]) if "n_pairs" in out else None


def test_pairs_on_ten_voxels(ten_map):
    """face neighbours that are usable, unusable, past the capacity and absent; rows in an absent own voxel with a usable
    neighbour; rows that are not finite or outside the grid"""
    m, ref, vox = ten_map
    scan = KR.neighbour_scan(vox)
    I = np.eye(4)
    row1, row7 = RR.pairs(ref, scan, I, 1)[1], RR.pairs(ref, scan, I, 7)[1]
    assert counts(m, scan)[0] == len(row1) == 35
    for kw in (dict(neighbours=7), options("cauchy", 3.0, 7)):
        assert counts(m, scan, **kw) == (len(np.unique(row7)), len(row7))
    assert counts(m, scan, **options("huber", 1.0, 1)) == (35, 35)
    only7 = scan[np.setdiff1d(row7, row1)]                              # absent own voxel, usable neighbour
    assert len(only7) >= 40 and counts(m, only7)[0] == 0
    assert counts(m, only7, neighbours=7)[0] == len(only7)
    never = np.delete(scan, np.unique(row7), 0)
    assert len(never) >= 60 and counts(m, never, neighbours=7) == (0, 0)


@pytest.mark.parametrize("shift", [0, 1 << 20, -(1 << 20)])
def test_pairs_at_the_grids_first_and_last_coordinate(shift):
    """map voxels at coordinate 0 and 2^21 - 1 on x: the neighbour outside the grid is skipped, and the keys of the other
    axes are untouched (a key that borrowed or carried would find KR.EDGE_VOXELS' partner voxel)"""
    pts, off, poses, origin, scan = KR.edge_map(shift)
    ref = R.build_dist(pts, off, poses, origin=origin)
    m = localizer(origin=origin, max_iteration=0)
    assert m.build([pts], poses)["complete"]
    I = np.eye(4)
    row1, row7 = RR.pairs(ref, scan, I, 1)[1], RR.pairs(ref, scan, I, 7)[1]
    assert (len(row1), len(row7), len(np.unique(row7))) == (12, 24, 24)
    assert counts(m, scan)[0] == 12
    assert counts(m, scan, neighbours=7) == (24, 24)
    assert counts(m, scan, **options("geman_mcclure", 2.0, 7)) == (24, 24)


# ---- 4. edges and sizes -----------------------------------------------------------------------------------------------

def test_edges_in_one_batch(scene_map):
    """scans of 0 and 1 rows mid-batch, a scan far from the map, a NaN initial pose: outputs NaN, n_correspondences and
    n_pairs -1, 0 iterations, weight_sum NaN"""
    s = K.scene()
    a, b = s["scans"][:2000], s["scans"][2000:4000]
    far = a + np.array([500.0, 500.0, 50.0], np.float32)                 # inside the grid, nowhere near the map
    nan_pose = s["init"][1].copy()
    nan_pose[1, 2] = np.nan
    scans = [a, a[:0], b[:1], far, b, b]
    init = np.stack([s["init"][0], s["init"][0], s["init"][1], s["init"][0], nan_pose, s["init"][1]])
    m = with_options(scene_map, **options("cauchy", 3.0, 7))
    out = host(m.register(scans, init, system0=True))
    alone = host(m.register([a, b], s["init"][:2]))
    for i, j in ((0, 0), (5, 1)):
        for k in alone:
            assert out[k][i].tobytes() == alone[k][j].tobytes(), (i, k)
    for i in (1, 3):
        assert out["n_correspondences"][i] == 0 and out["n_pairs"][i] == 0 and out["weight_sum"][i] == 0
        assert out["fitness"][i] == 0 and out["rmse"][i] == 0 and out["cost"][i] == 0
        assert np.array_equal(out["transform"][i], init[i]) and not out["information"][i].any()
    one = RR.linearize(K.scene_reference()["map"], b[:1], init[2], "cauchy", 3.0, 7)     # 0.14 voxels from a face
    assert out["n_correspondences"][2] == one[27] == 1 and out["n_pairs"][2] == one[31] == 5
    assert np.array_equal(out["transform"][2], init[2]) and out["iterations"][2] == 1    # rank 3: no step
    assert out["n_correspondences"][4] == -1 and out["n_pairs"][4] == -1 and out["iterations"][4] == 0
    for k in ("transform", "fitness", "rmse", "cost", "information", "system0", "weight_sum"):
        assert np.isnan(out[k][4]).all(), k
    assert out["n_pairs"][0] > out["n_correspondences"][0] > 1000 and out["fitness"][0] <= 1.0


@pytest.mark.parametrize("n", [16383, 16384, 16385])
def test_rows_at_the_sweep_boundary_over_seven_voxels(scene_map, n):
    """64 workgroups x 256 lanes take 16 384 rows per sweep"""
    s, ref = K.scene(), K.scene_reference()["map"]
    rows = np.concatenate([s["scans"][:2000]] * 9)[:n].astype(np.float64)
    rows += np.random.default_rng(n).normal(0, 0.01, rows.shape)
    T0 = s["init"][0]
    pts, off, _ = K.off_face_scans(ref, rows, np.array([0, n]), T0[None])
    pad = rows[:n - len(pts)]                                             # back to n rows, with rows that contribute nowhere
    pts = np.concatenate([pts, np.full_like(pad, np.nan)])
    assert len(pts) == n
    m = with_options(scene_map, **options("cauchy", 2.0, 7))
    m.reg.max_iteration = 1
    out = host(m.register([pts], T0[None], system0=True))
    want = RR.linearize(ref, pts, T0, "cauchy", 2.0, 7)
    got = out["system0"][0]
    assert got[27] == want[27] and got[31] == want[31] and want[31] > want[27] > 10000
    assert close(got[:21], want[:21]) and close(got[21:27], want[21:27]) and abs(got[30] - want[30]) <= 1e-6 * want[30]
    assert out["iterations"][0] == 1


def test_formats_agree(scene_map):
    s = K.scene()
    a = s["scans"][:2000]                                                 # float32 values
    off = dev(np.array([0, 2000], np.int64))
    rows4 = np.concatenate([a, np.full((2000, 1), np.nan, np.float32)], 1)
    m = with_options(scene_map, **options("geman_mcclure", 2.0, 7))
    outs = [host(m.register((dev(r), off), s["init"][:1])) for r in (a, rows4, a.astype(np.float64))]
    for other in outs[1:]:
        for k in outs[0]:
            assert other[k].tobytes() == outs[0][k].tobytes(), k
    assert outs[0]["n_correspondences"][0] > 1000


def test_alone_and_in_a_batch_and_twice(scene_map):
    s = K.scene()
    scans = list(np.split(s["scans"], 8))
    m = with_options(scene_map, **options("cauchy", 3.0, 7))
    batch = host(m.register(scans, s["init"]))
    again = host(m.register(scans, s["init"]))
    for k in batch:
        assert batch[k].tobytes() == again[k].tobytes(), k
    for i in (0, 5):
        alone = host(m.register(scans[i:i + 1], s["init"][i:i + 1]))
        for k in batch:
            assert alone[k][0].tobytes() == batch[k][i].tobytes(), (i, k)


# ---- 5. capture -------------------------------------------------------------------------------------------------------

def test_captured_replay_equals_eager(scene_map):
    from _hipgraph import capture_replay
    s = K.scene()
    m = with_options(scene_map, **options("cauchy", 3.0, 7))
    m.reg.max_iteration = 3
    pts, off, init = dev(s["scans"]), dev(s["scan_offsets"]), dev(s["init"])
    eager, cap, types = capture_replay(lambda: robust_entry(m, pts, off, init, 2, 7, 3.0))
    assert types == {"kernel": 1 + 2 * (3 + 1)}, types                   # the library's launches and nothing else
    for k in eager:
        assert torch.equal(eager[k], cap[k]), k
    assert bool((eager["iterations"] == 3).all()) and bool((eager["n_correspondences"] > 1000).all())
    # MapLocalizer adds one launch: n_pairs as int64
    eager, cap, types = capture_replay(lambda: m.register_device(pts, off, init))
    assert types == {"kernel": 1 + 2 * (3 + 1) + 1}, types
    for k in eager:
        assert torch.equal(eager[k], cap[k]), k
    assert bool((eager["n_pairs"] > eager["n_correspondences"]).all())


# ---- 6. end to end ----------------------------------------------------------------------------------------------------

def agreement(out, ref, what):
    """the device's result against the restatement's, over the scans the restatement finishes: the bar is 10 x what
    +-2^-24 m on every scan coordinate changes in the restatement's own result"""
    fin = ref["finished"]
    assert fin.sum() >= 7
    to_ref = KR.errors(out["transform"], ref["ref"]["transform"])[fin].max(0)
    print(f"{what}: to the restatement {to_ref[0]:.3g} m, {to_ref[1]:.3g} rad (bars {10 * ref['change'][0]:.3g}, "
          f"{10 * ref['change'][1]:.3g}) over {int(fin.sum())} scans; rounds {out['iterations'].tolist()}")
    assert (to_ref <= 10.0 * ref["change"]).all(), what


def test_clutter_end_to_end(scene_map):
    """(a): the quadratic and the Geman-McClure result each agree with the restatement's; the robust one is within twice
    the restatement's own worst error of the truth"""
    s = K.scene()
    scans = list(np.split(KR.clutter_scans(), 8))
    quad, rob = KR.clutter_reference(False), KR.clutter_reference(True)
    out_q = host(scene_map.register(scans, s["init"]))
    agreement(out_q, quad, "clutter, quadratic")
    m = with_options(scene_map, **options(*KR.CLUTTER_ROBUST))
    out_r = host(m.register(scans, s["init"]))
    agreement(out_r, rob, "clutter, geman_mcclure c=2")
    to_truth = KR.errors(out_r["transform"], s["truth"]).max(0)
    bent = KR.errors(out_q["transform"], s["truth"])[:, 0].max()
    print(f"to truth: quadratic {bent * 1e3:.2f} mm, robust {to_truth[0] * 1e3:.2f} mm, {to_truth[1] * 1e3:.3f} mrad "
          f"(bars {2e3 * rob['to_truth'][:, 0].max():.2f} mm, {2e3 * rob['to_truth'][:, 1].max():.3f} mrad)")
    assert (to_truth <= 2.0 * rob["to_truth"].max(0)).all()
    assert bent >= 5.0 * to_truth[0]


def test_wide_start_end_to_end(wide_map):
    """(b): round-0 counts are exact, and Cauchy c = 3 over seven voxels agrees with the restatement on all eight scans"""
    s, ws = K.scene(), KR.wide_scene()
    ref = KR.wide_reference()
    assert ref["finished"].all()
    scans = list(np.split(s["scans"], 8))
    off = s["scan_offsets"]
    for nb in (1, 7):
        m = with_options(wide_map, neighbours=nb)
        m.reg.max_iteration = 0
        out = host(m.register(scans, ws["init"], system0=True))
        want = np.array([RR.linearize(ws["map"], s["scans"][a:b], T, neighbours=nb)
                         for a, b, T in zip(off[:-1], off[1:], ws["init"])])
        assert out["n_correspondences"].tolist() == want[:, 27].astype(np.int64).tolist()
        if nb == 7:
            assert out["n_pairs"].tolist() == want[:, 31].astype(np.int64).tolist()
            assert (out["fitness"] > 0.5).all()
        else:
            assert (out["fitness"] < 0.2).all()
    m = with_options(wide_map, **options(*KR.WIDE_ROBUST))
    out = host(m.register(scans, ws["init"]))
    agreement(out, ref, "wide start, cauchy c=3 over seven voxels")
    assert (KR.errors(out["transform"], s["truth"])[:, 0] < 0.01).all()
    assert (KR.errors(out["transform"], s["truth"]).max(0) <= 2.0 * ref["to_truth"].max(0)).all()


# ---- 7. MapLocalizer with options -------------------------------------------------------------------------------------

def test_extend_follows_the_options():
    """``extend`` with a kernel and seven voxels inserts under the robust transforms, gated on fitness: the map is then,
    by bits, a build over the old clouds and the registered scans"""
    s = K.scene()
    kw = dict(max_voxels=8192, **options("cauchy", 3.0, 7))
    pts, off, poses = dev(s["points"]), dev(s["offsets"]), dev(s["poses"])
    a, b = localizer(insertable=True, **kw), localizer(**kw)
    a.build_device(pts, off, poses)
    b.build_device(pts, off, poses)
    scans, soff, init = dev(s["scans"]), dev(s["scan_offsets"]), dev(s["init"])
    out = a.extend((scans, soff), init, min_fitness=0.3)
    reg = b.register((scans, soff), init)
    assert set(out) == PLAIN_KEYS | {"weight_sum", "n_pairs"}
    for k in reg:
        assert torch.equal(out[k], reg[k]), k
    assert bool((out["fitness"] >= 0.3).all()) and bool((out["fitness"] <= 1.0).all())
    plain = with_options(b).register((scans, soff), init)
    assert set(plain) == PLAIN_KEYS and not torch.equal(plain["transform"], reg["transform"])
    want = host(localizer(max_voxels=8192).build_device(torch.cat([pts, scans]), torch.cat([off, soff[1:] + off[-1]]),
                                                        torch.cat([poses, reg["transform"]]), moments=True))
    n = int(want["stats"][1])
    assert a.stats.cpu().numpy().tobytes() == want["stats"].tobytes() and a.cursor.tolist() == [24000 + 16000, 6 + 8]
    for k in ("voxels", "info", "keys", "moments"):
        assert getattr(a, k)[:n].cpu().numpy().tobytes() == want[k][:n].tobytes(), k
