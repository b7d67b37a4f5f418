"""Seen-through voxels without a GPU: the restatement (tests/map_rays_restatement.py) against counts derived by hand, its
walk against the same walk in exact arithmetic, what the rule does on the scene with a box that leaves, the restated carve
against a rebuild, and what can be said about nsc_map_cast_rays and nsc_map_flag_rows without a device: refusals, the shape
of the symbols, the registers of the kernels."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import map_insert_restatement as IR
import map_localize_restatement as R
import map_rays_cases as RC
import map_rays_restatement as RR
import map_replace_restatement as RP

CASES = RC.hand_cases()


@pytest.fixture(scope="module")
def lib():
    from neural_spectral_codec_amd import build, _lib
    build.build_hip()
    return _lib.lib()


# ---- 1. counts derived by hand ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_gives_the_hand_derived_counts(case):
    m = R.build_dist(*RC.hand_map(), voxel_size=1.0)
    assert len(m["keys"]) == len(RC.PLANES) + len(RC.BLOBS) and bool((m["voxels"][:, 15] == 1.0).all())
    r = RR.cast(case["points"], case["offsets"], case["poses"], case["pose_ids"], m, **case["ray"])
    assert RC.crossed_by_voxel(r["crossed"], m["keys"]) == case["crossed"]
    assert r["stats"] == case["stats"] and r["rays_truncated"] == 0
    assert not r["closest_gate"] < 0.4                 # every decision of the hand cases is far from the gate


def test_hand_map_gaussians_are_what_the_cases_assume():
    m = R.build_dist(*RC.hand_map(), voxel_size=1.0)
    for v in RC.PLANES + RC.BLOBS:
        rec = m["voxels"][m["place"][RR.key_of(v)]]
        thin = v in RC.PLANES
        assert np.allclose(rec[:3], np.array(v) + 0.5, atol=1e-12)
        want = np.diag([1.0 / RC.THIN ** 2 if thin else 1.0 / RC.VAR, 1.0 / RC.VAR, 1.0 / RC.VAR])
        assert np.allclose(R.sym3(rec[None, 9:15])[0], want, rtol=1e-3, atol=1e-9), v


def test_accumulation_and_flags_of_the_restatement():
    m = R.build_dist(*RC.hand_map(), voxel_size=1.0)
    c = CASES[1]                                          # "end voxel": planes 2 .. 7 once per call
    crossed = None
    for _ in range(8):
        crossed = RR.cast(c["points"], c["offsets"], c["poses"], None, m, crossed=crossed, **c["ray"])["crossed"]
    assert RC.crossed_by_voxel(crossed, m["keys"]) == {(i, 0, 0): 8 for i in range(2, 8)}
    count = m["info"][:, 0].tolist()                      # a plane holds 16 rows: 8 crossings are half of them
    seen = RR.seen_through(count, crossed)
    assert {tuple(IR.key_voxel(int(k))) for k in m["keys"][seen]} == {(i, 0, 0) for i in range(2, 8)}
    assert not RR.seen_through(count, crossed, ratio=0.51).any() and not RR.seen_through(count, crossed, min_crossings=9).any()
    pts, off, poses = RC.hand_map()
    rows = np.concatenate([pts, [[np.nan, 0, 0], [50.5, 0.5, 0.5], [3.0e6, 0, 0]]])
    flags, stats = RR.flag_rows(rows, np.array([0, len(rows)]), poses, None, m, count, crossed)
    assert stats == [6 * 16, len(pts) - 6 * 16, 2, 1]
    assert np.array_equal(flags[:len(pts)], (pts[:, 2] < 1.0) & (pts[:, 0] < 8.0)) and not flags[len(pts):].any()


# ---- 2. the walk against exact arithmetic -----------------------------------------------------------------------------

def test_walk_visits_the_voxels_of_the_exact_walk():
    """3 000 random rays at voxel 0.3 and max_range 60, a share of them with one or two components of the direction exactly
    zero: the float64 walk and the walk in fractions.Fraction from the same fo, d, t0, t1 visit the same voxels"""
    rng = np.random.default_rng(31)
    n, voxel = 3000, 0.3
    o = rng.uniform(-20, 20, (n, 3))
    D = rng.normal(0, 1, (n, 3))
    D[rng.random((n, 3)) < 0.15] = 0.0
    D[(D == 0).all(1)] = [1.0, 0.0, 0.0]
    D *= (rng.uniform(0.5, 80, n) / np.linalg.norm(D, axis=1))[:, None]
    poses = np.tile(np.eye(4), (n, 1, 1))
    poses[:, :3, 3] = o
    r, walked = RR.walks(D, np.arange(n + 1), poses, None, (voxel, np.zeros(3)), 0.7, 60.0, None)
    assert len(walked) == int((r["kind"] == 0).sum()) > 2900 and bool(((r["d"] == 0).sum(1) > 0).sum() > 500)
    steps, longest, different = RR.max_steps(60.0, voxel), 0, 0
    for i, (visits, ended) in walked.items():
        exact, ended_exactly = RR.walk([Fraction(v) for v in r["fo"][i]], [Fraction(v) for v in r["d"][i]],
                                       Fraction(r["t0"][i]), Fraction(r["t1"][i]), steps)
        assert ended and ended_exactly
        longest = max(longest, len(visits))
        different += [v[0] for v in visits] != [v[0] for v in exact]
    print(f"longest walk {longest} steps of {steps} allowed, {different} rays differ from the exact walk")
    assert different == 0 and 150 < longest < steps


# ---- 3. the scene -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("voxel", [1.0, 0.5])
def test_scene_flags_the_box_and_leaves_the_rest(voxel):
    s, res = RC.scene(), RC.scene_result(voxel)
    assert int(s["is_box"].sum()) > 1000 and not s["is_box"][s["offsets"][3]:].any()
    print(f"voxel {voxel}: box rows flagged {res['box_share']:.4f} (>= 0.6), static rows flagged {res['static_share']:.4f} "
          f"(<= 0.005); closest gate decision {res['cast']['closest_gate']:.3g}, closest stop {res['cast']['closest_stop']:.3g}")
    assert res["box_share"] >= 0.6 and res["static_share"] <= 0.005
    assert res["cast"]["rays_truncated"] == 0 and res["cast"]["rays_cast"] == len(s["points"])
    assert res["flag_stats"][2:] == [0, 0] and res["flag_stats"][0] == int(res["flags"].sum())


@pytest.mark.parametrize("voxel", [1.0, 0.5])
def test_restated_carve_follows_the_rebuild(voxel):
    s, res = RC.scene(), RC.scene_result(voxel)
    n = len(s["points"])
    state = IR.start(res["m"], n, 6)
    carved, removed, fstats = RR.carve(state, s["points"], s["offsets"], s["poses"], None, res["cast"]["crossed"])
    assert np.array_equal(carved, res["flags"]) and fstats == res["flag_stats"]
    k = int(carved.sum())
    assert removed[:5] == [k, n - k, 0, 0, 0] and removed[7] == 0 and removed[6] > 0
    left = R.build_dist(RR.without(s["points"], carved), s["offsets"], s["poses"], voxel_size=voxel)
    assert RP.assert_follows(IR.arrays(state), left, voxel) == removed[6]


# ---- 4. the C ABI without a device ------------------------------------------------------------------------------------

def test_abi_refusals_and_constants(lib):
    import os
    import re
    from neural_spectral_codec_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "nsc.h")).read()
    for name, value in (("NSC_MAP_RAY_LAUNCHES", _lib.MAP_RAY_LAUNCHES), ("NSC_MAP_FLAG_LAUNCHES", _lib.MAP_FLAG_LAUNCHES),
                        ("NSC_MAP_RAY_STATS", _lib.MAP_RAY_STATS), ("NSC_MAP_FLAG_STATS", _lib.MAP_FLAG_STATS),
                        ("NSC_MAP_RAY_MAX_REACH", _lib.MAP_RAY_MAX_REACH)):
        assert int(re.search(rf"#define {name}\s+(\d+)", header).group(1)) == value, name
    assert len(_lib.MAP_RAY_STAT_NAMES) == _lib.MAP_RAY_STATS == 8 and _lib.MAP_RAY_STAT_NAMES == RR.RAY_STAT_NAMES
    assert len(_lib.MAP_FLAG_STAT_NAMES) == _lib.MAP_FLAG_STATS == 4 and _lib.MAP_FLAG_STAT_NAMES == RR.FLAG_STAT_NAMES
    assert _lib.MAP_RAY_LAUNCHES == 2 and _lib.MAP_RAY_MAX_REACH == RR.MAX_REACH == 1 << 16
    assert lib.nsc_abi_version() == 4
    ray = _lib.MapRayParams()
    lib.nsc_map_ray_default_params(C.byref(ray))
    assert (ray.min_range, ray.max_range, ray.end_margin, ray.gate) == (0.0, 60.0, -1.0, 3.0)
    lib.nsc_map_ray_default_params(None)

    some = lambda n=64: (C.c_int64 * n)()                   # noqa: E731  host memory: no call below launches anything
    grid = _lib.MapParams(voxel_size=1.0, origin=(C.c_double * 3)(0, 0, 0))
    base = dict(points=(C.c_float * 64)(), dtype=0, stride=3, offsets=some(), n_clouds=1, total_rows=4, poses=(C.c_double * 16)(),
                n_poses=1, pose_ids=None, params=C.byref(grid), voxels=(C.c_double * 64)(), index=(C.c_uint64 * 64)(), info=some(),
                max_voxels=4, ray=ray, crossed=some(), stats=some(), min_crossings=3, ratio=0.5, flags=(C.c_uint8 * 64)())

    def cast(**kw):
        a = dict(base, **kw)
        r = a["ray"]
        return lib.nsc_map_cast_rays(a["points"], a["dtype"], a["stride"], a["offsets"], a["n_clouds"], a["total_rows"],
                                     a["poses"], a["n_poses"], a["pose_ids"], a["params"], a["voxels"], a["index"],
                                     a["max_voxels"], None if r is None else C.byref(r), a["crossed"], a["stats"], None)

    def flag(**kw):
        a = dict(base, **kw)
        return lib.nsc_map_flag_rows(a["points"], a["dtype"], a["stride"], a["offsets"], a["n_clouds"], a["total_rows"],
                                     a["poses"], a["n_poses"], a["pose_ids"], a["params"], a["index"], a["info"], a["crossed"],
                                     a["max_voxels"], a["min_crossings"], a["ratio"], a["flags"], a["stats"], None)
    for call, needed in ((cast, ("points", "offsets", "poses", "params", "voxels", "index", "ray", "crossed", "stats")),
                         (flag, ("points", "offsets", "poses", "params", "index", "info", "crossed", "stats", "flags"))):
        for name in needed:
            assert call(**{name: None}) == -1, (call.__name__, name)
        for kw in (dict(dtype=2), dict(dtype=-1), dict(stride=2), dict(stride=5), dict(dtype=1, stride=4), dict(n_clouds=-1),
                   dict(total_rows=-1), dict(n_poses=-1), dict(max_voxels=-1)):
            assert call(**kw) == -1, (call.__name__, kw)
        for bad in (0.0, -1.0, math.nan, math.inf):
            g = _lib.MapParams(voxel_size=bad, origin=(C.c_double * 3)(0, 0, 0))
            assert call(params=C.byref(g)) == -1, (call.__name__, bad)
        assert call(max_voxels=_lib.MAP_MAX_VOXELS + 1) == -2 and call(total_rows=_lib.MAP_MAX_ROWS + 1) == -2
    nan, inf = math.nan, math.inf
    for kw in (dict(min_range=-0.5), dict(min_range=nan), dict(min_range=inf), dict(max_range=0.0), dict(max_range=-1.0),
               dict(max_range=nan), dict(max_range=inf), dict(end_margin=nan), dict(end_margin=inf), dict(end_margin=-inf),
               dict(gate=0.0), dict(gate=-3.0), dict(gate=nan), dict(gate=inf)):
        f = dict(min_range=0.0, max_range=60.0, end_margin=-1.0, gate=3.0)
        f.update(kw)
        assert cast(ray=_lib.MapRayParams(**f)) == -1, kw
    # max_range / voxel_size: 2^16 voxels are the most
    fine = _lib.MapParams(voxel_size=2.0 ** -11, origin=(C.c_double * 3)(0, 0, 0))
    assert cast(params=C.byref(fine), ray=_lib.MapRayParams(0.0, 32.0 + 2.0 ** -10, -1.0, 3.0)) == -2
    assert cast(ray=_lib.MapRayParams(0.0, 65536.5, -1.0, 3.0)) == -2
    for kw in (dict(min_crossings=0), dict(min_crossings=-2), dict(ratio=0.0), dict(ratio=-0.5), dict(ratio=nan), dict(ratio=inf)):
        assert flag(**kw) == -1, kw


def test_the_symbols_take_no_workspace():
    import workspace_contract as W
    from neural_spectral_codec_amd import _lib
    for name, n_args in (("nsc_map_cast_rays", 17), ("nsc_map_flag_rows", 19)):
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and C.c_size_t not in args and len(args) == n_args, name
        assert name not in W.wrapped_symbols()
    assert len(W.wrapped_symbols()) == 28
    assert _lib.SYMBOLS["nsc_map_ray_default_params"] == (None, [C.POINTER(_lib.MapRayParams)])
    assert C.sizeof(_lib.MapRayParams) == 32


def test_localizer_refusals_on_the_host():
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import MapLocalizer
    for kw in (dict(ray_min_range=-1.0), dict(ray_max_range=0.0), dict(ray_max_range=float("inf")), dict(ray_end_margin=-0.5),
               dict(ray_end_margin=float("nan")), dict(ray_gate=0.0), dict(ray_gate=float("nan")),
               dict(ray_max_range=60.0, voxel_size=2.0 ** -11), dict(min_crossings=0), dict(crossing_ratio=0.0),
               dict(crossing_ratio=float("nan"))):
        with pytest.raises(_lib.NscError):
            MapLocalizer(**kw)
    m = MapLocalizer(insertable=True, ray_end_margin=None)
    assert (m.ray.min_range, m.ray.max_range, m.ray.end_margin, m.ray.gate) == (0.0, 60.0, -1.0, 3.0)
    assert (m.min_crossings, m.crossing_ratio, m.crossed) == (3, 0.5, None)
    assert MapLocalizer(ray_end_margin=0.0).ray.end_margin == 0.0
    for call in (lambda: m.observe([], np.zeros((0, 4, 4))), m.seen_through, lambda: m.carve([], np.zeros((0, 4, 4)))):
        with pytest.raises(_lib.NscError, match="build a map"):
            call()


def test_ray_kernels_use_no_scratch(lib):
    """the cast keeps a ray's state in registers whatever the step axis (no array is indexed by it) and leaves room for
    four waves per SIMD; read from the gfx950 code object as tests/test_map_rehash_cpu.py does"""
    import kernel_budget as KB
    assert KB.binutils(), f"no llvm binutils in {KB.LLVM}"
    found = KB.kernels(r"ray_(cast|flag)_kernel")
    assert len(found) == 4, sorted(found)                  # float32 and float64 rows
    for k, (vg, sc) in found.items():
        print(f"{k}: {vg} VGPRs, {sc} B scratch")
        assert sc == 0 and vg <= 128, f"{k}: {vg} VGPRs, {sc} B scratch"
