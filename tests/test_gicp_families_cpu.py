"""The GICP input families (tests/gicp_clouds.py) without a GPU: every family, with every seed the GPU tests use
(tests/test_gicp_paths_gpu.py), reaches the kernel branch it is named after according to the float64 restatement
alone (``gicp_restatement.path_census``), leaves at most 5 % of its rows to the eigenvalue-separation mask, has no
near-tie at the k-th neighbour (or, for ``lattice``, ties that matter), and no correspondence at the radius; the
brute-force searches agree with the cKDTree ones; the down-sampling agrees with a second, dict-keyed restatement."""
import functools

import numpy as np
import pytest

import gicp_clouds as F
import gicp_restatement as G

MASK_CAP = 0.05            # a test may leave at most this share of a cloud's rows to the separation mask
# The kernel's down-sampled coordinates differ from the reference's by at most 2^-25 m (its fixed-point unit is
# 2^-24 m, exact for |p| >= 0.5 m), which moves a distance by less than 1.1e-7 m.  A k-th / (k+1)-th neighbour pair
# farther apart than MIN_GAP cannot change places, so such inputs need no tie mask.
MIN_GAP = 1e-6
RADIUS_MARGIN = 1e-9       # the existing rule: exact system comparison when no correspondence is this near the radius
MANY_SMALL_SEED, TINY_SEED, LATTICE_SEEDS, FACES_SEED = 2, 0, (0, 1), 0


@functools.lru_cache(maxsize=None)
def reference(name):
    A, B, T_fix, params, stride = F.stage_case(name)
    ra, rb = F.cloud_reference(A, params), F.cloud_reference(B, params)
    return ra, rb, G.path_census(ra["ds"], rb["ds"], params, ra["d2"], rb["d2"]), T_fix, params


def assert_claim(name, census):
    claim = F.CLAIMS.get(name)
    rows = [census["source"], census["target"]]
    if claim == "falls_back":
        assert all(not c["small"] and c["falls_back"].all() for c in rows), name
    elif claim == "both":
        assert all(c["falls_back"].sum() >= 5 and c["stops"].sum() >= 5 for c in rows), name
    elif claim == "linearize_brute":
        assert census["linearize_brute"] and census["span"] ** 3 > census["mt"] > 20, name
    else:                                                        # dense: the rings stop, linearize walks cells
        assert all(c["stops"].mean() > 0.99 for c in rows) and not census["linearize_brute"], name


@pytest.mark.parametrize("name", list(F.STAGE_CASES))
def test_stage_case_reaches_its_branch(name):
    ra, rb, census, T_fix, params = reference(name)
    assert_claim(name, census)
    for r in (ra, rb):
        assert r["gap"] > MIN_GAP, (name, r["gap"])
        assert 1.0 - r["sep"].mean() <= MASK_CAP, (name, r["sep"].mean())
        assert 100 <= len(r["ds"]) <= 5000
    radius = params["max_correspondence_distance"]
    assert F.radius_margin(ra["ds"], rb["ds"], T_fix, radius) > RADIUS_MARGIN
    lin = G.linearize(ra["ds"], rb["ds"], ra["cov"], rb["cov"], T_fix, radius)
    assert lin["n_corr"] >= 0.25 * len(ra["ds"]) or name == "small-target" and lin["n_corr"] > 100


def test_grid_covers_the_parameters():
    P = [p for _, p, _ in F.STAGE_CASES.values()]
    assert {p["voxel_size"] for p in P} >= {0.2, 0.5, 1.0, 2.0}
    assert {p["covariance_knn"] for p in P} >= {1, 2, 3, 5, 20, 32}
    assert {p["epsilon"] for p in P} >= {1e-3, 1e-2}
    spans = {int(np.floor(2 * p["max_correspondence_distance"] / p["voxel_size"])) + 2 for p in P}
    assert {3, 6} <= spans and max(spans) >= 12
    walked = [reference(n)[2]["span"] for n in F.STAGE_CASES if not reference(n)[2]["linearize_brute"]]
    assert {3, 6} <= set(walked) and max(walked) >= 12          # ... and the cell walk itself runs at each span
    assert {s for _, _, s in F.STAGE_CASES.values()} == {3, 4}


def test_mixed_reaches_the_key_range():
    A, B, _, params, _ = F.stage_case("mixed-v0.2-k12")
    for c in (A, B):
        p = G.finite_xyz(c)
        keys = np.floor((p - (p.min(0) - params["voxel_size"] / 2)) / params["voxel_size"]).max()
        assert 0.9 * 2 ** 21 < keys < 2 ** 21 - 1


def test_knn_exact_against_ckdtree():
    for cloud, voxel, k in ((F.surface(11, 1500), 0.5, 20), (F.sparse(3), 0.5, 7), (F.lattice(0, 12), 0.5, 9),
                            (F.surface(12, 40), 2.0, 20)):
        ds = G.voxel_down_sample(cloud, voxel)
        ie, d2 = G.knn_exact(ds, k)
        it, d = G.knn(ds, k)
        assert ie.shape == it.shape and d2.shape == d.shape
        assert np.allclose(np.sqrt(d2), d, rtol=1e-12, atol=1e-12)
        kk = ie.shape[1]
        clear = np.ones(len(ds), bool) if d.shape[1] == kk else d[:, kk] > d[:, kk - 1] * (1 + 1e-12)
        assert clear.any()
        assert np.array_equal(np.sort(ie[clear], 1), np.sort(it[clear], 1))
        order = np.lexsort((ie, d2[:, :kk]), axis=1)             # (distance, index) order within each row
        assert np.array_equal(order, np.tile(np.arange(kk), (len(ds), 1)))


@pytest.mark.parametrize("seed", LATTICE_SEEDS)
@pytest.mark.parametrize("k", [8, 20])
def test_lattice_ties_matter(seed, k):
    L = F.lattice(seed)
    ds = G.voxel_down_sample(L, 0.5)
    assert np.array_equal(ds, L[:, :3].astype(np.float64))      # one row per voxel, first-row order, exact
    idx, d2 = G.knn_exact(ds, k)
    sep = G.separated(ds, idx)
    assert 1.0 - sep.mean() <= MASK_CAP
    C, Cr = G.covariances(ds, k, exact=True), G.covariances(ds, k, reverse_ties=True)
    differ = np.abs(C - Cr).max(axis=(1, 2)) > 1e-4 * np.linalg.norm(C, axis=(1, 2))
    assert (d2[:, k] == d2[:, k - 1]).mean() >= 0.4             # equal distances at the k-th place ...
    assert (differ & sep).mean() >= 0.3                          # ... and the other tie rule is caught on these rows
    census = G.ring_census(ds, 0.5, k)
    assert census["stops"].all()                                 # through the ring search, not the full scan


def test_lattice_half_voxel_shift_ties_correspondences():
    """Every source row of the half-voxel-shifted lattice has two target rows at exactly the same distance."""
    ds = G.voxel_down_sample(F.lattice(0), 0.5)
    T = np.eye(4)
    T[0, 3] = 0.25
    q, i, j = G.correspondences(ds, ds, T, 1.0, exact=True)
    d = q[:, None, :] - ds[None, :, :]
    dd = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    assert len(i) == len(ds)
    nearest = dd == dd.min(1, keepdims=True)
    assert (nearest.sum(1) >= 2).mean() >= 0.5
    assert np.array_equal(j, np.argmax(nearest, axis=1))         # the smaller index of the equal ones


def down_sample_by_dict(points, voxel):
    """A second restatement of voxel_down_sample: a dict keyed by the integer voxel triple, first-seen order"""
    rows = [r for r in np.asarray(points, np.float32)[:, :3].astype(np.float64) if np.all(np.isfinite(r))]
    lo = np.min(rows, 0) - voxel / 2
    cells = {}
    for r in rows:
        key = tuple(int(np.floor((r[a] - lo[a]) / voxel)) for a in range(3))
        cells.setdefault(key, []).append(r)
    return np.array([np.sum(v, 0) / len(v) for v in cells.values()]), [len(v) for v in cells.values()]


def test_faces_and_duplicates_down_sample():
    cloud = F.faces_and_duplicates(FACES_SEED)
    p = cloud[:, :3].astype(np.float64)
    assert np.array_equal(p.min(0), [-3.0, -3.0, -3.0])
    on_face = np.all((p + 3.25) / 0.5 == np.round((p + 3.25) / 0.5), 1)       # min bound -3 - voxel / 2
    assert on_face.sum() >= 500
    ds = G.voxel_down_sample(cloud, 0.5)
    ref, counts = down_sample_by_dict(cloud, 0.5)
    assert len(ds) == len(ref) and max(counts) >= 30000
    assert np.abs(ds - ref).max() <= 1e-12                       # same voxels in the same order


def test_many_small_shapes():
    S, T = F.many_small(MANY_SMALL_SEED)
    assert len(S) == len(T) == 300 > 256
    mid = 150
    assert len(S[mid]) == 0 and len(T[mid + 1]) == 0 and np.isnan(S[mid + 2]).all() and np.isnan(T[mid + 3]).all()
    assert len(S[mid + 4]) == 1 and len(T[mid + 5]) == 1 and len(S[mid + 6]) == 2 and len(T[mid + 7]) == 2
    params = dict(G.DEFAULTS)
    wraps, caps, corr = 0, set(), 0
    for a, b in zip(S, T):
        assert len(a) <= 300 and len(b) <= 300
        assert all(np.abs(G.finite_xyz(c)).min(initial=1.0) >= 0.5 for c in (a, b))     # exact in units of 2^-24 m
        ra, rb = F.cloud_reference(a, params), F.cloud_reference(b, params)
        for c, r in ((a, ra), (b, rb)):
            assert r["sep"].all() and r["gap"] > MIN_GAP       # nothing masked, nothing near a tie
            w, cap = G.table_surely_wraps(c, 0.5)
            wraps += w
            caps.add(cap)
        assert F.radius_margin(ra["ds"], rb["ds"], np.eye(4), 1.0) > RADIUS_MARGIN
        corr += G.linearize(ra["ds"], rb["ds"], ra["cov"], rb["cov"], np.eye(4), 1.0)["n_corr"]
    assert caps >= set(range(2, 17, 2))                          # tables of 2 .. 16 slots
    assert wraps >= 20                                           # probes that must wrap past the last slot
    assert corr > 5000
    tiny = F.tiny_clouds(TINY_SEED)
    assert len(tiny) == 1100 > 1024 and {len(c) for c in tiny} == {1, 2, 3, 4, 5}


@pytest.mark.parametrize("name", list(F.END_TO_END))
def test_restatement_recovers_the_motion(name):
    build, params, (t_bar, r_bar) = F.END_TO_END[name]
    A, B, T = build()
    r = G.register(A, B, exact=True, **params)
    te, re = G.pose_error(r["transform"], T)
    assert te <= t_bar and re <= r_bar, (name, te, np.rad2deg(re))
    assert 0 < r["iterations"] < 30 and r["fitness"] > 0.25
