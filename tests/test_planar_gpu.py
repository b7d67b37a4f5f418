"""The planar initial guess on the MI355X: nsc_planar_align (estimate_planar) against the float64 restatement
(tests/planar_restatement.py) fed with the store's own rows, so every comparison is integer (or bitwise) equality:
constructed walls over a plane at every tile and per-lane boundary of the kernel, symmetric lattices for the tie
rules, empty and invalid pairs, determinism, split batches, hipGraph capture together with the registration, and the
loop-closing paths that use the guess."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gicp_restatement as G
import planar_restatement as PL
from test_gicp_cpu import R_BAR, T_BAR
from test_planar_cpu import GUESS_T_BAR, GUESS_YAW_BAR_DEG, other_world, revisit_pair, true_yaw_deg, wrap_deg

pytestmark = pytest.mark.gpu

IDENTITY = np.eye(4).tobytes()
KEYS = ("best", "scores", "counts", "init_transforms")
# the kernel's boundaries (csrc/nsc_planar.hip): 256 target rows per tile, 256 source rows per read, a source list of
# 1024 places (4 per lane) that is voted once fewer than 256 places are left
TILE, LIST = 256, 1024


def _pa():
    from neural_spectral_codec_amd.retrieval import planar_alignment as pa
    return pa


def _gv():
    from neural_spectral_codec_amd.retrieval import geometric_verification as gv
    return gv


def estimate(src, sids, tgt, tids, yaw_cs=None, stages=True, **params):
    out = _pa().estimate_planar(src, sids, tgt, tids, yaw_cs=yaw_cs, stages=stages, **params)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def rows_of(store, i):
    c = store.cloud(i)
    return c["points"].cpu().numpy(), c["covariances"].cpu().numpy()


def assert_matches(got, i, store_s, a, store_t, b, table, what="", **params):
    """pair i of estimate_planar's outputs against the restatement of the two stored clouds: exact"""
    near = {}
    sp, sc = rows_of(store_s, a)
    tp, tc = rows_of(store_t, b)
    r = PL.align(sp, sc, tp, tc, table, near=near, **params)
    print(what, "rows", len(sp), len(tp), "counts", r["counts"], "best", r["best"], "scores", r["scores"], "near", near)
    assert near == dict(edge=0, z=0), (what, near)           # nothing within 1e-9 of a decision, exact edges apart
    assert np.array_equal(got["votes"][i], r["votes"]), what
    assert np.array_equal(got["yaw_peaks"][i], r["yaw_peaks"]), what
    assert got["best"][i].tolist() == r["best"].tolist(), (what, got["best"][i], r["best"])
    assert got["scores"][i].tolist() == r["scores"].tolist(), (what, got["scores"][i], r["scores"])
    assert got["counts"][i].tolist() == r["counts"].tolist(), (what, got["counts"][i], r["counts"])
    assert got["init_transforms"][i].tobytes() == r["init"].tobytes(), what
    for k in ("best", "scores", "counts", "yaw_peaks", "votes"):
        assert got[k].dtype == np.int32, k
    return r


def assert_same(a, i, b, j, what="", keys=KEYS):
    for k in keys:
        x, y = np.ascontiguousarray(a[k][i]), np.ascontiguousarray(b[k][j])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, i, j, k, x, y)


# ------------------------------------------------------------------------------------------------
# constructed clouds: vertical wall patches over a horizontal plane, one row per voxel
# ------------------------------------------------------------------------------------------------
def walls(n_wall, n_ground, seed=0):
    """(n_wall + n_ground, 3) float32: columns of six points 0.5 m apart in z on a zigzag of wall segments (ten
    columns each, the last one up to nineteen; alternately on a plane of constant x and of constant y), then a ground
    patch 3 m below.  Every point
    sits on a 0.5 m lattice plus a jitter in [0, 0.2), so each is a voxel of its own at voxel_size 0.5 and the
    store's rows are these points in this order; the same seed gives the same leading points for any size."""
    rng = np.random.default_rng(seed)
    jit = rng.uniform(0.0, 0.2, (4096, 3))
    pts = []
    last = max(-(-n_wall // 6) // 10, 1) - 1                 # the last segment also takes the columns left over, so
    for i in range(n_wall):                                  # no column stands alone and every wall row is structure
        col, k = divmod(i, 6)
        seg, c = divmod(col, 10)
        if seg > last:
            seg, c = last, col - 10 * last
        x0 = 6.0 * (seg // 2) - 8.0
        xy = (x0, -5.0 + 0.5 * c) if seg % 2 == 0 else (x0 + 1.0 + 0.5 * c, 1.0)
        pts.append((xy[0], xy[1], 0.5 * k))
    for i in range(n_ground):
        r, c = divmod(i, 12)
        pts.append((-8.0 + 0.5 * c, -5.0 + 0.5 * r, -3.0))
    pts = np.array(pts, np.float64).reshape(-1, 3) + jit[:len(pts)] * [0.1, 0.1, 1.0]
    return pts.astype(np.float32)


def moved(points, yaw_deg, t):
    """Rz(yaw) p + t: a planted relative pose (quarter turns keep one row per voxel)"""
    c, s = {0: (1.0, 0.0), 90: (0.0, 1.0), 180: (-1.0, 0.0), -90: (0.0, -1.0)}.get(
        yaw_deg, (np.cos(np.radians(yaw_deg)), np.sin(np.radians(yaw_deg))))
    p = points.astype(np.float64)
    out = np.stack([c * p[:, 0] - s * p[:, 1] + t[0], s * p[:, 0] + c * p[:, 1] + t[1], p[:, 2]], 1)
    return out.astype(np.float32)


GROUND_ROWS = 60
# (half_bins, table degrees (None = the default 180), source_stride, cell, source wall rows, target wall rows, planted
# yaw, planted translation, seed, source ground rows).  Target rows (walls + 60 ground rows) sit on both sides of the
# 256-row tile.  The source is read 256 raw rows at a time and the rows taken fill a list of 1024 places, four per
# lane: sources of walls alone at stride 1, where every raw row is taken, have 255 / 256 / 257 / 512 rows (the last read
# is short, full, one row long; ms % 256 == 0; a lane holds one row or two), 1024 and 1025 (the list exactly full after
# the last read; voted full and then once more for one row) and 1320 (voted because it passed 768 with rows to follow,
# then a short pass); 196 walls + 60 ground rows are 256 raw rows of which fewer are taken; 1200 walls + ground at
# stride 1 take more than one pass.  The seeds are ones for which no pre-floor value lies within 1e-9 of a bin edge
# and no |dz| within 1e-9 of z_window (checked on the CPU with every row taken; assert_matches checks the rows the
# store holds).
CASES = [
    (1, [90.0], 1, 0.5, 240, TILE - 1 - GROUND_ROWS, 90, (0.5, -0.5), 1, GROUND_ROWS),
    (8, [0.0, 90.0, 180.0, -90.0], 2, 1.0, 300, TILE - GROUND_ROWS, 90, (3.0, -2.0), 1, GROUND_ROWS),
    (24, None, 2, 0.5, 360, TILE + 1 - GROUND_ROWS, -90, (3.0, -2.5), 2, GROUND_ROWS),
    (32, [180.0, 90.0, 0.0, 178.0], 1, 0.5, 1200, 300, 180, (-7.0, 9.0), 1, GROUND_ROWS),
    (24, None, 3, 0.5, 330, 380, 34, (3.0, -2.5), 1, GROUND_ROWS),
    (8, [-90.0, 0.0, 90.0, 180.0], 1, 0.5, 810, 2 * TILE - GROUND_ROWS, 0, (1.5, 2.0), 1, GROUND_ROWS),
    (8, [-90.0], 3, 1.0, 150, 3 * TILE + 1 - GROUND_ROWS, -90, (-2.0, 1.0), 1, GROUND_ROWS),
    (8, [0.0, 90.0, 180.0, -90.0], 1, 0.5, 255, 200, 90, (1.5, -1.0), 1, 0),
    (8, [0.0, 90.0, 180.0, -90.0], 1, 0.5, 256, 200, -90, (1.5, -1.0), 1, 0),
    (8, [0.0, 90.0, 180.0, -90.0], 1, 0.5, 257, 200, 180, (-2.0, 3.0), 1, 0),
    (8, [0.0, 90.0, 180.0, -90.0], 1, 0.5, 512, 200, 90, (1.5, -1.0), 1, 0),
    (8, [0.0, 90.0, 180.0, -90.0], 1, 0.5, 1024, 200, 90, (-3.0, 2.0), 1, 0),
    (8, [0.0, 90.0, 180.0, -90.0], 1, 0.5, 1025, 200, -90, (1.5, -1.0), 1, 0),
    (8, [0.0, 90.0, 180.0, -90.0], 1, 0.5, 1320, 200, 180, (2.0, 2.5), 1, 0),
    (8, [0.0, 90.0, 180.0, -90.0], 2, 0.5, 196, 200, 90, (1.5, -1.0), 1, GROUND_ROWS),
]


@pytest.fixture(scope="module")
def constructed():
    """one store holding source and target of every case: cloud 2 i and 2 i + 1"""
    store = _gv().PreparedClouds()
    for hb, deg, stride, cell, ns, nt, yaw, t, seed, sg in CASES:
        store.add([walls(ns, sg, seed), moved(walls(nt, GROUND_ROWS, seed), yaw, t)])
    return store


@pytest.mark.parametrize("case", range(len(CASES)))
def test_constructed_clouds_exact(constructed, case):
    hb, deg, stride, cell, ns, nt, yaw, t, seed, sg = CASES[case]
    table = PL.yaw_table()[0] if deg is None else PL.table_of(deg)
    params = dict(half_bins=hb, source_stride=stride, cell=cell)
    got = estimate(constructed, [2 * case], constructed, [2 * case + 1], None if deg is None else table, **params)
    assert got["votes"].shape == (1, len(table), 2 * hb + 1, 2 * hb + 1)
    assert got["yaw_peaks"].shape == (1, len(table), 2)
    r = assert_matches(got, 0, constructed, 2 * case, constructed, 2 * case + 1, table, CASES[case], **params)
    sp, sc = rows_of(constructed, 2 * case)
    tp, tc = rows_of(constructed, 2 * case + 1)
    assert len(sp) == ns + sg                                # one row per input point, in input order
    if yaw in (0, 90, 180, -90):
        assert len(tp) == nt + GROUND_ROWS
    # the plane's rows cast no vote: none of them is a structure row, nearly every wall row is
    assert (sp[ns:, 2] < -2.0).all() and (sp[:ns, 2] >= 0.0).all()
    assert not PL.structure(sc)[sp[:, 2] < -2.0].any() and not PL.structure(tc)[tp[:, 2] < -2.0].any()
    assert PL.structure(sc)[:ns].mean() > 0.9 and r["counts"][1] == PL.structure(tc)[tp[:, 2] >= 0.0].sum()
    if ns == 1200:
        assert r["counts"][0] > LIST                         # more source rows than one pass holds
    if sg == 0 and ns <= LIST + 1:
        assert stride == 1 and r["counts"][0] == ns          # walls alone: every raw row is taken
    if ns == 1320:                                           # all but a few: the list passes 768 at the fourth read
        assert stride == 1 and PL.structure(sc)[:LIST].sum() > LIST - TILE and r["counts"][0] > LIST + TILE
    # the planted pose wins: its hypothesis, and the bin of its translation to a cell
    best_deg = (PL.yaw_table()[1] if deg is None else np.array(deg))[r["best"][0]]
    assert wrap_deg(best_deg - yaw) == 0.0
    assert abs(r["best"][1] * cell - t[0]) <= cell and abs(r["best"][2] * cell - t[1]) <= cell
    assert r["scores"][0] > r["scores"][1]
    # without the stage outputs: the same results from the workspace
    plain = estimate(constructed, [2 * case], constructed, [2 * case + 1], None if deg is None else table,
                     stages=False, **params)
    assert set(plain) == set(KEYS)
    assert_same(plain, 0, got, 0, "no stages")


# ------------------------------------------------------------------------------------------------
# ties
# ------------------------------------------------------------------------------------------------
def square():
    """four walls of a square, exactly symmetric under quarter turns: 16 x 6 lattice points each, no jitter"""
    side = np.array([(4.25, -3.75 + 0.5 * j, 0.25 + 0.5 * k) for j in range(16) for k in range(6)])
    turns = [side, side[:, [1, 0, 2]] * [-1, 1, 1], side * [-1, -1, 1], side[:, [1, 0, 2]] * [1, -1, 1]]
    return np.concatenate(turns).astype(np.float32)


def test_symmetric_lattice_ties():
    store = _gv().PreparedClouds()
    wall = np.array([(0.25, 0.25 + 0.5 * j, 0.25 + 0.5 * k) for j in range(12) for k in range(6)], np.float32)
    twice = np.concatenate([wall + np.float32([-1.5, 0, 0]), wall + np.float32([1.0, 0, 0])])
    store.add([square(), wall, twice])
    # hypotheses a quarter turn apart, given exactly: the square maps onto itself, the four peaks tie, the smaller
    # index wins whatever its angle
    for order in ([0, 1, 2, 3], [1, 3, 0, 2], [3, 2, 1, 0]):
        table = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])[order]
        got = estimate(store, [0], store, [0], table, half_bins=8, source_stride=1)
        r = assert_matches(got, 0, store, 0, store, 0, table, order, half_bins=8, source_stride=1)
        assert len(set(r["yaw_peaks"][:, 0].tolist())) == 1 and r["yaw_peaks"][0, 0] > 0       # a four-way tie
        assert r["best"].tolist() == [0, 0, 0] and r["scores"][1] == 0      # all four inside the default guard
        guarded = estimate(store, [0], store, [0], table, half_bins=8, source_stride=1, guard=0)
        assert guarded["scores"][0].tolist() == [r["yaw_peaks"][0, 0]] * 2    # guard 0: the tied neighbours count
    # two bins of one hypothesis: the wall against two copies of itself, 1.5 m to one side and 1.0 m to the other
    table = np.array([[1.0, 0.0]])
    got = estimate(store, [1], store, [2], table, half_bins=8, source_stride=1)
    r = assert_matches(got, 0, store, 1, store, 2, table, "two bins", half_bins=8, source_stride=1)
    assert r["votes"][0, -3 + 8, 8] == r["votes"][0, 2 + 8, 8] == r["scores"][0] > 0
    assert got["best"][0].tolist() == [0, -3, 0] and got["init_transforms"][0, 0, 3] == -1.5


# ------------------------------------------------------------------------------------------------
# degenerate pairs, determinism, batches
# ------------------------------------------------------------------------------------------------
def test_empty_flat_and_invalid_pairs():
    store = _gv().PreparedClouds()
    ground = walls(0, 150, seed=2)
    store.add([walls(200, GROUND_ROWS, seed=3), np.zeros((0, 3), np.float32), ground,
               moved(walls(220, GROUND_ROWS, seed=3), 90, (1.0, 1.0))])
    table = PL.table_of([0.0, 90.0, 180.0, -90.0])
    sids = torch.tensor([0, 1, 0, 2, 0, -1, 0, 1 << 40, 0, 1, 0], dtype=torch.int64, device="cuda")
    tids = torch.tensor([3, 3, 1, 3, 2, 3, 4, 0, -7, 1, 3], dtype=torch.int64, device="cuda")
    got = estimate(store, sids, store, tids, table, half_bins=8)
    ref = assert_matches(got, 0, store, 0, store, 3, table, "valid", half_bins=8)
    assert ref["scores"][0] > 0 and ref["best"][0] == 1
    assert_same(got, 10, got, 0, "valid pair after invalid ones", KEYS + ("yaw_peaks", "votes"))
    for i, (a, b) in ((1, (1, 3)), (2, (0, 1)), (3, (2, 3)), (4, (0, 2)), (9, (1, 1))):       # empty, no structure
        r = assert_matches(got, i, store, a, store, b, table, (a, b), half_bins=8)
        assert r["scores"].tolist() == [0, 0]
        assert got["best"][i].tolist() == [-1, 0, 0] and got["init_transforms"][i].tobytes() == IDENTITY
    assert got["counts"][3].tolist() == [0, ref["counts"][1]] and got["counts"][1, 0] == 0
    for i in (5, 6, 7, 8):                                   # an id outside its store
        assert got["best"][i].tolist() == [-1, 0, 0] and got["scores"][i].tolist() == [-1, -1], i
        assert got["counts"][i].tolist() == [0, 0] and got["init_transforms"][i].tobytes() == IDENTITY, i
        assert not got["votes"][i].any() and not got["yaw_peaks"][i].any()
    empty = _gv().PreparedClouds()                           # an empty store: every id is invalid
    got = estimate(empty, [0], store, [0], table, half_bins=8)
    assert got["best"][0].tolist() == [-1, 0, 0] and got["scores"][0].tolist() == [-1, -1]
    none = estimate(store, [], store, [], table, half_bins=8)
    assert none["best"].shape == (0, 3) and none["init_transforms"].shape == (0, 4, 4) and \
        none["votes"].shape == (0, 4, 17, 17)


def test_deterministic_batch_independent_and_split(constructed, monkeypatch):
    pa = _pa()
    n = len(constructed)
    pl = [(a, b) for a in (0, 2, 7, 8) for b in (1, 3, 6, 9)] + [(n, 0), (0, -1)]
    keys = KEYS + ("yaw_peaks", "votes")
    table = PL.table_of(np.arange(-180.0, 180.0, 30.0))
    kw = dict(half_bins=12, source_stride=2)
    one = estimate(constructed, [a for a, _ in pl], constructed, [b for _, b in pl], table, **kw)
    two = estimate(constructed, [a for a, _ in pl], constructed, [b for _, b in pl], table, **kw)
    for i in range(len(pl)):
        assert_same(one, i, two, i, "second run", keys)
    perm = np.random.default_rng(1).permutation(len(pl))
    shuffled = estimate(constructed, [pl[k][0] for k in perm], constructed, [pl[k][1] for k in perm], table, **kw)
    for i, k in enumerate(perm):
        assert_same(shuffled, i, one, k, "order", keys)
    alone = _gv().PreparedClouds()                           # alone, in stores of its own
    other = _gv().PreparedClouds()
    hb, deg, stride, cell, ns, nt, yaw, t, seed, sg = CASES[1]
    alone.add([walls(ns, sg, seed)])
    other.add([np.zeros((5, 3), np.float32), moved(walls(nt, GROUND_ROWS, seed), yaw, t)])
    single = estimate(alone, [0], other, [1], table, **kw)
    assert_same(single, 0, one, pl.index((2, 3)), "single", keys)
    assert one["scores"][pl.index((2, 3)), 0] > 0
    monkeypatch.setattr(pa, "MAX_PAIRS_PER_CALL", 5)
    split = estimate(constructed, [a for a, _ in pl], constructed, [b for _, b in pl], table, **kw)
    assert split["best"].shape == (len(pl), 3) and split["votes"].shape == one["votes"].shape
    for i in range(len(pl)):
        assert_same(split, i, one, i, "split", keys)


def test_capture_with_registration(constructed):
    from _hipgraph import keep_graphs, node_types
    gv = _gv()
    sids = torch.tensor([0, 2, 4], dtype=torch.int64, device="cuda")
    tids = torch.tensor([1, 3, 5], dtype=torch.int64, device="cuda")
    table = torch.from_numpy(PL.yaw_table()[0]).cuda()

    def step():
        planar = _pa().estimate_planar(constructed, sids, constructed, tids, yaw_cs=table)
        out = gv.register_prepared(constructed, sids, constructed, tids, planar["init_transforms"])
        return {**planar, **out}
    eager = {k: v.clone() for k, v in step().items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                               # warm the allocator outside the capture
    torch.cuda.current_stream().wait_stream(s)
    with keep_graphs() as made:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cap = step()
    g.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(eager[k], cap[k]), k
    types = node_types(made[0])
    assert types.get("memset", 0) == 0 and types.get("memcpy", 0) == 0, types
    assert types.get("kernel", 0) == (1 + 2 * 31) + 3        # the registration's launches and the three of the guess
    assert cap["scores"][:, 0].min().item() > 0
    for i, case in enumerate((0, 1, 2)):                     # and the captured pairs ended on the planted pose
        yaw, t = CASES[case][6], CASES[case][7]
        T = cap["transform"][i].cpu().numpy()
        assert abs(wrap_deg(true_yaw_deg(T) - yaw)) < 1.0 and np.abs(T[:2, 3] - t).max() < 0.1, (case, T)


# ------------------------------------------------------------------------------------------------
# loop closing
# ------------------------------------------------------------------------------------------------
E2E_OFFSETS = [(4.0, -3.0, 17.5), (8.0, 8.0, -93.2), (10.0, -2.0, 30.0)]       # of world 3, as in DESIGN.md 4.10


@pytest.fixture(scope="module")
def scans():
    """(query scan, [three revisits, the other world], {keyframe id: true transform})"""
    pairs = [revisit_pair(3, o) for o in E2E_OFFSETS]
    return pairs[0][0], [p[1] for p in pairs] + [other_world()], {100 + i: p[2] for i, p in enumerate(pairs)}


def _edge_fn(source_pose, target_pose, relative_transform, information_matrix):
    return {"transform": relative_transform, "information": information_matrix}


def _database(clouds, n_queries=1):
    rng = np.random.default_rng(0)
    desc = rng.random((len(clouds) + n_queries, 800)).astype(np.float32)
    desc /= desc.sum(1, keepdims=True)
    kfs = [SimpleNamespace(keyframe_id=100 + i, scan_id=i, points=s, descriptor=desc[i], pose=None)
           for i, s in enumerate(clouds)]
    return kfs, desc[len(clouds):]


def _retrieval(kfs, **kw):
    from neural_spectral_codec_amd.retrieval import GeometricVerifier, create_two_stage_retrieval
    r = create_two_stage_retrieval(top_k=len(kfs), verifier=GeometricVerifier(), edge_fn=_edge_fn, **kw)
    r.add_keyframes(kfs[:2])
    for kf in kfs[2:]:
        r.add_keyframe(kf)
    return r


def _same_closures(a, b):
    assert [e["target_id"] for e in a] == [e["target_id"] for e in b]
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k


def test_translated_revisits_close_the_loop(scans):
    from neural_spectral_codec_amd.retrieval import GeometricVerifier, batch_loop_closing
    A, clouds, truth = scans
    kfs, qdesc = _database(clouds)
    query = SimpleNamespace(keyframe_id=7, scan_id=7, points=A, descriptor=qdesc[0], pose=None)
    with_planar = _retrieval(kfs, prepare_geometry=True, planar_init=True)
    edges = with_planar.get_loop_closures(query)
    assert {e["target_id"] for e in edges} >= set(truth)
    for e in edges:
        if e["target_id"] in truth:
            te, re_ = G.pose_error(e["transform"], truth[e["target_id"]])
            print("planar_init", e["target_id"], "translation error", te, "rotation error deg", np.rad2deg(re_),
                  e["fitness"])
            assert te <= T_BAR and re_ <= R_BAR, (e["target_id"], te, np.rad2deg(re_))

    # info: the new fields; the guess is within the bar of the truth; the support tells the other world apart
    everyone = with_planar._global_retrieval(query)
    with_planar._geometric_verification(query.points, everyone)
    assert len(everyone) == 4
    support = {}
    for c in everyone:
        assert {"init_yaw_deg", "init_translation", "planar_peak", "planar_peak_ratio", "planar_support", "fitness",
                "rmse"} <= set(c.info)
        support[c.database_idx] = c.info["planar_support"]
        print(c.database_idx, {k: c.info[k] for k in ("init_yaw_deg", "planar_peak", "planar_peak_ratio",
                                                      "planar_support", "fitness")}, c.info["init_translation"])
        if c.database_idx < 3:
            T_true = truth[100 + c.database_idx]
            assert c.verified and c.info["planar_peak_ratio"] > 1.0
            assert abs(wrap_deg(c.info["init_yaw_deg"] - true_yaw_deg(T_true))) <= GUESS_YAW_BAR_DEG
            assert np.linalg.norm(c.info["init_translation"][:2] - T_true[:2, 3]) <= GUESS_T_BAR
    assert min(support[i] for i in range(3)) > 2.0 * support[3]

    # the estimate the retrieval made is estimate_planar's on its stores, which is the restatement's
    got = estimate(with_planar._query_geometry, [0] * 4, with_planar.geometry, [0, 1, 2, 3], stages=False)
    for c in everyone:
        i = c.database_idx
        assert c.info["planar_peak"] == got["scores"][i, 0] and \
            c.info["planar_support"] == got["scores"][i, 0] / got["counts"][i, 0]
        assert np.array_equal(c.info["init_translation"], got["init_transforms"][i, :3, 3])

    # a support threshold the caller chose: the other world is not verified whatever GICP says, the revisits stay
    cut = 0.5 * (min(support[i] for i in range(3)) + support[3])
    strict = _retrieval(kfs, prepare_geometry=True, planar_init=True, planar_min_support=cut)
    _same_closures([e for e in edges if e["target_id"] in truth], strict.get_loop_closures(query))
    nothing = _retrieval(kfs, prepare_geometry=True, planar_init=True, planar_min_support=1e9)
    assert nothing.get_loop_closures(query) == []
    looked_at = nothing._global_retrieval(query)
    assert nothing._geometric_verification(query.points, looked_at) == [] and len(looked_at) == 4
    assert all(not c.verified and c.fitness > 0.3 and c.info["planar_support"] > 0 for c in looked_at)

    # the batched path: bitwise the per-query one
    batched = batch_loop_closing([query], kfs, top_k=4, verifier=GeometricVerifier(), edge_fn=_edge_fn,
                                 prepare_geometry=True, planar_init=True)
    _same_closures(edges, batched[0])
    with_planar.clear_database()
    assert len(with_planar.geometry) == 0 and with_planar.query(query) == []


def test_off_is_todays_path(scans, monkeypatch):
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import GeometricVerifier, TwoStageRetrieval, batch_loop_closing
    A, clouds, truth = scans
    kfs, qdesc = _database(clouds[:2] + clouds[3:])
    query = SimpleNamespace(keyframe_id=7, points=A, descriptor=qdesc[0], pose=None)
    called = []
    monkeypatch.setattr(_pa(), "estimate_planar", lambda *a, **kw: called.append(1))
    wrong = 0
    for prep in (False, True):
        plain = _retrieval(kfs, prepare_geometry=prep)
        off = _retrieval(kfs, prepare_geometry=prep, planar_init=False, planar_min_support=None)
        a, b = plain.query(query), off.query(query)
        assert [c.database_idx for c in a] == [c.database_idx for c in b] and len(a) >= 1      # the verified ones
        for x, y in zip(a, b):
            assert x.verified == y.verified and x.distance == y.distance
            assert x.fitness == y.fitness and x.rmse == y.rmse
            assert x.transform.tobytes() == y.transform.tobytes()
            assert x.information_matrix.tobytes() == y.information_matrix.tobytes()
            assert "planar_support" not in x.info and "planar_support" not in y.info
            if x.verified and x.database_idx < 2:             # today's path: verified, and metres wrong
                wrong += G.pose_error(x.transform, truth[100 + x.database_idx])[0] > 3.0
    assert wrong >= 1
    _same_closures(batch_loop_closing([query], kfs, top_k=3, verifier=GeometricVerifier(), edge_fn=_edge_fn,
                                      prepare_geometry=True)[0],
                   batch_loop_closing([query], kfs, top_k=3, verifier=GeometricVerifier(), edge_fn=_edge_fn,
                                      prepare_geometry=True, planar_init=False)[0])
    assert not called
    with pytest.raises(_lib.NscError):
        TwoStageRetrieval(verifier=GeometricVerifier(), planar_init=True)                 # needs the prepared stores
    with pytest.raises(_lib.NscError):
        batch_loop_closing([query], kfs, verifier=GeometricVerifier(), edge_fn=_edge_fn, planar_init=True)
    with pytest.raises(ValueError):
        TwoStageRetrieval(verifier=GeometricVerifier(), prepare_geometry=True, planar_init=True, yaw_init=True)
