"""The planar initial guess without a GPU: the float64 restatement (tests/planar_restatement.py) against a brute-force
loop on constructed rows with every inclusive edge and tie rule; on ray-cast revisits that are metres away and rotated
it finds yaw and translation inside GICP's basin, the restatement's GICP converges from that guess and, from the
identity, passes the thresholds with a transform that is metres wrong; nsc_planar_align validates its arguments on
the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gicp_restatement as G
import planar_restatement as PL
from neural_spectral_codec_amd import synth
from test_gicp_cpu import R_BAR, T_BAR

# (world, (x, y, yaw deg) of the second visit): translated and rotated revisits, all outside GICP's basin
REVISITS = [(3, (4.0, -3.0, 17.5)), (3, (8.0, 8.0, -93.2)), (5, (0.0, 11.5, -147.0))]
# The bar on the guess: the worst of a nine-revisit sweep of the restatement (worlds 3, 5, 7; translation up to
# 11.5 m, any yaw) was 0.54 m and 1.0 degrees; half again as margin, capped at GICP's
# documented basin of 1.0 m / 5 degrees.
GUESS_T_BAR, GUESS_YAW_BAR_DEG = 0.81, 1.5

STRUCTURE = [1e-3, 0.0, 0.0, 1.0, 0.0, 1.0]       # covariance of a row whose normal is the x axis: I - (1 - eps) n n^T
GROUND = [1.0, 0.0, 0.0, 1.0, 0.0, 1e-3]          # ... the z axis
QUARTER = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])        # 0, 90, 180, 270 degrees, exactly


def wrap_deg(d):
    return -((-d + 180.0) % 360.0 - 180.0)


def cov6(C33):
    return np.stack([C33[:, 0, 0], C33[:, 0, 1], C33[:, 0, 2], C33[:, 1, 1], C33[:, 1, 2], C33[:, 2, 2]], 1)


def reduced_table(truth_deg):
    """Degrees of a table that knows the answer: every 2 degrees within 20 of the truth, every 30 elsewhere"""
    centre = 2.0 * round(truth_deg / 2.0)
    near = [wrap_deg(centre + k) for k in range(-20, 21, 2)]
    far = [float(d) for d in range(-180, 180, 30) if abs(wrap_deg(d - truth_deg)) > 20]
    return sorted(set(near + far))


def revisit_pair(world, offset):
    """-> (A, B, T_true): scans of one world from the origin and from ``offset``; T_true maps A into B coordinates"""
    w = synth.make_world(world)
    PA, PB = synth.pose_xyz_yaw(0, 0), synth.pose_xyz_yaw(offset[0], offset[1], 0.0, offset[2])
    return synth.scan_world(w, PA, seed=1), synth.scan_world(w, PB, seed=2), np.linalg.inv(PB) @ PA


def other_world():
    return synth.scan_world(synth.make_world(11, ground_z=-4.0), synth.pose_xyz_yaw(0, 0), seed=5)


def true_yaw_deg(T):
    return float(np.degrees(np.arctan2(T[1, 0], T[0, 0])))


@pytest.fixture(scope="module")
def revisits():
    """[(offset, A, B, T_true, restatement's alignment over the reduced table)] for REVISITS"""
    out = []
    for world, o in REVISITS:
        A, B, T_true = revisit_pair(world, o)
        sp, sC = G.prepare(A, 0.5, 20, 1e-3)
        tp, tC = G.prepare(B, 0.5, 20, 1e-3)
        deg = reduced_table(true_yaw_deg(T_true))
        out.append((o, A, B, T_true, PL.align(sp, cov6(sC), tp, cov6(tC), PL.table_of(deg))))
    return out


# ------------------------------------------------------------------------------------------------
# the definition
# ------------------------------------------------------------------------------------------------
def test_restatement_matches_brute_force():
    rng = np.random.default_rng(0)
    # multiples of 1/8 m: every product with 0, +-1 and 1 / cell = 2, every sum and every bin edge is exact
    sp = rng.integers(-12, 13, (15, 3)) / 8.0
    tp = rng.integers(-12, 13, (15, 3)) / 8.0
    sc = np.array([STRUCTURE if i % 4 else GROUND for i in range(15)])
    tc = np.array([GROUND if i % 5 == 2 else STRUCTURE for i in range(15)])
    for kw in (dict(half_bins=2), dict(half_bins=1, source_stride=1), dict(half_bins=3, source_stride=3, cell=1.0),
               dict(half_bins=2, z_window=0.25, normal_z2_max=0.5)):
        v = PL.votes(sp, sc, tp, tc, QUARTER, **kw)
        assert v.sum() > 0 and np.array_equal(v, PL.votes_loop(sp, sc, tp, tc, QUARTER, **kw)), kw
    table = PL.table_of([-180.0, -37.0, 3.0, 91.0])           # inexact cosines
    assert np.array_equal(PL.votes(sp, sc, tp, tc, table, half_bins=2),
                          PL.votes_loop(sp, sc, tp, tc, table, half_bins=2))


def test_inclusive_edges():
    one = dict(half_bins=2, source_stride=1)
    sp, sc = np.zeros((1, 3)), np.array([STRUCTURE])

    def cast(x, y, z, **kw):
        v = PL.votes(sp, sc, np.array([[x, y, z]]), np.array([STRUCTURE]), QUARTER[:1], **dict(one, **kw))
        assert np.array_equal(v, PL.votes_loop(sp, sc, np.array([[x, y, z]]), np.array([STRUCTURE]), QUARTER[:1],
                                               **dict(one, **kw)))
        return v[0]
    # cell 0.5: bx = floor(2 x + 0.5); x = 1.0 -> 2 = half_bins: a vote; x = 1.25 -> 3: none; x = -1.25 -> -2 (a
    # pre-floor value on the edge): a vote; x = -1.5 -> -3: none
    assert cast(1.0, 0.0, 0.0)[4, 2] == 1 and cast(1.25, 0.0, 0.0).sum() == 0
    assert cast(-1.25, 0.0, 0.0)[0, 2] == 1 and cast(-1.5, 0.0, 0.0).sum() == 0
    assert cast(0.0, 1.0, 0.0)[2, 4] == 1 and cast(0.0, 1.25, 0.0).sum() == 0
    assert cast(0.0, -1.25, 0.0)[2, 0] == 1 and cast(0.0, -1.5, 0.0).sum() == 0
    # |dz| = z_window exactly votes, one ulp more does not
    assert cast(0.0, 0.0, 0.5).sum() == 1 and cast(0.0, 0.0, -0.5).sum() == 1
    assert cast(0.0, 0.0, np.nextafter(0.5, 1.0)).sum() == 0 and cast(0.0, 0.0, -np.nextafter(0.5, 1.0)).sum() == 0
    # stray coordinates are compared before they are converted
    for stray in (1e300, -1e300, np.inf, np.nan, 2.0 ** 40):
        v = PL.votes(sp, sc, np.array([[stray, 0.0, 0.0]]), np.array([STRUCTURE]), QUARTER[:1], **one)
        assert v.sum() == 0
    # structure: n_z^2 < normal_z2_max, strictly; fewer than 3 neighbours = the x axis = structure
    eps = 1e-3
    nz2 = np.array([0.0, 0.2, 0.25, 0.3, 1.0])
    czz = 1.0 - (1.0 - eps) * nz2
    got = PL.structure(np.stack([np.ones(5)] * 5 + [czz], 1))
    assert got.tolist() == [True, True, (1.0 - czz[2]) < 0.25 * (1.0 - eps), False, False]
    assert PL.structure(np.array([STRUCTURE])).all() and not PL.structure(np.array([GROUND])).any()
    # source_stride keys on the row index within the cloud, structure or not
    sp4 = np.zeros((4, 3))
    sc4 = np.array([GROUND, STRUCTURE, STRUCTURE, STRUCTURE])
    r = PL.align(sp4, sc4, np.zeros((1, 3)), np.array([STRUCTURE]), QUARTER[:1], half_bins=2, source_stride=2)
    assert r["counts"].tolist() == [1, 1] and r["scores"][0] == 1        # row 2 alone: row 0 is ground


def test_tie_rules_guard_and_empty():
    n = 5
    v = np.zeros((12, n, n), np.int32)
    v[3, 4, 1] = v[3, 1, 4] = 7                              # two bins of one hypothesis: flat 9 < flat 21
    v[8, 2, 2] = 7                                           # two hypotheses: the smaller h
    v[4, 0, 0] = 6                                           # inside the guard of 3
    v[0, 0, 1] = 5                                           # 3 indices from 3: outside a guard of 2
    v[10, 0, 0] = 4
    table = PL.table_of(np.arange(12) * 30.0 - 180.0)
    r = PL.reduce(v, table, cell=0.5, guard=2)
    assert r["best"].tolist() == [3, 1 - 2, 4 - 2] and r["scores"].tolist() == [7, 7]
    assert r["yaw_peaks"][3].tolist() == [7, 9] and r["yaw_peaks"][1].tolist() == [0, 0]
    assert np.array_equal(r["init"][:2, 3], [-0.5, 1.0]) and np.array_equal(r["init"][:2, :2],
                                                                            [[table[3, 0], -table[3, 1]],
                                                                             [table[3, 1], table[3, 0]]])
    v[8] = 0
    assert PL.reduce(v, table, guard=2)["scores"].tolist() == [7, 5]     # h = 4 is skipped, h = 0 counts
    # circular: best at h = 0 with guard 2 skips 10, 11, 1, 2
    w = np.zeros((12, n, n), np.int32)
    w[0, 2, 2], w[11, 0, 0], w[10, 0, 0], w[2, 0, 0], w[9, 0, 0] = 9, 8, 7, 6, 3
    assert PL.reduce(w, table, guard=2)["scores"].tolist() == [9, 3]
    assert PL.reduce(w, table, guard=6)["scores"].tolist() == [9, 0]     # nobody is further than 6 of 12
    assert PL.reduce(w[:1], table[:1], guard=0)["scores"].tolist() == [9, 0]
    # peak 0: nothing in the window, no structure rows, empty clouds
    far = PL.align(np.zeros((2, 3)), np.array([STRUCTURE] * 2), np.full((2, 3), 100.0), np.array([STRUCTURE] * 2),
                   QUARTER, half_bins=2)
    flat = PL.align(np.zeros((2, 3)), np.array([GROUND] * 2), np.zeros((2, 3)), np.array([STRUCTURE] * 2), QUARTER)
    none = PL.align(np.zeros((0, 3)), np.zeros((0, 6)), np.zeros((2, 3)), np.array([STRUCTURE] * 2), QUARTER)
    for r, counts in ((far, [1, 2]), (flat, [0, 2]), (none, [0, 2])):
        assert r["best"].tolist() == [-1, 0, 0] and r["scores"].tolist() == [0, 0] and r["counts"].tolist() == counts
        assert r["init"].tobytes() == np.eye(4).tobytes() and not r["votes"].any()
        assert PL.info(r)["planar_support"] == 0.0 and PL.info(r)["planar_peak_ratio"] == float("inf")
    cs, deg = PL.yaw_table()
    assert cs.shape == (180, 2) and deg[0] == -180.0 and deg[90] == 0.0 and cs[90].tolist() == [1.0, 0.0]


# ------------------------------------------------------------------------------------------------
# ray-cast revisits
# ------------------------------------------------------------------------------------------------
def test_restatement_finds_the_revisits(revisits):
    for o, _, _, T_true, r in revisits:
        te, _ = G.pose_error(r["init"], T_true)
        ye = wrap_deg(PL.info(r)["init_yaw_deg"] - true_yaw_deg(T_true))
        print(o, "best", r["best"], "scores", r["scores"], "counts", r["counts"], "translation error", te,
              "yaw error", ye, "support", PL.info(r)["planar_support"])
        assert te <= GUESS_T_BAR and abs(ye) <= GUESS_YAW_BAR_DEG, (o, te, ye)
        assert r["scores"][0] > r["scores"][1] > 0


@pytest.mark.parametrize("case", range(len(REVISITS)))
def test_gicp_converges_from_the_guess(revisits, case):
    o, A, B, T_true, r = revisits[case]
    out = G.register(A, B, init=r["init"])
    te, re_ = G.pose_error(out["transform"], T_true)
    print(o, "translation error", te, "rotation error deg", np.rad2deg(re_), "fitness", out["fitness"])
    assert te <= T_BAR and re_ <= R_BAR, (te, np.rad2deg(re_))
    assert out["fitness"] >= 0.3 and out["rmse"] <= 0.5


def test_identity_start_verifies_a_wrong_transform(revisits):
    """The gap planar_init closes: from the identity the revisit 5 m away passes the default thresholds on the ground
    plane alone, with a transform that is wrong by the whole offset."""
    o, A, B, T_true, _ = revisits[0]
    assert o == (4.0, -3.0, 17.5)
    out = G.register(A, B)
    te, re_ = G.pose_error(out["transform"], T_true)
    print("fitness", out["fitness"], "rmse", out["rmse"], "translation error", te, "rotation error deg", np.rad2deg(re_))
    assert out["fitness"] >= 0.3 and out["rmse"] <= 0.5
    assert te > 3.0


# ------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from neural_spectral_codec_amd import _lib, build
    build.build_hip()
    return _lib.lib()


def test_planar_abi_validates_on_host(lib):
    from neural_spectral_codec_amd import _lib
    EINVAL, EUNSUP, EWS = -1, -2, -3
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsc.h")).read()
    limits = {k: int(v) for k, v in re.findall(r"#define (NSC_PLANAR_[A-Z_]+)\s+(\d+)", hdr)}
    assert limits == {"NSC_PLANAR_MAX_HALF_BINS": _lib.PLANAR_MAX_HALF_BINS, "NSC_PLANAR_MAX_PAIRS": _lib.PLANAR_MAX_PAIRS}
    assert _lib.PLANAR_MAX_PAIRS <= 65535 and _lib.PLANAR_MAX_HALF_BINS == 32
    assert lib.nsc_abi_version() == _lib.ABI_VERSION == 4     # the symbols are additive
    p = _lib.PlanarParams()
    lib.nsc_planar_default_params(p)
    assert (p.cell, p.z_window, p.normal_z2_max, p.half_bins, p.source_stride, p.guard) == (0.5, 0.5, 0.25, 24, 2, 5)
    assert {k: getattr(p, k) for k in PL.DEFAULTS} == PL.DEFAULTS
    P, H = 3, 180
    need = lib.nsc_planar_align_workspace_bytes(P, H)
    assert need >= P * H * 8 and lib.nsc_planar_align_workspace_bytes(-1, H) == 0
    assert lib.nsc_planar_align_workspace_bytes(P, 0) == 0
    fake = C.c_void_p(4096)                                   # never dereferenced: every check runs before a launch

    def store(**kw):
        a = dict(voxel_size=0.5, epsilon=1e-3, covariance_knn=20, n_clouds=5, n_rows=10000, n_slots=20000,
                 cap_clouds=64, cap_rows=1 << 16, cap_slots=1 << 17,
                 **{k: 4096 for k in ("row_offsets", "slot_offsets", "bounds", "points", "covariances", "slots")})
        a.update(kw)
        return _lib.GicpCloudSet(**a)

    def call(**kw):
        a = dict(src=store(), tgt=store(), sid=fake, tid=fake, P=P, cs=fake, H=H, params=p, best=fake, scores=fake,
                 counts=fake, init=fake, ws=fake, nbytes=need)
        a.update(kw)
        return lib.nsc_planar_align(C.byref(a["src"]) if a["src"] is not None else None,
                                    C.byref(a["tgt"]) if a["tgt"] is not None else None, a["sid"], a["tid"], a["P"],
                                    a["cs"], a["H"], C.byref(a["params"]) if a["params"] is not None else None,
                                    a["best"], a["scores"], a["counts"], a["init"], None, a["ws"], a["nbytes"], None)

    for k in ("src", "tgt", "sid", "tid", "cs", "params", "best", "scores", "counts", "init"):
        assert call(**{k: None}) == EINVAL, k
    assert call(P=-1) == EINVAL and call(H=0) == EINVAL and call(H=-3) == EINVAL
    for k in ("row_offsets", "points", "covariances"):
        assert call(src=store(**{k: None})) == EINVAL and call(tgt=store(**{k: None})) == EINVAL, k
    assert call(src=store(n_rows=(1 << 16) + 1)) == EINVAL and call(tgt=store(n_clouds=-1)) == EINVAL

    def with_(**kw):
        q = _lib.PlanarParams()
        lib.nsc_planar_default_params(q)
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    for kw in (dict(cell=0.0), dict(cell=-0.5), dict(cell=float("nan")), dict(cell=float("inf")), dict(z_window=-1.0),
               dict(z_window=float("nan")), dict(normal_z2_max=float("nan")), dict(source_stride=0),
               dict(source_stride=-2), dict(guard=-1), dict(half_bins=0), dict(half_bins=-4)):
        assert call(params=with_(**kw)) == EINVAL, kw
    assert call(params=with_(half_bins=33)) == EUNSUP and call(params=with_(half_bins=1 << 20)) == EUNSUP
    assert call(params=with_(half_bins=32), nbytes=need - 1) == EWS      # the largest histogram is supported
    assert call(P=_lib.PLANAR_MAX_PAIRS + 1) == EUNSUP and call(P=2 ** 31 - 1) == EUNSUP
    at_limit = lib.nsc_planar_align_workspace_bytes(_lib.PLANAR_MAX_PAIRS, H)
    assert call(P=_lib.PLANAR_MAX_PAIRS, nbytes=at_limit - 1) == EWS
    # a bin must fit int32: sources.n_rows * min(36, targets.n_rows) <= 2^31 - 1 at the defaults
    big = dict(cap_rows=1 << 40)
    limit = (2 ** 31 - 1) // 36
    assert call(src=store(n_rows=limit, **big), tgt=store(n_rows=1 << 30, **big), nbytes=need - 1) == EWS
    assert call(src=store(n_rows=limit + 1, **big), tgt=store(n_rows=1 << 30, **big)) == EUNSUP
    assert call(src=store(n_rows=1 << 30, **big), tgt=store(n_rows=1), nbytes=need - 1) == EWS      # 2^30 x 1 fits
    assert call(src=store(n_rows=1 << 30, **big), tgt=store(n_rows=2)) == EUNSUP
    assert call(nbytes=need - 1) == EWS and call(ws=None) == EWS
    assert call(P=0) == 0 and call(P=0, sid=None, best=None, ws=None, nbytes=0) == 0       # nothing launched
