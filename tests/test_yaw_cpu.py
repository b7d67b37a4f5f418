"""The yaw initial guess without a GPU: the float64 restatement (tests/yaw_restatement.py) on the oracle's range images
of ray-cast revisits finds the yaw to 3 degrees, the restatement's GICP converges from that guess and, from the
identity, ends 90 degrees wrong with a passing fitness; every claim of the constructed cases (tests/yaw_cases.py: exact
ties, scalings, images that are not finite) holds on the restatement and on an int64 reference; yaw_info's contract;
nsc_yaw_align validates its arguments on the host."""
import ctypes as C

import numpy as np
import pytest

import gicp_restatement as G
import nsc_oracle
import yaw_cases as YC
import yaw_restatement as Y
from neural_spectral_codec_amd import synth
from test_gicp_cpu import R_BAR, REVISITS, T_BAR, revisit

# (x, y, yaw deg) of the second visit of world 3: revisits under another heading, from the identity outside GICP's basin
ROTATED = [(0.5, 0.3, 90.0), (1.0, -0.5, 180.0), (0.0, 0.0, -120.0), (0.8, 0.6, 45.0), (0.3, -0.9, -60.0),
           (0.6, -0.4, 137.3)]
UNGUESSED = [o for o, g in REVISITS if g is None]            # 2, 5 and 10 degrees: inside the basin already
YAW_BAR_DEG = 3.0        # the worst of a 45-revisit sweep (worlds 3, 5, 7; translation up to 1 m) was 2.53 degrees
MARGIN = 1e-6            # best score over the second best of all shifts, relative to the peak: no case is a tie


def images_of(A, B):
    return nsc_oracle.encode_points(A, want_images=True)[2], nsc_oracle.encode_points(B, want_images=True)[2]


def assert_margin(r):
    assert r["peak"] > 0 and r["peak"] - r["second"] > MARGIN * r["peak"], (r["peak"], r["second"])


@pytest.fixture(scope="module")
def rotated():
    """[(offset, A, B, T_true, restatement's alignment)] for ROTATED"""
    out = []
    for o in ROTATED:
        A, B, T_true, _ = revisit(o, None)
        out.append((o, A, B, T_true, Y.align(*images_of(A, B))))
    return out


def test_restatement_finds_the_yaw(rotated):
    cases = [(o, r) for o, _, _, _, r in rotated]
    for o in UNGUESSED:
        A, B, _, _ = revisit(o, None)
        cases.append((o, Y.align(*images_of(A, B))))
    assert len(cases) == 9
    for o, r in cases:
        assert_margin(r)
        err = Y.wrap_deg(r["yaw_deg"] + o[2])                # the guess maps query into candidate: -yaw of the offset
        print(o, "shift", r["shift"], "yaw error", err, "peak ratio", r["peak"] / r["runner_up"])
        assert abs(err) <= YAW_BAR_DEG, (o, r["shift"], err)
        assert abs(Y.wrap_deg(o[2] - r["shift"])) <= YAW_BAR_DEG     # a sensor yawed by +theta: shift ~ theta


def test_restatement_definition():
    rng = np.random.default_rng(0)
    I = rng.uniform(1, 80, (16, 360)).astype(np.float32)
    for planted in (0, 1, 179, 180, 181, 359):
        r = Y.align(I, np.roll(I, -planted, axis=1))           # Ic[c] = Iq[c + s]: the candidate sensor yawed by +s
        assert r["shift"] == planted and r["peak"] > r["runner_up"]
        assert -180.0 < r["yaw_deg"] <= 180.0 and (r["yaw_deg"] + planted) % 360 == 0
    assert Y.align(I, I)["init"].tobytes() == np.eye(4).tobytes()
    flat = Y.align(np.full((16, 360), 7.5, np.float32), I)
    assert flat["shift"] == 0 and flat["peak"] == 0.0 and np.array_equal(flat["init"], np.eye(4))
    # the FFT form of the same sums
    J = rng.uniform(1, 80, (16, 360)).astype(np.float32)
    a, b = I - I.astype(np.float64).mean(1, keepdims=True), J - J.astype(np.float64).mean(1, keepdims=True)
    fft = np.fft.irfft((np.fft.rfft(a, axis=1) * np.conj(np.fft.rfft(b, axis=1))).sum(0), 360)
    sc = Y.scores(I, J)
    assert np.max(np.abs(fft - sc)) <= 1e-12 * np.max(np.abs(sc))
    # runner-up: the guard excludes the peak's neighbourhood, circularly
    sc = Y.align(I, np.roll(I, -3, axis=1))
    far = [s for s in range(360) if min(abs(s - 3), 360 - abs(s - 3)) > Y.GUARD_BINS]
    assert len(far) == 360 - 21 and sc["runner_up"] == sc["scores"][far].max()


@pytest.mark.parametrize("case", range(len(ROTATED)))
def test_gicp_converges_from_the_guess(rotated, case):
    o, A, B, T_true, r = rotated[case]
    out = G.register(A, B, init=r["init"])
    te, re = G.pose_error(out["transform"], T_true)
    print(o, "translation error", te, "rotation error deg", np.rad2deg(re), "fitness", out["fitness"])
    assert te <= T_BAR and re <= R_BAR, (te, np.rad2deg(re))
    assert out["fitness"] >= 0.3 and out["rmse"] <= 0.5


def test_identity_start_verifies_a_wrong_transform(rotated):
    """The gap yaw_init closes: from the identity the 90-degree revisit passes the default thresholds on the ground
    plane alone, with a transform that is wrong by the whole yaw."""
    o, A, B, T_true, _ = rotated[0]
    assert o == (0.5, 0.3, 90.0)
    out = G.register(A, B)
    te, re = G.pose_error(out["transform"], T_true)
    print("fitness", out["fitness"], "rmse", out["rmse"], "rotation error deg", np.rad2deg(re))
    assert out["fitness"] >= 0.3 and out["rmse"] <= 0.5
    assert np.rad2deg(re) > 45.0


# ------------------------------------------------------------------------------------------------
# the constructed cases of yaw_cases.py: every claim, on the int64 reference and on the restatement
# ------------------------------------------------------------------------------------------------
IDENTITY = np.eye(4).tobytes()


def test_case_family_is_the_one_described():
    deltas, scaled, per = YC.delta_cases(), YC.scaled_delta_cases(), YC.periodic_cases()
    assert len(YC.ROWS) == 11 and len(YC.TIE_PAIRS) == 9
    assert len(deltas) == 11 * 10 and len(scaled) == 2 * 11 * 9 and len(per) == 3
    assert len({c.name for c in YC.exact_cases()}) == len(YC.exact_cases())
    assert sorted(YC.by_rows(YC.exact_cases())) == [1, 15, 16, 17, 31, 33, 48, 49, 63, 64]
    for c in YC.exact_cases():
        assert c.Iq.dtype == c.Ic.dtype == np.float32 and c.Iq.shape == c.Ic.shape == (c.rows, 360)
        assert np.isfinite(c.Iq).all() and np.isfinite(c.Ic).all()
    # the rows: the informative one is the last of a chunk, the first of the next, or closes a partial group
    assert {(R, r0) for R, r0 in YC.ROWS if r0 % 16 == 15} == {(16, 15), (49, 47), (64, 63), (48, 47)}
    assert {(R, r0) for R, r0 in YC.ROWS if r0 % 16 == 0} == {(1, 0), (17, 16), (33, 32), (64, 48)}
    assert {(R, r0) for R, r0 in YC.ROWS if R % 16 == 15} == {(15, 14), (31, 30), (63, 62)}
    # the scales: a float32 denormal and a large value, both exact
    tiny, huge = np.float32(360.0) * np.float32(2.0 ** -140), np.float32(360.0) * np.float32(2.0 ** 100)
    assert 0 < tiny < np.finfo(np.float32).tiny and float(tiny) == 360.0 * 2.0 ** -140
    assert float(huge) == 360.0 * 2.0 ** 100


@pytest.mark.parametrize("R", sorted(YC.by_rows(YC.delta_cases())))
def test_delta_ties_on_reference_and_restatement(R):
    for c in YC.by_rows(YC.delta_cases())[R]:
        ref = YC.int_align(c.Iq, c.Ic)
        sc = ref["scores"]
        lo, hi = c.ties
        assert ref["ties"] == c.ties and lo < hi, c.name
        assert sc[lo] == sc[hi] == YC.DELTA_PEAK and np.all(np.delete(sc, [lo, hi]) == YC.DELTA_FLOOR), c.name
        assert (ref["shift"], ref["peak"], ref["runner_up"]) == (c.shift, c.peak, c.runner_up) and c.shift == lo, c.name
        near = min(hi - lo, 360 - (hi - lo)) <= Y.GUARD_BINS
        assert c.runner_up == (YC.DELTA_FLOOR if near else c.peak), c.name
        r = Y.align(c.Iq, c.Ic)
        assert np.array_equal(r["scores"], sc), c.name        # float64 against int64: exact
        assert (r["shift"], r["peak"], r["runner_up"], r["second"]) == (c.shift, c.peak, c.runner_up, c.peak), c.name
        e = YC.expected(c)
        assert r["init"].tobytes() == e["init_transforms"].tobytes() == Y.init_transform(c.shift).tobytes(), c.name
        assert (int(e["shift"]), float(e["peak"]), float(e["runner_up"])) == (c.shift, c.peak, c.runner_up), c.name
    # which of the pairs lie inside the guard
    inside = {p for p in YC.TIE_PAIRS if YC.delta(16, 15, *p).runner_up == YC.DELTA_FLOOR}
    assert inside == set(YC.TIE_PAIRS) - {(100, 300), (0, 64)}


def test_delta_column_order_is_one_image():
    a, b = YC.delta(17, 16, 0, 359), YC.delta(17, 16, 359, 0)
    assert a.Ic.tobytes() == b.Ic.tobytes() and a[3:7] == b[3:7] and a.ties == (0, 359) and a.shift == 0


def test_periodic_ties_on_reference_and_restatement():
    for c, n in zip(YC.periodic_cases(), (3, 4, 72)):
        ref = YC.int_align(c.Iq, c.Ic)
        assert ref["ties"] == c.ties and len(c.ties) == n and c.ties[0] == 47 % (360 // n), c.name
        assert (ref["shift"], ref["peak"], ref["runner_up"]) == (c.shift, c.peak, c.runner_up), c.name
        assert c.shift == c.ties[0] and c.runner_up == c.peak > 0, c.name
        r = Y.align(c.Iq, c.Ic)
        assert np.array_equal(r["scores"], ref["scores"]), c.name
        assert (r["shift"], r["peak"], r["runner_up"], r["second"]) == (c.shift, c.peak, c.peak, c.peak), c.name
    p120, _, p5 = YC.periodic_cases()
    assert p120.ties == (47, 167, 287)
    d = YC.circular_distance(np.array(p5.ties), p5.shift)      # period 5: ties inside and outside the guard at once
    assert p5.shift == 2 and (d[1:] <= Y.GUARD_BINS).any() and (d > Y.GUARD_BINS).any()


@pytest.mark.parametrize("R", sorted(YC.by_rows(YC.scaled_delta_cases())))
def test_scaling_is_exact_on_the_restatement(R):
    base = {c.name: c for c in YC.delta_cases()}
    for c in YC.by_rows(YC.scaled_delta_cases())[R]:
        b, k = base[c.base], 2.0 ** c.scale_log2
        assert c.scale_log2 in YC.SCALES and np.array_equal(c.Iq.astype(np.float64), b.Iq.astype(np.float64) * k), c.name
        assert np.array_equal(c.Ic.astype(np.float64), b.Ic.astype(np.float64) * k), c.name
        assert (c.shift, c.ties) == (b.shift, b.ties) and c.peak == b.peak * k * k > 0, c.name
        assert c.runner_up == b.runner_up * k * k and np.isfinite(c.peak), c.name
        r = Y.align(c.Iq, c.Ic)
        e = YC.expected(c)
        assert np.array_equal(r["scores"], e["scores"]), c.name
        assert np.array_equal(e["scores"], YC.int_align(b.Iq, b.Ic)["scores"].astype(np.float64) * k * k), c.name
        assert (r["shift"], r["peak"], r["runner_up"]) == (c.shift, c.peak, c.runner_up), c.name
        assert (int(e["shift"]), float(e["peak"]), float(e["runner_up"])) == (c.shift, c.peak, c.runner_up), c.name
    assert YC.DELTA_PEAK * 2.0 ** -280 > np.finfo(np.float64).tiny and YC.DELTA_PEAK * 2.0 ** 200 < 1e300


def test_finite_maximum_on_the_restatement():
    Iq, Ic, planted = YC.finite_maximum()
    assert Iq.shape == (2, 360) and np.all(np.abs(Iq) == np.float32(3.4e38)) and np.isfinite(Iq).all()
    r = Y.align(Iq, Ic)
    assert np.isfinite(r["scores"]).all() and r["shift"] == planted == 2
    assert 8.2e79 < r["peak"] < 8.4e79
    assert_margin(r)


@pytest.mark.parametrize("R", [1, 16, 17])
def test_nonfinite_images_on_the_restatement(R):
    pairs = YC.nonfinite_pairs(R)
    assert len(pairs) == 3 * len(YC.NONFINITE) * (1 if R == 1 else 2)
    for name, Iq, Ic in pairs:
        bad_q, bad_c = ~np.isfinite(Iq), ~np.isfinite(Ic)
        assert 1 <= bad_q.sum() + bad_c.sum() <= 4 and ("both" in name) == (bad_q.any() and bad_c.any()), name
        rows = set(np.flatnonzero(bad_q.any(1))) | set(np.flatnonzero(bad_c.any(1)))
        assert len(rows) == 1 and rows <= {0, R - 1}, name
        with np.errstate(invalid="ignore"):
            r = Y.align(Iq, Ic)
        assert np.isnan(r["scores"]).all(), name             # one pixel: every one of the 360 scores
        assert r["shift"] == 0 and np.isnan(r["peak"]) and np.isnan(r["runner_up"]), name
        assert r["init"].tobytes() == IDENTITY and r["yaw_deg"] == 0.0, name


def test_yaw_info_contract():
    from neural_spectral_codec_amd.retrieval.yaw_alignment import yaw_info
    nan, inf = float("nan"), float("inf")
    assert yaw_info(350, 6.0, 4.0) == dict(init_yaw_deg=10.0, yaw_peak_ratio=1.5)           # finite peak and runner_up
    assert yaw_info(90, 6.0, 0.0) == dict(init_yaw_deg=-90.0, yaw_peak_ratio=inf)           # runner_up <= 0
    assert yaw_info(3, 128880.0, -720.0) == dict(init_yaw_deg=-3.0, yaw_peak_ratio=inf)
    for shift, runner_up, deg in ((0, nan, 0.0),            # an image that is not finite
                                  (0, -inf, 0.0),           # a NaN peak decides, whatever runner_up is
                                  (-1, nan, nan)):          # an invalid id
        info = yaw_info(shift, nan, runner_up)
        assert set(info) == {"init_yaw_deg", "yaw_peak_ratio"} and np.isnan(info["yaw_peak_ratio"]), (shift, runner_up)
        assert info["init_yaw_deg"] == deg or (np.isnan(deg) and np.isnan(info["init_yaw_deg"])), (shift, runner_up)
    info = yaw_info(np.float64(180.0), np.float64(2.0), np.float64(1.0))                    # numpy scalars, as stage 2 passes
    assert info == dict(init_yaw_deg=180.0, yaw_peak_ratio=2.0)


@pytest.fixture(scope="module")
def lib():
    from neural_spectral_codec_amd import _lib, build
    build.build_hip()
    return _lib.lib()


def test_yaw_abi_validates_on_host(lib):
    import os
    import re
    from neural_spectral_codec_amd import _lib
    EINVAL, EUNSUP = -1, -2
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsc.h")).read()
    limits = {k: int(v) for k, v in re.findall(r"#define (NSC_YAW_[A-Z_]+)\s+(\d+)", hdr)}
    assert limits == {"NSC_YAW_GUARD_BINS": _lib.YAW_GUARD_BINS, "NSC_YAW_MAX_PAIRS": _lib.YAW_MAX_PAIRS}
    assert _lib.YAW_GUARD_BINS == Y.GUARD_BINS == 10
    assert _lib.YAW_MAX_PAIRS * 768 < 2 ** 32                 # threads of one launch
    assert lib.nsc_abi_version() == _lib.ABI_VERSION == 4     # the symbol is additive
    fake = C.c_void_p(4096)                                   # never dereferenced: every check runs before a launch

    def call(**kw):
        a = dict(iq=fake, nq=5, ic=fake, nc=7, idq=fake, idc=fake, P=3, R=16, shift=fake, scores=fake, init=fake)
        a.update(kw)
        return lib.nsc_yaw_align(a["iq"], a["nq"], a["ic"], a["nc"], a["idq"], a["idc"], a["P"], a["R"], a["shift"],
                                 a["scores"], a["init"], None)

    for k in ("iq", "ic", "idq", "idc", "shift", "scores", "init"):
        assert call(**{k: None}) == EINVAL, k
    for k in ("nq", "nc", "P"):
        assert call(**{k: -1}) == EINVAL, k
    for R in (0, -1, 65, 1 << 20):
        assert call(R=R) == EINVAL, R
    assert call(P=_lib.YAW_MAX_PAIRS + 1) == EUNSUP and call(P=2 ** 31 - 1) == EUNSUP
    assert call(P=0) == 0 and call(P=0, iq=None, idq=None, init=None) == 0      # nothing to do, nothing launched
