"""The yaw initial guess without a GPU: the float64 restatement (tests/yaw_restatement.py) on the oracle's range images
of ray-cast revisits finds the yaw to 3 degrees, the restatement's GICP converges from that guess and, from the
identity, ends 90 degrees wrong with a passing fitness; nsc_yaw_align validates its arguments on the host."""
import ctypes as C

import numpy as np
import pytest

import gicp_restatement as G
import nsc_oracle
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
