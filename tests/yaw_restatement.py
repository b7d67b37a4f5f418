"""Float64 numpy restatement of the yaw initial guess (retrieval/yaw_alignment.py's definition; the kernel is
csrc/nsc_yaw.hip).  Independent of the library: the direct circular cross-correlation through numpy sums."""
import numpy as np

from neural_spectral_codec_amd import synth

GUARD_BINS = 10          # include/nsc.h NSC_YAW_GUARD_BINS
N_AZIMUTH = 360


def scores(Iq, Ic):
    """score[s] = sum_r sum_c a[r,c] b[r,(c - s) mod 360] of the mean-removed images, s = 0 .. 359"""
    Iq, Ic = np.asarray(Iq, np.float64), np.asarray(Ic, np.float64)
    assert Iq.shape == Ic.shape and Iq.ndim == 2 and Iq.shape[1] == N_AZIMUTH and 1 <= Iq.shape[0] <= 64
    a = Iq - Iq.mean(1, keepdims=True)
    b = Ic - Ic.mean(1, keepdims=True)
    return np.array([(a * np.roll(b, s, axis=1)).sum() for s in range(N_AZIMUTH)])


def circular_distance(s, shift):
    d = np.abs(np.asarray(s) - shift)
    return np.minimum(d, N_AZIMUTH - d)


def yaw_deg(shift):
    """-shift degrees wrapped to (-180, 180]"""
    return float(-shift if shift < 180 else N_AZIMUTH - shift)


def init_transform(shift):
    """Rz(yaw) with zero translation; exactly the identity for shift 0"""
    return np.eye(4) if shift == 0 else synth.pose_xyz_yaw(0.0, 0.0, 0.0, yaw_deg(shift))


def align(Iq, Ic):
    """-> dict(scores, shift, peak, runner_up, second, yaw_deg, init): ``second`` is the best score over all other
    shifts (the tests' margin against a tie)"""
    sc = scores(Iq, Ic)
    shift = int(np.argmax(sc))                               # the first of equal maxima: ties to the smaller s
    second = float(np.delete(sc, shift).max())
    if not sc[shift] > 0:
        shift = 0
    far = circular_distance(np.arange(N_AZIMUTH), shift) > GUARD_BINS
    return dict(scores=sc, shift=shift, peak=float(sc[shift]), runner_up=float(sc[far].max()), second=second,
                yaw_deg=yaw_deg(shift), init=init_transform(shift))


def wrap_deg(d):
    """an angle difference in degrees wrapped to (-180, 180]"""
    return -((-d + 180.0) % 360.0 - 180.0)
