"""Constructed range-image pairs on which the yaw initial guess (csrc/nsc_yaw.hip, retrieval/yaw_alignment.py) is
exact or not well posed, shared by test_yaw_cpu.py and test_yaw_gpu.py: exact ties between shifts, the informative row
at every edge of the kernel's 16-row chunks and 4-row groups, denormal and very large pixels, and pixels that are not
finite.

Integer images.  Every pixel is a non-negative integer and every row sum a multiple of 360, so the row means, the
mean-removed images, every product and every partial sum are integers far below 2^53: the float64 scores are exact
whatever the order of summation, and ``int_scores`` (an int64 correlation through np.roll, independent of
yaw_restatement) is their reference bit for bit.  A power-of-two scale keeps all of that exact.

Every case is a ``Case``: the two float32 images and what the case claims (``ties``: all shifts that share the largest
score, ``shift``, ``peak``, ``runner_up``).  The claims are written down from the construction, not computed:
``int_align`` of the unscaled images must reproduce them (test_yaw_cpu.py).
"""
from functools import lru_cache
from typing import NamedTuple, Optional, Tuple

import numpy as np

N_AZIMUTH = 360
GUARD_BINS = 10          # include/nsc.h NSC_YAW_GUARD_BINS

# ---- the int64 reference ---------------------------------------------------------------------------------------------


def int_scores(Iq, Ic):
    """(360,) int64 scores of two integer images whose row sums are multiples of 360"""
    q, c = np.asarray(Iq), np.asarray(Ic)
    assert q.shape == c.shape and q.ndim == 2 and q.shape[1] == N_AZIMUTH
    qi, ci = q.astype(np.int64), c.astype(np.int64)
    assert np.array_equal(qi, q) and np.array_equal(ci, c) and qi.min() >= 0 and ci.min() >= 0
    sq, sc = qi.sum(1, keepdims=True), ci.sum(1, keepdims=True)
    assert not (sq % N_AZIMUTH).any() and not (sc % N_AZIMUTH).any()
    a, b = qi - sq // N_AZIMUTH, ci - sc // N_AZIMUTH
    return np.array([(a * np.roll(b, s, axis=1)).sum() for s in range(N_AZIMUTH)], dtype=np.int64)


def circular_distance(s, shift):
    d = np.abs(np.asarray(s) - shift)
    return np.minimum(d, N_AZIMUTH - d)


def int_align(Iq, Ic):
    """-> dict(scores, ties, shift, peak, runner_up) in integers: the definition of yaw_alignment.py"""
    sc = int_scores(Iq, Ic)
    ties = tuple(int(s) for s in np.flatnonzero(sc == sc.max()))
    shift = ties[0] if sc.max() > 0 else 0
    far = circular_distance(np.arange(N_AZIMUTH), shift) > GUARD_BINS
    return dict(scores=sc, ties=ties, shift=shift, peak=int(sc[shift]), runner_up=int(sc[far].max()))


def init_transform(shift):
    """Rz(-shift degrees wrapped to (-180, 180]) as yaw_alignment.py defines it; exactly the identity for shift 0"""
    T = np.eye(4)
    if shift:
        yaw = np.deg2rad(float(-shift if shift < 180 else N_AZIMUTH - shift))
        T[0, 0] = T[1, 1] = np.cos(yaw)
        T[0, 1], T[1, 0] = -np.sin(yaw), np.sin(yaw)
    return T


# ---- cases -----------------------------------------------------------------------------------------------------------

class Case(NamedTuple):
    name: str
    Iq: np.ndarray                   # (R, 360) float32
    Ic: np.ndarray
    ties: Tuple[int, ...]            # every shift with the largest score, ascending
    shift: int
    peak: float                      # exact in float64
    runner_up: float
    scale_log2: int = 0              # the pixels are the integer images times 2^scale_log2
    base: Optional[str] = None       # a scaled case: the name of its unscaled case

    @property
    def rows(self):
        return self.Iq.shape[0]


DELTA_PEAK, DELTA_FLOOR = 128880, -720       # 360 * 358 at the two tied shifts, 360 * -2 at the 358 others

# (tied shifts): what the pair exercises in yaw_align_kernel's arg-max
TIE_PAIRS = (
    (353, 357),          # both inside the guard
    (63, 64),            # decided by the butterfly; the larger shift sits in the lower lane
    (127, 128),          # the same across lanes 63 and 0, and across the waves that summed them
    (0, 359),            # circular guard
    (100, 300),          # two lanes, outside the guard: runner_up == peak
    (0, 64),             # one lane of the scan, decided by its strict >
    (254, 255),          # the second wave boundary of the sums (shift pairs 127 | 128) ...
    (255, 256),          # ... from both sides
    (200, 201),          # the two shifts one lane of the sums owns (2t, 2t + 1 for t = 100)
)
# (R, r0): where the only informative row lies among the chunks of 16 rows and their groups of 4
ROWS = (
    (1, 0),              # one row
    (16, 15),            # last of a full chunk
    (17, 16),            # alone in a one-row last chunk
    (33, 32),            # the same in the third chunk
    (49, 47),            # last of a full chunk that a one-row chunk follows
    (64, 63),            # last row of the last full chunk
    (15, 14), (31, 30), (63, 62),            # last of a 15-row last chunk (its last group is partial): chunks 0, 1, 3
    (48, 47),            # last of the last full chunk, chunk 2
    (64, 48),            # first row of chunk 3
)
SCALES = (-140, 100)     # 360 * 2^-140 is a float32 denormal, 360 * 2^100 is large; both are exact


def _delta_images(R, r0, s1, s2):
    """query: 360 at column 0 of row r0; candidate: 360 at the columns (-s1) mod 360 and (-s2) mod 360 of row r0"""
    Iq, Ic = np.zeros((R, N_AZIMUTH), np.float32), np.zeros((R, N_AZIMUTH), np.float32)
    Iq[r0, 0] = 360.0
    Ic[r0, (-s1) % N_AZIMUTH] = Ic[r0, (-s2) % N_AZIMUTH] = 360.0
    return Iq, Ic


def delta(R, r0, s1, s2, scale_log2=0, name=None):
    """The two-way tie between shifts s1 and s2: score 128 880 at both and -720 at every other shift, exactly.  The
    smaller shift wins; runner_up is -720 when the two lie within the guard of each other, else equal to the peak."""
    Iq, Ic = _delta_images(R, r0, s1, s2)
    lo, hi = min(s1, s2), max(s1, s2)
    near = int(circular_distance(hi, lo)) <= GUARD_BINS
    k = 2.0 ** scale_log2
    base = f"delta R={R} r0={r0} ties=({s1},{s2})"
    return Case(name or (base if not scale_log2 else f"{base} x2^{scale_log2}"),
                (Iq * np.float32(k)), (Ic * np.float32(k)), (lo, hi), lo, DELTA_PEAK * k * k,
                (DELTA_FLOOR if near else DELTA_PEAK) * k * k, scale_log2, base if scale_log2 else None)


def periodic(period, planted=47, seed=0, R=16):
    """A random integer image of the given column period against itself rolled by -planted: an (360 / period)-way tie at
    planted mod period + k period.  Period 120: three ties, all outside the guard of each other; period 5: 72 ties,
    inside and outside the guard at once.  Either way runner_up == peak."""
    assert N_AZIMUTH % period == 0 and period < N_AZIMUTH
    rng = np.random.default_rng(1000 * period + seed)
    block = rng.integers(0, 80, (R, period)).astype(np.int64)
    block[:, 0] += (-block.sum(1)) % period                  # every row sum of the block divisible by the period
    Iq = np.tile(block, (1, N_AZIMUTH // period)).astype(np.float32)
    Ic = np.roll(Iq, -planted, axis=1)
    ties = tuple(range(planted % period, N_AZIMUTH, period))
    centred = block - block.sum(1, keepdims=True) // period
    peak = float((N_AZIMUTH // period) * (centred * centred).sum())      # the zero-lag autocorrelation
    return Case(f"periodic {period}", Iq, Ic, ties, ties[0], peak, peak)


@lru_cache(maxsize=None)
def delta_cases():
    """every TIE_PAIRS entry at every ROWS entry, (0, 359) also built from the columns in the other order"""
    out = []
    for R, r0 in ROWS:
        for s1, s2 in TIE_PAIRS:
            out.append(delta(R, r0, s1, s2))
        out.append(delta(R, r0, 359, 0, name=f"delta R={R} r0={r0} ties=(359,0)"))
    return tuple(out)


@lru_cache(maxsize=None)
def scaled_delta_cases():
    out = []
    for k in SCALES:
        for R, r0 in ROWS:
            for s1, s2 in TIE_PAIRS:
                out.append(delta(R, r0, s1, s2, scale_log2=k))
    return tuple(out)


@lru_cache(maxsize=None)
def periodic_cases():
    return periodic(120), periodic(90), periodic(5)


def exact_cases():
    """the whole exact family: every case's outputs are claimed bit for bit"""
    return delta_cases() + scaled_delta_cases() + periodic_cases()


_INT_ALIGN = {}


def expected(case):
    """The outputs nsc_yaw_align must give for ``case``, bit for bit, from the int64 reference and not from the case's
    claims: dict(shift int32, peak, runner_up float64, init_transforms (4,4) float64, scores (360,) float64, ties).
    A scaled case takes its unscaled case's integers times 4^scale_log2, which is exact."""
    key = case.base or case.name
    if key not in _INT_ALIGN:
        k = 2.0 ** -case.scale_log2                          # undo the scale in float64: exact, integers again
        _INT_ALIGN[key] = int_align(case.Iq.astype(np.float64) * k, case.Ic.astype(np.float64) * k)
    r = _INT_ALIGN[key]
    k2 = 4.0 ** case.scale_log2
    return dict(shift=np.int32(r["shift"]), peak=np.float64(r["peak"] * k2), runner_up=np.float64(r["runner_up"] * k2),
                init_transforms=init_transform(r["shift"]), scores=r["scores"].astype(np.float64) * k2, ties=r["ties"])


def by_rows(cases):
    """{R: [cases of R rows]}: what one launch can hold"""
    out = {}
    for c in cases:
        out.setdefault(c.rows, []).append(c)
    return out


def finite_maximum(seed=3):
    """(Iq, Ic, planted): a (2, 360) pair of +-3.4e38 pixels, the candidate rolled by -2.  Not integer-exact: the scores
    are finite (about 720 * 3.4e38^2 = 8.3e79 at the peak) and held to the float tolerance of the ordinary images."""
    rng = np.random.default_rng(seed)
    Iq = (np.float32(3.4e38) * rng.choice(np.array([-1.0, 1.0], np.float32), (2, N_AZIMUTH))).astype(np.float32)
    return Iq, np.roll(Iq, -2, axis=1), 2


# ---- images that are not finite ----------------------------------------------------------------------------------------

NONFINITE = ("nan", "+inf", "-inf", "+inf and -inf")


def poisoned(image, kind, row, col=123):
    """a copy of ``image`` with one pixel of ``row`` not finite (two for '+inf and -inf': their row sum is NaN where a
    single inf gives an inf mean)"""
    out = np.array(image, dtype=np.float32, copy=True)
    if kind == "nan":
        out[row, col] = np.nan
    elif kind == "+inf":
        out[row, col] = np.inf
    elif kind == "-inf":
        out[row, col] = -np.inf
    else:
        assert kind == "+inf and -inf"
        out[row, col], out[row, (col + 100) % N_AZIMUTH] = np.inf, -np.inf
    return out


def nonfinite_pairs(R, seed=0):
    """[(name, Iq, Ic)] for R rows: every kind of NONFINITE in the query only, the candidate only and both, in the
    first row and in the last (one set for R = 1), on ordinary random images"""
    rng = np.random.default_rng(500 + R + seed)
    q = rng.uniform(0.0, 80.0, (R, N_AZIMUTH)).astype(np.float32)
    c = rng.uniform(0.0, 80.0, (R, N_AZIMUTH)).astype(np.float32)
    out = []
    for row in sorted({0, R - 1}):
        for kind in NONFINITE:
            pq, pc = poisoned(q, kind, row), poisoned(c, kind, row, col=7)
            out += [(f"R={R} row {row} {kind} in the query", pq, c), (f"R={R} row {row} {kind} in the candidate", q, pc),
                    (f"R={R} row {row} {kind} in both", pq, pc)]
    return out
