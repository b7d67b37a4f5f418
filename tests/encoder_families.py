"""Constructed range images for the encoder's image stage, and the table of cases that sends them through every copy of it.

Everything after the scatter (sqrt, circular interpolation, empty-row fill, row pooling, 360-point FFT, bin histogram, L1
normalisation) exists five times in csrc/nsc_encoder.hip: ``finish_fast`` (encode_fast_kernel), ``finish_image<4>``,
``<8>`` and ``<16>`` (encode_fused_kernel, chosen by n_elevation) and ``finish_image<8>`` inside finish_kernel with its
three modes.  Dense random clouds leave most of their branches untaken, so the images here are built pixel by pixel: a
family is a named, seeded generator of a float32 (E, 360) image, values in [2, 70], 0 = no return, for any E in 1..64.

No GPU and no product code in this module: tests/test_encoder_families_cpu.py pins the oracle and the table on the CPU,
tests/test_encoder_paths_gpu.py runs the table on the device.
"""
import functools
from collections import namedtuple

import numpy as np

import nsc_oracle as orc

A = 360
F = 181
EDGE_COLS = (0, 63, 64, 319, 320, 359)       # first / last column of 64-column words 0, 1, 4 and 5 (word 5 holds 320..359)
ELEV_RANGE = (-24.8, 2.0)                    # the default field of view: what encode_fast_kernel requires
SPLIT_POINTS = 32768                         # smallest cloud that nsc_encode_clouds splits (2 parts of SPLIT_MIN_PTS)
HOLES = {"neg1": np.float32(-1.0), "negzero": np.float32(-0.0), "nan": np.float32(np.nan)}   # all fail `> 0`


def _rng(name, E, seed=0):
    return np.random.default_rng([sum(map(ord, name)), E, seed])


def _vals(rng, shape):
    return rng.uniform(2.0, 70.0, shape).astype(np.float32)


def _busy_row(rng):
    """A valid row of the row families: random ranges with about a fifth of the pixels missing."""
    row = _vals(rng, A)
    row[rng.random(A) < 0.2] = 0.0
    row[rng.integers(0, A)] = np.float32(33.0)               # never empty
    return row


# ------------------------------------------------------------------------------------------------------------------
# mask families: what interp_row_v searches for
# ------------------------------------------------------------------------------------------------------------------
def single_px(E, seed=0):
    """One valid pixel per row, at the word-edge columns in turn: the pixel is its own previous and next neighbour."""
    rng, img = _rng("single_px", E, seed), np.zeros((E, A), np.float32)
    for r in range(E):
        img[r, EDGE_COLS[r % 6]] = _vals(rng, ())
    return img


def one_hole(E, seed=0):
    """359 valid pixels, the hole at the word-edge columns in turn."""
    rng = _rng("one_hole", E, seed)
    img = _vals(rng, (E, A))
    for r in range(E):
        img[r, EDGE_COLS[r % 6]] = 0.0
    return img


def word5_only(E, seed=0):
    """Valid pixels only in columns 320..359 (the short last word); every other column wraps to reach them."""
    rng, img = _rng("word5_only", E, seed), np.zeros((E, A), np.float32)
    for r in range(E):
        cols = rng.choice(np.arange(320, A), size=1 + r % 7, replace=False)
        img[r, cols] = _vals(rng, len(cols))
    return img


def word0_only(E, seed=0):
    """Valid pixels only in columns 0..63."""
    rng, img = _rng("word0_only", E, seed), np.zeros((E, A), np.float32)
    for r in range(E):
        cols = rng.choice(np.arange(0, 64), size=1 + r % 7, replace=False)
        img[r, cols] = _vals(rng, len(cols))
    return img


def two_px(E, seed=0, rows=None):
    """Two valid pixels per row: in the same word on even rows, in words 0 and 5 on odd rows, so that the short way
    between them crosses 359 -> 0.  ``rows`` restricts the image to those rows (the others stay empty)."""
    rng, img = _rng("two_px", E, seed), np.zeros((E, A), np.float32)
    for i, r in enumerate(range(E) if rows is None else [r for r in rows if r < E]):
        if i % 2 == 0:
            w = (0, 2, 5)[(i // 2) % 3]
            lo, hi = 64 * w, min(64 * w + 64, A)
            cols = rng.choice(np.arange(lo, hi), size=2, replace=False)
        else:
            cols = np.array([rng.integers(0, 30), rng.integers(330, A)])
        img[r, cols] = _vals(rng, 2)
    return img


def ties(E, seed=0):
    """Holes at equal distance from two valid pixels.  Row kinds in turn: valid at 10 and 350 (the hole at 0 is 10 away
    from both across the wrap, the hole at 180 is 170 away from both; nearest takes the smaller column); valid at 100
    and 104 (hole 102); every even column valid (every odd hole ties, 359 between 358 and 0)."""
    rng, img = _rng("ties", E, seed), np.zeros((E, A), np.float32)
    for r in range(E):
        k = r % 3
        cols = np.array([10, 350]) if k == 0 else np.array([100, 104]) if k == 1 else np.arange(0, A, 2)
        img[r, cols] = _vals(rng, len(cols))
    return img


def density(E, seed=0, p=0.5):
    rng = _rng("density", E, seed + int(p * 1000))
    img = _vals(rng, (E, A))
    img[rng.random((E, A)) >= p] = 0.0
    return img


# ------------------------------------------------------------------------------------------------------------------
# row families: what the empty-row fill (rowsrc) does
# ------------------------------------------------------------------------------------------------------------------
def _rows(name, E, seed, valid_rows):
    rng, img = _rng(name, E, seed), np.zeros((E, A), np.float32)
    for r in valid_rows:
        img[r] = _busy_row(rng)
    return img


def rows_top_empty(E, seed=0):
    return _rows("rows_top_empty", E, seed, range(min((E + 2) // 3, E - 1), E))


def rows_bottom_empty(E, seed=0):
    return _rows("rows_bottom_empty", E, seed, range(0, max(E - (E + 2) // 3, 1)))


def rows_alternate(E, seed=0):
    return _rows("rows_alternate", E, seed, range(0, E, 2))


def rows_one_valid(E, seed=0, k=0):
    return _rows("rows_one_valid", E, seed + k, [k])


TIE_ROWS = (0, 2, 6, 12, 20, 30, 42, 56)     # gaps 2, 4, 6, ...: the middle row of each gap ties at k = 1, 2, 3, ...


def rows_tie(E, seed=0):
    """Rows r-k and r+k valid, r empty, nothing valid in between, for k = 1, 2, 3, ...; the rows under the last valid
    row are a run of empty rows at the bottom."""
    return _rows("rows_tie", E, seed, [r for r in TIE_ROWS if r < E])


def all_empty(E, seed=0):
    return np.zeros((E, A), np.float32)


def all_valid(E, seed=0):
    return _vals(_rng("all_valid", E, seed), (E, A))


# ------------------------------------------------------------------------------------------------------------------
# spectrum families: what the FFT and the histogram do
# ------------------------------------------------------------------------------------------------------------------
N_TONE_IMAGES = 12                           # 12 images x 16 rows = 192 rows: every frequency 0..180 at E = 16


def tone_freqs(E, i):
    return [(i * E + r) % F for r in range(E)]


def tones(E, seed=0, i=0):
    """Row r holds 10 + 5 cos(2 pi k_r n / 360), k_r = (i E + r) mod 181."""
    n = np.arange(A, dtype=np.float64)
    k = np.array(tone_freqs(E, i), dtype=np.float64)[:, None]
    return (10.0 + 5.0 * np.cos(2.0 * np.pi * k * n / A)).astype(np.float32)


def delta(E, seed=0):
    """One pixel per row, each row at another column (not the word edges of single_px)."""
    rng, img = _rng("delta", E, seed), np.zeros((E, A), np.float32)
    for r in range(E):
        img[r, (37 * r + 11) % A] = _vals(rng, ())
    return img


def constant(E, seed=0):
    return np.full((E, A), 25.0, np.float32)


def family_batch(E):
    """Every family at E rows, in one list of (name, image): the images of one launch, so that neighbouring workgroups
    take different branches."""
    out = [("single_px", single_px(E)), ("one_hole", one_hole(E)), ("word5_only", word5_only(E)),
           ("word0_only", word0_only(E)), ("two_px", two_px(E)), ("ties", ties(E))]
    out += [("density_%g" % p, density(E, p=p)) for p in (0.01, 0.05, 0.5, 0.95)]
    out += [("rows_top_empty", rows_top_empty(E)), ("rows_bottom_empty", rows_bottom_empty(E)),
            ("rows_alternate", rows_alternate(E))]
    out += [("rows_one_valid_%d" % k, rows_one_valid(E, k=k)) for k in sorted({0, E // 2, E - 1})]
    out += [("rows_tie", rows_tie(E)), ("all_empty", all_empty(E)), ("all_valid", all_valid(E))]
    out += [("tones_%d" % i, tones(E, i=i)) for i in range(N_TONE_IMAGES)]
    out += [("delta", delta(E)), ("constant", constant(E))]
    assert len(out) <= 64
    for name, img in out:
        assert img.shape == (E, A) and img.dtype == np.float32, name
        v = img[img != 0]
        assert np.all((v >= 2.0) & (v <= 70.0)), name
    return out


MASK_FAMILIES = ("single_px", "one_hole", "word5_only", "word0_only", "two_px", "ties", "density_0.01", "density_0.05",
                 "density_0.5", "density_0.95", "all_empty", "all_valid")
ROW_FAMILIES = ("rows_top_empty", "rows_bottom_empty", "rows_alternate", "rows_one_valid_", "rows_tie")


def interp_batch(E):
    """The images of a mode-2 launch: every mask and row family, plus three of them with each other way of writing a
    hole.  -1.0, -0.0 and NaN all fail ``> 0`` exactly like 0, and both sides overwrite them."""
    out = [(n, im) for n, im in family_batch(E) if n in MASK_FAMILIES or n.startswith(ROW_FAMILIES)]
    for hname, h in HOLES.items():
        for n, im in (("density_0.5", density(E, p=0.5)), ("rows_tie", rows_tie(E)), ("single_px", single_px(E)),
                      ("all_empty", all_empty(E))):
            x = im.copy()
            x[im == 0] = h
            out.append(("%s/%s" % (n, hname), x))
    assert len(out) <= 64
    return out


# ------------------------------------------------------------------------------------------------------------------
# images -> points
# ------------------------------------------------------------------------------------------------------------------
def points_for_image(img, params, stride, copies=1, shuffle_seed=0, n_points=None):
    """One point per valid pixel, at the centre of the pixel's azimuth / elevation bin, at the pixel's range.  With
    copies > 1 every pixel gets further points at larger ranges (the minimum must win); ``n_points`` asks for exactly
    that many points, spread over the valid pixels.  Random intensity (stride 4).  Asserts with the oracle's projection
    that every point lands in the pixel it was made for."""
    E = img.shape[0]
    assert E == params.n_elevation and stride in (3, 4)
    rng = np.random.default_rng([shuffle_seed, E, stride])
    rows, cols = np.nonzero(img > 0)
    if n_points is not None and len(rows):
        copies = -(-n_points // len(rows))
    rows, cols = np.tile(rows, copies), np.tile(cols, copies)
    rng_scale = np.ones(len(rows))
    nbase = len(rows) // max(copies, 1)
    rng_scale[nbase:] = 1.0 + rng.uniform(0.001, 0.1, len(rows) - nbase)       # <= 77 m, inside max_range
    if n_points is not None and len(rows):
        rows, cols, rng_scale = rows[:n_points], cols[:n_points], rng_scale[:n_points]
    r = img[rows, cols].astype(np.float64) * rng_scale
    az = (cols + 0.5) * (2.0 * np.pi / A) - np.pi                              # atan2(y, x) = az: column floor((az+pi)/2pi * 360)
    el = params.elev_min_rad + (rows + 0.5) * (params.elev_max_rad - params.elev_min_rad) / E
    pts = np.zeros((len(rows), stride), np.float32)
    pts[:, 0] = r * np.cos(el) * np.cos(az)
    pts[:, 1] = r * np.cos(el) * np.sin(az)
    pts[:, 2] = r * np.sin(el)
    if stride == 4:
        pts[:, 3] = rng.random(len(rows))
    perm = rng.permutation(len(rows))
    pts, want = pts[perm], (rows * A + cols)[perm].astype(np.int32)
    raw, idx, kept = orc.project(pts, params, want_idx=True)
    assert kept == len(pts) and np.array_equal(idx, want), "a constructed point missed its pixel"
    assert np.array_equal(raw > 0, img > 0)
    return pts


def pack(clouds):
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(clouds, 0)), off


def shuffled(pts, off, seed=1):
    rng, out = np.random.default_rng(seed), pts.copy()
    for c in range(len(off) - 1):
        out[off[c]:off[c + 1]] = pts[off[c]:off[c + 1]][rng.permutation(int(off[c + 1] - off[c]))]
    return out


def sqr_bits(img):
    """What nsc_scatter_clouds leaves for nsc_finish_images: float32 bits of the squared range, 0xffffffff = empty.  The
    correctly rounded float32 square root of float32(v * v) is v again, so the raw image is known exactly."""
    sq = (img * img).astype(np.float32)
    assert np.array_equal(np.sqrt(sq), img)
    return np.where(img > 0, sq.view(np.uint32), np.uint32(0xffffffff)).astype(np.uint32)


# ------------------------------------------------------------------------------------------------------------------
# reference: the oracle, stage by stage
# ------------------------------------------------------------------------------------------------------------------
def params_of(case, rows=None):
    return orc.default_params(n_elevation=case.E if rows is None else rows, n_bins=case.B, target_rows=case.R,
                              interpolate=case.interp, elev_f64=case.elev_f64, elevation_range=ELEV_RANGE)


@functools.lru_cache(maxsize=None)
def lut_of(alpha, B):
    return orc.bin_lut(alpha, B, F, 1e-8)[1]


def nearest_rows(img):
    """orc.interpolate_nearest with the per-pixel loop vectorised (pinned against it, and against the literal loop, in
    tests/test_encoder_families_cpu.py): first minimum of the circular distance over the ascending valid columns."""
    out = np.array(img, dtype=np.float32, copy=True)
    E = out.shape[0]
    cols = np.arange(A)
    for r in range(E):
        valid = np.where(out[r] > 0)[0]
        if len(valid) == 0 or len(valid) == A:
            continue
        d = np.abs(cols[:, None] - valid[None, :])
        pick = valid[np.argmin(np.minimum(d, A - d), axis=1)]
        hole = ~(out[r] > 0)
        out[r, hole] = out[r, pick[hole]]
    nonempty = [bool(np.any(out[r] > 0)) for r in range(E)]
    for r in range(E):
        if not nonempty[r]:
            for k in range(1, E):
                if r - k >= 0 and nonempty[r - k]:
                    out[r], nonempty[r] = out[r - k], True
                    break
                if r + k < E and nonempty[r + k]:
                    out[r], nonempty[r] = out[r + k], True
                    break
    return out


def interpolated(raw, interp):
    return raw.copy() if interp == 0 else orc.interpolate(raw) if interp == 1 else nearest_rows(raw)


def reference(raws, case):
    """(interpolated images, descriptors) of the oracle for raw images (n, rows, 360) under the case's parameters.
    For clouds this is orc.encode_points stage by stage (project -> interpolate -> encode_range_image), with the
    nearest method of range_image.py:66-75 where the case asks for it."""
    rows = raws.shape[1]
    p, lut = params_of(case, rows), lut_of(case.alpha, case.B)
    itp = np.stack([interpolated(x, case.interp) for x in raws])
    desc = np.stack([orc.encode_range_image(x, p, lut) for x in itp])
    return itp, desc


def bar(ref):
    """The project's descriptor bar against the oracle."""
    return 1e-6 * np.abs(ref) + 1e-9


# ------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name entry kernel E R B alpha interp stride elev_f64 batch")
# entry : clouds          nsc_encode_clouds on the family batch (one cloud per image)
#         split           nsc_encode_clouds on 1 or 2 clouds of SPLIT_POINTS points
#         finish_images   nsc_finish_images on squared-range bit images built directly
#         range_images    nsc_encode_range_images (mode 1; no interpolation, E = rows of the input)
#         interpolate_ex  nsc_interpolate_range_images_ex (mode 2; interp = method)
# kernel: fast | fused4 | fused8 | fused16 (encode_*_kernel) | finish8_m0 | finish8_m1 | finish8_m2 (finish_kernel<8>)
# batch : family_batch | interp_batch | split_two_px | split_density | split_both

ENC_PATH = {"fast": 1, "fused4": 2, "fused8": 2, "fused16": 2, "finish8_m0": 3}      # NSC_ENC_PATH_*
FAST_HSTRIDE = 64
SPLIT_MIN_PTS, SPLIT_TARGET_WGS = 16384, 512


def split_parts(n_clouds, total_points):
    if n_clouds <= 0 or n_clouds >= SPLIT_TARGET_WGS:
        return 1
    s = min(-(-SPLIT_TARGET_WGS // n_clouds), (total_points // n_clouds) // SPLIT_MIN_PTS)
    return 1 if s < 2 else s


def kernel_for_clouds(E, R, B, stride, n_clouds, total_points):
    """encode_path() and the launcher of nsc_encode_clouds, restated (default field of view and range window)."""
    if split_parts(n_clouds, total_points) > 1:
        return "finish8_m0"
    if stride == 4 and E == 16 and R == 16 and B <= FAST_HSTRIDE:
        return "fast"
    return "fused16" if E > 32 else "fused8" if E > 16 else "fused4"


def _c(entry, kernel, E, R, B=50, alpha=2.0, interp=1, stride=4, elev_f64=1, batch="family_batch"):
    name = "%s-%s-E%dR%dB%d-a%g-i%d-s%d%s%s" % (entry, kernel, E, R, B, alpha, interp, stride, "" if elev_f64 else "-f32rows",
                                                "" if batch in ("family_batch", "interp_batch") else "-" + batch)
    return Case(name, entry, kernel, E, R, B, float(alpha), interp, stride, elev_f64, batch)


@functools.lru_cache(maxsize=None)
def cases():
    t = []
    # nsc_encode_clouds -> encode_fast_kernel: every B x interpolate, the three alphas in turn (each meets every B)
    for ib, B in enumerate((1, 2, 50, 63, 64)):
        for interp in (0, 1, 2):
            t.append(_c("clouds", "fast", 16, 16, B, (0.25, 2.0, 6.0)[(ib + interp) % 3], interp))
    for alpha in (2.0, 6.0):                                    # ... and B = 50, linear, with the two alphas its turn left out
        t.append(_c("clouds", "fast", 16, 16, 50, alpha, 1))
    # -> encode_fused_kernel<4, 4, 4>
    t += [_c("clouds", "fused4", 16, 16, stride=3, interp=1), _c("clouds", "fused4", 16, 16, stride=3, interp=2),
          _c("clouds", "fused4", 16, 1, interp=1), _c("clouds", "fused4", 16, 5, interp=0),
          _c("clouds", "fused4", 16, 8, interp=2),
          _c("clouds", "fused4", 16, 16, B=65, interp=0), _c("clouds", "fused4", 16, 16, B=176, interp=2),
          _c("clouds", "fused4", 16, 16, B=176, alpha=6.0, interp=1),
          _c("clouds", "fused4", 16, 16, elev_f64=0, stride=3),
          _c("clouds", "fused4", 1, 1, interp=1), _c("clouds", "fused4", 5, 5, interp=2),
          _c("clouds", "fused4", 15, 15, interp=0), _c("clouds", "fused4", 15, 15, interp=1),
          _c("clouds", "fused4", 8, 16, interp=1), _c("clouds", "fused4", 8, 16, interp=0),
          _c("clouds", "fused4", 5, 16, interp=2)]
    # -> encode_fused_kernel<8, 4, 2>
    t += [_c("clouds", "fused8", 17, 16, interp=1), _c("clouds", "fused8", 24, 16, interp=0),
          _c("clouds", "fused8", 24, 16, interp=1), _c("clouds", "fused8", 32, 16, interp=2),
          _c("clouds", "fused8", 24, 5, interp=1)]
    # -> encode_fused_kernel<16, 4, 1>
    t += [_c("clouds", "fused16", 33, 16, interp=1), _c("clouds", "fused16", 40, 16, interp=0),
          _c("clouds", "fused16", 40, 16, interp=2), _c("clouds", "fused16", 64, 16, interp=1),
          _c("clouds", "fused16", 64, 16, interp=2), _c("clouds", "fused16", 64, 1, interp=1)]
    # -> split path: scatter_split_kernel + global atomicMin + finish_kernel<8> mode 0
    t += [_c("split", "finish8_m0", 16, 16, batch="split_two_px"), _c("split", "finish8_m0", 16, 16, batch="split_density"),
          _c("split", "finish8_m0", 16, 16, batch="split_both"), _c("split", "finish8_m0", 16, 16, interp=2, batch="split_both"),
          _c("split", "finish8_m0", 16, 16, interp=0, batch="split_both")]
    # nsc_finish_images -> finish_kernel<8> mode 0
    for E in (1, 16, 17, 33, 64):
        for interp in (0, 1, 2):
            t.append(_c("finish_images", "finish8_m0", E, min(E, 16), interp=interp))
    t.append(_c("finish_images", "finish8_m0", 1, 16, interp=1))
    # nsc_encode_range_images -> finish_kernel<8> mode 1 (no interpolation: interp is not read)
    for rows in (1, 8, 15, 16, 17, 24, 40, 64):
        t.append(_c("range_images", "finish8_m1", rows, 16, interp=0))
    # nsc_interpolate_range_images_ex -> finish_kernel<8> mode 2
    for rows in (1, 5, 16, 17, 33, 64):
        for method in (1, 2):
            t.append(_c("interpolate_ex", "finish8_m2", rows, min(rows, 16), interp=method, batch="interp_batch"))
    assert len({c.name for c in t}) == len(t)
    return tuple(t)


@functools.lru_cache(maxsize=None)
def images_of(case):
    """[(family name, image)] of the case's launch."""
    if case.batch == "family_batch":
        return tuple(family_batch(case.E))
    if case.batch == "interp_batch":
        return tuple(interp_batch(case.E))
    few = ("two_px/8px", two_px(case.E, rows=(0, 5, 10, 15)))                  # 4 rows x 2 pixels
    dens = ("density_0.05", density(case.E, p=0.05))
    return {"split_two_px": (few,), "split_density": (dens,), "split_both": (few, dens)}[case.batch]


@functools.lru_cache(maxsize=None)
def _clouds(E, stride, batch):
    p = orc.default_params(n_elevation=E, elevation_range=ELEV_RANGE)
    if batch == "family_batch":
        return tuple(points_for_image(im, p, stride, shuffle_seed=i) for i, (_, im) in enumerate(family_batch(E)))
    case = _c("split", "finish8_m0", E, E, stride=stride, batch=batch)
    return tuple(points_for_image(im, p, stride, shuffle_seed=i, n_points=SPLIT_POINTS)
                 for i, (_, im) in enumerate(images_of(case)))


def clouds_of(case):
    """(points, offsets) of a clouds / split case; the constructed points do not depend on R, B, alpha or interpolate."""
    assert case.entry in ("clouds", "split")
    return pack(_clouds(case.E, case.stride, case.batch))


def raw_images_of_clouds(case):
    """The oracle's projection of the case's clouds (also checks the float32 row math when the case asks for it)."""
    pts, off = clouds_of(case)
    p = params_of(case)
    return np.stack([orc.project(pts[off[c]:off[c + 1]], p) for c in range(len(off) - 1)])


def fill_taken(img):
    ne = np.any(img > 0, axis=1)
    return bool(ne.any() and not ne.all())


def coverage_of(case):
    """The (kernel, interp method, pooled, row fill taken) combinations the case's launch reaches."""
    imgs = [im for _, im in images_of(case)]
    if case.kernel == "finish8_m1":                              # no interpolation stage at all
        return {(case.kernel, None, case.E != case.R, False)}
    pooled = None if case.kernel == "finish8_m2" else case.E != case.R
    if case.interp == 0:
        return {(case.kernel, 0, pooled, False)}
    return {(case.kernel, case.interp, pooled, fill_taken(im)) for im in imgs}


def required_coverage():
    req = set()
    pooled_of = {"fast": (False,), "fused4": (False, True), "fused8": (True,), "fused16": (True,),     # E > 16 >= R
                 "finish8_m0": (False, True)}
    for k, pooled in pooled_of.items():
        for pl in pooled:
            req.add((k, 0, pl, False))
            req |= {(k, m, pl, f) for m in (1, 2) for f in (False, True)}
    req |= {("finish8_m1", None, pl, False) for pl in (False, True)}
    req |= {("finish8_m2", m, None, f) for m in (1, 2) for f in (False, True)}
    return req


def coverage_gaps():
    have = set()
    for c in cases():
        have |= coverage_of(c)
    return sorted(required_coverage() - have, key=str)
