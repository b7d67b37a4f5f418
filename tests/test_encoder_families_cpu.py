"""The encoder image families (tests/encoder_families.py) without a GPU.

Pins the parts of the oracle that no golden file pins (row pooling against torch, both interpolation methods against a
literal numpy restatement of the reference's loop, the product's bin LUT against the oracle's), admits the descriptor bar
with an independent algorithm (np.fft.rfft in float64) on every case of the table, checks that every family has the
property it is named for, and that every case reaches the kernel it is named after (nsc_encode_clouds_path is a host
function) with no (kernel x interpolation method x pooled x row fill) combination left out.
"""
import os

import numpy as np
import pytest
import torch

import encoder_families as EF
import nsc_oracle as orc
from encoder_families import A, F

CASES = EF.cases()
IDS = [c.name for c in CASES]
ER = sorted({(c.E, c.R) for c in CASES if c.kernel != "finish8_m2"})
ALPHA_B = sorted({(c.alpha, c.B) for c in CASES})
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "neural-spectral-codec_amd", "csrc",
                   "nsc_encoder.hip")
ROWS = (1, 2, 3, 5, 8, 15, 16, 17, 24, 33, 40, 64)


def u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------------
# literal restatement of the reference's interpolate_range_image (src/encoding/range_image.py:33-64 and :66-75 per row,
# :77-87 for empty rows), numpy calls as the reference makes them
# ----------------------------------------------------------------------------------------------------------------------
def literal_interpolate(range_image, method):
    interpolated = np.array(range_image, dtype=np.float32, copy=True)
    n_elevation, n_azimuth = interpolated.shape
    for row in range(n_elevation):                                                        # :33
        row_data = interpolated[row].copy()
        valid_mask = row_data > 0                                                         # :35
        if not np.any(valid_mask):                                                        # :37-38
            continue
        if np.all(valid_mask):                                                            # :41-43
            continue
        valid_indices = np.where(valid_mask)[0]                                           # :46
        valid_values = row_data[valid_indices]
        invalid_indices = np.where(~valid_mask)[0]
        if method == "linear":                                                            # :52-64
            xp = np.concatenate([valid_indices - n_azimuth, valid_indices, valid_indices + n_azimuth])
            fp = np.tile(valid_values, 3)
            interpolated[row, invalid_indices] = np.interp(invalid_indices, xp, fp)
        else:                                                                             # :66-75
            for idx in invalid_indices:
                distances = np.abs(valid_indices - idx)
                distances = np.minimum(distances, n_azimuth - distances)
                interpolated[row, idx] = row_data[valid_indices[np.argmin(distances)]]
    for row in range(n_elevation):                                                        # :77-87, in place
        if not np.any(interpolated[row] > 0):
            for offset in range(1, n_elevation):
                if row - offset >= 0 and np.any(interpolated[row - offset] > 0):
                    interpolated[row] = interpolated[row - offset]
                    break
                if row + offset < n_elevation and np.any(interpolated[row + offset] > 0):
                    interpolated[row] = interpolated[row + offset]
                    break
    return interpolated


# ----------------------------------------------------------------------------------------------------------------------
# pins
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,R", ER, ids=["%dto%d" % er for er in ER])
def test_adaptive_rows_is_adaptive_avg_pool2d(E, R):
    rng = np.random.default_rng([E, R])
    for img in (rng.uniform(0, 80, (E, A)).astype(np.float32), EF.density(E, p=0.5), EF.tones(E, i=3)):
        out = np.empty((R, A), np.float32)
        orc.lib().nsc_oracle_adaptive_rows(orc._f(img), E, A, R, orc._f(out))
        want = torch.nn.functional.adaptive_avg_pool2d(torch.from_numpy(img)[None, None], (R, A))[0, 0].numpy()
        assert np.array_equal(u32(out), u32(want))


@pytest.mark.parametrize("E", ROWS)
def test_oracle_linear_interpolation_is_the_reference_loop(E):
    for name, img in EF.family_batch(E) + EF.interp_batch(E):
        assert np.array_equal(u32(orc.interpolate(img)), u32(literal_interpolate(img, "linear"))), name


@pytest.mark.parametrize("E", ROWS)
def test_oracle_nearest_interpolation_is_the_reference_loop(E):
    for name, img in EF.interp_batch(E):
        want = u32(literal_interpolate(img, "nearest"))
        assert np.array_equal(u32(EF.nearest_rows(img)), want), name               # the vectorised form the GPU tests use
        if name == "ties" or name.startswith(EF.ROW_FAMILIES):
            assert np.array_equal(u32(orc.interpolate_nearest(img)), want), name


@pytest.mark.parametrize("alpha,B", ALPHA_B, ids=["a%g-B%d" % ab for ab in ALPHA_B])
def test_product_bin_lut_is_the_oracle_lut(alpha, B):
    from neural_spectral_codec_amd.encoding.spectral_encoder import compute_bin_lut
    lut = compute_bin_lut(alpha, B, F, 1e-8).numpy()
    assert lut.dtype == np.int32 and np.array_equal(lut, EF.lut_of(alpha, B))
    assert lut.min() >= 0 and lut.max() <= B - 1 and np.all(np.diff(lut) >= 0)


def test_stage_by_stage_reference_is_the_oracle_encoder():
    """EF.reference() on the projected images == orc.encode_clouds on the points, bit for bit (linear and off)."""
    for case in (c for c in CASES if c.name in ("clouds-fused4-E16R5B50-a2-i0-s4", "clouds-fused8-E24R16B50-a2-i1-s4")):
        pts, off = EF.clouds_of(case)
        od, oraw, oitp = orc.encode_clouds(pts, off, EF.params_of(case), EF.lut_of(case.alpha, case.B), n_threads=4,
                                           want_images=True)
        raw = EF.raw_images_of_clouds(case)
        itp, desc = EF.reference(raw, case)
        assert np.array_equal(u32(raw), u32(oraw)) and np.array_equal(u32(itp), u32(oitp))
        assert np.array_equal(u32(desc), u32(od))


# ----------------------------------------------------------------------------------------------------------------------
# admission of the descriptor bar: an independent algorithm meets it on every case
# ----------------------------------------------------------------------------------------------------------------------
def rfft_descriptor(itp, case):
    """The descriptor from an interpolated image with np.fft.rfft (float64, pocketfft -- not the oracle's direct sum):
    pooling in float32 as adaptive_avg_pool2d, magnitudes rounded to float32, bins summed in float32 in ascending k,
    one global L1 normalisation."""
    R, B, lut = case.R, case.B, EF.lut_of(case.alpha, case.B)
    x = itp
    if x.shape[0] != R:
        x = torch.nn.functional.adaptive_avg_pool2d(torch.from_numpy(itp)[None, None], (R, A))[0, 0].numpy()
    mags = np.abs(np.fft.rfft(x.astype(np.float64), axis=1)).astype(np.float32)
    desc = np.zeros((R, B), np.float32)
    for k in range(F):
        desc[:, lut[k]] += mags[:, k]
    s = np.float32(desc.astype(np.float64).sum())
    eps = np.float32(1e-8)
    return (desc / (s + eps) if s > eps else np.full((R, B), np.float32(1) / np.float32(R * B))).reshape(-1)


_RAW = {}


def raw_images(case):
    """The raw images of a case as the device will see them (projected for clouds, as built otherwise)."""
    key = (case.entry, case.E, case.stride, case.elev_f64, case.batch)
    if key not in _RAW:
        _RAW[key] = (EF.raw_images_of_clouds(case) if case.entry in ("clouds", "split")
                     else np.stack([im for _, im in EF.images_of(case)]))
    return _RAW[key]


@pytest.mark.parametrize("case", [c for c in CASES if c.kernel != "finish8_m2"],
                         ids=[c.name for c in CASES if c.kernel != "finish8_m2"])
def test_descriptor_bar_is_attainable(case):
    itp, desc = EF.reference(raw_images(case), case)
    worst = 0.0
    for i, (name, _) in enumerate(EF.images_of(case)):
        mine = rfft_descriptor(itp[i], case)
        err = np.abs(mine - desc[i]) / EF.bar(desc[i])
        worst = max(worst, float(err.max()))
        assert np.all(err <= 1.0), (name, float(err.max()))
        if name == "all_empty":
            assert np.array_equal(desc[i], np.full(case.R * case.B, np.float32(1) / np.float32(case.R * case.B)))
    print("%s: rfft restatement vs oracle, worst |d| / bar = %.3f" % (case.name, worst))


def test_a_frequency_in_the_wrong_bin_breaks_the_bar():
    """What the tones are for: move ONE frequency into the neighbouring bin (the first frequency of a bin, the kind of
    off-by-one a segment table makes) and the descriptor of the tone image that holds it misses the bar by orders of
    magnitude, while a dense random image moves by far less."""
    case = next(c for c in CASES if c.name == "range_images-finish8_m1-E16R16B50-a2-i0-s4")
    lut = EF.lut_of(case.alpha, case.B)
    firsts = [k for k in range(1, F) if lut[k] != lut[k - 1]]
    assert len(firsts) == len(np.unique(lut)) - 1
    for k in firsts[::7] + [180]:
        wrong = lut.copy()
        wrong[k] = lut[k] - 1
        i, r = next((i, EF.tone_freqs(16, i).index(k)) for i in range(EF.N_TONE_IMAGES) if k in EF.tone_freqs(16, i))
        img = EF.tones(16, i=i)
        ref = orc.encode_range_image(img, EF.params_of(case), lut)
        bad = orc.encode_range_image(img, EF.params_of(case), wrong)
        ratio = np.abs(bad - ref) / EF.bar(ref)
        assert ratio.max() > 1e4, (k, ratio.max())
        d = bad.reshape(16, 50)[r].copy()
        d[lut[0]] = -1.0
        assert int(np.argmax(d)) != lut[k] or lut[k] - 1 == lut[0]                            # ... and the argmax check sees it too


# ----------------------------------------------------------------------------------------------------------------------
# non-vacuity: each family has the property it is named for
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", ROWS)
def test_mask_families_have_their_property(E):
    fam = dict(EF.family_batch(E))
    v = {n: im > 0 for n, im in fam.items()}
    assert np.all(v["single_px"].sum(1) == 1) and np.all(v["one_hole"].sum(1) == A - 1)
    for r in range(E):
        assert v["single_px"][r, EF.EDGE_COLS[r % 6]] and not v["one_hole"][r, EF.EDGE_COLS[r % 6]]
    assert v["word5_only"][:, 320:].any(1).all() and not v["word5_only"][:, :320].any()
    assert v["word0_only"][:, :64].any(1).all() and not v["word0_only"][:, 64:].any()
    assert np.all(v["two_px"].sum(1) == 2)
    for r in range(E):
        a, b = np.where(v["two_px"][r])[0]
        assert (a // 64 == b // 64) if r % 2 == 0 else (a // 64 == 0 and b // 64 == 5 and a + A - b < b - a)   # 359 -> 0 is the short way
    for r in range(E):                                           # ties: a hole with two nearest valid pixels
        cols = np.where(v["ties"][r])[0]
        d = np.abs(np.arange(A)[:, None] - cols[None, :])
        d = np.minimum(d, A - d)
        srt = np.sort(d, axis=1)
        assert np.any((srt[:, 0] > 0) & (srt[:, 0] == srt[:, 1]))
    t0 = v["ties"][0]
    assert t0[10] and t0[350] and t0.sum() == 2                  # the wrapped tie: hole 0 between 350 and 10
    lin, near = orc.interpolate(fam["ties"]), EF.nearest_rows(fam["ties"])
    assert near[0, 0] == fam["ties"][0, 10] and near[0, 180] == fam["ties"][0, 10]          # the smaller column wins
    assert lin[0, 0] == np.float32((np.float64(fam["ties"][0, 10]) + np.float64(fam["ties"][0, 350])) / 2)
    for p in (0.01, 0.05, 0.5, 0.95):
        frac = v["density_%g" % p].mean()
        assert abs(frac - p) <= 4 * np.sqrt(p * (1 - p) / (E * A)) + 1e-12, (p, frac)      # 4 sigma of a binomial
    assert not v["all_empty"].any() and v["all_valid"].all() and v["constant"].all()
    assert np.all(v["delta"].sum(1) == 1) and len({int(np.argmax(r)) for r in v["delta"]}) == min(E, A)
    assert not any(int(np.argmax(r)) in EF.EDGE_COLS for r in v["delta"][:8])


@pytest.mark.parametrize("E", ROWS)
def test_row_families_have_their_property(E):
    fam = dict(EF.family_batch(E))
    ne = {n: (im > 0).any(1) for n, im in fam.items()}
    for k in sorted({0, E // 2, E - 1}):
        assert np.array_equal(np.where(ne["rows_one_valid_%d" % k])[0], [k])
    if E >= 2:
        top, bot = ne["rows_top_empty"], ne["rows_bottom_empty"]
        assert not top[0] and top[-1] and np.all(np.diff(top.astype(int)) >= 0)            # one run of empty rows on top
        assert bot[0] and not bot[-1] and np.all(np.diff(bot.astype(int)) <= 0)
        assert np.array_equal(ne["rows_alternate"], np.arange(E) % 2 == 0)
    ks = set()
    tie = ne["rows_tie"]
    for r in range(E):
        if not tie[r]:
            for k in range(1, E):
                up, down = r - k >= 0 and tie[r - k], r + k < E and tie[r + k]
                if up or down:
                    if up and down:
                        ks.add(k)
                    break
    assert ks == {k for k in range(1, 8) if EF.TIE_ROWS[k] < E}, ks                          # rows r-k and r+k valid, for every k that fits
    if E >= 3:
        r = 1                                                                                 # the row above wins the tie
        assert np.array_equal(orc.interpolate(fam["rows_tie"])[r], orc.interpolate(fam["rows_tie"])[0])
        assert not np.array_equal(orc.interpolate(fam["rows_tie"])[0], orc.interpolate(fam["rows_tie"])[2])
    if E > max(t for t in EF.TIE_ROWS if t < E) + 1:
        assert not tie[-1]                                                                    # and a run of empty rows at the bottom


def test_tones_cover_every_frequency_and_luts_have_empty_bins():
    ks = {k for i in range(EF.N_TONE_IMAGES) for k in EF.tone_freqs(16, i)}
    assert ks == set(range(F))
    img = EF.tones(16, i=2)
    mags = np.abs(np.fft.rfft(img.astype(np.float64), axis=1))
    for r, k in enumerate(EF.tone_freqs(16, 2)):
        rest = np.delete(mags[r], [0, k])
        assert mags[r, 0] > 3000 and mags[r, k] > 800 and rest.max() < 1e-2, (r, k)          # DC 3600, tone 900 (1800 at 180)
    empty = [(a, B) for a, B in ALPHA_B if len(np.unique(EF.lut_of(a, B))) < B]
    assert len(empty) >= 2 and (2.0, 176) in empty, empty
    assert {B for _, B in ALPHA_B} >= {1, 2, 50, 63, 64, 65, 176}


def test_constructed_points_reproduce_the_images():
    """points_for_image asserts pixel by pixel; here: the minimum of the copies is the pixel, the split clouds hold exactly
    the smallest size that splits, and the few-pixel cloud puts all of them into 8 pixels."""
    p = orc.default_params(n_elevation=16, elevation_range=EF.ELEV_RANGE)
    img = EF.density(16, p=0.05)
    one = orc.project(EF.points_for_image(img, p, 4), p)
    many_pts = EF.points_for_image(img, p, 4, copies=7, shuffle_seed=3)
    assert len(many_pts) == 7 * int((img > 0).sum())
    assert np.array_equal(u32(orc.project(many_pts, p)), u32(one))
    assert np.max(np.abs(one - img)) <= 1e-5 * 70
    for c in (c for c in CASES if c.entry == "split"):
        pts, off = EF.clouds_of(c)
        assert np.all(np.diff(off) == EF.SPLIT_POINTS)
        raw = EF.raw_images_of_clouds(c)
        if c.batch != "split_density":
            assert int((raw[0] > 0).sum()) == 8
    for c in (c for c in CASES if c.entry == "clouds" and not c.elev_f64):
        assert np.array_equal(EF.raw_images_of_clouds(c) > 0, np.stack([im for _, im in EF.images_of(c)]) > 0)


def test_sqr_bits_round_trip():
    for name, img in EF.family_batch(17):
        bits = EF.sqr_bits(img)
        back = np.where(bits == 0xffffffff, np.float32(0), np.sqrt(np.where(bits == 0xffffffff, 0, bits).astype(np.uint32).view(np.float32)))
        assert np.array_equal(u32(back), u32(img)), name


# ----------------------------------------------------------------------------------------------------------------------
# dispatch
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from neural_spectral_codec_amd import build, _lib
    build.build_hip()
    return _lib.lib()


def enc_params(case):
    from neural_spectral_codec_amd import _lib
    o, p = EF.params_of(case), _lib.EncParams()
    for f, _ in _lib.EncParams._fields_:
        setattr(p, f, getattr(o, f))
    return p


def test_every_case_reaches_the_kernel_it_is_named_after(lib):
    hip = open(HIP).read()
    for text in ("constexpr int FAST_HSTRIDE = 64;", "constexpr int SPLIT_MIN_PTS = 16384;", "constexpr int SPLIT_TARGET_WGS = 512;",
                 "if (d.E > 32)", "else if (d.E > 16)", "launch_fused<16, 4, 1>", "launch_fused<8, 4, 2>", "launch_fused<4, 4, 4>",
                 "launch_finish<FUSED_NW>", "constexpr int FUSED_NW = 8;", "constexpr int MAXB = (ROW_BYTES - HIST_OFF) / 4;"):
        assert text in hip, text                                  # what kernel_for_clouds() restates
    for c in CASES:
        if c.entry in ("clouds", "split"):
            pts, off = EF.clouds_of(c)
            n, total = len(off) - 1, len(pts)
            assert n <= 64
            assert EF.kernel_for_clouds(c.E, c.R, c.B, c.stride, n, total) == c.kernel, c.name
            assert lib.nsc_encode_clouds_path(n, total, c.stride, enc_params(c)) == EF.ENC_PATH[c.kernel], c.name
            assert (lib.nsc_encode_clouds_workspace_bytes(n, total, enc_params(c)) > 0) == (c.entry == "split"), c.name
        else:
            assert c.kernel == {"finish_images": "finish8_m0", "range_images": "finish8_m1", "interpolate_ex": "finish8_m2"}[c.entry]
            assert len(EF.images_of(c)) <= 64
        assert 1 <= c.E <= 64 and 1 <= c.R <= 16 and 1 <= c.B <= 176                        # inside what check_params accepts
    # the smallest size that splits really is the smallest: one point fewer per cloud does not split
    p = enc_params(next(c for c in CASES if c.entry == "split"))
    assert lib.nsc_encode_clouds_path(1, EF.SPLIT_POINTS - 1, 4, p) == 1 and lib.nsc_encode_clouds_path(2, 2 * EF.SPLIT_POINTS - 2, 4, p) == 1
    # B = 64 is the last fast shape, 65 the first fused one
    assert {c.B for c in CASES if c.kernel == "fast"} >= {64} and {c.B for c in CASES if c.kernel == "fused4" and c.E == 16 and c.R == 16} >= {65}


def test_shapes_outside_the_documented_limits_are_refused(lib):
    """include/nsc.h: n_azimuth 360, rows 1..64, target_rows 1..16, n_bins 1..176 -- one step outside each is
    NSC_EUNSUPPORTED (-2) before anything is launched, the last shape inside is accepted."""
    base = next(c for c in CASES if c.kernel == "fused4" and c.B == 176)
    for field, inside, outside in (("n_bins", 176, 177), ("n_bins", 1, 0), ("target_rows", 16, 17), ("target_rows", 1, 0),
                                   ("n_elevation", 64, 65), ("n_elevation", 1, 0), ("n_azimuth", 360, 359)):
        p = enc_params(base)
        setattr(p, field, inside)
        assert lib.nsc_encode_clouds_path(4, 4000, 4, p) > 0, (field, inside)
        setattr(p, field, outside)
        assert lib.nsc_encode_clouds_path(4, 4000, 4, p) == -2, (field, outside)
        assert lib.nsc_encode_clouds_workspace_bytes(4, 4 * 40000, p) == 0
        for fn, args in ((lib.nsc_finish_images, (None, 1, p, None, None, None, None, None)),
                         (lib.nsc_encode_range_images, (None, 1, 16, p, None, None, None))):
            assert fn(*args) == -2, (fn.__name__, field, outside)
    p = enc_params(base)
    for rows in (0, 65):
        assert lib.nsc_encode_range_images(None, 1, rows, p, None, None, None) == -2
        assert lib.nsc_interpolate_range_images_ex(None, 1, rows, None, 1, None, None) == -2


def test_the_table_covers_what_the_issue_lists():
    def have(**kw):
        return [c for c in CASES if all(getattr(c, k) == v for k, v in kw.items())]
    for B in (1, 2, 50, 63, 64):
        for interp in (0, 1, 2):
            assert have(kernel="fast", B=B, interp=interp)
    for alpha in (0.25, 2.0, 6.0):
        assert have(kernel="fast", alpha=alpha, B=50)
    assert have(kernel="fused4", E=16, stride=3) and have(kernel="fused4", E=16, elev_f64=0)
    for R in (1, 5, 8):
        assert have(kernel="fused4", E=16, R=R)
    for B in (65, 176):
        assert have(kernel="fused4", E=16, R=16, B=B)
    for E in (1, 5, 15):
        assert have(kernel="fused4", E=E, R=E)
    assert have(kernel="fused4", E=8, R=16)
    for E in (17, 24, 32):
        assert have(kernel="fused8", E=E, R=16)
    assert have(kernel="fused8", E=24, R=5)
    for E in (33, 40, 64):
        assert have(kernel="fused16", E=E, R=16)
    assert have(kernel="fused16", E=64, R=1)
    assert {c.batch for c in have(entry="split")} == {"split_two_px", "split_density", "split_both"}
    for E in (1, 16, 17, 33, 64):
        for interp in (0, 1, 2):
            assert have(entry="finish_images", E=E, interp=interp)
    for rows in (1, 8, 15, 16, 17, 24, 40, 64):
        assert have(entry="range_images", E=rows, R=16)
    for rows in (1, 5, 16, 17, 33, 64):
        for m in (1, 2):
            assert have(entry="interpolate_ex", E=rows, interp=m)


def test_no_coverage_gaps():
    assert EF.coverage_gaps() == []
    # and the definition of done: every finishing-stage instantiation meets filled rows, word-5 holes and a 359 -> 0 gap
    for k in ("fast", "fused4", "fused8", "fused16", "finish8_m0", "finish8_m2"):
        cs = [c for c in CASES if c.kernel == k and c.interp in (1, 2) and c.batch in ("family_batch", "interp_batch")]
        assert cs, k
        for c in cs:
            names = [n for n, _ in EF.images_of(c)]
            assert {"word0_only", "word5_only", "two_px", "one_hole"} <= set(names)
            if c.E > 1:
                assert any(EF.fill_taken(im) for _, im in EF.images_of(c))
    # the FFT scratch of finish_image lies in the dead image once E * 1440 >= waves * 2880 and the rows are pooled:
    # both sides of that switch, per instantiation that can pool
    for k, nw in (("fused4", 4), ("finish8_m0", 8), ("finish8_m1", 8)):
        sides = {c.E * 1440 >= nw * 2880 for c in CASES if c.kernel == k and c.E != c.R}
        assert sides == {False, True}, (k, sides)
