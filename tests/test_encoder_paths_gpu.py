"""Every copy of the encoder's image stage on constructed images (tests/encoder_families.py), against the oracle.

One test per case of EF.cases(); a case is one launch over a batch of up to 64 images of different families, so that
neighbouring workgroups take different branches.  The bars are the project's own:
  - raw and interpolated image bit-identical to the oracle (compared as uint32);
  - descriptor |gpu - oracle| <= 1e-6 |oracle| + 1e-9 element-wise (EF.bar; admitted on the CPU by an independent rfft
    restatement in tests/test_encoder_families_cpu.py);
  - an image without a single return gives exactly 1 / (R B) everywhere;
  - interpolate = 0 leaves the interpolated output equal to the raw one;
  - tones: see check_tones();
  - fast and split cases: shuffling the points inside each cloud leaves all three outputs bit-identical.
Each test prints the largest |gpu - oracle| / bar it saw, by kernel.
"""
import numpy as np
import pytest
import torch

import encoder_families as EF
from encoder_families import A
from neural_spectral_codec_amd import _lib
from neural_spectral_codec_amd.encoding import SpectralEncoder
from neural_spectral_codec_amd.encoding.range_image import interpolate_range_image
from neural_spectral_codec_amd.encoding.spectral_encoder import _run_encode_clouds

pytestmark = pytest.mark.gpu

CASES = EF.cases()
_RAW = {}


def by_entry(*entries):
    cs = [c for c in CASES if c.entry in entries]
    return pytest.mark.parametrize("case", cs, ids=[c.name for c in cs])


def u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def encoder(case):
    return SpectralEncoder(n_elevation=case.E, n_azimuth=A, n_bins=case.B, alpha=case.alpha, target_elevation_bins=case.R,
                           interpolate_empty=bool(case.interp), elevation_range=EF.ELEV_RANGE,
                           elev_float64=bool(case.elev_f64)).to("cuda")


def params(enc, case):
    """enc._params(), with the interpolation method where SpectralEncoder cannot express it (2 = nearest)."""
    p = enc._params()
    p.interpolate = case.interp
    return p


def raw_of_clouds(case):
    """The oracle's projection of the case's clouds: computed once per point set, shared, never modified."""
    key = (case.E, case.stride, case.elev_f64, case.batch)
    if key not in _RAW:
        _RAW[key] = EF.raw_images_of_clouds(case)
        _RAW[key].setflags(write=False)
    return _RAW[key]


def run_clouds(enc, case, pts, off):
    """nsc_encode_clouds through SpectralEncoder.encode_points_batch; through the launcher under it with edited
    parameters for the nearest method."""
    tp, to = torch.from_numpy(pts).cuda(), torch.from_numpy(off).cuda()
    n, total = len(off) - 1, len(pts)
    assert _lib.lib().nsc_encode_clouds_path(n, total, case.stride, params(enc, case)) == EF.ENC_PATH[case.kernel]
    if case.interp in (0, 1):
        d, raw, itp = enc.encode_points_batch((tp, to), return_images=True)
    else:
        d, raw, itp = _run_encode_clouds(tp, to, n, total, case.stride, params(enc, case), enc._lut(tp.device),
                                         want_images=True)
    torch.cuda.synchronize()
    return d.cpu().numpy(), raw.cpu().numpy(), itp.cpu().numpy()


def check_tones(case, names, desc, lut):
    """Row r of a tone image holds 10 + 5 cos(2 pi k_r n / 360): |X[0]| = 3600 (5400 for k_r = 0) against |X[k_r]| = 900
    (1800 for k_r = 180) and rounding noise everywhere else.  The DC term dominates every row, so the argmax bin of row r
    is lut[0]; and the largest bin OTHER than lut[0] is lut[k_r], wherever k_r has a bin of its own.  A frequency that
    lands in a neighbouring bin moves a whole tone.  Only where the rows are not pooled (a pooled row mixes tones)."""
    if case.E != case.R:
        return 0
    checked = 0
    for i, name in enumerate(names):
        if not name.startswith("tones_"):
            continue
        d = desc[i].reshape(case.R, case.B)
        for r, k in enumerate(EF.tone_freqs(case.E, int(name[6:]))):
            assert int(np.argmax(d[r])) == lut[0], (name, r, k)
            if lut[k] != lut[0]:
                rest = d[r].copy()
                rest[lut[0]] = -1.0
                assert int(np.argmax(rest)) == lut[k], (name, r, k)
                checked += 1
    return checked


def check(case, raws, gpu_desc, gpu_raw, gpu_itp):
    """All the bars of one launch; returns the largest |gpu - oracle| / bar of the descriptors."""
    names = [n for n, _ in EF.images_of(case)]
    itp, desc = EF.reference(raws, case)
    if gpu_raw is not None:
        for i, n in enumerate(names):
            assert np.array_equal(u32(gpu_raw[i]), u32(raws[i])), "raw image of %s differs from the oracle" % n
    if gpu_itp is not None:
        for i, n in enumerate(names):
            assert np.array_equal(u32(gpu_itp[i]), u32(itp[i])), "interpolated image of %s differs from the oracle" % n
        if case.interp == 0:
            assert np.array_equal(u32(gpu_itp), u32(gpu_raw))
    worst = 0.0
    for i, n in enumerate(names):
        ratio = np.abs(gpu_desc[i] - desc[i]) / EF.bar(desc[i])
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 1.0), "descriptor of %s: |gpu - oracle| / bar = %.3g at %d" % (n, ratio.max(), int(np.argmax(ratio)))
        if not np.any(raws[i] > 0):
            assert np.array_equal(gpu_desc[i], np.full(case.R * case.B, np.float32(1) / np.float32(case.R * case.B))), n
    lut = EF.lut_of(case.alpha, case.B)
    tones = check_tones(case, names, gpu_desc, lut)
    if case.E == case.R and case.batch == "family_batch" and case.B > 1:
        assert tones > 0
    print("%s %s: worst |gpu - oracle| / bar = %.3f" % (case.kernel, case.name, worst))
    return worst


@by_entry("clouds", "split")
def test_encode_clouds(case):
    enc = encoder(case)
    pts, off = EF.clouds_of(case)
    raws = raw_of_clouds(case)
    d, raw, itp = run_clouds(enc, case, pts, off)
    check(case, raws, d, raw, itp)
    if case.kernel == "fast" or case.entry == "split":          # min() is order-free
        d2, raw2, itp2 = run_clouds(enc, case, EF.shuffled(pts, off), off)
        assert np.array_equal(u32(d2), u32(d)) and np.array_equal(u32(raw2), u32(raw)) and np.array_equal(u32(itp2), u32(itp))


@by_entry("finish_images")
def test_finish_images(case):
    """nsc_finish_images on squared-range bit images built directly (0xffffffff = empty pixel)."""
    enc = encoder(case)
    raws = np.stack([im for _, im in EF.images_of(case)])
    n = len(raws)
    sq = torch.from_numpy(np.stack([EF.sqr_bits(im) for im in raws]).view(np.int32)).cuda()
    out = torch.empty((n, case.R * case.B), device="cuda")
    raw, itp = torch.empty((n, case.E, A), device="cuda"), torch.empty((n, case.E, A), device="cuda")
    st = _lib.lib().nsc_finish_images(_lib.ptr(sq), n, params(enc, case), _lib.ptr(enc._lut(sq.device)), _lib.ptr(out),
                                      _lib.ptr(raw), _lib.ptr(itp), _lib.stream_ptr(sq.device))
    assert st == 0
    torch.cuda.synchronize()
    check(case, raws, out.cpu().numpy(), raw.cpu().numpy(), itp.cpu().numpy())


@by_entry("range_images")
def test_encode_range_images(case):
    """SpectralEncoder.forward (finish_kernel mode 1): no interpolation, rows != 16 pooled in both directions."""
    enc = encoder(case)
    raws = np.stack([im for _, im in EF.images_of(case)])
    d = enc.forward(torch.from_numpy(raws).cuda())
    torch.cuda.synchronize()
    check(case, raws, d.cpu().numpy(), None, None)


@by_entry("interpolate_ex")
def test_interpolate_range_images(case):
    """interpolate_range_image (finish_kernel mode 2), linear and nearest, holes written as 0, -1.0, -0.0 and NaN."""
    names = [n for n, _ in EF.images_of(case)]
    raws = np.stack([im for _, im in EF.images_of(case)])
    out = interpolate_range_image(raws, method={1: "linear", 2: "nearest"}[case.interp])
    for i, n in enumerate(names):
        want = EF.interpolated(raws[i], case.interp)
        assert np.array_equal(u32(out[i]), u32(want)), n
        if np.any(raws[i] > 0):
            assert np.all(out[i] > 0), n                          # every way of writing a hole was overwritten
    one = interpolate_range_image(raws[0], method={1: "linear", 2: "nearest"}[case.interp])
    assert np.array_equal(u32(one), u32(out[0]))
