"""Parity of the HIP encoder (through the C ABI) against the CPU oracle and the reference goldens.

Bars (north_star): range image bit-exact; histogram bin indices bit-exact (LUT);
descriptor |gpu - oracle| <= 1e-6*|oracle| + 1e-9 (both evaluate the DFT in float64), and
|gpu - reference| <= 1e-5*|ref| + 1e-7 (the reference runs a float32 FFT).
"""
import glob
import os

import numpy as np
import pytest
import torch

import nsc_oracle as orc
from neural_spectral_codec_amd import synth
from neural_spectral_codec_amd.encoding import SpectralEncoder

pytestmark = pytest.mark.gpu

CASES = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "enc_*.npz")))
CLEAN = {"uniform20k", "safe20k", "uniform120k", "adversarial", "wide20k", "xyz_only", "empty",
         "single_pt", "e64_ring"}


def _enc(E=16, elevation_range=(-24.8, 2.0), **kw):
    return SpectralEncoder(n_elevation=E, n_azimuth=360, n_bins=50, alpha=2.0,
                           target_elevation_bins=16, elevation_range=elevation_range, **kw).to("cuda")


def _close(d, ref, rtol, atol):
    return np.all(np.abs(d - ref) <= rtol * np.abs(ref) + atol)


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(c)[4:-4] for c in CASES])
def test_golden_clouds(path):
    g = np.load(path)
    name = os.path.basename(path)[4:-4]
    E, er = int(g["n_elevation"]), tuple(g["elevation_range"])
    enc = _enc(E, er)
    d, raw, itp = enc.encode_points_batch([g["points"]], return_images=True)
    d, raw, itp = d[0].cpu().numpy(), raw[0].cpu().numpy(), itp[0].cpu().numpy()
    p = orc.default_params(n_elevation=E, elevation_range=er)
    od, oraw, oitp = orc.encode_points(g["points"], p, want_images=True)
    assert np.array_equal(raw.view(np.uint32), oraw.view(np.uint32)), "raw range image differs from oracle"
    assert np.array_equal(itp.view(np.uint32), oitp.view(np.uint32)), "interpolated image differs from oracle"
    assert _close(d, od, 1e-6, 1e-9)
    if name in CLEAN:                       # no atan2-ULP edge points: identical to the reference too
        assert np.array_equal(raw.view(np.uint32), g["ref_raw"])
        assert np.array_equal(itp.view(np.uint32), g["ref_interp"])
        assert _close(d, g["ref_desc"], 1e-5, 1e-7)


def test_encode_points_api_matches_reference_call_shape():
    g = np.load(CASES[0])
    enc = _enc()
    out = enc.encode_points(g["points"])
    assert out.shape == (800,) and out.is_cuda
    host = out.detach().cpu().numpy()       # what pipeline.py:245 does with it
    assert abs(host.sum() - 1.0) < 1e-5


def test_point_bins_match_oracle_and_slow_path_rate():
    from neural_spectral_codec_amd import _lib
    rng = np.random.default_rng(0)
    pts = synth.make_cloud(100, 2_000_000, "uniform")
    # a block of points sitting on / next to column and row edges
    n_e = 200_000
    c = rng.integers(0, 360, n_e)
    r = rng.integers(0, 17, n_e)
    az = -np.pi + c * (2 * np.pi / 360) + (rng.uniform(-1, 1, n_e) * 2e-6)
    lo, hi = np.deg2rad(-24.8), np.deg2rad(2.0)
    el = lo + r * (hi - lo) / 16 + rng.uniform(-1, 1, n_e) * 2e-6
    rr = rng.uniform(1, 70, n_e)
    edge = np.stack([rr * np.cos(el) * np.cos(az), rr * np.cos(el) * np.sin(az), rr * np.sin(el),
                     np.zeros(n_e)], 1).astype(np.float32)
    axis = np.zeros((8, 4), np.float32)
    axis[:, :3] = [[5, 0, 0], [-5, 0, 0], [0, 5, 0], [0, -5, 0], [-5, -0.0, 0], [3, 3, 0], [-3, 3, 1], [0, 0, 5]]
    allp = np.concatenate([pts, edge, axis], 0)
    p = orc.default_params()
    _, oidx, _ = orc.project(allp, p, want_idx=True)
    enc = _enc()
    t = torch.from_numpy(allp).cuda()
    idx = torch.empty(len(allp), dtype=torch.int32, device="cuda")
    fl = torch.empty(len(allp), dtype=torch.uint8, device="cuda")
    st = _lib.lib().nsc_debug_point_bins(_lib.ptr(t), len(allp), 4, enc._params(), _lib.ptr(idx),
                                         _lib.ptr(fl), _lib.stream_ptr(t.device))
    assert st == 0
    torch.cuda.synchronize()
    idx, fl = idx.cpu().numpy(), fl.cpu().numpy()
    assert np.array_equal(idx, oidx)
    kept = oidx[:len(pts)] >= 0
    slow = (fl[:len(pts)][kept] != 0).mean()
    print(f"exact-path fraction on uniform cloud: {slow:.2e}")
    assert slow < 1e-3                       # the float64 atan2 path (the uncertain queue) must stay rare


def test_ragged_batch_and_empty_clouds():
    enc = _enc()
    sizes = [5000, 0, 1, 17000, 333, 0, 2048]
    clouds = [synth.make_cloud(200 + i, n, "uniform") if n else np.zeros((0, 4), np.float32)
              for i, n in enumerate(sizes)]
    d = enc.encode_points_batch(clouds).cpu().numpy()
    for i, c in enumerate(clouds):
        od = orc.encode_points(c)
        assert _close(d[i], od, 1e-6, 1e-9), i
    assert np.array_equal(d[1], np.full(800, np.float32(1) / np.float32(800)))


def test_fast_kernel_window_edges():
    """encode_fast_kernel streams a cloud in rounds of U x 256 points with a rolling window of loads (U = 2 ships, 8 in
    round-2 development builds): cloud sizes around every boundary of both schemes (one lane, one wave, one workgroup
    pass, one round, several rounds +- 1), all in ONE batch so that every workgroup takes a different path through the
    prologue / main loop / tail."""
    enc = _enc()
    sizes = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048, 2049, 2303,
             2304, 4095, 4096, 4097, 6143, 6144, 6145, 8191, 8192, 20479, 20480, 20481, 33333]
    clouds = [synth.make_cloud(900 + i, n, ("uniform", "wide", "adversarial")[i % 3]) for i, n in enumerate(sizes)]
    assert [len(c) for c in clouds] == sizes
    d, raw, itp = enc.encode_points_batch(clouds, return_images=True)
    for i, c in enumerate(clouds):
        od, oraw, oitp = orc.encode_points(c, want_images=True)
        assert np.array_equal(raw[i].cpu().numpy().view(np.uint32), oraw.view(np.uint32)), sizes[i]
        assert np.array_equal(itp[i].cpu().numpy().view(np.uint32), oitp.view(np.uint32)), sizes[i]
        assert _close(d[i].cpu().numpy(), od, 1e-6, 1e-9), sizes[i]


def test_fast_kernel_uncertain_queue_overflow():
    """Clouds whose points ALL sit within a few 1e-6 rad of a bin edge: every point is 'uncertain', the 240-entry LDS
    queue of encode_fast_kernel overflows and the kernel falls back to streaming the cloud again with the per-point
    exact path.  Mixed into a batch with ordinary clouds; images bit-exact."""
    enc = _enc()
    rng = np.random.default_rng(5)
    clouds = []
    for k, n_e in enumerate((200, 241, 5000, 30000)):          # below, just above and far above the queue capacity
        c = rng.integers(0, 360, n_e)
        r = rng.integers(0, 17, n_e)
        az = -np.pi + c * (2 * np.pi / 360) + rng.uniform(-1, 1, n_e) * 2e-6
        lo, hi = np.deg2rad(-24.8), np.deg2rad(2.0)
        el = lo + r * (hi - lo) / 16 + rng.uniform(-1, 1, n_e) * 2e-6
        rr = rng.uniform(1, 70, n_e)
        edge = np.stack([rr * np.cos(el) * np.cos(az), rr * np.cos(el) * np.sin(az), rr * np.sin(el),
                         np.zeros(n_e)], 1).astype(np.float32)
        clouds += [edge, synth.make_cloud(950 + k, 7000, "uniform")]
    d, raw, itp = enc.encode_points_batch(clouds, return_images=True)
    for i, c in enumerate(clouds):
        od, oraw, oitp = orc.encode_points(c, want_images=True)
        assert np.array_equal(raw[i].cpu().numpy().view(np.uint32), oraw.view(np.uint32)), i
        assert np.array_equal(itp[i].cpu().numpy().view(np.uint32), oitp.view(np.uint32)), i
        assert _close(d[i].cpu().numpy(), od, 1e-6, 1e-9), i


def test_large_batch_stays_on_the_fast_kernel():
    """1 200 clouds x 120 000 points = 144 M points (2.3 GB): beyond the 2^27-point BATCH limit that sent anything above
    1 118 such clouds to the generic kernel in round 2.  The limit the kernel needs is per cloud; the launcher's own
    decision function must say "fast" for this batch, and the result must not depend on how the batch is cut: every
    cloud's descriptor equals, bit for bit, the one it gets in a 1 024-cloud / 176-cloud launch; sampled clouds equal
    the oracle."""
    from neural_spectral_codec_amd import _lib
    enc = _enc()
    n, npts = 1200, 120000
    L = _lib.lib()
    assert L.nsc_encode_clouds_path(n, n * npts, 4, enc._params()) == 1            # NSC_ENC_PATH_FAST
    assert L.nsc_encode_clouds_path(5000, 5000 * npts, 4, enc._params()) == 1
    assert L.nsc_encode_clouds_path(n, n * npts, 3, enc._params()) == 2            # (N,3) points: generic kernel
    assert L.nsc_encode_clouds_path(3, 3 * npts, 4, enc._params()) == 3            # few big clouds: split path
    pts, off = synth.make_clouds_device(n, npts, "cuda", seed=21)
    d = enc.encode_points_batch((pts, off))
    torch.cuda.synchronize()
    assert torch.allclose(d.sum(1), torch.ones(n, device="cuda"), atol=1e-5)
    d_a = enc.encode_points_batch((pts[:1024 * npts], off[:1025]))
    d_b = enc.encode_points_batch((pts[1024 * npts:], off[1024:] - off[1024]))
    assert torch.equal(d[:1024], d_a) and torch.equal(d[1024:], d_b)
    for c in (0, 1118, 1119, 1199):
        host = pts[c * npts:(c + 1) * npts].cpu().numpy()
        assert _close(d[c].cpu().numpy(), orc.encode_points(host), 1e-6, 1e-9), c


def test_cloud_beyond_the_streaming_limit_inside_a_fast_batch():
    """ONE cloud of 2^27 + 37 points (2.1 GB) among 511 small ones: the batch is launched on the fast kernel, whose
    streaming loop addresses a cloud with 32-bit byte offsets; the workgroup of the big cloud must take the kernel's
    64-bit cold loop, the others the stream.  Raw / interpolated image of the big cloud bit-exact against the oracle."""
    from neural_spectral_codec_amd import _lib
    enc = _enc()
    big = (1 << 27) + 37
    small = [synth.make_cloud(4000 + i, 100 + i, "uniform") for i in range(511)]
    bp, _ = synth.make_clouds_device(1, big, "cuda", seed=5)
    sp = torch.from_numpy(np.concatenate(small, 0)).cuda()
    k = 200                                                       # the big cloud sits in the middle of the batch
    n_before = sum(len(c) for c in small[:k])
    pts = torch.cat([sp[:n_before], bp, sp[n_before:]], 0).contiguous()
    sizes = [len(c) for c in small[:k]] + [big] + [len(c) for c in small[k:]]
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device="cuda")
    del bp, sp
    assert _lib.lib().nsc_encode_clouds_path(512, int(pts.shape[0]), 4, enc._params()) == 1
    d, raw, itp = enc.encode_points_batch((pts, off), return_images=True)
    torch.cuda.synchronize()
    host = pts[n_before:n_before + big].cpu().numpy()
    od, oraw, oitp = orc.encode_points(host, want_images=True)
    assert np.array_equal(raw[k].cpu().numpy().view(np.uint32), oraw.view(np.uint32))
    assert np.array_equal(itp[k].cpu().numpy().view(np.uint32), oitp.view(np.uint32))
    assert _close(d[k].cpu().numpy(), od, 1e-6, 1e-9)
    for i in (0, k - 1, k + 1, 511):
        c = small[i if i < k else i - 1]
        assert _close(d[i].cpu().numpy(), orc.encode_points(c), 1e-6, 1e-9), i


def test_split_path_small_batch_of_big_clouds():
    """3 x 120k points: clouds are split over workgroups and merged with global atomicMin."""
    enc = _enc()
    clouds = [synth.make_cloud(300 + i, 120000, k) for i, k in enumerate(["uniform", "ring", "wide"])]
    d, raw, itp = enc.encode_points_batch(clouds, return_images=True)
    for i, c in enumerate(clouds):
        od, oraw, oitp = orc.encode_points(c, want_images=True)
        assert np.array_equal(raw[i].cpu().numpy().view(np.uint32), oraw.view(np.uint32))
        assert np.array_equal(itp[i].cpu().numpy().view(np.uint32), oitp.view(np.uint32))
        assert _close(d[i].cpu().numpy(), od, 1e-6, 1e-9)


def test_fused_path_large_batch_and_point_order_invariance():
    """600 clouds x 3000 points -> one workgroup per cloud.  min() is order-free: shuffling the
    points of a cloud must give bit-identical output."""
    enc = _enc()
    pts, off = synth.make_clouds_packed(range(400, 1000), 3000, "uniform")
    d = enc.encode_points_batch((torch.from_numpy(pts), torch.from_numpy(off))).cpu().numpy()
    od = orc.encode_clouds(pts, off, n_threads=8)
    assert _close(d, od, 1e-6, 1e-9)
    rng = np.random.default_rng(1)
    sh = pts.copy()
    for c in range(len(off) - 1):
        sh[off[c]:off[c + 1]] = pts[off[c]:off[c + 1]][rng.permutation(off[c + 1] - off[c])]
    d2 = enc.encode_points_batch((torch.from_numpy(sh), torch.from_numpy(off))).cpu().numpy()
    assert np.array_equal(d.view(np.uint32), d2.view(np.uint32))


def test_forward_on_range_images(golden_dir):
    g = np.load(os.path.join(golden_dir, "range_images.npz"))
    enc = _enc()
    p = orc.default_params()
    for key_i, key_d in (("imgs16", "desc16"), ("imgs64", "desc64")):
        d = enc.forward(torch.from_numpy(g[key_i]).cuda()).cpu().numpy()
        for i in range(len(d)):
            assert _close(d[i], orc.encode_range_image(g[key_i][i], p), 1e-6, 1e-9)
            assert _close(d[i], g[key_d][i], 1e-5, 1e-7)
    one = enc.encode_range_image(torch.from_numpy(g["imgs16"][0]).cuda()).cpu().numpy()
    assert _close(one, g["desc16"][0], 1e-5, 1e-7)


def test_float32_row_math_mode():
    """numpy 1.24 value-based casting: row index computed in float32 (elev_f64 = 0)."""
    enc = _enc(elev_float64=False)
    c = synth.make_cloud(77, 50000, "uniform")
    d, raw, _ = enc.encode_points_batch([c], return_images=True)
    p = orc.default_params(elev_f64=0)
    od, oraw, _ = orc.encode_points(c, p, want_images=True)
    assert np.array_equal(raw[0].cpu().numpy().view(np.uint32), oraw.view(np.uint32))
    assert _close(d[0].cpu().numpy(), od, 1e-6, 1e-9)


def test_other_alpha_and_bins():
    enc = SpectralEncoder(n_elevation=16, n_bins=32, alpha=1.0, target_elevation_bins=16).to("cuda")
    c = synth.make_cloud(78, 30000, "ring")
    d = enc.encode_points(c).cpu().numpy()
    p = orc.default_params(n_bins=32)
    lut = orc.bin_lut(1.0, 32, 181, 1e-8)[1]
    assert d.shape == (16 * 32,)
    assert _close(d, orc.encode_points(c, p, lut), 1e-6, 1e-9)


def test_bench_sized_batch_sampled_against_oracle():
    """Full-size clouds generated in HBM (bench workload shape, 64 clouds here); sample checked."""
    enc = _enc()
    pts, off = synth.make_clouds_device(64, 120000, "cuda", seed=3)
    d = enc.encode_points_batch((pts, off))
    torch.cuda.synchronize()
    assert torch.allclose(d.sum(1), torch.ones(64, device="cuda"), atol=1e-5)
    for c in (0, 31, 63):
        host = pts[c * 120000:(c + 1) * 120000].cpu().numpy()
        assert _close(d[c].cpu().numpy(), orc.encode_points(host), 1e-6, 1e-9)


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(c)[4:-4] for c in CASES])
def test_interpolate_range_image_standalone(path):
    """interpolate_range_image() drop-in (range_image.py:15-89): reference raw image in, reference
    interpolated image out, bit for bit."""
    from neural_spectral_codec_amd.encoding.range_image import interpolate_range_image
    g = np.load(path)
    out = interpolate_range_image(g["ref_raw"].view(np.float32))
    assert np.array_equal(out.view(np.uint32), g["ref_interp"])


def test_interpolate_range_image_nearest(golden_dir):
    """method='nearest' (range_image.py:66-75): circularly nearest valid pixel, smaller column on a tie; bit for bit
    against the reference's outputs, single image and batched."""
    from neural_spectral_codec_amd.encoding.range_image import interpolate_range_image
    g = np.load(os.path.join(golden_dir, "interp_nearest.npz"))
    raw = g["raw"].view(np.float32)
    for im, want in zip(raw, g["nearest"]):
        assert np.array_equal(interpolate_range_image(im, method="nearest").view(np.uint32), want)
    assert np.array_equal(interpolate_range_image(raw, method="nearest").view(np.uint32), g["nearest"])
    with pytest.raises(ValueError):
        interpolate_range_image(raw[0], method="cubic")


def test_projector_project_matches_reference(golden_dir):
    from neural_spectral_codec_amd.encoding.range_image import RangeImageProjector
    g = np.load(os.path.join(golden_dir, "enc_uniform20k.npz"))
    img, inten = RangeImageProjector(n_elevation=16).project(g["points"], keep_intensity=False)
    assert inten is None and np.array_equal(img.view(np.uint32), g["ref_raw"])


def test_scatter_and_finish_as_separate_launches():
    """nsc_scatter_clouds + nsc_finish_images == nsc_encode_clouds (bit for bit) where nsc_encode_clouds runs other
    kernels; where it would run the same split kernels, both launches are held to the C oracle."""
    from neural_spectral_codec_amd import _lib
    enc = _enc()
    L, p = _lib.lib(), enc._params()
    # split_parts() gives 1 for the first two batches (20000 / 16384 = 1 part by size; 600 clouds >= 512): nsc_scatter_clouds
    # takes its one-workgroup-per-cloud branch, nsc_encode_clouds the fast kernel, which is the reference.  The third is the
    # smallest batch that splits (32768 / 16384 = 2 parts per cloud): nsc_scatter_clouds takes its parts > 1 branch,
    # nsc_encode_clouds would run the same two kernels, so the reference is the C oracle.
    for seeds, npts, kind in ((range(50, 60), 20000, "ring"), (range(600), 1000, "uniform"), (range(2), 32768, "uniform")):
        n = len(seeds)
        pts, off = synth.make_clouds_packed(seeds, npts, kind)
        tp, to = torch.from_numpy(pts).cuda(), torch.from_numpy(off).cuda()
        split = L.nsc_encode_clouds_path(n, n * npts, 4, p) == 3            # NSC_ENC_PATH_SPLIT
        assert split == (npts == 32768)
        sq = torch.empty((n, 16, 360), dtype=torch.int32, device="cuda")
        out = torch.empty((n, 800), device="cuda")
        lut, st = enc._lut(tp.device), _lib.stream_ptr(tp.device)
        assert L.nsc_scatter_clouds(_lib.ptr(tp), _lib.ptr(to), n, int(tp.shape[0]), 4, p, _lib.ptr(sq), st) == 0
        assert L.nsc_finish_images(_lib.ptr(sq), n, p, _lib.ptr(lut), _lib.ptr(out), None, None, st) == 0
        torch.cuda.synchronize()
        if not split:
            assert torch.equal(out, enc.encode_points_batch((tp, to)))
            continue
        od, oraw, _ = orc.encode_clouds(pts, off, want_images=True)
        bits = sq.cpu().numpy().view(np.uint32)
        empty = bits == 0xffffffff                                          # NSC_EMPTY_BITS: no point in the pixel -> range 0
        rng = np.where(empty, np.float32(0), np.sqrt(np.where(empty, 0, bits).astype(np.uint32).view(np.float32)))
        assert np.array_equal(rng.view(np.uint32), oraw.view(np.uint32)), "scatter image differs from oracle"
        assert _close(out.cpu().numpy(), od, 1e-6, 1e-9)


def test_full_bench_size_properties():
    """BASELINE configs[1] at full size (1 024 clouds x 120 000 points, 1.97 GB in HBM), through
    size-independent properties: rows sum to 1, a cloud's descriptor does not depend on its position in
    the batch or on its neighbours (reversed batch order gives the reversed result, bit for bit), and
    sampled clouds equal the oracle."""
    enc = _enc()
    n, npts = 1024, 120000
    pts, off = synth.make_clouds_device(n, npts, "cuda", seed=11)
    d = enc.encode_points_batch((pts, off))
    assert torch.allclose(d.sum(1), torch.ones(n, device="cuda"), atol=1e-5)
    rev = pts.view(n, npts, 4).flip(0).reshape(-1, 4).contiguous()
    d2 = enc.encode_points_batch((rev, off))
    assert torch.equal(d2.flip(0), d)
    del rev, d2
    for c in (0, 511, 1023):
        host = pts[c * npts:(c + 1) * npts].cpu().numpy()
        assert _close(d[c].cpu().numpy(), orc.encode_points(host), 1e-6, 1e-9)


def test_intensity_image_matches_reference():
    """RangeImageProjector.project(points, keep_intensity=True): range and intensity images against the fixture made
    by the reference itself (oracle/gen_golden_intensity.py) and against the oracle restatement."""
    from neural_spectral_codec_amd.encoding.range_image import RangeImageProjector
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "intensity.npz"))
    proj = RangeImageProjector(n_elevation=16, n_azimuth=360, device="cuda")
    for k in ("c0", "c1", "c2", "c3"):                  # c3: NaN / +inf intensities (np.maximum.at propagates NaN)
        pts = g[k + "_pts"]
        rimg, iimg = proj.project(pts, keep_intensity=True)
        assert rimg.dtype == np.float32 and iimg.dtype == np.float32 and iimg.shape == (16, 360)
        assert (rimg.view(np.uint32) == g[k + "_range"].view(np.uint32)).all(), k
        assert (iimg.view(np.uint32) == g[k + "_intensity"].view(np.uint32)).all(), k
        oimg, ointen = orc.project_intensity(pts)
        assert (iimg.view(np.uint32) == ointen.view(np.uint32)).all() and (rimg.view(np.uint32) == oimg.view(np.uint32)).all()
    r2, i2 = proj.project(g["c0_pts"], keep_intensity=False)
    assert i2 is None and (r2.view(np.uint32) == g["c0_range"].view(np.uint32)).all()
    r3, i3 = proj.project(g["c0_pts"][:, :3])                       # (N,3): no intensity column
    assert i3 is None and (r3.view(np.uint32) == g["c0_range"].view(np.uint32)).all()
    from neural_spectral_codec_amd.encoding.range_image import project_to_range_image
    r4 = project_to_range_image(g["c0_pts"], n_elevation=16)
    assert (r4.view(np.uint32) == g["c0_range"].view(np.uint32)).all()


def test_batch_whose_offsets_pass_2_31_floats():
    """Maximum sizes: 4 600 clouds x 120 000 points in ONE call = 2.2e9 floats (8.8 GB): the float offset of the last clouds'
    points lies beyond 2^31 and their byte offset beyond 2^33 -- every cloud's base is 64-bit arithmetic on cloud_offsets
    (int64), only the offsets INSIDE a cloud are 32-bit.  The last clouds' descriptors and range images equal what the same
    clouds give as a small batch of their own, bit for bit, and the oracle's on a sample."""
    enc = _enc()
    n, npts = 4600, 120000
    pts, off = synth.make_clouds_device(n, npts, "cuda", seed=11)
    assert pts.numel() > 2 ** 31 and int(off[-1]) == n * npts
    d, raw, _ = enc.encode_points_batch((pts, off), return_images=True)
    torch.cuda.synchronize()
    assert torch.allclose(d.sum(1), torch.ones(n, device="cuda"), atol=1e-5)
    for lo, hi in ((0, 4), (4470, 4482), (n - 12, n)):         # first clouds, the ones around 2^31 floats, the last ones
        sub = pts[lo * npts:hi * npts].clone()
        soff = torch.arange(0, (hi - lo + 1) * npts, npts, dtype=torch.int64, device="cuda")
        ds, rs, _ = enc.encode_points_batch((sub, soff), return_images=True)
        assert torch.equal(ds, d[lo:hi]) and torch.equal(rs, raw[lo:hi]), (lo, hi)
    for c in (4474, n - 1):
        host = pts[c * npts:(c + 1) * npts].cpu().numpy()
        assert _close(d[c].cpu().numpy(), orc.encode_points(host), 1e-6, 1e-9)


@pytest.mark.parametrize("shape", ["fast", "fused", "split", "range_images"])
def test_encoder_entry_points_replay_as_a_captured_graph(shape):
    """include/nsc.h: every call is asynchronous, allocates nothing, keeps no state and may be captured into a hipGraph.  Each
    path of nsc_encode_clouds (the streaming fast kernel, the fused kernel of other shapes, the split path with its workspace
    fill -- a kernel, not a memset node) and nsc_encode_range_images is captured once and replayed on NEW input written into
    the same buffers: the replay gives what an eager call on that input gives, bit for bit."""
    from neural_spectral_codec_amd import _lib
    L = _lib.lib()
    if shape == "range_images":
        enc = _enc()
        a, b = (torch.rand((32, 16, 360), device="cuda", generator=torch.Generator("cuda").manual_seed(s)) * 60 for s in (1, 2))
        run = lambda x: enc(x)
        inputs = (a, b)
    else:
        enc = _enc(E={"fast": 16, "fused": 64, "split": 16}[shape])
        n, npts = {"fast": (64, 30000), "fused": (64, 30000), "split": (2, 400000)}[shape]
        batches = [synth.make_clouds_device(n, npts, "cuda", seed=s) for s in (5, 6)]
        assert L.nsc_encode_clouds_path(n, n * npts, 4, enc._params()) == {"fast": 1, "fused": 2, "split": 3}[shape]   # NSC_ENC_PATH_*
        off = batches[0][1]
        run = lambda x: enc.encode_points_batch((x, off))
        inputs = (batches[0][0], batches[1][0])
    with torch.no_grad():
        want = [run(x).clone() for x in inputs]
        buf = inputs[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run(buf)                                           # warm-up on the capturing stream (lazy set-up, scratch)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg):
            out = run(buf)
        for x, w in zip((inputs[1], inputs[0], inputs[1]), (want[1], want[0], want[1])):
            buf.copy_(x)
            cg.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, w)
    assert not torch.equal(want[0], want[1])
