"""Every projection path of the encoder's point stage on the constructed clouds of tests/point_families.py, against the
oracle.  All comparisons are exact unless stated:
  - nsc_debug_point_bins: the pixel of every point (dropped = -1); the exact-path flag of every DETERMINED point (the three
    host builds of csrc/nsc_math.h agree on it); the share of undetermined points is printed, < 10 % in `edges`, 0 in `queue`;
  - nsc_encode_clouds through encode_fast_kernel, encode_fused_kernel<4 / 8 / 16> and the split path: raw and interpolated
    image bit for bit, descriptor |gpu - oracle| <= 1e-6 |oracle| + 1e-9; a sentinel batch packed and cloud by cloud;
  - nsc_scatter_clouds: the words of tests/point_families.py::scatter_words;
  - nsc_project_intensity: orc.project_intensity, NaN pixels included;
  - every batch again with the points of each cloud shuffled: bit-identical.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import nsc_oracle as orc
import point_families as PF
from point_families import A, SETS
from neural_spectral_codec_amd import _lib
from neural_spectral_codec_amd.encoding.spectral_encoder import _default_lut, _run_encode_clouds

pytestmark = pytest.mark.gpu

SS = [(ps, stride) for ps in SETS for stride in ps.strides]
SS_IDS = ["%s-s%d" % (ps.name, stride) for ps, stride in SS]
_CACHE = {}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return PF.host_libs(tmp_path_factory.mktemp("point_stage_host"))


def u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def enc_params(ps):
    p = _lib.EncParams()
    _lib.lib().nsc_enc_default_params(C.byref(p))
    p.n_elevation, p.target_rows, p.n_bins, p.elev_f64, p.interpolate = ps.E, PF.target_rows(ps), PF.N_BINS, ps.f64, 1
    p.elev_min_rad, p.elev_max_rad = PF.fov_rad(ps)
    p.min_range, p.max_range = ps.rmin, ps.rmax
    return p


def cols(buf, stride):
    return np.ascontiguousarray(buf if stride == 4 else buf[:, :3])


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def reference(ps, stride, buf, off):
    """(descriptors, raw images, interpolated images) of the oracle: computed once per batch, shared, never modified."""
    out = orc.encode_clouds(cols(buf, stride), off, PF.oparams(ps), lut_host(), want_images=True)
    for a in out:
        a.setflags(write=False)
    return out


def lut_host():
    return cached("lut", lambda: orc.bin_lut(2.0, PF.N_BINS, 181, 1e-8)[1])


def family_batch(host, ps, stride):
    def make():
        fams = PF.point_families(host, ps, stride)
        return PF.guarded(ps, [fams[n].pts for n in PF.POINT_FAMILIES])
    return cached(("families", ps.name, stride), make)


def gpu_encode(host, ps, stride, tp, off, c0=0, c1=None):
    """nsc_encode_clouds on clouds c0..c1 of the packed device buffer; asserts the path the restated dispatch names."""
    c1 = len(off) - 1 if c1 is None else c1
    n, total = c1 - c0, int(off[c1] - off[c0])
    to = torch.from_numpy(np.ascontiguousarray(off[c0:c1 + 1])).cuda()
    p = enc_params(ps)
    kernel = PF.kernel_for(ps, host[0].bin_params(ps)[1], stride, n, total)
    assert _lib.lib().nsc_encode_clouds_path(n, total, stride, p) == PF.ENC_PATH[kernel]
    d, raw, itp = _run_encode_clouds(tp, to, n, total, stride, p, _default_lut(tp.device), want_images=True)
    torch.cuda.synchronize()
    return kernel, d.cpu().numpy(), raw.cpu().numpy(), itp.cpu().numpy()


def check_encode(name, got, ref):
    _, d, raw, itp = got
    rd, rraw, ritp = ref
    for c in range(len(rd)):
        assert np.array_equal(u32(raw[c]), u32(rraw[c])), "%s: raw image of cloud %d differs from the oracle" % (name, c)
        assert np.array_equal(u32(itp[c]), u32(ritp[c])), "%s: interpolated image of cloud %d differs from the oracle" % (name, c)
        ratio = np.abs(d[c] - rd[c]) / PF.bar(rd[c])
        assert np.all(ratio <= 1.0), "%s: descriptor of cloud %d: |gpu - oracle| / bar = %.3g" % (name, c, ratio.max())


def same_bits(a, b):
    return all(np.array_equal(u32(x), u32(y)) for x, y in zip(a[1:], b[1:]))


def encode_and_shuffle(host, ps, stride, name, buf, off, kernel):
    tp = torch.from_numpy(cols(buf, stride)).cuda()
    got = gpu_encode(host, ps, stride, tp, off)
    assert got[0] == kernel, (name, got[0])
    check_encode(name, got, cached(("ref", name, ps.name, stride), lambda: reference(ps, stride, buf, off)))
    again = gpu_encode(host, ps, stride, torch.from_numpy(cols(PF.shuffled(buf, off), stride)).cuda(), off)
    assert same_bits(got, again), "%s: shuffling the points of each cloud changed the result" % name
    return tp, got


def gpu_scatter(ps, stride, tp, off):
    n, total = len(off) - 1, int(off[-1] - off[0])
    to = torch.from_numpy(off).cuda()
    sq = torch.empty((n, ps.E, A), dtype=torch.int32, device="cuda")
    st = _lib.lib().nsc_scatter_clouds(_lib.ptr(tp), _lib.ptr(to), n, total, stride, enc_params(ps), _lib.ptr(sq),
                                       _lib.stream_ptr(tp.device))
    assert st == 0
    torch.cuda.synchronize()
    return sq.cpu().numpy().view(np.uint32)


def check_scatter(host, ps, stride, name, buf, off, parts):
    assert PF.split_parts(len(off) - 1, int(off[-1] - off[0])) == parts
    bp = host[0].bin_params(ps)[0]
    want = cached(("words", name, ps.name, stride), lambda: PF.scatter_words(ps, bp, buf, off))
    got = gpu_scatter(ps, stride, torch.from_numpy(cols(buf, stride)).cuda(), off)
    assert np.array_equal(got, want), "%s: nsc_scatter_clouds differs from the reference words" % name
    again = gpu_scatter(ps, stride, torch.from_numpy(cols(PF.shuffled(buf, off), stride)).cuda(), off)
    assert np.array_equal(again, got)


@pytest.mark.parametrize("ps,stride", SS, ids=SS_IDS)
def test_point_bins(host, ps, stride):
    """nsc_debug_point_bins (point_bins_kernel, lean mode at (N, 4) points, 16 rows and a lean-valid parameter set) on every
    family the set has, in one launch."""
    names = PF.bins_families(ps, stride)
    fams = [PF.family_points(host, ps, stride, n) for n in names]
    pts = cols(np.concatenate(fams), stride)
    bounds = np.concatenate([[0], np.cumsum([len(f) for f in fams])])
    t = torch.from_numpy(pts).cuda()
    idx = torch.empty(len(pts), dtype=torch.int32, device="cuda")
    fl = torch.empty(len(pts), dtype=torch.uint8, device="cuda")
    st = _lib.lib().nsc_debug_point_bins(_lib.ptr(t), len(pts), stride, enc_params(ps), _lib.ptr(idx), _lib.ptr(fl),
                                         _lib.stream_ptr(t.device))
    assert st == 0
    torch.cuda.synchronize()
    idx, fl = idx.cpu().numpy(), fl.cpu().numpy()
    _, oidx = PF.project(ps, pts)
    want, det = PF.device_flags(host, ps, stride, pts)
    for i, n in enumerate(names):
        s = slice(bounds[i], bounds[i + 1])
        bad = np.nonzero(idx[s] != oidx[s])[0]
        assert len(bad) == 0, "%s: pixel of point %d (%s): device %d, oracle %d" % (n, bad[0], pts[s][bad[0]], idx[s][bad[0]], oidx[s][bad[0]])
        share = 1.0 - det[s].mean()
        print("%s stride %d %-8s: undetermined %.2f %%, exact path on the device %.2f %%" % (ps.name, stride, n, 100 * share, 100 * (fl[s] != 0).mean()))
        assert share < 0.10 if n == "edges" else True
        assert share == 0.0 if n == "queue" else True
        bad = np.nonzero(det[s] & (fl[s] != want[s]))[0]
        assert len(bad) == 0, "%s: flag of determined point %d (%s): device %d, host %d" % (n, bad[0], pts[s][bad[0]], fl[s][bad[0]], want[s][bad[0]])


@pytest.mark.parametrize("ps,stride", SS, ids=SS_IDS)
def test_encode_clouds_families(host, ps, stride):
    """edges, axes, window, min_wins and census as the five clouds of one batch."""
    buf, off = family_batch(host, ps, stride)
    small = ps.kernel4 if stride == 4 else {"fast": "fused4"}.get(ps.kernel4, ps.kernel4)
    encode_and_shuffle(host, ps, stride, "families", buf, off, small)


@pytest.mark.parametrize("ps,stride", SS, ids=SS_IDS)
def test_encode_clouds_sentinels(host, ps, stride):
    """The prefix-census clouds between guard clouds: packed, then every cloud alone in the same buffer."""
    fam = PF.sentinels(ps)
    buf, off = fam.pts, fam.claims["off"]
    small = ps.kernel4 if stride == 4 else {"fast": "fused4"}.get(ps.kernel4, ps.kernel4)
    tp, packed = encode_and_shuffle(host, ps, stride, "sentinels", buf, off, small)
    for c, role in enumerate(fam.claims["role"]):
        if role == "guard" and c > 2:                         # the guard clouds are all the same points: two of them do
            continue
        alone = gpu_encode(host, ps, stride, tp, off, c, c + 1)
        assert alone[0] == small
        assert all(np.array_equal(u32(x[0]), u32(y[c])) for x, y in zip(alone[1:], packed[1:])), \
            "cloud %d (%s, %d points) alone differs from the same cloud in the packed batch" % (c, role, off[c + 1] - off[c])


@pytest.mark.parametrize("ps,stride", SS, ids=SS_IDS)
def test_scatter_clouds(host, ps, stride):
    """nsc_scatter_clouds with one workgroup per cloud (scatter_split_kernel<4, 8>, parts = 1: plain stores, no pre-fill)."""
    buf, off = family_batch(host, ps, stride)
    check_scatter(host, ps, stride, "families", buf, off, 1)
    fam = PF.sentinels(ps)
    check_scatter(host, ps, stride, "sentinels", fam.pts, fam.claims["off"], 1)


@pytest.mark.parametrize("name", PF.QUEUE_SETS)
def test_queue(host, name):
    """n certain + k uncertain points, k = 0, 1, 239, 240, 241, 480 in three placements: the drain up to 240 queued points,
    the re-stream above.  A lost uncertain point empties a pixel."""
    ps = PF.SET[name]
    fam = PF.queue(host, ps)
    encode_and_shuffle(host, ps, 4, "queue", fam.pts, fam.claims["off"], "fast")


@pytest.mark.parametrize("name,stride", PF.SPLIT_SETS, ids=["%s-s%d" % s for s in PF.SPLIT_SETS])
@pytest.mark.parametrize("batch", sorted(PF.SPLIT_BATCHES))
def test_split(host, name, stride, batch):
    """scatter_split_kernel<8, 4> with two parts per cloud (one of them empty for the one-point cloud), the global
    atomicMin merge, finish_kernel; the same clouds through nsc_scatter_clouds with parts = 2 and with parts = 1."""
    ps = PF.SET[name]
    fam = PF.split(ps, batch)
    encode_and_shuffle(host, ps, stride, "split/" + batch, fam.pts, fam.claims["off"], "split")
    check_scatter(host, ps, stride, "split/" + batch, fam.pts, fam.claims["off"], 2)
    # ... and with an empty cloud appended, which brings split_parts() to 1: scatter_split_kernel<4, 8> over the same clouds
    check_scatter(host, ps, stride, "split1/" + batch, fam.pts, PF.split_unsplit(fam), 1)


def gpu_intensity(host, ps, buf, off):
    """(raw range images, intensity images) of nsc_encode_clouds + nsc_project_intensity."""
    n, total = len(off) - 1, int(off[-1] - off[0])
    tp, to = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
    _, _, raw, _ = gpu_encode(host, ps, 4, tp, off)
    rt = torch.from_numpy(raw).cuda()
    out = torch.empty_like(rt)
    st = _lib.lib().nsc_project_intensity(_lib.ptr(tp), _lib.ptr(to), n, total, enc_params(ps), _lib.ptr(rt), _lib.ptr(out),
                                          _lib.stream_ptr(tp.device))
    assert st == 0
    torch.cuda.synchronize()
    return raw, out.cpu().numpy()


@pytest.mark.parametrize("name", PF.INTENSITY_SETS)
def test_project_intensity(host, name):
    """intensity_kernel with parts 1 and 2; ties of equal range with intensities 0, negative, +inf and NaN.  The maximum is
    order-free: the same batch with each cloud's points shuffled (three orders) gives the same words, NaN pixels included."""
    ps = PF.SET[name]
    for batch, parts in zip(PF.intensity_batches(host, ps), (1, 2)):
        buf, off = PF.guarded(ps, batch)
        n = len(off) - 1
        assert PF.intensity_parts(n, int(off[-1] - off[0])) == parts
        raw, out = gpu_intensity(host, ps, buf, off)
        for c in range(n):
            oimg, ointen = orc.project_intensity(buf[off[c]:off[c + 1]], PF.oparams(ps))
            assert np.array_equal(u32(raw[c]), u32(oimg))
            assert np.array_equal(np.isnan(out[c]), np.isnan(ointen))
            if c or n == 1:                                     # the clouds with NaN intensities leave NaN pixels
                assert np.isnan(ointen).any()
            assert np.array_equal(out[c], ointen, equal_nan=True), "intensity image of cloud %d" % c
        for seed in (1, 2, 3):
            raw2, out2 = gpu_intensity(host, ps, PF.shuffled(buf, off, seed), off)
            assert np.array_equal(u32(raw2), u32(raw))
            assert np.array_equal(u32(out2), u32(out)), "shuffling the points of each cloud changed the intensity image"
