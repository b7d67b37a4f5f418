"""Constructed point clouds for the encoder's point stage, and the table of cases that sends them down every projection path.

The point stage is everything before the square root: the range window, the column and row estimates with their
certain / uncertain decision, the exact chain, the ds_min_u32 into the image, the uncertain queue of encode_fast_kernel
with its drain and its re-stream, and the merge of a split cloud.  Dense random clouds hide a dropped, duplicated or leaked
point behind the minimum of its pixel, so the clouds here are built value by value; the oracle (orc.project with
want_idx) names every point's pixel and whether it is kept, and each family checks on the CPU that it holds what it claims.

A point's uncertainty is DETERMINED when the three host builds of csrc/nsc_math.h (tests/native/point_stage_host.cpp:
plain, NSC_TEST_APPROX_BIAS = +1 and -1) agree on it: the device's 1-ULP instructions lie between the two biased builds and
every other operation is the same IEEE operation.  Only determined points get their device flag asserted.

No GPU and no product code in this module: tests/test_point_families_cpu.py pins the families, the host restatement and the
table on the CPU, tests/test_point_paths_gpu.py runs the table on the device.
"""
import ctypes as C
import functools
import os
import subprocess
from collections import namedtuple

import numpy as np

import nsc_oracle as orc

A = 360
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-spectral-codec_amd", "csrc")
HOST_SRC = os.path.join(ROOT, "tests", "native", "point_stage_host.cpp")
BIASES = (0, 1, -1)
FQ_CAP = 240                                  # queue entries of encode_fast_kernel
STREAM_ROUND = 2 * 256                        # points per round of stream_fast<256, 2>
SPLIT_MIN_PTS, SPLIT_TARGET_WGS = 16384, 512
FAST_HSTRIDE = 64
N_BINS = 50
PREFIX_N = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1537)
GUARD = 1537                                  # guard rows before, between and after the clouds of a sentinel batch
QUEUE_K = (0, 1, 239, 240, 241, 480)
QUEUE_PLACES = ("first", "last", "lane")

# ------------------------------------------------------------------------------------------------------------------
# parameter sets
# ------------------------------------------------------------------------------------------------------------------
ParamSet = namedtuple("ParamSet", "name E fov rmin rmax f64 narrow simple s_lo_zero lean kernel4 strides")
#   narrow / simple / s_lo_zero / lean: the literal flags nsc_make_bin_params must give; kernel4: what nsc_encode_clouds
#   launches for a small batch of (N, 4) points (stride 3 always takes the fused kernel of the same E)
_DEF = (-24.8, 2.0)
SETS = (
    ParamSet("lean16", 16, _DEF, 1.0, 80.0, 1, 1, 1, 0, 1, "fast", (4, 3)),
    ParamSet("lean16_f32", 16, _DEF, 1.0, 80.0, 0, 1, 1, 0, 1, "fast", (4, 3)),
    ParamSet("min0_16", 16, _DEF, 0.0, 80.0, 1, 1, 1, 1, 0, "fused4", (4,)),
    ParamSet("clip16", 16, _DEF, 1.0, 3e5, 1, 1, 0, 0, 0, "fused4", (4, 3)),
    ParamSet("wide16", 16, (-45.0, 45.0), 1.0, 80.0, 1, 0, 1, 0, 0, "fused4", (4, 3)),
    ParamSet("edge_narrow", 16, (5.0, 30.0), 1.0, 80.0, 1, 1, 1, 0, 1, "fast", (4,)),
    ParamSet("edge_wide", 16, (-31.0, 10.0), 1.0, 80.0, 1, 0, 1, 0, 0, "fused4", (4,)),
    ParamSet("hdl64", 64, _DEF, 1.0, 80.0, 1, 1, 1, 0, 1, "fused16", (4, 3)),
    ParamSet("thin64", 64, (-2.0, 2.0), 1.0, 80.0, 1, 1, 1, 0, 1, "fused16", (4,)),
    ParamSet("e32", 32, (-25.0, 15.0), 1.0, 80.0, 0, 1, 1, 0, 1, "fused8", (4, 3)),
    ParamSet("min0_wide16", 16, (-45.0, 45.0), 0.0, 80.0, 1, 0, 1, 1, 0, "fused4", (4,)),
    ParamSet("e1", 1, _DEF, 1.0, 80.0, 1, 1, 1, 0, 1, "fused4", (4,)),
    # the rest of nsc_point_pixel x {simple, clip} x {narrow, wide} x {f64, f32 rows}
    ParamSet("wide16_f32", 16, (-45.0, 45.0), 1.0, 80.0, 0, 0, 1, 0, 0, "fused4", (4,)),
    ParamSet("clip16_f32", 16, _DEF, 1.0, 3e5, 0, 1, 0, 0, 0, "fused4", (4,)),
    ParamSet("clipwide16", 16, (-45.0, 45.0), 1.0, 3e5, 1, 0, 0, 0, 0, "fused4", (4,)),
    ParamSet("clipwide16_f32", 16, (-45.0, 45.0), 1.0, 3e5, 0, 0, 0, 0, 0, "fused4", (3,)),
)
SET = {s.name: s for s in SETS}
QUEUE_SETS = ("lean16", "lean16_f32")
SPLIT_SETS = (("lean16", 4), ("lean16", 3), ("hdl64", 4), ("clip16", 4))
INTENSITY_SETS = ("lean16", "wide16", "clip16", "hdl64")


def target_rows(ps):
    return min(ps.E, 16)


def oparams(ps):
    """The oracle's parameters of a set."""
    return orc.default_params(n_elevation=ps.E, n_bins=N_BINS, target_rows=target_rows(ps), elevation_range=ps.fov,
                              min_range=ps.rmin, max_range=ps.rmax, elev_f64=ps.f64, interpolate=1)


def fov_rad(ps):
    return float(np.deg2rad(ps.fov[0])), float(np.deg2rad(ps.fov[1]))


# ------------------------------------------------------------------------------------------------------------------
# host library (three builds)
# ------------------------------------------------------------------------------------------------------------------
class BinParams(C.Structure):
    """struct NscBinParams (csrc/nsc_math.h)"""
    _fields_ = [("emin", C.c_double), ("espan", C.c_double), ("emin_f", C.c_float), ("espan_f", C.c_float),
                ("el_scale", C.c_float), ("az_delta", C.c_float), ("el_delta", C.c_float), ("s_lo", C.c_float),
                ("s_hi", C.c_float), ("el_u_scale", C.c_float), ("el_u_bias", C.c_float), ("E", C.c_int),
                ("elev_f64", C.c_int), ("narrow_fov", C.c_int), ("simple_valid", C.c_int)]


def build_host_lib(out_dir, bias, include_dir=CSRC, tag=""):
    """g++ -O2 -ffp-contract=off -shared -fPIC, as test_binning_margins_host builds its tool."""
    so = os.path.join(str(out_dir), "point_stage_host%s_%d.so" % (tag, bias))
    cmd = ["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I" + str(include_dir), HOST_SRC, "-o", so, "-lm"]
    if bias:
        cmd.insert(5, "-DNSC_TEST_APPROX_BIAS=%d" % bias)
    subprocess.check_call(cmd)
    return so


class HostLib:
    def __init__(self, so):
        L = C.CDLL(so)
        vp, i64, ci = C.c_void_p, C.c_int64, C.c_int
        bpp = C.POINTER(BinParams)
        L.psh_make_bin_params.argtypes = [ci, C.c_double, C.c_double, C.c_float, C.c_float, ci, bpp]
        L.psh_az_edge_slack.restype = C.c_float
        for f in (L.psh_point_lean, L.psh_point_pixel):
            f.argtypes = [vp, i64, ci, bpp, vp, vp, vp]
            f.restype = None
        L.psh_point_exact.argtypes = [vp, i64, ci, bpp, vp, vp]
        L.psh_point_exact.restype = None
        assert L.psh_sizeof_bin_params() == C.sizeof(BinParams)
        self.L, self.bias = L, L.psh_bias()

    def bin_params(self, ps):
        bp = BinParams()
        lo, hi = fov_rad(ps)
        lean = self.L.psh_make_bin_params(ps.E, lo, hi, ps.rmin, ps.rmax, ps.f64, C.byref(bp))
        return bp, bool(lean)

    def _run(self, fn, pts, bp):
        pts = np.ascontiguousarray(pts, dtype=np.float32)
        n = len(pts)
        a, pix, s = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        fn(pts.ctypes.data, n, pts.shape[1], C.byref(bp), a.ctypes.data, pix.ctypes.data, s.ctypes.data)
        return a, pix, s

    def point_lean(self, pts, bp):
        return self._run(self.L.psh_point_lean, pts, bp)

    def point_pixel(self, pts, bp):
        return self._run(self.L.psh_point_pixel, pts, bp)

    def point_exact(self, pts, bp, keep):
        pts = np.ascontiguousarray(pts, dtype=np.float32)
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        pix = np.zeros(len(pts), np.int32)
        self.L.psh_point_exact(pts.ctypes.data, len(pts), pts.shape[1], C.byref(bp), keep.ctypes.data, pix.ctypes.data)
        return pix


_HOST = {}


def host_libs(out_dir):
    """The three builds, compiled once per process into ``out_dir`` (pytest's tmp_path)."""
    if "libs" not in _HOST:
        _HOST["libs"] = tuple(HostLib(build_host_lib(out_dir, b)) for b in BIASES)
        assert tuple(h.bias for h in _HOST["libs"]) == BIASES
    return _HOST["libs"]


def lean_mode(ps, stride):
    """point_bins_kernel's mode, and whether nsc_encode_clouds may take encode_fast_kernel."""
    return bool(stride == 4 and ps.E == 16 and ps.lean)


def device_flags(host, ps, stride, pts):
    """(flag the device must report, determined) per point.  nsc_debug_point_bins reports flags >> 1 of nsc_point_pixel
    (1 = column exact, 2 = row exact), and in lean mode 3 for a parked point; 0 for a dropped one."""
    per = []
    for h in host:
        bp, _ = h.bin_params(ps)
        if lean_mode(ps, stride):
            st = h.point_lean(pts, bp)[0]
            per.append(np.where(st == 2, 3, 0))
        else:
            per.append(h.point_pixel(pts, bp)[0] >> 1)
    det = (per[0] == per[1]) & (per[0] == per[2])
    return per[0].astype(np.uint8), det


# ------------------------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------------------------
def col_edge(c):
    """Ideal lower edge of column c: atan2(y, x) = c 2 pi / 360 - pi."""
    return -np.pi + np.asarray(c, dtype=np.float64) * (2.0 * np.pi / A)


def row_edge(ps, r):
    lo, hi = fov_rad(ps)
    return lo + np.asarray(r, dtype=np.float64) * (hi - lo) / ps.E


def sph(r, az, el, w=None):
    """(n, 4) float32 points at range r, azimuth az, elevation el (float64 in, rounded once); column 3 = w or 0."""
    r, az, el = np.broadcast_arrays(np.asarray(r, np.float64), np.asarray(az, np.float64), np.asarray(el, np.float64))
    out = np.zeros((r.size, 4), np.float32)
    out[:, 0] = (r * np.cos(el) * np.cos(az)).ravel()
    out[:, 1] = (r * np.cos(el) * np.sin(az)).ravel()
    out[:, 2] = (r * np.sin(el)).ravel()
    if w is not None:
        out[:, 3] = w
    return out


def centre(ps, pix, r, w=None):
    """Points at the centres of pixels ``pix`` (row * 360 + col)."""
    pix = np.asarray(pix)
    return sph(r, col_edge(pix % A + 0.5), row_edge(ps, pix // A + 0.5), w)


def sq_range(pts, clip):
    """The squared range as every kernel computes it, in numpy float32: (x x + y y) + z z, each square clipped to 1e10 on
    the clip path (range_image.py:159-162)."""
    x, y, z = (np.ascontiguousarray(pts[:, i], dtype=np.float32) for i in range(3))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        xx, yy, zz = x * x, y * y, z * z
        if clip:
            xx, yy, zz = (np.where(v > np.float32(1e10), np.float32(1e10), v) for v in (xx, yy, zz))
        return ((xx + yy) + zz).astype(np.float32)


def window_keep(pts, bp):
    """The range window restated in numpy float32 (nsc_point_pixel's two forms)."""
    with np.errstate(invalid="ignore"):
        s = sq_range(pts, not bp.simple_valid)
        fin = np.all(np.abs(pts[:, :3]) < np.inf, axis=1)
        return fin & (s >= np.float32(bp.s_lo)) & (s <= np.float32(bp.s_hi))


def project(ps, pts):
    """(raw image, pixel per point with -1 = dropped) of the oracle."""
    img, idx, kept = orc.project(np.ascontiguousarray(pts), oparams(ps), want_idx=True)
    assert kept == int((idx >= 0).sum())
    return img, idx


Family = namedtuple("Family", "name pts claims")


def _rng(name, ps):
    return np.random.default_rng([sum(map(ord, name)), sum(map(ord, ps.name))])


# ------------------------------------------------------------------------------------------------------------------
# families
# ------------------------------------------------------------------------------------------------------------------
COL_OFFS = (0.0, 3e-7, -3e-7, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4)          # rad from the ideal column edge
ROW_OFFS = (0.0, 1e-5, -1e-5, 1e-4, -1e-4, 1e-3, -1e-3)                      # bins from the ideal row edge
ROW_AZ = (17, 95, 180, 271, 44, 315)                                         # columns (centres) the row-edge points sit in
SWITCH_CLEAR = 2e-13                                                         # rad
SWITCH_CLEAR_ULPS = 64.0                                                     # float64 steps of the angle
SWITCH_RANGES = 4                                                            # points per side of a column's switch
CORNER_COLS = (1, 44, 45, 90, 179, 180, 226, 359)                           # 45, 90, 180: octant seams and axes
CORNER_OFFS = ((0.0, 0.0), (1e-6, 1e-4), (-1e-6, -1e-4), (1e-6, -1e-4))      # (rad, bins)
FAR_EL = (-1.55, -1.0, 1.0, 1.55)                                            # rad: far outside every field of view


def atan2f_boundary_distance(pts):
    """|atan2(y, x) - nearest midpoint of two neighbouring float32 values| in float64, in units of one float64 step of the
    angle (the error of a double atan2 is relative: glibc < 1, ocml 2 such steps)."""
    a = np.arctan2(pts[:, 1].astype(np.float64), pts[:, 0].astype(np.float64))
    f = a.astype(np.float32)
    mids = [0.5 * (f.astype(np.float64) + np.nextafter(f, np.float32(s)).astype(np.float64)) for s in (-10, 10)]
    return np.minimum(np.abs(a - mids[0]), np.abs(a - mids[1])) / np.spacing(np.abs(a))


@functools.lru_cache(maxsize=None)
def edges(ps):
    E = ps.E
    lo, hi = fov_rad(ps)
    # column edges: edge c between columns c - 1 and c, rows and ranges varying from point to point
    c = np.repeat(np.arange(A), len(COL_OFFS))
    o = np.tile(np.array(COL_OFFS), A)
    k = np.arange(len(c))
    cpts = sph(2.0 + ((k * 37) % 613) / 613.0 * 70.0, col_edge(c) + o, row_edge(ps, (c * 5 + k) % E + 0.5))
    # row edges 0..E (0 and E are the clamp)
    naz = len(ROW_AZ) if E <= 16 else 3
    e = np.repeat(np.arange(E + 1), len(ROW_OFFS) * naz)
    ro = np.tile(np.repeat(np.array(ROW_OFFS), naz), E + 1)
    k2 = np.arange(len(e))
    rpts = sph(2.0 + ((k2 * 53) % 587) / 587.0 * 70.0, col_edge(np.array(ROW_AZ)[k2 % naz] + 0.5), row_edge(ps, e + ro))
    # far outside the field of view
    f_el = np.repeat(np.array(FAR_EL + (lo - 0.3, hi + 0.3)), len(ROW_AZ))
    fpts = sph(3.0 + np.arange(len(f_el)) * 2.0, col_edge(np.tile(np.array(ROW_AZ), 6) + 0.5), f_el)
    # the exact chain's own switch: per column edge the last point the oracle puts in column c - 1 and the first it puts in
    # column c (bisection over the azimuth), up to 6.7e-7 rad = 3.8e-5 columns away from the ideal edge
    sc = np.repeat(np.arange(A), SWITCH_RANGES)
    k4 = np.arange(len(sc))
    sr, sel = 2.2 + ((k4 * 41) % 577) / 577.0 * 69.0, row_edge(ps, (sc * 5 + k4) % E + 0.5)
    b_lo, b_hi = np.full(len(sc), -2e-6), np.full(len(sc), 2e-6)
    for _ in range(40):
        mid = 0.5 * (b_lo + b_hi)
        up = project(ps, sph(sr, col_edge(sc) + mid, sel))[1] % A == sc
        b_hi, b_lo = np.where(up, mid, b_hi), np.where(up, b_lo, mid)
    # ... but SWITCH_CLEAR away from the switch itself: there the azimuth sits on a rounding boundary of atan2f, and which
    # way (float)atan2(double, double) falls is decided by the last bits of a double atan2 (the oracle's own limit, stated at
    # nsc_oracle_atan2f: glibc < 1 ULP; the device's ocml atan2: 2 ULP = 1e-15 rad)
    sgn = np.concatenate([-np.ones(len(sc)), np.ones(len(sc))])
    base_az, clear = col_edge(np.tile(sc, 2)) + np.concatenate([b_lo, b_hi]), np.full(2 * len(sc), SWITCH_CLEAR)
    for _ in range(10):                                      # float32 points are coarser than that in places: step on
        spts = sph(np.tile(sr, 2), base_az + sgn * clear, np.tile(sel, 2))
        near = atan2f_boundary_distance(spts) < SWITCH_CLEAR_ULPS
        if not near.any():
            break
        clear = np.where(near, clear * 4.0, clear)
    n_plain = len(cpts)
    cpts, c = np.concatenate([cpts, spts]), np.concatenate([c, sc, sc])
    # corners: a column edge and a row edge at once (both exact chains for one point)
    ce, cc, co = np.meshgrid(np.arange(E + 1), np.array(CORNER_COLS), np.arange(len(CORNER_OFFS)), indexing="ij")
    offs = np.array(CORNER_OFFS)[co.ravel()]
    k3 = np.arange(ce.size)
    xpts = sph(2.5 + ((k3 * 29) % 601) / 601.0 * 70.0, col_edge(cc.ravel()) + offs[:, 0], row_edge(ps, ce.ravel() + offs[:, 1]))
    pts = np.concatenate([cpts, rpts, fpts, xpts])
    nx = len(xpts)
    col_of = np.concatenate([c, np.full(len(rpts) + len(fpts) + nx, -1)])
    row_of = np.concatenate([np.full(len(cpts), -1), e, np.full(len(fpts) + nx, -1)])
    far = np.concatenate([np.zeros(len(cpts) + len(rpts), bool), np.ones(len(fpts), bool), np.zeros(nx, bool)])
    below = np.concatenate([np.zeros(len(cpts) + len(rpts), bool), f_el < lo, np.zeros(nx, bool)])
    switch = np.zeros(len(pts), bool)
    switch[n_plain:n_plain + len(spts)] = True
    return Family("edges", pts, dict(col_edge=col_of, row_edge=row_of, far=far, far_below=below, switch=switch))


def check_edges(ps, fam, idx):
    """Both neighbours of every column edge and of every inner row edge are hit; edges 0 and E and the far points clamp."""
    assert np.all(idx >= 0), "every edge point lies inside the range window"
    col, row, cl = idx % A, idx // A, fam.claims
    for c in range(A):
        got = set(col[cl["col_edge"] == c].tolist())
        assert got == {(c - 1) % A, c}, (ps.name, "column edge", c, got)
    for e in range(ps.E + 1):
        got = set(row[cl["row_edge"] == e].tolist())
        want = {max(e - 1, 0), min(e, ps.E - 1)}
        assert got == want, (ps.name, "row edge", e, got)
    # the switch points: no azimuth within 64 float64 steps (32 times the device's double atan2 error) of a rounding
    # boundary of atan2f, and still closer to the ideal edge than the margin of the estimate
    sw = fam.pts[cl["switch"]].astype(np.float64)
    a = np.arctan2(sw[:, 1], sw[:, 0])
    assert atan2f_boundary_distance(fam.pts[cl["switch"]]).min() >= SWITCH_CLEAR_ULPS
    off = (a + np.pi) / (2 * np.pi / A) - cl["col_edge"][cl["switch"]]
    off = np.where(off > A / 2, off - A, off)
    assert np.abs(off).max() < 4.0e-5 and np.abs(off).max() > 3.0e-5, "columns from the ideal edge"
    assert set(row[cl["far"] & cl["far_below"]].tolist()) == {0}
    assert set(row[cl["far"] & ~cl["far_below"]].tolist()) == {ps.E - 1}


@functools.lru_cache(maxsize=None)
def axes(ps):
    lo, hi = fov_rad(ps)
    tz = float(np.tan(0.5 * (lo + hi)))                     # z / rxy of an elevation inside the field of view
    L, tag = [], []

    def add(t, *p):
        for q in p:
            L.append(q)
            tag.append(t)
    for r in (5.0, 20.0):
        zi = r * tz
        for s in (1.0, -1.0):
            add("axis", (s * r, 0.0, 0.0), (0.0, s * r, 0.0), (s * r, 0.0, zi), (0.0, s * r, zi))
            add("zaxis", (0.0, 0.0, s * r), (-0.0, 0.0, s * r), (0.0, -0.0, s * r), (1e-30, 0.0, s * r))
            # x and y both denormal under a z inside the window: sxy = 0, v_rcp_f32 of the flushed max(|x|, |y|) is inf
            add("subnormal_xy", (1e-40, 5e-41, s * r), (-5e-41, 1e-40, s * r), (1e-40, -1e-40, s * r), (0.0, -1e-42, s * r))
            add("negzero", (s * r, -0.0, zi), (-0.0, s * r, zi), (s * r, -0.0, -0.0), (s * r, 0.0, -0.0), (-0.0, s * r, 0.0))
            add("z0", (s * r, 0.5 * r, 0.0), (0.3 * r, s * r, 0.0))
            add("zratio", (r, 0.5 * r, s * r * 1e-7), (0.5 * r, -r, s * r * 1e-7), (r * 1e-7, 0.5e-7 * r, s * r))
        for sx in (1.0, -1.0):
            for sy in (1.0, -1.0):
                d = r * np.sqrt(2.0) * tz
                add("seam", (sx * r, sy * r, 0.0), (sx * r, sy * r, d), (sx * r, sy * r, -0.0))
                add("ratio", (sx * r, sy * r * 1e-7, zi), (sx * r * 1e-7, sy * r, zi))
    add("origin", (0.0, 0.0, 0.0), (-0.0, 0.0, 0.0), (0.0, 0.0, -0.0), (-0.0, -0.0, -0.0))
    pts = np.zeros((len(L), 4), np.float32)
    pts[:, :3] = np.array(L, dtype=np.float64)
    return Family("axes", pts, dict(tag=np.array(tag)))


def check_axes(ps, fam, idx):
    p, tag = fam.pts, fam.claims["tag"]
    assert np.all(np.abs(p[tag == "seam", 0]) == np.abs(p[tag == "seam", 1])) and (tag == "seam").sum() == 24
    assert {(np.sign(a), np.sign(b)) for a, b in p[tag == "seam", :2]} == {(1, 1), (1, -1), (-1, 1), (-1, -1)}
    assert all(np.any(np.signbit(p[:, i]) & (p[:, i] == 0)) for i in range(3)), "-0.0 in each coordinate"
    assert np.all((p[tag == "zaxis", 0] == 0) | (p[tag == "zaxis", 0] == np.float32(1e-30))) and np.all(p[tag == "zaxis", 2] != 0)
    mn, mx = np.minimum(np.abs(p[:, 0]), np.abs(p[:, 1])), np.maximum(np.abs(p[:, 0]), np.abs(p[:, 1]))
    assert np.all(np.abs(mn[tag == "ratio"] / mx[tag == "ratio"] - 1e-7) < 1e-13)
    assert np.all(p[tag == "z0", 2] == 0)
    # the origin is inside the window only where min_range = 0; everything else is 5 or 20 m away (7.1 / 28.3 on the seams)
    assert np.all((idx[tag == "origin"] >= 0) == bool(ps.s_lo_zero)) and np.all(idx[tag != "origin"] >= 0)
    # x = y = 0: atan2(+-0, +0) = +-0 is column 180, atan2(+0, -0) = pi wraps to column 0
    sub = tag == "subnormal_xy"
    assert sub.sum() == 16 and np.all(np.abs(p[sub, :2]) < np.float32(1.17549435e-38)) and np.all(np.any(p[sub, :2] != 0, axis=1))
    assert np.all(sq_range(p[sub], False) == p[sub, 2] * p[sub, 2]) and np.all(idx[sub] >= 0)
    assert len(set((idx[sub] % A).tolist())) >= 4, "the columns of denormal x, y come from the exact chain: several of them"
    za = tag == "zaxis"
    assert np.array_equal(idx[za] % A, np.where(np.signbit(p[za, 0]), 0, 180))


def _s_targets(bp):
    f = np.float32
    t = {}
    if bp.simple_valid:          # on the clip path three clipped squares give s <= 3e10 < s_hi: the upper bound is never met
        t.update({"s_hi-": np.nextafter(f(bp.s_hi), f(0)), "s_hi": f(bp.s_hi), "s_hi+": np.nextafter(f(bp.s_hi), f(np.inf))})
    else:
        assert bp.s_hi > 3e10
    if bp.s_lo > 0:
        t.update({"s_lo-": np.nextafter(f(bp.s_lo), f(0)), "s_lo": f(bp.s_lo), "s_lo+": np.nextafter(f(bp.s_lo), f(np.inf))})
    return t


SPECIAL = (np.inf, -np.inf, np.nan, 1e-40, -1e-42, 3e25, -3e25)


def window(ps, bp):
    """``bp``: the plain host build's NscBinParams of the set (s_lo, s_hi, simple_valid)."""
    clip = not bp.simple_valid
    pix = (ps.E // 2) * A + 100
    d = centre(ps, [pix], 1.0)[0, :3].astype(np.float64)
    L, names = [], []
    for name, t in _s_targets(bp).items():
        # the radius stepped finely, then every coordinate float by float (+-8) around the best radius: s walks through
        # every value around t
        r = np.sqrt(float(t)) * (1.0 + np.linspace(-4e-7, 4e-7, 4001))
        cand = (r[:, None] * d[None, :]).astype(np.float32)
        g = np.arange(-8, 9, dtype=np.int32)
        g = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        near = cand[int(np.argmin(np.abs(sq_range(cand, clip).astype(np.float64) - float(t))))]
        cand = np.concatenate([cand, (near.view(np.int32)[None, :] + g).view(np.float32)])
        hit = np.nonzero(sq_range(cand, clip) == t)[0]
        assert len(hit), (ps.name, name, "no point along the direction gives this squared range")
        L.append(cand[hit[len(hit) // 2]])
        names.append(name)
    for v in SPECIAL:                                      # one odd coordinate, the others ordinary
        for i in range(3):
            q = np.array([3.0, -4.0, -0.5], np.float32)
            q[i] = v
            L.append(q)
            names.append("special")
    # 1e5 .. 3e25: dropped by s <= s_hi everywhere but on the clip path, where the clip decides the range and the row comes
    # from the raw z over the clipped sxy
    for q in ((1e5, 0.0, -2e4), (2e5, 1e5, -3e4), (-1e5, 1e5, 1e3), (3e25, 1.0, 1.0), (3e25, 3e25, 3e25), (1e5, -1e5, -3e25),
              (5.0, 3e25, -1e4), (-7e9, 1e5, -3e4), (1e5, 1.0001e5, 0.0), (1e5, 1e5, 1e5), (1.5e5, -1e3, -4e4)):
        L.append(np.array(q, np.float32))
        names.append("huge")
    # the origin and its neighbours: s = 0 (inside the window only with min_range = 0), the smallest s > 0, an underflow
    for q in ((0.0, 0.0, 0.0), (3.8e-23, 0.0, 0.0), (1e-30, 0.0, 1e-30), (0.0, -1e-30, 0.0), (1e-20, 1e-20, -4e-21),
              (1e-20, -1e-20, 0.0), (-1e-20, 1e-20, 3e-21), (2e-20, 1e-21, -0.0)):       # sxy > 0 but denormal
        L.append(np.array(q, np.float32))
        names.append("origin")
    pts = np.zeros((len(L), 4), np.float32)
    pts[:, :3] = np.stack(L)
    return Family("window", pts, dict(name=np.array(names), pix=pix))


def check_window(ps, bp, fam, idx):
    names, s = fam.claims["name"], sq_range(fam.pts, not bp.simple_valid)
    for name, t in _s_targets(bp).items():
        i = int(np.nonzero(names == name)[0][0])
        assert s[i] == t, (ps.name, name)
        inside = name in ("s_lo", "s_lo+", "s_hi-", "s_hi")
        assert (idx[i] >= 0) == inside, (ps.name, name, "kept" if idx[i] >= 0 else "dropped")
        if inside:
            assert idx[i] == fam.claims["pix"]
    with np.errstate(invalid="ignore"):
        odd = ~np.all(np.abs(fam.pts[:, :3]) < np.inf, axis=1)
    assert odd.sum() == 9 and np.all(idx[odd] == -1)
    huge = names == "huge"
    assert np.all(idx[huge] >= 0) if not bp.simple_valid else np.all(idx[huge] == -1)
    org = names == "origin"
    assert np.all(idx[org] >= 0) if ps.s_lo_zero else np.all(idx[org] == -1)


def uncertain_in_pixels(host, ps, stride, pix, r):
    """One point per pixel of ``pix`` that sits just inside the pixel's lower column edge, is kept, lands in that pixel
    and is determined-uncertain (at this stride's mode); ranges r."""
    pix, r = np.asarray(pix), np.broadcast_to(np.asarray(r, np.float64), np.shape(pix))
    out = np.zeros((len(pix), 4), np.float32)
    todo = np.ones(len(pix), bool)
    for off in (1.0e-6, 7e-7, 1.3e-6, 5e-7, 1.6e-6, 3e-7):
        cand = sph(r, col_edge(pix % A) + off, row_edge(ps, pix // A + 0.5))
        _, idx = project(ps, cand)
        fl, det = device_flags(host, ps, stride, cand)
        ok = todo & (idx == pix) & det & (fl != 0)
        out[ok], todo = cand[ok], todo & ~ok
        if not todo.any():
            return out
    raise AssertionError("%s: no determined-uncertain point for pixels %s" % (ps.name, pix[todo][:8]))


def certain_in_pixels(host, ps, stride, pix, r):
    cand = centre(ps, pix, r)
    _, idx = project(ps, cand)
    fl, det = device_flags(host, ps, stride, cand)
    assert np.all(idx == np.asarray(pix)) and np.all(det & (fl == 0)), "a pixel-centre point is not determined-certain"
    return cand


def _ulp_group(base, m):
    """m points around ``base`` (every coordinate moved in up to 12 small steps either way) whose squared ranges are m CONSECUTIVE float32 values,
    ascending."""
    d = np.arange(-12, 13, dtype=np.int32)
    g = np.stack(np.meshgrid(d, d, d, indexing="ij"), -1).reshape(-1, 3)
    assert np.all(base[:3] != 0)
    cand = np.zeros((len(g), 4), np.float32)
    # a coordinate's step: as many floats as move its square by about a quarter of one float of s (at least one)
    b64 = np.abs(base[:3].astype(np.float64))
    ulp_s = float(np.spacing(sq_range(base[None, :], False)[0]))
    unit = np.maximum(1, (0.25 * ulp_s / (2.0 * b64 * np.spacing(np.abs(base[:3])).astype(np.float64))).astype(np.int32))
    cand[:, :3] = (base[:3].view(np.int32)[None, :] + g * unit[None, :]).view(np.float32)    # bits + 1 = the next float away from zero
    bits, first = np.unique(sq_range(cand, False).view(np.uint32), return_index=True)
    for a in range(len(bits) - m + 1):
        if int(bits[a + m - 1]) - int(bits[a]) == m - 1:
            return cand[first[a:a + m]]
    raise AssertionError("no run of %d consecutive squared ranges" % m)


def min_wins(host, ps, stride):
    """Pixels with 2..9 points whose squared ranges differ by single ULPs (exact duplicates of the minimum included), pixels
    whose minimum is a determined-uncertain point among determined-certain ones, and the reverse."""
    E = ps.E
    L, kind, pixs = [], [], []
    for m in range(2, 10):                                  # m points, then a duplicate of the closest
        pix = ((m * 3) % E) * A + (29 * m) % A
        g = _ulp_group(centre(ps, [pix], 6.0 + 3.0 * m)[0], m)
        g = np.concatenate([g[[0]], g[::-1]])                               # a duplicate of the minimum first, the minimum last
        L.append(g)
        kind += ["ulps"] * len(g)
        pixs += [pix] * len(g)
    npix = 6
    for j in range(npix):                                   # uncertain minimum among certain points
        pix = ((5 * j + 1) % E) * A + (61 * j + 7) % A
        L += [certain_in_pixels(host, ps, stride, [pix] * 3, [20.0 + j, 21.0 + j, 30.0]),
              uncertain_in_pixels(host, ps, stride, [pix], [19.5 + j])]
        kind += ["cert_loses"] * 3 + ["unc_wins"]
        pixs += [pix] * 4
    for j in range(npix):                                   # certain minimum among uncertain points
        pix = ((5 * j + 2) % E) * A + (67 * j + 12) % A
        L += [uncertain_in_pixels(host, ps, stride, [pix] * 3, [20.0 + j, 21.0 + j, 30.0]),
              certain_in_pixels(host, ps, stride, [pix], [19.5 + j])]
        kind += ["unc_loses"] * 3 + ["cert_wins"]
        pixs += [pix] * 4
    return Family("min_wins", np.concatenate(L), dict(kind=np.array(kind), pix=np.array(pixs)))


def check_min_wins(host, ps, stride, fam, img, idx):
    kind, pix, pts = fam.claims["kind"], fam.claims["pix"], fam.pts
    assert np.array_equal(idx, pix), "every point lands in the pixel it was built for"
    s = sq_range(pts, False)
    fl, det = device_flags(host, ps, stride, pts)
    flat = img.reshape(-1)
    for p in np.unique(pix[kind == "ulps"]):
        m = (pix == p)
        sv = np.sort(s[m])
        assert sv[0] == sv[1], "the minimum is there twice"
        assert np.array_equal(np.diff(sv.view(np.uint32).astype(np.int64)), [0] + [1] * (len(sv) - 2)), "single-ULP steps"
        assert flat[p] == np.sqrt(sv[0])
    for win, lose, wf in (("unc_wins", "cert_loses", True), ("cert_wins", "unc_loses", False)):
        for i in np.nonzero(kind == win)[0]:
            others = (pix == pix[i]) & (kind == lose)
            assert others.sum() == 3 and np.all(s[others] > s[i]) and flat[pix[i]] == np.sqrt(s[i])
            assert det[i] and np.all(det[others]) and (fl[i] != 0) == wf and np.all((fl[others] != 0) == (not wf))


@functools.lru_cache(maxsize=None)
def census_order(ps):
    """(pixel order, base range per position): every pixel once, shuffled, distinct ranges in [4.4, 60]."""
    npix = ps.E * A
    rng = _rng("census", ps)
    return rng.permutation(npix), 4.4 + 55.6 * rng.permutation(npix) / npix


def census_ext(ps, n, scale=1.0, grow=0.01):
    """n points: position j sits at the centre of pixel order[j mod npix] at range base * scale * (1 + grow (j div npix)):
    the first E x 360 positions are the census (one point per pixel), later copies never win a pixel."""
    order, base = census_order(ps)
    npix = len(order)
    j = np.arange(n)
    return centre(ps, order[j % npix], base[j % npix] * scale * (1.0 + grow * (j // npix)),
                  w=((j * 7) % 97) / 97.0)


@functools.lru_cache(maxsize=None)
def census(ps):
    return Family("census", census_ext(ps, ps.E * A), dict())


def check_census(ps, fam, img, idx):
    npix = ps.E * A
    assert len(fam.pts) == npix and np.array_equal(np.sort(idx), np.arange(npix)), "exactly one point per pixel"
    s = sq_range(fam.pts, False)
    assert len(np.unique(s)) == npix and np.all(img > 0)
    assert np.array_equal(img.reshape(-1)[idx], np.sqrt(s))


def guard_rows(ps):
    """Points on the pixels of the first census positions at a QUARTER of their range: whatever reads one of them into a
    neighbouring cloud lowers a pixel of that cloud, or fills one it leaves empty."""
    return census_ext(ps, GUARD, scale=0.25)


def guarded(ps, clouds):
    """Packed buffer: guard rows, the clouds, guard rows (padding inside the same allocation); offsets start behind the
    front guard.  Returns (buffer, offsets)."""
    g = guard_rows(ps)
    sizes = [len(c) for c in clouds]
    off = (len(g) + np.concatenate([[0], np.cumsum(sizes)])).astype(np.int64)
    return np.ascontiguousarray(np.concatenate([g] + [c for c in clouds if len(c)] + [g])), off


@functools.lru_cache(maxsize=None)
def sentinels(ps):
    """The prefix-census clouds in one batch, a guard CLOUD between any two of them (the rows before and after every
    census cloud hit its pixels at smaller range), empty clouds after every third."""
    clouds, role = [], []
    empty = np.zeros((0, 4), np.float32)
    for i, n in enumerate(PREFIX_N):
        if i:
            clouds.append(guard_rows(ps))
            role.append("guard")
        if i % 3 == 1:
            clouds.append(empty)
            role.append("empty")
        clouds.append(census_ext(ps, n))
        role.append("prefix")
        if i % 3 == 2:
            clouds.append(empty)
            role.append("empty")
    buf, off = guarded(ps, clouds)
    return Family("sentinels", buf, dict(off=off, role=tuple(role)))


def check_sentinels(ps, fam):
    buf, off, role = fam.pts, fam.claims["off"], fam.claims["role"]
    assert [int(off[i + 1] - off[i]) for i, r in enumerate(role) if r == "prefix"] == list(PREFIX_N)
    assert off[0] == GUARD and len(buf) == off[-1] + GUARD and role.count("empty") >= 5
    _, idx = project(ps, buf)
    r = np.sqrt(sq_range(buf, False))
    assert np.all(idx >= 0)
    for c, ro in enumerate(role):
        if ro != "prefix":
            continue
        a, b = int(off[c]), int(off[c + 1])
        own = dict(zip(idx[a:b].tolist(), r[a:b].tolist()))
        for lo, hi in ((a - STREAM_ROUND, a), (b, b + STREAM_ROUND)):      # one round of the stream on either side
            assert lo >= 0 and hi <= len(buf)
            for p, rr in zip(idx[lo:hi].tolist(), r[lo:hi].tolist()):
                assert rr < own.get(p, np.inf), "a neighbouring row would not change the cloud's image"


def queue_layout(k, place):
    """(cloud size, indices of the k uncertain points).  first: anywhere in the first round of the stream; last: in the last,
    partial round of three; lane: in the slots of lane 37 alone, one per half-round."""
    rng = np.random.default_rng([k, QUEUE_PLACES.index(place)])
    if place == "first":
        return 1537, np.sort(rng.permutation(STREAM_ROUND)[:k])
    if place == "last":
        return 2 * STREAM_ROUND + 500, 2 * STREAM_ROUND + np.sort(rng.permutation(500)[:k])
    return max(k, 1) * 256 + 57, 37 + 256 * np.arange(k)


def queue(host, ps):
    """n determined-certain points (rows 0..7) plus exactly k determined-uncertain ones, each the only point of a pixel of
    rows 8..15.  One cloud per (k, placement); returns the packed batch."""
    assert ps.name in QUEUE_SETS
    clouds, meta = [], []
    upix = (8 + np.arange(480) % 8) * A + (np.arange(480) // 8) * 6 + 1
    assert len(np.unique(upix)) == 480
    unc_all = uncertain_in_pixels(host, ps, 4, upix, 3.0 + 0.05 * np.arange(480))
    for k in QUEUE_K:
        for place in QUEUE_PLACES:
            n, at = queue_layout(k, place)
            j = np.arange(n)
            pts = centre(ps, (j % 8) * A + (j * 11) % A, 5.0 + ((j * 13) % 977) / 977.0 * 60.0)
            pts[at] = unc_all[:k]
            clouds.append(pts)
            meta.append((k, place, at))
    pts, off = guarded(ps, clouds)
    return Family("queue", pts, dict(off=off, meta=tuple(meta)))


def check_queue(host, ps, fam):
    pts, off = fam.pts, fam.claims["off"]
    fl, det = device_flags(host, ps, 4, pts)
    assert np.all(det), "an undetermined point in the queue family: change the generator's offsets"
    img_idx = project(ps, pts)[1]
    assert np.all(img_idx >= 0)
    for c, (k, place, at) in enumerate(fam.claims["meta"]):
        a, b = int(off[c]), int(off[c + 1])
        unc = np.nonzero(fl[a:b] != 0)[0]
        assert len(unc) == k and np.array_equal(unc, at), (k, place)
        pix = img_idx[a:b]
        assert len(np.unique(pix[unc])) == k and not np.intersect1d(pix[unc], np.delete(pix, unc)).size
        if place == "first":
            assert np.all(at < STREAM_ROUND)
        elif place == "last":
            assert -(-(b - a) // STREAM_ROUND) == 3 and np.all(at >= 2 * STREAM_ROUND)
        else:
            assert np.all(at % 256 == 37)


def split_parts(n_clouds, total_points):
    if n_clouds <= 0 or n_clouds >= SPLIT_TARGET_WGS:
        return 1
    s = min(-(-SPLIT_TARGET_WGS // n_clouds), (total_points // n_clouds) // SPLIT_MIN_PTS)
    return 1 if s < 2 else s


SPLIT_BATCHES = {"1_0_98303": (1, 0, 98303), "32768": (32768,)}


def split_special(n, parts):
    chunk = -(-n // parts)
    return sorted({0, chunk - 1, chunk, n - 1} & set(range(n)))


@functools.lru_cache(maxsize=None)
def split(ps, batch):
    """Clouds that nsc_encode_clouds splits in two parts; the points at 0, chunk - 1, chunk and n - 1 are the only points of
    their cloud closer than the census range of their pixel."""
    sizes = SPLIT_BATCHES[batch]
    parts = split_parts(len(sizes), sum(sizes))
    assert parts == 2
    order, base = census_order(ps)
    clouds = []
    for n in sizes:
        if n == 1:                                          # a pixel the big cloud holds at a larger range
            clouds.append(centre(ps, [order[7]], [base[7] * 0.9]))
            continue
        pts = census_ext(ps, n, grow=0.0005)
        for i in split_special(n, parts):
            pts[i] = centre(ps, [order[i % len(order)]], [base[i % len(order)] * 0.5])[0]
        clouds.append(pts)
    buf, off = guarded(ps, clouds)
    return Family("split", buf, dict(off=off, parts=parts))


def split_unsplit(fam):
    """The offsets of a split batch with as many empty clouds appended as bring the average cloud below 2 x SPLIT_MIN_PTS:
    the same clouds, the same chunk-boundary specials, but split_parts() = 1 (scatter_split_kernel<4, 8>)."""
    off = fam.claims["off"]
    while split_parts(len(off) - 1, int(off[-1] - off[0])) > 1:
        off = np.concatenate([off, off[-1:]])
    return off


def check_split(ps, fam):
    buf, off, parts = fam.pts, fam.claims["off"], fam.claims["parts"]
    assert split_parts(len(off) - 1, int(off[-1] - off[0])) == parts == 2
    _, idx = project(ps, buf)
    r = np.sqrt(sq_range(buf, False))
    for c in range(len(off) - 1):
        a, b = int(off[c]), int(off[c + 1])
        if b - a < 2:
            continue
        for i in split_special(b - a, parts):
            same = idx[a:b] == idx[a + i]
            assert np.sum(r[a:b][same] <= r[a + i]) == 1, "the special point is the unique minimum of its pixel"
    assert np.all(r[:GUARD] < 16) and np.all(r[-GUARD:] < 16) and r[off[0]:off[-1]].min() >= 2.0


def intensity(host, ps):
    """(clouds, offsets): the edges and min_wins points with intensities; closest points of equal range with different
    intensities, 0, negative, +inf and NaN among them; one 8 192-point cloud (nsc_project_intensity with parts = 2)."""
    rng = _rng("intensity", ps)
    a = np.concatenate([edges(ps).pts, min_wins(host, ps, 4).pts])
    a[:, 3] = rng.random(len(a)).astype(np.float32)
    base = centre(ps, (np.arange(40) % ps.E) * A + (np.arange(40) * 9 + 2), 10.0 + np.arange(40) * 0.5)
    odd = np.array([0.0, -1.0, np.inf, np.nan, 0.25, 0.75, -0.0, 1e-40], np.float32)
    ties = []
    for j in range(40):                                     # 2..5 copies of one point, intensities differ
        m = 2 + j % 4
        g = np.repeat(base[[j]], m, 0)
        g[:, 3] = rng.random(m)
        if j < 24:
            g[j % m, 3] = odd[j % 8]
        if 24 <= j < 30:                                    # only non-positive / NaN intensities in the pixel
            g[:, 3] = np.array([0.0, -1.0, -0.0, np.nan, -np.inf], np.float32)[(j + np.arange(m)) % (4 if j % 2 else 3)]
        ties.append(g)
    b = np.concatenate(ties + [a[::7]])
    big = census_ext(ps, 8192)
    big[:, 3] = rng.random(8192).astype(np.float32)
    big[::50, 3] = odd[np.arange(len(big[::50])) % 8]
    return [a, b, big]


def intensity_batches(host, ps):
    """The batches nsc_project_intensity is given: all three clouds (parts = 1), the 8 192-point cloud alone (parts = 2)."""
    clouds = intensity(host, ps)
    return [clouds, clouds[2:]]


def intensity_parts(n_clouds, total_points):
    if n_clouds >= 1024:
        return 1
    return max(1, min(-(-2048 // n_clouds), (total_points // n_clouds) // 4096))


# ------------------------------------------------------------------------------------------------------------------
# dispatch, restated; the table
# ------------------------------------------------------------------------------------------------------------------
ENC_PATH = {"fast": 1, "fused4": 2, "fused8": 2, "fused16": 2, "split": 3}          # NSC_ENC_PATH_*


def kernel_for(ps, bp_lean, stride, n_clouds, total_points, B=N_BINS):
    """encode_path() and the launcher of nsc_encode_clouds; ``bp_lean`` = nsc_lean_ok of the set."""
    if split_parts(n_clouds, total_points) > 1:
        return "split"
    if stride == 4 and ps.E == 16 and target_rows(ps) == 16 and B <= FAST_HSTRIDE and bp_lean:
        return "fast"
    return "fused16" if ps.E > 32 else "fused8" if ps.E > 16 else "fused4"


Case = namedtuple("Case", "family set stride entry kernel")
POINT_FAMILIES = ("edges", "axes", "window", "min_wins", "census")


@functools.lru_cache(maxsize=None)
def cases():
    """(family, parameter set, stride, entry point, kernel).  entry: bins = nsc_debug_point_bins, clouds =
    nsc_encode_clouds, scatter = nsc_scatter_clouds, intensity = nsc_project_intensity."""
    t = []
    for ps in SETS:
        for stride in ps.strides:
            small = ps.kernel4 if stride == 4 else {"fast": "fused4"}.get(ps.kernel4, ps.kernel4)
            for f in bins_families(ps, stride):
                t.append(Case(f, ps.name, stride, "bins", "bins_lean" if lean_mode(ps, stride) else "bins_pixel"))
            for f in POINT_FAMILIES:
                t.append(Case(f, ps.name, stride, "clouds", small))
                t.append(Case(f, ps.name, stride, "scatter", "scatter4x8"))
            t.append(Case("sentinels", ps.name, stride, "clouds", small))
            t.append(Case("sentinels", ps.name, stride, "scatter", "scatter4x8"))
    for name in QUEUE_SETS:
        t.append(Case("queue", name, 4, "clouds", "fast"))
    for name, stride in SPLIT_SETS:
        for b in SPLIT_BATCHES:
            t.append(Case("split/" + b, name, stride, "clouds", "split"))
            t.append(Case("split/" + b, name, stride, "scatter", "scatter8x4"))
            t.append(Case("split/" + b, name, stride, "scatter", "scatter4x8"))      # with an empty cloud appended: parts = 1
    for name in INTENSITY_SETS:
        t.append(Case("intensity", name, 4, "intensity", "intensity"))
    return tuple(t)


REQUIRED = tuple(
    ["lean_pair/half0", "lean_pair/half1", "lean_flags/overflow+uncertain", "lean_flags/overflow+certain"]
    + ["point_pixel/%s/%s/%s" % (a, b, c) for a in ("simple", "clip") for b in ("narrow", "wide") for c in ("f64", "f32")]
    + ["exact/col", "exact/row", "exact/both", "queue/drain", "queue/restream", "stream/T1", "stream/T2", "stream/T3",
       "stream/T4+", "scatter_range/stride4", "scatter_range/stride3", "merge/parts1", "merge/parts2", "merge/empty_part",
       "intensity/parts1", "intensity/parts2", "bins/lean", "bins/pixel"])


def coverage(host):
    """The branches the table reaches, from the restated dispatch and the host restatement's flags."""
    have = set()
    h0 = host[0]
    for c in cases():
        ps = SET[c.set]
        bp, lean = h0.bin_params(ps)
        combo = "point_pixel/%s/%s/%s" % ("simple" if bp.simple_valid else "clip", "narrow" if bp.narrow_fov else "wide",
                                          "f64" if bp.elev_f64 else "f32")
        if c.kernel in ("fused4", "fused8", "fused16", "split", "scatter4x8", "scatter8x4", "bins_pixel", "intensity"):
            have.add(combo)                                  # scatter_point / intensity_kernel / point_bins_kernel
        if c.kernel not in ("fast", "bins_lean", "bins_pixel", "intensity"):
            have.add("scatter_range/stride%d" % c.stride)
        if c.entry == "bins":
            have.add("bins/lean" if c.kernel == "bins_lean" else "bins/pixel")
            pts = family_points(host, ps, c.stride, c.family)
            fl, det = device_flags(host, ps, c.stride, pts)
            if c.kernel == "bins_lean":
                # point_bins_kernel puts point i in half i & 1 of nsc_point_lean_pair: a half counts when it holds a
                # determined-uncertain AND a determined-certain kept point of this family
                kept = project(ps, pts)[1] >= 0
                for h in (0, 1):
                    half = (np.arange(len(pts)) & 1) == h
                    if np.any(half & det & (fl != 0)) and np.any(half & det & (fl == 0) & kept):
                        have.add("lean_pair/half%d" % h)
            elif c.family == "edges":
                have |= {"exact/" + {1: "col", 2: "row", 3: "both"}[int(v)] for v in np.unique(fl[det]) if v}
        if c.kernel == "fast" and c.family == "sentinels":
            role, off = sentinels(ps).claims["role"], sentinels(ps).claims["off"]
            sizes = [int(off[i + 1] - off[i]) for i, r in enumerate(role) if r == "prefix"]
            have |= {"stream/T%s" % (t if t < 4 else "4+") for t in {-(-n // STREAM_ROUND) for n in sizes}}
        if c.kernel == "fast" and c.family == "queue":
            fam = queue(host, ps)
            fl, det = device_flags(host, ps, 4, fam.pts)
            for i in range(len(fam.claims["off"]) - 1):
                a, b = int(fam.claims["off"][i]), int(fam.claims["off"][i + 1])
                k = int((det[a:b] & (fl[a:b] != 0)).sum())                # what the stream parks
                have.add("queue/drain" if k <= FQ_CAP else "queue/restream")
                if k > FQ_CAP:                                            # the cold loop then meets both kinds of point
                    have.add("lean_flags/overflow+uncertain")
                    if np.any(det[a:b] & (fl[a:b] == 0)):
                        have.add("lean_flags/overflow+certain")
        if c.entry == "scatter":
            have.add("merge/parts1" if c.kernel == "scatter4x8" else "merge/parts2")
        if c.kernel == "split":
            have.add("merge/parts2")
            if c.family == "split/1_0_98303":
                have.add("merge/empty_part")
        if c.entry == "intensity":
            for batch in intensity_batches(host, ps):
                have.add("intensity/parts%d" % intensity_parts(len(batch), sum(len(x) for x in batch)))
    return have


def coverage_gaps(host):
    return sorted(set(REQUIRED) - coverage(host))


# ------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------
def pack(clouds):
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(clouds, 0)), off


def shuffled(pts, off, seed=1):
    rng, out = np.random.default_rng(seed), pts.copy()
    for c in range(len(off) - 1):
        a, b = int(off[c]), int(off[c + 1])
        out[a:b] = pts[a:b][rng.permutation(b - a)]
    return out


def scatter_words(ps, bp, pts, off):
    """What nsc_scatter_clouds must leave: per cloud and pixel the float32 bits of the minimum, over the oracle's pixels, of
    (x x + y y) + z z in float32 (clipped squares on the clip path); 0xffffffff for an empty pixel."""
    out = np.full((len(off) - 1, ps.E * A), 0xffffffff, np.uint32)
    s = sq_range(pts, not bp.simple_valid).view(np.uint32)      # s >= 0: the order of the bits is the order of the values
    _, idx = project(ps, pts)
    for c in range(len(off) - 1):
        a, b = int(off[c]), int(off[c + 1])
        keep = idx[a:b] >= 0
        np.minimum.at(out[c], idx[a:b][keep], s[a:b][keep])
    return out.reshape(len(off) - 1, ps.E, A)


def bar(ref):
    """The project's descriptor bar against the oracle."""
    return 1e-6 * np.abs(ref) + 1e-9


_FAMS = {}


def point_families(host, ps, stride):
    """{name: Family} of the five families that are plain point lists, built once per (set, stride)."""
    key = (ps.name, stride)
    if key not in _FAMS:
        bp, _ = host[0].bin_params(ps)
        _FAMS[key] = {"edges": edges(ps), "axes": axes(ps), "window": window(ps, bp), "min_wins": min_wins(host, ps, stride),
                      "census": census(ps)}
        for f in _FAMS[key].values():
            f.pts.setflags(write=False)
    return _FAMS[key]


def bins_families(ps, stride):
    """The families nsc_debug_point_bins is given at (set, stride): every one the set has."""
    names = list(POINT_FAMILIES) + ["sentinels"]
    if stride == 4 and ps.name in QUEUE_SETS:
        names.append("queue")
    if (ps.name, stride) in SPLIT_SETS:
        names += ["split/" + b for b in SPLIT_BATCHES]
    if stride == 4 and ps.name in INTENSITY_SETS:
        names.append("intensity")
    return names


def family_points(host, ps, stride, family):
    """All points of a family as one (n, 4) array (guard rows of the packed ones included)."""
    if family in POINT_FAMILIES:
        return point_families(host, ps, stride)[family].pts
    if family == "sentinels":
        return sentinels(ps).pts
    if family == "queue":
        return queue(host, ps).pts
    if family == "intensity":
        return np.concatenate(intensity(host, ps))
    assert family.startswith("split/")
    return split(ps, family[6:]).pts


def violations(h, ps, pts, idx):
    """Where one host build disagrees with the oracle: a keep decision, the pixel nsc_point_pixel returns (its exact chain
    included), or a pixel the lean estimate calls certain.  Returns the indices."""
    bp, lean = h.bin_params(ps)
    fl, pix, _ = h.point_pixel(pts, bp)
    bad = ((fl != 0) != (idx >= 0)) | ((fl != 0) & (pix != idx))
    if lean:
        st, lpix, _ = h.point_lean(pts, bp)
        bad |= ((st != 0) != (idx >= 0)) | ((st == 1) & (lpix != idx))
    return np.nonzero(bad)[0]
