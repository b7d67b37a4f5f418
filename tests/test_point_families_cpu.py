"""The constructed clouds of tests/point_families.py, the host restatement of csrc/nsc_math.h and the table of cases, pinned
without a GPU: the oracle's pixel is nsc_point_exact, its keep decision the range window in numpy float32; a host estimate
that claims certainty carries the oracle's pixel in all three builds; every family holds what it claims; the table reaches
every branch; and three mutants of the header each fail the family that is there to catch them."""
import ctypes as C
import os

import numpy as np
import pytest

import point_families as PF
from point_families import A, SETS

IDS = [s.name for s in SETS]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return PF.host_libs(tmp_path_factory.mktemp("point_stage_host"))


@pytest.mark.parametrize("ps", SETS, ids=IDS)
def test_parameter_table(host, ps):
    """The literal flags of the table, in all three builds, and the kernel nsc_encode_clouds_path names."""
    from neural_spectral_codec_amd import build, _lib
    build.build_hip()
    for h in host:
        bp, lean = h.bin_params(ps)
        assert (bp.narrow_fov, bp.simple_valid, int(bp.s_lo == 0.0), int(lean)) == (ps.narrow, ps.simple, ps.s_lo_zero, ps.lean)
        assert bp.E == ps.E and bp.elev_f64 == ps.f64 and bp.s_lo < bp.s_hi
        assert abs(np.sqrt(bp.s_hi) - ps.rmax) < 1e-4 * ps.rmax and (bp.s_hi < 1e10) == bool(ps.simple)
    p = _lib.EncParams()
    _lib.lib().nsc_enc_default_params(C.byref(p))
    p.n_elevation, p.target_rows, p.n_bins, p.elev_f64 = ps.E, PF.target_rows(ps), PF.N_BINS, ps.f64
    p.elev_min_rad, p.elev_max_rad = PF.fov_rad(ps)
    p.min_range, p.max_range = ps.rmin, ps.rmax
    for stride in (4, 3):
        k = PF.kernel_for(ps, ps.lean, stride, 20, 20 * 3000)
        assert k == (ps.kernel4 if stride == 4 else {"fast": "fused4"}.get(ps.kernel4, ps.kernel4))
        assert _lib.lib().nsc_encode_clouds_path(20, 20 * 3000, stride, p) == PF.ENC_PATH[k]
    assert _lib.lib().nsc_encode_clouds_path(1, 32768, 4, p) == PF.ENC_PATH["split"] == PF.ENC_PATH[PF.kernel_for(ps, ps.lean, 4, 1, 32768)]


def _all_points(host, ps):
    for stride in ps.strides:
        for name, fam in PF.point_families(host, ps, stride).items():
            yield stride, name, fam.pts
    yield 4, "sentinels", PF.sentinels(ps).pts
    if ps.name in PF.QUEUE_SETS:
        yield 4, "queue", PF.queue(host, ps).pts
    for name, stride in PF.SPLIT_SETS:
        if name == ps.name and stride == ps.strides[0]:
            for b in PF.SPLIT_BATCHES:
                yield stride, "split/" + b, PF.split(ps, b).pts


@pytest.mark.parametrize("ps", SETS, ids=IDS)
def test_oracle_is_the_exact_chain_and_certain_estimates_are_right(host, ps):
    for stride, name, pts in _all_points(host, ps):
        _, idx = PF.project(ps, pts)
        for h in host:
            bp, _ = h.bin_params(ps)
            keep = PF.window_keep(pts, bp)
            assert np.array_equal(keep, idx >= 0), (name, "keep decision of the oracle != the window in numpy float32")
            assert np.array_equal(h.point_exact(pts, bp, keep), idx), (name, "oracle pixel != nsc_point_exact")
            bad = PF.violations(h, ps, pts, idx)
            assert len(bad) == 0, (name, h.bias, bad[:5], pts[bad[:5]])
            fl, pix, s = h.point_pixel(pts, bp)
            assert np.array_equal(s[keep].view(np.uint32), PF.sq_range(pts, not bp.simple_valid)[keep].view(np.uint32))


@pytest.mark.parametrize("ps", SETS, ids=IDS)
def test_family_claims(host, ps, capsys):
    bp, _ = host[0].bin_params(ps)
    for stride in ps.strides:
        fams = PF.point_families(host, ps, stride)
        img = {n: PF.project(ps, f.pts) for n, f in fams.items()}
        PF.check_edges(ps, fams["edges"], img["edges"][1])
        PF.check_axes(ps, fams["axes"], img["axes"][1])
        PF.check_window(ps, bp, fams["window"], img["window"][1])
        PF.check_min_wins(host, ps, stride, fams["min_wins"], *img["min_wins"])
        PF.check_census(ps, fams["census"], *img["census"])
        for n, f in fams.items():
            fl, det = PF.device_flags(host, ps, stride, f.pts)
            share = 1.0 - det.mean()
            with capsys.disabled():
                print("\n  %s stride %d %-8s: %5d points, undetermined %.2f %%, exact-path (determined) %.2f %%"
                      % (ps.name, stride, n, len(f.pts), 100 * share, 100 * (det & (fl != 0)).mean()), end="")
            if n == "edges":
                assert share < 0.10
    PF.check_sentinels(ps, PF.sentinels(ps))


@pytest.mark.parametrize("name", PF.QUEUE_SETS)
def test_queue_condition(host, name):
    """No undetermined point, exactly k uncertain ones where the layout puts them, each alone in its pixel."""
    PF.check_queue(host, PF.SET[name], PF.queue(host, PF.SET[name]))


@pytest.mark.parametrize("name,stride", PF.SPLIT_SETS)
def test_split_claims(name, stride):
    for b in PF.SPLIT_BATCHES:
        fam = PF.split(PF.SET[name], b)
        PF.check_split(PF.SET[name], fam)
        off = PF.split_unsplit(fam)
        assert PF.split_parts(len(off) - 1, int(off[-1] - off[0])) == 1 and len(off) == len(fam.claims["off"]) + 1
        assert np.array_equal(off[:-1], fam.claims["off"]) and off[-1] == off[-2]


def test_intensity_family(host):
    for name in PF.INTENSITY_SETS:
        clouds = PF.intensity(host, PF.SET[name])
        assert len(clouds[2]) == 8192
        assert [PF.intensity_parts(len(b), sum(map(len, b))) for b in PF.intensity_batches(host, PF.SET[name])] == [1, 2]
        w = np.concatenate(clouds)[:, 3]
        assert np.isnan(w).any() and np.isposinf(w).any() and (w < 0).any() and (w == 0).any()
        b = clouds[1]
        same = np.all(b[1:, :3] == b[:-1, :3], axis=1) & (b[1:, 3] != b[:-1, 3])
        assert same.sum() >= 40, "closest points of equal range with different intensities"


def test_table_reaches_every_branch(host):
    assert PF.coverage_gaps(host) == []
    assert set(PF.REQUIRED) <= PF.coverage(host)
    assert {c.set for c in PF.cases()} == set(PF.SET) and {c.stride for c in PF.cases()} == {3, 4}


MUTANTS = {
    # name: (text in csrc/nsc_math.h, replacement, family, parameter set)
    "az_delta_without_edge_slack": ("bp.az_delta = nsc_az_edge_slack() + NSC_AZ_EST_ERR;", "bp.az_delta = NSC_AZ_EST_ERR;",
                                    "edges", "lean16"),
    "narrow_row_without_sxy_gt_0": ("return clear && (sxy >= NSC_F32_MIN_NORMAL);", "return clear;",
                                    "axes", "min0_16"),
    "window_lt_s_hi": ("s <= bp.s_hi", "s < bp.s_hi", "window", "lean16"),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutants_of_the_host_restatement_fail_their_family(host, tmp_path, mutant):
    old, new, family, set_name = MUTANTS[mutant]
    src = open(os.path.join(PF.CSRC, "nsc_math.h")).read()
    assert old in src, "the mutated line is gone from csrc/nsc_math.h: restate the mutant"
    with open(tmp_path / "nsc_math.h", "w") as f:
        f.write(src.replace(old, new))
    ps = PF.SET[set_name]
    pts = PF.point_families(host, ps, 4)[family].pts
    _, idx = PF.project(ps, pts)
    assert len(PF.violations(host[0], ps, pts, idx)) == 0
    caught = {}
    for bias in PF.BIASES:
        m = PF.HostLib(PF.build_host_lib(tmp_path, bias, include_dir=tmp_path, tag="_" + mutant))
        caught[bias] = len(PF.violations(m, ps, pts, idx))
    print("%s: points of %s that disagree with the oracle, by build: %s" % (mutant, family, caught))
    # Only the plain build is asserted: a mutant that is wrong there is wrong, whatever the biased builds say.  The margin
    # mutant shows only at the exact chain's own switch points and only where the estimate errs upwards (plain and +1
    # builds), so it cannot be asked of the -1 build; the other two mutants show in all three (printed above)
    assert caught[0] > 0, "the %s family does not notice the mutant" % family
