"""Stage-2 verification without a GPU: the float64 restatement (tests/gicp_restatement.py) recovers known relative
poses of ray-cast revisits and rejects scans of another world; the nsc_gicp_* C ABI validates its arguments on the
host."""
import ctypes as C

import numpy as np
import pytest

import gicp_restatement as G
from neural_spectral_codec_amd import synth

# GICP is local: from the identity it converges for ~1 m of offset or ~10 deg of yaw alone (calibrated on the
# restatement); the 2 m / 10 deg revisits start from an odometry-like guess within 0.6 m / 4 deg.
REVISITS = [((0.5, 0.3, 2.0), None), ((1.0, -0.5, 5.0), None), ((0.0, 0.0, 10.0), None),
            ((2.0, 0.0, 0.0), (1.4, 0.0, 0.0)), ((1.4, 1.4, 10.0), (1.0, 1.0, 6.0))]
T_BAR, R_BAR = 0.05, np.deg2rad(0.25)


def revisit(offset, guess, world_seed=3):
    w = synth.make_world(world_seed)
    PA = synth.pose_xyz_yaw(0, 0)
    PB = synth.pose_xyz_yaw(offset[0], offset[1], 0.0, offset[2])
    A, B = synth.scan_world(w, PA, seed=1), synth.scan_world(w, PB, seed=2)
    init = None if guess is None else np.linalg.inv(synth.pose_xyz_yaw(guess[0], guess[1], 0.0, guess[2])) @ PA
    return A, B, np.linalg.inv(PB) @ PA, init


@pytest.mark.parametrize("offset,guess", REVISITS)
def test_restatement_recovers_revisit(offset, guess):
    A, B, T_true, init = revisit(offset, guess)
    r = G.register(A, B, init=init)
    te, re = G.pose_error(r["transform"], T_true)
    assert te <= T_BAR and re <= R_BAR, (te, np.rad2deg(re))
    assert r["fitness"] >= 0.3 and r["rmse"] <= 0.5


def test_restatement_rejects_other_world():
    A = synth.scan_world(synth.make_world(3), synth.pose_xyz_yaw(0, 0), seed=1)
    B = synth.scan_world(synth.make_world(11, ground_z=-4.0), synth.pose_xyz_yaw(0, 0), seed=5)
    r = G.register(A, B)
    assert r["n_corr"] == 0 or r["fitness"] < 0.3 or r["rmse"] > 0.5


def test_restatement_down_sampling_order():
    p = np.array([[0.1, 0.1, 0.1], [5.0, 5.0, 5.0], [0.2, 0.2, 0.2], [np.nan, 0, 0], [5.1, 5.1, 5.1]], np.float32)
    d = G.voxel_down_sample(p, 1.0)
    np.testing.assert_allclose(d, [[0.15, 0.15, 0.15], [5.05, 5.05, 5.05]], rtol=1e-6)


@pytest.fixture(scope="module")
def lib():
    from neural_spectral_codec_amd import _lib, build
    build.build_hip()
    return _lib.lib()


def test_gicp_abi_validates_on_host(lib):
    from neural_spectral_codec_amd import _lib
    EINVAL, EUNSUP, EWS = -1, -2, -3
    p = _lib.GicpParams()
    lib.nsc_gicp_default_params(p)
    assert (p.voxel_size, p.max_correspondence_distance, p.max_iteration, p.covariance_knn) == (0.5, 1.0, 30, 20)
    P, Ns, Nt = 3, 1000, 2000
    need = lib.nsc_gicp_workspace_bytes(P, Ns, Nt)
    assert need > 0 and lib.nsc_gicp_workspace_bytes(-1, Ns, Nt) == 0 and lib.nsc_gicp_workspace_bytes(P, -1, Nt) == 0
    fake = C.c_void_p(4096)                      # never dereferenced: every check runs before a launch

    def call(**kw):
        a = dict(sp=fake, so=fake, tp=fake, to=fake, P=P, Ns=Ns, Nt=Nt, stride=4, params=p, init=fake, out=fake,
                 fr=fake, ci=fake, info=fake, ws=fake, nbytes=need)
        a.update(kw)
        return lib.nsc_gicp_register(a["sp"], a["so"], a["tp"], a["to"], a["P"], a["Ns"], a["Nt"], a["stride"],
                                     C.byref(a["params"]) if a["params"] is not None else None, a["init"], a["out"],
                                     a["fr"], a["ci"], a["info"], None, a["ws"], a["nbytes"], None)

    for k in ("sp", "so", "tp", "to", "init", "out", "fr", "ci", "info"):
        assert call(**{k: None}) == EINVAL, k
    assert call(params=None) == EINVAL
    for k in ("P", "Ns", "Nt"):
        assert call(**{k: -1}) == EINVAL, k
    assert call(stride=5) == EINVAL
    for bad in (0.0, -0.5, float("nan")):
        q = _lib.GicpParams()
        lib.nsc_gicp_default_params(q)
        q.voxel_size = bad
        assert call(params=q) == EINVAL
    q = _lib.GicpParams()
    lib.nsc_gicp_default_params(q)
    q.max_correspondence_distance = 0.0
    assert call(params=q) == EINVAL
    q.max_correspondence_distance, q.max_iteration = 1.0, -1
    assert call(params=q) == EINVAL
    q.max_iteration, q.covariance_knn = 30, _lib.GICP_MAX_KNN + 1
    assert call(params=q) == EUNSUP
    assert call(nbytes=need - 1) == EWS
    assert call(ws=None) == EWS
    assert call(P=0) == 0                        # nothing to do, nothing launched


def test_gicp_batch_limits_on_host(lib):
    """A pair or cloud count over what the launches can index (include/nsc.h NSC_GICP_MAX_*) is NSC_EUNSUPPORTED; a
    count at the limit is not (the workspace, declared one byte short, is what stops that call).  Either way the
    call returns before its first launch, so the fake pointers are never read."""
    import os
    import re
    from neural_spectral_codec_amd import _lib
    EUNSUP, EWS = -2, -3
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsc.h")).read()
    limits = {k: int(v) for k, v in re.findall(r"#define (NSC_GICP_MAX_[A-Z_]+)\s+(\d+)", hdr)}
    assert (limits["NSC_GICP_MAX_PAIRS"], limits["NSC_GICP_MAX_CLOUDS"], limits["NSC_GICP_MAX_PREPARED_PAIRS"]) == \
        (_lib.GICP_MAX_PAIRS, _lib.GICP_MAX_CLOUDS, _lib.GICP_MAX_PREPARED_PAIRS)
    assert 2 * _lib.GICP_MAX_PAIRS <= 65535 and _lib.GICP_MAX_CLOUDS <= 65535 and \
        _lib.GICP_MAX_PREPARED_PAIRS <= 65535                    # gridDim.y
    p = _lib.GicpParams()
    lib.nsc_gicp_default_params(p)
    fake = C.c_void_p(4096)
    rows = 1 << 20

    def register(P):
        need = lib.nsc_gicp_workspace_bytes(P, rows, rows)
        assert need > 0                                          # the size query works for any count
        return lib.nsc_gicp_register(fake, fake, fake, fake, P, rows, rows, 4, C.byref(p), fake, fake, fake, fake,
                                     fake, None, fake, need - 1, None)
    assert register(_lib.GICP_MAX_PAIRS + 1) == EUNSUP and register(2 ** 31 - 1) == EUNSUP
    assert register(_lib.GICP_MAX_PAIRS) == EWS

    big = 1 << 40
    store = _lib.GicpCloudSet(voxel_size=p.voxel_size, epsilon=p.epsilon, covariance_knn=p.covariance_knn, n_clouds=0,
                              n_rows=0, n_slots=0, cap_clouds=big, cap_rows=big, cap_slots=big,
                              **{k: 4096 for k in ("row_offsets", "slot_offsets", "bounds", "points", "covariances",
                                                   "slots")})

    def prepare(B):
        need = lib.nsc_gicp_prepare_workspace_bytes(B, rows)
        assert need > 0
        return lib.nsc_gicp_prepare(fake, fake, B, rows, 4, C.byref(p), C.byref(store), fake, need - 1, None)
    assert prepare(_lib.GICP_MAX_CLOUDS + 1) == EUNSUP and prepare(2 ** 31 - 1) == EUNSUP
    assert prepare(_lib.GICP_MAX_CLOUDS) == EWS

    def register_prepared(P):
        need = lib.nsc_gicp_register_prepared_workspace_bytes(P)
        assert need > 0
        return lib.nsc_gicp_register_prepared(C.byref(store), C.byref(store), fake, fake, P, C.byref(p), fake, fake,
                                              fake, fake, fake, None, fake, need - 1, None)
    assert register_prepared(_lib.GICP_MAX_PREPARED_PAIRS + 1) == EUNSUP and register_prepared(2 ** 31 - 1) == EUNSUP
    assert register_prepared(_lib.GICP_MAX_PREPARED_PAIRS) == EWS


def test_gicp_workspace_sizes(lib):
    """The three size queries, pinned where nsc_geometry.hip carved each workspace by hand (the values are that
    library's), and the structure they share: nsc_gicp_register's workspace is nsc_gicp_prepare's for its 2P clouds
    and Ns + Nt rows, followed by nsc_gicp_register_prepared's without the latter's first two regions (count: 2P
    int64; rows: P records of 64 bytes; every region is rounded up to 256 bytes)."""
    register, prepare = lib.nsc_gicp_workspace_bytes, lib.nsc_gicp_prepare_workspace_bytes
    prepared = lib.nsc_gicp_register_prepared_workspace_bytes
    assert [register(*a) for a in ((0, 0, 0), (1, 0, 0), (1, 1, 1), (3, 1000, 2000), (10, 255, 256),
                                   (32767, 1 << 20, 1 << 20))] == \
        [0, 29440, 30208, 687104, 390656, 1362595840]
    assert [prepare(*a) for a in ((0, 0), (1, 1), (6, 3000), (65535, 1 << 20))] == [0, 2816, 610048, 312998400]
    assert [prepared(P) for P in (0, 1, 3, 17, 65535)] == [0, 26368, 77568, 437760, 1685036032]

    def a256(x):
        return (x + 255) & ~255
    for P in (0, 1, 3, 17, 300, 32767):
        for Ns, Nt in ((0, 0), (1, 0), (255, 256), (1000, 2000), (1 << 20, 1 << 20)):
            assert register(P, Ns, Nt) == prepare(2 * P, Ns + Nt) + prepared(P) - a256(16 * P) - a256(64 * P), \
                (P, Ns, Nt)
