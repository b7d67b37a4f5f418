"""The store of prepared clouds without a GPU: nsc_gicp_prepare and nsc_gicp_register_prepared validate their
arguments on the host and return before launching anything."""
import ctypes as C

import pytest

EINVAL, EUNSUP, EWS = -1, -2, -3
FAKE = C.c_void_p(4096)                  # never dereferenced: every check runs before a launch


@pytest.fixture(scope="module")
def lib():
    from neural_spectral_codec_amd import _lib, build
    build.build_hip()
    return _lib.lib()


def params(lib, **kw):
    from neural_spectral_codec_amd import _lib
    p = _lib.GicpParams()
    lib.nsc_gicp_default_params(p)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def cloud_set(**kw):
    from neural_spectral_codec_amd import _lib
    s = _lib.GicpCloudSet(voxel_size=0.5, epsilon=1e-3, covariance_knn=20, n_clouds=2, n_rows=100, n_slots=200,
                          cap_clouds=10, cap_rows=2100, cap_slots=4200)
    for k in ("row_offsets", "slot_offsets", "bounds", "points", "covariances", "slots"):
        setattr(s, k, 4096)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_prepare_validates_on_host(lib):
    B, N = 3, 2000                       # the set above has room for exactly 2 + 3 clouds of 2000 rows at most
    need = lib.nsc_gicp_prepare_workspace_bytes(B, N)
    assert need > 0
    assert lib.nsc_gicp_prepare_workspace_bytes(-1, N) == 0 and lib.nsc_gicp_prepare_workspace_bytes(B, -1) == 0
    p0 = params(lib)

    def call(pts=FAKE, off=FAKE, n=B, total=N, stride=4, p=p0, st="default", ws=FAKE, nbytes=need):
        st = cloud_set() if st == "default" else st
        return lib.nsc_gicp_prepare(pts, off, n, total, stride, C.byref(p) if p is not None else None,
                                    C.byref(st) if st is not None else None, ws, nbytes, None)

    for k in ("pts", "off"):
        assert call(**{k: None}) == EINVAL, k
    assert call(st=None) == EINVAL and call(p=None) == EINVAL
    for k in ("row_offsets", "slot_offsets", "bounds", "points", "covariances", "slots"):
        assert call(st=cloud_set(**{k: None})) == EINVAL, k
    assert call(n=-1) == EINVAL and call(total=-1) == EINVAL
    assert call(stride=5) == EINVAL
    assert call(p=params(lib, voxel_size=0.25)) == EINVAL
    assert call(p=params(lib, covariance_knn=10)) == EINVAL
    assert call(p=params(lib, epsilon=1e-2)) == EINVAL
    assert call(p=params(lib, covariance_knn=33), st=cloud_set(covariance_knn=33)) == EUNSUP
    # the radius and the iteration parameters are not the set's business
    assert call(p=params(lib, max_correspondence_distance=2.0, max_iteration=3), ws=None) == EWS
    assert call(st=cloud_set(n_rows=cloud_set().cap_rows + 1)) == EINVAL       # inconsistent set
    # capacity for the batch's upper bound: one cloud, one row or one slot short
    assert call(st=cloud_set(cap_clouds=4)) == EWS
    assert call(st=cloud_set(cap_rows=100 + N - 1)) == EWS
    assert call(st=cloud_set(cap_slots=200 + 2 * N - 1)) == EWS
    assert call(nbytes=need - 1) == EWS
    assert call(ws=None) == EWS
    assert call(n=0) == 0                # nothing to do, nothing launched
    assert call(n=0, pts=None, off=None, ws=None) == 0


def test_register_prepared_validates_on_host(lib):
    P = 4
    need = lib.nsc_gicp_register_prepared_workspace_bytes(P)
    assert need > 0 and lib.nsc_gicp_register_prepared_workspace_bytes(-1) == 0
    p0 = params(lib)

    def call(src="default", tgt="default", sid=FAKE, tid=FAKE, n=P, p=p0, init=FAKE, out=FAKE, fr=FAKE, ci=FAKE,
             info=FAKE, ws=FAKE, nbytes=need):
        src = cloud_set() if src == "default" else src
        tgt = cloud_set() if tgt == "default" else tgt
        ref = lambda x: C.byref(x) if x is not None else None      # noqa: E731
        return lib.nsc_gicp_register_prepared(ref(src), ref(tgt), sid, tid, n, ref(p), init, out, fr, ci, info, None,
                                              ws, nbytes, None)

    for k in ("sid", "tid", "init", "out", "fr", "ci", "info"):
        assert call(**{k: None}) == EINVAL, k
    assert call(src=None) == EINVAL and call(tgt=None) == EINVAL and call(p=None) == EINVAL
    assert call(tgt=cloud_set(slots=None)) == EINVAL
    assert call(n=-1) == EINVAL
    for which in ("src", "tgt"):
        for k, v in (("voxel_size", 0.25), ("covariance_knn", 10), ("epsilon", 1e-2)):
            assert call(**{which: cloud_set(**{k: v})}) == EINVAL, (which, k)
    assert call(p=params(lib, voxel_size=0.25)) == EINVAL
    assert call(p=params(lib, max_correspondence_distance=0.0)) == EINVAL
    assert call(p=params(lib, max_correspondence_distance=2.0, max_iteration=5, relative_fitness=0.0),
                ws=None) == EWS                  # free per call: only the missing workspace is refused
    assert call(nbytes=need - 1) == EWS
    assert call(ws=None) == EWS
    assert call(n=0) == 0
    assert call(n=0, sid=None, tid=None, init=None, out=None, fr=None, ci=None, info=None, ws=None) == 0
