"""Stage 1 over quantised descriptors without a GPU: the restatement (tests/w1q_restatement.py) against the float32
retrieval oracle on dequantised rows, the canonical-row property of the quantiser, the argument checks of the two
entry points, and ``path_of`` against the constants of csrc/nsc_retrieval_q.hip and csrc/nsc_w1_rows.h (a change there
fails here)."""
import functools
import glob
import os

import numpy as np
import pytest

import keyframe_oracle as ko
import nsc_oracle as orc
import retrieval_oracle as ro
import w1q_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "neural-spectral-codec_amd", "csrc", "nsc_retrieval_q.hip")
SHARED = os.path.join(ROOT, "neural-spectral-codec_amd", "csrc", "nsc_w1_rows.h")


@functools.lru_cache(maxsize=1)
def encoder_descriptors(n=60):
    """(n, 800) float32 oracle descriptors of seeded uniform clouds"""
    from neural_spectral_codec_amd import synth
    return np.stack([orc.encode_points(synth.make_cloud(s, 20000, "uniform")) for s in range(n)])


@pytest.fixture(scope="module")
def lib():
    from neural_spectral_codec_amd import build, _lib
    build.build_hip()
    return _lib.lib()


def test_definition_agrees_with_the_float_oracle_on_dequantised_rows():
    """d_int / 65535 against retrieval_oracle.matrix on keyframe_oracle.dequantize'd rows: 1e-3 absolute.  The oracle
    sums 800 float32 CDF entries per pair, the restatement none; measured 3.0e-4 on distances 0.99 to 11.9."""
    d = encoder_descriptors()
    q = np.stack([ko.quantize(x) for x in d])
    want = ro.matrix(np.stack([ko.dequantize(x) for x in q]))
    got = R.dist(q, q)
    err = float(np.abs(got - want).max())
    print(f"max |restatement - oracle| = {err:.3e}; distances {want[want > 0].min():.3f} .. {want.max():.3f}; "
          f"largest d_int = {int(R.d_int(*[R.cdf(q)[0]] * 2).max())}")
    assert np.isfinite(got).all() and err <= 1e-3
    assert (np.diag(got) == 0).all() and np.array_equal(got, got.T)


def test_encoder_descriptors_quantise_to_canonical_rows():
    rows = [np.load(f)["ref_desc"] for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "enc_*.npz")))]
    assert len(rows) >= 12
    rows += list(encoder_descriptors())
    for h in rows:
        assert h.sum() > 0
        q = ko.quantize(h)
        assert R.canonical(q)[0] == 1 and int(q.astype(np.int64).sum()) == R.TOTAL
        c, ok = R.cdf(q)
        assert ok[0] == 1 and c[0, -1] == R.TOTAL and (np.diff(c[0].astype(np.int64)) >= 0).all()


def test_a_zero_histogram_is_not_canonical():
    q = ko.quantize(np.zeros(800, np.float32))
    assert not q.any() and R.canonical(q)[0] == 0
    c, ok = R.cdf(q)
    assert ok[0] == 0 and not c.any()
    assert np.isinf(R.dist(q, ko.quantize(encoder_descriptors()[0]))).all()


def test_edge_rows_and_the_wrap_row():
    for D in R.CDF_D:
        rows = R.edge_rows(D)
        sums = {k: int(v.astype(np.int64).sum()) for k, v in rows.items()}
        assert sums["random"] == sums["first"] == sums["last"] == 65535 and sums["zero"] == 0 and sums["sum_65534"] == 65534
        assert sums["all_max"] == 65535 * D
        if D >= 2:
            assert sums["sum_65536"] == 65536
        if D >= 3:
            assert sums["sum_131071"] == 131071 and sums["sum_131071"] & 0xffff == 65535     # 16-bit sums would pass it
        want = {k: int(s == 65535) for k, s in sums.items()}
        q = np.stack(list(rows.values()))
        c, ok = R.cdf(q)
        assert ok.tolist() == list(want.values())
        assert not c[ok == 0].any() and (c[ok == 1][:, -1] == 65535).all()
    for D in R.CDF_D:
        q = R.canonical_rows(7, D, seed=D)
        assert q.dtype == np.uint16 and R.canonical(q).all()


def test_extreme_pair_passes_2_pow_24():
    q = np.stack([R.one_hot(1024, 0), R.one_hot(1024, 1023)])
    di = R.d_int(*[R.cdf(q)[0]] * 2)
    assert di[0, 1] == 1023 * 65535 == 67042305 and di[0, 1] > 2 ** 24
    # 67 042 305 is odd and above 2^24: float32 holds multiples of 4 there, and the tie-free rounding goes down
    assert np.float32(di[0, 1]) == 67042304.0
    assert R.dist(q, q)[0, 1] == np.float32(67042305) / np.float32(65535)


def test_filter_is_strict_and_float32():
    pos = np.array([[0, 0, 0], [3, 4, 0], [6, 8, 0], [0, 3, 4], [5, 5, 5]], np.float32)
    q = np.zeros((1, 3), np.float32)
    up = np.nextafter(np.float32(5), np.float32(np.inf))
    assert R.filter_mask(pos, q, 5.0)[0].tolist() == [True, False, False, False, False]       # equal: kept
    assert R.filter_mask(pos, q, up)[0].tolist() == [True, True, False, True, False]
    assert R.filter_mask(pos, q, 10.0)[0].tolist() == [True, True, False, True, True]


def test_topk_rule():
    d = np.array([[3.0, 1.0, np.inf, 1.0, np.inf, 0.5], [np.inf] * 6], np.float32)
    idx, val = R.topk(d, 5)
    assert idx.tolist() == [[5, 1, 3, 0, -1], [-1] * 5]
    assert val[0].tolist() == [0.5, 1.0, 1.0, 3.0, np.inf] and np.isinf(val[1]).all()


def test_abi_argument_checks_without_gpu(lib):
    from neural_spectral_codec_amd import _lib
    assert {"nsc_w1q_cdf", "nsc_w1q_distances"} <= set(_lib.SYMBOLS) and lib.nsc_abi_version() == 4
    p = 256                                                    # non-null dummy pointer: nothing may be dereferenced
    for D in (0, -1, 1025):
        assert lib.nsc_w1q_cdf(p, 3, D, p, p, None) == -2
        assert lib.nsc_w1q_distances(p, p, 3, D, p, p, 1, None, None, 0.0, p, None) == -2
    assert lib.nsc_w1q_cdf(p, -1, 800, p, p, None) == -2
    assert lib.nsc_w1q_distances(p, p, -1, 800, p, p, 1, None, None, 0.0, p, None) == -2
    assert lib.nsc_w1q_distances(p, p, 3, 800, p, p, -1, None, None, 0.0, p, None) == -2
    assert lib.nsc_w1q_cdf(None, 0, 800, None, None, None) == 0                   # zero counts: nothing to do
    assert lib.nsc_w1q_distances(None, None, 0, 800, None, None, 3, None, None, 0.0, None, None) == 0
    assert lib.nsc_w1q_distances(None, None, 3, 800, None, None, 0, None, None, 0.0, None, None) == 0
    for args in ((None, 3, 800, p, p, None), (p, 3, 800, None, p, None), (p, 3, 800, p, None, None)):
        assert lib.nsc_w1q_cdf(*args) == -1
    ok = [p, p, 3, 800, p, p, 1, None, None, 0.0, p, None]
    for null in (0, 1, 4, 5, 10):
        a = list(ok)
        a[null] = None
        assert lib.nsc_w1q_distances(*a) == -1, null


def test_path_of_agrees_with_the_hip_source():
    src, shared = open(HIP).read(), open(SHARED).read()
    c = R.parse_constants(src, shared)
    assert c["QTL_I"] == R.QTL_I and c["QTL_KP"] == R.QTL_KP and c["STREAM_WG_CAP"] == R.STREAM_WG_CAP
    assert c["qnq"] == "Q <= 16 ? 1 : (Q <= 32 || (Q > 64 && Q <= 96) ? 2 : 4)"
    assert c["stream_split"] == "4"
    assert c["packed"] == ("D % 8 == 0 && !((reinterpret_cast<uintptr_t>(db_cdf) | "
                           "reinterpret_cast<uintptr_t>(q_cdf)) & 15u)")
    for inst in ("w1q_stream_kernel<1>", "w1q_stream_kernel<2>", "w1q_stream_kernel<4>", "launch_w1_tile(st, U16Rows{",
                 "w1q_generic_kernel", "w1q_cdf_kernel", "U16Rows::add("):
        assert inst in src, inst
    for inst in ("w1_tile_kernel<Rows, 1>", "w1_tile_kernel<Rows, 2>", "w1_tile_kernel<Rows, 4>",
                 "__builtin_amdgcn_sad_u16"):
        assert inst in shared, inst


def test_the_gpu_shapes_reach_the_paths_they_are_named_after():
    assert R.stream_n() == (1, 5, 8191, 8192, 8193, 20011)
    assert [R.path_of(N, 1, 800).trips for N in R.stream_n()] == [1, 1, 1, 1, 2, 3]
    for Q in R.STREAM_Q:
        for D in R.STREAM_D:
            p = R.path_of(20011, Q, D)
            assert p.kernel == "stream" and p.inst == {1: 1, 2: 2, 3: 4, 4: 4}[Q]
    assert R.tile_n() == (1, 63, 64, 65, 257)
    for Q in R.TILE_Q:
        for D in R.TILE_D:
            for N in R.tile_n():
                p = R.path_of(N, Q, D)
                assert p.kernel == "tile" and p.inst == R.TILE_INST[Q], (Q, D, N)
    assert {R.path_of(257, Q, 800).inst for Q in R.TILE_Q} == {1, 2, 4}
    assert {R.path_of(N, 5, 8).partial_rows for N in R.tile_n()} == {True, False}
    assert {R.path_of(1, 5, D).chunks for D in R.TILE_D} == {1, 13, 16}            # one chunk, a ragged last one, full
    for D in R.GENERIC_D:
        for Q in R.GENERIC_Q:
            assert R.path_of(257, Q, D).kernel == "generic"
    assert R.path_of(257, 1, 800, aligned=False).kernel == "generic" and R.path_of(257, 1, 800).kernel == "stream"
