"""The retrieval input families (tests/retrieval_families.py) without a GPU: the exact integer W1 equals the float32
oracle bit for bit on every dyadic family, ``path_of`` agrees with the constants of csrc/nsc_retrieval.hip and
csrc/nsc_w1_rows.h (a change there fails here, loudly), and every (N, Q, D) the GPU tests use reaches the kernel instance it is named after."""
import os

import numpy as np
import pytest

import miner_oracle as mo
import retrieval_families as F
import retrieval_oracle as ro
from retrieval_families import CDF_D, STREAM_D, STREAM_N, STREAM_Q, TILE_D, TILE_INST, TILE_N, TILE_Q, TOPK_K, TOPK_N, k_of

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "neural-spectral-codec_amd", "csrc")
HIP, SHARED = os.path.join(CSRC, "nsc_retrieval.hip"), os.path.join(CSRC, "nsc_w1_rows.h")


def hip_constants():
    return F.parse_constants(open(HIP).read(), open(SHARED).read())


def test_path_of_agrees_with_the_hip_source():
    c = hip_constants()
    assert c["TK_CHUNK"] == F.TK_CHUNK and c["TL_I"] == F.TL_I and c["STREAM_WG_CAP"] == F.STREAM_WG_CAP
    assert c["TK_MAX_K"] == F.TK_MAX_K and c["TK_MAX_CAND"] == F.TK_MAX_CAND
    assert c["per_of"] == "int p = ((D + 63) / 64 + 3) / 4 * 4; return p < 4 ? 4 : p;"
    assert c["nq"] == "Q <= 16 ? 1 : (Q <= 32 || (Q > 64 && Q <= 96) ? 2 : 4)"
    assert c["stream_split"] == "4"
    src, shared = open(HIP).read(), open(SHARED).read()
    for inst in ("w1_cdf_kernel<4>", "w1_cdf_kernel<8>", "w1_cdf_kernel<12>", "w1_cdf_kernel<16>", "w1_dist_kernel<8>",
                 "w1_dist_kernel<12>", "w1_stream_kernel<1>", "w1_stream_kernel<2>", "w1_stream_kernel<4>",
                 "launch_w1_tile(st, F32Rows{"):
        assert inst in src, inst
    for inst in ("w1_tile_kernel<Rows, 1>", "w1_tile_kernel<Rows, 2>", "w1_tile_kernel<Rows, 4>"):
        assert inst in shared, inst


def test_per_of_and_the_d_set_reach_all_four_instances():
    assert [F.per_of(D) for D in (1, 256, 257, 512, 513, 768, 769, 1024)] == [4, 4, 8, 8, 12, 12, 16, 16]
    assert {F.per_of(D) for D in CDF_D} == {4, 8, 12, 16}
    assert any(D % 4 for D in CDF_D) and any(D % 2 for D in CDF_D)
    for D in range(1, 1025):                                  # a lane's PER bins cover the row
        assert 64 * F.per_of(D) >= D


def test_stream_shapes_walk_one_two_and_three_rows():
    assert [F.path_of(N, 1, 800).trips for N in STREAM_N] == [1, 1, 1, 1, 2, 3]
    assert F.path_of(8192, 1, 800).waves == 8192 and F.path_of(5, 1, 800).waves == 8
    for Q in STREAM_Q:
        for D in STREAM_D:
            p = F.path_of(20011, Q, D)
            assert p.cached and p.kernel == "stream" and p.inst == {1: 1, 2: 2, 3: 4, 4: 4}[Q]


def test_tile_shapes_reach_every_instance_and_store_path():
    for Q in TILE_Q:
        for N in TILE_N:
            p = F.path_of(N, Q, 800)
            assert p.kernel == "tile" and p.inst == TILE_INST[Q], (Q, N)
    assert {F.path_of(N, 5, 4).scalar_store for N in TILE_N} == {True, False}
    assert {F.path_of(N, 5, 4).partial_rows for N in TILE_N} == {True, False}
    assert any(D % 32 for D in TILE_D) and any(D % 32 == 0 for D in TILE_D)       # a partial last k chunk and a full one


def test_topk_shapes_reach_the_boundary_and_the_fallback():
    assert F.topk_path(32768, 256).path == "kernel" and F.topk_path(32768, 256).chunks * 256 == F.TK_MAX_CAND
    assert F.topk_path(32769, 256).path == "sort" and F.topk_path(32769, 256).chunks * 256 == F.TK_MAX_CAND + 256
    assert F.topk_path(2050, 7).last == 2 and F.topk_path(2050, 7).chunks == 2            # a last chunk shorter than k
    assert F.topk_path(300, 257).path == "sort" and F.topk_path(20011, 256).path == "kernel"
    for k in TOPK_K:
        for N in TOPK_N:
            N = k if N == "k" else N
            if N >= k:
                assert F.topk_path(N, k).path == "kernel", (N, k)


@pytest.mark.parametrize("D", CDF_D + (52, 800, 36))
def test_exact_w1_equals_the_float32_oracle_bitwise(D):
    k = k_of(D)
    db = F.dyadic_hists(40, D, k, seed=D)
    assert (db[1] == 0).all() and db[39, D - 1] == 2 ** k and db[38, 0] == 2 ** k and (db[20] == db[0]).all()
    q = F.dyadic_hists(3, D, k, seed=D + 5000)
    want = F.w1_exact(q, db, k)
    for i in range(3):
        got = ro.batch(q[i].astype(np.float32), db.astype(np.float32))
        assert np.array_equal(got.view(np.uint32), want[i].view(np.uint32)), (D, i)
    got = ro.matrix(q.astype(np.float32), db.astype(np.float32))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # float64 keeps the 1e-8 of (sum + eps) that float32 absorbs: 1e-8 / 2^k per CDF entry, at most D of them
    assert np.abs(F.w1_f64(q, db) - want).max() <= D * 1e-8 / 2 ** k * 1.01
    assert want[0, 0] == want[0, 20]                                              # the duplicate is an exact tie
    # the zero row: its distance is the other row's CDF sum, and the tail bin contributes exactly 1
    c = F.cdf_exact(q, k)
    assert np.array_equal(want[:, 1], c.sum(1, dtype=np.float64).astype(np.float32)) and (c[:, -1] == 1.0).all()


@pytest.mark.parametrize("k", [6, 10, 12])
def test_exact_w1_at_the_largest_mass_and_width(k):
    db = F.dyadic_hists(30, 1024, k, seed=k)
    want = F.w1_exact(db[:4], db, k)
    assert np.array_equal(ro.matrix(db[:4].astype(np.float32), db.astype(np.float32)), want)


def test_topk_lex_rule():
    d = np.array([[3.0, 1.0, np.nan, 1.0, np.inf, 0.5], [np.inf] * 6, [np.nan, np.nan, 2.0, np.nan, np.nan, np.nan]],
                 np.float32)
    idx, val = F.topk_lex(d, 4)
    assert idx.tolist() == [[5, 1, 3, 0], [0, 1, 2, 3], [2, -1, -1, -1]]
    assert val[0].tolist() == [0.5, 1.0, 1.0, 3.0] and np.isinf(val[1]).all() and np.isinf(val[2][1:]).all()
    rng = np.random.default_rng(0)
    d = rng.integers(0, 50, (5, 400)).astype(np.float32)                           # many exact ties
    idx, val = F.topk_lex(d, 30)
    for r in range(5):
        o, v = ro.topk(d[r], 30)
        assert idx[r].tolist() == o.tolist() and np.array_equal(val[r], v)


def test_filter_mask_is_strict():
    pos = np.array([[0, 0, 0], [3, 4, 0], [6, 8, 0], [0, 3, 4], [5, 5, 5]], np.float32)
    q = np.zeros((1, 3), np.float32)
    up, down = np.nextafter(np.float32(5), np.float32(np.inf)), np.nextafter(np.float32(5), np.float32(0))
    assert F.filter_mask(pos, q, 5.0)[0].tolist() == [True, False, False, False, False]     # equal: kept
    assert F.filter_mask(pos, q, up)[0].tolist() == [True, True, False, True, False]
    assert F.filter_mask(pos, q, down)[0].tolist() == [True, False, False, False, False]
    assert F.filter_mask(pos, q, 10.0)[0].tolist() == [True, True, False, True, True]


def test_rounding_rows_and_the_derived_tolerance():
    for fam in ("counts", "cubed", "sparse"):
        h = F.rounding_rows(fam, 50, 1024, 0)
        assert h.dtype == np.float32 and (h >= 0).all() and (h.sum(1) > 0).all()
        ref = F.w1_f64(h[:2], h)
        orc = np.stack([ro.batch(h[i], h) for i in range(2)])
        tol, ratio = F.oracle_tolerance(ref, orc)
        assert (tol >= 1e-4 * np.abs(ref) + 1e-5).all() and (np.abs(orc - ref) <= tol).all() and ratio >= 0
    assert 0.01 < (F.rounding_rows("sparse", 50, 1024, 0) > 0).mean() < 0.03


def test_miner_reference_rules():
    # anchor 0 on the origin; frames 40.. at x = 12 with duplicated descriptors
    n, k = 70, 6
    pos = np.zeros((n, 3))
    pos[40:, 0] = 12.0
    pos[35] = (3.0, 4.0, 0.0)                                  # exactly on the positive radius: inclusive
    desc = F.dyadic_hists(n, 8, k, seed=1, plant=False)
    desc[50] = desc[45] = desc[41]
    ref = F.mine_reference(desc, k, pos)
    assert 35 in ref[0].pos and ref[0].neg.tolist() == list(range(40, 70))
    want = mo.mine_sequence(desc.astype(np.float64), pos)[0]
    assert want[0].tolist() == ref[0].pos.tolist() and np.array_equal(want[3].astype(np.float32), ref[0].w1)
    w = ref[0].w1
    assert ref[0].hard == 40 + int(np.argmin(w))                                  # np.argmin: the first of equal minima
    assert ref[0].semi == int(ref[0].neg[np.argsort(w, kind="stable")[len(w) // 2]])


def test_recall_references():
    e = np.arange(12, dtype=np.float32).reshape(6, 2)
    d, band = F.pairwise_l2_reference(e, [0, 3], 1)
    assert band.tolist() == [[True, True, False, False, False, False], [False, False, True, True, True, False]]
    assert d[0, 2] == np.float32(np.sqrt(32.0)) and np.isinf(d[1, 3])
    pos = np.array([[0, 0, 0], [10, 0, 0], [3, 4, 0], [0, 0, 1]], np.float64)
    assert F.revisit_reference(pos, 1, 5.0).tolist() == [3, -1, -1, -1]           # (3, 4, 0) is AT 5: excluded
    assert F.revisit_reference(pos, 0, 5.0).tolist() == [0, 1, 2, 3]
    assert F.recall_rank_reference(pos, [0, 0], np.array([[1, 2, 3], [1, -1, 3]]), 5.0).tolist() == [3, 0]
