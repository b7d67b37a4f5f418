"""Every dispatch path of the stage-1 retrieval kernels (csrc/nsc_retrieval.hip) on the MI355X: the five W1 distance
kernels and all their template instances, the top-k selection and its sort fallback, the triplet miner and the recall
helpers, on the seeded families of tests/retrieval_families.py.  Each test first asserts, from ``path_of`` /
``topk_path`` alone, that its input reaches the branch it is named after (tests/test_retrieval_families_cpu.py checks
the same claims and the constants behind them without a GPU).

Distances on dyadic histograms (integer rows with sum 2^k) are compared BIT FOR BIT with the int64 reference
``w1_exact``: nothing rounds, so no summation order can excuse a difference; ties are exact, so top-k indices are
compared exactly under the (value, index) rule.  General float32 rows are compared with the float64 restatement
``w1_f64`` under max(the suite's 1e-4 |d| + 1e-5, 2 x the float32 oracle's own worst deviation from float64 for the same
query on the same rows); the measured ratios are in DESIGN.md 4.4a."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import retrieval_families as F
import retrieval_oracle as ro
from retrieval_families import (CDF_D, CDF_N, STREAM_D, STREAM_N, STREAM_Q, TILE_D, TILE_INST, TILE_N, TILE_Q, TOPK_K,
                                TOPK_N, k_of)

pytestmark = pytest.mark.gpu
EPS = 1e-8
INF = np.float32(np.inf)


def _w():
    from neural_spectral_codec_amd.retrieval import wasserstein as w
    return w


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


def assert_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want, got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        at = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ, first at {at}: got {got[at]!r}, want {want[at]!r}")


def int_positions(n, seed, lo=-20, hi=21):
    return np.random.default_rng([seed, n]).integers(lo, hi, (n, 3)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact distances, every kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", CDF_D)
def test_cdf_kernel_exact(D):
    """nsc_w1_cdf: all four PER instances, odd D (rows only 4-byte aligned), both normalisations, a zero row, all mass in
    the first / the last bin."""
    assert F.path_of(1, 1, D).per == {1: 4, 3: 4, 4: 4, 51: 4, 256: 4, 257: 8, 512: 8, 513: 12, 768: 12, 769: 16, 801: 16,
                                      1023: 16, 1024: 16}[D]
    k = k_of(D)
    six = F.dyadic_hists(6, D, k, seed=D, dups=((0, 3),))[[0, 1, 5, 4, 3]]     # random, zero, last bin, first bin, copy of 0
    for n in CDF_N:
        h = six[:n]
        for plain in (True, False):
            got = _w()._cdf(dev(h), EPS, plain)
            assert_bits(got, F.cdf_exact(h, k), f"cdf D={D} n={n} plain={plain}")


@pytest.mark.parametrize("D", CDF_D)
def test_dist_kernel_exact(D):
    """nsc_w1_distances (raw histogram rows, normalised in the kernel): all four PER instances, Q in {1, 3}, N % 4 != 0,
    with and without positions."""
    N = 37
    assert F.path_of(N, 3, D).per == F.per_of(D) and N % 4 != 0
    k = k_of(D)
    db, q = F.dyadic_hists(N, D, k, seed=D), F.dyadic_hists(3, D, k, seed=D + 5000)
    want = F.w1_exact(q, db, k)
    pos, qpos = int_positions(N, D), int_positions(3, D + 1)
    mask = F.filter_mask(pos, qpos, 21.0)
    assert 0 < mask.sum() < mask.size
    dbt, qc, post, qpt = dev(db), dev(F.cdf_exact(q, k)), dev(pos), dev(qpos)
    for Q in (1, 3):
        assert_bits(_w()._distances(dbt, qc[:Q], EPS), want[:Q], f"dist D={D} Q={Q}")
        assert_bits(_w()._distances(dbt, qc[:Q], EPS, post, qpt[:Q], 21.0), np.where(mask[:Q], INF, want[:Q]),
                    f"dist+filter D={D} Q={Q}")
        # positions on one side only: no filter
        assert_bits(_w()._distances(dbt, qc[:Q], EPS, post, None, 21.0), want[:Q], f"dist db_pos only D={D} Q={Q}")


@pytest.fixture(scope="module", autouse=True)
def _free_big():
    yield
    big.cache_clear()
    cubed.cache_clear()


@functools.lru_cache(maxsize=1)
def big(D):
    """20 011 dyadic rows with duplicates on both sides of the 8 192-wave cap, 4 queries (two of them database rows), and
    their exact distances"""
    n, k = 20011, k_of(D)
    db = F.dyadic_hists(n, D, k, seed=D, dups=((0, n // 2), (0, 8192), (7, 8199), (7, 3), (20000, 11)))
    q = np.concatenate([db[[0, 7]], F.dyadic_hists(2, D, k, seed=D + 5000)])
    return db, q, F.w1_exact(q, db, k), k


@pytest.mark.parametrize("D", STREAM_D)
def test_stream_kernel_exact(D):
    """w1_stream_kernel<1|2|4>: Q = 1..4 (Q = 3 runs <4> with a zero-filled fourth query and the t >= Q break), N from 1 row
    to 20 011: at 8 192 rows every wave has one row, at 8 193 wave 0 walks two (prefetch, rotation, stride), at 20 011
    three."""
    assert [F.path_of(N, 1, D).trips for N in STREAM_N] == [1, 1, 1, 1, 2, 3]
    db, q, want, k = big(D)
    dbc, qc = dev(F.cdf_exact(db, k)), dev(F.cdf_exact(q, k))
    for N in STREAM_N:
        for Q in STREAM_Q:
            p = F.path_of(N, Q, D)
            assert p.kernel == "stream" and p.inst == {1: 1, 2: 2, 3: 4, 4: 4}[Q]
            assert_bits(_w()._distances_cdf(dbc[:N], qc[:Q]), want[:Q, :N], f"stream D={D} N={N} Q={Q}")
    # the second query alone: row 0 of a batch of one is not special
    assert_bits(_w()._distances_cdf(dbc, qc[1:2]), want[1:2], f"stream D={D} second query")


@pytest.mark.parametrize("D", TILE_D)
def test_tile_kernel_exact(D):
    """w1_tile_kernel<1|2|4>: every NQ choice on both sides of its Q boundaries, partial row tiles, partial query tiles, a
    last k chunk that is full (D % 32 == 0) or not, and N % 4 != 0 (the scalar store path)."""
    assert {F.path_of(257, Q, D).inst for Q in TILE_Q} == {1, 2, 4} and any(F.path_of(N, 5, D).scalar_store for N in TILE_N)
    k = k_of(D)
    db, q = F.dyadic_hists(257, D, k, seed=D + 1), F.dyadic_hists(130, D, k, seed=D + 5001)
    want = F.w1_exact(q, db, k)
    dbc, qc = dev(F.cdf_exact(db, k)), dev(F.cdf_exact(q, k))
    for Q in TILE_Q:
        for N in TILE_N:
            p = F.path_of(N, Q, D)
            assert p.kernel == "tile" and p.inst == TILE_INST[Q]
            assert_bits(_w()._distances_cdf(dbc[:N], qc[:Q]), want[:Q, :N], f"tile D={D} N={N} Q={Q}")


@functools.lru_cache(maxsize=1)
def cubed():
    """257 database rows and 97 queries on which float32 sums do round, as device CDF rows and read back"""
    D, N = 800, 257
    dbc = _w()._cdf(dev(F.rounding_rows("cubed", N, D, 11)), EPS, False)
    qc = _w()._cdf(dev(F.rounding_rows("cubed", 97, D, 12)), EPS, True)
    return dbc, qc, dbc.cpu().numpy(), qc.cpu().numpy()


def test_tile_kernel_batch_independence():
    """One query's row of distances is bitwise the same at Q = 5, 17, 33, 65, 97 and at any position in the batch (each
    (row, query) sum is accumulated by one thread in ascending k), on rows where rounding does happen -- and it IS the
    sequential float32 sum in ascending k of the CDF rows the kernel read (np.cumsum in float32 is sequential; a pairwise
    or a descending sum of these rows changes bits in more than 230 of the 257)."""
    D, N = 800, 257
    assert [F.path_of(N, Q, D).inst for Q in (5, 17, 33, 65, 97)] == [1, 2, 4, 2, 4]
    dbc, qc, dbc_h, qc_h = cubed()
    base = _w()._distances_cdf(dbc, qc[:5])[0].cpu().numpy()
    assert np.isfinite(base).all() and len(np.unique(base)) > 200
    diff = np.abs(dbc_h - qc_h[0])
    assert diff.dtype == np.float32
    assert_bits(base, np.cumsum(diff, axis=1, dtype=np.float32)[:, -1], "tile kernel vs the ascending-k float32 sum")
    for Q in (5, 17, 33, 65, 97):
        for at in sorted({0, 1, Q // 2, Q - 1}):
            order = list(range(1, Q))
            order.insert(at, 0)                                  # query 0 moved to position `at`
            got = _w()._distances_cdf(dbc, qc[torch.tensor(order).cuda()].contiguous())[at]
            assert_bits(got, base, f"batch independence Q={Q} at={at}")


def stream_sum(diff):
    """w1_stream_kernel's sum of each row of |a - b| (N, D) in float32: lane l adds its float4 chunks c = l + 64 j, j
    ascending, components x, y, z, w (a lane past the row adds zeros), then v += v[lane ^ o] for o = 32, 16, .., 1"""
    N, D = diff.shape
    assert diff.dtype == np.float32 and D % 4 == 0 and D <= 1024
    chunks = np.zeros((N, 4 * 64 * 4), np.float32)
    chunks[:, :D] = diff
    chunks = chunks.reshape(N, 4, 64, 4)                         # [row][j][lane][component]
    v = np.zeros((N, 64), np.float32)
    for j in range(4):
        for comp in range(4):
            v = v + chunks[:, j, :, comp]
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, np.arange(64) ^ o]
    assert v.dtype == np.float32
    return v[:, 0]


def test_stream_kernel_accumulation_order():
    """The float stream kernel at Q = 1 on the rounding rows equals its restated lane-strided sum and butterfly bit for
    bit; that order is not the ascending-k one (the restatement itself differs from it in most of the 257 rows)."""
    D, N = 800, 257
    assert F.path_of(N, 1, D).kernel == "stream" and F.path_of(N, 1, D).inst == 1
    dbc, qc, dbc_h, qc_h = cubed()
    diff = np.abs(dbc_h - qc_h[0])
    want = stream_sum(diff)
    assert (want.view(np.uint32) != np.cumsum(diff, axis=1, dtype=np.float32)[:, -1].view(np.uint32)).sum() > 200
    assert_bits(_w()._distances_cdf(dbc, qc[:1])[0], want, "stream kernel vs its restated order")


# ---------------------------------------------------------------------------------------------------------------------
# 2. spatial filter: strict '<' at the threshold, on all three distance kernels and the uncached retriever
# ---------------------------------------------------------------------------------------------------------------------
OFFSETS = np.array([[3, 4, 0], [0, -4, 3], [6, 8, 0], [0, 0, 0], [3, 4, 1], [-8, 0, 6], [4, 3, 0]], np.float32)


def filter_case(N, Q, seed):
    """integer positions: database rows far from every query except, for each of the first 3 queries, rows at offsets of
    length exactly 5 (3-4-5), exactly 10 (6-8-10), 0, and sqrt(26)"""
    rng = np.random.default_rng([seed, N, Q])
    pos = rng.integers(1000, 2000, (N, 3)).astype(np.float32)
    qpos = np.stack([[50.0 * t, -7.0 * t, 3.0] for t in range(Q)]).astype(np.float32)
    qpos[3:] -= 5000.0
    planted = {}
    for t in range(min(Q, 3)):
        rows = 10 * t + np.arange(len(OFFSETS))
        pos[rows] = qpos[t] + OFFSETS
        planted[t] = rows
    return pos, qpos, planted


def thresholds():
    out = []
    for r in (5.0, 10.0):
        r = np.float32(r)
        out += [float(r), float(np.nextafter(r, INF)), float(np.nextafter(r, np.float32(0)))]
    return out


@pytest.mark.parametrize("kernel,D,Q", [("dist", 51, 3), ("dist", 257, 3), ("stream", 52, 1), ("stream", 52, 2),
                                        ("stream", 52, 3), ("tile", 52, 17), ("tile", 800, 5)])
def test_spatial_filter_is_strict_at_the_threshold(kernel, D, Q):
    N = 301
    p = F.path_of(N, Q, D)
    assert (p.kernel if p.cached else "dist") == kernel
    k = k_of(D)
    db, q = F.dyadic_hists(N, D, k, seed=D), F.dyadic_hists(Q, D, k, seed=D + 9000)
    want = F.w1_exact(q, db, k)
    pos, qpos, planted = filter_case(N, Q, D)
    dbt, dbc, qc, post, qpt = dev(db), dev(F.cdf_exact(db, k)), dev(F.cdf_exact(q, k)), dev(pos), dev(qpos)
    for md in thresholds():
        mask = F.filter_mask(pos, qpos, md)
        for t, rows in planted.items():                          # rows at |offset| = 5, 5, 10, 0, sqrt 26, 10, 5
            near5, near10 = md > 5.0, md > 10.0                 # a distance EQUAL to min_dist is kept
            assert mask[t, rows].tolist() == [near5, near5, near10, True, md > 5.1, near10, near5], (md, t)
        assert mask.sum() == sum(mask[t, r].sum() for t, r in planted.items())
        if kernel == "dist":
            got = _w()._distances(dbt, qc, EPS, post, qpt, md)
        else:
            got = _w()._distances_cdf(dbc, qc, post, qpt, md)
        assert_bits(got, np.where(mask, INF, want), f"{kernel} D={D} Q={Q} min_dist={md!r}")


def test_uncached_retriever_filter_and_growth():
    """A retriever with D % 4 != 0 keeps no CDF rows and sends every query through nsc_w1_distances with positions; its
    buffers grow twice here, and the result equals a retriever filled in one call and the exact reference."""
    N, D, Q, kk = 2200, 50, 3, 7
    assert not F.path_of(N, Q, D).cached and F.path_of(N, Q, D).per == 4 and F.topk_path(N, kk).chunks == 2
    k = k_of(D)
    db, q = F.dyadic_hists(N, D, k, seed=D, dups=((0, 1100), (0, 2100), (30, 31))), F.dyadic_hists(Q, D, k, seed=D + 1)
    q[0] = db[0]
    pos, qpos, planted = filter_case(N, Q, D)
    grown = _w().WassersteinRetriever(device="cuda")
    caps = []
    for a, b in ((0, 600), (600, 1200), (1200, N)):
        grown.add_to_database(db[a:b].astype(np.float32), positions=pos[a:b])
        caps.append(int(grown._buf.shape[0]))
    assert caps == [1024, 2048, 4096] and grown._cdf_buf is None and grown.database_size == N
    once = _w().WassersteinRetriever(device="cuda")
    once.add_to_database(torch.from_numpy(db.astype(np.float32)), positions=pos)
    assert once._cdf_buf is None
    exact = F.w1_exact(q, db, k)
    for md in (0.0,) + tuple(thresholds()):
        want = np.where(F.filter_mask(pos, qpos, md), INF, exact)
        wi, wv = F.topk_lex(want, kk)
        for r in (grown, once):
            idx, val = r.query_batch(q.astype(np.float32), top_k=kk, query_positions=qpos, min_distance=md)
            assert np.array_equal(idx.cpu().numpy(), wi), md
            assert_bits(val, wv, f"uncached retriever min_dist={md!r}")
    idx, val = grown.query_batch(q.astype(np.float32), top_k=kk)                 # no positions: no filter
    wi, wv = F.topk_lex(exact, kk)
    assert np.array_equal(idx.cpu().numpy(), wi) and idx[0, :3].tolist() == [0, 1100, 2100]
    assert_bits(val, wv, "uncached retriever, no filter")


# ---------------------------------------------------------------------------------------------------------------------
# 3. top-k
# ---------------------------------------------------------------------------------------------------------------------
def tied_distances(Q, N, seed):
    """small integers, so almost every value is an exact tie somewhere in the row"""
    return np.random.default_rng([seed, Q, N]).integers(0, 1000, (Q, N)).astype(np.float32)


def check_topk(d, k, what):
    idx, val = _w()._topk(dev(d), k)
    wi, wv = F.topk_lex(d, k)
    got = idx.cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, wi), (what, got[got != wi][:5], wi[got != wi][:5])
    assert_bits(val, wv, what)


@pytest.mark.parametrize("k", TOPK_K)
def test_topk_kernel_exact(k):
    for N in TOPK_N:
        N = k if N == "k" else N
        if N < k:
            continue
        tp = F.topk_path(N, k)
        assert tp.path == "kernel"
        d = tied_distances(3, N, k)
        if N > 2048:
            d[:, 2046:min(N, 2051)] = -1.0                       # equal values straddling the first chunk boundary
        d[1, N - 1] = -2.0                                       # the last element of the row is the smallest
        if tp.last < k and tp.chunks > 1:
            d[2, N - tp.last:] = -1.0                            # ties inside a last chunk shorter than k
        check_topk(d, k, f"topk k={k} N={N}")
    for Q in (1, 300):
        check_topk(tied_distances(Q, 2049, k + Q), k, f"topk k={k} Q={Q}")


def test_topk_short_and_infinite_rows():
    """fewer than k finite values (the filter excluded the rest), and a row that is all +inf: +inf entries are ordinary
    values, returned with their indices in index order"""
    N, k = 2050, 64
    assert F.topk_path(N, k).path == "kernel" and F.topk_path(N, k).last == 2
    d = np.full((3, N), np.inf, np.float32)
    d[0, [2049, 5, 2047]] = [1.0, 1.0, 0.5]
    d[2] = tied_distances(1, N, 0)[0]
    d[2, 40:] = np.inf
    check_topk(d, k, "short rows")
    idx, val = _w()._topk(dev(d), k)
    assert idx[0, :4].tolist() == [2047, 5, 2049, 0] and idx[1].tolist() == list(range(k)) and bool(torch.isinf(val[1]).all())


@pytest.mark.parametrize("N,k,path", [(32768, 256, "kernel"), (32769, 256, "sort"), (131072, 64, "kernel"),
                                      (131073, 64, "sort"), (300, 300, "sort"), (257, 257, "sort"), (256, 256, "kernel"),
                                      (4097, 4097, "sort")])
def test_topk_boundary_and_sort_fallback(N, k, path):
    """chunks * k at 4 096 and one chunk past it, k == N beyond 256: the stable-sort fallback returns the same indices and
    values as the selection kernel's rule"""
    assert F.topk_path(N, k).path == path
    d = tied_distances(2, N, N + k)
    if N > 2051:
        d[0, 2046:2051] = -1.0
    d[1, N - 1] = -2.0
    check_topk(d, k, f"topk N={N} k={k} ({path})")


@pytest.mark.parametrize("N,k,path", [(2050, 7, "kernel"), (2050, 256, "kernel"), (300, 300, "sort"), (33000, 256, "sort")])
def test_topk_nan_distances(N, k, path):
    """A NaN distance (a NaN histogram row) is never selected and never ahead of a finite or infinite value: the slots a
    row cannot fill hold index -1 and +inf.  The selection kernel and the sort fallback agree on this."""
    assert F.topk_path(N, k).path == path
    d = tied_distances(3, N, N + k)
    d[0, [0, 3, 2047, 2048, N - 1][: (5 if N > 2048 else 2)]] = np.nan
    d[1, :] = np.nan
    d[1, [N - 1, 17, 2]] = [4.0, np.inf, 4.0]                    # three selectable values in the whole row
    d[2, 5] = np.nan
    check_topk(d, k, f"topk with NaN N={N} k={k} ({path})")
    idx, val = _w()._topk(dev(d), k)
    assert not bool(torch.isnan(val).any())
    if k >= 4:
        assert idx[1, :4].tolist() == [2, N - 1, 17, -1]


def test_query_batch_with_a_nan_row_is_the_same_on_both_topk_paths():
    """what a caller sees: a database with one NaN histogram, asked for 256 (kernel) and 257 (fallback) neighbours"""
    N, D = 300, 52
    assert F.topk_path(N, 256).path == "kernel" and F.topk_path(N, 257).path == "sort" and F.path_of(N, 1, D).kernel == "stream"
    k = k_of(D)
    db = F.dyadic_hists(N, D, k, seed=3).astype(np.float32)
    db[40] = np.nan
    r = _w().WassersteinRetriever(device="cuda")
    r.add_to_database(db)
    i256, v256 = r.query(db[0], top_k=256)
    i300, v300 = r.query(db[0], top_k=300)
    assert 40 not in i256 and 40 not in i300 and np.array_equal(i300[:256], i256) and np.array_equal(v300[:256], v256)
    assert i300[-1] == -1 and np.isinf(v300[-1]) and (i300[:-1] >= 0).all() and np.isfinite(v300[:-1]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. end to end on a dyadic database
# ---------------------------------------------------------------------------------------------------------------------
def test_retriever_end_to_end_exact():
    """WassersteinRetriever on 20 011 rows with duplicates: query (stream kernel, waves walk three rows) and query_batch
    with 40 queries (tile kernel) return exactly the (value, index) top-k of the exact distances."""
    D, kk = 800, 10
    db, q4, want4, k = big(D)
    N = len(db)
    p1, p40 = F.path_of(N, 1, D), F.path_of(N, 40, D)
    assert p1.kernel == "stream" and p1.trips == 3 and p40.kernel == "tile" and p40.inst == 4
    assert F.topk_path(N, kk).path == "kernel" and F.topk_path(N, kk).chunks == 10
    q = np.concatenate([q4, db[[8192, 8199, 20000, 1, N - 1, N - 2]], F.dyadic_hists(30, D, k, seed=77, plant=False)])
    want = F.w1_exact(q, db, k)
    wi, wv = F.topk_lex(want, kk)
    assert wi[0, :3].tolist() == [0, 8192, N // 2] and wi[1, :3].tolist() == [3, 7, 8199]       # the duplicates, by index
    r = _w().WassersteinRetriever(device="cuda")
    r.add_to_database(db[:9000].astype(np.float32))
    r.add_to_database(torch.from_numpy(db[9000:].astype(np.float32)))
    assert r._cdf_buf is not None and r.database_size == N
    assert_bits(r._cdf_buf[:N], F.cdf_exact(db, k), "cached CDF rows")
    for j in range(6):
        idx, val = r.query(q[j].astype(np.float32), top_k=kk)
        assert np.array_equal(idx, wi[j]), j
        assert_bits(val, wv[j], f"query {j}")
    idx, val = r.query_batch(q.astype(np.float32), top_k=kk)
    assert np.array_equal(idx.cpu().numpy(), wi)
    assert_bits(val, wv, "query_batch of 40")


# ---------------------------------------------------------------------------------------------------------------------
# 5. rounding-sensitive inputs against float64
# ---------------------------------------------------------------------------------------------------------------------
def check_valid_topk(idx, val, ref, tol, k, what):
    """a valid answer under tol: nothing returned is worse than the reference k-th by more than tol, nothing better than it
    by more than tol is missing, values ascending and within tol of the reference at their own index"""
    kth = np.sort(ref)[k - 1]
    assert len(set(idx.tolist())) == k and (idx >= 0).all(), what
    assert (ref[idx] <= kth + tol[idx]).all(), what
    must = np.nonzero(ref < kth - tol)[0]
    assert set(must.tolist()) <= set(idx.tolist()), what
    assert (np.diff(val) >= 0).all() and (np.abs(val.astype(np.float64) - ref[idx]) <= tol[idx]).all(), what


@pytest.mark.parametrize("D", [257, 768, 1024])
@pytest.mark.parametrize("family", ["counts", "cubed", "sparse"])
def test_rounding_sensitive_rows_against_float64(family, D):
    N, Q, kk = 2000, 8, 10
    p = F.path_of(N, Q, D)
    assert p.per == {257: 8, 768: 12, 1024: 16}[D] and p.cached == (D % 4 == 0)
    db, q = F.rounding_rows(family, N, D, 1), F.rounding_rows(family, Q, D, 2)
    ref = F.w1_f64(q, db, EPS, True)
    orc = np.stack([ro.batch(q[j], db) for j in range(Q)])
    tol, oracle_ratio = F.oracle_tolerance(ref, orc)
    suite = F.SUITE_TOL[0] * np.abs(ref) + F.SUITE_TOL[1]
    dbt, qc = dev(db), _w()._cdf(dev(q), EPS, True)
    runs = {"dist": _w()._distances(dbt, qc, EPS)}
    if p.cached:
        dbc = _w()._cdf(dbt, EPS, False)
        assert F.path_of(N, 4, D).kernel == "stream" and p.kernel == "tile"
        runs["stream<1>"] = _w()._distances_cdf(dbc, qc[:1])
        runs["stream<4>"] = _w()._distances_cdf(dbc, qc[:4])
        runs["tile"] = _w()._distances_cdf(dbc, qc)
    for name, got in runs.items():
        nq = int(got.shape[0])
        g = got.cpu().numpy().astype(np.float64)
        err = np.abs(g - ref[:nq])
        print(f"rounding {family} D={D} {name}: kernel worst ratio to the suite bound {(err / suite[:nq]).max():.3f}, "
              f"oracle worst ratio {oracle_ratio:.3f}, bound used / suite bound {(tol / suite).max():.3f}")
        assert (err <= tol[:nq]).all(), (family, D, name, float((err / tol[:nq]).max()))
        idx, val = _w()._topk(got, kk)
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        for j in range(nq):
            check_valid_topk(idx[j], val[j], ref[j], tol[j], kk, (family, D, name, j))


# ---------------------------------------------------------------------------------------------------------------------
# 6. miner
# ---------------------------------------------------------------------------------------------------------------------
MINE = dict(pmax=5.0, ptmin=3, nmin=10.0, nmax=50.0, ntmin=4)
# sites whose mutual distances sit exactly on the radii: 5 (inclusive positive), 10 (excluded negative), 50 (inclusive
# negative), and one step beyond each
SITES = np.array([[0, 0, 0], [3, 4, 0], [6, 8, 0], [30, 40, 0], [6, 8, 1], [30, 40, 1], [12, 0, 0], [0, 0, 1], [0, 10, 0],
                  [0, 50, 0]], np.float64)
FAR = np.array([500.0, 0.0, 0.0])


def mine_case(n, seed):
    """positions on SITES, descriptors from a pool of 5 (exact W1 ties among the negatives).  Frames >= 64 with an odd index
    sit in a second cluster 500 m away together with frame 5, whose candidates are therefore all in lanes >= 64 of the
    ballot loop; frame 9 is alone at 1 000 m (no candidate at all), frames 11 and 14 share a place at 2 000 m (each the
    other's positive, no negative), frames 16 and 21 are 20 m apart at 3 000 m (each the other's negative, no positive)."""
    rng = np.random.default_rng([seed, n])
    k, D = 6, 16
    pos = SITES[rng.integers(0, len(SITES), n)]
    far = np.array([i for i in range(n) if i >= 64 and i % 2] + ([5] if n > 64 else []), dtype=np.int64)
    pos[far] += FAR
    if n > 21:
        pos[9] = (0.0, 1000.0, 0.0)
        pos[11] = pos[14] = (0.0, 2000.0, 0.0)
        pos[16], pos[21] = (0.0, 3000.0, 0.0), (0.0, 3020.0, 0.0)
    pool = F.dyadic_hists(5, D, k, seed=seed, plant=False)
    desc = pool[rng.integers(0, 5, n)]
    return desc, pos, k


def mine(desc, pos, strategy, per_anchor=1, seed=0, **kw):
    from neural_spectral_codec_amd.gnn.triplet_miner import TripletMiner
    P = dict(MINE, **kw)
    m = TripletMiner(positive_distance_max=P["pmax"], positive_temporal_min=P["ptmin"], negative_distance_min=P["nmin"],
                     negative_distance_max=P["nmax"], negative_temporal_min=P["ntmin"], mining_strategy=strategy)
    np.random.seed(seed)
    trip, counts = m.mine_sequence(np.arange(len(pos)), dev(desc), torch.from_numpy(np.asarray(pos, np.float64)).cuda(),
                                   per_anchor)
    by = {}
    for a, p, n in trip.cpu().numpy().tolist():
        by.setdefault(a, []).append((p, n))
    return by, counts.cpu().numpy()


def mine_claims(n, ref, pos):
    """the case holds what the test is named after (from the reference alone)"""
    d = np.linalg.norm(pos[:, None] - pos[None], axis=2)
    gap = np.abs(np.arange(n)[:, None] - np.arange(n)[None])
    if n >= 63:
        assert ((d == 5.0) & (gap >= MINE["ptmin"])).any() and ((d == 10.0) & (gap >= MINE["ntmin"])).any()
        assert ((d == 50.0) & (gap >= MINE["ntmin"])).any()
        assert ((d <= 5.0) & (gap == MINE["ptmin"])).any() and ((d <= 5.0) & (gap == MINE["ptmin"] - 1)).any()
        assert ((d > 10.0) & (d <= 50.0) & (gap == MINE["ntmin"])).any()
        assert ((d > 10.0) & (d <= 50.0) & (gap == MINE["ntmin"] - 1)).any()
        assert any(r.hard is not None and (r.w1 == r.w1.min()).sum() > 1 for r in ref)          # tied hard negatives
        assert (len(ref[11].pos), len(ref[11].neg)) == (1, 0) and (len(ref[16].pos), len(ref[16].neg)) == (0, 1)
        assert len(ref[9].pos) == len(ref[9].neg) == 0
    if n == 200:
        assert ref[5].hard is not None and min(ref[5].pos.min(), ref[5].neg.min()) >= 64        # only lanes >= 64
        assert any(r.hard is not None and r.neg.min() < 64 <= r.neg.max() and r.pos.min() < 64 <= r.pos.max() for r in ref)


@pytest.mark.parametrize("n", [3, 63, 64, 65, 200])
def test_miner_constructed_sequences(n):
    desc, pos, k = mine_case(n, n)
    ref = F.mine_reference(desc, k, pos, **MINE)
    mine_claims(n, ref, pos)
    want_counts = np.array([[len(r.pos), len(r.neg)] for r in ref], np.int32)
    mining = {a for a, r in enumerate(ref) if r.hard is not None}
    assert (n == 3) == (not mining)
    for strategy, pick in (("hard", "hard"), ("semi-hard", "semi"), ("random", None)):
        for per_anchor in (1, 2):
            by, counts = mine(desc, pos, strategy, per_anchor, seed=n)
            assert np.array_equal(counts, want_counts), strategy
            assert set(by) == mining, strategy
            for a, pairs in by.items():
                assert len(pairs) == per_anchor
                for p, ng in pairs:
                    assert p in ref[a].pos, (strategy, a, p)
                    if pick:
                        assert ng == getattr(ref[a], pick), (strategy, a, ng, getattr(ref[a], pick))
                    else:
                        assert ng in ref[a].neg, (strategy, a, ng)
    if n == 3:                                                   # nothing qualifies: the public call returns an empty list
        from neural_spectral_codec_amd.gnn.triplet_miner import TripletMiner
        poses = np.tile(np.eye(4), (n, 1, 1))
        poses[:, :3, 3] = pos
        assert TripletMiner(positive_temporal_min=3, negative_temporal_min=4).mine_triplets(desc, poses, 1, None) == []


def test_miner_semi_hard_differs_from_hard_and_radii_are_as_stated():
    """one anchor, every radius case spelled out: d == positive_distance_max is a positive, d == negative_distance_min is
    not a negative, d == negative_distance_max is"""
    n, k, D = 70, 6, 16
    pos = np.array([[0.0, 1000.0 * (i + 1), 0.0] for i in range(n)])
    pos[0] = 0.0
    pos[10], pos[11] = (3, 4, 0), (3, 4, 1)                      # 5: positive; sqrt 26: nothing
    pos[2] = (0, 0, 1)                                           # gap 2 < positive_temporal_min
    pos[3] = (0, 0, 1)                                           # gap 3: positive
    pos[20], pos[21], pos[22], pos[23] = (6, 8, 0), (6, 8, 1), (30, 40, 0), (30, 40, 1)         # 10: no; yes; 50: yes; no
    pos[60:68] = [(12, j, 0) for j in range(8)]                  # negatives on both sides of lane 64
    desc = F.dyadic_hists(n, D, k, seed=5, plant=False)
    desc[61] = desc[65] = desc[21]                               # three equal W1 values
    ref = F.mine_reference(desc, k, pos, **MINE)
    assert ref[0].pos.tolist() == [3, 10] and ref[0].neg.tolist() == [21, 22] + list(range(60, 68))
    assert ref[0].neg.min() < 64 <= ref[0].neg.max()
    for strategy, want in (("hard", ref[0].hard), ("semi-hard", ref[0].semi)):
        by, counts = mine(desc, pos, strategy)
        assert counts[0].tolist() == [2, 10] and by[0][0][1] == want and by[0][0][0] in (3, 10), (strategy, by[0])
    assert ref[0].hard != ref[0].semi
    # the anchor's own descriptor among the negatives' ties: W1 = 0 at 21, 61, 65 -> hard takes the lowest index
    desc[0] = desc[21]
    ref = F.mine_reference(desc, k, pos, **MINE)
    assert ref[0].hard == 21 and (ref[0].w1 == 0).sum() == 3
    by, _ = mine(desc, pos, "hard")
    assert by[0][0][1] == 21
    by, _ = mine(desc, pos, "semi-hard")
    assert by[0][0][1] == ref[0].semi


def test_miner_nan_position_is_nobodys_candidate():
    n = 200
    desc, pos, k = mine_case(n, n)
    pos[7] = np.nan
    ref = F.mine_reference(desc, k, pos, **MINE)
    assert len(ref[7].pos) == len(ref[7].neg) == 0 and all(7 not in r.pos and 7 not in r.neg for r in ref)
    for strategy in ("hard", "semi-hard", "random"):
        by, counts = mine(desc, pos, strategy)
        assert np.array_equal(counts, np.array([[len(r.pos), len(r.neg)] for r in ref], np.int32))
        assert 7 not in by and all(7 not in pair for pairs in by.values() for pair in pairs)
        if strategy != "random":
            assert all(pairs[0][1] == getattr(ref[a], "hard" if strategy == "hard" else "semi") for a, pairs in by.items())


def test_miner_random_draws_reach_every_candidate():
    """2 000 draws (250 seeds x 8 per anchor) for an anchor with 5 positives and 5 negatives, the negatives on both sides of
    the 64-lane ballot boundary: every candidate appears, nothing else does"""
    n, k, D = 70, 6, 16
    pos = np.array([[0.0, 1000.0 * (i + 1), 0.0] for i in range(n)])
    pos[0] = 0.0
    pos[10:15] = (3, 4, 0)
    pos[61:66] = (12, 0, 0)
    desc = F.dyadic_hists(n, D, k, seed=6, plant=False)
    ref = F.mine_reference(desc, k, pos, **MINE)
    assert ref[0].pos.tolist() == list(range(10, 15)) and ref[0].neg.tolist() == list(range(61, 66))
    seen_p, seen_n = set(), set()
    for seed in range(250):
        by, _ = mine(desc, pos, "random", per_anchor=8, seed=seed)
        assert len(by[0]) == 8
        seen_p |= {p for p, _ in by[0]}
        seen_n |= {ng for _, ng in by[0]}
    assert seen_p == set(range(10, 15)) and seen_n == set(range(61, 66))


# ---------------------------------------------------------------------------------------------------------------------
# 7. recall helpers, called the way gnn/trainer.py calls them
# ---------------------------------------------------------------------------------------------------------------------
def _call(name, *args):
    from neural_spectral_codec_amd import _lib
    st = getattr(_lib.lib(), name)(*args, _lib.stream_ptr(torch.device("cuda", torch.cuda.current_device())))
    _lib.check(st, name)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("D", [1, 32, 63, 64, 65, 200])
def test_pairwise_l2_per_element(D):
    """integer embeddings: the float64 sum of squares is exact, one rounding (sqrt, then to float32) on both sides"""
    for n in (1, 15, 16, 17, 1000):
        for skip in (0, 30):
            emb = np.random.default_rng([D, n]).integers(-8, 9, (n, D)).astype(np.float32)
            qidx = np.unique(np.array([0, n // 2, n - 1, min(n - 1, 31), min(n - 1, 16)], np.int32))
            want, band = F.pairwise_l2_reference(emb, qidx, skip)
            assert band.sum() == sum(min(n - 1, q + skip) - max(0, q - skip) + 1 for q in qidx)
            e, qi = dev(emb), torch.from_numpy(qidx).cuda()
            dist = torch.full((len(qidx), n), -7.0, dtype=torch.float32, device="cuda")
            _call("nsc_pairwise_l2", _ptr(e), _ptr(qi), len(qidx), n, D, skip, _ptr(dist))
            assert_bits(dist, want, f"pairwise_l2 D={D} n={n} skip={skip}")


@pytest.mark.parametrize("n", [1, 17, 300])
def test_revisit_queries(n):
    for skip in (0, 3, 30):
        pos = SITES[np.random.default_rng([n, skip]).integers(0, len(SITES), n)]
        want = F.revisit_reference(pos, skip, 5.0)
        if n == 300 and skip:
            d = np.linalg.norm(pos[:, None] - pos[None], axis=2)
            i = np.arange(n)
            assert (d == 5.0).any()
            # a frame whose only candidates before its answer sit exactly AT the threshold (strict '<': passed over)
            assert any(want[a] > a + skip and (d[a, a + skip:want[a]] == 5.0).any() for a in i[want >= 0])
        if skip == 0:
            assert want.tolist() == list(range(n))               # every frame revisits itself at distance 0
        p = torch.from_numpy(pos).cuda()
        first = torch.full((n,), -9, dtype=torch.int32, device="cuda")
        _call("nsc_revisit_queries", _ptr(p), n, skip, C.c_double(5.0), _ptr(first))
        assert np.array_equal(first.cpu().numpy(), want), (n, skip)


def test_recall_rank_every_rank_and_padding():
    k, thr = 6, 5.0
    # query frames at the origin; 'near' 3 m away, 'edge' exactly at the threshold (3-4-5), 'far' 50 m away
    pos = np.zeros((40, 3))
    near, edge, far = 10, 11, 12
    pos[near], pos[edge], pos[far] = (3, 0, 0), (3, 4, 0), (30, 40, 0)
    rows, want = [], []
    for r in range(k):                                           # a hit at each rank 1..k, behind far and at-threshold frames
        row = [far if t % 2 else edge for t in range(k)]
        row[r] = near
        rows.append(row)
        want.append(r + 1)
    rows.append([far, edge] * (k // 2)); want.append(0)          # no hit: AT the threshold does not count
    rows.append([far, -1, near, -1, -1, -1]); want.append(0)     # a -1 ends the row before the hit
    rows.append([near, -1, -1, -1, -1, -1]); want.append(1)
    rows.append([-1] * k); want.append(0)
    reps = 30                                                    # 300 queries: more than one workgroup
    topk = np.array(rows * reps, np.int64)
    qidx = np.arange(len(topk), dtype=np.int32) % 9              # frames 0..8 are all at the origin
    assert len(qidx) > 256 and F.recall_rank_reference(pos, qidx, topk, thr).tolist() == want * reps
    p, qi, tk = torch.from_numpy(pos).cuda(), torch.from_numpy(qidx).cuda(), torch.from_numpy(topk).cuda()
    rank = torch.full((len(qidx),), -9, dtype=torch.int32, device="cuda")
    _call("nsc_recall_rank", _ptr(p), _ptr(qi), _ptr(tk), len(qidx), k, C.c_double(thr), _ptr(rank))
    assert rank.cpu().numpy().tolist() == want * reps
