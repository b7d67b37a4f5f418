"""Stage 1 over quantised descriptors on the MI355X (csrc/nsc_retrieval_q.hip, retrieval/compressed.py): the CDF kernel,
the three distance kernels and every template instance of them, the canonical flags and the spatial filter,
``CompressedRetriever`` and ``TwoStageRetrieval(compressed=True)``.

The distance is an integer sum below 2^26 followed by one float32 conversion and one IEEE division, so EVERY comparison
with the restatement (tests/w1q_restatement.py) is bit for bit, and each test first asserts from ``path_of`` that its
shapes reach the kernel it is named after (tests/test_w1q_cpu.py checks ``path_of`` against the source)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import keyframe_oracle as ko
import retrieval_families as F
import w1q_restatement as R

pytestmark = pytest.mark.gpu
INF = np.float32(np.inf)


def _c():
    from neural_spectral_codec_amd.retrieval import compressed
    return compressed


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.uint16))).cuda()


def devf(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).cuda()


def host(t):
    return t.cpu().numpy()


def assert_bits(got, want, what):
    got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want, got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        at = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ, first at {at}: got {got[at]!r}, want {want[at]!r}")


def misaligned(t):
    """a copy of the (n, D) 16-bit tensor whose base is 2 bytes past a 16-byte boundary"""
    src = t.contiguous().view(torch.int16)                      # the uint16 bits
    buf = torch.empty(src.numel() + 8, dtype=torch.int16, device=t.device)
    out = buf[1:1 + src.numel()].view(src.shape)
    out.copy_(src)
    assert out.data_ptr() % 16 == 2 and out.is_contiguous()
    return out


def gpu_cdf(q):
    cdf, ok = _c().quantized_cdf(dev16(q))
    return cdf, ok


def gpu_dist(dbc, dbok, qc, qok, *a):
    return _c().w1_distances_quantized(dbc, dbok, qc, qok, *a)


def planted(n, D, seed):
    """n canonical rows with what small databases here carry: duplicates (exact ties), both one-hot rows, and from six
    rows on one row of zeros and (D >= 3) the 131 071 row, neither canonical"""
    q = R.canonical_rows(n, D, seed)
    if n >= 6:
        e = R.edge_rows(D, seed)
        q[1] = e["zero"]
        q[n - 1], q[n - 2] = e["last"], e["first"]
        q[n // 2] = q[0]
        if D >= 3:
            q[4] = e["sum_131071"]
    return q


# ---------------------------------------------------------------------------------------------------------------------
# CDF
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", R.CDF_D)
def test_cdf_kernel(D):
    """nsc_w1q_cdf on every row around the definition of canonical (zero, sums 65534 / 65536, the 131 071 row whose low
    16 bits are 65535, every bin 65535, all mass in the first / the last bin), at 1..5 rows: partial last workgroup."""
    rows = R.edge_rows(D, seed=D)
    allrows = np.stack(list(rows.values()) + list(R.canonical_rows(3, D, seed=D)))
    want_c, want_ok = R.cdf(allrows)
    assert 0 < want_ok.sum() < len(want_ok)
    cdf, ok = gpu_cdf(allrows)
    assert cdf.dtype == torch.uint16 and ok.dtype == torch.uint8
    assert np.array_equal(host(ok), want_ok), (D, list(rows), host(ok))
    assert np.array_equal(host(cdf.view(torch.int16)).view(np.uint16), want_c)
    for n in R.CDF_N:
        for start in (0, 1, 4):                                  # the first row canonical, zero, all bins 65535
            part = allrows[start:start + n]
            cdf, ok = gpu_cdf(part)
            assert np.array_equal(host(ok), want_ok[start:start + n]), (D, n, start)
            assert np.array_equal(host(cdf.view(torch.int16)).view(np.uint16), want_c[start:start + n]), (D, n, start)


# ---------------------------------------------------------------------------------------------------------------------
# the three distance kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _free_big():
    yield
    big.cache_clear()
    mid.cache_clear()


@functools.lru_cache(maxsize=1)
def big(D):
    """20 011 rows with duplicates on both sides of the 8 192-wave cap and two rows that are not canonical, 4 queries (two
    of them database rows), and the restatement's distances"""
    n = 20011
    db = planted(n, D, seed=D)
    for a, b in ((0, 8192), (7, 8199), (7, 3), (20000, 11)):
        db[b] = db[a]
    q = np.concatenate([db[[0, 7]], R.canonical_rows(2, D, seed=D + 5000)])
    return db, q, R.dist(q, db)


@pytest.mark.parametrize("D", R.STREAM_D)
def test_stream_kernel(D):
    """w1q_stream_kernel<1|2|4>: Q = 1..4 (Q = 3 runs <4> with a zero-filled fourth query), N from one row to 20 011: at
    8 192 rows every wave has one row, at 8 193 wave 0 walks two, at 20 011 three (all three row buffers in use)."""
    ns = R.stream_n()
    assert [R.path_of(N, 1, D).trips for N in ns] == [1, 1, 1, 1, 2, 3]
    db, q, want = big(D)
    dbc, dbok = gpu_cdf(db)
    qc, qok = gpu_cdf(q)
    assert np.array_equal(host(dbok), R.canonical(db)) and host(qok).all()
    for N in ns:
        for Q in R.STREAM_Q:
            p = R.path_of(N, Q, D)
            assert p.kernel == "stream" and p.inst == {1: 1, 2: 2, 3: 4, 4: 4}[Q]
            assert_bits(gpu_dist(dbc[:N], dbok[:N], qc[:Q], qok[:Q]), want[:Q, :N], f"stream D={D} N={N} Q={Q}")
    assert_bits(gpu_dist(dbc, dbok, qc[1:2], qok[1:2]), want[1:2], f"stream D={D} second query")
    assert np.isinf(want[:, 1]).all() and want[0, 0] == 0 and want[0, 8192] == 0


@functools.lru_cache(maxsize=2)
def mid(D):
    """257 rows, 130 queries and the restatement's distances, positions and filter mask"""
    db, q = planted(257, D, seed=D + 1), planted(130, D, seed=D + 5001)
    pos, qpos = R.int_positions(257, D), R.int_positions(130, D + 1)
    pos[0] = qpos[0] + np.float32([6, 8, 0])                      # a pair at distance exactly min_dist = 10: kept
    return db, q, R.dist(q, db), pos, qpos, R.filter_mask(pos, qpos, 10.0)


@pytest.mark.parametrize("D", R.TILE_D)
def test_tile_kernel(D):
    """w1_tile_kernel<U16Rows, 1|2|4>: every NQ choice on both sides of its Q boundaries, partial row and query tiles, a last chunk
    of k-pairs that is full or not, N % 4 != 0 (the scalar store path)."""
    ns = R.tile_n()
    assert {R.path_of(257, Q, D).inst for Q in R.TILE_Q} == {1, 2, 4} and any(N % 4 for N in ns)
    db, q, want = mid(D)[:3]
    dbc, dbok = gpu_cdf(db)
    qc, qok = gpu_cdf(q)
    reached = set()
    for Q in R.TILE_Q:
        for N in ns:
            p = R.path_of(N, Q, D)
            assert p.kernel == "tile" and p.inst == R.TILE_INST[Q]
            reached.add(p.inst)
            assert_bits(gpu_dist(dbc[:N], dbok[:N], qc[:Q], qok[:Q]), want[:Q, :N], f"tile D={D} N={N} Q={Q}")
    assert reached == {1, 2, 4}
    assert np.isinf(want[1]).all() and np.isinf(want[:, 1]).all() and np.isfinite(want[0, 0])


@pytest.mark.parametrize("D", R.GENERIC_D)
def test_generic_kernel(D):
    """w1q_generic_kernel: every D the packed kernels do not take (odd, D % 8 != 0, one bin, 1 023)"""
    db, q, want = mid(D)[:3]
    dbc, dbok = gpu_cdf(db)
    qc, qok = gpu_cdf(q)
    for Q in R.GENERIC_Q:
        for N in R.GENERIC_N:
            assert R.path_of(N, Q, D).kernel == "generic"
            assert_bits(gpu_dist(dbc[:N], dbok[:N], qc[:Q], qok[:Q]), want[:Q, :N], f"generic D={D} N={N} Q={Q}")


def test_generic_kernel_on_a_misaligned_base():
    """D = 800 on a base 2 bytes past a 16-byte boundary takes the generic kernel instead of failing"""
    db, q, want = mid(800)[:3]
    dbc, dbok = gpu_cdf(db)
    qc, qok = gpu_cdf(q)
    assert R.path_of(257, 1, 800, aligned=False).kernel == "generic"
    off = misaligned(dbc)
    for Q in (1, 5):
        assert_bits(gpu_dist(off, dbok, qc[:Q], qok[:Q]), want[:Q], f"misaligned database Q={Q}")
        assert_bits(gpu_dist(dbc, dbok, misaligned(qc[:Q].contiguous()), qok[:Q]), want[:Q], f"misaligned queries Q={Q}")


def test_extreme_pair_through_all_three_kernels():
    """All mass in the first bin against all mass in the last at D = 1024: d_int = 1023 x 65535 = 67 042 305 > 2^24.  A
    float accumulator, a 16-bit wrap of the packed difference or a wrong int-to-float rounding all miss these bits."""
    D = 1024
    want = np.float32(67042305) / np.float32(65535)
    db = R.canonical_rows(70, D, seed=3)
    db[5], db[69] = R.one_hot(D, 0), R.one_hot(D, D - 1)
    q = np.concatenate([np.stack([R.one_hot(D, D - 1), R.one_hot(D, 0)]), R.canonical_rows(62, D, seed=4)])
    ref = R.dist(q, db)
    assert ref[0, 5] == want and ref[1, 69] == want and ref[0, 69] == 0
    dbc, dbok = gpu_cdf(db)
    qc, qok = gpu_cdf(q)
    for Q, kernel in ((1, "stream"), (2, "stream"), (4, "stream"), (5, "tile"), (32, "tile"), (64, "tile")):
        assert R.path_of(70, Q, D).kernel == kernel
        got = gpu_dist(dbc, dbok, qc[:Q], qok[:Q])
        assert_bits(got, ref[:Q], f"extreme {kernel} Q={Q}")
        assert host(got)[0, 5] == want
    for Q in (1, 5):
        assert_bits(gpu_dist(misaligned(dbc), dbok, qc[:Q], qok[:Q]), ref[:Q], f"extreme generic Q={Q}")


@pytest.mark.parametrize("D,Q", [(800, 3), (800, 7), (800, 40), (50, 3), (50, 7)])
def test_flags_and_filter(D, Q):
    """Rows and queries that are not canonical give +inf; the spatial filter excludes exactly the pairs the float32
    restatement excludes (strictly closer than min_dist: the pair at exactly 10 stays); positions on one side only filter
    nothing."""
    db, q, want, pos, qpos, mask = mid(D)
    assert R.path_of(257, Q, D).kernel == {(800, 3): "stream", (800, 7): "tile", (800, 40): "tile"}.get((D, Q), "generic")
    assert R.canonical(db)[1] == 0 and R.canonical(q)[1] == 0 and R.canonical(db)[0] == 1
    assert not mask[0, 0] and 0 < mask[:Q].sum() < mask[:Q].size
    d00 = qpos[0] - pos[0]
    assert float(np.sqrt((d00 * d00).sum())) == 10.0
    dbc, dbok = gpu_cdf(db)
    qc, qok = gpu_cdf(q[:Q])
    plain = host(gpu_dist(dbc, dbok, qc, qok))
    assert np.isinf(plain[:, 1]).all() and np.isinf(plain[1]).all() and np.isfinite(plain[0, 0])
    assert_bits(plain, want[:Q], f"flags D={D} Q={Q}")
    got = gpu_dist(dbc, dbok, qc, qok, devf(pos), devf(qpos[:Q]), 10.0)
    assert_bits(got, np.where(mask[:Q], INF, want[:Q]), f"filter D={D} Q={Q}")
    assert np.isfinite(host(got)[0, 0])
    assert_bits(gpu_dist(dbc, dbok, qc, qok, devf(pos), None, 10.0), want[:Q], f"db_pos only D={D} Q={Q}")
    # flags are read, not recomputed: a canonical row flagged 0 is excluded
    off = dbok.clone()
    off[0] = 0
    w2 = want[:Q].copy()
    w2[:, 0] = INF
    assert_bits(gpu_dist(dbc, off, qc, qok), w2, f"flag override D={D} Q={Q}")


def test_a_pair_does_not_depend_on_its_kernel_or_batch():
    db, q, want = mid(800)[:3]
    dbc, dbok = gpu_cdf(db)
    qc, qok = gpu_cdf(q)
    one = host(gpu_dist(dbc, dbok, qc[9:10], qok[9:10]))                                   # stream, Q = 1
    tile = host(gpu_dist(dbc, dbok, qc[:64], qok[:64]))                                    # tile, a batch of 64
    gen = host(gpu_dist(misaligned(dbc), dbok, qc[9:10], qok[9:10]))                       # generic
    assert R.path_of(257, 64, 800).kernel == "tile" and R.path_of(257, 1, 800).kernel == "stream"
    assert_bits(one, want[9:10], "stream")
    assert_bits(tile[9:10], one, "tile vs stream")
    assert_bits(gen, one, "generic vs stream")


def test_tile_grid_limit_on_both_entries():
    """Q = 64 x 65 535 + 1 queries need 65 536 column tiles, one more than a grid's y extent holds: nsc_w1q_distances and
    nsc_w1_distances_cdf both answer NSC_EUNSUPPORTED before launching anything, and ``dist`` keeps its sentinel."""
    from neural_spectral_codec_amd import _lib
    N, Q = 1, 64 * 65535 + 1
    assert R.path_of(N, Q, 8).kernel == "tile" and R.path_of(N, Q, 8).grid == (1, 65536)
    assert F.path_of(N, Q, 4).kernel == "tile" and F.path_of(N, Q, 4).grid == (1, 65536)
    L, st = _lib.lib(), _lib.stream_ptr(torch.device("cuda", torch.cuda.current_device()))
    dist = torch.full((Q, N), -7.0, dtype=torch.float32, device="cuda")
    qc = torch.zeros((Q, 8), dtype=torch.int16, device="cuda")                            # 67 MB, either way read
    ok = torch.ones((Q,), dtype=torch.uint8, device="cuda")
    p = _lib.ptr
    assert L.nsc_w1q_distances(p(qc[:1]), p(ok), N, 8, p(qc), p(ok), Q, None, None, 0.0, p(dist), st) == -2
    qf = qc.view(torch.float32)
    assert qf.shape == (Q, 4)
    assert L.nsc_w1_distances_cdf(p(qf[:1]), N, 4, p(qf), Q, None, None, 0.0, p(dist), st) == -2
    torch.cuda.synchronize()
    assert bool((dist == -7.0).all())
    assert L.nsc_w1_distances_cdf(p(qf[:1]), N, 4, p(qf), Q - 1, None, None, 0.0, p(dist), st) == 0    # 65 535 tiles: served
    torch.cuda.synchronize()
    assert bool((dist[:Q - 1] == 0.0).all()) and float(dist[Q - 1, 0]) == -7.0


# ---------------------------------------------------------------------------------------------------------------------
# CompressedRetriever
# ---------------------------------------------------------------------------------------------------------------------
def test_retriever_grows_and_ranks_like_the_restatement():
    C = _c()
    D, n = 56, C.CompressedRetriever.INITIAL_CAPACITY + 300
    db, q = planted(n, D, seed=11), planted(9, D, seed=12)
    q[0] = db[0]
    pos, qpos = R.int_positions(n, 5), R.int_positions(9, 6)
    r = C.CompressedRetriever()
    assert r.database_size == 0 and r.query(q[0])[0].size == 0
    cuts = (0, 1, 700, C.CompressedRetriever.INITIAL_CAPACITY + 1, n)                      # the third insert reallocates
    for a, b in zip(cuts[:-1], cuts[1:]):
        r.add_quantized(db[a:b], positions=pos[a:b])
    assert r.database_size == n and r._cdf.shape[0] >= n and r.n_bins == D and r.bytes_per_keyframe() == 2 * D + 13
    assert r.n_noncanonical == int((R.canonical(db) == 0).sum()) == 2
    assert np.array_equal(host(r.database_cdf.view(torch.int16)).view(np.uint16), R.cdf(db)[0])
    want = R.dist(q, db)
    idx, val = r.query_batch(q, top_k=10)
    wi, wv = R.topk(want, 10)
    assert np.array_equal(host(idx), wi)
    assert_bits(val, wv, "top-k values")
    assert (wi[1] == -1).all() and wi[0, 0] == 0 and wi[0, 1] == n // 2                    # a bad query; an exact tie
    idx, val = r.query_batch(q, top_k=10, query_positions=qpos, min_distance=21.0)
    wi, wv = R.topk(R.dist(q, db, pos, qpos, 21.0), 10)
    assert np.array_equal(host(idx), wi)
    assert_bits(val, wv, "filtered top-k values")
    i1, v1 = r.query(q[0], top_k=5)
    assert i1.tolist() == R.topk(want[:1], 5)[0][0].tolist() and isinstance(i1, np.ndarray)
    r.clear_database()
    assert r.database_size == 0 and r.n_noncanonical == 0 and r.database_cdf is None
    assert r.query_batch(q)[0].numel() == 0
    r.add_quantized(db[:3])
    assert r.database_size == 3 and host(r.query_batch(q[:1], top_k=10)[0]).shape == (1, 3)


def test_retriever_float_rows_and_queries():
    """add_to_database quantises float rows as quantize_batch does; a float query equals its own quantised row as a query"""
    from neural_spectral_codec_amd.encoding.quantization import quantize_batch
    C = _c()
    D = 800
    rng = np.random.default_rng(21)
    h = (rng.random((300, D)) ** 3).astype(np.float32)
    qh = (rng.random((6, D)) ** 3).astype(np.float32)
    qq = np.stack([ko.quantize(x) for x in h])
    qqh = np.stack([ko.quantize(x) for x in qh])
    assert np.array_equal(host(quantize_batch(devf(qh)).view(torch.int16)).view(np.uint16), qqh)
    r = C.CompressedRetriever()
    r.add_to_database(h)
    assert r.n_noncanonical == 0 and np.array_equal(host(r.database_cdf.view(torch.int16)).view(np.uint16), R.cdf(qq)[0])
    fi, fv = r.query_batch(devf(qh), top_k=10)
    ui, uv = r.query_batch(dev16(qqh), top_k=10)
    ni, nv = r.query_batch(qqh, top_k=10)                                                   # host uint16 rows
    wi, wv = R.topk(R.dist(qqh, qq), 10)
    for i, v in ((fi, fv), (ui, uv), (ni, nv)):
        assert np.array_equal(host(i), wi)
        assert_bits(v, wv, "values")


def test_retriever_records():
    """add_records of pack_records' output -- device tensor, list of bytes, one blob -- equals add_quantized of the rows"""
    from neural_spectral_codec_amd.encoding.quantization import pack_records
    C = _c()
    D, n = 800, 40
    db = planted(n, D, seed=31)
    rng = np.random.default_rng(32)
    pose7 = np.concatenate([R.int_positions(n, 33), rng.random((n, 4)).astype(np.float32)], 1)
    ts = np.arange(n) * 0.1 + 1e9
    ids = np.arange(n, dtype=np.int64) * 7 + 2 ** 31                                      # ids above 2^31 survive
    rec = pack_records(dev16(db), devf(pose7), torch.from_numpy(ts), torch.from_numpy(ids),
                       torch.zeros((n, 20), dtype=torch.uint8))
    blob = host(rec).tobytes()
    assert host(rec).tobytes()[:2 * D] == db[0].tobytes() and ko.unpack_record(blob[:rec.shape[1]], D)[3] == ids[0]
    q, qpos = planted(7, D, seed=34), R.int_positions(7, 35)
    a = C.CompressedRetriever()
    a.add_quantized(db, positions=pose7[:, :3])
    want = a.query_batch(q, top_k=10, query_positions=qpos, min_distance=21.0)
    wi, wv = R.topk(R.dist(q, db, pose7[:, :3], qpos, 21.0), 10)
    assert np.array_equal(host(want[0]), wi)
    rb = rec.shape[1]
    forms = (rec, [blob[i * rb:(i + 1) * rb] for i in range(n)], blob)
    for form in forms:
        b = C.CompressedRetriever()
        gi, gt = b.add_records(form, n_bins=D)
        assert host(gi).tolist() == ids.tolist() and np.array_equal(host(gt), ts)
        assert b.database_size == n and b.n_noncanonical == a.n_noncanonical == 2
        got = b.query_batch(q, top_k=10, query_positions=qpos, min_distance=21.0)
        assert np.array_equal(host(got[0]), wi)
        assert_bits(got[1], wv, "values")
    b = C.CompressedRetriever()
    b.add_records(blob[:rb])                                                               # one record: D from its length
    b.add_records(blob[rb:])                                                               # the database fixes D now
    assert b.database_size == n and np.array_equal(host(b.query_batch(q, top_k=10)[0]), host(a.query_batch(q, top_k=10)[0]))


def test_retriever_leaves_unfillable_slots_empty():
    """12 rows, 3 of them canonical, top_k = 10: slots 3.. hold -1 / +inf"""
    C = _c()
    D = 56
    db = np.zeros((12, D), np.uint16)
    db[[2, 5, 9]] = R.canonical_rows(3, D, seed=41)
    db[7, :2] = 40000                                                                      # sums to 80 000
    q = R.canonical_rows(2, D, seed=42)
    r = C.CompressedRetriever()
    r.add_quantized(db)
    assert r.n_noncanonical == 9
    idx, val = r.query_batch(q, top_k=10)
    wi, wv = R.topk(R.dist(q, db), 10)
    assert host(idx).shape == (2, 10) and np.array_equal(host(idx), wi)
    assert_bits(val, wv, "values")
    assert sorted(wi[0, :3].tolist()) == [2, 5, 9] and (wi[:, 3:] == -1).all() and np.isinf(wv[:, 3:]).all()


# ---------------------------------------------------------------------------------------------------------------------
# TwoStageRetrieval(compressed=True)
# ---------------------------------------------------------------------------------------------------------------------
def _keyframes(n, D, seed):
    from neural_spectral_codec_amd import synth
    rng = np.random.default_rng(seed)
    desc = (rng.random((n, D)) ** 3).astype(np.float32)
    desc[n // 2:] = desc[:n - n // 2] + (rng.random((n - n // 2, D)) * 0.05).astype(np.float32)   # the second half revisits
    poses = synth.make_pose_chain(n, seed=seed)
    return [SimpleNamespace(keyframe_id=1000 + i, scan_id=i, points=None, pose=poses[i], timestamp=float(i),
                            descriptor=desc[i], embedding=None) for i in range(n)], desc, poses


def test_two_stage_compressed_equals_the_restatement():
    from neural_spectral_codec_amd.retrieval import CompressedRetriever, TwoStageRetrieval, create_two_stage_retrieval
    n, D, k, thr = 300, 800, 10, 50.0
    kfs, desc, poses = _keyframes(n, D, seed=51)
    r = create_two_stage_retrieval(top_k=k, spatial_filter_distance=thr, compressed=True)
    assert isinstance(r.retriever, CompressedRetriever) and isinstance(r, TwoStageRetrieval)
    r.add_keyframes(kfs[:200])
    for kf in kfs[200:]:
        r.add_keyframe(kf)
    assert r.retriever.database_size == n and r.retriever.n_noncanonical == 0
    q = np.stack([ko.quantize(x) for x in desc])
    pos = poses[:, :3, 3].astype(np.float32)
    queries = [0, 17, 150, 151, 299]
    want = R.dist(q[queries], q, pos, pos[queries], thr)
    wi, wv = R.topk(want, k)
    assert (wi >= 0).any() and np.isinf(want[np.arange(5), queries]).all()                 # a query never finds itself
    got = r.global_retrieval_batch([kfs[i] for i in queries])
    for row, (ri, rv) in enumerate(zip(wi, wv)):
        keep = ri >= 0
        assert [c.database_idx for c in got[row]] == ri[keep].tolist()
        assert [np.float32(c.distance) for c in got[row]] == rv[keep].tolist()
    one = r.query(kfs[150], verify=False)
    assert [c.database_idx for c in one] == wi[2][wi[2] >= 0].tolist()
    r.clear_database()
    assert r.retriever.database_size == 0 and r.query(kfs[0], verify=False) == []


def test_two_stage_default_is_unchanged():
    from neural_spectral_codec_amd.retrieval import TwoStageRetrieval, WassersteinRetriever
    kfs, _, _ = _keyframes(300, 800, seed=52)
    a = TwoStageRetrieval(top_k=10, spatial_filter_distance=50.0)
    b = TwoStageRetrieval(top_k=10, spatial_filter_distance=50.0, compressed=False)
    assert type(a.retriever) is WassersteinRetriever and type(b.retriever) is WassersteinRetriever
    for r in (a, b):
        r.add_keyframes(kfs)
    qs = [kfs[i] for i in (0, 17, 150, 299)]
    ga, gb = a.global_retrieval_batch(qs), b.global_retrieval_batch(qs)
    assert [[(c.database_idx, c.distance) for c in row] for row in ga] == [[(c.database_idx, c.distance) for c in row] for row in gb]
    assert any(len(row) for row in ga)
