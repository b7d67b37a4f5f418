"""Every search path, parameter set and batch shape of the GICP kernels (csrc/nsc_geometry.hip) on the MI355X, against
the float64 restatement (tests/gicp_restatement.py) on the seeded families of tests/gicp_clouds.py.  Each test first
asserts, from the reference alone, that its input reaches the branch it is named after
(``gicp_restatement.path_census``; tests/test_gicp_families_cpu.py checks the same without a GPU).  Neighbour sets are
compared under the kernel's documented rule (distance, then index) with no mask for equal distances; the only rows a
test leaves out of a covariance comparison are those whose two smallest eigenvalues coincide (the normal is then
undefined), at most 5 % of a cloud, and for those the matrix must still be U diag(1, 1, epsilon) U^T.

Tolerances are the project's: points 1e-6 m, covariances 1e-4 of the reference's norm, system terms 1e-6 relative,
end to end 1e-3 m / 1e-4 on rotation entries / 1e-3 on fitness."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gicp_clouds as F
import gicp_restatement as G
from test_gicp_families_cpu import (FACES_SEED, LATTICE_SEEDS, MANY_SMALL_SEED, MASK_CAP, MIN_GAP, RADIUS_MARGIN,
                                    TINY_SEED, assert_claim, reference)
from test_gicp_gpu import dev_pack, run
from test_gicp_store_gpu import KEYS, _edge_fn, _same_closures, assert_bitwise, prepared, raw, store_of

pytestmark = pytest.mark.gpu


def _gv():
    from neural_spectral_codec_amd.retrieval import geometric_verification as gv
    return gv


def full3(c6):
    return np.stack([c6[:, [0, 1, 2]], c6[:, [1, 3, 4]], c6[:, [2, 4, 5]]], 1)


def check_cloud(what, points, cov6, count, ref, eps):
    """one cloud's stage outputs against its reference (gicp_clouds.cloud_reference)"""
    ds, C, sep = ref["ds"], ref["cov"], ref["sep"]
    assert count == len(ds), (what, count, len(ds))
    if count == 0:
        return
    assert np.max(np.abs(points[:count] - ds)) <= 1e-6, what
    got = full3(cov6[:count])
    assert 1.0 - sep.mean() <= MASK_CAP, (what, sep.mean())
    err = np.abs(got - C).max(axis=(1, 2)) / np.linalg.norm(C, axis=(1, 2))
    print(f"{what}: {count} rows, {int((~sep).sum())} left out, covariance error {err[sep].max():.3g}")
    assert err[sep].max() <= 1e-4, (what, err[sep].max(), int(np.argmax(np.where(sep, err, 0))))
    w = np.linalg.eigvalsh(got)                                  # every row, the left-out ones included
    assert np.abs(w - np.array([eps, 1.0, 1.0])).max() <= 1e-9, what


def check_system(what, out, p, lin, n_source):
    """pair p's system0, evaluation and information at the fixed transform against ``linearize``"""
    s0 = out["system0"][p]
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = s0[:21]
    H = H + np.triu(H, 1).T
    assert s0[27] == lin["n_corr"] == out["n_correspondences"][p], (what, s0[27], lin["n_corr"])
    assert out["iterations"][p] == 0
    assert np.array_equal(out["transform"][p], out["init"][p]), what
    tol = lambda ref: 1e-6 * max(np.abs(ref).max(), 1e-300)
    assert np.allclose(H, lin["H"], rtol=1e-6, atol=tol(lin["H"])), what
    assert np.allclose(s0[21:27], lin["g"], rtol=1e-6, atol=tol(lin["g"])), what
    assert abs(s0[28] - lin["sse"]) <= 1e-6 * lin["sse"], what
    assert abs(out["fitness"][p] - lin["fitness"]) <= 1e-6 * lin["fitness"], what
    assert abs(out["rmse"][p] - lin["rmse"]) <= 1e-6 * lin["rmse"], what
    assert np.allclose(out["information"][p], lin["info"], rtol=1e-6, atol=tol(lin["info"])), what


def staged(sources, targets, inits, stride=4, **params):
    out = run(sources, targets, inits, stages=True, stride=stride, max_iteration=0, **params)
    out["init"] = np.asarray(inits, np.float64)
    return out


@pytest.mark.parametrize("name", list(F.STAGE_CASES))
def test_stage_parity(name):
    A, B, T_fix, params, stride = F.stage_case(name)
    ra, rb, census, _, _ = reference(name)
    assert_claim(name, census)                                   # the input reaches the branch it is named after
    radius = params["max_correspondence_distance"]
    assert min(ra["gap"], rb["gap"]) > MIN_GAP                   # no neighbour near a tie: no tie mask
    assert F.radius_margin(ra["ds"], rb["ds"], T_fix, radius) > RADIUS_MARGIN
    out = staged([A], [B], [T_fix], stride=stride, **params)
    ns = len(A)
    check_cloud(name + " source", out["points"][:ns], out["covariances"][:ns], out["counts"][0], ra,
                params["epsilon"])
    check_cloud(name + " target", out["points"][ns:], out["covariances"][ns:], out["counts"][1], rb,
                params["epsilon"])
    lin = G.linearize(ra["ds"], rb["ds"], ra["cov"], rb["cov"], T_fix, radius)
    assert lin["n_corr"] > 100
    check_system(name, out, 0, lin, len(ra["ds"]))


@pytest.mark.parametrize("seed", LATTICE_SEEDS)
@pytest.mark.parametrize("k", [8, 20])
def test_lattice_ties(seed, k):
    """Equal distances everywhere, exact on both sides: the neighbour sets follow (distance, index) and the
    correspondences the smaller target index, with nothing masked."""
    L = F.lattice(seed)
    params = dict(voxel_size=0.5, covariance_knn=k, epsilon=1e-3, max_correspondence_distance=1.0)
    ref = F.cloud_reference(L, params)
    assert G.ring_census(ref["ds"], 0.5, k)["stops"].all()
    idx, d2 = G.knn_exact(ref["ds"], k)
    assert (d2[:, k] == d2[:, k - 1]).mean() >= 0.4
    T = np.eye(4)
    T[0, 3] = 0.25                                               # half a voxel: two nearest targets per source row
    out = staged([L], [L], [T], **params)
    n = len(L)
    for rows, c in ((slice(0, n), 0), (slice(n, None), 1)):
        assert np.array_equal(out["points"][rows][:out["counts"][c]], ref["ds"])       # exact, in first-row order
        check_cloud(f"lattice {seed} k={k}", out["points"][rows], out["covariances"][rows], out["counts"][c], ref,
                    1e-3)
    lin = G.linearize(ref["ds"], ref["ds"], ref["cov"], ref["cov"], T, 1.0, exact=True)
    assert lin["n_corr"] == n
    check_system(f"lattice {seed} k={k}", out, 0, lin, n)


def test_faces_and_duplicates():
    """Rows on voxel faces, repeated rows and one voxel of 30 000 rows: the same voxels in the same order."""
    cloud = F.faces_and_duplicates(FACES_SEED)
    ds = G.voxel_down_sample(cloud, 0.5)
    for stride in (3, 4):
        out = staged([cloud], [cloud[:1]], [np.eye(4)], stride=stride)
        assert out["counts"][0] == len(ds) and out["counts"][1] == 1
        assert np.max(np.abs(out["points"][:len(ds)] - ds)) <= 1e-6
    store, _ = store_of([cloud])
    assert store.cloud(0)["points"].cpu().numpy().tobytes() == out["points"][:len(ds)].tobytes()


@pytest.mark.parametrize("name", list(F.END_TO_END))
def test_end_to_end(name):
    build, params, (t_bar, r_bar) = F.END_TO_END[name]
    A, B, T_true = build()
    ref = G.register(A, B, exact=True, **params)
    out = run([A], [B], **params)
    T = out["transform"][0]
    print(f"{name}: iterations {out['iterations'][0]} / {ref['iterations']}, "
          f"dt {np.abs(T[:3, 3] - ref['transform'][:3, 3]).max():.3g}, "
          f"dR {np.abs(T[:3, :3] - ref['transform'][:3, :3]).max():.3g}")
    assert np.abs(T[:3, 3] - ref["transform"][:3, 3]).max() <= 1e-3
    assert np.abs(T[:3, :3] - ref["transform"][:3, :3]).max() <= 1e-4
    assert abs(out["fitness"][0] - ref["fitness"]) <= 1e-3
    info = ref["information"]
    assert np.abs(out["information"][0] - info).max() <= 1e-3 * np.abs(info).max()
    te, re = G.pose_error(T, T_true)
    # within the end-to-end tolerance of the reference, the kernel recovers the motion as well as the reference does
    assert te <= t_bar + 2e-3 and re <= r_bar + 5e-4, (name, te, np.rad2deg(re))


@pytest.fixture(scope="module")
def small():
    S, T = F.many_small(MANY_SMALL_SEED)
    return S, T, raw(S, T)


def test_many_small_against_restatement(small):
    """300 pairs of 0 .. 300 rows in one call (tables of 2 .. 16 slots, probes that wrap, empty / NaN / one-row /
    two-row clouds mid-batch): every cloud's stage outputs and every pair's system at the identity."""
    S, T, _ = small
    P = len(S)
    out = staged(S, T, np.tile(np.eye(4), (P, 1, 1)))
    so = np.concatenate([[0], np.cumsum([len(c) for c in S])])
    to = so[-1] + np.concatenate([[0], np.cumsum([len(c) for c in T])])
    params = dict(G.DEFAULTS)
    wraps = 0
    for p in range(P):
        ra, rb = F.cloud_reference(S[p], params), F.cloud_reference(T[p], params)
        assert ra["sep"].all() and rb["sep"].all() and min(ra["gap"], rb["gap"]) > MIN_GAP      # nothing left out
        wraps += G.table_surely_wraps(S[p], 0.5)[0] + G.table_surely_wraps(T[p], 0.5)[0]
        for what, r, at, c in (("source", ra, so[p], p), ("target", rb, to[p], P + p)):
            cnt = int(out["counts"][c])
            assert cnt == len(r["ds"]), (p, what)
            if cnt:
                assert np.max(np.abs(out["points"][at:at + cnt] - r["ds"])) <= 1e-6, (p, what)
                C = r["cov"]
                err = np.abs(full3(out["covariances"][at:at + cnt]) - C).max(axis=(1, 2)) / np.linalg.norm(C, axis=(1, 2))
                assert err.max() <= 1e-4, (p, what, err.max())
        assert F.radius_margin(ra["ds"], rb["ds"], np.eye(4), 1.0) > RADIUS_MARGIN
        lin = G.linearize(ra["ds"], rb["ds"], ra["cov"], rb["cov"], np.eye(4), 1.0)
        if lin["n_corr"]:
            check_system(f"pair {p}", out, p, lin, len(ra["ds"]))
        else:
            assert out["n_correspondences"][p] == 0 and out["fitness"][p] == 0 and out["rmse"][p] == 0
            assert not out["system0"][p].any() and not out["information"][p].any()
    assert wraps >= 20


def test_many_small_store_and_independence(small):
    """The same pairs through a store filled by one add of 600 clouds and by several, with invalid ids in the second
    block of prepared_setup_kernel: raw against prepared bit for bit; any pair alone equals itself in the batch."""
    S, T, full = small
    P = len(S)
    one, ids = store_of(S + T)
    assert ids == list(range(2 * P))
    several = _gv().PreparedClouds()
    clouds, at = S + T, 0
    for step in (7, 1, 100, 256, 3, 2 * P):
        several.add(clouds[at:at + step])
        at += step
    assert len(several) == 2 * P and several.n_rows == one.n_rows
    for store in (one, several):
        got = prepared(store, list(range(P)), store, list(range(P, 2 * P)))
        for i in range(P):
            assert_bitwise(got, i, full, i, "store")
    sids, tids = np.arange(P), np.arange(P, 2 * P)
    bad = {260: (-1, None), 275: (None, 2 * P), 299: (2 * P + 5, -3)}
    for i, (a, b) in bad.items():
        sids[i] = sids[i] if a is None else a
        tids[i] = tids[i] if b is None else b
    got = prepared(one, sids, several, tids)
    for i in range(P):
        if i in bad:
            for k in ("transform", "fitness", "rmse", "information"):
                assert np.all(np.isnan(got[k][i])), (i, k)
            assert got["n_correspondences"][i] == -1 and got["iterations"][i] == 0
        else:
            assert_bitwise(got, i, full, i, "beside invalid ids")
    for i in (0, 3, P // 2, P // 2 + 4, P // 2 + 7, 257, P - 1):
        alone = raw([S[i]], [T[i]])
        assert_bitwise(alone, 0, full, i, "alone")
    assert (full["n_correspondences"] > 0).sum() > 200


def test_tiny_clouds_one_add():
    """1 100 clouds of one to five rows in a single add: store_kernel's prefix over the batch's earlier counts runs
    past its 1 024 threads."""
    tiny = F.tiny_clouds(TINY_SEED)
    n = len(tiny)
    store, ids = store_of(tiny)
    assert ids == list(range(n))
    ds = [G.voxel_down_sample(c, 0.5) for c in tiny]
    off = np.concatenate([[0], np.cumsum([len(d) for d in ds])])
    assert np.array_equal(store._row_host, off)
    pts = store._buf["points"][:store.n_rows].cpu().numpy()
    assert np.max(np.abs(pts - np.concatenate(ds))) <= 1e-6
    cov = full3(store._buf["covariances"][:store.n_rows].cpu().numpy())
    params = dict(G.DEFAULTS)
    C = np.concatenate([F.cloud_reference(c, params)["cov"] for c in tiny])
    sep = np.concatenate([F.cloud_reference(c, params)["sep"] for c in tiny])
    assert 1.0 - sep.mean() <= MASK_CAP
    assert (np.abs(cov - C).max(axis=(1, 2)) / np.linalg.norm(C, axis=(1, 2)))[sep].max() <= 1e-4
    tids = [(i + 1) % n for i in range(n)]
    got = prepared(store, ids, store, tids)
    ref = raw(tiny, [tiny[t] for t in tids])
    for i in range(n):
        assert_bitwise(got, i, ref, i, "tiny")


def _meaningful(out, offsets):
    """stage rows that the call defines: the first counts[c] rows of every cloud"""
    rows = np.concatenate([np.arange(o, o + c) for o, c in zip(offsets, out["counts"])]).astype(np.int64)
    return out["points"][rows], out["covariances"][rows]


def test_split_calls_change_nothing(small, monkeypatch):
    """With the per-call limits lowered to 3, register_packed, PreparedClouds.add, register_prepared and
    batch_loop_closing split 10 pairs into several library calls; the results are those of one call, bit for bit."""
    gv = _gv()
    S, T = small[0][:10], small[1][:10]
    whole = run(S, T, stages=True)
    whole_store, _ = store_of(S + T)
    whole_prepared = prepared(whole_store, list(range(10)), whole_store, list(range(10, 20)))
    calls = []
    lib_call = gv._lib.check
    monkeypatch.setattr(gv._lib, "check", lambda status, what: (calls.append(what), lib_call(status, what))[1])
    monkeypatch.setattr(gv, "MAX_PAIRS_PER_CALL", 3)
    monkeypatch.setattr(gv, "MAX_CLOUDS_PER_CALL", 3)
    monkeypatch.setattr(gv, "MAX_PREPARED_PAIRS_PER_CALL", 3)
    split = run(S, T, stages=True)
    assert calls.count("nsc_gicp_register") == 4
    for k in KEYS + ("system0", "counts"):
        assert split[k].tobytes() == whole[k].tobytes(), k
    offsets = np.concatenate([np.cumsum([0] + [len(c) for c in S])[:-1],
                              sum(len(c) for c in S) + np.cumsum([0] + [len(c) for c in T])[:-1]])
    for a, b in zip(_meaningful(split, offsets), _meaningful(whole, offsets)):
        assert a.tobytes() == b.tobytes()
    store, ids = store_of(S + T)
    assert ids == list(range(20)) and calls.count("nsc_gicp_prepare") == 7
    assert np.array_equal(store._row_host, whole_store._row_host)
    for k in ("points", "covariances"):
        assert torch.equal(store._buf[k][:store.n_rows], whole_store._buf[k][:store.n_rows]), k
    got = prepared(store, list(range(10)), store, list(range(10, 20)))
    assert calls.count("nsc_gicp_register_prepared") == 4
    for i in range(10):
        assert_bitwise(got, i, whole_prepared, i, "split")
        assert_bitwise(got, i, whole, i, "split against raw")

    from neural_spectral_codec_amd.retrieval import GeometricVerifier, batch_loop_closing
    rng = np.random.default_rng(0)
    desc = rng.random((7, 800)).astype(np.float32)
    desc /= desc.sum(1, keepdims=True)
    T_true = G.delta_transform(F.MOTION)
    db = [SimpleNamespace(keyframe_id=100 + i, scan_id=i, points=F.moved(F.surface(40 + i, 1500), T_true),
                          descriptor=desc[i], pose=None) for i in range(4)]
    queries = [SimpleNamespace(keyframe_id=7 + i, scan_id=7 + i, points=F.surface(50 + i, 1500),
                               descriptor=desc[4 + i], pose=None) for i in range(3)]
    kw = dict(top_k=4, verify=True, edge_fn=_edge_fn, prepare_geometry=True)
    del calls[:]
    split_edges = batch_loop_closing(queries, db, verifier=GeometricVerifier(), **kw)
    assert calls.count("nsc_gicp_register_prepared") == 4 and calls.count("nsc_gicp_prepare") == 2 + 1   # 12 pairs
    monkeypatch.undo()
    whole_edges = batch_loop_closing(queries, db, verifier=GeometricVerifier(), **kw)
    assert set(split_edges) == set(whole_edges) == {0, 1, 2}
    for i in whole_edges:
        _same_closures(whole_edges[i], split_edges[i])
    assert sum(len(e) for e in whole_edges.values()) >= 6
