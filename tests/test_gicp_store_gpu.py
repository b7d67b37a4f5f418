"""The store of prepared clouds on the MI355X: PreparedClouds / register_prepared (nsc_gicp_prepare,
nsc_gicp_register_prepared) against register_packed on the same raw clouds, bit for bit -- stage outputs, every
registration output, index forms, edge clouds, invalid ids, growth, capture -- and the loop-closing paths built on
them."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gicp_restatement as G
from neural_spectral_codec_amd import synth
from test_gicp_cpu import R_BAR, REVISITS, T_BAR, revisit
from test_gicp_gpu import dev_pack, run

pytestmark = pytest.mark.gpu

KEYS = ("transform", "fitness", "rmse", "n_correspondences", "iterations", "information")


def _gv():
    from neural_spectral_codec_amd.retrieval import geometric_verification as gv
    return gv


@pytest.fixture(scope="module")
def pairs():
    return [revisit(o, g) for o, g in REVISITS]


@pytest.fixture(scope="module")
def other():
    return synth.scan_world(synth.make_world(11, ground_z=-4.0), synth.pose_xyz_yaw(0, 0), seed=5)


def store_of(clouds, stride=4, **kw):
    s = _gv().PreparedClouds(**kw)
    pts, off = dev_pack(clouds, stride)
    return s, s.add_packed(pts, off)


def prepared(src, sids, tgt, tids, inits=None, **params):
    out = _gv().register_prepared(src, sids, tgt, tids, inits, **params)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def raw(sources, targets, inits=None, stride=4, **params):
    sp, so = dev_pack(sources, stride)
    tp, to = dev_pack(targets, stride)
    P = len(sources)
    init = np.tile(np.eye(4), (P, 1, 1)) if inits is None else np.asarray(inits, np.float64)
    out = _gv().register_packed(sp, so, tp, to, torch.from_numpy(init).cuda(), **params)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_bitwise(a, i, b, j, what=""):
    for k in KEYS:
        x, y = np.ascontiguousarray(a[k][i]), np.ascontiguousarray(b[k][j])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, i, j, k, x, y)


def test_stage_parity(pairs, other):
    clouds = [p[0] for p in pairs] + [p[1] for p in pairs] + [other]
    out = run(clouds, clouds, stages=True, max_iteration=0)
    _, so = dev_pack(clouds)
    so = so.cpu().numpy()
    store, ids = store_of(clouds)
    assert ids == list(range(len(clouds))) and len(store) == len(clouds)
    for c in ids:
        cnt = int(out["counts"][c])
        got = store.cloud(c)
        assert got["points"].shape == (cnt, 3) and got["covariances"].shape == (cnt, 6)
        rows = slice(so[c], so[c] + cnt)
        assert got["points"].cpu().numpy().tobytes() == out["points"][rows].tobytes(), c
        assert got["covariances"].cpu().numpy().tobytes() == out["covariances"][rows].tobytes(), c
    assert store.n_rows == int(out["counts"][:len(clouds)].sum())


def test_packed_ranges():
    """``PreparedClouds.packed``: every range of a store of three clouds of 0, 5 and 300 rows (one row per voxel, so the
    store keeps them all) is the clouds' points by bits under offsets counted from 0; an empty store gives no rows and the
    offsets [0]; a bad range is refused."""
    from neural_spectral_codec_amd import _lib
    lattice = np.stack(np.meshgrid(np.arange(10.0), np.arange(10.0), np.arange(3.0), indexing="ij"), -1).reshape(-1, 3)
    sizes = [0, 5, 300]
    store, ids = store_of([np.zeros((0, 3)), lattice[:5] + 100.0, lattice], stride=3)
    stored = [store.cloud(i)["points"].cpu().numpy() for i in ids]
    assert [len(p) for p in stored] == sizes and store.n_rows == 305
    for start in range(4):
        for stop in range(start, 4):
            pts, off = store.packed(start, stop)
            assert pts.is_cuda and off.is_cuda and pts.dtype == torch.float64 and off.dtype == torch.int64
            want = np.concatenate(stored[start:stop] + [np.zeros((0, 3))])
            assert tuple(pts.shape) == want.shape and pts.cpu().numpy().tobytes() == want.tobytes(), (start, stop)
            assert off.cpu().tolist() == np.concatenate([[0], np.cumsum(sizes[start:stop])]).tolist(), (start, stop)
    for got in (store.packed(), store.packed(0), store.packed(0, None)):
        assert got[0].data_ptr() == store.packed(0, 3)[0].data_ptr() and tuple(got[0].shape) == (305, 3)
        assert got[1].cpu().tolist() == [0, 0, 5, 305]
    assert store.packed(2)[1].cpu().tolist() == [0, 300]
    for start, stop in ((-1, None), (4, None), (2, 1), (0, 4), (-2, -1)):
        with pytest.raises(_lib.NscError, match="start and stop must satisfy"):
            store.packed(start, stop)
    for empty in (_gv().PreparedClouds(), store):
        empty.clear()
        pts, off = empty.packed()
        assert tuple(pts.shape) == (0, 3) and pts.dtype == torch.float64 and pts.is_cuda and off.cpu().tolist() == [0]
        with pytest.raises(_lib.NscError, match="start and stop must satisfy"):
            empty.packed(0, 1)


@pytest.mark.parametrize("stride", [3, 4])
def test_registration_parity(pairs, other, stride):
    srcs = [p[0] for p in pairs] + [pairs[0][0]]
    tgts = [p[1] for p in pairs] + [other]                      # the last pair: another world
    inits = [np.eye(4) if p[3] is None else p[3] for p in pairs] + [np.eye(4)]
    P = len(srcs)
    store, ids = store_of(srcs + tgts, stride=stride)
    sids, tids = ids[:P], ids[P:]
    for kw in (dict(inits=inits), dict(inits=None), dict(inits=inits, max_correspondence_distance=1.5)):
        ref = raw(srcs, tgts, stride=stride, **kw)
        got = prepared(store, sids, store, tids, **kw)
        for i in range(P):
            assert_bitwise(got, i, ref, i, kw)
    assert ref["n_correspondences"][:-1].min() > 0


def test_index_forms(pairs, other):
    A, B0, B1, B2 = pairs[0][0], pairs[0][1], pairs[1][1], pairs[2][1]
    clouds = [A, B0, B1, B2, other]
    store, ids = store_of(clouds)
    # cloud 1 is a source in two pairs and a target in two others; (2, 2) is a self-pair
    pl = [(0, 1), (1, 0), (1, 2), (2, 1), (0, 3), (2, 2), (4, 0)]
    got = prepared(store, [a for a, _ in pl], store, [b for _, b in pl])
    ref = raw([clouds[a] for a, _ in pl], [clouds[b] for _, b in pl])
    for i in range(len(pl)):
        assert_bitwise(got, i, ref, i, pl[i])
    assert np.array_equal(got["transform"][5], np.eye(4)) and got["fitness"][5] == 1.0
    # any batch, any order: each pair's result depends on that pair alone
    perm = [6, 2, 5, 0, 4, 1, 3]
    shuffled = prepared(store, [pl[k][0] for k in perm], store, [pl[k][1] for k in perm])
    for i, k in enumerate(perm):
        assert_bitwise(shuffled, i, got, k, "order")
    single = prepared(store, [1], store, [2])
    assert_bitwise(single, 0, got, 2, "single")
    # sources from another store than the targets
    queries, _ = store_of([A, B1])
    targets, _ = store_of([B0, B1, B2])
    got = prepared(queries, [0, 0, 1], targets, [0, 2, 0])
    ref = raw([A, A, B1], [B0, B2, B0])
    for i in range(3):
        assert_bitwise(got, i, ref, i, "two stores")


def test_edge_clouds(pairs):
    A = pairs[0][0]
    rng = np.random.default_rng(7)
    one_voxel = np.concatenate([rng.uniform(3.0, 3.1, (400, 3)), np.zeros((400, 1))], 1).astype(np.float32)
    edges = [np.zeros((0, 4), np.float32), np.full((300, 4), np.nan, np.float32), A[:1], A[:2], one_voxel,
             np.concatenate([A[:500], one_voxel])]
    clouds = [A] + edges
    store, ids = store_of(clouds)
    pl = [(e, 0) for e in range(1, len(clouds))] + [(0, e) for e in range(1, len(clouds))] + [(4, 3), (3, 4)]
    got = prepared(store, [a for a, _ in pl], store, [b for _, b in pl])
    ref = raw([clouds[a] for a, _ in pl], [clouds[b] for _, b in pl])
    for i in range(len(pl)):
        assert_bitwise(got, i, ref, i, pl[i])
    assert len(store.cloud(1)["points"]) == 0 and len(store.cloud(2)["points"]) == 0
    assert len(store.cloud(5)["points"]) == 1


def test_invalid_ids(pairs):
    A, B = pairs[0][0], pairs[0][1]
    store, _ = store_of([A, B])
    sids = torch.tensor([0, -1, 2, 1, 0], dtype=torch.int64, device="cuda")
    tids = torch.tensor([1, 0, 0, 7, 1 << 40], dtype=torch.int64, device="cuda")
    got = prepared(store, sids, store, tids)
    ref = raw([A, B], [B, A])
    assert_bitwise(got, 0, ref, 0, "valid")
    for i in (1, 2, 3, 4):
        for k in ("transform", "fitness", "rmse", "information"):
            assert np.all(np.isnan(got[k][i])), (i, k)
        assert got["n_correspondences"][i] == -1 and got["iterations"][i] == 0
    got = prepared(store, [1, 5, 0], store, [0, 0, 1])       # the valid pairs beside it are unchanged
    assert_bitwise(got, 0, ref, 1, "beside")
    assert_bitwise(got, 2, ref, 0, "beside")


def test_growth_and_clear(pairs, other):
    scans = [p[0] for p in pairs] + [p[1] for p in pairs] + [other]
    clouds = [s[k::8] for k in range(3) for s in scans]                  # 33 clouds of ~16k rows
    store = _gv().PreparedClouds()
    sizes = []
    for c in clouds:
        store.add([c])
        sizes.append(store.nbytes)
    assert len(set(sizes)) >= 3, sizes                                    # at least two capacity doublings
    n = len(clouds)
    ref = raw(clouds, [clouds[0]] * n)
    got = prepared(store, list(range(n)), store, [0] * n)
    for i in range(n):
        assert_bitwise(got, i, ref, i, "grown")
    nbytes = store.nbytes
    store.clear()
    assert len(store) == 0 and store.n_rows == 0
    assert store.add(clouds[5:8]) == [0, 1, 2] and store.nbytes == nbytes
    got = prepared(store, [0, 1, 2], store, [2, 0, 1])
    ref = raw(clouds[5:8], [clouds[7], clouds[5], clouds[6]])
    for i in range(3):
        assert_bitwise(got, i, ref, i, "re-added")


def test_capture_replays_bit_identical(pairs):
    from _hipgraph import keep_graphs, node_types
    store, _ = store_of([pairs[0][0], pairs[0][1], pairs[1][1]])
    sids = torch.tensor([0, 0, 2], dtype=torch.int64, device="cuda")
    tids = torch.tensor([1, 2, 0], dtype=torch.int64, device="cuda")
    init = torch.eye(4, dtype=torch.float64, device="cuda").repeat(3, 1, 1)
    gv = _gv()
    eager = {k: v.clone() for k, v in gv.register_prepared(store, sids, store, tids, init).items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gv.register_prepared(store, sids, store, tids, init)          # warm the allocator outside the capture
    torch.cuda.current_stream().wait_stream(s)
    with keep_graphs() as made:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cap = gv.register_prepared(store, sids, store, tids, init)
    g.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(eager[k], cap[k]), k
    types = node_types(made[0])
    assert types.get("memset", 0) == 0 and types.get("memcpy", 0) == 0, types
    assert types.get("kernel", 0) == 1 + 2 * 31


def _pair_rows(res):
    """a register_* dict of device tensors or a verify_* list -> per pair (transform bytes, fitness, rmse,
    n_correspondences, iterations, information bytes)"""
    if isinstance(res, dict):
        torch.cuda.synchronize()
        h = {k: res[k].cpu().numpy() for k in KEYS}
        return [(h["transform"][i].tobytes(), float(h["fitness"][i]), float(h["rmse"][i]),
                 int(h["n_correspondences"][i]), int(h["iterations"][i]), h["information"][i].tobytes())
                for i in range(len(h["fitness"]))]
    return [(T.tobytes(), info["fitness"], info["rmse"], info["n_correspondences"], info["iterations"],
             info["information_matrix"].tobytes()) for _, T, info in res]


def test_init_transform_forms():
    """Every entry point takes ``init_transforms`` as a host float64 array or a device float64 tensor and, for the
    identity, as None or an explicit array; whatever the form and the entry point, raw or stored, the results are
    the same bits.  Two pairs of 400-row patches of one surface, the targets moved by about 4 degrees of yaw and
    0.2 m; the guess is that yaw and shift."""
    import gicp_clouds as GC
    gv = _gv()
    guess = synth.pose_xyz_yaw(0.2, 0.0, 0.0, 4.0)
    T_true = guess @ G.delta_transform(0.2 * GC.MOTION)
    A = GC.surface(0, 400, ext=6.0, relief=0.5)
    B = [GC.moved(GC.surface(1000 + j, 400, ext=6.0, relief=0.5), T_true) for j in range(2)]
    v = gv.GeometricVerifier()
    query, store = v.prepare([A]), v.prepare(B)
    calls = {"register_batch": lambda X: gv.register_batch([A, A], B, X),
             "register_prepared": lambda X: gv.register_prepared(query, [0, 0], store, [0, 1], X),
             "verify_batch": lambda X: v.verify_batch(A, B, X),
             "verify_prepared": lambda X: v.verify_prepared(query, 0, store, [0, 1], X),
             "verify_pairs": lambda X: v.verify_pairs(query, [0, 0], store, [0, 1], X)}
    guesses, eyes = np.stack([guess, guess]).astype(np.float64), np.tile(np.eye(4), (2, 1, 1))
    found = []
    for forms in ((guesses, torch.from_numpy(guesses).cuda()), (None, eyes, torch.from_numpy(eyes).cuda())):
        ref = None
        for name, call in calls.items():
            for X in forms:
                rows = _pair_rows(call(X))
                if ref is None:
                    ref = rows
                    assert len(ref) == 2 and all(r[3] > 0 for r in ref), ref
                assert rows == ref, (name, type(X))
        found.append(ref)
    assert found[0][0][0] != found[1][0][0]              # the guess is used: another start, other last bits


def _edge_fn(source_pose, target_pose, relative_transform, information_matrix):
    return {"transform": relative_transform, "information": information_matrix}


def _scenario(pairs, other):
    rng = np.random.default_rng(0)
    desc = rng.random((5, 800)).astype(np.float32)
    desc /= desc.sum(1, keepdims=True)
    scans = [pairs[0][1], pairs[1][1], other]
    kfs = [SimpleNamespace(keyframe_id=100 + i, scan_id=i, points=s, descriptor=desc[i], pose=None)
           for i, s in enumerate(scans)]
    queries = [SimpleNamespace(keyframe_id=7, scan_id=7, points=pairs[0][0], descriptor=desc[3], pose=None),
               SimpleNamespace(keyframe_id=8, scan_id=8, points=pairs[2][0], descriptor=desc[4], pose=None)]
    return kfs, queries


def _same_closures(a, b):
    assert [e["target_id"] for e in a] == [e["target_id"] for e in b]
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k


def test_two_stage_prepared_equals_default(pairs, other):
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import GeometricVerifier, create_two_stage_retrieval
    kfs, queries = _scenario(pairs, other)
    with pytest.raises(_lib.NscError):
        create_two_stage_retrieval(top_k=3, verifier=None, prepare_geometry=True)
    systems = []
    for prep in (False, True):
        r = create_two_stage_retrieval(top_k=3, verifier=GeometricVerifier(), edge_fn=_edge_fn,
                                       prepare_geometry=prep)
        r.add_keyframes(kfs[:2])
        r.add_keyframe(kfs[2])
        systems.append(r)
    d, p = systems
    assert len(p.geometry) == 3
    with pytest.raises(ValueError):
        p.add_keyframe(SimpleNamespace(keyframe_id=9, points=None, descriptor=kfs[0].descriptor, pose=None))
    for q in queries:
        cd, cp = d.query(q), p.query(q)
        assert [c.database_idx for c in cd] == [c.database_idx for c in cp]
        for x, y in zip(cd, cp):
            assert x.verified == y.verified and x.fitness == y.fitness and x.rmse == y.rmse
            assert x.transform.tobytes() == y.transform.tobytes()
            assert x.information_matrix.tobytes() == y.information_matrix.tobytes()
        _same_closures(d.get_loop_closures(q), p.get_loop_closures(q))
    assert {c["target_id"] for c in p.get_loop_closures(queries[0])} == {100, 101}
    p.clear_database()
    assert len(p.geometry) == 0 and p.query(queries[0]) == []


def test_batch_loop_closing_one_registration(pairs, other, monkeypatch):
    from neural_spectral_codec_amd.retrieval import GeometricVerifier, batch_loop_closing
    gv = _gv()
    kfs, queries = _scenario(pairs, other)
    per_query = batch_loop_closing(queries, kfs, top_k=3, verify=True, verifier=GeometricVerifier(),
                                   edge_fn=_edge_fn)
    calls = []
    orig = gv.register_prepared

    def counted(*a, **kw):
        calls.append(len(a[1]))
        return orig(*a, **kw)
    monkeypatch.setattr(gv, "register_prepared", counted)
    batched = batch_loop_closing(queries, kfs, top_k=3, verify=True, verifier=GeometricVerifier(),
                                 edge_fn=_edge_fn, prepare_geometry=True)
    assert calls == [2 * 3]                              # every query's candidates in one call
    assert set(batched) == set(per_query) == {0, 1}
    for i in per_query:
        _same_closures(per_query[i], batched[i])
    assert {e["target_id"] for e in batched[0]} == {100, 101}


def test_batch_loop_closing_finds_revisit():
    from neural_spectral_codec_amd.retrieval import GeometricVerifier, batch_loop_closing
    w = synth.make_world(3)
    poses = [synth.pose_xyz_yaw(3.0 * i, 0.5 * np.sin(i), 0.0, 2.0 * i) for i in range(8)]
    rng = np.random.default_rng(1)
    desc = rng.random((9, 800)).astype(np.float32)
    desc /= desc.sum(1, keepdims=True)
    db = [SimpleNamespace(keyframe_id=i, points=synth.scan_world(w, P, seed=10 + i), descriptor=desc[i], pose=None)
          for i, P in enumerate(poses)]
    PQ = synth.pose_xyz_yaw(0.6, -0.3, 0.0, 3.0)                     # back at the start
    q = SimpleNamespace(keyframe_id=99, points=synth.scan_world(w, PQ, seed=99), descriptor=desc[8], pose=None)
    out = batch_loop_closing([q], db, top_k=len(db), verify=True, verifier=GeometricVerifier(), edge_fn=_edge_fn,
                             prepare_geometry=True)
    edges = {e["target_id"]: e for e in out[0]}
    assert 0 in edges
    te, re = G.pose_error(edges[0]["transform"], np.linalg.inv(poses[0]) @ PQ)
    assert te <= T_BAR and re <= R_BAR, (te, np.rad2deg(re))
