"""Stage-2 verification on the MI355X: nsc_gicp_register against the float64 restatement (tests/gicp_restatement.py),
stage by stage and end to end; determinism, edge cases, int64 offsets, TwoStageRetrieval and hipGraph capture."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gicp_restatement as G
from neural_spectral_codec_amd import synth
from test_gicp_cpu import R_BAR, REVISITS, T_BAR, revisit

pytestmark = pytest.mark.gpu


def _gv():
    from neural_spectral_codec_amd.retrieval import geometric_verification as gv
    return gv


def dev_pack(clouds, stride=4):
    pts = [np.asarray(c, np.float32)[:, :stride] if len(c) else np.zeros((0, stride), np.float32) for c in clouds]
    off = np.zeros(len(pts) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in pts])
    return (torch.from_numpy(np.concatenate(pts, 0)).cuda(), torch.from_numpy(off).cuda())


def run(sources, targets, inits=None, stages=False, stride=4, **params):
    sp, so = dev_pack(sources, stride)
    tp, to = dev_pack(targets, stride)
    P = len(sources)
    init = np.tile(np.eye(4), (P, 1, 1)) if inits is None else np.asarray(inits, np.float64)
    out = _gv().register_packed(sp, so, tp, to, torch.from_numpy(init).cuda(), stages=stages, **params)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def pairs():
    return [revisit(o, g) for o, g in REVISITS]


@pytest.fixture(scope="module")
def negative():
    A = synth.scan_world(synth.make_world(3), synth.pose_xyz_yaw(0, 0), seed=1)
    B = synth.scan_world(synth.make_world(11, ground_z=-4.0), synth.pose_xyz_yaw(0, 0), seed=5)
    return A, B


def test_stage_parity(pairs):
    A, B, T_true, _ = pairs[1]
    T_fix = T_true @ G.delta_transform(np.array([0.01, -0.01, 0.02, 0.1, -0.05, 0.02]))
    out = run([A], [B], [T_fix], stages=True, max_iteration=0)
    ns = len(A)
    for cloud, rows, cnt in ((A, slice(0, ns), out["counts"][0]), (B, slice(ns, None), out["counts"][1])):
        ds = G.voxel_down_sample(cloud, 0.5)
        assert cnt == len(ds)
        got = out["points"][rows][:cnt]
        assert np.max(np.abs(got - ds)) <= 1e-6
        # k-NN sets equal except at ties of the 20th / 21st distance: compare covariances built from the oracle sets
        idx, d = G.knn(ds, 20)
        tie = np.abs(d[:, 20] - d[:, 19]) <= 1e-5 * d[:, 20]
        C = G.covariances(ds)
        cg = out["covariances"][rows][:cnt]
        full = np.stack([cg[:, [0, 1, 2]], cg[:, [1, 3, 4]], cg[:, [2, 4, 5]]], 1)
        # a repeated smallest eigenvalue leaves the plane normal undefined: compare where it is well separated
        nb = ds[idx]
        cc = nb - nb.mean(1, keepdims=True)
        w = np.linalg.eigvalsh(np.einsum("nki,nkj->nij", cc, cc) / 20)
        sep = (w[:, 1] - w[:, 0]) > 1e-3 * np.maximum(w[:, 2], 1e-12)
        ok = ~tie & sep
        assert ok.mean() > 0.9
        err = np.abs(full - C)[ok].max(axis=(1, 2)) / np.linalg.norm(C[ok], axis=(1, 2))
        assert err.max() <= 1e-4, err.max()
    # one linearisation at a fixed T
    src, tgt = G.voxel_down_sample(A, 0.5), G.voxel_down_sample(B, 0.5)
    lin = G.linearize(src, tgt, G.covariances(src), G.covariances(tgt), T_fix, 1.0)
    s0 = out["system0"][0]
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = s0[:21]
    H = H + np.triu(H, 1).T
    assert abs(s0[27] - lin["n_corr"]) <= 0.001 * lin["n_corr"]            # rows at the radius may flip
    q, i, j = G.correspondences(src, tgt, T_fix, 1.0)
    d = np.linalg.norm(q[i] - tgt[j], axis=1)
    if not np.any(np.abs(d - 1.0) < 1e-9):
        assert s0[27] == lin["n_corr"]
        assert np.allclose(H, lin["H"], rtol=1e-6, atol=1e-6 * np.abs(lin["H"]).max())
        assert np.allclose(s0[21:27], lin["g"], rtol=1e-6, atol=1e-6 * np.abs(lin["g"]).max())
        assert abs(out["fitness"][0] - lin["fitness"]) <= 1e-6 * lin["fitness"]
        assert abs(out["rmse"][0] - lin["rmse"]) <= 1e-6 * lin["rmse"]
        assert np.allclose(out["information"][0], lin["info"], rtol=1e-6, atol=1e-6 * np.abs(lin["info"]).max())


def test_end_to_end_matches_restatement(pairs):
    srcs, tgts, inits = [p[0] for p in pairs], [p[1] for p in pairs], [np.eye(4) if p[3] is None else p[3]
                                                                      for p in pairs]
    out = run(srcs, tgts, inits)
    for i, (A, B, T_true, init) in enumerate(pairs):
        ref = G.register(A, B, init=init)
        T = out["transform"][i]
        assert np.abs(T[:3, 3] - ref["transform"][:3, 3]).max() <= 1e-3
        assert np.abs(T[:3, :3] - ref["transform"][:3, :3]).max() <= 1e-4
        assert abs(out["fitness"][i] - ref["fitness"]) <= 1e-3
        info = ref["information"]
        assert np.abs(out["information"][i] - info).max() <= 1e-3 * np.abs(info).max()
        te, re = G.pose_error(T, T_true)
        assert te <= T_BAR and re <= R_BAR, (i, te, np.rad2deg(re))


def test_verifier_decisions(pairs, negative):
    v = _gv().GeometricVerifier()
    A, B, T_true, _ = pairs[0]
    ok, T, info = v.verify(A, B)
    assert ok and set(info) == {"fitness", "rmse", "information_matrix", "n_correspondences", "iterations"}
    assert T.shape == (4, 4) and T.dtype == np.float64 and info["information_matrix"].shape == (6, 6)
    ok, _, info = v.verify(*negative)
    assert not ok
    with pytest.raises(Exception):
        _gv().GeometricVerifier(method="point_to_plane")


def test_deterministic_and_batch_independent(pairs, negative):
    v = _gv().GeometricVerifier()
    A = pairs[0][0]
    cands = [pairs[0][1], negative[1], pairs[1][1], pairs[2][1]]
    b1 = v.verify_batch(A, cands)
    b2 = v.verify_batch(A, cands)
    single = [v.verify(A, c) for c in cands]
    other = v.verify_batch(A, [negative[1], pairs[2][1], pairs[0][1]])
    for x, y, z in zip(b1, b2, single):
        assert x[0] == y[0] == z[0]
        assert np.array_equal(x[1], y[1]) and np.array_equal(x[1], z[1])
        assert np.array_equal(x[2]["information_matrix"], z[2]["information_matrix"])
        assert x[2]["fitness"] == z[2]["fitness"] and x[2]["rmse"] == z[2]["rmse"]
    assert np.array_equal(other[2][1], b1[0][1]) and np.array_equal(other[1][1], b1[3][1])


def test_edges(pairs):
    A = pairs[0][0]
    nan = np.full((500, 4), np.nan, np.float32)
    empty = np.zeros((0, 4), np.float32)
    tiny = A[:15]                       # fewer than 20 rows
    two = A[:2]                         # fewer than 3
    far = A.copy()
    far[:, :3] += 500.0                  # no correspondence in range
    srcs = [empty, nan, A, A, tiny, two, A]
    tgts = [A, A, empty, nan, A, A, far]
    out = run(srcs, tgts)
    for i in range(4):
        assert out["fitness"][i] == 0 and out["n_correspondences"][i] == 0
        assert np.array_equal(out["transform"][i], np.eye(4))
    v = _gv().GeometricVerifier()
    res = v.verify_batch(A, [far, empty])
    assert not res[0][0] and not res[1][0] and np.array_equal(res[0][1], np.eye(4))
    for i, s in ((4, tiny), (5, two)):
        ref = G.register(s, A)
        assert out["n_correspondences"][i] == ref["n_corr"]
        assert abs(out["fitness"][i] - ref["fitness"]) <= 1e-3
        assert np.abs(out["transform"][i] - ref["transform"]).max() <= 1e-3
    assert out["n_correspondences"][6] == 0 and np.array_equal(out["transform"][6], np.eye(4))


def test_int64_offsets(pairs):
    """One batch whose last pair starts past 2^31 floats of the packed source: pair 0's source repeats one scan."""
    A, B = pairs[0][0], pairs[0][1]
    reps = (2 ** 29) // len(A) + 1
    a = torch.from_numpy(A).cuda()
    big = a.repeat(reps, 1)
    src = torch.cat([big, a], 0)
    del big
    assert (src.shape[0] - len(A)) * 4 > 2 ** 31
    so = torch.tensor([0, reps * len(A), reps * len(A) + len(A)], dtype=torch.int64, device="cuda")
    tgt = torch.from_numpy(np.concatenate([B, B])).cuda()
    to = torch.tensor([0, len(B), 2 * len(B)], dtype=torch.int64, device="cuda")
    from neural_spectral_codec_amd import _lib
    nbytes = _lib.lib().nsc_gicp_workspace_bytes(2, int(src.shape[0]), int(tgt.shape[0]))
    print(f"int64-offset batch: {src.shape[0]} source rows, workspace {nbytes} bytes")
    init = torch.eye(4, dtype=torch.float64, device="cuda").repeat(2, 1, 1)
    out = _gv().register_packed(src, so, tgt, to, init)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    del src, out
    torch.cuda.empty_cache()
    one = run([A], [B])
    for i in (0, 1):                     # repeated rows give the same voxels: bit-identical to the single scan
        assert np.array_equal(got["transform"][i], one["transform"][0])
        assert got["fitness"][i] == one["fitness"][0]


def test_two_stage_integration(pairs, negative):
    from neural_spectral_codec_amd.retrieval import GeometricVerifier, create_two_stage_retrieval
    A = pairs[0][0]
    scans = [pairs[0][1], pairs[1][1], negative[1]]
    rng = np.random.default_rng(0)
    desc = rng.random((4, 800)).astype(np.float32)
    desc /= desc.sum(1, keepdims=True)
    kfs = [SimpleNamespace(keyframe_id=100 + i, scan_id=i, points=s, descriptor=desc[i], pose=None)
           for i, s in enumerate(scans)]
    query = SimpleNamespace(keyframe_id=7, scan_id=7, points=A, descriptor=desc[3], pose=None)

    def edge_fn(source_pose, target_pose, relative_transform, information_matrix):
        return {"transform": relative_transform, "information": information_matrix}
    r = create_two_stage_retrieval(top_k=3, verifier=GeometricVerifier(), edge_fn=edge_fn)
    r.add_keyframes(kfs)
    closures = r.get_loop_closures(query)
    got = {c["target_id"]: c for c in closures}
    assert set(got) == {100, 101}                         # the unrelated world is dropped
    for tid, (_, _, T_true, init) in ((100, pairs[0]), (101, pairs[1])):
        te, re = G.pose_error(got[tid]["transform"], T_true)
        assert te <= T_BAR and re <= R_BAR


def test_capture_replays_bit_identical(pairs):
    from _hipgraph import keep_graphs, node_types
    A, B = pairs[0][0], pairs[0][1]
    sp, so = dev_pack([A, A])
    tp, to = dev_pack([B, pairs[1][1]])
    init = torch.eye(4, dtype=torch.float64, device="cuda").repeat(2, 1, 1)
    gv = _gv()
    eager = {k: v.clone() for k, v in gv.register_packed(sp, so, tp, to, init).items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gv.register_packed(sp, so, tp, to, init)          # warm the allocator outside the capture
    torch.cuda.current_stream().wait_stream(s)
    with keep_graphs() as made:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cap = gv.register_packed(sp, so, tp, to, init)
    g.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(eager[k], cap[k]), k
    types = node_types(made[0])
    assert types.get("memset", 0) == 0 and types.get("memcpy", 0) == 0, types
    assert types.get("kernel", 0) == 4 + 2 * 31
