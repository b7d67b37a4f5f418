"""The workspace contract on the MI355X ("Workspaces"): every entry point of include/nsc.h that takes
``(ws, ws_bytes)`` runs behind tests/workspace_contract.py's proxy, which hands it a workspace of exactly
``nsc_*_workspace_bytes()`` bytes, filled with a pattern, between two 4096-byte guards.

A scenario is a function over the smallest input of the suite's own case modules that reaches every launch of its entry
points.  It runs five times: twice without the proxy (the premise: two plain runs agree by bytes) and once per pattern
(0x00, 0xFF, 0x3C) behind it.  Compared:
  results    everything the scenario returns -- the returned tensors and the tensors updated in place -- equal by bytes
             across all runs.  One comparison is not of raw bytes, and the scenarios of the kept map say so: the map's
             ``index``, whose slot for a key depends on which of two keys wins a contested slot, is compared as the mapping
             key -> place, and the kept tensors over their defined rows [0, stats[1]), as tests/test_map_insert_gpu.py's
             ``assert_same_bits`` compares two maps
  workspace  proxy.verify(): no guard byte of any workspace handed out was written
  inputs     every device tensor a scenario hands to a wrapper equals a clone taken before the call, by bytes
  reach      the proxy intercepted the entry points COVERED claims for the scenario, each with a workspace above 0 bytes
"""
import ctypes as C

import numpy as np
import pytest
import torch

import encoder_families as EF
import gicp_clouds as GC
import keyframe_families as KF
import map_insert_cases as IK
import map_localize_cases as K
import posegraph_cov_restatement as V
import posegraph_restatement as P
import posegraph_robust_restatement as R
import workspace_contract as W
from _posegraph import optimizer, plain_linearize, plain_optimize
from neural_spectral_codec_amd import _lib
from test_cache_coherence_gpu import _train_setup
from test_encoder_paths_gpu import encoder
from test_gat_gpu import _model, irregular_graph
from test_gicp_families_cpu import MANY_SMALL_SEED
from test_map_insert_cpu import joined
from test_map_insert_gpu import KEPT
from test_map_localize_gpu import dev, index_of, localizer
from test_posegraph_cov_gpu import CAP
from test_retrieval_paths_gpu import MINE, mine_case, tied_distances

pytestmark = pytest.mark.gpu


# ---- the harness -----------------------------------------------------------------------------------------------------

def bits(t):
    """a tensor or an array as (dtype, shape, bytes): NaNs and signed zeros compare by their bits"""
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return str(a.dtype), tuple(a.shape), a.tobytes()


def flatten(res, path="result"):
    """nested dicts, lists and tuples of tensors, arrays and numbers -> [(path, value by bits)]"""
    if isinstance(res, dict):
        return [x for k in sorted(res, key=str) for x in flatten(res[k], f"{path}[{k!r}]")]
    if isinstance(res, (list, tuple)):
        return [x for i, v in enumerate(res) for x in flatten(v, f"{path}[{i}]")]
    if isinstance(res, (torch.Tensor, np.ndarray)):
        return [(path, bits(res))]
    return [(path, repr(res))]


def assert_same(want, got, what):
    assert [p for p, _ in want] == [p for p, _ in got], what
    for (path, a), (_, b) in zip(want, got):
        assert a == b, f"{what}: {path} differs"


class Inputs:
    """the device tensors a scenario hands to the wrappers, each with a clone taken before the call"""

    def __init__(self):
        self.held = []

    def __call__(self, t):
        t = t if isinstance(t, torch.Tensor) else dev(t)
        assert t.is_cuda
        self.held.append((t, t.clone()))
        return t

    def check(self):
        for i, (t, before) in enumerate(self.held):
            assert bits(t) == bits(before), f"input {i} {tuple(t.shape)} {t.dtype} was written"


def run(scenario, monkeypatch, pattern=None):
    """one run of a scenario, behind the proxy when a pattern is given -> (flattened results, the proxy or None)"""
    real = _lib.lib()
    assert not isinstance(real, W.WorkspaceProxy)
    proxy = None if pattern is None else W.WorkspaceProxy(real, pattern)
    if proxy is not None:
        monkeypatch.setattr(_lib, "_lib", proxy)
    try:
        inputs = Inputs()
        res = scenario(inputs)
        torch.cuda.synchronize()
        out = flatten(res)
        inputs.check()
    finally:
        if proxy is not None:
            monkeypatch.setattr(_lib, "_lib", real)
    if proxy is not None:
        proxy.verify()
    return out, proxy


def check(scenario, monkeypatch):
    plain, _ = run(scenario, monkeypatch)
    again, _ = run(scenario, monkeypatch)
    assert len(plain) > 0
    assert_same(plain, again, f"{scenario.__name__}: two runs without the proxy")
    claimed = {s for s, name in W.COVERED.items() if name == scenario.__name__}
    assert claimed
    for pattern in W.PATTERNS:
        got, proxy = run(scenario, monkeypatch, pattern)
        sizes = {}
        for name, need in proxy.calls:
            sizes.setdefault(name, set()).add(need)
        if pattern == W.PATTERNS[0]:
            print(scenario.__name__, "workspace bytes:", {k: sorted(v) for k, v in sorted(sizes.items())})
        assert claimed <= proxy.seen, (scenario.__name__, claimed - proxy.seen)
        for name in claimed:
            assert max(sizes[name]) > 0, f"{name}: no call of {scenario.__name__} had a workspace"
        assert_same(plain, got, f"{scenario.__name__} behind the proxy, workspaces filled with {pattern:#04x}")


# ---- encoder -----------------------------------------------------------------------------------------------------------

def scenario_encoder_split(inputs):
    """nsc_encode_clouds on the split path (scatter_split_kernel into the workspace's images, finish_kernel): the
    split_both batch of tests/encoder_families.py, two clouds of SPLIT_POINTS points, the only family with a workspace"""
    case, = [c for c in EF.cases() if c.entry == "split" and c.batch == "split_both" and c.interp == 1]
    pts, off = EF.clouds_of(case)
    assert EF.split_parts(len(off) - 1, len(pts)) > 1
    tp, to = inputs(pts), inputs(off)
    d, raw, itp = encoder(case).encode_points_batch((tp, to), return_images=True)
    return dict(descriptors=d, raw=raw, interpolated=itp)


# ---- inference GNN -------------------------------------------------------------------------------------------------------

def _graphs():
    from neural_spectral_codec_amd.keyframe import graph_manager as gm
    torch.manual_seed(1234)                                     # irregular_graph draws its features from torch's generator
    return [gm.synthetic_chain_graph(33, device="cuda", seed=33), gm.synthetic_chain_graph(257, device="cuda", seed=257),
            irregular_graph()]


def _abi_gat_forward(model, g):
    """nsc_gat_forward as the C ABI has it (SpectralGNN._run goes through nsc_gat_forward_ex), on the CSR the model
    builds for the graph -> (out, the CSR)"""
    gnn = model.gnn
    x = g.x.detach().to(torch.float32).contiguous()
    n = int(x.shape[0])
    csr = gnn._csr(g, True)                                     # a new model: nsc_graph_build_csr runs here
    L = _lib.lib()
    m, gs = gnn._model_struct(), csr.struct()
    out = torch.empty((n, gnn.output_dim), dtype=torch.float32, device=x.device)
    nbytes = L.nsc_gat_workspace_bytes(C.byref(m), n)
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.nsc_gat_forward(C.byref(m), C.byref(gs), _lib.ptr(x), _lib.ptr(csr.edge_attr), _lib.ptr(out), None,
                                     _lib.ptr(ws), nbytes, _lib.stream_ptr(x.device)), "nsc_gat_forward")
    return out, csr


def scenario_gat_forward(inputs):
    """nsc_graph_build_csr, then nsc_gat_forward, on the 33- and 257-node chain graphs (banded: one launch per layer) and
    on the irregular graph with self loops and a hub of tests/test_gat_gpu.py (GEMM and aggregate kernels)"""
    res = []
    for g in _graphs():
        for t in (g.x, g.edge_index, g.edge_attr):
            inputs(t)
        out, csr = _abi_gat_forward(_model(), g)
        with torch.no_grad():
            same = _model()(g)                                  # the wrapper's own path: nsc_gat_forward_ex, flags 0
        nnz = int(csr.row_ptr[-1])
        res.append(dict(out=out, wrapper=same, row_ptr=csr.row_ptr, src=csr.src[:nnz], eid=csr.eid[:nnz],
                        loop_attr=csr.loop_attr, band=csr.band))
        assert torch.equal(out, same)
    return res


def scenario_gat_forward_coresident(inputs):
    """nsc_gat_forward_ex with NSC_GAT_CORESIDENT (the LDS-free kernel set, generic layers) on the 33-node chain"""
    g = _graphs()[0]
    for t in (g.x, g.edge_index, g.edge_attr):
        inputs(t)
    m = _model()
    m.gnn.coresident = True
    with torch.no_grad():
        out = m(g)
    return dict(out=out)


# ---- training ------------------------------------------------------------------------------------------------------------

def scenario_training_step(inputs):
    """One training step on test_cache_coherence_gpu._train_setup's model and graph: nsc_graph_transpose,
    nsc_gat_forward_train, nsc_triplet_loss, nsc_gat_backward (which takes the forward's workspace: the state STATE names).
    At n = 96, and at n = 512, the first size whose weight gradients go through the split-K slabs of the workspace
    (``splits = N >= 512`` in nsc_gat_backward).  The triplets are n / 3 over distinct nodes, as
    test_captured_step_survives_csr_cache_turnover_on_distinct_nodes draws them: the triplet gradient is scattered with
    float atomics, and only without a repeated node are two runs equal by bytes.  Compared: the embeddings, the loss,
    every gradient and the running statistics the step updates."""
    from neural_spectral_codec_amd.gnn.trainer import TripletLoss
    res = {}
    for n in (96, 512):
        m, g, _ = _train_setup(n)
        for t in (g.x, g.edge_index, g.edge_attr):
            inputs(t)
        trip = np.random.default_rng(6).permutation(n)[:n // 3 * 3].reshape(-1, 3)
        m.train()
        emb = m(g)
        loss = TripletLoss(margin=0.1).forward_indexed(emb, trip[:, 0], trip[:, 1], trip[:, 2])
        loss.backward()
        grads = {k: p.grad for k, p in m.gnn.named_parameters()}
        assert all(v is not None for v in grads.values()) and float(loss.detach()) > 0.0
        res[n] = dict(emb=emb, loss=loss, grads=grads, buffers=dict(m.gnn.named_buffers()))
    return res


# ---- retrieval ------------------------------------------------------------------------------------------------------------

def scenario_mine_semi_hard(inputs):
    """nsc_mine_triplets_ws, strategy 2 (a row of candidate distances per anchor in the workspace), on
    test_retrieval_paths_gpu.mine_case(64)"""
    from neural_spectral_codec_amd.gnn.triplet_miner import TripletMiner
    desc, pos, _ = mine_case(64, 64)
    m = TripletMiner(positive_distance_max=MINE["pmax"], positive_temporal_min=MINE["ptmin"],
                     negative_distance_min=MINE["nmin"], negative_distance_max=MINE["nmax"],
                     negative_temporal_min=MINE["ntmin"], mining_strategy="semi-hard")
    np.random.seed(64)                                          # the miner draws its seed from numpy's generator
    trip, counts = m.mine_sequence(np.arange(64), inputs(desc), inputs(np.asarray(pos, np.float64)), 2)
    assert int(trip.shape[0]) > 0
    return dict(triplets=trip, counts=counts)


def scenario_topk(inputs):
    """nsc_topk_smallest for Q = 3, k = 10 at N = 10 (the smallest N the call takes for this k: one chunk, 240 bytes) and
    at N = 2049 (one row past the first chunk of 2048: two chunks), on test_retrieval_paths_gpu.tied_distances"""
    from neural_spectral_codec_amd.retrieval.wasserstein import _topk
    res = []
    for N in (10, 2049):
        idx, val = _topk(inputs(tied_distances(3, N, 10)), 10)
        res.append(dict(idx=idx, val=val))
    return res


def scenario_voxel_overlap(inputs):
    """nsc_voxel_overlap on five pairs of tests/keyframe_families.py (a few hundred rows in all; an empty cloud among
    them), one launch"""
    from neural_spectral_codec_amd.data import pose_utils as pu
    names = ("faces/v0.25", "collide40/split", "wrap/lookup", "empty/n1=0", "empty/dead_both")
    by = {p.name: p for p in KF.cloud_pairs(3)}
    pairs = [by[n] for n in names]
    p1 = [inputs(np.array(p.p1)) for p in pairs]
    p2 = [inputs(np.array(p.p2)) for p in pairs]
    iou, counts = pu.compute_overlap_batch(p1, p2, np.stack([p.T for p in pairs]), voxel_size=0.25,
                                           max_points=KF.VOX_MAX_POINTS, return_counts=True)
    return dict(iou=iou, counts=counts)


# ---- stage 2 -------------------------------------------------------------------------------------------------------------

def _small_pairs():
    """three pairs of gicp_clouds.many_small: a usual one, the one whose source is empty, the one whose source has one row"""
    src, tgt = GC.many_small(MANY_SMALL_SEED)
    mid = len(src) // 2
    ids = [1, mid, mid + 4]
    assert len(src[mid]) == 0 and len(src[mid + 4]) == 1 and len(src[1]) > 100
    return [src[i] for i in ids], [tgt[i] for i in ids]


def scenario_gicp_register(inputs):
    """nsc_gicp_register on three pairs of gicp_clouds.many_small, without stage outputs: the down-sampled points, the
    covariances and the counts stay in the workspace"""
    from neural_spectral_codec_amd.retrieval import geometric_verification as gv
    src, tgt = _small_pairs()
    sp, so = gv._pack(src, torch.device("cuda"))
    tp, to = gv._pack(tgt, torch.device("cuda"))
    init = torch.eye(4, dtype=torch.float64, device="cuda").repeat(3, 1, 1)
    return gv.register_packed(inputs(sp), inputs(so), inputs(tp), inputs(to), inputs(init))


def scenario_gicp_prepared_and_planar(inputs):
    """nsc_gicp_prepare of the same six clouds into one store, nsc_gicp_register_prepared on its pairs and
    nsc_planar_align on them with the default yaw table.  Compared: the three calls' outputs and what the store holds (row
    offsets, bounds, points, covariances; its index through the registration that reads it)"""
    from neural_spectral_codec_amd.retrieval import geometric_verification as gv
    from neural_spectral_codec_amd.retrieval import planar_alignment as pa
    src, tgt = _small_pairs()
    pts, off = gv._pack(src + tgt, torch.device("cuda"))
    store = gv.PreparedClouds()
    assert store.add_packed(inputs(pts), inputs(off)) == list(range(6))
    sid, tid = inputs(np.array([0, 1, 2], np.int64)), inputs(np.array([3, 4, 5], np.int64))
    reg = gv.register_prepared(store, sid, store, tid, stages=True)
    planar = pa.estimate_planar(store, sid, store, tid)      # no stage outputs: the peaks stay in the workspace
    b, n = store._buf, store.n_rows
    kept = dict(row_offsets=b["row_offsets"][:7], slot_offsets=b["slot_offsets"][:7], bounds=b["bounds"][:6],
                points=b["points"][:n], covariances=b["covariances"][:n])
    return dict(registered=reg, planar=planar, store=kept)


# ---- pose graph ------------------------------------------------------------------------------------------------------------

def scenario_posegraph_plain(inputs):
    """nsc_posegraph_linearize and nsc_posegraph_optimize as the C ABI has them (tests/_posegraph.py: the Python layer calls
    the robust forms), on the 64-ring with drift and one closure.  The helpers upload their own copies, so no input is
    held here."""
    _, init, e, Z, Om = P.drift_ring()
    return dict(linearize=plain_linearize(init, e, Z, Om), optimize=plain_optimize(init, e, Z, Om))


def _graph_on_device(inputs, X, e, Z, Om, *more):
    return [inputs(np.ascontiguousarray(a)) for a in (np.asarray(X, np.float64), np.asarray(e, np.int64),
                                                      np.asarray(Z, np.float64), np.asarray(Om, np.float64)) + more]


def scenario_posegraph_robust(inputs):
    """PoseGraphOptimizer.linearize and optimize_device (nsc_posegraph_linearize_robust, nsc_posegraph_optimize_robust):
    without a kernel on the 64-ring with drift and one closure, and with Cauchy on the outlier ring, width 3 on its
    closures (chi2 and weights: one launch more)"""
    res = {}
    X, e, Z, Om = _graph_on_device(inputs, *P.drift_ring()[1:])
    opt = optimizer()
    res["quadratic"] = dict(linearize=opt.linearize(X, e, Z, Om), optimize=opt.optimize_device(X, e, Z, Om, step0=True))
    _, init, e, Z, Om, closures = R.outlier_ring(0)
    X, e, Z, Om, scale = _graph_on_device(inputs, init, e, Z, Om, R.closure_scale(len(e), closures, 3.0))
    opt = optimizer(kernel="cauchy")
    res["cauchy"] = dict(linearize=opt.linearize(X, e, Z, Om, robust_scale=scale),
                         optimize=opt.optimize_device(X, e, Z, Om, step0=True, robust_scale=scale))
    return res


def scenario_posegraph_coarse(inputs):
    """nsc_posegraph_optimize_coarse with coarse_block = 8 at N = 65: nine aggregates, the last of one pose"""
    X, e, Z, Om = _graph_on_device(inputs, *P.drift_ring(65)[1:])
    out = optimizer(coarse_block=8).optimize_device(X, e, Z, Om, step0=True)
    assert out["coarse_stats"].tolist() == [9.0, 0.0]
    return out


def scenario_posegraph_covariance(inputs):
    """nsc_posegraph_covariance of 11 poses of the 65-ring (66 columns: a chunk of 64 and a second nearly empty, whose
    other columns never run), with block-Jacobi alone and with the coarse space of coarse_block = 8"""
    X, e, Z, Om = _graph_on_device(inputs, *P.drift_ring(65)[1:])
    nodes = inputs(np.array([1 + (7 * k) % 64 for k in range(11)], np.int64))
    res = {}
    for name, L in (("block-Jacobi", None), ("coarse", 8)):
        opt = optimizer(coarse_block=L, max_pcg_iterations=CAP, pcg_tolerance=V.TAU)
        res[name] = opt.covariance_device(X, e, Z, Om, nodes)
        assert int(res[name]["stats"][3]) == 0                  # every column converged
    return res


# ---- map -----------------------------------------------------------------------------------------------------------------

def scenario_global_map(inputs):
    """GlobalMap.build (nsc_map_build) on map_insert_cases.twelve_voxels, with room for every voxel (max_voxels = 16) and
    with eight places for twelve voxels"""
    from neural_spectral_codec_amd.retrieval import GlobalMap
    A, B, _ = IK.twelve_voxels()
    p, o, T = (inputs(a) for a in joined([A, B]))
    res = {}
    for M in (16, 8):
        res[M] = GlobalMap(voxel_size=1.0, max_voxels=M).build((p, o), T)
        assert (res[M]["voxels_found"], res[M]["voxels_written"]) == (12, min(M, 12))
    return res


def kept_map(m):
    """The kept map where it is defined, as tests/test_map_insert_gpu.py's assert_same_bits compares two maps: the stats
    and the cursor, the rows [0, stats[1]) of voxels, info, keys and moments, and the index as the mapping key -> place
    (which of two keys that meet in a slot claims it is free, so a key may sit in different slots)"""
    torch.cuda.synchronize()
    n = int(m.stats[1])
    res = {k: getattr(m, k)[:n] for k in KEPT}
    places, occupied = index_of(dict(index=m.index.cpu().numpy()))
    res.update(stats=m.stats, cursor=m.cursor, index=sorted(places.items()), occupied=occupied)
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}


def scenario_kept_map(inputs):
    """MapLocalizer.build_device, insert_device, remove_device and replace_device (nsc_map_build_dist, _insert_dist,
    _remove_dist, _replace_dist) on map_insert_cases.twelve_voxels: A built, B inserted, removed, inserted again and then
    moved by one voxel along x; at max_voxels = 16, and at 8 where four voxels are past the outputs.  Compared after every
    call: the kept map's seven tensors by kept_map(), which names the one comparison that is not of raw bytes, and the
    counts ``removed`` and ``placed``"""
    A, B, _ = IK.twelve_voxels()
    pa, oa, Ta = (inputs(a) for a in A)
    pb, ob, Tb = (inputs(a) for a in B)
    moved = B[2].copy()
    moved[:, 0, 3] += 1.0
    Tn = inputs(moved)
    res = {}
    for M in (16, 8):
        m = localizer(insertable=True, max_voxels=M)
        steps = []
        m.build_device(pa, oa, Ta)
        steps.append(("build", kept_map(m)))
        m.insert_device(pb, ob, Tb)
        steps.append(("insert", kept_map(m)))
        assert m.stats[:2].tolist() == [12, min(M, 12)]
        out = m.remove_device(pb, ob, Tb)
        steps.append(("remove", kept_map(m), out["removed"]))
        m.insert_device(pb, ob, Tb)
        steps.append(("insert again", kept_map(m)))
        out = m.replace_device(pb, ob, Tb, Tn, first_row=len(A[0]), first_cloud=1)
        steps.append(("replace", kept_map(m), out["removed"], out["placed"]))
        res[M] = steps
    return res


def _scans(inputs, n_scans=4):
    """scans for a map of map_localize_cases.ten_voxels: its two clouds, all of its rows, lookup_scan's rows (absent,
    unusable and overflowing voxels, rows outside the grid and not finite), then an empty scan and the first three
    again; a few centimetres and milliradians off"""
    pts, off, poses, vox = K.ten_voxels()
    h = int(off[1])
    clouds = [pts[:h], pts[h:], pts, K.lookup_scan(vox)[0], pts[:0], pts[:h], pts[h:], pts][:n_scans]
    init = np.stack([K.general_pose(0.004 * (i + 1), 0.001 * i, [0.03 - 0.01 * i, -0.02, 0.01 * i], roll=-0.002)
                     for i in range(n_scans)])
    sp, so = IK.pack(clouds)
    return (pts, off, poses), (inputs(sp), inputs(so)), init


def _register(inputs, **kw):
    (pts, off, poses), (sp, so), init = _scans(inputs)
    m = localizer(**kw)
    m.build_device(inputs(pts), inputs(off), inputs(poses))
    out = m.register_device(sp, so, inputs(init), system0=True)
    assert int(out["n_correspondences"].max()) > 0 and int(out["iterations"].max()) > 0
    return out


def scenario_map_register(inputs):
    """MapLocalizer.register_device with the defaults (nsc_map_register) on four scans of map_localize_cases.ten_voxels"""
    return _register(inputs)


def scenario_map_register_robust(inputs):
    """the same with kernel="cauchy", robust_scale=3.0, neighbours=7 (nsc_map_register_robust: the wide slabs)"""
    return _register(inputs, kernel="cauchy", robust_scale=3.0, neighbours=7)


SCENARIOS = [v for k, v in sorted(globals().items()) if k.startswith("scenario_") and callable(v)]


def test_covered_names_the_scenarios_of_this_file():
    assert {s.__name__ for s in SCENARIOS} == set(W.COVERED.values())
    assert set(W.COVERED) == set(W.wrapped_symbols())


@pytest.mark.parametrize("scenario", SCENARIOS, ids=[s.__name__ for s in SCENARIOS])
def test_workspace_contract(scenario, monkeypatch):
    check(scenario, monkeypatch)


# ---- MapLocalizer.register_device above MAP_REGISTER_MAX_SCANS ----------------------------------------------------------------

@pytest.mark.parametrize("system0", [False, True])
@pytest.mark.parametrize("kw", [{}, dict(kernel="cauchy", robust_scale=3.0, neighbours=7)], ids=["plain", "robust"])
def test_register_in_several_calls_equals_one_call(kw, system0, monkeypatch):
    """register_device hands batches above _lib.MAP_REGISTER_MAX_SCANS (65535) to the library in several calls, with views
    off[a:], init[a:], T[a:], ... into its buffers while points and N stay whole.  With the limit lowered to 3, eight scans
    of ten_voxels -- an empty one and one with a NaN pose among them -- go in calls of 3, 3 and 2: every output equals the
    one call's by bytes."""
    (pts, off, poses), (sp, so), init = _scans(Inputs(), 8)
    init[5, 1, 2] = np.nan
    assert int(so[5] - so[4]) == 0
    init = dev(init)
    m = localizer(**kw)
    m.build_device(dev(pts), dev(off), dev(poses))
    whole = flatten(m.register_device(sp, so, init, system0=system0))
    torch.cuda.synchronize()
    real = _lib.lib()
    proxy = W.WorkspaceProxy(real, 0xFF)
    monkeypatch.setattr(_lib, "MAP_REGISTER_MAX_SCANS", 3)
    monkeypatch.setattr(_lib, "_lib", proxy)
    try:
        out = m.register_device(sp, so, init, system0=system0)
        parts = flatten(out)
    finally:
        monkeypatch.setattr(_lib, "_lib", real)
    proxy.verify()
    entry = "nsc_map_register_robust" if kw else "nsc_map_register"
    assert [name for name, _ in proxy.calls] == [entry] * 3
    assert ("system0" in out) == system0 and torch.isnan(out["transform"][5]).all()
    assert int(out["n_correspondences"][5]) == -1 and int(out["n_correspondences"][4]) == 0
    assert_same(whole, parts, "calls of 3, 3 and 2 scans against one call of 8")
