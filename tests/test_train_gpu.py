"""Training step on the GPU (BASELINE configs[4]) against torch autograd through the CPU restatement.
Dropout is off for parity (the reference never seeds its RNG); a separate test covers dropout > 0."""
import numpy as np
import pytest
import torch

import gat_oracle as go
import train_families
from neural_spectral_codec_amd.gnn.model import create_spectral_gnn
from neural_spectral_codec_amd.gnn.trainer import TripletLoss, GNNTrainer
from neural_spectral_codec_amd.keyframe import graph_manager as gm

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _bar_ratio(out, ref64, rtol=1e-4, atol=1e-6):
    """Worst element of |out - ref| / (rtol |ref| + atol): <= 1 means inside the element-wise north_star bar."""
    out, ref64 = out.detach().cpu().double(), ref64.detach().cpu().double()
    return ((out - ref64).abs() / (rtol * ref64.abs() + atol)).max().item()


def _assert_train_forward(emb_gpu, emb32, emb64, what):
    """Train-mode forward against the float64 evaluation of the restatement.  Batch-statistics BatchNorm divides by a
    standard deviation estimated from the rows, which amplifies float32 rounding; the float32 restatement (the
    reference's own arithmetic) itself leaves the element-wise 1e-4 |ref| + 1e-6 bar on small batches.  So the kernels
    are held to the float32 restatement's own accuracy, both figures printed:
      * RMS error no worse than 1.5 x the float32 restatement's (a stable statistic; 1.5 covers the different summation
        order of two float32 evaluations of the same formulas),
      * worst element / bar no worse than max(1, 3 x the float32 restatement's) -- the maximum over ~1e5 heavy-tailed
        ratios (elements near zero have a 1e-6 bound) scatters by about 2 x between two equally accurate evaluations."""
    g, a, r = emb_gpu.detach().cpu().double(), emb32.detach().cpu().double(), emb64.detach().cpu().double()
    rms_gpu, rms_f32 = (g - r).pow(2).mean().sqrt().item(), (a - r).pow(2).mean().sqrt().item()
    w_gpu, w_f32 = _bar_ratio(g, r), _bar_ratio(a, r)
    print(f"{what}: RMS error kernels {rms_gpu:.3e} / float32 restatement {rms_f32:.3e}; worst element / bar "
          f"kernels {w_gpu:.2f} / float32 restatement {w_f32:.2f}")
    # floor: 2e-6 RMS on O(1) outputs is ~17 float32 ulp after five GEMMs deep (K up to 800, MFMA accumulates along k in
    # sequence, torch's CPU GEMM in blocks) -- below it the two float32 evaluations are not distinguishable in quality
    # (hidden_dim 64 variant, round 3: kernels 1.06e-6, restatement 5.2e-7; hidden_dim 256: 9.0e-7 vs 1.0e-6)
    assert rms_gpu <= max(1.5 * rms_f32, 2e-6), f"{what}: RMS error {rms_gpu:.3e} vs {rms_f32:.3e} of the float32 restatement"
    assert w_gpu <= max(1.0, 3.0 * w_f32), f"{what}: worst element {w_gpu:.2f} x the bar, float32 restatement {w_f32:.2f} x"


def _setup(n, edge_dim=2, dropout=0.0, seed=0):
    torch.manual_seed(seed)
    m = create_spectral_gnn(edge_dim=edge_dim, dropout=dropout)
    go.randomize_bn_stats(m, seed + 1)
    with torch.no_grad():
        for c in m.gnn.convs:
            c.bias.normal_(0, 0.1)
    m = m.to("cuda")
    g = gm.synthetic_chain_graph(n, device="cuda", seed=seed + 2)
    rng = np.random.default_rng(seed)
    trip = np.stack([rng.integers(0, n, 256), rng.integers(0, n, 256), rng.integers(0, n, 256)], 1)
    return m, g, trip


def _key_map(gnn):
    keys = ["input_proj.weight", "input_proj.bias", "input_norm.weight", "input_norm.bias",
            "output_proj.weight", "output_proj.bias"]
    for l, conv in enumerate(gnn.convs):
        keys += [f"convs.{l}.lin_src.weight", f"convs.{l}.att_src", f"convs.{l}.att_dst"]
        if conv.lin_edge is not None:
            keys += [f"convs.{l}.lin_edge.weight", f"convs.{l}.att_edge"]
        keys += [f"convs.{l}.bias", f"batch_norms.{l}.weight", f"batch_norms.{l}.bias"]
    return keys


@pytest.mark.parametrize("n,edge_dim", [(40, 2), (300, 2), (300, None), (1500, 2), (1500, None)])
def test_forward_train_and_gradients(n, edge_dim):
    m, g, trip = _setup(n, edge_dim)
    ref_model_state = {k: v.clone() for k, v in m.state_dict().items()}
    crit = TripletLoss(margin=0.1)
    tt = torch.from_numpy(trip)

    # triplet loss + a random linear probe (the triplet gradient alone sums to zero over the rows,
    # which would leave output_proj.bias untested)
    R = torch.randn(n, 800, generator=torch.Generator().manual_seed(9)) * 1e-3
    emb_ref, grads_ref, gx_ref, loss_ref = go.reference_gradients(
        m, g, lambda e: go.triplet_loss_reference(e, tt[:, 0], tt[:, 1], tt[:, 2], 0.1) + (e * R).sum())

    m.train()
    g.x.requires_grad_(True)
    emb = m(g)
    loss = crit.forward_indexed(emb, trip[:, 0], trip[:, 1], trip[:, 2]) + (emb * R.cuda()).sum()
    loss.backward()
    # north_star bar, element-wise (|gpu - ref| <= 1e-4 |ref| + 1e-6), against the float64 evaluation of the restatement
    taps64 = {}
    emb64 = go.reference_gradients(m, g, lambda e: (e * 0).sum(), dtype=torch.float64, taps=taps64)[0]
    _assert_train_forward(emb, emb_ref, emb64, f"train-mode forward, {n} nodes")
    assert abs(loss.item() - loss_ref.item()) <= 1e-4 * abs(loss_ref.item()) + 1e-6
    params = dict(m.gnn.named_parameters())
    gscale = max(v.abs().max().item() for v in grads_ref.values())
    for k in _key_map(m.gnn):
        got = params[k].grad.detach().cpu().reshape(grads_ref[k].shape)
        if k == "input_proj.bias" or k.endswith(".bias") and k.startswith("convs."):
            # a bias in front of a batch-statistics BatchNorm has an exactly-zero gradient: both sides
            # hold only float32 rounding noise
            assert got.abs().max().item() < 1e-3 * gscale and grads_ref[k].abs().max().item() < 1e-3 * gscale, k
            continue
        assert _rel(got, grads_ref[k]) < 2e-3, k            # float32 sums over n nodes, different order
    assert _rel(g.x.grad.cpu(), gx_ref) < 2e-3
    # BatchNorm running statistics moved like nn.BatchNorm1d (momentum 0.1, unbiased variance)
    with torch.no_grad():
        x = g.x.detach().cpu()
        z = x @ ref_model_state["gnn.input_proj.weight"].cpu().t() + ref_model_state["gnn.input_proj.bias"].cpu()
        rm = 0.9 * ref_model_state["gnn.input_norm.running_mean"].cpu() + 0.1 * z.mean(0)
        rv = 0.9 * ref_model_state["gnn.input_norm.running_var"].cpu() + 0.1 * z.var(0, unbiased=True)
    assert torch.allclose(m.gnn.input_norm.running_mean.cpu(), rm, rtol=1e-4, atol=1e-5)
    assert torch.allclose(m.gnn.input_norm.running_var.cpu(), rv, rtol=1e-4, atol=1e-5)
    assert int(m.gnn.input_norm.num_batches_tracked) == 1
    # ... and so did every layer's BatchNorm (batch statistics from the float64 restatement's taps)
    train_families.check_bn_running_stats(m, ref_model_state, taps64, n)


def test_gradients_on_hub_graph():
    """The attention kernels of the training step take a fast path for in-degree <= 64 (one entry per lane, float4 gathers)
    and a general loop above it; the per-source pass walks lists of any length in chunks of 64.  A graph with a hub that
    150 nodes point to and that points to 150 others (plus a chain, duplicate edges and explicit self loops) runs both;
    embedding, loss, every gradient and the input gradient against autograd through the restatement."""
    from types import SimpleNamespace
    n = 400
    torch.manual_seed(3)
    m = create_spectral_gnn(edge_dim=2, dropout=0.0)
    go.randomize_bn_stats(m, 4)
    m = m.to("cuda")
    rng = np.random.default_rng(5)
    i = np.arange(n - 1)
    hub = 7
    src = np.concatenate([i, i + 1, np.arange(20, 170), np.full(150, hub), rng.integers(0, n, 60), np.arange(0, n, 9)])
    dst = np.concatenate([i + 1, i, np.full(150, hub), np.arange(200, 350), rng.integers(0, n, 60), np.arange(0, n, 9)])
    src = np.concatenate([src, src[:40]]); dst = np.concatenate([dst, dst[:40]])         # duplicate edges
    ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64))
    x = torch.rand((n, 800)) ** 4
    x = x / x.sum(1, keepdim=True)
    ea = torch.rand((ei.shape[1], 2))
    g = SimpleNamespace(x=x.cuda(), edge_index=ei.cuda(), edge_attr=ea.cuda(), num_nodes=n)
    trip = np.stack([rng.integers(0, n, 256), rng.integers(0, n, 256), rng.integers(0, n, 256)], 1)
    tt = torch.from_numpy(trip)
    R = torch.randn(n, 800, generator=torch.Generator().manual_seed(9)) * 1e-3
    emb_ref, grads_ref, gx_ref, loss_ref = go.reference_gradients(
        m, g, lambda e: go.triplet_loss_reference(e, tt[:, 0], tt[:, 1], tt[:, 2], 0.1) + (e * R).sum())
    m.train()
    g.x.requires_grad_(True)
    emb = m(g)
    loss = TripletLoss(margin=0.1).forward_indexed(emb, trip[:, 0], trip[:, 1], trip[:, 2]) + (emb * R.cuda()).sum()
    loss.backward()
    emb64 = go.reference_gradients(m, g, lambda e: (e * 0).sum(), dtype=torch.float64)[0]
    _assert_train_forward(emb, emb_ref, emb64, "train-mode forward, hub graph")
    assert abs(loss.item() - loss_ref.item()) <= 1e-4 * abs(loss_ref.item()) + 1e-6
    params = dict(m.gnn.named_parameters())
    gscale = max(v.abs().max().item() for v in grads_ref.values())
    for k in _key_map(m.gnn):
        got = params[k].grad.detach().cpu().reshape(grads_ref[k].shape)
        if k == "input_proj.bias" or k.endswith(".bias") and k.startswith("convs."):
            assert got.abs().max().item() < 1e-3 * gscale and grads_ref[k].abs().max().item() < 1e-3 * gscale, k
            continue
        assert _rel(got, grads_ref[k]) < 2e-3, k
    assert _rel(g.x.grad.cpu(), gx_ref) < 2e-3


@pytest.mark.parametrize("in_dim,out_dim,residual", [(800, 800, False), (64, 32, False), (32, 64, False),
                                                     (64, 48, True), (48, 80, True)])
def test_residual_variants_train(in_dim, out_dim, residual):
    """SpectralGNN(residual=False) and residual_proj (input_dim != output_dim, model.py:91-94,147-149) through
    forward_train / backward with x.requires_grad: the input gradient carries dOut only through an identity
    residual, dOut W_res through residual_proj, and nothing when residual is off."""
    from neural_spectral_codec_amd.gnn.model import SpectralGNN
    n = 150
    torch.manual_seed(4)
    m = SpectralGNN(input_dim=in_dim, hidden_dim=64, output_dim=out_dim, n_layers=3, dropout=0.0,
                    residual=residual, edge_dim=2)
    go.randomize_bn_stats(m, 5)
    assert (m.residual_proj is not None) == (residual and in_dim != out_dim)
    m = m.to("cuda")
    g = gm.synthetic_chain_graph(n, device="cuda", seed=8, features=torch.rand(n, in_dim))
    R = torch.randn(n, out_dim, generator=torch.Generator().manual_seed(2))
    emb_ref, grads_ref, gx_ref, _ = go.reference_gradients(m, g, lambda e: (e * R).sum() + (e * e).sum())
    m.train()
    g.x.requires_grad_(True)
    emb = m(g)
    ((emb * R.cuda()).sum() + (emb * emb).sum()).backward()
    emb64 = go.reference_gradients(m, g, lambda e: (e * 0).sum(), dtype=torch.float64)[0]
    _assert_train_forward(emb, emb_ref, emb64, f"train-mode forward, residual variant {in_dim}->{out_dim}")
    assert _rel(g.x.grad.cpu(), gx_ref) < 2e-3
    params = dict(m.named_parameters())
    keys = _key_map(m) + (["residual_proj.weight", "residual_proj.bias"] if m.residual_proj is not None else [])
    gscale = max(v.abs().max().item() for v in grads_ref.values())
    for k in keys:
        got = params[k].grad.detach().cpu().reshape(grads_ref[k].shape)
        if k == "input_proj.bias" or k.endswith(".bias") and k.startswith("convs."):
            assert got.abs().max().item() < 1e-3 * gscale, k
            continue
        assert _rel(got, grads_ref[k]) < 2e-3, k
    # eval forward of the same shapes
    m.eval()
    with torch.no_grad():
        go.assert_within_bar(m(g), go.forward_reference(m, g, dtype=torch.float64))


def test_triplet_indices_follow_tensor_indexing():
    """embeddings[idx] semantics (trainer.py:207-209): negative indices wrap; out of range raises on the host and,
    for device-resident indices (no sync on that path), poisons the loss with NaN and writes nothing."""
    torch.manual_seed(1)
    n = 60
    emb = torch.randn(n, 800, device="cuda", requires_grad=True)
    crit = TripletLoss(0.1)
    ia, ip, in_ = np.array([0, 5, 59, 7]), np.array([3, 9, 1, 8]), np.array([10, 20, 30, 40])
    want = crit.forward_indexed(emb, ia, ip, in_)
    got = crit.forward_indexed(emb, ia - n, ip, in_ - n)               # wrapped negatives
    assert torch.equal(want, got)
    with pytest.raises(IndexError):
        crit.forward_indexed(emb, np.array([0, n]), np.array([1, 2]), np.array([3, 4]))
    with pytest.raises(IndexError):
        crit.forward_indexed(emb, np.array([0, 1]), np.array([1, -n - 1]), np.array([3, 4]))
    bad = torch.tensor([0, n + 7], device="cuda")
    ok = torch.tensor([1, 2], device="cuda")
    loss = crit.forward_indexed(emb, bad, ok, ok + 5)
    loss.backward()
    assert torch.isnan(loss)
    g = emb.grad.cpu()
    touched = torch.zeros(n, dtype=torch.bool)
    touched[[0, 1, 6]] = True                                            # the valid triplet (0, 1, 6)
    assert torch.isfinite(g).all() and bool((g[~touched] == 0).all())    # the bad triplet wrote nothing


def test_triplet_loss_matches_torch():
    torch.manual_seed(0)
    emb = torch.randn(500, 800, device="cuda", requires_grad=True)
    rng = np.random.default_rng(1)
    ia, ip, in_ = (rng.integers(0, 500, 1024) for _ in range(3))
    crit = TripletLoss(0.1)
    loss = crit.forward_indexed(emb, ia, ip, in_, scale=0.25)
    loss.backward()
    e2 = emb.detach().cpu().clone().requires_grad_(True)
    ref = go.triplet_loss_reference(e2, torch.from_numpy(ia), torch.from_numpy(ip), torch.from_numpy(in_), 0.1) * 0.25
    ref.backward()
    assert abs(loss.item() - ref.item()) < 1e-4 * abs(ref.item())
    assert _rel(emb.grad.cpu(), e2.grad) < 1e-4
    # reference call signature: three gathered tensors
    l2 = crit(emb[ia], emb[ip], emb[in_])
    assert abs(l2.item() - ref.item() * 4) < 1e-3 * abs(ref.item() * 4)


def test_train_steps_reduce_loss_and_match_cpu_adam():
    m, g, trip = _setup(400, 2)
    import copy
    cpu_model = copy.deepcopy(m).cpu()
    tr = GNNTrainer(m, device="cuda", learning_rate=5e-4, weight_decay=1e-5, margin=0.1,
                    batch_size=256, accumulation_steps=1)
    losses = [tr.train_batches(g, trip) for _ in range(8)]
    assert losses[-1] < losses[0]
    # one step on the CPU with torch autograd through the restatement gives the same update
    m2, g2, trip2 = _setup(400, 2)
    tr2 = GNNTrainer(m2, device="cuda", batch_size=256, accumulation_steps=1)
    tr2.train_batches(g2, trip2)
    tt = torch.from_numpy(trip2)
    _, grads_ref, _, _ = go.reference_gradients(
        cpu_model, g2, lambda e: go.triplet_loss_reference(e, tt[:, 0], tt[:, 1], tt[:, 2], 0.1))
    params = dict(cpu_model.gnn.named_parameters())
    opt = torch.optim.Adam(cpu_model.parameters(), lr=5e-4, weight_decay=1e-5)
    for k, gr in grads_ref.items():
        params[k].grad = gr.reshape(params[k].shape)
    opt.step()
    got = dict(m2.gnn.named_parameters())
    for k in ("output_proj.weight", "convs.1.lin_src.weight", "input_proj.weight"):
        assert torch.allclose(got[k].detach().cpu(), params[k].detach(), rtol=1e-3, atol=2e-5), k


def _scene_clouds(place, n_pts=3000):
    """Synthetic 16-ring scans whose SCENE (range profile: base, tilt, six azimuthal harmonics with place-seeded
    amplitudes / frequencies / phases) depends on the place id, plus 5 cm of per-visit noise: revisits of a place
    look alike, different places differ (the descriptor is rotation-invariant, so phases alone would not do)."""
    rings, steps = 16, n_pts // 16
    az = np.tile(np.linspace(-np.pi, np.pi, steps, endpoint=False), rings)
    ring = np.repeat(np.arange(rings), steps)
    el = np.deg2rad(-24.0 + 25.0 * (ring + 0.5) / rings)
    ce, se = np.cos(el), np.sin(el)
    out = []
    for i, p in enumerate(place):
        r = np.random.default_rng(int(p))
        f, a, ph = r.integers(1, 40, 6), r.uniform(0.5, 8.0, 6), r.uniform(0, 2 * np.pi, 6)
        rng = r.uniform(12, 40) + r.uniform(0, 25) * ring / rings
        for k in range(6):
            rng = rng + a[k] * np.sin(f[k] * az + ph[k] + 0.3 * ring * (k % 2))
        v = np.random.default_rng(1000003 + i)
        rng = np.clip(rng + v.normal(0, 0.05, rng.shape), 1.5, 79.0)
        out.append(np.stack([rng * ce * np.cos(az), rng * ce * np.sin(az), rng * se, v.uniform(0, 1, rng.shape)],
                            1).astype(np.float32))
    off = np.zeros(len(out) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in out])
    return np.concatenate(out), off


def _config5_dataset(dev):
    """BASELINE configs[4] shape: 15 synthetic sequences -- 9 "KITTI-like" + 6 "NCLT-like" -- 4 541 keyframes in
    all, every sequence a closed course driven 2-3 times so that revisits (positives) exist; descriptors come from the
    encoder on the place-dependent synthetic scans above."""
    from neural_spectral_codec_amd.encoding import SpectralEncoder
    rng = np.random.default_rng(7)
    kitti = [454, 110, 466, 80, 27, 276, 110, 110, 407]          # keyframes per sequence, sums to 2 040
    nclt = [420, 415, 418, 412, 421, 415]                        # 2 501
    lens = kitti + nclt
    assert sum(lens) == 4541 and len(lens) == 15
    poses, seq_ids, place = [], [], []
    for s, ln in enumerate(lens):
        laps = 2 if s < 9 else 3
        per_lap = ln / laps
        radius = per_lap * 1.2 / (2 * np.pi)                     # ~1.2 m between keyframes
        t = np.arange(ln) / per_lap * 2 * np.pi
        p = np.tile(np.eye(4), (ln, 1, 1))
        p[:, 0, 3] = radius * np.cos(t) + rng.normal(0, 0.3, ln) + 1000.0 * s
        p[:, 1, 3] = radius * np.sin(t) + rng.normal(0, 0.3, ln)
        c, sn = np.cos(t + np.pi / 2), np.sin(t + np.pi / 2)
        p[:, 0, 0], p[:, 0, 1], p[:, 1, 0], p[:, 1, 1] = c, -sn, sn, c
        poses.append(p)
        seq_ids += [s] * ln
        place += list(100000 * s + np.floor((np.arange(ln) % per_lap) / 3).astype(int))    # 3 keyframes share a scene
    poses = np.concatenate(poses)
    enc = SpectralEncoder(n_elevation=16).to(dev)
    pts, off = _scene_clouds(place)
    desc = enc.encode_points_batch((torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)))
    return desc, poses, np.asarray(seq_ids)


def test_config5_full_size_train_step():
    """BASELINE configs[4] at its stated size on one GPU: a 4 541-keyframe chain graph over 15 synthetic KITTI+NCLT
    sequences, triplets from the device miner, ONE 1 024-triplet batch through forward + TripletLoss + backward
    (hidden_dim=256, margin=0.1, dropout 0 for parity): loss, every parameter gradient, the input gradient and one
    Adam step against torch autograd through the restatement (reference src/gnn/trainer.py:186-221).

    Tolerances are evidence, not a dial: train-mode BatchNorm divides by the batch standard deviation, which on real
    descriptors (nearly equal rows) amplifies float32 rounding far beyond the 1e-4 eval bar -- so the restatement is
    evaluated in float32 (the reference's arithmetic) AND float64, and for every quantity the test prints and checks
    TWO numbers against the float64 result: the kernels' distance and the float32 restatement's own.  The kernels must
    be no worse than 1.5 x the float32 restatement (both are float32 evaluations of the same formulas; 1.5 covers the
    different summation order: wave-tree column sums and MFMA k-order here, sequential / pairwise sums in torch), with
    a floor of 1e-4 (embeddings) / 2e-3 (gradients: sums over 4 541 nodes) below which neither is resolved."""
    import copy
    from neural_spectral_codec_amd.gnn.triplet_miner import create_triplet_miner
    from neural_spectral_codec_amd.keyframe.graph_manager import build_chain_graph
    dev = torch.device("cuda")
    desc, poses, seq_ids = _config5_dataset(dev)
    n = 4541
    assert desc.shape == (n, 800)
    graph = build_chain_graph(desc, 5, "cuda", poses)            # one chain across all sequences
    assert graph.edge_index.shape == (2, 18158) and graph.edge_attr.shape == (18158, 2)
    np.random.seed(3)
    trip_all = np.asarray(create_triplet_miner().mine_triplets(desc.cpu().numpy(), poses, 1, sequence_ids=seq_ids))
    assert len(trip_all) >= 1024, f"only {len(trip_all)} triplets mined"
    assert (seq_ids[trip_all[:, 0]] == seq_ids[trip_all[:, 1]]).all() and (seq_ids[trip_all[:, 0]] == seq_ids[trip_all[:, 2]]).all()
    np.random.shuffle(trip_all)                                   # trainer.py:183
    trip = trip_all[:1024]
    tt = torch.from_numpy(trip)

    torch.manual_seed(0)
    m = create_spectral_gnn(input_dim=800, hidden_dim=256, output_dim=800, n_layers=3, dropout=0.0, edge_dim=2)
    go.randomize_bn_stats(m, 1)
    with torch.no_grad():
        for c in m.gnn.convs:
            c.bias.normal_(0, 0.1)
    cpu_model = copy.deepcopy(m)
    m = m.to(dev)

    def loss_fn(e):                                               # trainer.py:207-212 (accumulation_steps = 4)
        return go.triplet_loss_reference(e, tt[:, 0], tt[:, 1], tt[:, 2], 0.1) / 4
    emb32, g32, gx32, loss32 = go.reference_gradients(cpu_model, graph, loss_fn)
    emb64, g64, gx64, loss64 = go.reference_gradients(cpu_model, graph, loss_fn, dtype=torch.float64)

    def dist(a, b):                                               # max-norm distance relative to the exact result
        return ((a.double() - b).abs().max() / (b.abs().max() + 1e-300)).item()

    tr = GNNTrainer(m, device="cuda", learning_rate=5e-4, weight_decay=1e-5, margin=0.1, batch_size=1024,
                    accumulation_steps=4)                          # train_multi_dataset.yaml:127-129, trainer.py:187-188
    m.train()
    tr.optimizer.zero_grad()
    graph.x.requires_grad_(True)
    emb = m(graph)                                                # trainer.py:205
    loss = tr.criterion.forward_indexed(emb, trip[:, 0], trip[:, 1], trip[:, 2], scale=1.0 / 4)   # :207-212
    loss.backward()                                               # :213
    assert loss64.item() > 0
    assert abs(loss.item() - loss64.item()) <= 1e-4 * abs(loss64.item()) + 1e-7
    FACTOR = 1.5
    report = []

    def check(name, got, ref32, ref64, floor):
        d_gpu, d_f32 = dist(got, ref64), dist(ref32, ref64)
        report.append((name, d_gpu, d_f32))
        assert d_gpu <= max(floor, FACTOR * d_f32), (
            f"{name}: kernels {d_gpu:.3e} from the float64 restatement, the float32 restatement {d_f32:.3e} "
            f"(allowed {FACTOR} x, floor {floor:g})")

    check("embedding (train-mode forward)", emb.detach().cpu(), emb32, emb64, 1e-4)
    params = dict(m.gnn.named_parameters())
    gscale = max(v.abs().max().item() for v in g64.values())
    # Exactly-zero gradients (float32 noise on both sides): a bias in front of a batch-statistics BatchNorm; and,
    # because the triplet gradient sums to zero over the rows, output_proj.bias and the last BatchNorm's bias.
    zero = {"input_proj.bias", "output_proj.bias", "batch_norms.2.bias"} | {f"convs.{l}.bias" for l in range(3)}
    for k in _key_map(m.gnn):
        got = params[k].grad.detach().cpu().reshape(g64[k].shape)
        if k in zero:
            assert got.abs().max().item() < 1e-3 * gscale and g64[k].abs().max().item() < 1e-6 * gscale, k
            continue
        check("grad " + k, got, g32[k], g64[k], 2e-3)
    check("grad x", graph.x.grad.cpu(), gx32, gx64, 2e-3)
    print("\nconfigs[4] full size -- max-norm distance from the float64 restatement: kernels | float32 restatement | ratio")
    for name, d_gpu, d_f32 in report:
        print(f"  {name:40s} {d_gpu:.3e} | {d_f32:.3e} | {d_gpu / max(d_f32, 1e-300):.2f}")
    # one Adam step (lr 5e-4, L2 weight decay 1e-5, trainer.py:115-119) on both sides
    before = {k: v.detach().cpu().clone() for k, v in params.items()}
    tr.optimizer.step()
    cparams = dict(cpu_model.gnn.named_parameters())
    opt = torch.optim.Adam(cpu_model.parameters(), lr=5e-4, weight_decay=1e-5)
    for k, gr in g32.items():
        cparams[k].grad = gr.reshape(cparams[k].shape)
    opt.step()
    for k in _key_map(m.gnn):
        if k in zero:
            continue          # zero-gradient parameters: Adam turns rounding noise into +-lr steps on either side
        new, ref = params[k].detach().cpu().reshape(cparams[k].shape), cparams[k].detach()
        assert not torch.equal(new, before[k].reshape(new.shape)), k
        # the first Adam step moves every element by lr * sign(g) (|g| >> eps): compare the step, not the weight
        step_gpu, step_ref = new - before[k].reshape(new.shape), ref - before[k].reshape(new.shape)
        big = g64[k].abs() > 1e-3 * g64[k].abs().max()            # elements whose gradient sign is well determined
        assert torch.allclose(step_gpu[big], step_ref[big], rtol=2e-2, atol=1e-6), k


def test_dropout_masks():
    m, g, trip = _setup(600, 2, dropout=0.3)
    m.train()
    torch.manual_seed(5)
    a = m(g)
    torch.manual_seed(5)
    b = m(g)
    c = m(g)
    assert torch.equal(a, b)                   # same torch seed -> same counter-based masks
    assert not torch.equal(a, c)
    loss = TripletLoss()(a[trip[:, 0]], a[trip[:, 1]], a[trip[:, 2]])
    loss.backward()
    for p in m.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    m.eval()
    with torch.no_grad():
        e = m(g)
    assert torch.isfinite(e).all()


def test_trainer_epoch_loop_and_checkpoints(tmp_path):
    """GNNTrainer.train (trainer.py:389-476): mining + accumulation loop + validation + checkpoints, end to end on a
    two-lap trajectory (revisits exist), then a checkpoint round trip into a fresh trainer."""
    from neural_spectral_codec_amd.gnn.trainer import create_trainer
    from neural_spectral_codec_amd.gnn.triplet_miner import create_triplet_miner
    from neural_spectral_codec_amd.keyframe.graph_manager import build_chain_graph
    rng = np.random.default_rng(0)
    n = 300
    t = np.linspace(0, 4 * np.pi, n)
    poses = np.tile(np.eye(4), (n, 1, 1))
    poses[:, 0, 3], poses[:, 1, 3] = 40 * np.cos(t) + rng.normal(0, .3, n), 40 * np.sin(t) + rng.normal(0, .3, n)
    desc = (rng.random((n, 800)) ** 4).astype(np.float32)
    desc /= desc.sum(1, keepdims=True)
    graph = build_chain_graph(torch.from_numpy(desc), 5, "cuda", poses)
    torch.manual_seed(0)
    m = create_spectral_gnn(edge_dim=2, dropout=0.0)
    tr = create_trainer(m, device="cuda", checkpoint_dir=str(tmp_path), batch_size=128, accumulation_steps=2, patience=5)
    tr.train(graph, poses, desc, train_sequence_ids=np.zeros(n, int), val_graph=graph, val_poses=poses, n_epochs=2,
             triplet_miner=create_triplet_miner())
    assert len(tr.train_losses) == 2 and all(np.isfinite(tr.train_losses)) and tr.global_step > 0
    assert len(tr.val_metrics) == 2 and set(tr.val_metrics[0]) >= {"recall@1", "recall@5", "recall@10"}
    assert (tmp_path / "final_model.pth").exists()
    ck = torch.load(tmp_path / "final_model.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "global_step", "model_state_dict", "optimizer_state_dict", "best_val_metric",
                       "train_losses", "val_metrics", "epochs_without_improvement"}          # trainer.py:480-489
    m2 = create_spectral_gnn(edge_dim=2, dropout=0.0)
    tr2 = create_trainer(m2, device="cuda", checkpoint_dir=str(tmp_path))
    tr2.load_checkpoint("final_model.pth")
    assert tr2.global_step == tr.global_step and tr2.epoch == tr.epoch
    m.eval(), m2.eval()
    with torch.no_grad():
        assert torch.equal(m(graph), m2(graph))
    with pytest.raises(FileNotFoundError):
        tr2.load_checkpoint("missing.pth")


def test_captured_training_step_matches_eager():
    """GNNTrainer replays the per-batch step (forward_train + TripletLoss + backward, ~75 launches) as ONE captured
    hipGraph from the second batch of a shape on.  Dropout 0: the parameters after 2 optimizer steps (8 batches, one
    ragged) must equal the eagerly issued run's up to the float32 atomics of the triplet scatter.  Dropout 0.1: the
    seed lives in a device word the kernels read (NscGatTrainCfg.seed_dev) -- two replays of the SAME batch draw
    different masks, and training still reduces the loss."""
    n = 600
    rng = np.random.default_rng(2)
    trip = np.stack([rng.integers(0, n, 1800), rng.integers(0, n, 1800), rng.integers(0, n, 1800)], 1)   # 7 x 256 + 8
    outs = []
    # (eager, gradients through autograd's AccumulateGrad) / (eager, the backward adds into .grad itself:
    # NscGatTrainCfg.accumulate_grads) / (captured, the same)
    for use_graph, direct in ((False, False), (False, True), (True, True)):
        m, g, _ = _setup(n, 2)
        tr = GNNTrainer(m, device="cuda", learning_rate=5e-4, weight_decay=1e-5, margin=0.1, batch_size=256,
                        accumulation_steps=4, use_graph=use_graph, direct_grads=direct)
        loss = tr.train_batches(g, trip)
        assert bool(tr._captured) == use_graph and not tr._capture_failed
        outs.append((loss, {k: v.detach().cpu().clone() for k, v in m.gnn.named_parameters()},
                     m.gnn.input_norm.running_mean.cpu().clone(), int(m.gnn.input_norm.num_batches_tracked)))
    (l0, p0, rm0, nb0), (l2, p2, rm2, nb2), (l1, p1, rm1, nb1) = outs
    assert nb0 == nb1 == nb2 == 8
    assert abs(l0 - l1) <= 1e-5 * abs(l0) + 1e-7 and abs(l0 - l2) <= 1e-5 * abs(l0) + 1e-7
    for k in p0:                                             # in-kernel accumulation == autograd accumulation
        assert (p0[k] - p2[k]).abs().max().item() <= 4.2 * 5e-4, k
    # (after the first optimizer step the two runs' weights differ by +-lr where a gradient is rounding noise, see below;
    #  rows of x sum to 1, so the input projection's batch mean may move by a few lr)
    assert torch.allclose(rm0, rm1, rtol=0, atol=4 * 5e-4)
    # exactly-zero gradients (pure rounding noise): a bias in front of a batch-statistics BatchNorm; and, because the triplet
    # gradient sums to zero over the rows, output_proj.bias and the last BatchNorm's bias
    zero = {"input_proj.bias", "output_proj.bias", "batch_norms.2.bias"} | {f"convs.{l}.bias" for l in range(3)}
    for k in p0:
        # two Adam steps: an element whose gradient is rounding noise steps by +-lr per step on either side (4 lr apart at
        # most); everywhere else the two runs take the same steps
        assert (p0[k] - p1[k]).abs().max().item() <= 4.2 * 5e-4, k
        if k in zero:
            continue
        frac = ((p0[k] - p1[k]).abs() > 1e-6).float().mean().item()
        assert frac < 0.02, (k, frac)
    # dropout > 0 through the capture: fresh masks per replay
    m, g, _ = _setup(n, 2, dropout=0.1)
    tr = GNNTrainer(m, device="cuda", batch_size=256, accumulation_steps=1, use_graph=True)
    m.train()
    bt = trip[:256]
    torch.manual_seed(11)
    assert tr._captured_step(g, bt, 1.0) is None                 # first sight of the shape: the caller runs it eagerly
    l_a = float(tr._captured_step(g, bt, 1.0))                   # capture + replay
    l_b = float(tr._captured_step(g, bt, 1.0))                   # replay: same batch, same weights, a new seed in the device word
    l_c = float(tr._captured_step(g, bt, 1.0))
    assert tr._captured and not tr._capture_failed
    assert len({round(v, 7) for v in (l_a, l_b, l_c)}) == 3, (l_a, l_b, l_c)   # three masks -> three losses
    m2, g2, trip2 = _setup(400, 2, dropout=0.1)
    tr2 = GNNTrainer(m2, device="cuda", learning_rate=5e-4, batch_size=256, accumulation_steps=1)
    ls = [tr2.train_batches(g2, np.concatenate([trip2] * 2)) for _ in range(8)]
    assert tr2._captured and ls[-1] < ls[0]


@pytest.mark.parametrize("n,dropout", [(700, 0.0), (1500, 0.1)])
def test_in_kernel_gradient_accumulation_is_bit_exact(n, dropout):
    """A parity bar that does not lean on the triplet scatter's float atomics: with a deterministic upstream gradient
    (loss = <emb, W>) every kernel of the backward is deterministic, so
      * two runs of the same backward agree bit for bit,
      * NscGatTrainCfg.accumulate_grads = 1 into ZEROED gradient buffers equals accumulate_grads = 0 bit for bit (0 + g = g:
        the split-K slab sums, the column-reduction finishes and the fused bias partials all add their finished float to what
        the buffer holds),
      * a second accumulating backward doubles every gradient exactly (g + g)."""
    grads = []
    for mode in ("autograd", "autograd", "direct", "direct_twice"):
        m, g, _ = _setup(n, 2, dropout=dropout, seed=5)
        m.train()
        inner = m.gnn
        torch.manual_seed(3)                                       # the dropout seed is drawn from torch's CPU generator
        W = torch.linspace(-1.0, 1.0, n * 800, device="cuda").reshape(n, 800)
        if mode != "autograd":
            for p in m.parameters():
                p.grad = torch.zeros_like(p)
            inner._direct_grads = True
        for rep in range(2 if mode == "direct_twice" else 1):
            torch.manual_seed(3)
            (m(g) * W).sum().backward()
        inner._direct_grads = False
        grads.append({k: v.grad.detach().clone() for k, v in inner.named_parameters()})
    a0, a1, d, d2 = grads
    for k in a0:
        assert torch.equal(a0[k], a1[k]), f"{k}: the backward is not deterministic"
        assert torch.equal(a0[k], d[k]), f"{k}: accumulate_grads = 1 into zeros differs from accumulate_grads = 0"
        assert torch.equal(d2[k], d[k] + d[k]), f"{k}: a second accumulating backward does not double the gradient"
        assert torch.isfinite(a0[k]).all()


def test_captured_step_gradients_match_eager():
    """What the +-lr parameter checks above cannot see (Adam normalises the gradient's magnitude away): the GRADIENTS the
    optimizer is handed after four batches -- one issued eagerly and three replays of the captured step, then four replays -- must
    equal the eagerly issued run's (same kernels; the triplet scatter's float atomics are the only difference) at every one of
    three optimizer steps, and so must every batch's loss.  Round 4: a memset NODE in the captured graph (the zeroing of the
    triplet gradient) was not ordered before the accumulating kernel in replays; the gradient sums reached 1e25-1e32."""
    n = 1500
    m0, g, _ = _setup(n, 2, seed=9)
    rng = np.random.default_rng(4)
    trip = np.stack([rng.integers(0, n, 9 * 128 + 37) for _ in range(3)], 1)
    runs = []
    for use_graph in (False, True):
        m, g, _ = _setup(n, 2, seed=9)
        tr = GNNTrainer(m, device="cuda", learning_rate=5e-4, weight_decay=1e-5, margin=0.1, batch_size=128, accumulation_steps=4,
                        use_graph=use_graph)
        seen, step = [], tr.optimizer.step
        params = dict(m.gnn.named_parameters())

        def hooked(*a, _seen=seen, _params=params, _step=step, **kw):
            _seen.append({k: v.grad.detach().clone() for k, v in _params.items()})
            return _step(*a, **kw)
        tr.optimizer.step = hooked
        loss = tr.train_batches(g, trip)
        assert bool(tr._captured) == use_graph and not tr._capture_failed
        runs.append((loss, seen))
    (l0, s0), (l1, s1) = runs
    assert len(s0) == len(s1) == 3
    assert abs(l0 - l1) <= 1e-5 * abs(l0) + 1e-7
    zero = {"input_proj.bias", "output_proj.bias", "batch_norms.2.bias"} | {f"convs.{l}.bias" for l in range(3)}
    for step_no, (ga, gb) in enumerate(zip(s0, s1)):
        scale = max(float(v.abs().max()) for v in ga.values())
        for k in ga:
            assert torch.isfinite(gb[k]).all(), (step_no, k)
            ref = float(ga[k].abs().max())
            d = float((ga[k] - gb[k]).abs().max())
            if k in zero:                                   # exactly-zero gradients: rounding noise on both sides
                assert ref < 1e-3 * scale and float(gb[k].abs().max()) < 1e-3 * scale, (step_no, k)
                continue
            # step 0: identical weights in both runs; later steps: the weights differ by +-lr on noise-only elements
            assert d <= (2e-4 if step_no == 0 else 5e-2) * max(ref, 1e-6 * scale), (step_no, k, d, ref)


def test_captured_graphs_hold_kernel_nodes_only():
    """Round 4's bug class, checked structurally: a hipMemsetAsync / hipMemcpyAsync captured into a hipGraph becomes a memset /
    memcpy NODE, and those are not ordered before the kernel node after them when the graph is replayed on ROCm 7.2.  Every
    capture the package makes -- the training step (dropout on and off), the pipelined path's GNN forward -- must consist of
    kernel nodes alone (tests/_hipgraph.py reads the node types back through the HIP runtime)."""
    from _hipgraph import keep_graphs, node_types
    from neural_spectral_codec_amd import distributed as nd, synth
    from neural_spectral_codec_amd.encoding import SpectralEncoder
    n = 600
    rng = np.random.default_rng(4)
    trip = np.stack([rng.integers(0, n, 4 * 128) for _ in range(3)], 1)
    with keep_graphs() as made:
        for dropout in (0.0, 0.1):
            m, g, _ = _setup(n, 2, dropout=dropout, seed=9)
            tr = GNNTrainer(m, device="cuda", learning_rate=5e-4, batch_size=128, accumulation_steps=2, use_graph=True)
            tr.train_batches(g, trip)
            assert tr._captured and not tr._capture_failed
        n_train = len(made)
        enc = SpectralEncoder(n_elevation=16).to("cuda")
        m, _, _ = _setup(96, 2, seed=3)
        m.eval()
        piped = nd.ShardedDescriptorPath(enc, m, 96, synth.make_pose_chain(96, 0), pipeline=True, gnn_graph=True)
        with torch.no_grad():
            for s in range(6):
                piped.step(synth.make_clouds_device(96, 3000, "cuda", seed=s))
            piped.synchronize()
        torch.cuda.synchronize()
        assert n_train == 2 and len(made) > n_train, (n_train, len(made))
        for cg in made:
            types = node_types(cg)
            assert set(types) == {"kernel"} and types["kernel"] >= 8, types


@pytest.mark.parametrize("n_layers,in_dim,out_dim,hidden", [(1, 64, 64, 64), (2, 64, 64, 64), (5, 64, 64, 64), (8, 64, 64, 64),
                                                            (3, 64, 48, 64), (8, 48, 80, 64), (4, 64, 96, 128), (8, 64, 64, 128)])
def test_other_depths_train_on_the_split_k_path(n_layers, in_dim, out_dim, hidden):
    """The end-of-backward batching (round 4) is sized by NSC_GAT_MAX_LAYERS: depths 1-8 (eight layers + output + residual_proj
    + input weight = eleven slab jobs, each with a slab region of its own, all summed in the batched launch), at
    700 nodes -- above the 512 where the weight gradients split K over slabs.  Loss, every parameter gradient and the input
    gradient against autograd through the restatement.  hidden = 128 > max(in, out): the H x H lin gradient is then the largest
    weight-gradient product -- the slab region was sized without it until round 4 (found by tools/fuzz_train.py: a fault)."""
    from neural_spectral_codec_amd.gnn.model import SpectralGNN
    n = 700
    # (fixed draws: a pre-activation of ~1e-8 that the kernels and torch round to different sides of a ReLU moves single-channel
    # gradients by 1e-3 -- a tie, not an error; tools/fuzz_train.py re-draws the features to tell the two apart.  These draws have none.)
    torch.manual_seed(6 if hidden == 64 else 21)
    m = SpectralGNN(input_dim=in_dim, hidden_dim=hidden, output_dim=out_dim, n_layers=n_layers, dropout=0.0, residual=True, edge_dim=2)
    go.randomize_bn_stats(m, 7)
    assert (m.residual_proj is not None) == (in_dim != out_dim)
    m = m.to("cuda")
    g = gm.synthetic_chain_graph(n, device="cuda", seed=9, features=torch.rand(n, in_dim))
    R = torch.randn(n, out_dim, generator=torch.Generator().manual_seed(3))
    emb_ref, grads_ref, gx_ref, _ = go.reference_gradients(m, g, lambda e: (e * R).sum() + (e * e).sum())
    m.train()
    g.x.requires_grad_(True)
    emb = m(g)
    ((emb * R.cuda()).sum() + (emb * emb).sum()).backward()
    emb64 = go.reference_gradients(m, g, lambda e: (e * 0).sum(), dtype=torch.float64)[0]
    _assert_train_forward(emb, emb_ref, emb64, f"train-mode forward, {n_layers} layers {in_dim}->{out_dim}")
    tol = 2e-3 * max(1, n_layers // 2)                       # float32 against float32: the error grows with the depth
    assert _rel(g.x.grad.cpu(), gx_ref) < tol
    params = dict(m.named_parameters())
    keys = _key_map(m) + (["residual_proj.weight", "residual_proj.bias"] if m.residual_proj is not None else [])
    gscale = max(v.abs().max().item() for v in grads_ref.values())
    for k in keys:
        got = params[k].grad.detach().cpu().reshape(grads_ref[k].shape)
        assert torch.isfinite(got).all(), k
        if k == "input_proj.bias" or k.endswith(".bias") and k.startswith("convs."):
            assert got.abs().max().item() < 1e-3 * gscale * max(1, n_layers // 2), k
            continue
        assert _rel(got, grads_ref[k]) < tol, k
    # a second backward into the same buffers accumulates: exactly twice the gradient (the batched sums add into what is there)
    first = {k: params[k].grad.detach().clone() for k in keys}
    g.x.grad = None
    emb = m(g)
    ((emb * R.cuda()).sum() + (emb * emb).sum()).backward()
    for k in keys:
        if not (k == "input_proj.bias" or k.endswith(".bias") and k.startswith("convs.")):
            assert _rel(params[k].grad.cpu(), 2 * first[k].cpu()) < 1e-5, k
