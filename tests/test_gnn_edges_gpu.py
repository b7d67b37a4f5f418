"""The cases of tests/gnn_edge_cases.py on the device, in every kernel set of the inference forward (nsc_gat_forward_ex) and,
where a case says so, through the training step.  tests/test_gnn_edges_cpu.py proves what is expected here on the restatement.

  nan_* / inf_*   the output row is all NaN exactly on the breadth-first ball of the poisoned entry and keeps the bytes of the
                  clean call elsewhere -- through the forward, forward_with_attention, a captured replay and the training step.
                  Before the ReLUs of the GNN path kept a NaN (relu_nan, csrc/nsc_gat_epilogue.h) every nan_* case whose ball is
                  more than the poisoned row itself failed here with finite rows inside the ball.
  range_* / shape_*   within the element-wise bar of the float32 and the float64 restatement, every kernel set the same bytes,
                  attention weights against the reference's; range_* also through the training forward and backward."""
import copy
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import _hipgraph
import gat_oracle as go
import gnn_edge_cases as ec
import test_train_gpu as ttg
import train_families as tf
from neural_spectral_codec_amd import _lib
from neural_spectral_codec_amd.gnn import model as gnn_model

pytestmark = pytest.mark.gpu


def _dev(g):
    d = SimpleNamespace(x=g.x.cuda(), edge_index=g.edge_index.cuda(), num_nodes=g.num_nodes)
    if getattr(g, "edge_attr", None) is not None:
        d.edge_attr = g.edge_attr.cuda()
    return d


def _forward_sets(m, g):
    """{kernel set: output} of one graph"""
    outs = {}
    with torch.no_grad():
        for ks in ec.KERNEL_SETS:
            m.coresident = ks
            outs[ks] = m(g).clone()
    m.coresident = False
    return outs


def _attention_sets(m, g):
    """{kernel set: (output, [alpha of layer l in PyG order])} through forward_with_attention"""
    outs = {}
    with torch.no_grad():
        for ks in ec.KERNEL_SETS:
            m.coresident = ks
            out, att = m.forward_with_attention(g)
            outs[ks] = (out.clone(), [a[:, 0].clone() for _, a in att])
    m.coresident = False
    return outs


# ------------------------------------------------------------------------------------------------------------------
# nan_* / inf_*
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.NONFINITE)
def test_nonfinite_forward(name):
    case = ec.build(name)
    m = copy.deepcopy(case.model).cuda().eval()
    got, clean = _forward_sets(m, _dev(case.graph)), _forward_sets(m, _dev(case.clean))
    for ks in ec.KERNEL_SETS:
        ec.check_ball(got[ks], clean[ks], case.ball, f"{name}, kernel set {ks!r}")
    for ks in ec.KERNEL_SETS[1:]:
        assert torch.equal(ec.bits(clean[ks]), ec.bits(clean[False])), f"{name}: kernel set {ks!r} differs on the clean input"
        assert torch.equal(torch.isnan(got[ks]).cpu(), torch.isnan(got[False]).cpu())
        assert torch.equal(ec.bits(torch.nan_to_num(got[ks])), ec.bits(torch.nan_to_num(got[False]))), f"{name}: kernel set {ks!r}"


@pytest.mark.parametrize("name", ec.NONFINITE)
def test_nonfinite_forward_with_attention(name):
    """The softmax maxima are fmaxf, which drops a NaN -- and expf(NaN - m) brings it back: the weights of a target with one NaN
    logit are all NaN, layer by layer on the ball of that layer, and sum to 1 for every other target"""
    case = ec.without_edge_attr(ec.build(name))
    n = case.graph.num_nodes
    m = copy.deepcopy(case.model).cuda().eval()
    got, clean = _attention_sets(m, _dev(case.graph)), _attention_sets(m, _dev(case.clean))
    targets = ec.entry_targets(case.graph.edge_index, n)
    for ks in ec.KERNEL_SETS:
        ec.check_ball(got[ks][0], clean[ks][0], case.ball, f"{name}, kernel set {ks!r}")
        for l in range(ec.L):
            ec.check_alpha(got[ks][1][l], clean[ks][1][l], targets, case.layer_balls[l], n, f"{name}, kernel set {ks!r}, layer {l}")
            assert torch.equal(ec.bits(clean[ks][1][l]), ec.bits(clean[False][1][l]))


@pytest.mark.parametrize("name", ec.NONFINITE)
def test_nonfinite_captured_replay(name):
    case = ec.build(name)
    m = copy.deepcopy(case.model).cuda().eval()
    g, gc = _dev(case.graph), _dev(case.clean)
    with torch.no_grad():
        clean = m(gc).clone()

        def step():
            return {"out": m(g)}
        eager, replayed, nodes = _hipgraph.capture_replay(step)
    assert set(nodes) == {"kernel"}, nodes
    ec.check_ball(eager["out"], clean, case.ball, f"{name}, eager")
    ec.check_ball(replayed["out"], clean, case.ball, f"{name}, replayed")


def _train_step(gnn, g, ws, tt, grad_out=None):
    """nsc_gat_forward_train into the caller's workspace, nsc_triplet_loss and nsc_gat_backward (upstream gradient: the triplet
    loss's own, or `grad_out`).  -> (embedding, loss, parameter gradients, input gradient)"""
    x = g.x.detach().to(torch.float32).contiguous()
    csr = gnn._csr(g, gnn._uses_edge_attr(g))
    csr.ensure_transpose()
    ms, gs = gnn._train_struct(), csr.struct()
    cfg = _lib.GatTrainCfg()
    cfg.dropout_p, cfg.bn_momentum, cfg.seed, cfg.update_running_stats = 0.0, 0.1, 0, 1
    nbytes = _lib.lib().nsc_gat_train_workspace_bytes(C.byref(ms), C.byref(gs))
    assert ws.numel() == nbytes
    out = torch.empty((x.shape[0], gnn.output_dim), dtype=torch.float32, device=x.device)
    _lib.call("nsc_gat_forward_train", x.device, ms, gs, x, csr.edge_attr, cfg, out, ws, nbytes, _lib.STREAM)
    loss, grad = gnn_model._triplet_loss(out, tt[:, 0].contiguous(), tt[:, 1].contiguous(), tt[:, 2].contiguous(),
                                         ec.TRIPLET_MARGIN, 1.0, True)
    grads = [torch.empty_like(p) for p in gnn._train_params()]
    gx = gnn_model._train_backward_raw(gnn, (csr, cfg, ws, nbytes, x, None), grad if grad_out is None else grad_out, grads, False, True)
    return out, loss, grads, gx


def _train_ws(gnn, g):
    csr = gnn._csr(g, gnn._uses_edge_attr(g))
    csr.ensure_transpose()
    ms, gs = gnn._train_struct(), csr.struct()
    return torch.empty(_lib.lib().nsc_gat_train_workspace_bytes(C.byref(ms), C.byref(gs)), dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("name", [k for k in ec.NONFINITE if ec.CASES[k]["train"]])
def test_nonfinite_training_step(name):
    """Train mode: the batch statistics carry the NaN into every row, and the triplet loss over NaN rows is NaN, as torch.relu of
    a NaN is.  Nothing stays behind in the workspace: the next clean step in it equals a clean step in a fresh one, bit for
    bit (with a fixed upstream gradient: the triplet scatter's float atomics are not ordered)."""
    case = ec.build(name)
    n = case.graph.num_nodes
    tt = ec.triplets(n).cuda()
    W = torch.linspace(-1.0, 1.0, n * case.spec["out_dim"], device="cuda").reshape(n, case.spec["out_dim"])
    g, gc = _dev(case.graph), _dev(case.clean)
    used = copy.deepcopy(case.model).cuda().train()
    ws = _train_ws(used, g)
    out, loss, grads, gx = _train_step(used, g, ws, tt)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), f"{name}: {int(torch.isfinite(out).sum())} finite elements in the train-mode embedding"
    assert bool(torch.isnan(loss).all()), f"{name}: the loss is {loss.item()}"
    if n > 1:
        used.load_state_dict(case.model.state_dict())          # the running statistics took the NaN, as nn.BatchNorm1d's would
        fresh = copy.deepcopy(case.model).cuda().train()
        a = _train_step(used, gc, ws, tt, grad_out=W)
        b = _train_step(fresh, gc, _train_ws(fresh, gc), tt, grad_out=W)
        assert bool(torch.isfinite(b[0]).all()) and bool(torch.isfinite(b[1]).all())
        assert torch.equal(ec.bits(a[0]), ec.bits(b[0])) and torch.equal(ec.bits(a[1]), ec.bits(b[1]))
        for p, q in zip(a[2] + [a[3]], b[2] + [b[3]]):
            assert torch.equal(ec.bits(p), ec.bits(q))


# ------------------------------------------------------------------------------------------------------------------
# range_* / shape_*
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.RANGE + ec.SHAPE)
def test_finite_case_forward(name):
    case, ref = ec.build(name), ec.references(name)
    m = copy.deepcopy(case.model).cuda().eval()
    got = _forward_sets(m, _dev(case.graph))
    w32 = ttg._bar_ratio(got[False], ref.out32)
    w64 = ttg._bar_ratio(got[False], ref.out64)
    print(f"{name}: worst element / bar {w32:.2f} vs the float32 restatement, {w64:.2f} vs the float64 restatement")
    for ks in ec.KERNEL_SETS[1:]:
        assert torch.equal(ec.bits(got[ks]), ec.bits(got[False])), f"{name}: kernel set {ks!r} differs"
    go.assert_within_bar(got[False], ref.out32, what=f"{name} vs float32 restatement")
    go.assert_within_bar(got[False], ref.out64, what=f"{name} vs float64 restatement")


@pytest.mark.parametrize("name", ec.RANGE + ec.SHAPE)
def test_finite_case_attention(name):
    """forward_with_attention (the convs without edge_attr): every layer's weights against the float64 reference's, at the
    tolerances of test_gat_gpu.py::test_forward_with_attention"""
    case, ref = ec.without_edge_attr(ec.build(name)), ec.references(name, edge_attr=False)
    n = case.graph.num_nodes
    m = copy.deepcopy(case.model).cuda().eval()
    got = _attention_sets(m, _dev(case.graph))
    targets = ec.entry_targets(case.graph.edge_index, n)
    out, alphas = got[False]
    go.assert_within_bar(out, ref.out64, what=f"{name} without edge_attr vs float64 restatement")
    for l in range(ec.L):
        a, a_ref = alphas[l].cpu(), ref.taps64[f"l{l}.alpha"]
        assert torch.allclose(a.double(), a_ref, rtol=1e-4, atol=1e-6), \
            f"{name} layer {l}: weights off by {(a.double() - a_ref).abs().max().item():.3g}"
        s = torch.zeros(n, dtype=torch.float64).index_add_(0, targets, a.double())
        assert torch.allclose(s, torch.ones(n, dtype=torch.float64), rtol=0, atol=1e-5)
    for ks in ec.KERNEL_SETS[1:]:
        assert torch.equal(ec.bits(got[ks][0]), ec.bits(out))
        for l in range(ec.L):
            assert torch.equal(ec.bits(got[ks][1][l]), ec.bits(alphas[l])), f"{name}: kernel set {ks!r}, layer {l}"


@pytest.mark.parametrize("name", ec.RANGE)
def test_range_case_training_step(name):
    """Forward and backward at the case's train_factor, held as tests/test_train_gpu.py::test_forward_train_and_gradients
    holds its models: the embedding by _assert_train_forward, the loss to 1e-4, every gradient to 2e-3 of its largest element
    against reference_gradients (float32)"""
    case, ref = ec.build(name), ec.train_references(name)
    n = case.graph.num_nodes
    _, tt, R = ec.train_loss(n, case.spec["out_dim"])
    m = copy.deepcopy(ref.model).cuda().train()
    g = _dev(case.graph)
    g.x.requires_grad_(True)
    emb = m(g)
    a, p, q = emb[tt[:, 0].cuda()], emb[tt[:, 1].cuda()], emb[tt[:, 2].cuda()]
    loss = torch.relu(((a - p) ** 2).sum(1) - ((a - q) ** 2).sum(1) + ec.TRIPLET_MARGIN).mean() + (emb * R.cuda()).sum()
    loss.backward()
    ttg._assert_train_forward(emb, ref.emb32, ref.emb64, f"{name}, train-mode forward")
    assert abs(loss.item() - ref.loss32.item()) <= 1e-4 * abs(ref.loss32.item()) + 1e-6
    params = dict(m.named_parameters())
    gscale = max(v.abs().max().item() for v in ref.grads32.values())
    worst = (0.0, None)
    for k in ttg._key_map(m):
        got = params[k].grad.detach().cpu().reshape(ref.grads32[k].shape)
        if tf.is_zero_grad(k):
            assert got.abs().max().item() < 1e-3 * gscale and ref.grads32[k].abs().max().item() < 1e-3 * gscale, k
            continue
        worst = max(worst, (ttg._rel(got, ref.grads32[k]), k))
    gx = ttg._rel(g.x.grad.cpu(), ref.gx32)
    print(f"{name}: worst gradient {worst[0]:.2e} ({worst[1]}), input gradient {gx:.2e} of the largest element (bar 2e-3)")
    assert worst[0] < 2e-3, worst
    assert gx < 2e-3
