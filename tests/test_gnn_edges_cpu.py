"""What tests/test_gnn_edges_gpu.py relies on, proved on the restatement (oracle/gat_oracle.py) without a GPU: the expected NaN
balls of the nan_* / inf_* cases, the logit range, weight spread and float32 accuracy each range_* case states, the degrees and
chunk widths the shape_* cases claim -- and that restatements with the defects the cases are there for (a ReLU that drops NaN,
a softmax without the max subtraction, a maximum over the first 64 entries only) fail the same comparisons."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gat_oracle as go
import gnn_edge_cases as ec
import train_families as tf


# ------------------------------------------------------------------------------------------------------------------
# nan_* / inf_*
# ------------------------------------------------------------------------------------------------------------------
def _check_nonfinite(case, dtype):
    n = case.graph.num_nodes
    taps, taps_clean = {}, {}
    out = go.forward_reference(case.model, case.graph, dtype=dtype, taps=taps)
    clean = go.forward_reference(case.model, case.clean, dtype=dtype, taps=taps_clean)
    ec.check_ball(out, clean, case.ball, f"{case.name} {dtype}")
    targets = ec.entry_targets(case.graph.edge_index, n)
    for l in range(ec.L):
        ec.check_alpha(taps[f"l{l}.alpha"], taps_clean[f"l{l}.alpha"], targets, case.layer_balls[l], n, f"{case.name} {dtype} layer {l}")


@pytest.mark.parametrize("name", ec.NONFINITE)
def test_reference_is_nan_exactly_on_the_ball(name):
    """forward_reference, float32 and float64, eval mode: all-NaN rows exactly on the breadth-first ball, every other row the
    bits of the clean call; per layer, NaN attention weights exactly for the targets within l + 1 hops.  Also as
    forward_with_attention runs the convs (no edge_attr: a poisoned attribute then poisons nothing)."""
    case = ec.build(name)
    assert len(case.ball) > 0 and not (len(case.ball) == case.graph.num_nodes and case.graph.num_nodes > 1)
    for dtype in (torch.float32, torch.float64):
        _check_nonfinite(case, dtype)
        _check_nonfinite(ec.without_edge_attr(case), dtype)


@pytest.mark.parametrize("name", ec.NONFINITE)
def test_reference_train_mode_is_nan_everywhere(name):
    """Batch statistics carry one NaN into every row: the embedding is all NaN and so is the triplet loss"""
    case = ec.build(name)
    n = case.graph.num_nodes
    tt = ec.triplets(n)
    for dtype in (torch.float32, torch.float64):
        emb = go.forward_reference(case.model, case.graph, training=True, dtype=dtype)
        assert bool(torch.isnan(emb).all())
        assert bool(torch.isnan(go.triplet_loss_reference(emb, tt[:, 0], tt[:, 1], tt[:, 2], ec.TRIPLET_MARGIN)))
        assert bool(torch.isfinite(go.forward_reference(case.model, case.clean, training=True, dtype=dtype)).all()) or n == 1


def test_ball_is_a_breadth_first_search():
    """The expectation itself, on graphs small enough to read: hops follow the edge direction, the start is in the ball, a node
    without edges is its own ball"""
    ei = torch.tensor([[0, 1, 2, 4], [1, 2, 3, 0]])                       # 4 -> 0 -> 1 -> 2 -> 3, node 5 alone
    assert ec.ball(ei, 6, [0], 0).tolist() == [0]
    assert ec.ball(ei, 6, [0], 2).tolist() == [0, 1, 2]
    assert ec.ball(ei, 6, [0], 3).tolist() == [0, 1, 2, 3]                # never upstream to 4
    assert ec.ball(ei, 6, [5], 3).tolist() == [5]
    assert ec.ball(ei, 6, [4, 2], 1).tolist() == [0, 2, 3, 4]
    chain = ec.build("nan_chain")
    assert chain.ball.tolist() == list(range(14, 27))                    # +-2 rows per hop, three hops around row 20
    assert [b.tolist() for b in ec.build("nan_edge_attr_chain").layer_balls] == [[20], list(range(18, 23)), list(range(16, 25))]
    assert ec.build("nan_isolated").ball.tolist() == [199] and ec.build("nan_n1").ball.tolist() == [0]
    a, b = ec.ball(chain.graph.edge_index, 40, [15], 3), ec.ball(chain.graph.edge_index, 40, [19], 3)
    assert len(np.intersect1d(a, b)) > 0 and ec.build("nan_overlap").ball.tolist() == np.union1d(a, b).tolist()
    hub = ec.build("nan_hub_source")                                     # the 64-entry source reaches hubs and chain alike
    assert len(hub.ball) > 64 and len(hub.ball) < 200


class _DropNaN:
    """torch.nn.functional as gat_oracle sees it, with the ReLU of the kernels before the fix: fmaxf(v, 0) is 0 for a NaN"""
    leaky_relu = staticmethod(F.leaky_relu)

    @staticmethod
    def relu(v):
        return torch.where(v > 0, v, torch.zeros_like(v))


@pytest.mark.parametrize("name", [k for k in ec.NONFINITE if k.startswith("nan_")])
def test_a_relu_that_drops_nan_fails_the_comparison(name, monkeypatch):
    """... in every case whose ball is more than the poisoned row itself: that row is NaN whatever the ReLU does, through the
    residual projection of x (nan_isolated, nan_n1)"""
    case = ec.build(name)
    if name in ("nan_isolated", "nan_n1"):
        assert case.ball.tolist() == case.poisoned_rows
        return
    assert len(case.ball) > len(case.poisoned_rows)
    clean = go.forward_reference(case.model, case.clean)
    monkeypatch.setattr(go, "F", _DropNaN)
    out = go.forward_reference(case.model, case.graph)
    assert torch.equal(go.forward_reference(case.model, case.clean), clean)          # the same ReLU on finite values
    with pytest.raises(AssertionError):
        ec.check_ball(out, clean, case.ball, name)


# ------------------------------------------------------------------------------------------------------------------
# range_*
# ------------------------------------------------------------------------------------------------------------------
def _logits_alphas(taps):
    lg = torch.cat([taps[f"l{l}.logit"].detach() for l in range(ec.L)])
    al = torch.cat([taps[f"l{l}.alpha"].detach() for l in range(ec.L)])
    return lg, al


def _mid_share(al):
    return ((al > ec.RANGE_MID_LO) & (al < ec.RANGE_MID_HI)).double().mean().item()


@pytest.mark.parametrize("name", ec.RANGE)
def test_range_case_is_what_it_states(name):
    case, ref = ec.build(name), ec.references(name)
    lg, al = _logits_alphas(ref.taps64)
    share = _mid_share(al)
    d = (ref.out32.double() - ref.out64).abs()
    ratio = (d / (1e-4 * ref.out64.abs() + 1e-6)).max().item()
    print(f"{name}: logits {lg.min().item():.0f}..{lg.max().item():.0f} | mid-range weights {share:.2f} | float32 vs float64 "
          f"{ratio:.2f} of the bar")
    assert lg.max().item() > 100 and lg.min().item() < -100
    assert share >= case.spec["mid_share"]
    go.assert_within_bar(ref.out32, ref.out64, rtol=0.5e-4, atol=0.5e-6, what=f"{name}: float32 vs float64 restatement, half the bar")
    with ec.folded_order():
        go.assert_within_bar(ec.forward32(case.model, case.graph), ref.out64, rtol=0.5e-4, atol=0.5e-6,
                             what=f"{name}: float32 restatement in the folded order vs float64")
    # ... and as forward_with_attention runs the convs: the output and every layer's weights, in both orders
    plain, ref = ec.without_edge_attr(case), ec.references(name, edge_attr=False)
    for order in (contextlib.nullcontext, ec.folded_order):
        taps32 = {}
        with order():
            out32 = ec.forward32(plain.model, plain.graph, taps=taps32)
        go.assert_within_bar(out32, ref.out64, rtol=0.5e-4, atol=0.5e-6, what=f"{name} without edge_attr: float32 vs float64 restatement")
        for l in range(ec.L):
            go.assert_within_bar(taps32[f"l{l}.alpha"], ref.taps64[f"l{l}.alpha"], rtol=0.5e-4, atol=0.5e-6,
                                 what=f"{name} without edge_attr: float32 vs float64 weights of layer {l}")


def _csr_rows(case):
    perm, row_ptr = go.csr_order(case.graph.edge_index, case.graph.num_nodes)
    return lambda v, t: v[perm[row_ptr[t]:row_ptr[t + 1]]]


def test_range_equal_has_equal_logits():
    """Targets 20 (one logit per lane) and 40 (the loop over 64-entry blocks): every layer-0 logit of the row is the same number,
    so every weight is 1 / degree -- a softmax that divides by anything but the row's own sum shows at once"""
    case, ref = ec.build("range_equal"), ec.references("range_equal")
    row = _csr_rows(case)
    for t, deg in ((20, 64), (40, 128)):
        lg, al = row(ref.taps64["l0.logit"], t), row(ref.taps64["l0.alpha"], t)
        assert len(lg) == deg and bool((lg == lg[0]).all())
        assert torch.allclose(al, torch.full_like(al, 1.0 / deg), rtol=1e-12, atol=0)


def test_range_late_max_sits_past_entry_64():
    case, ref = ec.build(ec.LATE_MAX["case"]), ec.references(ec.LATE_MAX["case"])
    row = _csr_rows(case)
    ei = go.add_self_loops_mean(case.graph.edge_index, None, case.graph.num_nodes)[0]
    t, l = ec.LATE_MAX["target"], ec.LATE_MAX["layer"]
    lg = F.leaky_relu(row(ref.taps64[f"l{l}.logit"], t), 0.2)
    src = row(ei[0], t)
    assert len(lg) == 128 and int(lg.argmax()) >= ec.K.LANE_DEG and int(src[lg.argmax()]) == ec.LATE_MAX["source"]
    assert ec.LATE_MAX["source"] not in src[:ec.K.LANE_DEG].tolist()
    gap = (lg[ec.K.LANE_DEG:].max() - lg[:ec.K.LANE_DEG].max()).item()
    print(f"largest logit of target {t}, layer {l}: entry {int(lg.argmax()) + 1}, {gap:.1f} above the first {ec.K.LANE_DEG}")
    assert gap > ec.EXP_OVERFLOW


def _gatconv_mutant(mode):
    """gatconv_reference with a defective softmax: 'nomax' subtracts nothing, 'first64' takes the maximum over the first 64
    entries of each target's CSR row only (the loop form of gat_aggregate_kernel forgetting its later blocks)"""
    def conv(x, edge_index, edge_attr, lin_w, att_src, att_dst, lin_edge_w, att_edge, bias, negative_slope=0.2, taps=None,
             tap_prefix="", att_mask=None):
        n = x.shape[0]
        h = x @ lin_w.t()
        a_src, a_dst = (h * att_src.view(1, -1)).sum(-1), (h * att_dst.view(1, -1)).sum(-1)
        ei, ea = go.add_self_loops_mean(edge_index, edge_attr if lin_edge_w is not None else None, n)
        j, i = ei[0], ei[1]
        logit = a_src[j] + a_dst[i]
        if ea is not None and lin_edge_w is not None:
            logit = logit + ((ea @ lin_edge_w.t()) * att_edge.view(1, -1)).sum(-1)
        logit = F.leaky_relu(logit, negative_slope)
        if mode == "nomax":
            m = torch.zeros(n, dtype=x.dtype)
        else:
            perm, row_ptr = go.csr_order(edge_index, n)
            m = torch.stack([logit[perm[row_ptr[t]:min(row_ptr[t + 1], row_ptr[t] + 64)]].max() for t in range(n)])
        p = torch.exp(logit - m[i])
        den = torch.zeros(n, dtype=x.dtype).index_add_(0, i, p)
        alpha = p / (den[i] + 1e-16)
        return torch.zeros_like(h).index_add_(0, i, alpha.unsqueeze(1) * h[j]) + bias
    return conv


@pytest.mark.parametrize("name", ec.RANGE)
def test_softmax_without_max_subtraction_fails_the_comparison(name, monkeypatch):
    case, ref = ec.build(name), ec.references(name)
    monkeypatch.setattr(go, "gatconv_reference", _gatconv_mutant("nomax"))
    out = ec.forward32(case.model, case.graph)
    with pytest.raises(AssertionError):
        go.assert_within_bar(out, ref.out64)


def test_maximum_over_the_first_64_entries_fails_the_comparison(monkeypatch):
    name = ec.LATE_MAX["case"]
    case, ref = ec.build(name), ec.references(name)
    monkeypatch.setattr(go, "gatconv_reference", _gatconv_mutant("first64"))
    out = ec.forward32(case.model, case.graph)
    with pytest.raises(AssertionError):
        go.assert_within_bar(out, ref.out64)
    # ... and it is this case that catches it: where no late entry leads by 88.73 the shifted softmax is the same softmax
    other = ec.build("range_chain")
    go.assert_within_bar(ec.forward32(other.model, other.graph), ec.references("range_chain").out64)


def _rel(a, b):
    """tests/test_train_gpu.py's gradient figure: largest difference over largest reference element"""
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


@pytest.mark.parametrize("name", ec.RANGE)
def test_range_case_train_mode_is_what_it_states(name):
    """train_factor: the train-mode float64 logits pass +-100 and the float32 gradients sit within a quarter of the 2e-3 bar"""
    ref = ec.train_references(name)
    lg, al = _logits_alphas(ref.taps64)
    worst = max((_rel(ref.grads32[k].double(), ref.grads64[k]), k) for k in ref.grads64 if not tf.is_zero_grad(k))
    gx = _rel(ref.gx32.double(), ref.gx64)
    print(f"{name}: train-mode logits {lg.min().item():.0f}..{lg.max().item():.0f} | mid-range weights {_mid_share(al):.2f} | "
          f"float32 vs float64 gradients {worst[0]:.1e} ({worst[1]}), input gradient {gx:.1e}")
    assert lg.max().item() > 100 and lg.min().item() < -100
    assert worst[0] < 0.25 * 2e-3 and gx < 0.25 * 2e-3
    # the folded order: the same gradient margin, and the same RMS error of the embedding within 1.25 x
    case = ec.build(name)
    loss_fn, _, _ = ec.train_loss(case.spec["n"], case.spec["out_dim"])
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with ec.folded_order():
            emb, grads, gxf, _ = go.reference_gradients(ref.model, case.graph, loss_fn)
    finally:
        torch.set_num_threads(threads)
    worst_f = max((_rel(grads[k].double(), ref.grads64[k]), k) for k in ref.grads64 if not tf.is_zero_grad(k))
    rms = lambda e: (e.double() - ref.emb64).pow(2).mean().sqrt().item()
    print(f"    folded order: gradients {worst_f[0]:.1e} ({worst_f[1]}); RMS error of the embedding {rms(ref.emb32):.2e} / {rms(emb):.2e}")
    assert worst_f[0] < 0.25 * 2e-3 and _rel(gxf.double(), ref.gx64) < 0.25 * 2e-3
    assert max(rms(emb), rms(ref.emb32)) <= 1.25 * min(rms(emb), rms(ref.emb32))


# ------------------------------------------------------------------------------------------------------------------
# shape_*
# ------------------------------------------------------------------------------------------------------------------
def test_shape_cases_reach_what_they_claim():
    assert ec.K.LANE_DEG == 64 and ec.K.UR == [4, 8] and ec.K.CH_COLS == 256
    hub = ec.build("shape_hub_64_edge")
    din, dout = tf.degrees(hub.graph.edge_index.numpy(), 200)
    assert [int(din[t]) for t in (10, 20, 30, 40, 50)] == [63, 64, 65, 128, 129]
    assert [int(dout[s]) for s in (55, 57)] == [64, 65]
    reached = {ec.chunks(ec.CASES[k]["hidden"]) for k in ec.SHAPE if k.startswith("shape_hub")}
    assert reached == {(1, 64), (2, 16), (3, 16), (4, 16), (4, 256)}          # CH 1..4, a 16-column last chunk at 272 / 528 / 784
    for k in ec.SHAPE:
        if k.startswith("shape_hub"):
            assert ec.CASES[k]["graph"] == "hub" and ec.CASES[k]["n"] == 200
    assert {ec.CASES[k]["edge_dim"] for k in ec.SHAPE if k.startswith("shape_hub")} == {2, None}
    for k in ("shape_degrees_64", "shape_degrees_272"):
        c = ec.build(k)
        din, _ = tf.degrees(c.graph.edge_index.numpy(), c.graph.num_nodes)
        assert sorted(set(din.tolist())) == list(range(1, 10))
        for ur in ec.K.UR:
            assert {int(d) % ur for d in din} == set(range(ur))
    assert ec.chunks(272) == (2, 16)
    # the range cases' hub targets sit on both sides of the one-logit-per-lane switch as well
    din, _ = tf.degrees(ec.build("range_hub_64").graph.edge_index.numpy(), 200)
    assert int(din.max()) > ec.K.LANE_DEG and int((din == ec.K.LANE_DEG).sum()) >= 1


@pytest.mark.parametrize("name", ec.SHAPE)
def test_shape_case_restatements_agree(name):
    """The float32 restatement within the bar of the float64 one: the bar is a fair one for the kernels at these shapes"""
    ref = ec.references(name)
    go.assert_within_bar(ref.out32, ref.out64, what=f"{name}: float32 vs float64 restatement")


def test_every_case_is_small():
    for k, c in ec.CASES.items():
        assert c["n"] <= 200 and c["out_dim"] in (32, 50) and c["hidden"] in (64, 272, 528, 784, 1024), k
        assert not c["train"] or c["out_dim"] % 4 == 0, k                     # the training step stores float4s
