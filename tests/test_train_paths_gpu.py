"""Every dispatch path of the training step (csrc/nsc_gat_train.hip) on the device, against the float64 evaluation of the
restatement -- dropout included, through explicit masks.  tests/train_families.py holds the families, the restated host
dispatch and the literal row every family claims; tests/test_train_families_cpu.py checks those claims without a GPU.

The bar.  e(T) = ||T - T64||_F / ||T64||_F per tensor (embedding, loss, every parameter gradient, the input gradient, the
running statistics of all L + 1 BatchNorms), and for the node-indexed tensors also the worst row.  The float32 evaluation of the
same restatement gives e32_fam = the largest e(T) of the family; the kernels are held to e_gpu(T) <= K_BAR x e32_fam for every
tensor, and the worst rows to K_BAR x the float32 restatement's worst row.  K_BAR (tests/train_families.py) is twice the worst
ratio measured on the MI355X, rounded up; DESIGN.md section 4.3a has the table.  Every case prints its figures before it asserts."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gat_oracle as go
import train_families as tf

pytestmark = pytest.mark.gpu


def _report(what, ratios):
    worst = max(ratios, key=ratios.get)
    print(f"RATIO {what}: worst e_gpu / e32_fam {ratios[worst]:.2f} ({worst}); " +
          " ".join(f"{k}={v:.2f}" for k, v in sorted(ratios.items(), key=lambda kv: -kv[1])[:4]))


def check_family(name):
    """The common check: the claimed dispatch row, then one train-mode forward + backward against the float64 restatement."""
    fam = tf.family(name)
    assert tf.row_str(fam.paths) == tf.CLAIMS[name]
    r32, r64 = tf.reference(fam, torch.float32), tf.reference(fam, torch.float64)
    got = tf.run_gpu(fam)
    if not fam.spec["aligned"]:
        assert got["x"].data_ptr() % 16 == 4 and got["x"].is_contiguous()
    e32, rows32 = tf.figures(r32, r64)
    eg, rowsg = tf.figures(got, r64)
    e32_fam, rows32_fam = max(e32.values()), max(rows32.values())
    ratios = {k: v / e32_fam for k, v in eg.items()}
    ratios.update({k + " (worst row)": v / rows32_fam for k, v in rowsg.items()})
    _report(name + f" (e32_fam {e32_fam:.2e}, worst row {rows32_fam:.2e})", ratios)
    assert all(np.isfinite(v) for v in ratios.values())
    for k, v in ratios.items():
        assert v <= tf.K_BAR, f"{name}: {k} is {v:.2f} x the float32 restatement's error, bar {tf.K_BAR}"
    assert got["num_batches_tracked"] == [1] * (fam.spec["L"] + 1)
    # exactly-zero gradients: a bias in front of a batch-statistics BatchNorm holds rounding noise on both sides; an edge term
    # the forward did not have is exactly zero
    gscale = max(v.abs().max().item() for k, v in r64.items() if k.startswith("grad ") and k != "grad x")
    for k, v in got.items():
        if not k.startswith("grad ") or k == "grad x":
            continue
        if tf.is_zero_grad(k[5:]):
            assert v.abs().max().item() < 1e-3 * gscale and r32[k].abs().max().item() < 1e-3 * gscale, k
        elif k not in r64:
            assert "edge" in k and not fam.spec["attr"] and not bool(v.any()), k
    return fam, got


NO_DROPOUT = [n for n in tf.FAMILIES if tf.FAMILIES[n]["p"] == 0]
DROPOUT = [n for n in tf.FAMILIES if tf.FAMILIES[n]["p"] > 0]


@pytest.mark.parametrize("name", NO_DROPOUT)
def test_family(name):
    check_family(name)


@pytest.mark.parametrize("name", DROPOUT)
def test_dropout_family(name):
    """The reference is the float64 restatement with dropout_masks(...) of the seed the forward drew: one flipped keep bit moves an
    embedding row by far more than the bar, which pins the mask indices of the forward (bn_act_kernel, both forms of agg_train_kernel)
    and of the four regenerations in the backward (bn_bwd_colsum_kernel, both forms of att_bwd_target_kernel, att_bwd_source_kernel)."""
    fam, got = check_family(name)
    # another seed: other masks in the restatement, another embedding on the device
    f = fam.spec
    other = tf.dropout_masks(tf.seed_of(fam.torch_seed + 1), f["p"], f["N"], f["dims"][1], f["L"], fam.graph.edge_index.numpy())
    assert all(not torch.equal(a, b) for a, b in zip(other["att"] + other["feat"], fam.masks["att"] + fam.masks["feat"]))
    m = copy.deepcopy(fam.model).to("cuda").train()
    g = SimpleNamespace(x=fam.graph.x.cuda(), edge_index=fam.graph.edge_index.cuda(), edge_attr=fam.graph.edge_attr.cuda(),
                        num_nodes=f["N"])
    with torch.no_grad():
        torch.manual_seed(fam.torch_seed)
        same = m(g).cpu()
        torch.manual_seed(fam.torch_seed + 1)
        diff = m(g).cpu()
    assert torch.equal(same, got["emb"]) and not torch.equal(diff, got["emb"])


def test_absent_edge_term_leaves_accumulated_gradients_untouched():
    """A model with edge_dim = 2 fed a graph without edge_attr: with the backward adding into existing .grad tensors
    (_direct_grads) the gradients of lin_edge / att_edge are left as they are, every other gradient has the step's added."""
    fam = tf.family("edge-none-fed")
    m = copy.deepcopy(fam.model).to("cuda").train()
    g = SimpleNamespace(x=fam.graph.x.cuda(), edge_index=fam.graph.edge_index.cuda(), num_nodes=fam.spec["N"])
    for p in m.parameters():
        p.grad = torch.full_like(p, 0.25)
    m._direct_grads = True
    emb = m(g)
    ((emb * fam.R.cuda()).sum() + (emb * emb).sum()).backward()
    m._direct_grads = False
    r64 = tf.reference(fam, torch.float64)
    for k, p in m.named_parameters():
        if "lin_edge" in k or "att_edge" in k:
            assert bool((p.grad == 0.25).all()), k
        elif not tf.is_zero_grad(k):
            want = r64["grad " + k].reshape(p.shape) + 0.25
            # (the gradients themselves are held to the bar by test_family[edge-none-fed]; here only that the step's
            # gradient was ADDED: 1e-4 of ||g + 0.25|| is far below ||g|| for every tensor, far above float32 rounding)
            assert tf.err(p.grad, want) < 1e-4, k
            assert not bool((p.grad == 0.25).all()), k


def test_coverage_of_the_family_list():
    """Between them the literal rows cover every path of the host dispatch (the list is in train_families.coverage_gaps)"""
    assert tf.coverage_gaps() == []
    assert set(NO_DROPOUT + DROPOUT) == set(tf.CLAIMS)


# ---- nsc_triplet_loss ------------------------------------------------------------------------------------------------------
def _triplet_case(D, T, kind, n=300):
    """Embeddings and triplets whose hinge arguments keep 100 float32 errors away from zero (the same admission as the ReLU
    inputs of the families), first seed that does; kind: 'random', 'one_anchor' (every triplet shares its anchor: the scatter's
    atomics all land on one row) or 'inactive' (no triplet violates the margin)."""
    for seed in range(200):
        gen = torch.Generator().manual_seed(seed)
        emb = torch.randn(n, D, generator=gen) / D ** 0.5
        ia, ip, in_ = (torch.randint(0, n, (T,), generator=gen) for _ in range(3))
        if kind == "one_anchor":
            ia = torch.full((T,), 7)
        if kind == "inactive":
            ip = ia.clone()                                   # |a - p|^2 = 0, the negative is the node farthest from the anchor
            in_ = torch.cdist(emb[ia], emb).argmax(1)

        def hinge(e):
            return ((e[ia] - e[ip]) ** 2).sum(1) - ((e[ia] - e[in_]) ** 2).sum(1) + 0.1
        h32, h64 = hinge(emb).double(), hinge(emb.double())
        active = int((h64 > 0).sum())
        if (h64.abs().min() >= 100 * (h32 - h64).abs().max() and bool((torch.sign(h32) == torch.sign(h64)).all())
                and (active == 0 if kind == "inactive" else active >= (T + 1) // 2)):
            return emb, ia, ip, in_
    raise AssertionError("no admissible draw")


@pytest.mark.parametrize("kind", ["random", "one_anchor", "inactive"])
@pytest.mark.parametrize("T", [1, 255, 256, 257, 1024])
@pytest.mark.parametrize("D", [4, 36, 64, 800])
def test_triplet_loss_against_float64(D, T, kind):
    from neural_spectral_codec_amd.gnn.trainer import TripletLoss
    emb, ia, ip, in_ = _triplet_case(D, T, kind)
    refs = {}
    for dt in (torch.float32, torch.float64):
        e = emb.clone().to(dt).requires_grad_(True)
        loss = go.triplet_loss_reference(e, ia, ip, in_, 0.1)
        loss.backward()
        refs[dt] = (loss.detach(), e.grad)
    e = emb.cuda().requires_grad_(True)
    loss = TripletLoss(0.1).forward_indexed(e, ia.numpy(), ip.numpy(), in_.numpy())
    loss.backward()
    l64, g64 = refs[torch.float64]
    if kind == "inactive":
        assert l64.item() == 0 and loss.item() == 0.0 and not bool(e.grad.any())
        return
    rel = abs(loss.item() - l64.item()) / l64.item()
    e32, eg = tf.err(refs[torch.float32][1], g64), tf.err(e.grad, g64)
    print(f"RATIO triplet D={D} T={T} {kind}: loss rel {rel:.2e}; gradient e_gpu {eg:.2e} / e32 {e32:.2e} = {eg / e32:.2f}")
    assert rel <= 1e-5
    assert eg <= tf.K_BAR * e32
