"""The claims of tests/train_families.py, checked without a GPU: every family reaches the dispatch row it is there for, the numpy
restatement of the dropout masks is what hash3 / keep_scale compute, every family is admissible (no ReLU or leaky-ReLU kink within
100 float32 errors of a value, enough rows for batch statistics, a float32 floor that leaves the bar meaningful), and the bar the
GPU tests hold the kernels to is fine enough to see ONE lost row of a weight gradient."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gat_oracle as go
import train_families as tf

NAMES = list(tf.FAMILIES)


def test_every_family_has_a_claim():
    assert set(tf.CLAIMS) == set(tf.FAMILIES)
    assert tf.K.MAX_EDGE_DIM == 8 and tf.K.LANE_DEG == 64            # what the edge-8 and the degree families sit on


@pytest.mark.parametrize("name", NAMES)
def test_path_claims(name):
    assert tf.row_str(tf.family_paths(name)) == tf.CLAIMS[name]


def test_degree_families_sit_on_the_boundaries():
    """The hub graph: targets with exactly 63, 64, 65, 128 and 129 entries (own loop included), sources with exactly 64 and 65,
    duplicate edges and explicit self loops in the edge list"""
    for n in (130, 200, 577):
        ei = tf.hub_graph(n).numpy()
        din, dout = tf.degrees(ei, n)
        assert [int(din[10 * k + 10]) for k in range(5)] == [63, 64, 65, 128, 129]
        assert [int(dout[55]), int(dout[57])] == [64, 65]
        assert (ei[0] == ei[1]).sum() == len(range(0, n, 9))
        assert len({(a, b) for a, b in ei.T.tolist()}) < ei.shape[1]                  # duplicates


def test_pick_tile_is_the_librarys():
    """The max_bc = 2 form of the restated cost function against nsc_gat_gemm_tile (the launcher's own choice)"""
    from neural_spectral_codec_amd import build, _lib
    build.build_hip()
    lib = _lib.lib()
    for M in (1, 17, 130, 159, 161, 319, 321, 577, 639, 641, 959, 961, 1119, 1121, 4097, 4161, 4541):
        for N, Kd in ((64, 64), (64, 1600), (1600, 64), (896, 896), (132, 896), (800, 256), (256, 800), (20, 64), (1024, 64)):
            r, c, l, w = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
            assert lib.nsc_gat_gemm_tile(M, N, Kd, C.byref(r), C.byref(c), C.byref(l), C.byref(w)) == 0
            a, bc = tf.pick_tile(M, N, Kd)
            assert (r.value, c.value) == (16 * a, 64 * bc), (M, N, Kd)


def test_coverage_of_the_family_list():
    assert tf.coverage_gaps() == []


# ---- the mask restatement -------------------------------------------------------------------------------------------------
def test_hash_vector_form_equals_scalar_form():
    rng = np.random.default_rng(0)
    for seed in (0, 1, 2 ** 62 - 1, int(rng.integers(0, 2 ** 62))):
        for stream in (100, 102, 200, 207):
            idx = np.concatenate([np.arange(70), rng.integers(0, 2 ** 40, 200), [2 ** 32 - 1, 2 ** 32, 2 ** 63]]).astype(np.uint64)
            got = tf.hash3(seed, stream, idx)
            assert got.dtype == np.uint64 and int(got.max()) < 2 ** 24
            assert [int(v) for v in got] == [tf.hash3_scalar(seed, stream, int(i)) for i in idx]


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_keep_fraction(p):
    n = 10 ** 6
    ks = tf.keep_scale(12345, 201, np.arange(n), p)
    kept = ks > 0
    assert abs(kept.mean() - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n)
    assert ks.dtype == np.float32 and set(np.unique(ks)) == {np.float32(0), np.float32(1) / (np.float32(1) - np.float32(p))}
    # keep iff float32(bits) 2^-24 >= float32(p), on the scalar form
    for i in (0, 1, 17, 99999):
        assert bool(kept[i]) == (np.float32(tf.hash3_scalar(12345, 201, i)) * np.float32(2.0 ** -24) >= np.float32(p))


def test_attention_mask_order_is_the_oracles_csr():
    """csr_entries (the order the attention mask is indexed in) against the oracle's graph builder restatement, on a graph with
    duplicate edges, explicit self loops and an edge list in random order"""
    n = 200
    ei = tf.hub_graph(n)
    row_ptr, src, eid = tf.csr_entries(ei.numpy(), n)
    perm, rp = go.csr_order(ei, n)
    ei_loops = go.add_self_loops_mean(ei, None, n)[0]
    assert np.array_equal(row_ptr, rp.numpy())
    assert np.array_equal(src, ei_loops[0][perm].numpy())
    kept = np.flatnonzero((ei[0] != ei[1]).numpy())
    want_eid = np.concatenate([kept, np.full(n, -1)])[perm.numpy()]
    assert np.array_equal(eid, want_eid)
    for i in (0, 10, 20, 199):                                   # own loop last, edge-list order before it
        e = eid[row_ptr[i]:row_ptr[i + 1]]
        assert e[-1] == -1 and src[row_ptr[i + 1] - 1] == i and np.all(np.diff(e[:-1]) > 0)
    # out-of-range endpoints are dropped, as nsc_graph_build_csr documents
    bad = np.concatenate([ei.numpy(), np.array([[n, 3, -1], [3, n + 5, 4]])], 1)
    rp2, src2, eid2 = tf.csr_entries(bad, n)
    assert np.array_equal(rp2, row_ptr) and np.array_equal(src2, src) and np.array_equal(eid2, eid)


def test_masks_differ_between_seeds_and_are_applied():
    """Two seeds give different masks; the restatement with masks differs from the one without, and the taps are bitwise inert"""
    a, b = tf.seed_of(1), tf.seed_of(2)
    assert a != b and tf.seed_of(1) == a
    ei = tf.hub_graph(130).numpy()
    ma, mb = tf.dropout_masks(a, 0.3, 130, 64, 3, ei), tf.dropout_masks(b, 0.3, 130, 64, 3, ei)
    assert len(ma["att"]) == 3 and len(ma["feat"]) == 2
    for x, y in zip(ma["att"] + ma["feat"], mb["att"] + mb["feat"]):
        assert not torch.equal(x, y)
    assert not torch.equal(ma["att"][0], ma["att"][1]) and not torch.equal(ma["feat"][0], ma["feat"][1])   # a stream per layer
    fam = tf.family("dropout-0.5-64-130-hub")
    plain = go.forward_reference(fam.model, fam.graph, training=True)
    tapped = go.forward_reference(fam.model, fam.graph, training=True, taps={})
    masked = go.forward_reference(fam.model, fam.graph, training=True, masks=fam.masks)
    assert torch.equal(plain, tapped) and not torch.equal(plain, masked)


# ---- admission and power ----------------------------------------------------------------------------------------------------
PRODUCTS = {"w_out": ("out", lambda L: f"h{L}", "output_proj.weight"), "w_res": ("out", None, "residual_proj.weight"),
            "w_in": ("z0", None, "input_proj.weight")}


@functools.lru_cache(maxsize=2)
def _evaluate(name):
    fam = tf.family(name)
    t32, t64 = {}, {}
    return fam, tf.reference(fam, torch.float32, t32), tf.reference(fam, torch.float64, t64), t32, t64


def defects(fam, r64, t64):
    """{(product, row): ||dY[row]|| ||X[row]|| / ||dW||_F}: what a weight gradient loses, relative, with ONE node's term dropped"""
    n, L = fam.graph.num_nodes, fam.spec["L"]
    x = fam.graph.x.double()
    out = {}
    for prod, rows in tf.tail_rows(fam.paths, n).items():
        if prod == "w_lin":
            jobs = [(t64[f"l{l}.G"].grad, t64[f"h{l}"].detach(), f"convs.{l}.lin_src.weight") for l in range(L)]
        else:
            dy, xk, key = PRODUCTS[prod]
            jobs = [(t64[dy].grad, t64[xk(L)].detach() if xk else x, key)]
        for dY, X, key in jobs:
            for r in rows:
                out[(key, r)] = (dY[r].norm() * X[r].norm() / r64["grad " + key].norm()).item()
    return out


@pytest.mark.parametrize("name", NAMES)
def test_admission_and_power(name):
    fam, r32, r64, t32, t64 = _evaluate(name)
    # the placement stayed inside its stated limits: biases moved by at most 0.25, attention vectors scaled within [0.75, 1.5]
    assert len(fam.placed["bias_shift"]) == fam.spec["L"] and len(fam.placed["att_scale"]) == 2 * fam.spec["L"]
    assert max(fam.placed["bias_shift"]) <= 0.25 and all(0.75 <= t <= 1.5 for t in fam.placed["att_scale"])
    # (b) enough rows for batch statistics
    assert fam.graph.num_nodes >= 17
    # (a) no kink within 100 float32 errors of a ReLU input or a pre-leaky-ReLU logit (with the masks applied)
    for k, (same_sign, ratio) in tf.admission(fam, t32, t64).items():
        assert same_sign and ratio >= 100, (k, same_sign, ratio)
    # (c) the float32 floor
    e32, rows32 = tf.figures(r32, r64)
    assert max(e32.values()) <= 5e-5, max(e32, key=e32.get)
    # every gradient the bar is applied to is a gradient: not a zero that only holds rounding noise
    gscale = max(v.norm().item() for k, v in r64.items() if k.startswith("grad ") and k != "grad x")
    for k in e32:
        if k.startswith("grad ") and k != "grad x":
            assert r64[k].norm().item() > 1e-6 * gscale, k
    if fam.spec["graph"] == "hub":
        assert int(fam.in_degrees.max()) == 129 and int(fam.out_degrees.max()) == 65
    # power: in a K-tail family, one lost row of any split-K weight gradient stands 10 x above the bar
    if fam.spec["dagger"]:
        bar = tf.K_BAR * max(e32.values())
        d = defects(fam, r64, t64)
        assert d and min(d.values()) >= 10 * bar, (min(d, key=d.get), min(d.values()) / bar)
