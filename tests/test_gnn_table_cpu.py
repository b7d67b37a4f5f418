"""SpectralGNN's parameter table (gnn/model.py): the one list behind NscGatModel, NscGatGrads, _live_tensors() and
_train_params(); what copies of a model carry; the kernel-set codes; _lib.call's argument conversion.  Host code only:
nothing here touches a device."""
import copy
import ctypes as C
import io
import pickle

import pytest
import torch

from neural_spectral_codec_amd import _lib
from neural_spectral_codec_amd.gnn.model import _PRIVATE, LocalUpdateGNN, SpectralGNN, unwrap


def _pointer_fields(struct):
    return [n for n, t in struct._fields_ if t is C.c_void_p]


def _model(**kw):
    torch.manual_seed(0)
    args = dict(input_dim=48, hidden_dim=16, output_dim=32, n_layers=3, edge_dim=2)
    args.update(kw)
    return SpectralGNN(**args)


def test_table_names_every_pointer_field_once_with_every_option_on():
    g = _model(n_layers=8)                                       # edge_dim=2, input_dim != output_dim: residual_proj exists
    assert g.residual_proj is not None and g.convs[0].lin_edge is not None
    model_fields = [(r.layer, r.field) for r in g._table]
    want = [(None, f) for f in _pointer_fields(_lib.GatModel) if f != "folded"] + [
        (l, f) for l in range(8) for f in _pointer_fields(_lib.GatLayer)]
    assert len(set(model_fields)) == len(model_fields), "a model field appears twice"
    assert sorted(model_fields, key=str) == sorted(want, key=str)
    grad_fields = [(r.layer, r.grad) for r in g._table if r.grad is not None]
    want = [(None, f) for f in _pointer_fields(_lib.GatGrads) if f != "x"] + [
        (l, f) for l in range(8) for f in _pointer_fields(_lib.GatGradLayer)]
    assert len(set(grad_fields)) == len(grad_fields), "a gradient field appears twice"
    assert sorted(grad_fields, key=str) == sorted(want, key=str)
    # every row is a live tensor of the module, none twice, and all of the module's float tensors are there
    live = g._live_tensors()
    assert len({id(t) for t in live}) == len(live) == len(g._table)
    named = dict(g.named_parameters())
    named.update({k: v for k, v in g.named_buffers() if not k.endswith("num_batches_tracked")})
    assert {id(t) for t in live} == {id(t) for t in named.values()}


OPTIONS_OFF = {
    "no_edge": (dict(edge_dim=None), {"lin_edge_w", "att_edge"}),
    "no_residual_proj": (dict(input_dim=32, output_dim=32), {"res_w", "res_b"}),
    "one_layer": (dict(n_layers=1), set()),
}


@pytest.mark.parametrize("name", sorted(OPTIONS_OFF))
def test_table_with_one_option_off(name):
    kw, absent = OPTIONS_OFF[name]
    g = _model(**kw)
    n_layers = g.n_layers
    want_model = [(None, f) for f in _pointer_fields(_lib.GatModel) if f != "folded" and f not in absent] + [
        (l, f) for l in range(n_layers) for f in _pointer_fields(_lib.GatLayer) if f not in absent]
    assert sorted(((r.layer, r.field) for r in g._table), key=str) == sorted(want_model, key=str)
    want_grad = [(None, f) for f in _pointer_fields(_lib.GatGrads) if f != "x" and f not in absent] + [
        (l, f) for l in range(n_layers) for f in _pointer_fields(_lib.GatGradLayer) if f not in absent]
    assert sorted(((r.layer, r.grad) for r in g._table if r.grad is not None), key=str) == sorted(want_grad, key=str)
    # _train_params(): the order of struct NscGatGrads / NscGatGradLayer in include/nsc.h, written out --
    # in_w in_b in_bn_w in_bn_b out_w out_b (x) res_w res_b, then per layer lin_w att_src att_dst lin_edge_w att_edge bias
    # bn_w bn_b
    want = [g.input_proj.weight, g.input_proj.bias, g.input_norm.weight, g.input_norm.bias, g.output_proj.weight,
            g.output_proj.bias]
    if name != "no_residual_proj":
        want += [g.residual_proj.weight, g.residual_proj.bias]
    for conv, bn in zip(g.convs, g.batch_norms):
        want += [conv.lin_src.weight, conv.att_src, conv.att_dst]
        if name != "no_edge":
            want += [conv.lin_edge.weight, conv.att_edge]
        want += [conv.bias, bn.weight, bn.bias]
    got = g._train_params()
    assert len(got) == len(want) and all(a is b for a, b in zip(got, want))
    assert [(r.layer, r.grad) for r in g._grad_rows] == [(r.layer, r.grad) for r in g._table if r.grad is not None]


def test_table_follows_a_replaced_parameter():
    """The rows name the owning dict and key, not the tensor: a parameter assigned anew is the one the table gives."""
    g = _model()
    new = torch.nn.Parameter(torch.zeros_like(g.convs[1].att_src))
    g.convs[1].att_src = new
    assert any(t is new for t in g._live_tensors()) and any(t is new for t in g._train_params())


@pytest.mark.parametrize("how", ["deepcopy", "pickle", "torch.save"])
def test_copies_start_with_private_state_at_its_defaults(how):
    m = LocalUpdateGNN(_model())
    g = m.gnn
    assert unwrap(m) is g and unwrap(g) is g
    fn = lambda data: None                                        # noqa: E731 -- a plain callable is its own "inner"
    assert unwrap(fn) is fn
    g.coresident = "shared_b"
    marker = torch.zeros(1)
    g._csr_cache["a graph"] = marker
    g._struct_cache, g._train_struct_cache = ("key", marker), ("key", marker)
    g._fold_generation, g._seed_dev, g._direct_grads, g._nbt_flat = 5, marker, True, marker
    assert {n for n, _ in _PRIVATE} >= {"_csr_cache", "_struct_cache", "_train_struct_cache", "_fold_generation",
                                        "_seed_dev", "_direct_grads", "_nbt_flat"}
    assert {k for k in g.__dict__ if k.startswith("_") and k not in torch.nn.Module().__dict__} == (
        {n for n, _ in _PRIVATE} | {"_table", "_grad_rows", "_slots"}), "a private attribute outside the list of defaults"
    if how == "deepcopy":
        m2 = copy.deepcopy(m)
    elif how == "pickle":
        m2 = pickle.loads(pickle.dumps(m))
    else:
        f = io.BytesIO()
        torch.save(m, f)
        f.seek(0)
        m2 = torch.load(f, weights_only=False)
    g2 = m2.gnn
    assert g2.coresident == "shared_b"                            # a setting, not a cache: it travels
    for name, default in _PRIVATE:
        got = getattr(g2, name)
        assert type(got) is type(default) and got == default, name
    assert g2._csr_cache is not g._csr_cache and len(g._csr_cache) == 1 and g._seed_dev is marker   # the original keeps its own
    # the copy's table is over the copy's own tensors
    assert all(a is not b and torch.equal(a, b) for a, b in zip(g2._live_tensors(), g._live_tensors()))
    assert all(a is b for a, b in zip(g2._train_params(), [g2.input_proj.weight, g2.input_proj.bias]))
    assert [(r.key, r.field, r.grad, r.layer) for r in g2._table] == [(r.key, r.field, r.grad, r.layer) for r in g._table]


def test_kernel_sets_are_the_header_flags():
    """_lib.GAT_KERNEL_SETS against the NSC_GAT_* defines of include/nsc.h; ``coresident`` accepts exactly these five."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    flags = {k: int(v) for k, v in re.findall(r"#define NSC_GAT_(CORESIDENT|SHARED_B|LDS_TILED|GENERIC) (\d+)u",
                                              open(os.path.join(root, "include", "nsc.h")).read())}
    assert _lib.GAT_KERNEL_SETS == {False: 0, True: flags["CORESIDENT"], "shared_b": flags["CORESIDENT"] | flags["SHARED_B"],
                                    "lds_tiled": flags["LDS_TILED"], "generic": flags["GENERIC"]}


def test_call_converts_arguments_and_names_the_function_in_its_error(monkeypatch):
    """_lib.call: tensors -> pointers, None -> null, structures by reference, STREAM -> the device's current stream where
    it stands (not always last), everything else untouched; a non-zero status raises with the function's name."""
    import contextlib
    seen = {}

    class FakeLib:
        @staticmethod
        def nsc_fake(*args):
            seen["args"] = args
            return seen.get("status", 0)

    lib = _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: FakeLib)
    monkeypatch.setattr(_lib, "stream_ptr", lambda device: ("stream of", device))
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    t = torch.arange(6, dtype=torch.float32)
    params = _lib.MapRobustParams(kernel=1, neighbours=7, scale=2.0)
    assert _lib.call("nsc_fake", "dev", t, None, 3, 0.5, params, _lib.STREAM, t[2:], 7) is None
    a = seen["args"]
    assert isinstance(a[0], C.c_void_p) and a[0].value == t.data_ptr() and a[6].value == t.data_ptr() + 8
    assert a[1] is None and a[2] == 3 and a[3] == 0.5 and a[5] == ("stream of", "dev") and a[7] == 7
    assert C.cast(a[4], C.POINTER(_lib.MapRobustParams)).contents.neighbours == 7
    seen["status"] = -2
    monkeypatch.setattr(_lib, "lib", lambda: type("L", (), {"nsc_fake": FakeLib.nsc_fake,
                                                           "nsc_status_string": lib.nsc_status_string}))
    with pytest.raises(_lib.NscError, match=r"^nsc_fake failed: .+ \(status -2\)$"):
        _lib.call("nsc_fake", "dev", t, _lib.STREAM)
