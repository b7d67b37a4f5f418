"""SpectralGNN on MI355X -- drop-in for the reference's src/gnn/model.py.

Same classes, constructor arguments, state-dict keys and ``forward(data)`` contract
(model.py:21-205 SpectralGNN, :208-281 LocalUpdateGNN, :284-324 create_spectral_gnn).  The forward
pass is one call into the C ABI (nsc_gat_forward, csrc/nsc_gat.hip): f32-MFMA projection GEMMs with
fused BatchNorm/ReLU/residual epilogues and a wavefront-per-node attention/aggregation kernel.
The module must live on a HIP device; there is no CPU fallback.
"""
import collections
import copy
import ctypes as C
import os
from typing import Optional

import torch
import torch.nn as nn

from .. import _lib
from .gat_conv import GATConv

def _ws(device, nbytes, tag):
    # one scratch buffer per (device, stream, host thread, use), bounded and capture-safe: _lib.ScratchCache (two rank
    # threads building their CSR in one shared scratch faulted the aggregate kernel; an unbounded dict only grew)
    return _lib.scratch.get(device, nbytes, tag)


class GraphCSR:
    """Device CSR-by-target arrays of one graph (built by nsc_graph_build_csr, cached per graph)."""

    def __init__(self, edge_index: torch.Tensor, edge_attr: Optional[torch.Tensor], n_nodes: int):
        dev = edge_index.device
        _lib.require_cuda(edge_index, "data.edge_index")
        L = _lib.lib()
        ei = edge_index.to(torch.int64).contiguous()
        E = int(ei.shape[1])
        self.n_nodes, self.n_edges = n_nodes, E
        self.capacity = E + n_nodes
        self.row_ptr = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
        self.src = torch.empty(self.capacity, dtype=torch.int32, device=dev)
        self.eid = torch.empty(self.capacity, dtype=torch.int32, device=dev)
        self.edge_dim = 0
        self.loop_attr = None
        ea = None
        if edge_attr is not None:
            ea = edge_attr.to(device=dev, dtype=torch.float32).contiguous()
            if ea.dim() == 1:
                ea = ea.unsqueeze(1)
            self.edge_dim = int(ea.shape[1])
            self.loop_attr = torch.empty((n_nodes, self.edge_dim), dtype=torch.float32, device=dev)
        self.edge_attr = ea
        nbytes = L.nsc_graph_workspace_bytes(n_nodes, E)
        ws = _ws(dev, nbytes, "graph")
        _lib.call("nsc_graph_build_csr", dev, ei, E, n_nodes, ea, self.edge_dim, self.row_ptr, self.src, self.eid,
                  self.loop_attr, ws, nbytes, _lib.STREAM)
        self.t_ptr = self.t_entry = self.tgt = None
        # Banded form (nsc_graph_band_entries): the temporal chain of every reference caller has its sources within 2 rows
        # of the target (graph_manager.py:520-532), and such a graph runs a GATConv layer as ONE launch.  Whether THIS graph
        # qualifies is read back once per graph (two int32; the CSR is cached per graph by SpectralGNN._csr).
        self.band, self.band_entries = 0, None
        if n_nodes > 0 and self.edge_dim in (0, 2):
            ent = torch.empty((n_nodes, 8, 4), dtype=torch.float32, device=dev)
            info = torch.empty(2, dtype=torch.int32, device=dev)
            _lib.call("nsc_graph_band_entries", dev, self.struct(), ea, self.edge_dim, ent, info, _lib.STREAM)
            max_off, max_deg = info.tolist()
            if max_off <= 2 and max_deg <= 8:
                self.band, self.band_entries = 2, ent

    def ensure_transpose(self):
        """Entries grouped by source (nsc_graph_transpose); the backward needs it, built once."""
        if self.t_ptr is not None:
            return
        dev = self.row_ptr.device
        L = _lib.lib()
        self.t_ptr = torch.empty(self.n_nodes + 1, dtype=torch.int32, device=dev)
        self.t_entry = torch.empty(self.capacity, dtype=torch.int32, device=dev)
        self.tgt = torch.empty(self.capacity, dtype=torch.int32, device=dev)
        nbytes = L.nsc_graph_transpose_workspace_bytes(self.n_nodes)
        ws = _ws(dev, nbytes, "graph")
        _lib.call("nsc_graph_transpose", dev, self.struct(), self.t_ptr, self.t_entry, self.tgt, ws, nbytes, _lib.STREAM)

    def struct(self) -> _lib.Graph:
        g = _lib.Graph()
        g.n_nodes = self.n_nodes
        g.nnz = self.capacity
        g.row_ptr = self.row_ptr.data_ptr()
        g.src = self.src.data_ptr()
        g.eid = self.eid.data_ptr()
        g.loop_attr = self.loop_attr.data_ptr() if self.loop_attr is not None else None
        if self.t_ptr is not None:
            g.t_ptr, g.t_entry, g.tgt = self.t_ptr.data_ptr(), self.t_entry.data_ptr(), self.tgt.data_ptr()
        if self.band:
            g.band_entries, g.band = self.band_entries.data_ptr(), self.band
        return g


# One row per tensor NscGatModel points at: ``owner[key]`` is the live tensor (the owning module's own ``_parameters`` /
# ``_buffers`` dict), ``field`` its NscGatModel / NscGatLayer member, ``grad`` its NscGatGrads / NscGatGradLayer member (None:
# running statistics, which have no gradient), ``layer`` the index into ``layers[]`` (None: a member of the model itself).
ParamRow = collections.namedtuple("ParamRow", "owner key field grad layer")
# SpectralGNN._struct_cache: the NscGatModel of the eval forward, its folded attention vectors and the tensors of its key
FoldedStruct = collections.namedtuple("FoldedStruct", "key model folded live")
# SpectralGNN.capture_state(): what a captured eval forward over one graph bakes in
CaptureState = collections.namedtuple("CaptureState", "csr folded key")

# Derived state of a SpectralGNN (device pointers, what a capture in progress set): (name, default).  Created by __init__,
# reset by __getstate__, so deepcopy / pickle / torch.save carry none of it.
_PRIVATE = (
    ("_csr_cache", collections.OrderedDict()),   # graph key -> GraphCSR, least recently used first
    ("_struct_cache", None),           # FoldedStruct of the eval forward
    ("_train_struct_cache", None),     # (parameter addresses, NscGatModel) of the training calls
    ("_fold_generation", 0),           # counts the re-folds: a captured forward bakes the folded tensor in
    ("_seed_dev", None),               # device int64[1]: dropout seed the kernels read at run time (captured steps)
    ("_direct_grads", False),          # backward adds straight into the parameters' .grad tensors (GNNTrainer's steps)
    ("_nbt_flat", None),               # the BatchNorm step counters as one vector (_bump_batches_tracked)
)


def unwrap(model):
    """The SpectralGNN inside a LocalUpdateGNN, or ``model`` itself (a SpectralGNN, or any other callable)."""
    return model.gnn if isinstance(model, LocalUpdateGNN) else model


def _train_forward_raw(gnn, x, csr, dropout_p, seed):
    """nsc_gat_forward_train: returns (out, state); state holds the workspace with the saved activations for
    _train_backward_raw.  Used by the autograd Function below and, without autograd, by GNNTrainer's direct step."""
    dev = x.device
    m = gnn._train_struct()
    csr.ensure_transpose()
    g = csr.struct()
    cfg = _lib.GatTrainCfg()
    cfg.dropout_p, cfg.bn_momentum = float(dropout_p), float(gnn.input_norm.momentum or 0.1)
    cfg.seed, cfg.update_running_stats = int(seed), 1
    sd = gnn._seed_dev                            # a device word the kernels read the seed from (captured steps)
    cfg.seed_dev = sd.data_ptr() if sd is not None else None
    n = int(x.shape[0])
    out = torch.empty((n, gnn.output_dim), dtype=torch.float32, device=dev)
    nbytes = _lib.lib().nsc_gat_train_workspace_bytes(C.byref(m), C.byref(g))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)      # holds the saved activations
    if os.environ.get("NSC_DEBUG_WS_NAN") == "1":              # debugging: a read of never-written workspace shows up as NaN
        ws.fill_(0xFF)
    _lib.call("nsc_gat_forward_train", dev, m, g, x, csr.edge_attr, cfg, out, ws, nbytes, _lib.STREAM)
    _bump_batches_tracked(gnn)
    return out, (csr, cfg, ws, nbytes, x, sd)


def _bump_batches_tracked(gnn):
    """``num_batches_tracked += 1`` of every BatchNorm (what torch's own train-mode forward does) as ONE launch: the counters
    are 0-d views of one int64 vector (set up outside a capture, re-made whenever a ``.to()`` / a new buffer broke the aliasing;
    ``load_state_dict`` copies in place and keeps it).  Four 4 us kernels per batch of the captured training step were these."""
    bns = [bn for bn in [gnn.input_norm] + list(gnn.batch_norms) if bn.num_batches_tracked is not None]
    if not bns:
        return
    bufs = [bn.num_batches_tracked for bn in bns]
    flat = gnn._nbt_flat
    ok = (flat is not None and flat.numel() == len(bufs) and flat.device == bufs[0].device
          and all(b_.dtype == flat.dtype and b_.dim() == 0 and b_.device == flat.device
                  and b_.data_ptr() == flat.data_ptr() + i * flat.element_size() for i, b_ in enumerate(bufs)))
    if not ok:
        same = all(b_.dim() == 0 and b_.dtype == bufs[0].dtype and b_.device == bufs[0].device for b_ in bufs)
        if not same or (bufs[0].is_cuda and torch.cuda.is_current_stream_capturing()):
            for b_ in bufs:                                  # unusual buffers, or no allocation wanted inside a capture
                b_ += 1
            return
        flat = torch.stack([b_.detach() for b_ in bufs])
        for i, bn in enumerate(bns):
            bn._buffers["num_batches_tracked"] = flat[i]
        gnn._nbt_flat = flat
    flat += 1


def _train_backward_raw(gnn, state, grad_out, grads, accumulate, need_x):
    """nsc_gat_backward into ``grads`` (tensors in _train_params() order; accumulate: added to what they hold).  Returns the
    gradient w.r.t. x or None."""
    csr, cfg, ws, nbytes, x, _sd = state
    cfg.accumulate_grads = 1 if accumulate else 0
    gs = _lib.GatGrads()
    for row, t in zip(gnn._grad_rows, grads):
        setattr(gs if row.layer is None else gs.layers[row.layer], row.grad, t.data_ptr())
    gx = torch.empty_like(x) if need_x else None
    gs.x = gx.data_ptr() if gx is not None else None
    _lib.call("nsc_gat_backward", x.device, gnn._train_struct(), csr.struct(), x, csr.edge_attr, cfg, grad_out, gs, ws, nbytes,
              _lib.STREAM)
    return gx


def _direct_ok(params) -> bool:
    """The backward may add straight into the .grad tensors of ``params`` (_train_params() order): every one is trained and
    has a contiguous .grad.  A frozen parameter (requires_grad False) takes the autograd path, which drops its gradient."""
    return all(p.requires_grad and p.grad is not None and p.grad.is_contiguous() for p in params)


def _triplet_loss(out, ia, ip, in_, margin, scale, want_grad):
    """nsc_triplet_loss over the rows ``ia`` / ``ip`` / ``in_`` (int64 device vectors) of ``out`` (N, D) contiguous float32:
    returns (loss (1,), d loss / d out or None)."""
    dev = out.device
    n, d, t = int(out.shape[0]), int(out.shape[1]), int(ia.numel())
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    grad = torch.empty_like(out) if want_grad else None
    nbytes = _lib.lib().nsc_triplet_workspace_bytes(t)
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
    _lib.call("nsc_triplet_loss", dev, out, ia, ip, in_, t, n, d, float(margin), float(scale), loss, grad, ws, nbytes,
              _lib.STREAM)
    return loss, grad


class _GatTrainFunction(torch.autograd.Function):
    """model.train(); model(data) with autograd: nsc_gat_forward_train / nsc_gat_backward."""

    @staticmethod
    def forward(ctx, gnn, x, csr, dropout_p, seed, *params):
        out, state = _train_forward_raw(gnn, x, csr, dropout_p, seed)
        ctx.gnn, ctx.state = gnn, state
        ctx.need_x = x.requires_grad
        return out

    @staticmethod
    def backward(ctx, grad_out):
        gnn = ctx.gnn
        params = gnn._train_params()
        # GNNTrainer's steps: the kernels ADD into the existing .grad tensors (NscGatTrainCfg.accumulate_grads) and autograd
        # gets no parameter gradients back -- no AccumulateGrad axpy per parameter (30 small kernels per batch)
        direct = gnn._direct_grads and _direct_ok(params)
        grads = [p.grad for p in params] if direct else [torch.empty_like(p) for p in params]
        go = grad_out.contiguous().float()
        gx = _train_backward_raw(gnn, ctx.state, go, grads, direct, ctx.need_x)
        ctx.state = None
        if direct:
            return (None, gx, None, None, None) + (None,) * len(grads)
        return (None, gx, None, None, None, *grads)


class SpectralGNN(nn.Module):
    """Input(800) -> Proj(256) -> GAT x3 (256) -> Proj(800) -> Output(800)   (model.py:21-94)"""

    def __init__(self, input_dim: int = 800, hidden_dim: int = 256, output_dim: int = 800,
                 n_layers: int = 3, n_heads: int = 1, dropout: float = 0.1, residual: bool = True,
                 edge_dim: int = None):
        super().__init__()
        self.input_dim, self.hidden_dim, self.output_dim = input_dim, hidden_dim, output_dim
        self.n_layers, self.n_heads, self.dropout = n_layers, n_heads, dropout
        self.residual, self.edge_dim = residual, edge_dim
        self.input_proj = nn.Linear(input_dim, hidden_dim)                   # :67
        self.input_norm = nn.BatchNorm1d(hidden_dim)                         # :68
        self.convs = nn.ModuleList()
        self.batch_norms = nn.ModuleList()
        for _ in range(n_layers):                                            # :74-85
            self.convs.append(GATConv(hidden_dim, hidden_dim, heads=n_heads, concat=False,
                                      dropout=dropout, edge_dim=edge_dim))
            self.batch_norms.append(nn.BatchNorm1d(hidden_dim))
        self.output_proj = nn.Linear(hidden_dim, output_dim)                 # :88
        if residual and input_dim != output_dim:                             # :91-94
            self.residual_proj = nn.Linear(input_dim, output_dim)
        else:
            self.residual_proj = None
        # The kernel set of the eval forward (_lib.GAT_KERNEL_SETS).  True: the LDS-free, low-VGPR set (NSC_GAT_CORESIDENT)
        # whose workgroups fit beside a resident encoder grid -- used by distributed.ShardedDescriptorPath(pipeline=True).
        # "shared_b": that set with the small-LDS GEMMs (NSC_GAT_SHARED_B).  "lds_tiled": the stand-alone forward with the
        # register-staged GEMMs (NSC_GAT_LDS_TILED) instead of the LDS-DMA GEMM.  "generic": the stand-alone forward
        # without the one-launch layers of a banded graph (NSC_GAT_GENERIC).  Same output, bit for bit.
        self.coresident = False
        for name, default in _PRIVATE:
            setattr(self, name, copy.copy(default))
        self._set_table()

    # -- plumbing ---------------------------------------------------------------------------
    def __getstate__(self):
        # device-pointer caches are rebuilt on demand; keep them out of deepcopy / pickle / torch.save
        state = self.__dict__.copy()
        for name, default in _PRIVATE:
            state[name] = copy.copy(default)
        for name in ("_table", "_grad_rows", "_slots"):
            del state[name]
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        for name, default in _PRIVATE:     # (a module pickled before one of them existed)
            self.__dict__.setdefault(name, copy.copy(default))
        self._set_table()                  # over the copy's own parameter dicts

    def _set_table(self):
        """The parameter table (ParamRow), in the order NscGatGrads lists its members; an optional piece (residual_proj,
        lin_edge / att_edge) has its rows or has none.  Built once: the module tree is fixed after __init__."""
        def linear(mod, w, b):
            return [(mod._parameters, "weight", w, w), (mod._parameters, "bias", b, b)]

        def norm(bn, pre):
            return [(bn._parameters, "weight", pre + "w", pre + "w"), (bn._parameters, "bias", pre + "b", pre + "b"),
                    (bn._buffers, "running_mean", pre + "mean", None), (bn._buffers, "running_var", pre + "var", None)]

        rows = [ParamRow(*r, None) for r in linear(self.input_proj, "in_w", "in_b") + norm(self.input_norm, "in_bn_")
                + linear(self.output_proj, "out_w", "out_b")
                + (linear(self.residual_proj, "res_w", "res_b") if self.residual_proj is not None else [])]
        for l, (conv, bn) in enumerate(zip(self.convs, self.batch_norms)):
            cp = conv._parameters
            edge = [] if conv.lin_edge is None else [(conv.lin_edge._parameters, "weight", "lin_edge_w", "lin_edge_w"),
                                                     (cp, "att_edge", "att_edge", "att_edge")]
            rows += [ParamRow(*r, l) for r in [(conv.lin_src._parameters, "weight", "lin_w", "lin_w"),
                                               (cp, "att_src", "att_src", "att_src"), (cp, "att_dst", "att_dst", "att_dst")]
                     + edge + [(cp, "bias", "bias", "bias")] + norm(bn, "bn_")]
        self._table = tuple(rows)
        self._grad_rows = tuple(r for r in rows if r.grad is not None)
        self._slots = tuple((r.owner, r.key) for r in rows)      # what the per-step path walks

    def _csr(self, data, use_edge_attr: bool) -> GraphCSR:
        ei = data.edge_index
        ea = getattr(data, "edge_attr", None) if use_edge_attr else None
        n = int(data.x.shape[0])
        key = (ei.data_ptr(), ei._version, tuple(ei.shape), n,
               None if ea is None else (ea.data_ptr(), ea._version, tuple(ea.shape)))
        cache = self._csr_cache
        csr = cache.get(key)
        if csr is None:
            while len(cache) >= 8:
                cache.popitem(last=False)    # least recently used graph
            csr = GraphCSR(ei, ea, n)
            csr._keepalive = (ei, ea)        # pointers in the key stay valid while cached
            cache[key] = csr
        else:
            cache.move_to_end(key)
        return csr

    def _uses_edge_attr(self, data) -> bool:
        return getattr(data, "edge_attr", None) is not None and self.edge_dim is not None       # model.py:126

    def _live_tensors(self):
        """Every tensor NscGatModel points into, in table order.  Looked up through the modules' own ``_parameters`` /
        ``_buffers`` dicts: always the current tensor, without nn.Module.__getattr__ -- 113 attribute walks per call were a
        third of the host time of a pipelined step (nn.Module.parameters() / buffers() before that: 40 %; DESIGN.md section
        7, experiment 50)."""
        return [d[n] for d, n in self._slots]

    def _model_struct(self, live=None, versions=None) -> _lib.GatModel:
        """NscGatModel over the live parameter storage.  Rebuilt (and the attention vectors re-folded
        by nsc_gat_fold_weights) only when a parameter was modified or moved, or an optimizer stepped (_lib.param_epoch: fused
        optimizers do not bump version counters).  ``live``: the caller's _live_tensors(); ``versions``: its
        (data_ptr, _version) tuple over them, when it has built one."""
        if live is None:
            live = self._live_tensors()
        if versions is None:
            versions = tuple((t.data_ptr(), t._version) for t in live)
        key = (_lib.param_epoch, versions)
        if self._struct_cache is not None and self._struct_cache.key == key:
            return self._struct_cache.model
        m = self._build_struct(live)
        dev = live[0].device
        folded = torch.empty(int(_lib.lib().nsc_gat_folded_floats(C.byref(m))), dtype=torch.float32, device=dev)
        m.folded = folded.data_ptr()
        _lib.call("nsc_gat_fold_weights", dev, m, folded, _lib.STREAM)
        # the entry holds the tensors of its key: a replaced parameter cannot be freed and its address handed to the
        # replacement (same address, version 0 again) while the cache still describes it
        self._struct_cache = FoldedStruct(key, m, folded, live)
        self._fold_generation += 1         # a captured forward bakes `folded` in: part of capture_state()'s key
        return m

    def capture_state(self, data) -> CaptureState:
        """What a captured eval forward over ``data`` bakes in besides ``data.x``: the graph's GraphCSR, the folded
        attention vectors of the current weights (made now if need be), and a hashable key that changes whenever a replay
        would no longer compute ``self(data)``: parameter addresses and versions, the fold generation (an optimizer that
        writes through a multi-tensor kernel bumps no version counter, but every optimizer step bumps _lib.param_epoch and
        so forces a new fold), the kernel set and the identity of the GraphCSR.  Keep ``csr`` and ``folded`` alive as long
        as the capture: a replay reads them, and the key holds the GraphCSR's id."""
        live = self._live_tensors()
        versions = tuple((t.data_ptr(), t._version) for t in live)
        self._model_struct(live, versions)
        csr = self._csr(data, self._uses_edge_attr(data))
        return CaptureState(csr, self._struct_cache.folded, (versions, self._fold_generation, self.coresident, id(csr)))

    def _train_struct(self) -> _lib.GatModel:
        """NscGatModel for nsc_gat_forward_train / nsc_gat_backward: pointers into the live parameter storage, no folded
        attention vectors (the training kernels compute the attention dot products themselves, so an optimizer step
        does not force a re-fold before the next forward).  Rebuilt only when a parameter's storage moves."""
        live = self._live_tensors()
        key = tuple(t.data_ptr() for t in live)
        c = self._train_struct_cache
        if c is None or c[0] != key:
            c = self._train_struct_cache = (key, self._build_struct(live))
        return c[1]

    def _build_struct(self, live) -> _lib.GatModel:
        m = _lib.GatModel()
        m.in_dim, m.hidden, m.out_dim = self.input_dim, self.hidden_dim, self.output_dim
        m.n_layers = self.n_layers
        m.edge_dim = self.edge_dim or 0
        m.residual = int(bool(self.residual))
        m.bn_eps = float(self.input_norm.eps)
        m.negative_slope = float(self.convs[0].negative_slope)
        for row, t in zip(self._table, live):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise _lib.NscError("GNN parameters must be contiguous float32 tensors on the HIP device")
            setattr(m if row.layer is None else m.layers[row.layer], row.field, t.data_ptr())
        return m

    def _train_params(self):
        """Parameters in the order NscGatGrads lists them."""
        return [r.owner[r.key] for r in self._grad_rows]

    def _dropout_seed(self) -> int:
        """Seed of the counter-based dropout masks: one draw from torch's CPU generator per training forward with dropout;
        none when a captured step (GNNTrainer) keeps the seed in a device word (self._seed_dev), rewritten before every
        replay."""
        return int(torch.randint(0, 2 ** 62, (1,)).item()) if (self.dropout > 0 and self._seed_dev is None) else 0

    def _run_train(self, data, use_edge_attr: bool):
        """model.train() forward with autograd (trainer.py:205): batch-statistics BatchNorm, feature and
        attention dropout (counter-based masks seeded from torch's CPU generator)."""
        x = data.x
        _lib.require_cuda(x, "data.x")
        x = x.to(torch.float32).contiguous()
        csr = self._csr(data, use_edge_attr)
        return _GatTrainFunction.apply(self, x, csr, float(self.dropout), self._dropout_seed(), *self._train_params())

    def train_step_direct(self, data, anchor_idx, positive_idx, negative_idx, margin: float, scale: float):
        """forward (train mode) + TripletLoss + backward WITHOUT autograd (GNNTrainer's steps): nsc_gat_forward_train,
        nsc_triplet_loss (which returns d loss / d emb) and nsc_gat_backward adding into the parameters' existing .grad
        tensors -- what ``loss = criterion(model(graph)[a], ...); loss.backward()`` (trainer.py:205-213) computes, minus the
        autograd plumbing around the three ABI calls (a (N, 800) multiply by the upstream scalar, two dtype / layout copies and
        the engine's bookkeeping per batch).  Indices: int64 device tensors.  Returns the loss (0-d tensor)."""
        x = data.x
        _lib.require_cuda(x, "data.x")
        x = x.detach().to(torch.float32).contiguous()
        csr = self._csr(data, self._uses_edge_attr(data))
        params = self._train_params()
        if not _direct_ok(params):
            raise _lib.NscError("train_step_direct adds into the existing contiguous .grad tensors of trained parameters")
        out, state = _train_forward_raw(self, x, csr, float(self.dropout), self._dropout_seed())
        loss, grad = _triplet_loss(out, anchor_idx, positive_idx, negative_idx, margin, scale, True)
        _train_backward_raw(self, state, grad, [p.grad for p in params], True, False)
        return loss[0]

    def _run(self, data, use_edge_attr: bool, want_alpha: bool):
        x = data.x
        _lib.require_cuda(x, "data.x")
        if self.input_proj.weight.device != x.device:
            raise _lib.NscError("SpectralGNN and data must be on the same HIP device")
        if self.training:
            raise _lib.NscError("forward_with_attention is an inference helper: call model.eval() first")
        dev = x.device
        x = x.detach().to(torch.float32).contiguous()
        n = int(x.shape[0])
        csr = self._csr(data, use_edge_attr)
        m = self._model_struct()
        out = torch.empty((n, self.output_dim), dtype=torch.float32, device=dev)
        alpha = (torch.zeros((self.n_layers, csr.capacity), dtype=torch.float32, device=dev)
                 if want_alpha else None)
        nbytes = _lib.lib().nsc_gat_workspace_bytes(C.byref(m), n)
        ws = _ws(dev, nbytes, "gat")
        _lib.call("nsc_gat_forward_ex", dev, m, csr.struct(), x, csr.edge_attr, out, alpha, ws, nbytes,
                  _lib.GAT_KERNEL_SETS[self.coresident], _lib.STREAM)
        return out, alpha, csr

    # -- reference API ----------------------------------------------------------------------
    def forward(self, data) -> torch.Tensor:
        """model.py:96-153: data.x (N,in), data.edge_index (2,E), optional data.edge_attr (E,edge_dim)."""
        use_edge = self._uses_edge_attr(data)
        if self.training:
            return self._run_train(data, use_edge)
        out, _, _ = self._run(data, use_edge, False)
        return out

    def forward_with_attention(self, data) -> tuple:
        """model.py:155-201: convs are called WITHOUT edge_attr there; returns
        (embeddings, [(edge_index_with_self_loops (2,E'), alpha (E',1))] * n_layers) in PyG's
        order (kept edges in input order, then the N self loops)."""
        out, alpha, csr = self._run(data, False, True)
        nnz = int(csr.row_ptr[-1].item())
        eid = csr.eid[:nnz].long()
        ei = data.edge_index
        keep = ei[0] != ei[1]
        rank = torch.cumsum(keep.long(), 0) - 1                              # position among kept edges
        n_kept = int(keep.sum().item())
        tgt = torch.repeat_interleave(torch.arange(csr.n_nodes, device=ei.device),
                                      (csr.row_ptr[1:] - csr.row_ptr[:-1]).long())
        rank = torch.cat([rank, rank.new_zeros(1)])                         # a graph without edges: every entry is a loop (eid -1)
        pos = torch.where(eid >= 0, rank[eid.clamp(min=0)], n_kept + tgt)
        loops = torch.arange(csr.n_nodes, device=ei.device)
        ei_full = torch.cat([ei[:, keep], torch.stack([loops, loops])], 1)
        weights = []
        for l in range(self.n_layers):
            a = torch.empty(nnz, dtype=torch.float32, device=ei.device)
            a[pos] = alpha[l, :nnz]
            weights.append((ei_full, a.unsqueeze(1)))
        return out, weights

    def get_embedding_dim(self) -> int:
        return self.output_dim


class LocalUpdateGNN(nn.Module):
    """model.py:208-281: wrapper whose local update is a stub in the reference -- always full graph."""

    def __init__(self, gnn: SpectralGNN, k_hops: int = 3):
        super().__init__()
        self.gnn = gnn
        self.k_hops = k_hops

    def forward(self, data, update_nodes: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self.gnn(data)                                                # :248-255

    def forward_local(self, data, center_node: int, k_hops: Optional[int] = None) -> torch.Tensor:
        embeddings = self.gnn(data)                                          # :277-281
        return embeddings[center_node:center_node + 1]


def create_spectral_gnn(input_dim: int = 800, hidden_dim: int = 256, output_dim: int = 800,
                        n_layers: int = 3, dropout: float = 0.1, use_local_updates: bool = True,
                        local_update_hops: int = 3, edge_dim: int = None) -> nn.Module:
    """model.py:284-324"""
    base_gnn = SpectralGNN(input_dim=input_dim, hidden_dim=hidden_dim, output_dim=output_dim,
                           n_layers=n_layers, n_heads=1, dropout=dropout, residual=True,
                           edge_dim=edge_dim)
    if use_local_updates:
        return LocalUpdateGNN(base_gnn, k_hops=local_update_hops)
    return base_gnn
