"""The workspace contract of include/nsc.h, checked from outside the library ("Workspaces").

Every entry point that takes ``(void *ws, size_t ws_bytes)`` promises three things: the workspace need not be initialised,
the call touches at most ``nsc_*_workspace_bytes()`` bytes of it, and nothing but documented state survives in it between
calls.  ``WorkspaceProxy`` stands in front of the loaded library (``_lib._lib``, which every wrapper fetches per call through
``_lib.lib()``) and, for each such call, swaps the caller's workspace for one of its own: exactly the promised size, filled
with a pattern, between two guard blocks.  A region that is read before the call writes it then shows as a result that
changes with the pattern; a region indexed past its end shows as a damaged guard.

Plain Python: importing this module needs neither a GPU nor the built library.  tests/test_workspace_contract_cpu.py
checks the proxy itself and the two tables below against ``_lib.SYMBOLS``; tests/test_workspace_contract_gpu.py runs the
scenarios COVERED names."""
import ctypes as C

import torch

from neural_spectral_codec_amd import _lib

GUARD = 4096                  # bytes in front of and behind every workspace handed out: a multiple of 256, so the
GUARD_BYTE = 0xC3             # workspace keeps the alignment Carver assumes (torch allocations start on 256 at least)
PATTERNS = (0x00, 0xFF, 0x3C)   # zeros; NaN, -1, ~0 and every flag set; small finite floats and integers near 10^9


def wrapped_symbols(symbols=None):
    """the entry points with a workspace: those whose argtypes hold a c_size_t (ws_bytes; the argument before it is ws)
    -> {name: index of ws}"""
    symbols = _lib.SYMBOLS if symbols is None else symbols
    return {name: args.index(C.c_size_t) - 1 for name, (_, args) in symbols.items() if C.c_size_t in args}


def _obj(a):
    """the struct behind a byref(), a pointer or the struct itself"""
    if hasattr(a, "_obj"):
        return a._obj
    return a.contents if hasattr(a, "contents") else a


# The bytes the contract promises, one line per entry point, from include/nsc.h: (L, args) -> nsc_*_workspace_bytes(...)
NEED = {
    "nsc_encode_clouds": lambda L, a: L.nsc_encode_clouds_workspace_bytes(a[2], a[3], a[5]),
    "nsc_graph_build_csr": lambda L, a: L.nsc_graph_workspace_bytes(a[2], a[1]),
    "nsc_gat_forward": lambda L, a: L.nsc_gat_workspace_bytes(a[0], _obj(a[1]).n_nodes),
    "nsc_gat_forward_ex": lambda L, a: L.nsc_gat_workspace_bytes(a[0], _obj(a[1]).n_nodes),
    "nsc_graph_transpose": lambda L, a: L.nsc_graph_transpose_workspace_bytes(_obj(a[0]).n_nodes),
    "nsc_gat_forward_train": lambda L, a: L.nsc_gat_train_workspace_bytes(a[0], a[1]),
    "nsc_gat_backward": lambda L, a: L.nsc_gat_train_workspace_bytes(a[0], a[1]),
    "nsc_triplet_loss": lambda L, a: L.nsc_triplet_workspace_bytes(a[4]),
    "nsc_mine_triplets_ws": lambda L, a: L.nsc_mine_workspace_bytes(a[2], _obj(a[4]).strategy),
    "nsc_topk_smallest": lambda L, a: L.nsc_topk_workspace_bytes(a[1], a[2], a[3]),
    "nsc_voxel_overlap": lambda L, a: L.nsc_voxel_overlap_workspace_bytes(a[5], a[6]),
    "nsc_gicp_register": lambda L, a: L.nsc_gicp_workspace_bytes(a[4], a[5], a[6]),
    "nsc_gicp_prepare": lambda L, a: L.nsc_gicp_prepare_workspace_bytes(a[2], a[3]),
    "nsc_gicp_register_prepared": lambda L, a: L.nsc_gicp_register_prepared_workspace_bytes(a[4]),
    "nsc_planar_align": lambda L, a: L.nsc_planar_align_workspace_bytes(a[4], a[6]),
    "nsc_posegraph_linearize": lambda L, a: L.nsc_posegraph_workspace_bytes(a[1], a[5], None),
    "nsc_posegraph_linearize_robust": lambda L, a: L.nsc_posegraph_workspace_bytes(a[1], a[5], None),
    "nsc_posegraph_optimize": lambda L, a: L.nsc_posegraph_workspace_bytes(a[1], a[5], a[7]),
    "nsc_posegraph_optimize_robust": lambda L, a: L.nsc_posegraph_workspace_bytes(a[1], a[5], a[7]),
    "nsc_posegraph_optimize_coarse": lambda L, a: L.nsc_posegraph_coarse_workspace_bytes(a[1], a[5], a[19]),
    "nsc_posegraph_covariance": lambda L, a: L.nsc_posegraph_covariance_workspace_bytes(a[1], a[5], a[9], a[19]),
    "nsc_map_build": lambda L, a: L.nsc_map_workspace_bytes(a[5], a[10]),
    "nsc_map_build_dist": lambda L, a: L.nsc_map_dist_workspace_bytes(a[5], a[11]),
    "nsc_map_insert_dist": lambda L, a: L.nsc_map_insert_workspace_bytes(a[5]),
    "nsc_map_remove_dist": lambda L, a: L.nsc_map_remove_workspace_bytes(a[5]),
    "nsc_map_replace_dist": lambda L, a: L.nsc_map_replace_workspace_bytes(a[5]),
    "nsc_map_register": lambda L, a: L.nsc_map_register_workspace_bytes(a[4]),
    "nsc_map_register_robust": lambda L, a: L.nsc_map_register_robust_workspace_bytes(a[4]),
}

# The state the audit justifies ("Workspaces"): the training forward saves its activations for the backward,
# "pass the SAME buffer".  {the call that reads the state: the call that left it}; the proxy keys the buffer on the caller's
# own ws pointer.  Nothing else in include/nsc.h carries anything from one call to the next.
STATE = {"nsc_gat_backward": "nsc_gat_forward_train"}

# The scenario of tests/test_workspace_contract_gpu.py that reaches each entry point.  nsc_gat_forward,
# nsc_posegraph_linearize and nsc_posegraph_optimize have no caller in the Python layer (it goes through the _ex, _robust
# and _coarse forms): their scenarios call them as the C ABI has them, the pose graph's through tests/_posegraph.py.
COVERED = {
    "nsc_encode_clouds": "scenario_encoder_split",
    "nsc_graph_build_csr": "scenario_gat_forward",
    "nsc_gat_forward": "scenario_gat_forward",
    "nsc_gat_forward_ex": "scenario_gat_forward_coresident",
    "nsc_graph_transpose": "scenario_training_step",
    "nsc_gat_forward_train": "scenario_training_step",
    "nsc_gat_backward": "scenario_training_step",
    "nsc_triplet_loss": "scenario_training_step",
    "nsc_mine_triplets_ws": "scenario_mine_semi_hard",
    "nsc_topk_smallest": "scenario_topk",
    "nsc_voxel_overlap": "scenario_voxel_overlap",
    "nsc_gicp_register": "scenario_gicp_register",
    "nsc_gicp_prepare": "scenario_gicp_prepared_and_planar",
    "nsc_gicp_register_prepared": "scenario_gicp_prepared_and_planar",
    "nsc_planar_align": "scenario_gicp_prepared_and_planar",
    "nsc_posegraph_linearize": "scenario_posegraph_plain",
    "nsc_posegraph_optimize": "scenario_posegraph_plain",
    "nsc_posegraph_linearize_robust": "scenario_posegraph_robust",
    "nsc_posegraph_optimize_robust": "scenario_posegraph_robust",
    "nsc_posegraph_optimize_coarse": "scenario_posegraph_coarse",
    "nsc_posegraph_covariance": "scenario_posegraph_covariance",
    "nsc_map_build": "scenario_global_map",
    "nsc_map_build_dist": "scenario_kept_map",
    "nsc_map_insert_dist": "scenario_kept_map",
    "nsc_map_remove_dist": "scenario_kept_map",
    "nsc_map_replace_dist": "scenario_kept_map",
    "nsc_map_register": "scenario_map_register",
    "nsc_map_register_robust": "scenario_map_register_robust",
}


class _Buffer:
    def __init__(self, symbol, need, whole):
        self.symbol, self.need, self.whole = symbol, need, whole

    @property
    def ws(self):
        return self.whole.data_ptr() + GUARD


class WorkspaceProxy:
    """Forwards every attribute to ``real`` (the CDLL, or anything with the same callables) and wraps the entry points
    with a workspace.  ``pattern``: the byte the workspaces are filled with.  ``device``: where they are allocated, None
    for the current HIP device at the time of the call (the wrappers call inside ``torch.cuda.device(dev)``).
    ``symbols`` and ``need`` default to ``_lib.SYMBOLS`` and NEED.

    seen    the set of entry points intercepted
    calls   [(entry point, bytes the contract promises)] in call order
    verify()  synchronises, asserts every guard byte of every workspace handed out, and releases them"""

    def __init__(self, real, pattern, device=None, symbols=None, need=None, state=None):
        self.__dict__.update(_real=real, _pattern=int(pattern), _device=device, _at=wrapped_symbols(symbols),
                             _need=NEED if need is None else need, _state=STATE if state is None else state,
                             _buffers=[], _kept={}, seen=set(), calls=[])

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        at = self._at.get(name)
        if at is None:
            return fn
        return lambda *args: self._call(name, fn, at, args)

    def _where(self):
        if self._device is not None:
            return torch.device(self._device)
        return torch.device("cuda", torch.cuda.current_device())

    def _call(self, name, fn, at, args):
        dev = self._where()
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            return fn(*args)                                   # capture is not part of this test
        self.seen.add(name)
        ws, ws_bytes = args[at], int(args[at + 1])
        ws = ws.value if isinstance(ws, C.c_void_p) else ws
        need = int(self._need[name](self._real, args))
        self.calls.append((name, need))
        assert ws_bytes >= need, f"{name}: the caller passes ws_bytes {ws_bytes}, the contract asks for {need}"
        if need == 0 and not ws:
            return fn(*args)                                   # "may be NULL if 0"
        left_by = self._state.get(name)
        if left_by is not None:
            buf = self._kept.get((left_by, ws))
            assert buf is not None and buf.need == need, \
                f"{name}: no workspace of {need} bytes left by {left_by} for the caller's buffer {ws}"
        else:
            whole = torch.empty(GUARD + need + GUARD, dtype=torch.uint8, device=dev)
            assert not whole.is_cuda or whole.data_ptr() % 256 == 0
            # torch fills on the current stream: ordered before the call, which is issued on that stream
            whole[:GUARD].fill_(GUARD_BYTE)
            whole[GUARD:GUARD + need].fill_(self._pattern)
            whole[GUARD + need:].fill_(GUARD_BYTE)
            buf = _Buffer(name, need, whole)
            self._buffers.append(buf)
            if name in self._state.values():
                self._kept[(name, ws)] = buf
        args = list(args)
        args[at], args[at + 1] = C.c_void_p(buf.ws), need      # exactly what the size query promised, not a byte more
        return fn(*args)

    def verify(self):
        if any(b.whole.is_cuda for b in self._buffers):
            torch.cuda.synchronize()
        try:
            for k, b in enumerate(self._buffers):
                for side, part, base in (("leading", b.whole[:GUARD], -GUARD), ("trailing", b.whole[GUARD + b.need:], b.need)):
                    bad = (part != GUARD_BYTE).nonzero()
                    assert bad.numel() == 0, (f"call {k}, {b.symbol}: the {side} guard of its {b.need}-byte workspace was "
                                              f"written, first at byte {base + int(bad[0])} of the workspace")
        finally:
            self._buffers.clear()
            self._kept.clear()
