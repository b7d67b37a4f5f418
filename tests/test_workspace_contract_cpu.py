"""tests/workspace_contract.py without a GPU and without the library: the proxy against three fake entry points that are
plain Python callables on CPU tensors, and the NEED and COVERED tables against ``_lib.SYMBOLS``."""
import ast
import ctypes as C
import os

import pytest
import torch

import workspace_contract as W
from neural_spectral_codec_amd import _lib

_vp, _i32, _sz = C.c_void_p, C.c_int32, C.c_size_t
FAKE_SYMBOLS = {
    "fake_workspace_bytes": (_sz, [_i32]),
    "fake_good": (C.c_int, [_vp, _i32, _vp, _sz]),
    "fake_overrun": (C.c_int, [_vp, _i32, _vp, _sz]),
    "fake_reads_unwritten": (C.c_int, [_vp, _i32, _vp, _sz]),
    "fake_keeps": (C.c_int, [_vp, _i32, _vp, _sz]),
    "fake_takes": (C.c_int, [_vp, _i32, _vp, _sz]),
    "fake_no_workspace": (C.c_int, [_vp, _i32]),
}
FAKE_NEED = {k: (lambda L, a: L.fake_workspace_bytes(a[1])) for k in FAKE_SYMBOLS
             if k not in ("fake_workspace_bytes", "fake_no_workspace")}


def _bytes(ptr, n):
    ptr = ptr.value if isinstance(ptr, C.c_void_p) else ptr
    return (C.c_uint8 * n).from_address(ptr)


class FakeLibrary:
    """out (n bytes) = 2 * (0 .. n - 1) mod 256, staged through a workspace of 3 n + 5 bytes (no multiple of anything)"""

    def __init__(self):
        self.got = []                                   # (ws, ws_bytes) of every call

    @staticmethod
    def fake_workspace_bytes(n):
        return 3 * n + 5 if n > 0 else 0

    def _stage(self, out, n, ws, ws_bytes, extra=0, skip=None):
        self.got.append((ws.value if isinstance(ws, C.c_void_p) else ws, ws_bytes))
        if n == 0:
            return 0
        w, o = _bytes(ws, ws_bytes + extra), _bytes(out, n)
        for i in range(ws_bytes + extra):
            if i != skip:
                w[i] = (2 * i) % 256
        for i in range(n):
            o[i] = w[i]
        return 0

    def fake_good(self, out, n, ws, ws_bytes):
        return self._stage(out, n, ws, ws_bytes)

    def fake_overrun(self, out, n, ws, ws_bytes):
        return self._stage(out, n, ws, ws_bytes, extra=1)          # one byte past what it asked for

    def fake_reads_unwritten(self, out, n, ws, ws_bytes):
        return self._stage(out, n, ws, ws_bytes, skip=1)           # out[1] is a workspace byte it never wrote

    def fake_keeps(self, out, n, ws, ws_bytes):
        return self._stage(out, n, ws, ws_bytes)

    def fake_takes(self, out, n, ws, ws_bytes):                    # reads what fake_keeps left: documented state
        self.got.append((ws.value, ws_bytes))
        w, o = _bytes(ws, ws_bytes), _bytes(out, n)
        for i in range(n):
            o[i] = w[n + i]
        return 0

    @staticmethod
    def fake_no_workspace(out, n):
        return 7


def proxy(pattern, **kw):
    lib = FakeLibrary()
    return lib, W.WorkspaceProxy(lib, pattern, device="cpu", symbols=FAKE_SYMBOLS, need=FAKE_NEED,
                                 state=kw.get("state", {}))


def call(p, name, n, caller_bytes=None):
    out = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8)
    need = FakeLibrary.fake_workspace_bytes(n)
    caller = torch.zeros(max(need if caller_bytes is None else caller_bytes, 1) + 64, dtype=torch.uint8)
    st = getattr(p, name)(C.c_void_p(out.data_ptr()), n, C.c_void_p(caller.data_ptr()),
                          need + 64 if caller_bytes is None else caller_bytes)
    assert st == 0
    return out[:n].clone(), caller


def test_wrapped_symbols_of_the_fake():
    assert W.wrapped_symbols(FAKE_SYMBOLS) == {k: 2 for k in FAKE_NEED}


@pytest.mark.parametrize("pattern", W.PATTERNS)
def test_correct_entry_point(pattern):
    lib, p = proxy(pattern)
    out, caller = call(p, "fake_good", 37)
    assert out.tolist() == [(2 * i) % 256 for i in range(37)]
    assert not caller.any(), "the caller's own buffer was handed to the library"
    (ws, ws_bytes), = lib.got
    assert ws_bytes == 3 * 37 + 5, "the library gets exactly what the size query promised"
    assert ws != caller.data_ptr()
    assert p.seen == {"fake_good"} and p.calls == [("fake_good", 116)]
    p.verify()
    assert p.fake_no_workspace(None, 3) == 7 and p.seen == {"fake_good"}      # everything else is forwarded as it is


@pytest.mark.parametrize("pattern", W.PATTERNS)
def test_workspace_is_filled_with_the_pattern_between_guards(pattern):
    seen = {}

    class Peek(FakeLibrary):
        def fake_good(self, out, n, ws, ws_bytes):
            seen["before"] = bytes(_bytes(ws.value - W.GUARD, W.GUARD))
            seen["middle"] = bytes(_bytes(ws, ws_bytes))
            seen["after"] = bytes(_bytes(ws.value + ws_bytes, W.GUARD))
            return 0
    p = W.WorkspaceProxy(Peek(), pattern, device="cpu", symbols=FAKE_SYMBOLS, need=FAKE_NEED, state={})
    call(p, "fake_good", 11)
    assert seen["middle"] == bytes([pattern]) * 38
    assert seen["before"] == seen["after"] == bytes([W.GUARD_BYTE]) * W.GUARD
    p.verify()


def test_one_byte_past_the_workspace_fails_on_the_trailing_guard():
    lib, p = proxy(0x00)
    call(p, "fake_good", 5)
    call(p, "fake_overrun", 9)
    with pytest.raises(AssertionError, match=r"call 1, fake_overrun: the trailing guard .* first at byte 32 "):
        p.verify()
    p.verify()                                           # released: a second verify has nothing to find


def test_one_byte_in_front_of_the_workspace_fails_on_the_leading_guard():
    class Under(FakeLibrary):
        def fake_good(self, out, n, ws, ws_bytes):
            _bytes(ws.value - 1, 1)[0] = 0
            return 0
    p = W.WorkspaceProxy(Under(), 0xFF, device="cpu", symbols=FAKE_SYMBOLS, need=FAKE_NEED, state={})
    call(p, "fake_good", 5)
    with pytest.raises(AssertionError, match=r"the leading guard .* first at byte -1 "):
        p.verify()


def test_unwritten_workspace_byte_shows_between_patterns():
    outs = []
    for pattern in W.PATTERNS:
        lib, p = proxy(pattern)
        outs.append(call(p, "fake_reads_unwritten", 20)[0])
        p.verify()                                       # nothing out of bounds: only the comparison can tell
    assert outs[0][1] == 0x00 and outs[1][1] == 0xFF and outs[2][1] == 0x3C
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    good = [call(proxy(pt)[1], "fake_good", 20)[0] for pt in W.PATTERNS]
    assert torch.equal(good[0], good[1]) and torch.equal(good[1], good[2])


def test_caller_with_too_small_a_workspace_is_refused():
    lib, p = proxy(0x00)
    with pytest.raises(AssertionError, match="the contract asks for 35"):
        call(p, "fake_good", 10, caller_bytes=34)
    assert not lib.got


def test_no_workspace_needed_and_none_given_passes_through():
    lib, p = proxy(0xFF)
    assert p.fake_good(None, 0, None, 0) == 0
    assert lib.got == [(None, 0)] and p.calls == [("fake_good", 0)]
    p.verify()


def test_documented_state_reaches_the_second_call_without_new_poison():
    state = {"fake_takes": "fake_keeps"}
    lib, p = proxy(0xFF, state=state)
    n = 6
    out = torch.zeros(n, dtype=torch.uint8)
    caller = torch.zeros(64, dtype=torch.uint8)
    other = torch.zeros(64, dtype=torch.uint8)
    args = (C.c_void_p(out.data_ptr()), n, C.c_void_p(caller.data_ptr()), 64)
    assert p.fake_keeps(*args) == 0 and p.fake_takes(*args) == 0
    assert lib.got[0] == lib.got[1], "the second call gets the first call's buffer"
    assert out.tolist() == [(2 * (n + i)) % 256 for i in range(n)]
    with pytest.raises(AssertionError, match="no workspace of 23 bytes left by fake_keeps"):
        p.fake_takes(C.c_void_p(out.data_ptr()), n, C.c_void_p(other.data_ptr()), 64)
    p.verify()


# ---- the tables against the library's symbols -----------------------------------------------------------------------

def test_need_has_exactly_the_entry_points_with_a_workspace():
    wrapped = W.wrapped_symbols()
    assert set(W.NEED) == set(wrapped)
    assert len(wrapped) == 28
    for name, at in wrapped.items():
        args = _lib.SYMBOLS[name][1]
        assert args[at] is C.c_void_p and args.count(C.c_size_t) == 1, name
    # every size query NEED calls is a symbol, and each is called by some entry
    queries = {n for n, (res, args) in _lib.SYMBOLS.items() if res is C.c_size_t and n.endswith("_workspace_bytes")}
    used = set()
    for fn in W.NEED.values():
        used |= set(fn.__code__.co_names) & set(_lib.SYMBOLS)
    assert used == queries


def test_need_indexes_the_arguments_it_means():
    """each lambda against a recording stand-in: the sizes it hands the query are the arguments of those names in
    include/nsc.h, found here by their position in the argtypes"""
    class Rec:
        def __getattr__(self, q):
            return lambda *a: (q, a)
    g, mp = _lib.Graph(n_nodes=41), _lib.MineParams(strategy=2)
    m, prm = _lib.GatModel(), _lib.PoseGraphParams()
    a = list(range(100, 130))
    R = Rec()
    assert W.NEED["nsc_encode_clouds"](R, a)[1] == (102, 103, 105)
    assert W.NEED["nsc_graph_build_csr"](R, a)[1] == (102, 101)
    for k in ("nsc_gat_forward", "nsc_gat_forward_ex"):
        assert W.NEED[k](R, [m, C.byref(g)])[1] == (m, 41)
    assert W.NEED["nsc_graph_transpose"](R, [C.byref(g)])[1] == (41,)
    assert W.NEED["nsc_mine_triplets_ws"](R, a[:4] + [C.byref(mp)])[1] == (102, 2)
    assert W.NEED["nsc_topk_smallest"](R, a)[1] == (101, 102, 103)
    assert W.NEED["nsc_voxel_overlap"](R, a)[1] == (105, 106)
    assert W.NEED["nsc_gicp_register"](R, a)[1] == (104, 105, 106)
    assert W.NEED["nsc_gicp_prepare"](R, a)[1] == (102, 103)
    assert W.NEED["nsc_gicp_register_prepared"](R, a)[1] == (104,)
    assert W.NEED["nsc_planar_align"](R, a)[1] == (104, 106)
    assert W.NEED["nsc_posegraph_optimize"](R, a[:7] + [prm])[1] == (101, 105, prm)
    assert W.NEED["nsc_posegraph_optimize_coarse"](R, a)[1] == (101, 105, 119)
    assert W.NEED["nsc_posegraph_covariance"](R, a)[1] == (101, 105, 109, 119)
    assert W.NEED["nsc_map_build"](R, a)[1] == (105, 110)
    assert W.NEED["nsc_map_build_dist"](R, a)[1] == (105, 111)
    for k in ("nsc_map_insert_dist", "nsc_map_remove_dist", "nsc_map_replace_dist"):
        assert W.NEED[k](R, a)[1] == (105,)
    for k in ("nsc_map_register", "nsc_map_register_robust", "nsc_triplet_loss"):
        assert W.NEED[k](R, a)[1] == (104,)
    # the positions above, against the argtypes: the struct pointers and the 32- or 64-bit sizes stand where NEED reads them
    S = _lib.SYMBOLS
    assert S["nsc_posegraph_optimize_coarse"][1][19] is C.c_int32 and S["nsc_posegraph_covariance"][1][19] is C.c_int32
    assert S["nsc_posegraph_covariance"][1][9] is C.c_int32 and S["nsc_posegraph_optimize"][1][7] == C.POINTER(_lib.PoseGraphParams)
    assert S["nsc_map_build"][1][10] is C.c_int64 and S["nsc_map_build_dist"][1][11] is C.c_int64
    assert S["nsc_map_build_dist"][1][10] == C.POINTER(_lib.MapDistParams)
    assert S["nsc_mine_triplets_ws"][1][4] == C.POINTER(_lib.MineParams) and S["nsc_encode_clouds"][1][5] == C.POINTER(_lib.EncParams)


def test_state_names_entry_points_with_a_workspace():
    wrapped = W.wrapped_symbols()
    assert set(W.STATE) <= set(wrapped) and set(W.STATE.values()) <= set(wrapped)


def test_every_entry_point_with_a_workspace_has_a_gpu_scenario():
    """a future entry point with a workspace fails here until a scenario of the GPU file reaches it"""
    assert set(W.COVERED) == set(W.wrapped_symbols())
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_workspace_contract_gpu.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    scenarios = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("scenario_")}
    assert set(W.COVERED.values()) == scenarios
