"""Test helpers the pose-graph test files share: the mask that fixes pose 0 (the restatement's), the bitwise comparison of
two results, and the optimiser's entry points called as the C ABI has them (the Python layer goes through the robust and
coarse ones only).  torch and the library are imported where they are used, so the CPU tests can import this module."""
import ctypes as C

import numpy as np

from posegraph_cov_restatement import first_fixed  # noqa: F401


def same_bits(a, b, keys=None):
    for k in (keys or a):
        assert a[k].tobytes() == b[k].tobytes(), k


def optimizer(**params):
    from neural_spectral_codec_amd.retrieval import pose_graph as pg
    return pg.PoseGraphOptimizer(**params)


def host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- the entry points, called as the C ABI has them -------------------------------------------------------------------

def _device(X, e, Z, Om, *scale):
    import torch
    arrays = [np.asarray(X, np.float64), np.asarray(e, np.int64).reshape(-1, 2), np.asarray(Z, np.float64),
              np.asarray(Om, np.float64)] + [np.asarray(c, np.float64) for c in scale]
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def plain_linearize(X, e, Z, Om):
    import torch
    from neural_spectral_codec_amd import _lib
    L, ptr = _lib.lib(), _lib.ptr
    dX, de, dZ, dOm = _device(X, e, Z, Om)
    N, E = len(dX), len(de)
    f64 = dict(dtype=torch.float64, device="cuda")
    out = dict(residuals=torch.empty((E, 6), **f64), cost=torch.empty(1, **f64), gradient=torch.empty((N, 6), **f64),
               blocks=torch.empty((N, 21), **f64), skipped=torch.empty(1, dtype=torch.int64, device="cuda"))
    ws = torch.empty(max(int(L.nsc_posegraph_workspace_bytes(N, E, None)), 1), dtype=torch.uint8, device="cuda")
    _lib.check(L.nsc_posegraph_linearize(ptr(dX), N, ptr(de), ptr(dZ), ptr(dOm), E, ptr(out["residuals"]),
                                         ptr(out["cost"]), ptr(out["gradient"]), ptr(out["blocks"]), ptr(out["skipped"]),
                                         ptr(ws), int(ws.numel()), _lib.stream_ptr(ws.device)), "nsc_posegraph_linearize")
    return host(out)


def abi_optimize(entry, X, e, Z, Om, scale=None, kernel=None, coarse_block=None, fixed=None, ws=None, fill=None,
                 **params):
    """nsc_posegraph_optimize (no ``kernel``), nsc_posegraph_optimize_robust, or nsc_posegraph_optimize_coarse with
    ``coarse_block`` -> the outputs on the host: poses, stats, cost_history, step0, with a kernel chi2 and weights, with
    ``coarse_block`` coarse_stats.  ``fixed``: the mask, pose 0 when None.  ``ws``: the caller's own uint8 workspace
    tensor on the device, at least as large as the call needs.  ``fill``: a value every output holds before the call."""
    import torch
    from neural_spectral_codec_amd import _lib
    L, ptr = _lib.lib(), _lib.ptr
    prm = optimizer(**params).params
    dev = _device(X, e, Z, Om) if kernel is None else _device(X, e, Z, Om, scale)
    N, E = len(dev[0]), len(dev[1])
    fixed = torch.from_numpy((first_fixed(N) if fixed is None else np.asarray(fixed) != 0).astype(np.uint8)).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")

    def new(*shape):
        return torch.empty(shape, **f64) if fill is None else torch.full(shape, float(fill), **f64)
    out = dict(poses=new(N, 4, 4), stats=new(_lib.POSEGRAPH_STATS), cost_history=new(prm.max_iteration + 1),
               step0=new(N, 6))
    need = L.nsc_posegraph_workspace_bytes(N, E, None) if coarse_block is None else \
        L.nsc_posegraph_coarse_workspace_bytes(N, E, coarse_block)
    if ws is None:
        ws = torch.empty(max(int(need), 1), dtype=torch.uint8, device="cuda")
    assert ws.dtype == torch.uint8 and ws.is_cuda and ws.is_contiguous() and int(ws.numel()) >= int(need)
    args = (ptr(dev[0]), N, ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), E, ptr(fixed), C.byref(prm), ptr(out["poses"]),
            ptr(out["stats"]), ptr(out["cost_history"]), ptr(out["step0"]), ptr(ws), int(ws.numel()),
            _lib.stream_ptr(ws.device))
    if kernel is not None:
        out.update(chi2=new(E), weights=new(E))
        args += (kernel, ptr(dev[4]), ptr(out["chi2"]), ptr(out["weights"]))
    if coarse_block is not None:
        out["coarse_stats"] = new(2)
        args += (coarse_block, ptr(out["coarse_stats"]))
    _lib.check(getattr(L, entry)(*args), entry)
    return host(out)


def plain_optimize(X, e, Z, Om, **params):
    return abi_optimize("nsc_posegraph_optimize", X, e, Z, Om, **params)
