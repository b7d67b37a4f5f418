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


def abi_optimize(entry, X, e, Z, Om, scale=None, kernel=None, coarse_block=None, **params):
    """nsc_posegraph_optimize (no ``kernel``), nsc_posegraph_optimize_robust, or nsc_posegraph_optimize_coarse with
    ``coarse_block``, pose 0 fixed -> the outputs on the host: poses, stats, cost_history, step0, with a kernel chi2 and
    weights, with ``coarse_block`` coarse_stats"""
    import torch
    from neural_spectral_codec_amd import _lib
    L, ptr = _lib.lib(), _lib.ptr
    prm = optimizer(**params).params
    dev = _device(X, e, Z, Om) if kernel is None else _device(X, e, Z, Om, scale)
    N, E = len(dev[0]), len(dev[1])
    fixed = torch.from_numpy(first_fixed(N).astype(np.uint8)).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    out = dict(poses=torch.empty((N, 4, 4), **f64), stats=torch.empty(_lib.POSEGRAPH_STATS, **f64),
               cost_history=torch.empty(prm.max_iteration + 1, **f64), step0=torch.empty((N, 6), **f64))
    need = L.nsc_posegraph_workspace_bytes(N, E, None) if coarse_block is None else \
        L.nsc_posegraph_coarse_workspace_bytes(N, E, coarse_block)
    ws = torch.empty(max(int(need), 1), dtype=torch.uint8, device="cuda")
    args = (ptr(dev[0]), N, ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), E, ptr(fixed), C.byref(prm), ptr(out["poses"]),
            ptr(out["stats"]), ptr(out["cost_history"]), ptr(out["step0"]), ptr(ws), int(ws.numel()),
            _lib.stream_ptr(ws.device))
    if kernel is not None:
        out.update(chi2=torch.empty(E, **f64), weights=torch.empty(E, **f64))
        args += (kernel, ptr(dev[4]), ptr(out["chi2"]), ptr(out["weights"]))
    if coarse_block is not None:
        out["coarse_stats"] = torch.empty(2, **f64)
        args += (coarse_block, ptr(out["coarse_stats"]))
    _lib.check(getattr(L, entry)(*args), entry)
    return host(out)


def plain_optimize(X, e, Z, Om, **params):
    return abi_optimize("nsc_posegraph_optimize", X, e, Z, Om, **params)
