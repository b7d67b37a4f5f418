"""1-D Wasserstein retrieval on MI355X -- drop-in for the device-side functions of the reference's
src/retrieval/wasserstein.py: ``wasserstein_distance_batch_torch`` (:134-172),
``wasserstein_distance_matrix_torch`` (:232-273) and ``WassersteinRetriever`` (:276-389).

W1 between 1-D histograms is the L1 distance of their CDFs.  The database is streamed once per query
batch by nsc_w1_distances (one wavefront per row), the k smallest distances are selected on the device
(nsc_topk_smallest).  Additive over the reference: batched queries, the spatial filter of
TwoStageRetrieval._global_retrieval (two_stage_retrieval.py:160-170) fused into the distance kernel, and
an amortised-doubling database buffer instead of torch.cat per insert (:324).
"""
from typing import Optional, Union

import numpy as np
import torch

from .. import _lib


def _dev_f32(t, device=None):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t)
    t = t.detach().to(dtype=torch.float32)
    if device is not None:
        t = t.to(device)
    _lib.require_cuda(t, "histograms")
    return t.contiguous()


def _pos_f32(p, device):
    """(n,3) positions (host array or tensor on any device) -> contiguous float32 tensor on `device`."""
    if not isinstance(p, torch.Tensor):
        p = torch.from_numpy(np.asarray(p, dtype=np.float32))
    return p.detach().to(device=device, dtype=torch.float32).reshape(-1, 3).contiguous()


def _grow_rows(bufs, live: int, need: int, first: int = 1024):
    """Amortised doubling: zeroed (max(need, 2 * cap, first), ...) buffers holding the ``live`` rows; a None stays None."""
    cap = max(need, 2 * int(bufs[0].shape[0]), first)
    out = [None if b is None else b.new_zeros((cap,) + tuple(b.shape[1:])) for b in bufs]
    for nb, b in zip(out, bufs):
        if b is not None:
            nb[:live] = b[:live]
    return out


def _cdf(h: torch.Tensor, eps: float, divide_plain: bool) -> torch.Tensor:
    out = torch.empty_like(h)
    _lib.call("nsc_w1_cdf", h.device, h, int(h.shape[0]), int(h.shape[1]), float(eps), int(divide_plain), out, _lib.STREAM)
    return out


def _distances(db: torch.Tensor, qcdf: torch.Tensor, eps: float, db_pos=None, q_pos=None,
               min_dist: float = 0.0) -> torch.Tensor:
    n, d, q = int(db.shape[0]), int(db.shape[1]), int(qcdf.shape[0])
    dist = torch.empty((q, n), dtype=torch.float32, device=db.device)
    _lib.call("nsc_w1_distances", db.device, db, n, d, float(eps), qcdf, q, db_pos, q_pos, float(min_dist), dist, _lib.STREAM)
    return dist


def _distances_cdf(db_cdf: torch.Tensor, qcdf: torch.Tensor, db_pos=None, q_pos=None,
                   min_dist: float = 0.0) -> torch.Tensor:
    """W1 of query CDFs against rows that are already CDFs (nsc_w1_distances_cdf)."""
    n, d, q = int(db_cdf.shape[0]), int(db_cdf.shape[1]), int(qcdf.shape[0])
    dist = torch.empty((q, n), dtype=torch.float32, device=db_cdf.device)
    _lib.call("nsc_w1_distances_cdf", db_cdf.device, db_cdf, n, d, qcdf, q, db_pos, q_pos, float(min_dist), dist, _lib.STREAM)
    return dist


def _topk(dist: torch.Tensor, k: int):
    q, n = int(dist.shape[0]), int(dist.shape[1])
    idx = torch.empty((q, k), dtype=torch.int64, device=dist.device)
    val = torch.empty((q, k), dtype=torch.float32, device=dist.device)
    L = _lib.lib()
    nbytes = L.nsc_topk_workspace_bytes(q, n, k)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dist.device)
    with torch.cuda.device(dist.device):
        st = L.nsc_topk_smallest(_lib.ptr(dist), q, n, k, _lib.ptr(idx), _lib.ptr(val), _lib.ptr(ws), nbytes,
                                 _lib.stream_ptr(dist.device))
    if st == -2 and 0 < k <= n:
        # beyond the selection kernel's range (k > 256: the reference's callers ask for 10-50, but `query(top_k=n)` is legal there,
        # wasserstein.py:380): a stable device sort gives the same (value, index) order -- still on the device, no host copy
        val, idx = torch.sort(dist, dim=1, stable=True)
        idx, val = idx[:, :k].contiguous(), val[:, :k].contiguous()
        # the selection kernel never picks a NaN (a NaN histogram row): the slots a row cannot fill hold -1 / +inf.
        # torch.sort puts NaN last, so the same answer is the sorted one with its NaN tail rewritten
        nan = torch.isnan(val)
        return idx.masked_fill_(nan, -1), val.masked_fill_(nan, float("inf"))
    _lib.check(st, "nsc_topk_smallest")
    return idx, val


def wasserstein_distance_batch_torch(query_hist: torch.Tensor, database_hists: torch.Tensor,
                                     epsilon: float = 1e-8) -> torch.Tensor:
    """(n_bins,) query vs (n_database, n_bins) -> (n_database,)          wasserstein.py:134-172"""
    db = _dev_f32(database_hists)
    q = _dev_f32(query_hist, db.device).reshape(1, -1)
    return _distances(db, _cdf(q, epsilon, True), epsilon)[0]


def wasserstein_distance_matrix_torch(hists1: torch.Tensor, hists2: Optional[torch.Tensor] = None,
                                      epsilon: float = 1e-8) -> torch.Tensor:
    """(n1, n_bins) x (n2, n_bins) -> (n1, n2), D[i,j] = W1(hists1[i], hists2[j])   wasserstein.py:232-273"""
    h1 = _dev_f32(hists1)
    h2 = h1 if hists2 is None else _dev_f32(hists2, h1.device)
    return _distances(h2, _cdf(h1, epsilon, False), epsilon)


def wasserstein_distance_1d_torch(hist1: torch.Tensor, hist2: torch.Tensor, epsilon: float = 1e-8) -> torch.Tensor:
    """Two (n_bins,) histograms, both normalised by their plain sum -> scalar tensor   wasserstein.py:55-87"""
    h1 = _dev_f32(hist1)
    h2 = _dev_f32(hist2, h1.device)
    c = _cdf(torch.stack([h1.reshape(-1), h2.reshape(-1)]), epsilon, True)
    return (c[0] - c[1]).abs().sum()


def _default_device():
    if not torch.cuda.is_available():
        raise _lib.NscError("the Wasserstein functions run on a HIP device; none is available (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def wasserstein_distance_1d_numpy(hist1: np.ndarray, hist2: np.ndarray, epsilon: float = 1e-8) -> float:
    """wasserstein.py:20-52 with host arrays in and a Python float out (computed on the device)."""
    dev = _default_device()
    return float(wasserstein_distance_1d_torch(torch.from_numpy(np.asarray(hist1, dtype=np.float32)).to(dev),
                                               torch.from_numpy(np.asarray(hist2, dtype=np.float32)).to(dev),
                                               epsilon).item())


def wasserstein_distance_batch_numpy(query_hist: np.ndarray, database_hists: np.ndarray,
                                     epsilon: float = 1e-8) -> np.ndarray:
    """wasserstein.py:90-131: (n_bins,) vs (n_database, n_bins) -> (n_database,) ndarray."""
    dev = _default_device()
    return wasserstein_distance_batch_torch(torch.from_numpy(np.asarray(query_hist, dtype=np.float32)).to(dev),
                                            torch.from_numpy(np.asarray(database_hists, dtype=np.float32)).to(dev),
                                            epsilon).cpu().numpy()


def wasserstein_distance_matrix_numpy(hists1: np.ndarray, hists2: Optional[np.ndarray] = None,
                                      epsilon: float = 1e-8) -> np.ndarray:
    """wasserstein.py:175-229: (n1, n_bins) x (n2, n_bins) -> (n1, n2) ndarray."""
    dev = _default_device()
    h1 = torch.from_numpy(np.asarray(hists1, dtype=np.float32)).to(dev)
    h2 = None if hists2 is None else torch.from_numpy(np.asarray(hists2, dtype=np.float32)).to(dev)
    return wasserstein_distance_matrix_torch(h1, h2, epsilon).cpu().numpy()


class WassersteinRetriever:
    """wasserstein.py:276-389 (``use_torch`` is accepted for signature compatibility; the database
    always lives in HBM)."""

    def __init__(self, use_torch: bool = True, device: str = 'cuda'):
        self.use_torch = use_torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.NscError("WassersteinRetriever keeps its database in HBM: device must be a HIP device")
        self._buf = None
        self._cdf_buf = None       # normalised CDF of every database row (only when n_bins % 4 == 0)
        self._pos = None
        self.database_size = 0

    @property
    def database_hists(self):
        return None if self._buf is None else self._buf[:self.database_size]

    def add_to_database(self, histograms: Union[np.ndarray, torch.Tensor], positions=None):
        """:301-326.  ``positions`` (n,3) are optional keyframe translations for the spatial filter."""
        h = _dev_f32(histograms if not isinstance(histograms, np.ndarray) else torch.from_numpy(histograms),
                     self.device)
        if h.dim() == 1:
            h = h.unsqueeze(0)
        n, d = int(h.shape[0]), int(h.shape[1])
        need = self.database_size + n
        if self._buf is None:
            self._buf, self._pos = h.new_empty((0, d)), h.new_empty((0, 3))
            self._cdf_buf = h.new_empty((0, d)) if d % 4 == 0 else None
        if need > self._buf.shape[0]:
            self._buf, self._pos, self._cdf_buf = _grow_rows((self._buf, self._pos, self._cdf_buf), self.database_size, need)
        self._buf[self.database_size:need] = h
        if self._cdf_buf is not None:
            # the database form of the normalisation (wasserstein.py:158-163), done once per inserted row
            self._cdf_buf[self.database_size:need] = _cdf(h, 1e-8, False)
        if positions is not None:
            self._pos[self.database_size:need] = _pos_f32(positions, self.device)
        self.database_size = need

    def query_batch(self, query_hists, top_k: int = 10, query_positions=None, min_distance: float = 0.0):
        """(Q, n_bins) queries -> (indices (Q,k) int64, distances (Q,k)) device tensors, ascending.
        With ``query_positions`` database entries closer than ``min_distance`` are excluded
        (two_stage_retrieval.py:160-170)."""
        if self.database_size == 0:
            e = torch.empty((0, 0), device=self.device)
            return e.long(), e
        q = _dev_f32(query_hists, self.device)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        db = self._buf[:self.database_size]
        qp = dbp = None
        if query_positions is not None:
            qp = _pos_f32(query_positions, self.device)
            dbp = self._pos[:self.database_size]
        if self._cdf_buf is not None:
            dist = _distances_cdf(self._cdf_buf[:self.database_size], _cdf(q, 1e-8, True), dbp, qp, min_distance)
        else:
            dist = _distances(db, _cdf(q, 1e-8, True), 1e-8, dbp, qp, min_distance)
        return _topk(dist, min(top_k, self.database_size))

    def query(self, query_hist: Union[np.ndarray, torch.Tensor], top_k: int = 10) -> tuple:
        """:328-384: (indices (top_k,), distances (top_k,)) as numpy arrays, ascending distance."""
        if self.database_size == 0:
            return np.array([]), np.array([])
        idx, val = self.query_batch(query_hist, top_k)
        return idx[0].cpu().numpy(), val[0].cpu().numpy()

    def clear_database(self):
        """:386-389"""
        self._buf = self._pos = self._cdf_buf = None
        self.database_size = 0
