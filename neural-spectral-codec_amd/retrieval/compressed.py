"""Stage-1 retrieval over quantised descriptors on MI355X -- additive over the reference.

A descriptor travels as a uint16 histogram whose bins sum to 65535 (encoding/quantization.py, a *canonical* row).
Its integer CDF fits uint16 entry by entry, and ``sum_k |cdf_a[k] - cdf_b[k]| / 65535`` is W1 between the
dequantised histograms, with an integer sum that no kernel, tiling or batch can change.  ``CompressedRetriever``
keeps only that CDF (the bins are its first differences): ``2 * n_bins + 13`` bytes of HBM per keyframe where
``WassersteinRetriever`` keeps ``8 * n_bins + 12``, and half the bytes per query pass.  Records received from
another robot or read from disk are searched as they are (``add_records``), without a float32 copy.

A row that is not canonical (the quantiser emits one only for a histogram without mass) has no distance: it is
stored, never returned, and every pair with it is ``+inf``.  There is no CPU fallback.
"""
from typing import Optional, Union

import numpy as np
import torch

from .. import _lib
from ..encoding import quantization as _qz
from .wasserstein import _dev_f32, _grow_rows, _pos_f32, _topk


def _dev_u16(q, device=None, name="quantized") -> torch.Tensor:
    """(n, D) or (D,) uint16 rows (host array or tensor) -> contiguous (n, D) uint16 device tensor."""
    if isinstance(q, np.ndarray):
        q = torch.from_numpy(np.ascontiguousarray(q))
    if q.dtype != torch.uint16:
        raise _lib.NscError(f"{name} must be uint16 (got {q.dtype})")
    if device is not None:
        q = q.to(device)
    _lib.require_cuda(q, name)
    if q.dim() == 1:
        q = q.unsqueeze(0)
    return q.contiguous()


def quantized_cdf(quantized):
    """(n, D) uint16 quantised histograms -> (cdf (n, D) uint16, canonical (n,) uint8): the integer CDF of every row
    whose bins sum to exactly 65535, a row of zeros and flag 0 for any other row (nsc_w1q_cdf)."""
    q = _dev_u16(quantized)
    n, d = int(q.shape[0]), int(q.shape[1])
    cdf = torch.empty((n, d), dtype=torch.uint16, device=q.device)
    ok = torch.empty((n,), dtype=torch.uint8, device=q.device)
    _lib.call("nsc_w1q_cdf", q.device, q, n, d, cdf, ok, _lib.STREAM)
    return cdf, ok


def w1_distances_quantized(db_cdf, db_canonical, q_cdf, q_canonical, db_pos=None, q_pos=None,
                           min_distance: float = 0.0) -> torch.Tensor:
    """(N, D) and (Q, D) uint16 CDF rows with their canonical flags -> (Q, N) float32 distances (nsc_w1q_distances):
    ``float32(d_int) / float32(65535)``, ``+inf`` where either row is not canonical or, with both position arrays,
    the pair is closer than ``min_distance``."""
    for t, name in ((db_cdf, "db_cdf"), (q_cdf, "q_cdf")):
        _lib.require_cuda(t, name)
        if t.dtype not in (torch.uint16, torch.int16) or t.dim() != 2 or not t.is_contiguous():
            raise _lib.NscError(f"{name} must be a contiguous (n, D) uint16 tensor")
    n, d, q = int(db_cdf.shape[0]), int(db_cdf.shape[1]), int(q_cdf.shape[0])
    if int(q_cdf.shape[1]) != d or int(db_canonical.numel()) != n or int(q_canonical.numel()) != q:
        raise _lib.NscError("w1_distances_quantized: inconsistent shapes")
    dev = db_cdf.device
    db_ok = db_canonical.to(device=dev, dtype=torch.uint8).contiguous()
    q_ok = q_canonical.to(device=dev, dtype=torch.uint8).contiguous()
    dbp = None if db_pos is None else _pos_f32(db_pos, dev)
    qp = None if q_pos is None else _pos_f32(q_pos, dev)
    dist = torch.empty((q, n), dtype=torch.float32, device=dev)
    _lib.call("nsc_w1q_distances", dev, db_cdf, db_ok, n, d, q_cdf, q_ok, q, dbp, qp, float(min_distance), dist, _lib.STREAM)
    return dist


class CompressedRetriever:
    """``WassersteinRetriever`` over 16-bit rows: the same surface, a database of uint16 CDF rows.

    Results carry index ``-1`` and distance ``+inf`` in every slot that no canonical, unfiltered row fills.
    ``n_noncanonical`` counts the stored rows that can never be returned; it is kept on the host from a one-number
    readback per insert."""

    INITIAL_CAPACITY = 1024

    def __init__(self, device: str = 'cuda'):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.NscError("CompressedRetriever keeps its database in HBM: device must be a HIP device")
        self._cdf = self._ok = self._pos = None      # (cap, D) int16 (the uint16 bits), (cap,) uint8, (cap, 3) float32
        self.database_size = 0
        self.n_noncanonical = 0

    @property
    def n_bins(self) -> Optional[int]:
        return None if self._cdf is None else int(self._cdf.shape[1])

    @property
    def database_cdf(self):
        return None if self._cdf is None else self._cdf[:self.database_size].view(torch.uint16)

    def bytes_per_keyframe(self) -> int:
        return 0 if self._cdf is None else 2 * self.n_bins + 13

    # -- inserts ---------------------------------------------------------------------------------
    def _grow(self, need: int, d: int):
        if self._cdf is not None and int(self._cdf.shape[1]) != d:
            raise _lib.NscError(f"the database holds {self.n_bins}-bin rows (got {d})")
        if self._cdf is None:
            # int16 storage: the uint16 bits, in a dtype every torch copy supports
            self._cdf, self._ok, self._pos = (torch.empty(s, dtype=t, device=self.device) for s, t in
                                              (((0, d), torch.int16), ((0,), torch.uint8), ((0, 3), torch.float32)))
        if need > self._cdf.shape[0]:
            bufs = (self._cdf, self._ok, self._pos)
            self._cdf, self._ok, self._pos = _grow_rows(bufs, self.database_size, need, self.INITIAL_CAPACITY)

    def add_quantized(self, quantized, positions=None):
        """(n, D) uint16 rows as the quantiser emits them; ``positions`` (n, 3) optional keyframe translations for
        the spatial filter."""
        q = _dev_u16(quantized, self.device)
        n, d = int(q.shape[0]), int(q.shape[1])
        if n == 0:
            return
        need = self.database_size + n
        self._grow(need, d)
        cdf, ok = quantized_cdf(q)
        self._cdf[self.database_size:need] = cdf.view(torch.int16)
        self._ok[self.database_size:need] = ok
        if positions is not None:
            self._pos[self.database_size:need] = _pos_f32(positions, self.device)
        self.n_noncanonical += n - int(ok.sum(dtype=torch.int64).item())
        self.database_size = need

    def add_records(self, records, n_bins: Optional[int] = None):
        """Insert wire records (``2 * n_bins + 120`` bytes each, encoding/quantization.py): an (n, record) uint8 device
        tensor, a list of ``bytes`` (one record each), or ``bytes`` holding one record or several back to back (then
        ``n_bins`` says where they split unless the database already fixes it).  Positions come from the records'
        poses.  -> (keyframe_ids (n,) int64, timestamps (n,) float64) device tensors."""
        if isinstance(records, (bytes, bytearray, memoryview)):
            records = [bytes(records)]
            d = n_bins or self.n_bins
            if d is not None:
                blob, rb = records[0], _qz.record_bytes(d)
                if len(blob) == 0 or len(blob) % rb:
                    raise ValueError(f"{len(blob)} bytes are not a whole number of {rb}-byte records")
                records = [blob[i:i + rb] for i in range(0, len(blob), rb)]
        if not isinstance(records, torch.Tensor):
            records = list(records)
            if not records:
                e = torch.empty((0,), device=self.device)
                return e.long(), e.double()
            if len({len(r) for r in records}) != 1:
                raise ValueError("records of different lengths")
            host = np.frombuffer(b"".join(bytes(r) for r in records), dtype=np.uint8).reshape(len(records), -1)
            records = torch.from_numpy(host.copy())
        rec = records.to(self.device)
        if rec.dim() != 2 or rec.dtype != torch.uint8 or int(rec.shape[1]) < 122 or (int(rec.shape[1]) - 120) % 2:
            raise ValueError(f"not descriptor records: {tuple(rec.shape)} {rec.dtype}")
        d = (int(rec.shape[1]) - 120) // 2
        if n_bins is not None and d != n_bins:
            raise ValueError(f"records of {d} bins (n_bins={n_bins})")
        q, pose7, ts, ids, _ = _qz.unpack_records(rec, d)
        self.add_quantized(q, positions=pose7[:, :3])
        return ids.view(torch.int32).to(torch.int64) & 0xFFFFFFFF, ts

    def add_to_database(self, histograms: Union[np.ndarray, torch.Tensor], positions=None):
        """Float histograms, quantised at insert (``quantize_batch``): the signature of WassersteinRetriever."""
        h = _dev_f32(histograms, self.device)
        if h.dim() == 1:
            h = h.unsqueeze(0)
        self.add_quantized(_qz.quantize_batch(h), positions=positions)

    # -- queries ---------------------------------------------------------------------------------
    def _query_rows(self, queries) -> torch.Tensor:
        t = torch.from_numpy(queries) if isinstance(queries, np.ndarray) else queries
        if t.dtype == torch.uint16:
            return _dev_u16(t, self.device, "queries")
        h = _dev_f32(t, self.device)
        return _qz.quantize_batch(h.unsqueeze(0) if h.dim() == 1 else h)

    def _distances(self, queries, query_positions=None, min_distance: float = 0.0) -> torch.Tensor:
        """(Q, database_size) float32 distances of float32 (quantised first) or uint16 queries."""
        q = self._query_rows(queries)
        if int(q.shape[1]) != self.n_bins:
            raise _lib.NscError(f"the database holds {self.n_bins}-bin rows (got {int(q.shape[1])})")
        qc, qok = quantized_cdf(q)
        n = self.database_size
        qp = dbp = None
        if query_positions is not None:
            qp, dbp = _pos_f32(query_positions, self.device), self._pos[:n]
        return w1_distances_quantized(self._cdf[:n], self._ok[:n], qc, qok, dbp, qp, min_distance)

    def query_batch(self, queries, top_k: int = 10, query_positions=None, min_distance: float = 0.0):
        """(Q, n_bins) queries -> (indices (Q, k) int64, distances (Q, k)) device tensors, ascending, ties to the
        smaller index, k = min(top_k, database_size); ``-1`` / ``+inf`` where fewer than k rows qualify."""
        if self.database_size == 0:
            e = torch.empty((0, 0), device=self.device)
            return e.long(), e
        dist = self._distances(queries, query_positions, min_distance)
        idx, val = _topk(dist, min(top_k, self.database_size))
        return idx.masked_fill_(torch.isinf(val), -1), val

    def query(self, query_hist, top_k: int = 10) -> tuple:
        """(indices (top_k,), distances (top_k,)) as numpy arrays, ascending distance."""
        if self.database_size == 0:
            return np.array([]), np.array([])
        idx, val = self.query_batch(query_hist, top_k)
        return idx[0].cpu().numpy(), val[0].cpu().numpy()

    def clear_database(self):
        self._cdf = self._ok = self._pos = None
        self.database_size = 0
        self.n_noncanonical = 0
