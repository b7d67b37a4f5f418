"""Stage 2 of loop closing on the device -- mirror of the reference's src/retrieval/geometric_verification.py
``GeometricVerifier`` (:48-203), whose ``verify`` calls Open3D 0.18's ``registration_generalized_icp``.

Every candidate pair of a query is registered in one batch by nsc_gicp_register (csrc/nsc_geometry.hip).  The
algorithm follows Open3D's definitions; where Open3D leaves a choice open, the choice below is the contract the
kernels and tests/gicp_restatement.py share.  Parity with Open3D itself is not pinned.

Each pair is a source cloud (the query) and a target cloud (the candidate), (N,3) or (N,4) float32; only xyz is
used and rows with a non-finite coordinate are dropped.

1. Voxel down-sampling (Open3D ``voxel_down_sample``): ``min_bound = min(p) - voxel/2``,
   ``key = floor((p - min_bound) / voxel)``, each voxel becomes the centroid of its points.  Output rows are in the
   order of each voxel's first input row (Open3D's order is arbitrary).  Centroids are exact int64 sums in units of
   2^-24 m, so they do not depend on summation order.
2. Covariances (source and target): the ``covariance_knn`` nearest down-sampled neighbours of each down-sampled
   point, the point itself included, ties to the smaller index; ``C = (1/n) sum (p - mean)(p - mean)^T``, the
   identity if n < 3; then ``C <- U diag(1, 1, epsilon) U^T`` with U the eigenvectors by descending eigenvalue
   (of the identity the axes in order, so the normal is the x axis and the result diag(epsilon, 1, 1)).
3. Evaluation of T (float64): each transformed source point takes the nearest target point at distance
   ``<= max_correspondence_distance`` (ties to the smaller target index); ``fitness = n_corr / n_source``
   (down-sampled), ``rmse = sqrt(sum |d|^2 / n_corr)``, 0 without correspondences.
4. Gauss-Newton update from the correspondences of the current T: ``s' = T s``, ``d = s' - t``,
   ``M = C_t + R C_s R^T``, ``W = M^-1``, ``J = [-[s']x | I]``; solve ``(sum J^T W J) x = -sum J^T W d`` by
   Cholesky in float64; ``x = (alpha, beta, gamma, tx, ty, tz)`` gives dT with ``R = Rz(gamma) Ry(beta) Rx(alpha)``
   and ``T <- dT T``.  Without correspondences, or when the system is not positive definite, dT = I: a pivot counts
   only above 3.9e-9 of its diagonal term (csrc/nsc_gauss_newton.h), so one or two source rows, or collinear ones,
   whose system is singular whatever the weights are, leave T as it is.
5. Loop (Open3D ``RegistrationICP``): evaluate T0; up to ``max_iteration`` times update, then evaluate; stop when
   ``|d fitness| < relative_fitness`` and ``|d rmse| < relative_rmse``.  The last T and its evaluation are returned;
   ``iterations`` counts the updates applied.
6. Information matrix: Open3D's ``GetInformationMatrixFromPointClouds`` at the final T on the down-sampled clouds,
   ``sum G^T G`` with ``G = [-[t]x | I]`` over the correspondences (t the target point), rotation first.
7. Decision: ``verified = n_corr > 0 and fitness >= fitness_threshold and rmse <= rmse_threshold``.

Supported range (include/nsc.h): voxel keys are 21 bits per axis counted from the cloud's min bound and the centroid
sums are int64 in units of 2^-24 m, so a cloud must satisfy ``(max - min) / voxel_size < 2^21`` on every axis over
its finite rows and ``|coordinate| * rows-per-voxel < 2^39`` m.  Outside that range the result is unspecified (voxel
coordinates clamp to 2^21 - 1, so distant rows merge into one voxel; nothing is read or written out of bounds):
one finite stray row at, say, -1e7 m moves the min bound so far that at voxel 0.5 every other row clamps into one
voxel.  Callers drop such rows, or mark them non-finite, before registering.  One call takes at most
MAX_PAIRS_PER_CALL raw pairs, MAX_CLOUDS_PER_CALL clouds to prepare or MAX_PREPARED_PAIRS_PER_CALL stored pairs;
the functions below split larger requests.

GICP is a local method: from the identity it converges for offsets of about the correspondence radius (1 m) or
about 10 degrees of yaw alone, and from further away it can end on the ground plane alone with a fitness that passes
the default thresholds and a transform that is wrong by the whole yaw.  ``TwoStageRetrieval(yaw_init=True)`` covers
any yaw about the vertical axis: it starts every pair from the rotation ``estimate_yaw`` (yaw_alignment.py) reads
off the two range images, good to a few degrees.  It does not cover a translation beyond about 1 m:
``TwoStageRetrieval(planar_init=True)`` does, by searching yaw and planar translation jointly over the structure rows
of the prepared clouds (planar_alignment.py).  For roll and pitch pass ``init_transforms`` (odometry; host arrays or
device tensors).
"""
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import _lib

# Largest batch handed to one library call (include/nsc.h NSC_GICP_MAX_*: the launches index clouds and pairs by
# gridDim.y).  register_packed, register_prepared and PreparedClouds.add_packed split a larger request into several
# calls; a pair or cloud is independent of the rest of its batch, so the results are bit for bit the same.  Module
# constants, so a test can lower them.
MAX_PAIRS_PER_CALL = _lib.GICP_MAX_PAIRS
MAX_CLOUDS_PER_CALL = _lib.GICP_MAX_CLOUDS
MAX_PREPARED_PAIRS_PER_CALL = _lib.GICP_MAX_PREPARED_PAIRS


def _cat_outputs(parts):
    """dicts of per-pair / per-row tensors of consecutive chunks -> one dict"""
    return {k: torch.cat([q[k] for q in parts], 0) for k in parts[0]}


def _params(voxel_size=0.5, max_correspondence_distance=1.0, max_iteration=30, relative_fitness=1e-6,
            relative_rmse=1e-6, covariance_knn=20, epsilon=1e-3):
    return _lib.GicpParams(voxel_size=float(voxel_size), max_correspondence_distance=float(max_correspondence_distance),
                           relative_fitness=float(relative_fitness), relative_rmse=float(relative_rmse),
                           epsilon=float(epsilon), max_iteration=int(max_iteration),
                           covariance_knn=int(covariance_knn))


def _outputs(P, device, system0=False):
    """the tensors one library call over P pairs writes; system0 (P,29) when asked for"""
    f64 = dict(dtype=torch.float64, device=device)
    out = dict(transform=torch.empty((P, 4, 4), **f64), fit_rmse=torch.empty((P, 2), **f64),
               corr_iters=torch.empty((P, 2), dtype=torch.int64, device=device),
               information=torch.empty((P, 6, 6), **f64))
    if system0:
        out["system0"] = torch.empty((P, 29), **f64)
    return out


def _unpacked(out):
    """_outputs after the call: fit_rmse and corr_iters become fitness, rmse, n_correspondences and iterations"""
    fr, ci = out.pop("fit_rmse"), out.pop("corr_iters")
    out.update(fitness=fr[:, 0], rmse=fr[:, 1], n_correspondences=ci[:, 0], iterations=ci[:, 1])
    return out


def _workspace(nbytes, device):
    """the size a *_workspace_bytes query gave -> that many uint8 on ``device`` (one at least)"""
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def register_packed(source_points, source_offsets, target_points, target_offsets, init_transforms, stages=False,
                    **params):
    """Register packed clouds on the device: no host copy, allocation outside torch's allocator or sync, so a call
    can be captured.  ``*_points`` (N, 3|4) float32 device tensors of one stride, ``*_offsets`` (P+1,) int64 device
    tensors, ``init_transforms`` (P,4,4) float64 device tensor.  Returns a dict of device tensors: transform (P,4,4),
    fitness, rmse (P,), n_correspondences, iterations (P,) int64, information (P,6,6); with ``stages=True`` also
    points (Ns+Nt,3), counts (2P,), covariances (Ns+Nt,6) and system0 (P,29) (include/nsc.h NscGicpStages).
    More than MAX_PAIRS_PER_CALL pairs go to the library in several calls (the offsets are then read on the host, so
    such a call cannot be captured, and they must start at 0 and end at the last row); the outputs are those of
    one call, bit for bit."""
    dev = source_points.device
    for t, name in ((source_points, "source_points"), (target_points, "target_points"),
                    (source_offsets, "source_offsets"), (target_offsets, "target_offsets"),
                    (init_transforms, "init_transforms")):
        _lib.require_cuda(t, name)
    stride = int(source_points.shape[1])
    if int(target_points.shape[1]) != stride or source_points.dtype != torch.float32 or \
            target_points.dtype != torch.float32:
        raise _lib.NscError("source and target points must be float32 with the same number of columns (3 or 4)")
    P = int(source_offsets.numel()) - 1
    if int(target_offsets.numel()) - 1 != P or tuple(init_transforms.shape) != (P, 4, 4):
        raise _lib.NscError("offsets and init_transforms must describe the same number of pairs")
    if P > MAX_PAIRS_PER_CALL:
        return _register_packed_chunked(source_points, source_offsets, target_points, target_offsets,
                                        init_transforms, stages, params)
    src, tgt = source_points.contiguous(), target_points.contiguous()
    so, to = source_offsets.contiguous().to(torch.int64), target_offsets.contiguous().to(torch.int64)
    init = init_transforms.contiguous().to(torch.float64)
    Ns, Nt = int(src.shape[0]), int(tgt.shape[0])
    p = _params(**params)
    L = _lib.lib()
    out = _outputs(P, dev, system0=stages)
    st = None
    if stages:
        f64 = dict(dtype=torch.float64, device=dev)
        out.update(points=torch.empty((Ns + Nt, 3), **f64), counts=torch.empty(2 * P, dtype=torch.int64, device=dev),
                   covariances=torch.empty((Ns + Nt, 6), **f64))
        st = _lib.GicpStages(*(out[k].data_ptr() for k in ("points", "counts", "covariances", "system0")))
    ws = _workspace(L.nsc_gicp_workspace_bytes(P, Ns, Nt), dev)
    _lib.call("nsc_gicp_register", dev, src, so, tgt, to, P, Ns, Nt, stride, p, init, out["transform"], out["fit_rmse"],
              out["corr_iters"], out["information"], st, ws, int(ws.numel()), _lib.STREAM)
    return _unpacked(out)


def _register_packed_chunked(source_points, source_offsets, target_points, target_offsets, init_transforms, stages,
                             params):
    """register_packed of more than MAX_PAIRS_PER_CALL pairs: consecutive chunks of pairs, each on the rows its
    offsets name (one read of the offsets to the host), outputs concatenated in the order of the unsplit call."""
    so, to = source_offsets.cpu().tolist(), target_offsets.cpu().tolist()
    P = len(so) - 1
    parts = []
    for a in range(0, P, MAX_PAIRS_PER_CALL):
        b = min(a + MAX_PAIRS_PER_CALL, P)
        parts.append(register_packed(source_points[so[a]:so[b]], source_offsets[a:b + 1] - so[a],
                                     target_points[to[a]:to[b]], target_offsets[a:b + 1] - to[a],
                                     init_transforms[a:b], stages=stages, **params))
    if not stages:
        return _cat_outputs(parts)
    # stage rows: every chunk's source rows, then every chunk's target rows; counts likewise
    rows = [(so[min(a + MAX_PAIRS_PER_CALL, P)] - so[a], min(a + MAX_PAIRS_PER_CALL, P) - a)
            for a in range(0, P, MAX_PAIRS_PER_CALL)]
    out = _cat_outputs([{k: v for k, v in q.items() if k not in ("points", "covariances", "counts")} for q in parts])
    for k in ("points", "covariances"):
        out[k] = torch.cat([q[k][:ns] for q, (ns, _) in zip(parts, rows)] +
                           [q[k][ns:] for q, (ns, _) in zip(parts, rows)], 0)
    out["counts"] = torch.cat([q["counts"][:n] for q, (_, n) in zip(parts, rows)] +
                              [q["counts"][n:] for q, (_, n) in zip(parts, rows)], 0)
    return out


def _xyz(points, device):
    """(N,3) or (N,4) host array or tensor -> (N,3) float32 device tensor"""
    t = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.asarray(points, dtype=np.float32))
    if t.numel() == 0:
        t = t.reshape(0, 3)
    if t.ndim != 2 or t.shape[1] not in (3, 4):
        raise _lib.NscError(f"points must be (N,3) or (N,4), got {tuple(t.shape)}")
    return t[:, :3].to(device=device, dtype=torch.float32).contiguous()


def _pack(clouds, device):
    ts = [_xyz(c, device) for c in clouds]
    off = np.zeros(len(ts) + 1, np.int64)
    off[1:] = np.cumsum([int(t.shape[0]) for t in ts])
    pts = torch.cat(ts, 0) if ts else torch.zeros((0, 3), dtype=torch.float32, device=device)
    return pts, torch.from_numpy(off).to(device)


def _init_tensor(init_transforms, k, device):
    """(k,4,4) initial transforms -- None (the identity), a host array or a tensor (a device tensor is used in
    place: no host visit) -> (k,4,4) float64 tensor on ``device``"""
    if init_transforms is None:
        return torch.eye(4, dtype=torch.float64, device=device).repeat(k, 1, 1)
    t = init_transforms if isinstance(init_transforms, torch.Tensor) else \
        torch.from_numpy(np.ascontiguousarray(np.asarray(init_transforms, np.float64).reshape(k, 4, 4)))
    return t.to(device=device, dtype=torch.float64).reshape(k, 4, 4).contiguous()


def _device(device):
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


class PreparedClouds:
    """A device-resident store of prepared clouds (include/nsc.h NscGicpCloudSet): each cloud's down-sampled points,
    covariances, min bound and voxel index, computed once by nsc_gicp_prepare when the cloud is added.
    ``register_prepared`` then registers pairs given as cloud ids, bit for bit as ``register_packed`` on the raw
    clouds.  The buffers grow by amortised doubling; a cloud takes about 104 bytes per down-sampled row
    (points 24, covariances 48, index 32) plus 48 bytes.  Adding needs room for every input row being a voxel
    of its own, so the buffers are sized for the raw rows of the largest batch added."""

    def __init__(self, voxel_size: float = 0.5, covariance_knn: int = 20, epsilon: float = 1e-3, device="cuda"):
        self.params = dict(voxel_size=float(voxel_size), covariance_knn=int(covariance_knn), epsilon=float(epsilon))
        _params(**self.params)
        self.device = _device(device)
        self._row_host = np.zeros(1, np.int64)          # row offsets of the clouds present (host copy)
        self._n_slots = 0
        self._buf = None

    def __len__(self):
        return len(self._row_host) - 1

    @property
    def n_rows(self) -> int:
        return int(self._row_host[-1])

    @property
    def nbytes(self) -> int:
        """device bytes the store holds (its capacity)"""
        return 0 if self._buf is None else sum(t.numel() * t.element_size() for t in self._buf.values())

    def clear(self):
        """Forget every cloud; the buffers are kept for the next adds."""
        self._row_host = np.zeros(1, np.int64)
        self._n_slots = 0

    def _reserve(self, clouds, rows, slots):
        b = self._buf
        caps = (0, 0, 0) if b is None else (b["bounds"].shape[0], b["points"].shape[0], b["slots"].shape[0])
        if b is not None and clouds <= caps[0] and rows <= caps[1] and slots <= caps[2]:
            return
        nc, nr, ns = (max(need, 2 * cap, least) for need, cap, least in
                      zip((clouds, rows, slots), caps, (64, 1 << 16, 1 << 17)))
        i64 = dict(dtype=torch.int64, device=self.device)
        f64 = dict(dtype=torch.float64, device=self.device)
        nb = dict(row_offsets=torch.zeros(nc + 1, **i64), slot_offsets=torch.zeros(nc + 1, **i64),
                  bounds=torch.zeros((nc, 4), **f64), points=torch.empty((nr, 3), **f64),
                  covariances=torch.empty((nr, 6), **f64), slots=torch.zeros((ns, 2), **i64))
        if b is not None:
            n, r, s = len(self), self.n_rows, self._n_slots
            for k, m in (("row_offsets", n + 1), ("slot_offsets", n + 1), ("bounds", n), ("points", r),
                         ("covariances", r), ("slots", s)):
                nb[k][:m].copy_(b[k][:m])
        self._buf = nb

    def _set(self):
        """the NscGicpCloudSet of the store as it stands"""
        if self._buf is None:
            self._reserve(0, 0, 0)
        b = self._buf
        return _lib.GicpCloudSet(voxel_size=self.params["voxel_size"], epsilon=self.params["epsilon"],
                                 covariance_knn=self.params["covariance_knn"], n_clouds=len(self),
                                 n_rows=self.n_rows, n_slots=self._n_slots, cap_clouds=b["bounds"].shape[0],
                                 cap_rows=b["points"].shape[0], cap_slots=b["slots"].shape[0],
                                 **{k: v.data_ptr() for k, v in b.items()})

    def add_packed(self, points, offsets) -> List[int]:
        """Prepare packed clouds -- ``points`` (N, 3|4) float32 device tensor, ``offsets`` (B+1,) int64 device tensor
        -- in one nsc_gicp_prepare call; one sync to learn the new row and slot totals.  Returns the new ids."""
        _lib.require_cuda(points, "points")
        _lib.require_cuda(offsets, "offsets")
        if points.dtype != torch.float32 or points.ndim != 2 or int(points.shape[1]) not in (3, 4):
            raise _lib.NscError("points must be an (N,3) or (N,4) float32 tensor")
        pts, off = points.contiguous(), offsets.contiguous().to(torch.int64)
        B, N, n = int(off.numel()) - 1, int(pts.shape[0]), len(self)
        if B <= 0:
            return []
        if B > MAX_CLOUDS_PER_CALL:                      # several calls; one read of the offsets to the host
            host, ids = off.cpu().tolist(), []
            for a in range(0, B, MAX_CLOUDS_PER_CALL):
                b = min(a + MAX_CLOUDS_PER_CALL, B)
                ids += self.add_packed(pts[host[a]:host[b]], off[a:b + 1] - host[a])
            return ids
        self._reserve(n + B, self.n_rows + N, self._n_slots + 2 * N)
        st = self._set()
        p = _params(**self.params)
        L = _lib.lib()
        ws = _workspace(L.nsc_gicp_prepare_workspace_bytes(B, N), self.device)
        _lib.call("nsc_gicp_prepare", self.device, pts, off, B, N, int(pts.shape[1]), p, st, ws, int(ws.numel()), _lib.STREAM)
        b = self._buf
        new = torch.cat([b["row_offsets"][n + 1:n + B + 1], b["slot_offsets"][n + B:n + B + 1]]).cpu().numpy()
        self._row_host = np.concatenate([self._row_host, new[:B]])
        self._n_slots = int(new[B])
        return list(range(n, n + B))

    def add(self, clouds: Sequence) -> List[int]:
        """Prepare a list of (N,3|4) host arrays or device tensors in one nsc_gicp_prepare call -> their ids."""
        pts, off = _pack(list(clouds), self.device)
        return self.add_packed(pts, off)

    def cloud(self, i: int):
        """-> {points (m,3), covariances (m,6)}: float64 device views of stored cloud i"""
        if not 0 <= i < len(self):
            raise IndexError(i)
        r0, r1 = int(self._row_host[i]), int(self._row_host[i + 1])
        return dict(points=self._buf["points"][r0:r1], covariances=self._buf["covariances"][r0:r1])

    def packed(self, start: int = 0, stop: Optional[int] = None):
        """The stored clouds ``start`` to ``stop`` (the end, if None) as packed rows -> (points (m,3) float64, offsets
        (stop - start + 1,) int64 counted from 0): device views of the store; the offsets are a tensor of their own (one
        launch) unless the range begins at the store's row 0.  An empty store gives (0,3) rows and the offsets [0]."""
        n = len(self)
        stop = n if stop is None else stop
        if not 0 <= int(start) <= int(stop) <= n:
            raise _lib.NscError(f"start and stop must satisfy 0 <= start <= stop <= {n}, got {start} and {stop}")
        if self._buf is None:
            self._reserve(0, 0, 0)
        r0, r1 = int(self._row_host[int(start)]), int(self._row_host[int(stop)])
        off = self._buf["row_offsets"][int(start):int(stop) + 1]
        return self._buf["points"][r0:r1], off if r0 == 0 else off - r0


def _ids(ids, device):
    t = ids if isinstance(ids, torch.Tensor) else torch.as_tensor(np.asarray(ids, np.int64).reshape(-1))
    return t.to(device=device, dtype=torch.int64).contiguous().reshape(-1)


def register_prepared(sources: PreparedClouds, source_ids, targets: PreparedClouds, target_ids, init_transforms=None,
                      stages=False, **params):
    """Register cloud ``source_ids[i]`` of store ``sources`` onto cloud ``target_ids[i]`` of ``targets`` (ids: device
    int64 tensors or host sequences; the stores may be one).  Returns register_packed's dict of device tensors, bit
    for bit what register_packed gives on the raw clouds; with ``stages=True`` also system0 (P,29).  Nothing is
    synchronised, so a call with device ids and ``init_transforms`` can be captured.  The down-sampling and
    covariance parameters are the stores'; the others default as in register_packed.  A pair whose id is outside
    its store gets NaN transform, fitness, rmse and information, n_correspondences -1 and iterations 0.  More than
    MAX_PREPARED_PAIRS_PER_CALL pairs go to the library in several calls, with the same results."""
    dev = sources.device
    if targets.device != dev:
        raise _lib.NscError("register_prepared: the source and target stores are on different devices")
    p = _params(**{**sources.params, **params})
    sid, tid = _ids(source_ids, dev), _ids(target_ids, dev)
    P = int(sid.numel())
    if int(tid.numel()) != P:
        raise _lib.NscError("register_prepared needs as many target ids as source ids")
    init = _init_tensor(init_transforms, P, dev)
    if P > MAX_PREPARED_PAIRS_PER_CALL:
        step = MAX_PREPARED_PAIRS_PER_CALL
        return _cat_outputs([register_prepared(sources, sid[a:a + step], targets, tid[a:a + step], init[a:a + step],
                                               stages=stages, **params) for a in range(0, P, step)])
    L = _lib.lib()
    out = _outputs(P, dev, system0=stages)
    ss, ts = sources._set(), targets._set()
    ws = _workspace(L.nsc_gicp_register_prepared_workspace_bytes(P), dev)
    _lib.call("nsc_gicp_register_prepared", dev, ss, ts, sid, tid, P, p, init, out["transform"], out["fit_rmse"],
              out["corr_iters"], out["information"], out["system0"] if stages else None, ws, int(ws.numel()), _lib.STREAM)
    return _unpacked(out)


def register_batch(sources: Sequence, targets: Sequence, init_transforms=None, device="cuda", **params):
    """Register sources[i] onto targets[i] for every i in one batch.  Clouds are host arrays or device tensors,
    (N,3) or (N,4); ``init_transforms`` (P,4,4) maps source into target coordinates (identity by default).
    Returns register_packed's dict of device tensors."""
    if len(sources) != len(targets):
        raise _lib.NscError("register_batch needs as many targets as sources")
    dev = _device(device)
    sp, so = _pack(sources, dev)
    tp, to = _pack(targets, dev)
    return register_packed(sp, so, tp, to, _init_tensor(init_transforms, len(sources), dev), **params)


class GeometricVerifier:
    """Geometric verification of loop-closure candidates by Generalized-ICP on the device (geometric_verification.py
    :48-203).

    voxel_size                  0.5   down-sampling voxel edge (m)
    max_correspondence_distance 1.0   correspondence radius (m)
    max_iteration               30    Gauss-Newton updates at most
    relative_fitness            1e-6  convergence: |d fitness| below this ...
    relative_rmse               1e-6  ... and |d rmse| below this
    covariance_knn              20    neighbours per covariance, the point included (<= 32)
    epsilon                     1e-3  plane regularisation of the covariances
    fitness_threshold           0.3   verified needs fitness >= this ...
    rmse_threshold              0.5   ... and rmse <= this (TwoStageRetrieval's own defaults)
    method                      'gicp' (the only method)
    device                      'cuda'
    """

    def __init__(self, voxel_size: float = 0.5, max_correspondence_distance: float = 1.0, max_iteration: int = 30,
                 relative_fitness: float = 1e-6, relative_rmse: float = 1e-6, covariance_knn: int = 20,
                 epsilon: float = 1e-3, fitness_threshold: float = 0.3, rmse_threshold: float = 0.5,
                 method: str = "gicp", device: str = "cuda"):
        if method != "gicp":
            raise _lib.NscError(f"GeometricVerifier: method {method!r} is not supported (only 'gicp')")
        self.params = dict(voxel_size=voxel_size, max_correspondence_distance=max_correspondence_distance,
                           max_iteration=max_iteration, relative_fitness=relative_fitness,
                           relative_rmse=relative_rmse, covariance_knn=covariance_knn, epsilon=epsilon)
        _params(**self.params)
        self.fitness_threshold, self.rmse_threshold = float(fitness_threshold), float(rmse_threshold)
        self.method, self.device = method, device

    def verify(self, query_points, candidate_points, init_transform=None):
        """-> (verified, transform (4,4) float64 mapping query into candidate coordinates, info)"""
        init = None if init_transform is None else np.asarray(init_transform, np.float64).reshape(1, 4, 4)
        return self.verify_batch(query_points, [candidate_points], init)[0]

    def verify_batch(self, query_points, candidate_points_list: List, init_transforms: Optional[np.ndarray] = None):
        """verify() for every candidate of one query in one batch; one host sync when the results come back.
        ``init_transforms`` (k,4,4): a host array or a device tensor (here and in verify_prepared / verify_pairs)."""
        k = len(candidate_points_list)
        if k == 0:
            return []
        dev = _device(self.device)
        q = _xyz(query_points, dev)
        n = int(q.shape[0])
        sp = q.repeat(k, 1)
        so = torch.arange(k + 1, dtype=torch.int64).mul_(n).to(dev)
        tp, to = _pack(candidate_points_list, dev)
        init = _init_tensor(init_transforms, k, dev)
        return self._decide(register_packed(sp, so, tp, to, init, **self.params), k)

    def prepare(self, clouds: Sequence = ()) -> PreparedClouds:
        """A PreparedClouds store with this verifier's down-sampling and covariance parameters, holding ``clouds``."""
        store = PreparedClouds(voxel_size=self.params["voxel_size"], covariance_knn=self.params["covariance_knn"],
                               epsilon=self.params["epsilon"], device=self.device)
        if len(clouds):
            store.add(clouds)
        return store

    def verify_prepared(self, query_store: PreparedClouds, query_id: int, store: PreparedClouds, candidate_ids,
                        init_transforms: Optional[np.ndarray] = None):
        """verify_batch() of stored cloud ``query_id`` against stored clouds ``candidate_ids``: the same list, bit for
        bit, without touching raw points."""
        k = len(candidate_ids)
        return self.verify_pairs(query_store, [int(query_id)] * k, store, candidate_ids, init_transforms)

    def verify_pairs(self, query_store: PreparedClouds, query_ids, store: PreparedClouds, candidate_ids,
                     init_transforms: Optional[np.ndarray] = None):
        """verify() of stored pairs (query_ids[i], candidate_ids[i]) in one register_prepared call and one sync.  The
        stores must have been prepared with this verifier's parameters (else NscError)."""
        k = len(candidate_ids)
        if k == 0:
            return []
        return self._decide(register_prepared(query_store, query_ids, store, candidate_ids, init_transforms,
                                              **self.params), k)

    def _decide(self, out, k):
        """register_* outputs of k pairs -> [(verified, transform, info)]"""
        flat = torch.cat([out["transform"].reshape(k, 16), out["fitness"][:, None], out["rmse"][:, None],
                          out["n_correspondences"][:, None].double(), out["iterations"][:, None].double(),
                          out["information"].reshape(k, 36)], 1).cpu().numpy()      # the one sync
        results = []
        for row in flat:
            nc, fit, rmse = int(row[18]), float(row[16]), float(row[17])
            verified = nc > 0 and fit >= self.fitness_threshold and rmse <= self.rmse_threshold
            info = dict(fitness=fit, rmse=rmse, information_matrix=row[20:56].reshape(6, 6).copy(),
                        n_correspondences=nc, iterations=int(row[19]))
            results.append((bool(verified), row[:16].reshape(4, 4).copy(), info))
        return results
