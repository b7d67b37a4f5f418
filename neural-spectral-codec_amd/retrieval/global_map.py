"""The global voxel map on the device (csrc/nsc_map.hip): the keyframe clouds placed by the optimised poses and merged
into one consistent cloud, one point per occupied voxel.  The consumer of ``PoseGraphOptimizer.optimize``'s poses.

Every accepted closure moves all poses, so the map is not patched: it is rebuilt from the stored clouds each time, in
one pass over their rows.

Definition (the contract nsc_map_build and tests/map_restatement.py share; include/nsc.h), float64:

    input        clouds packed as rows with int64 offsets; float32 rows of 3 or 4 columns (raw clouds) or float64 rows of
                 3 (the points of a ``PreparedClouds``); poses (P,4,4) sensor to world; ``pose_ids`` per cloud, by default
                 cloud c uses pose c; a cloud with an id outside [0, P) is left out and its rows are counted (-1 is the
                 way to leave a cloud out)
    row          w = R p + t; dropped and counted when p or w is not finite
    voxel        k = floor((w - origin) / voxel_size) + 2^20 per axis, dropped and counted (not clamped) outside
                 [0, 2^21): +-524 km at 0.5 m; key = k_x | k_y << 21 | k_z << 42
    per voxel    count, the smallest packed row (first_row), the min and max cloud index (first_cloud, last_cloud),
                 centroid = exact int64 sums of rint(w 2^24), / 2^24 / count
    output       voxels in ascending first_row
    capacity     a table of 2 max_voxels slots; ``complete`` when voxels_found <= max_voxels and rows_unplaced == 0

Integer atomics only: two calls agree bit for bit, and the order of the clouds changes only the order of the voxels.

A check without ground truth that an optimisation helped: a bent trajectory draws every revisited wall twice, so its map
occupies more voxels than a consistent one -- compare ``voxels_found`` before and after.  ``revisited`` marks the voxels
seen from keyframes far apart in the sequence, the places where a closure is what makes the map consistent.

Not part of this module: insertion into a kept table, and ray casting with the removal of what later scans saw through
(``MapLocalizer`` has both, for its distribution map); intensity or colour, meshes.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from .. import _lib
from .geometric_verification import PreparedClouds, _device, _workspace


def revisited(first_cloud, last_cloud, min_gap):
    """The mask of voxels seen from keyframes at least ``min_gap`` apart: ``last_cloud - first_cloud >= min_gap``
    (arrays or tensors, as ``GlobalMap.build`` returns them)."""
    return (last_cloud - first_cloud) >= int(min_gap)


def _tensors(clouds):
    """a sequence of (n,3|4) host arrays or tensors -> a list of (n,3|4) tensors where they are, shapes checked"""
    ts = [c if isinstance(c, torch.Tensor) else torch.from_numpy(np.asarray(c)) for c in clouds]
    for i, t in enumerate(ts):
        if t.numel() == 0:
            ts[i] = t = t.reshape(0, 3)
        if t.ndim != 2 or t.shape[1] not in (3, 4):
            raise _lib.NscError(f"a cloud must be (n,3) or (n,4), got {tuple(t.shape)}")
    return ts


def _pack(ts, device):
    """_tensors' list -> (N,3) rows and (B+1,) int64 offsets on ``device``; float64 rows when every cloud is float64,
    float32 rows otherwise"""
    dtype = torch.float64 if ts and all(t.dtype == torch.float64 for t in ts) else torch.float32
    ts = [t[:, :3].to(device=device, dtype=dtype) for t in ts]
    off = np.zeros(len(ts) + 1, np.int64)
    off[1:] = np.cumsum([int(t.shape[0]) for t in ts])
    pts = torch.cat(ts, 0).contiguous() if ts else torch.zeros((0, 3), dtype=dtype, device=device)
    return pts, torch.from_numpy(off).to(device)


def _is_packed(clouds):
    return isinstance(clouds, tuple) and len(clouds) == 2 and isinstance(clouds[1], torch.Tensor) and clouds[1].ndim == 1


def _host_rows(clouds, poses, device, check):
    """The host form of a call's input -> what its ``*_device`` form takes: ``clouds`` a sequence of (n,3|4) host arrays
    or tensors, or a packed ``(points, offsets)`` pair of device tensors; ``poses`` (P,4,4), host or device.  Returns
    (points, offsets, float64 poses on ``device``, check(number of clouds, number of poses)); ``check`` is where the
    caller refuses what it can on the host, before anything goes to the device."""
    packed = _is_packed(clouds)
    clouds = clouds if packed else _tensors(clouds)
    pose = GlobalMap._poses(poses)
    checked = check(int(clouds[1].numel()) - 1 if packed else len(clouds), int(pose.shape[0]))
    dev = _device(device)
    pts, off = clouds if packed else _pack(clouds, dev)
    return pts, off, pose.to(device=dev, dtype=torch.float64), checked


def _host_clouds(clouds, poses, pose_ids, device):
    """_host_rows for clouds with a pose per id -> (points, offsets, poses, ids); host ids are refused before anything
    goes to the device and stay on the host"""
    return _host_rows(clouds, poses, device, lambda B, P: GlobalMap._host_ids(pose_ids, B, P))


def _host_scans(scans, init_poses, device):
    """_host_rows for scans with one pose each -> (points, offsets, poses, number of scans)"""
    def one_each(S, P):
        if P != S:
            raise _lib.NscError(f"init_poses must have one (4,4) pose per scan ({S}), got {P}")
        return S
    return _host_rows(scans, init_poses, device, one_each)


def _prepared_clouds(store, poses, pose_ids, start=0, stop=None):
    """_host_clouds for the clouds ``start`` to ``stop`` (the end, if None) of a ``PreparedClouds``, on the store's
    device; the caller has checked the range"""
    stop = len(store) if stop is None else stop
    pose = GlobalMap._poses(poses)
    ids = GlobalMap._host_ids(pose_ids, stop - start, int(pose.shape[0]))
    pts, off = store.packed(start, stop)
    return pts, off, pose.to(device=store.device, dtype=torch.float64), ids


_FORMATS = ((torch.float32, 3), (torch.float32, 4), (torch.float64, 3))


def _rows(points, offsets, what):
    """checked packed rows -> (contiguous rows, int64 offsets, number of clouds, number of rows, dtype code)"""
    if points.ndim != 2 or (points.dtype, int(points.shape[1])) not in _FORMATS:
        raise _lib.NscError(f"{what} must be (N,3) or (N,4) float32 or (N,3) float64")
    pts, off = points.contiguous(), offsets.contiguous().to(torch.int64).reshape(-1)
    if int(off.numel()) < 1:
        raise _lib.NscError("offsets must have one entry more than there are clouds")
    return pts, off, int(off.numel()) - 1, int(pts.shape[0]), \
        _lib.MAP_DTYPE_F64 if pts.dtype == torch.float64 else _lib.MAP_DTYPE_F32


_Clouds = namedtuple("_Clouds", "pts off B N dtype pose P ids")


def _clouds(points, offsets, poses, pose_ids):
    """checked device input of a build, an insertion or a removal -> (rows, offsets, clouds, rows, dtype code, float64
    poses, poses, device ids or None)"""
    for t, name in ((points, "points"), (offsets, "offsets"), (poses, "poses")):
        _lib.require_cuda(t, name)
    dev = points.device
    pts, off, B, N, dtype = _rows(points, offsets, "points")
    if poses.ndim != 3 or tuple(poses.shape[1:]) != (4, 4):
        raise _lib.NscError("poses must be (P,4,4)")
    pose = poses.contiguous().to(torch.float64)
    P = int(pose.shape[0])
    ids = GlobalMap._host_ids(pose_ids, B, P)
    if ids is not None:
        ids = ids.to(device=dev, dtype=torch.int64).contiguous().reshape(-1)
        if int(ids.numel()) != B:
            raise _lib.NscError(f"pose_ids must have one entry per cloud ({B}), got {int(ids.numel())}")
    return _Clouds(pts, off, B, N, dtype, pose, P, ids)


def _row_args(c, params, new_poses=None):
    """the arguments every map call starts with (as _lib.call takes them), from _clouds' tuple: the rows, the poses (the
    old and the new of a replacement), the ids and the grid"""
    poses = (c.pose,) if new_poses is None else (c.pose, new_poses)
    return (c.pts, c.dtype, int(c.pts.shape[1]), c.off, c.B, c.N, *poses, c.P, c.ids, params)


def _outputs(shapes, out, device):
    """The output tensors of a ``*_device`` call, name -> (shape, dtype) in ``shapes``: allocated, or the caller's
    ``out``, each checked"""
    if out is None:
        return {k: torch.empty(shape, dtype=dt, device=device) for k, (shape, dt) in shapes.items()}
    for k, (shape, dt) in shapes.items():
        t = out.get(k)
        if t is None or tuple(t.shape) != shape or t.dtype != dt or t.device != device or not t.is_contiguous():
            raise _lib.NscError(f"out[{k!r}] must be a contiguous {shape} {dt} tensor on {device}")
    return out


def _result(out, per_voxel):
    """A call's buffers -> the dict its host form returns, in one read of the stats: per_voxel(n)'s entries for the n
    voxels written, their info columns and keys, the stats by name and ``complete``"""
    stats = dict(zip(_lib.MAP_STAT_NAMES, out["stats"].cpu().tolist()))
    n = stats["voxels_written"]
    info = out["info"][:n]
    res = dict(per_voxel(n), count=info[:, 0], first_row=info[:, 1], first_cloud=info[:, 2], last_cloud=info[:, 3],
               keys=out["keys"][:n], **stats)
    res["complete"] = stats["voxels_found"] == stats["voxels_written"] and stats["rows_unplaced"] == 0
    return res


class GlobalMap:
    """Voxel map of many clouds under a pose per cloud, built by nsc_map_build.

    voxel_size   0.5      voxel edge (m)
    origin       (0,0,0)  world point where voxel (2^20, 2^20, 2^20) begins
    max_voxels   None     capacity of the outputs; the table has twice as many slots.  A voxel of capacity costs 192
                          bytes for the duration of a call (128 of table, 64 of outputs) and a row 0.2 bytes.  None means
                          one voxel per input row, which can never be short: 19 GB for the 10^8 rows of a KITTI-00
                          sized store.  A map has far fewer voxels than rows; give a bound and read ``complete``
    device       'cuda'   there is no CPU fallback
    """

    def __init__(self, voxel_size: float = 0.5, origin=(0.0, 0.0, 0.0), max_voxels=None, device="cuda"):
        origin = tuple(float(v) for v in origin)
        if not (np.isfinite(voxel_size) and voxel_size > 0.0) or len(origin) != 3 or not np.all(np.isfinite(origin)):
            raise _lib.NscError("GlobalMap: voxel_size must be finite and positive and origin three finite numbers")
        if max_voxels is not None and not 0 <= int(max_voxels) <= _lib.MAP_MAX_VOXELS:
            raise _lib.NscError(f"GlobalMap: max_voxels must lie in [0, {_lib.MAP_MAX_VOXELS}]")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.NscError(f"GlobalMap runs on a HIP device (got {dev}); there is no CPU fallback")
        self.params = _lib.MapParams(voxel_size=float(voxel_size), origin=(C.c_double * 3)(*origin))
        self.max_voxels = None if max_voxels is None else int(max_voxels)
        self.device = device

    @staticmethod
    def _host_ids(pose_ids, n_clouds, n_poses):
        """``pose_ids`` as given -> None or a device tensor as they are, host ids as a checked int64 host tensor: one
        entry per cloud, each -1 or an index of ``poses``.  Nothing here touches the device."""
        if pose_ids is None or (isinstance(pose_ids, torch.Tensor) and pose_ids.is_cuda):
            return pose_ids
        host = np.asarray(pose_ids, np.int64).reshape(-1)
        if host.size != n_clouds:
            raise _lib.NscError(f"pose_ids must have one entry per cloud ({n_clouds}), got {host.size}")
        if np.any((host < -1) | (host >= n_poses)):
            raise _lib.NscError(f"pose_ids must be -1 or lie in [0, {n_poses})")
        return torch.from_numpy(host)

    def build_device(self, points, offsets, poses, pose_ids=None, out=None):
        """The map of packed clouds, on the device and without a synchronisation: with device ``pose_ids`` (or none) a
        call can be captured.  ``points`` (N,3|4) float32 or (N,3) float64 device tensor, ``offsets`` (B+1,) int64 device
        tensor, ``poses`` (P,4,4) float64 device tensor.  Returns the full buffers: points (max_voxels,3) float64, info
        (max_voxels,4) int64 = [count, first_row, first_cloud, last_cloud], keys (max_voxels,) int64 and stats
        (``_lib.MAP_STAT_NAMES``) int64; entries past stats[1] = voxels_written are not defined.  ``out``: a dict of
        those four tensors to write into, for a map that is rebuilt after every closure."""
        c = _clouds(points, offsets, poses, pose_ids)
        dev, N = c.pts.device, c.N
        M = N if self.max_voxels is None else self.max_voxels
        out = _outputs(dict(points=((M, 3), torch.float64), info=((M, 4), torch.int64), keys=((M,), torch.int64),
                            stats=((_lib.MAP_STATS,), torch.int64)), out, dev)
        L = _lib.lib()
        ws = _workspace(L.nsc_map_workspace_bytes(N, M), dev)
        _lib.call("nsc_map_build", dev, *_row_args(c, self.params), M, out["points"], out["info"], out["keys"], out["stats"],
                  ws, int(ws.numel()), _lib.STREAM)
        return out

    def _result(self, out):
        """build_device's buffers -> the dict ``build`` returns (one read of the stats)"""
        return _result(out, lambda n: dict(points=out["points"][:n]))

    @staticmethod
    def _poses(poses):
        """(P,4,4) poses, host or device -> a tensor of that shape where it is"""
        t = poses if isinstance(poses, torch.Tensor) else torch.from_numpy(np.asarray(poses, np.float64))
        if t.numel() % 16:
            raise _lib.NscError(f"poses must be (P,4,4), got {tuple(t.shape)}")
        return t.reshape(-1, 4, 4)

    def build(self, clouds, poses, pose_ids=None):
        """The map of ``clouds`` -- a sequence of (n,3|4) host arrays or tensors, or a packed ``(points, offsets)`` pair of
        device tensors -- under ``poses`` (P,4,4), host or device.  Returns device tensors in ascending first_row --
        points (V,3) float64, count, first_row, first_cloud, last_cloud, keys (V,) int64 -- the stats by name
        (voxels_found, voxels_written, rows_used, rows_not_finite, rows_outside, rows_without_pose, rows_unplaced) and
        ``complete``.  One synchronisation, to read the stats."""
        return self._result(self.build_device(*_host_clouds(clouds, poses, pose_ids, self.device)))

    def build_prepared(self, store: PreparedClouds, poses, pose_ids=None):
        """``build`` on the clouds a ``PreparedClouds`` holds: its float64 points and row offsets are the input as they
        stand, so the clouds stage 2 keeps are the map's clouds (one point per voxel of the store's own voxel size)."""
        return self._result(self.build_device(*_prepared_clouds(store, poses, pose_ids)))
