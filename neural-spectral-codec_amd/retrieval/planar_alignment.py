"""Planar initial guess (yaw, x, y) for stage 2 by voting over structure rows (csrc/nsc_planar.hip).

Stage 1 hands stage 2 every keyframe within ``spatial_filter_distance`` of the query; GICP is local and from the
identity converges for about 1 m of offset or 10 degrees of yaw.  ``yaw_init`` closes the heading half of that gap
for scans taken in one place; a column shift of the range image is a yaw only when the two sensors stand in one
place, so it does not survive a translation of a few metres.  This guess searches yaw and planar translation jointly,
on the non-ground rows of the prepared clouds (``PreparedClouds``): the ground rings of a spinning LiDAR are
concentric about each sensor and would vote for zero offset.

Definition (the contract nsc_planar_align and tests/planar_restatement.py share; include/nsc.h), all in float64.

Inputs: two prepared clouds -- ``points`` (m,3) and ``covariances`` (m,6: xx xy xz yy yz zz) -- and a table of H yaw
hypotheses ``(cos theta_h, sin theta_h)``.  Parameters: ``cell`` 0.5 m, ``half_bins`` 24 (1..32), ``z_window`` 0.5 m,
``normal_z2_max`` 0.25, ``source_stride`` 2, ``guard`` 5.

    structure row  (1 - C_zz) < normal_z2_max * (1 - epsilon)     the stored covariance is I - (1 - epsilon) n n^T, so
                   this is n_z^2 < normal_z2_max; a row with fewer than 3 neighbours has the x axis as its normal and
                   is a structure row
    rows taken     source: structure rows whose row index within the cloud is divisible by source_stride
                   target: all structure rows
    per hypothesis h = (c, s), source row a, target row b, every operation rounded on its own, inv_cell = 1 / cell:
        xr = c a.x - s a.y ;  yr = s a.x + c a.y
        bx = floor((b.x - xr) inv_cell + 0.5) ;  by = floor((b.y - yr) inv_cell + 0.5)
        one vote for (h, bx, by) iff |bx| <= half_bins and |by| <= half_bins and |b.z - a.z| <= z_window (inclusive)
    peak_h, bin_h  the largest count of hypothesis h and its bin, ties to the smaller flat index
                   (bx + half_bins) (2 half_bins + 1) + (by + half_bins)
    best           the h of the largest peak_h, ties to the smaller h;  peak = peak_best
    runner_up      the largest peak_h among hypotheses more than guard indices from best, circularly over H; 0 if none
    init           [Rz from (c, s) of best | (bx cell, by cell, 0)]: query into candidate coordinates

With ``peak = 0`` (no structure rows, nothing inside the window) ``best = (-1, 0, 0)`` and ``init`` is the identity.
An id outside its store gives ``best = (-1, 0, 0)``, ``peak = runner_up = -1``, counts 0 and the identity.  The counts
are integers, so the results do not depend on any order and equal the restatement's exactly.

The guess carries no roll, pitch or z offset.  ``planar_support = peak / source rows taken`` is the number that tells
a revisit from another place; GICP's fitness on two ground planes does not.
"""
import math

import numpy as np
import torch

from .. import _lib
from .geometric_verification import PreparedClouds, _cat_outputs, _ids, _workspace

MAX_HALF_BINS = _lib.PLANAR_MAX_HALF_BINS
# Largest batch handed to one nsc_planar_align call (include/nsc.h NSC_PLANAR_MAX_PAIRS: pairs are a grid dimension);
# estimate_planar splits a larger request, with the same results.  A module constant, so a test can lower it.
MAX_PAIRS_PER_CALL = _lib.PLANAR_MAX_PAIRS

_tables = {}             # (device, step) -> the default table on the device: a captured call must not copy from the host


def yaw_table(step_deg: float = 2.0):
    """-> ((H,2) float64 array of (cos, sin) of theta_h = -180 + h * step_deg degrees, h = 0 .. H-1 with
    H = round(360 / step_deg); the (H,) angles in degrees)"""
    H = int(round(360.0 / step_deg))
    deg = np.array([-180.0 + h * step_deg for h in range(H)], np.float64)
    cs = np.array([[math.cos(math.radians(d)), math.sin(math.radians(d))] for d in deg], np.float64).reshape(H, 2)
    return cs, deg


def _params(cell=0.5, half_bins=24, z_window=0.5, normal_z2_max=0.25, source_stride=2, guard=5):
    return _lib.PlanarParams(cell=float(cell), z_window=float(z_window), normal_z2_max=float(normal_z2_max),
                             half_bins=int(half_bins), source_stride=int(source_stride), guard=int(guard))


def _table(yaw_cs, dev):
    if yaw_cs is None:
        key = (str(dev), 2.0)
        if key not in _tables:
            _tables[key] = torch.from_numpy(yaw_table()[0]).to(dev)
        return _tables[key]
    t = yaw_cs if isinstance(yaw_cs, torch.Tensor) else torch.from_numpy(np.asarray(yaw_cs, np.float64))
    if t.ndim != 2 or int(t.shape[1]) != 2 or int(t.shape[0]) < 1:
        raise _lib.NscError(f"yaw_cs must be an (H,2) table of (cos, sin), H >= 1, got {tuple(t.shape)}")
    return t.to(device=dev, dtype=torch.float64).contiguous()


def estimate_planar(sources: PreparedClouds, source_ids, targets: PreparedClouds, target_ids, yaw_cs=None,
                    stages=False, **params):
    """The planar guess of pairs (source_ids[i] of ``sources``, target_ids[i] of ``targets``) in one nsc_planar_align
    call: three launches, no sync, nothing allocated outside torch's allocator, so a call with device ids (and a
    device ``yaw_cs``, or the default table once it has been used on the device) can be captured.  ids: device int64
    tensors or host sequences; ``yaw_cs``: an (H,2) table (``yaw_table()`` by default); ``params``: cell, half_bins,
    z_window, normal_z2_max, source_stride, guard.  Returns a dict of device tensors: best (P,3) int32 = [h, bx, by],
    scores (P,2) int32 = [peak, runner_up], counts (P,2) int32 = [source rows taken, target structure rows],
    init_transforms (P,4,4) float64; with ``stages=True`` also yaw_peaks (P,H,2) and votes (P,H,n,n), n = 2 half_bins
    + 1, int32.  More than MAX_PAIRS_PER_CALL pairs go to the library in several calls, with the same results."""
    dev = sources.device
    if targets.device != dev:
        raise _lib.NscError("estimate_planar: the source and target stores are on different devices")
    p = _params(**params)
    table = _table(yaw_cs, dev)
    H = int(table.shape[0])
    sid, tid = _ids(source_ids, dev), _ids(target_ids, dev)
    P = int(sid.numel())
    if int(tid.numel()) != P:
        raise _lib.NscError("estimate_planar needs as many target ids as source ids")
    if P > MAX_PAIRS_PER_CALL:
        step = MAX_PAIRS_PER_CALL
        return _cat_outputs([estimate_planar(sources, sid[a:a + step], targets, tid[a:a + step], table, stages,
                                             **params) for a in range(0, P, step)])
    i32 = dict(dtype=torch.int32, device=dev)
    out = dict(best=torch.empty((P, 3), **i32), scores=torch.empty((P, 2), **i32), counts=torch.empty((P, 2), **i32),
               init_transforms=torch.empty((P, 4, 4), dtype=torch.float64, device=dev))
    st = None
    if stages:
        n = 2 * p.half_bins + 1
        if not 1 <= p.half_bins <= MAX_HALF_BINS:
            raise _lib.NscError(f"half_bins must be 1..{MAX_HALF_BINS}")
        out.update(yaw_peaks=torch.empty((P, H, 2), **i32), votes=torch.empty((P, H, n, n), **i32))
        st = _lib.PlanarStages(out["yaw_peaks"].data_ptr(), out["votes"].data_ptr())
    L = _lib.lib()
    ss, ts = sources._set(), targets._set()
    ws = _workspace(L.nsc_planar_align_workspace_bytes(P, H), dev)
    _lib.call("nsc_planar_align", dev, ss, ts, sid, tid, P, table, H, p, out["best"], out["scores"], out["counts"],
              out["init_transforms"], st, ws, int(ws.numel()), _lib.STREAM)
    return out


def planar_info(init_transform, peak: int, runner_up: int, taken: int) -> dict:
    """Host values of one pair -> the keys stage 2 adds to a candidate's info: ``init_yaw_deg`` and
    ``init_translation`` (x, y, z of the guess), ``planar_peak``, ``planar_peak_ratio`` (peak / runner_up, inf when
    runner_up <= 0: a ratio near 1 marks an ambiguous pair) and ``planar_support`` (peak / source rows taken, 0 when
    none were taken or the pair is invalid): the votes of the best bin per source row, high for a revisit and low
    for another place."""
    T = np.asarray(init_transform, np.float64).reshape(4, 4)
    peak, runner_up, taken = int(peak), int(runner_up), int(taken)
    return dict(init_yaw_deg=float(np.degrees(np.arctan2(T[1, 0], T[0, 0]))), init_translation=T[:3, 3].copy(),
                planar_peak=peak, planar_peak_ratio=peak / runner_up if runner_up > 0 else float("inf"),
                planar_support=peak / taken if taken > 0 and peak > 0 else 0.0)
