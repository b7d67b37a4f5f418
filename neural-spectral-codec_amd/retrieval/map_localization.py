"""Map localisation on the device (csrc/nsc_map.hip nsc_map_build_dist, csrc/nsc_localize.hip nsc_map_register): a map
that keeps a normal distribution per voxel and a table that outlives the build, and scans registered against it.  The
consumer of ``GlobalMap``'s input: the same clouds under the same optimised poses, kept in a form a scan can be placed in
without adding a keyframe and optimising again.

Definition (the contract the two entry points and tests/map_localize_restatement.py share; include/nsc.h), float64:

    map          rows placed, keyed, counted and ordered exactly as ``GlobalMap`` does.  Per voxel exact int64 moments of
                 q = rint(u 2^16) - 2^15, u the position inside the voxel in [0, 1): mean, covariance C, and the
                 information U diag(1 / max(l_i, eigen_ratio l_max, sigma_floor^2)) U^T of C = U diag(l) U^T.  A voxel
                 is usable with at least ``min_points`` rows
    index        (2 max_voxels, 2) uint64 = (key + 1, place) at the build table's own slots: a lookup walks the probe
                 sequence the insertion walked
    cost         E(T) = sum_i d_i^T Omega_v d_i,  d_i = T p_i - mean_v,  v the voxel that contains T p_i; only that voxel
                 is looked up.  Rows that are not finite, outside the grid or without a usable voxel do not contribute
    rounds       Gauss-Newton on [rotation | translation], J = [-[T p]x | I]; fitness = n_corr / rows,
                 rmse = sqrt(sum |d|^2 / n_corr); Open3D's convergence test; at most max_iteration updates
    insertion    (nsc_map_insert_dist) a map built ``insertable`` keeps its int64 moments and a cursor [rows, clouds taken
                 so far]; new clouds are added to the kept tensors in work proportional to their rows, and the map is
                 then, bit for bit, the map a build over all clouds would give.  Rows and clouds of an insertion are
                 numbered on from the cursor; poses and ``pose_ids`` are indexed within the call
    removal      (nsc_map_remove_dist) a removal is matched when every row it is given was added earlier with the same
                 bits of xyz and of its pose.  The row finds its voxel by the build's probe and its nine integers and its
                 count are subtracted, in work proportional to the rows.  After any sequence of builds, insertions,
                 matched removals and replacements the map holds, for every voxel of a build over the rows that remain,
                 that build's count, moments and record by bits, and ``register`` gives the bits it gives against that
                 build.  Every other keyed voxel is emptied: count 0, zero moments, a record of 16 zeros, not usable; it
                 keeps its key and its place, and a later insertion fills it again.  first_row stays the row that made the
                 voxel, first_cloud and last_cloud become bounds; ``rows_used`` goes down by the rows removed.  A voxel
                 whose count ends below 0, or at 0 with a moment left, is inconsistent (an unmatched removal): it gets
                 the zero record and is counted in ``removed``
    replacement  (nsc_map_replace_dist) clouds removed under ``old_poses`` and inserted under ``new_poses`` in one call;
                 rows and clouds are numbered from ``first_row`` and ``first_cloud``, the cursor stays as it is, and what
                 became of the rows goes into ``placed``.  ``update_prepared`` is the call to make after
                 ``PoseGraphOptimizer.optimize``: it chooses the clouds whose poses moved, on the device
    resize       (nsc_map_rehash_dist; ``resize*``, ``fit``) the kept map moved to another capacity, with or without its
                 emptied voxels, in one pass over its voxels: count, moments, key and record are copied by bits, the kept
                 voxels take the places 0, 1, ... in their old order (ascending first_row survives), and a new index is keyed
                 by the build's probe.  No row is read, so the clouds need not exist any more.  While the voxels kept fit
                 into the new capacity the result is, bit for bit, the build at that capacity over the rows the map holds
                 (after a compaction: voxel by voxel, under places of its own), and ``register`` gives the same bits before
                 and after.  A destination that is too small follows the build's overflow rule: the kept voxels in front
                 take the places, the others keep their key with place ~0.  ``new_place`` tells a caller who keeps side data
                 by place where every old place went.  An inconsistent voxel is kept with its integers
    seen through (nsc_map_cast_rays, nsc_map_flag_rows; ``observe*``, ``seen_through``, ``flag_rows_device``, ``carve*``)
                 the ray from a cloud's sensor (its pose's translation) to each of its placed rows is walked through the
                 grid from ``ray_min_range`` to ``ray_end_margin`` in front of the row, ``ray_max_range`` at most, the next
                 face recomputed from the voxel at every step.  A usable voxel other than the row's own is crossed when the
                 segment inside it comes within ``ray_gate`` standard deviations of the voxel's own Gaussian
                 (x^T Omega x <= gate^2 at the closest point): a ray that merely runs through the box of a floor voxel,
                 beside the floor, does not count.  ``crossed`` counts crossings per place and accumulates; a voxel is seen
                 through with count > 0, crossed >= ``min_crossings`` and crossed >= ``crossing_ratio`` x count.  Carving
                 removes the rows of given clouds that lie in such voxels, as a matched removal of the clouds with every
                 other row made NaN, and the map is then, bit for bit, the build over the rows kept

    robust      (nsc_map_register_robust; ``kernel``, ``robust_scale``, ``neighbours``) every pair (row, voxel) is weighted
                 by w = rho'(s), s = d^T Omega_v d, with the pose graph's kernels and one width c in units of sqrt(chi^2):
                 H = sum w J^T Omega J, g = sum w J^T Omega d, cost = sum rho(s), rmse = sqrt(sum w |d|^2 / sum w).  With
                 ``neighbours=7`` a row pairs with its own voxel and the six face neighbours, in the fixed order
                 (0, -x, +x, -y, +y, -z, +z); n_correspondences counts rows with at least one pair, n_pairs the pairs.
                 Geman-McClure refines from a good start (clutter in front of walls); Cauchy with seven voxels widens the
                 basin (starts a metre off at 0.5 m voxels).  Seven voxels without a kernel bias the result: a far voxel
                 pulls at full weight

Integer atomics and fixed-shape float64 sums only: two calls agree bit for bit and a scan's result does not depend on what
else is in the batch.

Not part of this module: source covariances (full VGICP), 27-voxel neighbourhoods, a width per scan, a step-acceptance
test, NDT's exponential score, detection of an unmatched removal that leaves a positive count, a resize in place or one
that ``extend`` starts by itself (it would need a read-back), unary edges in the pose graph.
"""

import numpy as np
import torch

from .. import _lib
from .geometric_verification import PreparedClouds, _workspace
from .global_map import (GlobalMap, _clouds, _host_clouds, _host_rows, _host_scans, _outputs, _prepared_clouds, _result,
                         _row_args, _rows)


class MapLocalizer:
    """A distribution voxel map built by nsc_map_build_dist and scans registered against it by nsc_map_register.

    voxel_size        1.0      voxel edge (m)
    origin            (0,0,0)  world point where voxel (2^20, 2^20, 2^20) begins
    max_voxels        None     capacity of the map; the build table has twice as many slots.  A voxel of capacity costs
                               256 bytes of table during the build and 200 bytes kept (record 128, index 32, info and key
                               40).  None means one voxel per input row of the first build, which can never be short
                               for that build; ``fit`` then gives back what the voxels do not need, and ``resize*`` sets
                               any other capacity later
    min_points        6        rows a voxel needs to take part in a registration
    eigen_ratio       1e-2     smallest eigenvalue of a voxel's covariance, as a share of its largest
    sigma_floor       1e-3     smallest standard deviation of a voxel along any axis (m)
    max_iteration     30       Gauss-Newton updates at most
    relative_fitness  1e-6     a scan is finished when fitness and rmse both change by less than these
    relative_rmse     1e-6
    device            'cuda'   there is no CPU fallback
    insertable        False    every build keeps ``moments`` (M,9) and ``cursor`` (2,) int64 = [rows, clouds taken so
                               far], so that ``insert*`` and ``extend`` can add scans to the kept map, and ``remove*``,
                               ``replace*`` and ``update_prepared`` take clouds out or move them.  The capacity does
                               not grow by itself: with ``max_voxels=None`` it is the first build's row count.  ``resize*``
                               moves the map to a larger one, and leaves behind the voxels that removals emptied, before
                               it fills up: a voxel found past the capacity (voxels_found > voxels_written) never had a
                               record, cannot be carried and is counted in ``source_keys_unplaced``
    kernel            None     robust kernel of the registration: None (quadratic), "huber", "cauchy" or "geman_mcclure"
    robust_scale      None     the kernel's width c, in units of sqrt(chi^2); needed with a kernel, refused without one
    neighbours        1        voxels a row is paired with: 1 (its own) or 7 (and the six face neighbours)
    ray_min_range     0.0      ``observe*``: a ray is walked from this far off its sensor (m)
    ray_max_range     60.0     to this far at most (m; at most ``_lib.MAP_RAY_MAX_REACH`` voxels)
    ray_end_margin    None     and to this far in front of its row (m); None: one voxel edge
    ray_gate          3.0      a ray crosses a voxel within this many standard deviations of its Gaussian
    min_crossings     3        a voxel is seen through with at least this many crossings
    crossing_ratio    0.5      and at least this many per row it holds

    With the defaults ``register*`` and ``extend`` call nsc_map_register; with a kernel or seven voxels they call
    nsc_map_register_robust, and ``extend`` still gates on ``fitness``.

    After a build the instance keeps ``voxels`` (M,16), ``index`` (2M,2), ``keys`` (M,), ``info`` (M,4), ``stats`` (7,)
    as device tensors over the full capacity M and, after ``build``, ``build_prepared``, ``insert`` or
    ``insert_prepared``, ``complete`` (``build_device``, ``insert_device`` and ``extend`` read nothing back:
    ``complete`` is then None).
    """

    def __init__(self, voxel_size: float = 1.0, origin=(0.0, 0.0, 0.0), max_voxels=None, min_points: int = 6,
                 eigen_ratio: float = 1e-2, sigma_floor: float = 1e-3, max_iteration: int = 30,
                 relative_fitness: float = 1e-6, relative_rmse: float = 1e-6, device="cuda", insertable: bool = False,
                 kernel=None, robust_scale=None, neighbours: int = 1, ray_min_range: float = 0.0,
                 ray_max_range: float = 60.0, ray_end_margin=None, ray_gate: float = 3.0, min_crossings: int = 3,
                 crossing_ratio: float = 0.5):
        self._grid = GlobalMap(voxel_size, origin, max_voxels, device)       # its refusals are this class's
        margin = -1.0 if ray_end_margin is None else ray_end_margin
        if not (all(np.isfinite(v) for v in (ray_min_range, ray_max_range, margin, ray_gate)) and
                float(ray_min_range) >= 0.0 and float(ray_max_range) > 0.0 and float(ray_gate) > 0.0 and
                (ray_end_margin is None or float(margin) >= 0.0)):
            raise _lib.NscError("MapLocalizer: finite ray ranges with ray_min_range >= 0, ray_max_range > 0, "
                                "ray_end_margin >= 0 or None, and ray_gate > 0")
        if float(ray_max_range) / float(voxel_size) > _lib.MAP_RAY_MAX_REACH:
            raise _lib.NscError(f"MapLocalizer: ray_max_range reaches at most {_lib.MAP_RAY_MAX_REACH} voxels")
        if int(min_crossings) < 1 or not (np.isfinite(crossing_ratio) and float(crossing_ratio) > 0.0):
            raise _lib.NscError("MapLocalizer: min_crossings >= 1 and a finite positive crossing_ratio")
        self.ray = _lib.MapRayParams(min_range=float(ray_min_range), max_range=float(ray_max_range),
                                     end_margin=float(margin), gate=float(ray_gate))
        self.min_crossings, self.crossing_ratio = int(min_crossings), float(crossing_ratio)
        if kernel not in _lib.MAP_KERNELS:
            raise _lib.NscError(f"MapLocalizer: unknown kernel {kernel!r}")
        if neighbours not in (1, 7):
            raise _lib.NscError(f"MapLocalizer: neighbours is 1 or 7, got {neighbours!r}")
        if kernel is None and robust_scale is not None:
            raise _lib.NscError("MapLocalizer: robust_scale is the width of a kernel; give one")
        if kernel is not None and not (robust_scale is not None and np.isfinite(robust_scale) and
                                       float(robust_scale) > 0.0):
            raise _lib.NscError(f"MapLocalizer: kernel {kernel!r} needs a finite positive robust_scale")
        self.robust = _lib.MapRobustParams(kernel=_lib.MAP_KERNELS[kernel], neighbours=int(neighbours),
                                           scale=0.0 if kernel is None else float(robust_scale))
        if int(min_points) < 1 or not 0.0 < float(eigen_ratio) <= 1.0 or \
                not (np.isfinite(sigma_floor) and float(sigma_floor) > 0.0):
            raise _lib.NscError("MapLocalizer: min_points >= 1, eigen_ratio in (0, 1] and a finite positive sigma_floor")
        if int(max_iteration) < 0 or not float(relative_fitness) >= 0.0 or not float(relative_rmse) >= 0.0:
            raise _lib.NscError("MapLocalizer: max_iteration, relative_fitness and relative_rmse must not be negative")
        self.params = self._grid.params
        self.dist = _lib.MapDistParams(min_points=int(min_points), reserved=0, eigen_ratio=float(eigen_ratio),
                                       sigma_floor=float(sigma_floor))
        self.reg = _lib.MapRegisterParams(max_iteration=int(max_iteration), reserved=0,
                                          relative_fitness=float(relative_fitness), relative_rmse=float(relative_rmse))
        self.max_voxels = self._grid.max_voxels
        self.device = device
        self.insertable = bool(insertable)
        self.voxels = self.index = self.keys = self.info = self.stats = self.moments = self.cursor = None
        self.crossed = None                  # (M,) int64 crossings per place, from the first ``observe*`` on
        self.complete = None
        self.capacity = None

    # ---- the map ------------------------------------------------------------------------------------------------------

    def build_device(self, points, offsets, poses, pose_ids=None, out=None, moments=False):
        """The map of packed clouds, on the device and without a synchronisation: with device ``pose_ids`` (or none) a
        call can be captured.  Arguments as ``GlobalMap.build_device``.  Returns, and keeps, the full buffers: voxels
        (M,16) float64, index (2M,2) uint64 stored as int64, info (M,4) int64, keys (M,) int64, stats (7,) int64 and, with
        ``moments=True``, moments (M,9) int64; entries of voxels, info, keys and moments past stats[1] are not defined.
        An insertable map always keeps moments, and cursor (2,) int64, set to this build's rows and clouds by two fills.
        ``out``: a dict of those tensors to write into."""
        dev = points.device
        c = _clouds(points, offsets, poses, pose_ids)
        B, N = c.B, c.N
        M = N if self.max_voxels is None else self.max_voxels
        keeps_moments = moments or self.insertable or (out is not None and "moments" in out)
        out = _outputs(self._shapes(M, keeps_moments, self.insertable), out, dev)
        L = _lib.lib()
        ws = _workspace(L.nsc_map_dist_workspace_bytes(N, M), dev)
        _lib.call("nsc_map_build_dist", dev, *_row_args(c, self.params), self.dist, M, out["voxels"], out["index"],
                  out["info"], out["keys"], out.get("moments"), out["stats"], ws, int(ws.numel()), _lib.STREAM)
        self._keep(out, M, out.get("moments"), out.get("cursor") if self.insertable else None)
        if self.cursor is not None:
            self.cursor[0].fill_(N)
            self.cursor[1].fill_(B)
        if self.crossed is not None:                                     # the places are new: what was seen through them is not
            self.crossed = self.crossed.fill_(0) if int(self.crossed.numel()) == M else None
        return out

    @staticmethod
    def _shapes(M, moments, cursor):
        """name -> (shape, dtype) of the kept tensors of a map of capacity M"""
        shapes = dict(voxels=((M, _lib.MAP_VOXEL_DOUBLES), torch.float64), index=((2 * M, 2), torch.int64),
                      info=((M, 4), torch.int64), keys=((M,), torch.int64), stats=((_lib.MAP_STATS,), torch.int64))
        if moments:
            shapes["moments"] = ((M, 9), torch.int64)
        if cursor:
            shapes["cursor"] = ((2,), torch.int64)
        return shapes

    def _keep(self, out, M, moments, cursor):
        """the kept tensors are ``out``'s from here on, over the capacity M"""
        self.voxels, self.index, self.keys, self.info, self.stats = (out[k] for k in ("voxels", "index", "keys", "info",
                                                                                     "stats"))
        self.moments, self.cursor = moments, cursor
        self.capacity, self.complete = M, None

    # ---- insertion ----------------------------------------------------------------------------------------------------

    def _kept(self):
        return {k: getattr(self, k) for k in ("voxels", "index", "info", "keys", "moments", "stats", "cursor")}

    def _kept_args(self):
        """the arguments of the kept map (as _lib.call takes them), as every call on it takes them after the rows"""
        return (self.dist, self.capacity, self.voxels, self.index, self.info, self.keys, self.moments, self.stats)

    def _insertable_map(self, what):
        """the host-side refusals every insertion starts with"""
        if self.voxels is None:
            raise _lib.NscError(f"MapLocalizer.{what}: build a map first")
        if not self.insertable or self.moments is None or self.cursor is None:
            raise _lib.NscError(f"MapLocalizer.{what}: the map was not built insertable (MapLocalizer(insertable=True))")

    def insert_device(self, points, offsets, poses, pose_ids=None):
        """Add packed clouds to the kept map (nsc_map_insert_dist), on the device and without a synchronisation: with
        device ``pose_ids`` (or none) a call can be captured, and every replay is a further insertion of what the buffers
        then hold.  Arguments as ``build_device``; poses and ``pose_ids`` are indexed within the call, rows and clouds are
        numbered on from ``cursor``.  The kept tensors are then those of a build over all clouds so far with the same
        capacity, bit for bit.  Returns the kept tensors (``build_device``'s dict and cursor); nothing is read back and
        ``complete`` is None."""
        self._insertable_map("insert_device")
        dev = self.voxels.device
        if points.device != dev:
            raise _lib.NscError(f"the scans must be on the map's device ({dev})")
        c = _clouds(points, offsets, poses, pose_ids)
        L = _lib.lib()
        ws = _workspace(L.nsc_map_insert_workspace_bytes(c.N), dev)
        _lib.call("nsc_map_insert_dist", dev, *_row_args(c, self.params), *self._kept_args(), self.cursor, ws,
                  int(ws.numel()), _lib.STREAM)
        self.complete = None
        return self._kept()

    def insert(self, clouds, poses, pose_ids=None):
        """``insert_device`` on the input forms of ``build``.  Returns ``build``'s dict over the whole map; one
        synchronisation, to read the stats."""
        self._insertable_map("insert")
        return self._result(self.insert_device(*_host_clouds(clouds, poses, pose_ids, self.voxels.device)))

    def insert_prepared(self, store: PreparedClouds, poses, pose_ids=None, start=0):
        """``insert`` on the clouds of a ``PreparedClouds`` from index ``start`` on: the clouds added to the store since
        the map was built or last extended.  ``poses`` and ``pose_ids`` have one entry per inserted cloud."""
        self._insertable_map("insert_prepared")
        n = len(store)
        if not 0 <= int(start) <= n:
            raise _lib.NscError(f"start must lie in [0, {n}], got {start}")
        return self._result(self.insert_device(*_prepared_clouds(store, poses, pose_ids, int(start))))

    def extend(self, scans, init_poses, min_fitness: float):
        """Register ``scans`` (as ``register`` takes them) and insert those whose fitness reaches ``min_fitness`` under
        their registered transforms: the map grows with the vehicle.  The choice is made on the device --
        pose_ids = where(fitness >= min_fitness, scan, -1) -- so nothing is read back and, with packed device scans, the
        pair of calls can be captured; the rows of the other scans are counted in rows_without_pose.  Returns
        ``register_device``'s dict."""
        self._insertable_map("extend")
        dev = self.voxels.device
        pts, off, pose, S = _host_scans(scans, init_poses, dev)
        out = self.register_device(pts, off, pose)
        scan = torch.arange(S, dtype=torch.int64, device=dev)
        ids = torch.where(out["fitness"] >= float(min_fitness), scan, -1)         # four launches: arange, >=, the -1 (a fill), where
        self.insert_device(pts, off, out["transform"], ids)
        return out

    # ---- removal and re-placing --------------------------------------------------------------------------------------

    def remove_device(self, points, offsets, poses, pose_ids=None):
        """Take packed clouds out of the kept map (nsc_map_remove_dist), on the device and without a synchronisation:
        with device ``pose_ids`` (or none) a call can be captured.  Arguments as ``insert_device``; the removal is matched
        when every row was added earlier with the same bits of xyz and of its pose, and the map is then, voxel by voxel,
        the build over the rows that remain (include/nsc.h).  Returns the kept tensors and ``removed`` (8,) int64
        (``_lib.MAP_REMOVE_STAT_NAMES``); nothing is read back and ``complete`` is None."""
        self._insertable_map("remove_device")
        dev = self.voxels.device
        if points.device != dev:
            raise _lib.NscError(f"the clouds must be on the map's device ({dev})")
        c = _clouds(points, offsets, poses, pose_ids)
        L = _lib.lib()
        ws = _workspace(L.nsc_map_remove_workspace_bytes(c.N), dev)
        removed = torch.empty((_lib.MAP_REMOVE_STATS,), dtype=torch.int64, device=dev)
        _lib.call("nsc_map_remove_dist", dev, *_row_args(c, self.params), *self._kept_args(), removed, ws, int(ws.numel()),
                  _lib.STREAM)
        self.complete = None
        return dict(self._kept(), removed=removed)

    def _removed(self, out):
        """remove_device's or replace_device's dict -> ``_result``'s dict and the eight counts by name"""
        removed = out["removed"]
        res = self._result(out)                                  # the one synchronisation
        res.update(zip(_lib.MAP_REMOVE_STAT_NAMES, removed.cpu().tolist()))
        return res

    def remove(self, clouds, poses, pose_ids=None):
        """``remove_device`` on the input forms of ``build``.  Returns ``build``'s dict over the whole map (emptied voxels
        included: count 0, not usable) and the eight counts of ``removed`` by name; one synchronisation."""
        self._insertable_map("remove")
        return self._removed(self.remove_device(*_host_clouds(clouds, poses, pose_ids, self.voxels.device)))

    def remove_prepared(self, store: PreparedClouds, poses, pose_ids=None, start=0, stop=None):
        """``remove`` on the clouds ``start`` to ``stop`` (the end, if None) of a ``PreparedClouds``, under the poses they
        were placed by.  ``poses`` and ``pose_ids`` have one entry per cloud of that range."""
        self._insertable_map("remove_prepared")
        n = len(store)
        stop = n if stop is None else stop
        if not 0 <= int(start) <= int(stop) <= n:
            raise _lib.NscError(f"start and stop must satisfy 0 <= start <= stop <= {n}, got {start} and {stop}")
        return self._removed(self.remove_device(*_prepared_clouds(store, poses, pose_ids, int(start), int(stop))))

    def replace_device(self, points, offsets, old_poses, new_poses, pose_ids=None, first_row=0, first_cloud=0):
        """Move packed clouds of the kept map from ``old_poses`` to ``new_poses`` (nsc_map_replace_dist; both (P,4,4)), on
        the device and without a synchronisation: cloud c is removed under old_poses[pose_ids[c]] and inserted under
        new_poses[pose_ids[c]], a cloud with id -1 is left alone.  Rows and clouds are numbered from ``first_row`` and
        ``first_cloud`` (the place of ``points`` in the store the map was built from), and ``cursor`` is neither read
        nor advanced.  Returns the kept tensors, ``removed`` (8,) and ``placed`` (7,) int64: what became of the call's rows
        in the layout of ``stats`` (new voxels, written after the call, used, not finite, outside, without pose,
        unplaced)."""
        self._insertable_map("replace_device")
        dev = self.voxels.device
        if points.device != dev:
            raise _lib.NscError(f"the clouds must be on the map's device ({dev})")
        if int(first_row) < 0 or int(first_cloud) < 0:
            raise _lib.NscError(f"first_row and first_cloud must not be negative, got {first_row} and {first_cloud}")
        _lib.require_cuda(new_poses, "new_poses")
        c = _clouds(points, offsets, old_poses, pose_ids)
        P = c.P
        if new_poses.ndim != 3 or tuple(new_poses.shape) != (P, 4, 4):
            raise _lib.NscError(f"new_poses must be ({P},4,4) as old_poses, got {tuple(new_poses.shape)}")
        new = new_poses.contiguous().to(torch.float64)
        L = _lib.lib()
        ws = _workspace(L.nsc_map_replace_workspace_bytes(c.N), dev)
        removed = torch.empty((_lib.MAP_REMOVE_STATS,), dtype=torch.int64, device=dev)
        placed = torch.empty((_lib.MAP_STATS,), dtype=torch.int64, device=dev)
        _lib.call("nsc_map_replace_dist", dev, *_row_args(c, self.params, new), *self._kept_args(), int(first_row),
                  int(first_cloud), removed, placed, ws, int(ws.numel()), _lib.STREAM)
        self.complete = None
        return dict(self._kept(), removed=removed, placed=placed)

    def replace(self, clouds, old_poses, new_poses, pose_ids=None, first_row=0, first_cloud=0):
        """``replace_device`` on the input forms of ``build``.  Returns ``remove``'s dict and ``placed`` (7,) as a device
        tensor; one synchronisation."""
        self._insertable_map("replace")
        def check(B, P):                          # after the clouds and old_poses, and before anything goes to the device
            new = GlobalMap._poses(new_poses)
            if P != int(new.shape[0]):
                raise _lib.NscError(f"old_poses and new_poses must have one pose each per id, got {P} and "
                                    f"{int(new.shape[0])}")
            if int(first_row) < 0 or int(first_cloud) < 0:
                raise _lib.NscError(f"first_row and first_cloud must not be negative, got {first_row} and {first_cloud}")
            return GlobalMap._host_ids(pose_ids, B, P), new
        dev = self.voxels.device
        pts, off, old, (ids, new) = _host_rows(clouds, old_poses, dev, check)
        out = self.replace_device(pts, off, old, new.to(device=dev, dtype=torch.float64), ids, first_row, first_cloud)
        return dict(self._removed(out), placed=out["placed"])

    def update_prepared(self, store: PreparedClouds, old_poses, new_poses, min_translation: float = 0.0,
                        min_rotation: float = 0.0):
        """Make the kept map follow the pose graph: after ``PoseGraphOptimizer.optimize`` has moved keyframes from
        ``old_poses`` to ``new_poses`` (one (4,4) pose per cloud of ``store``, the map's input), re-place the clouds that
        moved.  A cloud is re-placed when its two poses differ in any of the twelve entries, both are finite, and
        |t_new - t_old| >= ``min_translation`` (m) or the angle of R_old^T R_new (atan2 of the skew part's norm and
        (trace - 1) / 2, as the pose graph's Log) >= ``min_rotation`` (rad).  A cloud below both thresholds stays under its
        old pose: the caller keeps the poses the map holds, which are ``new_poses`` where ``moved`` >= 0 and
        ``old_poses`` elsewhere.  The choice is made on the device into ``pose_ids``, as ``extend`` does, so nothing is
        read back and the call can be captured.  Rows and clouds keep the store's numbering.  Returns
        ``replace_device``'s dict and ``moved`` (clouds,) int64: the cloud's own number, or -1.
        A replacement is two scattered-atomic passes over the moved clouds' rows and costs about two insertions of them
        (measured 1.85).  On the map of profiles/map_localize.md (4 541 clouds, 90.8 M rows) re-placing every second cloud
        took what ``build_prepared`` over all of them takes (44.9 ms each): from about half of all clouds moved a rebuild is
        cheaper.  The call walks the whole store to find the rows that moved (3.0 ms there for 64 moved clouds);
        ``replace_device`` on a contiguous range of clouds with its ``first_row`` and ``first_cloud`` pays for that range
        alone."""
        self._insertable_map("update_prepared")
        n = len(store)
        old, new = GlobalMap._poses(old_poses), GlobalMap._poses(new_poses)
        if int(old.shape[0]) != n or int(new.shape[0]) != n:          # refused before anything goes to the device
            raise _lib.NscError(f"old_poses and new_poses must have one (4,4) pose per cloud of the store ({n}), got "
                                f"{int(old.shape[0])} and {int(new.shape[0])}")
        if not (float(min_translation) >= 0.0 and float(min_rotation) >= 0.0):
            raise _lib.NscError("min_translation and min_rotation must not be negative")
        dev = store.device
        old, new = old.to(device=dev, dtype=torch.float64), new.to(device=dev, dtype=torch.float64)
        A, B = old[:, :3, :], new[:, :3, :]
        differ = (A != B).flatten(1).any(1)
        finite = torch.isfinite(A).flatten(1).all(1) & torch.isfinite(B).flatten(1).all(1)
        D = (A[:, :, :3].unsqueeze(3) * B[:, :, :3].unsqueeze(2)).sum(1)      # R_old^T R_new, elementwise: no BLAS call to capture
        v = 0.5 * torch.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], 1)
        angle = torch.atan2(v.norm(dim=1), 0.5 * (D[:, 0, 0] + D[:, 1, 1] + D[:, 2, 2] - 1.0))
        far = ((B[:, :, 3] - A[:, :, 3]).norm(dim=1) >= float(min_translation)) | (angle >= float(min_rotation))
        moved = torch.where(differ & finite & far, torch.arange(n, dtype=torch.int64, device=dev), -1)
        out = self.replace_device(*store.packed(), old, new, moved, 0, 0)
        out["moved"] = moved
        return out

    # ---- seen-through voxels: ray casting and carving ----------------------------------------------------------------

    def _observable(self, what, points):
        if self.voxels is None:
            raise _lib.NscError(f"MapLocalizer.{what}: build a map first")
        if points.device != self.voxels.device:
            raise _lib.NscError(f"the clouds must be on the map's device ({self.voxels.device})")
        if self.crossed is None:
            self.crossed = torch.zeros((self.capacity,), dtype=torch.int64, device=self.voxels.device)

    def observe_device(self, points, offsets, poses, pose_ids=None):
        """Cast the rays of packed clouds through the kept map (nsc_map_cast_rays), on the device and without a
        synchronisation: the ray of a row runs from its cloud's sensor, poses[id][:3, 3], to the placed row, and every
        usable voxel it passes within ``ray_gate`` standard deviations of, before ``ray_end_margin`` in front of its end,
        counts one crossing (include/nsc.h).  Arguments as ``build_device``.  The crossings are ADDED to ``crossed`` (M,)
        int64, which is made of zeros by the first call and zeroed by every build and every ``carve*``.  The map is only
        read.  Returns crossed and ray_stats (8,) int64 (``_lib.MAP_RAY_STAT_NAMES``), written anew by every call."""
        self._observable("observe_device", points)
        dev = self.voxels.device
        c = _clouds(points, offsets, poses, pose_ids)
        ray_stats = torch.empty((_lib.MAP_RAY_STATS,), dtype=torch.int64, device=dev)
        _lib.call("nsc_map_cast_rays", dev, *_row_args(c, self.params), self.voxels, self.index, self.capacity, self.ray,
                  self.crossed, ray_stats, _lib.STREAM)
        return dict(crossed=self.crossed, ray_stats=ray_stats)

    @staticmethod
    def _observed(out):
        """observe_device's dict -> the eight counts by name (the one synchronisation)"""
        return dict(zip(_lib.MAP_RAY_STAT_NAMES, out["ray_stats"].cpu().tolist()))

    def observe(self, clouds, poses, pose_ids=None):
        """``observe_device`` on the input forms of ``build``.  Returns the eight counts of ray_stats by name; one
        synchronisation."""
        if self.voxels is None:
            raise _lib.NscError("MapLocalizer.observe: build a map first")
        return self._observed(self.observe_device(*_host_clouds(clouds, poses, pose_ids, self.voxels.device)))

    def _store_range(self, what, store, start, stop):
        n = len(store)
        stop = n if stop is None else stop
        if not 0 <= int(start) <= int(stop) <= n:
            raise _lib.NscError(f"MapLocalizer.{what}: start and stop must satisfy 0 <= start <= stop <= {n}, got {start} "
                                f"and {stop}")
        return int(start), int(stop)

    def observe_prepared(self, store: PreparedClouds, poses, pose_ids=None, start=0, stop=None):
        """``observe`` on the clouds ``start`` to ``stop`` (the end, if None) of a ``PreparedClouds``; ``poses`` and
        ``pose_ids`` have one entry per cloud of that range."""
        if self.voxels is None:
            raise _lib.NscError("MapLocalizer.observe_prepared: build a map first")
        start, stop = self._store_range("observe_prepared", store, start, stop)
        return self._observed(self.observe_device(*_prepared_clouds(store, poses, pose_ids, start, stop)))

    def seen_through(self):
        """(M,) bool: the voxels later scans looked through -- count > 0, crossed >= ``min_crossings`` and
        crossed >= ``crossing_ratio`` x count.  Torch arithmetic on ``crossed`` and ``info``, for inspection;
        ``flag_rows_device`` decides the same on the device, per row."""
        if self.voxels is None or self.crossed is None:
            raise _lib.NscError("MapLocalizer.seen_through: build a map and observe scans first")
        count = self.info[:, 0]
        return (count > 0) & (self.crossed >= self.min_crossings) & \
            (self.crossed.to(torch.float64) >= self.crossing_ratio * count.to(torch.float64))

    def flag_rows_device(self, points, offsets, poses, pose_ids=None):
        """The rows of packed clouds whose own voxel is seen through (nsc_map_flag_rows), on the device and without a
        synchronisation.  Arguments as ``build_device``.  Returns row_flags (N,) bool and flag_stats (4,) int64
        (``_lib.MAP_FLAG_STAT_NAMES``: flagged, kept, dropped as a build drops rows, without a voxel in the map)."""
        self._observable("flag_rows_device", points)
        dev = self.voxels.device
        c = _clouds(points, offsets, poses, pose_ids)
        flags = torch.empty((c.N,), dtype=torch.bool, device=dev)
        flag_stats = torch.empty((_lib.MAP_FLAG_STATS,), dtype=torch.int64, device=dev)
        _lib.call("nsc_map_flag_rows", dev, *_row_args(c, self.params), self.index, self.info, self.crossed, self.capacity,
                  self.min_crossings, self.crossing_ratio, flags, flag_stats, _lib.STREAM)
        return dict(row_flags=flags, flag_stats=flag_stats)

    @staticmethod
    def without(points, mask):
        """``points`` with the rows of ``mask`` (N,) bool made NaN, on the device.  Every map call drops and counts a row
        that is not finite, so this is how a subset of a cloud's rows is given to a call that takes whole clouds."""
        nan = torch.full((), float("nan"), dtype=points.dtype, device=points.device)
        return torch.where(mask[:, None], nan, points)

    def carve_device(self, points, offsets, poses, pose_ids=None):
        """Take out of the kept map the rows of these clouds that lie in seen-through voxels: ``flag_rows_device``, then
        ``remove_device`` on the clouds with every row that is NOT flagged made NaN -- a matched removal of a subset, with
        no compaction and no read-back -- then ``crossed`` is zeroed.  The clouds must be in the map under these poses.
        The map is afterwards, voxel by voxel, the build over the rows that were kept.  With device ``pose_ids`` (or none)
        the sequence can be captured, ``observe_device`` in front of it included.  Returns the kept tensors, removed
        (8,) (carved rows as rows_removed, the others as removed_not_finite), flag_stats (4,) and carved (N,) bool.

        A cloud that has been carved must from then on be moved or removed as ``without(points, carved)``, its carved rows
        NaN, in ``remove*``, ``replace*`` and ``update_prepared`` alike: the map no longer holds those rows, and taking
        them out again sends the counts of their voxels below zero (``voxels_inconsistent``)."""
        self._insertable_map("carve_device")
        flagged = self.flag_rows_device(points, offsets, poses, pose_ids)
        carved = flagged["row_flags"]
        nan = torch.full((), float("nan"), dtype=points.dtype, device=points.device)
        out = self.remove_device(torch.where(carved[:, None], points, nan), offsets, poses, pose_ids)   # without(points, ~carved)
        self.crossed.fill_(0)                                    # a fill kernel, as the cursor's
        return dict(out, flag_stats=flagged["flag_stats"], carved=carved)

    def _carved(self, out):
        """carve_device's dict -> ``remove``'s dict, the four counts of flag_stats by name and ``carved``"""
        flag_stats = out["flag_stats"]
        res = self._removed(out)                                 # the one synchronisation
        res.update(zip(_lib.MAP_FLAG_STAT_NAMES, flag_stats.cpu().tolist()))
        res["carved"] = out["carved"]
        return res

    def carve(self, clouds, poses, pose_ids=None):
        """``carve_device`` on the input forms of ``build``.  Returns ``remove``'s dict, the four counts of flag_stats by
        name and carved (N,) bool over the packed rows; one synchronisation."""
        self._insertable_map("carve")
        return self._carved(self.carve_device(*_host_clouds(clouds, poses, pose_ids, self.voxels.device)))

    def carve_prepared(self, store: PreparedClouds, poses, pose_ids=None, start=0, stop=None):
        """``carve`` on the clouds ``start`` to ``stop`` (the end, if None) of a ``PreparedClouds``, under the poses they
        were placed by."""
        self._insertable_map("carve_prepared")
        start, stop = self._store_range("carve_prepared", store, start, stop)
        return self._carved(self.carve_device(*_prepared_clouds(store, poses, pose_ids, start, stop)))

    # ---- resizing and compaction -------------------------------------------------------------------------------------

    def _resizable(self, what, max_voxels):
        """the host-side refusals of a resize -> the new capacity"""
        if self.voxels is None:
            raise _lib.NscError(f"MapLocalizer.{what}: build a map first")
        M = self.capacity if max_voxels is None else int(max_voxels)
        if not 1 <= M <= _lib.MAP_MAX_VOXELS:
            raise _lib.NscError(f"MapLocalizer.{what}: max_voxels must lie in [1, {_lib.MAP_MAX_VOXELS}], got {M}")
        return M

    def resize_device(self, max_voxels=None, compact=True, out=None):
        """Move the kept map to the capacity ``max_voxels`` (nsc_map_rehash_dist; None keeps the capacity), on the device
        and without a synchronisation.  With ``compact`` the emptied voxels (count 0, zero moments) are left behind; the
        kept voxels take the places 0, 1, ... in their old order, records and integers copied by bits, and the index is
        keyed anew.  While the voxels kept fit, the map is then the build at the new capacity over the rows it holds, bit
        for bit, and the clouds are not needed for it.  ``out``: a dict of the destination tensors as ``build_device``
        takes them (moments and cursor when the map keeps them), with new_place (old capacity,), tile_base
        (ceil(old capacity / ``_lib.MAP_TILE_ROWS``) + 1,) and rehashed (6,) int64; with it a call can be captured (the
        graph reads the tensors that were kept when it was captured: the caller keeps them alive).
        The kept tensors are then the destination's, ``capacity`` and ``max_voxels`` the new size -- a later
        ``build_device`` and every ``insert*``, ``remove*``, ``replace*`` and ``register*`` use it -- and ``complete`` is
        None.  Returns the kept tensors, new_place (the new place of every old place, or -1), tile_base and rehashed
        (``_lib.MAP_REHASH_STAT_NAMES``).
        Measured on the map of profiles/map_localize.md (90.8 M rows, 484 681 voxels, capacity 4 194 304): 0.358 ms to
        the same capacity and 0.390 ms to twice the capacity, against 44.85 and 45.99 ms for ``build_prepared`` at the new
        capacity over the same clouds (1/125 and 1/118); 0.399 ms for a fit after every second cloud was removed, against
        22.48 ms (1/56).  The copy pass reaches a quarter of a flat device copy's rate there, because the voxels of a map
        far below its capacity stand in few tiles (profiles/map_localize.md, "Resizing the kept map")."""
        M = self._resizable("resize_device", max_voxels)
        dev, old = self.voxels.device, self.capacity
        tiles = -(-old // _lib.MAP_TILE_ROWS)
        shapes = self._shapes(M, self.moments is not None, self.cursor is not None)
        shapes.update(new_place=((old,), torch.int64), tile_base=((tiles + 1,), torch.int64),
                      rehashed=((_lib.MAP_REHASH_STATS,), torch.int64))
        out = _outputs(shapes, out, dev)
        _lib.call("nsc_map_rehash_dist", dev, self.voxels, self.info, self.keys, self.moments, self.stats, self.cursor, old,
                  0 if compact else 1, out["voxels"], out["index"], out["info"], out["keys"], out.get("moments"),
                  out["stats"], out.get("cursor"), M, out["new_place"], out["tile_base"], out["rehashed"], _lib.STREAM)
        if self.crossed is not None:
            # side data by place follows new_place; a place that was dropped adds to an entry past the end, which is cut off
            moved = torch.zeros((M + 1,), dtype=torch.int64, device=dev)
            moved.scatter_add_(0, torch.where(out["new_place"] >= 0, out["new_place"], M), self.crossed)
            self.crossed = moved[:M]
        self._keep(out, M, out["moments"] if self.moments is not None else None,
                   out["cursor"] if self.cursor is not None else None)
        self.max_voxels = M
        return dict(self._kept(), new_place=out["new_place"], tile_base=out["tile_base"], rehashed=out["rehashed"])

    def resize(self, max_voxels=None, compact=True):
        """``resize_device`` in its host form.  Returns ``build``'s dict over the whole map and the six counts of
        ``rehashed`` by name; one synchronisation."""
        out = self.resize_device(max_voxels, compact)
        rehashed = out["rehashed"]
        res = self._result(out)                                  # the one synchronisation
        res.update(zip(_lib.MAP_REHASH_STAT_NAMES, rehashed.cpu().tolist()))
        return res

    def fit(self, headroom: float = 1.0, compact=True):
        """``resize`` to max(1, ceil(``headroom`` x voxels_written)): the way to give back the memory of a build with
        ``max_voxels=None``, whose capacity is its row count.  Reads the stats once before the resize, so with
        ``compact`` the voxels dropped come off the new capacity only at the next ``fit``."""
        if self.voxels is None:
            raise _lib.NscError("MapLocalizer.fit: build a map first")
        if not (np.isfinite(headroom) and float(headroom) >= 1.0):
            raise _lib.NscError(f"MapLocalizer.fit: headroom must be finite and at least 1, got {headroom!r}")
        written = int(self.stats[1])                             # voxels_written
        return self.resize(max(1, int(np.ceil(float(headroom) * written))), compact)

    def _result(self, out):
        """build_device's buffers -> the dict ``build`` returns (one read of the stats)"""
        vox = out["voxels"]
        res = _result(out, lambda n: dict(mean=vox[:n, 0:3], covariance=vox[:n, 3:9], information=vox[:n, 9:15],
                                          usable=vox[:n, 15] == 1.0))
        self.complete = res["complete"]
        return res

    def build(self, clouds, poses, pose_ids=None):
        """The map of ``clouds`` -- a sequence of (n,3|4) host arrays or tensors, or a packed ``(points, offsets)`` pair of
        device tensors -- under ``poses`` (P,4,4), host or device.  Returns device tensors in ascending first_row -- mean
        (V,3), covariance and information (V,6: xx xy xz yy yz zz) float64, usable (V,) bool, count, first_row,
        first_cloud, last_cloud, keys (V,) int64 -- the stats by name and ``complete``.  One synchronisation, to read the
        stats."""
        return self._result(self.build_device(*_host_clouds(clouds, poses, pose_ids, self.device)))

    def build_prepared(self, store: PreparedClouds, poses, pose_ids=None):
        """``build`` on the clouds a ``PreparedClouds`` holds, as ``GlobalMap.build_prepared``."""
        return self._result(self.build_device(*_prepared_clouds(store, poses, pose_ids)))

    # ---- registration -------------------------------------------------------------------------------------------------

    def register_device(self, points, offsets, init_poses, system0=False):
        """Register packed scans against the kept map, on the device and without a synchronisation: a call can be
        captured.  ``points`` (N,3|4) float32 or (N,3) float64 device tensor, ``offsets`` (S+1,) int64 device tensor,
        ``init_poses`` (S,4,4) float64 device tensor, scan to world.  Returns a dict of device tensors: transform (S,4,4),
        fitness, rmse, cost (S,), n_correspondences, iterations (S,) int64, information (S,6,6); with ``system0=True``
        also system0 (S,30), the sums at ``init_poses`` (include/nsc.h).  With a kernel or seven voxels the dict also has
        weight_sum (S,) float64 and n_pairs (S,) int64 (one conversion launch after the library's), and system0 is
        (S,32): the 30 sums, then sum w and n_pairs.  More than ``_lib.MAP_REGISTER_MAX_SCANS`` scans
        go to the library in several calls, the outputs are those of one call."""
        if self.voxels is None:
            raise _lib.NscError("MapLocalizer.register: build a map first")
        for t, name in ((points, "points"), (offsets, "offsets"), (init_poses, "init_poses")):
            _lib.require_cuda(t, name)
        dev = self.voxels.device
        pts, off, S, N, dtype = _rows(points, offsets, "scan points")
        if pts.device != dev:
            raise _lib.NscError(f"the scans must be on the map's device ({dev})")
        if init_poses.ndim != 3 or tuple(init_poses.shape) != (S, 4, 4):
            raise _lib.NscError(f"init_poses must be ({S},4,4), got {tuple(init_poses.shape)}")
        init = init_poses.contiguous().to(torch.float64)
        f64 = dict(dtype=torch.float64, device=dev)
        T, fr, cost = torch.empty((S, 4, 4), **f64), torch.empty((S, 2), **f64), torch.empty((S,), **f64)
        ci = torch.empty((S, 2), dtype=torch.int64, device=dev)
        info = torch.empty((S, 6, 6), **f64)
        plain = self.robust.kernel == 0 and self.robust.neighbours == 1
        width = _lib.MAP_REGISTER_SYSTEM if plain else _lib.MAP_REGISTER_ROBUST_SYSTEM
        sys0 = torch.empty((S, width), **f64) if system0 else None
        wp = None if plain else torch.empty((S, 2), **f64)
        L = _lib.lib()
        most = _lib.MAP_REGISTER_MAX_SCANS
        need = L.nsc_map_register_workspace_bytes if plain else L.nsc_map_register_robust_workspace_bytes
        ws = _workspace(need(min(S, most)), dev)
        for a in range(0, S, most):
            b = min(a + most, S)
            head = (pts, dtype, int(pts.shape[1]), off[a:], b - a, N, self.voxels, self.index, self.capacity, self.params,
                    self.reg)
            outs = (init[a:], T[a:], fr[a:], cost[a:], ci[a:], info[a:], None if sys0 is None else sys0[a:])
            tail = (ws, int(ws.numel()), _lib.STREAM)
            if plain:
                _lib.call("nsc_map_register", dev, *head, *outs, *tail)
            else:
                _lib.call("nsc_map_register_robust", dev, *head, self.robust, *outs, wp[a:], *tail)
        out = dict(transform=T, fitness=fr[:, 0], rmse=fr[:, 1], cost=cost, n_correspondences=ci[:, 0],
                   iterations=ci[:, 1], information=info)
        if wp is not None:
            out["weight_sum"] = wp[:, 0]
            out["n_pairs"] = wp[:, 1].to(torch.int64)
        if sys0 is not None:
            out["system0"] = sys0
        return out

    def register(self, scans, init_poses, system0=False):
        """Register ``scans`` -- a sequence of (n,3|4) host arrays or tensors, or a packed ``(points, offsets)`` pair of
        device tensors -- from ``init_poses`` (S,4,4), host or device, scan to world.  Returns ``register_device``'s dict
        of device tensors."""
        if self.voxels is None:
            raise _lib.NscError("MapLocalizer.register: build a map first")
        pts, off, pose, _ = _host_scans(scans, init_poses, self.voxels.device)
        return self.register_device(pts, off, pose, system0=system0)
