"""Stage 1 of the reference's two-stage loop closing on MI355X -- mirror of src/retrieval/two_stage_retrieval.py
``TwoStageRetrieval`` (:40-295): ``add_keyframe`` (:91-105), ``query`` (:107-143), ``_global_retrieval`` (:145-202),
``get_loop_closures`` (:244-290), ``clear_database`` (:292-295), ``create_two_stage_retrieval`` (:298-320) and
``batch_loop_closing`` (:322-359).

What runs where
  * stage 1 (Wasserstein retrieval + the spatial filter) is the consumer of the descriptors the hot path produces and
    runs on the device: ``add_keyframe`` appends ONE row to an HBM-resident database (histogram, its normalised CDF
    -- nsc_w1_cdf -- and the keyframe position; amortised-doubling buffers instead of the reference's np.vstack per
    insert, wasserstein.py:324), ``_global_retrieval`` is one streaming pass over the CDF rows with the
    ``dist < spatial_filter_distance`` test of :160-170 fused in (nsc_w1_distances_cdf) and a device top-k
    (nsc_topk_smallest).  The reference ranks ALL rows, then walks the sorted list skipping filtered rows until it
    has top_k (:182-200): that is the top_k of the unfiltered rows, which is what the fused form returns.
  * stage 2 (GICP, src/retrieval/geometric_verification.py) is injected: pass ``verifier=`` (an object with the
    reference's ``verify(query_points, candidate_points) -> (verified, transform, info)``; ``GeometricVerifier()``
    of geometric_verification.py runs it on the device) and, for g2o edges, ``edge_fn=`` (the reference's
    ``compute_pose_graph_edge``).  Without them ``query(verify=True)`` / ``get_loop_closures`` raise.  A verifier
    with ``verify_batch(query_points, candidate_points_list)`` checks all candidates of a query in one call.
    With ``prepare_geometry=True`` (and a ``GeometricVerifier``) every keyframe's cloud is prepared once, when it is
    inserted, into a device store (PreparedClouds) whose ids are the database indices; a query prepares its own
    cloud once and is registered against its candidates by id.  The results are bitwise those of the default
    mode; the store costs about 100 B of HBM per down-sampled row and moves the cost to insert time.
    With ``yaw_init=True`` every pair starts from the yaw read off the two keyframes' range images (yaw_alignment.py,
    nsc_yaw_align) instead of the identity, so a revisit under another heading verifies: every keyframe's
    interpolated range image (``keyframe.range_image``, else ``yaw_encoder`` on its points) goes into a device store
    (YawImages, 23 KB per keyframe at 16 rows) when it is inserted, a query's candidates are estimated in one launch
    and the guesses reach the registration as a device tensor.  Off (the default) nothing of this runs.
    With ``planar_init=True`` (needs ``prepare_geometry=True``; not together with ``yaw_init``) every pair starts from
    the yaw and planar translation that the structure rows of the two prepared clouds vote for (planar_alignment.py,
    nsc_planar_align), so a revisit that is rotated and metres away -- the other lane -- verifies: a query's
    candidates are estimated in one call on the stores stage 2 already holds.  ``planar_min_support``, when given,
    marks a candidate whose ``planar_support`` is below it as not verified, whatever GICP returned.  Off (the
    default) nothing of this runs.
  * With ``compressed=True`` stage 1 runs over 16-bit rows: ``retriever`` is a ``CompressedRetriever`` (compressed.py),
    descriptors and queries are quantised as the wire format quantises them and ranked by the integer W1 of their
    CDFs -- a quarter of the HBM per keyframe, distances that are those of the dequantised descriptors.  Off (the
    default) nothing of this runs.

``ShardedTwoStageRetrieval`` is the multi-GPU form (BASELINE configs[3]): the database rows
stay sharded over the ranks in the layout of ``distributed.shard_range``; every rank scores its own rows, the
k best (distance, global index) pairs of every rank are exchanged with ONE all-gather of k entries per rank and
query, and merged -- identical on every rank, and identical to the single-GPU result (ties resolve to the smaller
global index in both).
"""
import inspect
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.distributed as dist

from .. import _lib
from . import geometric_verification as _gv
from . import planar_alignment as _planar
from . import yaw_alignment as _yaw
from .compressed import CompressedRetriever
from .wasserstein import WassersteinRetriever, _topk

_NO_POSE = np.full(3, np.inf, np.float32)     # a keyframe without a pose is never filtered out (:163)
_PREPARE_ROWS = 1 << 22                       # raw rows per prepare call: bounds its workspace (~200 B per row)


@dataclass
class LoopClosureCandidate:
    """two_stage_retrieval.py:28-37"""
    database_idx: int
    distance: float                      # Wasserstein distance
    verified: bool = False
    transform: Optional[np.ndarray] = None
    fitness: Optional[float] = None
    rmse: Optional[float] = None
    information_matrix: Optional[np.ndarray] = None
    info: Optional[dict] = None          # the verifier's info dict (with yaw_init: + init_yaw_deg, yaw_peak_ratio;
                                         # with planar_init: + planar_info's keys)


def _position(pose) -> np.ndarray:
    if pose is None:
        return _NO_POSE
    return np.asarray(pose, dtype=np.float64)[:3, 3].astype(np.float32)   # euclidean_distance: translations only


class TwoStageRetrieval:
    """Two-stage loop closing system (two_stage_retrieval.py:40-295); stage 1 on the device."""

    def __init__(self, top_k: int = 10, spatial_filter_distance: float = 50.0, context_window: int = 10,
                 fitness_threshold: float = 0.3, rmse_threshold: float = 0.5, verification_method: str = "gicp",
                 use_torch: bool = True, device: str = 'cuda', verifier=None, edge_fn=None,
                 prepare_geometry: bool = False, yaw_init: bool = False, yaw_encoder=None, compressed: bool = False,
                 planar_init: bool = False, planar_min_support: Optional[float] = None):
        self.top_k = top_k
        self.spatial_filter_distance = spatial_filter_distance
        self.context_window = context_window
        self.fitness_threshold, self.rmse_threshold = fitness_threshold, rmse_threshold
        self.verification_method = verification_method
        if compressed:                   # 16-bit database (compressed.py): descriptors are quantised at insert
            self.retriever = CompressedRetriever(device=device)
        else:
            self.retriever = WassersteinRetriever(use_torch=True, device=device)      # :76-79
        self.verifier = verifier                                                      # :82-86 (Open3D: injected)
        self.edge_fn = edge_fn
        self.keyframes: list = []                                                     # :89
        self.geometry = None             # prepare_geometry: PreparedClouds of the keyframes, id = database index
        self._query_geometry = None
        if prepare_geometry:
            if not isinstance(verifier, _gv.GeometricVerifier):
                raise _lib.NscError("prepare_geometry=True needs verifier=GeometricVerifier(...)")
            self.geometry = verifier.prepare()
            self._query_geometry = verifier.prepare()
        if planar_init and yaw_init:
            raise ValueError("planar_init=True already searches the yaw: do not combine it with yaw_init=True")
        if planar_init and self.geometry is None:
            raise _lib.NscError("planar_init=True reads the prepared stores: it needs prepare_geometry=True")
        self.planar_init = bool(planar_init)
        self.planar_min_support = None if planar_min_support is None else float(planar_min_support)
        self.yaw_images = None           # yaw_init: YawImages of the keyframes, id = database index
        self.yaw_encoder = None
        if yaw_init:
            method = "verify_prepared" if prepare_geometry else "verify_batch"
            fn = getattr(verifier, method, None)
            if fn is None or "init_transforms" not in inspect.signature(fn).parameters:
                raise _lib.NscError(f"yaw_init=True needs a verifier whose {method} takes init_transforms "
                                    "(GeometricVerifier does)")
            self.yaw_images = _yaw.YawImages(device=device)
            if yaw_encoder is None:
                from ..encoding import SpectralEncoder
                yaw_encoder = SpectralEncoder(n_elevation=16, device=device).to(device)
            self.yaw_encoder = yaw_encoder

    def _check_points(self, keyframes):
        if self.geometry is not None:
            for kf in keyframes:
                if getattr(kf, "points", None) is None:
                    raise ValueError("Keyframe must have points before adding to a database with prepare_geometry")

    def _range_images(self, keyframes, points=None) -> torch.Tensor:
        """(B, R, 360) float32 device tensor: each keyframe's ``range_image`` if it has one, else the interpolated
        image of its points (``points[i]`` in place of ``keyframes[i].points`` if given) by ``yaw_encoder``, all
        clouds in one encoder call."""
        dev = self.yaw_images.device
        given = [None if points is not None and points[i] is not None else getattr(kf, "range_image", None)
                 for i, kf in enumerate(keyframes)]
        clouds = [(points[i] if points is not None and points[i] is not None else kf.points)
                  for i, kf in enumerate(keyframes) if given[i] is None]
        if any(c is None for c in clouds):
            raise ValueError("Keyframe must have a range_image or points with yaw_init")
        made = iter(self.yaw_encoder.encode_points_batch(clouds, return_images=True)[2]) if clouds else iter(())
        out = [_yaw._images(g, dev)[0] if g is not None else next(made) for g in given]
        return torch.stack(out) if out else torch.empty((0, 1, _yaw.N_AZIMUTH), dtype=torch.float32, device=dev)

    # -- database --------------------------------------------------------------------------------
    def add_keyframe(self, keyframe):
        """:91-105"""
        if keyframe.descriptor is None:
            raise ValueError("Keyframe must have descriptor before adding to database")
        self._check_points([keyframe])
        image = self._range_images([keyframe]) if self.yaw_images is not None else None
        if self.geometry is not None:
            self.geometry.add([keyframe.points])
        if image is not None:
            self.yaw_images.add(image)
        self.keyframes.append(keyframe)
        descriptor = np.asarray(keyframe.descriptor, dtype=np.float32).reshape(1, -1)
        self.retriever.add_to_database(descriptor, positions=_position(keyframe.pose).reshape(1, 3))

    def add_keyframes(self, keyframes):
        """Additive: append a batch of keyframes with one device copy (the offline path of
        ``batch_loop_closing``, :344-346, inserts them one by one)."""
        keyframes = list(keyframes)
        if not keyframes:
            return
        for kf in keyframes:
            if kf.descriptor is None:
                raise ValueError("Keyframe must have descriptor before adding to database")
        self._check_points(keyframes)
        images = self._range_images(keyframes) if self.yaw_images is not None else None
        if self.geometry is not None:
            prepare_chunked(self.geometry, [kf.points for kf in keyframes])
        if images is not None:
            self.yaw_images.add(images)
        self.keyframes.extend(keyframes)
        desc = np.stack([np.asarray(kf.descriptor, dtype=np.float32).reshape(-1) for kf in keyframes])
        self.retriever.add_to_database(desc, positions=np.stack([_position(kf.pose) for kf in keyframes]))

    def clear_database(self):
        """:292-295"""
        self.keyframes.clear()
        self.retriever.clear_database()
        if self.geometry is not None:
            self.geometry.clear()
        if self.yaw_images is not None:
            self.yaw_images.clear()

    # -- stage 1 ---------------------------------------------------------------------------------
    def _retrieve(self, descriptors: np.ndarray, poses) -> tuple:
        """(Q, D) query descriptors + their poses (None entries = no pose) -> (idx (Q,k), dist (Q,k)) on the
        host, ascending; filtered-out / missing candidates come back as index -1."""
        n = len(self.keyframes)
        q = np.asarray(descriptors, dtype=np.float32).reshape(len(poses), -1)
        if n == 0:
            return np.zeros((len(poses), 0), np.int64), np.zeros((len(poses), 0), np.float32)
        k = min(self.top_k, n)
        # a query without a pose is not filtered (:163): give it a position infinitely far from everything
        qpos = np.stack([_position(p) for p in poses])
        idx, val = self.retriever.query_batch(q, top_k=k, query_positions=qpos,
                                              min_distance=float(self.spatial_filter_distance))
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        idx = np.where(np.isinf(val), -1, idx)          # rows the spatial filter excluded carry +inf
        return idx, val

    def _global_retrieval(self, query_keyframe) -> List[LoopClosureCandidate]:
        """:145-202"""
        idx, val = self._retrieve(np.asarray(query_keyframe.descriptor).reshape(1, -1), [query_keyframe.pose])
        return [LoopClosureCandidate(database_idx=int(i), distance=float(d)) for i, d in zip(idx[0], val[0]) if i >= 0]

    def global_retrieval_batch(self, query_keyframes) -> List[List[LoopClosureCandidate]]:
        """Additive: stage 1 for many query keyframes in one pass over the database."""
        query_keyframes = list(query_keyframes)
        if not query_keyframes:
            return []
        desc = np.stack([np.asarray(kf.descriptor, dtype=np.float32).reshape(-1) for kf in query_keyframes])
        idx, val = self._retrieve(desc, [kf.pose for kf in query_keyframes])
        return [[LoopClosureCandidate(database_idx=int(i), distance=float(d)) for i, d in zip(ri, rv) if i >= 0]
                for ri, rv in zip(idx, val)]

    # -- stage 2 (injected) ----------------------------------------------------------------------
    def _geometric_verification(self, query_points, candidates, query_image=None):
        """:204-242 with the injected verifier.  ``query_image``: the query's range image with yaw_init."""
        if self.verifier is None:
            raise _lib.NscError("stage 2 (GICP) is outside the MI355X descriptor path: construct TwoStageRetrieval "
                                "with verifier=<object with the reference's GeometricVerifier.verify> or call "
                                "query(..., verify=False)")
        ids = [c.database_idx for c in candidates]
        yaw, init = None, {}             # no yaw estimate, no init_transforms: an injected verifier need not take it
        if self.yaw_images is not None:
            yaw = _yaw.estimate_yaw(query_image, [0] * len(ids), self.yaw_images, ids)      # one launch, no sync
            init = dict(init_transforms=yaw["init_transforms"])
        if self.geometry is not None:
            self._query_geometry.clear()
            self._query_geometry.add([query_points])
            planar = None
            if self.planar_init:                                 # three launches, no sync
                planar = _planar.estimate_planar(self._query_geometry, [0] * len(ids), self.geometry, ids)
                init = dict(init_transforms=planar["init_transforms"])
            results = self.verifier.verify_prepared(self._query_geometry, 0, self.geometry, ids, **init)
            if planar is not None:
                results = _with_planar_info(results, planar, self.planar_min_support)
        elif hasattr(self.verifier, "verify_batch"):
            results = self.verifier.verify_batch(query_points, [self.keyframes[i].points for i in ids], **init)
        else:
            results = (self.verifier.verify(query_points, self.keyframes[i].points) for i in ids)
        if yaw is not None:
            results = _with_yaw_info(results, yaw)
        return _apply(candidates, results)

    def query(self, query_keyframe, query_points: Optional[np.ndarray] = None, verify: bool = True
              ) -> List[LoopClosureCandidate]:
        """:107-143"""
        if query_keyframe.descriptor is None:
            raise ValueError("Query keyframe must have descriptor")
        candidates = self._global_retrieval(query_keyframe)
        if len(candidates) == 0:
            return []
        if verify:
            image = None
            if self.yaw_images is not None:
                image = self._range_images([query_keyframe], [query_points])
            if query_points is None:
                query_points = query_keyframe.points
            candidates = self._geometric_verification(query_points, candidates, query_image=image)
        return candidates

    def get_loop_closures(self, query_keyframe, query_points: Optional[np.ndarray] = None) -> List[Dict]:
        """:244-290"""
        if self.edge_fn is None:
            raise _lib.NscError("get_loop_closures needs edge_fn=<the reference's compute_pose_graph_edge> "
                                "(geometric_verification.py, outside the MI355X descriptor path)")
        candidates = self.query(query_keyframe, query_points=query_points, verify=True)
        return self._edges(query_keyframe, candidates)

    def _edges(self, query_keyframe, candidates) -> List[Dict]:
        """The loop-closure edges of a query's verified candidates (:260-288)."""
        loop_closures = []
        for candidate in candidates:
            if not candidate.verified:
                continue
            candidate_kf = self.keyframes[candidate.database_idx]
            edge = self.edge_fn(source_pose=query_keyframe.pose, target_pose=candidate_kf.pose,
                                relative_transform=candidate.transform,
                                information_matrix=candidate.information_matrix)
            edge['source_id'] = query_keyframe.keyframe_id
            edge['target_id'] = candidate_kf.keyframe_id
            edge['fitness'] = candidate.fitness
            edge['rmse'] = candidate.rmse
            edge['wasserstein_distance'] = candidate.distance
            loop_closures.append(edge)
        return loop_closures


def _apply(candidates, results):
    """Write the stage-2 results onto the candidates; -> the verified ones (:204-242)."""
    verified_candidates = []
    for candidate, (verified, transform, info) in zip(candidates, results):
        candidate.verified = verified
        candidate.transform = transform
        candidate.fitness = info['fitness']
        candidate.rmse = info['rmse']
        candidate.information_matrix = info.get('information_matrix', None)
        candidate.info = info
        if verified:
            verified_candidates.append(candidate)
    return verified_candidates


def _with_yaw_info(results, yaw):
    """Add init_yaw_deg and yaw_peak_ratio of estimate_yaw's outputs to the info dicts of the pairs' results (read
    after the verifier's sync)."""
    host = torch.stack([yaw["shift"].double(), yaw["peak"], yaw["runner_up"]], 1).cpu().numpy()
    results = list(results)
    for (_, _, info), (shift, peak, runner_up) in zip(results, host):
        info.update(_yaw.yaw_info(shift, peak, runner_up))
    return results


def _with_planar_info(results, planar, min_support=None):
    """Add planar_info's keys of estimate_planar's outputs to the info dicts of the pairs' results (read after the
    verifier's sync); with ``min_support`` a pair whose planar_support is below it is not verified."""
    host = torch.cat([planar["init_transforms"].reshape(-1, 16), planar["scores"].double(),
                      planar["counts"].double()], 1).cpu().numpy()
    out = []
    for (verified, transform, info), row in zip(results, host):
        info.update(_planar.planar_info(row[:16], row[16], row[17], row[18]))
        if min_support is not None and info["planar_support"] < min_support:
            verified = False
        out.append((verified, transform, info))
    return out


def prepare_chunked(store, clouds, max_rows: int = _PREPARE_ROWS):
    """store.add(clouds) in calls of at most ``max_rows`` raw rows (one cloud at least) -> ids"""
    ids, chunk, rows = [], [], 0
    for c in clouds:
        n = len(c)
        if chunk and rows + n > max_rows:
            ids += store.add(chunk)
            chunk, rows = [], 0
        chunk.append(c)
        rows += n
    if chunk:
        ids += store.add(chunk)
    return ids


def create_two_stage_retrieval(top_k: int = 10, spatial_filter_distance: float = 50.0, use_gpu: bool = True,
                               **kwargs) -> TwoStageRetrieval:
    """:298-320 (``use_gpu`` is accepted for signature compatibility: stage 1 always runs on the HIP device)."""
    return TwoStageRetrieval(top_k=top_k, spatial_filter_distance=spatial_filter_distance, use_torch=True,
                             device='cuda', **kwargs)


def batch_loop_closing(query_keyframes, database_keyframes, top_k: int = 10, spatial_filter_distance: float = 50.0,
                       verify: bool = True, verifier=None, edge_fn=None, prepare_geometry: bool = False,
                       yaw_init: bool = False, planar_init: bool = False,
                       planar_min_support: Optional[float] = None) -> Dict[int, list]:
    """:322-359.  With ``verify=False`` the values are the stage-1 candidate lists (one database pass for all
    queries); with ``verify=True`` the injected stage 2 runs per query as in the reference.  With
    ``prepare_geometry=True`` (a GeometricVerifier) every database and query cloud is prepared once, stage 1 runs
    for all queries in one pass and stage 2 registers all queries' candidate pairs in one register_prepared call;
    the result equals the per-query one.  ``yaw_init=True`` starts every pair from its yaw guess (TwoStageRetrieval);
    with ``prepare_geometry=True`` all queries' pairs are estimated in one estimate_yaw call before the one
    registration.  ``planar_init=True`` (with ``prepare_geometry=True``) starts every pair from its planar guess
    (TwoStageRetrieval), all queries' pairs estimated in one estimate_planar call."""
    retrieval = create_two_stage_retrieval(top_k=top_k, spatial_filter_distance=spatial_filter_distance,
                                           verifier=verifier, edge_fn=edge_fn, prepare_geometry=prepare_geometry,
                                           yaw_init=yaw_init, planar_init=planar_init,
                                           planar_min_support=planar_min_support)
    retrieval.add_keyframes(database_keyframes)
    if not verify:
        return dict(enumerate(retrieval.global_retrieval_batch(query_keyframes)))
    if not prepare_geometry:
        return {i: retrieval.get_loop_closures(kf) for i, kf in enumerate(query_keyframes)}
    query_keyframes = list(query_keyframes)
    if retrieval.edge_fn is None and query_keyframes:
        retrieval.get_loop_closures(query_keyframes[0])          # raises, as the per-query path does
    for kf in query_keyframes:
        if kf.descriptor is None:
            raise ValueError("Query keyframe must have descriptor")
    retrieval._check_points(query_keyframes)
    candidates = retrieval.global_retrieval_batch(query_keyframes)
    queries = verifier.prepare()
    prepare_chunked(queries, [kf.points for kf in query_keyframes])
    qids = [i for i, cl in enumerate(candidates) for _ in cl]
    cids = [c.database_idx for cl in candidates for c in cl]
    if yaw_init and qids:
        yaw = _yaw.estimate_yaw(retrieval._range_images(query_keyframes), qids, retrieval.yaw_images, cids)
        results = _with_yaw_info(verifier.verify_pairs(queries, qids, retrieval.geometry, cids,
                                                       init_transforms=yaw["init_transforms"]), yaw)
    elif planar_init and qids:
        planar = _planar.estimate_planar(queries, qids, retrieval.geometry, cids)
        results = _with_planar_info(verifier.verify_pairs(queries, qids, retrieval.geometry, cids,
                                                          init_transforms=planar["init_transforms"]), planar,
                                    planar_min_support)
    else:
        results = verifier.verify_pairs(queries, qids, retrieval.geometry, cids)
    out, at = {}, 0
    for i, (kf, cl) in enumerate(zip(query_keyframes, candidates)):
        out[i] = retrieval._edges(kf, _apply(cl, results[at:at + len(cl)]))
        at += len(cl)
    return out


# ------------------------------------------------------------------------------------------------
# database rows sharded over the ranks
# ------------------------------------------------------------------------------------------------
def merge_topk(cand_dist: torch.Tensor, cand_idx: torch.Tensor, k: int):
    """(Q, C) candidate distances / global indices (C = world * k, rank-major, every rank's block ascending) ->
    the k smallest per query, ties to the earlier column (= the smaller global index, shards being contiguous and
    ascending).  Device tensors go through nsc_topk_smallest; host tensors (the gloo tests) through a stable sort."""
    k = min(k, int(cand_dist.shape[1]))
    if cand_dist.is_cuda:
        pos, val = _topk(cand_dist.contiguous(), k)
    else:
        val, pos = torch.sort(cand_dist, dim=1, stable=True)
        val, pos = val[:, :k], pos[:, :k]
    return torch.gather(cand_idx, 1, pos), val


class ShardedTwoStageRetrieval:
    """Stage 1 over a database whose rows are sharded over the ranks (rank r owns the global rows
    ``shard_range(n_total, r, world)``; ``local`` is that rank's retriever -- a WassersteinRetriever on the device,
    any object with its ``query_batch`` in the CPU tests).  Every rank passes the SAME queries."""

    def __init__(self, local, n_total: int, top_k: int = 10, spatial_filter_distance: float = 50.0, group=None):
        from ..distributed import shard_range
        self.local, self.group = local, group
        self.top_k, self.spatial_filter_distance = top_k, spatial_filter_distance
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.n_total = n_total
        self.lo, self.hi = shard_range(n_total, self.rank, self.world)

    def add_local_rows(self, descriptors, positions=None):
        """This rank's rows [lo, hi) of the gathered descriptor matrix (what the all-gather of the hot path hands
        over: pass ``desc_all[lo:hi]``), with their keyframe positions for the spatial filter."""
        assert int(descriptors.shape[0]) == self.hi - self.lo
        self.local.add_to_database(descriptors, positions=positions)

    def query_batch(self, query_hists, query_positions=None):
        """(Q, D) queries -> (global indices (Q, k) int64, distances (Q, k)), ascending, identical on every rank;
        index -1 where fewer than k unfiltered rows exist."""
        k = min(self.top_k, self.n_total)
        n_local = self.hi - self.lo
        kl = min(k, n_local)
        q = int(np.asarray(query_hists.shape)[0]) if hasattr(query_hists, "shape") else len(query_hists)
        if kl > 0:
            idx, val = self.local.query_batch(query_hists, top_k=kl, query_positions=query_positions,
                                              min_distance=float(self.spatial_filter_distance))
            dev = val.device
            idx = torch.where(torch.isinf(val), torch.full_like(idx, -1), idx + self.lo)
        else:
            dev = torch.device("cpu") if not hasattr(query_hists, "device") else query_hists.device
            idx = torch.empty((q, 0), dtype=torch.int64, device=dev)
            val = torch.empty((q, 0), dtype=torch.float32, device=dev)
        if kl < k:                                      # ragged shards: pad to k candidates per rank
            pad = k - kl
            idx = torch.cat([idx, torch.full((q, pad), -1, dtype=torch.int64, device=dev)], 1)
            val = torch.cat([val, torch.full((q, pad), float("inf"), dtype=torch.float32, device=dev)], 1)
        if self.world > 1:
            all_val = torch.empty((self.world * q, k), dtype=torch.float32, device=dev)      # rank-major concatenation
            all_idx = torch.empty((self.world * q, k), dtype=torch.int64, device=dev)
            dist.all_gather_into_tensor(all_val, val.contiguous(), group=self.group)     # k candidates per rank
            dist.all_gather_into_tensor(all_idx, idx.contiguous(), group=self.group)
            val = all_val.view(self.world, q, k).permute(1, 0, 2).reshape(q, self.world * k)
            idx = all_idx.view(self.world, q, k).permute(1, 0, 2).reshape(q, self.world * k)
            idx, val = merge_topk(val, idx, k)
        idx = torch.where(torch.isinf(val), torch.full_like(idx, -1), idx)
        return idx, val
