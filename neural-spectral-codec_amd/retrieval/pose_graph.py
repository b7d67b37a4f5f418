"""Pose-graph optimisation on the device (csrc/nsc_posegraph.hip): the consumer of stage 2's ``transform`` and
``information_matrix``.  Odometry edges and verified loop closures in, corrected poses out.

Definition (the contract nsc_posegraph_optimize and tests/posegraph_restatement.py share; include/nsc.h), float64:

    poses        (N,4,4) sensor to world;  edge (i, j) measures Z ~ X_i^-1 X_j with information Omega (6,6), rotation
                 first, upper triangle read
    residual     D = Z^-1 X_i^-1 X_j,  r = [Log_SO3(R_D); t_D],  cost F = sum r^T Omega r
    update       X_k <- [R_k Exp(phi_k) | t_k + R_k rho_k]
    Jacobians    J_j = B = blockdiag(Jr^-1(r_phi), R_D),  J_i = -B Ad(A^-1),  A = X_i^-1 X_j
    solver       Levenberg-Marquardt, (H + lambda diag H) delta = -g by block-Jacobi preconditioned conjugate gradients;
                 a step is accepted when the cost decreases

    coarse       ``coarse_block`` = L adds a coarse space to the preconditioner: one rigid motion per aggregate of L
                 consecutive poses, M^-1 r = B^-1 r + P (P^T A P)^-1 P^T r (include/nsc.h).  It carries the long
                 wavelengths of a trajectory that block-Jacobi needs of the order of N inner iterations for

    robust       with s = r^T Omega r and a width c per edge (``robust_scale``, in units of sqrt(chi^2)):
                 F = sum rho(s), g = sum w J^T Omega r, H = sum w J^T Omega J, w = rho'(s) (first order: IRLS)
                   huber          rho = s for s <= c^2, else 2 c sqrt(s) - c^2    w = 1, else c / sqrt(s)
                   cauchy         rho = c^2 log1p(s / c^2)                        w = 1 / (1 + s / c^2)
                   geman_mcclure  rho = c^2 s / (c^2 + s)                         w = (c^2 / (c^2 + s))^2
                 an edge whose width is not finite and positive is quadratic (rho = s, w = 1): give odometry edges 0

    covariance   Sigma = the inverse, over the free poses, of the undamped H at the given poses (robust weights included):
                 the covariance of the right perturbations delta_k in X_k Exp(delta_k), in the gauge the fixed poses set.
                 ``PoseGraphOptimizer.covariance`` returns the joint blocks of selected poses, each column a conjugate-
                 gradient solve of its own, all columns in one batch on the device

Edges with i == j or an index outside [0, N) are skipped and counted.  Residual rotations beyond 179 degrees are out of
scope.  2-D graphs and g2o files are not part of this module.

Gating a closure before it enters the graph: ``TwoStageRetrieval.query`` -> ``closure_edges`` (Z, Omega of each verified
candidate) -> ``PoseGraphOptimizer.covariance`` on the graph so far, with nodes = [query, candidates...] -> per candidate
``relative_covariance`` of the pair's blocks -> ``closure_mahalanobis`` against a chi^2 quantile at 6 degrees of freedom.

A false closure that passed geometric verification keeps weight 1 under the quadratic cost and bends the whole
trajectory; with ``kernel="cauchy"`` and a width of about 3 on the closure edges it ends with a weight below 1e-3, and
``optimize`` returns ``chi2`` and ``weights`` per edge so that the caller can drop it.

The consumer of ``optimize``'s poses is ``GlobalMap`` (global_map.py): it places the stored keyframe clouds by them and
merges the clouds into one voxel map, whose voxel count says, without ground truth, whether the closures helped.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib

# this module's order is rotation first (phi, rho), as nsc_gicp_register's information; g2o's EDGE_SE3 is translation first
_G2O = np.array([3, 4, 5, 0, 1, 2])


def information_to_g2o(information):
    """(…,6,6) rotation-first -> translation-first (the block order of g2o's EDGE_SE3:QUAT).  The rotation block stays
    that of a rotation vector: g2o's quaternion-vector parametrisation differs from it by a factor 2 per axis, which
    the caller applies when writing a file."""
    m = np.asarray(information, np.float64)
    return m[..., _G2O, :][..., :, _G2O]


def information_from_g2o(information):
    """The inverse of information_to_g2o (the permutation is its own inverse)."""
    return information_to_g2o(information)


def _hat(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def adjoint(T):
    """Ad(R, t) = [[R, 0], [[t]x R, R]] for twists ordered rotation first."""
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = _hat(t) @ R
    return A


def _inverse(T):
    R, t = T[..., :3, :3], T[..., :3, 3]
    out = np.zeros_like(T)
    out[..., :3, :3] = np.swapaxes(R, -1, -2)
    out[..., :3, 3] = -np.einsum("...ji,...j->...i", R, t)
    out[..., 3, 3] = 1.0
    return out


def odometry_edges(poses, information=None):
    """Chain edges of a trajectory: -> (edge_ij (N-1,2) int64, Z (N-1,4,4) with Z_k = X_k^-1 X_{k+1}, Omega (N-1,6,6)).
    ``information``: one (6,6) matrix for every edge, a (N-1,6,6) stack, or None for the identity."""
    X = poses.detach().cpu().numpy() if isinstance(poses, torch.Tensor) else np.asarray(poses)
    X = np.asarray(X, np.float64).reshape(-1, 4, 4)
    n = max(len(X) - 1, 0)
    e = np.stack([np.arange(n), np.arange(1, n + 1)], 1).astype(np.int64).reshape(n, 2)
    Z = _inverse(X[:-1]) @ X[1:] if n else np.zeros((0, 4, 4))
    om = np.eye(6) if information is None else np.asarray(information, np.float64)
    om = np.broadcast_to(om, (n, 6, 6)).copy()
    return e, Z, om


def closure_edges(query_index, candidates):
    """The verified ``LoopClosureCandidate``s of ``TwoStageRetrieval.query`` as edges: i = ``database_idx``, j =
    ``query_index``, Z = ``transform`` (query into candidate coordinates = X_i^-1 X_j).  GICP's information matrix is
    that of a left perturbation xi in the candidate's frame, T = Exp(xi) Z; the residual of this module is a right one,
    r = Ad(Z^-1) xi to first order, so Omega_r = Ad(Z)^T Omega Ad(Z).  The [t]x term of Ad carries the lever arm of an
    other-lane closure.  -> (edge_ij (M,2) int64, Z (M,4,4), Omega (M,6,6))"""
    e, Z, om = [], [], []
    for c in candidates:
        if not c.verified or c.transform is None or c.information_matrix is None:
            continue
        T = np.asarray(c.transform, np.float64).reshape(4, 4)
        A = adjoint(T)
        W = np.asarray(c.information_matrix, np.float64).reshape(6, 6)
        e.append((int(c.database_idx), int(query_index)))
        Z.append(T)
        om.append(A.T @ (0.5 * (W + W.T)) @ A)
    m = len(e)
    return (np.asarray(e, np.int64).reshape(m, 2), np.asarray(Z, np.float64).reshape(m, 4, 4),
            np.asarray(om, np.float64).reshape(m, 6, 6))


def _log_so3(R):
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = float(np.linalg.norm(v))
    return v if s < 1e-12 else v * (np.arctan2(s, 0.5 * (np.trace(R) - 1.0)) / s)


def relative_covariance(joint_pair, X_i, X_j):
    """The covariance of A = X_i^-1 X_j from the joint marginal of the two poses: ``joint_pair`` (2,2,6,6) is
    ``PoseGraphOptimizer.covariance``'s ``joint`` restricted to (i, j), in that order, i.e. the covariance of the right
    perturbations (delta_i, delta_j) in X_k Exp(delta_k).  To first order X_i^-1 X_j moves by the right perturbation
    delta_A = delta_j - Ad(A^-1) delta_i (this module's Jacobians J_j and J_i with B = I), so Sigma_rel = G Sigma G^T
    with G = [-Ad(A^-1), I].  The block is symmetrised first.  When one of the two poses is fixed its blocks are zero
    and Sigma_rel is the other pose's marginal, carried over.  -> (6,6), rotation first"""
    S = np.asarray(joint_pair, np.float64).reshape(2, 2, 6, 6).transpose(0, 2, 1, 3).reshape(12, 12)
    S = 0.5 * (S + S.T)
    A = _inverse(np.asarray(X_i, np.float64).reshape(4, 4)) @ np.asarray(X_j, np.float64).reshape(4, 4)
    G = np.concatenate([-adjoint(_inverse(A)), np.eye(6)], axis=1)
    return G @ S @ G.T


def closure_mahalanobis(Z, Omega, X_i, X_j, sigma_rel):
    """The gate of a closure candidate (i, j) with measurement ``Z`` ~ X_i^-1 X_j and information ``Omega`` (6,6), both as
    ``closure_edges`` returns them, against the graph *without* that closure: with r = [Log_SO3(R_D); t_D], D = Z^-1
    X_i^-1 X_j, this module's residual, and ``sigma_rel`` = ``relative_covariance`` of the two poses,
    d^2 = r^T (Omega^-1 + Sigma_rel)^-1 r.  For a true closure d^2 follows a chi^2 distribution with 6 degrees of
    freedom: compare it with a quantile, 12.59 for 95 %, 16.81 for 99 %, 22.46 for 99.9 %.  -> float"""
    D = _inverse(np.asarray(Z, np.float64).reshape(4, 4)) @ _inverse(np.asarray(X_i, np.float64).reshape(4, 4)) @ \
        np.asarray(X_j, np.float64).reshape(4, 4)
    r = np.concatenate([_log_so3(D[:3, :3]), D[:3, 3]])
    W = np.asarray(Omega, np.float64).reshape(6, 6)
    S = np.linalg.inv(0.5 * (W + W.T)) + np.asarray(sigma_rel, np.float64).reshape(6, 6)
    return float(r @ np.linalg.solve(S, r))


def _f64(a, dev, shape):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    return t.to(device=dev, dtype=torch.float64).reshape(shape).contiguous()


class PoseGraphOptimizer:
    """Levenberg-Marquardt over SE(3) poses on the device.  Parameters (include/nsc.h NscPoseGraphParams):
    max_iteration, max_pcg_iterations, pcg_tolerance, lambda0, lambda_min, lambda_factor, relative_cost, min_step.
    ``kernel``: None (quadratic), "huber", "cauchy" or "geman_mcclure"; it acts on the edges that the ``robust_scale``
    of a call gives a width.  ``coarse_block``: None (block-Jacobi alone: nothing changes), an int >= 2 (poses per
    aggregate of the two-level preconditioner) or "auto" = max(8, ceil(N / 64)) per call.  Aggregation is by index: it
    assumes consecutive poses are neighbours, as on a trajectory.  At most 128 aggregates."""

    def __init__(self, device="cuda", kernel=None, coarse_block=None, **params):
        self.device = torch.device(device)
        if kernel not in _lib.POSEGRAPH_KERNELS:
            raise _lib.NscError(f"PoseGraphOptimizer: unknown kernel {kernel!r}")
        self.kernel = _lib.POSEGRAPH_KERNELS[kernel]
        if not (coarse_block is None or coarse_block == "auto" or
                (isinstance(coarse_block, (int, np.integer)) and not isinstance(coarse_block, bool) and coarse_block >= 2)):
            raise _lib.NscError(f"PoseGraphOptimizer: coarse_block is None, an int >= 2 or 'auto' (got {coarse_block!r})")
        self.coarse_block = coarse_block
        p = _lib.PoseGraphParams()
        _lib.lib().nsc_posegraph_default_params(C.byref(p))
        names = {n for n, _ in _lib.PoseGraphParams._fields_}
        for k, v in params.items():
            if k not in names:
                raise _lib.NscError(f"PoseGraphOptimizer: unknown parameter {k!r}")
            setattr(p, k, int(v) if k in ("max_iteration", "max_pcg_iterations") else float(v))
        self.params = p

    def _coarse(self, N):
        """poses per aggregate for a graph of N poses; 0 without the coarse space"""
        if self.coarse_block is None:
            return 0
        return max(8, -(-N // 64)) if self.coarse_block == "auto" else int(self.coarse_block)

    def _coarse_within_cap(self, N):
        """``_coarse``, refused where it gives more aggregates than the library takes"""
        block = self._coarse(N)
        if block and -(-N // block) > _lib.POSEGRAPH_MAX_AGGREGATES:
            raise _lib.NscError(f"pose graph: coarse_block {block} gives {-(-N // block)} aggregates of {N} poses; "
                                f"at most {_lib.POSEGRAPH_MAX_AGGREGATES}")
        return block

    @staticmethod
    def _coarse_stats(out, res):
        """``coarse_stats`` of a device result, where the call had a coarse space, read back into ``res``"""
        if "coarse_stats" in out:
            cs = out["coarse_stats"].cpu().numpy()
            res.update(coarse_aggregates=int(cs[0]), coarse_failed=int(cs[1]))
        return res

    def _inputs(self, poses, edge_ij, measurements, information):
        dev = poses.device if isinstance(poses, torch.Tensor) else self.device
        if dev.type != "cuda":
            raise _lib.NscError(f"PoseGraphOptimizer runs on a HIP device (got {dev}); there is no CPU fallback")
        X = _f64(poses, dev, (-1, 4, 4))
        e = edge_ij if isinstance(edge_ij, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(np.asarray(edge_ij, np.int64).reshape(-1, 2)))
        e = e.to(device=dev, dtype=torch.int64).reshape(-1, 2).contiguous()
        E = int(e.shape[0])
        Z = _f64(measurements, dev, (-1, 4, 4))
        om = _f64(information, dev, (-1, 6, 6))
        if int(Z.shape[0]) != E or int(om.shape[0]) != E:
            raise _lib.NscError("pose graph: edge_ij, measurements and information must have one row per edge")
        return dev, X, e, Z, om

    @staticmethod
    def _scale(robust_scale, dev, E):
        """the (E,) widths on the device, or None"""
        if robust_scale is None:
            return None
        if (robust_scale.dim() if isinstance(robust_scale, torch.Tensor) else np.ndim(robust_scale)) != 1:
            raise _lib.NscError("pose graph: robust_scale is one width per edge, shape (E,); give the edges that stay "
                                "quadratic (odometry) the width 0")
        c = _f64(robust_scale, dev, (-1,))
        if int(c.numel()) != E:
            raise _lib.NscError("pose graph: robust_scale must have one entry per edge")
        return c

    def linearize(self, poses, edge_ij, measurements, information, fixed=None, robust_scale=None):
        """The system at ``poses`` (``fixed`` plays no part: every pose gets its row).  -> dict of device tensors:
        residuals (E,6) (never weighted), cost (1,), gradient (N,6) = sum w J^T Omega r, blocks (N,21) = upper triangles
        of the diagonal blocks of H, skipped (1,) int64, and with ``robust_scale`` (E,) weights (E,).  No sync: it can be
        captured."""
        dev, X, e, Z, om = self._inputs(poses, edge_ij, measurements, information)
        N, E = int(X.shape[0]), int(e.shape[0])
        c = self._scale(robust_scale, dev, E)
        f64 = dict(dtype=torch.float64, device=dev)
        out = dict(residuals=torch.empty((E, 6), **f64), cost=torch.empty(1, **f64),
                   gradient=torch.empty((N, 6), **f64), blocks=torch.empty((N, 21), **f64),
                   skipped=torch.empty(1, dtype=torch.int64, device=dev))
        if c is not None:
            out["weights"] = torch.empty(E, **f64)
        L = _lib.lib()
        ws = torch.empty(max(int(L.nsc_posegraph_workspace_bytes(N, E, C.byref(self.params))), 1), dtype=torch.uint8,
                         device=dev)
        _lib.call("nsc_posegraph_linearize_robust", dev, X, N, e, Z, om, E, out["residuals"], out["cost"], out["gradient"],
                  out["blocks"], out["skipped"], ws, int(ws.numel()), _lib.STREAM, self.kernel, c, out.get("weights"))
        return out

    def optimize_device(self, poses, edge_ij, measurements, information, fixed=None, poses_out=None, step0=False,
                        robust_scale=None):
        """``optimize`` without the read-back: device tensors in (or numpy), a dict of device tensors out -- poses
        (N,4,4), stats (10,) as include/nsc.h orders them, cost_history (max_iteration + 1,), step0 (N,6) on request (the
        first delta; not written when max_iteration = 0), and with ``robust_scale`` (E,) chi2 (E,) = r^T Omega r and
        weights (E,) of every edge at the final poses (one more launch; zeros for skipped edges), and with
        ``coarse_block`` coarse_stats (2,) = [aggregates, outer steps whose coarse factor failed].
        Nothing is synchronised, so a call on device tensors can be captured.  ``poses_out`` may be ``poses``."""
        dev, X, e, Z, om = self._inputs(poses, edge_ij, measurements, information)
        N, E = int(X.shape[0]), int(e.shape[0])
        c = self._scale(robust_scale, dev, E)
        fx = self._fixed(fixed, dev, N)
        f64 = dict(dtype=torch.float64, device=dev)
        out = dict(poses=torch.empty((N, 4, 4), **f64) if poses_out is None else poses_out,
                   stats=torch.empty(_lib.POSEGRAPH_STATS, **f64),
                   cost_history=torch.empty(self.params.max_iteration + 1, **f64))
        if out["poses"].dtype != torch.float64 or not out["poses"].is_contiguous() or \
                tuple(out["poses"].shape) != (N, 4, 4) or not out["poses"].is_cuda:
            raise _lib.NscError("pose graph: poses_out must be a contiguous (N,4,4) float64 tensor on the device")
        if step0:
            out["step0"] = torch.empty((N, 6), **f64)         # not written when max_iteration = 0
        if c is not None:
            out["chi2"], out["weights"] = torch.empty(E, **f64), torch.empty(E, **f64)
        L = _lib.lib()
        block = self._coarse_within_cap(N)
        if block:
            out["coarse_stats"] = torch.empty(2, **f64)
            need = L.nsc_posegraph_coarse_workspace_bytes(N, E, block)
        else:
            need = L.nsc_posegraph_workspace_bytes(N, E, C.byref(self.params))
        ws = torch.empty(max(int(need), 1), dtype=torch.uint8, device=dev)
        args = (X, N, e, Z, om, E, fx, self.params, out["poses"], out["stats"], out["cost_history"], out.get("step0"),
                ws, int(ws.numel()), _lib.STREAM, self.kernel, c, out.get("chi2"), out.get("weights"))
        if block:
            _lib.call("nsc_posegraph_optimize_coarse", dev, *args, block, out["coarse_stats"])
        else:
            _lib.call("nsc_posegraph_optimize_robust", dev, *args)
        return out

    def _fixed(self, fixed, dev, N):
        """the (N,) uint8 mask on the device; None fixes pose 0"""
        if fixed is None:
            fx = torch.zeros(N, dtype=torch.uint8, device=dev)
            fx[:1] = 1
            return fx
        fx = fixed if isinstance(fixed, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray((np.asarray(fixed) != 0).astype(np.uint8)))
        if fx.dtype != torch.uint8:                          # a uint8 device tensor is used as it is: no launch
            fx = fx != 0
        fx = fx.to(device=dev, dtype=torch.uint8).reshape(-1).contiguous()
        if int(fx.numel()) != N:
            raise _lib.NscError("pose graph: fixed must have one entry per pose")
        return fx

    def covariance_device(self, poses, edge_ij, measurements, information, nodes, fixed=None, robust_scale=None):
        """Marginal covariances of the poses ``nodes`` (Q,) at ``poses`` (include/nsc.h nsc_posegraph_covariance): Sigma
        is the inverse, over the free poses, of the H that ``linearize`` forms with this optimiser's ``kernel`` and the
        call's ``robust_scale`` -- the covariance of the right perturbations delta_k in X_k Exp(delta_k), rotation first,
        in the gauge the fixed poses set.  Give it the poses ``optimize`` returned.  -> dict of device tensors: joint
        (Q,Q,6,6) with joint[a,b] = Sigma[nodes[a], nodes[b]] (from the columns solved for nodes[b]; not symmetrised),
        residual (Q,6) = |r| of each column's PCG at exit, iterations (Q,6) int32, stats (4,) int64 = [skipped edges, indices outside
        [0,N), selected poses that are not free, columns above ``pcg_tolerance``], and with ``coarse_block``
        coarse_stats (2,).  Every column is a conjugate-gradient solve of its own, capped by ``max_pcg_iterations`` and
        ended at ``pcg_tolerance``: for covariances set the tolerance tight (1e-10) and, on a trajectory, a
        ``coarse_block``.  ``nodes`` as a device int64 tensor is used as it is; nothing is synchronised, so the call can
        be captured.  An index outside [0,N) in a device tensor gives zero rows and columns and is counted."""
        # what the host can refuse, before anything touches the device
        N = int(poses.numel() if isinstance(poses, torch.Tensor) else np.asarray(poses).size) // 16
        sel = nodes.reshape(-1) if isinstance(nodes, torch.Tensor) else np.asarray(nodes, np.int64).reshape(-1)
        Q = int(sel.numel() if isinstance(sel, torch.Tensor) else sel.size)
        if Q > _lib.POSEGRAPH_MAX_COV_NODES:
            raise _lib.NscError(f"pose graph: covariances of at most {_lib.POSEGRAPH_MAX_COV_NODES} poses per call "
                                f"(got {Q})")
        if not (isinstance(sel, torch.Tensor) and sel.is_cuda) and Q and (int(sel.min()) < 0 or int(sel.max()) >= N):
            raise _lib.NscError(f"pose graph: covariance nodes must lie in [0, {N}) (got {int(sel.min())} .. "
                                f"{int(sel.max())})")
        dev, X, e, Z, om = self._inputs(poses, edge_ij, measurements, information)
        E = int(e.shape[0])
        c = self._scale(robust_scale, dev, E)
        fx = self._fixed(fixed, dev, N)
        sel = (sel if isinstance(sel, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(sel))).to(
            device=dev, dtype=torch.int64).contiguous()
        block = self._coarse_within_cap(N)
        f64 = dict(dtype=torch.float64, device=dev)
        out = dict(joint=torch.empty((Q, Q, 6, 6), **f64), residual=torch.empty((Q, 6), **f64),
                   iterations=torch.empty((Q, 6), dtype=torch.int32, device=dev),
                   stats=torch.empty(_lib.POSEGRAPH_COV_STATS, dtype=torch.int64, device=dev))
        if block:
            out["coarse_stats"] = torch.empty(2, **f64)
        L = _lib.lib()
        ws = torch.empty(max(int(L.nsc_posegraph_covariance_workspace_bytes(N, E, Q, block)), 1), dtype=torch.uint8,
                         device=dev)
        _lib.call("nsc_posegraph_covariance", dev, X, N, e, Z, om, E, fx, self.params, sel, Q, out["joint"], out["residual"],
                  out["iterations"], out["stats"], ws, int(ws.numel()), _lib.STREAM, self.kernel, c, block,
                  out.get("coarse_stats"))
        return out

    def covariance(self, poses, edge_ij, measurements, information, nodes, fixed=None, robust_scale=None):
        """``covariance_device`` read back -> dict of numpy arrays: joint (Q,Q,6,6), residual (Q,6), iterations (Q,6),
        converged (Q,6) = residual <= ``pcg_tolerance`` (use only converged columns), and skipped, outside, not_free,
        not_converged as ints; with ``coarse_block`` also coarse_aggregates and coarse_failed.  The pair block of poses i
        and j is ``joint[np.ix_([a, b], [a, b])]`` for nodes[a] = i, nodes[b] = j: hand it to ``relative_covariance``,
        and its result to ``closure_mahalanobis``.  Synchronises."""
        out = self.covariance_device(poses, edge_ij, measurements, information, nodes, fixed, robust_scale)
        res = {k: out[k].cpu().numpy() for k in ("joint", "residual", "iterations")}
        res["converged"] = res["residual"] <= self.params.pcg_tolerance
        res.update(zip(_lib.POSEGRAPH_COV_STAT_NAMES, (int(s) for s in out["stats"].cpu().numpy())))
        return self._coarse_stats(out, res)

    def optimize(self, poses, edge_ij, measurements, information, fixed=None, robust_scale=None):
        """-> dict: poses (N,4,4) (a device tensor for device poses, numpy for numpy), cost0, cost, iterations, accepted,
        rejected, pcg_iterations, converged, cost_history (iterations + 1,), and lambda, skipped, step; the costs are
        robust costs.  ``fixed``: (N,) mask of the poses that stay; None fixes pose 0.  ``robust_scale``: (E,) widths of
        this optimiser's kernel, 0 for the edges that stay quadratic; with it the result has chi2 (E,) and weights (E,)
        as numpy arrays: a closure whose weight ends near 0 was rejected.  With ``coarse_block`` also coarse_aggregates
        and coarse_failed (outer steps whose coarse factor failed and that ran with block-Jacobi alone).  Reads the
        statistics back, so it synchronises."""
        out = self.optimize_device(poses, edge_ij, measurements, information, fixed, robust_scale=robust_scale)
        s = out["stats"].cpu().numpy()
        L = _lib
        its = int(s[L.POSEGRAPH_STAT_ITERATIONS])
        X = out["poses"] if isinstance(poses, torch.Tensor) else out["poses"].cpu().numpy()
        res = dict(poses=X, cost0=float(s[L.POSEGRAPH_STAT_INITIAL_COST]), cost=float(s[L.POSEGRAPH_STAT_FINAL_COST]),
                   iterations=its, accepted=int(s[L.POSEGRAPH_STAT_ACCEPTED]), rejected=int(s[L.POSEGRAPH_STAT_REJECTED]),
                   pcg_iterations=int(s[L.POSEGRAPH_STAT_PCG_ITERATIONS]), converged=bool(s[L.POSEGRAPH_STAT_CONVERGED]),
                   cost_history=out["cost_history"].cpu().numpy()[:its + 1], skipped=int(s[L.POSEGRAPH_STAT_SKIPPED]),
                   step=float(s[L.POSEGRAPH_STAT_STEP]), **{"lambda": float(s[L.POSEGRAPH_STAT_LAMBDA])})
        if robust_scale is not None:
            res.update(chi2=out["chi2"].cpu().numpy(), weights=out["weights"].cpu().numpy())
        return self._coarse_stats(out, res)
