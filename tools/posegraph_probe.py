#!/usr/bin/env python3
"""Pose-graph optimisation (retrieval/pose_graph.py, nsc_posegraph_optimize) on a KITTI-00-shaped graph: 4 541 poses of
synth.make_pose_chain, 4 540 odometry edges with noise (the start is their integration: accumulated drift) and 200
closures between random poses at least 50 frames apart.  Times ``optimize``
  * eagerly: device events around one call, warm, median and spread of ``reps`` calls, and
  * as a replayed hipGraph of the same call,
and, as a host baseline on the same residuals and Jacobians, Gauss-Newton with scipy.sparse.linalg.spsolve on the
normal equations (tests/posegraph_restatement.py builds them, edge by edge, in numpy: the linearisation time is
reported apart from the solve time).  Prints the launch count and the inner iterations per outer step.
usage: posegraph_probe.py [reps=10] [max_pcg_iterations=100] [max_iteration=20] [graph=1] [kernel=none] [width=3]
                          [coarse_block=N|auto] [lambda0=X] [lambda_min=X] [host=0] [cov=Q]
``graph=0`` leaves the capture out (for caps whose launch count makes a graph of several hundred thousand nodes).
``kernel`` = huber, cauchy or geman_mcclure puts that robust kernel, with ``width``, on the closure edges (the odometry
edges stay quadratic) and asks for the per-edge chi2 and weights: one more launch.  The host baseline stays quadratic.
The arguments written name=value may stand anywhere: ``coarse_block`` switches the two-level preconditioner on (poses per
aggregate, or auto), ``lambda0`` and ``lambda_min`` set the damping, ``host=0`` leaves the host baseline out.
``cov=Q`` times ``covariance_device`` instead (marginal covariances of the newest pose and Q - 1 earlier ones, at the poses
one ``optimize`` returns, tolerance 1e-10, ``max_pcg_iterations`` as the cap): eager and replayed, iterations per column,
the worst error against the bar 10 tau |Sigma|_2 of tests/test_posegraph_cov_gpu.py, and as the host row
scipy.sparse.linalg.splu of the same H plus 6 Q solves."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl
import torch
import posegraph_restatement as P
from neural_spectral_codec_amd import _lib as L, synth
from neural_spectral_codec_amd.retrieval import PoseGraphOptimizer

named = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
argv = sys.argv[:1] + [a for a in sys.argv[1:] if "=" not in a]
reps = int(argv[1]) if len(argv) > 1 else 10
max_pcg = int(argv[2]) if len(argv) > 2 else 100
max_it = int(argv[3]) if len(argv) > 3 else 20
with_graph = (int(argv[4]) if len(argv) > 4 else 1) != 0
kernel = argv[5] if len(argv) > 5 and argv[5] != "none" else None
width = float(argv[6]) if len(argv) > 6 else 3.0
coarse_block = named.pop("coarse_block", None)
if coarse_block not in (None, "auto"):
    coarse_block = int(coarse_block)
with_host = int(named.pop("host", 1)) != 0
cov_q = int(named.pop("cov", 0))
damping = {k: float(named.pop(k)) for k in ("lambda0", "lambda_min") if k in named}
assert not named, f"unknown arguments {sorted(named)}"
N, CLOSURES = 4541, 200

rng = np.random.default_rng(0)
truth = synth.make_pose_chain(N, seed=0)
oe = P.chain_edges(N)
oZ = P.noisy(P.relative(truth, oe), rng, rot=0.001, trans=0.01)
init = P.integrate(oZ, truth[0])
a = rng.integers(0, N, (4 * CLOSURES, 2))
ce = a[np.abs(a[:, 0] - a[:, 1]) >= 50][:CLOSURES].astype(np.int64)
cZ = P.noisy(P.relative(truth, ce), rng, rot=0.002, trans=0.02)
e, Z = np.concatenate([oe, ce]), np.concatenate([oZ, cZ])
Om = np.concatenate([np.tile(np.diag([1e6, 1e6, 1e6, 1e4, 1e4, 1e4]), (len(oe), 1, 1)),
                     np.tile(np.diag([2.5e5, 2.5e5, 2.5e5, 2.5e3, 2.5e3, 2.5e3]), (len(ce), 1, 1))])
print(f"graph: {N} poses, {len(oe)} odometry edges, {len(ce)} closures; trajectory error of the start "
      f"{P.trajectory_error(init, truth):.3f} m")

dev = torch.device("cuda")
opt = PoseGraphOptimizer(kernel=kernel, coarse_block=coarse_block, max_pcg_iterations=max_pcg, max_iteration=max_it,
                         **damping)
block = opt._coarse(N)
if block:
    print(f"two-level preconditioner: {block} poses per aggregate, {-(-N // block)} aggregates; {damping}")
args = [torch.from_numpy(x).to(dev) for x in (init, e, Z, Om)]
fixed = torch.zeros(N, dtype=torch.uint8, device=dev)
fixed[0] = 1
scale = None
if kernel is not None:
    scale = torch.zeros(len(e), dtype=torch.float64, device=dev)
    scale[len(oe):] = width
    print(f"robust kernel {kernel}, width {width:g} on the {len(ce)} closure edges")


def call():
    return opt.optimize_device(*args, fixed=fixed, robust_scale=scale)


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = fn()
    g.replay()
    torch.cuda.synchronize()
    return g, cap


def device_times(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1))
    return np.array(out)


if cov_q:
    import posegraph_coarse_restatement as Cr
    TAU = 1e-10
    X = call()["poses"]
    nodes = np.unique(np.concatenate([np.linspace(0.05 * N, 0.95 * N, cov_q - 1).astype(np.int64), [N - 1]]))
    assert len(nodes) == cov_q
    sel = torch.from_numpy(nodes).to(dev)
    cov = PoseGraphOptimizer(kernel=kernel, coarse_block=coarse_block, max_pcg_iterations=max_pcg, pcg_tolerance=TAU)

    def cov_call():
        return cov.covariance_device(X, *args[1:], sel, fixed=fixed, robust_scale=scale)
    res = cov_call()
    torch.cuda.synchronize()
    its, resid = res["iterations"].cpu().numpy(), res["residual"].cpu().numpy()
    print(f"covariance of {cov_q} poses ({6 * cov_q} columns): iterations per column {its.min()} .. {its.max()} (mean "
          f"{its.mean():.1f}), worst residual {resid.max():.3g}, stats {res['stats'].tolist()}; "
          f"{5 + 3 + (9 if block else 2) + (4 if block else 3) * max_pcg + 1} launches per call")
    t = device_times(cov_call, reps)
    print(f"eager: median {np.median(t):.2f} ms (min {t.min():.2f}, max {t.max():.2f}; {reps} calls)")
    if with_graph:
        g, cap = capture(cov_call)
        assert all(torch.equal(cap[k], res[k]) for k in res)
        t = device_times(g.replay, reps)
        print(f"replayed hipGraph: median {np.median(t):.2f} ms (min {t.min():.2f}, max {t.max():.2f}); bitwise the eager "
              "result")
    if with_host:
        Xh = X.cpu().numpy()
        t0 = time.perf_counter()
        H = Cr.linearize(Xh, e, Z, Om, 0 if kernel is None else L.POSEGRAPH_KERNELS[kernel],
                         None if scale is None else scale.cpu().numpy())["H"][6:, 6:].tocsc()
        t1 = time.perf_counter()
        lu = spl.splu(H)
        t2 = time.perf_counter()
        rhs = np.zeros((6 * (N - 1), 6 * cov_q))
        for b, n in enumerate(nodes):
            rhs[6 * (n - 1):6 * n, 6 * b:6 * b + 6] = np.eye(6)
        sol = lu.solve(rhs)
        t3 = time.perf_counter()
        ref = np.stack([np.stack([sol[6 * (na - 1):6 * na, 6 * b:6 * b + 6] for b in range(cov_q)]) for na in nodes])
        lam_min = spl.eigsh(H, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0]
        err = np.abs(res["joint"].cpu().numpy() - ref).max() * lam_min / TAU
        print(f"host: splu {1e3 * (t2 - t1):.0f} ms + {6 * cov_q} solves {1e3 * (t3 - t2):.0f} ms (numpy linearisation "
              f"{1e3 * (t1 - t0):.0f} ms); |Sigma|_2 = 1 / lambda_min(H) = {1.0 / lam_min:.4g}; device error / (tau "
              f"|Sigma|_2) = {err:.3g} (bar 10)")
    sys.exit(0)

out = call()
torch.cuda.synchronize()
s = out["stats"].cpu().numpy()
its, inner = int(s[L.POSEGRAPH_STAT_ITERATIONS]), int(s[L.POSEGRAPH_STAT_PCG_ITERATIONS])
launches = 5 + 1 + 3 + max_it * ((14 + 5 * max_pcg) if block else (8 + 4 * max_pcg)) + 1 + (kernel is not None)
print(f"optimize: {its} outer iterations ({int(s[L.POSEGRAPH_STAT_ACCEPTED])} accepted, "
      f"{int(s[L.POSEGRAPH_STAT_REJECTED])} rejected), {inner} inner iterations ({inner / max(its, 1):.1f} per outer "
      f"step), cost {s[L.POSEGRAPH_STAT_INITIAL_COST]:.6g} -> {s[L.POSEGRAPH_STAT_FINAL_COST]:.6g}, "
      f"converged {bool(s[L.POSEGRAPH_STAT_CONVERGED])}, "
      f"trajectory error {P.trajectory_error(out['poses'].cpu().numpy(), truth):.3f} m; {launches} launches per call")
if block:
    print(f"coarse factor failed in {int(out['coarse_stats'][1].item())} outer steps")
if kernel is not None:
    w = out["weights"].cpu().numpy()[len(oe):]
    print(f"closure weights: min {w.min():.3g}, median {np.median(w):.3g}, max {w.max():.3g}")
t = device_times(call, reps)
print(f"eager: median {np.median(t):.2f} ms (min {t.min():.2f}, max {t.max():.2f}; {reps} calls)")

if with_graph:
    g, cap = capture(call)
    assert all(torch.equal(cap[k], out[k]) for k in out)
    t = device_times(g.replay, reps)
    print(f"replayed hipGraph: median {np.median(t):.2f} ms (min {t.min():.2f}, max {t.max():.2f}); bitwise the eager "
          "result")

if not with_host:
    sys.exit(0)
# host baseline: Gauss-Newton, normal equations of the same residuals and Jacobians, scipy.sparse.linalg.spsolve
X = init.copy()
F = P.cost(X, e, Z, Om)
t_lin = t_solve = 0.0
for it in range(20):
    t0 = time.perf_counter()
    rows, cols, vals, rhs = [], [], [], np.zeros(6 * N)
    blk = np.arange(6)
    for k, (i, j) in enumerate(e):
        r, Ji, Jj = P.edge_terms(X[i], X[j], Z[k])
        W = Om[k]
        for (a_, Ja), (b_, Jb) in (((i, Ji), (i, Ji)), ((i, Ji), (j, Jj)), ((j, Jj), (i, Ji)), ((j, Jj), (j, Jj))):
            rows.append(np.repeat(6 * a_ + blk, 6))
            cols.append(np.tile(6 * b_ + blk, 6))
            vals.append((Ja.T @ W @ Jb).reshape(-1))
        rhs[6 * i:6 * i + 6] -= Ji.T @ W @ r
        rhs[6 * j:6 * j + 6] -= Jj.T @ W @ r
    H = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * N, 6 * N))
    t1 = time.perf_counter()
    d = np.zeros(6 * N)
    d[6:] = spl.spsolve(H[6:, 6:].tocsc(), rhs[6:])
    t2 = time.perf_counter()
    X = np.stack([P.retract(X[k], d[6 * k:6 * k + 6]) for k in range(N)])
    Fn = P.cost(X, e, Z, Om)
    t_lin += t1 - t0
    t_solve += t2 - t1
    done = F - Fn < 1e-9 * F
    F = Fn
    if done:
        break
print(f"host Gauss-Newton (scipy spsolve): {it + 1} iterations, cost {F:.6g}, trajectory error "
      f"{P.trajectory_error(X, truth):.3f} m; spsolve {1e3 * t_solve:.0f} ms in total, numpy linearisation "
      f"{1e3 * t_lin:.0f} ms in total")
