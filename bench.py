#!/usr/bin/env python3
"""Benchmark of the descriptor hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over one batch of synthetic input PER RANK:
    1 024 clouds x 120 000 points (resident in HBM, 1.97 GB)
      -> fused range-image / FFT / histogram encoder (nsc_encode_clouds)
      -> [N > 1] RCCL all-gather of the (1 024, 800) descriptor shards
      -> 3-layer GAT forward over the rank's keyframe range + 6-node halo (nsc_gat_forward)
Work per GPU is fixed as N grows (weak scaling); value = N * 1 024 * K / max-over-ranks time.

For N > 1 either launch this file under torch.distributed.run (one rank per GPU; RANK / LOCAL_RANK / WORLD_SIZE /
MASTER_* from the environment), or call it directly: without WORLD_SIZE in the environment ``python bench.py --gpus N``
starts its own N ranks as fresh child processes (self_launch) and relays rank 0's line.
Prints ONE JSON line on rank 0.

``--dump-outputs DIR`` also writes what the last timed step returned on rank 0 -- the gathered (n_total, 800) descriptors
and the rank's (n_local, 800) GAT embeddings -- as DIR/descriptors.npy and DIR/embeddings.npy (float32, 64 MB at most).
The inputs are seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def self_launch(n_gpus: int) -> int:
    """``python bench.py --gpus N`` called directly (no WORLD_SIZE in the environment) for N > 1: this process becomes a
    launcher that never touches the GPU (it imports neither torch nor anything of the package) -- it starts N fresh child
    processes of this file, one rank per GPU, with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set the way
    ``python -m torch.distributed.run`` would set them, relays rank 0's stdout (the ONE JSON line), sends the other ranks'
    stdout to stderr, and returns non-zero when any child does.  No exec: the children are ordinary subprocesses, and when
    one fails the others are ended by their exact PIDs."""
    import socket
    import subprocess
    import threading
    port = os.environ.get("MASTER_PORT")
    if not port:
        with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
            s.bind(("127.0.0.1", 0))
            port = str(s.getsockname()[1])
    base = dict(os.environ, WORLD_SIZE=str(n_gpus), LOCAL_WORLD_SIZE=str(n_gpus), MASTER_ADDR="127.0.0.1",
                MASTER_PORT=port, NSC_BENCH_SELF_LAUNCHED="1")
    base.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # RCCL's dmabuf IPC (the host driver has no legacy IPC)
    cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
    procs = []
    for r in range(n_gpus):
        env = dict(base, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE if r == 0 else sys.stderr))

    def relay():
        # only rank 0's JSON line goes to stdout; anything a library prints there (gloo announces its peers on stdout)
        # goes to stderr, so that the launcher's stdout stays ONE line
        for raw in procs[0].stdout:
            txt = raw.decode("utf-8", "replace")
            dst = sys.stdout if txt.lstrip().startswith("{") else sys.stderr
            dst.write(txt)
            dst.flush()

    th = threading.Thread(target=relay, daemon=True)
    th.start()
    rc, failed_at = 0, None
    while True:
        codes = [p.poll() for p in procs]
        bad = [c for c in codes if c not in (None, 0)]
        if bad and failed_at is None:
            rc, failed_at = bad[0], time.time()
            print(f"[bench launcher] a rank exited with status {rc}; ending the others", file=sys.stderr)
        if all(c is not None for c in codes):
            break
        if failed_at is not None:
            # the survivors are most likely parked in a collective waiting for the dead rank: give them a moment, then
            # end exactly the processes started above
            age = time.time() - failed_at
            for p in procs:
                if p.poll() is None:
                    if age > 20:
                        p.kill()
                    elif age > 5:
                        p.terminate()
        time.sleep(0.2)
    th.join(timeout=5)
    return rc if rc else max((abs(p.returncode) for p in procs), default=0)


class _stdout_to_stderr:
    """File descriptor 1 -> stderr for the duration (libraries that printf to stdout: RCCL's version banner); the C stdio
    buffer is flushed before the descriptor is restored, or the text would surface on the real stdout at exit."""

    def __enter__(self):
        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        import ctypes
        sys.stdout.flush()
        try:
            ctypes.CDLL(None).fflush(None)
        except OSError:
            pass
        os.dup2(self._saved, 1)
        os.close(self._saved)
        return False


def _early_gpus(argv):
    for i, a in enumerate(argv):
        if a == "--gpus" and i + 1 < len(argv):
            return int(argv[i + 1])
        if a.startswith("--gpus="):
            return int(a.split("=", 1)[1])
    return 1


if __name__ == "__main__" and "WORLD_SIZE" not in os.environ and _early_gpus(sys.argv[1:]) > 1:
    sys.exit(self_launch(_early_gpus(sys.argv[1:])))       # before torch is imported: the launcher stays off the GPU

# RCCL's peer access goes through dmabuf IPC on this platform (the host driver has no legacy IPC): must be in the environment
# before the HIP runtime starts, whoever launched this rank (torch.distributed.run inherits the caller's environment)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np
import torch
import torch.distributed as dist

N_CLOUDS = 1024          # BASELINE.json configs[1]: batch of 1024 synthetic clouds
N_POINTS = 120000        # 120k-pt clouds
BYTES_PER_CLOUD = 16 * N_POINTS + 3200     # algorithmic bytes of the fused encoder
HBM_PEAK_GBS = 8000.0    # MI355X_MICROARCH.md: 8 TB/s HBM3E spec


def usable_cores():
    """Host cores this process may actually run on: the affinity mask, capped by the cgroup CPU quota (a GPU box
    reports every core of the host in os.cpu_count() but grants a share of them)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]) + 0.5)))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, int(q / per + 0.5)))
            break
        except (OSError, ValueError, IndexError):
            continue
    return max(1, n)


def read_clocks():
    """Diagnostic (NSC_BENCH_CLOCKS=1): the active DPM levels and the power reading of card 0 from sysfs."""
    import glob
    out = {}
    for f in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_*")) + sorted(
            glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*/power1_*")) + sorted(
            glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*/freq*_input")):
        try:
            txt = open(f).read().strip()
        except OSError:
            continue
        key = "/".join(f.split("/")[4:5] + f.split("/")[-1:])
        act = [ln for ln in txt.splitlines() if ln.endswith("*")]
        out[key] = act[0] if act else txt[:60]
    return out


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(pts_dev, off_dev, model, n_sample):
    """Oracle ("port") on the host cores: encode n_sample clouds of the SAME workload with the C restatement (a
    work queue over pthreads, one thread per usable core) + the torch-CPU GAT restatement on an n_sample-node
    chain; and the same on ONE core over a quarter of the sample (SURVEY 8d asks for both)."""
    import nsc_oracle as orc
    import gat_oracle as go
    from neural_spectral_codec_amd.keyframe import graph_manager as gm
    from neural_spectral_codec_amd import synth
    import copy
    cores = usable_cores()
    pts = pts_dev[: n_sample * N_POINTS].cpu().numpy()
    off = off_dev[: n_sample + 1].cpu().numpy()
    orc.encode_clouds(pts[: 2 * cores * N_POINTS], off[: 2 * cores + 1], n_threads=cores)     # warm: threads, pages
    PASSES = 3                                   # ~17 core-seconds of CPU work on 16 cores (a bounded sample)
    t0 = time.perf_counter()
    for _ in range(PASSES):
        desc = orc.encode_clouds(pts, off, n_threads=cores)
    t_enc = (time.perf_counter() - t0) / PASSES
    model = copy.deepcopy(model).cpu()
    g = gm.build_chain_graph(torch.from_numpy(desc), 5, "cpu", synth.make_pose_chain(n_sample, 0))

    def gat_time(threads):
        torch.set_num_threads(threads)
        go.forward_reference(model, g)                                               # warm
        t0_ = time.perf_counter()
        go.forward_reference(model, g)
        return time.perf_counter() - t0_

    gat_threads = min(cores, 16)                 # a 1 024-node graph oversubscribes beyond that
    t_gat = gat_time(gat_threads)
    n1 = max(1, min(n_sample // 4, 256))         # one core: ~2.5 s of work
    t0 = time.perf_counter()
    orc.encode_clouds(pts[: n1 * N_POINTS], off[: n1 + 1], n_threads=1)
    t_enc1 = time.perf_counter() - t0
    t_gat1 = gat_time(1)                         # the n_sample-node forward; scaled to n1 nodes below
    one = n1 / (t_enc1 + t_gat1 * n1 / n_sample)
    return {
        "value": n_sample / (t_enc + t_gat), "unit": "keyframes/s", "cores": cores, "kind": "port",
        "one_core_value": one, "cpu_model": cpu_model(), "os_cpu_count": os.cpu_count(),
        "sample": f"{n_sample} of the {N_CLOUDS} x {N_POINTS}-point clouds of this run: oracle/nsc_oracle.c "
                  f"on {cores} threads ({t_enc:.2f} s wall per pass, {PASSES} passes) + torch-CPU GAT restatement ({gat_threads} threads) on a "
                  f"{n_sample}-node chain ({t_gat * 1e3:.1f} ms); one core: {n1} clouds in {t_enc1:.2f} s + the GAT "
                  f"restatement on 1 thread ({t_gat1 * 1e3:.1f} ms per {n_sample} nodes)",
    }, desc


EV_EVERY = 4
CALIB_STEPS = 30
GAT_FLOP_PER_NODE = 2.0 * (800 * 256 + 3 * 256 * 256 + 256 * 800)      # 5.51 GFLOP at N = 4 541
MFMA_F32_PEAK_TFLOPS = 157.3                                           # MI355X_MICROARCH.md: f32-input MFMA


def measure_extras(enc, model, dev, n_local, scratch, uniform):
    """Untimed side measurements reported next to the headline (rank 0, N = 1, after the timed region):
      * the GAT half alone on BASELINE configs[2] (4 541 keyframes, 18 158 edges): HIP-event time per forward and
        the f32-MFMA rate it amounts to (the rocprofv3 counter figures of the same workload are under profiles/);
      * the encoder kernel alone on SENSOR-ORDERED clouds (azimuth-major = HDL-64 firing order, ring-major): the
        LDS-atomic contention case of SURVEY section 7, next to the uniform-order launch."""
    from neural_spectral_codec_amd import synth
    from neural_spectral_codec_amd.keyframe import graph_manager as gm
    out = {}
    gc.collect()
    gc.disable()
    with torch.no_grad():
        inner = getattr(model, "gnn", model)
        was = inner.coresident
        inner.coresident = False
        gat, gat_graph = {}, {}
        for n in (4541, n_local):
            g = gm.synthetic_chain_graph(n, device=dev, seed=1)
            for _ in range(5):
                model(g)
            best = None
            for _ in range(3):              # best of three rounds: a host hiccup (a late gc pass costs ~40 ms) in one
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)   # round must not
                a.record()                                                                           # become the figure
                for _ in range(50):
                    model(g)
                b.record()
                torch.cuda.synchronize(dev)
                us = a.elapsed_time(b) / 50 * 1e3
                best = us if best is None else min(best, us)
            gat[n] = best
            # the same forward replayed as a captured hipGraph (what the pipelined step does with its GNN pass, DESIGN.md
            # section 5): one graph launch instead of eight kernel launches and their Python plumbing
            try:
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    model(g)
                torch.cuda.current_stream(dev).wait_stream(side)
                torch.cuda.synchronize(dev)
                cg = torch.cuda.CUDAGraph()
                with torch.cuda.graph(cg):
                    model(g)
                cg.replay()
                torch.cuda.synchronize(dev)
                bestg = None
                for _ in range(3):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(50):
                        cg.replay()
                    b.record()
                    torch.cuda.synchronize(dev)
                    us = a.elapsed_time(b) / 50 * 1e3
                    bestg = us if bestg is None else min(bestg, us)
                gat_graph[n] = bestg
                del cg
            except Exception as ex:  # noqa: BLE001 -- a side measurement must not take the bench down
                gat_graph[n] = None
                print(f"[bench] hipGraph replay of the GAT forward not measured ({type(ex).__name__}: {ex})", file=sys.stderr)
        inner.coresident = was
        tf = GAT_FLOP_PER_NODE * 4541 / (gat[4541] * 1e-6) / 1e12
        out["roofline_gat"] = {
            "bound": "mfma_f32", "kernel": "gemm_glds_kernel (800->256, 256->800) + 3 x gat_layer_banded_kernel (lin 256->256 + softmax + aggregation + BatchNorm in one launch per layer)",
            "workload": "BASELINE.json configs[2]: 4541 keyframes, 18158 temporal edges, edge_dim=2, eval mode, one GPU",
            "achieved": tf, "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf / MFMA_F32_PEAK_TFLOPS,
            "flop_per_forward": GAT_FLOP_PER_NODE * 4541, "forward_us": gat[4541],
            "forward_us_at_step_size": gat[n_local], "forward_us_as_hipgraph": gat_graph.get(4541),
            "forward_us_at_step_size_as_hipgraph": gat_graph.get(n_local), "traffic": None,
            "note": "whole forward (5 launches) by HIP events; per-kernel durations and the MFMA counters "
                    "(SQ_VALU_MFMA_BUSY_CYCLES, SQ_INSTS_VALU_MFMA_MOPS_F32) are in profiles/r04_gat_n4541_*",
        }
        # the three point orders interleaved, so that clock drift between "then" and "now" cannot pass for an effect of the
        # order: 5 rounds of 8 launches each, median per order
        sets = {"uniform": uniform}
        for order in ("azimuth_major", "ring_major"):
            sets[order] = synth.make_clouds_device(n_local, N_POINTS, dev, seed=77, order=order)
        times = {k: [] for k in sets}
        for k, (pts, off) in sets.items():
            for _ in range(3):
                enc.encode_points_batch((pts, off), out=scratch)
        for _ in range(5):
            for k, (pts, off) in sets.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(8):
                    enc.encode_points_batch((pts, off), out=scratch)
                b.record()
                torch.cuda.synchronize(dev)
                times[k].append(a.elapsed_time(b) / 8)
        orders = {k: float(np.median(v)) for k, v in times.items()}
        del sets
        out["encoder_input_order_ms"] = orders
        try:
            out["incl_h2d"] = measure_h2d(enc, model, dev, n_local, uniform)
            out["latency_us"] = measure_latencies(enc, model, dev)
            out["roofline_train"] = measure_train(dev)
        except Exception as ex:  # noqa: BLE001 -- side measurements must not take the bench down
            print(f"[bench] H2D / latency extras not measured ({type(ex).__name__}: {ex})", file=sys.stderr)
    gc.enable()
    return out


def measure_train(dev):
    """BASELINE configs[4]'s per-batch step (reference src/gnn/trainer.py:186-231: full-graph forward in train mode +
    TripletLoss over 1 024 triplets + backward) on the KITTI-00-shaped graph, replayed as the captured hipGraph GNNTrainer
    runs it as; MFMA work = forward + two backward products per forward product = 3 x 5.51 GFLOP."""
    from neural_spectral_codec_amd.gnn.model import create_spectral_gnn
    from neural_spectral_codec_amd.gnn.trainer import GNNTrainer
    from neural_spectral_codec_amd.keyframe import graph_manager as gm
    n = 4541
    with torch.enable_grad():
        torch.manual_seed(0)
        m = create_spectral_gnn(edge_dim=2, dropout=0.1)
        g = gm.synthetic_chain_graph(n, device=dev, seed=1)
        tr = GNNTrainer(m, device=str(dev), batch_size=1024, accumulation_steps=4, use_graph=True)
        trip = np.random.default_rng(0).integers(0, n, (4096, 3))
        for _ in range(3):
            tr.train_batches(g, trip)
        if not tr._captured:
            raise RuntimeError("the training step was not captured")
        cg = next(iter(tr._captured.values()))[0]
        best = None
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                cg.replay()
            b.record()
            torch.cuda.synchronize(dev)
            us = a.elapsed_time(b) / 20 * 1e3
            best = us if best is None else min(best, us)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(5):
            tr.train_batches(g, trip)
        torch.cuda.synchronize(dev)
        per_batch_ms = (time.perf_counter() - t0) / 5 / 4 * 1e3
        tr.release()
    flop = 3.0 * GAT_FLOP_PER_NODE * n
    tf = flop / (best * 1e-6) / 1e12
    return {"bound": "mfma_f32", "achieved": tf, "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf / MFMA_F32_PEAK_TFLOPS,
            "step_us": best, "flop_per_step": flop, "per_batch_incl_adam_ms": per_batch_ms,
            "workload": "BASELINE.json configs[4] shape on one GPU: 4541 keyframes, 1024 mined-triplet batch, hidden 256, margin 0.1, "
                        "dropout 0.1: forward (train mode) + TripletLoss + backward as ONE captured hipGraph replay "
                        "(~50 kernels: the step is launch- and latency-bound, not MFMA-bound); per_batch_incl_adam_ms = "
                        "GNNTrainer.train_batches with its optimizer step every 4 batches"}


def measure_h2d(enc, model, dev, n_local, uniform):
    """SURVEY 8(d)'s second number: the same step when the boundary hands over HOST buffers -- the batch starts in pinned
    host memory every step; the copy of batch k+1 (second stream) overlaps encoder + GAT of batch k.  PCIe-bound: never
    `value`.  The reference pays a per-keyframe H2D at src/encoding/spectral_encoder.py:224."""
    from neural_spectral_codec_amd.keyframe import graph_manager as gm
    pts, off = uniform
    host = torch.empty(pts.shape, dtype=torch.float32, pin_memory=True)
    host.copy_(pts)
    bufs = [torch.empty_like(pts) for _ in range(2)]
    desc = torch.empty((n_local, 800), dtype=torch.float32, device=dev)
    g = gm.synthetic_chain_graph(n_local, device=dev, seed=1)
    g.x = desc
    copy_s = torch.cuda.Stream(device=dev)
    evs = [torch.cuda.Event() for _ in range(2)]
    cur = torch.cuda.current_stream(dev)

    def run(steps):
        for k in range(steps):
            i = k & 1
            with torch.cuda.stream(copy_s):
                bufs[i].copy_(host, non_blocking=True)
                evs[i].record(copy_s)
            cur.wait_event(evs[i])
            enc.encode_points_batch((bufs[i], off), out=desc)
            model(g)
            copy_s.wait_stream(cur)                          # buffer i is free again two steps later
        torch.cuda.synchronize(dev)

    run(3)
    steps = 8
    t0 = time.perf_counter()
    run(steps)
    dt = (time.perf_counter() - t0) / steps
    del bufs, host
    return {"value": n_local / dt, "unit": "keyframes/s", "ms_per_step": dt * 1e3,
            "pcie_GBps": pts.numel() * 4 / dt / 1e9, "steps": steps,
            "what": f"the {n_local} x {N_POINTS}-point batch starts in PINNED HOST memory every step: H2D copy (second stream, "
                    "batch k+1 under the compute of batch k) + encoder + GAT forward; PCIe-bound, not `value`"}


def measure_latencies(enc, model, dev):
    """Per-call latency of the REFERENCE-SHAPED call sequence (src/pipeline.py:245-274: one encode_points + one
    sliding-window gnn(graph) per keyframe, add_keyframe + stage-1 query against the database; the reference's stated
    targets are latencies, configs/training.yaml:98-99: encoding < 10 ms, query 27 ms @ 100 K database).  Host wall clock
    per call, each call synchronous the way the reference's callers make it (they read the result on the host)."""
    from types import SimpleNamespace
    from neural_spectral_codec_amd import synth
    from neural_spectral_codec_amd.keyframe import graph_manager as gm
    from neural_spectral_codec_amd.retrieval.two_stage_retrieval import TwoStageRetrieval

    def timed(fn, reps, warm=5):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / reps * 1e6

    out = {}
    cloud = synth.make_cloud(0, N_POINTS)
    # pipeline.py:245  descriptor = self.encoder.encode_points(points).detach().cpu().numpy()
    out["encode_points_numpy_120k_incl_h2d_d2h"] = timed(lambda: enc.encode_points(cloud).detach().cpu().numpy(), 100)
    dcloud = torch.from_numpy(cloud).to(dev)
    out["encode_points_device_resident"] = timed(lambda: enc.encode_points(dcloud), 100)
    # pipeline.py:250-256  graph_manager.add_keyframe(kf); graph = get_graph(); embeddings = gnn(graph); update_embeddings
    window = 1000
    mgr = gm.TemporalGraphManager(temporal_neighbors=5, max_active_nodes=window, feature_dim=800, device=str(dev))
    rng = np.random.default_rng(5)
    descs = rng.random((window + 64, 800), dtype=np.float32)
    descs /= descs.sum(1, keepdims=True)
    kid = [0]

    def add_kf():
        kf = SimpleNamespace(keyframe_id=kid[0], descriptor=descs[kid[0] % len(descs)], embedding=None)
        kid[0] += 1
        mgr.add_keyframe(kf)
        return kf

    for _ in range(window):
        add_kf()

    def online_step():
        add_kf()
        emb = model(mgr.get_graph())
        return emb[-1].cpu()                                  # the caller reads the new keyframe's embedding

    out["add_keyframe_plus_gnn_1000_node_window"] = timed(online_step, 60)
    g = mgr.get_graph()
    out["gnn_graph_1000_node_window_synchronous"] = timed(lambda: (model(g), torch.cuda.synchronize(dev)), 100)
    out["gnn_graph_1000_node_window_async_issue"] = timed(lambda: model(g), 100)
    # pipeline.py:259-266  retrieval_system.add_keyframe(kf); get_loop_closures(kf) -- stage 1 on a 100 K database
    n_db = 100000
    ts = TwoStageRetrieval(top_k=10, spatial_filter_distance=50.0, device=str(dev))
    db = torch.rand((n_db, 800), dtype=torch.float32, device=dev) ** 3
    pos = torch.rand((n_db, 3), dtype=torch.float32, device=dev) * 2000.0
    ts.retriever.add_to_database(db, positions=pos)
    ts.keyframes.extend([None] * n_db)                        # stage 1 only needs the count (stage 2 reads the objects)
    pose = np.eye(4)
    q = [0]

    def retrieval_step():
        pose_k = pose.copy()
        pose_k[:3, 3] = (1000.0 + q[0], 1000.0, 0.0)
        kf = SimpleNamespace(keyframe_id=n_db + q[0], descriptor=descs[q[0] % len(descs)], pose=pose_k, points=None)
        q[0] += 1
        ts.add_keyframe(kf)
        return ts.query(kf, verify=False)

    out["add_keyframe_plus_stage1_query_100k_db"] = timed(retrieval_step, 40)
    out["targets_of_the_reference_us"] = {"encoding_time": 10000, "query_latency_100k_db": 27000}
    out["what"] = ("host wall clock per call of the reference-shaped sequence (src/pipeline.py:245-274), synchronous "
                   "where the reference's caller reads the result; targets: configs/training.yaml:98-99")
    del ts, db, pos
    return out


DUMP_BYTES_MAX = 64 << 20


def dump_outputs(out_dir, arrays):
    """--dump-outputs: one DIR/<name>.npy per array.  When together they exceed DUMP_BYTES_MAX (a larger --clouds), each
    array keeps a fixed, seeded sample of its rows, in order, so that two runs with the same arguments still compare row
    for row."""
    os.makedirs(out_dir, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    for name, a in arrays.items():
        if total > DUMP_BYTES_MAX:
            keep = max(1, len(a) * DUMP_BYTES_MAX // total)
            a = a[np.sort(np.random.default_rng(0).choice(len(a), keep, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))
        print(f"[bench] wrote {name}.npy {a.shape} {a.dtype}", file=sys.stderr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (rank 0: the gathered descriptors and its embedding rows) "
                         "as DIR/<name>.npy in float32, for output-for-output comparison of two builds")
    ap.add_argument("--clouds", type=int, default=N_CLOUDS, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-sample", type=int, default=1024, help=argparse.SUPPRESS)
    ap.add_argument("--no-cpu-baseline", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-extras", action="store_true", help=argparse.SUPPRESS)   # skip the untimed side measurements
    ap.add_argument("--gnn-kernels", choices=["auto", "lds", "direct", "shared_b"], default="auto", help=argparse.SUPPRESS)
    ap.add_argument("--ev-every", type=int, default=EV_EVERY, help=argparse.SUPPRESS)   # time every n-th encoder launch
    ap.add_argument("--serial", action="store_true", help=argparse.SUPPRESS)      # force the one-stream path
    ap.add_argument("--pipelined", action="store_true", help=argparse.SUPPRESS)   # force the software-pipelined path
    # consecutive encoder launches alternate over this many streams (2: they overlap); 0 = let the calibration choose
    ap.add_argument("--enc-streams", type=int, default=0, choices=[0, 1, 2], help=argparse.SUPPRESS)
    ap.add_argument("--one-batch", action="store_true", help=argparse.SUPPRESS)      # every step reads the same batch
    ap.add_argument("--calibrate", action="store_true", help=argparse.SUPPRESS)      # time all three step implementations
    ap.add_argument("--calibrate2", action="store_true", help=argparse.SUPPRESS)     # the N > 1 choice (pipelined2 / serial) at N = 1
    ap.add_argument("--gnn-streams", type=int, default=1, help=argparse.SUPPRESS)    # GNN passes alternate over this many streams
    ap.add_argument("--gnn-graph", type=int, default=-1, help=argparse.SUPPRESS)     # GNN forward as a replayed hipGraph: 1 / 0, -1 = the path's default
    ap.add_argument("--gnn-nodes", type=int, default=0, help=argparse.SUPPRESS)      # DIAGNOSTIC: GNN over the first n keyframes only
    ap.add_argument("--gnn-burn", default="", help=argparse.SUPPRESS)                # DIAGNOSTIC: MODE:WGS:PER_WAVE[:LAUNCHES] synthetic co-runner (nsc_debug_burn) in place of the GNN
    ap.add_argument("--no-gnn", action="store_true", help=argparse.SUPPRESS)         # DIAGNOSTIC (not the metric): identity in place of the GNN
    ap.add_argument("--pipe-buffers", type=int, default=0, help=argparse.SUPPRESS)   # descriptor buffers in rotation (0 = the path's default)
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.gpus > 1 and world == 1:
        # (python bench.py --gpus N without WORLD_SIZE never gets here: self_launch() above starts the N ranks)
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE=1: unset WORLD_SIZE to let bench.py start its own ranks, or "
                         "launch with python -m torch.distributed.run --nnodes=1 --nproc-per-node N "
                         "--master-addr 127.0.0.1 --master-port P bench.py --gpus N ...")
    # NSC_BENCH_REHEARSAL=1: rehearse the N > 1 code path on a ONE-GPU box (all ranks share cuda:0,
    # collectives over gloo).  Never used for reported numbers.
    rehearsal = os.environ.get("NSC_BENCH_REHEARSAL") == "1"
    dev_index = 0 if rehearsal else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    # NSC_BENCH_RCCL_WORLD1=1 (with --gpus 1): ONE rank, but in the N > 1 shape -- an RCCL process group of one rank, and every
    # collective of the N > 1 step, calibration and line really issued through it (the backend's stream semantics and
    # its kernels beside the encoder grid, on the one card a gpurun box has).  Never used for reported numbers.
    rccl1 = world == 1 and os.environ.get("NSC_BENCH_RCCL_WORLD1") == "1"
    multi = world > 1 or rccl1
    # self-description of the N > 1 line: how many ranks the communicator really joined (an all-reduce of ones), on what
    rccl_ranks, backend = 1, None
    if multi:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # RCCL prints a five-line version banner on STDOUT when rank 0's communicator comes up (C stdio, not Python's): the
        # contract is ONE JSON line on stdout, so file descriptor 1 points at stderr until the first collective has run
        with _stdout_to_stderr():
            if rccl1:
                os.environ.setdefault("MASTER_PORT", "29517")
                dist.init_process_group("nccl", device_id=dev, rank=0, world_size=1)
            elif rehearsal:
                dist.init_process_group("gloo")
            else:
                dist.init_process_group("nccl", device_id=dev)
            ones = torch.ones(1, dtype=torch.float32, device=dev)
            dist.all_reduce(ones)
            rccl_ranks, backend = int(round(float(ones.item()))), str(dist.get_backend())
            dist.barrier()
            torch.cuda.synchronize(dev)

    from neural_spectral_codec_amd import synth
    from neural_spectral_codec_amd import distributed as nd
    from neural_spectral_codec_amd.encoding import SpectralEncoder
    from neural_spectral_codec_amd.gnn.model import create_spectral_gnn

    if args.pipe_buffers > 0:
        nd.ShardedDescriptorPath._PIPE_BUFFERS = args.pipe_buffers
    n_local = args.clouds
    n_total = n_local * world
    enc = SpectralEncoder(n_elevation=16, n_azimuth=360, n_bins=50, alpha=2.0,
                          target_elevation_bins=16).to(dev)
    torch.manual_seed(0)                                    # identical random-init weights on all ranks
    model = create_spectral_gnn(input_dim=800, hidden_dim=256, output_dim=800, n_layers=3,
                                dropout=0.1, edge_dim=2)
    synth.randomize_bn_stats(model)
    model = model.to(dev).eval()
    pts, off = synth.make_clouds_device(n_local, N_POINTS, dev, seed=1234 + rank)
    # Consecutive steps read DIFFERENT batches (two resident sets of n_local clouds, alternating): launches of
    # consecutive steps overlap on the device, and two launches streaming the same 1.97 GB could meet each other's
    # lines in the 256 MB Infinity Cache -- bytes that would not have come from HBM.  --one-batch restores round 2's
    # single resident batch.
    batches = [(pts, off)]
    if not args.one_batch:
        batches.append(synth.make_clouds_device(n_local, N_POINTS, dev, seed=99991 + rank))
    nbat = len(batches)
    step_no = [0]

    def next_batch():
        b = batches[step_no[0] % nbat]
        step_no[0] += 1
        return b
    poses = synth.make_pose_chain(n_total, 0)
    # Two implementations of the same step: "pipelined" = consecutive steps software-pipelined
    # on two HIP streams (encoder of batch k+1 over the exchange + GNN of batch k), "serial" = one stream.  Every
    # step does the full work of the metric in both.  Unless --serial / --pipelined forces one, a short UNTIMED
    # calibration after the spin-up picks the faster one for this box / world size (all ranks agree through an
    # all-reduce) -- the N > 1 pipelined path meets RCCL kernels it could not be measured against in round 1.
    desc_local = torch.empty((n_local, 800), dtype=torch.float32, device=dev)

    class _Enc:                                             # serial path: encode into a fixed output buffer
        alpha = enc.alpha

        @staticmethod
        def encode_points_batch(clouds):
            return enc.encode_points_batch(clouds, out=desc_local)

    class _NoGnn:                                           # --no-gnn: what the step machinery costs without the GNN's kernels
        def __call__(self, g):
            return g.x

    class _BurnGnn:                                         # --gnn-burn MODE:WGS:PER_WAVE[:LAUNCHES]: a synthetic co-runner of ONE resource
        def __init__(self, spec):
            from neural_spectral_codec_amd import _lib as L_
            f = [int(v) for v in spec.split(":")]
            self.mode, self.wgs, self.per_wave, self.launches = f[0], f[1], f[2], (f[3] if len(f) > 3 else 1)
            self.L, self.lib = L_, L_.lib()
            if not hasattr(self.lib, "nsc_debug_burn"):
                raise SystemExit("--gnn-burn needs a development build of the library (NSC_DEV_BUILD=1 python "
                                 "neural-spectral-codec_amd/build.py): the product library has no nsc_debug_burn")
            self.scratch = torch.rand(1 << 19, dtype=torch.float32, device=dev)          # 2 MB

        def __call__(self, g):
            for _ in range(self.launches):
                self.L.check(self.lib.nsc_debug_burn(self.mode, self.wgs, self.per_wave, self.L.ptr(self.scratch),
                                                     self.scratch.numel() * 4, self.L.stream_ptr(dev)), "nsc_debug_burn")
            return g.x

    class _PartGnn:                                         # --gnn-nodes n: is the GNN's cost beside the encoder work- or launch-bound?
        def __init__(self, n):
            from neural_spectral_codec_amd.keyframe import graph_manager as gm_
            self.n, self.g = n, gm_.synthetic_chain_graph(n, device=dev, seed=1)

        def __call__(self, g):
            self.g.x = g.x[:self.n]
            out = torch.empty_like(g.x)
            out[:self.n] = model(self.g)
            return out

    def make_path(pipelined, enc_streams=1):
        gnn_ = (_BurnGnn(args.gnn_burn) if args.gnn_burn else _NoGnn() if args.no_gnn
                else (_PartGnn(args.gnn_nodes) if args.gnn_nodes else model))
        p_ = nd.ShardedDescriptorPath(enc, gnn_, n_total, poses, pipeline=pipelined,
                                      encoder_streams=enc_streams,
                                      gnn_streams=args.gnn_streams, gnn_graph=None if args.gnn_graph < 0 else bool(args.gnn_graph),
                                      rehearse_collectives=rccl1)
        if not pipelined:
            p_.encoder = _Enc
        return p_

    inner_gnn = getattr(model, "gnn", model)
    # Three implementations of the same step: "pipelined2" = software pipeline with consecutive encoder launches
    # overlapping on two streams, "pipelined1" = the round-2 form (one encoder stream), "serial".
    # One GPU: pipelined2, no calibration -- it won every interleaved comparison of round 3 (3.19-3.38 M keyframes/s
    # against 3.02 / 2.78 M); a calibration would only add a synchronise-heavy phase before the measurement.  N > 1: the
    # pipelined paths meet RCCL kernels they could not be measured against, so a short untimed calibration picks among
    # the three (all ranks agree through an all-reduce).  --calibrate: all three at N = 1 too.
    paths = {}
    want = []
    if args.serial:
        want = ["serial"]
    elif args.pipelined:
        want = ["pipelined1" if args.enc_streams == 1 else "pipelined2"]
    elif args.calibrate:
        want = ["pipelined2", "pipelined1", "serial"]
    elif not multi and not args.calibrate2:
        want = ["pipelined1" if args.enc_streams == 1 else "pipelined2"]
    elif args.calibrate2:
        want = ["pipelined2", "serial"]
    else:
        # N > 1: RCCL's all-gather kernel has to find room beside the resident encoder grid -- with overlapping launches
        # there is no gap between two encoder launches any more, with one encoder stream there is: let the box decide
        want = (["pipelined2"] if args.enc_streams != 1 else []) + ["pipelined1", "serial"]
    for name_ in want:
        paths[name_] = make_path(name_ != "serial", 2 if name_ == "pipelined2" else 1)
    for name_, p_ in paths.items():
        p_.coresident_gnn = (name_ != "serial" and args.gnn_kernels != "lds") and ("shared_b" if args.gnn_kernels == "shared_b" else True)
    path = next(iter(paths.values()))

    def sync():
        path.synchronize()                                  # both pipeline streams drained into the current one
        torch.cuda.synchronize(dev)
        if multi:
            dist.barrier()
            torch.cuda.synchronize(dev)

    def use(name):
        nonlocal path
        path = paths[name]
        # LDS-free GNN kernels only where they co-run with a resident encoder grid
        inner_gnn.coresident = ((name != "serial") if args.gnn_kernels == "auto" else
                                {"direct": True, "lds": False, "shared_b": "shared_b"}[args.gnn_kernels])

    SPINUP_STEPS = 40    # untimed device spin-up (clock ramp, TLB/first touch): ~16 ms, part of setup
    calib = None
    # Host-side housekeeping goes HERE, before the device is spun up: a gc.collect() (~40 ms) or an event allocation
    # between the warmup and t0 leaves the device idle long enough to drop its clocks, and the first ~20 launches
    # after such a pause run 20 % slower (round-1 BENCH: 0.446 ms/step at --steps 20 against 0.370 at --steps 200).
    # From the spin-up to the end of the timed region the device is never idle for more than a synchronize().
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    solo = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
    scratch = torch.empty((n_local, 800), dtype=torch.float32, device=dev)
    # streams of the encoder-alone reference measurement, picked (hardware-queue probe: ~20 ms of an almost idle device)
    # HERE, before the spin-up -- an idle stretch right before a measurement lets the device drop its clocks
    s2, _ = nd.concurrent_streams(dev, 2)
    gc.collect()
    gc.disable()                                            # no collector pause on the enqueueing thread
    with torch.no_grad():
        for name in paths:                                  # the first step also builds the cached graph
            use(name)
            for _ in range(max(SPINUP_STEPS - args.warmup, 1)):
                path.step(next_batch(), inputs_ready=True)
            sync()
        if len(paths) == 1:
            use(next(iter(paths)))
        else:
            calib, calib_all = {}, {}
            for rnd in range(2):
                for name in paths:
                    use(name)
                    sync()
                    tc = time.perf_counter()
                    for _ in range(CALIB_STEPS):
                        path.step(next_batch(), inputs_ready=True)
                    sync()
                    calib[name] = min(calib.get(name, 1e9), (time.perf_counter() - tc) / CALIB_STEPS)
                    calib_all.setdefault(name, []).append(round((time.perf_counter() - tc) / CALIB_STEPS * 1e3, 4))
            names = list(paths)
            tcal = torch.tensor([calib[n_] for n_ in names], dtype=torch.float64, device=dev)
            if multi:
                dist.all_reduce(tcal, op=dist.ReduceOp.MAX)
            calib = {f"{n_}_ms_per_step": float(tcal[i_]) * 1e3 for i_, n_ in enumerate(names)}
            calib["steps_each"] = 2 * CALIB_STEPS
            calib["rounds_ms_per_step_rank0"] = calib_all
            best = names[int(torch.argmin(tcal))]
            if best != "serial" and os.environ.get("NSC_BENCH_KEEP_PATH") != "1":     # (diagnostic: keep the calibrated object)
                # The timed region runs on a FRESH path object (new streams), spun up after the calibration.  Round 3: the
                # first multi-path process on a fresh box ran its timed region 8-10 % slower on the path object it had
                # calibrated (7 of 7 boxes; the same path calibrated fast, launches overlapped, distinct hardware queues);
                # on a fresh object it does not (2 of 2 boxes: 3.21 / 3.25 M keyframes/s).  Cause unknown; the state
                # sticks to the streams a path has used through the synchronise-heavy calibration.
                paths[best] = make_path(True, 2 if best == "pipelined2" else 1)
                paths[best].coresident_gnn = args.gnn_kernels != "lds"
                use(best)
                for _ in range(SPINUP_STEPS):
                    path.step(next_batch(), inputs_ready=True)
                sync()
            use(best)
        chosen = [n_ for n_, p_ in paths.items() if p_ is path][0]
        for _ in range(args.warmup):                        # the W untimed warmup steps of the contract
            path.step(next_batch(), inputs_ready=True)
        if multi:
            # HIP events around the descriptor all-gather, on the stream it is issued on (every step's; allocated here,
            # outside the timed region)
            path.collective_events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                                      for _ in range(args.steps)]
        sync()                                              # barrier + synchronize: microseconds of idle, no more
        t0 = time.perf_counter()
        for k in range(args.steps):
            # HIP events on the stream the encoder kernel is launched on -> live figures for the roofline object: the END
            # of every launch is time-stamped (the completion event the GNN stream waits on anyway; launch period =
            # time between consecutive completions), every EV_EVERY-th launch also gets a start stamp (per-launch
            # duration; a start + end pair costs its stream ~5 us of idle, kernel traces of round 2).
            last_batch = next_batch()
            desc_all, emb = path.step(last_batch, encoder_events=(ev[k][0] if k % args.ev_every == 0 else None, ev[k][1]),
                                      inputs_ready=True)
        t_issue = time.perf_counter() - t0                  # host side only: all K steps enqueued
        clocks_busy = read_clocks() if os.environ.get("NSC_BENCH_CLOCKS") == "1" else None   # device still mid-run
        sync()
        dt = time.perf_counter() - t0
        gc.enable()
        # read back before anything else runs on the device (the path's buffers rotate, a captured forward's output is reused)
        dumped = ({"descriptors": desc_all.float().cpu().numpy(), "embeddings": emb.float().cpu().numpy()}
                  if args.dump_outputs and rank == 0 else None)
        if chosen != "serial":
            desc_local = desc_all[rank * n_local:(rank + 1) * n_local] if multi else desc_all
        # outside the timed region: the same kernel alone on the device (no GNN co-running), for reference --
        # (a) one launch at a time on one stream, (b) consecutive launches overlapping on two streams
        for a, b in solo:
            a.record()
            enc.encode_points_batch((pts, off), out=scratch)
            b.record()
        torch.cuda.synchronize(dev)
        solo_ms = float(np.mean([a.elapsed_time(b) for a, b in solo]))
        scratch2 = [scratch, torch.empty_like(scratch)]
        ends = [torch.cuda.Event(enable_timing=True) for _ in range(24)]
        for st in s2:
            st.wait_stream(torch.cuda.current_stream(dev))
        for j, e in enumerate(ends):
            with torch.cuda.stream(s2[j % 2]):
                enc.encode_points_batch(batches[j % nbat], out=scratch2[j % 2])
                e.record(s2[j % 2])
        torch.cuda.synchronize(dev)
        solo_period_ms = ends[3].elapsed_time(ends[-1]) / (len(ends) - 4)
        extras = {}
        if rank == 0 and not multi and not args.no_extras:
            extras = measure_extras(enc, model, dev, n_local, scratch, (pts, off))
    t = torch.tensor([dt], dtype=torch.float64, device=dev)
    per_rank_ms, allgather = None, None
    if multi:
        tl = torch.zeros(world, dtype=torch.float64, device=dev)
        dist.all_gather_into_tensor(tl, t)
        per_rank_ms = [float(v) / args.steps * 1e3 for v in tl.tolist()]
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        # the descriptor all-gather: in situ (events of the timed region: from the moment the GNN stream reaches the
        # collective to its completion, beside the resident encoder grid) and alone on an idle device afterwards
        ce = [a.elapsed_time(b) for a, b in (path.collective_events or []) if a.query() and b.query()]
        ga = torch.empty((n_total, 800), dtype=torch.float32, device=dev)
        dist.all_gather_into_tensor(ga, desc_local.contiguous())
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            dist.all_gather_into_tensor(ga, desc_local.contiguous())
        b.record()
        torch.cuda.synchronize(dev)
        alone_ms = a.elapsed_time(b) / 20
        allgather = {"in_situ_ms": float(np.mean(ce)) if ce else None, "in_situ_max_ms": float(np.max(ce)) if ce else None,
                     "events": len(ce), "alone_ms": alone_ms, "bytes_per_rank": n_local * 3200,
                     "alone_bus_GBps": (world - 1) * n_local * 3200 / (alone_ms * 1e-3) / 1e9}
        del ga
    dt = float(t.item())
    enc_ms = float(np.mean([a.elapsed_time(b) for a, b in ev[::args.ev_every]]))
    # launch period in the timed region: completion to completion.  Steady state: the first RAMP launches after the
    # synchronise before t0 are left out (the first launch runs alone, the second starts a host-issue time later: their
    # completions are 340-370 us apart, the steady state's 300-310); the whole region's figure is reported beside it.
    # ... and the LAST interval too (round 4): the final launch drains without a successor streaming beside it, its
    # completion comes early (251 us against 300 in the round-3 driver run) and would flatter the in-situ figure.
    RAMP = 4 if args.steps >= 12 else 0
    DRAIN = 1 if args.steps >= 12 else 0
    period_all_ms = ev[0][1].elapsed_time(ev[-1][1]) / (args.steps - 1) if args.steps > 1 else enc_ms
    nper = args.steps - 1 - RAMP - DRAIN
    period_ms = (ev[RAMP][1].elapsed_time(ev[-1 - DRAIN][1]) / nper) if nper > 0 else period_all_ms
    overlapped = chosen == "pipelined2"

    if rank == 0:
        value = n_total * args.steps / dt
        # Launches that overlap (pipelined2) have no meaningful per-launch duration -- two are resident at a time, each
        # takes about two periods -- so the roofline figure is defined on the launch PERIOD there: algorithmic bytes of
        # one launch / time between consecutive launch completions.  One launch at a time: bytes / launch duration.
        roof_ms = period_ms if overlapped else enc_ms
        achieved = n_local * BYTES_PER_CLOUD / (roof_ms * 1e-3) / 1e9
        traffic = None
        tpath = os.path.join(ROOT, "profiles", "encoder_traffic.json")
        if os.path.exists(tpath):
            try:
                traffic = json.load(open(tpath)).get("hbm_bytes_per_launch") if n_local == N_CLOUDS else None
            except Exception:  # noqa: BLE001
                traffic = None
        line = {
            "metric": "keyframes/sec (encode+GAT fwd), 120k-pt clouds" + (" -- DIAGNOSTIC RUN WITHOUT THE FULL GNN, not the metric" if (args.no_gnn or args.gnn_nodes or args.gnn_burn) else ""),
            "value": value, "unit": "keyframes/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "host_issue_ms_per_step": t_issue / args.steps * 1e3, "higher_is_better": True,
            "clocks_mid_run": clocks_busy,
            "stream_debug": {"hw_queue_classes": getattr(path, "queue_classes", None), "pipe_buffers": nd.ShardedDescriptorPath._PIPE_BUFFERS,
                             "encoder_waits_for_gnn": getattr(path, "gnn_waits", None),
                             "launch_end_intervals_us": [round(ev[k][1].elapsed_time(ev[k + 1][1]) * 1e3, 1)
                                                         for k in range(min(args.steps, 64) - 1)],
                             # --ev-every 1: (start, end) of every launch relative to the first start
                             "launch_windows_us": ([(round(ev[0][0].elapsed_time(ev[k][0]) * 1e3, 1),
                                                     round(ev[0][0].elapsed_time(ev[k][1]) * 1e3, 1))
                                                    for k in range(min(args.steps, 64))] if args.ev_every == 1 else None)},
            "rccl_ranks": rccl_ranks, "backend": backend, "ms_per_step_by_rank": per_rank_ms, "allgather": allgather,
            "launched_by": ("bench.py itself (N fresh child processes)" if os.environ.get("NSC_BENCH_SELF_LAUNCHED") == "1"
                            else "torch.distributed.run / caller" if world > 1 else
                            "single process (RCCL world-1 rehearsal)" if rccl1 else "single process"),
            "step_path": "serial" if chosen == "serial" else "pipelined",
            "encoder_streams": {"pipelined2": 2, "pipelined1": 1}.get(chosen, 1), "calibration": calib,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic" + (" (REHEARSAL: ranks share one GPU, gloo)" if rehearsal else "")
                    + (" (REHEARSAL: one rank in the N > 1 shape, every collective through a one-rank RCCL group)" if rccl1 else ""),
            "config": {
                "workload": f"{n_local} clouds x {N_POINTS} points per GPU, i.i.d. uniform points in random order "
                            f"(BASELINE.json configs[1]; sensor-ordered clouds: roofline.standalone_launch_ms_by_input_order) "
                            f"+ 3-layer GAT forward over the {n_local}-keyframe temporal chain "
                            f"(5 temporal neighbours, edge_dim=2, eval mode)"
                            + (f", RCCL all-gather of {world} x ({n_local},800) f32 descriptor shards"
                               if world > 1 else ""),
                "clouds_per_gpu": n_local, "points_per_cloud": N_POINTS, "descriptor_dim": 800,
                "gat": "800->256->GATx3->800", "parallelism": f"keyframe-shard x{world}",
            },
            "roofline": {
                "bound": "hbm", "kernel": "encode_fast_kernel", "achieved": achieved,
                "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                "achieved_defined_on": ("launch period: algorithmic bytes of one launch / time between consecutive launch "
                                        "completions in the steady state of the timed region (its first %d launches, the "
                                        "pipeline's ramp after the synchronise before t0, and its last %d, which drains "
                                        "without a successor, left out; consecutive launches "
                                        "overlap on two streams, two are resident at a time)" % (RAMP, DRAIN) if overlapped else
                                        "launch duration: algorithmic bytes of one launch / HIP-event time around the launch"),
                "traffic": traffic,
                "traffic_source": "profiles/encoder_traffic.json (PMC FETCH_SIZE + WRITE_SIZE, separate rocprofv3 run; not a same-run counter)",
                "launch_period_ms": period_ms, "launch_period_whole_region_ms": period_all_ms, "launch_ms": enc_ms, "launches_timed": len(ev[::args.ev_every]),
                "co_running": None if chosen == "serial" else "GNN forward of the previous batch on a second stream"
                              + ("; the next encoder launch on a second encoder stream" if overlapped else ""),
                "standalone_launch_ms": solo_ms,
                "standalone_frac": n_local * BYTES_PER_CLOUD / (solo_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "standalone_overlapped_period_ms": solo_period_ms,
                "standalone_overlapped_frac": n_local * BYTES_PER_CLOUD / (solo_period_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "algorithmic_bytes_per_launch": n_local * BYTES_PER_CLOUD,
            },
        }
        if extras:
            line["roofline_gat"] = extras["roofline_gat"]
            if "incl_h2d" in extras:
                line["value_incl_h2d"] = extras["incl_h2d"]["value"]
                line["incl_h2d"] = extras["incl_h2d"]
            if "latency_us" in extras:
                line["latency_us"] = extras["latency_us"]
            if "roofline_train" in extras:
                line["roofline_train"] = extras["roofline_train"]
            # the headline workload is the uniform-order batch; the same kernel alone on sensor-ordered clouds:
            line["roofline"]["standalone_launch_ms_by_input_order"] = dict(extras["encoder_input_order_ms"])
        if world == 1 and not args.no_cpu_baseline:
            cb, odesc = cpu_baseline(last_batch[0], last_batch[1], model, min(args.cpu_sample, n_local))   # the batch of the last step
            line["cpu_baseline"] = cb
            # parity gate next to the number: sample of this run's descriptors vs the oracle
            got = desc_local[: odesc.shape[0]].cpu().numpy()
            line["parity"] = {
                "descriptor_max_abs_err_vs_oracle": float(np.abs(got - odesc).max()),
                "ok": bool(np.all(np.abs(got - odesc) <= 1e-6 * np.abs(odesc) + 1e-9)),
            }
        if dumped is not None:
            dump_outputs(args.dump_outputs, dumped)
        print(json.dumps(line), flush=True)
    if multi:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
