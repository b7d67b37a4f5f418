#!/usr/bin/env python3
"""Stage 2 of loop closing from a store of prepared clouds (PreparedClouds): times, on ray-cast scans of one
synthetic world (synth.scan_world, about 120 000 points each at n_azimuth=1950),
  * PreparedClouds.add of one scan and of 10 scans (one nsc_gicp_prepare call each);
  * GeometricVerifier.verify_prepared of 1 query x 10 candidates, next to verify_batch on the raw scans;
  * batch_loop_closing(verify=True) over a sequence of ``n_seq`` scans that drives out and comes back beside its start
    (every scan queries the database of all scans, top-10, random descriptors), per query and with
    prepare_geometry=True.
usage: gicp_store_workload.py [reps=10] [n_seq=200] [section=all|verify]
Host clock around synchronised calls.  ``section=verify`` runs only the 1 x 10 verify_prepared loop (for
``rocprofv3 --kernel-trace --stats``)."""
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from neural_spectral_codec_amd import synth
from neural_spectral_codec_amd.retrieval import GeometricVerifier, batch_loop_closing

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
n_seq = int(sys.argv[2]) if len(sys.argv) > 2 else 200
section = sys.argv[3] if len(sys.argv) > 3 else "all"


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, out


world = synth.make_world(3)
query = synth.scan_world(world, synth.pose_xyz_yaw(0, 0), seed=1, n_azimuth=1950)
cands = [synth.scan_world(world, synth.pose_xyz_yaw(0.1 * i, -0.05 * i, 0.0, 0.5 * i), seed=2 + i, n_azimuth=1950)
         for i in range(10)]
v = GeometricVerifier()
qs, store = v.prepare([query]), v.prepare(cands)
ids = list(range(10))
if section == "verify":
    dt, _ = timed(lambda: v.verify_prepared(qs, 0, store, ids), reps)
    print(f"verify_prepared 1x10 {dt * 1e3:.3f} ms")
    sys.exit(0)

rows = [int(store.cloud(i)["points"].shape[0]) for i in ids]
print(f"points/scan {len(query)}  down-sampled rows/scan {np.mean(rows):.0f} (min {min(rows)}, max {max(rows)})  "
      f"store bytes/keyframe {np.mean(rows) * (3 + 6 + 4) * 8 + 48:.0f} (+ capacity slack; store.nbytes "
      f"{store.nbytes})")


def prep(clouds):
    s = v.prepare()
    s.add(clouds)
    return s


dt1, _ = timed(lambda: prep([query]), reps)
dt10, _ = timed(lambda: prep(cands), reps)
print(f"prepare 1 scan {dt1 * 1e3:.2f} ms   prepare 10 scans {dt10 * 1e3:.2f} ms ({dt10 * 1e2:.2f} ms/scan)")
dtp, res_p = timed(lambda: v.verify_prepared(qs, 0, store, ids), reps)
dtb, res_b = timed(lambda: v.verify_batch(query, cands), max(1, reps // 2))
same = all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() for a, b in zip(res_p, res_b))
print(f"verify_prepared 1x10 {dtp * 1e3:.3f} ms   verify_batch 1x10 {dtb * 1e3:.2f} ms   "
      f"verified {sum(r[0] for r in res_p)}/10  bitwise equal {same}")

# a sequence out and back: 1 m steps along x, then back along y = 1.5 m (revisits of the way out)
half = n_seq // 2
poses = [synth.pose_xyz_yaw(1.0 * i, 0.0, 0.0, 0.0) for i in range(half)] + \
        [synth.pose_xyz_yaw(1.0 * (n_seq - 1 - i), 1.5, 0.0, 3.0) for i in range(half, n_seq)]
t0 = time.perf_counter()
scans = [synth.scan_world(world, P, seed=100 + i, n_azimuth=1024) for i, P in enumerate(poses)]
print(f"sequence: {n_seq} scans of ~{np.mean([len(s) for s in scans]):.0f} points, ray-cast in "
      f"{time.perf_counter() - t0:.1f} s")
rng = np.random.default_rng(0)
desc = rng.random((n_seq, 800)).astype(np.float32)
desc /= desc.sum(1, keepdims=True)
kfs = [SimpleNamespace(keyframe_id=i, points=s, descriptor=desc[i], pose=None) for i, s in enumerate(scans)]


def edge_fn(source_pose, target_pose, relative_transform, information_matrix):
    return {"transform": relative_transform}


results = {}
for prepare_geometry in (False, True):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = batch_loop_closing(kfs, kfs, top_k=10, verify=True, verifier=GeometricVerifier(), edge_fn=edge_fn,
                             prepare_geometry=prepare_geometry)
    torch.cuda.synchronize()
    results[prepare_geometry] = out
    print(f"batch_loop_closing prepare_geometry={prepare_geometry}: {time.perf_counter() - t0:.2f} s, "
          f"{sum(len(e) for e in out.values())} edges")
same = all([e["target_id"] for e in results[False][i]] == [e["target_id"] for e in results[True][i]] and
           all(a["transform"].tobytes() == b["transform"].tobytes() for a, b in zip(results[False][i],
                                                                                    results[True][i]))
           for i in range(n_seq))
print(f"batch_loop_closing both ways bitwise equal {same}")
