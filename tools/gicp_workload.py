#!/usr/bin/env python3
"""Stage 2 of loop closing as a stand-alone workload for rocprofv3: one query scan against 10 candidate scans of
about 120 000 points each (ray-cast revisits of one synthetic world, synth.scan_world), registered in one
GeometricVerifier.verify_batch call with the default parameters.  usage: gicp_workload.py [reps=10]
Prints the average verify_batch time (host clock around a synchronised call, un-profiled runs); under
``rocprofv3 --kernel-trace --stats`` use the kernel statistics instead."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from neural_spectral_codec_amd import synth
from neural_spectral_codec_amd.retrieval import GeometricVerifier

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
world = synth.make_world(3)
query = synth.scan_world(world, synth.pose_xyz_yaw(0, 0), seed=1, n_azimuth=1950)
cands = [synth.scan_world(world, synth.pose_xyz_yaw(0.1 * i, -0.05 * i, 0.0, 0.5 * i), seed=2 + i, n_azimuth=1950)
         for i in range(10)]
v = GeometricVerifier()
res = v.verify_batch(query, cands)                       # warm-up
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(reps):
    res = v.verify_batch(query, cands)
dt = (time.perf_counter() - t0) / reps
print(f"points/scan {len(query)}  verified {sum(r[0] for r in res)}/10  "
      f"iterations {[r[2]['iterations'] for r in res]}  verify_batch {dt * 1e3:.2f} ms")
