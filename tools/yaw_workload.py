#!/usr/bin/env python3
"""The yaw initial guess of stage 2 (retrieval/yaw_alignment.py, nsc_yaw_align): times
  * estimate_yaw of 10 and of 2 000 pairs of 16-row images and of 10 pairs of 64-row images (random images; the
    kernel's work does not depend on the values), by device events;
  * GeometricVerifier.verify_prepared of 1 query x 10 candidates on ray-cast scans of about 120 000 points
    (tools/gicp_store_workload.py's scans), from the identity and from the guess, alternating, on the host clock
    around the call's own sync;
  * filling the image store: YawImages.add of one image, and one keyframe's encode (SpectralEncoder, 16 rows) + add.
usage: yaw_workload.py [reps=200] [section=all|yaw]
``section=yaw`` runs only the three estimate_yaw loops (for ``rocprofv3 --kernel-trace --stats``)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from neural_spectral_codec_amd import synth
from neural_spectral_codec_amd.encoding import SpectralEncoder
from neural_spectral_codec_amd.retrieval import GeometricVerifier, YawImages, estimate_yaw

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
section = sys.argv[2] if len(sys.argv) > 2 else "all"
dev = torch.device("cuda")


def device_time(fn, n):
    """mean device time of fn over n calls, by events around the window (warm first)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n


def host_time(fn, n):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


rng = np.random.default_rng(0)
for R, P in ((16, 10), (16, 2000), (64, 10)):
    imgs = torch.from_numpy(rng.uniform(1.0, 80.0, (64, R, 360)).astype(np.float32)).to(dev)
    qid = torch.from_numpy(rng.integers(0, 64, P)).to(dev)
    cid = torch.from_numpy(rng.integers(0, 64, P)).to(dev)
    ms = device_time(lambda: estimate_yaw(imgs, qid, imgs, cid), reps)
    fma = P * 360 * R * 360
    print(f"estimate_yaw R={R} P={P}: {ms * 1e3:.1f} us per call ({fma * 1e-6 / ms:.0f} float64 GFMA/s)")
if section == "yaw":
    sys.exit(0)

world = synth.make_world(3)
query = synth.scan_world(world, synth.pose_xyz_yaw(0, 0), seed=1, n_azimuth=1950)
cands = [synth.scan_world(world, synth.pose_xyz_yaw(0.1 * i, -0.05 * i, 0.0, 0.5 * i), seed=2 + i, n_azimuth=1950)
         for i in range(10)]
v = GeometricVerifier()
qs, store = v.prepare([query]), v.prepare(cands)
enc = SpectralEncoder(n_elevation=16).to(dev)
images = YawImages()
images.add(enc.encode_points_batch(cands, return_images=True)[2])
qimg = enc.encode_points_batch([query], return_images=True)[2]
ids = list(range(10))
zeros = [0] * 10


def plain():
    return v.verify_prepared(qs, 0, store, ids)


def guessed():
    yaw = estimate_yaw(qimg, zeros, images, ids)
    return v.verify_prepared(qs, 0, store, ids, init_transforms=yaw["init_transforms"])


n = max(10, reps // 4)
rounds = [(host_time(plain, n), host_time(guessed, n)) for _ in range(3)]          # alternating
shifts = estimate_yaw(qimg, zeros, images, ids)["shift"].cpu().tolist()
for a, b in rounds:
    print(f"verify_prepared 1x10 ({len(query)} points/scan): identity {a:.3f} ms   yaw_init {b:.3f} ms")
print(f"  shifts {shifts}  verified {sum(r[0] for r in plain())}/10 and {sum(r[0] for r in guessed())}/10")

one = qimg[0].clone()


def fill():
    images.clear()
    for _ in range(64):
        images.add(one)


print(f"YawImages.add of one 16-row image: {host_time(fill, max(4, reps // 10)) / 64 * 1e3:.1f} us per insert")
ms = host_time(lambda: images.add(enc.encode_points_batch([query], return_images=True)[2]), max(10, reps // 4))
print(f"encode one {len(query)}-point scan (host array, H2D copy included) + add: {ms:.3f} ms per insert")
dq = torch.from_numpy(query).to(dev)
ms = host_time(lambda: images.add(enc.encode_points_batch([dq], return_images=True)[2]), max(10, reps // 4))
print(f"encode one scan already on the device + add: {ms:.3f} ms per insert")
