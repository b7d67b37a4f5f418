#!/usr/bin/env python3
"""What the 16-bit wire format costs stage 1, on the CPU (oracles only): descriptors of ray-cast scans
(synth.scan_world: a few worlds, a drive through each and a second pass that revisits it under another heading and a
lateral offset) are quantised (keyframe_oracle.quantize), and d_q = d_int / 65535 is compared with the float64 W1 of the
unquantised descriptors: share of canonical rows, worst |d_q - d|, overlap of the two top-10 lists per query.
usage: w1q_accuracy.py [worlds=3] [poses_per_pass=20] [n_azimuth=1024]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import keyframe_oracle as ko
import nsc_oracle as orc
import w1q_restatement as R
from neural_spectral_codec_amd import synth

worlds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
per_pass = int(sys.argv[2]) if len(sys.argv) > 2 else 20
n_az = int(sys.argv[3]) if len(sys.argv) > 3 else 1024


def w1_f64(h):
    h = h.astype(np.float64)
    c = np.cumsum(h / h.sum(1, keepdims=True), 1)
    return np.abs(c[:, None, :] - c[None, :, :]).sum(2)


desc = []
for w in range(worlds):
    world = synth.make_world(w)
    xs = np.linspace(-40.0, 40.0, per_pass)
    for i, x in enumerate(xs):                                   # first pass
        desc.append(orc.encode_points(synth.scan_world(world, synth.pose_xyz_yaw(x, 0.0), seed=1000 * w + i, n_azimuth=n_az)))
    for i, x in enumerate(xs):                                   # the revisit: 1.5 m to the side, heading reversed
        desc.append(orc.encode_points(synth.scan_world(world, synth.pose_xyz_yaw(x, 1.5, 0.0, 180.0),
                                                       seed=1000 * w + 500 + i, n_azimuth=n_az)))
desc = np.stack(desc)
q = np.stack([ko.quantize(d) for d in desc])
ok = R.canonical(q)
d = w1_f64(desc)
dq = R.dist(q, q).astype(np.float64)
off = ~np.eye(len(desc), dtype=bool)
fin = np.isfinite(dq) & off
overlap = []
for i in range(len(desc)):
    a = [j for j in np.lexsort((np.arange(len(desc)), d[i])) if j != i][:10]
    b = [j for j in np.lexsort((np.arange(len(desc)), dq[i])) if j != i][:10]
    overlap.append(len(set(a) & set(b)))
print(f"{len(desc)} scans ({worlds} worlds x 2 passes x {per_pass}), {desc.shape[1]} bins: canonical {int(ok.sum())}/{len(ok)}")
print(f"float64 W1 of the unquantised descriptors: {d[off].min():.3f} .. {d[off].max():.3f}, median {np.median(d[off]):.3f}")
print(f"worst |d_q - d| = {np.abs(dq - d)[fin].max():.4f}; largest d_int = {int(R.d_int(*[R.cdf(q)[0]] * 2).max())}")
print(f"top-10 overlap per query: min {min(overlap)}, mean {np.mean(overlap):.2f}")
