"""Time GlobalMap.build_device (csrc/nsc_map.hip) on the two workloads that size it, next to the PyTorch-operator
formulation of the same map on the same device and the same inputs -- the only yardstick there is.

    python tools/map_workload.py [--which kitti raw] [--warmup 3] [--repeats 10] [--scale 1.0] [--out FILE.md]

Inputs, generated on the device from a seed:
  kitti  4 541 clouds x 20 000 float64 rows (the rows a PreparedClouds keeps) along a circle of 150 m radius driven
         twice, so every place is revisited
  raw    1 024 clouds x 120 000 float32 rows of stride 4 (the bench batch's shape) along the same circle, once
Rows in the sensor frame: 70 % on a ground plane at z = -1.7 m with 2 cm of noise, 30 % uniform in a box of
80 x 80 x 6 m.

The operator formulation: the same float64 transform and keys, torch.unique(return_inverse=True), index_add_ of the
counts and of the fixed-point sums, the centroid division.  It leaves out first rows, first and last clouds and the
first-row order, which the HIP path also computes.

Times are HIP events around one call, after warm-up calls of the same shapes; the two formulations alternate inside the
repeat loop.  Printed per workload: median, min and max of both, rows/s, atomic bytes per row x rows / time and the
table's load factor.  Atomic bytes per row: 32 (the count and the three sums of every row) is a lower bound; first row
and first and last cloud add an 8-byte atomic each only when they improve on what the slot holds.  --scale shrinks the
number of clouds for a rehearsal; a figure is only a figure at scale 1."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VOXEL = 0.5
ATOMIC_BYTES_PER_ROW = 32


def make_input(which, scale, device):
    g = torch.Generator(device=device)
    g.manual_seed(7)
    if which == "kitti":
        B, n, dtype, cols, laps = max(int(4541 * scale), 2), 20000, torch.float64, 3, 2.0
    else:
        B, n, dtype, cols, laps = max(int(1024 * scale), 2), 120000, torch.float32, 4, 1.0
    N = B * n
    pts = torch.empty((N, cols), dtype=dtype, device=device)
    chunk = 1 << 24
    for a in range(0, N, chunk):
        m = min(chunk, N - a)
        u = torch.rand((m, 4), generator=g, device=device, dtype=torch.float64)
        xyz = torch.stack([80.0 * u[:, 0] - 40.0, 80.0 * u[:, 1] - 40.0, 6.0 * u[:, 2] - 2.0], 1)
        ground = u[:, 3] < 0.7
        xyz[ground, 2] = -1.7 + 0.02 * (2.0 * u[ground, 2] - 1.0)
        pts[a:a + m, :3] = xyz.to(dtype)
        if cols == 4:
            pts[a:a + m, 3] = u[:, 3].to(dtype)
    ang = torch.arange(B, dtype=torch.float64, device=device) * (laps * 2.0 * math.pi / B)
    poses = torch.zeros((B, 4, 4), dtype=torch.float64, device=device)
    yaw = ang + math.pi / 2                                   # heading along the tangent
    poses[:, 0, 0], poses[:, 0, 1], poses[:, 1, 0], poses[:, 1, 1] = yaw.cos(), -yaw.sin(), yaw.sin(), yaw.cos()
    poses[:, 2, 2] = poses[:, 3, 3] = 1.0
    poses[:, 0, 3], poses[:, 1, 3] = 150.0 * ang.cos(), 150.0 * ang.sin()
    off = torch.arange(B + 1, dtype=torch.int64, device=device) * n
    return pts, off, poses, B, n


def operator_map(pts, poses, B, n):
    """the PyTorch-operator formulation -> (centroids (V,3), counts (V,), keys (V,))"""
    p = pts[:, :3].to(torch.float64).view(B, n, 3)
    R, t = poses[:, :3, :3], poses[:, :3, 3]
    w = (torch.matmul(p, R.transpose(1, 2)) + t[:, None, :]).view(-1, 3)
    k = torch.floor(w / VOXEL).to(torch.int64) + (1 << 20)
    key = k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42)
    keys, inv = torch.unique(key, return_inverse=True)
    V = keys.numel()
    count = torch.zeros(V, dtype=torch.int64, device=pts.device).index_add_(0, inv, torch.ones_like(inv))
    sums = torch.zeros((V, 3), dtype=torch.int64, device=pts.device).index_add_(0, inv, torch.round(w * 16777216.0).to(torch.int64))
    return (sums.to(torch.float64) / 16777216.0) / count[:, None].to(torch.float64), count, keys


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def spread(ms):
    s = sorted(ms)
    return s[len(s) // 2], s[0], s[-1]


def run(which, args, device, lines):
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import GlobalMap
    pts, off, poses, B, n = make_input(which, args.scale, device)
    N = B * n
    gm = GlobalMap(voxel_size=VOXEL, max_voxels=args.max_voxels, device=device)
    hip, op = [], []
    for r in range(args.warmup + args.repeats):
        t_hip, out = timed(lambda: gm.build_device(pts, off, poses))
        t_op, ref = timed(lambda: operator_map(pts, poses, B, n))
        if r >= args.warmup:
            hip.append(t_hip)
            op.append(t_op)
    stats = dict(zip(_lib.MAP_STAT_NAMES, out["stats"].cpu().tolist()))
    V = stats["voxels_found"]
    assert stats["rows_unplaced"] == 0 and V == stats["voxels_written"], stats
    # the HIP map in key order against the operator map.  The operator transform is a batched matmul, whose rounding may
    # differ from the definition's: a row within an ulp of a voxel face can change its voxel, so this is reported only
    order = torch.argsort(out["keys"][:V])
    same = V == int(ref[2].numel()) and bool(torch.equal(out["keys"][:V][order], ref[2]) and
                                             torch.equal(out["info"][:V, 0][order], ref[1]))
    err = float((out["points"][:V][order] - ref[0]).abs().max()) if same else float("nan")
    h, o = spread(hip), spread(op)
    used = stats["rows_used"]
    lines += [
        f"### {which}: {B} clouds x {n} rows, {pts.dtype} x {pts.shape[1]}, {N:,} rows, {V:,} voxels",
        "",
        "| formulation | median ms | min ms | max ms | rows/s (median) |",
        "|---|---|---|---|---|",
        f"| nsc_map_build (6 launches) | {h[0]:.2f} | {h[1]:.2f} | {h[2]:.2f} | {N / h[0] * 1e3:.3g} |",
        f"| torch operators (transform, keys, unique, index_add_) | {o[0]:.2f} | {o[1]:.2f} | {o[2]:.2f} | {N / o[0] * 1e3:.3g} |",
        "",
        f"- HIP / operators (medians): {h[0] / o[0]:.3f}; {args.repeats} repeats after {args.warmup} warm-up calls, alternating",
        f"- atomic bytes: {ATOMIC_BYTES_PER_ROW} B/row x {used:,} rows used / {h[0]:.2f} ms = "
        f"{ATOMIC_BYTES_PER_ROW * used / h[0] / 1e9:.3f} TB/s (the whole call's time, not the insert pass alone)",
        f"- table: {2 * args.max_voxels:,} slots of 64 B, load factor {V / (2.0 * args.max_voxels):.3f}; rows per voxel {used / max(V, 1):.1f}",
        f"- same voxels and counts as the operator map: {same}; largest centroid difference {err:.3g} m",
        "",
    ]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--which", nargs="+", default=["kitti", "raw"], choices=["kitti", "raw"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--max-voxels", type=int, default=1 << 23)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_workload.py measures on the GPU; there is none here")
    device = torch.device("cuda", torch.cuda.current_device())
    lines = [f"Device: {torch.cuda.get_device_name(device)}; scale {args.scale}; voxel {VOXEL} m; max_voxels {args.max_voxels:,}", ""]
    for which in args.which:
        run(which, args, device, lines)
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
