"""Time map localisation (csrc/nsc_map.hip nsc_map_build_dist, csrc/nsc_localize.hip nsc_map_register) on the workload
that sizes it: the map of tools/map_workload.py's KITTI shape at 1.0 m, and 64 scans of 120 000 float32 rows registered
against it.

    python tools/map_localize_workload.py [--warmup 2] [--repeats 7] [--scale 1.0] [--rounds 10] [--only-hip]
                                          [--out FILE.md]

Reported:
  build     nsc_map_build_dist beside nsc_map_build on the same input, voxel size and capacity: what nine more 64-bit
            atomics per row and 128-byte slots cost
  register  nsc_map_register beside the PyTorch-operator formulation of the same rounds -- the map's keys sorted once
            outside the timed window, then per round the float64 transform, keys, searchsorted, a gather of the records,
            einsum for J^T Omega J and J^T Omega d, sums over the rows, a batched solve and the update.  Both run
            ``rounds`` updates and one more linearisation (relative_fitness = relative_rmse = 0, so no scan stops early).

Scans are clouds of map_workload's ``raw`` generator (70 % ground plane, 30 % uniform in a box) at 64 places along the
map's circle, starting 0.3 m and 3 degrees of yaw off.  Such a cloud shares only its ground plane with the map, so this is
a workload for time, not for accuracy: the two formulations are compared with each other.

Times are HIP events around one call, after warm-up calls of the same shapes, the formulations alternating inside the
repeat loop; the median, min and max are printed.  --only-hip runs the HIP paths alone, for a rocprofv3 --kernel-trace run
of its own.  --scale shrinks the map's number of clouds for a rehearsal; a figure is only a figure at scale 1."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from map_workload import make_input, spread, timed  # noqa: E402

VOXEL = 1.0
N_SCANS = 64


def scan_input(device):
    """64 raw clouds along the map's circle -> (points (N,4) float32, offsets, true poses, initial poses)"""
    pts, off, poses, B, n = make_input("raw", N_SCANS / 1024.0, device)
    assert B == N_SCANS
    yaw = torch.full((B,), math.radians(3.0), dtype=torch.float64, device=device)
    yaw[1::2] *= -1.0
    d = torch.zeros((B, 4, 4), dtype=torch.float64, device=device)
    d[:, 0, 0], d[:, 0, 1], d[:, 1, 0], d[:, 1, 1] = yaw.cos(), -yaw.sin(), yaw.sin(), yaw.cos()
    d[:, 2, 2] = d[:, 3, 3] = 1.0
    d[:, 0, 3], d[:, 1, 3] = 0.2, -0.2
    d[:, 2, 3] = 0.1
    return pts, off, poses, torch.matmul(poses, d), n


def skew_neg(w):
    """(...,3) -> -[w]x (...,3,3)"""
    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, w[..., 2], -w[..., 1]], -1), torch.stack([-w[..., 2], z, w[..., 0]], -1),
                        torch.stack([w[..., 1], -w[..., 0], z], -1)], -2)


def rot_zyx(x):
    a, b, g = x[:, 0], x[:, 1], x[:, 2]
    ca, sa, cb, sb, cg, sg = a.cos(), a.sin(), b.cos(), b.sin(), g.cos(), g.sin()
    return torch.stack([torch.stack([cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa], -1),
                        torch.stack([sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa], -1),
                        torch.stack([-sb, cb * sa, cb * ca], -1)], -2)


def operator_register(p, T0, keys_sorted, rec_sorted, rounds):
    """the PyTorch-operator formulation of the rounds.  p (S,n,3) float64, T0 (S,4,4), the map's keys in ascending order
    and its records in that order -> (T (S,4,4), n_corr (S,), cost (S,)) after ``rounds`` updates"""
    T = T0.clone()
    V = keys_sorted.numel()
    eye = torch.eye(3, dtype=torch.float64, device=p.device)
    for r in range(rounds + 1):
        w = torch.matmul(p, T[:, :3, :3].transpose(1, 2)) + T[:, None, :3, 3]
        k = torch.floor(w / VOXEL) + float(1 << 20)
        inside = ((k >= 0) & (k < float(1 << 21))).all(-1)
        ki = k.clamp(0, float((1 << 21) - 1)).to(torch.int64)
        key = ki[..., 0] | (ki[..., 1] << 21) | (ki[..., 2] << 42)
        pos = torch.searchsorted(keys_sorted, key.view(-1)).clamp(max=V - 1).view(key.shape)
        rec = rec_sorted[pos]
        ok = (inside & (keys_sorted[pos] == key) & (rec[..., 15] == 1.0)).to(torch.float64)
        d = (w - rec[..., 0:3]) * ok[..., None]
        O = rec[..., [9, 10, 11, 10, 12, 13, 11, 13, 14]].view(*key.shape, 3, 3) * ok[..., None, None]
        J = torch.cat([skew_neg(w), eye.expand(*key.shape, 3, 3)], -1)
        OJ = torch.einsum("snrc,sncb->snrb", O, J)
        H = torch.einsum("snra,snrb->sab", J, OJ)
        g = torch.einsum("snrb,snr->sb", OJ, d)
        if r == rounds:
            return T, ok.sum(1), torch.einsum("snr,snrc,snc->s", d, O, d)
        x = torch.linalg.solve(H, -g)
        dT = torch.zeros_like(T)
        dT[:, :3, :3], dT[:, :3, 3], dT[:, 3, 3] = rot_zyx(x), x[:, 3:], 1.0
        T = torch.matmul(dT, T)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--max-voxels", type=int, default=1 << 22)
    ap.add_argument("--only-hip", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_localize_workload.py measures on the GPU; there is none here")
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import GlobalMap, MapLocalizer
    device = torch.device("cuda", torch.cuda.current_device())
    pts, off, poses, B, n = make_input("kitti", args.scale, device)
    N = B * n
    gm = GlobalMap(voxel_size=VOXEL, max_voxels=args.max_voxels, device=device)
    loc = MapLocalizer(voxel_size=VOXEL, max_voxels=args.max_voxels, max_iteration=args.rounds, relative_fitness=0.0,
                       relative_rmse=0.0, device=device)
    t_dist, t_map = [], []
    for r in range(args.warmup + args.repeats):
        a, out = timed(lambda: loc.build_device(pts, off, poses))
        b, ref = timed(lambda: gm.build_device(pts, off, poses))
        if r >= args.warmup:
            t_dist.append(a)
            t_map.append(b)
    stats = dict(zip(_lib.MAP_STAT_NAMES, out["stats"].cpu().tolist()))
    V = stats["voxels_found"]
    assert stats["rows_unplaced"] == 0 and V == stats["voxels_written"], stats
    same = bool(torch.equal(out["stats"], ref["stats"]) and torch.equal(out["keys"][:V], ref["keys"][:V]) and
                torch.equal(out["info"][:V], ref["info"][:V]))
    usable = int((out["voxels"][:V, 15] == 1.0).sum())
    del pts, ref
    torch.cuda.empty_cache()
    d, m = spread(t_dist), spread(t_map)
    lines = [
        f"Device: {torch.cuda.get_device_name(device)}; scale {args.scale}; voxel {VOXEL} m; max_voxels {args.max_voxels:,}; "
        f"{args.repeats} repeats after {args.warmup} warm-up calls, alternating", "",
        f"### build: {B} clouds x {n} float64 rows = {N:,} rows, {V:,} voxels ({usable:,} usable)", "",
        "| entry point | median ms | min ms | max ms | rows/s (median) |", "|---|---|---|---|---|",
        f"| nsc_map_build_dist (6 launches, 128-byte slots) | {d[0]:.2f} | {d[1]:.2f} | {d[2]:.2f} | {N / d[0] * 1e3:.3g} |",
        f"| nsc_map_build (6 launches, 64-byte slots) | {m[0]:.2f} | {m[1]:.2f} | {m[2]:.2f} | {N / m[0] * 1e3:.3g} |", "",
        f"- nsc_map_build_dist / nsc_map_build (medians): {d[0] / m[0]:.3f}",
        f"- keys, info and stats equal nsc_map_build's: {same}; table load factor {V / (2.0 * args.max_voxels):.3f}", "",
    ]
    sp, soff, truth, init, sn = scan_input(device)
    t_hip, t_op = [], []
    if not args.only_hip:
        order = torch.argsort(out["keys"][:V])
        keys_sorted, rec_sorted = out["keys"][:V][order].contiguous(), out["voxels"][:V][order].contiguous()
        p64 = sp[:, :3].to(torch.float64).view(N_SCANS, sn, 3)
    for r in range(args.warmup + args.repeats):
        a, res = timed(lambda: loc.register_device(sp, soff, init))
        if not args.only_hip:
            b, ref = timed(lambda: operator_register(p64, init, keys_sorted, rec_sorted, args.rounds))
        if r >= args.warmup:
            t_hip.append(a)
            if not args.only_hip:
                t_op.append(b)
    h = spread(t_hip)
    rows = N_SCANS * sn
    lines += [
        f"### register: {N_SCANS} scans x {sn} float32 rows of stride {sp.shape[1]} = {rows:,} rows, {args.rounds} updates "
        f"({args.rounds + 1} linearisations)", "",
        "| formulation | median ms | min ms | max ms | rows x linearisations / s (median) |", "|---|---|---|---|---|",
        f"| nsc_map_register ({1 + 2 * (args.rounds + 1)} launches) | {h[0]:.2f} | {h[1]:.2f} | {h[2]:.2f} | "
        f"{rows * (args.rounds + 1) / h[0] * 1e3:.3g} |",
    ]
    fit = res["fitness"]
    if not args.only_hip:
        o = spread(t_op)
        dT = float((res["transform"] - ref[0]).abs().max())
        dn = int((res["n_correspondences"] - ref[1].to(torch.int64)).abs().max())
        lines += [
            f"| torch operators (transform, keys, searchsorted, gather, einsum, sums, solve) | {o[0]:.2f} | {o[1]:.2f} | "
            f"{o[2]:.2f} | {rows * (args.rounds + 1) / o[0] * 1e3:.3g} |", "",
            f"- HIP / operators (medians): {h[0] / o[0]:.3f}",
            f"- largest difference of a transform entry between the two: {dT:.3g}; of a correspondence count: {dn}",
        ]
    lines += [f"- fitness {float(fit.min()):.3f} .. {float(fit.max()):.3f}; per row and linearisation a lane reads "
              f"{4 * sp.shape[1]} B of row, 16 B per probe and a 128 B record", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
