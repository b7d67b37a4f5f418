"""Time the ray casting of one scan into a kept map (csrc/nsc_map_rays.hip nsc_map_cast_rays, MapLocalizer.observe_device)
beside nsc_map_insert_dist over the same rows, for scale, on the map of tools/map_insert_workload.py: the KITTI shape of
tools/map_workload.py, at voxels of 0.5 m and 1.0 m.

    python tools/map_rays_workload.py [--warmup 2] [--repeats 7] [--scale 1.0] [--max-voxels 4194304] [--voxels 0.5 1.0]
                                      [--only-hip] [--out FILE.md]

The scan is one cloud of map_workload's ``raw`` generator (120 000 float32 rows of stride 4, within +-40 m of the sensor,
seven in ten on the ground) under its own pose, cast with MapLocalizer's default ray parameters.  Before anything is timed
two casts into zeroed counts are compared by bits, and the eight counts are printed.

Times are HIP events around one call, after warm-up calls of the same shapes.  A cast only reads the map, so it is timed
back to back (``crossed`` keeps accumulating, which changes no work); an insertion changes the map, so every timed
insertion is preceded by a build into the same kept tensors, outside the events.  The median, min and max are printed.
--only-hip skips the insertion, for a rocprofv3 --kernel-trace run of its own.  --scale shrinks the map's number of clouds
for a rehearsal; a figure is only a figure at scale 1."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from map_workload import make_input, spread, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--max-voxels", type=int, default=1 << 22)
    ap.add_argument("--voxels", type=float, nargs="+", default=[0.5, 1.0])
    ap.add_argument("--only-hip", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_rays_workload.py measures on the GPU; there is none here")
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import MapLocalizer
    device = torch.device("cuda", torch.cuda.current_device())
    pts, off, poses, B, n = make_input("kitti", args.scale, device)
    sp, soff, sposes, _, sn = make_input("raw", 1.0 / 1024.0, device)
    scan = (sp[:sn], soff[:2], sposes[:1])
    lines = [f"Device: {torch.cuda.get_device_name(device)}; scale {args.scale}; {args.repeats} repeats after {args.warmup} "
             f"warm-up calls; map of {B} clouds x {n} float64 rows = {B * n:,} rows, max_voxels {args.max_voxels:,}; one scan "
             f"of {sn:,} float32 rows of stride 4", ""]
    table = ["| voxel m | voxels | call | median ms | min ms | max ms | rays/s (median) | voxels visited | visits/ray | "
             "visits/s (median) | crossings |", "|" + "---|" * 11]
    for voxel in args.voxels:
        loc = MapLocalizer(voxel_size=voxel, max_voxels=args.max_voxels, device=device, insertable=True)
        kept = loc.build_device(pts, off, poses)
        stats = dict(zip(_lib.MAP_STAT_NAMES, kept["stats"].tolist()))
        assert stats["voxels_found"] == stats["voxels_written"] and stats["rows_unplaced"] == 0, stats
        first = loc.observe_device(*scan)
        crossed, ray = first["crossed"].clone(), dict(zip(_lib.MAP_RAY_STAT_NAMES, first["ray_stats"].tolist()))
        loc.crossed.fill_(0)
        again = loc.observe_device(*scan)
        assert torch.equal(again["crossed"], crossed) and again["ray_stats"].tolist() == list(ray.values()), "two casts differ"
        assert ray["rays_truncated"] == 0 and ray["rays_cast"] > 0, ray
        lines.append(f"- voxel {voxel}: " + ", ".join(f"{k} {v:,}" for k, v in ray.items()))
        t_cast, t_ins = [], []
        for r in range(args.warmup + args.repeats):
            a, _ = timed(lambda: loc.observe_device(*scan))
            if not args.only_hip:
                loc.build_device(pts, off, poses, out=kept)
                b, _ = timed(lambda: loc.insert_device(*scan))
            if r >= args.warmup:
                t_cast.append(a)
                if not args.only_hip:
                    t_ins.append(b)
        c = spread(t_cast)
        visited, cast = ray["voxels_visited"], ray["rays_cast"]
        table.append(f"| {voxel} | {stats['voxels_found']:,} | nsc_map_cast_rays ({_lib.MAP_RAY_LAUNCHES} launches) | {c[0]:.3f} | "
                     f"{c[1]:.3f} | {c[2]:.3f} | {cast / c[0] * 1e3:.3g} | {visited:,} | {visited / cast:.1f} | "
                     f"{visited / c[0] * 1e3:.3g} | {ray['crossings']:,} |")
        if t_ins:
            i = spread(t_ins)
            table.append(f"| {voxel} | {stats['voxels_found']:,} | nsc_map_insert_dist ({_lib.MAP_INSERT_LAUNCHES} launches) | "
                         f"{i[0]:.3f} | {i[1]:.3f} | {i[2]:.3f} | {sn / i[0] * 1e3:.3g} | | | | |")
        del loc, kept
        torch.cuda.empty_cache()
    text = "\n".join(lines + [""] + table + [""])
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
