"""Time the insertion of scans into a kept map (csrc/nsc_map.hip nsc_map_insert_dist) beside the only alternative there
was, nsc_map_build_dist over all clouds again, on the map of tools/map_localize_workload.py: the KITTI shape of
tools/map_workload.py at 1.0 m.

    python tools/map_insert_workload.py [--warmup 2] [--repeats 7] [--scale 1.0] [--max-voxels 4194304 16777216]
                                        [--only-hip] [--out FILE.md]

Inserted are 1 scan and 64 scans of map_workload's ``raw`` generator (120 000 float32 rows of stride 4) under their poses
along the map's circle.  Per capacity in --max-voxels the same insertions are timed, so the table shows whether an
insertion costs in proportion to its rows whatever the capacity is.  The rebuild is timed at the first capacity, over the
map's rows followed by the scans' as float64 rows of 3 (a float32 value is that float64 value, so the two maps must agree
by bits).

Before anything is timed the script verifies that the inserted map equals the rebuild: stats, and voxels, info, keys and
moments of the written voxels by bits, and the index as a mapping key -> place.

Times are HIP events around one call, after warm-up calls of the same shapes; an insertion changes the map, so every timed
insertion is preceded by a build into the same kept tensors, outside the events.  The median, min and max are printed.
--only-hip skips the rebuild's timing, for a rocprofv3 --kernel-trace run of its own.  --scale shrinks the map's number of
clouds for a rehearsal; a figure is only a figure at scale 1."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from map_workload import make_input, spread, timed  # noqa: E402

VOXEL = 1.0
N_SCANS = 64


def index_pairs(index):
    """the index as (key + 1, place) rows of its occupied slots in key order: equal for two maps in which a lookup finds
    the same"""
    used = index[index[:, 0] != 0]
    return used[torch.argsort(used[:, 0])]


def same_map(a, b):
    """two dicts of kept tensors agree by bits where they are defined -> (bool, what differs)"""
    if not torch.equal(a["stats"], b["stats"]):
        return False, f"stats {a['stats'].tolist()} {b['stats'].tolist()}"
    n = int(a["stats"][1])
    for k in ("voxels", "info", "keys", "moments"):
        if not torch.equal(a[k][:n].view(torch.int64), b[k][:n].view(torch.int64)):
            return False, k
    return bool(torch.equal(index_pairs(a["index"]), index_pairs(b["index"]))), "index"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--max-voxels", type=int, nargs="+", default=[1 << 22, 1 << 24])
    ap.add_argument("--only-hip", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_insert_workload.py measures on the GPU; there is none here")
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import MapLocalizer
    device = torch.device("cuda", torch.cuda.current_device())
    pts, off, poses, B, n = make_input("kitti", args.scale, device)
    sp, soff, sposes, S, sn = make_input("raw", N_SCANS / 1024.0, device)
    assert S == N_SCANS
    N = B * n
    cases = [(1, sp[:sn], soff[:2], sposes[:1]), (N_SCANS, sp, soff, sposes)]
    lines = [f"Device: {torch.cuda.get_device_name(device)}; scale {args.scale}; voxel {VOXEL} m; {args.repeats} repeats "
             f"after {args.warmup} warm-up calls; map of {B} clouds x {n} float64 rows = {N:,} rows", ""]
    table = ["| max_voxels | scans | rows | insert median ms | min ms | max ms | rows/s (median) | voxels before -> after |",
             "|---|---|---|---|---|---|---|---|"]
    rebuilds = []
    for ci, M in enumerate(args.max_voxels):
        loc = MapLocalizer(voxel_size=VOXEL, max_voxels=M, device=device, insertable=True)
        kept = loc.build_device(pts, off, poses)
        for s, p, o, T in cases:
            rows = s * sn
            # equality with the rebuild, before any timing
            loc.build_device(pts, off, poses, out=kept)
            before = int(loc.stats[0])
            loc.insert_device(p, o, T)
            after = dict(zip(_lib.MAP_STAT_NAMES, loc.stats.cpu().tolist()))
            assert after["rows_unplaced"] == 0 and after["voxels_found"] == after["voxels_written"], after
            assert loc.cursor.tolist() == [N + rows, B + s]
            all_pts = torch.cat([pts, p[:, :3].to(torch.float64)])
            all_off = torch.cat([off, o[1:] + N])
            all_poses = torch.cat([poses, T])
            whole = MapLocalizer(voxel_size=VOXEL, max_voxels=M, device=device)
            ref = whole.build_device(all_pts, all_off, all_poses, moments=True)
            ok, what = same_map(loc._kept(), ref)
            assert ok, f"the inserted map differs from the rebuild in {what}"
            t_ins, t_re = [], []
            for r in range(args.warmup + args.repeats):
                loc.build_device(pts, off, poses, out=kept)
                a, _ = timed(lambda: loc.insert_device(p, o, T))
                if ci == 0 and not args.only_hip:
                    b, _ = timed(lambda: whole.build_device(all_pts, all_off, all_poses, out=ref))
                if r >= args.warmup:
                    t_ins.append(a)
                    if ci == 0 and not args.only_hip:
                        t_re.append(b)
            i = spread(t_ins)
            table.append(f"| {M:,} | {s} | {rows:,} | {i[0]:.3f} | {i[1]:.3f} | {i[2]:.3f} | {rows / i[0] * 1e3:.3g} | "
                         f"{before:,} -> {after['voxels_found']:,} |")
            if t_re:
                rebuilds.append((s, N + rows, spread(t_re), i))
            del all_pts, whole, ref
            torch.cuda.empty_cache()
        del loc, kept
        torch.cuda.empty_cache()
    lines += [f"### insert: nsc_map_insert_dist ({_lib.MAP_INSERT_LAUNCHES} launches), float32 rows of stride {sp.shape[1]}; "
              "every inserted map equal to the rebuild by bits", ""] + table + [""]
    if rebuilds:
        lines += [f"### the alternative: nsc_map_build_dist over all clouds, max_voxels {args.max_voxels[0]:,}", "",
                  "| scans added | rows of the rebuild | rebuild median ms | min ms | max ms | insert / rebuild (medians) |",
                  "|---|---|---|---|---|---|"]
        for s, rows, r, i in rebuilds:
            lines.append(f"| {s} | {rows:,} | {r[0]:.2f} | {r[1]:.2f} | {r[2]:.2f} | {i[0] / r[0]:.5f} |")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
