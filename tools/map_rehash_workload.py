"""Time the move of a kept map to another capacity (csrc/nsc_map.hip nsc_map_rehash_dist, MapLocalizer.resize_device)
beside the only alternative there was, nsc_map_build_dist at the new capacity over the same clouds, on the map of
tools/map_insert_workload.py: the KITTI shape of tools/map_workload.py at 1.0 m.

    python tools/map_rehash_workload.py [--warmup 2] [--repeats 7] [--scale 1.0] [--max-voxels 4194304] [--only-hip]
                                        [--out FILE.md]

Cases, per capacity M in --max-voxels:
    same     the map of all clouds moved to a map of M voxels
    twice    the same map moved to 2 M voxels
    fit      every second cloud removed (nsc_map_remove_dist, outside the timing), then the map moved without its emptied
             voxels to exactly the voxels that are left

Before anything is timed every result is compared with nsc_map_build_dist at the new capacity over the clouds the map
holds: ``same`` and ``twice`` by bits (stats, the written voxels' records, info, keys and moments, the index as a mapping),
``fit`` as a mapping key -> (count, moments, record), since its places are not the rebuild's; and no voxel is left emptied.

Times are HIP events around one call, after warm-up calls of the same shapes, into destination tensors allocated once.  A
move swaps the kept tensors, so every timed call is preceded by a build (and for ``fit`` the removal) into the source
tensors, outside the events.  The rebuild beside it is timed in the same loop, the two alternating.  The median, min and
max are printed.  Bytes moved are computed from shapes: 32 per voxel of new capacity (the index cleared), 8 per voxel of
old capacity (new_place), 64 per written place (its count read by the count and by the move pass, in lines of info), and
512 per kept voxel (240 read and 240 written: record, info, moments, key; 32 for its index slot read and written).  A flat
device copy (``Tensor.copy_``) of as many bytes, half read and half written, is timed beside each call.
--only-hip skips the rebuild's timing, for a rocprofv3 --kernel-trace run of its own.  --scale shrinks the map's number
of clouds for a rehearsal; a figure is only a figure at scale 1."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from map_replace_workload import follows, keyed  # noqa: E402
from map_workload import make_input, spread, timed  # noqa: E402

VOXEL = 1.0


def same_bits(a, b):
    """two maps agree by bits where they are defined and a lookup finds the same -> (bool, what differs)"""
    if not torch.equal(a["stats"], b["stats"]):
        return False, f"stats {a['stats'].tolist()} {b['stats'].tolist()}"
    n = int(b["stats"][1])
    for k in ("voxels", "info", "keys", "moments"):
        if not torch.equal(a[k][:n].view(torch.int64), b[k][:n].view(torch.int64)):
            return False, k
    (ka, pa), (kb, pb) = keyed(a), keyed(b)
    return (torch.equal(ka, kb) and torch.equal(pa, pb)), "index"


def bytes_moved(old, new, written, kept):
    return 32 * new + 8 * old + 64 * written + 512 * kept


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--max-voxels", type=int, nargs="+", default=[1 << 22])
    ap.add_argument("--only-hip", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_rehash_workload.py measures on the GPU; there is none here")
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import MapLocalizer
    device = torch.device("cuda", torch.cuda.current_device())
    pts, off, poses, B, n = make_input("kitti", args.scale, device)
    N = B * n
    cloud = torch.arange(B, device=device)
    gone, stay = torch.where(cloud % 2 == 1, cloud, -1), torch.where(cloud % 2 == 0, cloud, -1)
    lines = [f"Device: {torch.cuda.get_device_name(device)}; scale {args.scale}; voxel {VOXEL} m; {args.repeats} repeats "
             f"after {args.warmup} warm-up calls; map of {B} clouds x {n} float64 rows = {N:,} rows", ""]
    table = ["| max_voxels | case | new max_voxels | places written | voxels kept | dropped | median ms | min ms | max ms | "
             "MB moved | GB/s (median) | flat copy GB/s | rebuild median ms | min ms | max ms | rebuild / move |", "|" + "---|" * 16]
    for M in args.max_voxels:
        loc = MapLocalizer(voxel_size=VOXEL, max_voxels=M, device=device, insertable=True)
        source = loc.build_device(pts, off, poses)
        found = int(source["stats"][0])
        assert found <= M, f"the map's {found:,} voxels do not fit into {M:,}"
        half = MapLocalizer(voxel_size=VOXEL, max_voxels=M, device=device)
        left = int(half.build_device(pts, off, poses, stay)["stats"][0])
        del half
        for name, new, ids in (("same", M, None), ("twice", 2 * M, None), ("fit", left, stay)):
            def prepare():
                loc.max_voxels = M
                loc.build_device(pts, off, poses, out=source)
                if ids is not None:
                    loc.remove_device(pts, off, poses, gone)
            whole = MapLocalizer(voxel_size=VOXEL, max_voxels=new, device=device)
            ref = whole.build_device(pts, off, poses, ids, moments=True)
            prepare()
            out = loc.resize_device(new)
            dest = {k: out[k] for k in ("voxels", "index", "info", "keys", "moments", "stats", "cursor", "new_place",
                                        "tile_base", "rehashed")}
            re = out["rehashed"].tolist()
            if ids is None:
                ok, what = same_bits(loc._kept(), ref)
                assert ok and re == [found, 0, 0, 0, 0, 0], f"{name}: the moved map is not the rebuild: {what} {re}"
            else:
                ok, what = follows(loc._kept(), ref)
                assert ok and what == 0 and re[0] == left and re[1] == found - left and re[2:] == [0, 0, 0, 0], (name, what, re)
            # a flat device copy that moves as many bytes (half read, half written), timed in the same loop
            nbytes = bytes_moved(M, new, found, re[0])
            flat_src = torch.empty(nbytes // 2, dtype=torch.uint8, device=device)
            flat_dst = torch.empty_like(flat_src)
            t_move, t_re, t_flat = [], [], []
            for r in range(args.warmup + args.repeats):
                prepare()
                a, _ = timed(lambda: loc.resize_device(new, out=dest))
                f, _ = timed(lambda: flat_dst.copy_(flat_src))
                if r >= args.warmup:
                    t_flat.append(f)
                if not args.only_hip:
                    b, _ = timed(lambda: whole.build_device(pts, off, poses, ids, out=ref))
                if r >= args.warmup:
                    t_move.append(a)
                    if not args.only_hip:
                        t_re.append(b)
            c = spread(t_move)
            mb = nbytes / 1e6
            row = (f"| {M:,} | {name} | {new:,} | {found:,} | {re[0]:,} | {re[1]:,} | {c[0]:.3f} | {c[1]:.3f} | {c[2]:.3f} | "
                   f"{mb:.1f} | {mb / c[0]:.0f} | {mb / spread(t_flat)[0]:.0f} |")
            if t_re:
                b = spread(t_re)
                row += f" {b[0]:.2f} | {b[1]:.2f} | {b[2]:.2f} | {b[0] / c[0]:.0f} |"
            else:
                row += " | | | |"
            table.append(row)
            del whole, ref, out, dest, flat_src, flat_dst
            torch.cuda.empty_cache()
        del loc, source
        torch.cuda.empty_cache()
    lines += [f"### nsc_map_rehash_dist ({_lib.MAP_REHASH_LAUNCHES} launches) beside nsc_map_build_dist at the new capacity "
              "over the clouds the map holds; every moved map equalled its rebuild by bits", ""] + table + [""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
