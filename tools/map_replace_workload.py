"""Time the removal and the re-placing of clouds in a kept map (csrc/nsc_map.hip nsc_map_remove_dist and
nsc_map_replace_dist, MapLocalizer.update_prepared) beside the only alternative there was, nsc_map_build_dist over every
cloud again, on the map of tools/map_insert_workload.py: the KITTI shape of tools/map_workload.py at 1.0 m.

    python tools/map_replace_workload.py [--warmup 2] [--repeats 7] [--scale 1.0] [--max-voxels 4194304 16777216]
                                         [--only-hip] [--out FILE.md]

Cases, per capacity in --max-voxels:
    remove 1, remove 64     the map holds its clouds and 64 scans of map_workload's ``raw`` generator (120 000 float32
                            rows of stride 4); 1 scan and all 64 are taken out again
    replace 1, replace 64   the same map; 1 scan and all 64 are moved 0.3 m and 1 degree away
    replace half            the map of its own clouds; every second cloud is moved (pose_ids -1 for the others), bases 0
    update 64               ``update_prepared`` over the whole store, the poses of the last 64 clouds moved: the choice of
                            the clouds on the device, then one replacement over all rows

Before anything is timed every result is compared with nsc_map_build_dist over what the map should then hold: for every
key of the rebuild the kept map's count, moments and record by bits, every other voxel of the kept map emptied (zeros),
and the rows used.

Times are HIP events around one call, after warm-up calls of the same shapes; a call changes the map, so every timed call
is preceded by a build into the same kept tensors, outside the events.  The rebuild beside it is timed in the same loop.
The median, min and max are printed.  --only-hip skips the rebuild's timing, for a rocprofv3 --kernel-trace run of its
own.  --scale shrinks the map's number of clouds for a rehearsal; a figure is only a figure at scale 1."""
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
N_MOVED = 64


class StoreView:
    """the map's float64 rows of 3 as a ``PreparedClouds`` holds them: what ``update_prepared`` reads of a store"""

    def __init__(self, pts, off):
        self.device = pts.device
        self._packed = (pts, off)

    def __len__(self):
        return int(self._packed[1].numel()) - 1

    def packed(self):
        return self._packed


def moved(poses):
    """the poses turned by 1 degree about z where they stand and shifted by 0.3 m"""
    a = math.radians(1.0)
    turn = torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]],
                        dtype=torch.float64, device=poses.device)
    out = poses.clone()
    out[:, :3, :3] = turn @ poses[:, :3, :3]
    out[:, :3, 3] += torch.tensor([0.24, -0.18, 0.0], dtype=torch.float64, device=poses.device)
    return out


def keyed(m):
    """kept tensors -> (key + 1, place) of the voxels with a place, in key order"""
    idx = m["index"]
    used = idx[(idx[:, 0] != 0) & (idx[:, 1] >= 0)]              # place ~0 reads as -1
    order = torch.argsort(used[:, 0])
    return used[order, 0], used[order, 1]


def follows(a, b):
    """the kept map ``a`` holds every voxel of the rebuild ``b`` with its count, moments and record by bits and every
    other voxel of it is emptied -> (bool, what differs or the number of emptied voxels)"""
    if int(b["stats"][0]) != int(b["stats"][1]) or int(a["stats"][0]) != int(a["stats"][1]):
        return False, "a capacity was short"
    if int(a["stats"][2]) != int(b["stats"][2]):
        return False, f"rows used {int(a['stats'][2])} {int(b['stats'][2])}"
    ka, pa = keyed(a)
    kb, pb = keyed(b)
    at = torch.searchsorted(ka, kb).clamp(max=max(int(ka.numel()) - 1, 0))
    if not torch.equal(ka[at], kb):
        return False, "a key of the rebuild is missing"
    pm = pa[at]
    if not torch.equal(a["info"][pm, 0], b["info"][pb, 0]):
        return False, "count"
    for k in ("moments", "voxels"):
        if not torch.equal(a[k][pm].view(torch.int64), b[k][pb].view(torch.int64)):
            return False, k
    rest = torch.ones_like(ka, dtype=torch.bool)
    rest[at] = False
    pr = pa[rest]
    if bool(a["info"][pr, 0].any()) or bool(a["moments"][pr].any()) or bool(a["voxels"][pr].view(torch.int64).any()):
        return False, "a voxel the rebuild lacks is not emptied"
    return True, int(pr.numel())


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
        raise SystemExit("map_replace_workload.py measures on the GPU; there is none here")
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import MapLocalizer
    device = torch.device("cuda", torch.cuda.current_device())
    pts, off, poses, B, n = make_input("kitti", args.scale, device)
    sp, soff, sposes, S, sn = make_input("raw", N_SCANS / 1024.0, device)
    assert S == N_SCANS and B > N_MOVED
    N = B * n
    # the map with the scans in it: the map's rows followed by the scans' as float64 rows of 3 (a float32 value is that
    # float64 value, so a removal of the float32 rows is matched)
    all_pts = torch.cat([pts, sp[:, :3].to(torch.float64)])
    all_off = torch.cat([off, soff[1:] + N])
    all_poses = torch.cat([poses, sposes])
    new_sposes, new_poses = moved(sposes), moved(poses)
    every_second = torch.where(torch.arange(B, device=device) % 2 == 0, torch.arange(B, device=device), -1)
    half_poses = poses.clone()
    half_poses[0::2] = new_poses[0::2]
    last_poses = poses.clone()
    last_poses[B - N_MOVED:] = new_poses[B - N_MOVED:]
    store = StoreView(pts, off)
    with_scans, alone = (all_pts, all_off, all_poses), (pts, off, poses)

    def scans_moved(s):
        return torch.cat([poses, new_sposes[:s], sposes[s:]])
    # name, rows the call is given, rows it moves or removes, the build before it, the call, the build it must follow
    cases = []
    for s in (1, N_SCANS):
        part = (sp[:s * sn], soff[:s + 1], sposes[:s])
        cases.append((f"remove {s}", s * sn, s * sn, with_scans,
                      lambda loc, part=part: loc.remove_device(*part),
                      (torch.cat([pts, all_pts[N + s * sn:]]), torch.cat([off, all_off[B + s + 1:] - s * sn]),
                       torch.cat([poses, sposes[s:]]))))
    for s in (1, N_SCANS):
        part = (sp[:s * sn], soff[:s + 1], sposes[:s], new_sposes[:s])
        cases.append((f"replace {s}", s * sn, s * sn, with_scans,
                      lambda loc, part=part: loc.replace_device(*part, first_row=N, first_cloud=B),
                      (all_pts, all_off, scans_moved(s))))
    cases.append(("replace half", N, (B + 1) // 2 * n, alone,
                  lambda loc: loc.replace_device(pts, off, poses, new_poses, every_second), (pts, off, half_poses)))
    cases.append((f"update {N_MOVED}", N, N_MOVED * n, alone,
                  lambda loc: loc.update_prepared(store, poses, last_poses), (pts, off, last_poses)))
    lines = [f"Device: {torch.cuda.get_device_name(device)}; scale {args.scale}; voxel {VOXEL} m; {args.repeats} repeats "
             f"after {args.warmup} warm-up calls; map of {B} clouds x {n} float64 rows = {N:,} rows; {N_SCANS} scans of "
             f"{sn:,} float32 rows", ""]
    table = ["| max_voxels | case | rows given | rows moved | median ms | min ms | max ms | rows moved/s (median) | "
             "voxels emptied | rebuild median ms | min ms | max ms | call / rebuild |", "|" + "---|" * 13]
    for M in args.max_voxels:
        loc = MapLocalizer(voxel_size=VOXEL, max_voxels=M, device=device, insertable=True)
        whole = MapLocalizer(voxel_size=VOXEL, max_voxels=M, device=device)
        kept, ref = loc.build_device(*alone), whole.build_device(*alone, moments=True)
        for name, given, rows, start, call, want in cases:
            # the result against the rebuild, before any timing
            loc.build_device(*start, out=kept)
            out = call(loc)
            whole.build_device(*want, out=ref)
            ok, what = follows(loc._kept(), ref)
            assert ok, f"{name}: the kept map does not follow the rebuild: {what}"
            removed = out["removed"].tolist()
            assert removed[0] == rows and removed[1:3] == [0, 0] and removed[4] == 0 and removed[7] == 0, (name, removed)
            # `removed` is the removal half's: a replacement may fill a voxel again that its removal emptied
            assert removed[6] == what if name.startswith("remove") else removed[6] >= what, (name, removed, what)
            if "moved" in out:
                assert int((out["moved"] >= 0).sum()) == N_MOVED
            t_call, t_re = [], []
            for r in range(args.warmup + args.repeats):
                loc.build_device(*start, out=kept)
                a, _ = timed(lambda: call(loc))
                if not args.only_hip:
                    b, _ = timed(lambda: whole.build_device(*want, out=ref))
                if r >= args.warmup:
                    t_call.append(a)
                    if not args.only_hip:
                        t_re.append(b)
            c = spread(t_call)
            row = f"| {M:,} | {name} | {given:,} | {rows:,} | {c[0]:.3f} | {c[1]:.3f} | {c[2]:.3f} | {rows / c[0] * 1e3:.3g} | {what:,} |"
            if t_re:
                b = spread(t_re)
                row += f" {b[0]:.2f} | {b[1]:.2f} | {b[2]:.2f} | {c[0] / b[0]:.4f} |"
            else:
                row += " | | | |"
            table.append(row)
        del loc, whole, kept, ref
        torch.cuda.empty_cache()
    lines += [f"### nsc_map_remove_dist ({_lib.MAP_REMOVE_LAUNCHES} launches), nsc_map_replace_dist "
              f"({_lib.MAP_REPLACE_LAUNCHES} launches) and update_prepared beside nsc_map_build_dist over what the map then "
              "holds; every kept map followed its rebuild by bits", ""] + table + [""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
