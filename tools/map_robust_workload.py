"""Time nsc_map_register_robust (csrc/nsc_localize.hip) beside nsc_map_register on the workload of
tools/map_localize_workload.py: the KITTI-shaped map at 1.0 m, 64 scans of 120 000 float32 rows, ``rounds`` updates and one
more linearisation (relative_fitness = relative_rmse = 0, so no scan stops early).

    python tools/map_robust_workload.py [--warmup 2] [--repeats 7] [--scale 1.0] [--rounds 10] [--width 3.0]
                                        [--other-lib PATH/libnsc_hip.so] [--out FILE.md]

Timed, alternating inside the repeat loop: nsc_map_register; Cauchy over one voxel; no kernel over seven voxels; Cauchy over
seven voxels; and, with --other-lib, nsc_map_register of a second build of the library (another commit's), whose results
are also compared with this build's by bits.  Times are HIP events around one call of the C entry point, after warm-up calls
of the same shapes; the median, min and max are printed.  For per-kernel times run it under
``rocprofv3 --kernel-trace --stats`` in a run of its own.  A figure is only a figure at scale 1."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from map_localize_workload import N_SCANS, VOXEL, scan_input  # noqa: E402
from map_workload import make_input, spread, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--width", type=float, default=3.0)
    ap.add_argument("--max-voxels", type=int, default=1 << 22)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_robust_workload.py measures on the GPU; there is none here")
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import MapLocalizer
    device = torch.device("cuda", torch.cuda.current_device())
    pts, off, poses, B, n = make_input("kitti", args.scale, device)
    loc = MapLocalizer(voxel_size=VOXEL, max_voxels=args.max_voxels, max_iteration=args.rounds, relative_fitness=0.0,
                       relative_rmse=0.0, device=device)
    loc.build_device(pts, off, poses)
    del pts
    torch.cuda.empty_cache()
    sp, soff, truth, init, sn = scan_input(device)
    S, N = N_SCANS, int(sp.shape[0])
    f64 = dict(dtype=torch.float64, device=device)
    L = _lib.lib()
    ws = torch.empty(L.nsc_map_register_robust_workspace_bytes(S), dtype=torch.uint8, device=device)
    libs = {"this": L}
    if args.other_lib:
        O = C.CDLL(args.other_lib)
        O.nsc_map_register.restype, O.nsc_map_register.argtypes = _lib.SYMBOLS["nsc_map_register"]
        libs["other"] = O

    def outputs():
        return dict(T=torch.empty((S, 4, 4), **f64), fr=torch.empty((S, 2), **f64), cost=torch.empty((S,), **f64),
                    ci=torch.empty((S, 2), dtype=torch.int64, device=device), info=torch.empty((S, 6, 6), **f64),
                    wp=torch.empty((S, 2), **f64))

    def call(which, o, rob=None):
        head = (_lib.ptr(sp), _lib.MAP_DTYPE_F32, int(sp.shape[1]), _lib.ptr(soff), S, N, _lib.ptr(loc.voxels),
                _lib.ptr(loc.index), loc.capacity, C.byref(loc.params), C.byref(loc.reg))
        outs = (_lib.ptr(init), _lib.ptr(o["T"]), _lib.ptr(o["fr"]), _lib.ptr(o["cost"]), _lib.ptr(o["ci"]),
                _lib.ptr(o["info"]), None)
        tail = (_lib.ptr(ws), int(ws.numel()), _lib.stream_ptr(device))
        if rob is None:
            status = libs[which].nsc_map_register(*head, *outs, *tail)
        else:
            status = L.nsc_map_register_robust(*head, C.byref(rob), *outs, _lib.ptr(o["wp"]), *tail)
        _lib.check(status, "registration")

    cauchy = _lib.MAP_KERNELS["cauchy"]
    configs = [("nsc_map_register", "this", None)]
    if args.other_lib:
        configs.append(("nsc_map_register of --other-lib", "other", None))
    configs += [("Cauchy over one voxel", "this", _lib.MapRobustParams(kernel=cauchy, neighbours=1, scale=args.width)),
                ("no kernel over seven voxels", "this", _lib.MapRobustParams(kernel=0, neighbours=7, scale=0.0)),
                ("Cauchy over seven voxels", "this", _lib.MapRobustParams(kernel=cauchy, neighbours=7, scale=args.width))]
    res = {name: outputs() for name, _, _ in configs}
    times = {name: [] for name, _, _ in configs}
    for r in range(args.warmup + args.repeats):
        for name, which, rob in configs:
            t, _ = timed(lambda: call(which, res[name], rob))
            if r >= args.warmup:
                times[name].append(t)
    rows = S * sn
    base = spread(times["nsc_map_register"])[0]
    lines = [
        f"Device: {torch.cuda.get_device_name(device)}; scale {args.scale}; voxel {VOXEL} m; {S} scans x {sn} float32 rows "
        f"of stride {sp.shape[1]} = {rows:,} rows; {args.rounds} updates ({args.rounds + 1} linearisations, "
        f"{1 + 2 * (args.rounds + 1)} launches); width {args.width}; {args.repeats} repeats after {args.warmup} warm-up "
        f"calls, alternating", "",
        "| configuration | median ms | min ms | max ms | / nsc_map_register | fitness | pairs per corresponding row |",
        "|---|---|---|---|---|---|---|"]
    for name, _, rob in configs:
        m = spread(times[name])
        o = res[name]
        fit = o["fr"][:, 0]
        per = "1" if rob is None else f"{float((o['wp'][:, 1] / o['ci'][:, 0].clamp(min=1)).mean()):.2f}"
        lines.append(f"| {name} | {m[0]:.2f} | {m[1]:.2f} | {m[2]:.2f} | {m[0] / base:.2f} | {float(fit.min()):.3f} .. "
                     f"{float(fit.max()):.3f} | {per} |")
    if args.other_lib:
        a, b = res["nsc_map_register"], res["nsc_map_register of --other-lib"]
        same = all(torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)) for k in ("T", "fr", "cost", "ci", "info"))
        lines += ["", f"- nsc_map_register of the two builds: transforms, fitness, rmse, cost, counts, iterations and "
                      f"information equal by bits: {same}"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
