"""CPU-side checks of the boundary: the C-ABI library loads, exports every symbol include/nsc.h
declares, validates arguments without a GPU, and the fast binning estimate never disagrees with
the exact chain when it claims certainty."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-spectral-codec_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from neural_spectral_codec_amd import build, _lib
    build.build_hip()
    return _lib.lib()


def test_header_symbols_exported(lib):
    from neural_spectral_codec_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "nsc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(nsc_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/nsc.h but not exported"
    assert declared == set(_lib.SYMBOLS), "ctypes binding out of sync with include/nsc.h"
    assert not any(n.startswith("nsc_debug") for n in declared), "diagnostics belong in include/nsc_debug.h"
    dbg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nsc_debug.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(nsc_[a-z0-9_]+)\s*\(", dbg)) == set(_lib.DEBUG_SYMBOLS)
    assert hasattr(lib, "nsc_debug_point_bins")                       # parity triage: always built
    dev = "-DNSC_DEV_TUNING" in open(build.FLAGS_FILE).read()
    assert hasattr(lib, "nsc_debug_burn") == dev                      # the co-runner: development builds only


def test_gemm_tile_choice(lib):
    """Which tile the LDS-DMA GEMM takes is a host decision (nsc_gat_gemm_tile, shared with the launcher): at BASELINE
    configs[2] (4 541 keyframes) every projection is ONE round of at most 256 workgroups; for any shape the tile fits the
    160 KB of a CU and covers the output."""
    def tile(M, N, K):
        r, c, l, w = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        assert lib.nsc_gat_gemm_tile(M, N, K, C.byref(r), C.byref(c), C.byref(l), C.byref(w)) == 0
        return r.value, c.value, l.value, w.value
    assert tile(4541, 256, 800) == (80, 64, 3 * 144 * 256, 228)        # input_proj: 57 x 4 tiles
    assert tile(4541, 258, 256) == (96, 64, 3 * 160 * 256, 240)        # lin + 2 attention columns: 48 x 5
    assert tile(4541, 800, 256) == (128, 64, 3 * 192 * 256, 468)       # output_proj: two rounds of 36 x 13 (128 x 128 tiles spill)
    assert tile(1024, 256, 800) == (16, 64, 3 * 80 * 256, 256)         # the bench's GNN: one 16 x 16 block per wave
    for M in (1, 15, 16, 17, 100, 1023, 1024, 1025, 2500, 4541, 9000, 50000):
        for N, K in ((256, 800), (258, 256), (800, 256), (64, 48), (80, 64), (1024, 1024), (3, 16)):
            r, c, l, w = tile(M, N, K)
            assert r % 16 == 0 and 16 <= r <= 128 and c in (64, 128) and l <= 160 * 1024
            assert w == -(-M // r) * -(-N // c)
    assert lib.nsc_gat_gemm_tile(0, 256, 256, None, None, None, None) == -1
    assert lib.nsc_gat_gemm_tile(16, 256, 40, None, None, None, None) == -1       # K not a multiple of 16


def test_argument_validation_without_gpu(lib):
    from neural_spectral_codec_amd import _lib
    p = _lib.EncParams()
    lib.nsc_enc_default_params(C.byref(p))
    assert (p.n_elevation, p.n_azimuth, p.n_bins, p.target_rows) == (16, 360, 50, 16)
    assert abs(p.elev_min_rad - np.deg2rad(-24.8)) < 1e-15
    assert lib.nsc_abi_version() == _lib.ABI_VERSION == 4
    # errors are reported before anything is launched
    assert lib.nsc_encode_clouds(None, None, 1, 10, 4, p, None, None, None, None, None, 0, None) == -1
    assert lib.nsc_encode_clouds(None, None, 0, 0, 4, p, None, None, None, None, None, 0, None) == 0
    assert lib.nsc_encode_clouds(None, None, 1, 10, 5, p, None, None, None, None, None, 0, None) == -1
    p.n_azimuth = 720
    assert lib.nsc_encode_clouds(None, None, 1, 10, 4, p, None, None, None, None, None, 0, None) == -2
    assert b"unsupported" in lib.nsc_status_string(-2)
    p.n_azimuth = 360
    # split-path workspace: small batches of big clouds need E*360*4 bytes per cloud, big batches none
    assert lib.nsc_encode_clouds_workspace_bytes(4, 480000, p) == 4 * 16 * 360 * 4
    assert lib.nsc_encode_clouds_workspace_bytes(1024, 1024 * 120000, p) == 0
    # which kernel set a batch gets is a pure host decision, shared with the launcher: the fast kernel has no batch-size
    # cliff (round 2 fell back to the generic kernel above 2^27 points per BATCH = 1 118 clouds of 120 000 points)
    assert lib.nsc_encode_clouds_path(1024, 1024 * 120000, 4, p) == 1
    assert lib.nsc_encode_clouds_path(1119, 1119 * 120000, 4, p) == 1
    assert lib.nsc_encode_clouds_path(100000, 100000 * 120000, 4, p) == 1
    assert lib.nsc_encode_clouds_path(1024, 1024 * 120000, 3, p) == 2
    assert lib.nsc_encode_clouds_path(4, 480000, 4, p) == 3
    assert lib.nsc_encode_clouds_path(4, 480000, 5, p) == -1
    p.n_elevation = 64
    assert lib.nsc_encode_clouds_path(1024, 1024 * 120000, 4, p) == 2
    p.n_elevation = 16
    # the rows added around the path: shape checks answer without a device as well
    assert lib.nsc_gat_forward_ex(None, None, None, None, None, None, None, 0, 2, None) == -1     # unknown flag
    assert lib.nsc_gat_forward_ex(None, None, None, None, None, None, None, 0, 5, None) == -1     # LDS_TILED excludes CORESIDENT
    if hasattr(lib, "nsc_debug_burn"):                                # development builds only
        assert lib.nsc_debug_burn(9, 1, 1, None, 0, None) == -1 and lib.nsc_debug_burn(0, 1, 1, None, 1 << 20, None) == -1
    assert lib.nsc_quantize_descriptors(None, 0, 800, 1e-8, None, None) == 0
    assert lib.nsc_quantize_descriptors(None, 3, 800, 1e-8, None, None) == -1
    assert lib.nsc_quantize_descriptors(None, 3, 5000, 1e-8, None, None) in (-1, -2)
    assert lib.nsc_record_bytes(50) == 220 and lib.nsc_record_bytes(800) == 1720
    assert lib.nsc_chain_graph_num_edges(4541, 5, 0) == 18158                 # E = 4N - 6
    assert lib.nsc_chain_graph_num_edges(3, 5, 2) == 6 + 4 and lib.nsc_chain_graph_num_edges(1, 5, 0) == 0
    assert lib.nsc_voxel_overlap_workspace_bytes(5000, 5000) == 10000 * 16
    assert lib.nsc_voxel_overlap(None, None, None, None, 1, 20000, 0, 20000, 3, None, 0.2, None, None, None, 0, None) == -1
    assert lib.nsc_w1_distances_cdf(None, 10, 50, None, 1, None, None, 0.0, None, None) == -2        # dim % 4 != 0
    assert lib.nsc_topk_workspace_bytes(1, 100000, 10) == 49 * 10 * 8


@pytest.mark.parametrize("in_dim,hidden,out_dim,n_layers,n", [(800, 256, 800, 3, 4541), (64, 128, 96, 8, 700)])
def test_train_workspace_one_byte_short(lib, in_dim, hidden, out_dim, n_layers, n):
    """The training forward and backward take their workspace size from the layout nsc_gat_train_workspace_bytes reports: one
    byte less is NSC_EWORKSPACE before anything is launched -- at the bench shape, and at eight layers with residual_proj and
    hidden > max(in, out), where every weight-gradient product's split-K slabs have a region of their own."""
    from neural_spectral_codec_amd import _lib
    p = 256                                                          # non-null dummy pointers: nothing may be dereferenced
    m = _lib.GatModel(in_dim=in_dim, hidden=hidden, out_dim=out_dim, n_layers=n_layers, edge_dim=2, residual=1,
                      bn_eps=1e-5, negative_slope=0.2, res_w=p, res_b=p)
    g = _lib.Graph(n_nodes=n, nnz=4 * n, row_ptr=p, src=p, eid=p, loop_attr=p, t_ptr=p, t_entry=p, tgt=p)
    cfg = _lib.GatTrainCfg(dropout_p=0.1, bn_momentum=0.1)
    gr = _lib.GatGrads(x=p, res_w=p, res_b=p)
    need = lib.nsc_gat_train_workspace_bytes(C.byref(m), C.byref(g))
    assert need > 0
    assert lib.nsc_gat_forward_train(C.byref(m), C.byref(g), p, p, C.byref(cfg), p, p, need - 1, None) == -3
    assert lib.nsc_gat_backward(C.byref(m), C.byref(g), p, p, C.byref(cfg), p, C.byref(gr), p, need - 1, None) == -3


def test_product_refuses_cpu_tensors():
    import torch
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.encoding import SpectralEncoder
    enc = SpectralEncoder(n_elevation=16)
    with pytest.raises(_lib.NscError):
        enc.encode_points(np.zeros((4, 4), np.float32))
    with pytest.raises(_lib.NscError):
        enc.forward(torch.zeros(1, 16, 360))


@pytest.mark.parametrize("bias", [0, 1, -1])
def test_binning_margins_host(tmp_path, bias):
    """Fast estimate vs exact chain on 3e6 points (incl. points parked on bin edges), with the
    1-ULP error of v_rcp_f32 / v_sqrt_f32 pushed to either side."""
    exe = str(tmp_path / f"bc{bias}")
    cmd = ["g++", "-O2", "-ffp-contract=off", f"-I{CSRC}", os.path.join(ROOT, "tests", "native", "binning_check.cpp"),
           "-o", exe, "-lm"]
    if bias:
        cmd.insert(3, f"-DNSC_TEST_APPROX_BIAS={bias}")
    subprocess.check_call(cmd)
    for args in (["3000000", "7"], ["1000000", "8", "-15", "15", "16", "0"], ["1000000", "9", "-45", "45", "64", "1"]):
        out = subprocess.check_output([exe] + args).decode().split()
        n, azu, elu, azw, elw = map(int, out[:5])
        assert azw == 0 and elw == 0, out
        assert float(out[5]) < 1e-4          # column-edge slack of the exact float32 chain
    # the lean estimate of encode_fast_kernel (narrow FOV only): never wrong when it claims certainty, and it does
    # (a quarter of the mixed generator's points sit on bin edges, another quarter on the axes: all uncertain)
    for args in (["5000000", "17", "-24.8", "2.0", "16", "1", "1"], ["1000000", "18", "-15", "15", "16", "0", "1"],
                 ["1000000", "19", "-24.8", "2.0", "16", "0", "1"]):
        out = subprocess.check_output([exe] + args).decode().split()
        n, azu, elu, azw, elw = map(int, out[:5])
        assert azw == 0 and elw == 0, out
    # the parameter sets of tests/point_families.py whose bins are narrower or whose rows are float32: 64 rows at the
    # default field of view (the class default) in both row modes, 1.1 mrad bins, a symmetric and a lopsided narrow field
    # of view, 32 float32 rows -- each on edge-parked points alone (generator 2) and on the mixed generator
    for i, fov in enumerate((["-24.8", "2.0", "64", "1"], ["-24.8", "2.0", "64", "0"], ["-2", "2", "64", "1"],
                             ["-11.25", "11.25", "64", "1"], ["-30", "10", "64", "1"], ["-25", "15", "32", "0"])):
        for gen in ("2", "-1"):
            out = subprocess.check_output([exe, "1000000", str(30 + i)] + fov + ["0", gen]).decode().split()
            n, azu, elu, azw, elw = map(int, out[:5])
            assert azw == 0 and elw == 0, (fov, gen, out)
    out = subprocess.check_output([exe, "1000000", "40", "-24.8", "2.0", "16", "0", "1", "2"]).decode().split()
    assert int(out[3]) == 0 and int(out[4]) == 0, out          # the lean estimate, float32 rows, edge-parked points only
    # on bench-like points (generator 0) all but a few 1e-4 are certain: the uncertain queue stays short
    out = subprocess.check_output([exe, "4000000", "23", "-24.8", "2.0", "16", "1", "1", "0"]).decode().split()
    n, azu, elu, azw, elw = map(int, out[:5])
    assert azw == 0 and elw == 0 and azu < 1e-3 * n, out


def _code_objects(tmp_path):
    import shutil
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(f"{llvm}/llvm-objdump") and os.path.exists(f"{llvm}/llvm-readelf")):
        pytest.skip("llvm binutils of the ROCm image not found")
    so = shutil.copy(os.path.join(CSRC, "libnsc_hip.so"), tmp_path / "libnsc_hip.so")
    subprocess.run([f"{llvm}/llvm-objdump", "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    return llvm, [str(tmp_path / f) for f in sorted(os.listdir(tmp_path)) if "amdgcn" in f]


def test_coresident_register_budget(lib, tmp_path):
    """The overlapped step depends on occupancy arithmetic the compiler can silently break.  Round 3: FIVE resident
    encoder workgroups per CU (four of one launch + the first of the next: consecutive launches overlap) at <= 80 VGPRs
    leave 112 of the 512 registers of a SIMD lane, room for two waves of the LDS-free GNN kernels (<= 56 VGPRs each).
    At 92 encoder VGPRs (round 2) the fifth workgroup and the GNN's waves kept each other out; at 114 (seen once, after a
    finish-stage change) even four did.  Read the budgets from the code objects."""
    llvm, objs = _code_objects(tmp_path)
    kernels = {}
    for f in objs:
        notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f], check=True, capture_output=True, text=True).stdout
        for blk in notes.split(".agpr_count")[1:]:          # one metadata map per kernel, keys in alphabetical order
            name = re.search(r"\.name:\s+(\S+)", blk)
            vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
            sc = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            if name and vg and sc:
                kernels[name.group(1)] = (int(vg.group(1)), int(sc.group(1)))
    # every encode_fast_kernel instantiation the library can launch (development builds add more: all are held to it)
    enc = {k: v for k, v in kernels.items() if "encode_fast_kernel" in k}
    assert any("encode_fast_kernelILi2EE" in k for k in enc), sorted(kernels)
    for k, (vg, sc) in enc.items():
        assert vg <= 80 and sc == 0, f"{k}: {vg} VGPRs, {sc} B scratch"
    co = {k: v for k, v in kernels.items() if "gemm_nt_direct_kernel" in k or "gat_aggregate_kernelILi1ELi4ELb0" in k}
    assert len(co) >= 4, sorted(kernels)
    for k, (vg, sc) in co.items():
        assert vg <= 56 and sc == 0, f"{k}: {vg} VGPRs, {sc} B scratch"


def test_glds_gemm_code_objects(lib, tmp_path):
    """gemm_glds_kernel (512 threads = two waves per SIMD, one of each kind): every instantiation fits 256 registers per
    lane without scratch (the 128 x 128 tile did not: it is not instantiated), stages by LDS-DMA only (no wide ds_write),
    and the three-stage form keeps its counted wait -- `s_waitcnt vmcnt(N > 0)` directly followed by a raw `s_barrier`
    (validated: HIP 7.2, AMD clang 22.0.0git roc-7.2.0)."""
    llvm, objs = _code_objects(tmp_path)
    seen = 0
    for f in objs:
        notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f], check=True, capture_output=True, text=True).stdout
        for blk in notes.split(".agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name or "gemm_glds_kernel" not in name.group(1):
                continue
            ag = int(re.match(r":\s+(\d+)", blk).group(1))
            vg = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
            sc = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
            assert vg <= 256 and sc == 0, f"{name.group(1)}: {vg} VGPRs (+{ag} AGPRs), {sc} B scratch"
            seen += 1
        dis = subprocess.run([f"{llvm}/llvm-objdump", "-d", "--no-show-raw-insn", f], check=True, capture_output=True,
                             text=True).stdout
        for m in re.finditer(r"^[0-9a-f]+ <(\S*gemm_glds_kernel\S*)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, flags=re.S | re.M):
            name, body = m.group(1), m.group(2)
            ins = [ln.split("//")[0].strip() for ln in body.splitlines() if ln.strip()]
            dma = [t for t in ins if t.startswith("global_load_lds_dwordx4")]
            mf = [t for t in ins if t.startswith("v_mfma_f32_16x16x4")]
            assert dma and mf, f"{name}: {len(dma)} LDS-DMA loads, {len(mf)} MFMAs"
            # staging is LDS-DMA only: the epilogue's accumulator stores are the kernel's only LDS writes (one dword each)
            assert not [t for t in ins if re.match(r"ds_write(2)?_b(64|96|128)", t)], f"{name}: wide ds_write (register staging crept in)"
            # the staging waves' counted wait survives: vmcnt(N > 0) directly in front of a raw s_barrier
            counted = [i for i, t in enumerate(ins) if re.match(r"s_waitcnt vmcnt\([1-9]\d*\)$", t) and ins[i + 1].startswith("s_barrier")]
            if "ELi3ELi1ELb" in name:                          # three stages: one chunk stays in flight across the barrier
                assert counted, f"{name}: no counted vmcnt wait in front of a barrier"
    assert seen >= 45, seen                                   # (8 + 7) tiles x 3 epilogues


def test_round4_kernels_code_objects(lib, tmp_path):
    """gat_layer_banded_kernel (640 threads: three waves on two SIMDs -> at most 168 registers per lane) and
    gemm_tn_glds_kernel (512 threads): no scratch, staging by LDS-DMA only, MFMAs present, and the staging waves' counted wait
    (`s_waitcnt vmcnt(N > 0)` directly followed by a raw `s_barrier`) survives the compiler."""
    llvm, objs = _code_objects(tmp_path)
    seen = {"gat_layer_banded_kernel": 0, "gemm_tn_glds_kernel": 0}
    for f in objs:
        notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f], check=True, capture_output=True, text=True).stdout
        for blk in notes.split(".agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            kind = next((k for k in seen if name and k in name.group(1)), None)
            if kind is None:
                continue
            ag = int(re.match(r":\s+(\d+)", blk).group(1))
            vg = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
            sc = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
            cap = 168 if kind == "gat_layer_banded_kernel" else 256
            assert vg + ag <= cap and sc == 0, f"{name.group(1)}: {vg} VGPRs (+{ag} AGPRs), {sc} B scratch"
            seen[kind] += 1
        dis = subprocess.run([f"{llvm}/llvm-objdump", "-d", "--no-show-raw-insn", f], check=True, capture_output=True,
                             text=True).stdout
        for m in re.finditer(r"^[0-9a-f]+ <(\S*(?:gat_layer_banded_kernel|gemm_tn_glds_kernel)\S*)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis,
                             flags=re.S | re.M):
            name, body = m.group(1), m.group(2)
            ins = [ln.split("//")[0].strip() for ln in body.splitlines() if ln.strip()]
            assert [t for t in ins if t.startswith("global_load_lds_dwordx4")] and [t for t in ins if t.startswith("v_mfma_f32_16x16x4")], name
            assert not [t for t in ins if re.match(r"ds_write(2)?_b(96)", t)], name
            counted = [i for i, t in enumerate(ins) if re.match(r"s_waitcnt vmcnt\([1-9]\d*\)$", t) and ins[i + 1].startswith("s_barrier")]
            assert counted, f"{name}: no counted vmcnt wait in front of a barrier"
            if "gat_layer_banded_kernel" in name:              # the attention chains: u broadcast by v_readlane, the softmax by DPP
                assert [t for t in ins if t.startswith("v_readlane_b32")] and [t for t in ins if "row_ror:8" in t or "row_half_mirror" in t], name
    assert seen["gat_layer_banded_kernel"] == 6 and seen["gemm_tn_glds_kernel"] == 2, seen


def test_stream_loop_isa(lib, tmp_path):
    """The rolling window of encode_fast_kernel manages its loads and waits in inline asm (global_load_dwordx4 ... nt on a
    scalar base, s_waitcnt vmcnt(U - 2)).  That is only right while the compiler (validated: HIP 7.2, AMD clang 22.0.0git
    roc-7.2.0) adds no other VMEM operation to the loop -- a spill, a rematerialised load -- and never reads a slot's
    registers between its load and the wait.  Check both in the shipped code object."""
    llvm, objs = _code_objects(tmp_path)
    checked = 0
    for f in objs:
        dis = subprocess.run([f"{llvm}/llvm-objdump", "-d", "--no-show-raw-insn", f], check=True, capture_output=True,
                             text=True).stdout
        for m in re.finditer(r"^[0-9a-f]+ <(\S*encode_fast_kernel\S*)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, flags=re.S | re.M):
            name, body = m.group(1), m.group(2)
            ins = [ln.split("//")[0].strip() for ln in body.splitlines() if ln.strip()]
            slot = [i for i, t in enumerate(ins) if re.match(r"global_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\] nt", t)]
            assert len(slot) >= 6, f"{name}: the asm slot loads were not found ({len(slot)})"   # prologue, loop, tail round
            lo, hi = slot[0], slot[-1]
            for t in ins[lo:hi + 1]:
                op = t.split()[0]
                assert not op.startswith(("scratch_", "buffer_", "flat_")), f"{name}: {t} inside the stream"
                if op.startswith("global_"):
                    assert re.match(r"global_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\] nt", t), f"{name}: {t} inside the stream"
            for i in slot:                                   # nothing touches a slot between its load and the next wait
                a, b = map(int, re.match(r"global_load_dwordx4 v\[(\d+):(\d+)\]", ins[i]).groups())
                j = i + 1
                while j < len(ins) and not ins[j].startswith("s_waitcnt vmcnt"):
                    t = ins[j]
                    if not t.startswith(("global_load_dwordx4", "s_", ";")):
                        regs = set(int(x) for x in re.findall(r"\bv(\d+)\b", t))
                        for x, y in re.findall(r"v\[(\d+):(\d+)\]", t):
                            regs.update(range(int(x), int(y) + 1))
                        assert not (regs & set(range(a, b + 1))), f"{name}: `{t}` touches slot v[{a}:{b}] before its wait"
                    j += 1
                assert j < len(ins), f"{name}: no wait after the load at instruction {i}"
            checked += 1
    assert checked >= 1


def test_bench_launcher_reports_a_failed_rank():
    """``python bench.py --gpus 2`` without WORLD_SIZE becomes a launcher that never imports torch; here (no GPU) both
    ranks die at torch.cuda.set_device and the launcher must end with a non-zero status instead of hanging or exec-ing."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import torch
    if torch.cuda.is_available():
        pytest.skip("failure path of the launcher: only meaningful without a GPU")
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--clouds", "4"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode != 0
    assert b"[bench launcher]" in p.stderr
    assert p.stdout.strip() == b""


def test_no_memset_or_memcpy_nodes_on_capturable_paths():
    """Every entry point may be captured into a hipGraph (include/nsc.h).  A hipMemsetAsync captured into a graph becomes a memset
    node, and round 4 found such a node (the zeroing of the triplet gradient) not ordered before the kernel after it in replays of
    the captured training step: gradient sums of 1e25-1e32, hidden by Adam's normalisation from every +-lr parameter check.  The
    library fills and copies with kernels (csrc/nsc_fill.h); this keeps it that way."""
    import glob
    src = glob.glob(os.path.join(ROOT, "neural-spectral-codec_amd", "csrc", "*.hip")) + glob.glob(
        os.path.join(ROOT, "neural-spectral-codec_amd", "csrc", "*.h"))
    assert src
    for f in src:
        code = re.sub(r"//[^\n]*", "", open(f).read())
        assert "hipMemsetAsync" not in code and "hipMemcpyAsync" not in code and "hipMemset(" not in code, f


def test_batchnorm_step_counters_are_one_vector():
    """gnn/model.py::_bump_batches_tracked: the four ``num_batches_tracked`` counters count like torch's own train-mode
    forward would, as 0-d views of one vector (one launch per training forward instead of four); state_dict keys and values,
    load_state_dict, deepcopy, dtype casts and torch.save keep working."""
    import copy
    import io
    import torch
    from neural_spectral_codec_amd.gnn.model import create_spectral_gnn, _bump_batches_tracked
    m = create_spectral_gnn(edge_dim=2)
    g = m.gnn
    bns = [g.input_norm] + list(g.batch_norms)
    bns[1].num_batches_tracked.fill_(7)
    _bump_batches_tracked(g)
    _bump_batches_tracked(g)
    assert [int(b.num_batches_tracked) for b in bns] == [2, 9, 2, 2]
    flat = g._nbt_flat
    assert all(b.num_batches_tracked.data_ptr() == flat.data_ptr() + 8 * i for i, b in enumerate(bns))
    sd = copy.deepcopy(m.state_dict())
    assert sorted(k for k in sd if "num_batches" in k) == sorted(
        ["gnn.input_norm.num_batches_tracked"] + [f"gnn.batch_norms.{i}.num_batches_tracked" for i in range(3)])
    _bump_batches_tracked(g)
    m.load_state_dict(sd)                                   # copies in place: the views stay views
    assert g._nbt_flat is flat and flat.tolist() == [2, 9, 2, 2]
    m2 = copy.deepcopy(m)
    _bump_batches_tracked(m2.gnn)
    assert [int(b.num_batches_tracked) for b in [m2.gnn.input_norm] + list(m2.gnn.batch_norms)] == [3, 10, 3, 3]
    assert flat.tolist() == [2, 9, 2, 2]                    # the copy counts on its own
    m.double()                                              # module._apply: buffers may be re-made
    _bump_batches_tracked(g)
    assert [int(b.num_batches_tracked) for b in bns] == [3, 10, 3, 3]
    f = io.BytesIO()
    torch.save(m.state_dict(), f)
    f.seek(0)
    back = torch.load(f)
    assert int(back["gnn.batch_norms.0.num_batches_tracked"]) == 10 and int(back["gnn.input_norm.num_batches_tracked"]) == 3
    bns[2].num_batches_tracked = None                       # a BatchNorm without the counter (track_running_stats off)
    _bump_batches_tracked(g)
    assert [int(b.num_batches_tracked) for b in bns if b.num_batches_tracked is not None] == [4, 11, 4]
