#!/usr/bin/env python3
"""Stage 1 over float32 rows (WassersteinRetriever) and over 16-bit rows (CompressedRetriever) in ONE process, on the same
descriptors: 100 000 x 800, Q = 1 and Q = 64, whole query (query CDF, distances, top-10) and the distance launch alone (without
and with the spatial filter),
by device events around back-to-back calls; then the compressed retriever alone at 400 000 rows (the capacity side).
usage: w1q_workload.py [reps=200] [rows=100000] [big_rows=400000]
For per-kernel medians run it once under ``rocprofv3 --kernel-trace --stats -- python tools/w1q_workload.py 50 100000 0``
(big_rows = 0 skips the last part, so that every kernel instance sees one shape)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from neural_spectral_codec_amd.encoding.quantization import quantize_batch
from neural_spectral_codec_amd.retrieval import CompressedRetriever, WassersteinRetriever, quantized_cdf
from neural_spectral_codec_amd.retrieval import compressed as cq
from neural_spectral_codec_amd.retrieval import wasserstein as wf

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rows = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
big_rows = int(sys.argv[3]) if len(sys.argv) > 3 else 400000
D = 800
dev = torch.device("cuda")


def device_time(fn, n):
    """mean device time of fn over n calls in microseconds, by events around the window (warm first)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n * 1e3


def rows_like_descriptors(n, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.rand((n, D), generator=g, device=dev) ** 3


def positions(n, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.rand((n, 3), generator=g, device=dev) * torch.tensor([1000.0, 1000.0, 2.0], device=dev)


def fill(r, n, seed):
    for at in range(0, n, 50000):                              # bounded float32 staging for the 16-bit store
        m = min(50000, n - at)
        r.add_to_database(rows_like_descriptors(m, seed + at), positions=positions(m, seed + at + 1))


fl, co = WassersteinRetriever(), CompressedRetriever()
fill(fl, rows, 1)
fill(co, rows, 1)
print(f"database {rows} x {D}: float32 {fl._buf.element_size() * D * 2 + 12} B per keyframe (histogram + CDF + position), "
      f"16-bit {co.bytes_per_keyframe()} B; non-canonical rows {co.n_noncanonical}")
for Q in (1, 64):
    qf = rows_like_descriptors(Q, 999)
    qu = quantize_batch(qf)
    fi, fv = fl.query_batch(qf, top_k=10)
    ci, cv = co.query_batch(qf, top_k=10)
    same = (fi == ci).float().mean().item()
    print(f"Q={Q}: top-10 overlap of the two retrievers' index lists, position by position: {same:.3f}; "
          f"largest |d_q - d| among them {(fv - cv).abs().max().item():.2e}")
    qcf = wf._cdf(qf, 1e-8, True)
    qcu, qok = quantized_cdf(qu)
    n = rows
    t_fd = device_time(lambda: wf._distances_cdf(fl._cdf_buf[:n], qcf), reps)
    t_cd = device_time(lambda: cq.w1_distances_quantized(co._cdf[:n], co._ok[:n], qcu, qok), reps)
    t_fq = device_time(lambda: fl.query_batch(qf, top_k=10), reps)
    t_cq = device_time(lambda: co.query_batch(qf, top_k=10), reps)
    t_cu = device_time(lambda: co.query_batch(qu, top_k=10), reps)
    b_f, b_c = n * D * 4, n * (D * 2 + 1)
    print(f"Q={Q}: distances  float32 {t_fd:8.1f} us ({b_f / t_fd * 1e-6:5.2f} TB/s of {b_f * 1e-6:.0f} MB)   "
          f"16-bit {t_cd:8.1f} us ({b_c / t_cd * 1e-6:5.2f} TB/s of {b_c * 1e-6:.0f} MB)   ratio {t_cd / t_fd:.2f}")
    print(f"Q={Q}: whole query float32 {t_fq:8.1f} us   16-bit, float queries {t_cq:8.1f} us   16-bit, uint16 queries "
          f"{t_cu:8.1f} us   ratio {t_cq / t_fq:.2f}")
    qp = positions(Q, 998)                                     # the spatial filter of TwoStageRetrieval: 50 m around the query
    t_ff = device_time(lambda: wf._distances_cdf(fl._cdf_buf[:n], qcf, fl._pos[:n], qp, 50.0), reps)
    t_cf = device_time(lambda: cq.w1_distances_quantized(co._cdf[:n], co._ok[:n], qcu, qok, co._pos[:n], qp, 50.0), reps)
    print(f"Q={Q}: distances with the spatial filter  float32 {t_ff:8.1f} us   16-bit {t_cf:8.1f} us   ratio {t_cf / t_ff:.2f}")
    if Q > 4:
        sads = n * Q * D / 2
        print(f"Q={Q}: tile kernel {sads / t_cd * 1e-6:.2f} T v_sad_u16/s per device; float32 tile "
              f"{n * Q * D / t_fd * 1e-6:.2f} T |a-b| elements/s")

if big_rows <= 0:                                              # e.g. under the profiler: one shape per kernel instance
    sys.exit(0)
fl.clear_database()
co.clear_database()
del fl
torch.cuda.empty_cache()
fill(co, big_rows, 7)
print(f"16-bit database of {big_rows} rows: {co._cdf.shape[0]} rows of capacity, "
      f"{co._cdf.shape[0] * co.bytes_per_keyframe() * 1e-6:.0f} MB")
for Q in (1, 64):
    qu = quantize_batch(rows_like_descriptors(Q, 999))
    t = device_time(lambda: co.query_batch(qu, top_k=10), max(20, reps // 4))
    print(f"Q={Q} at {big_rows} rows: whole query {t:8.1f} us")
