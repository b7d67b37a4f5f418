"""Input families, a restatement of the host dispatch and of the dropout masks, and the float64 reference for the training step
(csrc/nsc_gat_train.hip).  A helper module: tests/test_train_families_cpu.py checks its claims without a GPU,
tests/test_train_paths_gpu.py runs the families on the device.

Every family names the dispatch path it is there for; ``train_paths`` restates nsc_gat_forward_train / nsc_gat_backward's host
decisions (its constants are parsed from the sources, so a changed constant fails the claimed rows, not silently the coverage)
and ``CLAIMS`` holds the literal row of every family.  The reference is the float64 evaluation of oracle/gat_oracle.py's
restatement -- with ``dropout_masks`` (a numpy restatement of hash3 / keep_scale) also for dropout > 0 -- and the yardstick is
the float32 evaluation of the same restatement: e(T) = ||T - T64||_F / ||T64||_F, kernels against k x the float32 figure."""
import os
import re
from types import SimpleNamespace

import numpy as np
import torch

import gat_oracle as go

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "neural-spectral-codec_amd", "csrc")


def _const(text, pattern):
    m = re.search(pattern, text)
    assert m, f"the source no longer holds {pattern!r}: restate train_paths"
    return int(m.group(1))


def _constants():
    hip = open(os.path.join(_CSRC, "nsc_gat_train.hip")).read()
    hdr = open(os.path.join(_CSRC, "nsc_gemm_glds.h")).read()
    c = SimpleNamespace()
    c.SPLITK_SLABS = _const(hip, r"constexpr int SPLITK_SLABS = (\d+);")
    c.COLRED_MAXR = _const(hip, r"constexpr int COLRED_MAXR = (\d+);")
    c.EDGE_BWD_WGS = _const(hip, r"constexpr int EDGE_BWD_WGS = (\d+);")
    c.SPLIT_MIN_N = _const(hip, r"const int splits = N >= (\d+) \? SPLITK_SLABS : 1;")
    c.TM2_MIN_TILES = _const(hip, r"\(\(M \+ 63\) / 64\) \* \(\(N \+ 63\) / 64\) >= (\d+) && M >= 128")
    c.TM2_MIN_M = _const(hip, r"\(\(M \+ 63\) / 64\) \* \(\(N \+ 63\) / 64\) >= \d+ && M >= (\d+)")
    c.TN_ROUND = _const(hip, r"int splits = (\d+) / tiles;")
    c.COLRED_ROWS = _const(hip, r"int R = \(N \+ 63\) / (\d+);")
    c.LANE_DEG = _const(hip, r"if \(end - beg <= (\d+)\) \{")
    c.LANE_DEG_BWD = _const(hip, r"if \(deg <= (\d+)\) \{")
    c.TILE_ROUND = _const(hdr, r"const long long rounds = \(tiles \+ 255\) / (\d+);")
    c.TILE_MFMA = _const(hdr, r"rounds \* \(a \* bc \* nch \* (\d+) \+ \d+\)")
    c.TILE_FIXED = _const(hdr, r"rounds \* \(a \* bc \* nch \* \d+ \+ (\d+)\)")
    c.MAX_EDGE_DIM = _const(open(os.path.join(os.path.dirname(os.path.dirname(_CSRC)), "include", "nsc.h")).read(),
                            r"#define NSC_GAT_MAX_EDGE_DIM\s+(\d+)")
    return c


K = _constants()


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------
# the host dispatch, restated
# ------------------------------------------------------------------------------------------------------------------
def pick_tile(M, N, Kd, max_bc=2):
    """glds_pick_tile (nsc_gemm_glds.h): (ACC, BC) of the LDS-DMA GEMM's tile (16 ACC) x (64 BC)"""
    nch = _cdiv(Kd, 64)
    best, best_cost = (1, 1), None
    for bc in range(1, max_bc + 1):
        ncb = _cdiv(N, 64 * bc)
        for a in range(1, (8 if bc == 1 else 7) + 1):
            tiles = ncb * _cdiv(M, 16 * a)
            cost = _cdiv(tiles, K.TILE_ROUND) * (a * bc * nch * K.TILE_MFMA + K.TILE_FIXED)
            if best_cost is None or cost < best_cost:
                best_cost, best = cost, (a, bc)
    return best


def _fwd_product(M, N, Kd, lda, ldb, a_aligned, resid=False, b_aligned=True):
    """gemm<false> / the output projection's direct launch_glds<2>: 'glds{ACC}x{BC}' or 'gen' (an operand, input or weight, that
    is not 16-byte aligned)"""
    if not ((lda & 3) or (ldb & 3) or (Kd & 15)) and a_aligned and b_aligned:
        a, bc = pick_tile(M, N, Kd)
        return f"glds{a}x{bc}" + ("+resid" if resid else "")
    return "gen" + ("+add" if resid else "")


def _dx_product(M, N, Kd, lda, ldb, resid=False, b_aligned=True):
    """gemm<true> (dX = dY W, the weight k-major; A is the library's own aligned buffer, B the parameter as the caller holds it):
    'bkm{ACC}' (launch_glds_bkm), 'transpose+glds..' (what launch_glds_bkm refuses -- a weight that is not 16-byte aligned -- copied
    transposed into the aligned workspace, then launch_glds<2>) or 'gen' (gemm_gen_kernel<false,true>); '+resid' = the fused
    epilogue, '+add' = add_inplace_kernel behind gemm_gen_kernel"""
    if not (Kd & 15):
        if not ((lda & 3) or (ldb & 3) or (N & 3) or N < 4) and b_aligned:
            return f"bkm{pick_tile(M, N, Kd, 1)[0]}" + ("+resid" if resid else "")
        if not (lda & 3):                      # the copy has ld = K: launch_glds takes it
            a, bc = pick_tile(M, N, Kd)
            return f"transpose+glds{a}x{bc}" + ("+resid" if resid else "")
    return "gen" + ("+add" if resid else "")


def _wgrad_product(M, N, Kd, lda, ldb, splits, b_aligned=True):
    """gemm_wgrad: 'gen' (one slice), 'tn{TM}:{kslab}x{slabs}:{rows of the last slab's last chunk}' (gemm_tn_glds_kernel) or
    'genslab:{kchunk}x{slabs}' (gemm_gen_kernel<true,true> over K slabs)"""
    if splits <= 1:
        return "gen"
    if not ((lda & 3) or (ldb & 3) or M < 4 or N < 4 or (M & 3) or (N & 3) or Kd < 1) and b_aligned:
        tm = 2 if _cdiv(M, 64) * _cdiv(N, 64) >= K.TM2_MIN_TILES and M >= K.TM2_MIN_M else 1
        tiles = _cdiv(M, 64 * tm) * _cdiv(N, 64)
        s = min(max(K.TN_ROUND // tiles, 1), K.SPLITK_SLABS)
        kslab = _cdiv(_cdiv(Kd, s), 64) * 64
        s = _cdiv(Kd, kslab)
        last = Kd - (s - 1) * kslab
        return f"tn{tm}:{kslab}x{s}:{last % 64 or 64}"
    kchunk = _cdiv(_cdiv(Kd, splits), 64) * 64
    return f"genslab:{kchunk}x{splits}"


def colred_rows(N):
    R = max(1, min(K.COLRED_MAXR, _cdiv(N, K.COLRED_ROWS)))
    return R, _cdiv(N, R)


def train_paths(N, in_dim, hidden, out_dim, n_layers, edge_dim, residual, x_aligned, max_in_degree, max_out_degree, w_aligned=True):
    """What nsc_gat_forward_train + nsc_gat_backward launch for this shape, as one row (a dict of short strings).  Degrees count
    CSR entries, the node's own loop included.  w_aligned: the projection and lin weights are 16-byte aligned (a parameter whose
    storage is a view one float into a buffer is not; the library takes the parameters' raw pointers)."""
    wa = w_aligned
    H, L = hidden, n_layers
    assert K.LANE_DEG == K.LANE_DEG_BWD
    splits = K.SPLITK_SLABS if N >= K.SPLIT_MIN_N else 1
    res_id, res_proj = residual and in_dim == out_dim, residual and in_dim != out_dim
    R, rows = colred_rows(N)
    row = {
        "splits": splits,
        "CH": _cdiv(H, 256),
        "colred": f"R{R}x{rows}:{N - (R - 1) * rows}",                     # blocks x rows per block : rows of the last block
        "target_form": "lane" if max_in_degree <= K.LANE_DEG else "loop",  # agg_train_kernel and att_bwd_target_kernel, widest target
        "source_chunks": _cdiv(max_out_degree, 64),                        # att_bwd_source_kernel, longest list
        "edge_dim": edge_dim or 0,
        # forward products
        "f_in": _fwd_product(N, H, in_dim, in_dim, in_dim, x_aligned, b_aligned=wa),
        "f_lin": _fwd_product(N, H, H, H, H, True, b_aligned=wa),
        "f_out": _fwd_product(N, out_dim, H, H, H, True, resid=res_id, b_aligned=wa),     # an unaligned x: the epilogue adds it element-wise
        "f_res": _fwd_product(N, out_dim, in_dim, in_dim, in_dim, x_aligned, b_aligned=wa) if res_proj else None,
        # weight gradients (K = N rows)
        "w_out": _wgrad_product(out_dim, H, N, out_dim, H, splits),
        "w_res": _wgrad_product(out_dim, in_dim, N, out_dim, in_dim, splits, x_aligned) if res_proj else None,
        "w_lin": _wgrad_product(H, H, N, H, H, splits),
        "w_in": _wgrad_product(H, in_dim, N, H, in_dim, splits, x_aligned),
        # input-side gradients
        "d_hL": _dx_product(N, H, out_dim, out_dim, H, b_aligned=wa),
        "d_res": _dx_product(N, in_dim, out_dim, out_dim, in_dim, b_aligned=wa) if res_proj else None,
        "d_lin": _dx_product(N, H, H, H, H, b_aligned=wa),
        "d_lin_resid": _dx_product(N, H, H, H, H, resid=True, b_aligned=wa) if (residual and L >= 3) else None,
        "d_x": _dx_product(N, in_dim, H, H, in_dim, b_aligned=wa),
    }
    return row


def row_str(row):
    """One line per row: the literal the tests compare"""
    return " ".join(f"{k}={v}" for k, v in row.items() if v is not None)


# ------------------------------------------------------------------------------------------------------------------
# the counter-based dropout masks, restated (nsc_gat_train.hip: hash3 / keep_scale)
# ------------------------------------------------------------------------------------------------------------------
_GOLD, _M1, _M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_U64 = (1 << 64) - 1


def hash3_scalar(seed, stream, idx):
    """hash3 on Python ints"""
    z = (seed + _GOLD * (idx + 1) + (stream << 48)) & _U64
    z = ((z ^ (z >> 30)) * _M1) & _U64
    z = ((z ^ (z >> 27)) * _M2) & _U64
    z = z ^ (z >> 31)
    return z >> 40


def hash3(seed, stream, idx):
    """hash3 on a uint64 array of indices (uint64 arithmetic wraps like the kernel's)"""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & _U64) + np.uint64(_GOLD) * (idx + np.uint64(1)) + np.uint64((stream << 48) & _U64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_M2)
        z = z ^ (z >> np.uint64(31))
    return z >> np.uint64(40)


def keep_scale(seed, stream, idx, p):
    """keep_scale: float32 array, 0 or 1 / (1 - p) in float32"""
    p32 = np.float32(p)
    u = hash3(seed, stream, idx).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.where(u >= p32, np.float32(1.0) / (np.float32(1.0) - p32), np.float32(0.0)).astype(np.float32)


def csr_entries(edge_index, n_nodes):
    """(row_ptr, src, eid) of nsc_graph_build_csr in numpy: targets ascending; a target's entries in edge-list order, existing self
    loops removed and edges with an endpoint outside [0, n) dropped; the target's own loop (eid -1) last."""
    ei = np.asarray(edge_index, dtype=np.int64)
    e = np.arange(ei.shape[1])
    ok = (ei[0] != ei[1]) & (ei[0] >= 0) & (ei[0] < n_nodes) & (ei[1] >= 0) & (ei[1] < n_nodes)
    src = np.concatenate([ei[0][ok], np.arange(n_nodes)])
    dst = np.concatenate([ei[1][ok], np.arange(n_nodes)])
    eid = np.concatenate([e[ok], np.full(n_nodes, -1)])
    order = np.argsort(dst, kind="stable")
    row_ptr = np.zeros(n_nodes + 1, np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(dst, minlength=n_nodes))
    return row_ptr, src[order], eid[order]


def dropout_masks(seed, p, n_nodes, hidden, n_layers, edge_index):
    """The masks a forward with this seed applies, in the form oracle.forward_from_state takes: attention masks per CSR entry
    (stream 100 + l, idx = entry), feature masks per element (stream 200 + l, idx = n H + c; layers l < L - 1)."""
    nnz = int(csr_entries(edge_index, n_nodes)[0][-1])
    att = [torch.from_numpy(keep_scale(seed, 100 + l, np.arange(nnz), p).astype(np.float64)) for l in range(n_layers)]
    feat = [torch.from_numpy(keep_scale(seed, 200 + l, np.arange(n_nodes * hidden), p).astype(np.float64)).reshape(n_nodes, hidden)
            for l in range(n_layers - 1)]
    return {"att": att, "feat": feat}


def seed_of(torch_seed):
    """The seed SpectralGNN._run_train draws after torch.manual_seed(torch_seed) (model.py: one randint from the CPU generator)"""
    torch.manual_seed(torch_seed)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


# ------------------------------------------------------------------------------------------------------------------
# graphs
# ------------------------------------------------------------------------------------------------------------------
def hub_graph(n, in_degrees=(63, 64, 65, 128, 129), out_degrees=(64, 65), seed=0):
    """A chain i <-> i + 1 plus hubs: target 10 k + 10 has exactly in_degrees[k] CSR entries (own loop included), source
    55 + 2 k exactly out_degrees[k] (own loop included), with duplicate edges and explicit self loops (which the CSR builder
    removes).  Returns edge_index (2, E) int64."""
    assert n >= 130
    i = np.arange(n - 1)
    src, dst = [i, i + 1], [i + 1, i]
    pool = np.arange(70, n)                                    # sources of the hubs' extra edges, cyclic: duplicates when short
    for k, d in enumerate(in_degrees):
        t = 10 * k + 10
        extra = d - 3                                          # two chain neighbours + own loop
        s = pool[(np.arange(extra) + 7 * k) % len(pool)]
        if k == 0:
            s = np.concatenate([s[:extra // 2], s[:extra - extra // 2]])     # every edge twice
        src.append(s); dst.append(np.full(extra, t))
    tpool = np.arange(62, n)
    for k, d in enumerate(out_degrees):
        s = 55 + 2 * k
        extra = d - 3
        src.append(np.full(extra, s)); dst.append(tpool[(np.arange(extra) + 3 * k) % len(tpool)])
    loops = np.arange(0, n, 9)
    src.append(loops); dst.append(loops)
    ei = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)
    perm = np.random.default_rng(seed).permutation(ei.shape[1])            # edge-list order unrelated to the target
    return torch.from_numpy(ei[:, perm])


def degrees(edge_index, n):
    """(in-degree per target, out-degree per source) in CSR entries, own loop included"""
    row_ptr, src, _ = csr_entries(edge_index, n)
    return np.diff(row_ptr), np.bincount(src, minlength=n)


# ------------------------------------------------------------------------------------------------------------------
# families
# ------------------------------------------------------------------------------------------------------------------
def _F(dims, N, L=2, edge_dim=2, residual=True, graph="chain", aligned=True, p=0.0, seed=0, attr=True, dagger=False, w_aligned=True):
    return dict(dims=dims, N=N, L=L, edge_dim=edge_dim, residual=residual, graph=graph, aligned=aligned, p=p, seed=seed, w_aligned=w_aligned,
                attr=attr, dagger=dagger)


FAMILIES = {}
for _n in (511, 512, 513):
    FAMILIES[f"split-{_n}"] = _F((64, 64, 64), _n, dagger=_n >= 512)
for _n in (1024, 1025, 1087):
    FAMILIES[f"slab-{_n}"] = _F((64, 64, 64), _n, dagger=True)
FAMILIES["wide-896x132"] = _F((64, 896, 132), 577, dagger=True)
FAMILIES["wide-default"] = _F((800, 256, 800), 577, L=3, dagger=True)
for _h in (272, 512, 528, 768, 784, 1024):
    FAMILIES[f"ch-{_h}-chain"] = _F((64, _h, 64), 130)
    FAMILIES[f"ch-{_h}-hub"] = _F((64, _h, 64), 130, graph="hub")
FAMILIES["ch-1024-577"] = _F((64, 1024, 64), 577, dagger=True)
for _h in (64, 272):
    FAMILIES[f"degree-{_h}"] = _F((64, _h, 64), 200, graph="hub")
for _o in (4, 20, 36):
    for _n in (130, 577):
        FAMILIES[f"out-{_o}-{_n}-resproj"] = _F((64, 64, _o), _n, dagger=_n == 577)
        FAMILIES[f"out-{_o}-{_n}-nores"] = _F((64, 64, _o), _n, residual=False, dagger=_n == 577)
for _e in (1, 3, 8):
    FAMILIES[f"edge-{_e}"] = _F((64, 64, 64), 130, edge_dim=_e)
FAMILIES["edge-none-fed"] = _F((64, 64, 64), 130, edge_dim=2, attr=False)
for _n in (17, 63, 64, 65, 4095, 4096, 4097, 4161):
    FAMILIES[f"colred-{_n}"] = _F((64, 64, 64), _n, L=3)
# dX tiles: in_dim = 1 600 makes d_x = dZ0 W_in (N x 1 600, K = 64) take ACC = ceil(N / 160) (25 column blocks: one round of 256
# workgroups holds ten row blocks); one row short of and one row past a multiple of the 16 ACC-row tile
for _acc, _n in ((1, 159), (2, 161), (2, 319), (3, 321), (4, 639), (5, 641), (6, 959), (7, 961), (7, 1119), (8, 1121)):
    FAMILIES[f"dx-acc{_acc}-{_n}"] = _F((1600, 64, 1600), _n, L=3)
for _o in (64, 48):
    for _n in (130, 577):
        FAMILIES[f"unaligned-{_o}-{_n}"] = _F((64, 64, _o), _n, aligned=False, dagger=_n == 577)
# weights one float into their buffers (the library takes the parameters' raw pointers): launch_glds_bkm refuses them, gemm<true>
# goes through transpose_kernel + launch_glds<2> on the aligned copy, with the fused resid epilogue at L = 3
for _o in (64, 48):
    for _n in (130, 577):
        FAMILIES[f"unaligned-w-{_o}-{_n}"] = _F((64, 64, _o), _n, L=3, w_aligned=False, dagger=_n == 577)
for _p in (0.1, 0.5):
    for _h in (64, 272):
        for _n in (130, 577):
            for _g in ("chain", "hub"):
                FAMILIES[f"dropout-{_p}-{_h}-{_n}-{_g}"] = _F((64, _h, 64), _n, L=3, graph=_g, p=_p)

# The literal train_paths row of every family (row_str form).  Written down, not computed: a changed dispatch constant or selector
# fails the comparison in tests/test_train_families_cpu.py and tests/test_train_paths_gpu.py and has to be looked at.
CLAIMS = {
    "split-511": "splits=1 CH=1 colred=R8x64:63 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "split-512": "splits=16 CH=1 colred=R8x64:64 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=tn1:64x8:64 w_lin=tn1:64x8:64 w_in=tn1:64x8:64 d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "split-513": "splits=16 CH=1 colred=R9x57:57 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=tn1:64x9:1 w_lin=tn1:64x9:1 w_in=tn1:64x9:1 d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "slab-1024": "splits=16 CH=1 colred=R16x64:64 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=tn1:64x16:64 w_lin=tn1:64x16:64 w_in=tn1:64x16:64 d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "slab-1025": "splits=16 CH=1 colred=R17x61:49 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=tn1:128x9:1 w_lin=tn1:128x9:1 w_in=tn1:128x9:1 d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "slab-1087": "splits=16 CH=1 colred=R17x64:63 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=tn1:128x9:63 w_lin=tn1:128x9:63 w_in=tn1:128x9:63 d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "wide-896x132": "splits=16 CH=4 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=glds3x1 f_lin=glds3x1 f_out=glds1x1 f_res=glds1x1 w_out=tn2:128x5:1 w_res=tn1:64x10:1 w_lin=tn2:320x2:1 w_in=tn1:64x10:1 d_hL=gen d_res=gen d_lin=bkm3 d_x=bkm1",
    "wide-default": "splits=16 CH=1 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds2x1+resid w_out=tn2:128x5:1 w_lin=tn1:64x10:1 w_in=tn2:128x5:1 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm2",
    "ch-272-chain": "splits=1 CH=2 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "ch-272-hub": "splits=1 CH=2 colred=R3x44:42 target_form=loop source_chunks=2 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "ch-512-chain": "splits=1 CH=2 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "ch-512-hub": "splits=1 CH=2 colred=R3x44:42 target_form=loop source_chunks=2 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "ch-528-chain": "splits=1 CH=3 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "ch-528-hub": "splits=1 CH=3 colred=R3x44:42 target_form=loop source_chunks=2 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "ch-768-chain": "splits=1 CH=3 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "ch-768-hub": "splits=1 CH=3 colred=R3x44:42 target_form=loop source_chunks=2 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "ch-784-chain": "splits=1 CH=4 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "ch-784-hub": "splits=1 CH=4 colred=R3x44:42 target_form=loop source_chunks=2 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "ch-1024-chain": "splits=1 CH=4 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "ch-1024-hub": "splits=1 CH=4 colred=R3x44:42 target_form=loop source_chunks=2 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "ch-1024-577": "splits=16 CH=4 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=glds3x1 f_lin=glds3x1 f_out=glds1x1+resid w_out=tn1:64x10:1 w_lin=tn2:320x2:1 w_in=tn1:64x10:1 d_hL=bkm3 d_lin=bkm3 d_x=bkm1",
    "degree-64": "splits=1 CH=1 colred=R4x50:50 target_form=loop source_chunks=2 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "degree-272": "splits=1 CH=2 colred=R4x50:50 target_form=loop source_chunks=2 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "out-4-130-resproj": "splits=1 CH=1 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1 f_res=glds1x1 w_out=gen w_res=gen w_lin=gen w_in=gen d_hL=gen d_res=gen d_lin=bkm1 d_x=bkm1",
    "out-4-130-nores": "splits=1 CH=1 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1 w_out=gen w_lin=gen w_in=gen d_hL=gen d_lin=bkm1 d_x=bkm1",
    "out-4-577-resproj": "splits=16 CH=1 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1 f_res=glds1x1 w_out=tn1:64x10:1 w_res=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=tn1:64x10:1 d_hL=gen d_res=gen d_lin=bkm1 d_x=bkm1",
    "out-4-577-nores": "splits=16 CH=1 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1 w_out=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=tn1:64x10:1 d_hL=gen d_lin=bkm1 d_x=bkm1",
    "out-20-130-resproj": "splits=1 CH=1 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1 f_res=glds1x1 w_out=gen w_res=gen w_lin=gen w_in=gen d_hL=gen d_res=gen d_lin=bkm1 d_x=bkm1",
    "out-20-130-nores": "splits=1 CH=1 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1 w_out=gen w_lin=gen w_in=gen d_hL=gen d_lin=bkm1 d_x=bkm1",
    "out-20-577-resproj": "splits=16 CH=1 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1 f_res=glds1x1 w_out=tn1:64x10:1 w_res=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=tn1:64x10:1 d_hL=gen d_res=gen d_lin=bkm1 d_x=bkm1",
    "out-20-577-nores": "splits=16 CH=1 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1 w_out=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=tn1:64x10:1 d_hL=gen d_lin=bkm1 d_x=bkm1",
    "out-36-130-resproj": "splits=1 CH=1 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1 f_res=glds1x1 w_out=gen w_res=gen w_lin=gen w_in=gen d_hL=gen d_res=gen d_lin=bkm1 d_x=bkm1",
    "out-36-130-nores": "splits=1 CH=1 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1 w_out=gen w_lin=gen w_in=gen d_hL=gen d_lin=bkm1 d_x=bkm1",
    "out-36-577-resproj": "splits=16 CH=1 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1 f_res=glds1x1 w_out=tn1:64x10:1 w_res=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=tn1:64x10:1 d_hL=gen d_res=gen d_lin=bkm1 d_x=bkm1",
    "out-36-577-nores": "splits=16 CH=1 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1 w_out=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=tn1:64x10:1 d_hL=gen d_lin=bkm1 d_x=bkm1",
    "edge-1": "splits=1 CH=1 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=1 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "edge-3": "splits=1 CH=1 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=3 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "edge-8": "splits=1 CH=1 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=8 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "edge-none-fed": "splits=1 CH=1 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=0 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "colred-17": "splits=1 CH=1 colred=R1x17:17 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "colred-63": "splits=1 CH=1 colred=R1x63:63 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "colred-64": "splits=1 CH=1 colred=R1x64:64 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "colred-65": "splits=1 CH=1 colred=R2x33:32 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "colred-4095": "splits=16 CH=1 colred=R64x64:63 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=tn1:256x16:63 w_lin=tn1:256x16:63 w_in=tn1:256x16:63 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "colred-4096": "splits=16 CH=1 colred=R64x64:64 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=tn1:256x16:64 w_lin=tn1:256x16:64 w_in=tn1:256x16:64 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "colred-4097": "splits=16 CH=1 colred=R64x65:2 target_form=lane source_chunks=1 edge_dim=2 f_in=glds2x1 f_lin=glds2x1 f_out=glds2x1+resid w_out=tn1:320x13:1 w_lin=tn1:320x13:1 w_in=tn1:320x13:1 d_hL=bkm2 d_lin=bkm2 d_lin_resid=bkm2+resid d_x=bkm2",
    "colred-4161": "splits=16 CH=1 colred=R64x66:3 target_form=lane source_chunks=1 edge_dim=2 f_in=glds2x1 f_lin=glds2x1 f_out=glds2x1+resid w_out=tn1:320x14:1 w_lin=tn1:320x14:1 w_in=tn1:320x14:1 d_hL=bkm2 d_lin=bkm2 d_lin_resid=bkm2+resid d_x=bkm2",
    "dx-acc1-159": "splits=1 CH=1 colred=R3x53:53 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "dx-acc2-161": "splits=1 CH=1 colred=R3x54:53 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds2x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm2",
    "dx-acc2-319": "splits=1 CH=1 colred=R5x64:63 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds2x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm2",
    "dx-acc3-321": "splits=1 CH=1 colred=R6x54:51 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds3x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm3",
    "dx-acc4-639": "splits=16 CH=1 colred=R10x64:63 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds4x1+resid w_out=tn1:64x10:63 w_lin=tn1:64x10:63 w_in=tn1:64x10:63 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm4",
    "dx-acc5-641": "splits=16 CH=1 colred=R11x59:51 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds5x1+resid w_out=tn1:128x6:1 w_lin=tn1:64x11:1 w_in=tn1:128x6:1 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm5",
    "dx-acc6-959": "splits=16 CH=1 colred=R15x64:63 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds6x1+resid w_out=tn1:128x8:63 w_lin=tn1:64x15:63 w_in=tn1:128x8:63 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm6",
    "dx-acc7-961": "splits=16 CH=1 colred=R16x61:46 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds7x1+resid w_out=tn1:128x8:1 w_lin=tn1:64x16:1 w_in=tn1:128x8:1 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm7",
    "dx-acc7-1119": "splits=16 CH=1 colred=R18x63:48 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds7x1+resid w_out=tn1:128x9:31 w_lin=tn1:128x9:31 w_in=tn1:128x9:31 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm7",
    "dx-acc8-1121": "splits=16 CH=1 colred=R18x63:50 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds8x1+resid w_out=tn1:128x9:33 w_lin=tn1:128x9:33 w_in=tn1:128x9:33 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm8",
    "unaligned-64-130": "splits=1 CH=1 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=gen f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "unaligned-64-577": "splits=16 CH=1 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=gen f_lin=glds1x1 f_out=glds1x1+resid w_out=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=genslab:64x16 d_hL=bkm1 d_lin=bkm1 d_x=bkm1",
    "unaligned-48-130": "splits=1 CH=1 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=gen f_lin=glds1x1 f_out=glds1x1 f_res=gen w_out=gen w_res=gen w_lin=gen w_in=gen d_hL=bkm1 d_res=bkm1 d_lin=bkm1 d_x=bkm1",
    "unaligned-48-577": "splits=16 CH=1 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=gen f_lin=glds1x1 f_out=glds1x1 f_res=gen w_out=tn1:64x10:1 w_res=genslab:64x16 w_lin=tn1:64x10:1 w_in=genslab:64x16 d_hL=bkm1 d_res=bkm1 d_lin=bkm1 d_x=bkm1",
    "unaligned-w-64-130": "splits=1 CH=1 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=gen f_lin=gen f_out=gen+add w_out=gen w_lin=gen w_in=gen d_hL=transpose+glds1x1 d_lin=transpose+glds1x1 d_lin_resid=transpose+glds1x1+resid d_x=transpose+glds1x1",
    "unaligned-w-64-577": "splits=16 CH=1 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=gen f_lin=gen f_out=gen+add w_out=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=tn1:64x10:1 d_hL=transpose+glds1x1 d_lin=transpose+glds1x1 d_lin_resid=transpose+glds1x1+resid d_x=transpose+glds1x1",
    "unaligned-w-48-130": "splits=1 CH=1 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=gen f_lin=gen f_out=gen f_res=gen w_out=gen w_res=gen w_lin=gen w_in=gen d_hL=transpose+glds1x1 d_res=transpose+glds1x1 d_lin=transpose+glds1x1 d_lin_resid=transpose+glds1x1+resid d_x=transpose+glds1x1",
    "unaligned-w-48-577": "splits=16 CH=1 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=gen f_lin=gen f_out=gen f_res=gen w_out=tn1:64x10:1 w_res=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=tn1:64x10:1 d_hL=transpose+glds1x1 d_res=transpose+glds1x1 d_lin=transpose+glds1x1 d_lin_resid=transpose+glds1x1+resid d_x=transpose+glds1x1",
    "dropout-0.1-64-130-chain": "splits=1 CH=1 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "dropout-0.1-64-130-hub": "splits=1 CH=1 colred=R3x44:42 target_form=loop source_chunks=2 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "dropout-0.1-64-577-chain": "splits=16 CH=1 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=tn1:64x10:1 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "dropout-0.1-64-577-hub": "splits=16 CH=1 colred=R10x58:55 target_form=loop source_chunks=2 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=tn1:64x10:1 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "dropout-0.1-272-130-chain": "splits=1 CH=2 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "dropout-0.1-272-130-hub": "splits=1 CH=2 colred=R3x44:42 target_form=loop source_chunks=2 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "dropout-0.1-272-577-chain": "splits=16 CH=2 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=tn1:64x10:1 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "dropout-0.1-272-577-hub": "splits=16 CH=2 colred=R10x58:55 target_form=loop source_chunks=2 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=tn1:64x10:1 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "dropout-0.5-64-130-chain": "splits=1 CH=1 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "dropout-0.5-64-130-hub": "splits=1 CH=1 colred=R3x44:42 target_form=loop source_chunks=2 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "dropout-0.5-64-577-chain": "splits=16 CH=1 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=tn1:64x10:1 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "dropout-0.5-64-577-hub": "splits=16 CH=1 colred=R10x58:55 target_form=loop source_chunks=2 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=tn1:64x10:1 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "dropout-0.5-272-130-chain": "splits=1 CH=2 colred=R3x44:42 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "dropout-0.5-272-130-hub": "splits=1 CH=2 colred=R3x44:42 target_form=loop source_chunks=2 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=gen w_lin=gen w_in=gen d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "dropout-0.5-272-577-chain": "splits=16 CH=2 colred=R10x58:55 target_form=lane source_chunks=1 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=tn1:64x10:1 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
    "dropout-0.5-272-577-hub": "splits=16 CH=2 colred=R10x58:55 target_form=loop source_chunks=2 edge_dim=2 f_in=glds1x1 f_lin=glds1x1 f_out=glds1x1+resid w_out=tn1:64x10:1 w_lin=tn1:64x10:1 w_in=tn1:64x10:1 d_hL=bkm1 d_lin=bkm1 d_lin_resid=bkm1+resid d_x=bkm1",
}

# Seeds other than 0: the draw (of twelve) that leaves admission (a) the widest margin where seed 0 leaves less than 200 x
# (tests/test_train_families_cpu.py checks the condition itself)
SEEDS = {"colred-4095": 7, "colred-4096": 5, "colred-4097": 7, "colred-4161": 7, "dropout-0.5-272-577-chain": 1,
         # ... and where seed 0 leaves the float32 floor of condition (c) above 1.5e-5 (limit 5e-5): the first draw below 8e-6
         "ch-272-chain": 1, "ch-528-chain": 2, "out-4-577-nores": 3, "colred-63": 1, "colred-65": 1, "dropout-0.5-272-130-chain": 1}
# k of the bar e_gpu(T) <= k x e32_fam: twice the worst ratio measured on the MI355X, rounded up
K_BAR = 16


def _widest_gap_scale(c, d, lo, hi):
    """t in [lo, hi] (or 1) that maximises min_e |c_e + t d_e|, searched over the middles of the 64 widest gaps between the roots"""
    roots = (-c / d)[(d != 0)]
    roots = torch.sort(roots[(roots > lo) & (roots < hi)])[0]
    roots = torch.cat([torch.tensor([lo], dtype=c.dtype), roots, torch.tensor([hi], dtype=c.dtype)])
    mid, width = (roots[1:] + roots[:-1]) / 2, roots[1:] - roots[:-1]
    cand = torch.cat([mid[torch.argsort(width, descending=True)[:64]], torch.ones(1, dtype=c.dtype)])
    margin = (c[None, :] + cand[:, None] * d[None, :]).abs().min(1)[0]
    return cand[margin.argmax()].item()


def _place_parameters(m, g, masks):
    """Admission (a) by construction, layer by layer on the float64 restatement.  With thousands of rows no draw keeps every one
    of ~1e6 ReLU inputs and ~1e5 logits 100 float32 errors away from the kink by chance, so the family places its parameters:
      * each layer's att_dst and att_src are scaled (each by a factor in [0.75, 1.5]) to the value that leaves the widest
        margin between the layer's pre-leaky-ReLU logits and zero;
      * each BatchNorm's bias is moved (by at most 0.25 per channel) into the middle of the widest gap that the channel's batch
        leaves around the ReLU's kink.
    Parameters are inputs like any other; the draws that remain are checked by tests/test_train_families_cpu.py."""
    L = len(m.convs)
    ei = go.add_self_loops_mean(g.edge_index, None, g.num_nodes)[0]
    placed = {"bias_shift": [], "att_scale": []}           # what was done: the CPU test holds it to the limits stated above

    def taps_now():
        taps = {}
        go.forward_reference(m, g, training=True, dtype=torch.float64, taps=taps, masks=masks)
        return taps

    def place_bias(bn, b):
        v = taps_now()[f"relu{b}"].detach() - bn.bias.detach().double()          # gamma * xhat, (N, H)
        s = torch.sort(v, 0)[0]
        mid, width = -(s[1:] + s[:-1]) / 2, s[1:] - s[:-1]                     # a bias in the middle of a gap, and the gap
        width = torch.where((mid - bn.bias.detach().double()).abs() <= 0.25, width, torch.zeros_like(width))
        best = width.argmax(0)
        new = torch.where(width.max(0)[0] > 0, mid.gather(0, best[None])[0], bn.bias.detach().double())
        placed["bias_shift"].append((new - bn.bias.detach().double()).abs().max().item())
        with torch.no_grad():
            bn.bias.copy_(new.float())

    place_bias(m.input_norm, 0)
    for l, conv in enumerate(m.convs):
        for att, end, lo, hi in ((conv.att_dst, 1, 0.75, 1.5), (conv.att_src, 0, 0.75, 1.5)):
            taps = taps_now()
            a = (taps[f"l{l}.G"].detach() * att.detach().double().view(1, -1)).sum(-1)[ei[end]]
            t = _widest_gap_scale(taps[f"l{l}.logit"].detach() - a, a, lo, hi)
            placed["att_scale"].append(t)
            with torch.no_grad():
                att.mul_(t)
        if l < L - 1:
            place_bias(m.batch_norms[l], l + 1)
    return placed


def family_graph(name):
    """(x, edge_index, edge_attr) of a family, CPU tensors"""
    from neural_spectral_codec_amd.keyframe import graph_manager as gm
    f = FAMILIES[name]
    seed = SEEDS.get(name, 0)
    n, i = f["N"], f["dims"][0]
    gen = torch.Generator().manual_seed(2000 + seed)
    x = torch.rand(n, i, generator=gen)
    if f["graph"] == "chain":
        cg = gm.synthetic_chain_graph(n, device="cpu", seed=seed + 2, features=x)
        ei, ea = cg.edge_index, cg.edge_attr
    else:
        ei = hub_graph(n, seed=seed)
        ea = torch.rand(ei.shape[1], 2, generator=gen)
    if f["edge_dim"] not in (None, 2):
        ea = torch.rand(ei.shape[1], f["edge_dim"], generator=gen)
    if not f["attr"]:
        ea = None
    return x, ei, ea


def family_paths(name, edge_index=None):
    """The train_paths row of a family (no model, no reference: cheap)"""
    f = FAMILIES[name]
    if edge_index is None:
        edge_index = family_graph(name)[1]
    din, dout = degrees(edge_index.numpy(), f["N"])
    (i, h, o) = f["dims"]
    return train_paths(f["N"], i, h, o, f["L"], f["edge_dim"] if f["attr"] else 0, f["residual"], f["aligned"], int(din.max()),
                       int(dout.max()), w_aligned=f["w_aligned"])


def tail_rows(paths, n):
    """{weight-gradient product: (last node row, first row of the product's last non-empty K slab)} for the split-K products"""
    out = {}
    for k in ("w_out", "w_res", "w_lin", "w_in"):
        v = paths.get(k)
        if v and v != "gen":
            kslab = int(re.match(r"\w+:(\d+)x", v).group(1))
            out[k] = (n - 1, (n - 1) // kslab * kslab)
    return out


def family(name):
    """SimpleNamespace(name, model (CPU), graph (CPU tensors: x, edge_index, edge_attr, num_nodes), R (probe), masks, torch_seed,
    paths (the train_paths row), spec).  Deterministic."""
    from neural_spectral_codec_amd.gnn.model import SpectralGNN
    f = FAMILIES[name]
    seed = SEEDS.get(name, 0)
    (i, h, o), n, L = f["dims"], f["N"], f["L"]
    torch.manual_seed(1000 + seed)
    m = SpectralGNN(input_dim=i, hidden_dim=h, output_dim=o, n_layers=L, dropout=f["p"], residual=f["residual"],
                    edge_dim=f["edge_dim"])
    go.randomize_bn_stats(m, seed + 1)
    with torch.no_grad():
        for c in m.convs:
            c.bias.normal_(0, 0.1)
    x, ei, ea = family_graph(name)
    g = SimpleNamespace(x=x, edge_index=ei, edge_attr=ea, num_nodes=n)
    paths = family_paths(name, ei)
    R = torch.randn(n, o, generator=torch.Generator().manual_seed(3))
    torch_seed = 77 + seed
    masks = dropout_masks(seed_of(torch_seed), f["p"], n, h, L, ei.numpy()) if f["p"] > 0 else None
    placed = _place_parameters(m, g, masks)
    din, dout = degrees(ei.numpy(), n)
    return SimpleNamespace(name=name, model=m, graph=g, R=R, masks=masks, torch_seed=torch_seed, paths=paths, spec=f,
                           in_degrees=din, out_degrees=dout, placed=placed)


# ------------------------------------------------------------------------------------------------------------------
# reference and error figures
# ------------------------------------------------------------------------------------------------------------------
def is_zero_grad(k):
    """A bias in front of a batch-statistics BatchNorm: exactly-zero gradient, rounding noise on both sides"""
    return k == "input_proj.bias" or (k.startswith("convs.") and k.endswith(".bias"))


def reference(fam, dtype, taps=None):
    """The restatement's evaluation in `dtype`: {'emb', 'loss', 'grad x', 'grad <key>' ..., '<bn>.running_mean' / '.running_var' ...}
    (`taps` additionally collects the intermediates and their gradients)."""
    taps = {} if taps is None else taps
    R = fam.R.to(dtype)
    threads = torch.get_num_threads()
    if dtype == torch.float32:
        # the float32 evaluation is the yardstick: one thread, so that its rounding (how torch's CPU GEMM splits its sums)
        # does not depend on how many cores the machine has
        torch.set_num_threads(1)
    try:
        emb, grads, gx, loss = go.reference_gradients(fam.model, fam.graph, lambda e: (e * R).sum() + (e * e).sum(), dtype=dtype,
                                                      taps=taps, masks=fam.masks)
    finally:
        torch.set_num_threads(threads)
    out = {"emb": emb, "loss": loss.reshape(1), "grad x": gx}
    for k, v in grads.items():
        out["grad " + k] = v
    n = fam.graph.num_nodes
    sd = fam.model.state_dict()
    for b, name in enumerate(["input_norm"] + [f"batch_norms.{l}" for l in range(fam.spec["L"])]):
        mean, var = taps[f"bn{b}.mean"], taps[f"bn{b}.var"] * (n / (n - 1))          # nn.BatchNorm1d: momentum 0.1, unbiased
        out[name + ".running_mean"] = 0.9 * sd[name + ".running_mean"].to(dtype) + 0.1 * mean
        out[name + ".running_var"] = 0.9 * sd[name + ".running_var"].to(dtype) + 0.1 * var
    return out


def err(t, t64):
    """e(T) = ||T - T64||_F / ||T64||_F"""
    t, t64 = t.detach().cpu().double().reshape(-1), t64.detach().cpu().double().reshape(-1)
    return ((t - t64).norm() / t64.norm().clamp_min(1e-300)).item()


def err_rows(t, t64):
    """worst row of a node-indexed tensor: max_n ||T[n] - T64[n]|| / ||T64[n]||"""
    t, t64 = t.detach().cpu().double(), t64.detach().cpu().double()
    return ((t - t64).norm(dim=1) / t64.norm(dim=1).clamp_min(1e-300)).max().item()


ROW_TENSORS = ("emb", "grad x")


def figures(got, ref64):
    """({tensor: e(T)}, {tensor: worst row}) over everything but the biases in front of a batch-statistics BatchNorm (is_zero_grad).
    No other reference tensor may be exactly zero: it would have no relative error and would drop out of the bar unseen."""
    e, rows = {}, {}
    for k, v in ref64.items():
        if k.startswith("grad ") and is_zero_grad(k[5:]):
            continue
        assert bool(v.abs().max() > 0), f"{k}: the float64 reference is exactly zero"
        e[k] = err(got[k], v)
        if k in ROW_TENSORS:
            rows[k] = err_rows(got[k], v)
    return e, rows


def admission(fam, taps32, taps64):
    """Condition (a): per ReLU input / pre-leaky-ReLU logit tensor, (signs agree, smallest |value| / largest |float32 - float64|)"""
    out = {}
    L = fam.spec["L"]
    for k in [f"relu{b}" for b in range(L)] + [f"l{l}.logit" for l in range(L)]:
        a, b = taps32[k].detach().double(), taps64[k].detach()
        small = min(a.abs().min().item(), b.abs().min().item())
        out[k] = (bool((torch.sign(a) == torch.sign(b)).all()), small / max((a - b).abs().max().item(), 1e-300))
    return out


def run_gpu(fam):
    """One train-mode forward and backward of the family through the Python module on the device: the same dict as reference()
    plus 'num_batches_tracked' (a list) and 'x' (the device input, for alignment asserts)."""
    import copy
    dev = "cuda"
    m = copy.deepcopy(fam.model).to(dev)
    if not fam.spec["w_aligned"]:
        # every GEMM weight becomes a contiguous view one float into a larger buffer
        for k, p in m.named_parameters():
            if k.endswith(("input_proj.weight", "output_proj.weight", "residual_proj.weight", "lin_src.weight")):
                buf = torch.zeros(p.numel() + 4, device=dev)
                v = buf[1:1 + p.numel()].view(p.shape)
                v.copy_(p.data)
                p.data = v
                assert p.data_ptr() % 16 == 4 and p.is_contiguous()
    g = fam.graph
    n, i = g.x.shape
    if fam.spec["aligned"]:
        x = g.x.to(dev)
    else:
        buf = torch.zeros(n * i + 4, device=dev)
        x = buf[1:1 + n * i].view(n, i)
        x.copy_(g.x)
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    x.requires_grad_(True)
    gg = SimpleNamespace(x=x, edge_index=g.edge_index.to(dev), num_nodes=n)
    if g.edge_attr is not None:
        gg.edge_attr = g.edge_attr.to(dev)
    m.train()
    torch.manual_seed(fam.torch_seed)
    emb = m(gg)
    R = fam.R.to(dev)
    loss = (emb * R).sum() + (emb * emb).sum()
    loss.backward()
    out = {"emb": emb.detach().cpu(), "loss": loss.detach().cpu().reshape(1), "grad x": x.grad.cpu(), "x": x}
    for k, p in m.named_parameters():
        out["grad " + k] = p.grad.detach().cpu()
    bns = [("input_norm", m.input_norm)] + [(f"batch_norms.{l}", bn) for l, bn in enumerate(m.batch_norms)]
    for name, bn in bns:
        out[name + ".running_mean"], out[name + ".running_var"] = bn.running_mean.cpu(), bn.running_var.cpu()
    out["num_batches_tracked"] = [int(bn.num_batches_tracked) for _, bn in bns]
    return out


def check_bn_running_stats(model, before, ref_taps, n, rtol=1e-4, atol=1e-5):
    """Every BatchNorm of the model (input_norm and batch_norms.{l}) moved like nn.BatchNorm1d: momentum 0.1 towards the batch
    mean and the UNBIASED batch variance of the reference's taps; num_batches_tracked advanced by one."""
    gnn = getattr(model, "gnn", model)
    pre = "gnn." if gnn is not model else ""
    for b, (name, bn) in enumerate([("input_norm", gnn.input_norm)] + [(f"batch_norms.{l}", x) for l, x in enumerate(gnn.batch_norms)]):
        rm = 0.9 * before[pre + name + ".running_mean"].cpu().double() + 0.1 * ref_taps[f"bn{b}.mean"].double()
        rv = 0.9 * before[pre + name + ".running_var"].cpu().double() + 0.1 * ref_taps[f"bn{b}.var"].double() * (n / (n - 1))
        assert torch.allclose(bn.running_mean.cpu().double(), rm, rtol=rtol, atol=atol), name + ".running_mean"
        assert torch.allclose(bn.running_var.cpu().double(), rv, rtol=rtol, atol=atol), name + ".running_var"
        assert int(bn.num_batches_tracked) == int(before[pre + name + ".num_batches_tracked"]) + 1, name


def coverage_gaps(claims=None):
    """What the literal rows of the family list do NOT reach, of the paths the training step's host dispatch can take (an empty
    list = covered)."""
    rows = [dict(t.split("=", 1) for t in r.split()) for r in (claims or CLAIMS).values()]
    vals = lambda *keys: {r[k] for r in rows for k in keys if k in r}
    wg, dx = vals("w_out", "w_res", "w_lin", "w_in"), vals("d_hL", "d_res", "d_lin", "d_lin_resid", "d_x")
    R = {int(re.match(r"R(\d+)x", v).group(1)) for v in vals("colred")}
    want = {
        "splits 1": "1" in vals("splits"), "splits > 1": any(int(v) > 1 for v in vals("splits")),
        "TM 1": any(v.startswith("tn1:") for v in wg), "TM 2": any(v.startswith("tn2:") for v in wg),
        "gemm_wgrad in one slice": "gen" in wg, "gen split-K slabs": any(v.startswith("genslab:") for v in wg),
        "target form lane": "lane" in vals("target_form"), "target form loop": "loop" in vals("target_form"),
        "source list > 64": any(int(v) > 1 for v in vals("source_chunks")),
        "gemm<true> on launch_glds_bkm": any(v.startswith("bkm") for v in dx), "gemm<true> on gemm_gen_kernel": "gen" in dx,
        "gemm<true> on the transposed copy": any(v.startswith("transpose+glds") for v in dx),
        "fused resid epilogue behind the transposed copy": any(v.startswith("transpose+glds") and v.endswith("+resid") for v in dx),
        "forward weight off the LDS-DMA GEMM": "gen" in vals("f_lin", "f_out") or "gen+add" in vals("f_out"),
        "fused resid epilogue": any(v.endswith("+resid") for v in dx),
        "forward on gemm_gen_kernel": "gen" in vals("f_in", "f_res"),
        "R 1": 1 in R, "1 < R < 64": any(1 < r < K.COLRED_MAXR for r in R), "R 64": K.COLRED_MAXR in R,
    }
    for last in (1, 63, 64):
        want[f"last chunk {last}"] = any(v.startswith("tn") and v.endswith(f":{last}") for v in wg)
    for ch in (1, 2, 3, 4):
        want[f"CH {ch}"] = str(ch) in vals("CH")
    for acc in range(1, 9):
        want[f"bkm ACC {acc}"] = any(re.fullmatch(rf"bkm{acc}(\+resid)?", v) for v in dx)
    for ed in (0, 1, 2, 3, 8):
        want[f"edge_dim {ed}"] = str(ed) in vals("edge_dim")
    return [k for k, ok in want.items() if not ok]
