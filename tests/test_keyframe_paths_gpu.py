"""Every branch of csrc/nsc_keyframe.hip on constructed inputs (tests/keyframe_families.py), against the oracle.

The bars are exact -- quantised words, dequantised float bits, record bytes, edge indices, voxel counts and IoU are
compared for equality with oracle/keyframe_oracle.{py,c} (admitted on the CPU in tests/test_keyframe_families_cpu.py)
-- except the two float32 edge features, which keep the bar of test_keyframe_rows.py::test_chain_graph_gpu: <= 2 ulp, or
<= 1e-7 absolute.  References are computed once per input (functools caches of the families module) and never modified.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import keyframe_families as KF
import keyframe_oracle as ko
from keyframe_families import MAX_U16
from neural_spectral_codec_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 256


def u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def host(t):
    return t.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# quantiser
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", KF.dims())
def test_quantizer_families(dim):
    """Words and dequantised bits identical to the oracle for every family of the dim at every row count (the rows of a
    launch cycle through the family from another start each time; 9 rows reach every row of every family)."""
    from neural_spectral_codec_amd.encoding import quantization as qz
    for name, (rows, q, d) in KF.quant_reference(dim).items():
        for n in KF.row_counts():
            idx = (n + np.arange(n)) % len(rows) if n < 9 else np.arange(n) % len(rows)
            got = qz.quantize_batch(dev(rows[idx]))
            assert got.dtype == torch.uint16 and tuple(got.shape) == (n, dim)
            gq = host(got)
            assert np.array_equal(gq, q[idx]), (name, n, np.argwhere(gq != q[idx])[:4].tolist())
            gd = host(qz.dequantize_batch(got))
            assert np.array_equal(u32(gd), u32(d[idx])), (name, n)
            want_tot = q[idx].astype(np.int64).sum(1)
            got_tot = gq.astype(np.int64).sum(1)
            assert np.array_equal(got_tot[want_tot == MAX_U16], np.full(int((want_tot == MAX_U16).sum()), MAX_U16))
            assert np.array_equal(got_tot, want_tot)                 # the clamped rows too: what the oracle says, not 65 535
    if dim == 4096:
        tot = int(KF.quant_reference(dim)["excess_over_max"][1][0].astype(np.int64).sum())
        assert tot == 66795


@pytest.mark.parametrize("dim", KF.dims())
def test_dequantizer_words(dim):
    from neural_spectral_codec_amd.encoding import quantization as qz
    w, d = KF.words_reference(dim)
    for n in KF.row_counts():
        idx = (n + np.arange(n)) % len(w) if n < 9 else np.arange(n) % len(w)
        got = host(qz.dequantize_batch(dev(w[idx])))
        assert np.array_equal(u32(got), u32(d[idx])), (n, np.argwhere(u32(got) != u32(d[idx]))[:4].tolist())


# ----------------------------------------------------------------------------------------------------------------------
# records
# ----------------------------------------------------------------------------------------------------------------------
def _record_tensors(rec):
    return (dev(rec.q), dev(rec.pose7.view(np.float32)), dev(rec.ts.view(np.float64).reshape(-1)),
            dev(rec.ids.view(np.uint32).reshape(-1)), dev(rec.hashes))


@pytest.mark.parametrize("dim", KF.RECORD_DIMS)
def test_pack_records(dim):
    from neural_spectral_codec_amd.encoding import quantization as qz
    L = _lib.lib()
    for n in KF.RECORD_N:
        rec = KF.records(n, dim)
        want = KF.records_reference(rec)
        q, p7, ts, ids, hs = _record_tensors(rec)
        got = qz.pack_records(q, p7, ts, ids, hs)
        assert tuple(got.shape) == (n, 2 * dim + 120) and np.array_equal(host(got), want), n
        # through the C ABI into a dirty buffer: reserved bytes zeroed, nothing written past the last record
        rb = 2 * dim + 120
        for fill in (0xFF, 0x5A):
            buf = torch.full((n * rb + GUARD,), fill, dtype=torch.uint8, device="cuda")
            st = L.nsc_pack_records(_lib.ptr(q), _lib.ptr(p7), _lib.ptr(ts), _lib.ptr(ids), _lib.ptr(hs), n, dim,
                                    _lib.ptr(buf), _lib.stream_ptr(buf.device))
            assert st == 0
            out = host(buf)
            body = out[:n * rb].reshape(n, rb)
            assert not body[:, -60:].any(), (n, fill)
            assert np.array_equal(body, want), (n, fill)
            assert (out[n * rb:] == fill).all(), (n, fill)


@pytest.mark.parametrize("dim", KF.RECORD_DIMS)
def test_unpack_records(dim):
    from neural_spectral_codec_amd.encoding import quantization as qz
    L = _lib.lib()
    for n in KF.RECORD_N:
        rec = KF.records(n, dim)
        dirty = KF.with_reserved(KF.records_reference(rec), rec)             # reserved bytes are garbage
        assert dirty[:, -60:].any(1).all()
        want = [rec.q.view(np.uint8).reshape(-1), rec.pose7.reshape(-1), rec.ts.reshape(-1), rec.ids.reshape(-1),
                rec.hashes.reshape(-1)]
        q, p7, ts, ids, hs = qz.unpack_records(dev(dirty), dim)
        assert q.dtype == torch.uint16 and ids.dtype == torch.uint32 and ts.dtype == torch.float64
        for t, w in zip((q, p7, ts, ids, hs), want):
            assert np.array_equal(np.ascontiguousarray(host(t)).view(np.uint8).reshape(-1), w), n
        # through the C ABI into pre-filled outputs: all of each field written, nothing beyond it
        rdev = dev(dirty)
        for fill in (0xFF, 0x00):
            outs = [torch.full((len(w) + GUARD,), fill, dtype=torch.uint8, device="cuda") for w in want]
            st = L.nsc_unpack_records(_lib.ptr(rdev), n, dim, *[_lib.ptr(o) for o in outs], _lib.stream_ptr(rdev.device))
            assert st == 0
            for o, w in zip(outs, want):
                got = host(o)
                assert np.array_equal(got[:len(w)], w), (n, fill)
                assert (got[len(w):] == fill).all(), (n, fill)


# ----------------------------------------------------------------------------------------------------------------------
# chain graph
# ----------------------------------------------------------------------------------------------------------------------
def _poses(n):
    from neural_spectral_codec_amd import synth
    return synth.make_pose_chain(n, 11 + n) if n else np.zeros((0, 4, 4))


def _ulp_rows(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def _check_graph(n, m, loops, poses, ref):
    """One build with poses, one without; edge_attr at the bar of test_chain_graph_gpu (2 ulp, or 1e-7 absolute)."""
    from neural_spectral_codec_amd.keyframe.graph_manager import build_chain_graph
    ei, ea = ref
    x = torch.zeros((n, 8))
    g = build_chain_graph(x, m, "cuda", poses, loops)
    assert g.edge_index.dtype == torch.int64 and tuple(g.edge_index.shape) == (2, ei.shape[1]), (n, m, loops)
    assert np.array_equal(host(g.edge_index), ei), (n, m, loops)
    if ea is None:
        assert g.edge_attr is None or g.edge_attr.numel() == 0
    else:
        got = host(g.edge_attr)
        assert got.shape == ea.shape and np.isfinite(got).all()
        close = np.abs(got - ea) <= 1e-7
        bad = ~(close | (_ulp_rows(got, ea) <= 2))
        assert not bad.any(), (n, m, loops, ei[:, np.where(bad.any(1))[0][:4]].tolist(), got[bad][:4], ea[bad][:4])
        k = len(KF.valid_loops(n, loops))
        if k:                                                # the two directions of a loop closure: identical features
            tail = u32(got[len(got) - 2 * k:]).reshape(k, 2, 2)
            assert np.array_equal(tail[:, 0], tail[:, 1]), (n, m, loops)
    g2 = build_chain_graph(x, m, "cuda", None, loops)
    assert g2.edge_attr is None and np.array_equal(host(g2.edge_index), ei), (n, m, loops)


@pytest.mark.parametrize("m", range(13))
def test_chain_graph_grid(m):
    for n in range(13):
        assert (n, m) in KF.chain_grid()
        poses = _poses(n)
        for loops in KF.loop_lists(n).values():
            _check_graph(n, m, loops, poses, ko.chain_graph_loop(n, m, poses, loops))


@pytest.mark.parametrize("n,m", [nm for nm in KF.chain_grid() if nm[0] > 12 or nm[1] > 12])
def test_chain_graph_large(n, m):
    poses = _poses(n)
    lists = KF.loop_lists(n)
    for name in (("none", "repeats") if n > 1000 else tuple(lists)):
        _check_graph(n, m, lists[name], poses, ko.chain_graph_loop(n, m, poses, lists[name]))


def test_chain_graph_special_poses():
    names, poses = KF.poses_special()
    n = len(poses)
    for m, loops in ((2 * n, [(9, 9), (12, 0), (0, 12)]), (2 * n + 1, None), (5, [(0, 10), (11, 13), (5, 5)]),
                     (n, [(i, j) for i in range(n) for j in range(n) if abs(i - j) > n // 2])):
        _check_graph(n, m, loops, poses, ko.chain_graph_loop(n, m, poses, loops))


# ----------------------------------------------------------------------------------------------------------------------
# voxel overlap
# ----------------------------------------------------------------------------------------------------------------------
def _overlap(pairs, voxel):
    from neural_spectral_codec_amd.data import pose_utils as pu
    iou, counts = pu.compute_overlap_batch([np.array(p.p1) for p in pairs], [np.array(p.p2) for p in pairs],
                                           np.stack([p.T for p in pairs]), voxel_size=voxel,
                                           max_points=KF.VOX_MAX_POINTS, return_counts=True)
    return host(iou), host(counts)


def _check_batch(pairs, ref, what):
    voxel = pairs[0].voxel
    assert all(p.voxel == voxel for p in pairs)
    iou, counts = _overlap(pairs, voxel)
    for i, p in enumerate(pairs):
        want_iou, want_counts = ref[p.name]
        assert counts[i].tolist() == want_counts.tolist(), (what, p.name, i)
        assert float(iou[i]) == want_iou, (what, p.name, i)


@pytest.mark.parametrize("stride", [3, 4])
def test_voxel_overlap_one_pair_per_call(stride):
    ref = KF.cloud_reference(stride)
    for p in KF.cloud_pairs(stride):
        _check_batch([p], ref, "single")


@pytest.mark.parametrize("stride", [3, 4])
def test_voxel_overlap_batched_both_orders_and_shuffled(stride):
    ref = KF.cloud_reference(stride)
    pairs = KF.cloud_pairs(stride)
    voxels = sorted({p.voxel for p in pairs})
    assert len(voxels) == 2                                  # one launch per voxel size
    for v in voxels:
        order = KF.batch_order([p for p in pairs if p.voxel == v])
        _check_batch(order, ref, "batch")
        _check_batch(order[::-1], ref, "reversed")
        _check_batch([KF.shuffled(p, seed=5 + i) for i, p in enumerate(order)], ref, "shuffled")


def test_voxel_overlap_over_capacity_guard():
    """One direct call whose middle pair holds 12 289 points while max_pair_points says 12 288: the kernel's own guard
    answers (-1, -1, -1) and -1.0 for it before touching the table; the pairs around it are correct."""
    L = _lib.lib()
    pairs = KF.guard_batch(3)
    n = [len(p.p1) + len(p.p2) for p in pairs]
    assert n[1] == KF.VOX_MAX_POINTS + 1 and max(n[0], n[2]) <= 100
    p1 = dev(np.concatenate([p.p1 for p in pairs]))
    p2 = dev(np.concatenate([p.p2 for p in pairs]))
    off1 = dev(np.concatenate([[0], np.cumsum([len(p.p1) for p in pairs])]).astype(np.int64))
    off2 = dev(np.concatenate([[0], np.cumsum([len(p.p2) for p in pairs])]).astype(np.int64))
    T = dev(np.stack([p.T for p in pairs]).reshape(3, 16))
    t1, t2 = int(p1.shape[0]), int(p2.shape[0])
    nbytes = L.nsc_voxel_overlap_workspace_bytes(t1, t2)
    assert nbytes == 16 * (t1 + t2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    counts = torch.full((3, 3), 7, dtype=torch.int32, device="cuda")
    iou = torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
    st = L.nsc_voxel_overlap(_lib.ptr(p1), _lib.ptr(off1), _lib.ptr(p2), _lib.ptr(off2), 3, t1, t2, KF.VOX_MAX_POINTS, 3,
                             _lib.ptr(T), C.c_double(KF.V), _lib.ptr(counts), _lib.ptr(iou), _lib.ptr(ws), nbytes,
                             _lib.stream_ptr(p1.device))
    assert st == 0
    counts, iou = host(counts), host(iou)
    assert counts[1].tolist() == [-1, -1, -1] and iou[1] == -1.0
    for i in (0, 2):
        want_iou, want_counts = ko.voxel_overlap(pairs[i].p1, pairs[i].p2, pairs[i].T, KF.V)
        assert counts[i].tolist() == want_counts.tolist() and iou[i] == want_iou and want_counts[2] > 0
