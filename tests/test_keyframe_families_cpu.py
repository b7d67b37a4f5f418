"""The keyframe families (tests/keyframe_families.py) without a GPU.

Admits every family against something other than the kernels: the oracle's quantiser against the literal numpy lines of
the reference, its pairwise sum against ndarray.sum(), the C voxel oracle (sort and merge) against np.unique, the
closed-form edge count (a host function of the library) against the literal loop.  Checks that each family has the
property it is named for, that Python restatements of the mutants named in DESIGN 4.7a give other results than the oracle
on the family meant to catch them, and that the path table has no gaps.
"""
import math

import numpy as np
import pytest

import keyframe_families as KF
import keyframe_oracle as ko
from keyframe_families import EPS32, F32, MAX_U16


def u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------------
# the reference's lines (src/encoding/quantization.py:131-168 and :170-191), numpy calls as the reference makes them
# ----------------------------------------------------------------------------------------------------------------------
def literal_quantize(histogram, epsilon=1e-8, max_value=65535, rnd=np.round, normalise=lambda s, e: s > e,
                     pick=np.argmax, clamp=True):
    hist_sum = histogram.sum()                                                            # :144
    if normalise(hist_sum, epsilon):                                                      # :145
        histogram = histogram / (hist_sum + epsilon)
    quantized = rnd(histogram * max_value).astype(np.uint16)                              # :150
    quantized_sum = quantized.sum()                                                       # :154
    if quantized_sum > 0:
        error = max_value - int(quantized_sum)                                            # :157
        if error != 0:
            max_idx = pick(quantized)                                                     # :161
            new_val = int(quantized[max_idx]) + error
            quantized[max_idx] = np.clip(new_val, 0, max_value) if clamp else new_val % 65536   # :162-166
    return quantized


def literal_dequantize(quantized, epsilon=1e-8):
    histogram = quantized.astype(np.float32)                                              # :181
    hist_sum = histogram.sum()
    if hist_sum > epsilon:
        return histogram / (hist_sum + epsilon)
    return np.ones(len(quantized), dtype=np.float32) / len(quantized)


def round_half_away(x):
    return np.where(x >= 0, np.floor(x + F32(0.5)), np.ceil(x - F32(0.5))).astype(np.float32)    # roundf


def last_max(q):
    return len(q) - 1 - int(np.argmax(q[::-1]))


# ----------------------------------------------------------------------------------------------------------------------
# histogram rows
# ----------------------------------------------------------------------------------------------------------------------
def test_dims_and_constants():
    d = KF.dims()
    assert set(range(1, 137)) <= set(d) and len(d) == len(set(d)) == 153
    for x in (255, 256, 257, 799, 800, 801, 1023, 1024, 1025, 2047, 2048, 2049, 4015, 4016, 4017, 4095, 4096):
        assert x in d
    assert KF.row_counts() == (1, 2, 3, 4, 5, 9)
    assert not KF.dynamic_lds(4016) and KF.dynamic_lds(4017) and KF.lds_bytes(4016) == 65536
    assert max(d) == KF.K["PW_MAX_DIM"] and max(len(KF.pw_leaves(x)) for x in d) <= KF.K["PW_MAX_LEAVES"]
    # the uneven splits the issue names
    for x in (257, 2049, 4095):
        assert {"split", "uneven-split", "tail"} <= KF.leaf_kinds(x), (x, KF.pw_leaves(x))
    assert KF.pw_leaves(257) == [(0, 128), (128, 64), (192, 65)] and "uneven-split" not in KF.leaf_kinds(4096)
    assert KF.leaf_kinds(3) == {"leaf<8"} and KF.leaf_kinds(8) == {"whole"} and "tail" in KF.leaf_kinds(129)
    from neural_spectral_codec_amd.data import pose_utils
    assert pose_utils.MAX_PAIR_POINTS == KF.VOX_MAX_POINTS == 12288 and KF.VOX_TABLE == 16384


def test_wide_rows_show_the_summation_order():
    for dim in KF.dims():
        w = KF.wide(dim, 9)
        assert w.dtype == np.float32 and w.shape == (9, dim) and np.isfinite(w).all() and (w >= 0).all()
        if dim >= 16:
            assert KF.order_shows(w) >= 0.5, dim
            assert float(w.max()) / float(w[w > 0].min()) > 1e4, dim
        if dim >= 8:                                     # and in the words, for the two wrong orders of the mutation list
            for i in range(0, 9, 2):
                assert KF.order_reaches_words(w[i], KF.leafseq_sum if i % 4 == 2 else KF.seq_sum), (dim, i)


def test_pairwise_sum_is_numpy_order_on_wide_rows():
    for dim in KF.dims():
        for r in KF.wide(dim, 9):
            assert ko.pairwise_sum_f32(r) == r.sum(), dim
    for dim in (7, 8, 129, 257, 4095):                   # the wrong orders are wrong: the restatement tells them apart
        r = KF.wide(dim, 9)[0]
        assert dim < 8 or KF.seq_sum(r) != ko.pairwise_sum_f32(r)
        assert dim >= 8 or KF.seq_sum(r) == ko.pairwise_sum_f32(r)


@pytest.mark.parametrize("chunk", range(8))
def test_oracle_quantizer_is_the_reference_lines(chunk):
    for dim in KF.dims()[chunk::8]:
        for name, (rows, q, d) in KF.quant_reference(dim).items():
            for i, r in enumerate(rows):
                assert np.array_equal(q[i], literal_quantize(r)), (dim, name, i)
                assert np.array_equal(u32(d[i]), u32(literal_dequantize(q[i]))), (dim, name, i)
                tot = int(q[i].astype(np.int64).sum())
                assert tot in (0, MAX_U16) or KF.quant_steps(r)["corr"] == "clamped", (dim, name, i, tot)
        w, d = KF.words_reference(dim)
        for i in range(len(w)):
            assert np.array_equal(u32(d[i]), u32(literal_dequantize(w[i]))), (dim, i)
        assert np.array_equal(u32(d[0]), u32(np.full(dim, F32(1) / F32(dim))))
        assert w[1].sum() == 1 and w[2].astype(np.int64).sum() == MAX_U16 and (w[3] == MAX_U16).all()
    assert KF.words(4096)[3].astype(np.float32).sum() > 2.0 ** 24


@pytest.mark.parametrize("dim", KF.TIE_DIMS)
def test_ties_family(dim):
    rows = KF.ties(dim)
    assert len(rows) == 5
    for r, (a, b) in zip(rows, KF.tie_pairs(dim)):
        assert r.sum() == F32(1.0) and KF.seq_sum(r) == F32(1.0) and KF.seq_sum(r[::-1]) == F32(1.0)      # dyadic: any order
        st = KF.quant_steps(r)
        assert st["norm"] and st["tot"] != MAX_U16 and st["tot"] == 65536
        mx = st["rounded"].max()
        assert np.array_equal(np.where(st["rounded"] == mx)[0], [a, b]) and st["first"] == a
        q = ko.quantize(r)
        assert q[a] == mx - 1 and q[b] == mx and int(q.astype(np.int64).sum()) == MAX_U16       # the first maximum pays
        assert not np.array_equal(literal_quantize(r, pick=last_max), q)                        # a rule that keeps the later one does not
    lanes = [(a % 64, b % 64) for a, b in KF.tie_pairs(dim)]
    assert (63, 0) in lanes and (5, 5) in lanes and (0, 0) in lanes      # first maximum in a higher lane; in the same lane


def test_excess_over_max_family():
    row = KF.excess_over_max()[0]
    assert len(row) == 4096 and np.all(row[:4000] == F32(0.52 / 65535)) and len(np.unique(row[4000:])) == 1
    st = KF.quant_steps(row)
    assert st["norm"] and st["tot"] == 67456 and st["rounded"].max() == 661 and st["corr"] == "clamped"
    q = ko.quantize(row)
    assert q[st["first"]] == 0 and int(q.astype(np.int64).sum()) == 66795
    assert np.array_equal(q, literal_quantize(row))
    assert not np.array_equal(literal_quantize(row, clamp=False), q)                            # without `v < 0 -> 0`


def test_half_ties_family():
    vals = KF.half_tie_values()
    assert len(vals) == 321 and vals[:2] == (65408, 65410)
    assert float(F32(65408 / 131072.0) * F32(65535)) == 32703.5 and float(F32(65410 / 131072.0) * F32(65535)) == 32704.5
    for dim in KF.HALF_TIE_DIMS:
        rows, (odd, even) = KF.half_ties(dim)
        for r, m, parity in zip(rows, (odd, even), (1, 0)):
            assert r.sum() == F32(1.0) and KF.seq_sum(r) == F32(1.0) and float(r.astype(np.float64).sum()) == 1.0
            p = float(KF.quant_steps(r)["prod"][dim // 2])
            assert p % 1.0 == 0.5 and int(p) % 2 == parity and r[dim // 2] == F32(m / 131072.0)
            assert int(np.argmax(r)) == 0 and r[0] == 0.5                        # the correction lands elsewhere
        assert not np.array_equal(literal_quantize(rows[1], rnd=round_half_away), ko.quantize(rows[1]))   # roundf


def test_eps_edge_family():
    for dim in KF.dims():
        rows = KF.eps_edge(dim)
        s = [r.sum() for r in rows]
        assert s[0] == 0 and s[1] == EPS32 and s[2] == np.nextafter(EPS32, F32(1)) and s[2] > EPS32
        assert (rows[3] == 1).sum() == 1 and s[3] == 1 and len(np.unique(rows[4])) == 1 and rows[4, 0] == F32(1) / F32(dim)
        assert [KF.quant_steps(r)["norm"] for r in rows] == [False, False, True, True, True]
        q = KF.quant_reference(dim)["eps_edge"][1]
        assert not q[0].any() and not q[1].any() and q[2].max() > 30000 and q[3].max() == MAX_U16
        assert not np.array_equal(literal_quantize(rows[1], normalise=lambda a, e: a >= F32(e)), q[1])   # `>=` for `>`


# ----------------------------------------------------------------------------------------------------------------------
# records
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", KF.RECORD_DIMS)
def test_records_round_trip(dim):
    for n in KF.RECORD_N:
        rec = KF.records(n, dim)
        block = np.concatenate([rec.pose7, rec.ts, rec.ids, rec.hashes, rec.reserved], 1)
        assert block.shape == (n, 120) and all(len(set(b.tolist())) == 120 for b in block)
        packed = KF.records_reference(rec)
        assert packed.shape == (n, 2 * dim + 120) and packed.dtype == np.uint8
        assert np.array_equal(packed[:, 2 * dim:2 * dim + 60], block[:, :60]) and not packed[:, -60:].any()
        assert np.array_equal(packed[:, :2 * dim], rec.q.view(np.uint8).reshape(n, -1))
        for src in (packed, KF.with_reserved(packed, rec)):                   # from_bytes never reads the reserved bytes
            for i in (0, n // 2, n - 1):
                q, pose, ts, kid, hsh = ko.unpack_record(src[i].tobytes(), dim)
                assert np.array_equal(q, rec.q[i]) and np.array_equal(pose.view(np.uint8), rec.pose7[i])
                assert np.array_equal(np.array([ts]).view(np.uint8), rec.ts[i])
                assert kid == int(rec.ids[i].view(np.uint32)[0]) and hsh == rec.hashes[i].tobytes()


# ----------------------------------------------------------------------------------------------------------------------
# chain graphs
# ----------------------------------------------------------------------------------------------------------------------
def test_edge_count_is_the_literal_loop():
    from neural_spectral_codec_amd import _lib
    L = _lib.lib()
    grid = KF.chain_grid()
    assert len(grid) == 173 and {(0, 0), (12, 12), (3, 12), (300, 5), (64, 9), (4541, 5), (7, 64)} <= set(grid)
    for n, m in grid:
        for name, loops in KF.loop_lists(n).items():
            ok = KF.valid_loops(n, loops)
            ei = ko.chain_graph_loop(n, m, None, loops)[0]
            assert L.nsc_chain_graph_num_edges(n, m, len(ok)) == ei.shape[1], (n, m, name)
    assert L.nsc_chain_graph_num_edges(-1, 5, 0) == -1 and L.nsc_chain_graph_num_edges(5, -1, 0) == -1
    lists = KF.loop_lists(9)
    assert lists["none"] is None and len(lists["one"]) == 1 and len(set(lists["repeats"])) < len(lists["repeats"])
    assert all(q == m for q, m in lists["self"]) and len(KF.valid_loops(9, lists["out_of_range"])) == 1


def scalar_edge_feature(poses, i, j):
    """The two features of one edge with math.* scalars (an independent libm), float64 -> float32 where the reference
    rounds."""
    d, tr = KF.edge_quantities(poses, i, j)
    tr = min(max(tr, -1.0), 3.0)
    ang = F32(math.acos(min(max((tr - 1.0) / 2.0, -1.0), 1.0)))
    return F32(math.log1p(float(F32(d)))) / F32(5.0), ang / F32(np.pi)


def test_special_poses_have_their_property_and_the_bar_is_attainable():
    names, poses = KF.poses_special()
    n = len(poses)
    idx = {k: i for i, k in enumerate(names)}
    q = lambda a, b: KF.edge_quantities(poses, idx[a], idx[b])                      # noqa: E731
    assert q("eye", "eye_again") == (0.0, 3.0) and q("eye", "t1e-9")[0] == 1e-9 and q("eye", "t1")[0] == 1.0
    assert q("eye", "t1e6")[0] == 1e6 and q("eye", "rz_pi")[1] == -1.0 and q("eye", "rz_pi2")[1] == 1.0
    assert q("eye", "rz_1e-8")[1] == 3.0 and 3.0 - 2e-8 < q("eye", "rz_1e-4")[1] < 3.0
    assert q("scale_up", "scale_up_again")[1] > 3.0 and q("scale_up", "scale_up_rz_pi")[1] < -1.0
    assert q("scale_down", "scale_down_rz_pi")[1] > -1.0 and q("scale_up", "scale_down")[1] < 3.0
    ei, ea = ko.chain_graph_loop(n, 2 * n, poses, [(9, 9), (12, 0), (0, 12)])
    assert ei.shape[1] == n * (n - 1) + 6                                           # every pair is an edge
    a = ea.view(np.int32).astype(np.int64)
    for e, (i, j) in enumerate(ei.T):
        mine = np.array(scalar_edge_feature(poses, i, j) if e < n * (n - 1) else scalar_edge_feature(poses, *ei[:, e - e % 2]),
                        dtype=np.float32)
        ulp = np.abs(mine.view(np.int32).astype(np.int64) - a[e])
        assert ((ulp <= 2) | (np.abs(mine - ea[e]) <= 1e-7)).all(), (names[i], names[j], mine, ea[e])
    assert np.array_equal(ea[-2], ea[-1]) and np.array_equal(ea[-6], ea[-5])        # both directions carry (q, m)
    assert ea[:, 1].max() == 1.0 and ea[:, 1].min() == 0.0


# ----------------------------------------------------------------------------------------------------------------------
# clouds
# ----------------------------------------------------------------------------------------------------------------------
def test_vox_hash_restatements_agree():
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.integers(-2 ** 31, 2 ** 31, (500, 3)), rng.integers(-50, 50, (500, 3)),
                        [[0, 0, 0], [-1, -1, -1], [2 ** 31 - 1, -2 ** 31, 5]]])
    want = [KF.vox_hash(int(x), int(y), int(z)) for x, y, z in v]
    assert KF.vox_hash_np(v).tolist() == want and len(set(want)) > 990
    assert KF.vox_hash(0, 0, 0) == 0 and KF.vox_hash(1, 0, 0) != KF.vox_hash(0, 1, 0)


@pytest.mark.parametrize("stride", [3, 4])
def test_oracle_overlap_is_the_numpy_restatement(stride):
    pairs = KF.cloud_pairs(stride)
    ref = KF.cloud_reference(stride)
    assert {p.name.split("/")[0].rstrip("0123456789") for p in pairs} == {"collide", "wrap", "full", "one_slot", "empty",
                                                                         "faces", "rigid"}
    for p in pairs:
        iou, counts = ref[p.name]
        n_iou, n_counts = KF.overlap_np(p)
        assert counts.tolist() == n_counts and iou == n_iou, p.name
        sh = KF.shuffled(p)
        assert ko.voxel_overlap(sh.p1, sh.p2, sh.T, sh.voxel)[1].tolist() == n_counts, p.name
    for b in KF.guard_batch(stride):
        assert ko.voxel_overlap(b.p1, b.p2, b.T, b.voxel)[1].tolist() == KF.overlap_np(b)[1]
    c = {p.name: ref[p.name][1].tolist() for p in pairs}
    for k in (2, 8, 40):
        assert c["collide%d/cloud1" % k] == [k, 0, 0] and c["collide%d/cloud2" % k] == [0, k, 0]
        a = (2 * k + 2) // 3
        assert c["collide%d/split" % k] == [a, k - k // 3, a - k // 3] and a - k // 3 > 0
    assert c["wrap/lookup"] == [12, 14, 12] and c["wrap/cloud2"] == [0, 14, 0]
    assert c["full/12288+0"] == [12288, 0, 0] and c["full/0+12288"] == [0, 12288, 0]
    assert c["full/disjoint"] == [6144, 6144, 0] and c["full/identical"] == [6144, 6144, 6144]
    assert c["one_slot/cloud1"] == [1, 0, 0] and c["one_slot/cloud2"] == [0, 1, 0]
    assert c["one_slot/plus_one"] == [2, 0, 0] and c["one_slot/two_voxels"] == [2, 2, 2]
    assert c["empty/both"] == [0, 0, 0] and c["empty/dead_both"] == [0, 0, 0] and ref["empty/both"][0] == 0.0
    assert c["empty/dead1"][0] == 0 and c["empty/dead2"][1] == 0 and c["empty/n1=0"][0] == 0 and c["empty/n2=0"][1] == 0
    assert c["rigid"][2] > 1000 and c["rigid"][2] < min(c["rigid"][:2])
    sizes = {p.name: len(p.p1) + len(p.p2) for p in pairs}
    assert max(sizes.values()) == 12288 and sum(v == 12288 for v in sizes.values()) >= 8


@pytest.mark.parametrize("stride", [3, 4])
def test_cloud_families_have_their_property(stride):
    by = {p.name: p for p in KF.cloud_pairs(stride)}
    slot = KF.fullest_slot()
    for k in (2, 8, 40):
        for variant in ("cloud1", "cloud2", "split"):
            v1, v2 = KF.voxels_np(by["collide%d/%s" % (k, variant)])
            vox = np.unique(np.concatenate([v1, v2]), axis=0)
            assert len(vox) == k and {KF.home_slot(*v) for v in vox.tolist()} == {slot}          # the Python-integer hash
    # wrap: the occupied set of a linear-probing table does not depend on the insertion order
    v1, v2 = KF.voxels_np(by["wrap/lookup"])
    homes = sorted(KF.home_slot(*v) for v in v1.tolist())
    assert homes == sorted(list(KF.WRAP_SLOTS) * 3)
    for order in (v1, v1[::-1], v1[np.random.default_rng(3).permutation(len(v1))]):
        table, br = KF.probe_table(order, order[:0])
        assert set(table) == set(range(16380, 16384)) | set(range(0, 8)) and "insert-after-wrap" in br
    table, br = KF.probe_table(v1, v2)
    assert set(table) == set(range(16380, 16384)) | set(range(0, 10)) and "match-set1-after-wrap" in br
    assert {KF.home_slot(*table[s]) for s in (8, 9)} == {0, 1}                   # the late voxels sit behind the chain
    # full: 12 288 distinct voxels, exactly the capacity; lattice points are exact in both precisions
    v1, v2 = KF.voxels_np(by["full/12288+0"])
    assert len(np.unique(v1, axis=0)) == KF.VOX_MAX_POINTS == len(v1) and len(v2) == 0
    assert np.array_equal(np.sort(v1.view("i4,i4,i4").ravel()), np.sort(KF.full_voxels().astype(np.int32).view("i4,i4,i4").ravel()))
    v1, v2 = KF.voxels_np(by["full/disjoint"])
    assert np.array_equal(np.unique(np.concatenate([v1, v2]), axis=0), np.unique(KF.full_voxels(), axis=0))
    for name in ("one_slot/cloud1", "one_slot/cloud2"):
        v1, v2 = KF.voxels_np(by[name])
        assert len(v1) + len(v2) == 12288 and len(np.unique(np.concatenate([v1, v2]), axis=0)) == 1
    # empties: the dead rows are all dropped, by each of the three reasons
    p = by["empty/dead_both"]
    assert len(KF.voxels_np(p)[0]) == 0 and len(KF.voxels_np(p)[1]) == 0
    assert np.isnan(p.p1[:, 0]).any() and np.isinf(p.p1[:, 1]).any() and (stride == 3 or np.isnan(p.p1[:, 3]).any())
    # faces: the two precisions disagree somewhere, and 0.6 / 0.2 is where the issue says
    p = by["faces/v0.2"]
    v1, v2 = KF.voxels_np(p)
    assert len(v1) == len(v2) == len(p.p1) and (v1 != v2).any()
    assert np.float64(F32(0.6)) / 0.2 != np.float64(F32(0.6) / F32(0.2)) and F32(0.6) in p.p1[:, 0]
    vals = KF.face_values(0.25).tolist()
    assert {0.25, -0.25, 1e6, -1e6, 1.5e6, -1.5e6, float(KF.FLT_MAX), -float(KF.FLT_MAX)} <= set(vals)
    assert np.signbit(KF.face_values(0.25)[0]) and float(np.nextafter(F32(0.25), F32(1))) in vals
    assert np.abs(np.concatenate([v1, v2])).max() == 5000000                     # clipped at 1e6 / 0.2
    # rigid: the fma chain of the oracle is numpy's T @ hom.T (overlap_np uses the latter; counts equal above), and the
    # transform matters
    p = by["rigid"]
    assert not np.array_equal(p.T, np.eye(4)) and abs(np.linalg.det(p.T[:3, :3]) - 1) < 1e-12
    assert ko.voxel_overlap(p.p1, p.p2, np.eye(4), p.voxel)[1][2] < 100


def test_batch_order_alternates_empty_and_full():
    order = KF.batch_order([p for p in KF.cloud_pairs(3) if p.voxel == KF.V])
    sizes = [len(p.p1) + len(p.p2) for p in order]
    assert sizes[0::2][:4] == [12288] * 4 and sizes[1] == 0 and max(sizes[1::2][:4]) <= 8
    assert sorted(p.name for p in order) == sorted(p.name for p in KF.cloud_pairs(3) if p.voxel == KF.V)
    g = KF.guard_batch()
    assert [len(p.p1) + len(p.p2) for p in g][1] == KF.VOX_MAX_POINTS + 1


def test_probe_mutants_are_seen():
    """The probe loop restated with its step as a parameter: step 1 gives the oracle's counts on the collision, wrap and
    capacity families.  (The dropped wrap mask runs off the table and is never run; wrap/* and full/* reach 16383 -> 0.)"""
    def counts_with_step(pair, step):
        v1, v2 = KF.voxels_np(pair)
        table, n = {}, [0, 0, 0]
        for which, vs in ((0, v1), (1, v2)):
            for v in map(tuple, vs.tolist()):
                h = KF.home_slot(*v)
                while h in table and table[h][0] != v:
                    h = (h + step) & KF.VOX_MASK
                if h not in table:
                    table[h] = [v, which, False]
                    n[which] += 1
                elif which == 1 and table[h][1] == 0 and not table[h][2]:
                    table[h][2] = True
                    n[2] += 1
        return [n[0], n[1] + n[2], n[2]]
    by = {p.name: p for p in KF.cloud_pairs(3)}
    for name in ("collide40/split", "wrap/lookup", "full/identical", "rigid"):
        assert counts_with_step(by[name], 1) == KF.cloud_reference(3)[name][1].tolist(), name
    # a step of 2 is another valid probe sequence over the half of the table that shares the home slot's parity: every
    # voxel still finds its own entry, so the counts cannot tell it from a step of 1 -- an equivalent mutant as long as
    # no more than 8 192 voxels share a parity (beyond that it would not terminate)
    for name in ("collide40/split", "wrap/lookup", "full/identical"):
        assert counts_with_step(by[name], 2) == KF.cloud_reference(3)[name][1].tolist(), name
    v1, _ = KF.voxels_np(by["full/12288+0"])
    homes = np.array([KF.home_slot(*v) for v in v1.tolist()])
    assert max(np.bincount(homes % 2)) <= KF.VOX_TABLE // 2


def test_no_coverage_gaps():
    assert KF.coverage_gaps() == []
    kernels = {c.kernel for c in KF.cases()}
    assert kernels == set(KF.REQUIRED) and len(kernels) == 6
    fams = {c.family.split("/")[0] for c in KF.cases()}
    assert {"wide", "ties", "excess_over_max", "half_ties", "eps_edge", "words", "records", "chain_grid", "poses_special",
            "wrap", "full", "one_slot", "empty", "faces", "rigid", "guard"} <= fams
