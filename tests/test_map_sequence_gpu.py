"""The kept map under sequences of calls on the MI355X: MapLocalizer's device calls against the composed model of
tests/map_sequence_cases.py after every operation, against a fresh build over the clouds that remain, and the row passes
and the index clear past one sweep of their grids.  tests/test_map_sequence_cpu.py asserts the claims of the inputs.

Every comparison is by bits.  Against the model these are the integers: stats, cursor, the typed outputs of every call,
keys, info and moments up to stats[1], the index read as a mapping key -> place, and of the records the usable flag and
the zero records.  The other doubles of a record are the device's evaluation of count, moments and key, and the model's are
exact rationals rounded once, so they are compared, by bits too, with the device's own evaluation of the same integers: a
rebuild over the clouds that remain (within capacity, all of it; past capacity, every voxel whose integers the rebuild
over the clouds the model holds also has), a second run, and the restated move of the device's own source."""
import numpy as np
import pytest
import torch

import map_insert_cases as IK
import map_localize_cases as K
import map_rehash_restatement as HR
import map_replace_cases as PK
import map_sequence_cases as S
from test_map_insert_cpu import group, joined
from test_map_insert_gpu import assert_same_bits, captured, kept, rebuilt
from test_map_localize_gpu import dev, index_of, localizer
from test_map_rehash_gpu import EMPTY, OUTS, REGISTERED, assert_restated, lattice_map, resized
from test_map_replace_gpu import assert_follows, mapping

pytestmark = pytest.mark.gpu


def devs(part):
    return tuple(None if x is None else dev(x) for x in part)


def apply_device(m, op):
    """one operation of tests/map_sequence_cases.py through the device calls -> the call's typed outputs on the host"""
    kind, a = op
    if kind == "resize":
        out = m.resize_device(a["max_voxels"], compact=a["compact"])
        return {k: out[k].cpu().numpy() for k in OUTS}
    p, o, T, ids = S.four(a["part"])
    pts, off, poses, ids = devs((p, o, np.asarray(T, np.float64), ids))
    if kind == "build":
        m.build_device(pts, off, poses, ids)
    elif kind == "insert":
        m.insert_device(pts, off, poses, ids)
    elif kind == "remove":
        return dict(removed=m.remove_device(pts, off, poses, ids)["removed"].cpu().numpy())
    else:
        out = m.replace_device(pts, off, poses, dev(a["new"]), ids, first_row=a["first_row"], first_cloud=a["first_cloud"])
        return dict(removed=out["removed"].cpu().numpy(), placed=out["placed"].cpu().numpy())
    return {}


def assert_clean_index(got, what=""):
    """in the whole index an empty slot is (0, ~0) and no place word has a bit at or above 36 set"""
    idx = got["index"].view(np.uint64)
    assert (idx[idx[:, 0] == 0, 1] == EMPTY).all(), what
    assert not (idx[idx[:, 1] != EMPTY, 1] >> np.uint64(36)).any(), what


def assert_arrays(got, ref, what=""):
    """kept tensors on the host against a map of the restatements (map_insert_restatement.arrays)"""
    cap = int(ref["capacity"])
    assert len(got["keys"]) == cap and got["stats"].tolist() == ref["stats"].tolist(), (what, got["stats"], ref["stats"])
    assert got["cursor"].tolist() == list(ref["cursor"]), (what, got["cursor"], ref["cursor"])
    n = int(ref["stats"][1])
    assert np.array_equal(got["keys"][:n], ref["keys"][:n]), what
    assert np.array_equal(got["info"][:n], ref["info"][:n]), (what, np.nonzero((got["info"][:n] != ref["info"][:n]).any(1))[0][:8])
    assert np.array_equal(got["moments"][:n], np.array(ref["moments"][:n].tolist(), np.int64).reshape(n, 9)), what
    assert np.array_equal(got["voxels"][:n, 15], ref["voxels"][:n, 15]), what
    none = ref["info"][:n, 0] <= 0
    assert got["voxels"][:n][none].tobytes() == bytes(128 * int(none.sum())), what
    assert_clean_index(got, what)
    places, occupied = index_of(got)
    want = {k: (p if p < cap else -1) for k, p in ref["place"].items()}
    assert places == want and occupied == len(want), what


def assert_same_function(got, want, share=0.0, what=""):
    """a record is a function of count, moments and key alone: wherever the kept map ``got`` and the build ``want`` hold
    a key with the same count and moments, they hold the same record; at least ``share`` of the voxels of ``got`` that
    hold rows are compared"""
    g, w = mapping(got), mapping(want)
    same = [k for k in g if k in w and g[k][:2] == w[k][:2]]
    assert all(g[k][2] == w[k][2] for k in same), what
    assert same and len(same) >= share * sum(v[0] > 0 for v in g.values()), (what, len(same))


def run(max_voxels, ops, rebuild=False, share=None, **options):
    """the operations on the device and in the model, compared after every one -> (the localizer, the model)"""
    m, md = localizer(insertable=True, max_voxels=max_voxels, **options), S.Model(max_voxels)
    for i, op in enumerate(ops):
        what = (i, op[0])
        src = kept(m) if op[0] == "resize" else None
        out, want = apply_device(m, op), md.apply(op)
        got = kept(m)
        assert m.capacity == md.max_voxels, what
        assert_arrays(got, md.arrays(), what)
        for k in ("removed", "placed"):
            assert (k in out) == (k in want) and (k not in out or out[k].tolist() == list(want[k])), (what, k, out.get(k), want.get(k))
        if op[0] == "resize":
            for k in OUTS:
                assert np.array_equal(out[k], want[k]), (what, k)
            assert_restated(got, out, HR.rehash(src, not op[1]["compact"], m.capacity), what)      # the move copies: by bits
        if rebuild and md.held:
            emptied = assert_follows(got, rebuilt([md.remaining()], max_voxels=md.max_voxels), what)
            assert len(emptied) == len(md.emptied()), what
        elif rebuild:                                                    # nothing remains: every voxel is emptied
            assert len(md.emptied()) == got["stats"][1], what
        if share is not None:
            assert_same_function(got, rebuilt([md.remaining()], max_voxels=4096), share, what)
    return m, md


# ---- 1. seeded sequences ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", S.WITHIN_SEEDS)
def test_within_capacity_sequence_equals_the_model_and_the_rebuild(seed):
    """after every operation: the model, and a GPU rebuild over the clouds that remain, by mapping"""
    run(*S.sequence(seed), rebuild=True)


@pytest.mark.parametrize("seed", S.PAST_SEEDS)
def test_past_capacity_sequence_equals_the_model(seed):
    run(*S.sequence(seed), share=S.PAST_SHARE)


# ---- 2. named chains --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(S.CHAINS))
def test_named_chain_equals_the_model_step_by_step(name):
    cap, ops, _ = S.CHAINS[name]()
    within = name in ("revival", "refill", "numbered_below")
    run(cap, ops, rebuild=within, share=None if within else 0.0)


# ---- 3. the round trip on the scene -----------------------------------------------------------------------------------

@pytest.mark.parametrize("options", [dict(), dict(kernel="cauchy", robust_scale=3.0, neighbours=7)],
                         ids=["plain", "cauchy-7"])
def test_scene_round_trip_registers_as_the_rebuild(options):
    s = K.scene()
    cap, ops = S.scene_round_trip()
    m = localizer(insertable=True, max_voxels=cap, **options)
    for op in ops:
        apply_device(m, op)
    whole = localizer(max_voxels=16384, **options)
    whole.build_device(dev(s["points"]), dev(s["offsets"]), dev(s["poses"]), moments=True)
    got, want = kept(m), kept(whole)
    assert m.capacity == 16384 and got["stats"][2:].tolist() == want["stats"][2:].tolist() == [24000, 0, 0, 0, 0]
    assert len(assert_follows(got, want, "round trip")) >= 1 and got["cursor"].tolist() == [28000, 7]
    assert_clean_index(got)
    scans = (dev(s["scans"]), dev(s["scan_offsets"]))
    a, b = m.register(scans, s["init"]), whole.register(scans, s["init"])
    for k in REGISTERED:
        assert torch.equal(a[k], b[k]), k
    assert bool((b["n_correspondences"] > 1000).all())


# ---- 4. the same sequence twice ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [S.WITHIN_SEEDS[3], S.PAST_SEEDS[1]])
def test_the_same_sequence_twice_gives_the_same_bits(seed):
    def once():
        cap, ops = S.sequence(seed)
        m = localizer(insertable=True, max_voxels=cap)
        outs = [apply_device(m, op) for op in ops]
        return kept(m), outs
    (a, oa), (b, ob) = once(), once()
    assert_same_bits(a, b)
    assert a["cursor"].tobytes() == b["cursor"].tobytes() and len(a["keys"]) == len(b["keys"])
    for x, y in zip(oa, ob):
        assert x.keys() == y.keys() and all(x[k].tobytes() == y[k].tobytes() for k in x)


# ---- 5. one captured chain --------------------------------------------------------------------------------------------

def test_one_captured_chain_replays_on_new_contents():
    """remove, insert and replace in one graph; the second replay works on other clouds in the same buffers"""
    from neural_spectral_codec_amd import _lib
    g = IK.general_split(np.float32)
    A, B, Co, Cn = (group(g, [n]) for n in ("A", "B", "C_old", "C_new"))
    there = lambda part: (part[0], part[1], PK.shifted(part[2], PK.B_SHIFT))
    rounds = [(Co, there(Co), A, there(A)[2]), (Cn, there(Cn), B, there(B)[2])]
    assert all(x.shape == y.shape for a, b in zip(*rounds) for x, y in zip(a, b))
    whole = joined([A, B, Co, Cn])
    m, md = localizer(insertable=True, max_voxels=512), S.Model(512)
    m.build_device(*devs(whole))
    md.build(whole)
    rem, ins, rep, new = devs(rounds[0][0]), devs(rounds[0][1]), devs(rounds[0][2]), dev(rounds[0][3])
    out = {}

    def chain():
        out["removed"] = m.remove_device(*rem)["removed"]
        m.insert_device(*ins)
        both = m.replace_device(*rep, new, first_row=0, first_cloud=0)
        out["replaced"], out["placed"] = both["removed"], both["placed"]
    graph, types = captured(chain)
    assert types == {"kernel": _lib.MAP_REMOVE_LAUNCHES + _lib.MAP_INSERT_LAUNCHES + _lib.MAP_REPLACE_LAUNCHES}, types
    assert_arrays(kept(m), md.arrays(), "a capture changes nothing")
    for i, (r, a, p, to) in enumerate(rounds):
        if i:
            for buffers, values in ((rem, r), (ins, a), (rep, p), ((new,), (to,))):
                for t, value in zip(buffers, values):
                    t.copy_(dev(value))
        graph.replay()
        torch.cuda.synchronize()
        removed = md.remove(r)["removed"]
        md.insert(a)
        want = md.replace(p, to, first_row=0, first_cloud=0)
        assert_arrays(kept(m), md.arrays(), ("round", i))
        assert out["removed"].tolist() == removed and out["replaced"].tolist() == want["removed"], i
        assert out["placed"].tolist() == want["placed"], i
    assert not md.facts["unmatched"] and len(assert_follows(kept(m), rebuilt([md.remaining()], max_voxels=512))) == len(md.emptied())


# ---- 6. row passes past one sweep -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", S.WRAP_SIZES)
def test_row_passes_past_one_sweep(n):
    """an insertion, a removal and a replacement of n rows: more than the 1 048 576 rows the workgroups of a row pass
    take in their first sweep"""
    from neural_spectral_codec_amd import _lib
    assert n > _lib.MAP_INSERT_ROWS * _lib.MAP_INSERT_BLOCKS == S.WRAP
    small, rows, ref = S.wrap_small()[:3], S.wrap_rows(n)[:3], S.wrap_reference(n)
    n_small, found = int(ref["small"]["stats"][0]), int(ref["inserted"]["stats"][0])
    touched = len(np.unique(S.keys_and_integers(S.wrap_rows(n), ref["small"]["grid"])[0]))       # the voxels the rows reach
    m = localizer(insertable=True, max_voxels=8192)
    m.build_device(*devs(small))
    base = kept(m)
    assert_arrays(base, ref["small"], "the small build")
    # the insertion: the vectorised reference, and the build over both by bits
    m.insert_device(*devs(rows))
    got = kept(m)
    assert_arrays(got, ref["inserted"], "inserted")
    assert_same_bits(got, rebuilt([small, rows], max_voxels=8192), "inserted, against the rebuild")
    # the removal: the small build again by bits, every voxel the big call made alone emptied
    removed = m.remove_device(*devs(rows))["removed"].tolist()
    after = kept(m)
    assert removed == [n, 0, 0, 0, 0, touched, found - n_small, 0], removed
    assert after["stats"].tolist() == [found, found] + base["stats"][2:].tolist() and after["cursor"].tolist() == [600 + n, 11]
    for k in ("voxels", "keys", "moments"):
        assert after[k][:n_small].tobytes() == base[k][:n_small].tobytes(), k
    assert np.array_equal(after["info"][:n_small, :2], base["info"][:n_small, :2])   # the cloud bounds stay as the insertion left them
    assert not after["info"][n_small:found, 0].any() and not after["moments"][n_small:found].any()
    assert after["voxels"][n_small:found].tobytes() == bytes(128 * (found - n_small))
    assert np.array_equal(after["keys"][:found], got["keys"][:found]) and np.array_equal(after["info"][:found, 1:], got["info"][:found, 1:])
    assert index_of(after) == index_of(got)
    assert_clean_index(after)
    # the replacement from one set of rot90 poses to another, numbered as the insertion numbered the rows
    m.insert_device(*devs(rows))
    out = m.replace_device(*devs(rows), dev(ref["new_poses"]), first_row=600, first_cloud=6)
    moved = kept(m)
    new = len(set(ref["moved"]["keys"].tolist()) - set(ref["inserted"]["keys"].tolist()))
    assert out["removed"].tolist() == [n, 0, 0, 0, 0, touched, found - n_small, 0], out["removed"]
    assert out["placed"].tolist() == [new, found + new, n, 0, 0, 0, 0], out["placed"]
    assert moved["stats"].tolist() == [found + new, found + new, 600 + n, 0, 0, 0, 0] and moved["cursor"].tolist() == [600 + 2 * n, 16]
    want = ref["moved"]
    held = mapping(moved)
    for i, key in enumerate(want["keys"].tolist()):
        assert held[key][0] == want["info"][i, 0] and held[key][1] == np.array(want["moments"][i].tolist(), np.int64).tobytes(), key
    emptied = assert_follows(moved, rebuilt([small, (rows[0], rows[1], ref["new_poses"])], max_voxels=8192), "re-placed")
    assert len(emptied) == found + new - int(want["stats"][0]) > 0
    places = index_of(moved)[0]
    first = {int(k): int(r) for k, r in zip(want["keys"], want["info"][:, 1])}
    made = [k for k in want["keys"].tolist() if places[k] >= found]
    assert len(made) == new and all(moved["info"][places[k], 1] == first[k] for k in made)      # the rows of the second sweep too
    assert_clean_index(moved)


# ---- 7. the index clear past one sweep --------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [262_145, 300_000])
def test_index_clear_past_one_sweep(size):
    """4 x size index words: more than the 1 048 576 words the workgroups of the clear take in their first sweep"""
    assert 4 * size > 256 * 4096
    m = lattice_map(257)
    src = kept(m)
    got, outs = resized(m, size)
    assert_restated(got, outs, HR.rehash(src, False, size), size)
    assert got["index"].shape == (2 * size, 2) and index_of(got)[1] == 257 - 86
