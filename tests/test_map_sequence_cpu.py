"""The kept map under sequences of calls without a GPU: the composed model of tests/map_sequence_cases.py against the
restated build over the clouds that remain (tests/map_localize_restatement.py, the independent reference) after every
operation, and the claims of the seeded sequences, the named chains, the scene round trip and the wrap-around rows that
tests/test_map_sequence_gpu.py relies on."""
import numpy as np
import pytest

import map_insert_cases as IK
import map_insert_restatement as IR
import map_localize_cases as K
import map_localize_restatement as R
import map_replace_restatement as PR
import map_sequence_cases as S
from map_sequence_cases import EMPTIED, MISSING


def run(max_voxels, ops):
    """the model after every operation -> [(operation, what the call returns, the model's arrays, facts, max_voxels)]"""
    m, out = S.Model(max_voxels), []
    for op in ops:
        res = m.apply(op)
        out.append((op, res, m.arrays(), dict(m.facts), m.max_voxels))
    return m, out


def places(a, vox):
    """the place of each of the voxels ``vox`` in the model's arrays: None for a key it lacks, -1 past the capacity"""
    at = [a["place"].get(IK.voxel_key(v)) for v in vox]
    return [p if p is None or p < a["capacity"] else -1 for p in at]


# ---- 1. the composed model against the rebuild -------------------------------------------------------------------------

@pytest.mark.parametrize("seed", S.WITHIN_SEEDS)
def test_model_follows_the_rebuild_after_every_operation(seed):
    max_voxels, ops = S.sequence(seed)
    m = S.Model(max_voxels)
    for i, op in enumerate(ops):
        m.apply(op)
        got, want = m.arrays(), m.rebuild()
        assert got["stats"][0] <= m.max_voxels and want["stats"][0] <= m.max_voxels, (i, op[0])
        assert PR.assert_follows(got, want, (seed, i, op[0])) == len(m.emptied()), (i, op[0])
        assert not m.inconsistent() and m.facts.get("unmatched", 0) == 0, (i, op[0])
        # the rows the map counts are the rows the rebuild uses; what it dropped it never counts twice
        assert got["stats"][2] == want["stats"][2] and got["stats"][6] == 0, (i, op[0])


# ---- 2. the claims of the sequences ------------------------------------------------------------------------------------

def kinds_of(ops):
    return {k: sum(op[0] == k for op in ops) for k in ("build", "insert", "remove", "replace", "resize")}


def ids_seen(ops):
    """how many clouds of the sequence are empty, have the id -1, and have an id behind the poses"""
    empty = skipped = past = 0
    for kind, a in ops:
        if kind == "resize":
            continue
        p, o, T, ids = S.four(a["part"])
        empty += int((np.diff(o) == 0).sum())
        if ids is not None:
            skipped += int((ids == -1).sum())
            past += int((ids >= len(T)).sum())
    return empty, skipped, past


@pytest.mark.parametrize("seed", S.WITHIN_SEEDS)
def test_within_capacity_sequences_are_what_they_claim(seed):
    max_voxels, ops = S.sequence(seed)
    P = S.pool(seed)
    assert 10 <= len(P["clouds"]) <= 16 and all(100 <= len(c) <= 300 for c in P["clouds"][:-2])
    assert P["clouds"][0].dtype == S.FORMATS[seed % 3][0] and P["clouds"][0].shape[1] == S.FORMATS[seed % 3][1]
    assert P["clouds"][0].shape[1] == 3 or np.isnan(P["clouds"][0][:, 3]).all()
    kinds = kinds_of(ops)
    assert len(ops) >= 12 and kinds == dict(build=1, insert=5, remove=5, replace=3, resize=3), kinds
    empty, skipped, past = ids_seen(ops)
    assert empty >= 4 and skipped >= 3 and past == 1
    m, steps = run(max_voxels, ops)
    assert max(a["capacity"] for _, _, a, _, _ in steps) <= 1024
    assert 100 <= max(a["stats"][0] for _, _, a, _, _ in steps) <= 512                 # a few hundred voxels
    revived = sum(len(f.get("revived", ())) for _, _, _, f, _ in steps)
    refilled = [f["refilled"] for op, _, _, f, _ in steps if op[0] == "replace"]
    assert revived >= 1 and refilled[0] >= 6 and all(r >= 0 for r in refilled)       # lone's six voxels, at the least
    # a replacement leaves a cloud alone: rows without a pose in both halves, none of them the map's
    for op, res, a, _, _ in steps:
        if op[0] == "replace" and S.four(op[1]["part"])[3] is not None:
            assert res["removed"][3] == res["placed"][5] > 0 and a["stats"][5] == steps[2][2]["stats"][5]
    dropped = [int(res["rehashed"][1]) for op, res, _, _, _ in steps if op[0] == "resize"]
    assert dropped[0] >= 6 and dropped[1] == 0 and dropped[2] >= 2                    # compacted, grown, compacted
    assert all((res["rehashed"][2:] == 0).all() for op, res, _, _, _ in steps if op[0] == "resize")
    # the small move keeps every row of lone in its voxel, one millimetre off the faces
    lone = (P["clouds"][P["lone"]], np.array([0, 120]), P["poses"][P["lone"]][None])
    there = (lone[0], lone[1], S.moved(lone[2], S.SMALL_SHIFT[None]))
    assert set(R.build_dist(*lone)["keys"].tolist()) == set(R.build_dist(*there)["keys"].tolist())


@pytest.mark.parametrize("seed", S.PAST_SEEDS)
def test_past_capacity_sequences_are_what_they_claim(seed):
    max_voxels, ops = S.sequence(seed)
    kinds = kinds_of(ops)
    assert len(ops) >= 12 and kinds == dict(build=1, insert=7, remove=6, replace=1, resize=3), kinds
    m, steps = run(max_voxels, ops)
    for i, (op, res, a, f, cap) in enumerate(steps):
        assert a["stats"][0] <= 2 * cap <= 2048 and a["stats"][6] == 0, (i, op[0])    # every key finds a slot
        assert a["stats"][1] == min(a["stats"][0], cap), (i, op[0])
    # most voxels with a place hold the integers of the build over the clouds the model holds: their records can be compared
    md = S.Model(max_voxels)
    for i, op in enumerate(ops):
        md.apply(op)
        a, n = md.arrays(), md.stats()[1]
        got = {k: v[:2] for k, v in PR.mapping({x: a[x][:n] for x in ("keys", "info", "moments", "voxels")}).items()}
        want = PR.mapping(R.build_dist(*md.remaining(), max_voxels=4096))
        same = sum(k in want and got[k] == want[k][:2] for k in got)
        assert same >= S.PAST_SHARE * sum(v[0] > 0 for v in got.values()) > 0 and len(want) <= 4096, (i, op[0], same)
    found = [a["stats"][0] for _, _, a, _, _ in steps]
    caps = [cap for *_, cap in steps]
    assert found[0] <= caps[0] < found[1] < found[2] == found[1] + 2                  # an insertion overflows; tiny into full outputs
    assert steps[3][1]["removed"] == [0, 0, 0, 0, 8, 0, 0, 0]                        # tiny: every row missing
    assert steps[4][1]["removed"][MISSING] > 0 < steps[4][1]["removed"][0]           # G1: its rows in unplaced voxels missing
    assert steps[5][1]["removed"][EMPTIED] == 6 and steps[5][3]["unmatched"] == 0
    assert steps[6][1]["removed"][5:] == [6, 0, 6] and steps[6][3]["unmatched"] == 1  # lone again: six inconsistent voxels
    grown = steps[7][1]["rehashed"].tolist()
    assert grown == [caps[0], 0, found[2] - caps[0], 6, 0, 0] and caps[7] > caps[0]   # they survive; the unplaced keys are lost
    a = steps[7][2]
    lone_places = [i for i in range(a["stats"][1]) if a["info"][i, 0] < 0 and not a["voxels"][i].any()]
    assert len(lone_places) == 6
    assert steps[8][2]["info"][lone_places, 0].tolist() == [0] * 6                    # one insertion: emptied
    P = S.pool(seed)
    alone = R.build_dist(P["clouds"][P["lone"]], np.array([0, 120]), P["poses"][P["lone"]][None])
    got, want = PR.mapping(steps[9][2]), PR.mapping(alone)
    assert all(got[k] == want[k] for k in want) and len(want) == 6                    # the second: restored
    assert steps[9][3]["revived"] == lone_places
    assert found[10] > found[9] == caps[0] and steps[11][1]["removed"][MISSING] == 0  # the lost voxels made again
    shrunk = steps[12][1]["rehashed"].tolist()
    assert shrunk[4] == found[11] - caps[12] > 0 and shrunk[5] == 0 and caps[12] < found[11]
    assert found[13] > found[12] and steps[13][2]["stats"][1] == caps[12]            # new keys into a full map with lost places
    back = steps[15][1]["rehashed"].tolist()
    assert back[2] == found[14] - caps[12] > 0 and back[0] + back[1] == caps[12]     # they stay lost
    assert steps[15][2]["stats"][2:].tolist() == steps[14][2]["stats"][2:].tolist()
    assert not m.inconsistent()


def test_some_past_capacity_removal_meets_voxels_that_lost_their_place():
    missing = [run(*S.sequence(seed))[1][14][1]["removed"][MISSING] for seed in S.PAST_SEEDS]
    assert sum(n > 0 for n in missing) >= 2, missing


# ---- 3. the named chains -----------------------------------------------------------------------------------------------

def test_chain_revival():
    cap, ops, vox = S.chain_revival()
    A, B, _ = IK.twelve_voxels()
    m, steps = run(cap, ops)
    a = steps[1][2]
    assert steps[1][1]["removed"] == [49, 0, 0, 0, 0, 7, 7, 0] and a["stats"].tolist() == [7, 7, 0, 0, 0, 0, 0]
    assert a["info"].tolist() == [[0, i, 0, 0] for i in range(7)] and not a["voxels"].any()
    a = steps[2][2]
    assert steps[2][3]["revived"] == [4, 5, 6] and places(a, vox) == list(range(12))
    # the revived voxels keep place and first row; their bounds are those of A's cloud 0 and B's cloud 1 together
    assert a["info"].tolist() == [[0, i, 0, 0] for i in range(4)] + [[7, i, 0, 1] for i in (4, 5, 6)] + \
        [[7, 49 + 3 + j, 1, 2] for j in range(5)]
    assert a["stats"].tolist() == [12, 12, 56, 0, 0, 0, 0] and a["cursor"] == [105, 3]
    alone = PR.mapping(R.build_dist(*B))
    got = PR.mapping(a)
    assert len(alone) == 8 and all(got[k] == alone[k] for k in alone)                  # the record is made again
    assert all(got[IK.voxel_key(v)] == PR.EMPTIED for v in vox[:4])
    a = steps[3][2]
    assert steps[3][1]["removed"] == [56, 0, 0, 0, 0, 8, 8, 0] and (a["info"][:, 0] == 0).all()
    assert a["info"][:, 1:].tolist() == steps[2][2]["info"][:, 1:].tolist() and not a["voxels"].any()
    # revived once more under a cloud number below the bounds: the lower bound moves, place, first row and upper bound stay
    res, a = steps[4][1], steps[4][2]
    assert res["removed"] == [0, 0, 0, 0, 28, 0, 0, 0] and res["placed"] == [0, 12, 28, 0, 0, 0, 0]
    assert steps[4][3]["revived"] == [7, 8, 9, 10, 11] and a["cursor"] == [105, 3]
    assert a["info"][7:].tolist() == [[4, 52, 0, 2]] + [[6, 53 + j, 0, 2] for j in range(4)]
    assert a["info"][:7].tolist() == steps[3][2]["info"][:7].tolist() and a["stats"].tolist() == [12, 12, 28, 0, 0, 0, 0]


def test_chain_refill():
    cap, ops, vox = S.chain_refill()
    m, steps = run(cap, ops)
    res, a, f = steps[1][1], steps[1][2], steps[1][3]
    assert res["removed"] == [56, 0, 0, 0, 0, 8, 5, 0] and res["placed"] == [5, 17, 56, 0, 0, 0, 0]
    assert f["refilled"] == 5 and not m.emptied()                                     # five emptied, none at the end
    assert a["info"][:12].tolist() == [[7, i, 0, 0] for i in range(4)] + [[14, i, 0, 1] for i in (4, 5, 6)] + \
        [[3, 52, 1, 2]] + [[1, 53 + j, 1, 2] for j in range(4)]
    assert a["info"][12:].tolist() == [[4, 77, 2, 2]] + [[6, 81 + 6 * j, 2, 2] for j in range(4)]    # B1, one voxel on
    assert [a["place"][IK.voxel_key(v + [1, 0, 0])] for v in vox[7:]] == [12, 13, 14, 15, 16]
    assert a["stats"].tolist() == [17, 17, 105, 0, 0, 0, 0] and a["cursor"] == [105, 3]
    assert PR.assert_follows(a, m.rebuild()) == 0


def test_chain_numbered_below():
    cap, ops, vox = S.chain_numbered_below()
    m, steps = run(cap, ops)
    first = steps[3][1]
    assert first["rehashed"].tolist() == [8, 4, 0, 0, 0, 0] and first["new_place"].tolist() == [-1] * 4 + list(range(8)) + [-1] * 4
    assert steps[3][2]["info"][:, 1].tolist() == list(range(28, 36))                  # every first row is 28 or more
    res, a = steps[4][1], steps[4][2]
    assert res["removed"] == [28, 0, 0, 0, 0, 5, 0, 0] and res["placed"] == [5, 13, 28, 0, 0, 0, 0]
    assert a["info"][8:].tolist() == [[4, 0, 0, 0], [6, 4, 0, 0], [6, 10, 0, 0], [6, 16, 0, 0], [6, 22, 0, 0]]
    assert [a["place"][IK.voxel_key(v + [1, 0, 0])] for v in vox[7:]] == [8, 9, 10, 11, 12]    # the places at the end
    assert (np.diff(a["info"][:, 1]) < 0).any() and a["cursor"] == [84, 3]            # ascending first rows no longer hold
    assert steps[5][1]["removed"] == [28, 0, 0, 0, 0, 8, 8, 0]
    last = steps[6][1]
    assert last["rehashed"].tolist() == [5, 8, 0, 0, 0, 0]
    assert last["new_place"].tolist() == [-1] * 8 + [0, 1, 2, 3, 4] + [-1] * 3        # strictly increasing on the kept places
    assert steps[6][2]["info"].tolist() == a["info"][8:].tolist() and PR.assert_follows(steps[6][2], m.rebuild()) == 0


def test_chain_overflow():
    cap, ops, vox = S.chain_overflow()
    m, steps = run(cap, ops)
    built = steps[0][2]
    assert built["stats"].tolist() == [12, 8, 105, 0, 0, 0, 0] and places(built, vox) == list(range(8)) + [-1] * 4
    assert steps[1][1]["removed"] == [0, 0, 0, 0, 28, 0, 0, 0]                        # all rows missing
    for k in ("keys", "info", "stats"):
        assert np.array_equal(steps[1][2][k][:8], built[k][:8]), k
    assert steps[1][2]["voxels"][:8].tobytes() == built["voxels"][:8].tobytes()
    assert steps[1][2]["moments"][:8].tolist() == built["moments"][:8].tolist()
    grown = steps[2][1]
    assert grown["rehashed"].tolist() == [8, 0, 4, 0, 0, 0] and places(steps[2][2], vox) == list(range(8)) + [None] * 4
    a = steps[3][2]
    assert a["stats"].tolist() == [12, 12, 133, 0, 0, 0, 0] and a["cursor"] == [133, 4]
    assert a["info"][8:].tolist() == [[7, 105 + j, 3, 3] for j in range(4)] and places(a, vox) == list(range(12))
    high = ops[3][1]["part"]
    alone, got = PR.mapping(R.build_dist(*high[:3])), PR.mapping(a)
    assert len(alone) == 4 and all(got[k] == alone[k] for k in alone)                 # these rows only


def test_chain_shrink():
    cap, ops, vox = S.chain_shrink()
    m, steps = run(cap, ops)
    res, a = steps[1][1], steps[1][2]
    assert res["rehashed"].tolist() == [12, 0, 0, 0, 4, 0] and res["new_place"].tolist() == list(range(8)) + [-1] * 8
    assert a["stats"].tolist() == [12, 8, 105, 0, 0, 0, 0] and places(a, vox) == list(range(8)) + [-1] * 4
    b = steps[2][2]                                                                   # voxel 2 takes its rows, voxel 9 and the new one none
    assert b["stats"].tolist() == [13, 8, 121, 0, 0, 0, 0] and b["cursor"] == [121, 6]
    assert b["info"][:8].tolist() == [[14, 2, 0, 3] if i == 2 else r for i, r in enumerate(a["info"][:8].tolist())]
    assert places(b, vox) == places(a, vox) and b["place"][IK.voxel_key([30, 30, 30])] >= 8
    assert steps[3][1]["removed"] == [0, 0, 0, 0, 7, 0, 0, 0]
    back = steps[4][1]
    assert back["rehashed"].tolist() == [8, 0, 5, 0, 0, 0]
    c = steps[4][2]
    assert places(c, vox) == list(range(8)) + [None] * 4 and IK.voxel_key([30, 30, 30]) not in c["place"]
    assert c["stats"].tolist() == [8, 8] + b["stats"][2:].tolist() and c["capacity"] == 16


# ---- 4. the round trip on the scene ------------------------------------------------------------------------------------

def test_scene_round_trip_ends_at_the_build_over_the_six_parts():
    cap, ops = S.scene_round_trip()
    m, steps = run(cap, ops)
    s = K.scene()
    whole = R.build_dist(s["points"], s["offsets"], s["poses"], max_voxels=16384)
    final = steps[-1][2]
    assert PR.assert_follows(final, whole, "round trip") == len(m.emptied()) > 0
    assert final["stats"][2:].tolist() == [24000, 0, 0, 0, 0] and final["cursor"] == [28000, 7] and final["capacity"] == 16384
    compacted = steps[4][1]
    n_dropped = int(compacted["rehashed"][1])
    assert n_dropped >= 1 and compacted["rehashed"].tolist()[2:] == [0, 0, 0, 0] and compacted["rehashed"][0] <= 6144
    kept = compacted["new_place"][compacted["new_place"] >= 0]
    assert kept.tolist() == list(range(int(compacted["rehashed"][0])))
    before = steps[3][2]
    gone = np.nonzero(compacted["new_place"][:before["stats"][1]] < 0)[0]
    assert len(gone) == n_dropped and (before["info"][gone, 0] == 0).all()            # which places exist after the compaction
    held = sorted((r.tobytes(), T.tobytes()) for r, T in m.held)
    assert held == sorted((s["points"][4000 * c:4000 * (c + 1)].tobytes(), s["poses"][c].tobytes()) for c in range(6))
    for i, (op, res, a, f, _) in enumerate(steps):
        assert a["stats"][0] <= a["capacity"] and a["stats"][3:].tolist() == [0, 0, 0, 0] and f.get("unmatched", 0) == 0, i


# ---- 5. the rows of the second sweep -----------------------------------------------------------------------------------

def test_wrap_sizes_are_the_kernels():
    from neural_spectral_codec_amd import _lib
    assert S.WRAP == _lib.MAP_INSERT_ROWS * _lib.MAP_INSERT_BLOCKS == 256 * 4096      # MAP_THREADS x MAP_SLOT_BLOCKS of nsc_map.hip
    assert S.WRAP_SIZES == (S.WRAP + 1, S.WRAP + 513)


@pytest.mark.parametrize("n", S.WRAP_SIZES)
def test_wrap_rows_and_their_vectorised_reference(n):
    rows = S.wrap_rows(n)
    ref = S.wrap_reference(n)
    assert rows[0].shape == (n, 3) and rows[1][-1] == n and (np.diff(rows[1]) == 0).sum() == 1
    assert ref["largest"] < 2 ** 50                                                   # no sum comes near 2^63
    small, ins = ref["small"], ref["inserted"]
    keys, _, _ = S.keys_and_integers(rows, small["grid"])
    head, tail = keys[:S.WRAP - 512], keys[n - S.WRAP_TAIL:]
    outside = len(set(small["keys"].tolist()) - set(head.tolist()))                   # small's voxels off the cube
    assert 0 < small["stats"][0] - outside and ins["stats"].tolist() == [4096 + 513 + outside] * 2 + [600 + n, 0, 0, 0, 0]
    assert ins["stats"][0] <= 8192
    assert ins["cursor"] == [600 + n, 6 + 5]
    # the first sweep reaches every voxel of the cube, many times; the last 513 rows make voxels of their own, in row order
    assert len(set(head.tolist())) == 4096 and np.bincount(np.unique(head, return_inverse=True)[1]).min() >= 255
    assert len(set(tail.tolist())) == S.WRAP_TAIL and not set(tail.tolist()) & set(keys[:n - S.WRAP_TAIL].tolist())
    at = [ins["place"][k] for k in tail.tolist()]
    assert at == list(range(4096 + outside, 4096 + outside + 513)) and ins["info"][at, 0].tolist() == [1] * 513
    assert ins["info"][at, 1].tolist() == list(range(600 + n - 513, 600 + n)) and n - 513 <= S.WRAP < n
    assert int(ins["info"][:, 0].sum()) == 600 + n
    # moved by one voxel along y: the line's voxels are new again, a face of the cube too
    mv = ref["moved"]
    assert mv["stats"][0] == small["stats"][0] + len(set(mv["keys"].tolist()) - set(small["keys"].tolist()))
    there = set(S.keys_and_integers((rows[0], rows[1], ref["new_poses"], None), small["grid"])[0][n - S.WRAP_TAIL:].tolist())
    assert len(there) == S.WRAP_TAIL and not there & set(ins["keys"].tolist())
    assert 513 + 200 < len(set(mv["keys"].tolist()) - set(ins["keys"].tolist())) <= 513 + 256
    # the vectorised reference is the per-row restatement on a prefix, by bits
    cut = 20_000
    prefix = (rows[0][:cut], np.minimum(rows[1], cut), rows[2], None)
    a, b = S.wrap_state(), S.wrap_state()
    IR.insert(a, *prefix)
    S.insert_vectorised(b, prefix)
    a, b = IR.arrays(a), IR.arrays(b)
    for k in ("keys", "info", "stats"):
        assert np.array_equal(a[k], b[k]), k
    assert a["moments"].tolist() == b["moments"].tolist() and a["voxels"].tobytes() == b["voxels"].tobytes()
    assert a["place"] == b["place"] and a["cursor"] == b["cursor"]
