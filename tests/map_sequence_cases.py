"""The kept map of include/nsc.h under sequences of calls: the restatements of tests/map_localize_restatement.py (build),
tests/map_insert_restatement.py, tests/map_replace_restatement.py and tests/map_rehash_restatement.py composed into one
model, and the inputs of tests/test_map_sequence_cpu.py and tests/test_map_sequence_gpu.py: seeded sequences, named chains
on the twelve voxels of tests/map_insert_cases.py, a round trip on the scene and rows for the second sweep of the row
passes.  The CPU file asserts what each case claims about itself; the GPU file relies on it.

A part is (points, offsets, poses, pose_ids or None).  An operation is (kind, arguments): ("build" | "insert" | "remove",
dict(part)), ("replace", dict(part, new, first_row, first_cloud)) with ``part`` under the old poses, or ("resize",
dict(max_voxels, compact))."""
import functools

import numpy as np

import map_insert_cases as IK
import map_insert_restatement as IR
import map_localize_cases as K
import map_localize_restatement as R
import map_rehash_restatement as HR
import map_replace_cases as PK
import map_replace_restatement as PR
import map_restatement as M

FORMATS = [(np.float32, 3), (np.float32, 4), (np.float64, 3)]
WITHIN_SEEDS = tuple(range(8))
PAST_SEEDS = tuple(range(100, 104))
TOUCHED, EMPTIED, INCONSISTENT, MISSING = 5, 6, 7, 4          # entries of ``removed``
SMALL_SHIFT = np.array([5e-4, -5e-4, 5e-4])                  # half the rows' distance from the faces: every row keeps its voxel
PAST_SHARE = 0.8             # of the voxels with rows in a past-capacity sequence, those a rebuild over ``held`` gives the integers of
WRAP = 512 * 2048                                            # rows of one sweep of every row pass (asserted against _lib)
WRAP_SIZES = (WRAP + 1, WRAP + 513)
WRAP_TAIL = 513                                              # the last rows of wrap_rows, each alone in a voxel


def four(part):
    return part if len(part) == 4 else tuple(part) + (None,)


def clouds_of(part, poses=None):
    """the (rows, pose) pairs of the clouds of a part that have a pose, under ``poses`` if given"""
    p, o, T, ids = four(part)
    T = np.asarray(T if poses is None else poses, np.float64)
    for c in range(len(o) - 1):
        i = c if ids is None else int(ids[c])
        if 0 <= i < len(T):
            yield np.asarray(p)[int(o[c]):int(o[c + 1])], T[i]


def state_of(out, old):
    """the destination of map_rehash_restatement.rehash -> a state of map_insert_restatement, grid and rule from ``old``.
    Every number is one of ``out``: the first stats[1] keys, info rows, moments (as Python integers) and records, the stats,
    the cursor and the mapping key -> place.  The source's keys without a place are not in ``out`` and are lost.  A kept key
    that found no place in the destination stays keyed: it stands behind the written ones with an empty row nothing
    compares, as a voxel past the outputs of a build does, so that found stays the number of keys"""
    assert out["place"] is not None, "more voxels kept than slots: there is no reference"
    n, N = int(out["stats"][1]), len(out["info"])
    s = dict(grid=old["grid"], capacity=N, rule=old["rule"], keys=out["keys"][:n].tolist(), info=out["info"][:n].tolist(),
             moments=[[int(v) for v in row] for row in out["moments"][:n]], voxels=[r.copy() for r in out["voxels"][:n]],
             stats=[int(v) for v in out["stats"]], cursor=[int(v) for v in out["cursor"]], place={})
    for key, q in out["place"].items():
        if q >= 0:
            s["place"][key] = q
            continue
        s["place"][key] = len(s["keys"])
        s["keys"].append(key)
        s["info"].append([0, 0, IR.BIG, -1])
        s["moments"].append([0] * 9)
        s["voxels"].append(np.zeros(16))
    assert len(s["keys"]) == s["stats"][0] and all(s["keys"][q] == key for key, q in s["place"].items())
    return s


class Model:
    """one state of the restatements under build, insert, remove, replace and resize; each call returns what the device
    call returns beside the kept tensors.  ``held`` is the multiset of (rows, pose) the map holds; ``facts`` of the last
    call: places revived (emptied before an insertion, holding rows after it) and refilled (emptied by a replacement's
    removal half, filled by its insertion half)"""

    def __init__(self, max_voxels, **rule):
        self.max_voxels, self.rule, self.s, self.held, self.facts = int(max_voxels), rule, None, [], {}

    def build(self, part):
        p, o, T, ids = four(part)
        m = R.build_dist(p, o, T, ids, max_voxels=self.max_voxels, **self.rule)
        self.s = IR.start(m, len(p), len(o) - 1, **self.rule)
        self.held, self.facts, self.empty = list(clouds_of(part)), {}, np.asarray(p)[:0]
        return {}

    def arrays(self):
        return IR.arrays(self.s)

    def stats(self):
        return list(self.s["stats"])

    def emptied(self):
        """the places below stats[1] that hold an emptied voxel"""
        s = self.s
        return {i for i in range(s["stats"][1]) if s["info"][i][0] == 0 and not any(s["moments"][i])}

    def inconsistent(self):
        s = self.s
        return {i for i in range(s["stats"][1]) if s["info"][i][0] < 0 or (s["info"][i][0] == 0 and any(s["moments"][i]))}

    def _take(self, rows, pose):
        for i, (r, T) in enumerate(self.held):
            if r.shape == rows.shape and r.tobytes() == rows.tobytes() and T.tobytes() == pose.tobytes():
                del self.held[i]
                return True
        return False

    def insert(self, part):
        before = self.emptied()
        touched = IR.insert(self.s, *four(part))
        self.held += list(clouds_of(part))
        self.facts = dict(revived=sorted(before - self.emptied()), touched=touched)
        return {}

    def remove(self, part):
        counts = PR.remove(self.s, *four(part))[0]
        self.facts = dict(unmatched=sum(not self._take(r, T) for r, T in clouds_of(part)))
        return dict(removed=counts)

    def replace(self, part, new, first_row=0, first_cloud=0):
        p, o, T, ids = four(part)
        before = self.emptied()
        counts, placed = PR.replace(self.s, p, o, T, new, ids, first_row, first_cloud)
        unmatched = sum(not self._take(r, T) for r, T in clouds_of(part))
        self.held += list(clouds_of(part, new))
        after = self.emptied()
        self.facts = dict(unmatched=unmatched, refilled=counts[EMPTIED] - len(after - before), revived=sorted(before - after))
        return dict(removed=counts, placed=placed)

    def resize(self, max_voxels=None, compact=True):
        """-> map_rehash_restatement.rehash's whole destination (the typed outputs rehashed, new_place and tile_base
        among it)"""
        N = self.max_voxels if max_voxels is None else int(max_voxels)
        out = HR.rehash(HR.as_kept(self.arrays()), not compact, N)
        self.s, self.max_voxels, self.facts = state_of(out, self.s), N, {}
        return out

    def apply(self, op):
        kind, a = op
        return getattr(self, kind)(**a)

    def remaining(self):
        """the clouds the map holds, packed for a rebuild -> (points, offsets, poses)"""
        if not self.held:
            return self.empty, np.zeros(1, np.int64), np.zeros((0, 4, 4))
        pts, off = IK.pack([r for r, _ in self.held])
        return pts, off, np.stack([T for _, T in self.held])

    def rebuild(self):
        return R.build_dist(*self.remaining(), max_voxels=self.max_voxels, **self.rule)


def n_voxels(part):
    p, o, T, ids = four(part)
    return len(M.build_map(p, o, T, ids, voxel_size=1.0)["keys"])


def moved(poses, shifts):
    """the poses with shifts[c] added to the translation of pose c"""
    out = np.array(poses, np.float64)
    out[:, :3, 3] += np.asarray(shifts, np.float64)
    return out


# ---- seeded sequences -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pool(seed):
    """clouds made like IK.general_split: general poses, every row 1e-3 voxel off the faces.  ``n`` regular clouds of 200
    to 300 rows, each in 36 voxels of a band of x, then ``lone`` (120 rows in six voxels no other cloud reaches) and
    ``tiny`` and ``extra`` (8 rows each, in two voxels of their own): ten to sixteen clouds.  The format follows the seed.  row0[c] is the first
    row of cloud c in the pool's own packing, the numbering a store would give"""
    rng = np.random.default_rng(7000 + seed)
    dtype, cols = FORMATS[seed % 3]
    n = 7 + seed % 7
    clouds, poses = [], []

    def add(lo, hi, rows):
        i = len(clouds)
        T = K.general_pose(0.4 * i - 1.2 + 0.05 * (seed % 10), 0.01 * i - 0.03, [1.1 * i - 3.0, 0.7 * i - 2.0, 0.1 * i], roll=0.02)
        world = rng.integers(lo, hi, (rows, 3)) + rng.uniform(1e-3, 1.0 - 1e-3, (rows, 3))
        sensor = ((world - T[:3, 3]) @ T[:3, :3]).astype(dtype)
        clouds.append(sensor if cols == 3 else np.concatenate([sensor, np.full((rows, 1), np.nan, dtype)], 1))
        poses.append(T)
    for _ in range(n):
        x = int(rng.integers(-7, 5))
        add([x, -3, -1], [x + 3, 3, 1], int(rng.integers(200, 301)))
    add([12, -2, 0], [14, 1, 1], 120)
    add([20, 5, 3], [22, 6, 4], 8)
    add([30, -8, 5], [32, -7, 6], 8)
    row0 = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    return dict(clouds=clouds, poses=np.stack(poses), n=n, lone=n, tiny=n + 1, extra=n + 2, row0=row0, format=(dtype, cols))


def part(P, which, skip=(), past=()):
    """the clouds ``which`` of a pool (None: a cloud of no rows) under their poses; the clouds at the positions ``skip``
    get the pose id -1 and those at ``past`` an id behind the poses -> (points, offsets, poses, ids, or None for neither)"""
    pts, off = IK.pack([P["clouds"][0][:0] if i is None else P["clouds"][i] for i in which])
    T = np.stack([np.eye(4) if i is None else P["poses"][i] for i in which])
    ids = None
    if len(skip) or len(past):
        ids = np.arange(len(which), dtype=np.int64)
        ids[list(skip)] = -1
        ids[list(past)] = len(which) + 3
    return pts, off, T, ids


def _replacement(P, which, shifts, skip=()):
    """the clouds ``which`` moved by shifts[c], numbered as the pool numbers the first of them"""
    p = part(P, which, skip=skip)
    return ("replace", dict(part=p, new=moved(p[2], shifts), first_row=int(P["row0"][which[0]]), first_cloud=int(which[0])))


def _back(op):
    """the replacement that undoes ``op``"""
    a = op[1]
    p, o, T, ids = a["part"]
    return ("replace", dict(part=(p, o, a["new"], ids), new=T, first_row=a["first_row"], first_cloud=a["first_cloud"]))


class _Recorder:
    """runs the model beside a list of operations, so that a sequence can size its capacities by what the map holds"""

    def __init__(self, max_voxels):
        self.model, self.ops = Model(max_voxels), []

    def __call__(self, kind, **a):
        self.ops.append((kind, a))
        return self.model.apply(self.ops[-1])

    def found(self):
        return self.model.s["stats"][0]


def _within(seed):
    P = pool(seed)
    rng = np.random.default_rng(seed)
    n, lone, tiny = P["n"], P["lone"], P["tiny"]
    a, b = 3 + seed % 2, 5 + seed % 2
    G0, G1, G2 = list(range(a)), list(range(a, b)), list(range(b, n))
    big = lambda k: rng.uniform(-0.45, 0.45, (k, 3))
    do = _Recorder(512)
    do("build", part=part(P, G0 + [None, lone, tiny], skip=[a + 2]))                 # tiny has no pose here
    do("insert", part=part(P, G1 + [None], past=[len(G1) - 1]))                       # the last of G1 neither
    do("insert", part=part(P, G2 + [G1[-1], tiny]))
    # G1 re-placed, its first cloud left alone; lone moves inside its voxels: all of them emptied and filled again
    there = _replacement(P, G1 + [lone], np.concatenate([big(len(G1)), SMALL_SHIFT[None]]), skip=[0])
    do(*there[:1], **there[1])
    do("remove", part=part(P, G0 + [None]))
    do("insert", part=part(P, G0))                                                   # G0's own voxels revived
    lone_there = (P["clouds"][lone], np.array([0, 120]), moved(P["poses"][lone:lone + 1], SMALL_SHIFT[None]), None)
    do("remove", part=lone_there)
    do("remove", part=part(P, G2[:1]))
    kept = do.found() - len(do.model.emptied())
    do("resize", max_voxels=kept + 80 + seed, compact=True)
    do("insert", part=part(P, [lone, None, G2[0]]))                                  # new voxels behind a compacted map
    back = _back(there)
    p, o, T, ids = back[1]["part"]
    back[1]["part"] = (p, o, T, np.where(np.arange(len(o) - 1) == len(G1), -1, ids))  # lone was removed: it stays out
    do(*back[:1], **back[1])
    do("resize", max_voxels=700 + seed, compact=False)
    there = _replacement(P, G2, big(len(G2)), skip=[len(G2) - 1] if len(G2) > 1 else [])
    do(*there[:1], **there[1])
    do("remove", part=part(P, [tiny, None]))
    do("remove", part=part(P, G1[-1:]))
    kept = do.found() - len(do.model.emptied())
    do("resize", max_voxels=kept + 45, compact=True)
    do("insert", part=part(P, [tiny, G1[-1]], skip=[0] if seed % 2 else []))
    return 512, do.ops


def _past(seed):
    P = pool(seed)
    rng = np.random.default_rng(seed)
    n, lone, tiny = P["n"], P["lone"], P["tiny"]
    G0, G1, G2 = [0, 1, 2, 3], [4, 5, 6], list(range(7, n))
    V01 = n_voxels(part(P, [lone] + G0 + G1))
    # the build fits and G1 overflows, so that G1 alone has rows the map never took; tiny's two voxels still find slots
    M0 = max(n_voxels(part(P, [lone] + G0)), (V01 + 2) // 2 + 1)
    assert M0 < V01
    do = _Recorder(M0)
    do("build", part=part(P, [lone] + G0 + [None]))
    do("insert", part=part(P, G1))                                                   # overflows: keys with place ~0
    do("insert", part=part(P, [tiny, None]))                                         # new keys into full outputs
    do("remove", part=part(P, [tiny]))                                               # every row missing
    do("remove", part=part(P, G1))                                                   # the rows of unplaced voxels missing
    do("remove", part=part(P, [lone]))
    do("remove", part=part(P, [lone]))                                               # unmatched: six inconsistent voxels
    do("resize", max_voxels=2 * V01, compact=True)                                   # the unplaced keys are lost
    do("insert", part=part(P, [lone]))
    do("insert", part=part(P, [lone]))                                               # restored
    do("insert", part=part(P, [tiny] + G1))                                          # the lost voxels made again
    there = _replacement(P, G0[1:3], rng.uniform(-0.45, 0.45, (2, 3)))
    do(*there[:1], **there[1])
    kept, nxt = do.found(), part(P, G2[:1] + [None, P["extra"]])
    N = max(-(-3 * kept // 5), (kept + n_voxels(nxt)) // 2 + 1)
    assert N < kept
    do("resize", max_voxels=N, compact=False)                                        # fewer places than kept voxels
    do("insert", part=nxt)                                                           # into a full map that holds keys with ~0
    do("remove", part=part(P, G1[1:2]))                                              # partly in voxels that lost their place
    do("resize", max_voxels=2 * do.found(), compact=True)                            # they stay lost
    do("insert", part=part(P, G1[1:2]))
    do("remove", part=part(P, [tiny]))
    return M0, do.ops


@functools.lru_cache(maxsize=None)
def sequence(seed):
    """the operations of a seed, the first of them the build -> (max_voxels of the build, the list)"""
    return (_within if seed in WITHIN_SEEDS else _past)(seed)


# ---- named chains on IK.twelve_voxels ----------------------------------------------------------------------------------
# A (49 rows, one cloud) has seven rows in each of the voxels 0 .. 6, row i < 7 in voxel i.  B (56 rows) has seven rows in
# each of the voxels 4 .. 11, row j < 8 in voxel 4 + j; its first cloud B0 (28 rows) has one row in each of them, six more
# in the voxels 4, 5 and 6 and two more in voxel 7; its second cloud B1 four rows in voxel 7 and six in each of 8 .. 11.

def rows_in(cloud, vox, which):
    """the rows of a part of IK.twelve_voxels (identity poses) that lie in the voxels ``which``, as a part of one cloud"""
    p = cloud[0]
    sel = (np.floor(p)[:, None, :] == vox[None, list(which), :]).all(2).any(1)
    return p[sel], np.array([0, int(sel.sum())], np.int64), np.eye(4)[None], None


def halves(B):
    """B of IK.twelve_voxels as its two clouds -> (B0, B1)"""
    p, o, T = B
    h = int(o[1])
    return (p[:h], np.array([0, h], np.int64), T[:1], None), (p[h:], np.array([0, len(p) - h], np.int64), T[1:], None)


X1 = np.array([[1.0, 0.0, 0.0]])                # one voxel along x: voxel i of twelve_voxels moves to a voxel none of them is


def chain_revival():
    """build A at 16; remove A; insert B; remove B; replace B1 from one voxel along x, where the map holds nothing, to
    where it was, numbered from row 0 and cloud 0: below the bounds its voxels keep"""
    A, B, vox = IK.twelve_voxels()
    B1 = halves(B)[1]
    return 16, [("build", dict(part=A + (None,))), ("remove", dict(part=A + (None,))), ("insert", dict(part=B + (None,))),
                ("remove", dict(part=B + (None,))),
                ("replace", dict(part=B1[:2] + (moved(B1[2], X1), None), new=B1[2], first_row=0, first_cloud=0))], vox


def chain_refill():
    """build A and B at 32; replace B with B0 where it is and B1 one voxel along x"""
    A, B, vox = IK.twelve_voxels()
    AB = IK.pack([A[0], B[0][:28], B[0][28:]]) + (np.tile(np.eye(4), (3, 1, 1)), None)
    new = moved(B[2], np.array([[0.0, 0.0, 0.0], X1[0]]))
    return 32, [("build", dict(part=AB)), ("replace", dict(part=B + (None,), new=new, first_row=49, first_cloud=1))], vox


def chain_numbered_below():
    """build the rows of A in the voxels 0 .. 3 at 16; insert B; remove the first; compact; replace B1 one voxel along x,
    numbered from row 0 and cloud 0; remove B0; compact"""
    A, B, vox = IK.twelve_voxels()
    low, (B0, B1) = rows_in(A, vox, range(4)), halves(B)
    return 16, [("build", dict(part=low)), ("insert", dict(part=B + (None,))), ("remove", dict(part=low)),
                ("resize", dict(max_voxels=16, compact=True)),
                ("replace", dict(part=B1, new=moved(B1[2], X1), first_row=0, first_cloud=0)),
                ("remove", dict(part=B0)), ("resize", dict(max_voxels=16, compact=True))], vox


def chain_overflow():
    """build A and B at 8; remove B's rows in the voxels 8 .. 11; grow to 16; insert them again"""
    A, B, vox = IK.twelve_voxels()
    AB = IK.pack([A[0], B[0][:28], B[0][28:]]) + (np.tile(np.eye(4), (3, 1, 1)), None)
    high = rows_in(B, vox, range(8, 12))
    return 8, [("build", dict(part=AB)), ("remove", dict(part=high)), ("resize", dict(max_voxels=16, compact=True)),
               ("insert", dict(part=high))], vox


def chain_shrink():
    """build A and B at 16; compact to 8; insert rows of the voxels 2 and 9 and of a new voxel; remove B's rows in voxel 9;
    grow to 16"""
    A, B, vox = IK.twelve_voxels()
    AB = IK.pack([A[0], B[0][:28], B[0][28:]]) + (np.tile(np.eye(4), (3, 1, 1)), None)
    two, nine = rows_in(A, vox, [2]), rows_in(B, vox, [9])
    new = (np.array([30, 30, 30]) * 64 + np.array([[3, 5, 7], [9, 11, 13]])) / 64.0
    mixed = IK.pack([two[0], nine[0], new]) + (np.tile(np.eye(4), (3, 1, 1)), None)
    return 16, [("build", dict(part=AB)), ("resize", dict(max_voxels=8, compact=True)), ("insert", dict(part=mixed)),
                ("remove", dict(part=nine)), ("resize", dict(max_voxels=16, compact=True))], vox


CHAINS = dict(revival=chain_revival, refill=chain_refill, numbered_below=chain_numbered_below, overflow=chain_overflow,
              shrink=chain_shrink)


# ---- the round trip on the scene ---------------------------------------------------------------------------------------

def scene_part(a, b):
    s = K.scene()
    return s["points"][4000 * a:4000 * b], s["offsets"][a:b + 1] - 4000 * a, s["poses"][a:b], None


def scene_round_trip():
    """build parts 0-2, insert 3-5, replace 1-2 to perturbed poses, remove 4, compact, replace 1-2 back, insert 4, grow
    -> (max_voxels of the build, the operations): the map then holds the six parts under their first poses"""
    p12 = scene_part(1, 3)
    new = p12[2].copy()
    new[:, :3, :3] = K.general_pose(PK.SCENE_TURN, 0.0, [0.0, 0.0, 0.0])[:3, :3] @ new[:, :3, :3]
    new[:, :3, 3] += PK.SCENE_SHIFT
    there = ("replace", dict(part=p12, new=new, first_row=4000, first_cloud=1))
    return 8192, [("build", dict(part=scene_part(0, 3))), ("insert", dict(part=scene_part(3, 6))), there,
                  ("remove", dict(part=scene_part(4, 5))), ("resize", dict(max_voxels=6144, compact=True)), _back(there),
                  ("insert", dict(part=scene_part(4, 5))), ("resize", dict(max_voxels=16384, compact=False))]


# ---- rows for the second sweep of the row passes -----------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def wrap_rows(n):
    """n lattice rows of 1 m voxels in five clouds (one of them empty) under rot90 poses: row r < n - WRAP_TAIL lies in
    voxel r % 4096 of a cube of 16^3 voxels, so the first sweep fills every one of them; each of the last WRAP_TAIL rows
    lies alone in a voxel of a line no other row reaches -> (points, offsets, poses, None), float64 and exact"""
    rng = np.random.default_rng(n)
    head = n - WRAP_TAIL
    i = np.arange(head) % 4096
    vox = np.concatenate([np.stack([i % 16, (i // 16) % 16, i // 256], 1) - 8,
                          np.stack([np.arange(WRAP_TAIL) + 40, np.full(WRAP_TAIL, 3), np.full(WRAP_TAIL, -2)], 1)])
    world = (vox * 64 + rng.integers(1, 64, (n, 3))) / 64.0
    off = np.array([0, 300_001, 300_001, 777_777, WRAP - 255, n], np.int64)
    poses = np.stack([K.rot90_pose(rng, 1.0) for _ in range(5)])
    pts = np.empty((n, 3))
    for c in range(5):
        a, b = off[c], off[c + 1]
        pts[a:b] = (world[a:b] - poses[c][:3, 3]) @ poses[c][:3, :3]      # R^T (w - t): exact under a rot90 pose
    return pts, off, poses, None


def wrap_small():
    """the small map the wrap rows are inserted into: K.exact_case of 600 rows, partly inside the cube"""
    return K.exact_case(90, 600) + (None,)


def keys_and_integers(part, grid):
    """-> keys (N,) int64, q (N,3) int64 and the cloud (N,) of every row of a part whose rows are all used"""
    p, o, T, ids = four(part)
    w, cloud, has_pose = M.world_rows(p, o, T, ids)
    k, q = R.inside_voxel(w, *grid)
    ki = (k + float(1 << 20)).astype(np.int64)
    assert has_pose.all() and np.isfinite(w).all() and ((ki >= 0) & (ki < (1 << M.KEY_BITS))).all()
    return ki[:, 0] | (ki[:, 1] << M.KEY_BITS) | (ki[:, 2] << (2 * M.KEY_BITS)), q.astype(np.int64), cloud


def insert_vectorised(s, part):
    """map_insert_restatement.insert for a part whose rows are all used, without the loop over rows: the rows are grouped
    by key with np.unique, counts and the nine moments summed with np.add.at in int64, new keys placed in the order of their
    first rows; the record of every voxel reached is map_localize_restatement.record -> the largest |sum| it formed"""
    keys, q, cloud = keys_and_integers(part, s["grid"])
    uniq, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    nine = np.concatenate([q, np.stack([q[:, a] * q[:, b] for a, b in PR.PAIRS], 1)], 1)
    sums = np.zeros((len(uniq), 9), np.int64)
    np.add.at(sums, inverse, nine)
    count = np.bincount(inverse, minlength=len(uniq))
    lo, hi = np.full(len(uniq), IR.BIG), np.full(len(uniq), -1, np.int64)
    np.minimum.at(lo, inverse, cloud)
    np.maximum.at(hi, inverse, cloud)
    row0, cloud0 = s["cursor"]
    for g in np.argsort(first, kind="stable").tolist():           # new voxels in the order of their first rows
        key = int(uniq[g])
        at = s["place"].get(key)
        if at is None:
            at = s["place"][key] = len(s["keys"])
            s["keys"].append(key)
            s["info"].append([0, row0 + int(first[g]), IR.BIG, -1])
            s["moments"].append([0] * 9)
            s["voxels"].append(None)
        info = s["info"][at]
        info[0] += int(count[g])
        info[2], info[3] = min(info[2], cloud0 + int(lo[g])), max(info[3], cloud0 + int(hi[g]))
        s["moments"][at] = [a + int(b) for a, b in zip(s["moments"][at], sums[g])]
        s["voxels"][at] = R.record(s["moments"][at], info[0], IR.key_voxel(key), *s["grid"], *s["rule"])
    st = s["stats"]
    st[0] = len(s["keys"])
    st[1] = min(st[0], s["capacity"])
    st[2] += len(keys)
    s["cursor"] = [row0 + len(keys), cloud0 + len(part[1]) - 1]
    return int(np.abs(sums).max(initial=0))


def wrap_state(max_voxels=8192):
    """the restated small build as a state"""
    p, o, T, _ = wrap_small()
    return IR.start(R.build_dist(p, o, T, max_voxels=max_voxels), len(p), len(o) - 1)


WRAP_MOVE = np.array([0.0, 1.0, 0.0])            # one voxel along y: the cube onto itself but for a face, the line onto new voxels


@functools.lru_cache(maxsize=2)
def wrap_reference(n):
    """-> dict: ``small`` (the small build), ``inserted`` (wrap_rows(n) inserted into it) and ``moved`` (the same rows
    inserted under their poses moved by WRAP_MOVE instead), as map_insert_restatement.arrays; ``largest`` |sum| formed"""
    rows = wrap_rows(n)
    there = rows[:2] + (PK.shifted(rows[2], WRAP_MOVE), None)
    s, t = wrap_state(), wrap_state()
    largest = max(insert_vectorised(s, rows), insert_vectorised(t, there))
    return dict(small=IR.arrays(wrap_state()), inserted=IR.arrays(s), moved=IR.arrays(t), largest=largest, new_poses=there[2])
