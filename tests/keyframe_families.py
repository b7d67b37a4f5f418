"""Constructed inputs for the five kernels of csrc/nsc_keyframe.hip, and the table that names the branch each one takes.

Dense random inputs leave the interesting branches of that file untaken, or taken without the result depending on them:
``rand()**4`` rows have the same float32 sum under most summation orders, no two quantised maxima are ever equal, no
product lands on k + 1/2, no two voxels of a few thousand share a slot of the 16 384-slot hash set.  The inputs here are
built value by value (histogram rows, records), pose by pose (chain graphs) and voxel by voxel (clouds), all seeded.

Histogram rows are non-negative and finite: the reference's ``astype(np.uint16)`` is undefined for NaN and wraps for
negative values, so those are outside the contract.  Voxel sizes are >= 0.001 (below ~4.7e-4 the clipped quotient passes
2^31).

No GPU and no product kernels in this module: tests/test_keyframe_families_cpu.py admits the families against numpy and
the oracle, tests/test_keyframe_paths_gpu.py runs them on the device.
"""
import functools
import os
import re
from collections import namedtuple

import numpy as np

import keyframe_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "neural-spectral-codec_amd", "csrc", "nsc_keyframe.hip")
EPS32 = np.float32(1e-8)
MAX_U16 = 65535
F32 = np.float32


# ----------------------------------------------------------------------------------------------------------------------
# the constants of the .hip text
# ----------------------------------------------------------------------------------------------------------------------
def parse_constants(src):
    def one(pat):
        m = re.search(pat, src)
        assert m, pat
        return m
    out = {k: int(one(r"constexpr int %s = (\d+);" % k).group(1))
           for k in ("PW_MAX_LEAVES", "PW_MAX_DIM", "VOX_TABLE", "VOX_MAX_POINTS")}
    m = one(r"\(unsigned\)x \* (\d+)u \^ \(unsigned\)y \* (\d+)u \^ \(unsigned\)z \* (\d+)u;")
    out["MUL"] = tuple(int(g) for g in m.groups())
    m = one(r"h \^= h >> 16; h \*= (0x[0-9a-f]+)u; h \^= h >> 13; h \*= (0x[0-9a-f]+)u; h \^= h >> 16;")
    out["MIX"] = tuple(int(g, 16) for g in m.groups())
    m = one(r"const size_t lds = (\d+) \* \(size_t\)\(dim \+ PW_MAX_LEAVES \+ (\d+)\) \* sizeof\(float\);")
    out["ROWS_PER_WG"], out["PW_STACK"] = int(m.group(1)), int(m.group(2))
    out["LDS_STATIC_MAX"] = int(one(r"if \(lds > (\d+) &&").group(1))
    assert "if (n <= 128) {" in src and "n2 -= n2 % 8;" in src and "if (len < 8) {" in src      # what pw_leaves restates
    assert "for (int j = threadIdx.x; j < dim; j += 128)" in src                                 # what record_branches restates
    return out


K = parse_constants(open(HIP).read())
VOX_TABLE, VOX_MAX_POINTS = K["VOX_TABLE"], K["VOX_MAX_POINTS"]
VOX_MASK = VOX_TABLE - 1


# ----------------------------------------------------------------------------------------------------------------------
# histogram rows
# ----------------------------------------------------------------------------------------------------------------------
def dims():
    return tuple(range(1, 137)) + (255, 256, 257, 799, 800, 801, 1023, 1024, 1025, 2047, 2048, 2049, 4015, 4016, 4017,
                                   4095, 4096)


def row_counts():
    """Rows per launch; a workgroup holds 4, the dead waves of the last one read row n - 1."""
    return (1, 2, 3, 4, 5, 9)


def pw_leaves(n, start=0):
    """(start, length) of the leaves of numpy's pairwise tree over n contiguous float32, left to right."""
    if n <= 128:
        return [(start, n)]
    n2 = n // 2
    n2 -= n2 % 8
    return pw_leaves(n2, start) + pw_leaves(n - n2, start + n2)


def leaf_kinds(dim):
    lv = pw_leaves(dim)
    out = {"split"} if len(lv) > 1 else set()
    for _, ln in lv:
        out.add("leaf<8" if ln < 8 else "tail" if ln & 7 else "whole")
    if len(lv) > 1 and len({ln for _, ln in lv}) > 1:
        out.add("uneven-split")
    return out


def lds_bytes(dim):
    return K["ROWS_PER_WG"] * (dim + K["PW_MAX_LEAVES"] + K["PW_STACK"]) * 4


def dynamic_lds(dim):
    return lds_bytes(dim) > K["LDS_STATIC_MAX"]


def seq_sum(row):
    """float32 sum in ascending order, one accumulator."""
    return np.cumsum(row, dtype=F32)[-1] if len(row) else F32(0)


def leafseq_sum(row):
    """numpy's pairwise tree, but with the 8 accumulators of a leaf combined r0 + r1 + ... + r7 in sequence instead of
    ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)): the wrong order a lane butterfly is most likely to have."""
    def rec(st, n):
        if n < 8:
            return seq_sum(row[st:st + n])
        if n <= 128:
            m = n - n % 8
            r = np.cumsum(row[st:st + m].reshape(-1, 8), axis=0, dtype=F32)[-1]
            res = r[0]
            for x in list(r[1:]) + list(row[st + m:st + n]):
                res = F32(res + x)
            return res
        n2 = n // 2
        n2 -= n2 % 8
        return F32(rec(st, n2) + rec(st + n2, n - n2))
    return rec(0, len(row))


def quantize_with_sum(row, s):
    """ko.quantize with the row sum given: what the quantiser returns if its sum comes out as ``s``."""
    h = row / (s + EPS32) if s > EPS32 else row
    q = np.round(h * F32(MAX_U16)).astype(np.uint16)
    qs = int(q.sum())
    if qs > 0 and qs != MAX_U16:
        i = int(q.argmax())
        q[i] = np.uint16(min(max(int(q[i]) + MAX_U16 - qs, 0), MAX_U16))
    return q


def order_reaches_words(row, alt=seq_sum):
    """True if summing the row in the order ``alt`` instead of numpy's changes the sum AND the quantised words."""
    s, sa = row.sum(), alt(row)
    return bool(s != sa and (quantize_with_sum(row, s) != quantize_with_sum(row, sa)).any())


def _sharpen(row, alt, rng, budget=400):
    """A last bit of the sum moves a product h * 65535 by a few 1e-8 of its value: it changes a word only if the product
    sits on a rounding boundary.  Move one bin after the other next to its boundary (x = (k + 1/2) (s + eps) / 65535,
    give or take 2 ulp) until the order ``alt`` gives other words than numpy's order (and the plain sequential order
    another sum).  Returns None if it never does."""
    row = row.copy()
    for _ in range(budget):
        if order_reaches_words(row, alt) and seq_sum(row) != row.sum():
            return row
        j = int(rng.integers(len(row)))
        den = row.sum() + EPS32
        k = np.floor(row[j] / den * F32(MAX_U16))
        x = F32((float(k) + 0.5) * float(den) / MAX_U16)
        for _ in range(abs(int(step := rng.integers(-2, 3)))):
            x = np.nextafter(x, F32(np.inf) if step > 0 else F32(0))
        row[j] = x
    return None


@functools.lru_cache(maxsize=None)
def _wide(dim, n, seed):
    rng = np.random.default_rng([11, dim, n, seed])
    rows = (rng.random((n, dim)) ** 8 * 10.0 ** rng.integers(-6, 4, (n, dim))).astype(F32)
    if dim >= 8:
        for i in range(0, n, 2):
            for _ in range(8):                               # a fresh draw where one cannot be sharpened
                s = _sharpen(rows[i], leafseq_sum if i % 4 == 2 else seq_sum, rng)
                if s is not None:
                    rows[i] = s
                    break
                rows[i] = (rng.random(dim) ** 8 * 10.0 ** rng.integers(-6, 4, dim)).astype(F32)
    rows.setflags(write=False)
    return rows


def wide(dim, n, seed=0):
    """rand()**8 * 10**randint(-6, 3): nine decades of magnitude and a heavy tail.  On such rows the order of the
    float32 additions shows in the sum for about half of them at dim 16..31 (0.38..0.55 over 200 rows, whatever the
    exponent and the decades) and almost never in the 16-bit words, so every other row (0, 2, 4, ...) is sharpened:
    bins are moved onto rounding boundaries until the sequential order (rows 0, 4, 8) or the sequentially combined leaf
    (rows 2, 6) changes the quantised words, not only the sum.  Below dim 8 there is one order only."""
    return _wide(dim, n, seed)


def order_shows(rows):
    """Share of the rows whose sequential float32 sum differs from ndarray.sum()."""
    seq = np.array([seq_sum(r) for r in rows])
    pw = np.array([r.sum() for r in rows])
    return float(np.mean(seq != pw))


TIE_DIMS = (130, 800)


def tie_pairs(dim):
    return ((0, dim - 1), (63, 64), (64, 128), (5, 69), (dim - 2, dim - 1))


def ties(dim):
    """One row per bin pair: 1/4 at both bins of the pair (16 383.75 -> 16 384 twice, the maximum), 1/2 spread evenly
    over a power-of-two number of other bins (each c + 1 - 2^-j -> c + 1, so the rounded words sum to 65 536, one too
    many).  Everything is dyadic and sums to exactly 1.0 in any order; the reference takes the 1 off the FIRST maximum,
    which for (63, 64) sits in lane 63 while the second sits in lane 0, and for (5, 69) in the same lane."""
    assert dim >= 130
    rows = np.zeros((len(tie_pairs(dim)), dim), F32)
    p = 1 << ((dim - 2).bit_length() - 1)                    # largest power of two <= dim - 2
    for r, (a, b) in enumerate(tie_pairs(dim)):
        rest = [j for j in range(dim) if j not in (a, b)][:p]
        rows[r, rest] = F32(0.5 / p)
        rows[r, [a, b]] = F32(0.25)
    return rows


def excess_over_max():
    """dim 4096: 4 000 bins of 0.52 / 65 535 (each rounds up to 1) and the remainder split evenly over the last 96.
    The rounded words sum to 67 456, the largest is 661: the correction of -1 921 would take it below zero."""
    row = np.empty(4096, F32)
    small = 0.52 / MAX_U16
    row[:4000] = F32(small)
    row[4000:] = F32((1.0 - 4000 * small) / 96)
    return row[None]


@functools.lru_cache(maxsize=None)
def half_tie_values():
    """Every m for which h = m / 2^17 has float32(h * 65535) exactly k + 1/2 (the exact product m * 65535 / 2^17 is
    never half-integral -- 65 535 is odd -- so these are the h whose product ROUNDS onto one)."""
    m = np.arange(1, 1 << 17, dtype=np.int64)
    prod = (m / 131072.0).astype(F32) * F32(MAX_U16)
    assert prod.dtype == np.float32
    hit = (prod.astype(np.float64) * 2 % 2) == 1
    return tuple(int(x) for x in m[hit])


HALF_TIE_DIMS = (4, 130, 2049)


def half_ties(dim):
    """Two rows summing to exactly 1.0: m / 2^17 with the first k-odd and the first k-even product k + 1/2 in the middle
    bin, 1/2 in bin 0 (the maximum, so that a correction lands there and not on the bin under test; 32 767.5 is a
    k-odd product itself) and the remainder, a 2^-17 multiple, in the last bin.  np.round goes to the even word, roundf
    away from zero: they differ on the k-even row."""
    assert dim >= 4
    vals = half_tie_values()
    k_of = {m: int(np.floor(float(F32(m / 131072.0) * F32(MAX_U16)))) for m in vals[:8]}
    odd = next(m for m in vals if k_of[m] % 2 == 1)
    even = next(m for m in vals if k_of[m] % 2 == 0)
    rows = np.zeros((2, dim), F32)
    for r, m in enumerate((odd, even)):
        rest = 131072 - m - 65536
        assert 0 < rest < m < 65536
        rows[r, dim // 2] = F32(m / 131072.0)
        rows[r, 0] = F32(0.5)
        rows[r, dim - 1] = F32(rest / 131072.0)
    return rows, (odd, even)


def eps_edge(dim):
    """Five rows at the boundary of ``s > eps``: sums 0, exactly float32(1e-8), one ulp above; a single 1.0; uniform."""
    rows = np.zeros((5, dim), F32)
    rows[1, dim - 1] = EPS32
    rows[2, dim // 2] = np.nextafter(EPS32, F32(1))
    rows[3, (2 * dim) // 3] = F32(1.0)
    rows[4] = F32(1.0) / F32(dim)
    return rows


def quant_families(dim):
    """name -> (rows, dim) float32 of every quantiser family that exists at this dim."""
    out = {"wide": wide(dim, 9), "eps_edge": eps_edge(dim)}
    if dim in TIE_DIMS:
        out["ties"] = ties(dim)
    if dim == 4096:
        out["excess_over_max"] = excess_over_max()
    if dim in HALF_TIE_DIMS:
        out["half_ties"] = half_ties(dim)[0]
    return out


def words(dim):
    """uint16 rows for the dequantiser: all zero (-> 1/dim), a single 1, a single 65 535, all 65 535 (float32 sum
    above 2^24 at dim 4096), random words."""
    rng = np.random.default_rng([12, dim])
    w = np.zeros((8, dim), np.uint16)
    w[1, dim // 3] = 1
    w[2, dim - 1] = MAX_U16
    w[3] = MAX_U16
    w[4:] = rng.integers(0, 65536, (4, dim)).astype(np.uint16)
    return w


def take_rows(rows, n, start=0):
    """n rows of a family, cycling through it from ``start``."""
    return np.ascontiguousarray(rows[(start + np.arange(n)) % len(rows)])


def quant_steps(row):
    """The reference's quantiser line by line, with what happened on the way (for the path table and the family checks)."""
    s = row.sum()
    norm = bool(s > EPS32)
    h = row / (s + EPS32) if norm else row
    prod = h * F32(MAX_U16)
    r = np.round(prod).astype(np.int64)
    tot = int(r.sum())
    first = int(np.argmax(r))
    if tot == 0 or tot == MAX_U16:
        corr = "none"
    elif int(r[first]) + MAX_U16 - tot < 0:
        corr = "clamped"
    else:
        corr = "plus" if tot < MAX_U16 else "minus"
    return dict(s=s, norm=norm, prod=prod, rounded=r, tot=tot, first=first, corr=corr)


@functools.lru_cache(maxsize=None)
def quant_reference(dim):
    """name -> (rows, oracle words, oracle dequantised words) for every quantiser family of the dim; computed once."""
    out = {}
    for name, rows in quant_families(dim).items():
        q = np.stack([ko.quantize(r) for r in rows])
        d = np.stack([ko.dequantize(x) for x in q])
        for a in (rows, q, d):
            a.setflags(write=False)
        out[name] = (rows, q, d)
    return out


@functools.lru_cache(maxsize=None)
def words_reference(dim):
    w = words(dim)
    d = np.stack([ko.dequantize(x) for x in w])
    w.setflags(write=False)
    d.setflags(write=False)
    return w, d


# ----------------------------------------------------------------------------------------------------------------------
# records
# ----------------------------------------------------------------------------------------------------------------------
RECORD_DIMS = (1, 2, 50, 127, 128, 129, 800, 4096)
RECORD_N = (1, 3, 257)
Records = namedtuple("Records", "q pose7 ts ids hashes reserved")


@functools.lru_cache(maxsize=None)
def records(n, dim):
    """Metadata as raw bytes: the 120 bytes of one record's block (28 pose + 8 timestamp + 4 id + 20 hash + 60
    reserved) are all distinct, so a byte moved to another offset is a different byte.  The floats are whatever those
    bytes are (NaN payloads included): compare by uint8 view.  ``reserved`` is garbage for the unpack tests; pack writes
    zeros there."""
    rng = np.random.default_rng([13, n, dim])
    q = rng.integers(0, 65536, (n, dim)).astype(np.uint16)
    q[0, 0], q[n - 1, dim - 1] = 0x0102, 0xfffe
    block = np.stack([rng.permutation(256)[:120] for _ in range(n)]).astype(np.uint8)
    out = Records(q, block[:, 0:28].copy(), block[:, 28:36].copy(), block[:, 36:40].copy(), block[:, 40:60].copy(),
                  block[:, 60:120].copy())
    for a in out:
        a.setflags(write=False)
    return out


def records_reference(rec):
    """(n, 2 dim + 120) uint8 from ko.pack_record, one record at a time."""
    n = len(rec.q)
    rows = []
    for i in range(n):
        b = ko.pack_record(rec.q[i], rec.pose7[i].view(np.float32), rec.ts[i].view(np.float64)[0],
                           int(rec.ids[i].view(np.uint32)[0]), rec.hashes[i].tobytes())
        rows.append(np.frombuffer(b, np.uint8))
    return np.stack(rows)


def with_reserved(packed, rec):
    """The packed records with the 60 reserved bytes replaced by the family's garbage."""
    out = packed.copy()
    out[:, -60:] = rec.reserved
    return out


def record_branches(dim):
    out = {"words-one-trip" if dim <= 128 else "words-several-trips"}
    if dim % 128:
        out.add("words-partial-trip")
    if dim < 128:
        out.add("idle-word-lanes")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# chain graphs
# ----------------------------------------------------------------------------------------------------------------------
def chain_grid():
    return tuple((n, m) for n in range(13) for m in range(13)) + ((300, 5), (64, 9), (4541, 5), (7, 64))


def loop_lists(n):
    """name -> loop-closure list for an n-node graph: none, one, several with repeats, q == m, and out-of-range entries
    (the wrapper filters them as the reference does)."""
    last = max(n - 1, 0)
    return {"none": None,
            "one": [(0, last)],
            "repeats": [(0, last), (last, 0), (0, last), (n // 2, n // 3), (n // 2, n // 3)],
            "self": [(n // 2, n // 2), (0, 0)],
            "out_of_range": [(0, n), (-1, 0), (n + 5, n + 7), (last, n // 2), (n, n)]}


def valid_loops(n, loops):
    return [(q, m) for q, m in (loops or []) if 0 <= q < n and 0 <= m < n]


def _rotz(a):
    c, s = np.cos(a), np.sin(a)
    if a == np.pi:
        c, s = -1.0, 0.0                                 # exactly pi
    if a == np.pi / 2:
        c, s = 0.0, 1.0
    T = np.eye(4)
    T[:2, :2] = [[c, -s], [s, c]]
    return T


def _trans(x, y=0.0, z=0.0):
    T = np.eye(4)
    T[:3, 3] = [x, y, z]
    return T


def poses_special():
    """(names, poses): identical poses, pure translations of 1e-9, 1 and 1e6, rotations about z by exactly pi, pi/2,
    1e-8 and 1e-4, and matrices scaled by 1 +- 1e-3 (against themselves and each other the trace passes 3, against
    their half-turn it passes -1: both clips act).  Run as a graph in which every pair is an edge (half >= n)."""
    names = ["eye", "eye_again", "t1e-9", "t1", "t1e6", "rz_pi", "rz_pi2", "rz_1e-8", "rz_1e-4", "scale_up",
             "scale_up_again", "scale_down", "scale_up_rz_pi", "scale_down_rz_pi"]
    up, down = np.eye(4), np.eye(4)
    up[:3, :3] *= 1.0 + 1e-3
    down[:3, :3] *= 1.0 - 1e-3
    up_pi, down_pi = _rotz(np.pi), _rotz(np.pi)
    up_pi[:3, :3] *= 1.0 + 1e-3
    down_pi[:3, :3] *= 1.0 - 1e-3
    poses = [np.eye(4), np.eye(4), _trans(1e-9), _trans(0.0, 1.0), _trans(0.0, 0.0, 1e6), _rotz(np.pi), _rotz(np.pi / 2),
             _rotz(1e-8), _rotz(1e-4), up, up.copy(), down, up_pi, down_pi]
    return names, np.ascontiguousarray(np.stack(poses), dtype=np.float64)


def edge_quantities(poses, i, j):
    """(distance, trace before the clip) of edge i -> j, in float64 as the reference computes them."""
    d = float(np.linalg.norm(poses[i, :3, 3] - poses[j, :3, 3]))
    return d, float(np.trace(poses[j, :3, :3] @ poses[i, :3, :3].T))


def chain_branches(n, m, loops, poses=None):
    half = m // 2
    out = {"half=0" if half == 0 else "n<=half" if n <= half else "n>half"}
    if n == 0:
        out.add("n=0")
    out.add("loops" if valid_loops(n, loops) else "no-loops")
    if loops and len(valid_loops(n, loops)) < len(loops):
        out.add("loops-filtered")
    if any(q == mm for q, mm in valid_loops(n, loops)):
        out.add("loop-self")
    if 2 * half * n + 2 * len(valid_loops(n, loops)) > 256:
        out.add("several-workgroups")
    if poses is not None:
        out.add("poses")
        ei = ko.chain_graph_loop(n, m, None, loops)[0]
        for i, j in ei.T:
            d, tr = edge_quantities(poses, i, j)
            if d == 0.0:
                out.add("distance-0")
            if tr > 3.0:
                out.add("trace>3")
            if tr < -1.0:
                out.add("trace<-1")
            if tr == 3.0:
                out.add("angle-0")
            if tr == -1.0:
                out.add("angle-pi")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# clouds
# ----------------------------------------------------------------------------------------------------------------------
V = 0.25                                                 # lattice voxel: (k + 0.5) * V is exact in float32 and float64
_M32 = 0xffffffff


def vox_hash(x, y, z):
    """The kernel's hash, in Python integers."""
    h = ((x & _M32) * K["MUL"][0] ^ (y & _M32) * K["MUL"][1] ^ (z & _M32) * K["MUL"][2]) & _M32
    h ^= h >> 16
    h = h * K["MIX"][0] & _M32
    h ^= h >> 13
    h = h * K["MIX"][1] & _M32
    h ^= h >> 16
    return h


def home_slot(x, y, z):
    return vox_hash(int(x), int(y), int(z)) & VOX_MASK


def vox_hash_np(v):
    """The same over an (n, 3) integer array (uint32 arithmetic wraps)."""
    u = np.asarray(v).astype(np.int64).astype(np.uint32)
    with np.errstate(over="ignore"):
        h = u[:, 0] * np.uint32(K["MUL"][0]) ^ u[:, 1] * np.uint32(K["MUL"][1]) ^ u[:, 2] * np.uint32(K["MUL"][2])
        h ^= h >> np.uint32(16)
        h *= np.uint32(K["MIX"][0])
        h ^= h >> np.uint32(13)
        h *= np.uint32(K["MIX"][1])
        h ^= h >> np.uint32(16)
    return h


BOX = 48                                                 # lattice box [-48, 48)^3: 54 voxels per slot on average


@functools.lru_cache(maxsize=None)
def _box():
    g = np.arange(-BOX, BOX, dtype=np.int32)
    v = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return v, (vox_hash_np(v) & np.uint32(VOX_MASK)).astype(np.int64)


def voxels_at_slot(slot, k):
    v, home = _box()
    out = v[home == slot][:k]
    assert len(out) == k, (slot, k)
    return out


def fullest_slot():
    _, home = _box()
    return int(np.argmax(np.bincount(home, minlength=VOX_TABLE)))


Pair = namedtuple("Pair", "name p1 p2 T voxel")


def _pts(vox, stride, rng, t=(0, 0, 0), jitter=False):
    """One point per row of ``vox``, at the centre of the lattice voxel (or anywhere in its middle half); moved by -t so
    that a translation by t (whole metres = 4 voxels) brings it back."""
    vox = np.asarray(vox, dtype=np.float64).reshape(-1, 3)
    frac = rng.integers(4, 13, vox.shape) / 16.0 if jitter else 0.5
    p = np.zeros((len(vox), stride), F32)
    p[:, :3] = ((vox + frac) * V - np.asarray(t, dtype=np.float64)).astype(F32)
    if stride == 4:
        p[:, 3] = rng.random(len(vox)).astype(F32)
    return p


def _T(t=(0, 0, 0)):
    return _trans(*[float(x) for x in t])


def _none(stride):
    return np.zeros((0, stride), F32)


def collide(stride):
    """K in {2, 8, 40} lattice voxels sharing one home slot: all in cloud 1, all in cloud 2, and split with the middle
    third in both (cloud 1 comes in through a translation there)."""
    out, slot = [], fullest_slot()
    for k in (2, 8, 40):
        rng = np.random.default_rng([14, k, stride])
        vox = voxels_at_slot(slot, k)
        a, b = vox[: (2 * k + 2) // 3], vox[k // 3:]
        t = (3, -2, 1)
        out += [Pair("collide%d/cloud1" % k, _pts(vox, stride, rng), _none(stride), _T(), V),
                Pair("collide%d/cloud2" % k, _none(stride), _pts(vox, stride, rng), _T(), V),
                Pair("collide%d/split" % k, _pts(a, stride, rng, t), _pts(b, stride, rng), _T(t), V)]
    return out


WRAP_SLOTS = (VOX_TABLE - 4, VOX_TABLE - 3, VOX_TABLE - 2, VOX_TABLE - 1)


def wrap_voxels():
    """Three voxels at each of the last four home slots: twelve voxels for four slots, the chain runs on to slot 7."""
    return np.concatenate([voxels_at_slot(s, 3) for s in WRAP_SLOTS])


def wrap(stride):
    """The chain 16380 .. 16383 -> 0 .. 7; cloud 2 looks the same voxels up again (twice each) and adds two voxels whose
    home is slot 0 and 1 and which land behind the chain.  Second pair: the chain is built by cloud 2 alone."""
    rng = np.random.default_rng([15, stride])
    vox = wrap_voxels()
    late = np.concatenate([voxels_at_slot(0, 1), voxels_at_slot(1, 1)])
    c2 = np.concatenate([vox, late, vox[::-1]])
    return [Pair("wrap/lookup", _pts(vox, stride, rng), _pts(c2, stride, rng, jitter=True), _T(), V),
            Pair("wrap/cloud2", _none(stride), _pts(c2, stride, rng, jitter=True), _T(), V)]


def full_voxels():
    g = np.stack(np.meshgrid(np.arange(-12, 12), np.arange(-16, 16), np.arange(-8, 8), indexing="ij"), -1).reshape(-1, 3)
    assert len(g) == VOX_MAX_POINTS
    return g[np.random.default_rng(16).permutation(len(g))]


def full(stride):
    """The table at its stated capacity: 12 288 distinct voxels (load 0.75)."""
    rng = np.random.default_rng([16, stride])
    vox, h = full_voxels(), VOX_MAX_POINTS // 2
    t = (-5, 0, 2)
    return [Pair("full/12288+0", _pts(vox, stride, rng), _none(stride), _T(), V),
            Pair("full/0+12288", _none(stride), _pts(vox, stride, rng), _T(), V),
            Pair("full/disjoint", _pts(vox[:h], stride, rng, t), _pts(vox[h:], stride, rng), _T(t), V),
            Pair("full/identical", _pts(vox[:h], stride, rng), _pts(vox[:h][::-1], stride, rng, jitter=True), _T(), V)]


def one_slot(stride):
    """12 288 points racing for one slot, in either cloud; one of them elsewhere; and both clouds on the same two
    voxels (6 144 points of cloud 2 race for two flag bits)."""
    rng = np.random.default_rng([17, stride])
    n, a, b = VOX_MAX_POINTS, np.array([7, -3, 2]), np.array([-20, 11, 0])
    two = np.where((np.arange(n // 2) % 2 == 0)[:, None], a, b)
    return [Pair("one_slot/cloud1", _pts(np.tile(a, (n, 1)), stride, rng, jitter=True), _none(stride), _T(), V),
            Pair("one_slot/cloud2", _none(stride), _pts(np.tile(a, (n, 1)), stride, rng, jitter=True), _T(), V),
            Pair("one_slot/plus_one", _pts(np.concatenate([np.tile(a, (n - 1, 1)), b[None]]), stride, rng, jitter=True),
                 _none(stride), _T(), V),
            Pair("one_slot/two_voxels", _pts(two, stride, rng, jitter=True), _pts(two[::-1], stride, rng, jitter=True),
                 _T(), V)]


def _dead(n, stride, rng):
    """Rows that the finite filter drops: NaN x, Inf y, and (stride 4) NaN intensity on an otherwise fine row."""
    p = _pts(rng.integers(-5, 5, (n, 3)), stride, rng)
    kind = np.arange(n) % (3 if stride == 4 else 2)
    p[kind == 0, 0] = np.nan
    p[kind == 1, 1] = np.inf
    if stride == 4:
        p[kind == 2, 3] = np.nan
    return p


def empties(stride):
    rng = np.random.default_rng([18, stride])
    some = rng.integers(-6, 6, (40, 3))
    return [Pair("empty/n1=0", _none(stride), _pts(some, stride, rng), _T(), V),
            Pair("empty/n2=0", _pts(some, stride, rng), _none(stride), _T(), V),
            Pair("empty/both", _none(stride), _none(stride), _T(), V),
            Pair("empty/dead1", _dead(30, stride, rng), _pts(some, stride, rng), _T(), V),
            Pair("empty/dead2", _pts(some, stride, rng), _dead(30, stride, rng), _T(), V),
            Pair("empty/dead_both", _dead(31, stride, rng), _dead(29, stride, rng), _T(), V)]


FLT_MAX = np.finfo(np.float32).max


def face_values(voxel):
    v = F32(voxel)
    up, dn = np.nextafter(v, F32(1)), np.nextafter(v, F32(0))          # v (1 +- 2^-23) (2^-24 below a power of two)
    vals = [-0.0, 0.0, v, -v, up, -up, dn, -dn, -1e-30, 1e-30, 0.6, -0.6, 3 * v, -3 * v, 1e6, -1e6, 1.5e6, -1.5e6,
            FLT_MAX, -FLT_MAX]
    return np.array(vals, dtype=F32)


def faces(stride):
    """Coordinates on and next to voxel faces, at the clip and beyond it, on every axis and on all three at once; the
    same points in both clouds, which divide in float64 and float32 (0.6 / 0.2: 2 against 3)."""
    out = []
    for voxel in (V, 0.2):
        rng = np.random.default_rng([19, stride])
        vals = face_values(voxel)
        rows = []
        for a in vals:
            rows += [(a, 0.1, 0.1), (0.1, a, 0.1), (0.1, 0.1, a), (a, a, a)]
        p = np.zeros((len(rows), stride), F32)
        p[:, :3] = np.array(rows, dtype=F32)
        if stride == 4:
            p[:, 3] = rng.random(len(rows)).astype(F32)
        out.append(Pair("faces/v%g" % voxel, p, p.copy(), _T(), voxel))
    return out


def rigid(stride):
    """3 000 random points under a general rotation and translation; cloud 2 is the moved cloud rounded to float32, every
    other point of it displaced."""
    rng = np.random.default_rng([20, stride])
    qm, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    T = np.eye(4)
    T[:3, :3] = qm * np.sign(np.linalg.det(qm))
    T[:3, 3] = [12.3456789, -7.25, 0.3]
    p1 = np.zeros((3000, stride), F32)
    p1[:, :3] = rng.uniform(-15, 15, (3000, 3)).astype(F32)
    p2 = np.zeros((3000, stride), F32)
    noise = rng.normal(0.0, 0.3, (3000, 3)) * (np.arange(3000) % 2)[:, None]          # every other point moves away
    p2[:, :3] = (p1[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3] + noise).astype(F32)
    if stride == 4:
        p1[:, 3], p2[:, 3] = rng.random(3000), rng.random(3000)
    return [Pair("rigid", p1, p2[rng.permutation(3000)], T, V)]


CLOUD_FAMILIES = (collide, wrap, full, one_slot, empties, faces, rigid)


@functools.lru_cache(maxsize=None)
def cloud_pairs(stride):
    out = tuple(p for fam in CLOUD_FAMILIES for p in fam(stride))
    assert len({p.name for p in out}) == len(out)
    for p in out:
        assert p.p1.shape[1] == p.p2.shape[1] == stride and len(p.p1) + len(p.p2) <= VOX_MAX_POINTS, p.name
        assert p.voxel >= 0.001
        for a in p[1:4]:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cloud_reference(stride):
    """name -> (iou, counts) of the oracle (sort and merge, no hash); computed once."""
    return {p.name: ko.voxel_overlap(p.p1, p.p2, p.T, p.voxel) for p in cloud_pairs(stride)}


def batch_order(pairs):
    """The pairs of one launch, ordered so that empty and full pairs alternate: largest, smallest, second largest, ..."""
    by = sorted(pairs, key=lambda p: len(p.p1) + len(p.p2))
    out = []
    while by:
        out.append(by.pop())
        if by:
            out.append(by.pop(0))
    return out


def shuffled(pair, seed=1):
    rng = np.random.default_rng(seed)
    return pair._replace(p1=pair.p1[rng.permutation(len(pair.p1))], p2=pair.p2[rng.permutation(len(pair.p2))])


def guard_batch(stride=3):
    """Three pairs for one direct call: the middle one holds 12 289 points (12 288 + 1), one more than the table takes."""
    rng = np.random.default_rng([21, stride])
    some = rng.integers(-6, 6, (50, 3))
    big = Pair("guard/12289", _pts(full_voxels(), stride, rng), _pts(some[:1], stride, rng), _T(), V)
    return [Pair("guard/before", _pts(some, stride, rng), _pts(some[10:], stride, rng), _T(), V), big,
            Pair("guard/after", _pts(some[:20], stride, rng), _pts(some, stride, rng), _T(), V)]


def voxels_np(pair):
    """numpy restatement of the two voxelisations: (int32 voxels of cloud 1, of cloud 2), rows in point order, dropped
    rows left out.  Cloud 1 through ``T @ hom.T`` in float64, cloud 2 in float32."""
    p1, p2, v = pair.p1, pair.p2, pair.voxel
    hom = np.concatenate([p1[:, :3].astype(np.float64), np.ones((len(p1), 1))], 1)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(pair.T, dtype=np.float64) @ hom.T).T[:, :3] if len(p1) else np.zeros((0, 3))
        ok1 = np.isfinite(t).all(1) & np.isfinite(p1[:, 3:]).all(1)
        v1 = np.floor(np.clip(t[ok1], -1e6, 1e6) / v).astype(np.int32)
        ok2 = np.isfinite(p2).all(1)
        q = np.clip(p2[ok2][:, :3], F32(-1e6), F32(1e6)) / F32(v)
        assert q.dtype == np.float32
        v2 = np.floor(q).astype(np.int32)
    return v1.reshape(-1, 3), v2.reshape(-1, 3)


def overlap_np(pair):
    v1, v2 = voxels_np(pair)
    u1 = np.unique(v1, axis=0) if len(v1) else v1
    u2 = np.unique(v2, axis=0) if len(v2) else v2
    inter = len(set(map(tuple, u1.tolist())) & set(map(tuple, u2.tolist())))
    uni = len(u1) + len(u2) - inter
    return (inter / uni if uni else 0.0), [len(u1), len(u2), inter]


def probe_table(v1, v2):
    """Linear probing as the kernel does it, one point after the other.  Returns (slot -> voxel, branches taken).  The
    occupied slots of a linear-probing table do not depend on the insertion order; which branch a given point takes
    does, but every branch named here is taken under any order (a displaced voxel stays displaced whoever comes first)."""
    table, owner, flagged, br = {}, {}, set(), set()
    for which, vs in ((1, v1), (2, v2)):
        for x, y, z in vs.tolist():
            h, steps, wrapped = home_slot(x, y, z), 0, False
            while True:
                if h not in table:
                    table[h], owner[h] = (x, y, z), which
                    br.add("insert-first-probe" if steps == 0 else "insert-after-wrap" if wrapped else "insert-after-collision")
                    break
                if table[h] == (x, y, z):
                    if which == 1:
                        br.add("present-in-set1")
                    elif owner[h] == 2:
                        br.add("match-set2-only")
                    elif h in flagged:
                        br.add("match-already-flagged")
                    else:
                        flagged.add(h)
                        br.add("match-set1-after-wrap" if wrapped else "match-set1")
                    break
                h = (h + 1) & VOX_MASK
                steps += 1
                wrapped = wrapped or h == 0
    return table, br


def voxel_branches(pair):
    if len(pair.p1) + len(pair.p2) > VOX_MAX_POINTS:
        return {"guard"}
    v1, v2 = voxels_np(pair)
    br = probe_table(v1, v2)[1]
    if len(v1) < len(pair.p1) or len(v2) < len(pair.p2):
        br.add("row-dropped")
    if len(pair.p1) == 0 or len(pair.p2) == 0:
        br.add("empty-cloud")
    if len(v1) + len(v2) == 0:
        br.add("empty-union")
    if not np.array_equal(np.asarray(pair.T), np.eye(4)):
        br.add("transform")
    if len(np.unique(np.concatenate([v1, v2]), axis=0) if len(v1) + len(v2) else []) == VOX_MAX_POINTS:
        br.add("table-at-capacity")
    return br


# ----------------------------------------------------------------------------------------------------------------------
# the path table
# ----------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "kernel family branches")

REQUIRED = {
    "quantize_kernel<false>": {"leaf<8", "tail", "whole", "split", "uneven-split", "normalised", "not-normalised",
                               "correction-none", "correction-plus", "correction-minus", "correction-clamped",
                               "tie-first-in-higher-lane", "tie-in-one-lane", "product-k+half-odd", "product-k+half-even",
                               "sum==eps", "sum==eps+1ulp", "lds-static", "lds-dynamic", "dead-waves"},
    "quantize_kernel<true>": {"leaf<8", "tail", "whole", "split", "uneven-split", "normalised", "not-normalised",
                              "sum>2^24", "lds-static", "lds-dynamic", "dead-waves"},
    "pack_kernel": {"words-one-trip", "words-several-trips", "words-partial-trip", "idle-word-lanes", "reserved-zeroed",
                    "several-records"},
    "unpack_kernel": {"words-one-trip", "words-several-trips", "words-partial-trip", "idle-word-lanes", "reserved-ignored",
                      "several-records"},
    "chain_graph_kernel": {"half=0", "n<=half", "n>half", "n=0", "loops", "no-loops", "loops-filtered", "loop-self",
                           "several-workgroups", "poses", "distance-0", "trace>3", "trace<-1", "angle-0", "angle-pi"},
    "voxel_overlap_kernel": {"insert-first-probe", "insert-after-collision", "insert-after-wrap", "present-in-set1",
                             "match-set1", "match-set1-after-wrap", "match-set2-only", "match-already-flagged",
                             "row-dropped", "empty-cloud", "empty-union", "transform", "table-at-capacity", "guard"},
}


def _quant_row_branches(name, rows, dim):
    br = set()
    for i, row in enumerate(rows):
        st = quant_steps(row)
        br.add("normalised" if st["norm"] else "not-normalised")
        br.add("correction-" + st["corr"])
        if st["s"] == EPS32:
            br.add("sum==eps")
        if st["s"] == np.nextafter(EPS32, F32(1)):
            br.add("sum==eps+1ulp")
        if name == "ties":
            a, b = tie_pairs(dim)[i]
            assert st["first"] == a and st["rounded"][a] == st["rounded"][b] == st["rounded"].max()
            if a % 64 > b % 64:
                br.add("tie-first-in-higher-lane")
            if a % 64 == b % 64:
                br.add("tie-in-one-lane")
        if name == "half_ties":
            frac = st["prod"].astype(np.float64) % 1.0 == 0.5
            for kk in np.floor(st["prod"][frac]).astype(np.int64):
                br.add("product-k+half-odd" if kk % 2 else "product-k+half-even")
    return br


@functools.lru_cache(maxsize=None)
def cases():
    t = []
    per_family = {}
    for dim in dims():
        shape = leaf_kinds(dim) | {"lds-dynamic" if dynamic_lds(dim) else "lds-static"}
        for name, rows in quant_families(dim).items():
            per_family.setdefault(("quantize_kernel<false>", name), set()).update(shape | _quant_row_branches(name, rows, dim))
        w, _ = words_reference(dim)
        br = set(shape)
        for row in w:
            s = row.astype(F32).sum()
            br.add("normalised" if s > EPS32 else "not-normalised")
            if s > F32(2.0 ** 24):
                br.add("sum>2^24")
        per_family.setdefault(("quantize_kernel<true>", "words"), set()).update(br)
    if any(n % K["ROWS_PER_WG"] for n in row_counts()):
        for k in per_family:
            per_family[k].add("dead-waves")
    for (kern, name), br in per_family.items():
        t.append(Case(kern, name, frozenset(br)))
    for kern, extra in (("pack_kernel", "reserved-zeroed"), ("unpack_kernel", "reserved-ignored")):
        for dim in RECORD_DIMS:
            br = record_branches(dim) | {extra}
            if max(RECORD_N) > 1:
                br.add("several-records")
            t.append(Case(kern, "records/dim%d" % dim, frozenset(br)))
    grid = set()
    for n, m in chain_grid():
        for loops in loop_lists(n).values():
            grid |= chain_branches(n, m, loops)
    t.append(Case("chain_graph_kernel", "chain_grid", frozenset(grid | {"poses"})))
    names, poses = poses_special()
    n = len(poses)
    t.append(Case("chain_graph_kernel", "poses_special",
                  frozenset(chain_branches(n, 2 * n, [(9, 9), (12, 0), (0, 12)], poses))))
    for p in cloud_pairs(3):
        t.append(Case("voxel_overlap_kernel", p.name, frozenset(voxel_branches(p))))
    t.append(Case("voxel_overlap_kernel", "guard/12289", frozenset(voxel_branches(guard_batch()[1]))))
    return tuple(t)


def coverage_gaps():
    have = {}
    for c in cases():
        have.setdefault(c.kernel, set()).update(c.branches)
    return sorted((k, b) for k, req in REQUIRED.items() for b in req - have.get(k, set()))
