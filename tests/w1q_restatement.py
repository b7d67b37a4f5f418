"""Restatement of stage 1 over quantised descriptors (csrc/nsc_retrieval_q.hip) in float-free numpy,
its seeded input families and the dispatch of nsc_w1q_distances.  CPU only.

Definitions.  ``quantized`` is (n, D) uint16, 1 <= D <= 1024.  A row is *canonical* iff its bins sum to exactly 65535,
the sum taken in 64 bits (a row summing to 131 071 has the low 16 bits of a canonical one and is not).  The CDF of a
canonical row is its running sum, which fits uint16 entry by entry; any other row has a CDF of zeros.
``d_int(a, b) = sum_k |cdf_a[k] - cdf_b[k]|`` is an integer below 2^26, so nothing about the way a kernel sums it can
show: every comparison with these functions is bit for bit.  The only floating-point steps are the final
``float32(d_int) / float32(65535)`` (one conversion, round to nearest even, and one IEEE division) and the spatial
filter, which is float32 by definition (the expression of w1_stream_kernel)."""
import re
from types import SimpleNamespace

import numpy as np

TOTAL = 65535

# ---- the dispatch constants of csrc/nsc_retrieval_q.hip and csrc/nsc_w1_rows.h, restated (tests/test_w1q_cpu.py parses
# the sources) ----
QTL_I = 64                 # database rows per tile-kernel workgroup (TL_I)
QTL_KP = 32                # k-pairs (64 bins) per staged chunk (TL_K words of two bins)
STREAM_WG_CAP = 256 * 8    # workgroups of the stream kernel; 4 waves each
WAVES_PER_WG = 4
PACK = 8                   # the packed kernels need D % 8 == 0 (16-byte chunks) and 16-byte aligned bases

CDF_D, CDF_N = (1, 3, 8, 50, 56, 800, 1023, 1024), (1, 3, 4, 5)
STREAM_Q, STREAM_D = (1, 2, 3, 4), (8, 56, 800, 1024)
TILE_Q, TILE_D = (5, 16, 17, 32, 33, 64, 65, 130), (8, 40, 56, 800, 1024)
TILE_INST = {5: 1, 16: 1, 17: 2, 32: 2, 33: 4, 64: 4, 65: 2, 130: 4}
GENERIC_D, GENERIC_Q, GENERIC_N = (1, 3, 50, 801, 1023), (1, 5), (1, 5, 257)


def path_of(N, Q, D, aligned=True):
    """Which kernel of nsc_w1q_distances serves (N rows, Q queries, D bins): 'generic', or with D % 8 == 0 and
    16-byte aligned bases 'stream' (Q <= 4; its QT, its wave count and ``trips`` = the most rows one wave walks) or
    'tile' (its NQ and grid)."""
    p = SimpleNamespace(kernel="generic", inst=None, packed=(D % PACK == 0 and aligned))
    if not p.packed:
        p.grid = (-(-N // WAVES_PER_WG),)
        return p
    if Q <= 4:
        wgs = min(-(-N // WAVES_PER_WG), STREAM_WG_CAP)
        p.kernel, p.inst = "stream", (1 if Q == 1 else 2 if Q == 2 else 4)
        p.waves = wgs * WAVES_PER_WG
        p.trips = -(-N // p.waves) if N else 0
    else:
        nq = 1 if Q <= 16 else (2 if (Q <= 32 or 64 < Q <= 96) else 4)
        p.kernel, p.inst = "tile", nq
        p.grid = (-(-N // QTL_I), -(-Q // (16 * nq)))
        p.partial_rows = N % QTL_I != 0
        p.chunks = -(-(D // 2) // QTL_KP)
    return p


def stream_boundary():
    """The largest N at which every wave of the stream kernel walks one row; one more and wave 0 walks two."""
    return STREAM_WG_CAP * WAVES_PER_WG


def stream_n():
    b = stream_boundary()
    return (1, 5, b - 1, b, b + 1, 20011)                       # 20 011 is prime


def tile_n():
    return (1, QTL_I - 1, QTL_I, QTL_I + 1, 257)


def parse_constants(src, shared):
    """the same constants read out of the .hip text and, for what both W1 files share, csrc/nsc_w1_rows.h"""
    def one(pat, text=src):
        m = re.search(pat, text)
        assert m, pat
        return m
    m = one(r"constexpr int TL_I = (\d+), TL_K = (\d+)", shared)
    out = {"QTL_I": int(m.group(1)), "QTL_KP": int(m.group(2))}
    one(r"static __device__ __forceinline__ int words\(int D\) \{ return D >> 1; \}", shared)     # a word is a k-pair
    m = one(r"constexpr int W1_STREAM_WG_CAP = (\d+) \* (\d+);", shared)
    one(r"int w1_stream_workgroups\(int N\) \{ const int wgs = \(N \+ 3\) / 4; "
        r"return wgs < W1_STREAM_WG_CAP \? wgs : W1_STREAM_WG_CAP; \}", shared)
    out["STREAM_WG_CAP"] = int(m.group(1)) * int(m.group(2))
    out["qnq"] = one(r"int w1_tile_nq\(int Q\) \{ return (.*?); \}", shared).group(1).strip()
    one(r"const int nq = w1_tile_nq\(Q\);", shared)
    one(r"else if \(Q <= W1_STREAM_MAX_Q\) \{\s*const dim3 grid\(w1_stream_workgroups\(N\)\)")
    out["stream_split"] = one(r"constexpr int W1_STREAM_MAX_Q = (\d+);", shared).group(1)
    out["packed"] = one(r"const bool packed = (.*?);").group(1).strip()
    return out


# ---- definitions ---------------------------------------------------------------------------------------------------
def canonical(quantized):
    """(n,) uint8: 1 where the row sums to exactly 65535"""
    q = np.atleast_2d(np.asarray(quantized))
    assert q.dtype == np.uint16 and 1 <= q.shape[1] <= 1024
    return (q.sum(1, dtype=np.int64) == TOTAL).astype(np.uint8)


def cdf(quantized):
    """-> (cdf (n, D) uint16, canonical (n,) uint8)"""
    q = np.atleast_2d(np.asarray(quantized))
    ok = canonical(q)
    c = np.cumsum(q, 1, dtype=np.int64)
    c[ok == 0] = 0
    assert c.max(initial=0) <= TOTAL
    return c.astype(np.uint16), ok


def d_int(q_cdf, db_cdf):
    """(Q, N) uint32 integer distances of CDF rows"""
    cq, cd = np.atleast_2d(q_cdf).astype(np.int32), np.atleast_2d(db_cdf).astype(np.int32)
    out = np.empty((len(cq), len(cd)), np.int64)
    for i in range(len(cq)):
        out[i] = np.abs(cd - cq[i]).sum(1, dtype=np.int64)
    assert out.max(initial=0) < 2 ** 26
    return out.astype(np.uint32)


def filter_mask(db_pos, q_pos, min_dist):
    """(Q, N) bool, True where the spatial filter excludes the pair: sqrtf(dx*dx + dy*dy + dz*dz) < min_dist with every
    operation rounded to float32, as the kernels write it."""
    p = np.asarray(db_pos, np.float32).reshape(-1, 3)
    q = np.asarray(q_pos, np.float32).reshape(-1, 3)
    d = p[None, :, :] - q[:, None, :]
    s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert s.dtype == np.float32
    return np.sqrt(s) < np.float32(min_dist)


def dist(q_quantized, db_quantized, db_pos=None, q_pos=None, min_dist=0.0):
    """(Q, N) float32 distances of quantised rows under the definition"""
    cq, okq = cdf(q_quantized)
    cd, okd = cdf(db_quantized)
    out = d_int(cq, cd).astype(np.float32) / np.float32(TOTAL)
    out[:, okd == 0] = np.inf
    out[okq == 0, :] = np.inf
    if db_pos is not None and q_pos is not None:
        out[filter_mask(db_pos, q_pos, min_dist)] = np.inf
    return out


def topk(d, k):
    """k smallest of each row under (value, index), ascending; slots no finite distance fills hold -1 / +inf (what
    CompressedRetriever.query_batch returns).  -> ((Q, k) int64, (Q, k) float32)"""
    d = np.atleast_2d(np.asarray(d, np.float32))
    idx = np.full((len(d), k), -1, np.int64)
    val = np.full((len(d), k), np.inf, np.float32)
    for r in range(len(d)):
        ok = np.nonzero(np.isfinite(d[r]))[0]
        o = ok[np.lexsort((ok, d[r][ok]))][:k]
        idx[r, :len(o)], val[r, :len(o)] = o, d[r][o]
    return idx, val


# ---- input families (integers only) --------------------------------------------------------------------------------
def canonical_rows(n, D, seed):
    """(n, D) uint16 canonical rows: the gaps between D - 1 sorted cut points of [0, 65535].  Every third row keeps its
    cuts inside a narrow window (mass concentrated in few bins, long flat stretches of the CDF)."""
    rng = np.random.default_rng([seed, n, D])
    cuts = rng.integers(0, TOTAL + 1, (n, D - 1))
    if D > 1:
        lo = rng.integers(0, TOTAL - 255, n)
        narrow = lo[:, None] + rng.integers(0, 256, (n, D - 1))
        cuts[::3] = narrow[::3]
    cuts.sort(axis=1)
    edges = np.concatenate([np.zeros((n, 1), np.int64), cuts, np.full((n, 1), TOTAL, np.int64)], 1)
    q = np.diff(edges, axis=1)
    assert q.shape == (n, D) and (q >= 0).all() and (q.sum(1) == TOTAL).all()
    return q.astype(np.uint16)


def one_hot(D, k):
    q = np.zeros(D, np.uint16)
    q[k] = TOTAL
    return q


def edge_rows(D, seed=0):
    """Rows around the definition of canonical, as a dict name -> (D,) uint16; a case D cannot express is left out
    (one bin cannot sum to 65536, two cannot sum to 131 071)."""
    base = canonical_rows(1, D, seed + 77)[0]
    top = int(base.argmax())
    rows = {"random": base, "zero": np.zeros(D, np.uint16), "first": one_hot(D, 0), "last": one_hot(D, D - 1),
            "all_max": np.full(D, TOTAL, np.uint16)}
    minus = base.copy()
    minus[top] -= 1                                             # the largest bin holds at least 65535 / D >= 63
    rows["sum_65534"] = minus
    if D >= 2:
        plus = base.copy()
        other = top if base[top] < TOTAL else (top + 1) % D
        plus[other] += 1
        rows["sum_65536"] = plus
    if D >= 3:
        wrap = np.zeros(D, np.uint16)
        wrap[0], wrap[D // 2], wrap[D - 1] = TOTAL, TOTAL, 1    # 131 071 = 0x1ffff
        rows["sum_131071"] = wrap
    return rows


def int_positions(n, seed, lo=-20, hi=21):
    return np.random.default_rng([seed, n, 3]).integers(lo, hi, (n, 3)).astype(np.float32)
