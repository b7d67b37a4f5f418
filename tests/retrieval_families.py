"""Seeded input families and plain references for the stage-1 retrieval kernels (csrc/nsc_retrieval.hip): the W1
distance kernels, the top-k selection, the triplet miner and the recall helpers.  CPU only.

The dyadic argument.  A histogram of non-negative integers whose row sum is exactly 2^k (k <= 12, D <= 1024) makes
every quantity of the W1 pipeline a multiple of 2^-k that fits in float32's 24 bits: h / sum and h / (sum + 1e-8f)
are the same exact value (2^k + 1e-8 rounds to 2^k), every CDF entry is j / 2^k with j <= 2^k, and every partial sum
of at most 1024 |differences| is a multiple of 2^-k below 2^10.  No rounding happens anywhere, so the result does not
depend on the summation order and every kernel must return the exact rational W1 BIT FOR BIT: ``w1_exact``.  A
zero-sum row stays unnormalised (its CDF is 0), so its distance to a normalised row is that row's CDF sum, to which the
last bin contributes exactly 1: a kernel that drops the tail bin is off by one there.

tests/test_retrieval_families_cpu.py checks these references against oracle/retrieval_oracle.py and ``path_of``
against the constants of the .hip source; tests/test_retrieval_paths_gpu.py runs the families on the device."""
import re
from types import SimpleNamespace

import numpy as np

import miner_oracle as mo

# ---- the dispatch constants of csrc/nsc_retrieval.hip and csrc/nsc_w1_rows.h, restated (test_retrieval_families_cpu.py
# parses the sources) ----
TK_CHUNK = 2048            # distances per top-k stage-1 workgroup
TK_MAX_K = 256             # k beyond this: stable device sort
TK_MAX_CAND = 4096         # chunks * k beyond this: stable device sort
TL_I = 64                  # database rows per tile-kernel workgroup
STREAM_WG_CAP = 256 * 8    # workgroups of the stream kernel; 4 waves each
WAVES_PER_WG = 4

# the shapes of tests/test_retrieval_paths_gpu.py; tests/test_retrieval_families_cpu.py checks the claims about them
CDF_D = (1, 3, 4, 51, 256, 257, 512, 513, 768, 769, 801, 1023, 1024)
CDF_N = (1, 3, 4, 5)
STREAM_Q, STREAM_D, STREAM_N = (1, 2, 3, 4), (4, 52, 800, 1024), (1, 5, 8191, 8192, 8193, 20011)
TILE_Q, TILE_D, TILE_N = (5, 16, 17, 32, 33, 64, 65, 96, 97, 130), (4, 36, 52, 800, 1024), (1, 63, 64, 65, 257)
TILE_INST = {5: 1, 16: 1, 17: 2, 32: 2, 33: 4, 64: 4, 65: 2, 96: 2, 97: 4, 130: 4}
TOPK_K, TOPK_N = (1, 7, 64, 255, 256), ("k", 2047, 2048, 2049, 2050, 32768)
K_OF_D = {1: 6, 3: 6, 4: 6}                                   # 2^k of mass per row; 10 unless D is tiny


def k_of(D):
    return K_OF_D.get(D, 10)


def per_of(D):
    """bins per lane of w1_cdf_kernel / w1_dist_kernel: 4, 8, 12 or 16"""
    return max(4, ((D + 63) // 64 + 3) // 4 * 4)


def path_of(N, Q, D):
    """Which kernel instance serves (N rows, Q queries, D bins) and how far its loops go.
    per: PER of nsc_w1_cdf / nsc_w1_distances.  For nsc_w1_distances_cdf (D % 4 == 0): kernel 'stream' (Q <= 4) with
    its QT, its wave count and ``trips`` = the most rows one wave walks; or 'tile' with NQ and its grid."""
    p = SimpleNamespace(per=per_of(D), cached=(D >= 4 and D % 4 == 0), kernel=None, inst=None, chunks=-(-N // TK_CHUNK))
    if not p.cached:
        return p
    if Q <= 4:
        wgs = min(-(-N // WAVES_PER_WG), STREAM_WG_CAP)
        p.kernel, p.inst = "stream", (1 if Q == 1 else 2 if Q == 2 else 4)
        p.waves = wgs * WAVES_PER_WG
        p.trips = -(-N // p.waves) if N else 0
    else:
        nq = 1 if Q <= 16 else (2 if (Q <= 32 or 64 < Q <= 96) else 4)
        p.kernel, p.inst = "tile", nq
        p.grid = (-(-N // TL_I), -(-Q // (16 * nq)))
        p.partial_rows = N % TL_I != 0
        p.scalar_store = N % 4 != 0                  # a row of dist that is not 16-byte aligned, or a ragged tail
    return p


def topk_path(N, k):
    """'kernel' (two-stage selection) or 'sort' (torch.sort fallback of wasserstein._topk), and the chunk count"""
    chunks = -(-N // TK_CHUNK)
    kern = k <= TK_MAX_K and chunks * k <= TK_MAX_CAND
    return SimpleNamespace(path="kernel" if kern else "sort", chunks=chunks, last=N - (chunks - 1) * TK_CHUNK)


def parse_constants(src, shared):
    """the same constants read out of the .hip text and, for what both W1 files share, csrc/nsc_w1_rows.h"""
    def one(pat, text=src):
        m = re.search(pat, text)
        assert m, pat
        return m
    out = {"TK_CHUNK": int(one(r"constexpr int TK_CHUNK = (\d+)").group(1)),
           "TL_I": int(one(r"constexpr int TL_I = (\d+)", shared).group(1)),
           "per_of": one(r"int per_of\(int D\) \{(.*?)\}").group(1).strip()}
    m = one(r"constexpr int W1_STREAM_WG_CAP = (\d+) \* (\d+);", shared)
    one(r"int w1_stream_workgroups\(int N\) \{ const int wgs = \(N \+ 3\) / 4; "
        r"return wgs < W1_STREAM_WG_CAP \? wgs : W1_STREAM_WG_CAP; \}", shared)
    one(r"const dim3 grid\(w1_stream_workgroups\(N\)\)")
    out["STREAM_WG_CAP"] = int(m.group(1)) * int(m.group(2))
    m = one(r"if \(k > (\d+) \|\| \(long long\)chunks \* k > (\d+)\) return NSC_EUNSUPPORTED;")
    out["TK_MAX_K"], out["TK_MAX_CAND"] = int(m.group(1)), int(m.group(2))
    out["nq"] = one(r"int w1_tile_nq\(int Q\) \{ return (.*?); \}", shared).group(1).strip()
    one(r"const int nq = w1_tile_nq\(Q\);", shared)
    one(r"if \(Q <= W1_STREAM_MAX_Q\) \{\s*const dim3 grid\(w1_stream_workgroups\(N\)\)")
    out["stream_split"] = one(r"constexpr int W1_STREAM_MAX_Q = (\d+);", shared).group(1)
    return out


# ---- dyadic histograms -------------------------------------------------------------------------------------------
def dyadic_hists(n, D, k, seed, dups=None, plant=True):
    """(n, D) int64 multinomial rows with sum 2^k.  Planted when n >= 6 (``plant``): row 1 is zero, row n - 1 has all its
    mass in bin D - 1, row n - 2 all in bin 0, and ``dups`` (default ((0, n // 2),)) copies row a over row b."""
    rng = np.random.default_rng([seed, n, D, k])
    h = rng.multinomial(2 ** k, np.full(D, 1.0 / D), size=n).astype(np.int64)
    if plant and n >= 6:
        h[1] = 0
        h[n - 1] = 0
        h[n - 1, D - 1] = 2 ** k
        h[n - 2] = 0
        h[n - 2, 0] = 2 ** k
        for a, b in (((0, n // 2),) if dups is None else dups):
            h[b] = h[a]
    assert ((h.sum(1) == 2 ** k) | (h.sum(1) == 0)).all() and (h >= 0).all()
    return h


def w1_exact(q, db, k):
    """(Q, N) float32: the exact W1 of dyadic rows, abs(cumsum(a) - cumsum(b)).sum() / 2^k in int64.  A zero row's CDF
    is 0 on both sides of the pipeline (it stays unnormalised), which the integer form gives without a special case
    because every other row has the same sum 2^k."""
    q, db = np.atleast_2d(np.asarray(q)), np.atleast_2d(np.asarray(db))
    assert q.dtype.kind == "i" and db.dtype.kind == "i" and k <= 12 and db.shape[1] <= 1024
    for h in (q, db):
        s = h.sum(1)
        assert ((s == 2 ** k) | (s == 0)).all()
    cq, cd = np.cumsum(q, 1, dtype=np.int64), np.cumsum(db, 1, dtype=np.int64)
    out = np.empty((len(q), len(db)), np.int64)
    for i in range(len(q)):
        out[i] = np.abs(cd - cq[i]).sum(1)
    assert out.max(initial=0) < 2 ** 24                       # fits float32 exactly
    return (out / 2.0 ** k).astype(np.float32)


def cdf_exact(h, k):
    """(n, D) float32 CDF rows of dyadic histograms, exact"""
    return (np.cumsum(np.asarray(h, np.int64), 1) / 2.0 ** k).astype(np.float32)


def w1_f64(q, db, eps=1e-8, divide_plain=True):
    """float64 restatement of wasserstein.py:134-172 (divide_plain: the query is h / sum) and :232-273 (both sides
    h / (sum + eps)) for general float32 inputs: (Q, N) float64."""
    q = np.atleast_2d(np.asarray(q, np.float32)).astype(np.float64)
    db = np.atleast_2d(np.asarray(db, np.float32)).astype(np.float64)
    qs, ds = q.sum(1, keepdims=True), db.sum(1, keepdims=True)
    q = np.where(qs > eps, q / (qs if divide_plain else qs + eps), q)
    db = np.where(ds > eps, db / (ds + eps), db)
    cq, cd = np.cumsum(q, 1), np.cumsum(db, 1)
    out = np.empty((len(q), len(db)))
    for i in range(len(q)):
        out[i] = np.abs(cd - cq[i]).sum(1)
    return out


def filter_mask(pos, qpos, min_dist):
    """(Q, N) bool, True where the spatial filter excludes the pair (two_stage_retrieval.py:160-170): translation
    distance strictly below min_dist.  float64 on the float32-rounded inputs; with integer positions every term is
    exact, so the only distances within an ulp of a threshold are the ones the test plants on it."""
    p = np.asarray(pos, np.float32).astype(np.float64).reshape(-1, 3)
    qp = np.asarray(qpos, np.float32).astype(np.float64).reshape(-1, 3)
    d = np.sqrt(((p[None, :, :] - qp[:, None, :]) ** 2).sum(-1))
    return d < float(np.float32(min_dist))


def topk_lex(d, k):
    """k smallest of each row under (value, index), ascending.  A NaN is never selected: slots beyond the row's
    non-NaN entries hold index -1 and value +inf (what nsc_topk_smallest gives).  -> ((Q, k) int64, (Q, k) float32)"""
    d = np.atleast_2d(np.asarray(d, np.float32))
    Q, N = d.shape
    idx = np.full((Q, k), -1, np.int64)
    val = np.full((Q, k), np.inf, np.float32)
    for r in range(Q):
        ok = np.nonzero(~np.isnan(d[r]))[0]
        o = ok[np.lexsort((ok, d[r][ok]))][:k]
        idx[r, :len(o)], val[r, :len(o)] = o, d[r][o]
    return idx, val


# ---- rounding-sensitive rows (general float32; compared with w1_f64 under a derived tolerance) -----------------------
def rounding_rows(family, n, D, seed):
    rng = np.random.default_rng([seed, D, {"counts": 1, "cubed": 2, "sparse": 3}[family]])
    if family == "counts":                                    # count-like: mean 2 500 per bin
        return rng.poisson(2500.0, (n, D)).astype(np.float32)
    if family == "cubed":
        return (rng.random((n, D)) ** 3).astype(np.float32)
    h = np.where(rng.random((n, D)) < 0.02, rng.random((n, D)), 0.0).astype(np.float32)      # 2 % of the bins occupied
    h[:, 0] += (h.sum(1) == 0)                                # no empty row in this family
    return h


SUITE_TOL = (1e-4, 1e-5)                                      # the suite's rtol, atol


def oracle_tolerance(ref64, oracle32):
    """item 5's bound per element: the larger of the suite's 1e-4 |d| + 1e-5 and 2 x the float32 oracle's own worst
    deviation from float64 for the SAME QUERY over these rows (kernel and oracle each carry their own summation order;
    the maximum is taken per query, not over the whole block, so that one bad query does not loosen the others).
    -> ((Q, N) tol array, the oracle's worst ratio to the suite bound)"""
    suite = SUITE_TOL[0] * np.abs(ref64) + SUITE_TOL[1]
    dev = np.abs(oracle32.astype(np.float64) - ref64)
    return np.maximum(suite, 2.0 * dev.max(axis=1, keepdims=True)), float((dev / suite).max())


# ---- miner ---------------------------------------------------------------------------------------------------------
MINE_DEFAULTS = dict(pmax=5.0, ptmin=30, nmin=10.0, nmax=50.0, ntmin=30)


def mine_reference(desc_int, k, positions, **kw):
    """Per anchor of one sequence: dict(pos, neg, w1 (exact float32, one per negative), hard, semi) -- hard = lowest
    index among the smallest W1, semi = rank len // 2 under (value, index); None for both when the anchor has no
    positive or no negative.  Candidate sets are miner_oracle.candidates (inclusive radii, float64)."""
    P = dict(MINE_DEFAULTS, **kw)
    positions = np.asarray(positions, np.float64)
    out = []
    for la in range(len(positions)):
        pos, neg = mo.candidates(positions, la, **P)
        r = SimpleNamespace(pos=pos, neg=neg, w1=None, hard=None, semi=None)
        if len(pos) and len(neg):
            r.w1 = w1_exact(desc_int[la], desc_int[neg], k)[0]
            order = neg[np.lexsort((neg, r.w1))]
            r.hard, r.semi = int(order[0]), int(order[len(neg) // 2])
        out.append(r)
    return out


# ---- recall helpers ------------------------------------------------------------------------------------------------
def pairwise_l2_reference(emb, qidx, skip):
    """(Q, n) float32: |e_q - e_c|_2 in float64 rounded once, +inf exactly where |c - q| <= skip"""
    e = np.asarray(emb, np.float32).astype(np.float64)
    q = np.asarray(qidx, np.int64)
    d = np.sqrt(((e[q][:, None, :] - e[None, :, :]) ** 2).sum(-1)).astype(np.float32)
    band = np.abs(np.arange(len(e))[None, :] - q[:, None]) <= skip
    d[band] = np.inf
    return d, band


def revisit_reference(pos, skip, thr):
    """first j >= i + skip with |p_i - p_j| < thr (strict), -1 if none (trainer.py:342-348): (n,) int32"""
    p = np.asarray(pos, np.float64)
    out = np.full(len(p), -1, np.int32)
    for i in range(len(p)):
        d = np.sqrt(((p[i + skip:] - p[i]) ** 2).sum(1))
        hit = np.nonzero(d < thr)[0]
        if len(hit):
            out[i] = i + skip + hit[0]
    return out


def recall_rank_reference(pos, qidx, topk_idx, thr):
    """1-based position of the first of each row's candidates within thr (strict) of its query, 0 if none; a -1 ends
    the row"""
    p = np.asarray(pos, np.float64)
    out = np.zeros(len(qidx), np.int32)
    for r, q in enumerate(qidx):
        for t, c in enumerate(topk_idx[r]):
            if c < 0:
                break
            if np.sqrt(((p[c] - p[q]) ** 2).sum()) < thr:
                out[r] = t + 1
                break
    return out
