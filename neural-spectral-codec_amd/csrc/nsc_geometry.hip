// nsc_geometry.hip -- stage 2 of loop closing: batched Generalized-ICP verification of cloud pairs.
//
// Reference: GeometricVerifier (src/retrieval/geometric_verification.py:48-203), which calls Open3D 0.18's
// voxel_down_sample, estimate covariances and registration_generalized_icp.  The definitions the kernels follow are
// written out in retrieval/geometric_verification.py and INTEGRATION.md section 2; tests/gicp_restatement.py restates
// them in float64 numpy.
//
// Clouds: cloud c < n_pairs is the source (query) of pair c, cloud n_pairs + c its target.  Rows of a cloud are
// addressed through int64 offsets, so a packed input may hold more than 2^31 floats.
//
// Launch sequence (all on the caller's stream, nothing allocated, copied or synchronised):
//   ds_prepare    (G, C)   clear the cloud's hash slots, per-block min over finite rows, reset pair state
//   ds_insert     (G, C)   voxel key per finite row; insert (64-bit CAS), first row (atomicMin), count and int64
//                          fixed-point coordinate sums -- exact, so independent of arrival order
//   ds_compact    (C)      voxels in first-row order (block scan of "row is its voxel's first"), centroids
//   covariance    (G, C)   exact k-NN over the voxel hash (one point per voxel: rings of voxels with a stopping
//                          bound), covariance, plane regularisation
//   max_iteration + 1 rounds of
//     linearize   (G, P)   nearest target within the radius, per-block float64 slab of the normal equations,
//                          Sum|d|^2, n_corr and the information matrix
//     finalize    (P)      slabs summed in a fixed order, evaluation, convergence test, 6x6 Cholesky, T <- dT T
//
// The store of prepared clouds (NscGicpCloudSet): a cloud's down-sampled points, covariances, min bound and voxel
// index depend on the cloud and on voxel_size, covariance_knn and epsilon only, so nsc_gicp_prepare computes them once
// per cloud and nsc_gicp_register_prepared registers pairs given as indices into one or two stores:
//   prepare:             ds_prepare, ds_insert, ds_compact, covariance as above over a batch of clouds (no pairs),
//                        then store  (C)  offsets after the store's end, rows, covariances, bound, compact index
//   register_prepared:   prepared_setup  (P / 256)  ids -> row ranges and counts, initial transform, pair state
//                        then the max_iteration + 1 rounds of linearize + finalize above
// The results equal nsc_gicp_register's bit for bit: the stored rows are the same values, and a voxel lookup gives the
// same row whatever the capacity of the table it is made in.
//
// No float atomics anywhere: results are bitwise reproducible and independent of what else shares the batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nsc.h"
#include "nsc_eig3.h"                   // jacobi_eig3
#include "nsc_gauss_newton.h"           // gn_solve6, gn_apply
#include "nsc_util.h"
#include "nsc_voxel_hash.h"             // KEY_BITS, KEY_MAX, FIX_SCALE, mix64, pack_key, next_slot

namespace {

constexpr int GEO_BLOCKS = 64;         // blocks per cloud (down-sampling, covariances) and per pair (linearize)
constexpr int GEO_THREADS = 256;
// gridDim.y is at most 65 535.  The per-cloud launches put the cloud in y (2 clouds per pair in nsc_gicp_register),
// the per-pair launches the pair; a larger count is NSC_EUNSUPPORTED before anything is launched, callers chunk.
constexpr int GRID_Y_MAX = 65535;
static_assert(2 * NSC_GICP_MAX_PAIRS <= GRID_Y_MAX && NSC_GICP_MAX_CLOUDS <= GRID_Y_MAX &&
                  NSC_GICP_MAX_PREPARED_PAIRS <= GRID_Y_MAX,
              "the batch limits of include/nsc.h must fit gridDim.y");
constexpr int COMPACT_THREADS = 1024;   // voxel keys count from the cloud's min bound
constexpr int SLAB = 50;                // 21 JtWJ + 6 JtWd + n_corr + Sum|d|^2 + 21 information terms
constexpr int SYS = 29;                 // the first 29 terms: the system of stage output system0

struct Slot {                           // one voxel of a cloud's open-addressing table (2 slots per input row)
    unsigned long long key;             // packed key + 1; 0 = empty
    unsigned long long first;           // smallest input row in the voxel
    unsigned long long count;
    long long sum[3];
    long long ds;                       // row of the voxel in the down-sampled cloud
    long long pad;
};

struct PairState {
    double prev_fitness, prev_rmse;
    int round, done, pad0, pad1;
};

struct Clouds {                         // the 2P clouds of a batch and where each one's data lives
    const float *src, *tgt;
    const long long *src_off, *tgt_off;
    long long total_src;
    int stride, n_pairs;
    // first row of cloud c, its row count, and its position in the combined (source | target) row space that
    // indexes the workspace regions
    __device__ void rows(int c, const float *&first, long long &n, long long &start) const
    {
        if (c < n_pairs) {
            start = src_off[c]; n = src_off[c + 1] - start; first = src + start * stride;
        } else {
            const long long b = tgt_off[c - n_pairs];
            n = tgt_off[c - n_pairs + 1] - b; first = tgt + b * stride; start = total_src + b;
        }
    }
};

__device__ __forceinline__ bool finite3(const float *q) { return isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]); }

__device__ __forceinline__ long long voxel_coord(double p, double lo, double v)
{
    const double k = floor((p - lo) / v);
    return k < 0.0 ? 0 : (k > (double)KEY_MAX ? KEY_MAX : (long long)k);
}

template <class T>
__device__ __forceinline__ unsigned long long voxel_key(const T *p, const double *lo, double voxel)
{
    return pack_key(voxel_coord(p[0], lo[0], voxel), voxel_coord(p[1], lo[1], voxel), voxel_coord(p[2], lo[2], voxel));
}

struct IndexSlot {                      // one voxel of a stored cloud's index (2 slots per down-sampled row)
    unsigned long long key;             // packed key + 1; 0 = empty
    unsigned long long row;             // row of the voxel in the down-sampled cloud
};

__device__ __forceinline__ long long ds_row(const Slot &s) { return s.ds; }
__device__ __forceinline__ long long ds_row(const IndexSlot &s) { return (long long)s.row; }

// Slot of a voxel key in a table of `cap` slots, or -1.
template <class S>
__device__ __forceinline__ long long find_slot(const S *tab, long long cap, unsigned long long key)
{
    if (cap == 0) return -1;
    long long h = (long long)(mix64(key) % (unsigned long long)cap);
    for (long long probe = 0; probe < cap; ++probe) {
        const unsigned long long e = tab[h].key;
        if (e == 0) return -1;
        if (e == key + 1) return h;
        h = next_slot(h, cap);
    }
    return -1;
}

// ------------------------------------------------------------------------------------------------------------------
// down-sampling
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GEO_THREADS) void ds_prepare_kernel(Clouds cl, Slot *slots, double *partial,
                                                                 const double *init, double *transforms,
                                                                 PairState *state)
{
    const int c = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    const float *base; long long n, start;
    cl.rows(c, base, n, start);
    Slot *tab = slots + 2 * start;
    for (long long i = (long long)g * GEO_THREADS + tid; i < 2 * n; i += (long long)GEO_BLOCKS * GEO_THREADS)
        tab[i] = Slot{0ULL, ~0ULL, 0ULL, {0, 0, 0}, -1, 0};
    double mn[3] = {INFINITY, INFINITY, INFINITY};
    for (long long i = (long long)g * GEO_THREADS + tid; i < n; i += (long long)GEO_BLOCKS * GEO_THREADS) {
        const float *q = base + i * cl.stride;
        if (!finite3(q)) continue;
        for (int a = 0; a < 3; ++a) mn[a] = fmin(mn[a], (double)q[a]);
    }
    __shared__ double red[3][GEO_THREADS];
    for (int a = 0; a < 3; ++a) red[a][tid] = mn[a];
    __syncthreads();
    for (int s = GEO_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int a = 0; a < 3; ++a) red[a][tid] = fmin(red[a][tid], red[a][tid + s]);
        __syncthreads();
    }
    if (tid < 3) partial[((long long)c * GEO_BLOCKS + g) * 3 + tid] = red[tid][0];
    if (g == 0 && c < cl.n_pairs) {
        if (tid < 16) transforms[16 * (long long)c + tid] = init[16 * (long long)c + tid];
        if (tid == 0) state[c] = PairState{0.0, 0.0, 0, 0, 0, 0};
    }
}

// min bound of cloud c: min over finite rows minus voxel / 2 (+inf when the cloud has no finite row)
__device__ __forceinline__ void min_bound(const double *partial, int c, double half, double lo[3])
{
    for (int a = 0; a < 3; ++a) {
        double m = INFINITY;
        for (int g = 0; g < GEO_BLOCKS; ++g) m = fmin(m, partial[((long long)c * GEO_BLOCKS + g) * 3 + a]);
        lo[a] = m - half;
    }
}

__global__ __launch_bounds__(GEO_THREADS) void ds_insert_kernel(Clouds cl, Slot *slots, const double *partial,
                                                                double *bound, double voxel)
{
    const int c = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    const float *base; long long n, start;
    cl.rows(c, base, n, start);
    double lo[3];
    min_bound(partial, c, 0.5 * voxel, lo);
    if (g == 0 && tid < 3) bound[4 * c + tid] = lo[tid];
    Slot *tab = slots + 2 * start;
    const long long cap = 2 * n;
    for (long long i = (long long)g * GEO_THREADS + tid; i < n; i += (long long)GEO_BLOCKS * GEO_THREADS) {
        const float *q = base + i * cl.stride;
        if (!finite3(q)) continue;
        const double p[3] = {q[0], q[1], q[2]};
        const unsigned long long key = voxel_key(p, lo, voxel);
        long long h = (long long)(mix64(key) % (unsigned long long)cap);
        for (;;) {                       // at most n distinct keys in 2n slots: an empty slot always exists
            unsigned long long e = tab[h].key;
            if (e == 0) {
                e = atomicCAS(&tab[h].key, 0ULL, key + 1);
                if (e == 0) e = key + 1;
            }
            if (e == key + 1) break;
            h = next_slot(h, cap);
        }
        Slot &s = tab[h];
        atomicMin(&s.first, (unsigned long long)i);
        atomicAdd(&s.count, 1ULL);
        for (int a = 0; a < 3; ++a)      // float32 -> 2^-24 m: exact for |p| >= 0.5 m
            atomicAdd(reinterpret_cast<unsigned long long *>(&s.sum[a]),
                      (unsigned long long)__double2ll_rn(p[a] * FIX_SCALE));
    }
}

__global__ __launch_bounds__(COMPACT_THREADS) void ds_compact_kernel(Clouds cl, Slot *slots, const double *bound,
                                                                     double voxel, double *points, long long *count)
{
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *base; long long n, start;
    cl.rows(c, base, n, start);
    const double lo[3] = {bound[4 * c], bound[4 * c + 1], bound[4 * c + 2]};
    Slot *tab = slots + 2 * start;
    double *out = points + 3 * start;
    __shared__ long long wsum[COMPACT_THREADS / 64];
    long long written = 0;
    for (long long b = 0; b < n; b += COMPACT_THREADS) {
        const long long i = b + tid;
        long long h = -1;
        if (i < n) {
            const float *q = base + i * cl.stride;
            if (finite3(q)) {
                h = find_slot(tab, 2 * n, voxel_key(q, lo, voxel));
                if (h >= 0 && tab[h].first != (unsigned long long)i) h = -1;
            }
        }
        const unsigned long long m = __ballot(h >= 0);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        long long before = written;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        long long total = 0;
        for (int w = 0; w < COMPACT_THREADS / 64; ++w) total += wsum[w];
        if (h >= 0) {
            const long long pos = before + __popcll(m & ((1ULL << lane) - 1ULL));
            Slot &s = tab[h];
            const double cnt = (double)s.count;
            for (int a = 0; a < 3; ++a) out[3 * pos + a] = ((double)s.sum[a] / FIX_SCALE) / cnt;
            s.ds = pos;
        }
        written += total;
        __syncthreads();
    }
    if (tid == 0) count[c] = written;
}

// ------------------------------------------------------------------------------------------------------------------
// covariances
// ------------------------------------------------------------------------------------------------------------------
constexpr int MAX_KNN = NSC_GICP_MAX_KNN;

struct TopK {                            // k smallest (d2, index), ascending; ties to the smaller index
    double d[MAX_KNN];
    long long j[MAX_KNN];
    int n, k;
    __device__ void insert(double d2, long long idx)
    {
        if (n == k && !(d2 < d[k - 1] || (d2 == d[k - 1] && idx < j[k - 1]))) return;
        int p = n < k ? n++ : k - 1;
        while (p > 0 && (d2 < d[p - 1] || (d2 == d[p - 1] && idx < j[p - 1]))) { d[p] = d[p - 1]; j[p] = j[p - 1]; --p; }
        d[p] = d2; j[p] = idx;
    }
};

__device__ __forceinline__ double dist2(const double *a, const double *b)
{
    const double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
    return x * x + y * y + z * z;
}

// eigenvector of the smallest eigenvalue of a symmetric 3x3 (cyclic Jacobi)
__device__ void smallest_eigvec(const double C[6], double u[3])
{
    double A[3][3], V[3][3];
    jacobi_eig3(C, A, V);
    int m = 0;
    for (int a = 1; a < 3; ++a) if (A[a][a] < A[m][m]) m = a;
    for (int a = 0; a < 3; ++a) u[a] = V[a][m];
}

__global__ __launch_bounds__(GEO_THREADS) void covariance_kernel(Clouds cl, const Slot *slots, const double *bound,
                                                                 const long long *count, const double *points,
                                                                 double *cov, double voxel, int knn, double eps)
{
    const int c = blockIdx.y;
    const float *base; long long n, start;
    cl.rows(c, base, n, start);
    const long long m = count[c];
    const Slot *tab = slots + 2 * start;
    const double *P = points + 3 * start;
    const double lo[3] = {bound[4 * c], bound[4 * c + 1], bound[4 * c + 2]};
    const int k = (int)(m < knn ? m : knn);
    for (long long i = (long long)blockIdx.x * GEO_THREADS + threadIdx.x; i < m;
         i += (long long)GEO_BLOCKS * GEO_THREADS) {
        const double *q = P + 3 * i;
        TopK top;
        top.n = 0; top.k = k;
        bool brute = m <= knn;
        if (!brute) {
            long long kc[3];
            for (int a = 0; a < 3; ++a) kc[a] = voxel_coord(q[a], lo[a], voxel);
            for (int r = 0;; ++r) {
                const long long side = 2LL * r + 1;
                if (side * side * side > 2 * m) { brute = true; break; }     // rings cost more than a scan
                for (long long dz = -r; dz <= r; ++dz)
                    for (long long dy = -r; dy <= r; ++dy)
                        for (long long dx = -r; dx <= r; ++dx) {
                            if (llabs(dx) != r && llabs(dy) != r && llabs(dz) != r) continue;   // shell only
                            const long long x = kc[0] + dx, y = kc[1] + dy, z = kc[2] + dz;
                            if (x < 0 || y < 0 || z < 0 || x > KEY_MAX || y > KEY_MAX || z > KEY_MAX) continue;
                            const long long h = find_slot(tab, 2 * n, pack_key(x, y, z));
                            if (h < 0) continue;
                            const long long j = tab[h].ds;
                            top.insert(dist2(q, P + 3 * j), j);
                        }
                // every row not yet seen lies in a voxel >= r+1 rings out: farther than r * voxel (minus rounding)
                const double reach = r * voxel * (1.0 - 1e-9) - 1e-6;
                if (top.n == k && reach > 0.0 && top.d[k - 1] < reach * reach) break;
            }
            if (brute) top.n = 0;
        }
        if (brute)
            for (long long j = 0; j < m; ++j) top.insert(dist2(q, P + 3 * j), j);
        double C[6] = {1, 0, 0, 1, 0, 1};
        if (top.n >= 3) {
            double mu[3] = {0, 0, 0};
            for (int t = 0; t < top.n; ++t)
                for (int a = 0; a < 3; ++a) mu[a] += P[3 * top.j[t] + a];
            for (int a = 0; a < 3; ++a) mu[a] /= top.n;
            for (int e = 0; e < 6; ++e) C[e] = 0.0;
            for (int t = 0; t < top.n; ++t) {
                const double *pt = P + 3 * top.j[t];
                const double x = pt[0] - mu[0], y = pt[1] - mu[1], z = pt[2] - mu[2];
                C[0] += x * x; C[1] += x * y; C[2] += x * z; C[3] += y * y; C[4] += y * z; C[5] += z * z;
            }
            for (int e = 0; e < 6; ++e) C[e] /= top.n;
        }
        double u[3];
        smallest_eigvec(C, u);            // U diag(1,1,eps) U^T = I - (1 - eps) u u^T
        const double f = 1.0 - eps;
        double *o = cov + 6 * (start + i);
        o[0] = 1.0 - f * u[0] * u[0]; o[1] = -f * u[0] * u[1]; o[2] = -f * u[0] * u[2];
        o[3] = 1.0 - f * u[1] * u[1]; o[4] = -f * u[1] * u[2]; o[5] = 1.0 - f * u[2] * u[2];
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Gauss-Newton rounds
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sym_from6(const double *s, double M[3][3])
{
    M[0][0] = s[0]; M[0][1] = M[1][0] = s[1]; M[0][2] = M[2][0] = s[2];
    M[1][1] = s[3]; M[1][2] = M[2][1] = s[4]; M[2][2] = s[5];
}

// acc[0..20] += upper triangle of [[A^T W A, A^T W], [W A, W]], acc[21..26] += [A^T W d; W d] for J = [A | I]
__device__ __forceinline__ void accumulate_jtwj(double *acc, const double A[3][3], const double W[3][3],
                                                const double *d)
{
    double J[3][6];
    for (int r = 0; r < 3; ++r) {
        for (int a = 0; a < 3; ++a) J[r][a] = A[r][a];
        for (int a = 0; a < 3; ++a) J[r][3 + a] = r == a ? 1.0 : 0.0;
    }
    double WJ[3][6];
    for (int r = 0; r < 3; ++r)
        for (int a = 0; a < 6; ++a) WJ[r][a] = W[r][0] * J[0][a] + W[r][1] * J[1][a] + W[r][2] * J[2][a];
    int t = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) acc[t++] += J[0][a] * WJ[0][b] + J[1][a] * WJ[1][b] + J[2][a] * WJ[2][b];
    for (int a = 0; a < 6; ++a) acc[21 + a] += WJ[0][a] * d[0] + WJ[1][a] * d[1] + WJ[2][a] * d[2];
}

// What linearize reads of pair p: the down-sampled source and target rows with their covariances, the target's min
// bound and its voxel table (`cap` slots of type S).
template <class S>
struct PairView {
    const double *S_pts, *S_cov, *T_pts, *T_cov;
    long long ms, mt, cap;
    double lo[3];
    const S *tab;
};

// nsc_gicp_register: both clouds of pair p were prepared in this call's workspace
struct BatchPairs {
    Clouds cl;
    const Slot *slots;
    const double *bound, *points, *cov;
    const long long *count;
    __device__ PairView<Slot> view(int p) const
    {
        const int cs = p, ct = cl.n_pairs + p;
        const float *base; long long ns, ss, nt, st;
        cl.rows(cs, base, ns, ss);
        cl.rows(ct, base, nt, st);
        PairView<Slot> v;
        v.ms = count[cs]; v.mt = count[ct];
        v.tab = slots + 2 * st; v.cap = 2 * nt;
        v.S_pts = points + 3 * ss; v.T_pts = points + 3 * st;
        v.S_cov = cov + 6 * ss; v.T_cov = cov + 6 * st;
        for (int a = 0; a < 3; ++a) v.lo[a] = bound[4 * ct + a];
        return v;
    }
};

// A NscGicpCloudSet as the kernels read it
struct StoreView {
    long long *row_off, *slot_off;
    double *bounds, *points, *cov;
    IndexSlot *slots;
    long long n_clouds;
};

struct PairRows {                       // pair p of nsc_gicp_register_prepared, resolved by prepared_setup_kernel
    long long s_row, t_row, t_slot, t_cap, t_cloud, pad[3];
};

// nsc_gicp_register_prepared: pair p reads two clouds of (possibly different) stores
struct StoredPairs {
    StoreView src, tgt;
    const PairRows *rows;
    const long long *count;
    int n_pairs;
    __device__ PairView<IndexSlot> view(int p) const
    {
        const PairRows r = rows[p];
        PairView<IndexSlot> v;
        v.ms = count[p]; v.mt = count[n_pairs + p];
        v.tab = tgt.slots + r.t_slot; v.cap = r.t_cap;
        v.S_pts = src.points + 3 * r.s_row; v.T_pts = tgt.points + 3 * r.t_row;
        v.S_cov = src.cov + 6 * r.s_row; v.T_cov = tgt.cov + 6 * r.t_row;
        for (int a = 0; a < 3; ++a) v.lo[a] = tgt.bounds[4 * r.t_cloud + a];
        return v;
    }
};

// One body for both entry points: Pairs (BatchPairs or StoredPairs) only says where a pair's clouds live.
template <class Pairs>
__global__ __launch_bounds__(GEO_THREADS) void linearize_kernel(Pairs pairs, const double *transforms,
                                                                const PairState *state, double *slab, double voxel,
                                                                double radius)
{
    const int p = blockIdx.y, tid = threadIdx.x;
    if (state[p].done) return;
    const auto v = pairs.view(p);
    const long long ms = v.ms, mt = v.mt;
    const double *S = v.S_pts, *Tp = v.T_pts, *CS = v.S_cov, *CT = v.T_cov;
    const double lo[3] = {v.lo[0], v.lo[1], v.lo[2]};
    const double *T = transforms + 16 * (long long)p;
    double R[3][3], tr[3];
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) R[a][b] = T[4 * a + b];
        tr[a] = T[4 * a + 3];
    }
    const double r2 = radius * radius;
    long long span = 1;                  // cells per axis the radius can reach
    if (mt > 0) span = (long long)floor(2.0 * radius / voxel) + 2;
    const bool brute = span * span * span > mt;
    double acc[SLAB];
    for (int e = 0; e < SLAB; ++e) acc[e] = 0.0;
    for (long long i = (long long)blockIdx.x * GEO_THREADS + tid; i < ms; i += (long long)GEO_BLOCKS * GEO_THREADS) {
        const double *s = S + 3 * i;
        double q[3];
        for (int a = 0; a < 3; ++a) q[a] = R[a][0] * s[0] + R[a][1] * s[1] + R[a][2] * s[2] + tr[a];
        double best = INFINITY;
        long long bj = -1;
        auto consider = [&](long long j) {
            const double d2 = dist2(q, Tp + 3 * j);
            if (d2 <= r2 && (d2 < best || (d2 == best && j < bj))) { best = d2; bj = j; }
        };
        if (brute) {
            for (long long j = 0; j < mt; ++j) consider(j);
        } else if (mt > 0) {
            long long klo[3], khi[3];
            bool any = true;
            for (int a = 0; a < 3; ++a) {
                const double fl = floor((q[a] - radius - lo[a]) / voxel), fh = floor((q[a] + radius - lo[a]) / voxel);
                if (!(fh >= 0.0) || !(fl <= (double)KEY_MAX)) { any = false; break; }
                klo[a] = fl < 0.0 ? 0 : (long long)fl;
                khi[a] = fh > (double)KEY_MAX ? KEY_MAX : (long long)fh;
            }
            if (any)
                for (long long z = klo[2]; z <= khi[2]; ++z)
                    for (long long y = klo[1]; y <= khi[1]; ++y)
                        for (long long x = klo[0]; x <= khi[0]; ++x) {
                            const long long kk[3] = {x, y, z};
                            double gap = 0.0;                  // distance from q to the cell's box
                            for (int a = 0; a < 3; ++a) {
                                const double c0 = lo[a] + kk[a] * voxel, c1 = c0 + voxel;
                                const double g = q[a] < c0 ? c0 - q[a] : (q[a] > c1 ? q[a] - c1 : 0.0);
                                gap += g * g;
                            }
                            if (gap > r2 * (1.0 + 1e-9) + 1e-12) continue;
                            const long long h = find_slot(v.tab, v.cap, pack_key(x, y, z));
                            if (h >= 0) consider(ds_row(v.tab[h]));
                        }
        }
        if (bj < 0) continue;
        const double *t = Tp + 3 * bj;
        const double d[3] = {q[0] - t[0], q[1] - t[1], q[2] - t[2]};
        double Cs[3][3], Ct[3][3], M[3][3], RC[3][3];
        sym_from6(CS + 6 * i, Cs);
        sym_from6(CT + 6 * bj, Ct);
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) RC[a][b] = R[a][0] * Cs[0][b] + R[a][1] * Cs[1][b] + R[a][2] * Cs[2][b];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) M[a][b] = Ct[a][b] + (RC[a][0] * R[b][0] + RC[a][1] * R[b][1] + RC[a][2] * R[b][2]);
        double W[3][3];                  // M^-1 by cofactors
        W[0][0] = M[1][1] * M[2][2] - M[1][2] * M[2][1];
        W[0][1] = M[0][2] * M[2][1] - M[0][1] * M[2][2];
        W[0][2] = M[0][1] * M[1][2] - M[0][2] * M[1][1];
        W[1][0] = M[1][2] * M[2][0] - M[1][0] * M[2][2];
        W[1][1] = M[0][0] * M[2][2] - M[0][2] * M[2][0];
        W[1][2] = M[0][2] * M[1][0] - M[0][0] * M[1][2];
        W[2][0] = M[1][0] * M[2][1] - M[1][1] * M[2][0];
        W[2][1] = M[0][1] * M[2][0] - M[0][0] * M[2][1];
        W[2][2] = M[0][0] * M[1][1] - M[0][1] * M[1][0];
        const double det = M[0][0] * W[0][0] + M[0][1] * W[1][0] + M[0][2] * W[2][0];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) W[a][b] /= det;
        const double A[3][3] = {{0.0, q[2], -q[1]}, {-q[2], 0.0, q[0]}, {q[1], -q[0], 0.0}};     // -[q]x
        accumulate_jtwj(acc, A, W, d);
        acc[27] += 1.0;
        acc[28] += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        const double B[3][3] = {{0.0, t[2], -t[1]}, {-t[2], 0.0, t[0]}, {t[1], -t[0], 0.0}};     // -[t]x, W = I
        const double I3[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        double info[27];
        for (int e = 0; e < 27; ++e) info[e] = 0.0;
        accumulate_jtwj(info, B, I3, d);
        for (int e = 0; e < 21; ++e) acc[SYS + e] += info[e];
    }
    // fixed-shape reduction: wave butterfly, then the 4 waves in order
    __shared__ double part[GEO_THREADS / 64][SLAB];
    const int lane = tid & 63, wave = tid >> 6;
    for (int e = 0; e < SLAB; ++e) {
        double v = acc[e];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) part[wave][e] = v;
    }
    __syncthreads();
    if (tid < SLAB) {
        double v = part[0][tid];
        for (int w = 1; w < GEO_THREADS / 64; ++w) v += part[w][tid];
        slab[((long long)p * GEO_BLOCKS + blockIdx.x) * SLAB + tid] = v;
    }
}

__global__ __launch_bounds__(64) void finalize_kernel(const long long *count, const double *slab, PairState *state,
                                                      double *transforms, double *fit_rmse, long long *corr_iters,
                                                      double *information, double *system0, int n_pairs,
                                                      int max_iteration, double rel_fitness, double rel_rmse)
{
    const int p = blockIdx.x, tid = threadIdx.x;
    PairState &stt = state[p];
    if (stt.done) return;
    __shared__ double sum[SLAB];
    if (tid < SLAB) {
        double v = 0.0;
        for (int g = 0; g < GEO_BLOCKS; ++g) v += slab[((long long)p * GEO_BLOCKS + g) * SLAB + tid];
        sum[tid] = v;
    }
    __syncthreads();
    const int round = stt.round;
    if (system0 && round == 0 && tid < SYS) system0[(long long)p * SYS + tid] = sum[tid];
    if (tid != 0) return;
    const double nc = sum[27];
    const long long ms = count[p];
    const double fitness = ms > 0 ? nc / (double)ms : 0.0;
    const double rmse = nc > 0.0 ? sqrt(sum[28] / nc) : 0.0;
    bool done = round == max_iteration;
    if (round > 0 && fabs(stt.prev_fitness - fitness) < rel_fitness && fabs(stt.prev_rmse - rmse) < rel_rmse)
        done = true;
    if (done) {
        stt.done = 1;
        fit_rmse[2 * p] = fitness;
        fit_rmse[2 * p + 1] = rmse;
        corr_iters[2 * p] = (long long)nc;
        corr_iters[2 * p + 1] = round;
        double *info = information + 36 * (long long)p;
        int t = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) { info[6 * a + b] = info[6 * b + a] = sum[SYS + t]; ++t; }
        return;
    }
    stt.prev_fitness = fitness;
    stt.prev_rmse = rmse;
    stt.round = round + 1;
    // (sum JtWJ) x = -sum JtWd by Cholesky; dT = I without correspondences or a positive-definite system
    double x[6];
    if (!(nc > 0.0) || !gn_solve6(sum, x)) return;
    gn_apply(x, transforms + 16 * (long long)p);
}

// ------------------------------------------------------------------------------------------------------------------
// the store of prepared clouds
// ------------------------------------------------------------------------------------------------------------------
// One block per cloud c of a prepare batch, after ds_compact and covariance: the cloud's store rows and index slots
// follow the store's end (rows0, slots0) and the batch's earlier clouds (fixed-order sum of count[0..c)).  Writes
// the offsets, the min bound, the down-sampled points and covariances, and the index: 2m slots keyed on the voxel
// keys of the workspace table (the input keys, not keys recomputed from the centroids, which may round into a
// neighbouring voxel).
__global__ __launch_bounds__(COMPACT_THREADS) void store_kernel(Clouds cl, const Slot *slots, const double *bound,
                                                                const long long *count, const double *points,
                                                                const double *cov, StoreView set, long long n0,
                                                                long long rows0, long long slots0)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    __shared__ long long red[COMPACT_THREADS];
    long long acc = 0;
    for (int b = tid; b < c; b += COMPACT_THREADS) acc += count[b];
    red[tid] = acc;
    __syncthreads();
    for (int s = COMPACT_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const long long m = count[c], row = rows0 + red[0], slot = slots0 + 2 * red[0], cap = 2 * m;
    if (tid == 0) {
        set.row_off[n0 + c + 1] = row + m;
        set.slot_off[n0 + c + 1] = slot + cap;
        if (c == 0) { set.row_off[n0] = rows0; set.slot_off[n0] = slots0; }
    }
    if (tid < 4) set.bounds[4 * (n0 + c) + tid] = tid < 3 ? bound[4 * c + tid] : 0.0;
    const float *base; long long n, start;
    cl.rows(c, base, n, start);
    for (long long i = tid; i < 3 * m; i += COMPACT_THREADS) set.points[3 * row + i] = points[3 * start + i];
    for (long long i = tid; i < 6 * m; i += COMPACT_THREADS) set.cov[6 * row + i] = cov[6 * start + i];
    IndexSlot *tab = set.slots + slot;
    for (long long i = tid; i < cap; i += COMPACT_THREADS) tab[i] = IndexSlot{0ULL, 0ULL};
    __threadfence();                     // the cleared slots are in memory before any block-mate's CAS below
    __syncthreads();
    const Slot *ws = slots + 2 * start;
    for (long long i = tid; i < 2 * n; i += COMPACT_THREADS) {
        const unsigned long long e = ws[i].key;
        if (e == 0) continue;
        long long h = (long long)(mix64(e - 1) % (unsigned long long)cap);
        while (atomicCAS(&tab[h].key, 0ULL, e) != 0ULL)      // m distinct keys in 2m slots
            h = next_slot(h, cap);
        tab[h].row = (unsigned long long)ws[i].ds;
    }
}

// One thread per pair of nsc_gicp_register_prepared: resolve the ids into row ranges and counts, copy the initial
// transform, reset the pair state.  A pair with an id outside its store is finished here with NaN outputs,
// n_correspondences -1 and 0 iterations; nothing of either store is read for it.
__global__ __launch_bounds__(GEO_THREADS) void prepared_setup_kernel(StoreView src, StoreView tgt,
                                                                     const long long *source_ids,
                                                                     const long long *target_ids, int n_pairs,
                                                                     const double *init, double *transforms,
                                                                     PairState *state, long long *count,
                                                                     PairRows *rows, double *fit_rmse,
                                                                     long long *corr_iters, double *information,
                                                                     double *system0)
{
    const int p = blockIdx.x * GEO_THREADS + threadIdx.x;
    if (p >= n_pairs) return;
    const long long a = source_ids[p], b = target_ids[p];
    double *T = transforms + 16 * (long long)p;
    if (a < 0 || a >= src.n_clouds || b < 0 || b >= tgt.n_clouds) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (int e = 0; e < 16; ++e) T[e] = nan;
        for (int e = 0; e < 36; ++e) information[36 * (long long)p + e] = nan;
        if (system0)
            for (int e = 0; e < SYS; ++e) system0[(long long)p * SYS + e] = nan;
        fit_rmse[2 * p] = fit_rmse[2 * p + 1] = nan;
        corr_iters[2 * p] = -1;
        corr_iters[2 * p + 1] = 0;
        count[p] = count[n_pairs + p] = 0;
        rows[p] = PairRows{0, 0, 0, 0, 0, {0, 0, 0}};
        state[p] = PairState{0.0, 0.0, 0, 1, 0, 0};
        return;
    }
    const long long s0 = src.row_off[a], t0 = tgt.row_off[b], ts0 = tgt.slot_off[b];
    count[p] = src.row_off[a + 1] - s0;
    count[n_pairs + p] = tgt.row_off[b + 1] - t0;
    rows[p] = PairRows{s0, t0, ts0, tgt.slot_off[b + 1] - ts0, b, {0, 0, 0}};
    for (int e = 0; e < 16; ++e) T[e] = init[16 * (long long)p + e];
    state[p] = PairState{0.0, 0.0, 0, 0, 0, 0};
}

// The workspaces are regions carved in order (Carver, nsc_util.h), each rounded up to 256 bytes; a size query lays out a
// null workspace.

// Per-cloud regions for n_clouds clouds of total_rows input rows in all, and the bytes they take: nsc_gicp_prepare's
// workspace, and the head of nsc_gicp_register's (2 clouds per pair; source rows, then target rows).
struct CloudRegions {
    double *partial, *bound, *points, *cov;
    long long *count;
    Slot *slots;
    size_t total;
};

CloudRegions cloud_regions(void *ws, size_t n_clouds, size_t total_rows)
{
    Carver c = {reinterpret_cast<uintptr_t>(ws), 0};
    CloudRegions r;
    r.partial = c.take<double>(n_clouds * GEO_BLOCKS * 3);
    r.bound = c.take<double>(n_clouds * 4);
    r.count = c.take<long long>(n_clouds);
    r.slots = c.take<Slot>(2 * total_rows);
    r.points = c.take<double>(total_rows * 3);
    r.cov = c.take<double>(total_rows * 6);
    r.total = c.o;
    return r;
}

// Per-pair regions from byte `base` on, and where they end: the tail of nsc_gicp_register's workspace, after its
// cloud regions, and, with count[2P] and rows in front (`stored`), nsc_gicp_register_prepared's workspace.
struct PairRegions {
    long long *count; PairRows *rows;   // of stored pairs only
    double *slab; PairState *state;
    size_t total;
};

PairRegions pair_regions(void *ws, size_t n_pairs, bool stored, size_t base)
{
    Carver c = {reinterpret_cast<uintptr_t>(ws), base};
    PairRegions r;
    r.count = c.take<long long>(stored ? 2 * n_pairs : 0);
    r.rows = c.take<PairRows>(stored ? n_pairs : 0);
    r.slab = c.take<double>(n_pairs * GEO_BLOCKS * SLAB);
    r.state = c.take<PairState>(n_pairs);
    r.total = c.o;
    return r;
}

int check_params(const NscGicpParams *p)
{
    if (!p) return NSC_EINVAL;
    if (!(p->voxel_size > 0.0) || !(p->max_correspondence_distance > 0.0) || !(p->epsilon > 0.0) ||
        !(p->relative_fitness >= 0.0) || !(p->relative_rmse >= 0.0) || p->max_iteration < 0 ||
        !isfinite(p->voxel_size) || !isfinite(p->max_correspondence_distance))
        return NSC_EINVAL;
    if (p->covariance_knn < 1 || p->covariance_knn > NSC_GICP_MAX_KNN) return NSC_EUNSUPPORTED;
    return NSC_OK;
}

inline bool stride_ok(int stride_floats) { return stride_floats == 3 || stride_floats == 4; }

inline bool outputs_ok(const double *init_transforms, const double *transforms, const double *fitness_rmse,
                       const int64_t *corr_iterations, const double *information)
{
    return init_transforms && transforms && fitness_rmse && corr_iterations && information;
}

// a set is usable: its arrays are there, its counts fit its capacities and it was prepared with p's down-sampling
// and covariance parameters
bool set_ok(const NscGicpCloudSet *s, const NscGicpParams *p)
{
    if (!s->row_offsets || !s->slot_offsets || !s->bounds || !s->points || !s->covariances || !s->slots) return false;
    if (s->n_clouds < 0 || s->n_rows < 0 || s->n_slots < 0 || s->n_clouds > s->cap_clouds ||
        s->n_rows > s->cap_rows || s->n_slots > s->cap_slots)
        return false;
    return s->voxel_size == p->voxel_size && s->covariance_knn == p->covariance_knn && s->epsilon == p->epsilon;
}

StoreView store_view(const NscGicpCloudSet *s)
{
    return StoreView{reinterpret_cast<long long *>(s->row_offsets), reinterpret_cast<long long *>(s->slot_offsets),
                     s->bounds, s->points, s->covariances, reinterpret_cast<IndexSlot *>(s->slots),
                     (long long)s->n_clouds};
}

// nsc_gicp_prepare's clouds: every cloud of the batch is a "target" of a batch without pairs: Clouds::rows addresses it
// at offsets[c], and ds_prepare has no pair state to reset
Clouds unpaired_clouds(const float *points, const int64_t *offsets, int stride_floats)
{
    const long long *off = reinterpret_cast<const long long *>(offsets);
    return Clouds{points, points, off, off, 0, stride_floats, 0};
}

// ds_prepare, ds_insert, ds_compact and covariance over n_clouds clouds.  init, transforms and state are the pairs'
// (nsc_gicp_register), or null for clouds without pairs.
void launch_prepare(const Clouds &cl, int n_clouds, const CloudRegions &r, const NscGicpParams *p, const double *init,
                    double *transforms, PairState *state, hipStream_t s)
{
    const dim3 per_cloud(GEO_BLOCKS, n_clouds), threads(GEO_THREADS);
    hipLaunchKernelGGL(ds_prepare_kernel, per_cloud, threads, 0, s, cl, r.slots, r.partial, init, transforms, state);
    hipLaunchKernelGGL(ds_insert_kernel, per_cloud, threads, 0, s, cl, r.slots, r.partial, r.bound, p->voxel_size);
    hipLaunchKernelGGL(ds_compact_kernel, dim3(n_clouds), dim3(COMPACT_THREADS), 0, s, cl, r.slots, r.bound,
                       p->voxel_size, r.points, r.count);
    hipLaunchKernelGGL(covariance_kernel, per_cloud, threads, 0, s, cl, r.slots, r.bound, r.count, r.points, r.cov,
                       p->voxel_size, p->covariance_knn, p->epsilon);
}

// The max_iteration + 1 rounds of linearize + finalize over n_pairs pairs; count[p] is pair p's source row count.
template <class Pairs>
void launch_rounds(const Pairs &pairs, int n_pairs, const long long *count, double *slab, PairState *state,
                   const NscGicpParams *p, double *transforms, double *fitness_rmse, int64_t *corr_iterations,
                   double *information, double *system0, hipStream_t s)
{
    for (int r = 0; r <= p->max_iteration; ++r) {
        hipLaunchKernelGGL(linearize_kernel<Pairs>, dim3(GEO_BLOCKS, n_pairs), dim3(GEO_THREADS), 0, s, pairs,
                           transforms, state, slab, p->voxel_size, p->max_correspondence_distance);
        hipLaunchKernelGGL(finalize_kernel, dim3(n_pairs), dim3(64), 0, s, count, slab, state, transforms,
                           fitness_rmse, reinterpret_cast<long long *>(corr_iterations), information, system0, n_pairs,
                           p->max_iteration, p->relative_fitness, p->relative_rmse);
    }
}

}  // namespace

extern "C" {

void nsc_gicp_default_params(NscGicpParams *p)
{
    if (!p) return;
    p->voxel_size = 0.5;
    p->max_correspondence_distance = 1.0;
    p->relative_fitness = 1e-6;
    p->relative_rmse = 1e-6;
    p->epsilon = 1e-3;
    p->max_iteration = 30;
    p->covariance_knn = 20;
}

size_t nsc_gicp_workspace_bytes(int32_t n_pairs, int64_t total_source_points, int64_t total_target_points)
{
    if (n_pairs < 0 || total_source_points < 0 || total_target_points < 0) return 0;
    const size_t clouds = cloud_regions(nullptr, 2 * (size_t)n_pairs, total_source_points + total_target_points).total;
    return pair_regions(nullptr, n_pairs, false, clouds).total;
}

int nsc_gicp_register(const float *source_points, const int64_t *source_offsets, const float *target_points,
                      const int64_t *target_offsets, int32_t n_pairs, int64_t total_source_points,
                      int64_t total_target_points, int32_t stride_floats, const NscGicpParams *p,
                      const double *init_transforms, double *transforms, double *fitness_rmse,
                      int64_t *corr_iterations, double *information, const NscGicpStages *stages, void *ws,
                      size_t ws_bytes, void *stream)
{
    if (n_pairs < 0 || total_source_points < 0 || total_target_points < 0 || !stride_ok(stride_floats))
        return NSC_EINVAL;
    if (const int st = check_params(p)) return st;
    if (n_pairs > NSC_GICP_MAX_PAIRS) return NSC_EUNSUPPORTED;
    if (n_pairs == 0) return NSC_OK;
    if (!source_offsets || !target_offsets ||
        !outputs_ok(init_transforms, transforms, fitness_rmse, corr_iterations, information))
        return NSC_EINVAL;
    if ((total_source_points > 0 && !source_points) || (total_target_points > 0 && !target_points)) return NSC_EINVAL;
    CloudRegions r = cloud_regions(ws, 2 * (size_t)n_pairs, total_source_points + total_target_points);
    const PairRegions q = pair_regions(ws, n_pairs, false, r.total);
    if (!ws || ws_bytes < q.total) return NSC_EWORKSPACE;
    double *system0 = nullptr;
    if (stages) {                        // stage outputs replace the workspace regions they name
        if (stages->points) r.points = stages->points;
        if (stages->covariances) r.cov = stages->covariances;
        if (stages->counts) r.count = reinterpret_cast<long long *>(stages->counts);
        system0 = stages->system0;
    }
    const Clouds cl{source_points, target_points, reinterpret_cast<const long long *>(source_offsets),
                    reinterpret_cast<const long long *>(target_offsets), (long long)total_source_points,
                    stride_floats, n_pairs};
    hipStream_t s = static_cast<hipStream_t>(stream);
    launch_prepare(cl, 2 * n_pairs, r, p, init_transforms, transforms, q.state, s);
    launch_rounds(BatchPairs{cl, r.slots, r.bound, r.points, r.cov, r.count}, n_pairs, r.count, q.slab, q.state, p,
                  transforms, fitness_rmse, corr_iterations, information, system0, s);
    return launch_status();
}

size_t nsc_gicp_prepare_workspace_bytes(int32_t n_clouds, int64_t total_points)
{
    if (n_clouds < 0 || total_points < 0) return 0;
    return cloud_regions(nullptr, n_clouds, total_points).total;
}

int nsc_gicp_prepare(const float *points, const int64_t *offsets, int32_t n_clouds, int64_t total_points,
                     int32_t stride_floats, const NscGicpParams *p, const NscGicpCloudSet *set, void *ws,
                     size_t ws_bytes, void *stream)
{
    if (n_clouds < 0 || total_points < 0 || !set || !stride_ok(stride_floats)) return NSC_EINVAL;
    if (const int st = check_params(p)) return st;
    if (!set_ok(set, p)) return NSC_EINVAL;
    if (n_clouds > NSC_GICP_MAX_CLOUDS) return NSC_EUNSUPPORTED;
    if (n_clouds == 0) return NSC_OK;
    if (!offsets || (total_points > 0 && !points)) return NSC_EINVAL;
    // room for the batch's upper bound: every input row a voxel of its own
    if ((int64_t)set->n_clouds + n_clouds > set->cap_clouds || set->n_rows > set->cap_rows - total_points ||
        set->n_slots > set->cap_slots - 2 * total_points)
        return NSC_EWORKSPACE;
    const CloudRegions r = cloud_regions(ws, n_clouds, total_points);
    if (!ws || ws_bytes < r.total) return NSC_EWORKSPACE;
    const Clouds cl = unpaired_clouds(points, offsets, stride_floats);
    hipStream_t s = static_cast<hipStream_t>(stream);
    launch_prepare(cl, n_clouds, r, p, nullptr, nullptr, nullptr, s);
    hipLaunchKernelGGL(store_kernel, dim3(n_clouds), dim3(COMPACT_THREADS), 0, s, cl, r.slots, r.bound, r.count,
                       r.points, r.cov, store_view(set), (long long)set->n_clouds, (long long)set->n_rows,
                       (long long)set->n_slots);
    return launch_status();
}

size_t nsc_gicp_register_prepared_workspace_bytes(int32_t n_pairs)
{
    if (n_pairs < 0) return 0;
    return pair_regions(nullptr, n_pairs, true, 0).total;
}

int nsc_gicp_register_prepared(const NscGicpCloudSet *sources, const NscGicpCloudSet *targets,
                               const int64_t *source_ids, const int64_t *target_ids, int32_t n_pairs,
                               const NscGicpParams *p, const double *init_transforms, double *transforms,
                               double *fitness_rmse, int64_t *corr_iterations, double *information, double *system0,
                               void *ws, size_t ws_bytes, void *stream)
{
    if (n_pairs < 0 || !sources || !targets) return NSC_EINVAL;
    if (const int st = check_params(p)) return st;
    if (!set_ok(sources, p) || !set_ok(targets, p)) return NSC_EINVAL;
    if (n_pairs > NSC_GICP_MAX_PREPARED_PAIRS) return NSC_EUNSUPPORTED;
    if (n_pairs == 0) return NSC_OK;
    if (!source_ids || !target_ids ||
        !outputs_ok(init_transforms, transforms, fitness_rmse, corr_iterations, information))
        return NSC_EINVAL;
    const PairRegions q = pair_regions(ws, n_pairs, true, 0);
    if (!ws || ws_bytes < q.total) return NSC_EWORKSPACE;
    const StoredPairs pairs{store_view(sources), store_view(targets), q.rows, q.count, n_pairs};
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(prepared_setup_kernel, dim3((n_pairs + GEO_THREADS - 1) / GEO_THREADS), dim3(GEO_THREADS), 0, s,
                       pairs.src, pairs.tgt, reinterpret_cast<const long long *>(source_ids),
                       reinterpret_cast<const long long *>(target_ids), n_pairs, init_transforms, transforms, q.state,
                       q.count, q.rows, fitness_rmse, reinterpret_cast<long long *>(corr_iterations), information,
                       system0);
    launch_rounds(pairs, n_pairs, q.count, q.slab, q.state, p, transforms, fitness_rmse, corr_iterations, information,
                  system0, s);
    return launch_status();
}

}  // extern "C"
