// nsc_localize.hip -- scans registered against the distribution map of nsc_map_build_dist (nsc_map_register; the
// definition is in include/nsc.h, tests/map_localize_restatement.py restates it in float64 numpy).  Point to distribution
// Gauss-Newton: a row's correspondence is the voxel its transformed point falls into, found by the row's key in the map's
// kept index, so there is no neighbour search.
//
// Launch sequence (all on the caller's stream, nothing allocated, copied or synchronised):
//   setup      (S / 256)   initial transform, row count and state of every scan; a scan with a non-finite initial
//                          transform is finished here with NaN outputs
//   then max_iteration + 1 rounds of
//   linearize  (64 x S)    one row per lane per sweep: T p, key, probe of the index (16 bytes per probe), one 128-byte
//                          record, the row's 30 terms into registers; per workgroup a slab of 30 float64, reduced by wave
//                          butterfly and then the four waves in order
//   finalize   (S)         slabs summed in block order, convergence test, 6x6 Cholesky, T <- dT T
// The round structure, the reduction and the update are those of nsc_geometry.hip's linearize_kernel and finalize_kernel.
//
// nsc_map_register_robust runs the same sequence.  With a robust kernel every (row, voxel) pair is weighted by
// w = rho'(d^T Omega d) (nsc_robust.h); with seven voxels a row pairs with its own voxel and the six face neighbours, probed
// in a runtime loop in the fixed order (0, -x, +x, -y, +y, -z, +z).  Those rounds keep 32 sums per workgroup (the 30, then
// sum w and the number of pairs).  linearize_rows is the one body: loc_linearize_kernel runs it with one voxel and no
// kernel over 30 sums, loc_linearize_robust_kernel with everything else over 32.
//
// No float atomics anywhere: results are bitwise reproducible and independent of what else shares the batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nsc.h"
#include "nsc_gauss_newton.h"           // gn_solve6, gn_apply
#include "nsc_robust.h"                 // robust_rho_w
#include "nsc_util.h"
#include "nsc_voxel_hash.h"             // MapGrid, place_row, world_voxel, mix64, next_slot

namespace {

constexpr int LOC_BLOCKS = NSC_MAP_REGISTER_BLOCKS;
constexpr int LOC_THREADS = 256;
constexpr int SLAB = NSC_MAP_REGISTER_SYSTEM;       // 21 JtOJ + 6 JtOd + n_corr + sum |d|^2 + sum dtOd
constexpr int N_CORR = 27, SUM_D2 = 28, COST = 29;
constexpr int WIDE = NSC_MAP_REGISTER_ROBUST_SYSTEM;        // the 30 sums, then sum w and n_pairs
constexpr int W_SUM = 30, N_PAIRS = 31;
constexpr int REC = NSC_MAP_VOXEL_DOUBLES;
static_assert(SLAB == 30 && WIDE == 32 && WIDE <= 64, "finalize sums one slab entry per lane of a wave");

typedef unsigned long long u64;

struct ScanState {
    double prev_fitness, prev_rmse;
    int round, done, pad0, pad1;
};

struct MapView {                        // what nsc_map_build_dist kept
    const double *voxels;
    const ulonglong2 *index;            // (key + 1, place)
    long long cap;
    MapGrid g;
};

__global__ __launch_bounds__(LOC_THREADS) void loc_setup_kernel(const long long *off, int n_scans, long long total,
                                                                const double *init,
                                                                double *transforms, ScanState *state, long long *count,
                                                                double *fit_rmse, double *cost, long long *corr_iters,
                                                                double *information, double *system0, int sys_width,
                                                                double *weight_pairs)
{
    const int p = blockIdx.x * LOC_THREADS + threadIdx.x;
    if (p >= n_scans) return;
    double *T = transforms + 16 * (long long)p;
    const double *T0 = init + 16 * (long long)p;
    bool finite = true;
    for (int e = 0; e < 16; ++e) finite = finite && isfinite(T0[e]);
    if (!finite) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (int e = 0; e < 16; ++e) T[e] = nan;
        for (int e = 0; e < 36; ++e) information[36 * (long long)p + e] = nan;
        if (system0)
            for (int e = 0; e < sys_width; ++e) system0[(long long)p * sys_width + e] = nan;
        if (weight_pairs) {
            weight_pairs[2 * p] = nan;
            weight_pairs[2 * p + 1] = -1.0;                          // as n_corr
        }
        fit_rmse[2 * p] = fit_rmse[2 * p + 1] = cost[p] = nan;
        corr_iters[2 * p] = -1;
        corr_iters[2 * p + 1] = 0;
        count[p] = 0;
        state[p] = ScanState{0.0, 0.0, 0, 1, 0, 0};
        return;
    }
    const long long b = off[p], e = off[p + 1];
    count[p] = b >= 0 && b <= e && e <= total ? e - b : 0;           // offsets outside the rows: a scan of no rows
    for (int e = 0; e < 16; ++e) T[e] = T0[e];
    state[p] = ScanState{0.0, 0.0, 0, 0, 0, 0};
}

// the record of the voxel with `key`, or null when the voxel is not in the index or has no place in the outputs
__device__ __forceinline__ const double *find_voxel(const MapView &m, u64 key)
{
    if (m.cap == 0) return nullptr;
    long long h = (long long)(mix64(key) % (u64)m.cap);
    for (long long probe = 0; probe < m.cap; ++probe) {
        const ulonglong2 e = m.index[h];
        if (e.x == 0) return nullptr;
        if (e.x == key + 1) return e.y == ~0ULL ? nullptr : m.voxels + REC * (long long)e.y;
        h = next_slot(h, m.cap);
    }
    return nullptr;
}

struct RobustOpt {                      // NscMapRobustParams on the device
    int kernel;
    double scale;
};

// The sums of one workgroup's rows at the scan's transform.  NB voxels per row (1: its own; 7: and the six face
// neighbours), ROBUST: every pair weighted by rho'(d^T Omega d).  <T, 1, false> keeps SLAB sums and is nsc_map_register's
// linearisation, operation for operation; everything else keeps WIDE sums.
template <class T, int NB, bool ROBUST>
__device__ __forceinline__ void linearize_rows(const T *pts, int stride, const long long *off, const long long *count,
                                               const MapView &map, const double *transforms, const ScanState *state,
                                               double *slab, RobustOpt opt)
{
    static_assert(NB == 1 || NB == 7, "a voxel, or a voxel and its six face neighbours");
    constexpr int W = NB > 1 || ROBUST ? WIDE : SLAB;
    const int p = blockIdx.y, tid = threadIdx.x;
    if (state[p].done) return;
    const long long n = count[p];
    const T *rows = pts + off[p] * stride;
    double P[12];
    for (int e = 0; e < 12; ++e) P[e] = transforms[16 * (long long)p + e];
    double acc[W];
    for (int e = 0; e < W; ++e) acc[e] = 0.0;
    for (long long i = (long long)blockIdx.x * LOC_THREADS + tid; i < n; i += (long long)LOC_BLOCKS * LOC_THREADS) {
        const T *q = rows + i * stride;
        const double x[3] = {(double)q[0], (double)q[1], (double)q[2]};
        double w[3], u[3];
        place_row(P, x, w);
        if (!(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) && isfinite(w[0]) && isfinite(w[1]) && isfinite(w[2])))
            continue;
        u64 key;
        if (!world_voxel(w, map.g, u, key)) continue;
        bool paired = false;
#pragma unroll 1
        for (int j = 0; j < NB; ++j) {
            u64 kj = key;
            if (j > 0) {
                // neighbour j: axis (j - 1) / 2, odd j one voxel down, even j one up.  Only that axis' 21 bits change,
                // and a coordinate that would leave [0, 2^21) has no voxel: nothing borrows from or carries into another
                // axis
                const int shift = KEY_BITS * ((j - 1) >> 1);
                const long long c = (long long)((key >> shift) & (u64)KEY_MAX) + ((j & 1) ? -1 : 1);
                if (c < 0 || c > KEY_MAX) continue;
                kj = (key & ~((u64)KEY_MAX << shift)) | ((u64)c << shift);
            }
            const double *rec = find_voxel(map, kj);        // the record is read only after the index says it exists
            if (!rec) continue;
            const double2 *r2 = reinterpret_cast<const double2 *>(rec);      // a record is one aligned 128-byte line
            const double2 a0 = r2[0], a1 = r2[1], a4 = r2[4], a5 = r2[5], a6 = r2[6], a7 = r2[7];
            if (a7.y != 1.0) continue;
            const double d[3] = {w[0] - a0.x, w[1] - a0.y, w[2] - a1.x};
            // Omega = [xx xy xz; xy yy yz; xz yz zz] from entries 9..14
            double O[3][3] = {{a4.y, a5.x, a5.y}, {a5.x, a6.x, a6.y}, {a5.y, a6.y, a7.x}};
            double e[3];
            for (int r = 0; r < 3; ++r) e[r] = (O[r][0] * d[0] + O[r][1] * d[1]) + O[r][2] * d[2];      // Omega d
            double rho = (d[0] * e[0] + d[1] * e[1]) + d[2] * e[2];          // s = d^T Omega d
            double d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
            double wt = 1.0;
            if constexpr (ROBUST) {
                // w J^T Omega J and w J^T Omega d are the sums below of w Omega and w Omega d
                const Robust k = robust_rho_w(opt.kernel, opt.scale, rho);
                wt = k.w;
                rho = k.rho;
                d2 *= wt;
                for (int r = 0; r < 3; ++r) {
                    e[r] *= wt;
                    for (int c = 0; c < 3; ++c) O[r][c] *= wt;
                }
            }
            // A = -[w]x has the columns (0, -w2, w1), (w2, 0, -w0), (-w1, w0, 0); OA = Omega A, row by row
            double OA[3][3];
            for (int r = 0; r < 3; ++r) {
                OA[r][0] = O[r][2] * w[1] - O[r][1] * w[2];
                OA[r][1] = O[r][0] * w[2] - O[r][2] * w[0];
                OA[r][2] = O[r][1] * w[0] - O[r][0] * w[1];
            }
            // A^T M for a 3-vector or a column of a matrix M: (w1 m2 - w2 m1, w2 m0 - w0 m2, w0 m1 - w1 m0)
            double AOA[3][3];
            for (int b = 0; b < 3; ++b) {
                AOA[0][b] = w[1] * OA[2][b] - w[2] * OA[1][b];
                AOA[1][b] = w[2] * OA[0][b] - w[0] * OA[2][b];
                AOA[2][b] = w[0] * OA[1][b] - w[1] * OA[0][b];
            }
            // the upper triangle of [[A^T O A, A^T O], [O A, O]], row by row
            int t = 0;
            for (int a = 0; a < 3; ++a) {
                for (int b = a; b < 3; ++b) acc[t++] += AOA[a][b];
                for (int b = 0; b < 3; ++b) acc[t++] += OA[b][a];
            }
            for (int a = 0; a < 3; ++a)
                for (int b = a; b < 3; ++b) acc[t++] += O[a][b];
            acc[21] += w[1] * e[2] - w[2] * e[1];
            acc[22] += w[2] * e[0] - w[0] * e[2];
            acc[23] += w[0] * e[1] - w[1] * e[0];
            acc[24] += e[0];
            acc[25] += e[1];
            acc[26] += e[2];
            acc[SUM_D2] += d2;
            acc[COST] += rho;
            if constexpr (W == WIDE) {
                acc[W_SUM] += wt;
                acc[N_PAIRS] += 1.0;
            }
            paired = true;
        }
        if (paired) acc[N_CORR] += 1.0;                     // rows with at least one pair
    }
    // fixed-shape reduction: wave butterfly, then the 4 waves in order
    __shared__ double part[LOC_THREADS / 64][W];
    const int lane = tid & 63, wave = tid >> 6;
    for (int e = 0; e < W; ++e) {
        double v = acc[e];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) part[wave][e] = v;
    }
    __syncthreads();
    if (tid < W) {
        double v = part[0][tid];
        for (int w = 1; w < LOC_THREADS / 64; ++w) v += part[w][tid];
        slab[((long long)p * LOC_BLOCKS + blockIdx.x) * W + tid] = v;
    }
}

template <class T>
__global__ __launch_bounds__(LOC_THREADS) void loc_linearize_kernel(const T *pts, int stride, const long long *off,
                                                                    const long long *count, MapView map,
                                                                    const double *transforms, const ScanState *state,
                                                                    double *slab)
{
    linearize_rows<T, 1, false>(pts, stride, off, count, map, transforms, state, slab, RobustOpt{0, 0.0});
}

template <class T, int NB, bool ROBUST>
__global__ __launch_bounds__(LOC_THREADS) void loc_linearize_robust_kernel(const T *pts, int stride, const long long *off,
                                                                           const long long *count, MapView map,
                                                                           const double *transforms,
                                                                           const ScanState *state, double *slab,
                                                                           RobustOpt opt)
{
    linearize_rows<T, NB, ROBUST>(pts, stride, off, count, map, transforms, state, slab, opt);
}

// `width` is the slabs' (SLAB or WIDE), `sys_width` system0's.  Over SLAB sums every pair has weight 1 and every
// corresponding row one pair: sum w = n_pairs = n_corr.
__global__ __launch_bounds__(64) void loc_finalize_kernel(const long long *count, const double *slab, int width,
                                                          ScanState *state, double *transforms, double *fit_rmse,
                                                          double *cost, long long *corr_iters, double *information,
                                                          double *system0, int sys_width, double *weight_pairs,
                                                          int max_iteration, double rel_fitness, double rel_rmse)
{
    const int p = blockIdx.x, tid = threadIdx.x;
    ScanState &stt = state[p];
    if (stt.done) return;
    __shared__ double sum[WIDE];
    if (tid < WIDE) {
        const int col = tid < width ? tid : N_CORR;
        double v = 0.0;
        for (int g = 0; g < LOC_BLOCKS; ++g) v += slab[((long long)p * LOC_BLOCKS + g) * width + col];
        sum[tid] = v;
    }
    __syncthreads();
    const int round = stt.round;
    if (system0 && round == 0 && tid < sys_width) system0[(long long)p * sys_width + tid] = sum[tid];
    if (tid != 0) return;
    const double nc = sum[N_CORR], ws = sum[W_SUM];
    const long long n = count[p];
    const double fitness = n > 0 ? nc / (double)n : 0.0;
    const double rmse = ws > 0.0 ? sqrt(sum[SUM_D2] / ws) : 0.0;
    bool done = round == max_iteration;
    if (round > 0 && fabs(stt.prev_fitness - fitness) < rel_fitness && fabs(stt.prev_rmse - rmse) < rel_rmse)
        done = true;
    if (done) {
        stt.done = 1;
        fit_rmse[2 * p] = fitness;
        fit_rmse[2 * p + 1] = rmse;
        cost[p] = sum[COST];
        corr_iters[2 * p] = (long long)nc;
        corr_iters[2 * p + 1] = round;
        if (weight_pairs) {
            weight_pairs[2 * p] = ws;
            weight_pairs[2 * p + 1] = sum[N_PAIRS];
        }
        double *info = information + 36 * (long long)p;
        int t = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) { info[6 * a + b] = info[6 * b + a] = sum[t]; ++t; }
        return;
    }
    stt.prev_fitness = fitness;
    stt.prev_rmse = rmse;
    stt.round = round + 1;
    // (sum w JtOJ) x = -sum w JtOd; dT = I without correspondences or a positive-definite system
    double x[6];
    if (!(nc > 0.0) || !gn_solve6(sum, x)) return;
    gn_apply(x, transforms + 16 * (long long)p);
}

struct ScanRegions {
    double *slab; ScanState *state; long long *count;
    size_t total;
};

ScanRegions scan_regions(void *ws, size_t n_scans, int width)
{
    Carver c = {reinterpret_cast<uintptr_t>(ws), 0};
    ScanRegions r;
    r.slab = c.take<double>(n_scans * LOC_BLOCKS * width);
    r.state = c.take<ScanState>(n_scans);
    r.count = c.take<long long>(n_scans);
    r.total = c.o;
    return r;
}

struct LinearizeArgs {
    hipStream_t s;
    const void *points;
    int stride;
    const int64_t *offsets;
    int n_scans;
    ScanRegions r;
    MapView map;
    const double *transforms;
    RobustOpt opt;
};

template <class T, int NB, bool ROBUST>
void launch_linearize(const LinearizeArgs &a)
{
    const dim3 grid(LOC_BLOCKS, a.n_scans), block(LOC_THREADS);
    const long long *off = reinterpret_cast<const long long *>(a.offsets);
    if constexpr (NB == 1 && !ROBUST)
        hipLaunchKernelGGL(loc_linearize_kernel<T>, grid, block, 0, a.s, static_cast<const T *>(a.points), a.stride, off,
                           a.r.count, a.map, a.transforms, a.r.state, a.r.slab);
    else
        hipLaunchKernelGGL((loc_linearize_robust_kernel<T, NB, ROBUST>), grid, block, 0, a.s,
                           static_cast<const T *>(a.points), a.stride, off, a.r.count, a.map, a.transforms, a.r.state,
                           a.r.slab, a.opt);
}

template <class T>
void launch_linearize(const LinearizeArgs &a, int neighbours, bool robust)
{
    if (neighbours == 1)
        robust ? launch_linearize<T, 1, true>(a) : launch_linearize<T, 1, false>(a);
    else
        robust ? launch_linearize<T, 7, true>(a) : launch_linearize<T, 7, false>(a);
}

bool robust_params_ok(const NscMapRobustParams *rob)
{
    if (!rob) return false;
    if (rob->kernel < NSC_MAP_KERNEL_NONE || rob->kernel > NSC_MAP_KERNEL_GEMAN_MCCLURE) return false;
    if (rob->neighbours != 1 && rob->neighbours != 7) return false;
    return rob->kernel == NSC_MAP_KERNEL_NONE || (isfinite(rob->scale) && rob->scale > 0.0);
}

// nsc_map_register (NONE, one voxel, a SLAB-wide system0, no weight_pairs) and nsc_map_register_robust
int register_scans(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_scans,
                   int64_t total_rows, const double *voxels, const uint64_t *index, int64_t max_voxels,
                   const NscMapParams *params, const NscMapRegisterParams *reg, const NscMapRobustParams &rob,
                   const double *init_transforms, double *transforms, double *fitness_rmse, double *cost,
                   int64_t *corr_iterations, double *information, double *system0, int sys_width, double *weight_pairs,
                   bool need_weight_pairs, void *ws, size_t ws_bytes, void *stream)
{
    if (n_scans < 0 || total_rows < 0 || max_voxels < 0) return NSC_EINVAL;
    if (dtype != NSC_MAP_DTYPE_F32 && dtype != NSC_MAP_DTYPE_F64) return NSC_EINVAL;
    if (stride_floats != 3 && !(stride_floats == 4 && dtype == NSC_MAP_DTYPE_F32)) return NSC_EINVAL;
    if (n_scans > NSC_MAP_REGISTER_MAX_SCANS) return NSC_EUNSUPPORTED;        // the scan is gridDim.y
    if (!params || !reg) return NSC_EINVAL;
    if (!(params->voxel_size > 0.0) || !isfinite(params->voxel_size) || !isfinite(params->origin[0]) ||
        !isfinite(params->origin[1]) || !isfinite(params->origin[2]))
        return NSC_EINVAL;
    if (reg->max_iteration < 0 || !(reg->relative_fitness >= 0.0) || !(reg->relative_rmse >= 0.0)) return NSC_EINVAL;
    if (total_rows > NSC_MAP_MAX_ROWS || max_voxels > NSC_MAP_MAX_VOXELS) return NSC_EUNSUPPORTED;
    if (n_scans == 0) return NSC_OK;
    if (!offsets || !init_transforms || !transforms || !fitness_rmse || !cost || !corr_iterations || !information)
        return NSC_EINVAL;
    if (need_weight_pairs && !weight_pairs) return NSC_EINVAL;
    if ((total_rows > 0 && !points) || (max_voxels > 0 && (!voxels || !index))) return NSC_EINVAL;
    const bool robust = rob.kernel != NSC_MAP_KERNEL_NONE;
    const int width = robust || rob.neighbours != 1 ? WIDE : SLAB;
    const ScanRegions r = scan_regions(ws, n_scans, width);
    if (!ws || ws_bytes < r.total) return NSC_EWORKSPACE;
    const MapView map{voxels, reinterpret_cast<const ulonglong2 *>(index), 2 * (long long)max_voxels,
                      MapGrid{params->voxel_size, {params->origin[0], params->origin[1], params->origin[2]}}};
    hipStream_t s = static_cast<hipStream_t>(stream);
    long long *ci = reinterpret_cast<long long *>(corr_iterations);
    hipLaunchKernelGGL(loc_setup_kernel, dim3((n_scans + LOC_THREADS - 1) / LOC_THREADS), dim3(LOC_THREADS), 0, s,
                       reinterpret_cast<const long long *>(offsets), n_scans, (long long)total_rows, init_transforms, transforms, r.state, r.count,
                       fitness_rmse, cost, ci, information, system0, sys_width, weight_pairs);
    const LinearizeArgs a{s, points, stride_floats, offsets, n_scans, r, map, transforms, RobustOpt{rob.kernel, rob.scale}};
    for (int round = 0; round <= reg->max_iteration; ++round) {
        if (dtype == NSC_MAP_DTYPE_F32)
            launch_linearize<float>(a, rob.neighbours, robust);
        else
            launch_linearize<double>(a, rob.neighbours, robust);
        hipLaunchKernelGGL(loc_finalize_kernel, dim3(n_scans), dim3(64), 0, s, r.count, r.slab, width, r.state, transforms,
                           fitness_rmse, cost, ci, information, system0, sys_width, weight_pairs, reg->max_iteration,
                           reg->relative_fitness, reg->relative_rmse);
    }
    return launch_status();
}

}  // namespace

extern "C" {

void nsc_map_register_default_params(NscMapRegisterParams *p)
{
    if (!p) return;
    p->max_iteration = 30;
    p->reserved = 0;
    p->relative_fitness = 1e-6;
    p->relative_rmse = 1e-6;
}

void nsc_map_robust_default_params(NscMapRobustParams *p)
{
    if (!p) return;
    p->kernel = NSC_MAP_KERNEL_NONE;
    p->neighbours = 1;
    p->scale = 0.0;
}

size_t nsc_map_register_workspace_bytes(int32_t n_scans)
{
    if (n_scans < 0) return 0;
    return scan_regions(nullptr, n_scans, SLAB).total;
}

size_t nsc_map_register_robust_workspace_bytes(int32_t n_scans)
{
    if (n_scans < 0) return 0;
    return scan_regions(nullptr, n_scans, WIDE).total;
}

int nsc_map_register(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_scans,
                     int64_t total_rows, const double *voxels, const uint64_t *index, int64_t max_voxels,
                     const NscMapParams *params, const NscMapRegisterParams *reg, const double *init_transforms,
                     double *transforms, double *fitness_rmse, double *cost, int64_t *corr_iterations,
                     double *information, double *system0, void *ws, size_t ws_bytes, void *stream)
{
    const NscMapRobustParams quadratic{NSC_MAP_KERNEL_NONE, 1, 0.0};
    return register_scans(points, dtype, stride_floats, offsets, n_scans, total_rows, voxels, index, max_voxels, params, reg,
                          quadratic, init_transforms, transforms, fitness_rmse, cost, corr_iterations, information, system0,
                          SLAB, nullptr, false, ws, ws_bytes, stream);
}

int nsc_map_register_robust(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets,
                            int32_t n_scans, int64_t total_rows, const double *voxels, const uint64_t *index,
                            int64_t max_voxels, const NscMapParams *params, const NscMapRegisterParams *reg,
                            const NscMapRobustParams *robust, const double *init_transforms, double *transforms,
                            double *fitness_rmse, double *cost, int64_t *corr_iterations, double *information,
                            double *system0, double *weight_pairs, void *ws, size_t ws_bytes, void *stream)
{
    if (!robust_params_ok(robust)) return NSC_EINVAL;
    return register_scans(points, dtype, stride_floats, offsets, n_scans, total_rows, voxels, index, max_voxels, params, reg,
                          *robust, init_transforms, transforms, fitness_rmse, cost, corr_iterations, information, system0,
                          WIDE, weight_pairs, true, ws, ws_bytes, stream);
}

}  // extern "C"
