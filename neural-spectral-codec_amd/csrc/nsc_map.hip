// nsc_map.hip -- the global voxel map: every keyframe cloud placed by its optimised pose and merged into one cloud,
// one centroid per occupied voxel (nsc_map_build; the definition is in include/nsc.h, tests/map_restatement.py restates
// it in float64 numpy).  The global form of the per-cloud down-sampling of nsc_geometry.hip: many clouds, one
// open-addressing table claimed with 64-bit CAS, a pose per cloud, and a compaction in first-row order that spans
// workgroups.
//
// Launch sequence (all on the caller's stream, nothing allocated, copied or synchronised; the grids depend on
// total_rows and max_voxels alone):
//   clear    the table's slots, the first-row bitmap (one bit per input row) and the stats
//   insert   one pass over the rows, NSC_MAP_INSERT_ROWS consecutive rows per workgroup at a time: cloud of the row
//            (binary search over the offsets, kept while the rows stay in the cloud), w = R p + t, key, claim (64-bit
//            CAS, a probe bounded by the slot count), then integer atomics on the slot: min first row, count, the three
//            int64 fixed-point sums, min and max cloud.  Counters of dropped rows: per thread, summed per workgroup
//   mark     per occupied slot: set bit `first` of the bitmap
//   count    one wave per tile of NSC_MAP_TILE_ROWS rows (64 bitmap words): the marks in front of each word within
//            its tile, and the tile's total
//   scan     one workgroup: exclusive scan of the tile totals in place; found and written into the stats
//   write    per occupied slot: its place = tile start + word prefix + marks below its bit; centroid, info and key
//            there if the place is below max_voxels
// The compaction walks the table and a bitmap, not the rows again: no second read of the points and no second probe.
//
// nsc_map_build_dist is the same six launches over slots of 128 bytes (DistSlot): the insert body, the mark pass and the
// write pass are templates over the slot, and a slot's sums are of the row's position inside its voxel and its six
// second moments.  Its write pass turns them into the record nsc_localize.hip reads (mean, covariance, information,
// usable flag) and writes the index (key + 1, place) at the table's own slot positions, for every slot.
//
// No float atomics anywhere: results are bitwise reproducible and do not depend on arrival order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nsc.h"
#include "nsc_eig3.h"
#include "nsc_util.h"
#include "nsc_voxel_hash.h"

namespace {

constexpr int MAP_THREADS = 256;
constexpr int MAP_SLOT_BLOCKS = 4096;                     // workgroups at most of the launches that walk slots or words
constexpr long long TILE_ROWS = NSC_MAP_TILE_ROWS;
constexpr int TILE_WORDS = NSC_MAP_TILE_ROWS / 64;
constexpr int SCAN_THREADS = NSC_MAP_SCAN_THREADS;
constexpr long long INSERT_ROWS = NSC_MAP_INSERT_ROWS;
static_assert(TILE_WORDS == 64, "one lane of a wave per bitmap word of a tile");
static_assert(INSERT_ROWS % MAP_THREADS == 0, "a workgroup takes its rows in whole sweeps");

typedef unsigned long long u64;

struct MapSlot {                        // one voxel of the table: 64 bytes, one cache line
    u64 key;                            // packed key + 1; 0 = empty
    u64 first;                          // smallest packed row in the voxel; ~0 until a row arrives
    u64 count;
    long long sum[3];                   // of rint(w 2^24)
    u64 cloud_min;                      // ~0 until a row arrives
    u64 cloud_max;                      // cloud + 1
};
static_assert(sizeof(MapSlot) == 64, "a slot is cleared as 8 words");

// A voxel of the distribution map (nsc_map_build_dist): MapSlot's words in MapSlot's places, the sums being of q, the
// position inside the voxel (include/nsc.h), and its six second moments: 128 bytes
struct DistSlot {
    u64 key, first, count;
    long long sum[3];                   // of q_a
    u64 cloud_min, cloud_max;
    long long sq[6];                    // of q_a q_b: xx xy xz yy yz zz
    u64 pad[2];
};
static_assert(sizeof(DistSlot) == 2 * sizeof(MapSlot), "a distribution slot is cleared as two slots' words");
template <class S> constexpr int slot_words() { return (int)(sizeof(S) / 8); }

__device__ __forceinline__ u64 peek(const u64 *p)        // a value other workgroups change: not from a stale line
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// per_slot: the words of a slot, a power of two; words 1 (first) and 6 (cloud_min) of a slot start at ~0
__global__ __launch_bounds__(MAP_THREADS) void map_clear_kernel(u64 *slots, long long slot_words, int per_slot, u64 *bits,
                                                                long long n_words, long long *stats)
{
    const long long i0 = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
    const long long stride = (long long)gridDim.x * MAP_THREADS;
    for (long long i = i0; i < slot_words; i += stride) {
        const int f = (int)(i & (per_slot - 1));
        slots[i] = (f == 1 || f == 6) ? ~0ULL : 0ULL;
    }
    for (long long i = i0; i < n_words; i += stride) bits[i] = 0ULL;
    if (i0 < NSC_MAP_STATS) stats[i0] = 0;
}

// the cloud of packed row `row`: the largest c in [0, n_clouds) with off[c] <= row, if row < off[c+1]; else -1
__device__ __forceinline__ int cloud_of(const long long *off, int n_clouds, long long row, long long &lo, long long &hi)
{
    int a = 0, b = n_clouds;
    while (a < b) {
        const int m = a + (b - a) / 2;
        if (off[m] <= row) a = m + 1; else b = m;
    }
    if (a == 0) return -1;
    lo = off[a - 1]; hi = off[a];
    return row < hi ? a - 1 : -1;
}

enum { C_USED, C_NOT_FINITE, C_OUTSIDE, C_NO_POSE, C_UNPLACED, N_COUNTERS };

// what a row adds to its voxel beside the count, the first row and the clouds
__device__ __forceinline__ void add_row(MapSlot &s, const double w[3], const double u[3])
{
    for (int a = 0; a < 3; ++a)
        atomicAdd(reinterpret_cast<u64 *>(&s.sum[a]), (u64)__double2ll_rn(w[a] * FIX_SCALE));
}

__device__ __forceinline__ void add_row(DistSlot &s, const double w[3], const double u[3])
{
    long long q[3];
    for (int a = 0; a < 3; ++a) q[a] = __double2ll_rn(u[a] * MOMENT_SCALE) - (long long)MOMENT_HALF;
    for (int a = 0; a < 3; ++a) atomicAdd(reinterpret_cast<u64 *>(&s.sum[a]), (u64)q[a]);
    int t = 0;
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) atomicAdd(reinterpret_cast<u64 *>(&s.sq[t++]), (u64)(q[a] * q[b]));
}

template <class T, class S>
__global__ __launch_bounds__(MAP_THREADS) void map_insert_kernel(const T *pts, int stride, const long long *off,
                                                                 int n_clouds, long long total, const double *poses,
                                                                 int n_poses, const long long *ids, MapGrid g,
                                                                 S *tab, long long cap, long long *stats)
{
    const int tid = threadIdx.x;
    long long cnt[N_COUNTERS] = {0, 0, 0, 0, 0};
    const long long n_sweeps = (total + INSERT_ROWS - 1) / INSERT_ROWS;
    for (long long sweep = blockIdx.x; sweep < n_sweeps; sweep += gridDim.x) {
        long long lo = 0, hi = 0;       // the rows of cloud c, while c >= 0
        int c = -1;
        for (int k = 0; k < INSERT_ROWS / MAP_THREADS; ++k) {
            const long long row = sweep * INSERT_ROWS + (long long)k * MAP_THREADS + tid;
            if (row >= total) break;
            if (c < 0 || row < lo || row >= hi) c = cloud_of(off, n_clouds, row, lo, hi);
            const long long id = c < 0 ? -1 : (ids ? ids[c] : (long long)c);
            if (id < 0 || id >= n_poses) { ++cnt[C_NO_POSE]; continue; }
            const T *q = pts + row * stride;
            const double p[3] = {(double)q[0], (double)q[1], (double)q[2]};
            double w[3];
            place_row(poses + 16 * id, p, w);
            if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(w[0]) && isfinite(w[1]) && isfinite(w[2]))) {
                ++cnt[C_NOT_FINITE];
                continue;
            }
            double u[3];
            u64 key;
            if (!world_voxel(w, g, u, key)) {
                ++cnt[C_OUTSIDE];
                continue;
            }
            long long h = cap > 0 ? (long long)(mix64(key) % (u64)cap) : 0;
            bool placed = false;
            for (long long probe = 0; probe < cap; ++probe) {          // every slot once at most
                u64 e = peek(&tab[h].key);
                if (e == 0) {
                    e = atomicCAS(&tab[h].key, 0ULL, key + 1);
                    if (e == 0) e = key + 1;
                }
                if (e == key + 1) { placed = true; break; }
                h = next_slot(h, cap);
            }
            if (!placed) { ++cnt[C_UNPLACED]; continue; }
            ++cnt[C_USED];
            S &s = tab[h];
            // min and max only move one way: a value read before the atomic that already beats ours stays beaten
            if (peek(&s.first) > (u64)row) atomicMin(&s.first, (u64)row);
            if (peek(&s.cloud_min) > (u64)c) atomicMin(&s.cloud_min, (u64)c);
            if (peek(&s.cloud_max) < (u64)c + 1) atomicMax(&s.cloud_max, (u64)c + 1);
            atomicAdd(&s.count, 1ULL);
            add_row(s, w, u);
        }
    }
    __shared__ long long red[N_COUNTERS][MAP_THREADS / 64];
    for (int k = 0; k < N_COUNTERS; ++k) {
        const long long v = nsc_wave_sum(cnt[k]);
        if ((tid & 63) == 0) red[k][tid >> 6] = v;
    }
    __syncthreads();
    if (tid < N_COUNTERS) {
        long long v = 0;
        for (int w = 0; w < MAP_THREADS / 64; ++w) v += red[tid][w];
        if (v) atomicAdd(reinterpret_cast<u64 *>(&stats[NSC_MAP_STAT_USED + tid]), (u64)v);
    }
}
static_assert(NSC_MAP_STAT_NOT_FINITE == NSC_MAP_STAT_USED + C_NOT_FINITE && NSC_MAP_STAT_OUTSIDE == NSC_MAP_STAT_USED + C_OUTSIDE &&
                  NSC_MAP_STAT_NO_POSE == NSC_MAP_STAT_USED + C_NO_POSE && NSC_MAP_STAT_UNPLACED == NSC_MAP_STAT_USED + C_UNPLACED,
              "the insert pass's counters are the stats from NSC_MAP_STAT_USED on, in order");

template <class S>
__global__ __launch_bounds__(MAP_THREADS) void map_mark_kernel(const S *tab, long long cap, u64 *bits,
                                                               long long n_words)
{
    for (long long h = (long long)blockIdx.x * MAP_THREADS + threadIdx.x; h < cap; h += (long long)gridDim.x * MAP_THREADS) {
        if (tab[h].key == 0) continue;
        const u64 first = tab[h].first;  // a claimed slot has had a row, so first < total_rows; checked all the same
        if ((first >> 6) >= (u64)n_words) continue;
        atomicOr(&bits[first >> 6], 1ULL << (first & 63));
    }
}

// tile t = words [64 t, 64 t + 64) of the bitmap: prefix[w] = marks of the tile's words before w, tile[t] = its marks
__global__ __launch_bounds__(MAP_THREADS) void map_count_kernel(const u64 *bits, long long n_words, long long n_tiles,
                                                                unsigned *prefix, long long *tile)
{
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (MAP_THREADS / 64);
    for (long long t = (long long)blockIdx.x * (MAP_THREADS / 64) + (threadIdx.x >> 6); t < n_tiles; t += waves) {
        const long long w = t * TILE_WORDS + lane;
        const int v = w < n_words ? __popcll(bits[w]) : 0;
        int inc = v;
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (w < n_words) prefix[w] = (unsigned)(inc - v);
        if (lane == 63) tile[t] = inc;
    }
}

// exclusive scan of tile[0 .. n_tiles) in place; a thread takes ceil(n_tiles / SCAN_THREADS) consecutive tiles
__global__ __launch_bounds__(SCAN_THREADS) void map_scan_kernel(long long *tile, long long n_tiles, long long max_voxels,
                                                                long long *stats)
{
    __shared__ long long part[SCAN_THREADS];
    const int tid = threadIdx.x;
    const long long chunk = (n_tiles + SCAN_THREADS - 1) / SCAN_THREADS;
    const long long b = min(tid * chunk, n_tiles), e = min(b + chunk, n_tiles);
    long long s = 0;
    for (long long i = b; i < e; ++i) s += tile[i];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < SCAN_THREADS; o <<= 1) {
        const long long v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    long long run = part[tid] - s;
    for (long long i = b; i < e; ++i) { const long long v = tile[i]; tile[i] = run; run += v; }
    if (tid == SCAN_THREADS - 1) {
        const long long found = part[tid];
        stats[NSC_MAP_STAT_FOUND] = found;
        stats[NSC_MAP_STAT_WRITTEN] = min(found, max_voxels);
    }
}

// what the compaction left for the write pass
struct MapPlaces {
    const u64 *bits; const unsigned *prefix; const long long *tile;
    long long n_words;
    // the place of the voxel whose first row is `first`: the marks in front of its bit
    __device__ long long of(u64 first) const
    {
        const long long w = (long long)(first >> 6);
        return tile[first / (u64)TILE_ROWS] + prefix[w] + __popcll(bits[w] & ((1ULL << (first & 63)) - 1ULL));
    }
};

template <class S>
__device__ __forceinline__ void write_info(const S &s, long long pos, long long *info, long long *keys)
{
    info[4 * pos] = (long long)s.count;
    info[4 * pos + 1] = (long long)s.first;
    info[4 * pos + 2] = (long long)s.cloud_min;
    info[4 * pos + 3] = (long long)s.cloud_max - 1;
    keys[pos] = (long long)(s.key - 1);
}

struct CentroidOut {                     // nsc_map_build: one centroid per voxel
    double *points;
    __device__ void empty(long long h) const {}
    __device__ void overflow(long long h, const MapSlot &s) const {}
    __device__ void voxel(long long h, const MapSlot &s, long long pos) const
    {
        const double n = (double)s.count;
        for (int a = 0; a < 3; ++a) points[3 * pos + a] = ((double)s.sum[a] / FIX_SCALE) / n;
    }
};

struct DistOut {                         // nsc_map_build_dist: a distribution record per voxel, and the kept index
    double *voxels; u64 *index; long long *moments;
    MapGrid g;
    double eigen_ratio, floor2;
    long long min_points;
    __device__ void empty(long long h) const { index[2 * h] = 0ULL; index[2 * h + 1] = ~0ULL; }
    // a voxel past the outputs keeps its key, so that probes continue past it
    __device__ void overflow(long long h, const DistSlot &s) const { index[2 * h] = s.key; index[2 * h + 1] = ~0ULL; }
    __device__ void voxel(long long h, const DistSlot &s, long long pos) const
    {
        index[2 * h] = s.key;
        index[2 * h + 1] = (u64)pos;
        if (moments) {
            for (int a = 0; a < 3; ++a) moments[9 * pos + a] = s.sum[a];
            for (int t = 0; t < 6; ++t) moments[9 * pos + 3 + t] = s.sq[t];
        }
        const double n = (double)s.count;
        const u64 key = s.key - 1;
        double rec[16], m[3];
        for (int a = 0; a < 3; ++a) {
            const double k = (double)(long long)((key >> (a * KEY_BITS)) & (u64)KEY_MAX) - KEY_OFFSET;
            m[a] = (double)s.sum[a] / n;                       // mean of q
            rec[a] = g.origin[a] + ((k + 0.5) + m[a] / MOMENT_SCALE) * g.voxel;
        }
        const double unit = g.voxel / MOMENT_SCALE, unit2 = unit * unit;
        int t = 0;
        for (int a = 0; a < 3; ++a)
            for (int b = a; b < 3; ++b, ++t) rec[3 + t] = ((double)s.sq[t] / n - m[a] * m[b]) * unit2;
        double A[3][3], V[3][3], inv[3];
        jacobi_eig3(rec + 3, A, V);
        const double top = fmax(A[0][0], fmax(A[1][1], A[2][2]));
        for (int i = 0; i < 3; ++i) inv[i] = 1.0 / fmax(fmax(A[i][i], eigen_ratio * top), floor2);
        t = 0;
        for (int a = 0; a < 3; ++a)
            for (int b = a; b < 3; ++b, ++t)
                rec[9 + t] = (V[a][0] * V[b][0] * inv[0] + V[a][1] * V[b][1] * inv[1]) + V[a][2] * V[b][2] * inv[2];
        bool usable = (long long)s.count >= min_points;
        for (int e = 0; e < 15; ++e) usable = usable && isfinite(rec[e]);
        rec[15] = usable ? 1.0 : 0.0;
        for (int e = 0; e < 16; ++e) voxels[16 * pos + e] = rec[e];
    }
};

template <class S, class Out>
__global__ __launch_bounds__(MAP_THREADS) void map_write_kernel(const S *tab, long long cap, MapPlaces places,
                                                                long long max_voxels, long long *info, long long *keys,
                                                                Out out)
{
    for (long long h = (long long)blockIdx.x * MAP_THREADS + threadIdx.x; h < cap; h += (long long)gridDim.x * MAP_THREADS) {
        const S s = tab[h];
        if (s.key == 0) { out.empty(h); continue; }
        // a claimed slot has had a row, so first < total_rows; checked all the same
        const long long pos = (s.first >> 6) < (u64)places.n_words ? places.of(s.first) : max_voxels;
        if (pos >= max_voxels) { out.overflow(h, s); continue; }
        out.voxel(h, s, pos);
        write_info(s, pos, info, keys);
    }
}

template <class S>
struct MapRegions {
    S *slots; u64 *bits; unsigned *prefix; long long *tile;
    long long cap, n_words, n_tiles;
    size_t total;
};

template <class S>
MapRegions<S> map_regions(void *ws, long long total_rows, long long max_voxels)
{
    Carver c = {reinterpret_cast<uintptr_t>(ws), 0};
    MapRegions<S> r;
    r.cap = 2 * max_voxels;
    r.n_words = (total_rows + 63) / 64;
    r.n_tiles = (total_rows + TILE_ROWS - 1) / TILE_ROWS;
    r.slots = c.take<S>(r.cap);
    r.bits = c.take<u64>(r.n_words);
    r.prefix = c.take<unsigned>(r.n_words);
    r.tile = c.take<long long>(r.n_tiles);
    r.total = c.o;
    return r;
}

inline unsigned blocks_for(long long n, long long per_block, long long most)
{
    const long long b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > most ? most : b));
}

// The arguments both builds take: NSC_OK, or what the call returns before anything is launched
int check_build(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_clouds,
                int64_t total_rows, const double *poses, int32_t n_poses, const NscMapParams *params, int64_t max_voxels,
                bool outputs, const int64_t *stats)
{
    if (n_clouds < 0 || n_poses < 0 || total_rows < 0 || max_voxels < 0 || !params || !stats || !offsets) return NSC_EINVAL;
    if (dtype != NSC_MAP_DTYPE_F32 && dtype != NSC_MAP_DTYPE_F64) return NSC_EINVAL;
    if (stride_floats != 3 && !(stride_floats == 4 && dtype == NSC_MAP_DTYPE_F32)) return NSC_EINVAL;
    if (!(params->voxel_size > 0.0) || !isfinite(params->voxel_size) || !isfinite(params->origin[0]) ||
        !isfinite(params->origin[1]) || !isfinite(params->origin[2]))
        return NSC_EINVAL;
    if ((total_rows > 0 && !points) || (n_poses > 0 && !poses) || (max_voxels > 0 && !outputs)) return NSC_EINVAL;
    if (total_rows > NSC_MAP_MAX_ROWS || max_voxels > NSC_MAP_MAX_VOXELS) return NSC_EUNSUPPORTED;
    return NSC_OK;
}

template <class S>
size_t workspace_bytes(int64_t total_rows, int64_t max_voxels)
{
    if (total_rows < 0 || max_voxels < 0 || total_rows > NSC_MAP_MAX_ROWS || max_voxels > NSC_MAP_MAX_VOXELS) return 0;
    return map_regions<S>(nullptr, total_rows, max_voxels).total;
}

// The six launches of a build over slots of type S; `out` is what the write pass writes per voxel beside info and keys
template <class S, class Out>
int launch_build(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_clouds,
                 int64_t total_rows, const double *poses, int32_t n_poses, const int64_t *pose_ids,
                 const NscMapParams *params, int64_t max_voxels, int64_t *info, int64_t *keys, int64_t *stats, const Out &out,
                 const MapRegions<S> &r, void *stream)
{
    const MapGrid g{params->voxel_size, {params->origin[0], params->origin[1], params->origin[2]}};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 threads(MAP_THREADS), per_rows(blocks_for(total_rows, INSERT_ROWS, NSC_MAP_INSERT_BLOCKS));
    const long long *off = reinterpret_cast<const long long *>(offsets), *ids = reinterpret_cast<const long long *>(pose_ids);
    long long *st = reinterpret_cast<long long *>(stats);
    const long long n_slot_words = r.cap * slot_words<S>();
    hipLaunchKernelGGL(map_clear_kernel, dim3(blocks_for(n_slot_words > r.n_words ? n_slot_words : r.n_words, MAP_THREADS, MAP_SLOT_BLOCKS)),
                       threads, 0, s, reinterpret_cast<u64 *>(r.slots), n_slot_words, slot_words<S>(), r.bits, r.n_words, st);
    if (dtype == NSC_MAP_DTYPE_F32)
        hipLaunchKernelGGL((map_insert_kernel<float, S>), per_rows, threads, 0, s, static_cast<const float *>(points),
                           stride_floats, off, n_clouds, (long long)total_rows, poses, n_poses, ids, g, r.slots, r.cap, st);
    else
        hipLaunchKernelGGL((map_insert_kernel<double, S>), per_rows, threads, 0, s, static_cast<const double *>(points),
                           stride_floats, off, n_clouds, (long long)total_rows, poses, n_poses, ids, g, r.slots, r.cap, st);
    const dim3 per_slot(blocks_for(r.cap, MAP_THREADS, MAP_SLOT_BLOCKS));
    hipLaunchKernelGGL(map_mark_kernel<S>, per_slot, threads, 0, s, r.slots, r.cap, r.bits, r.n_words);
    hipLaunchKernelGGL(map_count_kernel, dim3(blocks_for(r.n_tiles, MAP_THREADS / 64, MAP_SLOT_BLOCKS)), threads, 0, s,
                       r.bits, r.n_words, r.n_tiles, r.prefix, r.tile);
    hipLaunchKernelGGL(map_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, r.tile, r.n_tiles, (long long)max_voxels, st);
    hipLaunchKernelGGL((map_write_kernel<S, Out>), per_slot, threads, 0, s, r.slots, r.cap,
                       MapPlaces{r.bits, r.prefix, r.tile, r.n_words}, (long long)max_voxels,
                       reinterpret_cast<long long *>(info), reinterpret_cast<long long *>(keys), out);
    return launch_status();
}

}  // namespace

extern "C" {

void nsc_map_default_params(NscMapParams *p)
{
    if (!p) return;
    p->voxel_size = 0.5;
    p->origin[0] = p->origin[1] = p->origin[2] = 0.0;
}

void nsc_map_dist_default_params(NscMapDistParams *p)
{
    if (!p) return;
    p->min_points = 6;
    p->reserved = 0;
    p->eigen_ratio = 1e-2;
    p->sigma_floor = 1e-3;
}

size_t nsc_map_workspace_bytes(int64_t total_rows, int64_t max_voxels)
{
    return workspace_bytes<MapSlot>(total_rows, max_voxels);
}

size_t nsc_map_dist_workspace_bytes(int64_t total_rows, int64_t max_voxels)
{
    return workspace_bytes<DistSlot>(total_rows, max_voxels);
}

int nsc_map_build(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_clouds,
                  int64_t total_rows, const double *poses, int32_t n_poses, const int64_t *pose_ids,
                  const NscMapParams *params, int64_t max_voxels, double *out_points, int64_t *info, int64_t *keys,
                  int64_t *stats, void *ws, size_t ws_bytes, void *stream)
{
    if (const int st = check_build(points, dtype, stride_floats, offsets, n_clouds, total_rows, poses, n_poses, params,
                                   max_voxels, out_points && info && keys, stats))
        return st;
    const MapRegions<MapSlot> r = map_regions<MapSlot>(ws, total_rows, max_voxels);
    if (r.total > 0 && (!ws || ws_bytes < r.total)) return NSC_EWORKSPACE;
    return launch_build(points, dtype, stride_floats, offsets, n_clouds, total_rows, poses, n_poses, pose_ids, params,
                        max_voxels, info, keys, stats, CentroidOut{out_points}, r, stream);
}

int nsc_map_build_dist(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_clouds,
                       int64_t total_rows, const double *poses, int32_t n_poses, const int64_t *pose_ids,
                       const NscMapParams *params, const NscMapDistParams *dist, int64_t max_voxels, double *voxels,
                       uint64_t *index, int64_t *info, int64_t *keys, int64_t *moments, int64_t *stats, void *ws,
                       size_t ws_bytes, void *stream)
{
    if (const int st = check_build(points, dtype, stride_floats, offsets, n_clouds, total_rows, poses, n_poses, params,
                                   max_voxels, voxels && index && info && keys, stats))
        return st;
    if (!dist || dist->min_points < 1 || !(dist->eigen_ratio > 0.0) || !(dist->eigen_ratio <= 1.0) ||
        !(dist->sigma_floor > 0.0) || !isfinite(dist->sigma_floor))
        return NSC_EINVAL;
    const MapRegions<DistSlot> r = map_regions<DistSlot>(ws, total_rows, max_voxels);
    if (r.total > 0 && (!ws || ws_bytes < r.total)) return NSC_EWORKSPACE;
    const DistOut out{voxels, reinterpret_cast<u64 *>(index), reinterpret_cast<long long *>(moments),
                      MapGrid{params->voxel_size, {params->origin[0], params->origin[1], params->origin[2]}},
                      dist->eigen_ratio, dist->sigma_floor * dist->sigma_floor, (long long)dist->min_points};
    return launch_build(points, dtype, stride_floats, offsets, n_clouds, total_rows, poses, n_poses, pose_ids, params,
                        max_voxels, info, keys, stats, out, r, stream);
}

}  // extern "C"
