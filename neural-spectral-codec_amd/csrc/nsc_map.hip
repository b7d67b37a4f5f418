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
// No float atomics anywhere: results are bitwise reproducible and do not depend on arrival order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nsc.h"
#include "nsc_util.h"
#include "nsc_voxel_hash.h"

namespace {

constexpr int MAP_THREADS = 256;
constexpr int MAP_SLOT_BLOCKS = 4096;                     // workgroups at most of the launches that walk slots or words
constexpr long long TILE_ROWS = NSC_MAP_TILE_ROWS;
constexpr int TILE_WORDS = NSC_MAP_TILE_ROWS / 64;
constexpr int SCAN_THREADS = NSC_MAP_SCAN_THREADS;
constexpr long long INSERT_ROWS = NSC_MAP_INSERT_ROWS;
constexpr double KEY_OFFSET = 1048576.0;                  // 2^20: voxel coordinates count from -2^20
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
constexpr int SLOT_WORDS = 8;
static_assert(sizeof(MapSlot) == 8 * SLOT_WORDS, "a slot is cleared as 8 words");

struct MapGrid {
    double voxel, origin[3];
};

__device__ __forceinline__ u64 peek(const u64 *p)        // a value other workgroups change: not from a stale line
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(MAP_THREADS) void map_clear_kernel(u64 *slots, long long slot_words, u64 *bits,
                                                                long long n_words, long long *stats)
{
    const long long i0 = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
    const long long stride = (long long)gridDim.x * MAP_THREADS;
    for (long long i = i0; i < slot_words; i += stride) {
        const int f = (int)(i & (SLOT_WORDS - 1));
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

template <class T>
__global__ __launch_bounds__(MAP_THREADS) void map_insert_kernel(const T *pts, int stride, const long long *off,
                                                                 int n_clouds, long long total, const double *poses,
                                                                 int n_poses, const long long *ids, MapGrid g,
                                                                 MapSlot *tab, long long cap, long long *stats)
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
            const double *P = poses + 16 * id;
            double w[3];
            for (int a = 0; a < 3; ++a) w[a] = ((P[4 * a] * p[0] + P[4 * a + 1] * p[1]) + P[4 * a + 2] * p[2]) + P[4 * a + 3];
            if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(w[0]) && isfinite(w[1]) && isfinite(w[2]))) {
                ++cnt[C_NOT_FINITE];
                continue;
            }
            double kd[3];
            for (int a = 0; a < 3; ++a) kd[a] = floor((w[a] - g.origin[a]) / g.voxel) + KEY_OFFSET;
            if (!(kd[0] >= 0.0 && kd[0] <= (double)KEY_MAX && kd[1] >= 0.0 && kd[1] <= (double)KEY_MAX && kd[2] >= 0.0 &&
                  kd[2] <= (double)KEY_MAX)) {
                ++cnt[C_OUTSIDE];
                continue;
            }
            const u64 key = pack_key((long long)kd[0], (long long)kd[1], (long long)kd[2]);
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
            MapSlot &s = tab[h];
            // min and max only move one way: a value read before the atomic that already beats ours stays beaten
            if (peek(&s.first) > (u64)row) atomicMin(&s.first, (u64)row);
            if (peek(&s.cloud_min) > (u64)c) atomicMin(&s.cloud_min, (u64)c);
            if (peek(&s.cloud_max) < (u64)c + 1) atomicMax(&s.cloud_max, (u64)c + 1);
            atomicAdd(&s.count, 1ULL);
            for (int a = 0; a < 3; ++a)
                atomicAdd(reinterpret_cast<u64 *>(&s.sum[a]), (u64)__double2ll_rn(w[a] * FIX_SCALE));
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

__global__ __launch_bounds__(MAP_THREADS) void map_mark_kernel(const MapSlot *tab, long long cap, u64 *bits,
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

__global__ __launch_bounds__(MAP_THREADS) void map_write_kernel(const MapSlot *tab, long long cap, const u64 *bits,
                                                                const unsigned *prefix, const long long *tile,
                                                                long long n_words, long long max_voxels, double *points, long long *info,
                                                                long long *keys)
{
    for (long long h = (long long)blockIdx.x * MAP_THREADS + threadIdx.x; h < cap; h += (long long)gridDim.x * MAP_THREADS) {
        const MapSlot s = tab[h];
        if (s.key == 0 || (s.first >> 6) >= (u64)n_words) continue;
        const long long w = (long long)(s.first >> 6);
        const long long pos = tile[s.first / (u64)TILE_ROWS] + prefix[w] + __popcll(bits[w] & ((1ULL << (s.first & 63)) - 1ULL));
        if (pos >= max_voxels) continue;
        const double n = (double)s.count;
        for (int a = 0; a < 3; ++a) points[3 * pos + a] = ((double)s.sum[a] / FIX_SCALE) / n;
        info[4 * pos] = (long long)s.count;
        info[4 * pos + 1] = (long long)s.first;
        info[4 * pos + 2] = (long long)s.cloud_min;
        info[4 * pos + 3] = (long long)s.cloud_max - 1;
        keys[pos] = (long long)(s.key - 1);
    }
}

struct MapRegions {
    MapSlot *slots; u64 *bits; unsigned *prefix; long long *tile;
    long long cap, n_words, n_tiles;
    size_t total;
};

MapRegions map_regions(void *ws, long long total_rows, long long max_voxels)
{
    Carver c = {reinterpret_cast<uintptr_t>(ws), 0};
    MapRegions r;
    r.cap = 2 * max_voxels;
    r.n_words = (total_rows + 63) / 64;
    r.n_tiles = (total_rows + TILE_ROWS - 1) / TILE_ROWS;
    r.slots = c.take<MapSlot>(r.cap);
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

template <class T>
void launch_insert(hipStream_t s, const void *points, int stride, const int64_t *offsets, int n_clouds, long long total,
                   const double *poses, int n_poses, const int64_t *pose_ids, const MapGrid &g, const MapRegions &r,
                   int64_t *stats)
{
    hipLaunchKernelGGL(map_insert_kernel<T>, dim3(blocks_for(total, INSERT_ROWS, NSC_MAP_INSERT_BLOCKS)), dim3(MAP_THREADS),
                       0, s, static_cast<const T *>(points), stride, reinterpret_cast<const long long *>(offsets), n_clouds,
                       total, poses, n_poses, reinterpret_cast<const long long *>(pose_ids), g, r.slots, r.cap,
                       reinterpret_cast<long long *>(stats));
}

// sizes the layout and the row addresses are computed for without overflow
inline bool sizes_supported(int64_t total_rows, int64_t max_voxels)
{
    return total_rows <= NSC_MAP_MAX_ROWS && max_voxels <= NSC_MAP_MAX_VOXELS;
}

}  // namespace

extern "C" {

void nsc_map_default_params(NscMapParams *p)
{
    if (!p) return;
    p->voxel_size = 0.5;
    p->origin[0] = p->origin[1] = p->origin[2] = 0.0;
}

size_t nsc_map_workspace_bytes(int64_t total_rows, int64_t max_voxels)
{
    if (total_rows < 0 || max_voxels < 0 || !sizes_supported(total_rows, max_voxels)) return 0;
    return map_regions(nullptr, total_rows, max_voxels).total;
}

int nsc_map_build(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_clouds,
                  int64_t total_rows, const double *poses, int32_t n_poses, const int64_t *pose_ids,
                  const NscMapParams *params, int64_t max_voxels, double *out_points, int64_t *info, int64_t *keys,
                  int64_t *stats, void *ws, size_t ws_bytes, void *stream)
{
    if (n_clouds < 0 || n_poses < 0 || total_rows < 0 || max_voxels < 0 || !params || !stats || !offsets) return NSC_EINVAL;
    if (dtype != NSC_MAP_DTYPE_F32 && dtype != NSC_MAP_DTYPE_F64) return NSC_EINVAL;
    if (stride_floats != 3 && !(stride_floats == 4 && dtype == NSC_MAP_DTYPE_F32)) return NSC_EINVAL;
    if (!(params->voxel_size > 0.0) || !isfinite(params->voxel_size) || !isfinite(params->origin[0]) ||
        !isfinite(params->origin[1]) || !isfinite(params->origin[2]))
        return NSC_EINVAL;
    if ((total_rows > 0 && !points) || (n_poses > 0 && !poses) || (max_voxels > 0 && (!out_points || !info || !keys)))
        return NSC_EINVAL;
    if (!sizes_supported(total_rows, max_voxels)) return NSC_EUNSUPPORTED;
    const MapRegions r = map_regions(ws, total_rows, max_voxels);
    if (r.total > 0 && (!ws || ws_bytes < r.total)) return NSC_EWORKSPACE;
    const MapGrid g{params->voxel_size, {params->origin[0], params->origin[1], params->origin[2]}};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 threads(MAP_THREADS);
    const long long slot_words = r.cap * SLOT_WORDS;
    hipLaunchKernelGGL(map_clear_kernel, dim3(blocks_for(slot_words > r.n_words ? slot_words : r.n_words, MAP_THREADS, MAP_SLOT_BLOCKS)),
                       threads, 0, s, reinterpret_cast<u64 *>(r.slots), slot_words, r.bits, r.n_words,
                       reinterpret_cast<long long *>(stats));
    if (dtype == NSC_MAP_DTYPE_F32)
        launch_insert<float>(s, points, stride_floats, offsets, n_clouds, total_rows, poses, n_poses, pose_ids, g, r, stats);
    else
        launch_insert<double>(s, points, stride_floats, offsets, n_clouds, total_rows, poses, n_poses, pose_ids, g, r, stats);
    const dim3 per_slot(blocks_for(r.cap, MAP_THREADS, MAP_SLOT_BLOCKS));
    hipLaunchKernelGGL(map_mark_kernel, per_slot, threads, 0, s, r.slots, r.cap, r.bits, r.n_words);
    hipLaunchKernelGGL(map_count_kernel, dim3(blocks_for(r.n_tiles, MAP_THREADS / 64, MAP_SLOT_BLOCKS)), threads, 0, s,
                       r.bits, r.n_words, r.n_tiles, r.prefix, r.tile);
    hipLaunchKernelGGL(map_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, r.tile, r.n_tiles, (long long)max_voxels,
                       reinterpret_cast<long long *>(stats));
    hipLaunchKernelGGL(map_write_kernel, per_slot, threads, 0, s, r.slots, r.cap, r.bits, r.prefix, r.tile, r.n_words,
                       (long long)max_voxels, out_points, reinterpret_cast<long long *>(info),
                       reinterpret_cast<long long *>(keys));
    return launch_status();
}

}  // extern "C"
