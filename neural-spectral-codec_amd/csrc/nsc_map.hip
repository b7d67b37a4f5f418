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
// nsc_map_insert_dist adds rows to the kept tensors of such a build, with the result of a build over all rows; its eight
// launches are described where they stand, below the builds.  nsc_map_remove_dist takes rows out again and
// nsc_map_replace_dist moves clouds from one pose to another; their launches stand below the insertion's.
// nsc_map_rehash_dist moves a kept map to another capacity, without its emptied voxels; its four launches stand last.
//
// What the calls share stands once: for_each_row deals a call's rows to the lanes (the build's insert pass, the
// insertion's claim and accumulate passes, the removal's row pass), locate_row decides what becomes of a row, claim_slot
// and find_slot walk the probe sequence, touch_place keeps the touched list, dist_record makes a record, and on the host
// MapArgs / KeptArgs hold an entry point's arguments, their checks and the float32 / float64 dispatch.  What
// nsc_map_rays.hip takes the same way (for_each_row, locate_row, the counters, find_slot, MapArgs) is in nsc_map_rows.h.
//
// No float atomics anywhere: results are bitwise reproducible and do not depend on arrival order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nsc.h"
#include "nsc_eig3.h"
#include "nsc_map_rows.h"
#include "nsc_util.h"
#include "nsc_voxel_hash.h"

namespace {

constexpr long long TILE_ROWS = NSC_MAP_TILE_ROWS;
constexpr int TILE_WORDS = NSC_MAP_TILE_ROWS / 64;
constexpr int SCAN_THREADS = NSC_MAP_SCAN_THREADS;
static_assert(TILE_WORDS == 64, "one lane of a wave per bitmap word of a tile");

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

// The clear of a build: its table, its first-row bitmap and the stats.  per_slot: the words of a slot, a power of two;
// words 1 (first) and 6 (cloud_min) of a slot start at ~0
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

// what a row adds to its voxel beside the count, the first row and the clouds
__device__ __forceinline__ void add_row(MapSlot &s, const double w[3], const double u[3])
{
    for (int a = 0; a < 3; ++a)
        atomicAdd(reinterpret_cast<u64 *>(&s.sum[a]), (u64)__double2ll_rn(w[a] * FIX_SCALE));
}

// The nine integers a row adds to its distribution voxel, each handed to add(t, value) as it is made: q of the row's
// position u inside the voxel (t = 0 .. 2), then the six products xx xy xz yy yz zz (t = 3 .. 8)
template <class Add>
__device__ __forceinline__ void row_moments(const double u[3], Add add)
{
    long long q[3];
    for (int a = 0; a < 3; ++a) q[a] = __double2ll_rn(u[a] * MOMENT_SCALE) - (long long)MOMENT_HALF;
    for (int a = 0; a < 3; ++a) add(a, q[a]);
    int t = 3;
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) add(t++, q[a] * q[b]);
}

__device__ __forceinline__ void add_row(DistSlot &s, const double w[3], const double u[3])
{
    row_moments(u, [&s](int t, long long v) { atomicAdd(reinterpret_cast<u64 *>(t < 3 ? &s.sum[t] : &s.sq[t - 3]), (u64)v); });
}

// The slot of `key` in a table of `cap` slots whose slot h keeps key + 1 in keys[h * words] (0 = empty): found, or
// claimed with a 64-bit CAS (`claimed`); the probe visits every slot once at most; -1 when all hold other keys
__device__ __forceinline__ long long claim_slot(u64 *keys, int words, long long cap, u64 key, bool &claimed)
{
    claimed = false;
    long long h = cap > 0 ? (long long)(mix64(key) % (u64)cap) : 0;
    for (long long probe = 0; probe < cap; ++probe) {
        u64 e = peek(&keys[h * words]);
        if (e == 0) {
            e = atomicCAS(&keys[h * words], 0ULL, key + 1);
            if (e == 0) { e = key + 1; claimed = true; }
        }
        if (e == key + 1) return h;
        h = next_slot(h, cap);
    }
    return -1;
}

template <class T, class S>
__global__ __launch_bounds__(MAP_THREADS) void map_insert_kernel(InsertRows<T> in, S *tab, long long cap, long long *stats)
{
    RowCounters cnt;
    for_each_row(in.total, [&](long long row, CloudSpan &span) {
        double w[3], u[3];
        u64 key;
        int kind = locate_row(in, row, span, w, u, key);
        long long h = -1;
        bool claimed;
        if (kind == C_USED && (h = claim_slot(&tab[0].key, slot_words<S>(), cap, key, claimed)) < 0) kind = C_UNPLACED;
        cnt.count(kind);
        if (kind != C_USED) return;
        S &s = tab[h];
        const int c = span.c;
        // min and max only move one way: a value read before the atomic that already beats ours stays beaten
        if (peek(&s.first) > (u64)row) atomicMin(&s.first, (u64)row);
        if (peek(&s.cloud_min) > (u64)c) atomicMin(&s.cloud_min, (u64)c);
        if (peek(&s.cloud_max) < (u64)c + 1) atomicMax(&s.cloud_max, (u64)c + 1);
        atomicAdd(&s.count, 1ULL);
        add_row(s, w, u);
    });
    cnt.add_to(stats);
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
        const int v = w < n_words ? __popcll(bits[w]) : 0, inc = nsc_wave_scan(v);
        if (w < n_words) prefix[w] = (unsigned)(inc - v);
        if (lane == 63) tile[t] = inc;
    }
}

// exclusive scan of tile[0 .. n_tiles) in place by one workgroup of SCAN_THREADS -> the total, in every thread; a thread
// takes ceil(n_tiles / SCAN_THREADS) consecutive tiles
__device__ __forceinline__ long long scan_tiles(long long *tile, long long n_tiles)
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
    return part[SCAN_THREADS - 1];
}

__global__ __launch_bounds__(SCAN_THREADS) void map_scan_kernel(long long *tile, long long n_tiles, long long max_voxels,
                                                                long long *stats)
{
    const long long found = scan_tiles(tile, n_tiles);
    if (threadIdx.x == SCAN_THREADS - 1) {
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

struct DistRule {                        // what turns a voxel's integers into its record
    MapGrid g;
    double eigen_ratio, floor2;
    long long min_points;
};

// The record of a voxel (include/nsc.h): a function of its count, its nine sums (q first) and its key alone.  The one
// copy of this arithmetic: the build's write pass and the insertion's refresh pass call it, so their records agree bit
// for bit
__device__ inline void dist_record(u64 count, const long long sum[3], const long long sq[6], u64 key, const DistRule &r,
                                   double rec[16])
{
    const double n = (double)count;
    double m[3];
    for (int a = 0; a < 3; ++a) {
        const double k = (double)(long long)((key >> (a * KEY_BITS)) & (u64)KEY_MAX) - KEY_OFFSET;
        m[a] = (double)sum[a] / n;                             // mean of q
        rec[a] = r.g.origin[a] + ((k + 0.5) + m[a] / MOMENT_SCALE) * r.g.voxel;
    }
    const double unit = r.g.voxel / MOMENT_SCALE, unit2 = unit * unit;
    int t = 0;
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b, ++t) rec[3 + t] = ((double)sq[t] / n - m[a] * m[b]) * unit2;
    double A[3][3], V[3][3], inv[3];
    jacobi_eig3(rec + 3, A, V);
    const double top = fmax(A[0][0], fmax(A[1][1], A[2][2]));
    for (int i = 0; i < 3; ++i) inv[i] = 1.0 / fmax(fmax(A[i][i], r.eigen_ratio * top), r.floor2);
    t = 0;
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b, ++t)
            rec[9 + t] = (V[a][0] * V[b][0] * inv[0] + V[a][1] * V[b][1] * inv[1]) + V[a][2] * V[b][2] * inv[2];
    bool usable = (long long)count >= r.min_points;
    for (int e = 0; e < 15; ++e) usable = usable && isfinite(rec[e]);
    rec[15] = usable ? 1.0 : 0.0;
}

struct DistOut {                         // nsc_map_build_dist: a distribution record per voxel, and the kept index
    double *voxels; u64 *index; long long *moments;
    DistRule rule;
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
        double rec[16];
        dist_record(s.count, s.sum, s.sq, s.key - 1, rule, rec);
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

template <class S>
size_t workspace_bytes(int64_t total_rows, int64_t max_voxels)
{
    if (total_rows < 0 || max_voxels < 0 || total_rows > NSC_MAP_MAX_ROWS || max_voxels > NSC_MAP_MAX_VOXELS) return 0;
    return map_regions<S>(nullptr, total_rows, max_voxels).total;
}

// The six launches of a build over slots of type S; `out` is what the write pass writes per voxel beside info and keys
template <class S, class Out>
int launch_build(const MapArgs &a, int64_t *info, int64_t *keys, const Out &out, const MapRegions<S> &r, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 threads(MAP_THREADS), per_rows(blocks_for(a.total_rows, INSERT_ROWS, NSC_MAP_INSERT_BLOCKS));
    long long *st = reinterpret_cast<long long *>(a.stats);
    const long long n_slot_words = r.cap * slot_words<S>();
    hipLaunchKernelGGL(map_clear_kernel, dim3(blocks_for(n_slot_words > r.n_words ? n_slot_words : r.n_words, MAP_THREADS, MAP_SLOT_BLOCKS)),
                       threads, 0, s, reinterpret_cast<u64 *>(r.slots), n_slot_words, slot_words<S>(), r.bits, r.n_words, st);
    a.with_rows([&](auto in) {
        hipLaunchKernelGGL((map_insert_kernel<typename decltype(in)::scalar, S>), per_rows, threads, 0, s, in, r.slots, r.cap, st);
    });
    const dim3 per_slot(blocks_for(r.cap, MAP_THREADS, MAP_SLOT_BLOCKS));
    hipLaunchKernelGGL(map_mark_kernel<S>, per_slot, threads, 0, s, r.slots, r.cap, r.bits, r.n_words);
    hipLaunchKernelGGL(map_count_kernel, dim3(blocks_for(r.n_tiles, MAP_THREADS / 64, MAP_SLOT_BLOCKS)), threads, 0, s,
                       r.bits, r.n_words, r.n_tiles, r.prefix, r.tile);
    hipLaunchKernelGGL(map_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, r.tile, r.n_tiles, (long long)a.max_voxels, st);
    hipLaunchKernelGGL((map_write_kernel<S, Out>), per_slot, threads, 0, s, r.slots, r.cap,
                       MapPlaces{r.bits, r.prefix, r.tile, r.n_words}, (long long)a.max_voxels,
                       reinterpret_cast<long long *>(info), reinterpret_cast<long long *>(keys), out);
    return launch_status();
}

bool dist_ok(const NscMapDistParams *dist)
{
    return dist && dist->min_points >= 1 && dist->eigen_ratio > 0.0 && dist->eigen_ratio <= 1.0 && dist->sigma_floor > 0.0 &&
           isfinite(dist->sigma_floor);
}

// ---- nsc_map_insert_dist: rows added to a kept map ---------------------------------------------------------------------
// The kept index is the build's table: (key + 1, place) at the slots the build's probes walked, so new keys are claimed in
// it as the build claims them.  Nothing below walks the 2 max_voxels slots or the max_voxels records: every pass is over
// the call's rows, or over the places they reached.
//
// Launch sequence (8; the grids depend on total_rows alone):
//   clear       call_clear_kernel, the clear of every call on a kept map, on the call's first-row bitmap and its counters
//   claim       per row: the row's slot, found or claimed (64-bit CAS) along the build's probe sequence and kept in the
//               workspace; in the place word of a slot claimed in this call the smallest local row, PLACE_NEW | row
//               (atomic min); the counters of dropped, unplaced and used rows into the kept stats
//   mark        per row: the row a new slot's place word names sets its bit
//   count, scan map_count_kernel and map_scan_kernel as they are, on the call's bitmap: the new voxels in first-row order
//   assign      per first row of a new voxel: place = voxels written before the call + its rank; below max_voxels the
//               place word, the key and an empty info and moments row, else place ~0 as the build's overflow
//   accumulate  per row: integer atomics on info and moments of its place; the first row to reach a place in this call
//               (PLACE_TOUCHED, an atomic or on the place word) appends the slot to the touched list
//   refresh     per touched slot: PLACE_TOUCHED off, the record from dist_record; one thread folds the new voxels into
//               the kept stats and advances the cursor
// A map whose outputs are full (written == max_voxels before the call) can hold keyed slots with place ~0 from an
// earlier overflow, which a place word cannot tell from a slot claimed a moment ago.  No new voxel gets a place then, so
// only their number matters: the thread whose CAS claims the slot sets its own row's bit, and mark and assign do nothing.
constexpr u64 PLACE_NEW = 1ULL << 62;        // no place reaches these bits: places stay below NSC_MAP_MAX_VOXELS
constexpr u64 PLACE_TOUCHED = 1ULL << 61;
static_assert(NSC_MAP_MAX_VOXELS <= (1LL << 61) && NSC_MAP_MAX_ROWS <= (1LL << 61), "the flags lie above places and rows");
enum { CALL_FOUND = NSC_MAP_STAT_FOUND, CALL_WRITTEN = NSC_MAP_STAT_WRITTEN, CALL_TOUCHED, CALL_WORDS = NSC_MAP_STATS };

// The touched list of a call, of an insertion and of a removal: the first row to reach a place in this call (an atomic or
// of PLACE_TOUCHED on the place word decides which) appends the place's slot h.  `there` is the place word as the caller's
// guard read it: the one load serves both.  Returns the place, the flag stripped
__device__ __forceinline__ long long touch_place(u64 *place_word, u64 there, long long h, long long *touched, long long *call)
{
    if (!(there & PLACE_TOUCHED)) {
        there = atomicOr(place_word, PLACE_TOUCHED);
        if (!(there & PLACE_TOUCHED)) touched[atomicAdd(reinterpret_cast<u64 *>(&call[CALL_TOUCHED]), 1ULL)] = h;
    }
    return (long long)(there & ~PLACE_TOUCHED);
}

struct KeptMap {
    double *voxels; u64 *index; long long *info, *keys, *moments, *stats, *cursor;
    long long max_voxels;
    long long *counters;                // where the claim pass counts its rows: stats, or `placed` of a replacement
    // the outputs were full before this call; the stats' voxel counts stay as they were until the refresh pass
    __device__ bool full() const { return stats[NSC_MAP_STAT_WRITTEN] >= max_voxels; }
};

struct InsertRegions {
    u64 *bits; unsigned *prefix; long long *tile, *slot, *touched, *call;
    long long n_words, n_tiles;
    size_t total;
};

InsertRegions insert_regions(void *ws, long long total_rows)
{
    Carver c = {reinterpret_cast<uintptr_t>(ws), 0};
    InsertRegions r;
    r.n_words = (total_rows + 63) / 64;
    r.n_tiles = (total_rows + TILE_ROWS - 1) / TILE_ROWS;
    r.bits = c.take<u64>(r.n_words);
    r.prefix = c.take<unsigned>(r.n_words);
    r.tile = c.take<long long>(r.n_tiles);
    r.slot = c.take<long long>(total_rows);
    r.touched = c.take<long long>(total_rows);
    r.call = c.take<long long>(CALL_WORDS);
    r.total = c.o;
    return r;
}

template <class T>
__global__ __launch_bounds__(MAP_THREADS) void ins_claim_kernel(InsertRows<T> in, KeptMap m, u64 *bits, long long *slot)
{
    const long long cap = 2 * m.max_voxels;
    const bool full = m.full();
    RowCounters cnt;
    for_each_row(in.total, [&](long long row, CloudSpan &span) {
        double w[3], u[3];
        u64 key;
        int kind = locate_row(in, row, span, w, u, key);
        long long h = -1;
        bool claimed = false;
        if (kind == C_USED && (h = claim_slot(m.index, 2, cap, key, claimed)) < 0) kind = C_UNPLACED;
        cnt.count(kind);
        slot[row] = h;
        if (h < 0) return;
        if (full) {
            if (claimed) atomicOr(&bits[row >> 6], 1ULL << (row & 63));
            return;
        }
        // an empty slot's place word is ~0, which has PLACE_NEW set and is above every PLACE_NEW | row
        const u64 mine = PLACE_NEW | (u64)row, there = peek(&m.index[2 * h + 1]);
        if ((there & PLACE_NEW) && there > mine) atomicMin(&m.index[2 * h + 1], mine);
    });
    cnt.add_to(m.counters);
}

__global__ __launch_bounds__(MAP_THREADS) void ins_mark_kernel(KeptMap m, const long long *slot, long long total, u64 *bits)
{
    if (m.full()) return;
    for (long long row = (long long)blockIdx.x * MAP_THREADS + threadIdx.x; row < total; row += (long long)gridDim.x * MAP_THREADS) {
        const long long h = slot[row];
        if (h >= 0 && m.index[2 * h + 1] == (PLACE_NEW | (u64)row)) atomicOr(&bits[row >> 6], 1ULL << (row & 63));
    }
}

__global__ __launch_bounds__(MAP_THREADS) void ins_assign_kernel(KeptMap m, const long long *slot, long long total,
                                                                 MapPlaces places)
{
    if (m.full()) return;
    const long long written = m.stats[NSC_MAP_STAT_WRITTEN], row0 = m.cursor[0];
    for (long long row = (long long)blockIdx.x * MAP_THREADS + threadIdx.x; row < total; row += (long long)gridDim.x * MAP_THREADS) {
        const long long h = slot[row];
        if (h < 0 || m.index[2 * h + 1] != (PLACE_NEW | (u64)row)) continue;
        const long long pos = written + places.of((u64)row);
        if (pos >= m.max_voxels) { m.index[2 * h + 1] = ~0ULL; continue; }
        m.index[2 * h + 1] = (u64)pos;
        m.keys[pos] = (long long)(m.index[2 * h] - 1);
        m.info[4 * pos] = 0;
        m.info[4 * pos + 1] = row0 + row;
        m.info[4 * pos + 2] = INT64_MAX;
        m.info[4 * pos + 3] = -1;
        for (int t = 0; t < 9; ++t) m.moments[9 * pos + t] = 0;
    }
}

template <class T>
__global__ __launch_bounds__(MAP_THREADS) void ins_accumulate_kernel(InsertRows<T> in, KeptMap m, const long long *slot,
                                                                     long long *touched, long long *call)
{
    const long long cloud0 = m.cursor[1];
    for_each_row(in.total, [&](long long row, CloudSpan &span) {
        const long long h = slot[row];
        if (h < 0) return;
        const u64 there = peek(&m.index[2 * h + 1]);
        if (there & PLACE_NEW) return;                                 // ~0, a voxel past the outputs: its rows are counted, no more
        const long long pos = touch_place(&m.index[2 * h + 1], there, h, touched, call);
        // a row with a slot has a cloud, a pose, finite coordinates and a voxel: the claim pass found C_USED
        double w[3], u[3];
        u64 key;
        locate_row(in, row, span, w, u, key);
        const int c = span.c;
        long long *info = m.info + 4 * pos;
        const long long cloud = cloud0 + c;
        atomicAdd(reinterpret_cast<u64 *>(info), 1ULL);
        // min and max only move one way: a value read before the atomic that already beats ours stays beaten
        if ((long long)peek(reinterpret_cast<u64 *>(info + 2)) > cloud)
            __hip_atomic_fetch_min(info + 2, cloud, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((long long)peek(reinterpret_cast<u64 *>(info + 3)) < cloud)
            __hip_atomic_fetch_max(info + 3, cloud, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        long long *mo = m.moments + 9 * pos;
        row_moments(u, [mo](int t, long long v) { atomicAdd(reinterpret_cast<u64 *>(mo + t), (u64)v); });
    });
}

enum { PLACE_RECORD, PLACE_EMPTIED, PLACE_INCONSISTENT };

// The refresh of one touched slot, of an insertion and of a removal: PLACE_TOUCHED off, and the record of what the place
// now holds.  A positive count gives dist_record's record.  A count of 0 with nine zero moments is an emptied voxel, any
// other count below 1 an inconsistent one (an unmatched removal): both get the zero record, written as zeros, and keep
// their integers
__device__ __forceinline__ int refresh_place(const KeptMap &m, long long h, const DistRule &rule)
{
    const long long pos = (long long)(m.index[2 * h + 1] & ~PLACE_TOUCHED);
    m.index[2 * h + 1] = (u64)pos;
    const long long count = m.info[4 * pos], *mo = m.moments + 9 * pos;
    double rec[16];
    int kind = PLACE_RECORD;
    if (count > 0) {
        dist_record((u64)count, mo, mo + 3, m.index[2 * h] - 1, rule, rec);
    } else {
        bool zero = count == 0;
        for (int t = 0; t < 9; ++t) zero = zero && mo[t] == 0;
        kind = zero ? PLACE_EMPTIED : PLACE_INCONSISTENT;
        for (int e = 0; e < 16; ++e) rec[e] = 0.0;
    }
    for (int e = 0; e < 16; ++e) m.voxels[16 * pos + e] = rec[e];
    return kind;
}

__global__ __launch_bounds__(MAP_THREADS) void ins_refresh_kernel(KeptMap m, const long long *touched, const long long *call,
                                                                  DistRule rule, long long total, long long n_clouds)
{
    const long long n = call[CALL_TOUCHED];
    for (long long i = (long long)blockIdx.x * MAP_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * MAP_THREADS)
        refresh_place(m, touched[i], rule);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const long long found = m.stats[NSC_MAP_STAT_FOUND] + call[CALL_FOUND];
        m.stats[NSC_MAP_STAT_FOUND] = found;
        m.stats[NSC_MAP_STAT_WRITTEN] = min(found, m.max_voxels);
        if (m.counters != m.stats) {
            // a replacement: what became of the call's rows stays in `placed`; the map takes the rows it holds or lacks
            m.counters[NSC_MAP_STAT_FOUND] = call[CALL_FOUND];
            m.counters[NSC_MAP_STAT_WRITTEN] = min(found, m.max_voxels);
            m.stats[NSC_MAP_STAT_USED] += m.counters[NSC_MAP_STAT_USED];
            m.stats[NSC_MAP_STAT_UNPLACED] += m.counters[NSC_MAP_STAT_UNPLACED];
        }
        m.cursor[0] += total;
        m.cursor[1] += n_clouds;
    }
}

// The clear of every call on a kept map: the first-row bitmap and the counters of the insertion (bits, ins_call), the
// counters of the removal (rem_call, removed), and for a replacement `placed` and its cursor, set to the caller's bases.
// What a call does not have is null: an insertion alone has the first two, a removal alone the second two
__global__ __launch_bounds__(MAP_THREADS) void call_clear_kernel(u64 *bits, long long n_words, long long *ins_call,
                                                                 long long *rem_call, long long *removed, long long *placed,
                                                                 long long *cursor, long long first_row, long long first_cloud)
{
    const long long i0 = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
    for (long long i = i0; i < n_words; i += (long long)gridDim.x * MAP_THREADS) bits[i] = 0ULL;
    if (i0 < CALL_WORDS) {
        if (rem_call) rem_call[i0] = 0;
        if (ins_call) ins_call[i0] = 0;
        if (placed) placed[i0] = 0;
    }
    if (removed && i0 < NSC_MAP_REMOVE_STATS) removed[i0] = 0;
    if (i0 == 0 && cursor) { cursor[0] = first_row; cursor[1] = first_cloud; }
}

// the insertion's launches after its clear
template <class T>
void launch_insert_passes(const InsertRows<T> &in, const KeptMap &m, const DistRule &rule, const InsertRegions &r, hipStream_t s)
{
    const dim3 threads(MAP_THREADS), sweeps(blocks_for(in.total, INSERT_ROWS, NSC_MAP_INSERT_BLOCKS)),
        per_row(blocks_for(in.total, MAP_THREADS, MAP_SLOT_BLOCKS));
    hipLaunchKernelGGL(ins_claim_kernel<T>, sweeps, threads, 0, s, in, m, r.bits, r.slot);
    hipLaunchKernelGGL(ins_mark_kernel, per_row, threads, 0, s, m, r.slot, in.total, r.bits);
    hipLaunchKernelGGL(map_count_kernel, dim3(blocks_for(r.n_tiles, MAP_THREADS / 64, MAP_SLOT_BLOCKS)), threads, 0, s,
                       r.bits, r.n_words, r.n_tiles, r.prefix, r.tile);
    hipLaunchKernelGGL(map_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, r.tile, r.n_tiles, m.max_voxels, r.call);
    hipLaunchKernelGGL(ins_assign_kernel, per_row, threads, 0, s, m, r.slot, in.total,
                       MapPlaces{r.bits, r.prefix, r.tile, r.n_words});
    hipLaunchKernelGGL(ins_accumulate_kernel<T>, sweeps, threads, 0, s, in, m, r.slot, r.touched, r.call);
    hipLaunchKernelGGL(ins_refresh_kernel, per_row, threads, 0, s, m, r.touched, r.call, rule, in.total,
                       (long long)in.n_clouds);
}

template <class T>
void launch_insert_rows(const InsertRows<T> &in, const KeptMap &m, const DistRule &rule, const InsertRegions &r, hipStream_t s)
{
    long long *const none = nullptr;
    hipLaunchKernelGGL(call_clear_kernel, dim3(blocks_for(r.n_words, MAP_THREADS, MAP_SLOT_BLOCKS)), dim3(MAP_THREADS), 0, s,
                       r.bits, r.n_words, r.call, none, none, none, none, 0LL, 0LL);
    launch_insert_passes(in, m, rule, r, s);
}

// ---- nsc_map_remove_dist and nsc_map_replace_dist: rows taken out of a kept map, and clouds moved to other poses ---------
// A row finds the voxel it once went into by the build's probe, and what it added then is subtracted as integers: the
// record of a voxel that keeps rows is dist_record of what is left, as a build over the remaining rows gives it.  Nothing
// walks the slots or the records here either.
//
// Removal (NSC_MAP_REMOVE_LAUNCHES = 3; the grids depend on total_rows alone):
//   clear    the call's counters and `removed`
//   rows     per row: locate_row, a lookup of the kept index that claims nothing; a row whose key is absent or has place
//            ~0 is missing.  Else -1 on the count and the negated integers of row_moments on the moments; the first row to
//            reach a place in this call (PLACE_TOUCHED) appends the slot to the touched list
//   refresh  per touched slot: refresh_place; emptied and inconsistent voxels counted; one thread takes the removed rows
//            from the kept stats
// Replacement (NSC_MAP_REPLACE_LAUNCHES = 10): one clear for both halves, which also sets the workspace's own cursor to the
// caller's bases; rows and refresh of the removal under the old poses; the insertion's seven passes under the new poses,
// numbering from that cursor and counting into `placed`.
constexpr int REM_TOUCHED = NSC_MAP_REMOVE_STAT_TOUCHED, REM_EMPTIED = NSC_MAP_REMOVE_STAT_EMPTIED,
              REM_INCONSISTENT = NSC_MAP_REMOVE_STAT_INCONSISTENT;
static_assert(NSC_MAP_REMOVE_STAT_REMOVED == C_USED && NSC_MAP_REMOVE_STAT_NOT_FINITE == C_NOT_FINITE &&
                  NSC_MAP_REMOVE_STAT_OUTSIDE == C_OUTSIDE && NSC_MAP_REMOVE_STAT_NO_POSE == C_NO_POSE &&
                  NSC_MAP_REMOVE_STAT_MISSING == C_UNPLACED && NSC_MAP_REMOVE_STATS <= MAP_THREADS,
              "the row pass's counters are the first five entries of `removed`, which the clear's first threads zero");

struct RemoveRegions {
    long long *touched, *call, *cursor;
    size_t total;
};

// `with_cursor`: a replacement, whose insertion half numbers from two words of the workspace
RemoveRegions remove_regions(void *ws, size_t at, long long total_rows, bool with_cursor)
{
    Carver c = {reinterpret_cast<uintptr_t>(ws), at};
    RemoveRegions r;
    r.touched = c.take<long long>(total_rows);
    r.call = c.take<long long>(CALL_WORDS);
    r.cursor = with_cursor ? c.take<long long>(2) : nullptr;
    r.total = c.o;
    return r;
}

template <class T>
__global__ __launch_bounds__(MAP_THREADS) void rem_rows_kernel(InsertRows<T> in, KeptMap m, long long *touched, long long *call,
                                                               long long *removed)
{
    const long long cap = 2 * m.max_voxels;
    RowCounters cnt;
    for_each_row(in.total, [&](long long row, CloudSpan &span) {
        double w[3], u[3];
        u64 key;
        int kind = locate_row(in, row, span, w, u, key);
        long long pos = -1;
        if (kind == C_USED) {
            const long long h = find_slot(m.index, cap, key);
            const u64 there = h < 0 ? ~0ULL : peek(&m.index[2 * h + 1]);
            // ~0 has PLACE_NEW set: a voxel past the outputs holds no sums to take the row from
            if (!(there & PLACE_NEW) && (long long)(there & ~PLACE_TOUCHED) < m.max_voxels)
                pos = touch_place(&m.index[2 * h + 1], there, h, touched, call);
            else
                kind = C_UNPLACED;                                      // counted as missing
        }
        cnt.count(kind);
        if (kind != C_USED) return;
        atomicAdd(reinterpret_cast<u64 *>(m.info + 4 * pos), ~0ULL);                  // count - 1
        long long *mo = m.moments + 9 * pos;
        row_moments(u, [mo](int t, long long v) { atomicAdd(reinterpret_cast<u64 *>(mo + t), (u64)(-v)); });
    });
    cnt.add_from(removed);
}

__global__ __launch_bounds__(MAP_THREADS) void rem_refresh_kernel(KeptMap m, const long long *touched, const long long *call,
                                                                  DistRule rule, long long *removed)
{
    const long long n = call[CALL_TOUCHED];
    long long emptied = 0, inconsistent = 0;
    for (long long i = (long long)blockIdx.x * MAP_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * MAP_THREADS) {
        const int kind = refresh_place(m, touched[i], rule);
        emptied += kind == PLACE_EMPTIED;
        inconsistent += kind == PLACE_INCONSISTENT;
    }
    emptied = nsc_wave_sum(emptied);
    inconsistent = nsc_wave_sum(inconsistent);
    if ((threadIdx.x & 63) == 0) {
        if (emptied) atomicAdd(reinterpret_cast<u64 *>(&removed[REM_EMPTIED]), (u64)emptied);
        if (inconsistent) atomicAdd(reinterpret_cast<u64 *>(&removed[REM_INCONSISTENT]), (u64)inconsistent);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        removed[REM_TOUCHED] = n;
        m.stats[NSC_MAP_STAT_USED] -= removed[NSC_MAP_REMOVE_STAT_REMOVED];       // final: the row pass has ended
    }
}

// the removal's launches after the clear
template <class T>
void launch_remove_passes(const InsertRows<T> &in, const KeptMap &m, const DistRule &rule, const RemoveRegions &r,
                          long long *removed, hipStream_t s)
{
    const dim3 threads(MAP_THREADS);
    hipLaunchKernelGGL(rem_rows_kernel<T>, dim3(blocks_for(in.total, INSERT_ROWS, NSC_MAP_INSERT_BLOCKS)), threads, 0, s, in, m,
                       r.touched, r.call, removed);
    hipLaunchKernelGGL(rem_refresh_kernel, dim3(blocks_for(in.total, MAP_THREADS, MAP_SLOT_BLOCKS)), threads, 0, s, m,
                       r.touched, r.call, rule, removed);
}

template <class T>
void launch_remove_rows(const InsertRows<T> &in, const KeptMap &m, const DistRule &rule, const RemoveRegions &r,
                        long long *removed, hipStream_t s)
{
    long long *const none = nullptr;
    hipLaunchKernelGGL(call_clear_kernel, dim3(1), dim3(MAP_THREADS), 0, s, static_cast<u64 *>(nullptr), 0LL, none, r.call,
                       removed, none, none, 0LL, 0LL);
    launch_remove_passes(in, m, rule, r, removed, s);
}

template <class T>
void launch_replace_rows(const InsertRows<T> &old_rows, const double *new_poses, KeptMap m, const DistRule &rule,
                         const InsertRegions &ins, const RemoveRegions &rem, long long first_row, long long first_cloud,
                         long long *removed, long long *placed, hipStream_t s)
{
    hipLaunchKernelGGL(call_clear_kernel, dim3(blocks_for(ins.n_words, MAP_THREADS, MAP_SLOT_BLOCKS)), dim3(MAP_THREADS), 0, s,
                       ins.bits, ins.n_words, ins.call, rem.call, removed, placed, rem.cursor, first_row, first_cloud);
    launch_remove_passes(old_rows, m, rule, rem, removed, s);
    InsertRows<T> new_rows = old_rows;
    new_rows.poses = new_poses;
    m.cursor = rem.cursor;
    m.counters = placed;
    launch_insert_passes(new_rows, m, rule, ins, s);
}

// ---- nsc_map_rehash_dist: a kept map moved to another capacity, its emptied voxels left behind ------------------------
// A record is a function of count, moments and key alone, so the map at another capacity is its voxels copied by bits and
// an index keyed anew by the build's probe: passes over the max_voxels places, no row read and no record evaluated.
//
// Launch sequence (NSC_MAP_REHASH_LAUNCHES = 4; the grids depend on max_voxels and new_max_voxels alone):
//   clear   new_index to (0, ~0) and `rehashed` to 0
//   count   per tile of NSC_MAP_TILE_ROWS old places: which are kept (a ballot and its popcount per wave of 64 places), the
//           tile's number into tile_base; the inconsistent voxels among them counted
//   scan    one workgroup: tile_base scanned in place, the total behind it; new_stats, new_cursor and `rehashed`
//   move    one workgroup per tile: the kept flags again, ranks by ballot prefix, the tile's kept places as a list in LDS
//           and new_place of every place of the tile.  The tile's destination is the range [tile_base[t], tile_base[t+1])
//           of each tensor: records, info, moments and keys are copied as flat arrays, lane i taking word i of the range,
//           so stores are contiguous and loads come in whole records.  Then one lane per kept voxel claims its key's slot
//           in new_index (claim_slot, as the build) and stores the place
constexpr int TILE_ROUNDS = NSC_MAP_TILE_ROWS / MAP_THREADS;        // sweeps of a workgroup over the places of a tile
constexpr int MAP_WAVES = MAP_THREADS / 64;
constexpr int TILE_SEGMENTS = TILE_ROUNDS * MAP_WAVES;             // runs of 64 places, one ballot each, in ascending place
static_assert(TILE_SEGMENTS == 64, "one lane of a wave per segment of a tile");

enum { OLD_DROPPED, OLD_KEPT, OLD_INCONSISTENT };

struct RehashSource {
    const u64 *voxels; const long long *info, *keys, *moments, *stats;
    long long max_voxels;
    int keep_emptied;
    // the places that hold a voxel: read on the device, and held inside the tensors whatever the stats say
    __device__ long long written() const { return max(0LL, min((long long)stats[NSC_MAP_STAT_WRITTEN], max_voxels)); }
    // what becomes of old place p: nothing is read at or past `written`
    __device__ int kind(long long p, long long written) const
    {
        if (p >= written) return OLD_DROPPED;
        const long long count = info[4 * p];
        if (count > 0) return OLD_KEPT;
        bool zero = count == 0;
        if (moments)
            for (int t = 0; t < 9; ++t) zero = zero && moments[9 * p + t] == 0;
        if (!zero) return OLD_INCONSISTENT;
        return keep_emptied ? OLD_KEPT : OLD_DROPPED;
    }
};

struct RehashDest {
    u64 *voxels, *index; long long *info, *keys, *moments;
    long long max_voxels;
};

__global__ __launch_bounds__(MAP_THREADS) void rehash_clear_kernel(u64 *index, long long index_words, long long *rehashed)
{
    const long long i0 = (long long)blockIdx.x * MAP_THREADS + threadIdx.x;
    for (long long i = i0; i < index_words; i += (long long)gridDim.x * MAP_THREADS) index[i] = (i & 1) ? ~0ULL : 0ULL;
    if (i0 < NSC_MAP_REHASH_STATS) rehashed[i0] = 0;
}

__global__ __launch_bounds__(MAP_THREADS) void rehash_count_kernel(RehashSource src, long long n_tiles, long long *tile_base,
                                                                   long long *rehashed)
{
    __shared__ int part[2][MAP_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6;
    const long long written = src.written();
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        int kept = 0, bad = 0;                                           // the same in every lane of a wave
        for (int r = 0; r < TILE_ROUNDS; ++r) {
            const int k = src.kind(t * TILE_ROWS + r * MAP_THREADS + tid, written);
            kept += __popcll(__ballot(k != OLD_DROPPED));
            bad += __popcll(__ballot(k == OLD_INCONSISTENT));
        }
        if ((tid & 63) == 0) { part[0][wave] = kept; part[1][wave] = bad; }
        __syncthreads();
        if (tid == 0) {
            int n = 0, b = 0;
            for (int w = 0; w < MAP_WAVES; ++w) { n += part[0][w]; b += part[1][w]; }
            tile_base[t] = n;
            if (b) atomicAdd(reinterpret_cast<u64 *>(&rehashed[NSC_MAP_REHASH_STAT_INCONSISTENT]), (u64)b);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void rehash_scan_kernel(RehashSource src, const long long *cursor, long long n_tiles,
                                                                   long long new_max_voxels, long long *tile_base,
                                                                   long long *new_stats, long long *new_cursor,
                                                                   long long *rehashed)
{
    const long long kept = scan_tiles(tile_base, n_tiles);
    const int tid = threadIdx.x;
    if (tid == SCAN_THREADS - 1) {
        const long long written = src.written(), placed = min(kept, new_max_voxels);
        tile_base[n_tiles] = kept;
        new_stats[NSC_MAP_STAT_FOUND] = kept;
        new_stats[NSC_MAP_STAT_WRITTEN] = placed;
        rehashed[NSC_MAP_REHASH_STAT_KEPT] = kept;
        rehashed[NSC_MAP_REHASH_STAT_EMPTIED] = written - kept;
        rehashed[NSC_MAP_REHASH_STAT_SOURCE_UNPLACED] = src.stats[NSC_MAP_STAT_FOUND] - written;
        rehashed[NSC_MAP_REHASH_STAT_UNPLACED] = kept - placed;
    }
    if (tid >= NSC_MAP_STAT_USED && tid < NSC_MAP_STATS) new_stats[tid] = src.stats[tid];
    if (cursor && tid < 2) new_cursor[tid] = cursor[tid];
}

__global__ __launch_bounds__(MAP_THREADS) void rehash_move_kernel(RehashSource src, RehashDest dst, long long n_tiles,
                                                                  const long long *tile_base, long long *new_place,
                                                                  long long *rehashed)
{
    __shared__ int list[NSC_MAP_TILE_ROWS];                              // the tile's kept places, counted from its first
    __shared__ int seg[TILE_SEGMENTS + 1];                              // kept places in front of each segment; the tile's
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long written = src.written(), cap = 2 * dst.max_voxels;
    long long full = 0;
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const long long p0 = t * TILE_ROWS, q0 = tile_base[t];
        unsigned flags = 0;                                              // bit r: this lane's place of sweep r is kept
        for (int r = 0; r < TILE_ROUNDS; ++r) {
            const bool keep = src.kind(p0 + r * MAP_THREADS + tid, written) != OLD_DROPPED;
            const u64 b = __ballot(keep);
            flags |= (unsigned)keep << r;
            if (lane == 0) seg[r * MAP_WAVES + wave] = __popcll(b);
        }
        __syncthreads();
        if (wave == 0) {
            const int v = seg[lane], inc = nsc_wave_scan(v);
            seg[lane] = inc - v;
            if (lane == 63) seg[TILE_SEGMENTS] = inc;
        }
        __syncthreads();
        for (int r = 0; r < TILE_ROUNDS; ++r) {
            const bool keep = (flags >> r) & 1u;
            const u64 b = __ballot(keep);
            const int j = seg[r * MAP_WAVES + wave] + __popcll(b & ((1ULL << lane) - 1ULL));
            if (keep) list[j] = r * MAP_THREADS + tid;
            const long long p = p0 + r * MAP_THREADS + tid;
            if (p < src.max_voxels) new_place[p] = keep && q0 + j < dst.max_voxels ? q0 + j : -1;
        }
        __syncthreads();
        // k kept places in this tile, the first `fit` of them with a place in the destination
        const int k = seg[TILE_SEGMENTS];
        const int fit = (int)max(0LL, min((long long)k, dst.max_voxels - q0));
        for (int i = tid; i < 16 * fit; i += MAP_THREADS) dst.voxels[16 * q0 + i] = src.voxels[16 * (p0 + list[i >> 4]) + (i & 15)];
        for (int i = tid; i < 4 * fit; i += MAP_THREADS) dst.info[4 * q0 + i] = src.info[4 * (p0 + list[i >> 2]) + (i & 3)];
        if (src.moments)
            for (int i = tid; i < 9 * fit; i += MAP_THREADS) dst.moments[9 * q0 + i] = src.moments[9 * (p0 + list[i / 9]) + i % 9];
        for (int j = tid; j < k; j += MAP_THREADS) {
            const long long key = src.keys[p0 + list[j]];
            if (j < fit) dst.keys[q0 + j] = key;
            bool claimed;
            const long long h = claim_slot(dst.index, 2, cap, (u64)key, claimed);
            // a voxel past the outputs keeps its key with place ~0, the build's overflow rule
            if (h < 0) ++full; else dst.index[2 * h + 1] = j < fit ? (u64)(q0 + j) : ~0ULL;
        }
        __syncthreads();                                                 // list and seg are the next tile's
    }
    full = nsc_wave_sum(full);
    if (lane == 0 && full) atomicAdd(reinterpret_cast<u64 *>(&rehashed[NSC_MAP_REHASH_STAT_TABLE_FULL]), (u64)full);
}

// MapArgs and the kept tensors: what nsc_map_build_dist makes and the three calls on a kept map change
struct KeptArgs : MapArgs {
    const NscMapDistParams *dist;
    double *voxels; uint64_t *index; int64_t *info, *keys, *moments;
    // NSC_OK, or the refusal of nsc_map_build_dist, and of a missing `moments` where the call needs them
    int check(bool need_moments) const
    {
        if (const int st = MapArgs::check(voxels && index && info && keys)) return st;
        return dist_ok(dist) && (moments || !need_moments) ? NSC_OK : NSC_EINVAL;
    }
    DistRule rule() const
    {
        return DistRule{grid(), dist->eigen_ratio, dist->sigma_floor * dist->sigma_floor, (long long)dist->min_points};
    }
    KeptMap map(int64_t *cursor) const
    {
        return KeptMap{voxels, reinterpret_cast<u64 *>(index), reinterpret_cast<long long *>(info),
                       reinterpret_cast<long long *>(keys), reinterpret_cast<long long *>(moments),
                       reinterpret_cast<long long *>(stats), reinterpret_cast<long long *>(cursor), (long long)max_voxels,
                       reinterpret_cast<long long *>(stats)};
    }
};

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
    const MapArgs a{points, dtype, stride_floats, offsets, n_clouds, total_rows, poses, n_poses, pose_ids, params, max_voxels,
                    stats};
    if (const int st = a.check(out_points && info && keys)) return st;
    const MapRegions<MapSlot> r = map_regions<MapSlot>(ws, total_rows, max_voxels);
    if (r.total > 0 && (!ws || ws_bytes < r.total)) return NSC_EWORKSPACE;
    return launch_build(a, info, keys, CentroidOut{out_points}, r, stream);
}

int nsc_map_build_dist(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_clouds,
                       int64_t total_rows, const double *poses, int32_t n_poses, const int64_t *pose_ids,
                       const NscMapParams *params, const NscMapDistParams *dist, int64_t max_voxels, double *voxels,
                       uint64_t *index, int64_t *info, int64_t *keys, int64_t *moments, int64_t *stats, void *ws,
                       size_t ws_bytes, void *stream)
{
    const KeptArgs a{{points, dtype, stride_floats, offsets, n_clouds, total_rows, poses, n_poses, pose_ids, params,
                      max_voxels, stats}, dist, voxels, index, info, keys, moments};
    if (const int st = a.check(false)) return st;
    const MapRegions<DistSlot> r = map_regions<DistSlot>(ws, total_rows, max_voxels);
    if (r.total > 0 && (!ws || ws_bytes < r.total)) return NSC_EWORKSPACE;
    const DistOut out{voxels, reinterpret_cast<u64 *>(index), reinterpret_cast<long long *>(moments), a.rule()};
    return launch_build(a, info, keys, out, r, stream);
}

size_t nsc_map_insert_workspace_bytes(int64_t total_rows)
{
    if (total_rows < 0 || total_rows > NSC_MAP_MAX_ROWS) return 0;
    return insert_regions(nullptr, total_rows).total;
}

int nsc_map_insert_dist(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_clouds,
                        int64_t total_rows, const double *poses, int32_t n_poses, const int64_t *pose_ids,
                        const NscMapParams *params, const NscMapDistParams *dist, int64_t max_voxels, double *voxels,
                        uint64_t *index, int64_t *info, int64_t *keys, int64_t *moments, int64_t *stats, int64_t *cursor,
                        void *ws, size_t ws_bytes, void *stream)
{
    const KeptArgs a{{points, dtype, stride_floats, offsets, n_clouds, total_rows, poses, n_poses, pose_ids, params,
                      max_voxels, stats}, dist, voxels, index, info, keys, moments};
    if (const int st = a.check(true)) return st;
    if (!cursor) return NSC_EINVAL;
    const InsertRegions r = insert_regions(ws, total_rows);
    if (!ws || ws_bytes < r.total) return NSC_EWORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    a.with_rows([&](auto in) { launch_insert_rows(in, a.map(cursor), a.rule(), r, s); });
    return launch_status();
}

size_t nsc_map_remove_workspace_bytes(int64_t total_rows)
{
    if (total_rows < 0 || total_rows > NSC_MAP_MAX_ROWS) return 0;
    return remove_regions(nullptr, 0, total_rows, false).total;
}

size_t nsc_map_replace_workspace_bytes(int64_t total_rows)
{
    if (total_rows < 0 || total_rows > NSC_MAP_MAX_ROWS) return 0;
    return remove_regions(nullptr, insert_regions(nullptr, total_rows).total, total_rows, true).total;
}

int nsc_map_remove_dist(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_clouds,
                        int64_t total_rows, const double *poses, int32_t n_poses, const int64_t *pose_ids,
                        const NscMapParams *params, const NscMapDistParams *dist, int64_t max_voxels, double *voxels,
                        uint64_t *index, int64_t *info, int64_t *keys, int64_t *moments, int64_t *stats, int64_t *removed,
                        void *ws, size_t ws_bytes, void *stream)
{
    const KeptArgs a{{points, dtype, stride_floats, offsets, n_clouds, total_rows, poses, n_poses, pose_ids, params,
                      max_voxels, stats}, dist, voxels, index, info, keys, moments};
    if (const int st = a.check(true)) return st;
    if (!removed) return NSC_EINVAL;
    const RemoveRegions r = remove_regions(ws, 0, total_rows, false);
    if (!ws || ws_bytes < r.total) return NSC_EWORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    long long *rem = reinterpret_cast<long long *>(removed);
    a.with_rows([&](auto in) { launch_remove_rows(in, a.map(nullptr), a.rule(), r, rem, s); });
    return launch_status();
}

int nsc_map_replace_dist(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_clouds,
                         int64_t total_rows, const double *old_poses, const double *new_poses, int32_t n_poses,
                         const int64_t *pose_ids, const NscMapParams *params, const NscMapDistParams *dist,
                         int64_t max_voxels, double *voxels, uint64_t *index, int64_t *info, int64_t *keys, int64_t *moments,
                         int64_t *stats, int64_t first_row, int64_t first_cloud, int64_t *removed, int64_t *placed, void *ws,
                         size_t ws_bytes, void *stream)
{
    const KeptArgs a{{points, dtype, stride_floats, offsets, n_clouds, total_rows, old_poses, n_poses, pose_ids, params,
                      max_voxels, stats}, dist, voxels, index, info, keys, moments};
    if (const int st = a.check(true)) return st;
    if ((n_poses > 0 && !new_poses) || !removed || !placed || first_row < 0 || first_cloud < 0) return NSC_EINVAL;
    const InsertRegions ins = insert_regions(ws, total_rows);
    const RemoveRegions rem = remove_regions(ws, ins.total, total_rows, true);
    if (!ws || ws_bytes < rem.total) return NSC_EWORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    long long *rm = reinterpret_cast<long long *>(removed), *pl = reinterpret_cast<long long *>(placed);
    a.with_rows([&](auto old_rows) {
        launch_replace_rows(old_rows, new_poses, a.map(nullptr), a.rule(), ins, rem, (long long)first_row, (long long)first_cloud,
                            rm, pl, s);
    });
    return launch_status();
}

int nsc_map_rehash_dist(const double *voxels, const int64_t *info, const int64_t *keys, const int64_t *moments,
                        const int64_t *stats, const int64_t *cursor, int64_t max_voxels, int32_t keep_emptied,
                        double *new_voxels, uint64_t *new_index, int64_t *new_info, int64_t *new_keys, int64_t *new_moments,
                        int64_t *new_stats, int64_t *new_cursor, int64_t new_max_voxels, int64_t *new_place,
                        int64_t *tile_base, int64_t *rehashed, void *stream)
{
    if (max_voxels < 0 || new_max_voxels < 1) return NSC_EINVAL;
    if (!stats || !new_voxels || !new_index || !new_info || !new_keys || !new_stats || !tile_base || !rehashed) return NSC_EINVAL;
    if (max_voxels > 0 && !(voxels && info && keys && new_place)) return NSC_EINVAL;
    if (!moments != !new_moments || !cursor != !new_cursor) return NSC_EINVAL;
    // out of place: both maps exist while the call runs
    if (new_voxels == voxels || new_info == info || new_keys == keys || new_stats == stats ||
        (moments && new_moments == moments) || (cursor && new_cursor == cursor))
        return NSC_EINVAL;
    if (max_voxels > NSC_MAP_MAX_VOXELS || new_max_voxels > NSC_MAP_MAX_VOXELS) return NSC_EUNSUPPORTED;
    const RehashSource src{reinterpret_cast<const u64 *>(voxels), reinterpret_cast<const long long *>(info),
                           reinterpret_cast<const long long *>(keys), reinterpret_cast<const long long *>(moments),
                           reinterpret_cast<const long long *>(stats), (long long)max_voxels, keep_emptied != 0};
    const RehashDest dst{reinterpret_cast<u64 *>(new_voxels), reinterpret_cast<u64 *>(new_index),
                         reinterpret_cast<long long *>(new_info), reinterpret_cast<long long *>(new_keys),
                         reinterpret_cast<long long *>(new_moments), (long long)new_max_voxels};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long n_tiles = (max_voxels + TILE_ROWS - 1) / TILE_ROWS, index_words = 4 * (long long)new_max_voxels;
    long long *base = reinterpret_cast<long long *>(tile_base), *re = reinterpret_cast<long long *>(rehashed);
    const dim3 threads(MAP_THREADS), per_tile(blocks_for(n_tiles, 1, MAP_SLOT_BLOCKS));
    hipLaunchKernelGGL(rehash_clear_kernel, dim3(blocks_for(index_words, MAP_THREADS, MAP_SLOT_BLOCKS)), threads, 0, s,
                       dst.index, index_words, re);
    hipLaunchKernelGGL(rehash_count_kernel, per_tile, threads, 0, s, src, n_tiles, base, re);
    hipLaunchKernelGGL(rehash_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, src, reinterpret_cast<const long long *>(cursor),
                       n_tiles, (long long)new_max_voxels, base, reinterpret_cast<long long *>(new_stats),
                       reinterpret_cast<long long *>(new_cursor), re);
    hipLaunchKernelGGL(rehash_move_kernel, per_tile, threads, 0, s, src, dst, n_tiles, base,
                       reinterpret_cast<long long *>(new_place), re);
    return launch_status();
}

}  // extern "C"
