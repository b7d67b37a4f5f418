// nsc_map_rows.h -- what every call that takes the rows of nsc_map_build shares, in nsc_map.hip (builds, insertion, removal,
// replacement) and nsc_map_rays.hip (ray casting, row flags): the rows of a call and how they are dealt to the lanes
// (for_each_row), what becomes of a row (locate_row), the per-workgroup counters, the read-only probe of the kept index, and
// on the host an entry point's row arguments, their checks and the float32 / float64 dispatch (MapArgs).  Included at file
// scope; the namespace below gives each file its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nsc.h"
#include "nsc_util.h"
#include "nsc_voxel_hash.h"

namespace {

constexpr int MAP_THREADS = 256;
constexpr int MAP_SLOT_BLOCKS = 4096;                     // workgroups at most of the launches that walk slots or words
constexpr long long INSERT_ROWS = NSC_MAP_INSERT_ROWS;
static_assert(INSERT_ROWS % MAP_THREADS == 0, "a workgroup takes its rows in whole sweeps");

typedef unsigned long long u64;

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

// the rows of one call, as the two builds and the insertion take them
template <class T>
struct InsertRows {
    typedef T scalar;
    const T *pts; int stride; const long long *off; int n_clouds; long long total;
    const double *poses; int n_poses; const long long *ids;
    MapGrid g;
};

struct CloudSpan {                      // the rows [lo, hi) of cloud c, while c >= 0: kept while a lane's rows stay in it
    long long lo = 0, hi = 0;
    int c = -1;
};

// The one pass over the rows of a call: a workgroup takes INSERT_ROWS consecutive rows per sweep, a lane every
// MAP_THREADS-th of them, and body(row, span) runs per row, with a span of its own per sweep
template <class Body>
__device__ __forceinline__ void for_each_row(long long total, Body body)
{
    const long long n_sweeps = (total + INSERT_ROWS - 1) / INSERT_ROWS;
    for (long long sweep = blockIdx.x; sweep < n_sweeps; sweep += gridDim.x) {
        CloudSpan span;
        for (int k = 0; k < INSERT_ROWS / MAP_THREADS; ++k) {
            const long long row = sweep * INSERT_ROWS + (long long)k * MAP_THREADS + threadIdx.x;
            if (row >= total) break;
            body(row, span);
        }
    }
}

// the pose id of the cloud in `span`, or -1: a cloud without a pose, or a row of no cloud
template <class T>
__device__ __forceinline__ long long pose_of(const InsertRows<T> &in, const CloudSpan &span)
{
    const long long id = span.c < 0 ? -1 : (in.ids ? in.ids[span.c] : (long long)span.c);
    return id < 0 || id >= in.n_poses ? -1 : id;
}

// Row -> its cloud (in `span`), world point w, position u inside its voxel and key.  The one place that decides what
// becomes of a row: C_USED when it has a voxel, else the counter it falls into, the checks in this order
template <class T>
__device__ __forceinline__ int locate_row(const InsertRows<T> &in, long long row, CloudSpan &span, double w[3], double u[3],
                                          u64 &key)
{
    if (span.c < 0 || row < span.lo || row >= span.hi) span.c = cloud_of(in.off, in.n_clouds, row, span.lo, span.hi);
    const long long id = pose_of(in, span);
    if (id < 0) return C_NO_POSE;
    const T *q = in.pts + row * in.stride;
    const double p[3] = {(double)q[0], (double)q[1], (double)q[2]};
    place_row(in.poses + 16 * id, p, w);
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(w[0]) && isfinite(w[1]) && isfinite(w[2])))
        return C_NOT_FINITE;
    return world_voxel(w, in.g, u, key) ? C_USED : C_OUTSIDE;
}

// A lane's N counts, summed per workgroup and added with one integer atomic per counter
template <int N>
struct LaneCounters {
    long long n[N] = {};
    __device__ __forceinline__ void count(int kind)
    {
        for (int k = 0; k < N; ++k) n[k] += kind == k;
    }
    __device__ __forceinline__ void add_to(long long *stats) const { add_from(stats + NSC_MAP_STAT_USED); }
    // first[k] += the workgroup's count of kind k
    __device__ __forceinline__ void add_from(long long *first) const
    {
        __shared__ long long red[N][MAP_THREADS / 64];
        const int tid = threadIdx.x;
        for (int k = 0; k < N; ++k) {
            const long long v = nsc_wave_sum(n[k]);
            if ((tid & 63) == 0) red[k][tid >> 6] = v;
        }
        __syncthreads();
        if (tid < N) {
            long long v = 0;
            for (int w = 0; w < MAP_THREADS / 64; ++w) v += red[tid][w];
            if (v) atomicAdd(reinterpret_cast<u64 *>(&first[tid]), (u64)v);
        }
    }
};
typedef LaneCounters<N_COUNTERS> RowCounters;       // a lane's counts of what became of its rows, into the stats

// the slot of `key` in the kept index, or -1: the build's probe sequence, read only
__device__ __forceinline__ long long find_slot(const u64 *index, long long cap, u64 key)
{
    long long h = cap > 0 ? (long long)(mix64(key) % (u64)cap) : 0;
    for (long long probe = 0; probe < cap; ++probe) {
        const u64 e = index[2 * h];
        if (e == key + 1) return h;
        if (e == 0) return -1;
        h = next_slot(h, cap);
    }
    return -1;
}

inline unsigned blocks_for(long long n, long long per_block, long long most)
{
    const long long b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > most ? most : b));
}

// What the two builds and the calls on a kept map take alike: the rows, their poses, the grid, the capacity, the stats
struct MapArgs {
    const void *points; int32_t dtype, stride_floats; const int64_t *offsets; int32_t n_clouds; int64_t total_rows;
    const double *poses; int32_t n_poses; const int64_t *pose_ids; const NscMapParams *params; int64_t max_voxels;
    int64_t *stats;
    // NSC_OK, or what the call returns before anything is launched; `outputs`: the call's output tensors are all there
    int check(bool outputs) const
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
    MapGrid grid() const { return MapGrid{params->voxel_size, {params->origin[0], params->origin[1], params->origin[2]}}; }
    template <class T> InsertRows<T> rows() const
    {
        return InsertRows<T>{static_cast<const T *>(points), stride_floats, reinterpret_cast<const long long *>(offsets),
                             n_clouds, (long long)total_rows, poses, n_poses, reinterpret_cast<const long long *>(pose_ids),
                             grid()};
    }
    // launch(rows), the rows being float32 or float64 as `dtype` says
    template <class Launch> void with_rows(Launch launch) const
    {
        if (dtype == NSC_MAP_DTYPE_F32) launch(rows<float>()); else launch(rows<double>());
    }
};

}  // namespace
