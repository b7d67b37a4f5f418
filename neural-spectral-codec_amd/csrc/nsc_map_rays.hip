// nsc_map_rays.hip -- evidence of free space for a kept distribution map (nsc_map_build_dist): the rays from the sensor to
// the rows of later scans are walked through the voxel grid, and a voxel whose Gaussian a ray passes within `gate` standard
// deviations of, before the ray ends, is counted as crossed (nsc_map_cast_rays).  Rows whose own voxel has been crossed
// often enough for the rows it holds are flagged (nsc_map_flag_rows), so that a caller can take exactly those rows out with
// nsc_map_remove_dist.  The definition is in include/nsc.h; tests/map_rays_restatement.py restates it in float64 numpy.
//
// Launch sequence (all on the caller's stream, nothing allocated, copied or synchronised; the grids depend on total_rows
// alone):
//   nsc_map_cast_rays   clear  the eight ray_stats
//                       cast   one lane per ray, dealt as the build deals its rows (for_each_row): locate_row places the
//                              row, the walk steps from face to face with the next face recomputed from the voxel every
//                              step, and each voxel of the walk is looked up in the kept index; only after an index hit
//                              is the record's 128-byte line read.  crossed[place] += 1 by an int64 atomic; the counters
//                              per lane, summed per workgroup
//   nsc_map_flag_rows   clear  the four flag_stats
//                       flag   one lane per row: its voxel by locate_row and the index, count and crossed of its place
// Both walks are bounded whatever the input: the ray's by max_steps (from the host), the probe by the table's capacity.
// The map is read only, so a cast can run beside a registration; integer atomics only, so two calls agree by bits and the
// cloud order changes nothing.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nsc.h"
#include "nsc_fill.h"
#include "nsc_map_rows.h"
#include "nsc_util.h"
#include "nsc_voxel_hash.h"

namespace {

constexpr int REC = NSC_MAP_VOXEL_DOUBLES;
constexpr int C_SHORT = C_UNPLACED;                 // the fifth kind of a ray, where a row's is "unplaced"
static_assert(NSC_MAP_RAY_STAT_CAST == C_USED && NSC_MAP_RAY_STAT_NOT_FINITE == C_NOT_FINITE &&
                  NSC_MAP_RAY_STAT_OUTSIDE == C_OUTSIDE && NSC_MAP_RAY_STAT_NO_POSE == C_NO_POSE &&
                  NSC_MAP_RAY_STAT_SHORT == C_SHORT && NSC_MAP_RAY_STATS == 8,
              "what became of a ray is counted in the first five ray_stats, in locate_row's order");

struct RayRule {                        // NscMapRayParams as the kernel takes them
    double min_range, max_range, end_margin, gate2;
    long long max_steps;
};

struct RayMap {                         // the kept map, read only
    const double *voxels; const u64 *index;
    long long max_voxels;
};

// Does the ray o + t D, t in [ta, tb], come within the gate of the voxel with coordinates k?  No, if the voxel is outside
// the grid, not in the index, without a place, the ray's own end voxel or not usable
__device__ __forceinline__ bool ray_crosses(const RayMap &m, const double k[3], u64 end_key, const double o[3],
                                            const double D[3], double ta, double tb, double gate2, long long &place)
{
    const double kx = k[0] + KEY_OFFSET, ky = k[1] + KEY_OFFSET, kz = k[2] + KEY_OFFSET;
    if (!(kx >= 0.0 && kx <= (double)KEY_MAX && ky >= 0.0 && ky <= (double)KEY_MAX && kz >= 0.0 && kz <= (double)KEY_MAX))
        return false;
    const u64 key = pack_key((long long)kx, (long long)ky, (long long)kz);
    if (key == end_key) return false;
    const long long h = find_slot(m.index, 2 * m.max_voxels, key);
    if (h < 0) return false;
    const u64 at = m.index[2 * h + 1];
    if (at >= (u64)m.max_voxels) return false;                          // ~0 too: a voxel past the outputs
    const double2 *r2 = reinterpret_cast<const double2 *>(m.voxels + REC * (long long)at);   // one aligned 128-byte line
    const double2 a0 = r2[0], a1 = r2[1], a4 = r2[4], a5 = r2[5], a6 = r2[6], a7 = r2[7];
    if (a7.y != 1.0) return false;
    const double O[3][3] = {{a4.y, a5.x, a5.y}, {a5.x, a6.x, a6.y}, {a5.y, a6.y, a7.x}};
    const double a[3] = {o[0] - a0.x, o[1] - a0.y, o[2] - a1.x};
    double ea[3], eD[3];
    for (int r = 0; r < 3; ++r) {
        ea[r] = (O[r][0] * a[0] + O[r][1] * a[1]) + O[r][2] * a[2];
        eD[r] = (O[r][0] * D[0] + O[r][1] * D[1]) + O[r][2] * D[2];
    }
    const double num = (D[0] * ea[0] + D[1] * ea[1]) + D[2] * ea[2];
    const double den = (D[0] * eD[0] + D[1] * eD[1]) + D[2] * eD[2];
    double t = den > 0.0 ? -num / den : ta;
    t = fmin(fmax(t, ta), tb);
    const double x[3] = {a[0] + t * D[0], a[1] + t * D[1], a[2] + t * D[2]};
    double ex[3];
    for (int r = 0; r < 3; ++r) ex[r] = (O[r][0] * x[0] + O[r][1] * x[1]) + O[r][2] * x[2];
    const double s = (x[0] * ex[0] + x[1] * ex[1]) + x[2] * ex[2];
    place = (long long)at;
    return s <= gate2;
}

template <class T>
__global__ __launch_bounds__(MAP_THREADS) void ray_cast_kernel(InsertRows<T> in, RayMap m, RayRule rule, long long *crossed,
                                                               long long *stats)
{
    LaneCounters<NSC_MAP_RAY_STATS> cnt;
    for_each_row(in.total, [&](long long row, CloudSpan &span) {
        double w[3], u[3], o[3] = {0.0, 0.0, 0.0};
        u64 end_key, key;
        int kind = locate_row(in, row, span, w, u, end_key);
        if (kind == C_USED) {
            const double *P = in.poses + 16 * pose_of(in, span);
            for (int a = 0; a < 3; ++a) o[a] = P[4 * a + 3];
            if (!world_voxel(o, in.g, u, key)) kind = C_OUTSIDE;          // o is finite where w is
        }
        double fo[3], d[3], D[3], t0 = 0.0, t1 = 0.0;
        if (kind == C_USED) {
            for (int a = 0; a < 3; ++a) {
                fo[a] = (o[a] - in.g.origin[a]) / in.g.voxel;
                d[a] = (w[a] - in.g.origin[a]) / in.g.voxel - fo[a];
                D[a] = w[a] - o[a];
            }
            const double L = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) * in.g.voxel;
            t0 = rule.min_range / L;
            t1 = fmin(1.0 - rule.end_margin / L, rule.max_range / L);
            if (!(L > 0.0) || !(t0 < t1)) kind = C_SHORT;
        }
        cnt.count(kind);
        if (kind != C_USED) return;
        double k[3];
        for (int a = 0; a < 3; ++a) k[a] = floor(fo[a] + t0 * d[a]);
        double ta = t0;
        long long visited = 0, hits = 0;
        bool ended = false;
        for (long long step = 0; step < rule.max_steps; ++step) {
            // the next face per axis, from k itself: nothing is accumulated along the ray
            double tn[3];
            for (int a = 0; a < 3; ++a)
                tn[a] = d[a] > 0.0 ? ((k[a] + 1.0) - fo[a]) / d[a] : d[a] < 0.0 ? (k[a] - fo[a]) / d[a] : INFINITY;
            int axis = 0;
            double tx = tn[0];
            if (tn[1] < tx) { axis = 1; tx = tn[1]; }
            if (tn[2] < tx) { axis = 2; tx = tn[2]; }
            ++visited;
            long long place;
            if (ray_crosses(m, k, end_key, o, D, ta, fmin(tx, t1), rule.gate2, place)) {
                atomicAdd(reinterpret_cast<u64 *>(&crossed[place]), 1ULL);
                ++hits;
            }
            if (!(tx < t1)) { ended = true; break; }
            for (int a = 0; a < 3; ++a)
                if (a == axis) k[a] += d[a] > 0.0 ? 1.0 : -1.0;
            ta = tx;
        }
        cnt.n[NSC_MAP_RAY_STAT_VISITED] += visited;
        cnt.n[NSC_MAP_RAY_STAT_CROSSINGS] += hits;
        cnt.n[NSC_MAP_RAY_STAT_TRUNCATED] += !ended;
    });
    cnt.add_from(stats);
}

struct FlagRule {
    long long min_crossings;
    double ratio;
};

enum { F_FLAGGED = NSC_MAP_FLAG_STAT_FLAGGED, F_KEPT = NSC_MAP_FLAG_STAT_KEPT, F_DROPPED = NSC_MAP_FLAG_STAT_DROPPED,
       F_MISSING = NSC_MAP_FLAG_STAT_MISSING };

template <class T>
__global__ __launch_bounds__(MAP_THREADS) void ray_flag_kernel(InsertRows<T> in, const u64 *index, const long long *info,
                                                               const long long *crossed, long long max_voxels, FlagRule rule,
                                                               unsigned char *flags, long long *stats)
{
    LaneCounters<NSC_MAP_FLAG_STATS> cnt;
    for_each_row(in.total, [&](long long row, CloudSpan &span) {
        double w[3], u[3];
        u64 key;
        int kind = F_DROPPED;
        if (locate_row(in, row, span, w, u, key) == C_USED) {
            const long long h = find_slot(index, 2 * max_voxels, key);
            const u64 at = h < 0 ? ~0ULL : index[2 * h + 1];
            if (at >= (u64)max_voxels) {
                kind = F_MISSING;
            } else {
                const long long count = info[4 * at], c = crossed[at];
                const bool seen = count > 0 && c >= rule.min_crossings && (double)c >= rule.ratio * (double)count;
                kind = seen ? F_FLAGGED : F_KEPT;
            }
        }
        flags[row] = kind == F_FLAGGED;
        cnt.count(kind);
    });
    cnt.add_from(stats);
}

bool ray_ok(const NscMapRayParams *r)
{
    return r && isfinite(r->min_range) && isfinite(r->max_range) && isfinite(r->end_margin) && isfinite(r->gate) &&
           r->min_range >= 0.0 && r->max_range > 0.0 && r->gate > 0.0;
}

}  // namespace

extern "C" {

void nsc_map_ray_default_params(NscMapRayParams *p)
{
    if (!p) return;
    p->min_range = 0.0;
    p->max_range = 60.0;
    p->end_margin = -1.0;
    p->gate = 3.0;
}

int nsc_map_cast_rays(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_clouds,
                      int64_t total_rows, const double *poses, int32_t n_poses, const int64_t *pose_ids,
                      const NscMapParams *params, const double *voxels, const uint64_t *index, int64_t max_voxels,
                      const NscMapRayParams *ray, int64_t *crossed, int64_t *ray_stats, void *stream)
{
    const MapArgs a{points, dtype, stride_floats, offsets, n_clouds, total_rows, poses, n_poses, pose_ids, params, max_voxels,
                    ray_stats};
    if (const int st = a.check(voxels && index && crossed)) return st;
    if (!ray_ok(ray)) return NSC_EINVAL;
    const double reach = ray->max_range / params->voxel_size;
    if (!(reach <= (double)NSC_MAP_RAY_MAX_REACH)) return NSC_EUNSUPPORTED;
    const RayRule rule{ray->min_range, ray->max_range, ray->end_margin < 0.0 ? params->voxel_size : ray->end_margin,
                       ray->gate * ray->gate, 3 * ((long long)floor(reach) + 2)};
    const RayMap m{voxels, reinterpret_cast<const u64 *>(index), (long long)max_voxels};
    hipStream_t s = static_cast<hipStream_t>(stream);
    long long *st = reinterpret_cast<long long *>(ray_stats);
    nsc_fill_u32(s, st, 0u, 2 * NSC_MAP_RAY_STATS);
    a.with_rows([&](auto in) {
        hipLaunchKernelGGL(ray_cast_kernel<typename decltype(in)::scalar>,
                           dim3(blocks_for(in.total, INSERT_ROWS, NSC_MAP_INSERT_BLOCKS)), dim3(MAP_THREADS), 0, s, in, m, rule,
                           reinterpret_cast<long long *>(crossed), st);
    });
    return launch_status();
}

int nsc_map_flag_rows(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_clouds,
                      int64_t total_rows, const double *poses, int32_t n_poses, const int64_t *pose_ids,
                      const NscMapParams *params, const uint64_t *index, const int64_t *info, const int64_t *crossed,
                      int64_t max_voxels, int64_t min_crossings, double ratio, uint8_t *row_flags, int64_t *flag_stats,
                      void *stream)
{
    const MapArgs a{points, dtype, stride_floats, offsets, n_clouds, total_rows, poses, n_poses, pose_ids, params, max_voxels,
                    flag_stats};
    if (const int st = a.check(index && info && crossed)) return st;
    if ((total_rows > 0 && !row_flags) || min_crossings < 1 || !isfinite(ratio) || !(ratio > 0.0)) return NSC_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    long long *st = reinterpret_cast<long long *>(flag_stats);
    nsc_fill_u32(s, st, 0u, 2 * NSC_MAP_FLAG_STATS);
    a.with_rows([&](auto in) {
        hipLaunchKernelGGL(ray_flag_kernel<typename decltype(in)::scalar>,
                           dim3(blocks_for(in.total, INSERT_ROWS, NSC_MAP_INSERT_BLOCKS)), dim3(MAP_THREADS), 0, s, in,
                           reinterpret_cast<const u64 *>(index), reinterpret_cast<const long long *>(info),
                           reinterpret_cast<const long long *>(crossed), (long long)max_voxels,
                           FlagRule{(long long)min_crossings, ratio}, row_flags, st);
    });
    return launch_status();
}

}  // extern "C"
