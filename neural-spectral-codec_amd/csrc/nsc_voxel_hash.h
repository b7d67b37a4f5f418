// nsc_voxel_hash.h -- what the voxel tables of nsc_geometry.hip (one table per cloud) and nsc_map.hip (one table for
// all clouds) share: the packed 64-bit voxel key, its hash, the linear probe's step and the fixed point of the exact
// coordinate sums; and what nsc_map.hip and nsc_localize.hip share: the world grid, the placement of a row and the voxel
// of a world point.  Included at file scope; the namespace below gives each file its own copy.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int KEY_BITS = 21;            // voxel key per axis: 0 .. 2^21-1
constexpr long long KEY_MAX = (1LL << KEY_BITS) - 1;
constexpr double FIX_SCALE = 16777216.0;        // coordinate sums in int64 units of 2^-24 m

__device__ __forceinline__ unsigned long long mix64(unsigned long long x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return x;
}

__device__ __forceinline__ unsigned long long pack_key(long long x, long long y, long long z)
{
    return (unsigned long long)x | ((unsigned long long)y << KEY_BITS) | ((unsigned long long)z << (2 * KEY_BITS));
}

// the slot a linear probe visits after h, wrapping at the table's end
__device__ __forceinline__ long long next_slot(long long h, long long cap) { return h + 1 == cap ? 0 : h + 1; }

// ---- the world grid of nsc_map.hip and nsc_localize.hip: voxel (2^20, 2^20, 2^20) begins at `origin`
constexpr double KEY_OFFSET = 1048576.0;        // 2^20: voxel coordinates count from -2^20
constexpr double MOMENT_SCALE = 65536.0;        // positions inside a voxel in units of 2^-16 voxel
constexpr double MOMENT_HALF = 32768.0;

struct MapGrid {
    double voxel, origin[3];
};

// A placed row: R p + t, every operation rounded on its own.  P = rows 0..2 of a row-major 4x4
__device__ __forceinline__ void place_row(const double *P, const double p[3], double w[3])
{
    for (int a = 0; a < 3; ++a) w[a] = ((P[4 * a] * p[0] + P[4 * a + 1] * p[1]) + P[4 * a + 2] * p[2]) + P[4 * a + 3];
}

// The voxel of a finite world point: k = floor((w - origin) / voxel) per axis, u = the position inside the voxel in
// [0, 1) (exact), and the packed key of k + 2^20; false outside the 2^21 voxels per axis
__device__ __forceinline__ bool world_voxel(const double w[3], const MapGrid &g, double u[3], unsigned long long &key)
{
    double kd[3];
    for (int a = 0; a < 3; ++a) {
        const double f = (w[a] - g.origin[a]) / g.voxel, k = floor(f);
        u[a] = f - k;
        kd[a] = k + KEY_OFFSET;
    }
    if (!(kd[0] >= 0.0 && kd[0] <= (double)KEY_MAX && kd[1] >= 0.0 && kd[1] <= (double)KEY_MAX && kd[2] >= 0.0 &&
          kd[2] <= (double)KEY_MAX))
        return false;
    key = pack_key((long long)kd[0], (long long)kd[1], (long long)kd[2]);
    return true;
}

}  // namespace
