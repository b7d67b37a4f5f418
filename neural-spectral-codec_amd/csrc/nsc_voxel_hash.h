// nsc_voxel_hash.h -- what the voxel tables of nsc_geometry.hip (one table per cloud) and nsc_map.hip (one table for
// all clouds) share: the packed 64-bit voxel key, its hash, the linear probe's step and the fixed point of the exact
// coordinate sums.  Included at file scope; the namespace below gives each file its own copy.
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

}  // namespace
