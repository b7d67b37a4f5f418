// nsc_util.h -- the small jobs every .hip of the library does the same way: the status of an entry point's launches, the
// 64-lane butterfly sum and maximum, the opt-in for more than 64 KB of dynamic LDS, the workspace carver, and the scan and
// row sort of the two CSR builders (nsc_graph_build_csr, nsc_graph_transpose).  Included at file scope; the namespace below
// gives each file its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>

#include "../../include/nsc.h"

namespace {

// what an entry point returns after its last launch
inline int launch_status() { return hipGetLastError() == hipSuccess ? NSC_OK : NSC_ELAUNCH; }

// the sum over the 64 lanes of a wave, the same bits in every lane: xor butterfly, offsets 32 down to 1
template <class T> __device__ __forceinline__ T nsc_wave_sum(T v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the maximum over the 64 lanes of a wave, in every lane: the same butterfly
__device__ __forceinline__ float nsc_wave_max(float v)
{
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// the inclusive scan of an integer over the 64 lanes of a wave: lane l gets the sum of lanes 0 .. l
__device__ __forceinline__ int nsc_wave_scan(int v)
{
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// ---- more than 64 KB of dynamic LDS.  Above 64 KB a kernel has to be opted in, and the attribute is per DEVICE.  One atomic
// per (kernel instantiation, device): 0 not tried, 1 opted in, 2 refused; racing threads at worst both set the attribute
// (idempotent).  false: the device refuses, or its index is outside the table -- the caller falls back or reports.  The kernel is
// a template ARGUMENT, not a function argument: instantiations of one kernel template share their pointer type, and with it
// they would share the table.
template <auto KERNEL> bool nsc_opt_in_lds(unsigned bytes)
{
    if (bytes <= 64 * 1024) return true;
    static std::atomic<int> opted[16];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return false;
    int s = opted[dev].load(std::memory_order_acquire);
    if (s == 0) {
        s = hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) ==
                    hipSuccess ? 1 : 2;
        opted[dev].store(s, std::memory_order_release);
    }
    return s == 1;
}

// ---- workspaces.  A workspace is laid out by ONE function that maps (base or null, shape) to a struct of typed pointers
// plus `total`: the size query calls it with a null base, the entry points with the caller's pointer.
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

template <class T> struct Slots {                                   // `count` equal regions, `stride` elements apart
    T *p;
    size_t stride;
    T *operator()(int i) const { return p + stride * i; }
};

struct Carver {                                                      // consecutive regions from base (0: offsets only)
    uintptr_t base;
    size_t o;
    template <class T> T *take(size_t n) { T *p = reinterpret_cast<T *>(base + o); o += align256(n * sizeof(T)); return p; }
    template <class T> Slots<T> slots(size_t n, int count)
    {
        const size_t s = align256(n * sizeof(T)) / sizeof(T);
        return {take<T>(s * count), s};
    }
};

// ---- CSR builders

// exclusive scan of (cnt[i] + ADD) into ptr[0 .. N], ptr[N] the total: one workgroup of 1024 threads
template <int ADD>
__global__ __launch_bounds__(1024) void nsc_csr_scan_kernel(const int *__restrict__ cnt, int N, int *__restrict__ ptr)
{
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int chunk = (N + 1023) / 1024;
    const int b = tid * chunk, e = min(b + chunk, N);
    int s = 0;
    for (int i = b; i < e; ++i) s += cnt[i] + ADD;
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = (tid >= off) ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - s;
    for (int i = b; i < e; ++i) { ptr[i] = run; run += cnt[i] + ADD; }
    if (tid == 1023) ptr[N] = part[1023];
}

// a[b .. e) into ascending order by insertion (rows are short)
__device__ __forceinline__ void nsc_sort_row(int *__restrict__ a, int b, int e)
{
    for (int k = b + 1; k < e; ++k) {
        const int v = a[k];
        int c = k - 1;
        while (c >= b && a[c] > v) { a[c + 1] = a[c]; --c; }
        a[c + 1] = v;
    }
}

}  // namespace
