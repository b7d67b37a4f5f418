// nsc_retrieval_q.hip -- stage-1 Wasserstein retrieval over QUANTISED descriptors on gfx950.
//
// A descriptor travels as a uint16 histogram whose bins sum to 65535 (nsc_quantize_descriptors, a "canonical" row).
// Its integer CDF fits uint16 entry by entry, and
//     d_int(a, b) = sum_k |cdf_a[k] - cdf_b[k]|          (uint32, < 2^26 for D <= 1024)
// divided by 65535 is W1 between the dequantised histograms.  Everything below accumulates in integers, so a
// distance does not depend on the kernel, the tiling or the batch it was computed in.  v_sad_u16 takes two packed
// |a - b| and the accumulate in one VALU instruction: a uint32 of a CDF row already holds bins k and k + 1.
// nsc_w1_rows.h holds what this file shares with the float32 kernels of nsc_retrieval.hip: the spatial filter, the
// 16-bit row form U16Rows (the sum's step, d_int -> distance) and the tile kernel.
//
//   w1q_cdf_kernel       one wave per row: uint32 total and prefix, uint16 CDF and the canonical flag
//   w1q_stream_kernel<QT> Q <= 4: query CDFs in registers as packed pairs, every wave walks its rows with 16-byte
//                        non-temporal loads, the next two rows in flight (1 600 B per row at D = 800, read once)
//   w1_tile_kernel<U16Rows, NQ>  Q > 4: 64 rows x 16 NQ queries per workgroup, k-pairs staged k-major through LDS,
//                        4 x NQ results per thread, one v_sad_u16 per row, query and k-pair
//   w1q_generic_kernel   any D in [1, 1024] and any alignment: one wave per row, scalar uint16 loads
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nsc.h"
#include "nsc_w1_rows.h"
#include "nsc_util.h"

namespace {

__device__ __forceinline__ uint32_t wave_sumu(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

__global__ __launch_bounds__(256) void w1q_cdf_kernel(const uint16_t *__restrict__ h, int n, int D,
                                                      uint16_t *__restrict__ cdf, uint8_t *__restrict__ canonical)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    constexpr int PER = 16;                                     // consecutive bins per lane: D <= 1024
    const uint16_t *row = h + (long long)i * D;
    uint32_t v[PER], run = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = lane * PER + k;
        run += (c < D) ? (uint32_t)row[c] : 0u;
        v[k] = run;
    }
    const uint32_t total = wave_sumu(run);                      // <= 1024 * 65535: the 131 071 row is seen as such
    uint32_t inc = run;                                         // exclusive scan of the lane totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)inc, o);
        if (lane >= o) inc += t;
    }
    const uint32_t off = inc - run;
    const bool ok = total == 65535u;
    uint16_t *out = cdf + (long long)i * D;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = lane * PER + k;
        if (c < D) out[c] = ok ? (uint16_t)(v[k] + off) : (uint16_t)0;
    }
    if (lane == 0) canonical[i] = ok ? 1 : 0;
}

template <int QT>
__global__ __launch_bounds__(256) void w1q_stream_kernel(const uint16_t *__restrict__ dbc,
                                                         const uint8_t *__restrict__ db_ok, int N, int D,
                                                         const uint16_t *__restrict__ qc,
                                                         const uint8_t *__restrict__ q_ok, int Q,
                                                         const float *__restrict__ db_pos,
                                                         const float *__restrict__ q_pos, float min_dist,
                                                         float *__restrict__ dist)
{
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    const int nvec = D >> 3;                                    // D % 8 == 0 (checked by the host): 16-byte chunks
    constexpr int NV = 2;                                       // chunks per lane: D <= 1024
    const u32x4 zero = {0u, 0u, 0u, 0u};
    u32x4 qv[QT][NV];
    bool qok[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        qok[t] = t < Q && q_ok[t] != 0;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = lane + 64 * j;
            qv[t][j] = (t < Q && c < nvec) ? reinterpret_cast<const u32x4 *>(qc + (long long)t * D)[c] : zero;
        }
    }
    // A row's loads (its chunks and its flag) are issued without a branch around them -- a lane past the row's end reads
    // chunk 0 again and a wave past the database's end its current row again -- so that the compiler can wait for one
    // row by count and leave the loads of the next two in flight.
    auto load = [&](long long i, u32x4 (&v)[NV], uint32_t &ok) {
        const u32x4 *row = reinterpret_cast<const u32x4 *>(dbc + i * D);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = lane + 64 * j;
            v[j] = __builtin_nontemporal_load(&row[c < nvec ? c : 0]);
        }
        ok = db_ok[i];
    };
    auto score = [&](int i, const u32x4 (&v)[NV], uint32_t ok) {
        u32x4 r[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) r[j] = (lane + 64 * j < nvec) ? v[j] : zero;
        uint32_t s[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            uint32_t a = 0;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                a = U16Rows::add(r[j].x, qv[t][j].x, a);
                a = U16Rows::add(r[j].y, qv[t][j].y, a);
                a = U16Rows::add(r[j].z, qv[t][j].z, a);
                a = U16Rows::add(r[j].w, qv[t][j].w, a);
            }
            s[t] = wave_sumu(a);
        }
        if (lane == 0) {
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                if (t >= Q) break;
                dist[(long long)t * N + i] = w1_filter(U16Rows::scaled(s[t], ok != 0 && qok[t]), db_pos, i, q_pos, t, min_dist);
            }
        }
    };
    // three row buffers in rotation, spelled out so that no buffer is copied while its load is in flight
    u32x4 b0[NV], b1[NV], b2[NV];
    uint32_t f0, f1, f2;
    const long long step = nwaves;
    long long i = wave;                                         // i + 2 step can pass 2^31 near the largest N
    if (i >= N) return;
    auto ahead = [&](long long k) { return i + k * step < N ? i + k * step : i; };
    load(i, b0, f0);
    load(ahead(1), b1, f1);
    for (;;) {
        load(ahead(2), b2, f2);
        score((int)i, b0, f0);
        i += step;
        if (i >= N) break;
        load(ahead(2), b0, f0);
        score((int)i, b1, f1);
        i += step;
        if (i >= N) break;
        load(ahead(2), b1, f1);
        score((int)i, b2, f2);
        i += step;
        if (i >= N) break;
    }
}

// every other D and any alignment: one wave per row, the queries one after the other
__global__ __launch_bounds__(256) void w1q_generic_kernel(const uint16_t *__restrict__ dbc,
                                                          const uint8_t *__restrict__ db_ok, int N, int D,
                                                          const uint16_t *__restrict__ qc,
                                                          const uint8_t *__restrict__ q_ok, int Q,
                                                          const float *__restrict__ db_pos,
                                                          const float *__restrict__ q_pos, float min_dist,
                                                          float *__restrict__ dist)
{
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    constexpr int PER = 16;                                     // bins lane, lane + 64, ...: D <= 1024
    const uint16_t *row = dbc + i * D;
    uint32_t v[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = lane + 64 * k;
        v[k] = (c < D) ? (uint32_t)row[c] : 0u;
    }
    for (int q = 0; q < Q; ++q) {
        const uint16_t *qr = qc + (long long)q * D;
        uint32_t s = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int c = lane + 64 * k;
            const uint32_t w = (c < D) ? (uint32_t)qr[c] : 0u;
            s += v[k] > w ? v[k] - w : w - v[k];
        }
        s = wave_sumu(s);
        if (lane == 0)
            dist[(long long)q * N + i] = w1_filter(U16Rows::scaled(s, db_ok[i] && q_ok[q]), db_pos, (int)i, q_pos, q, min_dist);
    }
}

}  // namespace

extern "C" {

int nsc_w1q_cdf(const uint16_t *quantized, int32_t n, int32_t D, uint16_t *cdf, uint8_t *canonical, void *stream_)
{
    if (n < 0 || D < 1 || D > 1024) return NSC_EUNSUPPORTED;
    if (n == 0) return NSC_OK;
    if (!quantized || !cdf || !canonical) return NSC_EINVAL;
    hipLaunchKernelGGL(w1q_cdf_kernel, dim3((n + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream_), quantized, n, D,
                       cdf, canonical);
    return launch_status();
}

int nsc_w1q_distances(const uint16_t *db_cdf, const uint8_t *db_canonical, int32_t N, int32_t D,
                      const uint16_t *q_cdf, const uint8_t *q_canonical, int32_t Q,
                      const float *db_pos, const float *q_pos, float min_dist, float *dist, void *stream_)
{
    if (N < 0 || Q < 0 || D < 1 || D > 1024) return NSC_EUNSUPPORTED;
    if (N == 0 || Q == 0) return NSC_OK;
    if (!db_cdf || !db_canonical || !q_cdf || !q_canonical || !dist) return NSC_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream_);
    const bool packed = D % 8 == 0 && !((reinterpret_cast<uintptr_t>(db_cdf) | reinterpret_cast<uintptr_t>(q_cdf)) & 15u);
    const dim3 block(256);
#define W1Q_ARGS db_cdf, db_canonical, N, D, q_cdf, q_canonical, Q, db_pos, q_pos, min_dist, dist
    if (!packed) {
        hipLaunchKernelGGL(w1q_generic_kernel, dim3((N + 3) / 4), block, 0, st, W1Q_ARGS);
    } else if (Q <= W1_STREAM_MAX_Q) {
        const dim3 grid(w1_stream_workgroups(N));
        if (Q == 1) hipLaunchKernelGGL(w1q_stream_kernel<1>, grid, block, 0, st, W1Q_ARGS);
        else if (Q == 2) hipLaunchKernelGGL(w1q_stream_kernel<2>, grid, block, 0, st, W1Q_ARGS);
        else hipLaunchKernelGGL(w1q_stream_kernel<4>, grid, block, 0, st, W1Q_ARGS);
    } else {
        return launch_w1_tile(st, U16Rows{db_cdf, db_canonical, q_cdf, q_canonical}, N, D, Q, db_pos, q_pos, min_dist, dist);
    }
#undef W1Q_ARGS
    return launch_status();
}

}  // extern "C"
