// nsc_retrieval_q.hip -- stage-1 Wasserstein retrieval over QUANTISED descriptors on gfx950.
//
// A descriptor travels as a uint16 histogram whose bins sum to 65535 (nsc_quantize_descriptors, a "canonical" row).
// Its integer CDF fits uint16 entry by entry, and
//     d_int(a, b) = sum_k |cdf_a[k] - cdf_b[k]|          (uint32, < 2^26 for D <= 1024)
// divided by 65535 is W1 between the dequantised histograms.  Everything below accumulates in integers, so a
// distance does not depend on the kernel, the tiling or the batch it was computed in.  v_sad_u16 takes two packed
// |a - b| and the accumulate in one VALU instruction: a uint32 of a CDF row already holds bins k and k + 1.
//
//   w1q_cdf_kernel       one wave per row: uint32 total and prefix, uint16 CDF and the canonical flag
//   w1q_stream_kernel<QT> Q <= 4: query CDFs in registers as packed pairs, every wave walks its rows with 16-byte
//                        non-temporal loads, the next two rows in flight (1 600 B per row at D = 800, read once)
//   w1q_tile_kernel<NQ>  Q > 4: 64 rows x 16 NQ queries per workgroup, k-pairs staged k-major through LDS, 4 x NQ
//                        results per thread, one v_sad_u16 per row, query and k-pair
//   w1q_generic_kernel   any D in [1, 1024] and any alignment: one wave per row, scalar uint16 loads
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nsc.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float qf32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t wave_sumu(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// acc + |a.lo - b.lo| + |a.hi - b.hi| on the two uint16 halves: v_sad_u16
__device__ __forceinline__ uint32_t sad2(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_sad_u16(a, b, acc); }

// d_int -> distance; +inf for a non-canonical side (ok = both flags) or a pair the spatial filter excludes (the
// expression of w1_stream_kernel, nsc_retrieval.hip).  The division is IEEE: no reciprocal.
__device__ __forceinline__ float q_result(uint32_t s, bool ok, int i, int q, const float *__restrict__ db_pos,
                                          const float *__restrict__ q_pos, float min_dist)
{
    float r = ok ? (float)s / 65535.0f : INFINITY;
    if (db_pos && q_pos) {                                      // two_stage_retrieval.py:160-170
        const float dx = db_pos[i * 3] - q_pos[q * 3], dy = db_pos[i * 3 + 1] - q_pos[q * 3 + 1],
                    dz = db_pos[i * 3 + 2] - q_pos[q * 3 + 2];
        if (sqrtf(dx * dx + dy * dy + dz * dz) < min_dist) r = INFINITY;
    }
    return r;
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
                a = sad2(r[j].x, qv[t][j].x, a);
                a = sad2(r[j].y, qv[t][j].y, a);
                a = sad2(r[j].z, qv[t][j].z, a);
                a = sad2(r[j].w, qv[t][j].w, a);
            }
            s[t] = wave_sumu(a);
        }
        if (lane == 0) {
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                if (t >= Q) break;
                dist[(long long)t * N + i] = q_result(s[t], ok != 0 && qok[t], i, t, db_pos, q_pos, min_dist);
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

constexpr int QTL_I = 64, QTL_KP = 32, QTL_LD = 68;           // rows per tile, k-pairs per chunk, padded LDS row

template <int NQ>   // queries per thread: the tile is 64 rows x 16 NQ queries
__global__ __launch_bounds__(256) void w1q_tile_kernel(const uint16_t *__restrict__ dbc,
                                                       const uint8_t *__restrict__ db_ok, int N, int D,
                                                       const uint16_t *__restrict__ qc,
                                                       const uint8_t *__restrict__ q_ok, int Q,
                                                       const float *__restrict__ db_pos,
                                                       const float *__restrict__ q_pos, float min_dist,
                                                       float *__restrict__ dist)
{
    __shared__ __attribute__((aligned(16))) uint32_t As[2][QTL_KP * QTL_LD];   // [k-pair][row]
    __shared__ __attribute__((aligned(16))) uint32_t Bs[2][QTL_KP * QTL_LD];   // [k-pair][query]
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    constexpr int TL_Q = 16 * NQ;
    constexpr int HB = (TL_Q + 31) / 32;                        // staging passes for the query tile
    const int i0 = blockIdx.x * QTL_I, q0 = blockIdx.y * TL_Q;
    // staging: thread -> (tile row sr / sr + 32, k-pair offset sk): 16 bytes = 4 pairs per thread, 128 per 8 threads
    const int sr = tid >> 3, sk = (tid & 7) * 4;
    const int npairs = D >> 1;                                  // D % 8 == 0 (checked by the host)
    const uint32_t *ga[2], *gb[HB];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ri = i0 + sr + 32 * h;
        ga[h] = reinterpret_cast<const uint32_t *>(dbc + (long long)(ri < N ? ri : N - 1) * D) + sk;
    }
#pragma unroll
    for (int h = 0; h < HB; ++h) {
        const int rq = q0 + sr + 32 * h;
        gb[h] = reinterpret_cast<const uint32_t *>(qc + (long long)(rq < Q ? rq : Q - 1) * D) + sk;
    }
    const int nchunks = (npairs + QTL_KP - 1) / QTL_KP;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    auto gload = [&](int ch, u32x4 (&ra)[2], u32x4 (&rb)[HB]) {
        const int k = ch * QTL_KP + sk;                          // past D: zeros on both sides add |0 - 0|
#pragma unroll
        for (int h = 0; h < 2; ++h)
            ra[h] = (k + 4 <= npairs) ? *reinterpret_cast<const u32x4 *>(ga[h] + ch * QTL_KP) : zero;
#pragma unroll
        for (int h = 0; h < HB; ++h)
            rb[h] = (k + 4 <= npairs && sr + 32 * h < TL_Q) ? *reinterpret_cast<const u32x4 *>(gb[h] + ch * QTL_KP) : zero;
    };
    auto stage = [&](int buf, const u32x4 (&ra)[2], const u32x4 (&rb)[HB]) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int j = 0; j < 4; ++j) As[buf][(sk + j) * QTL_LD + sr + 32 * h] = ra[h][j];
#pragma unroll
        for (int h = 0; h < HB; ++h)
            if (sr + 32 * h < TL_Q)
#pragma unroll
                for (int j = 0; j < 4; ++j) Bs[buf][(sk + j) * QTL_LD + sr + 32 * h] = rb[h][j];
    };
    uint32_t acc[4][NQ];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < NQ; ++b) acc[a][b] = 0u;

    u32x4 ra[2], rb[HB];
    gload(0, ra, rb);
    stage(0, ra, rb);
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        const int cur = ch & 1;
        if (ch + 1 < nchunks) gload(ch + 1, ra, rb);
        const uint32_t *as = As[cur], *bs = Bs[cur];
#pragma unroll 8
        for (int k = 0; k < QTL_KP; ++k) {
            const u32x4 av = *reinterpret_cast<const u32x4 *>(&as[k * QTL_LD + 4 * tx]);
            uint32_t bv[NQ];
#pragma unroll
            for (int b = 0; b < NQ; ++b) bv[b] = bs[k * QTL_LD + NQ * ty + b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < NQ; ++b) acc[a][b] = sad2(av[a], bv[b], acc[a][b]);
        }
        if (ch + 1 < nchunks) stage(cur ^ 1, ra, rb);
        __syncthreads();
    }
#pragma unroll
    for (int b = 0; b < NQ; ++b) {
        const int q = q0 + NQ * ty + b;
        if (q >= Q) continue;
        float r[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int i = i0 + 4 * tx + a;
            r[a] = (i < N) ? q_result(acc[a][b], db_ok[i] && q_ok[q], i, q, db_pos, q_pos, min_dist) : 0.0f;
        }
        float *o = dist + (long long)q * N + i0 + 4 * tx;
        if (i0 + 4 * tx + 3 < N && ((reinterpret_cast<uintptr_t>(o) & 15u) == 0)) {
            *reinterpret_cast<qf32x4 *>(o) = qf32x4{r[0], r[1], r[2], r[3]};
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (i0 + 4 * tx + a < N) o[a] = r[a];
        }
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
        if (lane == 0) dist[(long long)q * N + i] = q_result(s, db_ok[i] && q_ok[q], (int)i, q, db_pos, q_pos, min_dist);
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
    return hipGetLastError() == hipSuccess ? NSC_OK : NSC_ELAUNCH;
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
    } else if (Q <= 4) {
        int qwgs = (N + 3) / 4;
        if (qwgs > 256 * 8) qwgs = 256 * 8;                    // 8 resident workgroups per CU walk the rows
        const dim3 grid(qwgs);
        if (Q == 1) hipLaunchKernelGGL(w1q_stream_kernel<1>, grid, block, 0, st, W1Q_ARGS);
        else if (Q == 2) hipLaunchKernelGGL(w1q_stream_kernel<2>, grid, block, 0, st, W1Q_ARGS);
        else hipLaunchKernelGGL(w1q_stream_kernel<4>, grid, block, 0, st, W1Q_ARGS);
    } else {
        // tile of 64 rows x 16 / 32 / 64 queries: the smallest one that covers Q in as few column tiles as 64 does
        const int qnq = Q <= 16 ? 1 : (Q <= 32 || (Q > 64 && Q <= 96) ? 2 : 4);
        const dim3 grid((N + QTL_I - 1) / QTL_I, (Q + 16 * qnq - 1) / (16 * qnq));
        if (grid.y > 65535u) return NSC_EUNSUPPORTED;           // Q > 1 M: callers chunk the queries
        if (qnq == 1) hipLaunchKernelGGL(w1q_tile_kernel<1>, grid, block, 0, st, W1Q_ARGS);
        else if (qnq == 2) hipLaunchKernelGGL(w1q_tile_kernel<2>, grid, block, 0, st, W1Q_ARGS);
        else hipLaunchKernelGGL(w1q_tile_kernel<4>, grid, block, 0, st, W1Q_ARGS);
    }
#undef W1Q_ARGS
    return hipGetLastError() == hipSuccess ? NSC_OK : NSC_ELAUNCH;
}

}  // extern "C"
