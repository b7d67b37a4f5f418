// nsc_w1_rows.h -- what the W1 distance kernels over float32 CDF rows (nsc_retrieval.hip) and over uint16 CDF rows
// (nsc_retrieval_q.hip) share: the spatial filter, the two row forms, the tile kernel for query batches
// and the dispatch rules of the stream and tile kernels.  The stream kernels stay in their own files: their load
// pipelines differ by design.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nsc.h"
#include "nsc_util.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- spatial filter (two_stage_retrieval.py:160-170): a database frame strictly closer than min_dist to the query is
// skipped.  float32 throughout, the squares summed left to right.
__device__ __forceinline__ bool w1_too_close(const float *p, const float *qp, float min_dist)
{
    const float dx = p[0] - qp[0], dy = p[1] - qp[1], dz = p[2] - qp[2];
    return sqrtf(dx * dx + dy * dy + dz * dz) < min_dist;
}

// r, or +inf where both position arrays are given and the filter excludes (row i, query q)
__device__ __forceinline__ float w1_filter(float r, const float *db_pos, int i, const float *q_pos, int q, float min_dist)
{
    if (db_pos && q_pos && w1_too_close(db_pos + i * 3, q_pos + q * 3, min_dist)) r = INFINITY;
    return r;
}

// ---- row forms: how a CDF row is held in 32-bit words, how |a - b| accumulates, how a sum becomes the distance
struct F32Rows {                                               // one float bin per word
    typedef float word;
    typedef f32x4 vec;
    typedef float sum;
    const float *db, *q;
    static __device__ __forceinline__ int words(int D) { return D; }
    __device__ __forceinline__ const word *db_row(int i, int D) const { return db + (long long)i * D; }
    __device__ __forceinline__ const word *q_row(int t, int D) const { return q + (long long)t * D; }
    static __device__ __forceinline__ sum add(word a, word b, sum s) { return s + fabsf(a - b); }
    __device__ __forceinline__ float result(sum s, int, int) const { return s; }
};

struct U16Rows {                                               // bins k and k + 1 per word; D % 2 == 0
    typedef uint32_t word;
    typedef u32x4 vec;
    typedef uint32_t sum;
    const uint16_t *db;
    const uint8_t *db_ok;                                      // canonical flags: a row without one has no distance
    const uint16_t *q;
    const uint8_t *q_ok;
    static __device__ __forceinline__ int words(int D) { return D >> 1; }
    __device__ __forceinline__ const word *db_row(int i, int D) const { return reinterpret_cast<const word *>(db + (long long)i * D); }
    __device__ __forceinline__ const word *q_row(int t, int D) const { return reinterpret_cast<const word *>(q + (long long)t * D); }
    // s + |a.lo - b.lo| + |a.hi - b.hi| on the two uint16 halves: v_sad_u16
    static __device__ __forceinline__ sum add(word a, word b, sum s) { return __builtin_amdgcn_sad_u16(a, b, s); }
    // d_int -> distance, +inf unless both rows are canonical.  The division is IEEE: no reciprocal.
    static __device__ __forceinline__ float scaled(sum s, bool ok) { return ok ? (float)s / 65535.0f : INFINITY; }
    __device__ __forceinline__ float result(sum s, int i, int t) const { return scaled(s, db_ok[i] && q_ok[t]); }
};

// ---- w1_tile_kernel: query batches.  VALU-bound (2 ops per float |a - b| element, one v_sad_u16 per uint16 pair): a
// 64-row x 16 NQ-query tile per workgroup, 4 x NQ results per thread, k in chunks of 32 words staged k-major through
// LDS -- the structure of a register-tiled SGEMM with |a - b| in place of a * b.  Each (row, query) sum is accumulated
// by ONE thread in ascending k, so it does not depend on the tiling.
constexpr int TL_I = 64, TL_K = 32, TL_LD = 68;               // rows per tile, words per chunk, padded LDS row

template <class Rows, int NQ>   // queries per thread: the tile is 64 rows x 16 NQ queries
__global__ __launch_bounds__(256) void w1_tile_kernel(Rows rows, int N, int D, int Q,
                                                      const float *__restrict__ db_pos,
                                                      const float *__restrict__ q_pos, float min_dist,
                                                      float *__restrict__ dist)
{
    typedef typename Rows::word word;
    typedef typename Rows::vec vec;
    __shared__ __attribute__((aligned(16))) word As[2][TL_K * TL_LD];   // [k][row]
    __shared__ __attribute__((aligned(16))) word Bs[2][TL_K * TL_LD];   // [k][query]
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    constexpr int TL_Q = 16 * NQ;
    constexpr int HB = (TL_Q + 31) / 32;                            // staging passes for the query tile
    const int i0 = blockIdx.x * TL_I, q0 = blockIdx.y * TL_Q;
    // staging: thread -> (tile row sr / sr + 32, word offset sk): 16 bytes per thread, 128 contiguous per 8 threads
    const int sr = tid >> 3, sk = (tid & 7) * 4;
    const int nwords = Rows::words(D);                              // a multiple of 4 (checked by the host)
    const word *ga[2], *gb[HB];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ri = i0 + sr + 32 * h;
        ga[h] = rows.db_row(ri < N ? ri : N - 1, D) + sk;
    }
#pragma unroll
    for (int h = 0; h < HB; ++h) {
        const int rq = q0 + sr + 32 * h;
        gb[h] = rows.q_row(rq < Q ? rq : Q - 1, D) + sk;
    }
    const int nchunks = (nwords + TL_K - 1) / TL_K;
    const vec zero = {};
    auto gload = [&](int ch, vec (&ra)[2], vec (&rb)[HB]) {
        const int k = ch * TL_K + sk;                                // past the row: zeros on both sides add |0 - 0|
#pragma unroll
        for (int h = 0; h < 2; ++h)
            ra[h] = (k + 4 <= nwords) ? *reinterpret_cast<const vec *>(ga[h] + ch * TL_K) : zero;
#pragma unroll
        for (int h = 0; h < HB; ++h)
            rb[h] = (k + 4 <= nwords && sr + 32 * h < TL_Q) ? *reinterpret_cast<const vec *>(gb[h] + ch * TL_K) : zero;
    };
    auto stage = [&](int buf, const vec (&ra)[2], const vec (&rb)[HB]) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int j = 0; j < 4; ++j) As[buf][(sk + j) * TL_LD + sr + 32 * h] = ra[h][j];
#pragma unroll
        for (int h = 0; h < HB; ++h)
            if (sr + 32 * h < TL_Q)
#pragma unroll
                for (int j = 0; j < 4; ++j) Bs[buf][(sk + j) * TL_LD + sr + 32 * h] = rb[h][j];
    };
    typename Rows::sum acc[4][NQ];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < NQ; ++b) acc[a][b] = 0;

    vec ra[2], rb[HB];
    gload(0, ra, rb);
    stage(0, ra, rb);
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        const int cur = ch & 1;
        if (ch + 1 < nchunks) gload(ch + 1, ra, rb);
        const word *as = As[cur], *bs = Bs[cur];
#pragma unroll 8
        for (int k = 0; k < TL_K; ++k) {
            const vec av = *reinterpret_cast<const vec *>(&as[k * TL_LD + 4 * tx]);
            word bv[NQ];
#pragma unroll
            for (int b = 0; b < NQ; ++b) bv[b] = bs[k * TL_LD + NQ * ty + b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < NQ; ++b) acc[a][b] = Rows::add(av[a], bv[b], acc[a][b]);
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
            const int i = i0 + 4 * tx + a;                           // past N: row N - 1 again, as in staging; never stored
            r[a] = rows.result(acc[a][b], i < N ? i : N - 1, q);
            if (db_pos && q_pos && i < N && w1_too_close(db_pos + i * 3, q_pos + q * 3, min_dist)) r[a] = INFINITY;
        }
        float *o = dist + (long long)q * N + i0 + 4 * tx;
        if (i0 + 4 * tx + 3 < N && ((reinterpret_cast<uintptr_t>(o) & 15u) == 0)) {
            *reinterpret_cast<f32x4 *>(o) = f32x4{r[0], r[1], r[2], r[3]};
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (i0 + 4 * tx + a < N) o[a] = r[a];
        }
    }
}

// ---- dispatch.  Up to W1_STREAM_MAX_Q queries go to a stream kernel (HBM-bound, the queries in registers), larger
// batches to the tile kernel.
constexpr int W1_STREAM_MAX_Q = 4;
constexpr int W1_STREAM_WG_CAP = 256 * 8;                     // 8 resident workgroups per CU walk the rows

// workgroups of a stream kernel: one wave per row up to the cap
inline int w1_stream_workgroups(int N) { const int wgs = (N + 3) / 4; return wgs < W1_STREAM_WG_CAP ? wgs : W1_STREAM_WG_CAP; }

// tile of 64 rows x 16 / 32 / 64 queries: the smallest one that covers Q in as few column tiles as 64 does
inline int w1_tile_nq(int Q) { return Q <= 16 ? 1 : (Q <= 32 || (Q > 64 && Q <= 96) ? 2 : 4); }

template <class Rows>
int launch_w1_tile(hipStream_t st, Rows rows, int N, int D, int Q, const float *db_pos, const float *q_pos,
                   float min_dist, float *dist)
{
    const int nq = w1_tile_nq(Q);
    const dim3 grid((N + TL_I - 1) / TL_I, (Q + 16 * nq - 1) / (16 * nq)), block(256);
    if (grid.y > 65535u) return NSC_EUNSUPPORTED;               // Q > 1 M: callers chunk the queries
    if (nq == 1) hipLaunchKernelGGL((w1_tile_kernel<Rows, 1>), grid, block, 0, st, rows, N, D, Q, db_pos, q_pos, min_dist, dist);
    else if (nq == 2) hipLaunchKernelGGL((w1_tile_kernel<Rows, 2>), grid, block, 0, st, rows, N, D, Q, db_pos, q_pos, min_dist, dist);
    else hipLaunchKernelGGL((w1_tile_kernel<Rows, 4>), grid, block, 0, st, rows, N, D, Q, db_pos, q_pos, min_dist, dist);
    return launch_status();
}

}  // namespace
