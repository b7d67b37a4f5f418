// nsc_planar.hip -- planar initial guess (yaw, x, y) for stage 2 of loop closing: a joint vote over yaw hypotheses and
// planar translation bins, cast by the structure rows of two prepared clouds (NscGicpCloudSet).
//
// The definition the kernels and tests/planar_restatement.py share is stated in include/nsc.h (nsc_planar_align) and
// retrieval/planar_alignment.py; DESIGN.md section 4.10 has the measurements.  In short, per hypothesis h with
// (c, s) = yaw_cs[h], source structure row a (row index divisible by source_stride) and target structure row b:
//   xr = c a.x - s a.y,  yr = s a.x + c a.y                      (every operation rounded on its own, float64:
//                                                                  contraction to fma is switched off below)
//   bx = floor((b.x - xr) inv_cell + 0.5),  by likewise
//   one vote for (h, bx, by) iff |bx| <= half_bins, |by| <= half_bins and |b.z - a.z| <= z_window
// The counts are integers, so no order of the rows, lanes or atomics changes a result.
//
// Three launches, no memset, no sync:
//   planar_setup_kernel   one workgroup per pair: ids -> row ranges (an id outside its store gives an empty pair and
//                         the invalid mark), and the two counts the caller gets back.
//   planar_vote_kernel    one workgroup of 256 lanes per (hypothesis, pair).  The (2 half_bins + 1)^2 int32 histogram
//                         lives in LDS.  Source rows are read 256 at a time; the rows taken are appended to an LDS
//                         list (an LDS counter hands out the places: the order is free) until fewer than 256 places
//                         of its 1024 are left; then lane l rotates the list's rows l, l + 256, l + 512, l + 768 once
//                         into registers and the target streams by: 256 rows at a time, the structure rows among
//                         them appended to an LDS tile that every lane then reads as a broadcast, one pair test per
//                         read for each of the ceil(list / 256) rows a lane can hold of this list (uniform; one
//                         unrolled variant per count).  Hits go to the histogram with LDS atomic adds.  When the
//                         source is used up, the largest count and its smallest flat bin are reduced over the
//                         workgroup and written as (peak_h, bin_h).
//   planar_reduce_kernel  one wave per pair: best hypothesis (ties to the smaller h), runner-up outside the guard
//                         (circular over H), and the pair's outputs.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nsc.h"
#include "nsc_util.h"

// The definition rounds every operation on its own.  hipcc's default contracts a * b + c into an fma, also through the
// _rn intrinsics (plain operators in a header, out of this pragma's reach), so the arithmetic below is written with
// plain operators under the pragma: exact equality with the restatement then holds whatever flags the file is built
// with (no v_fma_f64 in the code object with or without -ffp-contract=off).
#pragma clang fp contract(off)

namespace {

constexpr int VOTE_THREADS = 256;
constexpr int SRC_PER_LANE = 4;                          // source rows a lane holds in registers
constexpr int SRC_LIST = VOTE_THREADS * SRC_PER_LANE;    // places of the source list
constexpr int TILE = VOTE_THREADS;                       // target rows looked at per tile, one per lane
constexpr int MAX_SIDE = 2 * NSC_PLANAR_MAX_HALF_BINS + 1;
constexpr int MAX_BINS = MAX_SIDE * MAX_SIDE;            // 4225 int32: 16.9 KB
constexpr int SETUP_THREADS = 256;

struct Sets {                        // what the kernels read of the two NscGicpCloudSets
    const long long *s_off, *t_off;
    const double *s_pts, *s_cov, *t_pts, *t_cov;
    long long s_clouds, t_clouds;
    double s_thr, t_thr;             // normal_z2_max (1 - epsilon) of each set
};

struct PairRows {                    // pair p, resolved by planar_setup_kernel
    long long s_row, ms, t_row, mt;
    int valid, taken, structure, pad;
};

struct Vote {                        // the parameters of the vote
    double inv_cell, z_window, half;
    int half_bins, stride;
};

// a row is a structure row iff (1 - C_zz) < normal_z2_max (1 - epsilon); zz is the last of the six stored terms
__device__ __forceinline__ bool is_structure(const double *cov6, double thr) { return 1.0 - cov6[5] < thr; }

__global__ __launch_bounds__(SETUP_THREADS) void planar_setup_kernel(Sets st, const long long *source_ids,
                                                                     const long long *target_ids, int stride,
                                                                     PairRows *rows)
{
    __shared__ int part[2][SETUP_THREADS / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const long long a = source_ids[p], b = target_ids[p];
    if (a < 0 || a >= st.s_clouds || b < 0 || b >= st.t_clouds) {     // uniform; nothing of the stores is read
        if (tid == 0) rows[p] = PairRows{0, 0, 0, 0, 0, 0, 0, 0};
        return;
    }
    const long long s0 = st.s_off[a], ms = st.s_off[a + 1] - s0, t0 = st.t_off[b], mt = st.t_off[b + 1] - t0;
    int taken = 0, structure = 0;
    for (long long i = tid; i < ms; i += SETUP_THREADS)
        taken += (i % stride == 0) && is_structure(st.s_cov + 6 * (s0 + i), st.s_thr);
    for (long long i = tid; i < mt; i += SETUP_THREADS) structure += is_structure(st.t_cov + 6 * (t0 + i), st.t_thr);
    taken = nsc_wave_sum(taken);
    structure = nsc_wave_sum(structure);
    if ((tid & 63) == 0) {
        part[0][tid >> 6] = taken;
        part[1][tid >> 6] = structure;
    }
    __syncthreads();
    if (tid == 0) {
        taken = structure = 0;
        for (int w = 0; w < SETUP_THREADS / 64; ++w) {
            taken += part[0][w];
            structure += part[1][w];
        }
        rows[p] = PairRows{s0, ms, t0, mt, 1, taken, structure, 0};
    }
}

// The pair tests of one lane against the nt rows of a target tile, for the first N of the source rows it holds.
template <int N>
__device__ __forceinline__ void vote_tile(const double (*tile)[3], int nt, const double *xr, const double *yr,
                                          const double *zs, const Vote &v, int side, int *hist)
{
    for (int t = 0; t < nt; ++t) {
        const double tx = tile[t][0], ty = tile[t][1], tz = tile[t][2];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double fx = floor((tx - xr[k]) * v.inv_cell + 0.5);
            const double fy = floor((ty - yr[k]) * v.inv_cell + 0.5);
            const double dz = fabs(tz - zs[k]);
            // compared as float64: a stray coordinate is never converted; NaN fails every test.  (Testing the window
            // on the pre-floor values and flooring only the hits was measured slower: four compares in place of two,
            // 6.96 against 6.01 ms for 10 pairs.)
            if (fabs(fx) <= v.half && fabs(fy) <= v.half && dz <= v.z_window)
                atomicAdd(&hist[((int)fx + v.half_bins) * side + (int)fy + v.half_bins], 1);
        }
    }
}

__global__ __launch_bounds__(VOTE_THREADS) void planar_vote_kernel(Sets st, const PairRows *__restrict__ rows,
                                                                   const double *__restrict__ yaw_cs, int n_yaw,
                                                                   Vote v, int *__restrict__ yaw_peaks,
                                                                   int *__restrict__ votes)
{
    __shared__ int hist[MAX_BINS];
    __shared__ double src[SRC_LIST][3];
    __shared__ double tile[TILE][3];
    __shared__ int n_src, n_tile;
    __shared__ int red[2][VOTE_THREADS / 64];

    const int h = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const PairRows r = rows[p];
    const int side = 2 * v.half_bins + 1, bins = side * side;
    const double c = yaw_cs[2 * h], s = yaw_cs[2 * h + 1];

    for (int i = tid; i < bins; i += VOTE_THREADS) hist[i] = 0;
    if (tid == 0) n_src = 0;
    __syncthreads();

    // an invalid pair has ms = mt = 0: its histogram stays empty and planar_reduce_kernel marks it
    for (long long base = 0; base < r.ms; base += VOTE_THREADS) {
        const long long i = base + tid;
        if (i < r.ms && i % v.stride == 0 && is_structure(st.s_cov + 6 * (r.s_row + i), st.s_thr)) {
            const double *q = st.s_pts + 3 * (r.s_row + i);
            const int at = atomicAdd(&n_src, 1);             // at < SRC_LIST: a round starts with 256 places free
            src[at][0] = q[0];
            src[at][1] = q[1];
            src[at][2] = q[2];
        }
        __syncthreads();
        const int ns = n_src;
        __syncthreads();                                     // everyone has read the count before it moves again
        if (ns <= SRC_LIST - VOTE_THREADS && base + VOTE_THREADS < r.ms) continue;     // uniform: room for 256 more

        // this lane's source rows, rotated once; a place past the list holds NaN and votes for nothing
        double xr[SRC_PER_LANE], yr[SRC_PER_LANE], zs[SRC_PER_LANE];
#pragma unroll
        for (int k = 0; k < SRC_PER_LANE; ++k) {
            const int j = tid + k * VOTE_THREADS;
            if (j < ns) {
                const double x = src[j][0], y = src[j][1];
                xr[k] = c * x - s * y;
                yr[k] = s * x + c * y;
                zs[k] = src[j][2];
            } else {
                xr[k] = yr[k] = zs[k] = __longlong_as_double(0x7ff8000000000000LL);
            }
        }
        const int lane_rows = ns > tid ? (ns - tid + VOTE_THREADS - 1) / VOTE_THREADS : 0;
        const int list_rows = (ns + VOTE_THREADS - 1) / VOTE_THREADS;     // uniform: a short list costs what it holds
        for (long long tb = 0; tb < r.mt; tb += TILE) {
            if (tid == 0) n_tile = 0;
            __syncthreads();                                 // the tile's readers of the round before are done
            const long long j = tb + tid;
            if (j < r.mt && is_structure(st.t_cov + 6 * (r.t_row + j), st.t_thr)) {
                const double *q = st.t_pts + 3 * (r.t_row + j);
                const int at = atomicAdd(&n_tile, 1);
                tile[at][0] = q[0];
                tile[at][1] = q[1];
                tile[at][2] = q[2];
            }
            __syncthreads();
            const int nt = n_tile;
            __syncthreads();                                 // ... and has read its count
            if (lane_rows == 0) continue;                    // no barrier below
            switch (list_rows) {                             // uniform; each count is unrolled on its own
            case 1: vote_tile<1>(tile, nt, xr, yr, zs, v, side, hist); break;
            case 2: vote_tile<2>(tile, nt, xr, yr, zs, v, side, hist); break;
            case 3: vote_tile<3>(tile, nt, xr, yr, zs, v, side, hist); break;
            default: vote_tile<4>(tile, nt, xr, yr, zs, v, side, hist); break;
            }
        }
        if (tid == 0) n_src = 0;                             // read by all before the barrier above; the list's
        __syncthreads();                                     // rows are in registers
    }
    __syncthreads();

    // peak_h and its smallest flat bin
    int best = -1, at = 0;
    for (int i = tid; i < bins; i += VOTE_THREADS) {
        const int n = hist[i];
        if (n > best) {
            best = n;
            at = i;
        }
        if (votes) votes[((long long)p * n_yaw + h) * bins + i] = n;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int ob = __shfl_xor(best, off, 64), oa = __shfl_xor(at, off, 64);
        if (ob > best || (ob == best && oa < at)) {
            best = ob;
            at = oa;
        }
    }
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = best;
        red[1][tid >> 6] = at;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < VOTE_THREADS / 64; ++w) {
            const int ob = red[0][w], oa = red[1][w];
            if (ob > best || (ob == best && oa < at)) {
                best = ob;
                at = oa;
            }
        }
        int *out = yaw_peaks + 2 * ((long long)p * n_yaw + h);
        out[0] = best;
        out[1] = at;
    }
}

__global__ __launch_bounds__(64) void planar_reduce_kernel(const PairRows *__restrict__ rows,
                                                           const int *__restrict__ yaw_peaks,
                                                           const double *__restrict__ yaw_cs, int n_yaw, int guard,
                                                           int half_bins, double cell, int *__restrict__ best_out,
                                                           int *__restrict__ scores, int *__restrict__ counts,
                                                           double *__restrict__ init_out)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    const PairRows r = rows[p];
    const int *pk = yaw_peaks + 2 * (long long)p * n_yaw;
    int peak = -1, best = 0;
    for (int h = lane; h < n_yaw; h += 64)                    // ascending h per lane: the first of equal peaks stays
        if (pk[2 * h] > peak) {
            peak = pk[2 * h];
            best = h;
        }
    for (int off = 32; off > 0; off >>= 1) {
        const int ov = __shfl_xor(peak, off, 64), oh = __shfl_xor(best, off, 64);
        if (ov > peak || (ov == peak && oh < best)) {
            peak = ov;
            best = oh;
        }
    }
    int runner = 0;
    for (int h = lane; h < n_yaw; h += 64) {
        int d = abs(h - best);
        d = min(d, n_yaw - d);
        if (d > guard && pk[2 * h] > runner) runner = pk[2 * h];
    }
    for (int off = 32; off > 0; off >>= 1) runner = max(runner, __shfl_xor(runner, off, 64));

    const bool found = r.valid && peak > 0;
    const int side = 2 * half_bins + 1, bin = pk[2 * best + 1];
    const int bx = bin / side - half_bins, by = bin % side - half_bins;
    if (lane < 16) {
        double val = (lane % 5 == 0) ? 1.0 : 0.0;             // the identity unless a peak was found
        if (found) {
            const double c = yaw_cs[2 * best], s = yaw_cs[2 * best + 1];
            if (lane == 0 || lane == 5) val = c;               // [[c, -s], [s, c]] in rows 0 and 1
            else if (lane == 1) val = -s;
            else if (lane == 4) val = s;
            else if (lane == 3) val = (double)bx * cell;
            else if (lane == 7) val = (double)by * cell;
        }
        init_out[16 * (long long)p + lane] = val;
    }
    if (lane == 0) {
        int *b = best_out + 3 * (long long)p;
        b[0] = found ? best : -1;
        b[1] = found ? bx : 0;
        b[2] = found ? by : 0;
        scores[2 * (long long)p] = r.valid ? peak : -1;
        scores[2 * (long long)p + 1] = r.valid ? (found ? runner : 0) : -1;
        counts[2 * (long long)p] = r.taken;
        counts[2 * (long long)p + 1] = r.structure;
    }
}

struct Regions {                     // the workspace
    PairRows *rows;
    int *peaks;
    size_t total;
};

// ws = nullptr: the size only
Regions regions(void *ws, size_t n_pairs, size_t n_yaw)
{
    Carver c = {reinterpret_cast<uintptr_t>(ws), 0};
    Regions r;
    r.rows = c.take<PairRows>(n_pairs);
    r.peaks = c.take<int>(n_pairs * n_yaw * 2);
    r.total = c.o;
    return r;
}

bool set_ok(const NscGicpCloudSet *s)
{
    if (!s->row_offsets || !s->points || !s->covariances) return false;
    return s->n_clouds >= 0 && s->n_rows >= 0 && s->n_clouds <= s->cap_clouds && s->n_rows <= s->cap_rows &&
           s->voxel_size > 0.0 && isfinite(s->voxel_size);
}

// the largest count a bin can reach from `rows` source rows (header: "Counts")
bool counts_fit(const NscGicpCloudSet *sources, const NscGicpCloudSet *targets, const NscPlanarParams *p)
{
    const double v = targets->voxel_size;
    const double per_axis = floor(p->cell / v) + 2.0, per_z = floor(2.0 * p->z_window / v) + 2.0;
    double per_row = per_axis * per_axis * per_z;
    if (!(per_row < (double)targets->n_rows)) per_row = (double)targets->n_rows;
    return (double)sources->n_rows * per_row <= 2147483647.0;
}

}  // namespace

extern "C" {

void nsc_planar_default_params(NscPlanarParams *p)
{
    if (!p) return;
    p->cell = 0.5;
    p->z_window = 0.5;
    p->normal_z2_max = 0.25;
    p->half_bins = 24;
    p->source_stride = 2;
    p->guard = 5;
}

size_t nsc_planar_align_workspace_bytes(int32_t n_pairs, int32_t n_yaw)
{
    if (n_pairs < 0 || n_yaw < 1) return 0;
    return regions(nullptr, n_pairs, n_yaw).total;
}

int nsc_planar_align(const NscGicpCloudSet *sources, const NscGicpCloudSet *targets, const int64_t *source_ids,
                     const int64_t *target_ids, int32_t n_pairs, const double *yaw_cs, int32_t n_yaw,
                     const NscPlanarParams *params, int32_t *best, int32_t *scores, int32_t *counts,
                     double *init_transforms, const NscPlanarStages *stages, void *ws, size_t ws_bytes, void *stream)
{
    if (n_pairs < 0 || n_yaw < 1 || !sources || !targets || !params) return NSC_EINVAL;
    if (!(params->cell > 0.0) || !isfinite(params->cell) || !(params->z_window >= 0.0) || !isfinite(params->z_window) ||
        !isfinite(params->normal_z2_max) || params->source_stride < 1 || params->guard < 0)
        return NSC_EINVAL;
    if (params->half_bins < 1) return NSC_EINVAL;
    if (params->half_bins > NSC_PLANAR_MAX_HALF_BINS) return NSC_EUNSUPPORTED;
    if (!set_ok(sources) || !set_ok(targets)) return NSC_EINVAL;
    if (n_pairs > NSC_PLANAR_MAX_PAIRS || !counts_fit(sources, targets, params)) return NSC_EUNSUPPORTED;
    if (n_pairs == 0) return NSC_OK;
    if (!source_ids || !target_ids || !yaw_cs || !best || !scores || !counts || !init_transforms) return NSC_EINVAL;
    const Regions r = regions(ws, n_pairs, n_yaw);
    if (!ws || ws_bytes < r.total) return NSC_EWORKSPACE;
    PairRows *rows = r.rows;
    int *peaks = r.peaks;
    int *votes = nullptr;
    if (stages) {                        // a stage output replaces the workspace region it names
        if (stages->yaw_peaks) peaks = stages->yaw_peaks;
        votes = stages->votes;
    }
    const Sets st{reinterpret_cast<const long long *>(sources->row_offsets),
                  reinterpret_cast<const long long *>(targets->row_offsets),
                  sources->points, sources->covariances, targets->points, targets->covariances,
                  (long long)sources->n_clouds, (long long)targets->n_clouds,
                  params->normal_z2_max * (1.0 - sources->epsilon), params->normal_z2_max * (1.0 - targets->epsilon)};
    const Vote v{1.0 / params->cell, params->z_window, (double)params->half_bins, params->half_bins,
                 params->source_stride};
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(planar_setup_kernel, dim3(n_pairs), dim3(SETUP_THREADS), 0, s, st,
                       reinterpret_cast<const long long *>(source_ids), reinterpret_cast<const long long *>(target_ids),
                       params->source_stride, rows);
    hipLaunchKernelGGL(planar_vote_kernel, dim3(n_yaw, n_pairs), dim3(VOTE_THREADS), 0, s, st, rows, yaw_cs, n_yaw, v,
                       peaks, votes);
    hipLaunchKernelGGL(planar_reduce_kernel, dim3(n_pairs), dim3(64), 0, s, rows, peaks, yaw_cs, n_yaw, params->guard,
                       params->half_bins, params->cell, best, scores, counts, init_transforms);
    return launch_status();
}

}  // extern "C"
