// nsc_yaw.hip -- yaw initial guess for stage 2 of loop closing: the circular column shift that best aligns the
// interpolated range images of two scans of one place.
//
// A yaw between two scans of one place is a circular shift of the 360 columns of the range image the encoder
// already builds (csrc/nsc_encoder.hip, the `interpolated` output).  The definition the kernel and
// tests/yaw_restatement.py share (retrieval/yaw_alignment.py), all in float64:
//   a[r,c]   = Iq[r,c] - mean_c Iq[r,:],  b likewise from Ic
//   score[s] = sum_r sum_c a[r,c] * b[r,(c - s) mod 360]                       s = 0 .. 359
//   shift    = arg max score, ties to the smaller s; 0 when that score is not > 0 (flat or empty images)
//   peak     = score[shift];  runner_up = max score over shifts more than NSC_YAW_GUARD_BINS bins from shift
//   init     = Rz(-shift degrees wrapped to (-180, 180]); exactly the identity for shift 0
// Images that are not finite: one NaN or +-inf pixel among the R rows of either image makes its row mean, and with it
// every one of the 360 scores, NaN (finite float32 images cannot overflow float64: |score| < 64 * 360 * 2^258).  Such
// a pair gets shift 0, the identity bit for bit, peak NaN and runner_up NaN.  It stays distinct from a pair with an id
// outside its array, which gets shift -1 (and the identity and NaN scores) without an image read.
//
// One launch, one workgroup of 12 waves per pair, no workspace:
//   rows are taken in chunks of 16.  Per chunk: row means (one wave per row, lane-strided float64 sums and a
//   butterfly, a fixed order), then both mean-removed images are staged in LDS as float64 -- a as 16 x 360, b as
//   16 x 720 with every row stored twice in a row, so (c - s) mod 360 is the plain index c - s + 360:
//   45 KB + 90 KB of the CU's 160 KB.  The loop is bound by LDS reads, not by the float64 FMAs, so a lane owns
//   the two consecutive shifts 2t, 2t + 1 (t = (w % 3) * 64 + lane < 180) and walks the columns in pairs: one
//   16-byte read of b[r, c - 2t + 360 .. + 1] (consecutive lanes on consecutive 16 bytes: conflict-free
//   ds_read_b128; the third value the pair needs is the previous read's second) and one 16-byte broadcast of
//   a[r, c .. c + 1] feed four FMAs.  Wave w takes the rows 4 (w / 3) .. + 3 of the chunk.  Every lane keeps two
//   float64 accumulators per shift (even and odd columns) through all chunks; they and the four row groups are
//   added in a fixed order, so a pair's result depends on nothing but its two images: not on the batch, not on
//   the run.
//   Wave 0 then finds the peak and the runner-up (lane-strided scan in ascending s, butterfly with ties to the
//   smaller s) and writes the pair's outputs.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nsc.h"
#include "nsc_util.h"

namespace {

constexpr int COLS = 360;
constexpr int CHUNK = 16;                       // rows staged per round
constexpr int SHIFT_WAVES = 3;                  // 3 x 64 lanes >= 180 pairs of shifts
constexpr int ROW_SPLIT = 4;                    // row groups of a chunk, one set of shift waves each
constexpr int GROUP_ROWS = CHUNK / ROW_SPLIT;
constexpr int YAW_WAVES = SHIFT_WAVES * ROW_SPLIT;
constexpr int YAW_THREADS = 64 * YAW_WAVES;     // 768: three waves per SIMD
constexpr int MAX_ROWS = 64;
constexpr int GUARD = NSC_YAW_GUARD_BINS;
// hipLaunchKernel takes at most 2^32 - 1 threads per grid
static_assert((long long)NSC_YAW_MAX_PAIRS * YAW_THREADS < (1LL << 32), "NSC_YAW_MAX_PAIRS must fit one launch");
static_assert(SHIFT_WAVES * 128 >= COLS && COLS % 2 == 0 && CHUNK % ROW_SPLIT == 0, "layout");

__global__ __launch_bounds__(YAW_THREADS) void yaw_align_kernel(const float *__restrict__ images_q, long long n_q,
                                                               const float *__restrict__ images_c, long long n_c,
                                                               const long long *__restrict__ ids_q,
                                                               const long long *__restrict__ ids_c, int rows,
                                                               int *__restrict__ shift_out,
                                                               double *__restrict__ scores_out,
                                                               double *__restrict__ init_out)
{
    __shared__ __align__(16) double a[CHUNK * COLS];
    __shared__ __align__(16) double b2[CHUNK * 2 * COLS];
    __shared__ double mean_q[CHUNK], mean_c[CHUNK];
    __shared__ double partial[ROW_SPLIT][SHIFT_WAVES * 64][2];
    __shared__ double score[COLS];

    const long long pair = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long iq = ids_q[pair], ic = ids_c[pair];
    double *init = init_out + pair * 16;
    if (iq < 0 || iq >= n_q || ic < 0 || ic >= n_c) {          // uniform over the workgroup; nothing is read
        if (tid < 16) init[tid] = (tid % 5 == 0) ? 1.0 : 0.0;
        if (tid == 0) {
            shift_out[pair] = -1;
            scores_out[2 * pair] = scores_out[2 * pair + 1] = __longlong_as_double(0x7ff8000000000000LL);
        }
        return;
    }
    const float *q = images_q + iq * rows * COLS;
    const float *c = images_c + ic * rows * COLS;

    const int group = wave / SHIFT_WAVES;
    const int slot = (wave % SHIFT_WAVES) * 64 + lane;
    const int t = min(slot, COLS / 2 - 1);                  // shifts 2t, 2t + 1; slots past 179 repeat the last pair
    double e0 = 0.0, o0 = 0.0, e1 = 0.0, o1 = 0.0;          // shift 2t / 2t + 1, even / odd columns

    for (int r0 = 0; r0 < rows; r0 += CHUNK) {
        const int n = min(CHUNK, rows - r0);
        const float *qr = q + (long long)r0 * COLS, *cr = c + (long long)r0 * COLS;
        for (int r = wave; r < n; r += YAW_WAVES) {
            double sq = 0.0, sc = 0.0;
            for (int k = lane; k < COLS; k += 64) {
                sq += (double)qr[r * COLS + k];
                sc += (double)cr[r * COLS + k];
            }
            sq = nsc_wave_sum(sq);
            sc = nsc_wave_sum(sc);
            if (lane == 0) {
                mean_q[r] = sq / (double)COLS;
                mean_c[r] = sc / (double)COLS;
            }
        }
        __syncthreads();
        for (int i = tid; i < n * COLS; i += YAW_THREADS) {
            const int r = i / COLS, k = i - r * COLS;
            a[i] = (double)qr[i] - mean_q[r];
            const double v = (double)cr[i] - mean_c[r];
            b2[r * 2 * COLS + k] = v;
            b2[r * 2 * COLS + COLS + k] = v;
        }
        __syncthreads();
        const int r_end = min(n, (group + 1) * GROUP_ROWS);
        for (int r = group * GROUP_ROWS; r < r_end; ++r) {
            const double2 *ar = reinterpret_cast<const double2 *>(a + r * COLS);
            const double *br = b2 + r * 2 * COLS + (COLS - 2 * t);      // b[r, c - 2t] at c = 0: an even index, >= 2
            double prev = br[-1];                                        // b[r, c - (2t + 1)] at c = 0
#pragma unroll 4
            for (int k = 0; k < COLS / 2; ++k) {                         // columns c = 2k, 2k + 1
                const double2 av = ar[k];
                const double2 bv = *reinterpret_cast<const double2 *>(br + 2 * k);
                e0 = fma(av.x, bv.x, e0);
                o0 = fma(av.y, bv.y, o0);
                e1 = fma(av.x, prev, e1);
                o1 = fma(av.y, bv.x, o1);
                prev = bv.y;
            }
        }
        __syncthreads();                                               // the next chunk overwrites a and b2
    }
    partial[group][slot][0] = e0 + o0;
    partial[group][slot][1] = e1 + o1;
    __syncthreads();
    if (tid < COLS) {
        double v = partial[0][tid >> 1][tid & 1];
        for (int g = 1; g < ROW_SPLIT; ++g) v += partial[g][tid >> 1][tid & 1];
        score[tid] = v;
    }
    __syncthreads();
    if (wave != 0) return;

    double best = score[lane];
    int at = lane;
    for (int k = lane + 64; k < COLS; k += 64)
        if (score[k] > best) {
            best = score[k];
            at = k;
        }
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(at, off, 64);
        if (ov > best || (ov == best && oi < at)) {
            best = ov;
            at = oi;
        }
    }
    const int shift = best > 0.0 ? at : 0;
    double runner = -INFINITY;
    for (int k = lane; k < COLS; k += 64) {
        int d = abs(k - shift);
        d = min(d, COLS - d);
        if (d > GUARD && score[k] > runner) runner = score[k];
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(runner, off, 64);
        if (ov > runner) runner = ov;
    }
    if (lane < 16) {
        double v = (lane % 5 == 0) ? 1.0 : 0.0;
        if (shift != 0) {                                               // shift 0: the identity, exactly
            const int deg = shift < 180 ? -shift : 360 - shift;         // -shift wrapped to (-180, 180]
            const double yaw = (double)deg * (M_PI / 180.0);
            const double cy = cos(yaw), sy = sin(yaw);
            if (lane == 0 || lane == 5) v = cy;                         // [[c, -s], [s, c]] in rows 0 and 1
            else if (lane == 1) v = -sy;
            else if (lane == 4) v = sy;
        }
        init[lane] = v;
    }
    if (lane == 0) {
        const double peak = score[shift];
        shift_out[pair] = shift;
        scores_out[2 * pair] = peak;
        scores_out[2 * pair + 1] = peak != peak ? peak : runner;        // all scores NaN: no comparison above held
    }
}

}  // namespace

extern "C" {

int nsc_yaw_align(const float *images_q, int32_t n_q, const float *images_c, int32_t n_c, const int64_t *ids_q,
                  const int64_t *ids_c, int32_t n_pairs, int32_t rows, int32_t *shift, double *scores,
                  double *init_transforms, void *stream)
{
    if (n_pairs < 0 || n_q < 0 || n_c < 0 || rows < 1 || rows > MAX_ROWS) return NSC_EINVAL;
    if (n_pairs > NSC_YAW_MAX_PAIRS) return NSC_EUNSUPPORTED;
    if (n_pairs == 0) return NSC_OK;
    if (!images_q || !images_c || !ids_q || !ids_c || !shift || !scores || !init_transforms) return NSC_EINVAL;
    hipLaunchKernelGGL(yaw_align_kernel, dim3(n_pairs), dim3(YAW_THREADS), 0, static_cast<hipStream_t>(stream),
                       images_q, (long long)n_q, images_c, (long long)n_c, reinterpret_cast<const long long *>(ids_q),
                       reinterpret_cast<const long long *>(ids_c), rows, shift, scores, init_transforms);
    return launch_status();
}

}  // extern "C"
