// nsc_posegraph.hip -- pose-graph optimisation: odometry edges and verified loop closures in, corrected poses out.
// Float64 throughout.  The contract is stated in include/nsc.h (nsc_posegraph_optimize); tests/posegraph_restatement.py
// restates it in numpy; DESIGN.md section 4.11 has the launch sequence and the measurements.  nsc_posegraph_covariance
// (marginal covariances of selected poses: PCG on many right-hand sides at once) has a section of its own below.
//
//   D = Z^-1 X_i^-1 X_j,  r = [Log_SO3(R_D); t_D],  F = sum r^T Omega r,  update X_k <- [R_k Exp(phi_k) | t_k + R_k rho_k]
//   J_j = B = blockdiag(Jr^-1(r_phi), R_D),  J_i = -B Ad(A^-1) with A = X_i^-1 X_j
//   Levenberg-Marquardt with Marquardt scaling, (H + lambda diag H) delta = -g, solved by conjugate gradients
//   preconditioned with the Cholesky factor of each node's damped 6 x 6 diagonal block.
//   Robust kernels (nsc_posegraph_*_robust): with s = r^T Omega r and an edge's width c, F = sum rho(s),
//   g = sum w J^T Omega r, H = sum w J^T Omega J, w = rho'(s): iteratively reweighted, no second-order term.
//   edge_eval() is the one place s, rho and w are formed: pg_edge_cost_kernel (the cost, and the per-edge chi2 and w a
//   caller asks for) and pg_linearize_kernel both call it.
//
// Shape.  Every workgroup is one wave of 64 lanes: a graph of a few thousand poses is a few dozen waves, and one wave per
// workgroup spreads them over as many CUs; every reduction is then a butterfly of the wave, with no LDS and no barrier.
// One lane per edge linearises (pg_linearize_kernel: the four blocks of J^T Omega J and the two halves of J^T Omega r, kept
// structure-of-arrays so that the 78 block values of 64 neighbouring edges are read in 78 coalesced requests) and forms the
// edge half of H p (pg_edge_matvec_kernel); one lane per node gathers over the node's incident edges, in ascending
// edge index (the lists are built once per call).  A node of degree 300 is one lane walking 300 entries: correct, not
// fast; the graphs this is for have degree 2 to 4 almost everywhere.
//
// Determinism.  No floating-point atomics.  Node quantities are gathered in list order.  A scalar (cost, p.Ap, r.r,
// r.z, |delta|^2) is written as one partial per workgroup of nodes (the cost too: each node sums the edges it is the
// first end of); every consumer sums the partials itself, lane l taking partials l, l + 64, ... in ascending order and
// the wave finishing with the same butterfly, so every workgroup of every consumer holds the same bits.  The integer
// atomics that build the lists only count; the order they hand places out in is removed by ranking each node's
// entries.
//
// Control.  The launch sequence depends on the parameters alone.  All solver state lives in PgState on the device.
// `done` is written by single-wave kernels only and read at the top of every later kernel.  The inner loop ends through
// `stop_k`: iteration k runs iff k < stop_k, and the kernel that ends the loop at iteration k writes k + 1, so its own
// workgroups, which read stop_k while it is being written, see "run" either way.  The two r.z values alternate between
// two slots for the same reason.
//
// Two-level preconditioner (nsc_posegraph_optimize_coarse, coarse_block = L >= 2; include/nsc.h has the mathematics).
// Aggregate a holds the poses a L .. a L + L - 1; the coarse space is one rigid motion per aggregate, P's block of a free
// pose k being Ad(X_k^-1 X_ref); M^-1 r = B^-1 r + P A_c^-1 P^T r with A_c = P^T (H + lambda diag H) P.  Per outer step,
// after linearise and assemble: pg_coarse_basis_kernel (one lane per node: P), pg_coarse_galerkin_kernel (one wave per
// block (a, b), a <= b, of A_c: it walks the incident lists of a's nodes in ascending order and writes the block and its
// transpose), pg_coarse_factor_kernel (one workgroup of 512: right-looking Cholesky in global memory, U and U^T),
// pg_coarse_invert_kernel (one wave per column of A_c^-1: two substitutions in axpy form, the running column in
// registers), then the restrict and prolong kernels once on the start of PCG.  Per inner iteration the step kernel is
// replaced by pg_coarse_restrict_kernel (one wave per aggregate: the step, B^-1 r and its six entries of P^T r) and
// pg_coarse_prolong_kernel (one wave per aggregate: its six rows of A_c^-1 r_c, z += P y, the partials of r.r and r.z,
// one per aggregate, which pg_pcg_begin_kernel and pg_pcg_direction_kernel are handed in place of those per workgroup of
// nodes): five launches per inner iteration.  The same house rules hold: no floating-point atomics, every sum in a
// fixed order (a lane sums its nodes in ascending order, the wave finishes with the butterfly), no host
// synchronisation, no memset or memcpy nodes, no cooperative launch or grid barrier, `done` and `stop_k` honoured by
// every kernel, and a launch sequence that depends only on the parameters, N > 0, E > 0 and coarse_block:
//   5 (lists) + 1 (copy, unless aliased) + 3 + max_iteration (14 + 5 max_pcg_iterations) + 1 (+ 1 for chi2 / weights).
// A pivot of A_c that is not positive and finite leaves that outer step with B^-1 alone and is counted.
//
// Host.  layout() is the one place that knows the workspace (the graph's regions, then the coarse space's, then the
// covariance call's), graph_ok() the one check of the graph arguments, build_lists() the five launches of the incident
// lists (the scan is nsc_util.h's), launch_system() the launches from the linearisation to A_c^-1 that the optimiser runs
// per outer step and the covariance call once.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nsc.h"
#include "nsc_fill.h"
#include "nsc_robust.h"                 // Robust, robust_rho_w
#include "nsc_util.h"

namespace {

constexpr int TB = 64;                       // lanes per workgroup: one wave

struct PgState {
    double lambda, cost, cost0, bb, rz[2], step;
    int done, converged, stop_k, accept_it, iterations, accepted, rejected, pcg_total, skipped, pad;
};

struct Buffers {                             // the graph's part of the workspace: typed pointers into it
    PgState *st;                             // the head, head_bytes long: the state, then deg; zeroed as one
    int *row_ptr, *deg, *tmp, *list, *ei, *ej, *free_node;   // row_ptr (N + 1); deg (N): degrees, then places to hand out
    double *hii, *hjj, *hij;                 // (21,E), (21,E), (36,E)
    double *fe;                              // (E): rho(r^T Omega r)
    double *ge, *ye;                         // (E,12): J^T Omega r and the edge half of H p, node i's six then node j's
    size_t head_bytes;                       // here, eight bytes like the pointers around it: the struct is the kernels'
                                             // argument, and with the pointers below eight bytes further up
                                             // pg_pcg_step_kernel was compiled with its loads one behind the other: 1 us
    double *blocks, *chol;                   // (N,21), (N,21)
    double *x, *r, *z, *p, *ap;              // (N,6)
    double *cand;                            // (N,4,4), rows 0..2 used
    double *part_e, *part_a, *part_b, *part_s;   // partials, one per workgroup of nodes: cost, p.Ap, (r.r, r.z), |delta|^2
};

struct PgCoarse {
    int ok, failed;                          // this outer step's factor of A_c stands; outer steps whose factor failed
};

struct Coarse {                              // the coarse space's part of the workspace, behind Buffers'
    PgCoarse *cs;
    double *t;                               // (N,36): P's block of every node, row-major, zero for a node that is not free
    double *ac, *lt, *ainv;                  // (nc,nc): A_c, then U (upper triangle);  U^T;  A_c^-1
    double *rc;                              // (nc): P^T r
    double *part;                            // (2 n_agg): partials of r.r and r.z, one per aggregate
    int L, n_agg, nc;                        // nc = 6 n_agg
};

// the sum of nb partials, the same bits in every lane of every wave that calls it
__device__ __forceinline__ double finish(const double *part, int nb)
{
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += TB) s += part[i];
    return nsc_wave_sum(s);
}

__device__ __forceinline__ void write_partial(double *part, double v)
{
    v = nsc_wave_sum(v);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// ---- rotations -------------------------------------------------------------------------------------------------

__device__ __forceinline__ void load_pose(const double *P, long long n, double R[9], double t[3])
{
    const double *q = P + 16 * n;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        R[3 * r] = q[4 * r];
        R[3 * r + 1] = q[4 * r + 1];
        R[3 * r + 2] = q[4 * r + 2];
        t[r] = q[4 * r + 3];
    }
}

// C = A^T B
__device__ __forceinline__ void mul_tn(const double A[9], const double B[9], double C[9])
{
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[r] * B[c] + A[3 + r] * B[3 + c] + A[6 + r] * B[6 + c];
}

// y = A^T x
__device__ __forceinline__ void mulv_t(const double A[9], const double x[3], double y[3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) y[r] = A[r] * x[0] + A[3 + r] * x[1] + A[6 + r] * x[2];
}

__device__ __forceinline__ void hat(const double v[3], double K[9])
{
    K[0] = 0.0;   K[1] = -v[2]; K[2] = v[1];
    K[3] = v[2];  K[4] = 0.0;   K[5] = -v[0];
    K[6] = -v[1]; K[7] = v[0];  K[8] = 0.0;
}

// M = I + a [v]x + b [v]x^2, with [v]x^2 = v v^T - |v|^2 I
__device__ __forceinline__ void rodrigues_form(const double v[3], double a, double b, double M[9])
{
    const double n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    double K[9];
    hat(v, K);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            M[3 * r + c] = (r == c ? 1.0 : 0.0) + a * K[3 * r + c] + b * (v[r] * v[c] - (r == c ? n2 : 0.0));
}

__device__ __forceinline__ void exp_so3(const double phi[3], double R[9])
{
    const double t2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
    double a, b;
    if (t2 < 1e-8) {
        a = 1.0 - t2 / 6.0 + t2 * t2 / 120.0;
        b = 0.5 - t2 / 24.0 + t2 * t2 / 720.0;
    } else {
        const double t = sqrt(t2);
        a = sin(t) / t;
        b = (1.0 - cos(t)) / t2;
    }
    rodrigues_form(phi, a, b, R);
}

__device__ __forceinline__ void log_so3(const double R[9], double phi[3])
{
    const double v[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
    const double s = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double k = s < 1e-12 ? 1.0 : atan2(s, 0.5 * (R[0] + R[4] + R[8] - 1.0)) / s;
    phi[0] = v[0] * k;
    phi[1] = v[1] * k;
    phi[2] = v[2] * k;
}

__device__ __forceinline__ void jr_inv(const double phi[3], double J[9])
{
    const double t2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
    const double t = sqrt(t2);
    const double c = t < 1e-4 ? 1.0 / 12.0 + t2 / 720.0 : 1.0 / t2 - (1.0 + cos(t)) / (2.0 * t * sin(t));
    rodrigues_form(phi, 0.5, c, J);
}

// A = X_i^-1 X_j and D = Z^-1 A of one edge, and the residual
struct EdgeGeom {
    double RA[9], tA[3], RD[9], RZ[9], r[6];
};

__device__ __forceinline__ void edge_geometry(const double *poses, long long i, long long j, const double *Z, long long e,
                                              EdgeGeom &q)
{
    double Ri[9], ti[3], Rj[9], tj[3], tz[3];
    load_pose(poses, i, Ri, ti);
    load_pose(poses, j, Rj, tj);
    load_pose(Z, e, q.RZ, tz);
    mul_tn(Ri, Rj, q.RA);
    const double d[3] = {tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2]};
    mulv_t(Ri, d, q.tA);
    mul_tn(q.RZ, q.RA, q.RD);
    const double f[3] = {q.tA[0] - tz[0], q.tA[1] - tz[1], q.tA[2] - tz[2]};
    mulv_t(q.RZ, f, q.r + 3);
    log_so3(q.RD, q.r);
}

// Omega of edge e as a full symmetric matrix; only the upper triangle of the input is read
__device__ __forceinline__ void load_information(const double *information, long long e, double W[36])
{
    const double *q = information + 36 * e;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) W[6 * r + c] = W[6 * c + r] = q[6 * r + c];
}

__device__ __forceinline__ double quad_form(const double W[36], const double r[6])
{
    double f = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double w = 0.0;
#pragma unroll
        for (int b = 0; b < 6; ++b) w += W[6 * a + b] * r[b];
        f += r[a] * w;
    }
    return f;
}

// rho(s) and w = rho'(s) of one edge (nsc_robust.h; include/nsc.h has the table).  The edge is quadratic, rho = s and
// w = 1 exactly, for kernel 0, without widths, for a width c that is not finite and positive or whose square is not, and
// for s <= 0 or NaN.
__device__ __forceinline__ Robust robust_kernel(int kernel, const double *__restrict__ edge_scale, long long e, double s)
{
    if (kernel == NSC_POSEGRAPH_KERNEL_NONE || !edge_scale) return Robust{s, 1.0};
    return robust_rho_w(kernel, edge_scale[e], s);
}

// One edge at `poses`: its geometry, Omega as given, s = r^T Omega r, and rho(s) and w.  Every kernel that needs any of
// them takes them from here, so the cost the accept test compares and the model it is compared with are one sum.
__device__ __forceinline__ Robust edge_eval(const double *poses, long long i, long long j, const double *Z,
                                            const double *information, long long e, int kernel, const double *edge_scale,
                                            EdgeGeom &q, double W[36], double &s)
{
    edge_geometry(poses, i, j, Z, e, q);
    load_information(information, e, W);
    s = quad_form(W, q.r);
    return robust_kernel(kernel, edge_scale, e, s);
}

// index of (r, c), r <= c, in a row-major upper triangle of a 6 x 6 matrix
__device__ __host__ constexpr int tri(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }

// ---- incident-edge lists -----------------------------------------------------------------------------------------

__global__ __launch_bounds__(TB) void pg_count_kernel(const long long *__restrict__ edge_ij, int n_edges, int n_poses,
                                                      Buffers b)
{
    const int e = blockIdx.x * TB + threadIdx.x;
    if (e >= n_edges) return;
    const long long i = edge_ij[2 * (long long)e], j = edge_ij[2 * (long long)e + 1];
    const bool ok = i != j && i >= 0 && i < n_poses && j >= 0 && j < n_poses;
    b.ei[e] = ok ? (int)i : -1;
    b.ej[e] = ok ? (int)j : -1;
    if (ok) {
        atomicAdd(&b.deg[i], 1);
        atomicAdd(&b.deg[j], 1);
    } else {
        atomicAdd(&b.st->skipped, 1);
    }
}

// after the scan of the degrees into row_ptr: a node's places are handed out from its last down, until deg is zero again
__global__ __launch_bounds__(TB) void pg_fill_kernel(int n_edges, Buffers b)
{
    const int e = blockIdx.x * TB + threadIdx.x;
    if (e >= n_edges) return;
    const int i = b.ei[e], j = b.ej[e];
    if (i < 0) return;
    b.tmp[b.row_ptr[i] + atomicSub(&b.deg[i], 1) - 1] = 2 * e;
    b.tmp[b.row_ptr[j] + atomicSub(&b.deg[j], 1) - 1] = 2 * e + 1;
}

// one wave per node: its entries (2 e + side, all different) into ascending order by rank
__global__ __launch_bounds__(TB) void pg_sort_kernel(Buffers b)
{
    const int n = blockIdx.x;
    const int lo = b.row_ptr[n], hi = b.row_ptr[n + 1];
    for (int a = lo + threadIdx.x; a < hi; a += TB) {
        const int v = b.tmp[a];
        int rank = 0;
        for (int c = lo; c < hi; ++c) rank += b.tmp[c] < v;
        b.list[lo + rank] = v;
    }
}

__global__ __launch_bounds__(TB) void pg_copy_kernel(const double *__restrict__ src, double *__restrict__ dst, long long n)
{
    const long long i = (long long)blockIdx.x * TB + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// ---- edges -------------------------------------------------------------------------------------------------------

// One lane per edge at `poses`, each output where its pointer is given: rho(s) into fe (what the cost sums), s = r^T Omega r
// into chi2 and w into weight (what a caller drops closures by).  A skipped edge writes nothing to fe, zeros to the others.
// after_done: the launch that runs whatever `done` says, the chi2 and weights at the final poses.
__global__ __launch_bounds__(TB) void pg_edge_cost_kernel(const double *poses, const double *__restrict__ Z,
                                                          const double *__restrict__ information, int n_edges, Buffers b,
                                                          int after_done, int kernel, const double *__restrict__ edge_scale,
                                                          double *fe, double *__restrict__ chi2,
                                                          double *__restrict__ weight)
{
    if (!after_done && b.st->done) return;
    const int e = blockIdx.x * TB + threadIdx.x;
    if (e >= n_edges) return;
    const bool counted = b.ei[e] >= 0;
    double s = 0.0;
    Robust rb{0.0, 0.0};
    if (counted) {
        EdgeGeom q;
        double W[36];
        rb = edge_eval(poses, b.ei[e], b.ej[e], Z, information, e, kernel, edge_scale, q, W, s);
    }
    if (fe && counted) fe[e] = rb.rho;
    if (chi2) chi2[e] = s;
    if (weight) weight[e] = rb.w;
}

// F: every node sums the edges it is the first end of, in list order; one partial per workgroup.  The sum walks the
// lists, which hold counted edges only, so where the skipped edges stand among the others does not change a bit of it.
// Before the first accept kernel of a call `done` is 0, as build_lists left it, so every launch may test it.
__global__ __launch_bounds__(TB) void pg_cost_gather_kernel(int n_poses, Buffers b)
{
    if (b.st->done) return;
    const int n = blockIdx.x * TB + threadIdx.x;
    double f = 0.0;
    if (n < n_poses) {
        const int lo = b.row_ptr[n], hi = b.row_ptr[n + 1];
        for (int a = lo; a < hi; ++a) {
            const int code = b.list[a];
            if (!(code & 1)) f += b.fe[code >> 1];
        }
    }
    write_partial(b.part_e, f);
}

// residual, weight, the blocks of w J^T Omega J and the halves of w J^T Omega r of every edge (`done` as in the gather)
__global__ __launch_bounds__(TB) void pg_linearize_kernel(const double *poses, const double *__restrict__ Z,
                                                          const double *__restrict__ information, int n_edges,
                                                          Buffers b, double *__restrict__ residuals, int kernel,
                                                          const double *__restrict__ edge_scale,
                                                          double *__restrict__ weights)
{
    if (b.st->done) return;
    const int e = blockIdx.x * TB + threadIdx.x;
    if (e >= n_edges) return;
    if (b.ei[e] < 0) {
        if (residuals)
            for (int k = 0; k < 6; ++k) residuals[6 * (long long)e + k] = 0.0;
        if (weights) weights[e] = 0.0;
        return;
    }
    EdgeGeom q;
    double W[36], chi2;
    const double w = edge_eval(poses, b.ei[e], b.ej[e], Z, information, e, kernel, edge_scale, q, W, chi2).w;
    if (residuals)
        for (int k = 0; k < 6; ++k) residuals[6 * (long long)e + k] = q.r[k];
    if (weights) weights[e] = w;

    // J_j = blockdiag(Jr^-1, R_D);  J_i = -[[Jr^-1 R_A^T, 0], [-R_Z^T [t_A]x, R_Z^T]]  (R_D R_A^T = R_Z^T)
    double Ji[36], Jj[36], Jr[9], K[9];
    jr_inv(q.r, Jr);
    hat(q.tA, K);
#pragma unroll
    for (int k = 0; k < 36; ++k) Ji[k] = Jj[k] = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Jj[6 * r + c] = Jr[3 * r + c];
            Jj[6 * (r + 3) + c + 3] = q.RD[3 * r + c];
            // (Jr R_A^T)[r][c] = sum_k Jr[r][k] R_A[c][k];  (R_Z^T K)[r][c] = sum_k R_Z[k][r] K[k][c]
            Ji[6 * r + c] = -(Jr[3 * r] * q.RA[3 * c] + Jr[3 * r + 1] * q.RA[3 * c + 1] + Jr[3 * r + 2] * q.RA[3 * c + 2]);
            Ji[6 * (r + 3) + c] = q.RZ[r] * K[c] + q.RZ[3 + r] * K[3 + c] + q.RZ[6 + r] * K[6 + c];
            Ji[6 * (r + 3) + c + 3] = -q.RZ[3 * c + r];
        }

    // Omega <- w Omega
    double Wi[36], Wj[36], wr[6];
#pragma unroll
    for (int k = 0; k < 36; ++k) W[k] *= w;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double si = 0.0, sj = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                si += W[6 * a + k] * Ji[6 * k + c];
                sj += W[6 * a + k] * Jj[6 * k + c];
            }
            Wi[6 * a + c] = si;
            Wj[6 * a + c] = sj;
            s += W[6 * a + c] * q.r[c];
        }
        wr[a] = s;
    }
    const long long E = n_edges;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double gi = 0.0, gj = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            gi += Ji[6 * k + r] * wr[k];
            gj += Jj[6 * k + r] * wr[k];
        }
        b.ge[12 * (long long)e + r] = gi;
        b.ge[12 * (long long)e + 6 + r] = gj;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double hii = 0.0, hjj = 0.0, hij = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                hii += Ji[6 * k + r] * Wi[6 * k + c];
                hjj += Jj[6 * k + r] * Wj[6 * k + c];
                hij += Ji[6 * k + r] * Wj[6 * k + c];
            }
            b.hij[(6 * r + c) * E + e] = hij;
            if (c >= r) {
                b.hii[tri(r, c) * E + e] = hii;
                b.hjj[tri(r, c) * E + e] = hjj;
            }
        }
    }
}

// the edge half of H p: y_i = H_ii p_i + H_ij p_j, y_j = H_ij^T p_i + H_jj p_j
__global__ __launch_bounds__(TB) void pg_edge_matvec_kernel(int n_edges, Buffers b, int k)
{
    if (b.st->done || k >= b.st->stop_k) return;
    const int e = blockIdx.x * TB + threadIdx.x;
    if (e >= n_edges) return;
    const int i = b.ei[e], j = b.ej[e];
    if (i < 0) return;
    const long long E = n_edges;
    double pi[6], pj[6], yi[6], yj[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        pi[a] = b.p[6 * (long long)i + a];
        pj[a] = b.p[6 * (long long)j + a];
        yi[a] = yj[a] = 0.0;
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const double hij = b.hij[(6 * r + c) * E + e];
            yi[r] += hij * pj[c];
            yj[c] += hij * pi[r];
            if (c >= r) {
                const double hii = b.hii[tri(r, c) * E + e], hjj = b.hjj[tri(r, c) * E + e];
                yi[r] += hii * pi[c];
                yj[r] += hjj * pj[c];
                if (c > r) {
                    yi[c] += hii * pi[r];
                    yj[c] += hjj * pj[r];
                }
            }
        }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        b.ye[12 * (long long)e + a] = yi[a];
        b.ye[12 * (long long)e + 6 + a] = yj[a];
    }
}

// ---- nodes -------------------------------------------------------------------------------------------------------

// U^T U = M (upper triangle in place); false when a pivot is not positive and finite
__device__ __forceinline__ bool cholesky6(double U[21])
{
    bool ok = true;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double d = U[tri(r, r)];
#pragma unroll
        for (int k = 0; k < r; ++k) d -= U[tri(k, r)] * U[tri(k, r)];
        ok = ok && d > 0.0 && isfinite(d);
        d = sqrt(d);
        U[tri(r, r)] = d;
#pragma unroll
        for (int c = r + 1; c < 6; ++c) {
            double s = U[tri(r, c)];
#pragma unroll
            for (int k = 0; k < r; ++k) s -= U[tri(k, r)] * U[tri(k, c)];
            U[tri(r, c)] = s / d;
        }
    }
    return ok;
}

// z = (U^T U)^-1 r
__device__ __forceinline__ void cholesky_solve6(const double U[21], const double r[6], double z[6])
{
    double y[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double s = r[a];
#pragma unroll
        for (int k = 0; k < a; ++k) s -= U[tri(k, a)] * y[k];
        y[a] = s / U[tri(a, a)];
    }
#pragma unroll
    for (int a = 5; a >= 0; --a) {
        double s = y[a];
#pragma unroll
        for (int k = a + 1; k < 6; ++k) s -= U[tri(a, k)] * z[k];
        z[a] = s / U[tri(a, a)];
    }
}

// gather of g (written where g_out is given) and the diagonal blocks; with solve != 0 also the damped factor and the
// start of PCG: x = 0, r = -g, z = M^-1 r, p = z, partials of r.r and r.z
__global__ __launch_bounds__(TB) void pg_assemble_kernel(int n_poses, int n_edges, const uint8_t *__restrict__ fixed,
                                                         Buffers b, double *__restrict__ g_out,
                                                         double *__restrict__ blocks_out, int solve)
{
    if (solve && b.st->done) return;
    const int n = blockIdx.x * TB + threadIdx.x;
    const int nb = gridDim.x;
    double rr = 0.0, rz = 0.0;
    if (n < n_poses) {
        const long long E = n_edges;
        double g[6] = {0, 0, 0, 0, 0, 0}, D[21];
#pragma unroll
        for (int k = 0; k < 21; ++k) D[k] = 0.0;
        const int lo = b.row_ptr[n], hi = b.row_ptr[n + 1];
        for (int a = lo; a < hi; ++a) {
            const int code = b.list[a], e = code >> 1, side = code & 1;
            const double *h = side ? b.hjj : b.hii;
#pragma unroll
            for (int k = 0; k < 6; ++k) g[k] += b.ge[12 * (long long)e + 6 * side + k];
#pragma unroll
            for (int k = 0; k < 21; ++k) D[k] += h[k * E + e];
        }
        if (g_out)
            for (int k = 0; k < 6; ++k) g_out[6 * (long long)n + k] = g[k];
        for (int k = 0; k < 21; ++k) blocks_out[21 * (long long)n + k] = D[k];
        if (solve) {
            const double lambda = b.st->lambda;
            double U[21], r[6], z[6];
#pragma unroll
            for (int k = 0; k < 21; ++k) U[k] = D[k];
#pragma unroll
            for (int k = 0; k < 6; ++k) U[tri(k, k)] += lambda * D[tri(k, k)];
            bool free_n = !fixed[n] && hi > lo;
            free_n = cholesky6(U) && free_n;
            b.free_node[n] = free_n;
#pragma unroll
            for (int k = 0; k < 6; ++k) r[k] = free_n ? -g[k] : 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) z[k] = 0.0;
            if (free_n) cholesky_solve6(U, r, z);
            for (int k = 0; k < 21; ++k) b.chol[21 * (long long)n + k] = U[k];
            for (int k = 0; k < 6; ++k) {
                const long long at = 6 * (long long)n + k;
                b.x[at] = 0.0;
                b.r[at] = r[k];
                b.z[at] = z[k];
                b.p[at] = z[k];
                b.ap[at] = 0.0;
                rr += r[k] * r[k];
                rz += r[k] * z[k];
            }
        }
    }
    if (solve) {
        write_partial(b.part_b, rr);
        write_partial(b.part_b + nb, rz);
    }
}

// one wave: |g|^2 and r.z of the start; no inner iteration when the gradient is zero.  part: the nb partials of r.r, then
// those of r.z, one per workgroup of nodes (part_b) or, behind the prolong kernel, one per aggregate
__global__ __launch_bounds__(TB) void pg_pcg_begin_kernel(Buffers b, const double *part, int nb)
{
    if (b.st->done) return;
    const double bb = finish(part, nb), rz = finish(part + nb, nb);
    if (threadIdx.x == 0) {
        b.st->bb = bb;
        b.st->rz[0] = rz;
        b.st->stop_k = bb > 0.0 && rz > 0.0 ? INT_MAX : 0;
    }
}

// A p = gather + lambda diag(H) p on the free nodes; partial of p.Ap
__global__ __launch_bounds__(TB) void pg_node_matvec_kernel(int n_poses, Buffers b, int k)
{
    if (b.st->done || k >= b.st->stop_k) return;
    const int n = blockIdx.x * TB + threadIdx.x;
    double pap = 0.0;
    if (n < n_poses && b.free_node[n]) {
        const double lambda = b.st->lambda;
        double y[6] = {0, 0, 0, 0, 0, 0};
        const int lo = b.row_ptr[n], hi = b.row_ptr[n + 1];
        for (int a = lo; a < hi; ++a) {
            const int code = b.list[a], e = code >> 1, side = code & 1;
#pragma unroll
            for (int c = 0; c < 6; ++c) y[c] += b.ye[12 * (long long)e + 6 * side + c];
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const long long at = 6 * (long long)n + c;
            const double p = b.p[at];
            y[c] += lambda * b.blocks[21 * (long long)n + tri(c, c)] * p;
            b.ap[at] = y[c];
            pap += p * y[c];
        }
    }
    write_partial(b.part_a, pap);
}

// the PCG step on free node n: x += alpha p;  r -= alpha A p;  z = B^-1 r
__device__ __forceinline__ void pcg_step_node(const Buffers &b, int n, double alpha, double r[6], double z[6])
{
    double U[21];
    for (int c = 0; c < 21; ++c) U[c] = b.chol[21 * (long long)n + c];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const long long at = 6 * (long long)n + c;
        b.x[at] += alpha * b.p[at];
        r[c] = b.r[at] - alpha * b.ap[at];
        b.r[at] = r[c];
    }
    cholesky_solve6(U, r, z);
#pragma unroll
    for (int c = 0; c < 6; ++c) b.z[6 * (long long)n + c] = z[c];
}

// alpha = r.z / p.Ap;  the step;  partials of r.r and r.z
__global__ __launch_bounds__(TB) void pg_pcg_step_kernel(int n_poses, Buffers b, int k)
{
    if (b.st->done || k >= b.st->stop_k) return;
    const int nb = gridDim.x;
    const double pap = finish(b.part_a, nb);
    const double alpha = pap > 0.0 ? b.st->rz[k & 1] / pap : 0.0;
    const int n = blockIdx.x * TB + threadIdx.x;
    double rr = 0.0, rz = 0.0;
    if (n < n_poses && b.free_node[n]) {
        double r[6], z[6];
        pcg_step_node(b, n, alpha, r, z);
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            rr += r[c] * r[c];
            rz += r[c] * z[c];
        }
    }
    write_partial(b.part_b, rr);
    write_partial(b.part_b + nb, rz);
}

// beta = r.z (new) / r.z (old);  p = z + beta p;  the first lane of the grid counts the iteration and ends the loop at
// |r| <= tolerance |g|, at p.Ap <= 0 or at r.z <= 0.  part, nb: as in pg_pcg_begin_kernel
__global__ __launch_bounds__(TB) void pg_pcg_direction_kernel(int n_poses, Buffers b, int k, double tol2,
                                                              const double *part, int nb)
{
    if (b.st->done || k >= b.st->stop_k) return;
    // finish() of p.Ap, r.r and r.z, bit for bit, in one pass: the loads of the three sums are in flight together
    double pap = 0.0, rr = 0.0, rz = 0.0;
    const int na = gridDim.x;
    for (int i = threadIdx.x; i < max(na, nb); i += TB) {
        if (i < na) pap += b.part_a[i];
        if (i < nb) {
            rr += part[i];
            rz += part[nb + i];
        }
    }
    pap = nsc_wave_sum(pap);
    rr = nsc_wave_sum(rr);
    rz = nsc_wave_sum(rz);
    const double beta = rz / b.st->rz[k & 1];
    const int n = blockIdx.x * TB + threadIdx.x;
    if (n < n_poses && b.free_node[n]) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const long long at = 6 * (long long)n + c;
            b.p[at] = b.z[at] + beta * b.p[at];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        b.st->rz[(k + 1) & 1] = rz;
        b.st->pcg_total += 1;
        if (!(pap > 0.0) || rr <= tol2 * b.st->bb || !(rz > 0.0)) b.st->stop_k = k + 1;
    }
}

// ---- the coarse space ----------------------------------------------------------------------------------------------

constexpr int CB = 512;                      // lanes of the one workgroup that factors A_c: two waves per SIMD, 256 VGPRs
constexpr int CW = CB / TB;                  // its waves
constexpr int CR = 4;                        // rows a wave loads before it stores any
constexpr int CM = 6 * NSC_POSEGRAPH_MAX_AGGREGATES / TB;   // entries of a coarse vector per lane: 12

__device__ __forceinline__ void load36(const double *__restrict__ src, double M[36])
{
#pragma unroll
    for (int q = 0; q < 36; ++q) M[q] = src[q];
}

// acc += Tk^T H Tm, row of H by row
__device__ __forceinline__ void add_tht(const double Tk[36], const double H[36], const double Tm[36], double acc[36])
{
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double row[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 6; ++q) s += H[6 * r + q] * Tm[6 * q + c];
            row[c] = s;
        }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int c = 0; c < 6; ++c) acc[6 * i + c] += Tk[6 * r + i] * row[c];
    }
}

// P: the block of node k is Ad(X_k^-1 X_ref) = [[R, 0], [[t]x R, R]] with R = R_k^T R_ref, t = R_k^T (t_ref - t_k), X_ref
// the first pose of k's aggregate at the linearisation point; zeros for a node that is not free
__global__ __launch_bounds__(TB) void pg_coarse_basis_kernel(const double *poses, int n_poses, Buffers b, Coarse c)
{
    if (b.st->done) return;
    const int n = blockIdx.x * TB + threadIdx.x;
    if (n >= n_poses) return;
    double T[36];
#pragma unroll
    for (int q = 0; q < 36; ++q) T[q] = 0.0;
    if (b.free_node[n]) {
        double Rk[9], tk[3], Rf[9], tf[3], R[9], t[3], K[9];
        load_pose(poses, n, Rk, tk);
        load_pose(poses, (long long)(n / c.L) * c.L, Rf, tf);
        mul_tn(Rk, Rf, R);
        const double d[3] = {tf[0] - tk[0], tf[1] - tk[1], tf[2] - tk[2]};
        mulv_t(Rk, d, t);
        hat(t, K);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                T[6 * r + q] = T[6 * (r + 3) + q + 3] = R[3 * r + q];
                T[6 * (r + 3) + q] = K[3 * r] * R[q] + K[3 * r + 1] * R[3 + q] + K[3 * r + 2] * R[6 + q];
            }
    }
    for (int q = 0; q < 36; ++q) c.t[36 * (long long)n + q] = T[q];
}

// A_c = P^T (H + lambda diag H) P over the free nodes: one wave per block (a, b), a <= b.  Lane l takes the nodes
// a L + l, a L + l + 64, ... of aggregate a, each with its diagonal block (a == b) and its incident edges whose other end
// is a free node of aggregate b, in list order; the wave finishes with the butterfly and writes the block and, for
// a < b, its transpose, so every entry of A_c is written.  An aggregate without a free node gets the identity.
__global__ __launch_bounds__(TB) void pg_coarse_galerkin_kernel(int n_poses, int n_edges, Buffers b, Coarse c)
{
    if (b.st->done) return;
    const int ca = blockIdx.x / c.n_agg, cb = blockIdx.x % c.n_agg;
    if (ca > cb) return;
    const long long E = n_edges;
    const double lambda = b.st->lambda;
    double acc[36];
#pragma unroll
    for (int q = 0; q < 36; ++q) acc[q] = 0.0;
    int n_free = 0;
    const int lo = ca * c.L, hi = min(lo + c.L, n_poses);
    for (int n = lo + threadIdx.x; n < hi; n += TB) {
        if (!b.free_node[n]) continue;
        ++n_free;
        double Tk[36], Tm[36], H[36];
        load36(c.t + 36 * (long long)n, Tk);
        if (ca == cb) {
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int q = r; q < 6; ++q) {
                    const double v = b.blocks[21 * (long long)n + tri(r, q)];
                    H[6 * r + q] = H[6 * q + r] = r == q ? v + lambda * v : v;
                }
            add_tht(Tk, H, Tk, acc);
        }
        for (int a = b.row_ptr[n]; a < b.row_ptr[n + 1]; ++a) {
            const int code = b.list[a], e = code >> 1, side = code & 1;
            const int m = side ? b.ei[e] : b.ej[e];
            if (!b.free_node[m] || m / c.L != cb) continue;
            load36(c.t + 36 * (long long)m, Tm);
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int q = 0; q < 6; ++q) H[6 * r + q] = b.hij[(side ? 6 * q + r : 6 * r + q) * E + e];
            add_tht(Tk, H, Tm, acc);
        }
    }
    n_free = nsc_wave_sum(n_free);
#pragma unroll
    for (int q = 0; q < 36; ++q) acc[q] = nsc_wave_sum(acc[q]);
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double v = ca == cb && n_free == 0 ? (r == q ? 1.0 : 0.0) : acc[6 * r + q];
            c.ac[(6LL * ca + r) * c.nc + 6 * cb + q] = v;
            if (ca != cb) c.ac[(6LL * cb + q) * c.nc + 6 * ca + r] = v;
        }
}

// U^T U = A_c by one workgroup, in global memory (768^2 doubles do not fit the LDS), reading the upper triangle only.
// Right-looking, one barrier per column: at column j the rows below it lose (A_jr / A_jj) A_j., row j stays unscaled
// until the end, where U_j. = A_j. / sqrt(A_jj) is written over A_c and, transposed, into lt.  Lane l of every wave
// holds columns j + 1 + l, + 64, ... of the pivot row in registers; a wave takes four rows at a time and loads all
// before it stores any.  A pivot that is not positive and finite ends the factor: ok = 0, and the event is counted.
__global__ __launch_bounds__(CB) void pg_coarse_factor_kernel(Buffers b, Coarse c)
{
    if (b.st->done) return;
    const int n = c.nc, wave = threadIdx.x / TB, lane = threadIdx.x % TB;
    double *A = c.ac;
    bool ok = true;
    for (int j = 0; j < n; ++j) {
        const double *Aj = A + (long long)j * n;
        const double piv = Aj[j];                            // final since the barrier of column j - 1: the same in every lane
        if (!(piv > 0.0) || !isfinite(piv)) {
            ok = false;
            break;
        }
        const double inv = 1.0 / piv;
        double rowj[CM];
#pragma unroll
        for (int m = 0; m < CM; ++m) {
            const int col = j + 1 + lane + TB * m;
            rowj[m] = col < n ? Aj[col] : 0.0;
        }
        for (int r0 = j + 1 + CR * wave; r0 < n; r0 += CR * CW) {
            double f[CR], v[CR][CM];
#pragma unroll
            for (int q = 0; q < CR; ++q) {
                const int r = r0 + q;
                f[q] = r < n ? Aj[r] * inv : 0.0;
#pragma unroll
                for (int m = 0; m < CM; ++m) {
                    const int col = j + 1 + lane + TB * m;
                    v[q][m] = r < n && col >= r && col < n ? A[r * n + col] : 0.0;        // nc^2 < 2^31
                }
            }
#pragma unroll
            for (int q = 0; q < CR; ++q) {
                const int r = r0 + q;
#pragma unroll
                for (int m = 0; m < CM; ++m) {
                    const int col = j + 1 + lane + TB * m;
                    if (r < n && col >= r && col < n) A[r * n + col] = v[q][m] - f[q] * rowj[m];
                }
            }
        }
        __syncthreads();
    }
    if (ok) {
        for (int j = wave; j < n; j += CW) {
            const double d = 1.0 / sqrt(A[(long long)j * n + j]);
            for (int col = j + lane; col < n; col += TB) {
                const double u = A[(long long)j * n + col] * d;
                A[(long long)j * n + col] = u;
                c.lt[(long long)col * n + j] = u;
            }
        }
    }
    if (threadIdx.x == 0) {
        c.cs->ok = ok;
        if (!ok) c.cs->failed += 1;
    }
}

// A_c^-1, one column per wave: U^T y = e_col, then U x = y, both in axpy form so that every read is a contiguous row (of
// U, then of U^T).  Lane l holds entries l, l + 64, ... of the running column.
__global__ __launch_bounds__(TB) void pg_coarse_invert_kernel(Buffers b, Coarse c)
{
    if (b.st->done || !c.cs->ok) return;
    const int n = c.nc, col = blockIdx.x, lane = threadIdx.x;
    double v[CM];
#pragma unroll
    for (int m = 0; m < CM; ++m) v[m] = lane + TB * m == col ? 1.0 : 0.0;
#pragma unroll
    for (int mk = 0; mk < CM; ++mk)
        for (int kk = 0; kk < TB; ++kk) {
            const int k = TB * mk + kk;
            if (k < col || k >= n) continue;                 // y is zero above the column's own row
            const double *Uk = c.ac + (long long)k * n;
            const double yk = __shfl(v[mk], kk, 64) / Uk[k];
            if (lane == kk) v[mk] = yk;
#pragma unroll
            for (int m = mk; m < CM; ++m) {
                const int i = lane + TB * m;
                if (i > k && i < n) v[m] -= Uk[i] * yk;
            }
        }
#pragma unroll
    for (int mk = CM - 1; mk >= 0; --mk)
        for (int kk = TB - 1; kk >= 0; --kk) {
            const int k = TB * mk + kk;
            if (k >= n) continue;
            const double *Lk = c.lt + (long long)k * n;      // row k of U^T: column k of U
            const double xk = __shfl(v[mk], kk, 64) / Lk[k];
            if (lane == kk) v[mk] = xk;
#pragma unroll
            for (int m = 0; m <= mk; ++m) {
                const int i = lane + TB * m;
                if (i < k) v[m] -= Lk[i] * xk;
            }
        }
#pragma unroll
    for (int m = 0; m < CM; ++m) {
        const int i = lane + TB * m;
        if (i < n) c.ainv[(long long)i * n + col] = v[m];    // A_c^-1 is symmetric: row i of column col
    }
}

// One wave per aggregate.  k >= 0: the step of inner iteration k on the aggregate's free nodes, alpha = r.z / p.Ap;
// x += alpha p;  r -= alpha A p;  z = B^-1 r.  k < 0: the start, r and z as pg_assemble_kernel left them.  Either way
// the aggregate's six entries of r_c = P^T r, each lane summing its nodes in ascending order.
__global__ __launch_bounds__(TB) void pg_coarse_restrict_kernel(int n_poses, int nb_a, Buffers b, Coarse c, int k)
{
    if (b.st->done || k >= b.st->stop_k) return;
    double alpha = 0.0;
    if (k >= 0) {
        const double pap = finish(b.part_a, nb_a);
        alpha = pap > 0.0 ? b.st->rz[k & 1] / pap : 0.0;
    }
    double rc[6] = {0, 0, 0, 0, 0, 0};
    const int lo = blockIdx.x * c.L, hi = min(lo + c.L, n_poses);
    for (int n = lo + threadIdx.x; n < hi; n += TB) {
        if (!b.free_node[n]) continue;
        double r[6];
        if (k >= 0) {
            double z[6];
            pcg_step_node(b, n, alpha, r, z);
        } else {
#pragma unroll
            for (int q = 0; q < 6; ++q) r[q] = b.r[6 * (long long)n + q];
        }
        const double *T = c.t + 36 * (long long)n;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int q = 0; q < 6; ++q) rc[q] += T[6 * i + q] * r[i];
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) rc[q] = nsc_wave_sum(rc[q]);
    if (threadIdx.x == 0)
        for (int q = 0; q < 6; ++q) c.rc[6 * blockIdx.x + q] = rc[q];
}

// One wave per aggregate: its six rows of y = A_c^-1 r_c (none when the factor failed: B^-1 alone), z += P y on its free
// nodes, p = z at the start (k < 0), and the aggregate's partials of r.r and r.z
__global__ __launch_bounds__(TB) void pg_coarse_prolong_kernel(int n_poses, Buffers b, Coarse c, int k)
{
    if (b.st->done || k >= b.st->stop_k) return;
    const bool coarse = c.cs->ok;
    double y[6] = {0, 0, 0, 0, 0, 0};
    if (coarse) {
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double *row = c.ainv + (6LL * blockIdx.x + q) * c.nc;
            double s = 0.0;
            for (int i = threadIdx.x; i < c.nc; i += TB) s += row[i] * c.rc[i];
            y[q] = nsc_wave_sum(s);
        }
    }
    double rr = 0.0, rz = 0.0;
    const int lo = blockIdx.x * c.L, hi = min(lo + c.L, n_poses);
    for (int n = lo + threadIdx.x; n < hi; n += TB) {
        if (!b.free_node[n]) continue;
        const double *T = c.t + 36 * (long long)n;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const long long at = 6 * (long long)n + i;
            double z = b.z[at];
            if (coarse) {
                double s = 0.0;
#pragma unroll
                for (int q = 0; q < 6; ++q) s += T[6 * i + q] * y[q];
                z += s;
                b.z[at] = z;
            }
            if (k < 0) b.p[at] = z;
            const double r = b.r[at];
            rr += r * r;
            rz += r * z;
        }
    }
    write_partial(c.part, rr);
    write_partial(c.part + c.n_agg, rz);
}

// candidate poses X_k [Exp(phi_k) | rho_k]; partial of |delta|^2; the first delta of the call on request
__global__ __launch_bounds__(TB) void pg_update_kernel(const double *poses, int n_poses, Buffers b, int it,
                                                       double *__restrict__ step0)
{
    if (b.st->done) return;
    const int n = blockIdx.x * TB + threadIdx.x;
    double s2 = 0.0;
    if (n < n_poses) {
        double d[6];
        for (int c = 0; c < 6; ++c) {
            d[c] = b.x[6 * (long long)n + c];
            s2 += d[c] * d[c];
            if (it == 0 && step0) step0[6 * (long long)n + c] = d[c];
        }
        double R[9], t[3], Q[9];
        load_pose(poses, n, R, t);
        double *out = b.cand + 16 * (long long)n;
        if (b.free_node[n]) {
            exp_so3(d, Q);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) out[4 * r + c] = R[3 * r] * Q[c] + R[3 * r + 1] * Q[3 + c] + R[3 * r + 2] * Q[6 + c];
                out[4 * r + 3] = t[r] + (R[3 * r] * d[3] + R[3 * r + 1] * d[4] + R[3 * r + 2] * d[5]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) out[4 * r + c] = R[3 * r + c];
                out[4 * r + 3] = t[r];
            }
        }
    }
    write_partial(b.part_s, s2);
}

// one wave: the cost at the start
__global__ __launch_bounds__(TB) void pg_init_kernel(int nb_n, Buffers b, double lambda0, double *__restrict__ history,
                                                     PgCoarse *__restrict__ cs)
{
    const double f = finish(b.part_e, nb_n);
    if (threadIdx.x == 0) {
        if (cs) cs->ok = cs->failed = 0;
        b.st->cost = b.st->cost0 = f;
        b.st->lambda = lambda0;
        b.st->accept_it = -1;
        b.st->stop_k = 0;
        history[0] = f;
    }
}

// one wave: accept or reject the candidate, move lambda, test the stopping rules
__global__ __launch_bounds__(TB) void pg_accept_kernel(int nb_n, Buffers b, NscPoseGraphParams prm, int it,
                                                       double *__restrict__ history)
{
    if (b.st->done) return;
    const double fc = finish(b.part_e, nb_n), step = sqrt(finish(b.part_s, nb_n));
    if (threadIdx.x != 0) return;
    PgState *st = b.st;
    const double f = st->cost;
    bool stop = false;
    st->iterations += 1;
    st->step = step;
    if (fc < f) {
        st->accepted += 1;
        st->accept_it = it;
        stop = (f - fc) < prm.relative_cost * f;
        st->cost = fc;
        st->lambda = fmax(st->lambda / prm.lambda_factor, prm.lambda_min);
    } else {
        st->rejected += 1;
        st->lambda = st->lambda * prm.lambda_factor;
    }
    history[it + 1] = st->cost;
    if (stop || step < prm.min_step) {
        st->done = 1;
        st->converged = 1;
    }
}

// the accepted candidate becomes the pose of every free node
__global__ __launch_bounds__(TB) void pg_commit_kernel(double *poses, int n_poses, Buffers b, int it)
{
    if (b.st->accept_it != it) return;
    const int n = blockIdx.x * TB + threadIdx.x;
    if (n >= n_poses || !b.free_node[n]) return;
#pragma unroll
    for (int k = 0; k < 12; ++k) poses[16 * (long long)n + k] = b.cand[16 * (long long)n + k];
}

__global__ __launch_bounds__(TB) void pg_finalize_kernel(Buffers b, int max_iteration, double *__restrict__ stats,
                                                         double *__restrict__ history, const PgCoarse *__restrict__ cs,
                                                         int n_agg, double *__restrict__ coarse_stats)
{
    const PgState *st = b.st;
    for (int k = st->iterations + 1 + threadIdx.x; k <= max_iteration; k += TB) history[k] = st->cost;
    if (threadIdx.x != 0) return;
    if (coarse_stats) {
        coarse_stats[0] = n_agg;
        coarse_stats[1] = cs ? cs->failed : 0;
    }
    stats[NSC_POSEGRAPH_STAT_ITERATIONS] = st->iterations;
    stats[NSC_POSEGRAPH_STAT_ACCEPTED] = st->accepted;
    stats[NSC_POSEGRAPH_STAT_REJECTED] = st->rejected;
    stats[NSC_POSEGRAPH_STAT_PCG_ITERATIONS] = st->pcg_total;
    stats[NSC_POSEGRAPH_STAT_INITIAL_COST] = st->cost0;
    stats[NSC_POSEGRAPH_STAT_FINAL_COST] = st->cost;
    stats[NSC_POSEGRAPH_STAT_LAMBDA] = st->lambda;
    stats[NSC_POSEGRAPH_STAT_SKIPPED] = st->skipped;
    stats[NSC_POSEGRAPH_STAT_CONVERGED] = st->converged;
    stats[NSC_POSEGRAPH_STAT_STEP] = st->step;
}

// one wave: the outputs of nsc_posegraph_linearize that are scalars
__global__ __launch_bounds__(TB) void pg_linearize_out_kernel(int nb_n, Buffers b, double *__restrict__ cost,
                                                              long long *__restrict__ skipped)
{
    const double f = finish(b.part_e, nb_n);
    if (threadIdx.x == 0) {
        *cost = f;
        *skipped = b.st->skipped;
    }
}

// ---- marginal covariances: PCG on many right-hand sides ----------------------------------------------------------------
//
// nsc_posegraph_covariance solves H x = e for the R = 6 Q unit vectors of the selected poses, each an independent PCG.
// One lane per right-hand side: the vectors x, r, z, p, A p are (N, 6, R_pad) with the right-hand side fastest, R_pad = R
// rounded up to 64, and a workgroup owns a tile of CT consecutive nodes (an aggregate in the two coarse kernels) times one
// chunk of 64 right-hand sides.  Its VW waves all work on the same 64 columns and share the tile's nodes, wave w taking
// nodes w, w + VW, ...: with one wave a tile (measured on the 4 541-pose graph) every kernel was a chain of dependent trips
// to memory, 100 to 140 us each, whatever the number of columns.  The node, its incident list and therefore every address
// of hii / hjj / hij, chol, P and A_c^-1 are the same in all 64 lanes (scalar or broadcast loads); every vector load is 64
// consecutive doubles.  Every dot product stays in its lane: a wave sums its nodes in ascending order, the first wave the VW
// sums through the LDS in ascending order, and a scalar is one partial per (tile, right-hand side), or per (aggregate,
// right-hand side) behind the prolong kernel; a consumer sums the partials of its column in the fixed order of
// column_sum().  No cross-lane reduction, no floating-point atomics.  So a column's bits do not depend on which lane or
// chunk it sits in, nor on what the other columns are.  Column state (r.z in two slots, b.b, r.r, stop_k, iterations) lives in
// arrays of R_pad; the wave of tile 0 writes it in the direction kernel, with the stop_k and two-slot rules of the
// optimiser's loop.  A lane whose column has stopped stores nothing; a wave all of whose columns have stopped returns.

constexpr int CT = NSC_POSEGRAPH_COV_TILE;   // nodes per wave
constexpr int VW = 8;                       // waves of a workgroup of the two coarse kernels: they share an aggregate's nodes
constexpr int VB = VW * TB;

struct Cov {                                 // the covariance call's part of the workspace, behind Buffers' and Coarse's
    double *x, *r, *z, *p, *ap;              // (N,6,R_pad)
    double *part_a, *part_rr, *part_rz;      // (max(tiles, aggregates), R_pad): p.Ap per tile; r.r and r.z per tile or aggregate
    double *rc;                              // (nc, R_pad): P^T r
    double *hp;                              // (E,78): the blocks of every edge, edge by edge
    double *rz, *bb, *rr;                    // (2,R_pad), (R_pad), (R_pad)
    int *stop_k, *iters;                     // (R_pad)
    int R, R_pad, n_tiles;
};

__device__ __forceinline__ size_t cov_at(int n, int c, int Rp, int col) { return ((size_t)n * 6 + c) * Rp + col; }

// The sums of K lane-local values over the VW waves, in ascending wave order.  ALL: every wave gets them; otherwise wave 0
// alone, and the other waves keep what they had.  red: K VW rows of the workgroup's LDS, value q of wave w in row VW q + w.
template <int K, bool ALL> __device__ __forceinline__ void wave_sums(double (&v)[K], double (*red)[TB])
{
    const int wave = threadIdx.x / TB, lane = threadIdx.x % TB;
    __syncthreads();                                         // whoever still reads red from an earlier sum has finished
#pragma unroll
    for (int q = 0; q < K; ++q) red[VW * q + wave][lane] = v[q];
    __syncthreads();
    if (!ALL && wave != 0) return;
#pragma unroll
    for (int q = 0; q < K; ++q) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < VW; ++w) s += red[VW * q + w][lane];
        v[q] = s;
    }
}

// The nb partials of one column, for all VW waves of a workgroup at once (they share their 64 columns), the same bits in
// every wave of every workgroup of every kernel: wave w sums partials w, w + VW, ... in ascending order (four loads in
// flight), then every wave sums the VW results in ascending order.  red: VW rows of the workgroup's LDS.
__device__ __forceinline__ double column_sum(const double *part, int nb, int Rp, int col, double (*red)[TB])
{
    double s[1] = {0.0};
    int t = threadIdx.x / TB;
    for (; t + 3 * VW < nb; t += 4 * VW) {
        const double a0 = part[(size_t)t * Rp + col], a1 = part[(size_t)(t + VW) * Rp + col],
                     a2 = part[(size_t)(t + 2 * VW) * Rp + col], a3 = part[(size_t)(t + 3 * VW) * Rp + col];
        s[0] += a0;
        s[0] += a1;
        s[0] += a2;
        s[0] += a3;
    }
    for (; t < nb; t += VW) s[0] += part[(size_t)t * Rp + col];
    wave_sums<1, true>(s, red);
    return s[0];
}

// x = 0, r = e (column 6 q + c is the unit vector of entry c of pose nodes[q]; zero when that index is out of range or
// the pose is not free, and in the padding), z = B^-1 r, p = z, A p = 0; partials of r.r and r.z per tile
__global__ __launch_bounds__(VB) void pg_cov_init_kernel(int n_poses, const long long *__restrict__ nodes, Buffers b, Cov v)
{
    __shared__ double red[2 * VW][TB];
    const int wave = threadIdx.x / TB, col = blockIdx.y * TB + threadIdx.x % TB, Rp = v.R_pad;
    long long node = -1;
    if (col < v.R) {
        node = nodes[col / 6];
        if (node < 0 || node >= n_poses || !b.free_node[node]) node = -1;
    }
    const int comp = col % 6;
    double d[2] = {0.0, 0.0};                                // r.r, r.z
    const int lo = blockIdx.x * CT, hi = min(lo + CT, n_poses);
    for (int n = lo + wave; n < hi; n += VW) {
        double r[6], z[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 6; ++c) r[c] = node == n && comp == c ? 1.0 : 0.0;
        if (b.free_node[n]) {
            double U[21];
            for (int q = 0; q < 21; ++q) U[q] = b.chol[21 * (long long)n + q];
            cholesky_solve6(U, r, z);
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const size_t at = cov_at(n, c, Rp, col);
            v.x[at] = 0.0;
            v.r[at] = r[c];
            v.z[at] = z[c];
            v.p[at] = z[c];
            v.ap[at] = 0.0;
            d[0] += r[c] * r[c];
            d[1] += r[c] * z[c];
        }
    }
    wave_sums<2, false>(d, red);
    if (wave != 0) return;
    v.part_rr[(size_t)blockIdx.x * Rp + col] = d[0];
    v.part_rz[(size_t)blockIdx.x * Rp + col] = d[1];
    // the matvec kernel writes p.Ap for the columns that run; a column that never runs has its alpha formed all the same
    // (cov_alpha) and dropped: it sums zeros then, not what the caller's workspace happened to hold
    v.part_a[(size_t)blockIdx.x * Rp + col] = 0.0;
}

// one workgroup per chunk: b.b and r.z of the start from nb partials; a column with b = 0 runs no iteration
__global__ __launch_bounds__(VB) void pg_cov_begin_kernel(int nb, Cov v)
{
    __shared__ double red[VW][TB];
    const int col = blockIdx.x * TB + threadIdx.x % TB, Rp = v.R_pad;
    const double bb = column_sum(v.part_rr, nb, Rp, col, red), rz = column_sum(v.part_rz, nb, Rp, col, red);
    if (threadIdx.x >= TB) return;
    v.bb[col] = bb;
    v.rr[col] = bb;
    v.rz[col] = rz;
    v.rz[Rp + col] = 0.0;
    v.iters[col] = 0;
    v.stop_k[col] = bb > 0.0 && rz > 0.0 ? INT_MAX : 0;
}

// The blocks of every counted edge once more, edge by edge: hp (E,78) = [H_ii (21), H_jj (21), H_ij (36)].  The
// linearisation keeps them structure-of-arrays for one lane per edge; read by a whole wave for ONE edge that layout is 57
// cache lines a side (measured: 87 us a matvec on the 4 541-pose graph).  One lane per edge, once per call.
__global__ __launch_bounds__(TB) void pg_cov_pack_kernel(int n_edges, Buffers b, double *__restrict__ hp)
{
    const int e = blockIdx.x * TB + threadIdx.x;
    if (e >= n_edges || b.ei[e] < 0) return;
    const long long E = n_edges;
    double *out = hp + 78LL * e;
    for (int q = 0; q < 21; ++q) {
        out[q] = b.hii[q * E + e];
        out[21 + q] = b.hjj[q * E + e];
    }
    for (int q = 0; q < 36; ++q) out[42 + q] = b.hij[q * E + e];
}

// A p on the free nodes of the tile, gathered on the node side: for every incident (edge, side) H_ss p_n + H_st p_other,
// straight from the packed edge blocks; partial of p.Ap
__global__ __launch_bounds__(VB) void pg_cov_matvec_kernel(int n_poses, const int *__restrict__ row_ptr,
                                                           const int *__restrict__ list, const int *__restrict__ ei,
                                                           const int *__restrict__ ej, const int *__restrict__ free_node,
                                                           const double *__restrict__ hp, Cov v, int k)
{
    __shared__ double red[VW][TB];
    const int wave = threadIdx.x / TB, col = blockIdx.y * TB + threadIdx.x % TB, Rp = v.R_pad;
    const bool active = k < v.stop_k[col];
    if (!__any(active)) return;                              // the same columns in every wave: the workgroup leaves as one
    const double *__restrict__ P = v.p;
    double pap[1] = {0.0};
    const int lo = blockIdx.x * CT, hi = min(lo + CT, n_poses);
    for (int n = lo + wave; n < hi; n += VW) {
        if (!free_node[n]) continue;
        double pn[6], y[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 6; ++c) pn[c] = P[cov_at(n, c, Rp, col)];
        for (int a = row_ptr[n]; a < row_ptr[n + 1]; ++a) {
            const int code = list[a], e = code >> 1, side = code & 1;
            const int m = side ? ei[e] : ej[e];
            const double *__restrict__ hs = hp + 78LL * e + (side ? 21 : 0), *__restrict__ hx = hp + 78LL * e + 42;
            double pm[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) pm[c] = P[cov_at(m, c, Rp, col)];
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    // side 0: this node is i, y_i += H_ij p_j;  side 1: this node is j, y_j += H_ij^T p_i
                    y[r] += hx[side ? 6 * c + r : 6 * r + c] * pm[c];
                    if (c >= r) {
                        const double h = hs[tri(r, c)];
                        y[r] += h * pn[c];
                        if (c > r) y[c] += h * pn[r];
                    }
                }
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            if (active) v.ap[cov_at(n, c, Rp, col)] = y[c];
            pap[0] += pn[c] * y[c];
        }
    }
    wave_sums<1, false>(pap, red);
    if (wave == 0 && active) v.part_a[(size_t)blockIdx.x * Rp + col] = pap[0];
}

// alpha = r.z / p.Ap;  x += alpha p;  r -= alpha A p;  z = B^-1 r on node n, one column per lane; adds to r.r and r.z
__device__ __forceinline__ void cov_step_node(const Buffers &b, const Cov &v, int n, int col, double alpha, bool active,
                                              double r[6], double z[6])
{
    const int Rp = v.R_pad;
    double U[21];
    for (int q = 0; q < 21; ++q) U[q] = b.chol[21 * (long long)n + q];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const size_t at = cov_at(n, c, Rp, col);
        const double x = v.x[at] + alpha * v.p[at];
        r[c] = v.r[at] - alpha * v.ap[at];
        if (active) {
            v.x[at] = x;
            v.r[at] = r[c];
        }
    }
    cholesky_solve6(U, r, z);
    if (active) {
#pragma unroll
        for (int c = 0; c < 6; ++c) v.z[cov_at(n, c, Rp, col)] = z[c];
    }
}

__device__ __forceinline__ double cov_alpha(const Cov &v, int k, int col, double (*red)[TB])
{
    const double pap = column_sum(v.part_a, v.n_tiles, v.R_pad, col, red);
    return pap > 0.0 ? v.rz[(k & 1) * v.R_pad + col] / pap : 0.0;
}

// the step on the free nodes of the tile; partials of r.r and r.z
__global__ __launch_bounds__(VB) void pg_cov_step_kernel(int n_poses, Buffers b, Cov v, int k)
{
    __shared__ double red[2 * VW][TB];
    const int wave = threadIdx.x / TB, col = blockIdx.y * TB + threadIdx.x % TB, Rp = v.R_pad;
    const bool active = k < v.stop_k[col];
    if (!__any(active)) return;                              // the same columns in every wave: the workgroup leaves as one
    const double alpha = cov_alpha(v, k, col, red);
    double d[2] = {0.0, 0.0};                                // r.r, r.z
    const int lo = blockIdx.x * CT, hi = min(lo + CT, n_poses);
    for (int n = lo + wave; n < hi; n += VW) {
        if (!b.free_node[n]) continue;
        double r[6], z[6];
        cov_step_node(b, v, n, col, alpha, active, r, z);
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            d[0] += r[c] * r[c];
            d[1] += r[c] * z[c];
        }
    }
    wave_sums<2, false>(d, red);
    if (wave == 0 && active) {
        v.part_rr[(size_t)blockIdx.x * Rp + col] = d[0];
        v.part_rz[(size_t)blockIdx.x * Rp + col] = d[1];
    }
}

// beta = r.z (new) / r.z (old);  p = z + beta p on the tile; the first wave of tile 0 counts the iteration of its columns, keeps
// r.r and ends a column at r.r <= tol^2 b.b, at p.Ap <= 0 or at r.z <= 0.  nb_b partials of r.r and of r.z
__global__ __launch_bounds__(VB) void pg_cov_direction_kernel(int n_poses, Buffers b, Cov v, int k, double tol2, int nb_b)
{
    __shared__ double red[VW][TB];
    const int wave = threadIdx.x / TB, col = blockIdx.y * TB + threadIdx.x % TB, Rp = v.R_pad;
    const bool active = k < v.stop_k[col];
    if (!__any(active)) return;                              // the same columns in every wave: the workgroup leaves as one
    const double pap = column_sum(v.part_a, v.n_tiles, Rp, col, red), rr = column_sum(v.part_rr, nb_b, Rp, col, red),
                 rz = column_sum(v.part_rz, nb_b, Rp, col, red);
    const double beta = rz / v.rz[(k & 1) * Rp + col];
    const int lo = blockIdx.x * CT, hi = min(lo + CT, n_poses);
    for (int n = lo + wave; n < hi; n += VW) {
        if (!b.free_node[n]) continue;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const size_t at = cov_at(n, c, Rp, col);
            const double p = v.z[at] + beta * v.p[at];
            if (active) v.p[at] = p;
        }
    }
    if (blockIdx.x == 0 && wave == 0 && active) {
        v.rz[((k + 1) & 1) * Rp + col] = rz;
        v.rr[col] = rr;
        v.iters[col] += 1;
        if (!(pap > 0.0) || rr <= tol2 * v.bb[col] || !(rz > 0.0)) v.stop_k[col] = k + 1;
    }
}

// One workgroup of VW waves per (aggregate, chunk), every wave on the same 64 columns: wave w takes the aggregate's nodes
// w, w + VW, ...  k >= 0: the step of inner iteration k on the aggregate's free nodes; k < 0: the start, r as the init
// kernel left it.  Either way the aggregate's six rows of r_c = P^T r: a wave sums its nodes in ascending order, the first
// wave the VW sums in the LDS in ascending order.
__global__ __launch_bounds__(VB) void pg_cov_restrict_kernel(int n_poses, Buffers b, Coarse c, Cov v, int k)
{
    __shared__ double red[6 * VW][TB];
    const int wave = threadIdx.x / TB, lane = threadIdx.x % TB;
    const int col = blockIdx.y * TB + lane, Rp = v.R_pad;
    const bool active = k < 0 || k < v.stop_k[col];
    if (!__any(active)) return;                              // the same columns in every wave: the workgroup leaves as one
    const double alpha = k >= 0 ? cov_alpha(v, k, col, red) : 0.0;
    double rc[6] = {0, 0, 0, 0, 0, 0};
    const int lo = blockIdx.x * c.L, hi = min(lo + c.L, n_poses);
    for (int n = lo + wave; n < hi; n += VW) {
        if (!b.free_node[n]) continue;
        double r[6], z[6];
        if (k >= 0) {
            cov_step_node(b, v, n, col, alpha, active, r, z);
        } else {
#pragma unroll
            for (int q = 0; q < 6; ++q) r[q] = v.r[cov_at(n, q, Rp, col)];
        }
        const double *T = c.t + 36 * (long long)n;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int q = 0; q < 6; ++q) rc[q] += T[6 * i + q] * r[i];
    }
    wave_sums<6, false>(rc, red);                            // its first barrier: every wave has read the sum for alpha
    if (wave == 0 && active) {
#pragma unroll
        for (int q = 0; q < 6; ++q) v.rc[(6 * (size_t)blockIdx.x + q) * Rp + col] = rc[q];
    }
}

// One workgroup of VW waves per (aggregate, chunk): its six rows of y = A_c^-1 r_c (none when the factor failed: B^-1
// alone; wave w sums entries w, w + VW, ... of each row, every wave the VW sums), z += P y on its free nodes, p = z at
// the start (k < 0), and the aggregate's partials of r.r and r.z, summed as the restrict kernel sums
__global__ __launch_bounds__(VB) void pg_cov_prolong_kernel(int n_poses, Buffers b, Coarse c, Cov v, int k)
{
    __shared__ double red[6 * VW][TB];
    const int wave = threadIdx.x / TB, lane = threadIdx.x % TB;
    const int col = blockIdx.y * TB + lane, Rp = v.R_pad;
    const bool active = k < 0 || k < v.stop_k[col];
    if (!__any(active)) return;                              // the same columns in every wave: the workgroup leaves as one
    const bool coarse = c.cs->ok;
    double y[6] = {0, 0, 0, 0, 0, 0};
    if (coarse) {
        const double *row = c.ainv + 6LL * blockIdx.x * c.nc;
        for (int i = wave; i < c.nc; i += VW) {
            const double rc = v.rc[(size_t)i * Rp + col];
#pragma unroll
            for (int q = 0; q < 6; ++q) y[q] += row[(long long)q * c.nc + i] * rc;
        }
        wave_sums<6, true>(y, red);
    }
    double d[2] = {0.0, 0.0};                                // r.r, r.z
    const int lo = blockIdx.x * c.L, hi = min(lo + c.L, n_poses);
    for (int n = lo + wave; n < hi; n += VW) {
        if (!b.free_node[n]) continue;
        const double *T = c.t + 36 * (long long)n;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const size_t at = cov_at(n, i, Rp, col);
            double z = v.z[at];
            if (coarse) {
                double s = 0.0;
#pragma unroll
                for (int q = 0; q < 6; ++q) s += T[6 * i + q] * y[q];
                z += s;
                if (active) v.z[at] = z;
            }
            if (k < 0) v.p[at] = z;
            const double r = v.r[at];
            d[0] += r * r;
            d[1] += r * z;
        }
    }
    wave_sums<2, false>(d, red);                             // its first barrier: every wave has read the sums for y
    if (wave == 0 && active) {
        v.part_rr[(size_t)blockIdx.x * Rp + col] = d[0];
        v.part_rz[(size_t)blockIdx.x * Rp + col] = d[1];
    }
}

// One wave per selected pose b: joint[a, b] = rows of nodes[a] of the six columns solved for nodes[b], zero where
// nodes[a] is out of range; residual and iterations of those columns.  The first wave also counts: skipped edges, selected
// indices outside [0, N), selected poses that are not free, columns that did not reach the tolerance.  solved = 0 (no
// pose at all): nothing was solved and every output is zero.
__global__ __launch_bounds__(TB) void pg_cov_final_kernel(int n_poses, int n_nodes, const long long *__restrict__ nodes,
                                                          Buffers b, Cov v, int solved, double tol2,
                                                          double *__restrict__ joint, double *__restrict__ residual,
                                                          int *__restrict__ iterations, long long *__restrict__ stats,
                                                          const PgCoarse *__restrict__ cs, int n_agg,
                                                          double *__restrict__ coarse_stats)
{
    const int qb = blockIdx.x, lane = threadIdx.x, Rp = v.R_pad;
    if (qb < n_nodes && lane < 36) {
        const int r = lane / 6, c = lane % 6;
        for (int qa = 0; qa < n_nodes; ++qa) {
            const long long na = nodes[qa];
            const bool in = solved && na >= 0 && na < n_poses;
            joint[((long long)qa * n_nodes + qb) * 36 + lane] = in ? v.x[cov_at((int)na, r, Rp, 6 * qb + c)] : 0.0;
        }
    }
    if (qb < n_nodes && lane < 6) {
        residual[6 * qb + lane] = solved ? sqrt(v.rr[6 * qb + lane]) : 0.0;
        iterations[6 * qb + lane] = solved ? v.iters[6 * qb + lane] : 0;
    }
    if (qb != 0 || lane != 0) return;
    long long outside = 0, not_free = 0, open = 0;
    for (int q = 0; q < n_nodes; ++q) {
        const long long n = nodes[q];
        if (n < 0 || n >= n_poses)
            ++outside;
        else if (!solved || !b.free_node[n])
            ++not_free;
    }
    for (int j = 0; solved && j < 6 * n_nodes; ++j) open += !(v.rr[j] <= tol2 * v.bb[j]);
    stats[NSC_POSEGRAPH_COV_STAT_SKIPPED] = b.st->skipped;
    stats[NSC_POSEGRAPH_COV_STAT_OUTSIDE] = outside;
    stats[NSC_POSEGRAPH_COV_STAT_NOT_FREE] = not_free;
    stats[NSC_POSEGRAPH_COV_STAT_NOT_CONVERGED] = open;
    if (coarse_stats) {
        coarse_stats[0] = n_agg;
        coarse_stats[1] = cs && solved ? cs->failed : 0;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------

inline int blocks_of(long long n) { return (int)((n + TB - 1) / TB); }

struct Layout {
    Buffers b;
    Coarse c;                                // zeros without the coarse space
    Cov v;                                   // zeros outside the covariance call
    size_t total;                            // bytes; 0 where cap_ok is false
    bool cap_ok;                             // at most NSC_POSEGRAPH_MAX_AGGREGATES aggregates
};

constexpr int NO_COV = -1;                   // layout()'s Q outside the covariance call, whose own Q may be 0

// The one place that knows the workspace's layout; ws = nullptr: the size only.  The graph's regions, then with L >= 2
// those of the coarse space (aggregates of L consecutive poses), then with Q >= 0 those of a covariance call on Q poses.
Layout layout(void *ws, size_t N, size_t E, int L, int Q)
{
    Layout y = {};
    const size_t n_agg = L ? (N + L - 1) / L : 0, nc = 6 * n_agg;
    y.cap_ok = n_agg <= NSC_POSEGRAPH_MAX_AGGREGATES;
    if (!y.cap_ok) return y;
    Carver c = {reinterpret_cast<uintptr_t>(ws), 0};

    Buffers &b = y.b;
    const size_t nbn = (N + TB - 1) / TB, st_bytes = align256(sizeof(PgState));
    b.head_bytes = st_bytes + N * sizeof(int);
    char *head = c.take<char>(b.head_bytes);
    b.st = reinterpret_cast<PgState *>(head);
    b.deg = reinterpret_cast<int *>(reinterpret_cast<uintptr_t>(head) + st_bytes);
    b.row_ptr = c.take<int>(N + 1);
    b.tmp = c.take<int>(2 * E);
    b.list = c.take<int>(2 * E);
    b.ei = c.take<int>(E);
    b.ej = c.take<int>(E);
    b.free_node = c.take<int>(N);
    b.hii = c.take<double>(21 * E);
    b.hjj = c.take<double>(21 * E);
    b.hij = c.take<double>(36 * E);
    b.fe = c.take<double>(E);
    b.ge = c.take<double>(12 * E);
    b.ye = c.take<double>(12 * E);
    b.blocks = c.take<double>(21 * N);
    b.chol = c.take<double>(21 * N);
    b.x = c.take<double>(6 * N);
    b.r = c.take<double>(6 * N);
    b.z = c.take<double>(6 * N);
    b.p = c.take<double>(6 * N);
    b.ap = c.take<double>(6 * N);
    b.cand = c.take<double>(16 * N);
    b.part_e = c.take<double>(nbn);
    b.part_a = c.take<double>(nbn);
    b.part_b = c.take<double>(2 * nbn);
    b.part_s = c.take<double>(nbn);

    if (L) {
        Coarse &q = y.c;
        q.cs = c.take<PgCoarse>(1);
        q.t = c.take<double>(36 * N);
        q.ac = c.take<double>(nc * nc);
        q.lt = c.take<double>(nc * nc);
        q.ainv = c.take<double>(nc * nc);
        q.rc = c.take<double>(nc);
        q.part = c.take<double>(2 * n_agg);
        q.L = L;
        q.n_agg = (int)n_agg;
        q.nc = (int)nc;
    }

    if (Q >= 0) {
        Cov &v = y.v;
        const size_t R = 6 * (size_t)Q, Rp = (R + TB - 1) / TB * TB, tiles = (N + CT - 1) / CT;
        const size_t rows = tiles > n_agg ? tiles : n_agg;
        v.x = c.take<double>(6 * N * Rp);
        v.r = c.take<double>(6 * N * Rp);
        v.z = c.take<double>(6 * N * Rp);
        v.p = c.take<double>(6 * N * Rp);
        v.ap = c.take<double>(6 * N * Rp);
        v.part_a = c.take<double>(rows * Rp);
        v.part_rr = c.take<double>(rows * Rp);
        v.part_rz = c.take<double>(rows * Rp);
        v.rc = c.take<double>(nc * Rp);
        v.hp = c.take<double>(78 * E);
        v.rz = c.take<double>(2 * Rp);
        v.bb = c.take<double>(Rp);
        v.rr = c.take<double>(Rp);
        v.stop_k = c.take<int>(Rp);
        v.iters = c.take<int>(Rp);
        v.R = (int)R;
        v.R_pad = (int)Rp;
        v.n_tiles = (int)tiles;
    }
    y.total = c.o;
    return y;
}

bool params_ok(const NscPoseGraphParams *p)
{
    return p && p->max_iteration >= 0 && p->max_pcg_iterations >= 0 && p->pcg_tolerance >= 0.0 &&
           isfinite(p->pcg_tolerance) && p->lambda0 > 0.0 && isfinite(p->lambda0) && p->lambda_min > 0.0 &&
           isfinite(p->lambda_min) && p->lambda_factor > 1.0 && isfinite(p->lambda_factor) && p->relative_cost >= 0.0 &&
           isfinite(p->relative_cost) && p->min_step >= 0.0 && isfinite(p->min_step);
}

bool sizes_ok(int32_t n_poses, int32_t n_edges, int32_t coarse_block)
{
    return n_poses >= 0 && n_edges >= 0 && coarse_block >= 0 && coarse_block != 1;
}

// what every entry point asks of the graph it is given: the sizes, the kernel id and the pointers n_poses and n_edges imply
bool graph_ok(const double *poses, int32_t n_poses, const int64_t *edge_ij, const double *measurements,
              const double *information, int32_t n_edges, int32_t kernel, int32_t coarse_block)
{
    return sizes_ok(n_poses, n_edges, coarse_block) && n_edges <= NSC_POSEGRAPH_MAX_EDGES &&
           kernel >= NSC_POSEGRAPH_KERNEL_NONE && kernel <= NSC_POSEGRAPH_KERNEL_GEMAN_MCCLURE && (n_poses == 0 || poses) &&
           (n_edges == 0 || (edge_ij && measurements && information));
}

// the head (state and degrees) zeroed, then the lists: 5 launches (2 when there are no edges)
void build_lists(hipStream_t s, const int64_t *edge_ij, int N, int E, const Buffers &b)
{
    nsc_fill_u32(s, b.st, 0u, (long long)(b.head_bytes / 4));
    if (E > 0) {
        hipLaunchKernelGGL(pg_count_kernel, dim3(blocks_of(E)), dim3(TB), 0, s,
                           reinterpret_cast<const long long *>(edge_ij), E, N, b);
    }
    hipLaunchKernelGGL(nsc_csr_scan_kernel<0>, dim3(1), dim3(1024), 0, s, b.deg, N, b.row_ptr);
    if (E > 0) {
        hipLaunchKernelGGL(pg_fill_kernel, dim3(blocks_of(E)), dim3(TB), 0, s, E, b);
        if (N > 0) hipLaunchKernelGGL(pg_sort_kernel, dim3(N), dim3(TB), 0, s, b);
    }
}

// The system at `poses` and the state's lambda, N > 0: linearise, assemble with the start of PCG, and with the coarse
// space P, A_c, its factor and its inverse.  2 launches (1 without edges), 4 more with the coarse space.
void launch_system(hipStream_t s, const double *poses, const double *measurements, const double *information,
                   const uint8_t *fixed, int N, int E, int kernel, const double *edge_scale, const Layout &y)
{
    const Buffers &b = y.b;
    const Coarse &c = y.c;
    const int gn = blocks_of(N);
    if (E > 0)
        hipLaunchKernelGGL(pg_linearize_kernel, dim3(blocks_of(E)), dim3(TB), 0, s, poses, measurements, information, E, b,
                           nullptr, kernel, edge_scale, nullptr);
    hipLaunchKernelGGL(pg_assemble_kernel, dim3(gn), dim3(TB), 0, s, N, E, fixed, b, nullptr, b.blocks, 1);
    if (c.L) {
        hipLaunchKernelGGL(pg_coarse_basis_kernel, dim3(gn), dim3(TB), 0, s, poses, N, b, c);
        hipLaunchKernelGGL(pg_coarse_galerkin_kernel, dim3(c.n_agg * c.n_agg), dim3(TB), 0, s, N, E, b, c);
        hipLaunchKernelGGL(pg_coarse_factor_kernel, dim3(1), dim3(CB), 0, s, b, c);
        hipLaunchKernelGGL(pg_coarse_invert_kernel, dim3(c.nc), dim3(TB), 0, s, b, c);
    }
}

// nsc_posegraph_optimize_robust (coarse_block = 0) and nsc_posegraph_optimize_coarse
int optimize(const double *poses, int32_t n_poses, const int64_t *edge_ij, const double *measurements,
             const double *information, int32_t n_edges, const uint8_t *fixed, const NscPoseGraphParams *params,
             double *poses_out, double *stats, double *cost_history, double *step0, void *ws, size_t ws_bytes,
             void *stream, int32_t kernel, const double *edge_scale, double *edge_chi2, double *edge_weight,
             int32_t coarse_block, double *coarse_stats)
{
    if (!graph_ok(poses, n_poses, edge_ij, measurements, information, n_edges, kernel, coarse_block) || !params_ok(params) ||
        !stats || !cost_history || (n_poses > 0 && (!poses_out || !fixed)))
        return NSC_EINVAL;
    const int L = coarse_block;
    const Layout y = layout(ws, n_poses, n_edges, L, NO_COV);
    if (!y.cap_ok) return NSC_EUNSUPPORTED;
    // per outer step 8 launches and 4 per inner iteration; with the coarse space 14 and 5
    if ((long long)params->max_iteration * ((L ? 5LL : 4LL) * params->max_pcg_iterations + (L ? 14 : 8)) >
        NSC_POSEGRAPH_MAX_LAUNCHES)
        return NSC_EUNSUPPORTED;
    if (!ws || ws_bytes < y.total) return NSC_EWORKSPACE;
    const Buffers &b = y.b;
    const Coarse &c = y.c;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int N = n_poses, E = n_edges, gn = blocks_of(N), ge = blocks_of(E), ga = c.n_agg;
    const NscPoseGraphParams prm = *params;
    const double tol2 = prm.pcg_tolerance * prm.pcg_tolerance;
    // r.r and r.z reach the begin and direction kernels as one partial per workgroup of nodes or, with the coarse space, one
    // per aggregate
    const double *part = L ? c.part : b.part_b;
    const int n_part = L ? ga : gn;

    build_lists(s, edge_ij, N, E, b);
    if (N > 0 && poses_out != poses)
        hipLaunchKernelGGL(pg_copy_kernel, dim3(blocks_of(16LL * N)), dim3(TB), 0, s, poses, poses_out, 16LL * N);
    if (E > 0)
        hipLaunchKernelGGL(pg_edge_cost_kernel, dim3(ge), dim3(TB), 0, s, poses_out, measurements, information, E, b, 0,
                           kernel, edge_scale, b.fe, nullptr, nullptr);
    if (N > 0) hipLaunchKernelGGL(pg_cost_gather_kernel, dim3(gn), dim3(TB), 0, s, N, b);
    hipLaunchKernelGGL(pg_init_kernel, dim3(1), dim3(TB), 0, s, gn, b, prm.lambda0, cost_history, c.cs);

    for (int it = 0; it < prm.max_iteration && N > 0; ++it) {
        launch_system(s, poses_out, measurements, information, fixed, N, E, kernel, edge_scale, y);
        if (L) {
            hipLaunchKernelGGL(pg_coarse_restrict_kernel, dim3(ga), dim3(TB), 0, s, N, gn, b, c, -1);
            hipLaunchKernelGGL(pg_coarse_prolong_kernel, dim3(ga), dim3(TB), 0, s, N, b, c, -1);
        }
        hipLaunchKernelGGL(pg_pcg_begin_kernel, dim3(1), dim3(TB), 0, s, b, part, n_part);
        for (int k = 0; k < prm.max_pcg_iterations && E > 0; ++k) {
            hipLaunchKernelGGL(pg_edge_matvec_kernel, dim3(ge), dim3(TB), 0, s, E, b, k);
            hipLaunchKernelGGL(pg_node_matvec_kernel, dim3(gn), dim3(TB), 0, s, N, b, k);
            if (L) {
                hipLaunchKernelGGL(pg_coarse_restrict_kernel, dim3(ga), dim3(TB), 0, s, N, gn, b, c, k);
                hipLaunchKernelGGL(pg_coarse_prolong_kernel, dim3(ga), dim3(TB), 0, s, N, b, c, k);
            } else {
                hipLaunchKernelGGL(pg_pcg_step_kernel, dim3(gn), dim3(TB), 0, s, N, b, k);
            }
            hipLaunchKernelGGL(pg_pcg_direction_kernel, dim3(gn), dim3(TB), 0, s, N, b, k, tol2, part, n_part);
        }
        hipLaunchKernelGGL(pg_update_kernel, dim3(gn), dim3(TB), 0, s, poses_out, N, b, it, step0);
        if (E > 0)
            hipLaunchKernelGGL(pg_edge_cost_kernel, dim3(ge), dim3(TB), 0, s, b.cand, measurements, information, E, b, 0,
                               kernel, edge_scale, b.fe, nullptr, nullptr);
        hipLaunchKernelGGL(pg_cost_gather_kernel, dim3(gn), dim3(TB), 0, s, N, b);
        hipLaunchKernelGGL(pg_accept_kernel, dim3(1), dim3(TB), 0, s, gn, b, prm, it, cost_history);
        hipLaunchKernelGGL(pg_commit_kernel, dim3(gn), dim3(TB), 0, s, poses_out, N, b, it);
    }
    hipLaunchKernelGGL(pg_finalize_kernel, dim3(1), dim3(TB), 0, s, b, prm.max_iteration, stats, cost_history, c.cs, ga,
                       coarse_stats);
    if (E > 0 && (edge_chi2 || edge_weight))
        hipLaunchKernelGGL(pg_edge_cost_kernel, dim3(ge), dim3(TB), 0, s, poses_out, measurements, information, E, b, 1,
                           kernel, edge_scale, nullptr, edge_chi2, edge_weight);
    return launch_status();
}

}  // namespace

extern "C" {

size_t nsc_posegraph_covariance_workspace_bytes(int32_t n_poses, int32_t n_edges, int32_t n_nodes, int32_t coarse_block)
{
    if (!sizes_ok(n_poses, n_edges, coarse_block) || n_edges > NSC_POSEGRAPH_MAX_EDGES || n_nodes < 0 ||
        n_nodes > NSC_POSEGRAPH_MAX_COV_NODES)
        return 0;
    return layout(nullptr, n_poses, n_edges, coarse_block, n_nodes).total;
}

int nsc_posegraph_covariance(const double *poses, int32_t n_poses, const int64_t *edge_ij, const double *measurements,
                             const double *information, int32_t n_edges, const uint8_t *fixed,
                             const NscPoseGraphParams *params, const int64_t *nodes, int32_t n_nodes, double *joint,
                             double *residual, int32_t *iterations, int64_t *stats, void *ws, size_t ws_bytes,
                             void *stream, int32_t kernel, const double *edge_scale, int32_t coarse_block,
                             double *coarse_stats)
{
    if (!graph_ok(poses, n_poses, edge_ij, measurements, information, n_edges, kernel, coarse_block) || !params_ok(params) ||
        !stats || (n_poses > 0 && !fixed) || n_nodes < 0 || (n_nodes > 0 && (!nodes || !joint || !residual || !iterations)))
        return NSC_EINVAL;
    if (n_nodes > NSC_POSEGRAPH_MAX_COV_NODES) return NSC_EUNSUPPORTED;
    const int L = coarse_block;
    // per inner iteration 3 launches, 4 with the coarse space; at most 18 around the loop
    if ((L ? 4LL : 3LL) * params->max_pcg_iterations + 18 > NSC_POSEGRAPH_MAX_LAUNCHES) return NSC_EUNSUPPORTED;
    const Layout y = layout(ws, n_poses, n_edges, L, n_nodes);
    if (!y.cap_ok) return NSC_EUNSUPPORTED;
    if (!ws || ws_bytes < y.total) return NSC_EWORKSPACE;
    const Buffers &b = y.b;
    const Coarse &c = y.c;
    const Cov &v = y.v;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int N = n_poses, E = n_edges, Q = n_nodes, ga = c.n_agg;
    const double tol2 = params->pcg_tolerance * params->pcg_tolerance;
    const dim3 tiles(v.n_tiles, v.R_pad / TB), aggs(ga, v.R_pad / TB);
    const long long *sel = reinterpret_cast<const long long *>(nodes);
    const bool solve = N > 0 && Q > 0;

    build_lists(s, edge_ij, N, E, b);        // the state zeroed: done = 0 and lambda = 0, the undamped system
    if (solve) {
        if (L) nsc_fill_u32(s, c.cs, 0u, (long long)(sizeof(PgCoarse) / 4));
        launch_system(s, poses, measurements, information, fixed, N, E, kernel, edge_scale, y);
        if (E > 0) hipLaunchKernelGGL(pg_cov_pack_kernel, dim3(blocks_of(E)), dim3(TB), 0, s, E, b, v.hp);
        hipLaunchKernelGGL(pg_cov_init_kernel, tiles, dim3(VB), 0, s, N, sel, b, v);
        if (L) {
            hipLaunchKernelGGL(pg_cov_restrict_kernel, aggs, dim3(VB), 0, s, N, b, c, v, -1);
            hipLaunchKernelGGL(pg_cov_prolong_kernel, aggs, dim3(VB), 0, s, N, b, c, v, -1);
        }
        hipLaunchKernelGGL(pg_cov_begin_kernel, dim3(v.R_pad / TB), dim3(VB), 0, s, L ? ga : v.n_tiles, v);
        for (int k = 0; k < params->max_pcg_iterations && E > 0; ++k) {
            hipLaunchKernelGGL(pg_cov_matvec_kernel, tiles, dim3(VB), 0, s, N, b.row_ptr, b.list, b.ei, b.ej, b.free_node,
                               v.hp, v, k);
            if (L) {
                hipLaunchKernelGGL(pg_cov_restrict_kernel, aggs, dim3(VB), 0, s, N, b, c, v, k);
                hipLaunchKernelGGL(pg_cov_prolong_kernel, aggs, dim3(VB), 0, s, N, b, c, v, k);
            } else {
                hipLaunchKernelGGL(pg_cov_step_kernel, tiles, dim3(VB), 0, s, N, b, v, k);
            }
            hipLaunchKernelGGL(pg_cov_direction_kernel, tiles, dim3(VB), 0, s, N, b, v, k, tol2, L ? ga : v.n_tiles);
        }
    }
    hipLaunchKernelGGL(pg_cov_final_kernel, dim3(Q > 0 ? Q : 1), dim3(TB), 0, s, N, Q, sel, b, v, solve ? 1 : 0, tol2, joint,
                       residual, iterations, reinterpret_cast<long long *>(stats), solve ? c.cs : nullptr, ga, coarse_stats);
    return launch_status();
}

void nsc_posegraph_default_params(NscPoseGraphParams *p)
{
    if (!p) return;
    p->max_iteration = 20;
    p->max_pcg_iterations = 100;
    p->pcg_tolerance = 1e-6;
    p->lambda0 = 1e-4;
    p->lambda_min = 1e-9;
    p->lambda_factor = 10.0;
    p->relative_cost = 1e-9;
    p->min_step = 1e-9;
}

size_t nsc_posegraph_workspace_bytes(int32_t n_poses, int32_t n_edges, const NscPoseGraphParams *params)
{
    (void)params;                            // the layout holds one outer and one inner iteration whatever the caps
    return nsc_posegraph_coarse_workspace_bytes(n_poses, n_edges, 0);
}

int nsc_posegraph_linearize(const double *poses, int32_t n_poses, const int64_t *edge_ij, const double *measurements,
                            const double *information, int32_t n_edges, double *residuals, double *cost,
                            double *gradient, double *blocks, int64_t *skipped, void *ws, size_t ws_bytes, void *stream)
{
    return nsc_posegraph_linearize_robust(poses, n_poses, edge_ij, measurements, information, n_edges, residuals, cost,
                                          gradient, blocks, skipped, ws, ws_bytes, stream, NSC_POSEGRAPH_KERNEL_NONE,
                                          nullptr, nullptr);
}

int nsc_posegraph_linearize_robust(const double *poses, int32_t n_poses, const int64_t *edge_ij,
                                   const double *measurements, const double *information, int32_t n_edges,
                                   double *residuals, double *cost, double *gradient, double *blocks, int64_t *skipped,
                                   void *ws, size_t ws_bytes, void *stream, int32_t kernel, const double *edge_scale,
                                   double *weights)
{
    if (!graph_ok(poses, n_poses, edge_ij, measurements, information, n_edges, kernel, 0) || !cost || !skipped ||
        (n_poses > 0 && (!gradient || !blocks)) || (n_edges > 0 && !residuals))
        return NSC_EINVAL;
    const Layout y = layout(ws, n_poses, n_edges, 0, NO_COV);
    if (!ws || ws_bytes < y.total) return NSC_EWORKSPACE;
    const Buffers &b = y.b;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int N = n_poses, E = n_edges;
    build_lists(s, edge_ij, N, E, b);
    if (E > 0) {
        hipLaunchKernelGGL(pg_edge_cost_kernel, dim3(blocks_of(E)), dim3(TB), 0, s, poses, measurements, information, E, b,
                           0, kernel, edge_scale, b.fe, nullptr, nullptr);
        hipLaunchKernelGGL(pg_linearize_kernel, dim3(blocks_of(E)), dim3(TB), 0, s, poses, measurements, information, E, b,
                           residuals, kernel, edge_scale, weights);
    }
    if (N > 0) {
        hipLaunchKernelGGL(pg_cost_gather_kernel, dim3(blocks_of(N)), dim3(TB), 0, s, N, b);
        hipLaunchKernelGGL(pg_assemble_kernel, dim3(blocks_of(N)), dim3(TB), 0, s, N, E, nullptr, b, gradient, blocks, 0);
    }
    hipLaunchKernelGGL(pg_linearize_out_kernel, dim3(1), dim3(TB), 0, s, blocks_of(N), b, cost,
                       reinterpret_cast<long long *>(skipped));
    return launch_status();
}

int nsc_posegraph_optimize(const double *poses, int32_t n_poses, const int64_t *edge_ij, const double *measurements,
                           const double *information, int32_t n_edges, const uint8_t *fixed,
                           const NscPoseGraphParams *params, double *poses_out, double *stats, double *cost_history,
                           double *step0, void *ws, size_t ws_bytes, void *stream)
{
    return nsc_posegraph_optimize_robust(poses, n_poses, edge_ij, measurements, information, n_edges, fixed, params,
                                         poses_out, stats, cost_history, step0, ws, ws_bytes, stream,
                                         NSC_POSEGRAPH_KERNEL_NONE, nullptr, nullptr, nullptr);
}

int nsc_posegraph_optimize_robust(const double *poses, int32_t n_poses, const int64_t *edge_ij,
                                  const double *measurements, const double *information, int32_t n_edges,
                                  const uint8_t *fixed, const NscPoseGraphParams *params, double *poses_out,
                                  double *stats, double *cost_history, double *step0, void *ws, size_t ws_bytes,
                                  void *stream, int32_t kernel, const double *edge_scale, double *edge_chi2,
                                  double *edge_weight)
{
    return optimize(poses, n_poses, edge_ij, measurements, information, n_edges, fixed, params, poses_out, stats,
                    cost_history, step0, ws, ws_bytes, stream, kernel, edge_scale, edge_chi2, edge_weight, 0, nullptr);
}

size_t nsc_posegraph_coarse_workspace_bytes(int32_t n_poses, int32_t n_edges, int32_t coarse_block)
{
    if (!sizes_ok(n_poses, n_edges, coarse_block)) return 0;
    return layout(nullptr, n_poses, n_edges, coarse_block, NO_COV).total;
}

int nsc_posegraph_optimize_coarse(const double *poses, int32_t n_poses, const int64_t *edge_ij,
                                  const double *measurements, const double *information, int32_t n_edges,
                                  const uint8_t *fixed, const NscPoseGraphParams *params, double *poses_out,
                                  double *stats, double *cost_history, double *step0, void *ws, size_t ws_bytes,
                                  void *stream, int32_t kernel, const double *edge_scale, double *edge_chi2,
                                  double *edge_weight, int32_t coarse_block, double *coarse_stats)
{
    return optimize(poses, n_poses, edge_ij, measurements, information, n_edges, fixed, params, poses_out, stats,
                    cost_history, step0, ws, ws_bytes, stream, kernel, edge_scale, edge_chi2, edge_weight, coarse_block,
                    coarse_stats);
}

}  // extern "C"
