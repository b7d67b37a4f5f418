// What every kernel set of the GNN path must compute with the same bits, stated once: the BatchNorm(eval) fold, the value
// of a projection ahead of its residual, and where an attention column goes.  The kernels keep their own loads (each issues
// its bias, BatchNorm operands and residual where it measured best) and their own row passes and branches, and call these
// for the arithmetic.  The functions are straight-line on purpose: hipcc optimises a callee on its own before it inlines it,
// and one with a branch in it (a whole store path, say) comes back with its address arithmetic hoisted differently -- other
// registers, another schedule in every GEMM of the path (profiles/gnn_refactor.md).  With these the six kernels compile to
// the instructions they had when each spelled the expressions out.
// Also here, because both forwards dispatch and check the same way: the epilogue descriptor of the GEMMs, the CH dispatch of
// the attention kernels and the model checks that the inference and the training entry points share.
// Included by nsc_gat.hip and nsc_gat_train.hip inside their anonymous namespace, ahead of nsc_gemm_glds.h and
// nsc_gat_banded.h (the includer has <hip/hip_runtime.h>, <type_traits> and include/nsc.h before it opens that namespace).
#pragma once

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Columns >= n_main of a GEMM come from the extra rows Bx (the folded attention vectors of the inference forward) and are
// written to aux0 / aux1 instead of C.
struct GemmEpi {
    const float *bias;                              // per column, nullable
    const float *bn_w, *bn_b, *bn_mean, *bn_var;    // BatchNorm eval, nullable as a group
    float bn_eps;
    int relu;
    const float *resid;                             // (M, ldr) added last, nullable
    int ldr;
    float *aux0, *aux1;                             // columns n_main, n_main+1 (M each), nullable
};

// EPI: 0 = plain store + aux columns (lin), 1 = bias + BatchNorm + ReLU (input_proj),
//      2 = bias + residual (output_proj / residual_proj)

// torch batch_norm eval: alpha = invstd * weight, beta = bias - mean * alpha
__device__ __forceinline__ float bn_scale(float var, float eps, float w)
{
    const float invstd = 1.0f / sqrtf(var + eps);
    return invstd * w;
}
__device__ __forceinline__ float bn_shift(float b, float mean, float scale) { return b - mean * scale; }

// both for column `col`, read from memory here: var and w, then b and mean
__device__ __forceinline__ void bn_fold(const float *var, float eps, const float *w, const float *b, const float *mean, int col,
                                        float &scale, float &shift)
{
    scale = bn_scale(var[col], eps, w[col]);
    shift = bn_shift(b[col], mean[col], scale);
}

// BatchNorm(eval) applied: the folded scale and shift on a value that already has its bias
__device__ __forceinline__ float bn_apply(float v, float scale, float shift) { return v * scale + shift; }

// ReLU as torch.relu computes it: a NaN stays a NaN.  fmaxf(NaN, 0) is 0, and a poisoned row came out as a row of zeros that
// every later stage took for real (include/nsc.h, nsc_gat_forward).  For every other value this is what fmaxf(v, 0.0f)
// returns, except -0, which stays -0 where fmaxf gives +0 (the value is added to sums and multiplied from here on: nothing
// downstream tells the two apart).  A compare and a select, straight-line: every ReLU of the GNN path -- inference and
// training, all kernel sets -- is this expression.
__device__ __forceinline__ float relu_nan(float v) { return v < 0.0f ? 0.0f : v; }

// a projection's value ahead of its residual
template <int EPI> __device__ __forceinline__ float epi_value(float v, float bias, float scale, float shift)
{
    if (EPI != 0) v = v + bias;
    if (EPI == 1) v = relu_nan(bn_apply(v, scale, shift));
    return v;
}

// a column past n_main (the attention columns of the lin GEMM) goes to its aux vector as it is
__device__ __forceinline__ void epi_store_aux(float v, float *aux0, float *aux1, int row, int col, int n_main)
{
    float *aux = (col == n_main) ? aux0 : aux1;
    aux[row] = v;
}

// CH = ceil(H / 256) of the attention kernels (H <= 1024: check_gat_dims) as a compile-time constant: f(std::integral_constant<int, CH>)
template <class F> void dispatch_ch(int H, F f)
{
    switch ((H + 255) / 256) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
    }
}

// What check_model (inference) and check_train ask of a model's dimensions, in the order both report it.  out_quad: the
// training step stores the output in float4s (out_dim a multiple of 4).  eval_bn: the inference forward reads the input
// BatchNorm's running statistics, and reports a missing one (NSC_EINVAL) ahead of an unsupported edge_dim.
inline int check_gat_dims(const NscGatModel *m, bool out_quad, bool eval_bn)
{
    if (m->n_layers < 1 || m->n_layers > NSC_GAT_MAX_LAYERS) return NSC_EUNSUPPORTED;
    if (m->hidden < 16 || m->hidden > 1024 || (m->hidden & 15)) return NSC_EUNSUPPORTED;   // GEMM k-blocks of 16
    if (m->in_dim < 16 || (m->in_dim & 15) || m->out_dim < (out_quad ? 4 : 1) || (out_quad && (m->out_dim & 3))) return NSC_EUNSUPPORTED;
    if (eval_bn && (!m->in_bn_w || !m->in_bn_b || !m->in_bn_mean || !m->in_bn_var)) return NSC_EINVAL;
    if (m->edge_dim < 0 || m->edge_dim > NSC_GAT_MAX_EDGE_DIM) return NSC_EUNSUPPORTED;
    if (m->residual && m->in_dim != m->out_dim && (!m->res_w || !m->res_b)) return NSC_EINVAL;   // model.py:91-94
    return NSC_OK;
}
