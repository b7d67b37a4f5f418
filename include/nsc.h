/*
 * nsc.h -- C ABI of libnsc_hip.so, the MI355X (gfx950) implementation of the Neural-Spectral-Codec
 * descriptor hot path.
 *
 * The reference is pure Python and has no FFI layer; its boundary for this path is two nn.Module
 * APIs.  Each entry point below replaces the device work behind one of those
 * calls; the Python classes in neural-spectral-codec_amd/{encoding,gnn}/ keep the reference's
 * names and signatures and bind these functions with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer owned by the caller (e.g. torch tensor storage);
 *     parameter structs are HOST pointers, read before the call returns
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), allocates nothing,
 *     keeps no mutable global state and is safe to capture into a hipGraph
 *   - return value: 0 = NSC_OK, negative = NscStatus error; nothing is launched on error
 *   - no torch types, no C++ types, no exceptions across the boundary
 */
#ifndef NSC_H
#define NSC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSC_ABI_VERSION 4

typedef enum NscStatus {
    NSC_OK            = 0,
    NSC_EINVAL        = -1,  /* null pointer / negative size / inconsistent arguments          */
    NSC_EUNSUPPORTED  = -2,  /* shape outside what the kernels are built for (see each call)   */
    NSC_EWORKSPACE    = -3,  /* workspace smaller than nsc_*_workspace_bytes()                  */
    NSC_ELAUNCH       = -4   /* hipLaunchKernel reported an error (hipGetLastError has details) */
} NscStatus;

int         nsc_abi_version(void);
const char *nsc_status_string(int status);

/* ------------------------------------------------------------------------------------------
 * Encoder: point cloud -> E x 360 min-range image -> circular gap interpolation -> row-wise
 * 360-point real FFT magnitude -> per-row 181->n_bins histogram -> global L1 normalisation.
 * Replaces SpectralEncoder.encode_points / encode_range_image / forward
 *   (reference src/encoding/spectral_encoder.py:206, :160, :231) and what they call:
 *   RangeImageProjector.project (src/encoding/range_image.py:129) and
 *   interpolate_range_image    (src/encoding/range_image.py:15).
 * ------------------------------------------------------------------------------------------ */
typedef struct NscEncParams {
    int32_t n_elevation;   /* projector rows E: 1..64          range_image.py:104              */
    int32_t n_azimuth;     /* projector cols A: must be 360    range_image.py:105              */
    int32_t n_bins;        /* histogram bins per row, 1..176   spectral_encoder.py:39          */
    int32_t target_rows;   /* target_elevation_bins R, 1..16   spectral_encoder.py:43          */
    double  elev_min_rad;  /* np.deg2rad(elevation_range[0])   range_image.py:126              */
    double  elev_max_rad;  /* np.deg2rad(elevation_range[1])   range_image.py:127              */
    float   min_range;     /* 1.0                              range_image.py:108              */
    float   max_range;     /* 80.0                             range_image.py:107              */
    float   epsilon;       /* 1e-8                             spectral_encoder.py:42          */
    int32_t interpolate;   /* interpolate_empty                spectral_encoder.py:44,220      */
    int32_t elev_f64;      /* 1 = row math in float64 (numpy >= 2 promotion of range_image.py:186),
                              0 = float32 (numpy 1.24 value-based casting)                      */
} NscEncParams;

void nsc_enc_default_params(NscEncParams *p);

/* Bytes of scratch nsc_encode_clouds needs for this batch (0 when the fused one-workgroup-per-
 * cloud kernel is used; non-zero when clouds are split across workgroups). */
size_t nsc_encode_clouds_workspace_bytes(int32_t n_clouds, int64_t total_points,
                                         const NscEncParams *p);

/* Which kernel set nsc_encode_clouds launches for a batch of this shape (the launcher calls the same decision
 * function): NSC_ENC_PATH_FAST = encode_fast_kernel, the streaming kernel of the configuration every reference caller
 * uses (16 x 360 image, no pooling, (N,4) points, default FOV / range window; any number of clouds, a single cloud of
 * >= 2^27 points takes a slower loop inside it); NSC_ENC_PATH_FUSED = encode_fused_kernel (any other shape);
 * NSC_ENC_PATH_SPLIT = scatter_split_kernel + finish_kernel (few large clouds).  Negative = NscStatus error. */
#define NSC_ENC_PATH_FAST 1
#define NSC_ENC_PATH_FUSED 2
#define NSC_ENC_PATH_SPLIT 3
int nsc_encode_clouds_path(int32_t n_clouds, int64_t total_points, int32_t stride_floats, const NscEncParams *p);

/* SpectralEncoder.encode_points for a packed batch of clouds.
 *   pts            (total_points, stride) float32, row-major AoS [x,y,z(,intensity)]; stride 3 or 4
 *   cloud_offsets  (n_clouds+1) int64 point offsets, cloud c = [off[c], off[c+1]); off[0] = 0
 *   lut            (181) int32  frequency -> bin table (spectral_encoder.py:136-145), monotone
 *   out_desc       (n_clouds, target_rows*n_bins) float32
 *   out_raw        nullable (n_clouds, E, 360) float32  image before interpolation
 *   out_interp     nullable (n_clouds, E, 360) float32  image after interpolation
 *   ws, ws_bytes   scratch of at least nsc_encode_clouds_workspace_bytes() (may be NULL if 0) */
int nsc_encode_clouds(const float *pts, const int64_t *cloud_offsets, int32_t n_clouds,
                      int64_t total_points, int32_t stride_floats, const NscEncParams *p,
                      const int32_t *lut, float *out_desc, float *out_raw, float *out_interp,
                      void *ws, size_t ws_bytes, void *stream);

/* The two halves of nsc_encode_clouds as separate launches, so a caller can overlap the (ALU-bound)
 * finish of batch k with the (HBM-bound) scatter of batch k+1 on two streams:
 *   nsc_scatter_clouds: points -> (n_clouds, E, 360) uint32 images of the MINIMUM SQUARED range
 *                       (float32 bit pattern, 0xffffffff = empty pixel)    range_image.py:129-208
 *   nsc_finish_images : those images -> sqrt, interpolation, FFT, histogram, normalisation */
int nsc_scatter_clouds(const float *pts, const int64_t *cloud_offsets, int32_t n_clouds,
                       int64_t total_points, int32_t stride_floats, const NscEncParams *p,
                       uint32_t *out_sqr, void *stream);
int nsc_finish_images(const uint32_t *sqr, int32_t n_images, const NscEncParams *p, const int32_t *lut,
                      float *out_desc, float *out_raw, float *out_interp, void *stream);

/* SpectralEncoder.forward / encode_range_image for a batch of range images (no projection, no
 * interpolation; rows != target_rows are average-pooled like adaptive_avg_pool2d).
 *   imgs      (n_images, rows, 360) float32, rows 1..64
 *   out_desc  (n_images, target_rows*n_bins) float32 */
int nsc_encode_range_images(const float *imgs, int32_t n_images, int32_t rows,
                            const NscEncParams *p, const int32_t *lut, float *out_desc,
                            void *stream);

/* Intensity image of RangeImageProjector.project(points, keep_intensity=True) (reference range_image.py:216-228):
 * per pixel the maximum intensity over the points whose float32 range equals the pixel's minimum range, 0 where no
 * point fell (and never below 0: the reference max-reduces into a zero image).  points are (N,4) rows; range_raw is
 * the raw range image batch of the same clouds (out_raw of nsc_encode_clouds).  A NaN intensity among a pixel's closest
 * points makes the pixel NaN (np.maximum.at propagates it; the result is the canonical quiet NaN). */
int nsc_project_intensity(const float *points, const int64_t *cloud_offsets, int32_t n_clouds, int64_t total_points,
                          const NscEncParams *p, const float *range_raw, float *out_intensity, void *stream);

/* interpolate_range_image(img, 'linear') (reference range_image.py:15-89) for a batch of float32 range
 * images (n_images, rows, 360), 0 = empty pixel; rows 1..64. */
int nsc_interpolate_range_images(const float *imgs, int32_t n_images, int32_t rows, const int32_t *lut,
                                 float *out, void *stream);
/* The same with the reference's `method` argument: NSC_INTERP_LINEAR (range_image.py:52-64) or NSC_INTERP_NEAREST
 * (:66-75: the circularly nearest valid pixel of the row, the smaller column on a tie).  NscEncParams.interpolate
 * takes the same values (0 = off). */
#define NSC_INTERP_LINEAR 1
#define NSC_INTERP_NEAREST 2
int    nsc_interpolate_range_images_ex(const float *imgs, int32_t n_images, int32_t rows, const int32_t *lut,
                                       int32_t method, float *out, void *stream);


/* ------------------------------------------------------------------------------------------
 * GNN enhancer: Linear 800->256 + BN + ReLU, 3 x GATConv(256->256, heads=1, edge_dim) + BN,
 * Linear 256->800 + input residual.  Replaces SpectralGNN.forward / forward_with_attention
 * (reference src/gnn/model.py:96-153, :155-201) and the torch_geometric 2.4.0 GATConv it calls
 * (model.py:16,75-84,127; algorithm restated in SURVEY.md Appendix B).
 * ------------------------------------------------------------------------------------------ */
#define NSC_GAT_MAX_LAYERS 8
#define NSC_GAT_MAX_EDGE_DIM 8

typedef struct NscGatLayer {      /* device pointers; names are the reference's state-dict keys */
    const float *lin_w;           /* convs.{l}.lin_src.weight (H,H)  (lin_dst is the same tensor)   */
    const float *att_src;         /* convs.{l}.att_src (H)                                          */
    const float *att_dst;         /* convs.{l}.att_dst (H)                                          */
    const float *lin_edge_w;      /* convs.{l}.lin_edge.weight (H,edge_dim), NULL without edge_dim  */
    const float *att_edge;        /* convs.{l}.att_edge (H), NULL without edge_dim                  */
    const float *bias;            /* convs.{l}.bias (H)                                             */
    const float *bn_w, *bn_b, *bn_mean, *bn_var;   /* batch_norms.{l}.{weight,bias,running_*} (H)  */
} NscGatLayer;

typedef struct NscGatModel {
    int32_t in_dim;               /* 800   model.py:33 (multiple of 16) */
    int32_t hidden;               /* 256   model.py:34 (multiple of 16, <= 1024) */
    int32_t out_dim;              /* 800   model.py:35 */
    int32_t n_layers;             /* 3     model.py:36 */
    int32_t edge_dim;             /* 0 = GATConv built without edge_dim (pipeline.py:158-166) */
    int32_t residual;             /* model.py:39 */
    float   bn_eps;               /* 1e-5 */
    float   negative_slope;       /* 0.2 (GATConv default) */
    const float *in_w, *in_b;     /* input_proj.{weight (H,in), bias (H)}      model.py:67 */
    const float *in_bn_w, *in_bn_b, *in_bn_mean, *in_bn_var;   /* input_norm.* model.py:68 */
    const float *out_w, *out_b;   /* output_proj.{weight (out,H), bias (out)}  model.py:88 */
    const float *res_w, *res_b;   /* residual_proj.* (out,in) or NULL when in_dim == out_dim (model.py:91-94) */
    const float *folded;          /* nsc_gat_fold_weights() output, nsc_gat_folded_floats() floats */
    NscGatLayer layers[NSC_GAT_MAX_LAYERS];
} NscGatModel;

/* Graph in CSR-by-target form with PyG's self-loop convention applied (existing self loops removed,
 * one loop per node appended last, its edge attribute = mean of the node's incoming edge attributes). */
typedef struct NscGraph {
    int32_t n_nodes;
    int32_t nnz;                  /* capacity of src/eid = E + n_nodes (stride of alpha_out layers) */
    const int32_t *row_ptr;       /* (n_nodes+1) */
    const int32_t *src;           /* (nnz) source node of each entry, entries of a target in edge order */
    const int32_t *eid;           /* (nnz) index into the caller's edge list, -1 for the self loop */
    const float   *loop_attr;     /* (n_nodes, edge_dim) or NULL */
    /* transposed view (entries grouped by SOURCE), needed by nsc_gat_backward only; NULL otherwise */
    const int32_t *t_ptr;         /* (n_nodes+1) */
    const int32_t *t_entry;       /* (nnz) entry indices into src/eid, ascending per source */
    const int32_t *tgt;           /* (nnz) target node of each entry */
    /* banded form (nsc_graph_band_entries), NULL / 0 otherwise: lets nsc_gat_forward run a GATConv layer as one launch */
    const float   *band_entries;  /* (n_nodes, 8, 4) float32, 16-byte aligned */
    int32_t        band;          /* half bandwidth the caller vouches for (max |source - target| <= band, and at most 8
                                     entries per target incl. the self loop), 0 = not banded.  The kernels support <= 2 */
} NscGraph;

size_t nsc_graph_workspace_bytes(int32_t n_nodes, int64_t n_edges);

/* edge_index (2,E) int64 [row 0 = source j, row 1 = target i] -> CSR arrays (caller-allocated:
 * row_ptr n_nodes+1, src/eid E+n_nodes, loop_attr n_nodes*edge_dim); row_ptr[n_nodes] is the entry
 * count.  Edges with an endpoint outside [0,n_nodes) are dropped. */
int nsc_graph_build_csr(const int64_t *edge_index, int64_t n_edges, int32_t n_nodes,
                        const float *edge_attr, int32_t edge_dim, int32_t *row_ptr, int32_t *src,
                        int32_t *eid, float *loop_attr, void *ws, size_t ws_bytes, void *stream);

/* Banded form of a graph whose CSR exists: per target 8 slots {source (int32 bits), edge_attr[0], edge_attr[1], CSR entry
 * index (int32 bits, -1 = empty slot)} in CSR order, self loop last with loop_attr -- the neighbourhood of a target in ONE
 * 128-byte fetch -- plus info[0] = max |source - target| and info[1] = max entries per target over the graph (int32,
 * device).  A caller that reads info[0] <= 2 and info[1] <= 8 sets NscGraph.band_entries / band = 2: nsc_gat_forward then
 * runs every GATConv layer as one launch (gat_layer_banded_kernel: lin GEMM + 2-row halo, softmax, aggregation, BatchNorm
 * in one kernel, h never leaves LDS) -- the temporal chain of the reference (src/keyframe/graph_manager.py:520-532,
 * abs(i - j) <= 2) always qualifies.  The entries embed the edge attributes (edge_dim 0 or 2; otherwise the banded path is
 * not taken): rebuild them when edge_attr changes.  entries: (n_nodes, 8, 4) float32, 16-byte aligned. */
int nsc_graph_band_entries(const NscGraph *g, const float *edge_attr, int32_t edge_dim, float *entries, int32_t *info,
                           void *stream);

/* Weights-only folding, redone only when the GATConv parameters change: per layer
 * u_src = W^T att_src, u_dst = W^T att_dst (the attention dot products then ride along the lin GEMM as
 * two extra output columns) and v = W_edge^T att_edge (the edge term becomes an edge_dim-long dot). */
size_t nsc_gat_folded_floats(const NscGatModel *m);
int    nsc_gat_fold_weights(const NscGatModel *m, float *folded, void *stream);

size_t nsc_gat_workspace_bytes(const NscGatModel *m, int32_t n_nodes);

/* Inference forward (BatchNorm running statistics, no dropout) == model.eval(); model(data).
 *   x          (n_nodes, in_dim) float32
 *   edge_attr  (E, edge_dim) float32 indexed by g->eid, or NULL (then the edge term is skipped,
 *              as model.py:126-129 does when data has no edge_attr)
 *   out        (n_nodes, out_dim) float32
 *   alpha_out  nullable (n_layers, nnz) attention coefficients (forward_with_attention)
 * Inputs that are not finite go where the reference's arithmetic takes them: every ReLU of the path keeps a NaN
 * (torch.relu; fmaxf would turn it into 0 and the row into one that looks real).
 *   A row of x with a NaN entry makes EVERY output column of EVERY node within n_layers hops of it NaN.  Hops follow the
 *   edge direction (source -> target); the node itself is in the ball (its own loop), a node without edges is its own
 *   ball.  Layer l's attention coefficients are NaN for every entry of a target within l + 1 hops (one NaN logit makes the
 *   target's whole softmax NaN: the maxima drop a NaN, expf(NaN - max) brings it back).  The rows of all other nodes, and
 *   the coefficients of all other targets, are the bits of the same call without that entry, in every kernel set.
 *   A +-inf entry does the same: the input projection makes the row +-inf in every column whose weight for that entry is
 *   not zero, the ReLU keeps the +inf and zeroes the -inf, and the first lin GEMM adds +inf and -inf to NaN.  (Only a row
 *   that reaches a ReLU as -inf in every column comes out as zeros, as in the reference; a weight row of one sign does that.)
 *   A NaN in edge_attr is a NaN logit of the edge's target in every layer (its own loop carries the mean of the incoming
 *   attributes as well): that target's coefficients are NaN from layer 0 on and the output is NaN within n_layers - 1 hops
 *   of the target.  An infinite attribute makes the logit +-inf, layer by layer by the sign of the attribute's folded
 *   weight v = W_edge^T att_edge: a logit of +inf is NaN coefficients as above (expf(inf - inf)), a logit of -inf is a
 *   weight of exactly 0 in that layer and no NaN.
 *   The poisoned row itself is NaN also without any layer, through the residual (x or residual_proj(x)).
 * tests/gnn_edge_cases.py holds the cases, tests/test_gnn_edges_gpu.py runs them in every kernel set. */
int nsc_gat_forward(const NscGatModel *m, const NscGraph *g, const float *x, const float *edge_attr,
                    float *out, float *alpha_out, void *ws, size_t ws_bytes, void *stream);
/* Same forward with launch options.  NSC_GAT_CORESIDENT: every kernel uses 0 bytes of LDS and <= 56 VGPRs, so two waves
 * of it fit on a SIMD beside a resident nsc_encode_clouds grid (up to five encoder workgroups per CU: 5 x 27.9 KB of LDS,
 * 5 x 80 VGPRs): issue it on its own stream to run the GNN of batch k under the encoders of batches k+1, k+2.
 * NSC_GAT_SHARED_B (with NSC_GAT_CORESIDENT): the GEMMs use 64 x 64 tiles that share the weight block through 10 KB of LDS
 * (two such workgroups fit in the 20 KB a CU has left beside five encoder workgroups): fewer LDS-pipe and L1 operations
 * per FLOP.  NSC_GAT_LDS_TILED (alone): the stand-alone forward with the round-2 GEMMs (register-staged 16/32/64 x 64 tiles)
 * instead of the default LDS-DMA, wave-specialised GEMM of round 3 -- kept for A/B measurements and as the fall-back when
 * that kernel cannot run (unaligned operands, LDS opt-in refused).  Bit-identical output in every combination. */
#define NSC_GAT_CORESIDENT 1u
#define NSC_GAT_SHARED_B 2u
#define NSC_GAT_LDS_TILED 4u
/* NSC_GAT_GENERIC: ignore NscGraph.band_entries -- every layer as lin GEMM + gat_aggregate_kernel (what irregular graphs
 * always get).  Bit-identical to the banded path; for A/B measurements and the parity tests. */
#define NSC_GAT_GENERIC 8u
int nsc_gat_forward_ex(const NscGatModel *m, const NscGraph *g, const float *x, const float *edge_attr,
                       float *out, float *alpha_out, void *ws, size_t ws_bytes, uint32_t flags, void *stream);
/* Which tile the default (LDS-DMA) GEMM takes for C[M,N] = A[M,K] B[N,K]^T -- host function, no device work: rows and
 * columns of a workgroup tile, its LDS bytes and the number of workgroups (a grid of at most 256 is one round on the
 * 256 CUs).  Returns NSC_OK, or NSC_EINVAL for non-positive sizes / K not a multiple of 16. */
int nsc_gat_gemm_tile(int32_t M, int32_t N, int32_t K, int32_t *tile_rows, int32_t *tile_cols, int32_t *lds_bytes,
                      int64_t *workgroups);

/* ------------------------------------------------------------------------------------------
 * Training step of the GNN (BASELINE configs[4]): model.train(); emb = model(graph);
 * loss = TripletLoss(emb[a], emb[p], emb[n]); loss.backward()
 * (reference src/gnn/trainer.py:205-213, TripletLoss :44-68; model.py:96-153 in train mode:
 * BatchNorm batch statistics, feature dropout :137, GATConv attention dropout).
 * ------------------------------------------------------------------------------------------ */
typedef struct NscGatTrainCfg {
    float    dropout_p;            /* model.py:38; 0 for parity runs (the reference never seeds its RNG) */
    float    bn_momentum;          /* 0.1 (nn.BatchNorm1d default) */
    uint64_t seed;                 /* counter-based dropout masks: same seed in forward and backward */
    int32_t  update_running_stats; /* 1: running_mean / running_var of the model are updated IN PLACE */
    int32_t  accumulate_grads;     /* nsc_gat_backward: 1 = every PARAMETER gradient is ADDED to what its NscGatGrads buffer
                                      holds (gradient accumulation over the batches of an optimizer step, trainer.py:207-221,
                                      without a pass of axpy kernels behind the backward); 0 = overwritten.  grads->x is
                                      always overwritten */
    const uint64_t *seed_dev;      /* nullable DEVICE pointer: when set, the kernels read the seed from this word at run
                                      time instead of `seed` -- a training step captured into a hipGraph then replays
                                      with a fresh mask per step (the caller rewrites the word between replays) */
} NscGatTrainCfg;

typedef struct NscGatGradLayer {   /* device buffers shaped like the NscGatLayer parameters; overwritten, or added to
                                      with NscGatTrainCfg.accumulate_grads */
    float *lin_w, *att_src, *att_dst, *lin_edge_w, *att_edge, *bias, *bn_w, *bn_b;
} NscGatGradLayer;

typedef struct NscGatGrads {
    float *in_w, *in_b, *in_bn_w, *in_bn_b, *out_w, *out_b;
    float *x;                      /* nullable: gradient w.r.t. the input features (n_nodes, in_dim) */
    float *res_w, *res_b;          /* residual_proj (model.py:91-94): required iff residual && in_dim != out_dim */
    NscGatGradLayer layers[NSC_GAT_MAX_LAYERS];
} NscGatGrads;

size_t nsc_graph_transpose_workspace_bytes(int32_t n_nodes);
int    nsc_graph_transpose(const NscGraph *g, int32_t *t_ptr, int32_t *t_entry, int32_t *tgt, void *ws,
                           size_t ws_bytes, void *stream);

/* The workspace holds the activations the forward saves for the backward: pass the SAME buffer (and
 * cfg) to nsc_gat_backward.  residual && in_dim != out_dim trains residual_proj (m->res_w / res_b).
 * Inputs that are not finite (see nsc_gat_forward): in train mode the batch statistics of the first BatchNorm behind the
 * poisoned value are NaN, so EVERY row of out is NaN, nsc_triplet_loss over it is NaN (relu keeps a NaN), the running
 * statistics updated in place take the NaN as nn.BatchNorm1d's would, and the backward passes NaN gradients on (the ReLU's
 * derivative passes the gradient where its input is NaN, as torch's does).  Nothing stays in the workspace: the next call
 * with finite inputs writes everything it reads. */
size_t nsc_gat_train_workspace_bytes(const NscGatModel *m, const NscGraph *g);
int    nsc_gat_forward_train(const NscGatModel *m, const NscGraph *g, const float *x, const float *edge_attr,
                             const NscGatTrainCfg *cfg, float *out, void *ws, size_t ws_bytes, void *stream);
int    nsc_gat_backward(const NscGatModel *m, const NscGraph *g, const float *x, const float *edge_attr,
                        const NscGatTrainCfg *cfg, const float *grad_out, const NscGatGrads *grads, void *ws,
                        size_t ws_bytes, void *stream);

/* TripletLoss forward (+ backward when grad_emb != NULL): loss = scale * mean_t relu(|a-p|^2 - |a-n|^2 + margin);
 * grad_emb (n_nodes, dim) is zeroed and receives d loss / d emb.  Indices follow embeddings[idx] (trainer.py:207-209):
 * values in [-n_nodes, 0) wrap; a triplet with an index outside [-n_nodes, n_nodes) reads and writes nothing and turns
 * the loss into NaN (the reference raises IndexError there). */
size_t nsc_triplet_workspace_bytes(int32_t n_triplets);
int    nsc_triplet_loss(const float *emb, const int64_t *anchors, const int64_t *positives,
                        const int64_t *negatives, int32_t n_triplets, int32_t n_nodes, int32_t dim,
                        float margin, float scale, float *loss, float *grad_emb, void *ws, size_t ws_bytes,
                        void *stream);

/* ------------------------------------------------------------------------------------------
 * Stage-1 retrieval: 1-D Wasserstein distance = L1 of CDFs, top-k.
 * Replaces wasserstein_distance_batch_torch / _matrix_torch (reference src/retrieval/wasserstein.py
 * :134-172, :232-273), WassersteinRetriever.query (:328-384) and the spatial filter of
 * TwoStageRetrieval._global_retrieval (src/retrieval/two_stage_retrieval.py:145-202).
 * ------------------------------------------------------------------------------------------ */
/* cdf[i] = cumsum(normalised hists[i]);  divide_plain = 1: h / sum (query form, wasserstein.py:153-155),
 * 0: h / (sum + eps) (database / matrix form, :158-163); rows with sum <= eps stay unnormalised. */
int nsc_w1_cdf(const float *hists, int32_t n, int32_t dim, float eps, int32_t divide_plain, float *cdf,
               void *stream);
/* dist (Q, N): W1 of every query CDF against every database row (raw histograms, normalised on the
 * fly).  db_pos (N,3) / q_pos (Q,3) nullable: pairs closer than min_dist get +inf (spatial filter). */
int nsc_w1_distances(const float *db, int32_t N, int32_t dim, float eps, const float *q_cdf, int32_t Q,
                     const float *db_pos, const float *q_pos, float min_dist, float *dist, void *stream);
/* Same distances against a database whose rows are already CDFs (= nsc_w1_cdf(db, divide_plain = 0), kept by
 * WassersteinRetriever next to the raw histograms so that the normalise + prefix-sum is not redone per query).
 * dim % 4 == 0, both matrices 16-byte aligned.  Q <= 4: HBM-streaming kernel (rows read once, queries in
 * registers); Q > 4: register-tiled |a-b| kernel (VALU-bound). */
int nsc_w1_distances_cdf(const float *db_cdf, int32_t N, int32_t dim, const float *q_cdf, int32_t Q,
                         const float *db_pos, const float *q_pos, float min_dist, float *dist, void *stream);
/* idx/val (Q, k): the k smallest entries of each row of dist, ascending, ties to the smaller index
 * (k <= 256 and ceil(N/2048)*k <= 4096). */
size_t nsc_topk_workspace_bytes(int32_t Q, int32_t N, int32_t k);
int nsc_topk_smallest(const float *dist, int32_t Q, int32_t N, int32_t k, int64_t *idx, float *val,
                      void *ws, size_t ws_bytes, void *stream);

/* Stage 1 over QUANTISED descriptors.  quantized (n, dim) uint16, 1 <= dim <= 1024.  A row is
 * canonical iff its bins sum to exactly 65535 (summed in 32 bits; what nsc_quantize_descriptors emits for every
 * histogram with a positive sum).  cdf[i][k] = sum_{j <= k} quantized[i][j] as uint16 for canonical rows, a row of
 * zeros otherwise; canonical[i] = 1 / 0.  One launch, no workspace. */
int nsc_w1q_cdf(const uint16_t *quantized, int32_t n, int32_t dim, uint16_t *cdf, uint8_t *canonical, void *stream);
/* dist (Q, N) = float(sum_k |db_cdf[i][k] - q_cdf[q][k]|) / 65535.0f: the integer sum is exact in uint32, so a
 * distance does not depend on the kernel or the batch; it is W1 between the dequantised histograms.  +inf where the
 * database row or the query row is not canonical, or (both position arrays given) the pair is closer than min_dist,
 * as in nsc_w1_distances.  dim % 8 == 0 and both CDF matrices 16-byte aligned: Q <= 4 HBM-streaming kernel (2 dim
 * bytes per row, read once), Q > 4 register-tiled kernel; any other dim or alignment: a wave-per-row kernel with
 * scalar loads.  One launch, no workspace.  Feed dist to nsc_topk_smallest. */
int nsc_w1q_distances(const uint16_t *db_cdf, const uint8_t *db_canonical, int32_t N, int32_t dim,
                      const uint16_t *q_cdf, const uint8_t *q_canonical, int32_t Q,
                      const float *db_pos, const float *q_pos, float min_dist, float *dist, void *stream);

/* Hard-negative triplet mining inside ONE sequence: replaces
 * TripletMiner._mine_sequence_triplets / _select_hard_negative (reference src/gnn/triplet_miner.py
 * :141-229, :314-359).  Members of the sequence are rows 0..n-1 in temporal order. */
typedef struct NscMineParams {
    double   positive_distance_max;   /* 5.0   triplet_miner.py:43 */
    double   negative_distance_min;   /* 10.0  :45 */
    double   negative_distance_max;   /* 50.0  :46 */
    int32_t  positive_temporal_min;   /* 30    :44 */
    int32_t  negative_temporal_min;   /* 30    :47 */
    int32_t  strategy;                /* 0 = "hard" (argmin W1, :347-350), 1 = "random" (:333-334),
                                       * 2 = "semi-hard" (candidate at position len // 2 of the W1 order, :352-357) */
    int32_t  triplets_per_anchor;
    uint64_t seed;                    /* counter-based choice of the positive (np.random.choice in the reference) */
} NscMineParams;
/* positions (n,3) float64 translations; cdf (n,dim) = nsc_w1_cdf(descriptors, divide_plain = 1);
 * out_pos / out_neg (n, triplets_per_anchor) local row indices or -1 when the anchor has no positive
 * or no negative candidate; counts (n,2) = [#positive, #negative candidates]. */
int nsc_mine_triplets(const double *positions, const float *cdf, int32_t n, int32_t dim,
                      const NscMineParams *mp, int32_t *out_pos, int32_t *out_neg, int32_t *counts,
                      void *stream);
/* The same with a workspace: strategy 2 keeps one row of candidate distances per anchor (n * n floats). */
size_t nsc_mine_workspace_bytes(int32_t n, int32_t strategy);
int nsc_mine_triplets_ws(const double *positions, const float *cdf, int32_t n, int32_t dim,
                         const NscMineParams *mp, int32_t *out_pos, int32_t *out_neg, int32_t *counts,
                         void *ws, size_t ws_bytes, void *stream);

/* Validation recall for loop closure: the pieces of
 * GNNTrainer._compute_recall_loop_closure (reference src/gnn/trainer.py:306-387).
 *   nsc_revisit_queries: first_revisit[i] = first j >= i + skip_frames with |p_i - p_j| < thr, else -1  (:342-348)
 *   nsc_pairwise_l2    : dist (Q,n) = euclidean embedding distance of query q to every c with |c - q| > skip_frames,
 *                        +inf for the excluded temporal neighbours (:355-370); feed to nsc_topk_smallest
 *   nsc_recall_rank    : rank[q] = 1-based position of the first of the k nearest candidates that lies within
 *                        thr of the query pose, 0 if none (:376-383)  ->  recall@K = mean(0 < rank <= K) */
int nsc_revisit_queries(const double *positions, int32_t n, int32_t skip_frames, double distance_threshold,
                        int32_t *first_revisit, void *stream);
int nsc_pairwise_l2(const float *emb, const int32_t *query_idx, int32_t Q, int32_t n, int32_t dim,
                    int32_t skip_frames, float *dist, void *stream);
int nsc_recall_rank(const double *positions, const int32_t *query_idx, const int64_t *topk_idx, int32_t Q,
                    int32_t k, double distance_threshold, int32_t *rank, void *stream);

/* ------------------------------------------------------------------------------------------
 * Keyframe-side helpers either side of the path.
 * ------------------------------------------------------------------------------------------ */
/* Offline temporal graph: replaces the O(N*M) Python loop of build_graph_from_keyframes_batch (reference
 * src/keyframe/graph_manager.py:515-596).  Edges [i, i+off], off = -M/2..M/2 except 0, node-major in ascending
 * offset, then two edges [q,m],[m,q] per loop closure (loops (n_loops,2), already range-checked by the host
 * as :555).  poses (n,4,4) float64 row-major, nullable -> no edge_attr.  edge_index (2,E) int64,
 * edge_attr (E,2) float32 = [log1p(|t_i - t_j|)/5, arccos(clip((clip(tr(R_j R_i^T),-1,3)-1)/2,-1,1))/pi]. */
int64_t nsc_chain_graph_num_edges(int32_t n_nodes, int32_t temporal_neighbors, int32_t n_loops);
int nsc_build_chain_graph(const double *poses, int32_t n_nodes, int32_t temporal_neighbors, const int64_t *loops,
                          int32_t n_loops, int64_t *edge_index, float *edge_attr, void *stream);

/* 16-bit descriptor wire format: HistogramQuantizer.quantize / dequantize (reference
 * src/encoding/quantization.py:131-191) for n histograms of dim bins (dim <= 4096; the float32 sums follow
 * numpy's pairwise order bit for bit), and CompressedDescriptor.to_bytes / from_bytes (:41-110) generalised
 * from 50 bins to dim: records of nsc_record_bytes(dim) = 2*dim + 120 bytes (220 for 50 bins):
 * [dim x u16][pose 7 x f32][timestamp f64][keyframe id u32][20-byte hash][60 zero bytes]. */
int nsc_quantize_descriptors(const float *hist, int32_t n, int32_t dim, float eps, uint16_t *quantized, void *stream);
int nsc_dequantize_descriptors(const uint16_t *quantized, int32_t n, int32_t dim, float eps, float *hist, void *stream);
size_t nsc_record_bytes(int32_t dim);
int nsc_pack_records(const uint16_t *quantized, const float *pose7, const double *timestamps,
                     const uint32_t *keyframe_ids, const uint8_t *hashes, int32_t n, int32_t dim,
                     uint8_t *records, void *stream);
int nsc_unpack_records(const uint8_t *records, int32_t n, int32_t dim, uint16_t *quantized, float *pose7,
                       double *timestamps, uint32_t *keyframe_ids, uint8_t *hashes, void *stream);

/* Geometric-novelty test of the keyframe selector: compute_overlap (reference src/data/pose_utils.py:323-389,
 * called from keyframe/criteria.py:123) after its random down-sampling (:340-347, done by the caller) for
 * n_pairs cloud pairs at once.  points1/points2: packed float32 rows of stride_floats (3 or 4) columns,
 * offsets (n_pairs+1) int64; transforms (n_pairs,4,4) float64 maps cloud 1 into the frame of cloud 2.
 * max_pair_points = host-known max over pairs of n1+n2 (<= 12288; the reference caps each cloud at 5000).
 * counts (n_pairs,3) = [|voxels 1|, |voxels 2|, |intersection|], iou (n_pairs) float64. */
size_t nsc_voxel_overlap_workspace_bytes(int64_t total_points1, int64_t total_points2);
int nsc_voxel_overlap(const float *points1, const int64_t *offsets1, const float *points2, const int64_t *offsets2,
                      int32_t n_pairs, int64_t total_points1, int64_t total_points2, int64_t max_pair_points,
                      int32_t stride_floats, const double *transforms, double voxel_size, int32_t *counts,
                      double *iou, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Stage 2 of loop closing: batched Generalized-ICP verification (reference GeometricVerifier,
 * src/retrieval/geometric_verification.py:48-203, after Open3D 0.18's registration_generalized_icp).
 * The algorithm -- voxel down-sampling in first-row order, k-NN plane covariances, Gauss-Newton rounds
 * with Open3D's convergence test, the information matrix -- is defined in
 * neural-spectral-codec_amd/retrieval/geometric_verification.py and INTEGRATION.md section 2.
 *
 * Pair p registers source rows [source_offsets[p], source_offsets[p+1]) onto target rows
 * [target_offsets[p], target_offsets[p+1]): packed float32 rows of stride_floats (3 or 4) columns, xyz first;
 * rows with a non-finite xyz are dropped.  Offsets are (n_pairs+1) int64.  init_transforms and transforms are
 * (n_pairs,4,4) float64 row-major and map source coordinates into the target frame (they may alias).
 * Out: fitness_rmse (n_pairs,2) float64, corr_iterations (n_pairs,2) int64 = [n_correspondences, Gauss-Newton
 * updates applied], information (n_pairs,6,6) float64 (rotation first).
 * Voxel keys are 21 bits per axis from the cloud's min bound: a cloud must span fewer than 2^21 voxels per axis.
 * Centroids are exact sums in int64 units of 2^-24 m: |coordinate| x rows per voxel must stay below 2^39 m.
 * ------------------------------------------------------------------------------------------ */
#define NSC_GICP_MAX_KNN 32
/* Largest batch of one call (the launches index clouds or pairs by gridDim.y <= 65 535): a larger count returns
 * NSC_EUNSUPPORTED before anything is launched and the caller splits the batch -- pairs and clouds are independent
 * of the rest of their batch, so splitting changes no result.  The *_workspace_bytes queries accept any count. */
#define NSC_GICP_MAX_PAIRS          32767   /* nsc_gicp_register: 2 clouds per pair                  */
#define NSC_GICP_MAX_CLOUDS         65535   /* nsc_gicp_prepare                                       */
#define NSC_GICP_MAX_PREPARED_PAIRS 65535   /* nsc_gicp_register_prepared                             */

typedef struct NscGicpParams {
    double  voxel_size;                   /* 0.5   voxel_down_sample edge, > 0                        */
    double  max_correspondence_distance;  /* 1.0   correspondence radius, > 0                          */
    double  relative_fitness;             /* 1e-6  stop when |d fitness| < this ...                    */
    double  relative_rmse;                /* 1e-6  ... and |d rmse| < this                              */
    double  epsilon;                      /* 1e-3  plane regularisation U diag(1,1,eps) U^T, > 0        */
    int32_t max_iteration;                /* 30    Gauss-Newton updates at most, >= 0                   */
    int32_t covariance_knn;               /* 20    neighbours per covariance, self included, 1..32      */
} NscGicpParams;

/* Optional stage outputs (any pointer may be NULL).  points (total_source+total_target, 3) float64 and
 * covariances (same rows, 6: xx xy xz yy yz zz) float64: the down-sampled rows of source cloud p start at row
 * source_offsets[p], those of target cloud p at total_source_points + target_offsets[p]; counts (2*n_pairs)
 * int64 = down-sampled rows of source 0..P-1 then target 0..P-1; system0 (n_pairs,29) float64 = the sums at
 * init_transforms: JtWJ upper triangle row-major (21), JtW d (6), n_correspondences, Sum |d|^2.  The kernels
 * work in these buffers in place of the workspace regions they name. */
typedef struct NscGicpStages {
    double  *points;
    int64_t *counts;
    double  *covariances;
    double  *system0;
} NscGicpStages;

void   nsc_gicp_default_params(NscGicpParams *p);
size_t nsc_gicp_workspace_bytes(int32_t n_pairs, int64_t total_source_points, int64_t total_target_points);
int    nsc_gicp_register(const float *source_points, const int64_t *source_offsets, const float *target_points,
                         const int64_t *target_offsets, int32_t n_pairs, int64_t total_source_points,
                         int64_t total_target_points, int32_t stride_floats, const NscGicpParams *p,
                         const double *init_transforms, double *transforms, double *fitness_rmse,
                         int64_t *corr_iterations, double *information, const NscGicpStages *stages, void *ws,
                         size_t ws_bytes, void *stream);

/* A store of prepared clouds.  A cloud's down-sampled points, covariances, min bound and voxel index depend only
 * on the cloud and on voxel_size, covariance_knn and epsilon: nsc_gicp_prepare computes them once per cloud and
 * appends them to a store, nsc_gicp_register_prepared registers pairs given as cloud indices into stores.  Its
 * results are bitwise those of nsc_gicp_register on the same raw clouds with the same parameters.
 * The struct is a host struct of device pointers; the caller owns the memory and the host counts.  Cloud c owns
 * rows [row_offsets[c], row_offsets[c+1]) of points / covariances (rows as in NscGicpStages) and index slots
 * [slot_offsets[c], slot_offsets[c+1]) (2 per row: packed voxel key + 1, 0 = empty; row within the cloud);
 * bounds[c] = the cloud's min bound (x, y, z, 0).  After nsc_gicp_prepare of B clouds the caller reads
 * row_offsets[n_clouds + B] and slot_offsets[n_clouds + B] back into n_rows and n_slots and adds B to n_clouds. */
typedef struct NscGicpCloudSet {
    double   voxel_size, epsilon;         /* parameters the clouds were prepared with                        */
    int32_t  covariance_knn, n_clouds;    /* ... and the clouds present                                      */
    int64_t  n_rows, n_slots;             /* rows / index slots present                                      */
    int64_t  cap_clouds, cap_rows, cap_slots;
    int64_t  *row_offsets, *slot_offsets; /* (cap_clouds + 1) int64                                          */
    double   *bounds;                     /* (cap_clouds, 4) float64                                         */
    double   *points, *covariances;       /* (cap_rows, 3), (cap_rows, 6) float64                            */
    uint64_t *slots;                      /* (cap_slots, 2)                                                  */
} NscGicpCloudSet;

/* Prepare clouds [offsets[c], offsets[c+1]) of points (as nsc_gicp_register's) and append them to set as clouds
 * set->n_clouds .. + n_clouds - 1.  p's voxel_size, covariance_knn and epsilon must equal the set's (NSC_EINVAL);
 * the set must have room for every input row being a voxel of its own: n_clouds + n_clouds(batch) <= cap_clouds,
 * n_rows + total_points <= cap_rows, n_slots + 2 total_points <= cap_slots (else NSC_EWORKSPACE). */
size_t nsc_gicp_prepare_workspace_bytes(int32_t n_clouds, int64_t total_points);
int    nsc_gicp_prepare(const float *points, const int64_t *offsets, int32_t n_clouds, int64_t total_points,
                        int32_t stride_floats, const NscGicpParams *p, const NscGicpCloudSet *set, void *ws,
                        size_t ws_bytes, void *stream);
/* Register cloud source_ids[i] of sources onto cloud target_ids[i] of targets (device int64 ids; the two sets may be
 * one).  p's voxel_size, covariance_knn and epsilon must equal both sets'; the correspondence radius and the
 * iteration and convergence parameters are free.  Outputs as nsc_gicp_register's; system0 (optional) as
 * NscGicpStages.system0.  A pair with an id outside [0, n_clouds) of its set gets NaN transform, fitness, rmse,
 * information and system0, n_correspondences -1 and 0 iterations; nothing of the sets is read for it.
 * Launches 1 + 2 (max_iteration + 1) kernels and nothing else. */
size_t nsc_gicp_register_prepared_workspace_bytes(int32_t n_pairs);
int    nsc_gicp_register_prepared(const NscGicpCloudSet *sources, const NscGicpCloudSet *targets,
                                  const int64_t *source_ids, const int64_t *target_ids, int32_t n_pairs,
                                  const NscGicpParams *p, const double *init_transforms, double *transforms,
                                  double *fitness_rmse, int64_t *corr_iterations, double *information,
                                  double *system0, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Yaw initial guess for stage 2: the circular column shift that best aligns two interpolated range images
 * (the encoder's `interpolated` output, (rows, 360) float32, 1 <= rows <= 64, the same rows for both).
 * In float64: a = Iq - its row means, b = Ic - its row means,
 *   score[s] = sum_r sum_c a[r,c] * b[r,(c - s) mod 360],  s = 0 .. 359;
 * shift = the s of the largest score, ties to the smaller s, 0 when that score is not > 0 (flat or empty images);
 * peak = score[shift]; runner_up = the largest score among shifts more than NSC_YAW_GUARD_BINS bins from shift
 * (circularly).  The guess is the rotation Rz(-shift degrees, wrapped to (-180, 180]) with zero translation,
 * mapping query into candidate coordinates: exactly the identity for shift 0.
 *
 * Pair i aligns image ids_q[i] of images_q (n_q, rows, 360) with image ids_c[i] of images_c (n_c, rows, 360); the
 * two arrays may be one.  Out: shift (n_pairs) int32, scores (n_pairs, 2) float64 = [peak, runner_up],
 * init_transforms (n_pairs, 4, 4) float64 row-major.  A pair with an id outside its array gets shift -1, NaN scores
 * and the identity; nothing of the images is read for it.  A pair in which either image holds a NaN or +-inf pixel
 * in its rows has NaN row means and so 360 NaN scores: it gets shift 0, the identity bit for bit, peak NaN and
 * runner_up NaN (shift 0, not -1: the ids were valid).  Finite images, denormal or up to FLT_MAX, have finite
 * scores.  One kernel launch and nothing else, no workspace; a pair's outputs depend on its two images alone.
 * A launch holds at most 2^32 - 1 threads, 768 per pair: more than NSC_YAW_MAX_PAIRS pairs return
 * NSC_EUNSUPPORTED before anything is launched and the caller splits the batch.
 * ------------------------------------------------------------------------------------------ */
#define NSC_YAW_GUARD_BINS 10
#define NSC_YAW_MAX_PAIRS  4194304
int nsc_yaw_align(const float *images_q, int32_t n_q, const float *images_c, int32_t n_c, const int64_t *ids_q,
                  const int64_t *ids_c, int32_t n_pairs, int32_t rows, int32_t *shift, double *scores,
                  double *init_transforms, void *stream);

/* ------------------------------------------------------------------------------------------
 * Planar initial guess (yaw, x, y) for stage 2: a joint vote over yaw hypotheses and planar translation bins, cast
 * by the structure rows of two prepared clouds.  It covers what the yaw guess cannot: a revisit that is also
 * translated by more than GICP's basin (about 1 m), e.g. in the other lane.
 *
 * Inputs: cloud source_ids[i] of sources and cloud target_ids[i] of targets (rows of an NscGicpCloudSet: points
 * (m,3), covariances (m,6), both float64; the two sets may be one), and a table yaw_cs (n_yaw, 2) float64 of
 * hypotheses (cos theta_h, sin theta_h).
 * Structure row: (1 - C_zz) < normal_z2_max * (1 - epsilon), epsilon being the row's set's.  The stored covariance
 * is I - (1 - epsilon) n n^T, so this is n_z^2 < normal_z2_max: a surface steeper than 30 degrees from horizontal at
 * the default.  A row with fewer than 3 neighbours has the x axis as its normal and is a structure row.
 * Rows taken: the source's structure rows whose row index within the cloud is divisible by source_stride, and all
 * structure rows of the target.
 * Vote, for hypothesis h = (c, s), source row a and target row b, in float64, every operation rounded on its own
 * (no fused multiply-add), inv_cell = 1 / cell computed once:
 *   xr = c a.x - s a.y;  yr = s a.x + c a.y
 *   bx = floor((b.x - xr) inv_cell + 0.5);  by = floor((b.y - yr) inv_cell + 0.5)
 *   one vote for (h, bx, by) iff |bx| <= half_bins and |by| <= half_bins and |b.z - a.z| <= z_window (inclusive;
 *   compared as float64, before any conversion to an integer).
 * Per hypothesis: peak_h = its largest count, bin_h = that bin, ties to the smaller flat index
 *   (bx + half_bins) (2 half_bins + 1) + (by + half_bins).
 * Per pair: best = the h of the largest peak_h, ties to the smaller h; peak = peak_best; runner_up = the largest
 * peak_h among hypotheses more than guard indices from best, circularly over n_yaw (0 if there are none).  The
 * guess [Rz from (c, s) of best | (bx cell, by cell, 0)] maps query (source) into candidate (target) coordinates.
 * With peak = 0 (no structure rows, nothing inside the window) best = (-1, 0, 0) and the guess is the identity.  A
 * pair with an id outside its set gets best = (-1, 0, 0), peak = runner_up = -1, counts 0 and the identity; nothing
 * of the sets is read for it.
 *
 * Out: best (n_pairs,3) int32 = [h, bx, by]; scores (n_pairs,2) int32 = [peak, runner_up]; counts (n_pairs,2) int32
 * = [source rows taken, target structure rows]; init_transforms (n_pairs,4,4) float64 row-major.  Optional stage
 * outputs (either pointer may be NULL): yaw_peaks (n_pairs, n_yaw, 2) int32 = [peak_h, flat bin_h] and votes
 * (n_pairs, n_yaw, 2 half_bins + 1, 2 half_bins + 1) int32, all zero for a pair with an invalid id.
 *
 * Counts: a target row is the centroid of one voxel of the target set's voxel_size, so one source row casts at most
 * K = (floor(cell / voxel_size) + 2)^2 (floor(2 z_window / voxel_size) + 2) votes into one bin (36 at the defaults),
 * and never more than the target has rows.  A cloud has at most its set's n_rows rows: the call returns
 * NSC_EUNSUPPORTED, before anything is launched, unless sources->n_rows * min(K, targets->n_rows) <= 2^31 - 1 (59
 * million source rows in the set at the defaults).  Pairs are indexed by a grid dimension: more than
 * NSC_PLANAR_MAX_PAIRS pairs return NSC_EUNSUPPORTED and the caller splits the batch; a pair's outputs depend on its
 * two clouds, the table and the parameters alone.
 * Three kernel launches (resolve ids and count rows; vote, one workgroup per hypothesis and pair; reduce over the
 * hypotheses) and nothing else.
 * ------------------------------------------------------------------------------------------ */
#define NSC_PLANAR_MAX_HALF_BINS 32
#define NSC_PLANAR_MAX_PAIRS     65535

typedef struct NscPlanarParams {
    double  cell;            /* 0.5   bin edge (m), > 0                                            */
    double  z_window;        /* 0.5   a pair votes iff |dz| <= this (m), >= 0                      */
    double  normal_z2_max;   /* 0.25  structure rows have n_z^2 below this                         */
    int32_t half_bins;       /* 24    bins -half_bins .. half_bins per axis; 1 .. 32               */
    int32_t source_stride;   /* 2     source rows taken: row index % source_stride == 0; >= 1      */
    int32_t guard;           /* 5     hypotheses either side of best the runner-up skips; >= 0     */
} NscPlanarParams;

typedef struct NscPlanarStages {   /* optional stage outputs (any pointer may be NULL) */
    int32_t *yaw_peaks;
    int32_t *votes;
} NscPlanarStages;

void   nsc_planar_default_params(NscPlanarParams *p);
size_t nsc_planar_align_workspace_bytes(int32_t n_pairs, int32_t n_yaw);
int    nsc_planar_align(const NscGicpCloudSet *sources, const NscGicpCloudSet *targets, const int64_t *source_ids,
                        const int64_t *target_ids, int32_t n_pairs, const double *yaw_cs, int32_t n_yaw,
                        const NscPlanarParams *params, int32_t *best, int32_t *scores, int32_t *counts,
                        double *init_transforms, const NscPlanarStages *stages, void *ws, size_t ws_bytes,
                        void *stream);

/* ------------------------------------------------------------------------------------------
 * Pose-graph optimisation: the consumer of stage 2's `transform` and `information`.  Odometry edges and verified loop
 * closures in, corrected poses out (restated in tests/posegraph_restatement.py).  Float64.
 *
 * Problem.  poses (n_poses,4,4) row-major, sensor to world, rigid: rows 0..2 are read and written, row 3 is copied.
 * edge_ij (n_edges,2) int64.  measurements (n_edges,4,4) with Z ~ X_i^-1 X_j: stage 2's `transform` for i = candidate,
 * j = query.  information (n_edges,6,6), rotation first (the order of nsc_gicp_register's `information`), symmetric
 * positive definite; only the upper triangle is read.  fixed (n_poses) uint8: a pose with fixed != 0 is never changed.
 * An edge with i == j or an index outside [0, n_poses) is skipped: it contributes nothing and is counted.  A pose no
 * counted edge touches, or whose damped diagonal block is not positive definite (a pivot of its Cholesky factor that is
 * not positive and finite: NaN and infinite entries count), is not moved either.
 *
 * Residual of an edge.  D = Z^-1 X_i^-1 X_j;  r = [Log_SO3(R_D); t_D];  cost F = sum r^T Omega r.
 *   Log_SO3(R): v = vee(R - R^T) / 2, theta = atan2(|v|, (tr R - 1) / 2), phi = v theta / |v|, and phi = v for
 *   |v| < 1e-12.  Residual rotations beyond 179 degrees are out of scope: the axis is lost where |v| -> 0 at pi.
 * Update.  X_k <- [R_k Exp(phi_k) | t_k + R_k rho_k] for delta_k = (phi_k, rho_k); Exp is Rodrigues' formula, with
 *   its series below |phi|^2 = 1e-8.
 * Jacobians, exact for this residual and this update.  With A = X_i^-1 X_j and B = blockdiag(Jr^-1(r_phi), R_D):
 *   J_j = B,  J_i = -B Ad(A^-1),  Ad(R, t) = [[R, 0], [[t]x R, R]],
 *   Jr^-1(phi) = I + [phi]x / 2 + c [phi]x^2,  c = 1 / theta^2 - (1 + cos theta) / (2 theta sin theta), and
 *   c = 1/12 + theta^2 / 720 for theta < 1e-4.
 * System.  g = sum J^T Omega r (half the gradient of F), H = sum J^T Omega J.
 *
 * Solver.  Levenberg-Marquardt with Marquardt scaling.  Per outer iteration, at damping lambda:
 *   (H + lambda diag H) delta = -g over the poses that move, delta = 0 elsewhere, by preconditioned conjugate
 *   gradients from delta = 0.  Preconditioner: the Cholesky factor of each node's 6 x 6 diagonal block of the damped
 *   matrix.  An inner iteration is counted once its p.Ap is formed; the loop ends at |r| <= pcg_tolerance |g|, at
 *   max_pcg_iterations, or when p.Ap or r.z is not positive (an iteration whose p.Ap is not positive applies no step
 *   and is counted like any other).  No inner iteration runs for g = 0.
 *   Candidate poses = the update by delta; F_c = their cost; step = |delta| over all poses.
 *   F_c < F: accepted, the candidate replaces the poses, lambda <- max(lambda / lambda_factor, lambda_min), and the
 *     optimiser stops (converged) when F - F_c < relative_cost F.
 *   Otherwise: rejected, lambda <- lambda lambda_factor.
 *   Either way it stops (converged) when step < min_step, and (capped) after max_iteration outer iterations.
 *
 * Robust kernels (nsc_posegraph_linearize_robust, nsc_posegraph_optimize_robust).  One kernel id per call and a width
 * per edge, edge_scale (n_edges) float64, in units of sqrt(chi^2).  With s = r^T Omega r and c the edge's width:
 *   kernel                               rho(s)                                w(s) = rho'(s)
 *   NSC_POSEGRAPH_KERNEL_NONE            s                                     1
 *   NSC_POSEGRAPH_KERNEL_HUBER           s for s <= c^2, else 2 c sqrt(s) - c^2  1 for s <= c^2, else c / sqrt(s)
 *   NSC_POSEGRAPH_KERNEL_CAUCHY          c^2 log1p(s / c^2)                    1 / (1 + s / c^2)
 *   NSC_POSEGRAPH_KERNEL_GEMAN_MCCLURE   c^2 s / (c^2 + s)                     (c^2 / (c^2 + s))^2
 *   Geman-McClure is the closed form of a switchable constraint, min over sigma of sigma^2 s + c^2 (1 - sigma)^2, with
 *   w = sigma^2: what dynamic covariance scaling computes.
 *   F = sum rho(s_e),  g = sum w J^T Omega r,  H = sum w J^T Omega J: iteratively reweighted least squares, first order
 *   (no second-order correction of H, as in g2o).  s is formed with Omega as given; then Omega is scaled by w.
 *   Accept, reject, lambda and the stopping rules are those above, applied to the robust F; cost0, cost and
 *   cost_history are robust costs.
 *   An edge is quadratic, rho = s and w = 1 exactly, when edge_scale is NULL, when its width is not finite and positive
 *   (<= 0, NaN, +-inf; likewise a width whose square underflows to 0 or overflows), or when s <= 0.  So odometry edges
 *   with width 0 stay quadratic.  With kernel NONE, or with quadratic edges only, every output has the bits of the
 *   plain entry points.  A kernel id outside 0..3 is NSC_EINVAL.  A skipped edge reports chi2 = 0 and weight = 0.
 *
 * Determinism.  Node quantities are gathered over a node's incident edges in ascending edge index; scalars (the cost
 * too: a node sums the edges it is the first end of) are summed as fixed-shape partials over the nodes; no floating-
 * point atomics.  Two calls on the same inputs agree bit for bit, and where the skipped edges stand among the others
 * changes no bit of any other output.
 * Launches.  A sequence that depends on n_poses > 0, n_edges > 0, poses_out == poses, max_iteration and
 * max_pcg_iterations alone: 5 (lists) + 1 (copy, unless aliased) + 3 + max_iteration (8 + 4 max_pcg_iterations) + 1,
 * at most NSC_POSEGRAPH_MAX_LAUNCHES in the loop (else NSC_EUNSUPPORTED), + 1 at the end when nsc_posegraph_optimize_robust
 * is given edge_chi2 or edge_weight and n_edges > 0.  Kernels of a finished phase return at once.
 * No host synchronisation, no memset or memcpy nodes: the call can be captured.
 *
 * Two-level preconditioner (nsc_posegraph_optimize_coarse; restated, sparse, in tests/posegraph_coarse_restatement.py).
 * Block-Jacobi PCG needs of the order of n_poses inner iterations for the long wavelengths of a trajectory, which are
 * what a closure corrects.  With coarse_block = L >= 2, pose k belongs to aggregate a(k) = k / L; there are
 * n_a = ceil(n_poses / L) aggregates, the last one possibly ragged.
 *   Prolongation P (6 n_poses, 6 n_a): the block of a free pose k in column a(k) is Ad(X_k^-1 X_ref), X_ref the first
 *     pose of the aggregate at the linearisation point, fixed or not: a coarse 6-vector is a rigid motion of the whole
 *     aggregate in the frame of X_ref.  Rows of poses that are not free (fixed, without a counted edge, or with a
 *     damped diagonal block that is not positive definite) are zero.
 *   A = H + lambda diag H on the free poses, with the robust weights as assembled;  A_c = P^T A P, and the identity
 *     block for an aggregate without a free pose.
 *   Preconditioner  M^-1 r = B^-1 r + P A_c^-1 P^T r,  B^-1 the per-node Cholesky solve above: additive, symmetric
 *     positive definite, so PCG, its stopping rule and the count of inner iterations are those above.
 *   A_c is factored by Cholesky and inverted explicitly once per outer step.  A pivot that is not positive and finite
 *     leaves that outer step with B^-1 alone; coarse_stats counts such steps.
 *   Aggregation by index assumes that consecutive indices are neighbours in the graph, which holds for a trajectory.
 *     On any other graph M^-1 is still symmetric positive definite, only less useful.
 *   At most NSC_POSEGRAPH_MAX_AGGREGATES aggregates (A_c is at most 768 x 768), else NSC_EUNSUPPORTED.
 *   Launches: 5 (lists) + 1 (copy, unless aliased) + 3 + max_iteration (14 + 5 max_pcg_iterations) + 1, the loop's share
 *     at most NSC_POSEGRAPH_MAX_LAUNCHES, + 1 for edge_chi2 or edge_weight: a sequence that depends on the parameters,
 *     n_poses > 0, n_edges > 0, the aliasing and coarse_block alone.  The determinism and capture rules above hold.
 * ------------------------------------------------------------------------------------------ */
#define NSC_POSEGRAPH_MAX_EDGES    1073741823   /* list entries are 2 edge + side in int32 */
#define NSC_POSEGRAPH_MAX_LAUNCHES 1000000
#define NSC_POSEGRAPH_MAX_AGGREGATES 128        /* A_c is (6 x this)^2 float64: 768 x 768 */
#define NSC_POSEGRAPH_STATS        10

#define NSC_POSEGRAPH_KERNEL_NONE           0
#define NSC_POSEGRAPH_KERNEL_HUBER          1
#define NSC_POSEGRAPH_KERNEL_CAUCHY         2
#define NSC_POSEGRAPH_KERNEL_GEMAN_MCCLURE  3

typedef struct NscPoseGraphParams {
    int32_t max_iteration;        /* 20     outer iterations at most, >= 0                                  */
    int32_t max_pcg_iterations;   /* 100    inner iterations per outer iteration at most, >= 0              */
    double  pcg_tolerance;        /* 1e-6   inner loop ends at |r| <= this |g|, >= 0                        */
    double  lambda0;              /* 1e-4   initial damping, > 0                                            */
    double  lambda_min;           /* 1e-9   floor of the damping, > 0                                       */
    double  lambda_factor;        /* 10     lambda is divided (accept) or multiplied (reject) by this, > 1  */
    double  relative_cost;        /* 1e-9   stop when an accepted step gains less than this times F, >= 0   */
    double  min_step;             /* 1e-9   stop when |delta| is below this, >= 0                           */
} NscPoseGraphParams;

void   nsc_posegraph_default_params(NscPoseGraphParams *p);
/* Bytes of workspace for a graph of this size; params may be NULL (the layout does not depend on the caps). */
size_t nsc_posegraph_workspace_bytes(int32_t n_poses, int32_t n_edges, const NscPoseGraphParams *params);

/* The system at `poses`: residuals (n_edges,6), zero rows for skipped edges; cost (1) = F; gradient (n_poses,6) = g;
 * blocks (n_poses,21) = upper triangle, row-major, of each pose's diagonal block of H; skipped (1) int64.  Fixed poses
 * play no part here: every pose gets its row.  The outputs of the counted edges do not depend on the skipped ones. */
int    nsc_posegraph_linearize(const double *poses, int32_t n_poses, const int64_t *edge_ij, const double *measurements,
                               const double *information, int32_t n_edges, double *residuals, double *cost,
                               double *gradient, double *blocks, int64_t *skipped, void *ws, size_t ws_bytes,
                               void *stream);
/* The same with a robust kernel: nsc_posegraph_linearize is this call with kernel NONE and NULLs.  edge_scale
 * (n_edges), nullable.  residuals stay unweighted; cost = sum rho(s), gradient and blocks carry w.  weights (n_edges),
 * nullable: w of every edge, 0 for a skipped one. */
int    nsc_posegraph_linearize_robust(const double *poses, int32_t n_poses, const int64_t *edge_ij,
                                      const double *measurements, const double *information, int32_t n_edges,
                                      double *residuals, double *cost, double *gradient, double *blocks,
                                      int64_t *skipped, void *ws, size_t ws_bytes, void *stream, int32_t kernel,
                                      const double *edge_scale, double *weights);

/* stats[...] of nsc_posegraph_optimize, in the order of the list below */
#define NSC_POSEGRAPH_STAT_ITERATIONS      0
#define NSC_POSEGRAPH_STAT_ACCEPTED        1
#define NSC_POSEGRAPH_STAT_REJECTED        2
#define NSC_POSEGRAPH_STAT_PCG_ITERATIONS  3
#define NSC_POSEGRAPH_STAT_INITIAL_COST    4
#define NSC_POSEGRAPH_STAT_FINAL_COST      5
#define NSC_POSEGRAPH_STAT_LAMBDA          6
#define NSC_POSEGRAPH_STAT_SKIPPED         7
#define NSC_POSEGRAPH_STAT_CONVERGED       8
#define NSC_POSEGRAPH_STAT_STEP            9

/* poses_out (n_poses,4,4) may alias poses.  stats (NSC_POSEGRAPH_STATS) float64 = [outer iterations done, accepted,
 * rejected, inner iterations in total, initial cost, final cost, final lambda, skipped edges, 1 = stopped by a
 * criterion / 0 = capped at max_iteration, |delta| of the last outer iteration].  cost_history (max_iteration + 1):
 * entry 0 the initial cost, entry k the cost after outer iteration k (unchanged by a rejected step), entries past the
 * last iteration the final cost.  step0 (n_poses,6), nullable: the first delta (not written when max_iteration = 0).
 * With max_iteration = 0 poses_out = poses bit for bit and the costs are those of the input. */
int    nsc_posegraph_optimize(const double *poses, int32_t n_poses, const int64_t *edge_ij, const double *measurements,
                              const double *information, int32_t n_edges, const uint8_t *fixed,
                              const NscPoseGraphParams *params, double *poses_out, double *stats, double *cost_history,
                              double *step0, void *ws, size_t ws_bytes, void *stream);
/* The same with a robust kernel: nsc_posegraph_optimize is this call with kernel NONE and NULLs.  edge_scale (n_edges),
 * nullable.  edge_chi2 (n_edges) = r^T Omega r and edge_weight (n_edges) = w of every edge at poses_out, zeros for a
 * skipped edge; both nullable, one more launch when either is given: what a caller decides by which closures to drop. */
int    nsc_posegraph_optimize_robust(const double *poses, int32_t n_poses, const int64_t *edge_ij,
                                     const double *measurements, const double *information, int32_t n_edges,
                                     const uint8_t *fixed, const NscPoseGraphParams *params, double *poses_out,
                                     double *stats, double *cost_history, double *step0, void *ws, size_t ws_bytes,
                                     void *stream, int32_t kernel, const double *edge_scale, double *edge_chi2,
                                     double *edge_weight);

/* Bytes of workspace for nsc_posegraph_optimize_coarse.  coarse_block = 0: nsc_posegraph_workspace_bytes.  0 for a
 * negative size, for coarse_block < 0 or == 1, and for more than NSC_POSEGRAPH_MAX_AGGREGATES aggregates. */
size_t nsc_posegraph_coarse_workspace_bytes(int32_t n_poses, int32_t n_edges, int32_t coarse_block);
/* nsc_posegraph_optimize_robust with the two-level preconditioner above.  coarse_block = 0 is the robust call, launch for
 * launch and bit for bit (then the workspace of nsc_posegraph_workspace_bytes suffices); 1 or a negative value is
 * NSC_EINVAL; more than NSC_POSEGRAPH_MAX_AGGREGATES aggregates is NSC_EUNSUPPORTED.  coarse_stats (2) float64, nullable:
 * [aggregates, outer steps whose coarse factor failed and that ran with the block-Jacobi preconditioner alone]. */
int    nsc_posegraph_optimize_coarse(const double *poses, int32_t n_poses, const int64_t *edge_ij,
                                     const double *measurements, const double *information, int32_t n_edges,
                                     const uint8_t *fixed, const NscPoseGraphParams *params, double *poses_out,
                                     double *stats, double *cost_history, double *step0, void *ws, size_t ws_bytes,
                                     void *stream, int32_t kernel, const double *edge_scale, double *edge_chi2,
                                     double *edge_weight, int32_t coarse_block, double *coarse_stats);

/* ------------------------------------------------------------------------------------------
 * Marginal covariances of selected poses (nsc_posegraph_covariance; restated in tests/posegraph_cov_restatement.py):
 * how uncertain pose j is relative to pose i, which is what a Mahalanobis gate on a loop closure needs.
 *
 * System.  The one nsc_posegraph_linearize_robust forms at `poses`: H = sum w J^T Omega J with `kernel` and `edge_scale`
 *   as they are there, so a closure whose weight is ~ 0 adds no information.  The damping is lambda = 0.  The free poses
 *   are those of the optimiser: not fixed, at least one counted edge, and a positive definite (here undamped) diagonal
 *   block.  Sigma is the inverse of H restricted to the free poses, and zero elsewhere: the covariance of the right
 *   perturbations delta_k in X_k Exp(delta_k), rotation first, in the gauge the fixed poses set.
 * Output.  For the selected poses nodes[0 .. n_nodes): joint (n_nodes,n_nodes,6,6), joint[a,b] the block (nodes[a],
 *   nodes[b]) of Sigma, taken from the six columns solved for nodes[b]: H x = e_{6 nodes[b] + c}, joint[a,b][:,c] =
 *   x[nodes[a]].  It is not symmetrised.  residual (n_nodes,6) = |r| of each column at exit (|b| = 1: the relative
 *   residual); iterations (n_nodes,6) int32; stats (NSC_POSEGRAPH_COV_STATS) int64 = [skipped edges, selected indices
 *   outside [0, n_poses), selected poses that are not free, columns whose residual is above pcg_tolerance].
 *   An index outside [0, n_poses) gives zero rows and columns and is counted; a pose that is not free has b = 0: its
 *   columns run no iteration and are zero.  Duplicates are allowed.  At most NSC_POSEGRAPH_MAX_COV_NODES poses.
 * Solver.  Each of the R = 6 n_nodes columns is a preconditioned conjugate gradient iteration of its own, from x = 0,
 *   with the rules of the optimiser's inner loop: it ends at r.r <= pcg_tolerance^2 b.b, when p.Ap or r.z is not
 *   positive, or at max_pcg_iterations; its alpha, beta, stop and count are its own, and a column that has stopped
 *   changes nothing.  Of params only max_pcg_iterations and pcg_tolerance are used; all of it must be valid.
 *   Preconditioner: block-Jacobi, and with coarse_block = L >= 2 the two-level one above (lambda = 0), its coarse matrix
 *   factored once.  coarse_stats (2), nullable: [aggregates, 1 when that factor failed and B^-1 ran alone].
 *   A column's bits do not depend on the other selected poses nor on its place among them, and two calls agree bitwise.
 * Launches.  5 (lists; 2 without edges) + 1 (the final gather), and for n_poses > 0 and n_nodes > 0 in between
 *   2 (linearise and pack, n_edges > 0) + 1 (assemble) + 2 (start) + max_pcg_iterations x 3 (n_edges > 0), or with
 *   coarse_block 2 + 1 + 5 (coarse matrix) + 4 (start) + max_pcg_iterations x 4: a sequence that depends on the parameters,
 *   n_poses > 0, n_edges > 0, n_nodes and coarse_block alone; 18 + 4 max_pcg_iterations (3 without the coarse space) above
 *   NSC_POSEGRAPH_MAX_LAUNCHES is NSC_EUNSUPPORTED.  No host synchronisation, no memset or memcpy nodes: the call can be
 *   captured.
 * ------------------------------------------------------------------------------------------ */
#define NSC_POSEGRAPH_MAX_COV_NODES 64
#define NSC_POSEGRAPH_COV_TILE      16          /* consecutive poses one wave of the covariance kernels walks */
#define NSC_POSEGRAPH_COV_STATS     4
#define NSC_POSEGRAPH_COV_STAT_SKIPPED        0
#define NSC_POSEGRAPH_COV_STAT_OUTSIDE        1
#define NSC_POSEGRAPH_COV_STAT_NOT_FREE       2
#define NSC_POSEGRAPH_COV_STAT_NOT_CONVERGED  3

/* Bytes of workspace for nsc_posegraph_covariance; 0 for arguments the call would refuse: a negative size, n_nodes above
 * NSC_POSEGRAPH_MAX_COV_NODES, coarse_block < 0 or == 1, more than NSC_POSEGRAPH_MAX_AGGREGATES aggregates. */
size_t nsc_posegraph_covariance_workspace_bytes(int32_t n_poses, int32_t n_edges, int32_t n_nodes, int32_t coarse_block);
/* nodes (n_nodes) int64 on the device.  NSC_EINVAL for a null or negative argument, a kernel id outside 0..3, invalid
 * params, coarse_block < 0 or == 1; NSC_EUNSUPPORTED for n_nodes above NSC_POSEGRAPH_MAX_COV_NODES, too many aggregates or
 * launches; NSC_EWORKSPACE for a workspace that is missing or too small: all before anything is launched. */
int    nsc_posegraph_covariance(const double *poses, int32_t n_poses, const int64_t *edge_ij, const double *measurements,
                                const double *information, int32_t n_edges, const uint8_t *fixed,
                                const NscPoseGraphParams *params, const int64_t *nodes, int32_t n_nodes, double *joint,
                                double *residual, int32_t *iterations, int64_t *stats, void *ws, size_t ws_bytes,
                                void *stream, int32_t kernel, const double *edge_scale, int32_t coarse_block,
                                double *coarse_stats);

/* ------------------------------------------------------------------------------------------
 * Global voxel map (nsc_map_build; restated in tests/map_restatement.py): the keyframe clouds placed by the optimised
 * poses and merged into one cloud, one point per occupied voxel.  The consumer of nsc_posegraph_optimize's poses.
 *
 * Input.  n_clouds clouds packed as rows, cloud c the rows [offsets[c], offsets[c+1]) of `points`; offsets (n_clouds+1)
 *   int64.  dtype NSC_MAP_DTYPE_F32: float32 rows of stride_floats 3 or 4, xyz first (as nsc_gicp_register takes them);
 *   NSC_MAP_DTYPE_F64: float64 rows of 3 (the `points` of an NscGicpCloudSet; stride_floats = 3).  poses (n_poses,4,4)
 *   float64 row-major, sensor to world, rows 0..2 are read.  pose_ids (n_clouds) int64, or NULL: cloud c uses pose c.
 *   A cloud whose id lies outside [0, n_poses) is left out and its rows are counted; -1 is the way to leave a cloud out.
 *   A row of [0, total_rows) that lies in no cloud of `offsets` is counted with them.
 * A row, in float64, every operation rounded on its own:  w_a = ((R_a0 x + R_a1 y) + R_a2 z) + t_a.  A row whose xyz or w
 *   is not finite is dropped and counted.  k_a = floor((w_a - origin_a) / voxel_size) + 2^20; a row with a k_a outside
 *   [0, 2^21) is dropped and counted, not clamped (at 0.5 m: +-524 km).  key = k_x | k_y << 21 | k_z << 42.
 * Per voxel: count; first_row, the smallest index into the packed rows among the voxel's rows; first_cloud and
 *   last_cloud, the min and max cloud index among them; exact int64 sums of rint(w_a 2^24);
 *   centroid_a = (sum_a / 2^24) / count.  |coordinate| x rows per voxel must stay below 2^39 m.
 * Output, voxels in ascending first_row: out_points (max_voxels,3) float64, info (max_voxels,4) int64 = [count,
 *   first_row, first_cloud, last_cloud], keys (max_voxels) int64, stats (NSC_MAP_STATS) int64.  Entries past
 *   stats[NSC_MAP_STAT_WRITTEN] are not defined.
 * Capacity.  The table has 2 max_voxels slots and lives in the workspace.  A probe visits every slot once at most; a
 *   row that finds neither its key nor an empty slot is counted as unplaced and nothing else happens.  `found` counts the
 *   voxels in the table.  The result is complete when found <= max_voxels and unplaced = 0; with unplaced = 0 and
 *   found > max_voxels the written voxels are the first max_voxels of the complete result.  Nothing is written outside
 *   the buffers.
 * Determinism.  Integer atomics only: two calls agree bit for bit, and the order of the clouds changes only the order
 *   of the output voxels and first_row.
 * Launches.  6 kernels (clear, insert, mark first rows, count them per word and tile, scan the tiles, write) whose grids
 *   depend on total_rows and max_voxels alone; no host synchronisation, no memset or memcpy nodes: the call can be
 *   captured.
 * ------------------------------------------------------------------------------------------ */
#define NSC_MAP_DTYPE_F32 0
#define NSC_MAP_DTYPE_F64 1
#define NSC_MAP_STATS              7
#define NSC_MAP_STAT_FOUND         0    /* voxels in the table                                   */
#define NSC_MAP_STAT_WRITTEN       1    /* min(found, max_voxels)                                */
#define NSC_MAP_STAT_USED          2    /* rows summed into a voxel                              */
#define NSC_MAP_STAT_NOT_FINITE    3    /* rows with a non-finite xyz or world coordinate        */
#define NSC_MAP_STAT_OUTSIDE       4    /* rows outside the 2^21 voxels per axis                 */
#define NSC_MAP_STAT_NO_POSE       5    /* rows of clouds without a pose (and rows of no cloud)  */
#define NSC_MAP_STAT_UNPLACED      6    /* rows that found the table full                        */
/* the shapes of the launches, for tests that walk their boundaries */
#define NSC_MAP_TILE_ROWS      4096     /* rows whose first-row marks one wave counts: the compaction's tile  */
#define NSC_MAP_SCAN_THREADS   256      /* the one workgroup that scans the tile counts; a thread takes
                                           ceil(tiles / this) consecutive tiles                              */
#define NSC_MAP_INSERT_ROWS    512      /* consecutive rows a workgroup of the insert pass takes at a time   */
#define NSC_MAP_INSERT_BLOCKS  2048     /* its workgroups at most: beyond INSERT_ROWS x this rows they wrap  */
#define NSC_MAP_MAX_VOXELS     (1LL << 36)
#define NSC_MAP_MAX_ROWS       (1LL << 46)

typedef struct NscMapParams {
    double voxel_size;              /* 0.5    voxel edge (m), finite and positive */
    double origin[3];               /* 0,0,0  world point where voxel (2^20, 2^20, 2^20) begins */
} NscMapParams;

void   nsc_map_default_params(NscMapParams *p);
/* Bytes of workspace for nsc_map_build: 128 per voxel of max_voxels (the table) and about 0.2 per row; monotone in both;
 * 0 for arguments the call would refuse (a negative size, max_voxels above NSC_MAP_MAX_VOXELS, total_rows above
 * NSC_MAP_MAX_ROWS). */
size_t nsc_map_workspace_bytes(int64_t total_rows, int64_t max_voxels);
/* NSC_EINVAL for a null or negative argument, a dtype other than the two above, stride_floats not 3 or 4, float64 with a
 * stride other than 3, a voxel_size not finite and positive, an origin not finite; NSC_EUNSUPPORTED for max_voxels above
 * NSC_MAP_MAX_VOXELS or total_rows above NSC_MAP_MAX_ROWS; NSC_EWORKSPACE for a workspace that is missing or too small:
 * all before anything is launched.  points may be NULL with total_rows = 0, poses with n_poses = 0, and out_points, info, keys with max_voxels = 0. */
int    nsc_map_build(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_clouds,
                     int64_t total_rows, const double *poses, int32_t n_poses, const int64_t *pose_ids,
                     const NscMapParams *params, int64_t max_voxels, double *out_points, int64_t *info, int64_t *keys,
                     int64_t *stats, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Map localisation (restated in tests/map_localize_restatement.py): a map that keeps a normal distribution per voxel and
 * a table that outlives the call (nsc_map_build_dist), and the registration of scans against it (nsc_map_register).
 *
 * nsc_map_build_dist.  Inputs, validation, row placement, keys, the seven stats, the order of the output voxels (ascending
 *   first row), the table of 2 max_voxels slots and its full-table rule, `info` and `keys` are nsc_map_build's, bit for bit.
 * Per voxel, in place of the coordinate sums, exact integer moments of the position inside the voxel:
 *   f_a = (w_a - origin_a) / voxel_size, k_a = floor(f_a), u_a = f_a - k_a (exact), q_a = rint(u_a 2^16) - 2^15;
 *   three int64 sums of q_a and six of q_a q_b (xx xy xz yy yz zz).  |q| <= 2^15, so the sums are exact for fewer than
 *   2^31 rows per voxel.
 * Output for the first min(found, max_voxels) voxels:
 *   voxels (max_voxels,16) float64, one 128-byte record per voxel:
 *     [0..2]   mean_a = origin_a + ((k_a + 1/2) + (sum q_a / n) / 2^16) voxel_size
 *     [3..8]   C_ab = ((sum q_a q_b) / n - (sum q_a / n)(sum q_b / n)) (voxel_size / 2^16)^2, xx xy xz yy yz zz
 *     [9..14]  information U diag(1 / l'_i) U^T of C = U diag(l_i) U^T (cyclic Jacobi),
 *              l'_i = max(l_i, eigen_ratio l_max, sigma_floor^2)
 *     [15]     1.0 when the voxel is usable (count >= min_points and every entry above finite), else 0.0
 *   moments (max_voxels,9) int64, or NULL: the raw sums, q first.
 *   index (2 max_voxels,2) uint64, every entry written: (key + 1, place) at the table's own slot positions, (0, ~0) for
 *     an empty slot.  A lookup walks the probe sequence the insertion walked: slot mix(key) % (2 max_voxels), then the
 *     next, wrapping, until the key or an empty slot.  A voxel whose place is >= max_voxels keeps its key (probes
 *     continue past it) with place ~0: not usable.  Which of two keys that meet in a slot claims it is free, so two
 *     builds may keep a key in different slots; what a lookup finds is the same.
 * Launches: the six of nsc_map_build in the same shapes; no host synchronisation, no memset or memcpy nodes.
 *
 * nsc_map_insert_dist (restated in tests/map_insert_restatement.py).  Rows added to a kept map without a rebuild.
 *   Given the kept tensors of a nsc_map_build_dist call with the same max_voxels, grid and dist -- voxels, index, info,
 *   keys, moments, stats -- and `cursor` (2) int64 = [rows taken so far, clouds taken so far] (after a build: its
 *   total_rows and n_clouds), and n_clouds new clouds in the formats of nsc_map_build: after the call the kept tensors
 *   hold, bit for bit, what nsc_map_build_dist produces over the old clouds followed by the new ones with the same
 *   max_voxels: voxels, info, keys, moments, the seven stats, and the index read as a mapping key -> place.  The order of
 *   the voxels too: new voxels take the places after stats[NSC_MAP_STAT_WRITTEN], in ascending first row.  A record is
 *   a function of count, moments and key alone, so adding rows is integer arithmetic and one evaluation of that function.
 *   This holds while the voxels found stay at most 2 max_voxels, the table's slots; with a full table, which rows are
 *   unplaced is as free as it is in the build.
 * Numbers.  Row `r` of the call is row cursor[0] + r of the map and cloud `c` cloud cursor[1] + c: these enter first_row,
 *   first_cloud and last_cloud.  The pose of cloud c is poses[pose_ids[c]], or poses[c]: indexed within the call.
 * Stats accumulate: rows without a pose (id outside [0, n_poses), rows of no cloud), rows not finite, rows outside the
 *   grid, rows that find all 2 max_voxels slots keyed (unplaced), rows used.  A new voxel whose place would be >=
 *   max_voxels keeps its key in the index with place ~0, as in the build; its rows count as used, found counts it,
 *   written = min(found, max_voxels).
 * Cursor.  The last launch advances cursor by (total_rows, n_clouds): a captured call can be replayed with new contents
 *   in the same buffers, and every replay is a further insertion.
 * Cost.  Work and workspace scale with total_rows, not with max_voxels: no launch walks the slots or the records, and
 *   only voxels that received a row have their record computed again.
 * Launches.  NSC_MAP_INSERT_LAUNCHES kernels (clear the call's bitmap and counters; claim: probe the kept index, 64-bit
 *   CAS for new keys, the smallest row of each new voxel; mark those rows; count; scan; assign places to new voxels;
 *   accumulate: integer atomics on info and moments, a list of the places reached; refresh their records, fold the new
 *   voxels into the stats, advance the cursor) whose grids depend on total_rows alone, on the caller's stream; integer
 *   atomics only; no host synchronisation, no memset or memcpy nodes.  While a call runs, bits 61 and 62 of an index
 *   place word are in use; they are clear when it ends.
 *
 * nsc_map_remove_dist and nsc_map_replace_dist (restated in tests/map_replace_restatement.py).  Rows taken out of a kept
 *   map, and clouds moved from one pose to another, in work proportional to their rows.
 * Matched removal.  A removal is matched when every row it is given was added earlier by a build or an insertion, with
 *   the same bits of xyz and of the pose: the row then has the key, the position inside its voxel and the nine integers it
 *   had then.  It finds its voxel by the build's probe (a lookup that claims nothing) and subtracts: -1 on the count, the
 *   negated integers on the moments.
 * Contract.  Let M be a kept map after any sequence of builds, insertions, matched removals and replacements, and B
 *   nsc_map_build_dist over the rows that remain, in any cloud order, with the same grid, dist and max_voxels, while the
 *   voxels found stay at most max_voxels in both.  Then
 *   - for every key of B, M holds the key with a place, and info[place][0] (the count), moments[place] and the 16 doubles
 *     of voxels[place] equal B's by bits;
 *   - every other keyed slot of M is an emptied voxel: count 0, nine zero moments, a record of 16 zeros (written as
 *     zeros: the record function is not evaluated for a count of 0), hence not usable.  It keeps its key, its slot and its
 *     place (places are never reused; nsc_map_rehash_dist moves the map without them).  A later insertion into it adds to the zeros and makes its record again:
 *     the voxel keeps its place and info[place][1], the row that first made it, and info[place][2] and info[place][3]
 *     become the min and the max of the bounds it kept and the numbers of the clouds now added.  An insertion into an
 *     inconsistent voxel adds to its integers in the same way, and the record stays zero while the count is below 1;
 *   - nsc_map_register and nsc_map_register_robust (every kernel, 1 and 7 voxels) against M give the bits they give
 *     against B: an emptied voxel is found and skipped by its usable flag exactly where B's lookup finds nothing;
 *   - info[:,1] is the row that made the voxel; info[:,2] and info[:,3] become a lower and an upper bound of the cloud
 *     numbers present, no longer attained; keys and the order of places never change for voxels that exist.
 * removed (NSC_MAP_REMOVE_STATS int64), written, not accumulated, by every call: rows removed, rows not finite, rows
 *   outside the grid, rows without a pose, rows missing (their voxel is not in the index, or it has place ~0), voxels
 *   touched, voxels emptied, voxels inconsistent.  In a replacement these are the removal half's: a voxel it emptied may
 *   be filled again by the insertion half.
 * Inconsistent voxels.  A touched voxel whose count ends below 0, or at 0 with a moment that is not 0, is inconsistent:
 *   it gets the zero record and keeps its integers (so adding the rows again restores it), and it is not counted as
 *   emptied.  The call writes nowhere but to the places the index names.  An unmatched removal that leaves a positive
 *   count cannot be detected: the voxel then has the record of integers no set of rows gives.
 * Kept stats.  stats[NSC_MAP_STAT_USED] goes down by the rows removed; a removal changes no other entry (found and
 *   written keep counting emptied voxels).
 * Replacement.  clouds, old_poses and new_poses (both (n_poses,4,4)) and one pose_ids: a cloud with an id is removed
 *   under old_poses[id] and inserted under new_poses[id]; a cloud with id -1 (or past n_poses) is left alone.  The
 *   insertion half is nsc_map_insert_dist's with two differences: rows and clouds are numbered from first_row and
 *   first_cloud, so that a store's numbering survives, and no cursor is read or advanced; and what became of the call's rows
 *   goes into placed (NSC_MAP_STATS int64 in the layout of stats: new voxels, written after the call, used, not finite,
 *   outside, no pose, unplaced), of which only found, written, used and unplaced are folded into the kept stats, so that
 *   leaving clouds out does not inflate the map's rows without pose.  New voxels take the places after
 *   stats[NSC_MAP_STAT_WRITTEN] in ascending call row; overflow and the full-table rule are the insertion's.  With
 *   first_row and first_cloud equal to the cursor a replacement leaves what nsc_map_remove_dist followed by
 *   nsc_map_insert_dist leaves, bit for bit, apart from the cursor.
 * Launches.  NSC_MAP_REMOVE_LAUNCHES kernels (clear the call's counters; rows: lookup, integer atomics, the list of
 *   places reached; refresh: their records, the counters) and NSC_MAP_REPLACE_LAUNCHES (one clear for both halves, the
 *   removal's rows and refresh, the insertion's seven passes).  No launch walks the slots or the records; the grids depend
 *   on total_rows alone; integer atomics only, so two identical sequences of calls leave identical bits in every kept
 *   tensor (the index as a mapping) and a cloud's effect does not depend on what else is in the call; no host
 *   synchronisation, no memset or memcpy nodes.  Bits 61 and 62 of a place word may be in use during a call and are clear
 *   at its end.
 *
 * nsc_map_rehash_dist (restated in tests/map_rehash_restatement.py).  A kept map moved to another capacity, with or
 *   without its emptied voxels, in work proportional to its voxels: a record is a function of count, moments and key
 *   alone, so the integers and the record are copied by bits (the record function is not evaluated) and a new index is
 *   keyed by the build's probe.  No row is read: the clouds need not exist any more.  The source -- voxels, info, keys,
 *   moments, stats, cursor of capacity max_voxels -- is read only (its index is not needed: `keys` holds the key of every
 *   place); the destination tensors of capacity new_max_voxels are other memory, and both maps exist while the call runs.
 *   moments and new_moments are both given or both NULL (a map that is not insertable can be moved too), cursor and
 *   new_cursor likewise.
 * Kept voxels.  Place p < stats[NSC_MAP_STAT_WRITTEN] is dropped iff keep_emptied == 0, its count is 0 and its nine moments
 *   are 0 (with moments == NULL the count alone decides).  Every other place is kept, an inconsistent one too (count below
 *   0, or 0 with a moment left): it keeps its integers and its zero record, so adding the rows again still restores it.
 * Order.  Kept voxels take the new places 0, 1, ... in ascending old place: ascending first_row survives.
 * new_place (max_voxels) int64, every entry written: the new place of old place p; -1 where p was dropped, where
 *   p >= written, and where the new place would be >= new_max_voxels.  For side data a caller keeps by place.
 * tile_base (n_tiles + 1) int64, n_tiles = ceil(max_voxels / NSC_MAP_TILE_ROWS), every entry written: entry t is the number
 *   of kept places before old place t NSC_MAP_TILE_ROWS, the last entry the number kept.  The call's own scan, and an
 *   output.
 * Copies.  For every kept voxel with new place q < new_max_voxels: the 16 doubles of its record, its 4 info entries, its 9
 *   moments and its key, by bits.  Entries of the destination at and past new_stats[NSC_MAP_STAT_WRITTEN] are not defined.
 * new_index (2 new_max_voxels,2) uint64, every entry written: (0, ~0) for an empty slot; each kept key claimed along the
 *   build's probe sequence (mix(key) % (2 new_max_voxels), linear, 64-bit CAS) with its new place, or with place ~0 when
 *   q >= new_max_voxels (the build's overflow rule).  Bits 61 and 62 of every place word are clear.  Which of two keys
 *   that meet in a slot claims it is free, as in the build; the index read as a mapping key -> place is fixed.  With
 *   kept <= new_max_voxels the destination is, bit for bit, what nsc_map_build_dist gives at new_max_voxels over the rows
 *   the source holds (voxels, info, keys, moments, stats, the index as a mapping), provided the source never overflowed.
 * new_stats: found = voxels kept, written = min(kept, new_max_voxels), entries 2 to 6 copied.  new_cursor: copied.
 * rehashed (NSC_MAP_REHASH_STATS int64), written, not accumulated: voxels kept; voxels dropped as emptied; source keys
 *   without a place (found - written of the source: they never had a record and cannot be carried); inconsistent voxels
 *   kept; kept voxels without a place in the destination (kept - written); kept voxels that found all 2 new_max_voxels
 *   slots keyed (only with kept > 2 new_max_voxels; which voxels these are is as free as in a full build table).
 * No workspace: the two arrays the call needs beyond the map, new_place and tile_base, are typed outputs with a defined
 *   value in every element.
 * Launches.  NSC_MAP_REHASH_LAUNCHES kernels (clear new_index and rehashed; count the kept places per tile; scan: one
 *   workgroup, also the stats, the cursor and rehashed; move: per tile the kept places listed in LDS, the four tensors
 *   copied as flat ranges, the keys claimed) whose grids depend on max_voxels and new_max_voxels alone; the source's
 *   stats are read on the device; integer atomics only; no host synchronisation, no memset or memcpy nodes.
 *
 * nsc_map_register.  n_scans scans packed as rows in the formats of nsc_map_build, offsets (n_scans+1) int64,
 *   init_transforms (n_scans,4,4) float64 row-major, scan to world.  The target is `voxels` and `index` of a
 *   nsc_map_build_dist call with the same max_voxels and grid (params).
 * Cost, point to distribution:  E(T) = sum_i d_i^T Omega_v d_i,  d_i = T p_i - mean_v,  v the voxel that contains
 *   T p_i = ((R_a0 x + R_a1 y) + R_a2 z) + t_a: its key is looked up in the index, no neighbour and no radius.  A row
 *   contributes when its voxel is in the index and usable; rows that are not finite, outside the grid or without a usable
 *   voxel do not.
 * Rounds, as nsc_gicp_register_prepared: one set-up kernel, then max_iteration + 1 pairs of linearize
 *   (NSC_MAP_REGISTER_BLOCKS x n_scans workgroups of 256; J = [-[T p]x | I]; per workgroup a float64 slab of 21 J^T Omega J
 *   + 6 J^T Omega d + n_corr + sum |d|^2 + sum d^T Omega d, reduced in a fixed shape) and finalize (one workgroup per scan:
 *   slabs summed in order, fitness = n_corr / rows, rmse = sqrt(sum |d|^2 / n_corr), Open3D's convergence test on both,
 *   6x6 Cholesky, T <- dT T with dT = [Rz Ry Rx of the three angles | translation]; without correspondences or a
 *   positive-definite system T stays: a pivot counts only above 3.9e-9 of its diagonal term, so a scan of one row or of
 *   collinear rows keeps its pose).  1 + 2 (max_iteration + 1) launches and nothing else; a finished scan's later
 *   rounds are no-ops.
 * Outputs per scan: transforms (4,4), fitness_rmse (2), cost = sum d^T Omega d at the result, corr_iterations (2) int64,
 *   information (6,6) = sum J^T Omega J at the result, rotation first; system0 (n_scans,NSC_MAP_REGISTER_SYSTEM) or
 *   NULL: the sums at init_transforms, the first 29 laid out as NscGicpStages.system0, then sum d^T Omega d.
 * A scan whose init_transform is not finite gets NaN outputs, n_corr -1 and 0 iterations; none of its rows is read.
 * Results are bitwise reproducible and a scan's results do not depend on what else is in the batch.
 *
 * nsc_map_register_robust (restated in tests/map_robust_restatement.py).  nsc_map_register with robust weights and face-
 *   neighbour voxels; with NSC_MAP_KERNEL_NONE and neighbours = 1 it is nsc_map_register, bit for bit.  Float64:
 * Voxels.  For a row with w = T p finite and inside the grid the candidates are its own voxel k and, with neighbours = 7,
 *   k -+ e_x, k -+ e_y, k -+ e_z, in the fixed order (0, -x, +x, -y, +y, -z, +z).  A neighbour whose coordinate leaves
 *   [0, 2^21) on its axis is skipped: a packed key never borrows from or carries into another axis' bits.
 * Pairs.  A pair (row, voxel) exists when the voxel is in the index, has a place below max_voxels and is usable
 *   (record[15] == 1.0), as nsc_map_register decides for the own voxel.
 * Per pair.  d = w - mean_v, s = d^T Omega_v d, J = [-[w]x | I], and the weight w = rho'(s) of the pose graph's kernels
 *   (the table at nsc_posegraph_optimize_robust) with one width c = `scale` per call, in units of sqrt(chi^2):
 *   Huber w = 1 for s <= c^2 else c / sqrt(s); Cauchy w = 1 / (1 + s / c^2); Geman-McClure w = (c^2 / (c^2 + s))^2;
 *   NONE rho = s, w = 1.
 * System.  H = sum_pairs w J^T Omega J, g = sum_pairs w J^T Omega d, cost = sum_pairs rho(s).
 * Counts.  n_correspondences = rows with at least one pair (fitness = that / rows stays <= 1), n_pairs = the number of
 *   pairs, weight_sum = sum w.  rmse = sqrt(sum w |d|^2 / sum w), 0 when sum w = 0.
 * Rounds.  Convergence test, update, NaN initial transforms and scans without correspondences as nsc_map_register;
 *   information = H at the result.  A row's pairs are added in the fixed order and the reduction keeps its fixed shape:
 *   two calls agree bit for bit and a scan's result does not depend on what else is in the batch.
 * Outputs.  nsc_map_register's, with system0 (n_scans,NSC_MAP_REGISTER_ROBUST_SYSTEM) or NULL: the 30 sums of
 *   nsc_map_register in their places (sum w |d|^2 at 28, sum rho at 29), then sum w and n_pairs; and weight_pairs
 *   (n_scans,2) float64 = [weight_sum, n_pairs] at the result.  A scan whose init_transform is not finite gets
 *   weight_pairs = [NaN, -1] and a system0 of NaN.
 * Launches.  1 + 2 (max_iteration + 1), in nsc_map_register's shapes; NONE with one voxel launches nsc_map_register's
 *   own kernels.  Neighbours without a kernel pull every row towards up to seven means at full weight and bias the result:
 *   neighbours = 7 is meant to be used with a kernel.  Geman-McClure refines from a good start; Cauchy suits wide starts.
 * ------------------------------------------------------------------------------------------ */
#define NSC_MAP_VOXEL_DOUBLES       16
#define NSC_MAP_INSERT_LAUNCHES     8       /* kernels of one nsc_map_insert_dist call */
#define NSC_MAP_REMOVE_LAUNCHES     3       /* kernels of one nsc_map_remove_dist call */
#define NSC_MAP_REPLACE_LAUNCHES    10      /* of one nsc_map_replace_dist call: one clear, 2 of the removal, 7 of the insertion */
#define NSC_MAP_REMOVE_STATS            8   /* entries of `removed` */
#define NSC_MAP_REMOVE_STAT_REMOVED     0   /* rows taken out of a voxel                             */
#define NSC_MAP_REMOVE_STAT_NOT_FINITE  1   /* rows with a non-finite xyz or world coordinate        */
#define NSC_MAP_REMOVE_STAT_OUTSIDE     2   /* rows outside the 2^21 voxels per axis                 */
#define NSC_MAP_REMOVE_STAT_NO_POSE     3   /* rows of clouds without a pose (and rows of no cloud)  */
#define NSC_MAP_REMOVE_STAT_MISSING     4   /* rows whose voxel is not in the index or has place ~0  */
#define NSC_MAP_REMOVE_STAT_TOUCHED     5   /* voxels a row was taken out of                         */
#define NSC_MAP_REMOVE_STAT_EMPTIED     6   /* of those: count 0 and nine zero moments afterwards    */
#define NSC_MAP_REMOVE_STAT_INCONSISTENT 7  /* of those: count below 0, or 0 with a moment left      */
#define NSC_MAP_REHASH_LAUNCHES     4       /* kernels of one nsc_map_rehash_dist call */
#define NSC_MAP_REHASH_STATS            6   /* entries of `rehashed` */
#define NSC_MAP_REHASH_STAT_KEPT        0   /* voxels kept                                            */
#define NSC_MAP_REHASH_STAT_EMPTIED     1   /* voxels dropped as emptied                              */
#define NSC_MAP_REHASH_STAT_SOURCE_UNPLACED 2 /* source keys without a place: found - written          */
#define NSC_MAP_REHASH_STAT_INCONSISTENT 3  /* inconsistent voxels kept                               */
#define NSC_MAP_REHASH_STAT_UNPLACED    4   /* kept voxels without a place in the destination         */
#define NSC_MAP_REHASH_STAT_TABLE_FULL  5   /* kept voxels that found all 2 new_max_voxels slots keyed */
#define NSC_MAP_REGISTER_BLOCKS     64      /* workgroups of 256 lanes per scan in linearize */
#define NSC_MAP_REGISTER_SYSTEM     30
#define NSC_MAP_REGISTER_MAX_SCANS  65535
#define NSC_MAP_REGISTER_ROBUST_SYSTEM  32  /* the NSC_MAP_REGISTER_SYSTEM sums, then sum w and n_pairs */

/* NscMapRobustParams.kernel: the values of NSC_POSEGRAPH_KERNEL_* */
#define NSC_MAP_KERNEL_NONE           0
#define NSC_MAP_KERNEL_HUBER          1
#define NSC_MAP_KERNEL_CAUCHY         2
#define NSC_MAP_KERNEL_GEMAN_MCCLURE  3

typedef struct NscMapDistParams {
    int32_t min_points;             /* 6      rows a voxel needs to be usable, >= 1 */
    int32_t reserved;               /* 0 */
    double  eigen_ratio;            /* 1e-2   smallest eigenvalue kept, as a share of the largest; in (0, 1] */
    double  sigma_floor;            /* 1e-3   smallest standard deviation kept (m), finite and positive */
} NscMapDistParams;

typedef struct NscMapRegisterParams {
    int32_t max_iteration;          /* 30     >= 0 */
    int32_t reserved;               /* 0 */
    double  relative_fitness;       /* 1e-6   >= 0 */
    double  relative_rmse;          /* 1e-6   >= 0 */
} NscMapRegisterParams;

typedef struct NscMapRobustParams {
    int32_t kernel;                 /* NSC_MAP_KERNEL_NONE */
    int32_t neighbours;             /* 1      voxels a row is paired with: 1 (its own) or 7 (and the six face neighbours) */
    double  scale;                  /* 0      the kernel's width c, finite and positive with a kernel; not read with NONE */
} NscMapRobustParams;

void   nsc_map_dist_default_params(NscMapDistParams *p);
/* As nsc_map_workspace_bytes, with 256 bytes per voxel of max_voxels (the table of 128-byte slots). */
size_t nsc_map_dist_workspace_bytes(int64_t total_rows, int64_t max_voxels);
/* Refusals as nsc_map_build's, with voxels, index, info and keys needed when max_voxels > 0; NSC_EINVAL also for a null
 * `dist`, min_points < 1, eigen_ratio outside (0, 1] or a sigma_floor not finite and positive. */
int    nsc_map_build_dist(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets,
                          int32_t n_clouds, int64_t total_rows, const double *poses, int32_t n_poses,
                          const int64_t *pose_ids, const NscMapParams *params, const NscMapDistParams *dist,
                          int64_t max_voxels, double *voxels, uint64_t *index, int64_t *info, int64_t *keys,
                          int64_t *moments, int64_t *stats, void *ws, size_t ws_bytes, void *stream);

/* Bytes of workspace for nsc_map_insert_dist: about 16.2 per row (a slot and a list entry per row, the bitmap and its
 * prefixes) and nothing per voxel; monotone; 0 for a total_rows the call would refuse. */
size_t nsc_map_insert_workspace_bytes(int64_t total_rows);
/* Refusals as nsc_map_build_dist's; NSC_EINVAL also for a null `moments` or `cursor`; NSC_EWORKSPACE for a workspace that
 * is missing or too small: all before anything is launched. */
int    nsc_map_insert_dist(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets,
                           int32_t n_clouds, int64_t total_rows, const double *poses, int32_t n_poses,
                           const int64_t *pose_ids, const NscMapParams *params, const NscMapDistParams *dist,
                           int64_t max_voxels, double *voxels, uint64_t *index, int64_t *info, int64_t *keys,
                           int64_t *moments, int64_t *stats, int64_t *cursor, void *ws, size_t ws_bytes, void *stream);

/* Bytes of workspace for nsc_map_remove_dist (about 8 per row: a list entry) and for nsc_map_replace_dist (the sum of the
 * insertion's and the removal's); nothing per voxel; monotone; 0 for a total_rows the call would refuse. */
size_t nsc_map_remove_workspace_bytes(int64_t total_rows);
size_t nsc_map_replace_workspace_bytes(int64_t total_rows);
/* Refusals as nsc_map_build_dist's; NSC_EINVAL also for a null `moments` or `removed`; NSC_EWORKSPACE for a workspace that
 * is missing or too small (one is needed even for no rows): all before anything is launched. */
int    nsc_map_remove_dist(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets,
                           int32_t n_clouds, int64_t total_rows, const double *poses, int32_t n_poses,
                           const int64_t *pose_ids, const NscMapParams *params, const NscMapDistParams *dist,
                           int64_t max_voxels, double *voxels, uint64_t *index, int64_t *info, int64_t *keys,
                           int64_t *moments, int64_t *stats, int64_t *removed, void *ws, size_t ws_bytes, void *stream);
/* Refusals as nsc_map_remove_dist's; NSC_EINVAL also for a null new_poses with n_poses > 0, a null `placed` and a
 * negative first_row or first_cloud. */
int    nsc_map_replace_dist(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets,
                            int32_t n_clouds, int64_t total_rows, const double *old_poses, const double *new_poses,
                            int32_t n_poses, const int64_t *pose_ids, const NscMapParams *params,
                            const NscMapDistParams *dist, int64_t max_voxels, double *voxels, uint64_t *index,
                            int64_t *info, int64_t *keys, int64_t *moments, int64_t *stats, int64_t first_row,
                            int64_t first_cloud, int64_t *removed, int64_t *placed, void *ws, size_t ws_bytes,
                            void *stream);
/* NSC_EINVAL for a negative max_voxels, new_max_voxels < 1, a null stats, tile_base, rehashed or destination tensor
 * (new_voxels, new_index, new_info, new_keys, new_stats), with max_voxels > 0 a null voxels, info, keys or new_place,
 * moments or cursor given on one side only, or a destination pointer equal to its source pointer (the call is out of
 * place); NSC_EUNSUPPORTED for a size above NSC_MAP_MAX_VOXELS: all before anything is launched.  No workspace. */
int    nsc_map_rehash_dist(const double *voxels, const int64_t *info, const int64_t *keys, const int64_t *moments,
                           const int64_t *stats, const int64_t *cursor, int64_t max_voxels, int32_t keep_emptied,
                           double *new_voxels, uint64_t *new_index, int64_t *new_info, int64_t *new_keys,
                           int64_t *new_moments, int64_t *new_stats, int64_t *new_cursor, int64_t new_max_voxels,
                           int64_t *new_place, int64_t *tile_base, int64_t *rehashed, void *stream);

void   nsc_map_register_default_params(NscMapRegisterParams *p);
/* Bytes of workspace for nsc_map_register: the slabs and the state of n_scans scans; 0 for a negative n_scans. */
size_t nsc_map_register_workspace_bytes(int32_t n_scans);
/* NSC_EINVAL for a null or negative argument, a format nsc_map_build would refuse, a grid not finite and positive or
 * parameters out of range; NSC_EUNSUPPORTED for more than NSC_MAP_REGISTER_MAX_SCANS scans (callers split the batch) or
 * sizes above nsc_map_build's; NSC_EWORKSPACE for a workspace that is missing or too small: all before anything is
 * launched.  n_scans = 0 returns NSC_OK and launches nothing.  points may be NULL with total_rows = 0, voxels and index
 * with max_voxels = 0. */
int    nsc_map_register(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_scans,
                        int64_t total_rows, const double *voxels, const uint64_t *index, int64_t max_voxels,
                        const NscMapParams *params, const NscMapRegisterParams *reg, const double *init_transforms,
                        double *transforms, double *fitness_rmse, double *cost, int64_t *corr_iterations,
                        double *information, double *system0, void *ws, size_t ws_bytes, void *stream);

void   nsc_map_robust_default_params(NscMapRobustParams *p);
/* Bytes of workspace for nsc_map_register_robust: nsc_map_register's layout with slabs of NSC_MAP_REGISTER_ROBUST_SYSTEM
 * sums; monotone; 0 for a negative n_scans.  It is enough for every kernel and neighbourhood. */
size_t nsc_map_register_robust_workspace_bytes(int32_t n_scans);
/* NSC_EINVAL for a null `robust`, a kernel outside 0..3, neighbours other than 1 or 7, or a kernel other than NONE with a
 * scale that is not finite and positive: checked first, whatever else is passed.  Then nsc_map_register's refusals, and
 * NSC_EINVAL for a null weight_pairs with n_scans > 0. */
int    nsc_map_register_robust(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets,
                               int32_t n_scans, int64_t total_rows, const double *voxels, const uint64_t *index,
                               int64_t max_voxels, const NscMapParams *params, const NscMapRegisterParams *reg,
                               const NscMapRobustParams *robust, const double *init_transforms, double *transforms,
                               double *fitness_rmse, double *cost, int64_t *corr_iterations, double *information,
                               double *system0, double *weight_pairs, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Seen-through voxels (nsc_map_cast_rays, nsc_map_flag_rows; restated in tests/map_rays_restatement.py): which voxels of
 * a kept map did later scans look through, and which rows lie in them.  The map is read only.  Float64, every operation
 * rounded on its own; sums of three products are (x0 y0 + x1 y1) + x2 y2.
 *
 * nsc_map_cast_rays.  Rows, poses, pose_ids and params in the formats of nsc_map_build; voxels, index and max_voxels of a
 *   nsc_map_build_dist call with the same grid.
 * A ray is one row of a cloud with a pose P: o_a = P[a][3] the sensor, w the placed row (nsc_map_build's w),
 *   fo_a = (o_a - origin_a) / voxel, fw_a = (w_a - origin_a) / voxel, d = fw - fo, D = w - o (m),
 *   L = sqrt((d_x^2 + d_y^2) + d_z^2) voxel.
 * Dropped rays, each kind counted, the checks in this order: the cloud has no pose (pose_ids as in the build); xyz or w is
 *   not finite; the voxel of o or of w lies outside the 2^21 voxels per axis; the ray is short: with t0 = min_range / L and
 *   t1 = min(1 - end_margin / L, max_range / L), L > 0 is false or t0 < t1 is false.  A negative end_margin stands for one
 *   voxel edge.
 * The walk starts at k = floor(fo + t0 d).  Per axis the next face is tn_a = ((k_a + 1) - fo_a) / d_a for d_a > 0,
 *   (k_a - fo_a) / d_a for d_a < 0, +inf for d_a = 0: from k every step, never accumulated.  The step axis is the one with
 *   the smallest tn, the lowest axis winning a tie.  Voxel k is examined over [ta, tb]: ta = t0 for the first voxel, else
 *   the tn of the step that entered it; tb = min(tn_axis, t1).  If tn_axis < t1 is false the ray has ended; else
 *   k_axis +- 1.  A ray examines 3 (floor(max_range / voxel) + 2) voxels at most; one that has not ended by then stops and
 *   is counted in rays_truncated (in exact arithmetic none is).
 * Examining voxel k.  It is skipped when it is outside the grid or not in the index (nsc_map_register's probe), its place
 *   is ~0 or not below max_voxels, its key is the key of the voxel of w, or it is not usable (record[15] != 1.0).  Else,
 *   with the record's mean m and information Omega: a = o - m, num = D^T (Omega a), den = D^T (Omega D), Omega x formed
 *   row by row; t* = -num / den if den > 0, else ta; t* = min(max(t*, ta), tb); x = a + t* D; s = x^T (Omega x).  The ray
 *   crosses the voxel iff s <= gate^2: the segment comes within `gate` standard deviations of the voxel's own Gaussian.
 *   A ray that only runs through the box of a voxel, beside what the voxel holds, does not count.
 * Outputs.  crossed (max_voxels) int64: crossed[place] += 1 per crossing, ADDED to what the caller passes, so calls
 *   accumulate.  ray_stats (NSC_MAP_RAY_STATS) int64, written: rays cast (truncated ones included), not finite, outside,
 *   without pose, short, voxels examined, crossings, rays truncated.
 * Launches.  NSC_MAP_RAY_LAUNCHES kernels (clear the stats; cast: one lane per ray) whose grids depend on total_rows alone;
 *   integer atomics only, so two calls agree by bits and the cloud order changes nothing; no host synchronisation, no
 *   memset or memcpy nodes.  No workspace.
 *
 * nsc_map_flag_rows.  The rows again, with index, info (nsc_map_build_dist's) and crossed.  The voxel at a place is seen
 *   through iff count > 0, crossed >= min_crossings and (double)crossed >= ratio (double)count.  row_flags (total_rows)
 *   uint8, every entry written: 1 iff the row's own voxel (nsc_map_build's key, the index's probe) is seen through.
 *   flag_stats (NSC_MAP_FLAG_STATS) int64, written: rows flagged; rows kept; rows dropped (no pose, not finite or outside
 *   the grid); rows missing (the voxel is not in the index or has no place below max_voxels).
 *   A caller removes the flagged rows with nsc_map_remove_dist on the same cloud with every other row made NaN: a row that
 *   is not finite is dropped by every call here, so this is a matched removal of a subset.
 * Launches.  NSC_MAP_FLAG_LAUNCHES kernels (clear the stats; flag: one lane per row), as above.  No workspace.
 * ------------------------------------------------------------------------------------------ */
#define NSC_MAP_RAY_LAUNCHES        2       /* kernels of one nsc_map_cast_rays call */
#define NSC_MAP_FLAG_LAUNCHES       2       /* kernels of one nsc_map_flag_rows call */
#define NSC_MAP_RAY_MAX_REACH       65536   /* max_range / voxel_size at most */
#define NSC_MAP_RAY_STATS           8       /* entries of `ray_stats` */
#define NSC_MAP_RAY_STAT_CAST       0       /* rays walked                                           */
#define NSC_MAP_RAY_STAT_NOT_FINITE 1       /* rays with a non-finite xyz or world coordinate        */
#define NSC_MAP_RAY_STAT_OUTSIDE    2       /* rays whose sensor or end voxel is outside the grid    */
#define NSC_MAP_RAY_STAT_NO_POSE    3       /* rays of clouds without a pose (and rows of no cloud)  */
#define NSC_MAP_RAY_STAT_SHORT      4       /* rays with nothing between min_range and their end     */
#define NSC_MAP_RAY_STAT_VISITED    5       /* voxels examined                                       */
#define NSC_MAP_RAY_STAT_CROSSINGS  6       /* additions to `crossed`                                */
#define NSC_MAP_RAY_STAT_TRUNCATED  7       /* of the rays cast: stopped by the step bound           */
#define NSC_MAP_FLAG_STATS          4       /* entries of `flag_stats` */
#define NSC_MAP_FLAG_STAT_FLAGGED   0
#define NSC_MAP_FLAG_STAT_KEPT      1
#define NSC_MAP_FLAG_STAT_DROPPED   2
#define NSC_MAP_FLAG_STAT_MISSING   3

typedef struct NscMapRayParams {
    double  min_range;              /* 0      the walk starts this far from the sensor (m), >= 0 */
    double  max_range;              /* 60     and ends here at the latest (m), > 0; at most NSC_MAP_RAY_MAX_REACH voxels */
    double  end_margin;             /* -1     and this far in front of the row (m); negative: one voxel edge */
    double  gate;                   /* 3      a crossing comes within this many standard deviations, > 0 */
} NscMapRayParams;

void   nsc_map_ray_default_params(NscMapRayParams *p);
/* nsc_map_build's refusals, with voxels, index and crossed needed when max_voxels > 0 and ray_stats always; NSC_EINVAL also
 * for a null `ray`, a field of it that is not finite, min_range < 0, max_range <= 0 or gate <= 0; NSC_EUNSUPPORTED for
 * max_range / voxel_size above NSC_MAP_RAY_MAX_REACH: all before anything is launched. */
int    nsc_map_cast_rays(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_clouds,
                         int64_t total_rows, const double *poses, int32_t n_poses, const int64_t *pose_ids,
                         const NscMapParams *params, const double *voxels, const uint64_t *index, int64_t max_voxels,
                         const NscMapRayParams *ray, int64_t *crossed, int64_t *ray_stats, void *stream);
/* nsc_map_build's refusals, with index, info and crossed needed when max_voxels > 0, row_flags when total_rows > 0 and
 * flag_stats always; NSC_EINVAL also for min_crossings < 1 and a ratio not finite and positive: all before anything is
 * launched. */
int    nsc_map_flag_rows(const void *points, int32_t dtype, int32_t stride_floats, const int64_t *offsets, int32_t n_clouds,
                         int64_t total_rows, const double *poses, int32_t n_poses, const int64_t *pose_ids,
                         const NscMapParams *params, const uint64_t *index, const int64_t *info, const int64_t *crossed,
                         int64_t max_voxels, int64_t min_crossings, double ratio, uint8_t *row_flags, int64_t *flag_stats,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSC_H */
