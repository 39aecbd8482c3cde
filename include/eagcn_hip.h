/*
 * eagcn_hip.h -- C ABI of the MI355X (gfx950) EAGCN hot path.
 *
 * Drop-in boundary.  The reference (Luckick/EAGCN) has no FFI of its own: the hot path is the
 * Python nn.Module surface of eagcn_pytorch/layers.py and models.py, whose bodies are chains of
 * ATen calls.  Each entry point below replaces one such body; the reference-side binding a
 * maintainer would add is a ctypes stub inside the module's forward (shown in INTEGRATION.md,
 * implemented in eagcn_amd/_lib.py + eagcn_amd/layers.py).
 *
 *   eagcn_index_*        <- layers.py:294-304 (masks), layers.py:82 (1x1 conv over one-hot
 *                           relation tensors == dictionary lookup), utils.py:575-640 (layout)
 *   eagcn_index_from_bonds <- the same index from a compact bond list: replaces the dense padding of
 *                           utils.py:586-640 + neural_fp.py:57-122 on the device side
 *   eagcn_pack_rows / eagcn_unpack_rows
 *                        <- the padded [B,N,F] activation layout of layers.py:293 / models.py:96
 *   eagcn_layer_forward  <- GraphConv_Layer.forward, layers.py:293-316 with
 *                           GraphConv_block.forward layers.py:81-95, GraphConv_base.forward
 *                           layers.py:38-45, AFM_BatchNorm.forward layers.py:408-412,
 *                           Ave_multi_view.forward layers.py:431-437
 *   eagcn_layer_backward <- autograd of the above (the reference has no hand-written backward)
 *   eagcn_attention_dense<- the A_weight return value, layers.py:318 (stack of A1, layers.py:83)
 *   eagcn_readout_*      <- models.py:108-111 (sum / ave over atoms)
 *   eagcn_pool_*         <- Diff_Pooling.forward layers.py:498-506 as used by models.py:104-106 (molfp_mode='pool'), with
 *                           the last layer's A_weight of layers.py:319-324 (and its autograd backward)
 *   eagcn_gemm_f32       <- Dense.forward layers.py:382-387 (x @ W), used by models.py:114-120
 *   eagcn_bce_loss / eagcn_mse_loss
 *                        <- the loss of train.py:321-331 incl. weight_tensor utils.py:653-679
 *   eagcn_eval_append / eagcn_eval_class_metrics / eagcn_eval_reg_metrics
 *                        <- the evaluation functions train.py:130-211 (sklearn roc_curve + auc per task, RMSE; plus
 *                           average precision and MAE)
 *   eagcn_eval_reg_agreement / eagcn_eval_class_threshold
 *                        <- rsquared utils.py:714 (the squared Pearson coefficient), with R^2, Spearman and Kendall; the
 *                           thresholded metrics and log-loss of a classification trained with the weighted BCE of utils.py:642-700
 *   eagcn_rep_gather / eagcn_kmeans_*
 *                        <- dump_atom_rep train.py:213-287 (the selected atoms' representations) and the Lloyd k-means the
 *                           reference's analysis runs over them on the host (kmeans_atomrep.py)
 *   eagcn_knn / eagcn_knn_rank
 *                        <- the nearest molecules mol_to_vec_plot.py picks by eye; the ranks behind a trustworthiness score of
 *                           the embeddings of tsnes.py
 *   eagcn_silhouette / eagcn_cluster_moments
 *                        <- nothing in the reference, which reads the confusion matrix of kmeans_atomrep.py by eye: the
 *                           scores of a clustering (sklearn.metrics silhouette, Davies-Bouldin, Calinski-Harabasz)
 *   eagcn_model_forward / eagcn_model_backward
 *                        <- EAGCN.forward models.py:96-121 end to end (layers, read-out, Graph_BN,
 *                           den1/bn_den1/relu/dropout/den2/bn_den2/relu/den3) and its autograd backward
 *   eagcn_model_backward_input / eagcn_attr_*
 *                        <- afm.requires_grad_() (models.py:96) and autograd to the atom features; integrated gradients
 *   eagcn_layer_bond_grad / eagcn_bond_attr_finalize
 *                        <- nothing comparable in the reference (nearest: the A_weight return value, layers.py:318): autograd
 *                           to A1 of layers.py:82-83 per bond and view, times the attention (or the relation input)
 *
 * Conventions: all pointers are device pointers unless named host_*; tensors are fp32,
 * contiguous, row-major; `stream` is a hipStream_t passed as void*; functions return 0 on
 * success and a negative code on failure with a message available from eagcn_last_error().
 * No function synchronises the stream.  Nothing here falls back to a CPU path.
 *
 * Packed ("compact") activation layout: molecule b occupies rows row0[b] .. row0[b]+nat[b]-1 of a
 * [T, ld] matrix, nat[b] = 1 + (largest atom index that has a bond).  Rows of the padded
 * reference tensor beyond nat[b] (padding and trailing bond-less atoms) are never stored: every
 * one of them has the same value, which the kernels account for analytically.  Feature columns
 * are grouped in segments (one per view for a Concate layer output), each segment padded with zero
 * columns to a multiple of 16.
 */
#ifndef EAGCN_HIP_H
#define EAGCN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EAGCN_MAX_VIEWS 8
#define EAGCN_MAX_SEGS 8
#define EAGCN_MAX_CHANNELS 255
#define EAGCN_STRUCT_CONCATE 0
#define EAGCN_STRUCT_WEIGHTED 1

#define EAGCN_OK 0
#define EAGCN_ERR_ARG (-1)
#define EAGCN_ERR_HIP (-2)
#define EAGCN_ERR_SCRATCH (-3)

/* meta[] slots written by eagcn_index_build (device) and mirrored to host_meta */
#define EAGCN_META_T 0        /* packed rows                                   */
#define EAGCN_META_NMAX 1     /* max nat[b]                                    */
#define EAGCN_META_NTILES 2   /* sum_b ceil(nat[b]/16)                         */
#define EAGCN_META_BAD_ADJ 3  /* # adjacency entries not in {0,1}              */
#define EAGCN_META_BAD_REL 4  /* # bonded (i,j,view) whose channels are not one-hot */
#define EAGCN_META_NEDGE 5    /* # directed edges                              */
#define EAGCN_META_OVERFLOW 6 /* packed rows of a batch that does not fit the row capacity eagcn_batch.T (0 if it
                                 fits): such a batch is indexed as EMPTY (meta[T] = meta[NTILES] = 0), so that no
                                 kernel touches memory beyond the capacity-sized buffers              */
#define EAGCN_META_EDGE_OVERFLOW 7 /* directed bonds of a batch that does not fit the edge capacity eagcn_batch.E (0 if it
                                 fits); handled like EAGCN_META_OVERFLOW: the batch is indexed as empty                   */
#define EAGCN_META_NLOG 8     /* logical padded molecule size of THIS batch when it is smaller than the capacity eagcn_batch.N
                                 (eagcn_batch.n_logical): the reference pads every batch to its own maximum (utils.py:583) and
                                 counts the padding rows in its BatchNorm statistics and filler weights, so kernels take
                                 B * N_logical, N_logical - nat[b] from here; 0 = eagcn_batch.N                           */
#define EAGCN_META_NBLK 9     /* row blocks of eagcn_batch.blk (bond-list aggregation, csrc/lagg.hip)               */
#define EAGCN_META_WORDS 16

typedef struct eagcn_batch {
    int32_t B, N, K;
    int32_t ldc;                            /* row stride of code maps in bytes, multiple of 16 */
    int32_t T, n_max, n_tiles;              /* T / n_tiles: CAPACITIES (row stride of [K][T] buffers,
                                               grid sizing); the actual counts are meta[T], meta[NTILES]
                                               on the device and every kernel reads them there, so the
                                               caller may pass upper bounds without a host read-back  */
    int32_t channels[EAGCN_MAX_VIEWS];
    uint8_t* code;                          /* [K][B][N][ldc] 0 = no bond, c+1 = bond type c;
                                               rows with deg_bn == 0 are undefined (never given weight) */
    int32_t* deg_bn;                        /* [B][N] degree of every padded row                */
    int32_t* nat;                           /* [B]                                              */
    int32_t* row0;                          /* [B+1] exclusive prefix of nat                    */
    int32_t* tile0;                         /* [B+1] exclusive prefix of ceil(nat/16)           */
    int32_t* meta;                          /* [EAGCN_META_WORDS]                               */
    int32_t* row_mol;                       /* [T]                                              */
    int32_t* row_loc;                       /* [T] atom index inside the molecule               */
    float* row_m;                           /* [T] row mask m_i = max_j adj[i,j]                */
    int32_t* row_deg;                       /* [T]                                              */
    int32_t* tile_mol;                      /* [n_tiles]                                        */
    int32_t* row_info;                      /* [T][4] {molecule, atom, nat[mol], row0[mol]}: one
                                               16-byte load instead of a two-hop lookup          */
    int32_t* tile_info;                     /* [n_tiles][4] {molecule, row tile, nat[mol], row0[mol]} */
    /* General (non one-hot) relation tensors, layers.py:82: at a bond the reference evaluates sigmoid(sum_c w[c] R[c,i,j]) for
       ANY channel values.  The index keeps bond-type CODES; a code's meaning is a channel VECTOR: rel_vec[k] = [channels[k]]
       [rel_c[k]] floats (code c+1 -> row c), built per batch from the distinct vectors at the bonds (eagcn_amd/collate.py; at
       most 255 per view).  NULL (the default): code c+1 means the one-hot vector e_c, i.e. sigma(w[c]).                 */
    const float* rel_vec[EAGCN_MAX_VIEWS];
    int32_t rel_c[EAGCN_MAX_VIEWS];         /* channels of view k's attention weight when rel_vec[k] is set           */
    /* Bond lists (built by eagcn_index_rows from the code maps when build_lists is set): the GAT baseline layers
       (csrc/gat.hip, layers.py:99-203) walk them -- scores per atom, softmax over the deg+1 entries of a row.       */
    int32_t E;                              /* CAPACITY of the four edge arrays (directed bonds)             */
    int32_t n_logical;                      /* HOST input of the index entry points: padded size N_in <= N of the caller's
                                               tensors for this batch (their row stride), 0 = N; mirrored to meta[NLOG] */
    int32_t* ecnt;                          /* [B]   directed bonds of each molecule                         */
    int32_t* edge0;                         /* [B+1] exclusive prefix of ecnt                                */
    int32_t* mol_info;                      /* [B][4] {nat, row0, edge0, directed bonds}: one 16-byte load   */
    int32_t* row_ptr;                       /* [T][2] {first entry, count}: bonds (i,j) of packed row i      */
    int32_t* col_ptr;                       /* [T][2] {first entry, count}: bonds (i,j) INTO packed row j    */
    int32_t* nbr;                           /* [E] row lists: atom index j inside the molecule               */
    int32_t* tnbr;                          /* [E] column lists: atom index i inside the molecule            */
    uint64_t* ecode;                        /* [E] row lists: byte k = bond-type code of view k (1-based)    */
    uint64_t* tcode;                        /* [E] column lists: the same for bond (i,j)                     */
    int32_t build_lists;                    /* HOST input of eagcn_index_rows: build the bond lists (GAT layers, the
                                               LDS-staged bond-list aggregation of csrc/lagg.hip)              */
    int32_t t_hint;                         /* HOST hint: about how many packed rows batches of this shape really hold (0: unknown ->
                                               T).  Only steers size-dependent kernel CHOICES whose launch is baked into a captured
                                               graph (the plane GEMM's tile shape); every kernel is correct for any actual count.   */
    int32_t* blk;                           /* [8 (B + 1)] (optional, 16-byte aligned; built by eagcn_index_rows with the bond lists):
                                               ROW BLOCKS of the LDS-staged aggregation (csrc/lagg.hip) -- whole molecules, greedily
                                               packed to at most 256 packed rows and 16 molecules; block q = two int4 records {first
                                               molecule, molecules, first packed row, rows} {first list entry, entries, 0, 0};
                                               meta[NBLK] blocks                                                                    */
} eagcn_batch;

/* column layout of a packed activation matrix */
typedef struct eagcn_layout {
    int32_t nseg;
    int32_t width[EAGCN_MAX_SEGS];          /* exact widths                                     */
    int32_t pad[EAGCN_MAX_SEGS];            /* padded widths (sum = ld)                         */
} eagcn_layout;

typedef struct eagcn_layer_params {
    int32_t K;                              /* views                                            */
    int32_t structure;                      /* EAGCN_STRUCT_*                                   */
    int32_t training;                       /* BatchNorm batch statistics + dropout             */
    int32_t width[EAGCN_MAX_VIEWS];         /* F_k                                              */
    eagcn_layout in;                        /* layout of x                                      */
    float dropout;
    float bn_eps, bn_momentum;
    uint64_t seed;                          /* dropout stream for this call                     */
    const uint64_t* seed_dev;               /* if non-NULL the seed is read from this DEVICE word  */
                                            /* instead (a replayed HIP graph cannot change by-value */
                                            /* arguments)                                          */
    const float* att_w[EAGCN_MAX_VIEWS];    /* [C_k]    blockK.att.weight                       */
    const float* self_r[EAGCN_MAX_VIEWS];   /* [1]      blockK.self_r                           */
    const float* W[EAGCN_MAX_VIEWS];        /* [fin,F_k] blockK.graph_conv.weight               */
    const float* bias[EAGCN_MAX_VIEWS];     /* [F_k]    blockK.graph_conv.bias                  */
    const float* gamma[EAGCN_MAX_VIEWS];    /* [F_k]    blockK.batch_norm.bn.weight             */
    const float* beta[EAGCN_MAX_VIEWS];     /* [F_k]    blockK.batch_norm.bn.bias               */
    float* run_mean[EAGCN_MAX_VIEWS];       /* [F_k]    updated in place when training          */
    float* run_var[EAGCN_MAX_VIEWS];
    const float* ave_w;                     /* [K]      layer.ave.weight (Weighted_sum)         */
} eagcn_layer_params;

/* Cross-rank sum of `n` doubles in place on `stream` (sync-BatchNorm, SURVEY.md 8e "BN modes (ii)"): the per-channel partial
 * sums of a layer's BatchNorm (sum y, sum y^2, rows -- backward: sum dH, sum dH xhat, rows) are handed to the caller between
 * the reduction and the finalize kernel of that BatchNorm, forward and backward; the caller all-reduces them (RCCL through
 * torch.distributed in eagcn_amd/parallel.py -- also while the call is being captured into a HIP graph, the collective then
 * becomes a node of that graph).  Returns 0 on success.  NULL hook: BatchNorm over this rank's rows only ("local-BN"). */
typedef int (*eagcn_allreduce_fn)(double* buf, int n, void* stream, void* user);

typedef struct eagcn_layer_bufs {
    const float* x;                         /* [T][ld_in]                                       */
    float* P;                               /* [T][Fp]  X.[W_1|..|W_K]            (saved)       */
    float* Y;                               /* [T][Fp]  A_k.P_k, pre-bias, pre-BN (saved)       */
    float* rscale;                          /* [K][T]   m_i / rowsum_i            (saved)       */
    float* bn;                              /* [4][Fp]  scale, shift, mean, invstd (saved)      */
    float* xout;                            /* [T][ld_out]                                      */
    float* pad_row;                         /* [ld_out] value of every non-stored row of xout   */
    void* scratch;
    size_t scratch_bytes;
    void* aux_stream;                       /* reserved, must be NULL (a value: EAGCN_ERR_ARG). The */
                                            /* backward runs on the one stream of the call; the     */
                                            /* field keeps the struct's layout                      */
    void* packed;                           /* optional, eagcn_layer_packed_bytes(): forward keeps  */
    size_t packed_bytes;                    /* the re-laid parameters here and backward reuses them */
    eagcn_allreduce_fn stats_hook;          /* sync-BatchNorm: cross-rank sum of the BatchNorm partial sums (NULL: local-BN) */
    void* stats_user;
    /* bf16 plane images (gemm mode 3 / 4, csrc/gemm_bx3.hip: the layer products run on the bf16 matrix cores from operands    */
    /* their producers already split): x_planes = the plane images of x (panel-major images of row capacity eagcn_batch.T and   */
    /* ld_in columns, plane stride eagcn_bx3_plane_elems(T, ld_in) -- layout below at eagcn_bx3_split; three planes in mode 3,   */
    /* one in mode 4), written by the layer below through ITS xout_planes; NULL: the layer splits x itself (one more launch) /   */
    /* does not write them.  Ignored in the fp32 modes and for layers narrower than 128 input columns.                          */
    const uint16_t* x_planes;
    uint16_t* xout_planes;                  /* [planes] images of [T rows][ld_out], stride eagcn_bx3_plane_elems(T, ld_out)    */
} eagcn_layer_bufs;

typedef struct eagcn_layer_grads {
    float* dW[EAGCN_MAX_VIEWS];
    float* dbias[EAGCN_MAX_VIEWS];
    float* dgamma[EAGCN_MAX_VIEWS];
    float* dbeta[EAGCN_MAX_VIEWS];
    float* datt_w[EAGCN_MAX_VIEWS];
    float* dself_r[EAGCN_MAX_VIEWS];
    float* dave_w;                          /* [K] or NULL                                      */
} eagcn_layer_grads;

/* 1 when batches of this shape take a bond-list form of the aggregation in either direction (csrc/lagg.hip: a block of up to 256
 * packed rows staged in LDS, each row gathers its bonded rows, one rank-one term per molecule -- instead of the dense nat x nat
 * block on the matrix cores; default for large molecules, for batches of up to 256 molecules and for the backward of Concate
 * layers, padded sizes up to 256 atoms): the index must then carry bond lists and row
 * blocks -- set eagcn_batch.build_lists = 1 (and eagcn_batch.blk) before eagcn_index_rows.  `structure`: EAGCN_STRUCT_* of the
 * layers the index will serve, -1 when not known (the two-argument form). */
int eagcn_agg_wants_bond_lists(int B, int N);
int eagcn_agg_wants_bond_lists_for(int B, int N, int structure);

/* ---- library ------------------------------------------------------------------------------- */
int eagcn_abi_version(void);           /* 8 (eagcn_layer_route); bumped with every struct-layout / signature change */
size_t eagcn_struct_size(int which);   /* 0 batch, 1 layout, 2 layer_params, 3 layer_bufs, 4 layer_grads,
                                          5 head_params, 6 head_grads, 7 model, 8 gat_params, 9 pool_att */
const char* eagcn_last_error(void);
int eagcn_pad16(int width);
int eagcn_layer_out_ld(const eagcn_layer_params* p);   /* ld of xout                            */
int eagcn_layer_fp(const eagcn_layer_params* p);       /* Fp = sum_k pad16(F_k)                 */
size_t eagcn_layer_packed_bytes(const eagcn_batch* b, const eagcn_layer_params* p);
size_t eagcn_layer_fwd_scratch_bytes(const eagcn_batch* b, const eagcn_layer_params* p);
size_t eagcn_layer_bwd_scratch_bytes(const eagcn_batch* b, const eagcn_layer_params* p);
/* Which kernels a layer call would run for this batch: the route the library plans once per call and then carries out, for tests
 * and tools.  A pure host function -- no device pointer is dereferenced (addresses only count through their alignment), nothing is
 * launched.  has_dx: d(layer input) is asked for; mol_grad: the upstream gradient comes per molecule (top layer of the model
 * engine); input_only: the backward forms d(layer input) alone; has_drain_out: a layer below could take the edge-gradient reduction.
 *   out[0]  forward product     0 none (no packed row) | 1 operand planes | 2 balanced fp32 kernel | 3 tiled fp32 kernel |
 *           4 refused (x exists as plane images only and the plane product does not apply: the call fails)
 *   out[1]  the forward splits x into planes itself     out[11] the backward does
 *   out[2]  forward aggregation 0 matrix-core kernels | 1 LDS-staged bond lists           out[3] backward aggregation, likewise
 *   out[4]  second pass of the BatchNorm backward: 0 none | 1 elementwise, from the stored dH | 2 second pass of the reduction
 *           kernel | staged by the LDS-staged aggregation: 3 from the stored dH | 4 from the upstream gradient | 5 from the
 *           upstream gradient and the row mask (eval-mode input-only Concate)
 *   out[5]  the per-molecule gradient is written as rows before the reduction    out[6] ... after it (never both)
 *   out[7]  the reduction stores dH
 *   out[8]  edge gradients      0 none | 1 inside the LDS-staged aggregation | 2 one grid with the aggregation (3, an own launch,
 *           is no longer produced)
 *   out[9]  ... leave through the shared fp64 accumulators
 *   out[10] backward products   0 none | planes: 1 dX with dW | 2 dW alone | 3 dX alone | balanced pair: 4 XCD-local slabs |
 *           5 dW scattered in place | tiled: 6 pair | 7 dW alone (no dX asked) | 8 dX alone | 9 refused (as out[0])
 *   out[12] the edge-gradient reduction is left to the next layer's first backward kernel
 *   out[13] a layer handed plane images of x alone would cope in both directions (what the model engine asks before it drops the
 *           fp32 matrix: out[0] == 1 and out[10] == 1 of a call with has_dx that brings x_planes)
 *   out[14], out[15] 0 */
int eagcn_layer_route(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w, int has_dx, int mol_grad,
                      int input_only, int has_drain_out, int32_t out[16]);

/* ---- batch index ----------------------------------------------------------------------------- */
/* stage 1: needs code, deg_bn, nat, row0, tile0, meta; copies meta to host_meta (pinned) async */
int eagcn_index_build(const float* adj, const float* const* rel, eagcn_batch* b,
                      int32_t* host_meta, void* stream);
/* stage 1 from a COMPACT batch instead of the dense collate tensors: E directed bonds given as
 * bond_mol/bond_i/bond_j [E] (int32) and bond_code [E][K] (uint8, type index per view, < channels[k]).
 * Produces exactly the index eagcn_index_build derives from adj + one-hot relation tensors; touches
 * O(E) input bytes instead of 4*(1+sum C_k)*B*N*N. */
int eagcn_index_from_bonds(const int32_t* bond_mol, const int32_t* bond_i, const int32_t* bond_j,
                           const uint8_t* bond_code, int64_t E, eagcn_batch* b, int32_t* host_meta, void* stream);
/* stage 2 (after the caller read host_meta and allocated the per-row arrays) */
int eagcn_index_rows(const eagcn_batch* b, void* stream);

/* ---- layout conversion ----------------------------------------------------------------------- */
int eagcn_pack_rows(const eagcn_batch* b, const float* dense, int F, const eagcn_layout* lay,
                    float* packed, void* stream);
/* The GAT baseline layer (reference layers.py:99-203, models.py:69-73): x [T][ld_in] packed rows with a
   single-segment layout -> xout [T][pad16(F)].  h [T][pad16(F)] and s12 [2][T] are saved for the backward.  Needs a batch
   index with bond lists (eagcn_batch.build_lists).  Attention dropout 0.5 (layers.py:104) and the layer dropout are applied in
   training mode from the counter-based stream `seed`.                                                                      */
typedef struct eagcn_gat_params {
    int32_t fin, ld_in, F, training;
    float alpha, att_dropout, dropout;      /* leaky-relu slope (0.2), attention dropout (0.5), layer dropout          */
    float reserved_;
    uint64_t seed;
    const float* W;                         /* [fin][F]  graph_conv.W                                                   */
    const float* a;                         /* [2F]      graph_conv.a                                                   */
    const uint64_t* seed_dev;               /* optional: the seed is read from device memory (captured launches)       */
} eagcn_gat_params;
size_t eagcn_gat_scratch_bytes(const eagcn_batch* b, int F);
int eagcn_gat_forward(const eagcn_batch* b, const eagcn_gat_params* p, const float* x, float* h, float* s12, float* xout,
                      void* stream);
int eagcn_gat_backward(const eagcn_batch* b, const eagcn_gat_params* p, const float* x, const float* h, const float* s12,
                       const float* xout, const float* dxout, float* dx, float* dW, float* da, void* scratch,
                       size_t scratch_bytes, void* stream);

/* ---- Diff_Pooling read-out, molfp_mode='pool' (layers.py:492-506, models.py:90-92, 104-106) ------------------------------------
   g[b] = sum_p relu(S^T . relu((A.x).Wf)),  S = softmax((A.x).Ws), A = the attention matrix the LAST layer returns.
   The call sequence of one forward: eagcn_pool_attention_forward (A as packed rows [T][lda], lda >= N; rinv [T] = 1 / row sum;
   padsum [T] = total weight of the non-stored columns) -> eagcn_pool_mix_forward (AX [T][F] = A.x, exact columns) ->
   eagcn_gemm_f32 (Z [T][ldz] = AX . [Wf | Ws], F + P columns) -> eagcn_pool_reduce_forward (S [T][P], Pm [B][P][F], g [B][F]).
   Backward: the same entry points mirrored (reduce -> two GEMMs -> mix -> attention).  The pooled adjacency S^T.A.S that
   layers.py:504 also returns is never read by models.py and is not computed.                                             */
#define EAGCN_POOL_MAX 8                    /* clusters P (pool_num, models.py:25: 5)                                        */
typedef struct eagcn_pool_att {
    int32_t K;                              /* views of the layer that produced A (1 for the baselines)                      */
    int32_t mode;                           /* 0: edge-attention layer with last=True (layers.py:319-324)
                                               1: Vanilla_GCN (layers.py:250-253)   2: GAT (layers.py:189: adj + mask*I)     */
    int32_t att_c[EAGCN_MAX_VIEWS];         /* entries of att_w[k] / datt_w[k]                                               */
    const float* att_w[EAGCN_MAX_VIEWS];    /* mode 0: blockK.att.weight                                                     */
    const float* ave_a;                     /* mode 0: [K] ave_A.weight                                                      */
    const float* self_r;                    /* mode 0: [1] the LAYER's self_r (layers.py:287)                                */
    float* datt_w[EAGCN_MAX_VIEWS];         /* backward outputs (mode 0); NULL entries are skipped                           */
    float* dave_a;
    float* dself_r;
} eagcn_pool_att;
size_t eagcn_pool_scratch_bytes(void);
int eagcn_pool_attention_forward(const eagcn_batch* b, const eagcn_pool_att* p, float* A, int lda, float* rinv, float* padsum,
                                 void* stream);
int eagcn_pool_attention_backward(const eagcn_batch* b, const eagcn_pool_att* p, const float* A, int lda, const float* rinv,
                                  const float* dA, void* scratch, size_t scratch_bytes, void* stream);
/* x: packed activations [T][ld(lay)] of the last layer, pad_row [ld] (or NULL = 0): the value of every non-stored row */
int eagcn_pool_mix_forward(const eagcn_batch* b, const eagcn_layout* lay, const float* A, int lda, const float* padsum,
                           const float* x, const float* pad_row, float* AX, int F, void* stream);
/* dA [T][lda], dx [T][ld] (ZERO-FILLED by the caller: only exact columns are written), dpad_row [ld]; each may be NULL */
int eagcn_pool_mix_backward(const eagcn_batch* b, const eagcn_layout* lay, const float* A, int lda, const float* padsum,
                            const float* x, const float* pad_row, const float* dAX, int F, float* dA, float* dx,
                            float* dpad_row, void* stream);
int eagcn_pool_reduce_forward(const eagcn_batch* b, const float* Z, int ldz, int F, int P, float* S, float* Pm, float* g,
                              void* stream);
int eagcn_pool_reduce_backward(const eagcn_batch* b, const float* Z, int ldz, int F, int P, const float* S, const float* Pm,
                               const float* dg, float* dZ, void* stream);

/* Device half of the reference's collate (utils.py:504-640: every molecule zero-padded to the batch maximum): per-molecule
   atom-feature rows, concatenated [sum n_b][F] with molecule b = rows mol_offset[b] .. mol_offset[b+1], -> padded [B][N][F].
   Together with eagcn_index_from_bonds a batch reaches the device as O(atoms + bonds) bytes instead of
   4 (1 + sum C_k) B N^2.                                                                     */
int eagcn_pad_rows(const float* rows, const int32_t* mol_offset, int B, int N, int F, float* out, void* stream);

int eagcn_unpack_rows(const eagcn_batch* b, const float* packed, const eagcn_layout* lay,
                      const float* pad_row, float* dense, int F, void* stream);

/* ---- graph-conv layer ------------------------------------------------------------------------ */
int eagcn_layer_forward(const eagcn_batch* b, const eagcn_layer_params* p,
                        const eagcn_layer_bufs* w, void* stream);
/* dxout: [T][ld_out]; dpad_row: [ld_out] gradient w.r.t. bufs.pad_row (the common value of all
 * non-stored rows; Weighted_sum only) or NULL; dx: [T][ld_in] or NULL */
int eagcn_layer_backward(const eagcn_batch* b, const eagcn_layer_params* p,
                         const eagcn_layer_bufs* w, const float* dxout, const float* dpad_row,
                         float* dx, const eagcn_layer_grads* g, void* stream);
/* A1_k = sigmoid(w_k[type]) * adj for every view: out [K][B][N][N] */
int eagcn_attention_dense(const eagcn_batch* b, const eagcn_layer_params* p, float* out,
                          void* stream);

/* ---- read-out -------------------------------------------------------------------------------- */
/* g[b][f] = sum_i x[b,i,f] (all N rows; non-stored rows contribute pad_row) ; mode 1: / size[b] */
int eagcn_readout_forward(const eagcn_batch* b, const float* x, const eagcn_layout* lay,
                          const float* pad_row, const int64_t* size, int mode, float* g, int F,
                          void* stream);
/* dx: [T][ld]; dpad_row: [ld] or NULL */
int eagcn_readout_backward(const eagcn_batch* b, const float* dg, const eagcn_layout* lay,
                           const int64_t* size, int mode, int F, float* dx, float* dpad_row,
                           void* stream);

/* ---- whole model: one call forward, one call backward (reference models.py:96-121) -------------- */
typedef struct eagcn_head_params {
    int32_t f_in, n_den1, n_den2, nclass;
    float dropout, bn_eps, bn_momentum;
    const float *den1_w, *den2_w, *den3_w;          /* [f_in,n_den1] [n_den1,n_den2] [n_den2,nclass]   */
    const float *gbn_w, *gbn_b;  float *gbn_rm, *gbn_rv;   /* Graph_BN   (models.py:80-88, 112)        */
    const float *bn1_w, *bn1_b;  float *bn1_rm, *bn1_rv;   /* bn_den1    (models.py:115)               */
    const float *bn2_w, *bn2_b;  float *bn2_rm, *bn2_rv;   /* bn_den2    (models.py:119)               */
} eagcn_head_params;

typedef struct eagcn_head_grads {
    float *d_den1_w, *d_den2_w, *d_den3_w, *d_gbn_w, *d_gbn_b, *d_bn1_w, *d_bn1_b, *d_bn2_w, *d_bn2_b;
} eagcn_head_grads;

typedef struct eagcn_model {
    int32_t n_layers;                       /* 1..4                                                    */
    int32_t molfp_mode;                     /* 0 = 'sum', 1 = 'ave' (models.py:108-111)                */
    int32_t training;
    uint64_t head_seed;                     /* dropout stream of the head (models.py:116)              */
    const uint64_t* head_seed_dev;          /* device-resident alternative (see eagcn_layer_params)    */
    int32_t input_packed;                   /* 1: saved already holds the packed input (eagcn_model_pack_input) */
    void* aux_stream;                       /* reserved, must be NULL (a value: EAGCN_ERR_ARG); keeps the layout */
    eagcn_layer_params layer[4];            /* layer[l].in must equal the output layout of layer l-1   */
    eagcn_head_params head;
    eagcn_allreduce_fn stats_hook;          /* sync-BatchNorm of EVERY BatchNorm of the model (the per-view ones of the layers and
                                               Graph_BN / bn_den1 / bn_den2 of the head; see eagcn_layer_bufs); NULL: local-BN   */
    void* stats_user;
    int32_t stats_world;                    /* ranks behind the hook (>= 1): the head's d gamma / d beta are formed from the
                                               summed sums and divided by it, so that the gradient AVERAGE over ranks is exact */
    int32_t fuse_readout;                   /* 1: a Concate top layer does not materialise its output matrix in the forward: its
                                               relu / dropout / mask are applied while the read-out sums the atoms (one launch
                                               instead of bn_apply + read-out + column statistics).  The matrix
                                               (atom_representations, models.py:102) is built on request by
                                               eagcn_model_atom_rep_materialize.  Ignored for other structures.            */
    uint32_t* fwd_signal;                   /* optional device word: the forward adds 1 to it behind the read-out (the head's first
                                               launch does, with a relaxed atomic: the word places work, it guards no data), i.e. when the
                                               layer products / aggregations of the step have been issued and only short kernels
                                               follow for a while (head, loss, head backward, the top BatchNorm backward).  Another
                                               stream can wait for a count with eagcn_stream_wait_counter: the caller's batch
                                               preparation for the NEXT step is placed under those kernels instead of beside the
                                               persistent GEMMs (eagcn_amd/graph.py).  NULL: no signal                        */
    uint32_t* wait_flag;                    /* optional device word: the forward's FIRST launch polls it until it is non-zero and
                                               clears it -- the batch-ready hand-off from the stream that built the index and packed
                                               the input (eagcn_stream_signal_flag behind its last kernel) without a
                                               hipStreamWaitEvent, whose cross-queue dependency costs the waiting stream ~40 us per
                                               step on ROCm 7.2.  The signal must already be enqueued when the forward is issued
                                               (on a stream that runs concurrently with this one).  NULL: no wait               */
    uint32_t* start_signal;                 /* optional device word: the forward's FIRST launch adds 1 to it -- everything issued on the
                                               stream before this forward (the previous steps: their index / saved blocks are free) has
                                               completed.  The stream that prepares the batch after next waits for the count
                                               (eagcn_stream_wait_counter) instead of for a stream event recorded between two step
                                               graphs (recording one that another stream waits for costs the recording stream ~27 us
                                               per step on ROCm 7.2).  NULL: no signal.  Both hand-offs ride in the parameter-packing
                                               launch (no launch of their own) when the input arrives packed (input_packed = 1)       */
} eagcn_model;

/* *flag = 1 behind everything issued on `stream` so far (release, device scope) */
int eagcn_stream_signal_flag(uint32_t* flag, void* stream);
/* one parked wavefront on `stream` that polls *flag until it is non-zero, then clears it (what eagcn_model.wait_flag does in front of a
 * forward); after budget_seconds without a signal it gives up and raises the sticky word below */
int eagcn_stream_wait_flag(uint32_t* flag, double budget_seconds, void* stream);
int eagcn_stream_wait_timeouts(void);   /* non-zero once any flag wait gave up (host-mapped word, no synchronisation) */
void eagcn_stream_wait_reset(void);

/* `stream` does not run anything issued behind this call until *counter (device memory, see eagcn_model.fwd_signal / start_signal)
 * >= value: one parked wavefront that polls the word.  The signalling work must already be enqueued (or be enqueued without
 * waiting for this stream); after 2 s without it the poll gives up and raises the sticky word of eagcn_stream_wait_timeouts. */
int eagcn_stream_wait_counter(const uint32_t* counter, uint32_t value, void* stream);

size_t eagcn_model_saved_bytes(const eagcn_batch* b, const eagcn_model* m);    /* kept forward -> backward */
size_t eagcn_model_scratch_bytes(const eagcn_batch* b, const eagcn_model* m);  /* transient, either call  */
/* where the last layer's packed activations [T][ld] and pad_row [ld] live inside `saved` */
int eagcn_model_atom_rep(const eagcn_batch* b, const eagcn_model* m, size_t* xout_offset,
                         size_t* pad_row_offset, int* ld);
/* builds the last layer's packed output [T][ld] (+ pad_row) inside `saved` from the saved pre-BatchNorm matrix when the forward
 * ran with fuse_readout = 1 (same values as a forward without the fusion, same dropout masks); a no-op otherwise */
int eagcn_model_atom_rep_materialize(const eagcn_batch* b, const eagcn_model* m, void* saved, size_t saved_bytes, void* stream);
/* packs afm [B][N][n_afeat] into the input slot of `saved` (the first step of eagcn_model_forward) */
int eagcn_model_pack_input(const eagcn_batch* b, const eagcn_model* m, const float* afm, void* saved,
                           size_t saved_bytes, void* stream);
/* afm: dense [B][N][n_afeat]; out: [B][nclass]; graph_rep: [B][n_den2] (den2 output, models.py:118) */
int eagcn_model_forward(const eagcn_batch* b, const eagcn_model* m, const float* afm, const int64_t* size,
                        void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, float* out,
                        float* graph_rep, void* stream);
/* dgraph_rep may be NULL; lg: n_layers entries */
int eagcn_model_backward(const eagcn_batch* b, const eagcn_model* m, const int64_t* size, void* saved,
                         size_t saved_bytes, void* scratch, size_t scratch_bytes, const float* dout,
                         const float* dgraph_rep, const eagcn_layer_grads* lg, const eagcn_head_grads* hg,
                         void* stream);

/* The same backward in two pieces, so that a data-parallel caller can start the gradient all-reduce of the upper layers while the
 * lower ones are still running: with_head != 0 runs the head + read-out backward first; then the layers layer_hi, layer_hi-1,
 * ..., layer_lo (n_layers-1 >= layer_hi >= layer_lo >= 0).  eagcn_model_backward == (with_head = 1, n_layers-1, 0); a split
 * must be issued top-down on one stream: (1, n_layers-1, l) then (0, l-1, 0). */
int eagcn_model_backward_range(const eagcn_batch* b, const eagcn_model* m, const int64_t* size, void* saved,
                               size_t saved_bytes, void* scratch, size_t scratch_bytes, const float* dout,
                               const float* dgraph_rep, const eagcn_layer_grads* lg, const eagcn_head_grads* hg,
                               int with_head, int layer_hi, int layer_lo, void* stream);
/* The plan of one engine call, for tests and tools: what the library decides ONCE per eagcn_model_forward* / eagcn_model_backward* call,
 * from the buffers the call runs on, and then carries out.  A pure host function as eagcn_layer_route -- `saved` / `scratch` are only
 * carved (sizes are checked), nothing is dereferenced or launched.  The ask is that of eagcn_model_backward_range, with has_dx0:
 * layer 0 forms d(its input) and input_only: no parameter gradient (both: eagcn_model_backward_input); layer_hi < layer_lo asks for
 * no layer's backward -- the plan of a forward call.
 *   out[l][0..13]  as eagcn_layer_route, of the calls the engine makes for layer l: the forward's out[0..2] for every layer, the
 *                  backward's out[3..12] for the layers in [layer_lo, layer_hi] (0 elsewhere); out[l][13] = the layer is handed no fp32
 *                  input (the layer below wrote plane images only)
 *   out[l][14]     bits: 1 the output leaves as plane images only | 2 the apply pass is skipped (fused read-out) | 4 the top layer's
 *                  BatchNorm column sums are formed by the read-out and the head's backward | 8 the top layer uses them | 16 ... and
 *                  gathers the read-out gradient per molecule | 32 dH and its column sums are given by the layer above | 64 this layer's
 *                  dX product carries the tail pass that forms them for the layer below | 128 dW leaves the aggregation's epilogue |
 *                  256 the plane pair / dW launch runs on the 256 x 128 kernel.  Bits 1, 2, 4 do not depend on the ask
 *   out[l][15]     slabs of that epilogue (dw_ny) */
int eagcn_model_route(const eagcn_batch* b, const eagcn_model* m, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes,
                      int with_head, int layer_hi, int layer_lo, int has_dx0, int input_only, int32_t out[4][16]);

/* ---- d / d afm: the gradient of a prediction with respect to the atom features ("which atoms drive this prediction") ----------------
 * d(out.dout + graph_rep.dgraph_rep) / d afm, dense [B][N][n_afeat] (the row stride eagcn_model_pack_input reads): every entry written
 * (rows that are not stored are 0).  dgraph_rep may be NULL.
 *   lg, hg non-NULL: the same parameter gradients as eagcn_model_backward, plus dafm.
 *   lg == NULL && hg == NULL: INPUT-ONLY backward: no parameter gradient is formed.  Per hidden layer only the transposed aggregation
 *     (no edge gradients) and dX = dP.Wcat^T run; in eval mode (m->training == 0) no BatchNorm reduction either (the eval BatchNorm
 *     backward is the per-column scale gamma rsqrt(rv + eps) with the relu / view-merge mask, applied where the aggregation stages its
 *     rows).  The head's backward kernels run with their weight gradients written into `scratch`.  Training mode keeps the
 *     BatchNorm reductions (the mean-removal terms need them) and still skips every weight and edge gradient.
 * scratch_bytes >= eagcn_model_input_scratch_bytes (the model scratch plus layer 0's packed d(input) and the discarded head gradients).
 * Rejected before any HIP call: dafm NULL; exactly one of lg / hg NULL; a structure or read-out the engine does not run (GAT, pool). */
size_t eagcn_model_input_scratch_bytes(const eagcn_batch* b, const eagcn_model* m);
int eagcn_model_backward_input(const eagcn_batch* b, const eagcn_model* m, const int64_t* size, void* saved,
                               size_t saved_bytes, void* scratch, size_t scratch_bytes, const float* dout,
                               const float* dgraph_rep, const eagcn_layer_grads* lg, const eagcn_head_grads* hg,
                               float* dafm, void* stream);

/* ---- attribution: integrated gradients (csrc/attr.hip) ------------------------------------------------------------------------------
 * attr = (x - x') . integral_0^1 d target / d x (x' + a (x - x')) da  by the MIDPOINT rule over m points:
 *     alpha_s = (s + 1/2) / m,   w_s = 1 / m,   s = 0 .. m-1          (eagcn_attr_alpha / eagcn_attr_weight return them)
 * One point: eagcn_attr_pack_input(alpha_s) -> eagcn_model_forward with m->input_packed = 1 -> eagcn_attr_step(w_s, first = s == 0);
 * then ONE eagcn_attr_finalize.  m = 1 with alpha = 1 and no baseline is gradient x input.  Every call is capturable (no host sync). */
float eagcn_attr_alpha(int step, int steps);
float eagcn_attr_weight(int steps);
/* floats of the packed accumulator [T][ld] (ld: the packed width of layer 0's input layout) */
size_t eagcn_attr_acc_elems(const eagcn_batch* b, const eagcn_model* m);
/* packs baseline + alpha (afm - baseline) into the input slot of `saved` (what eagcn_model_pack_input fills); baseline NULL = 0 */
int eagcn_attr_pack_input(const eagcn_batch* b, const eagcn_model* m, const float* afm, const float* baseline, float alpha,
                          void* saved, size_t saved_bytes, void* stream);
/* the input-only backward of eagcn_model_backward_input behind a forward, then acc = weight dX0 (first != 0) or acc += weight dX0, in
 * packed rows (the dense gradient of a point is not formed).  scratch_bytes >= eagcn_model_input_scratch_bytes */
int eagcn_attr_step(const eagcn_batch* b, const eagcn_model* m, const int64_t* size, void* saved, size_t saved_bytes,
                    void* scratch, size_t scratch_bytes, const float* dout, const float* dgraph_rep, float weight, int first,
                    float* acc, void* stream);
/* attr[B][N][n_afeat] = (afm - baseline) * acc (0 at rows that are not stored), score[B][N] = sum over the features: one launch */
int eagcn_attr_finalize(const eagcn_batch* b, const eagcn_model* m, const float* afm, const float* baseline, const float* acc,
                        float* attr, float* score, void* stream);

/* ---- bond attribution: gradient x attention per bond (csrc/battr.hip) -----------------------------------------------------------------
 * For an EVAL-mode layer (p->training == 0) whose forward left P, Y, rscale, bn in `w`, the gradient dxout [T][ld_out] of a scalar
 * target at the layer's output, view k and the bond e = (i, j) of the batch index's ROW LISTS (packed rows i, j of one molecule):
 *     dY_i[c]  = sc[c] * [sc[c] * Y_i[c] + sh[c] > 0] * dH_i[c]            (sc, sh = rows 0, 1 of the bn table)
 *     dH_i[c]  = m_i * dxout_i[c]                   Concate (ld_out == Fp)
 *              = ave_w[k] * dxout_i[c - off_k]      Weighted_sum (and the GCN baseline, which is a one-view Weighted_sum layer)
 *     D[k][e]  = d target / d A1^k_ij = rscale_k[i] * < dY_i , P_j - Y_i >   over view k's columns
 * with A1 = sigmoid(z) * adj the tensor of layers.py:82-83 and z the bond's attention logit (att_w[k][code - 1], or <att_w[k],
 * rel_vec[k][code - 1]> for general relations).  eagcn_layer_bond_grad performs, for every entry e the row lists name,
 *     acc[k][e] = (first ? 0 : acc[k][e]) + weight * f(z) * D[k][e]          acc: [K][b->E], 16-byte aligned
 *     mode 0   f = sigmoid(z)                    A1 * d target / d A1: gradient x attention
 *     mode 1   f = sigmoid(z) (1 - sigmoid(z)) z  sum_c rel[c] * d target / d rel[c]: gradient x input of the relation tensor
 * so that one call per layer into the same accumulator sums the layers.  One wave per packed row, P_j gathered from global memory
 * (no molecule is staged in LDS: any molecule size), no atomics: every (k, e) has one owner and repeated runs are bit-identical.
 * Needs an index with bond lists (eagcn_batch.build_lists); a list entry whose j is not a stored row reads nothing and adds 0 (the
 * index lists no such bond: a one-directional bond into an atom beyond nat[b] has no entry at all).  Entries of the edge arrays that
 * no row list names are not written.  Rejected before any HIP call (EAGCN_ERR_ARG): a null pointer, mode outside {0, 1}, training
 * mode, an index without bond lists, acc / dxout / P / Y / bn that are not 16-byte aligned.  Nothing comparable exists in the
 * reference: its nearest output is the A_weight return value (eagcn_attention_dense).
 *
 * eagcn_bond_attr_finalize: for every entry e of the row lists (row-list order) mol[e], bi[e], bj[e] = (molecule, i, j) and
 * score[e] = sum_k acc[k][e]; with `dense` non-NULL also dense[k][mol][i][j] = acc[k][e] into a [K][B][N][N] tensor the caller
 * zero-filled (N: the row stride eagcn_model_pack_input reads).  mol / bi / bj / score: [b->E]. */
int eagcn_layer_bond_grad(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w, const float* dxout, int mode,
                          float weight, int first, float* acc, void* stream);
int eagcn_bond_attr_finalize(const eagcn_batch* b, const float* acc, int K, int32_t* mol, int32_t* bi, int32_t* bj, float* score,
                             float* dense, void* stream);

/* ---- a training step's forward + loss + HEAD backward as one call (reference train.py:317-331 in front of models.py:112-120 and
 * their autograd): the model forward as eagcn_model_forward, then the loss on `out` and the backward of den3 / bn_den2 / den2 /
 * bn_den1 / den1 / Graph_BN.  Where a row block of the logits is one tile (nclass <= 64) and no sync-BatchNorm hook sits between the
 * stages, the last forward product, the loss and dense 3's d(input) product run as ONE launch per 16-row block (csrc/head2.hip
 * head_mid_kernel) and dense 3's weight gradient rides in dense 2's backward launch: six launches instead of eight; otherwise
 * the separate launches -- same arithmetic, same results.  On return *loss->loss, loss->dout, every head gradient
 * of `hg` and the gradient of the molecule fingerprints (inside `scratch`) exist: the caller continues with
 * eagcn_model_backward_range(..., dout = loss->dout, with_head = 0, n_layers - 1, layer_lo). */
typedef struct eagcn_step_loss {
    int32_t kind;                /* 0: weighted BCE with logits over the labelled entries (train.py:326-331, eagcn_bce_loss)
                                    1: mean squared error (train.py:321-325, eagcn_mse_loss)                                 */
    const float* labels;         /* [B][nclass]; kind 0: 1 / 0 / anything else = missing                                     */
    const float* class_weight;   /* kind 0: [nclass][2] = {w_pos, w_neg}; kind 1: unused                                     */
    float* loss;                 /* device scalar (out)                                                                      */
    const float* scale;          /* optional device scalar: loss and d loss / d out are multiplied by it (the data-parallel
                                    normalisation of eagcn_amd/parallel.py); NULL = 1                                        */
    float* dout;                 /* [B][nclass] (out): d loss / d out                                                        */
} eagcn_step_loss;
int eagcn_model_forward_step(const eagcn_batch* b, const eagcn_model* m, const float* afm, const int64_t* size,
                             void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, float* out,
                             float* graph_rep, const eagcn_step_loss* loss, const float* dgraph_rep,
                             const eagcn_head_grads* hg, void* stream);

/* ---- the head ALONE (models.py:112-120: Graph_BN -> den1 -> bn_den1 -> relu -> dropout -> den2 = graph_representation ->
 * bn_den2 -> relu -> den3) for callers that form the molecule fingerprints g [B][f_in] themselves: the GAT baseline
 * (models.py:69-73) and the Diff_Pooling read-out (models.py:104-106), whose layers run through the layer-level entry points.
 * Same kernels, same launch sequence as the head inside eagcn_model_forward / eagcn_model_backward (four launches + one clear
 * per direction).  saved: eagcn_head_saved_bytes, written by the forward, read by the backward (the caller keeps g as well);
 * scratch: eagcn_head_scratch_bytes, transient per call.  training != 0 updates the running statistics in place and needs B > 1.
 * seed / seed_dev: the head's dropout stream (seed_dev: a device-resident seed, read by the kernels -- captured launches).
 * The backward writes d loss / d g into dg [B][f_in] and every head gradient through hg. */
size_t eagcn_head_saved_bytes(const eagcn_head_params* h, int B);
size_t eagcn_head_scratch_bytes(const eagcn_head_params* h, int B);
int eagcn_head_forward(const eagcn_head_params* h, int B, int training, uint64_t seed, const uint64_t* seed_dev, const float* g,
                       void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, float* out, float* graph_rep,
                       void* stream);
int eagcn_head_backward(const eagcn_head_params* h, int B, int training, uint64_t seed, const uint64_t* seed_dev, const float* g,
                        void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, const float* dout,
                        const float* dgraph_rep, const eagcn_head_grads* hg, float* dg, void* stream);

/* ---- losses of the training loop (train.py:321-331), value + d/dlogits in one launch --------------- */
/* labels [B][T] with 1 / 0 / anything else = missing; class_weight [T][2] = {w_pos, w_neg} (utils.py:681-700) */
int eagcn_bce_loss(const float* logits, const float* labels, const float* class_weight, int B, int T,
                   float* loss, float* dlogits, void* stream);
int eagcn_mse_loss(const float* pred, const float* target, int n, float* loss, float* dpred, void* stream);

/* ---- optimizer step (train.py:303 `optim.Adam(..., weight_decay=wd)`, train.py:334) as ONE launch over flat fp32 buffers: every
 * hot-path parameter in one buffer, gradients / first / second moments in buffers of the same layout (n floats, a multiple of 4,
 * 16-byte aligned).  torch.optim.Adam arithmetic.  hyper_dev = {lr, beta1, beta2, eps, weight_decay} as DOUBLES (torch's scalars
 * are Python doubles: 1 - beta2 formed from an fp32 0.999 is off by 1.7e-5) and the step count *step_dev (advanced by the launch)
 * live in device memory, so the launch can sit in a captured graph; *ticket_dev must be 0 on entry (the launch leaves it 0).
 * ticket_dev == NULL: the range is updated and the count NOT advanced (several ranges of one step: the last call brings the ticket). */
int eagcn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const double* hyper_dev,
                    int64_t* step_dev, uint32_t* ticket_dev, void* stream);

/* ---- gradient-norm clipping and non-finite step skipping for that step, on the device (csrc/clip.hip): what
 * torch.nn.utils.clip_grad_norm_(params, max_norm) in front of optimizer.step() does, as two capturable launches, no host read.
 *   eagcn_grad_norm: sum of squares (squares and sums in fp64) and count of non-finite values (NaN, +-Inf) over the LIVE elements of
 *     grad[0..n) (n floats, a multiple of 4, 16-byte aligned).  live_lanes[i], i < n / 4, = how many LEADING floats of the i-th
 *     group of four are live (0..4): a parameter's slot is its elements, then <= 3 pad words; a frozen parameter's slot is all 0.
 *     live_lanes == NULL: every element is live.  At most 1024 workgroups of 256 each write one partial into their own slot; the
 *     one that finishes last adds the slots in slot order: the totals are bit-identical from run to run (no floating-point atomics).
 *     accumulate != 0: the totals are ADDED to the stored ones (several ranges of one step) instead of replacing them.
 *   workspace: eagcn_grad_norm_workspace_bytes() = 32 + 1024 * 16 bytes, 16-byte aligned, ZERO before its first use (a launch
 *     leaves the ticket 0):
 *       byte  0  double   sumsq      total of the last launch (or of the accumulating launches since the last replacing one)
 *       byte  8  uint64   n_bad      non-finite live elements, likewise
 *       byte 16  uint32   ticket     workgroups finished in the running launch; 0 between launches
 *       byte 20  12 bytes reserved
 *       byte 32  1024 x { double sumsq ; uint64 n_bad }    one slot per workgroup
 *   eagcn_adam_step_clipped: eagcn_adam_step with g' = coef * g in place of g (rounded to fp32 before the weight decay is added,
 *     as torch scales p.grad before the step; grad itself is NOT written), coef = the fp32 image of
 *     min(1, max_norm / (sqrt(sumsq) + 1e-6)) formed in double from norm_workspace's totals.  With coef == 1 every output bit equals
 *     eagcn_adam_step's.  clip_dev = double[2] {max_norm (+Inf: measure, never clip), skip_nonfinite (0 / not 0)}.  When n_bad > 0
 *     and skip_nonfinite is set NOTHING is written to param / exp_avg / exp_avg_sq and *step_dev does not advance.
 *     The launch that brings ticket_dev (the last range of a step) also resets norm_workspace's ticket and updates
 *       stats_dev: int64 applied | int64 skipped | int64 clipped (applied with coef < 1) | double last_norm (= sqrt(sumsq),
 *       NaN / Inf when the gradient held one), 32 bytes, 8-byte aligned. */
size_t eagcn_grad_norm_workspace_bytes(void);
int eagcn_grad_norm(const float* grad, const uint8_t* live_lanes, int64_t n, void* workspace, int accumulate, void* stream);
int eagcn_adam_step_clipped(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const double* hyper_dev,
                            int64_t* step_dev, uint32_t* ticket_dev, void* norm_workspace, const double* clip_dev,
                            int64_t* stats_dev, void* stream);

/* ---- evaluation outputs (train.py:130-211): append one batch to device-resident [cap][T] buffers at row `row_offset`:
 * scores = sigmoid(logits) (classification = 1) or the predictions (0), targets = labels, valid = label in {0,1} / 1 ---- */
int eagcn_eval_append(const float* logits, const float* labels, int B, int T, int classification, float* scores,
                      float* targets, uint8_t* valid, int64_t row_offset, void* stream);

/* ---- evaluation metrics over those buffers (train.py:156-211), on the device: two launches per call, no host read, no atomics.
 * scores / targets / valid: the [rows][T] prefix that eagcn_eval_append filled.  An entry of a classification task is a positive
 * where valid and target == 1, a negative where valid and target == 0, unlabelled otherwise.
 *   eagcn_eval_class_metrics: out[5T + 2] doubles = auc[T] | ap[T] | P[T] | N[T] | bad[T] | mean_auc | mean_ap
 *     auc = roc_curve + auc of sklearn (the Mann-Whitney statistic with average ranks, an exact integer count over 2 P N),
 *     ap = average_precision_score, P / N = labelled positives / negatives, bad = labelled entries whose score is not finite.
 *     A task with P == 0, N == 0 or bad > 0 has auc = ap = NaN; the means run over the other tasks (NaN if there is none).
 *   eagcn_eval_reg_metrics: out[3T + 2] doubles = rmse[T] | mae[T] | count[T] | rmse_all | mae_all over the valid entries, the last
 *     two over all tasks' entries together (train.py:211); NaN where nothing is valid.
 * workspace: at least eagcn_eval_metrics_workspace_bytes(rows, T) bytes, 8-byte aligned, contents irrelevant on entry (every word
 * that is read is written by the call before); with tiles = ceil(rows / 256) and chunks = ceil(rows / 1024) that is
 *     T * tiles * min(chunks, 8) * (256 * 8 + 32)        (0 for rows < 1 or T < 1)
 * -- per task, tile of 256 entries and share of the rows (at most 8 workgroups share them) two 32-bit counts per entry and one
 * 32-byte record.  rows < 2^31 (32-bit counts), T <= 65535. */
size_t eagcn_eval_metrics_workspace_bytes(int64_t rows, int T);
int eagcn_eval_class_metrics(const float* scores, const float* targets, const uint8_t* valid, int64_t rows, int T, void* workspace,
                             size_t workspace_bytes, double* out, void* stream);
int eagcn_eval_reg_metrics(const float* scores, const float* targets, const uint8_t* valid, int64_t rows, int T, void* workspace,
                           size_t workspace_bytes, double* out, void* stream);

/* ---- agreement of a regression with its targets, thresholded metrics of a classification, over the same buffers (csrc/agree.hip):
 * two launches per call, no sort, no host read, no atomics, bit-identical from run to run.  A task's entries are its rows with
 * valid != 0, n their number; comparisons are on the fp32 values (-0 == +0).
 *   eagcn_eval_reg_agreement: out[6T + 4] doubles = r2[T] | pearson[T] | spearman[T] | kendall[T] | count[T] | bad[T] | mean_r2 |
 *   mean_pearson | mean_spearman | mean_kendall.  With s the scores, y the targets and, per entry i, the exact 32-bit pair counts
 *       lt_s = #{j: s_j < s_i}, eq_s = #{j: s_j == s_i} (i included), lt_y, eq_y likewise, S_i = sum_j sgn(s_i - s_j) sgn(y_i - y_j):
 *     r2 = 1 - sum (y - s)^2 / sum (y - mean y)^2                                   (sklearn r2_score(targets, scores))
 *     pearson = sum (s - mean s)(y - mean y) / sqrt(sum (s - mean s)^2 sum (y - mean y)^2)  (scipy pearsonr; its square is the
 *       reference's rsquared, utils.py:714) -- fp64 sums centred per tile of 256 entries, merged in tile order by the pairwise update
 *       of Chan, Golub and LeVeque; no raw sum of squares
 *     spearman = sum ab / sqrt(sum a^2 sum b^2), a_i = 2 lt_s + eq_s - n = 2 (average rank) - (n + 1), b_i likewise: 64-bit integer
 *       products, summed in 64-bit integers for n <= 3 000 000 (where they provably fit), in fp64 in a fixed order beyond
 *     kendall = tau-b = (sum_i S_i / 2) / sqrt((n0 - n1)(n0 - n2)), n0 = n (n - 1) / 2, n1 = sum (eq_s - 1) / 2, n2 = sum (eq_y - 1) / 2,
 *       exact 64-bit integers
 *     count = n, bad = entries whose score or target is not finite.  A task with bad > 0 or n < 2 has NaN in all four.  A constant
 *     scores or targets column (every pair tied) gives NaN for pearson, spearman and kendall, as scipy does; a constant targets
 *     column gives NaN for r2 -- a deviation: sklearn returns 0.0 or 1.0 there.  Each mean runs over the tasks where its metric is not
 *     NaN (NaN if there is none).
 *   eagcn_eval_class_threshold: an entry is labelled where valid and target is 0 or 1, predicted positive where score > threshold.
 *   out[12T + 4] doubles = log_loss[T] | brier[T] | tp[T] | fp[T] | tn[T] | fn[T] | accuracy[T] | precision[T] | recall[T] | f1[T] |
 *   mcc[T] | bad[T] | mean_log_loss | mean_brier | mean_f1 | mean_mcc.
 *     log_loss = -mean(y log p + (1 - y) log(1 - p)) in fp64, p = double(score) clipped to [2^-52, 1 - 2^-52]; brier = mean((p - y)^2);
 *     the counts are exact; a zero denominator gives 0.0 for precision, recall, f1 and mcc (sklearn's value under its default
 *     warning).  bad = labelled entries whose score is not finite.  A task without labelled entries or with bad > 0 is NaN throughout
 *     (bad itself excepted) and stays out of the means.  threshold must not be NaN.
 * workspace (either call): at least eagcn_eval_agreement_workspace_bytes(rows, T) bytes, 8-byte aligned, contents irrelevant on entry
 * (every word that is read is written by the call before); with tiles = ceil(rows / 256) and chunks = ceil(rows / 1024) that is
 *     T * tiles * (min(chunks, 8) * 256 * 20 + 128)        (0 for rows < 1 or T < 1)
 * -- per task and tile of 256 entries one 128-byte record and, per share of the rows (at most 8 workgroups share them), five 32-bit
 * counts per entry.  eagcn_eval_agreement_splits: how many workgroups share a tile's rows in the pair kernel at that shape (1: each
 * lane walks all rows and forms a, b itself; more: the finalize forms them from the summed counts).  rows < 2^31, T <= 65535. */
size_t eagcn_eval_agreement_workspace_bytes(int64_t rows, int T);
int eagcn_eval_agreement_splits(int64_t rows, int T);
int eagcn_eval_reg_agreement(const float* scores, const float* targets, const uint8_t* valid, int64_t rows, int T, void* workspace,
                             size_t workspace_bytes, double* out, void* stream);
int eagcn_eval_class_threshold(const float* scores, const float* targets, const uint8_t* valid, int64_t rows, int T, float threshold,
                               void* workspace, size_t workspace_bytes, double* out, void* stream);

/* ---- atom-representation dump (train.py:213-287) on the device: the rows of the last layer's output whose sub-type lies in the closed
 * range [lo, hi] (1 .. 18 in the reference, train.py:265), appended behind a DEVICE row counter.  Two launches, no host read.
 *   packed / lay / pad_row: the last layer's packed output [T][ld], its layout and the row of the atoms that are not stored (NULL: zeros),
 *     exactly the arguments of eagcn_unpack_rows; F = the layout's exact width.
 *   subtype: int32 [B][N_in], N_in = b->n_logical if it is set, else b->N.  mol_index: int64 [B].
 *   The selected atoms are written in ascending (molecule, atom) order -- the order of the reference's loop over the flattened batch:
 *     X[*count ..][F] (exact columns, no segment padding), sub[*count ..], mol[*count ..]; then *count advances by their number.
 *     A selected atom's row is bit for bit what eagcn_unpack_rows writes at [b][i], atoms beyond nat[b] included.
 *   scratch: B * N_in int32 (contents irrelevant).  cap: rows of X / sub / mol; the caller guarantees *count + B * N_in <= cap < 2^31
 *     (a row that would land at or beyond cap is dropped and *count stops at cap: no memory is overwritten).
 *   eagcn_rep_gather_dense: the same from a dense [B][N][F] tensor, N >= N_in. */
int eagcn_rep_gather(const eagcn_batch* b, const float* packed, const eagcn_layout* lay, const float* pad_row, const int32_t* subtype,
                     int lo, int hi, const int64_t* mol_index, int64_t* count, int32_t* scratch, float* X, int32_t* sub, int64_t* mol,
                     int64_t cap, void* stream);
int eagcn_rep_gather_dense(const float* dense, int B, int N, int F, const int32_t* subtype, int N_in, int lo, int hi,
                           const int64_t* mol_index, int64_t* count, int32_t* scratch, float* X, int32_t* sub, int64_t* mol, int64_t cap,
                           void* stream);

/* ---- k-means (Lloyd) over device rows X[n][ld] (fp32, F <= ld columns used; rows need not be 16-byte aligned), on the caller's stream,
 * no host read, no floating-point atomics: results are bit-identical from run to run.  In fp64 terms
 *     tol_abs = tol * mean_f var_n(X[:, f])                                   (scikit-learn's scaling; eagcn_kmeans_begin)
 *     one iteration: l = argmin_c sum_f (x_f - c_f)^2 (direct differences, lowest index on ties); Cn[c] = mean of the rows with l == c,
 *       or C[c] where there is none (an EMPTY CLUSTER KEEPS ITS CENTROID; scikit-learn relocates it); shift = sum (Cn - C)^2; C = Cn;
 *       n_iter += 1; done when no label changed against the iteration before, or shift <= tol_abs     (eagcn_kmeans_iterate)
 *     labels = argmin against the final C, inertia = the sum of the minimal distances, counts per cluster     (eagcn_kmeans_finish)
 *   eagcn_kmeans_iterate enqueues ONE iteration (three launches); every launch returns at once when `done` is set, so iterations
 *   enqueued behind convergence change nothing and the host may read `done` as rarely as it likes.  Distances are fp32 sums in a fixed
 *   order, cluster sums fp64 (per workgroup in LDS, then over the workgroups' slabs in slab order), centroids stored in fp32.
 *   Envelope: 1 <= k <= 16, 1 <= F <= 1024, k * pad4(F) <= 8192, k <= n < 2^31, ld >= F; anything else is refused before any HIP call.
 *   workspace: 256-byte aligned, at least eagcn_kmeans_workspace_bytes(n, F, k) bytes, written by eagcn_kmeans_begin.  With
 *   a(x) = x rounded up to a multiple of 256, F4 = pad4(F), G = min(ceil(n / 64), 768) and kk = max(k, 2) it is, in this order,
 *       256            state: int32 done | n_iter | changed | n_empty, then double inertia | shift | tol_abs (bytes 0 .. 39)
 *       a(4 k F)       centroids [k][F] fp32
 *       256            counts [k] int32 (of the last iteration; of the final labels after eagcn_kmeans_finish)
 *       a(4 n)         labels [n] int32
 *       a(4 n)         minimal squared distances [n] fp32 (of the last assignment pass)
 *       a(8 G kk F4) + a(64 G) + a(4 G) + a(8 G) + 8192      per-workgroup sums / counts / changed labels / inertia, block partials
 *   (0 for arguments outside the envelope).
 *   eagcn_kmeans_assign: the assignment pass alone against any centres [k][F]: labels [n] and minimal squared distances [n] (the
 *   D^2 weights of a k-means++ seeding); the workspace (sized for this k or a larger one) is scratch. */
size_t eagcn_kmeans_workspace_bytes(int64_t n, int F, int k);
int eagcn_kmeans_begin(const float* X, int64_t n, int F, int ld, int k, const float* init, double tol, void* workspace,
                       size_t workspace_bytes, void* stream);
int eagcn_kmeans_iterate(const float* X, int64_t n, int F, int ld, int k, void* workspace, size_t workspace_bytes, void* stream);
int eagcn_kmeans_finish(const float* X, int64_t n, int F, int ld, int k, void* workspace, size_t workspace_bytes, void* stream);
int eagcn_kmeans_assign(const float* X, int64_t n, int F, int ld, const float* centers, int k, int32_t* labels, float* mind,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- exact t-SNE and PCA of device rows (the reference's tsnes.py / mol_to_vec_plot.py; csrc/embed.hip), on the caller's stream, no
 * floating-point atomics, every sum folded in a fixed order: results are bit-identical from run to run.  Semantics are those of
 * sklearn.manifold.TSNE(method='exact', n_components=2, metric='euclidean') and sklearn.decomposition.PCA(svd_solver='full') (1.7.2)
 * with the deviations marked DEVIATION below.  Envelope: X fp32 with unit column stride, ld >= F, 1 <= F <= 1024; t-SNE and distances
 * 17 <= n <= 32768; PCA 17 <= n < 2^31, k <= min(8, F) components.  Anything else returns EAGCN_ERR_ARG before any HIP call.
 *
 *   eagcn_sqdist: D[n][n] fp32, D_ij = sum_f (x_if - x_jf)^2 as direct differences in a fixed order (never the Gram identity); the
 *     diagonal is exactly 0 and D exactly symmetric.
 *   eagcn_tsne_affinities: scikit-learn's _binary_search_perplexity and _joint_probabilities.  Per row i, in fp64 on the fp32 distances:
 *     beta = 1, bisected for at most 100 evaluations of  s = sum_{j != i} exp(-D_ij beta) (1e-8 where it is 0),
 *     H = log s + beta sum_j D_ij exp(-D_ij beta) / s, stopping when |H - log perplexity| <= 1e-5; C_ij = exp(-D_ij beta) / s.  Then
 *     P_ij = max((C_ij + C_ji) / sum(C + C^T), DBL_EPSILON), P_ii = 0, stored in fp32 as P[n][ldp]: ldp a multiple of 4, >= n, P 16-byte
 *     aligned; the columns n .. ldp - 1 are written as 0.  betas[n] fp64: the precision of the LAST EVALUATION of every row;
 *     steps[n] int32 (may be NULL): evaluations made.  D is read as [n][n]; 0 < perplexity < n.  The workspace (as below) is scratch.
 *   eagcn_tsne_gradient: one evaluation of the objective at Y[n][2] (fp32, 16-byte aligned) with the exaggeration alpha:
 *     w_ij = 1 / (1 + |y_i - y_j|^2); per row the fp32 sums over j != i  a_i = sum alpha P_ij w_ij (y_i - y_j),
 *     r_i = sum w_ij^2 (y_i - y_j), z_i = sum w_ij; Z = sum_i z_i in fp64; grad_i = 4 (a_i - r_i / Z) -> grad[n][2] fp32.
 *     out[3] doubles = Z | KL | |grad|_2, where, if compute_kl, KL = sum_{i != j} q log max(q, eps) + sum q log(1 + |y_i - y_j|^2)
 *     + log Z sum q with q = alpha P_ij and eps = DBL_EPSILON, in fp64 (NaN otherwise).  DEVIATION: scikit-learn clamps Q_ij = w_ij / Z
 *     below at eps inside the logarithm; this form does not.
 *   eagcn_tsne_begin / iterate / finish: scikit-learn's two-stage _gradient_descent on the device.  Iteration it (0-based) runs with
 *     alpha = early_exaggeration and momentum 0.5 while it < 250, then alpha = 1, momentum 0.8 and update / gains reset to 0 / 1 at
 *     it = 250.  Element-wise in fp32, without contraction:  gains += 0.2 where update * grad < 0, else gains *= 0.8; gains =
 *     max(gains, 0.01); grad *= gains; update = momentum update - learning_rate grad; Y += update.  Every 50th iteration
 *     ((it + 1) % 50 == 0) the divergence (against alpha P, as scikit-learn reports it) and the norm of the GAINED gradient are formed:
 *     a divergence below the best one so far is recorded with its iteration, otherwise the fit stops when it - best_iter exceeds the
 *     window (250 while it < 250, n_iter_without_progress after; the best is reset at it = 250); it stops when the norm is at most
 *     min_grad_norm; and it stops when n_iter reaches max_iter.  DEVIATIONS: a stop in the first stage ends the FIT (scikit-learn goes
 *     on with the second stage); n_iter counts iterations made (scikit-learn's n_iter_ is the index of the last one); max_iter may
 *     be below 250.  eagcn_tsne_iterate enqueues ONE iteration (four launches); every launch returns at once when `done` is set, so
 *     iterations enqueued behind a stop change nothing and the host may read `done` as rarely as it likes.  eagcn_tsne_finish leaves
 *     in last_kl the divergence of the FINAL embedding against the un-exaggerated P (DEVIATION: scikit-learn's kl_divergence_ is the
 *     value of its last check).
 *   workspace: 256-byte aligned, at least eagcn_tsne_workspace_bytes(n) bytes (0 outside the envelope), written by eagcn_tsne_begin:
 *       bytes 0 .. 63   state: int32 done | n_iter | reason | best_iter, double best_err | last_kl | last_gnorm,
 *                       float early_exaggeration | learning_rate, int32 max_iter | n_iter_without_progress, double min_grad_norm
 *       bytes 256 ..    the embedding Y [n][2] fp32, then update [n][2] and gains [n][2] fp32, each part rounded up to a multiple of
 *                       256 bytes; the rest is internal.
 *   eagcn_pca_cov: mean[F] fp64 (column sums in fp64, per workgroup and then over the workgroups in order) and cov[F][F] fp64 =
 *     (X - mean)^T (X - mean) / (n - 1): products of the fp32-centred rows summed in fp32 over 256 rows, then in fp64; exactly
 *     symmetric.  workspace: 256-byte aligned, eagcn_pca_workspace_bytes(n, F) bytes.  The eigen-decomposition is the caller's.
 *   eagcn_pca_project: out[n][k] fp32 = (X - mean) components^T, components [k][F] fp32. */
#define EAGCN_TSNE_STOP_MAX_ITER 1
#define EAGCN_TSNE_STOP_NO_PROGRESS 2
#define EAGCN_TSNE_STOP_GRAD_NORM 3
int eagcn_sqdist(const float* X, int64_t n, int F, int ld, float* D, void* stream);
size_t eagcn_tsne_workspace_bytes(int64_t n);
int eagcn_tsne_affinities(const float* D, int64_t n, double perplexity, float* P, int ldp, double* betas, int32_t* steps, void* workspace,
                          size_t workspace_bytes, void* stream);
int eagcn_tsne_gradient(const float* P, int ldp, const float* Y, int64_t n, float alpha, int compute_kl, float* grad, double* out,
                        void* workspace, size_t workspace_bytes, void* stream);
int eagcn_tsne_begin(const float* P, int ldp, int64_t n, const float* Y0, float early_exaggeration, float learning_rate, int max_iter,
                     int n_iter_without_progress, double min_grad_norm, void* workspace, size_t workspace_bytes, void* stream);
int eagcn_tsne_iterate(const float* P, int ldp, int64_t n, void* workspace, size_t workspace_bytes, void* stream);
int eagcn_tsne_finish(const float* P, int ldp, int64_t n, void* workspace, size_t workspace_bytes, void* stream);
size_t eagcn_pca_workspace_bytes(int64_t n, int F);
int eagcn_pca_cov(const float* X, int64_t n, int F, int ld, double* mean, double* cov, void* workspace, size_t workspace_bytes, void* stream);
int eagcn_pca_project(const float* X, int64_t n, int F, int ld, const double* mean, const float* components, int k, float* out,
                      void* stream);

/* ---- exact nearest neighbours of device rows and the rank of given candidates among them (csrc/knn.hip): the similarity search the
 * reference's mol_to_vec_plot.py does by eye, and what a trustworthiness score of an embedding needs.  On the caller's stream, no host
 * read, no floating-point atomics, and no n x n or m x n buffer: the 64 x 64 distance tiles are consumed in registers.
 *   The distance of query row q and data row x_j:  d(q, j) = fmaf(t, t, acc) folded over c = 0 .. F - 1 from acc = 0.0f, t = q[c] - x_j[c]
 *     in fp32 -- one accumulator per pair, in column order: the bits of eagcn_sqdist for that pair (never the Gram identity).
 *   The order: candidates ascend by (d, j): equal distances by the smaller row index; a NaN distance ranks behind every number (ties
 *     again by index).  A total order: results are unique, bit-identical from run to run and THE SAME FOR EVERY VALUE OF slabs.
 *   eagcn_knn: row i of idx / dist [m][k] holds the k first candidates of query row i of Q [m][ldq] among the rows of X [n][ldx] and
 *     their distances (a NaN distance is stored as the quiet NaN 0x7FC00000).  Q may be X.  exclude_self = 1 (only with m == n) removes
 *     candidate j == i BY INDEX: a duplicate of row i elsewhere stays a neighbour at distance 0.
 *   eagcn_knn_rank: for j = cand[i][c] (int32 [n][k], device data):  rank[i][c] = 1 + #{ l != i : (d(i, l), l) < (d(i, j), j) }, the
 *     1-based position of j among the neighbours of row i of X; -1 for a candidate equal to i or outside 0 .. n - 1 (which is never
 *     used as an address).
 *   Envelope: 1 <= F <= 1024, 1 <= k <= EAGCN_KNN_MAX_K, k <= n - exclude_self (eagcn_knn), 1 <= n < 2^31, 1 <= m < 2^31, ld >= F, rows
 *     4-byte aligned, slabs >= 0; anything else returns EAGCN_ERR_ARG before any HIP call.
 *   slabs: the data rows are cut into tiles of 64, dt = ceil(n / 64), and the tiles among S workgroups per tile of 64 query rows, so that
 *     few queries still fill the chip.  With qt = ceil(m / 64) (eagcn_knn_rank: m = n):
 *         S0 = slabs, or for slabs == 0  min(ceil(4096 / qt), 64);   S1 = max(1, min(S0, 4096, dt));   per = ceil(dt / S1) tiles a slab;
 *         S = ceil(dt / per)   (no slab is empty).
 *   workspace: 256-byte aligned, at least eagcn_knn_workspace_bytes(n, m, F, k, slabs) = a(8 S m k) + a(8 m k) bytes, a(x) = x rounded
 *     up to a multiple of 256 (0 for arguments outside the envelope); contents are scratch.  eagcn_knn keeps the slabs' sorted lists of
 *     64-bit keys (distance bits << 32 | index) in the first part and merges them in a second launch; eagcn_knn_rank keeps int32 counts
 *     per slab there and the candidates' keys in the second part (three launches). */
#define EAGCN_KNN_MAX_K 128
size_t eagcn_knn_workspace_bytes(int64_t n, int64_t m, int F, int k, int slabs);
int eagcn_knn(const float* X, int64_t n, int F, int ldx, const float* Q, int64_t m, int ldq, int k, int exclude_self, int slabs,
              int32_t* idx, float* dist, void* ws, size_t ws_bytes, void* stream);
int eagcn_knn_rank(const float* X, int64_t n, int F, int ld, const int32_t* cand, int k, int slabs, int32_t* rank, void* ws,
                   size_t ws_bytes, void* stream);

/* ---- scores of a clustering of device rows (csrc/silhouette.hip): the silhouette coefficient of every row, and the cluster moments from
 * which the Davies-Bouldin and Calinski-Harabasz indices follow -- the numbers behind the confusion matrix the reference's
 * kmeans_atomrep.py reads by eye.  On the caller's stream, no host read, no floating-point atomics, no n x n buffer; the distance front end
 * is the 64 x 64 tile of eagcn_knn (csrc/dist_tile.h), consumed in registers.
 *   labels [n] int32, device data.  A row whose label is outside 0 .. k - 1 takes no part: it is neither scored nor a member of a cluster.
 *   eagcn_silhouette: sklearn.metrics.silhouette_samples(metric='euclidean').
 *     d(i, j) = the correctly rounded fp32 square root of the fp32 squared distance of eagcn_sqdist / eagcn_knn (one fmaf chain in column
 *       order; d(i, i) is an exact 0).
 *     S[i][c] = the sum of d(i, j) over the rows j of cluster c, in fp64.  The rows are brought into cluster order (row index ascending
 *       inside a cluster; a permutation, X is not copied) and every cluster is cut into data tiles of 64 of its own rows, T <= tb =
 *       ceil(n / 64) + k tiles in all.  The tiles are cut into slabs by the rule of eagcn_knn with dt = tb and qt = ceil(n / 64):
 *           S0 = slabs, or for slabs == 0  min(ceil(4096 / qt), 64);   S1 = max(1, min(S0, 4096, tb));   per = ceil(tb / S1);   S = ceil(tb / per)
 *       (slabs behind the last real tile do nothing).  Within a slab a thread adds its four distances of a query row and a tile in
 *       column order to one fp64 accumulator per (row, cluster); the 16 threads of a query row are added by a fixed xor tree when the
 *       cluster changes or the slab ends; the slabs are added in slab order.  The order is a function of labels, n and S alone:
 *       results are bit-identical from run to run, and equal for every value of slabs up to the rounding of fp64 sums.
 *     With cnt[c] the rows of cluster c and own = labels[i]:  a = S[i][own] / (cnt[own] - 1),  b = min over c != own, cnt[c] > 0 of
 *       S[i][c] / cnt[c],  samples[i] = (b - a) / max(a, b);  0 where cnt[own] == 1 and where the quotient is no number (scikit-learn's
 *       nan_to_num);  NaN for a row outside the labelling.
 *     cluster_mean[c] = the mean sample of cluster c (NaN for an empty one): per thread in row order, then a fixed tree.  counts[c] = cnt[c].
 *     stats[4] = the mean sample over the scored rows (the cluster sums in cluster order; NaN when fewer than two clusters are non-empty)
 *       | rows scored | non-empty clusters | rows outside the labelling.
 *   eagcn_cluster_moments: centers [k][F] = the fp64 centroids (sums of the fp32 rows in cluster order, cut into R = min(ceil(n / 8192), 16)
 *     stretches per cluster that are added in order; NaN for an empty cluster);  scatter[c] = the mean over the cluster's rows of the
 *     fp64 Euclidean distance to its centre (differences in fp64; NaN for an empty cluster);  wss[c] = the sum of the squared distances;
 *     counts[c].  One read of X for the centroids and one for the distances.
 *   Envelope: 1 <= F <= 1024, 1 <= n < 2^31, ld >= F, 2 <= k <= EAGCN_SIL_MAX_K, rows 4-byte aligned, slabs >= 0; anything else returns
 *     EAGCN_ERR_ARG before any HIP call.
 *   workspace: 256-byte aligned, contents are scratch; 0 bytes for arguments outside the envelope.  With a(x) = x rounded up to a
 *     multiple of 256, W0 = min(ceil(n / 1024), 1024) waves of the counting sort, chunk = ceil(n / W0) rounded up to a multiple of 64,
 *     W = ceil(n / chunk), and  sort = a(4 W (k + 1)) + a(4 W k) + 2 a(4 (k + 1)) + a(4 n)  (histograms, offsets, cluster and tile
 *     offsets, the permutation):
 *         eagcn_silhouette_workspace_bytes(n, F, k, slabs) = sort + a(16 tb) + a(8 k) + a(8 S n k)      (tiles, cluster sums, part [S][n][k])
 *         eagcn_cluster_moments_workspace_bytes(n, F, k)   = sort + a(8 R k F) + a(16 R k) */
#define EAGCN_SIL_MAX_K 256
size_t eagcn_silhouette_workspace_bytes(int64_t n, int F, int k, int slabs);
int eagcn_silhouette(const float* X, int64_t n, int F, int ld, const int32_t* labels, int k, int slabs, double* samples, double* cluster_mean,
                     int64_t* counts, double* stats, void* ws, size_t ws_bytes, void* stream);
size_t eagcn_cluster_moments_workspace_bytes(int64_t n, int F, int k);
int eagcn_cluster_moments(const float* X, int64_t n, int F, int ld, const int32_t* labels, int k, double* centers, double* scatter,
                          double* wss, int64_t* counts, void* ws, size_t ws_bytes, void* stream);

/* Matrix-core path of the layer products (the reference's torch.mm and its two autograd products, layers.py:40):
 *   0 = fp32 MFMA: exact fp32 products, a k-ordered fmaf chain (csrc/gemm3.hip);
 *   1 = every fp32 operand split into three bf16 pieces by the CONSUMER on its way into LDS, six bf16 MFMA products
 *       accumulated in fp32 (csrc/gemm_x6.h; kept for comparison);
 *   2 = operands rounded to bf16 by the consumer, ONE product (csrc/gemm_x6.h; NOT the parity path);
 *   3 = fp32-equivalent products at the bf16 matrix rate (exact operand split, piece products to 3 x 2^-24 |a b|, fp32 accumulate): the PRODUCERS of a matrix (BatchNorm apply, transposed aggregation,
 *       parameter packing) write it as three bf16 planes, the products run from them by LDS-DMA (csrc/gemm_bx3.hip);
 *   4 = the same kernels on ONE bf16 plane (operands rounded to bf16, fp32 accumulation): BASELINE configs[1] "bf16".
 * The mode is read when a model's buffers are sized: set it before the first forward.  Returns the previous mode. */
int eagcn_set_gemm_mode(int mode);

/* ---- the plane GEMM of modes 3 / 4 as stand-alone entry points (tests, tools/bx3_bench.cpp) -----------------------------
 * PLANE IMAGE of a matrix with `rows_cap` rows and ld columns (ld a multiple of 8): the columns are cut into panels of 32, a panel
 * holds the rows_cap rows of its 32 columns at 64 bytes per row, and the four 16-byte chunks of a row are XOR-swizzled by the row:
 *     element (r, c) at  ((c >> 5) * rows_cap + r) * 32 + ((((c >> 3) & 3) ^ ((r >> 2) & 3)) << 3) + (c & 7)      [bf16 elements]
 * (the layout the GEMM's LDS-DMA copies verbatim: every 1 KB it moves is contiguous); eagcn_bx3_plane_elems(rows_cap, ld) elements.
 * eagcn_bx3_split writes the images of a row-major fp32 matrix [rows][ld], rows <= rows_cap: np = 3: x = x0 + x1 + x2 exactly (each
 * piece the bf16 nearest to what the pieces before it left over), np = 1: round to nearest even; plane q at planes + q *
 * plane_stride (elements, >= eagcn_bx3_plane_elems, a multiple of 8); planes 16-byte aligned. */
size_t eagcn_bx3_plane_elems(int rows_cap, int ld);
int eagcn_bx3_split(const float* x, int rows, int ld, uint16_t* planes, size_t plane_stride, int rows_cap, int np, void* stream);
/* tn = 0: C[M,N] = A[M,K].B[N,K]^T (images of A [a_rows >= M][lda >= K] and B [b_rows >= N][ldb >= K], K a multiple of 8);
 * tn = 1: C[M,N] = A[K,M]^T.B[K,N] (images [a_rows >= K][lda >= M], [b_rows >= K][ldb >= N]) as k-chunk slabs C + z * slab,
 *         z < eagcn_bx3_used_splits(splits, M, N, K) (at least 768 and at most 4096 rows of K per chunk; slabs beyond that count are
 *         NOT written), whose sum is the product. */
int eagcn_bx3_used_splits(int splits, int M, int N, int K);
/* Two kernels serve these entry points (csrc/bx3.h): 128 x 128 tiles, 4 compute + 2 loader waves (launches of about one wave of tiles)
 * and 256 x 128 tiles, 8 compute waves = two per SIMD (csrc/gemm_bx3w.hip; launches with several waves of tiles).  mode -1: picked per
 * launch by its size (default; EAGCN_BX3_WIDE in the environment presets it) | 0: always the first | 1: always the second.
 * Returns the previous setting.  The used-splits queries follow the setting. */
int eagcn_set_bx3_wide(int mode);
/* The BatchNorm backward of a Concate top layer behind the fused read-out (model engine, training, local BatchNorm, bond-list route):
 * 1 (default; EAGCN_TOP_BN_SUMS=0 in the environment presets 0): its column sums are taken over the molecules from two per-molecule
 * sums of the read-out, no pass over the rows and no stored dH; the transposed aggregation gathers the read-out gradient per molecule
 * | 2: the same, but that gradient is first written out as rows (view widths that are no multiples of four take this form anyway)
 * | 0: the reduction pass over the rows.  Returns the previous setting.
 * For tests and A/B runs; set it between steps (a forward and its backward must see the same value), before a graph is captured. */
int eagcn_set_top_bn_sums(int on);
/* The BatchNorm backward of a Concate layer BELOW a layer whose backward products run as the plane-GEMM pair (model engine, training,
 * local BatchNorm, one stream, bond-list route): 1 (default; EAGCN_HIDDEN_BN_SUMS=0 in the environment presets 0): the launch of the dX
 * product of the layer above (128 x 128 kernel) forms this layer's dH and the column sums of dH and dH xhat in a tail pass, no
 * reduction launch over the rows
 * | 0: the reduction pass.  Returns the previous setting.  For tests and A/B runs; set it between steps, before a graph is captured
 * (a captured graph keeps its route). */
int eagcn_set_hidden_bn_sums(int on);
/* How many layer backward calls took that route since the last reset (a captured call counts when it is captured); reset != 0 clears
 * the count.  For tests. */
long eagcn_hidden_bn_sums_taken(int reset);
/* The weight gradient of a layer of at most 32 input columns whose input gradient is not asked for (the first layer of a model in
 * training; route values BWD_TILED_SEPARATE with the bond-list aggregation and its edge gradients, exact fp32 products): 1 (default;
 * EAGCN_FIRST_LAYER_FUSED=0 in the environment presets 0): formed in the epilogue of the transposed aggregation, which then neither
 * stores dP nor is followed by a product launch; the route values eagcn_layer_route shows stay what they are
 * | 0: dP is stored and the split-K product is a launch of its own.  Returns the previous setting.  For tests and A/B runs; set it
 * between steps, before a graph is captured (a captured graph keeps its route). */
int eagcn_set_first_layer_fused(int on);
/* How many layer backward calls took that route since the last reset (a captured call counts when it is captured); reset != 0 clears
 * the count.  For tests. */
long eagcn_first_layer_fused_taken(int reset);
/* ... and of the last such call: out[0] = slabs written (the launch's y extent), out[1] = 1 when they live in the dP area of the
 * scratch block (more slabs than the dWcat area holds), out[2] = the y extent the launch would have had without the slab capacity's
 * cap (larger than out[0]: workgroup rows walk several blocks).  For tests. */
void eagcn_first_layer_fused_last(int32_t out[3]);
/* ... of the TN problem (M, N, K) of eagcn_gemm_bx3_pair: its chunks are sized against the NT problem (M0, N0, K0) of the launch */
int eagcn_bx3_pair_used_splits(int splits, int M, int N, int K, int M0, int N0, int K0);
int eagcn_gemm_bx3(int tn, int M, int N, int K, const uint16_t* A, size_t a_pstride, int lda, int a_rows, const uint16_t* B,
                   size_t b_pstride, int ldb, int b_rows, float* C, int ldc, int splits, size_t slab, int np, void* stream);
/* an NT product and a TN product (the dX / dW pair of a layer's backward) in ONE persistent launch */
int eagcn_gemm_bx3_pair(int M0, int N0, int K0, const uint16_t* A0, size_t a0_pstride, int lda0, int a0_rows, const uint16_t* B0,
                        size_t b0_pstride, int ldb0, int b0_rows, float* C0, int ldc0, int M1, int N1, int K1, const uint16_t* A1,
                        size_t a1_pstride, int lda1, int a1_rows, const uint16_t* B1, size_t b1_pstride, int ldb1, int b1_rows,
                        float* C1, int ldc1, int splits, size_t slab, int np, void* stream);

/* ---- plain fp32 MFMA GEMM (head / tests) ------------------------------------------------------ */
/* C[M,N] = op(A).op(B); ta/tb: 0 = as stored, 1 = transposed; leading dimensions in floats */
int eagcn_gemm_f32(int ta, int tb, int M, int N, int K, const float* A, int lda, const float* B,
                   int ldb, float* C, int ldc, void* stream);
/* the same product with one extent read from device memory (M / K are then capacities): which = 0 the rows of A and C,
   which = 2 the reduction length -- products over the packed rows of a capacity-sized batch index (eagcn_batch.meta[0]);
   any extent in any of the four forms: nothing of either operand at k >= extent enters the product, extent 0 gives zeros */
int eagcn_gemm_f32_dev(int ta, int tb, int M, int N, int K, const float* A, int lda, const float* B,
                       int ldb, float* C, int ldc, const int32_t* extent_dev, int which, void* stream);

/* ---- persistent, balanced ("stream-K") form of the same products: the kernel the layer products run on ---------
 * A launch is a fixed grid; the iteration space (tiles x k-tiles, counted on the device) is cut into equal ranges, tiles
 * cut between workgroups are finished in the launch (no split-K slabs, no reduction launch).  Needs 16-byte aligned
 * operands, leading dimensions / contiguous extents that are multiples of 4, and eagcn_gemm_sk_workspace_bytes() bytes
 * of device scratch (need not be initialised).  (ta,tb) in {(0,0), (0,1), (1,0)}. */
size_t eagcn_gemm_sk_workspace_bytes(void);
int eagcn_gemm_f32_sk(int ta, int tb, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C,
                      int ldc, void* workspace, size_t workspace_bytes, void* stream);
/* C0[M0,N0] = A0[M0,K0].B0[N0,K0]^T and C1[M1,N1] = A1[K1,M1]^T.B1[K1,N1] in ONE launch: the two autograd products of
 * reference layers.py:40 (dX = dP.W^T, dW = X^T.dP) */
int eagcn_gemm_pair_sk(int M0, int N0, int K0, const float* A0, int lda0, const float* B0, int ldb0, float* C0, int ldc0,
                       int M1, int N1, int K1, const float* A1, int lda1, const float* B1, int ldb1, float* C1, int ldc1,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The same pair on the XCD-local schedule used by the layer backward: the long reduction of the second product is split across
 * the eight XCDs (each XCD reads only its own eighth of the K rows, for both products); C1 receives 8 partial slabs, `slab`
 * floats apart, whose sum (in slab order) is the product. */
int eagcn_gemm_pair_sk_slabs(int M0, int N0, int K0, const float* A0, int lda0, const float* B0, int ldb0, float* C0, int ldc0,
                             int M1, int N1, int K1, const float* A1, int lda1, const float* B1, int ldb1, float* C1, int ldc1,
                             size_t slab, void* workspace, size_t workspace_bytes, void* stream);
/* host-side mirror of that schedule's partition: a[9] = row-block (64 rows) boundaries of the first product per XCD segment,
 * c[9] = k-step (16 rows) boundaries of the second; wgs = 0: the library's grid */
int eagcn_gemm_sk_plan(int M0, int N0, int K0, int M1, int N1, int K1, int wgs, int* a, int* c);
int eagcn_gemm_sk_timeouts(void);   /* hand-offs that gave up waiting since load (must stay 0); synchronising device read */
/* A hand-off that times out is FATAL, never silent: the owner wave poisons its output tile with NaN and stores 1 into a
 * sticky word in host-mapped memory.  eagcn_gemm_sk_failed() reads that word without synchronising (the graph-replay host
 * loop polls it every step, eagcn_amd/graph.py); every eagcn_model_* / eagcn_layer_* entry point returns EAGCN_ERR_HIP while
 * it is set.  eagcn_gemm_sk_reset_failed() clears it; eagcn_gemm_sk_inject_failure() sets it (test hook). */
int eagcn_gemm_sk_failed(void);
void eagcn_gemm_sk_reset_failed(void);
void eagcn_gemm_sk_inject_failure(void);

/* ---- optional per-kernel-class timing with HIP events on the launch stream (bench.py roofline) -- */
void eagcn_prof_enable(int on);
void eagcn_prof_reset(void);
int eagcn_prof_ntags(void);
const char* eagcn_prof_tag_name(int tag);
/* sums event-pair durations of class `tag` since the last reset (waits for them); work = summed
 * algorithmic flops for the gemm class */
int eagcn_prof_read(int tag, double* total_ms, double* work, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* EAGCN_HIP_H */
