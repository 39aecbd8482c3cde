// Argument blocks and launchers shared between the HIP translation units.
#pragma once
#include "bx3.h"
#include "common.h"

namespace eagcn {

struct AggArgs {
    eagcn_batch bt;
    ViewCols vc;
    const float* src; int lds;   // P (forward) or dY' (transposed) [T][lds]
    float* dst; int ldd;         // Y' (forward) or dP (transposed)
    const float* sig;            // [K][256] sigmoid(att weight) by bond code, entry 0 = 0
    const float* rsig;           // [K] sigmoid(self_r)
    float* rscale;               // [K][T] m_i/rowsum_i: written by forward, read by transposed
    double* stats;               // forward: [grid.x][Fp][2] partial (sum y, sum y^2)
    int nchunk;
    int cpw = 1;                 // lagg.hip: consecutive 32-column chunks a workgroup takes per block (nchunk then counts chunk GROUPS)
    int xcd = 0;                 // wave-per-tile variant: tiles handed out so that an XCD works on CONTIGUOUS tiles (agg.hip)
    // input-only backward, Concate layer in eval mode (lagg_in.hip, with w_aw set): `src` is the upstream gradient at the PACKED column and
    // dH = src m_i [relu'(sc Y' + sh) > 0] (bn_bwd_reduce_kernel<false,...> with c1 = c2 = 0); w_aw is not read then.  (Here, in the
    // padding in front of `planes`: the argument block of the other forms keeps its layout.)  Also the staging of lagg_top.hip: a Concate
    // top layer in training mode whose dH is never stored, with the dropout draw and the means of the BatchNorm backward
    bool w_rowm = false;
    // ... with the edge gradients (lagg_top.hip): `src` is the per-MOLECULE gradient [B][lds] at the EXACT column (dg / size of the
    // read-out, HeadTopSums.dge) and a row gathers its molecule's -- no T x Fp upstream matrix exists at all
    bool w_gather = false;
    BxOut planes = {nullptr, 0, 0, 0};   // transposed: dP leaves as bf16 planes INSTEAD of the fp32 matrix (only the plane GEMMs read it)
    // transposed, lagg.hip only: `src` holds dH (the BatchNorm's upstream gradient), not dY': the BatchNorm backward's second pass
    //     dY' = sc (dH - c1 - (Y' - mu) inv c2)      (layer.hip bn_bwd_apply_kernel)
    // is evaluated while the rows are staged (bn = the layer's [4][Fp] table, cc = [2][Fp] {c1, c2}, Y' = EdgeArgs.Y); null: src is dY'
    const float* bn_tab = nullptr; const float* bn_cc = nullptr; int bn_fp = 0;
    // ... and for a Weighted_sum layer (w_aw != null, round 6) `src` is the layer's UPSTREAM gradient [T][lds], K times narrower than dH:
    //     dH[r][off_k + f] = src[r][f] ave_w[off_k + f] dropout(r, off_k + f) [relu'(sc Y' + sh) > 0]   (layer.hip bn_bwd_reduce_kernel<true,...>)
    // is re-formed in the staging as well -- neither dH nor dY' of the layer (T x K F floats each) ever exists in memory
    const float* w_aw = nullptr;                 // [Fp] the view weight per packed column (colp row CP_AVEW)
    int w_drop = 0; uint32_t w_thr = 0; float w_inv_keep = 1.0f; uint64_t w_seed = 0; const uint64_t* w_seed_dev = nullptr;
    // transposed with the edge gradients, lagg_dw.hip (a first layer whose input gradient nobody asks for): dP is not stored; the
    // weight gradient fx^T . dP leaves as one slab per workgroup row, dw [dw_ny][fx_ld][Fp] (fx: the layer's input [T][fx_ld],
    // fx_ld <= 32); the launch's y extent is dw_ny, every slab is written whatever the block count
    const float* fx = nullptr; int fx_ld = 0; float* dw = nullptr; size_t dw_slab = 0; int dw_ny = 0;
};
// dropout of an activation as the kernels draw it: keep where hash(seed, element) >= thr, scaled by inv_keep (seed_dev: the seed
// read on the device instead).  The ONE place threshold and scale are derived from the probability
struct DropArgs { int on; uint32_t thr; float inv_keep; uint64_t seed; const uint64_t* seed_dev; };
inline DropArgs drop_args(float p, bool training, uint64_t seed, const uint64_t* seed_dev) {
    const double thr = (double)p * 4294967296.0;
    return DropArgs{(training && p > 0.0f) ? 1 : 0, (uint32_t)(thr < 4294967295.0 ? thr : 4294967295.0), 1.0f / (1.0f - p), seed, seed_dev};
}
inline void agg_set_drop(AggArgs& a, const DropArgs& d) {
    a.w_drop = d.on; a.w_thr = d.thr; a.w_inv_keep = d.inv_keep; a.w_seed = d.seed; a.w_seed_dev = d.seed_dev;
}
int agg_grid_x(const eagcn_batch* b);
bool agg_ksplit(const eagcn_batch* b);
int launch_agg(AggArgs a, bool trans, hipStream_t s);
// the same operator over the bond lists of the index, LDS-staged (lagg.hip): a workgroup owns a ROW BLOCK of whole molecules (eagcn_batch.blk) x a 32-column chunk of one view
constexpr int LAGG_RB = 256;                 // packed rows per block (= the largest molecule the path takes)
constexpr int LAGG_MAXM = 16;                // molecules per block
struct EdgeArgs;
int lagg_parts();
bool lagg_wfuse();                           // Weighted_sum layers: the transposed kernel re-forms dH from the upstream gradient (EAGCN_LAGG_WFUSE=0: off)
bool lagg_use(const eagcn_batch* b, int dir, bool absorbs_bn, const ViewCols* vc = nullptr);   // this batch takes that path (policy per direction + the index carries bond lists and row blocks)
bool lagg_wanted(int B, int N, int structure);
int lagg_block_rows(const eagcn_batch* b);     // rows per row block for batches of this shape (index_blocks_kernel; <= LAGG_RB)
int lagg_slabs(const eagcn_batch* b);        // capacity of its BatchNorm partial slabs (one per row block; meta[NBLK] of them are live)
int launch_lagg_fwd(AggArgs a, hipStream_t s);
// transposed aggregation + edge gradients (e.atomic must be set); edge = false: the aggregation alone (input-only backward)
int launch_lagg_bwd(AggArgs a, const EdgeArgs& e, hipStream_t s, bool edge = true);
// lagg_in.hip: the edge = false instantiations, on the grid launch_lagg_bwd computed
int launch_lagg_bwd_input(const AggArgs& a, const EdgeArgs& e, dim3 grid, hipStream_t s);
// lagg_top.hip: the row-mask staging WITH the edge gradients (Concate top layer whose dH is never stored), same grid
int launch_lagg_bwd_top(const AggArgs& a, const EdgeArgs& e, dim3 grid, hipStream_t s);
// lagg_dw.hip: the plain transposed kernel with the weight gradient in its epilogue (AggArgs.dw), same grid with y = AggArgs.dw_ny
int launch_lagg_bwd_dw(const AggArgs& a, const EdgeArgs& e, dim3 grid, hipStream_t s);
int lagg_bwd_grid_y(const eagcn_batch* b, const ViewCols& vc);    // y extent launch_lagg_bwd gives its grid for this batch

struct EdgeArgs {
    eagcn_batch bt;
    ViewCols vc;
    const float* dY; const float* Y; const float* P; int ld;
    const float* sig; const float* rsig; const float* rscale;
    double* datt;                // [grid.x][K][EDGE_SLAB] per-workgroup partials: 256 codes + self term ...
    int atomic;                  // ... or (atomic != 0) [EDGE_COPIES][K][EDGE_SLAB] shared accumulators (fp64 atomics)
    int xcd = 0;                 // row blocks handed out so that an XCD works on CONTIGUOUS packed rows (agg.hip edge_grad_body)
};
constexpr int EDGE_SLAB = 264;
// The edge-gradient workgroups add their bond-type histograms (a dozen non-zero bins each) to one of EDGE_COPIES fp64 accumulator
// slabs instead of writing a slab of their own: the reduction that follows reads 8 slabs, not one per workgroup (12.7 MB at
// batch 1024).  The accumulators live right behind the GEMM hand-off workspace in every layer scratch carving -- same place for
// every layer and direction, never used for anything else --, are cleared together with the hand-off flags once per API call
// and zeroed again by the reduction that drains them.
constexpr int EDGE_COPIES = 8;
inline size_t edge_acc_bytes() { return align256((size_t)EDGE_COPIES * EAGCN_MAX_VIEWS * EDGE_SLAB * sizeof(double)); }
int edge_grid_x(const eagcn_batch* b);
int launch_agg_edge(AggArgs a, const EdgeArgs& e, hipStream_t s);   // transposed aggregation + edge gradients, one grid

enum { BN_SC = 0, BN_SH, BN_MU, BN_INV };     // rows of a layer's [4][Fp] BatchNorm coefficient table

struct ColMapD {                 // exact <-> packed column map of a layout
    int nseg;
    int w[EAGCN_MAX_SEGS], p[EAGCN_MAX_SEGS];
};
inline ColMapD make_colmap(const eagcn_layout* l) {
    ColMapD m;
    m.nseg = l->nseg;
    for (int i = 0; i < EAGCN_MAX_SEGS; ++i) {
        m.w[i] = i < l->nseg ? l->width[i] : 0;
        m.p[i] = i < l->nseg ? l->pad[i] : 0;
    }
    return m;
}

// Upstream gradient of the LAST layer given per molecule instead of per row: the read-out backward
// (dx[r] = dg[mol(r)] / size, reference models.py:108-111) evaluated inside the layer's first backward
// kernel, so the [T][ldo] broadcast is never written or read.
struct ReadoutGrad {
    const float* dg; int F;      // [B][F] gradient of the molecule fingerprints
    const int64_t* size; int mode;
    ColMapD map;                 // layout of the layer output (packed column -> exact column)
};
int launch_readout_bwd_rows(const eagcn_batch* b, const ReadoutGrad& rg, int ld, float* dx, hipStream_t s);   // readout.hip
// ---- wave-autonomous balanced GEMM (gemm3.hip): NT (ta=0,tb=1) and TN (ta=1,tb=0) forms --------------------------------
struct G2Prob {                  // one product C[M,N] = op(A).op(B) in one of the three operand forms of a layer
    const float* A; const float* B; float* C;
    int lda, ldb, ldc;
    int M, N, K;                 // static extents (capacities where a device-side count exists)
    const int* M_dev;            // actual M (rows of A and C), read on the device
    const int* K_dev;            // actual K
};
struct DwScatter {               // epilogue of a layer's dW product: packed (input column, output column) -> blockK.graph_conv.weight.grad
    float* dW[EAGCN_MAX_VIEWS];
    ViewCols vc;
    ColMapD in;
    int in_identity;             // the input layout has no padded columns: packed row == exact row (set by the launchers)
};
// ---- XCD-local schedule of a paired launch (dX = dP.W^T with dW = X^T.dP) -------------------------------------------------
// The linear iteration space of the pair is laid out as eight SEGMENTS, one per XCD (dispatch slot b runs on XCD b % 8 and
// the kernel hands every XCD a contiguous run of wave ranges): segment x = the dX tiles of the row blocks [a_x, a_x+1) followed
// by, for EVERY dW tile, the k-steps [c_x, c_x+1) -- i.e. the long reduction of dW (K = packed rows) is split ACROSS the XCDs
// and each XCD only ever touches the rows [~x T/8, ~(x+1) T/8) of dP and X (both products!): they cross the fabric once
// and stay in that XCD's 4 MB L2, instead of every XCD streaming full-K column strips for "its" dW tiles.  The price is one
// partial dW slab per XCD (plain tile stores), summed by the gradient-unpacking launch that follows anyway.  The boundaries
// are a pure function of the device-side extents, shared by the kernel and that reduction.
constexpr int G3_XSEG = 8;
struct G3Plan {
    int a[G3_XSEG + 1];          // dX row-block boundaries
    int c[G3_XSEG + 1];          // dW k-step boundaries
};
__host__ __device__ inline void g3_plan(int RB, int CT0, int ipt0, int T1, int ipt1, int G, G3Plan& pl) {
    const long total = (long)RB * CT0 * ipt0 + (long)T1 * ipt1;
    const int R = 4 * G;
    const long per = total / R, rem = total - per * R;
    const int qn = G >> 3, rn = G & 7;
    pl.a[0] = 0;
    pl.c[0] = 0;
    for (int x = 1; x < G3_XSEG; ++x) {
        const long L = 4L * (x * qn + (x < rn ? x : rn));            // first wave range of XCD x
        const long tgt = L * per + (L < rem ? L : rem);              // iteration where that range starts
        int a = (int)(((long)RB * L + R / 2) / R);                   // row blocks in proportion to the waves in front
        a = a < pl.a[x - 1] ? pl.a[x - 1] : (a > RB ? RB : a);
        long cc = T1 > 0 ? (tgt - (long)a * CT0 * ipt0 + T1 / 2) / T1 : 0;
        if (tgt - (long)a * CT0 * ipt0 < 0) cc = 0;
        int c = (int)(cc > ipt1 ? ipt1 : cc);
        c = c < pl.c[x - 1] ? pl.c[x - 1] : c;
        pl.a[x] = a;
        pl.c[x] = c;
    }
    pl.a[G3_XSEG] = RB;
    pl.c[G3_XSEG] = ipt1;
}
size_t gemm3_workspace_bytes();
bool gemm3_xk_enabled();          // the schedule above is used for the paired backward products (EAGCN_GEMM3_XK=0 turns it off)
int gemm3_grid();
// the hand-off flags must be zero when a launch starts; every launch leaves them zero again, so ONE clear at the start of
// an API call (a tiny kernel, also under capture) covers all its launches on the same workspace
// (`zero`: optionally `nzero` doubles cleared by the same launch -- the head's BatchNorm sums)
int gemm3_clear_flags(void* workspace, size_t bytes, hipStream_t s, double* zero = nullptr, int nzero = 0);
int gemm3_failed();              // sticky, host-visible: a hand-off of some earlier launch timed out (its tile is NaN)
#define EAGCN_CHECK_GEMM3(who)                                                                                         \
    do {                                                                                                               \
        if (::eagcn::gemm3_failed()) {                                                                                 \
            ::eagcn::set_error("%s: a stream-K hand-off of an earlier GEMM launch timed out (a contributor wave was not " \
                               "co-resident with its owner): that launch's results are NaN-poisoned; call "           \
                               "eagcn_gemm_sk_reset_failed() after fixing the cause (EAGCN_GEMM3_WGS, concurrent work)", who); \
            return EAGCN_ERR_HIP;                                                                                      \
        }                                                                                                              \
    } while (0)
// words another kernel clears on the way (instead of a launch of its own): the hand-off flags of gemm3.hip and fp64 sums
int gemm_mode();             // 0 fp32 MFMA | 1 exact bf16 x 6, split by the consumer | 2 plain bf16 operands (gemm.hip)
                             // 3 exact bf16 x 3 PLANES written by the producers | 4 ONE bf16 plane (gemm_bx3.hip)
inline int gemm_planes() { const int m = gemm_mode(); return m == 3 ? 3 : m == 4 ? 1 : 0; }
struct ZeroJob { unsigned* u; int nu; double* d; int nd; };
// stream hand-offs that ride in a step's first launch (eagcn_model.start_signal / wait_flag): +1 on `start`, then a poll of `flag`
// until it is non-zero (cleared afterwards); after `budget` ticks of the 100 MHz clock the poll gives up and raises *err
struct HandOff { uint32_t* start; uint32_t* flag; int* err; unsigned long long budget; };
__device__ __forceinline__ void handoff_body(const HandOff& h) {
    if (h.start) __hip_atomic_fetch_add(h.start, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    if (h.flag) {
        const unsigned long long t0 = wall_clock64();
        while (__hip_atomic_load(h.flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
            __builtin_amdgcn_s_sleep(8);
            if (wall_clock64() - t0 > h.budget) {
                if (h.err) __hip_atomic_store(h.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            }
        }
        __hip_atomic_store(h.flag, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
int gemm3_zero_job(void* workspace, size_t bytes, double* zero, int nzero, ZeroJob* out);
// zero-fill by a kernel (memset NODES of a captured graph are not ordered with their neighbours on replay, ROCm 7.x): for every
// clear that can sit inside a captured sequence
int zero_fill(void* p, size_t bytes, hipStream_t s);
bool gemm3_ok(const GemmDesc& g);
int launch_gemm3(const GemmDesc& g, const DwScatter* sc, void* workspace, size_t bytes, hipStream_t s);
// xk_slab > 0: XCD-local schedule, dW leaves as G3_XSEG partial slabs dw.C + x * xk_slab (sc must be null)
int launch_gemm3_pair(const GemmDesc& dx, const GemmDesc& dw, const DwScatter* sc, void* workspace, size_t bytes, hipStream_t s,
                      size_t xk_slab = 0);

// ---- model head (head2.hip) -----------------------------------------------------------------------------------------------
constexpr int HEAD_COPIES = 8;  // replicas of the head's forward BatchNorm sums (one with sync-BatchNorm: the hook reduces ONE block)
using HeadDrop = DropArgs;
struct HeadFwd {                 // y = act(bn(x)) . W  (+ column sums of y)
    int B, K, N;
    const float* x; const double* st_in; const float *gamma, *beta; float *run_mean, *run_var; float* bn;
    const float* W; float* y; float* y2; double* st_out;
    int training, relu; float eps, momentum; HeadDrop drop;
    const double* cnt_in = nullptr;      // sync-BatchNorm: rows of the BatchNorm over ALL ranks (st_in holds their summed sums)
    // the sums live in st_copies replicas, st_stride doubles apart: a producer workgroup adds to replica (row tile % copies),
    // the consumer adds the replicas up (fp64 atomics on one 128-byte line are served one after the other, ~11 ns each: 1024
    // arrivals per line at B = 1024 kept den1 / den2 waiting 11 us each)
    int st_copies = 1, st_stride = 0;
    // optional job on the way: count the entries of lab[0 .. nlab) that are 0 or 1 (the batch's labelled entries of the BCE loss)
    // into *lab_cnt (zero on entry), every workgroup its share
    const float* lab = nullptr; int nlab = 0; unsigned* lab_cnt = nullptr;
    int nw = 0;                          // waves per workgroup that split the reduction: 4 / 8, 0 = by the launch's tile count
    uint32_t* signal = nullptr;          // optional: a device word bumped by the launch's first workgroup (eagcn_model.fwd_signal: "the forward
                                         // has passed its read-out" -- a launch of its own cost the step 4.6 us on the main stream)
};
struct HeadBwd {                 // backward of  y = act(bn_p(x)) . W : d(bn_p output) with its sums, and dW
    int B, K, N;
    const float* x; const float* bnp; int relu_p; HeadDrop drop; const float* W;
    const float* dy; const float* y; const float* bny; const double* sb_y; const float* extra;
    float *dgamma_y, *dbeta_y; float* dyp; double* sb_p; float* dW; int training;
    const double* cnt_y = nullptr;       // sync-BatchNorm: global row count of the BatchNorm behind y (sb_y: sums of all ranks)
    float gscale = 1.0f;                 // ... and 1 / world: d gamma / d beta = this rank's share of the summed sums
    // ks > 1: the weight gradient's reduction over the B batch rows is cut into ks row chunks, one workgroup per (tile, chunk);
    // chunk c's partial goes to dW_part + c * K * N and head_gbn_bwd adds the partials up in chunk order (a tile's whole
    // reduction in one workgroup is a chain of B / 128 dependent load batches: 8 at B = 1024, the longest pole of the launch)
    int ks = 1; float* dW_part = nullptr;
    int nw = 0;                          // (as HeadFwd.nw)
};
inline int head_dw_chunks(int B) { return B > 256 ? (B + 255) / 256 < 16 ? (B + 255) / 256 : 16 : 1; }
struct HeadDwSum { float* dst; const float* part; int n, ks; };     // dst[i] = sum_c part[c * n + i]
// the column sums of the top layer's BatchNorm backward, taken where dg is formed (layer.hip BN2_STAGED_FROM_READOUT):
//   slab[s][cp][0..1] = sum over the molecules b = s, s + nslab, ... of dg_eff[b][c] * (A1, A2)[b][c]   (fp64; cp = packed column of c,
//   zero at the padded columns), dg_eff = dg / size in 'ave' mode (ReadoutGrad).  A1 == null: no such job
//   dge (optional): [B][F] dg_eff itself, for the kernels that gather it per row (lagg_top.hip)
struct HeadTopSums { const float *A1, *A2; double* slab; int nslab, fp; ColMapD map; const int64_t* size; int mode; float* dge; };
struct HeadGbn { int B, F; const float *dgn, *g, *bn; const double* sb; float *dg, *dgamma, *dbeta; int training;
                 const double* cnt = nullptr; float gscale = 1.0f;
                 HeadDwSum sum[3] = {}; int nsum = 0;               // partial weight gradients of the dense layers (HeadBwd.ks)
                 HeadTopSums top = {}; };
// slabs of those sums: a small fixed count (the finalize adds up to 64 with sixteen lanes per column), each a chain of B / count molecules
inline int top_bn_slabs(int B) { return B > 256 ? 64 : 16; }
// the middle of a TRAINING step's head in one launch: last forward stage, loss, dense 3's d(input) (head2.hip head_mid_kernel)
struct HeadLoss { int kind;                 // 0: weighted BCE with logits over the labelled entries (train.py:326-331), 1: MSE (train.py:321-325)
                  const float* labels; const float* weight; float* loss; const float* scale; float* dout; };
struct HeadMid { HeadFwd f3; HeadBwd b3; HeadLoss L;
                 double* ws; };            // HEAD_WS doubles, zero on entry: {unused, labelled entries} as two 32-bit words, loss sum
constexpr int HEAD_WS = 4;
struct HeadLossFin { float* loss; const double* ws; const float* scale; int kind, n; };   // loss value = ws[1] / count (* scale); loss == null: no job
bool head_mid_ok(int n_den2, int nclass);
int head_mid(const HeadMid& a, hipStream_t s);
int head_bwd_pair(const HeadBwd& a, const HeadBwd& e, const HeadLossFin& lf, hipStream_t s);
// cnt (optional): three slots that receive B as a double (row counts of the head's BatchNorms, summed with the statistics)
int head_colstats(const float* g, int B, int F, double* st, hipStream_t s, double* cnt0 = nullptr, double* cnt1 = nullptr,
                  double* cnt2 = nullptr);
int head_fwd(const HeadFwd& a, hipStream_t s);
int head_bwd(const HeadBwd& a, hipStream_t s);
int head_gbn_bwd(const HeadGbn& a, hipStream_t s);

// The final reduction of a layer's edge gradients (8 shared accumulator slabs -> d att.weight, d self_r) handed to the NEXT
// layer's first backward kernel instead of a launch of its own (unpack_grads has nothing else to do for a layer on the balanced
// GEMM): eacc == nullptr means nothing is pending.
struct EdgeDrain {
    double* eacc; int K;
    float* datt_w[EAGCN_MAX_VIEWS]; float* dself_r[EAGCN_MAX_VIEWS]; int channels[EAGCN_MAX_VIEWS];
    const float* rsig;           // [K] sigmoid(self_r) of the layer the gradients belong to
};
// the optional arguments of a layer's backward
struct LayerBwdOpts {
    const ReadoutGrad* rg = nullptr;         // the upstream gradient per molecule (dxout is null then)
    bool dpad_views = false;                 // dpad_row holds one gradient row per VIEW ([K][ld_out]: sampled dropout of the non-stored rows)
    const ZeroJob* zero_after = nullptr;
    const EdgeDrain* drain_in = nullptr;     // pending edge reduction of the layer above
    EdgeDrain* drain_out = nullptr;          // receives this layer's, if nothing else is left for its gradient unpacking
    bool input_only = false;                 // (below)
    // model engine, Concate top layer behind the fused read-out: sum dH and sum dH xhat per packed column arrive as top_nslab fp64
    // slabs [slab][fp][2] (HeadTopSums) -- the reduction pass over the rows is skipped and no dH is stored
    const double* top_sums = nullptr; int top_nslab = 0;
    const float* top_dge = nullptr;          // ... and dg / size per molecule [B][rg.F] (HeadTopSums.dge), or null: rows of rg are written
    // model engine, a plane-pair layer above a Concate layer whose route carries the tail pass (LayerRoute.carries_below): the dX
    // product's launch forms the layer BELOW's dH and its column sums (bx3.h BxBnEpi, complete but for C) ...
    const BxBnEpi* below = nullptr;
    // ... and that layer's call: dxout already holds dH, sum dH and sum dH xhat arrive as one fp64 slab [fp][2] per BX_EPI_ROWS packed
    // rows (dh_nslab: the slab CAPACITY; the finalize counts the written ones from the device-side row count) -- no reduction pass
    const double* dh_sums = nullptr; int dh_nslab = 0;
};
inline int hidden_bn_slabs(int T) { return (T > 0 ? T + BX_EPI_ROWS - 1 : BX_EPI_ROWS) / BX_EPI_ROWS; }      // slab capacity for T packed rows
bool top_bn_sums_enabled();                  // eagcn_set_top_bn_sums != 0
bool top_bn_gather_enabled();                // ... == 1: the staging gathers dg per molecule (2: rows of the read-out gradient are written)
bool planes_only_enabled();                  // EAGCN_PLANES_ONLY: a hidden layer whose reader takes plane images alone leaves no fp32 output
// a top layer's staging can gather the read-out gradient dge [B][F] per molecule: four adjacent exact columns with one 16-byte load
bool top_gather_ok(const eagcn_layer_params* p, const float* dge, int F);

// ---- the route of a layer call: which kernels it runs, decided ONCE by plan_layer (layer.hip) -- a pure host function of the batch
// description, the layer, the buffers' addresses (alignment only), the ask and the switches.  The public entry points plan for
// themselves, the model engine plans all layers of a call at once (head.hip plan_model); layer_forward_impl / layer_backward_impl carry
// the route out, eagcn_layer_route / eagcn_model_route show it to the tests (the values are part of the C ABI: include/eagcn_hip.h)
// REFUSED: x exists as plane images only and the plane products do not apply -- the call fails
enum FwdProd { FWD_NONE = 0, FWD_PLANES, FWD_BALANCED, FWD_TILED, FWD_REFUSED };        // gemm_bx3.hip | gemm3.hip | gemm.hip
enum AggPath { AGG_DENSE = 0, AGG_LAGG };                                 // matrix-core kernels of agg.hip | LDS-staged bond lists (lagg.hip)
// where the BatchNorm backward's second pass dY' = sc (dH - c1 - xhat c2) happens
enum Bn2 {
    BN2_NONE = 0,
    BN2_ELEMENTWISE,             // bn_bwd_apply_kernel on the dH the first pass stored (Concate: the upstream gradient is as wide as dH)
    BN2_REDUCE_APPLY,            // bn_bwd_reduce_kernel again, dH re-formed (Weighted_sum: the upstream gradient is K times narrower:
                                 // no write and read of T x Fp floats, HIV 9.74 -> 9.53 ms per step)
    BN2_STAGED_FROM_DH,          // lagg.hip, while it stages the rows of the stored dH (it is the only consumer of dY')
    BN2_STAGED_FROM_UPSTREAM,    // lagg.hip re-forms dH AND dY' from the layer's upstream gradient: neither exists in memory
    BN2_STAGED_ROWMASK,          // ... of a Concate layer in eval mode (input-only form: dH = upstream x row mask x relu')
    BN2_STAGED_FROM_READOUT      // ... of a Concate top layer in training mode whose column sums came from the read-out (LayerBwdOpts.top_sums):
                                 // no reduction pass, no stored dH; lagg_top.hip re-forms dH from the read-out gradient, gathered per
                                 // molecule (LayerBwdOpts.top_dge) or written out as rows first (rows_late)
};
enum EdgePath { EDGE_NONE = 0, EDGE_WITH_LAGG, EDGE_COLAUNCH };   // lagg.hip's gathers | one grid with agg.hip (3, an own launch: retired)
enum BwdProd {
    BWD_NONE = 0, BWD_PLANES_PAIR, BWD_PLANES_DW, BWD_PLANES_DX,      // gemm_bx3.hip: dX with dW | dW alone | dX alone (input-only)
    BWD_G3_XK, BWD_G3_SCATTER,   // gemm3.hip pair: dW as one partial slab per XCD | written straight into the per-view gradients
    BWD_TILED_PAIR, BWD_TILED_SEPARATE, BWD_TILED_DX,                 // gemm.hip: one grid | dW alone (no dX asked) | dX alone
    BWD_REFUSED
};
struct PlanAsk {                 // (all false: a forward call)
    bool has_dx = false;         // d(layer input) is asked for
    bool mol_grad = false;       // the upstream gradient comes per molecule (ReadoutGrad)
    bool input_only = false;
    bool has_drain_out = false;  // a layer below could take this layer's edge-gradient reduction
    bool top_sums = false;       // the BatchNorm backward's column sums are given (LayerBwdOpts.top_sums; the model engine alone asks)
    bool top_gather = false;     // ... and the read-out gradient per molecule in a form the staging can gather (LayerBwdOpts.top_dge)
    bool dh_given = false;       // the upstream buffer holds dH already and its column sums are given (LayerBwdOpts.dh_sums)
    bool below = false;          // the layer below would take its dH and sums from this call's dX product (LayerBwdOpts.below)
};
struct LayerRoute {
    FwdProd fwd_prod = FWD_NONE; bool fwd_split_x = false;      // split: the planes of x are produced here (launch_bx3_split)
    AggPath fwd_agg = AGG_DENSE, bwd_agg = AGG_DENSE;
    Bn2 bn2 = BN2_NONE;
    bool rows_first = false, rows_late = false;                  // launch_readout_bwd_rows before the reduction | before the aggregation
    bool store_dh = false;                                       // the first pass of the BatchNorm backward stores dH
    EdgePath edge = EDGE_NONE; bool edge_atomic = false;         // atomic: the partials leave through the shared accumulators
    BwdProd bwd_prod = BWD_NONE; bool bwd_split_x = false;
    bool bx_wide = false;                                        // PLANES_PAIR / PLANES_DW: the launch runs on the 256 x 128 kernel (bx3_pick_wide)
    // PlanAsk.below on PLANES_PAIR, 128 x 128 kernel: dX carries the tail pass that forms the layer below's dH and column sums (the 256 x
    // 128 kernel does not: with it every launch of that kernel ran slower, DESIGN.md section 1 -- the layer below keeps its pass)
    bool carries_below = false;
    bool defer_drain = false;                                    // the edge reduction is left to the next layer's first kernel
    bool dh_given = false;                                       // no reduction pass: dH and its sums came from the layer above's dX product
    // a refinement below BWD_TILED_SEPARATE (first layer, no dX asked): dWcat leaves the transposed aggregation's epilogue as dw_ny
    // slabs (lagg_dw.hip) -- no dP, no product launch; the slabs live in the dWcat area, or in the dP area this route leaves free
    bool dw_fused = false; int dw_ny = 0; bool dw_in_dp = false;
    bool bn2_staged() const { return bn2 >= BN2_STAGED_FROM_DH; }
    bool bwd_planes() const { return bwd_prod >= BWD_PLANES_PAIR && bwd_prod <= BWD_PLANES_DX; }
};
LayerRoute plan_layer(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w, const PlanAsk& ask);
int layer_backward_impl(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w, const float* dxout,
                        const float* dpad_row, float* dx, const eagcn_layer_grads* g, void* stream, const LayerRoute& r,
                        const LayerBwdOpts& o = LayerBwdOpts{});
// model engine (head.hip): the backward of eagcn_model_backward_input with layer 0's d(input) left PACKED ([T][ld_in] inside the scratch
// block, *dx0), and where the packed input lives inside `saved` (attr.hip)
int model_backward_input_packed(const eagcn_batch* b, const eagcn_model* m, const int64_t* size, void* saved, size_t saved_bytes,
                                void* scratch, size_t scratch_bytes, const float* dout, const float* dgraph_rep,
                                const eagcn_layer_grads* lg, const eagcn_head_grads* hg, float** dx0, void* stream, const char* who);
// attr.hip: dense [B][N][F] from packed rows acc [T][ld] of layout `in`, times (x - base) when x != null; score[b][i] = row sums or null
int launch_attr_dense(const eagcn_batch* b, const eagcn_layout* in, const float* acc, const float* x, const float* base, float* attr,
                      float* score, hipStream_t s);
int model_input_slot(const eagcn_batch* b, const eagcn_model* m, void* saved, size_t saved_bytes, float** x0, const char* who);
// input_only: d(layer input) alone -- g may be null, no parameter gradient is formed (no dW product, no edge gradients, no gradient
// unpacking; in eval mode no BatchNorm reduction either: dY' = sc dH is formed where the transposed aggregation stages its rows)
// skip_apply: stop after the BatchNorm table (the caller applies it while it consumes Y: fused read-out of the top layer)
// planes_only: the output leaves as the operand planes of the next layer's products ONLY (w->xout_planes; the fp32 matrix w->xout
// is not written): the model engine asks for it when the layer above, planned without an fp32 input, runs both directions from the
// planes (head.hip plan_model); a layer that is handed w->x == nullptr fails loudly if it reaches a fallback
int layer_forward_impl(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w, void* stream, const LayerRoute& r,
                       bool prepacked, bool skip_apply = false, bool planes_only = false);
// eagcn_layer_bufs.aux_stream / eagcn_model.aux_stream are reserved (the backward runs on the call's one stream): a value is refused
inline int check_reserved_null(const void* value, const char* who, const char* field) {
    EAGCN_CHECK_ARG(!value, "%s: %s is reserved and must be null", who, field);
    return EAGCN_OK;
}
// relu / dropout / mask / view merge of a layer from its saved Y and BatchNorm table (what layer_forward_impl ends with)
int layer_apply_impl(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w, void* stream);
int pack_params_all(const eagcn_batch* b, const eagcn_layer_params* const* ps, void* const* packed,
                    const size_t* packed_bytes, int n, void* stream, const ZeroJob* zj = nullptr, const HandOff* ho = nullptr);
struct ReadoutBn {
    const float* Y; int ldy;                 // [T][Fp] pre-BatchNorm (bias-free) aggregation output
    const float* bn; int fp;                 // [4][Fp] scale / shift / ...
    int do_drop; uint32_t thr; float inv_keep; uint64_t seed; const uint64_t* seed_dev;
    const int64_t* size; int mode;
    float* g; int F;                         // [B][F]
    double* st;                              // [2 F] sum g, sum g^2 (fp64 atomics; zero on entry)
    int st_copies = 1, st_stride = 0;        // replicas of st (HeadFwd): workgroup x adds to replica x % st_copies
    bool pair = false;                       // set by the launcher: a lane quad shares a dropout draw
    double *cnt0, *cnt1, *cnt2;              // optional row-count slots of the head's BatchNorms (sync-BatchNorm)
    // optional: [B][F] per-molecule sums of q and q * xhat, q = d x[r][c] / d(relu argument) = m_r * dropout scale * [sc Y' + sh > 0],
    // xhat = (Y' - mu) inv -- what the BatchNorm backward's column sums need of the rows (HeadTopSums); null: not formed
    float* A1 = nullptr; float* A2 = nullptr;
};
int readout_bn_forward(const eagcn_batch* b, const eagcn_layout* lay, const ReadoutBn& a, void* stream);
int readout_forward_sampled(const eagcn_batch* b, const float* x, const eagcn_layout* lay, const eagcn_layer_params* p,
                            const float* bn_sh, const int64_t* size, int mode, float* g, int F, uint16_t* cnt, float* padc,
                            uint32_t* tab, void* stream);   // tab: (N + 1)^2 words of scratch
int readout_backward_pad_views(const eagcn_batch* b, const float* dg, const eagcn_layout* lay, const int64_t* size, int mode,
                               int F, int K, const uint16_t* cnt, float dropout, float* dpad, void* stream);
int readout_backward_pad(const eagcn_batch* b, const float* dg, const eagcn_layout* lay, const int64_t* size,
                         int mode, int F, float* dpad_row, void* stream);
// agree.hip: the two launches of eagcn_eval_reg_agreement (agree_pair_kernel, agree_reg_finalize_kernel) and of
// eagcn_eval_class_threshold (agree_class_kernel, agree_class_finalize_kernel) on checked arguments (api.cpp checks them), the
// workspace either takes, how many workgroups share a tile's rows in the pair kernel, and the tiles of AGR_R entries of a task
size_t agree_workspace_bytes(int64_t rows, int T);
int agree_splits(int64_t rows, int T);
int64_t agree_tiles(int64_t rows);
int launch_agree_reg(const float* scores, const float* targets, const uint8_t* valid, int64_t rows, int T, void* workspace, double* out,
                     hipStream_t s);
int launch_agree_class(const float* scores, const float* targets, const uint8_t* valid, int64_t rows, int T, float threshold,
                       void* workspace, double* out, hipStream_t s);

}  // namespace eagcn
