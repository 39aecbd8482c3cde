// Edge-attention aggregation over bond lists with the operand STAGED IN LDS: the operator of agg.hip (reference
// layers.py:82-92 with the masks of layers.py:294-304), per molecule b and view k
//     U[i,j]  = sigmoid(w_k[type(i,j)]) adj[i,j] + sigmoid(self_r) m_i [i == j] + 1e-9 (1 - adj[i,j])
//     A^[i,j] = m_i U[i,j] / sum_j' U[i,j'] ,   Y'[i,:] = sum_j A^[i,j] P_k[j,:]
// evaluated as what it is -- sigma at the two to four bonds of an atom, sigma(self_r) on the diagonal, the constant 1e-9 elsewhere:
//     sum_j U[i,j] P[j,:] = sum_{bonds (i,j)} sigma_ij P[j,:] + r m_i P[i,:] + 1e-9 ( S_b - sum_{bonds (i,j)} P[j,:] ),   S_b = sum_{j < nat} P[j,:]
// a gather of deg + 1 rows plus one rank-one term per molecule (exact, filler included).
//
// Why a third form.  The matrix-core kernels (agg.hip) multiply the full nat x nat block: at 256 atoms
// 99 % of their MFMAs multiply by 1e-9, and over small molecules with wide layers (HIV: 1250 columns per view) they re-read every
// operand row once per 16-row tile and stream at 1-1.7 TB/s.  The bond-list kernel of round 4 (sagg.hip, removed in round 6) did 64x fewer multiply-adds
// and lost anyway: a wavefront owned a molecule and gathered its neighbour rows from L2, every batch of rows one memory round trip
// behind the previous one.  Here the round trips are taken ONCE per workgroup, for everything, and the gathers are LDS reads:
//   * a workgroup owns a ROW BLOCK -- whole molecules, greedily packed to <= 256 packed rows / 16 molecules (eagcn_batch.blk, built
//     with the batch index) -- and a 32-column chunk of one view;
//   * it loads the block's rows of the operand (one 16-byte load per lane and row: 128 contiguous bytes per row), the rows' list
//     headers and the block's list entries (contiguous: the entries of molecule b live in [edge0[b], edge0[b+1])) in ONE batch of
//     independent loads, and puts them into LDS (32 KB of operand; list entries as {atom, sigma});
//   * one thread per row turns the row's list into a RECORD -- four bond weights with the row scale and the filler folded in, the
//     source rows, the self / rank-one weights (struct comment below) -- so that the row loop has no list walk and no branch;
//   * S_b: 32 groups of 8 lanes sum contiguous row ranges (one batch of LDS reads) and add them to the molecule's LDS slot;
//   * then 8 lanes own a row: 2-3 record reads, five `ds_read_b128` gathers, 24 FMAs, one 16-byte store.  BatchNorm partial sums
//     (fp64) are carried per lane and leave as one slab per row block (layer.hip bn_finalize counts the live blocks from meta[NBLK]).
// Every operand element is read from memory once and every result written once; the matrix cores are not involved (there is no
// dense block to multiply).
// Backward (one kernel): the transposed aggregation dP[j,:] = sum_{bonds (i,j)} s_i sigma_ij dY'[i,:] + s_j r dY'[j,:] + 1e-9 (G_b -
// sum_{bonds} s_i dY'[i,:]), G_b = sum_i s_i dY'[i,:], s_i = m_i / rowsum_i -- and, from the SAME gathers, the edge gradients of
// agg.hip's edge_grad_body: with dY' of the block in LDS, row j's own P and Y' rows in registers,
//     dA^[i,j] = <dY'[i,:], P[j,:]> ,  rowdot_i = <dY'[i,:], Y'[i,:]> ,  dU[i,j] = s_i (dA^[i,j] - rowdot_i)
// are partial sums over the workgroup's 32 columns (everything is linear in them): d w_k[c] += dU s (1 - s) by bond type through an
// LDS histogram, d self_r from the diagonal, flushed with fp64 atomics into the shared accumulator slabs (kernels.h EDGE_COPIES).
// The BatchNorm backward's second pass (layer.hip bn_bwd_apply_kernel: dY' from dH, Y' and five per-column constants) is applied to the
// rows while they are staged (AggArgs.bn_tab; Concate layers): that launch, and a write and a read of T x Fp floats, are gone -- which
// is what makes this kernel the faster BACKWARD for every Concate configuration, small molecules included (policy: lagg_use below).
// Accuracy: the filler enters as one exact rank-one term per molecule instead of nat - deg products of 1e-9 summed one by one on the
// fp32 matrix core: against float64 d att.weight is off by 1e-6 of its scale at 256-atom molecules where agg.hip is off by up to 6e-4.
#include <stdlib.h>

#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "lagg_kernel.h"

namespace eagcn {

// (the kernel template: lagg_kernel.h)

// ---- policy ------------------------------------------------------------------------------------------------------------------------------
// EAGCN_AGG = lds (always, N <= 256) | dense; default: by shape and DIRECTION.  Measured on MI355X, whole step in ms
// with this path forced in the backward only / in both directions against the matrix-core kernels of agg.hip (tools/r5_lagg_parts.sh,
// profiles/r05_lagg_policy.txt; the transposed kernel also absorbs bn_bwd_apply for the Concate layers):
//     K = 8, N = 256, all molecules 256 atoms, B = 1024 (BASELINE configs[4]):          - / 10.6      against 14.6
//     Tox21 (19 atoms on average, N = 132) B = 256, Concate (configs[1]):           0.442 / 0.428    against 0.447
//     Tox21 B = 1024:                                                               0.898 / 0.906    against 0.922
//     Lipo 3-layer Concate B = 512:                                                 1.350 / 1.357    against 1.401
//     HIV Weighted_sum (24 atoms on average, N = 222, 5 x 1250 columns), B = 1024:   7.19 / 7.15     against 6.94
// -> round-5 policy: forward for LARGE molecules (padded size from EAGCN_LAGG_MIN_N = 240 and -- once the rows the batches of the shape
//    really hold are known, eagcn_batch.t_hint -- 96 atoms per molecule on average) or batches of up to 256 molecules; backward: large
//    molecules, or any layer whose BatchNorm backward leaves its second pass to this kernel (Concate); Weighted_sum layers of small
//    molecules on the matrix cores.
// Round 6 (group sums through DPP, edge gradients inside the row loop, several chunks per workgroup, the Weighted_sum staging; same-box
// A/B against the round-5 kernels, tools/r6_ab_lib2.sh): HIV 6.90 -> 6.10 ms with BOTH directions here, Tox21 B = 1024 and Lipo equal
// or faster with the forward here as well -> every layer of every structure takes this path in both directions whenever the
// padded size allows it (N <= 256); agg.hip serves larger molecules, code-book relations and EAGCN_AGG=dense.
static int lagg_cpw(const eagcn_batch& bt, const ViewCols& vc, bool trans);
static int lagg_policy() {
    static const int v = [] {
        const char* e = getenv("EAGCN_AGG");
        if (e && !strcmp(e, "lds")) return 1;
        if (e && !strcmp(e, "dense")) return 0;
        return 2;                                     // by shape
    }();
    return v;
}
static int lagg_min_n() {
    static const int v = env_int("EAGCN_LAGG_MIN_N", 240);
    return v;
}
static int lagg_fwd_maxb() {
    // (round 6: no limit by default.  Up to round 5 batches of more than 256 small molecules took the matrix-core forward of agg.hip;
    //  measured again with this round's kernels the step is equal or faster on this path -- Tox21 B = 1024 0.828 -> 0.822 ms, Lipo
    //  1.254 -> 1.258 -- and the default forward no longer sums the 1e-9 filler products one by one in fp32)
    static const int v = env_int("EAGCN_LAGG_FWD_MAXB", 0x7FFFFFFF);
    return v;
}
bool lagg_wfuse() {
    static const bool on = env_flag("EAGCN_LAGG_WFUSE", true);
    return on;
}
// should the index of batches of this shape carry bond lists and row blocks?  structure: EAGCN_STRUCT_* of the layers, or -1 (not known)
bool lagg_wanted(int B, int N, int structure) {
    const int p = lagg_policy();
    if (p == 0 || N > LAGG_RB) return false;
    if (p == 1) return true;
    return N >= lagg_min_n() || B <= lagg_fwd_maxb() || structure != EAGCN_STRUCT_WEIGHTED || lagg_wfuse();
}
int lagg_parts() {                                    // (debug switch) bit 0: forward, bit 1: backward on this path
    static const int v = env_int("EAGCN_LAGG_PARTS", 3);
    return v;
}
// does this batch take the path?  dir 0: forward, 1: backward; absorbs_bn: the layer's BatchNorm backward would leave its second pass here
bool lagg_use(const eagcn_batch* b, int dir, bool absorbs_bn, const ViewCols* vc) {
    if (!(b->build_lists && b->blk && b->mol_info && b->row_ptr && b->col_ptr && b->nbr && b->tnbr && b->ecode && b->tcode && b->row_info))
        return false;
    const int p = lagg_policy();
    if (p == 0 || b->N > LAGG_RB || !(lagg_parts() & (dir ? 2 : 1))) return false;
    if (p == 1) return true;
    const bool large = b->N >= lagg_min_n() && !(b->t_hint > 0 && (long)b->t_hint < 96L * b->B);
    if (large) return true;
    // forward of small molecules: batches of up to 256 molecules, or (round 6) launches of so many workgroups that each takes several
    // chunks of a block and builds its records once (HIV widths: agg_wave 0.79 -> 0.70 ms)
    return dir ? absorbs_bn : (b->B <= lagg_fwd_maxb() || (vc && lagg_cpw(*b, *vc, false) > 1));
}
// Rows per block: always LAGG_RB.  Measured (EAGCN_LAGG_RB = 256 / 128 / 64 / 32, whole step in ms): Tox21 B = 256 0.423 / 0.431 / 0.458 /
// 0.541, B = 1024 0.889 / 0.906 / 0.991 / 1.172, Lipo B = 512 1.348 / 1.375 / 1.518 / 1.641 -- more, smaller blocks (more workgroups per CU
// to hide a block's barrier-separated phases) lose: a block's fixed cost (eight clamped row loads per thread whatever the row count, the
// record pass, four barriers) is what a launch pays per block, and the per-molecule column sums stop being shared.
int lagg_block_rows(const eagcn_batch* b) {
    static const int fixed = env_int("EAGCN_LAGG_RB", 0);
    (void)b;
    return fixed > 0 ? std::min(fixed, LAGG_RB) : LAGG_RB;
}
int lagg_slabs(const eagcn_batch* b) { return std::max(1, b->B); }

// chunks of the widest view / an ESTIMATE of the block count from the rows batches of this shape hold (a block closes at LAGG_RB rows or
// LAGG_MAXM molecules: 1.25 x the larger of the two quotients; the kernel loops, so any count is handled, and a tight grid spares the
// launch thousands of workgroups that would only find out that they have no block)
static void lagg_extent(const eagcn_batch& bt, const ViewCols& vc, int* chunks, int* gy) {
    int wmax = 0;
    for (int k = 0; k < vc.K; ++k) wmax = std::max(wmax, vc.off[k + 1] - vc.off[k]);
    *chunks = cdiv(wmax, LG_CW);
    const int rows = bt.t_hint > 0 ? std::min(bt.t_hint, bt.T) : bt.T;
    const int est = 5 * std::max(rows / lagg_block_rows(&bt), bt.B / LAGG_MAXM) / 4 + 2;
    *gy = std::max(1, std::min(std::min(bt.B, est), 65535));
}
// chunks per workgroup: 1 while the launch is a few rounds of the chip's ~768 resident workgroups (the step then wants as many short
// workgroups as it can get: configs[1], B = 1024 and Lipo measured 3-5 % SLOWER with more), several where there are thousands (C5:
// 41 k, HIV widths: 26 k / 10 k): forward up to 8 (C5 forward 681 -> 593 us), transposed up to 4 (C5 -2 %, HIV: no difference between 1, 4, 8)
static int lagg_cpw(const eagcn_batch& bt, const ViewCols& vc, bool trans) {
    static const int cpw_env = env_int("EAGCN_LAGG_CPW", 0);
    static const int cpw_bwd = env_int("EAGCN_LAGG_CPW_BWD", 1);
    int chunks, gy;
    lagg_extent(bt, vc, &chunks, &gy);
    const long wgs = (long)vc.K * chunks * gy;
    int per = (trans && !cpw_bwd) ? 1 : cpw_env > 0 ? cpw_env : (int)std::min<long>(trans ? 4 : 8, std::max<long>(1, wgs / 3072));
    return std::max(1, std::min(per, chunks));
}
static int lagg_grid(const AggArgs& a, dim3* grid, int* nchunk, int* cpw, bool trans) {
    int chunks, gy;
    lagg_extent(a.bt, a.vc, &chunks, &gy);
    *cpw = lagg_cpw(a.bt, a.vc, trans);
    *nchunk = cdiv(chunks, *cpw);
    *grid = dim3((unsigned)(a.vc.K * *nchunk), (unsigned)gy);
    return EAGCN_OK;
}

int lagg_bwd_grid_y(const eagcn_batch* b, const ViewCols& vc) {
    int chunks, gy;
    lagg_extent(*b, vc, &chunks, &gy);
    return gy;
}

int launch_lagg_fwd(AggArgs a, hipStream_t s) {
    if (a.bt.B == 0 || a.bt.T == 0) return EAGCN_OK;
    dim3 grid;
    int rc = lagg_grid(a, &grid, &a.nchunk, &a.cpw, false);
    if (rc) return rc;
    ProfScope ps(PROF_AGG, s);
    EdgeArgs e;
    memset(&e, 0, sizeof(e));
    if (a.cpw > 1) lagg_kernel<false, true><<<grid, 256, 0, s>>>(a, e);
    else lagg_kernel<false, false><<<grid, 256, 0, s>>>(a, e);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

int launch_lagg_bwd(AggArgs a, const EdgeArgs& e, hipStream_t s, bool edge) {
    if (a.bt.B == 0 || a.bt.T == 0) return EAGCN_OK;
    EAGCN_CHECK_ARG(!edge || (e.atomic && e.datt), "lagg: the edge gradients leave through the shared accumulator slabs (EdgeArgs.atomic)");
    dim3 grid;
    int rc = lagg_grid(a, &grid, &a.nchunk, &a.cpw, true);
    if (rc) return rc;
    ProfScope ps(PROF_AGG, s);
    EAGCN_CHECK_ARG(!a.w_aw || a.bn_tab, "lagg: the upstream-gradient form needs the BatchNorm tables");
    EAGCN_CHECK_ARG(!a.w_rowm || a.bn_tab, "lagg: the row-mask staging needs the BatchNorm tables");
    if (!edge) {
        rc = launch_lagg_bwd_input(a, e, grid, s);                    // input-only backward (layer.hip): lagg_in.hip
        if (rc) return rc;
    } else if (a.w_rowm) {
        rc = launch_lagg_bwd_top(a, e, grid, s);                      // Concate top layer without a stored dH: lagg_top.hip
        if (rc) return rc;
    } else if (a.dw) {
        grid.y = (unsigned)std::max(1, std::min((int)grid.y, a.dw_ny));       // (never more workgroup rows than slabs: the kernel loops)
        rc = launch_lagg_bwd_dw(a, e, grid, s);                       // weight gradient in the epilogue, no dP: lagg_dw.hip
        if (rc) return rc;
    } else if (a.w_aw) {
        // (one instantiation: with one chunk per workgroup the records of a block are simply built in front of its only chunk; the
        //  single-chunk body with this form's staging needs 177 registers)
        lagg_kernel<true, true, true><<<grid, 256, 0, s>>>(a, e);
    } else {
        if (a.cpw > 1) lagg_kernel<true, true><<<grid, 256, 0, s>>>(a, e);
        else lagg_kernel<true, false><<<grid, 256, 0, s>>>(a, e);
    }
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

}  // namespace eagcn

extern "C" int eagcn_agg_wants_bond_lists(int B, int N) { return eagcn::lagg_wanted(B, N, -1) ? 1 : 0; }
extern "C" int eagcn_agg_wants_bond_lists_for(int B, int N, int structure) { return eagcn::lagg_wanted(B, N, structure) ? 1 : 0; }
