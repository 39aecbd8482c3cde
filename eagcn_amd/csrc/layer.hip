// One multi-view graph-conv layer, forward and backward: parameter packing, the per-view
// BatchNorm over all B*N_pad rows (reference layers.py:408-412) with its grid-wide reduction, the
// relu / dropout / mask / view-merge epilogue (layers.py:93-94, 313-316), and the orchestration of
// the GEMM and aggregation kernels behind the C ABI.
//
// BatchNorm over rows that are not stored: the reference normalises over every row of the padded
// [B,N,F] tensor.  A padded (or bond-less) row has an all-zero attention row, so its pre-BN value
// is exactly the bias.  Working with y' = y - bias (the GEMM output without bias) those rows are
// exactly 0: they add nothing to sum(y') and sum(y'^2) and only enter through the row count
// M = B*N.  The bias cancels inside a training-mode BatchNorm; it re-enters in the running mean
// and in eval mode.
#include <algorithm>

#include <stdlib.h>

#include "common.h"
#include "kernels.h"

namespace eagcn {

struct ParamPtrs {
    const float* att_w[EAGCN_MAX_VIEWS];
    const float* self_r[EAGCN_MAX_VIEWS];
    const float* W[EAGCN_MAX_VIEWS];
    const float* bias[EAGCN_MAX_VIEWS];
    const float* gamma[EAGCN_MAX_VIEWS];
    const float* beta[EAGCN_MAX_VIEWS];
    float* run_mean[EAGCN_MAX_VIEWS];
    float* run_var[EAGCN_MAX_VIEWS];
    const float* ave_w;
    int channels[EAGCN_MAX_VIEWS];          // bond-type codes of view k (1..channels[k])
    const float* rel_vec[EAGCN_MAX_VIEWS];  // general relations: code c+1 -> channel vector rel_vec[k][c][0..rel_c[k]); null: one-hot
    int rel_c[EAGCN_MAX_VIEWS];
};
// attention logit of bond code c (1-based) in view k: w[c-1] for one-hot relation tensors, <w, vec[c-1]> in general (layers.py:82)
__device__ __forceinline__ float att_logit(const ParamPtrs& pp, int k, int c) {
    if (!pp.rel_vec[k]) return pp.att_w[k][c - 1];
    const float* v = pp.rel_vec[k] + (size_t)(c - 1) * pp.rel_c[k];
    float s = 0.0f;
    for (int ch = 0; ch < pp.rel_c[k]; ++ch) s = fmaf(pp.att_w[k][ch], v[ch], s);
    return s;
}
struct GradPtrs {
    float* dW[EAGCN_MAX_VIEWS];
    float* dbias[EAGCN_MAX_VIEWS];
    float* dgamma[EAGCN_MAX_VIEWS];
    float* dbeta[EAGCN_MAX_VIEWS];
    float* datt_w[EAGCN_MAX_VIEWS];
    float* dself_r[EAGCN_MAX_VIEWS];
    float* dave_w;
};

// colp rows
enum { CP_GAMMA = 0, CP_BETA, CP_BIAS, CP_RMEAN, CP_RVAR, CP_AVEW, CP_ROWS = 8 };
// bn rows

__device__ __forceinline__ int col_view(const ViewCols& vc, int cp) {
    int k = 0;
#pragma unroll
    for (int v = 1; v < EAGCN_MAX_VIEWS; ++v) k += (v < vc.K && cp >= vc.off[v]) ? 1 : 0;
    return k;
}
__device__ __forceinline__ int packed_to_exact(const ColMapD& m, int cp) {
    int eo = 0, po = 0;
    for (int s = 0; s < m.nseg; ++s) {
        if (cp < po + m.p[s]) return (cp - po < m.w[s]) ? eo + (cp - po) : -1;
        eo += m.w[s];
        po += m.p[s];
    }
    return -1;
}

// ---- parameter packing -------------------------------------------------------------------------
__device__ __forceinline__ void pack_params_body(const ParamPtrs& pp, const ViewCols& vc, const ColMapD& in, int ld_in,
                                                 int fp, float* __restrict__ Wcat, float* __restrict__ WcatT,
                                                 float* __restrict__ colp, float* __restrict__ sig, float* __restrict__ rsig,
                                                 const BxOut wp = BxOut{nullptr, 0, 0, 0}, const BxOut wtp = BxOut{nullptr, 0, 0, 0}) {
    // 32 x 32 tiles through LDS: Wcat rows AND the rows of its transpose are written as contiguous 128-byte runs (the
    // transpose used to leave as 4-byte stores ld_in floats apart: one cache line per lane)
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;              // 32 columns x 8 rows per pass
    const int ntx = (fp + 31) >> 5, nty = (ld_in + 31) >> 5;
    for (int t = blockIdx.x; t < ntx * nty; t += gridDim.x) {
        const int ip0 = (t / ntx) << 5, cp0 = (t % ntx) << 5;
        {
            const int cp = cp0 + tx;
            const int k = cp < fp ? col_view(vc, cp) : 0;
            const int f = cp - vc.off[k];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ip = ip0 + ty + 8 * j;
                float v = 0.0f;
                if (ip < ld_in && cp < fp) {
                    const int fi = packed_to_exact(in, ip);
                    if (fi >= 0 && f < vc.width[k]) v = pp.W[k][(size_t)fi * vc.width[k] + f];
                    Wcat[(size_t)ip * fp + cp] = v;
                }
                tile[ty + 8 * j][tx] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cp = cp0 + ty + 8 * j, ip = ip0 + tx;
            // [Fp][ld_in]: the K-contiguous B operand of the forward product (NT form)
            if (cp < fp && ip < ld_in) WcatT[(size_t)cp * ld_in + ip] = tile[tx][ty + 8 * j];
        }
        // operand planes of the plane GEMMs (gemm_bx3.hip) of both matrices, four adjacent elements per thread (8-byte stores:
        // scalar 2-byte stores made this launch four times as long); fp and ld_in are multiples of 16 for every layer that has planes
        if (wp.p) {
            const int r = threadIdx.x >> 3, c4 = (threadIdx.x & 7) << 2;
            if (ip0 + r < ld_in && cp0 + c4 < fp)
                bx_store4(wp, ip0 + r, cp0 + c4, make_float4(tile[r][c4], tile[r][c4 + 1], tile[r][c4 + 2], tile[r][c4 + 3]));
            if (cp0 + r < fp && ip0 + c4 < ld_in)
                bx_store4(wtp, cp0 + r, ip0 + c4, make_float4(tile[c4][r], tile[c4 + 1][r], tile[c4 + 2][r], tile[c4 + 3][r]));
        }
        __syncthreads();
    }
    for (int cp = blockIdx.x * blockDim.x + threadIdx.x; cp < fp; cp += gridDim.x * blockDim.x) {
        const int k = col_view(vc, cp), f = cp - vc.off[k];
        const bool ok = f < vc.width[k];
        colp[CP_GAMMA * fp + cp] = ok ? pp.gamma[k][f] : 0.0f;
        colp[CP_BETA * fp + cp] = ok ? pp.beta[k][f] : 0.0f;
        colp[CP_BIAS * fp + cp] = ok ? pp.bias[k][f] : 0.0f;
        colp[CP_RMEAN * fp + cp] = ok ? pp.run_mean[k][f] : 0.0f;
        colp[CP_RVAR * fp + cp] = ok ? pp.run_var[k][f] : 1.0f;
        colp[CP_AVEW * fp + cp] = pp.ave_w ? pp.ave_w[k] : 1.0f;
    }
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < vc.K * 256; e += gridDim.x * blockDim.x) {
        const int k = e >> 8, c = e & 255;
        sig[e] = (c >= 1 && c <= pp.channels[k]) ? sigmoidf_(att_logit(pp, k, c)) : 0.0f;
    }
    if (blockIdx.x == 0 && threadIdx.x < vc.K) rsig[threadIdx.x] = sigmoidf_(pp.self_r[threadIdx.x][0]);
}
__global__ __launch_bounds__(256) void pack_params_kernel(ParamPtrs pp, ViewCols vc, ColMapD in, int ld_in, int fp,
                                                           float* __restrict__ Wcat, float* __restrict__ WcatT,
                                                           float* __restrict__ colp, float* __restrict__ sig,
                                                           float* __restrict__ rsig, BxOut wp, BxOut wtp) {
    pack_params_body(pp, vc, in, ld_in, fp, Wcat, WcatT, colp, sig, rsig, wp, wtp);
}
// every layer of a model in one launch (blockIdx.y = layer): the parameters of all layers are known before the
// first layer runs, and each packing launch is a few microseconds of fixed cost on the critical path
struct PackJob {
    ParamPtrs pp; ViewCols vc; ColMapD in; int ld_in, fp;
    float *Wcat, *WcatT, *colp, *sig, *rsig;
    BxOut wp, wtp;
};
struct PackJobs { PackJob j0, j1, j2, j3; };
__global__ __launch_bounds__(256) void pack_params_multi_kernel(PackJobs jobs, ZeroJob zj, HandOff ho) {
    // the call prologue of the model engine rides along: hand-off flags of gemm3.hip and the head's fp64 BatchNorm sums
    if (blockIdx.y == 0) {
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < max(zj.nu, zj.nd); i += gridDim.x * blockDim.x) {
            if (i < zj.nu) zj.u[i] = 0u;
            if (i < zj.nd) zj.d[i] = 0.0;
        }
    }
    // (an if-chain, not an indexed array: indexing the by-value argument block dynamically would move it to scratch)
    if (blockIdx.y == 0) pack_params_body(jobs.j0.pp, jobs.j0.vc, jobs.j0.in, jobs.j0.ld_in, jobs.j0.fp, jobs.j0.Wcat, jobs.j0.WcatT, jobs.j0.colp, jobs.j0.sig, jobs.j0.rsig, jobs.j0.wp, jobs.j0.wtp);
    else if (blockIdx.y == 1) pack_params_body(jobs.j1.pp, jobs.j1.vc, jobs.j1.in, jobs.j1.ld_in, jobs.j1.fp, jobs.j1.Wcat, jobs.j1.WcatT, jobs.j1.colp, jobs.j1.sig, jobs.j1.rsig, jobs.j1.wp, jobs.j1.wtp);
    else if (blockIdx.y == 2) pack_params_body(jobs.j2.pp, jobs.j2.vc, jobs.j2.in, jobs.j2.ld_in, jobs.j2.fp, jobs.j2.Wcat, jobs.j2.WcatT, jobs.j2.colp, jobs.j2.sig, jobs.j2.rsig, jobs.j2.wp, jobs.j2.wtp);
    else pack_params_body(jobs.j3.pp, jobs.j3.vc, jobs.j3.in, jobs.j3.ld_in, jobs.j3.fp, jobs.j3.Wcat, jobs.j3.WcatT, jobs.j3.colp, jobs.j3.sig, jobs.j3.rsig, jobs.j3.wp, jobs.j3.wtp);
    // ... and the step's stream hand-offs (kernels.h HandOff): this launch reads parameters only, the batch is needed from the next one on
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) handoff_body(ho);
}

// sum of per-workgroup partial pairs slab[s][cp][0..1] over s, L (16 or 64) lanes per column: with hundreds of
// slabs, 64 lanes per column turn five dependent batches of loads per lane into one or two
template <int L>
__device__ __forceinline__ void slab_sum(const double* __restrict__ slab, int nslab, int fp, int cp, int sl,
                                           double& s1, double& s2) {
    s1 = 0.0;
    s2 = 0.0;
    for (int s0 = sl; s0 < nslab; s0 += L * 8) {           // 8 slab pairs in flight per lane
        double2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int s = s0 + L * u;
            v[u] = s < nslab ? *reinterpret_cast<const double2*>(slab + ((size_t)s * fp + cp) * 2) : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) { s1 += v[u].x; s2 += v[u].y; }
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
}

// ---- sync-BatchNorm (SURVEY.md 8e "BN modes (ii)"): this rank's per-channel sums as ONE vector out[2 Fp + 1] = (sum, sum of
//      squares / sum dH, sum dH xhat per column; rows of the BatchNorm) that the caller's hook all-reduces across the ranks; the
//      finalize kernels then read the reduced vector (forward: as a single slab with the global row count; backward: for the
//      means c1, c2 only -- d gamma / d beta stay this rank's sums, the gradient all-reduce averages them like every gradient).
//      mode 1: forward slabs (live count from the tile count), mode 2: backward slabs (from the row count)
constexpr int BWD_ROWS = 7;
template <int L>
__global__ __launch_bounds__(256) void bn_stats_sum_kernel(const double* __restrict__ slab, int nslab, int fp, double M,
                                                            double* __restrict__ out, const int32_t* __restrict__ meta,
                                                            int mode, int tiles_per_wg, int nvirt, int batch_B) {
    if (meta[EAGCN_META_NLOG] > 0) M = (double)batch_B * (double)meta[EAGCN_META_NLOG];
    if (mode == 1 && tiles_per_wg > 0) nslab = min(nslab, (meta[EAGCN_META_NTILES] + tiles_per_wg - 1) / tiles_per_wg);
    if (mode == 1 && tiles_per_wg < 0) nslab = min(nslab, meta[EAGCN_META_NBLK]);      // (lagg.hip: one slab per row block)
    if (mode == 2) nslab = max(1, min(nslab, (meta[EAGCN_META_T] + nvirt + BWD_ROWS - 1) / BWD_ROWS));
    const int cpr = blockIdx.x * (256 / L) + threadIdx.x / L, sl = threadIdx.x % L;
    const int cp = min(cpr, fp - 1);
    double s1, s2;
    slab_sum<L>(slab, nslab, fp, cp, sl, s1, s2);
    if (cpr < fp && sl == 0) { out[2 * cp] = s1; out[2 * cp + 1] = s2; }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[2 * fp] = M;
}

// ---- BatchNorm forward ---------------------------------------------------------------------------
// 256/L columns per workgroup, L lanes per column
template <int L>
__global__ __launch_bounds__(256) void bn_finalize_kernel(const double* __restrict__ slab, int nslab, int fp,
                                                           double M, int training, float eps, float momentum,
                                                           const float* __restrict__ colp, ParamPtrs pp,
                                                           ViewCols vc, float* __restrict__ bn,
                                                           const int32_t* __restrict__ meta, int tiles_per_wg, int batch_B,
                                                           const double* __restrict__ M_dev) {
    // aggregation workgroups beyond the actual tile count exit without writing their slab
    if (meta[EAGCN_META_NLOG] > 0) M = (double)batch_B * (double)meta[EAGCN_META_NLOG];    // (M was computed from the capacity N)
    if (M_dev) M = *M_dev;                             // sync-BatchNorm: rows of ALL ranks (slab = the all-reduced sums)
    if (tiles_per_wg > 0) nslab = min(nslab, (meta[EAGCN_META_NTILES] + tiles_per_wg - 1) / tiles_per_wg);   // (0: every slab is written)
    if (tiles_per_wg < 0) nslab = min(nslab, meta[EAGCN_META_NBLK]);                    // (lagg.hip: one slab per row block)
    const int cpr = blockIdx.x * (256 / L) + threadIdx.x / L, sl = threadIdx.x % L;
    const int cp = min(cpr, fp - 1);
    double s1 = 0.0, s2 = 0.0;
    if (training) slab_sum<L>(slab, nslab, fp, cp, sl, s1, s2);
    if (cpr >= fp || sl != 0) return;
    const int k = col_view(vc, cp), f = cp - vc.off[k];
    const float gamma = colp[CP_GAMMA * fp + cp], beta = colp[CP_BETA * fp + cp];
    const float bias = colp[CP_BIAS * fp + cp];
    float mu, inv;
    if (training) {
        const double mean = s1 / M;
        double var = s2 / M - mean * mean;
        var = var > 0.0 ? var : 0.0;
        mu = (float)mean;
        inv = (float)(1.0 / sqrt(var + (double)eps));
        if (f < vc.width[k]) {
            const double unbiased = var * (M / (M - 1.0));
            pp.run_mean[k][f] = (float)((1.0 - momentum) * (double)colp[CP_RMEAN * fp + cp] + momentum * (mean + (double)bias));
            pp.run_var[k][f] = (float)((1.0 - momentum) * (double)colp[CP_RVAR * fp + cp] + momentum * unbiased);
        }
    } else {
        mu = colp[CP_RMEAN * fp + cp] - bias;
        inv = 1.0f / sqrtf(colp[CP_RVAR * fp + cp] + eps);
    }
    const float sc = gamma * inv;
    bn[BN_SC * fp + cp] = sc;
    bn[BN_SH * fp + cp] = beta - mu * sc;
    bn[BN_MU * fp + cp] = mu;
    bn[BN_INV * fp + cp] = inv;
}

struct ApplyArgs {
    eagcn_batch bt;
    ViewCols vc;
    int structure, fp;
    const float* Y; int ldy;
    const float* bn;
    const float* colp;
    float* out; int ldo;
    float* pad_row;
    int do_drop; uint32_t thr; float inv_keep; uint64_t seed; const uint64_t* seed_dev;
    BxOut planes;                // optional: the operand planes of the next layer's products (gemm_bx3.hip), written here
    int tile_map;                // element -> lane map: 0: row-major groups of four columns (a wavefront = 256 columns of one row: eight
                                 // 64-byte pieces per plane image); 1: a wavefront = 8 rows x one 32-column panel = 512 CONTIGUOUS bytes
                                 // of every plane image (bx3.h: panel-major) and eight 128-byte row segments of the fp32 matrices
};

__global__ __launch_bounds__(256) void bn_apply_kernel(ApplyArgs a) {
    const int fp = a.fp;
    const uint64_t seed = a.seed_dev ? *a.seed_dev : a.seed;   // (never write to the by-value argument block:
                                                               //  that would demote it to scratch memory)
    if (blockIdx.x == 0) {   // value of the rows that are not stored
        for (int c = threadIdx.x; c < a.ldo; c += blockDim.x) {
            float v = 0.0f;
            if (a.structure == EAGCN_STRUCT_WEIGHTED)
                for (int k = 0; k < a.vc.K; ++k) {
                    const int cp = a.vc.off[k] + c;
                    v += a.colp[CP_AVEW * fp + cp] * fmaxf(a.bn[BN_SH * fp + cp], 0.0f);
                }
            a.pad_row[c] = v;
        }
    }
    const int T = dev_rows(a.bt);
    // (element index -> (row, column group) with a 32-bit division: T * columns / 4 of any batch that fits the index fits 31 bits)
    if (a.structure == EAGCN_STRUCT_CONCATE) {
        const uint32_t g4 = a.tile_map ? ((uint32_t)(fp + 31) >> 5) : fp / 4;
        const uint32_t total = a.tile_map ? (((uint32_t)T + 7) >> 3) * g4 * 64u : (uint32_t)T * g4;
        for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
            int r, c;
            if (a.tile_map) {                        // 64 lanes = 8 rows x one 32-column panel (see ApplyArgs.tile_map)
                const uint32_t it = e >> 6, rg = it / g4;
                r = (int)(rg * 8u + ((e >> 3) & 7u)); c = (int)((it - rg * g4) * 32u + (e & 7u) * 4u);
                if (r >= T || c >= fp) continue;
            } else {
                r = (int)(e / g4); c = (int)(e - (uint32_t)r * g4) * 4;
            }
            const float4 y = *reinterpret_cast<const float4*>(a.Y + (size_t)r * a.ldy + c);
            const float4 sc = *reinterpret_cast<const float4*>(a.bn + BN_SC * fp + c);
            const float4 sh = *reinterpret_cast<const float4*>(a.bn + BN_SH * fp + c);
            const float m = a.bt.row_m[r];
            float4 o;
            o.x = fmaxf(y.x * sc.x + sh.x, 0.0f) * m;
            o.y = fmaxf(y.y * sc.y + sh.y, 0.0f) * m;
            o.z = fmaxf(y.z * sc.z + sh.z, 0.0f) * m;
            o.w = fmaxf(y.w * sc.w + sh.w, 0.0f) * m;
            if (a.do_drop) {
                float ds[4];
                drop_scale4(seed, (uint64_t)r * fp + c, a.thr, a.inv_keep, ds);
                o.x *= ds[0]; o.y *= ds[1]; o.z *= ds[2]; o.w *= ds[3];
            }
            if (a.out) *reinterpret_cast<float4*>(a.out + (size_t)r * a.ldo + c) = o;
            if (a.planes.p) bx_store4(a.planes, r, c, o);
        }
    } else {
        // weighted sum over the views: a thread owns four adjacent output columns, the K view loads of a row are independent
        // 16-byte loads (view column ranges and the output pitch are multiples of 16)
        const uint32_t g4 = a.tile_map ? ((uint32_t)(a.ldo + 31) >> 5) : a.ldo / 4;
        const uint32_t total = a.tile_map ? (((uint32_t)T + 7) >> 3) * g4 * 64u : (uint32_t)T * g4;
        for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
            int r, f;
            if (a.tile_map) {
                const uint32_t it = e >> 6, rg = it / g4;
                r = (int)(rg * 8u + ((e >> 3) & 7u)); f = (int)((it - rg * g4) * 32u + (e & 7u) * 4u);
                if (r >= T || f >= a.ldo) continue;
            } else {
                r = (int)(e / g4); f = (int)(e - (uint32_t)r * g4) * 4;
            }
            float4 y[EAGCN_MAX_VIEWS];
#pragma unroll
            for (int k = 0; k < EAGCN_MAX_VIEWS; ++k)
                if (k < a.vc.K) y[k] = *reinterpret_cast<const float4*>(a.Y + (size_t)r * a.ldy + a.vc.off[k] + f);
            float4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < EAGCN_MAX_VIEWS; ++k)
                if (k < a.vc.K) {
                    const int cp = a.vc.off[k] + f;
                    const float4 sc = *reinterpret_cast<const float4*>(a.bn + BN_SC * fp + cp);
                    const float4 sh = *reinterpret_cast<const float4*>(a.bn + BN_SH * fp + cp);
                    const float4 w = *reinterpret_cast<const float4*>(a.colp + CP_AVEW * fp + cp);
                    float4 p;
                    p.x = fmaxf(y[k].x * sc.x + sh.x, 0.0f);
                    p.y = fmaxf(y[k].y * sc.y + sh.y, 0.0f);
                    p.z = fmaxf(y[k].z * sc.z + sh.z, 0.0f);
                    p.w = fmaxf(y[k].w * sc.w + sh.w, 0.0f);
                    if (a.do_drop) {
                        float ds[4];
                        drop_scale4(seed, (uint64_t)r * fp + cp, a.thr, a.inv_keep, ds);
                        p.x *= ds[0]; p.y *= ds[1]; p.z *= ds[2]; p.w *= ds[3];
                    }
                    acc.x += w.x * p.x; acc.y += w.y * p.y; acc.z += w.z * p.z; acc.w += w.w * p.w;
                }
            if (a.out) *reinterpret_cast<float4*>(a.out + (size_t)r * a.ldo + f) = acc;
            if (a.planes.p) bx_store4(a.planes, r, f, acc);
        }
    }
}

// ---- BatchNorm backward ----------------------------------------------------------------------------
struct BwdArgs {
    const int32_t* meta; int Tcap;       // (only what the kernel reads of the batch index: the argument block stays in SGPRs)
    const int32_t* row_mol;
    const float* row_m;
    ViewCols vc;
    int structure, fp, nvirt;
    const float* dxout; int ldo;
    ReadoutGrad rg;              // rg.dg != null: the upstream gradient is dg[row_mol[r]] (dxout unused)
    const float* dpad;           // [ldo] gradient of the common non-stored row, or null
    int dpad_views;              // dpad is [K][ldo]: one row per view (sampled dropout of the non-stored rows)
    const float* Y; int ldy;
    const float* bn;
    const float* colp;
    float* dH;                   // [T][fp]
    double* slab;                // [grid][fp][2]
    double* slab_da;             // [grid][MAX_VIEWS]
    int do_drop; uint32_t thr; float inv_keep; uint64_t seed; const uint64_t* seed_dev;
    double* zero; int nzero;     // fp64 words cleared on the way (the head's backward sums, for the next backward call)
    EdgeDrain drain;             // pending edge-gradient reduction of the layer above (eacc == nullptr: none)
    const float* cc;             // APPLY pass: [2][fp] means of dH and of dH * xhat (bn_bwd_finalize)
    int store_dh;                // first pass also stores dH (EAGCN_BWD_STORE_DH=1: the elementwise second pass of round 2 reads it)
};

// One workgroup owns BWD_ROWS consecutive-strided rows; a thread owns FOUR adjacent columns (one float4 per row
// and operand) and has all BWD_ROWS rows in flight at once: a single batch of independent 16-byte loads
// instead of a column loop of scalar ones.  View column ranges are multiples of 16, so the four columns share
// their view.
// Compile-time variants (structure, per-molecule upstream gradient, dropout): the general kernel carried every path at once
// -- 7.7 k instructions, scalar registers spilled to vector lanes, a few hundred exec-mask branches -- and was bound by
// that, not by memory.
// Two passes share this body, so that both form dH = upstream * dropout * relu' in exactly the same way:
//   APPLY = false: the column sums of dH and dH * xhat (fp64 slabs); dH itself is NOT stored;
//   APPLY = true (after bn_bwd_finalize): dH is formed again and dY' = sc * (dH - c1 - xhat * c2) is written.
// (Round 2 stored dH in the first pass and re-read it in an elementwise second one: one write and one read of T x Fp floats
//  more than re-forming it from Y and the upstream gradient, which the second pass reads anyway or gathers per molecule.)
template <bool WEIGHTED, bool DG, bool DROP, bool APPLY>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(BwdArgs a) {
    __shared__ double da_s[EAGCN_MAX_VIEWS];
    const uint64_t seed = DROP ? (a.seed_dev ? *a.seed_dev : a.seed) : 0ull;
    const int fp = a.fp, T = min(a.meta[EAGCN_META_T], a.Tcap);
    const int rows = T + (APPLY ? 0 : a.nvirt);
    // the grid is sized for the row CAPACITY: only the first ceil(rows / BWD_ROWS) workgroups work (and write a
    // slab); bn_bwd_finalize derives the same count from the device-side row count
    const int nwg = max(1, min((int)gridDim.x, (rows + BWD_ROWS - 1) / BWD_ROWS));
    if (!APPLY && a.drain.eacc && blockIdx.x == 0 && blockIdx.y == 0) {
        // the layer above left its bond-type histograms in the shared accumulator slabs: reduce them into its d att.weight /
        // d self_r and leave the slabs zero for this layer's own edge gradients (agg_edge runs after this kernel)
        const int K = a.drain.K;
        for (int e = threadIdx.x; e < K * EDGE_SLAB; e += blockDim.x) {
            const int k = e / EDGE_SLAB, c = e - k * EDGE_SLAB;
            if (c > 256) continue;
            double v[EDGE_COPIES];
#pragma unroll
            for (int z = 0; z < EDGE_COPIES; ++z) v[z] = a.drain.eacc[((size_t)z * K + k) * EDGE_SLAB + c];
            double t = 0.0;
#pragma unroll
            for (int z = 0; z < EDGE_COPIES; ++z) { t += v[z]; a.drain.eacc[((size_t)z * K + k) * EDGE_SLAB + c] = 0.0; }
            float* dw = nullptr;
            float* dr = nullptr;
            int ch = 0;
#pragma unroll
            for (int q = 0; q < EAGCN_MAX_VIEWS; ++q)
                if (q == k) { dw = a.drain.datt_w[q]; dr = a.drain.dself_r[q]; ch = a.drain.channels[q]; }
            if (c == 256) {
                const double r = (double)a.drain.rsig[k];
                dr[0] = (float)(t * r * (1.0 - r));
            } else if (c >= 1 && c <= ch) {
                dw[c - 1] = (float)t;
            }
        }
    }
    if ((int)blockIdx.x >= nwg || (APPLY && T == 0)) return;
    if constexpr (!APPLY) {
        if (threadIdx.x < EAGCN_MAX_VIEWS) da_s[threadIdx.x] = 0.0;
        __syncthreads();
    }
    constexpr bool weighted = WEIGHTED;
    double da[EAGCN_MAX_VIEWS];
#pragma unroll
    for (int k = 0; k < EAGCN_MAX_VIEWS; ++k) da[k] = 0.0;
    // grid.y cuts the columns into chunks of 1024 (one pass of the workgroup): a wide layer (Fp = 6320 at the HIV widths) is
    // limited to a few hundred row blocks by the size of its partial slabs -- too few waves to stream at HBM rate
    const int c_lo = blockIdx.y * (int)blockDim.x * 4;
    for (int cp = c_lo + threadIdx.x * 4; cp < min(fp, c_lo + (int)blockDim.x * 4); cp += blockDim.x * 4) {
        const int k = col_view(a.vc, cp), f = cp - a.vc.off[k];
        const float4 sc = *reinterpret_cast<const float4*>(a.bn + BN_SC * fp + cp);
        const float4 sh = *reinterpret_cast<const float4*>(a.bn + BN_SH * fp + cp);
        const float4 mu = *reinterpret_cast<const float4*>(a.bn + BN_MU * fp + cp);
        const float4 iv = *reinterpret_cast<const float4*>(a.bn + BN_INV * fp + cp);
        const float4 aw = *reinterpret_cast<const float4*>(a.colp + CP_AVEW * fp + cp);
        float4 c1 = make_float4(0.f, 0.f, 0.f, 0.f), c2 = c1;
        if constexpr (APPLY) {
            c1 = *reinterpret_cast<const float4*>(a.cc + cp);
            c2 = *reinterpret_cast<const float4*>(a.cc + fp + cp);
        }
        const int cu = weighted ? f : cp;           // first column of the upstream gradient
        // ... and its exact column when that gradient is per molecule (ce4: the four columns are consecutive
        // exact columns, 16-byte aligned -> one load; otherwise each is looked up on its own)
        auto exact = [&](int c) {
            int eo = 0, po = 0, res = -1;
            bool done = false;
#pragma unroll
            for (int sg = 0; sg < EAGCN_MAX_SEGS; ++sg) {     // unrolled: constant indices into the argument block
                if (sg < a.rg.map.nseg && !done) {
                    if (c < po + a.rg.map.p[sg]) { res = (c - po < a.rg.map.w[sg]) ? eo + (c - po) : -1; done = true; }
                    eo += a.rg.map.w[sg];
                    po += a.rg.map.p[sg];
                }
            }
            return res;
        };
        int ce0 = -1, ce1 = -1, ce2 = -1, ce3 = -1;                // exact columns of the four packed columns: once per thread
        bool ce4 = false;
        if constexpr (DG) {
            ce0 = exact(cu); ce1 = exact(cu + 1); ce2 = exact(cu + 2); ce3 = exact(cu + 3);
            ce4 = ce0 >= 0 && ce3 == ce0 + 3 && (ce0 & 3) == 0 && (a.rg.F & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(a.rg.dg) & 15) == 0;
        }
        double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0}, dak = 0.0;
        for (int rb = blockIdx.x; rb < rows; rb += BWD_ROWS * nwg) {
            float4 yv[BWD_ROWS], upv[BWD_ROWS];
#pragma unroll
            for (int u = 0; u < BWD_ROWS; ++u) {
                const int r = rb + u * nwg;
                yv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                upv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r < T) {
                    yv[u] = *reinterpret_cast<const float4*>(a.Y + (size_t)r * a.ldy + cp);
                    if constexpr (DG) {
                        const int mol = a.row_mol[r];
                        const float* g = a.rg.dg + (size_t)mol * a.rg.F;
                        float4 v;
                        if (ce4) {
                            v = *reinterpret_cast<const float4*>(g + ce0);
                        } else {
                            v.x = ce0 >= 0 ? g[ce0] : 0.0f;
                            v.y = ce1 >= 0 ? g[ce1] : 0.0f;
                            v.z = ce2 >= 0 ? g[ce2] : 0.0f;
                            v.w = ce3 >= 0 ? g[ce3] : 0.0f;
                        }
                        if (a.rg.mode == 1) {
                            const float is = 1.0f / (float)a.rg.size[mol];
                            v.x *= is; v.y *= is; v.z *= is; v.w *= is;
                        }
                        upv[u] = v;
                    } else {
                        upv[u] = *reinterpret_cast<const float4*>(a.dxout + (size_t)r * a.ldo + cu);
                    }
                    if (!weighted) {
                        const float m = a.row_m[r];
                        upv[u].x *= m; upv[u].y *= m; upv[u].z *= m; upv[u].w *= m;
                    }
                } else if (r < rows) {                 // the one virtual row standing for all non-stored rows
                    upv[u] = *reinterpret_cast<const float4*>(a.dpad + (size_t)(a.dpad_views ? k : (r - T)) * a.ldo + cu);
                }
            }
#pragma unroll
            for (int u = 0; u < BWD_ROWS; ++u) {
                const int r = rb + u * nwg;
                if (r >= rows) continue;
                const float yy[4] = {yv[u].x, yv[u].y, yv[u].z, yv[u].w};
                const float uu[4] = {upv[u].x, upv[u].y, upv[u].z, upv[u].w};
                const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
                const float muv[4] = {mu.x, mu.y, mu.z, mu.w}, ivv[4] = {iv.x, iv.y, iv.z, iv.w};
                const float awv[4] = {aw.x, aw.y, aw.z, aw.w};
                const float c1v[4] = {c1.x, c1.y, c1.z, c1.w}, c2v[4] = {c2.x, c2.y, c2.z, c2.w};
                float dh[4], dsv[4] = {1.0f, 1.0f, 1.0f, 1.0f};
                if (DROP && r < T) drop_scale4(seed, (uint64_t)r * fp + cp, a.thr, a.inv_keep, dsv);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float up = uu[j];
                    const float ds = dsv[j];
                    const float h = yy[j] * scv[j] + shv[j];
                    if (weighted) { if constexpr (!APPLY) dak += (double)(up * ds * fmaxf(h, 0.0f)); up *= awv[j]; }
                    dh[j] = h > 0.0f ? up * ds : 0.0f;
                    const float xh = (yy[j] - muv[j]) * ivv[j];
                    if constexpr (APPLY) {
                        dh[j] = scv[j] * (dh[j] - c1v[j] - xh * c2v[j]);
                    } else {
                        s1[j] += (double)dh[j];
                        s2[j] += (double)(dh[j] * xh);
                    }
                }
                if ((APPLY || a.store_dh) && r < T)
                    *reinterpret_cast<float4*>(a.dH + (size_t)r * fp + cp) = make_float4(dh[0], dh[1], dh[2], dh[3]);
            }
        }
        if constexpr (!APPLY) {
            double* sl = a.slab + ((size_t)blockIdx.x * fp + cp) * 2;
            *reinterpret_cast<double4*>(sl) = make_double4(s1[0], s2[0], s1[1], s2[1]);
            *reinterpret_cast<double4*>(sl + 4) = make_double4(s1[2], s2[2], s1[3], s2[3]);
            if (weighted) {
#pragma unroll
                for (int v = 0; v < EAGCN_MAX_VIEWS; ++v) da[v] += (v == k) ? dak : 0.0;
            }
        }
    }
    if (weighted && !APPLY) {
#pragma unroll
        for (int v = 0; v < EAGCN_MAX_VIEWS; ++v) {
            const double t = wave_sum(da[v]);
            if ((threadIdx.x & 63) == 0 && t != 0.0) atomicAdd(&da_s[v], t);
        }
        __syncthreads();
        if (threadIdx.x < EAGCN_MAX_VIEWS)
            a.slab_da[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * EAGCN_MAX_VIEWS + threadIdx.x] = da_s[threadIdx.x];
    }
}

template <int L>
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const double* __restrict__ slab,
                                                               const double* __restrict__ slab_da, int nslab,
                                                               int fp, double M, int training,
                                                               const float* __restrict__ bn, ViewCols vc,
                                                               GradPtrs gp, float* __restrict__ cc, const int32_t* __restrict__ meta, int nvirt,
                                                               int batch_B, int da_chunks, int da_stride,
                                                               const double* __restrict__ gsum, double* __restrict__ zero, int nzero,
                                                               int exact_slabs) {
    // fp64 words cleared on the way (the head's backward sums, for the next backward call; every reader -- the reduction in
    // front of this launch reads Graph_BN's sums -- is done by now)
    if (blockIdx.x == 0 && zero)
        for (int i = threadIdx.x; i < nzero; i += blockDim.x) zero[i] = 0.0;
    if (meta[EAGCN_META_NLOG] > 0) M = (double)batch_B * (double)meta[EAGCN_META_NLOG];
    // slabs actually written (exact_slabs: they do not come from the row pass -- HeadTopSums writes every one whatever the row count)
    // (exact_slabs == 2: one per BX_EPI_ROWS packed rows, written by the dX product of the layer above -- bx3.h BxBnEpi; no row: no slab)
    if (!exact_slabs) nslab = max(1, min(nslab, (meta[EAGCN_META_T] + nvirt + BWD_ROWS - 1) / BWD_ROWS));
    else if (exact_slabs == 2) nslab = min(nslab, (max(meta[EAGCN_META_T], 0) + BX_EPI_ROWS - 1) / BX_EPI_ROWS);
    const int cpr = blockIdx.x * (256 / L) + threadIdx.x / L, sl = threadIdx.x % L;
    const int cp = min(cpr, fp - 1);
    if (blockIdx.x == 0 && gp.dave_w) {                 // d ave.weight: 32 lanes per view over the row-partial slabs
        const int v = threadIdx.x >> 5, l = threadIdx.x & 31;
        double t = 0.0;
        if (v < vc.K)
            for (int y = 0; y < da_chunks; ++y)             // (column chunk y of the reduce grid, row block s)
                for (int s = l; s < nslab; s += 32) t += slab_da[((size_t)y * da_stride + s) * EAGCN_MAX_VIEWS + v];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) t += __shfl_xor(t, o);
        if (v < vc.K && l == 0) gp.dave_w[v] = (float)t;
    }
    double s1, s2;
    slab_sum<L>(slab, nslab, fp, cp, sl, s1, s2);
    if (cpr >= fp || sl != 0) return;
    {   // the means of dY = sc (dH - c1 - xhat c2) run over ALL rows of the BatchNorm: with sync-BatchNorm those of every rank
        double g1 = s1, g2 = s2;
        if (gsum) { g1 = gsum[2 * cp]; g2 = gsum[2 * cp + 1]; M = gsum[2 * fp]; }
        cc[cp] = training ? (float)(g1 / M) : 0.0f;
        cc[fp + cp] = training ? (float)(g2 / M) : 0.0f;
    }
    const int k = col_view(vc, cp), f = cp - vc.off[k];
    if (f < vc.width[k]) {
        gp.dgamma[k][f] = (float)s2;
        gp.dbeta[k][f] = (float)s1;
        // training: sum over ALL B*N rows of dY is identically zero (mean removal); eval: sc * sum(dH)
        gp.dbias[k][f] = training ? 0.0f : (float)((double)bn[BN_SC * fp + cp] * s1);
    }
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(eagcn_batch bt, int fp, const float* __restrict__ Y, int ldy,
                                                            const float* __restrict__ bn,
                                                            const float* __restrict__ cc, float* __restrict__ dH) {
    const uint32_t g4 = fp / 4;
    const uint32_t total = (uint32_t)dev_rows(bt) * g4;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int r = (int)(e / g4), c = (int)(e - (uint32_t)r * g4) * 4;
        const float4 y = *reinterpret_cast<const float4*>(Y + (size_t)r * ldy + c);
        float4 d = *reinterpret_cast<float4*>(dH + (size_t)r * fp + c);
        const float4 sc = *reinterpret_cast<const float4*>(bn + BN_SC * fp + c);
        const float4 mu = *reinterpret_cast<const float4*>(bn + BN_MU * fp + c);
        const float4 iv = *reinterpret_cast<const float4*>(bn + BN_INV * fp + c);
        const float4 c1 = *reinterpret_cast<const float4*>(cc + c);
        const float4 c2 = *reinterpret_cast<const float4*>(cc + fp + c);
        d.x = sc.x * (d.x - c1.x - (y.x - mu.x) * iv.x * c2.x);
        d.y = sc.y * (d.y - c1.y - (y.y - mu.y) * iv.y * c2.y);
        d.z = sc.z * (d.z - c1.z - (y.z - mu.z) * iv.z * c2.z);
        d.w = sc.w * (d.w - c1.w - (y.w - mu.w) * iv.w * c2.w);
        *reinterpret_cast<float4*>(dH + (size_t)r * fp + c) = d;
    }
}

// grid.x = ceil(ld_in*fp / 256) blocks for dW (one thread per element, sum over the split-K slabs) followed by
// ceil(K*EDGE_SLAB / 16) blocks for the edge-gradient partials (16 lanes per entry)
__global__ __launch_bounds__(256) void unpack_grads_kernel(GradPtrs gp, ParamPtrs pp, ViewCols vc, ColMapD in,
                                                            int ld_in, int fp, const float* __restrict__ dWcat,
                                                            int nsplit, size_t slab, double* __restrict__ datt,
                                                            int nedge, const float* __restrict__ rsig, int wblocks,
                                                            const int32_t* __restrict__ meta, int xk_G, int edge_drain, int bx_per, int bx_wide,
                                                            int all_slabs) {
    nedge = nedge < 0 ? -nedge : min(nedge, (meta[EAGCN_META_T] + 15) / 16);   // edge-gradient workgroups that had rows (< 0: all wrote)
    // split-K partials actually written: gemm.hip writes eff_splits of them; the plane GEMM (gemm_bx3.hip) passes its slab count
    // negated and writes bx3_used_splits() of them
    // (bx_per > 0: the weight gradient shared its launch with the dX product -- T x ld_in over fp -- and sized its chunks against it)
    // (tiles of the kernel that wrote them: 128 x 128, or 256 x 128 for gemm_bx3w.hip)
    const int bxm = bx_wide ? BX3W_BM : BX3_BM, bxn = bx_wide ? BX3W_BN : BX3_BN;
    nsplit = nsplit < 0 ? bx3_used_splits_wave(-nsplit, meta[EAGCN_META_T], ((ld_in + bxm - 1) / bxm) * ((fp + bxn - 1) / bxn),
                                          bx_per > 0 ? ((meta[EAGCN_META_T] + bxm - 1) / bxm) * ((ld_in + bxn - 1) / bxn) : 0, max(1, (fp + 31) >> 5), bx_per)
                        : all_slabs ? nsplit                         // (lagg_dw.hip: one slab per workgroup row, every one written)
                        : max(1, min(nsplit, meta[EAGCN_META_T] >> 7));
    if ((int)blockIdx.x < wblocks) {
        // split-K slabs: FOUR lanes per group of four adjacent elements (one 16-byte load per slab: a wavefront covers 256 contiguous
        // bytes of four slabs), each lane adds every fourth slab (the first layer's weight gradient leaves gemm.hip as up to 146 slabs:
        // one thread per element was a chain of 37 dependent load rounds, 14 us at B = 1024; four lanes per SINGLE element, 64-byte
        // pieces: 15 us for the 14 slabs of configs[1]'s hidden layer)
        const int tid = blockIdx.x * blockDim.x + threadIdx.x;
        if (xk_G > 0) {
            const int e = tid;
            if (e >= ld_in * fp) return;
            const int ip = e / fp, cp = e % fp;
            const int k = col_view(vc, cp), f = cp - vc.off[k];
            const int fi = packed_to_exact(in, ip);
            if (fi < 0 || f >= vc.width[k]) return;
            // partial slabs of the XCD-local paired GEMM (gemm3.hip, kernels.h g3_plan): slab x exists iff segment x holds
            // k-steps of the dW product; summed in segment order (deterministic)
            const int T = meta[EAGCN_META_T];
            G3Plan pl;
            g3_plan((T + 63) / 64, (ld_in + 63) / 64, max(1, (fp + 15) / 16), ((ld_in + 63) / 64) * ((fp + 63) / 64),
                    max(1, (T + 15) / 16), xk_G, pl);
            float v[G3_XSEG];
#pragma unroll
            for (int x = 0; x < G3_XSEG; ++x) v[x] = pl.c[x + 1] > pl.c[x] ? dWcat[(size_t)x * slab + e] : 0.0f;
            float t = 0.0f;
#pragma unroll
            for (int x = 0; x < G3_XSEG; ++x) t += v[x];
            gp.dW[k][(size_t)fi * vc.width[k] + f] = T > 0 ? t : 0.0f;
            return;
        }
        const int sub = tid & 3;
        const int e = (tid >> 2) * 4;                                // (fp is a multiple of 16: the four elements share row and view)
        if (e >= ld_in * fp) return;
        const int ip = e / fp, cp = e % fp;
        const int k = col_view(vc, cp), f = cp - vc.off[k];
        const int fi = packed_to_exact(in, ip);
        if (fi < 0 || f >= vc.width[k]) return;
        float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
        int z = sub;
#pragma unroll 4
        for (; z + 4 < nsplit; z += 8) {
            const float4 a0 = *reinterpret_cast<const float4*>(dWcat + (size_t)z * slab + e);
            const float4 a1 = *reinterpret_cast<const float4*>(dWcat + (size_t)(z + 4) * slab + e);
            s0.x += a0.x; s0.y += a0.y; s0.z += a0.z; s0.w += a0.w;
            s1.x += a1.x; s1.y += a1.y; s1.z += a1.z; s1.w += a1.w;
        }
        if (z < nsplit) {
            const float4 a0 = *reinterpret_cast<const float4*>(dWcat + (size_t)z * slab + e);
            s0.x += a0.x; s0.y += a0.y; s0.z += a0.z; s0.w += a0.w;
        }
        float t[4] = {s0.x + s1.x, s0.y + s1.y, s0.z + s1.z, s0.w + s1.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) { t[j] += __shfl_xor(t[j], 1); t[j] += __shfl_xor(t[j], 2); }
        // lane j of the four stores element j
        const float tv = sub == 0 ? t[0] : sub == 1 ? t[1] : sub == 2 ? t[2] : t[3];
        if (f + sub < vc.width[k]) gp.dW[k][(size_t)fi * vc.width[k] + f + sub] = tv;
        return;
    }
    // edge-gradient partials [nedge][K][EDGE_SLAB]: entry c in 1..C_k -> d att_w[c-1]; entry 256 -> self term.
    // General relation vectors (pp.rel_vec[k]): the histogram is per bond CODE, the gradient per CHANNEL:
    //   d att_w[ch] = sum_codes h[code] * vec[code][ch]  -- entry ch of view k sums over all codes (rare path, not tuned)
    const int er = ((int)blockIdx.x - wblocks) * 16 + (threadIdx.x >> 4), sl = threadIdx.x & 15;
    const int tot = vc.K * EDGE_SLAB;
    const int e = min(er, tot - 1);
    const int k = e / EDGE_SLAB, c = e % EDGE_SLAB;
    const bool general = pp.rel_vec[k] != nullptr && c != 256;
    double t = 0.0;
    if (!general) {
        for (int z0 = sl; z0 < nedge; z0 += 16 * 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int z = z0 + 16 * u;
                v[u] = z < nedge ? datt[(size_t)z * tot + e] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) t += v[u];
            if (edge_drain && er < tot) {                  // shared accumulator slabs: every element is read by exactly one lane
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int z = z0 + 16 * u;
                    if (z < nedge) datt[(size_t)z * tot + e] = 0.0;
                }
            }
        }
    } else if (c >= 1 && c <= pp.rel_c[k]) {
        const float* vec = pp.rel_vec[k];
        const int C = pp.rel_c[k], D = pp.channels[k];
        for (int z = sl; z < nedge; z += 16)
            for (int code = 1; code <= D; ++code)
                t += datt[(size_t)z * tot + k * EDGE_SLAB + code] * (double)vec[(size_t)(code - 1) * C + (c - 1)];
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if (er >= tot || sl != 0) return;
    if (c == 256) {
        const double r = (double)rsig[k];
        gp.dself_r[k][0] = (float)(t * r * (1.0 - r));
    } else if (c >= 1 && c <= (pp.rel_vec[k] ? pp.rel_c[k] : pp.channels[k])) {
        gp.datt_w[k][c - 1] = (float)t;
    }
}

// A1_k[b,i,j] = sigmoid(w_k[type]) * adj  -- the A_weight return value of layers.py:318 (stack of the
// per-view A1 of layers.py:83), materialised only when a caller asks for it.
__global__ __launch_bounds__(256) void attention_dense_kernel(eagcn_batch bt, ParamPtrs pp, float* __restrict__ out) {
    const size_t total = (size_t)bt.K * bt.B * bt.N * bt.N;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(e % bt.N);
        const size_t kbi = e / bt.N;                 // (k*B + b)*N + i
        const int k = (int)(kbi / ((size_t)bt.B * bt.N));
        const size_t bi = kbi - (size_t)k * bt.B * bt.N;      // b*N + i: rows without bonds have no valid code row
        const uint32_t c = bt.deg_bn[bi] > 0 ? bt.code[kbi * bt.ldc + j] : 0u;
        out[e] = (c >= 1 && (int)c <= pp.channels[k]) ? sigmoidf_(att_logit(pp, k, (int)c)) : 0.0f;
    }
}

// ---- scratch carving -------------------------------------------------------------------------------
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* p) : base((char*)p) {}
    template <typename T>
    T* take(size_t n) {
        T* p = base ? (T*)(base + off) : nullptr;
        off = align256(off + n * sizeof(T));
        return p;
    }
};

struct LayerDims {
    ViewCols vc;
    int fp, ld_in, fin, ldo, gx, gxb, nsplit;
    int gslab;                   // capacity of the forward BatchNorm partial slabs (the aggregation kernels' grids)
    size_t wslab;
    size_t wpslab, wtpslab;      // plane images (bx3.h) of Wcat [ld_in rows][fp] and WcatT [fp rows][ld_in]
    int np;                      // 3 / 1: this layer's products run from bf16 operand planes (gemm_bx3.hip); 0: fp32 operands
    int bx_splits;               // ... and its weight gradient leaves as this many k-chunk slabs
};
// the forward aggregation of this batch runs on the LDS-staged kernel (lagg.hip; one BatchNorm slab per row block): asked by
// layer_dims for the slab capacity and by plan_layer for the kernel
static bool fwd_agg_lagg(const eagcn_batch* b, const ViewCols& vc) { return lagg_use(b, 0, false, &vc); }
static LayerDims layer_dims(const eagcn_batch* b, const eagcn_layer_params* p) {
    LayerDims d;
    d.vc = view_cols(p);
    d.fp = d.vc.off[p->K];
    d.ld_in = layout_ld(&p->in);
    d.fin = layout_width(&p->in);
    d.ldo = p->structure == EAGCN_STRUCT_CONCATE ? d.fp : pad16(p->width[0]);
    d.gx = agg_grid_x(b);
    d.gslab = std::max(d.gx, fwd_agg_lagg(b, d.vc) ? lagg_slabs(b) : 0);
    // row-partial slabs of the BatchNorm backward: 7 rows per workgroup, at most 2048 workgroups and at most
    // 32 MB of fp64 partials (wide layers: Fp = 6320 -> 331 workgroups).  Fewer, longer workgroups were measured
    // slower (the kernel is bound by its instruction stream and one memory round trip per 7-row batch, not by the
    // partial slabs: cap 512 -> +4 us, 192 -> +22 us at the Tox21 shape)
    {
        const long by_rows = cdiv(b->T + 1, BWD_ROWS);
        const long by_bytes = std::max<long>(64, (32L << 20) / ((long)d.fp * 16));
        d.gxb = (int)std::max<long>(1, std::min<long>(std::min<long>(by_rows, 2048), by_bytes));
    }
    const int tiles = cdiv(d.ld_in, 64) * cdiv(d.fp, 64);
    d.nsplit = std::max(1, std::min(std::max(1, 1024 / tiles), cdiv(std::max(b->T, 1), 128)));
    d.wslab = (size_t)d.ld_in * d.fp;
    d.wpslab = bx_plane_elems(d.ld_in, d.fp);
    d.wtpslab = bx_plane_elems(d.fp, d.ld_in);
    // plane GEMMs (gemm modes 3 / 4): the hidden layers (the 24-feature first layer stays on the fp32 kernels of gemm.hip)
    d.np = (d.ld_in >= 128 && (d.ld_in & 15) == 0 && (d.fp & 15) == 0) ? gemm_planes() : 0;
    // slab capacity of the weight gradient's k-chunks (how many are used is decided on the device from the actual row count:
    // bx3.h bx3_used_splits)
    // (at most 64 slabs, but never k-chunks beyond the 4096 rows gemm_bx3.hip's accumulation chains are bounded to: T > 262144 rows
    //  takes more slabs instead of longer chunks; < 1024 = the key packing of bx3_used_splits_wave)
    d.bx_splits = std::max(1, std::min(std::min(1023, std::max(64, cdiv(std::max(b->T, 1), 4096))), std::max(cdiv(std::max(b->T, 1), 4096), cdiv(std::max(b->T, 1), 256))));
    return d;
}

struct Packed { float *Wcat, *WcatT, *colp, *sig, *rsig; uint16_t *Wp, *WTp; };   // Wp / WTp: [np][ld_in * fp] operand planes
static Packed take_packed(Carver& c, const LayerDims& d) {
    Packed t;
    t.Wcat = c.take<float>(d.wslab);
    t.WcatT = c.take<float>(d.wslab);
    t.colp = c.take<float>((size_t)CP_ROWS * d.fp);
    t.sig = c.take<float>(EAGCN_MAX_VIEWS * 256);
    t.rsig = c.take<float>(EAGCN_MAX_VIEWS);
    t.Wp = c.take<uint16_t>(d.np ? (size_t)d.np * d.wpslab : 1);
    t.WTp = c.take<uint16_t>(d.np ? (size_t)d.np * d.wtpslab : 1);
    return t;
}
static size_t carve_packed(void* base, const LayerDims& d, Packed* s) {
    Carver c(base);
    const Packed t = take_packed(c, d);
    if (s) *s = t;
    return c.off;
}
// The scratch block of a forward (stats) or a backward (dY .. datt, dPp) call.  Both carvings start alike:
struct LayerScratch {
    void* gws;                   // GEMM hand-off workspace: FIRST, so that every layer of a model and both directions share one
                                 // region (one flag clear per API call, kernels.h gemm3_clear_flags)
    double* eacc;                // edge-gradient accumulator slabs (kernels.h EDGE_COPIES): right behind it, zero between uses
    Packed pk;                   // the packed parameters -- or the caller's block (eagcn_layer_bufs.packed)
    double* stats;
    float *dY, *dP, *cc, *dWcat;
    double *slab, *slab_da, *datt, *gsum;
    uint16_t *dPp, *xp;          // planes of dP (written by the transposed aggregation) and of x when the caller did not bring them
};
static size_t carve_layer(void* base, const eagcn_batch* b, const LayerDims& d, bool bwd, LayerScratch* s) {
    Carver c(base);
    LayerScratch t{};
    t.gws = c.take<char>(gemm3_workspace_bytes());
    t.eacc = (double*)c.take<char>(edge_acc_bytes());
    t.pk = take_packed(c, d);
    if (!bwd) t.stats = c.take<double>((size_t)d.gslab * d.fp * 2);
    else {
        t.dY = c.take<float>((size_t)std::max(b->T, 1) * d.fp);
        t.dP = c.take<float>((size_t)std::max(b->T, 1) * d.fp);
        t.cc = c.take<float>((size_t)2 * d.fp);
        t.dWcat = c.take<float>(d.wslab * std::max(std::max(d.nsplit, G3_XSEG), d.np ? d.bx_splits : 1));
        t.slab = c.take<double>((size_t)d.gxb * d.fp * 2);
        t.slab_da = c.take<double>((size_t)d.gxb * cdiv(d.fp, 1024) * EAGCN_MAX_VIEWS);
        t.datt = c.take<double>((size_t)edge_grid_x(b) * EAGCN_MAX_VIEWS * EDGE_SLAB);
    }
    t.gsum = c.take<double>((size_t)2 * d.fp + 8);
    if (bwd) t.dPp = c.take<uint16_t>(d.np ? (size_t)d.np * bx_plane_elems(b->T, d.fp) : 1);
    t.xp = c.take<uint16_t>(d.np ? (size_t)d.np * bx_plane_elems(b->T, d.ld_in) : 1);
    if (s) *s = t;
    return c.off;
}
// ... checked against the caller's block; the parameters an earlier call re-laid and the caller kept take the place of its own copy
static int carve_checked(const eagcn_batch* b, const eagcn_layer_bufs* w, const LayerDims& d, bool bwd, LayerScratch* sc, const char* who) {
    const size_t need = carve_layer(w->scratch, b, d, bwd, sc);
    const size_t pneed = w->packed ? carve_packed(w->packed, d, &sc->pk) : 0;
    if (need > w->scratch_bytes || pneed > w->packed_bytes) {
        if (need > w->scratch_bytes) set_error("%s: scratch too small (%zu < %zu)", who, w->scratch_bytes, need);
        else set_error("%s: packed buffer too small (%zu < %zu)", who, w->packed_bytes, pneed);
        return EAGCN_ERR_SCRATCH;
    }
    return EAGCN_OK;
}

static int check_layer(const eagcn_batch* b, const eagcn_layer_params* p, const char* who) {
    EAGCN_CHECK_ARG(b && p, "%s: null argument", who);
    EAGCN_CHECK_ARG(p->K >= 1 && p->K <= EAGCN_MAX_VIEWS && p->K == b->K,
                    "%s: layer has %d views, batch index has %d", who, p->K, b->K);
    EAGCN_CHECK_ARG(p->structure == EAGCN_STRUCT_CONCATE || p->structure == EAGCN_STRUCT_WEIGHTED,
                    "%s: unknown structure %d", who, p->structure);
    EAGCN_CHECK_ARG(p->in.nseg >= 1 && p->in.nseg <= EAGCN_MAX_SEGS, "%s: bad input layout", who);
    for (int s = 0; s < p->in.nseg; ++s)
        EAGCN_CHECK_ARG(p->in.width[s] >= 1 && p->in.pad[s] >= p->in.width[s] && (p->in.pad[s] % 4) == 0,
                        "%s: input segment %d: width %d pad %d (pad must be a multiple of 4 >= width)", who, s,
                        p->in.width[s], p->in.pad[s]);
    for (int k = 0; k < p->K; ++k) {
        EAGCN_CHECK_ARG(p->width[k] >= 1, "%s: view %d has width %d", who, k, p->width[k]);
        EAGCN_CHECK_ARG(p->att_w[k] && p->self_r[k] && p->W[k] && p->bias[k] && p->gamma[k] && p->beta[k] &&
                            p->run_mean[k] && p->run_var[k], "%s: view %d has a null parameter", who, k);
        if (p->structure == EAGCN_STRUCT_WEIGHTED)
            EAGCN_CHECK_ARG(p->width[k] == p->width[0], "%s: Weighted_sum needs equal view widths", who);
    }
    if (p->structure == EAGCN_STRUCT_WEIGHTED) EAGCN_CHECK_ARG(p->ave_w, "%s: Weighted_sum needs ave_w", who);
    EAGCN_CHECK_ARG(p->dropout >= 0.0f && p->dropout < 1.0f, "%s: dropout %f out of [0,1)", who, p->dropout);
    // the elementwise BatchNorm passes index (row, 4-column group) pairs with 32 bits
    EAGCN_CHECK_ARG((uint64_t)std::max(b->T, 0) * (uint64_t)view_cols(p).off[p->K] / 4 < (1ull << 32),
                    "%s: %d rows x %d packed columns exceed the 32-bit element index of the BatchNorm passes", who, b->T,
                    view_cols(p).off[p->K]);
    return EAGCN_OK;
}

static ParamPtrs param_ptrs(const eagcn_batch* b, const eagcn_layer_params* p) {
    ParamPtrs pp;
    memset(&pp, 0, sizeof(pp));
    for (int k = 0; k < p->K; ++k) {
        pp.att_w[k] = p->att_w[k]; pp.self_r[k] = p->self_r[k]; pp.W[k] = p->W[k]; pp.bias[k] = p->bias[k];
        pp.gamma[k] = p->gamma[k]; pp.beta[k] = p->beta[k]; pp.run_mean[k] = p->run_mean[k];
        pp.run_var[k] = p->run_var[k]; pp.channels[k] = b->channels[k];
        pp.rel_vec[k] = b->rel_vec[k]; pp.rel_c[k] = b->rel_c[k];
    }
    pp.ave_w = p->structure == EAGCN_STRUCT_WEIGHTED ? p->ave_w : nullptr;
    return pp;
}

static inline int ew_grid(size_t n) { return (int)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 2048)); }

static void launch_pack_params(const ParamPtrs& pp, const LayerDims& d, const ColMapD& in, const Packed& pk, hipStream_t s) {
    ProfScope ps(PROF_PACK, s);
    pack_params_kernel<<<ew_grid(d.wslab), 256, 0, s>>>(pp, d.vc, in, d.ld_in, d.fp, pk.Wcat, pk.WcatT, pk.colp, pk.sig, pk.rsig,
                                                        BxOut{d.np ? pk.Wp : nullptr, d.wpslab, d.np, d.ld_in},
                                                        BxOut{d.np ? pk.WTp : nullptr, d.wtpslab, d.np, d.fp});
}
// algorithmic flops of the flat transform: exact widths, packed rows
static double layer_gemm_work(const eagcn_batch* b, const eagcn_layer_params* p, const LayerDims& d) {
    double fsum = 0.0;
    for (int k = 0; k < p->K; ++k) fsum += p->width[k];
    return 2.0 * (double)b->T * (double)d.fin * fsum;
}

// ---- the three products of a layer: P = X.W^T, dX = dP.W^T, dW = X^T.dP ---------------------------------------------------------
// ONE description of each, for the executors below and for plan_layer (which only asks whether a kernel takes them).
struct LayerOperands {
    const float* x; const uint16_t* xp;               // the input: fp32, and its planes (the caller's, or the scratch block's copy)
    float* P; Packed pk;
    float* dP; uint16_t* dPp; float* dx; float* dWcat;
};
static LayerOperands layer_operands(const eagcn_layer_bufs* w, const LayerScratch& sc, float* dx) {
    return LayerOperands{w->x, w->x_planes ? w->x_planes : sc.xp, w->P, sc.pk, sc.dP, sc.dPp, dx, sc.dWcat};
}
// ... from bf16 operand planes (gemm_bx3.hip): dX and dW share one persistent launch, dW leaves as k-chunk slabs (summed by
// unpack_grads), dP comes from the transposed aggregation as planes and is never written as fp32
struct PlaneProducts { BxProb bp, bx, bw; };
static PlaneProducts layer_plane_products(const eagcn_batch* b, const LayerDims& d, const LayerOperands& o) {
    const size_t xstride = bx_plane_elems(b->T, d.ld_in), pstride = bx_plane_elems(b->T, d.fp);
    const int* T_dev = b->meta + EAGCN_META_T;
    PlaneProducts q;
    memset(&q, 0, sizeof(q));
    q.bp.A = BxPlanes{o.xp, xstride, d.ld_in, b->T}; q.bp.B = BxPlanes{o.pk.WTp, d.wtpslab, d.ld_in, d.fp}; q.bp.C = o.P; q.bp.ldc = d.fp;
    q.bp.M = b->T; q.bp.N = d.fp; q.bp.K = d.ld_in; q.bp.M_dev = T_dev; q.bp.tn = 0; q.bp.splits = 1;
    q.bx.A = BxPlanes{o.dPp, pstride, d.fp, b->T}; q.bx.B = BxPlanes{o.pk.Wp, d.wpslab, d.fp, d.ld_in}; q.bx.C = o.dx; q.bx.ldc = d.ld_in;
    q.bx.M = b->T; q.bx.N = d.ld_in; q.bx.K = d.fp; q.bx.M_dev = T_dev; q.bx.tn = 0; q.bx.splits = 1;
    q.bw.A = BxPlanes{o.xp, xstride, d.ld_in, b->T}; q.bw.B = BxPlanes{o.dPp, pstride, d.fp, b->T};
    q.bw.C = o.dWcat; q.bw.ldc = d.fp; q.bw.M = d.ld_in; q.bw.N = d.fp; q.bw.K = b->T; q.bw.K_dev = T_dev; q.bw.tn = 1;
    q.bw.splits = d.bx_splits; q.bw.slab = d.wslab;
    return q;
}
// ... from fp32 operands: gp = the forward on the pre-transposed weight (NT form: gemm3.hip), gt = the same on Wcat (gemm.hip)
struct Fp32Products { GemmDesc gp, gt, gx, gw; };
static Fp32Products layer_fp32_products(const eagcn_batch* b, const LayerDims& d, const LayerOperands& o, double work) {
    const int* T_dev = b->meta + EAGCN_META_T;
    Fp32Products q{GemmDesc{0, 1, b->T, d.fp, d.ld_in, o.x, d.ld_in, o.pk.WcatT, d.ld_in, o.P, d.fp, 1, 0, work},
                   GemmDesc{0, 0, b->T, d.fp, d.ld_in, o.x, d.ld_in, o.pk.Wcat, d.fp, o.P, d.fp, 1, 0, work},
                   GemmDesc{0, 1, b->T, d.ld_in, d.fp, o.dP, d.fp, o.pk.Wcat, d.fp, o.dx, d.ld_in, 1, 0, work},
                   GemmDesc{1, 0, d.ld_in, d.fp, b->T, o.x, d.ld_in, o.dP, d.fp, o.dWcat, d.fp, d.nsplit, d.wslab, work}};
    q.gp.M_dev = T_dev; q.gt.M_dev = T_dev; q.gx.M_dev = T_dev; q.gw.K_dev = T_dev;
    return q;
}

// ---- the route of a layer call (kernels.h LayerRoute): the switches (each read once).  EAGCN_AGG / EAGCN_LAGG_*: lagg.hip; EAGCN_GEMM_X6: gemm.hip; EAGCN_GEMM3_XK: gemm3.hip
static bool sw_gemm3() { static const bool on = !env_flag("EAGCN_NO_GEMM3", false); return on; }
bool planes_only_enabled() { static const bool on = env_flag("EAGCN_PLANES_ONLY", true); return on; }
// EAGCN_BWD_STORE_DH=1 / 0 forces the elementwise / the re-forming second pass (default: Bn2 above)
static bool bn_bwd_two_pass(bool weighted) {
    static const int force = getenv("EAGCN_BWD_STORE_DH") ? (env_flag("EAGCN_BWD_STORE_DH", false) ? 1 : 0) : -1;
    return force < 0 ? weighted : force == 0;
}
// Which layers run their products on the wave-autonomous balanced kernel (gemm3.hip): the hidden layers.  The first
// layer (24 atom features) is a different animal: its forward product has two k-steps per tile and its weight gradient
// seven 64x64 tiles with thousands of k-steps each -- a balanced cut would make every wave hand a partial tile to a
// single owner per tile (measured: 0.2 ms instead of 0.02 ms) -- it stays on the workgroup-tiled kernels (gemm.hip).
static bool gemm3_layer(int ld_in) {
    return sw_gemm3() && ld_in >= 128 && gemm_mode() != 2;       // (the bf16 mode runs on the LDS-tiled kernels of gemm.hip)
}
// EAGCN_FIRST_LAYER_FUSED=0 in the environment / eagcn_set_first_layer_fused(0): the first layer's weight gradient stays a launch of its own
static int g_first_layer_fused = env_flag("EAGCN_FIRST_LAYER_FUSED", true) ? 1 : 0;
static long g_first_layer_fused_taken = 0;
static int32_t g_first_layer_fused_last[3] = {0, 0, 0};      // of the last such call: slabs (= the grid's y extent), slabs in the dP area, uncapped y extent
static bool first_layer_fused_enabled() { return g_first_layer_fused != 0; }
// EAGCN_HIDDEN_BN_SUMS=0 in the environment / eagcn_set_hidden_bn_sums(0): the hidden layers' BatchNorm backward keeps its reduction pass
static int g_hidden_bn_sums = env_flag("EAGCN_HIDDEN_BN_SUMS", true) ? 1 : 0;
static long g_hidden_bn_taken = 0;

static LayerRoute plan_layer(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w, const LayerDims& d,
                             const PlanAsk& ask) {
    LayerRoute r;
    const bool wt = p->structure == EAGCN_STRUCT_WEIGHTED;
    bool general = false;                             // (code books: the edge reduction reads a view's whole histogram per channel)
    for (int k = 0; k < p->K; ++k) general = general || b->rel_vec[k] != nullptr;
    r.edge_atomic = !general;
    r.store_dh = !bn_bwd_two_pass(wt);
    if (b->T <= 0) return r;                          // no packed row: no product, no aggregation, a row-less reduction
    r.fwd_agg = fwd_agg_lagg(b, d.vc) ? AGG_LAGG : AGG_DENSE;
    float* const some_dx = reinterpret_cast<float*>(static_cast<uintptr_t>(4096));       // (the products' checks want an address)
    // (addresses enter through their alignment alone and every piece of either carving is 256-byte aligned: the backward's stands for both)
    LayerScratch sc;
    carve_layer(w->scratch, b, d, true, &sc);
    if (w->packed) carve_packed(w->packed, d, &sc.pk);
    const LayerOperands o = layer_operands(w, sc, ask.has_dx ? some_dx : nullptr);
    const PlaneProducts bq = layer_plane_products(b, d, o);
    const Fp32Products gq = layer_fp32_products(b, d, o, 0.0);

    // forward product: planes (x planes from the layer below, or split here), else the balanced kernel on the pre-transposed
    // weight; operands that are not 16-byte aligned fall back to the workgroup-tiled kernel
    r.fwd_split_x = d.np && !w->x_planes;
    if (d.np && bx3_ok(bq.bp)) r.fwd_prod = FWD_PLANES;
    else if (!w->x) r.fwd_prod = FWD_REFUSED;
    else r.fwd_prod = (gemm3_layer(d.ld_in) && gemm3_ok(gq.gp)) ? FWD_BALANCED : FWD_TILED;

    // The LDS-staged kernel runs the transposed aggregation + edge gradients (which must then leave through the shared
    // accumulators).  It absorbs the second pass of the BatchNorm backward: of a Concate layer from the stored dH, of a Weighted_sum
    // layer from the upstream gradient; input-only: no edge gradients to route, and the staging absorbs whatever the structure
    const bool fuse_w = bn_bwd_two_pass(wt) && wt && lagg_wfuse();
    const bool absorbs = !bn_bwd_two_pass(wt) || (wt && lagg_wfuse());
    const bool lagg = ask.input_only ? lagg_use(b, 1, true) : (r.edge_atomic && lagg_use(b, 1, absorbs));
    r.bwd_agg = lagg ? AGG_LAGG : AGG_DENSE;
    if (ask.input_only && !p->training) {
        // eval-mode BatchNorm backward of the input-only form: dY' = sc dH (the running statistics are constants: c1 = c2 = 0), no
        // reduction and no finalize; off the LDS-staged kernel the reduction kernel's second pass forms dY' from zero means
        r.bn2 = !lagg ? BN2_REDUCE_APPLY : wt ? BN2_STAGED_FROM_UPSTREAM : BN2_STAGED_ROWMASK;
        r.rows_first = lagg && ask.mol_grad;
    } else if (lagg && fuse_w) {
        // lagg.hip wants a per-molecule read-out gradient as ROWS ([T][ldo], K times narrower than dH) -- written first, so that the
        // reduction reads them with 16-byte loads as well instead of gathering dg[molecule] element by element
        r.bn2 = BN2_STAGED_FROM_UPSTREAM;
        r.rows_first = ask.mol_grad;
    } else if (bn_bwd_two_pass(wt)) r.bn2 = BN2_REDUCE_APPLY;
    else r.bn2 = lagg ? BN2_STAGED_FROM_DH : BN2_ELEMENTWISE;
    if (ask.top_sums && r.bn2 == BN2_STAGED_FROM_DH && ask.mol_grad && !wt) {
        // the sums are there already; the staging gathers the read-out gradient per molecule, or reads it as rows (as wide as dH,
        // never dH itself) written behind the finalize
        r.bn2 = BN2_STAGED_FROM_READOUT;
        r.rows_late = !ask.top_gather;
        r.store_dh = false;
    }

    // dH and its sums were formed by the dX product of the layer above: the one route whose pass that replaces (dH stored by the
    // pass, the second pass in lagg.hip's staging -- which then stages from the upstream buffer; a Concate layer in training mode,
    // never more slabs than the pass writes)
    r.dh_given = ask.dh_given && g_hidden_bn_sums && r.bn2 == BN2_STAGED_FROM_DH && r.store_dh && !wt && p->training && !ask.mol_grad &&
                 !ask.input_only && hidden_bn_slabs(b->T) <= d.gxb;
    const bool planes = d.np && bx3_ok(bq.bw) && (!ask.has_dx || bx3_ok(bq.bx));
    r.bwd_split_x = planes && !w->x_planes && !ask.input_only;
    if (ask.input_only) r.bwd_prod = planes ? BWD_PLANES_DX : BWD_TILED_DX;
    else if (!planes && !w->x) r.bwd_prod = BWD_REFUSED;
    if (r.bwd_prod != BWD_NONE) return r;
    r.edge = (lagg && r.edge_atomic) ? EDGE_WITH_LAGG : EDGE_COLAUNCH;
    if (planes) {
        r.bwd_prod = ask.has_dx ? BWD_PLANES_PAIR : BWD_PLANES_DW;
        r.bx_wide = (ask.has_dx ? bx3_pick_wide(bq.bx, &bq.bw, b->t_hint) : bx3_pick_wide(bq.bw, nullptr, b->t_hint)) != 0;
        r.carries_below = ask.below && ask.has_dx && !r.bx_wide;
    } else if (ask.has_dx && gemm3_layer(d.ld_in) && gemm3_ok(gq.gw) && gemm3_ok(gq.gx))
        r.bwd_prod = gemm3_xk_enabled() ? BWD_G3_XK : BWD_G3_SCATTER;
    else r.bwd_prod = ask.has_dx ? BWD_TILED_PAIR : BWD_TILED_SEPARATE;
    // nothing but the edge reduction is left for this layer (no dW slabs to sum): the next layer's first backward kernel does it
    r.defer_drain = ask.has_drain_out && r.edge_atomic && r.bwd_prod == BWD_G3_SCATTER;
    // the first layer's weight gradient inside the aggregation launch: the plain transposed kernel (dY' or dH staged, not the
    // upstream-gradient forms), exact fp32 products in both places, at most 32 input columns (one pair of 16-row MFMA tiles)
    const bool plain_staging = r.bn2 != BN2_STAGED_FROM_UPSTREAM && r.bn2 != BN2_STAGED_ROWMASK && r.bn2 != BN2_STAGED_FROM_READOUT;
    if (first_layer_fused_enabled() && r.bwd_prod == BWD_TILED_SEPARATE && r.edge == EDGE_WITH_LAGG && r.bwd_agg == AGG_LAGG &&
        plain_staging && d.ld_in <= 32 && gemm_mode() != 1 && gemm_mode() != 2 && w->x) {
        const long cap_w = std::max(std::max(d.nsplit, G3_XSEG), d.np ? d.bx_splits : 1);       // (carve_layer: slabs of the dWcat area)
        const long cap_p = (long)(((size_t)std::max(b->T, 1) * d.fp) / d.wslab);               // ... and of the dP area
        r.dw_fused = true;
        r.dw_ny = (int)std::max<long>(1, std::min<long>(lagg_bwd_grid_y(b, d.vc), std::max(cap_w, cap_p)));
        r.dw_in_dp = r.dw_ny > cap_w;
    }
    return r;
}
LayerRoute plan_layer(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w, const PlanAsk& ask) {
    return plan_layer(b, p, w, layer_dims(b, p), ask);
}
bool top_gather_ok(const eagcn_layer_params* p, const float* dge, int F) {
    bool ok = dge && (reinterpret_cast<uintptr_t>(dge) & 15) == 0 && (F & 3) == 0;
    for (int k = 0; k < p->K; ++k) ok = ok && (p->width[k] & 3) == 0;
    return ok;
}

static int apply_launch(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w, const LayerDims& d,
                        const float* colp, hipStream_t s, bool planes_only = false) {
    ProfScope psbn(PROF_BN, s);
    ApplyArgs aa;
    aa.bt = *b; aa.vc = d.vc; aa.structure = p->structure; aa.fp = d.fp; aa.Y = w->Y; aa.ldy = d.fp;
    aa.bn = w->bn; aa.colp = colp; aa.out = w->xout; aa.ldo = d.ldo; aa.pad_row = w->pad_row;
    const DropArgs dr = drop_args(p->dropout, p->training != 0, p->seed, p->seed_dev);
    aa.do_drop = dr.on; aa.thr = dr.thr; aa.inv_keep = dr.inv_keep; aa.seed = dr.seed; aa.seed_dev = dr.seed_dev;
    aa.planes = BxOut{gemm_planes() ? w->xout_planes : nullptr, bx_plane_elems(b->T, d.ldo), gemm_planes(), b->T};
    if (planes_only && aa.planes.p) aa.out = nullptr;        // (the only reader is the layer above, through the planes)
    aa.tile_map = aa.planes.p ? 1 : 0;
    const size_t nthr = aa.tile_map ? (size_t)cdiv(std::max(b->T, 1), 8) * cdiv(d.ldo, 32) * 64 : (size_t)std::max(b->T, 1) * d.ldo / 4;
    bn_apply_kernel<<<ew_grid(nthr), 256, 0, s>>>(aa);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

}  // namespace eagcn

using namespace eagcn;

extern "C" int eagcn_pad16(int w) { return pad16(w); }
extern "C" int eagcn_layer_fp(const eagcn_layer_params* p) { return view_cols(p).off[p->K]; }
extern "C" int eagcn_layer_out_ld(const eagcn_layer_params* p) {
    return p->structure == EAGCN_STRUCT_CONCATE ? eagcn_layer_fp(p) : pad16(p->width[0]);
}
extern "C" size_t eagcn_layer_packed_bytes(const eagcn_batch* b, const eagcn_layer_params* p) {
    return carve_packed(nullptr, layer_dims(b, p), nullptr);
}
extern "C" size_t eagcn_layer_fwd_scratch_bytes(const eagcn_batch* b, const eagcn_layer_params* p) {
    return carve_layer(nullptr, b, layer_dims(b, p), false, nullptr);
}
extern "C" size_t eagcn_layer_bwd_scratch_bytes(const eagcn_batch* b, const eagcn_layer_params* p) {
    return carve_layer(nullptr, b, layer_dims(b, p), true, nullptr);
}

// both directions of layer p would take their input x from its bf16 plane images alone: the route of a hypothetical call that brings
// them and nothing else (eagcn_layer_route out[13]; the model engine plans its real calls: head.hip plan_model)
static bool layer_reads_planes_only(const eagcn_batch* b, const eagcn_layer_params* p) {
    // (bx3_ok looks at alignment, strides and extents: the addresses stand for the 256-byte aligned pieces the executors carve)
    void* const some = reinterpret_cast<void*>(static_cast<uintptr_t>(4096));
    eagcn_layer_bufs w{};
    w.x_planes = static_cast<const uint16_t*>(some); w.P = static_cast<float*>(some); w.scratch = some;
    PlanAsk ask;
    ask.has_dx = true;
    const LayerRoute r = plan_layer(b, p, &w, ask);             // (no packed row: no product at all)
    return planes_only_enabled() && r.fwd_prod == FWD_PLANES && r.bwd_prod == BWD_PLANES_PAIR;
}

extern "C" int eagcn_layer_route(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w, int has_dx,
                                 int mol_grad, int input_only, int has_drain_out, int32_t out[16]) {
    int rc = check_layer(b, p, "eagcn_layer_route");
    if (rc) return rc;
    EAGCN_CHECK_ARG(w && out, "eagcn_layer_route: null argument");
    rc = check_reserved_null(w->aux_stream, "eagcn_layer_route", "eagcn_layer_bufs.aux_stream");
    if (rc) return rc;
    PlanAsk ask;
    ask.has_dx = has_dx != 0; ask.mol_grad = mol_grad != 0; ask.input_only = input_only != 0; ask.has_drain_out = has_drain_out != 0;
    const LayerRoute r = plan_layer(b, p, w, ask);
    const int32_t v[16] = {(int32_t)r.fwd_prod, r.fwd_split_x, (int32_t)r.fwd_agg, (int32_t)r.bwd_agg, (int32_t)r.bn2, r.rows_first, r.rows_late, r.store_dh, (int32_t)r.edge,
                           r.edge_atomic, (int32_t)r.bwd_prod, r.bwd_split_x, r.defer_drain,
                           layer_reads_planes_only(b, p), 0, 0};
    memcpy(out, v, sizeof(v));
    return EAGCN_OK;
}

// a layer-level call starts with the hand-off flags of its scratch block cleared (the model engine clears once per model call)
static int clear_handoff_flags(const eagcn_layer_bufs* w, void* stream) {
    if (!(w && w->scratch && w->scratch_bytes >= gemm3_workspace_bytes())) return EAGCN_OK;
    return gemm3_clear_flags(w->scratch, w->scratch_bytes, (hipStream_t)stream);
}
// the public entry points plan for themselves, behind the checks plan_layer relies on
static int plan_checked(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w, const PlanAsk& ask, const char* who,
                        LayerRoute* r) {
    const int rc = check_layer(b, p, who);
    if (rc) return rc;
    EAGCN_CHECK_ARG(w, "%s: null buffer", who);
    *r = plan_layer(b, p, w, ask);
    return EAGCN_OK;
}
extern "C" int eagcn_layer_forward(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w,
                                   void* stream) {
    EAGCN_CHECK_GEMM3("eagcn_layer_forward");
    LayerRoute r;
    int rc = check_reserved_null(w ? w->aux_stream : nullptr, "eagcn_layer_forward", "eagcn_layer_bufs.aux_stream");
    if (!rc) rc = plan_checked(b, p, w, PlanAsk{}, "eagcn_layer_forward", &r);
    if (!rc) rc = clear_handoff_flags(w, stream);
    return rc ? rc : layer_forward_impl(b, p, w, stream, r, false);
}

// parameters of up to four layers re-laid into their `packed` blocks by ONE launch (model engine)
int eagcn::pack_params_all(const eagcn_batch* b, const eagcn_layer_params* const* ps, void* const* packed,
                           const size_t* packed_bytes, int n, void* stream, const ZeroJob* zj, const HandOff* ho) {
    hipStream_t s = (hipStream_t)stream;
    EAGCN_CHECK_ARG(n >= 1 && n <= 4, "pack_params_all: 1..4 layers");
    PackJob jobs[4];
    size_t wmax = 0;
    for (int l = 0; l < 4; ++l) {
        const int ll = l < n ? l : n - 1;
        int rc = check_layer(b, ps[ll], "eagcn_model_forward");
        if (rc) return rc;
        const LayerDims d = layer_dims(b, ps[ll]);
        Packed pk;
        const size_t pneed = carve_packed(packed[ll], d, &pk);
        if (pneed > packed_bytes[ll]) {
            set_error("pack_params_all: packed buffer of layer %d too small (%zu < %zu)", ll, packed_bytes[ll], pneed);
            return EAGCN_ERR_SCRATCH;
        }
        jobs[l].pp = param_ptrs(b, ps[ll]); jobs[l].vc = d.vc; jobs[l].in = make_colmap(&ps[ll]->in);
        jobs[l].ld_in = d.ld_in; jobs[l].fp = d.fp;
        jobs[l].Wcat = pk.Wcat; jobs[l].WcatT = pk.WcatT; jobs[l].colp = pk.colp; jobs[l].sig = pk.sig; jobs[l].rsig = pk.rsig;
        jobs[l].wp = BxOut{d.np ? pk.Wp : nullptr, d.wpslab, d.np, d.ld_in};
        jobs[l].wtp = BxOut{d.np ? pk.WTp : nullptr, d.wtpslab, d.np, d.fp};
        if (l < n) wmax = std::max(wmax, d.wslab);
    }
    PackJobs pj{jobs[0], jobs[1], jobs[2], jobs[3]};
    ProfScope ps_(PROF_PACK, s);
    const ZeroJob none{nullptr, 0, nullptr, 0};
    const HandOff noho{nullptr, nullptr, nullptr, 0};
    pack_params_multi_kernel<<<dim3(ew_grid(wmax), n), 256, 0, s>>>(pj, zj ? *zj : none, ho ? *ho : noho);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

// kernels templated by the number of partial slabs a thread sums at a time: few slabs -> 16 columns per workgroup, many -> 4
#define EAGCN_BY_SLABS(n, kernel, ...) do { if ((n) > 64) kernel<64><<<cdiv(d.fp, 4), 256, 0, s>>>(__VA_ARGS__); \
                                            else kernel<16><<<cdiv(d.fp, 16), 256, 0, s>>>(__VA_ARGS__); } while (0)

int eagcn::layer_forward_impl(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w,
                              void* stream, const LayerRoute& r, bool prepacked, bool skip_apply, bool planes_only) {
    hipStream_t s = (hipStream_t)stream;
    int rc = check_layer(b, p, "eagcn_layer_forward");
    if (rc) return rc;
    EAGCN_CHECK_ARG(w && w->bn && w->xout && w->pad_row && w->scratch, "eagcn_layer_forward: null buffer");
    // (w->x may be null when the layer below wrote plane images only: every fp32 fallback below then refuses)
    EAGCN_CHECK_ARG(b->T == 0 || ((w->x || w->x_planes) && w->P && w->Y && w->rscale), "eagcn_layer_forward: null activation buffer");
    EAGCN_CHECK_ARG(!planes_only || (w->xout_planes && gemm_planes()), "eagcn_layer_forward: planes-only output without plane images");
    const LayerDims d = layer_dims(b, p);
    LayerScratch sc;
    rc = carve_checked(b, w, d, false, &sc, "eagcn_layer_forward");
    if (rc) return rc;
    const ParamPtrs pp = param_ptrs(b, p);
    EAGCN_CHECK_ARG(!prepacked || w->packed, "eagcn_layer_forward: prepacked parameters need the packed block");
    if (!prepacked) launch_pack_params(pp, d, make_colmap(&p->in), sc.pk, s);
    EAGCN_LAUNCH_CHECK();
    int nslab = 0, tiles_per_wg = agg_ksplit(b) ? 1 : 4;
    if (b->T > 0) {
        const double gemm_work = layer_gemm_work(b, p, d);
        const LayerOperands o = layer_operands(w, sc, nullptr);
        const Fp32Products gq = layer_fp32_products(b, d, o, gemm_work);
        if (r.fwd_prod == FWD_REFUSED) {
            set_error("eagcn_layer_forward: the input exists as plane images only and the plane product does not apply");
            return EAGCN_ERR_ARG;
        }
        if (r.fwd_split_x) {
            rc = launch_bx3_split(w->x, b->T, b->meta + EAGCN_META_T, d.ld_in, sc.xp, bx_plane_elems(b->T, d.ld_in), b->T, d.np, s);
            if (rc) return rc;
        }
        switch (r.fwd_prod) {
        case FWD_PLANES: {
            const BxProb bp = layer_plane_products(b, d, o).bp;
            rc = launch_bx3(bp, nullptr, d.np, s, gemm_work, PROF_GEMM, bx3_pick_wide(bp, nullptr, b->t_hint));
            break;
        }
        case FWD_BALANCED: rc = launch_gemm3(gq.gp, nullptr, sc.gws, gemm3_workspace_bytes(), s); break;
        default: rc = launch_gemm(gq.gt, s); break;
        }
        if (rc) return rc;
        AggArgs a;
        a.bt = *b; a.vc = d.vc; a.src = w->P; a.lds = d.fp; a.dst = w->Y; a.ldd = d.fp;
        a.sig = sc.pk.sig; a.rsig = sc.pk.rsig; a.rscale = w->rscale; a.stats = sc.stats; a.nchunk = 1;
        if (r.fwd_agg == AGG_LAGG) {                  // one slab per row block
            rc = launch_lagg_fwd(a, s);
            nslab = lagg_slabs(b);
            tiles_per_wg = -1;
        } else {
            rc = launch_agg(a, false, s);
            nslab = d.gx;
        }
        if (rc) return rc;
    }
    const double M = (double)b->B * (double)b->N;
    {
        ProfScope psbn(PROF_BN, s);
        const bool sync = w->stats_hook && p->training;
        if (sync) {
            // sync-BatchNorm: this rank's sums -> one vector, summed across the ranks by the caller's hook, finalize from that
            EAGCN_BY_SLABS(nslab, bn_stats_sum_kernel, sc.stats, nslab, d.fp, M, sc.gsum, b->meta, 1, tiles_per_wg, 0, b->B);
            EAGCN_LAUNCH_CHECK();
            if (w->stats_hook(sc.gsum, 2 * d.fp + 1, stream, w->stats_user)) {
                set_error("eagcn_layer_forward: the sync-BatchNorm all-reduce hook failed");
                return EAGCN_ERR_HIP;
            }
            nslab = 1;
        }
        EAGCN_BY_SLABS(nslab, bn_finalize_kernel, sync ? sc.gsum : sc.stats, nslab, d.fp, M, p->training, p->bn_eps, p->bn_momentum, sc.pk.colp,
                       pp, d.vc, w->bn, b->meta, sync ? 0 : tiles_per_wg, b->B, sync ? sc.gsum + 2 * d.fp : nullptr);
        EAGCN_LAUNCH_CHECK();
    }
    if (skip_apply) return EAGCN_OK;
    return apply_launch(b, p, w, d, sc.pk.colp, s, planes_only);
}

// EAGCN_TOP_BN_SUMS=0 in the environment / eagcn_set_top_bn_sums(0): the top layer's BatchNorm backward keeps its reduction pass
static int g_top_bn_sums = !env_flag("EAGCN_TOP_BN_SUMS", true) ? 0 : env_int("EAGCN_TOP_BN_SUMS", 1) == 2 ? 2 : 1;
bool eagcn::top_bn_sums_enabled() { return g_top_bn_sums != 0; }
bool eagcn::top_bn_gather_enabled() { return g_top_bn_sums == 1; }
extern "C" int eagcn_set_top_bn_sums(int on) {
    const int old = g_top_bn_sums;
    g_top_bn_sums = on == 2 ? 2 : on ? 1 : 0;
    return old;
}
/* layer backward calls (captured ones count when they are captured) that took dH and its sums from the layer above, since the last reset */
extern "C" long eagcn_hidden_bn_sums_taken(int reset) {
    const long n = g_hidden_bn_taken;
    if (reset) g_hidden_bn_taken = 0;
    return n;
}
extern "C" int eagcn_set_hidden_bn_sums(int on) {
    const int old = g_hidden_bn_sums;
    g_hidden_bn_sums = on ? 1 : 0;
    return old;
}
/* layer backward calls (captured ones count when they are captured) whose weight gradient left the transposed aggregation's epilogue, since the last reset */
extern "C" long eagcn_first_layer_fused_taken(int reset) {
    const long n = g_first_layer_fused_taken;
    if (reset) g_first_layer_fused_taken = 0;
    return n;
}
extern "C" void eagcn_first_layer_fused_last(int32_t out[3]) { memcpy(out, g_first_layer_fused_last, sizeof(g_first_layer_fused_last)); }
extern "C" int eagcn_set_first_layer_fused(int on) {
    const int old = g_first_layer_fused;
    g_first_layer_fused = on ? 1 : 0;
    return old;
}
int eagcn::layer_apply_impl(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w, void* stream) {
    EAGCN_CHECK_ARG(b && p && w && w->bn && w->xout && w->pad_row && w->packed, "layer_apply: null buffer");
    const LayerDims d = layer_dims(b, p);
    Packed pk;
    EAGCN_CHECK_ARG(carve_packed(w->packed, d, &pk) <= w->packed_bytes, "layer_apply: packed buffer too small");
    return apply_launch(b, p, w, d, pk.colp, (hipStream_t)stream);
}

// the two passes of bn_bwd_reduce_kernel (apply = false: sums, apply = true: dY') in their compile-time variants
static void launch_bn_bwd_pass(bool apply, bool wt, bool dg, bool dr, dim3 grid, const BwdArgs& ba, hipStream_t s) {
#define EAGCN_BWD(W, G, D) do { if (apply) bn_bwd_reduce_kernel<W, G, D, true><<<grid, 256, 0, s>>>(ba); \
                                else bn_bwd_reduce_kernel<W, G, D, false><<<grid, 256, 0, s>>>(ba); } while (0)
    if (wt) { if (dg) { if (dr) EAGCN_BWD(true, true, true); else EAGCN_BWD(true, true, false); }
              else    { if (dr) EAGCN_BWD(true, false, true); else EAGCN_BWD(true, false, false); } }
    else    { if (dg) { if (dr) EAGCN_BWD(false, true, true); else EAGCN_BWD(false, true, false); }
              else    { if (dr) EAGCN_BWD(false, false, true); else EAGCN_BWD(false, false, false); } }
#undef EAGCN_BWD
}

extern "C" int eagcn_layer_backward(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w,
                                    const float* dxout, const float* dpad_row, float* dx,
                                    const eagcn_layer_grads* g, void* stream) {
    EAGCN_CHECK_GEMM3("eagcn_layer_backward");
    LayerRoute r;
    int rc = check_reserved_null(w ? w->aux_stream : nullptr, "eagcn_layer_backward", "eagcn_layer_bufs.aux_stream");
    PlanAsk ask;
    ask.has_dx = dx != nullptr;
    if (!rc) rc = plan_checked(b, p, w, ask, "eagcn_layer_backward", &r);
    if (!rc) rc = clear_handoff_flags(w, stream);
    return rc ? rc : layer_backward_impl(b, p, w, dxout, dpad_row, dx, g, stream, r);
}

namespace {
// one backward call: its arguments, carving and route, and what the products leave for unpack_grads
struct LayerBwd {
    const eagcn_batch* b; const eagcn_layer_params* p; const eagcn_layer_bufs* w;
    const float* dxout; const float* dpad_row; LayerBwdOpts o;
    LayerDims d; LayerScratch sc; LayerRoute r; ParamPtrs pp; GradPtrs gp; ColMapD in;
    hipStream_t s;
    bool wt, dg; DropArgs drop; double gemm_work;
    int nsplit = 0, xk_G = 0;
    bool bx_slabs = false;       // dWcat holds the k-chunk slabs of the plane GEMM (all of them written)
    int bx_per = 0;              // > 0: that product shared its launch with dX (workgroups per XCD: bx3.h bx3_used_splits; the chunk policy
                                 // counts the tiles of the kernel that wrote the slabs: r.bx_wide)
};
}  // namespace

// where the parameter gradients go; input-only: a training-mode BatchNorm finalize still writes d gamma / d beta / d bias /
// d ave.weight on its way -- into the weight-gradient slab area, which that form does not use; nothing reads them
static GradPtrs grad_ptrs(const eagcn_layer_params* p, const eagcn_layer_grads* g, const LayerDims& d, float* discard) {
    GradPtrs gp;
    memset(&gp, 0, sizeof(gp));
    for (int k = 0; k < p->K; ++k) {
        if (discard) {
            gp.dgamma[k] = discard + d.vc.off[k];
            gp.dbeta[k] = discard + d.fp + d.vc.off[k];
            gp.dbias[k] = discard + 2 * d.fp + d.vc.off[k];
        } else {
            gp.dW[k] = g->dW[k]; gp.dbias[k] = g->dbias[k]; gp.dgamma[k] = g->dgamma[k]; gp.dbeta[k] = g->dbeta[k];
            gp.datt_w[k] = g->datt_w[k]; gp.dself_r[k] = g->dself_r[k];
        }
    }
    gp.dave_w = p->structure != EAGCN_STRUCT_WEIGHTED ? nullptr : discard ? discard + 3 * d.fp : g->dave_w;
    return gp;
}

// BatchNorm backward up to where the route leaves dY' (or what lagg.hip's staging forms it from) in sc.dY
static int bwd_batchnorm(LayerBwd& c) {
    const eagcn_batch* b = c.b; const eagcn_layer_params* p = c.p; const eagcn_layer_bufs* w = c.w;
    const LayerDims& d = c.d; const LayerScratch& sc = c.sc; const LayerRoute& r = c.r; hipStream_t s = c.s;
    BwdArgs ba;
    ba.meta = b->meta; ba.Tcap = b->T; ba.row_mol = b->row_mol; ba.row_m = b->row_m;
    ba.vc = d.vc; ba.structure = p->structure; ba.fp = d.fp;
    ba.nvirt = (c.dpad_row && c.wt) ? 1 : 0;
    ba.dxout = c.dxout; ba.ldo = d.ldo; ba.dpad = c.dpad_row; ba.dpad_views = c.o.dpad_views ? 1 : 0;
    if (c.o.rg) ba.rg = *c.o.rg; else memset(&ba.rg, 0, sizeof(ba.rg)); ba.Y = w->Y; ba.ldy = d.fp; ba.bn = w->bn;
    ba.colp = sc.pk.colp; ba.dH = sc.dY; ba.slab = sc.slab; ba.slab_da = sc.slab_da;
    ba.do_drop = c.drop.on; ba.thr = c.drop.thr; ba.inv_keep = c.drop.inv_keep; ba.seed = c.drop.seed; ba.seed_dev = c.drop.seed_dev;
    const ZeroJob* za = c.o.zero_after;
    ba.zero = za ? za->d : nullptr;
    ba.nzero = za ? za->nd : 0;
    if (c.o.drain_in && c.o.drain_in->eacc) ba.drain = *c.o.drain_in; else memset(&ba.drain, 0, sizeof(ba.drain));
    ba.cc = sc.cc; ba.store_dh = r.store_dh ? 1 : 0;
    const int ny = cdiv(d.fp, 1024);
    const dim3 grid2(std::max(1, std::min(b->T, d.gxb)), ny);          // second pass: the stored rows alone
    const bool dr = ba.do_drop != 0;
    int rc;
    if (c.o.input_only && !p->training) {
        if (r.rows_first) { rc = launch_readout_bwd_rows(b, ba.rg, d.ldo, sc.dY, s); if (rc) return rc; }
        if (r.bn2 == BN2_REDUCE_APPLY) {
            rc = zero_fill(sc.cc, (size_t)2 * d.fp * sizeof(float), s);
            if (rc) return rc;
            launch_bn_bwd_pass(true, c.wt, c.dg, false, grid2, ba, s);
            EAGCN_LAUNCH_CHECK();
        }
        // (the head's backward sums are left zero for a later backward call: the finalize that clears them on the way did not run)
        return (za && za->nd) ? zero_fill(za->d, (size_t)za->nd * sizeof(double), s) : EAGCN_OK;
    }
    ProfScope ps(PROF_BN, s);
    const double M = (double)b->B * (double)b->N;
    if (r.bn2 == BN2_STAGED_FROM_READOUT) {
        // sum dH and sum dH xhat were taken over the molecules where dg was formed (head2.hip HeadTopSums): no pass over the rows;
        // the finalize adds up those slabs (all of them, whatever the row count) and clears the head's sums on the way as ever
        const int ns = c.o.top_nslab;
        EAGCN_BY_SLABS(ns, bn_bwd_finalize_kernel, c.o.top_sums, sc.slab_da, ns, d.fp, M, p->training, w->bn, d.vc, c.gp, sc.cc, b->meta, 0,
                       b->B, ny, ns, nullptr, ba.zero, ba.nzero, 1);
        EAGCN_LAUNCH_CHECK();
        return r.rows_late ? launch_readout_bwd_rows(b, ba.rg, d.ldo, sc.dY, s) : EAGCN_OK;
    }
    if (r.dh_given) {
        ++g_hidden_bn_taken;
        // the dX units of the layer above left dH in the upstream buffer and one slab of sums per BX_EPI_ROWS rows: no pass over the rows
        const int ns = c.o.dh_nslab;
        EAGCN_BY_SLABS(ns, bn_bwd_finalize_kernel, c.o.dh_sums, sc.slab_da, ns, d.fp, M, p->training, w->bn, d.vc, c.gp, sc.cc, b->meta, 0,
                       b->B, ny, ns, nullptr, ba.zero, ba.nzero, 2);
        EAGCN_LAUNCH_CHECK();
        return EAGCN_OK;
    }
    const int gxb = std::max(1, std::min(b->T + ba.nvirt, d.gxb));
    bool dg = c.dg;
    if (r.rows_first) {
        rc = launch_readout_bwd_rows(b, ba.rg, d.ldo, sc.dY, s);
        if (rc) return rc;
        ba.dxout = sc.dY;
        dg = false;
    }
    launch_bn_bwd_pass(false, c.wt, dg, dr, dim3(gxb, ny), ba, s);
    EAGCN_LAUNCH_CHECK();
    const double* gsum = nullptr;
    if (w->stats_hook && p->training) {
        // sync-BatchNorm: sum dH, sum dH xhat and the row count of this rank -> summed across the ranks by the caller's hook
        EAGCN_BY_SLABS(gxb, bn_stats_sum_kernel, sc.slab, gxb, d.fp, M, sc.gsum, b->meta, 2, 0, ba.nvirt, b->B);
        EAGCN_LAUNCH_CHECK();
        if (w->stats_hook(sc.gsum, 2 * d.fp + 1, (void*)s, w->stats_user)) {
            set_error("eagcn_layer_backward: the sync-BatchNorm all-reduce hook failed");
            return EAGCN_ERR_HIP;
        }
        gsum = sc.gsum;
    }
    EAGCN_BY_SLABS(gxb, bn_bwd_finalize_kernel, sc.slab, sc.slab_da, gxb, d.fp, M, p->training, w->bn, d.vc, c.gp, sc.cc, b->meta, ba.nvirt,
                   b->B, ny, gxb, gsum, ba.zero, ba.nzero, 0);
    EAGCN_LAUNCH_CHECK();
    if (r.rows_late) { rc = launch_readout_bwd_rows(b, ba.rg, d.ldo, sc.dY, s); if (rc) return rc; }
    if (r.bn2 == BN2_REDUCE_APPLY) launch_bn_bwd_pass(true, c.wt, c.dg, dr, grid2, ba, s);       // dH formed again, dY' written
    else if (r.bn2 == BN2_ELEMENTWISE)
        bn_bwd_apply_kernel<<<ew_grid((size_t)b->T * d.fp / 4), 256, 0, s>>>(*b, d.fp, w->Y, d.fp, w->bn, sc.cc, sc.dY);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

// transposed aggregation dP (fp32, or bf16 planes for the plane GEMMs) and, in the full form, the edge gradients
static int bwd_aggregate(LayerBwd& c) {
    const eagcn_batch* b = c.b; const eagcn_layer_bufs* w = c.w; const LayerDims& d = c.d; const LayerScratch& sc = c.sc;
    const LayerRoute& r = c.r; hipStream_t s = c.s;
    AggArgs a;
    a.bt = *b; a.vc = d.vc; a.src = sc.dY; a.lds = d.fp; a.dst = sc.dP; a.ldd = d.fp;
    a.sig = sc.pk.sig; a.rsig = sc.pk.rsig; a.rscale = w->rscale; a.stats = nullptr; a.nchunk = 1;
    if (r.bwd_planes()) a.planes = BxOut{sc.dPp, bx_plane_elems(b->T, d.fp), d.np, b->T};
    if (r.bn2_staged()) {        // lagg.hip forms dY' while it stages its rows (eval mode: zero means, no table of them)
        a.bn_tab = w->bn; a.bn_cc = (c.o.input_only && !c.p->training) ? nullptr : sc.cc; a.bn_fp = d.fp;
    }
    if (r.dh_given) { a.src = c.dxout; a.lds = d.ldo; }          // dH as the layer above's dX product left it (Concate: ldo == fp)
    if (r.dw_fused) {            // no dP: the weight gradient leaves the epilogue as one slab per workgroup row
        ++g_first_layer_fused_taken;
        g_first_layer_fused_last[0] = r.dw_ny; g_first_layer_fused_last[1] = r.dw_in_dp ? 1 : 0; g_first_layer_fused_last[2] = lagg_bwd_grid_y(b, d.vc);
        a.dst = nullptr; a.fx = w->x; a.fx_ld = d.ld_in; a.dw = r.dw_in_dp ? sc.dP : sc.dWcat; a.dw_slab = d.wslab; a.dw_ny = r.dw_ny;
    }
    if (r.bn2 == BN2_STAGED_FROM_UPSTREAM || r.bn2 == BN2_STAGED_ROWMASK || r.bn2 == BN2_STAGED_FROM_READOUT) {
        // ... and dH before it, from the upstream gradient
        a.src = c.dg ? sc.dY : c.dxout; a.lds = d.ldo;
        a.w_aw = sc.pk.colp + (size_t)CP_AVEW * d.fp;
        a.w_rowm = r.bn2 != BN2_STAGED_FROM_UPSTREAM;
        if (r.bn2 == BN2_STAGED_FROM_READOUT && !r.rows_late) { a.src = c.o.top_dge; a.lds = c.o.rg->F; a.w_gather = true; }
        agg_set_drop(a, c.drop);
    }
    EdgeArgs e;
    e.bt = *b; e.vc = d.vc; e.dY = sc.dY; e.Y = w->Y; e.P = w->P; e.ld = d.fp; e.sig = sc.pk.sig;
    e.rsig = sc.pk.rsig; e.rscale = w->rscale; e.datt = r.edge_atomic ? sc.eacc : sc.datt; e.atomic = r.edge_atomic ? 1 : 0;
    switch (r.edge) {
    case EDGE_NONE:              // input-only (agg.hip: molecules of more than 256 atoms, code books)
        return r.bwd_agg == AGG_LAGG ? launch_lagg_bwd(a, e, s, false) : launch_agg(a, true, s);
    case EDGE_WITH_LAGG: return launch_lagg_bwd(a, e, s);       // both from the same LDS gathers
    default: return launch_agg_edge(a, e, s);                   // EDGE_COLAUNCH: one grid for both
    }
}

// dX = dP.Wcat^T and dW = X^T.dP
static int bwd_products(LayerBwd& c, const LayerOperands& o) {
    const eagcn_batch* b = c.b; const LayerDims& d = c.d; const LayerScratch& sc = c.sc; hipStream_t s = c.s;
    const PlaneProducts bq = layer_plane_products(b, d, o);
    const Fp32Products gq = layer_fp32_products(b, d, o, c.gemm_work);
    DwScatter dsc;
    for (int k = 0; k < EAGCN_MAX_VIEWS; ++k) dsc.dW[k] = c.gp.dW[k];
    dsc.vc = d.vc;
    dsc.in = c.in;
    int rc;
    c.nsplit = d.nsplit;
    if (c.r.dw_fused) {          // the transposed aggregation wrote every one of its slabs: nothing to launch
        c.nsplit = c.r.dw_ny;
        return EAGCN_OK;
    }
    switch (c.r.bwd_prod) {
    case BWD_PLANES_DX: return launch_bx3(bq.bx, nullptr, d.np, s, c.gemm_work, PROF_GEMM, bx3_pick_wide(bq.bx, nullptr, b->t_hint));
    case BWD_TILED_DX: return launch_gemm(gq.gx, s);
    case BWD_PLANES_PAIR: {
        BxProb bx = bq.bx;
        if (c.r.carries_below) {       // the layer below's dH and column sums leave with dX (bx3.h BxBnEpi)
            EAGCN_CHECK_ARG(c.o.below->Y && c.o.below->bn && c.o.below->row_m && c.o.below->slab && c.o.below->fp == bx.N && bx.ldc == bx.N,
                            "eagcn_layer_backward: incomplete description of the layer below");
            // (bx3_epi.h: a lane takes four adjacent columns of dX and Y' at once -- inside or outside the matrix together)
            EAGCN_CHECK_ARG((bx.N & 3) == 0 && (c.o.below->ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(c.o.below->slab) & 15) == 0,
                            "eagcn_layer_backward: the tail pass of the dX product needs packed widths that are multiples of 4");
            bx.ep = *c.o.below;
        }
        rc = launch_bx3(bx, &bq.bw, d.np, s, 2.0 * c.gemm_work, PROF_GEMM_PAIR, c.r.bx_wide);
        c.nsplit = d.bx_splits;                       // partial slabs of dWcat: summed and scattered by unpack_grads
        c.bx_slabs = true;
        c.bx_per = bx3_pair_policy() ? std::max(1, bx3_grid() >> 3) : 0;
        return rc;
    }
    case BWD_PLANES_DW:
        rc = launch_bx3(bq.bw, nullptr, d.np, s, c.gemm_work, PROF_GEMM, c.r.bx_wide);
        c.nsplit = d.bx_splits;
        c.bx_slabs = true;
        return rc;
    case BWD_G3_XK:              // every XCD works on its own eighth of the packed rows for BOTH products
        rc = launch_gemm3_pair(gq.gx, gq.gw, nullptr, sc.gws, gemm3_workspace_bytes(), s, d.wslab);
        c.nsplit = 1;
        c.xk_G = gemm3_grid();
        return rc;
    case BWD_G3_SCATTER:
        rc = launch_gemm3_pair(gq.gx, gq.gw, &dsc, sc.gws, gemm3_workspace_bytes(), s);
        c.nsplit = 0;                                 // no partial slabs: unpack_grads only reduces the edge partials
        return rc;
    case BWD_TILED_PAIR: return launch_gemm_pair(gq.gx, gq.gw, s);              // dX and dW share one grid
    default: return launch_gemm(gq.gw, s);           // BWD_TILED_SEPARATE: dW alone (no dX was asked for)
    }
}

// dW slabs summed and scattered into the per-view gradients, edge partials reduced -- or that reduction handed down
static int bwd_unpack(LayerBwd& c) {
    const eagcn_batch* b = c.b; const eagcn_layer_params* p = c.p; const LayerDims& d = c.d; const LayerScratch& sc = c.sc;
    if (b->T == 0) {
        // a batch without a single bond has no packed row: no product ran, the weight gradients are exactly zero (the edge
        // partials below are summed over zero workgroups; the BatchNorm gradients came from the row-less reduction)
        for (int k = 0; k < p->K; ++k)
            { int rcz = zero_fill(c.gp.dW[k], (size_t)d.fin * p->width[k] * sizeof(float), c.s); if (rcz) return rcz; }
    }
    if (c.r.defer_drain) {
        EdgeDrain* out = c.o.drain_out;
        out->eacc = sc.eacc; out->K = p->K; out->rsig = sc.pk.rsig;
        for (int k = 0; k < EAGCN_MAX_VIEWS; ++k) {
            out->datt_w[k] = c.gp.datt_w[k]; out->dself_r[k] = c.gp.dself_r[k]; out->channels[k] = c.pp.channels[k];
        }
        return EAGCN_OK;
    }
    const int wblocks = c.nsplit > 0 ? cdiv((int)d.wslab, 256) : 0;     // (one thread per element: four lanes per four elements, unpack_grads)
    const bool shared = b->T > 0 && c.r.edge_atomic;                    // shared accumulators: zeroed again by the threads that read them
    const int nedge = b->T > 0 ? (shared ? -EDGE_COPIES : edge_grid_x(b)) : 0;
    ProfScope psu(PROF_PACK, c.s);
    unpack_grads_kernel<<<wblocks + cdiv(p->K * EDGE_SLAB, 16), 256, 0, c.s>>>(c.gp, c.pp, d.vc, c.in, d.ld_in, d.fp,
                                                                                  (c.r.dw_fused && c.r.dw_in_dp) ? sc.dP : sc.dWcat,
                                                                                  c.bx_slabs ? -c.nsplit : c.nsplit, d.wslab,
                                                                                  shared ? sc.eacc : sc.datt, nedge, sc.pk.rsig,
                                                                                  wblocks, b->meta, c.xk_G, shared ? 1 : 0, c.bx_per, c.r.bx_wide ? 1 : 0,
                                                                                  c.r.dw_fused ? 1 : 0);        // (the aggregation's epilogue wrote every one of its slabs, whatever the row count)
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

int eagcn::layer_backward_impl(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w,
                               const float* dxout, const float* dpad_row, float* dx, const eagcn_layer_grads* g, void* stream,
                               const LayerRoute& r, const LayerBwdOpts& o) {
    if (o.drain_out) o.drain_out->eacc = nullptr;
    int rc = check_layer(b, p, "eagcn_layer_backward");
    if (rc) return rc;
    EAGCN_CHECK_ARG(w && (g || o.input_only) && w->bn && w->scratch, "eagcn_layer_backward: null buffer");
    EAGCN_CHECK_ARG(!o.input_only || (dx && !o.drain_in), "eagcn_layer_backward: the input-only form needs dx and takes no edge reduction");
    EAGCN_CHECK_ARG(b->T == 0 || ((dxout || o.rg) && (o.input_only || w->x || w->x_planes) && w->P && w->Y && w->rscale),
                    "eagcn_layer_backward: null activation buffer");
    if (!o.input_only)
        for (int k = 0; k < p->K; ++k)
            EAGCN_CHECK_ARG(g->dW[k] && g->dbias[k] && g->dgamma[k] && g->dbeta[k] && g->datt_w[k] && g->dself_r[k],
                            "eagcn_layer_backward: view %d has a null gradient buffer", k);
    LayerBwd c;
    c.b = b; c.p = p; c.w = w; c.dxout = dxout; c.dpad_row = dpad_row; c.o = o;
    c.d = layer_dims(b, p);
    const LayerDims& d = c.d;
    rc = carve_checked(b, w, d, true, &c.sc, "eagcn_layer_backward");      // (packed: re-laid by the forward call and kept)
    if (rc) return rc;
    if (o.input_only)
        EAGCN_CHECK_ARG(d.wslab >= (size_t)3 * d.fp + EAGCN_MAX_VIEWS, "eagcn_layer_backward: no room for the discarded BatchNorm gradients");
    c.s = (hipStream_t)stream;
    c.wt = p->structure == EAGCN_STRUCT_WEIGHTED;
    c.dg = o.rg && o.rg->dg;
    c.pp = param_ptrs(b, p);
    c.gp = grad_ptrs(p, g, d, o.input_only ? c.sc.dWcat : nullptr);
    c.in = make_colmap(&p->in);
    c.drop = drop_args(p->dropout, p->training != 0, p->seed, p->seed_dev);
    c.gemm_work = layer_gemm_work(b, p, d);
    if (!w->packed) launch_pack_params(c.pp, d, c.in, c.sc.pk, c.s);
    EAGCN_LAUNCH_CHECK();
    EAGCN_CHECK_ARG(!o.top_sums || (o.top_nslab >= 1 && c.dg && !o.input_only && !o.drain_in && p->training && !w->stats_hook),
                    "eagcn_layer_backward: column sums from the read-out belong to a top layer in training mode with a local BatchNorm");
    EAGCN_CHECK_ARG(!o.dh_sums || (o.dh_nslab >= hidden_bn_slabs(b->T) && dxout && !c.dg && !o.input_only && !o.drain_in && !o.zero_after &&
                                   !dpad_row && p->training && !w->stats_hook && !o.top_sums),
                    "eagcn_layer_backward: dH and its column sums from the layer above belong to a hidden layer in training mode with a local BatchNorm");
    c.r = r;
    // options and a route that do not belong together (the model engine derives both from one plan)
    EAGCN_CHECK_ARG(!o.dh_sums || r.dh_given, "eagcn_layer_backward: dH and its column sums were given, but the layer's route has no use for them");
    EAGCN_CHECK_ARG(!o.top_sums || r.bn2 == BN2_STAGED_FROM_READOUT,
                    "eagcn_layer_backward: column sums from the read-out were given, but the layer's route has no use for them");
    EAGCN_CHECK_ARG((!r.dh_given || o.dh_sums) && (!r.carries_below || o.below) &&
                        (r.bn2 != BN2_STAGED_FROM_READOUT || (o.top_sums && (r.rows_late || top_gather_ok(p, o.top_dge, o.rg->F)))),
                    "eagcn_layer_backward: the route was planned for other arguments");

    rc = bwd_batchnorm(c);
    if (rc) return rc;
    if (b->T > 0) {
        if (c.r.bwd_prod == BWD_REFUSED) {
            set_error("eagcn_layer_backward: the input exists as plane images only and the plane products do not apply");
            return EAGCN_ERR_ARG;
        }
        if (c.r.bwd_split_x) {
            rc = launch_bx3_split(w->x, b->T, b->meta + EAGCN_META_T, d.ld_in, c.sc.xp, bx_plane_elems(b->T, d.ld_in), b->T, d.np, c.s);
            if (rc) return rc;
        }
        rc = bwd_aggregate(c);
        if (rc) return rc;
        rc = bwd_products(c, layer_operands(w, c.sc, dx));
        if (rc) return rc;
    }
    if (o.input_only) return EAGCN_OK;                 // (no parameter gradient is formed)
    return bwd_unpack(c);
}

extern "C" int eagcn_attention_dense(const eagcn_batch* b, const eagcn_layer_params* p, float* out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    EAGCN_CHECK_ARG(b && p && out, "eagcn_attention_dense: null argument");
    EAGCN_CHECK_ARG(p->K == b->K, "eagcn_attention_dense: view count mismatch");
    EAGCN_CHECK_ARG(b->code, "eagcn_attention_dense: batch has no code map");
    ParamPtrs pp;
    memset(&pp, 0, sizeof(pp));
    for (int k = 0; k < p->K; ++k) {
        EAGCN_CHECK_ARG(p->att_w[k], "eagcn_attention_dense: view %d has no attention weight", k);
        pp.att_w[k] = p->att_w[k];
        pp.channels[k] = b->channels[k];
        pp.rel_vec[k] = b->rel_vec[k]; pp.rel_c[k] = b->rel_c[k];
    }
    const size_t total = (size_t)b->K * b->B * b->N * b->N;
    attention_dense_kernel<<<ew_grid(total), 256, 0, s>>>(*b, pp, out);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}
