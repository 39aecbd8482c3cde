// Bond attributions: d target / d A1 of every bond of the batch index's row lists, per view and layer, times a function of the bond's
// attention logit (include/eagcn_hip.h, "bond attribution"), and the finalize launch behind the layers' sum.
//   eval-mode layer, saved P (X.Wcat), Y (pre-bias aggregation), rscale (m_i / rowsum_i), bn (scale / shift), upstream gradient dxout:
//     dY_i[c]  = sc[c] [sc[c] Y_i[c] + sh[c] > 0] dH_i[c],   dH_i[c] = m_i dxout_i[c] (Concate) | ave_w[k] dxout_i[c - off_k] (Weighted_sum)
//     D[k][e]  = rscale_k[i] < dY_i , P_j - Y_i >  over view k's columns          (e = bond (i, j) of packed row i)
//     acc[k][e] (+)= weight f(z_k(e)) D[k][e],   f = sigmoid (mode 0) | sigmoid (1 - sigmoid) z (mode 1)
// One wave per packed row: the row's rscale dY_i and Y_i are formed once into registers (16-byte loads; a view segment is padded to 16
// columns, so four adjacent columns never straddle views), then every bond of the row streams P_j once from global memory -- no molecule
// is staged in LDS, so the kernel serves molecules of any size -- with the difference P_j - Y_i formed BEFORE the multiply (the two dots
// cancel), one partial sum per view and one reduce-scatter of the views across the wave.  Every (k, e) has one owner (lane 8 k of the
// row's wave): no atomics, repeated runs are bit-identical.  A launch covers 256 NCH packed columns; wider layers take several launches
// (D is a sum over columns).
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace eagcn {

struct BondGradArgs {
    eagcn_batch bt;
    const float* P; const float* Y; const float* rscale; const float* bn; const float* dxout;
    const float* att_w[EAGCN_MAX_VIEWS];
    const float* ave_w;
    ViewCols vc;
    int fp, ldo, structure, mode, first, c0;   // c0: first packed column of this launch
    float weight;
    float* acc;
};

// attention logit of bond code c (1-based) in view K: w[c-1] for one-hot relation tensors, <w, vec[c-1]> in general (layers.py:82; as
// att_logit of layer.hip); 0 for a code outside the view's range.  K is a compile-time index: every table is read at a static slot.
template <int K>
__device__ __forceinline__ float bond_logit(const BondGradArgs& a, int c) {
    if (c < 1 || c > a.bt.channels[K]) return 0.0f;
    if (!a.bt.rel_vec[K]) return a.att_w[K][c - 1];
    const float* v = a.bt.rel_vec[K] + (size_t)(c - 1) * a.bt.rel_c[K];
    float s = 0.0f;
    for (int ch = 0; ch < a.bt.rel_c[K]; ++ch) s = fmaf(a.att_w[K][ch], v[ch], s);
    return s;
}
__device__ __forceinline__ float bond_factor(float z, int mode) {
    const float s = sigmoidf_(z);
    return mode == 0 ? s : s * (1.0f - s) * z;
}

__device__ __forceinline__ float dot4_diff(const float4& g, const float4& p, const float4& y) {
    return (g.x * (p.x - y.x) + g.y * (p.y - y.y)) + (g.z * (p.z - y.z) + g.w * (p.w - y.w));
}

// f(z) of every view at the bond's codes, left in the lanes that own the view's sum (lanes 8 K .. 8 K + 7, view_reduce_scatter)
template <int K>
__device__ __forceinline__ void bond_factors(const BondGradArgs& a, uint64_t code, int lane, float& fz) {
    if constexpr (K < EAGCN_MAX_VIEWS) {
        if (K < a.vc.K) {                                   // (wave-uniform)
            const int c = (int)((code >> (8 * K)) & 255u);
            const bool live = c >= 1 && c <= a.bt.channels[K];
            const float f = live ? bond_factor(bond_logit<K>(a, c), a.mode) : 0.0f;
            if ((lane >> 3) == K) fz = f;
            bond_factors<K + 1>(a, code, lane, fz);
        }
    }
}

// Per-lane partial sums of the eight views -> view (lane >> 3)'s total over the wave, in every lane: a reduce-scatter over lane bits
// 5, 4, 3 (a lane keeps the half of its values whose view has the lane's bit and sends the other half: 8 -> 4 -> 2 -> 1 values),
// then a butterfly over bits 2, 1, 0.  Ten exchanges in a fixed order instead of six per view.
__device__ __forceinline__ float view_reduce_scatter(const float (&v)[EAGCN_MAX_VIEWS], int lane) {
    static_assert(EAGCN_MAX_VIEWS == 8, "the reduce-scatter halves eight values three times");
    const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;
    float w4[4], w2[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) w4[i] = (b5 ? v[i + 4] : v[i]) + __shfl_xor(b5 ? v[i] : v[i + 4], 32);
#pragma unroll
    for (int i = 0; i < 2; ++i) w2[i] = (b4 ? w4[i + 2] : w4[i]) + __shfl_xor(b4 ? w4[i] : w4[i + 2], 16);
    float s = (b3 ? w2[1] : w2[0]) + __shfl_xor(b3 ? w2[0] : w2[1], 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    return s;
}

template <int NCH>
__global__ __launch_bounds__(256) void bond_grad_kernel(BondGradArgs a) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int T = dev_rows(a.bt), fp = a.fp;
    for (int r = blockIdx.x * 4 + wid; r < T; r += gridDim.x * 4) {
        const int2 rp = reinterpret_cast<const int2*>(a.bt.row_ptr)[r];
        if (rp.y <= 0 || rp.x < 0 || rp.x > a.bt.E - rp.y) continue;           // no bond of its own / not a list range (wave-uniform)
        const int4 ri = reinterpret_cast<const int4*>(a.bt.row_info)[r];       // {molecule, atom, nat, row0}
        const float m = a.bt.row_m[r];
        float4 g[NCH], y[NCH];
        int vk[NCH], cl[NCH];
#pragma unroll
        for (int u = 0; u < NCH; ++u) {
            const int c = a.c0 + 4 * (lane + 64 * u);
            const bool ok = c < fp;
            const int cc = ok ? c : 0;                      // (columns beyond the layer load column 0 and weigh nothing)
            int k = 0, off = 0, wd = a.vc.width[0];
#pragma unroll
            for (int v = 1; v < EAGCN_MAX_VIEWS; ++v)
                if (v < a.vc.K && cc >= a.vc.off[v]) { k = v; off = a.vc.off[v]; wd = a.vc.width[v]; }
            const int f = cc - off;
            const float4 yv = *reinterpret_cast<const float4*>(a.Y + (size_t)r * fp + cc);
            const float4 sc = *reinterpret_cast<const float4*>(a.bn + (size_t)BN_SC * fp + cc);
            const float4 sh = *reinterpret_cast<const float4*>(a.bn + (size_t)BN_SH * fp + cc);
            const float4 dx = *reinterpret_cast<const float4*>(a.dxout + (size_t)r * a.ldo + (a.structure == EAGCN_STRUCT_CONCATE ? cc : f));
            // rscale_k[i] dH: the row mask (Concate) or the view's mixing weight (Weighted_sum)
            const float hs = a.rscale[(size_t)k * a.bt.T + r] * (a.structure == EAGCN_STRUCT_CONCATE ? m : a.ave_w[k]);
            float4 gv;
            gv.x = (ok && f + 0 < wd && sc.x * yv.x + sh.x > 0.0f) ? hs * sc.x * dx.x : 0.0f;
            gv.y = (ok && f + 1 < wd && sc.y * yv.y + sh.y > 0.0f) ? hs * sc.y * dx.y : 0.0f;
            gv.z = (ok && f + 2 < wd && sc.z * yv.z + sh.z > 0.0f) ? hs * sc.z * dx.z : 0.0f;
            gv.w = (ok && f + 3 < wd && sc.w * yv.w + sh.w > 0.0f) ? hs * sc.w * dx.w : 0.0f;
            g[u] = gv; y[u] = yv; vk[u] = ok ? k : -1; cl[u] = cc;
        }
        for (int t0 = 0; t0 < rp.y; t0 += 64) {             // the row's list entries, 64 at a time: one load per lane
            const int nt = min(rp.y - t0, 64);
            const int el = rp.x + t0 + min(lane, nt - 1);
            const int jl = a.bt.nbr[el];
            const uint64_t codel = a.bt.ecode[el];
            for (int t = 0; t < nt; ++t) {
                const int e = rp.x + t0 + t;
                const int j = __shfl(jl, t);
                const uint64_t code = ((uint64_t)(uint32_t)__shfl((int)(codel >> 32), t) << 32) | (uint32_t)__shfl((int)codel, t);
                const bool jok = j >= 0 && j < ri.z && ri.w + j < T;          // a bond into a row that is not stored weighs 0
                const float* prow = a.P + (size_t)(ri.w + (jok ? j : 0)) * fp;
                float4 p[NCH];
#pragma unroll
                for (int u = 0; u < NCH; ++u) p[u] = *reinterpret_cast<const float4*>(prow + cl[u]);
                float fz = 0.0f;
                bond_factors<0>(a, code, lane, fz);
                float v[EAGCN_MAX_VIEWS];
#pragma unroll
                for (int k = 0; k < EAGCN_MAX_VIEWS; ++k) v[k] = 0.0f;
#pragma unroll
                for (int u = 0; u < NCH; ++u) {
                    const float d = dot4_diff(g[u], p[u], y[u]);
#pragma unroll
                    for (int k = 0; k < EAGCN_MAX_VIEWS; ++k) v[k] += vk[u] == k ? d : 0.0f;
                }
                const float res = view_reduce_scatter(v, lane);
                if ((lane & 7) == 0 && (lane >> 3) < a.vc.K) {               // lane 8 k owns (view k, e)
                    float* o = a.acc + (size_t)(lane >> 3) * a.bt.E + e;
                    const float val = jok ? a.weight * fz * res : 0.0f;
                    *o = a.first ? val : *o + val;
                }
            }
        }
    }
}

// one thread per packed row: the triples (molecule, i, j) of its list entries, score[e] = sum_k acc[k][e], and the per-view scores at
// [k][molecule][i][j] of the (zero-filled) dense tensor
__global__ __launch_bounds__(256) void bond_attr_finalize_kernel(eagcn_batch bt, const float* __restrict__ acc, int K, int Nin,
                                                                  int32_t* __restrict__ mol, int32_t* __restrict__ bi,
                                                                  int32_t* __restrict__ bj, float* __restrict__ score,
                                                                  float* __restrict__ dense) {
    const int T = dev_rows(bt);
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < T; r += gridDim.x * blockDim.x) {
        const int2 rp = reinterpret_cast<const int2*>(bt.row_ptr)[r];
        if (rp.y <= 0 || rp.x < 0 || rp.x > bt.E - rp.y) continue;
        const int4 ri = reinterpret_cast<const int4*>(bt.row_info)[r];
        for (int t = 0; t < rp.y; ++t) {
            const int e = rp.x + t, j = bt.nbr[e];
            float s = 0.0f;
            const bool in = dense && ri.x >= 0 && ri.x < bt.B && ri.y >= 0 && ri.y < Nin && j >= 0 && j < Nin;
            for (int k = 0; k < K; ++k) {
                const float v = acc[(size_t)k * bt.E + e];
                s += v;
                if (in) dense[(((size_t)k * bt.B + ri.x) * Nin + ri.y) * Nin + j] = v;
            }
            mol[e] = ri.x; bi[e] = ri.y; bj[e] = j; score[e] = s;
        }
    }
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool has_row_lists(const eagcn_batch* b) {
    return b->build_lists && b->row_ptr && b->row_info && b->row_m && b->meta && (b->E == 0 || (b->nbr && b->ecode));
}

}  // namespace eagcn

using namespace eagcn;

extern "C" int eagcn_layer_bond_grad(const eagcn_batch* b, const eagcn_layer_params* p, const eagcn_layer_bufs* w, const float* dxout,
                                     int mode, float weight, int first, float* acc, void* stream) {
    // (every argument is checked before anything is issued)
    EAGCN_CHECK_ARG(b && p && w && dxout && acc, "eagcn_layer_bond_grad: null argument");
    EAGCN_CHECK_ARG(w->P && w->Y && w->rscale && w->bn, "eagcn_layer_bond_grad: the layer's saved P / Y / rscale / bn are needed");
    EAGCN_CHECK_ARG(mode == 0 || mode == 1, "eagcn_layer_bond_grad: mode %d (0: gradient x attention, 1: gradient x relation input)", mode);
    EAGCN_CHECK_ARG(p->training == 0, "eagcn_layer_bond_grad: eval mode only (training-mode BatchNorm couples the molecules of a batch)");
    EAGCN_CHECK_ARG(has_row_lists(b), "eagcn_layer_bond_grad: the batch index carries no bond lists (eagcn_batch.build_lists)");
    EAGCN_CHECK_ARG(p->K == b->K && p->K >= 1 && p->K <= EAGCN_MAX_VIEWS, "eagcn_layer_bond_grad: view count mismatch (%d / %d)", p->K, b->K);
    EAGCN_CHECK_ARG(p->structure == EAGCN_STRUCT_CONCATE || p->structure == EAGCN_STRUCT_WEIGHTED, "eagcn_layer_bond_grad: structure %d",
                    p->structure);
    EAGCN_CHECK_ARG(p->structure != EAGCN_STRUCT_WEIGHTED || p->ave_w, "eagcn_layer_bond_grad: a Weighted_sum layer needs ave_w");
    for (int k = 0; k < p->K; ++k) {
        EAGCN_CHECK_ARG(p->att_w[k] && p->width[k] >= 1, "eagcn_layer_bond_grad: view %d has no attention weight / width", k);
        EAGCN_CHECK_ARG(p->structure != EAGCN_STRUCT_WEIGHTED || p->width[k] == p->width[0], "eagcn_layer_bond_grad: unequal view widths");
    }
    EAGCN_CHECK_ARG(aligned16(acc) && aligned16(dxout) && aligned16(w->P) && aligned16(w->Y) && aligned16(w->bn),
                    "eagcn_layer_bond_grad: accumulator / dxout / P / Y / bn not 16-byte aligned");
    EAGCN_CHECK_ARG(b->T >= 0 && b->E >= 0, "eagcn_layer_bond_grad: negative capacity");
    if (b->T == 0 || b->E == 0) return EAGCN_OK;
    BondGradArgs a;
    memset(&a, 0, sizeof(a));
    a.bt = *b;
    a.P = w->P; a.Y = w->Y; a.rscale = w->rscale; a.bn = w->bn; a.dxout = dxout;
    for (int k = 0; k < p->K; ++k) a.att_w[k] = p->att_w[k];
    a.ave_w = p->structure == EAGCN_STRUCT_WEIGHTED ? p->ave_w : nullptr;
    a.vc = view_cols(p);
    a.fp = a.vc.off[p->K];
    a.ldo = p->structure == EAGCN_STRUCT_CONCATE ? a.fp : pad16(p->width[0]);
    a.structure = p->structure; a.mode = mode; a.weight = weight; a.acc = acc;
    hipStream_t s = (hipStream_t)stream;
    const int grid = std::max(1, std::min(cdiv(b->T, 4), 8192));
    ProfScope ps(PROF_EDGE, s);
    constexpr int MAXC = 256 * 8;                          // packed columns of the widest instantiation
    for (int c0 = 0; c0 < a.fp; c0 += MAXC) {
        a.c0 = c0;
        a.first = (first && c0 == 0) ? 1 : 0;
        const int nch = cdiv(std::min(a.fp - c0, MAXC), 256);
        if (nch <= 1) bond_grad_kernel<1><<<grid, 256, 0, s>>>(a);
        else if (nch <= 2) bond_grad_kernel<2><<<grid, 256, 0, s>>>(a);
        else if (nch <= 3) bond_grad_kernel<3><<<grid, 256, 0, s>>>(a);
        else if (nch <= 4) bond_grad_kernel<4><<<grid, 256, 0, s>>>(a);
        else bond_grad_kernel<8><<<grid, 256, 0, s>>>(a);
        EAGCN_LAUNCH_CHECK();
    }
    return EAGCN_OK;
}

extern "C" int eagcn_bond_attr_finalize(const eagcn_batch* b, const float* acc, int K, int32_t* mol, int32_t* bi, int32_t* bj, float* score,
                                        float* dense, void* stream) {
    EAGCN_CHECK_ARG(b && mol && bi && bj && score, "eagcn_bond_attr_finalize: null argument");
    EAGCN_CHECK_ARG(has_row_lists(b), "eagcn_bond_attr_finalize: the batch index carries no bond lists (eagcn_batch.build_lists)");
    EAGCN_CHECK_ARG(K >= 1 && K <= EAGCN_MAX_VIEWS, "eagcn_bond_attr_finalize: %d views", K);
    EAGCN_CHECK_ARG(b->T >= 0 && b->E >= 0, "eagcn_bond_attr_finalize: negative capacity");
    if (b->T == 0 || b->E == 0) return EAGCN_OK;
    EAGCN_CHECK_ARG(acc, "eagcn_bond_attr_finalize: null accumulator");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_PACK, s);
    bond_attr_finalize_kernel<<<std::max(1, std::min(cdiv(b->T, 256), 4096)), 256, 0, s>>>(*b, acc, K, b->n_logical > 0 ? b->n_logical : b->N,
                                                                                         mol, bi, bj, score, dense);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}
