// Atom attributions: the gradient of a prediction with respect to the atom features (eagcn_model_backward_input, head.hip) and the
// three small kernels of integrated gradients around it (include/eagcn_hip.h, "attribution"):
//   pack       x_alpha = x' + alpha (x - x') into the packed input slot of `saved` (what eagcn_model_pack_input fills);
//   accumulate acc[T][ld] (+)= w dX0 in PACKED rows, after the input-only backward of one quadrature point (the dense gradient of a
//              point is never formed);
//   finalize   attr[B][N][F] = (x - x') * acc (0 at rows that are not stored) and score[B][N] = sum_f attr, one launch.
// The dense scatter of a plain d / d afm (eagcn_model_backward_input) is the finalize kernel without the (x - x') factor.
// All of them are elementwise over T x ld or B x N x F floats: a few microseconds beside the backward of a point.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace eagcn {

// packed column of exact column ce (segments of width w[s] padded to p[s])
__device__ __forceinline__ int attr_exact_to_packed(const ColMapD& m, int ce) {
    int eo = 0, po = 0;
    for (int s = 0; s < m.nseg; ++s) {
        if (ce < eo + m.w[s]) return po + (ce - eo);
        eo += m.w[s];
        po += m.p[s];
    }
    return -1;
}
// exact column of packed column cp, or -1 in a segment's padding
__device__ __forceinline__ int attr_packed_to_exact(const ColMapD& m, int cp) {
    int eo = 0, po = 0;
    for (int s = 0; s < m.nseg; ++s) {
        if (cp < po + m.p[s]) return cp - po < m.w[s] ? eo + (cp - po) : -1;
        eo += m.w[s];
        po += m.p[s];
    }
    return -1;
}

// x' + alpha (x - x') at every packed element (x' = 0 without a baseline); padding columns 0
__global__ __launch_bounds__(256) void attr_pack_kernel(eagcn_batch bt, const float* __restrict__ x, const float* __restrict__ base,
                                                         float alpha, ColMapD m, int ld, int F, int Nin, float* __restrict__ packed) {
    const uint32_t total = (uint32_t)dev_rows(bt) * (uint32_t)ld;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int r = (int)(e / (uint32_t)ld), cp = (int)(e - (uint32_t)r * (uint32_t)ld);
        const int ce = attr_packed_to_exact(m, cp);
        float v = 0.0f;
        if (ce >= 0) {
            const size_t i = ((size_t)bt.row_mol[r] * Nin + bt.row_loc[r]) * F + ce;
            const float b0 = base ? base[i] : 0.0f;
            v = fmaf(alpha, x[i] - b0, b0);
        }
        packed[e] = v;
    }
}

// acc = w g (first point) or acc += w g, over the packed rows that exist
__global__ __launch_bounds__(256) void attr_accumulate_kernel(eagcn_batch bt, const float* __restrict__ g, float w, int ld, int first,
                                                               float* __restrict__ acc) {
    const uint32_t n4 = (uint32_t)dev_rows(bt) * (uint32_t)ld / 4;           // (ld: a multiple of 4)
    float4* a4 = reinterpret_cast<float4*>(acc);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += gridDim.x * blockDim.x) {
        const float4 v = g4[e];
        float4 o = first ? make_float4(0.f, 0.f, 0.f, 0.f) : a4[e];
        o.x = fmaf(w, v.x, o.x); o.y = fmaf(w, v.y, o.y); o.z = fmaf(w, v.z, o.z); o.w = fmaf(w, v.w, o.w);
        a4[e] = o;
    }
}

// one thread per atom row (b, i): attr[b][i][f] = d (x - x') acc[packed row][packed column of f] (d = 1 and no input factor when
// x == null: the plain dense scatter of a gradient), 0 at rows that are not stored; score[b][i] = sum_f attr (score may be null)
__global__ __launch_bounds__(256) void attr_dense_kernel(eagcn_batch bt, const float* __restrict__ acc, ColMapD m, int ld, int F, int Nin,
                                                          const float* __restrict__ x, const float* __restrict__ base,
                                                          float* __restrict__ attr, float* __restrict__ score) {
    const int nrow = bt.B * Nin;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < nrow; q += gridDim.x * blockDim.x) {
        const int b = q / Nin, i = q - b * Nin;
        const bool stored = i < bt.nat[b] && bt.row0[b] + i < dev_rows(bt);
        const float* ar = acc + (size_t)(stored ? bt.row0[b] + i : 0) * ld;
        const size_t o = (size_t)q * F;
        float s = 0.0f;
        for (int f = 0; f < F; ++f) {
            float v = 0.0f;
            if (stored) {
                v = ar[attr_exact_to_packed(m, f)];
                if (x) v *= x[o + f] - (base ? base[o + f] : 0.0f);
            }
            attr[o + f] = v;
            s += v;
        }
        if (score) score[q] = s;
    }
}

static inline int attr_grid(size_t n) { return (int)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 4096)); }
static inline int attr_nin(const eagcn_batch* b) { return b->n_logical > 0 ? b->n_logical : b->N; }

int launch_attr_dense(const eagcn_batch* b, const eagcn_layout* in, const float* acc, const float* x, const float* base, float* attr,
                      float* score, hipStream_t s) {
    const int Nin = attr_nin(b);
    ProfScope ps(PROF_PACK, s);
    attr_dense_kernel<<<attr_grid((size_t)b->B * Nin), 256, 0, s>>>(*b, acc, make_colmap(in), layout_ld(in), layout_width(in), Nin, x,
                                                                   base, attr, score);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

}  // namespace eagcn

using namespace eagcn;

extern "C" float eagcn_attr_alpha(int step, int steps) { return steps > 0 ? ((float)step + 0.5f) / (float)steps : 0.0f; }
extern "C" float eagcn_attr_weight(int steps) { return steps > 0 ? 1.0f / (float)steps : 0.0f; }

extern "C" size_t eagcn_attr_acc_elems(const eagcn_batch* b, const eagcn_model* m) {
    return (b && m) ? (size_t)std::max(b->T, 1) * layout_ld(&m->layer[0].in) : 0;
}

extern "C" int eagcn_attr_pack_input(const eagcn_batch* b, const eagcn_model* m, const float* afm, const float* baseline, float alpha,
                                     void* saved, size_t saved_bytes, void* stream) {
    EAGCN_CHECK_ARG(b && m && afm && saved, "eagcn_attr_pack_input: null argument");
    int rc = check_reserved_null(m->aux_stream, "eagcn_attr_pack_input", "eagcn_model.aux_stream");
    if (rc) return rc;
    float* x0 = nullptr;
    rc = model_input_slot(b, m, saved, saved_bytes, &x0, "eagcn_attr_pack_input");
    if (rc) return rc;
    if (b->T == 0) return EAGCN_OK;
    const eagcn_layout* in = &m->layer[0].in;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_PACK, s);
    attr_pack_kernel<<<attr_grid((size_t)b->T * layout_ld(in)), 256, 0, s>>>(*b, afm, baseline, alpha, make_colmap(in), layout_ld(in),
                                                                           layout_width(in), attr_nin(b), x0);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

extern "C" int eagcn_attr_step(const eagcn_batch* b, const eagcn_model* m, const int64_t* size, void* saved, size_t saved_bytes,
                               void* scratch, size_t scratch_bytes, const float* dout, const float* dgraph_rep, float weight, int first,
                               float* acc, void* stream) {
    // (every argument is checked before the backward is issued: nothing is queued for a call that fails)
    EAGCN_CHECK_ARG(b && m && acc, "eagcn_attr_step: null argument");
    const int ld = layout_ld(&m->layer[0].in);
    EAGCN_CHECK_ARG((ld & 3) == 0 && (reinterpret_cast<uintptr_t>(acc) & 15) == 0,
                    "eagcn_attr_step: accumulator not 16-byte aligned / input row width %d not a multiple of 4", ld);
    float* dx0 = nullptr;
    int rc = model_backward_input_packed(b, m, size, saved, saved_bytes, scratch, scratch_bytes, dout, dgraph_rep, nullptr, nullptr,
                                         &dx0, stream, "eagcn_attr_step");
    if (rc) return rc;
    if (b->T == 0) return EAGCN_OK;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_PACK, s);
    attr_accumulate_kernel<<<attr_grid((size_t)b->T * ld / 4), 256, 0, s>>>(*b, dx0, weight, ld, first ? 1 : 0, acc);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

extern "C" int eagcn_attr_finalize(const eagcn_batch* b, const eagcn_model* m, const float* afm, const float* baseline, const float* acc,
                                   float* attr, float* score, void* stream) {
    EAGCN_CHECK_ARG(b && m && afm && attr && score, "eagcn_attr_finalize: null argument");
    EAGCN_CHECK_ARG(b->T == 0 || acc, "eagcn_attr_finalize: null accumulator");
    const int rc = check_reserved_null(m->aux_stream, "eagcn_attr_finalize", "eagcn_model.aux_stream");
    if (rc) return rc;
    return launch_attr_dense(b, &m->layer[0].in, acc, afm, baseline, attr, score, (hipStream_t)stream);
}
