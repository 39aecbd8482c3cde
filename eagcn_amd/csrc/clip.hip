// Gradient-norm clipping and non-finite step skipping for the flat optimizer step (eagcn_amd/optim.py FlatAdam), on the device:
// what `torch.nn.utils.clip_grad_norm_(params, max_norm)` in front of `optimizer.step()` is in the reference's kind of training
// loop, without the host ever seeing the norm (the update is the last launch of a captured step graph).  Two launches:
//   eagcn_grad_norm          sum of squares (fp64, squares formed in fp64) and count of non-finite values of the LIVE gradient
//                            elements of the flat buffer -> workspace {sumsq, n_bad}
//   eagcn_adam_step_clipped  eagcn_adam_step (csrc/loss.hip) on g' = coef g, coef = min(1, max_norm / (sqrt(sumsq) + 1e-6)); no
//                            workgroup touches anything when n_bad > 0 and skipping is on
// The norm is bit-reproducible from run to run: every workgroup writes ONE partial into its own slot of the workspace, the
// workgroup that finishes last (a ticket, as adam_step_kernel finds the one that advances the step count) adds the slots in slot
// order.  No floating-point atomics, no waiting on another workgroup.
#include <algorithm>

#include "common.h"

namespace eagcn {

constexpr int NORM_MAX_WGS = 1024;       // the grid cap of eagcn_adam_step
constexpr int NORM_UNROLL = 4;           // float4 loads a thread has in flight

// workspace (include/eagcn_hip.h): 32-byte head, then one 16-byte slot per workgroup
struct NormHead {
    double sumsq;
    unsigned long long n_bad;
    unsigned ticket;
    unsigned reserved[3];
};
struct NormSlot {
    double sumsq;
    unsigned long long n_bad;
};
static_assert(sizeof(NormHead) == 32 && sizeof(NormSlot) == 16, "workspace layout of include/eagcn_hip.h");

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// lanes == NULL: every element is live.  Otherwise lanes[i] = number of leading live floats of float4 i (0..4): a parameter's
// slot is its elements followed by <= 3 pad words, a frozen parameter's slot holds 0 throughout.
template <bool HAS_LANES>
__global__ __launch_bounds__(256) void grad_norm_kernel(const float* __restrict__ g, const uint8_t* __restrict__ lanes, size_t n4,
                                                        NormHead* __restrict__ head, NormSlot* __restrict__ slots, int accumulate) {
    __shared__ double s_sum[4];
    __shared__ unsigned long long s_bad[4];
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    double acc = 0.0;
    unsigned bad = 0;
    for (size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n4; i0 += stride * NORM_UNROLL) {
        float4 gg[NORM_UNROLL];
        int live[NORM_UNROLL];
#pragma unroll
        for (int u = 0; u < NORM_UNROLL; ++u) {        // all loads of the trip first: NORM_UNROLL x 16 bytes per thread in flight
            const size_t i = i0 + u * stride;
            const bool ok = i < n4;
            const size_t ic = ok ? i : i0;             // (past the end: re-read this trip's first group, count none of its lanes)
            gg[u] = reinterpret_cast<const float4*>(g)[ic];
            const int ln = HAS_LANES ? (int)lanes[ic] : 4;
            live[u] = ok ? ln : 0;
        }
#pragma unroll
        for (int u = 0; u < NORM_UNROLL; ++u) {
            const float* ge = &gg[u].x;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool on = e < live[u];
                const double x = on ? (double)ge[e] : 0.0;     // the square of an fp32 value is exact in fp64 and cannot overflow
                acc += x * x;
                bad += (on && !(fabsf(ge[e]) <= 3.402823466e+38f)) ? 1u : 0u;  // NaN and +-Inf fail the comparison
            }
        }
    }
    acc = wave_sum(acc);
    unsigned long long nb = wave_sum_u64((unsigned long long)bad);
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = acc; s_bad[threadIdx.x >> 6] = nb; }
    __syncthreads();
    __shared__ unsigned s_last;
    if (threadIdx.x == 0) {
        const double part = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        const unsigned long long pbad = s_bad[0] + s_bad[1] + s_bad[2] + s_bad[3];
        // publish the slot (write-through stores, agent-scope release), then take a ticket
        __hip_atomic_store(&slots[blockIdx.x].sumsq, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&slots[blockIdx.x].n_bad, pbad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(&head->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == gridDim.x - 1 ? 1u : 0u;
        if (s_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!s_last) return;
    // the last workgroup: every slot has been published.  All threads fetch the slots past L1 (one round of independent loads; a
    // single thread's chain of dependent loads took 70 us for 480 slots), ONE thread adds them in slot order: the same sum in every run
    __shared__ double s_part[NORM_MAX_WGS];
    __shared__ unsigned long long s_pbad[NORM_MAX_WGS];
    for (unsigned k = threadIdx.x; k < gridDim.x; k += blockDim.x) {
        s_part[k] = __hip_atomic_load(&slots[k].sumsq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_pbad[k] = __hip_atomic_load(&slots[k].n_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double tot = 0.0;
    unsigned long long tbad = 0;
#pragma unroll 8
    for (unsigned k = 0; k < gridDim.x; ++k) {
        tot += s_part[k];
        tbad += s_pbad[k];
    }
    if (accumulate) { tot += head->sumsq; tbad += head->n_bad; }       // (written by an earlier launch of the stream)
    head->sumsq = tot;
    head->n_bad = tbad;
    __hip_atomic_store(&head->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// adam_step_kernel of csrc/loss.hip on the scaled gradient.  SCALE = false is that kernel's loop, expression by expression (the
// coefficient's fp32 image is 1: same bits as eagcn_adam_step); SCALE = true rounds coef * g to fp32 FIRST (torch scales p.grad in
// place before Adam adds the weight decay: fma(coef, g, wd p) would round differently).
template <bool SCALE>
__device__ __forceinline__ void adam_update_loop(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                 float* __restrict__ v, size_t n4, float coef, float wd, float omb1, float b2,
                                                 float omb2, float eps, float step_size, float inv_sqrt_bc2) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 pp = reinterpret_cast<float4*>(p)[i], mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float* pe = &pp.x; float* me = &mm.x; float* ve = &vv.x; const float* ge = &gg.x;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float gs = SCALE ? __fmul_rn(coef, ge[e]) : ge[e];
            const float gr = gs + wd * pe[e];
            me[e] = me[e] + omb1 * (gr - me[e]);
            ve[e] = b2 * ve[e] + omb2 * gr * gr;
            const float denom = sqrtf(ve[e]) * inv_sqrt_bc2 + eps;
            pe[e] = pe[e] - step_size * (me[e] / denom);
        }
        reinterpret_cast<float4*>(p)[i] = pp; reinterpret_cast<float4*>(m)[i] = mm; reinterpret_cast<float4*>(v)[i] = vv;
    }
}

// stats = {applied, skipped, clipped} as 64-bit counts, then last_norm as a double (include/eagcn_hip.h)
__global__ __launch_bounds__(256) void adam_step_clipped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                float* __restrict__ v, size_t n4, const double* __restrict__ hyper,
                                                                long long* step, unsigned* done, NormHead* norm,
                                                                const double* __restrict__ clip, long long* stats) {
    const long long t = *reinterpret_cast<volatile long long*>(step) + 1;
    // (the norm launch in front of this one wrote the totals; nobody writes them during this launch)
    const double sumsq = *reinterpret_cast<volatile double*>(&norm->sumsq);
    const unsigned long long n_bad = *reinterpret_cast<volatile unsigned long long*>(&norm->n_bad);
    const double max_norm = clip[0];
    const bool skip = n_bad > 0 && clip[1] != 0.0;
    // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1 (a NaN stays a NaN, as torch.clamp
    // leaves it); one fp32 image of it multiplies every gradient
    const double total_norm = sqrt(sumsq);
    const double c = max_norm / (total_norm + 1e-6);
    const float coef = (float)(c >= 1.0 ? 1.0 : c);
    if (!skip) {
        const double b1d = hyper[1], b2d = hyper[2];
        const float b2 = (float)b2d, omb1 = (float)(1.0 - b1d), omb2 = (float)(1.0 - b2d);
        const float eps = (float)hyper[3], wd = (float)hyper[4];
        const double bc1 = 1.0 - pow(b1d, (double)t), bc2 = 1.0 - pow(b2d, (double)t);
        const float step_size = (float)(hyper[0] / bc1), inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
        if (coef == 1.0f) adam_update_loop<false>(p, g, m, v, n4, coef, wd, omb1, b2, omb2, eps, step_size, inv_sqrt_bc2);
        else adam_update_loop<true>(p, g, m, v, n4, coef, wd, omb1, b2, omb2, eps, step_size, inv_sqrt_bc2);
    }
    if (!done) return;                                 // (a partial update: the caller's last range brings the ticket)
    __shared__ unsigned ticket;
    __syncthreads();
    if (threadIdx.x == 0) ticket = atomicAdd(done, 1u);
    __syncthreads();
    if (ticket == gridDim.x - 1 && threadIdx.x == 0) {
        *done = 0u;
        norm->ticket = 0u;
        if (skip) {
            stats[1] += 1;
        } else {
            *step = t;
            stats[0] += 1;
            if (coef < 1.0f) stats[2] += 1;
        }
        reinterpret_cast<double*>(stats)[3] = total_norm;
    }
}

}  // namespace eagcn

using namespace eagcn;

extern "C" size_t eagcn_grad_norm_workspace_bytes(void) { return sizeof(NormHead) + (size_t)NORM_MAX_WGS * sizeof(NormSlot); }

static unsigned flat_grid(size_t n4) { return (unsigned)std::max<size_t>(1, std::min<size_t>((n4 + 255) / 256, NORM_MAX_WGS)); }

extern "C" int eagcn_grad_norm(const float* grad, const uint8_t* live_lanes, int64_t n, void* workspace, int accumulate, void* stream) {
    EAGCN_CHECK_ARG(grad && workspace, "eagcn_grad_norm: null argument");
    EAGCN_CHECK_ARG(n >= 0 && (n & 3) == 0, "eagcn_grad_norm: the flat buffer holds a multiple of 4 floats (ModelPlan pads every parameter)");
    EAGCN_CHECK_ARG(((reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(workspace)) & 15) == 0,
                    "eagcn_grad_norm: the gradient buffer and the workspace must be 16-byte aligned");
    const size_t n4 = (size_t)n / 4;
    // (n == 0 still launches: one workgroup that replaces the totals by 0 or leaves them, so that a stale total is never applied)
    NormHead* head = static_cast<NormHead*>(workspace);
    NormSlot* slots = reinterpret_cast<NormSlot*>(head + 1);
    if (live_lanes) grad_norm_kernel<true><<<flat_grid(n4), 256, 0, (hipStream_t)stream>>>(grad, live_lanes, n4, head, slots, accumulate ? 1 : 0);
    else grad_norm_kernel<false><<<flat_grid(n4), 256, 0, (hipStream_t)stream>>>(grad, live_lanes, n4, head, slots, accumulate ? 1 : 0);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

extern "C" int eagcn_adam_step_clipped(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                       const double* hyper_dev, int64_t* step_dev, uint32_t* ticket_dev, void* norm_workspace,
                                       const double* clip_dev, int64_t* stats_dev, void* stream) {
    EAGCN_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && hyper_dev && step_dev && norm_workspace && clip_dev && stats_dev,
                    "eagcn_adam_step_clipped: null argument");
    EAGCN_CHECK_ARG(n >= 0 && (n & 3) == 0,
                    "eagcn_adam_step_clipped: the flat buffers hold a multiple of 4 floats (ModelPlan pads every parameter)");
    EAGCN_CHECK_ARG(((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
                      reinterpret_cast<uintptr_t>(exp_avg_sq) | reinterpret_cast<uintptr_t>(norm_workspace)) & 15) == 0,
                    "eagcn_adam_step_clipped: buffers must be 16-byte aligned");
    EAGCN_CHECK_ARG(((reinterpret_cast<uintptr_t>(clip_dev) | reinterpret_cast<uintptr_t>(stats_dev)) & 7) == 0,
                    "eagcn_adam_step_clipped: clip_dev and stats_dev must be 8-byte aligned");
    if (n == 0) return EAGCN_OK;
    const size_t n4 = (size_t)n / 4;
    adam_step_clipped_kernel<<<flat_grid(n4), 256, 0, (hipStream_t)stream>>>(param, grad, exp_avg, exp_avg_sq, n4, hyper_dev,
                                                                              (long long*)step_dev, ticket_dev,
                                                                              static_cast<NormHead*>(norm_workspace), clip_dev,
                                                                              (long long*)stats_dev);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}
