// Evaluation metrics of the reference training loop (train.py:130-211) over the device-resident buffers of an evaluation pass
// (eagcn_eval_append: scores / targets fp32, valid uint8, row-major [rows][T]), without a sort and without a host read:
//   classification: per-task ROC-AUC (roc_curve + auc == the Mann-Whitney statistic with average ranks) and average precision,
//   regression:     per-task and overall RMSE and MAE.
// For a task with positives i and labelled entries j
//     neg_lt_i = #{neg j: s_j <  s_i}     neg_eq_i = #{neg j: s_j == s_i}     pos_ge_i = #{pos j: s_j >= s_i}
//     AUC = sum_i (2 neg_lt_i + neg_eq_i) / (2 P N)          AP = 1/P sum_i pos_ge_i / (pos_ge_i + N - neg_lt_i)
// (all positives of one score share one threshold of the precision-recall curve: sklearn's average_precision_score).  The counts
// are integers: the AUC numerator is exact and does not depend on the order of the rows.
//
// Two launches per evaluation, no atomics, no host sync: eval_rank_kernel (or eval_sums_kernel) fills workspace words that
// belong to one workgroup each, eval_finalize_kernel adds them up in a fixed order.  Every word the finalize reads has been
// written by the launch before it, so the workspace is never cleared.  A workgroup of eval_rank_kernel holds 256 entries i of one
// task and walks the task's rows; where the tiles alone would leave most CUs idle (one task, many rows) up to 8 workgroups share a
// tile's rows, each leaves its part of the per-entry counts, and the finalize forms the AP ratios from their sums (the integer AUC
// sums simply add).
#include "common.h"

namespace eagcn {

constexpr int EVAL_R = 256;          // entries i of a workgroup (one per lane)
constexpr int EVAL_J = 1024;         // entries j staged into LDS at a time
constexpr int EVAL_MAX_SPLIT = 8;    // workgroups that share the j range of one tile at the most
constexpr int EVAL_TARGET_WGS = 1024;// four workgroups of four waves per CU: every SIMD issues from several waves
constexpr int EVAL_CHIP_WGS = 256;   // one workgroup per CU: a launch of that many tiles is not split
constexpr int EVAL_FIN_THREADS = 1024;

struct EvalSlot {                    // what one workgroup of eval_rank_kernel leaves (32 bytes)
    unsigned long long num;          // sum over its positive lanes of 2 neg_lt + neg_eq, over its j range
    double ap;                       // sum over its positive lanes of pos_ge / (pos_ge + N - neg_lt) where it walked ALL rows, else 0
    uint32_t P, N, bad;              // positives / negatives / labelled entries with a non-finite score in its j range
    uint32_t pad;
};
struct EvalSums {                    // one workgroup of eval_sums_kernel (32 bytes)
    double sse, sae, cnt, pad;
};
static_assert(sizeof(EvalSlot) == 32 && sizeof(EvalSums) == 32, "the workspace formula of eagcn_hip.h counts 32-byte records");

static inline int64_t eval_tiles(int64_t rows) { return (rows + EVAL_R - 1) / EVAL_R; }
static inline int64_t eval_chunks(int64_t rows) { return (rows + EVAL_J - 1) / EVAL_J; }
static inline size_t eval_workspace_bytes(int64_t rows, int T) {
    const int64_t chunks = eval_chunks(rows);
    const int64_t smax = chunks < EVAL_MAX_SPLIT ? chunks : EVAL_MAX_SPLIT;
    return (size_t)T * (size_t)eval_tiles(rows) * (size_t)smax * (EVAL_R * 8 + sizeof(EvalSlot));
}
// How many workgroups share a tile's j range (each takes `per` chunks of EVAL_J, never an empty one).  One, unless the tiles alone
// leave CUs idle AND the task has many rows for its width (rows >= 1024 T): a lane's walk over the rows is the launch's critical
// path (measured: about 45 ns per row), while a split costs the finalize -- ONE workgroup -- a pass over the per-entry counts of
// every task.  Split: the positives' ratios are formed by the finalize (a lane has only a part of its counts); else by the lane.
static inline void eval_split(int64_t rows, int T, int* nsplit, int* per) {
    const int64_t chunks = eval_chunks(rows), wgs = eval_tiles(rows) * T;
    int64_t s = (wgs < EVAL_CHIP_WGS && rows >= (int64_t)EVAL_J * T) ? EVAL_TARGET_WGS / wgs : 1;
    s = s < 1 ? 1 : (s > EVAL_MAX_SPLIT ? EVAL_MAX_SPLIT : s);
    if (s > chunks) s = chunks;
    *per = (int)((chunks + s - 1) / s);
    *nsplit = (int)((chunks + *per - 1) / *per);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The flat elements [e0, e1) of a row-major [rows][T] block, visited by a workgroup of EVAL_R threads with loads that are
// contiguous over the lanes; a thread follows (row, column) of its element without a division per step.
struct ColWalk {
    int T, q, r, row, col;
    __device__ ColWalk(int T_, int tid) : T(T_), q(EVAL_R / T_), r(EVAL_R % T_), row(tid / T_), col(tid % T_) {}
    __device__ void next() {
        row += q;
        col += r;
        if (col >= T) { col -= T; ++row; }
    }
};

// grid (tiles, nsplit, T).  Lane `tid` holds entry i = tile * EVAL_R + tid of task t (its score if it is a POSITIVE, NaN
// otherwise: only positives carry counts, and a NaN compares false with everything) and walks the rows [jlo, jhi) of the task in
// chunks of EVAL_J staged into LDS as two arrays: the score where the entry is a negative / a positive, NaN where it is not.  The
// class test is thereby paid once per staged entry, not once per pair; in the pair loop every lane reads the same 16 bytes
// (a broadcast, no bank conflicts) and a count costs a compare and an add-with-carry.
__global__ __launch_bounds__(EVAL_R) void eval_rank_kernel(const float* __restrict__ scores, const float* __restrict__ targets,
                                                            const uint8_t* __restrict__ valid, int rows, int T, int per,
                                                            uint2* __restrict__ counts, EvalSlot* __restrict__ slots) {
    __shared__ __attribute__((aligned(16))) float s_neg[EVAL_J];
    __shared__ __attribute__((aligned(16))) float s_pos[EVAL_J];
    __shared__ unsigned long long s_num[EVAL_R / WAVE];
    __shared__ uint32_t s_cls[EVAL_R / WAVE][3];
    __shared__ double s_ap[EVAL_R / WAVE];
    const int tid = threadIdx.x, tile = blockIdx.x, split = blockIdx.y, t = blockIdx.z;
    const int tiles = gridDim.x, nsplit = gridDim.y;
    const float qnan = __int_as_float(0x7fc00000);

    const long long i = (long long)tile * EVAL_R + tid;
    float si = qnan;
    if (i < rows) {
        const size_t e = (size_t)i * T + t;
        if (valid[e] && targets[e] == 1.0f) si = scores[e];
    }
    const long long span = (long long)per * EVAL_J;        // (64-bit: rows may be close to 2^31)
    const int jlo = (int)min((long long)rows, split * span), jhi = (int)min((long long)rows, jlo + span);
    uint32_t neg_lt = 0, neg_eq = 0, pos_ge = 0, nP = 0, nN = 0, nBad = 0;
    for (int j0 = jlo; j0 < jhi; j0 += EVAL_J) {
        const int nj = min(EVAL_J, jhi - j0);
        const size_t base = (size_t)j0 * T, n_el = (size_t)nj * T;
        __syncthreads();                                  // the pair loop of the chunk before has read the arrays
        ColWalk w(T, tid);
        for (size_t e = tid; e < n_el; e += EVAL_R, w.next()) {
            const float s = scores[base + e], y = targets[base + e];
            const bool ok = valid[base + e] != 0;
            if (w.col == t) {
                const bool pos = ok && y == 1.0f, neg = ok && y == 0.0f;
                s_pos[w.row] = pos ? s : qnan;
                s_neg[w.row] = neg ? s : qnan;
                nP += pos;
                nN += neg;
                nBad += (pos || neg) && !isfinite(s);
            }
        }
        const int nj8 = (nj + 7) & ~7;                     // the pair loop takes eight entries per step
        if (nj + tid < nj8) s_pos[nj + tid] = s_neg[nj + tid] = qnan;
        __syncthreads();
        for (int j = 0; j < nj8; j += 8) {
            const float4 a0 = *reinterpret_cast<const float4*>(s_neg + j), a1 = *reinterpret_cast<const float4*>(s_neg + j + 4);
            const float4 b0 = *reinterpret_cast<const float4*>(s_pos + j), b1 = *reinterpret_cast<const float4*>(s_pos + j + 4);
            const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                neg_lt += a[u] < si ? 1u : 0u;
                neg_eq += a[u] == si ? 1u : 0u;
                pos_ge += b[u] >= si ? 1u : 0u;
            }
        }
    }
    // a split launch: the per-entry counts of this j range (zero on every lane that is no positive) go to the finalize, which adds
    // the ranges and forms the ratios
    if (nsplit > 1) counts[((size_t)(t * nsplit + split) * tiles + tile) * EVAL_R + tid] = make_uint2(pos_ge, neg_lt);
    const unsigned long long num = wave_sum(2ull * neg_lt + neg_eq);
    nP = (uint32_t)wave_sum((int)nP);
    nN = (uint32_t)wave_sum((int)nN);
    nBad = (uint32_t)wave_sum((int)nBad);
    if ((tid & 63) == 0) {
        s_num[tid >> 6] = num;
        s_cls[tid >> 6][0] = nP; s_cls[tid >> 6][1] = nN; s_cls[tid >> 6][2] = nBad;
    }
    __syncthreads();
    EvalSlot o = {};
    for (int k = 0; k < EVAL_R / WAVE; ++k) { o.num += s_num[k]; o.P += s_cls[k][0]; o.N += s_cls[k][1]; o.bad += s_cls[k][2]; }
    // not split: the lane has walked every row, its counts are complete and o.N is the task's N
    double ap = (nsplit == 1 && pos_ge) ? (double)pos_ge / ((double)pos_ge + ((double)o.N - (double)neg_lt)) : 0.0;
    ap = wave_sum(ap);
    if ((tid & 63) == 0) s_ap[tid >> 6] = ap;
    __syncthreads();
    if (tid == 0) {
        for (int k = 0; k < EVAL_R / WAVE; ++k) o.ap += s_ap[k];
        slots[(size_t)(t * nsplit + split) * tiles + tile] = o;
    }
}

// grid (tiles, T): sum d^2, sum |d| and the count over the valid entries of EVAL_R rows of one task, in fp64
__global__ __launch_bounds__(EVAL_R) void eval_sums_kernel(const float* __restrict__ scores, const float* __restrict__ targets,
                                                            const uint8_t* __restrict__ valid, int rows, int T,
                                                            EvalSums* __restrict__ slots) {
    __shared__ double s_part[EVAL_R / WAVE][3];
    const int tid = threadIdx.x, tile = blockIdx.x, t = blockIdx.y, tiles = gridDim.x;
    const int j0 = tile * EVAL_R, nj = min(EVAL_R, rows - j0);
    const size_t base = (size_t)j0 * T, n_el = (size_t)nj * T;
    double sse = 0.0, sae = 0.0, cnt = 0.0;
    ColWalk w(T, tid);
    for (size_t e = tid; e < n_el; e += EVAL_R, w.next()) {
        const double d = (double)scores[base + e] - (double)targets[base + e];
        if (w.col == t && valid[base + e]) {
            sse += d * d;
            sae += fabs(d);
            cnt += 1.0;
        }
    }
    sse = wave_sum(sse);
    sae = wave_sum(sae);
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0) { s_part[tid >> 6][0] = sse; s_part[tid >> 6][1] = sae; s_part[tid >> 6][2] = cnt; }
    __syncthreads();
    if (tid == 0) {
        EvalSums o = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < EVAL_R / WAVE; ++k) { o.sse += s_part[k][0]; o.sae += s_part[k][1]; o.cnt += s_part[k][2]; }
        slots[(size_t)t * tiles + tile] = o;
    }
}

// sum of one value per thread over the workgroup, in a fixed order (lanes by butterfly, waves in wave order); every thread gets it
template <typename V>
__device__ __forceinline__ V block_sum(V v, V* s_buf) {
    v = wave_sum(v);
    __syncthreads();                                      // s_buf may still be read from the sum before
    if ((threadIdx.x & 63) == 0) s_buf[threadIdx.x >> 6] = v;
    __syncthreads();
    V tot = 0;
    for (int k = 0; k < EVAL_FIN_THREADS / WAVE; ++k) tot += s_buf[k];
    return tot;
}

// One workgroup.  CLASS: out = [auc T | ap T | P T | N T | bad T | mean_auc | mean_ap]; a task without both classes or with a
// non-finite labelled score is NaN and stays out of the means.  else: out = [rmse T | mae T | count T | rmse_all | mae_all], the last
// two over the flattened outputs (train.py:211).
template <bool CLASS>
__global__ __launch_bounds__(EVAL_FIN_THREADS) void eval_finalize_kernel(const void* __restrict__ slots_, const uint2* __restrict__ counts,
                                                                          int rows, int T, int tiles, int nsplit,
                                                                          double* __restrict__ out) {
    __shared__ double s_d[EVAL_FIN_THREADS / WAVE];
    __shared__ unsigned long long s_u[EVAL_FIN_THREADS / WAVE];
    const int tid = threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double m0 = 0.0, m1 = 0.0, m2 = 0.0;                  // running sums over the tasks (thread 0 writes them)
    if (CLASS) {
        const EvalSlot* slots = static_cast<const EvalSlot*>(slots_);
        for (int t = 0; t < T; ++t) {
            const int nslot = nsplit * tiles;
            unsigned long long num = 0, pn = 0, bad = 0;     // pn: P in the high, N in the low half
            double ap = 0.0;
            for (int k = tid; k < nslot; k += EVAL_FIN_THREADS) {
                const EvalSlot o = slots[(size_t)t * nslot + k];
                num += o.num;
                ap += o.ap;
                if (k % tiles == 0) {                        // a j range is counted by every tile: take it from the first
                    pn += ((unsigned long long)o.P << 32) | o.N;
                    bad += o.bad;
                }
            }
            num = block_sum(num, s_u);
            pn = block_sum(pn, s_u);
            bad = block_sum(bad, s_u);
            const double P = (double)(pn >> 32), N = (double)(pn & 0xffffffffull);
            if (nsplit > 1) {                                // (the slots' ap is zero: the ratios need the counts of all ranges)
                for (int r = tid; r < rows; r += EVAL_FIN_THREADS) {
                    uint32_t pg = 0, nl = 0;
                    for (int s = 0; s < nsplit; ++s) {
                        const uint2 c = counts[(size_t)(t * nsplit + s) * tiles * EVAL_R + r];
                        pg += c.x;
                        nl += c.y;
                    }
                    if (pg) ap += (double)pg / ((double)pg + (N - (double)nl));
                }
            }
            ap = block_sum(ap, s_d);
            if (tid == 0) {
                const bool ok = P > 0.0 && N > 0.0 && bad == 0;
                const double auc = ok ? (double)num / (2.0 * P * N) : nan;
                out[t] = auc;
                out[T + t] = ok ? ap / P : nan;
                out[2 * T + t] = P;
                out[3 * T + t] = N;
                out[4 * T + t] = (double)bad;
                if (ok) { m0 += auc; m1 += ap / P; m2 += 1.0; }
            }
        }
        if (tid == 0) {
            out[5 * T] = m2 > 0.0 ? m0 / m2 : nan;
            out[5 * T + 1] = m2 > 0.0 ? m1 / m2 : nan;
        }
    } else {
        const EvalSums* slots = static_cast<const EvalSums*>(slots_);
        for (int t = 0; t < T; ++t) {
            double sse = 0.0, sae = 0.0, cnt = 0.0;
            for (int k = tid; k < tiles; k += EVAL_FIN_THREADS) {
                const EvalSums o = slots[(size_t)t * tiles + k];
                sse += o.sse;
                sae += o.sae;
                cnt += o.cnt;
            }
            sse = block_sum(sse, s_d);
            sae = block_sum(sae, s_d);
            cnt = block_sum(cnt, s_d);
            if (tid == 0) {
                out[t] = cnt > 0.0 ? sqrt(sse / cnt) : nan;
                out[T + t] = cnt > 0.0 ? sae / cnt : nan;
                out[2 * T + t] = cnt;
                m0 += sse; m1 += sae; m2 += cnt;
            }
        }
        if (tid == 0) {
            out[3 * T] = m2 > 0.0 ? sqrt(m0 / m2) : nan;
            out[3 * T + 1] = m2 > 0.0 ? m1 / m2 : nan;
        }
    }
}

static int eval_check(const char* fn, const float* scores, const float* targets, const uint8_t* valid, int64_t rows, int T,
                      const void* workspace, size_t workspace_bytes, const double* out) {
    EAGCN_CHECK_ARG(scores, "%s: scores is null", fn);
    EAGCN_CHECK_ARG(targets, "%s: targets is null", fn);
    EAGCN_CHECK_ARG(valid, "%s: valid is null", fn);
    EAGCN_CHECK_ARG(workspace, "%s: workspace is null", fn);
    EAGCN_CHECK_ARG(out, "%s: out is null", fn);
    EAGCN_CHECK_ARG(rows >= 1, "%s: rows = %lld, an evaluation needs at least one", fn, (long long)rows);
    EAGCN_CHECK_ARG(T >= 1 && T <= 65535, "%s: T = %d is not in 1 .. 65535", fn, T);
    EAGCN_CHECK_ARG(rows < (int64_t(1) << 31), "%s: rows = %lld does not fit the 32-bit counters (rows < 2^31)", fn, (long long)rows);
    EAGCN_CHECK_ARG(eval_tiles(rows) * T < (int64_t(1) << 31), "%s: rows x T = %lld x %d is more than one launch takes", fn,
                    (long long)rows, T);
    EAGCN_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "%s: workspace must be 8-byte aligned", fn);
    EAGCN_CHECK_ARG(workspace_bytes >= eval_workspace_bytes(rows, T), "%s: workspace too small (%zu < %zu bytes)", fn, workspace_bytes,
                    eval_workspace_bytes(rows, T));
    return EAGCN_OK;
}

}  // namespace eagcn

using namespace eagcn;

extern "C" size_t eagcn_eval_metrics_workspace_bytes(int64_t rows, int T) {
    return rows < 1 || T < 1 ? 0 : eval_workspace_bytes(rows, T);
}

extern "C" int eagcn_eval_class_metrics(const float* scores, const float* targets, const uint8_t* valid, int64_t rows, int T,
                                        void* workspace, size_t workspace_bytes, double* out, void* stream) {
    if (int rc = eval_check("eagcn_eval_class_metrics", scores, targets, valid, rows, T, workspace, workspace_bytes, out)) return rc;
    int nsplit, per;
    eval_split(rows, T, &nsplit, &per);
    const int tiles = (int)eval_tiles(rows);
    uint2* counts = static_cast<uint2*>(workspace);
    EvalSlot* slots = reinterpret_cast<EvalSlot*>(counts + (size_t)T * nsplit * tiles * EVAL_R);
    eval_rank_kernel<<<dim3(tiles, nsplit, T), EVAL_R, 0, (hipStream_t)stream>>>(scores, targets, valid, (int)rows, T, per, counts, slots);
    EAGCN_LAUNCH_CHECK();
    eval_finalize_kernel<true><<<1, EVAL_FIN_THREADS, 0, (hipStream_t)stream>>>(slots, counts, (int)rows, T, tiles, nsplit, out);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

extern "C" int eagcn_eval_reg_metrics(const float* scores, const float* targets, const uint8_t* valid, int64_t rows, int T,
                                      void* workspace, size_t workspace_bytes, double* out, void* stream) {
    if (int rc = eval_check("eagcn_eval_reg_metrics", scores, targets, valid, rows, T, workspace, workspace_bytes, out)) return rc;
    const int tiles = (int)eval_tiles(rows);
    EvalSums* slots = static_cast<EvalSums*>(workspace);
    eval_sums_kernel<<<dim3(tiles, T), EVAL_R, 0, (hipStream_t)stream>>>(scores, targets, valid, (int)rows, T, slots);
    EAGCN_LAUNCH_CHECK();
    eval_finalize_kernel<false><<<1, EVAL_FIN_THREADS, 0, (hipStream_t)stream>>>(slots, nullptr, (int)rows, T, tiles, 1, out);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}
