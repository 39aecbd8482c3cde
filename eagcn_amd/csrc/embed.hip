// Two-dimensional embeddings of the dumped representations (the reference's tsnes.py / mol_to_vec_plot.py: PCA and t-SNE), on the device.
// Semantics in include/eagcn_hip.h; no floating-point atomics, every sum folded in a fixed order: runs are bit-identical.
//
//   eagcn_sqdist            D = direct sums of (x_i - x_j)^2 over 64 x 64 output tiles staged through LDS (EM_KC columns at a time, the
//                           tiles transposed on their way in so that a thread's four rows are one 16-byte LDS read).  Only the tiles on or
//                           above the diagonal are computed; each is stored twice: D is symmetric to the bit, its diagonal exactly zero.
//   eagcn_tsne_affinities   ts_search_kernel: one workgroup per row bisects the row's precision in fp64 on the fp32 distances (the row is
//                           re-read from L2 every step); ts_joint_kernel: (P_cond + P_cond^T) / sum by tile pairs, the mirror tile through LDS.
//   eagcn_tsne_gradient /   ts_pair_kernel, the hot one: a workgroup owns TS_ROWS rows and walks P's columns TS_CHUNK at a time -- thread t
//   eagcn_tsne_iterate      holds the embedding of columns 4t .. 4t+3 of the chunk in registers (two 16-byte loads from L2) and one float4
//                           of P per row, the next chunk's eight loads in flight while this one is worked on.  Five fp32 sums per row
//                           (a, r, z), folded over the lanes, then over the waves in wave order.  ts_kl_kernel: the divergence's part that
//                           depends on the embedding, in fp64, on check iterations only.  ts_row_kernel: Z from the workgroups' partials, the
//                           gradient, scikit-learn's update rule; ts_decide_kernel (one wave): schedule and stop rule.
//   eagcn_pca_cov / project fp64 column means from per-workgroup slabs, the covariance from 64 x 64 tiles of centred rows (fp32 products
//                           over 256 rows, then fp64; row slabs added in slab order), the projection one wave per row.
#include <float.h>

#include "common.h"

namespace eagcn {

constexpr int EM_TILE = 64;          // rows (and columns) of an output tile of the distance, joint-probability and covariance kernels
constexpr int EM_KC = 32;            // feature columns (covariance: rows) staged per step
constexpr int EM_THREADS = 256;
constexpr int EM_PADT = EM_TILE + 4; // LDS row of a transposed tile: 16-byte aligned rows
constexpr int EM_MAX_F = 1024;
constexpr int EM_MIN_N = 17;
constexpr int EM_MAX_N = 32768;
constexpr int EM_MAX_K = 8;          // PCA components
constexpr int EM_COL_WGS = 768;      // workgroups (= slabs) of the column-sum pass
constexpr int EM_COL_ROWS = 64;      // rows of the chunk such a workgroup takes at a time
constexpr int EM_COV_SLABS = 16;     // row slabs of the covariance at the most
constexpr int EM_COV_FLUSH = 8;      // steps of EM_KC rows between two flushes of the fp32 tile sums into fp64
constexpr int TS_ROWS = 8;           // rows of P a workgroup of the gradient pass owns
constexpr int TS_CHUNK = 4 * EM_THREADS;   // columns of P it walks at a time: one float4 per thread and row
constexpr int TS_EXPLORE = 250;      // iterations of the early-exaggeration stage (scikit-learn's _EXPLORATION_MAX_ITER)
constexpr int TS_CHECK = 50;         // the stop rule is evaluated every TS_CHECK-th iteration (_N_ITER_CHECK)
constexpr int TS_SEARCH_STEPS = 100;
constexpr double TS_PERP_TOL = 1e-5;
constexpr double TS_ZERO_SUM = 1e-8;
static_assert(EM_TILE * EM_TILE == 16 * EM_THREADS, "a thread holds a 4 x 4 block of an output tile");

struct TsState {                     // the first 64 bytes of the t-SNE workspace (eagcn_hip.h)
    int32_t done, n_iter, reason, best_iter;
    double best_err, last_kl, last_gnorm;
    float exag, lr;
    int32_t max_iter, nwp;
    double min_gn;
};
static_assert(sizeof(TsState) == 64, "eagcn_hip.h documents a 64-byte state block");

struct TsWs {                        // the workspace, cut up (every part 256-byte aligned)
    TsState* st; float* Y; float* U; float* gains; float* A; float* R; float* z; double* klrows; float* grad; double* prow;
    double* zpart; double* parts; double* consts;
    int G, W; size_t bytes;
};
// consts: [0..1] S1, S3 at the early exaggeration, [2..3] at alpha = 1, [4..5] of a stand-alone call, [6] Z of the last pass
static inline TsWs ts_layout(void* base, int64_t n) {
    TsWs w;
    char* p = static_cast<char*>(base);
    size_t o = 0;
    auto take = [&](size_t bytes) { char* q = p + o; o += align256(bytes); return q; };
    w.G = (int)((n + TS_ROWS - 1) / TS_ROWS);
    w.W = (int)((n + EM_THREADS - 1) / EM_THREADS);
    w.st = reinterpret_cast<TsState*>(take(256));
    w.Y = reinterpret_cast<float*>(take((size_t)n * 8));
    w.U = reinterpret_cast<float*>(take((size_t)n * 8));
    w.gains = reinterpret_cast<float*>(take((size_t)n * 8));
    w.A = reinterpret_cast<float*>(take((size_t)n * 8));
    w.R = reinterpret_cast<float*>(take((size_t)n * 8));
    w.z = reinterpret_cast<float*>(take((size_t)n * 4));
    w.klrows = reinterpret_cast<double*>(take((size_t)n * 8));
    w.grad = reinterpret_cast<float*>(take((size_t)n * 8));
    w.prow = reinterpret_cast<double*>(take((size_t)n * 16));
    w.zpart = reinterpret_cast<double*>(take((size_t)w.G * 8));
    w.parts = reinterpret_cast<double*>(take((size_t)w.W * 16));
    w.consts = reinterpret_cast<double*>(take(256));
    w.bytes = o;
    return w;
}

// the sum over the workgroup of one double per thread: lanes by butterfly, then the four waves in wave order -- the same bits in every thread
__device__ __forceinline__ double em_block_sum(double v, double* s_w /* [4] */) {
    v = wave_sum(v);
    __syncthreads();                                       // (s_w may still be read from the sum before)
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// ---- pairwise squared distances --------------------------------------------------------------------------------------------------
// grid (nt, nt), nt = ceil(n / 64); the blocks below the diagonal return at once
__global__ __launch_bounds__(EM_THREADS) void em_sqdist_kernel(const float* __restrict__ X, int n, int F, int ld, float* __restrict__ D) {
    __shared__ __attribute__((aligned(16))) float sA[EM_KC][EM_PADT];
    __shared__ __attribute__((aligned(16))) float sB[EM_KC][EM_PADT];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lc = tid & 31, lr = tid >> 5;
    const int i0 = bi * EM_TILE, j0 = bj * EM_TILE;
    float acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0f;
    for (int c0 = 0; c0 < F; c0 += EM_KC) {
        const int c = c0 + lc;
#pragma unroll
        for (int u = 0; u < EM_TILE / 8; ++u) {
            const int r = lr + 8 * u, ra = i0 + r, rb = j0 + r;
            sA[lc][r] = (ra < n && c < F) ? X[(size_t)ra * ld + c] : 0.0f;
            sB[lc][r] = (rb < n && c < F) ? X[(size_t)rb * ld + c] : 0.0f;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < EM_KC; ++k) {
            const float4 a4 = *reinterpret_cast<const float4*>(&sA[k][ty * 4]);
            const float4 b4 = *reinterpret_cast<const float4*>(&sB[k][tx * 4]);
            const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float d = a[u] - b[v];
                    acc[u][v] = fmaf(d, d, acc[u][v]);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int i = i0 + ty * 4 + u, j = j0 + tx * 4 + v;
            if (i < n && j < n) {
                D[(size_t)i * n + j] = acc[u][v];
                if (bi != bj) D[(size_t)j * n + i] = acc[u][v];
            }
        }
}

// ---- affinities --------------------------------------------------------------------------------------------------------------------
// grid n: scikit-learn's _binary_search_perplexity for row blockIdx.x, in fp64.  beta: the precision of the last evaluation, srow: its
// row sum (1e-8 where it was zero), rs: the sum of the row's conditional probabilities, steps: evaluations made
__global__ __launch_bounds__(EM_THREADS) void ts_search_kernel(const float* __restrict__ D, int n, double log_perp, double* __restrict__ beta_out,
                                                               double* __restrict__ srow, double* __restrict__ rs, int32_t* __restrict__ steps) {
    __shared__ double s_p[2][EM_THREADS / WAVE][2];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* __restrict__ row = D + (size_t)i * n;
    double beta = 1.0, bmin = -INFINITY, bmax = INFINITY, beval = 1.0, sum_p = 1.0, raw = 0.0;
    int step = 0;
    while (step < TS_SEARCH_STEPS) {
        double sp = 0.0, sd = 0.0;
        for (int j = tid; j < n; j += EM_THREADS) {
            if (j != i) {
                const double d = (double)row[j], p = exp(-d * beta);
                sp += p;
                sd += d * p;
            }
        }
        sp = wave_sum(sp);
        sd = wave_sum(sd);
        if (lane == 0) { s_p[step & 1][wave][0] = sp; s_p[step & 1][wave][1] = sd; }
        __syncthreads();                                   // (the buffers alternate: one barrier per step)
        sp = ((s_p[step & 1][0][0] + s_p[step & 1][1][0]) + s_p[step & 1][2][0]) + s_p[step & 1][3][0];
        sd = ((s_p[step & 1][0][1] + s_p[step & 1][1][1]) + s_p[step & 1][2][1]) + s_p[step & 1][3][1];
        raw = sp;
        if (sp == 0.0) sp = TS_ZERO_SUM;
        sum_p = sp;
        beval = beta;
        ++step;
        const double diff = log(sp) + beta * (sd / sp) - log_perp;
        if (fabs(diff) <= TS_PERP_TOL) break;
        if (diff > 0.0) {
            bmin = beta;
            beta = bmax == INFINITY ? beta * 2.0 : (beta + bmax) / 2.0;
        } else {
            bmax = beta;
            beta = bmin == -INFINITY ? beta / 2.0 : (beta + bmin) / 2.0;
        }
    }
    if (tid == 0) {
        beta_out[i] = beval;
        srow[i] = sum_p;
        rs[i] = raw / sum_p;
        if (steps) steps[i] = step;
    }
}

// one workgroup: out[q] = scale * sum_i v[i * stride + q], q < nq <= 2, thread-strided in index order, then em_block_sum
__global__ __launch_bounds__(EM_THREADS) void em_sum_kernel(const double* __restrict__ v, int m, int stride, int nq, double scale,
                                                            double* __restrict__ out) {
    __shared__ double s_w[EM_THREADS / WAVE];
    for (int q = 0; q < nq; ++q) {
        double a = 0.0;
        for (int i = threadIdx.x; i < m; i += EM_THREADS) a += v[(size_t)i * stride + q];
        a = em_block_sum(a, s_w);
        if (threadIdx.x == 0) out[q] = scale * a;
    }
}

// grid (nt, nt), blocks below the diagonal return: P = max((C + C^T) / total, DBL_EPSILON) off the diagonal, C_ij = exp(-D_ij beta_i) / s_i,
// for the tile (bi, bj) and its mirror; the columns n .. ldp - 1 of every row are zeroed
__global__ __launch_bounds__(EM_THREADS) void ts_joint_kernel(const float* __restrict__ D, int n, int ldp, const double* __restrict__ beta,
                                                              const double* __restrict__ srow, const double* __restrict__ total,
                                                              float* __restrict__ P) {
    __shared__ double s_c2[EM_TILE][EM_TILE + 1];
    __shared__ float s_out[EM_TILE][EM_TILE + 1];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;
    const int tid = threadIdx.x, i0 = bi * EM_TILE, j0 = bj * EM_TILE;
    const double tot = fmax(*total, DBL_EPSILON);
    for (int e = tid; e < EM_TILE * EM_TILE; e += EM_THREADS) {
        const int r = e >> 6, c = e & 63, gr = j0 + r, gc = i0 + c;
        double v = 0.0;
        if (gr < n && gc < n && gr != gc) v = exp(-(double)D[(size_t)gr * n + gc] * beta[gr]) / srow[gr];
        s_c2[r][c] = v;
    }
    __syncthreads();
    for (int e = tid; e < EM_TILE * EM_TILE; e += EM_THREADS) {
        const int r = e >> 6, c = e & 63, gr = i0 + r, gc = j0 + c;
        float o = 0.0f;
        if (gr < n && gc < n && gr != gc) {
            const double v = exp(-(double)D[(size_t)gr * n + gc] * beta[gr]) / srow[gr] + s_c2[c][r];
            o = (float)fmax(v / tot, DBL_EPSILON);
        }
        if (gr < n && gc < ldp) P[(size_t)gr * ldp + gc] = o;
        s_out[r][c] = o;
    }
    if (bi == bj) return;
    __syncthreads();
    for (int e = tid; e < EM_TILE * EM_TILE; e += EM_THREADS) {
        const int r = e >> 6, c = e & 63, gr = j0 + r, gc = i0 + c;
        if (gr < n && gc < n) P[(size_t)gr * ldp + gc] = s_out[c][r];
    }
}

// ---- the gradient pass -----------------------------------------------------------------------------------------------------------
// grid n: per row the two sums of the divergence that do not depend on the embedding, in fp64:
//   prow[2 i] = sum_j q log max(q, eps), prow[2 i + 1] = sum_j q, q = alpha P_ij over j != i
__global__ __launch_bounds__(EM_THREADS) void ts_pstat_kernel(const float* __restrict__ P, int n, int ldp, float alpha, double* __restrict__ prow) {
    __shared__ double s_w[EM_THREADS / WAVE];
    const int i = blockIdx.x;
    const float* __restrict__ row = P + (size_t)i * ldp;
    double s1 = 0.0, s3 = 0.0;
    for (int j = 4 * threadIdx.x; j < n; j += TS_CHUNK) {
        const float4 p = *reinterpret_cast<const float4*>(row + j);
        const float pv[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double q = j + e < n && j + e != i ? (double)(alpha * pv[e]) : 0.0;
            s1 += q * log(fmax(q, DBL_EPSILON));
            s3 += q;
        }
    }
    s1 = em_block_sum(s1, s_w);
    s3 = em_block_sum(s3, s_w);
    if (threadIdx.x == 0) { prow[2 * i] = s1; prow[2 * i + 1] = s3; }
}

// one pair term of one row.  MASK: the chunk holds the row's own column or columns beyond n; they get w = 0
template <bool MASK>
__device__ __forceinline__ void ts_term(float pv, float yjx, float yjy, float yix, float yiy, bool valid, float alpha, float (&a)[5]) {
    const float dx = yix - yjx, dy = yiy - yjy;
    const float d2 = fmaf(dy, dy, dx * dx);
    float w = __builtin_amdgcn_rcpf(1.0f + d2);
    if (MASK) w = valid ? w : 0.0f;
    const float q = alpha * pv, pw = q * w, w2 = w * w;
    a[0] = fmaf(pw, dx, a[0]);
    a[1] = fmaf(pw, dy, a[1]);
    a[2] = fmaf(w2, dx, a[2]);
    a[3] = fmaf(w2, dy, a[3]);
    a[4] += w;
}

__device__ __forceinline__ void ts_pair_body(const float* __restrict__ P, int ldp, const float* __restrict__ Y, int n, float alpha,
                                             float* __restrict__ A, float* __restrict__ R, float* __restrict__ z,
                                             double* __restrict__ zpart, float (*s_red)[TS_ROWS * 5]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r0 = blockIdx.x * TS_ROWS;
    float yix[TS_ROWS], yiy[TS_ROWS], acc[TS_ROWS][5];
    size_t off[TS_ROWS];
#pragma unroll
    for (int r = 0; r < TS_ROWS; ++r) {
        const int row = min(r0 + r, n - 1);                // (a row beyond n repeats the last one; it is not stored)
        yix[r] = Y[2 * row];
        yiy[r] = Y[2 * row + 1];
        off[r] = (size_t)row * ldp;
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[r][q] = 0.0f;
    }
    // columns beyond pad4(n) are never read; TS_CHUNK % TS_ROWS == 0: one chunk holds all own columns
    const int n4 = (n + 3) & ~3, nchunks = (n4 + TS_CHUNK - 1) / TS_CHUNK, own = r0 / TS_CHUNK;
    auto load = [&](float4 (&p)[TS_ROWS], int c) {
        const int j = c * TS_CHUNK + 4 * tid;
#pragma unroll
        for (int r = 0; r < TS_ROWS; ++r)
            p[r] = j < n4 ? *reinterpret_cast<const float4*>(P + off[r] + j) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    float4 p[TS_ROWS], pn[TS_ROWS];
    load(p, 0);
    for (int c = 0; c < nchunks; ++c) {
        const int j = c * TS_CHUNK + 4 * tid;
        if (c + 1 < nchunks) load(pn, c + 1);              // the next chunk streams in while this one is worked on
        float yj[8];
        if (j + 4 <= n) {
            const float4 y0 = *reinterpret_cast<const float4*>(Y + 2 * j), y1 = *reinterpret_cast<const float4*>(Y + 2 * j + 4);
            yj[0] = y0.x; yj[1] = y0.y; yj[2] = y0.z; yj[3] = y0.w;
            yj[4] = y1.x; yj[5] = y1.y; yj[6] = y1.z; yj[7] = y1.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                yj[2 * e] = j + e < n ? Y[2 * (j + e)] : 0.0f;
                yj[2 * e + 1] = j + e < n ? Y[2 * (j + e) + 1] : 0.0f;
            }
        }
        if (c == own || c == nchunks - 1) {
#pragma unroll
            for (int r = 0; r < TS_ROWS; ++r) {
                const float pv[4] = {p[r].x, p[r].y, p[r].z, p[r].w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    ts_term<true>(pv[e], yj[2 * e], yj[2 * e + 1], yix[r], yiy[r], j + e < n && j + e != r0 + r, alpha, acc[r]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < TS_ROWS; ++r) {
                const float pv[4] = {p[r].x, p[r].y, p[r].z, p[r].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) ts_term<false>(pv[e], yj[2 * e], yj[2 * e + 1], yix[r], yiy[r], true, alpha, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < TS_ROWS; ++r) p[r] = pn[r];
    }
#pragma unroll
    for (int r = 0; r < TS_ROWS; ++r) {
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const float t = wave_sum(acc[r][q]);
            if (lane == 0) s_red[wave][r * 5 + q] = t;
        }
    }
    __syncthreads();
    if (tid < TS_ROWS * 5) {
        const float v = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
        const int r = tid / 5, q = tid - 5 * r, row = r0 + r;
        if (row < n) {
            if (q < 2) A[2 * row + q] = v;
            else if (q < 4) R[2 * row + q - 2] = v;
            else z[row] = v;
        }
    }
    if (tid == 0) {
        double zp = 0.0;
        for (int r = 0; r < TS_ROWS && r0 + r < n; ++r) {
            const int q = r * 5 + 4;
            zp += (double)(((s_red[0][q] + s_red[1][q]) + s_red[2][q]) + s_red[3][q]);
        }
        zpart[blockIdx.x] = zp;
    }
}

// grid ceil(n / TS_ROWS).  st: the driver's state (the launch returns at once when it is done; alpha comes from n_iter), or null with
// alpha_h from the host
__global__ __launch_bounds__(EM_THREADS) void ts_pair_kernel(const float* __restrict__ P, int ldp, const float* __restrict__ Y, int n,
                                                             const TsState* __restrict__ st, float alpha_h, float* __restrict__ A,
                                                             float* __restrict__ R, float* __restrict__ z, double* __restrict__ zpart) {
    __shared__ float s_red[EM_THREADS / WAVE][TS_ROWS * 5];
    float alpha = alpha_h;
    if (st) {
        if (st->done) return;
        alpha = st->n_iter < TS_EXPLORE ? st->exag : 1.0f;
    }
    ts_pair_body(P, ldp, Y, n, alpha, A, R, z, zpart, s_red);
}

// grid n, on check iterations only (with st the launch returns at once on every other one): the embedding's part of the divergence,
// klrows[i] = sum_{j != i} q log(1 + |y_i - y_j|^2) = -sum q log w, q = alpha P_ij, in fp64 -- a second read of P every 50th iteration,
// kept out of the hot kernel, whose registers the fp64 logarithm would take
__global__ __launch_bounds__(EM_THREADS) void ts_kl_kernel(const float* __restrict__ P, int ldp, const float* __restrict__ Y, int n,
                                                           const TsState* __restrict__ st, float alpha_h, double* __restrict__ klrows) {
    __shared__ double s_w[EM_THREADS / WAVE];
    float alpha = alpha_h;
    if (st) {
        if (st->done) return;
        const int it = st->n_iter;
        if ((it + 1) % TS_CHECK != 0) return;
        alpha = it < TS_EXPLORE ? st->exag : 1.0f;
    }
    const int i = blockIdx.x;
    const float* __restrict__ row = P + (size_t)i * ldp;
    const float yix = Y[2 * i], yiy = Y[2 * i + 1];
    double s2 = 0.0;
    for (int j = 4 * threadIdx.x; j < n; j += TS_CHUNK) {
        const float4 p = *reinterpret_cast<const float4*>(row + j);
        const float pv[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (j + e < n && j + e != i) {
                const float dx = yix - Y[2 * (j + e)], dy = yiy - Y[2 * (j + e) + 1];
                s2 += (double)(alpha * pv[e]) * log1p((double)fmaf(dy, dy, dx * dx));
            }
        }
    }
    s2 = em_block_sum(s2, s_w);
    if (threadIdx.x == 0) klrows[i] = s2;
}

// grid W = ceil(n / 256), one thread per row: Z = the sum of the G partials (the same fixed order in every workgroup),
// grad = 4 (a - r / Z); UPDATE: scikit-learn's _gradient_descent step on (Y, update, gains), else the gradient is stored.
// parts[2 w] = this workgroup's sum of squares of the (UPDATE: gained) gradient, parts[2 w + 1] = of klrows; consts[6] = Z
template <bool UPDATE>
__global__ __launch_bounds__(EM_THREADS) void ts_row_kernel(const TsState* __restrict__ st, int n, int G, const double* __restrict__ zpart,
                                                            const float* __restrict__ A, const float* __restrict__ R, float* __restrict__ Y,
                                                            float* __restrict__ U, float* __restrict__ gains, float* __restrict__ grad,
                                                            const double* __restrict__ klrows, int kl_h, double* __restrict__ parts,
                                                            double* __restrict__ consts) {
    __shared__ double s_w[EM_THREADS / WAVE];
    if (UPDATE && st->done) return;
    const int tid = threadIdx.x, i = blockIdx.x * EM_THREADS + tid;
    const int it = UPDATE ? st->n_iter : 0;
    const bool kl = UPDATE ? (it + 1) % TS_CHECK == 0 : kl_h != 0;
    double zs = 0.0;
    for (int g = tid; g < G; g += EM_THREADS) zs += zpart[g];
    const double Z = em_block_sum(zs, s_w);
    double gn = 0.0, k = 0.0;
    if (i < n) {
        const float inv = (float)(1.0 / Z);
        float g[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) g[q] = 4.0f * fmaf(-R[2 * i + q], inv, A[2 * i + q]);    // (one form in both instantiations)
        if (UPDATE) {
            const float mom = it < TS_EXPLORE ? 0.5f : 0.8f, lr = st->lr;
            const bool fresh = it == TS_EXPLORE;           // the second stage starts from update = 0, gains = 1
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float u = fresh ? 0.0f : U[2 * i + q];
                float gain = fresh ? 1.0f : gains[2 * i + q];
                gain = __fmul_rn(u, g[q]) < 0.0f ? __fadd_rn(gain, 0.2f) : __fmul_rn(gain, 0.8f);
                gain = fmaxf(gain, 0.01f);
                const float gg = __fmul_rn(g[q], gain);
                const float un = __fsub_rn(__fmul_rn(mom, u), __fmul_rn(lr, gg));
                gains[2 * i + q] = gain;
                U[2 * i + q] = un;
                Y[2 * i + q] = __fadd_rn(Y[2 * i + q], un);
                gn += (double)gg * (double)gg;
            }
        } else {
            grad[2 * i] = g[0];
            grad[2 * i + 1] = g[1];
            gn = (double)g[0] * (double)g[0] + (double)g[1] * (double)g[1];
        }
        if (kl) k = klrows[i];
    }
    gn = em_block_sum(gn, s_w);
    k = em_block_sum(k, s_w);
    if (tid == 0) {
        parts[2 * blockIdx.x] = gn;
        parts[2 * blockIdx.x + 1] = k;
        if (blockIdx.x == 0) consts[6] = Z;
    }
}

__device__ __forceinline__ double ts_wave_total(const double* __restrict__ v, int m, int stride) {
    double a = 0.0;
    for (int i = threadIdx.x; i < m; i += WAVE) a += v[(size_t)i * stride];
    return wave_sum(a);
}

// one wave.  mode 0: the bookkeeping of an iteration, the schedule and the stop rule; mode 1: out = {Z, KL, |grad|} of a stand-alone
// gradient pass (pc = its S1, S3); mode 2: the divergence of the final embedding into the state
__global__ __launch_bounds__(WAVE) void ts_decide_kernel(TsState* __restrict__ st, int mode, int W, const double* __restrict__ parts,
                                                         const double* __restrict__ consts, int pc, double* __restrict__ out) {
    if (mode == 0 && st->done) return;
    const double gn2 = ts_wave_total(parts, W, 2), s2 = ts_wave_total(parts + 1, W, 2);
    if (threadIdx.x != 0) return;
    const double Z = consts[6];
    if (mode != 0) {
        const double kl = pc < 0 ? (double)NAN : consts[pc] + s2 + log(Z) * consts[pc + 1];
        if (mode == 1) { out[0] = Z; out[1] = kl; out[2] = sqrt(gn2); }
        else st->last_kl = kl;
        return;
    }
    const int it = st->n_iter;
    const bool early = it < TS_EXPLORE;
    int done = 0, reason = 0;
    if (it == TS_EXPLORE) { st->best_err = DBL_MAX; st->best_iter = it; }
    if ((it + 1) % TS_CHECK == 0) {
        const int q = early ? 0 : 2;
        const double kl = consts[q] + s2 + log(Z) * consts[q + 1], gnorm = sqrt(gn2);
        st->last_kl = kl;
        st->last_gnorm = gnorm;
        if (kl < st->best_err) { st->best_err = kl; st->best_iter = it; }
        else if (it - st->best_iter > (early ? TS_EXPLORE : st->nwp)) { done = 1; reason = EAGCN_TSNE_STOP_NO_PROGRESS; }
        if (!done && gnorm <= st->min_gn) { done = 1; reason = EAGCN_TSNE_STOP_GRAD_NORM; }
    }
    st->n_iter = it + 1;
    if (!done && it + 1 >= st->max_iter) { done = 1; reason = EAGCN_TSNE_STOP_MAX_ITER; }
    if (done) { st->reason = reason; st->done = 1; }
}

// grid W: update = 0, gains = 1; thread 0 of block 0 writes the state
__global__ __launch_bounds__(EM_THREADS) void ts_begin_kernel(TsState* __restrict__ st, int n, float* __restrict__ U, float* __restrict__ gains,
                                                              float exag, float lr, int max_iter, int nwp, double min_gn) {
    const int i = blockIdx.x * EM_THREADS + threadIdx.x;
    if (i < n) {
        U[2 * i] = U[2 * i + 1] = 0.0f;
        gains[2 * i] = gains[2 * i + 1] = 1.0f;
    }
    if (i == 0) {
        st->done = max_iter <= 0;
        st->n_iter = 0;
        st->reason = max_iter <= 0 ? EAGCN_TSNE_STOP_MAX_ITER : 0;
        st->best_iter = 0;
        st->best_err = DBL_MAX;
        st->last_kl = 0.0;
        st->last_gnorm = 0.0;
        st->exag = exag; st->lr = lr; st->max_iter = max_iter; st->nwp = nwp; st->min_gn = min_gn;
    }
}

// ---- PCA ---------------------------------------------------------------------------------------------------------------------------
// grid G: per workgroup and column the fp64 sum over its chunks of EM_COL_ROWS rows -> slabs [g][F4] (thread t: columns 4t .. 4t+3)
__global__ __launch_bounds__(EM_THREADS) void em_colsum_kernel(const float* __restrict__ X, int n, int F, int ld, double* __restrict__ slabs) {
    const int tid = threadIdx.x, F4 = (F + 3) & ~3, col = 4 * tid;
    if (col >= F4) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const int chunks = (n + EM_COL_ROWS - 1) / EM_COL_ROWS;
    for (int chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int r1 = min(n, (chunk + 1) * EM_COL_ROWS);
        for (int r0 = chunk * EM_COL_ROWS; r0 < r1; r0 += 8) {
            float x[8][4];
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int u = 0; u < 4; ++u) x[r][u] = (r0 + r < r1 && col + u < F) ? X[(size_t)(r0 + r) * ld + col + u] : 0.0f;
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int u = 0; u < 4; ++u) s[u] += (double)x[r][u];
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) slabs[(size_t)blockIdx.x * F4 + col + u] = s[u];
}

// grid ceil(F / 256): mean[j] = the slabs' sums in slab order / n
__global__ __launch_bounds__(EM_THREADS) void em_mean_kernel(int n, int F, int G, const double* __restrict__ slabs, double* __restrict__ mean) {
    const int j = blockIdx.x * EM_THREADS + threadIdx.x, F4 = (F + 3) & ~3;
    if (j >= F) return;
    double a = 0.0;
    for (int g = 0; g < G; ++g) a += slabs[(size_t)g * F4 + j];
    mean[j] = a / (double)n;
}

__device__ __forceinline__ void em_tile_pair(int t, int nt, int& bi, int& bj) {     // the t-th tile on or above the diagonal, row by row
    bi = 0;
    while (t >= nt - bi) { t -= nt - bi; ++bi; }
    bj = bi + t;
}

// grid (ntp, S): the 64 x 64 tile blockIdx.x of (X - mean)^T (X - mean) over row slab blockIdx.y -> tiles [s][t][64][64] fp64
__global__ __launch_bounds__(EM_THREADS) void em_cov_kernel(const float* __restrict__ X, int n, int F, int ld, const double* __restrict__ mean,
                                                            int nt, int per, double* __restrict__ tiles) {
    __shared__ __attribute__((aligned(16))) float sA[EM_KC][EM_TILE];
    __shared__ __attribute__((aligned(16))) float sB[EM_KC][EM_TILE];
    int bi, bj;
    em_tile_pair(blockIdx.x, nt, bi, bj);
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lc = tid & 63, lr = tid >> 6;
    const int a0 = bi * EM_TILE, b0 = bj * EM_TILE;
    const int rbeg = min(n, (int)blockIdx.y * per), rend = min(n, rbeg + per);
    const bool oka = a0 + lc < F, okb = b0 + lc < F;
    const double ma = oka ? mean[a0 + lc] : 0.0, mb = okb ? mean[b0 + lc] : 0.0;
    float acc[4][4];
    double dacc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) { acc[u][v] = 0.0f; dacc[u][v] = 0.0; }
    int since = 0;
    for (int rc = rbeg; rc < rend; rc += EM_KC) {
#pragma unroll
        for (int u = 0; u < EM_KC / 4; ++u) {
            const int k = lr + 4 * u, row = rc + k;
            const bool in = row < rend;
            sA[k][lc] = (in && oka) ? (float)((double)X[(size_t)row * ld + a0 + lc] - ma) : 0.0f;
            sB[k][lc] = (in && okb) ? (float)((double)X[(size_t)row * ld + b0 + lc] - mb) : 0.0f;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < EM_KC; ++k) {
            const float4 a4 = *reinterpret_cast<const float4*>(&sA[k][ty * 4]);
            const float4 b4 = *reinterpret_cast<const float4*>(&sB[k][tx * 4]);
            const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(a[u], b[v], acc[u][v]);
        }
        __syncthreads();
        if (++since == EM_COV_FLUSH) {
            since = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) { dacc[u][v] += (double)acc[u][v]; acc[u][v] = 0.0f; }
        }
    }
    double* out = tiles + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (EM_TILE * EM_TILE);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) out[(ty * 4 + u) * EM_TILE + tx * 4 + v] = dacc[u][v] + (double)acc[u][v];
}

// grid ntp: the slabs of a tile in slab order, / (n - 1), stored at (i, j) and (j, i) of cov [F][F]
__global__ __launch_bounds__(EM_THREADS) void em_cov_reduce_kernel(int n, int F, int nt, int S, const double* __restrict__ tiles,
                                                                   double* __restrict__ cov) {
    int bi, bj;
    em_tile_pair(blockIdx.x, nt, bi, bj);
    for (int e = threadIdx.x; e < EM_TILE * EM_TILE; e += EM_THREADS) {
        const int i = bi * EM_TILE + (e >> 6), j = bj * EM_TILE + (e & 63);
        if (i >= F || j >= F) continue;
        double a = 0.0;
        for (int s = 0; s < S; ++s) a += tiles[((size_t)s * gridDim.x + blockIdx.x) * (EM_TILE * EM_TILE) + e];
        a /= (double)(n - 1);
        cov[(size_t)i * F + j] = a;
        cov[(size_t)j * F + i] = a;
    }
}

// one wave per row: out[row][m] = sum_f (x_f - mean_f) V[m][f], m < k
__global__ __launch_bounds__(EM_THREADS) void em_project_kernel(const float* __restrict__ X, int n, int F, int ld, const double* __restrict__ mean,
                                                                const float* __restrict__ V, int k, float* __restrict__ out) {
    __shared__ float s_v[EM_MAX_K][EM_MAX_F];
    __shared__ double s_mu[EM_MAX_F];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < k * F; e += EM_THREADS) s_v[e / F][e % F] = V[e];
    for (int e = tid; e < F; e += EM_THREADS) s_mu[e] = mean[e];
    __syncthreads();
    for (int row = blockIdx.x * (EM_THREADS / WAVE) + wave; row < n; row += gridDim.x * (EM_THREADS / WAVE)) {
        float acc[EM_MAX_K];
#pragma unroll
        for (int m = 0; m < EM_MAX_K; ++m) acc[m] = 0.0f;
        for (int c = lane; c < F; c += WAVE) {
            const float xc = (float)((double)X[(size_t)row * ld + c] - s_mu[c]);
#pragma unroll
            for (int m = 0; m < EM_MAX_K; ++m)
                if (m < k) acc[m] = fmaf(xc, s_v[m][c], acc[m]);
        }
#pragma unroll
        for (int m = 0; m < EM_MAX_K; ++m) {
            const float t = wave_sum(acc[m]);
            if (lane == 0 && m < k) out[(size_t)row * k + m] = t;
        }
    }
}

struct PcaWs { double* slabs; double* tiles; int G, nt, ntp, S, per; size_t bytes; };
static inline PcaWs pca_layout(void* base, int64_t n, int F) {
    PcaWs w;
    char* p = static_cast<char*>(base);
    size_t o = 0;
    auto take = [&](size_t bytes) { char* q = p + o; o += align256(bytes); return q; };
    const int64_t chunks = (n + EM_COL_ROWS - 1) / EM_COL_ROWS;
    w.G = (int)(chunks < EM_COL_WGS ? chunks : EM_COL_WGS);
    w.nt = cdiv(F, EM_TILE);
    w.ntp = w.nt * (w.nt + 1) / 2;
    const int64_t steps = (n + EM_KC * EM_COV_FLUSH - 1) / (EM_KC * EM_COV_FLUSH);      // a slab is a whole number of flush periods
    w.S = (int)(steps < EM_COV_SLABS ? steps : EM_COV_SLABS);
    w.per = (int)((steps + w.S - 1) / w.S) * EM_KC * EM_COV_FLUSH;
    w.slabs = reinterpret_cast<double*>(take((size_t)w.G * pad4(F) * 8));
    w.tiles = reinterpret_cast<double*>(take((size_t)w.S * w.ntp * EM_TILE * EM_TILE * 8));
    w.bytes = o;
    return w;
}

static int em_check_x(const char* fn, const float* X, int64_t n, int F, int ld, int64_t max_n) {
    EAGCN_CHECK_ARG(X, "%s: X is null", fn);
    EAGCN_CHECK_ARG(F >= 1 && F <= EM_MAX_F, "%s: F = %d is not in 1 .. %d", fn, F, EM_MAX_F);
    EAGCN_CHECK_ARG(n >= EM_MIN_N && n <= max_n, "%s: n = %lld is not in %d .. %lld", fn, (long long)n, EM_MIN_N, (long long)max_n);
    EAGCN_CHECK_ARG(ld >= F, "%s: row stride ld = %d is smaller than F = %d", fn, ld, F);
    EAGCN_CHECK_ARG((reinterpret_cast<uintptr_t>(X) & 3) == 0, "%s: X must be 4-byte aligned", fn);
    return EAGCN_OK;
}
static int ts_check(const char* fn, const float* P, int64_t n, int ldp, const void* ws, size_t ws_bytes) {
    EAGCN_CHECK_ARG(P, "%s: P is null", fn);
    EAGCN_CHECK_ARG(n >= EM_MIN_N && n <= EM_MAX_N, "%s: n = %lld is not in %d .. %d", fn, (long long)n, EM_MIN_N, EM_MAX_N);
    EAGCN_CHECK_ARG(ldp >= n && (ldp & 3) == 0, "%s: ldp = %d must be a multiple of 4 and at least n = %lld", fn, ldp, (long long)n);
    EAGCN_CHECK_ARG((reinterpret_cast<uintptr_t>(P) & 15) == 0, "%s: P must be 16-byte aligned", fn);
    EAGCN_CHECK_ARG(ws, "%s: workspace is null", fn);
    EAGCN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
    const size_t need = ts_layout(nullptr, n).bytes;
    EAGCN_CHECK_ARG(ws_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", fn, ws_bytes, need);
    return EAGCN_OK;
}
static int ts_pstat(const float* P, int n, int ldp, float alpha, const TsWs& w, int slot, hipStream_t s) {
    ts_pstat_kernel<<<n, EM_THREADS, 0, s>>>(P, n, ldp, alpha, w.prow);
    EAGCN_LAUNCH_CHECK();
    em_sum_kernel<<<1, EM_THREADS, 0, s>>>(w.prow, n, 2, 2, 1.0, w.consts + slot);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

}  // namespace eagcn

using namespace eagcn;

extern "C" int eagcn_sqdist(const float* X, int64_t n, int F, int ld, float* D, void* stream) {
    if (int rc = em_check_x("eagcn_sqdist", X, n, F, ld, EM_MAX_N)) return rc;
    EAGCN_CHECK_ARG(D, "eagcn_sqdist: D is null");
    const int nt = cdiv((int)n, EM_TILE);
    em_sqdist_kernel<<<dim3(nt, nt), EM_THREADS, 0, (hipStream_t)stream>>>(X, (int)n, F, ld, D);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

extern "C" size_t eagcn_tsne_workspace_bytes(int64_t n) {
    if (n < EM_MIN_N || n > EM_MAX_N) return 0;
    return ts_layout(nullptr, n).bytes;
}

extern "C" int eagcn_tsne_affinities(const float* D, int64_t n, double perplexity, float* P, int ldp, double* betas, int32_t* steps,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    EAGCN_CHECK_ARG(D, "eagcn_tsne_affinities: D is null");
    EAGCN_CHECK_ARG(betas, "eagcn_tsne_affinities: betas is null");
    if (int rc = ts_check("eagcn_tsne_affinities", P, n, ldp, workspace, workspace_bytes)) return rc;
    EAGCN_CHECK_ARG(perplexity > 0.0 && perplexity < (double)n, "eagcn_tsne_affinities: perplexity = %g is not in (0, n = %lld)", perplexity,
                    (long long)n);
    const TsWs w = ts_layout(workspace, n);
    double* srow = w.prow;               // [n] row sums, then [n] sums of the conditional rows
    double* rs = w.prow + n;
    ts_search_kernel<<<(int)n, EM_THREADS, 0, s>>>(D, (int)n, log(perplexity), betas, srow, rs, steps);
    EAGCN_LAUNCH_CHECK();
    em_sum_kernel<<<1, EM_THREADS, 0, s>>>(rs, (int)n, 1, 1, 2.0, w.consts + 4);
    EAGCN_LAUNCH_CHECK();
    const int nt = cdiv((int)n, EM_TILE);
    ts_joint_kernel<<<dim3(nt, nt), EM_THREADS, 0, s>>>(D, (int)n, ldp, betas, srow, w.consts + 4, P);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

extern "C" int eagcn_tsne_gradient(const float* P, int ldp, const float* Y, int64_t n, float alpha, int compute_kl, float* grad, double* out,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ts_check("eagcn_tsne_gradient", P, n, ldp, workspace, workspace_bytes)) return rc;
    EAGCN_CHECK_ARG(Y, "eagcn_tsne_gradient: Y is null");
    EAGCN_CHECK_ARG((reinterpret_cast<uintptr_t>(Y) & 15) == 0, "eagcn_tsne_gradient: Y must be 16-byte aligned");
    EAGCN_CHECK_ARG(grad, "eagcn_tsne_gradient: grad is null");
    EAGCN_CHECK_ARG(out, "eagcn_tsne_gradient: out is null");
    const TsWs w = ts_layout(workspace, n);
    if (compute_kl)
        if (int rc = ts_pstat(P, (int)n, ldp, alpha, w, 4, s)) return rc;
    ts_pair_kernel<<<w.G, EM_THREADS, 0, s>>>(P, ldp, Y, (int)n, nullptr, alpha, w.A, w.R, w.z, w.zpart);
    EAGCN_LAUNCH_CHECK();
    if (compute_kl) {
        ts_kl_kernel<<<(int)n, EM_THREADS, 0, s>>>(P, ldp, Y, (int)n, nullptr, alpha, w.klrows);
        EAGCN_LAUNCH_CHECK();
    }
    ts_row_kernel<false><<<w.W, EM_THREADS, 0, s>>>(nullptr, (int)n, w.G, w.zpart, w.A, w.R, nullptr, nullptr, nullptr, grad, w.klrows,
                                                    compute_kl, w.parts, w.consts);
    EAGCN_LAUNCH_CHECK();
    ts_decide_kernel<<<1, WAVE, 0, s>>>(nullptr, 1, w.W, w.parts, w.consts, compute_kl ? 4 : -1, out);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

extern "C" int eagcn_tsne_begin(const float* P, int ldp, int64_t n, const float* Y0, float early_exaggeration, float learning_rate,
                                int max_iter, int n_iter_without_progress, double min_grad_norm, void* workspace, size_t workspace_bytes,
                                void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ts_check("eagcn_tsne_begin", P, n, ldp, workspace, workspace_bytes)) return rc;
    EAGCN_CHECK_ARG(Y0, "eagcn_tsne_begin: Y0 is null");
    EAGCN_CHECK_ARG(early_exaggeration >= 1.0f, "eagcn_tsne_begin: early_exaggeration = %g is below 1", (double)early_exaggeration);
    EAGCN_CHECK_ARG(learning_rate > 0.0f, "eagcn_tsne_begin: learning_rate = %g is not positive", (double)learning_rate);
    EAGCN_CHECK_ARG(max_iter >= 0 && n_iter_without_progress >= 0, "eagcn_tsne_begin: max_iter = %d, n_iter_without_progress = %d", max_iter,
                    n_iter_without_progress);
    const TsWs w = ts_layout(workspace, n);
    EAGCN_HIP(hipMemcpyAsync(w.Y, Y0, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
    ts_begin_kernel<<<w.W, EM_THREADS, 0, s>>>(w.st, (int)n, w.U, w.gains, early_exaggeration, learning_rate, max_iter, n_iter_without_progress,
                                               min_grad_norm);
    EAGCN_LAUNCH_CHECK();
    if (int rc = ts_pstat(P, (int)n, ldp, early_exaggeration, w, 0, s)) return rc;
    return ts_pstat(P, (int)n, ldp, 1.0f, w, 2, s);
}

extern "C" int eagcn_tsne_iterate(const float* P, int ldp, int64_t n, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ts_check("eagcn_tsne_iterate", P, n, ldp, workspace, workspace_bytes)) return rc;
    const TsWs w = ts_layout(workspace, n);
    ts_pair_kernel<<<w.G, EM_THREADS, 0, s>>>(P, ldp, w.Y, (int)n, w.st, 1.0f, w.A, w.R, w.z, w.zpart);
    EAGCN_LAUNCH_CHECK();
    ts_kl_kernel<<<(int)n, EM_THREADS, 0, s>>>(P, ldp, w.Y, (int)n, w.st, 1.0f, w.klrows);
    EAGCN_LAUNCH_CHECK();
    ts_row_kernel<true><<<w.W, EM_THREADS, 0, s>>>(w.st, (int)n, w.G, w.zpart, w.A, w.R, w.Y, w.U, w.gains, nullptr, w.klrows, 0, w.parts,
                                                   w.consts);
    EAGCN_LAUNCH_CHECK();
    ts_decide_kernel<<<1, WAVE, 0, s>>>(w.st, 0, w.W, w.parts, w.consts, 0, nullptr);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

extern "C" int eagcn_tsne_finish(const float* P, int ldp, int64_t n, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ts_check("eagcn_tsne_finish", P, n, ldp, workspace, workspace_bytes)) return rc;
    const TsWs w = ts_layout(workspace, n);
    ts_pair_kernel<<<w.G, EM_THREADS, 0, s>>>(P, ldp, w.Y, (int)n, nullptr, 1.0f, w.A, w.R, w.z, w.zpart);
    EAGCN_LAUNCH_CHECK();
    ts_kl_kernel<<<(int)n, EM_THREADS, 0, s>>>(P, ldp, w.Y, (int)n, nullptr, 1.0f, w.klrows);
    EAGCN_LAUNCH_CHECK();
    ts_row_kernel<false><<<w.W, EM_THREADS, 0, s>>>(nullptr, (int)n, w.G, w.zpart, w.A, w.R, nullptr, nullptr, nullptr, w.grad, w.klrows, 1,
                                                    w.parts, w.consts);
    EAGCN_LAUNCH_CHECK();
    ts_decide_kernel<<<1, WAVE, 0, s>>>(w.st, 2, w.W, w.parts, w.consts, 2, nullptr);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

extern "C" size_t eagcn_pca_workspace_bytes(int64_t n, int F) {
    if (n < EM_MIN_N || n >= (int64_t(1) << 31) || F < 1 || F > EM_MAX_F) return 0;
    return pca_layout(nullptr, n, F).bytes;
}

extern "C" int eagcn_pca_cov(const float* X, int64_t n, int F, int ld, double* mean, double* cov, void* workspace, size_t workspace_bytes,
                             void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = em_check_x("eagcn_pca_cov", X, n, F, ld, (int64_t(1) << 31) - 1)) return rc;
    EAGCN_CHECK_ARG(mean, "eagcn_pca_cov: mean is null");
    EAGCN_CHECK_ARG(cov, "eagcn_pca_cov: cov is null");
    EAGCN_CHECK_ARG(workspace, "eagcn_pca_cov: workspace is null");
    EAGCN_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "eagcn_pca_cov: workspace must be 256-byte aligned");
    const PcaWs w = pca_layout(workspace, n, F);
    EAGCN_CHECK_ARG(workspace_bytes >= w.bytes, "eagcn_pca_cov: workspace too small (%zu < %zu bytes)", workspace_bytes, w.bytes);
    em_colsum_kernel<<<w.G, EM_THREADS, 0, s>>>(X, (int)n, F, ld, w.slabs);
    EAGCN_LAUNCH_CHECK();
    em_mean_kernel<<<cdiv(F, EM_THREADS), EM_THREADS, 0, s>>>((int)n, F, w.G, w.slabs, mean);
    EAGCN_LAUNCH_CHECK();
    em_cov_kernel<<<dim3(w.ntp, w.S), EM_THREADS, 0, s>>>(X, (int)n, F, ld, mean, w.nt, w.per, w.tiles);
    EAGCN_LAUNCH_CHECK();
    em_cov_reduce_kernel<<<w.ntp, EM_THREADS, 0, s>>>((int)n, F, w.nt, w.S, w.tiles, cov);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

extern "C" int eagcn_pca_project(const float* X, int64_t n, int F, int ld, const double* mean, const float* components, int k, float* out,
                                 void* stream) {
    if (int rc = em_check_x("eagcn_pca_project", X, n, F, ld, (int64_t(1) << 31) - 1)) return rc;
    EAGCN_CHECK_ARG(mean, "eagcn_pca_project: mean is null");
    EAGCN_CHECK_ARG(components, "eagcn_pca_project: components is null");
    EAGCN_CHECK_ARG(out, "eagcn_pca_project: out is null");
    EAGCN_CHECK_ARG(k >= 1 && k <= EM_MAX_K && k <= F, "eagcn_pca_project: k = %d is not in 1 .. min(%d, F = %d)", k, EM_MAX_K, F);
    const int64_t want = (n + 3) / 4;
    em_project_kernel<<<(int)(want < 2048 ? want : 2048), EM_THREADS, 0, (hipStream_t)stream>>>(X, (int)n, F, ld, mean, components, k, out);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}
