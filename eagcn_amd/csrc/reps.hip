// The evaluation-time consumers of the atom representations (train.py:213-287 and the clustering of kmeans_atomrep.py), on the device:
//
//   eagcn_rep_gather[_dense]  the rows of the last layer's output whose sub-type lies in [lo, hi], appended behind a DEVICE row counter in
//                             ascending (molecule, atom) order -- the order of the reference's loop over the flattened batch -- straight
//                             from the PACKED matrix: the padded [B, N, F] tensor is never formed and nothing is read by the host.
//   eagcn_kmeans_*            Lloyd's k-means over such rows.  One iteration is three launches and no host read:
//     km_assign_kernel  every row is fetched ONCE; a workgroup of 256 threads takes KM_R rows at a time, thread t holding columns
//                       4t .. 4t+3 of each (F <= 1024) while the next KM_R rows stream in.  Squared distances are direct sums of
//                       (x - c)^2: per thread, then over the wave (km_fold8), then over the four waves in wave order through LDS.  The argmin takes the lowest index on ties.  The
//                       rows, still in registers, are then added to the workgroup's per-cluster sums, fp64 in LDS: the words of columns
//                       4t .. 4t+3 belong to thread t alone and receive the rows in ascending order -- no atomics, a fixed order.  A
//                       workgroup walks chunks of KM_ROWS rows (chunk g, g + grid, ...) and leaves ONE slab of sums and counts.
//     km_reduce_kernel  adds the slabs in slab order (fp64), forms the new centroids (an empty cluster keeps its own) and the squared
//                       shift of its 16 elements.
//     km_decide_kernel  one wave: changed labels, inertia, shift, n_iter and the stop decision.
//   Every launch of an iteration returns at once when `done` is set: iterations enqueued behind convergence change nothing.
#include "common.h"
#include "kernels.h"

namespace eagcn {

constexpr int KM_ROWS = 64;          // rows of the chunk a workgroup owns at a time
constexpr int KM_R = 8;              // rows of a chunk in flight (in registers) at a time
constexpr int KM_BPC = KM_ROWS / KM_R; // batches per chunk
constexpr int KM_THREADS = 256;      // one float4 of a row per thread: F <= 1024
constexpr int KM_MAX_WGS = 768;      // workgroups of the assign launch (three per CU at the reference's width) = slabs the reduce adds up
constexpr int KM_MAX_K = 16;
constexpr int KM_MAX_F = 1024;
constexpr int KM_MAX_KF = 8192;      // k * pad4(F): 32 KB of centroids + 64 KB of fp64 sums in LDS at the most
constexpr int KM_RED_COLS = 16;      // elements of a workgroup of the reduce launch, KM_RED_PARTS threads each
constexpr int KM_RED_PARTS = KM_THREADS / KM_RED_COLS;
constexpr int KM_STATIC_LDS = 4096;    // more than the assign kernel's static LDS (partial sums, labels)
constexpr int KM_PARTS_BYTES = 8192; // per-block shifts of the reduce (<= 512 doubles) / per-column variances of begin (<= 1024)
static_assert(KM_ROWS % KM_R == 0 && KM_R == 8 && KM_THREADS * 4 == KM_MAX_F, "a thread holds one float4 of each of eight rows");

struct KmState {                     // the first 64 bytes of the workspace (eagcn_hip.h)
    int32_t done, n_iter, changed, n_empty;
    double inertia, shift, tol_abs;
    int32_t reserved[6];
};
static_assert(sizeof(KmState) == 64, "eagcn_hip.h documents a 64-byte state block");

struct KmWs {                        // the workspace, cut up (every part 256-byte aligned)
    KmState* st; float* cen; int32_t* counts; int32_t* labels; float* mind;
    double* slabs; int32_t* wgcnt; int32_t* wgchg; double* wgine; double* parts;
    int G; size_t bytes;
};
static inline int km_grid(int64_t n) {
    const int64_t chunks = (n + KM_ROWS - 1) / KM_ROWS;
    return (int)(chunks < KM_MAX_WGS ? chunks : KM_MAX_WGS);
}
static inline KmWs km_layout(void* base, int64_t n, int F, int k) {
    KmWs w;
    char* p = static_cast<char*>(base);
    size_t o = 0;
    auto take = [&](size_t bytes) { char* q = p + o; o += align256(bytes); return q; };
    const int G = km_grid(n), F4 = pad4(F), kk = k < 2 ? 2 : k;      // (begin's column statistics use two slab rows)
    w.G = G;
    w.st = reinterpret_cast<KmState*>(take(256));
    w.cen = reinterpret_cast<float*>(take((size_t)k * F * 4));
    w.counts = reinterpret_cast<int32_t*>(take(KM_MAX_K * 4));
    w.labels = reinterpret_cast<int32_t*>(take((size_t)n * 4));
    w.mind = reinterpret_cast<float*>(take((size_t)n * 4));
    w.slabs = reinterpret_cast<double*>(take((size_t)G * kk * F4 * 8));
    w.wgcnt = reinterpret_cast<int32_t*>(take((size_t)G * KM_MAX_K * 4));
    w.wgchg = reinterpret_cast<int32_t*>(take((size_t)G * 4));
    w.wgine = reinterpret_cast<double*>(take((size_t)G * 8));
    w.parts = reinterpret_cast<double*>(take(KM_PARTS_BYTES));
    w.bytes = o;
    return w;
}

// four adjacent columns of a row; columns >= F read as zero.  VEC: the rows are 16-byte aligned (base and stride)
template <bool VEC>
__device__ __forceinline__ float4 km_load4(const float* __restrict__ row, int col, int F) {
    if (VEC && col + 4 <= F) return *reinterpret_cast<const float4*>(row + col);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (col < F) v.x = row[col];
    if (col + 1 < F) v.y = row[col + 1];
    if (col + 2 < F) v.z = row[col + 2];
    if (col + 3 < F) v.w = row[col + 3];
    return v;
}

// The sums over the wave of eight values per lane in 10 cross-lane steps instead of 48: at the offsets 32, 16 and 8 a lane keeps half of
// its values and hands the other half to its partner, then three butterfly steps on the one value left.  Every lane ends with the
// wave's sum of v[4 b3 + 2 b4 + b5] (b_i = bit i of the lane), the same bits in all eight lanes that share those bits.  A fixed order.
__device__ __forceinline__ float km_fold8(const float (&v)[8], int lane) {
    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
    float w[4], u[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (h5 ? v[2 * i + 1] : v[2 * i]) + __shfl_xor(h5 ? v[2 * i] : v[2 * i + 1], 32);
#pragma unroll
    for (int i = 0; i < 2; ++i) u[i] = (h4 ? w[2 * i + 1] : w[2 * i]) + __shfl_xor(h4 ? w[2 * i] : w[2 * i + 1], 16);
    float t = (h3 ? u[1] : u[0]) + __shfl_xor(h3 ? u[0] : u[1], 8);
    t += __shfl_xor(t, 4);
    t += __shfl_xor(t, 2);
    t += __shfl_xor(t, 1);
    return t;
}

// grid G.  ACC: one Lloyd iteration's assignment and per-cluster sums (returns at once when st->done); else the assignment alone.
// LDS: centroids [k][F4] fp32, then (ACC) the sums as two planes [k][F4 / 4] of double2 (columns 4q, 4q+1 | 4q+2, 4q+3), so that a
// thread's 16-byte LDS accesses are contiguous over the lanes.
template <bool VEC, bool ACC>
__global__ __launch_bounds__(KM_THREADS) void km_assign_kernel(const float* __restrict__ X, int n, int F, int ld, int k,
                                                               const float* __restrict__ C, const KmState* __restrict__ st,
                                                               int32_t* __restrict__ labels, float* __restrict__ mind,
                                                               double* __restrict__ slabs, int32_t* __restrict__ wgcnt,
                                                               int32_t* __restrict__ wgchg, double* __restrict__ wgine) {
    extern __shared__ __attribute__((aligned(16))) unsigned char km_smem[];
    __shared__ __attribute__((aligned(16))) float s_part[KM_R][KM_MAX_K][KM_THREADS / WAVE];
    __shared__ int s_lab[KM_R];
    __shared__ int s_chg[KM_R];
    __shared__ double s_ine[KM_R];
    if (ACC && st->done) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F4 = (F + 3) & ~3, Q = F4 >> 2, col = 4 * tid;
    const bool active = col < F4;
    float* s_cen = reinterpret_cast<float*>(km_smem);
    double2* s_acc0 = reinterpret_cast<double2*>(km_smem + (size_t)k * F4 * 4);
    double2* s_acc1 = s_acc0 + (size_t)k * Q;
    for (int e = tid; e < k * F4; e += KM_THREADS) {
        const int c = e / F4, j = e - c * F4;
        s_cen[e] = j < F ? C[(size_t)c * F + j] : 0.0f;
    }
    if (ACC)
        for (int e = tid; e < 2 * k * Q; e += KM_THREADS) s_acc0[e] = make_double2(0.0, 0.0);
    int my_cnt = 0;                                        // threads < k: rows of cluster tid
    int my_chg = 0;                                        // threads < KM_R: over the rows r0 + tid of every batch, in row order
    double my_ine = 0.0;
    __syncthreads();

    // The batches of this workgroup in order: batch j is KM_R rows of chunk blockIdx.x + (j / KM_BPC) * grid; nr = 0 ends the walk (only
    // the last chunk of all is short, and it is the last one of its workgroup).
    const int chunks = (n + KM_ROWS - 1) / KM_ROWS;
    auto batch = [&](int j, int& r0) -> int {
        const int chunk = blockIdx.x + (j / KM_BPC) * gridDim.x;
        r0 = 0;
        if (chunk >= chunks) return 0;
        r0 = chunk * KM_ROWS + (j % KM_BPC) * KM_R;
        const int cend = (int)min((long long)n, (long long)(chunk + 1) * KM_ROWS);
        return max(0, min(KM_R, cend - r0));
    };
    auto load = [&](float4 (&v)[KM_R], int r0, int nr) {
#pragma unroll
        for (int r = 0; r < KM_R; ++r)
            v[r] = (active && r < nr) ? km_load4<VEC>(X + (size_t)(r0 + r) * ld, col, F) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    const int prow = ((lane >> 3) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 5) & 1);    // the row km_fold8 leaves in this lane
    float4 x[KM_R], xn[KM_R];
    int r0, nr = batch(0, r0);
    load(x, r0, nr);
    for (int j = 0; nr > 0; ++j) {
        int r0n;
        const int nrn = batch(j + 1, r0n);
        load(xn, r0n, nrn);                                // the next batch streams in while this one is worked on
        const int old = tid < nr ? labels[r0 + tid] : 0;   // (read here: its latency is gone by the time the argmin needs it)
        for (int c = 0; c < k; ++c) {
            const float4 cv = active ? *reinterpret_cast<const float4*>(s_cen + c * F4 + col) : make_float4(0.f, 0.f, 0.f, 0.f);
            float p[KM_R];
#pragma unroll
            for (int r = 0; r < KM_R; ++r) {
                const float dx = x[r].x - cv.x, dy = x[r].y - cv.y, dz = x[r].z - cv.z, dw = x[r].w - cv.w;
                p[r] = dx * dx;
                p[r] = fmaf(dy, dy, p[r]);
                p[r] = fmaf(dz, dz, p[r]);
                p[r] = fmaf(dw, dw, p[r]);
            }
            const float t = km_fold8(p, lane);
            if ((lane & 7) == 0) s_part[prow][c][wave] = t;
        }
        __syncthreads();
        int best = -1;                                     // (wave 0: -1 in the lanes that hold no row)
        if (tid < nr) {
            const int row = r0 + tid;
            float bd = 0.0f;
            for (int c0 = 0; c0 < k; c0 += 4) {            // four clusters' partial sums in flight (s_part holds KM_MAX_K per row)
                float4 q[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) q[u] = *reinterpret_cast<const float4*>(&s_part[tid][c0 + u][0]);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float d = ((q[u].x + q[u].y) + q[u].z) + q[u].w;
                    if (c0 + u < k && (best < 0 || d < bd)) { bd = d; best = c0 + u; }
                }
            }
            s_lab[tid] = best;
            my_chg += old != best;
            labels[row] = best;
            mind[row] = bd;
            my_ine += (double)bd;
        }
        if (wave == 0)                                     // lane c counts the rows of cluster c
            for (int c = 0; c < k; ++c) {
                const int m = __popcll(__ballot(best == c));
                if (lane == c) my_cnt += m;
            }
        __syncthreads();
        if (ACC && active) {
#pragma unroll
            for (int r = 0; r < KM_R; ++r) {
                if (r < nr) {
                    const int o = s_lab[r] * Q + tid;
                    double2 a = s_acc0[o], b = s_acc1[o];
                    a.x += (double)x[r].x; a.y += (double)x[r].y;
                    b.x += (double)x[r].z; b.y += (double)x[r].w;
                    s_acc0[o] = a;
                    s_acc1[o] = b;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < KM_R; ++r) x[r] = xn[r];
        r0 = r0n;
        nr = nrn;
    }
    if (tid < KM_R) { s_chg[tid] = my_chg; s_ine[tid] = my_ine; }
    __syncthreads();
    const int g = blockIdx.x;
    if (ACC && active) {
        for (int c = 0; c < k; ++c) {
            double2* out = reinterpret_cast<double2*>(slabs + ((size_t)g * k + c) * F4 + col);
            out[0] = s_acc0[c * Q + tid];
            out[1] = s_acc1[c * Q + tid];
        }
    }
    if (tid < KM_MAX_K) wgcnt[g * KM_MAX_K + tid] = my_cnt;
    if (tid == 0) {
        int chg = 0;
        double ine = 0.0;
        for (int r = 0; r < KM_R; ++r) { chg += s_chg[r]; ine += s_ine[r]; }
        wgchg[g] = chg;
        wgine[g] = ine;
    }
}

// sum over the slabs g of v[g * stride]: thread (part, col) of the workgroup takes the slabs [part * per, ...) in slab order, eight loads
// in flight at a time, and the threads of part 0 add the KM_RED_PARTS partial sums in part order: a fixed order.  s_q: [parts][cols]
// doubles.  The result is valid in the threads < KM_RED_COLS.
__device__ __forceinline__ double km_slab_sum(const double* __restrict__ v, size_t stride, int G, bool ok, double (*s_q)[KM_RED_COLS]) {
    const int col = threadIdx.x % KM_RED_COLS, part = threadIdx.x / KM_RED_COLS, per = (G + KM_RED_PARTS - 1) / KM_RED_PARTS;
    const int g0 = min(G, part * per), g1 = min(G, g0 + per);
    double a = 0.0;
    if (ok) {
        int g = g0;
        for (; g + 8 <= g1; g += 8) {
            double t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = v[(size_t)(g + u) * stride];
#pragma unroll
            for (int u = 0; u < 8; ++u) a += t[u];
        }
        for (; g < g1; ++g) a += v[(size_t)g * stride];
    }
    __syncthreads();                                       // (s_q may still be read from the sum before)
    s_q[part][col] = a;
    __syncthreads();
    double tot = 0.0;
    if (part == 0)
        for (int q = 0; q < KM_RED_PARTS; ++q) tot += s_q[q][col];
    return tot;
}

// grid ceil(k * F4 / 16), 256 threads: new centroids of 16 (cluster, column) elements, the cluster counts (block 0 stores them) and
// this block's part of the squared shift
__global__ __launch_bounds__(KM_THREADS) void km_reduce_kernel(KmState* __restrict__ st, float* __restrict__ C, int F, int k, int G,
                                                               const double* __restrict__ slabs, const int32_t* __restrict__ wgcnt,
                                                               int32_t* __restrict__ counts, double* __restrict__ parts) {
    __shared__ double s_q[KM_RED_PARTS][KM_RED_COLS];
    __shared__ int s_cq[KM_THREADS / KM_MAX_K][KM_MAX_K];
    __shared__ int s_cnt[KM_MAX_K];
    if (st->done) return;
    const int tid = threadIdx.x;
    const int F4 = (F + 3) & ~3;
    {   // the cluster counts (integers: any order): thread (q, c) over the slabs q, q + 16, ...
        const int c = tid % KM_MAX_K, q = tid / KM_MAX_K;
        int a = 0;
        for (int g = q; g < G; g += KM_THREADS / KM_MAX_K) a += wgcnt[g * KM_MAX_K + c];
        s_cq[q][c] = a;
    }
    __syncthreads();
    if (tid < KM_MAX_K) {
        int a = 0;
        for (int q = 0; q < KM_THREADS / KM_MAX_K; ++q) a += s_cq[q][tid];
        s_cnt[tid] = a;
        if (blockIdx.x == 0) counts[tid] = a;
    }
    const int e = blockIdx.x * KM_RED_COLS + tid % KM_RED_COLS;
    const int c = e / F4, j = e - c * F4;
    const bool ok = e < k * F4 && j < F;
    const double sum = km_slab_sum(slabs + e, (size_t)k * F4, G, ok, s_q);     // (its barriers publish s_cnt as well)
    if (tid < WAVE) {
        double sq = 0.0;
        if (ok && tid < KM_RED_COLS) {
            const float old = C[(size_t)c * F + j];
            const int cnt = s_cnt[c];
            const float cn = cnt > 0 ? (float)(sum / (double)cnt) : old;
            const double d = (double)cn - (double)old;
            C[(size_t)c * F + j] = cn;
            sq = d * d;
        }
        sq = wave_sum(sq);
        if (tid == 0) parts[blockIdx.x] = sq;
    }
}

// lane-strided sum of v[0 .. m) over one wave: lanes in index order, then the butterfly -- a fixed order
__device__ __forceinline__ double km_wave_total(const double* __restrict__ v, int m) {
    double a = 0.0;
    for (int i = threadIdx.x; i < m; i += WAVE) a += v[i];
    return wave_sum(a);
}
__device__ __forceinline__ int km_wave_total(const int32_t* __restrict__ v, int m, int stride) {
    int a = 0;
    for (int i = threadIdx.x; i < m; i += WAVE) a += v[(size_t)i * stride];
    return wave_sum(a);
}

// one wave: the bookkeeping of an iteration and its stop decision
__global__ __launch_bounds__(WAVE) void km_decide_kernel(KmState* __restrict__ st, int k, int G, int nblk, const int32_t* __restrict__ wgchg,
                                                         const double* __restrict__ wgine, const double* __restrict__ parts,
                                                         const int32_t* __restrict__ counts) {
    if (st->done) return;
    const int changed = km_wave_total(wgchg, G, 1);
    const double inertia = km_wave_total(wgine, G), shift = km_wave_total(parts, nblk);
    int empty = (int)threadIdx.x < k && counts[threadIdx.x] == 0;
    empty = wave_sum(empty);
    if (threadIdx.x == 0) {
        st->n_iter += 1;
        st->changed = changed;
        st->inertia = inertia;
        st->shift = shift;
        st->n_empty = empty;
        if (changed == 0 || shift <= st->tol_abs) st->done = 1;
    }
}

// one wave, behind the assignment pass of eagcn_kmeans_finish: inertia, final counts and n_empty
__global__ __launch_bounds__(WAVE) void km_finish_kernel(KmState* __restrict__ st, int k, int G, const int32_t* __restrict__ wgcnt,
                                                         const double* __restrict__ wgine, int32_t* __restrict__ counts) {
    const double inertia = km_wave_total(wgine, G);
    int empty = 0;
    for (int c = 0; c < k; ++c) {
        const int cnt = km_wave_total(wgcnt + c, G, KM_MAX_K);
        if (threadIdx.x == 0) counts[c] = cnt;
        empty += cnt == 0;
    }
    if (threadIdx.x == 0) {
        st->inertia = inertia;
        st->n_empty = empty;
    }
}

// begin, 1 of 3 (grid G): per workgroup and column the fp64 sums of x and x^2 over its chunks -> slab [g][2][F4]
template <bool VEC>
__global__ __launch_bounds__(KM_THREADS) void km_colstat_kernel(const float* __restrict__ X, int n, int F, int ld, double* __restrict__ slabs) {
    const int tid = threadIdx.x, F4 = (F + 3) & ~3, col = 4 * tid;
    if (col >= F4) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    const int chunks = (n + KM_ROWS - 1) / KM_ROWS;
    for (int chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int cend = min(n, (chunk + 1) * KM_ROWS);
        for (int r0 = chunk * KM_ROWS; r0 < cend; r0 += KM_R) {
            float4 x[KM_R];
#pragma unroll
            for (int r = 0; r < KM_R; ++r)
                x[r] = r0 + r < cend ? km_load4<VEC>(X + (size_t)(r0 + r) * ld, col, F) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int r = 0; r < KM_R; ++r) {
                const double v[4] = {(double)x[r].x, (double)x[r].y, (double)x[r].z, (double)x[r].w};
#pragma unroll
                for (int u = 0; u < 4; ++u) { s[u] += v[u]; q[u] += v[u] * v[u]; }
            }
        }
    }
    double* out = slabs + (size_t)blockIdx.x * 2 * F4 + col;
#pragma unroll
    for (int u = 0; u < 4; ++u) { out[u] = s[u]; out[F4 + u] = q[u]; }
}

// begin, 2 of 3 (grid ceil(F4 / 16)): the variance over the rows of 16 columns -> var[F4]
__global__ __launch_bounds__(KM_THREADS) void km_var_kernel(int n, int F, int G, const double* __restrict__ slabs, double* __restrict__ var) {
    __shared__ double s_q[KM_RED_PARTS][KM_RED_COLS];
    const int F4 = (F + 3) & ~3, j = blockIdx.x * KM_RED_COLS + threadIdx.x % KM_RED_COLS;
    const bool ok = j < F;
    const double s = km_slab_sum(slabs + j, (size_t)2 * F4, G, ok, s_q);
    const double q = km_slab_sum(slabs + F4 + j, (size_t)2 * F4, G, ok, s_q);
    if (threadIdx.x < KM_RED_COLS && j < F4) {
        const double mean = s / (double)n;
        var[j] = ok ? fmax(q / (double)n - mean * mean, 0.0) : 0.0;
    }
}

// begin, 3 of 3 (one wave): tol_abs = tol * mean of the column variances (scikit-learn's scaling); the state cleared
__global__ __launch_bounds__(WAVE) void km_begin_kernel(KmState* __restrict__ st, int F, double tol, const double* __restrict__ var,
                                                        int32_t* __restrict__ counts) {
    const double tot = km_wave_total(var, F);
    if (threadIdx.x < KM_MAX_K) counts[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        st->done = 0; st->n_iter = 0; st->changed = 0; st->n_empty = 0;
        st->inertia = 0.0; st->shift = 0.0;
        st->tol_abs = tol * (tot / (double)F);
    }
}

static int km_check(const char* fn, const float* X, int64_t n, int F, int ld, int k) {
    EAGCN_CHECK_ARG(X, "%s: X is null", fn);
    EAGCN_CHECK_ARG(k >= 1 && k <= KM_MAX_K, "%s: k = %d is not in 1 .. %d", fn, k, KM_MAX_K);
    EAGCN_CHECK_ARG(F >= 1 && F <= KM_MAX_F, "%s: F = %d is not in 1 .. %d", fn, F, KM_MAX_F);
    EAGCN_CHECK_ARG(k * pad4(F) <= KM_MAX_KF, "%s: k x pad4(F) = %d x %d is more than %d", fn, k, pad4(F), KM_MAX_KF);
    EAGCN_CHECK_ARG(n >= k, "%s: n = %lld rows are fewer than k = %d clusters", fn, (long long)n, k);
    EAGCN_CHECK_ARG(n < (int64_t(1) << 31), "%s: n = %lld does not fit the 32-bit row index (n < 2^31)", fn, (long long)n);
    EAGCN_CHECK_ARG(ld >= F, "%s: row stride ld = %d is smaller than F = %d", fn, ld, F);
    EAGCN_CHECK_ARG((reinterpret_cast<uintptr_t>(X) & 3) == 0, "%s: X must be 4-byte aligned", fn);
    return EAGCN_OK;
}
static int km_check_ws(const char* fn, const void* ws, size_t ws_bytes, int64_t n, int F, int k) {
    EAGCN_CHECK_ARG(ws, "%s: workspace is null", fn);
    EAGCN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
    const size_t need = km_layout(nullptr, n, F, k).bytes;
    EAGCN_CHECK_ARG(ws_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", fn, ws_bytes, need);
    return EAGCN_OK;
}
static inline bool km_vec(const float* X, int ld) { return (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0; }

// the assign launch.  Its LDS (centroids, sums) is dynamic: up to 96 KB; above the 64 KB a kernel may take unasked the limit is raised
template <bool VEC, bool ACC>
static int km_launch_assign(const float* X, int64_t n, int F, int ld, int k, const float* C, const KmState* st, int32_t* labels, float* mind,
                            double* slabs, int32_t* wgcnt, int32_t* wgchg, double* wgine, hipStream_t s) {
    const size_t lds = (size_t)k * pad4(F) * (ACC ? 12 : 4);
    if (lds + KM_STATIC_LDS > 64 * 1024)                   // (set per launch: the attribute belongs to the current device)
        EAGCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&km_assign_kernel<VEC, ACC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds));
    km_assign_kernel<VEC, ACC><<<km_grid(n), KM_THREADS, lds, s>>>(X, (int)n, F, ld, k, C, st, labels, mind, slabs, wgcnt, wgchg, wgine);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}
template <bool ACC>
static int km_assign(const float* X, int64_t n, int F, int ld, int k, const float* C, const KmWs& w, int32_t* labels, float* mind, hipStream_t s) {
    return km_vec(X, ld) ? km_launch_assign<true, ACC>(X, n, F, ld, k, C, w.st, labels, mind, w.slabs, w.wgcnt, w.wgchg, w.wgine, s)
                         : km_launch_assign<false, ACC>(X, n, F, ld, k, C, w.st, labels, mind, w.slabs, w.wgcnt, w.wgchg, w.wgine, s);
}

// ---- the selected-atom gather ------------------------------------------------------------------------------------------------------
constexpr int REP_SCAN_THREADS = 1024;

// One workgroup: rank of every selected (molecule, atom) among the selected ones, in ascending (b, i) order, behind *count.
// dst[e] = destination row, or -1 (not selected, or beyond `cap`: nothing is written there); sub / mol columns written; *count advanced.
__global__ __launch_bounds__(REP_SCAN_THREADS) void rep_scan_kernel(const int32_t* __restrict__ subtype, int total, int Nin, int lo, int hi,
                                                                    const int64_t* __restrict__ mol_index, int64_t cap,
                                                                    int64_t* __restrict__ count, int32_t* __restrict__ dst,
                                                                    int32_t* __restrict__ out_sub, int64_t* __restrict__ out_mol) {
    __shared__ int s_wave[REP_SCAN_THREADS / WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (total + REP_SCAN_THREADS - 1) / REP_SCAN_THREADS;
    const int e0 = min(total, tid * per), e1 = min(total, e0 + per);
    int mine = 0;
    for (int e = e0; e < e1; ++e) {
        const int v = subtype[e];
        mine += v >= lo && v <= hi;
    }
    int incl = mine;                                       // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == WAVE - 1) s_wave[wave] = incl;
    const int64_t base = *count;
    __syncthreads();                                       // (every thread has read *count before thread 0 advances it)
    int before = 0, all = 0;
    for (int w = 0; w < REP_SCAN_THREADS / WAVE; ++w) {
        if (w < wave) before += s_wave[w];
        all += s_wave[w];
    }
    int64_t pos = base + before + (incl - mine);
    for (int e = e0; e < e1; ++e) {
        const int v = subtype[e];
        int d = -1;
        if (v >= lo && v <= hi) {
            if (pos < cap) {
                d = (int)pos;
                out_sub[pos] = v;
                out_mol[pos] = mol_index[e / Nin];
            }
            ++pos;
        }
        dst[e] = d;
    }
    if (tid == 0) *count = min(cap, base + all);
}

// One wave per (molecule, atom): a selected one copies its F exact columns to row dst of X.  PACKED: from the packed matrix as
// eagcn_unpack_rows would (an atom beyond nat[b] reads pad_row, or zeros); else from a dense [B][Nd][F] tensor.
template <bool PACKED>
__global__ __launch_bounds__(256) void rep_copy_kernel(eagcn_batch bt, const float* __restrict__ src, ColMapD m, int ld,
                                                       const float* __restrict__ pad_row, int total, int Nin, int Nd, int F,
                                                       const int32_t* __restrict__ dst, float* __restrict__ X) {
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    for (int e = blockIdx.x * wpb + (threadIdx.x >> 6); e < total; e += gridDim.x * wpb) {
        const int d = dst[e];
        if (d < 0) continue;
        const int b = e / Nin, i = e - b * Nin;
        float* out = X + (size_t)d * F;
        if (PACKED) {
            const float* row = i < bt.nat[b] ? src + (size_t)(bt.row0[b] + i) * ld : pad_row;
            int eo = 0, po = 0;
            for (int s = 0; s < m.nseg; ++s) {
                for (int f = lane; f < m.w[s]; f += WAVE) out[eo + f] = row ? row[po + f] : 0.0f;
                eo += m.w[s];
                po += m.p[s];
            }
        } else {
            const float* row = src + ((size_t)b * Nd + i) * F;
            for (int f = lane; f < F; f += WAVE) out[f] = row[f];
        }
    }
}

static int rep_check(const char* fn, int B, int Nin, int F, const int32_t* subtype, const int64_t* mol_index, const int64_t* count,
                     const int32_t* scratch, const float* X, const int32_t* sub, const int64_t* mol, int64_t cap) {
    EAGCN_CHECK_ARG(subtype, "%s: subtype is null", fn);
    EAGCN_CHECK_ARG(mol_index, "%s: mol_index is null", fn);
    EAGCN_CHECK_ARG(count, "%s: count is null", fn);
    EAGCN_CHECK_ARG(scratch, "%s: scratch is null", fn);
    EAGCN_CHECK_ARG(X && sub && mol, "%s: an output buffer is null", fn);
    EAGCN_CHECK_ARG(B >= 1 && Nin >= 1 && F >= 1, "%s: B = %d, N = %d, F = %d must be positive", fn, B, Nin, F);
    EAGCN_CHECK_ARG((int64_t)B * Nin < (int64_t(1) << 31), "%s: B x N = %d x %d does not fit 32 bits", fn, B, Nin);
    EAGCN_CHECK_ARG(cap >= (int64_t)B * Nin && cap < (int64_t(1) << 31), "%s: cap = %lld is not in B x N = %lld .. 2^31 - 1", fn,
                    (long long)cap, (long long)B * Nin);
    return EAGCN_OK;
}
static inline int rep_copy_grid(int total) { return total / 4 + 1 < 2048 ? total / 4 + 1 : 2048; }

}  // namespace eagcn

using namespace eagcn;

extern "C" int eagcn_rep_gather(const eagcn_batch* b, const float* packed, const eagcn_layout* lay, const float* pad_row,
                                const int32_t* subtype, int lo, int hi, const int64_t* mol_index, int64_t* count, int32_t* scratch,
                                float* X, int32_t* sub, int64_t* mol, int64_t cap, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    EAGCN_CHECK_ARG(b, "eagcn_rep_gather: batch is null");
    EAGCN_CHECK_ARG(lay, "eagcn_rep_gather: layout is null");
    EAGCN_CHECK_ARG(b->T == 0 || packed, "eagcn_rep_gather: null packed matrix");
    const int Nin = b->n_logical > 0 ? b->n_logical : b->N, F = layout_width(lay);
    if (int rc = rep_check("eagcn_rep_gather", b->B, Nin, F, subtype, mol_index, count, scratch, X, sub, mol, cap)) return rc;
    EAGCN_CHECK_ARG(b->nat && b->row0, "eagcn_rep_gather: the batch index is not built");
    const int total = b->B * Nin;
    ProfScope ps(PROF_PACK, s);
    rep_scan_kernel<<<1, REP_SCAN_THREADS, 0, s>>>(subtype, total, Nin, lo, hi, mol_index, cap, count, scratch, sub, mol);
    EAGCN_LAUNCH_CHECK();
    rep_copy_kernel<true><<<rep_copy_grid(total), 256, 0, s>>>(*b, packed, make_colmap(lay), layout_ld(lay), pad_row, total, Nin, Nin, F, scratch, X);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

extern "C" int eagcn_rep_gather_dense(const float* dense, int B, int N, int F, const int32_t* subtype, int N_in, int lo, int hi,
                                      const int64_t* mol_index, int64_t* count, int32_t* scratch, float* X, int32_t* sub, int64_t* mol,
                                      int64_t cap, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    EAGCN_CHECK_ARG(dense, "eagcn_rep_gather_dense: dense is null");
    if (int rc = rep_check("eagcn_rep_gather_dense", B, N_in, F, subtype, mol_index, count, scratch, X, sub, mol, cap)) return rc;
    EAGCN_CHECK_ARG(N >= N_in, "eagcn_rep_gather_dense: N = %d is smaller than the sub-types' N_in = %d", N, N_in);
    const int total = B * N_in;
    eagcn_batch none;
    memset(&none, 0, sizeof(none));
    ProfScope ps(PROF_PACK, s);
    rep_scan_kernel<<<1, REP_SCAN_THREADS, 0, s>>>(subtype, total, N_in, lo, hi, mol_index, cap, count, scratch, sub, mol);
    EAGCN_LAUNCH_CHECK();
    rep_copy_kernel<false><<<rep_copy_grid(total), 256, 0, s>>>(none, dense, ColMapD{}, 0, nullptr, total, N_in, N, F, scratch, X);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

extern "C" size_t eagcn_kmeans_workspace_bytes(int64_t n, int F, int k) {
    if (n < 1 || n >= (int64_t(1) << 31) || F < 1 || F > KM_MAX_F || k < 1 || k > KM_MAX_K) return 0;
    return km_layout(nullptr, n, F, k).bytes;
}

extern "C" int eagcn_kmeans_assign(const float* X, int64_t n, int F, int ld, const float* centers, int k, int32_t* labels, float* mind,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = km_check("eagcn_kmeans_assign", X, n, F, ld, k)) return rc;
    EAGCN_CHECK_ARG(centers, "eagcn_kmeans_assign: centers is null");
    EAGCN_CHECK_ARG(labels, "eagcn_kmeans_assign: labels is null");
    EAGCN_CHECK_ARG(mind, "eagcn_kmeans_assign: mind is null");
    if (int rc = km_check_ws("eagcn_kmeans_assign", workspace, workspace_bytes, n, F, k)) return rc;
    const KmWs w = km_layout(workspace, n, F, k);
    return km_assign<false>(X, n, F, ld, k, centers, w, labels, mind, (hipStream_t)stream);
}

extern "C" int eagcn_kmeans_begin(const float* X, int64_t n, int F, int ld, int k, const float* init, double tol, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = km_check("eagcn_kmeans_begin", X, n, F, ld, k)) return rc;
    EAGCN_CHECK_ARG(init, "eagcn_kmeans_begin: init is null");
    EAGCN_CHECK_ARG(tol >= 0.0, "eagcn_kmeans_begin: tol = %g is negative", tol);
    if (int rc = km_check_ws("eagcn_kmeans_begin", workspace, workspace_bytes, n, F, k)) return rc;
    const KmWs w = km_layout(workspace, n, F, k);
    const int F4 = pad4(F);
    EAGCN_HIP(hipMemcpyAsync(w.cen, init, (size_t)k * F * 4, hipMemcpyDeviceToDevice, s));
    EAGCN_HIP(hipMemsetAsync(w.labels, 0xff, (size_t)n * 4, s));                 // -1: every label changes in the first iteration
    if (km_vec(X, ld)) km_colstat_kernel<true><<<w.G, KM_THREADS, 0, s>>>(X, (int)n, F, ld, w.slabs);
    else km_colstat_kernel<false><<<w.G, KM_THREADS, 0, s>>>(X, (int)n, F, ld, w.slabs);
    EAGCN_LAUNCH_CHECK();
    km_var_kernel<<<cdiv(F4, KM_RED_COLS), KM_THREADS, 0, s>>>((int)n, F, w.G, w.slabs, w.parts);
    EAGCN_LAUNCH_CHECK();
    km_begin_kernel<<<1, WAVE, 0, s>>>(w.st, F, tol, w.parts, w.counts);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

extern "C" int eagcn_kmeans_iterate(const float* X, int64_t n, int F, int ld, int k, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = km_check("eagcn_kmeans_iterate", X, n, F, ld, k)) return rc;
    if (int rc = km_check_ws("eagcn_kmeans_iterate", workspace, workspace_bytes, n, F, k)) return rc;
    const KmWs w = km_layout(workspace, n, F, k);
    const int nblk = cdiv(k * pad4(F), KM_RED_COLS);
    if (int rc = km_assign<true>(X, n, F, ld, k, w.cen, w, w.labels, w.mind, s)) return rc;
    km_reduce_kernel<<<nblk, KM_THREADS, 0, s>>>(w.st, w.cen, F, k, w.G, w.slabs, w.wgcnt, w.counts, w.parts);
    EAGCN_LAUNCH_CHECK();
    km_decide_kernel<<<1, WAVE, 0, s>>>(w.st, k, w.G, nblk, w.wgchg, w.wgine, w.parts, w.counts);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

extern "C" int eagcn_kmeans_finish(const float* X, int64_t n, int F, int ld, int k, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = km_check("eagcn_kmeans_finish", X, n, F, ld, k)) return rc;
    if (int rc = km_check_ws("eagcn_kmeans_finish", workspace, workspace_bytes, n, F, k)) return rc;
    const KmWs w = km_layout(workspace, n, F, k);
    if (int rc = km_assign<false>(X, n, F, ld, k, w.cen, w, w.labels, w.mind, s)) return rc;
    km_finish_kernel<<<1, WAVE, 0, s>>>(w.st, k, w.G, w.wgcnt, w.wgine, w.counts);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}
