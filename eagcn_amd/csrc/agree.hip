// Agreement of a regression's predictions with its targets, and the thresholded metrics of a classification, over the device-resident
// buffers of an evaluation pass (eagcn_eval_append: scores / targets fp32, valid uint8, row-major [rows][T]) -- the technique of
// metrics.hip carried over: rank statistics as exact integer pair counts, no sort, no float atomic, no host read.
//   regression:     per task R^2 (sklearn r2_score), Pearson r (scipy pearsonr; its square is the reference's rsquared, utils.py:714),
//                   Spearman rho and Kendall tau-b,
//   classification: log-loss, Brier score, the confusion counts at a threshold and accuracy / precision / recall / F1 / MCC from them.
// For the valid entries i, j of a task (n of them)
//     lt_s_i = #{j: s_j < s_i}   eq_s_i = #{j: s_j == s_i} (i itself included)   lt_y_i, eq_y_i likewise   S_i = sum_j sgn(s_i - s_j) sgn(y_i - y_j)
//     a_i = 2 lt_s_i + eq_s_i - n = 2 (average rank of s_i) - (n + 1), b_i likewise:   rho = sum ab / sqrt(sum a^2  sum b^2)
//     n0 = n (n - 1) / 2, n1 = sum (eq_s_i - 1) / 2, n2 = sum (eq_y_i - 1) / 2:          tau_b = (sum S_i / 2) / sqrt((n0 - n1) (n0 - n2))
// all integers.  The moments behind r and R^2 are fp64 sums centred per tile of AGR_R entries (count, means, centred second moments) and
// merged in tile order by the pairwise update of Chan, Golub and LeVeque: no raw sum of squares is ever formed.
//
// Two launches per call: agree_pair_kernel (or agree_class_kernel) fills workspace words that belong to one workgroup each, the
// finalize adds them up in a fixed order -- bit-identical from run to run, and the workspace is never cleared.  A workgroup of the pair
// kernel holds AGR_R entries i of one task and walks the task's rows; where the tiles alone would leave most CUs idle up to
// AGR_MAX_SPLIT workgroups share a tile's rows, each leaves its part of the per-entry counts, and the finalize forms a, b and the sums
// from the counts added up (a lane has only a part of them).
#include "common.h"
#include "kernels.h"

namespace eagcn {

constexpr int AGR_R = 256;           // entries i of a workgroup (one per lane)
constexpr int AGR_J = 1024;          // entries j staged into LDS at a time
constexpr int AGR_MAX_SPLIT = 8;     // workgroups that share the j range of one tile at the most
constexpr int AGR_TARGET_WGS = 1024; // four workgroups of four waves per CU
constexpr int AGR_CHIP_WGS = 256;    // one workgroup per CU: a launch of that many tiles is not split
constexpr int AGR_FIN_THREADS = 256;     // (the finalize is latency-bound scalar work: more threads only cost registers)
constexpr int AGR_MERGE = 16;        // fan-in of the two upper levels of the moment merge (AGR_MERGE^2 threads merge tile ranges)
constexpr int AGR_PLANES = 5;        // 32-bit counts per entry and j range: lt_s, eq_s, lt_y, eq_y, S
// sum a^2 <= n (n^2 - 1) / 3 (no ties) < 2^63 up to this n, |sum ab| and every partial sum of |ab| <= (sum a^2 + sum b^2) / 2 likewise:
// up to it the three sums are taken in 64-bit integers, beyond it in fp64
constexpr long long AGR_INT_N = 3000000;

struct AgrTile {                     // what the workgroup (tile, split 0, t) of agree_pair_kernel leaves (128 bytes)
    uint32_t cnt, bad;               // valid entries of the tile | those whose score or target is not finite
    double ms, my;                   // their mean score and target
    double css, cyy, csy, sse;       // sum (s - ms)^2, (y - my)^2, (s - ms)(y - my), (y - s)^2
    // not split only (zero otherwise): the tile's part of the rank sums, the lanes' counts being complete
    double dab, daa, dbb;            // sum ab, a^2, b^2 in fp64 (used where n > AGR_INT_N)
    unsigned long long iab, iaa, ibb;// ... in wrapping 64-bit integers (used, and exact, where n <= AGR_INT_N)
    long long S;                     // sum S_i
    unsigned long long e1, e2;       // sum (eq_s - 1), sum (eq_y - 1)
};
struct AgrCls {                      // one workgroup of agree_class_kernel (40 bytes)
    double ll, br;                   // sum of the log-loss terms, of (p - y)^2, over the tile's labelled entries with a finite score
    uint32_t tp, fp, tn, fn, bad, pad;
};
static_assert(sizeof(AgrTile) == 128 && sizeof(AgrCls) <= 128, "the workspace formula of eagcn_hip.h counts 128 bytes per tile");

static inline int64_t agr_tiles(int64_t rows) { return (rows + AGR_R - 1) / AGR_R; }
static inline int64_t agr_chunks(int64_t rows) { return (rows + AGR_J - 1) / AGR_J; }
size_t agree_workspace_bytes(int64_t rows, int T) {
    const int64_t chunks = agr_chunks(rows);
    const int64_t smax = chunks < AGR_MAX_SPLIT ? chunks : AGR_MAX_SPLIT;
    return (size_t)T * (size_t)agr_tiles(rows) * ((size_t)smax * AGR_R * AGR_PLANES * 4 + sizeof(AgrTile));
}
// How many workgroups share a tile's j range (each takes `per` chunks of AGR_J, never an empty one): the rule of metrics.hip's
// eval_split -- one, unless the tiles alone leave CUs idle and the task has many rows for its width.
static inline void agr_split(int64_t rows, int T, int* nsplit, int* per) {
    const int64_t chunks = agr_chunks(rows), wgs = agr_tiles(rows) * T;
    int64_t s = (wgs < AGR_CHIP_WGS && rows >= (int64_t)AGR_J * T) ? AGR_TARGET_WGS / wgs : 1;
    s = s < 1 ? 1 : (s > AGR_MAX_SPLIT ? AGR_MAX_SPLIT : s);
    if (s > chunks) s = chunks;
    *per = (int)((chunks + s - 1) / s);
    *nsplit = (int)((chunks + *per - 1) / *per);
}
int agree_splits(int64_t rows, int T) {
    int nsplit, per;
    agr_split(rows, T, &nsplit, &per);
    return nsplit;
}

__device__ __forceinline__ unsigned long long agr_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ long long agr_wave_sum(long long v) { return (long long)agr_wave_sum((unsigned long long)v); }
__device__ __forceinline__ uint32_t agr_wave_sum(uint32_t v) { return (uint32_t)wave_sum((int)v); }
__device__ __forceinline__ double agr_wave_sum(double v) { return wave_sum(v); }

// sum of one value per thread over a workgroup of NT threads, in a fixed order (lanes by butterfly, waves in wave order); every thread
// gets it.  s_buf: NT / WAVE words of 8 bytes.
template <int NT, typename V>
__device__ __forceinline__ V agr_block_sum(V v, unsigned long long* s_buf) {
    static_assert(sizeof(V) <= 8, "one 8-byte word per wave");
    V* buf = reinterpret_cast<V*>(s_buf);
    v = agr_wave_sum(v);
    __syncthreads();                                      // s_buf may still be read from the sum before
    if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
    __syncthreads();
    V tot = 0;
    for (int k = 0; k < NT / WAVE; ++k) tot += buf[k];
    return tot;
}

// The flat elements of a row-major [rows][T] block, visited by a workgroup of AGR_R threads with loads that are contiguous over the
// lanes; a thread follows (row, column) of its element without a division per step.
struct AgrWalk {
    int T, q, r, row, col;
    __device__ AgrWalk(int T_, int tid) : T(T_), q(AGR_R / T_), r(AGR_R % T_), row(tid / T_), col(tid % T_) {}
    __device__ void next() {
        row += q;
        col += r;
        if (col >= T) { col -= T; ++row; }
    }
};

// a, b and the rank sums of one entry from its complete counts (eq_s == 0: not a valid entry -- a valid one counts itself)
struct AgrRank {
    unsigned long long iab = 0, iaa = 0, ibb = 0, e1 = 0, e2 = 0;
    double dab = 0.0, daa = 0.0, dbb = 0.0;
    long long S = 0;
    __device__ __forceinline__ void add(uint32_t lt_s, uint32_t eq_s, uint32_t lt_y, uint32_t eq_y, int Si, long long n) {
        if (eq_s == 0 || eq_y == 0) return;
        const long long a = 2ll * lt_s + eq_s - n, b = 2ll * lt_y + eq_y - n;      // |a|, |b| < n < 2^31: the products fit 64 bits
        const long long ab = a * b, aa = a * a, bb = b * b;
        iab += (unsigned long long)ab; iaa += (unsigned long long)aa; ibb += (unsigned long long)bb;
        dab += (double)ab; daa += (double)aa; dbb += (double)bb;
        S += Si;
        e1 += eq_s - 1;
        e2 += eq_y - 1;
    }
};

// grid (tiles, nsplit, T).  Lane `tid` holds entry i = tile * AGR_R + tid of task t (score and target, NaN where it is not valid: a NaN
// compares false with everything, so such a lane counts nothing) and walks the rows [jlo, jhi) of the task in chunks of AGR_J staged
// into LDS as two arrays, NaN where the entry is not valid: the validity test is paid once per staged entry, not once per pair.  In
// the pair loop every lane reads the same 16 bytes (a broadcast); the six compares of a pair leave lane masks, the sign product is
// formed from the masks.
__global__ __launch_bounds__(AGR_R) void agree_pair_kernel(const float* __restrict__ scores, const float* __restrict__ targets,
                                                            const uint8_t* __restrict__ valid, int rows, int T, int per,
                                                            uint32_t* __restrict__ counts, AgrTile* __restrict__ tiles_out) {
    __shared__ __attribute__((aligned(16))) float s_s[AGR_J];
    __shared__ __attribute__((aligned(16))) float s_y[AGR_J];
    __shared__ unsigned long long s_red[AGR_R / WAVE];
    const int tid = threadIdx.x, tile = blockIdx.x, split = blockIdx.y, t = blockIdx.z;
    const int tiles = gridDim.x, nsplit = gridDim.y;
    const float qnan = __int_as_float(0x7fc00000);

    const long long i = (long long)tile * AGR_R + tid;
    float si = qnan, yi = qnan;
    bool vi = false;
    if (i < rows) {
        const size_t e = (size_t)i * T + t;
        if (valid[e]) { vi = true; si = scores[e]; yi = targets[e]; }
    }
    const long long span = (long long)per * AGR_J;         // (64-bit: rows may be close to 2^31)
    const int jlo = (int)min((long long)rows, split * span), jhi = (int)min((long long)rows, jlo + span);
    uint32_t lt_s = 0, eq_s = 0, lt_y = 0, eq_y = 0, nv = 0;
    int S = 0;
    for (int j0 = jlo; j0 < jhi; j0 += AGR_J) {
        const int nj = min(AGR_J, jhi - j0);
        const size_t base = (size_t)j0 * T, n_el = (size_t)nj * T;
        __syncthreads();                                  // the pair loop of the chunk before has read the arrays
        AgrWalk w(T, tid);
        for (size_t e = tid; e < n_el; e += AGR_R, w.next()) {
            const float s = scores[base + e], y = targets[base + e];
            const bool ok = valid[base + e] != 0;
            if (w.col == t) {
                s_s[w.row] = ok ? s : qnan;
                s_y[w.row] = ok ? y : qnan;
                nv += ok;
            }
        }
        const int nj8 = (nj + 7) & ~7;                     // the pair loop takes eight entries per step
        if (nj + tid < nj8) s_s[nj + tid] = s_y[nj + tid] = qnan;
        __syncthreads();
        for (int j = 0; j < nj8; j += 8) {
            const float4 a0 = *reinterpret_cast<const float4*>(s_s + j), a1 = *reinterpret_cast<const float4*>(s_s + j + 4);
            const float4 b0 = *reinterpret_cast<const float4*>(s_y + j), b1 = *reinterpret_cast<const float4*>(s_y + j + 4);
            const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bool ls = a[u] < si, es = a[u] == si, gs = a[u] > si;
                const bool ly = b[u] < yi, ey = b[u] == yi, gy = b[u] > yi;
                lt_s += ls ? 1u : 0u;
                eq_s += es ? 1u : 0u;
                lt_y += ly ? 1u : 0u;
                eq_y += ey ? 1u : 0u;
                S += ((ls && ly) || (gs && gy)) ? 1 : 0;
                S -= ((ls && gy) || (gs && ly)) ? 1 : 0;
            }
        }
    }
    AgrRank rk;
    if (nsplit > 1) {
        // the per-entry counts of this j range (zero on every lane that is not valid) go to the finalize, which adds the ranges
        const size_t plane = (size_t)T * nsplit * tiles * AGR_R;
        const size_t at = ((size_t)(t * nsplit + split) * tiles + tile) * AGR_R + tid;
        counts[at] = lt_s;
        counts[plane + at] = eq_s;
        counts[2 * plane + at] = lt_y;
        counts[3 * plane + at] = eq_y;
        counts[4 * plane + at] = (uint32_t)S;
        if (split != 0) return;                           // (uniform over the workgroup)
    } else {
        // the workgroup has staged every row of the task: the lanes' counts are complete and the staged valid entries are the task's n
        const long long n = agr_block_sum<AGR_R>(nv, s_red);
        rk.add(lt_s, eq_s, lt_y, eq_y, S, n);
    }
    AgrTile o;
    o.iab = agr_block_sum<AGR_R>(rk.iab, s_red);
    o.iaa = agr_block_sum<AGR_R>(rk.iaa, s_red);
    o.ibb = agr_block_sum<AGR_R>(rk.ibb, s_red);
    o.dab = agr_block_sum<AGR_R>(rk.dab, s_red);
    o.daa = agr_block_sum<AGR_R>(rk.daa, s_red);
    o.dbb = agr_block_sum<AGR_R>(rk.dbb, s_red);
    o.S = agr_block_sum<AGR_R>(rk.S, s_red);
    o.e1 = agr_block_sum<AGR_R>(rk.e1, s_red);
    o.e2 = agr_block_sum<AGR_R>(rk.e2, s_red);
    // the tile's moments, centred on the tile's own means
    const double ds = vi ? (double)si : 0.0, dy = vi ? (double)yi : 0.0;
    o.cnt = agr_block_sum<AGR_R>(vi ? 1u : 0u, s_red);
    o.bad = agr_block_sum<AGR_R>((vi && !(isfinite(si) && isfinite(yi))) ? 1u : 0u, s_red);
    const double inv = o.cnt ? 1.0 / (double)o.cnt : 0.0;
    o.ms = agr_block_sum<AGR_R>(ds, s_red) * inv;
    o.my = agr_block_sum<AGR_R>(dy, s_red) * inv;
    const double cs = vi ? ds - o.ms : 0.0, cy = vi ? dy - o.my : 0.0, d = dy - ds;
    o.css = agr_block_sum<AGR_R>(cs * cs, s_red);
    o.cyy = agr_block_sum<AGR_R>(cy * cy, s_red);
    o.csy = agr_block_sum<AGR_R>(cs * cy, s_red);
    o.sse = agr_block_sum<AGR_R>(d * d, s_red);
    if (tid == 0) tiles_out[(size_t)t * tiles + tile] = o;
}

struct AgrMom { double n, ms, my, css, cyy, csy, sse; };
// b merged behind a (Chan, Golub, LeVeque 1979: the pairwise update of means and centred second moments)
__device__ __forceinline__ AgrMom agr_merge(const AgrMom& a, const AgrMom& b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    AgrMom o;
    o.n = a.n + b.n;
    const double ds = b.ms - a.ms, dy = b.my - a.my, f = b.n / o.n, w = a.n * f;
    o.ms = a.ms + ds * f;
    o.my = a.my + dy * f;
    o.css = a.css + b.css + ds * ds * w;
    o.cyy = a.cyy + b.cyy + dy * dy * w;
    o.csy = a.csy + b.csy + ds * dy * w;
    o.sse = a.sse + b.sse;
    return o;
}

// One workgroup.  out = [r2 T | pearson T | spearman T | kendall T | count T | bad T | mean_r2 | mean_pearson | mean_spearman |
// mean_kendall]; a task with bad > 0 or n < 2 is NaN in all four, a constant column as the header says; the means run over the tasks
// that are not NaN.
__global__ __launch_bounds__(AGR_FIN_THREADS) void agree_reg_finalize_kernel(const AgrTile* __restrict__ tile_recs,
                                                                              const uint32_t* __restrict__ counts, int rows, int T,
                                                                              int tiles, int nsplit, double* __restrict__ out) {
    __shared__ unsigned long long s_red[AGR_FIN_THREADS / WAVE];
    __shared__ AgrMom s_mom[AGR_MERGE * AGR_MERGE];
    const int tid = threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, c0 = 0.0, c1 = 0.0;   // running sums over the tasks, tasks with an r2 / with the other
                                                                         // three (thread 0)
    const size_t plane = (size_t)T * nsplit * tiles * AGR_R;
    for (int t = 0; t < T; ++t) {
        const AgrTile* recs = tile_recs + (size_t)t * tiles;
        // the moments: thread k < AGR_MERGE^2 merges a contiguous range of tiles in tile order, then AGR_MERGE threads merge AGR_MERGE
        // of those each, then thread 0 the rest (into s_mom[0]) -- always the same tree for the same shape
        __syncthreads();                                  // s_mom of the task before has been read
        if (tid < AGR_MERGE * AGR_MERGE) {
            const int each = (tiles + AGR_MERGE * AGR_MERGE - 1) / (AGR_MERGE * AGR_MERGE);
            const int lo = min(tiles, tid * each), hi = min(tiles, lo + each);
            AgrMom acc = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
            for (int k = lo; k < hi; ++k) {
                const AgrTile o = recs[k];
                const AgrMom b = {(double)o.cnt, o.ms, o.my, o.css, o.cyy, o.csy, o.sse};
                acc = agr_merge(acc, b);
            }
            s_mom[tid] = acc;
        }
        __syncthreads();
        if (tid < AGR_MERGE) {
            AgrMom acc = s_mom[tid * AGR_MERGE];
#pragma unroll 1
            for (int k = 1; k < AGR_MERGE; ++k) acc = agr_merge(acc, s_mom[tid * AGR_MERGE + k]);
            s_mom[tid * AGR_MERGE] = acc;                 // (only this thread reads the words it overwrites)
        }
        __syncthreads();
        if (tid == 0) {                                   // (ahead of the rank sums: the merge is heavy on registers)
            AgrMom mo = s_mom[0];
#pragma unroll 1
            for (int k = 1; k < AGR_MERGE; ++k) mo = agr_merge(mo, s_mom[k * AGR_MERGE]);
            s_mom[0] = mo;
        }
        unsigned long long nb = 0;                        // count in the high, bad in the low half
        for (int k = tid; k < tiles; k += AGR_FIN_THREADS) nb += ((unsigned long long)recs[k].cnt << 32) | recs[k].bad;
        nb = agr_block_sum<AGR_FIN_THREADS>(nb, s_red);
        const long long n = (long long)(nb >> 32), bad = (long long)(nb & 0xffffffffull);
        AgrRank rk;
        if (nsplit > 1) {
#pragma unroll 1
            for (long long r = tid; r < rows; r += AGR_FIN_THREADS) {      // (64-bit: rows may be close to 2^31)
                uint32_t c[AGR_PLANES] = {0, 0, 0, 0, 0};
#pragma unroll 1
                for (int s = 0; s < nsplit; ++s) {
                    const size_t at = (size_t)(t * nsplit + s) * tiles * AGR_R + r;
#pragma unroll
                    for (int p = 0; p < AGR_PLANES; ++p) c[p] += counts[p * plane + at];
                }
                rk.add(c[0], c[1], c[2], c[3], (int)c[4], n);
            }
        } else {
            for (int k = tid; k < tiles; k += AGR_FIN_THREADS) {
                const AgrTile o = recs[k];
                rk.iab += o.iab; rk.iaa += o.iaa; rk.ibb += o.ibb;
                rk.dab += o.dab; rk.daa += o.daa; rk.dbb += o.dbb;
                rk.S += o.S; rk.e1 += o.e1; rk.e2 += o.e2;
            }
        }
        const unsigned long long iab = agr_block_sum<AGR_FIN_THREADS>(rk.iab, s_red);
        const unsigned long long iaa = agr_block_sum<AGR_FIN_THREADS>(rk.iaa, s_red);
        const unsigned long long ibb = agr_block_sum<AGR_FIN_THREADS>(rk.ibb, s_red);
        const double dab = agr_block_sum<AGR_FIN_THREADS>(rk.dab, s_red);
        const double daa = agr_block_sum<AGR_FIN_THREADS>(rk.daa, s_red);
        const double dbb = agr_block_sum<AGR_FIN_THREADS>(rk.dbb, s_red);
        const long long S = agr_block_sum<AGR_FIN_THREADS>(rk.S, s_red);
        const unsigned long long e1 = agr_block_sum<AGR_FIN_THREADS>(rk.e1, s_red);
        const unsigned long long e2 = agr_block_sum<AGR_FIN_THREADS>(rk.e2, s_red);
        if (tid == 0) {
            const AgrMom mo = s_mom[0];
            double r2 = nan, pearson = nan, spearman = nan, kendall = nan;
            if (bad == 0 && n >= 2) {
                const long long n0 = n * (n - 1) / 2, n1 = (long long)(e1 / 2), n2 = (long long)(e2 / 2);
                const bool s_varies = n0 > n1, y_varies = n0 > n2;          // a constant column: every pair is tied
                if (y_varies) { r2 = 1.0 - mo.sse / mo.cyy; m0 += r2; c0 += 1.0; }
                if (s_varies && y_varies) {
                    pearson = mo.csy / sqrt(mo.css * mo.cyy);
                    const bool ints = n <= AGR_INT_N;
                    const double ab = ints ? (double)(long long)iab : dab, aa = ints ? (double)iaa : daa, bb = ints ? (double)ibb : dbb;
                    spearman = ab / sqrt(aa * bb);
                    kendall = (double)(S / 2) / (sqrt((double)(n0 - n1)) * sqrt((double)(n0 - n2)));
                    m1 += pearson; m2 += spearman; m3 += kendall; c1 += 1.0;
                }
            }
            out[t] = r2;
            out[T + t] = pearson;
            out[2 * T + t] = spearman;
            out[3 * T + t] = kendall;
            out[4 * T + t] = (double)n;
            out[5 * T + t] = (double)bad;
        }
    }
    if (tid == 0) {
        out[6 * T] = c0 > 0.0 ? m0 / c0 : nan;
        out[6 * T + 1] = c1 > 0.0 ? m1 / c1 : nan;
        out[6 * T + 2] = c1 > 0.0 ? m2 / c1 : nan;
        out[6 * T + 3] = c1 > 0.0 ? m3 / c1 : nan;
    }
}

// grid (tiles, T): over the labelled entries (valid, target 0 or 1) of AGR_R rows of one task the fp64 sums of the log-loss terms and
// of (p - y)^2, p = the score clipped to [2^-52, 1 - 2^-52], and the confusion counts at `threshold` (positive: score > threshold)
__global__ __launch_bounds__(AGR_R) void agree_class_kernel(const float* __restrict__ scores, const float* __restrict__ targets,
                                                             const uint8_t* __restrict__ valid, int rows, int T, float threshold,
                                                             AgrCls* __restrict__ slots) {
    __shared__ unsigned long long s_red[AGR_R / WAVE];
    const int tid = threadIdx.x, tile = blockIdx.x, t = blockIdx.y, tiles = gridDim.x;
    const int j0 = tile * AGR_R, nj = min(AGR_R, rows - j0);
    const size_t base = (size_t)j0 * T, n_el = (size_t)nj * T;
    const double eps = 2.220446049250313e-16;             // 2^-52
    double ll = 0.0, br = 0.0;
    uint32_t tp = 0, fp = 0, tn = 0, fn = 0, bad = 0;
    AgrWalk w(T, tid);
    for (size_t e = tid; e < n_el; e += AGR_R, w.next()) {
        const float s = scores[base + e], y = targets[base + e];
        const bool ok = valid[base + e] != 0;
        if (w.col == t && ok && (y == 0.0f || y == 1.0f)) {
            const bool pos = y == 1.0f, pred = s > threshold;
            tp += pos && pred;
            fn += pos && !pred;
            fp += !pos && pred;
            tn += !pos && !pred;
            if (isfinite(s)) {
                const double p = fmin(fmax((double)s, eps), 1.0 - eps);
                ll -= log(pos ? p : 1.0 - p);
                const double d = p - (pos ? 1.0 : 0.0);
                br += d * d;
            } else {
                ++bad;
            }
        }
    }
    AgrCls o;
    o.ll = agr_block_sum<AGR_R>(ll, s_red);
    o.br = agr_block_sum<AGR_R>(br, s_red);
    o.tp = agr_block_sum<AGR_R>(tp, s_red);
    o.fp = agr_block_sum<AGR_R>(fp, s_red);
    o.tn = agr_block_sum<AGR_R>(tn, s_red);
    o.fn = agr_block_sum<AGR_R>(fn, s_red);
    o.bad = agr_block_sum<AGR_R>(bad, s_red);
    o.pad = 0;
    if (tid == 0) slots[(size_t)t * tiles + tile] = o;
}

// One workgroup.  out = [log_loss T | brier T | tp T | fp T | tn T | fn T | accuracy T | precision T | recall T | f1 T | mcc T | bad T |
// mean_log_loss | mean_brier | mean_f1 | mean_mcc]
__global__ __launch_bounds__(AGR_FIN_THREADS) void agree_class_finalize_kernel(const AgrCls* __restrict__ slots, int T, int tiles,
                                                                                double* __restrict__ out) {
    __shared__ unsigned long long s_red[AGR_FIN_THREADS / WAVE];
    const int tid = threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, mc = 0.0;
    for (int t = 0; t < T; ++t) {
        double ll = 0.0, br = 0.0;
        unsigned long long tp = 0, fp = 0, tn = 0, fn = 0, bad = 0;
        for (int k = tid; k < tiles; k += AGR_FIN_THREADS) {
            const AgrCls o = slots[(size_t)t * tiles + k];
            ll += o.ll; br += o.br;
            tp += o.tp; fp += o.fp; tn += o.tn; fn += o.fn; bad += o.bad;
        }
        ll = agr_block_sum<AGR_FIN_THREADS>(ll, s_red);
        br = agr_block_sum<AGR_FIN_THREADS>(br, s_red);
        tp = agr_block_sum<AGR_FIN_THREADS>(tp, s_red);
        fp = agr_block_sum<AGR_FIN_THREADS>(fp, s_red);
        tn = agr_block_sum<AGR_FIN_THREADS>(tn, s_red);
        fn = agr_block_sum<AGR_FIN_THREADS>(fn, s_red);
        bad = agr_block_sum<AGR_FIN_THREADS>(bad, s_red);
        if (tid == 0) {
            const unsigned long long n = tp + fp + tn + fn;                // < 2^31 each
            const bool ok = n > 0 && bad == 0;
            const double dn = (double)n;
            const long long num = (long long)(tp * tn) - (long long)(fp * fn);      // each product < 2^62
            const double den = sqrt((double)((tp + fp) * (tp + fn)) * (double)((tn + fp) * (tn + fn)));
            const double f1 = 2 * tp + fp + fn ? (double)(2 * tp) / (double)(2 * tp + fp + fn) : 0.0;
            const double mcc = den > 0.0 ? (double)num / den : 0.0;
            out[t] = ok ? ll / dn : nan;
            out[T + t] = ok ? br / dn : nan;
            out[2 * T + t] = ok ? (double)tp : nan;
            out[3 * T + t] = ok ? (double)fp : nan;
            out[4 * T + t] = ok ? (double)tn : nan;
            out[5 * T + t] = ok ? (double)fn : nan;
            out[6 * T + t] = ok ? (double)(tp + tn) / dn : nan;
            out[7 * T + t] = ok ? (tp + fp ? (double)tp / (double)(tp + fp) : 0.0) : nan;
            out[8 * T + t] = ok ? (tp + fn ? (double)tp / (double)(tp + fn) : 0.0) : nan;
            out[9 * T + t] = ok ? f1 : nan;
            out[10 * T + t] = ok ? mcc : nan;
            out[11 * T + t] = (double)bad;
            if (ok) { m0 += ll / dn; m1 += br / dn; m2 += f1; m3 += mcc; mc += 1.0; }
        }
    }
    if (tid == 0) {
        out[12 * T] = mc > 0.0 ? m0 / mc : nan;
        out[12 * T + 1] = mc > 0.0 ? m1 / mc : nan;
        out[12 * T + 2] = mc > 0.0 ? m2 / mc : nan;
        out[12 * T + 3] = mc > 0.0 ? m3 / mc : nan;
    }
}

int64_t agree_tiles(int64_t rows) { return agr_tiles(rows); }

int launch_agree_reg(const float* scores, const float* targets, const uint8_t* valid, int64_t rows, int T, void* workspace, double* out,
                     hipStream_t s) {
    int nsplit, per;
    agr_split(rows, T, &nsplit, &per);
    const int tiles = (int)agr_tiles(rows);
    AgrTile* recs = static_cast<AgrTile*>(workspace);
    uint32_t* counts = reinterpret_cast<uint32_t*>(recs + (size_t)T * tiles);
    agree_pair_kernel<<<dim3(tiles, nsplit, T), AGR_R, 0, s>>>(scores, targets, valid, (int)rows, T, per, counts, recs);
    EAGCN_LAUNCH_CHECK();
    agree_reg_finalize_kernel<<<1, AGR_FIN_THREADS, 0, s>>>(recs, counts, (int)rows, T, tiles, nsplit, out);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

int launch_agree_class(const float* scores, const float* targets, const uint8_t* valid, int64_t rows, int T, float threshold,
                       void* workspace, double* out, hipStream_t s) {
    const int tiles = (int)agr_tiles(rows);
    AgrCls* slots = static_cast<AgrCls*>(workspace);
    agree_class_kernel<<<dim3(tiles, T), AGR_R, 0, s>>>(scores, targets, valid, (int)rows, T, threshold, slots);
    EAGCN_LAUNCH_CHECK();
    agree_class_finalize_kernel<<<1, AGR_FIN_THREADS, 0, s>>>(slots, T, tiles, out);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

}  // namespace eagcn
