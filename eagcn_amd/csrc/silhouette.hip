// Scores of a clustering of device rows (the number behind the reference's kmeans_atomrep.py, which reads its confusion matrix by eye):
// the silhouette coefficient of every row, and the per-cluster centres, scatter and within-cluster sums of squares from which the
// Davies-Bouldin and Calinski-Harabasz indices follow.  Semantics in include/eagcn_hip.h; no floating-point atomics, no host read, no
// n x n buffer; every fp64 sum in an order that depends on the labels, n and the slab count only.
//
//   sil_hist_kernel /   a deterministic counting sort of the row indices by label: a wave counts the labels of its own stretch of rows
//   sil_scan_kernel /   (ballots, counters in registers), one workgroup scans the waves' histograms column by column, the waves then
//   sil_scatter_kernel  write their rows' indices behind their offsets -- row index ascending inside a cluster.  A permutation only:
//                       X is never copied.  Rows whose label is outside 0 .. k - 1 are left out.
//   sil_tiles_kernel    every cluster cut into data tiles of 64 of its own rows: (cluster, first position, rows) per tile, -1 behind
//                       the last real tile (the launch below is sized by the host-known bound ceil(n / 64) + k).
//   sil_sum_kernel      grid (query tiles, slabs): kn_tile (csrc/dist_tile.h) with the data rows taken through the permutation; a
//                       thread adds the roots of its 4 x 4 block, column by column, to four fp64 accumulators (one per query row)
//                       and flushes them -- a fixed xor tree over the 16 lanes of a query row -- when the cluster changes or the slab
//                       ends: part [slab][row][cluster].
//   sil_finish_kernel   a thread per row: the slabs that hold tiles of a cluster summed in slab order, then a, b and s.
//   sil_mean_kernel /   a workgroup per cluster: its rows' samples summed per thread in row order, then a fixed tree; the cluster
//   sil_total_kernel    sums in cluster order give the mean over all scored rows.
//   cm_*                centres, scatter and sums of squares over the same cluster order (eagcn_cluster_moments).
#include "dist_tile.h"

namespace eagcn {

constexpr int SIL_MAX_K = EAGCN_SIL_MAX_K;
constexpr int SIL_SORT_ROWS = 1024;   // a wave of the counting sort takes at least this many rows ...
constexpr int SIL_SORT_WAVES = 1024;  // ... and there are at most this many waves
constexpr int CM_SPLIT_ROWS = 8192;   // moments: the rows of every cluster are cut into ceil(n / this) parts ...
constexpr int CM_MAX_SPLITS = 16;     // ... at most this many
static_assert(SIL_MAX_K <= 4 * WAVE, "a lane of the counting sort holds the counters of four clusters");

// ---- counting sort -----------------------------------------------------------------------------------------------------------------
// One wave over the rows [r0, r1): lane L holds the counters of the clusters L, L + 64, L + 128, L + 192.  Per 64 rows the distinct
// labels are taken one at a time (ballot); a row's place is its cluster's counter plus the number of lower lanes with the same label.
template <bool SCATTER>
__device__ __forceinline__ void sil_wave_pass(const int32_t* __restrict__ labels, int k, int64_t r0, int64_t r1, int (&cnt)[4], int& ign,
                                              int32_t* __restrict__ perm) {
    const int lane = threadIdx.x & (WAVE - 1);
    for (int64_t base = r0; base < r1; base += WAVE) {
        const int64_t i = base + lane;
        const bool in = i < r1;
        const int l = in ? labels[i] : -1;
        const bool ok = in && l >= 0 && l < k;
        ign += (in && !ok) ? 1 : 0;
        uint64_t todo = __ballot(ok);
        while (todo) {
            const int cl = __shfl(l, __ffsll((unsigned long long)todo) - 1);      // (wave-uniform)
            const bool mine = ok && l == cl;
            const uint64_t same = __ballot(mine);
            const int q = cl >> 6, src = cl & (WAVE - 1);
            const int held = q == 0 ? cnt[0] : q == 1 ? cnt[1] : q == 2 ? cnt[2] : cnt[3];
            const int off = __shfl(held, src);
            if (SCATTER && mine) perm[off + __popcll(same & ((1ull << lane) - 1ull))] = (int32_t)i;
            const int add = lane == src ? __popcll(same) : 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) cnt[j] += q == j ? add : 0;
            todo &= ~same;
        }
    }
}

// hist [W][k + 1]: the rows of every cluster in wave w's stretch [w chunk, (w + 1) chunk); column k counts the rows outside the labelling
__global__ __launch_bounds__(KN_THREADS) void sil_hist_kernel(const int32_t* __restrict__ labels, int64_t n, int k, int W, int64_t chunk,
                                                              int32_t* __restrict__ hist) {
    const int w = blockIdx.x * (KN_THREADS / WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & (WAVE - 1);
    if (w >= W) return;
    int cnt[4] = {0, 0, 0, 0}, ign = 0;
    const int64_t r0 = (int64_t)w * chunk, r1 = min(n, r0 + chunk);
    sil_wave_pass<false>(labels, k, r0, r1, cnt, ign, nullptr);
    ign = wave_sum(ign);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (lane + WAVE * j < k) hist[(size_t)w * (k + 1) + lane + WAVE * j] = cnt[j];
    if (lane == 0) hist[(size_t)w * (k + 1) + k] = ign;
}

// one workgroup: offs [W][k] = the first position of wave w's rows of cluster c in the cluster order; row_off / tile_off [k + 1] = the
// clusters' first positions and first tiles; counts [k]; stats[1 .. 3] = rows scored | non-empty clusters | rows ignored (may be null)
__global__ __launch_bounds__(KN_THREADS) void sil_scan_kernel(const int32_t* __restrict__ hist, int W, int k, int32_t* __restrict__ offs,
                                                              int32_t* __restrict__ row_off, int32_t* __restrict__ tile_off,
                                                              int64_t* __restrict__ counts, double* __restrict__ stats) {
    __shared__ int s_tot[SIL_MAX_K + 1], s_row[SIL_MAX_K + 1], s_tile[SIL_MAX_K + 1];
    const int tid = threadIdx.x;
    for (int c = tid; c <= k; c += KN_THREADS) {
        int tot = 0;
#pragma unroll 8
        for (int w = 0; w < W; ++w) tot += hist[(size_t)w * (k + 1) + c];
        s_tot[c] = tot;
    }
    __syncthreads();
    if (tid == 0) {
        int r = 0, t = 0, ne = 0;
        for (int c = 0; c < k; ++c) {
            s_row[c] = r;
            s_tile[c] = t;
            r += s_tot[c];
            t += (s_tot[c] + KN_TILE - 1) / KN_TILE;
            ne += s_tot[c] > 0 ? 1 : 0;
        }
        s_row[k] = r;
        s_tile[k] = t;
        if (stats) {
            stats[1] = (double)r;
            stats[2] = (double)ne;
            stats[3] = (double)s_tot[k];
        }
    }
    __syncthreads();
    for (int c = tid; c <= k; c += KN_THREADS) {
        row_off[c] = s_row[c];
        tile_off[c] = s_tile[c];
        if (c == k) break;
        counts[c] = s_tot[c];
        int run = s_row[c];
#pragma unroll 8
        for (int w = 0; w < W; ++w) {
            offs[(size_t)w * k + c] = run;
            run += hist[(size_t)w * (k + 1) + c];
        }
    }
}

// perm [rows scored]: the row indices in cluster order, ascending inside a cluster
__global__ __launch_bounds__(KN_THREADS) void sil_scatter_kernel(const int32_t* __restrict__ labels, int64_t n, int k, int W, int64_t chunk,
                                                                 const int32_t* __restrict__ offs, int32_t* __restrict__ perm) {
    const int w = blockIdx.x * (KN_THREADS / WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & (WAVE - 1);
    if (w >= W) return;
    int cnt[4], ign = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt[j] = lane + WAVE * j < k ? offs[(size_t)w * k + lane + WAVE * j] : 0;
    const int64_t r0 = (int64_t)w * chunk, r1 = min(n, r0 + chunk);
    sil_wave_pass<true>(labels, k, r0, r1, cnt, ign, perm);
}

// tiles [tb]: (cluster, first position in perm, rows, 0) of data tile t; cluster -1 behind the last real tile
__global__ __launch_bounds__(KN_THREADS) void sil_tiles_kernel(const int32_t* __restrict__ row_off, const int32_t* __restrict__ tile_off, int k,
                                                               int tb, int4* __restrict__ tiles) {
    for (int t = blockIdx.x * KN_THREADS + threadIdx.x; t < tb; t += gridDim.x * KN_THREADS) {
        int4 out = make_int4(-1, 0, 0, 0);
        if (t < tile_off[k]) {
            int lo = 0, hi = k;                             // tile_off[lo] <= t < tile_off[hi]: the last cluster that starts at or before t
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (tile_off[mid] <= t) lo = mid; else hi = mid;
            }
            const int p0 = row_off[lo] + (t - tile_off[lo]) * KN_TILE;
            out = make_int4(lo, p0, min(KN_TILE, row_off[lo + 1] - p0), 0);
        }
        tiles[t] = out;
    }
}

// ---- sums of distances -------------------------------------------------------------------------------------------------------------
// grid (ceil(n / 64), S): part [S][n][k], entry (y, i, c) = the sum of d(i, j) over the rows j of cluster c in the tiles
// [y per, (y + 1) per) -- written only where the slab holds a tile of c (sil_finish_kernel reads exactly those)
__global__ __launch_bounds__(KN_THREADS) void sil_sum_kernel(const float* __restrict__ X, int64_t n, int F, int ld, const int32_t* __restrict__ perm,
                                                             const int4* __restrict__ tiles, int k, int per, int tb, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sA[KN_KC][KN_PADT];
    __shared__ __attribute__((aligned(16))) float sB[KN_KC][KN_PADT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * KN_TILE;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    int cur = -1;
    auto flush = [&]() {                                    // (the whole workgroup is in one cluster: no lane is away)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            double v = sum[u];
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
            const int64_t i = i0 + ty * 4 + u;
            if (tx == 0 && i < n) part[((size_t)blockIdx.y * n + i) * k + cur] = v;
            sum[u] = 0.0;
        }
    };
    const int tbeg = blockIdx.y * per, tend = min(tb, tbeg + per);
    for (int t = tbeg; t < tend; ++t) {
        const int4 tt = tiles[t];                           // cluster | first position | rows
        if (tt.x < 0) break;                                // (behind the last real tile there are no more)
        if (tt.x != cur) {
            if (cur >= 0) flush();
            cur = tt.x;
        }
        float acc[4][4];
        kn_tile<true>(X, n, ld, X, (int64_t)tt.y + tt.z, ld, F, i0, (int64_t)tt.y, sA, sB, acc, perm);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (tx * 4 + v < tt.z) sum[u] += (double)__fsqrt_rn(acc[u][v]);
    }
    if (cur >= 0) flush();
}

// a thread per row: S[i][c] over the slabs in slab order, then the coefficient
__global__ __launch_bounds__(KN_THREADS) void sil_finish_kernel(const double* __restrict__ part, const int32_t* __restrict__ labels, int64_t n, int k,
                                                                int per, const int32_t* __restrict__ row_off, const int32_t* __restrict__ tile_off,
                                                                double* __restrict__ samples) {
    __shared__ int s_cnt[SIL_MAX_K], s_t0[SIL_MAX_K + 1];
    for (int c = threadIdx.x; c <= k; c += KN_THREADS) {
        s_t0[c] = tile_off[c];
        if (c < k) s_cnt[c] = row_off[c + 1] - row_off[c];
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * KN_THREADS + threadIdx.x;
    if (i >= n) return;
    const int own = labels[i];
    if (own < 0 || own >= k) {
        samples[i] = __longlong_as_double(0x7FF8000000000000ll);
        return;
    }
    double a_sum = 0.0, b = __longlong_as_double(0x7FF0000000000000ll);
    for (int c = 0; c < k; ++c) {
        if (s_cnt[c] == 0) continue;
        double sc = 0.0;
        for (int y = s_t0[c] / per; y <= (s_t0[c + 1] - 1) / per; ++y) sc += part[((size_t)y * n + i) * k + c];
        if (c == own) a_sum = sc;
        else b = fmin(b, sc / (double)s_cnt[c]);
    }
    double s = 0.0;
    if (s_cnt[own] > 1) {
        const double a = a_sum / (double)(s_cnt[own] - 1);
        s = (b - a) / fmax(a, b);
        if (s != s) s = 0.0;                                // (0 / 0, all rows alike, or no other cluster: scikit-learn's nan_to_num)
    }
    samples[i] = s;
}

// a workgroup per cluster: csum[c] = the sum of its rows' samples, cluster_mean[c] = their mean (NaN for an empty cluster)
__global__ __launch_bounds__(KN_THREADS) void sil_mean_kernel(const double* __restrict__ samples, const int32_t* __restrict__ perm,
                                                              const int32_t* __restrict__ row_off, double* __restrict__ csum,
                                                              double* __restrict__ cluster_mean) {
    __shared__ double s_v[KN_THREADS];
    const int c = blockIdx.x, tid = threadIdx.x, p0 = row_off[c], p1 = row_off[c + 1];
    double v = 0.0;
    for (int p = p0 + tid; p < p1; p += KN_THREADS) v += samples[perm[p]];
    s_v[tid] = v;
    for (int o = KN_THREADS / 2; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) s_v[tid] += s_v[tid + o];
    }
    if (tid == 0) {
        csum[c] = s_v[0];
        cluster_mean[c] = p1 > p0 ? s_v[0] / (double)(p1 - p0) : __longlong_as_double(0x7FF8000000000000ll);
    }
}

// stats[0] = the mean sample over the scored rows: the cluster sums in cluster order; NaN with fewer than two non-empty clusters
__global__ void sil_total_kernel(const double* __restrict__ csum, int k, double* __restrict__ stats) {
    if (threadIdx.x || blockIdx.x) return;
    double tot = 0.0;
    for (int c = 0; c < k; ++c) tot += csum[c];
    stats[0] = stats[2] >= 2.0 ? tot / stats[1] : __longlong_as_double(0x7FF8000000000000ll);
}

// ---- moments -----------------------------------------------------------------------------------------------------------------------
// grid (k, ceil(F / 64), R): psum [R][k][F] = the column sums of part z of cluster c's rows (cluster order cut into R stretches), fp64;
// a wave reads 64 adjacent columns of a row, its four waves take the rows in turn and are added in wave order
__global__ __launch_bounds__(KN_THREADS) void cm_sum_kernel(const float* __restrict__ X, int F, int ld, const int32_t* __restrict__ perm,
                                                            const int32_t* __restrict__ row_off, int k, double* __restrict__ psum) {
    __shared__ double s_v[KN_THREADS / WAVE][WAVE];
    const int c = blockIdx.x, lane = threadIdx.x & (WAVE - 1), g = threadIdx.x >> 6, col = blockIdx.y * WAVE + lane;
    const int p0 = row_off[c], cnt = row_off[c + 1] - p0, chunk = (cnt + gridDim.z - 1) / gridDim.z;
    const int j0 = min(cnt, (int)blockIdx.z * chunk), j1 = min(cnt, j0 + chunk);
    double v = 0.0;
    if (col < F)
        for (int j = j0 + g; j < j1; j += KN_THREADS / WAVE) v += (double)X[(size_t)perm[p0 + j] * ld + col];
    s_v[g][lane] = v;
    __syncthreads();
    if (g == 0 && col < F) psum[((size_t)blockIdx.z * k + c) * F + col] = ((s_v[0][lane] + s_v[1][lane]) + s_v[2][lane]) + s_v[3][lane];
}

// a thread per (cluster, column): the R parts in order, over the count (NaN for an empty cluster)
__global__ __launch_bounds__(KN_THREADS) void cm_center_kernel(const double* __restrict__ psum, const int32_t* __restrict__ row_off, int k, int F, int R,
                                                               double* __restrict__ centers) {
    const int e = blockIdx.x * KN_THREADS + threadIdx.x;
    if (e >= k * F) return;
    const int c = e / F;
    double v = 0.0;
    for (int z = 0; z < R; ++z) v += psum[(size_t)z * k * F + e];
    centers[e] = v / (double)(row_off[c + 1] - row_off[c]);
}

// grid (k, R), dynamic LDS F doubles: pd [R][k][2] = sum of the squared distances | sum of the distances of part z of cluster c's rows
// to its centre, differences and sums in fp64; a wave per row, rows in turn, a fixed xor tree over the lanes, waves added in wave order
__global__ __launch_bounds__(KN_THREADS) void cm_dist_kernel(const float* __restrict__ X, int F, int ld, const int32_t* __restrict__ perm,
                                                             const int32_t* __restrict__ row_off, int k, const double* __restrict__ centers,
                                                             double* __restrict__ pd) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cm_smem[];
    double* s_cen = reinterpret_cast<double*>(cm_smem);
    __shared__ double s_w[KN_THREADS / WAVE][2];
    const int c = blockIdx.x, lane = threadIdx.x & (WAVE - 1), g = threadIdx.x >> 6;
    const int p0 = row_off[c], cnt = row_off[c + 1] - p0, chunk = (cnt + gridDim.y - 1) / gridDim.y;
    const int j0 = min(cnt, (int)blockIdx.y * chunk), j1 = min(cnt, j0 + chunk);
    for (int f = threadIdx.x; f < F; f += KN_THREADS) s_cen[f] = centers[(size_t)c * F + f];
    __syncthreads();
    double wss = 0.0, sc = 0.0;
    for (int j = j0 + g; j < j1; j += KN_THREADS / WAVE) {
        const float* __restrict__ x = X + (size_t)perm[p0 + j] * ld;
        double d2 = 0.0;
        for (int f = lane; f < F; f += WAVE) {
            const double t = (double)x[f] - s_cen[f];
            d2 += t * t;
        }
        d2 = wave_sum(d2);
        wss += d2;
        sc += sqrt(d2);
    }
    if (lane == 0) { s_w[g][0] = wss; s_w[g][1] = sc; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int q = threadIdx.x;
        pd[((size_t)blockIdx.y * k + c) * 2 + q] = ((s_w[0][q] + s_w[1][q]) + s_w[2][q]) + s_w[3][q];
    }
}

// a thread per cluster: the R parts in order
__global__ __launch_bounds__(KN_THREADS) void cm_finish_kernel(const double* __restrict__ pd, const int32_t* __restrict__ row_off, int k, int R,
                                                               double* __restrict__ scatter, double* __restrict__ wss) {
    const int c = blockIdx.x * KN_THREADS + threadIdx.x;
    if (c >= k) return;
    double w = 0.0, s = 0.0;
    for (int z = 0; z < R; ++z) {
        w += pd[((size_t)z * k + c) * 2];
        s += pd[((size_t)z * k + c) * 2 + 1];
    }
    const int cnt = row_off[c + 1] - row_off[c];
    wss[c] = w;
    scatter[c] = cnt ? s / (double)cnt : __longlong_as_double(0x7FF8000000000000ll);
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
// the workspace parts (eagcn_hip.h), every one rounded up to 256 bytes
struct SortPlan { int W; int64_t chunk; size_t o_hist, o_offs, o_row, o_tile, o_perm, end; };
static inline SortPlan sort_plan(int64_t n, int k) {
    SortPlan p;
    int64_t W = (n + SIL_SORT_ROWS - 1) / SIL_SORT_ROWS;
    if (W > SIL_SORT_WAVES) W = SIL_SORT_WAVES;
    p.chunk = ((n + W - 1) / W + WAVE - 1) / WAVE * WAVE;
    p.W = (int)((n + p.chunk - 1) / p.chunk);
    p.o_hist = 0;
    p.o_offs = p.o_hist + align256((size_t)4 * p.W * (k + 1));
    p.o_row = p.o_offs + align256((size_t)4 * p.W * k);
    p.o_tile = p.o_row + align256((size_t)4 * (k + 1));
    p.o_perm = p.o_tile + align256((size_t)4 * (k + 1));
    p.end = p.o_perm + align256((size_t)4 * n);
    return p;
}
struct SilPlan { SortPlan sort; KnSlabs sl; size_t o_tiles, o_csum, o_part, bytes; };
static inline SilPlan sil_plan(int64_t n, int k, int slabs) {
    SilPlan p;
    p.sort = sort_plan(n, k);
    const int64_t qt = (n + KN_TILE - 1) / KN_TILE;
    p.sl = kn_slabs(qt + k, qt, slabs);                     // the tile bound: every cluster may end in a partial tile
    p.o_tiles = p.sort.end;
    p.o_csum = p.o_tiles + align256((size_t)16 * p.sl.tiles);
    p.o_part = p.o_csum + align256((size_t)8 * k);
    p.bytes = p.o_part + align256((size_t)8 * p.sl.S * (size_t)n * k);
    return p;
}
struct CmPlan { SortPlan sort; int R; size_t o_psum, o_pd, bytes; };
static inline CmPlan cm_plan(int64_t n, int F, int k) {
    CmPlan p;
    p.sort = sort_plan(n, k);
    int64_t R = (n + CM_SPLIT_ROWS - 1) / CM_SPLIT_ROWS;
    p.R = (int)(R > CM_MAX_SPLITS ? CM_MAX_SPLITS : R);
    p.o_psum = p.sort.end;
    p.o_pd = p.o_psum + align256((size_t)8 * p.R * k * F);
    p.bytes = p.o_pd + align256((size_t)16 * p.R * k);
    return p;
}
static inline bool sil_envelope(int64_t n, int F, int k) {
    return n >= 1 && n < (int64_t(1) << 31) && F >= 1 && F <= KN_MAX_F && k >= 2 && k <= SIL_MAX_K;
}
static int sil_check_rows(const char* fn, const float* X, int64_t n, int F, int ld, const int32_t* labels, int k) {
    EAGCN_CHECK_ARG(F >= 1 && F <= KN_MAX_F, "%s: F = %d is not in 1 .. %d", fn, F, KN_MAX_F);
    EAGCN_CHECK_ARG(X, "%s: X is null", fn);
    EAGCN_CHECK_ARG(n >= 1 && n < (int64_t(1) << 31), "%s: %lld rows of X are not in 1 .. 2^31 - 1", fn, (long long)n);
    EAGCN_CHECK_ARG(ld >= F, "%s: row stride %d of X is smaller than F = %d", fn, ld, F);
    EAGCN_CHECK_ARG((reinterpret_cast<uintptr_t>(X) & 3) == 0, "%s: X must be 4-byte aligned", fn);
    EAGCN_CHECK_ARG(labels, "%s: labels is null", fn);
    EAGCN_CHECK_ARG(k >= 2 && k <= SIL_MAX_K, "%s: k = %d is not in 2 .. %d", fn, k, SIL_MAX_K);
    return EAGCN_OK;
}
static int sil_check_ws(const char* fn, const void* ws, size_t ws_bytes, size_t need) {
    EAGCN_CHECK_ARG(ws, "%s: workspace is null", fn);
    EAGCN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
    EAGCN_CHECK_ARG(ws_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", fn, ws_bytes, need);
    return EAGCN_OK;
}
// the counting sort of the labels into the workspace parts of `p`; counts [k] and, if not null, stats[1 .. 3]
static int sort_rows(const SortPlan& p, char* ws, const int32_t* labels, int64_t n, int k, int64_t* counts, double* stats, hipStream_t s) {
    int32_t* hist = reinterpret_cast<int32_t*>(ws + p.o_hist);
    int32_t* offs = reinterpret_cast<int32_t*>(ws + p.o_offs);
    const int blocks = (p.W + KN_THREADS / WAVE - 1) / (KN_THREADS / WAVE);
    sil_hist_kernel<<<blocks, KN_THREADS, 0, s>>>(labels, n, k, p.W, p.chunk, hist);
    EAGCN_LAUNCH_CHECK();
    sil_scan_kernel<<<1, KN_THREADS, 0, s>>>(hist, p.W, k, offs, reinterpret_cast<int32_t*>(ws + p.o_row), reinterpret_cast<int32_t*>(ws + p.o_tile),
                                             counts, stats);
    EAGCN_LAUNCH_CHECK();
    sil_scatter_kernel<<<blocks, KN_THREADS, 0, s>>>(labels, n, k, p.W, p.chunk, offs, reinterpret_cast<int32_t*>(ws + p.o_perm));
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

}  // namespace eagcn

using namespace eagcn;

extern "C" size_t eagcn_silhouette_workspace_bytes(int64_t n, int F, int k, int slabs) {
    if (!sil_envelope(n, F, k) || slabs < 0) return 0;
    return sil_plan(n, k, slabs).bytes;
}

extern "C" int eagcn_silhouette(const float* X, int64_t n, int F, int ld, const int32_t* labels, int k, int slabs, double* samples,
                                double* cluster_mean, int64_t* counts, double* stats, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const char* fn = "eagcn_silhouette";
    if (int rc = sil_check_rows(fn, X, n, F, ld, labels, k)) return rc;
    EAGCN_CHECK_ARG(slabs >= 0, "%s: slabs = %d is negative", fn, slabs);
    EAGCN_CHECK_ARG(samples, "%s: samples is null", fn);
    EAGCN_CHECK_ARG(cluster_mean, "%s: cluster_mean is null", fn);
    EAGCN_CHECK_ARG(counts, "%s: counts is null", fn);
    EAGCN_CHECK_ARG(stats, "%s: stats is null", fn);
    const SilPlan p = sil_plan(n, k, slabs);
    if (int rc = sil_check_ws(fn, ws, ws_bytes, p.bytes)) return rc;
    char* w = static_cast<char*>(ws);
    const int32_t* row_off = reinterpret_cast<const int32_t*>(w + p.sort.o_row);
    const int32_t* tile_off = reinterpret_cast<const int32_t*>(w + p.sort.o_tile);
    const int32_t* perm = reinterpret_cast<const int32_t*>(w + p.sort.o_perm);
    int4* tiles = reinterpret_cast<int4*>(w + p.o_tiles);
    double* csum = reinterpret_cast<double*>(w + p.o_csum);
    double* part = reinterpret_cast<double*>(w + p.o_part);
    if (int rc = sort_rows(p.sort, w, labels, n, k, counts, stats, s)) return rc;
    const int tgrid = (p.sl.tiles + KN_THREADS - 1) / KN_THREADS;
    sil_tiles_kernel<<<tgrid < 65536 ? tgrid : 65536, KN_THREADS, 0, s>>>(row_off, tile_off, k, p.sl.tiles, tiles);
    EAGCN_LAUNCH_CHECK();
    const unsigned qt = (unsigned)((n + KN_TILE - 1) / KN_TILE);
    sil_sum_kernel<<<dim3(qt, p.sl.S), KN_THREADS, 0, s>>>(X, n, F, ld, perm, tiles, k, p.sl.per, p.sl.tiles, part);
    EAGCN_LAUNCH_CHECK();
    sil_finish_kernel<<<(unsigned)((n + KN_THREADS - 1) / KN_THREADS), KN_THREADS, 0, s>>>(part, labels, n, k, p.sl.per, row_off, tile_off, samples);
    EAGCN_LAUNCH_CHECK();
    sil_mean_kernel<<<k, KN_THREADS, 0, s>>>(samples, perm, row_off, csum, cluster_mean);
    EAGCN_LAUNCH_CHECK();
    sil_total_kernel<<<1, WAVE, 0, s>>>(csum, k, stats);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

extern "C" size_t eagcn_cluster_moments_workspace_bytes(int64_t n, int F, int k) {
    if (!sil_envelope(n, F, k)) return 0;
    return cm_plan(n, F, k).bytes;
}

extern "C" int eagcn_cluster_moments(const float* X, int64_t n, int F, int ld, const int32_t* labels, int k, double* centers, double* scatter,
                                     double* wss, int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const char* fn = "eagcn_cluster_moments";
    if (int rc = sil_check_rows(fn, X, n, F, ld, labels, k)) return rc;
    EAGCN_CHECK_ARG(centers, "%s: centers is null", fn);
    EAGCN_CHECK_ARG(scatter, "%s: scatter is null", fn);
    EAGCN_CHECK_ARG(wss, "%s: wss is null", fn);
    EAGCN_CHECK_ARG(counts, "%s: counts is null", fn);
    const CmPlan p = cm_plan(n, F, k);
    if (int rc = sil_check_ws(fn, ws, ws_bytes, p.bytes)) return rc;
    char* w = static_cast<char*>(ws);
    const int32_t* row_off = reinterpret_cast<const int32_t*>(w + p.sort.o_row);
    const int32_t* perm = reinterpret_cast<const int32_t*>(w + p.sort.o_perm);
    double* psum = reinterpret_cast<double*>(w + p.o_psum);
    double* pd = reinterpret_cast<double*>(w + p.o_pd);
    if (int rc = sort_rows(p.sort, w, labels, n, k, counts, nullptr, s)) return rc;
    cm_sum_kernel<<<dim3(k, (F + WAVE - 1) / WAVE, p.R), KN_THREADS, 0, s>>>(X, F, ld, perm, row_off, k, psum);
    EAGCN_LAUNCH_CHECK();
    cm_center_kernel<<<(k * F + KN_THREADS - 1) / KN_THREADS, KN_THREADS, 0, s>>>(psum, row_off, k, F, p.R, centers);
    EAGCN_LAUNCH_CHECK();
    cm_dist_kernel<<<dim3(k, p.R), KN_THREADS, sizeof(double) * F, s>>>(X, F, ld, perm, row_off, k, centers, pd);
    EAGCN_LAUNCH_CHECK();
    cm_finish_kernel<<<(k + KN_THREADS - 1) / KN_THREADS, KN_THREADS, 0, s>>>(pd, row_off, k, p.R, scatter, wss);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}
