// Exact nearest-neighbour search over device rows and the rank of given candidates among a row's neighbours (the similarity search
// the reference's mol_to_vec_plot.py does by eye, and the input of a trustworthiness score), on the device.
// Semantics in include/eagcn_hip.h; no floating-point atomics, every distance one fmaf chain in column order -- the bits of
// eagcn_sqdist -- and every candidate ordered by the 64-bit key (distance bits << 32 | row index): results are unique, hence
// bit-identical from run to run and for every split of the data rows.
//
//   kn_tile            (csrc/dist_tile.h) the 64 x 64 distance tile of em_sqdist_kernel (csrc/embed.hip): KN_KC columns of 64 query and 64
//                      data rows transposed into LDS, a 4 x 4 block per thread.  It is never stored: two consumers work on the registers.
//   kn_search_kernel   grid (query tiles, slabs).  A query row's k best keys so far are a sorted list in LDS.  Every thread compares
//                      its 16 distances with its four rows' k-th keys (a reject costs that one compare), passes the few that beat it
//                      through LDS with a bit in the row's 64-bit mask, and wave 0 -- one lane per query row -- inserts them while
//                      the other waves already stage the next tile.  The lists go to the workspace, one per slab.
//   kn_merge_kernel    a thread per (query, slab, position): the position of its key among all of the query's slab lists by
//                      binary search (keys are distinct); the first k are stored.
//   kn_thr_kernel /    the keys of the candidates (one thread per candidate, the same fmaf chain), then per tile and query row
//   kn_count_kernel /  integer counts of the data rows whose key is below each of them: LDS integer adds, per-slab partial counts,
//   kn_rank_kernel     summed per candidate at the end (integer sums do not depend on their order).
#include "dist_tile.h"

namespace eagcn {

constexpr int KN_MAX_K = EAGCN_KNN_MAX_K;
constexpr uint64_t KN_SENTINEL = 0x7FC000007FFFFFFFull;    // (NaN, 2^31 - 1): behind every candidate, n < 2^31
constexpr uint64_t KN_INVALID = ~0ull;                     // threshold of a candidate that is the row itself or no row at all

// the order: distances ascending (their bits, as unsigned: they are sums of squares and never negative), a NaN behind every number,
// equal distances by the smaller row index
__device__ __forceinline__ uint64_t kn_key(float d, int j) {
    const uint32_t b = d != d ? 0x7FC00000u : __float_as_uint(d);
    return ((uint64_t)b << 32) | (uint32_t)j;
}

// ---- search ------------------------------------------------------------------------------------------------------------------------
// dynamic LDS: the two staging tiles | sD [64][65] | the rows' k-th keys [64] | masks [64][2] | lists [64][k | 1]
static inline size_t kn_search_lds(int k) {
    return KN_STAGE_BYTES + sizeof(float) * KN_TILE * (KN_TILE + 1) + 8 * KN_TILE + 8 * KN_TILE + 8 * (size_t)KN_TILE * (k | 1);
}

// grid (ceil(m / 64), S): the k first candidates of 64 query rows among the data rows of the tiles [y per, (y + 1) per) -> part [S][m][k]
__global__ __launch_bounds__(KN_THREADS) void kn_search_kernel(const float* __restrict__ X, int64_t n, int F, int ld, const float* __restrict__ Q,
                                                               int64_t m, int ldq, int k, int exclude_self, int per, int tiles,
                                                               uint64_t* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char kn_smem[];
    float (*sA)[KN_PADT] = reinterpret_cast<float (*)[KN_PADT]>(kn_smem);
    float (*sB)[KN_PADT] = sA + KN_KC;
    float (*sD)[KN_TILE + 1] = reinterpret_cast<float (*)[KN_TILE + 1]>(kn_smem + KN_STAGE_BYTES);
    uint64_t* s_tau = reinterpret_cast<uint64_t*>(kn_smem + KN_STAGE_BYTES + sizeof(float) * KN_TILE * (KN_TILE + 1));
    uint32_t* s_mask = reinterpret_cast<uint32_t*>(s_tau + KN_TILE);
    uint64_t* s_list = s_tau + 2 * KN_TILE;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, kp = k | 1;      // (an odd row length: the 64 lists start in different banks)
    const int64_t i0 = (int64_t)blockIdx.x * KN_TILE;
    for (int e = tid; e < KN_TILE * kp; e += KN_THREADS) s_list[e] = KN_SENTINEL;
    if (tid < KN_TILE) { s_tau[tid] = KN_SENTINEL; s_mask[2 * tid] = 0u; s_mask[2 * tid + 1] = 0u; }
    __syncthreads();
    const int tbeg = blockIdx.y * per, tend = min(tiles, tbeg + per);
    for (int t = tbeg; t < tend; ++t) {
        const int64_t j0 = (int64_t)t * KN_TILE;
        float acc[4][4];
        kn_tile(Q, m, ldq, X, n, ld, F, i0, j0, sA, sB, acc);
        // (wave 0 has finished the tile before: it passed the barriers of kn_tile behind its insertions)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = ty * 4 + u;
            const int64_t i = i0 + row;
            if (i >= m) continue;
            const uint64_t tau = s_tau[row];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int col = tx * 4 + v;
                const int64_t j = j0 + col;
                if (j >= n || (exclude_self && j == i)) continue;
                if (kn_key(acc[u][v], (int)j) < tau) {
                    sD[row][col] = acc[u][v];
                    atomicOr(&s_mask[2 * row + (col >> 5)], 1u << (col & 31));
                }
            }
        }
        __syncthreads();
        if (tid < KN_TILE) {                                // one lane per query row: the survivors in column order into the sorted list
            uint64_t mm = ((uint64_t)s_mask[2 * tid + 1] << 32) | s_mask[2 * tid];
            if (mm) {
                uint64_t* L = s_list + tid * kp;
                uint64_t tau = s_tau[tid];
                while (mm) {
                    const int col = __ffsll((unsigned long long)mm) - 1;
                    mm &= mm - 1;
                    const uint64_t key = kn_key(sD[tid][col], (int)(j0 + col));
                    if (key < tau) {
                        int p = k - 1;
                        while (p > 0) {
                            const uint64_t prev = L[p - 1];
                            if (prev < key) break;
                            L[p] = prev;
                            --p;
                        }
                        L[p] = key;
                        tau = L[k - 1];
                    }
                }
                s_tau[tid] = tau;
                s_mask[2 * tid] = 0u;
                s_mask[2 * tid + 1] = 0u;
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < KN_TILE * k; e += KN_THREADS) {
        const int row = e / k, p = e - row * k;
        if (i0 + row < m) part[((size_t)blockIdx.y * m + i0 + row) * k + p] = s_list[row * kp + p];
    }
}

// a thread per key of part [S][m][k]: its position among the S lists of its query; the first k -> idx / dist [m][k]
__global__ __launch_bounds__(KN_THREADS) void kn_merge_kernel(const uint64_t* __restrict__ part, int64_t m, int k, int S, int32_t* __restrict__ idx,
                                                              float* __restrict__ dist) {
    const size_t total = (size_t)m * S * k;
    for (size_t t = (size_t)blockIdx.x * KN_THREADS + threadIdx.x; t < total; t += (size_t)gridDim.x * KN_THREADS) {
        const size_t q = t / ((size_t)S * k);
        const int rem = (int)(t - q * S * k), s = rem / k, p = rem - s * k;
        const uint64_t key = part[((size_t)s * m + q) * k + p];
        if (key == KN_SENTINEL) continue;
        int pos = p;
        for (int o = 0; o < S && pos < k; ++o) {
            if (o == s) continue;
            const uint64_t* __restrict__ L = part + ((size_t)o * m + q) * k;
            int lo = 0, hi = k;                             // the number of keys of list o below this one
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (L[mid] < key) lo = mid + 1; else hi = mid;
            }
            pos += lo;
        }
        if (pos < k) {
            idx[q * k + pos] = (int32_t)(uint32_t)key;
            dist[q * k + pos] = __uint_as_float((uint32_t)(key >> 32));
        }
    }
}

// ---- ranks ---------------------------------------------------------------------------------------------------------------------------
// a thread per candidate: thr[i][c] = the key of (d(i, j), j), j = cand[i][c]; KN_INVALID where j is i or not a row
__global__ __launch_bounds__(KN_THREADS) void kn_thr_kernel(const float* __restrict__ X, int64_t n, int F, int ld, const int32_t* __restrict__ cand,
                                                            int k, uint64_t* __restrict__ thr) {
    const size_t total = (size_t)n * k;
    for (size_t t = (size_t)blockIdx.x * KN_THREADS + threadIdx.x; t < total; t += (size_t)gridDim.x * KN_THREADS) {
        const int64_t i = (int64_t)(t / k), j = cand[t];
        uint64_t key = KN_INVALID;
        if (j >= 0 && j < n && j != i) {
            const float* __restrict__ a = X + (size_t)i * ld;
            const float* __restrict__ b = X + (size_t)j * ld;
            float acc = 0.0f;
            for (int c = 0; c < F; ++c) {
                const float d = a[c] - b[c];
                acc = fmaf(d, d, acc);
            }
            key = kn_key(acc, (int)j);
        }
        thr[t] = key;
    }
}

// dynamic LDS: the two staging tiles | thresholds [64][k | 1] | counts [64][k | 1]
static inline size_t kn_count_lds(int k) { return KN_STAGE_BYTES + 12 * (size_t)KN_TILE * (k | 1); }

// grid (ceil(n / 64), S): cnt [S][n][k] = the rows l != i of the slab's tiles with key(d(i, l), l) < thr[i][c]
__global__ __launch_bounds__(KN_THREADS) void kn_count_kernel(const float* __restrict__ X, int64_t n, int F, int ld, int k, int per, int tiles,
                                                              const uint64_t* __restrict__ thr, int32_t* __restrict__ cnt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char kn_smem[];
    float (*sA)[KN_PADT] = reinterpret_cast<float (*)[KN_PADT]>(kn_smem);
    float (*sB)[KN_PADT] = sA + KN_KC;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, kp = k | 1;
    uint64_t* s_thr = reinterpret_cast<uint64_t*>(kn_smem + KN_STAGE_BYTES);
    int* s_cnt = reinterpret_cast<int*>(s_thr + KN_TILE * kp);
    const int64_t i0 = (int64_t)blockIdx.x * KN_TILE;
    for (int e = tid; e < KN_TILE * k; e += KN_THREADS) {
        const int row = e / k, c = e - row * k;
        s_thr[row * kp + c] = i0 + row < n ? thr[(size_t)(i0 + row) * k + c] : 0ull;
        s_cnt[row * kp + c] = 0;
    }
    __syncthreads();
    const int tbeg = blockIdx.y * per, tend = min(tiles, tbeg + per);
    for (int t = tbeg; t < tend; ++t) {
        const int64_t j0 = (int64_t)t * KN_TILE;
        float acc[4][4];
        kn_tile(X, n, ld, X, n, ld, F, i0, j0, sA, sB, acc);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = ty * 4 + u;
            const int64_t i = i0 + row;
            if (i >= n) continue;
            uint64_t key[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t l = j0 + tx * 4 + v;
                key[v] = (l < n && l != i) ? kn_key(acc[u][v], (int)l) : KN_INVALID;     // (nothing is above KN_INVALID)
            }
            for (int c = 0; c < k; ++c) {
                const uint64_t th = s_thr[row * kp + c];
                const int below = (int)(key[0] < th) + (int)(key[1] < th) + (int)(key[2] < th) + (int)(key[3] < th);
                if (below) atomicAdd(&s_cnt[row * kp + c], below);
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < KN_TILE * k; e += KN_THREADS) {
        const int row = e / k, c = e - row * k;
        if (i0 + row < n) cnt[((size_t)blockIdx.y * n + i0 + row) * k + c] = s_cnt[row * kp + c];
    }
}

// a thread per candidate: rank = 1 + the slabs' counts, -1 for a candidate without a threshold
__global__ __launch_bounds__(KN_THREADS) void kn_rank_kernel(const uint64_t* __restrict__ thr, const int32_t* __restrict__ cnt, int64_t n, int k, int S,
                                                             int32_t* __restrict__ rank) {
    const size_t total = (size_t)n * k;
    for (size_t t = (size_t)blockIdx.x * KN_THREADS + threadIdx.x; t < total; t += (size_t)gridDim.x * KN_THREADS) {
        int r = 1;
        for (int s = 0; s < S; ++s) r += cnt[(size_t)s * total + t];
        rank[t] = thr[t] == KN_INVALID ? -1 : r;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
struct KnPlan { int tiles, S, per; size_t part_bytes, bytes; };
// the split of the data rows (eagcn_hip.h): whole tiles of 64 rows, `per` tiles a slab, no empty slab
static inline KnPlan kn_plan(int64_t n, int64_t m, int k, int slabs) {
    KnPlan p;
    const KnSlabs sl = kn_slabs((n + KN_TILE - 1) / KN_TILE, (m + KN_TILE - 1) / KN_TILE, slabs);
    p.tiles = sl.tiles;
    p.per = sl.per;
    p.S = sl.S;
    p.part_bytes = align256((size_t)8 * p.S * (size_t)m * k);
    p.bytes = p.part_bytes + align256((size_t)8 * (size_t)m * k);
    return p;
}
static inline bool kn_envelope(int64_t n, int64_t m, int F, int k) {
    return n >= 1 && n < (int64_t(1) << 31) && m >= 1 && m < (int64_t(1) << 31) && F >= 1 && F <= KN_MAX_F && k >= 1 && k <= KN_MAX_K;
}
static int kn_check_rows(const char* fn, const char* what, const float* X, int64_t n, int F, int ld) {
    EAGCN_CHECK_ARG(X, "%s: %s is null", fn, what);
    EAGCN_CHECK_ARG(n >= 1 && n < (int64_t(1) << 31), "%s: %lld rows of %s are not in 1 .. 2^31 - 1", fn, (long long)n, what);
    EAGCN_CHECK_ARG(ld >= F, "%s: row stride %d of %s is smaller than F = %d", fn, ld, what, F);
    EAGCN_CHECK_ARG((reinterpret_cast<uintptr_t>(X) & 3) == 0, "%s: %s must be 4-byte aligned", fn, what);
    return EAGCN_OK;
}
static int kn_check_common(const char* fn, int F, int k, int slabs, const void* ws, size_t ws_bytes, size_t need) {
    EAGCN_CHECK_ARG(F >= 1 && F <= KN_MAX_F, "%s: F = %d is not in 1 .. %d", fn, F, KN_MAX_F);
    EAGCN_CHECK_ARG(k >= 1 && k <= KN_MAX_K, "%s: k = %d is not in 1 .. %d", fn, k, KN_MAX_K);
    EAGCN_CHECK_ARG(slabs >= 0, "%s: slabs = %d is negative", fn, slabs);
    EAGCN_CHECK_ARG(ws, "%s: workspace is null", fn);
    EAGCN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: workspace must be 256-byte aligned", fn);
    EAGCN_CHECK_ARG(ws_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", fn, ws_bytes, need);
    return EAGCN_OK;
}
static inline int kn_flat_grid(size_t items) {
    const size_t want = (items + KN_THREADS - 1) / KN_THREADS;
    return (int)(want < 65536 ? (want ? want : 1) : 65536);
}

}  // namespace eagcn

using namespace eagcn;

extern "C" size_t eagcn_knn_workspace_bytes(int64_t n, int64_t m, int F, int k, int slabs) {
    if (!kn_envelope(n, m, F, k) || slabs < 0) return 0;
    return kn_plan(n, m, k, slabs).bytes;
}

extern "C" int eagcn_knn(const float* X, int64_t n, int F, int ldx, const float* Q, int64_t m, int ldq, int k, int exclude_self, int slabs,
                         int32_t* idx, float* dist, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const char* fn = "eagcn_knn";
    EAGCN_CHECK_ARG(F >= 1 && F <= KN_MAX_F, "%s: F = %d is not in 1 .. %d", fn, F, KN_MAX_F);
    if (int rc = kn_check_rows(fn, "X", X, n, F, ldx)) return rc;
    if (int rc = kn_check_rows(fn, "Q", Q, m, F, ldq)) return rc;
    EAGCN_CHECK_ARG(k >= 1 && k <= KN_MAX_K, "%s: k = %d is not in 1 .. %d", fn, k, KN_MAX_K);
    EAGCN_CHECK_ARG(exclude_self == 0 || exclude_self == 1, "%s: exclude_self = %d is not 0 or 1", fn, exclude_self);
    EAGCN_CHECK_ARG(!exclude_self || m == n, "%s: exclude_self needs m = n (m = %lld, n = %lld)", fn, (long long)m, (long long)n);
    EAGCN_CHECK_ARG(k <= n - exclude_self, "%s: k = %d is more than the %lld candidates of a query", fn, k, (long long)(n - exclude_self));
    EAGCN_CHECK_ARG(idx, "%s: idx is null", fn);
    EAGCN_CHECK_ARG(dist, "%s: dist is null", fn);
    const KnPlan p = kn_plan(n, m, k, slabs < 0 ? 0 : slabs);
    if (int rc = kn_check_common(fn, F, k, slabs, ws, ws_bytes, p.bytes)) return rc;
    uint64_t* part = static_cast<uint64_t*>(ws);
    const size_t lds = kn_search_lds(k);
    if (lds > 64 * 1024)                                    // (set per launch: the attribute belongs to the current device)
        EAGCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&kn_search_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kn_search_kernel<<<dim3((unsigned)((m + KN_TILE - 1) / KN_TILE), p.S), KN_THREADS, lds, s>>>(X, n, F, ldx, Q, m, ldq, k, exclude_self, p.per,
                                                                                                  p.tiles, part);
    EAGCN_LAUNCH_CHECK();
    kn_merge_kernel<<<kn_flat_grid((size_t)m * p.S * k), KN_THREADS, 0, s>>>(part, m, k, p.S, idx, dist);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

extern "C" int eagcn_knn_rank(const float* X, int64_t n, int F, int ld, const int32_t* cand, int k, int slabs, int32_t* rank, void* ws,
                              size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const char* fn = "eagcn_knn_rank";
    EAGCN_CHECK_ARG(F >= 1 && F <= KN_MAX_F, "%s: F = %d is not in 1 .. %d", fn, F, KN_MAX_F);
    if (int rc = kn_check_rows(fn, "X", X, n, F, ld)) return rc;
    EAGCN_CHECK_ARG(cand, "%s: cand is null", fn);
    EAGCN_CHECK_ARG(rank, "%s: rank is null", fn);
    EAGCN_CHECK_ARG(k >= 1 && k <= KN_MAX_K, "%s: k = %d is not in 1 .. %d", fn, k, KN_MAX_K);
    const KnPlan p = kn_plan(n, n, k, slabs < 0 ? 0 : slabs);
    if (int rc = kn_check_common(fn, F, k, slabs, ws, ws_bytes, p.bytes)) return rc;
    int32_t* cnt = static_cast<int32_t*>(ws);               // [S][n][k] int32 in the part of the search's lists
    uint64_t* thr = reinterpret_cast<uint64_t*>(static_cast<char*>(ws) + p.part_bytes);
    const int flat = kn_flat_grid((size_t)n * k);
    kn_thr_kernel<<<flat, KN_THREADS, 0, s>>>(X, n, F, ld, cand, k, thr);
    EAGCN_LAUNCH_CHECK();
    const size_t lds = kn_count_lds(k);
    if (lds > 64 * 1024)
        EAGCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&kn_count_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kn_count_kernel<<<dim3((unsigned)((n + KN_TILE - 1) / KN_TILE), p.S), KN_THREADS, lds, s>>>(X, n, F, ld, k, p.per, p.tiles, thr, cnt);
    EAGCN_LAUNCH_CHECK();
    kn_rank_kernel<<<flat, KN_THREADS, 0, s>>>(thr, cnt, n, k, p.S, rank);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}
