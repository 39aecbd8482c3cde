// The 64 x 64 distance tile of em_sqdist_kernel (csrc/embed.hip) as a register-resident front end, and the rule that cuts the data tiles
// into slabs: shared by the nearest-neighbour kernels (csrc/knn.hip) and the silhouette kernels (csrc/silhouette.hip).  Every distance is
// one fmaf chain in column order -- the bits of eagcn_sqdist -- whichever consumer works on the registers.
#pragma once
#include "common.h"

namespace eagcn {

constexpr int KN_TILE = 64;          // query rows and data rows of a tile
constexpr int KN_KC = 32;            // feature columns staged per step
constexpr int KN_THREADS = 256;
constexpr int KN_PADT = KN_TILE + 4; // LDS row of a transposed tile: 16-byte aligned rows
constexpr int KN_MAX_F = 1024;
constexpr int KN_TARGET_WGS = 4096;  // slabs = 0: as many slabs as bring the launch to this many workgroups ...
constexpr int KN_AUTO_SLABS = 64;    // ... and at most this many
constexpr int KN_MAX_SLABS = 4096;
constexpr size_t KN_STAGE_BYTES = 2 * sizeof(float) * KN_KC * KN_PADT;
static_assert(KN_TILE * KN_TILE == 16 * KN_THREADS, "a thread holds a 4 x 4 block of a tile");
static_assert(KN_STAGE_BYTES % 16 == 0, "the parts behind the staging tiles stay 16-byte aligned");

// acc[u][v] = d(query tile row 4 ty + u, data tile row 4 tx + v).  rowA(r, row) / rowB(r, row) set the row of Q / X behind tile row r and
// say whether there is one: a tile row without reads as zeros.  Ends behind a barrier.
template <class RowA, class RowB>
__device__ __forceinline__ void kn_tile_rows(const float* __restrict__ Q, int ldq, const float* __restrict__ X, int ld, int F, RowA rowA, RowB rowB,
                                             float (*sA)[KN_PADT], float (*sB)[KN_PADT], float (&acc)[4][4]) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lc = tid & 31, lr = tid >> 5;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0f;
    for (int c0 = 0; c0 < F; c0 += KN_KC) {
        const int c = c0 + lc;
#pragma unroll
        for (int u = 0; u < KN_TILE / 8; ++u) {
            const int r = lr + 8 * u;
            int64_t ra, rb;
            const bool oka = rowA(r, ra), okb = rowB(r, rb);
            sA[lc][r] = (oka && c < F) ? Q[(size_t)ra * ldq + c] : 0.0f;
            sB[lc][r] = (okb && c < F) ? X[(size_t)rb * ld + c] : 0.0f;
        }
        __syncthreads();
        auto step = [&](int k) {
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
        };
        if (c0 + KN_KC <= F) {
#pragma unroll 8
            for (int k = 0; k < KN_KC; ++k) step(k);
        } else {                                            // (the columns beyond F would add exact zeros: the same bits, less work)
            for (int k = 0; k < F - c0; ++k) step(k);
        }
        __syncthreads();
    }
}

// acc[u][v] = d(query row i0 + 4 ty + u, data row j0 + 4 tx + v); rows beyond m / n read as zeros.  Ends behind a barrier.
// PERM: the data rows are perm[j0 + 4 tx + v] instead, j0 and n positions in `perm` (n the end of the tile's rows there), so that a tile
// may hold any 64 rows or fewer of X without a copy of them; the entries of perm are rows of X.
template <bool PERM = false>
__device__ __forceinline__ void kn_tile(const float* __restrict__ Q, int64_t m, int ldq, const float* __restrict__ X, int64_t n, int ld, int F,
                                        int64_t i0, int64_t j0, float (*sA)[KN_PADT], float (*sB)[KN_PADT], float (&acc)[4][4],
                                        const int32_t* __restrict__ perm = nullptr) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lc = tid & 31, lr = tid >> 5;
    int prow[PERM ? KN_TILE / 8 : 1];
    if constexpr (PERM) {
#pragma unroll
        for (int u = 0; u < KN_TILE / 8; ++u) prow[u] = j0 + lr + 8 * u < n ? perm[j0 + lr + 8 * u] : 0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0f;
    for (int c0 = 0; c0 < F; c0 += KN_KC) {
        const int c = c0 + lc;
#pragma unroll
        for (int u = 0; u < KN_TILE / 8; ++u) {
            const int r = lr + 8 * u;
            const int64_t ra = i0 + r, rb = j0 + r;
            sA[lc][r] = (ra < m && c < F) ? Q[(size_t)ra * ldq + c] : 0.0f;
            if constexpr (PERM) sB[lc][r] = (rb < n && c < F) ? X[(size_t)prow[u] * ld + c] : 0.0f;
            else sB[lc][r] = (rb < n && c < F) ? X[(size_t)rb * ld + c] : 0.0f;
        }
        __syncthreads();
        auto step = [&](int k) {
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
        };
        if (c0 + KN_KC <= F) {
#pragma unroll 8
            for (int k = 0; k < KN_KC; ++k) step(k);
        } else {                                            // (the columns beyond F would add exact zeros: the same bits, less work)
            for (int k = 0; k < F - c0; ++k) step(k);
        }
        __syncthreads();
    }
}

// The split of `dt` data tiles among S workgroups per tile of 64 query rows (include/eagcn_hip.h): whole tiles, `per` tiles a slab, no
// empty slab.  qt = the number of query tiles.
struct KnSlabs { int tiles, S, per; };
static inline KnSlabs kn_slabs(int64_t dt, int64_t qt, int slabs) {
    int64_t S = slabs;
    if (S <= 0) {
        S = (KN_TARGET_WGS + qt - 1) / qt;
        if (S > KN_AUTO_SLABS) S = KN_AUTO_SLABS;
    }
    if (S > KN_MAX_SLABS) S = KN_MAX_SLABS;
    if (S > dt) S = dt;
    if (S < 1) S = 1;
    KnSlabs p;
    p.tiles = (int)dt;
    p.per = (int)((dt + S - 1) / S);
    p.S = (int)((dt + p.per - 1) / p.per);
    return p;
}

}  // namespace eagcn
