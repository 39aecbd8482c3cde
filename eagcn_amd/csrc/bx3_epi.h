// The BatchNorm-backward tail pass of the plane GEMM's NT units (bx3.h BxBnEpi; gemm_bx3.hip bx_compute runs it behind its stream).
#pragma once
#include "bx3.h"
#include "common.h"
#include "kernels.h"

namespace eagcn {

// the value of lane Q of every quad, in all four lanes of the quad (DPP quad_perm: no LDS crossbar)
template <int Q>
__device__ __forceinline__ uint32_t bx_quad_bcast(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, Q * 0x55, 0xF, 0xF, true);
}
// keep-scale of this lane's column out of the draw z of its 4-column group (common.h drop_scale4: field column & 3)
__device__ __forceinline__ float bx_keep(uint32_t zlo, uint32_t zhi, int piece, uint32_t t16, float inv_keep) {
    const uint32_t w = (piece & 2) ? zhi : zlo;
    return ((piece & 1) ? (w >> 16) : (w & 0xFFFFu)) >= t16 ? inv_keep : 0.0f;
}

// One wave's 64 x 64 block at (m0, n0) of an NT product with p.ep set, BEHIND the plain store of the block (m0, n0 multiples of 64; the
// caller has checked m0 < Mlim and n0 < p.N, both uniform over the wave; every lane of the wave takes part).  The block's accumulators
// (128 registers), the next unit's first fragments and this code's operands do not fit a wave's 256 registers side by side: the block
// is stored as ever, which frees the accumulators, and every lane reads ITS elements back (L2: the lines were written a moment ago) as
// it goes.  D layout of v_mfma_f32_32x32x16_bf16: tile (i, jj), register r holds row m0 + 32 i + (r & 3) + 8 (r >> 2) + 4 (lane >> 5),
// column n0 + 32 jj + (lane & 31): a lane has two columns x 32 rows.
//   * memory: BUFFER loads and stores over the block's rows inside the matrix (Y', the row mask and C each get a descriptor that ends
//     with the block's last row below Mlim; a lane whose column is outside asks beyond it): what lies outside arrives as zero and
//     is not written -- one code path for whole and partial blocks, no predicate and no 64-bit lane address per element;
//   * dX, Y' and the row mask arrive in batches of 16 (one tile);
//   * dropout: one 64-bit draw serves the four adjacent columns of a row (drop_scale4) = the four lanes of a quad; lane q of a quad
//     draws for the rows r & 3 == q of its tile (4 hashes per lane and tile instead of 16) and the quad passes them round;
//   * sums: fp64, in-lane over the lane's 32 rows, one exchange with lane ^ 32, lanes 0-31 write slab row m0 / 64.
__device__ __forceinline__ void bx_bn_epilogue(const int pidx, const int m0_, const int n0_, const int Mlim_, const int lane_) {
    // (uniform, but not provably: the unit list of a TN stream goes through a wave-wide minimum, and a descriptor in vector
    //  registers costs a loop over the lanes per memory instruction)
    const int m0 = __builtin_amdgcn_readfirstlane(m0_), n0 = __builtin_amdgcn_readfirstlane(n0_), Mlim = __builtin_amdgcn_readfirstlane(Mlim_);
    // (the problem is read HERE, per unit, from the kernel's argument segment -- problem `pidx` of a kernel whose arguments START with
    //  its BxProb's -- through a pointer the optimiser cannot see through: fetched at the kernel's entry its twenty words stayed live
    //  across the k-loop, scalar registers spilled to vector lanes, and cost the loop its last registers)
    static_assert(sizeof(BxProb) % 8 == 0 && alignof(BxProb) == 8, "consecutive BxProb kernel arguments are an array");
    typedef const __attribute__((address_space(4))) BxProb* BxProbArg;
    BxProbArg pa = (BxProbArg)__builtin_amdgcn_kernarg_segment_ptr() + __builtin_amdgcn_readfirstlane(pidx);
    asm volatile("" : "+s"(pa));
    // (the strides and the lane number pass through an empty asm: the per-lane offsets derived from them are formed HERE, per unit
    //  -- as invariants of the k-loop they were hoisted out of it, dozens of registers spilled in the prologue and re-loaded one by one)
    int ldy = pa->ep.ldy, ldc = pa->ldc, fp = pa->ep.fp, lane = lane_;
    asm volatile("" : "+s"(ldy), "+s"(ldc), "+s"(fp), "+v"(lane));
    const int half = lane >> 5, piece = lane & 3;
    const uint64_t seed = pa->ep.do_drop ? (pa->ep.seed_dev ? *pa->ep.seed_dev : pa->ep.seed) : 0ull;
    // (no dropout: threshold 0 keeps every element at scale 1 -- the same code, nothing drawn)
    const uint32_t t16 = pa->ep.do_drop ? pa->ep.thr >> 16 : 0u;
    const float keep = pa->ep.do_drop ? pa->ep.inv_keep : 1.0f;
    const int rows_in = min(64, Mlim - m0);
    const uint32_t OUTSIDE = 0x80000000u;              // beyond every num_records below (64 rows of a matrix)
    const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc((void*)(pa->ep.row_m + m0), 0, rows_in * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)(pa->ep.Y + (size_t)m0 * ldy), 0, rows_in * ldy * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc((void*)(pa->C + (size_t)m0 * ldc), 0, rows_in * ldc * 4, 0x00020000);
    auto rin = [&](int i, int r) __attribute__((always_inline)) { return i * 32 + (r & 3) + 8 * (r >> 2); };      // (+ 4 half: row of the block)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's stores of the block have left
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int col = n0 + jj * 32 + (lane & 31);
        const bool cok = col < pa->N;
        const int cl = cok ? col : 0;
        const float sc = pa->ep.bn[BN_SC * fp + cl], sh = pa->ep.bn[BN_SH * fp + cl], mu = pa->ep.bn[BN_MU * fp + cl], iv = pa->ep.bn[BN_INV * fp + cl];
        const uint32_t yoff = cok ? (uint32_t)(4 * half * ldy + col) * 4u : OUTSIDE, coff = cok ? (uint32_t)(4 * half * ldc + col) * 4u : OUTSIDE;
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int ih = 0; ih < 4; ++ih) {               // (batches of 8: rows 16 (ih & 1) .. + 15 of tile i -- sixteen took the k-loop's last registers)
            const int i = ih >> 1, r0 = 8 * (ih & 1);
            asm volatile("" ::: "memory");             // one batch at a time, behind the stores of the batch before
            float y[8], up[8], m[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int r = r0 + q;
                // (glc: past the vector cache -- the lines were written by this wave's stores)
                up[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rc, (int)(coff + (uint32_t)(rin(i, r) * ldc) * 4u), 0, 1));
                y[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ry, (int)(yoff + (uint32_t)(rin(i, r) * ldy) * 4u), 0, 0));
                m[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rm, (4 * half + rin(i, r)) * 4, 0, 0));
            }
            uint32_t zl[2] = {0u, 0u}, zh[2] = {0u, 0u};
            if (pa->ep.do_drop) {
#pragma unroll
                for (int g = 0; g < 2; ++g) {          // this lane's share of the quad's draws: rows (r & 3) == piece
                    const uint64_t z = rng_u64(seed, ((uint64_t)(m0 + i * 32 + 4 * half + piece + 8 * ((r0 >> 2) + g)) * (uint64_t)fp + (uint64_t)col) >> 2);
                    zl[g] = (uint32_t)z; zh[g] = (uint32_t)(z >> 32);
                }
            }
            // the same factors in the same order as bn_bwd_reduce_kernel: up = dX m; dH = h > 0 ? up ds : 0; xhat = (Y' - mu) inv
            // (a row or column outside: dX, m and Y' arrive as 0 -> dH = 0 adds nothing, and its store is dropped)
            auto element = [&](const int q, const float ds) __attribute__((always_inline)) {
                const float u = up[q] * m[q];
                const float h = y[q] * sc + sh;
                const float dh = h > 0.0f ? u * ds : 0.0f;
                const float xh = (y[q] - mu) * iv;
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, dh), rc, (int)(coff + (uint32_t)(rin(i, r0 + q) * ldc) * 4u), 0, 0);
                s1 += (double)dh;
                s2 += (double)(dh * xh);
            };
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                element(4 * g + 0, bx_keep(bx_quad_bcast<0>(zl[g]), bx_quad_bcast<0>(zh[g]), piece, t16, keep));
                element(4 * g + 1, bx_keep(bx_quad_bcast<1>(zl[g]), bx_quad_bcast<1>(zh[g]), piece, t16, keep));
                element(4 * g + 2, bx_keep(bx_quad_bcast<2>(zl[g]), bx_quad_bcast<2>(zh[g]), piece, t16, keep));
                element(4 * g + 3, bx_keep(bx_quad_bcast<3>(zl[g]), bx_quad_bcast<3>(zh[g]), piece, t16, keep));
            }
        }
        s1 += __shfl_xor(s1, 32);
        s2 += __shfl_xor(s2, 32);
        if (half == 0 && cok)
            *reinterpret_cast<double2*>(pa->ep.slab + ((size_t)(m0 / BX_EPI_ROWS) * fp + col) * 2) = make_double2(s1, s2);
    }
}

}  // namespace eagcn
