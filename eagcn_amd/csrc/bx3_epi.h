// The BatchNorm-backward tail pass of the plane GEMM's NT units (bx3.h BxBnEpi; gemm_bx3.hip bx_compute runs it behind its stream).
#pragma once
#include "bx3.h"
#include "common.h"
#include "kernels.h"

namespace eagcn {

typedef float bx_epi_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t bx_epi_u32x4 __attribute__((ext_vector_type(4)));

// One wave's 64 x 64 block at (m0, n0) of an NT product with p.ep set, BEHIND the stream of the wave (m0, n0 multiples of 64; the caller
// has checked m0 < Mlim and n0 < p.N, both uniform over the wave; every lane of the wave takes part).  The block was stored as ever
// (MFMA D layout) and is read back from memory (L2: the lines were written a moment ago), so the pass is free to choose its lane map,
// and behind barrier B_end the 128 accumulator registers are dead.  ROW-MAJOR, 16 bytes per access: lane l owns the four adjacent
// columns n0 + 4 (l & 15) .. + 3 of the rows m0 + 4 t + (l >> 4), t = 0 .. 15 -- sixteen lanes cover a 64-column row, one wave
// instruction four rows, sixteen instructions the block.
//   * TWO load batches, nothing used before the last request: Y', the row mask and the BatchNorm table (32 + 16 loads) go out while
//     the wave's stores of the block drain, the sixteen dX loads behind the wait for those stores, and the block's sixteen dropout
//     draws are hashed while dX is on its way: 144 registers of operands + 32 of draws.  (The first version walked the D layout in
//     eight dependent batches of 24 scalar loads, each behind the stores of the batch before, with the Y' / C descriptors in vector
//     registers -- a loop over the lanes round every load and store.  Pair launch of configs[1], rocprofv3 medians of 48 launches,
//     eagcn_set_hidden_bn_sums at 1 | 0: 57.6 | 45.4 us then = 12.2 us of tail; 49.2 | 45.5 us now = 3.7 us:
//     profiles/pair_tail_speed.txt.  With everything requested behind the wait, and the draws hashed behind the loads: 5.9 us.)
//   * memory: BUFFER loads and stores over the block's rows inside the matrix (Y', the row mask and C each get a descriptor that ends
//     with the block's last row below Mlim; a lane whose columns are outside asks beyond it): what lies outside arrives as zero and
//     is not written -- one code path for whole and partial blocks, no predicate and no 64-bit lane address per element.  N and the
//     row strides are multiples of 4 (the caller's contract: layer.hip), so a lane's four columns are inside or outside together;
//   * dropout: the one 64-bit draw that serves four adjacent columns of a row (drop_scale4) is exactly a lane's float4;
//   * sums: fp64, in-lane over the lane's 16 rows, two exchanges (lane ^ 16, lane ^ 32) over the four row groups, lanes 0-15 write
//     their four columns of slab row m0 / 64.
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
    const int grp = lane >> 4, col = n0 + 4 * (lane & 15);
    const uint64_t seed = pa->ep.do_drop ? (pa->ep.seed_dev ? *pa->ep.seed_dev : pa->ep.seed) : 0ull;
    // (no dropout: threshold 0 keeps every element at scale 1 -- the same code, nothing drawn)
    const uint32_t t16 = pa->ep.do_drop ? pa->ep.thr >> 16 : 0u;
    const float keep = pa->ep.do_drop ? pa->ep.inv_keep : 1.0f;
    const int rows_in = min(64, Mlim - m0);
    const uint32_t OUTSIDE = 0x80000000u;              // beyond every num_records below (64 rows of a matrix)
    // (base and extent through readfirstlane: the 64-bit row offset was formed in vector registers, and every load and store of Y' and
    //  C sat in a loop over the lanes' descriptors)
    auto rows_of = [&](const float* base, int ld) __attribute__((always_inline)) {
        const uint64_t a = (uint64_t)(uintptr_t)base + (uint64_t)m0 * (uint64_t)ld * 4u;
        const uint64_t s = ((uint64_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
        return __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)s, 0, __builtin_amdgcn_readfirstlane(rows_in * ld * 4), 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc((void*)(pa->ep.row_m + m0), 0, rows_in * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = rows_of(pa->ep.Y, ldy);
    const __amdgpu_buffer_rsrc_t rc = rows_of(pa->C, ldc);
    const bool cok = col < pa->N;
    const int cl = cok ? col : 0;
    const uint32_t yoff = cok ? (uint32_t)(grp * ldy + col) * 4u : OUTSIDE, coff = cok ? (uint32_t)(grp * ldc + col) * 4u : OUTSIDE;
    // what does not depend on this wave's stores of the block (Y', the row mask, the BatchNorm table) is requested while they drain
    bx_epi_f32x4 up[16], y[16];
    float m[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        y[t] = __builtin_bit_cast(bx_epi_f32x4, __builtin_amdgcn_raw_buffer_load_b128(ry, (int)(yoff + (uint32_t)(4 * t * ldy) * 4u), 0, 0));
        m[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rm, (4 * t + grp) * 4, 0, 0));
    }
    float sc[4], sh[4], mu[4], iv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        sc[c] = pa->ep.bn[BN_SC * fp + cl + c]; sh[c] = pa->ep.bn[BN_SH * fp + cl + c];
        mu[c] = pa->ep.bn[BN_MU * fp + cl + c]; iv[c] = pa->ep.bn[BN_INV * fp + cl + c];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's stores of the block have left
#pragma unroll
    for (int t = 0; t < 16; ++t)                       // (glc: past the vector cache -- the lines were written by this wave's stores)
        up[t] = __builtin_bit_cast(bx_epi_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rc, (int)(coff + (uint32_t)(4 * t * ldc) * 4u), 0, 1));
    // the block's sixteen draws while dX is on its way (the empty asm keeps the hashes HERE: the compiler placed each one behind the
    // wait for its row's loads, where nothing hides it)
    uint32_t zlo[16], zhi[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) zlo[t] = zhi[t] = 0u;
    if (pa->ep.do_drop) {
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const uint64_t z = rng_u64(seed, ((uint64_t)(m0 + 4 * t + grp) * (uint64_t)fp + (uint64_t)col) >> 2);
            zlo[t] = (uint32_t)z; zhi[t] = (uint32_t)(z >> 32);
        }
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) asm volatile("" : "+v"(zlo[t]), "+v"(zhi[t]));
    asm volatile("" ::: "memory");                     // every load of the block is requested before the first store
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const float ds[4] = {(zlo[t] & 0xFFFFu) >= t16 ? keep : 0.0f, (zlo[t] >> 16) >= t16 ? keep : 0.0f,
                             (zhi[t] & 0xFFFFu) >= t16 ? keep : 0.0f, (zhi[t] >> 16) >= t16 ? keep : 0.0f};
        // the same factors in the same order as bn_bwd_reduce_kernel: up = dX m; dH = h > 0 ? up ds : 0; xhat = (Y' - mu) inv
        // (a row or column outside: dX, m and Y' arrive as 0 -> dH = 0 adds nothing, and its store is dropped)
        bx_epi_f32x4 dh4;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float u = up[t][c] * m[t];
            const float h = y[t][c] * sc[c] + sh[c];
            const float dh = h > 0.0f ? u * ds[c] : 0.0f;
            const float xh = (y[t][c] - mu[c]) * iv[c];
            dh4[c] = dh;
            s1[c] += (double)dh;
            s2[c] += (double)(dh * xh);
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(bx_epi_u32x4, dh4), rc, (int)(coff + (uint32_t)(4 * t * ldc) * 4u), 0, 0);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        s1[c] += __shfl_xor(s1[c], 16); s2[c] += __shfl_xor(s2[c], 16);
        s1[c] += __shfl_xor(s1[c], 32); s2[c] += __shfl_xor(s2[c], 32);
    }
    if (grp == 0 && cok) {
        double2* sl = reinterpret_cast<double2*>(pa->ep.slab + ((size_t)(m0 / BX_EPI_ROWS) * fp + col) * 2);
#pragma unroll
        for (int c = 0; c < 4; ++c) sl[c] = make_double2(s1[c], s2[c]);
    }
}

}  // namespace eagcn
