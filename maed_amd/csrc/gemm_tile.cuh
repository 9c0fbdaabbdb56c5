// Tile geometry and K-tile product shared by the 128x128 direct-to-LDS NT GEMM (gemm.hip) and the implicit-GEMM 3x3 convolutions that
// use the same LDS image (conv3x3.hip).
#pragma once
#include "common.cuh"

#define GM_BM 128
#define GM_BN 128
#define GM_BK 64

// One K tile (GM_BK) of products from the swizzled LDS image: unpadded 128-byte rows whose 16-byte chunk index is XOR-ed by (row >> 1) & 7.
// As / Bs: this lane's first fragment row (row base + lane & 31) of each operand; NA / NB blocks of 32 rows follow each other; hi = lane >> 5,
// fsw = ((lane & 31) >> 1) & 7.  acc[ia * NB + ib] is the 32x32 tile of A block ia and B block ib.  TR: transposed tiles (first MFMA operand =
// B rows), so that a lane owns one output row (see epilogue_shuffled); the atomic epilogue keeps the natural orientation.
// (acc indices are compile-time after unrolling: the accumulators stay registers)
template <int NA, int NB, bool TR = true>
__device__ __forceinline__ void mfma_ktile_swizzled(const unsigned short* As, const unsigned short* Bs, int hi, int fsw, f32x16_t (&acc)[4]) {
    static_assert(NA * NB <= 4, "four accumulators");
#pragma unroll
    for (int kk = 0; kk < GM_BK / 16; ++kk) {
        const int co = ((kk * 2 + hi) ^ fsw) * 8;
        bf16x8_t a[NA], b[NB];
#pragma unroll
        for (int ia = 0; ia < NA; ++ia) a[ia] = *reinterpret_cast<const bf16x8_t*>(As + ia * 32 * GM_BK + co);
#pragma unroll
        for (int ib = 0; ib < NB; ++ib) b[ib] = *reinterpret_cast<const bf16x8_t*>(Bs + ib * 32 * GM_BK + co);
#pragma unroll
        for (int ia = 0; ia < NA; ++ia)
#pragma unroll
            for (int ib = 0; ib < NB; ++ib)
                acc[ia * NB + ib] = TR ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[ib], a[ia], acc[ia * NB + ib], 0, 0, 0)
                                       : __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ia], b[ib], acc[ia * NB + ib], 0, 0, 0);
    }
}
