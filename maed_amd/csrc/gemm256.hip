// nn.Linear family on 256x256x64 tiles with a counted-vmcnt LDS-DMA pipeline (bf16, fp32 accumulation): the kernel behind
// maed_gemm_nt for the large-M shapes of the STE (vision_transformer.py:98-111,124-128,147,176) and the wide 1x1 convolutions.
//
// Why a second tile size.  Measured ablation of the 128x128 kernel at the qkv shape (profiles/r02_gemm_ablation.txt): loads alone
// 28 us (21 TB/s L2->LDS: the load path is saturated), MFMA + fragment reads alone 28 us, stores alone 18 us -- and 59 us together:
// the three barely overlap, because with 32 KB of LDS per workgroup only ~64 KB of loads are in flight per CU, and a 128x128 tile
// needs 64 B/clk/CU of operand traffic at the MFMA rate.  A 256x256 tile needs half of that, and the schedule below keeps 64 KB of
// LDS-DMA in flight per CU at every moment of the main loop.
//
// Geometry, LDS ring, the four-phase K tile, the counted vmcnt(8) wait and the staggered wave groups: gemm256_pipe.cuh -- the pipeline this kernel shares with
// gemm_sk.hip and gemm_tn_sk.hip.  Here one workgroup computes ONE output tile: prologue, steady K-tile pairs, a tail that drains with vmcnt(6/4/2/0), epilogue.
//
// Epilogue: the fused epilogues of gemm_epilogue.cuh through the same LDS shuffle as the 128x128 kernel (a lane owns one output row in
// the transposed accumulators; each wave parks 32 x 64 fp32 in LDS and stores full 128/256-byte row segments).
#include "common.cuh"
#include "gemm_epilogue.cuh"
#include "gemm_internal.h"
#define P256_COMPUTE_GUARD if (!(ablate & 4))      // (ablate: a constant 0 outside the diagnostic build)
#include "gemm256_pipe.cuh"

template <int EPI>
__global__ __launch_bounds__(512, 2) void gemm_nt_256_bf16_kernel(const bf16* __restrict__ A, int64_t lda, const bf16* __restrict__ B, int64_t ldb,
                                                                   int64_t M, int64_t N, int64_t K, int tiles_n, EpiArgs e
#ifdef MAED_GEMM_ABLATE
                                                                   , int ablate    // diagnostic build only: 1 no stores, 2 no loads, 4 no MFMA / fragment reads
#endif
                                                                   ) {
#ifndef MAED_GEMM_ABLATE
    constexpr int ablate = 0;
#endif
    __shared__ __attribute__((aligned(1024))) unsigned short lds_raw[P256_RING_ELEMS];            // 128 KB; the epilogue re-uses it
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);        // scalar: LDS-DMA bases (M0) and the wave-group branches stay on the SALU
    const int wr = wave >> 2, wc = wave & 3;
    const int l31 = lane & 31, hi = lane >> 5;
    const int id = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t m0 = (int64_t)(id / tiles_n) * P256_T, n0 = (int64_t)(id % tiles_n) * P256_T;
    const int nkt = (int)(K / P256_BK);                                                            // >= 2 (host-checked)

    // ---- staging map: a half-tile is 128 rows x 128 B = 1024 chunks of 16 B, two per thread (round i = 0, 1); wave w fills slot rows
    //      8w + 64i .. +7, lane l the (swizzled) chunk of row 8w + 64i + (l>>3).  Slot row s of A-half q is tile row (s>>6)*128 + q*64 + (s&63)
    //      (the 64 rows of quadrant row q of M-wave s>>6); slot row s of B-half q is tile column (s>>5)*64 + q*32 + (s&31).
    const int r = wave * 8 + (lane >> 3);                                                          // slot row of round 0
    const int schunk = (lane & 7) ^ ((r >> 1) & 7);
    uint32_t ao0, ao1, ao2, ao3, bo0, bo1, bo2, bo3;                                               // index 2*i + q; BYTE offsets (host-checked < 4 GB)
#define G2_OFFS(j)                                                                                  \
    {                                                                                               \
        const int i_ = (j) >> 1, q_ = (j) & 1;                                                      \
        int64_t ar = m0 + i_ * 128 + q_ * 64 + r;                                                   \
        int64_t br = n0 + ((r >> 5) + 2 * i_) * 64 + q_ * 32 + (r & 31);                            \
        if (ar > M - 1) ar = M - 1;                                                                 \
        if (br > N - 1) br = N - 1;                                                                 \
        ao##j = (uint32_t)((ar * lda + schunk * 8) * 2); bo##j = (uint32_t)((br * ldb + schunk * 8) * 2); \
    }
    G2_OFFS(0) G2_OFFS(1) G2_OFFS(2) G2_OFFS(3)
#undef G2_OFFS
    unsigned short* const ldsw = lds_raw + wave * 8 * P256_BK;                                      // this wave's rows of round 0 inside a slot (scalar)
    const char* const Ab = reinterpret_cast<const char*>(A);
    const char* const Bb = reinterpret_cast<const char*>(B);
    // one LDS-DMA per thread: scalar base (operand + K tile kt_: always a real K tile, the tail issues nothing) + 32-bit lane offset:
    // global_load_lds_dwordx4 v_off, s[base:base+1] -- no VALU per DMA.  (Both operands' bases are formed at every copy, the unused one included: where the
    // compiler first meets a base is where it places that base's scalar arithmetic among the prologue's copies.)
#define G2_DMA(op_, kt_, off_, buf_, slot_, i_)                                                     \
    if (!(ablate & 2)) {                                                                            \
        const char* const ak__ = Ab + (int64_t)(kt_) * (P256_BK * 2);                               \
        const char* const bk__ = Bb + (int64_t)(kt_) * (P256_BK * 2);                               \
        MAED_LDS_DMA16(op_##k__, off_, ldsw + ((buf_) * 4 + (slot_)) * P256_SLOT + (i_) * 64 * P256_BK); \
    }
#define P256_DMA_A(kt_, off_, buf_, slot_, i_) G2_DMA(a, kt_, off_, buf_, slot_, i_)
#define P256_DMA_B(kt_, off_, buf_, slot_, i_) G2_DMA(b, kt_, off_, buf_, slot_, i_)
#define P256_PA1 ao1                                // (one tile: the A1 offsets are the same for every K tile)
#define P256_PA3 ao3
#define P256_READ_A P256_NT_READ_A
#define P256_READ_B0 P256_NT_READ_B0
#define P256_READ_B1 P256_NT_READ_B1
    P256_NT_FRAG_BASES()
    P256_DECLARE_REGS()
    P256_ZERO_ACC()
    // the last two or three K tiles, t_ in buffer b_ (o_ = the other buffer); h1_ / h2_: K tile t+1 / t+2 exists (wave-uniform): issue what is left, drain with
    // the exact counts
#define G2_TAIL_PHASE(READS_, h_, DMA_, kt_, o0_, o1_, buf_, slot_, WAIT_, c0_, c1_, bq_)           \
    P256_PHASE(READS_, if (h_) DMA_(kt_, o0_, buf_, slot_, 0), if (h_) DMA_(kt_, o1_, buf_, slot_, 1), WAIT_, c0_, c1_, bq_, )
#define G2_KTILE(b_, o_, t_)                                                                                                                  \
    {                                                                                                                                         \
        const bool h1_ = (t_) + 1 < nkt, h2_ = (t_) + 2 < nkt;                                                                                \
        G2_TAIL_PHASE(P256_READ_A(b_, P256_A0) P256_READ_B0(b_), h1_, P256_DMA_A, (t_) + 1, ao1, ao3, o_, P256_A1, if (h1_) MAED_WAIT_VMCNT(8); else MAED_WAIT_VMCNT(0), c000, c010, b0) \
        G2_TAIL_PHASE(P256_READ_B1(b_), h2_, P256_DMA_A, (t_) + 2, ao0, ao2, b_, P256_A0, if (h2_) MAED_WAIT_VMCNT(8); else if (h1_) MAED_WAIT_VMCNT(6), c001, c011, b1) \
        G2_TAIL_PHASE(P256_READ_A(b_, P256_A1), h2_, P256_DMA_B, (t_) + 2, bo0, bo2, b_, P256_B0, if (h2_) MAED_WAIT_VMCNT(8); else if (h1_) MAED_WAIT_VMCNT(4), c101, c111, b1) \
        G2_TAIL_PHASE(, h2_, P256_DMA_B, (t_) + 2, bo1, bo3, b_, P256_B1, if (h2_) MAED_WAIT_VMCNT(8); else if (h1_) MAED_WAIT_VMCNT(2), c100, c110, b0) \
    }

    // ---- prologue: K tile 0 whole and A0, B0, B1 of K tile 1; A0, B0, B1 of tile 0 must have landed
    P256_PROLOGUE(0, 1)
    MAED_WAIT_VMCNT(8);
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();        // waves 4-7 run one barrier behind (wave-uniform branch)
    int t = 0;
    for (; t + 3 < nkt; t += 2) {                     // steady state, two tiles per trip (static buffer index): tiles t, t+1 <= nkt-3
        P256_PAIR(MAED_WAIT_VMCNT(8), t + 1, t + 2, t + 3)
    }
    for (; t < nkt; t += 2) {                         // the last two or three tiles: issue and wait by what is left
        G2_KTILE(0, 1, t)
        if (t + 1 < nkt) G2_KTILE(1, 0, t + 1)
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();        // re-align the two groups: nobody reads operand tiles past this point

    // ---- epilogue: per (qm, rt) a 32 x 64 piece of the wave's tile through its private LDS staging area
    const bool vec_ok = epilogue_vec_ok<EPI, bf16, 8>(e);
    float* stg = reinterpret_cast<float*>(lds_raw) + wave * 32 * GL_ST;
    const int64_t c0 = n0 + wc * 64 + (lane & 7) * 8;
    const int64_t r0 = m0 + wr * 128;
    const bool st = !(ablate & 1);
    epilogue_shuffled<EPI, bf16>(c000, c001, stg, lane, e, r0, c0, M, N, vec_ok, st);           // (qm, rt) = (0, 0): rows qm * 64 + rt * 32 of the wave's 128
    epilogue_shuffled<EPI, bf16>(c010, c011, stg, lane, e, r0 + 32, c0, M, N, vec_ok, st);
    epilogue_shuffled<EPI, bf16>(c100, c101, stg, lane, e, r0 + 64, c0, M, N, vec_ok, st);
    epilogue_shuffled<EPI, bf16>(c110, c111, stg, lane, e, r0 + 96, c0, M, N, vec_ok, st);
}

template <int EPI>
static void launch_256(const void* A, int64_t lda, const void* B, int64_t ldb, int64_t M, int64_t N, int64_t K, const EpiArgs& e, hipStream_t s) {
    const int tm = (int)((M + P256_T - 1) / P256_T), tn = (int)((N + P256_T - 1) / P256_T);
#ifdef MAED_GEMM_ABLATE
    hipLaunchKernelGGL((gemm_nt_256_bf16_kernel<EPI>), dim3((unsigned)(tm * tn)), dim3(512), 0, s, (const bf16*)A, lda, (const bf16*)B, ldb, M, N, K, tn, e, maed_opt(MAED_OPT_ABLATE));
#else
    hipLaunchKernelGGL((gemm_nt_256_bf16_kernel<EPI>), dim3((unsigned)(tm * tn)), dim3(512), 0, s, (const bf16*)A, lda, (const bf16*)B, ldb, M, N, K, tn, e);
#endif
}

// called by maed_gemm_nt's dispatcher (gemm.hip); returns false for epilogues this kernel does not carry (fp32 atomics: split-K)
bool maed_gemm_nt_256_launch(int epilogue, const void* A, int64_t lda, const void* B, int64_t ldb, int64_t M, int64_t N, int64_t K, const EpiArgs& e,
                             hipStream_t s) {
    return epilogue_switch<EPI_SET_STORES>(epilogue, [&](auto epi) { launch_256<decltype(epi)::value>(A, lda, B, ldb, M, N, K, e, s); });
}
