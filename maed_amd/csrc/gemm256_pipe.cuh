// The 256x256x64 half-tile K-stream pipeline (bf16, fp32 accumulation): the ONE definition of the main loop of gemm256.hip (one output tile per workgroup),
// gemm_sk.hip (persistent stream of work items) and gemm_tn_sk.hip (weight gradient, transposing fragment reads).  Macros over named scalar registers: the kernels
// expand them inside their bodies, nothing here is a function (accumulators and fragments in arrays or behind references get demoted to scratch).
//
// Geometry.  8 waves = 2 (wr) x 4 (wc); a wave owns 128 x 64 of the output = 4 quadrants of 64 x 32 (2 MFMA 32x32x16 tiles each), 128 accumulator registers.  A K tile
// (BK = 64) is four 16-KB HALF-TILES: A0 / A1 = what every wave needs of the first operand for its quadrant row qm = 0 / 1, B0 / B1 = the second operand for quadrant
// column qn = 0 / 1.  The ring = 2 buffers x 4 half-tile slots = 128 KB, slots in consumption order (A0, B0, B1, A1), filled by LDS-DMA (16 B per lane, two copies
// per thread and half-tile: "round" i = 0, 1).  What a slot's image looks like -- and with it the copy's source offsets and the fragment reads -- is the kernel's:
// [128 rows][64 k] for the NT kernels (below), [64 reduction rows][128 columns] read by ds_read_b64_tr_b16 for gemm_tn_sk.hip.
//
// Schedule (one "phase" = one quadrant: fragment reads, barrier, 8 MFMAs with one half-tile of LDS-DMA issued in their shadow, counted wait, barrier).
// K tile t, phases q = 1..4:
//     q   reads                  MFMA quadrant   LDS-DMA issued between the MFMAs (2 per thread)
//     1   A0 (8) + B0 (4)        (0,0)           A1 of tile t+1
//     2   B1 (4)                 (0,1)           A0 of tile t+2
//     3   A1 (8)                 (1,1)           B0 of tile t+2
//     4   --                     (1,0)           B1 of tile t+2
// Issue order = consumption order, six to seven phases ahead of the read.  Every phase ends with s_waitcnt vmcnt(8), BEHIND its issue: the four most recent
// half-tiles (64 KB) stay in flight, the one issued four phases ago has landed; it is read two phases later at the earliest (the other wave group runs one barrier
// behind), and a slot is re-targeted by a DMA one phase after its last read at the earliest (the issue sits behind the phase's first barrier) -- what LDS-DMA needs
// under staggered wave groups (MI355X_MICROARCH.md: nothing orders a ds_read behind a pending LDS-DMA except the issuing wave's counted vmcnt plus a barrier).
// Waves 4-7 run one barrier behind waves 0-3 (one wave of each group per SIMD): while one group issues its MFMAs the other reads fragments, and s_setprio favours
// the group in its MFMA segment (an LDS-DMA costs the wave 100-185 issue cycles next to fragment reads, ~60 between MFMAs).  Raw s_barrier only: a __syncthreads()
// would drain the DMA queue.  Transposed tiles (first MFMA operand = the B fragment): a lane owns one output ROW and 4 consecutive columns per register group.
//
// Hooks.  Defined by the kernel BEFORE this header is included (optional, default: nothing):
//     P256_COMPUTE_GUARD        prefix of the blocks that hold a phase's fragment reads and its MFMAs (gemm256.hip's ablation build: if (!(ablate & 4)))
//     P256_AFTER_MFMA_A(qm_)    block behind the MFMAs of a phase that read A half qm_ (gemm_tn_sk.hip: column sums of those fragments)
//     P256_AFTER_MFMA           the same for the phases that read no A half
// defined by the kernel before it expands P256_PROLOGUE / P256_PAIR:
//     P256_READ_A(buf_, slot_) / P256_READ_B0(buf_) / P256_READ_B1(buf_)      fragment reads (P256_NT_READ_* below, or the kernel's own)
//     P256_DMA_A(k_, off_, buf_, slot_, i_) / P256_DMA_B(...)                  ONE copy of round i_ of the A / B operand at K position k_, lane offset off_
//     P256_PA1 / P256_PA3                                                      the offsets of the A1 half still to be issued for the pair's even tile
#pragma once
#include "common.cuh"

#define P256_T 256
#define P256_BK 64
#define P256_SLOT (128 * P256_BK)                       // elements per half-tile slot (16 KB)
#define P256_A0 0                                       // slot order inside a buffer: consumption order
#define P256_B0 1
#define P256_B1 2
#define P256_A1 3
#define P256_RING_ELEMS (2 * 4 * P256_SLOT)             // 128 KB
#define P256_LDS_ELEMS (P256_RING_ELEMS + 4 * 2048)     // + 16 KB: epilogue staging of waves 4-7 (the persistent kernels)
#define P256_STAGE_BYTE0 (7 * P256_SLOT * 2)            // staging of wave w: byte offset P256_STAGE_BYTE0 + w * 4096 (buffer 1 slot A1, then the extra 16 KB)

// wave-uniform values the compiler must keep in SGPRs (loop-carried values of the item bookkeeping end up in VGPRs otherwise)
#define P256_UNI(x_) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x_)))
// a lane value the compiler must not see through: what is derived from it is recomputed where it is used instead of living in registers across the K stream
#ifdef MAED_HOSTSIM
#define P256_OPAQUE(v_) ((void)0)
#else
#define P256_OPAQUE(v_) asm volatile("" : "+v"(v_))
#endif

#ifndef P256_COMPUTE_GUARD
#define P256_COMPUTE_GUARD
#endif
#ifndef P256_AFTER_MFMA
#define P256_AFTER_MFMA
#endif
#ifndef P256_AFTER_MFMA_A
#define P256_AFTER_MFMA_A(qm_) P256_AFTER_MFMA
#endif

// ---- registers: named scalars (never demoted to scratch)
#define P256_DECLARE_REGS()                                                                         \
    bf16x8_t a00, a01, a02, a03, a10, a11, a12, a13;            /* a[rt][kk] */                     \
    bf16x8_t b00, b01, b02, b03, b10, b11, b12, b13;            /* b[qn][kk] */                     \
    f32x16_t c000, c001, c010, c011, c100, c101, c110, c111;    /* c[qm][rt][qn] */
#define P256_ZERO_ACC()                                                                             \
    _Pragma("unroll") for (int x = 0; x < 16; ++x) { c000[x] = 0.f; c001[x] = 0.f; c010[x] = 0.f; c011[x] = 0.f; c100[x] = 0.f; c101[x] = 0.f; c110[x] = 0.f; c111[x] = 0.f; }

// ---- NT operand path (gemm256.hip, gemm_sk.hip): a slot is a [128][64] bf16 image, 16-B chunk index XOR-swizzled with (row>>1)&7 on the LDS-DMA SOURCE address
//      (the DMA writes base + lane*16) and on the ds_read_b128 fragment reads: conflict-free.  A rows wr*64 + rt*32 + l31 of slot A[qm], B rows wc*32 + l31 of
//      slot B[qn]; chunk (2*kk + hi) ^ fsw.  One base per (operand, kk): everything else -- buffer, slot, rt -- is a compile-time offset < 64 KB (the ds_read immediate).
//      Expects lds_raw, wr, wc, l31, hi.
#define P256_NT_FRAG_BASES()                                                                        \
    const int fsw = (l31 >> 1) & 7;                                                                 \
    const char* const ldsb = reinterpret_cast<const char*>(lds_raw);                                \
    const char* const fa0 = ldsb + (wr * 64 + l31) * (P256_BK * 2) + ((0 + hi) ^ fsw) * 16;         \
    const char* const fa1 = ldsb + (wr * 64 + l31) * (P256_BK * 2) + ((2 + hi) ^ fsw) * 16;         \
    const char* const fa2 = ldsb + (wr * 64 + l31) * (P256_BK * 2) + ((4 + hi) ^ fsw) * 16;         \
    const char* const fa3 = ldsb + (wr * 64 + l31) * (P256_BK * 2) + ((6 + hi) ^ fsw) * 16;         \
    const char* const fb0 = ldsb + (wc * 32 + l31) * (P256_BK * 2) + ((0 + hi) ^ fsw) * 16;         \
    const char* const fb1 = ldsb + (wc * 32 + l31) * (P256_BK * 2) + ((2 + hi) ^ fsw) * 16;         \
    const char* const fb2 = ldsb + (wc * 32 + l31) * (P256_BK * 2) + ((4 + hi) ^ fsw) * 16;         \
    const char* const fb3 = ldsb + (wc * 32 + l31) * (P256_BK * 2) + ((6 + hi) ^ fsw) * 16;
#define P256_NT_FRAG(base_, buf_, slot_, rowoff_) (*reinterpret_cast<const bf16x8_t*>((base_) + (((buf_) * 4 + (slot_)) * P256_SLOT + (rowoff_) * P256_BK) * 2))
#define P256_NT_READ_A(buf_, slot_)                                                                                                                             \
    a00 = P256_NT_FRAG(fa0, buf_, slot_, 0); a01 = P256_NT_FRAG(fa1, buf_, slot_, 0); a02 = P256_NT_FRAG(fa2, buf_, slot_, 0); a03 = P256_NT_FRAG(fa3, buf_, slot_, 0); \
    a10 = P256_NT_FRAG(fa0, buf_, slot_, 32); a11 = P256_NT_FRAG(fa1, buf_, slot_, 32); a12 = P256_NT_FRAG(fa2, buf_, slot_, 32); a13 = P256_NT_FRAG(fa3, buf_, slot_, 32);
#define P256_NT_READ_B0(buf_) b00 = P256_NT_FRAG(fb0, buf_, P256_B0, 0); b01 = P256_NT_FRAG(fb1, buf_, P256_B0, 0); b02 = P256_NT_FRAG(fb2, buf_, P256_B0, 0); b03 = P256_NT_FRAG(fb3, buf_, P256_B0, 0);
#define P256_NT_READ_B1(buf_) b10 = P256_NT_FRAG(fb0, buf_, P256_B1, 0); b11 = P256_NT_FRAG(fb1, buf_, P256_B1, 0); b12 = P256_NT_FRAG(fb2, buf_, P256_B1, 0); b13 = P256_NT_FRAG(fb3, buf_, P256_B1, 0);

// ---- one phase: fragment reads ; barrier ; fragments landed ; 8 MFMAs at raised priority with the phase's two LDS-DMA instructions (ISSUE0_, ISSUE1_) in their
//      shadow ; AFTER_ ; counted wait ; barrier.  bq_ = b0 / b1: the B fragments of quadrant column qn.
#define P256_PHASE(READS_, ISSUE0_, ISSUE1_, WAIT_, c0_, c1_, bq_, AFTER_)                          \
    P256_COMPUTE_GUARD { READS_ }                                                                   \
    __builtin_amdgcn_s_barrier();                                                                   \
    MAED_WAIT_LGKMCNT0();                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    __builtin_amdgcn_s_setprio(1);                                                                  \
    P256_COMPUTE_GUARD {                                                                            \
        c0_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bq_##0, a00, c0_, 0, 0, 0);                   \
        c1_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bq_##0, a10, c1_, 0, 0, 0);                   \
    }                                                                                               \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    ISSUE0_;                                                                                        \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    P256_COMPUTE_GUARD {                                                                            \
        c0_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bq_##1, a01, c0_, 0, 0, 0);                   \
        c1_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bq_##1, a11, c1_, 0, 0, 0);                   \
        c0_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bq_##2, a02, c0_, 0, 0, 0);                   \
    }                                                                                               \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    ISSUE1_;                                                                                        \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    P256_COMPUTE_GUARD {                                                                            \
        c1_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bq_##2, a12, c1_, 0, 0, 0);                   \
        c0_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bq_##3, a03, c0_, 0, 0, 0);                   \
        c1_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bq_##3, a13, c1_, 0, 0, 0);                   \
    }                                                                                               \
    AFTER_                                                                                          \
    __builtin_amdgcn_s_setprio(0);                                                                  \
    WAIT_;                                                                                          \
    __builtin_amdgcn_s_barrier();
#define P256_NONE ((void)0)

// ---- prologue: K tile k0_ whole (buffer 0) and A0, B0, B1 of K tile k1_ (buffer 1) -- seven half-tiles in the issue order of the steady state
#define P256_PROLOGUE(k0_, k1_)                                                                     \
    P256_DMA_A(k0_, ao0, 0, P256_A0, 0); P256_DMA_A(k0_, ao2, 0, P256_A0, 1);                       \
    P256_DMA_B(k0_, bo0, 0, P256_B0, 0); P256_DMA_B(k0_, bo2, 0, P256_B0, 1);                       \
    P256_DMA_B(k0_, bo1, 0, P256_B1, 0); P256_DMA_B(k0_, bo3, 0, P256_B1, 1);                       \
    P256_DMA_A(k0_, ao1, 0, P256_A1, 0); P256_DMA_A(k0_, ao3, 0, P256_A1, 1);                       \
    P256_DMA_A(k1_, ao0, 1, P256_A0, 0); P256_DMA_A(k1_, ao2, 1, P256_A0, 1);                       \
    P256_DMA_B(k1_, bo0, 1, P256_B0, 0); P256_DMA_B(k1_, bo2, 1, P256_B0, 1);                       \
    P256_DMA_B(k1_, bo1, 1, P256_B1, 0); P256_DMA_B(k1_, bo3, 1, P256_B1, 1);

// ---- K-tile pair (t, t+1), t in buffer 0:
//        even tile  q1: A1(t+1) [P256_PA1 / P256_PA3 at kpa_]   q2..q4: A0, B0, B1 of tile t+2 [ao / bo at k0_]
//        odd tile   q1: A1(t+2) [ao1 / ao3 at k0_]              q2..q4: A0, B0, B1 of tile t+3 [ao / bo at k1_]
//      EVENWAIT_: the wait of the even tile's four phases (the persistent kernels run the FIRST pair of an item without waits: everything issued before has landed)
#define P256_PAIR(EVENWAIT_, kpa_, k0_, k1_)                                                                                                                                    \
    P256_PHASE(P256_READ_A(0, P256_A0) P256_READ_B0(0), P256_DMA_A(kpa_, P256_PA1, 1, P256_A1, 0), P256_DMA_A(kpa_, P256_PA3, 1, P256_A1, 1), EVENWAIT_, c000, c010, b0, P256_AFTER_MFMA_A(0)) \
    P256_PHASE(P256_READ_B1(0), P256_DMA_A(k0_, ao0, 0, P256_A0, 0), P256_DMA_A(k0_, ao2, 0, P256_A0, 1), EVENWAIT_, c001, c011, b1, P256_AFTER_MFMA)                              \
    P256_PHASE(P256_READ_A(0, P256_A1), P256_DMA_B(k0_, bo0, 0, P256_B0, 0), P256_DMA_B(k0_, bo2, 0, P256_B0, 1), EVENWAIT_, c101, c111, b1, P256_AFTER_MFMA_A(1))                 \
    P256_PHASE(, P256_DMA_B(k0_, bo1, 0, P256_B1, 0), P256_DMA_B(k0_, bo3, 0, P256_B1, 1), EVENWAIT_, c100, c110, b0, P256_AFTER_MFMA)                                           \
    P256_PHASE(P256_READ_A(1, P256_A0) P256_READ_B0(1), P256_DMA_A(k0_, ao1, 0, P256_A1, 0), P256_DMA_A(k0_, ao3, 0, P256_A1, 1), MAED_WAIT_VMCNT(8), c000, c010, b0, P256_AFTER_MFMA_A(0)) \
    P256_PHASE(P256_READ_B1(1), P256_DMA_A(k1_, ao0, 1, P256_A0, 0), P256_DMA_A(k1_, ao2, 1, P256_A0, 1), MAED_WAIT_VMCNT(8), c001, c011, b1, P256_AFTER_MFMA)                     \
    P256_PHASE(P256_READ_A(1, P256_A1), P256_DMA_B(k1_, bo0, 1, P256_B0, 0), P256_DMA_B(k1_, bo2, 1, P256_B0, 1), MAED_WAIT_VMCNT(8), c101, c111, b1, P256_AFTER_MFMA_A(1))        \
    P256_PHASE(, P256_DMA_B(k1_, bo1, 1, P256_B1, 0), P256_DMA_B(k1_, bo3, 1, P256_B1, 1), MAED_WAIT_VMCNT(8), c100, c110, b0, P256_AFTER_MFMA)

// ---- wave-private staging area of the persistent kernels' epilogues: 16 rows x 256 B of fp32 at stg_, 16-byte chunk c of row r at slot c ^ r.  Row half h_ of a
//      32 x 64 piece (accumulators accA_ | accB_): the lanes that hold it (rhalf == h_; r16_ = their row) write their eight float4 ...
#define P256_STAGE_WRITE_HALF(accA_, accB_, h_, stg_, r16_)                                                                 \
    MAED_WAVE_LDS_SYNC();                                                                                                   \
    if (rhalf == (h_)) {                                                                                                    \
        _Pragma("unroll") for (int q4 = 0; q4 < 4; ++q4) {                                                                  \
            *reinterpret_cast<float4*>((stg_) + (r16_) * 256 + (((2 * q4 + hi) ^ (r16_)) << 4)) = make_float4(accA_[4 * q4], accA_[4 * q4 + 1], accA_[4 * q4 + 2], accA_[4 * q4 + 3]);      \
            *reinterpret_cast<float4*>((stg_) + (r16_) * 256 + (((8 + 2 * q4 + hi) ^ (r16_)) << 4)) = make_float4(accB_[4 * q4], accB_[4 * q4 + 1], accB_[4 * q4 + 2], accB_[4 * q4 + 3]);  \
        }                                                                                                                   \
    }                                                                                                                       \
    MAED_WAVE_LDS_SYNC();
//      ... and all lanes read full row segments back: lane (row lr_, 8-lane column c8_) gets 8 consecutive floats u0_ | u1_ (8 lanes cover 64 columns)
#define P256_STAGE_READ8(u0_, u1_, stg_, lr_, c8_)                                                                          \
    const float4 u0_ = *reinterpret_cast<const float4*>((stg_) + (lr_) * 256 + (((2 * (c8_)) ^ (lr_)) << 4));               \
    const float4 u1_ = *reinterpret_cast<const float4*>((stg_) + (lr_) * 256 + (((2 * (c8_) + 1) ^ (lr_)) << 4));
