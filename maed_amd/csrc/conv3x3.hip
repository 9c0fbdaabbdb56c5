// 3x3 convolutions of the backbone as implicit GEMMs on the tile / swizzled LDS image / LDS-shuffled epilogue of gemm.hip's
// gemm_nt_glds_bf16_kernel: 128-row tiles (any shape; also the stride-2 input gradient by parity classes) and one frame per workgroup
// (stage 3 of the R50).  The weight gradient lives in conv3x3_rows.hip.  Compiled as part of gemm.hip's translation unit (its last line includes
// this file) and therefore NOT a member of the SOURCES lists of maed_amd/build.py and tests/hostsim/build_sim.py, which both count it as a header of
// every object; it compiles alone only for scripts/isa_audit.py.
#include "common.cuh"
#include "gemm_epilogue.cuh"
#include "gemm_tile.cuh"
#include "gemm_x3.h"

// ------------------------------------------------------------------------------------------------
// 3x3 convolution as an implicit GEMM on the same tile / LDS image / epilogue as gemm_nt_glds_bf16_kernel<EPI, 1>
// (resnetv2.py:74-93 StdConv2dSame 3x3: 16 of the backbone's 53 convolutions; today they run on MIOpen).
//   out[m][co] = sum_{tap, ci} X[pixel(m) shifted by tap][ci] * Wt[co][tap*Cin + ci]      m = (f, oy, ox), channels_last
// A-operand rows are GATHERED: every lane of the LDS-DMA computes its own source address, so "im2col" costs nothing -- for K tile
// kt the tap is (kt*64)/Cin (Cin % 64 == 0: a K tile never straddles taps), and a lane whose shifted pixel falls outside the image
// points at a 128-byte page of zeros instead (TF-SAME zero padding, any stride).  The input gradient of a stride-1 convolution is
// the same kernel on dY with the flipped, transposed weight image.  Default path of the backbone since it was timed against MIOpen
// on MI355X (resnetv2.py; profiles/r02_call1_conv3x3_micro.txt).
// ------------------------------------------------------------------------------------------------
// B (weight) addressing: element (n, tap, c) of the GEMM's B operand lives at Wt[b_base + tap * b_tap + n * b_row + c]
struct Conv3x3Dims { int F, H, W, Cin, Ho, Wo, stride, pad_top, pad_left; int64_t b_row, b_tap, b_base;
                     // CLS (one parity class of a stride-2 input gradient, maed_conv3x3_s2_dgrad): nty x ntx taps; loop tap (ty, tx) pairs with the FORWARD tap
                     // (ky0 - 2 ty, kx0 - 2 tx); output pixel (f, a, b) of the class is row (f * o_h + 2 a + o_py) * o_w + 2 b + o_px of dX
                     int nty = 3, ntx = 3, ky0 = 0, kx0 = 0, o_h = 0, o_w = 0, o_py = 0, o_px = 0; };

// CLS: row m = (f, a, b) of a parity class -> its row of dX
__device__ __forceinline__ int64_t cv_class_row(const Conv3x3Dims& d, int64_t m) {
    const int b = (int)(m % d.Wo), a = (int)((m / d.Wo) % d.Ho);
    const int64_t f = m / ((int64_t)d.Wo * d.Ho);
    return (f * d.o_h + 2 * a + d.o_py) * (int64_t)d.o_w + 2 * b + d.o_px;
}

// NARROW: 128 x 64 output tile for Cout <= 64 (stage 1 of the R50: a 128-wide tile would spend half its MFMAs on duplicated weight rows):
// the four waves take 32 pixel rows each and both 32-column halves; only 64 weight rows are staged.
template <int EPI, bool NARROW, bool GN, bool CLS = false>
__global__ __launch_bounds__(256, 4) void conv3x3_glds_bf16_kernel(const bf16* __restrict__ X, const bf16* __restrict__ Wt, const bf16* __restrict__ zero_page,
                                                                   Conv3x3Dims d, int64_t M, int64_t N, int tiles_n, EpiArgs e) {
    constexpr int kTileElems = 2 * GM_BM * GM_BK, kStageElems = 4 * 32 * GL_ST * 2;
    constexpr int kMainElems = kTileElems > kStageElems ? kTileElems : kStageElems;
    __shared__ __attribute__((aligned(1024))) unsigned short lds_raw[kMainElems + (GN ? GN_TAB_FLOATS * 2 : 0)];   // (+ GroupNorm-statistics table)
    unsigned short (*lds)[GM_BM * GM_BK] = reinterpret_cast<unsigned short (*)[GM_BM * GM_BK]>(lds_raw);     // [A|B][128*64]
    double* const gn_tab = reinterpret_cast<double*>(lds_raw + kMainElems);
    if (GN && threadIdx.x < GN_TAB_FLOATS / 2) gn_tab[threadIdx.x] = 0.0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = NARROW ? wave : wave >> 1, wc = NARROW ? 0 : wave & 1, l31 = lane & 31, hi = lane >> 5;
    const int id = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t m0 = (int64_t)(id / tiles_n) * GM_BM, n0 = (int64_t)(id % tiles_n) * (NARROW ? 64 : GM_BN);
    const int nkt = (CLS ? d.nty * d.ntx : 9) * d.Cin / GM_BK;
    const int srow = wave * 8 + (lane >> 3);
    const int schunk = (lane & 7) ^ ((4 * wave + (lane >> 4)) & 7);
    // per staging round i: the output pixel of this lane's A row (top-left input tap, element offset of it) and its B row
#define CV_PTRS(i)                                                                                        \
    int iy##i, ix##i; int64_t aoff##i; const bf16* gbp##i;                                                \
    {                                                                                                     \
        const int row = srow + 32 * i;                                                                    \
        const int64_t m = (m0 + row < M) ? m0 + row : M - 1;                                              \
        const int ox = (int)(m % d.Wo), oy = (int)((m / d.Wo) % d.Ho);                                    \
        const int64_t f = m / ((int64_t)d.Wo * d.Ho);                                                     \
        iy##i = oy * d.stride - d.pad_top; ix##i = ox * d.stride - d.pad_left;                            \
        aoff##i = ((f * d.H + iy##i) * d.W + ix##i) * (int64_t)d.Cin + schunk * 8;                        \
        const int64_t br = (n0 + row < N) ? n0 + row : N - 1;                                             \
        gbp##i = Wt + d.b_base + br * d.b_row + schunk * 8;                                               \
    }
    CV_PTRS(0) CV_PTRS(1) CV_PTRS(2) CV_PTRS(3)
#define CV_ISSUE1(i, ty_, tx_, toff_, k0_)                                                                                            \
    {                                                                                                                                 \
        const bool ok = (unsigned)(iy##i + ty_) < (unsigned)d.H && (unsigned)(ix##i + tx_) < (unsigned)d.W;                           \
        const bf16* src = ok ? X + aoff##i + toff_ : zero_page + schunk * 8;                                                          \
        __builtin_amdgcn_global_load_lds((glb_void_t*)src, (lds_void_t*)&lds[0][(4 * i + wave) * 8 * GM_BK], 16, 0, 0);               \
        if (!NARROW || i < 2)                                                                                                         \
            __builtin_amdgcn_global_load_lds((glb_void_t*)(gbp##i + k0_), (lds_void_t*)&lds[1][(4 * i + wave) * 8 * GM_BK], 16, 0, 0); \
    }
    f32x16_t acc[4];                                                // [32-row block of pixels][32-column block]; NARROW: the first two
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int fsw = (l31 >> 1) & 7;
    int ty = 0, tx = 0, c0 = 0;                                     // K tile -> (tap, channel chunk), advanced incrementally (wave-uniform)
    for (int kt = 0; kt < nkt; ++kt) {
        const int64_t k0 = (int64_t)(CLS ? (d.ky0 - 2 * ty) * 3 + (d.kx0 - 2 * tx) : ty * 3 + tx) * d.b_tap + c0;     // B offset of this K tile
        const int64_t toff = ((int64_t)ty * d.W + tx) * d.Cin + c0;
        CV_ISSUE1(0, ty, tx, toff, k0) CV_ISSUE1(1, ty, tx, toff, k0) CV_ISSUE1(2, ty, tx, toff, k0) CV_ISSUE1(3, ty, tx, toff, k0)
        MAED_WAIT_VMCNT0();
        __syncthreads();
        // transposed tiles: lane = output row (pixel)
        mfma_ktile_swizzled<(NARROW ? 1 : 2), 2>(&lds[0][(wr * (NARROW ? 32 : 64) + l31) * GM_BK], &lds[1][(wc * 64 + l31) * GM_BK], hi, fsw, acc);
        __syncthreads();
        c0 += GM_BK;
        if (c0 == d.Cin) { c0 = 0; if (++tx == (CLS ? d.ntx : 3)) { tx = 0; ++ty; } }
    }
#undef CV_PTRS
#undef CV_ISSUE1
    // LDS-shuffled epilogue (gemm_epilogue.cuh), as in gemm_nt_glds_bf16_kernel; CLS: a row of the class lands on its row of dX
    const bool vec_ok = (e.ldo % 8 == 0) && (e.ldaux % 8 == 0);
    float* stg = reinterpret_cast<float*>(lds_raw) + wave * 32 * GL_ST;
    const int64_t col0 = n0 + wc * 64 + (lane & 7) * 8;
    const GnTile gnt = GN ? gn_tile(gn_tab, m0, n0, N, e.gn_hw) : GnTile{nullptr, 0, 0, 0};
    GnRegs gnr;
    if constexpr (GN) gn_zero(gnr);
    const auto out_row = [&](int64_t row) { return CLS ? cv_class_row(d, row) : row; };
#pragma unroll
    for (int i = 0; i < (NARROW ? 1 : 2); ++i)
        epilogue_shuffled<EPI, bf16, GN>(acc[2 * i], acc[2 * i + 1], stg, lane, e, m0 + wr * (NARROW ? 32 : 64) + i * 32, col0, M, N, vec_ok, true, true, &gnr, &gnt, out_row);
    if constexpr (GN) {
        gn_commit(gnr, gnt, lane, col0, N);
        __syncthreads();
        gn_flush(gnt, e.gn_sums, m0, M, e.gn_hw, NARROW ? 64 : GM_BN, tid, 256);
    }
}

// ------------------------------------------------------------------------------------------------
// Round 6 (second session): the same implicit GEMM on ONE FRAME x 128 output channels per workgroup, for feature maps of at most 256 pixels (stage 3 of the R50:
// 14 x 14 = 196; cfg5: 16 x 16).  Why: at stage 3 the 128 x 128 tiling gives 392 workgroups -- 1.5 per CU.  Its single-buffered loop costs a workgroup one exposed copy
// round trip per K tile (36 of them: ~45 us whoever shares the CU), and the CUs that got two workgroups move 2.3 MB through the LDS-DMA path in that time, which is what
// that path gives a CU (~50 GB/s): latency-bound and fill-bound at once, more workgroups of the same kind re-read more (r06_conv3x3_narrow_tiles_rejected.txt).  A frame
// tile has NO imbalance (128 frames x 2 column tiles = 256 workgroups = one per CU), moves 1.6 MB per CU (a frame's 196 rows + 128 weight rows per K tile: the weight
// rows are shared by twice the pixels) and, alone on its CU, can afford a ring: three stages of 48 KB, copies two K tiles ahead, ONE barrier per K tile.
// Eight waves: wave w owns pixel rows 32 w .. 32 w + 31 of the frame (rows past the frame: nothing to copy, nothing to multiply) against all 128 columns
// (four 32 x 32 accumulators); GroupNorm statistics as in the 128-row kernel (a tile is one frame: the table's second frame stays empty).
// ------------------------------------------------------------------------------------------------
#define CF_STAGES 3
#define CF_A_ELEMS (256 * GM_BK)
#define CF_STAGE_ELEMS (CF_A_ELEMS + 128 * GM_BK)          // 48 KB
template <int EPI, bool GN>
__global__ __launch_bounds__(512, 2) void conv3x3_frame_bf16_kernel(const bf16* __restrict__ X, const bf16* __restrict__ Wt, const bf16* __restrict__ zero_page,
                                                                    Conv3x3Dims d, int64_t M, int64_t N, int tiles_n, EpiArgs e) {
    MAED_DYN_SHARED(unsigned short, lds);                     // CF_STAGES x [A: 256 x 64][B: 128 x 64] (+ the GroupNorm-statistics table)
    double* const gn_tab = reinterpret_cast<double*>(lds + CF_STAGES * CF_STAGE_ELEMS);
    if (GN && threadIdx.x < GN_TAB_FLOATS / 2) gn_tab[threadIdx.x] = 0.0;          // (published by the main loop's barriers)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, hi = lane >> 5;
    const int id = xcd_remap(blockIdx.x, gridDim.x);
    const int HW = d.Ho * d.Wo;
    const int f = id / tiles_n;
    const int64_t m0 = (int64_t)f * HW, n0 = (int64_t)(id % tiles_n) * 128;
    const bool active = wave * 32 < HW;                       // wave-uniform: this wave has pixel rows
    const int nkt = 9 * d.Cin / GM_BK;
    // copies: round j of A = this wave's rows 8 j .. 8 j + 7 (one 1 KB instruction), round j of B = weight rows 16 wave + 8 j ..; the 16-byte chunk a lane copies
    // undoes the fragment reads' swizzle: slot (lane & 7) of row r holds chunk slot ^ ((r >> 1) & 7), and (r >> 1) & 7 = (4 j + (lane >> 4)) & 7 for both operands
    int iy[4], ix[4]; int64_t aoff[4]; const bf16* gbp[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int sch = (lane & 7) ^ ((4 * j + (lane >> 4)) & 7);
        int p = wave * 32 + 8 * j + (lane >> 3);
        if (p > HW - 1) p = HW - 1;
        const int ox = p % d.Wo, oy = p / d.Wo;
        iy[j] = oy * d.stride - d.pad_top; ix[j] = ox * d.stride - d.pad_left;
        aoff[j] = (((int64_t)f * d.H + iy[j]) * d.W + ix[j]) * (int64_t)d.Cin + sch * 8;
        if (j < 2) {
            const int64_t br = n0 + 16 * wave + 8 * j + (lane >> 3);
            gbp[j] = Wt + d.b_base + (br < N ? br : N - 1) * d.b_row + sch * 8;
        }
    }
    const int zch = ((lane & 7)) * 8;                         // any chunk of the zero page
#define CF_ISSUE(stage_, ty_, tx_, toff_, k0_) {                                                                                          \
        unsigned short* const sa__ = lds + (stage_) * CF_STAGE_ELEMS;                                                                     \
        if (active) {                                                                                                                     \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                                               \
                const bool ok = (unsigned)(iy[j] + (ty_)) < (unsigned)d.H && (unsigned)(ix[j] + (tx_)) < (unsigned)d.W;                   \
                const bf16* src = ok ? X + aoff[j] + (toff_) : zero_page + zch;                                                           \
                MAED_LDS_DMA16_PTR(src, sa__ + (32 * wave + 8 * j) * GM_BK);                                                              \
            }                                                                                                                             \
        }                                                                                                                                 \
        _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                                     \
            MAED_LDS_DMA16_PTR(gbp[j] + (k0_), sa__ + CF_A_ELEMS + (16 * wave + 8 * j) * GM_BK);                                          \
    }
    f32x16_t acc[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
    const int fsw = (l31 >> 1) & 7;
    // the copy stream runs two K tiles ahead of the products: its own (tap, channel chunk) counters
    int ity = 0, itx = 0, ic0 = 0;
#define CF_ISSUE_NEXT(stage_) {                                                                                                           \
        const int64_t k0__ = (int64_t)(ity * 3 + itx) * d.b_tap + ic0;                                                                    \
        const int64_t toff__ = ((int64_t)ity * d.W + itx) * d.Cin + ic0;                                                                  \
        CF_ISSUE(stage_, ity, itx, toff__, k0__)                                                                                          \
        ic0 += GM_BK;                                                                                                                     \
        if (ic0 == d.Cin) { ic0 = 0; if (++itx == 3) { itx = 0; ++ity; } }                                                                \
    }
    CF_ISSUE_NEXT(0)
    CF_ISSUE_NEXT(1)                                            // (nkt >= 9)
    for (int kt = 0; kt < nkt; ++kt) {
        // tile kt has landed once at most the younger tile's copies (6 per active wave, 2 per idle one) are outstanding
        if (kt + 1 < nkt) { if (active) { MAED_WAIT_VMCNT(6); } else { MAED_WAIT_VMCNT(2); } } else { MAED_WAIT_VMCNT0(); }
        __syncthreads();                                        // ... for every wave; and every wave is done with tile kt - 1: its stage is free
        if (kt + 2 < nkt) CF_ISSUE_NEXT((kt + 2) % CF_STAGES)
        if (active) {
            const unsigned short* const st = lds + (kt % CF_STAGES) * CF_STAGE_ELEMS;
            mfma_ktile_swizzled<1, 4>(st + (wave * 32 + l31) * GM_BK, st + CF_A_ELEMS + l31 * GM_BK, hi, fsw, acc);      // transposed tiles: lane = output row (pixel)
        }
    }
#undef CF_ISSUE_NEXT
#undef CF_ISSUE
    // LDS-shuffled epilogue as in the 128-row kernels: a wave's 32 x 64 half through its private staging area (in the ring: the first barrier inside
    // is also "every wave is done with the last K tile"); an idle wave only meets the barriers; statistics committed per half
    const bool vec_ok = (e.ldo % 8 == 0) && (e.ldaux % 8 == 0);
    float* stg = reinterpret_cast<float*>(lds) + wave * 32 * GL_ST;
    const GnTile gnt = GN ? gn_tile(gn_tab, m0, n0, N, HW) : GnTile{nullptr, 0, 0, 0};
    GnRegs gnr;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int64_t c0 = n0 + h * 64 + (lane & 7) * 8;
        if constexpr (GN) gn_zero(gnr);
        epilogue_shuffled<EPI, bf16, GN>(acc[2 * h], acc[2 * h + 1], stg, lane, e, m0 + wave * 32, c0, m0 + HW, N, vec_ok, true, active, &gnr, &gnt);
        if constexpr (GN) { if (active) gn_commit(gnr, gnt, lane, c0, N); }
    }
    if constexpr (GN) {
        __syncthreads();
        gn_flush(gnt, e.gn_sums, m0, M, HW, 128, tid, 512);
    }
}

extern "C" int maed_conv3x3_fwd(const void* x, const void* w_taps, const void* zero_page, void* y, int F, int H, int W, int Cin, int Cout,
                                int stride, int pad_top, int pad_left, int Ho, int Wo, const void* add, int w_layout, int dtype, double* gn_sums,
                                void* stream) {
    MAED_CHECK_ARG(!gn_sums || (gn_stats_shape_ok(Cout, (int64_t)Ho * Wo) && !add), MAED_ERR_SHAPE,
                   "conv3x3_fwd: GroupNorm statistics need Cout = 32 * 2^k >= 64, Ho*Wo >= 128 and no `add` (Cout=%d Ho*Wo=%d)", Cout, Ho * Wo);
    MAED_CHECK_ARG(w_layout == 0 || w_layout == 1, MAED_ERR_ARG, "conv3x3_fwd: w_layout must be 0 (Cout,3,3,Cin) or 1 (transposed image of the forward weight)");
    MAED_CHECK_ARG(x && w_taps && zero_page && y, MAED_ERR_ARG, "conv3x3_fwd: null pointer");
    const int np_call = maed_x3_take_dtype(dtype);
    MAED_CHECK_ARG(dtype == MAED_BF16 || dtype == MAED_F32, MAED_ERR_ARG, "conv3x3_fwd: bad dtype %d", dtype);
    const int x3np = dtype == MAED_F32 ? (np_call ? np_call : maed_x3_planes()) : 0;
    MAED_CHECK_ARG(dtype == MAED_BF16 || x3np, MAED_ERR_UNSUPPORTED, "conv3x3_fwd: f32 needs the split-bf16 matmul mode (maed_set_option(MAED_OPT_F32_MATMUL, 1 or 2))");
    MAED_CHECK_ARG(F >= 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && stride >= 1 && pad_top >= 0 && pad_left >= 0, MAED_ERR_SHAPE, "conv3x3_fwd: bad extents");
    MAED_CHECK_ARG(Cin % (dtype == MAED_F32 ? 32 : GM_BK) == 0 && Cout % 8 == 0, MAED_ERR_SHAPE, "conv3x3_fwd: need Cin %% 64 == 0 (f32: 32) and Cout %% 8 == 0 (Cin=%d Cout=%d)", Cin, Cout);
    MAED_CHECK_ARG((Ho - 1) * stride - pad_top + 2 < H + 2 && (Wo - 1) * stride - pad_left + 2 < W + 2, MAED_ERR_SHAPE, "conv3x3_fwd: output extent exceeds the padded input");
    MAED_CHECK_ARG(is_aligned(x, 16) && is_aligned(w_taps, 16) && is_aligned(zero_page, 16) && is_aligned(y, 16), MAED_ERR_ALIGN, "conv3x3_fwd: 16-B alignment");
    if (F == 0) return MAED_OK;
    const int64_t M = (int64_t)F * Ho * Wo, N = Cout;
    const int tm = (int)((M + GM_BM - 1) / GM_BM);
    // 128 x 64 output tiles for Cout <= 64, and (MAED_OPT_CONV3X3_NARROW_WGS) wherever 128 x 128 tiles would leave the chip with too few workgroups to hide the
    // single-buffered loop's copy latency (stage 3 of the R50: 392 workgroups = 1.5 per CU)
    const bool narrow = N <= 64 || (int64_t)tm * ((N + GM_BN - 1) / GM_BN) < maed_opt(MAED_OPT_CONV3X3_NARROW_WGS);
    const int tn = narrow ? (int)((N + 63) / 64) : (int)((N + GM_BN - 1) / GM_BN);
    // layout 0: w_taps[co][tap][ci].  layout 1 (input gradient from the forward weight's transposed image Wt[tap_f][c_f][o_f], as
    // maed_weight_std_fwd writes it next to the forward image): here Cin = O_f, Cout = I_f, and element (n = c_f, tap, c = o_f) is
    // Wt[(8 - tap)][n][c] -- the tap flip is a negative tap stride, nothing is copied.
    const Conv3x3Dims d = w_layout == 0
        ? Conv3x3Dims{F, H, W, Cin, Ho, Wo, stride, pad_top, pad_left, 9 * (int64_t)Cin, (int64_t)Cin, 0}
        : Conv3x3Dims{F, H, W, Cin, Ho, Wo, stride, pad_top, pad_left, (int64_t)Cin, -(int64_t)Cout * Cin, 8 * (int64_t)Cout * Cin};
    EpiArgs e{nullptr, y, (int64_t)Cout, nullptr, add, (int64_t)Cout, gn_sums, Ho * Wo};
    if (dtype == MAED_F32) {        // fp32 operands on the split-bf16 MFMA kernel (gemm_x3.hip): out-of-image taps are zeros in registers, zero_page unused
        const X3ConvDims xd{d.F, d.H, d.W, d.Cin, d.Ho, d.Wo, d.stride, d.pad_top, d.pad_left, d.b_row, d.b_tap, d.b_base};
        MAED_PROPAGATE(maed_conv3x3_x3_launch(x3np, x, w_taps, xd, M, Cout, e, add != nullptr, gn_sums != nullptr, (hipStream_t)stream));
        MAED_CHECK_LAUNCH("conv3x3_fwd(x3)");
        return MAED_OK;
    }
    // one frame x 128 channels per workgroup where a frame is at most 256 pixels and the frames fill the chip (stage 3 of the R50)
    const int fhw = Ho * Wo;
    const int fopt = maed_opt(MAED_OPT_CONV3X3_FRAME);     // 2: whenever the shape allows (tests)
    if (fopt && fhw <= 256 && fhw > 128 && N % 8 == 0 && ((int64_t)F * ((N + 127) / 128) >= 192 || fopt == 2) && (!gn_sums || gn_stats_shape_ok(Cout, fhw))) {
        const int ftn = (int)((N + 127) / 128);
        constexpr size_t lds_bytes = (size_t)CF_STAGES * CF_STAGE_ELEMS * 2 + GN_TAB_FLOATS * 4;
        static bool attr_set = false;
        if (!attr_set) {
            (void)hipFuncSetAttribute((const void*)conv3x3_frame_bf16_kernel<MAED_EPI_ADD, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            (void)hipFuncSetAttribute((const void*)conv3x3_frame_bf16_kernel<MAED_EPI_STORE, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            (void)hipFuncSetAttribute((const void*)conv3x3_frame_bf16_kernel<MAED_EPI_STORE, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            attr_set = true;
        }
#define CF_LAUNCH(EPI_, GN_) hipLaunchKernelGGL((conv3x3_frame_bf16_kernel<EPI_, GN_>), dim3((unsigned)(F * ftn)), dim3(512), lds_bytes, (hipStream_t)stream, (const bf16*)x, \
                                                (const bf16*)w_taps, (const bf16*)zero_page, d, M, N, ftn, e)
        if (add) CF_LAUNCH(MAED_EPI_ADD, false); else if (gn_sums) CF_LAUNCH(MAED_EPI_STORE, true); else CF_LAUNCH(MAED_EPI_STORE, false);
#undef CF_LAUNCH
        MAED_CHECK_LAUNCH("conv3x3_fwd(frame)");
        return MAED_OK;
    }
    const dim3 grid((unsigned)(tm * tn));
#define CV_LAUNCH(EPI_, NARROW_, GN_) hipLaunchKernelGGL((conv3x3_glds_bf16_kernel<EPI_, NARROW_, GN_>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)x, \
                                                   (const bf16*)w_taps, (const bf16*)zero_page, d, M, N, tn, e)
    if (add) { if (narrow) CV_LAUNCH(MAED_EPI_ADD, true, false); else CV_LAUNCH(MAED_EPI_ADD, false, false); }
    else if (gn_sums) { if (narrow) CV_LAUNCH(MAED_EPI_STORE, true, true); else CV_LAUNCH(MAED_EPI_STORE, false, true); }
    else { if (narrow) CV_LAUNCH(MAED_EPI_STORE, true, false); else CV_LAUNCH(MAED_EPI_STORE, false, false); }
#undef CV_LAUNCH
    MAED_CHECK_LAUNCH("conv3x3_fwd");
    return MAED_OK;
}

// Input gradient of a STRIDE-2 3x3 SAME convolution (resnetv2.py:74-93: conv2 of the first block of stages 2 and 3) as four implicit GEMMs, one per parity
// class of the input pixel: dX[f, iy, ix, :] = sum over the forward taps (ky, kx) with (iy + pad_top - ky) and (ix + pad_left - kx) EVEN of
// dY[f, (iy + pad_top - ky) / 2, (ix + pad_left - kx) / 2, :] W[:, ky, kx, :] -- a pixel of parity (py, px) sees 2 or 1 taps per axis (9/4 of the dense
// kernel's multiply-adds in total), each class is a small stride-1 convolution over dY whose outputs land on every second row / column of dX.  Same kernel as the
// forward (gathered LDS-DMA rows, zero page for taps outside dY), transposed forward-weight image read in place; the four launches cover dX: no zero-fill.
// Replaces MIOpen's backward-data solver for these two layers together with the padded / sliced copies its symmetric-padding interface forced
// (0.3 ms per cfg3 step, profiles/r03_rocprofv3_last_step_kernel_sequence.txt).
extern "C" int maed_conv3x3_s2_dgrad(const void* dy, const void* wt_image, const void* zero_page, void* dx, int F, int H, int W, int Cin, int Cout,
                                     int pad_top, int pad_left, int Ho, int Wo, int dtype, void* stream) {
    // H, W, Cin: the forward convolution's INPUT (= dX) extents and channels; Ho, Wo, Cout: its output (= dY); wt_image (3,3,Cin,Cout) as maed_weight_std_fwd writes it
    MAED_CHECK_ARG(dy && wt_image && zero_page && dx, MAED_ERR_ARG, "conv3x3_s2_dgrad: null pointer");
    MAED_CHECK_ARG(dtype == MAED_BF16, MAED_ERR_UNSUPPORTED, "conv3x3_s2_dgrad: bf16 only (dtype=%d)", dtype);
    MAED_CHECK_ARG(F >= 0 && H > 1 && W > 1 && Ho > 0 && Wo > 0 && pad_top >= 0 && pad_top <= 1 && pad_left >= 0 && pad_left <= 1, MAED_ERR_SHAPE, "conv3x3_s2_dgrad: bad extents");
    MAED_CHECK_ARG(Cout % GM_BK == 0 && Cin % 8 == 0, MAED_ERR_SHAPE, "conv3x3_s2_dgrad: need Cout %% 64 == 0 and Cin %% 8 == 0 (Cin=%d Cout=%d)", Cin, Cout);
    MAED_CHECK_ARG(is_aligned(dy, 16) && is_aligned(wt_image, 16) && is_aligned(zero_page, 16) && is_aligned(dx, 16), MAED_ERR_ALIGN, "conv3x3_s2_dgrad: 16-B alignment");
    MAED_CHECK_ARG((uint64_t)F * H * W * Cin * 2 < (1ull << 32) && (uint64_t)F * Ho * Wo * Cout * 2 < (1ull << 32), MAED_ERR_SHAPE, "conv3x3_s2_dgrad: tensor larger than 4 GB");
    if (F == 0) return MAED_OK;
    const int64_t N = Cin;
    const bool narrow = N <= 64;
    const int tn = narrow ? 1 : (int)((N + GM_BN - 1) / GM_BN);
    EpiArgs e{nullptr, dx, (int64_t)Cin, nullptr, nullptr, (int64_t)Cin};
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px) {
            const int Ha = (H - py + 1) / 2, Wb = (W - px + 1) / 2;                 // pixels of this class per frame
            if (Ha <= 0 || Wb <= 0) continue;
            const int ey = (py + pad_top) & 1, ex = (px + pad_left) & 1;            // parity the forward tap must have
            const int nty = ey ? 1 : 2, ntx = ex ? 1 : 2;
            // forward taps ky = ey + 2 jy read dY row a + (py + pad_top - ey) / 2 - jy; loop tap ty = nty - 1 - jy walks the rows upwards
            const int base_y = (py + pad_top - ey) / 2 - (nty - 1), base_x = (px + pad_left - ex) / 2 - (ntx - 1);
            Conv3x3Dims d{F, Ho, Wo, Cout, Ha, Wb, 1, -base_y, -base_x, (int64_t)Cout, (int64_t)Cin * Cout, 0};
            d.nty = nty; d.ntx = ntx; d.ky0 = ey + 2 * (nty - 1); d.kx0 = ex + 2 * (ntx - 1); d.o_h = H; d.o_w = W; d.o_py = py; d.o_px = px;
            const int64_t M = (int64_t)F * Ha * Wb;
            const dim3 grid((unsigned)(((M + GM_BM - 1) / GM_BM) * tn));
            if (narrow) hipLaunchKernelGGL((conv3x3_glds_bf16_kernel<MAED_EPI_STORE, true, false, true>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)dy,
                                           (const bf16*)wt_image, (const bf16*)zero_page, d, M, N, tn, e);
            else hipLaunchKernelGGL((conv3x3_glds_bf16_kernel<MAED_EPI_STORE, false, false, true>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)dy,
                                    (const bf16*)wt_image, (const bf16*)zero_page, d, M, N, tn, e);
        }
    MAED_CHECK_LAUNCH("conv3x3_s2_dgrad");
    return MAED_OK;
}
