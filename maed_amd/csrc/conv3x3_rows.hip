// Weight gradient of the stride-1 3x3 SAME convolution (resnetv2.py:74-93; the conv2 of every stage-1 bottleneck) for 64 -> 64 channels, one IMAGE ROW at a time:
//   dW[co][tap][ci] += sum_x dy[f, y, x][co] * x[f, y + ky - 1, x + kx - 1][ci]
// The general TN kernel (gemm_tn.hip) treats this as a (pixels x 64)^T (pixels x 576) GEMM on 128 x 128 output tiles: half of every tile is empty at 64 output
// channels, and the dy tile is transposed through registers once per K tile (five times).  Here a work item is one image row (f, y): its dy row and the three
// input rows y - 1 .. y + 1 are copied into LDS unchanged by LDS-DMA -- the input rows into a ring of row slots, so a workgroup walking consecutive rows
// fetches ONE new input row per item; the copies run three items ahead (14 KB per item and workgroup: with one item in flight the launch was bound by the DMA
// round trip, 82 us) -- and all nine taps are contracted from there: wave = tap, operands through ds_read_b64_tr_b16 of the row-major images (the
// tap's column shift is a pointer offset, the image borders are zero pixels that frame every row slot; rows above / below the image: the wave skips the item).
// Same scheme as the stem's weight gradient (stem.hip).  Chunk c of pixel slot s is stored at c ^ 4 * ((s >> 1) & 1): pixel rows are 128 bytes apart and a
// transposing read covers four consecutive pixels.
#include "common.cuh"
#include "prof.h"

#define R3_ROWPX 66                       // pixel slots per ring row: zero pixel, up to 64 image pixels, zero pixel
#define R3_ROW_ELEMS (R3_ROWPX * 64)
#define R3_DY_ELEMS (64 * 64)             // dy buffer: 64 pixel slots (slots >= W stay zero)
#define R3_THREADS 576                    // nine waves: one per tap
#define R3_RING 8                         // input-row slots: rows g - 1 .. g + 4 are live at item g (three in use, three on their way); 8 for the mask
#define R3_NDY 4                          // dy row buffers: item g in use, g + 1 .. g + 3 on their way
#define R3_LDS_BYTES ((R3_RING * R3_ROW_ELEMS + R3_NDY * R3_DY_ELEMS) * 2)       // 100 KB: one workgroup per CU

__global__ __launch_bounds__(R3_THREADS, 1) void conv3x3_wgrad_rows64_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ x, float* __restrict__ dW,
                                                                               float* __restrict__ partial, int H, int W, int n_rows, int rows_per_wg) {
    MAED_DYN_SHARED(unsigned short, smem);
    const int tid = threadIdx.x, lane = tid & 63, tap = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, hi = lane >> 5, i16 = lane & 15;
    const int ky = tap / 3, kx = tap - 3 * ky;
    const int g0 = blockIdx.x * rows_per_wg;
    int g1 = g0 + rows_per_wg;
    if (g1 > n_rows) g1 = n_rows;
    if (g0 >= g1) return;
    for (int i = tid; i < R3_LDS_BYTES / 16; i += R3_THREADS) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    unsigned short* const ring = smem;
    unsigned short* const dyb = smem + R3_RING * R3_ROW_ELEMS;
    const int row_chunks = W * 8, n_instr = row_chunks >> 6;          // W % 8 == 0 (host-checked): whole wave-instructions of 64 chunks
    const int64_t row_bytes = (int64_t)W * 128;
    // position p of a row's chunks = (pixel p >> 3, LDS chunk p & 7); the global chunk that belongs there undoes the slot swizzle
#define R3_ISSUE_X(g_) if (tap < n_instr) { const int g__ = (g_); const int p = tap * 64 + lane, px = p >> 3, c = p & 7; \
        MAED_LDS_DMA16((const char*)x + g__ * row_bytes, (uint32_t)((px * 8 + (c ^ ((((px + 1) >> 1) & 1) << 2))) * 16), ring + (g__ & (R3_RING - 1)) * R3_ROW_ELEMS + 64 + tap * 512); }
#define R3_ISSUE_DY(g_, b_) if (tap < n_instr) { const int g__ = (g_); const int p = tap * 64 + lane, px = p >> 3, c = p & 7; \
        MAED_LDS_DMA16((const char*)dy + g__ * row_bytes, (uint32_t)((px * 8 + (c ^ (((px >> 1) & 1) << 2))) * 16), dyb + ((b_) & (R3_NDY - 1)) * R3_DY_ELEMS + tap * 512); }

    f32x16_t acc[2][2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][0][r] = 0.f; acc[0][1][r] = 0.f; acc[1][0][r] = 0.f; acc[1][1][r] = 0.f; }
    // transposing reads: pixel row 4 hi + (i16 >> 2) (+ 8) of a 16-pixel k-step, channels (lane & 16) + 4 (i16 & 3) .. (+ 32 for the second channel tile)
    const int prow = 4 * hi + (i16 >> 2), pcol = (lane & 16) + 4 * (i16 & 3);
    const int swa = ((prow >> 1) & 1) << 2, swb = (((prow + kx) >> 1) & 1) << 2;      // bit 1 of the pixel slot: unchanged by + 8 and + 16 s
    const int a_off0 = prow * 64 + ((((pcol >> 3) ^ swa) << 3) | (pcol & 7)), a_off1 = prow * 64 + (((((pcol + 32) >> 3) ^ swa) << 3) | (pcol & 7));
    const int b_off0 = (prow + kx) * 64 + ((((pcol >> 3) ^ swb) << 3) | (pcol & 7)), b_off1 = (prow + kx) * 64 + (((((pcol + 32) >> 3) ^ swb) << 3) | (pcol & 7));
    const int ksteps = (W + 15) >> 4;

    // prefetch of item k: its dy row and input row k + 1 (rows k - 1, k came with the items before); the first item also brings rows g0 - 1, g0
#define R3_PREFETCH(k_) { const int k__ = (k_); if (k__ < g1) { R3_ISSUE_DY(k__, k__ - g0); if (k__ + 1 < n_rows) R3_ISSUE_X(k__ + 1); } }
    if (g0 > 0) R3_ISSUE_X(g0 - 1);
    R3_ISSUE_X(g0);
    R3_PREFETCH(g0);
    R3_PREFETCH(g0 + 1);
    R3_PREFETCH(g0 + 2);
    for (int g = g0; g < g1; ++g) {
        const int b = g - g0;
        // item g's copies are complete once at most the two younger items' (two DMAs per wave each, when they were issued in full) are outstanding
        if (g + 2 < g1 && g + 3 < n_rows) { MAED_WAIT_VMCNT(4); } else { MAED_WAIT_VMCNT0(); }
        __syncthreads();                 // row g's images have landed for every wave; nobody still reads item g - 1's dy buffer and oldest ring slot
        R3_PREFETCH(g + 3);
        const int y = g % H, yy = y + ky - 1;
        if (yy < 0 || yy >= H) continue;                                  // wave-uniform: this tap's input row lies outside the image
        const unsigned short* da = dyb + (b & (R3_NDY - 1)) * R3_DY_ELEMS;
        const unsigned short* xb = ring + ((g + ky - 1) & (R3_RING - 1)) * R3_ROW_ELEMS;
        for (int s = 0; s < ksteps; ++s) {
            union { bf16x8_t v; uint2 u[2]; } a0, a1, b0, b1;
#define R3_FRAG(dst_, base_, off_) { auto lo__ = MAED_DS_READ_TR16((base_) + s * 1024 + (off_)); auto hi__ = MAED_DS_READ_TR16((base_) + s * 1024 + 512 + (off_)); \
            __builtin_memcpy(&dst_.u[0], &lo__, 8); __builtin_memcpy(&dst_.u[1], &hi__, 8); }
            R3_FRAG(a0, da, a_off0) R3_FRAG(a1, da, a_off1) R3_FRAG(b0, xb, b_off0) R3_FRAG(b1, xb, b_off1)
#undef R3_FRAG
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0.v, b0.v, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0.v, b1.v, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1.v, b0.v, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1.v, b1.v, acc[1][1], 0, 0, 0);
        }
    }
#undef R3_PREFETCH
#undef R3_ISSUE_X
#undef R3_ISSUE_DY
    // D[co][ci]: column ci = l31 (+ 32 b), rows (r & 3) + 8 (r >> 2) + 4 hi (+ 32 a);  dW (64, 9, 64).
    // With `partial` the workgroup stores its 64 x 576 block with plain stores into its own slot (summed by wgrad_slots_reduce_kernel): 256 workgroups adding
    // 147 KB each with atomics onto the SAME 147 KB cost 39 of the launch's 80 us (fp32 atomics on a hot spot: ~1 TB/s, the same at workgroup scope).
    float* const base = partial ? partial + (size_t)blockIdx.x * (64 * 576) : dW;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int bt = 0; bt < 2; ++bt) {
            float* d = base + tap * 64 + 32 * bt + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float* e = d + (32 * a + (r & 3) + 8 * (r >> 2) + 4 * hi) * 576;
                if (partial) *e = acc[a][bt][r]; else atomicAdd(e, acc[a][bt][r]);
            }
        }
}

// dW[e] += sum over workgroup slots w of partial[w][e]: 36864 elements, one per thread and slot chunk (grid.y chunks of <= 32 slots: coalesced 1 KB rows)
__global__ __launch_bounds__(256) void wgrad_slots_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dW, int n_slots, int n_elems) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_elems) return;
    const int w0 = blockIdx.y * 32, w1 = min(n_slots, w0 + 32);
    float t0 = 0.f, t1 = 0.f;
    int w = w0;
    for (; w + 1 < w1; w += 2) { t0 += partial[(size_t)w * n_elems + e]; t1 += partial[(size_t)(w + 1) * n_elems + e]; }
    if (w < w1) t0 += partial[(size_t)w * n_elems + e];
    atomicAdd(dW + e, t0 + t1);
}

bool maed_conv3x3_wgrad_rows64_ok(int F, int H, int W, int Cin, int Cout) {
    // (F >= 1: an empty batch has no rows to split over workgroups -- callers get "not applicable" and take the general route, which returns early on M == 0)
    return maed_opt(MAED_OPT_CONV3X3_ROWS_WGS) > 0 && F >= 1 && Cin == 64 && Cout == 64 && W % 8 == 0 && W >= 8 && W <= 64 && H >= 1 && (int64_t)F * H * W * 128 < (1ll << 31);
}

void maed_wgrad_slots_reduce(const float* partial, float* dW, int n_slots, int n_elems, hipStream_t stream) {
    hipLaunchKernelGGL(wgrad_slots_reduce_kernel, dim3((n_elems + 255) / 256, (n_slots + 31) / 32), dim3(256), 0, stream, partial, dW, n_slots, n_elems);
}

// workgroups (= partial-sum slots) of a launch over n_rows image rows
static int rows64_wgs(int n_rows, int* per_out) {
    int wgs = maed_opt(MAED_OPT_CONV3X3_ROWS_WGS);   // default 256, one per CU: every workgroup ends with a 147 KB partial result
    if (n_rows < 1 || wgs < 1) { *per_out = 0; return 0; }
    if (wgs > n_rows) wgs = n_rows;
    const int per = (n_rows + wgs - 1) / wgs;
    *per_out = per;
    return (n_rows + per - 1) / per;
}

// dW (64, 3, 3, 64) fp32 += weight gradient from dy, x (F, H, W, 64) channels_last bf16.  scratch (optional): maed_conv3x3_wgrad_rows64_scratch_floats(...) floats for
// the per-workgroup partial results (plain stores + one reduction pass); without it the workgroups add into dW with atomics.
int maed_conv3x3_wgrad_rows64_launch(const void* dy, const void* x, float* dW, void* scratch, int F, int H, int W, hipStream_t stream) {
    const int n_rows = F * H;
    int per = 0;
    const int wgs = rows64_wgs(n_rows, &per);
    if (wgs == 0) return MAED_OK;
    static bool attr_set = false;
    if (!attr_set) { (void)hipFuncSetAttribute((const void*)conv3x3_wgrad_rows64_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr_set = true; }
    hipLaunchKernelGGL(conv3x3_wgrad_rows64_kernel, dim3(wgs), dim3(R3_THREADS), R3_LDS_BYTES, stream, (const bf16*)dy, (const bf16*)x, dW, (float*)scratch, H, W, n_rows, per);
    if (scratch) maed_wgrad_slots_reduce((const float*)scratch, dW, wgs, 64 * 576, stream);
    MAED_CHECK_LAUNCH("conv3x3_wgrad(rows)");
    return MAED_OK;
}

extern "C" int maed_conv3x3_wgrad_rows64_scratch_floats(int F, int H, int W, int Cin, int Cout) {
    if (!maed_conv3x3_wgrad_rows64_ok(F, H, W, Cin, Cout)) return 0;
    int per = 0;
    return rows64_wgs(F * H, &per) * 64 * 576;
}

extern "C" int maed_conv3x3_wgrad_rows64(const void* dy, const void* x, float* dW, void* scratch, int F, int H, int W, int dtype, void* stream) {
    MAED_CHECK_ARG(dy && x && dW, MAED_ERR_ARG, "conv3x3_wgrad_rows64: null pointer");
    MAED_CHECK_ARG(dtype == MAED_BF16, MAED_ERR_UNSUPPORTED, "conv3x3_wgrad_rows64: bf16 only (dtype=%d)", dtype);
    MAED_CHECK_ARG(F > 0 && maed_conv3x3_wgrad_rows64_ok(F, H, W, 64, 64), MAED_ERR_SHAPE, "conv3x3_wgrad_rows64: needs W %% 8 == 0, 8 <= W <= 64 (F=%d H=%d W=%d)", F, H, W);
    MAED_CHECK_ARG(is_aligned(dy, 16) && is_aligned(x, 16) && is_aligned(scratch, 16), MAED_ERR_ALIGN, "conv3x3_wgrad_rows64: 16-B alignment");
    ProfScope prof__(PROF_TN_CONV, stream, 2.0 * (double)F * H * W * 64 * 576, 2.0 * (double)F * H * W * 128 + 36.0 * 64 * 64);
    return maed_conv3x3_wgrad_rows64_launch(dy, x, dW, scratch, F, H, W, (hipStream_t)stream);
}

// ---- Tap-resident weight gradient for channel counts that are multiples of 64 (the conv2 of the stage-2 / stage-3 bottlenecks: 128 -> 128 at 28 x 28, 256 -> 256 at
// 14 x 14, and the two stride-2 ones), MAED_OPT_CONV3X3_WGRAD_TAPS.  The row kernel above, generalised:
//   * a workgroup owns a 64 (co) x 9 (tap) x 64 (ci) block of dW (wave = tap, the same four 32 x 32 accumulators) -- grid.y walks the co x ci blocks, grid.x chunks
//     of work items; the 64-channel slice of a pixel is 128 contiguous bytes of the channels-last row, so the LDS images and the transposing reads stay as they are.
//   * a work item is R consecutive output rows of one frame as ONE linear run of pixel slots with pitch P: the dy image has P - Wo zero slots behind every row, the
//     x image is the matching window of input rows framed by zero pixels, and a tap is a constant slot offset (stride 1: P = W + 2, tap = ky P + kx;  stride 2:
//     P = Wo + 1, the input rows are split by row and column parity into four phase images of XP slots each, tap = ((ky & 1) 2 + (kx & 1)) XP + (ky >> 1) P +
//     (kx >> 1)).  K is the run in 16-slot steps.  Items never straddle a frame; rows above / below the image, a ragged last item and the tail of the last k-step are
//     zero slots like the borders.
//   * EVERY slot an item reads is written by that item's copies: each lane of a copy instruction picks its own 16-byte source -- a pixel chunk or the page of zeros --
//     so no row length has to fill a 64-lane instruction, nothing is zeroed up front, and no lane is predicated.  The lane -> (row, column) map does not depend on the
//     item and is computed once per lane.  Chunk c of slot s is stored at c ^ 4 ((s >> 1) & 1), as above.
//   * two or three stages of (dy image + x image); the copies of item g + 1 (g + 2) are issued right behind the barrier that frees the stage of item g - 1.
#define T9_THREADS 576
#define T9_MAXDY 4                        // copy instructions per wave and item for the dy image: 36 x 8 = 288 slots
#define T9_MAXX 8                         // ... for the x image(s): 576 slots
#define T9_MAX_SLOTS 1280                 // dy + x slots of all stages: 160 KB

struct TapsGeo {
    int H, W, Ho, Wo, Cin, Cout, s2, pt, pl;
    int R, ipf, n_items;                  // output rows per item, items per frame, items
    int P, ksteps, DS, XP, XS, nst;       // slot pitch, 16-slot steps, dy slots, slots per phase image (stride 2), x slots, stages
    int per, chunks, cib, cob;            // items per workgroup, grid.x, ci / co blocks
};

#define T9_WAIT(n_) switch (n_) { case 1: MAED_WAIT_VMCNT(1); break; case 2: MAED_WAIT_VMCNT(2); break; case 3: MAED_WAIT_VMCNT(3); break; case 4: MAED_WAIT_VMCNT(4); break; \
    case 5: MAED_WAIT_VMCNT(5); break; case 6: MAED_WAIT_VMCNT(6); break; case 7: MAED_WAIT_VMCNT(7); break; case 8: MAED_WAIT_VMCNT(8); break; case 9: MAED_WAIT_VMCNT(9); break; \
    case 10: MAED_WAIT_VMCNT(10); break; case 11: MAED_WAIT_VMCNT(11); break; case 12: MAED_WAIT_VMCNT(12); break; default: MAED_WAIT_VMCNT0(); }

__global__ __launch_bounds__(T9_THREADS, 1) void conv3x3_wgrad_taps_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ x, const bf16* __restrict__ zero,
                                                                             float* __restrict__ dW, float* __restrict__ partial, TapsGeo g) {
    MAED_DYN_SHARED(unsigned short, smem);
    const int tid = threadIdx.x, lane = tid & 63, tap = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, hi = lane >> 5, i16 = lane & 15;
    const int ky = tap / 3, kx = tap - 3 * ky;
    const int i0 = blockIdx.x * g.per;
    int i1 = i0 + g.per;
    if (i1 > g.n_items) i1 = g.n_items;
    if (i0 >= i1) return;
    const int cb = blockIdx.y / g.cib, ib = blockIdx.y - cb * g.cib;
    const int P = g.P, ndi = g.DS >> 3, nxi = g.XS >> 3, stage_elems = (g.DS + g.XS) * 64;

    // source of this lane's 16 bytes in copy instruction tap + 9 q of an item: row relative to the item's first row (1 << 20: a slot that is zero in every item) and
    // byte offset relative to that row's start; position (slot, chunk) = (8 j + (lane >> 3), lane & 7) of instruction j
    int dyrel[T9_MAXDY], dyrow[T9_MAXDY], xrel[T9_MAXX], xrow[T9_MAXX];
    int n_mine = 0;
#pragma unroll
    for (int q = 0; q < T9_MAXDY; ++q) {
        const int s = (tap + 9 * q) * 8 + (lane >> 3), r = s / P, c = s - r * P, ch = (lane & 7) ^ (((s >> 1) & 1) << 2);
        dyrow[q] = (c < g.Wo && r < g.R) ? r : (1 << 20);
        dyrel[q] = ((r * g.Wo + c) * g.Cout + cb * 64) * 2 + ch * 16;
        n_mine += (tap + 9 * q < ndi) ? 1 : 0;
    }
#pragma unroll
    for (int q = 0; q < T9_MAXX; ++q) {
        const int u = (tap + 9 * q) * 8 + (lane >> 3), ch = (lane & 7) ^ (((u >> 1) & 1) << 2);
        int ro, col;
        bool ok;
        if (!g.s2) { const int rr = u / P; ro = rr - 1; col = u - rr * P - 1; ok = rr < g.R + 2; }
        else { const int ph = u / g.XP, v = u - ph * g.XP, rr = v / P; ro = 2 * rr + (ph >> 1); col = 2 * (v - rr * P) + (ph & 1) - g.pl; ok = rr < g.R + 1; }
        xrow[q] = (ok && (unsigned)col < (unsigned)g.W) ? ro : (1 << 20);
        xrel[q] = ((ro * g.W + col) * g.Cin + ib * 64) * 2 + ch * 16;
        n_mine += (tap + 9 * q < nxi) ? 1 : 0;
    }
    n_mine = __builtin_amdgcn_readfirstlane(n_mine);
#define T9_ISSUE(it_, st_) { const int it__ = (it_), f__ = it__ / g.ipf, y0__ = (it__ - f__ * g.ipf) * g.R, yb__ = g.s2 ? 2 * y0__ - g.pt : y0__; \
        unsigned short* const sb__ = smem + (st_) * stage_elems; \
        const char* const dyb__ = (const char*)dy + ((int64_t)f__ * g.Ho + y0__) * g.Wo * g.Cout * 2; \
        const char* const xb__ = (const char*)x + ((int64_t)f__ * g.H + yb__) * g.W * g.Cin * 2; \
        _Pragma("unroll") for (int q = 0; q < T9_MAXDY; ++q) if (tap + 9 * q < ndi) { \
            const char* s__ = (unsigned)(y0__ + dyrow[q]) < (unsigned)g.Ho ? dyb__ + dyrel[q] : (const char*)zero; \
            MAED_LDS_DMA16_PTR(s__, sb__ + (tap + 9 * q) * 512); } \
        _Pragma("unroll") for (int q = 0; q < T9_MAXX; ++q) if (tap + 9 * q < nxi) { \
            const char* s__ = (unsigned)(yb__ + xrow[q]) < (unsigned)g.H ? xb__ + xrel[q] : (const char*)zero; \
            MAED_LDS_DMA16_PTR(s__, sb__ + g.DS * 64 + (tap + 9 * q) * 512); } }

    f32x16_t acc[2][2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][0][r] = 0.f; acc[0][1][r] = 0.f; acc[1][0][r] = 0.f; acc[1][1][r] = 0.f; }
    // transposing reads as in the row kernel; the x operand's slot is the dy slot + the tap's offset (bit 1 of a slot is unchanged by + 8 and + 16 s)
    const int toff = g.s2 ? ((ky & 1) * 2 + (kx & 1)) * g.XP + (ky >> 1) * P + (kx >> 1) : ky * P + kx;
    const int prow = 4 * hi + (i16 >> 2), pcol = (lane & 16) + 4 * (i16 & 3);
    const int swa = ((prow >> 1) & 1) << 2, swb = (((prow + toff) >> 1) & 1) << 2;
    const int a_off0 = prow * 64 + ((((pcol >> 3) ^ swa) << 3) | (pcol & 7)), a_off1 = prow * 64 + (((((pcol + 32) >> 3) ^ swa) << 3) | (pcol & 7));
    const int b_off0 = (prow + toff) * 64 + ((((pcol >> 3) ^ swb) << 3) | (pcol & 7)), b_off1 = (prow + toff) * 64 + (((((pcol + 32) >> 3) ^ swb) << 3) | (pcol & 7));

    const int ahead = g.nst - 1;                                          // items whose copies run ahead of the one in use: 1 or 2
    T9_ISSUE(i0, 0);
    if (ahead > 1 && i0 + 1 < i1) T9_ISSUE(i0 + 1, 1);
    int st = 0;                                                           // stage of item it
    for (int it = i0; it < i1; ++it) {
        // item it's copies are complete once only the younger item's (n_mine per wave, when it was issued) are outstanding
        if (ahead > 1 && it + 1 < i1) { T9_WAIT(n_mine) } else { MAED_WAIT_VMCNT0(); }
        __syncthreads();                 // item it's images have landed for every wave; nobody still reads item it - 1's stage
        if (it + ahead < i1) { int sn = st + ahead; if (sn >= g.nst) sn -= g.nst; T9_ISSUE(it + ahead, sn); }
        const unsigned short* da = smem + st * stage_elems;
        const unsigned short* xb = da + g.DS * 64;
        // two fragment sets: the reads of k-step s + 1 are issued before the MFMAs of k-step s (a wave shares its SIMD with at most two others: the LDS round trip
        // of a step read and multiplied in turn stayed exposed)
        union Frag { bf16x8_t v; uint2 u[2]; };
        Frag pa0, pa1, pb0, pb1, qa0, qa1, qb0, qb1;
#define T9_FRAG(dst_, base_, s_, off_) { auto lo__ = MAED_DS_READ_TR16((base_) + (s_) * 1024 + (off_)); auto hi__ = MAED_DS_READ_TR16((base_) + (s_) * 1024 + 512 + (off_)); \
            __builtin_memcpy(&dst_.u[0], &lo__, 8); __builtin_memcpy(&dst_.u[1], &hi__, 8); }
#define T9_LOAD(p_, s_) { T9_FRAG(p_##a0, da, s_, a_off0) T9_FRAG(p_##a1, da, s_, a_off1) T9_FRAG(p_##b0, xb, s_, b_off0) T9_FRAG(p_##b1, xb, s_, b_off1) }
#define T9_MFMA(p_) { acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p_##a0.v, p_##b0.v, acc[0][0], 0, 0, 0); \
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p_##a0.v, p_##b1.v, acc[0][1], 0, 0, 0); \
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p_##a1.v, p_##b0.v, acc[1][0], 0, 0, 0); \
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p_##a1.v, p_##b1.v, acc[1][1], 0, 0, 0); }
        T9_LOAD(p, 0)
        int s = 0;
        for (; s + 2 <= g.ksteps; s += 2) {
            T9_LOAD(q, s + 1)
            __builtin_amdgcn_sched_barrier(0);      // (hipcc sinks the reads below the MFMAs otherwise)
            T9_MFMA(p)
            __builtin_amdgcn_sched_barrier(0);
            { const int sn = s + 2 < g.ksteps ? s + 2 : s; T9_LOAD(p, sn) }      // (branch-free: past the end it reads a step again; a branch here lets hipcc sink the reads)
            __builtin_amdgcn_sched_barrier(0);
            T9_MFMA(q)
            __builtin_amdgcn_sched_barrier(0);
        }
        if (s < g.ksteps) T9_MFMA(p)
#undef T9_MFMA
#undef T9_LOAD
#undef T9_FRAG
        if (++st == g.nst) st = 0;
    }
#undef T9_ISSUE
    // D[co][ci] as in the row kernel; dW (Cout, 9, Cin).  With `partial` the workgroup stores its block with plain stores into the partial dW of its chunk
    // (grid.x of them, summed by wgrad_slots_reduce_kernel); without, it adds into dW with atomics.
    const size_t ld = (size_t)9 * g.Cin;
    float* const base = (partial ? partial + (size_t)blockIdx.x * g.Cout * ld : dW) + (size_t)cb * 64 * ld + tap * g.Cin + ib * 64;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int bt = 0; bt < 2; ++bt) {
            float* d = base + 32 * bt + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float* e = d + (size_t)(32 * a + (r & 3) + 8 * (r >> 2) + 4 * hi) * ld;
                if (partial) *e = acc[a][bt][r]; else atomicAdd(e, acc[a][bt][r]);
            }
        }
}

// geometry of a launch; false: the shape (or the option's value) leaves it to the general kernels
static bool taps_geo(int F, int H, int W, int Cin, int Cout, int stride, int pt, int pl, int Ho, int Wo, TapsGeo* out) {
    const int opt = maed_opt(MAED_OPT_CONV3X3_WGRAD_TAPS);
    if (opt <= 0 || F < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || Cin < 64 || Cout < 64 || Cin % 64 || Cout % 64) return false;
    if (stride == 1) { if (Ho != H || Wo != W || maed_conv3x3_wgrad_rows64_ok(F, H, W, Cin, Cout)) return false; }
    else if (stride == 2) { if (Ho != (H + 1) / 2 || Wo != (W + 1) / 2 || pt < 0 || pt > 1 || pl < 0 || pl > 1) return false; }
    else return false;
    if ((int64_t)H * W * Cin * 2 >= (1ll << 30) || (int64_t)Ho * Wo * Cout * 2 >= (1ll << 30) || (int64_t)Cout * 9 * Cin >= (1ll << 28)) return false;
    const int64_t M = (int64_t)F * Ho * Wo;
    if (opt == 1 && M < 4096 && M % 64 == 0) return false;               // small launches the general kernel can take stay there
    TapsGeo g{};
    g.H = H; g.W = W; g.Ho = Ho; g.Wo = Wo; g.Cin = Cin; g.Cout = Cout; g.s2 = stride == 2; g.pt = pt; g.pl = pl;
    g.P = g.s2 ? Wo + 1 : Wo + 2;
    // the most rows per item whose images fit the copy maps and two stages of LDS, then evened out over the frame
    int rmax = 0;
    for (int R = 1; R <= Ho; ++R) {
        const int DS = (R * g.P + 15) / 16 * 16, XP = (DS + g.P + 1 + 7) / 8 * 8, XS = g.s2 ? 4 * XP : (DS + 2 * g.P + 2 + 7) / 8 * 8;
        if (DS > T9_MAXDY * 72 || XS > T9_MAXX * 72 || 2 * (DS + XS) > T9_MAX_SLOTS) break;
        rmax = R;
    }
    if (rmax == 0) return false;
    g.ipf = (Ho + rmax - 1) / rmax;
    g.R = (Ho + g.ipf - 1) / g.ipf;
    g.ipf = (Ho + g.R - 1) / g.R;
    if ((int64_t)F * g.ipf >= (1ll << 30)) return false;
    g.n_items = F * g.ipf;
    g.DS = (g.R * g.P + 15) / 16 * 16; g.ksteps = g.DS / 16;
    g.XP = (g.DS + g.P + 1 + 7) / 8 * 8;
    g.XS = g.s2 ? 4 * g.XP : (g.DS + 2 * g.P + 2 + 7) / 8 * 8;
    g.nst = 3 * (g.DS + g.XS) <= T9_MAX_SLOTS ? 3 : 2;
    g.cib = Cin / 64; g.cob = Cout / 64;
    if ((int64_t)g.cib * g.cob > 65535) return false;
    // workgroups: one per CU when the launch has the GPU to itself; beside the main stream (the weight gradients' side stream) a quarter of them -- a workgroup holds
    // most of a CU's LDS and registers, so a full grid shuts the main stream's kernels out for the length of the launch: 256 workgroups measured no step-time gain
    // over the general kernel, 128 / 96 / 64 measured -0.11 / -0.23 / -0.29 ms per cfg3 step (profiles/conv3x3_wgrad_taps_ab.txt)
    const int wgs = maed_opt(MAED_OPT_SIDE_STREAM) ? 64 : 256;
    int chunks = opt > 2 ? opt - 2 : (wgs + g.cib * g.cob - 1) / (g.cib * g.cob);
    if (chunks > g.n_items) chunks = g.n_items;
    g.per = (g.n_items + chunks - 1) / chunks;
    g.chunks = (g.n_items + g.per - 1) / g.per;
    *out = g;
    return true;
}

bool maed_conv3x3_wgrad_taps_ok(int F, int H, int W, int Cin, int Cout, int stride, int pad_top, int pad_left, int Ho, int Wo) {
    TapsGeo g;
    return taps_geo(F, H, W, Cin, Cout, stride, pad_top, pad_left, Ho, Wo, &g);
}

int maed_conv3x3_wgrad_taps_launch(const void* dy, const void* x, const void* zero_page, float* dW, void* scratch, int F, int H, int W, int Cin, int Cout, int stride,
                                   int pad_top, int pad_left, int Ho, int Wo, hipStream_t stream) {
    TapsGeo g;
    if (!taps_geo(F, H, W, Cin, Cout, stride, pad_top, pad_left, Ho, Wo, &g)) { maed_set_error("conv3x3_wgrad_taps: shape not covered"); return MAED_ERR_SHAPE; }
    static bool attr_set = false;
    if (!attr_set) { (void)hipFuncSetAttribute((const void*)conv3x3_wgrad_taps_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr_set = true; }
    const size_t lds_bytes = (size_t)g.nst * (g.DS + g.XS) * 128;
    hipLaunchKernelGGL(conv3x3_wgrad_taps_kernel, dim3(g.chunks, g.cib * g.cob), dim3(T9_THREADS), lds_bytes, stream, (const bf16*)dy, (const bf16*)x,
                       (const bf16*)zero_page, dW, (float*)scratch, g);
    if (scratch) maed_wgrad_slots_reduce((const float*)scratch, dW, g.chunks, Cout * 9 * Cin, stream);
    MAED_CHECK_LAUNCH("conv3x3_wgrad(taps)");
    return MAED_OK;
}

extern "C" int maed_conv3x3_wgrad_taps_scratch_floats(int F, int H, int W, int Cin, int Cout, int stride, int Ho, int Wo) {
    TapsGeo g;
    if (!taps_geo(F, H, W, Cin, Cout, stride, 0, 0, Ho, Wo, &g)) return 0;
    const int64_t n = (int64_t)g.chunks * Cout * 9 * Cin;
    return n < (1ll << 31) ? (int)n : 0;
}

extern "C" int maed_conv3x3_wgrad_taps(const void* dy, const void* x, const void* zero_page, float* dW, void* scratch, int F, int H, int W, int Cin, int Cout,
                                       int stride, int pad_top, int pad_left, int Ho, int Wo, int dtype, void* stream) {
    MAED_CHECK_ARG(dy && x && zero_page && dW, MAED_ERR_ARG, "conv3x3_wgrad_taps: null pointer");
    MAED_CHECK_ARG(dtype == MAED_BF16, MAED_ERR_UNSUPPORTED, "conv3x3_wgrad_taps: bf16 only (dtype=%d)", dtype);
    MAED_CHECK_ARG(maed_conv3x3_wgrad_taps_ok(F, H, W, Cin, Cout, stride, pad_top, pad_left, Ho, Wo), MAED_ERR_SHAPE,
                   "conv3x3_wgrad_taps: shape not covered (F=%d H=%d W=%d Cin=%d Cout=%d stride=%d pads %d/%d Ho=%d Wo=%d, option %d)", F, H, W, Cin, Cout, stride,
                   pad_top, pad_left, Ho, Wo, maed_opt(MAED_OPT_CONV3X3_WGRAD_TAPS));
    MAED_CHECK_ARG(is_aligned(dy, 16) && is_aligned(x, 16) && is_aligned(zero_page, 16) && is_aligned(scratch, 16), MAED_ERR_ALIGN, "conv3x3_wgrad_taps: 16-B alignment");
    ProfScope prof__(PROF_TN_CONV, stream, 2.0 * (double)F * Ho * Wo * Cout * 9 * Cin, 2.0 * ((double)F * Ho * Wo * Cout + (double)F * H * W * Cin) + 36.0 * (double)Cout * Cin);
    return maed_conv3x3_wgrad_taps_launch(dy, x, zero_page, dW, scratch, F, H, W, Cin, Cout, stride, pad_top, pad_left, Ho, Wo, (hipStream_t)stream);
}
