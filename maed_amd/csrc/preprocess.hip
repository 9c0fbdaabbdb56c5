// Device-side clip preprocessing (reference: train.py:41-70 + lib/data_utils/transforms/{crop,color_jitter,random_erase,random_hflip,basic}.py):
// uint8 source regions + a small table of per-frame / per-clip parameters -> the normalised fp32 (F, 3, H, W) tensor MAED.forward takes.
//
//   crop       bilinear sample of the source at the inverse affine map (crop.py:88-92), zero outside, rounded to uint8
//   jitter     brightness / saturation / hue / contrast in the order the clip drew (color_jitter.py:55-97), uint8 in, uint8 out per operation (the
//              PIL arithmetic torchvision calls: ImageEnhance's blend, the C RGB <-> HSV rows)
//   erase      rows at the top / bottom set to zero (random_erase.py:23-87; `_erase_left` / `_erase_right` blank ROWS too)
//   flip       x -> W-1-x (random_hflip.py:113)
//   normalise  (u8 / 255 - mean) / std, three correctly rounded fp32 operations (basic.py:24-49, 95-108)
//
// Everything except the contrast step is a function of one pixel.  Contrast blends against the mean grey level of the WHOLE frame as it
// is at that point of the order, so a frame is processed in two stages around that reduction:
//   stage 1 = warp + the operations before contrast, grey level summed in integers (exact, order-free)
//   stage 2 = contrast + the operations after it + erase + flip + normalise
// and the three forms differ only in where the uint8 patch lives between the stages:
//   DIRECT  (no clip has a contrast step: evaluation, the 2D stream)  nowhere: both stages in registers, one launch, grid over pixel quads
//   TWO     (a clip has a contrast step; any patch size)             two launches through a uint8 scratch + one integer atomic per workgroup
//   LDS     (on request; 3*H*W bytes fit the 160 KB of a CU: 224 x 224) one workgroup per frame, patch in LDS, the sum is a workgroup reduction
// The same two device functions run in all three, so they agree bit for bit.  The LDS form was the first choice for 224 x 224 and measured SLOWER than the
// two-launch form (230 vs 103 us for 128 frames of the stage-2 config, profiles/preprocess_micro.txt: half the CUs idle, too few waves per gather), so form 0 never picks it.
//
// Layout of the staged patch: PLANAR uint8, a thread owns 4 consecutive pixels of a row (W % 4 == 0) = one dword per plane: LDS writes and
// reads are consecutive dwords across the lanes (no bank conflict, guide section on ds_read/ds_write_b32), a flipped quad is the mirrored dword with its
// bytes reversed, and the output is one float4 store per plane and lane (full 16-B stores, 1 KB contiguous per wave).  Rejected: interleaved RGB
// (3-byte pixels: byte-wide LDS operations, or a 12-byte repack per quad whose dwords mix channels and cannot be mirrored by a byte swap).
// The gathers from the source are 12 byte loads per pixel at arbitrary addresses: neighbouring lanes read neighbouring source pixels, so they
// hit the same cache lines; wider loads would need 3-byte-pixel realignment per tap and the kernel's floor is the fp32 write, not the gather.
#include "common.cuh"

// the uint8 arithmetic below restates C code that rounds after every operation: no fused multiply-add may replace a multiply and an add
#pragma clang fp contract(off)

namespace {

enum { OP_NONE = 0, OP_BRIGHTNESS = 1, OP_SATURATION = 2, OP_HUE = 3, OP_CONTRAST = 4 };
enum { FORM_AUTO = 0, FORM_DIRECT = 1, FORM_LDS = 2, FORM_TWO = 3 };
constexpr int PRE_LDS_BUDGET = 160 * 1024 - 512;      // dynamic LDS of the LDS form (the reduction cells are static)
constexpr int PRE_THREADS = 256;
#ifdef MAED_HOSTSIM
constexpr int PRE_LDS_THREADS = 128;                  // one host thread per lane: keep the simulated workgroup small
#else
constexpr int PRE_LDS_THREADS = 1024;                 // one workgroup per CU: 16 waves to hide the gather latency
#endif

struct Norm { float mean[3], stdv[3]; };

// per-frame view of the parameter tables (include/maed_hip.h maed_clip_preprocess)
struct FrameP {
    int off, h, w, pitch, erase_top, erase_bot;
    float m[6];
    int flip, ops, hue_shift, pos_c;                  // ops: four 4-bit operation codes, first one lowest (no indexed private array: that would live in scratch memory); pos_c: index of the contrast step, 4 if there is none
    float f_brightness, f_saturation, f_contrast;
};

__device__ inline FrameP load_frame(const int* __restrict__ frame_i, const float* __restrict__ frame_minv, const int* __restrict__ clip_i,
                                    const float* __restrict__ clip_f, int f, int N) {
    FrameP p;
    const int* fi = frame_i + (size_t)f * 8;
    p.off = fi[0]; p.h = fi[1]; p.w = fi[2]; p.pitch = fi[3];
    int c = fi[4];
    c = c < 0 ? 0 : c >= N ? N - 1 : c;               // (the host validates; a bad index must still stay inside the tables)
    p.erase_top = fi[5]; p.erase_bot = fi[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) p.m[i] = frame_minv[(size_t)f * 6 + i];
    const int* ci = clip_i + (size_t)c * 8;
    p.flip = ci[0];
    p.pos_c = 4;
    p.ops = 0;
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        const int op = ci[1 + i] & 15;
        p.ops |= op << (4 * i);
        if (op == OP_CONTRAST) p.pos_c = i;           // (descending: the first one wins; the host lists each operation once)
    }
    p.hue_shift = ci[5] & 255;
    p.f_brightness = clip_f[(size_t)c * 4 + 0];
    p.f_saturation = clip_f[(size_t)c * 4 + 1];
    p.f_contrast = clip_f[(size_t)c * 4 + 3];
    return p;
}

// ---- the uint8 pixel operations ---------------------------------------------------------------------------------------------
// ITU-R 601-2 luma as PIL's RGB -> L conversion computes it
__device__ __forceinline__ int grey_level(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// PIL's Image.blend(degenerate, image, f): degenerate + f * (x - degenerate) in fp32, clipped, truncated
__device__ __forceinline__ int blend_u8(int a, float f, int x) {
    const float t = (float)a + f * (float)(x - a);
    return t <= 0.f ? 0 : t >= 255.f ? 255 : (int)t;
}

// hue shift: RGB -> HSV, H += shift (mod 256), HSV -> RGB, with the rounding of PIL's C rows (which follow colorsys.py): float
// quotients, the h / 6 + 1 fold and the scaling to 0..255 in double, truncation on the way in, round-half-away on the way out
__device__ inline void hue_shift_u8(int& r, int& g, int& b, int shift) {
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int uh = 0, us = 0;
    const int uv = maxc;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        float h;
        if (r == maxc) h = bc - gc;
        else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
        uh = min(255, max(0, (int)((double)h * 255.0)));
        us = min(255, max(0, (int)((double)s * 255.0)));
    }
    uh = (uh + shift) & 255;
    if (us == 0) { r = g = b = uv; return; }
    const double h6 = (double)(float)uh * 6.0 / 255.0;
    const int i = (int)floor(h6);
    const float f = (float)(h6 - (double)(float)i);
    const float fs = (float)((double)(float)us / 255.0);
    const float v = (float)uv;
    const int p = min(255, max(0, (int)round((double)v * (1.0 - (double)fs))));
    const int q = min(255, max(0, (int)round((double)v * (1.0 - (double)fs * (double)f))));
    const int t = min(255, max(0, (int)round((double)v * (1.0 - (double)fs * (1.0 - (double)f)))));
    switch (i % 6) {
        case 0: r = uv; g = t; b = p; break;
        case 1: r = q; g = uv; b = p; break;
        case 2: r = p; g = uv; b = t; break;
        case 3: r = p; g = q; b = uv; break;
        case 4: r = t; g = p; b = uv; break;
        default: r = uv; g = p; b = q; break;
    }
}

// operations ops[from .. to) on one pixel; `mean_grey` is read by the contrast step only
__device__ inline void apply_ops(const FrameP& p, int from, int to, int mean_grey, int& r, int& g, int& b) {
    for (int i = from; i < to; ++i) {
        const int op = (p.ops >> (4 * i)) & 15;
        if (op == OP_BRIGHTNESS) {
            const float f = p.f_brightness;
            r = blend_u8(0, f, r); g = blend_u8(0, f, g); b = blend_u8(0, f, b);
        } else if (op == OP_SATURATION) {
            const float f = p.f_saturation;
            const int l = grey_level(r, g, b);
            r = blend_u8(l, f, r); g = blend_u8(l, f, g); b = blend_u8(l, f, b);
        } else if (op == OP_HUE) {
            hue_shift_u8(r, g, b, p.hue_shift);
        } else if (op == OP_CONTRAST) {
            const float f = p.f_contrast;
            r = blend_u8(mean_grey, f, r); g = blend_u8(mean_grey, f, g); b = blend_u8(mean_grey, f, b);
        }
    }
}

// ---- the warp ---------------------------------------------------------------------------------------------------------------
// one source tap: zero outside the region; the address is also held inside the packed buffer whatever the tables say
__device__ __forceinline__ void tap(const uint8_t* __restrict__ src, int64_t src_bytes, const FrameP& p, int x, int y, float wgt, float (&acc)[3]) {
    if ((unsigned)x >= (unsigned)p.w || (unsigned)y >= (unsigned)p.h) return;
    const int64_t a = (int64_t)p.off + (int64_t)y * p.pitch + (int64_t)x * 3;
    if (a < 0 || a + 3 > src_bytes) return;
    acc[0] += wgt * (float)src[a];
    acc[1] += wgt * (float)src[a + 1];
    acc[2] += wgt * (float)src[a + 2];
}

__device__ inline void warp_pixel(const uint8_t* __restrict__ src, int64_t src_bytes, const FrameP& p, int x, int y, int& r, int& g, int& b) {
    float sx = p.m[0] * (float)x + p.m[1] * (float)y + p.m[2];
    float sy = p.m[3] * (float)x + p.m[4] * (float)y + p.m[5];
    sx = fminf(fmaxf(sx, -2.f), (float)p.w + 1.f);      // (also maps a NaN coordinate to a finite one: every tap then lies outside)
    sy = fminf(fmaxf(sy, -2.f), (float)p.h + 1.f);
    const float fx = floorf(sx), fy = floorf(sy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float ax = sx - fx, ay = sy - fy;
    float acc[3] = {0.f, 0.f, 0.f};
    tap(src, src_bytes, p, x0, y0, (1.f - ax) * (1.f - ay), acc);
    tap(src, src_bytes, p, x0 + 1, y0, ax * (1.f - ay), acc);
    tap(src, src_bytes, p, x0, y0 + 1, (1.f - ax) * ay, acc);
    tap(src, src_bytes, p, x0 + 1, y0 + 1, ax * ay, acc);
    r = min(255, max(0, (int)rintf(acc[0])));
    g = min(255, max(0, (int)rintf(acc[1])));
    b = min(255, max(0, (int)rintf(acc[2])));
}

// ---- the two stages on a quad of pixels --------------------------------------------------------------------------------------
// stage 1 on patch pixels (x .. x+3, y): three dwords (one per plane, pixel x in the low byte); returns the quad's grey sum at the contrast step
__device__ inline int stage1_quad(const uint8_t* __restrict__ src, int64_t src_bytes, const FrameP& p, int x, int y, uint32_t (&planes)[3]) {
    int grey = 0;
    planes[0] = planes[1] = planes[2] = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int r, g, b;
        warp_pixel(src, src_bytes, p, x + k, y, r, g, b);
        apply_ops(p, 0, p.pos_c, 0, r, g, b);
        if (p.pos_c < 4) grey += grey_level(r, g, b);
        planes[0] |= (uint32_t)r << (8 * k);
        planes[1] |= (uint32_t)g << (8 * k);
        planes[2] |= (uint32_t)b << (8 * k);
    }
    return grey;
}

// PIL: int(ImageStat.Stat(grey).mean[0] + 0.5), the mean a double quotient of two integers
__device__ __forceinline__ int mean_grey_of(unsigned sum, int npix) { return (int)((double)sum / (double)npix + 0.5); }

// stage 2 for OUTPUT pixels (xo .. xo+3, y): `planes` hold the patch pixels that land there (the mirrored quad when the clip is flipped)
__device__ inline void stage2_store(const FrameP& p, const Norm& nm, int xo, int y, int H, int W, const uint32_t (&planes)[3], int mean_grey,
                                    float* __restrict__ out_frame) {
    const bool erased = y < p.erase_top || y >= H - p.erase_bot;
    float o[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int sh = 8 * (p.flip ? 3 - k : k);
        int r = (planes[0] >> sh) & 255, g = (planes[1] >> sh) & 255, b = (planes[2] >> sh) & 255;
        apply_ops(p, p.pos_c, 4, mean_grey, r, g, b);
        if (erased) r = g = b = 0;
        o[0][k] = ((float)r / 255.0f - nm.mean[0]) / nm.stdv[0];
        o[1][k] = ((float)g / 255.0f - nm.mean[1]) / nm.stdv[1];
        o[2][k] = ((float)b / 255.0f - nm.mean[2]) / nm.stdv[2];
    }
    const size_t plane = (size_t)H * W, at = (size_t)y * W + xo;
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(out_frame + c * plane + at) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over the workgroup, returned to every thread (every thread of the workgroup calls this)
__device__ inline unsigned block_sum(int v) {
    __shared__ unsigned cells[17];
    v = wave_sum_i(v);
    const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();                                   // (a previous use of the cells is over)
    if ((threadIdx.x & 63) == 0) cells[wave] = (unsigned)v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned s = 0;
        for (int w = 0; w < nw; ++w) s += cells[w];
        cells[16] = s;
    }
    __syncthreads();
    return cells[16];
}

// ---- DIRECT: no contrast step anywhere; grid (quads / PRE_THREADS, F) ----------------------------------------------------------
__global__ __launch_bounds__(PRE_THREADS) void preprocess_direct_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int* __restrict__ frame_i,
                                                                        const float* __restrict__ frame_minv, const int* __restrict__ clip_i,
                                                                        const float* __restrict__ clip_f, int N, int H, int W, Norm nm, float* __restrict__ out) {
    const int f = blockIdx.y, q = blockIdx.x * PRE_THREADS + threadIdx.x, wq = W >> 2;
    if (q >= H * wq) return;
    const FrameP p = load_frame(frame_i, frame_minv, clip_i, clip_f, f, N);
    const int y = q / wq, xo = (q - y * wq) * 4;
    uint32_t planes[3];
    stage1_quad(src, src_bytes, p, p.flip ? W - 4 - xo : xo, y, planes);
    stage2_store(p, nm, xo, y, H, W, planes, 0, out + (size_t)f * 3 * H * W);
}

// ---- LDS: one workgroup per frame, the uint8 patch (3 planes) in dynamic LDS --------------------------------------------------
__global__ __launch_bounds__(PRE_LDS_THREADS) void preprocess_lds_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int* __restrict__ frame_i,
                                                                         const float* __restrict__ frame_minv, const int* __restrict__ clip_i,
                                                                         const float* __restrict__ clip_f, int N, int H, int W, Norm nm, float* __restrict__ out) {
    MAED_DYN_SHARED(uint32_t, patch);                  // [3][H * W / 4]
    const int f = blockIdx.x, wq = W >> 2, nq = H * wq;
    const FrameP p = load_frame(frame_i, frame_minv, clip_i, clip_f, f, N);
    int grey = 0;
    for (int q = threadIdx.x; q < nq; q += blockDim.x) {
        const int y = q / wq, x = (q - y * wq) * 4;
        uint32_t planes[3];
        grey += stage1_quad(src, src_bytes, p, x, y, planes);
        patch[q] = planes[0]; patch[nq + q] = planes[1]; patch[2 * nq + q] = planes[2];
    }
    int mean_grey = 0;
    if (p.pos_c < 4) mean_grey = mean_grey_of(block_sum(grey), H * W);      // (its barriers order the patch writes before the reads below)
    else __syncthreads();
    float* out_frame = out + (size_t)f * 3 * H * W;
    for (int q = threadIdx.x; q < nq; q += blockDim.x) {
        const int y = q / wq, xq = q - y * wq;
        const int qs = p.flip ? y * wq + (wq - 1 - xq) : q;
        const uint32_t planes[3] = {patch[qs], patch[nq + qs], patch[2 * nq + qs]};
        stage2_store(p, nm, xq * 4, y, H, W, planes, mean_grey, out_frame);
    }
}

// ---- TWO: stage 1 into a uint8 scratch (F, 3, H*W) + grey sums (F), then stage 2; both on grid (quads / PRE_THREADS, F) -----------
__global__ __launch_bounds__(PRE_THREADS) void preprocess_stage1_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int* __restrict__ frame_i,
                                                                        const float* __restrict__ frame_minv, const int* __restrict__ clip_i,
                                                                        const float* __restrict__ clip_f, int N, int H, int W, uint32_t* __restrict__ scratch,
                                                                        unsigned* __restrict__ sums) {
    const int f = blockIdx.y, q = blockIdx.x * PRE_THREADS + threadIdx.x, wq = W >> 2, nq = H * wq;
    const FrameP p = load_frame(frame_i, frame_minv, clip_i, clip_f, f, N);
    int grey = 0;
    if (q < nq) {
        const int y = q / wq, x = (q - y * wq) * 4;
        uint32_t planes[3];
        grey = stage1_quad(src, src_bytes, p, x, y, planes);
        uint32_t* s = scratch + (size_t)f * 3 * nq;
        s[q] = planes[0]; s[nq + q] = planes[1]; s[2 * nq + q] = planes[2];
    }
    if (p.pos_c < 4) {                                 // (uniform over the workgroup: one frame, one clip)
        const unsigned s = block_sum(grey);
        if (threadIdx.x == 0) atomicAdd(sums + f, s);
    }
}

__global__ __launch_bounds__(PRE_THREADS) void preprocess_stage2_kernel(const int* __restrict__ frame_i, const float* __restrict__ frame_minv,
                                                                        const int* __restrict__ clip_i, const float* __restrict__ clip_f, int N, int H, int W,
                                                                        Norm nm, const uint32_t* __restrict__ scratch, const unsigned* __restrict__ sums,
                                                                        float* __restrict__ out) {
    const int f = blockIdx.y, q = blockIdx.x * PRE_THREADS + threadIdx.x, wq = W >> 2, nq = H * wq;
    if (q >= nq) return;
    const FrameP p = load_frame(frame_i, frame_minv, clip_i, clip_f, f, N);
    const int mean_grey = p.pos_c < 4 ? mean_grey_of(sums[f], H * W) : 0;
    const int y = q / wq, xq = q - y * wq;
    const int qs = p.flip ? y * wq + (wq - 1 - xq) : q;
    const uint32_t* s = scratch + (size_t)f * 3 * nq;
    const uint32_t planes[3] = {s[qs], s[nq + qs], s[2 * nq + qs]};
    stage2_store(p, nm, xq * 4, y, H, W, planes, mean_grey, out + (size_t)f * 3 * H * W);
}

inline size_t sums_bytes(int F) { return ((size_t)F * 4 + 255) / 256 * 256; }

}  // namespace

extern "C" size_t maed_clip_preprocess_workspace(int F, int H, int W) {
    if (F <= 0 || H <= 0 || W <= 0) return 0;
    return sums_bytes(F) + (size_t)F * 3 * H * W;
}

extern "C" int maed_clip_preprocess(const uint8_t* src, int64_t src_bytes, const int32_t* frame_i, const float* frame_minv, const int32_t* clip_i,
                                    const float* clip_f, int F, int N, int H, int W, const float* norm_host, int has_contrast, int form, float* out,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    MAED_CHECK_ARG(src && frame_i && frame_minv && clip_i && clip_f && norm_host && out, MAED_ERR_ARG, "clip_preprocess: null pointer");
    MAED_CHECK_ARG(F >= 0 && N > 0 && H > 0 && W > 0 && src_bytes > 0, MAED_ERR_SHAPE, "clip_preprocess: bad extents");
    MAED_CHECK_ARG(F <= 65535, MAED_ERR_SHAPE, "clip_preprocess: %d frames in one call (the frame index is a 16-bit grid dimension: at most 65535)", F);
    MAED_CHECK_ARG(W % 4 == 0, MAED_ERR_SHAPE, "clip_preprocess: patch width %d is not a multiple of 4", W);
    MAED_CHECK_ARG(src_bytes < ((int64_t)1 << 31) && (int64_t)H * W < ((int64_t)1 << 24), MAED_ERR_SHAPE, "clip_preprocess: 32-bit source offsets / 24-bit pixel counts exceeded");
    MAED_CHECK_ARG(is_aligned(out, 16), MAED_ERR_ALIGN, "clip_preprocess: out must be 16-byte aligned");
    MAED_CHECK_ARG(form >= FORM_AUTO && form <= FORM_TWO, MAED_ERR_ARG, "clip_preprocess: form %d", form);
    for (int c = 0; c < 3; ++c) MAED_CHECK_ARG(norm_host[3 + c] != 0.f, MAED_ERR_ARG, "clip_preprocess: zero std");
    if (F == 0) return MAED_OK;
    const size_t patch_bytes = (size_t)3 * H * W;
    const bool fits = patch_bytes <= (size_t)PRE_LDS_BUDGET;
    // measured (profiles/preprocess_micro.txt, 128 frames, stage-2 config): two-launch 103 us against 230 us for the LDS form at 224 x 224 -- 128 workgroups leave half
    // of the 256 CUs idle and the gathers of one frame wait on 16 waves only, which costs more than the 39 MB of uint8 scratch traffic saves; the LDS form stays
    // selectable (form 2) and bit-identical
    if (form == FORM_AUTO) form = has_contrast ? FORM_TWO : FORM_DIRECT;
    MAED_CHECK_ARG(!(form == FORM_DIRECT && has_contrast), MAED_ERR_UNSUPPORTED, "clip_preprocess: the direct form has no whole-frame reduction (a clip has a contrast step)");
    MAED_CHECK_ARG(!(form == FORM_LDS && !fits), MAED_ERR_UNSUPPORTED, "clip_preprocess: a %d x %d patch (%zu B) does not fit the LDS form", H, W, patch_bytes);
    Norm nm;
    for (int c = 0; c < 3; ++c) { nm.mean[c] = norm_host[c]; nm.stdv[c] = norm_host[3 + c]; }
    const int nq = H * (W / 4);
    const dim3 grid((nq + PRE_THREADS - 1) / PRE_THREADS, F);
    hipStream_t st = (hipStream_t)stream;
    if (form == FORM_DIRECT) {
        hipLaunchKernelGGL(preprocess_direct_kernel, grid, dim3(PRE_THREADS), 0, st, src, src_bytes, frame_i, frame_minv, clip_i, clip_f, N, H, W, nm, out);
    } else if (form == FORM_LDS) {
        static bool attr_set = false;
        if (!attr_set) { (void)hipFuncSetAttribute((const void*)preprocess_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PRE_LDS_BUDGET); attr_set = true; }
        hipLaunchKernelGGL(preprocess_lds_kernel, dim3(F), dim3(PRE_LDS_THREADS), patch_bytes, st, src, src_bytes, frame_i, frame_minv, clip_i, clip_f, N, H, W, nm, out);
    } else {
        MAED_CHECK_ARG(workspace && workspace_bytes >= maed_clip_preprocess_workspace(F, H, W), MAED_ERR_ARG,
                       "clip_preprocess: the two-launch form needs %zu bytes of workspace", maed_clip_preprocess_workspace(F, H, W));
        MAED_CHECK_ARG(is_aligned(workspace, 16), MAED_ERR_ALIGN, "clip_preprocess: workspace must be 16-byte aligned");
        unsigned* sums = (unsigned*)workspace;
        uint32_t* scratch = (uint32_t*)((char*)workspace + sums_bytes(F));
        MAED_HIP(hipMemsetAsync(sums, 0, sums_bytes(F), st), "clip_preprocess");
        hipLaunchKernelGGL(preprocess_stage1_kernel, grid, dim3(PRE_THREADS), 0, st, src, src_bytes, frame_i, frame_minv, clip_i, clip_f, N, H, W, scratch, sums);
        hipLaunchKernelGGL(preprocess_stage2_kernel, grid, dim3(PRE_THREADS), 0, st, frame_i, frame_minv, clip_i, clip_f, N, H, W, nm, (const uint32_t*)scratch,
                           (const unsigned*)sums, out);
    }
    MAED_CHECK_LAUNCH("clip_preprocess");
    return MAED_OK;
}
