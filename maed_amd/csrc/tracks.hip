// Video inference, the step between a person tracker and the model (reference: lib/utils/smooth_bbox.py:11-123, lib/data_utils/threedpw_utils.py:103-108,
// lib/data_utils/transforms/crop.py:57-92; definitions in docs/design/17_video_inference.md):
//
//   maed_track_boxes   K keypoint tracks -> smoothed crop boxes: per-frame (cx, cy, scale) from the visible keypoints' rectangle, linear fill of the frames without
//                      one, median filter (zeros outside the series), Gaussian filter (edge sample repeated outside), box = 150 / scale * box_scale.  fp64 throughout.
//   maed_crop_tables   boxes + (box, frame) indices -> the parameter tables of maed_clip_preprocess for whole frames that lie on the device, so that the pixels go
//                      through the existing preprocessing kernels.
//
// One workgroup per track, one launch for all tracks.  The three series live in two buffers of 3 x cap doubles that the four phases ping-pong between:
//   raw -> A,  fill A -> B,  median B -> A,  Gaussian A -> outputs
// cap = TRK_LDS_N and the buffers are LDS for a track of at most TRK_LDS_N frames; a longer track takes its 6 x L doubles of the caller's workspace instead (same
// code, same results; the waves of a workgroup share the CU's vector cache, so the workgroup barrier between the phases orders those accesses as it orders LDS).
// No private arrays: the median is taken by rank counting over the window as it lies in the buffer, the Gaussian weights lie in LDS.
#include "common.cuh"
#include <limits.h>
#include <math.h>

// parity with numpy / scipy is a statement about rounding: every product and sum below is rounded on its own, as theirs are
#pragma clang fp contract(off)

namespace {

constexpr int TRK_LDS_N = 1024;                        // frames of a track that stay in LDS: 6 x 1024 x 8 B = 48 KB of the 64 KB static limit
constexpr int TRK_MAX_R = 512;                         // Gaussian radius: 513 weights = 4 KB
constexpr int TRK_MAX_L = 1 << 24;
constexpr int TRK_MAX_J = 64;
#ifdef MAED_HOSTSIM
constexpr int TRK_THREADS = 64;                        // one host thread per lane: keep the simulated workgroup small
#else
constexpr int TRK_THREADS = 256;
#endif
constexpr double TRK_INVALID = -1.0;                   // scale of a frame without a box (a real scale is positive, or NaN from NaN keypoints)

struct TrackArgs {
    const float* kps;                                  // keypoints, or
    const double* series;                              // (K, L, 3) parameters that are already complete: phases 1 and 2 are a copy, the span is (0, length)
    const int* lengths;
    int L, J, ksize, r;
    double vis_thresh, sigma, box_scale;
    float* boxes;
    double* params;
    int* span;
    double* ws;
};

// rows [lo, hi) of a track's outputs = 0
__device__ inline void zero_rows(const TrackArgs& a, int k, int lo, int hi) {
    for (int i = lo + (int)threadIdx.x; i < hi; i += (int)blockDim.x) {
        const size_t row = (size_t)k * a.L + i;
        a.boxes[row * 4 + 0] = 0.f; a.boxes[row * 4 + 1] = 0.f; a.boxes[row * 4 + 2] = 0.f; a.boxes[row * 4 + 3] = 0.f;
        if (a.params) { a.params[row * 3 + 0] = 0.0; a.params[row * 3 + 1] = 0.0; a.params[row * 3 + 2] = 0.0; }
    }
}

// one track on buffers A, B of 3 x cap doubles each (series s at [s * cap]); wgt: normalised Gaussian weights 0..r in LDS; cell_a / cell_b: TRK_THREADS ints each
__device__ __forceinline__ void track_series(const TrackArgs& a, int k, int len, double* A, double* B, int cap, const double* wgt, int* cell_a, int* cell_b,
                                             int* span_lds) {
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    // ---- phase 1: raw parameters of every frame (smooth_bbox.py:38-61) and the first / last frame that has them ----
    if (a.series) {                                                  // (uniform over the grid)
        const double* x = a.series + (size_t)k * a.L * 3;
        for (int i = tid; i < len; i += nt) { B[i] = x[3 * i]; B[cap + i] = x[3 * i + 1]; B[2 * cap + i] = x[3 * i + 2]; }
        if (tid == 0) { span_lds[0] = len > 0 ? 0 : -1; span_lds[1] = len; }
        __syncthreads();
    } else {
        const float* kp = a.kps + (size_t)k * a.L * a.J * 3;
        int first = INT_MAX, last = -1;
        for (int i = tid; i < len; i += nt) {
            const float* p = kp + (size_t)i * a.J * 3;
            double x0 = 0.0, x1 = 0.0, y0 = 0.0, y1 = 0.0;
            bool any = false;
            for (int j = 0; j < a.J; ++j) {
                if (!((double)p[3 * j + 2] > a.vis_thresh)) continue;
                const double x = (double)p[3 * j], y = (double)p[3 * j + 1];
                if (!any) { x0 = x1 = x; y0 = y1 = y; any = true; }
                else { x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1; y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1; }
            }
            const double dx = x1 - x0, dy = y1 - y0;
            const double height = sqrt(dx * dx + dy * dy);
            const bool valid = any && !(height < 0.5);
            A[i] = (x0 + x1) / 2.0;
            A[cap + i] = (y0 + y1) / 2.0;
            A[2 * cap + i] = valid ? 150.0 / height : TRK_INVALID;
            if (valid) { first = i < first ? i : first; last = i; }
        }
        cell_a[tid] = first; cell_b[tid] = last;
        __syncthreads();
        if (tid == 0) {
            for (int t = 0; t < nt; ++t) { first = cell_a[t] < first ? cell_a[t] : first; last = cell_b[t] > last ? cell_b[t] : last; }
            span_lds[0] = last < 0 ? -1 : first;
            span_lds[1] = last + 1;
            a.span[2 * k] = span_lds[0]; a.span[2 * k + 1] = span_lds[1];
        }
        __syncthreads();
    }
    const int start = span_lds[0], end = span_lds[1];
    if (start < 0) { zero_rows(a, k, 0, a.L); return; }              // (uniform over the workgroup) no frame has a box: the one case the reference raises on
    const int m = end - start;
    // ---- phase 2: frames without a box, linearly between their nearest neighbours that have one (smooth_bbox.py:94-102, numpy.linspace's arithmetic) ----
    if (!a.series) {
        // a thread owns `chunk` consecutive frames; what lies before / behind its chunk it learns from the other threads' cells
        const int chunk = (m + nt - 1) / nt;
        const int lo = start + (tid * chunk < m ? tid * chunk : m), hi = (lo + chunk < end) ? lo + chunk : end;
        int first = INT_MAX, last = -1;
        for (int i = lo; i < hi; ++i)
            if (A[2 * cap + i] != TRK_INVALID) { first = i < first ? i : first; last = i; }
        __syncthreads();                                             // (thread 0 is done reading the cells of phase 1)
        cell_a[tid] = first; cell_b[tid] = last;
        __syncthreads();
        int p = -1, q_out = -1;
        for (int t = tid - 1; t >= 0 && p < 0; --t) p = cell_b[t];
        for (int t = tid + 1; t < nt && q_out < 0; ++t) q_out = cell_a[t] == INT_MAX ? -1 : cell_a[t];
        int q = -1;
        for (int i = lo; i < hi; ++i) {
            if (A[2 * cap + i] != TRK_INVALID) {
                B[i] = A[i]; B[cap + i] = A[cap + i]; B[2 * cap + i] = A[2 * cap + i];
                p = i;
                continue;
            }
            if (q < i) {
                for (q = i + 1; q < hi && A[2 * cap + q] == TRK_INVALID; ++q) { }
                if (q >= hi) q = q_out;
            }
            if (p < 0 || q < 0) continue;                            // (cannot happen inside the span: its first and last frame have a box)
            const double di = (double)(i - p), dq = (double)(q - p);
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const double xp = A[s * cap + p], xq = A[s * cap + q];
                B[s * cap + i] = di * ((xq - xp) / dq) + xp;
            }
        }
        __syncthreads();
    }
    // ---- phase 3: median filter, zeros outside the series (scipy.signal.medfilt; smooth_bbox.py:121-122) ----
    {
        const int h = a.ksize >> 1;
        for (int e = tid; e < 3 * m; e += nt) {
            const int s = e / m, u = e - s * m;
            const double* x = B + s * cap + start;
            double med = NAN;                                        // (a window that holds a NaN has no element of the wanted rank)
            for (int c = -h; c <= h; ++c) {
                const int tc = u + c;
                const double vc = (tc < 0 || tc >= m) ? 0.0 : x[tc];
                int below = 0;
                for (int d = -h; d <= h; ++d) {
                    const int td = u + d;
                    const double vd = (td < 0 || td >= m) ? 0.0 : x[td];
                    below += (vd < vc || (vd == vc && d < c)) ? 1 : 0;
                }
                if (below == h) { med = vc; break; }
            }
            A[s * cap + start + u] = med;
        }
        __syncthreads();
    }
    // ---- phase 4: Gaussian filter, the edge sample repeated outside (scipy.ndimage reflect; smooth_bbox.py:123), and the outputs ----
    {
        const int r = a.r, m2 = 2 * m;
        for (int u = tid; u < m; u += nt) {
            double v[3];
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const double* x = A + s * cap + start;
                double acc = 0.0;
                if (u - r >= 0 && u + r < m) {
                    for (int j = -r; j <= r; ++j) acc += wgt[j < 0 ? -j : j] * x[u + j];
                } else {
                    for (int j = -r; j <= r; ++j) {
                        int t = (u + j) % m2;
                        t = t < 0 ? t + m2 : t;
                        t = t >= m ? m2 - 1 - t : t;
                        acc += wgt[j < 0 ? -j : j] * x[t];
                    }
                }
                v[s] = acc;
            }
            const size_t row = (size_t)k * a.L + start + u;
            if (a.params) { a.params[row * 3 + 0] = v[0]; a.params[row * 3 + 1] = v[1]; a.params[row * 3 + 2] = v[2]; }
            const float side = (float)(150.0 / v[2] * a.box_scale);  // (threedpw_utils.py:103-108; a smoothed scale of 0 gives infinity, as the reference's division does)
            a.boxes[row * 4 + 0] = (float)v[0]; a.boxes[row * 4 + 1] = (float)v[1]; a.boxes[row * 4 + 2] = side; a.boxes[row * 4 + 3] = side;
        }
    }
    zero_rows(a, k, 0, start);
    zero_rows(a, k, end, a.L);
}

__global__ __launch_bounds__(TRK_THREADS) void track_boxes_kernel(TrackArgs a) {
    __shared__ double series[6 * TRK_LDS_N];
    __shared__ double wgt[TRK_MAX_R + 1];
    __shared__ double wsum;
    __shared__ int cell_a[TRK_THREADS], cell_b[TRK_THREADS], span_lds[2];
    const int k = (int)blockIdx.x, tid = (int)threadIdx.x;
    // normalised weights exp(-0.5 / sigma^2 * j^2) / sum (scipy.ndimage._gaussian_kernel1d)
    const double c = -0.5 / (a.sigma * a.sigma);
    for (int j = tid; j <= a.r; j += (int)blockDim.x) wgt[j] = exp(c * (double)(j * j));
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int j = -a.r; j <= a.r; ++j) s += wgt[j < 0 ? -j : j];
        wsum = s;
    }
    __syncthreads();
    const double total = wsum;
    __syncthreads();                                                 // (every thread has read the sum before the weights change)
    for (int j = tid; j <= a.r; j += (int)blockDim.x) wgt[j] = wgt[j] / total;
    __syncthreads();
    int len = a.lengths[k];
    len = len < 0 ? 0 : len > a.L ? a.L : len;
    if (len <= TRK_LDS_N) {
        track_series(a, k, len, series, series + 3 * TRK_LDS_N, TRK_LDS_N, wgt, cell_a, cell_b, span_lds);
    } else {
        double* A = a.ws + (size_t)k * 6 * a.L;                      // (the host checked that L > TRK_LDS_N comes with a workspace)
        track_series(a, k, len, A, A + (size_t)3 * a.L, a.L, wgt, cell_a, cell_b, span_lds);
    }
}

__global__ __launch_bounds__(256) void crop_tables_kernel(const float* __restrict__ boxes, int n_boxes, const int* __restrict__ box_index,
                                                          const int* __restrict__ frame_index, int M, int T, int n_frames, int img_h, int img_w, int H, int W,
                                                          int* __restrict__ frame_i, float* __restrict__ frame_minv, int* __restrict__ clip_i,
                                                          float* __restrict__ clip_f) {
    const int m = (int)(blockIdx.x * 256 + threadIdx.x);
    if (m >= M) return;
    const int n_clips = (M + T - 1) / T;
    if (m < n_clips) {
        for (int i = 0; i < 8; ++i) clip_i[(size_t)m * 8 + i] = 0;
        for (int i = 0; i < 4; ++i) clip_f[(size_t)m * 4 + i] = 0.f;
    }
    const int b = box_index[m];
    int f = frame_index[m];
    bool ok = b >= 0 && b < n_boxes && f >= 0 && f < n_frames;       // (the host cannot see the index tables: an index outside them reads nothing and gives a black patch)
    f = ok ? f : 0;
    double cx = 0.0, cy = 0.0, w = 0.0, h = 0.0;
    if (ok) {
        const float* bx = boxes + (size_t)b * 4;
        cx = (double)bx[0]; cy = (double)bx[1]; w = (double)bx[2]; h = (double)bx[3];
        ok = isfinite(cx) && isfinite(cy) && isfinite(w) && isfinite(h) && w > 0.0 && h > 0.0;
    }
    int* fi = frame_i + (size_t)m * 8;
    fi[0] = f * img_h * img_w * 3; fi[1] = img_h; fi[2] = img_w; fi[3] = 3 * img_w; fi[4] = m / T; fi[5] = 0; fi[6] = 0; fi[7] = 0;
    float* mv = frame_minv + (size_t)m * 6;
    if (ok) {
        // patch -> frame: the inverse of crop.py:57-86's map without rotation, scale jitter or shift
        mv[0] = (float)(w / (double)W); mv[1] = 0.f; mv[2] = (float)(cx - w / 2.0);
        mv[3] = 0.f; mv[4] = (float)(h / (double)H); mv[5] = (float)(cy - h / 2.0);
    } else {
        mv[0] = 0.f; mv[1] = 0.f; mv[2] = -2.f;                      // every patch pixel samples at (-2, -2): all four taps lie outside, the patch is black
        mv[3] = 0.f; mv[4] = 0.f; mv[5] = -2.f;
    }
}

}  // namespace

extern "C" size_t maed_track_boxes_workspace(int K, int L) {
    if (K <= 0 || L <= TRK_LDS_N) return 0;
    return (size_t)K * 6 * (size_t)L * sizeof(double);
}

static int track_launch(const char* who, const float* kps, const double* series, const int32_t* lengths, int K, int L, int J, double vis_thresh, int kernel_size,
                        double sigma, double box_scale, float* boxes, double* params, int32_t* span, void* workspace, size_t workspace_bytes, void* stream) {
    MAED_CHECK_ARG((kps || series) && lengths && boxes && (span || series), MAED_ERR_ARG, "%s: null pointer", who);
    MAED_CHECK_ARG(K >= 0 && L >= 1, MAED_ERR_SHAPE, "%s: bad extents K=%d L=%d", who, K, L);
    MAED_CHECK_ARG(L <= TRK_MAX_L, MAED_ERR_SHAPE, "%s: %d frames per track (at most 2^24)", who, L);
    MAED_CHECK_ARG(J >= 1 && J <= TRK_MAX_J, MAED_ERR_SHAPE, "%s: %d keypoints per frame (1 .. 64)", who, J);
    MAED_CHECK_ARG(kernel_size >= 1 && kernel_size <= 63 && (kernel_size & 1), MAED_ERR_ARG, "%s: kernel_size %d (the median window must be odd, 1 .. 63)", who, kernel_size);
    MAED_CHECK_ARG(sigma > 0.0 && sigma <= 1e6, MAED_ERR_ARG, "%s: sigma %g (must be > 0)", who, sigma);
    const int r = (int)(4.0 * sigma + 0.5);
    MAED_CHECK_ARG(r <= TRK_MAX_R, MAED_ERR_ARG, "%s: sigma %g gives a Gaussian radius of %d samples (at most 512)", who, sigma, r);
    MAED_CHECK_ARG((!params || is_aligned(params, 8)) && (!series || is_aligned(series, 8)), MAED_ERR_ALIGN, "%s: fp64 arrays must be 8-byte aligned", who);
    if (K == 0) return MAED_OK;
    const size_t need = maed_track_boxes_workspace(K, L);
    MAED_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need), MAED_ERR_ARG, "%s: tracks of %d frames (more than %d) need %zu bytes of workspace", who, L,
                   TRK_LDS_N, need);
    MAED_CHECK_ARG(need == 0 || is_aligned(workspace, 8), MAED_ERR_ALIGN, "%s: workspace must be 8-byte aligned", who);
    TrackArgs a;
    a.kps = kps; a.series = series; a.lengths = lengths; a.L = L; a.J = J; a.ksize = kernel_size; a.r = r;
    a.vis_thresh = vis_thresh; a.sigma = sigma; a.box_scale = box_scale;
    a.boxes = boxes; a.params = params; a.span = span; a.ws = need ? (double*)workspace : nullptr;
    hipLaunchKernelGGL(track_boxes_kernel, dim3(K), dim3(TRK_THREADS), 0, (hipStream_t)stream, a);
    MAED_CHECK_LAUNCH(who);
    return MAED_OK;
}

extern "C" int maed_track_boxes(const float* kps, const int32_t* lengths, int K, int L, int J, double vis_thresh, int kernel_size, double sigma, double box_scale,
                                float* boxes, double* params, int32_t* span, void* workspace, size_t workspace_bytes, void* stream) {
    MAED_CHECK_ARG(kps && span, MAED_ERR_ARG, "track_boxes: null pointer");
    return track_launch("track_boxes", kps, nullptr, lengths, K, L, J, vis_thresh, kernel_size, sigma, box_scale, boxes, params, span, workspace, workspace_bytes, stream);
}

extern "C" int maed_track_smooth(const double* series, const int32_t* lengths, int K, int L, int kernel_size, double sigma, double box_scale, float* boxes,
                                 double* params, void* workspace, size_t workspace_bytes, void* stream) {
    MAED_CHECK_ARG(series, MAED_ERR_ARG, "track_smooth: null pointer");
    return track_launch("track_smooth", nullptr, series, lengths, K, L, 1, 0.0, kernel_size, sigma, box_scale, boxes, params, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int maed_crop_tables(const float* boxes, int n_boxes, const int32_t* box_index, const int32_t* frame_index, int M, int T, int n_frames, int img_h,
                                int img_w, int H, int W, int32_t* frame_i, float* frame_minv, int32_t* clip_i, float* clip_f, void* stream) {
    MAED_CHECK_ARG(boxes && box_index && frame_index && frame_i && frame_minv && clip_i && clip_f, MAED_ERR_ARG, "crop_tables: null pointer");
    MAED_CHECK_ARG(M >= 0 && T >= 1 && n_boxes >= 1 && n_frames >= 1 && img_h >= 1 && img_w >= 1 && H >= 1 && W >= 1, MAED_ERR_SHAPE, "crop_tables: bad extents");
    MAED_CHECK_ARG(M <= 65535, MAED_ERR_SHAPE, "crop_tables: %d crops in one call (maed_clip_preprocess takes at most 65535 frames)", M);
    MAED_CHECK_ARG(W % 4 == 0, MAED_ERR_SHAPE, "crop_tables: patch width %d is not a multiple of 4", W);
    MAED_CHECK_ARG((int64_t)n_frames * img_h * img_w * 3 < ((int64_t)1 << 31), MAED_ERR_SHAPE,
                   "crop_tables: %d frames of %d x %d are %lld bytes (the 32-bit offsets of maed_clip_preprocess need less than 2^31: pass fewer frames per call)", n_frames,
                   img_h, img_w, (long long)((int64_t)n_frames * img_h * img_w * 3));
    if (M == 0) return MAED_OK;
    hipLaunchKernelGGL(crop_tables_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, boxes, n_boxes, box_index, frame_index, M, T, n_frames, img_h,
                       img_w, H, W, frame_i, frame_minv, clip_i, clip_f);
    MAED_CHECK_LAUNCH("crop_tables");
    return MAED_OK;
}
