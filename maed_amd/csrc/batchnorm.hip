// BatchNorm2d, MaxPool2d(3, 2, padding 1) and the global average pool of the stage-1 encoder (MAED(encoder='cnn'): a torchvision-layout ResNet-50,
// reference lib/models/maed.py:35-37) on channels_last activations: a tensor is a row-major (M = N*H*W rows, C) matrix in bf16 or fp32, C % 8 == 0.
//
// All of these are streaming / reduction passes bound by HBM.  Structure shared by the statistics pass and the backward reduction:
//   * a lane owns 16 bytes of a row (8 bf16 or 4 fp32 channels; 8 channels in both dtypes where it also owns a byte of the 1-bit ReLU mask),
//     a workgroup of 256 lanes covers min(C / vec, 256) lane-columns x 256 / that many rows per step and walks a CHUNK of rows,
//   * per-lane sums run in fp32 over four rows at a time (four independent 16-byte loads in flight) and are folded into fp64 accumulators,
//   * the row lanes of a workgroup are folded through LDS in a fixed order and the workgroup writes its fp64 partials with plain stores into
//     caller scratch (chunks, C, 2); a second small kernel adds the chunks in a fixed order.  No atomics anywhere: results are bit-identical
//     from run to run, and the finalize step takes (sum, sum of squares, count), so a cross-rank reduction of the partials can be put in front of it.
#include "common.cuh"
#include <math.h>

namespace {

constexpr int BN_NT = 256;            // lanes per workgroup
constexpr int BN_TARGET_WGS = 1024;   // row chunks a large tensor is striped over (4 workgroups per CU)
constexpr int BN_MIN_ROWS = 32;       // ... but no chunk shorter than this

struct bn_geom { int cbn, CG, ntile, rstep, rpc, chunks; };

static int bn_rows_per_chunk(int64_t M) {
    int64_t rpc = (M + BN_TARGET_WGS - 1) / BN_TARGET_WGS;
    return (int)(rpc < BN_MIN_ROWS ? BN_MIN_ROWS : rpc);
}

static int bn_chunks(int64_t M) {
    if (M <= 0) return 0;
    const int rpc = bn_rows_per_chunk(M);
    return (int)((M + rpc - 1) / rpc);
}

static bn_geom bn_geometry(int64_t M, int C, int vec) {
    bn_geom g;
    g.cbn = C / vec;
    g.CG = g.cbn < BN_NT ? g.cbn : BN_NT;
    g.ntile = (g.cbn + g.CG - 1) / g.CG;
    g.rstep = BN_NT / g.CG;
    g.rpc = bn_rows_per_chunk(M);
    g.chunks = bn_chunks(M);
    return g;
}

template <int VEC, typename T> __device__ __forceinline__ void ldv(const T* p, float (&o)[VEC]) {
    if constexpr (VEC == 8) ld8(p, o); else ld4(p, o);
}
template <int VEC, typename T> __device__ __forceinline__ void stv(T* p, const float (&o)[VEC]) {
    if constexpr (VEC == 8) st8(p, o); else st4(p, o);
}

// low part of the mean (mean = hi + lo, two floats): NULL = zero (eval mode: the mean is the fp32 running buffer itself)
template <int VEC> __device__ __forceinline__ void bn_load_lo(const float* __restrict__ mean_lo, int cg, float (&ml)[VEC]) {
    if (mean_lo) { ldv<VEC>(mean_lo + cg * VEC, ml); return; }
#pragma unroll
    for (int j = 0; j < VEC; ++j) ml[j] = 0.f;
}

// position of a lane in the (row chunk, lane-column tile) grid
struct bn_lane { int cgl, rsub, cg, CG, rstep, r0, r1; bool active; };
template <int VEC> __device__ __forceinline__ bn_lane bn_where(int M, int C, int rpc) {
    bn_lane l;
    const int cbn = C / VEC;
    l.CG = min(cbn, BN_NT);
    l.rstep = BN_NT / l.CG;
    l.cgl = (int)threadIdx.x % l.CG;
    l.rsub = (int)threadIdx.x / l.CG;
    l.cg = (int)blockIdx.y * l.CG + l.cgl;
    l.active = l.rsub < l.rstep && l.cg < cbn;
    l.r0 = (int)min((int64_t)blockIdx.x * rpc, (int64_t)M);
    l.r1 = (int)min((int64_t)l.r0 + rpc, (int64_t)M);
    return l;
}

// fold the row lanes of a workgroup (fixed order: row lane 0, 1, 2, ...) and store (sum, sum2) of this chunk: part_row = partials + chunk * C * 2
template <int VEC>
__device__ __forceinline__ void bn_fold_store(const double (&s)[VEC], const double (&q)[VEC], double* __restrict__ part_row, const bn_lane& l) {
    __shared__ double fold[2 * VEC][BN_NT];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { fold[j][threadIdx.x] = s[j]; fold[VEC + j][threadIdx.x] = q[j]; }
    __syncthreads();
    if (l.active && l.rsub == 0) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            double ts = fold[j][l.cgl], tq = fold[VEC + j][l.cgl];
            for (int k = 1; k < l.rstep; ++k) { ts += fold[j][k * l.CG + l.cgl]; tq += fold[VEC + j][k * l.CG + l.cgl]; }
            double* o = part_row + ((int64_t)l.cg * VEC + j) * 2;
            o[0] = ts; o[1] = tq;
        }
    }
}

// ---- statistics: partials[chunk][c] = (sum x, sum x^2) over the rows of the chunk ----------------------------------------------------------------------
template <typename T, int VEC>
__global__ __launch_bounds__(BN_NT) void bn_stats_kernel(const T* __restrict__ x, double* __restrict__ part, int M, int C, int rpc) {
    const bn_lane l = bn_where<VEC>(M, C, rpc);
    double s[VEC], q[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { s[j] = 0.0; q[j] = 0.0; }
    if (l.active) {
        const T* px = x + (int64_t)l.cg * VEC;
        int r = l.r0 + l.rsub;
        for (; r + 3 * l.rstep < l.r1; r += 4 * l.rstep) {
            float v0[VEC], v1[VEC], v2[VEC], v3[VEC];
            ldv<VEC>(px + (int64_t)r * C, v0);
            ldv<VEC>(px + (int64_t)(r + l.rstep) * C, v1);
            ldv<VEC>(px + (int64_t)(r + 2 * l.rstep) * C, v2);
            ldv<VEC>(px + (int64_t)(r + 3 * l.rstep) * C, v3);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                s[j] += (double)((v0[j] + v1[j]) + (v2[j] + v3[j]));
                q[j] += (double)(fmaf(v0[j], v0[j], v1[j] * v1[j]) + fmaf(v2[j], v2[j], v3[j] * v3[j]));
            }
        }
        for (; r < l.r1; r += l.rstep) {
            float v[VEC];
            ldv<VEC>(px + (int64_t)r * C, v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) { s[j] += (double)v[j]; q[j] += (double)v[j] * (double)v[j]; }
        }
    }
    bn_fold_store<VEC>(s, q, part + (int64_t)blockIdx.x * C * 2, l);
}

// 16 channels x 16 chunk lanes per workgroup: lane k adds chunks k, k + 16, ... in order, then the 16 lane totals are added in order
__device__ __forceinline__ bool bn_combine(const double* __restrict__ part, int chunks, int C, int& c, double& s, double& q) {
    __shared__ double f[2][16][16];
    const int cl = threadIdx.x & 15, lane = threadIdx.x >> 4;
    c = blockIdx.x * 16 + cl;
    double ts = 0.0, tq = 0.0;
    if (c < C)
        for (int k = lane; k < chunks; k += 16) { ts += part[((int64_t)k * C + c) * 2]; tq += part[((int64_t)k * C + c) * 2 + 1]; }
    f[0][lane][cl] = ts; f[1][lane][cl] = tq;
    __syncthreads();
    if (lane != 0 || c >= C) return false;
    s = f[0][0][cl]; q = f[1][0][cl];
    for (int k = 1; k < 16; ++k) { s += f[0][k][cl]; q += f[1][k][cl]; }
    return true;
}

__global__ __launch_bounds__(BN_NT) void bn_finalize_kernel(const double* __restrict__ part, int chunks, int C, double count, float eps, float* __restrict__ mean,
                                                            float* __restrict__ mean_lo, float* __restrict__ rstd, float* __restrict__ rmean, float* __restrict__ rvar,
                                                            float momentum) {
    int c; double s, q;
    if (!bn_combine(part, chunks, C, c, s, q)) return;
    const double m = s / count;
    double var = q / count - m * m;          // biased
    if (var < 0.0) var = 0.0;
    mean[c] = (float)m;
    if (mean_lo) mean_lo[c] = (float)(m - (double)(float)m);     // the backward's x - mean cancels where a channel is almost constant: it subtracts both parts
    rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (rmean) rmean[c] = (float)((1.0 - (double)momentum) * (double)rmean[c] + (double)momentum * m);
    if (rvar) {
        const double unbiased = count > 1.0 ? var * (count / (count - 1.0)) : var;
        rvar[c] = (float)((1.0 - (double)momentum) * (double)rvar[c] + (double)momentum * unbiased);
    }
}

// sums[c] = (sum dy', sum dy' xhat) for the apply pass; dgamma / dbeta accumulate
__global__ __launch_bounds__(BN_NT) void bn_bwd_finalize_kernel(const double* __restrict__ part, int chunks, int C, float* __restrict__ sums,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta) {
    int c; double s, q;
    if (!bn_combine(part, chunks, C, c, s, q)) return;
    if (sums) { sums[2 * c] = (float)s; sums[2 * c + 1] = (float)q; }
    if (dbeta) dbeta[c] += (float)s;
    if (dgamma) dgamma[c] += (float)q;
}

// ---- forward apply: y = act(x * a + b [+ residual]), a = rstd * gamma, b = beta - mean * a ------------------------------------------------------------
// MASK (VEC == 8 only): write bit j of byte (row, c / 8) = (output channel 8 * (c / 8) + j > 0), the layout of maed_groupnorm_fwd's relu_mask
template <typename T, int VEC, bool RES, bool RELU, bool MASK>
__global__ __launch_bounds__(BN_NT) void bn_apply_kernel(const T* __restrict__ x, const T* __restrict__ res, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, T* __restrict__ y, uint8_t* __restrict__ mask,
                                                         int M, int C, int rpc) {
    const bn_lane l = bn_where<VEC>(M, C, rpc);
    if (!l.active) return;
    float a[VEC], b[VEC];
    {
        float mu[VEC], rs[VEC], gg[VEC], bb[VEC];
        ldv<VEC>(mean + l.cg * VEC, mu); ldv<VEC>(rstd + l.cg * VEC, rs); ldv<VEC>(gamma + l.cg * VEC, gg); ldv<VEC>(beta + l.cg * VEC, bb);
#pragma unroll
        for (int j = 0; j < VEC; ++j) { a[j] = rs[j] * gg[j]; b[j] = fmaf(-mu[j], a[j], bb[j]); }
    }
    const int64_t col = (int64_t)l.cg * VEC;
    // one row: from the loaded x (and residual) to the stored y (and mask byte)
    auto finish = [&](int r, const float (&v)[VEC], const float (&rr)[VEC]) {
        float o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = fmaf(v[j], a[j], b[j]);
        if (RES) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) o[j] += rr[j];
        }
        if (RELU) {
            if (MASK) {
                uint32_t bits = 0;
#pragma unroll
                for (int j = 0; j < VEC; ++j) bits |= (o[j] > 0.f ? 1u : 0u) << j;
                mask[(int64_t)r * (C / 8) + l.cg] = (uint8_t)bits;
            }
#pragma unroll
            for (int j = 0; j < VEC; ++j) o[j] = fmaxf(o[j], 0.f);
        }
        stv<VEC>(y + (int64_t)r * C + col, o);
    };
    int r = l.r0 + l.rsub;
    for (; r + 3 * l.rstep < l.r1; r += 4 * l.rstep) {       // four rows per step: all loads are issued before the first dependent store
        float v[4][VEC], rr[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            ldv<VEC>(x + (int64_t)(r + u * l.rstep) * C + col, v[u]);
            if (RES) ldv<VEC>(res + (int64_t)(r + u * l.rstep) * C + col, rr[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) finish(r + u * l.rstep, v[u], rr[u]);
    }
    for (; r < l.r1; r += l.rstep) {
        float v[VEC], rr[VEC];
        ldv<VEC>(x + (int64_t)r * C + col, v);
        if (RES) ldv<VEC>(res + (int64_t)r * C + col, rr);
        finish(r, v, rr);
    }
}

// dy' of one row for one lane: dy masked by the ReLU decision.  MODE 0: no ReLU; 1: recomputed from x exactly as the forward computed it (no residual was added);
// 2: the forward's bit mask (VEC == 8)
template <typename T, int VEC, int MODE>
__device__ __forceinline__ void bn_dy_eff(const T* __restrict__ x, const T* __restrict__ dy, const uint8_t* __restrict__ mask, int64_t r, int C, int cg, const float (&a)[VEC],
                                          const float (&b)[VEC], float (&v)[VEC], float (&d)[VEC]) {
    const int64_t at = r * C + (int64_t)cg * VEC;
    ldv<VEC>(x + at, v);
    ldv<VEC>(dy + at, d);
    if (MODE == 1) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) d[j] = fmaf(v[j], a[j], b[j]) > 0.f ? d[j] : 0.f;
    } else if (MODE == 2) {
        const uint32_t bits = mask[r * (C / 8) + cg];
#pragma unroll
        for (int j = 0; j < VEC; ++j) d[j] = ((bits >> j) & 1u) ? d[j] : 0.f;
    }
}

template <typename T, int VEC, int MODE>
__global__ __launch_bounds__(BN_NT) void bn_bwd_reduce_kernel(const T* __restrict__ x, const T* __restrict__ dy, const uint8_t* __restrict__ mask, const float* __restrict__ mean,
                                                              const float* __restrict__ mean_lo, const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              double* __restrict__ part, int M, int C, int rpc) {
    const bn_lane l = bn_where<VEC>(M, C, rpc);
    double s[VEC], q[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { s[j] = 0.0; q[j] = 0.0; }
    if (l.active) {
        float mu[VEC], ml[VEC], rs[VEC], a[VEC], b[VEC];
        {
            float gg[VEC], bb[VEC];
            bn_load_lo<VEC>(mean_lo, l.cg, ml);
            ldv<VEC>(mean + l.cg * VEC, mu); ldv<VEC>(rstd + l.cg * VEC, rs); ldv<VEC>(gamma + l.cg * VEC, gg); ldv<VEC>(beta + l.cg * VEC, bb);
#pragma unroll
            for (int j = 0; j < VEC; ++j) { a[j] = rs[j] * gg[j]; b[j] = fmaf(-mu[j], a[j], bb[j]); }
        }
        int r = l.r0 + l.rsub;
        for (; r + 3 * l.rstep < l.r1; r += 4 * l.rstep) {
            float v[4][VEC], d[4][VEC];
#pragma unroll
            for (int u = 0; u < 4; ++u) bn_dy_eff<T, VEC, MODE>(x, dy, mask, (int64_t)r + u * l.rstep, C, l.cg, a, b, v[u], d[u]);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                float ts = 0.f, tq = 0.f;
#pragma unroll
                for (int u = 0; u < 4; ++u) { ts += d[u][j]; tq = fmaf(d[u][j], ((v[u][j] - mu[j]) - ml[j]) * rs[j], tq); }
                s[j] += (double)ts; q[j] += (double)tq;
            }
        }
        for (; r < l.r1; r += l.rstep) {
            float v[VEC], d[VEC];
            bn_dy_eff<T, VEC, MODE>(x, dy, mask, (int64_t)r, C, l.cg, a, b, v, d);
#pragma unroll
            for (int j = 0; j < VEC; ++j) { s[j] += (double)d[j]; q[j] += (double)(d[j] * (((v[j] - mu[j]) - ml[j]) * rs[j])); }
        }
    }
    bn_fold_store<VEC>(s, q, part + (int64_t)blockIdx.x * C * 2, l);
}

// dx = gamma rstd (dy' - sum(dy') / M - xhat sum(dy' xhat) / M); FROZEN (eval-mode statistics): dx = dy' gamma rstd; dres = dy'
template <typename T, int VEC, int MODE, bool FROZEN>
__global__ __launch_bounds__(BN_NT) void bn_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ dy, const uint8_t* __restrict__ mask, const float* __restrict__ mean,
                                                             const float* __restrict__ mean_lo, const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ sums, T* __restrict__ dx, T* __restrict__ dres, int M, int C, int rpc) {
    const bn_lane l = bn_where<VEC>(M, C, rpc);
    if (!l.active) return;
    float mu[VEC], ml[VEC], rs[VEC], a[VEC], b[VEC], c1[VEC], c2[VEC];
    {
        float gg[VEC], bb[VEC];
        bn_load_lo<VEC>(mean_lo, l.cg, ml);
        ldv<VEC>(mean + l.cg * VEC, mu); ldv<VEC>(rstd + l.cg * VEC, rs); ldv<VEC>(gamma + l.cg * VEC, gg); ldv<VEC>(beta + l.cg * VEC, bb);
        const float inv = 1.0f / (float)M;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            a[j] = rs[j] * gg[j]; b[j] = fmaf(-mu[j], a[j], bb[j]);
            c1[j] = FROZEN ? 0.f : sums[2 * (l.cg * VEC + j)] * inv;
            c2[j] = FROZEN ? 0.f : sums[2 * (l.cg * VEC + j) + 1] * inv;
        }
    }
    const int64_t col = (int64_t)l.cg * VEC;
    auto finish = [&](int r, const float (&v)[VEC], const float (&d)[VEC]) {
        float o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = FROZEN ? d[j] * a[j] : a[j] * ((d[j] - c1[j]) - ((v[j] - mu[j]) - ml[j]) * rs[j] * c2[j]);
        stv<VEC>(dx + (int64_t)r * C + col, o);
        if (dres) stv<VEC>(dres + (int64_t)r * C + col, d);
    };
    int r = l.r0 + l.rsub;
    for (; r + 3 * l.rstep < l.r1; r += 4 * l.rstep) {       // four rows per step: all loads are issued before the first dependent store
        float v[4][VEC], d[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; ++u) bn_dy_eff<T, VEC, MODE>(x, dy, mask, (int64_t)r + u * l.rstep, C, l.cg, a, b, v[u], d[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) finish(r + u * l.rstep, v[u], d[u]);
    }
    for (; r < l.r1; r += l.rstep) {
        float v[VEC], d[VEC];
        bn_dy_eff<T, VEC, MODE>(x, dy, mask, (int64_t)r, C, l.cg, a, b, v, d);
        finish(r, v, d);
    }
}

// ---- statistics over the batch of all ranks (maed_batchnorm_*_local / *_dev) ---------------------------------------------------------------------------------
// Between the reduction and its consumer sits an all-reduce(SUM) of an fp64 record the host issues: forward record = (sum x, sum x^2) per channel followed by the
// row count (2 C + 1 doubles; ranks may hold different numbers of rows, so the global count is device data and never visits the host), backward record =
// (sum dy', sum dy' xhat) per channel (2 C doubles).  The chunk partials are added in bn_combine's order and the consumers repeat bn_finalize_kernel's /
// bn_bwd_apply_kernel's arithmetic, so a record that was not reduced (one rank) gives the bits of the one-rank entry points.
__global__ __launch_bounds__(BN_NT) void bn_record_kernel(const double* __restrict__ part, int chunks, int C, double* __restrict__ rec, double count,
                                                          float* __restrict__ dgamma, float* __restrict__ dbeta) {
    int c; double s, q;
    if (!bn_combine(part, chunks, C, c, s, q)) return;
    rec[2 * c] = s; rec[2 * c + 1] = q;
    if (count > 0.0 && c == 0) rec[2 * (int64_t)C] = count;     // forward record only
    if (dbeta) dbeta[c] += (float)s;
    if (dgamma) dgamma[c] += (float)q;
}

__global__ __launch_bounds__(BN_NT) void bn_finalize_dev_kernel(const double* __restrict__ rec, int C, float eps, float* __restrict__ mean, float* __restrict__ mean_lo,
                                                                float* __restrict__ rstd, float* __restrict__ rmean, float* __restrict__ rvar, float momentum) {
    const int c = (int)blockIdx.x * BN_NT + (int)threadIdx.x;
    if (c >= C) return;
    const double s = rec[2 * c], q = rec[2 * c + 1], count = rec[2 * (int64_t)C];
    const double m = s / count;
    double var = q / count - m * m;          // biased
    if (var < 0.0) var = 0.0;
    mean[c] = (float)m;
    if (mean_lo) mean_lo[c] = (float)(m - (double)(float)m);
    rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (rmean) rmean[c] = (float)((1.0 - (double)momentum) * (double)rmean[c] + (double)momentum * m);
    if (rvar) {
        const double unbiased = count > 1.0 ? var * (count / (count - 1.0)) : var;
        rvar[c] = (float)((1.0 - (double)momentum) * (double)rvar[c] + (double)momentum * unbiased);
    }
}

// bn_bwd_apply_kernel (not FROZEN) with the sums and the row count read from the reduced records
template <typename T, int VEC, int MODE>
__global__ __launch_bounds__(BN_NT) void bn_bwd_apply_dev_kernel(const T* __restrict__ x, const T* __restrict__ dy, const uint8_t* __restrict__ mask, const float* __restrict__ mean,
                                                                 const float* __restrict__ mean_lo, const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, const double* __restrict__ sums, const double* __restrict__ count,
                                                                 T* __restrict__ dx, T* __restrict__ dres, int M, int C, int rpc) {
    const bn_lane l = bn_where<VEC>(M, C, rpc);
    if (!l.active) return;
    float mu[VEC], ml[VEC], rs[VEC], a[VEC], b[VEC], c1[VEC], c2[VEC];
    {
        float gg[VEC], bb[VEC];
        bn_load_lo<VEC>(mean_lo, l.cg, ml);
        ldv<VEC>(mean + l.cg * VEC, mu); ldv<VEC>(rstd + l.cg * VEC, rs); ldv<VEC>(gamma + l.cg * VEC, gg); ldv<VEC>(beta + l.cg * VEC, bb);
        const float inv = 1.0f / (float)count[0];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            a[j] = rs[j] * gg[j]; b[j] = fmaf(-mu[j], a[j], bb[j]);
            c1[j] = (float)sums[2 * (l.cg * VEC + j)] * inv;
            c2[j] = (float)sums[2 * (l.cg * VEC + j) + 1] * inv;
        }
    }
    const int64_t col = (int64_t)l.cg * VEC;
    auto finish = [&](int r, const float (&v)[VEC], const float (&d)[VEC]) {
        float o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = a[j] * ((d[j] - c1[j]) - ((v[j] - mu[j]) - ml[j]) * rs[j] * c2[j]);
        stv<VEC>(dx + (int64_t)r * C + col, o);
        if (dres) stv<VEC>(dres + (int64_t)r * C + col, d);
    };
    int r = l.r0 + l.rsub;
    for (; r + 3 * l.rstep < l.r1; r += 4 * l.rstep) {
        float v[4][VEC], d[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; ++u) bn_dy_eff<T, VEC, MODE>(x, dy, mask, (int64_t)r + u * l.rstep, C, l.cg, a, b, v[u], d[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) finish(r + u * l.rstep, v[u], d[u]);
    }
    for (; r < l.r1; r += l.rstep) {
        float v[VEC], d[VEC];
        bn_dy_eff<T, VEC, MODE>(x, dy, mask, (int64_t)r, C, l.cg, a, b, v, d);
        finish(r, v, d);
    }
}

// ---- MaxPool2d(kernel 3, stride 2, padding 1) ------------------------------------------------------------------------------------------------------------
// The structure of maed_maxpool3s2_same_* (backbone.hip) with symmetric padding: windows start at 2 * o - 1, Ho = (H - 1) / 2 + 1.  Ties / NaN follow ATen: the
// first strictly greater value in (kh, kw) scan order wins, a NaN always wins.  A window always holds its centre tap (kh = kw = 1 is inside the image).
template <typename T>
__global__ __launch_bounds__(256) void maxpool_p1_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ idx, int N, int H, int W, int C, int Ho, int Wo) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;          // one thread: 8 channels of one output pixel
    const int cb = C / 8;
    if (i >= (int64_t)N * Ho * Wo * cb) return;
    const int c8 = (int)(i % cb) * 8;
    const int64_t pix = i / cb;
    const int wo = (int)(pix % Wo), ho = (int)((pix / Wo) % Ho), n = (int)(pix / ((int64_t)Wo * Ho));
    float m[8]; int am[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { m[j] = -INFINITY; am[j] = 0; }
    bool first = true;
    for (int kh = 0; kh < 3; ++kh) {
        const int h = 2 * ho - 1 + kh;
        if (h < 0 || h >= H) continue;
        for (int kw = 0; kw < 3; ++kw) {
            const int w = 2 * wo - 1 + kw;
            if (w < 0 || w >= W) continue;
            float v[8];
            ld8(x + (((int64_t)n * H + h) * W + w) * C + c8, v);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (first || v[j] > m[j] || v[j] != v[j]) { m[j] = v[j]; am[j] = kh * 3 + kw; }
            first = false;
        }
    }
    st8(y + i * 8, m);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { lo |= (uint32_t)am[j] << (8 * j); hi |= (uint32_t)am[4 + j] << (8 * j); }
    *reinterpret_cast<uint2*>(idx + i * 8) = make_uint2(lo, hi);
}

// Backward gathers: a thread owns 8 channels of the 2 x 2 block of input pixels (2k - 1 + dh, 2l - 1 + dw); rows 2k - 1 and 2k lie under windows k - 1 and k only,
// so the block reads at most four windows' gradients and winning taps once.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_p1_bwd_kernel(const T* __restrict__ dy, const uint8_t* __restrict__ idx, T* __restrict__ dx, int N, int H, int W, int C, int Ho,
                                                             int Wo) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int cb = C / 8, Hb = (H + 2) >> 1, Wb = (W + 2) >> 1;
    if (i >= (int64_t)N * Hb * Wb * cb) return;
    const int c8 = (int)(i % cb) * 8;
    const int64_t blk = i / cb;
    const int l = (int)(blk % Wb), k = (int)((blk / Wb) % Hb), n = (int)(blk / ((int64_t)Wb * Hb));
    float g[2][2][8];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int j = 0; j < 8; ++j) g[a][b][j] = 0.f;
#pragma unroll
    for (int wh = 0; wh < 2; ++wh) {
        const int ho = k - 1 + wh;
        if (ho < 0 || ho >= Ho) continue;
#pragma unroll
        for (int ww = 0; ww < 2; ++ww) {
            const int wo = l - 1 + ww;
            if (wo < 0 || wo >= Wo) continue;
            const int64_t o = ((((int64_t)n * Ho + ho) * Wo + wo) * C + c8);
            const uint2 a = *reinterpret_cast<const uint2*>(idx + o);
            float d[8];
            ld8(dy + o, d);
            // pixel (dh, dw) of the block is tap (2 (1 - wh) + dh, 2 (1 - ww) + dw) of this window
#pragma unroll
            for (int dh = 0; dh < 2; ++dh) {
                const int kh = 2 * (1 - wh) + dh;
                if (kh > 2) continue;
#pragma unroll
                for (int dw = 0; dw < 2; ++dw) {
                    const int kw = 2 * (1 - ww) + dw;
                    if (kw > 2) continue;
                    const uint32_t tap = (uint32_t)(kh * 3 + kw);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (((a.x >> (8 * j)) & 0xffu) == tap) g[dh][dw][j] += d[j];
                        if (((a.y >> (8 * j)) & 0xffu) == tap) g[dh][dw][4 + j] += d[4 + j];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int dh = 0; dh < 2; ++dh) {
        const int h = 2 * k - 1 + dh;
        if (h < 0 || h >= H) continue;
#pragma unroll
        for (int dw = 0; dw < 2; ++dw) {
            const int w = 2 * l - 1 + dw;
            if (w < 0 || w >= W) continue;
            st8(dx + (((int64_t)n * H + h) * W + w) * C + c8, g[dh][dw]);
        }
    }
}

// ---- global average pool: (F, HW, C) -> (F, C) fp32 ----------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const T* __restrict__ x, float* __restrict__ y, int F, int HW, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;          // 8 channels of one frame
    const int cb = C / 8;
    if (i >= (int64_t)F * cb) return;
    const int c8 = (int)(i % cb) * 8;
    const int64_t f = i / cb;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    const T* p = x + f * HW * C + c8;
    for (int r = 0; r < HW; ++r) {
        float v[8];
        ld8(p + (int64_t)r * C, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += v[j];
    }
    const float inv = 1.0f / (float)HW;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= inv;
    st8(y + f * C + c8, acc);
}

template <typename T>
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const float* __restrict__ dy, T* __restrict__ dx, int F, int HW, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;          // 8 channels of one pixel
    const int cb = C / 8;
    if (i >= (int64_t)F * HW * cb) return;
    const int c8 = (int)(i % cb) * 8;
    const int64_t f = i / cb / HW;
    float g[8];
    ld8(dy + f * C + c8, g);
    const float inv = 1.0f / (float)HW;
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] *= inv;
    st8(dx + i * 8, g);
}

static int bn_check(const char* who, int64_t M, int C) {
    MAED_CHECK_ARG(C > 0 && C % 8 == 0, MAED_ERR_SHAPE, "%s: C=%d must be a multiple of 8", who, C);
    MAED_CHECK_ARG(M >= 0 && M < (int64_t)1 << 31, MAED_ERR_SHAPE, "%s: M=%lld rows out of range", who, (long long)M);
    return MAED_OK;
}

static int bn_finalize(const double* sums, int chunks, int C, double count, float eps, float* mean, float* mean_lo, float* rstd, float* running_mean, float* running_var,
                       float momentum, hipStream_t s) {
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)((C + 15) / 16)), dim3(BN_NT), 0, s, sums, chunks, C, count, eps, mean, mean_lo, rstd, running_mean, running_var,
                       momentum);
    MAED_CHECK_LAUNCH("batchnorm_finalize");
    return MAED_OK;
}

}  // namespace

extern "C" int maed_batchnorm_chunks(int64_t M) { return bn_chunks(M); }

extern "C" int maed_batchnorm_finalize(const double* sums, int chunks, int C, double count, float eps, float* mean, float* mean_lo, float* rstd, float* running_mean,
                                       float* running_var, float momentum, void* stream) {
    MAED_CHECK_ARG(sums && mean && rstd, MAED_ERR_ARG, "batchnorm_finalize: null pointer");
    MAED_CHECK_ARG(chunks > 0 && C > 0 && count >= 1.0, MAED_ERR_SHAPE, "batchnorm_finalize: chunks=%d C=%d count=%g", chunks, C, count);
    return bn_finalize(sums, chunks, C, count, eps, mean, mean_lo, rstd, running_mean, running_var, momentum, (hipStream_t)stream);
}

extern "C" int maed_batchnorm_stats(const void* x, int64_t M, int C, int dtype, double* partials, float eps, float* mean, float* mean_lo, float* rstd, float* running_mean,
                                    float* running_var, float momentum, void* stream) {
    MAED_CHECK_ARG(x && partials && mean && rstd, MAED_ERR_ARG, "batchnorm_stats: null pointer");
    MAED_PROPAGATE(bn_check("batchnorm_stats", M, C));
    MAED_CHECK_ARG(M >= 1, MAED_ERR_SHAPE, "batchnorm_stats: no rows");
    MAED_CHECK_ARG(is_aligned(x, 16), MAED_ERR_ALIGN, "batchnorm_stats: x must be 16-B aligned");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MAED_BF16) {
        const bn_geom g = bn_geometry(M, C, 8);
        hipLaunchKernelGGL((bn_stats_kernel<bf16, 8>), dim3(g.chunks, g.ntile), dim3(BN_NT), 0, s, (const bf16*)x, partials, (int)M, C, g.rpc);
    } else if (dtype == MAED_F32) {
        const bn_geom g = bn_geometry(M, C, 4);
        hipLaunchKernelGGL((bn_stats_kernel<float, 4>), dim3(g.chunks, g.ntile), dim3(BN_NT), 0, s, (const float*)x, partials, (int)M, C, g.rpc);
    } else { maed_set_error("batchnorm_stats: bad dtype %d", dtype); return MAED_ERR_ARG; }
    MAED_CHECK_LAUNCH("batchnorm_stats");
    return bn_finalize(partials, bn_chunks(M), C, (double)M, eps, mean, mean_lo, rstd, running_mean, running_var, momentum, s);
}

extern "C" int maed_batchnorm_apply_fwd(const void* x, const void* residual, const float* mean, const float* rstd, const float* gamma, const float* beta, void* y,
                                        uint8_t* relu_mask, int64_t M, int C, int relu, int dtype, void* stream) {
    MAED_CHECK_ARG(x && mean && rstd && gamma && beta && y, MAED_ERR_ARG, "batchnorm_apply_fwd: null pointer");
    MAED_PROPAGATE(bn_check("batchnorm_apply_fwd", M, C));
    MAED_CHECK_ARG(is_aligned(x, 16) && is_aligned(y, 16) && is_aligned(residual, 16) && is_aligned(mean, 16) && is_aligned(rstd, 16) && is_aligned(gamma, 16) &&
                   is_aligned(beta, 16), MAED_ERR_ALIGN, "batchnorm_apply_fwd: 16-B alignment");
    if (M == 0) return MAED_OK;
    hipStream_t s = (hipStream_t)stream;
    const bool mask = residual && relu && relu_mask;
#define BN_APPLY(T_, V_, RES_, RELU_, MASK_) do { const bn_geom g = bn_geometry(M, C, V_); \
        hipLaunchKernelGGL((bn_apply_kernel<T_, V_, RES_, RELU_, MASK_>), dim3(g.chunks, g.ntile), dim3(BN_NT), 0, s, (const T_*)x, (const T_*)residual, mean, rstd, gamma, beta, \
                           (T_*)y, relu_mask, (int)M, C, g.rpc); } while (0)
#define BN_APPLY_T(T_, V_) do { \
        if (mask) BN_APPLY(T_, 8, true, true, true); \
        else if (residual && relu) BN_APPLY(T_, V_, true, true, false); \
        else if (residual) BN_APPLY(T_, V_, true, false, false); \
        else if (relu) BN_APPLY(T_, V_, false, true, false); \
        else BN_APPLY(T_, V_, false, false, false); } while (0)
    if (dtype == MAED_BF16) BN_APPLY_T(bf16, 8);
    else if (dtype == MAED_F32) BN_APPLY_T(float, 4);
    else { maed_set_error("batchnorm_apply_fwd: bad dtype %d", dtype); return MAED_ERR_ARG; }
#undef BN_APPLY_T
#undef BN_APPLY
    MAED_CHECK_LAUNCH("batchnorm_apply_fwd");
    return MAED_OK;
}

// ReLU handling of the backward: 0 none, 1 recomputed from x, 2 the forward's bit mask
static int bn_bwd_mode(int relu, const uint8_t* relu_mask) { return !relu ? 0 : relu_mask ? 2 : 1; }

extern "C" int maed_batchnorm_bwd_reduce(const void* x, const void* dy, const uint8_t* relu_mask, const float* mean, const float* mean_lo, const float* rstd, const float* gamma, const float* beta,
                                         double* partials, float* sums, float* dgamma, float* dbeta, int64_t M, int C, int relu, int dtype, void* stream) {
    MAED_CHECK_ARG(x && dy && mean && rstd && gamma && beta && partials, MAED_ERR_ARG, "batchnorm_bwd_reduce: null pointer");
    MAED_PROPAGATE(bn_check("batchnorm_bwd_reduce", M, C));
    MAED_CHECK_ARG(M >= 1, MAED_ERR_SHAPE, "batchnorm_bwd_reduce: no rows");
    MAED_CHECK_ARG(is_aligned(x, 16) && is_aligned(dy, 16) && is_aligned(mean, 16) && is_aligned(mean_lo, 16) && is_aligned(rstd, 16) && is_aligned(gamma, 16) && is_aligned(beta, 16), MAED_ERR_ALIGN,
                   "batchnorm_bwd_reduce: 16-B alignment");
    hipStream_t s = (hipStream_t)stream;
    const int mode = bn_bwd_mode(relu, relu_mask);
#define BN_RED(T_, V_, MODE_) do { const bn_geom g = bn_geometry(M, C, V_); \
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<T_, V_, MODE_>), dim3(g.chunks, g.ntile), dim3(BN_NT), 0, s, (const T_*)x, (const T_*)dy, relu_mask, mean, mean_lo, rstd, gamma, beta, \
                           partials, (int)M, C, g.rpc); } while (0)
#define BN_RED_T(T_, V_) do { if (mode == 2) BN_RED(T_, 8, 2); else if (mode == 1) BN_RED(T_, V_, 1); else BN_RED(T_, V_, 0); } while (0)
    if (dtype == MAED_BF16) BN_RED_T(bf16, 8);
    else if (dtype == MAED_F32) BN_RED_T(float, 4);
    else { maed_set_error("batchnorm_bwd_reduce: bad dtype %d", dtype); return MAED_ERR_ARG; }
#undef BN_RED_T
#undef BN_RED
    MAED_CHECK_LAUNCH("batchnorm_bwd_reduce");
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)((C + 15) / 16)), dim3(BN_NT), 0, s, (const double*)partials, bn_chunks(M), C, sums, dgamma, dbeta);
    MAED_CHECK_LAUNCH("batchnorm_bwd_finalize");
    return MAED_OK;
}

extern "C" int maed_batchnorm_bwd_apply(const void* x, const void* dy, const uint8_t* relu_mask, const float* mean, const float* mean_lo, const float* rstd, const float* gamma, const float* beta,
                                        const float* sums, void* dx, void* dres, int64_t M, int C, int relu, int dtype, void* stream) {
    MAED_CHECK_ARG(x && dy && mean && rstd && gamma && beta && dx, MAED_ERR_ARG, "batchnorm_bwd_apply: null pointer");
    MAED_PROPAGATE(bn_check("batchnorm_bwd_apply", M, C));
    MAED_CHECK_ARG(is_aligned(x, 16) && is_aligned(dy, 16) && is_aligned(dx, 16) && is_aligned(dres, 16) && is_aligned(mean, 16) && is_aligned(mean_lo, 16) && is_aligned(rstd, 16) &&
                   is_aligned(gamma, 16) && is_aligned(beta, 16), MAED_ERR_ALIGN, "batchnorm_bwd_apply: 16-B alignment");
    if (M == 0) return MAED_OK;
    hipStream_t s = (hipStream_t)stream;
    const int mode = bn_bwd_mode(relu, relu_mask);
    const bool frozen = sums == nullptr;
#define BN_BAP(T_, V_, MODE_, FR_) do { const bn_geom g = bn_geometry(M, C, V_); \
        hipLaunchKernelGGL((bn_bwd_apply_kernel<T_, V_, MODE_, FR_>), dim3(g.chunks, g.ntile), dim3(BN_NT), 0, s, (const T_*)x, (const T_*)dy, relu_mask, mean, mean_lo, rstd, gamma, beta, \
                           sums, (T_*)dx, (T_*)dres, (int)M, C, g.rpc); } while (0)
#define BN_BAP_M(T_, V_, FR_) do { if (mode == 2) BN_BAP(T_, 8, 2, FR_); else if (mode == 1) BN_BAP(T_, V_, 1, FR_); else BN_BAP(T_, V_, 0, FR_); } while (0)
#define BN_BAP_T(T_, V_) do { if (frozen) BN_BAP_M(T_, V_, true); else BN_BAP_M(T_, V_, false); } while (0)
    if (dtype == MAED_BF16) BN_BAP_T(bf16, 8);
    else if (dtype == MAED_F32) BN_BAP_T(float, 4);
    else { maed_set_error("batchnorm_bwd_apply: bad dtype %d", dtype); return MAED_ERR_ARG; }
#undef BN_BAP_T
#undef BN_BAP_M
#undef BN_BAP
    MAED_CHECK_LAUNCH("batchnorm_bwd_apply");
    return MAED_OK;
}

// ---- the entry points with an all-reduce of a record between reduction and consumer (the one-rank entry points above stay as they are) ----
extern "C" int maed_batchnorm_stats_local(const void* x, int64_t M, int C, int dtype, double* partials, double* record, void* stream) {
    MAED_CHECK_ARG(x && partials && record, MAED_ERR_ARG, "batchnorm_stats_local: null pointer");
    MAED_PROPAGATE(bn_check("batchnorm_stats_local", M, C));
    MAED_CHECK_ARG(M >= 1, MAED_ERR_SHAPE, "batchnorm_stats_local: no rows");
    MAED_CHECK_ARG(is_aligned(x, 16) && is_aligned(record, 8), MAED_ERR_ALIGN, "batchnorm_stats_local: x must be 16-B aligned, record 8-B");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MAED_BF16) {
        const bn_geom g = bn_geometry(M, C, 8);
        hipLaunchKernelGGL((bn_stats_kernel<bf16, 8>), dim3(g.chunks, g.ntile), dim3(BN_NT), 0, s, (const bf16*)x, partials, (int)M, C, g.rpc);
    } else if (dtype == MAED_F32) {
        const bn_geom g = bn_geometry(M, C, 4);
        hipLaunchKernelGGL((bn_stats_kernel<float, 4>), dim3(g.chunks, g.ntile), dim3(BN_NT), 0, s, (const float*)x, partials, (int)M, C, g.rpc);
    } else { maed_set_error("batchnorm_stats_local: bad dtype %d", dtype); return MAED_ERR_ARG; }
    MAED_CHECK_LAUNCH("batchnorm_stats_local");
    hipLaunchKernelGGL(bn_record_kernel, dim3((unsigned)((C + 15) / 16)), dim3(BN_NT), 0, s, (const double*)partials, bn_chunks(M), C, record, (double)M, (float*)nullptr,
                       (float*)nullptr);
    MAED_CHECK_LAUNCH("batchnorm_stats_local record");
    return MAED_OK;
}

extern "C" int maed_batchnorm_finalize_dev(const double* record, int C, float eps, float* mean, float* mean_lo, float* rstd, float* running_mean, float* running_var,
                                           float momentum, void* stream) {
    MAED_CHECK_ARG(record && mean && rstd, MAED_ERR_ARG, "batchnorm_finalize_dev: null pointer");
    MAED_CHECK_ARG(C > 0, MAED_ERR_SHAPE, "batchnorm_finalize_dev: C=%d", C);
    MAED_CHECK_ARG(is_aligned(record, 8), MAED_ERR_ALIGN, "batchnorm_finalize_dev: record must be 8-B aligned");
    hipLaunchKernelGGL(bn_finalize_dev_kernel, dim3((unsigned)((C + BN_NT - 1) / BN_NT)), dim3(BN_NT), 0, (hipStream_t)stream, record, C, eps, mean, mean_lo, rstd, running_mean,
                       running_var, momentum);
    MAED_CHECK_LAUNCH("batchnorm_finalize_dev");
    return MAED_OK;
}

extern "C" int maed_batchnorm_bwd_reduce_local(const void* x, const void* dy, const uint8_t* relu_mask, const float* mean, const float* mean_lo, const float* rstd, const float* gamma,
                                               const float* beta, double* partials, double* record, float* dgamma, float* dbeta, int64_t M, int C, int relu, int dtype, void* stream) {
    MAED_CHECK_ARG(x && dy && mean && rstd && gamma && beta && partials && record, MAED_ERR_ARG, "batchnorm_bwd_reduce_local: null pointer");
    MAED_PROPAGATE(bn_check("batchnorm_bwd_reduce_local", M, C));
    MAED_CHECK_ARG(M >= 1, MAED_ERR_SHAPE, "batchnorm_bwd_reduce_local: no rows");
    MAED_CHECK_ARG(is_aligned(x, 16) && is_aligned(dy, 16) && is_aligned(mean, 16) && is_aligned(mean_lo, 16) && is_aligned(rstd, 16) && is_aligned(gamma, 16) && is_aligned(beta, 16) &&
                   is_aligned(record, 8), MAED_ERR_ALIGN, "batchnorm_bwd_reduce_local: 16-B alignment (record: 8-B)");
    hipStream_t s = (hipStream_t)stream;
    const int mode = bn_bwd_mode(relu, relu_mask);
#define BN_RED(T_, V_, MODE_) do { const bn_geom g = bn_geometry(M, C, V_); \
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<T_, V_, MODE_>), dim3(g.chunks, g.ntile), dim3(BN_NT), 0, s, (const T_*)x, (const T_*)dy, relu_mask, mean, mean_lo, rstd, gamma, beta, \
                           partials, (int)M, C, g.rpc); } while (0)
#define BN_RED_T(T_, V_) do { if (mode == 2) BN_RED(T_, 8, 2); else if (mode == 1) BN_RED(T_, V_, 1); else BN_RED(T_, V_, 0); } while (0)
    if (dtype == MAED_BF16) BN_RED_T(bf16, 8);
    else if (dtype == MAED_F32) BN_RED_T(float, 4);
    else { maed_set_error("batchnorm_bwd_reduce_local: bad dtype %d", dtype); return MAED_ERR_ARG; }
#undef BN_RED_T
#undef BN_RED
    MAED_CHECK_LAUNCH("batchnorm_bwd_reduce_local");
    hipLaunchKernelGGL(bn_record_kernel, dim3((unsigned)((C + 15) / 16)), dim3(BN_NT), 0, s, (const double*)partials, bn_chunks(M), C, record, 0.0, dgamma, dbeta);
    MAED_CHECK_LAUNCH("batchnorm_bwd_reduce_local record");
    return MAED_OK;
}

extern "C" int maed_batchnorm_bwd_apply_dev(const void* x, const void* dy, const uint8_t* relu_mask, const float* mean, const float* mean_lo, const float* rstd, const float* gamma,
                                            const float* beta, const double* record, const double* count, void* dx, void* dres, int64_t M, int C, int relu, int dtype, void* stream) {
    MAED_CHECK_ARG(x && dy && mean && rstd && gamma && beta && record && count && dx, MAED_ERR_ARG, "batchnorm_bwd_apply_dev: null pointer");
    MAED_PROPAGATE(bn_check("batchnorm_bwd_apply_dev", M, C));
    MAED_CHECK_ARG(is_aligned(x, 16) && is_aligned(dy, 16) && is_aligned(dx, 16) && is_aligned(dres, 16) && is_aligned(mean, 16) && is_aligned(mean_lo, 16) && is_aligned(rstd, 16) &&
                   is_aligned(gamma, 16) && is_aligned(beta, 16) && is_aligned(record, 8) && is_aligned(count, 8), MAED_ERR_ALIGN,
                   "batchnorm_bwd_apply_dev: 16-B alignment (record, count: 8-B)");
    if (M == 0) return MAED_OK;
    hipStream_t s = (hipStream_t)stream;
    const int mode = bn_bwd_mode(relu, relu_mask);
#define BN_BAP(T_, V_, MODE_) do { const bn_geom g = bn_geometry(M, C, V_); \
        hipLaunchKernelGGL((bn_bwd_apply_dev_kernel<T_, V_, MODE_>), dim3(g.chunks, g.ntile), dim3(BN_NT), 0, s, (const T_*)x, (const T_*)dy, relu_mask, mean, mean_lo, rstd, gamma, beta, \
                           record, count, (T_*)dx, (T_*)dres, (int)M, C, g.rpc); } while (0)
#define BN_BAP_T(T_, V_) do { if (mode == 2) BN_BAP(T_, 8, 2); else if (mode == 1) BN_BAP(T_, V_, 1); else BN_BAP(T_, V_, 0); } while (0)
    if (dtype == MAED_BF16) BN_BAP_T(bf16, 8);
    else if (dtype == MAED_F32) BN_BAP_T(float, 4);
    else { maed_set_error("batchnorm_bwd_apply_dev: bad dtype %d", dtype); return MAED_ERR_ARG; }
#undef BN_BAP_T
#undef BN_BAP
    MAED_CHECK_LAUNCH("batchnorm_bwd_apply_dev");
    return MAED_OK;
}

static int pool_check(const char* who, int N, int H, int W, int C) {
    MAED_CHECK_ARG(N >= 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, MAED_ERR_SHAPE, "%s: N=%d H=%d W=%d C=%d (C must be a multiple of 8)", who, N, H, W, C);
    return MAED_OK;
}

extern "C" int maed_maxpool3s2p1_fwd(const void* x, void* y, uint8_t* idx, int N, int H, int W, int C, int dtype, void* stream) {
    MAED_CHECK_ARG(x && y && idx, MAED_ERR_ARG, "maxpool3s2p1_fwd: null pointer");
    MAED_PROPAGATE(pool_check("maxpool3s2p1_fwd", N, H, W, C));
    MAED_CHECK_ARG(is_aligned(x, 16) && is_aligned(y, 16) && is_aligned(idx, 8), MAED_ERR_ALIGN, "maxpool3s2p1_fwd: alignment");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int64_t n = (int64_t)N * Ho * Wo * (C / 8);
    if (n == 0) return MAED_OK;
    MAED_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((maxpool_p1_fwd_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                                                      (const T*)x, (T*)y, idx, N, H, W, C, Ho, Wo));
    MAED_CHECK_LAUNCH("maxpool3s2p1_fwd");
    return MAED_OK;
}

extern "C" int maed_maxpool3s2p1_bwd(const void* dy, const uint8_t* idx, void* dx, int N, int H, int W, int C, int dtype, void* stream) {
    MAED_CHECK_ARG(dy && idx && dx, MAED_ERR_ARG, "maxpool3s2p1_bwd: null pointer");
    MAED_PROPAGATE(pool_check("maxpool3s2p1_bwd", N, H, W, C));
    MAED_CHECK_ARG(is_aligned(dy, 16) && is_aligned(dx, 16) && is_aligned(idx, 8), MAED_ERR_ALIGN, "maxpool3s2p1_bwd: alignment");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int64_t n = (int64_t)N * ((H + 2) / 2) * ((W + 2) / 2) * (C / 8);       // 2 x 2 blocks of input pixels
    if (n == 0) return MAED_OK;
    MAED_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((maxpool_p1_bwd_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                                                      (const T*)dy, idx, (T*)dx, N, H, W, C, Ho, Wo));
    MAED_CHECK_LAUNCH("maxpool3s2p1_bwd");
    return MAED_OK;
}

extern "C" int maed_avgpool_fwd(const void* x, float* y, int F, int HW, int C, int dtype, void* stream) {
    MAED_CHECK_ARG(x && y, MAED_ERR_ARG, "avgpool_fwd: null pointer");
    MAED_CHECK_ARG(F >= 0 && HW > 0 && C > 0 && C % 8 == 0, MAED_ERR_SHAPE, "avgpool_fwd: F=%d HW=%d C=%d (C must be a multiple of 8)", F, HW, C);
    MAED_CHECK_ARG(is_aligned(x, 16) && is_aligned(y, 16), MAED_ERR_ALIGN, "avgpool_fwd: 16-B alignment");
    const int64_t n = (int64_t)F * (C / 8);
    if (n == 0) return MAED_OK;
    MAED_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((avgpool_fwd_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const T*)x, y, F, HW, C));
    MAED_CHECK_LAUNCH("avgpool_fwd");
    return MAED_OK;
}

extern "C" int maed_avgpool_bwd(const float* dy, void* dx, int F, int HW, int C, int dtype, void* stream) {
    MAED_CHECK_ARG(dy && dx, MAED_ERR_ARG, "avgpool_bwd: null pointer");
    MAED_CHECK_ARG(F >= 0 && HW > 0 && C > 0 && C % 8 == 0, MAED_ERR_SHAPE, "avgpool_bwd: F=%d HW=%d C=%d (C must be a multiple of 8)", F, HW, C);
    MAED_CHECK_ARG(is_aligned(dy, 16) && is_aligned(dx, 16), MAED_ERR_ALIGN, "avgpool_bwd: 16-B alignment");
    const int64_t n = (int64_t)F * HW * (C / 8);
    if (n == 0) return MAED_OK;
    MAED_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((avgpool_bwd_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, (T*)dx, F, HW, C));
    MAED_CHECK_LAUNCH("avgpool_bwd");
    return MAED_OK;
}
