// Attention for head sizes other than 64: the tiled kernels of attn_long.hip as templates on the head size DH (DH % 32 == 0, DH <= 128) over a
// strided-sequence geometry, so that ONE family serves spatial attention, coupling and temporal attention.  Included from attn_long.hip (no source of
// its own: both builds treat it as a header), after that file's kernels: LT, WG_ROWS, long_xcd_remap and the fragment helpers of attn_mfma.cuh are shared.
//
// Geometry: `G` groups of `L` x `inner` token rows; sequence (g, h, i) is rows g*L*inner + j*inner + i (j < L) of the (rows, 3C) qkv matrix, channels
// h*DH .. h*DH + DH - 1 of the q | k | v blocks.
//   spatial  (vision_transformer.py:206-214)  G = F,     L = P,   inner = 1   F*H sequences of P rows at stride 3C
//   coupling (:160-163)                       G = F/T,   L = T*P, inner = 1
//   temporal (:216-228)                       G = F/T,   L = T,   inner = P   N*P*H sequences of T rows at stride P*3C: (F,P,3C) / (F,P,C) in place
// lse keeps the layouts of the 64-wide kernels: inner == 1: (G, H, L); inner > 1: (G*L, H, inner) = (F, H, P).
//
// Same arithmetic as attn_long.hip: S^T = K Q^T (softmax statistics per lane), lazy rescaling, lse in natural log, result tiles leave as full lines
// through LDS patches, `accumulate` adds into dqkv.  What depends on DH: DH/16 k-steps per score tile, DH/32 output sub-tiles (f32x16 accumulators),
// DH/8 16-byte chunks per tile row.  LDS rows have stride DH + 8 elements = an ODD number of 16-byte units (5 / 9 / 13 / 17 for 32 / 64 / 96 / 128), the
// property KLD = 72 has for DH = 64: the 32 rows a ds_read_b128 touches start in 32 different 16-byte bank groups.
// The 64 instantiation exists for the tests only (it must agree with attn_long.hip's kernels); the 64-wide entry points never come here.
#undef D

namespace {

struct SeqGeom { int G, L, inner, H; };

__device__ __forceinline__ int64_t seq_lse_index(const SeqGeom& gm, int g, int h, int i, int j) {
    return gm.inner == 1 ? ((int64_t)g * gm.H + h) * gm.L + j : (((int64_t)g * gm.L + j) * gm.H + h) * gm.inner + i;
}

template <int LDK>
__device__ __forceinline__ bf16x8_t lds_frag_tr_rm_ld(const unsigned short* X, int key_base, int e_base, int lane) {   // lds_frag_tr_rm (attn_mfma.cuh) at row stride LDK
    const int i = lane & 15;
    const unsigned short* p = X + (key_base + 4 * (lane >> 5) + (i >> 2)) * LDK + e_base + (lane & 16) + 4 * (i & 3);
    union { bf16x8_t v; uint2 u[2]; } f;
    auto lo = MAED_DS_READ_TR16(p);
    auto hi = MAED_DS_READ_TR16(p + 8 * LDK);
    __builtin_memcpy(&f.u[0], &lo, 8);
    __builtin_memcpy(&f.u[1], &hi, 8);
    return f.v;
}

// One streamed tile = 64 rows x DH bf16.  Thread t stages row t >> 2, chunks (t & 3) + 4k (k < DH/32): the four threads of a row are consecutive lanes (the
// dK/dV pass sums delta = rowsum(dO * O) over them with two shuffles) and one instruction of a wave reads 16 rows x 64 contiguous bytes.
// (named members, not an array: see TileRegs in attn_long.hip -- and exactly the members an instantiation loads: a struct with members that are never written
//  stays in scratch memory as a whole)
typedef uint32_t seq_u32x4_t __attribute__((ext_vector_type(4)));      // (a native vector: a chunk is one SSA value, never a 16-byte struct copy through memory)
template <int DH> struct TileRegsH;
template <> struct TileRegsH<32> { seq_u32x4_t a; };
template <> struct TileRegsH<64> { seq_u32x4_t a, b; };
template <> struct TileRegsH<96> { seq_u32x4_t a, b, c; };
template <> struct TileRegsH<128> { seq_u32x4_t a, b, c, d; };

template <int DH>
__device__ __forceinline__ void tile_load_h(TileRegsH<DH>& t, const bf16* src, int64_t ld, int r0, int L, int tid) {
    int row = r0 + (tid >> 2);
    if (row > L - 1) row = L - 1;                   // finite filler that the callers mask
    const seq_u32x4_t* p = reinterpret_cast<const seq_u32x4_t*>(src + (int64_t)row * ld) + (tid & 3);
    t.a = p[0];
    if constexpr (DH >= 64) t.b = p[4];
    if constexpr (DH >= 96) t.c = p[8];
    if constexpr (DH >= 128) t.d = p[12];
}
template <int DH>
__device__ __forceinline__ void tile_store_h(const TileRegsH<DH>& t, unsigned short* rows, int tid) {
    seq_u32x4_t* p = reinterpret_cast<seq_u32x4_t*>(rows + (tid >> 2) * (DH + 8)) + (tid & 3);
    p[0] = t.a;
    if constexpr (DH >= 64) p[4] = t.b;
    if constexpr (DH >= 96) p[8] = t.c;
    if constexpr (DH >= 128) p[12] = t.d;
}
__device__ __forceinline__ float chunk_dot_h(const seq_u32x4_t x, const seq_u32x4_t y) {
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        d = fmaf(__uint_as_float(x[j] << 16), __uint_as_float(y[j] << 16), d);
        d = fmaf(__uint_as_float(x[j] & 0xffff0000u), __uint_as_float(y[j] & 0xffff0000u), d);
    }
    return d;
}
template <int DH>
__device__ __forceinline__ float tile_dot_h(const TileRegsH<DH>& x, const TileRegsH<DH>& y) {
    float d = chunk_dot_h(x.a, y.a);
    if constexpr (DH >= 64) d += chunk_dot_h(x.b, y.b);
    if constexpr (DH >= 96) d += chunk_dot_h(x.c, y.c);
    if constexpr (DH >= 128) d += chunk_dot_h(x.d, y.d);
    return d;
}

// store_tile_lines (attn_mfma.cuh) for a 32 x DH result tile: the wave's patch holds 32 rows of DH bf16 (64 * DH bytes), 16-byte chunk c of row r at slot
// (c + r) mod DH/8 (a rotation: DH/8 = 12 is no power of two), then DH/16 16-byte stores per lane, DH/8 lanes per row: every row leaves as one 2*DH-byte line.
template <int DH>
__device__ __forceinline__ void store_tile_lines_h(unsigned short* patch, bf16* row0_ptr, int64_t row_stride, int n_valid, const f32x16_t (&acc)[DH / 32], int lane,
                                                   int accumulate) {
    constexpr int NCH = DH / 8;
    const int l31 = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int et = 0; et < DH / 32; ++et)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<uint2*>(patch + l31 * DH + (((4 * et + g + l31) % NCH) << 3) + 4 * hi) =
                make_uint2(pack_bf2(acc[et][4 * g], acc[et][4 * g + 1]), pack_bf2(acc[et][4 * g + 2], acc[et][4 * g + 3]));
    MAED_WAVE_LDS_SYNC();
#pragma unroll
    for (int r = 0; r < NCH / 2; ++r) {
        const int n = r * 64 + lane, row = n / NCH, c = n - row * NCH;
        if (row < n_valid) {
            bf16* dst = row0_ptr + row * row_stride + c * 8;
            uint4 v = *reinterpret_cast<const uint4*>(patch + row * DH + (((c + row) % NCH) << 3));
            if (accumulate) {
                float a[8];
                ld8(dst, a);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) { a[2 * j] += __uint_as_float(w[j] << 16); a[2 * j + 1] += __uint_as_float(w[j] & 0xffff0000u); }
                st8(dst, a);
            } else *reinterpret_cast<uint4*>(dst) = v;
        }
    }
    MAED_WAVE_LDS_SYNC();
}

// workgroups per CU the register budget allows (256 threads = one wave per SIMD, 512 registers per lane and SIMD): forward and dQ pass hold DH/32 accumulators,
// DH/16 (x2) operand fragments and two tiles in flight; the dK/dV pass two sets of accumulators, two sets of fragments and three tiles
constexpr int seq_occ_fwd(int DH) { return DH <= 64 ? 4 : 2; }
constexpr int seq_occ_dq(int DH) { return DH <= 64 ? 3 : 2; }
constexpr int seq_occ_dkv(int DH) { return DH <= 64 ? 2 : 1; }

template <int DH>
__global__ __launch_bounds__(256, seq_occ_fwd(DH)) void attn_seq_fwd_mfma(const bf16* __restrict__ qkv, bf16* __restrict__ o, float* __restrict__ lse, int seq_len,
                                                                         int seq_inner, int seq_heads, int ntile, float scale_log2e) {
    const SeqGeom gm{0, seq_len, seq_inner, seq_heads};
    constexpr int KL = DH + 8, NK = DH / 16, NE = DH / 32;
    __shared__ __attribute__((aligned(16))) unsigned short smem[2 * LT * KL];
    unsigned short* const Ks = smem;
    unsigned short* const Vs = smem + LT * KL;       // row-major: V^T fragments come from transposing reads
    const int bid = long_xcd_remap(blockIdx.x, gridDim.x);
    const int item = bid / ntile, tile = bid - item * ntile;
    const int i = item % gm.inner, gh = item / gm.inner, g = gh / gm.H, h = gh - g * gm.H;
    const int L = gm.L, C = gm.H * DH;
    const int64_t ld = 3 * (int64_t)C * gm.inner, ldo = (int64_t)C * gm.inner, row0 = (int64_t)g * L * gm.inner + i;
    const bf16* base = qkv + row0 * 3 * C + h * DH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int q0 = tile * WG_ROWS + wave * 32, q = q0 + l31;
    const bool active = q0 < L;                     // wave-uniform; inactive waves still stage tiles and meet the barriers
    const int qc = q < L ? q : L - 1;
    bf16x8_t qf[NK];
#pragma unroll
    for (int t = 0; t < NK; ++t) qf[t] = *reinterpret_cast<const bf16x8_t*>(base + (int64_t)qc * ld + t * 16 + hi * 8);
    f32x16_t oacc[NE];
#pragma unroll
    for (int et = 0; et < NE; ++et)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[et][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int nkt = (L + LT - 1) / LT;
    TileRegsH<DH> kreg, vreg;
    tile_load_h<DH>(kreg, base + C, ld, 0, L, tid);
    tile_load_h<DH>(vreg, base + 2 * C, ld, 0, L, tid);
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();                            // every wave is done with the previous tile
        tile_store_h<DH>(kreg, Ks, tid);
        tile_store_h<DH>(vreg, Vs, tid);
        __syncthreads();
        if (kt + 1 < nkt) {                         // next tile's loads fly while this one is consumed
            tile_load_h<DH>(kreg, base + C, ld, (kt + 1) * LT, L, tid);
            tile_load_h<DH>(vreg, base + 2 * C, ld, (kt + 1) * LT, L, tid);
        }
        if (!active) continue;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int k0 = kt * LT + sub * 32;
            if (k0 >= L) break;
            f32x16_t s;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f;
            const unsigned short* kp = Ks + (sub * 32 + l31) * KL + hi * 8;
#pragma unroll
            for (int t = 0; t < NK; ++t)
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(kp + t * 16), qf[t], s, 0, 0, 0);
            // lane holds keys k0 + (r&3) + 8*(r>>2) + 4*hi of its query; only the sequence's last sub-tile has padding keys
            if (k0 + 32 > L) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = (k0 + (r & 3) + 8 * (r >> 2) + 4 * hi < L) ? s[r] : -INFINITY;
            }
            float mt = s[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mt = fmaxf(mt, s[r]);
            mt = fmaxf(mt, __shfl_xor(mt, 32, 64)) * scale_log2e;
            const bool grow = mt > m + 8.0f;        // lazy rescaling (attn_long.hip)
            if (__any(grow)) {
                const float mn = grow ? mt : m;
                const float alpha = __builtin_amdgcn_exp2f(m - mn);
                l *= alpha;
                m = mn;
#pragma unroll
                for (int et = 0; et < NE; ++et)
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[et][r] *= alpha;
            }
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], scale_log2e, -m)); ps += s[r]; }
            l += ps;
#pragma unroll
            for (int st = 0; st < 2; ++st) {        // O^T += V^T P^T, 16 keys per step
                const bf16x8_t pf = pack_frag(s, st);
#pragma unroll
                for (int et = 0; et < NE; ++et)
                    oacc[et] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_frag_tr_rm_ld<KL>(Vs, sub * 32 + 16 * st, et * 32, lane), pf, oacc[et], 0, 0, 0);
            }
        }
    }
    l += __shfl_xor(l, 32, 64);
    __syncthreads();                                // the K / V tiles are retired: their LDS carries the waves' output patches
    if (active) {
        const float inv = 1.f / l;
#pragma unroll
        for (int et = 0; et < NE; ++et)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[et][r] *= inv;
        store_tile_lines_h<DH>(smem + wave * 32 * DH, o + (row0 + (int64_t)q0 * gm.inner) * C + h * DH, ldo, L - q0, oacc, lane, 0);
    }
    if (active && q < L && hi == 0) lse[seq_lse_index(gm, g, h, i, q)] = (m + log2f(l)) * 0.69314718055994530942f;
}

template <int DH>
__global__ __launch_bounds__(256, seq_occ_dq(DH)) void attn_seq_bwd_dq_mfma(const bf16* __restrict__ qkv, const bf16* __restrict__ o, const bf16* __restrict__ d_o,
                                                                           const float* __restrict__ lse, bf16* __restrict__ dqkv, int accumulate, int seq_len, int seq_inner, int seq_heads, int ntile,
                                                                           float scale) {
    const SeqGeom gm{0, seq_len, seq_inner, seq_heads};
    constexpr int KL = DH + 8, NK = DH / 16, NE = DH / 32;
    __shared__ __attribute__((aligned(16))) unsigned short smem[2 * LT * KL];
    unsigned short* const Ks = smem;
    unsigned short* const Vs = smem + LT * KL;
    const int bid = long_xcd_remap(blockIdx.x, gridDim.x);
    const int item = bid / ntile, tile = bid - item * ntile;
    const int i = item % gm.inner, gh = item / gm.inner, g = gh / gm.H, h = gh - g * gm.H;
    const int L = gm.L, C = gm.H * DH;
    const int64_t ld = 3 * (int64_t)C * gm.inner, ldo = (int64_t)C * gm.inner, row0 = (int64_t)g * L * gm.inner + i;
    const bf16* base = qkv + row0 * 3 * C + h * DH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int q0 = tile * WG_ROWS + wave * 32, q = q0 + l31;
    const bool active = q0 < L;
    const int qc = q < L ? q : L - 1;
    const bf16* orow = o + (row0 + (int64_t)qc * gm.inner) * C + h * DH;
    const bf16* dorow = d_o + (row0 + (int64_t)qc * gm.inner) * C + h * DH;
    bf16x8_t qf[NK], dof[NK];
    float Dq = 0.f;                                 // delta = rowsum(dO * O) of this lane's query
#pragma unroll
    for (int t = 0; t < NK; ++t) {
        qf[t] = *reinterpret_cast<const bf16x8_t*>(base + (int64_t)qc * ld + t * 16 + hi * 8);
        dof[t] = *reinterpret_cast<const bf16x8_t*>(dorow + t * 16 + hi * 8);
        float a[8], b[8];
        ld8(dorow + t * 16 + hi * 8, a); ld8(orow + t * 16 + hi * 8, b);
#pragma unroll
        for (int j = 0; j < 8; ++j) Dq = fmaf(a[j], b[j], Dq);
    }
    Dq += __shfl_xor(Dq, 32, 64);
    const float l2e = 1.44269504088896340736f;
    const float L2 = lse[seq_lse_index(gm, g, h, i, qc)] * l2e, sl2e = scale * l2e;
    f32x16_t dq[NE];
#pragma unroll
    for (int et = 0; et < NE; ++et)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[et][r] = 0.f;
    const int nkt = (L + LT - 1) / LT;
    TileRegsH<DH> kreg, vreg;
    tile_load_h<DH>(kreg, base + C, ld, 0, L, tid);
    tile_load_h<DH>(vreg, base + 2 * C, ld, 0, L, tid);
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();
        tile_store_h<DH>(kreg, Ks, tid);
        tile_store_h<DH>(vreg, Vs, tid);
        __syncthreads();
        if (kt + 1 < nkt) {
            tile_load_h<DH>(kreg, base + C, ld, (kt + 1) * LT, L, tid);
            tile_load_h<DH>(vreg, base + 2 * C, ld, (kt + 1) * LT, L, tid);
        }
        if (!active) continue;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int k0 = kt * LT + sub * 32;
            if (k0 >= L) break;
            // -delta rides in the dP accumulator's initial value, the 1/sqrt(d) factor is applied once at the end (attn_long.hip)
            f32x16_t s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = -Dq; }
            const int off = (sub * 32 + l31) * KL + hi * 8;
#pragma unroll
            for (int t = 0; t < NK; ++t) {
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(Ks + off + t * 16), qf[t], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(Vs + off + t * 16), dof[t], dp, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], sl2e, -L2)) * dp[r];    // dS^T / scale
            if (k0 + 32 > L) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = (k0 + (r & 3) + 8 * (r >> 2) + 4 * hi < L) ? s[r] : 0.f;
            }
#pragma unroll
            for (int st = 0; st < 2; ++st) {        // dQ^T += K^T dS^T
                const bf16x8_t dsf = pack_frag(s, st);
#pragma unroll
                for (int et = 0; et < NE; ++et)
                    dq[et] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_frag_tr_rm_ld<KL>(Ks, sub * 32 + 16 * st, et * 32, lane), dsf, dq[et], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int et = 0; et < NE; ++et)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[et][r] *= scale;
    __syncthreads();
    if (active) store_tile_lines_h<DH>(smem + wave * 32 * DH, dqkv + (row0 + (int64_t)q0 * gm.inner) * 3 * C + h * DH, ld, L - q0, dq, lane, accumulate);
}

template <int DH>
__global__ __launch_bounds__(256, seq_occ_dkv(DH)) void attn_seq_bwd_dkv_mfma(const bf16* __restrict__ qkv, const bf16* __restrict__ o, const bf16* __restrict__ d_o,
                                                                             const float* __restrict__ lse, bf16* __restrict__ dqkv, int accumulate, int seq_len, int seq_inner, int seq_heads, int ntile,
                                                                             float scale) {
    const SeqGeom gm{0, seq_len, seq_inner, seq_heads};
    constexpr int KL = DH + 8, NK = DH / 16, NE = DH / 32;
    __shared__ __attribute__((aligned(16))) unsigned short smem[2 * LT * KL];
    __shared__ float Ls[LT], Ds[LT];
    unsigned short* const Qs = smem;
    unsigned short* const dOs = smem + LT * KL;
    const int bid = long_xcd_remap(blockIdx.x, gridDim.x);
    const int item = bid / ntile, tile = bid - item * ntile;
    const int i = item % gm.inner, gh = item / gm.inner, g = gh / gm.H, h = gh - g * gm.H;
    const int L = gm.L, C = gm.H * DH;
    const int64_t ld = 3 * (int64_t)C * gm.inner, ldo = (int64_t)C * gm.inner, row0 = (int64_t)g * L * gm.inner + i;
    const bf16* base = qkv + row0 * 3 * C + h * DH;
    const bf16* obase = o + row0 * C + h * DH;
    const bf16* dobase = d_o + row0 * C + h * DH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int k0w = tile * WG_ROWS + wave * 32, k = k0w + l31;
    const bool active = k0w < L;
    const int kc = k < L ? k : L - 1;
    bf16x8_t kf[NK], vf[NK];
#pragma unroll
    for (int t = 0; t < NK; ++t) {
        kf[t] = *reinterpret_cast<const bf16x8_t*>(base + C + (int64_t)kc * ld + t * 16 + hi * 8);
        vf[t] = *reinterpret_cast<const bf16x8_t*>(base + 2 * C + (int64_t)kc * ld + t * 16 + hi * 8);
    }
    const float l2e = 1.44269504088896340736f, sl2e = scale * l2e;
    f32x16_t dk[NE], dv[NE];
#pragma unroll
    for (int et = 0; et < NE; ++et)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[et][r] = 0.f; dv[et][r] = 0.f; }
    const int nqt = (L + LT - 1) / LT;
    // delta = rowsum(dO * O) of the tile's queries from the dO chunks a thread stages anyway and the matching O chunks, prefetched with them (4 threads share a row)
    TileRegsH<DH> qreg, doreg, oreg;
    float lreg = 0.f;
    auto load_stats = [&](int qt_) {
        tile_load_h<DH>(oreg, obase, ldo, qt_ * LT, L, tid);
        if (tid < LT) { int qi = qt_ * LT + tid; if (qi > L - 1) qi = L - 1; lreg = lse[seq_lse_index(gm, g, h, i, qi)] * l2e; }
    };
    tile_load_h<DH>(qreg, base, ld, 0, L, tid);
    tile_load_h<DH>(doreg, dobase, ldo, 0, L, tid);
    load_stats(0);
    for (int qt = 0; qt < nqt; ++qt) {
        __syncthreads();
        tile_store_h<DH>(qreg, Qs, tid);
        tile_store_h<DH>(doreg, dOs, tid);
        {
            float d0 = tile_dot_h<DH>(doreg, oreg);
            d0 += __shfl_xor(d0, 1, 64);
            d0 += __shfl_xor(d0, 2, 64);
            if ((tid & 3) == 0) Ds[tid >> 2] = d0;
            if (tid < LT) Ls[tid] = lreg;
        }
        __syncthreads();
        if (qt + 1 < nqt) {
            tile_load_h<DH>(qreg, base, ld, (qt + 1) * LT, L, tid);
            tile_load_h<DH>(doreg, dobase, ldo, (qt + 1) * LT, L, tid);
            load_stats(qt + 1);
        }
        if (!active) continue;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int q0 = qt * LT + sub * 32;
            if (q0 >= L) break;
            f32x16_t s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = -Ds[sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi]; }
            const int off = (sub * 32 + l31) * KL + hi * 8;
#pragma unroll
            for (int t = 0; t < NK; ++t) {
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(Qs + off + t * 16), kf[t], s, 0, 0, 0);      // D[q][k]: lane = key
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(dOs + off + t * 16), vf[t], dp, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ql = sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;         // row within the tile
                s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], sl2e, -Ls[ql]));         // P
                dp[r] *= s[r];                                                     // dS / scale
            }
            if (q0 + 32 > L) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool ok = q0 + (r & 3) + 8 * (r >> 2) + 4 * hi < L;
                    s[r] = ok ? s[r] : 0.f; dp[r] = ok ? dp[r] : 0.f;
                }
            }
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const bf16x8_t pf = pack_frag(s, st), dsf = pack_frag(dp, st);
#pragma unroll
                for (int et = 0; et < NE; ++et) {
                    dv[et] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_frag_tr_rm_ld<KL>(dOs, sub * 32 + 16 * st, et * 32, lane), pf, dv[et], 0, 0, 0);    // dV^T += dO^T P
                    dk[et] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_frag_tr_rm_ld<KL>(Qs, sub * 32 + 16 * st, et * 32, lane), dsf, dk[et], 0, 0, 0);     // dK^T += Q^T dS
                }
            }
        }
    }
#pragma unroll
    for (int et = 0; et < NE; ++et)
#pragma unroll
        for (int r = 0; r < 16; ++r) dk[et][r] *= scale;
    __syncthreads();
    if (active) {
        unsigned short* patch = smem + wave * 32 * DH;
        bf16* drow0 = dqkv + (row0 + (int64_t)k0w * gm.inner) * 3 * C + h * DH;
        store_tile_lines_h<DH>(patch, drow0 + C, ld, L - k0w, dk, lane, accumulate);
        store_tile_lines_h<DH>(patch, drow0 + 2 * C, ld, L - k0w, dv, lane, accumulate);
    }
}

// ==================================================================================================
// Exact-arithmetic (VALU) variants: the tiled kernels of attn_long.hip on the same geometry, storage type T (fp32: the "exact" engine; bf16: MAED_IMPL_VALU).
// Thread per row; DH <= 64 streams 64-row tiles, wider heads 32-row tiles (two fp32 tiles of 64 x 129 would not fit 64 KB of static LDS).
// ==================================================================================================
constexpr int seq_vt(int DH) { return DH <= 64 ? 64 : 32; }

template <typename T, int DH>
__device__ __forceinline__ void stage_tile_f32_h(float* dst, const T* src, int64_t ld, int r0, int L, int tid) {
    for (int idx = tid; idx < seq_vt(DH) * (DH / 4); idx += 256) {
        const int p = idx / (DH / 4), c = (idx % (DH / 4)) * 4;
        int row = r0 + p;
        if (row > L - 1) row = L - 1;
        float v[4];
        ld4(src + (int64_t)row * ld + c, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[p * (DH + 1) + c + j] = v[j];
    }
}

template <typename T, int DH>
__device__ __forceinline__ void store_row_acc_h(T* dst, const float (&acc)[DH], int accumulate) {
#pragma unroll
    for (int c = 0; c < DH; c += 4) {
        float v[4] = {acc[c], acc[c + 1], acc[c + 2], acc[c + 3]};
        if (accumulate) { float old[4]; ld4(dst + c, old); v[0] += old[0]; v[1] += old[1]; v[2] += old[2]; v[3] += old[3]; }
        st4(dst + c, v);
    }
}

template <typename T, int DH>
__global__ __launch_bounds__(256) void attn_seq_fwd_valu(const T* __restrict__ qkv, T* __restrict__ o, float* __restrict__ lse, int seq_len, int seq_inner, int seq_heads, int ntile, float scale) {
    const SeqGeom gm{0, seq_len, seq_inner, seq_heads};
    constexpr int VTH = seq_vt(DH), VL = DH + 1;
    __shared__ float Ks[VTH * VL], Vs[VTH * VL];
    const int item = blockIdx.x / ntile, tile = blockIdx.x - item * ntile;
    const int i = item % gm.inner, gh = item / gm.inner, g = gh / gm.H, h = gh - g * gm.H;
    const int L = gm.L, C = gm.H * DH;
    const int64_t ld = 3 * (int64_t)C * gm.inner, row0 = (int64_t)g * L * gm.inner + i;
    const T* base = qkv + row0 * 3 * C + h * DH;
    const int tid = threadIdx.x, q = tile * VROWS + tid;
    const int qc = q < L ? q : L - 1;
    float qv[DH], acc[DH];
#pragma unroll
    for (int c = 0; c < DH; c += 4) { float v[4]; ld4(base + (int64_t)qc * ld + c, v); qv[c] = v[0]; qv[c + 1] = v[1]; qv[c + 2] = v[2]; qv[c + 3] = v[3]; }
#pragma unroll
    for (int c = 0; c < DH; ++c) acc[c] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < L; k0 += VTH) {
        __syncthreads();
        stage_tile_f32_h<T, DH>(Ks, base + C, ld, k0, L, tid);
        stage_tile_f32_h<T, DH>(Vs, base + 2 * C, ld, k0, L, tid);
        __syncthreads();
        const int kn = (L - k0 < VTH) ? L - k0 : VTH;
        for (int k = 0; k < kn; ++k) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < DH; ++c) s = fmaf(qv[c], Ks[k * VL + c], s);
            s *= scale;
            const float mn = fmaxf(m, s);
            const float a = __expf(m - mn), p = __expf(s - mn);
            l = l * a + p;
#pragma unroll
            for (int c = 0; c < DH; ++c) acc[c] = fmaf(p, Vs[k * VL + c], acc[c] * a);
            m = mn;
        }
    }
    if (q < L) {
        const float inv = 1.f / l;
        T* orow = o + (row0 + (int64_t)q * gm.inner) * C + h * DH;
#pragma unroll
        for (int c = 0; c < DH; c += 4) { float v[4] = {acc[c] * inv, acc[c + 1] * inv, acc[c + 2] * inv, acc[c + 3] * inv}; st4(orow + c, v); }
        lse[seq_lse_index(gm, g, h, i, q)] = m + __logf(l);
    }
}

// thread per query for DH <= 64; wider heads: TWO threads per query, each owning half of the channels (q, dO and dq rows of 3 x DH values would not fit one
// lane's registers), partial dot products joined with one shuffle.  A workgroup owns 256 / TPR rows.
constexpr int seq_dq_tpr(int DH) { return DH <= 64 ? 1 : 2; }

template <typename T, int DH>
__global__ __launch_bounds__(256) void attn_seq_bwd_dq_valu(const T* __restrict__ qkv, const T* __restrict__ o, const T* __restrict__ d_o, const float* __restrict__ lse,
                                                            T* __restrict__ dqkv, int accumulate, int seq_len, int seq_inner, int seq_heads, int ntile, float scale) {
    const SeqGeom gm{0, seq_len, seq_inner, seq_heads};
    constexpr int VTH = seq_vt(DH), VL = DH + 1, TPR = seq_dq_tpr(DH), CH = DH / TPR;
    __shared__ float Ks[VTH * VL], Vs[VTH * VL];
    const int item = blockIdx.x / ntile, tile = blockIdx.x - item * ntile;
    const int i = item % gm.inner, gh = item / gm.inner, g = gh / gm.H, h = gh - g * gm.H;
    const int L = gm.L, C = gm.H * DH;
    const int64_t ld = 3 * (int64_t)C * gm.inner, row0 = (int64_t)g * L * gm.inner + i;
    const T* base = qkv + row0 * 3 * C + h * DH;
    const int tid = threadIdx.x, q = tile * (VROWS / TPR) + tid / TPR, cofs = (tid % TPR) * CH;
    const int qc = q < L ? q : L - 1;
    const T* orow = o + (row0 + (int64_t)qc * gm.inner) * C + h * DH + cofs;
    const T* dorow = d_o + (row0 + (int64_t)qc * gm.inner) * C + h * DH + cofs;
    float qv[CH], dov[CH], dq[CH];
    float Dq = 0.f;
#pragma unroll
    for (int c = 0; c < CH; c += 4) {
        float v[4], w[4], u[4];
        ld4(base + (int64_t)qc * ld + cofs + c, v); ld4(dorow + c, w); ld4(orow + c, u);
#pragma unroll
        for (int j = 0; j < 4; ++j) { qv[c + j] = v[j]; dov[c + j] = w[j]; Dq = fmaf(w[j], u[j], Dq); dq[c + j] = 0.f; }
    }
    if constexpr (TPR == 2) Dq += __shfl_xor(Dq, 1, 64);
    const float Lq = lse[seq_lse_index(gm, g, h, i, qc)];
    for (int k0 = 0; k0 < L; k0 += VTH) {
        __syncthreads();
        stage_tile_f32_h<T, DH>(Ks, base + C, ld, k0, L, tid);
        stage_tile_f32_h<T, DH>(Vs, base + 2 * C, ld, k0, L, tid);
        __syncthreads();
        const int kn = (L - k0 < VTH) ? L - k0 : VTH;
        for (int k = 0; k < kn; ++k) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int c = 0; c < CH; ++c) { s = fmaf(qv[c], Ks[k * VL + cofs + c], s); dp = fmaf(dov[c], Vs[k * VL + cofs + c], dp); }
            if constexpr (TPR == 2) { s += __shfl_xor(s, 1, 64); dp += __shfl_xor(dp, 1, 64); }
            const float ds = __expf(s * scale - Lq) * (dp - Dq) * scale;
#pragma unroll
            for (int c = 0; c < CH; ++c) dq[c] = fmaf(ds, Ks[k * VL + cofs + c], dq[c]);
        }
    }
    if (q < L) store_row_acc_h<T, CH>(dqkv + (row0 + (int64_t)q * gm.inner) * 3 * C + h * DH + cofs, dq, accumulate);
}

// thread per key; SWEEP 0: dV[k] = sum_q p dO[q]; SWEEP 1: dK[k] = sum_q dS Q[q]  (two sweeps over the query tiles to stay in registers)
template <typename T, int DH>
__global__ __launch_bounds__(256) void attn_seq_bwd_dkv_valu(const T* __restrict__ qkv, const T* __restrict__ o, const T* __restrict__ d_o, const float* __restrict__ lse,
                                                             T* __restrict__ dqkv, int accumulate, int seq_len, int seq_inner, int seq_heads, int ntile, float scale) {
    const SeqGeom gm{0, seq_len, seq_inner, seq_heads};
    constexpr int VTH = seq_vt(DH), VL = DH + 1;
    __shared__ float Qs[VTH * VL], dOs[VTH * VL], Ls[VTH], Ds[VTH];
    const int item = blockIdx.x / ntile, tile = blockIdx.x - item * ntile;
    const int i = item % gm.inner, gh = item / gm.inner, g = gh / gm.H, h = gh - g * gm.H;
    const int L = gm.L, C = gm.H * DH;
    const int64_t ld = 3 * (int64_t)C * gm.inner, ldo = (int64_t)C * gm.inner, row0 = (int64_t)g * L * gm.inner + i;
    const T* base = qkv + row0 * 3 * C + h * DH;
    const T* obase = o + row0 * C + h * DH;
    const T* dobase = d_o + row0 * C + h * DH;
    const int tid = threadIdx.x, k = tile * VROWS + tid;
    const int kc = k < L ? k : L - 1;
    float kv[DH], vv[DH], acc[DH];
#pragma unroll
    for (int c = 0; c < DH; c += 4) {
        float a[4], b[4];
        ld4(base + C + (int64_t)kc * ld + c, a); ld4(base + 2 * C + (int64_t)kc * ld + c, b);
#pragma unroll
        for (int j = 0; j < 4; ++j) { kv[c + j] = a[j]; vv[c + j] = b[j]; }
    }
    for (int sweep = 0; sweep < 2; ++sweep) {
#pragma unroll
        for (int c = 0; c < DH; ++c) acc[c] = 0.f;
        for (int q0 = 0; q0 < L; q0 += VTH) {
            __syncthreads();
            stage_tile_f32_h<T, DH>(Qs, base, ld, q0, L, tid);
            stage_tile_f32_h<T, DH>(dOs, dobase, ldo, q0, L, tid);
            if (tid < VTH) {
                int qi = q0 + tid;
                if (qi > L - 1) qi = L - 1;
                float dsum = 0.f;
#pragma unroll
                for (int c = 0; c < DH; c += 4) {
                    float a[4], b[4];
                    ld4(dobase + (int64_t)qi * ldo + c, a); ld4(obase + (int64_t)qi * ldo + c, b);
#pragma unroll
                    for (int j = 0; j < 4; ++j) dsum = fmaf(a[j], b[j], dsum);
                }
                Ds[tid] = dsum;
                Ls[tid] = lse[seq_lse_index(gm, g, h, i, qi)];
            }
            __syncthreads();
            const int qn = (L - q0 < VTH) ? L - q0 : VTH;
            for (int qq = 0; qq < qn; ++qq) {
                float s = 0.f, dp = 0.f;
#pragma unroll
                for (int c = 0; c < DH; ++c) { s = fmaf(Qs[qq * VL + c], kv[c], s); dp = fmaf(dOs[qq * VL + c], vv[c], dp); }
                const float p = __expf(s * scale - Ls[qq]);
                const float w = sweep == 0 ? p : p * (dp - Ds[qq]) * scale;
                const float* src = sweep == 0 ? dOs + qq * VL : Qs + qq * VL;
#pragma unroll
                for (int c = 0; c < DH; ++c) acc[c] = fmaf(w, src[c], acc[c]);
            }
        }
        if (k < L) store_row_acc_h<T, DH>(dqkv + (row0 + (int64_t)k * gm.inner) * 3 * C + (sweep == 0 ? 2 * C : C) + h * DH, acc, accumulate);
    }
}

template <int DH>
int seq_fwd_launch(const void* qkv, void* o, float* lse, const SeqGeom& gm, float scale, int dtype, bool mfma, hipStream_t s) {
    const int64_t nseq = (int64_t)gm.G * gm.inner * gm.H;
    if (mfma) {
        const int ntile = (gm.L + WG_ROWS - 1) / WG_ROWS;
        MAED_CHECK_ARG(nseq * ntile < (1ll << 31), MAED_ERR_SHAPE, "attn_seq_fwd: grid too large");
        hipLaunchKernelGGL((attn_seq_fwd_mfma<DH>), dim3((unsigned)(nseq * ntile)), dim3(256), 0, s, (const bf16*)qkv, (bf16*)o, lse, gm.L, gm.inner, gm.H, ntile,
                           scale * 1.44269504088896340736f);
    } else {
        const int ntile = (gm.L + VROWS - 1) / VROWS;
        MAED_CHECK_ARG(nseq * ntile < (1ll << 31), MAED_ERR_SHAPE, "attn_seq_fwd: grid too large");
        const dim3 grid((unsigned)(nseq * ntile));
        MAED_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((attn_seq_fwd_valu<T, DH>), grid, dim3(256), 0, s, (const T*)qkv, (T*)o, lse, gm.L, gm.inner, gm.H, ntile, scale));
    }
    MAED_CHECK_LAUNCH("attn_seq_fwd");
    return MAED_OK;
}

template <int DH>
int seq_bwd_launch(const void* qkv, const void* o, const void* d_o, const float* lse, void* dqkv, int accumulate, const SeqGeom& gm, float scale, int dtype, bool mfma,
                   hipStream_t s) {
    const int64_t nseq = (int64_t)gm.G * gm.inner * gm.H;
    if (mfma) {
        const int ntile = (gm.L + WG_ROWS - 1) / WG_ROWS;
        MAED_CHECK_ARG(nseq * ntile < (1ll << 31), MAED_ERR_SHAPE, "attn_seq_bwd: grid too large");
        const dim3 grid((unsigned)(nseq * ntile));
        hipLaunchKernelGGL((attn_seq_bwd_dq_mfma<DH>), grid, dim3(256), 0, s, (const bf16*)qkv, (const bf16*)o, (const bf16*)d_o, lse, (bf16*)dqkv, accumulate, gm.L, gm.inner, gm.H, ntile,
                           scale);
        hipLaunchKernelGGL((attn_seq_bwd_dkv_mfma<DH>), grid, dim3(256), 0, s, (const bf16*)qkv, (const bf16*)o, (const bf16*)d_o, lse, (bf16*)dqkv, accumulate, gm.L, gm.inner, gm.H, ntile,
                           scale);
    } else {
        const int ntile = (gm.L + VROWS - 1) / VROWS;
        MAED_CHECK_ARG(nseq * ntile < (1ll << 31), MAED_ERR_SHAPE, "attn_seq_bwd: grid too large");
        const dim3 grid((unsigned)(nseq * ntile));
        const int ntile_q = (gm.L + VROWS / seq_dq_tpr(DH) - 1) / (VROWS / seq_dq_tpr(DH));
        MAED_CHECK_ARG(nseq * ntile_q < (1ll << 31), MAED_ERR_SHAPE, "attn_seq_bwd: grid too large");
        MAED_DISPATCH_DTYPE(dtype, T, {
            hipLaunchKernelGGL((attn_seq_bwd_dq_valu<T, DH>), dim3((unsigned)(nseq * ntile_q)), dim3(256), 0, s, (const T*)qkv, (const T*)o, (const T*)d_o, lse, (T*)dqkv,
                               accumulate, gm.L, gm.inner, gm.H, ntile_q, scale);
            hipLaunchKernelGGL((attn_seq_bwd_dkv_valu<T, DH>), grid, dim3(256), 0, s, (const T*)qkv, (const T*)o, (const T*)d_o, lse, (T*)dqkv, accumulate, gm.L, gm.inner, gm.H, ntile, scale);
        });
    }
    MAED_CHECK_LAUNCH("attn_seq_bwd");
    return MAED_OK;
}

// shared argument checks; *mfma: the engine the call takes
int seq_check(const char* who, int groups, int len, int inner, int H, int D_, int dtype, int impl, bool* mfma) {
    MAED_CHECK_ARG(groups >= 0 && len > 0 && inner > 0 && H > 0, MAED_ERR_SHAPE, "%s: bad extents (groups=%d len=%d inner=%d H=%d)", who, groups, len, inner, H);
    MAED_CHECK_ARG(D_ == 32 || D_ == 64 || D_ == 96 || D_ == 128, MAED_ERR_UNSUPPORTED, "%s: head size %d (supported: 32, 64, 96, 128)", who, D_);
    MAED_CHECK_ARG(dtype == MAED_F32 || dtype == MAED_BF16, MAED_ERR_ARG, "%s: bad dtype %d", who, dtype);
    MAED_CHECK_ARG(impl == MAED_IMPL_AUTO || impl == MAED_IMPL_VALU || impl == MAED_IMPL_MFMA_LONG, MAED_ERR_UNSUPPORTED,
                   "%s: impl %d names a kernel that exists for head size 64 only (whole-head MFMA, split-bf16 x3 / x6: maed_attn_spatial_* / maed_attn_temporal_*); "
                   "this entry point takes MAED_IMPL_AUTO, MAED_IMPL_VALU or MAED_IMPL_MFMA_LONG", who, impl);
    MAED_CHECK_ARG(!(impl == MAED_IMPL_MFMA_LONG && dtype != MAED_BF16), MAED_ERR_UNSUPPORTED, "%s: the MFMA kernels need bf16", who);
    *mfma = dtype == MAED_BF16 && impl != MAED_IMPL_VALU;       // fp32 always runs the exact kernels here, whatever MAED_OPT_F32_MATMUL says
    return MAED_OK;
}

}  // namespace

extern "C" int maed_attn_seq_fwd(const void* qkv, void* o, float* lse, int groups, int len, int inner, int H, int head_dim, float scale, int dtype, int impl,
                                 void* stream) {
    MAED_CHECK_ARG(qkv && o && lse, MAED_ERR_ARG, "attn_seq_fwd: null pointer");
    MAED_CHECK_ARG(is_aligned(qkv, 16) && is_aligned(o, 16), MAED_ERR_ALIGN, "attn_seq_fwd: qkv/o must be 16-B aligned");
    bool mfma = false;
    MAED_PROPAGATE(seq_check("attn_seq_fwd", groups, len, inner, H, head_dim, dtype, impl, &mfma));
    if (groups == 0) return MAED_OK;
    const SeqGeom gm{groups, len, inner, H};
    hipStream_t s = (hipStream_t)stream;
    switch (head_dim) {
        case 32: return seq_fwd_launch<32>(qkv, o, lse, gm, scale, dtype, mfma, s);
        case 64: return seq_fwd_launch<64>(qkv, o, lse, gm, scale, dtype, mfma, s);
        case 96: return seq_fwd_launch<96>(qkv, o, lse, gm, scale, dtype, mfma, s);
        default: return seq_fwd_launch<128>(qkv, o, lse, gm, scale, dtype, mfma, s);
    }
}

extern "C" int maed_attn_seq_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, void* dqkv, int accumulate, int groups, int len, int inner, int H,
                                 int head_dim, float scale, int dtype, int impl, void* stream) {
    MAED_CHECK_ARG(qkv && o && d_o && lse && dqkv, MAED_ERR_ARG, "attn_seq_bwd: null pointer");
    MAED_CHECK_ARG(is_aligned(qkv, 16) && is_aligned(o, 16) && is_aligned(d_o, 16) && is_aligned(dqkv, 16), MAED_ERR_ALIGN, "attn_seq_bwd: tensors must be 16-B aligned");
    bool mfma = false;
    MAED_PROPAGATE(seq_check("attn_seq_bwd", groups, len, inner, H, head_dim, dtype, impl, &mfma));
    if (groups == 0) return MAED_OK;
    const SeqGeom gm{groups, len, inner, H};
    hipStream_t s = (hipStream_t)stream;
    switch (head_dim) {
        case 32: return seq_bwd_launch<32>(qkv, o, d_o, lse, dqkv, accumulate, gm, scale, dtype, mfma, s);
        case 64: return seq_bwd_launch<64>(qkv, o, d_o, lse, dqkv, accumulate, gm, scale, dtype, mfma, s);
        case 96: return seq_bwd_launch<96>(qkv, o, d_o, lse, dqkv, accumulate, gm, scale, dtype, mfma, s);
        default: return seq_bwd_launch<128>(qkv, o, d_o, lse, dqkv, accumulate, gm, scale, dtype, mfma, s);
    }
}
