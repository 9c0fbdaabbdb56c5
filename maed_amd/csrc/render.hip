// Mesh overlay on the device (reference: lib/utils/renderer.py Renderer.render, which is pyrender on OpenGL -- an Instinct accelerator has no graphics
// pipeline, so this is a compute rasteriser): a batch of triangle meshes that share one face list -> z-buffered, shaded, composited over uint8 frames.
// Definitions, derivations and measurements: docs/design/11_render.md.  The numpy restatement is tests/_render_ref.py.
//
//   vertex    rotate (x, -y, -z) [renderer.py:78-79], optional 3 x 3 rotation [:84-86], weak-perspective projection [:31-38], snap to 1/256 px
//   normal    per vertex: normalised sum of the (area-weighted) normals of its faces, gathered through a vertex -> face CSR in face order (deterministic)
//   raster    per triangle: back-face cull, 64-bit integer edge functions with a top-left rule, fp32 depth from the integer weights, |ndc_z| <= 1,
//             one 64-bit atomicMin per covered pixel into the visibility buffer: (order-preserving depth bits << 32) | face index
//   resolve   per pixel: winner's weights again (same integers, same fp32 operations), shade, wireframe test, composite over the frame
//
// Coverage and the visible face are functions of integers and of single correctly rounded fp32 operations in a fixed order, and the minimum over 64-bit keys
// does not depend on the order of arrival: the result is the same bits for every launch geometry and every form.
// Forms of the raster pass:
//   LANE   every triangle on one lane (the bounding-box loop of a large triangle then holds its whole wave)
//   SPLIT  triangles whose clamped bounding box has at most RENDER_SMALL_BOX pixel centres on one lane; the others are appended to a queue (one vector atomic add
//          each) and a second launch gives each of them a workgroup.  The automatic choice.
// Only vector atomics (global_atomic_umin_x2, global_atomic_add) and plain stores are used.
#include "common.cuh"
#ifdef MAED_HOSTSIM
#include "render_support.h"
#endif

// projection, snapping and depth are restated in numpy operation by operation: no fused multiply-add may replace a multiply and an add
#pragma clang fp contract(off)

namespace {

enum { FORM_AUTO = 0, FORM_LANE = 1, FORM_SPLIT = 2 };
constexpr int RENDER_MAX_DIM = 16384;                 // viewport limit: pixel centres * 256 stay below 2^23, every edge-function product below 2^62
constexpr float RENDER_COORD_CLAMP = 1073741824.0f;   // 2^30 sub-pixel units: snapped vertex coordinates are clamped here (4 194 304 px from the origin)
constexpr int RENDER_SMALL_BOX = 256;                 // SPLIT form: bounding boxes up to this many pixel centres stay on a lane
constexpr unsigned long long RENDER_EMPTY = ~0ull;
#ifdef MAED_HOSTSIM
constexpr int RENDER_THREADS = 64;                    // one host thread per lane: small workgroups, few of them, grid-stride loops do the rest
constexpr int RENDER_MAX_GRID = 4;
#else
constexpr int RENDER_THREADS = 256;
constexpr int RENDER_MAX_GRID = 1 << 20;
#endif
constexpr int RENDER_LARGE_GRID = RENDER_MAX_GRID < 2048 ? RENDER_MAX_GRID : 2048;

struct alignas(16) ProjV { int X, Y; float z; int ok; };        // snapped window position (1/256 px, y down), ndc_z, finite flag
struct alignas(16) Vec4 { float x, y, z, w; };

struct Shade { float base[3]; float wire_px; int wireframe; };

// ---- vertex pass ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RENDER_THREADS) void render_vertex_kernel(const float* __restrict__ verts, const float* __restrict__ cam, const float* __restrict__ rot,
                                                                       int B, int V, int H, int W, ProjV* __restrict__ pv, Vec4* __restrict__ pos) {
    const int64_t n = (int64_t)B * V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / V);
        const float* v = verts + i * 3;
        float X = v[0], Y = -v[1], Z = -v[2];
        if (rot) {
            const float* r = rot + (size_t)b * 9;
            const float x0 = X, y0 = Y, z0 = Z;
            X = (r[0] * x0 + r[1] * y0) + r[2] * z0;
            Y = (r[3] * x0 + r[4] * y0) + r[5] * z0;
            Z = (r[6] * x0 + r[7] * y0) + r[8] * z0;
        }
        const float sx = cam[b * 4 + 0], sy = cam[b * 4 + 1], tx = cam[b * 4 + 2], ty = cam[b * 4 + 3];
        const float ndx = sx * (X + tx);
        const float ndy = sy * (Y - ty);
        const float ndz = -Z + 0.0f;                                       // (+ 0: one zero only, so equal depths have equal keys)
        const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
        float fx = ((ndx + 1.0f) * hw) * 256.0f;
        float fy = ((1.0f - ndy) * hh) * 256.0f;
        const float big = 3.4028234e38f;
        const int ok = (fabsf(fx) <= big) && (fabsf(fy) <= big) && (fabsf(ndz) <= big);      // false for NaN and infinity
        fx = fminf(fmaxf(fx, -RENDER_COORD_CLAMP), RENDER_COORD_CLAMP);
        fy = fminf(fmaxf(fy, -RENDER_COORD_CLAMP), RENDER_COORD_CLAMP);
        ProjV p;
        p.X = ok ? (int)rintf(fx) : 0;
        p.Y = ok ? (int)rintf(fy) : 0;
        p.z = ndz;
        p.ok = ok;
        pv[i] = p;
        pos[i] = Vec4{X, Y, Z, 0.f};
    }
}

// ---- vertex normals: CSR gather, faces of a vertex in ascending face order ---------------------------------------------------------
__global__ __launch_bounds__(RENDER_THREADS) void render_normal_kernel(const Vec4* __restrict__ pos, const int* __restrict__ faces, const int* __restrict__ vf_off,
                                                                       const int* __restrict__ vf_idx, int B, int V, int n_faces, Vec4* __restrict__ nrm) {
    const int64_t n = (int64_t)B * V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / V), v = (int)(i - (int64_t)b * V);
        const Vec4* P = pos + (size_t)b * V;
        int k0 = vf_off[v], k1 = vf_off[v + 1];
        k0 = max(0, min(k0, 3 * n_faces));
        k1 = max(k0, min(k1, 3 * n_faces));
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (int k = k0; k < k1; ++k) {
            const int f = vf_idx[k];
            if ((unsigned)f >= (unsigned)n_faces) continue;
            const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
            if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) continue;
            const Vec4 a = P[i0], c1 = P[i1], c2 = P[i2];
            const float ux = c1.x - a.x, uy = c1.y - a.y, uz = c1.z - a.z;
            const float wx = c2.x - a.x, wy = c2.y - a.y, wz = c2.z - a.z;
            sx += uy * wz - uz * wy;
            sy += uz * wx - ux * wz;
            sz += ux * wy - uy * wx;
        }
        const float len = sqrtf((sx * sx + sy * sy) + sz * sz);
        const float inv = len > 0.f ? 1.0f / len : 0.f;
        nrm[i] = Vec4{sx * inv, sy * inv, sz * inv, 0.f};
    }
}

// ---- the triangle ----------------------------------------------------------------------------------------------------------------
// Edge i runs from vertex (i+1)%3 to vertex (i+2)%3.  w_i(P) = dy_i (Px - ax_i) - dx_i (Py - ay_i) in 1/256 px units is >= 0 inside a front face (clockwise in
// the y-down image = counter-clockwise in GL window coordinates) and the three sum to A = twice the area > 0.  A sample exactly on an edge (w_i = 0) belongs to
// the triangle when the edge is a left edge (dy > 0: w grows with x) or a top edge (dy = 0 and dx < 0: w grows with y); bias_i is 0 there and -1 elsewhere.
struct Tri {
    int ax[3], ay[3], dx[3], dy[3], bias[3];
    float z[3];
    int64_t A;
    int x0, x1, y0, y1;                                // clamped bounding box of pixel centres (inclusive)
};

__device__ __forceinline__ bool tri_setup(const ProjV& p0, const ProjV& p1, const ProjV& p2, int H, int W, Tri& t) {
    if (!(p0.ok && p1.ok && p2.ok)) return false;
    const int X[3] = {p0.X, p1.X, p2.X}, Y[3] = {p0.Y, p1.Y, p2.Y};
    const int64_t area2 = (int64_t)(X[1] - X[0]) * (int64_t)(Y[2] - Y[0]) - (int64_t)(X[2] - X[0]) * (int64_t)(Y[1] - Y[0]);
    t.A = -area2;
    if (t.A <= 0) return false;                        // back face or no area
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        t.ax[i] = X[a]; t.ay[i] = Y[a];
        t.dx[i] = X[b] - X[a]; t.dy[i] = Y[b] - Y[a];
        t.bias[i] = (t.dy[i] > 0 || (t.dy[i] == 0 && t.dx[i] < 0)) ? 0 : -1;
    }
    t.z[0] = p0.z; t.z[1] = p1.z; t.z[2] = p2.z;
    const int xmin = min(X[0], min(X[1], X[2])), xmax = max(X[0], max(X[1], X[2]));
    const int ymin = min(Y[0], min(Y[1], Y[2])), ymax = max(Y[0], max(Y[1], Y[2]));
    t.x0 = max(0, (xmin + 127) >> 8);                  // first pixel whose centre 256 i + 128 is >= xmin
    t.x1 = min(W - 1, (xmax - 128) >> 8);              // last pixel whose centre is <= xmax
    t.y0 = max(0, (ymin + 127) >> 8);
    t.y1 = min(H - 1, (ymax - 128) >> 8);
    return t.x0 <= t.x1 && t.y0 <= t.y1;
}

__device__ __forceinline__ int64_t edge_at(const Tri& t, int i, int Px, int Py) {
    return (int64_t)t.dy[i] * (int64_t)(Px - t.ax[i]) - (int64_t)t.dx[i] * (int64_t)(Py - t.ay[i]);
}

// ndc_z at a sample from the integer weights: three correctly rounded quotients, then (l0 z0 + l1 z1) + l2 z2
__device__ __forceinline__ float depth_at(const Tri& t, int64_t w0, int64_t w1, int64_t w2, float& l0, float& l1, float& l2) {
    const float fA = (float)t.A;
    l0 = (float)w0 / fA; l1 = (float)w1 / fA; l2 = (float)w2 / fA;
    return ((l0 * t.z[0] + l1 * t.z[1]) + l2 * t.z[2]) + 0.0f;
}

__device__ __forceinline__ unsigned long long depth_key(float z, int face) {
    const uint32_t u = __float_as_uint(z);
    const uint32_t ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)ord << 32) | (unsigned long long)(uint32_t)face;
}
__device__ __forceinline__ float key_depth(unsigned long long key) {
    const uint32_t ord = (uint32_t)(key >> 32);
    return __uint_as_float((ord & 0x80000000u) ? (ord & 0x7fffffffu) : ~ord);
}

__device__ __forceinline__ void fragment(const Tri& t, int64_t w0, int64_t w1, int64_t w2, int face, unsigned long long* __restrict__ cell) {
    if ((w0 + t.bias[0]) < 0 || (w1 + t.bias[1]) < 0 || (w2 + t.bias[2]) < 0) return;
    float l0, l1, l2;
    const float z = depth_at(t, w0, w1, w2, l0, l1, l2);
    if (!(fabsf(z) <= 1.0f)) return;                   // GL clip volume (also drops NaN)
    atomicMin(cell, depth_key(z, face));
}

__device__ __forceinline__ bool load_tri(const int* __restrict__ faces, const ProjV* __restrict__ pv, int f, int V, int H, int W, Tri& t, bool& bad) {
    const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    bad = (unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V;
    if (bad) return false;                             // (never an unchecked gather)
    return tri_setup(pv[i0], pv[i1], pv[i2], H, W, t);
}

// ---- raster, one triangle per lane; split != 0: boxes above RENDER_SMALL_BOX go to the queue instead ------------------------------------
__global__ __launch_bounds__(RENDER_THREADS) void render_raster_lane_kernel(const int* __restrict__ faces, const ProjV* __restrict__ pv, int B, int V, int n_faces, int H,
                                                                            int W, int split, unsigned long long* __restrict__ vis, unsigned* __restrict__ counters,
                                                                            int* __restrict__ queue) {
    const int64_t n = (int64_t)B * n_faces;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / n_faces), f = (int)(i - (int64_t)b * n_faces);
        Tri t;
        bool bad;
        if (!load_tri(faces, pv + (size_t)b * V, f, V, H, W, t, bad)) {
            if (bad && b == 0) atomicAdd(counters + 1, 1u);
            continue;
        }
        if (split && (int64_t)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) > RENDER_SMALL_BOX) {
            queue[atomicAdd(counters, 1u)] = (int)i;   // (at most B * n_faces entries: the queue's size)
            continue;
        }
        unsigned long long* frame = vis + (size_t)b * H * W;
        const int Px0 = t.x0 * 256 + 128;
        const int64_t s0 = (int64_t)t.dy[0] * 256, s1 = (int64_t)t.dy[1] * 256, s2 = (int64_t)t.dy[2] * 256;
        for (int y = t.y0; y <= t.y1; ++y) {
            const int Py = y * 256 + 128;
            int64_t w0 = edge_at(t, 0, Px0, Py), w1 = edge_at(t, 1, Px0, Py), w2 = edge_at(t, 2, Px0, Py);
            for (int x = t.x0; x <= t.x1; ++x) {
                fragment(t, w0, w1, w2, f, frame + (size_t)y * W + x);
                w0 += s0; w1 += s1; w2 += s2;          // (exact: integers)
            }
        }
    }
}

// ---- raster, one queued triangle per workgroup -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(RENDER_THREADS) void render_raster_large_kernel(const int* __restrict__ faces, const ProjV* __restrict__ pv, int B, int V, int n_faces, int H,
                                                                             int W, unsigned long long* __restrict__ vis, const unsigned* __restrict__ counters,
                                                                             const int* __restrict__ queue) {
    const unsigned count = min((int64_t)counters[0], (int64_t)B * n_faces);
    for (unsigned q = blockIdx.x; q < count; q += gridDim.x) {
        const int i = queue[q];
        if ((unsigned)i >= (unsigned)(B * n_faces)) continue;
        const int b = i / n_faces, f = i - b * n_faces;
        Tri t;
        bool bad;
        if (!load_tri(faces, pv + (size_t)b * V, f, V, H, W, t, bad)) continue;
        unsigned long long* frame = vis + (size_t)b * H * W;
        const int bw = t.x1 - t.x0 + 1;
        const int64_t np = (int64_t)bw * (t.y1 - t.y0 + 1);
        for (int64_t p = threadIdx.x; p < np; p += blockDim.x) {
            const int yy = (int)(p / bw), x = t.x0 + (int)(p - (int64_t)yy * bw), y = t.y0 + yy;
            const int Px = x * 256 + 128, Py = y * 256 + 128;
            fragment(t, edge_at(t, 0, Px, Py), edge_at(t, 1, Px, Py), edge_at(t, 2, Px, Py), f, frame + (size_t)y * W + x);
        }
    }
}

// ---- resolve: shade the winner, composite ---------------------------------------------------------------------------------------------
// colour = base * (0.3 + g * sum_i max(0, n . l_i)), lights at (0,-1,1), (0,1,1), (1,1,2) in the camera frame (renderer.py:55-67), g = RENDER_LIGHT_GAIN
constexpr float RENDER_AMBIENT = 0.3f, RENDER_LIGHT_GAIN = 0.3f;

struct Px { int covered; int face; float depth; uint8_t rgb[3]; int draw; };

__device__ inline Px resolve_pixel(unsigned long long key, int b, int x, int y, const int* __restrict__ faces, const ProjV* __restrict__ pv, const Vec4* __restrict__ pos,
                                   const Vec4* __restrict__ nrm, int V, int n_faces, int H, int W, const Shade& sh, bool want_colour) {
    Px o;
    o.covered = 0; o.face = -1; o.depth = __uint_as_float(0x7f800000u); o.draw = 0; o.rgb[0] = o.rgb[1] = o.rgb[2] = 0;
    if (key == RENDER_EMPTY) return o;
    const int f = (int)(uint32_t)key;
    if ((unsigned)f >= (unsigned)n_faces) return o;
    const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return o;
    const size_t vb = (size_t)b * V;
    Tri t;
    if (!tri_setup(pv[vb + i0], pv[vb + i1], pv[vb + i2], H, W, t)) return o;
    o.covered = 1; o.face = f; o.depth = key_depth(key); o.draw = 1;
    if (!want_colour) return o;
    const int Px_ = x * 256 + 128, Py_ = y * 256 + 128;
    const int64_t w0 = edge_at(t, 0, Px_, Py_), w1 = edge_at(t, 1, Px_, Py_), w2 = edge_at(t, 2, Px_, Py_);
    float l0, l1, l2;
    (void)depth_at(t, w0, w1, w2, l0, l1, l2);
    if (sh.wireframe) {
        const int64_t w[3] = {w0, w1, w2};
        float dmin = 3.4028234e38f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int64_t len2 = (int64_t)t.dx[i] * t.dx[i] + (int64_t)t.dy[i] * t.dy[i];
            dmin = fminf(dmin, (float)w[i] / (sqrtf((float)len2) * 256.0f));
        }
        if (!(dmin <= sh.wire_px)) { o.draw = 0; return o; }
    }
    const Vec4 n0 = nrm[vb + i0], n1 = nrm[vb + i1], n2 = nrm[vb + i2];
    const Vec4 p0 = pos[vb + i0], p1 = pos[vb + i1], p2 = pos[vb + i2];
    float nx = l0 * n0.x + l1 * n1.x + l2 * n2.x, ny = l0 * n0.y + l1 * n1.y + l2 * n2.y, nz = l0 * n0.z + l1 * n1.z + l2 * n2.z;
    const float nl = sqrtf(nx * nx + ny * ny + nz * nz);
    const float ninv = nl > 0.f ? 1.0f / nl : 0.f;
    nx *= ninv; ny *= ninv; nz *= ninv;
    const float px = l0 * p0.x + l1 * p1.x + l2 * p2.x, py = l0 * p0.y + l1 * p1.y + l2 * p2.y, pz = l0 * p0.z + l1 * p1.z + l2 * p2.z;
    const float L[3][3] = {{0.f, -1.f, 1.f}, {0.f, 1.f, 1.f}, {1.f, 1.f, 2.f}};
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float lx = L[i][0] - px, ly = L[i][1] - py, lz = L[i][2] - pz;
        const float ll = sqrtf(lx * lx + ly * ly + lz * lz);
        const float d = ll > 0.f ? (nx * lx + ny * ly + nz * lz) / ll : 0.f;
        sum += fmaxf(d, 0.f);
    }
    const float lum = RENDER_AMBIENT + RENDER_LIGHT_GAIN * sum;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = fminf(fmaxf(sh.base[c] * lum, 0.f), 1.f);
        o.rgb[c] = (uint8_t)(int)(v * 255.0f);
    }
    return o;
}

// A thread owns four consecutive pixels of the flattened (B * H * W) batch = 12 bytes of frame = three aligned dwords; the last n % 4 pixels go bytewise.
__global__ __launch_bounds__(RENDER_THREADS) void render_resolve_kernel(const unsigned long long* __restrict__ vis, const int* __restrict__ faces, const ProjV* __restrict__ pv,
                                                                        const Vec4* __restrict__ pos, const Vec4* __restrict__ nrm, const uint8_t* frames_in,
                                                                        uint8_t* out, int* __restrict__ face_id, float* __restrict__ depth, int B, int V, int n_faces,
                                                                        int H, int W, Shade sh) {
    const int64_t n = (int64_t)B * H * W, nq = (n + 3) / 4, hw = (int64_t)H * W;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t first = q * 4;
        const int cnt = (int)min((int64_t)4, n - first);
        uint8_t bytes[12];
        if (out) {
            if (frames_in && cnt == 4) {
                const uint32_t* s = reinterpret_cast<const uint32_t*>(frames_in + first * 3);
                const uint32_t a = s[0], c = s[1], d = s[2];
#pragma unroll
                for (int k = 0; k < 4; ++k) { bytes[k] = (uint8_t)(a >> (8 * k)); bytes[4 + k] = (uint8_t)(c >> (8 * k)); bytes[8 + k] = (uint8_t)(d >> (8 * k)); }
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k) bytes[k] = (frames_in && k < cnt * 3) ? frames_in[first * 3 + k] : (uint8_t)0;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= cnt) break;
            const int64_t i = first + k;
            const int b = (int)(i / hw);
            const int64_t r = i - (int64_t)b * hw;
            const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
            const Px o = resolve_pixel(vis[i], b, x, y, faces, pv, pos, nrm, V, n_faces, H, W, sh, out != nullptr);
            if (face_id) face_id[i] = o.face;
            if (depth) depth[i] = o.depth;
            if (o.draw) { bytes[3 * k] = o.rgb[0]; bytes[3 * k + 1] = o.rgb[1]; bytes[3 * k + 2] = o.rgb[2]; }
        }
        if (out) {
            if (cnt == 4) {
                uint32_t* d = reinterpret_cast<uint32_t*>(out + first * 3);
                uint32_t wv[3];
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    wv[j] = (uint32_t)bytes[4 * j] | ((uint32_t)bytes[4 * j + 1] << 8) | ((uint32_t)bytes[4 * j + 2] << 16) | ((uint32_t)bytes[4 * j + 3] << 24);
                d[0] = wv[0]; d[1] = wv[1]; d[2] = wv[2];
            } else {
                for (int k = 0; k < cnt * 3; ++k) out[first * 3 + k] = bytes[k];
            }
        }
    }
}

inline size_t up256(size_t n) { return (n + 255) / 256 * 256; }
struct Layout { size_t vis, pv, pos, nrm, counters, queue, total; };
inline Layout layout(int B, int V, int n_faces, int H, int W) {
    Layout l;
    size_t at = 0;
    l.vis = at; at += up256((size_t)B * H * W * 8);
    l.pv = at; at += up256((size_t)B * V * sizeof(ProjV));
    l.pos = at; at += up256((size_t)B * V * sizeof(Vec4));
    l.nrm = at; at += up256((size_t)B * V * sizeof(Vec4));
    l.counters = at; at += 256;
    l.queue = at; at += up256((size_t)B * n_faces * 4);
    l.total = at;
    return l;
}
inline int grid_for(int64_t items) { return (int)max((int64_t)1, min((int64_t)RENDER_MAX_GRID, (items + RENDER_THREADS - 1) / RENDER_THREADS)); }

}  // namespace

extern "C" size_t maed_render_mesh_workspace(int B, int V, int n_faces, int H, int W, int flags) {
    (void)flags;
    if (B <= 0 || V <= 0 || n_faces <= 0 || H <= 0 || W <= 0) return 0;
    return layout(B, V, n_faces, H, W).total;
}

extern "C" int maed_render_mesh(const float* verts, const int32_t* faces, const int32_t* faces_host, const int32_t* vf_off, const int32_t* vf_idx, const float* cam,
                                const float* rot, const uint8_t* frames_in, uint8_t* out, int32_t* face_id, float* depth, int B, int V, int n_faces, int H, int W,
                                const float* base_host, float wire_px, int flags, void* workspace, size_t workspace_bytes, void* stream) {
    MAED_CHECK_ARG(B > 0 && V > 0 && n_faces > 0 && H > 0 && W > 0, MAED_ERR_SHAPE, "render_mesh: sizes must be positive (B %d, V %d, faces %d, viewport %d x %d)", B, V,
                   n_faces, W, H);
    MAED_CHECK_ARG(H <= RENDER_MAX_DIM && W <= RENDER_MAX_DIM, MAED_ERR_SHAPE,
                   "render_mesh: viewport %d x %d is too large (at most %d in each direction: sub-pixel coordinates have 8 fractional bits and edge functions 64)", W, H,
                   RENDER_MAX_DIM);
    MAED_CHECK_ARG((int64_t)B * H * W < ((int64_t)1 << 31) && (int64_t)B * n_faces < ((int64_t)1 << 31) && (int64_t)B * V < ((int64_t)1 << 31), MAED_ERR_SHAPE,
                   "render_mesh: batch too large (pixels, faces and vertices of a call are counted in 31 bits)");
    MAED_CHECK_ARG(verts && faces && cam, MAED_ERR_ARG, "render_mesh: null pointer");
    MAED_CHECK_ARG(out || face_id || depth, MAED_ERR_ARG, "render_mesh: no output requested");
    MAED_CHECK_ARG(!out || (vf_off && vf_idx && base_host), MAED_ERR_ARG, "render_mesh: a colour output needs the vertex -> face CSR and the base colour");
    MAED_CHECK_ARG(!out || (is_aligned(out, 4) && (!frames_in || is_aligned(frames_in, 4))), MAED_ERR_ALIGN, "render_mesh: frames must be 4-byte aligned");
    const int form_in = (flags & MAED_RENDER_FORM_MASK) >> MAED_RENDER_FORM_SHIFT;
    MAED_CHECK_ARG(form_in >= FORM_AUTO && form_in <= FORM_SPLIT, MAED_ERR_ARG, "render_mesh: form %d", form_in);
    const int wireframe = (flags & MAED_RENDER_WIREFRAME) != 0;
    MAED_CHECK_ARG(!wireframe || (wire_px >= 0.f && wire_px <= 1024.f), MAED_ERR_ARG, "render_mesh: wireframe distance %g px", (double)wire_px);
    if (faces_host)
        for (int64_t i = 0; i < (int64_t)n_faces * 3; ++i)
            MAED_CHECK_ARG((uint32_t)faces_host[i] < (uint32_t)V, MAED_ERR_ARG, "render_mesh: face %lld has vertex index %d outside [0, %d)", (long long)(i / 3),
                           (int)faces_host[i], V);
    const Layout l = layout(B, V, n_faces, H, W);
    MAED_CHECK_ARG(workspace && workspace_bytes >= l.total, MAED_ERR_ARG, "render_mesh: needs %zu bytes of workspace", l.total);
    MAED_CHECK_ARG(is_aligned(workspace, 16), MAED_ERR_ALIGN, "render_mesh: workspace must be 16-byte aligned");
    char* ws = (char*)workspace;
    unsigned long long* vis = (unsigned long long*)(ws + l.vis);
    ProjV* pv = (ProjV*)(ws + l.pv);
    Vec4* pos = (Vec4*)(ws + l.pos);
    Vec4* nrm = (Vec4*)(ws + l.nrm);
    unsigned* counters = (unsigned*)(ws + l.counters);
    int* queue = (int*)(ws + l.queue);
    hipStream_t st = (hipStream_t)stream;
    // measured (profiles/render_micro.txt): see docs/design/11_render.md for the choice of the automatic form
    const int form = form_in == FORM_AUTO ? FORM_SPLIT : form_in;
    const dim3 blk(RENDER_THREADS);
    MAED_HIP(hipMemsetAsync(vis, 0xFF, (size_t)B * H * W * 8, st), "render_mesh");
    MAED_HIP(hipMemsetAsync(counters, 0, 256, st), "render_mesh");
    hipLaunchKernelGGL(render_vertex_kernel, dim3(grid_for((int64_t)B * V)), blk, 0, st, verts, cam, rot, B, V, H, W, pv, pos);
    if (out && !(flags & MAED_RENDER_RASTER_ONLY))
        hipLaunchKernelGGL(render_normal_kernel, dim3(grid_for((int64_t)B * V)), blk, 0, st, (const Vec4*)pos, faces, vf_off, vf_idx, B, V, n_faces, nrm);
    hipLaunchKernelGGL(render_raster_lane_kernel, dim3(grid_for((int64_t)B * n_faces)), blk, 0, st, faces, (const ProjV*)pv, B, V, n_faces, H, W, (int)(form == FORM_SPLIT), vis,
                       counters, queue);
    if (form == FORM_SPLIT)
        hipLaunchKernelGGL(render_raster_large_kernel, dim3(RENDER_LARGE_GRID), blk, 0, st, faces, (const ProjV*)pv, B, V, n_faces, H, W, vis, (const unsigned*)counters,
                           (const int*)queue);
    if (!(flags & MAED_RENDER_RASTER_ONLY)) {
        Shade sh;
        for (int c = 0; c < 3; ++c) sh.base[c] = base_host ? base_host[c] : 1.0f;
        sh.wire_px = wire_px;
        sh.wireframe = wireframe;
        hipLaunchKernelGGL(render_resolve_kernel, dim3(grid_for(((int64_t)B * H * W + 3) / 4)), blk, 0, st, (const unsigned long long*)vis, faces, (const ProjV*)pv,
                           (const Vec4*)pos, (const Vec4*)nrm, frames_in, out, face_id, depth, B, V, n_faces, H, W, sh);
    }
    MAED_CHECK_LAUNCH("render_mesh");
    return MAED_OK;
}
