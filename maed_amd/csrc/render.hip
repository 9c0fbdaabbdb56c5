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
//
// Many meshes per frame (maed_render_people): the same passes over M meshes and ONE visibility buffer of B frames; every kernel below is a template over how a mesh
// finds its frame and how a fragment becomes a 64-bit key (OneMesh: the layout above; Layered: the painter and the shared-depth layouts, see the struct).
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
constexpr int RENDER_MAX_FACES = 1 << 24;             // many meshes per frame: the key holds 24 bits of face index and 8 bits of layer
constexpr int RENDER_MAX_LAYERS = 255;
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

// order-preserving bits of a float: unsigned comparison of ord32(a), ord32(b) is the comparison of a, b
__device__ __forceinline__ uint32_t ord32(float z) {
    const uint32_t u = __float_as_uint(z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord32_depth(uint32_t ord) { return __uint_as_float((ord & 0x80000000u) ? (ord & 0x7fffffffu) : ~ord); }

// ---- how a mesh finds its frame and a fragment its key ------------------------------------------------------------------------------------
// A mode gives, per mesh, a Ctx {frame, key(z, face)} for the raster pass and, per pixel, decode(key, frame) -> mesh, face, depth for the resolve pass.
struct Winner { int mesh, face; float depth; };

// one mesh per frame: mesh b draws into frame b;  key = (ord32(z) << 32) | face
struct OneMesh {
    int unused;
    struct Ctx {
        int frame;
        __device__ __forceinline__ unsigned long long key(float z, int face) const { return ((unsigned long long)ord32(z) << 32) | (unsigned long long)(uint32_t)face; }
    };
    __device__ __forceinline__ Ctx ctx(int m) const { return Ctx{m}; }
    __device__ __forceinline__ bool decode(unsigned long long key, int b, Winner& w) const {
        w.mesh = b; w.face = (int)(uint32_t)key; w.depth = ord32_depth((uint32_t)(key >> 32));
        return true;
    }
    __device__ __forceinline__ const float* base(int, const float* shade_base) const { return shade_base; }
    __device__ __forceinline__ void put_mesh(int64_t, int) const {}
};

// many meshes per frame: first (B + 1) is the frame -> first mesh table, mesh_frame (M) its inverse; the layer of mesh m is m - first[mesh_frame[m]] (< 255).
//   painter       key = ((255 - layer) << 56) | (ord32(z) << 24) | face        the highest layer that covers the pixel, then the nearest fragment, then the lowest face
//   shared depth  key = (ord32(z + zoff[m]) << 32) | (layer << 24) | face      the nearest fragment of all meshes, then the lowest layer, then the lowest face
// No key equals RENDER_EMPTY: faces are below 2^24 - 1 and layers below 255.
struct Layered {
    const int* first;
    const int* mesh_frame;
    const float* zoff;                                 // (M) or null; shared depth only
    const float* colour;                               // (M, 3)
    int* mesh_id;                                      // (B, H, W) or null
    int shared;
    struct Ctx {
        int frame;
        uint32_t layer;
        float zoff;
        int shared;
        __device__ __forceinline__ unsigned long long key(float z, int face) const {
            if (shared) return ((unsigned long long)ord32(z + zoff) << 32) | (unsigned long long)((layer << 24) | (uint32_t)face);
            return ((unsigned long long)(255u - layer) << 56) | ((unsigned long long)ord32(z) << 24) | (unsigned long long)(uint32_t)face;
        }
    };
    __device__ __forceinline__ Ctx ctx(int m) const {
        const int b = mesh_frame[m];
        return Ctx{b, (uint32_t)(m - first[b]) & 0xffu, (shared && zoff) ? zoff[m] : 0.0f, shared};
    }
    __device__ __forceinline__ bool decode(unsigned long long key, int b, Winner& w) const {
        uint32_t layer, ord;
        if (shared) { ord = (uint32_t)(key >> 32); layer = (uint32_t)(key >> 24) & 0xffu; }
        else { ord = (uint32_t)(key >> 24); layer = 255u - (uint32_t)(key >> 56); }
        const int m0 = first[b];
        if ((int)layer >= first[b + 1] - m0) return false;         // (never a gather through a layer the frame does not have)
        w.mesh = m0 + (int)layer; w.face = (int)((uint32_t)key & 0xffffffu); w.depth = ord32_depth(ord);
        return true;
    }
    __device__ __forceinline__ const float* base(int m, const float*) const { return colour + (size_t)m * 3; }
    __device__ __forceinline__ void put_mesh(int64_t i, int m) const { if (mesh_id) mesh_id[i] = m; }
};

template <class Ctx>
__device__ __forceinline__ void fragment(const Tri& t, int64_t w0, int64_t w1, int64_t w2, int face, unsigned long long* __restrict__ cell, const Ctx& c) {
    if ((w0 + t.bias[0]) < 0 || (w1 + t.bias[1]) < 0 || (w2 + t.bias[2]) < 0) return;
    float l0, l1, l2;
    const float z = depth_at(t, w0, w1, w2, l0, l1, l2);
    if (!(fabsf(z) <= 1.0f)) return;                   // GL clip volume (also drops NaN); a mesh's depth offset is added after it
    atomicMin(cell, c.key(z, face));
}

__device__ __forceinline__ bool load_tri(const int* __restrict__ faces, const ProjV* __restrict__ pv, int f, int V, int H, int W, Tri& t, bool& bad) {
    const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    bad = (unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V;
    if (bad) return false;                             // (never an unchecked gather)
    return tri_setup(pv[i0], pv[i1], pv[i2], H, W, t);
}

// ---- raster, one triangle per lane; split != 0: boxes above RENDER_SMALL_BOX go to the queue instead ------------------------------------
template <class Mode>
__global__ __launch_bounds__(RENDER_THREADS) void render_raster_lane_kernel(const int* __restrict__ faces, const ProjV* __restrict__ pv, int B, int V, int n_faces, int H,
                                                                            int W, int split, unsigned long long* __restrict__ vis, unsigned* __restrict__ counters,
                                                                            int* __restrict__ queue, Mode mode) {
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
            queue[atomicAdd(counters, 1u)] = (int)i;   // (at most B * n_faces entries: the queue's size; the entry names the mesh as well as the face)
            continue;
        }
        const typename Mode::Ctx c = mode.ctx(b);
        unsigned long long* frame = vis + (size_t)c.frame * H * W;
        const int Px0 = t.x0 * 256 + 128;
        const int64_t s0 = (int64_t)t.dy[0] * 256, s1 = (int64_t)t.dy[1] * 256, s2 = (int64_t)t.dy[2] * 256;
        for (int y = t.y0; y <= t.y1; ++y) {
            const int Py = y * 256 + 128;
            int64_t w0 = edge_at(t, 0, Px0, Py), w1 = edge_at(t, 1, Px0, Py), w2 = edge_at(t, 2, Px0, Py);
            for (int x = t.x0; x <= t.x1; ++x) {
                fragment(t, w0, w1, w2, f, frame + (size_t)y * W + x, c);
                w0 += s0; w1 += s1; w2 += s2;          // (exact: integers)
            }
        }
    }
}

// ---- raster, one queued triangle per workgroup -----------------------------------------------------------------------------------------
template <class Mode>
__global__ __launch_bounds__(RENDER_THREADS) void render_raster_large_kernel(const int* __restrict__ faces, const ProjV* __restrict__ pv, int B, int V, int n_faces, int H,
                                                                             int W, unsigned long long* __restrict__ vis, const unsigned* __restrict__ counters,
                                                                             const int* __restrict__ queue, Mode mode) {
    const unsigned count = min((int64_t)counters[0], (int64_t)B * n_faces);
    for (unsigned q = blockIdx.x; q < count; q += gridDim.x) {
        const int i = queue[q];
        if ((unsigned)i >= (unsigned)(B * n_faces)) continue;
        const int b = i / n_faces, f = i - b * n_faces;
        Tri t;
        bool bad;
        if (!load_tri(faces, pv + (size_t)b * V, f, V, H, W, t, bad)) continue;
        const typename Mode::Ctx c = mode.ctx(b);
        unsigned long long* frame = vis + (size_t)c.frame * H * W;
        const int bw = t.x1 - t.x0 + 1;
        const int64_t np = (int64_t)bw * (t.y1 - t.y0 + 1);
        for (int64_t p = threadIdx.x; p < np; p += blockDim.x) {
            const int yy = (int)(p / bw), x = t.x0 + (int)(p - (int64_t)yy * bw), y = t.y0 + yy;
            const int Px = x * 256 + 128, Py = y * 256 + 128;
            fragment(t, edge_at(t, 0, Px, Py), edge_at(t, 1, Px, Py), edge_at(t, 2, Px, Py), f, frame + (size_t)y * W + x, c);
        }
    }
}

// ---- resolve: shade the winner, composite ---------------------------------------------------------------------------------------------
// colour = base * (0.3 + g * sum_i max(0, n . l_i)), lights at (0,-1,1), (0,1,1), (1,1,2) in the camera frame (renderer.py:55-67), g = RENDER_LIGHT_GAIN
constexpr float RENDER_AMBIENT = 0.3f, RENDER_LIGHT_GAIN = 0.3f;

struct Px { int covered; int mesh; int face; float depth; uint8_t rgb[3]; int draw; };

// b: the pixel's frame.  The winner's mesh (b itself with one mesh per frame) names the block of pv / pos / nrm that is gathered and the base colour.
template <class Mode>
__device__ inline Px resolve_pixel(unsigned long long key, int b, int x, int y, const int* __restrict__ faces, const ProjV* __restrict__ pv, const Vec4* __restrict__ pos,
                                   const Vec4* __restrict__ nrm, int V, int n_faces, int H, int W, const Shade& sh, bool want_colour, const Mode& mode) {
    Px o;
    o.covered = 0; o.mesh = -1; o.face = -1; o.depth = __uint_as_float(0x7f800000u); o.draw = 0; o.rgb[0] = o.rgb[1] = o.rgb[2] = 0;
    if (key == RENDER_EMPTY) return o;
    Winner win;
    if (!mode.decode(key, b, win)) return o;
    const int f = win.face;
    if ((unsigned)f >= (unsigned)n_faces) return o;
    const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return o;
    const size_t vb = (size_t)win.mesh * V;
    Tri t;
    if (!tri_setup(pv[vb + i0], pv[vb + i1], pv[vb + i2], H, W, t)) return o;
    o.covered = 1; o.mesh = win.mesh; o.face = f; o.depth = win.depth; o.draw = 1;
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
    const float* base = mode.base(win.mesh, sh.base);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = fminf(fmaxf(base[c] * lum, 0.f), 1.f);
        o.rgb[c] = (uint8_t)(int)(v * 255.0f);
    }
    return o;
}

// A thread owns four consecutive pixels of the flattened (B * H * W) batch = 12 bytes of frame = three aligned dwords; the last n % 4 pixels go bytewise.
template <class Mode>
__global__ __launch_bounds__(RENDER_THREADS) void render_resolve_kernel(const unsigned long long* __restrict__ vis, const int* __restrict__ faces, const ProjV* __restrict__ pv,
                                                                        const Vec4* __restrict__ pos, const Vec4* __restrict__ nrm, const uint8_t* frames_in,
                                                                        uint8_t* out, int* __restrict__ face_id, float* __restrict__ depth, int B, int V, int n_faces,
                                                                        int H, int W, Shade sh, Mode mode) {
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
            const Px o = resolve_pixel(vis[i], b, x, y, faces, pv, pos, nrm, V, n_faces, H, W, sh, out != nullptr, mode);
            mode.put_mesh(i, o.mesh);
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

// ---- host tables -> device, as kernel arguments -------------------------------------------------------------------------------------------
// The frame -> first mesh table and its inverse are built on the host per call.  They travel in the kernel-argument block of a one-workgroup launch (a copy the
// runtime takes at launch time): no staging copy from pageable memory, so the call neither waits for the stream nor keeps a host buffer alive.
constexpr int RENDER_TABLE_CHUNK = 512;
struct TableChunk { int v[RENDER_TABLE_CHUNK]; };
__global__ __launch_bounds__(RENDER_THREADS) void render_table_kernel(TableChunk c, int n, int* __restrict__ dst) {
    for (int i = threadIdx.x; i < n && i < RENDER_TABLE_CHUNK; i += blockDim.x) dst[i] = c.v[i];
}

inline size_t up256(size_t n) { return (n + 255) / 256 * 256; }
// B frames of H x W pixels, M meshes of V vertices (M = B with one mesh per frame), table_ints of host tables
struct Layout { size_t vis, pv, pos, nrm, counters, queue, table, total; };
inline Layout layout(int B, int M, int V, int n_faces, int H, int W, size_t table_ints) {
    Layout l;
    size_t at = 0;
    l.vis = at; at += up256((size_t)B * H * W * 8);
    l.pv = at; at += up256((size_t)M * V * sizeof(ProjV));
    l.pos = at; at += up256((size_t)M * V * sizeof(Vec4));
    l.nrm = at; at += up256((size_t)M * V * sizeof(Vec4));
    l.counters = at; at += 256;
    l.queue = at; at += up256((size_t)M * n_faces * 4);
    l.table = at; at += up256(table_ints * 4);
    l.total = at;
    return l;
}
inline int grid_for(int64_t items) { return (int)max((int64_t)1, min((int64_t)RENDER_MAX_GRID, (items + RENDER_THREADS - 1) / RENDER_THREADS)); }

struct Targets { const uint8_t* frames_in; uint8_t* out; int32_t* face_id; float* depth; };

// the passes of one call: M meshes into the visibility buffer of B frames, then one resolve over the B frames
template <class Mode>
int run_passes(const char* who, const float* verts, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_idx, const float* cam, const float* rot, const Targets& t,
               int B, int M, int V, int n_faces, int H, int W, const Shade& sh, int flags, int form, char* ws, const Layout& l, const Mode& mode, hipStream_t st) {
    unsigned long long* vis = (unsigned long long*)(ws + l.vis);
    ProjV* pv = (ProjV*)(ws + l.pv);
    Vec4* pos = (Vec4*)(ws + l.pos);
    Vec4* nrm = (Vec4*)(ws + l.nrm);
    unsigned* counters = (unsigned*)(ws + l.counters);
    int* queue = (int*)(ws + l.queue);
    const dim3 blk(RENDER_THREADS);
    MAED_HIP(hipMemsetAsync(vis, 0xFF, (size_t)B * H * W * 8, st), who);
    MAED_HIP(hipMemsetAsync(counters, 0, 256, st), who);
    if (M > 0) {
        hipLaunchKernelGGL(render_vertex_kernel, dim3(grid_for((int64_t)M * V)), blk, 0, st, verts, cam, rot, M, V, H, W, pv, pos);
        if (t.out && !(flags & MAED_RENDER_RASTER_ONLY))
            hipLaunchKernelGGL(render_normal_kernel, dim3(grid_for((int64_t)M * V)), blk, 0, st, (const Vec4*)pos, faces, vf_off, vf_idx, M, V, n_faces, nrm);
        hipLaunchKernelGGL(render_raster_lane_kernel<Mode>, dim3(grid_for((int64_t)M * n_faces)), blk, 0, st, faces, (const ProjV*)pv, M, V, n_faces, H, W,
                           (int)(form == FORM_SPLIT), vis, counters, queue, mode);
        if (form == FORM_SPLIT)
            hipLaunchKernelGGL(render_raster_large_kernel<Mode>, dim3(RENDER_LARGE_GRID), blk, 0, st, faces, (const ProjV*)pv, M, V, n_faces, H, W, vis,
                               (const unsigned*)counters, (const int*)queue, mode);
    }
    if (!(flags & MAED_RENDER_RASTER_ONLY))
        hipLaunchKernelGGL(render_resolve_kernel<Mode>, dim3(grid_for(((int64_t)B * H * W + 3) / 4)), blk, 0, st, (const unsigned long long*)vis, faces, (const ProjV*)pv,
                           (const Vec4*)pos, (const Vec4*)nrm, t.frames_in, t.out, t.face_id, t.depth, B, V, n_faces, H, W, sh, mode);
    MAED_CHECK_LAUNCH(who);
    return MAED_OK;
}

}  // namespace

extern "C" size_t maed_render_mesh_workspace(int B, int V, int n_faces, int H, int W, int flags) {
    (void)flags;
    if (B <= 0 || V <= 0 || n_faces <= 0 || H <= 0 || W <= 0) return 0;
    return layout(B, B, V, n_faces, H, W, 0).total;
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
    const Layout l = layout(B, B, V, n_faces, H, W, 0);
    MAED_CHECK_ARG(workspace && workspace_bytes >= l.total, MAED_ERR_ARG, "render_mesh: needs %zu bytes of workspace", l.total);
    MAED_CHECK_ARG(is_aligned(workspace, 16), MAED_ERR_ALIGN, "render_mesh: workspace must be 16-byte aligned");
    // measured (profiles/render_micro.txt): see docs/design/11_render.md for the choice of the automatic form
    const int form = form_in == FORM_AUTO ? FORM_SPLIT : form_in;
    Shade sh;
    for (int c = 0; c < 3; ++c) sh.base[c] = base_host ? base_host[c] : 1.0f;
    sh.wire_px = wire_px;
    sh.wireframe = wireframe;
    return run_passes("render_mesh", verts, faces, vf_off, vf_idx, cam, rot, Targets{frames_in, out, face_id, depth}, B, B, V, n_faces, H, W, sh, flags, form, (char*)workspace,
                      l, OneMesh{0}, (hipStream_t)stream);
}

extern "C" size_t maed_render_people_workspace(int M, int B, int V, int n_faces, int H, int W, int flags) {
    (void)flags;
    if (M < 0 || B <= 0 || V <= 0 || n_faces <= 0 || H <= 0 || W <= 0) return 0;
    return layout(B, M, V, n_faces, H, W, (size_t)B + 1 + (size_t)M).total;
}

extern "C" int maed_render_people(const float* verts, const int32_t* faces, const int32_t* faces_host, const int32_t* vf_off, const int32_t* vf_idx, const float* cam,
                                  const float* rot, const float* colour, const float* zoff, const int32_t* mesh_frame_host, const uint8_t* frames_in, uint8_t* out,
                                  int32_t* mesh_id, int32_t* face_id, float* depth, int M, int B, int V, int n_faces, int H, int W, int flags, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    MAED_CHECK_ARG(M >= 0 && B > 0 && V > 0 && n_faces > 0 && H > 0 && W > 0, MAED_ERR_ARG,
                   "render_people: sizes must be positive (M %d may be 0; B %d, V %d, faces %d, viewport %d x %d)", M, B, V, n_faces, W, H);
    MAED_CHECK_ARG(H <= RENDER_MAX_DIM && W <= RENDER_MAX_DIM, MAED_ERR_ARG,
                   "render_people: viewport %d x %d is too large (at most %d in each direction: sub-pixel coordinates have 8 fractional bits and edge functions 64)", W, H,
                   RENDER_MAX_DIM);
    MAED_CHECK_ARG(n_faces < RENDER_MAX_FACES, MAED_ERR_ARG, "render_people: %d faces, the key holds a face index below 2^24 = %d", n_faces, RENDER_MAX_FACES);
    MAED_CHECK_ARG((int64_t)B * H * W < ((int64_t)1 << 31) && (int64_t)M * n_faces < ((int64_t)1 << 31) && (int64_t)M * V < ((int64_t)1 << 31), MAED_ERR_ARG,
                   "render_people: call too large (B H W, M n_faces and M V are each counted in 31 bits)");
    const int shared = (flags & MAED_RENDER_SHARED_DEPTH) != 0;
    MAED_CHECK_ARG(!(flags & MAED_RENDER_WIREFRAME), MAED_ERR_UNSUPPORTED,
                   "render_people: no wireframe in the one-pass form (a pixel that fails the edge test shows the layer below; one winner per pixel cannot say that): "
                   "draw the layers one after the other with maed_render_mesh");
    const int form_in = (flags & MAED_RENDER_FORM_MASK) >> MAED_RENDER_FORM_SHIFT;
    MAED_CHECK_ARG(form_in >= FORM_AUTO && form_in <= FORM_SPLIT, MAED_ERR_ARG, "render_people: form %d", form_in);
    MAED_CHECK_ARG(M == 0 || (verts && faces && cam && mesh_frame_host), MAED_ERR_ARG, "render_people: null pointer");
    MAED_CHECK_ARG(out || mesh_id || face_id || depth, MAED_ERR_ARG, "render_people: no output requested");
    MAED_CHECK_ARG(!out || M == 0 || (vf_off && vf_idx && colour), MAED_ERR_ARG, "render_people: a colour output needs the vertex -> face CSR and the colours");
    MAED_CHECK_ARG(!out || (is_aligned(out, 4) && (!frames_in || is_aligned(frames_in, 4))), MAED_ERR_ALIGN, "render_people: frames must be 4-byte aligned");
    MAED_CHECK_ARG(shared || !zoff, MAED_ERR_ARG, "render_people: a depth offset needs MAED_RENDER_SHARED_DEPTH (the painter order does not compare depths between meshes)");
    for (int m = 0, run = 0; m < M; ++m) {
        const int b = mesh_frame_host[m];
        MAED_CHECK_ARG(b >= 0 && b < B, MAED_ERR_ARG, "render_people: mesh %d is in frame %d, outside [0, %d)", m, b, B);
        MAED_CHECK_ARG(m == 0 || b >= mesh_frame_host[m - 1], MAED_ERR_ARG, "render_people: mesh_frame must not decrease (mesh %d: frame %d after frame %d)", m, b,
                       (int)mesh_frame_host[m - 1]);
        run = (m > 0 && b == mesh_frame_host[m - 1]) ? run + 1 : 1;
        MAED_CHECK_ARG(run <= RENDER_MAX_LAYERS, MAED_ERR_ARG, "render_people: frame %d has more than %d meshes (the key holds 8 bits of layer)", b, RENDER_MAX_LAYERS);
    }
    if (faces_host)
        for (int64_t i = 0; i < (int64_t)n_faces * 3; ++i)
            MAED_CHECK_ARG((uint32_t)faces_host[i] < (uint32_t)V, MAED_ERR_ARG, "render_people: face %lld has vertex index %d outside [0, %d)", (long long)(i / 3),
                           (int)faces_host[i], V);
    const size_t table_ints = (size_t)B + 1 + (size_t)M;
    const Layout l = layout(B, M, V, n_faces, H, W, table_ints);
    MAED_CHECK_ARG(workspace && workspace_bytes >= l.total, MAED_ERR_ARG, "render_people: needs %zu bytes of workspace", l.total);
    MAED_CHECK_ARG(is_aligned(workspace, 16), MAED_ERR_ALIGN, "render_people: workspace must be 16-byte aligned");
    char* ws = (char*)workspace;
    int* table_dev = (int*)(ws + l.table);
    hipStream_t st = (hipStream_t)stream;
    // the table, a chunk at a time: first[j] = number of meshes in frames below j (B + 1 entries), then the frame of every mesh (M entries)
    for (size_t at = 0, m = 0; at < table_ints; at += RENDER_TABLE_CHUNK) {
        TableChunk c;
        const int n = (int)std::min((size_t)RENDER_TABLE_CHUNK, table_ints - at);
        for (int k = 0; k < RENDER_TABLE_CHUNK; ++k) {
            const size_t j = at + k;
            if (k >= n) { c.v[k] = 0; continue; }
            if (j <= (size_t)B) {
                while (m < (size_t)M && (size_t)mesh_frame_host[m] < j) ++m;
                c.v[k] = (int)m;
            } else {
                c.v[k] = mesh_frame_host[j - (size_t)B - 1];
            }
        }
        hipLaunchKernelGGL(render_table_kernel, dim3(1), dim3(RENDER_THREADS), 0, st, c, n, table_dev + at);
    }
    const int form = form_in == FORM_AUTO ? FORM_SPLIT : form_in;
    Shade sh;
    sh.base[0] = sh.base[1] = sh.base[2] = 1.0f;
    sh.wire_px = 0.f;
    sh.wireframe = 0;
    Layered mode;
    mode.first = table_dev; mode.mesh_frame = table_dev + B + 1; mode.zoff = zoff; mode.colour = colour; mode.mesh_id = mesh_id; mode.shared = shared;
    return run_passes("render_people", verts, faces, vf_off, vf_idx, cam, rot, Targets{frames_in, out, face_id, depth}, B, M, V, n_faces, H, W, sh, flags, form, ws, l, mode, st);
}

