"""TEST INFRASTRUCTURE: numpy restatement of the mesh rasteriser's definitions (docs/design/11_render.md), plus the procedural scenes the tests draw.

Three parts mirror the kernel's arithmetic ON PURPOSE, operation by operation, so that coverage can be compared exactly: the float32 projection and snap
(project_f32), the int64 edge functions with the top-left rule, and the float32 depth that decides the |ndc_z| <= 1 clip (a clipped fragment is not covered, so
the clip is part of coverage).  Everything else -- the depth that is compared, the second-nearest candidate, vertex normals, shading, the wireframe distance --
is float64 and is the definition the kernels are measured against."""
import numpy as np

AMBIENT, GAIN = 0.3, 0.3
LIGHTS = np.array([[0.0, -1.0, 1.0], [0.0, 1.0, 1.0], [1.0, 1.0, 2.0]])
CLAMP = np.float32(2.0 ** 30)
F = np.float32


# ---- the mirrored parts ------------------------------------------------------------------------------------------------------------
def project_f32(verts, cam, rot, H, W):
    """-> X, Y (int64, 1/256 px, y down), z (float32 ndc_z), ok (finite)"""
    with np.errstate(all="ignore"):
        v = np.asarray(verts, dtype=F)
        X, Y, Z = v[:, 0], -v[:, 1], -v[:, 2]
        if rot is not None:
            r = np.asarray(rot, dtype=F).reshape(9)
            x0, y0, z0 = X, Y, Z
            X = (r[0] * x0 + r[1] * y0) + r[2] * z0
            Y = (r[3] * x0 + r[4] * y0) + r[5] * z0
            Z = (r[6] * x0 + r[7] * y0) + r[8] * z0
        sx, sy, tx, ty = (F(c) for c in cam)
        ndx = sx * (X + tx)
        ndy = sy * (Y - ty)
        ndz = -Z + F(0)
        hw, hh = F(0.5) * F(W), F(0.5) * F(H)
        fx = ((ndx + F(1)) * hw) * F(256)
        fy = ((F(1) - ndy) * hh) * F(256)
        ok = np.isfinite(fx) & np.isfinite(fy) & np.isfinite(ndz)
        fx = np.minimum(np.maximum(fx, -CLAMP), CLAMP)
        fy = np.minimum(np.maximum(fy, -CLAMP), CLAMP)
        Xi = np.where(ok, np.rint(fx), 0).astype(np.int64)
        Yi = np.where(ok, np.rint(fy), 0).astype(np.int64)
    assert ndz.dtype == F and fx.dtype == F
    return Xi, Yi, ndz, ok


def rotated_f64(verts, rot):
    v = np.asarray(verts, dtype=np.float32).astype(np.float64) * np.array([1.0, -1.0, -1.0])
    return v if rot is None else v @ np.asarray(rot, dtype=np.float32).astype(np.float64).T


class TriSetup:
    """per-face integers of one frame: edge origins / deltas / biases, twice the area, clamped bounding boxes, the front-facing & finite & on-screen flag"""

    def __init__(self, X, Y, ok, faces, H, W):
        fx, fy = X[faces], Y[faces]                      # (n, 3)
        self.A = -((fx[:, 1] - fx[:, 0]) * (fy[:, 2] - fy[:, 0]) - (fx[:, 2] - fx[:, 0]) * (fy[:, 1] - fy[:, 0]))
        a, b = [1, 2, 0], [2, 0, 1]
        self.ax, self.ay = fx[:, a], fy[:, a]
        self.dx, self.dy = fx[:, b] - fx[:, a], fy[:, b] - fy[:, a]
        self.bias = np.where((self.dy > 0) | ((self.dy == 0) & (self.dx < 0)), 0, -1).astype(np.int64)
        self.x0 = np.maximum(0, (fx.min(1) + 127) >> 8)
        self.x1 = np.minimum(W - 1, (fx.max(1) - 128) >> 8)
        self.y0 = np.maximum(0, (fy.min(1) + 127) >> 8)
        self.y1 = np.minimum(H - 1, (fy.max(1) - 128) >> 8)
        self.live = ok[faces].all(1) & (self.A > 0) & (self.x0 <= self.x1) & (self.y0 <= self.y1)

    def edges(self, f, PX, PY):
        return [self.dy[f, i] * (PX - self.ax[f, i]) - self.dx[f, i] * (PY - self.ay[f, i]) for i in range(3)]


def depth_f32(w, A, z):
    """the kernel's depth: three float32 quotients, (l0 z0 + l1 z1) + l2 z2, + 0"""
    fA = F(A) if np.isscalar(A) or np.ndim(A) == 0 else A.astype(F)
    l = [wi.astype(F) / fA for wi in w]
    return ((l[0] * z[0] + l[1] * z[1]) + l[2] * z[2]) + F(0)


# ---- one frame -----------------------------------------------------------------------------------------------------------------------
def render_ref(verts, faces, cam, H, W, rot=None, base=(1.0, 1.0, 0.9), frame=None, wire_px=0.5):
    """-> dict(covered bool (H, W), face_id int32, depth fp64 (inf where uncovered), second fp64 (second-nearest candidate depth, inf if none), rgb uint8 shaded
    composite, lum fp64 per channel before truncation, wire_dist fp64 (distance of the centre to the nearest edge of the visible face, px), wire uint8 composite)"""
    faces = np.asarray(faces, dtype=np.int64)
    X, Y, z32, ok = project_f32(verts, cam, rot, H, W)
    P = rotated_f64(verts, rot)
    z64 = -P[:, 2]
    T = TriSetup(X, Y, ok, faces, H, W)
    best = np.full((H, W), np.inf)
    second = np.full((H, W), np.inf)
    face_id = np.full((H, W), -1, dtype=np.int32)
    for f in np.nonzero(T.live)[0]:
        ys, xs = slice(T.y0[f], T.y1[f] + 1), slice(T.x0[f], T.x1[f] + 1)
        PX = (np.arange(T.x0[f], T.x1[f] + 1, dtype=np.int64) * 256 + 128)[None, :]
        PY = (np.arange(T.y0[f], T.y1[f] + 1, dtype=np.int64) * 256 + 128)[:, None]
        w = T.edges(f, PX, PY)
        inside = (w[0] + T.bias[f, 0] >= 0) & (w[1] + T.bias[f, 1] >= 0) & (w[2] + T.bias[f, 2] >= 0)
        if not inside.any():
            continue
        i = faces[f]
        with np.errstate(all="ignore"):
            cov = inside & (np.abs(depth_f32(w, T.A[f], z32[i])) <= F(1))
        if not cov.any():
            continue
        d = (w[0] * z64[i[0]] + w[1] * z64[i[1]] + w[2] * z64[i[2]]) / float(T.A[f])
        b, s = best[ys, xs], second[ys, xs]
        nearer = cov & (d < b)                           # (strict: an exact tie keeps the lower face index)
        second[ys, xs] = np.where(nearer, b, np.where(cov & (d < s), d, s))
        best[ys, xs] = np.where(nearer, d, b)
        face_id[ys, xs] = np.where(nearer, f, face_id[ys, xs])
    covered = face_id >= 0
    out = dict(covered=covered, face_id=face_id, depth=best, second=second)
    # shading of the winners, all pixels at once
    yy, xx = np.nonzero(covered)
    fw = face_id[yy, xx].astype(np.int64)
    PX, PY = xx.astype(np.int64) * 256 + 128, yy.astype(np.int64) * 256 + 128
    w = [T.dy[fw, i] * (PX - T.ax[fw, i]) - T.dx[fw, i] * (PY - T.ay[fw, i]) for i in range(3)]
    A = T.A[fw].astype(np.float64)
    lam = [wi / A for wi in w]
    fn = np.cross(P[faces[:, 1]] - P[faces[:, 0]], P[faces[:, 2]] - P[faces[:, 0]])
    vn = np.zeros_like(P)
    for k in range(3):
        np.add.at(vn, faces[:, k], fn)
    ln = np.linalg.norm(vn, axis=1, keepdims=True)
    vn = np.divide(vn, ln, out=np.zeros_like(vn), where=ln > 0)
    idx = faces[fw]
    n = sum(lam[k][:, None] * vn[idx[:, k]] for k in range(3))
    nl = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.divide(n, nl, out=np.zeros_like(n), where=nl > 0)
    p = sum(lam[k][:, None] * P[idx[:, k]] for k in range(3))
    tot = np.zeros(len(fw))
    for Lp in LIGHTS:
        l = Lp[None, :] - p
        l /= np.linalg.norm(l, axis=1, keepdims=True)
        tot += np.maximum(0.0, (n * l).sum(1))
    lum = np.clip(np.asarray(base, dtype=np.float32).astype(np.float64)[None, :] * (AMBIENT + GAIN * tot)[:, None], 0.0, 1.0) * 255.0
    bg = np.zeros((H, W, 3), dtype=np.uint8) if frame is None else np.asarray(frame).astype(np.uint8)
    rgb = bg.copy()
    rgb[yy, xx] = np.floor(lum).astype(np.uint8)
    lum_img = np.zeros((H, W, 3))
    lum_img[yy, xx] = lum
    dist = np.full((H, W), np.inf)
    dist[yy, xx] = np.min([w[i] / (np.sqrt((T.dx[fw, i] ** 2 + T.dy[fw, i] ** 2).astype(np.float64)) * 256.0) for i in range(3)], axis=0)
    # the kernel's float32 distance, restated (used only to MEASURE the float32 error that sizes the exclusion band: tests/_render_cases.py WIRE_ERR)
    dist32 = np.full((H, W), np.inf, dtype=F)
    dist32[yy, xx] = np.min([w[i].astype(F) / (np.sqrt((T.dx[fw, i] ** 2 + T.dy[fw, i] ** 2).astype(F)) * F(256)) for i in range(3)], axis=0)
    out["wire_dist32"] = dist32
    wire = bg.copy()
    drawn = dist <= wire_px
    wire[drawn] = rgb[drawn]
    out.update(rgb=rgb, lum=lum_img, wire_dist=dist, wire=wire, background=bg)
    return out


def render_ref_batch(verts, faces, cams, H, W, rots=None, base=(1.0, 1.0, 0.9), frames=None, wire_px=0.5):
    res = [render_ref(verts[b], faces, cams[b], H, W, None if rots is None else rots[b], base, None if frames is None else frames[b], wire_px) for b in range(len(verts))]
    return {k: np.stack([r[k] for r in res]) for k in res[0]}


# ---- procedural meshes (closed, outward counter-clockwise) ---------------------------------------------------------------------------------
def icosphere(level=2, radius=1.0):
    t = (1.0 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8),
         (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, dtype=np.int32)


def uv_sphere(rings, segs, radii=(1.0, 1.0, 1.0)):
    """closed latitude / longitude mesh: rings * segs + 2 vertices, 2 * rings * segs faces (82 x 84: 6890 and 13776, the counts of SMPL)"""
    th = np.pi * (np.arange(rings) + 1) / (rings + 1)
    ph = 2 * np.pi * np.arange(segs) / segs
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None, :], np.cos(th)[:, None] * np.ones(segs)[None, :], np.sin(th)[:, None] * np.sin(ph)[None, :]], -1)
    v = np.concatenate([[[0.0, 1.0, 0.0]], ring.reshape(-1, 3), [[0.0, -1.0, 0.0]]]) * np.asarray(radii)
    idx = lambda r, s: 1 + r * segs + (s % segs)
    f = []
    south = 1 + rings * segs
    for s in range(segs):
        f.append((0, idx(0, s + 1), idx(0, s)))
        f.append((south, idx(rings - 1, s), idx(rings - 1, s + 1)))
        for r in range(rings - 1):
            f.append((idx(r, s), idx(r, s + 1), idx(r + 1, s + 1)))
            f.append((idx(r, s), idx(r + 1, s + 1), idx(r + 1, s)))
    return v.astype(np.float32), np.array(f, dtype=np.int32)


def torus(nu=32, nv=16, R=0.6, r=0.25):
    u = 2 * np.pi * np.arange(nu) / nu
    w = 2 * np.pi * np.arange(nv) / nv
    v = np.stack([(R + r * np.cos(w)[None, :]) * np.cos(u)[:, None], (R + r * np.cos(w)[None, :]) * np.sin(u)[:, None], r * np.sin(w)[None, :] * np.ones(nu)[:, None]], -1)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    f = []
    for i in range(nu):
        for j in range(nv):
            f.append((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)))
            f.append((idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))
    return v.reshape(-1, 3).astype(np.float32), np.array(f, dtype=np.int32)


def outward(verts, faces):
    """flip the faces of a star-shaped-about-its-centroid closed mesh that point inwards (used once per generator in the tests' self-check)"""
    c = verts.mean(0)
    n = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]])
    flip = (n * (verts[faces].mean(1) - c)).sum(1) < 0
    out = faces.copy()
    out[flip] = out[flip][:, [0, 2, 1]]
    return out


def merge(*meshes):
    vs, fs, at = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + at)
        at += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


def smpl_sized():
    """a closed, body-proportioned mesh with SMPL's counts: 6890 vertices, 13776 faces, about 1.7 units tall"""
    v, f = uv_sphere(82, 84, radii=(0.3, 0.85, 0.2))
    v = v.copy()
    v[:, 0] += 0.08 * np.sin(5.0 * v[:, 1])              # (not a surface of revolution: normals and silhouettes vary)
    assert v.shape == (6890, 3) and f.shape == (13776, 3)
    return v.astype(np.float32), outward(v, f)


def fit_cam(verts, H, W, height_frac, centre=(0.0, 0.0)):
    """camera that makes the mesh `height_frac` of the viewport tall with square pixels, centred at `centre` (ndc)"""
    ext = float(verts[:, 1].max() - verts[:, 1].min())
    sy = 2.0 * height_frac / ext
    sx = sy * H / W
    mid = 0.5 * (verts.max(0) + verts.min(0))
    return np.array([sx, sy, -mid[0] + centre[0] / sx, -mid[1] + centre[1] / sy], dtype=np.float32)
