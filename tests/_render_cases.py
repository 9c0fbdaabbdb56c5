"""TEST INFRASTRUCTURE: the scenes of the rasteriser's tests and the comparison against tests/_render_ref.py, shared by the simulator tests
(tests/test_hostsim_render.py) and the GPU tests (tests/test_gpu_render.py).  Scenes are procedural: no licensed mesh, nothing read from outside tests/."""
import functools

import numpy as np

import _render_ref as R

# Measured on the host simulator over every scene below (tests/test_hostsim_render.py::test_measured_bounds prints and re-checks them):
DEPTH_ERR = 2.01e-7         # largest |depth_kernel - depth_fp64|; the fp32 depth formula is three quotients, three products and three sums on |z| <= 1
DELTA = 4 * DEPTH_ERR       # a pixel whose two nearest candidates are closer than this is a tie pixel and is excluded from the face / colour comparison
WIRE_ERR = 1.02e-7          # largest |distance_kernel - distance_fp64| in px, over covered pixels whose fp64 distance is below 1 px
WIRE_DELTA = 4 * WIRE_ERR   # a pixel whose edge distance is this close to the threshold is excluded from the wireframe comparison
MAX_EXCLUDED = 1e-3         # at most this share of a scene's covered pixels may be excluded


def _front(verts, faces, cam, H, W):
    """wind every face so that it faces the camera of frame 0 (for hand-made triangle soups)"""
    X, Y, _, _ = R.project_f32(verts, cam, None, H, W)
    A = -((X[faces[:, 1]] - X[faces[:, 0]]) * (Y[faces[:, 2]] - Y[faces[:, 0]]) - (X[faces[:, 2]] - X[faces[:, 0]]) * (Y[faces[:, 1]] - Y[faces[:, 0]]))
    out = faces.copy()
    out[A < 0] = out[A < 0][:, [0, 2, 1]]
    return out


def _scene(verts, faces, cams, H, W, rots=None, seed=0):
    verts = np.asarray(verts, dtype=np.float32)
    if verts.ndim == 2:
        verts = np.broadcast_to(verts, (len(cams),) + verts.shape)
    frames = np.random.default_rng(seed).integers(0, 256, size=(len(cams), H, W, 3), dtype=np.uint8)
    return dict(verts=np.ascontiguousarray(verts), faces=np.ascontiguousarray(faces, dtype=np.int32), cams=np.ascontiguousarray(cams, dtype=np.float32),
                rots=None if rots is None else np.ascontiguousarray(rots, dtype=np.float32), H=H, W=W, frames=frames)


def _generic(v):
    """a fixed rotation in general position: the symmetric generators otherwise give axis-aligned edges, whose pixel centres lie at EXACTLY 0.5 px (representable
    in both precisions and drawn by both, but inside any exclusion band around the threshold, which the scenes have to keep under the cap)"""
    from maed_amd.render import rotation_matrix
    return (np.asarray(v, dtype=np.float64) @ rotation_matrix(37.3, [0.31, -0.52, 0.8]).T).astype(np.float32)


def _rots(n, seed):
    from maed_amd.render import rotation_matrix
    g = np.random.default_rng(seed)
    return np.stack([rotation_matrix(g.uniform(-180, 180), g.normal(size=3)) for _ in range(n)])


def ico_224():
    v, f = R.icosphere(3, 0.9)
    v = _generic(v)
    return _scene(v, f, [R.fit_cam(v, 224, 224, 0.7)], 224, 224)


def ico_b16_224():
    v, f = R.icosphere(2, 0.8)
    v = v * np.array([1.0, 1.2, 0.7], dtype=np.float32)
    g = np.random.default_rng(3)
    cams = [R.fit_cam(v, 224, 224, g.uniform(0.2, 0.9), centre=g.uniform(-0.4, 0.4, size=2)) for _ in range(16)]
    return _scene(v, f, cams, 224, 224, rots=_rots(16, 4), seed=1)


def torus_odd():
    from maed_amd.render import rotation_matrix
    v, f = R.torus()
    return _scene(v, f, [R.fit_cam(v, 353, 637, 0.55)], 353, 637, rots=[rotation_matrix(55.0, [1.0, 0.3, 0.1])], seed=2)


def two_spheres():
    a, b = R.icosphere(3, 0.5), R.icosphere(3, 0.4)
    va = _generic(a[0]) + np.array([-0.15, 0.0, -0.35], dtype=np.float32)      # smaller ndc_z = nearer
    vb = _generic(b[0]) + np.array([0.2, 0.1, 0.45], dtype=np.float32)
    v, f = R.merge((va, a[1]), (vb, b[1]))
    return _scene(v, f, [np.array([0.9, 0.9, 0.0, 0.0])], 224, 224, seed=3)


def smpl_1080():
    v, f = R.smpl_sized()
    return _scene(v, f, [R.fit_cam(v, 1080, 1920, 1 / 3, centre=(0.2, -0.1))], 1080, 1920, seed=4)


def smpl_b16_224():
    v, f = R.smpl_sized()
    cams = [R.fit_cam(v, 224, 224, h, centre=(0.02 * k - 0.15, 0.01 * k)) for k, h in enumerate(np.linspace(0.3, 0.95, 16))]
    from maed_amd.render import rotation_matrix
    rots = np.stack([rotation_matrix(22.5 * k, [0.0, 1.0, 0.0]) for k in range(16)])
    return _scene(v, f, cams, 224, 224, rots=rots, seed=5)


def large_triangles():
    """a tilted ground quad far larger than the viewport, a triangle that covers most of it, and a small sphere in front: bounding boxes of millions of pixels"""
    quad = np.array([[-9.0, -7.0, 0.9], [9.0, -7.0, 0.9], [9.0, 7.0, 0.2], [-9.0, 7.0, 0.2]], dtype=np.float32)
    tri = np.array([[-0.9, -0.8, 0.1], [0.95, -0.6, -0.2], [0.1, 0.9, 0.15]], dtype=np.float32)
    s = R.icosphere(2, 0.3)
    v, f = R.merge((quad, np.array([[0, 1, 2], [0, 2, 3]])), (tri, np.array([[0, 1, 2]])), (_generic(s[0]) + np.array([0.0, 0.0, -0.5], dtype=np.float32), s[1]))
    cam = np.array([0.9 * 1080 / 1920, 0.9, 0.0, 0.0])
    f[:3] = _front(v, f[:3], cam, 1080, 1920)
    return _scene(v, f, [cam], 1080, 1920, seed=6)


def subpixel():
    v, f = R.smpl_sized()
    return _scene(v, f, [R.fit_cam(v, 224, 224, 0.12, centre=(-0.3, 0.4))], 224, 224, seed=7)


def borders():
    v, f = R.icosphere(2, 0.8)
    v = _generic(v)
    cams = [R.fit_cam(v, 353, 637, 0.8, centre=c) for c in ((-1.0, 0.0), (1.0, 0.1), (0.1, -1.0), (0.0, 1.0), (1.0, 1.0))]
    return _scene(v, f, cams, 353, 637, seed=8)


def zclip():
    v, f = R.icosphere(3, 0.6)
    v = _generic(v)
    verts = np.stack([v + np.array([0.0, 0.0, 0.7], dtype=np.float32), v + np.array([0.0, 0.0, -0.7], dtype=np.float32)])
    return _scene(verts, f, [np.array([0.9, 0.9, 0.0, 0.0])] * 2, 224, 224, seed=9)


SCENES = dict(ico_224=ico_224, ico_b16_224=ico_b16_224, torus_odd=torus_odd, two_spheres=two_spheres, smpl_1080=smpl_1080, smpl_b16_224=smpl_b16_224,
              large_triangles=large_triangles, subpixel=subpixel, borders=borders, zclip=zclip)


def interpenetrating():
    """two spheres that cut through each other: depth ties along the intersection curve by design (only determinism and coverage are asserted on it)"""
    a, b = R.icosphere(3, 0.5), R.icosphere(3, 0.5)
    v, f = R.merge((_generic(a[0]) + np.array([-0.2, 0.0, 0.0], dtype=np.float32), a[1]), (_generic(b[0]) + np.array([0.2, 0.05, 0.1], dtype=np.float32), b[1]))
    return _scene(v, f, [np.array([0.9, 0.9, 0.0, 0.0])], 224, 224, seed=10)


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    s = scene(name)
    return R.render_ref_batch(s["verts"], s["faces"], s["cams"], s["H"], s["W"], s["rots"], frames=s["frames"])


def oracle_stats(name):
    """share of covered pixels that are tie pixels / near the wireframe threshold, by the oracle alone"""
    ref = reference(name)
    cov = ref["covered"]
    tie = cov & (ref["second"] - ref["depth"] < DELTA)
    near = cov & (np.abs(ref["wire_dist"] - 0.5) < WIRE_DELTA)
    return dict(covered=int(cov.sum()), tie=int(tie.sum()), near=int(near.sum()))


def compare(name, got, got_wire=None):
    """got: dict(out uint8 (B,H,W,3), face_id, depth) of the kernels on scene(name) with its frames as background; got_wire: the wireframe composite.  Returns the
    figures; the caller prints and asserts."""
    s, ref = scene(name), reference(name)
    cov = ref["covered"]
    st = dict(scene=name, covered=int(cov.sum()))
    gcov = got["face_id"] >= 0
    st["coverage_diff"] = int((gcov != cov).sum())
    both = gcov & cov
    with np.errstate(invalid="ignore"):
        derr = np.abs(got["depth"].astype(np.float64) - ref["depth"])
        tie = cov & (ref["second"] - ref["depth"] < DELTA)
    keep = both & ~tie
    st["excluded"] = int(tie.sum())
    st["face_diff"] = int((got["face_id"] != ref["face_id"])[keep].sum())
    st["face_diff_any"] = int((got["face_id"] != ref["face_id"])[both].sum())
    st["depth_err"] = float(derr[keep].max()) if keep.any() else 0.0
    st["depth_err_any"] = float(derr[both].max()) if both.any() else 0.0
    st["uncovered_inf"] = bool(np.isposinf(got["depth"][~gcov]).all())
    same = keep & (got["face_id"] == ref["face_id"])
    lv = np.abs(got["out"].astype(np.int64) - ref["rgb"].astype(np.int64))
    st["colour_diff"] = int(lv[same].max()) if same.any() else 0
    st["colour_share_off"] = float((lv[same] > 0).mean()) if same.any() else 0.0
    st["background_diff"] = int((got["out"][~gcov] != s["frames"][~gcov]).sum())
    if got_wire is not None:
        near = cov & (np.abs(ref["wire_dist"] - 0.5) < WIRE_DELTA)
        wkeep = same & ~near
        st["wire_excluded"] = int(near.sum())
        drawn_ref = ref["wire_dist"] <= 0.5
        bg = s["frames"]
        want = np.where(drawn_ref[..., None], got["out"], bg)       # (the kernel's own shaded colour where the oracle draws: the colour itself is checked above)
        st["wire_diff"] = int((got_wire != want).any(-1)[wkeep | ~gcov].sum())
        st["wire_drawn"] = int(drawn_ref.sum())
    return st


def assert_stats(st):
    assert st["coverage_diff"] == 0, st
    assert st["excluded"] <= MAX_EXCLUDED * st["covered"], st
    assert st["face_diff"] == 0, st
    assert st["depth_err"] <= DEPTH_ERR, st
    assert st["uncovered_inf"], st
    assert st["colour_diff"] <= 1, st
    assert st["background_diff"] == 0, st
    if "wire_diff" in st:
        assert st["wire_excluded"] <= MAX_EXCLUDED * st["covered"], st
        assert st["wire_diff"] == 0, st
