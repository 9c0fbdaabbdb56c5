"""TEST INFRASTRUCTURE of the video-inference tests (tests/test_hostsim_tracks.py on the host simulator, tests/test_gpu_tracks.py on the GPU): the fixture of
tests/golden/g19_tracks.npz (scripts/make_golden_tracks.py: inputs and the reference's results), numpy restatements of what csrc/tracks.hip has to give, the scenes
of the crop tests, a deterministic stand-in for the model, and the checks both files share.  A `run_tracks(kps, lengths, vis, k, sigma, box_scale)` callable
returns numpy (boxes (K, L, 4) f32, params (K, L, 3) f64, span (K, 2)); a `run_tables(boxes, box_index, frame_index, T, n_frames, h, w, H, W)` one the dict of
the four tables."""
import os

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g19_tracks.npz")
_CASES = None


def cases():
    """[(name, kps (L, J, 3) f32 with -inf confidence where the tracker had nothing, list form for the reference-named functions, (vis, k, sigma), raw, span, params)]"""
    global _CASES
    if _CASES is None:
        z = np.load(GOLDEN)
        out = []
        for i, name in enumerate(z["names"]):
            kps, none = z[f"c{i}_kps"].copy(), z[f"c{i}_none"]
            lst = [None if none[t] else kps[t].astype(np.float64) for t in range(len(kps))]
            kps[none, :, 2] = -np.inf
            vis, k, sigma = z[f"c{i}_cfg"]
            out.append(dict(name=str(name), kps=kps, list=lst, vis=float(vis), k=int(k), sigma=float(sigma), raw=z[f"c{i}_raw"], span=tuple(int(v) for v in z[f"c{i}_span"]),
                            params=z[f"c{i}_params"]))
        _CASES = out
    return _CASES


def case(name):
    return next(c for c in cases() if c["name"] == name)


def params_bar(ref):
    """|got - ref| <= 1e-12 * max(1, max|ref|): both sides are fp64 sums of at most 2 r + 1 <= 1025 terms with weights summing to 1 on inputs that differ by a few
    ulp (sqrt, division, the interpolation formula); the median selects and adds no error: (2 r + 6) * 2^-52 * max|x| < 3e-13 * max|x|"""
    return 1e-12 * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)


def ulp_apart(a, b):
    """distance in fp32 representable values (0 for equal values, infinities of one sign included)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def check_track(c, boxes, params, span, L=None, box_scale=1.1):
    """one track's outputs (boxes (L, 4), params (L, 3), span (2)) against the fixture: acceptance 1-3, and zero rows outside the span"""
    start, end = c["span"]
    assert tuple(int(v) for v in span) == (start, end), (c["name"], span, c["span"])
    ref = c["params"]
    err = float(np.abs(params[:end] - ref).max())
    print(f"{c['name']}: max |params - ref| = {err:.3e}, bar {params_bar(ref):.3e}")
    assert err <= params_bar(ref), (c["name"], err)
    assert (params[end:] == 0).all() and (params[:start] == 0).all() and (boxes[end:] == 0).all() and (boxes[:start] == 0).all(), c["name"]
    with np.errstate(divide="ignore"):
        side = (150.0 / params[start:end, 2] * box_scale).astype(np.float32)
    want = np.stack([params[start:end, 0].astype(np.float32), params[start:end, 1].astype(np.float32), side, side], axis=1)
    assert ulp_apart(boxes[start:end], want).max() <= 1, c["name"]
    assert (np.isinf(side) == np.isinf(boxes[start:end, 2])).all()
    return err


def pad_tracks(cs, extra=2):
    """cases of one J -> kps (K, L, J, 3) with L = longest + extra and lengths; the padding rows hold NaN: they are never read"""
    L = max(len(c["kps"]) for c in cs) + extra
    kps = np.full((len(cs), L) + cs[0]["kps"].shape[1:], np.nan, dtype=np.float32)
    for k, c in enumerate(cs):
        kps[k, :len(c["kps"])] = c["kps"]
    return kps, np.array([len(c["kps"]) for c in cs], dtype=np.int32)


def line_track(L):
    """a track no fixture could hold (L up to 2^20): a person of constant size moving on a straight line, every seventh frame without keypoints.  A line is a fixed
    point of the linear fill, of the median (monotone series) and of the symmetric Gaussian away from the ends, so every interior row is known in closed form."""
    i = np.arange(L, dtype=np.float64)
    kps = np.zeros((1, L, 2, 3), dtype=np.float32)
    kps[0, :, 0, 0], kps[0, :, 0, 1] = 0.5 * i + 10, 100.0
    kps[0, :, 1, 0], kps[0, :, 1, 1] = 0.5 * i + 70, 180.0          # rectangle 60 x 80: height 100, scale 1.5, centre (0.5 i + 40, 140)
    kps[0, :, :, 2] = 1.0
    kps[0, 3:L - 1:7, :, 2] = 0.0
    return kps


def check_line(L, boxes, params, span, k, sigma, box_scale=1.1):
    edge = int(4 * sigma + 0.5) + k // 2 + 1
    assert tuple(int(v) for v in span[0]) == (0, L) and np.isfinite(params).all() and np.isfinite(boxes).all()
    i = np.arange(edge, L - edge, dtype=np.float64)
    want = np.stack([0.5 * i + 40, np.full_like(i, 140.0), np.full_like(i, 1.5)], axis=1)
    err = float(np.abs(params[0, edge:L - edge] - want).max())
    print(f"line of {L} frames: max |params - closed form| = {err:.3e}, bar {params_bar(want):.3e}")
    assert err <= params_bar(want)
    side = np.float32(150.0 / 1.5 * box_scale)
    assert ulp_apart(boxes[0, edge:L - edge, 2:], side).max() <= 1 and ulp_apart(boxes[0, edge:L - edge, 0], want[:, 0].astype(np.float32)).max() <= 1
    return err


# ---- crop tables ---------------------------------------------------------------------------------------------------------------------------------------
def minv_closed_form(boxes, H, W):
    """[w/W 0 cx - w/2; 0 h/H cy - h/2] in fp64 from the fp32 box, rounded once; [0 0 -2; 0 0 -2] for a box that is not finite or not positive"""
    b = np.asarray(boxes, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    out = np.zeros((len(b), 6), dtype=np.float32)
    for i, (cx, cy, w, h) in enumerate(b):
        if np.isfinite([cx, cy, w, h]).all() and w > 0 and h > 0:
            out[i] = [w / W, 0, cx - w / 2, 0, h / H, cy - h / 2]
        else:
            out[i] = [0, 0, -2, 0, 0, -2]
    return out


def degenerate(boxes):
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    return ~(np.isfinite(b).all(axis=1) & (b[:, 2] > 0) & (b[:, 3] > 0))


def check_tables(t, boxes, box_index, frame_index, T, img_h, img_w, H, W):
    """acceptance 5: frame_minv within 1 fp32 ulp of the closed form and within 4 * 2^-24 * max(|cx| + w, |cy| + h) of the inverse of data.gen_trans's matrix
    (that is the fp32 rounding gen_trans applies to its three source points); the other tables exactly"""
    from maed_amd import data as D
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    M = len(box_index)
    used = boxes[np.asarray(box_index)]
    assert ulp_apart(t["frame_minv"], minv_closed_form(used, H, W)).max() <= 1
    for m in np.nonzero(~degenerate(used))[0]:
        cx, cy, w, h = (float(v) for v in used[m])
        ref = D.invert_affine(D.gen_trans(used[m].astype(np.float64), (1, 1), 0, (0, 0), W, H)).reshape(6)
        bound = 4 * 2.0 ** -24 * max(abs(cx) + w, abs(cy) + h)
        assert np.abs(t["frame_minv"][m].astype(np.float64) - ref).max() <= bound, (m, used[m])
    want = np.zeros((M, 8), dtype=np.int32)
    want[:, 0] = np.asarray(frame_index, dtype=np.int64) * img_h * img_w * 3
    want[:, 1], want[:, 2], want[:, 3], want[:, 4] = img_h, img_w, 3 * img_w, np.arange(M) // T
    assert np.array_equal(t["frame_i"], want)
    N = -(-M // T)
    assert t["clip_i"].shape == (N, 8) and not t["clip_i"].any() and t["clip_f"].shape == (N, 4) and not t["clip_f"].any()


def scene_frames(seed, B, h, w):
    """frames that are smooth + noise, so that a wrong tap, pitch or frame offset moves many levels"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for b in range(B):
        base = np.stack([(x * 3 + y + 40 * b) % 256, (x + y * 2 + 90 * b) % 256, (x * y // 16 + b) % 256], -1).astype(np.uint8)
        out.append(base ^ rng.integers(0, 32, (h, w, 1), dtype=np.uint8))
    return np.stack(out)


def scene_boxes(h, w, exact):
    """(cx, cy, w, h): inside the frame, hanging over each of the four borders, wholly outside (twice), degenerate (four ways): 12 boxes.

    exact=True: sides 7 * 2^a (7 .. 112 px: the scale side / 64 = 7 * 2^(a-6) and side / 224 = 2^(a-5) has at most three mantissa bits for both patch sizes)
    and corners on the 1/8 px grid, so that the fp32 evaluation of the map in csrc/preprocess.hip (m0 * x + m2 with x < 2^8: on a 1/64 px grid, below 2^24) and the
    bilinear sum (weights on a 2^-12 grid times 8-bit levels: 20 bits) are EXACT and must agree with the fp64 restatement bit for bit.  exact=False: arbitrary
    boxes; there the existing kernel's fp32 coordinates may move a value across a rounding tie, which the preprocessing tests pin at one level."""
    if exact:
        s = [28.0, 14.0, 56.0, 7.0, 112.0, 28.0, 14.0]
        boxes = [(w / 2 + 0.5, h / 2 - 0.25, s[0], s[0]), (3.0, h / 2, s[1], s[2]), (w - 2.5, h / 2 + 1, s[2], s[1]), (w / 2, 1.125, s[3], s[3]),
                 (w / 2 - 3, h - 4.0, s[4], s[4]), (-200.0, -100.0, s[5], s[5]), (w + 300.0, h + 40.0, s[6], s[6])]
    else:
        boxes = [(w * 0.51, h * 0.47, w * 0.31, h * 0.37), (5.3, h * 0.5, 50.7, 61.1), (w - 3.1, h * 0.4, 40.9, 60.2), (w * 0.45, 3.3, 30.1, 30.1),
                 (w * 0.5, h - 2.2, 44.4, 47.7), (-200.5, -200.25, 50.3, 50.3), (w + 333.3, h + 77.7, 30.3, 30.3)]
    boxes += [(w / 2, h / 2, 0.0, 10.0), (np.nan, h / 2, 20.0, 20.0), (10.0, 10.0, -5.0, 5.0), (w / 2, h / 2, np.inf, 20.0), (w / 2, h / 2, 28.0, 56.0) if exact else (w / 2, h / 2, 24.3, 40.7)]
    return np.array(boxes, dtype=np.float32)


def packed_from_tables(t, frames, T, H, W):
    """the data.PackedClips that tests/_preprocess_ref.packed_reference restates: the tables as they came back + the same whole frames"""
    from maed_amd import data as D
    M = len(t["frame_i"])
    assert M % T == 0
    N = M // T
    off = D.table_offsets(N, T)
    px = np.ascontiguousarray(frames).reshape(-1)
    blob = torch.zeros(off[4] + px.size, dtype=torch.uint8)
    p = D.PackedClips(blob, px.size, N, T, H, W)
    p.frame_i[:], p.frame_minv[:], p.clip_i[:], p.clip_f[:] = t["frame_i"], t["frame_minv"], t["clip_i"], t["clip_f"]
    blob.numpy()[off[4]:] = px
    return p


# ---- the driver --------------------------------------------------------------------------------------------------------------------------------------------
class StandInModel(nn.Module):
    """MAED.forward's contract on a few linear maps of the pooled crop: deterministic, any device, every output depends on the pixels of its own frame only"""

    def __init__(self, n_verts=12):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.n_verts = n_verts
        self.register_buffer("w", torch.randn(3 * 4 * 4, 85 + n_verts * 3 + 49 * 5, generator=g) * 0.2)

    def forward(self, x, J_regressor=None):
        n, t = x.shape[:2]
        feat = torch.nn.functional.adaptive_avg_pool2d(x.reshape(n * t, *x.shape[2:]), 4).reshape(n * t, -1) @ self.w
        V = self.n_verts
        theta = feat[:, :85].clone()
        theta[:, 0] = 0.8 + 0.1 * torch.tanh(theta[:, 0])             # a plausible camera scale
        return dict(theta=theta.reshape(n, t, 85), verts=feat[:, 85:85 + 3 * V].reshape(n, t, V, 3), kp_3d=feat[:, 85 + 3 * V:85 + 3 * V + 147].reshape(n, t, 49, 3),
                    kp_2d=feat[:, 85 + 3 * V + 147:].reshape(n, t, 49, 2), rotmat=torch.zeros(n, t, 24, 3, 3, device=x.device))


def driver_scene(seed=3, B=26, h=96, w=128, J=25):
    """two people in B frames of h x w: 'kp' has joints2d over 21 frames (3 .. 23) with a gap of two frames, 'box' has bbox over 16 frames (0 .. 15); nobody is
    in frames 24 and 25"""
    rng = np.random.default_rng(seed)
    frames = scene_frames(seed, B, h, w)
    n = 21
    kp = np.zeros((n, J, 3), dtype=np.float32)
    for i in range(n):
        c = np.array([40.0 + 2 * i, 48.0 + 0.5 * i])
        kp[i, :, :2] = c + rng.uniform(-0.5, 0.5, (J, 2)) * np.array([30.0, 60.0])
        kp[i, :, 2] = rng.uniform(0.5, 1.0, J)
    kp[7:9, :, 2] = 0.01
    bbox = np.stack([np.linspace(90, 70, 16), np.full(16, 50.0), np.full(16, 48.0), np.full(16, 48.0)], axis=1).astype(np.float32)
    tracks = {"kp": dict(frames=np.arange(3, 3 + n), joints2d=kp), "box": dict(frames=np.arange(16), bbox=bbox)}
    return frames, tracks


def check_driver(results, skipped, dbg, model, tracks, h, w):
    """acceptance 8 on what VideoInference.run returned with debug=True: every output equals a hand-driven model(clips) on the driver's own crop tensors, padded slots
    dropped; orig_cam = convert_crop_cam_to_orig_img of those values"""
    from maed_amd.render import convert_crop_cam_to_orig_img
    assert not skipped and set(results) == set(tracks)
    persons = list(results)
    model.eval()
    runs = []
    with torch.no_grad():
        for _ in range(2):
            want = {p: {} for p in persons}
            for c, clips in zip(dbg["chunks"], dbg["clips"]):
                out = model(clips)
                for n, (pi, wi, real) in enumerate(c["windows"]):
                    want[persons[pi]][wi] = {k: out[k][n, :real] for k in ("theta", "verts")}
            runs.append(want)
    figures = {}
    for p in persons:
        r = results[p]
        n = len(tracks[p]["frames"])
        assert np.array_equal(r["frame_ids"], np.asarray(tracks[p]["frames"])), p          # (both tracks are valid from their first to their last frame)
        theta, verts = ([torch.cat([want[p][wi][k] for wi in sorted(want[p])]).float() for want in runs] for k in ("theta", "verts"))
        assert theta[0].shape[0] == n and r["verts"].shape[0] == n, (p, theta[0].shape)    # the padded slots never reach the results
        for name, a, b in (("pred_cam", r["pred_cam"], [t[:, :3] for t in theta]), ("pose", r["pose"], [t[:, 3:75] for t in theta]),
                           ("betas", r["betas"], [t[:, 75:] for t in theta]), ("verts", r["verts"], verts)):
            assert a.shape == b[0].shape, (p, name)
            # bit-equal where the forward is bit-identical from run to run (spread 0); otherwise four times the spread of two hand-driven runs
            spread = float((b[0].double() - b[1].double()).abs().max())
            d = float((a.double() - b[0].double()).abs().max())
            figures[f"{p}.{name}"] = (d, spread)
            print(f"{p}.{name}: max difference to the hand-driven forward {d:.3e}, spread of two hand-driven runs {spread:.3e}")
            assert bool(torch.isfinite(a).all()) and d <= 4 * spread, (p, name, d, spread)
        oc = convert_crop_cam_to_orig_img(r["pred_cam"], r["bboxes"], w, h)
        assert torch.equal(r["orig_cam"], oc) and tuple(r["bboxes"].shape) == (n, 4) and bool(torch.isfinite(r["orig_cam"]).all()), p
        assert r["joints3d"].shape[0] == n and r["joints2d"].shape[0] == n
    return figures
