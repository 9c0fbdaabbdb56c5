"""TEST INFRASTRUCTURE for the clip-preprocessing tests: numpy restatements of what csrc/preprocess.hip has to compute, a seeded generator of source
frames / crop parameters, and a runner that drives the C-ABI entry point from numpy arrays (simulator) or device tensors (GPU).

  warp_fp64        the definition of the crop: inverse map of the integer pixel grid, bilinear weights, zero outside, round to nearest -- in fp64.
                   (cv2.warpAffine additionally snaps coordinates to 1/32 px and uses 15-bit weights: agreement with THAT rounding is unpinned.)
  jitter_u8        the four uint8 -> uint8 operations as PIL computes them (ImageEnhance's blend in fp32; the C RGB <-> HSV rows)
  normalise_f32    (u8 / 255 - mean) / std in fp32
"""
import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
F32 = np.float32


def warp_fp64(region, minv, H, W):
    region = np.asarray(region)
    h, w = region.shape[:2]
    m = np.asarray(minv, dtype=np.float64).reshape(2, 3)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    sx = m[0, 0] * x + m[0, 1] * y + m[0, 2]
    sy = m[1, 0] * x + m[1, 1] * y + m[1, 2]
    x0, y0 = np.floor(sx), np.floor(sy)
    ax, ay = (sx - x0)[..., None], (sy - y0)[..., None]

    def tap(xi, yi):
        ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        v = region[np.clip(yi, 0, h - 1).astype(np.int64), np.clip(xi, 0, w - 1).astype(np.int64)].astype(np.float64)
        return v * ok[..., None]

    v = (1 - ax) * (1 - ay) * tap(x0, y0) + ax * (1 - ay) * tap(x0 + 1, y0) + (1 - ax) * ay * tap(x0, y0 + 1) + ax * ay * tap(x0 + 1, y0 + 1)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def grey(img):
    i = img.astype(np.int64)
    return (19595 * i[..., 0] + 38470 * i[..., 1] + 7471 * i[..., 2] + 0x8000) >> 16


def blend(deg, f, img):
    """PIL's Image.blend(degenerate, image, f) on uint8: fp32 arithmetic, clipped, truncated"""
    t = deg.astype(F32) + F32(f) * (img.astype(np.int64) - deg.astype(np.int64)).astype(F32)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def hue_shift(img, shift):
    """RGB -> HSV, H + shift modulo 256, HSV -> RGB with the rounding of PIL's C rows: float quotients, the fold and the 0..255 scaling in double"""
    i = img.astype(np.int64)
    r, g, b = i[..., 0], i[..., 1], i[..., 2]
    maxc, minc = i.max(-1), i.min(-1)
    flat = maxc == minc
    cr = np.where(flat, 1, maxc - minc).astype(F32)
    s = cr / np.maximum(maxc, 1).astype(F32)
    rc, gc, bc = ((maxc - c).astype(F32) / cr for c in (r, g, b))
    d = np.float64
    h = np.where(r == maxc, (bc - gc).astype(F32), np.where(g == maxc, (2.0 + rc.astype(d) - bc.astype(d)).astype(F32), (4.0 + gc.astype(d) - rc.astype(d)).astype(F32)))
    h = np.fmod(h.astype(d) / 6.0 + 1.0, 1.0).astype(F32)
    uh = np.where(flat, 0, np.clip((h.astype(d) * 255.0).astype(np.int64), 0, 255))
    us = np.where(flat, 0, np.clip((s.astype(d) * 255.0).astype(np.int64), 0, 255))
    uv = maxc
    uh = (uh + int(shift)) & 255
    h6 = uh.astype(F32).astype(d) * 6.0 / 255.0
    k = np.floor(h6).astype(np.int64)
    f = (h6 - k.astype(F32).astype(d)).astype(F32).astype(d)
    fs = (us.astype(F32).astype(d) / 255.0).astype(F32).astype(d)
    v = uv.astype(d)
    rnd = lambda a: np.clip(np.where(a >= 0, np.floor(a + 0.5), np.ceil(a - 0.5)).astype(np.int64), 0, 255)     # C round(): half away from zero
    p, q, t = rnd(v * (1.0 - fs)), rnd(v * (1.0 - fs * f)), rnd(v * (1.0 - fs * (1.0 - f)))
    k = k % 6
    R = np.choose(k, [uv, q, p, p, t, uv])
    G = np.choose(k, [t, uv, uv, q, p, p])
    B = np.choose(k, [p, p, t, uv, uv, q])
    out = np.stack([R, G, B], -1)
    out[us == 0] = uv[us == 0][:, None]
    return out.astype(np.uint8)


def jitter_u8(img, order, brightness=1.0, saturation=1.0, contrast=1.0, shift=0):
    """operation codes of maed_amd/data.py (1 brightness, 2 saturation, 3 hue, 4 contrast) applied in `order`, uint8 after each"""
    img = np.asarray(img, dtype=np.uint8)
    for op in order:
        if op == 1:
            img = blend(np.zeros_like(img), brightness, img)
        elif op == 2:
            img = blend(np.repeat(grey(img)[..., None], 3, -1), saturation, img)
        elif op == 3:
            img = hue_shift(img, shift)
        elif op == 4:
            m = int(grey(img).sum() / grey(img).size + 0.5)
            img = blend(np.full_like(img, m), contrast, img)
    return img


def normalise_f32(img_u8, mean=MEAN, std=STD):
    x = img_u8.astype(F32) / F32(255.0)
    return ((x - mean.astype(F32)) / std.astype(F32)).astype(F32).transpose(2, 0, 1)


def chain_ref(patch_u8, order=(), brightness=1.0, saturation=1.0, contrast=1.0, shift=0, erase_top=0, erase_bot=0, flip=False):
    """everything after the warp, on one uint8 patch -> fp32 (3, H, W)"""
    img = jitter_u8(patch_u8, order, brightness, saturation, contrast, shift).copy()
    H = img.shape[0]
    if erase_top:
        img[:erase_top] = 0
    if erase_bot:
        img[H - min(erase_bot, H):] = 0
    if flip:
        img = img[:, ::-1]
    return normalise_f32(img)


def identity_tables(patches, clip_of=None, n_clips=1):
    """parameter tables + packed pixels for patches that are already the crop (identity map): the post-warp stages in isolation.
    Returns dict(src, frame_i, frame_minv, clip_i, clip_f) of numpy arrays; the caller fills clip_i / clip_f / the erase columns."""
    F = len(patches)
    H, W = patches[0].shape[:2]
    src = np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in patches])
    frame_i = np.zeros((F, 8), dtype=np.int32)
    for f in range(F):
        frame_i[f, :5] = (f * H * W * 3, H, W, W * 3, 0 if clip_of is None else clip_of[f])
    frame_minv = np.tile(np.array([1, 0, 0, 0, 1, 0], dtype=np.float32), (F, 1))
    return dict(src=src, frame_i=frame_i, frame_minv=frame_minv, clip_i=np.zeros((n_clips, 8), dtype=np.int32),
                clip_f=np.tile(np.array([1, 1, 0, 1], dtype=np.float32), (n_clips, 1)))


def random_scene(seed, n_clips, T, H, W, lo=100, hi=900, jitter=True):
    """seeded frames + ClipParams with region sizes spread over roughly lo..hi px (bbox side; coordinates stay below 1024 px), some bboxes hanging over
    the image border.  Frames are smooth + noise so that a wrong tap or weight moves many levels."""
    from maed_amd import data as D
    rng = np.random.default_rng(seed)
    frames, records = [], []
    for n in range(n_clips):
        side = float(np.exp(rng.uniform(np.log(lo), np.log(hi))))
        ih, iw = int(rng.integers(480, 1000)), int(rng.integers(640, 1000))
        y, x = np.mgrid[0:ih, 0:iw]
        base = np.stack([(x * 3 + y) % 256, (x + y * 2) % 256, (x * y // 64) % 256], -1).astype(np.uint8)
        clip, boxes = [], []
        for t in range(T):
            img = base ^ rng.integers(0, 32, (ih, iw, 1), dtype=np.uint8)
            clip.append(img)
            boxes.append([rng.uniform(0, iw), rng.uniform(0, ih), side / 1.3 * rng.uniform(0.9, 1.1), side / 1.3 * rng.uniform(0.9, 1.1)])
        rec = D.ClipParams(bboxes=np.array(boxes), scale=(1.3 * rng.uniform(0.8, 1.2),) * 2, rot=float(rng.uniform(-30, 30)),
                           shift=(float(rng.uniform(-0.1, 0.1)), float(rng.uniform(-0.1, 0.1))))
        if jitter:
            rec.brightness, rec.saturation, rec.contrast = (float(v) for v in rng.uniform(0.7, 1.3, 3))
            rec.hue = float(rng.uniform(-0.3, 0.3))
            rec.jitter_order = D.JITTER_ORDERS[int(rng.integers(24))]
            rec.erase_side = int(rng.integers(4))
            rec.erase_ratio = np.where(rng.random(T) < 0.3, rng.random(T) * 0.7, 0.0)
            rec.flip = bool(rng.random() < 0.5)
        frames.append(clip)
        records.append(rec)
    return frames, records


def packed_reference(packed, warp_tolerant=False):
    """fp32 (F, 3, H, W) the chain must give for a data.PackedClips, from the fp64 warp + the uint8 restatements; also the uint8 patches"""
    from maed_amd import data as D
    F = packed.N * packed.T
    raw = packed.blob.numpy()
    px = raw[packed.offsets[4]:]
    outs, patches = [], []
    for f in range(F):
        off, h, w, pitch, c, et, eb = (int(v) for v in packed.frame_i[f, :7])
        region = px[off:off + h * pitch].reshape(h, w, 3)
        patch = warp_fp64(region, packed.frame_minv[f].astype(np.float64), packed.H, packed.W)
        ci, cf = packed.clip_i[c], packed.clip_f[c]
        order = [int(o) for o in ci[1:5] if o]
        patches.append(patch)
        outs.append(chain_ref(patch, order, cf[0], cf[1], cf[3], int(ci[5]), et, eb, bool(ci[0])))
    return np.stack(outs), np.stack(patches)


def to_levels(out_f32, mean=MEAN, std=STD):
    """normalised fp32 (…, 3, H, W) back to uint8 levels (exact: the levels are 1/255 apart, the rounding error ~1e-7)"""
    x = out_f32.astype(np.float64) * std.astype(np.float64)[:, None, None] + mean.astype(np.float64)[:, None, None]
    return np.rint(x * 255.0).astype(np.int64)
