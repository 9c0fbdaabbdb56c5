"""Clip preprocessing: the reference's transform chain (train.py:41-70, lib/data_utils/transforms/*.py) with the pixels on the device.

    aug = ClipAugment(rot_jitter=..., color_jitter=..., erase_prob=..., flip_p=..., seed=...)   # the reference's config names
    rec = aug.sample(bboxes)                     # one clip's random draws, a plain record (every field can be set by hand)
    tgt = aug.targets(rec, kp_2d, kp_3d, pose)   # the target side, numpy on the host (a few hundred floats per clip)
    packed = pack_clips(frames, records)         # source regions -> one pinned uint8 buffer + the parameter tables
    clip = preprocess_clips(packed)              # (N, T, 3, H, W) fp32 on the device: what MAED.forward takes

Random numbers are drawn on the host (a dozen scalars per clip); pixels are only touched by csrc/preprocess.hip.  The reference's random
STREAM is not reproduced (it mixes `random` and `numpy.random`); its distributions and their per-clip / per-frame granularity are.
"""
import dataclasses
import itertools

import numpy as np
import torch

from . import ops
from ._lib import MaedHipError

OP_NONE, OP_BRIGHTNESS, OP_SATURATION, OP_HUE, OP_CONTRAST = range(5)
ERASE_LEFT, ERASE_RIGHT, ERASE_TOP, ERASE_BOTTOM = range(4)       # the order of random_erase.py:128's choice list
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
JITTER_ORDERS = tuple(itertools.permutations((OP_BRIGHTNESS, OP_SATURATION, OP_HUE, OP_CONTRAST)))

# left / right exchange of the 49 SPIN joints and of the 24 SMPL joints (the published tables of SPIN's constants.py; kp_utils.py builds the same ones from names)
SPIN_FLIP_PERM = (0, 1, 5, 6, 7, 2, 3, 4, 8, 12, 13, 14, 9, 10, 11, 16, 15, 18, 17, 22, 23, 24, 19, 20, 21, 30, 29, 28, 27, 26, 25, 36, 35, 34, 33, 32, 31,
                  37, 38, 39, 40, 41, 42, 43, 44, 46, 45, 48, 47)
SMPL_FLIP_PERM = (0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 11, 10, 12, 14, 13, 15, 17, 16, 19, 18, 21, 20, 23, 22)


@dataclasses.dataclass
class ClipParams:
    """one clip's draws.  bboxes (T, 4) = (cx, cy, w, h) per frame; scale / rot / shift, the jitter, the erase side and the flip once per clip;
    erase_ratio per frame (0 = that frame is not erased).  jitter_order lists operation codes in the order applied, () = no jitter."""
    bboxes: np.ndarray
    scale: tuple = (1.3, 1.3)
    rot: float = 0.0
    shift: tuple = (0.0, 0.0)
    brightness: float = 1.0
    contrast: float = 1.0
    saturation: float = 1.0
    hue: float = 0.0
    jitter_order: tuple = ()
    erase_side: int = ERASE_LEFT
    erase_ratio: np.ndarray = None
    flip: bool = False


def hue_shift_levels(hue):
    """what torchvision's PIL path adds to the H channel: uint8(hue * 255), i.e. truncation toward zero, modulo 256"""
    return int(hue * 255) & 255


def gen_trans(bbox, scale, rot, shift, patch_width, patch_height):
    """crop.py:57-86: the 2 x 3 source -> patch matrix from three point pairs (centre, centre + down, centre + right; the points rounded to fp32 as the
    reference stores them, the solve in fp64)"""
    bbox = np.asarray(bbox, dtype=np.float64)
    src_w, src_h = bbox[2] * scale[0], bbox[3] * scale[1]
    center = bbox[:2] + bbox[2:] * np.asarray(shift, dtype=np.float64)
    rad = np.pi * rot / 180
    sn, cs = np.sin(rad), np.cos(rad)

    def rotate(pt):
        x, y = np.float64(np.float32(pt[0])), np.float64(np.float32(pt[1]))
        return np.array([x * cs - y * sn, x * sn + y * cs], dtype=np.float32)

    src = np.zeros((3, 2), dtype=np.float32)
    src[0] = center
    src[1] = center + rotate((0, src_h * 0.5))
    src[2] = center + rotate((src_w * 0.5, 0))
    dst = np.zeros((3, 2), dtype=np.float32)
    dst_c = np.array([patch_width * 0.5, patch_height * 0.5], dtype=np.float32)
    dst[0] = dst_c
    dst[1] = dst_c + np.array([0, patch_height * 0.5], dtype=np.float32)
    dst[2] = dst_c + np.array([patch_width * 0.5, 0], dtype=np.float32)
    A = np.concatenate([src.astype(np.float64), np.ones((3, 1))], axis=1)
    return np.linalg.solve(A, dst.astype(np.float64)).T


def invert_affine(trans):
    """patch -> source map of a 2 x 3 source -> patch matrix (what cv2.warpAffine samples at)"""
    full = np.concatenate([np.asarray(trans, dtype=np.float64), [[0.0, 0.0, 1.0]]], axis=0)
    return np.linalg.inv(full)[:2]


def trans_keypoints(kp_2d, trans):
    """crop.py:94-105: (x, y) through the forward matrix, the remaining columns untouched"""
    kp_2d = np.asarray(kp_2d)
    out = np.array(kp_2d, dtype=np.result_type(kp_2d.dtype, np.float64))
    xy1 = np.concatenate([kp_2d[..., :2].astype(np.float64), np.ones(kp_2d.shape[:-1] + (1,))], axis=-1)
    out[..., :2] = xy1 @ np.asarray(trans, dtype=np.float64).T
    return out.astype(kp_2d.dtype) if kp_2d.dtype.kind == "f" else out


def keypoint_2d_hflip(kp_2d, img_width):
    """kp_utils.py:25-40 on (T, 49, C)"""
    out = np.asarray(kp_2d, dtype=np.float64)[:, list(SPIN_FLIP_PERM)].copy()
    out[:, :, 0] = (img_width - 1.) - out[:, :, 0]
    return out


def keypoint_3d_hflip(kp_3d):
    """kp_utils.py:43-61 on (T, 49, C): x mirrored about the pelvis (midpoint of joints 27, 28); like the reference, every column goes through the
    subtract / add of the pelvis row"""
    out = np.asarray(kp_3d, dtype=np.float64)[:, list(SPIN_FLIP_PERM)].copy()
    pelvis = (out[:, 27, :] + out[:, 28, :]) / 2
    out = out - pelvis[:, None, :]
    out[:, :, 0] = -out[:, :, 0]
    out += pelvis[:, None, :]
    return out


def smpl_pose_hflip(pose):
    """kp_utils.py:63-80 on (T, 72): left / right joints exchanged, the y and z components of each axis-angle negated.  The reference's loop stops one joint
    short (range(24 - 1)), so joint 23 keeps its own, unmirrored rotation; reproduced."""
    orig = np.asarray(pose).reshape(-1, 24, 3)
    out = orig.copy()
    perm = list(SMPL_FLIP_PERM[:23])
    out[:, :23, 0] = orig[:, perm, 0]
    out[:, :23, 1:] = -orig[:, perm, 1:]
    return out.reshape(-1, 72)


def normalize_2d_kp(kp_xy, patch_size=224):
    """basic.py:14-19"""
    return 2.0 * kp_xy * (1.0 / patch_size) - 1.0


class ClipAugment:
    """The reference's augmentation knobs under its config names (DATASET.ROT_JITTER, SIZE_JITTER, RANDOM_CROP_P, RANDOM_CROP_SIZE, COLOR_JITTER, ERASE_PROB,
    ERASE_PART, ERASE_FILL, ERASE_KP, ERASE_MARGIN, RANDOM_FLIP).  color_jitter > 0 = the 3D stream's ColorJitterVideo with that one value for all four."""

    def __init__(self, patch_height=224, patch_width=224, rot_jitter=0., size_jitter=0., random_crop_p=0., random_crop_size=0.5, color_jitter=0.,
                 erase_prob=0., erase_part=0.5, erase_fill=False, erase_kp=False, erase_margin=0.1, flip_p=0.5, seed=None,
                 mean=IMAGENET_MEAN, std=IMAGENET_STD):
        if erase_fill:
            raise NotImplementedError("maed_amd/data.py ClipAugment.__init__: ERASE_FILL=True (random filling, random_erase.py:26-28) is not built: "
                                      "both shipped configs use zero fill")
        if erase_kp:
            raise NotImplementedError("maed_amd/data.py ClipAugment.__init__: ERASE_KP=True is not built (the reference's branch, random_erase.py:31-36, "
                                      "writes kp_2d[2] and reads an undefined `t`); both shipped configs use False")
        self.patch_height, self.patch_width = int(patch_height), int(patch_width)
        self.rot_jitter, self.size_jitter = rot_jitter, size_jitter
        self.random_crop_p, self.random_crop_size = random_crop_p, random_crop_size
        self.color_jitter = color_jitter
        self.erase_prob, self.erase_part, self.erase_margin = erase_prob, erase_part, erase_margin
        self.flip_p = flip_p
        self.mean, self.std = tuple(mean), tuple(std)
        self.rng = np.random.default_rng(seed)

    @classmethod
    def eval(cls, patch_height=224, patch_width=224, **kw):
        """transforms_val (train.py:64-69): crop at scale 1.3, to-tensor, normalise"""
        return cls(patch_height, patch_width, flip_p=0., **kw)

    def sample(self, bboxes):
        """one clip's draws with the reference's distributions: crop.py:38-47 (per clip), color_jitter.py:14-37 + the shuffle of :81 (per clip),
        random_erase.py:128 (side per clip) and :132-133 (probability and ratio per FRAME), random_hflip.py:102 (per clip)"""
        r = self.rng
        bboxes = np.asarray(bboxes, dtype=np.float64).reshape(-1, 4)
        T = len(bboxes)
        scale = r.uniform(1.3 - self.size_jitter, 1.3 + self.size_jitter)
        rot = r.uniform(-self.rot_jitter, self.rot_jitter)
        shift = (0.0, 0.0)
        if r.random() < self.random_crop_p:
            scale = r.uniform(1.3 - self.random_crop_size, 1.3)
            half = (1.3 - scale) / 2.0
            shift = (r.uniform(-half, half), r.uniform(-half, half))
        rec = ClipParams(bboxes=bboxes, scale=(scale, scale), rot=rot, shift=shift)
        cj = self.color_jitter
        if cj > 0:
            rec.brightness = r.uniform(max(0, 1 - cj), 1 + cj)
            rec.contrast = r.uniform(max(0, 1 - cj), 1 + cj)
            rec.saturation = r.uniform(max(0, 1 - cj), 1 + cj)
            rec.hue = r.uniform(-cj, cj)
            rec.jitter_order = JITTER_ORDERS[int(r.integers(len(JITTER_ORDERS)))]
        rec.erase_side = int(r.integers(4))
        hit = r.random(T) < self.erase_prob
        rec.erase_ratio = np.where(hit, r.random(T) * self.erase_part, 0.0)
        rec.flip = bool(r.random() < self.flip_p)
        return rec

    def matrices(self, rec):
        """(T, 2, 3) source -> patch matrices of a clip"""
        return np.stack([gen_trans(b, rec.scale, rec.rot, rec.shift, self.patch_width, self.patch_height) for b in np.asarray(rec.bboxes).reshape(-1, 4)])

    def erase_rows(self, rec):
        """(T, 2) rows blanked at the top / bottom of each frame.  random_erase.py:23-87: top / bottom take int(h * ratio) rows; `_erase_left` / `_erase_right`
        index the first axis too, so they blank int(w * ratio) ROWS at the top / bottom."""
        T = len(np.asarray(rec.bboxes).reshape(-1, 4))
        ratio = np.zeros(T) if rec.erase_ratio is None else np.asarray(rec.erase_ratio, dtype=np.float64)
        if len(ratio) != T:
            raise ValueError(f"erase_ratio has {len(ratio)} entries for {T} frames")
        extent = self.patch_width if rec.erase_side in (ERASE_LEFT, ERASE_RIGHT) else self.patch_height
        n = np.minimum((extent * ratio).astype(np.int64), self.patch_height)
        out = np.zeros((T, 2), dtype=np.int32)
        out[:, 0 if rec.erase_side in (ERASE_LEFT, ERASE_TOP) else 1] = n
        return out

    def targets(self, rec, kp_2d=None, kp_3d=None, pose=None, normalize=True):
        """the target side of the chain on the host: kp_2d (T, 49, 3) through the crop matrices, then the three flips, then kp_2d[..., :2] -> 2 kp / patch - 1
        (NormalizeVideo's default patch_size 224, as train.py constructs it)"""
        out = {}
        if kp_2d is not None:
            M = self.matrices(rec)
            kp = np.stack([trans_keypoints(k, m) for k, m in zip(np.asarray(kp_2d), M)])
            if rec.flip:
                kp = keypoint_2d_hflip(kp, self.patch_width)
            if normalize:
                kp = np.array(kp, dtype=np.float64)
                kp[..., :2] = normalize_2d_kp(kp[..., :2], 224)
            out["kp_2d"] = kp
        if kp_3d is not None:
            out["kp_3d"] = keypoint_3d_hflip(kp_3d) if rec.flip else np.asarray(kp_3d)
        if pose is not None:
            out["pose"] = smpl_pose_hflip(pose) if rec.flip else np.asarray(pose)
        return out


def table_offsets(N, T):
    """byte offsets of (frame_i, frame_minv, clip_i, clip_f, pixels) in a packed buffer of N clips of T frames: the layout is a function of (N, T) alone"""
    F = N * T
    o_fm = F * 32
    o_ci = o_fm + F * 24
    o_cf = o_ci + N * 32
    return 0, o_fm, o_ci, o_cf, (o_cf + N * 16 + 255) // 256 * 256


@dataclasses.dataclass
class PackedClips:
    """what pack_clips hands to preprocess_clips: ONE uint8 host buffer = [frame_i | frame_minv | clip_i | clip_f | pixels] and its extents.  The four tables are
    numpy VIEWS of that buffer, made on demand: writing to `packed.clip_f[0, 0]` changes what the kernel reads, also after the record went through pickle or a
    DataLoader worker (the tensor travels, the views are rebuilt on the other side).  Nothing here touches the GPU runtime, so a loader worker can build one;
    pin_memory() -- which `DataLoader(pin_memory=True)` calls in the MAIN process -- moves the buffer into page-locked memory for a non-blocking upload."""
    blob: torch.Tensor
    src_bytes: int
    N: int
    T: int
    H: int
    W: int
    mean: tuple = IMAGENET_MEAN
    std: tuple = IMAGENET_STD

    @property
    def offsets(self):
        return table_offsets(self.N, self.T)

    def _table(self, k, dtype, cols):
        rows = self.N * self.T if k < 2 else self.N
        o = self.offsets[k]
        if self.blob.dtype != torch.uint8 or self.blob.dim() != 1 or o + rows * cols * 4 > self.blob.numel():
            raise MaedHipError(f"preprocess_clips: the packed buffer ({self.blob.numel()} bytes) is too short for the tables of {self.N} clips of {self.T} frames")
        return self.blob.numpy()[o:o + rows * cols * 4].view(dtype).reshape(rows, cols)

    frame_i = property(lambda self: self._table(0, np.int32, 8))        # int32 (F, 8)   include/maed_hip.h maed_clip_preprocess
    frame_minv = property(lambda self: self._table(1, np.float32, 6))   # fp32 (F, 6)
    clip_i = property(lambda self: self._table(2, np.int32, 8))         # int32 (N, 8)
    clip_f = property(lambda self: self._table(3, np.float32, 4))       # fp32 (N, 4)

    @property
    def has_contrast(self):
        return bool((self.clip_i[:, 1:5] == OP_CONTRAST).any())

    def pin_memory(self):
        return dataclasses.replace(self, blob=self.blob.pin_memory())


def source_region(minv, img_h, img_w, H, W):
    """axis-aligned bounding rectangle (x0, y0, x1, y1, inclusive) of every bilinear tap of an H x W patch, clamped to the image.  One pixel of margin on each
    side covers the kernel's fp32 coordinates (tests keep coordinates below 1024 px, error ~6e-5 px).  Never empty: a quad wholly outside the image clamps to
    the nearest border row / column, whose taps then all carry zero weight or lie outside the region."""
    cx = np.array([0.0, W - 1.0, 0.0, W - 1.0])
    cy = np.array([0.0, 0.0, H - 1.0, H - 1.0])
    sx = minv[0, 0] * cx + minv[0, 1] * cy + minv[0, 2]
    sy = minv[1, 0] * cx + minv[1, 1] * cy + minv[1, 2]
    if not (np.isfinite(sx).all() and np.isfinite(sy).all()):
        raise ValueError("non-finite crop matrix (a bbox of zero size?)")
    clampi = lambda v, hi: int(min(max(v, 0.0), hi))
    x0, x1 = clampi(np.floor(sx.min()) - 1, img_w - 1), clampi(np.floor(sx.max()) + 2, img_w - 1)
    y0, y1 = clampi(np.floor(sy.min()) - 1, img_h - 1), clampi(np.floor(sy.max()) + 2, img_h - 1)
    return x0, y0, x1, y1


def pack_clips(frames, records, aug=None, patch_height=None, patch_width=None, mean=None, std=None, pin=False):
    """frames: N clips of T uint8 (h, w, 3) RGB arrays (any size per frame); records: N ClipParams.  Slices each frame's source region (a numpy view, no
    resampling), copies it into one staging buffer and fills the parameter tables.  `aug` supplies the patch size and the normalisation.  Pure host work: safe in
    a DataLoader worker.  pin=True page-locks the buffer here (that initialises the GPU runtime in THIS process: main process only); otherwise pin it with
    PackedClips.pin_memory() / DataLoader(pin_memory=True), or leave it pageable and pay a blocking upload."""
    H = int(patch_height or (aug.patch_height if aug else 224))
    W = int(patch_width or (aug.patch_width if aug else 224))
    aug = aug or ClipAugment(H, W)
    if (aug.patch_height, aug.patch_width) != (H, W):
        aug = ClipAugment(H, W, mean=aug.mean, std=aug.std)
    N = len(frames)
    if N == 0 or len(records) != N:
        raise ValueError(f"{len(records)} records for {N} clips")
    T = len(frames[0])
    F = N * T
    regions, total = [], 0
    minv_all = np.zeros((F, 6), dtype=np.float64)
    erase = np.zeros((F, 2), dtype=np.int32)
    for n, (clip, rec) in enumerate(zip(frames, records)):
        if len(clip) != T or len(np.asarray(rec.bboxes).reshape(-1, 4)) != T:
            raise ValueError(f"clip {n}: every clip needs {T} frames and {T} bboxes")
        M = aug.matrices(rec)
        erase[n * T:(n + 1) * T] = aug.erase_rows(rec)
        for t, img in enumerate(clip):
            if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
                raise ValueError(f"clip {n} frame {t}: expected a uint8 (h, w, 3) array")
            minv = invert_affine(M[t])
            x0, y0, x1, y1 = source_region(minv, img.shape[0], img.shape[1], H, W)
            minv[:, 2] -= (x0, y0)
            minv_all[n * T + t] = minv.reshape(6)
            regions.append((img[y0:y1 + 1, x0:x1 + 1], total))
            total += (y1 - y0 + 1) * (x1 - x0 + 1) * 3
    o_px = table_offsets(N, T)[4]
    packed = PackedClips(torch.empty(o_px + total, dtype=torch.uint8), total, N, T, H, W, tuple(mean or aug.mean), tuple(std or aug.std))
    raw = packed.blob.numpy()
    frame_i, frame_minv, clip_i, clip_f = packed.frame_i, packed.frame_minv, packed.clip_i, packed.clip_f
    raw[:o_px] = 0
    frame_i[:] = 0
    clip_i[:] = 0
    frame_minv[:] = minv_all
    for f, (view, off) in enumerate(regions):
        h, w = view.shape[:2]
        raw[o_px + off:o_px + off + h * w * 3].reshape(h, w, 3)[:] = view
        frame_i[f, :7] = (off, h, w, w * 3, f // T, erase[f, 0], erase[f, 1])
    for n, rec in enumerate(records):
        order = tuple(rec.jitter_order)
        if len(order) > 4 or len(set(order)) != len(order) or any(o not in (1, 2, 3, 4) for o in order):
            raise ValueError(f"clip {n}: jitter_order {order} must list each of the operation codes 1..4 at most once")
        clip_i[n, 0] = int(bool(rec.flip))
        clip_i[n, 1:1 + len(order)] = order
        clip_i[n, 5] = hue_shift_levels(rec.hue)
        clip_f[n] = (rec.brightness, rec.saturation, 0.0, rec.contrast)
    return packed.pin_memory() if pin else packed


def validate_packed(p):
    """the checks the kernel cannot make: the buffer is long enough for the tables and pixels its extents announce (the table properties raise otherwise), and
    every region lies inside the pixel part"""
    if min(p.N, p.T, p.H, p.W) < 1 or p.src_bytes < 1:
        raise MaedHipError("preprocess_clips: bad extents")
    fi = p.frame_i.astype(np.int64)
    minv, clip_i, clip_f = p.frame_minv, p.clip_i, p.clip_f
    if p.offsets[4] + p.src_bytes > p.blob.numel():
        raise MaedHipError(f"preprocess_clips: the packed buffer ({p.blob.numel()} bytes) is shorter than its tables and {p.src_bytes} bytes of pixels")
    off, h, w, pitch, clip = fi[:, 0], fi[:, 1], fi[:, 2], fi[:, 3], fi[:, 4]
    if (h < 1).any() or (w < 1).any() or (pitch < 3 * w).any() or (off < 0).any() or (off + (h - 1) * pitch + 3 * w > p.src_bytes).any():
        raise MaedHipError("preprocess_clips: a source region lies outside the packed pixels")
    if (clip < 0).any() or (clip >= p.N).any() or (fi[:, 5:7] < 0).any():
        raise MaedHipError("preprocess_clips: bad clip index or erase row count")
    if ((clip_i[:, 1:5] < 0) | (clip_i[:, 1:5] > 4)).any():
        raise MaedHipError("preprocess_clips: bad jitter operation code")
    if not (np.isfinite(minv).all() and np.isfinite(clip_f).all()):
        raise MaedHipError("preprocess_clips: non-finite parameter")
    if p.W % 4:
        raise MaedHipError(f"preprocess_clips: patch width {p.W} is not a multiple of 4")


def preprocess_clips(packed, out=None, stream=None, device=None, form=ops.PRE_FORM_AUTO):
    """(N, T, 3, H, W) fp32, contiguous, normalised, on the device: MAED.forward's input, no copy or cast in between.  A CPU `out` or device is an error.

    The packed buffer (tables + pixels) is uploaded with ONE copy and the kernels follow it on the same stream: the current stream, or `stream` if given.
    Ordering with `stream=s` is settled here, not left to the caller: the caller's CURRENT stream is made to wait for `s` before the function returns, and
    the result is marked as in use on the current stream (record_stream), so the returned tensor can be consumed on the current stream at once, without an event
    or a host synchronise, and its memory is not recycled under the consumer.  Work queued on the current stream BEFORE the call (the previous train step) is
    not ordered against `s` and overlaps with it.  With `out=` the side stream first waits for the current stream (earlier readers of `out` must be done), which
    gives up that overlap: let the function allocate when overlap is the point.
    What remains the caller's: the upload is asynchronous only from page-locked memory (PackedClips.pin_memory(), DataLoader(pin_memory=True) or
    pack_clips(pin=True)); a pageable buffer is copied with a blocking call.  Do not write to `packed` between this call and the stream reaching the copy; dropping
    it is fine (the framework's pinned allocator keeps the block until the copy ran)."""
    validate_packed(packed)
    if out is not None:
        device = out.device
    elif device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    device = torch.device(device)
    F = packed.N * packed.T
    shape = (packed.N, packed.T, 3, packed.H, packed.W)
    if out is not None and tuple(out.shape) != shape:
        raise MaedHipError(f"preprocess_clips: out is {tuple(out.shape)}, expected {shape}")

    def run():
        blob = packed.blob.to(device, non_blocking=True) if device.type == "cuda" else packed.blob
        o = out if out is not None else torch.empty(shape, dtype=torch.float32, device=device)
        ops.clip_preprocess(blob, packed.offsets, packed.src_bytes, F, packed.N, packed.H, packed.W, packed.mean, packed.std, packed.has_contrast, o, form)
        return o

    if stream is None or device.type != "cuda":
        return run()
    current = torch.cuda.current_stream(device)
    if stream == current:
        return run()
    if out is not None:
        stream.wait_stream(current)
    with torch.cuda.stream(stream):
        o = run()
    current.wait_stream(stream)
    if out is not None:
        o.record_stream(stream)         # allocated on the caller's side, written over there
    else:
        o.record_stream(current)        # allocated in `stream`'s pool, read over here
    return o
