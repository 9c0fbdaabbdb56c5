"""Video inference: person tracks -> smoothed crop boxes -> crops of device-resident frames -> MAED -> per-person results.

    boxes, span = track_boxes(kps, lengths)                      # K padded keypoint tracks on the device (csrc/tracks.hip maed_track_boxes)
    vi = VideoInference(model, seqlen=16, clips_per_batch=8)
    results, skipped = vi.run(frames, tracks)                    # frames uint8 (B, h, w, 3) on the device; tracks {person: {'frames', 'joints2d' | 'bbox'}}
    render_frame_results(frames, prepare_rendering_results(results, B), faces)

and the reference's lib/utils/smooth_bbox.py by name (get_smooth_bbox_params, kp_to_bbox_param, get_all_bbox_params, smooth_bbox_params: lists / numpy in, numpy
out, computed by the same kernel).  The pixels go through the existing clip preprocessing (ops.clip_preprocess); its parameter tables are built on the device by
maed_crop_tables from the boxes, so nothing but the K spans travels to the host before the model runs.  No tracker, detector, decoder or file output lives here;
everything is queued on the current stream.  Definitions, the table contract and the chunking rule: docs/design/17_video_inference.md.
"""
import numpy as np
import torch

from . import _lib as L
from . import data, ops
from .render import convert_crop_cam_to_orig_img

LDS_FRAMES = 1024             # csrc/tracks.hip TRK_LDS_N
MAX_RADIUS = 512
MAX_KEYPOINTS = 64
MAX_CROPS = 65535             # maed_clip_preprocess: the frame index is a 16-bit grid dimension
MAX_SRC_BYTES = 1 << 31       # maed_clip_preprocess: 32-bit source offsets; a chunk of frames stays BELOW this
_IDENTITY_SIGMA = 0.1         # radius int(4 * 0.1 + 0.5) = 0: one weight exp(0) / exp(0) = 1, the Gaussian pass returns its input


def _check_filter(kernel_size, sigma):
    """the argument checks of maed_track_boxes, made here as well so that they read as ValueError before anything is allocated"""
    if int(kernel_size) != kernel_size or kernel_size < 1 or kernel_size > 63 or int(kernel_size) % 2 == 0:
        raise ValueError(f"kernel_size {kernel_size}: the median window must be odd, 1 .. 63")
    if not (sigma > 0):
        raise ValueError(f"sigma {sigma}: must be > 0")
    if int(4.0 * sigma + 0.5) > MAX_RADIUS:
        raise ValueError(f"sigma {sigma} gives a Gaussian radius of {int(4.0 * sigma + 0.5)} samples: at most {MAX_RADIUS}")


def _launch_tracks(kps, series, lengths, vis_thresh, kernel_size, sigma, box_scale, want_params):
    src = kps if kps is not None else series
    K, Lf = int(src.shape[0]), int(src.shape[1])
    dev = src.device
    boxes = torch.empty((K, Lf, 4), dtype=torch.float32, device=dev)
    params = torch.empty((K, Lf, 3), dtype=torch.float64, device=dev) if want_params else None
    span = torch.empty((K, 2), dtype=torch.int32, device=dev)
    lib = L.lib()
    need = int(lib.maed_track_boxes_workspace(K, Lf))
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    if kps is not None:
        L.check(lib.maed_track_boxes(ops._p(kps), ops._p(lengths), K, Lf, int(kps.shape[2]), float(vis_thresh), int(kernel_size), float(sigma), float(box_scale),
                                     ops._p(boxes), ops._p(params), ops._p(span), ops._p(ws), need, ops._stream()), "track_boxes")
    else:
        L.check(lib.maed_track_smooth(ops._p(series), ops._p(lengths), K, Lf, int(kernel_size), float(sigma), float(box_scale), ops._p(boxes), ops._p(params),
                                      ops._p(ws), need, ops._stream()), "track_smooth")
        span[:, 0] = torch.where(lengths > 0, 0, -1)
        span[:, 1] = lengths
    return boxes, span, params


def track_boxes(kps, lengths, vis_thresh=0.3, kernel_size=11, sigma=8, box_scale=1.1, return_params=False):
    """Smoothed crop boxes of K keypoint tracks (lib/utils/smooth_bbox.py:11-123 + lib/data_utils/threedpw_utils.py:103-108), on the device.

    kps fp32 (K, L, J, 3) = x, y, confidence with J <= 64; lengths int32 (K): frames >= lengths[k] of track k are padding.  Returns boxes fp32 (K, L, 4) = cx, cy,
    w, h and span int32 (K, 2) = first frame that has a box, last such frame + 1 -- (-1, 0) and zero rows for a track without one; rows outside the span are zero.
    A span shorter than (kernel_size + 1) / 2 gives infinite boxes (the median's zero padding wins, the smoothed scale is 0): VideoInference skips such tracks.
    return_params=True adds the fp64 (K, L, 3) smoothed cx, cy, scale.  CPU tensors are an error: there is no host path."""
    _check_filter(kernel_size, sigma)
    if not (isinstance(kps, torch.Tensor) and isinstance(lengths, torch.Tensor)):
        raise L.MaedHipError("track_boxes: kps and lengths must be device tensors (no CPU path)")
    if kps.dim() != 4 or kps.shape[3] != 3 or kps.dtype != torch.float32:
        raise ValueError(f"track_boxes: kps must be fp32 (K, L, J, 3), got {kps.dtype} {tuple(kps.shape)}")
    if kps.shape[2] < 1 or kps.shape[2] > MAX_KEYPOINTS:
        raise ValueError(f"track_boxes: {kps.shape[2]} keypoints per frame: at most {MAX_KEYPOINTS}")
    if lengths.dtype != torch.int32 or tuple(lengths.shape) != (kps.shape[0],):
        raise ValueError("track_boxes: lengths must be int32 (K)")
    ops._p(kps), ops._p(lengths)
    boxes, span, params = _launch_tracks(kps.contiguous(), None, lengths.contiguous(), vis_thresh, kernel_size, sigma, box_scale, return_params)
    return (boxes, span, params) if return_params else (boxes, span)


# ---- the reference's functions by name (lists / numpy in, numpy out) --------------------------------------------------------------------------------
def _device():
    """where the numpy-facing functions compute: the current GPU (tests/_hostsim_tracks.patched: host memory stands for it)"""
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def _pack_kps(kps):
    """list of (J, 3) arrays or None -> fp32 (1, L, J, 3) with zero rows (confidence 0) where there is None, and the mask of those rows"""
    shapes = {np.asarray(kp).shape for kp in kps if kp is not None}
    if len(shapes) > 1 or any(len(s) != 2 or s[1] != 3 for s in shapes):
        raise ValueError(f"keypoints must all be (J, 3) arrays of one J, got {sorted(shapes)}")
    J = shapes.pop()[0] if shapes else 1
    out = np.zeros((1, max(len(kps), 1), J, 3), dtype=np.float32)
    none = np.ones(max(len(kps), 1), dtype=bool)
    for i, kp in enumerate(kps):
        if kp is not None:
            out[0, i] = np.asarray(kp, dtype=np.float32)
            none[i] = False
    return out, none


def _run_list(kps, vis_thresh, kernel_size, sigma):
    """one track given as the reference's list -> (params fp64 (L, 3), start, end) as numpy / ints"""
    _check_filter(kernel_size, sigma)
    arr, none = _pack_kps(kps)
    if arr.shape[2] > MAX_KEYPOINTS:
        raise ValueError(f"{arr.shape[2]} keypoints per frame: at most {MAX_KEYPOINTS}")
    if none.any():
        # a missing frame must be invalid whatever the threshold is: its confidences lie below it
        arr[0, none, :, 2] = -np.inf
    dev = _device()
    t = torch.from_numpy(arr).to(dev)
    lengths = torch.tensor([len(kps)], dtype=torch.int32, device=dev)
    _, span, params = _launch_tracks(t, None, lengths, vis_thresh, kernel_size, sigma, 1.0, True)
    span = span.cpu().numpy()
    return params[0].cpu().numpy(), int(span[0, 0]), int(span[0, 1])


def kp_to_bbox_param(kp, vis_thresh):
    """smooth_bbox.py:38-61: [center_x, center_y, scale] of one frame's (J, 3) keypoints, or None if there is no box"""
    if kp is None:
        return None
    params, start, end = _run_list([kp], vis_thresh, 1, _IDENTITY_SIGMA)
    return None if start < 0 else params[0].copy()


def get_all_bbox_params(kps, vis_thresh=2):
    """smooth_bbox.py:64-105: (bbox_params (end - start, 3) with the frames in between filled linearly, start index (inclusive), end index (exclusive)); a list
    without any valid frame gives (empty, -1, 0)"""
    if len(kps) == 0:
        return np.empty((0, 3), dtype=np.float64), -1, 0
    params, start, end = _run_list(kps, vis_thresh, 1, _IDENTITY_SIGMA)          # window 1 and radius 0: both filters return their input
    if start < 0:
        return np.empty((0, 3), dtype=np.float64), -1, 0
    return params[start:end].copy(), start, end


def smooth_bbox_params(bbox_params, kernel_size=11, sigma=8):
    """smooth_bbox.py:108-123: median filter, then Gaussian filter, of (N, 3) parameters"""
    _check_filter(kernel_size, sigma)
    x = np.ascontiguousarray(np.asarray(bbox_params, dtype=np.float64).reshape(-1, 3))
    if len(x) == 0:
        raise ValueError("smooth_bbox_params: empty series")
    dev = _device()
    series = torch.from_numpy(x[None]).to(dev)
    lengths = torch.tensor([len(x)], dtype=torch.int32, device=dev)
    _, _, params = _launch_tracks(None, series, lengths, 0.0, kernel_size, sigma, 1.0, True)
    return params[0].cpu().numpy()


def get_smooth_bbox_params(kps, vis_thresh=2, kernel_size=11, sigma=3):
    """smooth_bbox.py:11-35: (smoothed [cx, cy, scale] of frames 0 .. end-1 with zero rows before start, start, end).  ValueError if no frame has a box (the reference
    fails inside scipy there)."""
    if len(kps) == 0:
        raise ValueError("get_smooth_bbox_params: no frames")
    params, start, end = _run_list(kps, vis_thresh, kernel_size, sigma)
    if start < 0:
        raise ValueError("get_smooth_bbox_params: no frame has a visible bounding box")
    return params[:end].copy(), start, end


# ---- host logic of the driver: windows, padding, chunks (pure numpy) ----------------------------------------------------------------------------------
def window_positions(n, seqlen):
    """positions 0 .. n-1 cut into consecutive windows of seqlen, the tail padded as lib/data_utils/img_utils.py:32-54 pads with pad=True
    (np.pad(indices, (0, padlen), 'reflect'): the edge sample is NOT repeated, a single index repeats).  Returns (positions (n_windows, seqlen), real (n_windows,
    seqlen) bool: False for the padded slots, which always trail)."""
    if n < 1 or seqlen < 1:
        raise ValueError(f"window_positions: n={n} seqlen={seqlen}")
    nw = -(-n // seqlen)
    i = np.arange(nw * seqlen, dtype=np.int64)
    if n == 1:
        pos = np.zeros_like(i)
    else:
        t = i % (2 * (n - 1))
        pos = np.where(t >= n, 2 * (n - 1) - t, t)
    return pos.reshape(nw, seqlen), (i < n).reshape(nw, seqlen)


def plan_chunks(people, seqlen, frame_bytes, clips_per_batch, max_src_bytes=MAX_SRC_BYTES, max_crops=MAX_CROPS):
    """people: list of (frame_ids (m) int array, box_base int): the frames a kept person is cropped from and the row of its first box in the box table.
    Every person's frames are cut into windows (window_positions); the windows, ordered by their first frame, are gathered into chunks = one call each of
    maed_crop_tables, maed_clip_preprocess and the model, such that per chunk
        windows <= clips_per_batch,   crops <= max_crops,   (last frame - first frame + 1) * frame_bytes < max_src_bytes
    (the source pointer of a chunk is its first frame, so every table offset stays below max_src_bytes).  Returns a list of dicts: first_frame, n_frames,
    frame_index (M) int32 relative to first_frame, box_index (M) int32, windows = [(person index, window index, real slots)]."""
    wins = []
    for pi, (frame_ids, base) in enumerate(people):
        frame_ids = np.asarray(frame_ids, dtype=np.int64)
        pos, real = window_positions(len(frame_ids), seqlen)
        for w in range(len(pos)):
            f = frame_ids[pos[w]]
            wins.append((int(f.min()), int(f.max()), pi, w, f, base + pos[w], int(real[w].sum())))
    if seqlen > max_crops:
        raise ValueError(f"plan_chunks: seqlen {seqlen} exceeds the {max_crops} crops of one preprocessing call")
    wins.sort(key=lambda x: (x[0], x[2], x[3]))
    chunks, cur = [], []

    def close():
        if not cur:
            return
        lo, hi = min(x[0] for x in cur), max(x[1] for x in cur)
        chunks.append(dict(first_frame=lo, n_frames=hi - lo + 1, frame_index=(np.concatenate([x[4] for x in cur]) - lo).astype(np.int32),
                           box_index=np.concatenate([x[5] for x in cur]).astype(np.int32), windows=[(x[2], x[3], x[6]) for x in cur]))
        cur.clear()

    for x in wins:
        if (x[1] - x[0] + 1) * frame_bytes >= max_src_bytes:
            raise ValueError(f"plan_chunks: one window spans frames {x[0]} .. {x[1]} = {(x[1] - x[0] + 1) * frame_bytes} bytes of {frame_bytes}-byte frames: the "
                             f"clip preprocessing addresses less than 2^31 = {max_src_bytes} bytes per call")
        if cur:
            lo, hi = min(cur[0][0], x[0]), max(max(y[1] for y in cur), x[1])
            if len(cur) >= clips_per_batch or (len(cur) + 1) * seqlen > max_crops or (hi - lo + 1) * frame_bytes >= max_src_bytes:
                close()
        cur.append(x)
    close()
    return chunks


class VideoInference:
    """Thin driver from (device frames, person tracks) to the per-person results render.prepare_rendering_results takes.

    model: a MAED (any module with its forward contract: (N, T, 3, H, W) fp32 -> {'theta', 'verts', 'kp_2d', 'kp_3d'}); it runs in eval mode under no_grad,
    clips_per_batch windows of seqlen crops at a time.  patch: the side of the square crop.  vis_thresh / kernel_size / sigma / box_scale: track_boxes.
    min_frames: keypoint tracks whose span is shorter are skipped; default (kernel_size + 1) // 2, below which the median filter makes every scale 0."""

    def __init__(self, model, seqlen=16, clips_per_batch=8, patch=224, vis_thresh=0.3, kernel_size=11, sigma=8, box_scale=1.1, min_frames=None,
                 mean=data.IMAGENET_MEAN, std=data.IMAGENET_STD):
        _check_filter(kernel_size, sigma)
        if patch % 4:
            raise ValueError(f"VideoInference: patch width {patch} is not a multiple of 4")
        if seqlen < 1 or clips_per_batch < 1 or seqlen > MAX_CROPS:
            raise ValueError(f"VideoInference: seqlen={seqlen} clips_per_batch={clips_per_batch} (at most {MAX_CROPS} crops per preprocessing call)")
        self.model, self.seqlen, self.clips_per_batch, self.patch = model, int(seqlen), int(clips_per_batch), int(patch)
        self.vis_thresh, self.kernel_size, self.sigma, self.box_scale = vis_thresh, int(kernel_size), sigma, box_scale
        self.min_frames = (self.kernel_size + 1) // 2 if min_frames is None else int(min_frames)
        self.mean, self.std = tuple(mean), tuple(std)

    # -- boxes of every track on the device + ONE host read (spans and a finiteness flag) --
    def _boxes(self, tracks, B, dev):
        """-> box table fp32 (n_boxes, 4) on the device, {person: (frame ids (m) numpy, row of its first box)} for the kept tracks, {person: reason} for the rest"""
        names, frame_ids, tables, bases, info = [], [], [], [], []
        n_rows = 0
        by_J = {}
        for person, rec in tracks.items():
            f = np.asarray(rec["frames"].cpu() if isinstance(rec["frames"], torch.Tensor) else rec["frames"]).astype(np.int64).reshape(-1)
            if len(f) == 0 or f.min() < 0 or f.max() >= B:
                raise ValueError(f"VideoInference: person {person!r}: frame indices must be non-empty and lie in 0 .. {B - 1}")
            if rec.get("joints2d") is not None:
                kp = torch.as_tensor(rec["joints2d"]).to(device=dev, dtype=torch.float32)
                if kp.dim() != 3 or kp.shape[0] != len(f) or kp.shape[2] != 3:
                    raise ValueError(f"VideoInference: person {person!r}: joints2d must be (n, J, 3) with n = {len(f)} frames, got {tuple(kp.shape)}")
                if kp.shape[1] > MAX_KEYPOINTS:
                    raise ValueError(f"VideoInference: person {person!r}: {kp.shape[1]} keypoints per frame: at most {MAX_KEYPOINTS}")
                by_J.setdefault(int(kp.shape[1]), []).append((person, f, kp))
            elif rec.get("bbox") is not None:
                bb = torch.as_tensor(rec["bbox"]).to(device=dev, dtype=torch.float32)
                if tuple(bb.shape) != (len(f), 4):
                    raise ValueError(f"VideoInference: person {person!r}: bbox must be (n, 4) with n = {len(f)} frames, got {tuple(bb.shape)}")
                ok = (torch.isfinite(bb).all() & (bb[:, 2:] > 0).all()).to(torch.int32)
                names.append((person, False)); frame_ids.append(f); tables.append(bb); bases.append(n_rows)
                info.append(torch.stack([torch.zeros_like(ok), torch.full_like(ok, len(f)), ok])[None])
                n_rows += len(f)
            else:
                raise ValueError(f"VideoInference: person {person!r} has neither 'joints2d' nor 'bbox'")
        for J, group in by_J.items():
            Lmax = max(len(f) for _, f, _ in group)
            kps = torch.zeros((len(group), Lmax, J, 3), dtype=torch.float32, device=dev)
            for k, (_, f, kp) in enumerate(group):
                kps[k, :len(f)] = kp
            lengths = torch.tensor([len(f) for _, f, _ in group], dtype=torch.int32, device=dev)
            boxes, span = track_boxes(kps, lengths, self.vis_thresh, self.kernel_size, self.sigma, self.box_scale)
            ok = torch.isfinite(boxes).all(dim=2).all(dim=1).to(torch.int32)          # (rows outside the span are zero)
            info.append(torch.cat([span, ok[:, None]], dim=1))
            for k, (person, f, _) in enumerate(group):
                names.append((person, True)); frame_ids.append(f); bases.append(n_rows + k * Lmax)
            tables.append(boxes.reshape(-1, 4))
            n_rows += len(group) * Lmax
        if not names:
            return None, {}, {}
        host = torch.cat(info, dim=0).cpu().numpy()               # the one host read before the model runs
        kept, skipped = {}, {}
        for (person, from_kps), f, base, (start, end, ok) in zip(names, frame_ids, bases, host):
            if start < 0:
                skipped[person] = "no frame has a visible bounding box"
            elif from_kps and end - start < self.min_frames:
                skipped[person] = f"span of {end - start} frames is shorter than min_frames={self.min_frames}"
            elif not ok:
                skipped[person] = "non-finite or non-positive bounding box"
            else:
                kept[person] = (f[start:end], base + int(start))
        return torch.cat(tables, dim=0), kept, skipped

    @torch.no_grad()
    def run(self, frames, tracks, debug=False):
        """frames: uint8 (B, h, w, 3) RGB on the device.  tracks: {person: {'frames': (n) ints, 'joints2d': (n, J, 3) or 'bbox': (n, 4) = cx, cy, w, h}} (numpy or
        tensors; joints2d goes through track_boxes, bbox is used as given).  Returns (results, skipped): results[person] = {'frame_ids' (numpy int64: the host knows
        them), and on the device 'bboxes' (m, 4), 'pred_cam' (m, 3), 'orig_cam' (m, 4), 'verts', 'pose' (m, 72), 'betas' (m, 10), 'joints3d', 'joints2d'};
        skipped[person] = the reason.  debug=True adds a third value: {'chunks': the plan, 'clips': the crop tensor of every chunk}."""
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError("VideoInference.run: frames must be a uint8 (B, h, w, 3) tensor")
        ops._p(frames)                                          # (a CPU tensor is an error, not a fallback)
        frames = frames.contiguous()
        B, h, w = (int(v) for v in frames.shape[:3])
        dev, T, P = frames.device, self.seqlen, self.patch
        frame_bytes = h * w * 3
        table, kept, skipped = self._boxes(tracks, B, dev)
        results, dbg = {}, dict(chunks=[], clips=[])
        if not kept:
            return (results, skipped, dbg) if debug else (results, skipped)
        persons = list(kept)
        chunks = plan_chunks([kept[p] for p in persons], T, frame_bytes, self.clips_per_batch)
        index = torch.from_numpy(np.concatenate([np.stack([c["box_index"], c["frame_index"]]) for c in chunks], axis=1)).to(dev)      # int32 (2, all crops)
        flat = frames.view(-1)
        lib = L.lib()
        outs = {p: {} for p in persons}
        was_training = self.model.training
        self.model.eval()
        try:
            at = 0
            for c in chunks:
                M = len(c["box_index"])
                N = M // T
                o_fi, o_fm, o_ci, o_cf, total = data.table_offsets(N, T)
                tables = torch.empty(total, dtype=torch.uint8, device=dev)
                bi, fi = index[0, at:at + M], index[1, at:at + M]
                at += M
                tp = ops._p(tables)
                L.check(lib.maed_crop_tables(ops._p(table), int(table.shape[0]), ops._p(bi), ops._p(fi), M, T, c["n_frames"], h, w, P, P, tp + o_fi, tp + o_fm,
                                             tp + o_ci, tp + o_cf, ops._stream()), "crop_tables")
                clips = torch.empty((N, T, 3, P, P), dtype=torch.float32, device=dev)
                # ops.clip_preprocess addresses everything relative to one buffer: that buffer is the frame tensor, the pixel offset is the chunk's first frame,
                # and the tables (their own allocation) lie at the difference of the two addresses
                rel = tp - ops._p(flat)
                ops.clip_preprocess(flat, (rel + o_fi, rel + o_fm, rel + o_ci, rel + o_cf, c["first_frame"] * frame_bytes), c["n_frames"] * frame_bytes, M, N, P, P,
                                    self.mean, self.std, False, clips)
                out = self.model(clips)
                for n, (pi, wi, real) in enumerate(c["windows"]):
                    outs[persons[pi]][wi] = {k: out[k][n, :real] for k in ("theta", "verts", "kp_3d", "kp_2d")}       # the padded slots trail: dropped here
                if debug:
                    dbg["chunks"].append(c)
                    dbg["clips"].append(clips)
        finally:
            self.model.train(was_training)
        for p in persons:
            f, base = kept[p]
            got = {k: torch.cat([outs[p][wi][k] for wi in sorted(outs[p])], dim=0) for k in ("theta", "verts", "kp_3d", "kp_2d")}
            theta = got["theta"].float()
            bboxes = table[base:base + len(f)]
            pred_cam = theta[:, :3]
            results[p] = dict(frame_ids=f.copy(), bboxes=bboxes, pred_cam=pred_cam, orig_cam=convert_crop_cam_to_orig_img(pred_cam, bboxes, w, h),
                              verts=got["verts"], pose=theta[:, 3:75], betas=theta[:, 75:], joints3d=got["kp_3d"], joints2d=got["kp_2d"])
        return (results, skipped, dbg) if debug else (results, skipped)
