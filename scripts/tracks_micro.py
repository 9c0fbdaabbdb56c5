"""Video inference (csrc/tracks.hip, maed_amd/video.py) in isolation, event-timed.  Recorded, not gated:
  1. maed_track_boxes for 64 tracks x 2000 frames x 25 keypoints (k = 11, sigma = 8; 2000 > 1024 frames: the series live in the workspace) and for 64 x 1000
     (the series live in LDS);
  2. 128 crops of 224 x 224 from sixteen 1080p frames: maed_crop_tables + maed_clip_preprocess on the resident frames, against the host-packed path for the same
     crops (data.pack_clips on one core + data.preprocess_clips: upload and kernel, host clock to a synchronise);
  3. the whole VideoInference.run for two people over 64 frames of 270 x 480 on MAED(num_blocks=2, num_heads=2, embed_dim=128, hidden_dim=64, img_size=64, bf16).
Each kernel row is the minimum / median of REPEATS windows of `iters` calls.
usage: tracks_micro.py [--out FILE] [--iters N]      (writes FILE, default profiles/tracks_micro.txt, and prints it)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maed_amd import MAED, data as D, ops, video as V          # noqa: E402
from maed_amd import _lib as L                                  # noqa: E402

REPEATS = 3
LINES = []


def say(line):
    LINES.append(line)
    print(line, flush=True)


def windows(call, iters):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / iters)
    return min(us), float(np.median(us))


def tracks(K, Lf, J, iters):
    rng = np.random.default_rng(0)
    kps = rng.uniform(0, 1000, (K, Lf, J, 3)).astype(np.float32)
    kps[..., 2] = rng.uniform(0, 1, (K, Lf, J))
    kps[:, ::7, :, 2] = 0.0                                      # every seventh frame has no box
    kps_d = torch.from_numpy(kps).cuda()
    len_d = torch.full((K,), Lf, dtype=torch.int32, device="cuda")
    lo, med = windows(lambda: V.track_boxes(kps_d, len_d, 0.3, 11, 8), iters)
    say(f"track_boxes   {K} tracks x {Lf} frames x {J} keypoints, k=11 sigma=8 ({'workspace' if Lf > V.LDS_FRAMES else 'LDS'} form, allocation of the outputs included)"
        f"   {lo:9.1f} / {med:9.1f} us")


def crops(iters):
    B, h, w, P, T, M = 16, 1080, 1920, 224, 16, 128
    rng = np.random.default_rng(1)
    frames = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    boxes = np.stack([rng.uniform(300, 1600, M), rng.uniform(200, 900, M), rng.uniform(150, 700, M)], 1).astype(np.float32)
    boxes = np.concatenate([boxes, boxes[:, 2:]], 1)
    fidx = (np.arange(M) % B).astype(np.int32)
    fr_d = torch.from_numpy(frames).cuda()
    flat = fr_d.view(-1)
    bx_d, bi_d, fi_d = torch.from_numpy(boxes).cuda(), torch.arange(M, dtype=torch.int32, device="cuda"), torch.from_numpy(fidx).cuda()
    N = M // T
    o = D.table_offsets(N, T)
    tables = torch.empty(o[4], dtype=torch.uint8, device="cuda")
    out = torch.empty((N, T, 3, P, P), device="cuda")
    lib, tp = L.lib(), tables.data_ptr()
    rel = tp - flat.data_ptr()

    def device_path():
        L.check(lib.maed_crop_tables(bx_d.data_ptr(), M, bi_d.data_ptr(), fi_d.data_ptr(), M, T, B, h, w, P, P, tp + o[0], tp + o[1], tp + o[2], tp + o[3], ops._stream()),
                "crop_tables")
        ops.clip_preprocess(flat, (rel + o[0], rel + o[1], rel + o[2], rel + o[3], 0), flat.numel(), M, N, P, P, D.IMAGENET_MEAN, D.IMAGENET_STD, False, out)

    lo, med = windows(device_path, iters)
    say(f"crops         {M} x {P}^2 from {B} resident frames of {h} x {w}: crop_tables + clip_preprocess   {lo:9.1f} / {med:9.1f} us")
    dev_out = out.clone()
    clips = [[frames[fidx[n * T + t]] for t in range(T)] for n in range(N)]
    recs = [D.ClipParams(bboxes=boxes[n * T:(n + 1) * T].astype(np.float64), scale=(1.0, 1.0)) for n in range(N)]
    aug = D.ClipAugment.eval(P, P)
    t0 = time.perf_counter()
    packed = D.pack_clips(clips, recs, aug)
    t_pack = time.perf_counter() - t0
    pinned = packed.pin_memory()
    host_ms = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = D.preprocess_clips(pinned)
        torch.cuda.synchronize()
        host_ms.append(1e3 * (time.perf_counter() - t0))
    lv = (ref.reshape(dev_out.shape) - dev_out).abs().max().item() * 255 * 0.229
    say(f"crops         the same crops host-packed: pack_clips {1e3 * t_pack:.1f} ms on one core ({packed.src_bytes / 1e6:.1f} MB of regions) + upload from pinned memory and "
        f"kernel, host clock to synchronise {min(host_ms):.2f} / {float(np.median(host_ms)):.2f} ms; largest difference between the two paths {lv:.2f} levels")


def driver():
    torch.manual_seed(0)
    model = MAED(num_blocks=2, num_heads=2, embed_dim=128, hidden_dim=64, img_size=64, compute_dtype=torch.bfloat16).cuda()
    B, h, w, J = 64, 270, 480, 25
    rng = np.random.default_rng(2)
    frames = torch.from_numpy(rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)).cuda()
    kp = np.zeros((B, J, 3), dtype=np.float32)
    kp[..., 0] = 240 + rng.uniform(-40, 40, (B, J))
    kp[..., 1] = 135 + rng.uniform(-80, 80, (B, J))
    kp[..., 2] = 0.9
    bbox = np.tile(np.float32([300, 140, 120, 120]), (B, 1))
    tracks_in = {0: dict(frames=np.arange(B), joints2d=kp), 1: dict(frames=np.arange(B), bbox=bbox)}
    vi = V.VideoInference(model, seqlen=16, clips_per_batch=8, patch=64)
    ms = []
    for i in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        results, skipped = vi.run(frames, tracks_in)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    assert not skipped and results[0]["verts"].shape[0] == B
    say(f"driver        VideoInference.run, 2 people x {B} frames of {h} x {w}, 8 windows of 16 crops of 64^2 in one model call, small MAED (bf16): first call "
        f"{ms[0]:.1f} ms, then {min(ms[1:]):.2f} / {float(np.median(ms[1:])):.2f} ms (host clock to synchronise)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_micro.txt"))
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tracks_micro needs a GPU"
    say(f"scripts/tracks_micro.py on {torch.cuda.get_device_name(0)}: {a.iters} calls per window, {REPEATS} windows per row, min / median; recorded, not gated")
    tracks(64, 2000, 25, a.iters)
    tracks(64, 1000, 25, a.iters)
    crops(a.iters)
    driver()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
