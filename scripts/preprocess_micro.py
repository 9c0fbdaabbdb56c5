"""Clip preprocessing (csrc/preprocess.hip) in isolation, event-timed: 128 frames at 224 x 224 for the evaluation path and the stage-2 training config
(flip 0.5, crop 0.2 / 0.6, jitter 0.3, erase 0.3 / 0.7) in every launch form that applies, 128 frames at 256 x 256, and the host time of pack_clips per clip.
Bytes = the fp32 write + the packed region reads (+ the uint8 scratch written and read once in the two-launch form); share of HBM peak = those bytes at 8 TB/s
over the measured time (the kernel is bound by bytes, not operations).  The kernel time excludes the upload: the packed buffer is made resident first.
Each row is timed over `iters` calls (default 5000: a window of 0.25-1 s) that rotate over SETS copies of the packed buffer and of the output, so that the
working set (SETS x 115-200 MB) does not fit the 256 MB Infinity Cache and the traffic has to reach HBM; the window is repeated REPEATS times and the minimum
and the median are printed.  The scene generator is the tests' (tests/_preprocess_ref.py): this script needs the test tree next to it.
usage: preprocess_micro.py [iters]      (one process; run it under a time limit)"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _preprocess_ref as R          # the seeded scene generator of the tests
from maed_amd import data as D, ops

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5000
SETS, REPEATS = 4, 3
HBM_PEAK = 8.0e12
FORMS = {ops.PRE_FORM_DIRECT: "direct", ops.PRE_FORM_LDS: "lds", ops.PRE_FORM_TWO: "two-launch"}


def scene(n, T, size, aug, seed):
    frames, records = R.random_scene(seed, n, T, size, size, lo=100, hi=900, jitter=False)
    return frames, [aug.sample(r.bboxes) for r in records]


def timed(packed, form):
    F = packed.N * packed.T
    blobs = [packed.blob.cuda() for _ in range(SETS)]
    outs = [torch.empty(packed.N, packed.T, 3, packed.H, packed.W, device="cuda") for _ in range(SETS)]
    call = lambda i: ops.clip_preprocess(blobs[i % SETS], packed.offsets, packed.src_bytes, F, packed.N, packed.H, packed.W, packed.mean, packed.std,
                                         packed.has_contrast, outs[i % SETS], form)
    for i in range(2 * SETS):
        call(i)
    torch.cuda.synchronize()
    us = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            call(i)
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / iters)
    nbytes = outs[0].numel() * 4 + packed.src_bytes + (2 * F * 3 * packed.H * packed.W if form == ops.PRE_FORM_TWO else 0)
    return min(us), float(np.median(us)), nbytes, outs[0]


def main():
    assert torch.cuda.is_available(), "preprocess_micro needs a GPU"
    print(f"device {torch.cuda.get_device_name(0)}; {iters} calls per window over {SETS} buffer sets, {REPEATS} windows per row (min / median)", flush=True)
    for name, size, kw, forms in (
            ("eval", 224, dict(flip_p=0.0), (ops.PRE_FORM_DIRECT, ops.PRE_FORM_LDS, ops.PRE_FORM_TWO)),
            ("stage2", 224, dict(flip_p=0.5, random_crop_p=0.2, random_crop_size=0.6, color_jitter=0.3, erase_prob=0.3, erase_part=0.7), (ops.PRE_FORM_LDS, ops.PRE_FORM_TWO)),
            ("eval", 256, dict(flip_p=0.0), (ops.PRE_FORM_DIRECT, ops.PRE_FORM_TWO)),
            ("stage2", 256, dict(flip_p=0.5, random_crop_p=0.2, random_crop_size=0.6, color_jitter=0.3, erase_prob=0.3, erase_part=0.7), (ops.PRE_FORM_TWO,))):
        aug = D.ClipAugment(size, size, seed=1, **kw)
        frames, records = scene(8, 16, size, aug, 7)
        t0 = time.perf_counter()
        reps = 5
        for _ in range(reps):
            packed = D.pack_clips(frames, records, aug)
        host_ms = 1e3 * (time.perf_counter() - t0) / reps / len(frames)
        ref = None
        for form in forms:
            us, med, nbytes, out = timed(packed, form)
            same = "" if ref is None else f"  bit-equal to {FORMS[forms[0]]}: {bool(torch.equal(out, ref))}"
            ref = out if ref is None else ref
            print(f"preprocess {name:6s} 128 x {size}^2 {FORMS[form]:10s} {us:8.1f} / {med:6.1f} us  {nbytes / 1e6:7.1f} MB  {nbytes / us / 1e6:6.2f} TB/s = {nbytes / (us * 1e-6) / HBM_PEAK:.3f} of HBM peak{same}", flush=True)
        for label, pk in (("pinned", packed.pin_memory()), ("pageable", packed)):
            for _ in range(3):
                D.preprocess_clips(pk)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(50):
                o = D.preprocess_clips(pk)
            torch.cuda.synchronize()
            e2e = 1e3 * (time.perf_counter() - t0) / 50
            print(f"preprocess {name:6s} 128 x {size}^2 upload from {label} memory + kernels, host clock to synchronise: {e2e:.2f} ms per step ({packed.src_bytes / 1e6:.1f} MB uploaded)", flush=True)
            del o
        print(f"preprocess {name:6s} 128 x {size}^2 pack_clips {host_ms:.2f} ms per clip of 16 frames on one core", flush=True)


if __name__ == "__main__":
    main()
