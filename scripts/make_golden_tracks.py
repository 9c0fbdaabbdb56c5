"""Writes tests/golden/g19_tracks.npz: seeded keypoint tracks and what the reference's lib/utils/smooth_bbox.py returns for them (inputs and recorded results only).

    python scripts/make_golden_tracks.py <root of the reference checkout>

The reference module is loaded by path and needs numpy and scipy only.  Keypoints are fp32-representable values handed to the reference as float64, so that it
computes in fp64 throughout (with float32 input it mixes precisions); they are stored as float32.  A frame the tracker has no keypoints for (None in the reference's
list) is stored as a row of zeros with its flag set in `none`.  Tracks without any valid frame are not in the file: the reference raises on them.

Per case i: c{i}_kps (L, J, 3) f32, c{i}_none (L) bool, c{i}_cfg = (vis_thresh, kernel_size, sigma) f64, c{i}_raw (m, 3) = get_all_bbox_params, c{i}_span = (start, end),
c{i}_params (end, 3) = get_smooth_bbox_params (rows before start are zero, as the reference returns them); `names` lists what each case is there for."""
import importlib.util
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIS = 0.1
NONE, INVISIBLE, SMALL = 1, 2, 3          # why a frame is invalid: no keypoints at all, none above the threshold, a rectangle below half a pixel


def make_track(rng, kinds, J):
    """kinds (L): 0 = a valid frame, else one of the three reasons above"""
    L = len(kinds)
    kps = np.zeros((L, J, 3), dtype=np.float32)
    centre = rng.uniform(200, 800, 2)
    for i, kind in enumerate(kinds):
        centre = centre + rng.normal(0, 6, 2)
        size = rng.uniform(60, 320)
        if kind == NONE:
            continue
        xy = centre + rng.uniform(-0.5, 0.5, (J, 2)) * (0.2 if kind == SMALL else size)
        conf = rng.uniform(0.3, 1.0, J)
        if kind == INVISIBLE:
            conf = rng.uniform(0.0, 0.09, J)
        elif J > 2:
            far = rng.random(J) < 0.2                       # keypoints below the threshold, far away: they must not move the rectangle
            far[:2] = False
            xy[far] += rng.uniform(-900, 900, (int(far.sum()), 2))
            conf[far] = rng.uniform(0.0, 0.09, int(far.sum()))
        if kind == 0 and J >= 2:
            xy[1] = xy[0] + rng.uniform(20, size, 2)        # two visible keypoints a clear distance apart, whatever J is
        kps[i, :, :2] = xy
        kps[i, :, 2] = conf
    return kps


def cases():
    rng = np.random.default_rng(19)
    out = []

    def add(name, kinds, J=25, k=11, sigma=3.0):
        kinds = np.asarray(kinds, dtype=np.int64)
        out.append((name, make_track(rng, kinds, J), kinds == NONE, (VIS, k, sigma)))

    # span lengths around (k + 1) / 2 for k = 11, around r and 2 r + 1 for sigma = 3, and one that the reflect map wraps several times for sigma = 8
    for m in (1, 5, 6, 7, 12, 13, 24, 25, 26, 97):
        kinds = [NONE, INVISIBLE] + [0] * m + [SMALL, NONE, INVISIBLE]          # gaps in front of and behind the span
        if m >= 12:
            kinds[5] = INVISIBLE                                               # a gap of one frame
            kinds[8:10] = [NONE, SMALL]
        add(f"span{m}_s3", kinds)
    for m in (7, 26, 97):
        add(f"span{m}_s8", [0] * m, sigma=8.0)
        add(f"span{m}_s05", [0] * m, sigma=0.5)
    add("all_but_ends", [0] + [NONE] * 30 + [0])
    add("all_but_ends_mixed", [0] + [NONE, INVISIBLE, SMALL] * 9 + [0], sigma=8.0)
    for k in (1, 3, 11, 31, 63):
        kinds = rng.choice([0, 0, 0, NONE, INVISIBLE, SMALL], 40)
        kinds[3] = kinds[36] = 0
        add(f"k{k}", kinds, k=k)
    for J in (2, 25, 49, 64):
        kinds = rng.choice([0, 0, NONE, INVISIBLE, SMALL], 33)
        kinds[1] = kinds[30] = 0
        add(f"J{J}", kinds, J=J)
    # one span on each side of the 1024-frame boundary between the two forms of the kernel (J = 2 keeps the file small)
    for m in (1024, 1025):
        kinds = rng.choice([0, 0, 0, 0, NONE, INVISIBLE], m)
        kinds[0] = kinds[-1] = 0
        add(f"len{m}", kinds, J=2, sigma=8.0)
    return out


def main():
    ref_root = sys.argv[1]
    spec = importlib.util.spec_from_file_location("ref_smooth_bbox", os.path.join(ref_root, "lib", "utils", "smooth_bbox.py"))
    ref = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec.loader.exec_module(ref)
    data, names = {}, []
    for i, (name, kps, none, cfg) in enumerate(cases()):
        vis, k, sigma = cfg
        lst = [None if none[t] else kps[t].astype(np.float64) for t in range(len(kps))]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            raw, start, end = ref.get_all_bbox_params(lst, vis)
            params, s2, e2 = ref.get_smooth_bbox_params(lst, vis, k, sigma)
        assert (start, end) == (s2, e2) and params.shape == (end, 3) and raw.shape == (end - start, 3)
        names.append(name)
        data[f"c{i}_kps"] = kps
        data[f"c{i}_none"] = none
        data[f"c{i}_cfg"] = np.array([vis, k, sigma], dtype=np.float64)
        data[f"c{i}_raw"] = raw.astype(np.float64)
        data[f"c{i}_span"] = np.array([start, end], dtype=np.int64)
        data[f"c{i}_params"] = params.astype(np.float64)
    data["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "g19_tracks.npz")
    np.savez_compressed(path, **data)
    print(f"{path}: {len(names)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
