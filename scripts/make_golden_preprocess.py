"""Writes tests/golden/g16_clip_preprocess.npz: inputs and the REFERENCE's outputs for every stage of its transform chain after the warp
(lib/data_utils/transforms/{crop,color_jitter,random_erase,random_hflip,basic}.py, lib/data_utils/kp_utils.py), which the tests of
maed_amd/data.py and csrc/preprocess.hip compare against.  CPU only:

    python scripts/make_golden_preprocess.py --reference /path/to/maed

The reference's modules are imported from its own files.  Three stand-ins take the place of packages that need not be installed:
  cv2.getAffineTransform                     an fp64 three-point solve (cv2.warpAffine is never called here: the warp's oracle is the fp64
                                             restatement in tests/_preprocess_ref.py)
  torchvision.transforms.functional          hflip / adjust_* / to_tensor / normalize as the PIL and tensor calls torchvision makes
Arrays only; nothing of the reference's text is stored.
"""
import argparse
import importlib.util
import itertools
import os
import random
import sys
import types

import numpy as np
import torch
from PIL import Image, ImageEnhance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def install_stubs():
    cv2 = types.ModuleType("cv2")

    def get_affine_transform(src, dst):
        A = np.concatenate([np.asarray(src, dtype=np.float64), np.ones((3, 1))], axis=1)
        return np.linalg.solve(A, np.asarray(dst, dtype=np.float64)).T

    cv2.getAffineTransform = get_affine_transform
    cv2.INTER_LINEAR, cv2.BORDER_CONSTANT = 1, 0
    sys.modules["cv2"] = cv2

    tv, tvt, tvf = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms"), types.ModuleType("torchvision.transforms.functional")
    tvf.hflip = lambda im: im.transpose(Image.FLIP_LEFT_RIGHT)
    tvf.adjust_brightness = lambda im, f: ImageEnhance.Brightness(im).enhance(f)
    tvf.adjust_saturation = lambda im, f: ImageEnhance.Color(im).enhance(f)
    tvf.adjust_contrast = lambda im, f: ImageEnhance.Contrast(im).enhance(f)

    def adjust_hue(im, hue):
        h, s, v = im.convert("HSV").split()
        np_h = np.array(h, dtype=np.uint8)
        np_h = (np_h.astype(np.int32) + (int(hue * 255) & 255)).astype(np.uint8)       # uint8 addition with wrap-around
        return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")

    tvf.adjust_hue = adjust_hue
    tvf.to_tensor = lambda pic: torch.from_numpy(np.ascontiguousarray(np.asarray(pic).transpose(2, 0, 1))).to(torch.float32).div(255)

    def normalize(t, mean, std, inplace=False):
        t = t if inplace else t.clone()
        mean = torch.as_tensor(mean, dtype=t.dtype)
        std = torch.as_tensor(std, dtype=t.dtype)
        return t.sub_(mean.view(-1, 1, 1)).div_(std.view(-1, 1, 1))

    tvf.normalize = normalize
    tv.transforms, tvt.functional = tvt, tvf
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf})


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def make_patches(rng):
    """two frame sizes; smooth colour gradients plus a noise patch (the hue rounding differs from PIL only on rare pixels: gradients keep the share low,
    noise covers the whole cube)"""
    def gradient(h, w, phase):
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        r = 127.5 + 127.5 * np.sin(x / w * 3.1 + phase)
        g = 127.5 + 127.5 * np.sin(y / h * 2.3 + 2 * phase + 1.0)
        b = 127.5 + 127.5 * np.sin((x + y) / (w + h) * 4.0 + 3 * phase + 2.0)
        return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)

    a = np.stack([gradient(64, 48, 0.3), gradient(64, 48, 1.7)])
    b = np.stack([rng.integers(0, 256, (56, 56, 3), dtype=np.uint8), gradient(56, 56, 0.9)])
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g16_clip_preprocess.npz"))
    args = ap.parse_args()
    install_stubs()
    ref = args.reference
    sys.path.insert(0, ref)
    kp = load("lib.data_utils.kp_utils", os.path.join(ref, "lib", "data_utils", "kp_utils.py"))
    T = os.path.join(ref, "lib", "data_utils", "transforms")
    crop, jit, er, fl, basic = (load("ref_" + n, os.path.join(T, n + ".py")) for n in ("crop", "color_jitter", "random_erase", "random_hflip", "basic"))
    rng = np.random.default_rng(16)
    out = {}

    # ---- crop matrices and affine keypoints ------------------------------------------------------------------------------------
    cases = [(224, 224, [300., 200., 180., 180.], 1.3, 0., (0., 0.)), (224, 224, [310.5, 190.25, 150., 210.], 1.1, 25., (0.05, -0.02)),
             (256, 256, [80., 400., 90., 60.], 1.45, -40., (0., 0.)), (64, 48, [20., 30., 40., 50.], 0.9, 170., (-0.1, 0.08)),
             (224, 224, [1000.3, 17.9, 33.3, 471.1], 1.3, -3.5, (0.2, 0.2))]
    out["trans_cases"] = np.array([[h, w, *b, s, r, *sh] for h, w, b, s, r, sh in cases], dtype=np.float64)
    kp_in = np.concatenate([rng.uniform(-50, 700, (len(cases), 49, 2)), rng.integers(0, 2, (len(cases), 49, 1)).astype(np.float64)], -1)
    out["trans_kp_in"] = kp_in
    mats, kps = [], []
    for (h, w, b, s, r, sh), k in zip(cases, kp_in):
        c = crop.CropVideo(h, w)
        m = c.gen_trans(np.array(b), (s, s), r, sh)
        mats.append(m)
        kps.append(c.trans_keypoints(k, m))
    out["trans_out"], out["trans_kp_out"] = np.stack(mats), np.stack(kps)

    # ---- colour jitter: every order once, alternating between the two clips; then each operation alone --------------------------
    pa, pb = make_patches(rng)
    out["patch_a"], out["patch_b"] = pa, pb
    orders, factors, res_a, res_b = [], [], [], []
    for i, perm in enumerate(itertools.permutations(range(4))):
        f = [rng.uniform(0.7, 1.3), rng.uniform(0.7, 1.3), rng.uniform(0.7, 1.3), rng.uniform(-0.3, 0.3)]      # brightness, contrast, saturation, hue
        j = jit.ColorJitterVideo(0.3, 0.3, 0.3, 0.3)
        j.get_params = lambda *a, f=f: tuple(f)
        keep = random.shuffle
        random.shuffle = lambda lst, perm=perm: lst.__setitem__(slice(None), [lst[k] for k in perm])
        try:
            clip = (pa, pb)[i % 2]
            res = j({"clip": [clip[(i // 2) % 2].copy()]})["clip"]
        finally:
            random.shuffle = keep
        orders.append([[1, 2, 3, 4][k] for k in perm])     # reference list order = brightness, saturation, hue, contrast = codes 1, 2, 3, 4
        factors.append(f)
        (res_a, res_b)[i % 2].append(np.array(res[0]))
    out["jit_orders"], out["jit_factors"] = np.array(orders, dtype=np.int32), np.array(factors)
    out["jit_out_a"], out["jit_out_b"] = np.stack(res_a), np.stack(res_b)
    single, single_f = [], []
    for code, fvals in ((1, (0.7, 1.3)), (2, (0.7, 1.3)), (3, (-0.3, 0.11)), (4, (0.7, 1.3))):
        for fv in fvals:
            f = [None, None, None, None]
            f[{1: 0, 4: 1, 2: 2, 3: 3}[code]] = fv
            j = jit.ColorJitterVideo(0.3, 0.3, 0.3, 0.3)
            j.get_params = lambda *a, f=f: tuple(f)
            single.append(np.stack([np.array(x) for x in j({"clip": [pb[0].copy(), pb[1].copy()]})["clip"]]))
            single_f.append([code, fv])
    out["single_out"], out["single_ops"] = np.stack(single), np.array(single_f)

    # ---- erase: the four sides through the reference's own methods -----------------------------------------------------------------
    e = er.RandomEraseVideo(1.0, 0.7, False, False, 0.1)
    methods = [e._erase_left, e._erase_right, e._erase_top, e._erase_bottom]       # the order of the reference's choice list
    ratios = np.array([[0.31, 0.0], [0.12, 0.655], [0.5, 0.02], [0.699, 0.25]])
    out["erase_ratios"] = ratios
    out["erase_out"] = np.stack([np.stack([m(pa[t].copy(), np.zeros((49, 3)), None, r)[0] for t, r in enumerate(rs)]) for m, rs in zip(methods, ratios)])

    # ---- flip: pixels and the three target flips ---------------------------------------------------------------------------------
    kp2 = np.concatenate([rng.uniform(0, 48, (2, 49, 2)), rng.integers(0, 2, (2, 49, 1)).astype(np.float64)], -1)
    kp3 = np.concatenate([rng.normal(0, 0.4, (2, 49, 3)), np.ones((2, 49, 1))], -1)
    pose = rng.normal(0, 0.5, (2, 72))
    f = fl.RandomHorizontalFlipVideo(1.0)
    r = f({"clip": [pa[0].copy(), pa[1].copy()], "kp_2d": kp2.copy(), "kp_3d": kp3.copy(), "pose": pose.copy()})
    out["flip_kp2_in"], out["flip_kp3_in"], out["flip_pose_in"] = kp2, kp3, pose
    out["flip_out"] = np.stack([np.array(x) for x in r["clip"]])
    out["flip_kp2_out"], out["flip_kp3_out"], out["flip_pose_out"] = r["kp_2d"], r["kp_3d"], r["pose"]
    names, names_f = kp.get_spin_joint_names(), kp.get_spin_joint_names(True)
    out["spin_flip_perm"] = np.array([names.index(n) for n in names_f], dtype=np.int32)

    # ---- stack + to-tensor + normalise -------------------------------------------------------------------------------------------
    chain = [basic.StackFrames(), basic.ToTensorVideo(), basic.NormalizeVideo()]
    inst = {"clip": [Image.fromarray(pb[0]), Image.fromarray(pb[1])], "kp_2d": np.concatenate([rng.uniform(0, 224, (2, 49, 2)), np.ones((2, 49, 1))], -1)}
    out["norm_kp_in"] = inst["kp_2d"].copy()
    for t in chain:
        inst = t(inst)
    out["norm_out"], out["norm_kp_out"] = inst["clip"].numpy(), inst["kp_2d"].numpy()

    # ---- the whole chain after the warp, two clips --------------------------------------------------------------------------------
    for tag, clip, order, fac, side, rs in (("a", pa, (3, 0, 1, 2), [1.21, 0.78, 1.12, -0.17], 1, (0.4, 0.0)), ("b", pb, (2, 3, 0, 1), [0.83, 1.27, 0.74, 0.23], 2, (0.0, 0.3))):
        j = jit.ColorJitterVideo(0.3, 0.3, 0.3, 0.3)
        j.get_params = lambda *a, fac=fac: tuple(fac)
        keep = random.shuffle
        random.shuffle = lambda lst, order=order: lst.__setitem__(slice(None), [lst[k] for k in order])
        try:
            inst = j({"clip": [clip[0].copy(), clip[1].copy()]})
        finally:
            random.shuffle = keep
        frames = [np.array(x) for x in inst["clip"]]
        frames = [methods[side](fr, np.zeros((49, 3)), None, r)[0] for fr, r in zip(frames, rs)]
        inst = fl.RandomHorizontalFlipVideo(1.0)({"clip": frames, "kp_2d": np.zeros((2, 49, 3))})
        inst = {"clip": inst["clip"]}
        for t in chain:
            inst = t(inst)
        out[f"chain_{tag}_order"] = np.array([[1, 2, 3, 4][k] for k in order], dtype=np.int32)
        out[f"chain_{tag}_factors"] = np.array(fac)
        out[f"chain_{tag}_erase"] = np.array([side, *rs])
        out[f"chain_{tag}_out"] = inst["clip"].numpy()

    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
