"""Host side of the clip preprocessing (maed_amd/data.py) against the reference's recorded outputs (tests/golden/g16_clip_preprocess.npz): crop matrices,
affine keypoints, the three flips, normalize_2d_kp -- fp64 numpy on both sides, compared at 1e-12 relative (the only freedom is the order of a handful of
additions); the distributions and granularity of ClipAugment.sample; the region arithmetic of pack_clips."""
import dataclasses

import numpy as np
import pytest

import _preprocess_ref as R
from maed_amd import data as D


@pytest.fixture(scope="module")
def g16(golden):
    return golden("g16_clip_preprocess")


def close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref).max()
    print(f"{what}: max abs error {err:.3e} at scale {np.abs(ref).max():.3e}")
    assert err <= 1e-12 * max(1.0, np.abs(ref).max()), what


def test_crop_matrices_and_affine_keypoints(g16):
    for case, kp_in, m_ref, kp_ref in zip(g16["trans_cases"], g16["trans_kp_in"], g16["trans_out"], g16["trans_kp_out"]):
        h, w, *bbox = case[:6]
        s, rot, sx, sy = case[6:]
        m = D.gen_trans(bbox, (s, s), rot, (sx, sy), w, h)
        close(m, m_ref, "gen_trans")
        kp = D.trans_keypoints(kp_in, m)
        close(kp, kp_ref, "trans_keypoints")
        assert (kp[:, 2] == kp_in[:, 2]).all()           # visibility column untouched
        inv = D.invert_affine(m)
        close(np.concatenate([m, [[0, 0, 1]]]) @ np.concatenate([inv, [[0, 0, 1]]]), np.eye(3), "inverse")


def test_flips_and_keypoint_normalisation(g16):
    assert list(g16["spin_flip_perm"]) == list(D.SPIN_FLIP_PERM)
    close(D.keypoint_2d_hflip(g16["flip_kp2_in"], 48), g16["flip_kp2_out"], "keypoint_2d_hflip")
    close(D.keypoint_3d_hflip(g16["flip_kp3_in"]), g16["flip_kp3_out"], "keypoint_3d_hflip")
    close(D.smpl_pose_hflip(g16["flip_pose_in"]), g16["flip_pose_out"], "smpl_pose_hflip")
    kp = g16["norm_kp_in"].copy()
    kp[..., :2] = D.normalize_2d_kp(kp[..., :2], 224)
    close(kp, g16["norm_kp_out"], "normalize_2d_kp")


def test_targets_compose_crop_flip_normalise(g16):
    aug = D.ClipAugment(64, 48)
    case = g16["trans_cases"][3]
    rec = D.ClipParams(bboxes=np.array([case[2:6], case[2:6]]), scale=(case[6], case[6]), rot=case[7], shift=(case[8], case[9]), flip=True)
    kp_in = g16["trans_kp_in"][3]
    out = aug.targets(rec, kp_2d=np.stack([kp_in, kp_in]), kp_3d=g16["flip_kp3_in"], pose=g16["flip_pose_in"])
    ref = D.keypoint_2d_hflip(g16["trans_kp_out"][3][None], 48)[0]
    ref[:, :2] = 2.0 * ref[:, :2] * (1.0 / 224) - 1.0
    close(out["kp_2d"][1], ref, "targets kp_2d")
    close(out["kp_3d"], g16["flip_kp3_out"], "targets kp_3d")
    close(out["pose"], g16["flip_pose_out"], "targets pose")
    rec.flip = False
    out = aug.targets(rec, kp_2d=np.stack([kp_in, kp_in]), pose=g16["flip_pose_in"], normalize=False)
    close(out["kp_2d"][0], g16["trans_kp_out"][3], "targets without flip")
    assert (out["pose"] == g16["flip_pose_in"]).all()


def test_sample_distributions_and_granularity():
    aug = D.ClipAugment(rot_jitter=30., size_jitter=0.2, random_crop_p=0.2, random_crop_size=0.6, color_jitter=0.3, erase_prob=0.3, erase_part=0.7, flip_p=0.5, seed=1)
    boxes = np.tile([100., 100., 50., 80.], (16, 1))
    recs = [aug.sample(boxes) for _ in range(2000)]
    cropped = np.array([r.shift != (0.0, 0.0) for r in recs])
    assert 0.15 < cropped.mean() < 0.25
    for r, c in zip(recs, cropped):
        assert r.scale[0] == r.scale[1] and -30 <= r.rot <= 30
        if c:
            assert 0.7 <= r.scale[0] <= 1.3 and all(abs(s) <= (1.3 - r.scale[0]) / 2 for s in r.shift)
        else:
            assert 1.1 <= r.scale[0] <= 1.5
        assert 0.7 <= r.brightness <= 1.3 and 0.7 <= r.contrast <= 1.3 and 0.7 <= r.saturation <= 1.3 and -0.3 <= r.hue <= 0.3
        assert sorted(r.jitter_order) == [1, 2, 3, 4]
        assert r.erase_side in (0, 1, 2, 3) and r.erase_ratio.shape == (16,) and (r.erase_ratio >= 0).all() and (r.erase_ratio <= 0.7).all()
    # per-clip draws are scalars / one tuple; the erase draw is per frame: inside one clip some frames are hit and some are not
    ratios = np.stack([r.erase_ratio for r in recs])
    assert 0.27 < (ratios > 0).mean() < 0.33
    assert np.mean([(0 < (x > 0).sum() < 16) for x in ratios]) > 0.9
    assert len({r.jitter_order for r in recs}) == 24 and {r.erase_side for r in recs} == {0, 1, 2, 3}
    assert 0.45 < np.mean([r.flip for r in recs]) < 0.55
    assert abs(np.mean([r.scale[0] for r, c in zip(recs, cropped) if not c]) - 1.3) < 0.01
    # the same seed gives the same draws; the evaluation transform draws nothing
    a, b = D.ClipAugment(color_jitter=0.3, seed=7).sample(boxes), D.ClipAugment(color_jitter=0.3, seed=7).sample(boxes)
    assert a.jitter_order == b.jitter_order and a.brightness == b.brightness
    e = D.ClipAugment.eval().sample(boxes)
    assert e.scale == (1.3, 1.3) and e.rot == 0 and e.shift == (0.0, 0.0) and e.jitter_order == () and not e.flip and not e.erase_ratio.any()


def test_erase_rows_follow_the_code_not_the_names():
    aug = D.ClipAugment(64, 48)
    rows = lambda side, r: aug.erase_rows(D.ClipParams(bboxes=np.zeros((1, 4)), erase_side=side, erase_ratio=np.array([r])))[0].tolist()
    assert rows(D.ERASE_LEFT, 0.5) == [24, 0] and rows(D.ERASE_RIGHT, 0.5) == [0, 24]        # int(w * ratio) ROWS
    assert rows(D.ERASE_TOP, 0.5) == [32, 0] and rows(D.ERASE_BOTTOM, 0.26) == [0, 16]
    assert rows(D.ERASE_TOP, 0.0) == [0, 0]


def test_unbuilt_settings_raise():
    with pytest.raises(NotImplementedError, match=r"random_erase\.py:26"):
        D.ClipAugment(erase_fill=True)
    with pytest.raises(NotImplementedError, match=r"random_erase\.py:31"):
        D.ClipAugment(erase_kp=True)


def _one(img, bbox, H=16, W=16, **kw):
    rec = D.ClipParams(bboxes=np.array([bbox], dtype=np.float64), **kw)
    return D.pack_clips([[img]], [rec], D.ClipAugment(H, W)), rec


def test_pack_clips_region_arithmetic():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (60, 80, 3), dtype=np.uint8)
    # quads leaving the image on every side, wholly outside, and a 1-pixel-wide region
    for bbox, rot in (([40., 30., 20., 20.], 0.), ([2., 30., 30., 30.], 10.), ([78., 30., 30., 30.], -10.), ([40., 1., 30., 30.], 45.), ([40., 59., 30., 30.], 0.),
                      ([40., 30., 300., 300.], 33.), ([-200., -200., 20., 20.], 0.), ([500., 30., 20., 20.], 0.), ([-13.6, 30., 20., 20.], 0.)):
        p, rec = _one(img, bbox, rot=rot)
        D.validate_packed(p)
        off, h, w, pitch, clip = (int(v) for v in p.frame_i[0, :5])
        assert off == 0 and pitch == 3 * w and clip == 0 and 1 <= h <= 60 and 1 <= w <= 80 and p.src_bytes == h * w * 3
        # the region is a verbatim slice of the frame and the shifted map addresses it: sampling the region equals sampling the whole frame
        M = D.gen_trans(bbox, rec.scale, rot, rec.shift, 16, 16)
        whole = R.warp_fp64(img, D.invert_affine(M), 16, 16)
        ref, patches = R.packed_reference(p)
        d = np.abs(patches[0].astype(int) - whole.astype(int))
        assert d.max() <= 1, (bbox, d.max())         # (fp32 storage of the shifted map flips rounding ties only; a region off by one pixel moves this noise image by ~100 levels)
        if bbox[0] < -100 or bbox[0] > 400:
            assert not patches.any() and (h, w) != (0, 0)                        # wholly outside: all-zero patch before normalisation
            assert np.array_equal(ref[0], R.normalise_f32(np.zeros((16, 16, 3), np.uint8)))
    p, _ = _one(img, [-13.6, 30., 20., 20.])
    assert int(p.frame_i[0, 2]) == 1                                              # the 1-pixel-wide region: only column 0 can be touched


def test_pack_clips_layout_and_refusals():
    rng = np.random.default_rng(1)
    frames, records = R.random_scene(3, 2, 3, 16, 16, lo=20, hi=200)
    p = D.pack_clips(frames, records, D.ClipAugment(16, 16))
    assert (p.N, p.T, p.H, p.W) == (2, 3, 16, 16) and p.frame_i.shape == (6, 8) and p.has_contrast
    assert p.frame_i[:, 4].tolist() == [0, 0, 0, 1, 1, 1] and p.offsets[4] % 256 == 0
    assert p.frame_i.base is not None and p.blob.dtype.is_floating_point is False       # the tables are views into the one staging buffer
    ends = p.frame_i[:, 0].astype(np.int64) + p.frame_i[:, 1].astype(np.int64) * p.frame_i[:, 3]
    assert ends[-1] == p.src_bytes and (np.diff(p.frame_i[:, 0]) > 0).all()
    D.validate_packed(p)
    with pytest.raises(ValueError):
        D.pack_clips(frames, records[:1])
    with pytest.raises(ValueError):
        D.pack_clips([[f.astype(np.float32) for f in frames[0]]], records[:1])
    bad = D.ClipParams(bboxes=records[0].bboxes, jitter_order=(1, 1))
    with pytest.raises(ValueError):
        D.pack_clips(frames[:1], [bad])
    from maed_amd._lib import MaedHipError
    # the tables are views of the one buffer, made on demand: a write through them is what the kernel will read, and there is no second copy to disagree with
    p.clip_f[0, 0] = 0.5
    assert p.blob.numpy()[p.offsets[3]:p.offsets[3] + 4].view(np.float32)[0] == 0.5 and p.clip_f[0, 0] == 0.5
    short = dataclasses.replace(p, blob=p.blob[:p.offsets[4] + p.src_bytes - 1].clone())
    with pytest.raises(MaedHipError, match="shorter"):
        D.validate_packed(short)
    with pytest.raises(MaedHipError, match="too short for the tables"):      # a parameter array of the wrong length: the buffer ends inside a table
        D.validate_packed(dataclasses.replace(p, blob=p.blob[:p.offsets[3] + 8].clone()))
    with pytest.raises(MaedHipError):                                       # extents that announce more frames than the tables hold
        D.validate_packed(dataclasses.replace(p, T=p.T + 40))
    del rng


def test_pack_clips_does_not_touch_the_gpu_runtime_and_survives_pickle():
    import pickle
    import torch
    frames, records = R.random_scene(3, 2, 2, 16, 16, lo=20, hi=200)
    was = torch.cuda.is_initialized()
    p = D.pack_clips(frames, records, D.ClipAugment(16, 16))
    assert torch.cuda.is_initialized() == was and not p.blob.is_pinned()
    q = pickle.loads(pickle.dumps(p))
    assert torch.equal(q.blob, p.blob) and (q.N, q.T, q.H, q.W, q.src_bytes, q.mean, q.std) == (p.N, p.T, p.H, p.W, p.src_bytes, p.mean, p.std)
    assert np.array_equal(q.frame_i, p.frame_i) and np.shares_memory(q.clip_f, q.blob.numpy())
    D.validate_packed(q)
