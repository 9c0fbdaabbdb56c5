"""csrc/tracks.hip on the host simulator (tests/_hostsim_tracks.py): maed_track_boxes against the reference's recorded results (tests/golden/g19_tracks.npz) at the
shapes where the kernel can go wrong, maed_crop_tables against its closed form, the crops of device-built tables against the fp64 restatement of the clip
preprocessing, the reference-named functions of maed_amd/video.py, the refusals, and VideoInference end to end.  No GPU."""
import numpy as np
import pytest
import torch

import _hostsim_tracks as S
import _preprocess_ref as R
import _tracks_cases as TC


def run_tracks(kps, lengths, vis, k, sigma, box_scale=1.1):
    return S.track_boxes(kps, lengths, vis, k, sigma, box_scale)


def run_tables(boxes, box_index, frame_index, T, n_frames, h, w, H, W):
    return S.crop_tables(boxes, box_index, frame_index, T, n_frames, h, w, H, W)


@pytest.mark.parametrize("name", [c["name"] for c in TC.cases()])
def test_track_matches_the_reference(name):
    """K = 1, L = the track: spans 1, 5, 6, 7 (around (k + 1) / 2), 12 .. 26 (around r and 2 r + 1 for sigma 3), 97 (the reflect map wraps for sigma 8), gaps in
    front, behind, inside, of one frame and of all frames but two, every reason a frame is invalid for, J 2 .. 64, k 1 .. 63, sigma 0.5 .. 8, both sides of the
    1024-frame boundary between the LDS and the workspace form"""
    c = TC.case(name)
    boxes, params, span = run_tracks(c["kps"][None], [len(c["kps"])], c["vis"], c["k"], c["sigma"])
    TC.check_track(c, boxes[0], params[0], span[0])


def test_short_spans_give_infinite_boxes_and_span_six_does_not():
    for m, inf in ((1, True), (5, True), (6, False), (7, False)):
        c = TC.case(f"span{m}_s3")
        boxes, params, span = run_tracks(c["kps"][None], [len(c["kps"])], c["vis"], c["k"], c["sigma"])
        s, e = span[0]
        assert np.isinf(boxes[0, s:e, 2:]).all() == inf and (params[0, s:e, 2] == 0).all() == inf, m


def test_five_tracks_of_unequal_lengths_in_one_launch():
    """lengths shorter than L (the rows behind them hold NaN and are never read), guard rows behind every output (the runner checks them), and the same bits as
    one track per launch"""
    cs = [TC.case(f"span{m}_s3") for m in (1, 6, 13, 26, 97)]
    kps, lengths = TC.pad_tracks(cs, extra=3)
    boxes, params, span = run_tracks(kps, lengths, cs[0]["vis"], cs[0]["k"], cs[0]["sigma"])
    for k, c in enumerate(cs):
        TC.check_track(c, boxes[k], params[k], span[k])
        b1, p1, _ = run_tracks(c["kps"][None], [len(c["kps"])], c["vis"], c["k"], c["sigma"])
        n = len(c["kps"])
        assert np.array_equal(p1[0], params[k, :n]) and np.array_equal(b1[0], boxes[k, :n], equal_nan=True)


def test_both_forms_in_one_launch_and_on_their_own():
    """L = 1027 > 1024: the 1024-frame track keeps its series in LDS, the 1025-frame track in the workspace, side by side"""
    cs = [TC.case("len1024"), TC.case("len1025")]
    kps, lengths = TC.pad_tracks(cs, extra=2)
    boxes, params, span = run_tracks(kps, lengths, cs[0]["vis"], cs[0]["k"], cs[0]["sigma"])
    for k, c in enumerate(cs):
        TC.check_track(c, boxes[k], params[k], span[k])


def test_long_line_in_the_workspace_form():
    """3000 frames (workspace form) against the closed form of tests/_tracks_cases.line_track; the GPU test runs the same at 2^20 frames"""
    L = 3000
    boxes, params, span = run_tracks(TC.line_track(L), [L], 0.1, 11, 8.0)
    TC.check_line(L, boxes, params, span, 11, 8.0)


def test_tracks_without_a_valid_frame():
    """the one place where behaviour is defined, not copied: span (-1, 0), every row zero.  J = 1 is always invalid (a rectangle of one point has height 0)"""
    rng = np.random.default_rng(0)
    one = rng.uniform(10, 200, (2, 9, 1, 3)).astype(np.float32)
    boxes, params, span = run_tracks(one, [9, 4], 0.1, 11, 3.0)
    assert (span == [[-1, 0], [-1, 0]]).all() and not boxes.any() and not params.any()
    mixed = rng.uniform(10, 200, (3, 7, 5, 3)).astype(np.float32)
    mixed[0, :, :, 2] = 0.05                                   # nothing visible
    mixed[1, :, :, :2] = 50 + rng.uniform(0, 0.2, (7, 5, 2))   # height below 0.5
    boxes, params, span = run_tracks(mixed, [7, 7, 0], 0.1, 3, 0.5)     # (and a track of length 0)
    assert (span == -1 * np.array([[1, 0]] * 3)).all() and not boxes.any() and not params.any()


def test_params_are_optional():
    c = TC.case("span26_s3")
    b0, _, s0 = run_tracks(c["kps"][None], [len(c["kps"])], c["vis"], c["k"], c["sigma"])
    b1, p1, s1 = S.track_boxes(c["kps"][None], [len(c["kps"])], c["vis"], c["k"], c["sigma"], want_params=False)
    assert np.array_equal(b0, b1, equal_nan=True) and np.array_equal(s0, s1)


def test_reference_named_functions():
    """acceptance 4: get_smooth_bbox_params, get_all_bbox_params, smooth_bbox_params, kp_to_bbox_param return what the fixture holds"""
    from maed_amd import video as V
    with S.patched():
        for name in ("span7_s3", "span26_s8", "all_but_ends_mixed", "k31", "J49", "span5_s3"):
            c = TC.case(name)
            params, start, end = V.get_smooth_bbox_params(c["list"], vis_thresh=c["vis"], kernel_size=c["k"], sigma=c["sigma"])
            assert (start, end) == c["span"] and params.shape == c["params"].shape and np.abs(params - c["params"]).max() <= TC.params_bar(c["params"])
            raw, s2, e2 = V.get_all_bbox_params(c["list"], vis_thresh=c["vis"])
            assert (s2, e2) == c["span"] and raw.shape == c["raw"].shape and np.abs(raw - c["raw"]).max() <= TC.params_bar(c["raw"])
            sm = V.smooth_bbox_params(c["raw"], kernel_size=c["k"], sigma=c["sigma"])
            assert np.abs(sm - c["params"][start:]).max() <= TC.params_bar(c["params"])
            one = V.kp_to_bbox_param(c["list"][start], c["vis"])
            assert np.abs(one - c["raw"][0]).max() <= TC.params_bar(c["raw"])
        c = TC.case("span12_s3")
        assert V.kp_to_bbox_param(c["list"][0], c["vis"]) is None and V.kp_to_bbox_param(None, 0.1) is None      # frame 0 of these tracks is None
        assert V.kp_to_bbox_param(c["list"][1], c["vis"]) is None                                                # nothing above the threshold
        assert V.get_all_bbox_params([None, None], 0.1)[1:] == (-1, 0)
        with pytest.raises(ValueError, match="no frame"):
            V.get_smooth_bbox_params([None, None], 0.1)
        # the defaults are the reference's
        import inspect
        assert [p.default for p in inspect.signature(V.get_smooth_bbox_params).parameters.values()][1:] == [2, 11, 3]
        assert [p.default for p in inspect.signature(V.smooth_bbox_params).parameters.values()][1:] == [11, 8]
        assert [p.default for p in inspect.signature(V.get_all_bbox_params).parameters.values()][1:] == [2]


@pytest.mark.parametrize("h,w,B", [(96, 128, 3), (270, 480, 2)])
@pytest.mark.parametrize("exact", [True, False])
def test_crop_tables(h, w, B, exact):
    boxes = TC.scene_boxes(h, w, exact)
    for T, P in ((4, 64), (5, 224)):
        M = 12 if T == 4 else 11                               # (11 crops in clips of 5: the last clip is short)
        bi = (np.arange(M) * 5) % len(boxes)
        fi = np.arange(M) % B
        t = run_tables(boxes, bi, fi, T, B, h, w, P, P)
        TC.check_tables(t, boxes, bi, fi, T, h, w, P, P)
    # an index outside its table reads nothing: black patch, frame 0
    t = run_tables(boxes, [0, len(boxes), -1, 0], [0, 0, 0, B], 2, B, h, w, 64, 64)
    assert np.array_equal(t["frame_minv"][1:], np.tile(np.float32([0, 0, -2, 0, 0, -2]), (3, 1))) and (t["frame_i"][1:, 0] == 0).all()
    assert t["frame_minv"][0, 0] > 0


def _crops(frames, boxes, T, P):
    B, h, w = frames.shape[:3]
    M = len(boxes)
    bi, fi = np.arange(M), np.arange(M) % B
    t = run_tables(boxes, bi, fi, T, B, h, w, P, P)
    got = torch.empty((M, 3, P, P), dtype=torch.float32)
    flat = torch.from_numpy(np.ascontiguousarray(frames)).view(-1)
    tabs = {k: torch.from_numpy(v.copy()) for k, v in t.items()}
    from maed_amd import ops
    with S.patched():
        rel = [tabs[k].data_ptr() - flat.data_ptr() for k in ("frame_i", "frame_minv", "clip_i", "clip_f")]
        ops.clip_preprocess(flat, (*rel, 0), flat.numel(), M, M // T, P, P, R.MEAN, R.STD, False, got)
    ref, patches = R.packed_reference(TC.packed_from_tables(t, frames, T, P, P))
    return got.numpy(), ref, patches, boxes


@pytest.mark.parametrize("h,w,B,P", [(96, 128, 3, 64), (270, 480, 2, 64), (96, 128, 3, 224)])
def test_pixels_of_device_built_tables_bit_equal(h, w, B, P):
    """acceptance 6: ops.clip_preprocess on (whole frames, tables built by maed_crop_tables) == tests/_preprocess_ref.packed_reference of the same tables copied
    back and the same frames, bit for bit; boxes inside, over each border, wholly outside, degenerate (black)"""
    frames = TC.scene_frames(7, B, h, w)
    got, ref, patches, boxes = _crops(frames, TC.scene_boxes(h, w, True) if P == 64 else TC.scene_boxes(h, w, True)[[0, 2, 5, 7]], 4, P)
    assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    bad = TC.degenerate(boxes)
    assert not patches[bad].any() and patches[0].any() and patches[~bad].any()
    if P == 64:
        assert not patches[5].any() and not patches[6].any()          # wholly outside the frame
        for m in (1, 2, 3, 4):                                           # over a border: part frame, part black
            assert patches[m].any() and (patches[m].reshape(-1, 3).sum(axis=1) == 0).any(), m


def test_pixels_of_arbitrary_boxes_within_one_level():
    """beyond the acceptance list: boxes whose maps are NOT exact in fp32.  The existing kernel evaluates the map in fp32, the restatement in fp64, so a value may cross
    a rounding tie; tests/test_hostsim_preprocess.py pins that at one level, and so does this"""
    frames = TC.scene_frames(8, 3, 96, 128)
    got, ref, patches, _ = _crops(frames, TC.scene_boxes(96, 128, False), 4, 64)
    d = np.abs(R.to_levels(got) - R.to_levels(ref))
    print(f"arbitrary boxes: max level difference {d.max()}, share {np.mean(d > 0):.5f}")
    assert d.max() <= 1


def test_refusals():
    """acceptance 9: each bad argument is an error whose message names the limit, from the library's host checks and from maed_amd/video.py"""
    from maed_amd import video as V
    from maed_amd._lib import MaedHipError
    kps = np.ones((1, 4, 3, 3), dtype=np.float32)
    for kw, pat in ((dict(kernel_size=4), "odd"), (dict(kernel_size=65), "63"), (dict(sigma=0.0), "> 0"), (dict(sigma=-1.0), "> 0"), (dict(sigma=128.2), "512")):
        args = dict(kernel_size=11, sigma=3.0)
        args.update(kw)
        with pytest.raises(RuntimeError, match=pat):
            S.track_boxes(kps, [4], 0.1, args["kernel_size"], args["sigma"])
        with pytest.raises(ValueError, match=pat):
            V.track_boxes(torch.from_numpy(kps), torch.tensor([4], dtype=torch.int32), 0.1, **args)
    S.track_boxes(kps, [4], 0.1, 11, 128.1)                              # r = int(4 * 128.1 + 0.5) = 512 is the largest radius
    with pytest.raises(RuntimeError, match="64"):
        S.track_boxes(np.ones((1, 2, 65, 3), dtype=np.float32), [2], 0.1, 11, 3.0)
    box = np.float32([[10, 10, 8, 8]])
    with pytest.raises(RuntimeError, match="multiple of 4"):
        S.crop_tables(box, [0], [0], 1, 1, 32, 32, 64, 62)
    with pytest.raises(RuntimeError, match="65535"):
        S.crop_tables(box, np.zeros(65536, dtype=np.int32), np.zeros(65536, dtype=np.int32), 16, 1, 32, 32, 64, 64)
    with pytest.raises(RuntimeError, match=r"2\^31"):
        S.crop_tables(box, [0], [0], 1, 87, 2160, 3840, 64, 64)           # 87 frames of 2160 x 3840 x 3 bytes >= 2^31
    S.crop_tables(box, [0], [85], 1, 86, 2160, 3840, 64, 64)              # 86 are below it
    # CPU tensors are an error, never a fallback (outside the simulator's patch)
    with pytest.raises(MaedHipError, match="no CPU path"):
        V.track_boxes(torch.from_numpy(kps), torch.tensor([4], dtype=torch.int32))
    with pytest.raises(MaedHipError, match="no CPU path"):
        V.VideoInference(TC.StandInModel(), patch=64).run(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), {})
    with pytest.raises(ValueError, match="64"):
        V.track_boxes(torch.ones((1, 2, 65, 3)), torch.tensor([2], dtype=torch.int32))
    with pytest.raises(ValueError, match="multiple of 4"):
        V.VideoInference(TC.StandInModel(), patch=62)


def test_driver_end_to_end_on_the_simulator():
    """acceptance 8 with a stand-in for the model (tests/_tracks_cases.StandInModel: MAED itself needs the GPU, tests/test_gpu_tracks.py): two people, one from
    joints2d over 21 frames with a gap (two windows of 16, the second padded), one from bbox over 16 frames; a third whose keypoints span too few frames and a
    fourth with an infinite box are skipped with the reason"""
    from maed_amd import video as V
    from maed_amd.render import prepare_rendering_results
    frames_np, tracks = TC.driver_scene()
    B, h, w = frames_np.shape[:3]
    model = TC.StandInModel()
    vi = V.VideoInference(model, seqlen=16, clips_per_batch=2, patch=64, vis_thresh=0.3, kernel_size=11, sigma=3)
    extra = dict(tracks)
    extra["short"] = dict(frames=np.arange(5), joints2d=tracks["kp"]["joints2d"][:5])
    extra["hidden"] = dict(frames=np.arange(8), joints2d=tracks["kp"]["joints2d"][:8] * np.float32([1, 1, 0.01]))
    bad = tracks["box"]["bbox"].copy()
    bad[3, 2] = np.inf
    extra["inf"] = dict(frames=np.arange(16), bbox=bad)
    with S.patched():
        results, skipped, dbg = vi.run(torch.from_numpy(frames_np), extra, debug=True)
        assert set(skipped) == {"short", "hidden", "inf"} and "min_frames=6" in skipped["short"] and "no frame" in skipped["hidden"] and "non-finite" in skipped["inf"]
        assert [len(c["windows"]) for c in dbg["chunks"]] == [2, 1] and all(cl.shape[1:] == (16, 3, 64, 64) for cl in dbg["clips"])
        TC.check_driver(results, {}, dbg, model, tracks, h, w)
        # the crops are the frames: the first crop of 'box' is frame 0 at its first box
        t = S.crop_tables(tracks["box"]["bbox"][:1], [0], [0], 1, B, h, w, 64, 64)
        ref, _ = R.packed_reference(TC.packed_from_tables(t, frames_np, 1, 64, 64))
        wins = [(ci, n) for ci, c in enumerate(dbg["chunks"]) for n, (pi, wi, _) in enumerate(c["windows"]) if list(results)[pi] == "box"]
        (ci, n), = wins
        d = np.abs(R.to_levels(dbg["clips"][ci][n, 0].numpy()) - R.to_levels(ref[0]))
        assert d.max() <= 1
    per_frame = prepare_rendering_results(results, B)
    assert len(per_frame) == B
    assert [sorted(p) for p in per_frame] == [sorted(k for k in ("kp", "box") if f in set(tracks[k]["frames"])) for f in range(B)]
