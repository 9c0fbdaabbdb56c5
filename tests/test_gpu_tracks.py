"""csrc/tracks.hip and maed_amd/video.py on the MI355X: maed_track_boxes against the reference's recorded results (tests/golden/g19_tracks.npz), maed_crop_tables
against its closed form, the crops of device-built tables against the fp64 restatement of the clip preprocessing, and VideoInference end to end on a small MAED,
through to render_frame_results.  The cases and bars are those of tests/test_hostsim_tracks.py (tests/_tracks_cases.py); every launch here is a few tracks of at
most 1027 frames or a few crops of small frames."""
import numpy as np
import pytest
import torch

import _preprocess_ref as R
import _tracks_cases as TC
from _util import note

pytestmark = [pytest.mark.gpu]


def run_tracks(kps, lengths, vis, k, sigma, box_scale=1.1):
    from maed_amd import video as V
    kps_d = torch.from_numpy(np.ascontiguousarray(kps, dtype=np.float32)).cuda()
    len_d = torch.tensor(list(lengths), dtype=torch.int32, device="cuda")
    boxes, span, params = V.track_boxes(kps_d, len_d, vis, k, sigma, box_scale, return_params=True)
    torch.cuda.synchronize()
    return boxes.cpu().numpy(), params.cpu().numpy(), span.cpu().numpy()


def run_tables(boxes, box_index, frame_index, T, n_frames, h, w, H, W, keep=None):
    """maed_crop_tables with guard rows behind every table; keep: a dict that receives the device tensors"""
    from maed_amd import _lib as L
    from maed_amd import ops
    b = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)).cuda()
    bi = torch.tensor(list(box_index), dtype=torch.int32, device="cuda")
    fi = torch.tensor(list(frame_index), dtype=torch.int32, device="cuda")
    M, G = len(bi), 2
    N = -(-M // T)
    t = dict(frame_i=torch.full((M + G, 8), -777, dtype=torch.int32, device="cuda"), frame_minv=torch.full((M + G, 6), -777.0, device="cuda"),
             clip_i=torch.full((N + G, 8), -777, dtype=torch.int32, device="cuda"), clip_f=torch.full((N + G, 4), -777.0, device="cuda"))
    L.check(L.lib().maed_crop_tables(b.data_ptr(), len(b), bi.data_ptr(), fi.data_ptr(), M, T, n_frames, h, w, H, W, t["frame_i"].data_ptr(), t["frame_minv"].data_ptr(),
                                     t["clip_i"].data_ptr(), t["clip_f"].data_ptr(), ops._stream()), "crop_tables")
    torch.cuda.synchronize()
    if keep is not None:
        keep.update(t)
    host = {k: v.cpu().numpy() for k, v in t.items()}
    for k, n in (("frame_i", M), ("frame_minv", M), ("clip_i", N), ("clip_f", N)):
        assert (host[k][n:] == -777).all(), f"a guard row behind {k} was written"
        host[k] = host[k][:n]
    return host


@pytest.mark.parametrize("name", [c["name"] for c in TC.cases()])
def test_track_matches_the_reference(name):
    c = TC.case(name)
    boxes, params, span = run_tracks(c["kps"][None], [len(c["kps"])], c["vis"], c["k"], c["sigma"])
    err = TC.check_track(c, boxes[0], params[0], span[0])
    note(f"tracks {name:24s} max |params - ref| {err:.3e} (bar {TC.params_bar(c['params']):.3e})")


def test_five_tracks_of_unequal_lengths_in_one_launch():
    """lengths shorter than L (NaN behind them, never read); output rows behind a track's length are zero; the same bits as one track per launch"""
    cs = [TC.case(f"span{m}_s3") for m in (1, 6, 13, 26, 97)]
    kps, lengths = TC.pad_tracks(cs, extra=3)
    boxes, params, span = run_tracks(kps, lengths, cs[0]["vis"], cs[0]["k"], cs[0]["sigma"])
    for k, c in enumerate(cs):
        TC.check_track(c, boxes[k], params[k], span[k])
        b1, p1, _ = run_tracks(c["kps"][None], [len(c["kps"])], c["vis"], c["k"], c["sigma"])
        n = len(c["kps"])
        assert np.array_equal(p1[0], params[k, :n]) and np.array_equal(b1[0], boxes[k, :n], equal_nan=True)


def test_both_forms_in_one_launch():
    """L = 1027: the 1024-frame track keeps its series in LDS, the 1025-frame track in the workspace"""
    cs = [TC.case("len1024"), TC.case("len1025")]
    kps, lengths = TC.pad_tracks(cs, extra=2)
    boxes, params, span = run_tracks(kps, lengths, cs[0]["vis"], cs[0]["k"], cs[0]["sigma"])
    for k, c in enumerate(cs):
        TC.check_track(c, boxes[k], params[k], span[k])


def test_track_of_2_20_frames():
    """no length limit below L = 2^20: one track of 1048576 frames in the workspace form against the closed form of tests/_tracks_cases.line_track (every interior
    row is checked, so a wrong index anywhere in the 48 MB of series shows)"""
    L = 1 << 20
    boxes, params, span = run_tracks(TC.line_track(L), [L], 0.1, 11, 8.0)
    err = TC.check_line(L, boxes, params, span, 11, 8.0)
    note(f"tracks line of {L} frames: max |params - closed form| {err:.3e}")


def test_tracks_without_a_valid_frame():
    rng = np.random.default_rng(0)
    one = rng.uniform(10, 200, (2, 9, 1, 3)).astype(np.float32)               # J = 1 is always invalid
    boxes, params, span = run_tracks(one, [9, 4], 0.1, 11, 3.0)
    assert (span == [[-1, 0], [-1, 0]]).all() and not boxes.any() and not params.any()
    mixed = rng.uniform(10, 200, (3, 7, 5, 3)).astype(np.float32)
    mixed[0, :, :, 2] = 0.05
    mixed[1, :, :, :2] = 50 + rng.uniform(0, 0.2, (7, 5, 2))
    boxes, params, span = run_tracks(mixed, [7, 7, 0], 0.1, 3, 0.5)
    assert (span == -1 * np.array([[1, 0]] * 3)).all() and not boxes.any() and not params.any()


def test_reference_named_functions():
    from maed_amd import video as V
    for name in ("span7_s3", "all_but_ends_mixed", "k31"):
        c = TC.case(name)
        params, start, end = V.get_smooth_bbox_params(c["list"], vis_thresh=c["vis"], kernel_size=c["k"], sigma=c["sigma"])
        assert (start, end) == c["span"] and np.abs(params - c["params"]).max() <= TC.params_bar(c["params"])
        raw, s2, e2 = V.get_all_bbox_params(c["list"], vis_thresh=c["vis"])
        assert (s2, e2) == c["span"] and np.abs(raw - c["raw"]).max() <= TC.params_bar(c["raw"])
        assert np.abs(V.smooth_bbox_params(c["raw"], kernel_size=c["k"], sigma=c["sigma"]) - c["params"][start:]).max() <= TC.params_bar(c["params"])
        assert np.abs(V.kp_to_bbox_param(c["list"][start], c["vis"]) - c["raw"][0]).max() <= TC.params_bar(c["raw"])


@pytest.mark.parametrize("h,w,B", [(96, 128, 3), (270, 480, 2)])
def test_crop_tables(h, w, B):
    for exact in (True, False):
        boxes = TC.scene_boxes(h, w, exact)
        for T, P, M in ((4, 64, 12), (5, 224, 11)):
            bi = (np.arange(M) * 5) % len(boxes)
            fi = np.arange(M) % B
            TC.check_tables(run_tables(boxes, bi, fi, T, B, h, w, P, P), boxes, bi, fi, T, h, w, P, P)
    t = run_tables(boxes, [0, len(boxes), -1, 0], [0, 0, 0, B], 2, B, h, w, 64, 64)
    assert np.array_equal(t["frame_minv"][1:], np.tile(np.float32([0, 0, -2, 0, 0, -2]), (3, 1))) and (t["frame_i"][1:, 0] == 0).all()


def _crops(frames, boxes, T, P):
    from maed_amd import ops
    B, h, w = frames.shape[:3]
    M = len(boxes)
    dev = {}
    t = run_tables(boxes, np.arange(M), np.arange(M) % B, T, B, h, w, P, P, keep=dev)
    flat = torch.from_numpy(np.ascontiguousarray(frames)).cuda().view(-1)
    got = torch.full((M, 3, P, P), float("nan"), device="cuda")
    rel = [dev[k].data_ptr() - flat.data_ptr() for k in ("frame_i", "frame_minv", "clip_i", "clip_f")]
    ops.clip_preprocess(flat, (*rel, 0), flat.numel(), M, M // T, P, P, R.MEAN, R.STD, False, got)
    torch.cuda.synchronize()
    ref, patches = R.packed_reference(TC.packed_from_tables(t, frames, T, P, P))
    return got.cpu().numpy(), ref, patches


@pytest.mark.parametrize("h,w,B,P", [(96, 128, 3, 64), (270, 480, 2, 64), (96, 128, 3, 224)])
def test_pixels_of_device_built_tables_bit_equal(h, w, B, P):
    """ops.clip_preprocess on (device frames, tables built on the device) == tests/_preprocess_ref.packed_reference of the same tables copied back and the same whole
    frames, bit for bit (boxes whose maps are exact in fp32: tests/_tracks_cases.scene_boxes)"""
    frames = TC.scene_frames(7, B, h, w)
    boxes = TC.scene_boxes(h, w, True)
    boxes = boxes if P == 64 else boxes[[0, 2, 5, 7]]
    got, ref, patches = _crops(frames, boxes, 4, P)
    diff = got.view(np.uint32) != ref.view(np.uint32)
    note(f"tracks crops {h}x{w} patch {P}: differing values {int(diff.sum())}/{diff.size}")
    assert got.shape == ref.shape and not diff.any()
    bad = TC.degenerate(boxes)
    assert not patches[bad].any() and patches[0].any()


def test_pixels_of_arbitrary_boxes_within_one_level():
    """boxes whose maps are not exact in fp32: the bound the preprocessing tests pin for the existing kernel's fp32 coordinates, one level"""
    frames = TC.scene_frames(8, 3, 96, 128)
    got, ref, _ = _crops(frames, TC.scene_boxes(96, 128, False), 4, 64)
    d = np.abs(R.to_levels(got) - R.to_levels(ref))
    note(f"tracks crops arbitrary boxes: max level difference {d.max()}, share {np.mean(d > 0):.5f}")
    assert d.max() <= 1


def test_refusals_on_device_tensors():
    from maed_amd import video as V
    from maed_amd import _lib as L
    kps = torch.ones((1, 4, 3, 3), device="cuda")
    n = torch.tensor([4], dtype=torch.int32, device="cuda")
    for kw, pat in ((dict(kernel_size=4), "odd"), (dict(sigma=0.0), "> 0"), (dict(sigma=128.2), "512")):
        with pytest.raises(ValueError, match=pat):
            V.track_boxes(kps, n, 0.1, **kw)
    with pytest.raises(ValueError, match="64"):
        V.track_boxes(torch.ones((1, 2, 65, 3), device="cuda"), torch.tensor([2], dtype=torch.int32, device="cuda"))
    with pytest.raises(L.MaedHipError, match="no CPU path"):
        V.track_boxes(kps.cpu(), n.cpu())
    # the library's own host checks (nothing is launched)
    lib = L.lib()
    z = torch.zeros(64, device="cuda")
    assert lib.maed_track_boxes(kps.data_ptr(), n.data_ptr(), 1, 4, 3, 0.1, 12, 3.0, 1.1, z.data_ptr(), None, z.data_ptr(), None, 0, None) != 0
    assert "odd" in lib.maed_last_error().decode()
    assert lib.maed_crop_tables(z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), 1, 1, 87, 2160, 3840, 64, 64, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None) != 0
    assert "2^31" in lib.maed_last_error().decode()
    assert lib.maed_crop_tables(z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), 65536, 16, 1, 32, 32, 64, 64, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None) != 0
    assert "65535" in lib.maed_last_error().decode()
    assert lib.maed_crop_tables(z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), 1, 1, 1, 32, 32, 64, 62, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None) != 0
    assert "multiple of 4" in lib.maed_last_error().decode()


def test_driver_end_to_end_and_render():
    """two people in 24 frames of 96 x 128 through MAED(num_blocks=2, num_heads=2, embed_dim=128, hidden_dim=64, img_size=64, bf16): the outputs equal a hand-driven
    model(clips) on the driver's own crops (bit-equal if the eval forward is bit-identical from run to run, else within four times the spread of two hand-driven
    runs; the figures are printed), orig_cam follows from them, and prepare_rendering_results / render_frame_results take the results as they are"""
    from maed_amd import MAED
    from maed_amd import video as V
    from maed_amd.render import FaceList, prepare_rendering_results, render_frame_results
    torch.manual_seed(0)
    model = MAED(num_blocks=2, num_heads=2, embed_dim=128, hidden_dim=64, img_size=64, compute_dtype=torch.bfloat16).cuda()
    with torch.no_grad():
        model.decoder.deccam.bias.copy_(torch.tensor([0.9, 0.0, 0.0]))          # the usual initial camera: the mesh is about as large as its box
    frames_np, tracks = TC.driver_scene()
    B, h, w = frames_np.shape[:3]
    frames = torch.from_numpy(frames_np).cuda()
    vi = V.VideoInference(model, seqlen=16, clips_per_batch=2, patch=64, vis_thresh=0.3, kernel_size=11, sigma=3)
    results, skipped, dbg = vi.run(frames, tracks, debug=True)
    assert [len(c["windows"]) for c in dbg["chunks"]] == [2, 1]
    for key, (d, spread) in TC.check_driver(results, skipped, dbg, model, tracks, h, w).items():
        note(f"tracks driver {key:16s} difference to the hand-driven forward {d:.3e}, spread of two hand-driven runs {spread:.3e}")
    plain, none = vi.run(frames, tracks)
    assert not none and all(torch.equal(plain[p]["bboxes"], results[p]["bboxes"]) for p in results)
    per_frame = prepare_rendering_results(results, B)
    V_n = int(results["kp"]["verts"].shape[1])
    tri = np.arange(0, V_n - 2, 3)
    faces = np.concatenate([np.stack([tri, tri + 1, tri + 2], 1), np.stack([tri, tri + 2, tri + 1], 1)])      # both windings: whatever faces the camera is drawn
    out = render_frame_results(frames.clone(), per_frame, FaceList(faces, V_n))
    torch.cuda.synchronize()
    changed = (out != frames).reshape(B, -1).any(dim=1).cpu().numpy()
    present = np.array([any(f in set(tracks[p]["frames"]) for p in tracks) for f in range(B)])
    note(f"tracks driver render: frames drawn on {changed.astype(int).tolist()}")
    assert np.array_equal(changed, present)
