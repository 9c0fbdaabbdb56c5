"""maed_amd.render without a GPU: the camera mapping and the per-frame ordering against recorded outputs of the reference's own functions
(tests/golden/g17_render_cam.npz), set_faces against its definition, the face list's CSR, and the Python API end to end on the host simulator."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import _hostsim_render as S
import _render_cases as K
import _render_ref as R


@pytest.fixture(scope="module")
def g17(golden):
    return golden("g17_render_cam")


def test_convert_crop_cam_matches_the_recorded_reference(g17):
    from maed_amd.render import convert_crop_cam_to_orig_img
    w, h = (int(x) for x in g17["img_wh"])
    got = convert_crop_cam_to_orig_img(g17["cam"], g17["bbox"], w, h)
    assert got.dtype == np.float64 and got.shape == (12, 4)
    assert np.abs(got - g17["orig_cam"]).max() <= 1e-12 * np.abs(g17["orig_cam"]).max()
    assert (np.abs(got - g17["orig_cam"]) <= 1e-12 * np.abs(g17["orig_cam"])).all()
    got32 = convert_crop_cam_to_orig_img(g17["cam"].astype(np.float32), g17["bbox"].astype(np.float32), w, h)
    assert got32.dtype == np.float32
    assert (np.abs(got32.astype(np.float64) - g17["orig_cam"]) <= 1e-6 * np.maximum(1.0, np.abs(g17["orig_cam"]))).all()
    t64 = convert_crop_cam_to_orig_img(torch.from_numpy(g17["cam"]), torch.from_numpy(g17["bbox"]), w, h)
    assert isinstance(t64, torch.Tensor) and t64.dtype == torch.float64
    assert (np.abs(t64.numpy() - g17["orig_cam"]) <= 1e-12 * np.abs(g17["orig_cam"])).all()
    t32 = convert_crop_cam_to_orig_img(torch.from_numpy(g17["cam"]).float(), torch.from_numpy(g17["bbox"]).float(), w, h)
    assert t32.dtype == torch.float32
    assert (np.abs(t32.double().numpy() - g17["orig_cam"]) <= 1e-6 * np.maximum(1.0, np.abs(g17["orig_cam"]))).all()


def test_prepare_rendering_results_matches_the_recorded_reference(g17):
    from maed_amd.render import prepare_rendering_results
    people = OrderedDict((int(p), {k: g17[f"p{int(p)}_{k}"] for k in ("frame_ids", "verts", "orig_cam")}) for p in g17["person_ids"])
    res = prepare_rendering_results(people, int(g17["nframes"]))
    assert len(res) == int(g17["nframes"])
    for fi, frame in enumerate(res):
        want = [int(p) for p in g17["order"][fi] if p >= 0]
        assert isinstance(frame, OrderedDict) and list(frame.keys()) == want, (fi, list(frame.keys()), want)
        for p, rec in frame.items():
            assert np.array_equal(rec["verts"], g17[f"r{fi}_{p}_verts"]) and np.array_equal(rec["cam"], g17[f"r{fi}_{p}_cam"])


def test_set_faces_is_its_three_line_definition():
    from maed_amd.render import Renderer
    v, f = R.icosphere(2)
    idx = np.random.default_rng(0).permutation(len(v))[:90]
    r = Renderer(resolution=(64, 64), faces=f, device="cpu")
    r.set_faces(idx)
    inter = [np.intersect1d(face, idx, assume_unique=True) for face in f]
    want = f[[x.size == 3 for x in inter]]
    assert 0 < len(want) < len(f) and np.array_equal(r.faces, want)


def test_face_list_csr_lists_each_vertex_s_faces_in_ascending_order():
    from maed_amd.render import FaceList
    v, f = R.torus()
    fl = FaceList(f, len(v))
    assert fl.vf_off[0] == 0 and fl.vf_off[-1] == 3 * len(f) and fl.vf_off.dtype == np.int32 and fl.vf_idx.dtype == np.int32
    for vert in (0, 17, len(v) - 1):
        mine = fl.vf_idx[fl.vf_off[vert]:fl.vf_off[vert + 1]]
        assert np.array_equal(mine, np.nonzero((f == vert).any(1))[0])


def test_synthetic_model_has_no_faces_and_says_so():
    from maed_amd._lib import MaedHipError
    from maed_amd.render import Renderer
    from maed_amd.smpl import synthetic_smpl_arrays
    with pytest.raises(MaedHipError, match="synthetic SMPL stand-in .* has no faces"):
        Renderer(resolution=(64, 64))
    with pytest.raises(MaedHipError, match="no faces"):
        Renderer(resolution=(64, 64), smpl_arrays=synthetic_smpl_arrays(0))
    v, f = R.icosphere(1)
    assert len(Renderer(resolution=(64, 64), smpl_arrays={"f": f.astype(np.uint32)}, device="cpu").faces) == len(f)


def test_python_side_refusals():
    from maed_amd._lib import MaedHipError
    from maed_amd.render import FaceList, render_batch
    v, f = R.icosphere(1)
    bad = f.copy()
    bad[3, 2] = len(v)
    with pytest.raises(MaedHipError, match="outside"):
        FaceList(bad, len(v))
    with S.patched():
        with pytest.raises(MaedHipError, match="outside"):                         # the library's own check, through ops.render_mesh
            from maed_amd import ops
            fl = FaceList(f, len(v))
            ft, off, idx = fl.on("cpu")
            bt = torch.from_numpy(bad)
            ops.render_mesh(torch.from_numpy(v)[None].contiguous(), bt, bad, off, idx, torch.tensor([[1.0, 1.0, 0.0, 0.0]]), 32, 32, out=torch.zeros(1, 32, 32, 3, dtype=torch.uint8))
        with pytest.raises(MaedHipError, match="positive"):
            render_batch(None, torch.from_numpy(v)[None], torch.tensor([[1.0, 1.0, 0.0, 0.0]]), f, resolution=(0, 32))
        with pytest.raises(MaedHipError, match="too large"):
            ops.render_mesh(torch.from_numpy(v)[None].contiguous(), ft, fl.faces, off, idx, torch.tensor([[1.0, 1.0, 0.0, 0.0]]), 1, 16385,
                            face_id=torch.zeros(1, 1, 16385, dtype=torch.int32))


def test_renderer_round_trips_numpy_in_the_reference_s_call_shape():
    from maed_amd.render import Renderer, rotation_matrix
    s = K.scene("torus_odd")
    v, f, H, W = s["verts"][0], s["faces"], s["H"], s["W"]
    img = s["frames"][0]
    with S.patched():
        r = Renderer(resolution=(W, H), faces=f, orig_img=True, wireframe=False, device="cpu")
        out = r.render(img, v, cam=s["cams"][0], color=[0.7, 0.9, 1.0])
        side = r.render(np.zeros_like(img), v, cam=s["cams"][0], angle=270, axis=[0, 1, 0], color=[0.7, 0.9, 1.0])
        wire = Renderer(resolution=(W, H), faces=f, wireframe=True, device="cpu").render(img, v, cam=s["cams"][0])
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == img.shape
    ref = R.render_ref(v, f, s["cams"][0], H, W, None, (0.7, 0.9, 1.0), img)
    assert np.array_equal((out != img).any(-1) | ref["covered"], ref["covered"]) and np.abs(out.astype(int) - ref["rgb"].astype(int)).max() <= 1
    ref_side = R.render_ref(v, f, s["cams"][0], H, W, rotation_matrix(270, [0, 1, 0]), (0.7, 0.9, 1.0), None)
    assert np.array_equal(side.any(-1), ref_side["covered"])
    assert 0 < (wire != img).any(-1).sum() < ref["covered"].sum()


def test_render_batch_takes_model_shaped_output_and_three_entry_cameras():
    from maed_amd.render import FaceList, render_batch
    v, f = R.smpl_sized()
    N, T = 2, 3
    g = torch.Generator().manual_seed(0)
    verts = torch.from_numpy(v)[None, None].repeat(N, T, 1, 1) + 0.01 * torch.randn(N, T, 1, 3, generator=g)
    cams = torch.tensor([0.9, 0.0, 0.0]).repeat(N, T, 1)
    frames = torch.randint(0, 256, (N, T, 96, 96, 3), dtype=torch.uint8, generator=g)
    fl = FaceList(f, 6890)
    with S.patched():
        fid = torch.empty(N * T, 96, 96, dtype=torch.int32)
        out = render_batch(frames, verts, cams, fl, face_id=fid)
        again = render_batch(frames.clone(), verts, cams, fl, out=None)
    assert out.shape == frames.shape and out.dtype == torch.uint8 and torch.equal(out, again)
    cov = (fid >= 0).reshape(N, T, 96, 96)
    assert cov.any() and torch.equal(out[~cov], frames[~cov])
    ref = R.render_ref(verts[1, 2].numpy(), f, np.array([0.9, 0.9, 0.0, 0.0]), 96, 96, None, frame=frames[1, 2].numpy())
    assert np.array_equal(cov[1, 2].numpy(), ref["covered"])
