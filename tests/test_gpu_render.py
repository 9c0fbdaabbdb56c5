"""csrc/render.hip on the MI355X through maed_amd.ops.render_mesh / maed_amd.render, against the numpy restatement tests/_render_ref.py on the procedural scenes of
tests/_render_cases.py (nothing is read from outside tests/).  The bounds are those of tests/test_hostsim_render.py, measured on the host simulator: coverage exact;
DEPTH_ERR = 2.01e-7 (measured 2.007e-7), tie pixels (two nearest fp64 candidates closer than 4 x that) excluded, at most 0.1 % of a scene's covered pixels; colour
within one level of the fp64 shading; wireframe mask equal outside 4 x 1.02e-7 px (measured 1.018e-7) of the 0.5 px threshold."""
import numpy as np
import pytest
import torch

import _render_cases as K
import _render_ref as R
from _util import note

pytestmark = [pytest.mark.gpu]
LANE, SPLIT = 1, 2


def run_gpu(s, frames="scene", wireframe=False, form=0, want=("out", "face_id", "depth")):
    from maed_amd import ops
    from maed_amd.render import FaceList
    B, V, H, W = s["verts"].shape[0], s["verts"].shape[1], s["H"], s["W"]
    fl = FaceList(s["faces"], V)
    f_t, off, idx = fl.on("cuda")
    cu = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    fr = s["frames"] if isinstance(frames, str) else frames
    out = torch.full((B, H, W, 3), 77, dtype=torch.uint8, device="cuda") if "out" in want else None
    fid = torch.full((B, H, W), -7, dtype=torch.int32, device="cuda") if "face_id" in want else None
    dep = torch.full((B, H, W), float("nan"), device="cuda") if "depth" in want else None
    ops.render_mesh(cu(s["verts"]), f_t, fl.faces, off, idx, cu(s["cams"]), H, W, frames=cu(fr), rot=cu(s.get("rots")), out=out, face_id=fid, depth=dep,
                    wireframe=wireframe, form=form)
    torch.cuda.synchronize()
    return {k: None if t is None else t.cpu().numpy() for k, t in (("out", out), ("face_id", fid), ("depth", dep))}


@pytest.mark.parametrize("name", list(K.SCENES))
def test_scene_against_the_restatement(name):
    s = K.scene(name)
    got = run_gpu(s)
    wire = run_gpu(s, wireframe=True, want=("out",))["out"]
    st = K.compare(name, got, wire)
    note(f"render {st}")
    K.assert_stats(st)


@pytest.mark.parametrize("name", ["large_triangles", "smpl_b16_224", "borders", "torus_odd", "smpl_1080"])
def test_forms_and_runs_are_bit_equal(name):
    s = K.scene(name)
    a, b, c, auto = run_gpu(s, form=SPLIT), run_gpu(s, form=SPLIT), run_gpu(s, form=LANE), run_gpu(s, form=0)
    for k in ("out", "face_id", "depth"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (name, k, "two runs")
        assert np.array_equal(a[k].view(np.uint8), c[k].view(np.uint8)), (name, k, "lane form vs split form")
        assert np.array_equal(a[k].view(np.uint8), auto[k].view(np.uint8)), (name, k, "automatic form")


@pytest.mark.parametrize("name", ["torus_odd", "two_spheres", "ico_b16_224"])
def test_face_permutation_only_renames(name):
    s = K.scene(name)
    perm = np.random.default_rng(11).permutation(len(s["faces"]))
    a, b = run_gpu(s), run_gpu(dict(s, faces=np.ascontiguousarray(s["faces"][perm])))
    cov = a["face_id"] >= 0
    assert np.array_equal(cov, b["face_id"] >= 0)
    renamed = np.where(b["face_id"] >= 0, perm[np.maximum(b["face_id"], 0)], -1)
    ref = K.reference(name)
    exact_tie = cov & (ref["second"] == ref["depth"])
    assert np.array_equal(renamed[~exact_tie], a["face_id"][~exact_tie])
    assert np.array_equal(a["depth"][~exact_tie].view(np.uint32), b["depth"][~exact_tie].view(np.uint32))


def test_interpenetrating_meshes_are_deterministic_and_covered_exactly():
    s = K.interpenetrating()
    ref = R.render_ref_batch(s["verts"], s["faces"], s["cams"], s["H"], s["W"], s["rots"], frames=s["frames"])
    a, b, c = run_gpu(s), run_gpu(s), run_gpu(s, form=LANE)
    assert np.array_equal(a["face_id"] >= 0, ref["covered"])
    for k in ("out", "face_id", "depth"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) and np.array_equal(a[k].view(np.uint8), c[k].view(np.uint8)), k


def test_no_frame_means_black_and_in_place_composite():
    from maed_amd.render import render_batch
    s = K.scene("two_spheres")
    black, over = run_gpu(s, frames=None), run_gpu(s)
    cov = over["face_id"] >= 0
    assert (black["out"][~cov] == 0).all() and np.array_equal(black["out"][cov], over["out"][cov])
    frames = torch.from_numpy(s["frames"]).cuda()
    same = render_batch(frames, torch.from_numpy(s["verts"]).cuda(), torch.from_numpy(s["cams"]).cuda(), s["faces"], out=frames)
    assert same.data_ptr() == frames.data_ptr() and np.array_equal(frames.cpu().numpy(), over["out"])


def test_renderer_round_trips_numpy_in_the_reference_s_call_shape():
    from maed_amd.render import Renderer
    s = K.scene("torus_odd")
    v, f, H, W, img = s["verts"][0], s["faces"], s["H"], s["W"], s["frames"][0]
    r = Renderer(resolution=(W, H), faces=f, orig_img=True, wireframe=False)
    out = r.render(img, v, cam=s["cams"][0], color=[0.7, 0.9, 1.0])
    side = r.render(np.zeros_like(img), v, cam=s["cams"][0], angle=270, axis=[0, 1, 0])
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == img.shape and side.shape == img.shape
    ref = R.render_ref(v, f, s["cams"][0], H, W, None, (0.7, 0.9, 1.0), img)
    assert np.array_equal(out[~ref["covered"]], img[~ref["covered"]]) and np.abs(out.astype(int) - ref["rgb"].astype(int)).max() <= 1
    # two people in one frame, the reference's loop: one after the other over the previous result
    img2 = r.render(out, v + np.float32([0.3, 0.1, -0.2]), cam=s["cams"][0], color=[1.0, 0.6, 0.6])
    ref2 = R.render_ref(v + np.float32([0.3, 0.1, -0.2]), f, s["cams"][0], H, W, None, (1.0, 0.6, 0.6), out)
    assert np.abs(img2.astype(int) - ref2["rgb"].astype(int)).max() <= 1 and np.array_equal(img2[~ref2["covered"]], out[~ref2["covered"]])


def test_render_batch_consumes_a_model_output_on_the_device_without_synchronising():
    import maed_amd
    from maed_amd.render import FaceList, render_batch
    m = maed_amd.MAED(num_blocks=2, num_heads=2, embed_dim=128, hidden_dim=64, img_size=64, compute_dtype=torch.float32).to("cuda").eval()
    clip = torch.randn(2, 4, 3, 64, 64, device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    with torch.no_grad():
        out = m(clip)
    verts = out["verts"]
    assert verts.is_cuda and verts.shape[-2:] == (6890, 3)
    verts = verts.reshape(2, 4, 6890, 3)
    _, f = R.smpl_sized()                                     # (a face list of SMPL's size over the stand-in's vertices: the synthetic model itself has none)
    fl = FaceList(f, 6890)
    frames = torch.randint(0, 256, (2, 4, 120, 160, 3), dtype=torch.uint8, device="cuda")
    cams = torch.tensor([0.8, 0.0, 0.0], device="cuda").repeat(2, 4, 1)
    fid = torch.empty(8, 120, 160, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # honours the current stream
        img = render_batch(frames, verts, cams, fl, face_id=fid)
    side.synchronize()
    assert img.shape == frames.shape and img.is_cuda and img.dtype == torch.uint8
    cov = (fid >= 0).reshape(2, 4, 120, 160)
    assert torch.equal(img[~cov], frames[~cov])
    ref = R.render_ref(verts[1, 3].cpu().numpy(), f, np.array([0.8, 0.8, 0.0, 0.0]), 120, 160, None, frame=frames[1, 3].cpu().numpy())
    assert np.array_equal(cov[1, 3].cpu().numpy(), ref["covered"])


def test_refusals():
    from maed_amd import ops
    from maed_amd._lib import MaedHipError
    from maed_amd.render import FaceList, Renderer, render_batch
    v, f = R.icosphere(1)
    fl = FaceList(f, len(v))
    ft, off, idx = fl.on("cuda")
    vt, cam = torch.from_numpy(v)[None].cuda(), torch.tensor([[1.0, 1.0, 0.0, 0.0]], device="cuda")
    bad = f.copy()
    bad[3, 2] = len(v)
    with pytest.raises(MaedHipError, match="outside"):
        ops.render_mesh(vt, torch.from_numpy(bad).cuda(), bad, off, idx, cam, 32, 32, out=torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(MaedHipError, match="positive"):
        render_batch(None, vt, cam, fl, resolution=(0, 32))
    with pytest.raises(MaedHipError, match="too large"):
        ops.render_mesh(vt, ft, fl.faces, off, idx, cam, 1, 16385, face_id=torch.zeros(1, 1, 16385, dtype=torch.int32, device="cuda"))
    with pytest.raises(MaedHipError, match="no faces"):
        Renderer(resolution=(64, 64))
    with pytest.raises(MaedHipError):                       # a CPU tensor is an error, never a fallback
        render_batch(None, torch.from_numpy(v)[None], cam.cpu(), fl, resolution=(32, 32))
