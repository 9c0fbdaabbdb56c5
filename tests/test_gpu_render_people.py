"""Many meshes per frame in one pass (maed_render_people through maed_amd.render) on the MI355X: the cases of tests/_render_people_cases.py on the device -- every
mesh alone through the single-mesh path, combined per pixel in numpy, all comparisons bit-equal -- and one case at 1920 x 1080 with three SMPL-sized meshes on one
frame against the sequential device loop."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import _render_cases as K
import _render_people_cases as P
import _render_ref as R

pytestmark = [pytest.mark.gpu]
DEV = "cuda"


@pytest.mark.parametrize("frames", [True, False], ids=["over_frames", "on_black"])
def test_painter_equals_the_sequential_loop(frames):
    P.case_painter(DEV, frames)


def test_shared_depth_is_the_argmin_over_people():
    P.case_shared_depth(DEV)


def test_ties_and_interpenetration():
    P.case_ties(DEV)


def test_mesh_index_travels_through_the_large_triangle_queue():
    P.case_queue(DEV)


def test_renderer_render_people_equals_the_loop_over_render():
    from maed_amd.render import Renderer
    s = P.crowd()
    ms = [1, 2, 3]
    people = OrderedDict((f"person{m}", {"verts": s["verts"][m], "cam": s["cams"][m]}) for m in ms)
    colours = {f"person{m}": s["colours"][m] for m in ms[:2]}
    r = Renderer(resolution=(s["W"], s["H"]), faces=s["faces"], orig_img=True)
    img = s["frames"][2]
    want = img
    for person, rec in people.items():                              # INTEGRATION.md section 2b, the host loop
        want = r.render(want, rec["verts"], cam=rec["cam"], color=colours.get(person, (1.0, 1.0, 0.9)))
    got = r.render_people(img, people, colours)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want) and (got != img).any()


def test_render_frame_results_on_the_recorded_people(golden):
    P.case_frame_results(DEV, golden)


def test_three_smpl_sized_people_at_1080p_equal_the_sequential_device_loop():
    """three 6890-vertex meshes on one 1920 x 1080 frame (the smpl_1080 builder; each its own camera, partly overlapping): one pass against render_batch once per
    person in place, and the shared-depth pass against the combined single-mesh depths"""
    from maed_amd.render import FaceList, render_batch, render_people
    s = K.scene("smpl_1080")
    v, f, H, W = s["verts"][0], s["faces"], s["H"], s["W"]
    fl = FaceList(f, len(v))
    cams = np.stack([R.fit_cam(v, H, W, h, centre=c) for h, c in ((1 / 3, (0.2, -0.1)), (0.45, (0.28, -0.05)), (0.4, (0.1, 0.0)))]).astype(np.float32)
    verts = torch.from_numpy(np.stack([v, v + np.float32([0.0, 0.0, 0.1]), v + np.float32([0.0, 0.0, -0.1])])).cuda()
    colours = np.float32([[1.0, 1.0, 0.9], [0.7, 0.9, 1.0], [1.0, 0.6, 0.6]])
    frames = torch.from_numpy(s["frames"]).cuda()
    loop = frames.clone()
    fid = torch.empty((3, 1, H, W), dtype=torch.int32, device="cuda")
    dep = torch.empty((3, 1, H, W), dtype=torch.float32, device="cuda")
    for m in range(3):
        render_batch(loop, verts[m:m + 1], torch.from_numpy(cams[m:m + 1]).cuda(), fl, color=tuple(colours[m]), out=loop, face_id=fid[m], depth=dep[m])
    mid = torch.empty((1, H, W), dtype=torch.int32, device="cuda")
    got = render_people(frames, verts, torch.from_numpy(cams).cuda(), [0, 0, 0], fl, colors=colours, mesh_id=mid)
    assert torch.equal(got, loop)
    cov = fid[:, 0] >= 0
    last = torch.where(cov[2], 2, torch.where(cov[1], 1, torch.where(cov[0], 0, -1))).to(torch.int32)
    assert torch.equal(mid[0], last) and all(int((last == m).sum()) > 1000 for m in range(3)) and bool((cov.sum(0) > 1).any())
    dmid = torch.empty((1, H, W), dtype=torch.int32, device="cuda")
    ddep = torch.empty((1, H, W), dtype=torch.float32, device="cuda")
    render_people(frames, verts, torch.from_numpy(cams).cuda(), [0, 0, 0], fl, colors=colours, mode="depth", mesh_id=dmid, depth=ddep)
    z = torch.where(cov, dep[:, 0], torch.full_like(dep[:, 0], float("inf")))
    near, arg = z.min(0), z.argmin(0)
    assert torch.equal(ddep[0].view(torch.int32), near.values.view(torch.int32))
    untied = cov.any(0) & ((z == near.values).sum(0) == 1)              # (torch.argmin does not promise the first of equal minima)
    assert torch.equal(dmid[0][untied], arg[untied].to(torch.int32)) and bool((dmid[0][~cov.any(0)] == -1).all())
