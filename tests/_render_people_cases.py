"""TEST INFRASTRUCTURE: many meshes per frame (maed_amd.render.render_people), shared by the simulator tests (tests/test_hostsim_render_people.py, device "cpu" inside
_hostsim_render.patched()) and the GPU tests (tests/test_gpu_render_people.py, device "cuda").  Scenes come from the procedural builders of tests/_render_cases.py;
every mesh has its own camera and shift, so the meshes of a frame overlap partly.

The oracle is the single-mesh path, which tests/test_hostsim_render.py / tests/test_gpu_render.py pin against the numpy restatement: every mesh is drawn ALONE with
render_batch on black with face_id and depth, and the meshes are combined per pixel in numpy.  Every comparison is bit-equal (uint8 colours, int32 ids, fp32 depth by
bit pattern): the one-pass kernels run the same integer coverage and the same fp32 operations in the same order, and only the 64-bit key differs."""
import collections

import numpy as np
import torch

import _render_cases as K
import _render_ref as R

F = np.float32


def _rot(angle, axis):
    from maed_amd.render import rotation_matrix
    return rotation_matrix(angle, axis).astype(F)


def crowd():
    """B = 3 frames with 0, 1 and 3 meshes (an empty frame, a single layer, layer 2) at 61 x 37: B H W = 6771 = 3 mod 4, so the resolve pass's bytewise tail runs.
    One mesh of each frame has its own colour."""
    H, W = 37, 61
    t = K.scene("torus_odd")
    v, f = t["verts"][0], t["faces"]
    shift = F([[0.0, 0.0, 0.0], [-0.25, 0.1, 0.2], [0.2, -0.05, -0.1], [0.0, 0.15, 0.05]])
    verts = np.stack([v + d for d in shift]).astype(F)
    centre = [(0.1, -0.1), (-0.35, 0.1), (0.3, 0.0), (0.0, 0.2)]
    cams = np.stack([R.fit_cam(v, H, W, h, centre=c) for h, c in zip((0.8, 0.7, 0.75, 0.5), centre)]).astype(F)
    rots = np.stack([_rot(55.0, [1.0, 0.3, 0.1]), _rot(20.0, [0.2, 1.0, 0.0]), _rot(-70.0, [1.0, 0.0, 0.4]), _rot(130.0, [0.3, 0.3, 1.0])])
    colours = F([[0.7, 0.9, 1.0], [1.0, 1.0, 0.9], [1.0, 0.6, 0.6], [1.0, 1.0, 0.9]])
    frames = np.random.default_rng(21).integers(0, 256, size=(3, H, W, 3), dtype=np.uint8)
    # each of the three meshes of frame 2 is pushed to the front of the others somewhere: offsets of the order of the meshes' depth extent
    zoff = F([0.0, 0.05, -0.1, 0.2])
    return dict(verts=verts, faces=f, cams=cams, rots=rots, colours=colours, frame_index=np.array([1, 2, 2, 2]), B=3, H=H, W=W, frames=frames, zoff=zoff)


def twins(zoff=(0.0, 0.0)):
    """the same mesh twice in one frame with the same camera: every covered pixel is an exact depth tie between the two"""
    H, W = 37, 61
    t = K.scene("torus_odd")
    v = t["verts"][0]
    cam = R.fit_cam(v, H, W, 0.8, centre=(0.05, -0.05)).astype(F)
    rot = _rot(55.0, [1.0, 0.3, 0.1])
    frames = np.random.default_rng(22).integers(0, 256, size=(1, H, W, 3), dtype=np.uint8)
    return dict(verts=np.stack([v, v]).astype(F), faces=t["faces"], cams=np.stack([cam, cam]), rots=np.stack([rot, rot]), colours=F([[0.7, 0.9, 1.0], [1.0, 0.6, 0.6]]),
                frame_index=np.array([0, 0]), B=1, H=H, W=W, frames=frames, zoff=F(zoff))


def queued():
    """the large_triangles scene (bounding boxes of millions of pixels: the split form sends them through the queue) as the FIRST of two meshes of a frame, at its own
    resolution; the second mesh is the same soup under a smaller camera shifted far to the side, so that its own large triangles cover part of the first one's"""
    s = K.scene("large_triangles")
    v = s["verts"][0]
    cam0 = s["cams"][0]
    cam1 = F([0.55 * cam0[0], 0.55 * cam0[1], 10.5, -0.3])      # (the quad's left edge, x = -9, lands at ndc_x = 0.42: its large triangles cover the right third)
    verts = np.stack([v, v + F([0.0, 0.0, -0.05])]).astype(F)
    return dict(verts=verts, faces=s["faces"], cams=np.stack([cam0, cam1]).astype(F), rots=None, colours=F([[1.0, 1.0, 0.9], [0.6, 1.0, 0.6]]), frame_index=np.array([0, 0]),
                B=1, H=s["H"], W=s["W"], frames=s["frames"], zoff=F([0.0, 0.0]))


def on(dev, a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype=dtype))).to(dev)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def singles(s, dev):
    """every mesh alone, on black, through the single-mesh path: list of dict(out, face_id, depth) as numpy (H, W[, 3])"""
    from maed_amd.render import FaceList, render_batch
    fl = FaceList(s["faces"], s["verts"].shape[1])
    H, W = s["H"], s["W"]
    res = []
    for m in range(len(s["verts"])):
        fid = torch.full((1, H, W), -7, dtype=torch.int32, device=dev)
        dep = torch.full((1, H, W), float("nan"), dtype=torch.float32, device=dev)
        out = render_batch(None, on(dev, s["verts"][m:m + 1]), on(dev, s["cams"][m:m + 1]), fl, rot=None if s["rots"] is None else on(dev, s["rots"][m:m + 1]),
                           color=tuple(float(x) for x in s["colours"][m]), resolution=(W, H), face_id=fid, depth=dep)
        res.append(dict(out=out[0].cpu().numpy(), face_id=fid[0].cpu().numpy(), depth=dep[0].cpu().numpy()))
    return res


def chain(s, dev, frames, wireframe=False):
    """the parent's way: the meshes in array order (= layer by layer in every frame), each drawn by render_batch over the previous result, in place"""
    from maed_amd.render import FaceList, render_batch
    fl = FaceList(s["faces"], s["verts"].shape[1])
    H, W = s["H"], s["W"]
    # (one tensor per frame: a frame of an odd size inside a batch is not 4-byte aligned, which the single-mesh entry point asks of its frames)
    cur = [torch.zeros((1, H, W, 3), dtype=torch.uint8, device=dev) if frames is None else on(dev, frames[b:b + 1]).clone() for b in range(s["B"])]
    for m, b in enumerate(s["frame_index"]):
        render_batch(cur[b], on(dev, s["verts"][m:m + 1]), on(dev, s["cams"][m:m + 1]), fl, rot=None if s["rots"] is None else on(dev, s["rots"][m:m + 1]),
                     color=tuple(float(x) for x in s["colours"][m]), out=cur[b], wireframe=wireframe)
    return torch.cat(cur).cpu().numpy()


def people(s, dev, frames="scene", mode="painter", form=0, order=None, wireframe=False, ids=True):
    """render_people on the scene -> dict(out, mesh_id, face_id, depth) as numpy; order: a permutation the arrays are given in (frame_index goes with them)"""
    from maed_amd.render import FaceList, render_people
    fl = FaceList(s["faces"], s["verts"].shape[1])
    B, H, W = s["B"], s["H"], s["W"]
    sel = np.arange(len(s["verts"])) if order is None else np.asarray(order)
    fr = s["frames"] if isinstance(frames, str) else frames
    mid = torch.full((B, H, W), -7, dtype=torch.int32, device=dev) if ids else None
    fid = torch.full((B, H, W), -7, dtype=torch.int32, device=dev) if ids else None
    dep = torch.full((B, H, W), float("nan"), dtype=torch.float32, device=dev) if ids else None
    out = render_people(on(dev, fr), on(dev, s["verts"][sel]), on(dev, s["cams"][sel]), [int(x) for x in s["frame_index"][sel]], fl, colors=on(dev, s["colours"][sel]),
                        rot=None if s["rots"] is None else on(dev, s["rots"][sel]), mode=mode, z_offset=on(dev, s["zoff"][sel]) if mode == "depth" else None,
                        wireframe=wireframe, mesh_id=mid, face_id=fid, depth=dep, resolution=(W, H), form=form, n_frames=B)
    assert tuple(out.shape) == (B, H, W, 3) and out.dtype == torch.uint8
    g = lambda t: None if t is None else t.cpu().numpy()
    return dict(out=g(out), mesh_id=g(mid), face_id=g(fid), depth=g(dep))


def combine(s, alone, frames, mode):
    """the oracle: the single-mesh results combined per pixel.
    painter: the last mesh of the frame (array order = layer order) whose own face_id >= 0;  depth: the smallest float32(z_m + zoff_m) among the meshes whose own
    face_id >= 0, an exact tie to the lower layer (np.argmin returns the first).  Colour, face and (painter) depth are the winner's own."""
    B, H, W = s["B"], s["H"], s["W"]
    out = np.zeros((B, H, W, 3), dtype=np.uint8) if frames is None else frames.copy()
    mid = np.full((B, H, W), -1, dtype=np.int32)
    fid = np.full((B, H, W), -1, dtype=np.int32)
    dep = np.full((B, H, W), np.inf, dtype=F)
    for b in range(B):
        ms = [m for m, fb in enumerate(s["frame_index"]) if fb == b]
        if not ms:
            continue
        cov = np.stack([alone[m]["face_id"] >= 0 for m in ms])
        if mode == "painter":
            z = np.stack([alone[m]["depth"] for m in ms])
            win = len(ms) - 1 - np.argmax(cov[::-1], axis=0)
        else:
            z = np.stack([np.where(alone[m]["face_id"] >= 0, (alone[m]["depth"] + s["zoff"][m]).astype(F), F(np.inf)) for m in ms])
            win = np.argmin(z, axis=0)
        any_ = cov.any(0)
        pick = lambda key: np.take_along_axis(np.stack([alone[m][key] for m in ms]), win[None].reshape((1,) + win.shape + (1,) * (alone[ms[0]][key].ndim - 2)), 0)[0]
        mid[b] = np.where(any_, np.asarray(ms, dtype=np.int32)[win], -1)
        fid[b] = np.where(any_, pick("face_id"), -1)
        dep[b] = np.where(any_, np.take_along_axis(z, win[None], 0)[0], F(np.inf))
        out[b] = np.where(any_[..., None], pick("out"), out[b])
    return dict(out=out, mesh_id=mid, face_id=fid, depth=dep)


def assert_same(got, want, what=""):
    for k in ("out", "mesh_id", "face_id", "depth"):
        if got.get(k) is None:
            continue
        g, w = got[k], want[k]
        same = np.array_equal(bits(g), bits(w))
        assert same, (what, k, int((bits(g).reshape(g.shape + (-1,)) != bits(w).reshape(w.shape + (-1,))).any(-1).sum()), "elements differ")


# ---- the cases, run by both test files on their device --------------------------------------------------------------------------------------
def case_painter(dev, frames):
    s = crowd()
    fr = s["frames"] if frames else None
    alone = singles(s, dev)
    got = people(s, dev, frames=fr)
    want = combine(s, alone, fr, "painter")
    assert_same(got, want, "painter vs the combined single-mesh renders")
    assert np.array_equal(got["out"], chain(s, dev, fr)), "painter vs the chain of render_batch calls"
    assert np.array_equal(got["out"][0], fr[0] if frames else np.zeros_like(got["out"][0])) and (got["mesh_id"][0] == -1).all(), "the empty frame"
    assert set(np.unique(got["mesh_id"][1])) == {-1, 0} and set(np.unique(got["mesh_id"][2])) == {-1, 1, 2, 3}, "every layer shows somewhere"
    hidden = (alone[1]["face_id"] >= 0) & (got["mesh_id"][2] != 1)
    assert hidden.any(), "the layers overlap"


def case_shared_depth(dev):
    s = crowd()
    alone = singles(s, dev)
    want = combine(s, alone, s["frames"], "depth")
    hist = np.bincount(want["mesh_id"][want["mesh_id"] >= 0], minlength=4)
    assert (hist > 0).all(), f"the oracle must see every mesh in front somewhere, histogram {hist}"
    painter = combine(s, alone, s["frames"], "painter")
    assert (want["mesh_id"] != painter["mesh_id"]).any(), "depth order and painter order must differ on this scene"
    got = people(s, dev, mode="depth")
    assert_same(got, want, "shared depth vs the per-pixel argmin of the single-mesh depths")


def case_ties(dev):
    for zoff, winner in (((0.0, 0.0), 0), ((0.0, -2.0 ** -10), 1)):
        s = twins(zoff)
        alone = singles(s, dev)
        cov = alone[0]["face_id"] >= 0
        assert cov.any() and np.array_equal(cov, alone[1]["face_id"] >= 0)
        got = people(s, dev, mode="depth")
        assert np.array_equal(got["mesh_id"][0], np.where(cov, winner, -1)), (zoff, "depth mode")
        assert_same(got, combine(s, alone, s["frames"], "depth"), f"twins {zoff}")
    s = twins()
    alone = singles(s, dev)
    got = people(s, dev)
    assert np.array_equal(got["mesh_id"][0], np.where(alone[0]["face_id"] >= 0, 1, -1)), "painter: the second mesh"
    assert_same(got, combine(s, alone, s["frames"], "painter"), "twins, painter")


def case_queue(dev):
    s = queued()
    alone = singles(s, dev)
    big = np.isin(alone[0]["face_id"], (0, 1, 2))                 # the ground quad's two triangles and the large triangle: the queued ones
    for mode in ("painter", "depth"):
        want = combine(s, alone, s["frames"], mode)
        lane, split = people(s, dev, mode=mode, form=1), people(s, dev, mode=mode, form=2)
        assert_same(lane, split, f"lane form vs split form, {mode}")
        assert_same(split, want, f"split form vs the oracle, {mode}")
        inside = big & (want["mesh_id"][0] == 0)
        assert inside.sum() > 100000 and (split["mesh_id"][0][inside] == 0).all() and np.isin(split["face_id"][0][inside], (0, 1, 2)).all()
        assert (want["mesh_id"][0] == 1).sum() > 10000, "the second mesh covers part of the first"


def frame_results_of_the_fixture(golden):
    """the recorded people of tests/golden/g17_render_cam.npz (frame ids and cameras of the reference's demo functions) with procedural vertices in place of the
    licensed mesh: person p in frame k is the torus, shifted by a fixed amount per person and frame"""
    from maed_amd.render import prepare_rendering_results
    g = golden("g17_render_cam")
    v = K.scene("torus_odd")["verts"][0]
    results = collections.OrderedDict()
    for p in (int(x) for x in g["person_ids"]):
        ids = g[f"p{p}_frame_ids"]
        verts = np.stack([v + np.float32([0.01 * p, 0.02 * k, 0.03 * (p % 3)]) for k in ids]).astype(np.float32)
        results[p] = {"frame_ids": ids, "verts": verts, "orig_cam": g[f"p{p}_orig_cam"].astype(np.float32)}
    return prepare_rendering_results(results, int(g["nframes"])), int(g["nframes"])


def case_frame_results(dev, golden):
    from maed_amd.render import FaceList, render_frame_results, render_people
    res, n = frame_results_of_the_fixture(golden)
    assert [len(x) for x in res] == [1, 2, 3, 1, 3, 1]
    f = K.scene("torus_odd")["faces"]
    fl = FaceList(f, 512)
    H, W = 54, 96
    frames = torch.from_numpy(np.random.default_rng(23).integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)).to(dev)
    colours = {3: (0.7, 0.9, 1.0), 7: (1.0, 0.6, 0.6)}
    mid = torch.full((n, H, W), -7, dtype=torch.int32, device=dev)
    got = render_frame_results(frames, res, fl, colors=colours, mesh_id=mid)
    flat = [(i, p, rec) for i, people in enumerate(res) for p, rec in people.items()]
    verts = torch.from_numpy(np.stack([rec["verts"] for _, _, rec in flat])).to(dev)
    cams = torch.from_numpy(np.stack([rec["cam"] for _, _, rec in flat])).to(dev)
    cols = np.float32([colours.get(p, (1.0, 1.0, 0.9)) for _, p, _ in flat])
    mid2 = torch.full((n, H, W), -7, dtype=torch.int32, device=dev)
    want = render_people(frames, verts, cams, [i for i, _, _ in flat], fl, colors=cols, mesh_id=mid2)
    assert got.device == frames.device and got.data_ptr() != frames.data_ptr()
    assert torch.equal(got, want) and torch.equal(mid, mid2)
    seen = np.unique(mid.cpu().numpy())
    print("meshes of the fixture that show:", seen)
    assert len(seen) > 3 and not torch.equal(got, frames)
