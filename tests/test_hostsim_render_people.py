"""Many meshes per frame in one pass (maed_render_people, maed_amd.render.render_people / render_frame_results / Renderer.render_people) on the host simulator.
The cases and the oracle are in tests/_render_people_cases.py: every mesh alone through the single-mesh path, combined per pixel in numpy; all comparisons bit-equal."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import _hostsim_render as S
import _render_people_cases as P

ERR_ARG, ERR_UNSUPPORTED = -1, -5
WIREFRAME, SHARED_DEPTH = 1, 4


@pytest.fixture(scope="module")
def lib():
    from maed_amd import _lib as L
    h = S.load()
    for name in ("maed_render_people", "maed_render_people_workspace"):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    return h


@pytest.fixture()
def sim(lib):
    with S.patched():
        yield "cpu"


@pytest.mark.parametrize("frames", [True, False], ids=["over_frames", "on_black"])
def test_painter_equals_the_sequential_loop(sim, frames):
    P.case_painter(sim, frames)


def test_shared_depth_is_the_argmin_over_people(sim):
    P.case_shared_depth(sim)


def test_ties_and_interpenetration(sim):
    P.case_ties(sim)


def test_mesh_index_travels_through_the_large_triangle_queue(sim):
    P.case_queue(sim)


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------------
GUARD, POISON = 4096, 0xA5


class Guarded:
    """a buffer between two poisoned zones"""

    def __init__(self, nbytes, align=16):
        self.raw = np.full(nbytes + 2 * GUARD + align, POISON, dtype=np.uint8)
        self.at = GUARD + (-(self.raw.ctypes.data + GUARD)) % align
        self.n = nbytes

    @property
    def ptr(self):
        return self.raw.ctypes.data + self.at

    def view(self, dtype, shape):
        return self.raw[self.at:self.at + self.n].view(dtype).reshape(shape)

    def intact(self):
        return bool((self.raw[:self.at] == POISON).all() and (self.raw[self.at + self.n:] == POISON).all())


def call(lib, s, mesh_frame=None, flags=0, zoff=None, frames="scene", M=None):
    """maed_render_people itself on a scene dict -> (status, outputs as numpy, the guarded buffers)"""
    from maed_amd.render import FaceList
    M = len(s["verts"]) if M is None else M
    V, nf, B, H, W = s["verts"].shape[1], len(s["faces"]), s["B"], s["H"], s["W"]
    fl = FaceList(s["faces"], V)
    mf = np.ascontiguousarray(s["frame_index"] if mesh_frame is None else mesh_frame, dtype=np.int32)
    fr = s["frames"] if isinstance(frames, str) else frames
    need = lib.maed_render_people_workspace(M, B, V, nf, H, W, flags)
    g = dict(out=Guarded(B * H * W * 3), mesh_id=Guarded(B * H * W * 4), face_id=Guarded(B * H * W * 4), depth=Guarded(B * H * W * 4), ws=Guarded(need))
    p = lambda a: None if a is None else a.ctypes.data
    keep = [np.ascontiguousarray(a) if a is not None else None for a in (s["verts"], s["faces"], fl.vf_off, fl.vf_idx, s["cams"], s["rots"], s["colours"], zoff, fr)]
    verts, faces, off, idx, cams, rots, col, zo, fr = keep
    rc = lib.maed_render_people(p(verts), p(faces), p(faces), p(off), p(idx), p(cams), p(rots), p(col), p(zo), p(mf), p(fr), g["out"].ptr, g["mesh_id"].ptr,
                                g["face_id"].ptr, g["depth"].ptr, M, B, V, nf, H, W, flags, g["ws"].ptr, need, None)
    res = dict(out=g["out"].view(np.uint8, (B, H, W, 3)), mesh_id=g["mesh_id"].view(np.int32, (B, H, W)), face_id=g["face_id"].view(np.int32, (B, H, W)),
               depth=g["depth"].view(np.float32, (B, H, W)))
    return rc, res, g


def test_c_entry_point_equals_the_python_call_and_stays_inside_its_buffers(lib, sim):
    s = P.crowd()
    for flags, mode, zoff in ((0, "painter", None), (SHARED_DEPTH, "depth", s["zoff"])):
        rc, res, g = call(lib, s, flags=flags, zoff=zoff)
        assert rc == 0, lib.maed_last_error().decode()
        P.assert_same(res, P.people(s, sim, mode=mode), mode)
        assert all(b.intact() for b in g.values()), {k: b.intact() for k, b in g.items()}
    rc, res, g = call(lib, P.queued())                                # (the queue, and a second table chunk is not needed: B + 1 + M = 4 entries)
    assert rc == 0 and all(b.intact() for b in g.values())


def test_many_frames_use_more_than_one_table_chunk(lib, sim):
    """B + 1 + M above 512 table entries: the table travels in several launches.  600 frames of 5 x 4 pixels, a mesh in every 7th."""
    s = P.twins()
    B = 600
    fidx = np.arange(0, B, 7)
    M = len(fidx)
    big = dict(s, verts=np.repeat(s["verts"][:1], M, 0), cams=np.repeat(s["cams"][:1], M, 0), rots=np.repeat(s["rots"][:1], M, 0), colours=np.repeat(s["colours"][:1], M, 0),
               frame_index=fidx, B=B, H=4, W=5, frames=np.random.default_rng(5).integers(0, 256, size=(B, 4, 5, 3), dtype=np.uint8), zoff=np.zeros(M, dtype=np.float32))
    rc, res, g = call(lib, big)
    assert rc == 0 and all(b.intact() for b in g.values())
    alone = P.singles(dict(big, verts=big["verts"][:1]), sim)[0]
    want = np.full((B, 4, 5), -1, dtype=np.int32)
    want[fidx] = np.where(alone["face_id"] >= 0, np.arange(M)[:, None, None], -1)
    assert (alone["face_id"] >= 0).any() and np.array_equal(res["mesh_id"], want)
    assert np.array_equal(res["out"][np.setdiff1d(np.arange(B), fidx)], big["frames"][np.setdiff1d(np.arange(B), fidx)])


def test_refusals_of_the_c_entry_point(lib):
    s = P.crowd()
    msg = lambda: lib.maed_last_error().decode()
    rc, res, g = call(lib, s, mesh_frame=[1, 2, 1, 2])
    assert rc == ERR_ARG and "decrease" in msg(), msg()
    assert all((b.raw == POISON).all() for b in g.values()), "nothing may be written before the refusal"
    for bad in ([1, 2, 2, 3], [-1, 2, 2, 2]):
        rc, _, g = call(lib, s, mesh_frame=bad)
        assert rc == ERR_ARG and "outside [0, 3)" in msg(), msg()
        assert all((b.raw == POISON).all() for b in g.values())
    rc, _, _ = call(lib, s, zoff=s["zoff"])
    assert rc == ERR_ARG and "SHARED_DEPTH" in msg(), msg()
    rc, _, g = call(lib, s, flags=WIREFRAME)
    assert rc == ERR_UNSUPPORTED and "wireframe" in msg(), msg()
    assert all((b.raw == POISON).all() for b in g.values())
    # 256 meshes in one frame: the arrays are never read (the count is checked first), so one mesh's worth of data stands in for them
    many = dict(s, frame_index=np.ones(256, dtype=np.int32))
    rc, _, g = call(lib, many, M=256)
    assert rc == ERR_ARG and "255" in msg(), msg()
    assert all((b.raw == POISON).all() for b in g.values())
    rc, _, _ = call(lib, dict(s, W=16385), frames=None, M=0)
    assert rc == ERR_ARG and "16384" in msg(), msg()


def test_no_mesh_copies_the_frames(lib, sim):
    from maed_amd.render import render_people
    s = P.crowd()
    rc, res, g = call(lib, s, M=0)
    assert rc == 0, lib.maed_last_error().decode()
    assert np.array_equal(res["out"], s["frames"]) and (res["mesh_id"] == -1).all() and (res["face_id"] == -1).all() and np.isposinf(res["depth"]).all()
    assert all(b.intact() for b in g.values())
    rc, res, _ = call(lib, s, M=0, frames=None)
    assert rc == 0 and not res["out"].any()
    out = render_people(torch.from_numpy(s["frames"]), torch.zeros(0, s["verts"].shape[1], 3), torch.zeros(0, 4), [], s["faces"])
    assert np.array_equal(out.numpy(), s["frames"])


def test_unsorted_frame_index_equals_the_sorted_call(sim):
    s = P.crowd()
    order = [2, 0, 3, 1]                                            # frames 2, 1, 2, 2: meshes 2, 3, 1 of frame 2 in that painter order
    resorted = [1, 0, 2, 3]                                         # what the stable sort makes of it, as indices into `order`: frame 1 first, then frame 2 as given
    sorted_scene = {k: (v[[order[i] for i in resorted]] if k in ("verts", "cams", "rots", "colours", "zoff", "frame_index") else v) for k, v in s.items()}
    for mode in ("painter", "depth"):
        got, want = P.people(s, sim, mode=mode, order=order), P.people(sorted_scene, sim, mode=mode)
        for k in ("out", "face_id", "depth"):
            assert np.array_equal(P.bits(got[k]), P.bits(want[k])), (mode, k)
        # mesh_id counts in the arrays AS GIVEN: position i of the sorted call is position resorted[i] of the unsorted one
        assert np.array_equal(got["mesh_id"], np.where(want["mesh_id"] >= 0, np.asarray(resorted)[np.maximum(want["mesh_id"], 0)], -1)), mode
    assert set(np.unique(got["mesh_id"])) == {-1, 0, 1, 2, 3}


def test_wireframe_falls_back_to_the_sequential_loop(sim):
    s = P.crowd()
    got = P.people(s, sim, wireframe=True, ids=False)
    want = P.chain(s, sim, s["frames"], wireframe=True)
    solid = P.people(s, sim, ids=False)
    assert np.array_equal(got["out"], want) and (got["out"] != solid["out"]).any()
    from maed_amd._lib import MaedHipError
    with pytest.raises(MaedHipError, match="painter mode only"):
        P.people(s, sim, wireframe=True, mode="depth", ids=False)


def test_python_side_refusals(sim):
    from maed_amd._lib import MaedHipError
    from maed_amd.render import render_people
    s = P.crowd()
    v, c = torch.from_numpy(s["verts"]), torch.from_numpy(s["cams"])
    with pytest.raises(MaedHipError, match="z_offset needs mode='depth'"):
        render_people(None, v, c, [0, 0, 0, 0], s["faces"], z_offset=[0.0] * 4, resolution=(8, 8))
    with pytest.raises(MaedHipError, match="outside"):
        render_people(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), v, c, [0, 1, 2, 0], s["faces"])
    with pytest.raises(MaedHipError, match="one integer per mesh"):
        render_people(None, v, c, [0, 1], s["faces"], resolution=(8, 8))
    with pytest.raises(MaedHipError, match="255"):
        render_people(None, v[:1].expand(256, -1, -1).contiguous(), c[:1].expand(256, -1), [0] * 256, s["faces"], resolution=(8, 8))
    with pytest.raises(MaedHipError, match="mode must be"):
        render_people(None, v, c, [0, 0, 0, 0], s["faces"], mode="nearest", resolution=(8, 8))


# ---- host API ------------------------------------------------------------------------------------------------------------------------------------
def test_renderer_render_people_equals_the_loop_over_render(sim):
    from maed_amd.render import Renderer
    s = P.crowd()
    H, W = s["H"], s["W"]
    ms = [1, 2, 3]                                                  # the three people of frame 2
    people = OrderedDict((f"person{m}", {"verts": s["verts"][m], "cam": s["cams"][m]}) for m in ms)
    colours = {f"person{m}": s["colours"][m] for m in ms[:2]}       # (the third gets the default colour)
    r = Renderer(resolution=(W, H), faces=s["faces"], orig_img=True, device=sim)
    img = s["frames"][2]
    want = img
    for person, rec in people.items():                              # INTEGRATION.md section 2b, the host loop
        want = r.render(want, rec["verts"], cam=rec["cam"], color=colours.get(person, (1.0, 1.0, 0.9)))
    got = r.render_people(img, people, colours)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want) and (got != img).any()
    assert np.array_equal(r.render_people(img, OrderedDict()), img)
    nearest = r.render_people(img, people, colours, mode="depth")
    assert nearest.shape == got.shape and (nearest != got).any()
    wire = Renderer(resolution=(W, H), faces=s["faces"], wireframe=True, device=sim)
    want = img
    for person, rec in people.items():
        want = wire.render(want, rec["verts"], cam=rec["cam"], color=colours.get(person, (1.0, 1.0, 0.9)))
    assert np.array_equal(wire.render_people(img, people, colours), want)


def test_render_frame_results_on_the_recorded_people(sim, golden):
    P.case_frame_results(sim, golden)
