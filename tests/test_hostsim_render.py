"""csrc/render.hip on the host simulator (tests/_hostsim_render.py builds it alone), against the numpy restatement tests/_render_ref.py on the procedural scenes of
tests/_render_cases.py.

Bounds (docs/design/11_render.md): coverage equals the restatement's exactly (float32 projection / snap, int64 edges, top-left rule and the float32 clip depth are
mirrored operation by operation).  The largest |depth_kernel - depth_fp64| measured on this simulator over all scenes is 2.007e-7 (DEPTH_ERR = 2.01e-7); a pixel
whose two nearest fp64 candidates are closer than DELTA = 4 x that = 8.04e-7 is a tie pixel, excluded from the face / depth / colour comparison, and at most 0.1 % of
a scene's covered pixels may be excluded (the scenes have none).  The float32 wireframe distance is off by at most 1.018e-7 px where the distance is below 1 px
(WIRE_ERR = 1.02e-7); pixels within 4 x that of the 0.5 px threshold are excluded under the same cap.  Colour: at most one level per channel from the fp64 shading."""
import numpy as np
import pytest

import _hostsim_render as S
import _render_cases as K
import _render_ref as R

LANE, SPLIT = 1, 2


@pytest.mark.parametrize("name", list(K.SCENES))
def test_scene_against_the_restatement(name):
    s = K.scene(name)
    got = S.run(s)
    wire = S.run(s, wireframe=True, want=("out",))["out"]
    st = K.compare(name, got, wire)
    print(st)
    K.assert_stats(st)


@pytest.mark.parametrize("name", list(K.SCENES))
def test_oracle_alone_meets_the_exclusion_cap(name):
    st = K.oracle_stats(name)
    print(name, st)
    assert st["covered"] > 0
    assert st["tie"] <= K.MAX_EXCLUDED * st["covered"] and st["near"] <= K.MAX_EXCLUDED * st["covered"], st


def test_measured_bounds():
    """the two measured figures behind DELTA and WIRE_DELTA, measured again: the depth error from the kernel's own output, the wireframe distance error from the float32
    restatement of the kernel's formula -- which is tied to the kernel by requiring that it reproduces the kernel's drawn mask exactly"""
    worst_d = worst_w = 0.0
    for name in K.SCENES:
        s, ref = K.scene(name), K.reference(name)
        got = S.run(s, want=("out", "face_id", "depth"))
        wire = S.run(s, wireframe=True, want=("out",))["out"]
        same = ref["covered"] & (got["face_id"] == ref["face_id"])
        worst_d = max(worst_d, float(np.abs(got["depth"].astype(np.float64) - ref["depth"])[same].max()))
        m = ref["covered"] & (ref["wire_dist"] < 1.0)
        worst_w = max(worst_w, float(np.abs(ref["wire_dist32"].astype(np.float64) - ref["wire_dist"])[m].max()))
        drawn_mirror = ref["wire_dist32"] <= np.float32(0.5)
        want = np.where(drawn_mirror[..., None], got["out"], s["frames"])
        assert np.array_equal(wire[same], want[same]), name
    print(f"largest depth error {worst_d:.4e} (DEPTH_ERR {K.DEPTH_ERR:.3e}); largest float32 wireframe distance error {worst_w:.4e} (WIRE_ERR {K.WIRE_ERR:.3e})")
    assert worst_d <= K.DEPTH_ERR and worst_w <= K.WIRE_ERR
    assert K.DELTA == 4 * K.DEPTH_ERR and K.WIRE_DELTA == 4 * K.WIRE_ERR


@pytest.mark.parametrize("name", ["large_triangles", "smpl_b16_224", "borders", "torus_odd"])
def test_forms_and_runs_are_bit_equal(name):
    s = K.scene(name)
    a, b, c = S.run(s, form=SPLIT), S.run(s, form=SPLIT), S.run(s, form=LANE)
    auto = S.run(s, form=0)
    for k in ("out", "face_id", "depth"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (name, k, "two runs")
        assert np.array_equal(a[k].view(np.uint8), c[k].view(np.uint8)), (name, k, "lane form vs split form")
        assert np.array_equal(a[k].view(np.uint8), auto[k].view(np.uint8)), (name, k, "automatic form")


@pytest.mark.parametrize("name", ["torus_odd", "two_spheres", "ico_b16_224"])
def test_face_permutation_only_renames(name):
    s = K.scene(name)
    perm = np.random.default_rng(11).permutation(len(s["faces"]))
    p = dict(s, faces=np.ascontiguousarray(s["faces"][perm]))
    a, b = S.run(s), S.run(p)
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
    a, b, c = S.run(s), S.run(s), S.run(s, form=LANE)
    assert np.array_equal(a["face_id"] >= 0, ref["covered"])
    for k in ("out", "face_id", "depth"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) and np.array_equal(a[k].view(np.uint8), c[k].view(np.uint8)), k


def test_shared_edges_belong_to_exactly_one_triangle():
    """a fan of triangles around a vertex that lies exactly on a pixel centre, edges through pixel centres: with depth disabled as a tie-breaker (all z equal) every
    pixel of the union is covered, and the restatement agrees face by face (lower index wins an exact depth tie, so ownership shows in face_id)"""
    c = np.array([0.0, 0.0, 0.0])
    ring = [np.array([np.cos(a), np.sin(a), 0.0]) * 0.75 for a in np.linspace(0, 2 * np.pi, 9)[:-1]]
    v = np.array([c] + ring, dtype=np.float32)
    f = np.array([[0, 1 + k, 1 + (k + 1) % 8] for k in range(8)], dtype=np.int32)
    cam = np.array([1.0, 1.0, 0.0, 0.0], dtype=np.float32)
    f = K._front(v, f, cam, 64, 64)
    s = K._scene(v, f, [cam], 64, 64)
    got = S.run(s)
    ref = R.render_ref_batch(s["verts"], s["faces"], s["cams"], 64, 64, None, frames=s["frames"])
    assert np.array_equal(got["face_id"], ref["face_id"])
    # single ownership: drawing each triangle alone covers disjoint sets whose union is the fan
    total = np.zeros((1, 64, 64), dtype=np.int32)
    for k in range(8):
        total += S.run(dict(s, faces=np.ascontiguousarray(f[k:k + 1])), want=("face_id",))["face_id"] >= 0
    assert total.max() == 1 and np.array_equal(total == 1, got["face_id"] >= 0)


def test_no_frame_means_black_and_in_place_composite():
    s = K.scene("two_spheres")
    black = S.run(s, frames=None)
    over = S.run(s)
    cov = over["face_id"] >= 0
    assert (black["out"][~cov] == 0).all() and np.array_equal(black["out"][cov], over["out"][cov])


def test_non_finite_and_far_vertices_remove_or_clamp():
    s = K.scene("ico_224")
    v = s["verts"].copy()
    v[0, 5] = np.nan
    v[0, 9, 0] = np.inf
    v[0, 20] = [3e30, -3e30, 0.0]
    bad = dict(s, verts=v)
    got = S.run(bad)
    ref = R.render_ref_batch(v, s["faces"], s["cams"], s["H"], s["W"], None, frames=s["frames"])
    assert np.array_equal(got["face_id"], ref["face_id"])
    touched = np.isin(s["faces"], [5, 9]).any(1)
    assert not np.isin(got["face_id"], np.nonzero(touched)[0]).any()


def test_refusals():
    s = K.scene("two_spheres")
    f = s["faces"].copy()
    f[7, 1] = s["verts"].shape[1]
    with pytest.raises(RuntimeError, match="outside"):
        S.run(dict(s, faces=f))
    f[7, 1] = -1
    with pytest.raises(RuntimeError, match="outside"):
        S.run(dict(s, faces=f))
    with pytest.raises(RuntimeError, match="positive"):
        S.run(dict(s, H=0, frames=np.zeros((1, 0, 224, 3), dtype=np.uint8)), frames=None)
    with pytest.raises(RuntimeError, match="too large"):
        S.load()      # (the size check comes before any pointer is read: no 16385-wide buffers are made)
        S.run(dict(s, W=16385), frames=None, want=())
    # without the host copy the kernels' own range check keeps a bad face out: nothing is gathered through it, the other faces are drawn as before
    f[7, 1] = 1 << 30
    got = S.run(dict(s, faces=f), faces_host=False)
    good = S.run(dict(s, faces=np.delete(s["faces"], 7, axis=0)))
    assert np.array_equal(got["face_id"] >= 0, good["face_id"] >= 0) and not (got["face_id"] == 7).any()
