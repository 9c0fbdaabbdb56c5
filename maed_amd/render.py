"""Mesh overlays on the device: the reference's visualisation step (lib/utils/renderer.py Renderer, lib/utils/demo_utils.py convert_crop_cam_to_orig_img /
prepare_rendering_results) on csrc/render.hip.  The reference draws with pyrender on OpenGL; an Instinct accelerator has no graphics pipeline, so the mesh is
rasterised by compute kernels (docs/design/11_render.md: projection, fill rule and depth are pinned, the look of the shader is this project's own).

    r = Renderer(resolution=(w, h), faces=faces, orig_img=True)          # faces: (n, 3) vertex indices, or smpl_arrays['f'] of the licensed model
    img = r.render(img, verts, cam=orig_cam[i], color=colour)             # numpy in, numpy out: the loop of the reference's visualize.py runs on it unchanged
    out = render_batch(frames, out["verts"], cams, faces)                  # device tensors in, device tensor out, no host synchronisation
    out = render_frame_results(frames, prepare_rendering_results(results, n), faces)   # every person of every frame in ONE pass (render_people on flat arrays)
"""
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
from . import ops

DEFAULT_COLOR = (1.0, 1.0, 0.9)


class FaceList:
    """A triangle list shared by every mesh of a call: the int32 (n, 3) array, the vertex -> face CSR the vertex normals are gathered through (built once, on the
    host, faces of a vertex in ascending order = a deterministic sum), and their device copies per device."""

    def __init__(self, faces, n_verts):
        f = np.asarray(faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] == 0:
            raise L.MaedHipError(f"render: faces must be a non-empty (n, 3) array of vertex indices, got shape {f.shape}")
        if f.dtype.kind not in "iu":
            raise L.MaedHipError(f"render: faces must be integers, got {f.dtype}")
        self.n_verts = int(n_verts)
        if int(f.min()) < 0 or int(f.max()) >= self.n_verts:
            raise L.MaedHipError(f"render: a face refers to vertex {int(f.min()) if f.min() < 0 else int(f.max())}, outside [0, {self.n_verts})")
        self.faces = np.ascontiguousarray(f, dtype=np.int32)
        flat = self.faces.reshape(-1)
        order = np.argsort(flat, kind="stable")                  # (stable: the faces of a vertex stay in ascending order)
        self.vf_idx = (order // 3).astype(np.int32)
        self.vf_off = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=self.n_verts))]).astype(np.int32)
        self._dev = {}

    def __len__(self):
        return len(self.faces)

    def on(self, device):
        device = torch.device(device)
        key = (device.type, device.index)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(a).to(device) for a in (self.faces, self.vf_off, self.vf_idx))
        return self._dev[key]


def smpl_faces(smpl_arrays=None):
    """the face list of the licensed SMPL model (smpl_arrays['f'], the field the model file calls `f`).  The synthetic stand-in of maed_amd.smpl has vertices and
    blend weights but NO faces: there is nothing to draw triangles from."""
    if smpl_arrays is None or "f" not in smpl_arrays:
        raise L.MaedHipError("render: no face list.  The synthetic SMPL stand-in (maed_amd.smpl.synthetic_smpl_arrays) has no faces; pass faces=(n, 3) vertex indices, "
                             "or smpl_arrays= of the licensed model, whose field 'f' holds them.")
    return np.asarray(smpl_arrays["f"]).astype(np.int64)


def rotation_matrix(angle_deg, axis):
    """3 x 3 rotation by `angle_deg` degrees about `axis` (right-handed, axis normalised): what the reference applies to the mesh for its side views"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    t = math.radians(float(angle_deg))
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


def render_batch(frames, verts, cams, faces, rot=None, color=DEFAULT_COLOR, wireframe=False, wire_px=0.5, resolution=None, out=None, face_id=None, depth=None,
                 form=ops.RENDER_FORM_AUTO):
    """Draw one mesh per frame over a batch of frames, all on the device: no host synchronisation, launches go to the current stream.
    frames  uint8 (..., H, W, 3) device tensor, or None with resolution=(w, h) for a black background
    verts   fp32 (..., V, 3), e.g. MAED.forward's out['verts'] (N, T, 6890, 3); the leading dimensions are flattened and must match those of frames / cams
    cams    (..., 4) = sx, sy, tx, ty (convert_crop_cam_to_orig_img), or (..., 3) = s, tx, ty of the crop (drawn with sx = sy = s)
    faces   FaceList, or an (n, 3) index array (a FaceList is built: keep one when calling repeatedly)
    rot     (..., 3, 3) or (3, 3) rotation applied to the rotated mesh, or None
    out     uint8 tensor of the shape of frames (may be `frames` itself); face_id int32 / depth fp32 (B, H, W) are filled when given
    Returns out in the shape of frames."""
    V = int(verts.shape[-2])
    v = verts.reshape(-1, V, 3)
    B = int(v.shape[0])
    dev = v.device
    if frames is not None:
        H, W = int(frames.shape[-3]), int(frames.shape[-2])
        lead = tuple(frames.shape[:-3])
        fr = frames.reshape(B, H, W, 3)
        if fr.dtype != torch.uint8:
            raise L.MaedHipError(f"render_batch: frames must be uint8, got {fr.dtype}")
        fr = fr if fr.is_contiguous() else fr.contiguous()
    else:
        if resolution is None:
            raise L.MaedHipError("render_batch: give frames or resolution=(w, h)")
        W, H = int(resolution[0]), int(resolution[1])
        lead, fr = tuple(verts.shape[:-2]), None
    fl = faces if isinstance(faces, FaceList) else FaceList(faces, V)
    if fl.n_verts != V:
        raise L.MaedHipError(f"render_batch: the face list was built for {fl.n_verts} vertices, verts has {V}")
    f_t, off_t, idx_t = fl.on(dev)
    c = torch.as_tensor(cams, device=dev).reshape(B, -1).to(torch.float32)
    if c.shape[1] == 3:
        c = torch.stack([c[:, 0], c[:, 0], c[:, 1], c[:, 2]], dim=1)
    if c.shape[1] != 4:
        raise L.MaedHipError(f"render_batch: cams must have 4 (sx, sy, tx, ty) or 3 (s, tx, ty) entries per frame, got {c.shape[1]}")
    r = None
    if rot is not None:
        r = torch.as_tensor(rot, device=dev).to(torch.float32)
        r = (r.expand(B, 3, 3) if r.dim() == 2 else r.reshape(B, 3, 3)).contiguous()
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    o = out.reshape(B, H, W, 3)
    if not o.is_contiguous() or o.data_ptr() != out.data_ptr():
        raise L.MaedHipError("render_batch: out must be contiguous")
    ops.render_mesh(v.to(torch.float32).contiguous(), f_t, fl.faces, off_t, idx_t, c.contiguous(), H, W, frames=fr, rot=r, out=o, face_id=face_id, depth=depth,
                    base=color, wireframe=wireframe, wire_px=wire_px, form=form)
    return o.reshape(*lead, H, W, 3)


def _colour_rows(colors, M, dev):
    """(M, 3) fp32 on the device from None, one triple or one triple per mesh.  One triple is written by three fills (scalars travel as kernel arguments: no copy
    from the host, no synchronisation); a host array of M triples is one small host -> device copy; a device tensor is used as it is."""
    if isinstance(colors, torch.Tensor) and colors.dim() == 2:
        c = colors.to(device=dev, dtype=torch.float32)
    else:
        a = np.asarray(DEFAULT_COLOR if colors is None else colors.cpu() if isinstance(colors, torch.Tensor) else colors, dtype=np.float32)
        if a.shape == (3,):
            c = torch.empty((M, 3), dtype=torch.float32, device=dev)
            for k in range(3):
                c[:, k].fill_(float(a[k]))
            return c
        c = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if tuple(c.shape) != (M, 3):
        raise L.MaedHipError(f"render_people: colors must be one (r, g, b) or {M} of them, got shape {tuple(c.shape)}")
    return c.contiguous()


def render_people(frames, verts, cams, frame_index, faces, colors=None, rot=None, mode="painter", z_offset=None, wireframe=False, wire_px=0.5, out=None, mesh_id=None,
                  face_id=None, depth=None, resolution=None, form=ops.RENDER_FORM_AUTO, n_frames=None):
    """Draw every person of every frame in ONE pass on the device: M meshes into B frames, any number (up to 255) per frame, none included.
    frames       uint8 (..., H, W, 3) device tensor (the leading dimensions are flattened to B frames), or None with resolution=(w, h): n_frames black frames
                 (default: up to the largest value of frame_index)
    verts        fp32 (M, V, 3);  cams (M, 4) = sx, sy, tx, ty or (M, 3) = s, tx, ty, as render_batch takes them;  rot (M, 3, 3) or (3, 3) or None
    frame_index  (M) the frame of every mesh, in ANY order: a host list / array, or a tensor.  It is sorted stably by frame here, so the order in which the meshes of one
                 frame are given is their painter order (the later one is drawn over the earlier one).  The frame table is built on the host: a DEVICE tensor is read
                 back first, which waits for the stream -- the one host synchronisation of this function; keep frame_index on the host to avoid it.  When the meshes
                 are not already grouped by ascending frame, the arrays are gathered into that order on the device (the permutation is staged through pinned memory)
    colors       (M, 3), one (r, g, b), or None (= DEFAULT_COLOR)
    mode         "painter": the meshes of a frame in the given order, each over the previous ones -- bit for bit the result of calling render_batch once per mesh
                 "depth": one depth buffer per frame shared by its meshes, the nearest fragment wins; z_offset (M) is added to the ndc_z of a mesh (fp32) before the
                 comparison (a caller who knows how far apart the people stand -- e.g. from the camera scale, depth ~ 1 / s -- puts it there), None = 0.  An exact tie
                 goes to the mesh given first
    wireframe    the one-pass kernels do not draw wireframes (a pixel that fails the edge test shows the layer below, which one winner per pixel cannot express):
                 True draws with render_batch, one call per layer over the frames that have that layer, in place on the device; painter mode only, no id outputs
    out          uint8, the shape of frames (may be frames itself);  mesh_id int32 (B, H, W): index INTO THE GIVEN ARRAYS of the visible mesh, -1 where none;
                 face_id int32 / depth fp32 (B, H, W): its visible face and depth (ndc_z, in depth mode ndc_z + z_offset), as render_batch writes them
    Returns out in the shape of frames."""
    if mode not in ("painter", "depth"):
        raise L.MaedHipError(f"render_people: mode must be 'painter' or 'depth', got {mode!r}")
    if z_offset is not None and mode != "depth":
        raise L.MaedHipError("render_people: z_offset needs mode='depth' (the painter order does not compare depths between meshes)")
    if verts.dim() != 3 or verts.shape[-1] != 3:
        raise L.MaedHipError(f"render_people: verts must be (M, V, 3), got {tuple(verts.shape)}")
    M, V = int(verts.shape[0]), int(verts.shape[1])
    dev = verts.device
    fi = np.asarray(frame_index.cpu() if isinstance(frame_index, torch.Tensor) else frame_index).reshape(-1)
    if fi.shape[0] != M or (M and fi.dtype.kind not in "iu"):
        raise L.MaedHipError(f"render_people: frame_index must hold one integer per mesh ({M}), got {fi.shape[0]} of {fi.dtype}")
    fi = fi.astype(np.int64)
    if frames is not None:
        H, W = int(frames.shape[-3]), int(frames.shape[-2])
        lead = tuple(frames.shape[:-3])
        fr = frames.reshape(-1, H, W, 3)
        B = int(fr.shape[0])
        if fr.dtype != torch.uint8:
            raise L.MaedHipError(f"render_people: frames must be uint8, got {fr.dtype}")
        fr = fr if fr.is_contiguous() else fr.contiguous()
    else:
        if resolution is None:
            raise L.MaedHipError("render_people: give frames or resolution=(w, h)")
        W, H = int(resolution[0]), int(resolution[1])
        B = int(n_frames) if n_frames is not None else (int(fi.max()) + 1 if M else 1)
        lead, fr = (B,), None
    if M and (int(fi.min()) < 0 or int(fi.max()) >= B):
        raise L.MaedHipError(f"render_people: frame_index has a value outside [0, {B}) (the number of frames)")
    fl = faces if isinstance(faces, FaceList) else FaceList(faces, V)
    if fl.n_verts != V:
        raise L.MaedHipError(f"render_people: the face list was built for {fl.n_verts} vertices, verts has {V}")
    f_t, off_t, idx_t = fl.on(dev)
    v = verts.to(torch.float32)
    c = torch.as_tensor(cams, device=dev).reshape(M, -1).to(torch.float32) if M else torch.empty((0, 4), dtype=torch.float32, device=dev)
    if M and c.shape[1] == 3:
        c = torch.stack([c[:, 0], c[:, 0], c[:, 1], c[:, 2]], dim=1)
    if M and c.shape[1] != 4:
        raise L.MaedHipError(f"render_people: cams must have 4 (sx, sy, tx, ty) or 3 (s, tx, ty) entries per mesh, got {c.shape[1]}")
    c = c.reshape(M, 4)
    col = _colour_rows(colors, M, dev)
    r = None
    if rot is not None:
        r = torch.as_tensor(rot, device=dev).to(torch.float32)
        r = r.expand(M, 3, 3) if r.dim() == 2 else r.reshape(M, 3, 3)
    z = None if z_offset is None else torch.as_tensor(z_offset, device=dev).to(torch.float32).reshape(M)
    order = np.argsort(fi, kind="stable")                 # (stable: the given order within a frame is the painter order)
    perm = None
    if not np.array_equal(order, np.arange(M)):
        perm = ops._upload_table(order.astype(np.int64), dev).view(torch.int64)
        v, c, col = v.index_select(0, perm), c.index_select(0, perm), col.index_select(0, perm)
        r = None if r is None else r.index_select(0, perm)
        z = None if z is None else z.index_select(0, perm)
    mesh_frame = np.ascontiguousarray(fi[order], dtype=np.int32)
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    o = out.reshape(B, H, W, 3)
    if not o.is_contiguous() or o.data_ptr() != out.data_ptr():
        raise L.MaedHipError("render_people: out must be contiguous")
    v, c = v.contiguous(), c.contiguous()
    r = None if r is None else r.contiguous()
    if wireframe:
        if mode != "painter" or mesh_id is not None or face_id is not None or depth is not None:
            raise L.MaedHipError("render_people: wireframe=True draws layer by layer with render_batch: painter mode only, and no mesh_id / face_id / depth outputs")
        if fr is None:
            o.zero_()
        elif fr.data_ptr() != o.data_ptr():
            o.copy_(fr)
        layer = np.arange(M) - np.searchsorted(mesh_frame, mesh_frame, side="left")
        for k in range(int(layer.max()) + 1 if M else 0):
            sel = np.nonzero(layer == k)[0]
            ms = torch.from_numpy(sel).to(dev)
            args = dict(rot=None if r is None else r.index_select(0, ms), wireframe=True, wire_px=wire_px, form=form)
            if len(sel) == B:                             # (every frame has this layer: the frames of the layer are the batch itself)
                _render_layer(o, v.index_select(0, ms), c.index_select(0, ms), fl, col.index_select(0, ms), args)
            else:
                fs = torch.from_numpy(mesh_frame[sel].astype(np.int64)).to(dev)
                sub = o.index_select(0, fs)
                _render_layer(sub, v.index_select(0, ms), c.index_select(0, ms), fl, col.index_select(0, ms), args)
                o.index_copy_(0, fs, sub)
        return o.reshape(*lead, H, W, 3)
    ops.render_people(v, f_t, fl.faces, off_t, idx_t, c, col.contiguous(), mesh_frame, B, H, W, frames=fr, rot=r, zoff=None if z is None else z.contiguous(), out=o,
                      mesh_id=mesh_id, face_id=face_id, depth=depth, shared_depth=(mode == "depth"), form=form)
    if perm is not None and mesh_id is not None:          # the kernels number the meshes in the sorted order: back to the caller's
        mesh_id.copy_(torch.where(mesh_id >= 0, perm[mesh_id.clamp(min=0).long()], mesh_id.long()).to(torch.int32))
    return o.reshape(*lead, H, W, 3)


def _render_layer(frames, verts, cams, fl, colours, args):
    """one layer of the wireframe form: render_batch takes one base colour per call, so the meshes of the layer are drawn in groups of equal colour (the colours
    are read back for that: this form synchronises)"""
    host = colours.cpu().numpy()
    groups = {}
    for k, rgb in enumerate(map(tuple, host)):
        groups.setdefault(rgb, []).append(k)
    if len(groups) == 1:
        render_batch(frames, verts, cams, fl, color=host[0], out=frames, **args)
        return
    for rgb, ks in groups.items():
        idx = torch.tensor(ks, device=frames.device)
        sub = frames.index_select(0, idx)
        render_batch(sub, verts.index_select(0, idx), cams.index_select(0, idx), fl, color=rgb, out=sub,
                     **dict(args, rot=None if args["rot"] is None else args["rot"].index_select(0, idx)))
        frames.index_copy_(0, idx, sub)


def render_frame_results(frames, frame_results, faces, colors=None, **kw):
    """Draw what prepare_rendering_results returns: frame_results[i] is the OrderedDict person -> {'verts', 'cam'} of frame i, drawn in the dict's order (ascending
    camera scale: the largest last).  frames uint8 (B, H, W, 3) on the device with B = len(frame_results), or None with resolution=(w, h) and device=...; colors: an
    optional dict person -> (r, g, b) (people not in it get DEFAULT_COLOR); every other keyword goes to render_people.  Returns the device tensor."""
    dev = kw.pop("device", None)
    verts, cams, fidx, cols = [], [], [], []
    for i, people in enumerate(frame_results):
        for person, rec in people.items():
            verts.append(rec["verts"])
            cams.append(rec["cam"])
            fidx.append(i)
            cols.append(tuple(float(x) for x in (colors or {}).get(person, DEFAULT_COLOR)))
    if frames is not None:
        if int(np.prod(frames.shape[:-3])) != len(frame_results):
            raise L.MaedHipError(f"render_frame_results: {len(frame_results)} frames of results for frames of shape {tuple(frames.shape)}")
        dev = frames.device
    elif dev is None:
        dev = verts[0].device if verts and isinstance(verts[0], torch.Tensor) else torch.device("cuda")
    if not verts:
        fl = faces if isinstance(faces, FaceList) else None
        V = fl.n_verts if fl is not None else int(np.asarray(faces).max()) + 1
        v = torch.empty((0, V, 3), dtype=torch.float32, device=dev)
        c = torch.empty((0, 4), dtype=torch.float32, device=dev)
    elif isinstance(verts[0], torch.Tensor):
        v = torch.stack([x.to(dev) for x in verts])
        c = torch.stack([torch.as_tensor(x, device=dev).to(torch.float32) for x in cams])
    else:
        v = torch.from_numpy(np.stack([np.asarray(x, dtype=np.float32) for x in verts])).to(dev)
        c = torch.from_numpy(np.stack([np.asarray(x, dtype=np.float32) for x in cams])).to(dev)
    return render_people(frames, v, c, fidx, faces, colors=np.asarray(cols, dtype=np.float32).reshape(-1, 3) if cols else None, n_frames=len(frame_results), **kw)


class Renderer:
    """The reference's Renderer (lib/utils/renderer.py) on the device rasteriser: same constructor and `render` call shape, numpy in and numpy out.
    faces: (n, 3) vertex indices (required unless smpl_arrays of the licensed model is given); device: where the kernels run."""

    def __init__(self, resolution=(224, 224), orig_img=False, wireframe=False, faces=None, smpl_arrays=None, n_verts=None, device="cuda", wire_px=0.5):
        self.resolution = resolution
        self.faces = np.asarray(smpl_faces(smpl_arrays) if faces is None else faces)
        self.orig_img = orig_img
        self.wireframe = wireframe
        self.wire_px = wire_px
        self.device = torch.device(device)
        self.n_verts = n_verts
        self._fl = None

    def set_faces(self, indices):
        """keep the faces whose three vertices are all in `indices` (renderer.py:69-72)"""
        self.faces = self.faces[np.isin(self.faces, np.asarray(indices)).all(axis=1)]
        self._fl = None

    def _face_list(self, V):
        if self._fl is None or self._fl.n_verts != V:
            self._fl = FaceList(self.faces, V)
        return self._fl

    def render(self, img, verts, cam, angle=None, axis=None, mesh_filename=None, color=DEFAULT_COLOR):
        if mesh_filename is not None:
            raise NotImplementedError("Renderer.render: mesh export is not part of this port (docs/design/07_scope.md)")
        verts = np.array(verts, dtype=np.float32)
        W, H = int(self.resolution[0]), int(self.resolution[1])
        frame = None
        if img is not None:
            img = np.asarray(img)
            if img.shape != (H, W, 3):
                raise L.MaedHipError(f"Renderer.render: img has shape {img.shape}, the renderer was made for {(H, W, 3)}")
            frame = torch.from_numpy(np.ascontiguousarray(img.astype(np.uint8))).to(self.device)[None]
        rot = rotation_matrix(angle, axis) if (angle and axis) else None
        out = render_batch(frame, torch.from_numpy(verts).to(self.device)[None], torch.tensor([[float(x) for x in cam]], dtype=torch.float32), self._face_list(verts.shape[0]),
                           rot=rot, color=color, wireframe=self.wireframe, wire_px=self.wire_px, resolution=(W, H))
        return out[0].cpu().numpy()

    def render_people(self, img, people, colors=None, mode="painter"):
        """Every person of one frame in one call: `people` is one entry of prepare_rendering_results' list (OrderedDict person -> {'verts', 'cam'}, drawn in its
        order), colors an optional dict person -> (r, g, b).  numpy in, numpy out; the frame is uploaded once and downloaded once, whatever the number of people
        (the loop over Renderer.render moves it both ways per person).  Same pixels as that loop in painter mode."""
        W, H = int(self.resolution[0]), int(self.resolution[1])
        frame = None
        if img is not None:
            img = np.asarray(img)
            if img.shape != (H, W, 3):
                raise L.MaedHipError(f"Renderer.render_people: img has shape {img.shape}, the renderer was made for {(H, W, 3)}")
            frame = torch.from_numpy(np.ascontiguousarray(img.astype(np.uint8))).to(self.device)[None]
        if not people:
            return np.zeros((H, W, 3), dtype=np.uint8) if img is None else img.astype(np.uint8)
        V = int(np.asarray(next(iter(people.values()))["verts"]).shape[0])
        out = render_frame_results(frame, [people], self._face_list(V), colors=colors, mode=mode, wireframe=self.wireframe, wire_px=self.wire_px, resolution=(W, H),
                                   device=self.device)
        return out[0].cpu().numpy()


def convert_crop_cam_to_orig_img(cam, bbox, img_width, img_height):
    """weak-perspective camera of the crop (N, 3) = s, tx, ty and the crop boxes (N, 4) = cx, cy, w, h -> camera in the original image (N, 4) = sx, sy, tx, ty
    (demo_utils.py:98-115).  numpy arrays or tensors (any device); the result has the type, dtype and device of the input."""
    cx, cy, w, h = bbox[:, 0], bbox[:, 1], bbox[:, 2], bbox[:, 3]
    hw, hh = img_width / 2., img_height / 2.
    sx = cam[:, 0] * (1. / (img_width / w))
    sy = cam[:, 0] * (1. / (img_height / h))
    tx = ((cx - hw) / hw / sx) + cam[:, 1]
    ty = ((cy - hh) / hh / sy) + cam[:, 2]
    if isinstance(cam, torch.Tensor):
        return torch.stack([sx, sy, tx, ty], dim=1)
    return np.stack([sx, sy, tx, ty], axis=1)


def prepare_rendering_results(results, nframes):
    """per-person results {person: {'frame_ids', 'verts', 'orig_cam'}} -> one OrderedDict per frame {person: {'verts', 'cam'}}, the people of a frame in ascending
    order of the camera's y scale (demo_utils.py:118-135): drawn in that order, each over the previous result, the largest last"""
    per_frame = [[] for _ in range(nframes)]
    for person, data in results.items():
        for k, frame in enumerate(data["frame_ids"]):
            per_frame[frame].append((person, {"verts": data["verts"][k], "cam": data["orig_cam"][k]}))
    out = []
    for people in per_frame:
        order = np.argsort([float(rec["cam"][1]) for _, rec in people]) if people else []
        out.append(OrderedDict((people[i][0], people[i][1]) for i in order))
    return out
