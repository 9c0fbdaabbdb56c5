"""Mesh overlays on the device: the reference's visualisation step (lib/utils/renderer.py Renderer, lib/utils/demo_utils.py convert_crop_cam_to_orig_img /
prepare_rendering_results) on csrc/render.hip.  The reference draws with pyrender on OpenGL; an Instinct accelerator has no graphics pipeline, so the mesh is
rasterised by compute kernels (docs/design/11_render.md: projection, fill rule and depth are pinned, the look of the shader is this project's own).

    r = Renderer(resolution=(w, h), faces=faces, orig_img=True)          # faces: (n, 3) vertex indices, or smpl_arrays['f'] of the licensed model
    img = r.render(img, verts, cam=orig_cam[i], color=colour)             # numpy in, numpy out: the loop of the reference's visualize.py runs on it unchanged
    out = render_batch(frames, out["verts"], cams, faces)                  # device tensors in, device tensor out, no host synchronisation
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
