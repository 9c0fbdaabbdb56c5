"""Mesh overlay (csrc/render.hip) in isolation, event-timed: 16 frames of the SMPL-sized procedural mesh (6890 vertices, 13776 faces) at 224 x 224 and at
1920 x 1080, the mesh a third of the frame height and filling the frame, in both raster forms.  Per row: frames per second of the whole call, the split between
the raster part (visibility-buffer clear + vertex pass + raster pass, timed with MAED_RENDER_RASTER_ONLY) and the rest (normals + resolve, by difference), and the
bytes the resolve pass moves (8 B of visibility word + 3 B of frame read + 3 B written per pixel) as a share of HBM peak.  Every window rotates over SETS copies of
the frames and outputs; with the 8-byte visibility buffer the 1080p working set (265 MB + SETS x 200 MB) is past the 256 MB Infinity Cache, the 224 x 224 one
(6 MB + SETS x 5 MB) is cache-resident as it would be in use.  The window is repeated REPEATS times; minimum and median are printed.
Section "people": 16 frames at 1920 x 1080 with K = 1, 2 and 4 people each (the same mesh under K cameras, a third to half of the frame height, overlapping partly).
Three arms, alternating window by window in one process: render_people in painter and in shared-depth mode (one pass); the per-layer device loop (render_batch once per
layer, the first from the frames into the output, the others in place); and the host loop of INTEGRATION.md section 2b (Renderer.render per person and frame, numpy in
and out, host clock, NUMPY_PASSES passes).  Painter, the device loop and the host loop must give the same pixels; the script checks it.
The mesh generator is the tests' (tests/_render_ref.py): this script needs the test tree next to it.
usage: render_micro.py [iters] [all|mesh|people]      (one process; run it under a time limit)"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _render_ref as R          # the procedural meshes of the tests
from maed_amd import ops
from maed_amd.render import FaceList, Renderer, render_batch, render_people

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
section = sys.argv[2] if len(sys.argv) > 2 else "all"
SETS, REPEATS, B = 4, 3, 16
NUMPY_PASSES = 5
HBM_PEAK = 8.0e12
FORMS = {ops.RENDER_FORM_LANE: "lane", ops.RENDER_FORM_SPLIT: "split"}


def timed(call):
    for i in range(2 * SETS):
        call(i)
    torch.cuda.synchronize()
    us = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            call(i)
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / iters)
    return min(us), float(np.median(us))


def window(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        call(i)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def people_section(v, fl):
    W, H = 1920, 1080
    frames = [torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(SETS)]
    outs = [torch.empty_like(x) for x in frames]
    colours = np.float32([[1.0, 1.0, 0.9], [0.7, 0.9, 1.0], [1.0, 0.6, 0.6], [0.6, 1.0, 0.6]])
    spots = [(1 / 3, (-0.1, 0.0)), (0.5, (0.05, -0.05)), (0.4, (-0.3, 0.1)), (0.45, (0.25, 0.05))]
    for K in (1, 2, 4):
        # mesh b * K + k: person k of frame b (already grouped by frame: render_people has nothing to reorder)
        cams = np.stack([R.fit_cam(v, H, W, spots[k][0], centre=(spots[k][1][0] + 0.01 * b, spots[k][1][1])) for b in range(B) for k in range(K)]).astype(np.float32)
        shift = np.float32([[0.0, 0.0, 0.1 * k] for b in range(B) for k in range(K)])
        verts = torch.from_numpy(v[None] + shift[:, None, :]).cuda().contiguous()
        cams_t = torch.from_numpy(cams).cuda()
        col_t = torch.from_numpy(colours[np.arange(B * K) % K]).cuda()
        fidx = np.repeat(np.arange(B), K)
        layer_v = [verts[k::K].contiguous() for k in range(K)]
        layer_c = [cams_t[k::K].contiguous() for k in range(K)]

        def one_pass(mode):
            return lambda i: render_people(frames[i % SETS], verts, cams_t, fidx, fl, colors=col_t, mode=mode, out=outs[i % SETS])

        def per_layer(i):
            src = frames[i % SETS]
            for k in range(K):
                render_batch(src, layer_v[k], layer_c[k], fl, color=tuple(colours[k]), out=outs[i % SETS])
                src = outs[i % SETS]

        arms = {"render_people painter": one_pass("painter"), "render_people depth": one_pass("depth"), "render_batch per layer": per_layer}
        for call in arms.values():
            for i in range(2 * SETS):
                call(i)
        torch.cuda.synchronize()
        us = {name: [] for name in arms}
        for _ in range(REPEATS):                          # (alternating: every round times every arm once)
            for name, call in arms.items():
                us[name].append(window(call))
        arms["render_people painter"](0)
        a = outs[0].clone()
        per_layer(0)
        same = bool(torch.equal(a, outs[0]))
        # the host loop: numpy in and out, one Renderer.render per person and frame
        r = Renderer(resolution=(W, H), faces=fl.faces, orig_img=True)
        r._fl = fl
        host_frames, host_verts = frames[0].cpu().numpy(), verts.cpu().numpy()
        host = []
        for _ in range(1 + NUMPY_PASSES):                 # (the first pass is the warm-up)
            t0 = time.perf_counter()
            for b in range(B):
                img = host_frames[b]
                for k in range(K):
                    img = r.render(img, host_verts[b * K + k], cam=cams[b * K + k], color=colours[k])
            host.append(1e6 * (time.perf_counter() - t0))
        same_host = bool(np.array_equal(img, a[B - 1].cpu().numpy()))
        row = "   ".join(f"{name} {min(t):8.1f} / {float(np.median(t)):8.1f} us" for name, t in us.items())
        print(f"people {B} x {W}x{H} K={K}  {row}   numpy loop {min(host[1:]):10.1f} / {float(np.median(host[1:])):10.1f} us   painter == per layer: {same}, == numpy loop (last frame): {same_host}", flush=True)


def main():
    assert torch.cuda.is_available(), "render_micro needs a GPU"
    print(f"device {torch.cuda.get_device_name(0)}; {iters} calls per window over {SETS} buffer sets, {REPEATS} windows per row (min / median)", flush=True)
    v, f = R.smpl_sized()
    fl = FaceList(f, len(v))
    f_t, off, idx = fl.on("cuda")
    if section in ("all", "people"):
        people_section(v, fl)
    if section == "people":
        return
    for W, H in ((224, 224), (1920, 1080)):
        frames = [torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(SETS)]
        outs = [torch.empty_like(x) for x in frames]
        for label, frac in (("third of the height", 1 / 3), ("filling the frame", 0.98)):
            cams = torch.from_numpy(np.stack([R.fit_cam(v, H, W, frac, centre=(0.01 * k, 0.0)) for k in range(B)])).cuda()
            verts = torch.from_numpy(v)[None].repeat(B, 1, 1).contiguous().cuda()
            ref = None
            for form in FORMS:
                full = lambda i: ops.render_mesh(verts, f_t, fl.faces, off, idx, cams, H, W, frames=frames[i % SETS], out=outs[i % SETS], form=form)
                rast = lambda i: ops.render_mesh(verts, f_t, fl.faces, off, idx, cams, H, W, frames=frames[i % SETS], out=outs[i % SETS], form=form, raster_only=True)
                t_full, med = timed(full)
                t_rast, _ = timed(rast)
                full(0)
                got = outs[0].clone()
                same = "" if ref is None else f"  bit-equal to lane: {bool(torch.equal(got, ref))}"
                ref = got if ref is None else ref
                resolve = max(t_full - t_rast, 1e-3)
                nbytes = B * H * W * 14
                print(f"render {B} x {W}x{H} {label:20s} {FORMS[form]:5s} {t_full:8.1f} / {med:8.1f} us = {B / (t_full * 1e-6):9.0f} frames/s   raster part {t_rast:8.1f} us, "
                      f"normals + resolve {resolve:8.1f} us moving {nbytes / 1e6:6.1f} MB = {nbytes / (resolve * 1e-6) / 1e12:5.2f} TB/s = "
                      f"{nbytes / (resolve * 1e-6) / HBM_PEAK:.3f} of HBM peak{same}", flush=True)
        del frames, outs


if __name__ == "__main__":
    main()
