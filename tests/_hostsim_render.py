"""TEST INFRASTRUCTURE: csrc/render.hip alone on the host simulator (tests/hostsim), the way tests/_hostsim_preprocess.py builds csrc/preprocess.hip: a second small
library with the simulator's compiler and flags, so that the rasteriser is checked without a GPU.  tests/hostsim/render_support.h adds the 64-bit atomic minimum.
MAED_SIM_ASAN=1: the AddressSanitizer build (host code only: a gather or store outside a buffer is a report with the kernel's source line)."""
import contextlib
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIM = os.path.join(HERE, "hostsim")
CSRC = os.path.join(ROOT, "maed_amd", "csrc")
ASAN = os.environ.get("MAED_SIM_ASAN", "0") not in ("", "0")
OUT_DIR = os.path.join(SIM, "_build_asan" if ASAN else "_build")
OUT = os.path.join(OUT_DIR, "libmaed_hostsim_render.so")
CLANG = os.environ.get("MAED_HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")


def build(force=False):
    srcs = [os.path.join(CSRC, "render.hip"), os.path.join(SIM, "sim_support.cpp"), os.path.join(SIM, "pre_support.cpp")]
    deps = srcs + [os.path.join(SIM, "hip", "hip_runtime.h"), os.path.join(SIM, "render_support.h"), os.path.join(CSRC, "common.cuh"),
                   os.path.join(ROOT, "include", "maed_hip.h")]
    if not force and os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    os.makedirs(OUT_DIR, exist_ok=True)
    san = ["-fsanitize=address", "-g", "-fno-omit-frame-pointer"] if ASAN else []
    flags = [CLANG, "-std=c++20", "-O1", "-fPIC", "-pthread", "-I", SIM, "-Wno-unused-value"] + san
    tmp = OUT + f".{os.getpid()}.tmp"
    subprocess.run(flags + ["-shared"] + (["-shared-libsan"] if ASAN else []) + [a for s in srcs for a in ("-x", "c++", s)] + ["-o", tmp], check=True)
    os.replace(tmp, OUT)
    return OUT


_HANDLE = None


def load():
    global _HANDLE
    if _HANDLE is None:
        from maed_amd import _lib as L
        h = C.CDLL(build())
        for name in ("maed_last_error", "maed_version", "maed_render_mesh", "maed_render_mesh_workspace"):
            fn = getattr(h, name)
            fn.restype, fn.argtypes = L.SIGNATURES[name]
        assert h.maed_version() < 0, "this must be the simulator, not the product library"
        _HANDLE = h
    return _HANDLE


@contextlib.contextmanager
def patched():
    """maed_amd.render / ops.render_mesh on the simulator library, CPU tensors standing in for device memory (the pattern of tests/_hostsim_preprocess.patched)"""
    from maed_amd import _lib as L
    from maed_amd import ops
    saved = (L._lib, L._init_pending, ops._p, ops._stream)
    L._lib, L._init_pending = load(), False
    ops._p = lambda t: None if t is None else t.data_ptr()
    ops._stream = lambda: None
    try:
        yield L._lib
    finally:
        L._lib, L._init_pending, ops._p, ops._stream = saved


def run(s, frames="scene", wireframe=False, wire_px=0.5, form=0, base=(1.0, 1.0, 0.9), lib=None, want=("out", "face_id", "depth"), faces_host=True, raster_only=False):
    """maed_render_mesh of the simulator library on a scene dict of tests/_render_cases.py (numpy in, numpy out); raises RuntimeError with the library's message"""
    import numpy as np
    from maed_amd.render import FaceList
    lib = lib or load()
    verts, faces, cams, H, W = s["verts"], s["faces"], s["cams"], s["H"], s["W"]
    B, V, nf = verts.shape[0], verts.shape[1], len(faces)
    fl = FaceList(np.clip(faces, 0, V - 1), V)          # (the CSR of a deliberately bad face list: built from the clipped copy; the library sees the bad one)
    fr = s["frames"] if isinstance(frames, str) else frames
    out = np.full((B, H, W, 3), 77, dtype=np.uint8) if "out" in want else None
    fid = np.full((B, H, W), -7, dtype=np.int32) if "face_id" in want else None
    dep = np.full((B, H, W), np.nan, dtype=np.float32) if "depth" in want else None
    rots = s.get("rots")
    flags = (1 if wireframe else 0) | (2 if raster_only else 0) | (form << 4)
    need = lib.maed_render_mesh_workspace(B, V, nf, H, W, flags)
    ws = np.zeros(need + 16, dtype=np.uint8)
    ws_ptr = (ws.ctypes.data + 15) & ~15
    p = lambda a: None if a is None else a.ctypes.data
    rc = lib.maed_render_mesh(p(verts), p(faces), p(faces) if faces_host else None, p(fl.vf_off), p(fl.vf_idx), p(cams), p(rots), p(fr), p(out), p(fid), p(dep), B, V, nf,
                              H, W, (C.c_float * 3)(*base), wire_px, flags, ws_ptr, need, None)
    if rc != 0:
        raise RuntimeError(f"maed_render_mesh -> {rc}: {lib.maed_last_error().decode()}")
    return dict(out=out, face_id=fid, depth=dep)
