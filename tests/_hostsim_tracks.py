"""TEST INFRASTRUCTURE: csrc/tracks.hip and csrc/preprocess.hip on the host simulator (tests/hostsim), built with the compiler and flags of
tests/_hostsim_preprocess.py into their own small library, so that the track-box kernels, the crop-table builder and the video driver's device path are checked
without a GPU.  Global memory is host memory here: the runners take numpy arrays."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIM = os.path.join(HERE, "hostsim")
CSRC = os.path.join(ROOT, "maed_amd", "csrc")
OUT_DIR = os.path.join(SIM, "_build")
OUT = os.path.join(OUT_DIR, "libmaed_hostsim_tracks.so")
CLANG = os.environ.get("MAED_HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")
NAMES = ("maed_last_error", "maed_version", "maed_clip_preprocess", "maed_clip_preprocess_workspace", "maed_track_boxes", "maed_track_boxes_workspace",
         "maed_track_smooth", "maed_crop_tables")
LDS_FRAMES = 1024        # csrc/tracks.hip TRK_LDS_N: longer tracks keep their series in the workspace


def build(force=False):
    srcs = [os.path.join(CSRC, "tracks.hip"), os.path.join(CSRC, "preprocess.hip"), os.path.join(SIM, "sim_support.cpp"), os.path.join(SIM, "pre_support.cpp")]
    deps = srcs + [os.path.join(SIM, "hip", "hip_runtime.h"), os.path.join(CSRC, "common.cuh"), os.path.join(ROOT, "include", "maed_hip.h")]
    if not force and os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    os.makedirs(OUT_DIR, exist_ok=True)
    flags = [CLANG, "-std=c++20", "-O1", "-fPIC", "-pthread", "-I", SIM, "-Wno-unused-value"]
    tmp = OUT + f".{os.getpid()}.tmp"
    subprocess.run(flags + ["-shared"] + [a for s in srcs for a in ("-x", "c++", s)] + ["-o", tmp], check=True)
    os.replace(tmp, OUT)
    return OUT


_HANDLE = None


def load():
    global _HANDLE
    if _HANDLE is None:
        from maed_amd import _lib as L
        h = C.CDLL(build())
        for name in NAMES:
            fn = getattr(h, name)
            fn.restype, fn.argtypes = L.SIGNATURES[name]
        assert h.maed_version() < 0, "this must be the simulator, not the product library"
        _HANDLE = h
    return _HANDLE


@contextlib.contextmanager
def patched():
    """maed_amd.video / ops.clip_preprocess on the simulator library for the duration of a block (the pattern of tests/_hostsim_preprocess.patched): CPU tensors
    stand for device tensors"""
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


def _err(lib, what, rc):
    return RuntimeError(f"{what} -> {rc}: {lib.maed_last_error().decode()}")


def track_boxes(kps, lengths, vis_thresh, kernel_size, sigma, box_scale=1.1, guard=3, want_params=True):
    """maed_track_boxes on numpy: kps (K, L, J, 3), lengths (K) -> boxes fp32 (K, L, 4), params fp64 (K, L, 3), span int32 (K, 2).  Every output is allocated with
    `guard` extra rows behind it, filled with a pattern that must still be there on return."""
    lib = load()
    kps = np.ascontiguousarray(kps, dtype=np.float32)
    K, L, J = kps.shape[:3]
    lengths = np.ascontiguousarray(lengths, dtype=np.int32)
    boxes = np.full((K * L + guard, 4), -777.0, dtype=np.float32)
    params = np.full((K * L + guard, 3), -777.0, dtype=np.float64)
    span = np.full((K + guard, 2), -777, dtype=np.int32)
    need = lib.maed_track_boxes_workspace(K, L)
    ws = np.full(need // 8 + 1, np.nan, dtype=np.float64)
    rc = lib.maed_track_boxes(kps.ctypes.data, lengths.ctypes.data, K, L, J, float(vis_thresh), int(kernel_size), float(sigma), float(box_scale), boxes.ctypes.data,
                              params.ctypes.data if want_params else None, span.ctypes.data, ws.ctypes.data if need else None, need, None)
    if rc != 0:
        raise _err(lib, "maed_track_boxes", rc)
    assert (boxes[K * L:] == -777.0).all() and (span[K:] == -777).all(), "a guard row behind an output was written"
    assert (params[K * L:] == -777.0).all() if want_params else (params == -777.0).all(), "a guard row behind params was written"
    return boxes[:K * L].reshape(K, L, 4), params[:K * L].reshape(K, L, 3), span[:K]


def crop_tables(boxes, box_index, frame_index, T, n_frames, img_h, img_w, H, W, guard=2):
    """maed_crop_tables on numpy -> dict(frame_i, frame_minv, clip_i, clip_f), guard rows checked as above"""
    lib = load()
    boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
    bi = np.ascontiguousarray(box_index, dtype=np.int32)
    fi = np.ascontiguousarray(frame_index, dtype=np.int32)
    M = len(bi)
    N = (M + T - 1) // T
    frame_i = np.full((M + guard, 8), -777, dtype=np.int32)
    frame_minv = np.full((M + guard, 6), -777.0, dtype=np.float32)
    clip_i = np.full((N + guard, 8), -777, dtype=np.int32)
    clip_f = np.full((N + guard, 4), -777.0, dtype=np.float32)
    rc = lib.maed_crop_tables(boxes.ctypes.data, len(boxes), bi.ctypes.data, fi.ctypes.data, M, T, n_frames, img_h, img_w, H, W, frame_i.ctypes.data,
                              frame_minv.ctypes.data, clip_i.ctypes.data, clip_f.ctypes.data, None)
    if rc != 0:
        raise _err(lib, "maed_crop_tables", rc)
    for t, n in ((frame_i, M), (frame_minv, M), (clip_i, N), (clip_f, N)):
        assert (t[n:] == -777).all(), "a guard row behind a table was written"
    return dict(frame_i=frame_i[:M], frame_minv=frame_minv[:M], clip_i=clip_i[:N], clip_f=clip_f[:N])
