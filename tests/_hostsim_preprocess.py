"""TEST INFRASTRUCTURE: csrc/preprocess.hip alone on the host simulator (tests/hostsim), built with the compiler and flags of tests/hostsim/build_sim.py into a
second small library, so that the clip-preprocessing kernels are checked without a GPU.  MAED_SIM_ASAN=1: the AddressSanitizer build (global memory is heap
memory in the simulator: a gather or store outside a buffer, silent on the GPU, is a report with the kernel's source line)."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIM = os.path.join(HERE, "hostsim")
CSRC = os.path.join(ROOT, "maed_amd", "csrc")
ASAN = os.environ.get("MAED_SIM_ASAN", "0") not in ("", "0")
OUT_DIR = os.path.join(SIM, "_build_asan" if ASAN else "_build")
OUT = os.path.join(OUT_DIR, "libmaed_hostsim_preprocess.so")
CLANG = os.environ.get("MAED_HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")


def build(force=False):
    srcs = [os.path.join(CSRC, "preprocess.hip"), os.path.join(SIM, "sim_support.cpp"), os.path.join(SIM, "pre_support.cpp")]
    deps = srcs + [os.path.join(SIM, "hip", "hip_runtime.h"), os.path.join(CSRC, "common.cuh"), os.path.join(ROOT, "include", "maed_hip.h")]
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
        for name in ("maed_last_error", "maed_version", "maed_clip_preprocess", "maed_clip_preprocess_workspace"):
            fn = getattr(h, name)
            fn.restype, fn.argtypes = L.SIGNATURES[name]
        assert h.maed_version() < 0, "this must be the simulator, not the product library"
        _HANDLE = h
    return _HANDLE


@contextlib.contextmanager
def patched():
    """maed_amd.data / ops.clip_preprocess on the simulator library for the duration of a block (the pattern of tests/_hostsim.patched)"""
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


def run(tables, H, W, form=0, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), lib=None, pad=0):
    """maed_clip_preprocess on numpy tables (tests/_preprocess_ref.identity_tables layout) -> fp32 (F, 3, H, W); raises RuntimeError with the library's message"""
    lib = lib or load()
    src = np.ascontiguousarray(tables["src"], dtype=np.uint8)
    fi = np.ascontiguousarray(tables["frame_i"], dtype=np.int32)
    fm = np.ascontiguousarray(tables["frame_minv"], dtype=np.float32)
    ci = np.ascontiguousarray(tables["clip_i"], dtype=np.int32)
    cf = np.ascontiguousarray(tables["clip_f"], dtype=np.float32)
    F, N = len(fi), len(ci)
    out = np.full((F, 3, H, W), np.nan, dtype=np.float32)
    has_c = int((ci[:, 1:5] == 4).any())
    need = lib.maed_clip_preprocess_workspace(F, H, W)
    ws = np.zeros(need + 16, dtype=np.uint8)
    ws_ptr = (ws.ctypes.data + 15) & ~15
    norm = (C.c_float * 6)(*mean, *std)
    rc = lib.maed_clip_preprocess(src.ctypes.data, src.size, fi.ctypes.data, fm.ctypes.data, ci.ctypes.data, cf.ctypes.data, F, N, H, W, norm, has_c, form,
                                  out.ctypes.data, ws_ptr, need, None)
    if rc != 0:
        raise RuntimeError(f"maed_clip_preprocess -> {rc}: {lib.maed_last_error().decode()}")
    return out
