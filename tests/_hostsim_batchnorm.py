"""TEST INFRASTRUCTURE: csrc/batchnorm.hip alone on the host simulator (tests/hostsim), the way tests/_hostsim_render.py builds csrc/render.hip: a second small
library with the simulator's compiler and flags, so that the BatchNorm / pooling kernels of the stage-1 encoder are checked without a GPU.

Every entry point is called on buffers this module allocates itself: each output and scratch buffer sits between two guard zones of sentinel bytes, and a call
that changes a guard byte fails (`Guarded.check`)."""
import contextlib
import ctypes as C
import os
import subprocess

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIM = os.path.join(HERE, "hostsim")
CSRC = os.path.join(ROOT, "maed_amd", "csrc")
OUT_DIR = os.path.join(SIM, "_build")
OUT = os.path.join(OUT_DIR, "libmaed_hostsim_batchnorm.so")
CLANG = os.environ.get("MAED_HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")
NAMES = ("maed_last_error", "maed_version", "maed_batchnorm_chunks", "maed_batchnorm_stats", "maed_batchnorm_finalize", "maed_batchnorm_apply_fwd",
         "maed_batchnorm_bwd_reduce", "maed_batchnorm_bwd_apply", "maed_maxpool3s2p1_fwd", "maed_maxpool3s2p1_bwd", "maed_avgpool_fwd", "maed_avgpool_bwd")


def build(force=False):
    srcs = [os.path.join(CSRC, "batchnorm.hip"), os.path.join(SIM, "sim_support.cpp"), os.path.join(SIM, "pre_support.cpp")]
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
    """maed_amd.ops / maed_amd.resnet on this simulator library, CPU tensors standing in for device memory (the pattern of tests/_hostsim_render.patched)"""
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


GUARD = 64          # bytes on either side
SENTINEL = 0xA5


class Guarded:
    """a tensor of `shape` / `dtype` between two guard zones; `.t` is the tensor the kernel writes (64-byte aligned), check() asserts the guards are untouched"""
    live = []

    def __init__(self, shape, dtype, fill=None):
        n = 1
        for s in shape:
            n *= s
        nbytes = n * torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8)
        assert self.buf.data_ptr() % 64 == 0
        self.t = self.buf[GUARD:GUARD + nbytes].view(dtype).view(shape)
        if fill is not None:
            self.t.copy_(fill)
        Guarded.live.append(self)

    def check(self, what=""):
        assert bool((self.buf[:GUARD] == SENTINEL).all()), f"{what}: guard bytes in front of the buffer were written"
        assert bool((self.buf[-GUARD:] == SENTINEL).all()), f"{what}: guard bytes behind the buffer were written"


def check_all(what):
    for g in Guarded.live:
        g.check(what)
    Guarded.live.clear()


def _ok(lib, rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc}: {lib.maed_last_error().decode()}")


def _dt(dtype):
    return 0 if dtype == torch.float32 else 1


def bn_train(case, relu, eps=1e-5, momentum=0.1, frozen=False, lib=None):
    """forward + backward of one tests/_batchnorm_cases case through the C-ABI on guarded buffers; returns a dict of CPU tensors ((M, C) rows for activations)"""
    lib = lib or load()
    p = lambda t: None if t is None else t.data_ptr()
    x, res, dy = case["x2"], case["res2"], case["dy2"]
    M, C_ = x.shape
    dt = x.dtype
    chunks = lib.maed_batchnorm_chunks(M)
    part = Guarded((chunks * C_ * 2,), torch.float64)
    mean, rstd, mlo = Guarded((C_,), torch.float32), Guarded((C_,), torch.float32), Guarded((C_,), torch.float32, torch.zeros(C_))
    rm, rv = Guarded((C_,), torch.float32, case["rm"]), Guarded((C_,), torch.float32, case["rv"])
    if frozen:
        mean.t.copy_(case["rm"]); rstd.t.copy_(torch.rsqrt(case["rv"] + eps))
    else:
        _ok(lib, lib.maed_batchnorm_stats(p(x), M, C_, _dt(dt), p(part.t), eps, p(mean.t), p(mlo.t), p(rstd.t), p(rm.t), p(rv.t), momentum, None), "batchnorm_stats")
    y = Guarded((M, C_), dt)
    mask = Guarded((M * (C_ // 8),), torch.uint8) if (relu and res is not None) else None
    _ok(lib, lib.maed_batchnorm_apply_fwd(p(x), p(res), p(mean.t), p(rstd.t), p(case["gamma"]), p(case["beta"]), p(y.t), p(mask.t) if mask else None, M, C_, int(relu),
                                          _dt(dt), None), "batchnorm_apply_fwd")
    dgamma, dbeta = Guarded((C_,), torch.float32, case["dgamma0"]), Guarded((C_,), torch.float32, case["dbeta0"])
    sums = None if frozen else Guarded((C_ * 2,), torch.float32)
    part2 = Guarded((chunks * C_ * 2,), torch.float64)
    _ok(lib, lib.maed_batchnorm_bwd_reduce(p(x), p(dy), p(mask.t) if mask else None, p(mean.t), None if frozen else p(mlo.t), p(rstd.t), p(case["gamma"]), p(case["beta"]), p(part2.t),
                                           p(sums.t) if sums else None, p(dgamma.t), p(dbeta.t), M, C_, int(relu), _dt(dt), None), "batchnorm_bwd_reduce")
    dx = Guarded((M, C_), dt)
    dres = Guarded((M, C_), dt) if res is not None else None
    _ok(lib, lib.maed_batchnorm_bwd_apply(p(x), p(dy), p(mask.t) if mask else None, p(mean.t), None if frozen else p(mlo.t), p(rstd.t), p(case["gamma"]), p(case["beta"]), p(sums.t) if sums else None,
                                          p(dx.t), p(dres.t) if dres else None, M, C_, int(relu), _dt(dt), None), "batchnorm_bwd_apply")
    out = dict(y=y.t.clone(), dx=dx.t.clone(), dres=None if dres is None else dres.t.clone(), dgamma=dgamma.t.clone(), dbeta=dbeta.t.clone(), rm=rm.t.clone(),
               rv=rv.t.clone(), mean=mean.t.clone(), rstd=rstd.t.clone())
    check_all(f"batchnorm {tuple(x.shape)} {dt} relu={relu} res={res is not None}")
    return out


def maxpool(x_nhwc, dy_nhwc=None, lib=None):
    lib = lib or load()
    N, H, W, C_ = x_nhwc.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y, idx = Guarded((N, Ho, Wo, C_), x_nhwc.dtype), Guarded((N, Ho, Wo, C_), torch.uint8)
    _ok(lib, lib.maed_maxpool3s2p1_fwd(x_nhwc.data_ptr(), y.t.data_ptr(), idx.t.data_ptr(), N, H, W, C_, _dt(x_nhwc.dtype), None), "maxpool3s2p1_fwd")
    dx = None
    if dy_nhwc is not None:
        dx = Guarded((N, H, W, C_), x_nhwc.dtype)
        _ok(lib, lib.maed_maxpool3s2p1_bwd(dy_nhwc.data_ptr(), idx.t.data_ptr(), dx.t.data_ptr(), N, H, W, C_, _dt(x_nhwc.dtype), None), "maxpool3s2p1_bwd")
    out = (y.t.clone(), None if dx is None else dx.t.clone())
    check_all(f"maxpool {tuple(x_nhwc.shape)}")
    return out


def avgpool(x_fhwc, dy=None, lib=None):
    lib = lib or load()
    F_, HW, C_ = x_fhwc.shape
    y = Guarded((F_, C_), torch.float32)
    _ok(lib, lib.maed_avgpool_fwd(x_fhwc.data_ptr(), y.t.data_ptr(), F_, HW, C_, _dt(x_fhwc.dtype), None), "avgpool_fwd")
    dx = None
    if dy is not None:
        dx = Guarded((F_, HW, C_), x_fhwc.dtype)
        _ok(lib, lib.maed_avgpool_bwd(dy.data_ptr(), dx.t.data_ptr(), F_, HW, C_, _dt(x_fhwc.dtype), None), "avgpool_bwd")
    out = (y.t.clone(), None if dx is None else dx.t.clone())
    check_all(f"avgpool {tuple(x_fhwc.shape)}")
    return out
