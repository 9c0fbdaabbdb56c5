"""TEST INFRASTRUCTURE: the entry points of csrc/batchnorm.hip that take their statistics over the batch of all ranks (maed_batchnorm_stats_local /
finalize_dev / bwd_reduce_local / bwd_apply_dev) on the host simulator.  Built by tests/_hostsim_batchnorm.build(); the ctypes signatures of the new names are
set here.  `bn_sharded` runs one tests/_batchnorm_cases case cut into row shards -- one shard stands for one rank, the records are added on the host in fp64
where the all-reduce would add them -- with every output, record and scratch buffer between guard zones (`Guarded`)."""
import contextlib
import ctypes as C

import torch
import torch.nn as nn

import _hostsim_batchnorm as S
from _hostsim_batchnorm import Guarded

vp, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int, C.c_float
SIGNATURES = {
    "maed_batchnorm_stats_local": (i32, [vp, i64, i32, i32, vp, vp, vp]),
    "maed_batchnorm_finalize_dev": (i32, [vp, i32, f32, vp, vp, vp, vp, vp, f32, vp]),
    "maed_batchnorm_bwd_reduce_local": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, vp]),
    "maed_batchnorm_bwd_apply_dev": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, vp]),
}


def load():
    lib = S.load()
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


@contextlib.contextmanager
def patched():
    """_hostsim_batchnorm.patched() with the signatures above set on the handle (a spawned rank loads its own)"""
    load()
    with S.patched() as lib:
        yield lib


# ---- module level: a small stack of resnet.BatchNorm2d (CPU ranks over gloo and the one-rank collectives on the GPU share it) ----
CHANNELS = (8, 72)
SPLIT = (3, 1)                  # images of 5 x 5 on rank 0 / rank 1


class Stack(nn.Module):
    """plain, ReLU, and residual + ReLU"""

    def __init__(self, C_):
        from maed_amd.resnet import BatchNorm2d
        super().__init__()
        self.bn1, self.bn2, self.bn3 = BatchNorm2d(C_), BatchNorm2d(C_), BatchNorm2d(C_)
        g = torch.Generator().manual_seed(C_)
        with torch.no_grad():
            for bn in (self.bn1, self.bn2, self.bn3):
                bn.weight.copy_(torch.rand(C_, generator=g) + 0.5); bn.bias.copy_(torch.randn(C_, generator=g) * 0.3)
                bn.running_mean.copy_(torch.randn(C_, generator=g) * 0.2); bn.running_var.copy_(torch.rand(C_, generator=g) + 0.5)

    def forward(self, x):
        a = self.bn1(x)
        b = self.bn2(a + 0.5 * x, relu=True)
        return self.bn3(2.0 * b - x, residual=a, relu=True)


def data(C_):
    g = torch.Generator().manual_seed(100 + C_)
    n = sum(SPLIT)
    x = torch.randn(n, C_, 5, 5, generator=g) * (torch.rand(1, C_, 1, 1, generator=g) * 1.5 + 0.5) + torch.randn(1, C_, 1, 1, generator=g) * 0.5
    return x.contiguous(memory_format=torch.channels_last), torch.randn(n, C_, 5, 5, generator=g)


def train_step(model, x, w):
    """summed loss; returns what the comparisons need as plain tensors"""
    x = x.clone().requires_grad_(True)
    y = model(x)
    (y * w).sum().backward()
    out = dict(y=y.detach().clone(), dx=x.grad.clone())
    for n, p in model.named_parameters():
        out["grad." + n] = p.grad.clone()
    for n, b in model.named_buffers():
        out["buf." + n] = b.clone()
    return out


def _p(t):
    return None if t is None else t.data_ptr()


def bn_sharded(case, relu, sizes, eps=1e-5, momentum=0.1, lib=None, G=Guarded, check_all=S.check_all, dev="cpu", stream=None):
    """forward + backward of `case` with its rows cut into shards of `sizes` rows.  Returns what tests/_hostsim_batchnorm.bn_train returns (y / dx / dres
    concatenated, dgamma / dbeta = the case's start values + the sum of the shards' increments, the running buffers of shard 0) plus mean / rstd / mean_lo of
    shard 0; the statistics and running buffers of every shard must be bit-equal.
    The GPU tests run the same sequence on the product library: G / check_all are then their guarded device allocations, dev / stream the device and its stream."""
    lib = lib or load()
    x, dy = case["x2"].to(dev), case["dy2"].to(dev)
    res = None if case["res2"] is None else case["res2"].to(dev)
    M, C_ = x.shape
    dt = x.dtype
    assert sum(sizes) == M and min(sizes) >= 1
    cuts = [0]
    for n in sizes:
        cuts.append(cuts[-1] + n)
    sh = [dict(x=x[a:b].clone(), dy=dy[a:b].clone(), res=None if res is None else res[a:b].clone(), M=b - a) for a, b in zip(cuts, cuts[1:])]
    gamma, beta = case["gamma"].to(dev), case["beta"].to(dev)
    for s in sh:                                                    # every rank: local sums + its row count
        s["part"] = G((lib.maed_batchnorm_chunks(s["M"]) * C_ * 2,), torch.float64)
        s["rec"] = G((2 * C_ + 1,), torch.float64)
        S._ok(lib, lib.maed_batchnorm_stats_local(_p(s["x"]), s["M"], C_, S._dt(dt), _p(s["part"].t), _p(s["rec"].t), stream), "batchnorm_stats_local")
    total = torch.stack([s["rec"].t for s in sh]).sum(0)            # the all-reduce
    assert float(total[2 * C_]) == M
    for s in sh:
        s["rec"].t.copy_(total)
        s["mean"], s["rstd"], s["mlo"] = G((C_,), torch.float32), G((C_,), torch.float32), G((C_,), torch.float32)
        s["rm"], s["rv"] = G((C_,), torch.float32, case["rm"]), G((C_,), torch.float32, case["rv"])
        S._ok(lib, lib.maed_batchnorm_finalize_dev(_p(s["rec"].t), C_, eps, _p(s["mean"].t), _p(s["mlo"].t), _p(s["rstd"].t), _p(s["rm"].t), _p(s["rv"].t), momentum, stream),
              "batchnorm_finalize_dev")
        s["y"] = G((s["M"], C_), dt)
        s["mask"] = G((s["M"] * (C_ // 8),), torch.uint8) if (relu and res is not None) else None
        S._ok(lib, lib.maed_batchnorm_apply_fwd(_p(s["x"]), _p(s["res"]), _p(s["mean"].t), _p(s["rstd"].t), _p(gamma), _p(beta), _p(s["y"].t), _p(s["mask"].t) if s["mask"] else None,
                                                s["M"], C_, int(relu), S._dt(dt), stream), "batchnorm_apply_fwd")
    for s in sh:
        s["dgamma"], s["dbeta"] = G((C_,), torch.float32, torch.zeros(C_, device=dev)), G((C_,), torch.float32, torch.zeros(C_, device=dev))
        s["part2"] = G((lib.maed_batchnorm_chunks(s["M"]) * C_ * 2,), torch.float64)
        s["rec2"] = G((2 * C_,), torch.float64)
        S._ok(lib, lib.maed_batchnorm_bwd_reduce_local(_p(s["x"]), _p(s["dy"]), _p(s["mask"].t) if s["mask"] else None, _p(s["mean"].t), _p(s["mlo"].t), _p(s["rstd"].t), _p(gamma),
                                                       _p(beta), _p(s["part2"].t), _p(s["rec2"].t), _p(s["dgamma"].t), _p(s["dbeta"].t), s["M"], C_, int(relu), S._dt(dt), stream),
              "batchnorm_bwd_reduce_local")
    total2 = torch.stack([s["rec2"].t for s in sh]).sum(0)
    for s in sh:
        s["rec2"].t.copy_(total2)
        s["dx"] = G((s["M"], C_), dt)
        s["dres"] = G((s["M"], C_), dt) if res is not None else None
        S._ok(lib, lib.maed_batchnorm_bwd_apply_dev(_p(s["x"]), _p(s["dy"]), _p(s["mask"].t) if s["mask"] else None, _p(s["mean"].t), _p(s["mlo"].t), _p(s["rstd"].t), _p(gamma),
                                                    _p(beta), _p(s["rec2"].t), _p(s["rec"].t[2 * C_:]), _p(s["dx"].t), _p(s["dres"].t) if s["dres"] else None, s["M"], C_, int(relu),
                                                    S._dt(dt), stream), "batchnorm_bwd_apply_dev")
    for s in sh[1:]:
        for k in ("mean", "rstd", "mlo", "rm", "rv"):
            assert torch.equal(s[k].t, sh[0][k].t), f"{k} differs between shards"
    out = dict(y=torch.cat([s["y"].t for s in sh]), dx=torch.cat([s["dx"].t for s in sh]), dres=None if res is None else torch.cat([s["dres"].t for s in sh]),
               dgamma=case["dgamma0"].to(dev) + torch.stack([s["dgamma"].t for s in sh]).sum(0), dbeta=case["dbeta0"].to(dev) + torch.stack([s["dbeta"].t for s in sh]).sum(0),
               rm=sh[0]["rm"].t.clone(), rv=sh[0]["rv"].t.clone(), mean=sh[0]["mean"].t.clone(), rstd=sh[0]["rstd"].t.clone(), mean_lo=sh[0]["mlo"].t.clone())
    check_all(f"batchnorm shards {sizes} of {tuple(x.shape)} {dt} relu={relu} res={res is not None}")
    return out
