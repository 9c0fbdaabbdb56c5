"""TEST INFRASTRUCTURE: inputs and fp64 references of the BatchNorm / pooling kernels of the stage-1 encoder (csrc/batchnorm.hip), shared by the host-simulator
tests (tests/test_hostsim_batchnorm.py) and the GPU tests (tests/test_gpu_cnn.py).  References are computed once per case and cached."""
import functools

import torch
import torch.nn.functional as F

# (N, C, H, W): 126 ragged rows; 75 rows of 256 channels; two values per channel (unbiased factor 2); C no multiple of 64; 6400 rows = many row chunks;
# 1323 rows = several chunks of 32 rows with a partial last one (the reductions stripe max(32, M / 1024) rows per workgroup)
BN_SHAPES = [(2, 64, 7, 9), (3, 256, 5, 5), (1, 2048, 1, 2), (2, 72, 3, 3), (4, 64, 40, 40), (3, 64, 21, 21)]
EPS, MOMENTUM = 1e-5, 0.1


def rows(t):
    """(N, C, H, W) -> contiguous (N*H*W, C): the channels_last row matrix"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def unrows(t2, shape):
    N, C_, H, W = shape
    return t2.reshape(N, H, W, C_).permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def case(shape, dtype, res, seed=0, mean_over_std=0.0):
    """CPU tensors, activations already rounded to `dtype`; x has per-channel standard deviation ~ U(0.5, 2) and mean = mean_over_std * that"""
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    N, C_, H, W = shape
    std = torch.rand(C_, generator=g) * 1.5 + 0.5
    mean = (mean_over_std * std) if mean_over_std else torch.randn(C_, generator=g) * 0.5
    x = (torch.randn(shape, generator=g) * std.view(1, -1, 1, 1) + mean.view(1, -1, 1, 1)).to(dtype)
    r = torch.randn(shape, generator=g).to(dtype) if res else None
    dy = torch.randn(shape, generator=g).to(dtype)
    c = dict(shape=shape, dtype=dtype, x=x, res=r, dy=dy, gamma=torch.rand(C_, generator=g) + 0.5, beta=torch.randn(C_, generator=g) * 0.3,
             rm=torch.randn(C_, generator=g) * 0.2, rv=torch.rand(C_, generator=g) + 0.5, dgamma0=torch.randn(C_, generator=g), dbeta0=torch.randn(C_, generator=g))
    c["x2"], c["dy2"], c["res2"] = rows(x), rows(dy), (rows(r) if res else None)
    return c


@functools.lru_cache(maxsize=None)
def reference(shape, dtype, res, relu, training=True, seed=0, mean_over_std=0.0):
    """fp64 on the dtype-rounded inputs: y, dx, dres, dgamma / dbeta (added to the case's non-zero start values), running buffers after one step"""
    c = case(shape, dtype, res, seed, mean_over_std)
    x = c["x"].double().requires_grad_(True)
    r = c["res"].double().requires_grad_(True) if res else None
    gm, bt = c["gamma"].double().requires_grad_(True), c["beta"].double().requires_grad_(True)
    rm, rv = c["rm"].double().clone(), c["rv"].double().clone()
    y = F.batch_norm(x, rm, rv, gm, bt, training, MOMENTUM, EPS)
    if res:
        y = y + r
    if relu:
        y = F.relu(y)
    y.backward(c["dy"].double())
    return dict(y=rows(y.detach()), dx=rows(x.grad), dres=rows(r.grad) if res else None, dgamma=c["dgamma0"].double() + gm.grad, dbeta=c["dbeta0"].double() + bt.grad,
                rm=rm, rv=rv)


def tol(dtype, scale=1.0):
    """tests/_util.tol (the project's elementwise tolerance)"""
    return dict(rtol=2e-5, atol=2e-5 * scale) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2 * scale)


def affine_tol(dtype, ref):
    """dgamma / dbeta: test_groupnorm_fused's bars"""
    big = max(1.0, float(ref.abs().max()))
    return dict(rtol=1e-4, atol=1e-4 * big) if dtype == torch.float32 else dict(rtol=2e-2, atol=3e-2 * big)


def close(name, got, ref, rtol, atol):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    print(f"{name:60s} max_abs={float(err.max()):.3e} ref_max={float(ref.abs().max()):.3e}")
    assert not torch.isnan(got).any(), name
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.numel()} elements outside atol={atol:g} rtol={rtol:g}; max |err| {float(err.max()):.3e}"


def check_bn(name, got, ref, dtype, training=True):
    close(name + " y", got["y"], ref["y"], **tol(dtype, 4))
    close(name + " dx", got["dx"], ref["dx"], **tol(dtype, 2))
    if ref["dres"] is not None:
        close(name + " dres", got["dres"], ref["dres"], **tol(dtype, 2))
    close(name + " dgamma", got["dgamma"], ref["dgamma"], **affine_tol(dtype, ref["dgamma"]))
    close(name + " dbeta", got["dbeta"], ref["dbeta"], **affine_tol(dtype, ref["dbeta"]))
    if training:
        # rtol 1e-5; the absolute term only covers a running mean that cancels to almost nothing: two fp32 roundings (2^-24 each) of terms of magnitude <= 2
        close(name + " running_mean", got["rm"], ref["rm"], rtol=1e-5, atol=2e-7)
        close(name + " running_var", got["rv"], ref["rv"], rtol=1e-5, atol=2e-7)
