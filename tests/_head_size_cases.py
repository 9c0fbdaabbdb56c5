"""Cases and fp64 references shared by the head-size tests (tests/test_hostsim_head_sizes.py on the host simulator, tests/test_gpu_head_sizes.py on the GPU):
maed_attn_seq_fwd / _bwd at head sizes 32 / 96 / 128 against oracle.maed_ref in fp64 on the same rounded inputs.  A reference is computed once per
(case, head size, storage type) and never modified."""
import functools

import torch

from oracle import maed_ref as R
from maed_amd import _lib as L
from maed_amd import ops

from _util import q, rnd, tol

HEAD_SIZES = [32, 96, 128]
H = 2
# (kind, size): spatial L = the edges of the 32-row sub-tile, the 64-row LDS tile and the 128-row workgroup; temporal T with P = 5 tokens; coupling T*P = 3*43 = 129
CASES = [("spatial", 5), ("spatial", 33), ("spatial", 64), ("spatial", 65), ("spatial", 130), ("temporal", 1), ("temporal", 3), ("temporal", 16), ("coupling", 3)]
ENGINES = [("bf16-mfma", torch.bfloat16, L.IMPL_AUTO), ("f32-valu", torch.float32, L.IMPL_AUTO), ("bf16-valu", torch.bfloat16, L.IMPL_VALU)]


def geometry(kind, size):
    """(frames, tokens per frame, clip length, (groups, length, inner)) -- two groups each: F = 2 frames for spatial attention, N = 2 clips otherwise"""
    if kind == "spatial":
        return 2, size, 1, (2, size, 1)
    if kind == "temporal":
        return 2 * size, 5, size, (2, size, 5)
    return 2 * size, 43, size, (2, size * 43, 1)


@functools.lru_cache(maxsize=None)
def reference(kind, size, D, dtype):
    """(qkv, d_o) rounded to the storage type, and o / lse / dqkv in fp64 (lse in the layout the entry point writes)"""
    Fr, P, T, _ = geometry(kind, size)
    C_ = D * H
    qkv = q(rnd(Fr, P, 3 * C_, seed=7 * size + D), dtype)
    do = q(rnd(Fr, P, C_, seed=4), dtype)
    x = qkv.double().requires_grad_(True)
    qq, kk, vv = R.split_qkv(x, H)
    scale = D ** -0.5
    if kind == "spatial":
        oref = R.attention_spatial(qq, kk, vv, scale)
        lse = torch.logsumexp((qq @ kk.transpose(-2, -1)) * scale, dim=-1)                       # (F, H, P)
    elif kind == "temporal":
        oref = R.attention_temporal(qq, kk, vv, T, scale)
        qt, kt = (t.reshape(-1, T, H, P, D).permute(0, 2, 3, 1, 4) for t in (qq, kk))         # (N, H, P, T, d)
        lse = torch.logsumexp((qt @ kt.transpose(-2, -1)) * scale, dim=-1).permute(0, 3, 1, 2).reshape(Fr, H, P)
    else:
        oref = R.attention_coupling(qq, kk, vv, T, scale)
        qc, kc = (t.reshape(-1, T, H, P, D).transpose(1, 2).reshape(-1, H, T * P, D) for t in (qq, kk))
        lse = torch.logsumexp((qc @ kc.transpose(-2, -1)) * scale, dim=-1)                       # (N, H, T*P)
    oref.backward(do.double())
    return qkv, do, oref.detach(), lse.detach(), x.grad.detach()


def close(got, ref, rtol, atol, what=""):
    got, ref = got.double().cpu(), ref.double().cpu()
    err = (got - ref).abs()
    print(f"{what:40s} max_abs_err={err.max().item():.3e} ref_max={ref.abs().max().item():.3e}")
    assert torch.allclose(got, ref, rtol=rtol, atol=atol), (what, err.max().item())


def run_case(kind, size, D, dtype, impl, device="cpu"):
    """forward, backward and accumulate = 1 of one case at the bars of the D = 64 cases of tests/test_hostsim_attention.py"""
    _, _, _, geo = geometry(kind, size)
    qkv, do, oref, lse_ref, gref = reference(kind, size, D, dtype)
    qd, dod = qkv.to(dtype).to(device), do.to(dtype).to(device)
    o, lse = ops.attn_seq_fwd(qd, H, *geo, impl=impl)
    dqkv = ops.attn_seq_bwd(qd, o, dod, lse, H, *geo, impl=impl)
    acc = ops.attn_seq_bwd(qd, o, dod, lse, H, *geo, dqkv=dqkv.clone(), accumulate=True, impl=impl)
    tag = f"{kind}{size} D={D} "
    close(o.float(), oref, **tol(dtype), what=tag + "o")
    close(lse.reshape(lse_ref.shape), lse_ref, rtol=1e-4, atol=1e-3 if dtype == torch.float32 else 2e-2, what=tag + "lse")
    close(dqkv.float(), gref, **tol(dtype, 0.5), what=tag + "dqkv")
    close(acc.float(), 2 * gref, **tol(dtype, 1.0), what=tag + "dqkv accumulate")
