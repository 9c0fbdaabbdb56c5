"""Head sizes 32 / 96 / 128 (NUM_HEADS other than dim/64): constructors, the head-size-generic attention kernels (csrc/attn_heads.hip: bf16 MFMA, exact fp32,
bf16 storage on the exact kernels) and the fused STE block at C = D*H, on the host simulator against fp64 autograd through the CPU oracle.  Bars are those of
the D = 64 cases of tests/test_hostsim_attention.py."""
from functools import partial

import pytest
import torch
import torch.nn as nn

import maed_amd
from oracle import maed_ref as R
from maed_amd import _lib as L
from maed_amd import ops
from maed_amd.vision_transformer import Attention, Block

from _hostsim import patched
from _util import q, rnd, tol
import _head_size_cases as HS


# ---- constructors (no kernel runs) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,heads", [(128, 4), (192, 2), (128, 1), (128, 2)])
def test_attention_accepts_the_supported_head_sizes(dim, heads):
    a = Attention(dim, heads, st_mode="parallel")
    assert a.num_heads == heads and a.scale == (dim // heads) ** -0.5


@pytest.mark.parametrize("dim,heads", [(96, 2), (384, 2), (512, 2), (100, 3)])
def test_attention_names_the_supported_set_for_other_head_sizes(dim, heads):
    with pytest.raises(NotImplementedError, match=r"32, 64, 96, 128"):
        Attention(dim, heads)


def test_attention_still_rejects_an_unknown_mode_first():
    with pytest.raises(NotImplementedError, match="bogus"):
        Attention(128, 4, st_mode="bogus")
    with pytest.raises(NotImplementedError, match="bogus"):
        Attention(96, 2, st_mode="bogus")       # (the mode check comes before the head-size check)


@pytest.mark.parametrize("embed_dim,heads", [(128, 4), (192, 2), (128, 1)])
def test_maed_constructs_with_num_heads_other_than_dim_over_64(embed_dim, heads):
    m = maed_amd.MAED(num_blocks=1, num_heads=heads, embed_dim=embed_dim, img_size=64, hidden_dim=64)
    assert m.encoder.blocks[0].attn.num_heads == heads and m.encoder.blocks[0].fused


# ---- kernels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,impl", HS.ENGINES)
@pytest.mark.parametrize("D", HS.HEAD_SIZES)
@pytest.mark.parametrize("kind,size", HS.CASES)
def test_attn_seq_fwd_bwd(kind, size, D, name, dtype, impl):
    with patched():
        HS.run_case(kind, size, D, dtype, impl)


@pytest.mark.parametrize("kind,size", [("spatial", 130), ("temporal", 3), ("coupling", 3)])
def test_the_64_instantiation_agrees_with_the_existing_kernels(kind, size):
    """D = 64 through maed_attn_seq_* (the only place that instantiation is used) against attn_long.hip / attn_temporal.hip on the same inputs"""
    dtype = torch.bfloat16
    Fr, P, T, geo = HS.geometry(kind, size)
    qkv = q(rnd(Fr, P, 3 * 64 * HS.H, seed=9), dtype).to(dtype)
    do = q(rnd(Fr, P, 64 * HS.H, seed=10), dtype).to(dtype)
    with patched():
        o2, l2 = ops.attn_seq_fwd(qkv, HS.H, *geo)
        if kind == "temporal":
            o1, l1 = ops.attn_temporal_fwd(qkv, HS.H, T)
            g1 = ops.attn_temporal_bwd(qkv, o1, do, l1, HS.H, T)
        else:
            v = qkv.view(geo[0], geo[1], -1)
            o1, l1 = ops.attn_spatial_fwd(v, HS.H, L.IMPL_MFMA_LONG)
            g1 = ops.attn_spatial_bwd(v, o1, do.view(geo[0], geo[1], -1), l1, HS.H, impl=L.IMPL_MFMA_LONG)
        g2 = ops.attn_seq_bwd(qkv, o1.view_as(o2), do, l1.view_as(l2), HS.H, *geo)
    HS.close(o2.float(), o1.float().view_as(o2), **tol(dtype), what="o")
    HS.close(l2, l1.view_as(l2), rtol=1e-4, atol=2e-2, what="lse")
    HS.close(g2.float(), g1.float().view_as(g2), **tol(dtype, 0.5), what="dqkv")


def test_selectors_of_64_only_kernels_and_other_head_sizes_are_refused_with_a_message():
    qkv = rnd(2, 5, 3 * 64, seed=1).to(torch.bfloat16)
    with patched() as lib:
        for impl in (L.IMPL_MFMA, L.IMPL_X3, L.IMPL_X6):
            with pytest.raises(L.MaedHipError, match="head size 64 only"):
                ops.attn_seq_fwd(qkv, 2, 2, 5, 1, impl=impl)
        o, lse = ops.attn_seq_fwd(qkv, 2, 2, 5, 1)
        with pytest.raises(L.MaedHipError, match="head size 64 only"):
            ops.attn_seq_bwd(qkv, o, o, lse, 2, 2, 5, 1, impl=L.IMPL_MFMA)
        rc = lib.maed_attn_seq_fwd(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), 2, 5, 1, 2, 48, 0.1, L.BF16, L.IMPL_AUTO, None)
        assert rc == -5 and b"32, 64, 96, 128" in lib.maed_last_error()
    with pytest.raises(NotImplementedError):
        ops.attn_spatial_fwd(rnd(2, 5, 3 * 96, seed=1), 2)      # D = 48


def test_block_refuses_selectors_of_64_only_kernels_at_other_head_sizes():
    blk = Block(128, 4, mlp_ratio=1, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), st_mode="parallel", compute_dtype=torch.bfloat16, impl=L.IMPL_MFMA)
    with patched():
        with pytest.raises(L.MaedHipError, match="head size 64 only"):
            blk(rnd(6, 5, 128, seed=1).requires_grad_(True), 3)
        blk.impl = L.IMPL_VALU
        assert torch.isfinite(blk(rnd(6, 5, 128, seed=1), 3)).all()


# ---- the fused block ---------------------------------------------------------------------------------------------------------------------
def _block_and_reference(C, H, P, T, Fr, dtype, hidden_ratio=4):
    p = {k[len("encoder.blocks.0."):]: v for k, v in R.make_params(embed_dim=C, depth=1, hidden_dim=64, layers=(1, 1, 1), n_tokens=P, seed=3).items()
         if k.startswith("encoder.blocks.0.")}
    p = {k: v * (3.0 if k.endswith("weight") and v.dim() == 2 else 1.0) for k, v in p.items()}
    x, dy = rnd(Fr, P, C, seed=1), rnd(Fr, P, C, seed=2)
    pd = {k: v.double().requires_grad_(True) for k, v in p.items()}
    xr = x.double().requires_grad_(True)
    yref = R.block(xr, pd, "", H, T)
    yref.backward(dy.double())
    blk = Block(C, H, mlp_ratio=hidden_ratio, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), st_mode="parallel", compute_dtype=dtype, impl=0)
    blk.load_state_dict(p)
    return blk, x, dy, yref.detach(), xr.grad, {k: v.grad for k, v in pd.items()}


@pytest.mark.parametrize("dtype,f32_mode", [(torch.bfloat16, "exact"), (torch.float32, "exact"), (torch.float32, "bf16x3"), (torch.float32, "bf16x3+bwd:bf16")])
@pytest.mark.parametrize("C,H", [(128, 4), (192, 2), (128, 1)])
def test_ste_block_forward_backward_vs_oracle(C, H, dtype, f32_mode):
    """maed_ste_block_fwd / _bwd at head sizes 32 / 96 / 128 incl. every parameter gradient, at the bars of the D = 64 block test.  fp32 under "bf16x3": the GEMMs
    follow the mode, the attention contractions stay exact; "+bwd:bf16": no twin forward for these sizes -- the block takes the forward's engine"""
    Fr, P, T = 6, 5, 3
    blk, x, dy, yref, dxref, gref = _block_and_reference(C, H, P, T, Fr, dtype)
    xg = x.clone().requires_grad_(True)
    f32_mode, _, bwd = f32_mode.partition("+bwd:")
    old = ops.get_float32_matmul_precision()
    try:
        ops.set_float32_matmul_precision(f32_mode)
        ops.set_float32_backward_precision(bwd or None)
        twins = ops.TWIN_FORWARDS[0]
        with patched():
            y = blk(xg, T)
            y.backward(dy)
        assert ops.TWIN_FORWARDS[0] == twins
    finally:
        ops.set_float32_matmul_precision(old)
        ops.set_float32_backward_precision(None)
    f32 = dtype == torch.float32
    tl = (dict(rtol=3e-4, atol=3e-4) if f32_mode == "bf16x3" else dict(rtol=1e-4, atol=1e-4)) if f32 else dict(rtol=3e-2, atol=3e-2)
    HS.close(y.detach(), yref, **tl, what="y")
    if bwd:
        f32, tl = False, dict(rtol=3e-2, atol=3e-2)
    HS.close(xg.grad, dxref, **tl, what="dx")
    for name, prm in blk.named_parameters():
        ref = gref[name]
        scale = max(ref.abs().max().item(), 1e-3)
        assert prm.grad is not None, name
        HS.close(prm.grad, ref, rtol=1e-3 if f32 else 5e-2, atol=(1e-4 if f32 else 3e-2) * scale, what=name)


@pytest.mark.parametrize("C,H", [(128, 4), (192, 2)])
def test_fused_block_agrees_with_the_staged_composition(C, H):
    """the fused call against ste_modes.attention_parallel + the staged MLP of the same module (exact fp32: same kernels, another call sequence)"""
    from maed_amd import ste_modes
    Fr, P, T = 6, 5, 3
    blk, x, dy, _, _, _ = _block_and_reference(C, H, P, T, Fr, torch.float32)
    with patched():
        xg = x.clone().requires_grad_(True)
        y = blk(xg, T)
        y.backward(dy)
        fused = [y.detach().clone(), xg.grad.clone()] + [p_.grad.clone() for p_ in blk.parameters()]
        blk.zero_grad(set_to_none=True)
        xs = x.clone().requires_grad_(True)
        S, cd = ste_modes, blk.compute_dtype
        h = S.LayerNormFn.apply(xs.reshape(-1, C), blk.norm1.weight, blk.norm1.bias, blk.norm1.eps, cd).view(Fr, P, C)
        xm = xs + S.attention_parallel(blk.attn, h, T, cd, blk.impl)
        h = S.LayerNormFn.apply(xm.reshape(-1, C), blk.norm2.weight, blk.norm2.bias, blk.norm2.eps, cd)
        ys = xm + S.MlpFn.apply(h, blk.mlp.fc1.weight, blk.mlp.fc1.bias, blk.mlp.fc2.weight, blk.mlp.fc2.bias, blk.mlp._cache).view(Fr, P, C)
        ys.backward(dy)
        staged = [ys.detach(), xs.grad] + [p_.grad for p_ in blk.parameters()]
    for a, b in zip(fused, staged):
        HS.close(a, b, rtol=1e-4, atol=1e-4 * max(b.abs().max().item(), 1e-3), what="fused vs staged")


@pytest.mark.parametrize("mode", ["series", "vanilla", "temporal", "coupling"])
def test_staged_modes_at_head_size_32(mode):
    C, H, Fr, P, T = 128, 4, 6, 5, 3
    torch.manual_seed(11)
    blk = Block(C, H, mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), st_mode=mode, compute_dtype=torch.float32, impl=0)
    sd = {k: v.detach().double().requires_grad_(True) for k, v in blk.state_dict().items()}
    x, dy = rnd(Fr, P, C, seed=1), rnd(Fr, P, C, seed=2)
    xr = x.double().requires_grad_(True)
    yref = R.block(xr, sd, "", H, T, mode)
    yref.backward(dy.double())
    xg = x.clone().requires_grad_(True)
    with patched():
        y = blk(xg, T)
        y.backward(dy)
    HS.close(y.detach(), yref.detach(), rtol=1e-4, atol=1e-4, what=mode + " y")
    HS.close(xg.grad, xr.grad, rtol=1e-4, atol=1e-4, what=mode + " dx")
