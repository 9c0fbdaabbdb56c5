"""Head sizes 32 / 96 / 128 on the GPU: the kernel cases of tests/test_hostsim_head_sizes.py through the product library, the fused STE block at C = D*H
(forward + every gradient against fp64 autograd through the oracle, and against the staged composition of the same module), and a whole train step of a
MAED with num_heads = embed_dim / 32."""
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import maed_ref as R
from maed_amd import _lib as L
from maed_amd import ops

from _util import DEV, report, rnd
import _head_size_cases as HS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,dtype,impl", HS.ENGINES)
@pytest.mark.parametrize("D", HS.HEAD_SIZES)
@pytest.mark.parametrize("kind,size", HS.CASES)
def test_attn_seq_fwd_bwd(kind, size, D, name, dtype, impl):
    HS.run_case(kind, size, D, dtype, impl, device=DEV)


def test_the_64_instantiation_agrees_with_the_existing_kernels():
    dtype = torch.bfloat16
    qkv = rnd(2, 130, 3 * 128, seed=9).to(dtype).to(DEV)
    do = rnd(2, 130, 128, seed=10).to(dtype).to(DEV)
    o1, l1 = ops.attn_spatial_fwd(qkv, 2, L.IMPL_MFMA_LONG)
    g1 = ops.attn_spatial_bwd(qkv, o1, do, l1, 2, impl=L.IMPL_MFMA_LONG)
    o2, l2 = ops.attn_seq_fwd(qkv, 2, 2, 130, 1)
    g2 = ops.attn_seq_bwd(qkv, o1, do, l1, 2, 2, 130, 1)
    report("attn_seq D=64 o vs attn_long", o2.float(), o1.float(), rtol=2e-2, atol=2e-2)
    report("attn_seq D=64 lse vs attn_long", l2, l1, rtol=1e-4, atol=2e-2)
    report("attn_seq D=64 dqkv vs attn_long", g2.float(), g1.float(), rtol=2e-2, atol=1e-2)


def _block(C, H, dtype, state=None):
    from maed_amd.vision_transformer import Block
    blk = Block(C, H, mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), st_mode="parallel", compute_dtype=dtype, impl=0)
    if state is not None:
        blk.load_state_dict(state)
    return blk.to(DEV)


def _params(C, P):
    p = {k[len("encoder.blocks.0."):]: v for k, v in R.make_params(embed_dim=C, depth=1, hidden_dim=64, layers=(1, 1, 1), n_tokens=P, seed=3).items()
         if k.startswith("encoder.blocks.0.")}
    return {k: v * (3.0 if k.endswith("weight") and v.dim() == 2 else 1.0) for k, v in p.items()}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("Fr,P,C,H,T", [(6, 5, 128, 4, 3), (6, 5, 192, 2, 3), (4, 197, 256, 2, 2)])
def test_block_forward_backward_vs_oracle(Fr, P, C, H, T, dtype):
    """the fused block (bf16; and the exact fp32 engine) at head sizes 32 / 96 / 128 -- the last shape has the real token count -- at the bars of
    tests/test_gpu_model.py::test_block_forward_backward_vs_oracle"""
    p = _params(C, P)
    blk = _block(C, H, dtype, p)
    x, dy = rnd(Fr, P, C, seed=1), rnd(Fr, P, C, seed=2)
    pd = {k: v.double().requires_grad_(True) for k, v in p.items()}
    xr = x.double().requires_grad_(True)
    yref = R.block(xr, pd, "", H, T)
    yref.backward(dy.double())
    xg = x.to(DEV).requires_grad_(True)
    y = blk(xg, T)
    y.backward(dy.to(DEV))
    f32 = dtype == torch.float32
    tl = dict(rtol=1e-4, atol=1e-4) if f32 else dict(rtol=3e-2, atol=3e-2)
    tag = f"[{dtype},D{C // H},F{Fr} P{P}]"
    report(f"Block.forward{tag}", y, yref, **tl)
    report(f"Block.backward.dx{tag}", xg.grad, xr.grad, **tl)
    for name, prm in blk.named_parameters():
        ref = pd[name].grad
        scale = ref.abs().max().item()
        report(f"Block.backward.d[{name}]{tag}", prm.grad, ref, rtol=1e-3 if f32 else 5e-2, atol=(1e-4 if f32 else 3e-2) * max(scale, 1e-3))


@pytest.mark.parametrize("C,H", [(128, 4), (192, 2)])
def test_fused_block_agrees_with_the_staged_composition(C, H):
    """bf16: the fused call against ste_modes.attention_parallel + the staged MLP of the same module (same kernels for the attentions and the GEMMs; the staged
    form rounds the attention branch's output to fp32 through another epilogue): the bf16 bars of the block test"""
    from maed_amd import ste_modes as S
    Fr, P, T = 6, 5, 3
    blk = _block(C, H, torch.bfloat16, _params(C, P))
    x, dy = rnd(Fr, P, C, seed=1).to(DEV), rnd(Fr, P, C, seed=2).to(DEV)
    xg = x.clone().requires_grad_(True)
    y = blk(xg, T)
    y.backward(dy)
    fused = [("y", y.detach().clone()), ("dx", xg.grad.clone())] + [(n, p_.grad.clone()) for n, p_ in blk.named_parameters()]
    blk.zero_grad(set_to_none=True)
    xs = x.clone().requires_grad_(True)
    cd = blk.compute_dtype
    h = S.LayerNormFn.apply(xs.reshape(-1, C), blk.norm1.weight, blk.norm1.bias, blk.norm1.eps, cd).view(Fr, P, C)
    xm = xs + S.attention_parallel(blk.attn, h, T, cd, blk.impl)
    h = S.LayerNormFn.apply(xm.reshape(-1, C), blk.norm2.weight, blk.norm2.bias, blk.norm2.eps, cd)
    ys = xm + S.MlpFn.apply(h, blk.mlp.fc1.weight, blk.mlp.fc1.bias, blk.mlp.fc2.weight, blk.mlp.fc2.bias, blk.mlp._cache).view(Fr, P, C)
    ys.backward(dy)
    staged = [ys.detach(), xs.grad] + [p_.grad for p_ in blk.parameters()]
    for (name, a), b in zip(fused, staged):
        report(f"fused vs staged D{C // H} {name}", a, b, rtol=5e-2, atol=3e-2 * max(b.abs().max().item(), 1e-3))


def test_maed_train_step_with_head_size_32():
    """MAED(num_blocks=2, num_heads=4, embed_dim=128): forward, loss, backward, FusedAdam on the arena -- finite, non-zero gradients on every parameter"""
    import maed_amd
    from maed_amd.ddp import FusedAdam, GradBucketer, ParamArena
    torch.manual_seed(3)
    m = maed_amd.MAED(num_blocks=2, num_heads=4, embed_dim=128, hidden_dim=64, img_size=64, compute_dtype=torch.bfloat16).to(DEV)
    m.train()
    arena = ParamArena(m)
    bucketer = GradBucketer(arena, m, bucket_bytes=1 << 20)
    opt = FusedAdam(arena, lr=1e-3, weight_decay=1e-5, bucketer=bucketer)
    clip = rnd(2, 4, 3, 64, 64, seed=11).to(DEV)
    tgt = rnd(2, 4, 49, 3, seed=12).to(DEV) * 0.1
    opt.zero_grad()
    out = m(clip)
    loss = ((out["kp_3d"] - tgt) ** 2).mean() + 1e-3 * (out["theta"] ** 2).mean()
    loss.backward()
    bad = [n for n, p_ in m.named_parameters() if p_.requires_grad and (p_.grad is None or not torch.isfinite(p_.grad).all() or not (p_.grad != 0).any())]
    assert not bad, bad
    opt.step()
    torch.cuda.synchronize()
    assert np.isfinite(loss.item())
    assert all(torch.isfinite(p_).all() for p_ in m.parameters())
    assert L.device_faults() == 0
