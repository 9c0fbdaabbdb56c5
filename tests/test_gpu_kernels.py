"""GPU parity tests, kernel level: every libmaed_hip entry point against the CPU oracle
(oracle/maed_ref.py, pinned to the reference by tests/golden) on the same seeded inputs.

Tolerances: f32 kernels 2e-5 (exact-f32 arithmetic, different summation order); bf16 kernels are
compared with the oracle evaluated in fp32 on the SAME bf16-rounded inputs, so what remains is the
bf16 rounding of outputs / probabilities (2^-8 relative).  Integer/index work is bit-exact.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import maed_ref as R

pytestmark = pytest.mark.gpu

from _util import DEV, note, q, report, rnd, tol  # noqa: E402


def _ops():
    from maed_amd import ops, _lib
    return ops, _lib


DTYPES = [torch.float32, torch.bfloat16]


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C", [(37, 128), (197 * 3, 512), (64, 768)])
def test_layernorm_fwd_bwd(dtype, rows, C):
    ops, _ = _ops()
    x = rnd(rows, C, seed=1) * 2 + 0.3
    g, b = 1 + 0.2 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
    y, mean, rstd = ops.layernorm_fwd(x.to(DEV), g.to(DEV), b.to(DEV), dtype)
    ref = R.layer_norm(x, g, b)
    report(f"layernorm_fwd[{dtype},{rows}x{C}]", y.float(), ref, **tol(dtype, 4))
    dy = q(rnd(rows, C, seed=4), dtype)
    dres = rnd(rows, C, seed=5)
    xr = x.double().requires_grad_(True)
    gr, br = g.double().requires_grad_(True), b.double().requires_grad_(True)
    R.layer_norm(xr, gr, br).backward(dy.double())
    dx, dg, db = ops.layernorm_bwd(dy.to(DEV).to(dtype), x.to(DEV), g.to(DEV), mean, rstd, dres=dres.to(DEV))
    report(f"layernorm_bwd.dx[{dtype},{rows}x{C}]", dx, xr.grad + dres.double(), rtol=2e-5, atol=1e-4)
    report(f"layernorm_bwd.dgamma[{dtype}]", dg, gr.grad, rtol=1e-4, atol=1e-3)
    report(f"layernorm_bwd.dbeta[{dtype}]", db, br.grad, rtol=1e-4, atol=1e-3)


def test_layernorm_strided_rows():
    ops, _ = _ops()
    x = rnd(6, 5, 128, seed=7)
    g, b = 1 + 0.2 * rnd(128, seed=2), 0.1 * rnd(128, seed=3)
    y, _, _ = ops.layernorm_fwd(x.to(DEV), g.to(DEV), b.to(DEV), torch.float32, row_stride=5 * 128, rows=6)
    report("layernorm_fwd[cls rows, stride P*C]", y, R.layer_norm(x[:, 0], g, b), **tol(torch.float32, 4))


# ---------------------------------------------------------------------------------------------
GEMM_CASES = [("f32-valu", torch.float32, 1), ("bf16-valu", torch.bfloat16, 1), ("bf16-mfma", torch.bfloat16, 2), ("bf16-auto", torch.bfloat16, 0),
              ("bf16-glds1", torch.bfloat16, 3)]


@pytest.mark.parametrize("name,dtype,impl", GEMM_CASES)
@pytest.mark.parametrize("M,N,K", [(300, 100, 64), (197 * 4, 384, 128), (130, 512, 2048), (128, 128, 64)])
def test_gemm_epilogues(name, dtype, impl, M, N, K):
    ops, L = _ops()
    A, B = q(rnd(M, K, seed=1), dtype), q(rnd(N, K, seed=2, scale=K ** -0.5), dtype)
    bias = rnd(N, seed=3)
    Ad, Bd, bd = A.to(DEV).to(dtype), B.to(DEV).to(dtype), bias.to(DEV)
    ref = A.double() @ B.double().t()
    t = tol(dtype, 2)
    out = ops.gemm_nt(Ad, Bd, L.EPI_STORE, bias=bd, impl=impl)
    report(f"gemm[{name},STORE,{M}x{N}x{K}]", out.float(), ref + bias.double(), **t)
    out = ops.gemm_nt(Ad, Bd, L.EPI_STORE_F32, bias=bd, impl=impl)
    report(f"gemm[{name},STORE_F32]", out, ref + bias.double(), rtol=2e-5, atol=1e-4)
    act, pre = ops.gemm_nt(Ad, Bd, L.EPI_GELU, bias=bd, impl=impl)
    report(f"gemm[{name},GELU.pre]", pre.float(), ref + bias.double(), **t)
    report(f"gemm[{name},GELU.act]", act.float(), R.gelu(pre.float().cpu().double()), **t)
    res = rnd(M, N, seed=4)
    out = ops.gemm_nt(Ad, Bd, L.EPI_RESID_F32, bias=bd, aux=res.to(DEV), impl=impl)
    report(f"gemm[{name},RESID_F32]", out, ref + bias.double() + res.double(), rtol=2e-5, atol=1e-4)
    pre_in = q(rnd(M, N, seed=5), dtype)
    out = ops.gemm_nt(Ad, Bd, L.EPI_MUL_DGELU, aux=pre_in.to(DEV).to(dtype), impl=impl)
    xg = pre_in.double().requires_grad_(True)
    R.gelu(xg).sum().backward()
    report(f"gemm[{name},MUL_DGELU]", out.float(), ref * xg.grad, **t)
    out = ops.gemm_nt(Ad, Bd, L.EPI_TANH, bias=bd, impl=impl)
    report(f"gemm[{name},TANH]", out.float(), torch.tanh(ref + bias.double()), **t)
    acc = rnd(M, N, seed=6).to(DEV)
    acc0 = acc.clone()
    splitk = 4 if K >= 256 else 1
    ops.gemm_nt(Ad, Bd, L.EPI_ATOMIC_F32, out=acc, splitk=splitk, impl=impl)
    report(f"gemm[{name},ATOMIC_F32,splitk={splitk}]", acc, acc0.cpu().double() + ref, rtol=2e-5, atol=2e-4)


@pytest.mark.parametrize("M,N,K", [(300, 264, 128), (197 * 8, 512, 192), (1000, 1536, 512), (777, 256, 2048), (256, 512, 320)])
def test_gemm_256_pipelined_tiles(M, N, K):
    """csrc/gemm256.hip (256x256x64 tiles, half-tile LDS-DMA ring with counted vmcnt, staggered wave groups) against the fp64 oracle and
    BITWISE against the 128x128 kernel (same k order, fp32 accumulation): ragged M / N edges, 2 ... 32 K tiles, even and odd tile counts
    (both drains), every fused epilogue it carries."""
    ops, L = _ops()
    dtype = torch.bfloat16
    A, B = q(rnd(M, K, seed=11), dtype), q(rnd(N, K, seed=12, scale=K ** -0.5), dtype)
    bias = rnd(N, seed=13)
    Ad, Bd, bd = A.to(DEV).to(dtype), B.to(DEV).to(dtype), bias.to(DEV)
    ref = A.double() @ B.double().t()
    t = tol(dtype, 2)
    out = ops.gemm_nt(Ad, Bd, L.EPI_STORE, bias=bd, impl=L.IMPL_MFMA_256)
    report(f"gemm256[STORE,{M}x{N}x{K}]", out.float(), ref + bias.double(), **t)
    assert torch.equal(out, ops.gemm_nt(Ad, Bd, L.EPI_STORE, bias=bd, impl=3))
    res = rnd(M, N, seed=14)
    out = ops.gemm_nt(Ad, Bd, L.EPI_RESID_F32, bias=bd, aux=res.to(DEV), impl=L.IMPL_MFMA_256)
    report("gemm256[RESID_F32]", out, ref + bias.double() + res.double(), rtol=2e-5, atol=1e-4)
    act, pre = ops.gemm_nt(Ad, Bd, L.EPI_GELU, bias=bd, impl=L.IMPL_MFMA_256)
    report("gemm256[GELU.pre]", pre.float(), ref + bias.double(), **t)
    report("gemm256[GELU.act]", act.float(), R.gelu(pre.float().cpu().double()), **t)
    pre_in = q(rnd(M, N, seed=15), dtype)
    out = ops.gemm_nt(Ad, Bd, L.EPI_MUL_DGELU, aux=pre_in.to(DEV).to(dtype), impl=L.IMPL_MFMA_256)
    assert torch.equal(out, ops.gemm_nt(Ad, Bd, L.EPI_MUL_DGELU, aux=pre_in.to(DEV).to(dtype), impl=3))
    out = ops.gemm_nt(Ad, Bd, L.EPI_STORE_F32, bias=bd, impl=L.IMPL_MFMA_256)
    report("gemm256[STORE_F32]", out, ref + bias.double(), rtol=2e-5, atol=1e-4)


def test_gemm_256_race_screen_at_cfg3_shapes():
    """the benchmarked shapes (M = 128 frames x 197 tokens): 25 back-to-back launches each, every one bit-identical to the 128x128 kernel's
    result.  A screen, not a proof -- the reads are placed by the vmcnt / barrier count (gemm256.hip header) -- but an LDS-DMA landing late
    or a slot re-targeted early shows up here as a differing tile."""
    ops, L = _ops()
    M = 128 * 197
    for N, K in [(512, 2048), (512, 1536), (512, 512), (1536, 512)]:
        A = (torch.randn(M, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(K + N))).bfloat16()
        B = (torch.randn(N, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(N)) * K ** -0.5).bfloat16()
        want = ops.gemm_nt(A, B, L.EPI_STORE, impl=3)
        bad = 0
        for _ in range(25):
            bad += int(not torch.equal(ops.gemm_nt(A, B, L.EPI_STORE, impl=L.IMPL_MFMA_256), want))
        assert bad == 0, f"{bad}/25 launches of the 256x256 kernel differ at N={N} K={K}"


def test_gemm_mfma_rejects_bad_k():
    ops, L = _ops()
    A = torch.zeros(64, 48, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(L.MaedHipError):
        ops.gemm_nt(A, A, L.EPI_STORE, impl=L.IMPL_MFMA)


@pytest.mark.parametrize("din,dout", [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)])
def test_transpose_cast(din, dout):
    ops, _ = _ops()
    x = q(rnd(197 * 3 + 1, 200, seed=1), din)
    cs = torch.zeros(200, device=DEV)
    xt, xc = ops.transpose_cast(x.to(DEV).to(din), dout, want_c=True, colsum=cs)
    M = x.shape[0]
    assert xt.shape == (200, (M + 63) // 64 * 64)
    assert torch.equal(xt[:, :M].float().cpu(), x.to(dout).float().t()), "transpose must be exact"
    assert torch.count_nonzero(xt[:, M:]) == 0, "padding must be zero"
    assert torch.equal(xc.float().cpu(), x.to(dout).float())
    report(f"transpose_cast.colsum[{din}->{dout}]", cs, x.double().sum(0), rtol=1e-5, atol=1e-3)


# ---------------------------------------------------------------------------------------------
def _qkv(Fr, P, H, dtype, seed=0):
    return q(rnd(Fr, P, 3 * 64 * H, seed=seed), dtype)


ATTN_CASES = [("f32-valu", torch.float32, 1), ("bf16-valu", torch.bfloat16, 1), ("bf16-mfma", torch.bfloat16, 2), ("bf16-auto", torch.bfloat16, 0)]   # auto = the K/V-tiled kernels where they measured faster


@pytest.mark.parametrize("name,dtype,impl", ATTN_CASES)
@pytest.mark.parametrize("Fr,P,H", [(4, 5, 2), (3, 197, 2), (2, 257, 3), (2, 32, 1), (2, 33, 1)])
def test_attn_spatial_fwd(name, dtype, impl, Fr, P, H):
    ops, _ = _ops()
    qkv = _qkv(Fr, P, H, dtype, seed=P)
    qq, kk, vv = R.split_qkv(qkv.double(), H)
    ref = R.attention_spatial(qq, kk, vv, 64 ** -0.5)
    lse_ref = torch.logsumexp((qq @ kk.transpose(-2, -1)) * 64 ** -0.5, dim=-1)
    o, lse = ops.attn_spatial_fwd(qkv.to(DEV).to(dtype), H, impl)
    report(f"attn_spatial_fwd[{name},F{Fr} P{P} H{H}]", o.float(), ref, **tol(dtype))
    report(f"attn_spatial_fwd.lse[{name},P{P}]", lse, lse_ref, rtol=1e-4, atol=1e-3 if dtype == torch.float32 else 2e-2)


def test_attn_spatial_fwd_mfma_spiked_scores():
    """online-softmax rescale path: one key dominates late in the sequence (large running-max jump)."""
    ops, _ = _ops()
    Fr, P, H = 2, 197, 1
    qkv = rnd(Fr, P, 192, seed=11)
    qkv[:, 150, 64:128] = qkv[:, 3, 0:64] * 6.0   # key 150 aligned with query 3
    qkv[:, 40, 64:128] = qkv[:, 100, 0:64] * 4.0
    qkv = q(qkv, torch.bfloat16)
    qq, kk, vv = R.split_qkv(qkv.double(), H)
    ref = R.attention_spatial(qq, kk, vv, 64 ** -0.5)
    o, _ = ops.attn_spatial_fwd(qkv.to(DEV).bfloat16(), H, 2)
    report("attn_spatial_fwd[bf16-mfma, spiked]", o.float(), ref, **tol(torch.bfloat16))


@pytest.mark.parametrize("name,dtype,impl", ATTN_CASES)
@pytest.mark.parametrize("Fr,P,H", [(2, 5, 2), (2, 197, 2), (1, 257, 1), (1, 64, 1)])
def test_attn_spatial_bwd(name, dtype, impl, Fr, P, H):
    ops, _ = _ops()
    qkv = _qkv(Fr, P, H, dtype, seed=3)
    do = q(rnd(Fr, P, 64 * H, seed=4), dtype)
    x = qkv.double().requires_grad_(True)
    qq, kk, vv = R.split_qkv(x, H)
    oref = R.attention_spatial(qq, kk, vv, 64 ** -0.5)
    oref.backward(do.double())
    qd = qkv.to(DEV).to(dtype)
    o, lse = ops.attn_spatial_fwd(qd, H, 1)
    dqkv = ops.attn_spatial_bwd(qd, o, do.to(DEV).to(dtype), lse, H, impl=impl)
    C = 64 * H
    for nm, sl in (("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C))):
        report(f"attn_spatial_bwd.{nm}[{name},P{P}]", dqkv[..., sl].float(), x.grad[..., sl], **tol(dtype, 0.5))
    base = torch.ones_like(dqkv)
    dq2 = ops.attn_spatial_bwd(qd, o, do.to(DEV).to(dtype), lse, H, dqkv=base.clone(), accumulate=True, impl=impl)
    report(f"attn_spatial_bwd.accumulate[{name}]", dq2.float(), x.grad + 1.0, **tol(dtype, 0.5))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,T,P,H", [(2, 3, 5, 2), (2, 16, 50, 2), (1, 1, 7, 1), (1, 64, 9, 1)])
def test_attn_temporal_fwd_bwd(dtype, N, T, P, H):
    ops, _ = _ops()
    Fr = N * T
    qkv = _qkv(Fr, P, H, dtype, seed=5)
    do = q(rnd(Fr, P, 64 * H, seed=6), dtype)
    x = qkv.double().requires_grad_(True)
    qq, kk, vv = R.split_qkv(x, H)
    oref = R.attention_temporal(qq, kk, vv, T, 64 ** -0.5)
    oref.backward(do.double())
    qd = qkv.to(DEV).to(dtype)
    o, lse = ops.attn_temporal_fwd(qd, H, T)
    report(f"attn_temporal_fwd[{dtype},N{N} T{T} P{P}]", o.float(), oref, **tol(dtype))
    dqkv = ops.attn_temporal_bwd(qd, o, do.to(DEV).to(dtype), lse, H, T)
    report(f"attn_temporal_bwd[{dtype},T{T}]", dqkv.float(), x.grad, **tol(dtype, 0.5))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_st_mix_fwd_bwd(dtype):
    ops, _ = _ops()
    Fr, P, C = 6, 37, 128
    xs, xt = q(rnd(Fr, P, C, seed=1), dtype), q(rnd(Fr, P, C, seed=2), dtype)
    logits = rnd(Fr, 2 * C, seed=3)
    means = ops.st_colmean(xs.to(DEV).to(dtype), xt.to(DEV).to(dtype))
    report(f"st_colmean[{dtype}]", means.float(), torch.cat([xs, xt], -1).double().mean(1), **tol(dtype))
    a = xs.double().requires_grad_(True)
    b = xt.double().requires_grad_(True)
    lg = logits.double().requires_grad_(True)
    alpha = lg.reshape(Fr, 1, C, 2).softmax(-1)
    ref = b * alpha[:, :, :, 1] + a * alpha[:, :, :, 0]
    mix = ops.st_mix_fwd(xs.to(DEV).to(dtype), xt.to(DEV).to(dtype), logits.to(DEV))
    report(f"st_mix_fwd[{dtype}]", mix.float(), ref, **tol(dtype))
    dmix = q(rnd(Fr, P, C, seed=4), dtype)
    ref.backward(dmix.double())
    W = rnd(2 * C, 2 * C, seed=5, scale=0.05)  # stands in for the ts_attn weight: dmeans = dlogits @ W
    dmeans_ref = lg.grad @ W.double()
    dxs, dxt, dlog = ops.st_mix_bwd(dmix.to(DEV).to(dtype), xs.to(DEV).to(dtype), xt.to(DEV).to(dtype), logits.to(DEV),
                                    lambda dl: (dl.float() @ W.to(DEV)).to(dtype))
    report(f"st_mix_bwd.dlogits[{dtype}]", dlog.float(), lg.grad, **tol(dtype, 2))
    report(f"st_mix_bwd.dx_s[{dtype}]", dxs.float(), a.grad + dmeans_ref[:, None, :C] / P, **tol(dtype))
    report(f"st_mix_bwd.dx_t[{dtype}]", dxt.float(), b.grad + dmeans_ref[:, None, C:] / P, **tol(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_embed_add_fwd_bwd(dtype):
    ops, _ = _ops()
    N, T, P, C = 2, 3, 5, 128
    patch = q(rnd(N * T, P - 1, C, seed=1), dtype)
    prm = {"cls_token": rnd(1, 1, C, seed=2), "pos_embed": rnd(1, P, C, seed=3), "temp_embed": rnd(1, 16, 1, C, seed=4)}
    leaves = {k: v.double().requires_grad_(True) for k, v in prm.items()}
    pt = patch.double().requires_grad_(True)
    ref = R.embed_tokens(pt, leaves, "", T)
    dtok = rnd(N * T, P, C, seed=5)
    ref.backward(dtok.double())
    args = [t.to(DEV).requires_grad_(True) for t in (patch.to(dtype), prm["cls_token"], prm["pos_embed"], prm["temp_embed"])]
    tok = ops.EmbedAddFn.apply(*args, T)
    report(f"embed_add_fwd[{dtype}]", tok, ref, rtol=1e-6, atol=1e-6)
    tok.backward(dtok.to(DEV))
    report(f"embed_add_bwd.dpatch[{dtype}]", args[0].grad.float(), pt.grad, **tol(dtype))
    report(f"embed_add_bwd.dcls[{dtype}]", args[1].grad, leaves["cls_token"].grad, rtol=1e-5, atol=1e-5)
    report(f"embed_add_bwd.dpos[{dtype}]", args[2].grad, leaves["pos_embed"].grad, rtol=1e-5, atol=1e-5)
    report(f"embed_add_bwd.dtemp[{dtype}]", args[3].grad, leaves["temp_embed"].grad, rtol=1e-5, atol=1e-5)


def test_adam_matches_torch():
    ops, _ = _ops()
    n = 1000 * 4 + 3
    p0, g = rnd(n, seed=1), rnd(n, seed=2)
    ref = torch.nn.Parameter(p0.clone().double())
    opt = torch.optim.Adam([ref], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
    p = p0.to(DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    shadow = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    for step in range(1, 4):
        gs = g * step
        ref.grad = (gs / 2).double()
        opt.step()
        ops.adam_step(p, gs.to(DEV), m, v, shadow, 1e-3, 0.9, 0.999, 1e-8, 1e-5, step, gscale=0.5)
    report("adam_step[3 steps, gscale=0.5]", p, ref.data, rtol=1e-5, atol=1e-6)
    assert torch.equal(shadow.float(), p.bfloat16().float())


# ---------------------------------------------------------------------------------------------
def test_ktd_chain_and_rot6d(golden):
    ops, L = _ops()
    fx = golden("g6_ktd")
    from maed_amd.ktd import KTD
    dec = KTD(feat_dim=128, hidden_dim=64).eval()
    sd = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("sd.")}
    missing, unexpected = dec.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("smpl.") for k in missing)
    dec = dec.to(DEV)
    with torch.no_grad():
        pose, shape, cam = dec._head_hip(torch.from_numpy(fx["x"]).to(DEV))
    report("ktd_head.pose6d (golden g6)", pose, torch.from_numpy(fx["pose6d"]), rtol=1e-4, atol=1e-5)
    report("ktd_head.shape (golden g6)", shape, torch.from_numpy(fx["shape"]), rtol=1e-4, atol=1e-5)
    report("ktd_head.cam (golden g6)", cam, torch.from_numpy(fx["cam"]), rtol=1e-4, atol=1e-5)
    with torch.no_grad():
        o = dec(torch.from_numpy(fx["x"]).to(DEV), seqlen=3)
        o17 = dec(torch.from_numpy(fx["x"]).to(DEV), seqlen=3, J_regressor=R.make_synthetic_smpl(0)["J_regressor_h36m"].to(DEV))
    for k in ("theta", "rotmat", "kp_3d"):
        report(f"KTD.forward.{k} (golden g6)", o[k], torch.from_numpy(fx[k]), rtol=1e-3, atol=1e-5)
    report("KTD.forward.kp_2d (golden g6)", o["kp_2d"], torch.from_numpy(fx["kp_2d"]), rtol=1e-3, atol=1e-4)
    report("KTD.forward.verts (golden g6)", o["verts"][:, ::53], torch.from_numpy(fx["verts_sub"]), rtol=1e-3, atol=1e-5)
    report("KTD.forward.kp_3d_h36m (golden g6)", o17["kp_3d"], torch.from_numpy(fx["kp_3d_h36m"]), rtol=1e-3, atol=1e-5)
    report("KTD.forward.kp_2d_h36m (golden g6)", o17["kp_2d"], torch.from_numpy(fx["kp_2d_h36m"]), rtol=1e-3, atol=1e-4)


def test_rot6d_pose_golden(golden):
    ops, L = _ops()
    fx = golden("g7_geometry")
    r6 = torch.from_numpy(fx["rot6d"]).to(DEV)
    n = r6.shape[0]
    rot = torch.empty(n, 3, 3, device=DEV)
    aa = torch.empty(n, 3, device=DEV)
    ops.check(L.lib().maed_rot6d_pose_fwd(r6.data_ptr(), rot.data_ptr(), aa.data_ptr(), n, torch.cuda.current_stream().cuda_stream))
    report("rot6d_to_rotmat (golden g7)", rot, torch.from_numpy(fx["rotmat"]), rtol=1e-5, atol=1e-6)
    report("rotmat_to_angle_axis (golden g7)", aa, torch.from_numpy(fx["angle_axis"][:n]), rtol=1e-4, atol=1e-5)


def test_smpl_lbs_and_joint_gather_bit_exact():
    ops, L = _ops()
    from maed_amd.smpl import SMPL
    sp = R.make_synthetic_smpl(0)
    smpl = SMPL().to(DEV)
    Fr = 7
    betas = rnd(Fr, 10, seed=1)
    rot = R.rot6d_to_rotmat(rnd(Fr * 24, 6, seed=2)).reshape(Fr, 24, 3, 3)
    verts_ref, j24_ref = R.smpl_lbs(betas.double(), rot.double(), {k: (v.double() if v.is_floating_point() else v) for k, v in sp.items()})
    verts, j24 = smpl.lbs_hip(betas.to(DEV), rot.to(DEV))
    report("smpl_lbs.verts", verts, verts_ref, rtol=1e-4, atol=1e-5)
    report("smpl_lbs.joints24", j24, j24_ref, rtol=1e-4, atol=1e-5)
    extra = smpl.joint_regress_hip(smpl.J_regressor_extra, verts)
    report("joint_regress[J=9, f32 MFMA]", extra, torch.einsum("bik,ji->bjk", verts.cpu().double(), sp["J_regressor_extra"].double()), rtol=1e-4, atol=1e-5)
    h36m = smpl.joint_regress_hip(sp["J_regressor_h36m"].to(DEV), verts)
    report("joint_regress[J=17, f32 MFMA]", h36m, torch.einsum("bik,ji->bjk", verts.cpu().double(), sp["J_regressor_h36m"].double()), rtol=1e-4, atol=1e-5)
    # (both regressors are sparse: the calls above took the CSR kernel; the dense f32-MFMA kernel on a regressor that is not)
    assert smpl.regressor_csr(smpl.J_regressor_extra) is not None
    dense = (torch.rand(9, 6890, generator=torch.Generator().manual_seed(3)) / 6890).to(DEV)
    assert smpl.regressor_csr(dense) is None
    report("joint_regress[J=9, dense, f32 MFMA]", smpl.joint_regress_hip(dense, verts), torch.einsum("bik,ji->bjk", verts.cpu().double(), dense.cpu().double()), rtol=1e-4, atol=1e-5)
    cam = torch.tensor([[0.9, 0.1, -0.2]]).repeat(Fr, 1).to(DEV)
    kp3d = torch.empty(Fr, 49, 3, device=DEV)
    kp2d = torch.empty(Fr, 49, 2, device=DEV)
    ops.check(L.lib().maed_smpl_joints_project_fwd(j24.data_ptr(), verts.data_ptr(), smpl.extra_vertex_ids.data_ptr(), extra.data_ptr(),
                                                   smpl.joint_map.data_ptr(), cam.data_ptr(), None, 0, kp3d.data_ptr(), kp2d.data_ptr(), Fr,
                                                   torch.cuda.current_stream().cuda_stream))
    j54 = torch.cat([j24, verts[:, sp["extra_vertex_ids"].to(DEV)], extra], 1)
    expect = j54[:, torch.tensor(R.JOINT_MAP_49, device=DEV)]
    assert torch.equal(kp3d, expect), "joint_map gather must be bit-exact"
    report("projection", kp2d, R.projection(expect.cpu(), cam.cpu()), rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------
# backbone helpers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,C,H,W", [(3, 64, 9, 7), (2, 256, 14, 14), (2, 1024, 5, 5), (2, 128, 28, 28)])
@pytest.mark.parametrize("res,relu", [(False, True), (True, True), (False, False), (True, False)])
def test_groupnorm_fused(dtype, N, C, H, W, res, relu):
    ops, _ = _ops()
    x = q(rnd(N, C, H, W, seed=1) * 1.5 + 0.2, dtype)
    r = q(rnd(N, C, H, W, seed=2), dtype) if res else None
    g, b = 1 + 0.2 * rnd(C, seed=3), 0.1 * rnd(C, seed=4)
    dy = q(rnd(N, C, H, W, seed=5), dtype)
    xd = x.double().requires_grad_(True)
    rd = r.double().requires_grad_(True) if res else None
    gd, bd = g.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.group_norm(xd, 32, gd, bd, 1e-5)
    if res:
        ref = ref + rd
    if relu:
        ref = F.relu(ref)
    ref.backward(dy.double())
    cl = lambda t: t.to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
    xg = cl(x).requires_grad_(True)
    rg = cl(r).requires_grad_(True) if res else None
    gg, bg = g.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = ops.GroupNormFn.apply(xg, rg, gg, bg, 1e-5, relu, False)
    y.backward(cl(dy))
    tag = f"[{dtype},{N}x{C}x{H}x{W},res={res},relu={relu}]"
    t = tol(dtype, 4)
    report(f"groupnorm_fwd{tag}", y.float(), ref, **t)
    report(f"groupnorm_bwd.dx{tag}", xg.grad.float(), xd.grad, **tol(dtype, 2))
    if res:
        report(f"groupnorm_bwd.dres{tag}", rg.grad.float(), rd.grad, **tol(dtype, 2))
    scale = max(1.0, gd.grad.abs().max().item())
    report(f"groupnorm_bwd.dgamma{tag}", gg.grad, gd.grad, rtol=1e-4 if dtype == torch.float32 else 2e-2, atol=(1e-4 if dtype == torch.float32 else 3e-2) * scale)
    report(f"groupnorm_bwd.dbeta{tag}", bg.grad, bd.grad, rtol=1e-4 if dtype == torch.float32 else 2e-2, atol=(1e-4 if dtype == torch.float32 else 3e-2) * scale)


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_std_batched(dtype):
    ops, _ = _ops()

    class Owner:
        _pending_backwards = 0
        grads_ready = None

        def __init__(self, ws):
            self.ws = ws

        def fused_parameters(self):
            return self.ws

        conv_weights = fused_parameters

    shapes = [(64, 3, 7, 7), (16, 32, 1, 1), (40, 24, 3, 3), (8, 256, 1, 1)]
    ws = [torch.nn.Parameter((rnd(*s, seed=i) * 0.3 + 0.05).to(DEV)) for i, s in enumerate(shapes)]
    owner = Owner(ws)
    outs = ops.WeightStdFn.apply(owner, dtype, 1e-5, *ws)
    gs = [q(rnd(*s, seed=10 + i), dtype) for i, s in enumerate(shapes)]
    torch.autograd.backward(outs, [g.to(DEV).to(dtype) for g in gs])
    for i, (w, o, g) in enumerate(zip(ws, outs, gs)):
        wd = w.detach().cpu().double().requires_grad_(True)
        std, mean = torch.std_mean(wd, dim=[1, 2, 3], keepdim=True, unbiased=False)
        ref = (wd - mean) / (std + 1e-5)
        ref.backward(g.double())
        assert o.shape == w.shape and o.is_contiguous(memory_format=torch.channels_last) or w.shape[2] == 1
        report(f"weight_std_fwd[{dtype},{shapes[i]}]", o.float(), ref, **tol(dtype, 2))
        report(f"weight_std_bwd[{dtype},{shapes[i]}]", w.grad, wd.grad, rtol=1e-4 if dtype == torch.float32 else 2e-2,
               atol=(1e-4 if dtype == torch.float32 else 2e-2) * wd.grad.abs().max().item())


@pytest.mark.parametrize("M,N,K", [(300, 136, 72), (197 * 8, 512, 256), (64, 128, 128), (1000, 1536, 512), (37, 8, 8),
                                   (197 * 128, 1536, 512), (197 * 128, 512, 2048)])                                        # the last two: cfg3 STE shapes
def test_gemm_tn_wgrad(M, N, K):
    """dW += Y^T X and db += colsum(Y) straight from row-major bf16 operands (register 8x8 transposes, split-M atomics)"""
    ops, _ = _ops()
    Y = q(rnd(M, N, seed=1), torch.bfloat16)
    X = q(rnd(M, K, seed=2), torch.bfloat16)
    dW0, db0 = rnd(N, K, seed=3), rnd(N, seed=4)
    dW, db = dW0.clone().to(DEV), db0.clone().to(DEV)
    ops.gemm_tn_wgrad(Y.to(DEV).bfloat16(), X.to(DEV).bfloat16(), dW=dW, dbias=db)
    ref = dW0.double() + Y.double().t() @ X.double()
    report(f"gemm_tn_wgrad.dW[{M}x{N}x{K}]", dW, ref, rtol=2e-5, atol=2e-5 * max(1.0, M ** 0.5))
    report(f"gemm_tn_wgrad.db[{M}x{N}]", db, db0.double() + Y.double().sum(0), rtol=2e-5, atol=2e-5 * max(1.0, M ** 0.5))


@pytest.mark.parametrize("N,I,O,H,W", [(3, 64, 256, 14, 14), (2, 256, 512, 14, 14), (2, 128, 64, 7, 9), (5, 1024, 256, 14, 14)])
def test_conv1x1_as_gemm(N, I, O, H, W):
    """ops.Conv1x1Fn (the 1x1 stride-1 convolutions of the backbone on maed_gemm_nt / maed_gemm_tn_wgrad) vs fp64 conv2d"""
    ops, _ = _ops()
    x = q(rnd(N, I, H, W, seed=1), torch.bfloat16)
    w = q(rnd(O, I, 1, 1, seed=2, scale=I ** -0.5), torch.bfloat16)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ref = F.conv2d(xd, wd)
    dy = q(rnd(*ref.shape, seed=3), torch.bfloat16)
    ref.backward(dy.double())
    xg = x.to(DEV).bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wg = w.to(DEV).bfloat16().requires_grad_(True)
    wt = wg.detach().reshape(O, I).t().contiguous()
    dw = torch.ones(O, I, dtype=torch.float32, device=DEV)            # the kernel ACCUMULATES: start from ones
    y = ops.Conv1x1Fn.apply(xg, wg, wt, dw)
    y.backward(dy.to(DEV).bfloat16())
    tag = f"[{N}x{I}->{O},{H}x{W}]"
    report(f"conv1x1 fwd{tag}", y.float(), ref, **tol(torch.bfloat16, 2))
    report(f"conv1x1 dx{tag}", xg.grad.float(), xd.grad, **tol(torch.bfloat16, 2))
    report(f"conv1x1 dw{tag} (fp32 accumulator)", dw - 1.0, wd.grad.reshape(O, I), rtol=2e-3, atol=2e-3 * wd.grad.abs().max().item())
    assert wg.grad is None, "the weight gradient travels through the fp32 accumulator, not autograd"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,C,H,W", [(3, 64, 112, 112), (2, 8, 7, 9), (1, 16, 16, 16)])
def test_maxpool_same_3x3s2(dtype, N, C, H, W):
    """ops.MaxPool3s2SameFn (no padded copy forward, gather backward) == F.max_pool2d on the -inf padded tensor (resnetv2.py:61-72),
    bit-exact including ATen's tie rule on the ReLU zeros"""
    ops, _ = _ops()
    x = F.relu(rnd(N, C, H, W, seed=3)).to(DEV).to(dtype)
    xr = x.clone().requires_grad_(True)
    ph = max((-(-H // 2) - 1) * 2 + 3 - H, 0); pw = max((-(-W // 2) - 1) * 2 + 3 - W, 0)
    ref = F.max_pool2d(F.pad(xr, [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2], value=-float("inf")), 3, 2, 0)
    g = rnd(*ref.shape, seed=4).to(DEV).to(dtype)
    ref.backward(g)
    xs = x.clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ops.MaxPool3s2SameFn.apply(xs)
    y.backward(g.contiguous(memory_format=torch.channels_last))
    assert torch.equal(y.detach(), ref.detach())
    report(f"maxpool3s2_same bwd[{dtype},{N}x{C}x{H}x{W}]", xs.grad.float(), xr.grad.float(), rtol=0, atol=(0 if dtype == torch.float32 else 2e-2))


def test_conv1x1_fork_adds_shortcut_gradient_in_epilogue():
    """Conv1x1Fn(fork=True) hands out an alias of its input for the identity shortcut; the alias' gradient is added inside the
    input-gradient GEMM (MAED_EPI_ADD) -- must equal dgrad + shortcut gradient."""
    ops, _ = _ops()
    N, I, O, H, W = 2, 128, 64, 9, 7
    x = q(rnd(N, I, H, W, seed=5), torch.bfloat16)
    w = q(rnd(O, I, 1, 1, seed=6, scale=I ** -0.5), torch.bfloat16)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    gy, gs = q(rnd(N, O, H, W, seed=7), torch.bfloat16), q(rnd(N, I, H, W, seed=8), torch.bfloat16)
    (F.conv2d(xd, wd) * gy.double()).sum().backward()
    ref = xd.grad + gs.double()
    xg = x.to(DEV).bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wg = w.to(DEV).bfloat16().requires_grad_(True)
    y, xa = ops.Conv1x1Fn.apply(xg, wg, wg.detach().reshape(O, I).t().contiguous(), torch.zeros(O, I, device=DEV), True)
    assert xa.data_ptr() == xg.data_ptr()
    ((y * gy.to(DEV)).sum() + (xa * gs.to(DEV)).sum()).backward()
    report("conv1x1 fork: dx = dgrad + shortcut gradient", xg.grad.float(), ref, **tol(torch.bfloat16, 2))
    # shortcut only (main branch unused): the gradient passes through untouched
    xg2 = x.to(DEV).bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y2, xa2 = ops.Conv1x1Fn.apply(xg2, wg, wg.detach().reshape(O, I).t().contiguous(), None, True)
    (xa2 * gs.to(DEV)).sum().backward()
    assert torch.equal(xg2.grad, gs.to(DEV).to(xg2.grad.dtype))


@pytest.mark.parametrize("kind,F,H,W,Cin,Cout,stride", [("1x1", 16, 56, 56, 64, 256, 1), ("1x1", 8, 56, 56, 256, 64, 1), ("1x1", 6, 14, 14, 256, 1024, 1),
                                                        ("1x1", 3, 12, 12, 512, 128, 1), ("3x3", 8, 56, 56, 64, 64, 1), ("3x3", 4, 28, 28, 128, 128, 1),
                                                        ("3x3", 4, 56, 56, 128, 128, 2), ("3x3", 5, 14, 14, 256, 256, 1)])
def test_convolution_epilogue_groupnorm_statistics(kind, F, H, W, Cin, Cout, stride):
    """maed_conv1x1_fwd / maed_conv3x3_fwd gn_sums: the (sum, sum of squares) per (frame, group) the following GroupNorm needs, accumulated by
    the convolution's epilogue from the bf16-rounded values it stores (2 ... 32 channels per group, frames of 144 ... 3136 pixels that
    straddle the 128-row tiles) == the same sums computed from the stored tensor; the output itself is bit-identical to the plain call"""
    ops, _ = _ops()
    x = q(rnd(F, Cin, H, W, seed=1), torch.bfloat16).to(DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    sums = torch.zeros(F, 32, 2, dtype=torch.float64, device=DEV)
    if kind == "1x1":
        w = q(rnd(Cout, Cin, 1, 1, seed=2, scale=Cin ** -0.5), torch.bfloat16).to(DEV).bfloat16()
        y, y0 = ops.Conv1x1Fn.apply(x, w, None, None, False, sums), ops.Conv1x1Fn.apply(x, w, None, None, False, None)
    else:
        w = q(rnd(Cout, 3, 3, Cin, seed=2, scale=(9 * Cin) ** -0.5), torch.bfloat16).to(DEV).bfloat16()
        y, y0 = ops.conv3x3(x, w, stride, gn_sums=sums), ops.conv3x3(x, w, stride)
    assert torch.equal(y, y0)
    yg = y.permute(0, 2, 3, 1).reshape(F, -1, 32, Cout // 32).double()
    want = torch.stack([yg.sum(dim=(1, 3)), (yg * yg).sum(dim=(1, 3))], dim=-1)
    report(f"conv{kind} gn statistics[{F}x{Cin}->{Cout},{H}x{W}/{stride}]", sums, want, rtol=2e-5, atol=2e-5 * want.abs().max().item())


@pytest.mark.parametrize("N,I,O,H,W", [(4, 256, 512, 56, 56), (3, 512, 1024, 28, 28), (2, 64, 128, 7, 9)])
def test_conv1x1_stride2_on_packed_pixels(N, I, O, H, W):
    """ops.Conv1x1Fn(stride=2): the downsample shortcuts of stages 2 / 3 (cfg3 extents in the first two cases) = maed_subsample2_fwd + GEMMs on a
    quarter of the rows + maed_subsample2_bwd, vs fp64 conv2d(stride=2)"""
    ops, _ = _ops()
    x = q(rnd(N, I, H, W, seed=1), torch.bfloat16)
    w = q(rnd(O, I, 1, 1, seed=2, scale=I ** -0.5), torch.bfloat16)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ref = F.conv2d(xd, wd, stride=2)
    dy = q(rnd(*ref.shape, seed=3), torch.bfloat16)
    ref.backward(dy.double())
    xg = x.to(DEV).bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wg = w.to(DEV).bfloat16()
    wt = wg.reshape(O, I).t().contiguous()
    dw = torch.ones(O, I, dtype=torch.float32, device=DEV)
    y = ops.Conv1x1Fn.apply(xg, wg, wt, dw, False, None, 2)
    y.backward(dy.to(DEV).bfloat16())
    tag = f"[{N}x{I}->{O},{H}x{W}/2]"
    report(f"conv1x1s2 fwd{tag}", y.float(), ref, **tol(torch.bfloat16, 2))
    report(f"conv1x1s2 dx{tag}", xg.grad.float(), xd.grad, **tol(torch.bfloat16, 2))
    report(f"conv1x1s2 dw{tag}", dw - 1.0, wd.grad.reshape(O, I), rtol=2e-3, atol=2e-3 * wd.grad.abs().max().item())


@pytest.mark.parametrize("N,H,W", [(16, 224, 224), (2, 256, 256), (3, 32, 64)])
def test_stem7x7s2_forward_statistics_and_weight_gradient(N, H, W):
    """round 4: the stem convolution on the library (csrc/stem.hip) at the cfg3 / cfg5 frame sizes and a small one: forward from the padded 4-slot image vs fp64
    conv2d on the TF-SAME padded frames, the GroupNorm statistics of the rounded outputs from the epilogue, the weight gradient (LDS-DMA rows, transposing reads,
    512 workgroups walking 3-4 output rows each at cfg3) accumulated into a non-zero fp32 slice; bit-identical between the two forward variants and repeatable."""
    ops, _ = _ops()
    x = rnd(N, 3, H, W, seed=1)
    w = q(rnd(64, 3, 7, 7, seed=2, scale=147 ** -0.5), torch.bfloat16)
    wd = w.double().requires_grad_(True)
    ref = F.conv2d(F.pad(q(x, torch.bfloat16).double(), [2, 3, 2, 3]), wd, stride=2)
    dy = q(rnd(*ref.shape, seed=3), torch.bfloat16)
    ref.backward(dy.double())
    assert ops.stem7x7s2_supported(H, W)
    xp = ops.stem_input(x.to(DEV), torch.bfloat16, 7, 2, own=True)
    wg = w.to(DEV).bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    sums = torch.zeros(N, 32, 2, dtype=torch.float64, device=DEV)
    dw = torch.ones(64, 147, dtype=torch.float32, device=DEV)
    y = ops.StemConvFn.apply(xp, wg, dw, sums, (H, W))
    y0 = ops.StemConvFn.apply(xp, wg, dw, None, (H, W))
    assert torch.equal(y, y0)
    tag = f"[{N}x{H}x{W}]"
    report(f"stem7x7s2 fwd{tag}", y.float(), ref, **tol(torch.bfloat16, 2))
    yg = y.permute(0, 2, 3, 1).reshape(N, -1, 32, 2).double()
    want = torch.stack([yg.sum(dim=(1, 3)), (yg * yg).sum(dim=(1, 3))], dim=-1)
    report(f"stem7x7s2 gn statistics{tag}", sums, want, rtol=2e-5, atol=2e-5 * want.abs().max().item())
    y.backward(dy.to(DEV).bfloat16().contiguous(memory_format=torch.channels_last))
    ops.side_stream_join(torch.device(DEV))
    torch.cuda.synchronize()
    got = (dw - 1.0).view(64, 7, 7, 3).permute(0, 3, 1, 2)
    report(f"stem7x7s2 dw{tag}", got, wd.grad, rtol=2e-3, atol=2e-3 * wd.grad.abs().max().item())


@pytest.mark.parametrize("N,H,W", [(16, 56, 56), (3, 64, 64), (2, 5, 8)])
def test_conv3x3_weight_gradient_row_items_64_channels(N, H, W):
    """round 4: maed_conv3x3_wgrad at 64 -> 64 channels takes the row-item kernel (conv3x3_rows.hip: LDS-DMA rows in a ring, wave = tap, transposing reads) --
    the stage-1 shape of cfg3 (56 x 56) and cfg5 (64 x 64), and a tiny ragged one (5 x 8: 80 pixels, not a multiple of 64 -- the general kernel would refuse);
    accumulation into a non-zero slice, vs fp64 autograd through conv2d"""
    ops, _ = _ops()
    x = q(rnd(N, 64, H, W, seed=1), torch.bfloat16)
    dy = q(rnd(N, 64, H, W, seed=2), torch.bfloat16)
    wd = rnd(64, 64, 3, 3, seed=3, scale=576 ** -0.5).double().requires_grad_(True)
    F.conv2d(x.double(), wd, padding=1).backward(dy.double())
    dW = torch.ones(64, 3, 3, 64, dtype=torch.float32, device=DEV)
    cl = lambda t: t.to(DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    ops.conv3x3_wgrad(cl(dy), cl(x), out=dW)
    torch.cuda.synchronize()
    report(f"conv3x3 wgrad rows[{N}x64x{H}x{W}]", (dW - 1.0).permute(0, 3, 1, 2), wd.grad, rtol=2e-3, atol=2e-3 * wd.grad.abs().max().item())


@pytest.mark.parametrize("NF,H,W,Cin,Cout", [(2, 14, 14, 64, 128), (1, 16, 16, 128, 136), (2, 11, 13, 64, 64)])
def test_conv3x3_one_frame_per_workgroup_is_bit_identical_to_the_128_row_tiles(NF, H, W, Cin, Cout):
    """conv3x3_frame_bf16_kernel (csrc/conv3x3.hip: one frame x 128 channels per workgroup, three-stage copy ring, eight waves of 32 pixel rows, the last ones partly
    or wholly past the frame) forced with MAED_OPT_CONV3X3_FRAME = 2 against the 128 x 128 tiles (= 0): same K order, same MFMA shape, so the SAME bits -- forward
    with GroupNorm statistics (where Cout allows), with an `add` operand, and as the input gradient (transposed weight image, flipped taps; Cout % 64 == 0); a ragged
    last column tile (Cout = 136), and 143 pixels with a 64-column tile.  Cin = 64 is the ring prologue's minimum of 9 K tiles.  The host simulator's test of the
    same name (tests/test_hostsim_backbone.py), on the device."""
    ops, L = _ops()
    lib = L.lib()
    torch.manual_seed(7)
    cl = lambda t: t.bfloat16().to(DEV).contiguous(memory_format=torch.channels_last)
    x, dy, addt = cl(torch.randn(NF, Cin, H, W)), cl(torch.randn(NF, Cout, H, W)), cl(torch.randn(NF, Cout, H, W))
    wt = (torch.randn(Cout, 3, 3, Cin) * (9 * Cin) ** -0.5).bfloat16().to(DEV)
    wimg = wt.permute(1, 2, 3, 0).contiguous()             # (3, 3, Cin, Cout): the transposed image maed_weight_std_fwd writes beside the forward weight
    cpg = Cout // 32
    gn_ok = Cout % 32 == 0 and cpg >= 2 and (cpg & (cpg - 1)) == 0
    out = {}
    old = lib.maed_get_option(L.OPT_CONV3X3_FRAME)
    try:
        for mode in (0, 2):
            assert lib.maed_set_option(L.OPT_CONV3X3_FRAME, mode) == 0
            sums = torch.zeros(NF, 32, 2, dtype=torch.float64, device=DEV)
            y = ops.conv3x3(x, wt, 1, gn_sums=sums if gn_ok else None)
            ya = ops.conv3x3(x, wt, 1, add=addt)
            dx = ops.conv3x3(dy, wimg, 1, w_layout=1) if Cout % 64 == 0 else y
            torch.cuda.synchronize()
            out[mode] = (y, ya, dx, sums)
    finally:
        lib.maed_set_option(L.OPT_CONV3X3_FRAME, old)
    for a, b in zip(out[0][:3], out[2][:3]):
        assert a.shape == b.shape and torch.equal(a, b)
    assert torch.allclose(out[0][3], out[2][3], rtol=1e-6, atol=1e-4)       # (fp32 partial sums per lane over other row sets: the statistics agree to fp32 rounding)
    ref = F.conv2d(x.double(), wt.permute(0, 3, 1, 2).double(), padding=1)
    assert torch.allclose(out[2][0].double(), ref, rtol=2e-2, atol=2e-2)
    if Cout % 64 == 0:
        assert out[2][2].shape == (NF, Cin, H, W)


def test_stream_fence_orders_two_streams():
    """maed_stream_fence(from, to): everything enqueued on `from` so far happens before whatever is enqueued on `to` from now on (the fence the host uses for
    side-stream launches instead of framework events).  A long fill on stream A, the fence, a read on stream B: B must see the fill -- 20 rounds, fresh values."""
    from maed_amd import _lib as L, ops
    lib = L.lib()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    x = torch.zeros(64 << 20, dtype=torch.float32, device=DEV)          # 256 MB: the fill takes ~100 us
    y = torch.empty(1, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    for k in range(1, 21):
        with torch.cuda.stream(a):
            x.fill_(float(k))
        ops.check(lib.maed_stream_fence(a.cuda_stream, b.cuda_stream), "stream_fence")
        with torch.cuda.stream(b):
            y.copy_(x[-1:])
        ops.check(lib.maed_stream_fence(b.cuda_stream, a.cuda_stream), "stream_fence")      # (the next fill must not overtake the read)
        b.synchronize()
        assert y.item() == float(k), (k, y.item())
    assert lib.maed_stream_fence(a.cuda_stream, a.cuda_stream) == 0                          # same stream: nothing to do
    note("maed_stream_fence: 20 producer/consumer rounds across two streams in order")



def test_frame_barrier_timeout_is_reported_and_the_library_falls_back():
    """the one-pass GroupNorm backward synchronises the workgroups of a frame inside the launch with a bounded spin.  A peer that never arrives --
    forced here by a frame_sync arrival counter that is NOT zero at launch (the wait is for equality) -- used to end in a silently NaN-poisoned dx.  Now the poisoned
    call also raises the library's device-fault word: maed_device_faults() > 0, maed_last_error() explains, and from the next call on the two-pass kernels run and
    give the right answer.  The counter is cleared at the end so that the rest of the suite keeps the one-pass kernels."""
    ops, L = _ops()
    lib = L.lib()
    assert lib.maed_device_faults() == 0, "an earlier test already tripped a frame barrier"
    N, C, H, W = 2, 256, 56, 56
    dtype = torch.bfloat16
    x = q(rnd(N, C, H, W, seed=1) * 1.5 + 0.2, dtype)
    g, b = 1 + 0.2 * rnd(C, seed=3), 0.1 * rnd(C, seed=4)
    dy = q(rnd(N, C, H, W, seed=5), dtype)
    xd = x.double().requires_grad_(True)
    ref = F.relu(F.group_norm(xd, 32, g.double(), b.double(), 1e-5))
    ref.backward(dy.double())
    cl = lambda t: t.to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)

    def run(dirty):
        xg = cl(x).requires_grad_(True)
        gg, bg = g.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        ab = torch.zeros(N, C, 2, device=DEV)
        sync = torch.zeros(N * ops.GN_SYNC_WORDS, dtype=torch.int32, device=DEV)
        if dirty:
            sync.view(N, ops.GN_SYNC_WORDS)[:, 0] = 1000        # arrival counters that can never EQUAL the number of workgroups of a frame
        sums = torch.zeros(N, 32, 2, dtype=torch.float64, device=DEV)
        y = ops.GroupNormFn.apply(xg, None, gg, bg, 1e-5, True, False, sums, ab, False, False, sync)
        y.backward(cl(dy))
        torch.cuda.synchronize()
        return xg.grad.float().cpu()
    try:
        bad = run(dirty=True)
        assert torch.isnan(bad).any(), "a frame barrier that cannot complete must poison the result (if this shape no longer takes the one-pass kernel, pick one that does)"
        assert lib.maed_device_faults() > 0
        good = run(dirty=False)                 # the library has switched to the two-pass kernels
        assert lib.maed_device_faults() > 0 and "frame-barrier timeout" in lib.maed_last_error().decode()
        report("groupnorm_bwd.dx after a frame-barrier timeout (two-pass fallback)", good, xd.grad, **tol(dtype, 2))
        assert L.device_faults() > 0
    finally:
        lib.maed_device_faults_clear()
    assert lib.maed_device_faults() == 0
    again = run(dirty=False)                    # ... and the one-pass kernel is back
    report("groupnorm_bwd.dx after the fault word was cleared (one-pass kernel again)", again, xd.grad, **tol(dtype, 2))


# ---- round 6: the persistent K-stream GEMM (csrc/gemm_sk.hip) -----------------------------------------------------------------------------
from _gemm_cases import _sk_mode  # noqa: E402  (shared with tests/test_gpu_gemm_epilogues.py)


@pytest.mark.parametrize("M,N,K", [(300, 264, 128), (197 * 8, 512, 256), (1000, 1536, 512), (777, 256, 2048), (25216, 512, 512), (32896, 768, 3072)])
def test_gemm_persistent_kstream(M, N, K):
    """csrc/gemm_sk.hip against the fp64 oracle on the bf16-rounded operands -- whole tiles only (mode 2: bitwise equal to the 128x128 kernel, same k order), stream-K
    cuts on the full grid (mode 3) and on grids of 7 / 96 workgroups (several items per workgroup, tiles cut two and three ways, empty ranges), every epilogue the
    STE uses; ragged M / N edges; cfg3's proj and cfg5's fc2 at full size."""
    ops, L = _ops()
    dtype = torch.bfloat16
    A, B = q(rnd(M, K, seed=21), dtype), q(rnd(N, K, seed=22, scale=K ** -0.5), dtype)
    bias = rnd(N, seed=23)
    Ad, Bd, bd = A.to(DEV).to(dtype), B.to(DEV).to(dtype), bias.to(DEV)
    ref = (Ad.double() @ Bd.double().t()).cpu()
    t = tol(dtype, 2)
    res, pre_in = rnd(M, N, seed=24), q(rnd(M, N, seed=25), dtype)
    xg = pre_in.double().requires_grad_(True)
    R.gelu(xg).sum().backward()
    for mode, grid in [(2, 0), (3, 0), (3, 7), (3, 96)]:
        with _sk_mode(mode, grid):
            tag = f"gemm_sk[mode {mode} grid {grid},{M}x{N}x{K}]"
            out = ops.gemm_nt(Ad, Bd, L.EPI_STORE, bias=bd, impl=L.IMPL_MFMA_SK)
            report(tag + "[STORE]", out.float(), ref + bias.double(), **t)
            if mode == 2:
                assert torch.equal(out, ops.gemm_nt(Ad, Bd, L.EPI_STORE, bias=bd, impl=3))
            out = ops.gemm_nt(Ad, Bd, L.EPI_RESID_F32, bias=bd, aux=res.to(DEV), impl=L.IMPL_MFMA_SK)
            report(tag + "[RESID_F32]", out, ref + bias.double() + res.double(), rtol=2e-5, atol=1e-4)
            act, pre = ops.gemm_nt(Ad, Bd, L.EPI_GELU, bias=bd, impl=L.IMPL_MFMA_SK)
            report(tag + "[GELU.pre]", pre.float(), ref + bias.double(), **t)
            report(tag + "[GELU.act]", act.float(), R.gelu(pre.float().cpu().double()), **t)
            out = ops.gemm_nt(Ad, Bd, L.EPI_MUL_DGELU, aux=pre_in.to(DEV).to(dtype), impl=L.IMPL_MFMA_SK)
            report(tag + "[MUL_DGELU]", out.float(), ref * xg.grad, **t)
    assert L.lib().maed_device_faults() == 0


def test_gemm_persistent_kstream_race_screen():
    """the benchmarked shapes, 25 back-to-back launches per mode into NaN-filled outputs, every one bit-identical to the first and NaN-free: a copy landing late, a
    ring slot re-targeted early, a stale or half-written slab shows up as a differing launch.  A screen, not a proof -- the reads are placed by the vmcnt / barrier
    count and the hand-off by the release / acquire protocol (gemm_sk.hip header)."""
    ops, L = _ops()
    for M, N, K in [(25216, 512, 2048), (25216, 1536, 512), (25216, 2048, 512), (32896, 768, 3072)]:
        A = (torch.randn(M, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(K + N))).bfloat16()
        B = (torch.randn(N, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(N)) * K ** -0.5).bfloat16()
        for mode in (2, 3):
            with _sk_mode(mode):
                want = ops.gemm_nt(A, B, L.EPI_STORE, impl=L.IMPL_MFMA_SK)
                assert not torch.isnan(want.float()).any()
                bad = 0
                for _ in range(25):
                    out = torch.full_like(want, float("nan"))
                    ops.gemm_nt(A, B, L.EPI_STORE, out=out, impl=L.IMPL_MFMA_SK)
                    bad += int(not torch.equal(out, want))
                assert bad == 0, f"{bad}/25 launches of the persistent kernel (mode {mode}) differ at {M}x{N}x{K}"
    assert L.lib().maed_device_faults() == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_groupnorm_affine_gradients_deferred_to_one_batched_launch(dtype):
    """round 6: with the pass's pre-zeroed scratch arena the GroupNorm backward leaves its per-frame (dbeta, dgamma) partials in `ab`; ONE maed_gn_affine_grad_batch
    launch (ops.gn_affine_flush) folds every layer into gamma.grad / beta.grad.  Three layers of different widths and frame counts -- one of them twice (+= onto the
    first result) -- against the fp64 oracle, and against the per-layer closing kernel (MAED_GN_DEFER_AFFINE=0: same fold order per column)."""
    ops, _ = _ops()
    layers = [(3, 64, 9, 7), (5, 256, 14, 14), (2, 1024, 5, 5), (5, 256, 14, 14)]
    cl = lambda t: t.to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
    params = {}
    res = {}
    for defer in (True, False):
        ops.GN_DEFER_AFFINE = defer
        grads = {}
        try:
            for li, (N, C, H, W) in enumerate(layers):
                key = (C,)
                if key not in grads:
                    g, b = 1 + 0.2 * rnd(C, seed=3 + C), 0.1 * rnd(C, seed=4 + C)
                    params[key] = (g, b)
                    grads[key] = (g.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True))
                gg, bg = grads[key]
                x, dy = q(rnd(N, C, H, W, seed=10 + li) * 1.5 + 0.2, dtype), q(rnd(N, C, H, W, seed=20 + li), dtype)
                ab = torch.zeros(N, C, 2, dtype=torch.float32, device=DEV)
                sums = torch.zeros(N, 32, 2, dtype=torch.float64, device=DEV)
                sync = torch.zeros(N * ops.GN_SYNC_WORDS, dtype=torch.int32, device=DEV)
                xg = cl(x).requires_grad_(True)
                y = ops.GroupNormFn.apply(xg, None, gg, bg, 1e-5, True, True, sums, ab, False, False, sync)
                y.backward(cl(dy))
            ops.gn_affine_flush(torch.device(DEV))        # (the engine's end-of-pass callback has done it already: this must be a no-op then)
            torch.cuda.synchronize()
            res[defer] = {k: (a.grad.clone(), b.grad.clone()) for k, (a, b) in grads.items()}
        finally:
            ops.GN_DEFER_AFFINE = True
    for k in res[True]:
        # (same fold per column; the PARTIALS are atomically accumulated by the frame's workgroups in the one-pass backward -- up to four per frame in fp32 -- so two
        #  runs agree to the last bits, not bit for bit; scripts/r6/gn_defer_diag.py shows equality where the partials are equal)
        for a, b in zip(res[True][k], res[False][k]):
            assert (a - b).abs().max().item() <= 2e-6 * max(1.0, b.abs().max().item()), k
    # the oracle
    for key, (g, b) in params.items():
        gd, bd = g.double().requires_grad_(True), b.double().requires_grad_(True)
        for li, (N, C, H, W) in enumerate(layers):
            if (C,) != key:
                continue
            x, dy = q(rnd(N, C, H, W, seed=10 + li) * 1.5 + 0.2, dtype), q(rnd(N, C, H, W, seed=20 + li), dtype)
            F.relu(F.group_norm(x.double(), 32, gd, bd, 1e-5)).backward(dy.double())
        scale = max(1.0, gd.grad.abs().max().item())
        f32 = dtype == torch.float32
        report(f"groupnorm_bwd.dgamma[deferred,{dtype},C={key[0]}]", res[True][key][0], gd.grad, rtol=1e-4 if f32 else 2e-2, atol=(1e-4 if f32 else 3e-2) * scale)
        report(f"groupnorm_bwd.dbeta[deferred,{dtype},C={key[0]}]", res[True][key][1], bd.grad, rtol=1e-4 if f32 else 2e-2, atol=(1e-4 if f32 else 3e-2) * scale)


@pytest.mark.parametrize("M,N,K,bias", [(25216, 1536, 512, True), (25216, 512, 2048, True), (32896, 768, 3072, True), (1280, 264, 392, False), (25088, 1024, 256, False)])
def test_gemm_tn_persistent_kstream(M, N, K, bias):
    """csrc/gemm_tn_sk.hip (weight gradient dW += Y^T X, dbias += colsum Y on 256 x 256 tiles, one workgroup per CU, slabs + fixed-order reduce launch) against fp64 at
    the STE's shapes of cfg3 / cfg5, a ragged shape and a stage-3 convolution: fp32-accumulation accuracy, `+=` onto existing gradients, and -- no atomics -- bit-identical
    results over repeated launches (the split-M kernels differ from run to run)."""
    ops, L = _ops()
    lib = L.lib()
    g = torch.Generator(device=DEV).manual_seed(M + N)
    Y = torch.randn(M, N, device=DEV, generator=g).bfloat16()
    X = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    dW0, db0 = torch.randn(N, K, device=DEV, generator=g), torch.randn(N, device=DEV, generator=g)
    ref = dW0.double() + Y.double().t() @ X.double()
    refb = db0.double() + Y.double().sum(0)
    old = (lib.maed_get_option(L.OPT_TN_SK), lib.maed_get_option(L.OPT_SK_GRID))
    try:
        for grid in (255, 96):           # (an explicit grid takes the kernel whatever the heuristic says: 255 ~ one workgroup per CU, 96: longer items, other tile shares)
            lib.maed_set_option(L.OPT_TN_SK, 1); lib.maed_set_option(L.OPT_SK_GRID, grid)
            outs = []
            for _ in range(4):
                dW, db = dW0.clone(), (db0.clone() if bias else None)
                ops.gemm_tn_wgrad(Y, X, dW=dW, dbias=db)
                outs.append((dW, db))
            scale = ref.abs().max().item()
            report(f"gemm_tn_sk[{M}x{N}x{K},grid {grid}] dW", outs[0][0], ref, rtol=0, atol=2e-6 * scale)
            if bias:
                report(f"gemm_tn_sk[{M}x{N}x{K},grid {grid}] dbias", outs[0][1], refb, rtol=0, atol=2e-6 * refb.abs().max().item())
            for dW, db in outs[1:]:
                assert torch.equal(dW, outs[0][0]) and (not bias or torch.equal(db, outs[0][1])), "the persistent weight-gradient kernel must be deterministic"
    finally:
        lib.maed_set_option(L.OPT_TN_SK, old[0]); lib.maed_set_option(L.OPT_SK_GRID, old[1])
