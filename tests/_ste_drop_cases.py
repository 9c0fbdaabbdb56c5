"""TEST INFRASTRUCTURE: dropout / stochastic depth of the STE blocks (docs/design/14_ste_regularisation.md) -- the mask definition of include/maed_hip.h restated
in numpy uint64, an fp64 regularised block composed from oracle.maed_ref pieces with explicit masks, and the case bodies shared by the simulator tests
(tests/test_hostsim_ste_drop.py, device "cpu" under tests/_hostsim.patched()) and the GPU tests (tests/test_gpu_ste_drop.py).  No GPU code here: the callers say
on which device the tensors live; the library handle is whatever maed_amd._lib.lib() returns at the time.

Bounds.  Epilogues: the derived elementwise bound of the unmasked epilogue (tests/_gemm_cases.py), its accumulation / activation terms multiplied by the case's
scale 1 / ((1 - drop)(1 - drop_path)) -- the surviving terms are the same products times that constant -- plus 2 * 2^-23 |masked term| for the three extra fp32
roundings of the masked form (the scale constant, g * k, and the product with the value).  Block: the bars of tests/test_gpu_model.py::
test_block_forward_backward_vs_oracle with atol times the same scale."""
import functools
from functools import partial

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import _gemm_cases as G
from maed_amd import _lib as L
from maed_amd import ops
from oracle import maed_ref as R

GOLD, SITE = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xD1B54A32D192ED03)
M64 = (1 << 64) - 1
F32, BF16 = torch.float32, torch.bfloat16
LN = partial(nn.LayerNorm, eps=1e-6)


# ---- the mask definition (include/maed_hip.h "MASK DEFINITION") in numpy uint64: every product and sum wraps mod 2^64 ---------------------------------------
def keep(seed, n, p):
    """bool[n]: keep(seed, idx) for idx = 0 .. n-1 -- splitmix64 finaliser of seed + (idx + 1) * GOLD, top 24 bits >= floor(p * 2^24)"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & M64) + (np.arange(n, dtype=np.uint64) + np.uint64(1)) * GOLD
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)) >= np.uint64(int(p * 16777216.0))


def block_seed_of_record(base, call_id):
    return (base + call_id * int(GOLD)) & M64


def site_seed(block_seed, s):
    return (block_seed + s * int(SITE)) & M64


def site_masks(block_seed, drop, drop_path, rows, N, group_rows, site_drop, site_path):
    """(k bool (rows, N), g bool (rows, 1)) of one site pair; a rate of 0 (or site 0) keeps everything"""
    k = np.ones((rows, N), dtype=bool)
    g = np.ones((rows, 1), dtype=bool)
    if site_drop and drop > 0:
        k = keep(site_seed(block_seed, site_drop), rows * N, drop).reshape(rows, N)
    if site_path and drop_path > 0:
        frames = (rows + group_rows - 1) // group_rows
        g = np.repeat(keep(site_seed(block_seed, site_path), frames, drop_path), group_rows)[:rows].reshape(rows, 1)
    return k, g


def scale_of(drop, drop_path):
    return 1.0 / ((1.0 - drop) * (1.0 - drop_path))


def mask_f64(block_seed, drop, drop_path, rows, N, group_rows, site_drop, site_path):
    """the multiplier g(r / group_rows) * k(r, c) as an fp64 tensor (rows, N)"""
    k, g = site_masks(block_seed, drop, drop_path, rows, N, group_rows, site_drop, site_path)
    m = (k & g).astype(np.float64) * (1.0 / (1.0 - drop) if site_drop and drop > 0 else 1.0) * (1.0 / (1.0 - drop_path) if site_path and drop_path > 0 else 1.0)
    return torch.from_numpy(m)


def pick_seed(frames, drop_path, start):
    """smallest block seed >= start whose frame masks at sites 2 and 5 both keep at least one frame and drop at least one (drop_path = 0: start itself)"""
    s = start
    while drop_path > 0:
        ok = all(0 < int(keep(site_seed(s, site), frames, drop_path).sum()) < frames for site in (2, 5))
        if ok:
            break
        s += 1
    return s


def reg_of(drop, drop_path, seed):
    return (float(drop), float(drop_path), seed, None, 0)


# ---- 1. epilogues through maed_gemm_nt_drop -----------------------------------------------------------------------------------------------------------------
EPI_SHAPES = [(30, 128, 128, 5), (4 * 197, 256, 256, 197), (30, 100, 128, 5)]      # (M, N, K, rows per frame)
EPI_RATES = (0.25, 0.3)                                                              # (drop, drop_path)
IMPLS = {"f32": (F32, L.IMPL_AUTO), "bf16-valu": (BF16, L.IMPL_VALU), "bf16-mfma": (BF16, L.IMPL_MFMA), "bf16-glds1": (BF16, G.IMPL_MFMA_GLDS1)}
EPI_SEED = 0x5EED0123456789AB


def run_epilogue_case(dev, kernel, shape, epilogue, log=None):
    dtype, impl = IMPLS[kernel]
    M, N, K, P = shape
    drop, drop_path = EPI_RATES
    d = G.operands(dtype, M, N, K)
    A, B, bias = d["A"].to(dev), d["B"].to(dev), d["bias"].to(dev)
    tag = f"{epilogue}[{kernel},{M}x{N}x{K},P{P}]"
    if epilogue == "RESID_DROP_F32":
        m = mask_f64(EPI_SEED, drop, drop_path, M, N, P, 1, 2)
        da = ops.drop_args(reg_of(drop, drop_path, EPI_SEED), 1, 2, P)
        sc = scale_of(drop, drop_path)
        v = d["acc"] + d["bias"].double()
        # aux = 0: the zero set of the output IS the mask
        out0 = ops.gemm_nt_drop(A, B, L.EPI_RESID_DROP_F32, da, bias=bias, aux=torch.zeros(M, N, device=dev), impl=impl).cpu()
        assert torch.equal(out0 == 0, m == 0), f"{tag}: the zero set of the output differs from the numpy mask in {int(((out0 == 0) != (m == 0)).sum())} places"
        assert 0 < int((m == 0).sum()) < m.numel() and (m == 0).all(dim=1).any() and not (m == 0).all(dim=1).all()      # element AND frame masks are in play
        out = ops.gemm_nt_drop(A, B, L.EPI_RESID_DROP_F32, da, bias=bias, aux=d["res"].to(dev), impl=impl)
        ref = d["res"].double() + m * v
        G.check(tag, out, ref, sc * d["acc_bound"] + G.U23 * ref.abs() + 2 * G.U23 * (m * v).abs(), log)
    elif epilogue == "GELU_DROP":
        m = mask_f64(EPI_SEED, drop, 0.0, M, N, P, 3, 0)
        da = ops.drop_args(reg_of(drop, drop_path, EPI_SEED), 3, 0, P)
        sc = scale_of(drop, 0.0)
        out, pre = ops.gemm_nt_drop(A, B, L.EPI_GELU_DROP, da, bias=bias, impl=impl)
        (_, pref, pbound), = G.reference("GELU", d, dtype)
        G.check(tag + ".pre", pre, pref, pbound, log)                       # out2 = the pre-activation as today
        aref, abound = G.activation_reference("GELU", d, dtype, pre.detach().double().cpu())
        ref, bound = m * aref, sc * abound + 2 * G.U23 * (m * aref).abs()
        G.check(tag, out, ref, bound, log)
        outc = out.detach().double().cpu()
        assert (outc[m == 0] == 0).all(), f"{tag}: a dropped element is not zero"
        assert ((outc != 0) | (m == 0) | (ref.abs() <= bound)).all(), f"{tag}: a kept element with a non-zero activation is zero"
    elif epilogue == "MUL_DGELU_DROP":
        m = mask_f64(EPI_SEED, drop, 0.0, M, N, P, 3, 0)
        da = ops.drop_args(reg_of(drop, drop_path, EPI_SEED), 3, 0, P)
        sc = scale_of(drop, 0.0)
        out = ops.gemm_nt_drop(A, B, L.EPI_MUL_DGELU_DROP, da, aux=d["aux"].to(dev), impl=impl)
        (_, uref, ubound), = G.reference("MUL_DGELU", d, dtype)
        ref, bound = m * uref, sc * ubound + 2 * G.U23 * (m * uref).abs()
        G.check(tag, out, ref, bound, log)
        outc = out.detach().double().cpu()
        assert (outc[m == 0] == 0).all(), f"{tag}: a dropped element is not zero"
        assert ((outc != 0) | (m == 0) | (ref.abs() <= bound)).all(), f"{tag}: a kept element with a non-zero product is zero"
    else:
        raise KeyError(epilogue)


# ---- 2. maed_drop_scale_cast --------------------------------------------------------------------------------------------------------------------------------
def run_scale_cast_case(dev, dtype, rows, N, P):
    drop, drop_path, seed = 0.25, 0.3, 0x1234
    x = G.rnd(rows, N, seed=11)
    da = ops.drop_args(reg_of(drop, drop_path, seed), 4, 5, P)
    k, g = site_masks(seed, drop, drop_path, rows, N, P, 4, 5)
    keepm = torch.from_numpy(k & g)
    # the kernel's multiplier: the two fp32 scale constants, multiplied in fp32
    mul = np.float32(1.0) / (np.float32(1.0) - np.float32(drop_path)) * (np.float32(1.0) / (np.float32(1.0) - np.float32(drop)))
    y = ops.drop_scale_cast(x.to(dev), dtype, da).cpu()
    assert torch.equal(y != 0, keepm), "zero set differs from the numpy mask"
    want = torch.where(keepm, x * float(mul), torch.zeros(())).to(dtype)      # one fp32 product, then the output rounding
    assert torch.equal(y, want), f"values differ from mask * scale * x by up to {(y.float() - want.float()).abs().max().item():.3e}"
    # its own backward: applied twice with one seed = one application, scaled once more
    y1 = ops.drop_scale_cast(x.to(dev), F32, da)
    y2 = ops.drop_scale_cast(y1, F32, da).cpu()
    assert torch.equal(y2, torch.where(keepm, y1.cpu() * float(mul), torch.zeros(())))
    # in place (fp32)
    z = x.to(dev).clone()
    ops.drop_scale_cast(z, F32, da, out=z)
    assert torch.equal(z.cpu(), y1.cpu())


# ---- 3 / 4. the block against the fp64 masked oracle ----------------------------------------------------------------------------------------------------------
def block_ref(x, p, H, T, mode, drop, drop_path, block_seed):
    """vision_transformer.py:106-112,176-177,259-260 with the five masks explicit: oracle.maed_ref pieces in fp64"""
    Fr, P, C = x.shape
    a = R.attention_mode(R.layer_norm(x, p["norm1.weight"], p["norm1.bias"]), p, "attn.", H, T, mode)      # (F, P, C); 'temporal': (F, 1, C)
    P1 = a.shape[1]
    x = x + mask_f64(block_seed, drop, drop_path, Fr * P1, C, P1, 1, 2).view(Fr, P1, C) * a
    h = R.gelu(F.linear(R.layer_norm(x, p["norm2.weight"], p["norm2.bias"]), p["mlp.fc1.weight"], p["mlp.fc1.bias"]))
    Hd = h.shape[-1]
    h = mask_f64(block_seed, drop, 0.0, Fr * P, Hd, P, 3, 0).view(Fr, P, Hd) * h
    y = F.linear(h, p["mlp.fc2.weight"], p["mlp.fc2.bias"])
    return x + mask_f64(block_seed, drop, drop_path, Fr * P, C, P, 4, 5).view(Fr, P, C) * y


@functools.lru_cache(maxsize=4)
def block_params(C, P, mode):
    p = {k[len("encoder.blocks.0."):]: v for k, v in R.make_params(embed_dim=C, depth=1, hidden_dim=64, layers=(1, 1, 1), n_tokens=P, seed=3).items()
         if k.startswith("encoder.blocks.0.") and (mode == "parallel" or "ts_attn" not in k)}
    return {k: v * (3.0 if k.endswith("weight") and v.dim() == 2 else 1.0) for k, v in p.items()}


@functools.lru_cache(maxsize=16)
def block_reference(Fr, P, C, H, T, mode, drop, drop_path, seed):
    """(y, dx, {name: grad}) of the fp64 oracle -- computed once per case, shared by the dtypes, read only"""
    p = block_params(C, P, mode)
    x, dy = G.rnd(Fr, P, C, seed=1), G.rnd(Fr, P, C, seed=2)
    pd = {k: v.double().requires_grad_(True) for k, v in p.items()}
    xr = x.double().requires_grad_(True)
    y = block_ref(xr, pd, H, T, mode, drop, drop_path, seed)
    y.backward(dy.double())
    return y.detach(), xr.grad, {k: v.grad for k, v in pd.items()}


def make_block(C, H, dtype, mode, dev, drop=0.0, drop_path=0.0, impl=0, state=None, with_rates=True):
    from maed_amd.vision_transformer import Block
    kw = dict(drop=drop, drop_path=drop_path) if with_rates else {}
    blk = Block(C, H, mlp_ratio=4, qkv_bias=True, norm_layer=LN, st_mode=mode, compute_dtype=dtype, impl=impl, **kw)
    if state is not None:
        blk.load_state_dict(state)
    return blk.to(dev)


def run_block_case(dev, dims, dtype, rates, mode="parallel", impl=0, report=None):
    Fr, P, C, H, T = dims
    drop_path, drop = rates
    seed = pick_seed(Fr, drop_path, 1000)
    if drop_path > 0:     # the condition of the case: at sites 2 and 5 the mask keeps at least one frame and drops at least one
        for site in (2, 5):
            kept = int(keep(site_seed(seed, site), Fr, drop_path).sum())
            assert 0 < kept < Fr, (site, kept)
    yref, dxref, gref = block_reference(Fr, P, C, H, T, mode, drop, drop_path, seed)
    blk = make_block(C, H, dtype, mode, dev, drop, drop_path, impl, block_params(C, P, mode))
    blk.drop_seed = seed
    blk.train()
    xg = G.rnd(Fr, P, C, seed=1).to(dev).requires_grad_(True)
    y = blk(xg, T)
    y.backward(G.rnd(Fr, P, C, seed=2).to(dev))
    sc = scale_of(drop, drop_path)
    f32 = dtype == F32
    tl = dict(rtol=1e-4, atol=1e-4 * sc) if f32 else dict(rtol=3e-2, atol=3e-2 * sc)
    tag = f"[{mode},{dtype},impl{impl},F{Fr} P{P},dp{drop_path} d{drop}]"
    report(f"RegBlock.forward{tag}", y, yref, **tl)
    report(f"RegBlock.backward.dx{tag}", xg.grad, dxref, **tl)
    for name, prm in blk.named_parameters():
        ref = gref[name]
        assert prm.grad is not None, name
        report(f"RegBlock.backward.d[{name}]{tag}", prm.grad, ref, rtol=1e-3 if f32 else 5e-2, atol=(1e-4 if f32 else 3e-2) * max(ref.abs().max().item(), 1e-3) * sc)
    # the masks are really in the output: a dropped frame of the MLP branch AND the attention branch is the input itself
    k2, k5 = keep(site_seed(seed, 2), Fr, drop_path) if drop_path > 0 else np.ones(Fr, bool), keep(site_seed(seed, 5), Fr, drop_path) if drop_path > 0 else np.ones(Fr, bool)
    for f in np.nonzero(~k2 & ~k5)[0]:
        assert torch.equal(y[int(f)].detach().cpu(), xg[int(f)].detach().cpu()), f"frame {f} dropped at both sites must pass through unchanged"


def log_report(name, got, ref, rtol, atol):
    """the assertion of tests/_util.report without its file (simulator tests write no report)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and not torch.isnan(got).any(), name
    err = (got - ref).abs()
    bad = err > (atol + rtol * ref.abs())
    print(f"{name:70s} max_abs={err.max().item():.3e} ref_max={ref.abs().max().item():.3e}")
    assert not bad.any(), f"{name}: {int(bad.sum())}/{bad.numel()} elements out of tolerance (max_abs={err.max().item():.3e})"


# ---- 5. identity and determinism ---------------------------------------------------------------------------------------------------------------------------
def _identity_setup(dev, dtype, mode):
    Fr, P, C, H, T = 6, 5, 128, 2, 3
    state = block_params(C, P, mode)
    x, dy = G.rnd(Fr, P, C, seed=1).to(dev), G.rnd(Fr, P, C, seed=2).to(dev)

    def run(blk, grad=True, backward=True):
        xg = x.clone().requires_grad_(grad)
        for q in blk.parameters():
            q.grad = None
        y = blk(xg, T)
        if grad and backward:
            y.backward(dy)
            return [y.detach().clone(), xg.grad.clone()] + [q.grad.clone() for q in blk.parameters()]
        return [y.detach().clone()]

    return Fr, C, H, state, run


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


def run_identity_case(dev, dtype, mode="parallel"):
    """rates of 0, eval() and no_grad inference are the identity ON TODAY'S ENTRY POINTS: bit-identical to a Block built without the arguments"""
    Fr, C, H, state, run = _identity_setup(dev, dtype, mode)
    plain = make_block(C, H, dtype, mode, dev, state=state, with_rates=False)
    zero = make_block(C, H, dtype, mode, dev, 0.0, 0.0, state=state)
    reg = make_block(C, H, dtype, mode, dev, 0.1, 0.3, state=state)
    assert isinstance(zero.drop_path, nn.Identity) and type(reg.drop_path).__name__ == "DropPath" and reg.drop_path.drop_prob == 0.3
    assert list(reg.state_dict()) == list(plain.state_dict())                      # state-dict keys do not change
    assert _same(run(zero.train()), run(plain.train())), "rate-0 training differs from a Block built without the arguments"
    with torch.no_grad():
        want = run(plain.eval(), False)
        assert _same(run(reg.eval(), False), want), "eval() with non-zero rates differs from the rate-0 model"
        assert _same(run(reg.train(), False), want), "no_grad inference with non-zero rates differs from the rate-0 model"


def run_determinism_case(dev, dtype, mode="parallel"):
    """one pinned seed: the same bits, forward and gradients; another seed, or none: other masks"""
    Fr, C, H, state, run = _identity_setup(dev, dtype, mode)
    reg = make_block(C, H, dtype, mode, dev, 0.1, 0.3, state=state).train()
    reg.drop_seed = pick_seed(Fr, 0.3, 77)
    a, b = run(reg), run(reg)
    assert _same(a, b), "two training forwards with one pinned seed differ"
    reg.drop_seed = pick_seed(Fr, 0.3, reg.drop_seed + 1)
    assert not torch.equal(run(reg, backward=False)[0], a[0]), "another seed gave the same output"
    reg.drop_seed = None
    assert not torch.equal(run(reg, backward=False)[0], run(reg, backward=False)[0]), "unpinned seeds: two forwards drew the same masks"


# ---- 6. distribution --------------------------------------------------------------------------------------------------------------------------------------------
def within(kept, n, p):
    return abs(kept / n - (1.0 - p)) <= 5.0 * (p * (1.0 - p) / n) ** 0.5


def run_distribution_case(dev):
    rows, N, P, p = 400, 256, 5, 0.3
    x = (G.rnd(rows, N, seed=5).abs() + 1.0).to(dev)                                # no zeros: survivors are countable
    for site in (1, 3, 4):
        for seed in (1, 2 ** 63 + 12345):
            y = ops.drop_scale_cast(x, F32, ops.drop_args(reg_of(p, 0.0, seed), site, 0, P))
            kept = int((y != 0).sum())
            assert within(kept, rows * N, p), (site, seed, kept / (rows * N))
            assert kept == int(keep(site_seed(seed, site), rows * N, p).sum())
    # the element sites inside the GEMM epilogues draw the same masks: covered exactly by the epilogue cases; here the frame sites over many frames
    for site in (2, 5):
        y = ops.drop_scale_cast(x[:, :8].contiguous().repeat(25, 1), F32, ops.drop_args(reg_of(0.0, p, 99), 0, site, 1))
        kept = int((y[:, 0] != 0).sum())
        assert within(kept, rows * 25, p), (site, kept / (rows * 25))


def run_pos_drop_case(dev):
    from maed_amd import ste_modes
    p = 0.1
    x = (G.rnd(16, 50, 128, seed=6).abs() + 1.0).to(dev)
    y = ste_modes.dropout(x, p, True)
    nz = y != 0
    assert within(int(nz.sum()), x.numel(), p), int(nz.sum()) / x.numel()
    torch.testing.assert_close(y[nz], (x / (1.0 - p))[nz], rtol=1e-6, atol=0.0)
    assert ste_modes.dropout(x, p, False) is x and ste_modes.dropout(x, 0.0, True) is x


# ---- 7. plumbing ---------------------------------------------------------------------------------------------------------------------------------------------
def small_maed(dev, dtype=BF16, **kw):
    import maed_amd
    return maed_amd.MAED(num_blocks=1, embed_dim=128, num_heads=2, img_size=64, hidden_dim=64, compute_dtype=dtype, **kw).to(dev)


def train_targets(dev, N=1, T=2):
    g = torch.Generator().manual_seed(10)
    tgt = dict(kp_2d=torch.cat([torch.randn(N, T, 49, 2, generator=g) * 0.3, torch.rand(N, T, 49, 1, generator=g)], -1),
               kp_3d=torch.cat([torch.randn(N, T, 49, 3, generator=g) * 0.3, torch.ones(N, T, 49, 1)], -1),
               theta=torch.randn(N, T, 85, generator=g) * 0.2, w_smpl=torch.ones(N, T))
    return {k: v.to(dev) for k, v in tgt.items()}


def run_train_step_case(dev, dtype=BF16):
    from maed_amd.loss import LossVideo
    torch.manual_seed(0)
    m = small_maed(dev, dtype, drop_path_rate=0.1, drop_rate=0.1).train()
    blk = m.encoder.blocks[0]
    assert blk.drop == 0.1 and blk.drop_path_prob == 0.0 and m.encoder.pos_drop.p == 0.1      # linspace(0, 0.1, 1) = [0]
    clip = torch.randn(1, 2, 3, 64, 64, generator=torch.Generator().manual_seed(9)).to(dev)
    out = m(clip)
    loss, _ = LossVideo()(out, train_targets(dev), None)
    loss.backward()
    assert torch.isfinite(loss).item(), loss
    assert all(torch.isfinite(q.grad).all().item() for q in m.encoder.blocks.parameters())
