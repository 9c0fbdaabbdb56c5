"""Cases shared by tests/test_hostsim_backbone_fused_fwd.py (CPU simulator) and tests/test_gpu_backbone_fused_fwd.py (MI355X): the backbone's one-pass forward
forms -- stem GroupNorm + ReLU inside the max-pool (maed_gn_relu_maxpool3s2_fwd), the shortcut's GroupNorm inside the block's closing GroupNorm
(maed_groupnorm_dual_fwd) -- against the kernel sequences they replace, bit for bit; and the backward of the folded pair (ops.GroupNormFn later=True + its consumer) against the plain
two-Function composition with a materialised shortcut gradient, both held to fp32 autograd.

Every function takes the device the tensors live on; the simulator suite calls them inside _hostsim.patched()."""
import torch
import torch.nn.functional as F

from maed_amd import _lib as L
from maed_amd import ops

from _util import rnd, tol

EPS = 1e-5
BF = torch.bfloat16

STEM_SHAPES = [(2, 64, 17, 15), (2, 64, 16, 16)]          # odd sizes: asymmetric SAME padding (top / left 0, bottom / right 1)
DUAL_SHAPES = [(3, 64, 14, 14), (3, 128, 14, 14), (3, 256, 14, 14),       # 2 / 4 / 8 channels per group; 196 pixels: no multiple of the kernels' row tile
               (2, 512, 8, 8)]                                            # 16 channels per group: a thread's 8 channels share one group


def report_quiet(name, got, ref, rtol, atol):
    """_util.report without the parity-report file (the simulator suite): print the largest error, then assert |got - ref| <= atol + rtol * |ref| elementwise"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = (got - ref).abs()
    print(f"{name:70s} max_abs={err.max().item():.3e} ref_max={ref.abs().max().item():.3e}")
    assert got.shape == ref.shape and not torch.isnan(got).any(), name
    bad = err > (atol + rtol * ref.abs())
    assert not bad.any(), f"{name}: {int(bad.sum())}/{bad.numel()} elements out of tolerance, max_abs={err.max().item():.3e}"


def nhwc(t, dev, dtype=BF):
    """(N, C, H, W) values -> channels_last tensor of the compute dtype on `dev`"""
    return t.to(dev).to(dtype).contiguous(memory_format=torch.channels_last)


def _affine(C, dev, seed):
    return (1 + 0.2 * rnd(C, seed=seed)).to(dev), (0.1 * rnd(C, seed=seed + 1)).to(dev)


def _gn_fwd(x, res, gamma, beta, relu, want_mask=False):
    """maed_groupnorm_fwd (own statistics pass): y, sums, mask"""
    N, C, H, W = x.shape
    y = torch.empty_like(x, memory_format=torch.channels_last)
    sums = torch.zeros(N, 32, 2, dtype=torch.float64, device=x.device)
    mask = torch.zeros(N * H * W * (C // 8), dtype=torch.uint8, device=x.device) if want_mask else None
    L.check(L.lib().maed_groupnorm_fwd(ops._p(x), ops._p(res), ops._p(gamma), ops._p(beta), ops._p(y), ops._p(sums), ops._p(mask), N, H * W, C, EPS, int(relu),
                                       ops.dt_code(x.dtype), 1, ops._stream()), "groupnorm_fwd")
    return y, sums, mask


def check_stem_kernel(dev, N, C, H, W):
    x = nhwc(rnd(N, C, H, W, seed=1) * 1.5 + 0.2, dev)
    gamma, beta = _affine(C, dev, 3)          # beta around zero: about half of the normalised values are negative -> exact zeros behind the ReLU, ties in most windows
    yn, sums, _ = _gn_fwd(x, None, gamma, beta, True)
    zeros = (yn == 0).float().mean().item()
    assert 0.3 < zeros < 0.7, zeros
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    y_ref = torch.empty((N, C, Ho, Wo), dtype=BF, device=dev).contiguous(memory_format=torch.channels_last)
    idx_ref = torch.zeros(N * Ho * Wo * C, dtype=torch.uint8, device=dev)
    L.check(L.lib().maed_maxpool3s2_same_fwd(ops._p(yn), ops._p(y_ref), ops._p(idx_ref), N, H, W, C, L.BF16, ops._stream()), "maxpool3s2_same_fwd")
    for stats in (2, 0):            # statistics as the convolution's epilogue leaves them / computed by the entry point itself
        y = torch.full_like(y_ref, float("nan"))
        idx = torch.full_like(idx_ref, 255)
        s = sums.clone() if stats == 2 else torch.full_like(sums, 7.0)
        L.check(L.lib().maed_gn_relu_maxpool3s2_fwd(ops._p(x), ops._p(gamma), ops._p(beta), ops._p(y), ops._p(idx), ops._p(s), N, H, W, C, EPS, L.BF16, stats,
                                                    ops._stream()), "gn_relu_maxpool3s2_fwd")
        assert torch.equal(y.view(torch.int16), y_ref.view(torch.int16)), (stats, "y")
        assert torch.equal(idx, idx_ref), (stats, "idx", int((idx != idx_ref).sum()))
    assert (y_ref == 0).any()          # windows that are all zero: the first tap must have won them


def check_stem_function(dev, N, C, H, W, report):
    """ops.GroupNormReluMaxPoolFn against GroupNormFn(relu) -> MaxPool3s2SameFn: forward bits, then dx / dgamma / dbeta under the groupnorm_bwd bounds of
    tests/test_gpu_kernels.py::test_groupnorm_fused (both backwards are the same two kernels on the same bits: what remains is the order of the fp32 atomics)"""
    x = nhwc(rnd(N, C, H, W, seed=1) * 1.5 + 0.2, dev)
    gamma, beta = _affine(C, dev, 3)
    dy = nhwc(rnd(N, C, (H + 1) // 2, (W + 1) // 2, seed=7), dev)
    out = []
    for fused in (True, False):
        xl, gl, bl = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
        y = ops.GroupNormReluMaxPoolFn.apply(xl, gl, bl, EPS, False) if fused else ops.MaxPool3s2SameFn.apply(ops.GroupNormFn.apply(xl, None, gl, bl, EPS, True, False))
        y.backward(dy)
        out.append((y.detach(), xl.grad, gl.grad, bl.grad))
    (y1, dx1, dg1, db1), (y0, dx0, dg0, db0) = out
    assert torch.equal(y1.view(torch.int16), y0.view(torch.int16))
    tag = f"[{N}x{C}x{H}x{W}]"
    report(f"gn_relu_maxpool_bwd.dx{tag}", dx1.float(), dx0.float(), **tol(BF, 2))
    scale = max(1.0, dg0.abs().max().item())
    report(f"gn_relu_maxpool_bwd.dgamma{tag}", dg1, dg0, rtol=2e-2, atol=3e-2 * scale)
    report(f"gn_relu_maxpool_bwd.dbeta{tag}", db1, db0, rtol=2e-2, atol=3e-2 * scale)


def _dual_inputs(dev, N, C, H, W):
    x = nhwc(rnd(N, C, H, W, seed=1) * 1.5 + 0.2, dev)
    xs = nhwc(rnd(N, C, H, W, seed=2) * 0.7 - 0.1, dev)
    return x, xs, _affine(C, dev, 3), _affine(C, dev, 5)


def check_dual_kernel(dev, N, C, H, W):
    x, xs, (g, b), (g2, b2) = _dual_inputs(dev, N, C, H, W)
    short, sums2, _ = _gn_fwd(xs, None, g2, b2, False)
    y_ref, sums, mask_ref = _gn_fwd(x, short, g, b, True, want_mask=True)
    for stats in (2, 0):
        y = torch.full_like(y_ref, float("nan"))
        mask = torch.full_like(mask_ref, 0xA5)
        s, s2 = (sums.clone(), sums2.clone()) if stats == 2 else (torch.full_like(sums, 7.0), torch.full_like(sums2, 7.0))
        L.check(L.lib().maed_groupnorm_dual_fwd(ops._p(x), ops._p(g), ops._p(b), ops._p(s), ops._p(xs), ops._p(g2), ops._p(b2), ops._p(s2), ops._p(y), ops._p(mask),
                                                N, H * W, C, EPS, EPS, L.BF16, stats, stats, ops._stream()), "groupnorm_dual_fwd")
        assert torch.equal(y.view(torch.int16), y_ref.view(torch.int16)), (stats, "y")
        assert torch.equal(mask, mask_ref), (stats, "mask")


def _autograd_reference(x, xs, g, b, g2, b2, dy):
    """fp32 torch autograd on the same bf16 inputs.  The normalised shortcut is a bf16 TENSOR in the computation under test (stored by the two-kernel path, rounded
    in registers by the fused one), so the reference rounds it too, with a straight-through gradient: without that, about |shortcut| * 2^-9 * density(0) ~ 6e-4 of
    the elements would sit on the other side of the ReLU than in either composition, each such element an O(1) difference in dx that no rounding bound covers
    (measured on the simulator at 3 x 64 x 14 x 14: the OLD two-kernel composition against the un-rounded reference has 7 of 37632 dx elements out of bound,
    the largest off by 1.4)."""
    xr, sr = x.detach().float().cpu().clone().requires_grad_(True), xs.detach().float().cpu().clone().requires_grad_(True)
    p = [t.detach().float().cpu().clone().requires_grad_(True) for t in (g, b, g2, b2)]
    s = F.group_norm(sr, 32, p[2], p[3], EPS)
    s = s + (s.to(BF).float() - s).detach()
    F.relu(F.group_norm(xr, 32, p[0], p[1], EPS) + s).backward(dy.float().cpu())
    return [xr.grad, sr.grad] + [t.grad for t in p]


def check_dual_backward(dev, N, C, H, W, report):
    """folded pair (shortcut norm announced with later=True, applied by the closing norm) vs the old composition (two GroupNormFn, dres materialised) vs fp32 autograd: dx, dx_shortcut, dgamma / dbeta of both norms under the bounds
    tests/test_gpu_kernels.py::test_groupnorm_fused applies to groupnorm_bwd"""
    x, xs, (g, b), (g2, b2) = _dual_inputs(dev, N, C, H, W)
    dy = nhwc(rnd(N, C, H, W, seed=7), dev)
    ref = _autograd_reference(x, xs, g, b, g2, b2, dy)
    out = {}
    for name in ("fused", "fused-dres", "composed"):
        leaves = [t.clone().requires_grad_(True) for t in (x, xs, g, b, g2, b2)]
        xl, sl, gl, bl, g2l, b2l = leaves
        if name == "composed":
            y = ops.GroupNormFn.apply(xl, ops.GroupNormFn.apply(sl, None, g2l, b2l, EPS, False, False), gl, bl, EPS, True, False)
        else:
            alias = ops.GroupNormFn.apply(sl, None, g2l, b2l, EPS, False, False, None, None, False, False, None, True)      # later=True: applied by the consumer
            assert alias.data_ptr() == sl.data_ptr()
            y = ops.GroupNormFn.apply(xl, alias, gl, bl, EPS, True, False, None, None, False, name == "fused")      # lazy_res: no materialised shortcut gradient
        y.backward(dy)
        out[name] = (y.detach(), [t.grad for t in leaves])
    assert torch.equal(out["fused"][0].view(torch.int16), out["composed"][0].view(torch.int16)), "forward"
    assert torch.equal(out["fused-dres"][0].view(torch.int16), out["composed"][0].view(torch.int16)), "forward"
    tag = f"[{N}x{C}x{H}x{W}]"
    for name, (_, grads) in out.items():
        for what, got, want in zip(("dx", "dx_shortcut"), grads[:2], ref[:2]):
            report(f"groupnorm_dual_bwd.{what}[{name}]{tag}", got.float(), want, **tol(BF, 2))
        for k, what in ((2, "dgamma"), (3, "dbeta"), (4, "dgamma_shortcut"), (5, "dbeta_shortcut")):
            scale = max(1.0, ref[2 + 2 * (k // 4)].abs().max().item())          # (as test_groupnorm_fused: the scale of that norm's dgamma)
            report(f"groupnorm_dual_bwd.{what}[{name}]{tag}", grads[k], ref[k], rtol=2e-2, atol=3e-2 * scale)
    # new vs old directly: the same arithmetic up to the order of the fp32 atomics
    for k, what in enumerate(("dx", "dx_shortcut", "dgamma", "dbeta", "dgamma_shortcut", "dbeta_shortcut")):
        want = out["composed"][1][k]
        kw = tol(BF, 2) if k < 2 else dict(rtol=2e-2, atol=3e-2 * max(1.0, out["composed"][1][2 + 2 * (k // 4)].abs().max().item()))
        report(f"groupnorm_dual_bwd.{what}[fused vs composed]{tag}", out["fused"][1][k].float(), want.float(), **kw)


def watch_folds(monkeypatch):
    """counters of the WIRING: how often Bottleneck._shortcut deferred the shortcut's norm to the closing pass, how often the stem took the one-pass form"""
    from maed_amd import resnetv2
    seen = {"folded": 0, "unfolded": 0, "pool": 0}
    real_shortcut, real_pool = resnetv2.Bottleneck._shortcut, resnetv2.GroupNormAct.forward_pool

    def shortcut(self, x):
        r = real_shortcut(self, x)
        seen["folded" if r[1] else "unfolded"] += 1
        return r

    def pool(self, x):
        seen["pool"] += 1
        return real_pool(self, x)
    monkeypatch.setattr(resnetv2.Bottleneck, "_shortcut", shortcut)
    monkeypatch.setattr(resnetv2.GroupNormAct, "forward_pool", pool)
    return seen


def bottleneck_runs(dev, monkeypatch, in_chs, out_chs, stride, N, H, W):
    """one Bottleneck with a downsample shortcut in train mode, shortcut fusion on / on with materialised dres / off: {name: (y, {gradient name: tensor})}.
    The block stands alone, so its convolutions are the framework's: they are asked for their deterministic algorithms, the compared passes differ in the norms only"""
    from maed_amd import resnetv2
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    seen = watch_folds(monkeypatch)
    torch.manual_seed(3)
    blk = resnetv2.Bottleneck(in_chs, out_chs, stride=stride, downsample=True)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, resnetv2.GroupNormAct):
                m.weight.copy_(1 + 0.2 * rnd(m.num_channels, seed=11)); m.bias.copy_(0.1 * rnd(m.num_channels, seed=12))
    blk = blk.to(dev).train()
    x0 = nhwc(rnd(N, in_chs, H, W, seed=1), dev)
    dy = None
    out = {}
    blk(x0.clone().requires_grad_(True)).sum().backward()        # the framework's convolutions choose their algorithms in the first pass: all compared passes run alike
    for name, fuse, lazy in (("fused", True, True), ("fused-dres", True, False), ("composed", False, True)):
        monkeypatch.setattr(resnetv2, "_FUSE_SHORTCUT_NORM", fuse)
        monkeypatch.setattr(resnetv2, "_LAZY_SHORTCUT_DRES", lazy)
        seen.update(folded=0, unfolded=0)
        blk.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = blk(x)
        assert (seen["folded"], seen["unfolded"]) == ((1, 0) if fuse else (0, 1)), (name, seen)      # the path under test is the one that ran ...
        assert not ops.NORM_LATER, name                                                               # ... and the closing norm took the announced shortcut norm
        if dy is None:
            dy = nhwc(rnd(*y.shape, seed=9), dev)
        y.backward(dy)
        grads = {n: p.grad.detach().float().clone() for n, p in blk.named_parameters()}
        grads["input"] = x.grad.float()
        out[name] = (y.detach(), grads)
    return out


def check_bottleneck(out, report, tag):
    y_ref, g_ref = out["composed"]
    for name in ("fused", "fused-dres"):
        y, grads = out[name]
        differ = y != y_ref
        assert not differ.any(), (tag, name, "forward", int(differ.sum()), differ.numel(), (y.float() - y_ref.float()).abs().max().item(),
                                  "fused == fused-dres: %s" % torch.equal(out["fused"][0], out["fused-dres"][0]))
        assert set(grads) == set(g_ref)
        for n, got in grads.items():
            want = g_ref[n]
            # the input gradient under groupnorm_bwd's dx bound; every parameter gradient -- a sum over the pixels, as dgamma / dbeta -- under theirs
            kw = tol(BF, 2) if n == "input" else dict(rtol=2e-2, atol=3e-2 * max(1.0, want.abs().max().item()))
            report(f"bottleneck{tag}.{n}[{name} vs composed]", got, want, **kw)


SWITCHES = {"all on": (True, True, True), "stem off": (False, True, True), "shortcut off": (True, False, True), "shortcut dres off": (True, True, False),
            "all off (repeat)": (False, False, False), "all off": (False, False, False)}      # (repeat: the old path against itself -- the noise every row carries)


def backbone_run(dev, monkeypatch, switches, N, H, W):
    """a two-stage backbone (64 -> 256 stride 1, 256 -> 512 stride 2: both blocks have a downsample shortcut; at 64 x 64 frames the first block sees 16 x 16) in
    bf16 train mode on fp32 frames, on the product's own path (library convolutions, scratch arena, statistics from the convolution epilogues, direct gradients)
    under (_FUSE_STEM_POOL, _FUSE_SHORTCUT_NORM, _LAZY_SHORTCUT_DRES): (features, {parameter name: gradient, "<block>.input": gradient of that block's input})"""
    from maed_amd import resnetv2
    seen = watch_folds(monkeypatch)
    torch.manual_seed(3)
    net = resnetv2.ResNetV2(layers=(1, 1), channels=(256, 512), compute_dtype=BF)
    with torch.no_grad():
        for m in net._norms:
            m.weight.copy_(1 + 0.2 * rnd(m.num_channels, seed=11)); m.bias.copy_(0.1 * rnd(m.num_channels, seed=12))
    net = net.to(dev).train()
    for name, value in zip(("_FUSE_STEM_POOL", "_FUSE_SHORTCUT_NORM", "_LAZY_SHORTCUT_DRES"), switches):
        monkeypatch.setattr(resnetv2, name, value)
    grads = {}
    hooks = [m.register_forward_pre_hook(lambda mod, inp, n=n: inp[0].register_hook(lambda g, n=n: grads.__setitem__(n + ".input", g.detach().float().cpu())) and None)
             for n, m in net.named_modules() if isinstance(m, resnetv2.Bottleneck)]
    y = net(rnd(N, 3, H, W, seed=31).to(dev))
    for h in hooks:
        h.remove()
    assert (seen["pool"], seen["folded"], seen["unfolded"]) == (int(switches[0]), 2 * int(switches[1]), 2 * int(not switches[1])), (switches, seen)
    assert not ops.NORM_LATER
    y.backward(nhwc(rnd(*y.shape, seed=33), dev))
    assert len(grads) == 2, sorted(grads)
    grads.update({n: p.grad.detach().float().cpu() for n, p in net.named_parameters()})
    return y.detach(), grads


def check_backbone_runs(out, report):
    """Same feature bits under every switch setting, and the gradients against the all-off run.
    The stride-2 block (stages.1) comes FIRST in the backward, so every run hands it the same bits: its parameter gradients and its input gradient are held to the
    bounds tests/test_gpu_kernels.py::test_groupnorm_fused applies to groupnorm_bwd -- tol(bf16, 2) for the dx, rtol 2e-2 / atol 3e-2 * scale for gradients that
    are sums over the pixels (the norms' affine parameters; convolution weights are sums of the same kind).
    Everything behind it (stage 0, the stem) receives a dy that already differs from run to run: every GroupNorm backward sums through fp32 atomics, an occasional
    bf16 step of a dx element follows, the norms behind amplify it.  Measured on MI355X between two runs that execute IDENTICAL kernels on identical bits down to
    that point (stem fold on / off: stages.0.blocks.0.input): 7 of 32768 elements outside tol(bf16, 2), the largest off by 0.125 at a gradient scale of 17.9 --
    in one run of three, none in the others.  The dx bound per element cannot hold there for the OLD path against itself (the "all off (repeat)" row prints that
    noise each time), so those tensors, the input gradient of stage 0's block included, are held to the scale-relative bound of the summed gradients:
    rtol 2e-2, atol 3e-2 * max|reference| -- a mis-wired scratch slice, mask or saved tensor is off by the scale itself."""
    y0, g0 = out["all off"]
    for name, (y1, g1) in out.items():
        if name == "all off":
            continue
        differ = y1 != y0
        assert not differ.any(), (name, "features", int(differ.sum()), differ.numel())
        assert set(g1) == set(g0)
        for n, want in g0.items():
            kw = tol(BF, 2) if n == "stages.1.blocks.0.input" else dict(rtol=2e-2, atol=3e-2 * max(1.0, want.abs().max().item()))
            report(f"backbone.{n}[{name} vs all off]", g1[n], want, **kw)
