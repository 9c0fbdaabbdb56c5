"""maed_grad_norm / maed_opt_step on the device (fp64 references and bit-identity statements of docs/design/15_optimizers.md; cases shared with the simulator suite in
tests/_optim_cases.py) and clipped FusedSGD steps on the small model of tests/test_gpu_graph.py."""
import pytest
import torch

import _optim_cases as K

pytestmark = pytest.mark.gpu
GUARD = 64


def _dev():
    return torch.device("cuda", 0)


def _guarded(t, fill=K.SENTINEL):
    """t on the device between two guard zones of 64 sentinel elements -> (whole buffer, the 256-B aligned interior view)"""
    buf = torch.full((t.numel() + 2 * GUARD,), fill, dtype=t.dtype, device=_dev())
    buf[GUARD:GUARD + t.numel()] = t.to(_dev())
    return buf, buf[GUARD:GUARD + t.numel()]


def _guards_intact(buf, n, fill=K.SENTINEL):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


@pytest.mark.parametrize("gscale", K.NORM_GSCALES)
@pytest.mark.parametrize("n", K.NORM_SIZES)
def test_grad_norm_against_fp64(n, gscale):
    from maed_amd import ops
    g_host = K.norm_input(n, seed=n)
    g = g_host.to(_dev())
    partials = torch.empty(ops.grad_norm_partials(), dtype=torch.float32, device=_dev())
    rec = ops.clip_record(_dev())
    sq = K.ref_sqnorm(g_host, gscale)
    norm = sq ** 0.5
    bits = []
    for max_norm in (0.5 * norm, 2.0 * norm, None):          # binding, not binding, no bound; three calls: the same bits every time
        ops.grad_norm(g, gscale, max_norm, partials, rec)
        got_sq, got_norm, coef, flag = K.read_record(rec)
        bits.append(rec[:2].cpu().view(torch.int32).tolist())
        print(f"n={n} gscale={gscale}: norm {got_norm!r} against {norm!r} (rel {abs(got_norm - norm) / norm:.2e}), coef {coef!r}")
        assert abs(got_norm - norm) <= K.NORM_RTOL * norm and flag == 0
        want = K.ref_coef(norm, max_norm)
        assert abs(coef - want) <= K.NORM_RTOL * want
        assert coef == 1.0 if (max_norm is None or max_norm > norm) else coef < 0.51
    assert bits[0] == bits[1] == bits[2], "sqnorm must not depend on the arrival order of the workgroups"


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_grad_norm_flags_a_non_finite_gradient(bad):
    from maed_amd import ops
    g = K.norm_input(65537).to(_dev())
    partials = torch.empty(ops.grad_norm_partials(), dtype=torch.float32, device=_dev())
    rec = ops.clip_record(_dev())
    ops.grad_norm(g, 1.0, 1.0, partials, rec)
    assert K.read_record(rec)[3] == 0
    g[40000] = bad
    ops.grad_norm(g, 1.0, 1.0, partials, rec)
    assert K.read_record(rec)[3] == 1


RULES = [(K.ADAM, False, 0.9), (K.ADAMW, False, 0.9), (K.SGD, False, 0.9), (K.SGD, True, 0.9), (K.SGD, False, 0.0)]


@pytest.mark.parametrize("n", K.STEP_SIZES)
@pytest.mark.parametrize("kind,nesterov,momentum", RULES)
def test_one_step_of_each_rule_against_fp64(kind, nesterov, momentum, n):
    from maed_amd import ops
    p, g, m, v = K.step_inputs(n, seed=kind)
    h = dict(K.HYPER, momentum=momentum)
    pb, pd = _guarded(p)
    mb, md = _guarded(m)
    vb, vd = _guarded(v)
    sb, sd = _guarded(torch.zeros(n, dtype=torch.bfloat16))
    gd = g.to(_dev())
    no_buffer = kind == K.SGD and momentum == 0.0          # SGD without momentum needs no buffer: m may be NULL
    ops.opt_step(kind, pd, gd, None if no_buffer else md, None if kind == K.SGD else vd, sd, lr=h["lr"], beta1=h["beta1"], beta2=h["beta2"], eps=h["eps"],
                 wd=h["wd"], step=h["step"], momentum=momentum, nesterov=nesterov, gscale=h["gscale"])
    torch.cuda.synchronize()
    rp, rm, rv = K.ref_step(kind, p, g, m, v, nesterov=nesterov, **h)
    for name, got, want in (("p", pd, rp), ("m", md, rm), ("v", vd, rv)):
        err = (got.double().cpu() - want).abs()
        print(f"kind={kind} n={n} {name}: max abs err {float(err.max()):.3e}")
        assert torch.allclose(got.double().cpu(), want, rtol=K.STEP_RTOL, atol=K.STEP_ATOL), name
    assert torch.equal(sd, pd.bfloat16()), "the bf16 shadow is the rounded new parameter"
    assert not torch.equal(pd.cpu(), p)
    for buf in (pb, mb, vb, sb):
        assert _guards_intact(buf, n)


def _flat(n, seed=0):
    return [t.to(_dev()) for t in K.step_inputs(n, seed)]


@pytest.mark.parametrize("with_record", [False, True])
def test_kind_adam_equals_adam_step_bit_for_bit(with_record):
    from maed_amd import ops, _lib as L
    n, h = 1000003, K.HYPER
    p, g, m, v = _flat(n)
    pa, ma, va = p.clone(), m.clone(), v.clone()
    pb, mb, vb = p.clone(), m.clone(), v.clone()
    st = None
    if with_record:
        st = ops.DeviceTrainState(_dev())
        st.set_hyper(h["lr"], 1.0 - h["beta1"] ** h["step"], 1.0 - h["beta2"] ** h["step"])
        st.upload()
        ops.adam_step_dev(pa, g, ma, va, None, st.dev, h["beta1"], h["beta2"], h["eps"], h["wd"], gscale=h["gscale"])
    else:
        ops.adam_step(pa, g, ma, va, None, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], h["step"], gscale=h["gscale"])
    ops.opt_step(L.OPT_ADAM, pb, g, mb, vb, None, lr=0.0 if with_record else h["lr"], beta1=h["beta1"], beta2=h["beta2"], eps=h["eps"], wd=h["wd"], step=h["step"],
                 gscale=h["gscale"], state=None if st is None else st.dev)
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb) and not torch.equal(pa, p)


@pytest.mark.parametrize("kind", [K.ADAM, K.ADAMW, K.SGD])
def test_a_clip_that_does_not_bind_changes_no_bit(kind):
    from maed_amd import ops
    n, h = 1000003, K.HYPER
    p, g, m, v = _flat(n, seed=kind)
    partials = torch.empty(ops.grad_norm_partials(), dtype=torch.float32, device=_dev())
    rec = ops.clip_record(_dev())
    ops.grad_norm(g, h["gscale"], 1e30, partials, rec)
    out = []
    for clip in (None, rec):
        q, mq, vq = p.clone(), m.clone(), v.clone()
        ops.opt_step(kind, q, g, mq, vq, None, lr=h["lr"], beta1=h["beta1"], beta2=h["beta2"], eps=h["eps"], wd=h["wd"], step=h["step"], momentum=h["momentum"],
                     gscale=h["gscale"], clip=clip)
        out.append((q, mq, vq))
    torch.cuda.synchronize()
    assert K.read_record(rec)[2] == 1.0
    for a, b in zip(*out):
        assert torch.equal(a, b)
    # and one that binds scales the gradient: the same step as gscale * coef handed in as the scale
    ops.grad_norm(g, h["gscale"], 1.0, partials, rec)
    coef = K.read_record(rec)[2]
    assert 0 < coef < 0.01
    q, mq, vq = p.clone(), m.clone(), v.clone()
    ops.opt_step(kind, q, g, mq, vq, None, lr=h["lr"], beta1=h["beta1"], beta2=h["beta2"], eps=h["eps"], wd=h["wd"], step=h["step"], momentum=h["momentum"],
                 gscale=h["gscale"], clip=rec)
    rp, _, _ = K.ref_step(kind, p, g, m, v, coef=coef, **h)
    assert torch.allclose(q.double().cpu(), rp, rtol=K.STEP_RTOL, atol=K.STEP_ATOL)


@pytest.mark.parametrize("kind", [K.ADAM, K.ADAMW, K.SGD])
def test_37_ragged_segments_equal_per_segment_launches_and_leave_the_gaps_alone(kind):
    from maed_amd import ops
    n, h = 1000003, K.HYPER
    segs = K.ragged_segments(n, 37)
    assert segs[1][0] == segs[1][1] and sum(1 for _, e, _, _ in segs if e % 4) > 20 and segs[-1][1] == n
    inside = K.covered(n, segs).to(_dev())
    assert 0 < int(inside.sum()) < n
    p, g, m, v = K.step_inputs(n, seed=kind)
    g = g.to(_dev())
    bufs = [_guarded(t) for t in (p, m, v)]
    for _, view in bufs:
        view[~inside] = K.SENTINEL             # between the segments: sentinels as well
    (pb, pd), (mb, md), (vb, vd) = bufs
    p0, m0, v0 = pd.clone(), md.clone(), vd.clone()
    # one launch per segment (a slice starts at a multiple of 4 elements: 16-B aligned), what FusedAdam's per-group path used to issue
    pe, me, ve = p0.clone(), m0.clone(), v0.clone()
    for b, e, lr, wd in segs:
        if e > b:
            if kind == K.ADAM:
                ops.adam_step(pe[b:e], g[b:e], me[b:e], ve[b:e], None, lr, h["beta1"], h["beta2"], h["eps"], wd, h["step"], gscale=h["gscale"])
            else:
                ops.opt_step(kind, pe[b:e], g[b:e], me[b:e], ve[b:e], None, lr=lr, beta1=h["beta1"], beta2=h["beta2"], eps=h["eps"], wd=wd, step=h["step"],
                             momentum=h["momentum"], gscale=h["gscale"])
    tab = ops.opt_segments(segs, _dev())
    ops.opt_step(kind, pd, g, md, vd, None, lr=123.0, beta1=h["beta1"], beta2=h["beta2"], eps=h["eps"], wd=456.0, step=h["step"], momentum=h["momentum"],
                 gscale=h["gscale"], segments=tab, n_segments=len(segs))
    torch.cuda.synchronize()
    assert torch.equal(pd, pe) and torch.equal(md, me) and (kind == K.SGD or torch.equal(vd, ve))
    assert not torch.equal(pd[inside], p0[inside])
    for got, was, buf in ((pd, p0, pb), (md, m0, mb), (vd, v0, vb)):
        assert torch.equal(got[~inside], was[~inside]) and bool((got[~inside] == K.SENTINEL).all()), "elements outside every segment are not touched"
        assert _guards_intact(buf, n)


def test_clipped_sgd_steps_on_the_small_model():
    """the small model of tests/test_gpu_graph.py under FusedSGD(momentum=0.9, max_grad_norm=...): the bound comes from an unclipped step and binds, grad_norm is
    the norm torch computes over the same gradients, tensors without a gradient stay where they are"""
    import maed_amd
    from maed_amd.ddp import FusedSGD, GradBucketer, ParamArena
    from maed_amd.loss import LossVideo
    dev = _dev()
    torch.manual_seed(0)
    model = maed_amd.MAED(num_blocks=2, num_heads=2, embed_dim=128, hidden_dim=256, img_size=64, max_seqlen=16, compute_dtype=torch.bfloat16).to(dev)
    model.train()
    arena = ParamArena(model)
    bucketer = GradBucketer(arena, model)
    gen = torch.Generator().manual_seed(5)
    n, T = 2, 4
    clip = torch.randn(n, T, 3, 64, 64, generator=gen).to(dev)
    r = lambda *s: torch.randn(*s, generator=gen)
    tgt = {k: v.to(dev) for k, v in dict(kp_2d=torch.cat([r(n, T, 49, 2) * 0.3, torch.rand(n, T, 49, 1, generator=gen)], -1),
                                         kp_3d=torch.cat([r(n, T, 49, 3) * 0.3, torch.ones(n, T, 49, 1)], -1),
                                         theta=torch.cat([r(n, T, 3) * 0.1, r(n, T, 72) * 0.2, r(n, T, 10)], -1),
                                         w_smpl=(torch.rand(n, T, generator=gen) > 0.2).float()).items()}
    crit = LossVideo(e_loss_weight=300.0, e_3d_loss_weight=600.0, e_pose_loss_weight=60.0, e_shape_loss_weight=0.06, e_smpl_norm_loss=1.0, e_smpl_accl_loss=0.0)

    def backward(opt):
        opt.zero_grad()
        loss, _ = crit(model(clip), tgt, None)
        loss.backward()
        return float(loss.detach())

    probe = FusedSGD(arena, lr=0.0, bucketer=bucketer, max_grad_norm=1e30)      # lr = 0: the parameters stay put, the record holds the unclipped norm
    backward(probe)
    probe.step()
    n0 = float(probe.grad_norm)
    assert n0 > 0 and int(probe.grad_nonfinite) == 0
    bound = 0.2 * n0
    opt = FusedSGD(arena, lr=0.04 / n0, momentum=0.9, bucketer=bucketer, max_grad_norm=bound)
    p0 = arena.flat.detach().clone()
    losses = []
    for _ in range(3):
        losses.append(backward(opt))
        want = float(torch.linalg.vector_norm(arena.grad.double()))          # the reduced gradients the step is about to read (world 1)
        opt.step()
        skipped = list(bucketer.unmarked)
        got = float(opt.grad_norm)
        print(f"loss {losses[-1]:.4f} grad_norm {got!r} against {want!r}, bound {bound!r}, {len(skipped)} tensors without a gradient")
        assert abs(got - want) <= K.NORM_RTOL * want and got > bound and int(opt.grad_nonfinite) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(arena.flat).all() and not torch.equal(arena.flat, p0) and losses[-1] < losses[0]
    # every step moved the parameter vector by at most lr * (1 + 0.9 + 0.81) * bound
    assert float((arena.flat - p0).norm()) <= 1.01 * (0.04 / n0) * (1 + 1.9 + 2.71) * bound
    for i in skipped:
        o, k = arena.offsets[i], arena.params[i].numel()
        assert torch.equal(arena.flat[o:o + k], p0[o:o + k]), arena.names[i]
