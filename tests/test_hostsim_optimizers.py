"""FusedSGD / FusedAdamW / global-norm clipping / the segment launch (maed_grad_norm, maed_opt_step through the host simulator) against torch.optim.SGD, AdamW and
torch.nn.utils.clip_grad_norm_, built as the reference builds its optimizer (lib/utils/utils.py:120-135: one group per tensor; train.py:123-127: LambdaLR;
trainer.py:330-368: checkpoints carry optimizer.state_dict()).  The device side of the same statements: tests/test_gpu_optimizers.py."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from maed_amd import _lib as L
from maed_amd import ops
from maed_amd.ddp import FusedAdam, FusedAdamW, FusedSGD, GradBucketer, ParamArena, no_decay_groups

from _hostsim import patched
import _optim_cases as K
from _optim_cases import Tiny, TinyWithUnused, named_groups, warm

HERE = os.path.dirname(os.path.abspath(__file__))
RTOL, ATOL = K.STEP_RTOL, K.STEP_ATOL


def _step(m, o, x, y, ref=False, clip=None):
    o.zero_grad(set_to_none=True) if ref else o.zero_grad()
    ((m(x) - y) ** 2).mean().backward()
    norm = torch.nn.utils.clip_grad_norm_(m.parameters(), clip) if (ref and clip is not None) else None
    o.step()
    return norm


def _assert_params_close(model, ref_model):
    for (n, p), (_, q) in zip(model.named_parameters(), ref_model.named_parameters()):
        assert torch.allclose(p, q, rtol=RTOL, atol=ATOL), (n, float((p - q).abs().max()))


def _assert_params_equal(model, other):
    for (n, p), (_, q) in zip(model.named_parameters(), other.named_parameters()):
        assert torch.equal(p, q), (n, float((p - q).abs().max()))


@pytest.mark.parametrize("momentum,nesterov,wd", [(0.0, False, 0.0), (0.9, False, 0.0), (0.9, True, 1e-3)])
def test_fused_sgd_matches_torch_sgd_with_lambda_lr_and_checkpoints(momentum, nesterov, wd):
    torch.manual_seed(0)
    ref_model = Tiny()
    model = copy.deepcopy(ref_model)
    x, y = torch.randn(16, 6), torch.randn(16, 5)
    ref_opt = torch.optim.SGD(lr=1e-1, params=named_groups(ref_model), momentum=momentum, nesterov=nesterov, weight_decay=wd)      # utils.py:122-126
    ref_sched = torch.optim.lr_scheduler.LambdaLR(ref_opt, lr_lambda=warm)
    with patched():
        arena = ParamArena(model)
        opt = FusedSGD(arena, lr=1e-1, momentum=momentum, nesterov=nesterov, weight_decay=wd, model=model)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=warm)
        assert isinstance(opt, torch.optim.Optimizer) and [g["name"] for g in opt.param_groups] == [n for n, _ in model.named_parameters()]
        assert opt.state_dict()["state"] == {}, "tensors that never stepped have no state"
        for epoch in range(6):
            _step(ref_model, ref_opt, x, y, ref=True)
            _step(model, opt, x, y)
            ref_sched.step()
            sched.step()
            assert abs(opt.param_groups[0]["lr"] - ref_opt.param_groups[0]["lr"]) < 1e-12
            if epoch == 2:   # checkpoint hand-over in both directions, mid-run
                sd_ref, sd = ref_opt.state_dict(), opt.state_dict()
                assert sd["param_groups"][0].keys() >= {"lr", "momentum", "dampening", "weight_decay", "nesterov", "params", "name"}
                assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in sd_ref["param_groups"]]
                assert sd["state"].keys() == sd_ref["state"].keys() and (len(sd["state"]) == (6 if momentum else 0))
                for i in sd_ref["state"]:
                    assert torch.allclose(sd["state"][i]["momentum_buffer"], sd_ref["state"][i]["momentum_buffer"], rtol=RTOL, atol=ATOL)
                ref_opt.load_state_dict(copy.deepcopy(sd))          # torch SGD resumes from OUR state
                opt.load_state_dict(copy.deepcopy(sd_ref))          # we resume from torch SGD's state
        _assert_params_close(model, ref_model)


class TinyNoDecay(Tiny):
    def no_weight_decay(self):
        return {"decoder.weight"}


@pytest.mark.parametrize("groups", ["uniform", "no_decay"])
def test_fused_adamw_matches_torch_adamw_in_one_launch_per_step(groups):
    torch.manual_seed(0)
    ref_model = TinyNoDecay()
    model = copy.deepcopy(ref_model)
    x, y = torch.randn(16, 6), torch.randn(16, 5)
    ref_opt = torch.optim.AdamW(lr=1e-2, params=named_groups(ref_model), weight_decay=0.1)
    ref_sched = torch.optim.lr_scheduler.LambdaLR(ref_opt, lr_lambda=warm)
    with patched() as lib:
        calls, real = [], lib.maed_opt_step

        def counting(*a):
            calls.append(1)
            return real(*a)
        lib.maed_opt_step = counting
        try:
            arena = ParamArena(model)
            opt = FusedAdamW(arena, lr=1e-2, weight_decay=0.1, model=model)
            sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=warm)
            if groups == "no_decay":
                changed = no_decay_groups(opt, model)
                assert sorted(changed) == sorted(["decoder.weight"] + [n for n, p in model.named_parameters() if p.ndim == 1])
                for g in ref_opt.param_groups:                      # the same groups in torch
                    if g["name"] in changed:
                        g["weight_decay"] = 0.0
                assert {g["weight_decay"] for g in opt.param_groups} == {0.0, 0.1}
            for epoch in range(6):
                _step(ref_model, ref_opt, x, y, ref=True)
                _step(model, opt, x, y)
                assert len(calls) == epoch + 1, "one maed_opt_step launch per step, whatever the groups"
                ref_sched.step()
                sched.step()
                if epoch == 2:
                    sd_ref, sd = ref_opt.state_dict(), opt.state_dict()
                    for i in sd_ref["state"]:
                        assert torch.allclose(sd["state"][i]["exp_avg"], sd_ref["state"][i]["exp_avg"], rtol=1e-5, atol=1e-8)
                        assert float(sd["state"][i]["step"]) == float(sd_ref["state"][i]["step"])
                    ref_opt.load_state_dict(copy.deepcopy(sd))
                    opt.load_state_dict(copy.deepcopy(sd_ref))
                    assert opt.step_count == 3 and all(g["decoupled_weight_decay"] for g in ref_opt.param_groups)
        finally:
            lib.maed_opt_step = real
        _assert_params_close(model, ref_model)


def _ours(kind, model, **kw):
    if kind == "sgd":
        return FusedSGD(ParamArena(model), lr=5e-2, momentum=0.9, model=model, **kw)
    return FusedAdam(ParamArena(model), lr=1e-2, weight_decay=1e-3, model=model, **kw)


def _torchs(kind, model):
    """the same hyper-parameters in torch, built as the reference builds it"""
    if kind == "sgd":
        return torch.optim.SGD(lr=5e-2, params=named_groups(model), momentum=0.9)
    return torch.optim.Adam(lr=1e-2, params=named_groups(model), weight_decay=1e-3)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_clipping_matches_clip_grad_norm_when_it_binds_and_when_it_does_not(kind):
    torch.manual_seed(0)
    base = Tiny()
    x, y = torch.randn(16, 6), 3.0 * torch.randn(16, 5)
    # six steps under the LambdaLR of the Adam test, as every comparison against torch here
    def torch_run(clip):
        m = copy.deepcopy(base)
        o = _torchs(kind, m)
        sched = torch.optim.lr_scheduler.LambdaLR(o, lr_lambda=warm)
        norms = []
        for _ in range(6):
            norms.append(float(_step(m, o, x, y, ref=True, clip=clip)))
            sched.step()
        return m, norms
    # the bound comes from the reference run: the median norm of an unclipped torch run
    max_norm = float(np.median(torch_run(1e30)[1]))
    # first, on the torch arm alone: the bound binds on some of the six steps and not on others
    ref_model, ref_norms = torch_run(max_norm)
    assert any(n > max_norm for n in ref_norms) and any(n <= max_norm for n in ref_norms), (max_norm, ref_norms)
    model = copy.deepcopy(base)
    with patched():
        opt = _ours(kind, model, max_grad_norm=max_norm)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=warm)
        assert opt.grad_norm.shape == () and opt.grad_nonfinite.dtype == torch.int32
        for ref_norm in ref_norms:
            _step(model, opt, x, y)
            sched.step()
            assert abs(float(opt.grad_norm) - ref_norm) <= K.NORM_RTOL * ref_norm, (float(opt.grad_norm), ref_norm)
            assert int(opt.grad_nonfinite) == 0
    _assert_params_close(model, ref_model)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_a_clip_that_never_binds_changes_no_bit(kind):
    """coef == 1 exactly; for Adam the unclipped arm is maed_adam_step, the clipped one maed_opt_step: the two kernels share their per-element arithmetic"""
    torch.manual_seed(3)
    base = Tiny()
    plain, clipped = copy.deepcopy(base), copy.deepcopy(base)
    x, y = torch.randn(16, 6), torch.randn(16, 5)
    with patched():
        o_plain, o_clip = _ours(kind, plain), _ours(kind, clipped, max_grad_norm=1e30)
        for _ in range(4):
            _step(plain, o_plain, x, y)
            _step(clipped, o_clip, x, y)
        assert float(o_clip.grad_norm) > 0 and read_coef(o_clip) == 1.0
    _assert_params_equal(clipped, plain)


def read_coef(opt):
    return K.read_record(opt._clip)[2]


def test_segment_launch_equals_per_tensor_launches_bit_for_bit():
    """the per-group case of tests/test_hostsim_optim.py: FusedAdam now serves it with ONE maed_opt_step over a segment table; one maed_adam_step per tensor (what
    it used to issue) gives the same bits"""
    torch.manual_seed(1)
    base = Tiny()
    seg_model, per_model = copy.deepcopy(base), copy.deepcopy(base)
    x, y = torch.randn(8, 6), torch.randn(8, 5)
    with patched() as lib:
        calls, real = [], lib.maed_opt_step

        def counting(*a):
            calls.append(1)
            return real(*a)
        lib.maed_opt_step = counting
        try:
            opt = FusedAdam(ParamArena(seg_model), lr=1e-2, weight_decay=1e-3, model=seg_model)
            opt.param_groups[1]["lr"] = 3e-3
            opt.param_groups[2]["weight_decay"] = 0.0
            a = ParamArena(per_model)
            m, v = torch.zeros_like(a.flat), torch.zeros_like(a.flat)
            hyper = {g["name"]: (g["lr"], g["weight_decay"]) for g in opt.param_groups}
            for t in range(1, 4):
                _step(seg_model, opt, x, y)
                a.zero_grad()
                ((per_model(x) - y) ** 2).mean().backward()
                for name, p, o in zip(a.names, a.params, a.offsets):
                    n = p.numel()
                    ops.adam_step(a.flat[o:o + n], a.grad[o:o + n], m[o:o + n], v[o:o + n], None, hyper[name][0], 0.9, 0.999, 1e-8, hyper[name][1], t)
            assert len(calls) == 3
        finally:
            lib.maed_opt_step = real
        assert torch.equal(opt.exp_avg, m) and torch.equal(opt.exp_avg_sq, v)
    _assert_params_equal(seg_model, per_model)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_parameters_without_a_gradient_are_left_alone(kind):
    """torch leaves a parameter whose .grad is None alone; with weight decay 0.1 any touch would show"""
    torch.manual_seed(1)
    ref_model = TinyWithUnused()
    model = copy.deepcopy(ref_model)
    x, y = torch.randn(8, 6), torch.randn(8, 5)
    if kind == "sgd":
        ref_opt = torch.optim.SGD(lr=1e-2, params=named_groups(ref_model), momentum=0.9, weight_decay=0.1)
    else:
        ref_opt = torch.optim.AdamW(lr=1e-2, params=named_groups(ref_model), weight_decay=0.1)
    with patched():
        arena = ParamArena(model)
        bucketer = GradBucketer(arena, model)
        opt = (FusedSGD(arena, lr=1e-2, momentum=0.9, weight_decay=0.1, bucketer=bucketer) if kind == "sgd"
               else FusedAdamW(arena, lr=1e-2, weight_decay=0.1, bucketer=bucketer))
        for _ in range(3):
            _step(ref_model, ref_opt, x, y, ref=True)
            _step(model, opt, x, y)
        assert len(opt.state_dict()["state"]) == len(ref_opt.state_dict()["state"]) == 6, "the spare tensors never stepped: no state"
    _assert_params_close(model, ref_model)
    torch.manual_seed(1)
    fresh = TinyWithUnused()
    for (n, p), (_, q) in zip(model.named_parameters(), fresh.named_parameters()):
        if "spare" in n:
            assert torch.equal(p, q), f"{n} must not have been touched"


@pytest.mark.parametrize("with_record", [False, True])
def test_opt_step_kind_adam_equals_adam_step_bit_for_bit(with_record):
    n = 1027
    p, g, m, v = K.step_inputs(n)
    h = K.HYPER
    with patched():
        pa, ma, va = p.clone(), m.clone(), v.clone()
        pb, mb, vb = p.clone(), m.clone(), v.clone()
        st = None
        if with_record:
            st = ops.DeviceTrainState(torch.device("cpu"))
            st.set_hyper(h["lr"], 1.0 - h["beta1"] ** h["step"], 1.0 - h["beta2"] ** h["step"])
            st.upload()
            ops.adam_step_dev(pa, g, ma, va, None, st.dev, h["beta1"], h["beta2"], h["eps"], h["wd"], gscale=h["gscale"])
        else:
            ops.adam_step(pa, g, ma, va, None, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], h["step"], gscale=h["gscale"])
        ops.opt_step(L.OPT_ADAM, pb, g, mb, vb, None, lr=0.0 if with_record else h["lr"], beta1=h["beta1"], beta2=h["beta2"], eps=h["eps"], wd=h["wd"],
                     step=h["step"], gscale=h["gscale"], state=None if st is None else st.dev)
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb) and not torch.equal(pa, p)


@pytest.mark.parametrize("n", K.NORM_SIZES[:-1])
def test_grad_norm_on_the_simulator_against_fp64(n):
    g = K.norm_input(n, seed=n)
    with patched():
        partials, rec = torch.zeros(ops.grad_norm_partials()), ops.clip_record(torch.device("cpu"))
        for gscale in K.NORM_GSCALES:
            sq = K.ref_sqnorm(g, gscale)
            norm = sq ** 0.5
            for max_norm in (0.5 * norm, 2.0 * norm, None):
                ops.grad_norm(g, gscale, max_norm, partials, rec)
                got_sq, got_norm, coef, flag = K.read_record(rec)
                assert abs(got_norm - norm) <= K.NORM_RTOL * norm and abs(got_sq - sq) <= 2 * K.NORM_RTOL * sq and flag == 0
                want = K.ref_coef(norm, max_norm)
                assert abs(coef - want) <= K.NORM_RTOL * want and (max_norm is None or max_norm < norm or coef == 1.0)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_grad_norm_flags_a_non_finite_gradient(bad):
    g = K.norm_input(1025)
    g[777] = bad
    with patched():
        partials, rec = torch.zeros(ops.grad_norm_partials()), ops.clip_record(torch.device("cpu"))
        ops.grad_norm(g, 1.0, 1.0, partials, rec)
        assert K.read_record(rec)[3] == 1
        g[777] = 1.0
        ops.grad_norm(g, 1.0, 1.0, partials, rec)
        assert K.read_record(rec)[3] == 0


@pytest.mark.parametrize("kind", [K.ADAM, K.ADAMW, K.SGD])
def test_segment_edges_empty_segments_ragged_ends_and_gaps(kind):
    n = 2051
    segs = K.ragged_segments(n, 5)
    assert segs[1][0] == segs[1][1] and any(e % 4 for _, e, _, _ in segs) and all(b % 4 == 0 for b, _, _, _ in segs)
    inside = K.covered(n, segs)
    assert 0 < int(inside.sum()) < n
    p, g, m, v = K.step_inputs(n, seed=kind)
    for t in (p, m, v):
        t[~inside] = K.SENTINEL            # the gaps: must come back untouched
    h = dict(K.HYPER)
    with patched():
        tab = ops.opt_segments(segs, torch.device("cpu"))
        po, mo, vo = p.clone(), m.clone(), v.clone()
        shadow = torch.full((n,), K.SENTINEL, dtype=torch.bfloat16)
        ops.opt_step(kind, po, g, mo, vo, shadow, lr=123.0, beta1=h["beta1"], beta2=h["beta2"], eps=h["eps"], wd=456.0, step=h["step"], momentum=h["momentum"],
                     gscale=h["gscale"], segments=tab, n_segments=len(segs))
    for t, t0 in ((po, p), (mo, m), (vo, v)):
        assert torch.equal(t[~inside], t0[~inside]), "elements outside every segment are not touched"
    assert torch.equal(shadow[~inside].float(), torch.full((int((~inside).sum()),), K.SENTINEL)) and torch.equal(shadow[inside], po[inside].bfloat16())
    for b, e, lr, wd in segs:           # every segment with its own lr / weight_decay
        hp = dict(h, lr=lr, wd=wd)
        rp, rm, rv = K.ref_step(kind, p[b:e], g[b:e], m[b:e], v[b:e], **hp)
        assert torch.allclose(po[b:e].double(), rp, rtol=RTOL, atol=ATOL)
        if kind != K.SGD:
            assert torch.allclose(vo[b:e].double(), rv, rtol=RTOL, atol=ATOL)
        assert torch.allclose(mo[b:e].double(), rm, rtol=RTOL, atol=ATOL)


def test_get_optimizer_restates_the_reference():
    from maed_amd import trainer
    m = Tiny()
    with patched():
        arena = ParamArena(m)
        for name in ("sgd", "SGD"):
            o = trainer.get_optimizer(arena, name, 0.1, 0.5, 0.9, model=m)
            assert isinstance(o, FusedSGD) and o.param_groups[0]["momentum"] == 0.9 and o.param_groups[0]["weight_decay"] == 0.0   # utils.py:122-126 passes no decay
        for name in ("Adam", "adam", "ADAM"):
            o = trainer.get_optimizer(arena, name, 0.1, 0.5, 0.9, model=m, max_grad_norm=1.0)
            assert isinstance(o, FusedAdam) and not o.decoupled and o.param_groups[0]["weight_decay"] == 0.5 and o.max_grad_norm == 1.0
        for name in ("adamw", "Sgd", "rmsprop"):
            with pytest.raises(ModuleNotFoundError):
                trainer.get_optimizer(arena, name, 0.1, 0.5, 0.9)
        with pytest.raises(ValueError):
            FusedSGD(arena, lr=0.1, momentum=0.9, dampening=0.1)
        o = FusedSGD(arena, lr=0.1, momentum=0.9)
        o.param_groups[0]["dampening"] = 0.5
        with pytest.raises(ValueError):
            o.step()


def test_vision_transformer_declares_its_no_decay_names():
    from maed_amd.vision_transformer import VisionTransformer
    vit = VisionTransformer(img_size=32, embed_dim=64, depth=1, num_heads=1, num_classes=0, hybrid_backbone=nn.Conv2d(3, 8, 16, 16), compute_dtype=torch.float32)
    assert vit.no_weight_decay() == {"pos_embed", "cls_token"}          # vision_transformer.py:378-379
    wrapper = nn.ModuleDict({"encoder": vit})
    with patched():
        opt = FusedAdamW(ParamArena(wrapper), lr=1e-3, weight_decay=0.05)
        changed = set(no_decay_groups(opt, wrapper))
    assert {"encoder.pos_embed", "encoder.cls_token"} <= changed
    for g in opt.param_groups:
        p = g["params"][0]
        assert g["weight_decay"] == (0.0 if (p.ndim <= 1 or g["name"] in ("encoder.pos_embed", "encoder.cls_token")) else 0.05), g["name"]


# ---- two gloo ranks ------------------------------------------------------------------------------------------------------------------------------------------
def _world2_batch():
    g = torch.Generator().manual_seed(7)
    return torch.randn(16, 6, generator=g), 3.0 * torch.randn(16, 5, generator=g)


def _world2_model():
    torch.manual_seed(11)
    return Tiny()


def _worker(rank, world, port, max_norm, out):
    import torch.distributed as dist
    sys.path.insert(0, HERE)
    from _hostsim import patched
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        with patched():
            model = _world2_model()
            arena = ParamArena(model, device=torch.device("cpu"))
            bucketer = GradBucketer(arena, model, bucket_bytes=128)
            assert bucketer.collectives and len(bucketer.buckets) > 1
            opt = FusedSGD(arena, lr=5e-2, momentum=0.9, bucketer=bucketer, model=model, max_grad_norm=max_norm)
            x, y = _world2_batch()
            shard = slice(rank * 8, rank * 8 + 8)
            norms = []
            for _ in range(3):
                opt.zero_grad()
                ((model(x[shard]) - y[shard]) ** 2).mean().backward()
                opt.step()
                norms.append(float(opt.grad_norm))
            out[rank] = (arena.flat.clone(), norms)
    finally:
        dist.destroy_process_group()


def test_two_ranks_clip_the_averaged_gradient_and_stay_in_step():
    import torch.multiprocessing as mp
    sys.path.insert(0, os.path.join(HERE, "hostsim"))
    import build_sim
    build_sim.build()
    # the averaged gradient of two equal shards is the whole batch's gradient
    model = _world2_model()
    x, y = _world2_batch()
    ((model(x) - y) ** 2).mean().backward()
    want = float(torch.nn.utils.clip_grad_norm_(model.parameters(), 1e30))
    max_norm = 0.5 * want                                   # binds
    world = 2
    port = 31733 + os.getpid() % 1000
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, max_norm, out), nprocs=world, join=True)
    (flat0, norms0), (flat1, norms1) = out[0], out[1]
    assert norms0 == norms1, "both ranks see the norm of the same reduced gradient"
    assert abs(norms0[0] - want) <= K.NORM_RTOL * want, (norms0[0], want)
    assert torch.equal(flat0, flat1), "parameters stay equal across ranks after three clipped steps"
    assert not torch.equal(flat0, ParamArena(_world2_model(), device=torch.device("cpu")).flat)
