"""GPU tests of the stage-1 encoder (MAED(encoder='cnn')): the BatchNorm / pooling kernels of csrc/batchnorm.hip against fp64 torch on the dtype-rounded inputs,
the torchvision-padded stem and stride-2 3x3 convolutions on the library's kernels, and the whole model against the fp64 restatement of torchvision's ResNet-50
(tests/_resnet50_ref.py) in train mode, eval mode and a short training loop."""
import copy

import pytest
import torch
import torch.nn.functional as F

import _batchnorm_cases as K
import _resnet50_ref as RR
from _util import DEV, note, q, report, rnd, tol

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]


def _ops():
    from maed_amd import ops
    return ops


def _bn_gpu(case, relu, training=True):
    """one case of tests/_batchnorm_cases through the ops wrappers (statistics, apply, backward) on the GPU; dgamma / dbeta accumulate into the case's start values"""
    ops = _ops()
    x2, dy2 = case["x2"].to(DEV), case["dy2"].to(DEV)
    res2 = case["res2"].to(DEV) if case["res2"] is not None else None
    gamma, beta = case["gamma"].to(DEV), case["beta"].to(DEV)
    rm, rv = case["rm"].to(DEV).clone(), case["rv"].to(DEV).clone()
    dgamma, dbeta = case["dgamma0"].to(DEV).clone(), case["dbeta0"].to(DEV).clone()
    if training:
        mean, rstd, mean_lo = ops.batchnorm_stats(x2, K.EPS, rm, rv, K.MOMENTUM)
    else:
        mean, rstd, mean_lo = rm.clone(), torch.rsqrt(rv + K.EPS), None
    y, mask = ops.batchnorm_apply(x2, mean, rstd, gamma, beta, res2, relu, want_mask=True)
    assert (mask is not None) == (relu and res2 is not None)
    dx, dres = ops.batchnorm_bwd(x2, dy2, mean, rstd, gamma, beta, mask, relu, frozen=not training, dgamma=dgamma, dbeta=dbeta, want_dres=res2 is not None, mean_lo=mean_lo)
    torch.cuda.synchronize()
    return dict(y=y, dx=dx, dres=dres, dgamma=dgamma, dbeta=dbeta, rm=rm, rv=rv)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [False, True], ids=["norelu", "relu"])
@pytest.mark.parametrize("shape", K.BN_SHAPES, ids=str)
def test_batchnorm_train_forward_backward(shape, relu, res, dtype):
    case = K.case(shape, dtype, res)
    got = _bn_gpu(case, relu)
    K.check_bn(f"bn {shape} {IDS[DTYPES.index(dtype)]} res={res} relu={relu}", got, K.reference(shape, dtype, res, relu), dtype)
    again = _bn_gpu(case, relu)
    for k, v in got.items():
        assert v is None or torch.equal(v, again[k]), f"{k}: two runs differ"


def test_batchnorm_shapes_span_several_row_chunks():
    from maed_amd import _lib as L
    assert L.lib().maed_batchnorm_chunks(4 * 40 * 40) == 200 and L.lib().maed_batchnorm_chunks(3 * 21 * 21) == 42 and (3 * 21 * 21) % 32 == 11


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 64, 7, 9), (3, 256, 5, 5)], ids=str)
def test_batchnorm_eval_forward_and_frozen_backward(shape, dtype):
    for res, relu in ((False, True), (True, True), (False, False)):
        got = _bn_gpu(K.case(shape, dtype, res), relu, training=False)
        K.check_bn(f"bn eval {shape} res={res} relu={relu}", got, K.reference(shape, dtype, res, relu, training=False), dtype, training=False)


def test_batchnorm_function_through_autograd():
    """ops.BatchNormFn: the autograd wiring on the GPU (the kernels' arithmetic is covered above)"""
    ops = _ops()
    c = K.case((2, 64, 7, 9), torch.bfloat16, True)
    ref = K.reference((2, 64, 7, 9), torch.bfloat16, True, True)
    x = c["x"].to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    r = c["res"].to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    g, b = c["gamma"].to(DEV).requires_grad_(True), c["beta"].to(DEV).requires_grad_(True)
    rm, rv = c["rm"].to(DEV).clone(), c["rv"].to(DEV).clone()
    y = ops.BatchNormFn.apply(x, r, g, b, (rm, rv), True, K.MOMENTUM, K.EPS, True)
    y.backward(c["dy"].to(DEV))
    report("BatchNormFn y", K.rows(y), ref["y"], **tol(torch.bfloat16, 4))
    report("BatchNormFn dx", K.rows(x.grad), ref["dx"], **tol(torch.bfloat16, 2))
    report("BatchNormFn dres", K.rows(r.grad), ref["dres"], **tol(torch.bfloat16, 2))
    report("BatchNormFn dgamma", g.grad, ref["dgamma"] - c["dgamma0"].double(), **K.affine_tol(torch.bfloat16, ref["dgamma"]))
    report("BatchNormFn running_var", rv, ref["rv"], rtol=1e-5, atol=2e-7)


def _pool_input(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, shape, generator=g).float()          # integer values: many ties
    x[0, 3, shape[2] // 2, shape[3] // 2] = float("nan")
    return x.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 64, 9, 12), (1, 64, 7, 7), (2, 64, 16, 16)], ids=str)
def test_maxpool3s2p1(shape, dtype):
    ops = _ops()
    x = _pool_input(shape, dtype, 5)
    ref = F.max_pool2d(x.float(), 3, 2, 1)
    dy = q(rnd(*ref.shape, seed=6), dtype)
    xg = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ops.MaxPool3s2P1Fn.apply(xg)
    y.backward(dy.to(DEV).to(dtype))
    yf = y.float().cpu()
    assert yf.shape == ref.shape
    assert torch.equal(torch.isnan(yf), torch.isnan(ref)) and torch.equal(torch.nan_to_num(yf, nan=123.0), torch.nan_to_num(ref, nan=123.0))
    x64 = x.double().requires_grad_(True)
    F.max_pool2d(x64, 3, 2, 1).backward(dy.double())
    report(f"maxpool3s2p1 dx {shape} {dtype}", xg.grad, x64.grad, **tol(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C_", [64, 2048])
@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (7, 7)], ids=["hw1", "hw4", "hw49"])
def test_global_avgpool(hw, C_, dtype):
    ops = _ops()
    x = q(rnd(3, C_, *hw, seed=C_ + hw[0]), dtype)
    dy = rnd(3, C_, seed=9)
    xg = x.to(DEV).to(dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ops.GlobalAvgPoolFn.apply(xg)
    y.backward(dy.to(DEV))
    assert y.dtype == torch.float32
    report(f"avgpool y {hw} {C_} {dtype}", y, x.double().mean((2, 3)), **tol(dtype))
    report(f"avgpool dx {hw} {C_} {dtype}", xg.grad, (dy.double() / (hw[0] * hw[1]))[:, :, None, None].expand(3, C_, *hw), **tol(dtype))


def test_stem_with_padding_3_through_the_models_stem_path():
    """torchvision's conv1 (7x7, stride 2, padding 3) on maed_stem7x7s2_*: the same kernel on an image padded (3, 2, 3, 3) into the (H + 5, W + 6, 4) buffer"""
    from maed_amd.resnet import resnet50
    torch.manual_seed(3)
    enc = resnet50(compute_dtype=torch.bfloat16).to(DEV).train()
    x = rnd(2, 3, 64, 64, seed=1)
    assert dict(enc.plan(2, 64, 64)["convs"])["conv1"] == "stem"
    seen = {}

    def grab(mod, inputs, output):
        seen.update(route=mod._route, y=output.detach().clone())
        output.register_hook(lambda g: seen.update(dy=g.detach().clone()))

    hook = enc.conv1.register_forward_hook(grab)
    out = enc(x.to(DEV))
    out.float().square().mean().backward()
    hook.remove()
    assert seen["route"] == "stem"
    w = q(enc.conv1.weight.detach().cpu(), torch.bfloat16).double().requires_grad_(True)
    ref = F.conv2d(q(x, torch.bfloat16).double(), w, None, stride=2, padding=3)
    report("stem padding 3 fwd (2,3,64,64)", seen["y"].float(), ref, **tol(torch.bfloat16, 2))
    dy = seen["dy"].float().cpu()
    ref.backward(dy.double())
    report("stem padding 3 dw (2,3,64,64)", enc.conv1.weight.grad, w.grad, rtol=2e-3, atol=2e-3 * w.grad.abs().max().item())


@pytest.mark.parametrize("N,C_,H,W", [(4, 64, 8, 8), (1, 128, 16, 16), (2, 64, 6, 10)])
def test_conv3x3_stride2_padding1(N, C_, H, W):
    """ops.Conv3x3S2P1Fn (conv2 of layer2..4's first blocks): even sizes are where zero padding 1 differs from TF-SAME; (2, 64, 6, 10): 30 output rows, the weight
    gradient takes the framework's backward inside the Function"""
    ops = _ops()
    O = 2 * C_
    x = q(rnd(N, C_, H, W, seed=1), torch.bfloat16)
    w = q(rnd(O, C_, 3, 3, seed=2, scale=(9 * C_) ** -0.5), torch.bfloat16)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ref = F.conv2d(xd, wd, None, 2, 1)
    dy = q(rnd(*ref.shape, seed=3), torch.bfloat16)
    ref.backward(dy.double())
    img = w.to(DEV).bfloat16().permute(0, 2, 3, 1).contiguous()                 # (O, 3, 3, I)
    wt = img.view(O, -1).t().contiguous()
    dw = torch.ones(O, 9 * C_, dtype=torch.float32, device=DEV)
    xg = x.to(DEV).bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ops.Conv3x3S2P1Fn.apply(xg, img.permute(0, 3, 1, 2), wt, dw, None)
    y.backward(dy.to(DEV).bfloat16())
    ops.side_stream_join(torch.device(DEV))
    torch.cuda.synchronize()
    tag = f"[{N}x{C_}x{H}x{W}]"
    report(f"conv3x3 s2 p1 fwd{tag}", y.float(), ref, **tol(torch.bfloat16, 2))
    report(f"conv3x3 s2 p1 dx{tag}", xg.grad.float(), xd.grad, **tol(torch.bfloat16, 2))
    got = (dw - 1.0).view(O, 3, 3, C_).permute(0, 3, 1, 2)
    report(f"conv3x3 s2 p1 dw{tag}", got, wd.grad, rtol=2e-3, atol=2e-3 * wd.grad.abs().max().item())


# ---- model level -------------------------------------------------------------------------------------------------------------------------------------------
CLIP = (2, 8, 3, 64, 64)        # 16 frames: layer4 has 16 * 2 * 2 = 64 rows, so the library convolutions run at every stage


def _fresh(dtype, seed=11):
    from maed_amd.maed import MAED
    torch.manual_seed(seed)
    m = MAED(encoder="cnn", compute_dtype=dtype)
    RR.randomise(m.encoder, seed)
    m.decoder.drop1.p = 0.0
    m.decoder.drop2.p = 0.0
    return m


@pytest.fixture(scope="module")
def oracle():
    """fp64 restatement + the project's decoder on the CPU, train mode: computed once, shared by the model-level tests"""
    m = _fresh(torch.float32).train()
    clip = rnd(*CLIP, seed=21)
    ref = RR.reference_of(m.encoder)
    dec = copy.deepcopy(m.decoder)
    feat, out = RR.forward_with_decoder(ref, dec, clip)
    RR.loss_of(out).backward()
    ref.eval()
    dec.eval()
    with torch.no_grad():
        feat_eval, out_eval = RR.forward_with_decoder(ref, dec, clip)      # eval mode on the buffers the train-mode forward left
    return dict(state=copy.deepcopy(m.state_dict()), clip=clip, feat=feat.detach(), out={k: out[k].detach() for k in RR.OUT_KEYS},
                enc_grad=torch.cat([p.grad.flatten() for p in ref.parameters()]), feat_eval=feat_eval, out_eval={k: out_eval[k] for k in RR.OUT_KEYS})


def _dist(got, ref, rtol, atol):
    """elementwise distance in units of the bar atol + rtol |ref|: <= 1 passes"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and not torch.isnan(got).any()
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())


def _run_arm(oracle, dtype, lib_bn, monkeypatch):
    from maed_amd import resnet
    monkeypatch.setattr(resnet, "_LIB_BN", lib_bn)
    m = _fresh(dtype)
    m.load_state_dict(oracle["state"])
    m = m.to(DEV).train()
    clip = oracle["clip"].to(DEV)
    with torch.no_grad():
        feat = copy.deepcopy(m).extract_feature(clip)
    out = m(clip)
    RR.loss_of(out).backward()
    g = torch.cat([p.grad.detach().double().cpu().flatten() for p in m.encoder.parameters()])
    cos = float(F.cosine_similarity(g, oracle["enc_grad"], dim=0))
    m.eval()
    with torch.no_grad():
        feat_eval, out_eval = m.extract_feature(clip), m(clip)
    torch.cuda.synchronize()
    return dict(model=m, feat=feat, out=out, one_minus_cos=1.0 - cos, feat_eval=feat_eval, out_eval=out_eval)


def test_model_f32_train_and_eval_match_the_restatement(oracle, monkeypatch):
    """compute_dtype = float32: convolutions on the framework's fp32 engine, BatchNorm and pools on the library; the project's small-model bars"""
    r = _run_arm(oracle, torch.float32, True, monkeypatch)
    report("cnn f32 extract_feature", r["feat"], oracle["feat"], rtol=1e-3, atol=1e-4)
    for k in RR.OUT_KEYS:
        report(f"cnn f32 train {k}", r["out"][k], oracle["out"][k], rtol=1e-3, atol=1e-4)
    report("cnn f32 1 - cosine(encoder gradient, fp64)", torch.tensor([r["one_minus_cos"]]), torch.zeros(1), rtol=0, atol=2e-3)
    report("cnn f32 eval extract_feature", r["feat_eval"], oracle["feat_eval"], rtol=1e-3, atol=1e-4)
    for k in RR.OUT_KEYS:
        report(f"cnn f32 eval {k}", r["out_eval"][k], oracle["out_eval"][k], rtol=1e-3, atol=1e-4)


def test_model_bf16_train_and_eval_match_the_restatement(oracle, monkeypatch):
    """bf16: both arms -- library BatchNorm / pools, and MAED_CNN_BN=torch -- against fp64 at the bars of test_backbone_gemm_convolutions_match_miopen_path
    (rtol 5e-2, atol 5e-2 max|ref|; encoder gradient 1 - cos <= 0.1).  Where the framework arm itself misses a bar, the library arm must stay within twice the
    framework arm's distance."""
    lib = _run_arm(oracle, torch.bfloat16, True, monkeypatch)
    fw = _run_arm(oracle, torch.bfloat16, False, monkeypatch)
    rows = []
    for mode, fk, ok in (("train", "feat", "out"), ("eval", "feat_eval", "out_eval")):
        quantities = [("extract_feature", lib[fk], fw[fk], oracle[fk])] + [(k, lib[ok][k], fw[ok][k], oracle[ok][k]) for k in RR.OUT_KEYS]
        for name, a, b, ref in quantities:
            bar = dict(rtol=5e-2, atol=5e-2 * float(ref.abs().max()))
            rows.append((f"cnn bf16 {mode} {name}", _dist(a, ref, **bar), _dist(b, ref, **bar), 1.0))
    rows.append(("cnn bf16 1 - cosine(encoder gradient, fp64)", lib["one_minus_cos"], fw["one_minus_cos"], 0.1))
    failures = []
    for name, d_lib, d_fw, bar in rows:
        limit = bar if d_fw <= bar else 2.0 * d_fw
        report(name + " [framework arm, logged]", torch.tensor([d_fw]), torch.zeros(1), rtol=0, atol=float("inf"))
        try:
            report(name + f" [library arm, limit {limit:.3g}]", torch.tensor([d_lib]), torch.zeros(1), rtol=0, atol=limit)
        except AssertionError as e:
            failures.append(f"{name}: library {d_lib:.3g} framework {d_fw:.3g} limit {limit:.3g} ({e})")
    assert not failures, "\n".join(failures)


def test_training_loop_lowers_the_loss_and_moves_the_running_buffers():
    import maed_amd
    from maed_amd import ops
    from maed_amd.ddp import FusedAdam, GradBucketer, ParamArena
    m = _fresh(torch.bfloat16, seed=13).to(DEV).train()
    before = {k: v.clone() for k, v in m.encoder.state_dict().items() if "running" in k}
    arena = ParamArena(m)
    opt = FusedAdam(arena, lr=1e-4, weight_decay=1e-5, bucketer=GradBucketer(arena, m, bucket_bytes=1 << 20))
    clip = rnd(2, 8, 3, 64, 64, seed=31).to(DEV)
    tgt = rnd(2, 8, 49, 3, seed=32).to(DEV) * 0.1
    rebuilds0 = ops.WeightImageFn.rebuilds
    losses = []
    for _ in range(4):
        opt.zero_grad()
        out = m(clip)
        loss = ((out["kp_3d"] - tgt) ** 2).mean() + 1e-3 * (out["theta"] ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    note(f"cnn training loop losses: {losses}")
    assert all(torch.isfinite(torch.tensor(losses))), losses
    assert losses[-1] < losses[0], losses
    after = m.encoder.state_dict()
    assert all(not torch.equal(after[k], v) for k, v in before.items())
    assert int(after["bn1.num_batches_tracked"]) == 4
    assert ops.WeightImageFn.rebuilds - rebuilds0 == 4, "weight images are rebuilt once per optimizer step"
    assert all(p.grad.data_ptr() >= arena.grad.data_ptr() for p in arena.params)
    assert maed_amd.device_faults() == 0
