"""MAED(encoder='cnn') on the CPU composition: the stage-1 encoder (maed_amd/resnet.py) against the fp64 restatement of torchvision's ResNet-50
(tests/_resnet50_ref.py) -- state dict, SyncBatchNorm conversion, forward / backward parity, and the host-side kernel selection at the stage-1 size."""
import copy
import os

import pytest
import torch

os.environ.setdefault("MAED_SYNTHETIC_SMPL_OK", "1")

import _resnet50_ref as RR


def _model(seed=0, **kw):
    from maed_amd.maed import MAED
    torch.manual_seed(seed)
    m = MAED(encoder="cnn", compute_dtype=torch.float32, **kw)
    RR.randomise(m.encoder, seed)
    return m


@pytest.fixture(scope="module")
def model():
    return _model()


def test_state_dict_is_torchvisions(model):
    from maed_amd.resnet import resnet50
    enc = resnet50()
    sd, ref_sd = enc.state_dict(), RR.RefResNet50().state_dict()
    assert list(sd) == list(ref_sd)
    assert all(sd[k].shape == ref_sd[k].shape and sd[k].dtype == ref_sd[k].dtype for k in sd)
    assert len(sd) == 318 == 53 + 53 * 5
    assert sum(k.endswith("conv1.weight") or k.endswith("conv2.weight") or k.endswith("conv3.weight") or k.endswith("downsample.0.weight") for k in sd) == 53
    assert sum(p.numel() for p in enc.parameters() if p.requires_grad) == 23_508_032 == 25_557_032 - 2_049_000
    RR.RefResNet50().load_state_dict(sd, strict=True)
    enc.load_state_dict(ref_sd, strict=True)
    full = model.state_dict()
    assert all("encoder." + k in full for k in sd)
    assert isinstance(enc.fc, torch.nn.Identity) and enc.num_features == 2048
    for name in ("conv1", "bn1", "layer1", "layer2", "layer3", "layer4", "avgpool", "fc"):
        assert hasattr(enc, name)
    assert [len(getattr(enc, f"layer{i}")) for i in (1, 2, 3, 4)] == [3, 4, 6, 3]
    assert enc.layer2[0].conv2.stride == (2, 2) and enc.layer2[0].conv1.stride == (1, 1)
    assert enc.bn1.eps == 1e-5 and enc.bn1.momentum == 0.1


def test_initialisation_is_torchvisions():
    from maed_amd.resnet import resnet50
    torch.manual_seed(1)
    enc = resnet50()
    w = enc.layer3[2].conv2.weight
    assert abs(float(w.detach().std()) / (2.0 / (256 * 9)) ** 0.5 - 1) < 0.02          # Kaiming normal, fan_out
    assert all(bool((m.weight == 1).all()) and bool((m.bias == 0).all()) for m in enc._norms)
    with pytest.raises(NotImplementedError, match="network access"):
        resnet50(pretrained=True)


def test_unknown_encoder_still_raises():
    from maed_amd.maed import MAED
    with pytest.raises(NotImplementedError):
        MAED(encoder="mlp")


def test_sync_batchnorm_conversion_leaves_the_norm_modules(model):
    from maed_amd.resnet import BatchNorm2d
    m = copy.deepcopy(model)
    before = sum(isinstance(x, BatchNorm2d) for x in m.modules())
    conv = torch.nn.SyncBatchNorm.convert_sync_batchnorm(m)
    assert before == 53 and sum(isinstance(x, BatchNorm2d) for x in conv.modules()) == 53
    assert not any(isinstance(x, torch.nn.modules.batchnorm._BatchNorm) for x in conv.modules())


def test_training_with_one_value_per_channel_raises():
    from maed_amd.resnet import BatchNorm2d
    bn = BatchNorm2d(8)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        bn(torch.randn(1, 8, 1, 1))
    bn.eval()
    bn(torch.randn(1, 8, 1, 1))


def _cos(a, b):
    return float(torch.nn.functional.cosine_similarity(a.double().flatten(), b.double().flatten(), dim=0))


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_forward_and_backward_match_the_restatement(train):
    m = _model(seed=2)
    m.train(train)
    m.decoder.drop1.p = 0.0
    m.decoder.drop2.p = 0.0
    clip = torch.randn(2, 2, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    ref = RR.reference_of(m.encoder)
    dec = copy.deepcopy(m.decoder)
    feat_ref, out_ref = RR.forward_with_decoder(ref, dec, clip)
    RR.loss_of(out_ref).backward()
    feat = m.extract_feature(clip) if not train else None
    if train:       # extract_feature on a copy: a second train-mode forward would move the running buffers twice
        feat = copy.deepcopy(m).extract_feature(clip)
    out = m(clip)
    RR.loss_of(out).backward()
    a = float(feat_ref.detach().abs().max())
    torch.testing.assert_close(feat.double(), feat_ref, rtol=1e-4, atol=1e-4 * a)
    for k in RR.OUT_KEYS:
        torch.testing.assert_close(out[k].double(), out_ref[k].double(), rtol=1e-4, atol=1e-4 * float(out_ref[k].detach().abs().max()))
    if train:
        sd, rsd = m.encoder.state_dict(), ref.state_dict()
        for k in sd:
            if k.endswith("running_var"):
                torch.testing.assert_close(sd[k].double(), rsd[k], rtol=1e-5, atol=0, msg=lambda s, k=k: f"{k}: {s}")
            elif k.endswith("running_mean"):
                # rtol 1e-5 -- of the value, or of the channel's spread where the mean itself is (almost) zero: a convolution output's mean has no scale of its own
                spread = rsd[k.replace("running_mean", "running_var")].sqrt()
                bad = (sd[k].double() - rsd[k]).abs() > 1e-5 * (rsd[k].abs() + spread)
                assert not bad.any(), f"{k}: {int(bad.sum())} channels off"
            elif k.endswith("num_batches_tracked"):
                assert int(sd[k]) == int(rsd[k]) == 1, k
    rp = dict(ref.named_parameters())
    for name, p in m.encoder.named_parameters():
        assert p.grad is not None, name
        c = _cos(p.grad, rp[name].grad)
        assert c >= 1 - 2e-3, f"encoder.{name}: 1 - cos = {1 - c:.3e}"
    dp = dict(dec.named_parameters())
    for name, p in m.decoder.named_parameters():
        if p.grad is None:
            assert dp[name].grad is None, name
            continue
        c = _cos(p.grad, dp[name].grad)
        assert c >= 1 - 2e-3, f"decoder.{name}: 1 - cos = {1 - c:.3e}"


def test_stage1_shapes_qualify_for_the_library():
    """config_stage1.yaml: 128 frames of 224 x 224 per GPU, bf16: every one of the 53 convolutions, 53 BatchNorms and both pools takes a library kernel"""
    from maed_amd.resnet import resnet50
    plan = resnet50(compute_dtype=torch.bfloat16).plan(128, 224, 224)
    assert len(plan["convs"]) == 53 and len(plan["norms"]) == 53 and len(plan["pools"]) == 2
    assert 128 * 7 * 7 == 98 * 64 and (112 * 112) % 128 == 0 and 112 % 16 == 0
    routes = dict(plan["convs"])
    assert routes["conv1"] == "stem"
    assert all(r != "aten" for r in routes.values()), [n for n, r in routes.items() if r == "aten"]
    assert [n for n, r in routes.items() if r == "conv3x3s2"] == ["layer2.0.conv2", "layer3.0.conv2", "layer4.0.conv2"]
    assert sum(r == "conv3x3" for r in routes.values()) == 13 and sum(r == "gemm" for r in routes.values()) == 36
    assert all(ok for _, ok in plan["norms"]) and all(ok for _, ok in plan["pools"])
    # fp32 on the exact engine: convolutions on the framework, BatchNorm and pools still on the library
    plan32 = resnet50(compute_dtype=torch.float32).plan(128, 224, 224)
    assert all(r == "aten" for _, r in plan32["convs"]) and all(ok for _, ok in plan32["norms"])
    # a frame count whose last stage is no multiple of the 64-row tile: those convolutions fall back, the rest do not
    small = dict(resnet50(compute_dtype=torch.bfloat16).plan(4, 64, 64)["convs"])
    assert small["layer4.1.conv1"] == "aten" and small["layer1.0.conv1"] == "gemm"


def test_bn_knob_switches_to_the_framework_composition(monkeypatch):
    from maed_amd import resnet
    monkeypatch.setattr(resnet, "_LIB_BN", False)
    bn = resnet.BatchNorm2d(8)
    x = torch.randn(2, 8, 3, 3)
    ref = torch.nn.BatchNorm2d(8)
    torch.testing.assert_close(bn(x, relu=True), torch.relu(ref(x)))
