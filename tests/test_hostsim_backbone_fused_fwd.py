"""The backbone's one-pass forward forms on the host simulator (cases: tests/_backbone_fused_cases.py): the stem's GroupNorm + ReLU inside the max-pool and the
shortcut's GroupNorm inside the closing GroupNorm of a downsample block are bit for bit the kernel sequences they replace; the backward of the fused block norm
(two maed_groupnorm_bwd calls sharing dy and the ReLU bits, no materialised shortcut gradient) matches the two-Function composition and fp32 autograd."""
import pytest

import _backbone_fused_cases as K
from _hostsim import patched


@pytest.mark.parametrize("N,C,H,W", K.STEM_SHAPES)
def test_stem_norm_relu_pool_kernel_is_bit_equal_to_norm_then_pool(N, C, H, W):
    with patched():
        K.check_stem_kernel("cpu", N, C, H, W)


@pytest.mark.parametrize("N,C,H,W", K.STEM_SHAPES)
def test_stem_norm_relu_pool_function_matches_norm_then_pool(N, C, H, W):
    with patched():
        K.check_stem_function("cpu", N, C, H, W, K.report_quiet)


@pytest.mark.parametrize("N,C,H,W", K.DUAL_SHAPES)
def test_dual_norm_kernel_is_bit_equal_to_shortcut_norm_then_closing_norm(N, C, H, W):
    with patched():
        K.check_dual_kernel("cpu", N, C, H, W)


@pytest.mark.parametrize("N,C,H,W", K.DUAL_SHAPES)
def test_dual_norm_backward_matches_composition_and_autograd(N, C, H, W):
    with patched():
        K.check_dual_backward("cpu", N, C, H, W, K.report_quiet)


@pytest.mark.parametrize("in_chs,out_chs,stride", [(64, 256, 1), (256, 512, 2)])
def test_bottleneck_with_downsample_fused_and_composed(monkeypatch, in_chs, out_chs, stride):
    """(the simulator's size: 2 frames of 8 x 8)"""
    with patched():
        out = K.bottleneck_runs("cpu", monkeypatch, in_chs, out_chs, stride, 2, 8, 8)
    K.check_bottleneck(out, K.report_quiet, f"[{in_chs}->{out_chs},s{stride}]")


def test_backbone_is_the_same_under_every_switch(monkeypatch):
    """ResNetV2's own wiring (stem route, downsample blocks of stride 1 and 2, scratch arena, direct gradients) with each fusion switched off in turn: same
    feature bits, parameter and block-input gradients within the groupnorm_bwd bounds"""
    with patched():
        out = {name: K.backbone_run("cpu", monkeypatch, sw, 2, 32, 32) for name, sw in K.SWITCHES.items()}
    K.check_backbone_runs(out, K.report_quiet)
