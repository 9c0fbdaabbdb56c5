"""The backbone's one-pass forward forms on the GPU (cases: tests/_backbone_fused_cases.py, the same as tests/test_hostsim_backbone_fused_fwd.py): the stem's
GroupNorm + ReLU inside the max-pool and the shortcut's GroupNorm inside the closing GroupNorm of a downsample block are bit for bit the kernel sequences they
replace; the backward of the fused block norm matches the two-Function composition and fp32 autograd under the bounds of test_gpu_kernels.py::test_groupnorm_fused."""
import pytest

import _backbone_fused_cases as K
from _util import DEV, report

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,C,H,W", K.STEM_SHAPES)
def test_stem_norm_relu_pool_kernel_is_bit_equal_to_norm_then_pool(N, C, H, W):
    K.check_stem_kernel(DEV, N, C, H, W)


@pytest.mark.parametrize("N,C,H,W", K.STEM_SHAPES)
def test_stem_norm_relu_pool_function_matches_norm_then_pool(N, C, H, W):
    K.check_stem_function(DEV, N, C, H, W, report)


@pytest.mark.parametrize("N,C,H,W", K.DUAL_SHAPES)
def test_dual_norm_kernel_is_bit_equal_to_shortcut_norm_then_closing_norm(N, C, H, W):
    K.check_dual_kernel(DEV, N, C, H, W)


@pytest.mark.parametrize("N,C,H,W", K.DUAL_SHAPES)
def test_dual_norm_backward_matches_composition_and_autograd(N, C, H, W):
    K.check_dual_backward(DEV, N, C, H, W, report)


@pytest.mark.parametrize("in_chs,out_chs,stride", [(64, 256, 1), (256, 512, 2)])
def test_bottleneck_with_downsample_fused_and_composed(monkeypatch, in_chs, out_chs, stride):
    out = K.bottleneck_runs(DEV, monkeypatch, in_chs, out_chs, stride, 2, 16, 16)
    K.check_bottleneck(out, report, f"[{in_chs}->{out_chs},s{stride}]")


def test_backbone_is_the_same_under_every_switch(monkeypatch):
    """ResNetV2's own wiring on 2 frames of 64 x 64: the block 64 -> 256 (stride 1) at 16 x 16 and the block 256 -> 512 (stride 2) behind it, stem route, scratch
    arena, statistics from the convolution epilogues, direct gradients -- with each fusion switched off in turn: same feature bits, parameter and block-input gradients
    within the groupnorm_bwd bounds"""
    out = {name: K.backbone_run(DEV, monkeypatch, sw, 2, 64, 64) for name, sw in K.SWITCHES.items()}
    K.check_backbone_runs(out, report)
