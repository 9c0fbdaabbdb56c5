"""Tap-resident 3x3 weight gradient (maed_amd/csrc/conv3x3_rows.hip: conv3x3_wgrad_taps_kernel, MAED_OPT_CONV3X3_WGRAD_TAPS) on the host simulator: channel counts
that are multiples of 64, R image rows per work item as one linear run of pixel slots, stride 1 and stride 2 (four phase images) -- through ops.conv3x3_wgrad /
ops.conv3x3_s2_wgrad against fp64 autograd through F.conv2d on the same bf16-rounded x, dy, with the product's bound for this gradient,
|got - ref| <= 2e-3 max|ref|.  Every case accumulates into a non-zero dW."""
import functools

import pytest
import torch
import torch.nn.functional as F

from maed_amd import _lib as L
from maed_amd import ops

from _hostsim import option, patched

FORCE = 2                       # the option's test value: the kernel whenever the shape allows; FORCE + n: with the work items cut into n chunks
GRIDS = [FORCE, FORCE + 1, FORCE + 2, FORCE + 5]


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def case(Fr, H, W, Cin, Cout, stride=1, pt=0, pl=0):
    """bf16 operands, the non-zero dW to accumulate into and the fp64 reference (dW0 + gradient), computed once per shape"""
    g = torch.Generator().manual_seed(1000 * H + 10 * W + Cin + stride + pt)
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W)
    x = cl(torch.randn(Fr, Cin, H, W, generator=g).bfloat16())
    dy = cl(torch.randn(Fr, Cout, Ho, Wo, generator=g).bfloat16())
    dW0 = torch.randn(Cout, 3, 3, Cin, generator=g)
    w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    if stride == 1:
        y = F.conv2d(x.double(), w, padding=1)
    else:
        pb, pr = (Ho - 1) * 2 + 3 - H - pt, (Wo - 1) * 2 + 3 - W - pl
        assert pb >= 0 and pr >= 0
        y = F.conv2d(F.pad(x.double(), [pl, pr, pt, pb]), w, stride=2)
    assert y.shape[-2:] == (Ho, Wo)
    y.backward(dy.double())
    ref = dW0.double() + w.grad.permute(0, 2, 3, 1)
    return x, dy, dW0, ref


def check(got, ref, dW0):
    grad = ref - dW0.double()
    err = (got.double() - ref).abs().max().item()
    bound = 2e-3 * grad.abs().max().item()
    print(f"max|got - ref| = {err:.3e}, bound = {bound:.3e}")
    assert err <= bound, (err, bound)


def run(lib, opt, Fr, H, W, Cin, Cout, stride=1, pt=0, pl=0, expect_taken=True):
    x, dy, dW0, ref = case(Fr, H, W, Cin, Cout, stride, pt, pl)
    dW = dW0.clone()
    with option(lib, L.OPT_CONV3X3_WGRAD_TAPS, opt):
        Ho, Wo = dy.shape[-2:]
        assert (lib.maed_conv3x3_wgrad_taps_scratch_floats(Fr, H, W, Cin, Cout, stride, Ho, Wo) > 0) == expect_taken
        if stride == 1:
            ops.conv3x3_wgrad(dy, x, out=dW)
        else:
            ops.conv3x3_s2_wgrad(dy, x, pt, pl, out=dW)
    check(dW, ref, dW0)
    return dW


S1 = [(2, 14, 14, 128, 128), (1, 14, 14, 256, 256), (2, 28, 28, 128, 128), (1, 16, 16, 128, 128), (1, 32, 32, 128, 128), (3, 3, 5, 128, 128), (2, 2, 14, 128, 128),
      (2, 6, 28, 64, 128), (2, 6, 28, 128, 64)]


@pytest.mark.parametrize("opt", GRIDS)
@pytest.mark.parametrize("Fr,H,W,Cin,Cout", S1)
def test_stride1_matches_fp64_autograd(Fr, H, W, Cin, Cout, opt):
    """whole frames per item (14 x 14, 16 x 16), several items per frame with a ragged last one (28 x 28: 7 rows; 32 x 32: 8), image borders, a W that fills no copy
    instruction (5, 14, 28), all 16 channel blocks at 256 channels, rectangular blocks; the default grid and 1 / 2 / 5 chunks of work items: workgroups walk item lists
    across frames and through ragged tails"""
    with patched() as lib:
        run(lib, opt, Fr, H, W, Cin, Cout)


def test_shape_outside_the_family_takes_the_general_kernel():
    with patched() as lib:
        run(lib, FORCE, 1, 8, 8, 64, 136, expect_taken=False)


def test_option_0_and_1_agree_within_the_bound():
    """(4096 output pixels: the default takes the new kernel)  Not bit-equal: the summation order differs"""
    with patched() as lib:
        new = run(lib, 1, 4, 32, 32, 64, 128)
        old = run(lib, 0, 4, 32, 32, 64, 128, expect_taken=False)
        x, dy, dW0, ref = case(4, 32, 32, 64, 128)
        assert (new.double() - old.double()).abs().max().item() <= 2e-3 * (ref - dW0.double()).abs().max().item()


def test_default_leaves_small_launches_to_the_general_kernel_and_takes_ragged_pixel_counts():
    with patched() as lib:
        run(lib, 1, 2, 14, 14, 128, 128, expect_taken=True)       # 392 pixels: no multiple of 64, the general kernel has no ragged tile
        run(lib, 1, 1, 8, 8, 128, 128, expect_taken=False)


S2 = [(2, 28, 28, 128, 128, 0, 0), (1, 8, 8, 128, 128, 0, 0), (1, 8, 8, 128, 128, 1, 1), (1, 9, 9, 128, 128, 1, 1)]


@pytest.mark.parametrize("opt", [FORCE, FORCE + 1])
@pytest.mark.parametrize("Fr,H,W,Cin,Cout,pt,pl", S2)
def test_stride2_matches_fp64_autograd(Fr, H, W, Cin, Cout, pt, pl, opt):
    """28 x 28 -> 14 x 14 and 8 x 8 -> 4 x 4 with the pads SAME gives an even input (0 / 0), 8 x 8 with the cnn encoder's 1 / 1, an odd input with SAME's 1 / 1; the
    default grid and a single workgroup per channel block"""
    with patched() as lib:
        run(lib, opt, Fr, H, W, Cin, Cout, 2, pt, pl)
