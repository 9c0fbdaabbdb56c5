"""Tap-resident 3x3 weight gradient (maed_amd/csrc/conv3x3_rows.hip: conv3x3_wgrad_taps_kernel, MAED_OPT_CONV3X3_WGRAD_TAPS) on the device, through
ops.conv3x3_wgrad / ops.conv3x3_s2_wgrad: the stage-2 / stage-3 shapes of cfg3, cfg5's 16 x 16, a tiny ragged one, and the stride-2 forms with SAME's and the cnn
encoder's pads -- against fp64 autograd through F.conv2d on the same bf16-rounded x, dy, |got - ref| <= 2e-3 max|ref|, accumulating into a non-zero dW; at the
default option, at the test value (2: the kernel whenever the shape allows) and, one shape per stride, at 0 (the general TN kernels).  The host simulator's
tests/test_hostsim_conv3x3_wgrad_taps.py covers the item / grid geometry; this is the same arithmetic on the hardware."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _util import DEV  # noqa: E402


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def case(Fr, H, W, C, stride=1, pt=0, pl=0):
    """bf16 operands on the device, the non-zero dW to accumulate into and the fp64 gradient (device), computed once per shape"""
    g = torch.Generator().manual_seed(1000 * H + 10 * W + C + stride + pt)
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W)
    x = cl(torch.randn(Fr, C, H, W, generator=g).bfloat16().to(DEV))
    dy = cl(torch.randn(Fr, C, Ho, Wo, generator=g).bfloat16().to(DEV))
    dW0 = torch.randn(C, 3, 3, C, generator=g).to(DEV)
    w = torch.zeros(C, C, 3, 3, dtype=torch.float64, device=DEV, requires_grad=True)
    if stride == 1:
        y = F.conv2d(x.double(), w, padding=1)
    else:
        pb, pr = (Ho - 1) * 2 + 3 - H - pt, (Wo - 1) * 2 + 3 - W - pl
        assert pb >= 0 and pr >= 0
        y = F.conv2d(F.pad(x.double(), [pl, pr, pt, pb]), w, stride=2)
    assert y.shape[-2:] == (Ho, Wo)
    y.backward(dy.double())
    return x, dy, dW0, w.grad.permute(0, 2, 3, 1).contiguous()


def run(opt, Fr, H, W, C, stride=1, pt=0, pl=0):
    from maed_amd import _lib as L
    from maed_amd import ops
    lib = L.lib()
    x, dy, dW0, grad = case(Fr, H, W, C, stride, pt, pl)
    dW = dW0.clone()
    old = lib.maed_get_option(L.OPT_CONV3X3_WGRAD_TAPS)
    try:
        assert lib.maed_set_option(L.OPT_CONV3X3_WGRAD_TAPS, opt) == 0
        taken = lib.maed_conv3x3_wgrad_taps_scratch_floats(Fr, H, W, C, C, stride, dy.shape[-2], dy.shape[-1]) > 0
        M = Fr * dy.shape[-2] * dy.shape[-1]   # the default takes >= 4096 output pixels, and pixel counts the general kernel has no tile for (no multiple of 64)
        assert taken == (opt >= 2 or (opt == 1 and (M >= 4096 or M % 64 != 0)))
        if stride == 1:
            ops.conv3x3_wgrad(dy, x, out=dW)
        else:
            ops.conv3x3_s2_wgrad(dy, x, pt, pl, out=dW)
        torch.cuda.synchronize()            # raises if the device reported an error
    finally:
        lib.maed_set_option(L.OPT_CONV3X3_WGRAD_TAPS, old)
    err = (dW.double() - dW0.double() - grad).abs().max().item()
    bound = 2e-3 * grad.abs().max().item()
    print(f"conv3x3 wgrad taps[{Fr}x{C}x{H}x{W} s{stride} pads {pt}/{pl} opt {opt}]: max|got - ref| = {err:.3e}, bound = {bound:.3e}")
    assert err <= bound, (err, bound)
    assert L.device_faults() == 0


@pytest.mark.parametrize("opt", [1, 2])
@pytest.mark.parametrize("Fr,H,W,C", [(4, 28, 28, 128), (4, 14, 14, 256), (2, 16, 16, 256), (2, 3, 5, 128)])
def test_stride1(Fr, H, W, C, opt):
    """(4 x 14 x 14, 2 x 16 x 16, 2 x 3 x 5: pixel counts the general kernel has no tile for -- the default takes them too)"""
    run(opt, Fr, H, W, C)


def test_stride1_general_kernel():
    run(0, 4, 28, 28, 128)


@pytest.mark.parametrize("opt", [1, 2])
@pytest.mark.parametrize("Fr,H,W,C,pt,pl", [(2, 56, 56, 128, 0, 0), (2, 28, 28, 256, 0, 0), (1, 8, 8, 128, 1, 1)])
def test_stride2(Fr, H, W, C, pt, pl, opt):
    run(opt, Fr, H, W, C, 2, pt, pl)


@pytest.mark.parametrize("opt", [0, 2])
def test_stride2_general_kernel(opt):
    """the general stride-2 kernel needs a multiple of 64 output pixels, which none of the shapes above has: 16 frames of 14 x 14, with option 0 and, same operands,
    the new kernel"""
    run(opt, 16, 28, 28, 128, 2, 0, 0)
