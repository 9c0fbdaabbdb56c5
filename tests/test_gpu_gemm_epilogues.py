"""GPU parity matrix of maed_gemm_nt: every NT GEMM kernel x every fused epilogue it carries x the shapes of that kernel's tile (tests/_gemm_cases.py), against an
fp64 reference of the plain definition under an elementwise bound derived from the arithmetic (one bf16 spacing, not 2e-2); operands and outputs that are
windows of wider buffers with pattern-filled guard bands that must come back bit for bit; the bitwise promises of gemm256.hip / gemm_sk.hip for the epilogues
the older tests skip.  The host simulator runs the same table (tests/test_hostsim_gemm_matrix.py), but it lands LDS-DMA copies at issue time and runs the waves
of a workgroup in order: the two barriers of epilogue_shuffled, which overlay the staging area on the operand tiles, are exercised here only."""
import pytest
import torch

import _gemm_cases as G
from _util import DEV, note

pytestmark = pytest.mark.gpu


def _faults():
    from maed_amd import _lib as L
    return L.lib().maed_device_faults()


@pytest.mark.parametrize("kernel,variant,shape", G.matrix_cases())
def test_gemm_matrix(kernel, variant, shape):
    G.run_case(kernel, variant, shape, DEV, log=note)
    assert _faults() == 0


@pytest.mark.parametrize("kernel,variant,shape,shift", G.strided_cases())
def test_gemm_strided_operands_and_guard_bands(kernel, variant, shape, shift):
    G.run_case(kernel, variant, shape, DEV, log=note, strided=True, shift=shift)
    assert _faults() == 0


@pytest.mark.parametrize("kernel,shape,variants", [
    ("bf16-256", (260, 264, 128), ["TANH", "ADD", "ADD.mask"]),
    ("bf16-sk-m2", (300, 264, 128), ["STORE_F32", "TANH", "ADD", "ADD.mask"]),
], ids=["256", "sk-mode2"])
def test_gemm_kernels_agree_bitwise_where_they_promise_to(kernel, shape, variants):
    """gemm256.hip and gemm_sk.hip (whole tiles: MAED_OPT_SK = 2) promise the k order of the 128 x 128 LDS-DMA kernel (impl = 3): the same bits, for the epilogues
    the torch.equal checks of tests/test_gpu_kernels.py do not reach"""
    spec = G.KERNELS[kernel]
    d = G.operands(spec["dtype"], *shape)
    for variant in variants:
        outs = []
        for impl in (spec["impl"], G.IMPL_MFMA_GLDS1):
            lay = G.Layout(d, variant, spec["dtype"], DEV)
            with G.kernel_mode(kernel):
                G.gemm_call(lay.A, lay.B, G.EPI_OF[variant], lay.bias, lay.out, lay.out2, lay.aux, 1, impl)
            outs.append(lay.out)
            assert not (G._ints(lay.out) == (G.FILL16 if lay.out.dtype == G.BF16 else G.FILL32)).any(), f"{variant}: impl {impl} left part of its output unwritten"
        assert torch.equal(outs[0], outs[1]), f"{kernel} and the 128 x 128 LDS-DMA kernel differ for {variant} at {shape}"
        note(f"gemm_bitwise[{kernel} == bf16-glds1,{variant},{shape[0]}x{shape[1]}x{shape[2]}] identical")
    assert _faults() == 0
