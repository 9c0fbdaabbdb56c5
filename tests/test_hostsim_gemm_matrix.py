"""The kernel x epilogue table of tests/_gemm_cases.py on the host simulator (the x86 build of the same sources, tests/hostsim): the smallest and the first (ragged) shape of
every kernel with every epilogue variant against the fp64 reference under the derived bound, the pairs a launcher does not carry (they must be refused), and the
strided-operand / guard-band cases.  What the simulator cannot show -- the placement of the two workgroup barriers of epilogue_shuffled, LDS-DMA copies that land
late -- is what tests/test_gpu_gemm_epilogues.py runs the same table on the device for."""
import pytest

import _gemm_cases as G
from _hostsim import patched


@pytest.mark.parametrize("kernel,variant,shape", G.matrix_cases(simulator=True))
def test_gemm_matrix(kernel, variant, shape):
    with patched():
        G.run_case(kernel, variant, shape, "cpu")


@pytest.mark.parametrize("kernel,variant,shape,shift", G.strided_cases())
def test_gemm_strided_operands_and_guard_bands(kernel, variant, shape, shift):
    with patched():
        G.run_case(kernel, variant, shape, "cpu", strided=True, shift=shift)

