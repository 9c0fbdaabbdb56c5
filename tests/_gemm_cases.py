"""TEST INFRASTRUCTURE: the case table, the fp64 reference and the derived elementwise error bound of maed_gemm_nt's kernels x fused epilogues, shared by the
GPU tests (tests/test_gpu_gemm_epilogues.py) and the simulator tests (tests/test_hostsim_gemm_matrix.py).  No GPU code: the callers say on which device the
operands live and through which library handle the call goes (maed_amd._lib.lib(), which tests/_hostsim.patched() swaps).

Shapes come from the tile sizes of the sources (csrc/gemm.hip: 128 x 128 x 64, 64 x 64 x 16 for the VALU kernel; csrc/gemm256.hip and csrc/gemm_sk.hip:
256 x 256 x 64), not from the workload.

The bound (elementwise, nothing tuned):
  acc   = 2 K 2^-24 (|A| @ |B|^T) in fp64 -- the forward bound of a length-K fp32 sum in any order, doubled for the fused multiply-adds of the matrix cores and a
          split-K meeting point
  bf16 outputs: + 2^-8 |ref| (half a bf16 spacing of rounding; the accumulation error that may flip the rounding direction is the acc term)
  fp32 outputs: + 2^-23 |ref|
  GELU / TANH / MUL_DGELU: acc times the epilogue's Lipschitz factor (max |gelu'| < 1.13, |tanh'| <= 1, |gelu'(aux)|) + 2^-20 for the device's tanhf / erff
  GELU activation: against gelu of the STORED pre-activation; without a stored pre-activation (out2 = NULL) against gelu of the bf16-rounded reference
          pre-activation, plus 1.13 x (one bf16 spacing 2^-7 |pre| + 2 acc) wherever pre +- acc round to different bf16 values (the kernel's pre-activation may
          then be the neighbour)
"""
import functools
import math

import pytest
import torch

from maed_amd import _lib as L
from maed_amd import ops

F32, BF16 = torch.float32, torch.bfloat16
U24, U23, U20, U8, U7 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -20, 2.0 ** -8, 2.0 ** -7
GELU_LIP = 1.13                     # max |gelu'(x)| = 1.1289 (at x = sqrt(2))


class _sk_mode:
    """MAED_OPT_SK for the duration of a block (2 = whole tiles only, 3 = stream-K cuts whenever the tiles do not fill whole rounds of the grid)"""

    def __init__(self, mode, grid=0):
        self.mode, self.grid = mode, grid

    def __enter__(self):
        self.lib = L.lib()
        self.old = (self.lib.maed_get_option(L.OPT_SK), self.lib.maed_get_option(L.OPT_SK_GRID))
        assert self.lib.maed_set_option(L.OPT_SK, self.mode) == 0 and self.lib.maed_set_option(L.OPT_SK_GRID, self.grid) == 0

    def __exit__(self, *a):
        self.lib.maed_set_option(L.OPT_SK, self.old[0])
        self.lib.maed_set_option(L.OPT_SK_GRID, self.old[1])


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------------------
SHAPES_128 = [
    (130, 136, 64),      # ragged M and N tiles, N % 8 == 0, one K tile
    (300, 100, 192),     # N % 8 != 0: bf16 rows are not 16-byte aligned, the scalar tail (vec_ok false); three K tiles
    (64, 72, 128),       # M smaller than one tile
    (1, 8, 64),          # a single row, a single 8-column group
]
SHAPES_256 = [           # gemm.hip ok256: K >= 128, K % 64 == 0
    (260, 264, 128),
    (300, 100, 192),
    (70, 520, 320),      # five K tiles: an odd count, both drains
]
SHAPES_SK = [            # gemm_sk.hip maed_gemm_nt_sk_shape_ok: M, N >= 256, N % 8 == 0, K % 128 == 0
    (300, 264, 128),
    (513, 520, 384),
]

# ---- epilogue variants ------------------------------------------------------------------------------------------------------------------------------------
VARIANTS = ["STORE", "STORE.nobias", "STORE_F32", "GELU", "GELU.noout2", "RESID_F32", "MUL_DGELU", "TANH", "ADD", "ADD.mask", "ATOMIC_F32.k1", "ATOMIC_F32.k2"]
EPI_OF = {"STORE": L.EPI_STORE, "STORE.nobias": L.EPI_STORE, "STORE_F32": L.EPI_STORE_F32, "GELU": L.EPI_GELU, "GELU.noout2": L.EPI_GELU,
          "RESID_F32": L.EPI_RESID_F32, "MUL_DGELU": L.EPI_MUL_DGELU, "TANH": L.EPI_TANH, "ADD": L.EPI_ADD, "ADD.mask": L.EPI_ADD,
          "ATOMIC_F32.k1": L.EPI_ATOMIC_F32, "ATOMIC_F32.k2": L.EPI_ATOMIC_F32}

# What each launcher carries (csrc/gemm_epilogue.cuh EPI_SET_STORES / EPI_SET_ALL, csrc/gemm.hip dispatch<EPI>):
#   maed_gemm_nt itself switches over EPI_SET_ALL; launch_valu / launch_mfma / launch_glds<.., 1 | 2> are instantiated for every EPI of it;
#   ok256 (and with it oksk) holds `EPI != MAED_EPI_ATOMIC_F32 && splitk == 1`, and maed_gemm_nt_256_launch / maed_gemm_nt_sk_launch switch over EPI_SET_STORES.
EPI_SET_STORES = frozenset([L.EPI_STORE, L.EPI_GELU, L.EPI_RESID_F32, L.EPI_MUL_DGELU, L.EPI_STORE_F32, L.EPI_TANH, L.EPI_ADD])
EPI_SET_ALL = EPI_SET_STORES | {L.EPI_ATOMIC_F32}
IMPL_MFMA_GLDS1, IMPL_MFMA_GLDS2 = 3, 4     # include/maed_hip.h MAED_IMPL_MFMA_GLDS1 / _GLDS2 (the Python binding has no names for them)

# name -> dtype, impl, (MAED_OPT_SK, MAED_OPT_SK_GRID) or None, shapes, carried epilogues
KERNELS = {
    "f32-valu":    dict(dtype=F32, impl=L.IMPL_VALU, sk=None, shapes=SHAPES_128, carries=EPI_SET_ALL),
    "bf16-valu":   dict(dtype=BF16, impl=L.IMPL_VALU, sk=None, shapes=SHAPES_128, carries=EPI_SET_ALL),
    "bf16-mfma":   dict(dtype=BF16, impl=L.IMPL_MFMA, sk=None, shapes=SHAPES_128, carries=EPI_SET_ALL),
    "bf16-glds1":  dict(dtype=BF16, impl=IMPL_MFMA_GLDS1, sk=None, shapes=SHAPES_128, carries=EPI_SET_ALL),
    "bf16-glds2":  dict(dtype=BF16, impl=IMPL_MFMA_GLDS2, sk=None, shapes=SHAPES_128, carries=EPI_SET_ALL),
    "bf16-auto":   dict(dtype=BF16, impl=L.IMPL_AUTO, sk=None, shapes=SHAPES_128, carries=EPI_SET_ALL),
    "bf16-256":    dict(dtype=BF16, impl=L.IMPL_MFMA_256, sk=None, shapes=SHAPES_256, carries=EPI_SET_STORES),
    "bf16-sk-m2":  dict(dtype=BF16, impl=L.IMPL_MFMA_SK, sk=(2, 0), shapes=SHAPES_SK, carries=EPI_SET_STORES),
    "bf16-sk-m3":  dict(dtype=BF16, impl=L.IMPL_MFMA_SK, sk=(3, 0), shapes=SHAPES_SK, carries=EPI_SET_STORES),
    "bf16-sk-m3g7": dict(dtype=BF16, impl=L.IMPL_MFMA_SK, sk=(3, 7), shapes=SHAPES_SK, carries=EPI_SET_STORES),
}
DMA_KERNELS = ["bf16-glds1", "bf16-glds2", "bf16-256"]      # LDS-DMA kernels whose epilogue has a scalar path (the K-stream kernel carries the 8-wide one only)
STRIDED_VARIANTS = ["STORE", "GELU", "RESID_F32", "MUL_DGELU", "ADD.mask", "ATOMIC_F32.k1", "ATOMIC_F32.k2"]
STRIDED_SHAPE = {k: v["shapes"][0] for k, v in KERNELS.items()}      # the first shape of every list is ragged in M and N
# N % 8 != 0 inside leading dimensions that ARE multiples of 8 (ldo = 128, ldaux = 120): vec_ok holds, and the column group at c0 = 96 must leave the vector
# form of epilogue_store8 for the scalar tail (c0 + 8 > N) -- with a plain output of this shape vec_ok is false and no group is ever stored as a vector.
# The register-staged kernel stores groups of 4 (epilogue_store4), and 100 is a multiple of 4: its tail (c0 + 4 > N) needs N % 4 != 0, a shape of its own.
TAIL_SHAPE = (300, 100, 192)
TAIL_SHAPE_4WIDE = {"bf16-mfma": (130, 98, 64)}
TAIL_VARIANTS = ["STORE", "GELU", "RESID_F32", "MUL_DGELU", "ADD.mask"]


def carried(kernel, variant):
    return EPI_OF[variant] in KERNELS[kernel]["carries"]


def _id(kernel, variant, shape):
    return f"{kernel}-{variant}-{shape[0]}x{shape[1]}x{shape[2]}"


def matrix_cases(simulator=False):
    """simulator: the smallest shape of every kernel's list and its first one (ragged in M and N with N % 8 == 0: the vector forms of the epilogues)"""
    out = []
    for kernel, spec in KERNELS.items():
        shapes = spec["shapes"]
        if simulator:
            shapes = [s for s in shapes if s in (shapes[0], min(shapes, key=lambda s: s[0] * s[1] * s[2]))]
        for shape in shapes:
            for variant in VARIANTS:
                out.append(pytest.param(kernel, variant, shape, id=_id(kernel, variant, shape)))
    return out


def strided_cases():
    """(kernel, variant, shape, shift of the output view in elements)"""
    out = [pytest.param(kernel, variant, STRIDED_SHAPE[kernel], 8, id=f"{kernel}-{variant}") for kernel in KERNELS for variant in STRIDED_VARIANTS]
    out += [pytest.param(kernel, variant, TAIL_SHAPE, 8, id=f"{kernel}-{variant}-tail") for kernel, spec in KERNELS.items() if TAIL_SHAPE in spec["shapes"]
            for variant in TAIL_VARIANTS]
    out += [pytest.param(kernel, variant, shape, 8, id=f"{kernel}-{variant}-tail4") for kernel, shape in TAIL_SHAPE_4WIDE.items() for variant in TAIL_VARIANTS]
    # the output view shifted by 4 elements: row bases aligned to 8 bytes only, so epilogue_vec_ok (which looks at the pointers as well as the leading
    # dimensions) sends every group down the scalar path; the K-stream kernel has none and must refuse the call
    out += [pytest.param(kernel, "STORE", STRIDED_SHAPE[kernel], 4, id=f"{kernel}-STORE-shift4") for kernel in DMA_KERNELS + ["bf16-sk-m2"]]
    return out


# ---- operands and reference ---------------------------------------------------------------------------------------------------------------------------------
def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def dgelu(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def to_bf16_f64(x):
    """fp64 -> nearest bf16, as fp64"""
    return x.float().bfloat16().double()


def pack_bits(keep):
    """(M, W) bool, W % 8 == 0 -> (M, W / 8) uint8, bit c & 7 of byte c >> 3"""
    M, W = keep.shape
    w = (1 << torch.arange(8, dtype=torch.int32))
    return (keep.view(M, W // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8).contiguous()


@functools.lru_cache(maxsize=8)
def operands(dtype, M, N, K):
    """the operands of one (dtype, shape), rounded to dtype, and everything of the reference that does not depend on the epilogue -- computed once, read only"""
    A, B = rnd(M, K, seed=1).to(dtype), rnd(N, K, seed=2, scale=K ** -0.5).to(dtype)
    Np = (N + 7) // 8 * 8
    d = dict(A=A, B=B, bias=rnd(N, seed=3), res=rnd(M, N, seed=4), aux=rnd(M, N, seed=5).to(dtype), acc0=rnd(M, N, seed=6),
             keep=torch.rand(M, Np, generator=torch.Generator().manual_seed(7)) > 0.4)
    d["acc"] = A.double() @ B.double().t()
    d["absacc"] = A.double().abs() @ B.double().abs().t()
    d["acc_bound"] = 2 * K * U24 * d["absacc"]
    return d


def reference(variant, d, out_dtype):
    """[(what, ref fp64, bound fp64)] of the plain definition; `what` = "out" or "out2".  The GELU activation is not in here (activation_reference)."""
    acc, ab, bias = d["acc"], d["acc_bound"], d["bias"].double()
    rnd_term = U8 if out_dtype == BF16 else U23
    N = acc.shape[1]
    if variant == "STORE":
        ref = acc + bias
        return [("out", ref, ab + rnd_term * ref.abs())]
    if variant == "STORE.nobias":
        return [("out", acc, ab + rnd_term * acc.abs())]
    if variant == "STORE_F32":
        ref = acc + bias
        return [("out", ref, ab + U23 * ref.abs())]
    if variant == "GELU":
        ref = acc + bias
        return [("out2", ref, ab + rnd_term * ref.abs())]
    if variant == "GELU.noout2":
        return []
    if variant == "RESID_F32":
        ref = d["res"].double() + acc + bias
        return [("out", ref, ab + U23 * ref.abs())]
    if variant == "MUL_DGELU":
        g = dgelu(d["aux"].double())
        ref = acc * g
        return [("out", ref, g.abs() * ab + U20 + rnd_term * ref.abs())]
    if variant == "TANH":
        ref = torch.tanh(acc + bias)
        return [("out", ref, ab + U20 + rnd_term * ref.abs())]
    if variant == "ADD":
        ref = d["aux"].double() + acc + bias
        return [("out", ref, ab + rnd_term * ref.abs())]
    if variant == "ADD.mask":
        ref = d["aux"].double() * d["keep"][:, :N] + acc + bias
        return [("out", ref, ab + rnd_term * ref.abs())]
    if variant.startswith("ATOMIC_F32"):
        ref = d["acc0"].double() + acc
        return [("out", ref, ab + U23 * ref.abs())]
    raise KeyError(variant)


def activation_reference(variant, d, out_dtype, stored_pre):
    """(ref, bound) of the GELU activation: of the stored pre-activation (fp64 tensor on the CPU), or -- GELU.noout2 -- of the rounded reference pre-activation"""
    rnd_term = U8 if out_dtype == BF16 else U23
    if variant == "GELU":
        ref = gelu(stored_pre)
        return ref, U20 + rnd_term * ref.abs()
    z, ab = d["acc"] + d["bias"].double(), d["acc_bound"]
    if out_dtype == BF16:
        pre = to_bf16_f64(z)
        flip = to_bf16_f64(z - ab) != to_bf16_f64(z + ab)           # the kernel's pre-activation may be the neighbouring bf16 value: one spacing away
        dpre = flip * (U7 * pre.abs() + 2 * ab)
    else:
        pre, dpre = z, ab + U23 * z.abs()
    ref = gelu(pre)
    return ref, GELU_LIP * dpre + U20 + rnd_term * ref.abs()


def check(name, got, ref, bound, log=None):
    """assert |got - ref| <= bound elementwise; returns (and logs) the worst ratio of error to bound"""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    ratio = (got - ref).abs() / bound
    worst = int(ratio.argmax())
    r, c = divmod(worst, ref.shape[1])
    line = (f"{name:62s} worst err/bound={ratio.max().item():.3f} at ({r},{c}): got={got[r, c].item():.9g} ref={ref[r, c].item():.9g} "
            f"bound={bound[r, c].item():.3e}")
    if log is not None:
        log(line)
    bad = ratio > 1.0
    assert not bad.any(), f"{int(bad.sum())}/{bad.numel()} elements over the derived bound; {line}"
    return ratio.max().item()


# ---- the call -------------------------------------------------------------------------------------------------------------------------------------------
def out_dtype_of(variant, dtype):
    return F32 if EPI_OF[variant] in (L.EPI_RESID_F32, L.EPI_ATOMIC_F32, L.EPI_STORE_F32) else dtype


def gemm_call(A, B, epilogue, bias, out, out2, aux, splitk, impl):
    """maed_gemm_nt as maed_amd.ops.gemm_nt calls it, but with every output given by the caller and out2 passed as it is (ops.gemm_nt always allocates the GELU
    pre-activation; out2 = NULL is the inference path)"""
    M, K = A.shape
    assert A.stride(1) == 1 and B.stride(1) == 1 and out.stride(1) == 1
    ops.check(L.lib().maed_gemm_nt(ops._p(A), A.stride(0), ops._p(B), B.stride(0), M, B.shape[0], K, ops.mm_code(A.dtype), epilogue, ops._p(bias),
                                   ops._p(out), out.stride(0), ops._p(out2), ops._p(aux), aux.stride(0) if aux is not None else 0, splitk, impl,
                                   ops._stream()), "gemm_nt")


class _nothing:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def kernel_mode(kernel):
    sk = KERNELS[kernel]["sk"]
    return _sk_mode(*sk) if sk else _nothing()


FILL16, FILL32 = 0x4b4b, 0x4b4b4b4b      # bf16 1.33e7 / fp32 1.33e7: finite, far outside every bound if it is left or copied where a result belongs


def _filled(rows, cols, dtype, dev):
    if dtype == BF16:
        return torch.full((rows, cols), FILL16, dtype=torch.int16, device=dev).view(BF16)
    return torch.full((rows, cols), FILL32, dtype=torch.int32, device=dev).view(F32)


def _ints(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


class Layout:
    """where the operands of one case live.  Plain: contiguous tensors of exactly the operand's size.  Strided: A / B are column windows (offset 8) of matrices with
    lda = K + 40 / ldb = K + 24; out (and the GELU pre-activation) are views O[2:2+M, shift:shift+N] of pattern-filled buffers with two guard rows above and
    below and ldo = N + 24 rounded up to 8; aux is a window of a matrix with ldaux = N + 16 rounded up to 8; the ADD mask has a row pitch of ldaux / 8 bytes
    counted from the byte of aux's first element (csrc/gemm_epilogue.cuh epilogue_store: bit c & 7 of byte (r * ldaux + c) >> 3).
    The mask's addressing needs ldaux % 8 == 0, so a plain aux with N % 8 != 0 is widened to the next multiple of 8 for ADD.mask."""

    def __init__(self, d, variant, dtype, dev, strided=False, shift=8):
        M, K = d["A"].shape
        N = d["B"].shape[0]
        self.M, self.N, self.strided, self.shift = M, N, strided, shift
        odt = out_dtype_of(variant, dtype)
        epi = EPI_OF[variant]
        up8 = lambda n: (n + 7) // 8 * 8
        gen = torch.Generator().manual_seed(11)

        def window(x, ld, off):
            w = torch.randn(x.shape[0], ld, generator=gen).to(x.dtype)
            w[:, off:off + x.shape[1]] = x
            return w.to(dev)[:, off:off + x.shape[1]]

        self.A = window(d["A"], K + 40, 8) if strided else d["A"].to(dev)
        self.B = window(d["B"], K + 24, 8) if strided else d["B"].to(dev)
        self.bias = None if variant in ("STORE.nobias", "MUL_DGELU") or epi == L.EPI_ATOMIC_F32 else d["bias"].to(dev)
        self.bufs = []                                  # (buffer, the view the kernel writes)
        self.out = self._output(odt, dev)
        if epi == L.EPI_ATOMIC_F32:
            self.out.copy_(d["acc0"].to(dev))
        self.out2 = self._output(odt, dev) if variant == "GELU" else None
        self.aux = None
        if epi in (L.EPI_RESID_F32, L.EPI_MUL_DGELU, L.EPI_ADD):
            x = d["res"] if epi == L.EPI_RESID_F32 else d["aux"]
            ldaux = up8(N + 16) if strided else (up8(N) if variant == "ADD.mask" else N)
            self.aux = window(x, ldaux, 0) if ldaux != N else x.to(dev)
            if variant == "ADD.mask":
                keep = torch.rand(M, ldaux, generator=gen) > 0.5            # bits of the pad columns: arbitrary
                keep[:, :d["keep"].shape[1]] = d["keep"]
                self.out2 = pack_bits(keep).to(dev)

    def _output(self, odt, dev):
        M, N = self.M, self.N
        if not self.strided:
            buf = _filled(M, N, odt, dev)
            self.bufs.append((buf, buf))
            return buf
        ldo = (N + 24 + 7) // 8 * 8
        buf = _filled(M + 4, ldo, odt, dev)
        view = buf[2:2 + M, self.shift:self.shift + N]
        self.bufs.append((buf, view))
        return view

    def guards_untouched(self):
        """every element of the output buffers outside the views still holds the fill pattern, bit for bit"""
        for buf, view in self.bufs:
            if buf is view:
                continue
            ints = _ints(buf).clone()
            fill = FILL16 if buf.dtype == BF16 else FILL32
            ints[2:2 + self.M, self.shift:self.shift + self.N] = fill
            bad = (ints != fill).nonzero()
            assert bad.numel() == 0, f"{bad.shape[0]} guard elements changed, the first at buffer (row, column) {tuple(bad[0].tolist())}; the view starts at (2, {self.shift})"


def run_case(kernel, variant, shape, dev, log=None, strided=False, shift=8):
    """one (kernel, epilogue variant, shape): the launch(es), the comparison with the fp64 reference under the derived bound, the guard bands of a strided layout.
    A pair the launcher does not carry must be refused with MaedHipError.  Returns the worst ratio of error to bound (None for a refused pair)."""
    spec = KERNELS[kernel]
    dtype, impl = spec["dtype"], spec["impl"]
    d = operands(dtype, *shape)
    lay = Layout(d, variant, dtype, dev, strided=strided, shift=shift)
    epi = EPI_OF[variant]
    splitk = 2 if variant == "ATOMIC_F32.k2" else 1
    tag = f"gemm_matrix[{kernel},{variant},{shape[0]}x{shape[1]}x{shape[2]}{',strided' if strided else ''}{',shift4' if shift != 8 else ''}]"
    with kernel_mode(kernel):
        if not carried(kernel, variant):
            with pytest.raises(L.MaedHipError):
                ops.gemm_nt(lay.A, lay.B, epi, bias=lay.bias, out=lay.out, out2=lay.out2, aux=lay.aux, splitk=splitk, impl=impl)
            return None
        if spec["sk"] and shift % 8:
            # gemm_sk.hip sk_epi_ok: the K-stream kernel instantiates the 8-wide epilogues only and refuses an output that is not 16-byte aligned
            with pytest.raises(L.MaedHipError):
                gemm_call(lay.A, lay.B, epi, lay.bias, lay.out, lay.out2, lay.aux, splitk, impl)
            lay.guards_untouched()
            return None
        gemm_call(lay.A, lay.B, epi, lay.bias, lay.out, lay.out2, lay.aux, splitk, impl)
    odt = out_dtype_of(variant, dtype)
    worst = 0.0
    for what, ref, bound in reference(variant, d, odt):
        got = lay.out if what == "out" else lay.out2
        worst = max(worst, check(tag + ("" if what == "out" else ".pre"), got, ref, bound, log))
    if epi == L.EPI_GELU:
        stored = lay.out2.detach().double().cpu() if variant == "GELU" else None
        ref, bound = activation_reference(variant, d, odt, stored)
        worst = max(worst, check(tag + ".act", lay.out, ref, bound, log))
    lay.guards_untouched()
    return worst
