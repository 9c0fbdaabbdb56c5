"""csrc/batchnorm.hip on the host simulator (tests/_hostsim_batchnorm.py) against fp64 torch: BatchNorm statistics / apply / backward, the 3x3/2 max-pool with
padding 1 and the global average pool.  Every output and scratch buffer sits between sentinel-filled guard zones that must come back unchanged."""
import pytest
import torch
import torch.nn.functional as F

import _batchnorm_cases as K
import _hostsim_batchnorm as S

DTYPES = [torch.float32, torch.bfloat16]
# the large shapes run the two extreme variants only (a simulated workgroup is 256 host threads)
SMALL = [s for s in K.BN_SHAPES if s[0] * s[2] * s[3] < 1000]
LARGE = [s for s in K.BN_SHAPES if s[0] * s[2] * s[3] >= 1000]


@pytest.fixture(scope="module")
def lib():
    return S.load()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [False, True], ids=["norelu", "relu"])
@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_batchnorm_train_small(lib, shape, relu, res, dtype):
    got = S.bn_train(K.case(shape, dtype, res), relu, K.EPS, K.MOMENTUM, lib=lib)
    K.check_bn(f"sim bn {shape}", got, K.reference(shape, dtype, res, relu), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("res,relu", [(False, False), (True, True), (False, True)], ids=["plain", "res_relu", "relu"])
@pytest.mark.parametrize("shape", LARGE, ids=str)
def test_batchnorm_train_many_chunks(lib, shape, res, relu, dtype):
    assert lib.maed_batchnorm_chunks(shape[0] * shape[2] * shape[3]) > 1
    got = S.bn_train(K.case(shape, dtype, res), relu, K.EPS, K.MOMENTUM, lib=lib)
    K.check_bn(f"sim bn {shape}", got, K.reference(shape, dtype, res, relu), dtype)


def test_partial_last_chunk_is_covered(lib):
    """(3, 64, 21, 21): 1323 rows = 41 chunks of 32 rows + one of 11"""
    M = 3 * 21 * 21
    assert lib.maed_batchnorm_chunks(M) == 42 and M % 32 == 11


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 64, 7, 9), (3, 256, 5, 5)], ids=str)
def test_batchnorm_eval_frozen_statistics(lib, shape, dtype):
    for res, relu in ((False, True), (True, True), (False, False)):
        got = S.bn_train(K.case(shape, dtype, res), relu, K.EPS, K.MOMENTUM, frozen=True, lib=lib)
        K.check_bn(f"sim bn eval {shape} res={res} relu={relu}", got, K.reference(shape, dtype, res, relu, training=False), dtype, training=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_two_runs_are_bit_equal(lib, dtype):
    c = K.case((3, 64, 21, 21), dtype, True)
    a, b = S.bn_train(c, True, lib=lib), S.bn_train(c, True, lib=lib)
    for k in a:
        assert a[k] is None or torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 64, 7, 9), (3, 64, 21, 21)], ids=str)
def test_large_mean_meets_the_same_tolerance(lib, shape, dtype):
    """per-channel mean = 8 x standard deviation (post-ReLU activations stay below 2 x): E[x^2] - mean^2 loses 6 bits; the fp64 combine must absorb that"""
    got = S.bn_train(K.case(shape, dtype, True, mean_over_std=8.0), True, lib=lib)
    K.check_bn(f"sim bn large mean {shape}", got, K.reference(shape, dtype, True, True, mean_over_std=8.0), dtype)


def test_finalize_takes_sums_and_count(lib):
    """the finalize step alone on (sum, sum of squares, count): what a cross-rank reduction of the partials would call"""
    C_, chunks, count = 24, 3, 50.0
    g = torch.Generator().manual_seed(3)
    x = torch.randn(50, C_, generator=g, dtype=torch.float64) * 2 + 1
    parts = torch.zeros(chunks, C_, 2, dtype=torch.float64)
    for k, sl in enumerate((slice(0, 20), slice(20, 37), slice(37, 50))):
        parts[k, :, 0], parts[k, :, 1] = x[sl].sum(0), (x[sl] ** 2).sum(0)
    mean, rstd = S.Guarded((C_,), torch.float32), S.Guarded((C_,), torch.float32)
    rm, rv = S.Guarded((C_,), torch.float32, torch.zeros(C_)), S.Guarded((C_,), torch.float32, torch.ones(C_))
    S._ok(lib, lib.maed_batchnorm_finalize(parts.data_ptr(), chunks, C_, count, 1e-5, mean.t.data_ptr(), None, rstd.t.data_ptr(), rm.t.data_ptr(), rv.t.data_ptr(), 0.1, None), "finalize")
    K.close("finalize mean", mean.t, x.mean(0), rtol=1e-6, atol=1e-7)
    K.close("finalize rstd", rstd.t, 1 / torch.sqrt(x.var(0, unbiased=False) + 1e-5), rtol=1e-6, atol=0)
    K.close("finalize running_var", rv.t, 0.9 + 0.1 * x.var(0, unbiased=True), rtol=1e-6, atol=0)
    K.close("finalize running_mean", rm.t, 0.1 * x.mean(0), rtol=1e-6, atol=1e-8)
    S.check_all("finalize")


def test_bad_arguments_are_errors(lib):
    x = torch.zeros(4, 12)
    f = torch.zeros(16)
    part = torch.zeros(64, dtype=torch.float64)
    assert lib.maed_batchnorm_stats(x.data_ptr(), 4, 12, 0, part.data_ptr(), 1e-5, f.data_ptr(), None, f.data_ptr(), None, None, 0.1, None) == -2      # C % 8
    assert lib.maed_batchnorm_stats(None, 4, 16, 0, part.data_ptr(), 1e-5, f.data_ptr(), None, f.data_ptr(), None, None, 0.1, None) == -1
    assert b"C=12" in lib.maed_last_error() or lib.maed_last_error()


def _pool_input(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, shape, generator=g).float()          # integer values: many ties
    x[0, 3, shape[2] // 2, shape[3] // 2] = float("nan")
    return x.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 64, 9, 12), (1, 64, 7, 7), (2, 64, 16, 16)], ids=str)
def test_maxpool_matches_aten_exactly(lib, shape, dtype):
    x = _pool_input(shape, dtype, 5)
    ref = F.max_pool2d(x.float(), 3, 2, 1)
    g = torch.Generator().manual_seed(6)
    dy = torch.randn(ref.shape, generator=g).to(dtype)
    y, dx = S.maxpool(x.permute(0, 2, 3, 1).contiguous(), dy.permute(0, 2, 3, 1).contiguous(), lib=lib)
    y = y.permute(0, 3, 1, 2).float()
    assert torch.equal(torch.isnan(y), torch.isnan(ref)) and torch.equal(torch.nan_to_num(y, nan=123.0), torch.nan_to_num(ref, nan=123.0))
    x64 = x.double().requires_grad_(True)
    F.max_pool2d(x64, 3, 2, 1).backward(dy.double())
    K.close(f"sim maxpool dx {shape}", dx.permute(0, 3, 1, 2), x64.grad, **K.tol(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("HW,C_", [(1, 64), (4, 2048), (49, 64), (49, 2048)])
def test_avgpool(lib, HW, C_, dtype):
    g = torch.Generator().manual_seed(HW + C_)
    x = torch.randn(3, HW, C_, generator=g).to(dtype)
    dy = torch.randn(3, C_, generator=g)
    y, dx = S.avgpool(x, dy, lib=lib)
    K.close(f"sim avgpool y {HW}x{C_}", y, x.double().mean(1), **K.tol(dtype))
    K.close(f"sim avgpool dx {HW}x{C_}", dx, (dy.double() / HW).unsqueeze(1).expand(3, HW, C_), **K.tol(dtype))


def test_module_on_the_simulator_matches_torch_batchnorm():
    """maed_amd.resnet.BatchNorm2d / pools through ops.BatchNormFn on the simulator library: autograd wiring, buffers, num_batches_tracked"""
    from maed_amd import resnet
    torch.manual_seed(0)
    with S.patched():
        bn = resnet.BatchNorm2d(16)
        ref = torch.nn.BatchNorm2d(16).double()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5); bn.bias.normal_()
            ref.weight.copy_(bn.weight); ref.bias.copy_(bn.bias)
        x = torch.randn(2, 16, 5, 6).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        r = torch.randn(2, 16, 5, 6).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        x64, r64 = x.detach().double().requires_grad_(True), r.detach().double().requires_grad_(True)
        y = bn(x, residual=r, relu=True)
        y64 = F.relu(ref(x64) + r64)
        w = torch.randn(y.shape)
        (y * w).sum().backward()
        (y64 * w.double()).sum().backward()
        K.close("module y", y, y64, **K.tol(torch.float32, 4))
        K.close("module dx", x.grad, x64.grad, **K.tol(torch.float32, 2))
        K.close("module dres", r.grad, r64.grad, **K.tol(torch.float32, 2))
        K.close("module dgamma", bn.weight.grad, ref.weight.grad, **K.affine_tol(torch.float32, ref.weight.grad))
        K.close("module dbeta", bn.bias.grad, ref.bias.grad, **K.affine_tol(torch.float32, ref.bias.grad))
        K.close("module running_var", bn.running_var, ref.running_var, rtol=1e-5, atol=2e-7)
        assert int(bn.num_batches_tracked) == 1
        bn.eval(); ref.eval()
        K.close("module eval", bn(x.detach(), relu=True), F.relu(ref(x64.detach())), **K.tol(torch.float32, 4))
        p = resnet.MaxPool3s2P1()(x.detach()[:, :, :, :5].contiguous(memory_format=torch.channels_last))
        assert torch.equal(p, F.max_pool2d(x.detach()[:, :, :, :5], 3, 2, 1))
        a = resnet.GlobalAvgPool()(x.detach())
        K.close("module avgpool", a, x.detach().double().mean((2, 3)), **K.tol(torch.float32))
        with pytest.raises(ValueError):
            bn.train()
            bn(torch.randn(1, 16, 1, 1))
