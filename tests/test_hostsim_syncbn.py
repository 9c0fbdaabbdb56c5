"""BatchNorm statistics over the batch of all ranks (resnet.convert_sync_batchnorm; docs/design/16_sync_batchnorm.md) without a GPU: the entry points of
csrc/batchnorm.hip on the host simulator with the rows of a case cut into unequal shards (tests/_hostsim_syncbn.py), and resnet.BatchNorm2d under two gloo
ranks -- on the simulator library and on the framework composition -- against the single-process run of the whole batch."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _batchnorm_cases as K  # noqa: E402
import _hostsim_batchnorm as S  # noqa: E402
import _hostsim_syncbn as Y  # noqa: E402

DTYPES = [torch.float32, torch.bfloat16]
# rows -> unequal shards; (1, 2048, 1, 2): each shard alone holds one value per channel
SHARDS = {(2, 64, 7, 9): (37, 89), (3, 256, 5, 5): (5, 32, 38), (1, 2048, 1, 2): (1, 1), (4, 64, 40, 40): (1323, 5077), (3, 64, 21, 21): (31, 1292), (2, 72, 3, 3): (7, 11)}
assert set(SHARDS) == set(K.BN_SHAPES)
SMALL = [s for s in K.BN_SHAPES if s[0] * s[2] * s[3] < 1000]
LARGE = [s for s in K.BN_SHAPES if s[0] * s[2] * s[3] >= 1000]


@pytest.fixture(scope="module")
def lib():
    return Y.load()


# ---- 1. shards compose to the whole batch (crossed as tests/test_hostsim_batchnorm.py crosses residual x ReLU) ---------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [False, True], ids=["norelu", "relu"])
@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_shards_compose_to_the_whole_batch_small(lib, shape, relu, res, dtype):
    got = Y.bn_sharded(K.case(shape, dtype, res), relu, SHARDS[shape], K.EPS, K.MOMENTUM, lib=lib)
    K.check_bn(f"sim sync bn {shape} = {SHARDS[shape]}", got, K.reference(shape, dtype, res, relu), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("res,relu", [(False, False), (True, True), (False, True)], ids=["plain", "res_relu", "relu"])
@pytest.mark.parametrize("shape", LARGE, ids=str)
def test_shards_compose_to_the_whole_batch_many_chunks(lib, shape, res, relu, dtype):
    assert max(lib.maed_batchnorm_chunks(n) for n in SHARDS[shape]) > 1
    got = Y.bn_sharded(K.case(shape, dtype, res), relu, SHARDS[shape], K.EPS, K.MOMENTUM, lib=lib)
    K.check_bn(f"sim sync bn {shape} = {SHARDS[shape]}", got, K.reference(shape, dtype, res, relu), dtype)


# ---- 2. one shard: the bits of the one-rank entry points ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape,res,relu", [((2, 64, 7, 9), True, True), ((3, 256, 5, 5), False, True), ((1, 2048, 1, 2), False, False), ((3, 64, 21, 21), True, True),
                                            ((2, 72, 3, 3), True, False)], ids=str)
def test_one_shard_is_bit_identical_to_the_one_rank_entry_points(lib, shape, res, relu, dtype):
    """the record is the chunk partials added in finalize's order and the consumers repeat finalize's / bwd_apply's arithmetic: with count = M nothing differs"""
    case = K.case(shape, dtype, res)
    M, C_ = case["x2"].shape
    got = Y.bn_sharded(case, relu, (M,), K.EPS, K.MOMENTUM, lib=lib)
    ref = S.bn_train(case, relu, K.EPS, K.MOMENTUM, lib=lib)
    for k in ("mean", "rstd", "rm", "rv", "y", "dx", "dres", "dgamma", "dbeta"):
        assert (got[k] is None and ref[k] is None) or torch.equal(got[k], ref[k]), k
    part = torch.empty(lib.maed_batchnorm_chunks(M) * C_ * 2, dtype=torch.float64)          # (bn_train does not return mean_lo)
    mean, mlo, rstd = torch.empty(C_), torch.empty(C_), torch.empty(C_)
    S._ok(lib, lib.maed_batchnorm_stats(case["x2"].data_ptr(), M, C_, S._dt(dtype), part.data_ptr(), K.EPS, mean.data_ptr(), mlo.data_ptr(), rstd.data_ptr(), None, None,
                                        K.MOMENTUM, None), "batchnorm_stats")
    assert torch.equal(got["mean_lo"], mlo) and torch.equal(got["mean"], mean)


def test_bad_arguments_are_errors(lib):
    x, f = torch.zeros(4, 16), torch.zeros(16)
    part, rec = torch.zeros(64, dtype=torch.float64), torch.zeros(33, dtype=torch.float64)
    assert lib.maed_batchnorm_stats_local(x.data_ptr(), 4, 12, 0, part.data_ptr(), rec.data_ptr(), None) == -2          # C % 8
    assert lib.maed_batchnorm_stats_local(x.data_ptr(), 0, 16, 0, part.data_ptr(), rec.data_ptr(), None) == -2          # every rank needs a row
    assert lib.maed_batchnorm_stats_local(x.data_ptr(), 4, 16, 0, part.data_ptr(), None, None) == -1
    assert lib.maed_batchnorm_finalize_dev(None, 16, 1e-5, f.data_ptr(), None, f.data_ptr(), None, None, 0.1, None) == -1
    assert lib.maed_batchnorm_bwd_apply_dev(x.data_ptr(), x.data_ptr(), None, f.data_ptr(), None, f.data_ptr(), f.data_ptr(), f.data_ptr(), rec.data_ptr(), None, x.data_ptr(), None,
                                            4, 16, 0, 0, None) == -1                                                      # the count is device data: required


# ---- 3-5. module level, two gloo ranks ------------------------------------------------------------------------------------------------------------------------
CHANNELS, SPLIT = Y.CHANNELS, Y.SPLIT
_Stack, _data, _train = Y.Stack, Y.data, Y.train_step


def _ctx(mode):
    import contextlib
    return Y.patched() if mode == "sim" else contextlib.nullcontext()


class _Counter:
    def __init__(self):
        from maed_amd import ops
        self.n, self.real = 0, ops.StatSync.all_reduce
        counter = self

        def counting(sync, t):
            counter.n += 1
            return counter.real(sync, t)
        ops.StatSync.all_reduce = counting

    def take(self):
        n, self.n = self.n, 0
        return n


def _worker(rank, world, port, out):
    import datetime
    import torch.distributed as dist
    from maed_amd import resnet
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))    # a rank that never arrives is an error, not a wait
    try:
        calls = _Counter()
        lo = sum(SPLIT[:rank])
        sl = slice(lo, lo + SPLIT[rank])
        res = {}
        for mode in ("sim", "torch"):
            with _ctx(mode):
                for C_ in CHANNELS:
                    x, w = _data(C_)
                    model = resnet.convert_sync_batchnorm(_Stack(C_))
                    assert model.bn1.sync is model.bn3.sync and model.bn1.sync.world == 2 and model.bn1.sync.active
                    assert list(model.state_dict()) == list(_Stack(C_).state_dict())
                    y = model(x[sl])
                    fwd_calls = calls.take()
                    (y * w[sl]).sum().backward()
                    bwd_calls = calls.take()
                    model.zero_grad()
                    r = _train(model, x[sl], w[sl])              # second step: num_batches_tracked = 2, buffers moved twice
                    calls.take()
                    model.eval()
                    with torch.no_grad():
                        model(x[sl])
                    r["calls"] = dict(fwd=fwd_calls, bwd=bwd_calls, eval=calls.take())
                    _train(_Stack(C_), x[sl], w[sl])             # not converted: every rank on its own batch
                    r["calls"]["unconverted"] = calls.take()
                    res[(mode, C_)] = r
                # one row on rank 1, two on rank 0
                g = torch.Generator().manual_seed(7)
                x1, w1 = torch.randn(3, 8, 1, 1, generator=g).contiguous(memory_format=torch.channels_last), torch.randn(3, 8, 1, 1, generator=g)
                one = slice(0, 2) if rank == 0 else slice(2, 3)
                res[(mode, "one_row")] = _train(resnet.convert_sync_batchnorm(_Stack(8)), x1[one], w1[one])
                assert calls.take() == 6
        out[rank] = res
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks():
    """both ranks' results (spawned once for tests 3 to 5) and the single-process runs of the whole batch"""
    import torch.multiprocessing as mp
    S.build()
    world, port = 2, 28433 + os.getpid() % 1000          # below the ephemeral range, clear of the other files' ports
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    whole = {}
    for mode in ("sim", "torch"):
        with _ctx(mode):
            for C_ in CHANNELS:
                x, w = _data(C_)
                model = _Stack(C_)
                _train(model, x, w)
                model.zero_grad()
                whole[(mode, C_)] = _train(model, x, w)
            g = torch.Generator().manual_seed(7)
            x1, w1 = torch.randn(3, 8, 1, 1, generator=g).contiguous(memory_format=torch.channels_last), torch.randn(3, 8, 1, 1, generator=g)
            whole[(mode, "one_row")] = _train(_Stack(8), x1, w1)
    return dict(ranks=[out[0], out[1]], whole=whole)


def _compare(name, ranks, whole):
    """check_bn's fp32 bars: y at tol(4), dx at tol(2), affine gradients at affine_tol, running buffers at rtol 1e-5 / atol 2e-7"""
    f32 = torch.float32
    K.close(name + " y", torch.cat([r["y"] for r in ranks]), whole["y"], **K.tol(f32, 4))
    K.close(name + " dx", torch.cat([r["dx"] for r in ranks]), whole["dx"], **K.tol(f32, 2))
    for k in whole:
        if k.startswith("grad."):
            K.close(f"{name} {k}", sum(r[k] for r in ranks), whole[k], **K.affine_tol(f32, whole[k]))
        elif k.startswith("buf.") and k.endswith("num_batches_tracked"):
            assert all(int(r[k]) == int(whole[k]) for r in ranks), k
        elif k.startswith("buf."):
            assert torch.equal(ranks[0][k], ranks[1][k]), f"{k}: the ranks' running buffers differ"
            K.close(f"{name} {k}", ranks[0][k], whole[k], rtol=1e-5, atol=2e-7)


@pytest.mark.parametrize("C_", CHANNELS)
@pytest.mark.parametrize("mode", ["sim", "torch"])
def test_two_gloo_ranks_reproduce_the_whole_batch(two_ranks, mode, C_):
    """3 + 1 images: outputs, input gradients, summed parameter gradients and running buffers after two steps against one process with all 4 images"""
    ranks, whole = [r[(mode, C_)] for r in two_ranks["ranks"]], two_ranks["whole"][(mode, C_)]
    assert int(whole["buf.bn1.num_batches_tracked"]) == 2
    _compare(f"gloo x2 {mode} C={C_}", ranks, whole)


@pytest.mark.parametrize("mode", ["sim", "torch"])
def test_collectives_on_two_ranks_one_per_layer_and_direction(two_ranks, mode):
    for r in two_ranks["ranks"]:
        for C_ in CHANNELS:
            assert r[(mode, C_)]["calls"] == dict(fwd=3, bwd=3, eval=0, unconverted=0), r[(mode, C_)]["calls"]


@pytest.mark.parametrize("mode", ["sim", "torch"])
def test_world_of_one_issues_no_collective_and_keeps_the_bits(mode, monkeypatch):
    from maed_amd import ops, resnet
    n = []
    monkeypatch.setattr(ops.StatSync, "all_reduce", lambda self, t: n.append(1))
    with _ctx(mode):
        x, w = _data(8)
        plain = _train(_Stack(8), x, w)
        model = resnet.convert_sync_batchnorm(_Stack(8))
        assert model.bn2.sync.world == 1 and not model.bn2.sync.active
        conv = _train(model, x, w)
        model.eval()
        model(x)
    assert n == []
    for k in plain:
        assert torch.equal(plain[k], conv[k]), k


@pytest.mark.parametrize("mode", ["sim", "torch"])
def test_one_row_per_rank_is_legal_when_the_global_count_exceeds_one(two_ranks, mode):
    ranks, whole = [r[(mode, "one_row")] for r in two_ranks["ranks"]], two_ranks["whole"][(mode, "one_row")]
    assert ranks[1]["y"].shape[0] == 1
    _compare(f"gloo x2 {mode} one row", ranks, whole)


@pytest.mark.parametrize("mode", ["sim", "torch"])
def test_one_value_per_channel_is_still_an_error_in_a_world_of_one(mode):
    from maed_amd import resnet
    with _ctx(mode):
        bn = resnet.convert_sync_batchnorm(resnet.BatchNorm2d(16))
        with pytest.raises(ValueError, match="more than 1 value per channel"):
            bn(torch.randn(1, 16, 1, 1))


def test_nine_argument_call_of_the_function_still_works():
    """ops.BatchNormFn.apply without the trailing reducer (tests/test_gpu_cnn.py calls it that way): the backward's extra None is dropped by autograd"""
    from maed_amd import ops
    with Y.patched():
        x = torch.randn(2, 8, 3, 3).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        g, b = torch.ones(8, requires_grad=True), torch.zeros(8, requires_grad=True)
        y = ops.BatchNormFn.apply(x, None, g, b, None, True, 0.1, 1e-5, True)
        y.sum().backward()
        assert x.grad is not None and g.grad is not None
