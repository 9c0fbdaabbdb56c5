"""GPU tests of the BatchNorm statistics over the batch of all ranks (resnet.convert_sync_batchnorm; docs/design/16_sync_batchnorm.md).  One GPU: the shards of
a case stand for the ranks and their records are added on the device (the sequence of tests/_hostsim_syncbn.bn_sharded on the product library), and the
collectives run over a world of one, forced -- through torch.distributed's nccl group and through the library's own communicator."""
import os

import pytest
import torch

import _batchnorm_cases as K
import _hostsim_syncbn as Y
from _util import DEV, report

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
SHARDS = {(2, 64, 7, 9): (37, 89), (1, 2048, 1, 2): (1, 1), (4, 64, 40, 40): (1323, 5077), (3, 256, 5, 5): (5, 32, 38)}
MARGIN = 256            # bytes of sentinel on either side of an output
SENTINEL = 0xA5


class Margins:
    """tests/_hostsim_batchnorm.Guarded on the device: the tensor a kernel writes lies inside a larger sentinel-filled allocation"""
    live = []

    def __init__(self, shape, dtype, fill=None):
        n = 1
        for s in shape:
            n *= s
        nbytes = n * torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((nbytes + 2 * MARGIN,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.t = self.buf[MARGIN:MARGIN + nbytes].view(dtype).view(shape)
        if fill is not None:
            self.t.copy_(fill)
        Margins.live.append(self)

    @staticmethod
    def check_all(what):
        torch.cuda.synchronize()
        for g in Margins.live:
            assert bool((g.buf[:MARGIN] == SENTINEL).all()) and bool((g.buf[-MARGIN:] == SENTINEL).all()), f"{what}: bytes outside an output were written"
        Margins.live.clear()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("res,relu", [(False, False), (True, True), (False, True)], ids=["plain", "res_relu", "relu"])
@pytest.mark.parametrize("shape", list(SHARDS), ids=str)
def test_shards_compose_to_the_whole_batch_on_the_device(shape, res, relu, dtype):
    from maed_amd import _lib as L
    from maed_amd import ops
    Margins.live.clear()
    got = Y.bn_sharded(K.case(shape, dtype, res), relu, SHARDS[shape], K.EPS, K.MOMENTUM, lib=L.lib(), G=Margins, check_all=Margins.check_all, dev=DEV, stream=ops._stream())
    K.check_bn(f"sync bn {shape} = {SHARDS[shape]} {IDS[DTYPES.index(dtype)]} res={res} relu={relu}", got, K.reference(shape, dtype, res, relu), dtype)


def _stack_pair(C_, **convert):
    """(unconverted, converted) runs of tests/_hostsim_syncbn.Stack on all 4 images, fp32"""
    from maed_amd import resnet
    x, w = Y.data(C_)
    x, w = x.to(DEV), w.to(DEV)
    plain = Y.train_step(Y.Stack(C_).to(DEV), x, w)
    model = resnet.convert_sync_batchnorm(Y.Stack(C_).to(DEV), **convert)
    assert model.bn1.sync.world == 1 and model.bn1.sync.active
    calls = []
    real = model.bn1.sync.all_reduce
    model.bn1.sync.all_reduce = lambda t: (calls.append(t.numel()), real(t))[1]
    conv = Y.train_step(model, x, w)
    torch.cuda.synchronize()
    assert calls == [2 * C_ + 1] * 3 + [2 * C_] * 3, calls
    return plain, conv


def _compare(name, plain, conv):
    """check_bn's fp32 bars (a sum over one rank is the identity and the arithmetic is the one-rank entry points': the difference is expected to be zero)"""
    f32 = torch.float32
    report(name + " y", conv["y"], plain["y"], **K.tol(f32, 4))
    report(name + " dx", conv["dx"], plain["dx"], **K.tol(f32, 2))
    for k in plain:
        if k.startswith("grad."):
            report(f"{name} {k}", conv[k], plain[k], **K.affine_tol(f32, plain[k]))
        elif k.endswith("num_batches_tracked"):
            assert int(conv[k]) == int(plain[k]) == 1
        elif k.startswith("buf."):
            report(f"{name} {k}", conv[k], plain[k], rtol=1e-5, atol=2e-7)


def test_forced_collectives_through_an_nccl_world_of_one():
    """set up and torn down as tests/test_gpu_model.py::test_rccl_bucketed_allreduce_single_rank does"""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 300))
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        created = True
    try:
        for C_ in Y.CHANNELS:
            plain, conv = _stack_pair(C_, force_collectives=True)
            _compare(f"sync bn nccl world 1 C={C_}", plain, conv)
    finally:
        if created:
            dist.destroy_process_group()


@pytest.fixture(scope="module")
def comm():
    from maed_amd.ddp import RcclComm
    c = RcclComm(rank=0, world=1)
    yield c
    c.destroy()


def test_forced_collectives_through_the_librarys_communicator(comm):
    for C_ in Y.CHANNELS:
        plain, conv = _stack_pair(C_, comm=comm, force_collectives=True)
        _compare(f"sync bn RcclComm world 1 C={C_}", plain, conv)


def test_fp64_allreduce_over_one_rank_is_the_identity(comm):
    buf = torch.arange(1 << 16, dtype=torch.float64, device=DEV) * 1.0000001 + 1e-9
    want = buf.clone()
    comm.allreduce_f64_async(buf)
    comm.wait()
    torch.cuda.synchronize()
    assert torch.equal(buf, want)


def test_full_cnn_model_converted_and_forced_matches_the_unconverted_model(comm):
    """MAED(encoder='cnn') at (2, 2, 3, 64, 64), fp32, train mode: all 53 norm layers through the record + collective path; the bar tests/test_gpu_cnn.py uses for
    the fp32 features (rtol 1e-3, atol 1e-4)"""
    import copy
    import _resnet50_ref as RR
    from maed_amd import resnet
    from maed_amd.maed import MAED
    from _util import rnd
    torch.manual_seed(11)
    m = MAED(encoder="cnn", compute_dtype=torch.float32)
    RR.randomise(m.encoder, 11)
    m = m.to(DEV).train()
    s = copy.deepcopy(m)
    resnet.convert_sync_batchnorm(s, comm=comm, force_collectives=True)
    assert sum(1 for mod in s.modules() if isinstance(mod, resnet.BatchNorm2d) and mod.sync is not None and mod.sync.active) == 53
    assert list(s.state_dict()) == list(m.state_dict())
    clip = rnd(2, 2, 3, 64, 64, seed=21).to(DEV)
    feat = m.extract_feature(clip)
    feat_s = s.extract_feature(clip)
    feat_s.square().mean().backward()
    torch.cuda.synchronize()
    report("cnn f32 extract_feature, converted vs unconverted", feat_s, feat, rtol=1e-3, atol=1e-4)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in s.encoder.parameters())
    assert int(s.encoder.bn1.num_batches_tracked) == 1
