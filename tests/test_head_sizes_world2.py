"""Two gloo ranks on a box without GPUs: a FUSED STE block with head size 32 (dim 128, 4 heads; kernels on the host simulator) under ParamArena + GradBucketer.
The block's kernels write every parameter gradient themselves and report once, through `grads_ready`: every parameter must reach the bucketer exactly once per
backward, every bucket must launch exactly once, and the all-reduced gradient must equal the single-process gradient of the whole batch."""
import os
import sys
from functools import partial

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

C, H, T, P = 128, 4, 3, 5


def _block():
    from maed_amd.vision_transformer import Block
    torch.manual_seed(0)
    return Block(C, H, mlp_ratio=2, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), st_mode="parallel", compute_dtype=torch.float32)


def _batch(world):
    g = torch.Generator().manual_seed(5)
    return torch.randn(world * T, P, C, generator=g), torch.randn(world * T, P, C, generator=g)


def _worker(rank, world, port, out):
    import torch.distributed as dist
    from _hostsim import patched
    from maed_amd.ddp import GradBucketer, ParamArena
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        with patched():
            blk = _block()
            arena = ParamArena(blk, device=torch.device("cpu"))
            bucketer = GradBucketer(arena, blk, bucket_bytes=64 << 10)
            assert bucketer.collectives and len(bucketer.buckets) > 1
            assert bucketer._fused == {id(p) for p in blk.parameters()}            # the fused backward owns every gradient of the block
            reports, marked = [], []
            real_mark = bucketer._mark

            def counting_mark(p):
                i = arena.index[id(p)]
                if not bucketer._seen[i]:
                    marked.append(i)
                real_mark(p)

            bucketer._mark = counting_mark
            blk.grads_ready = lambda b: (reports.append(1), bucketer._block_ready(b))
            x, dy = _batch(world)
            shard = slice(rank * T, rank * T + T)
            for step in range(2):
                arena.zero_grad()
                del reports[:], marked[:]
                (blk(x[shard], T) * dy[shard]).sum().backward()
                assert len(reports) == 1, reports
                assert sorted(marked) == list(range(len(arena.params))), marked      # every gradient handed over exactly once
                assert sorted(bucketer.launch_order) == list(range(len(bucketer.buckets))), bucketer.launch_order
                bucketer.finish()
            out[rank] = arena.grad.clone()
    finally:
        dist.destroy_process_group()


def test_fused_block_with_head_size_32_hands_every_gradient_to_the_bucketer_once_on_two_ranks():
    import torch.multiprocessing as mp
    from _hostsim import patched
    from maed_amd.ddp import ParamArena
    sys.path.insert(0, os.path.join(HERE, "hostsim"))
    import build_sim
    build_sim.build()
    world = 2
    port = 30633 + os.getpid() % 1000
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    assert torch.equal(out[0], out[1]), "every rank must hold the same reduced gradient"
    with patched():
        blk = _block()
        arena = ParamArena(blk, device=torch.device("cpu"))
        x, dy = _batch(world)
        arena.zero_grad()
        (blk(x, T) * dy).sum().backward()
    # (sum of the ranks' gradients of a summed loss = the whole batch's gradient; weight gradients meet in another order: fp32 rounding only)
    torch.testing.assert_close(out[0], arena.grad, rtol=1e-4, atol=1e-5 * float(arena.grad.abs().max()))
