"""What the cross-rank BatchNorm statistics (resnet.convert_sync_batchnorm) cost on ONE GPU: the stage-1 encoder (MAED(encoder='cnn'), maed_amd/resnet.py) forward +
backward at the stage-1 size of config_stage1.yaml -- 128 frames of 3 x 224 x 224, bf16 -- timed with device events, three arms alternating inside one loop on the
same model and the same batch, the way scripts/cnn_micro.py alternates its arms:
  local       not converted: the one-rank entry points (the path of profiles/cnn_micro.txt's last row)
  sync/rccl   converted, collectives forced over a world of one through the library's communicator (ddp.RcclComm: side stream + event fences)
  sync/nccl   converted, collectives forced over a world of one through torch.distributed's nccl process group
A world of one measures the 106 record passes (53 forward, 53 backward), their launches, and the enqueue / fence cost of 106 all-reduces that move nothing.  It
does NOT measure wire latency or a stat collective queueing behind a gradient bucket on the communicator: that needs more than one GPU.
Reads nothing outside the tree.   usage: syncbn_micro.py [output file, default profiles/syncbn_micro.txt] [frames, default 128]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MAED_SYNTHETIC_SMPL_OK", "1")
from maed_amd import ops, resnet  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "syncbn_micro.txt")
FRAMES = int(sys.argv[2]) if len(sys.argv) > 2 else 128
ROUNDS, ITERS, WARM = 4, 4, 2
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


_BALLAST = None


def ballast(ms=25.0):
    """scripts/cnn_micro.ballast: ~`ms` of other work in front of a timing block, so that the events see the kernels back to back, not the host's launch rate"""
    global _BALLAST
    if _BALLAST is None:
        _BALLAST = torch.empty(1 << 30, dtype=torch.uint8, device="cuda").zero_()
    for _ in range(int(ms / 0.45)):
        _BALLAST.add_(1)


def main():
    assert torch.cuda.is_available(), "syncbn_micro needs a GPU"
    import torch.distributed as dist
    from maed_amd.ddp import RcclComm
    dev = torch.device("cuda", 0)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 300))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    comm = RcclComm(rank=0, world=1)
    try:
        enc = resnet.resnet50(compute_dtype=torch.bfloat16).to(dev).train()
        norms = [m for m in enc.modules() if isinstance(m, resnet.BatchNorm2d)]
        arms = {"local": None, "sync/rccl": ops.StatSync(comm=comm, force_collectives=True), "sync/nccl": ops.StatSync(force_collectives=True)}
        assert all(s is None or (s.active and s.world == 1) for s in arms.values())
        clip = torch.randn(FRAMES, 3, 224, 224, device=dev)

        def step(ev=None):
            for p in enc.parameters():
                p.grad = None
            if ev:
                ev[0].record()
            y = enc(clip)
            if ev:
                ev[1].record()
            y.float().square().mean().backward()
            if ev:
                ev[2].record()

        def use(name):
            for m in norms:
                m.sync = arms[name]

        say(f"device {torch.cuda.get_device_name(0)}; encoder forward + backward, {FRAMES} frames of 3 x 224 x 224, bf16, {len(norms)} norm layers; world of one, collectives forced;")
        say(f"{ROUNDS} rounds x {ITERS} timed iterations per arm after {WARM} warm-up iterations per arm, arms alternating, each block enqueued behind ~25 ms of other work")
        for name in arms:
            use(name)
            for _ in range(WARM):
                step()
        torch.cuda.synchronize()
        per_round = {name: [] for name in arms}
        for _ in range(ROUNDS):
            for name in arms:
                use(name)
                ballast()
                evs = []
                for _ in range(ITERS):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    step(ev)
                    evs.append(ev)
                torch.cuda.synchronize()
                per_round[name].append((sum(e[0].elapsed_time(e[1]) for e in evs) / ITERS, sum(e[1].elapsed_time(e[2]) for e in evs) / ITERS))
        base = sum(f + b for f, b in per_round["local"]) / ROUNDS
        for name, rows in per_round.items():
            f, b = sum(r[0] for r in rows) / ROUNDS, sum(r[1] for r in rows) / ROUNDS
            steps = ", ".join(f"{r[0] + r[1]:.2f}" for r in rows)
            say(f"{name:10s} fwd {f:7.3f} ms  bwd {b:7.3f} ms  step {f + b:7.3f} ms  ({(f + b) - base:+.3f} ms vs local)   per round: {steps}")
        use("local")
        say(f"peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    finally:
        comm.destroy()
        dist.destroy_process_group()
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
