"""Attention and fused-block timings per head size at the cfg3 token geometry (F = 128 frames, P = 197 tokens, T = 16, C = 768):
H = 24 / 8 / 6 (head sizes 32 / 96 / 128, csrc/attn_heads.hip) next to H = 12 (head size 64, the tuned kernels).  bf16.  Needs the GPU.

    python scripts/head_sizes_micro.py [OUT.txt]

Times are device events around `iters` back-to-back calls after `warm` warm-up calls; FLOPs are the algorithm's (4 L^2 D per sequence forward,
2.5 x that backward with the recompute counted once)."""
import os
import sys
from functools import partial

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maed_amd import ops                                           # noqa: E402
from maed_amd.vision_transformer import Block                       # noqa: E402

F_, P, T, C = 128, 197, 16, 768
DEV = "cuda"


def timed(fn, warm=5, iters=30):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters      # us per call


def main():
    if not torch.cuda.is_available():
        raise SystemExit("head_sizes_micro: no GPU")
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    say(f"# bf16, F={F_} P={P} T={T} C={C}; us per call (device events, 30 calls after 5 warm-up); TFLOP/s = algorithmic FLOPs / time")
    say(f"{'H':>3} {'D':>4} | {'sp fwd':>8} {'TF/s':>6} {'sp bwd':>8} {'TF/s':>6} | {'tm fwd':>8} {'tm bwd':>8} | {'block fwd+bwd ms':>16}")
    g = torch.Generator().manual_seed(0)
    for H in (12, 24, 8, 6):
        D = C // H
        qkv = torch.randn(F_, P, 3 * C, generator=g).to(torch.bfloat16).to(DEV)
        do = torch.randn(F_, P, C, generator=g).to(torch.bfloat16).to(DEV)
        dqkv = torch.empty_like(qkv)
        o, lse = ops.attn_spatial_fwd(qkv, H)
        ot, lset = ops.attn_temporal_fwd(qkv, H, T)
        sf = timed(lambda: ops.attn_spatial_fwd(qkv, H))
        sb = timed(lambda: ops.attn_spatial_bwd(qkv, o, do, lse, H, dqkv=dqkv))
        tf = timed(lambda: ops.attn_temporal_fwd(qkv, H, T))
        tb = timed(lambda: ops.attn_temporal_bwd(qkv, ot, do, lset, H, T, dqkv=dqkv))
        fl = 4.0 * F_ * H * P * P * D
        blk = Block(C, H, mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), st_mode="parallel", compute_dtype=torch.bfloat16).to(DEV)
        x = torch.randn(F_, P, C, generator=g).to(DEV).requires_grad_(True)
        dy = torch.randn(F_, P, C, generator=g).to(DEV)

        def step():
            y = blk(x, T)
            y.backward(dy)

        bs = timed(step, warm=3, iters=10) / 1e3
        say(f"{H:>3} {D:>4} | {sf:8.1f} {fl / sf / 1e6:6.1f} {sb:8.1f} {2.5 * fl / sb / 1e6:6.1f} | {tf:8.1f} {tb:8.1f} | {bs:16.3f}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
