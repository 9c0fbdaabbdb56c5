"""One fused STE block, forward + backward, bf16, at cfg3's block dims (F=128, P=197, C=512, H=8, T=16, hidden 2048): rates 0 (today's entry points) against
drop = drop_path = 0.1 (maed_ste_block_fwd_reg / _bwd_reg: masks in the proj / fc1 / fc2 epilogues, two masked casts in the backward).

    python scripts/ste_drop_micro.py [--iters 30] [--out profiles/ste_drop_ab.txt]

Each leg is a fresh child process under `timeout`; the legs are chained: the first one that fails (or runs into its limit) ends the script with its status and
nothing more is started on the GPU.  `--leg NAME` runs one leg in this process."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {"rate0": (0.0, 0.0), "drop0.1_path0.1": (0.1, 0.1)}
DIMS = dict(F=128, P=197, C=512, H=8, T=16)


def leg(name, iters):
    sys.path.insert(0, ROOT)
    from functools import partial
    import torch
    import torch.nn as nn
    from maed_amd.vision_transformer import Block
    drop, drop_path = LEGS[name]
    torch.manual_seed(0)
    blk = Block(DIMS["C"], DIMS["H"], mlp_ratio=4, qkv_bias=True, drop=drop, drop_path=drop_path, norm_layer=partial(nn.LayerNorm, eps=1e-6), st_mode="parallel",
                compute_dtype=torch.bfloat16).cuda().train()
    x = torch.randn(DIMS["F"], DIMS["P"], DIMS["C"], device="cuda", requires_grad=True)
    dy = torch.randn(DIMS["F"], DIMS["P"], DIMS["C"], device="cuda")

    def step():
        blk(x, DIMS["T"]).backward(dy)

    for _ in range(5):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(3):      # three timed batches: their spread is the figure's error bar
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            step()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / iters)
    print(f"ste_drop_micro {name:16s} F={DIMS['F']} P={DIMS['P']} C={DIMS['C']} bf16 fwd+bwd: " + " ".join(f"{t:.3f}" for t in times) + f" ms per block (min {min(times):.3f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=list(LEGS))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--limit", type=int, default=120, help="seconds per leg")
    args = ap.parse_args()
    if args.leg:
        return leg(args.leg, args.iters)
    for name in LEGS:
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--leg", name, "--iters", str(args.iters)],
                           capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(f"ste_drop_micro: leg {name} ended with status {r.returncode}; stopping", flush=True)
            return r.returncode
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(r.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
