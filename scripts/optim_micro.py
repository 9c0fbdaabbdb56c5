"""The optimizer stage alone over a cfg3-sized arena (39.7 M fp32 parameters, 307 tensors): maed_adam_step (the benchmarked path, unchanged), the global gradient
norm, norm + clipped Adam, one segment launch with 307 segments against 307 per-tensor launches, and SGD with momentum (docs/design/15_optimizers.md).

    python scripts/optim_micro.py [--iters 50] [--out profiles/optim_micro.txt]

Times come from device events around `iters` back-to-back calls, three batches per leg (their spread is the error bar); GB/s is the bytes the rule has to move
(reads + writes of the arenas it touches) over that time.  Each leg is a fresh child process under `timeout`; the legs are chained: the first one that fails (or
runs into its limit) ends the script with its status and nothing more is started on the GPU.  `--leg NAME` runs one leg in this process."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TENSORS, N_BIG = 307, 100
N_TOTAL = 39_700_000 // 64 * 64
LEGS = ["adam_step", "grad_norm", "norm_clipped_adam", "segments_307", "per_tensor_307", "sgd_momentum"]


def tensors():
    """(offset, numel) of 307 tensors in an arena of N_TOTAL floats: 207 vectors of 512 .. 2048 elements (biases, norm scales) between 100 equal matrices, every
    offset a multiple of 64 as ParamArena lays them out"""
    small = [512 * (1 + k % 4) for k in range(N_TENSORS - N_BIG)]
    big = (N_TOTAL - sum(small)) // N_BIG // 64 * 64
    sizes, s, b = [], 0, 0
    for k in range(N_TENSORS):
        if k % 3 == 0 and b < N_BIG:
            sizes.append(big); b += 1
        elif s < len(small):
            sizes.append(small[s]); s += 1
        else:
            sizes.append(big); b += 1
    out, off = [], 0
    for n in sizes:
        out.append((off, n))
        off += n
    assert off <= N_TOTAL and len(out) == N_TENSORS
    return out


def leg(name, iters):
    sys.path.insert(0, ROOT)
    import torch
    from maed_amd import ops, _lib as L
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    n = N_TOTAL
    p, g = torch.randn(n, device=dev), torch.randn(n, device=dev) * 1e-2
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    partials = torch.empty(ops.grad_norm_partials(), dtype=torch.float32, device=dev)
    rec = ops.clip_record(dev)
    tens = tensors()
    hyper = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-5, step=10)
    arenas = {"adam_step": 7, "grad_norm": 1, "norm_clipped_adam": 8, "segments_307": 7, "per_tensor_307": 7, "sgd_momentum": 5}[name]     # reads + writes, in arenas
    if name == "adam_step":
        call = lambda: ops.adam_step(p, g, m, v, None, 1e-4, 0.9, 0.999, 1e-8, 1e-5, 10)
    elif name == "grad_norm":
        call = lambda: ops.grad_norm(g, 1.0, 1.0, partials, rec)
    elif name == "norm_clipped_adam":
        def call():
            ops.grad_norm(g, 1.0, 1.0, partials, rec)
            ops.opt_step(L.OPT_ADAM, p, g, m, v, None, clip=rec, **hyper)
    elif name == "segments_307":
        tab = ops.opt_segments([(o, o + k, 1e-4 * (1 + i % 3), 1e-5 * (i % 2)) for i, (o, k) in enumerate(tens)], dev)
        call = lambda: ops.opt_step(L.OPT_ADAM, p, g, m, v, None, segments=tab, n_segments=len(tens), **hyper)
    elif name == "per_tensor_307":
        views = [(p[o:o + k], g[o:o + k], m[o:o + k], v[o:o + k], 1e-4 * (1 + i % 3), 1e-5 * (i % 2)) for i, (o, k) in enumerate(tens)]

        def call():
            for pp, gg, mm, vv, lr, wd in views:
                ops.adam_step(pp, gg, mm, vv, None, lr, 0.9, 0.999, 1e-8, wd, 10)
    else:
        call = lambda: ops.opt_step(L.OPT_SGD, p, g, m, None, None, lr=1e-4, wd=1e-5, momentum=0.9)
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(3):      # three timed batches: their spread is the figure's error bar
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        times.append(1e3 * e0.elapsed_time(e1) / iters)
    best = min(times)
    print(f"optim_micro {name:18s} n={n} fp32: " + " ".join(f"{t:.1f}" for t in times) + f" us per step (min {best:.1f}; {arenas} x {4e-6 * n:.0f} MB moved: "
          f"{arenas * 4 * n / best / 1e3:.0f} GB/s)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--iters", type=int, default=50)
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
            print(f"optim_micro: leg {name} ended with status {r.returncode}; stopping", flush=True)
            return r.returncode
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(r.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
