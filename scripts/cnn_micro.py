"""Stage-1 encoder (MAED(encoder='cnn'), maed_amd/resnet.py) in isolation at the stage-1 size of config_stage1.yaml -- 128 frames of 3 x 224 x 224 per GPU, bf16 --
timed with device events: every distinct BatchNorm site shape forward and backward, the two pools, and the whole encoder forward + backward.
Every row alternates the library kernels (csrc/batchnorm.hip) with the framework composition (MAED_CNN_BN=torch: F.batch_norm + add + ReLU, F.max_pool2d,
adaptive_avg_pool2d) inside one loop, after a warm-up, so that both arms see the same clocks.  Bytes are computed from the shapes for the LIBRARY's passes
(forward: statistics read + apply read / write [+ residual read, + 1 bit per element]; backward: reduce reads x, dy + apply reads x, dy, writes dx [+ dres]);
"share" is those bytes over the measured time against the ~6.3 TB/s an MI355X sustains from HBM.  Reads nothing outside the tree.
usage: cnn_micro.py [output file, default profiles/cnn_micro.txt] [frames, default 128]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MAED_SYNTHETIC_SMPL_OK", "1")
from maed_amd import resnet  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cnn_micro.txt")
FRAMES = int(sys.argv[2]) if len(sys.argv) > 2 else 128
HBM = 6.3e12
DT = torch.bfloat16
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


_BALLAST = None


def ballast(ms=25.0):
    """keeps the GPU busy for about `ms` so that the host can enqueue a whole timing block behind it: the events then see the kernels back to back on the device,
    not the host's launch rate (a synchronised loop measures 100+ us of Python per call at the small shapes)"""
    global _BALLAST
    if _BALLAST is None:
        _BALLAST = torch.empty(1 << 30, dtype=torch.uint8, device="cuda").zero_()       # 1 GiB: an in-place add moves 2 GiB, ~0.45 ms
    for _ in range(int(ms / 0.45)):
        _BALLAST.add_(1)


def timed(fwd, bwd, iters=5, rounds=2, warm=2):
    """{arm: (fwd ms, bwd ms)} over `rounds` alternating blocks of `iters` iterations per arm; fwd(arm) -> state, bwd(arm, state)"""
    acc = {True: [0.0, 0.0], False: [0.0, 0.0]}
    for arm in (True, False):
        resnet._LIB_BN = arm
        for _ in range(warm):
            st = fwd(arm)
            if bwd is not None:
                bwd(arm, st)
            del st
    torch.cuda.synchronize()
    for _ in range(rounds):
        for arm in (True, False):
            resnet._LIB_BN = arm
            ev = []
            ballast()
            for _ in range(iters):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                st = fwd(arm)
                e[1].record()
                if bwd is not None:
                    bwd(arm, st)
                e[2].record()
                ev.append(e)
                del st
            torch.cuda.synchronize()
            for e in ev:
                acc[arm][0] += e[0].elapsed_time(e[1]) / (iters * rounds)
                acc[arm][1] += e[1].elapsed_time(e[2]) / (iters * rounds)
    resnet._LIB_BN = True
    return acc


def row(name, nbytes_f, nbytes_b, acc):
    lf, lb = acc[True]
    ff, fb = acc[False]

    def share(nbytes, ms):
        return f"{nbytes / 1e6:8.1f} MB {ms * 1e3:8.1f} us {nbytes / (ms * 1e-3) / HBM:5.2f}" if nbytes else f"{'':8s}    {ms * 1e3:8.1f} us      "

    slower = [d for d, a, b in (("fwd", lf, ff), ("bwd", lb, fb)) if a > b * 1.02]
    say(f"{name:44s} lib fwd {share(nbytes_f, lf)} | lib bwd {share(nbytes_b, lb)} | framework fwd {ff * 1e3:8.1f} us bwd {fb * 1e3:8.1f} us"
        + (f"   LIBRARY SLOWER: {', '.join(slower)}" if slower else ""))


def bn_sites(enc, H):
    """distinct (rows per frame, C, residual, relu) of the 53 BatchNorm sites"""
    sites, seen = [], set()
    h = H // 2

    def add(hw, C_, res, relu):
        k = (hw, C_, res, relu)
        if k not in seen:
            seen.add(k)
            sites.append(k)

    add(h * h, 64, False, True)
    h = (h - 1) // 2 + 1
    for layer in (enc.layer1, enc.layer2, enc.layer3, enc.layer4):
        for blk in layer:
            ho = (h - 1) // blk.stride + 1
            add(h * h, blk.bn1.num_features, False, True)
            add(ho * ho, blk.bn2.num_features, False, True)
            if blk.downsample is not None:
                add(ho * ho, blk.bn3.num_features, False, False)
            add(ho * ho, blk.bn3.num_features, True, True)
            h = ho
    return sites


def main():
    assert torch.cuda.is_available(), "cnn_micro needs a GPU"
    dev = torch.device("cuda")
    say(f"device {torch.cuda.get_device_name(0)}; {FRAMES} frames of 3 x 224 x 224, bf16; per row 2 x 5 timed iterations per arm after warm-up, library and framework arms alternating, each block enqueued behind ~25 ms of other work;")
    say(f"share = bytes / time / {HBM / 1e12:.1f} TB/s")
    enc = resnet.resnet50(compute_dtype=DT).to(dev).train()
    for hw, C_, res, relu in bn_sites(enc, 224):
        side = int(round(hw ** 0.5))
        M = FRAMES * hw
        bn = resnet.BatchNorm2d(C_).to(dev).train()
        x = torch.randn(FRAMES, C_, side, side, device=dev, dtype=DT).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        r = torch.randn_like(x).requires_grad_(True) if res else None
        dy = torch.randn_like(x)
        el = M * C_ * 2

        def fwd(arm):
            return bn(x, residual=r, relu=relu)

        def bwd(arm, y):
            x.grad = None
            if r is not None:
                r.grad = None
            bn.weight.grad = bn.bias.grad = None
            y.backward(dy)

        acc = timed(fwd, bwd)
        nf = (3 + (1 if res else 0)) * el + (M * C_ // 8 if (res and relu) else 0)
        nb = (5 + (1 if res else 0)) * el + (2 * M * C_ // 8 if (res and relu) else 0)
        row(f"BN {FRAMES}x{side}x{side}x{C_} res={int(res)} relu={int(relu)}", nf, nb, acc)
        del x, r, dy, bn
    # pools
    x = torch.randn(FRAMES, 64, 112, 112, device=dev, dtype=DT).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    pool = resnet.MaxPool3s2P1()
    dy = torch.randn(FRAMES, 64, 56, 56, device=dev, dtype=DT).contiguous(memory_format=torch.channels_last)
    acc = timed(lambda arm: pool(x), lambda arm, y: (setattr(x, "grad", None), y.backward(dy)))
    n_in, n_out = x.numel() * 2, dy.numel() * 2
    row(f"maxpool {FRAMES}x112x112x64", n_in + n_out + n_out // 2, n_out + n_out // 2 + n_in, acc)
    del x, dy
    x = torch.randn(FRAMES, 2048, 7, 7, device=dev, dtype=DT).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ap = resnet.GlobalAvgPool()
    dyf = torch.randn(FRAMES, 2048, device=dev)
    acc = timed(lambda arm: ap(x), lambda arm, y: (setattr(x, "grad", None), y.backward(dyf.to(y.dtype))))
    row(f"avgpool {FRAMES}x7x7x2048", x.numel() * 2 + dyf.numel() * 4, x.numel() * 2 + dyf.numel() * 4, acc)
    del x
    # the whole encoder
    clip = torch.randn(FRAMES, 3, 224, 224, device=dev)
    routes = [r for _, r in enc.plan(FRAMES, 224, 224)["convs"]]
    say(f"encoder convolutions: {', '.join(f'{routes.count(k)} {k}' for k in sorted(set(routes)))}")

    def efwd(arm):
        return enc(clip)

    def ebwd(arm, y):
        for p in enc.parameters():
            p.grad = None
        y.float().square().mean().backward()

    acc = timed(efwd, ebwd, iters=3, rounds=2, warm=2)
    row(f"encoder {FRAMES}x3x224x224 forward + backward", 0, 0, acc)
    say(f"encoder step: library BN/pools {sum(acc[True]):.2f} ms, framework BN/pools {sum(acc[False]):.2f} ms; peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
