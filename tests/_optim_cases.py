"""Shared cases of tests/test_hostsim_optimizers.py (host simulator) and tests/test_gpu_optimizers.py (device): sizes, fp64 references of maed_grad_norm and of
the three update rules of maed_opt_step (torch's definitions, include/maed_hip.h), ragged segment tables and the tiny models of tests/test_hostsim_optim.py."""
import math

import numpy as np
import torch
import torch.nn as nn

ADAM, ADAMW, SGD = 0, 1, 2                                              # maed_opt_args.kind
NORM_SIZES = (1, 3, 255, 256, 1023, 1024, 1025, 65537, 1000003)         # around one float4, one wave, one workgroup (1024 elements), several workgroups, an odd large size
NORM_GSCALES = (1.0, 0.5)
NORM_RTOL = 2e-5            # the kernel's addition chains are <= 256 long and every term is >= 0: 256 * 2^-24 = 1.5e-5 on the sum, half that on the norm
STEP_SIZES = (5, 1024, 1000003)
STEP_RTOL, STEP_ATOL = 2e-5, 2e-7                                       # the project's Adam tolerance (tests/test_hostsim_optim.py)
SENTINEL = -77.5            # exact in bf16 too
HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2, step=3, momentum=0.9, gscale=0.5)


class Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.decoder = nn.Linear(7, 5)                       # arena order (forward-order key) differs from definition order
        self.encoder = nn.ModuleDict({"blocks": nn.ModuleList([nn.Linear(6, 7), nn.Linear(7, 7)])})

    def forward(self, x):
        for b in self.encoder["blocks"]:
            x = torch.tanh(b(x))
        return self.decoder(x)


class TinyWithUnused(Tiny):
    def __init__(self):
        super().__init__()
        self.encoder["spare"] = nn.Linear(7, 7)               # a parameter pair that never takes part in the forward


def warm(epoch):      # train.py:123, as tests/test_hostsim_optim.py
    return (epoch + 1) * 0.2 if epoch < 3 else 0.1 ** len([m for m in (4,) if m <= epoch])


def named_groups(model):
    """the parameter groups lib/utils/utils.py:120-135 builds"""
    return [{"params": p, "name": n} for n, p in model.named_parameters()]


def norm_input(n, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(n, generator=g) * 3.0


def ref_sqnorm(g, gscale):
    """fp64, from the same fp32 inputs"""
    return float(((g.double().cpu() * gscale) ** 2).sum())


def ref_coef(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6)) if max_norm and max_norm > 0 else 1.0


def read_record(rec):
    """maed_clip_state -> (sqnorm, norm, coef, nonfinite)"""
    host = rec.detach().cpu().contiguous()
    f = host.numpy().view(np.float32)
    return float(f[0]), float(f[1]), float(f[2]), int(host.numpy().view(np.uint32)[3])


def step_inputs(n, seed=0):
    """p, g, m, v as fp32, with v >= m^2 as in any state Adam itself produced (up to its constants): |m| / sqrt(v) <= 1 bounds the update by lr-sized steps.  With
    an independent v, one element in a million has v ~ 1e-9 under m ~ 0.1: its update is several units, fp32 carries it to 1e-7 of THAT, and where the new parameter
    lands near zero no tolerance relative to the result can hold -- a statement about the inputs, not about the kernel."""
    g = torch.Generator().manual_seed(2000 + seed)
    p, gr, m = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    return p, gr, m, m * m + torch.rand(n, generator=g) * 0.01


def ref_step(kind, p, g, m, v, lr, beta1, beta2, eps, wd, step, momentum, gscale, nesterov=False, coef=1.0):
    """one step of the rule in fp64 from fp32 inputs -> (p, m, v) in fp64; the scalars are the fp32 values the kernel receives"""
    f = lambda x: float(np.float32(x))
    lr, beta1, beta2, eps, wd, momentum, gscale, coef = map(f, (lr, beta1, beta2, eps, wd, momentum, gscale, coef))
    bc1, bc2 = f(1.0 - beta1 ** step), f(1.0 - beta2 ** step)
    p, g, m, v = (t.double().cpu() for t in (p, g, m, v))
    gp = g * gscale * coef
    if kind == SGD:
        d = gp + wd * p
        if momentum != 0:
            m = momentum * m + d
            d = d + momentum * m if nesterov else m
        return p - lr * d, m, v
    if kind == ADAMW:
        p = p * (1.0 - lr * wd)
        gr = gp
    else:
        gr = wd * p + gp
    m = beta1 * m + (1 - beta1) * gr
    v = beta2 * v + (1 - beta2) * gr * gr
    return p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps), m, v


def ragged_segments(n, count, seed=0, lr=1e-2, wd=1e-2):
    """`count` disjoint segments over [0, n), sorted: begins are multiples of 4, most ends are not, there are gaps between them, entry 1 is empty, the last one ends
    at n exactly.  Every segment has its own lr / weight_decay."""
    rng = np.random.RandomState(seed)
    pitch = n // count
    segs = []
    for k in range(count):
        lo = (k * pitch + 3) // 4 * 4
        hi = (k + 1) * pitch
        begin = min(hi, lo + 4 * int(rng.randint(0, max(1, (hi - lo) // 16))))
        begin = begin // 4 * 4
        end = begin + int(rng.randint(1, max(2, hi - begin)))
        if k == 1:
            end = begin
        if k == count - 1:
            end = n
        segs.append((begin, min(end, n), lr * (1 + 0.1 * k), wd * (k % 3)))
    return segs


def covered(n, segs):
    mask = torch.zeros(n, dtype=torch.bool)
    for b, e, _, _ in segs:
        mask[b:e] = True
    return mask
