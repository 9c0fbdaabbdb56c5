"""Writes tests/golden/g18_head_sizes.npz: the REFERENCE's own Block (st_mode='parallel') at head sizes 32 / 96 / 128 -- (dim, heads) = (128, 4), (192, 2),
(128, 1) -- and its 'coupling' Attention at (128, 4): parameters, input, output, input gradient and (row-subsampled) parameter gradients against a stored
cotangent, x of shape (6, 5, dim), seqlen 3, eval mode.  CPU only, where a checkout of the reference is present:

    python scripts/make_golden_head_sizes.py

The reference is imported through oracle/ref_shims.py (its stand-ins for packages that need not be installed).  Arrays only; nothing of the reference's text
is stored.  To keep the file small the weight matrices are int8-coded: w = code * scale in fp32, exactly what the reference module is loaded with, so the fixture
is lossless (tests decode with decode_state below); the two dim-128 blocks share one set of parameters (the shapes do not depend on the head count), mlp_ratio is 1
and matrix gradients keep every 16th row.
"""
import argparse
import os
import sys
from functools import partial

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW_STEP = 16
CASES = [("b128h4", "s128", 128, 4), ("b192h2", "s192", 192, 2), ("b128h1", "s128", 128, 1)]


def coded_state(module, seed):
    """non-trivial parameters: matrices as int8 codes x one fp32 scale (3 sigma = code 127, sigma = 0.06), vectors in fp32 (LayerNorm weights around 1)"""
    g = torch.Generator().manual_seed(seed)
    fx, sd = {}, {}
    for n, p in module.state_dict().items():
        if p.dim() == 2:
            code = torch.randn(p.shape, generator=g).mul(127 / 3).round().clamp(-127, 127).to(torch.int8)
            scale = np.float32(0.18 / 127)
            fx["q." + n], fx["scale." + n] = code.numpy(), scale
            sd[n] = torch.from_numpy(code.numpy().astype(np.float32) * scale)
        else:
            v = (1.0 if n.endswith("weight") else 0.0) + 0.2 * torch.randn(p.shape, generator=g)
            fx["v." + n] = v.numpy()
            sd[n] = v
    return fx, sd


def decode_state(fx, prefix):
    """the state dict coded_state wrote under `prefix` (tests import this)"""
    sd = {}
    for k in fx.files:
        if k.startswith(prefix + "q."):
            n = k[len(prefix) + 2:]
            sd[n] = torch.from_numpy(fx[k].astype(np.float32) * np.float32(fx[prefix + "scale." + n]))
        elif k.startswith(prefix + "v."):
            sd[k[len(prefix) + 2:]] = torch.from_numpy(fx[k])
    return sd


def grads_np(module, prefix):
    return {prefix + k: (p.grad[::ROW_STEP] if p.dim() == 2 else p.grad).detach().numpy() for k, p in module.named_parameters() if p.grad is not None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g18_head_sizes.npz"))
    args = ap.parse_args()
    from oracle import ref_shims
    ref_shims.install(smpl_seed=0)
    import lib.models.vision_transformer as vt
    LN = partial(nn.LayerNorm, eps=1e-6)
    g = torch.Generator().manual_seed(18)
    out = dict(row_step=ROW_STEP, seqlen=3)
    states = {}
    for tag, stag, dim, heads in CASES:
        blk = vt.Block(dim, heads, mlp_ratio=1, qkv_bias=True, norm_layer=LN, st_mode="parallel").eval()
        if stag not in states:
            fx, states[stag] = coded_state(blk, seed=dim)
            out.update({f"{stag}.{k}": v for k, v in fx.items()})
            out[f"{stag}.x"] = torch.randn(6, 5, dim, generator=g).numpy()
            out[f"{stag}.cot"] = torch.randn(6, 5, dim, generator=g).numpy()
        blk.load_state_dict(states[stag])
        x = torch.from_numpy(out[f"{stag}.x"]).clone().requires_grad_(True)
        y = blk(x, 3)
        (y * torch.from_numpy(out[f"{stag}.cot"])).sum().backward()
        out.update({f"{tag}.out": y.detach().numpy(), f"{tag}.dx": x.grad.numpy(), f"{tag}.dim": dim, f"{tag}.heads": heads, f"{tag}.state": stag})
        out.update(grads_np(blk, f"{tag}.grad."))
    # the coupling Attention at (128, 4): the attention parameters of s128 minus ts_attn
    att = vt.Attention(128, num_heads=4, qkv_bias=True, st_mode="coupling").eval()
    att.load_state_dict({k[len("attn."):]: v for k, v in states["s128"].items() if k.startswith("attn.") and "ts_attn" not in k})
    x = torch.from_numpy(out["s128.x"]).clone().requires_grad_(True)
    y = att(x, 3)
    (y * torch.from_numpy(out["s128.cot"])).sum().backward()
    out.update({"c128h4.out": y.detach().numpy(), "c128h4.dx": x.grad.numpy()})
    out.update(grads_np(att, "c128h4.grad."))
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
