"""Head sizes 32 / 96 / 128 against the fixture the REFERENCE's own Block ('parallel') and 'coupling' Attention produced (tests/golden/g18_head_sizes.npz, written by
scripts/make_golden_head_sizes.py): compute_dtype float32 on the "exact" engine, at g13's bars (2e-5 on outputs, 1e-4 on gradients; tests/test_hostsim_modes.py),
on the host simulator and on the GPU.  The bf16 mode of the same blocks is held to fp64 autograd through the oracle in tests/test_hostsim_head_sizes.py /
tests/test_gpu_head_sizes.py."""
import os
import sys
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import maed_ref as R
from maed_amd.vision_transformer import Attention, Block

from _hostsim import patched

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
from make_golden_head_sizes import decode_state  # noqa: E402

LN = partial(nn.LayerNorm, eps=1e-6)
BLOCKS = ["b128h4", "b192h2", "b128h1"]


def t(a):
    return torch.from_numpy(np.asarray(a))


def rel(a, b):
    a, b = a.detach().double().cpu(), t(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def check(module, fx, tag, out, dx):
    step = int(fx["row_step"])
    print(f"{tag}: out {rel(out, fx[tag + '.out']):.2e} dx {rel(dx, fx[tag + '.dx']):.2e}")
    assert rel(out, fx[tag + ".out"]) < 2e-5
    assert rel(dx, fx[tag + ".dx"]) < 1e-4
    for n, p in module.named_parameters():
        want = fx[f"{tag}.grad.{n}"]
        assert p.grad is not None, n
        got = p.grad[::step] if p.dim() == 2 else p.grad
        print(f"{tag}: d[{n}] {rel(got, want):.2e}")
        assert rel(got, want) < 1e-4, (n, rel(got, want))


def run_block(fx, tag, device):
    dim, heads, stag, T = int(fx[tag + ".dim"]), int(fx[tag + ".heads"]), str(fx[tag + ".state"]), int(fx["seqlen"])
    blk = Block(dim, heads, mlp_ratio=1, qkv_bias=True, norm_layer=LN, st_mode="parallel", compute_dtype=torch.float32)
    blk.load_state_dict(decode_state(fx, stag + "."))              # strict: the reference's keys
    blk = blk.to(device)
    x = t(fx[stag + ".x"]).to(device).requires_grad_(True)
    out = blk(x, T)
    (out * t(fx[stag + ".cot"]).to(device)).sum().backward()
    check(blk, fx, tag, out, x.grad)


def run_coupling(fx, device):
    T = int(fx["seqlen"])
    att = Attention(128, num_heads=4, qkv_bias=True, st_mode="coupling")
    att.load_state_dict({k[len("attn."):]: v for k, v in decode_state(fx, "s128.").items() if k.startswith("attn.") and "ts_attn" not in k})
    att = att.to(device)
    x = t(fx["s128.x"]).to(device).requires_grad_(True)
    out = att(x, T, compute_dtype=torch.float32)
    (out * t(fx["s128.cot"]).to(device)).sum().backward()
    check(att, fx, "c128h4", out, x.grad)


@pytest.mark.parametrize("tag", BLOCKS)
def test_oracle_reproduces_the_reference_block(golden, tag):
    """oracle.maed_ref (what the bf16 tests differentiate in fp64) is the reference's arithmetic at these head sizes too"""
    fx = golden("g18_head_sizes")
    stag = str(fx[tag + ".state"])
    p = {k: v.double() for k, v in decode_state(fx, stag + ".").items()}
    x = t(fx[stag + ".x"]).double().requires_grad_(True)
    y = R.block(x, p, "", int(fx[tag + ".heads"]), int(fx["seqlen"]))
    (y * t(fx[stag + ".cot"]).double()).sum().backward()
    assert rel(y, fx[tag + ".out"]) < 2e-5 and rel(x.grad, fx[tag + ".dx"]) < 1e-4


@pytest.mark.parametrize("tag", BLOCKS)
def test_fused_block_f32_matches_reference_hostsim(golden, tag):
    with patched():
        run_block(golden("g18_head_sizes"), tag, "cpu")


def test_coupling_attention_f32_matches_reference_hostsim(golden):
    with patched():
        run_coupling(golden("g18_head_sizes"), "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("tag", BLOCKS)
def test_fused_block_f32_matches_reference_gpu(golden, tag):
    run_block(golden("g18_head_sizes"), tag, "cuda")


@pytest.mark.gpu
def test_coupling_attention_f32_matches_reference_gpu(golden):
    run_coupling(golden("g18_head_sizes"), "cuda")
