"""Dropout / stochastic depth of the STE blocks with the kernels on the host simulator: the cases of tests/_ste_drop_cases.py on the CPU (the GPU runs the same
bodies in tests/test_gpu_ste_drop.py).  Masked GEMM epilogues and maed_drop_scale_cast against the numpy mask definition, the fused and the staged regularised
block against the fp64 masked oracle, identity / determinism, distribution, constructor plumbing."""
import pytest
import torch

import _ste_drop_cases as S
from _hostsim import patched

DEV = "cpu"


@pytest.mark.parametrize("epilogue", ["RESID_DROP_F32", "GELU_DROP", "MUL_DGELU_DROP"])
@pytest.mark.parametrize("shape", S.EPI_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kernel", list(S.IMPLS))
def test_masked_epilogues(kernel, shape, epilogue):
    with patched():
        S.run_epilogue_case(DEV, kernel, shape, epilogue, log=print)


@pytest.mark.parametrize("dtype", [S.F32, S.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,N,P", [(30, 128, 5), (4 * 197, 256, 197), (30, 100, 5)])
def test_drop_scale_cast(dtype, rows, N, P):
    with patched():
        S.run_scale_cast_case(DEV, dtype, rows, N, P)


@pytest.mark.parametrize("rates", [(0.5, 0.0), (0.0, 0.25), (0.3, 0.1)], ids=["path", "drop", "both"])
@pytest.mark.parametrize("dtype", [S.F32, S.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("dims", [(6, 5, 128, 2, 3)], ids=["F6P5C128"])      # ((4, 197, 256, 4, 2) takes 50 s per case on the simulator: GPU only)
def test_fused_block_vs_masked_oracle(dims, dtype, rates):
    with patched():
        S.run_block_case(DEV, dims, dtype, rates, report=S.log_report)


@pytest.mark.parametrize("dtype", [S.F32, S.BF16], ids=["f32", "bf16"])
def test_fused_block_exact_path_vs_masked_oracle(dtype):
    """impl = MAED_IMPL_VALU: the backward on transposed copies, where the mask goes before maed_transpose_cast"""
    with patched():
        S.run_block_case(DEV, (6, 5, 128, 2, 3), dtype, (0.3, 0.1), impl=1, report=S.log_report)


@pytest.mark.parametrize("mode", ["series", "vanilla", "temporal", "coupling"])
def test_staged_block_vs_masked_oracle(mode):
    with patched():
        S.run_block_case(DEV, (6, 5, 128, 2, 3), S.F32, (0.3, 0.1), mode=mode, report=S.log_report)


@pytest.mark.parametrize("dtype", [S.F32, S.BF16], ids=["f32", "bf16"])
def test_rate_zero_eval_and_no_grad_are_the_identity(dtype):
    with patched():
        S.run_identity_case(DEV, dtype)


@pytest.mark.parametrize("dtype,mode", [(S.F32, "parallel"), (S.BF16, "parallel"), (S.F32, "series")], ids=["f32", "bf16", "staged"])
def test_pinned_seed_is_deterministic_and_other_seeds_differ(dtype, mode):
    with patched():
        S.run_determinism_case(DEV, dtype, mode)


def test_distribution_of_the_sites():
    with patched():
        S.run_distribution_case(DEV)


def test_pos_drop_distribution_and_scale():
    with patched():
        S.run_pos_drop_case(DEV)


def test_vit_gives_the_blocks_the_linspace_of_drop_path_rates():
    from maed_amd.resnetv2 import ResNetV2
    from maed_amd.vision_transformer import DropPath, VisionTransformer
    bb = ResNetV2(layers=(1, 1, 1), channels=(128, 256, 512), compute_dtype=torch.float32)
    vit = VisionTransformer(img_size=32, embed_dim=128, depth=3, num_heads=2, hybrid_backbone=bb, st_mode="parallel", num_classes=-1, drop_path_rate=0.2,
                            compute_dtype=torch.float32)
    assert [round(b.drop_path_prob, 6) for b in vit.blocks] == [0.0, 0.1, 0.2]
    assert isinstance(vit.blocks[0].drop_path, torch.nn.Identity) and isinstance(vit.blocks[2].drop_path, DropPath)
    assert abs(vit.blocks[2].drop_path.drop_prob - 0.2) < 1e-6 and all(b.drop == 0.0 for b in vit.blocks) and vit.pos_drop.p == 0.0


def test_maed_forwards_the_rates_and_still_rejects_attention_dropout_and_qk_scale():
    from maed_amd.vision_transformer import Attention, Block
    m = S.small_maed(DEV, drop_path_rate=0.1, drop_rate=0.1)
    assert m.encoder.pos_drop.p == 0.1 and m.encoder.blocks[0].drop == 0.1 and m.encoder.blocks[0].mlp.drop.p == 0.1 and m.encoder.blocks[0].attn.proj_drop.p == 0.1
    ref = S.small_maed(DEV)
    assert list(m.state_dict()) == list(ref.state_dict())
    with pytest.raises(NotImplementedError, match="attn_drop"):
        S.small_maed(DEV, attn_drop_rate=0.1)
    with pytest.raises(NotImplementedError, match="attn_drop"):
        Block(128, 2, attn_drop=0.1, st_mode="parallel")
    with pytest.raises(NotImplementedError, match="qk_scale"):
        Block(128, 2, qk_scale=0.1, st_mode="parallel")
    with pytest.raises(NotImplementedError, match="qk_scale"):
        Attention(128, num_heads=2, qk_scale=0.1, st_mode="parallel")
    with pytest.raises(ValueError):
        Block(128, 2, drop_path=1.0, st_mode="parallel")


def test_regularised_maed_runs_a_training_step():
    with patched(module_paths=False):      # the backbone on ATen: this test is about the encoder's regularisers (the GPU test runs the whole library path)
        S.run_train_step_case(DEV)


def test_rate_zero_encoder_consumes_no_call_ids():
    """the blocks and pos_drop of a rate-0 encoder draw no call id from the device record (the decoder's two Dropout layers stay calls 1 and 2: the GPU test
    counts them on the whole model); with rates, pos_drop and every regularised block draw one each"""
    from maed_amd import ops
    st = ops.DeviceTrainState(torch.device("cpu"))
    st.begin_step(seed=7)
    st.upload()
    old, ops.DEVICE_STATE = ops.DEVICE_STATE, st
    img = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(9))
    try:
        with patched(module_paths=False):      # (backbone on ATen: this test is about the encoder's blocks)
            S.small_maed(DEV).train().encoder(img, seqlen=2)
            assert st.calls == 0, st.calls
            S.small_maed(DEV, drop_rate=0.1).train().encoder(img, seqlen=2)
            assert st.calls == 2, st.calls      # pos_drop + the one block
    finally:
        ops.DEVICE_STATE = old


def test_stand_alone_mlp_and_drop_path_modules():
    """Mlp(drop=) and DropPath called on their own (outside a Block): training mode masks through the library, eval is the identity"""
    from maed_amd.vision_transformer import DropPath, Mlp
    torch.manual_seed(3)
    x = (torch.randn(40, 5, 128).abs() + 1.0).requires_grad_(True)
    with patched():
        dp = DropPath(0.5).train()
        y = dp(x)
        frames = (y.reshape(40, -1) != 0).any(dim=1)
        assert 0 < int(frames.sum()) < 40 and torch.equal(y[frames], (x * 2.0)[frames]) and not y[~frames].any()
        y.sum().backward()
        assert torch.equal(x.grad[frames], torch.full_like(x.grad[frames], 2.0)) and not x.grad[~frames].any()
        assert dp.eval()(x) is x
        mlp = Mlp(128, 256, drop=0.25).train()
        out = mlp(x.detach().requires_grad_(True))
        frac = float((out == 0).float().mean())
        assert abs(frac - 0.25) < 5 * (0.25 * 0.75 / out.numel()) ** 0.5, frac      # site 4: a quarter of the outputs are zero
        out.sum().backward()
        assert all(torch.isfinite(q.grad).all() for q in mlp.parameters())
        with torch.no_grad():
            a, b = mlp.eval()(x), Mlp.forward(mlp, x)
        assert torch.equal(a, b) and not (a == 0).any()
