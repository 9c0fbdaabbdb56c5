"""Dropout / stochastic depth of the STE blocks on the device: the cases of tests/_ste_drop_cases.py (the simulator runs the same bodies in
tests/test_hostsim_ste_drop.py) plus what only a GPU shows -- the three store forms of the masked epilogues on the real kernels, the frames-straddle-tiles block
shape, and a captured training step that replays with fresh masks."""
import pytest
import torch

import _ste_drop_cases as S
from _util import DEV, note, report

pytestmark = pytest.mark.gpu


def _faults():
    from maed_amd import _lib as L
    return L.lib().maed_device_faults()


@pytest.mark.parametrize("epilogue", ["RESID_DROP_F32", "GELU_DROP", "MUL_DGELU_DROP"])
@pytest.mark.parametrize("shape", S.EPI_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kernel", list(S.IMPLS))
def test_masked_epilogues(kernel, shape, epilogue):
    S.run_epilogue_case(DEV, kernel, shape, epilogue, log=note)
    assert _faults() == 0


@pytest.mark.parametrize("dtype", [S.F32, S.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,N,P", [(30, 128, 5), (4 * 197, 256, 197), (30, 100, 5)])
def test_drop_scale_cast(dtype, rows, N, P):
    S.run_scale_cast_case(DEV, dtype, rows, N, P)


@pytest.mark.parametrize("rates", [(0.5, 0.0), (0.0, 0.25), (0.3, 0.1)], ids=["path", "drop", "both"])
@pytest.mark.parametrize("dtype", [S.F32, S.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("dims", [(6, 5, 128, 2, 3), (4, 197, 256, 4, 2)], ids=["F6P5C128", "F4P197C256"])
def test_fused_block_vs_masked_oracle(dims, dtype, rates):
    S.run_block_case(DEV, dims, dtype, rates, report=report)
    assert _faults() == 0


@pytest.mark.parametrize("dtype", [S.F32, S.BF16], ids=["f32", "bf16"])
def test_fused_block_exact_path_vs_masked_oracle(dtype):
    """impl = MAED_IMPL_VALU: the backward on transposed copies, where the mask goes before maed_transpose_cast"""
    S.run_block_case(DEV, (6, 5, 128, 2, 3), dtype, (0.3, 0.1), impl=1, report=report)


def test_fused_block_f32_split_matmul_mode_vs_masked_oracle():
    """fp32 with the process-wide split-bf16 matmul mode: the backward takes the row-major (no transposed copies) path with fp32 masked copies.  Bars: the exact
    mode's times 10 = the accurate mode's documented 1e-3 (operands carry 16 significand bits instead of 24; csrc/block.hip "north_star's 1e-3 on the outputs")"""
    from maed_amd import ops
    old = ops.get_float32_matmul_precision()
    ops.set_float32_matmul_precision("bf16x3")
    try:
        S.run_block_case(DEV, (6, 5, 128, 2, 3), S.F32, (0.3, 0.1), report=lambda name, got, ref, rtol, atol: report(name + "[bf16x3]", got, ref, rtol=10 * rtol, atol=10 * atol))
    finally:
        ops.set_float32_matmul_precision(old)


@pytest.mark.parametrize("mode", ["series", "vanilla", "temporal", "coupling"])
def test_staged_block_vs_masked_oracle(mode):
    S.run_block_case(DEV, (6, 5, 128, 2, 3), S.F32, (0.3, 0.1), mode=mode, report=report)


# Bitwise checks run in bf16 on the device.  In fp32 two runs of one UNCHANGED rate-0 block already differ in the last bits at these dims (products with few output
# tiles and a long K meet through fp32 atomics: csrc/gemm.hip "few output tiles, long K"), so fp32 bit-identity is checked where execution is deterministic: on the
# simulator (tests/test_hostsim_ste_drop.py, same bodies).
def test_rate_zero_eval_and_no_grad_are_the_identity():
    S.run_identity_case(DEV, S.BF16)


@pytest.mark.parametrize("mode", ["parallel", "series"])
def test_pinned_seed_is_deterministic_and_other_seeds_differ(mode):
    S.run_determinism_case(DEV, S.BF16, mode)


def test_distribution_of_the_sites():
    S.run_distribution_case(DEV)


def test_pos_drop_distribution_and_scale():
    S.run_pos_drop_case(DEV)


@pytest.mark.parametrize("dtype", [S.F32, S.BF16], ids=["f32", "bf16"])
def test_regularised_maed_runs_a_training_step(dtype):
    S.run_train_step_case(DEV, dtype)
    assert _faults() == 0


def test_twin_forward_is_not_taken_by_a_regularised_block():
    """set_float32_backward_precision('bf16'): a rate-0 block takes the twin forward, a regularised one runs on the forward's engine and says so once"""
    import warnings
    from maed_amd import ops
    old_p, old_b = ops.get_float32_matmul_precision(), ops.get_float32_backward_precision()
    ops.set_float32_matmul_precision("bf16x3")
    ops.set_float32_backward_precision("bf16")
    try:
        Fr, P, C, H, T = 6, 5, 128, 2, 3
        blk = S.make_block(C, H, S.F32, "parallel", DEV, 0.1, 0.3, state=S.block_params(C, P, "parallel")).train()
        blk.drop_seed = 5
        x = S.G.rnd(Fr, P, C, seed=1).to(DEV).requires_grad_(True)
        n = ops.TWIN_FORWARDS[0]
        ops._REG_TWIN_WARNED[0] = False
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            blk(x, T).sum().backward()
        assert ops.TWIN_FORWARDS[0] == n and any(issubclass(i.category, RuntimeWarning) and "twin" in str(i.message) for i in w)
        assert torch.isfinite(x.grad).all()
    finally:
        ops.set_float32_matmul_precision(old_p)
        ops.set_float32_backward_precision(old_b)


def _graph_setup(**rates):
    import maed_amd
    from maed_amd.ddp import FusedAdam, GradBucketer, ParamArena
    from maed_amd.loss import LossVideo
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = maed_amd.MAED(num_blocks=2, num_heads=2, embed_dim=128, hidden_dim=256, img_size=64, compute_dtype=torch.bfloat16, **rates).to(dev).train()
    arena = ParamArena(model)
    opt = FusedAdam(arena, lr=0.0, bucketer=GradBucketer(arena, model))      # lr = 0: the parameters stay put, the loss of a step depends on the masks alone
    clip = torch.randn(2, 4, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(dev)
    return model, arena, opt, LossVideo(), clip, S.train_targets(dev, 2, 4)


def test_graph_replays_draw_fresh_masks_and_the_same_record_gives_the_same_step():
    from maed_amd.graphed import GraphedTrainStep
    model, arena, opt, crit, clip, tgt = _graph_setup(drop_rate=0.1, drop_path_rate=0.2)
    step = GraphedTrainStep(model, crit, opt, clip, tgt, warmup=2)
    try:
        assert step.state.calls == 1 + 2 + 2, step.state.calls      # pos_drop, the two blocks, the decoder's two Dropout layers
        a = float(step().item())
        b = float(step().item())                                   # a new seed in the record, the same launches
        assert abs(a - b) > 1e-5 * abs(a), (a, b)

        def replay(seed):
            step._prepare(seed=seed)
            step.graph.replay()
            return float(step.loss.item())

        c, d, e = replay(1234), replay(99), replay(1234)
        assert abs(c - d) > 1e-5 * abs(c), (c, d)
        # the same record contents: the same masks (to the order of the fp32 atomics inside a step, as tests/test_gpu_graph.py)
        assert abs(c - e) <= 1e-6 * abs(c), (c, e)
        assert _faults() == 0
    finally:
        step.close()


def test_rate_zero_model_leaves_the_decoder_its_two_call_ids():
    from maed_amd.graphed import GraphedTrainStep
    model, arena, opt, crit, clip, tgt = _graph_setup()
    step = GraphedTrainStep(model, crit, opt, clip, tgt, eager=True)
    try:
        step()
        assert step.state.calls == 2, step.state.calls
    finally:
        step.close()
