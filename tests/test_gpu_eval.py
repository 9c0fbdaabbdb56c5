"""Evaluation kernels on the GPU (csrc/eval_metrics.hip through maed_amd/eval_utils.py and Evaluator.evaluate): the cases, fp64 references and checks of
tests/_eval_cases.py -- the table tests/test_hostsim_eval_edges.py runs on the host simulator -- on device tensors through the product library.  Every measured
error goes into the parity report."""
import pytest
import torch

from maed_amd import _lib as L
from maed_amd import eval_utils as EU

import _eval_cases as EC
from _util import DEV, note, report

pytestmark = pytest.mark.gpu


def _id(c):
    return "-".join(str(x) for x in c)


@pytest.mark.parametrize("case", EC.SIM_CASES, ids=_id)
def test_similarity_transform_vs_fp64(case):
    """Aligned points where the optimum is unique: max|got - ref| / max|ref| measured 5.910e-8 on the host simulator and 5.910e-8 on the MI355X (the floor is
    half an fp32 ulp of the largest coordinate, 2^-24 = 5.96e-8); bound EC.ALIGNED_REL = 8 x the larger = 4.73e-7, cap 1e-5.  Residual against the closed-form
    optimum: |res - opt| / var2 measured 8.05e-8 on the simulator and 7.34e-8 on the MI355X; bound 1e-5."""
    EC.run_sim_case(*case, device=DEV, note=note)


@pytest.mark.parametrize("case", EC.POSE_CASES, ids=_id)
def test_pose_errors_vs_fp64(case):
    EC.run_pose_case(*case, device=DEV, close=report, note=note)


@pytest.mark.parametrize("case", EC.ACCEL_CASES, ids=_id)
def test_acceleration_vs_fp64(case):
    EC.run_accel_case(*case, device=DEV, close=report)


@pytest.mark.parametrize("case", EC.VERTEX_CASES, ids=_id)
def test_vertex_error_vs_fp64(case):
    EC.run_vertex_case(*case, device=DEV, close=report)


def test_outputs_stay_inside_their_windows():
    EC.run_guarded_calls(device=DEV, close=report)


def test_bad_arguments_return_their_status_and_launch_nothing():
    EC.run_argument_checks(device=DEV)


def test_target_vertices_chunking_is_bit_exact():
    EC.run_target_vertices_chunks(device=DEV)


def test_evaluator_means_vs_fp64():
    EC.run_evaluator(device=DEV, close=report)


def test_launches_are_ordered_on_the_current_stream():
    """inputs produced on a side stream behind a matrix product that is still running when the wrappers are called, result consumed on that stream: a launch on
    any other stream would read the inputs before they exist"""
    kind, vis, N, J = "generic", "6", 9, 17
    pred, tgt = EC.pose_inputs(kind, vis, N, J)
    ref = EC.pose_reference(kind, vis, N, J)
    pred_h, tgt_h = pred.pin_memory(), tgt.pin_memory()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        busy = torch.ones(4096, 4096, device=DEV)
        for _ in range(4):
            busy = (busy @ busy) * 0.0 + 1.0
        zero = (busy.sum() - 4096.0 * 4096.0)                               # 0, known only once the products are done
        p_d = torch.full((N, J, 3), float("nan"), device=DEV).copy_(pred_h, non_blocking=True) + zero
        t_d = torch.full((N, J, 4), float("nan"), device=DEV).copy_(tgt_h, non_blocking=True) + zero
        mpjpe, pa, pred_c, tgt_c = EU.pose_errors(p_d, t_d)
        hat = EU.batch_compute_similarity_transform_torch(pred_c, tgt_c)   # consumes the first launch's outputs on the same stream
        got = [x.to("cpu", non_blocking=True) for x in (mpjpe, pa, pred_c, tgt_c, hat)]
        side.synchronize()
    report("side stream pose_errors mpjpe", got[0], ref["mpjpe"], **EC.SCALAR)
    report("side stream pose_errors pa_mpjpe", got[1], ref["pa"], **EC.SCALAR)
    EC.check_similarity(got[4], EC.similarity_ref(got[2], got[3]), "side stream similarity of the centred sets", note)
    torch.cuda.synchronize()


def test_measured_maxima_and_no_device_faults():
    """the figures the bounds of tests/_eval_cases.py were derived from, over the cases this process ran, into the parity report; and the library saw no fault"""
    note(f"eval kernels vs fp64: aligned points max rel err {EC.MEASURED['aligned']:.3e} (bound {EC.ALIGNED_REL:.3e}); residual max |res-opt|/var2 "
         f"{EC.MEASURED['residual']:.3e} (bound {EC.RESIDUAL_REL:.0e})")
    assert EC.MEASURED["aligned"] <= EC.ALIGNED_REL and EC.MEASURED["residual"] <= EC.RESIDUAL_REL
    torch.cuda.synchronize()
    assert L.device_faults() == 0
