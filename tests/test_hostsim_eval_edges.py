"""Evaluation kernels (csrc/eval_metrics.hip through maed_amd/eval_utils.py and Evaluator.evaluate) against fp64 statements of the operations at the edges of
the kernels' geometry -- partial workgroups, J from 1 to 64 lanes, J and V past one stride -- and on rank-deficient point sets, on the host simulator.  Cases,
references and checks are tests/_eval_cases.py's; tests/test_gpu_eval.py runs the same table on the GPU."""
import pytest

import _eval_cases as EC
from _hostsim import patched


def _id(c):
    return "-".join(str(x) for x in c)


@pytest.mark.parametrize("case", EC.SIM_CASES, ids=_id)
def test_similarity_transform_vs_fp64(case):
    """Aligned points where the optimum is unique: max|got - ref| / max|ref| measured 5.910e-8 on the host simulator and 5.910e-8 on the MI355X (the floor is
    half an fp32 ulp of the largest coordinate, 2^-24 = 5.96e-8); bound EC.ALIGNED_REL = 8 x the larger = 4.73e-7, cap 1e-5.  Residual against the closed-form
    optimum: |res - opt| / var2 measured 8.05e-8 on the simulator and 7.34e-8 on the MI355X; bound 1e-5.  Before procrustes_rotation completed the basis of a
    rank-1 K the axis_s2 cases missed the residual bound by up to 6.3 % of var2."""
    with patched():
        EC.run_sim_case(*case)


@pytest.mark.parametrize("case", EC.POSE_CASES, ids=_id)
def test_pose_errors_vs_fp64(case):
    with patched():
        EC.run_pose_case(*case)


@pytest.mark.parametrize("case", EC.ACCEL_CASES, ids=_id)
def test_acceleration_vs_fp64(case):
    with patched():
        EC.run_accel_case(*case)


@pytest.mark.parametrize("case", EC.VERTEX_CASES, ids=_id)
def test_vertex_error_vs_fp64(case):
    with patched():
        EC.run_vertex_case(*case)


def test_outputs_stay_inside_their_windows():
    with patched():
        EC.run_guarded_calls()


def test_bad_arguments_return_their_status_and_launch_nothing():
    with patched():
        EC.run_argument_checks()


def test_target_vertices_chunking_is_bit_exact():
    with patched():
        EC.run_target_vertices_chunks()


def test_evaluator_means_vs_fp64():
    with patched():
        EC.run_evaluator()


def test_measured_maxima():
    """the figures the bounds of tests/_eval_cases.py were derived from, over the cases this process ran before this test (pytest -s shows them)"""
    print(f"aligned points: max rel err {EC.MEASURED['aligned']:.3e} (bound {EC.ALIGNED_REL:.3e}); residual: max |res-opt|/var2 {EC.MEASURED['residual']:.3e} "
          f"(bound {EC.RESIDUAL_REL:.0e})")
    assert EC.MEASURED["aligned"] <= EC.ALIGNED_REL and EC.MEASURED["residual"] <= EC.RESIDUAL_REL
