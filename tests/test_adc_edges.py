"""Adaptive density control (csrc/densify.hip: adc_classify_kernel, the three scan kernels, adc_scatter_kernel; fgs_adc_plan_thresholds / fgs_adc_apply;
Backend.adaptive_density_control) on the CPU simulation against the numpy restatement of the reference's Model.py:312-366, at thresholds, on non-finite
inputs, at the scan's edges and under saturated and empty plans. Cases, bars and checks: tests/adc_cases.py; on hardware: tests/test_gpu_adc_edges.py.

The restatement's own semantics are pinned first (test_restatement_masks_equal_torch): torch compares a float32 tensor with a Python double in float32,
and its row-wise max returns a NaN component.

Out of scope: the second trip of adc_scan_blocks_kernel's outer loop (more than 16 Ki block sums = 67 M Gaussians). The step across the waves of that
kernel (more than 1024 block sums = 4.2 M Gaussians) runs on hardware only: the simulation takes 13 s for it."""
import math

import numpy as np
import pytest
import torch

import helpers  # noqa: F401  (sets up import paths)
import adc_cases as cases


@pytest.mark.parametrize('name', cases.PINNED_CASES, ids=cases.case_id)
def test_restatement_masks_equal_torch(oracle, name):
    """oracle.adc_masks, which oracle.adaptive_density_control applies, against the same four expressions in torch on float32 CPU tensors with Python-double
    scalars, on the inputs that sit on a threshold or are not finite."""
    c = cases.case(name)
    with np.errstate(all='ignore'):
        ours = oracle.adc_masks(c.info.numpy(), c.P['opacities'].numpy(), c.P['scales'].numpy(), c.P['rotations'].numpy(), c.grad_threshold, c.min_opacity,
                                c.percent_dense, c.extent)
    theirs = cases.torch_masks(c)
    assert set(ours) == set(theirs) == {'densify', 'small', 'dead', 'too_large'}
    for k, mask in theirs.items():
        assert mask.dtype == torch.bool and np.array_equal(ours[k], mask.numpy()), (name, k)


def test_torch_compares_in_float32_and_its_max_returns_nan():
    """The two facts the restatement rests on, on their own: a float32 tensor at f32(x) compares as EQUAL to the double x although f32(x) != x, on either
    side of it; torch.max(dim=1) and Tensor.max(dim=1) return a NaN component wherever it sits."""
    x = math.log(0.01 * 3.925284601749901)
    candidates = (x, math.log(0.1 * 11.058493794857288), 0.1, 0.7)               # f32(0.1) > 0.1, f32(0.7) < 0.7
    up = [v for v in candidates if float(np.float32(v)) > v][0]
    down = [v for v in candidates if float(np.float32(v)) < v][0]
    for v in (up, down):
        t = torch.tensor([float(np.float32(v))], dtype=torch.float32)
        assert t.item() != v and bool(t <= v) and bool(t >= v) and not bool(t < v) and not bool(t > v)
    rows = torch.tensor([[float('nan'), 1.0, 2.0], [1.0, float('nan'), 2.0], [1.0, 2.0, float('nan')], [1.0, 3.0, 2.0]])
    for values in (torch.max(rows, dim=1).values, rows.max(dim=1).values):
        assert torch.isnan(values[:3]).all() and float(values[3]) == 3.0
    assert np.isnan(rows.numpy().max(axis=1)[:3]).all()


def test_reference_min_opacities_round_differently_from_their_float32():
    """REFERENCE_MIN_OPACITIES: f32(log(p / (1 - p))) differs between the double p and f32(p) (98 of the 999 values k / 10000 below 0.1 do);
    0.005, 0.01 and 0.05 round alike."""
    logit = lambda p: np.float32(math.log(p / (1 - p)))
    for p in cases.REFERENCE_MIN_OPACITIES:
        assert p < 0.1 and logit(p) != logit(float(np.float32(p))), p
    for p in (0.005, 0.01, 0.05):
        assert logit(p) == logit(float(np.float32(p))), p


@pytest.mark.parametrize('name', cases.THRESHOLD_CASES, ids=cases.case_id)
def test_thresholds_and_interactions(sim_backend, oracle, name):
    cases.check_case(sim_backend, oracle, 'cpu', name)


@pytest.mark.parametrize('name', cases.REFERENCE_THRESHOLD_CASES, ids=cases.case_id)
def test_thresholds_are_the_references(sim_backend, oracle, name):
    """percent_dense = 0.01, extents and min_opacity that float32 cannot carry: the device applies f32(log(pd * extent)), f32(log(0.1 * extent)) and
    f32(log(p / (1 - p))) formed from the doubles. (Through fgs_adc_plan's float arguments 4 of these 23 log_small and 13 of the log_large are one ulp off.)"""
    cases.check_case(sim_backend, oracle, 'cpu', name)


@pytest.mark.parametrize('name', cases.NONFINITE_CASES, ids=cases.case_id)
def test_nonfinite_inputs_are_not_sanitised(sim_backend, oracle, name):
    cases.check_case(sim_backend, oracle, 'cpu', name)


@pytest.mark.parametrize('name', cases.MIXED_CASES, ids=cases.case_id)
def test_row_counts_with_a_mixed_plan(sim_backend, oracle, name):
    cases.check_case(sim_backend, oracle, 'cpu', name)


@pytest.mark.parametrize('name', cases.PLAN_CASES, ids=cases.case_id)
def test_saturated_and_empty_plans(sim_backend, oracle, name):
    cases.check_case(sim_backend, oracle, 'cpu', name)


def test_block_scan_beyond_one_thread(sim_backend, oracle):
    """17 * 4096 + 5 Gaussians: 18 block sums, so the second thread of adc_scan_blocks_kernel adds the first one's total, in all four channels."""
    counts = cases.check_case(sim_backend, oracle, 'cpu', cases.TWO_THREADS_CASE)
    assert min(counts) > 4096


@pytest.mark.parametrize('name', cases.THRESHOLD_CASES + cases.NONFINITE_CASES + cases.REFERENCE_THRESHOLD_CASES[:3] + (('mixed', 17, True, True), ('mixed', 4097, True, True, 15),
                                                                                                                       ('plan', 'all_split', 4096), ('plan', 'all_pruned', 4097)),
                         ids=cases.case_id)
def test_product_flavour(sim_product_backend, oracle, name):
    """The same sources without the dev switches (the host paths of libfgs_hip.so), against the references the tests above computed."""
    cases.check_case(sim_product_backend, oracle, 'cpu', name)


def test_harness_survives_pruning_everything(sim_backend):
    cases.check_harness_prunes_everything(sim_backend, 'cpu')


def test_plan_entry_with_float_arguments_keeps_its_thresholds(sim_backend, oracle):
    """fgs_adc_plan stays for callers that hold float32 scalars: it forms the thresholds from float(percent_dense) and float(extent) in double. With scalars
    that float32 carries it plans what fgs_adc_plan_thresholds plans."""
    import ctypes as C
    _, _backend = helpers.backend_modules()
    be, c = sim_backend, cases.case('interactions')
    counts = (C.c_int32 * 4)()
    scratch = torch.empty(max(int(be.lib.fgs_adc_scratch_bytes(c.n)), 1), dtype=torch.uint8)
    be._check(be.lib.fgs_adc_plan(_backend._ptr(c.info), _backend._ptr(c.P['scales']), _backend._ptr(c.P['rotations']), _backend._ptr(c.P['opacities']), c.n,
                                  c.grad_threshold, c.min_opacity, 1, c.percent_dense, c.extent, scratch.data_ptr(), counts, 0), 'fgs_adc_plan')
    assert tuple(counts) == cases.reference(oracle, 'interactions')[3] == c.expect
    assert be.lib.fgs_adc_plan_thresholds(_backend._ptr(c.info), _backend._ptr(c.P['scales']), _backend._ptr(c.P['rotations']), _backend._ptr(c.P['opacities']), c.n,
                                          c.grad_threshold, float('nan'), 1, -3.0, -1.0, scratch.data_ptr(), counts, 0) == -1
    assert b'NaN' in be.lib.fgs_last_error()
