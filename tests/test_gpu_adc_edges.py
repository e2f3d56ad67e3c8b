"""GPU tests (-m gpu): adaptive density control (csrc/densify.hip) on the MI355X against the numpy restatement of the reference's Model.py:312-366 at
thresholds, on non-finite inputs, at the scan's edges and under saturated and empty plans -- the cases, bars and checks that tests/test_adc_edges.py runs on
the CPU simulation (tests/adc_cases.py), where the packed 16-bit DPP scan and the 1024-thread block scan are emulations. One case more than there: 4 198 405
Gaussians, whose 1026 block sums reach the second wave of adc_scan_blocks_kernel.

Out of scope: the second trip of that kernel's outer loop (more than 16 Ki block sums = 67 M Gaussians)."""
import pytest

import adc_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('name', cases.THRESHOLD_CASES, ids=cases.case_id)
def test_gpu_thresholds_and_interactions(hip_backend, oracle, name):
    cases.check_case(hip_backend, oracle, DEV, name)


@pytest.mark.parametrize('name', cases.REFERENCE_THRESHOLD_CASES, ids=cases.case_id)
def test_gpu_thresholds_are_the_references(hip_backend, oracle, name):
    cases.check_case(hip_backend, oracle, DEV, name)


@pytest.mark.parametrize('name', cases.NONFINITE_CASES, ids=cases.case_id)
def test_gpu_nonfinite_inputs_are_not_sanitised(hip_backend, oracle, name):
    cases.check_case(hip_backend, oracle, DEV, name)


@pytest.mark.parametrize('name', cases.MIXED_CASES, ids=cases.case_id)
def test_gpu_row_counts_with_a_mixed_plan(hip_backend, oracle, name):
    cases.check_case(hip_backend, oracle, DEV, name)


@pytest.mark.parametrize('name', cases.PLAN_CASES, ids=cases.case_id)
def test_gpu_saturated_and_empty_plans(hip_backend, oracle, name):
    cases.check_case(hip_backend, oracle, DEV, name)


def test_gpu_block_scan_beyond_one_thread(hip_backend, oracle):
    counts = cases.check_case(hip_backend, oracle, DEV, cases.TWO_THREADS_CASE)
    assert min(counts) > 4096


def test_gpu_block_scan_beyond_one_wave(hip_backend, oracle):
    """1024 * 4096 + 4096 + 5 Gaussians: 1026 block sums, sixteen per thread, so the first wave of adc_scan_blocks_kernel holds 1024 of them and the first thread
    of the SECOND wave the last two: every channel's prefix crosses the wave boundary through the LDS totals. Seeded mixed plan, no SH-rest bases, no moments; the time is the numpy restatement's."""
    counts = cases.check_case(hip_backend, oracle, DEV, cases.SECOND_WAVE_CASE)
    assert min(counts) > 64 * 4096


def test_gpu_harness_survives_pruning_everything(hip_backend):
    cases.check_harness_prunes_everything(hip_backend, DEV)
