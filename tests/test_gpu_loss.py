"""The fused L1 + DSSIM loss kernels (csrc/loss.hip) on the MI355X against the fp64 conv2d + autograd model, three-way with the fp32 oracle: the cases,
bars and checks of tests/loss_cases.py, which tests/test_loss.py runs on the CPU simulation. Each case is two or three launches of microseconds and the
fp64 model on the host. Measured figures: profiles/loss_tolerance_slack.txt (FGS_TOL_LOG)."""
import pytest

import loss_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_id = lambda s: f'{s[0]}x{s[1]}'


@pytest.mark.parametrize('shape', cases.SHAPES, ids=_id)
def test_gpu_loss_one_call_matches_fp64_at_tile_edges(hip_backend, oracle, shape):
    """be.l1_dssim(with_grad=True) -- the entry point of the benchmark and the multi-GPU trainers: workgroup 0 of the backward kernel reduces the forward
    partials -- at every shape of the edge table."""
    cases.check_against_truth(hip_backend, oracle, DEV, shape, 'noise', 'one_call')


@pytest.mark.parametrize('shape', cases.FORM_SHAPES, ids=_id)
def test_gpu_loss_three_forms_agree_bit_for_bit(hip_backend, oracle, shape):
    cases.check_forms_agree(hip_backend, oracle, DEV, shape)


@pytest.mark.parametrize('shape', cases.CONTENT_SHAPES, ids=_id)
@pytest.mark.parametrize('content', cases.CONTENTS)
def test_gpu_loss_contents_match_fp64(hip_backend, oracle, content, shape):
    cases.check_against_truth(hip_backend, oracle, DEV, shape, content, 'one_call')


@pytest.mark.parametrize('lambdas', [(0.35, 1.7), (1.0, 0.0), (0.0, 1.0)], ids=lambda l: f'{l[0]}-{l[1]}')
def test_gpu_loss_lambdas(hip_backend, oracle, lambdas):
    cases.check_against_truth(hip_backend, oracle, DEV, (33, 65), 'noise', 'one_call', lambdas)


def test_gpu_loss_upstream_scalars(hip_backend, oracle):
    """-0.37 handed to the backward kernel as a scalar; 3 arriving from a composite autograd graph; -0.37 through autograd."""
    cases.check_against_truth(hip_backend, oracle, DEV, (33, 65), 'noise', 'split', upstream=-0.37)
    cases.check_against_truth(hip_backend, oracle, DEV, (33, 65), 'noise', 'autograd', upstream=-0.37)
    cases.check_composite_graph(hip_backend, oracle, DEV, (33, 65))


def test_gpu_loss_non_contiguous_image(hip_backend):
    cases.check_non_contiguous(hip_backend, DEV, (33, 65))


@pytest.mark.parametrize('shape', [(33, 65), (70, 100)], ids=_id)
def test_gpu_loss_does_not_read_scratch_it_did_not_write(hip_backend, shape):
    cases.check_scratch_independence(hip_backend, DEV, shape)


@pytest.mark.parametrize('shape', [(70, 100), cases.LARGE], ids=_id)
def test_gpu_loss_is_reproducible(hip_backend, shape):
    cases.check_reproducible(hip_backend, DEV, shape)


@pytest.mark.parametrize('content', ['noise', 'smooth_bright'])
def test_gpu_loss_contents_at_size(hip_backend, oracle, content):
    """360 x 640: 720 forward partials, 360 backward workgroups -- content effects grow with the number of partials."""
    cases.check_against_truth(hip_backend, oracle, DEV, cases.LARGE, content, 'one_call')
