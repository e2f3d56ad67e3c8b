"""The streaming L1 + DSSIM loss kernels (csrc/loss.hip) on the MI355X at the edges of their geometry, and against the tiled formulation of the dev
library (csrc/loss_exhibits.hip, option 16): the cases, references and bars of tests/loss_stream_cases.py. Each case is a few dozen launches of
microseconds and the fp64 model on the host."""
import pytest

import loss_stream_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('shape', cases.ALL_SHAPES, ids=cases.shape_id)
def test_gpu_loss_stream_edges(hip_backend, oracle, shape):
    cases.check_shape(hip_backend, oracle, DEV, shape)


@pytest.mark.parametrize('shape', cases.FORMULATION_SHAPES, ids=cases.shape_id)
def test_gpu_loss_streaming_equals_tiled(hip_dev_backend, oracle, shape):
    cases.check_streaming_against_tiled(hip_dev_backend, oracle, DEV, shape)


def test_gpu_loss_streaming_equals_tiled_smooth(hip_dev_backend, oracle):
    cases.check_streaming_against_tiled(hip_dev_backend, oracle, DEV, cases.FORMULATION_SHAPES[1], 'smooth_bright')

