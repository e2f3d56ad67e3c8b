"""The streaming L1 + DSSIM loss kernels (csrc/loss.hip) on the CPU simulation at the edges of their geometry -- strips of 64 columns, bands of rows, the
11-row register ring, workgroups of four waves dealt to XCD regions -- and against the tiled formulation they replaced (csrc/loss_exhibits.hip, option 16):
the cases, references and bars of tests/loss_stream_cases.py, which tests/test_gpu_loss_stream.py runs on the MI355X."""
import pytest

import loss_stream_cases as cases


@pytest.mark.parametrize('shape', cases.ALL_SHAPES, ids=cases.shape_id)
def test_sim_loss_stream_edges(sim_backend, oracle, shape):
    cases.check_shape(sim_backend, oracle, 'cpu', shape)


@pytest.mark.parametrize('shape', cases.FORMULATION_SHAPES, ids=cases.shape_id)
def test_sim_loss_streaming_equals_tiled(sim_backend, oracle, shape):
    cases.check_streaming_against_tiled(sim_backend, oracle, 'cpu', shape)


def test_sim_loss_streaming_equals_tiled_smooth(sim_backend, oracle):
    """smooth_bright: s11 cancels against C2, the content on which a different rounding of one tap shows first."""
    cases.check_streaming_against_tiled(sim_backend, oracle, 'cpu', cases.FORMULATION_SHAPES[1], 'smooth_bright')


def test_product_flavour_gives_the_streaming_bits(sim_backend, sim_product_backend):
    """The product flavour (no FGS_DEV_SWITCHES, no exhibit unit) and the dev flavour at its default run the same kernels: loss, means and gradient bit for bit."""
    import torch
    x, y = cases.base.pair(cases.UNEVEN, 'noise')
    a, b = cases.base.run(sim_product_backend, 'cpu', x, y), cases.base.run(sim_backend, 'cpu', x, y)
    assert torch.equal(a['loss'], b['loss']) and torch.equal(a['means'], b['means']) and torch.equal(a['grad'], b['grad'])


def test_tiled_kernels_are_in_the_dev_library_only():
    """The product library holds one forward and one backward loss kernel: the names of the tiled kernels (registered with the HIP runtime as strings, so
    they are in the file's bytes) appear in libfgs_hip_dev.so and not in libfgs_hip.so; the streaming kernels' names appear in both."""
    import helpers
    _lib, _ = helpers.backend_modules()
    product = _lib.DEFAULT_LIBRARY.read_bytes()
    for name in (b'ssim_forward_kernel', b'ssim_backward_kernel'):
        assert name in product, name
    for name in (b'ssim_forward_tiled_kernel', b'ssim_backward_tiled_kernel'):
        assert name not in product, name
    if _lib.DEV_LIBRARY.exists():
        dev = _lib.DEV_LIBRARY.read_bytes()
        for name in (b'ssim_forward_kernel', b'ssim_backward_kernel', b'ssim_forward_tiled_kernel', b'ssim_backward_tiled_kernel'):
            assert name in dev, name
