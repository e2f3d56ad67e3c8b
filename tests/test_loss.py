"""Fused L1 + DSSIM loss. The reference's `fused_dssim` lives in the un-vendored NeRFICG framework,
so parity is defined against the published SSIM (3DGS convention): the oracle restatement is pinned by an independent
torch conv2d + autograd implementation, the HIP kernels (simulation here, hardware under -m gpu) by the oracle -- and, three-way, by that fp64 model
itself at the shapes, contents and call forms of tests/loss_cases.py (the same cases run on the MI355X in tests/test_gpu_loss.py)."""
import numpy as np
import pytest
import torch

import helpers
import loss_cases as cases


_pair = cases.noise_pair


def _torch_reference(x, y, l1=0.8, ds=0.2):
    loss, _, ssim, grad = cases.truth(x, y, l1, ds)          # the fp64 conv2d + autograd model: tests/loss_cases.py
    return loss, ssim, grad


@pytest.mark.parametrize('h,w', [(37, 53), (16, 32), (5, 7)])
def test_oracle_loss_matches_torch_conv2d_autograd(oracle, h, w):
    x, y = _pair(h, w)
    loss, l1, ssim, grad = oracle.l1_dssim(x, y)
    rl, rs, rg = _torch_reference(x, y)
    assert abs(loss - rl) < 1e-6 and abs(ssim - rs) < 1e-6
    assert helpers.rel_inf(grad, rg) < 1e-5
    assert oracle.l1_dssim(x, x)[2] == pytest.approx(1.0, abs=1e-6)          # SSIM(x, x) = 1


@pytest.mark.parametrize('h,w', [(37, 53), (48, 64), (5, 7)])
def test_sim_loss_kernels_match_oracle(sim_backend, oracle, h, w):
    x, y = _pair(h, w, seed=3)
    loss, grad, means = sim_backend.l1_dssim(torch.from_numpy(x), torch.from_numpy(y))
    ol, o_l1, o_ssim, og = oracle.l1_dssim(x, y)
    assert abs(float(loss) - ol) < 1e-6 and abs(float(means[0]) - o_l1) < 1e-6 and abs(float(means[1]) - o_ssim) < 1e-6
    assert helpers.rel_inf(grad.numpy(), og) < 1e-5
    loss2, none, _ = sim_backend.l1_dssim(torch.from_numpy(x), torch.from_numpy(y), with_grad=False)
    assert none is None and abs(float(loss2) - ol) < 1e-6
    # the autograd shape: forward keeps the derivative maps, backward alone produces dloss/dimage * upstream (a device scalar)
    loss3, means3, scratch = sim_backend.l1_dssim_forward(torch.from_numpy(x), torch.from_numpy(y))
    assert float(loss3) == float(loss) and torch.equal(means3, means)
    g1 = sim_backend.l1_dssim_backward(torch.from_numpy(x), torch.from_numpy(y), scratch)
    assert torch.equal(g1, grad)                                                   # upstream None = 1: the same kernel, bit for bit
    g2 = sim_backend.l1_dssim_backward(torch.from_numpy(x), torch.from_numpy(y), scratch, torch.tensor(-0.37))
    assert helpers.rel_inf(g2.numpy(), -0.37 * og) < 1e-5
    with pytest.raises(RuntimeError):
        sim_backend.l1_dssim_backward(torch.from_numpy(x), torch.from_numpy(y), scratch[:16])


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', [(37, 53), (360, 640), (1080, 1920)])
def test_gpu_loss_matches_oracle(hip_backend, oracle, h, w):
    from harness.loss import l1_dssim_loss
    x, y = _pair(h, w, seed=5)
    tx = torch.from_numpy(x).cuda().requires_grad_(True)
    loss = l1_dssim_loss(tx, torch.from_numpy(y).cuda())
    (2.0 * loss).backward()
    ol, _, _, og = oracle.l1_dssim(x, y)
    assert abs(float(loss) - ol) < 2e-6
    assert helpers.rel_inf(tx.grad.cpu().numpy(), 2.0 * og) < 1e-4      # fp32 tolerance of BASELINE.json


# ---- the kernels (simulated) against the fp64 model, three-way with the fp32 oracle: tests/loss_cases.py -----------------------------------------------
@pytest.mark.parametrize('shape', cases.SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_sim_loss_one_call_matches_fp64_at_tile_edges(sim_backend, oracle, shape):
    """be.l1_dssim(with_grad=True) -- the entry point of the benchmark and the multi-GPU trainers: workgroup 0 of the backward kernel reduces the forward
    partials -- at every shape of the edge table."""
    cases.check_against_truth(sim_backend, oracle, 'cpu', shape, 'noise', 'one_call')


@pytest.mark.parametrize('shape', cases.FORM_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_sim_loss_three_forms_agree_bit_for_bit(sim_backend, oracle, shape):
    cases.check_forms_agree(sim_backend, oracle, 'cpu', shape)


@pytest.mark.parametrize('shape', cases.CONTENT_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('content', cases.CONTENTS)
def test_sim_loss_contents_match_fp64(sim_backend, oracle, content, shape):
    cases.check_against_truth(sim_backend, oracle, 'cpu', shape, content, 'one_call')


@pytest.mark.parametrize('lambdas', [(0.35, 1.7), (1.0, 0.0), (0.0, 1.0)], ids=lambda l: f'{l[0]}-{l[1]}')
def test_sim_loss_lambdas(sim_backend, oracle, lambdas):
    cases.check_against_truth(sim_backend, oracle, 'cpu', (33, 65), 'noise', 'one_call', lambdas)


def test_sim_loss_upstream_scalars(sim_backend, oracle):
    """-0.37 handed to the backward kernel as a scalar; 3 arriving from a composite autograd graph; -0.37 through autograd."""
    cases.check_against_truth(sim_backend, oracle, 'cpu', (33, 65), 'noise', 'split', upstream=-0.37)
    cases.check_against_truth(sim_backend, oracle, 'cpu', (33, 65), 'noise', 'autograd', upstream=-0.37)
    cases.check_composite_graph(sim_backend, oracle, 'cpu', (33, 65))


def test_sim_loss_non_contiguous_image(sim_backend):
    cases.check_non_contiguous(sim_backend, 'cpu', (33, 65))


@pytest.mark.parametrize('shape', [(33, 65), (70, 100)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_sim_loss_does_not_read_scratch_it_did_not_write(sim_backend, shape):
    cases.check_scratch_independence(sim_backend, 'cpu', shape)


def test_sim_loss_is_reproducible(sim_backend):
    cases.check_reproducible(sim_backend, 'cpu', (70, 100))
