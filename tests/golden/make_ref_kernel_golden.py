"""Writes tests/golden/ref_kernels_<scene>.npz: what the REFERENCE'S OWN kernels and host code compute, run on the CPU (oracle/build_ref.py builds
them against oracle/cuda_on_cpu; oracle/reference.py drives them). Build container only -- it needs the reference tree. Run from the repo root:

    python tests/golden/make_ref_kernel_golden.py

Per scene (tests/ref_pin_cases.py: CPU_FIXTURES): the inputs (all of them, sh_coefficients_rest included: the seeded generators go through torch's CPU
transcendentals, whose last bit differs between machines, so a fixture regenerated from its seed elsewhere is another scene), every intermediate of the forward, the image, the seed of grad_image, the six gradients,
densification_info, and the pruning scores accumulated on ref_pin_cases.score_base_of. Nothing here is computed by the oracle: the files hold data
the reference's programs wrote while they ran. Fields the reference leaves undefined are stored as zeros: records of Gaussians with n_touched == 0,
and bucket checkpoints a pixel did not store (`ckpt_written_bits` tells which it did). ref_kernels_mcmc.npz: the two MCMC kernels on one seeded case.
"""
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent.parent
sys.path[:0] = [str(REPO), str(REPO / 'faster-gaussian-splatting_amd'), str(REPO / 'tests')]
import helpers  # noqa: E402
import ref_pin_cases as cases  # noqa: E402
from oracle import reference as R  # noqa: E402

KEEP = ('V', 'I', 'B', 'selector', 'end_bit', 'n_touched', 'screen_bounds', 'mean2d', 'conic_opacity', 'color', 'depth_keys', 'prim_idx', 'offsets', 'inst_keys',
        'inst_prims', 'ranges', 'n_buckets', 'bucket_offsets', 'image', 'final_T', 'n_processed', 'max_n_processed', 'bucket_tile_index', 'bucket_ckpt')


def dump(name: str) -> None:
    params, view, K, aa = cases.scene(name)
    S, _ = helpers.settings_pair(view, K, aa)
    a = helpers.np_params(params)
    n = a[0].shape[0]
    out = {f'in_{k}': v for k, v in zip(helpers.NAMES, a)}
    out['settings'] = np.array([K, view.width, view.height, view.focal_x, view.focal_y, view.center_x, view.center_y, view.near_plane, view.far_plane,
                                float(aa)], np.float64)
    out['w2c'], out['cam_position'], out['bg_color'] = S.w2c, S.cam_position, S.bg_color
    r = R.forward(*a, S)
    gi = cases.grad_image_of(r['image'].shape)
    dens = np.zeros((2, n), np.float32)
    g = R.backward(r, S, gi, dens)
    vis = r['n_touched'] > 0
    for k in cases.RECORD_FIELDS + ('screen_bounds',):
        r[k] = np.where(vis[:, None], r[k], 0).astype(r[k].dtype)
    r['bucket_ckpt'] = np.where(r['ckpt_written'][:, :, None], r['bucket_ckpt'], 0).astype(np.float32)
    out.update({k: np.asarray(r[k]) for k in KEEP})
    out['ckpt_written_bits'] = np.packbits(r['ckpt_written'].reshape(-1))
    out['grad_seed'] = np.int64(cases.GRAD_SEED)
    out.update({f'grad_{k}': g[k] for k in helpers.GRAD_KEYS})
    out['densification_info'] = dens
    scores = cases.score_base_of(n)
    R.pruning_scores(scores, *a, S)
    out['pruning_scores'] = scores
    path = cases.fixture_path(name)
    np.savez_compressed(path, **out)
    print(path.name, {k: int(out[k]) for k in ('V', 'I', 'B')}, f'{path.stat().st_size / 1e6:.2f} MB')


def dump_mcmc() -> None:
    """ref_kernels_mcmc.npz: the inputs of ref_pin_cases.mcmc_case and what the reference's relocation and noise kernels made of them."""
    out = cases.mcmc_case()
    out['new_opacities'], out['new_scales'] = R.relocation_adjustment(out['old_opacities'], out['old_scales'], out['n_samples'])
    moved = out['means'].copy()
    R.add_noise(out['raw_scales'], out['raw_rotations'], out['raw_opacities'], out['noise'], moved, float(out['current_lr']))
    out['moved_means'] = moved
    path = cases.fixture_path('mcmc')
    np.savez_compressed(path, **out)
    print(path.name, f'{path.stat().st_size / 1e6:.2f} MB')


if __name__ == '__main__':
    for name in cases.CPU_FIXTURES:
        dump(name)
    dump_mcmc()
