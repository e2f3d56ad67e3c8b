"""Shared by the reference-pin tests and tests/golden/make_ref_kernel_golden.py: the scenes, the field-by-field comparison at the bars of the pin, and
the fixture format (tests/golden/ref_kernels_*.npz: what the reference's own kernels computed, run on the CPU by oracle/build_ref.py).

Bars. Integers and indices: exact. Floats without float atomics (records, image, final transmittance, bucket checkpoints): bit for bit between the
oracle and the reference (both -ffp-contract=off fp32 on one libm). Atomic sums (six gradients, densification_info, pruning scores): 1e-5 of the
tensor's maximum (helpers.rel_inf) -- only the order of the additions may differ.
"""
from pathlib import Path

import numpy as np
import torch

import helpers
from harness.scenes import View, make_s0

GOLDEN = Path(__file__).resolve().parent / 'golden'
PARTIAL = [(48, 36, 4, True), (50, 30, 16, False), (16, 12, 1, False), (130, 25, 9, True), (333, 211, 16, False)]
FIXTURES = ('s0', 'tiny_aa', 'partial_333x211', 'partial_130x25')
CPU_FIXTURES = FIXTURES + ('on_the_cut',)          # exact ties are a property of one libm and unfused arithmetic: CPU only
# (raw scale bits x3, raw opacity bits): Gaussians at the origin whose antialiased opacity is EXACTLY 1/255 in unfused fp32 on glibc's expf, found by
# scanning adjacent floats around the logit. Seen through a camera whose principal point is a pixel centre they sit on pixel (64, 64) with delta = 0,
# so there alpha = opacity * exp(0) is exactly the cut as well: `opacity < 1/255` (preprocess cull) and `alpha < 1/255` (both blends) are taken ON the
# threshold, where `<` and `<=` differ.
ON_THE_CUT = ((3229614080, 3229194650, 3230033510, 3232343850), (3227936358, 3227516928, 3228775219, 3232601542),
              (3225629491, 3225210061, 3226468352, 3232756358), (3221435187, 3220806042, 3222274048, 3232826852))
GRAD_SEED = 5
INT_FIELDS = ('n_touched', 'depth_keys', 'prim_idx', 'offsets', 'inst_keys', 'inst_prims', 'ranges')
BLEND_INT_FIELDS = ('n_buckets', 'bucket_offsets', 'n_processed', 'max_n_processed', 'bucket_tile_index')
RECORD_FIELDS = ('mean2d', 'conic_opacity', 'color')
ATOMIC_BAR = 1e-5


def scene(name: str):
    """(params, view, active SH bases, proper antialiasing) of a named scene; every generator is the project's own, seeded."""
    if name == 's0':
        p, v = make_s0()
        return p, v, 16, False
    if name == 'tiny_aa':                       # tests/golden/make_golden.py
        p, v = make_s0(seed=3, n=150)
        return p, View(v.w2c, v.position, 48, 36, 40.0, 40.0, 24.0, 18.0, 0.2, 1e4, torch.tensor([0.2, 0.5, 0.7])), 4, True
    if name.startswith('partial_'):             # test_gpu_parity.py: test_partial_tiles_sh_degrees_antialiasing
        w, h, K, aa = next(c for c in PARTIAL if name == f'partial_{c[0]}x{c[1]}')
        p, v = make_s0(seed=3, n=300)
        return p, View(v.w2c, v.position, w, h, 0.8 * w, 0.8 * w, w / 2.0, h / 2.0, 0.2, 1e4, torch.tensor([0.2, 0.5, 0.7])), K, aa
    if name == 'tied_depth':
        p, v = helpers.tied_depth_scene()
        return p, v, 16, False
    if name == 'large_footprints':              # test_gpu_parity.py: test_large_footprints_and_long_lists, first scene
        p, v = make_s0(seed=7, n=200)
        p['scales'] = p['scales'] + 2.3
        return p, v, 16, False
    if name == 'on_the_cut':
        p, v = make_s0(seed=9, n=120)
        bits = np.array(ON_THE_CUT, np.uint32)
        k = len(ON_THE_CUT)
        p['means'][:k] = 0.0
        p['scales'][:k] = torch.from_numpy(bits[:, :3].copy().view(np.float32))
        p['rotations'][:k] = torch.tensor([1.0, 0.0, 0.0, 0.0])
        p['opacities'][:k] = torch.from_numpy(bits[:, 3:].copy().view(np.float32)).reshape(p['opacities'][:k].shape)
        return p, View(v.w2c, v.position, 128, 128, v.focal_x, v.focal_y, 64.5, 64.5, v.near_plane, v.far_plane, torch.tensor([0.1, 0.2, 0.3])), 16, True
    if name.startswith('fuzz_'):
        p, v, K, aa, _ = helpers.fuzz_configuration(int(name[5:]))
        return p, v, K, aa
    raise KeyError(name)


def mcmc_case() -> dict:
    """Inputs of the MCMC pin: opacities at 0, 1 and next to them, sample counts outside [1, 50] (the kernel clamps), degenerate quaternions."""
    rng = np.random.default_rng(3)
    n = 700
    op = rng.uniform(0.004, 0.999, n).astype(np.float32)
    op[:4] = [0.0, 1.0, 1e-7, 0.5]
    sc = rng.uniform(-3, 1, (n, 3)).astype(np.float32)
    ns = rng.integers(-2, 60, n)
    ns[:6] = [0, 1, 2, 50, 51, 49]
    q = rng.standard_normal((n, 4)).astype(np.float32)
    q[:3] = 0.0
    q[3] = [1e-5, 0, 0, 0]                        # |q|^2 = 1e-10 < 1e-8: left alone
    return {'old_opacities': op, 'old_scales': sc, 'n_samples': ns.astype(np.int64), 'raw_scales': sc, 'raw_rotations': q,
            'raw_opacities': rng.uniform(-8, 8, n).astype(np.float32), 'noise': rng.standard_normal((n, 3)).astype(np.float32),
            'means': rng.standard_normal((n, 3)).astype(np.float32), 'current_lr': np.float32(5e-3)}


def grad_image_of(shape, seed: int = GRAD_SEED) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def score_base_of(n: int) -> np.ndarray:
    """The non-zero vector the pruning scores are accumulated on top of."""
    return np.random.default_rng(17).uniform(0.5, 2.0, n).astype(np.float32)


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def compare_structure(got: dict, ref: dict, label: str, blend: bool = True) -> None:
    """Every integer / index output, zero budget."""
    for k in ('V', 'I') + (('B',) if blend else ()):
        assert int(got[k]) == int(ref[k]), (label, k, int(got[k]), int(ref[k]))
    vis = np.asarray(ref['n_touched']) > 0
    for k in INT_FIELDS + (BLEND_INT_FIELDS if blend else ()):
        assert np.array_equal(np.asarray(got[k]), np.asarray(ref[k])), (label, k, int((np.asarray(got[k]) != np.asarray(ref[k])).sum()))
    assert np.array_equal(np.asarray(got['screen_bounds'])[vis], np.asarray(ref['screen_bounds'])[vis]), (label, 'screen_bounds')


def compare_floats_bitwise(got: dict, ref: dict, label: str, blend: bool = True) -> None:
    """Float outputs that involve no float atomics, bit for bit; records only where the reference defines them (n_touched > 0), checkpoints only
    where a pixel stored one (`ckpt_written` of the reference side, kept in the fixtures)."""
    vis = np.asarray(ref['n_touched']) > 0
    for k in RECORD_FIELDS:
        assert same_bits(np.asarray(got[k])[vis], np.asarray(ref[k])[vis]), (label, k, helpers.rel_inf(np.asarray(got[k])[vis], np.asarray(ref[k])[vis]))
    assert same_bits(got['image'], ref['image']), (label, 'image', helpers.rel_inf(got['image'], ref['image']))
    if blend:
        assert same_bits(got['final_T'], ref['final_T']), (label, 'final_T')
        w = np.asarray(ref['ckpt_written'])
        assert same_bits(np.asarray(got['bucket_ckpt'])[w], np.asarray(ref['bucket_ckpt'])[w]), (label, 'bucket_ckpt')


def compare_atomic_sums(got: dict, ref: dict, label: str, keys=helpers.GRAD_KEYS, bar: float = ATOMIC_BAR, support: bool = True) -> dict:
    """`support`: the Gaussians whose sum is not zero are the same on both sides. A row is zero because no (pixel, Gaussian) pair passed the culls and
    cuts of the backward pass, which is structure, not rounding: a Gaussian whose only contributing pair sits exactly on the alpha cut (the
    on_the_cut scene) moves its tensor's maximum by far less than the bar when that pair is dropped, but it leaves or joins the support."""
    worst = {}
    for k in keys:
        a, r = np.asarray(got[k]), np.asarray(ref[k])
        a = a.reshape(r.shape)
        worst[k] = helpers.rel_inf(a, r)
        if support and k != 'densification_info':          # [2, N]: row 0 counts visits, checked by the bar
            rows = lambda x: (x.reshape(x.shape[0], -1) != 0).any(axis=1)
            assert np.array_equal(rows(a), rows(r)), (label, k, 'support', int((rows(a) != rows(r)).sum()))
        helpers.log_note('reference_pin_atomic_sum', worst[k], scene=label, field=k)
    assert max(worst.values(), default=0.0) < bar, (label, worst)
    return worst


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------
def fixture_path(name: str) -> Path:
    return GOLDEN / f'ref_kernels_{name}.npz'


def load_fixture(name: str):
    """(the reference's outputs under oracle.forward's keys plus 'grad_*', params, view, active SH bases, antialiasing) -- everything from the file:
    the seeded scene generators go through torch's CPU transcendentals, whose last bit differs between machines, so the inputs are stored."""
    g = dict(np.load(fixture_path(name)))
    params = {k: torch.from_numpy(g[f'in_{k}']) for k in helpers.NAMES}
    s = g['settings']
    K, W, H, aa = int(s[0]), int(s[1]), int(s[2]), bool(s[9])
    view = View(torch.from_numpy(g['w2c']), torch.from_numpy(g['cam_position']), W, H, float(s[3]), float(s[4]), float(s[5]), float(s[6]), float(s[7]),
                float(s[8]), torch.from_numpy(g['bg_color']))
    g['grad_image'] = grad_image_of((3, H, W), int(g['grad_seed']))
    for k in ('V', 'I', 'B'):
        g[k] = int(g[k])
    g['ckpt_written'] = np.unpackbits(g['ckpt_written_bits'])[:g['B'] * 192].reshape(g['B'], 192).astype(bool)
    g['bucket_size'] = 32
    return g, params, view, K, aa


def check_backend_against_fixture(be, oracle, name: str, device: str, on_hardware: bool) -> dict:
    """A backend of the HIP sources (the CPU simulation, or the library on an MI355X) against what the reference's kernels computed (the fixture).
    The device's buckets hold 64 entries, the reference's 32: bucket counts are compared with those the fixture's own ranges give at 64, and the
    bucket-independent fields with the fixture.
    Simulation: integers exact, floats 1e-5 of the tensor's maximum (what tests/test_sim_parity.py holds against the oracle).
    Hardware: counts, n_touched, instance keys and primitives, ranges exact; image, gradients, densification_info and pruning scores within 1e-4 of
    the tensor's maximum -- on the partial-tile fixtures outside helpers.flip_masks (pixels / Gaussians that own a pair within an ULP-scale margin of
    the alpha or transmittance cut; at most 1e-3 of the pixels and one Gaussian in a thousand, at least one, may be masked)."""
    g, params, view, K, aa = load_fixture(name)
    S, RS = helpers.settings_pair(view, K, aa, device=device)
    dp = {k: v.to(device).contiguous() for k, v in params.items()}
    n, W, H = dp['means'].shape[0], view.width, view.height
    bar = 1e-4 if on_hardware else 1e-5
    res = be.forward(*[dp[k] for k in helpers.NAMES], RS)
    dec = helpers.decode_forward(be, res, n, W, H)
    assert dec['V'] == g['V'] and dec['I'] == g['I'], (name, dec['V'], g['V'], dec['I'], g['I'])
    for k in ('n_touched', 'inst_keys', 'inst_prims', 'ranges'):
        assert np.array_equal(dec[k], g[k]), (name, k, int((dec[k] != g[k]).sum()))
    lens = (g['ranges'][:, 1] - g['ranges'][:, 0]).astype(np.int64)
    assert np.array_equal(np.cumsum((lens + 31) // 32), g['bucket_offsets'])                 # the fixture's own rule, then the same rule at 64
    assert np.array_equal(dec['bucket_offsets'], np.cumsum((lens + 63) // 64)), (name, 'bucket_offsets at 64')
    vis = g['n_touched'] > 0
    pixel_keep, prim_keep, report = np.ones((H, W), bool), np.ones(n, bool), {}
    if not on_hardware:
        sel = 0 if np.array_equal(dec['prim_idx0'], g['prim_idx']) else 1
        assert np.array_equal(dec[f'prim_idx{sel}'], g['prim_idx']) and np.array_equal(dec[f'depth_keys{sel}'], g['depth_keys']), (name, 'depth order')
        assert np.array_equal(dec['offsets'], g['offsets']) and np.array_equal(dec['screen_bounds'][vis], g['screen_bounds'][vis]), (name, 'offsets / bounds')
        assert np.array_equal(helpers.tiles_to_image(dec['n_processed_tiles'], W, H).reshape(-1), g['n_processed']), (name, 'n_processed')
        assert np.array_equal(dec['max_n_processed'], g['max_n_processed']), (name, 'max_n_processed')
        for k in RECORD_FIELDS:
            assert helpers.rel_inf(dec[k][vis], g[k][vis]) < bar, (name, k)
        assert helpers.rel_inf(helpers.tiles_to_image(dec['final_T_tiles'], W, H).reshape(-1), g['final_T']) < bar, (name, 'final_T')
    elif name.startswith('partial_'):
        f = oracle.forward(*helpers.np_params(params), S, bucket_size=64)
        masks = helpers.flip_masks(oracle, f, S, dec)
        pixel_keep, prim_keep = ~masks['pixel'], ~masks['prim']
        report['masked_pixels'], report['masked_gaussians'] = int(masks['pixel'].sum()), int(masks['prim'].sum())
        helpers.log_note('reference_pin_masked', report['masked_pixels'], scene=name, gaussians=report['masked_gaussians'])
        assert report['masked_pixels'] < 1e-3 * W * H and report['masked_gaussians'] <= max(1, n // 1000), (name, report)
    image = res.image.detach().cpu().numpy()
    err = np.abs(image.astype(np.float64) - g['image']).max(axis=0)
    report['image'] = float(err[pixel_keep].max() / (np.abs(g['image']).max() + 1e-30))
    print(f'{name}: image {report["image"]:.3e}')
    assert report['image'] < bar, (name, 'image', report)
    dens = torch.zeros(2, n, device=device)
    grads = be.backward(dens, torch.from_numpy(g['grad_image']).to(device), res.image, dp['means'], dp['scales'], dp['rotations'], dp['opacities'],
                        dp['sh_coefficients_rest'], res.buffers, RS, res.state)
    got = {k: t.detach().cpu().numpy() for k, t in zip(helpers.GRAD_KEYS, grads)}
    got['densification_info'] = dens.cpu().numpy().T                   # Gaussian index first, like the gradients
    ref = {k: g[f'grad_{k}'] for k in helpers.GRAD_KEYS}
    ref['densification_info'] = g['densification_info'].T
    scores = torch.from_numpy(score_base_of(n)).to(device)
    be.pruning_scores(scores, *[dp[k] for k in helpers.NAMES], RS)
    got['pruning_scores'], ref['pruning_scores'] = scores.cpu().numpy(), g['pruning_scores']
    for k in ref:
        report[k] = helpers.masked_rel_inf(got[k].reshape(ref[k].shape), ref[k], prim_keep)
        helpers.log_note('reference_pin_fixture', report[k], scene=name, field=k, hardware=on_hardware)
        print(f'{name}: {k} {report[k]:.3e}')
    assert max(report[k] for k in ref) < bar, (name, report)
    return report
