"""Cases and checks shared by tests/test_adc_edges.py (CPU simulation) and tests/test_gpu_adc_edges.py (MI355X) for adaptive density control:
adc_classify_kernel, the three scan kernels, adc_scatter_kernel<KIND> (csrc/densify.hip), fgs_adc_plan_thresholds / fgs_adc_apply and
Backend.adaptive_density_control. Every check takes (backend, oracle, device, case name).

Reference: oracle.adaptive_density_control, the numpy restatement of the reference's Model.py:312-366; its four masks (oracle.adc_masks) are held to the
same expressions written with torch on float32 CPU tensors by tests/test_adc_edges.py::test_restatement_masks_equal_torch.

Bars (check_case):
  counts                          equal, and the REFERENCE's counts are what the case was built to produce (`expect`), so a case that drifts cannot pass vacuously
  sh0, sh_rest, opacities, rotations, survivor and clone rows of means / scales        bit-equal (they are copies)
  children's means / scales       2e-6 (1 + max |ref|) over the finite entries of the reference tensor: expf / logf / sqrtf of different libms; non-finite
                                  entries must be the same NaN positions and the same infinities
  moments                         survivors bit-equal, clones and children exactly 0
  noise                           asked for once, 2 * split rows, from a seeded generator

Threshold cases use percent_dense = 2^-7, extent = 4, min_opacity = 2^-8: exact in float32, so every way of forming the thresholds gives the same three
floats and only the comparison itself is under test. The 'refthr' cases are the exception: they hold the device to the reference's thresholds for scalars
that float32 cannot carry.

Children next to log_large: logf(expf(s)) differs between libms by a few ulps, so every case keeps the children's largest scale at least 64 ulps away
from log_large (asserted on the reference values, _assert_child_margin)."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np
import torch

ORDER = ('means', 'sh_coefficients_0', 'sh_coefficients_rest', 'opacities', 'scales', 'rotations')
PD, EXTENT, MIN_OPACITY, GRAD_T = 2.0 ** -7, 4.0, 2.0 ** -8, 2e-4
F = np.float32
LOG_SMALL, LOG_LARGE, OPACITY_LOGIT = F(math.log(PD * EXTENT)), F(math.log(0.1 * EXTENT)), F(math.log(MIN_OPACITY / (1 - MIN_OPACITY)))
SMALL, MEDIUM = -5.0, -2.0                  # below log_small = -3.47: cloned when densified; between it and log_large = -0.92: split
ROW_COUNTS = (0, 1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 8192, 2 * 4096 + 37)      # 16 words per thread, 256 threads, 4096 per workgroup
PLAN_COUNTS = (1, 16, 4096, 4097)
PLANS = ('all_cloned', 'all_split', 'nothing_densified', 'all_pruned', 'only_last', 'only_first')
TWO_THREADS = 17 * 4096 + 5                 # 18 block sums, 16 per thread: the second thread of adc_scan_blocks_kernel holds two of them
SECOND_WAVE = 1024 * 4096 + 4096 + 5        # 1026 block sums: a wave holds 64 x 16 = 1024, the first thread of the second wave the last two
REFERENCE_EXTENTS = (3.925284601749901, 11.058493794857288, 19.945593747889614) + tuple(float(e) for e in np.random.default_rng(20261020).uniform(0.5, 20.0, 20))
# min_opacity whose logit rounds differently from the double and from its float32 neighbour (searched over k / 10000, k < 1000: 98 of 999 do)
REFERENCE_MIN_OPACITIES = (0.001, 0.0054)
# |q|^2 = 1e-8f - 1 ulp, 1e-8f, 1e-8f + 1 ulp EXACTLY, in every summation order: 1e-8f = 11258999 * 2^-50 and each of the three integers is a sum of four
# squares of integers below 2^12 (products and partial sums are integers below 2^24)
QUATERNION_SQUARES = ((3355, 14, 44, 29), (3355, 27, 47, 6), (3348, 40, 214, 50))


@dataclasses.dataclass
class Case:
    P: dict                                  # float32 CPU tensors keyed ORDER
    info: torch.Tensor                       # [2, n]: counts, gradient sums
    expect: tuple | None                     # (survivors, clones, children per copy, split) the reference must give; None: only 'more than nothing of each'
    prune_large: bool = True
    with_state: bool = True
    grad_threshold: float = GRAD_T
    min_opacity: float = MIN_OPACITY
    percent_dense: float = PD
    extent: float = EXTENT
    child_margin: bool = True

    @property
    def n(self) -> int:
        return self.P['means'].shape[0]

    def moments(self, which: int) -> dict:
        gen = torch.Generator().manual_seed(100 + which)
        return {k: (torch.randn(self.P[k].shape, generator=gen) * 1e-3 if which == 0 else torch.rand(self.P[k].shape, generator=gen) * 1e-6 + 1e-9) for k in ORDER}


def _base(n: int, bases: int = 15, seed: int = 0, scale: float = MEDIUM):
    """n live Gaussians that nothing happens to: gradient sum 0 with count 1, opacity logits in [-1, 1], generic rotations, the largest scale `scale`."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.rand(shape, generator=gen)
    scales = scale - rnd(n, 3)
    if n:
        scales[torch.arange(n), torch.randint(0, 3, (n,), generator=gen)] = scale
    P = {'means': rnd(n, 3) * 4.0 - 2.0, 'sh_coefficients_0': rnd(n, 1, 3) - 0.5, 'sh_coefficients_rest': rnd(n, bases, 3) * 0.2 - 0.1,
         'opacities': rnd(n, 1) * 2.0 - 1.0, 'scales': scales, 'rotations': torch.nn.functional.normalize(rnd(n, 4) + 0.1, dim=1) * (0.5 + rnd(n, 1))}
    info = torch.zeros(2, n)
    info[0] = 1.0
    return P, info


def _around(x) -> list:
    """The float32 below x, x, the float32 above x."""
    x = F(x)
    return [float(np.nextafter(x, F(-np.inf))), float(x), float(np.nextafter(x, F(np.inf)))]


def _set_max_scale(P, row: int, value: float, component: int = 0, below: float = 1.0) -> None:
    P['scales'][row] = value - below
    P['scales'][row, component] = value


def _gradient_threshold_case() -> Case:
    """grad_sum against grad_threshold * max(count, 1) (>=), count 0 / 1 / 29, below / at / above; rows 0-8 small (cloned), 9-17 medium (split)."""
    P, info = _base(18)
    P['scales'][:9] += SMALL - MEDIUM
    for half in (0, 9):
        for i, count in enumerate((0.0, 1.0, 29.0)):
            threshold = F(GRAD_T) * max(F(count), F(1.0))
            for j, value in enumerate(_around(threshold)):
                info[0, half + 3 * i + j], info[1, half + 3 * i + j] = count, value
    return Case(P, info, (9 + 3, 6, 6, 6))


def _log_small_case(prune_large: bool) -> Case:
    """The largest scale against log_small (<=), in each of the three components, all densified: below and at are cloned, above is split."""
    P, info = _base(9)
    for comp in range(3):
        for j, value in enumerate(_around(LOG_SMALL)):
            _set_max_scale(P, 3 * comp + j, value, comp)
    info[1] = 1.0
    return Case(P, info, (6, 6, 3, 3), prune_large=prune_large)


def _log_large_case(prune_large: bool) -> Case:
    """The largest scale against log_large (>), in each component: rows 0-8 not densified (above is pruned with prune_large only), rows 9-17 densified
    (split whatever the verdict; their children are far below)."""
    P, info = _base(18)
    for half in (0, 9):
        for comp in range(3):
            for j, value in enumerate(_around(LOG_LARGE)):
                _set_max_scale(P, half + 3 * comp + j, value, comp)
    info[1, 9:] = 1.0
    return Case(P, info, (6 if prune_large else 9, 0, 9, 9), prune_large=prune_large)


def _opacity_case() -> Case:
    """The opacity against the logit of min_opacity (<): below is dead. Rows 0-2 not densified, 3-5 cloned, 6-8 split."""
    P, info = _base(9)
    P['scales'][3:6] += SMALL - MEDIUM
    info[1, 3:] = 1.0
    for group in range(3):
        for j, value in enumerate(_around(OPACITY_LOGIT)):
            P['opacities'][3 * group + j] = value
    return Case(P, info, (2 + 2, 2, 2, 3))


def quaternion_edges() -> list:
    """(quaternion, dead) pairs around |q|^2 < 1e-8f. Exact sums (QUATERNION_SQUARES, also permuted and with signs), and one-component quaternions: no float32
    a has fl(a * a) == 1e-8f (the neighbours of 1e-4f give 0x1.5798ecp-27 and 0x1.5798f0p-27), so those are the last dead and the first live a."""
    t = F(1e-8)
    out = []
    for squares, dead in zip(QUATERNION_SQUARES, (True, False, False)):
        q = np.array(squares, F) * F(2.0 ** -25)
        assert float((q.astype(np.float64) ** 2).sum()) == float(_around(t)[len(out) // 3])
        out += [(q, dead), (q[::-1].copy(), dead), (q * np.array([-1, 1, -1, 1], F), dead)]
    a = F(1e-4)
    while F(a * a) >= t:
        a = np.nextafter(a, F(0))
    while F(np.nextafter(a, F(1)) * np.nextafter(a, F(1))) < t:
        a = np.nextafter(a, F(1))
    b = np.nextafter(a, F(1))
    assert F(a * a) < t < F(b * b)
    for position in (0, 3):
        for value, dead in ((a, True), (b, False)):
            q = np.zeros(4, F)
            q[position] = value
            out.append((q, dead))
    return out


def _rotation_case() -> Case:
    """|q|^2 against 1e-8f (<): every quaternion of quaternion_edges() once not densified, once cloned, once split."""
    edges = quaternion_edges()
    k = len(edges)
    P, info = _base(3 * k)
    P['scales'][k:2 * k] += SMALL - MEDIUM
    info[1, k:] = 1.0
    for group in range(3):
        for j, (q, _) in enumerate(edges):
            P['rotations'][group * k + j] = torch.from_numpy(q)
    live = sum(not dead for _, dead in edges)
    return Case(P, info, (2 * live, live, live, k))


def _interactions_case() -> Case:
    """Parents above log_large whose children log(0.625 exp(s)) = s - 0.47 fall below it (rows 0-2: live, dead opacity, degenerate rotation), a parent whose
    children are still too large (row 3), dead clones (rows 4-5), a live clone (6), a bystander that is too large (7) and one that is not (8)."""
    P, info = _base(9)
    info[1, :7] = 1.0
    for row in range(3):
        _set_max_scale(P, row, -0.7, row)
    _set_max_scale(P, 3, 0.0, 1)
    for row in (4, 5, 6):
        _set_max_scale(P, row, SMALL, row % 3)
    _set_max_scale(P, 7, -0.5, 2)
    P['opacities'][1] = P['opacities'][4] = -9.0
    P['rotations'][2] = P['rotations'][5] = 0.0
    # survivors: rows 6 and 8; clones: row 6; children per copy: row 0; split: rows 0-3
    return Case(P, info, (2, 1, 1, 4))


def _clone_too_large_case() -> Case:
    """percent_dense = 0.5 (exact) puts log_small = log 2 above log_large = log 0.4: a clone can be too large, and then neither copy survives (row 0);
    row 1 is a clone small enough, row 2 a too-large bystander, row 3 splits (its children, 1.0 - 0.47, are too large: every child is under this
    percent_dense), row 4 a bystander small enough."""
    P, info = _base(5)
    info[1, [0, 1, 3]] = 1.0
    _set_max_scale(P, 0, 0.0, 1)
    _set_max_scale(P, 1, -1.5, 2)
    _set_max_scale(P, 2, 0.5, 0)
    _set_max_scale(P, 3, 1.0, 0)
    _set_max_scale(P, 4, -1.5, 1)
    return Case(P, info, (2, 1, 0, 1), percent_dense=0.5)


def _nonfinite_case(prune_large: bool) -> Case:
    """Non-finite inputs are not sanitised, the comparisons are the reference's: every comparison with a NaN is false.
      rows 0-7    grad_sum NaN, +inf, -inf, -1 with count 0 and count 5, small scales: only +inf densifies (two clones)
      rows 8-10   a NaN in scale component 0 / 1 / 2, densified: the largest scale is NaN, not small -> split; the children's largest scale is NaN, not too
                  large. The other components are small in rows 8-9 (a max that drops the NaN clones them) and 0.0 in row 10 (it prunes the children)
      row 11      a NaN scale component beside two above log_large, not densified: NaN is not too large, it stays (a max that drops the NaN prunes it)
      rows 12-13  NaN opacity, not densified / cloned: NaN is not below the logit, alive
      rows 14-15  a NaN rotation component, not densified / split: the squared norm is NaN, not below 1e-8, alive; the children's means are NaN
      rows 16-17  +inf scale component, not densified / split: too large with prune_large (the children as well: log(0.625 inf) = inf)"""
    nan, inf = float('nan'), float('inf')
    P, info = _base(18)
    P['scales'][:8] += SMALL - MEDIUM
    for i, g in enumerate((nan, inf, -inf, -1.0)):
        info[0, i], info[1, i] = 0.0, g
        info[0, 4 + i], info[1, 4 + i] = 5.0, g
    P['scales'][8:10] += SMALL - MEDIUM
    P['scales'][10] = 0.0
    P['scales'][11] = -0.5
    for comp in range(3):
        P['scales'][8 + comp, comp] = nan
    P['scales'][11, 1] = nan
    info[1, 8:11] = 1.0
    P['opacities'][12] = P['opacities'][13] = nan
    P['scales'][13] += SMALL - MEDIUM
    info[1, 13] = 1.0
    P['rotations'][14, 2] = P['rotations'][15, 0] = nan
    info[1, 15] = 1.0
    P['scales'][16, 2] = P['scales'][17, 0] = inf
    info[1, 17] = 1.0
    kept = 8 + 1 + 2 + 1 + (0 if prune_large else 1)                  # rows 0-7, 11, 12-13, 14, 16
    children = 3 + 1 + (0 if prune_large else 1)                      # rows 8-10, 15, 17
    return Case(P, info, (kept, 2 + 1, children, 5), prune_large=prune_large, child_margin=False)


def _mixed_case(n: int, prune_large: bool, with_state: bool, bases: int | None = None, seed: int = 5) -> Case:
    """A seeded plan in which every verdict occurs at random positions: half densify; a third each small / medium / above log_large (children below it: -0.7,
    or still above it: 0.0); a tenth dead by opacity, a twentieth by rotation."""
    bases = (15 if n < 4095 else 0) if bases is None else bases
    P, info = _base(n, bases=bases, seed=seed)
    gen = torch.Generator().manual_seed(seed + 1)
    pick = lambda frac: torch.rand(n, generator=gen) < frac
    info[0] = torch.randint(0, 30, (n,), generator=gen).float()
    info[1] = pick(0.5).float() * info[0].clamp_min(1.0) * (1.5 * GRAD_T)
    kind = torch.randint(0, 4, (n,), generator=gen)
    shift = torch.tensor([SMALL - MEDIUM, 0.0, -0.7 - MEDIUM, 0.0 - MEDIUM])[kind]
    P['scales'] += shift[:, None]
    P['opacities'][pick(0.1)] = -9.0
    P['rotations'][pick(0.05)] = 0.0
    return Case(P, info, None, prune_large=prune_large, with_state=with_state)


def _plan_case(plan: str, n: int) -> Case:
    """Saturated and empty plans: a full 4096-Gaussian workgroup block puts 4096 = 2^12 into one 16-bit field of the packed scan, in one, two or all four fields."""
    P, info = _base(n, bases=15 if n < 4095 else 0, seed=n)
    expect = {'all_cloned': (n, n, 0, 0), 'all_split': (0, 0, n, n), 'nothing_densified': (n, 0, 0, 0), 'all_pruned': (0, 0, 0, n // 2),
              'only_last': (n - 1, 0, 1, 1), 'only_first': (n, 1, 0, 0)}[plan]
    if plan == 'all_cloned':
        info[1] = 1.0
        P['scales'] += SMALL - MEDIUM
    elif plan == 'all_split':
        info[1] = 1.0
    elif plan == 'all_pruned':                   # dead by opacity; the odd rows are split on top (noise is drawn for children that are never written)
        info[1, 1::2] = 1.0
        P['opacities'][:] = -9.0
    elif plan == 'only_last':
        info[1, n - 1] = 1.0
    elif plan == 'only_first':
        info[1, 0] = 1.0
        P['scales'][0] += SMALL - MEDIUM
    return Case(P, info, expect)


def _reference_threshold_case(extent: float, min_opacity: float) -> Case:
    """The reference's thresholds for scalars that float32 cannot carry: f32(log(pd * extent)), f32(log(0.1 * extent)), f32(log(p / (1 - p))) from DOUBLE
    pd = 0.01, extent and p, each with its float32 neighbours. rows 0-2 densified around log_small (two clones, one split), 3-5 not densified around log_large
    (one pruned), 6-8 densified around log_large (split), 9-11 not densified around the opacity logit (one dead)."""
    assert float(F(extent)) != extent and float(F(min_opacity)) != min_opacity
    P, info = _base(12, seed=int(extent * 1000))
    info[1, :3] = info[1, 6:9] = 1.0
    for j in range(3):
        _set_max_scale(P, j, _around(math.log(0.01 * extent))[j], j)
        _set_max_scale(P, 3 + j, _around(math.log(0.1 * extent))[j], j)
        _set_max_scale(P, 6 + j, _around(math.log(0.1 * extent))[j], (j + 1) % 3)
        P['opacities'][9 + j] = _around(math.log(min_opacity / (1 - min_opacity)))[j]
    P['scales'][9:] = float(F(math.log(0.01 * extent))) + 0.5            # medium, whatever the extent
    return Case(P, info, (2 + 2 + 2, 2, 4, 4), min_opacity=min_opacity, percent_dense=0.01, extent=extent)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    """Cases by name; tuples are (kind, ...). The tensors of a case are shared between the tests: nobody writes to them."""
    if name == 'gradient_threshold':
        return _gradient_threshold_case()
    if name == 'opacity':
        return _opacity_case()
    if name == 'rotation':
        return _rotation_case()
    if name == 'interactions':
        return _interactions_case()
    if name == 'clone_too_large':
        return _clone_too_large_case()
    kind = name[0]
    if kind == 'log_small':
        return _log_small_case(name[1])
    if kind == 'log_large':
        return _log_large_case(name[1])
    if kind == 'nonfinite':
        return _nonfinite_case(name[1])
    if kind == 'mixed':
        return _mixed_case(*name[1:])
    if kind == 'plan':
        return _plan_case(*name[1:])
    if kind == 'refthr':
        return _reference_threshold_case(*name[1:])
    raise KeyError(name)


THRESHOLD_CASES = ('gradient_threshold', ('log_small', True), ('log_small', False), ('log_large', True), ('log_large', False), 'opacity', 'rotation',
                   'interactions', 'clone_too_large')
NONFINITE_CASES = (('nonfinite', True), ('nonfinite', False))
# every count with and without prune_large, with and without moments; (4097, ..., 15): the case beyond a workgroup block that keeps its 15 SH-rest bases
MIXED_CASES = tuple(('mixed', n, pl, st) for n in ROW_COUNTS for pl in (True, False) for st in (True, False)) + (('mixed', 4097, True, True, 15),)
PLAN_CASES = tuple(('plan', plan, n) for n in PLAN_COUNTS for plan in PLANS)
TWO_THREADS_CASE = ('mixed', TWO_THREADS, True, False, 0)
SECOND_WAVE_CASE = ('mixed', SECOND_WAVE, True, False, 0)
REFERENCE_THRESHOLD_CASES = tuple(('refthr', e, 0.005) for e in REFERENCE_EXTENTS) + tuple(('refthr', REFERENCE_EXTENTS[0], p) for p in REFERENCE_MIN_OPACITIES)
PINNED_CASES = THRESHOLD_CASES + NONFINITE_CASES + REFERENCE_THRESHOLD_CASES       # the inputs on which the restatement's masks are held to torch's


def case_id(name) -> str:
    return name if isinstance(name, str) else '-'.join(str(part) for part in name)


def seeded_noise(rows: int) -> torch.Tensor:
    return torch.randn((rows, 3), generator=torch.Generator().manual_seed(11))


_REFERENCES: dict = {}


def reference(oracle, name):
    """(params, exp_avgs, exp_avg_sqs, counts) of the restatement for a case, computed once per process."""
    if name not in _REFERENCES:
        c = case(name)
        as_np = lambda d: {k: d[k].numpy() for k in ORDER}
        with np.errstate(all='ignore'):
            masks = oracle.adc_masks(c.info.numpy(), c.P['opacities'].numpy(), c.P['scales'].numpy(), c.P['rotations'].numpy(), c.grad_threshold, c.min_opacity,
                                     c.percent_dense, c.extent)
            n_split = int((masks['densify'] & ~masks['small']).sum())
            ref = oracle.adaptive_density_control(as_np(c.P), as_np(c.moments(0)) if c.with_state else None, as_np(c.moments(1)) if c.with_state else None,
                                                  c.info.numpy(), seeded_noise(2 * n_split).numpy(), c.grad_threshold, c.min_opacity, c.prune_large,
                                                  c.percent_dense, c.extent)
        counts = tuple(ref[3])
        assert counts[3] == n_split
        if c.expect is not None:
            assert counts == tuple(c.expect), ('the case no longer produces what it was built for', name, counts, c.expect)
        elif c.n >= 255:
            assert min(counts) > 0 and counts[0] < c.n, ('a mixed plan must hold every verdict', name, counts)
        if c.child_margin and c.prune_large and counts[3]:
            _assert_child_margin(c, masks)
        _REFERENCES[name] = (ref[0], ref[1], ref[2], counts)
    return _REFERENCES[name]


def _assert_child_margin(c: Case, masks: dict) -> None:
    """The largest scale of every child is at least 64 ulps away from log_large: on which side it falls does not depend on the libm."""
    split = masks['densify'] & ~masks['small']
    s = c.P['scales'].numpy()[split]
    child_max = np.log(np.exp(s) * F(0.625)).max(axis=1)
    log_large = F(math.log(0.1 * c.extent))
    assert np.all(np.abs(child_max - log_large) >= 64 * np.spacing(np.abs(log_large))), float(np.abs(child_max - log_large).min())


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_children_close(a: np.ndarray, ref: np.ndarray, whole_ref: np.ndarray, what) -> None:
    finite = np.isfinite(ref)
    assert np.array_equal(np.isnan(a), np.isnan(ref)), (what, 'NaN positions')
    infinite = ~finite & ~np.isnan(ref)
    assert np.array_equal(a[infinite], ref[infinite]), (what, 'infinities')
    if finite.any():
        whole_finite = whole_ref[np.isfinite(whole_ref)]
        bar = 2e-6 * (1.0 + float(np.abs(whole_finite).max()))
        err = float(np.abs(a[finite].astype(np.float64) - ref[finite]).max())
        assert err <= bar, (what, err, bar)


def check_case(be, oracle, device, name) -> tuple:
    """Backend.adaptive_density_control on `device` against the restatement; returns the counts."""
    c = case(name)
    ref_p, ref_m, ref_v, ref_counts = reference(oracle, name)
    asked = []

    def noise_fn(rows):
        asked.append(rows)
        return seeded_noise(rows).to(device)
    on_device = lambda d: [d[k].to(device) for k in ORDER]
    m_in, v_in = (c.moments(0), c.moments(1)) if c.with_state else (None, None)
    out_p, out_m, out_v, counts = be.adaptive_density_control(c.info.to(device), on_device(c.P), on_device(m_in) if c.with_state else None,
                                                              on_device(v_in) if c.with_state else None, c.grad_threshold, c.min_opacity, c.prune_large,
                                                              c.percent_dense, c.extent, noise_fn)
    assert tuple(counts) == ref_counts, (name, 'counts (survivors, clones, children per copy, split)', tuple(counts), ref_counts)
    assert asked == [2 * ref_counts[3]], (name, asked)
    kept, clones, children, _ = ref_counts
    copies = kept + clones
    for i, k in enumerate(ORDER):
        a = out_p[i].cpu().numpy()
        assert a.shape == ref_p[k].shape == (copies + 2 * children,) + tuple(c.P[k].shape[1:]) and a.dtype == np.float32, (name, k, a.shape)
        if k in ('means', 'scales'):
            assert np.array_equal(_bits(a[:copies]), _bits(ref_p[k][:copies])), (name, k, 'survivors and clones')
            _assert_children_close(a[copies:], ref_p[k][copies:], ref_p[k], (name, k, 'children'))
        else:
            assert np.array_equal(_bits(a), _bits(ref_p[k])), (name, k)
        if c.with_state:
            for out, ref, which in ((out_m, ref_m, 'exp_avg'), (out_v, ref_v, 'exp_avg_sq')):
                s = out[i].cpu().numpy()
                assert s.shape == a.shape, (name, k, which)
                assert np.array_equal(_bits(s[:kept]), _bits(ref[k][:kept])), (name, k, which, 'survivors')
                assert not ref[k][kept:].any() and np.all(s[kept:] == 0.0), (name, k, which, 'clones and children start at zero')
    if not c.with_state:
        assert out_m is None and out_v is None
    return ref_counts


def torch_masks(c: Case) -> dict:
    """The four masks of the reference's adaptive density control written with torch on float32 CPU tensors and Python-double scalars (what torch makes of
    'float32 tensor <= double scalar' and of a row-wise max over a NaN is the point)."""
    info, scales, rotations, opacities = c.info, c.P['scales'], c.P['rotations'], c.P['opacities']
    assert all(t.dtype == torch.float32 and t.device.type == 'cpu' for t in (info, scales, rotations, opacities))
    row_max = torch.max(scales, dim=1).values
    return {'densify': info[1] >= c.grad_threshold * info[0].clamp_min(1.0),
            'small': row_max <= math.log(c.percent_dense * c.extent),
            'dead': (opacities.flatten() < math.log(c.min_opacity / (1 - c.min_opacity))) | (rotations.mul(rotations).sum(dim=1) < 1e-8),
            'too_large': row_max > math.log(0.1 * c.extent)}


def all_dead_model(device, n: int = 300):
    """A harness model in which every Gaussian is dead (opacity logit -9), half of them above the gradient threshold, with recognisable optimizer state."""
    from harness.scenes import make_s0
    from harness.trainer import Gaussians
    params, _ = make_s0(seed=3, n=n)
    params['opacities'][:] = -9.0
    g = Gaussians(params, device)
    g.training_setup(training_cameras_extent=5.0)
    for group in g.optimizer.param_groups:
        p = group['params'][0]
        g.optimizer.state[p] = {'step': 7, 'exp_avg': torch.full_like(p, 0.5), 'exp_avg_sq': torch.full_like(p, 0.25)}
    info = torch.zeros(2, n)
    info[0] = 10.0
    info[1, ::2] = 1.0
    g.densification_info = info.to(device)
    return g


def check_harness_prunes_everything(be, device) -> None:
    """harness.densify.adaptive_density_control when nothing survives: no exception, zero-row parameters and zero-row moments of matching shapes."""
    from harness import densify as D
    from harness.trainer import PARAM_ORDER
    g = all_dead_model(device)
    shapes = {k: tuple(getattr(g, k).shape[1:]) for k in PARAM_ORDER}
    stats = D.adaptive_density_control(g, 2e-4, 0.005, True, generator=torch.Generator().manual_seed(0), ops_backend=be)
    assert stats['total'] == 0 and stats['kept'] == 0 and stats['cloned'] == 0 and stats['children_per_copy'] == 0 and stats['pruned'] == 300
    assert g.densification_info is None
    for group in g.optimizer.param_groups:
        p = group['params'][0]
        assert p is getattr(g, group['name']) and tuple(p.shape) == (0,) + shapes[group['name']], group['name']
        st = g.optimizer.state[p]
        assert st['step'] == 7 and st['exp_avg'].shape == p.shape and st['exp_avg_sq'].shape == p.shape and st['exp_avg'].device == p.device, group['name']
