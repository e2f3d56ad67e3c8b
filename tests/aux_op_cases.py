"""Models, inputs and checks shared by tests/test_aux_ops.py (CPU simulation) and tests/test_gpu_aux_ops.py (MI355X) for the three operators of
csrc/aux_ops.hip: update_3d_filter, relocation_adjustment, add_noise. Every check takes (backend, oracle, device).

Models (none is a restatement of the kernel's loops, none comes from the kernels' output):
  relocation   x = 1 - (1 - o)^(1/n), den = sum_k C(n, k+1) (-1)^k x^(k+1) / sqrt(k+1) (the hockey-stick form of the kernel's double loop over its
               50 x 50 table), factor = o / den, in `decimal` at 50 digits; a 1-in-37 subsample is re-evaluated at 80 digits and must agree to 1e-15
  add_noise    R diag(exp(2 s)) R^T from the unnormalised quaternion, the sigmoid and lr / (1 + exp(100 sigma - 0.5)) in fp64 numpy
  3D filter    the five frustum tests and the filter comparison in fp64 numpy; on the boundary scenes every quantity is exact in fp32 AND fp64, so the
               decisions are compared exactly against labels written down beside the points

Bars:
  new_opacity  max |kernel - model| <= 2 x max |restatement - model| + 2^-24 (absolute: the relative error of 1 - powf reaches 2.7e-4 at o = 0.005)
  scale factor relerr_i / u_i, u_i = 2^-24 (1 / x_i + A_i), A_i = sum |terms| / |sum terms|: the kernel's maximum <= 2 x the restatement's, and the
               restatement's <= 2 (asserted: a change of inputs cannot loosen the bar). 1 / x_i carries the cancellation of 1 - powf into the powers
               of x, A_i the cancellation of the alternating sum.
  displacement e_i = max-norm error / (factor max(var) |noise|_2) over (100 sigma_i + 8) 2^-24 -- the exponent 100 sigma - 0.5 carries its own rounding
               into exp -- the kernel's maximum <= 2 x the restatement's, the restatement's <= 4; rows whose true factor is below 1e-30 (fp32 gives
               exactly 0 once expf overflows, sigma > 0.892) are held absolutely: |displacement| <= 1e-25
The factor 2 allows the device's powf / expf to be an ulp or two off glibc's, plus FMA contraction; nothing else may differ.

Guard rows: every output and in-place tensor is allocated with GUARD_ROWS extra rows of a sentinel behind the N rows handed to the operator and those
rows must be bit-unchanged afterwards -- a write past N is caught inside the allocation. Inputs carry the same padding, so no lane could read outside one."""
from __future__ import annotations

import decimal
import functools
import math

import numpy as np
import torch

import helpers

U = 2.0 ** -24
GUARD_ROWS = 64
ROW_COUNTS = (0, 1, 255, 256, 257, 1000)
SENTINEL = 7777.25
THREE_WAY = 2.0                  # kernel's maximum over the restatement's
RELOCATION_CONDITION = 2.0       # the restatement's own r on relocation_inputs(); measured 1.07 on these inputs
NOISE_CONDITION = 4.0            # the restatement's own maximum on noise_inputs(); measured 1.19 on these inputs
NOISE_LR = 80.0                  # 5e5 * 1.6e-4, the trainer's first value
MAX_SAMPLES = 50


# ---- guard rows ------------------------------------------------------------------------------------------------------------------------------------------
def guarded(values: torch.Tensor, device, sentinel=SENTINEL):
    """(contiguous view of the first N rows, the whole allocation of N + GUARD_ROWS rows) on `device`."""
    n = values.shape[0]
    whole = torch.full((n + GUARD_ROWS,) + tuple(values.shape[1:]), sentinel, dtype=values.dtype)
    whole[:n] = values
    whole = whole.to(device)
    view = whole[:n]
    assert view.is_contiguous() and (n == 0 or view.data_ptr() == whole.data_ptr())
    return view, whole


def guard_intact(whole: torch.Tensor, n: int, sentinel=SENTINEL) -> bool:
    tail = whole[n:].cpu()
    return tail.shape[0] == GUARD_ROWS and torch.equal(tail, torch.full_like(tail, sentinel))


def _padded(values: torch.Tensor, device, fill) -> torch.Tensor:
    """Read-only input: its first N rows as a view of an allocation with GUARD_ROWS more rows of `fill` (values a lane would act on)."""
    return guarded(values, device, fill)[0]


def _t(a, dtype=torch.float32) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(dtype)                    # a copy: the cached inputs are read-only


# ---- relocation_adjustment -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def relocation_inputs():
    """(opacities [3100] f32, scales [3100, 3] f32, n_samples [3100] i64): n cycles 1..50 over the rows; the columns of the scales differ in magnitude."""
    rng = np.random.default_rng(2024)
    f = np.float32
    low = np.exp(rng.uniform(np.log(0.005), np.log(0.5), 1500))
    high = rng.uniform(0.5, 1.0, 1500)
    o = np.concatenate([low, high, np.full(50, 1.0 - U), np.full(50, 0.005)]).astype(f)
    o = np.clip(o, f(0.005), f(1.0 - U))
    ns = (np.arange(o.size) % MAX_SAMPLES + 1).astype(np.int64)
    sc = (10.0 ** rng.uniform([-4.0, -2.0, 0.0], [-3.0, 0.0, 1.0], (o.size, 3))).astype(f)
    for a in (o, ns, sc):
        a.setflags(write=False)
    return o, sc, ns


@functools.lru_cache(maxsize=None)
def _sqrt_table(prec: int):
    ctx = decimal.Context(prec=prec)
    return [None] + [ctx.sqrt(decimal.Decimal(k)) for k in range(1, MAX_SAMPLES + 1)]


def _relocation_row(o: float, n: int, prec: int):
    """(x, factor, A) as Decimals at `prec` digits; n already clamped."""
    D, ctx, roots = decimal.Decimal, decimal.Context(prec=prec), _sqrt_table(prec)
    o, one = D(float(o)), D(1)
    rest = ctx.subtract(one, o)
    x = ctx.subtract(one, ctx.power(rest, ctx.divide(one, D(n)))) if rest != 0 else one
    total, total_abs, power = D(0), D(0), one
    for k in range(n):
        power = ctx.multiply(power, x)
        term = ctx.divide(ctx.multiply(D(math.comb(n, k + 1)), power), roots[k + 1])
        total_abs = ctx.add(total_abs, term)
        total = ctx.add(total, term) if k % 2 == 0 else ctx.subtract(total, term)
    return x, ctx.divide(o, total), ctx.divide(total_abs, total.copy_abs())


def relocation_model(o: np.ndarray, ns: np.ndarray):
    """fp64 arrays (x, factor, A) of the 50-digit model, each correctly rounded from it; every 37th row re-evaluated at 80 digits."""
    n_clamped = np.clip(np.asarray(ns, np.int64), 1, MAX_SAMPLES)
    rows = [_relocation_row(float(a), int(b), 50) for a, b in zip(o, n_clamped)]
    for i in range(0, len(rows), 37):
        x80, f80, _ = _relocation_row(float(o[i]), int(n_clamped[i]), 80)
        assert abs(rows[i][0] - x80) <= decimal.Decimal('1e-15') * x80 and abs(rows[i][1] - f80) <= decimal.Decimal('1e-15') * abs(f80), (i, rows[i], x80, f80)
    return tuple(np.array([float(r[j]) for r in rows]) for j in range(3))


@functools.lru_cache(maxsize=None)
def _relocation_truth():
    o, _, ns = relocation_inputs()
    return relocation_model(o, ns)


@functools.lru_cache(maxsize=None)
def _relocation_restatement(oracle):
    """The fp32 numpy restatement on relocation_inputs() and its own two figures against the model."""
    o, sc, ns = relocation_inputs()
    op32, sc32 = oracle.relocation_adjustment(o, sc, ns)
    return op32, sc32, _opacity_error(op32, _relocation_truth()), _factor_ratio(sc32, sc, _relocation_truth())


def _opacity_error(new_op, truth) -> float:
    return float(np.abs(np.asarray(new_op, np.float64).reshape(-1) - truth[0]).max())


def _factor_ratio(new_sc, old_sc, truth) -> float:
    """max_i relerr_i / u_i of new_scale / old_scale (the worst of the three columns) against the model's factor."""
    x, factor, cond = truth
    ratio = np.asarray(new_sc, np.float64) / np.asarray(old_sc, np.float64)
    rel = (np.abs(ratio - factor[:, None]) / np.abs(factor[:, None])).max(axis=1)
    return float((rel / (U * (1.0 / x + cond))).max())


def _relocate(be, device, o, sc, ns, ns_dtype=torch.int64):
    new_op, new_sc = be.relocation_adjustment(_t(o).reshape(-1, 1).to(device), _t(sc).to(device), _t(ns, ns_dtype).to(device))
    return new_op.cpu().numpy(), new_sc.cpu().numpy()


def check_relocation_against_model(be, oracle, device) -> dict:
    o, sc, ns = relocation_inputs()
    truth = _relocation_truth()
    _, _, e_oracle, r_oracle = _relocation_restatement(oracle)
    new_op, new_sc = _relocate(be, device, o, sc, ns)
    assert new_op.shape == (o.size, 1) and new_sc.shape == (o.size, 3)
    e_kernel, r_kernel = _opacity_error(new_op, truth), _factor_ratio(new_sc, sc, truth)
    figures = {'opacity_abs_err_kernel_in_2^-24': e_kernel / U, 'opacity_abs_err_restatement_in_2^-24': e_oracle / U, 'r_kernel': r_kernel, 'r_restatement': r_oracle}
    print('relocation_adjustment', device, figures)
    helpers.log_note('aux_three_way', f'{r_kernel:.3f}', op='relocation_scales', restatement=f'{r_oracle:.3f}', opacity_kernel=f'{e_kernel / U:.3f}', opacity_restatement=f'{e_oracle / U:.3f}')
    assert e_kernel <= 2.0 * e_oracle + U, figures
    assert r_oracle <= RELOCATION_CONDITION, figures
    assert r_kernel <= THREE_WAY * r_oracle, figures
    ratio = new_sc.astype(np.float64) / sc.astype(np.float64)
    assert np.isfinite(ratio).all() and (ratio > 0).all()
    # one fp32 factor times three scales, each product rounded once: the three quotients lie within 2^-24 of that factor, so within 2 x 2^-24 of each other
    assert ((ratio.max(axis=1) - ratio.min(axis=1)) <= 2.0 * U * ratio.max(axis=1) * (1.0 + 1e-6)).all()
    return figures


CLAMP_CASES = ((-3, 1), (0, 1), (1, 1), (50, 50), (51, 50), (10 ** 6, 50), (2 ** 40, 50), (2 ** 40 + 7, 50))


def check_relocation_clamp_and_dtypes(be, oracle, device) -> None:
    """Counts outside [1, 50] give, bit for bit, the result at the clamped value. The count is 64-bit and is clamped as such: the reference narrows it to int
    before clamping, by which 2^40 draws become 0 (1 after the clamp) and 2^40 + 7 become 7 -- an accident of the cast, not what clamp(n, 1, 50) is there for (oracle.py clips the
    int64). An int32 count tensor and a non-contiguous opacity view pass through the wrapper's conversions unchanged."""
    f = np.float32
    o = np.array([0.005, 0.03, 0.25, 0.5, 0.75, 0.97, 1.0 - 2.0 ** -12, 1.0 - U], f)
    sc = np.stack([o * f(0.01), o + f(1.0), f(3.0) - o], axis=1).astype(f)
    at = {n: _relocate(be, device, o, sc, np.full(o.size, n, np.int64)) for n in (1, 7, 50)}
    assert not np.array_equal(at[1][1], at[50][1]) and not np.array_equal(at[7][1], at[50][1]) and not np.array_equal(at[1][0], at[7][0])
    for n, clamped in CLAMP_CASES:
        got = _relocate(be, device, o, sc, np.full(o.size, n, np.int64))
        assert np.array_equal(got[0], at[clamped][0]) and np.array_equal(got[1], at[clamped][1]), (n, clamped)
    ns = np.array([1, 2, 7, 13, 29, 49, 50, 60], np.int64)
    plain = _relocate(be, device, o, sc, ns)
    as_int32 = _relocate(be, device, o, sc, ns, torch.int32)
    assert np.array_equal(plain[0], as_int32[0]) and np.array_equal(plain[1], as_int32[1])
    two_columns = torch.stack([_t(o), torch.full((o.size,), 0.123)], dim=1).to(device)
    view = two_columns[:, :1]
    assert not view.is_contiguous()
    strided = be.relocation_adjustment(view, _t(sc).to(device), _t(ns, torch.int64).to(device))
    assert np.array_equal(plain[0], strided[0].cpu().numpy()) and np.array_equal(plain[1], strided[1].cpu().numpy())


def check_relocation_saturated_opacity(be, oracle, device) -> dict:
    """o == 1.0 exactly (sigmoid of a logit of 17.3 or more in fp32): x = 1 and the alternating sum cancels from terms up to C(n, n/2). Up to n = 10 the kernel
    is held to the scales bar; beyond, the reference's arithmetic collapses (negative at n = 50) and the caller keeps o below 1 (harness/densify.py:_split_mass)."""
    ns = np.arange(1, 11, dtype=np.int64)
    o = np.ones(ns.size, np.float32)
    sc = np.stack([np.full(ns.size, 0.02), np.full(ns.size, 0.7), np.full(ns.size, 5.0)], axis=1).astype(np.float32)
    truth = relocation_model(o, ns)
    _, _, _, r_oracle = _relocation_restatement(oracle)
    new_op, new_sc = _relocate(be, device, o, sc, ns)
    assert np.array_equal(new_op.reshape(-1), o)                      # 1 - powf(0, 1 / n)
    r_kernel = _factor_ratio(new_sc, sc, truth)
    r_rows = _factor_ratio(oracle.relocation_adjustment(o, sc, ns)[1], sc, truth)
    figures = {'r_kernel_at_o=1': r_kernel, 'r_restatement_at_o=1': r_rows, 'r_restatement': r_oracle}
    print('relocation_adjustment o == 1', device, figures)
    helpers.log_note('aux_three_way', f'{r_kernel:.3f}', op='relocation_scales_o=1', restatement_same_rows=f'{r_rows:.3f}', restatement=f'{r_oracle:.3f}')
    assert r_kernel <= THREE_WAY * r_oracle, figures
    assert np.isfinite(new_sc).all() and (new_sc > 0).all()
    return figures


def _relocation_into_guarded_outputs(be, device, o, sc, ns):
    """fgs_relocation_adjustment as Backend.relocation_adjustment calls it, but into outputs this test allocated (the wrapper allocates exact-size ones)."""
    _, _backend = helpers.backend_modules()
    n = o.shape[0]
    op_d, sc_d = _padded(_t(o).reshape(-1, 1), device, 0.5), _padded(_t(sc), device, 1.0)
    ns_d = _padded(_t(ns, torch.int64), device, 3)
    be.relocation_adjustment(torch.full((1, 1), 0.5).to(device), torch.ones(1, 3).to(device), torch.ones(1, dtype=torch.int64).to(device))
    table = be._relocation_table[op_d.device]
    new_op, whole_op = guarded(torch.empty(n, 1), device)
    new_sc, whole_sc = guarded(torch.empty(n, 3), device)
    ptr = _backend._ptr
    be._check(be.lib.fgs_relocation_adjustment(ptr(op_d), ptr(sc_d), ptr(ns_d), table.data_ptr(), ptr(new_op), ptr(new_sc), n, _backend._stream_of(op_d.device)),
              'fgs_relocation_adjustment')
    return new_op.cpu().numpy(), new_sc.cpu().numpy(), guard_intact(whole_op, n) and guard_intact(whole_sc, n)


# ---- add_noise -------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noise_inputs():
    """(log-scales [1000, 3], quaternions [1000, 4], logits [1000, 1], noise [1000, 3], means [1000, 3]), all float32."""
    rng = np.random.default_rng(77)
    n = 1000
    s = rng.uniform(-12.0, 2.0, (n, 3))
    q = rng.standard_normal((n, 4))
    q *= np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (n, 1))) / np.linalg.norm(q, axis=1, keepdims=True)
    logit = rng.uniform(-8.0, 3.0, (n, 1))
    noise = rng.standard_normal((n, 3))
    means = rng.uniform(-5.0, 5.0, (n, 3))
    out = tuple(np.ascontiguousarray(a, np.float32) for a in (s, q, logit, noise, means))
    for a in out:
        a.setflags(write=False)
    return out


def noise_model(s, q, logit, noise, lr):
    """fp64: (displacement [N, 3], factor [N], max variance [N], sigma [N], updated [N] bool)."""
    s, q, logit, noise = (np.asarray(a, np.float64) for a in (s, q, logit, noise))
    var = np.exp(2.0 * s)
    r, x, y, z = q.T
    nsq = r * r + x * x + y * y + z * z
    updated = nsq >= 1e-8
    inv = 1.0 / np.where(updated, nsq, 1.0)
    R = np.stack([1 - 2 * (y * y + z * z) * inv, 2 * (x * y - r * z) * inv, 2 * (x * z + r * y) * inv,
                  2 * (x * y + r * z) * inv, 1 - 2 * (x * x + z * z) * inv, 2 * (y * z - r * x) * inv,
                  2 * (x * z - r * y) * inv, 2 * (y * z + r * x) * inv, 1 - 2 * (x * x + y * y) * inv], axis=1).reshape(-1, 3, 3)
    cov = np.einsum('nij,nj,nkj->nik', R, var, R)
    sigma = 1.0 / (1.0 + np.exp(-logit.reshape(-1)))
    factor = lr / (1.0 + np.exp(100.0 * sigma - 0.5))
    disp = factor[:, None] * np.einsum('nij,nj->ni', cov, noise)
    return np.where(updated[:, None], disp, 0.0), factor, var.max(axis=1), sigma, updated


@functools.lru_cache(maxsize=None)
def _noise_truth():
    s, q, logit, noise, _ = noise_inputs()
    return noise_model(s, q, logit, noise, NOISE_LR)


def _restated_displacement(oracle, s, q, logit, noise, lr):
    moved = np.zeros(noise.shape, np.float32)
    with np.errstate(over='ignore'):                      # expf(100 sigma - 0.5) overflows to +inf on the opaque rows: that is the reference's arithmetic
        oracle.add_noise(s, q, logit, noise, moved, lr)
    return moved


@functools.lru_cache(maxsize=None)
def _noise_restatement(oracle):
    s, q, logit, noise, _ = noise_inputs()
    moved = _restated_displacement(oracle, s, q, logit, noise, NOISE_LR)
    return moved, _displacement_ratio(moved, noise, _noise_truth())


def _displacement_ratio(moved, noise, truth) -> float:
    disp, factor, max_var, sigma, _ = truth
    rows = factor >= 1e-30
    err = np.abs(np.asarray(moved, np.float64) - disp).max(axis=1)
    e = err[rows] / (factor[rows] * max_var[rows] * np.linalg.norm(np.asarray(noise, np.float64)[rows], axis=1))
    return float((e / ((100.0 * sigma[rows] + 8.0) * U)).max())


def _add_noise(be, device, s, q, logit, noise, means, lr, n=None):
    """One in-place call on the first n rows; returns (means after [n, 3], guard rows intact)."""
    n = means.shape[0] if n is None else n
    args = [_padded(_t(a[:n]), device, fill) for a, fill in ((s, -1.0), (q, 0.5), (logit, -2.0), (noise, 1.0))]
    m, whole = guarded(_t(means[:n]), device)
    be.add_noise(*args, m, lr)
    return m.cpu().numpy(), guard_intact(whole, n)


def check_add_noise_against_model(be, oracle, device) -> dict:
    s, q, logit, noise, means = noise_inputs()
    truth = _noise_truth()
    disp, factor = truth[0], truth[1]
    _, r_oracle = _noise_restatement(oracle)
    moved, intact = _add_noise(be, device, s, q, logit, noise, np.zeros_like(means), NOISE_LR)       # from zero: the displacement itself
    assert intact
    r_kernel = _displacement_ratio(moved, noise, truth)
    tiny = factor < 1e-30
    figures = {'r_kernel': r_kernel, 'r_restatement': r_oracle, 'rows_relative': int((~tiny).sum()), 'rows_absolute': int(tiny.sum()),
               'max_abs_displacement_of_tiny_rows': float(np.abs(moved[tiny]).max())}
    print('add_noise', device, figures)
    helpers.log_note('aux_three_way', f'{r_kernel:.3f}', op='add_noise_displacement', restatement=f'{r_oracle:.3f}')
    assert (~tiny).sum() > 500 and tiny.sum() > 50 and (factor[tiny] > 0).all(), figures
    assert r_oracle <= NOISE_CONDITION, figures
    assert r_kernel <= THREE_WAY * r_oracle, figures
    assert np.abs(moved[tiny]).max() <= 1e-25, figures
    assert np.abs(disp).max() > 1.0                                                                 # the comparison is of something
    # in place on the real means: mean + displacement, to one ulp of the updated mean (the kernel's multiply-add may be fused, the sum below is not)
    after, intact = _add_noise(be, device, s, q, logit, noise, means, NOISE_LR)
    assert intact
    expected = (means + moved).astype(np.float32)
    assert (np.abs(after.astype(np.float64) - expected.astype(np.float64)) <= np.spacing(np.abs(expected)).astype(np.float64)).all()
    assert not np.array_equal(after, means)
    return figures


def check_add_noise_thresholds(be, oracle, device) -> None:
    """|q|^2 < 1e-8 leaves the mean alone (0 and 5e-9; 2e-8 is updated -- a factor 2 from the threshold on either side, the kernel's norm may be fused
    multiply-adds); so does an activated opacity above 0.892, where expf(100 sigma - 0.5) is +inf and the factor exactly 0."""
    f = np.float32
    q = np.zeros((6, 4), f)
    q[1, 0] = math.sqrt(5e-9)
    q[2] = math.sqrt(5e-9 / 4.0)
    q[3, 0] = math.sqrt(2e-8)
    q[4] = math.sqrt(2e-8 / 4.0) * np.array([1, -1, 1, -1])
    q[5] = (0.3, -0.1, 0.9, 0.2)
    nsq = (q.astype(np.float64) ** 2).sum(axis=1)
    assert (nsq[:3] < 0.51e-8).all() and (nsq[3:5] > 1.99e-8).all()
    s = np.tile(np.array([[-1.0, -2.0, 0.5]], f), (6, 1))
    logit = np.full((6, 1), -3.0, f)
    noise = np.tile(np.array([[0.7, -1.3, 0.4]], f), (6, 1))
    means = np.tile(np.array([[1.25, -3.5, 0.75]], f), (6, 1))
    after, intact = _add_noise(be, device, s, q, logit, noise, means, NOISE_LR)
    assert intact
    assert np.array_equal(after[:3], means[:3])
    truth = noise_model(s, q, logit, noise, NOISE_LR)
    assert (np.abs(truth[0][3:]).min(axis=1) > 1e-3).all()
    assert (np.abs(after[3:] - means[3:]).min(axis=1) > 1e-3).all()
    disp, factor, max_var, sigma, _ = (a[3:] for a in truth)
    bar = THREE_WAY * NOISE_CONDITION * (100.0 * sigma + 8.0) * U * factor * max_var * np.linalg.norm(noise[3:].astype(np.float64), axis=1)
    assert (np.abs(after[3:] - (means[3:] + disp)).max(axis=1) <= bar + np.spacing(np.abs(after[3:])).max(axis=1)).all()
    # opaque rows, on the backend and in the restatement
    logit = np.array([[2.2], [5.0], [20.0], [-3.0]], f)
    q, s, noise, means = (a[[5, 5, 5, 5]] for a in (q, s, noise, means))
    after, intact = _add_noise(be, device, s, q, logit, noise, means, NOISE_LR)
    assert intact and np.array_equal(after[:3], means[:3]) and not np.array_equal(after[3], means[3])
    restated = means.copy()
    with np.errstate(over='ignore'):
        oracle.add_noise(s, q, logit, noise, restated, NOISE_LR)
    assert np.array_equal(restated[:3], means[:3]) and not np.array_equal(restated[3], means[3])


# ---- update_3d_filter ------------------------------------------------------------------------------------------------------------------------------------
def filter_model(positions, w2c, filter_3d, mask, width, height, focal_x, focal_y, center_x, center_y, near_plane, clipping_tolerance, distance2filter,
                 dtype=np.float64) -> dict:
    """The operator in `dtype`: kept = on or inside all five planes; rewritten (and marked) = kept and the old filter is not below the new one."""
    d = dtype
    p, w = np.asarray(positions, d), np.asarray(w2c, d).reshape(-1)[:12]
    half_w, half_h = d(0.5) * d(width), d(0.5) * d(height)
    reach_x, reach_y = (d(clipping_tolerance) + d(0.5)) * d(width), (d(clipping_tolerance) + d(0.5)) * d(height)
    shift_x, shift_y = d(center_x) - half_w, d(center_y) - half_h
    bounds = {'left': (-reach_x - shift_x) / d(focal_x), 'right': (reach_x - shift_x) / d(focal_x),
              'top': (-reach_y - shift_y) / d(focal_y), 'bottom': (reach_y - shift_y) / d(focal_y)}
    row = lambda k: (w[4 * k] * p[:, 0] + w[4 * k + 1] * p[:, 1] + w[4 * k + 2] * p[:, 2]) + w[4 * k + 3]
    size = lambda k: np.abs(w[4 * k] * p[:, 0]) + np.abs(w[4 * k + 1] * p[:, 1]) + np.abs(w[4 * k + 2] * p[:, 2]) + np.abs(w[4 * k + 3])
    xc, yc, z = row(0), row(1), row(2)
    kept = (z >= d(near_plane)) & (xc >= bounds['left'] * z) & (xc <= bounds['right'] * z) & (yc >= bounds['top'] * z) & (yc <= bounds['bottom'] * z)
    new = d(distance2filter) * z
    old = np.asarray(filter_3d, d)
    rewritten = kept & (old >= new)
    # margins of the six comparisons over the magnitudes they compare (sums of absolute terms: a cancelling dot product carries its terms' rounding)
    margins = [np.abs(z - d(near_plane)) / (size(2) + abs(d(near_plane)))]
    for name, c, k in (('left', xc, 0), ('right', xc, 0), ('top', yc, 1), ('bottom', yc, 1)):
        margins.append(np.abs(c - bounds[name] * z) / (size(k) + abs(bounds[name]) * size(2)))
    margins.append(np.abs(old - new) / (np.abs(old) + abs(d(distance2filter)) * size(2)))
    return {'xc': xc, 'yc': yc, 'z': z, 'bounds': bounds, 'kept': kept, 'rewritten': rewritten, 'filter': np.where(rewritten, new, old),
            'mask': np.asarray(mask, bool) | rewritten, 'margin': np.min(margins, axis=0)}


def _run_filter(be, device, positions, w2c, filter_3d, mask, camera, n=None):
    """One call on the first n rows; returns (filter after, mask after, guard rows intact)."""
    n = positions.shape[0] if n is None else n
    pos = _padded(_t(positions[:n]), device, 0.0)
    filt, whole_f = guarded(_t(filter_3d[:n]), device)
    msk, whole_m = guarded(torch.from_numpy(np.array(mask[:n])), device, False)
    be.update_3d_filter(pos, _t(w2c).to(device), filt, msk, *camera)
    return filt.cpu().numpy(), msk.cpu().numpy(), guard_intact(whole_f, n) and guard_intact(whole_m, n, False)


EXACT_TRANSLATION = (0.5, -0.25, 1.0)
EXACT_PRINCIPAL_POINTS = ((64.0, 32.0), (80.0, 24.0))       # the middle of 128 x 64; 16 px right of it and 8 px above: left -1.75, right 1.25, top -0.625, bottom 0.875


def exact_camera(center_x, center_y):
    """(width, height, focal_x, focal_y, center_x, center_y, near, clipping tolerance, distance2filter): every bound a dyadic number."""
    return (128, 64, 64.0, 64.0, center_x, center_y, 0.25, 0.25, 0.125)


def _exact_w2c(translation=EXACT_TRANSLATION, from_behind=False) -> np.ndarray:
    w = np.eye(4, dtype=np.float32)
    if from_behind:                                        # half a turn about y: still only 0 and +-1
        w[0, 0] = w[2, 2] = -1.0
    w[:3, 3] = translation
    return w


def _stepped(value: float, offset: float, direction: int, factors=()) -> float:
    """The nearest float32 beyond `value` in `direction` whose world coordinate value - offset, and whose products with `factors`, are float32 numbers as
    well: one step of `value` where both coordinates lie in one binade, a power of two more where the world coordinate is the coarser of the two or a
    depth has to leave bits for the frustum's slopes."""
    step = float(np.spacing(np.float32(abs(value))))
    is_f32 = lambda a: float(np.float32(a)) == a
    for _ in range(6):
        v = value + direction * step
        if is_f32(v) and is_f32(v - offset) and all(is_f32(v * m) for m in factors):
            return v
        step *= 2.0
    raise AssertionError((value, offset))


def exact_filter_scene(center_x, center_y):
    """Points in camera coordinates ON each of the five planes and one step to either side, plus the filter comparison and the untouched cases.
    Returns (positions f32, filter f32, mask bool, kept labels, rewritten labels, names)."""
    width, height, fx, fy, cx, cy, near, tol, d2f = exact_camera(center_x, center_y)
    left, right = (-(tol + 0.5) * width - (cx - 0.5 * width)) / fx, ((tol + 0.5) * width - (cx - 0.5 * width)) / fx
    top, bottom = (-(tol + 0.5) * height - (cy - 0.5 * height)) / fy, ((tol + 0.5) * height - (cy - 0.5 * height)) / fy
    tx, ty, tz = EXACT_TRANSLATION
    rows = []

    def point(name, xc, yc, z, kept, old=1000.0, marked=False, rewritten=None):
        rows.append((name, (xc - tx, yc - ty, z - tz), old, marked, kept, kept if rewritten is None else rewritten))
    z0 = 2.0
    for name, bound, outward in (('left', left, -1), ('right', right, +1)):
        point(name + ' on', bound * z0, 0.0, z0, True)
        point(name + ' inside', _stepped(bound * z0, tx, -outward), 0.0, z0, True)
        point(name + ' outside', _stepped(bound * z0, tx, outward), 0.0, z0, False)
    for name, bound, outward in (('top', top, -1), ('bottom', bottom, +1)):
        point(name + ' on', 0.0, bound * z0, z0, True)
        point(name + ' inside', 0.0, _stepped(bound * z0, ty, -outward), z0, True)
        point(name + ' outside', 0.0, _stepped(bound * z0, ty, outward), z0, False)
    point('near on', 0.0, 0.0, near, True)
    point('near inside', 0.0, 0.0, _stepped(near, tz, +1, (left, right, top, bottom, d2f)), True)
    point('near outside', 0.0, 0.0, _stepped(near, tz, -1, (left, right, top, bottom, d2f)), False)
    point('corner of the right, bottom and near planes', right * near, bottom * near, near, True)
    new = d2f * z0
    point('filter equal', 0.0, 0.0, z0, True, old=new)                                               # rewritten (to the same value) and marked
    point('filter one step above', 0.0, 0.0, z0, True, old=float(np.nextafter(np.float32(new), np.float32(1.0))))
    point('filter one step below', 0.0, 0.0, z0, True, old=float(np.nextafter(np.float32(new), np.float32(0.0))), rewritten=False)
    point('filter far below', 0.25, -0.125, z0, True, old=2.0 ** -13, rewritten=False)
    point('outside, marked by an earlier view', 10.0, 0.0, z0, False, old=0.75, marked=True)
    point('behind the camera, marked by an earlier view', 0.0, 0.0, -1.0, False, old=0.375, marked=True)
    point('inside, marked by an earlier view, filter below', 0.0, 0.0, z0, True, old=2.0 ** -13, marked=True, rewritten=False)
    names = [r[0] for r in rows]
    positions = np.array([r[1] for r in rows], np.float32)
    assert np.array_equal(positions.astype(np.float64), np.array([r[1] for r in rows], np.float64)), 'every coordinate is a float32'
    return (positions, np.array([r[2] for r in rows], np.float32), np.array([r[3] for r in rows], bool), np.array([r[4] for r in rows], bool),
            np.array([r[5] for r in rows], bool), names)


def check_filter_exact_boundaries(be, oracle, device, principal_point) -> None:
    camera = exact_camera(*principal_point)
    positions, old, marked, kept, rewritten, names = exact_filter_scene(*principal_point)
    w2c = _exact_w2c()
    m64 = filter_model(positions, w2c, old, marked, *camera, dtype=np.float64)
    m32 = filter_model(positions, w2c, old, marked, *camera, dtype=np.float32)
    for k in ('xc', 'yc', 'z'):                                         # exact in both formats: no contraction or ordering of the fp32 kernel can move a decision
        assert m32[k].dtype == np.float32 and np.array_equal(m32[k].astype(np.float64), m64[k]), k
    for k, v in m64['bounds'].items():
        assert float(m32['bounds'][k]) == float(v), k
    for k in ('left', 'right', 'top', 'bottom'):
        assert np.array_equal((m32['bounds'][k] * m32['z']).astype(np.float64), m64['bounds'][k] * m64['z']), k
    assert np.array_equal((np.float32(camera[8]) * m32['z']).astype(np.float64), camera[8] * m64['z'])
    # the labels written beside the points, the model, and the numpy restatement agree ...
    assert np.array_equal(m64['kept'], kept), [n for n, a, b in zip(names, m64['kept'], kept) if a != b]
    assert np.array_equal(m64['rewritten'], rewritten), [n for n, a, b in zip(names, m64['rewritten'], rewritten) if a != b]
    f_ref, m_ref = old.copy(), marked.copy()
    oracle.update_3d_filter(positions, w2c, f_ref, m_ref, *camera)
    assert np.array_equal(f_ref.astype(np.float64), m64['filter']) and np.array_equal(m_ref, m64['mask'])
    # ... and so does the backend, bit for bit
    f_d, m_d, intact = _run_filter(be, device, positions, w2c, old, marked, camera)
    assert intact
    wrong = [n for n, a, b in zip(names, m_d, marked | rewritten) if a != b]
    assert not wrong, ('mask', wrong)
    expected = np.where(rewritten, np.float32(camera[8]) * m32['z'], old).astype(np.float32)
    wrong = [n for n, a, b in zip(names, f_d, expected) if a.tobytes() != b.tobytes()]
    assert not wrong, ('filter', wrong)
    assert np.array_equal(f_d[~rewritten].view(np.uint32), old[~rewritten].view(np.uint32))           # untouched: the same bits


def check_filter_two_views(be, oracle, device) -> None:
    """Two views one after the other, in either order, leave the smaller of the two filter values; a point only one view sees gets that view's."""
    camera = exact_camera(*EXACT_PRINCIPAL_POINTS[0])
    grid = np.array([(x, y, z) for x in (-0.5, 0.0, 0.5) for y in (-0.25, 0.25) for z in (0.0, 0.5, 1.0)] + [(-0.5, 0.25, 1.875), (-0.5, 0.25, -0.875)], np.float32)
    views = (_exact_w2c((0.5, -0.25, 1.0)), _exact_w2c((0.0, 0.0, 2.0), from_behind=True))      # depths pz + 1 and 2 - pz
    old, marked = np.full(grid.shape[0], 1000.0, np.float32), np.zeros(grid.shape[0], bool)
    each = [filter_model(grid, w, old, marked, *camera) for w in views]
    both = np.arange(grid.shape[0]) < 18
    assert np.array_equal(each[0]['kept'], both | (np.arange(20) == 18)) and np.array_equal(each[1]['kept'], both | (np.arange(20) == 19))
    assert (each[0]['filter'][both] < each[1]['filter'][both]).any() and (each[1]['filter'][both] < each[0]['filter'][both]).any()
    smallest = np.minimum(each[0]['filter'], each[1]['filter'])
    assert (smallest < 1000.0).all() and np.array_equal(smallest.astype(np.float32).astype(np.float64), smallest)
    for order in ((0, 1), (1, 0)):
        f, m = old, marked
        for v in order:
            f, m, intact = _run_filter(be, device, grid, views[v], f, m, camera)
            assert intact
        assert np.array_equal(f.astype(np.float64), smallest) and m.all(), order


RANDOM_CAMERA = (128, 96, 100.0, 110.0, 60.0, 50.0, 0.2, 0.15, 0.2 ** 0.5 / 100.0)
RISK_BAND = 16.0 * U
RISK_CAP = 0.01


@functools.lru_cache(maxsize=None)
def random_filter_scene():
    """(positions [1000, 3], w2c [4, 4], filter [1000], mask [1000]) under a rotated camera; a third of the filters sit around the new value."""
    rng = np.random.default_rng(5)
    n = 1000
    q = np.array([0.8, 0.3, -0.4, 0.2])
    q /= np.linalg.norm(q)
    r, x, y, z = q
    w2c = np.eye(4)
    w2c[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                   [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]]
    w2c[:3, 3] = (0.3, -0.2, 3.0)
    w2c = w2c.astype(np.float32)
    positions = rng.uniform(-4.0, 4.0, (n, 3)).astype(np.float32)
    depth = positions.astype(np.float64) @ w2c[2, :3].astype(np.float64) + float(w2c[2, 3])
    kind = rng.integers(0, 3, n)
    old = np.where(kind == 0, 1000.0, np.where(kind == 1, 1e-4, RANDOM_CAMERA[8] * np.abs(depth) * (1.0 + 0.1 * rng.standard_normal(n)))).astype(np.float32)
    marked = rng.random(n) < 0.1
    for a in (positions, w2c, old, marked):
        a.setflags(write=False)
    return positions, w2c, old, marked


def check_filter_random_scene(be, oracle, device) -> dict:
    positions, w2c, old, marked = random_filter_scene()
    model = filter_model(positions, w2c, old, marked, *RANDOM_CAMERA)
    risky = model['margin'] < RISK_BAND
    figures = {'risky_share': float(risky.mean()), 'kept': int(model['kept'].sum()), 'rewritten': int(model['rewritten'].sum())}
    assert figures['risky_share'] <= RISK_CAP, figures
    assert 100 < figures['rewritten'] < figures['kept'] < 900, figures                  # every branch is taken by many points
    f_d, m_d, intact = _run_filter(be, device, positions, w2c, old, marked, RANDOM_CAMERA)
    assert intact
    keep = ~risky
    figures['filter_rel_err'] = float((np.abs(f_d.astype(np.float64) - model['filter']) / np.abs(model['filter']))[keep].max())
    print('update_3d_filter', device, figures)
    helpers.log_note('aux_filter_random', f'{figures["filter_rel_err"]:.3e}', risky_share=f'{figures["risky_share"]:.4f}')
    assert np.array_equal(m_d[keep], model['mask'][keep]), int((m_d[keep] != model['mask'][keep]).sum())
    assert figures['filter_rel_err'] <= 1e-6, figures
    untouched = keep & ~model['rewritten']
    assert np.array_equal(f_d[untouched].view(np.uint32), old[untouched].view(np.uint32))
    return figures


# ---- every operator at every row count -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _full_runs(be, device):
    """Each operator once on all its rows through the plain calls: what the first N rows of a shorter call must reproduce bit for bit (one lane per row)."""
    o, sc, ns = relocation_inputs()
    s, q, logit, noise, means = noise_inputs()
    positions, w2c, old, marked = random_filter_scene()
    return {'relocation': _relocate(be, device, o, sc, ns), 'noise': _add_noise(be, device, s, q, logit, noise, means, NOISE_LR)[0],
            'filter': _run_filter(be, device, positions, w2c, old, marked, RANDOM_CAMERA)[:2]}


def check_row_counts(be, oracle, device, n: int) -> None:
    """N rows (0, 1, one short of a 256-thread workgroup, exactly one, one more, four with a ragged last): the results are the first N rows of the full runs
    held to the models above, and nothing is written behind row N."""
    full = _full_runs(be, device)
    o, sc, ns = relocation_inputs()
    new_op, new_sc, intact = _relocation_into_guarded_outputs(be, device, o[:n], sc[:n], ns[:n])
    assert intact, 'relocation_adjustment wrote behind row N'
    assert new_op.shape == (n, 1) and np.array_equal(new_op, full['relocation'][0][:n]) and np.array_equal(new_sc, full['relocation'][1][:n])
    via_wrapper = _relocate(be, device, o[:n], sc[:n], ns[:n])
    assert via_wrapper[0].shape == (n, 1) and via_wrapper[1].shape == (n, 3) and np.array_equal(via_wrapper[0], new_op) and np.array_equal(via_wrapper[1], new_sc)
    s, q, logit, noise, means = noise_inputs()
    after, intact = _add_noise(be, device, s, q, logit, noise, means, NOISE_LR, n)
    assert intact, 'add_noise wrote behind row N'
    assert np.array_equal(after, full['noise'][:n])
    positions, w2c, old, marked = random_filter_scene()
    f_d, m_d, intact = _run_filter(be, device, positions, w2c, old, marked, RANDOM_CAMERA, n)
    assert intact, 'update_3d_filter wrote behind row N'
    assert np.array_equal(f_d, full['filter'][0][:n]) and np.array_equal(m_d, full['filter'][1][:n])


def check_public_add_noise(be, device, seed: int = 1234) -> None:
    """FasterGSCudaBackend.add_noise draws torch.randn_like(means) itself (the reference's densification.py:20): the same seed and the backend call give the same bits."""
    import FasterGSCudaBackend as B
    s, q, logit, _, means = (_t(a).to(device) for a in noise_inputs())
    public, direct = means.clone(), means.clone()
    torch.manual_seed(seed)
    B.add_noise(s, q, logit, public, NOISE_LR)
    torch.manual_seed(seed)
    be.add_noise(s, q, logit, torch.randn_like(direct), direct, NOISE_LR)
    assert torch.equal(public, direct) and not torch.equal(public, means)
