"""Shapes and checks shared by tests/test_glue.py (CPU simulation) and tests/test_gpu_glue.py (MI355X): the validation branches and the call forms of the
torch glue (FasterGSCudaBackend/_backend.py), pinned at the smallest shapes at which its shared helpers can go wrong.

N = 65 (make_s0(seed=3, n=65)): two blocks of 64 Gaussians, the second holding one, so ceil(N / 64) = 2 and N // 64 = 1; the 48 x 36 view of the tiny_aa
fixture (partial tiles, proper antialiasing, coloured background); 16 SH bases (15 rest coefficients), 1 base ([N, 0, 3]) and a 1-D empty
sh_coefficients_rest, which is the branch of the rest-coefficient count that does not read shape[1].

Refusals: every literal below is the message the glue raises, copied from it. A refused call launches nothing: every tensor the call could have written
keeps its sentinel fill. Accepted: what the sharded and fused paths let through today stays let through (they take densification_info as it comes).
Identities: two call forms of one computation give the same bytes. The simulation is deterministic (two backward passes over the same inputs are
byte-identical, checked first), so gradients are compared with torch.equal there; on hardware K11's float atomics make two backward passes differ in the
last bits, and two passes are compared at 1e-5 of the tensor's max-abs value, the bar tests/k12_fold_cases.py and tests/test_reached_blocks.py use for
that pair. The loss and the forward-only render are deterministic on both and compared bit for bit."""
from __future__ import annotations

import functools
import re
from types import SimpleNamespace

import pytest
import torch

import helpers
from harness.scenes import View, make_s0
from unreached_cases import LRS, ORDER

N, BLOCKS = 65, 2
KINDS = ('k16', 'k1', 'flat')
FORM_TOL = 1e-5
SENTINEL, FLAG_SENTINEL = 7.0, 9
FIVE = ('means', 'scales', 'rotations', 'opacities', 'sh_coefficients_rest')

FLAGS_MESSAGE = "{} must be a contiguous uint8 tensor of ceil(N / 64) elements on the parameters' device"
QUIET_SCAN_MESSAGE = "quiet_blocks must be a contiguous uint8 tensor of ceil(N / 64) elements on the moments' device"
GRADIENT_MESSAGE = 'preallocated gradient has shape {}, expected contiguous float32 {}'
SHARD_GRADIENT_MESSAGE = 'preallocated gradient has shape {}, expected {}'
DENSIFICATION_MESSAGE = "densification_info must be a contiguous float32 [2, N] tensor on the parameters' device"
ACC_RECORDS_MESSAGE = 'acc_records must be contiguous float32 [sum(n_visible), 9] and n_visible one entry per view'
RECORDS_MESSAGE = 'records must be a contiguous uint8 tensor of n_records * 56 bytes'
SHARD_RECORDS_MESSAGE = "records must be uint8 [views, N, 56] and counts int32 [views, 2] on the parameters' device"
ACCUMULATOR_MESSAGE = 'accumulator records must be contiguous float32 [n_records, 9]'
ROWS_MESSAGE = 'live_blocks / quiet_blocks need parameter tensors that all have one row per Gaussian'
SCAN_ROWS_MESSAGE = 'adam_quiet_scan needs moment tensors that all have one row per Gaussian'


def parameter_message(name: str, device) -> str:
    return f"Input tensor '{name}' must be a contiguous float32 tensor on {device}."


def refused(message: str, kind=RuntimeError):
    return pytest.raises(kind, match='^' + re.escape(message) + '$')


@functools.lru_cache(maxsize=None)
def scene(kind: str):
    K = 16 if kind == 'k16' else 1
    p, v = make_s0(seed=3, n=N, sh_bases=K)
    if kind == 'flat':
        p['sh_coefficients_rest'] = torch.empty(0)
    view = View(v.w2c, v.position, 48, 36, 40.0, 40.0, 24.0, 18.0, 0.2, 1e4, torch.tensor([0.2, 0.5, 0.7]))
    gi = torch.randn(3, 36, 48, generator=torch.Generator().manual_seed(5))
    return {k: t.contiguous() for k, t in p.items()}, view, K, gi


def shapes_of(kind: str) -> tuple:
    rest = 15 if kind == 'k16' else 0
    return ((N, 3), (N, 3), (N, 4), (N, 1), (N, 1, 3), (N, rest, 3))


_PASSES: dict = {}


def forward_pass(be, device: str, kind: str = 'k16') -> SimpleNamespace:
    """One forward pass per backend, device and kind, shared by every check (nothing in it is written again)."""
    key = (id(be), device, kind)
    if key not in _PASSES:
        params, view, K, gi = scene(kind)
        _, RS = helpers.settings_pair(view, K, True, device=device)
        dp = {k: t.to(device) for k, t in params.items()}
        res = be.forward(*[dp[k] for k in helpers.NAMES], RS)
        _PASSES[key] = SimpleNamespace(dp=dp, six=[dp[k] for k in helpers.NAMES], five=[dp[k] for k in FIVE], RS=RS, res=res, gi=gi.to(device),
                                       shapes=shapes_of(kind), device=dp['means'].device)
    return _PASSES[key]


def backward_of(be, s: SimpleNamespace, dens=None, **kwargs) -> tuple:
    return be.backward(dens, s.gi, s.res.image, *s.five, s.res.buffers, s.RS, s.res.state, **kwargs)


def backward_aux_of(be, s: SimpleNamespace, dens=None, grad_alpha=None, grad_depth=None, depth=None, **kwargs) -> tuple:
    return be.backward_aux(dens, s.gi, grad_alpha, grad_depth, s.res.image, depth, *s.five, s.res.buffers, s.RS, s.res.state, **kwargs)


def sentinel_gradients(s: SimpleNamespace) -> list:
    return [torch.full(sh, SENTINEL, dtype=torch.float32, device=s.device) for sh in s.shapes]


def untouched(*tensors) -> bool:
    return all(bool((t == (SENTINEL if t.is_floating_point() else FLAG_SENTINEL)).all()) for t in tensors if t is not None and t.numel())


def same_gradients(a, b, exact: bool, what) -> None:
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape, (what, i)
        if exact:
            assert torch.equal(x, y), (what, i)
        elif x.numel():
            assert helpers.rel_inf(x.cpu().numpy(), y.cpu().numpy()) < FORM_TOL, (what, i)


def bad_flags(device, other_device=None) -> dict:
    """The refused forms of a block-flag array: wrong dtype, ceil(N / 64) - 1 elements, not contiguous; on hardware also one on the host."""
    bad = {'dtype': torch.full((BLOCKS,), FLAG_SENTINEL, dtype=torch.int8, device=device),
           'length': torch.full((BLOCKS - 1,), FLAG_SENTINEL, dtype=torch.uint8, device=device),
           'strided': torch.full((2 * BLOCKS,), FLAG_SENTINEL, dtype=torch.uint8, device=device)[::2]}
    if other_device is not None:
        bad['device'] = torch.full((BLOCKS,), FLAG_SENTINEL, dtype=torch.uint8, device=other_device)
    return bad


def adam_state(device, seed: int = 3):
    gen = torch.Generator().manual_seed(seed)
    row = {'means': (3,), 'sh_coefficients_0': (1, 3), 'sh_coefficients_rest': (15, 3), 'opacities': (1,), 'scales': (3,), 'rotations': (4,)}
    make = lambda scale: [(torch.randn((N,) + row[k], generator=gen) * scale).to(device) for k in ORDER]
    return make(1e-2), make(1.0), make(1e-3), [t.abs() * 1e-3 + 1e-7 for t in make(1e-3)]


# ---- 1. refusals ----------------------------------------------------------------------------------------------------------------------------------
def check_parameter_refusals(be, device: str) -> None:
    """The six-, five- and eighteen-tensor parameter checks of every method that carries one: a float64 `means`, a strided sh_coefficients_rest."""
    s = forward_pass(be, device)
    dev = s.device
    wrong = dict(s.dp, means=s.dp['means'].double())
    strided = dict(s.dp, sh_coefficients_rest=torch.zeros((N, 15, 6), device=dev)[:, :, ::2])
    records = torch.full((1, N, 56), FLAG_SENTINEL, dtype=torch.uint8, device=dev)
    counts = torch.full((1, 2), 5, dtype=torch.int32, device=dev)
    scores = torch.full((N,), SENTINEL, device=dev)
    for dp, name in ((wrong, 'means'), (strided, 'sh_coefficients_rest')):
        six, five = [dp[k] for k in helpers.NAMES], [dp[k] for k in FIVE]
        message = parameter_message(name, dev)
        for call in (lambda: be.forward(*six, s.RS), lambda: be.forward_aux(*six, s.RS), lambda: be.inference(*six, s.RS, True, True),
                     lambda: be.inference_aux(*six, s.RS, True, True), lambda: be.pruning_scores(scores, *six, s.RS),
                     lambda: be.shard_preprocess(*six, [s.RS], records, counts)):
            with refused(message):
                call()
        out, dens = sentinel_gradients(s), torch.full((2, N), SENTINEL, device=dev)
        with refused(message):
            be.backward(dens, s.gi, s.res.image, *five, s.res.buffers, s.RS, s.res.state, out=tuple(out))
        with refused(message):
            be.backward_aux(dens, s.gi, torch.ones(36, 48, device=dev), None, s.res.image, None, *five, s.res.buffers, s.RS, s.res.state, out=tuple(out))
        with refused(message):
            be.shard_backward(torch.zeros((N, 9), device=dev), [N], s.res.buffers[0], dens, *five, [s.RS], tuple(out))
        assert untouched(*out, dens, records, scores) and bool((counts == 5).all())
    params = [s.dp[k] for k in ORDER]
    moments, second = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    before = [p.clone() for p in params]
    bad_moments = [moments[0].double()] + moments[1:]
    with refused(parameter_message('param/moment', dev)):
        be.backward_adam_fused(None, s.gi, s.res.image, params, bad_moments, second, s.res.buffers, s.RS, s.res.state, 1, LRS)
    with refused(parameter_message('param/moment', dev)):
        be.shard_backward_adam_fused(torch.zeros((N, 9), device=dev), [N], s.res.buffers[0], None, params, bad_moments, second, [s.RS], 1, LRS)
    assert all(torch.equal(a, b) for a, b in zip(before, params)) and all(not bool(t.any()) for t in moments + second)


def check_block_flag_refusals(be, device: str, other_device=None) -> None:
    """live_blocks / reached_blocks of backward and backward_aux, live_blocks / quiet_blocks of adam_step_multi, `out` of adam_quiet_scan."""
    s = forward_pass(be, device)
    dev = s.device
    alpha = torch.ones(36, 48, device=dev)
    for name in ('live_blocks', 'reached_blocks'):
        for why, flags in bad_flags(dev, other_device).items():
            good = torch.full((BLOCKS,), FLAG_SENTINEL, dtype=torch.uint8, device=dev)
            kwargs = {'live_blocks': good, 'reached_blocks': good, name: flags}
            for run in (lambda **kw: backward_of(be, s, dens, **kw), lambda **kw: backward_aux_of(be, s, dens, grad_alpha=alpha, **kw)):
                out, dens = sentinel_gradients(s), torch.full((2, N), SENTINEL, device=dev)
                with refused(FLAGS_MESSAGE.format(name)):
                    run(out=tuple(out), **kwargs)
                assert untouched(*out, dens, good, flags), (name, why)
    grads, params, m, v = adam_state(dev)
    before = [t.clone() for t in params + m + v]
    for name in ('live_blocks', 'quiet_blocks'):
        for why, flags in bad_flags(dev, other_device).items():
            good = torch.full((BLOCKS,), FLAG_SENTINEL, dtype=torch.uint8, device=dev)
            with refused(FLAGS_MESSAGE.format(name)):
                be.adam_step_multi(grads, params, m, v, [1] * 6, LRS, 0.9, 0.999, 1e-15, **{'live_blocks': good, 'quiet_blocks': good, name: flags})
            assert untouched(good, flags), (name, why)
    with refused(ROWS_MESSAGE):
        be.adam_step_multi(grads[:1] + [grads[1][:64]], params[:1] + [params[1][:64]], m[:1] + [m[1][:64]], v[:1] + [v[1][:64]], [1] * 2, LRS[:2], 0.9, 0.999,
                           1e-15, live_blocks=torch.ones(BLOCKS, dtype=torch.uint8, device=dev))
    for why, flags in bad_flags(dev, other_device).items():
        with refused(QUIET_SCAN_MESSAGE):
            be.adam_quiet_scan(m, v, out=flags)
        assert untouched(flags), why
    with refused(SCAN_ROWS_MESSAGE):
        be.adam_quiet_scan(m[:1] + [m[1][:64]], v[:1] + [v[1][:64]])
    assert all(torch.equal(a, b) for a, b in zip(before, params + m + v))


def check_gradient_and_densification_refusals(be, device: str, other_device=None) -> None:
    """`out` with one gradient of the wrong shape (dtype, stride, device) and a densification_info of 2 N - 1 elements."""
    s = forward_pass(be, device)
    dev = s.device
    alpha = torch.ones(36, 48, device=dev)
    runs = (lambda **kw: backward_of(be, s, **kw), lambda **kw: backward_aux_of(be, s, grad_alpha=alpha, **kw))
    bad = {'shape': (2, torch.full((N, 3), SENTINEL, device=dev)),
           'dtype': (3, torch.full((N, 1), SENTINEL, dtype=torch.float64, device=dev)),
           'strided': (5, torch.full((N, 15, 6), SENTINEL, device=dev)[:, :, ::2])}
    if other_device is not None:
        bad['device'] = (0, torch.full((N, 3), SENTINEL, device=other_device))
    for why, (i, g) in bad.items():
        for run in runs:
            out, dens = sentinel_gradients(s), torch.full((2, N), SENTINEL, device=dev)
            out[i] = g
            with refused(GRADIENT_MESSAGE.format(tuple(g.shape), s.shapes[i])):
                run(dens=dens, out=tuple(out))
            assert untouched(*out, dens), why
    for run in runs:
        out, dens = sentinel_gradients(s), torch.full((2 * N - 1,), SENTINEL, device=dev)
        with refused(DENSIFICATION_MESSAGE):
            run(dens=dens, out=tuple(out))
        assert untouched(*out, dens)
    # the sharded owner pass: shapes by its own check, everything else by the parameter check in front of it
    out, dens = sentinel_gradients(s), torch.full((2, N), SENTINEL, device=dev)
    out[2] = bad['shape'][1]
    with refused(SHARD_GRADIENT_MESSAGE.format((N, 3), (N, 4))):
        be.shard_backward(torch.zeros((N, 9), device=dev), [N], s.res.buffers[0], dens, *s.five, [s.RS], tuple(out))
    out[2], out[5] = torch.full((N, 4), SENTINEL, device=dev), bad['strided'][1]
    with refused(parameter_message('grad', dev)):
        be.shard_backward(torch.zeros((N, 9), device=dev), [N], s.res.buffers[0], dens, *s.five, [s.RS], tuple(out))
    assert untouched(*out, dens)


def sharded_pass(be, device: str) -> SimpleNamespace:
    """The record path of one owner and one view over the same scene: preprocess, render from the records, K11 to accumulator records."""
    key = (id(be), device, 'sharded')
    if key not in _PASSES:
        s = forward_pass(be, device)
        records = torch.zeros((1, N, 56), dtype=torch.uint8, device=s.device)
        counts = torch.zeros((1, 2), dtype=torch.int32, device=s.device)
        prim = be.shard_preprocess(*s.six, [s.RS], records, counts)
        n_visible, n_instances = (int(c) for c in counts[0].cpu())
        assert 0 < n_visible <= N
        res = be.forward_from_records(records.view(-1), n_visible, n_instances, s.RS, 15)
        acc = be.backward_to_records(s.gi, res.image, res.buffers, s.RS, res.state, 15)
        _PASSES[key] = SimpleNamespace(records=records, prim=prim, n_visible=n_visible, n_instances=n_instances, res=res, acc=acc)
    return _PASSES[key]


def check_record_refusals(be, device: str) -> None:
    """records one record short, acc_records one row short, n_visible of the wrong length, an accumulator of the wrong size."""
    s, r = forward_pass(be, device), sharded_pass(be, device)
    dev = s.device
    counts = torch.full((1, 2), 5, dtype=torch.int32, device=dev)
    short = torch.full((N * 56 - 56,), FLAG_SENTINEL, dtype=torch.uint8, device=dev)
    with refused(SHARD_RECORDS_MESSAGE):
        be.shard_preprocess(*s.six, [s.RS], short, counts)
    with refused(SHARD_RECORDS_MESSAGE):
        be.shard_preprocess(*s.six, [s.RS], torch.full((1, N, 56), FLAG_SENTINEL, dtype=torch.uint8, device=dev), counts[0, :1])
    assert untouched(short) and bool((counts == 5).all())
    with refused(RECORDS_MESSAGE):
        be.forward_from_records(r.records.view(-1)[:r.n_visible * 56 - 56], r.n_visible, r.n_instances, s.RS, 15)
    with refused(RECORDS_MESSAGE):
        be.forward_from_records(r.records.view(-1).to(torch.int8), r.n_visible, r.n_instances, s.RS, 15)
    acc = torch.full((r.n_visible - 1, 9), SENTINEL, device=dev)
    with refused(ACCUMULATOR_MESSAGE):
        be.backward_to_records(s.gi, r.res.image, r.res.buffers, s.RS, r.res.state, 15, out=acc)
    assert untouched(acc)
    params = [s.dp[k].clone() for k in ORDER]
    moments, second = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    for acc_records, n_visible in ((r.acc[:-1], [r.n_visible]), (r.acc, [r.n_visible, 0]), (r.acc, []), (r.acc.double(), [r.n_visible]),
                                   (torch.zeros((r.n_visible, 18), device=dev)[:, ::2], [r.n_visible])):
        out, dens = sentinel_gradients(s), torch.full((2, N), SENTINEL, device=dev)
        with refused(ACC_RECORDS_MESSAGE):
            be.shard_backward(acc_records, n_visible, r.prim, dens, *s.five, [s.RS], tuple(out))
        with refused(ACC_RECORDS_MESSAGE):
            be.shard_backward_adam_fused(acc_records, n_visible, r.prim, dens, params, moments, second, [s.RS], 1, LRS)
        assert untouched(*out, dens)
    assert all(torch.equal(p, s.dp[k]) for p, k in zip(params, ORDER)) and all(not bool(t.any()) for t in moments + second)


# ---- 2. accepted where it was accepted --------------------------------------------------------------------------------------------------------------
def check_accepted_forms(be, device: str) -> None:
    """The sharded owner pass and the fused paths take densification_info unvalidated: 2 N + 1 floats (the kernels write the first 2 N) pass, and give
    what a [2, N] tensor gives. shard_backward hands back the very `out` it was given, a list included. None and an empty tensor mean "no statistics"."""
    s, r = forward_pass(be, device), sharded_pass(be, device)
    dev, exact = s.device, device == 'cpu'
    odd, even = torch.zeros(2 * N + 1, device=dev), torch.zeros((2, N), device=dev)
    with refused(DENSIFICATION_MESSAGE):
        backward_of(be, s, dens=odd)
    outs = []
    for dens in (odd, even):
        out = [torch.empty(sh, device=dev) for sh in s.shapes]
        assert be.shard_backward(r.acc, [r.n_visible], r.prim, dens, *s.five, [s.RS], out) is out
        outs.append(out)
    same_gradients(outs[0] + [odd[:2 * N]], outs[1] + [even.view(-1)], exact, 'shard_backward, densification_info of 2 N + 1 elements')
    assert float(odd[2 * N]) == 0.0 and bool(even.any())
    for fused in (lambda d, p, m, v: be.backward_adam_fused(d, s.gi, s.res.image, p, m, v, s.res.buffers, s.RS, s.res.state, 1, LRS),
                  lambda d, p, m, v: be.shard_backward_adam_fused(r.acc, [r.n_visible], r.prim, d, p, m, v, [s.RS], 1, LRS)):
        states = []
        for dens in (torch.zeros(2 * N + 1, device=dev), torch.zeros((2, N), device=dev), None, torch.empty(0, device=dev)):
            params = [s.dp[k].clone() for k in ORDER]          # seeded moments: helpers.seeded_moments says why two passes are not compared from zero
            moments, second = zip(*[[t.to(dev) for t in helpers.seeded_moments(p.shape, 5 + i)] for i, p in enumerate(params)])
            fused(dens, params, list(moments), list(second))
            states.append(params + list(moments) + list(second))
            assert not torch.equal(params[0], s.dp['means'])
            if dens is not None and dens.numel() > 2 * N:
                assert bool(dens[:2 * N].any()) and float(dens[2 * N]) == 0.0
        for state in states[1:]:
            same_gradients(state, states[0], exact, 'fused step, another form of densification_info')
    plain = backward_of(be, s, dens=torch.zeros((2, N), device=dev))
    for nothing in (None, torch.empty(0, device=dev)):
        same_gradients(backward_of(be, s, dens=nothing), plain, exact, 'backward without statistics')


# ---- 3. bit-for-bit identities ----------------------------------------------------------------------------------------------------------------------
def check_backward_forms(be, device: str, kind: str) -> None:
    """backward twice (the premise), backward_aux without map gradients == backward, backward(out=views of one arena) == backward into fresh tensors:
    the six gradients and densification_info."""
    from FasterGSCudaBackend import rasterization
    s = forward_pass(be, device, kind)
    exact = device == 'cpu'
    runs = {}
    for name in ('backward', 'again', 'aux', 'views'):
        dens = torch.zeros((2, N), device=s.device)
        if name == 'aux':
            grads = backward_aux_of(be, s, dens)
        elif name == 'views':
            arena, views = rasterization._gradient_arena(s.shapes, s.device)
            arena.fill_(SENTINEL)
            grads = backward_of(be, s, dens, out=views)
            assert all(g is v for g, v in zip(grads, views))
        else:
            grads = backward_of(be, s, dens)
        assert tuple(tuple(g.shape) for g in grads) == s.shapes and all(g.dtype == torch.float32 and g.is_contiguous() for g in grads)
        runs[name] = tuple(grads) + (dens,)
    assert bool(runs['backward'][0].any()) and bool(runs['backward'][6].any())
    for name in ('again', 'aux', 'views'):
        same_gradients(runs[name], runs['backward'], exact, (kind, name))


def check_loss_and_inference_forms(be, device: str, kind: str) -> None:
    """l1_dssim(with_grad=False) == l1_dssim_forward in the loss and the (l1, ssim) pair; inference(return_state=True).image == inference()."""
    s = forward_pass(be, device, kind)
    target = torch.rand(3, 36, 48, generator=torch.Generator().manual_seed(9)).to(s.device)
    loss, grad, parts = be.l1_dssim(s.res.image, target, 0.8, 0.2, with_grad=False)
    loss_f, parts_f, scratch = be.l1_dssim_forward(s.res.image, target, 0.8, 0.2)
    assert grad is None and scratch.dtype == torch.uint8 and loss.dim() == 0 and parts.shape == (2,)
    assert torch.equal(loss, loss_f) and torch.equal(parts, parts_f) and float(loss) > 0
    loss_g, grad_g, parts_g = be.l1_dssim(s.res.image, target, 0.8, 0.2)
    assert torch.equal(loss_g, loss) and torch.equal(parts_g, parts) and grad_g.shape == target.shape
    for to_chw in ((kind != 'k1'),):          # one layout per kind (a simulated forward pass takes a second): CHW, HWC, CHW
        image = be.inference(*s.six, s.RS, to_chw, True)
        res = be.inference(*s.six, s.RS, to_chw, True, return_state=True)
        assert isinstance(image, torch.Tensor) and torch.equal(res.image, image) and len(res.buffers) == 4 and len(res.state) == 4
        assert image.shape == ((3, 36, 48) if to_chw else (36, 48, 3))
