"""Checks shared by tests/test_gradient_recycling.py (CPU simulation) and tests/test_gpu_gradient_recycling.py (MI355X): the backward gradients kernel
takes a promise about what the gradient tensors hold already (include/fgs_hip.h: fgs_backward_recycled, `prior_blocks`) and leaves a block of 64 Gaussians
alone if the promise says "zero", the pass reaches none of its Gaussians and the block's first element agrees in all six tensors; the autograd path uses
that by writing into the arena of the previous pass (FasterGSCudaBackend/rasterization.py: set_gradient_recycling).

Scenes: the wall scene of tests/unreached_cases.py (N = 1483: block 12 visible and unreached, 13 mixed, 14 behind the camera, ragged last wave visible and
unreached) under its own camera and under a second one that looks at the wall from behind, and make_s0(n=64). Bars: bit-identical in the simulation; on
hardware two passes differ by the order of K11's float atomics, the suite's bar for that pair is 1e-5 of the tensor's max-abs value (tests/test_reached_blocks.py)."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import helpers
import test_reached_blocks as rb
import unreached_cases as cases
from harness.scenes import look_at_view, make_s0

ORDER, LRS, N = cases.ORDER, cases.LRS, cases.N
GUARD, FILL = rb.GUARD, rb.FILL
NB = (N + 63) // 64
CANARY = 123.0
PAIR_TOL = 1e-5
SH_CASES = ((1, 0), (4, 3), (9, 8), (16, 15))          # active_sh_bases, total_sh_rest


@functools.lru_cache(maxsize=None)
def views():
    """The wall scene's camera and one on the other side of the wall (what is hidden from the first is in front for the second), with their loss gradients."""
    c = cases.case()
    second = look_at_view((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), 128, 128, 128.0)
    gi2 = (np.random.default_rng(9).standard_normal(c['gi'].shape) / c['gi'].size).astype(np.float32)
    return (c['view'], c['gi']), (second, gi2)


def _close(a: torch.Tensor, b: torch.Tensor, dev: str, what) -> None:
    if dev == 'cpu':
        assert torch.equal(a, b), what
    else:
        fig = helpers.rel_inf(a.cpu().numpy(), b.cpu().numpy())
        print('gradient recycling', what, fig)
        assert fig < PAIR_TOL, (what, fig)


def _rows(blocks_mask: np.ndarray, n: int, dev: str) -> torch.Tensor:
    return torch.from_numpy(np.repeat(blocks_mask, 64)[:n]).to(dev)


def run_pass(be, dev, params, view, gi, K=16, out=None, prior=None, reached=True):
    """Forward + backward with guarded flag arrays; `prior` (uint8 [ceil(n / 64)]) goes in as prior_blocks and must come back untouched."""
    n = params['means'].shape[0]
    nb = (n + 63) // 64
    _, RS = helpers.settings_pair(view, K, device=dev)
    dp = {k: v.to(dev).contiguous() for k, v in params.items()}
    dp['sh_coefficients_rest'] = dp['sh_coefficients_rest'][:, :K - 1].contiguous()
    res = be.forward(*[dp[k] for k in helpers.NAMES], RS)
    L, R, _ = rb._flag_arrays(n, dev, True, reached)
    P = None
    if prior is not None:
        P = torch.cat([prior.to(dev).to(torch.uint8), torch.full((GUARD,), FILL, dtype=torch.uint8, device=dev)])
        before = P.clone()
    grads = be.backward(None, torch.as_tensor(gi).to(dev), res.image, dp['means'], dp['scales'], dp['rotations'], dp['opacities'], dp['sh_coefficients_rest'],
                        res.buffers, RS, res.state, out=out, live_blocks=L[:nb], reached_blocks=None if R is None else R[:nb],
                        prior_blocks=None if P is None else P[:nb])
    for t in (L, R):
        assert t is None or bool((t[nb:] == FILL).all()), 'a flag was written behind its array'
    assert P is None or torch.equal(P, before), 'prior_blocks is an input'
    dec = helpers.decode_forward(be, res, n, view.width, view.height)
    visible = dec['n_touched'] > 0
    reached_g = visible & rb._records(be, res, n, view)
    return {'grads': dict(zip(helpers.NAMES, grads)), 'visible': visible, 'reached': reached_g, 'live_flags': L[:nb].clone(),
            'reached_flags': None if R is None else R[:nb].clone(), 'want_flags': cases.blocks_of(reached_g).any(axis=1).astype(np.uint8)}


def _shapes(n: int, R: int) -> dict:
    return {'means': (n, 3), 'scales': (n, 3), 'rotations': (n, 4), 'opacities': (n, 1), 'sh_coefficients_0': (n, 1, 3), 'sh_coefficients_rest': (n, R, 3)}


def _tensors(n: int, R: int, dev: str, fill: float, odd: bool = False) -> dict:
    """Six gradient tensors full of `fill`; odd: each starts 4 bytes past a 16-byte boundary."""
    out = {}
    for k, sh in _shapes(n, R).items():
        base = torch.full((int(np.prod(sh)) + 1,), fill, dtype=torch.float32, device=dev)
        out[k] = base[1:].view(sh) if odd else base[:-1].view(sh)
        assert not odd or out[k].numel() == 0 or out[k].data_ptr() % 16 == 4
    return out


def _block(t: torch.Tensor, b: int) -> torch.Tensor:
    """Block b of a gradient tensor as a flat view (its first element is the kernel's sentinel)."""
    return t.reshape(t.shape[0], -1)[64 * b:64 * b + 64].reshape(-1)


_PLAIN = {}


def plain(be, dev, which: int = 0, K: int = 16):
    """The pass without a promise into new tensors: once per device, view and SH layout; read-only."""
    key = (dev, which, K)
    if key not in _PLAIN:
        view, gi = views()[which]
        _PLAIN[key] = run_pass(be, dev, cases.case()['params'], view, gi, K=K)
    return _PLAIN[key]


def check_views_differ(be, dev):
    """The premise of everything below that alternates the two cameras: both reach something, and each reaches blocks the other does not."""
    a, b = plain(be, dev, 0)['reached_flags'].cpu().numpy(), plain(be, dev, 1)['reached_flags'].cpu().numpy()
    only_a, only_b = int(((a == 1) & (b == 0)).sum()), int(((a == 0) & (b == 1)).sum())
    print('reached blocks', dev, int(a.sum()), int(b.sum()), 'only first', only_a, 'only second', only_b, 'of', NB)
    assert a.sum() > 0 and b.sum() > 0 and only_a > 0 and only_b > 0
    assert ((a == 0) & (b == 0)).sum() > 0, 'no block that stays zero from one view to the next'
    for w in (0, 1):
        assert np.array_equal(plain(be, dev, w)['reached_flags'].cpu().numpy(), plain(be, dev, w)['want_flags'])


def check_equal_to_plain(be, dev):
    """The second view's pass into the tensors of the first view's, as the promise describes them (zeros where its flag is 0, NaN elsewhere: every block
    flagged 1 must be written), against the same pass without a promise."""
    first, second = plain(be, dev, 0), plain(be, dev, 1)
    P = first['reached_flags']
    zero_blocks = P.cpu().numpy() == 0
    T = _tensors(N, 15, dev, float('nan'))
    for k in helpers.NAMES:
        T[k][_rows(zero_blocks, N, dev)] = 0.0
    view, gi = views()[1]
    o = run_pass(be, dev, cases.case()['params'], view, gi, out=tuple(T[k] for k in helpers.NAMES), prior=P)
    assert np.array_equal(o['reached_flags'].cpu().numpy(), o['want_flags']), 'flags against the device\'s own records'
    if dev == 'cpu':
        assert torch.equal(o['reached_flags'], second['reached_flags']) and torch.equal(o['live_flags'], second['live_flags'])
    rows = _rows(o['reached_flags'].cpu().numpy() == 0, N, dev)
    skipped = int(((o['reached_flags'].cpu().numpy() == 0) & zero_blocks).sum())
    assert skipped > 0 and int((~zero_blocks).sum()) > 0
    for k in helpers.NAMES:
        g = o['grads'][k]
        assert g.data_ptr() == T[k].data_ptr()
        assert not torch.isnan(g).any(), (k, 'an element of a block without a promise was not written')
        assert not g[rows].any(), (k, 'a row of a block flagged 0 is not zero')
        _close(g, second['grads'][k], dev, ('into the first view\'s tensors', k))


def check_blocks(be, dev, K: int = 16, odd: bool = False):
    """One pass over tensors prepared block by block (first camera; the scene's premises are asserted by unreached_cases.case()):
      block 12 (visible, unreached), the ragged last block (unreached): promise 0, first element of every tensor 0, CANARY in every other element
                                                    -> nothing is stored: the canaries survive
      block 14 (behind the camera): promise 0, canaries, first element non-zero in ONE tensor only -> all six tensors' rows are written as zeros
      block 13 (mixed, reached): promise 0, canaries -> written in full, flag 1
      every other block: promise 1, NaN -> written; flags as without a promise."""
    R = K - 1
    ref = plain(be, dev, 0, K)
    keep, sentinel, written = (cases.UNREACHED_BLOCK, NB - 1), cases.BEHIND_CAMERA_BLOCK, cases.MIXED_BLOCK
    P = torch.ones(NB, dtype=torch.uint8)
    P[[*keep, sentinel, written]] = 0
    T = _tensors(N, R, dev, float('nan'), odd)
    names = [k for k in helpers.NAMES if T[k].numel() > 0]
    assert len(names) == (5 if R == 0 else 6)
    for k in names:
        for b in (*keep, sentinel, written):
            _block(T[k], b).fill_(CANARY)
            _block(T[k], b)[0] = 0.0
    _block(T['scales'], sentinel)[0] = -2.5
    view, gi = views()[0]
    o = run_pass(be, dev, cases.case()['params'], view, gi, K=K, out=tuple(T[k] for k in helpers.NAMES), prior=P)
    flags = o['reached_flags'].cpu().numpy()
    assert np.array_equal(flags, o['want_flags'])
    assert [int(flags[b]) for b in (*keep, sentinel, written)] == [0, 0, 0, 1], flags
    if dev == 'cpu':
        assert torch.equal(o['reached_flags'], ref['reached_flags']) and torch.equal(o['live_flags'], ref['live_flags'])
    for k in names:
        g = o['grads'][k]
        for b in keep:
            blk = _block(g, b)
            assert float(blk[0]) == 0.0 and bool((blk[1:] == CANARY).all()), (k, b, 'a block that was promised zero and stayed unreached was stored to')
            blk.zero_()                                  # what the promise said was there: the rest is compared with the plain pass
        assert not _block(g, sentinel).any(), (k, 'the sentinel of ONE tensor must make the wave write all six')
        assert not (_block(g, written) == CANARY).any() and _block(g, written).any(), (k, 'a reached block must be written in full')
        assert not torch.isnan(g).any(), (k, 'a block without a promise was not written')
        assert not g[_rows(flags == 0, N, dev)].any(), k
        _close(g, ref['grads'][k], dev, ('blocks', K, odd, k))


def check_single_block(be, dev):
    """N = 64, one full wave: visible (reached: written over the canaries, flag 1) and all behind the camera (nothing stored, flag 0)."""
    params, view = make_s0(seed=3, n=64)
    gi = (np.random.default_rng(2).standard_normal((3, view.height, view.width)) / (3 * view.height * view.width)).astype(np.float32)
    for behind in (False, True):
        p = {k: v.clone() for k, v in params.items()}
        if behind:
            p['means'][:, 2] = -30.0
        T = _tensors(64, 15, dev, CANARY)
        for k in helpers.NAMES:
            _block(T[k], 0)[0] = 0.0
        o = run_pass(be, dev, p, view, gi, out=tuple(T[k] for k in helpers.NAMES), prior=torch.zeros(1, dtype=torch.uint8))
        assert o['reached_flags'].tolist() == [0 if behind else 1] and o['live_flags'].tolist() == [0 if behind else 1]
        for k in helpers.NAMES:
            blk = _block(o['grads'][k], 0)
            if behind:
                assert float(blk[0]) == 0.0 and bool((blk[1:] == CANARY).all()), k
            else:
                assert not (blk == CANARY).any() and blk.any(), k


def check_refusals(be, dev):
    params, view = make_s0(seed=3, n=64)
    gi = torch.zeros(3, view.height, view.width, device=dev)
    _, RS = helpers.settings_pair(view, device=dev)
    dp = {k: v.to(dev).contiguous() for k, v in params.items()}
    res = be.forward(*[dp[k] for k in helpers.NAMES], RS)
    byte = lambda: torch.zeros(1, dtype=torch.uint8, device=dev)
    call = lambda **kw: be.backward(None, gi, res.image, dp['means'], dp['scales'], dp['rotations'], dp['opacities'], dp['sh_coefficients_rest'],
                                    res.buffers, RS, res.state, **kw)
    with pytest.raises(RuntimeError, match='prior_blocks without reached_blocks'):
        call(prior_blocks=byte())
    with pytest.raises(RuntimeError, match='prior_blocks without reached_blocks'):
        call(prior_blocks=byte(), live_blocks=byte())
    shared = byte()
    with pytest.raises(RuntimeError, match='prior_blocks aliases reached_blocks'):
        call(prior_blocks=shared, reached_blocks=shared)
    with pytest.raises(RuntimeError, match='prior_blocks aliases live_blocks'):
        call(prior_blocks=shared, reached_blocks=byte(), live_blocks=shared)
    for bad in (torch.zeros(2, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)):
        with pytest.raises(RuntimeError, match='prior_blocks must be'):
            call(prior_blocks=bad, reached_blocks=byte())
    grads = call(prior_blocks=byte() + 1, reached_blocks=byte())          # and the accepted form runs
    assert all(bool(torch.isfinite(g).all()) for g in grads)


def check_two_kernel_form(be, dev):
    """Simulation (dev library) only: the two-kernel A/B form writes every element and publishes all-ones flags, whatever the promise says."""
    T = _tensors(N, 15, dev, CANARY)
    for k in helpers.NAMES:
        T[k].reshape(N, -1)[::64, 0] = 0.0
    view, gi = views()[0]
    assert be.lib.fgs_debug_set_option(3, 0) == 0
    try:
        o = run_pass(be, dev, cases.case()['params'], view, gi, out=tuple(T[k] for k in helpers.NAMES), prior=torch.zeros(NB, dtype=torch.uint8))
    finally:
        assert be.lib.fgs_debug_set_option(3, 1) == 0
    assert bool((o['reached_flags'] == 1).all()) and bool((o['live_flags'] == 1).all())
    for k in helpers.NAMES:
        assert not (o['grads'][k] == CANARY).any(), k
        assert helpers.rel_inf(o['grads'][k].cpu().numpy(), plain(be, dev, 0)['grads'][k].cpu().numpy()) < PAIR_TOL, k


# ---- through autograd: diff_rasterize -> loss -> backward -> FusedAdam.step -> zero_grad, the two cameras in turn ----------------------------------------
def _model(params: dict, dev: str, seed: int = 31):
    import FasterGSCudaBackend as FGS
    P = {k: params[k].to(dev).clone().requires_grad_(True) for k in ORDER}
    opt = FGS.FusedAdam([{'params': [P[k]], 'lr': lr, 'name': k} for k, lr in zip(ORDER, LRS)], lr=0.0, eps=1e-15)
    for i, k in enumerate(ORDER):
        m0, v0 = helpers.seeded_moments(P[k].shape, seed + i)
        opt.state[P[k]] = {'step': 0, 'exp_avg': m0.to(dev), 'exp_avg_sq': v0.to(dev)}
    return P, opt


def _state(P, opt) -> dict:
    out = {('p', k): P[k].detach().clone() for k in ORDER}
    out.update({('m', k): opt.state[P[k]]['exp_avg'].clone() for k in ORDER})
    out.update({('v', k): opt.state[P[k]]['exp_avg_sq'].clone() for k in ORDER})
    return out


def train(dev, steps: int, recycle: bool, hook=None, grow_at: int | None = None):
    """Returns (parameters and moments, 'R' / 'F' per backward pass in order, live_block_stats deltas). hook(step, phase, ctx) with phase in
    'after_backward', 'zero_grad' (return True if the hook did the zeroing itself), 'after_zero_grad'; ctx: P, opt, backward. grow_at: the model gets one
    more Gaussian (and a new optimizer) in front of that step."""
    import FasterGSCudaBackend as FGS
    FGS.set_gradient_recycling(recycle)
    FGS.set_live_block_handover(True)
    base_r, base_l = FGS.gradient_recycling_stats(), FGS.live_block_stats()
    settings = [(helpers.settings_pair(v, device=dev)[1], torch.from_numpy(g).to(dev)) for v, g in views()]
    P, opt = _model(cases.case()['params'], dev)
    passes = []
    try:
        for i in range(steps):
            if grow_at == i:
                grown = {k: torch.cat([P[k].detach(), P[k].detach()[1000:1001]]).cpu() for k in ORDER}      # a copy of a small Gaussian in front of the wall,
                grown['means'][-1] += 0.013                                                                # moved off its original (no tied depth key)
                P, opt = _model(grown, dev, seed=57)
            RS, gi = settings[i % 2]

            def backward():
                before = FGS.gradient_recycling_stats()
                image = FGS.diff_rasterize(P['means'], P['scales'], P['rotations'], P['opacities'], P['sh_coefficients_0'], P['sh_coefficients_rest'],
                                           torch.empty(0, device=dev), RS)
                (image * gi).sum().backward()
                after = FGS.gradient_recycling_stats()
                delta = (after['recycled'] - before['recycled'], after['fresh'] - before['fresh'])
                assert delta in ((1, 0), (0, 1)), delta
                passes.append('R' if delta == (1, 0) else 'F')
            ctx = {'P': P, 'opt': opt, 'backward': backward}
            backward()
            if hook is not None:
                hook(i, 'after_backward', ctx)
            opt.step()
            if not (hook is not None and hook(i, 'zero_grad', ctx)):
                opt.zero_grad()
            if hook is not None:
                hook(i, 'after_zero_grad', ctx)
        out = _state(P, opt)
        live = FGS.live_block_stats()
    finally:
        FGS.set_gradient_recycling(True)
    assert FGS.gradient_recycling_stats()['recycled'] - base_r['recycled'] == passes.count('R')
    return out, ''.join(passes), {k: live[k] - base_l[k] for k in live}


def _same(a: dict, b: dict, dev: str, what: str) -> None:
    assert a.keys() == b.keys()
    for key in a:
        assert a[key].shape == b[key].shape, (what, key)
        _close(a[key], b[key], dev, (what, key))


def point_operators_at(be, dev, monkeypatch) -> None:
    """The public operators refuse CPU tensors (there is no CPU implementation): in the simulation they are pointed at the simulated library."""
    from FasterGSCudaBackend import adam as A, rasterization as R
    if dev == 'cpu':
        monkeypatch.setattr(R, '_require_gpu', lambda t: None)
        monkeypatch.setattr(R, 'default_backend', lambda: be)
        monkeypatch.setattr(A, 'default_backend', lambda: be)
    assert R._STORAGE_USE_COUNT is not None, 'this torch has no storage reference count: nothing would be recycled and nothing below would be tested'


_OFF = {}


def _off(dev, steps=4):
    """The run without recycling and without interference: once per device; read-only."""
    if (dev, steps) not in _OFF:
        _OFF[dev, steps] = train(dev, steps, False)
    return _OFF[dev, steps]


def check_recycling_changes_nothing(be, dev, monkeypatch):
    point_operators_at(be, dev, monkeypatch)
    off, passes_off, live_off = _off(dev)
    on, passes_on, live_on = train(dev, 4, True)
    assert passes_off == 'FFFF' and passes_on == 'FRRR', (passes_off, passes_on)
    assert live_on == live_off == {'matched': 4, 'missed': 0}, (live_on, live_off)
    _same(on, off, dev, 'recycling on / off')
    moved = (on['p', 'means'] - cases.case()['params']['means'].to(dev)).abs().amax(dim=1)
    assert bool((moved > 0).all())


def _kept_gradient(alias):
    """A reference to the gradient of `means` (or an alias of it) is taken after step 1 and held across zero_grad and the next backward pass: that pass
    must not write into the memory it points to."""
    held = {}

    def hook(i, phase, ctx):
        if i == 1 and phase == 'after_backward':
            held['t'] = alias(ctx['P']['means'].grad)
            held['copy'] = held['t'].clone()
        if i == 2 and phase == 'after_backward':
            assert torch.equal(held['t'], held['copy']), 'a gradient the user still holds changed under them'
            assert held['t'].data_ptr() != ctx['P']['means'].grad.data_ptr()
            held.clear()
    return hook


def _keep_tensors_in_zero_grad(i, phase, ctx):
    if i == 1 and phase == 'zero_grad':
        ctx['opt'].zero_grad(set_to_none=False)
        return True
    return False


def _scale_gradients(i, phase, ctx):
    if i == 1 and phase == 'after_backward':
        for p in ctx['P'].values():
            p.grad.mul_(0.5)


def _second_backward(i, phase, ctx):
    if i == 1 and phase == 'after_backward':
        ctx['backward']()


def _weight_decay_behind_the_version_counter(i, phase, ctx):
    if i == 1 and phase == 'after_backward':
        for p in ctx['P'].values():
            p.grad.data.add_(0.01 * p.detach())


# name -> (hook, passes with recycling on). In every case the pass that follows the interference takes new memory ('F'); the one after that recycles again.
INTERFERENCE = {
    'kept_grad': (lambda: _kept_gradient(lambda g: g), 'FRFR'),
    'kept_detached_alias': (lambda: _kept_gradient(lambda g: g.detach()), 'FRFR'),
    'kept_flat_view': (lambda: _kept_gradient(lambda g: g.view(-1)), 'FRFR'),
    'zero_grad_keeps_tensors': (lambda: _keep_tensors_in_zero_grad, 'FRFR'),
    'scaled_in_place': (lambda: _scale_gradients, 'FRFR'),
    'second_backward': (lambda: _second_backward, 'FRFRR'),              # the second pass of step 1: its first one holds the spare
    # Behind the version counter nothing torch can see has happened: the arena IS recycled, and the kernel's sentinels -- the first element of each block
    # is 0.01 p != 0 in at least one tensor (rotations and scales are never zero) -- make it write every block, exactly as the optimizer reads every block
    'weight_decay_behind_the_version_counter': (lambda: _weight_decay_behind_the_version_counter, 'FRRR'),
}


VALUES_UNCHANGED = ('kept_grad', 'kept_detached_alias', 'kept_flat_view', 'zero_grad_keeps_tensors')


def check_interference(be, dev, monkeypatch, name: str):
    point_operators_at(be, dev, monkeypatch)
    make, want = INTERFERENCE[name]
    # holding on to a gradient, or zeroing it in place, changes no value: those cases share the undisturbed run without recycling
    off, passes_off, _ = _off(dev) if name in VALUES_UNCHANGED else train(dev, 4, False, make())
    on, passes_on, _ = train(dev, 4, True, make())
    assert passes_on == want and passes_off == 'F' * len(want), (name, passes_on, passes_off)
    _same(on, off, dev, name)


def check_growing_model(be, dev, monkeypatch):
    """Density control changed N between two steps: the shapes differ, the pass takes new memory, the next one recycles again."""
    point_operators_at(be, dev, monkeypatch)
    off, passes_off, _ = train(dev, 4, False, grow_at=2)
    on, passes_on, _ = train(dev, 4, True, grow_at=2)
    assert (passes_on, passes_off) == ('FRFR', 'FFFF')
    assert on['p', 'means'].shape[0] == N + 1
    _same(on, off, dev, 'one Gaussian more')


def check_second_model_takes_the_spare(be, dev, monkeypatch):
    """Spares are keyed by device and shapes: a second model of the same shapes writes into the arena the first one's step left."""
    import FasterGSCudaBackend as FGS
    point_operators_at(be, dev, monkeypatch)
    FGS.set_gradient_recycling(True)
    RS, gi = helpers.settings_pair(views()[0][0], device=dev)[1], torch.from_numpy(views()[0][1]).to(dev)
    results = []
    for recycle in (True, False):
        FGS.set_gradient_recycling(recycle)
        base = FGS.gradient_recycling_stats()
        models = [_model(cases.case()['params'], dev, seed) for seed in (31, 77)]
        for P, opt in models:
            image = FGS.diff_rasterize(P['means'], P['scales'], P['rotations'], P['opacities'], P['sh_coefficients_0'], P['sh_coefficients_rest'],
                                       torch.empty(0, device=dev), RS)
            (image * gi).sum().backward()
            opt.step()
            opt.zero_grad()
        after = FGS.gradient_recycling_stats()
        assert (after['recycled'] - base['recycled'], after['fresh'] - base['fresh']) == ((1, 1) if recycle else (0, 2))
        results.append(_state(*models[1]))
    FGS.set_gradient_recycling(True)
    _same(results[0], results[1], dev, 'second model')
