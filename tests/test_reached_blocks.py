"""Reached-block flags (include/fgs_hip.h: fgs_backward_reached): beside `live_blocks` ("some Gaussian of the block of 64 is visible") the backward
gradients kernel publishes `reached_blocks` ("the backward blend pass reached some Gaussian of the block"). 0 there is a promise that every row of the
block is +-0 in all six gradient tensors, which lets fgs_adam_step_multi_live skip reading them -- also for the visible blocks hidden behind opaque
Gaussians. The flags are exact (compared with the device's own accumulator records), the optimizer's result is bit-identical with and without them, and
`live_blocks` keeps its meaning. Scenes: tests/unreached_cases.py (wall_scene: block 12 visible and unreached, 13 mixed, 14 behind the camera, ragged last
wave visible and unreached; hot_scene: a Gaussian of more than 256 tiles). This file runs the checks on the CPU simulation of the kernel sources;
tests/test_gpu_reached_blocks.py runs the same functions on the MI355X."""
import numpy as np
import pytest
import torch

import helpers
import unreached_cases as cases

ORDER, LRS, N = cases.ORDER, cases.LRS, cases.N
GUARD = 5                    # bytes behind each flag array that must keep their fill value
FILL = 7


def _flag_arrays(n, dev, live=True, reached=True):
    nb = (n + 63) // 64
    make = lambda: torch.full((nb + GUARD,), FILL, dtype=torch.uint8, device=dev)
    return (make() if live else None), (make() if reached else None), nb


def _records(be, res, n, view):
    layout = be.blob_layout(0, n, view.width, view.height, res.state[1], res.state[2])
    acc = be.view(res.buffers[0].cpu(), layout, 'acc', torch.float32)[:9 * n].reshape(n, 9).numpy()
    return ((acc.view(np.uint32) & 0x7fffffff) != 0).any(axis=1)


def _pass(be, dev, params, view, gi, out=None, live=True, reached=True):
    """One forward + backward pass with both flag arrays (pre-filled, guard bytes behind them); K11's records are read back from the primitive blob."""
    n = params['means'].shape[0]
    _, RS = helpers.settings_pair(view, device=dev)
    dp = {k: v.to(dev).contiguous() for k, v in params.items()}
    res = be.forward(*[dp[k] for k in helpers.NAMES], RS)
    L, R, nb = _flag_arrays(n, dev, live, reached)
    grads = be.backward(None, torch.as_tensor(gi).to(dev), res.image, dp['means'], dp['scales'], dp['rotations'], dp['opacities'], dp['sh_coefficients_rest'],
                        res.buffers, RS, res.state, out=out, live_blocks=None if L is None else L[:nb], reached_blocks=None if R is None else R[:nb])
    dec = helpers.decode_forward(be, res, n, view.width, view.height)
    visible = dec['n_touched'] > 0
    for t in (L, R):
        assert t is None or bool((t[nb:] == FILL).all()), 'a flag kernel wrote behind its array'
    return {'dp': dp, 'grads': dict(zip(helpers.NAMES, grads)), 'visible': visible, 'reached': visible & _records(be, res, n, view),
            'live_flags': None if L is None else L[:nb].clone(), 'reached_flags': None if R is None else R[:nb].clone(), 'n_touched': dec['n_touched']}


def _wall(be, dev, **kw):
    c = cases.case()
    return _pass(be, dev, c['params'], c['view'], c['gi'], **kw)


_WALL = {}


def wall(be, dev):
    """The wall scene's pass, once per device and process; read-only."""
    if dev not in _WALL:
        _WALL[dev] = _wall(be, dev)
    return _WALL[dev]


def _zero_rows(flags_np, n):
    return np.repeat(flags_np == 0, 64)[:n]


def check_flags(be, dev):
    w = wall(be, dev)
    live, reached = w['live_flags'].cpu().numpy(), w['reached_flags'].cpu().numpy()
    assert np.array_equal(w['visible'], cases.case()['visible'])
    want_reached = cases.blocks_of(w['reached']).any(axis=1).astype(np.uint8)          # the DEVICE's records: exact, no borderline-pixel allowance
    want_live = cases.blocks_of(w['visible']).any(axis=1).astype(np.uint8)
    assert np.array_equal(reached, want_reached), np.nonzero(reached != want_reached)
    assert np.array_equal(live, want_live), np.nonzero(live != want_live)
    assert (reached <= live).all()
    pairs = lambda b: (int(live[b]), int(reached[b]))
    assert pairs(cases.UNREACHED_BLOCK) == (1, 0) and pairs(cases.MIXED_BLOCK) == (1, 1) and pairs(cases.BEHIND_CAMERA_BLOCK) == (0, 0) and pairs(-1) == (1, 0)
    assert 0 < reached.sum() < reached.size and 0 < live.sum() < live.size


def check_promise(be, dev):
    """Every row of a block flagged 0 is exactly zero in all six tensors -- 16-byte aligned gradient tensors and tensors at data_ptr() % 16 == 4."""
    w = wall(be, dev)
    rows = torch.from_numpy(_zero_rows(w['reached_flags'].cpu().numpy(), N)).to(dev)
    assert int(rows.sum()) > 64 * 3
    for k in helpers.NAMES:
        assert not w['grads'][k][rows].any(), (k, 'aligned')
        assert w['grads'][k][~rows].any(), k
    shapes = [tuple(w['grads'][k].shape) for k in helpers.NAMES]
    odd = tuple(torch.full((int(np.prod(sh)) + 1,), float('nan'), dtype=torch.float32, device=dev)[1:].view(sh) for sh in shapes)
    assert all(t.data_ptr() % 16 == 4 for t in odd)
    o = _wall(be, dev, out=odd)
    assert torch.equal(o['reached_flags'], w['reached_flags']) or dev != 'cpu'          # hardware: a borderline pixel may move a record between two passes
    rows_odd = torch.from_numpy(_zero_rows(o['reached_flags'].cpu().numpy(), N)).to(dev)
    assert np.array_equal(o['reached_flags'].cpu().numpy(), cases.blocks_of(o['reached']).any(axis=1).astype(np.uint8))
    for k in helpers.NAMES:
        assert not o['grads'][k][rows_odd].any(), (k, 'unaligned')
        assert not torch.isnan(o['grads'][k]).any(), (k, 'an element was not written')
        if dev == 'cpu':
            assert torch.equal(o['grads'][k], w['grads'][k]), k


def check_adam(be, dev):
    """adam_step_multi on the SAME gradient tensors with live_blocks=None and with the reached array: bit-exact (no atomics), also with NaN in every
    unread element, and equal to the plain path once the gradients were edited behind the version counter (the sentinel)."""
    w = wall(be, dev)
    dp, flags = w['dp'], w['reached_flags']
    grads = {k: w['grads'][k] for k in ORDER}

    def adam(g, live):
        gen = torch.Generator().manual_seed(5)
        P = {k: dp[k].clone() for k in ORDER}
        M = {k: (torch.randn(dp[k].shape, generator=gen) * 1e-3).to(dev) for k in ORDER}
        V = {k: (torch.rand(dp[k].shape, generator=gen) * 1e-6 + 1e-7).to(dev) for k in ORDER}
        for step in (1, 2):
            be.adam_step_multi([g[k] for k in ORDER], [P[k] for k in ORDER], [M[k] for k in ORDER], [V[k] for k in ORDER], [step] * 6, LRS,
                               0.9, 0.999, 1e-15, live_blocks=live)
        return P, M, V
    ref, got = adam(grads, None), adam(grads, flags)
    zero_rows = torch.from_numpy(_zero_rows(flags.cpu().numpy(), N)).to(dev)
    first_rows = torch.from_numpy(np.arange(N) % 64 == 0).to(dev)
    poisoned = {k: grads[k].clone() for k in ORDER}
    for k in ORDER:
        flat = poisoned[k].reshape(N, -1)
        flat[zero_rows & ~first_rows] = float('nan')
        flat[zero_rows & first_rows, 1:] = float('nan')                  # everything but the block's sentinel element
    got_poisoned = adam(poisoned, flags)
    for a, b, c in zip(ref, got, got_poisoned):
        for k in ORDER:
            assert torch.equal(a[k], b[k]), k
            assert torch.equal(a[k], c[k]), ('poisoned', k)
    edited = {k: grads[k].clone() for k in ORDER}
    for k in ORDER:
        edited[k].data.add_(0.01 * dp[k])
    for a, b in zip(adam(edited, None), adam(edited, flags)):
        for k in ORDER:
            assert torch.equal(a[k], b[k]), ('edited behind the version counter', k)


def check_hot(be, dev):
    """The record of a Gaussian with more than 256 tiles arrives through the hot replicas and is complete only behind the fold. With the six small
    Gaussians moved behind the camera, Gaussian 0 alone decides the block's flag."""
    params, view = cases.hot_scene()
    gi = (np.random.default_rng(6).standard_normal((3, view.height, view.width)) / (3 * view.height * view.width)).astype(np.float32)
    for alone in (False, True):
        p = {k: v.clone() for k, v in params.items()}
        if alone:
            p['means'][1:, 2] = -10.0
        o = _pass(be, dev, p, view, gi)
        assert o['n_touched'][0] > 256 and (not alone or not o['visible'][1:].any()), o['n_touched']
        assert o['reached'][0]
        assert o['reached_flags'].tolist() == [1] and o['live_flags'].tolist() == [1], alone
        assert all(bool(o['grads'][k][0].any()) for k in helpers.NAMES)


def check_depth(be, dev):
    """Depth-only pass (grad_image = 0) of aux_grad_cases' partial_tiles: a block flagged 0 stays zero in grad_means after the depth mean-gradient kernel, and
    every Gaussian the fp64 reference gives a gradient sits in a block flagged 1."""
    import aux_grad_cases as aux
    c = aux.case('partial_tiles')
    ref = cases.depth_only_reference()
    RS = aux.settings_of(c, dev)
    p = [c['params'][k].to(dev) for k in helpers.NAMES]
    n = p[0].shape[0]
    res = be.forward_aux(*p, RS)
    L, R, nb = _flag_arrays(n, dev)
    grads = be.backward_aux(None, torch.zeros_like(res.image), None, torch.as_tensor(c['gD']).to(dev), res.image, res.depth, p[0], p[1], p[2], p[3], p[5],
                            res.buffers, RS, res.state, live_blocks=L[:nb], reached_blocks=R[:nb])
    g = dict(zip(helpers.NAMES, grads))
    live, reached = L[:nb].cpu().numpy(), R[:nb].cpu().numpy()
    assert bool((L[nb:] == FILL).all()) and bool((R[nb:] == FILL).all())
    assert set(np.unique(reached)) <= {0, 1} and (reached <= live).all()
    rows = torch.from_numpy(_zero_rows(reached, n)).to(dev)
    print('depth-only pass', dev, 'blocks', nb, 'live', int(live.sum()), 'reached', int(reached.sum()))
    for k in helpers.NAMES:
        assert not g[k][rows].any(), (k, 'a block flagged 0 has a non-zero row')
    contributes = np.abs(np.asarray(ref['means']).reshape(n, 3)).max(axis=1) > 1e-3 * np.abs(ref['means']).max()
    assert contributes.sum() > 50 and not _zero_rows(reached, n)[contributes].any()
    assert (np.abs(g['means'].cpu().numpy()[contributes]).max(axis=1) > 0).all()
    # partial_tiles has no block without a reached Gaussian; the wall scene under the same kind of pass does: with grad_image = 0 the colour sums of every
    # record are zero, the flag rests on the other sums and on dL/dz, and the blocks behind the wall stay flagged 0 and zero through the depth term
    w = cases.case()
    _, RS = helpers.settings_pair(w['view'], device=dev)
    p = [w['params'][k].to(dev).contiguous() for k in helpers.NAMES]
    res = be.forward_aux(*p, RS)
    gD = (np.random.default_rng(8).standard_normal((RS.height, RS.width)) / (RS.height * RS.width)).astype(np.float32)
    L, R, nb = _flag_arrays(N, dev)
    grads = be.backward_aux(None, torch.zeros_like(res.image), None, torch.as_tensor(gD).to(dev), res.image, res.depth, p[0], p[1], p[2], p[3], p[5],
                            res.buffers, RS, res.state, live_blocks=L[:nb], reached_blocks=R[:nb])
    g = dict(zip(helpers.NAMES, grads))
    live, reached = L[:nb].cpu().numpy(), R[:nb].cpu().numpy()
    assert bool((L[nb:] == FILL).all()) and bool((R[nb:] == FILL).all())
    assert np.array_equal(live, cases.blocks_of(w['visible']).any(axis=1).astype(np.uint8))
    pairs = lambda b: (int(live[b]), int(reached[b]))
    assert pairs(cases.UNREACHED_BLOCK) == (1, 0) and pairs(cases.MIXED_BLOCK) == (1, 1) and pairs(cases.BEHIND_CAMERA_BLOCK) == (0, 0) and pairs(-1) == (1, 0)
    rows = torch.from_numpy(_zero_rows(reached, N)).to(dev)
    for k in helpers.NAMES:
        assert not g[k][rows].any(), (k, 'wall scene, depth-only: a block flagged 0 has a non-zero row')
    assert not g['sh_coefficients_0'].any() and not g['sh_coefficients_rest'].any()
    mixed = slice(64 * cases.MIXED_BLOCK, 64 * cases.MIXED_BLOCK + 64)
    assert g['means'][mixed].any() and g['opacities'][mixed].any()


def check_bounds(be, dev):
    """N = 1483 (ragged last block: covered with guard bytes by every wall pass) and N = 64 (one full block); either array alone."""
    w = wall(be, dev)
    only_live, only_reached = _wall(be, dev, reached=False), _wall(be, dev, live=False)
    assert only_live['reached_flags'] is None and only_reached['live_flags'] is None
    assert torch.equal(only_live['live_flags'], w['live_flags'])
    assert np.array_equal(only_reached['reached_flags'].cpu().numpy(), cases.blocks_of(only_reached['reached']).any(axis=1).astype(np.uint8))
    if dev == 'cpu':
        assert torch.equal(only_reached['reached_flags'], w['reached_flags'])
        for k in helpers.NAMES:
            assert torch.equal(only_live['grads'][k], w['grads'][k]) and torch.equal(only_reached['grads'][k], w['grads'][k]), k
    from harness.scenes import make_s0
    params, view = make_s0(seed=3, n=64)
    gi = (np.random.default_rng(2).standard_normal((3, view.height, view.width)) / (3 * view.height * view.width)).astype(np.float32)
    for behind in (False, True):
        p = {k: v.clone() for k, v in params.items()}
        if behind:
            p['means'][:, 2] = -30.0
        o = _pass(be, dev, p, view, gi)
        want = [0] if behind else [1]
        assert o['live_flags'].tolist() == want and o['reached_flags'].tolist() == [int(o['reached'].any())] == want, (behind, o['reached'].sum())
    # an array that does not fit the tensors is refused before anything is launched
    _, RS = helpers.settings_pair(view, device=dev)
    dp = {k: v.to(dev).contiguous() for k, v in params.items()}
    res = be.forward(*[dp[k] for k in helpers.NAMES], RS)
    for bad in (torch.zeros(2, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)):
        with pytest.raises(RuntimeError, match='reached_blocks'):
            be.backward(None, torch.as_tensor(gi).to(dev), res.image, dp['means'], dp['scales'], dp['rotations'], dp['opacities'], dp['sh_coefficients_rest'],
                        res.buffers, RS, res.state, reached_blocks=bad)


def _train(dev, steps, handover, tamper=None):
    """render -> loss -> backward -> FusedAdam.step -> zero_grad on the wall scene through the public operators; parameters and both moments."""
    import FasterGSCudaBackend as FGS
    FGS.set_live_block_handover(handover)
    c = cases.case()
    _, RS = helpers.settings_pair(c['view'], device=dev)
    gi = torch.from_numpy(c['gi']).to(dev)
    P = {k: c['params'][k].to(dev).clone().requires_grad_(True) for k in ORDER}
    opt = FGS.FusedAdam([{'params': [P[k]], 'lr': lr, 'name': k} for k, lr in zip(ORDER, LRS)], lr=0.0, eps=1e-15)
    for i, k in enumerate(ORDER):
        m0, v0 = helpers.seeded_moments(P[k].shape, 31 + i)
        opt.state[P[k]] = {'step': 0, 'exp_avg': m0.to(dev), 'exp_avg_sq': v0.to(dev)}

    def backward():
        image = FGS.diff_rasterize(P['means'], P['scales'], P['rotations'], P['opacities'], P['sh_coefficients_0'], P['sh_coefficients_rest'],
                                   torch.empty(0, device=dev), RS)
        (image * gi).sum().backward()
    stats = []
    try:
        for _ in range(steps):
            backward()
            if tamper is not None:
                tamper(backward)
            opt.step()
            opt.zero_grad()
            stats.append(FGS.live_block_stats())
    finally:
        FGS.set_live_block_handover(True)
    out = {('p', k): P[k].detach().clone() for k in ORDER}
    out.update({('m', k): opt.state[P[k]]['exp_avg'].clone() for k in ORDER})
    out.update({('v', k): opt.state[P[k]]['exp_avg_sq'].clone() for k in ORDER})
    return out, stats


def check_autograd(be, dev, monkeypatch):
    import FasterGSCudaBackend as FGS
    from FasterGSCudaBackend import adam as A, rasterization as R
    if dev == 'cpu':                                   # the public operators refuse CPU tensors (no CPU implementation): point them at the simulation
        monkeypatch.setattr(R, '_require_gpu', lambda t: None)
        monkeypatch.setattr(R, 'default_backend', lambda: be)
        monkeypatch.setattr(A, 'default_backend', lambda: be)

    def same(a, b, what):
        for key in a:
            if dev == 'cpu':
                assert torch.equal(a[key], b[key]), (what, key)
            else:                                      # two hardware passes: K11's float atomics add in another order
                fig = helpers.rel_inf(a[key].cpu().numpy(), b[key].cpu().numpy())
                print('autograd', what, key, fig)
                assert fig < 1e-5, (what, key, fig)
    base = FGS.live_block_stats()
    plain, stats = _train(dev, 2, False)
    assert stats == [base, base]
    fast, stats = _train(dev, 2, True)
    assert [s['matched'] for s in stats] == [base['matched'] + 1, base['matched'] + 2] and stats[-1]['missed'] == base['missed']      # one per step
    same(fast, plain, 'hand-over')
    second = lambda backward: backward()               # accumulation into .grad before the step: the gradients are no longer what one pass wrote
    before = FGS.live_block_stats()
    a, _ = _train(dev, 1, True, second)
    after = FGS.live_block_stats()
    assert after['matched'] == before['matched'] and after['missed'] == before['missed'] + 1
    b, _ = _train(dev, 1, False, second)
    same(a, b, 'second backward')
    moved = (a['p', 'means'] - cases.case()['params']['means'].to(dev)).abs().amax(dim=1)
    assert bool((moved > 0).all())


def test_sim_flags_are_exact(sim_backend):
    check_flags(sim_backend, 'cpu')


def test_sim_rows_of_unreached_blocks_are_zero(sim_backend):
    check_promise(sim_backend, 'cpu')


def test_sim_adam_is_bit_exact_with_the_reached_flags(sim_backend):
    check_adam(sim_backend, 'cpu')


def test_sim_hot_gaussian_flags_its_block(sim_backend):
    check_hot(sim_backend, 'cpu')


def test_sim_depth_pass_keeps_the_promise(sim_backend):
    check_depth(sim_backend, 'cpu')


def test_sim_bounds_and_single_arrays(sim_backend):
    check_bounds(sim_backend, 'cpu')


def test_sim_handover_through_autograd(sim_backend, monkeypatch):
    check_autograd(sim_backend, 'cpu', monkeypatch)


def test_sim_two_kernel_form_flags_every_block(sim_backend):
    """The dev library's two-kernel A/B form of K12 publishes no flags: both arrays are set to 1 throughout."""
    be = sim_backend
    assert be.lib.fgs_debug_set_option(3, 0) == 0
    try:
        o = _wall(be, 'cpu')
    finally:
        assert be.lib.fgs_debug_set_option(3, 1) == 0
    assert bool((o['live_flags'] == 1).all()) and bool((o['reached_flags'] == 1).all())
    for k in helpers.NAMES:
        assert helpers.rel_inf(o['grads'][k].numpy(), wall(be, 'cpu')['grads'][k].numpy()) < 1e-5, k
