"""Quiet-block flags of the optimizer (include/fgs_hip.h: fgs_adam_step_multi_quiet, fgs_adam_quiet_scan; FasterGSCudaBackend/adam.py): one byte per block of
64 Gaussians, 1 = "both Adam moments of the block are zero in every group". A block that is quiet and whose gradient is not needed is neither read nor
written by the step -- with g = m = v = 0 the update is the identity -- so parameters and moments must be bit for bit what the existing entry
fgs_adam_step_multi_live leaves (+-0 compared as equal), the flags must never promise more than the moments hold, and FusedAdam must rebuild them whenever
somebody else wrote the moments. Shapes: N = 1483 (23 blocks of 64 and a ragged one of 11; `means` has 4449 floats: the optimizer kernel's scalar tail
exists), N = 64 and N = 1, the six tensors at SH degree 3. This file runs the checks on the CPU simulation of the kernel sources;
tests/test_gpu_quiet_blocks.py runs the same functions on the MI355X."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import helpers
import unreached_cases as cases

ORDER, LRS = cases.ORDER, cases.LRS
ROW = {'means': (3,), 'sh_coefficients_0': (1, 3), 'sh_coefficients_rest': (15, 3), 'opacities': (1,), 'scales': (3,), 'rotations': (4,)}
GUARD, FILL = 5, 7               # bytes behind the flag array that must keep their fill value
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15
NOT_QUIET = (1, 2, 5, 9)         # blocks that start with non-zero moments
# blocks whose gradient is needed in step 1 .. 5. With NOT_QUIET: quiet and reached (0 in step 1, 3 in step 2, 7 -- reached in step 3 ONLY -- and the ragged
# block 23 in step 3), quiet and not reached (most), not quiet and reached (1, 2, 9), not quiet and not reached (5 throughout: momentum alone)
REACHED = ((0, 1, 22), (1, 3), (7, 2, 23), (3,), (0, 9))
NEVER = 10                       # quiet and never reached: carries a -0.0 moment that only a store would turn into +0


def _blocks(n):
    return (n + 63) // 64


def _flags(nb, dev, ones=()):
    full = torch.full((nb + GUARD,), FILL, dtype=torch.uint8, device=dev)
    full[:nb] = 0
    for b in ones:
        if b < nb:
            full[b] = 1
    return full


def _rows_of(blocks, n, dev):
    rows = torch.zeros(_blocks(n) * 64, dtype=torch.bool)
    for b in blocks:
        if b < _blocks(n):
            rows[64 * b:64 * b + 64] = True
    return rows[:n].to(dev)


def _state(n, dev, seed=3):
    gen = torch.Generator().manual_seed(seed)
    P = {k: torch.randn((n,) + ROW[k], generator=gen).to(dev) for k in ORDER}
    busy = _rows_of(NOT_QUIET if _blocks(n) > 1 else (), n, 'cpu')
    M, V = {}, {}
    for k in ORDER:
        m = torch.randn((n,) + ROW[k], generator=gen) * 1e-3
        v = torch.rand((n,) + ROW[k], generator=gen) * 1e-6 + 1e-7
        m[~busy], v[~busy] = 0.0, 0.0
        M[k], V[k] = m.to(dev), v.to(dev)
    return P, M, V


def _gradients(n, dev, reached, seed):
    gen = torch.Generator().manual_seed(seed)
    rows = _rows_of(reached, n, 'cpu')
    G = {}
    for k in ORDER:
        g = torch.randn((n,) + ROW[k], generator=gen) * 1e-2
        g[~rows] = 0.0
        G[k] = g.to(dev)
    return G


def quiet_reference(M, V, n):
    """The torch reduction the scan is held to: a block is quiet iff no element of either moment of any tensor differs from zero (NaN differs)."""
    busy = torch.zeros(n, dtype=torch.bool, device=next(iter(M.values())).device)
    for k in M:
        for t in (M[k], V[k]):
            busy |= (~(t.reshape(n, -1) == 0)).any(dim=1)
    pad = torch.zeros((-n) % 64, dtype=torch.bool, device=busy.device)
    return (~torch.cat([busy, pad]).reshape(-1, 64).any(dim=1)).to(torch.uint8)


def check_invariant(quiet, M, V, n, reached=None):
    """quiet[b] == 1 implies that every moment of b reads zero; a block whose gradient was read reads 0."""
    assert set(np.unique(quiet.cpu().numpy())) <= {0, 1}
    assert bool((quiet <= quiet_reference(M, V, n)).all()), 'a block flagged quiet has a non-zero moment'
    if reached is not None:
        for b in reached:
            if b < _blocks(n):
                assert int(quiet[b]) == 0, ('reached block still flagged quiet', b)


def live_entry(be, G, P, M, V, step, live, eps=EPS, lrs=LRS):
    """The EXISTING entry point fgs_adam_step_multi_live (or fgs_adam_step_multi without flags), called directly: the expected result of every comparison."""
    _, B = helpers.backend_modules()
    k, n = len(ORDER), P[ORDER[0]].shape[0]
    arr = lambda d: (C.c_void_p * k)(*[B._ptr(d[name]) for name in ORDER])
    numel = (C.c_int64 * k)(*[P[name].numel() for name in ORDER])
    steps, rates = (C.c_int32 * k)(*[step] * k), (C.c_double * k)(*lrs)
    stream = B._stream_of(P[ORDER[0]].device)
    if live is None:
        rc = be.lib.fgs_adam_step_multi(k, arr(G), arr(P), arr(M), arr(V), numel, steps, rates, BETA1, BETA2, eps, stream)
    else:
        rows = (C.c_int32 * k)(*[P[name].numel() // n for name in ORDER])
        rc = be.lib.fgs_adam_step_multi_live(k, arr(G), arr(P), arr(M), arr(V), numel, steps, rates, BETA1, BETA2, eps, B._ptr(live), rows, stream)
    assert rc == 0, be.lib.fgs_last_error()


def _same(a, b, what):
    for k in ORDER:
        assert torch.equal(a[k], b[k]), (what, k)           # value comparison: +0 == -0, and no NaN anywhere


def check_equivalence(be, dev, n):
    nb = _blocks(n)
    reached_of = REACHED if nb > 1 else ((), (), (0,), (), ())
    ref, got = _state(n, dev), _state(n, dev)
    if nb > NEVER:
        for state in (ref, got):
            state[1]['sh_coefficients_rest'][64 * NEVER + 31, 7, 1] = -0.0
    Q = _flags(nb, dev)
    quiet = Q[:nb]
    be.adam_quiet_scan([got[1][k] for k in ORDER], [got[2][k] for k in ORDER], out=quiet)
    assert torch.equal(quiet, quiet_reference(got[1], got[2], n))
    assert int(quiet.sum()) == (nb - len(NOT_QUIET) if nb > 1 else 1)
    for step, reached in enumerate(reached_of, start=1):
        G = _gradients(n, dev, reached, seed=100 + step)
        live = _flags(nb, dev, ones=reached)[:nb]
        before = quiet.clone()
        live_entry(be, G, *ref, step, live)
        be.adam_step_multi([G[k] for k in ORDER], *[[t[k] for k in ORDER] for t in got], [step] * 6, LRS, BETA1, BETA2, EPS, live_blocks=live, quiet_blocks=quiet)
        for a, b, what in zip(ref, got, 'pmv'):
            _same(a, b, (n, step, what))
        assert bool((Q[nb:] == FILL).all()), 'the step wrote behind the flag array'
        check_invariant(quiet, got[1], got[2], n, reached)
        assert torch.equal(quiet, before * (1 - live)), 'the flag of a block that was not reached changed, or a flag was set'
    if nb > NEVER:
        # the never-reached quiet block was not stored to: its -0.0 moment is still -0.0 (the full step leaves +0 there: fma(beta1, -0 - 0, 0))
        assert bool(torch.signbit(got[1]['sh_coefficients_rest'][64 * NEVER + 31, 7, 1])) and not bool(torch.signbit(ref[1]['sh_coefficients_rest'][64 * NEVER + 31, 7, 1]))
        assert int(quiet.sum()) == nb - len(set(NOT_QUIET) | {b for r in REACHED for b in r})


def check_scan(be, dev):
    n, nb = 1483, _blocks(1483)
    gen = torch.Generator().manual_seed(17)
    M = {k: torch.zeros((n,) + ROW[k]) for k in ORDER}
    V = {k: torch.zeros((n,) + ROW[k]) for k in ORDER}
    for b in torch.nonzero(torch.rand(nb, generator=gen) < 0.3).flatten().tolist():        # random block sparsity: one element somewhere in the block
        if b in (4, 6, 8, 11, 13, 23):
            continue
        k = ORDER[int(torch.randint(6, (1,), generator=gen))]
        row = 64 * b + int(torch.randint(min(64, n - 64 * b), (1,), generator=gen))
        (M if b % 2 else V)[k][row].view(-1)[-1] = 0.25
    M['scales'][64 * 4 + 5, 1] = -0.0                                       # a lone -0.0: still quiet
    M['sh_coefficients_rest'][64 * 6 + 63, 14, 2] = 1e-45                   # a lone denormal: not zero
    V['opacities'][64 * 8, 0] = float('nan')                                # a lone NaN: not zero
    V['rotations'][64 * 11 + 17, 3] = 1e-12                                 # only exp_avg_sq of the last tensor
    V['means'][n - 1, 2] = 3.0                                              # the last float of the ragged block
    M, V = {k: t.to(dev) for k, t in M.items()}, {k: t.to(dev) for k, t in V.items()}
    want = quiet_reference(M, V, n)
    assert [int(want[b]) for b in (4, 6, 8, 11, 13, 23)] == [1, 0, 0, 0, 1, 0] and 0 < int(want.sum()) < nb
    Q = _flags(nb, dev)
    out = be.adam_quiet_scan([M[k] for k in ORDER], [V[k] for k in ORDER], out=Q[:nb])
    assert torch.equal(out, want), torch.nonzero(out != want).flatten().tolist()
    assert bool((Q[nb:] == FILL).all()), 'the scan wrote behind its array'
    V['means'][n - 1, 2] = 0.0                                              # ... and an all-zero ragged block is quiet
    assert int(be.adam_quiet_scan([M[k] for k in ORDER], [V[k] for k in ORDER])[nb - 1]) == 1
    # tensors that are not 16-byte aligned take the scalar path
    shift = lambda t: torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(t.shape)
    Mo, Vo = {k: shift(M[k]) for k in ORDER}, {k: shift(V[k]) for k in ORDER}
    assert all(t.data_ptr() % 16 == 4 for t in Mo.values())
    assert torch.equal(be.adam_quiet_scan([Mo[k] for k in ORDER], [Vo[k] for k in ORDER]), quiet_reference(M, V, n))
    for small in (64, 1):
        m = {k: torch.zeros((small,) + ROW[k], device=dev) for k in ORDER}
        v = {k: torch.zeros((small,) + ROW[k], device=dev) for k in ORDER}
        assert be.adam_quiet_scan([m[k] for k in ORDER], [v[k] for k in ORDER]).tolist() == [1]
        v['rotations'][small - 1, 3] = 1.0
        assert be.adam_quiet_scan([m[k] for k in ORDER], [v[k] for k in ORDER]).tolist() == [0]
    # groups that do not share one N are refused
    _, B = helpers.backend_modules()
    two = [torch.zeros(128, 3, device=dev), torch.zeros(64, 4, device=dev)]
    ptrs = (C.c_void_p * 2)(*[B._ptr(t) for t in two])
    rc = be.lib.fgs_adam_quiet_scan(2, ptrs, ptrs, (C.c_int64 * 2)(384, 256), (C.c_int32 * 2)(3, 4), B._ptr(torch.zeros(2, dtype=torch.uint8, device=dev)),
                                    B._stream_of(two[0].device))
    assert rc == -1 and b'same N' in be.lib.fgs_last_error()


def check_eps_zero(be, dev):
    """eps = 0: the full step divides 0 by 0 where gradient and moments are zero. The quiet entry must leave the same NaN pattern (nothing skipped)
    and no flag standing."""
    n, nb = 1483, _blocks(1483)
    ref, got = _state(n, dev), _state(n, dev)
    G = _gradients(n, dev, (0, 1), seed=9)
    live = _flags(nb, dev, ones=(0, 1))[:nb]
    quiet = quiet_reference(got[1], got[2], n)
    assert int(quiet.sum()) == nb - len(NOT_QUIET)
    live_entry(be, G, *ref, 1, live, eps=0.0)
    be.adam_step_multi([G[k] for k in ORDER], *[[t[k] for k in ORDER] for t in got], [1] * 6, LRS, BETA1, BETA2, 0.0, live_blocks=live, quiet_blocks=quiet)
    assert bool(torch.isnan(ref[0]['means'][_rows_of((3,), n, dev)]).all()) and not bool(torch.isnan(ref[0]['means'][_rows_of((1,), n, dev)]).any())
    for a, b in zip(ref, got):
        for k in ORDER:
            assert torch.equal(torch.isnan(a[k]), torch.isnan(b[k])), k
            assert torch.equal(torch.nan_to_num(a[k]), torch.nan_to_num(b[k])), k
    assert not bool(quiet.any())
    # quiet flags without live flags: nothing says which blocks get a gradient -- every flag is cleared, the step is the plain one
    ref, got = _state(n, dev), _state(n, dev)
    quiet = quiet_reference(got[1], got[2], n)
    live_entry(be, G, *ref, 1, None)
    be.adam_step_multi([G[k] for k in ORDER], *[[t[k] for k in ORDER] for t in got], [1] * 6, LRS, BETA1, BETA2, EPS, quiet_blocks=quiet)
    for a, b, what in zip(ref, got, 'pmv'):
        _same(a, b, ('no live flags', what))
    assert not bool(quiet.any())


# ---- through FusedAdam: the wall scene of tests/unreached_cases.py (blocks 12 and 19 .. 23 lie behind the wall, block 14 behind the camera) -------------------------
class _Counting:
    """The backend with its scans counted and the flags of every step kept as they were handed over."""
    def __init__(self, be):
        self._be, self.scans, self.handed = be, 0, []

    def __getattr__(self, name):
        return getattr(self._be, name)

    def adam_quiet_scan(self, *a, **kw):
        self.scans += 1
        return self._be.adam_quiet_scan(*a, **kw)

    def adam_step_multi(self, grads, params, exp_avgs, exp_avg_sqs, *a, live_blocks=None, quiet_blocks=None, **kw):
        self.handed.append(None if quiet_blocks is None else (quiet_blocks.clone(), self._be.adam_quiet_scan(exp_avgs, exp_avg_sqs)))
        return self._be.adam_step_multi(grads, params, exp_avgs, exp_avg_sqs, *a, live_blocks=live_blocks, quiet_blocks=quiet_blocks, **kw)


class _Pair:
    """Two optimizers in lockstep on identical state. A takes its gradients from the rasterizer's backward pass (reached-block hand-over, quiet flags); B is
    handed clones of the same gradients as `.grad` -- no hand-over, hence never a quiet flag: the plain step. After every step they must agree bit for bit."""
    def __init__(self, be, dev, monkeypatch):
        import FasterGSCudaBackend as FGS
        from FasterGSCudaBackend import adam as A, rasterization as R
        self.FGS, self.dev, self.be = FGS, dev, _Counting(be)
        if dev == 'cpu':                                   # the public operators refuse CPU tensors (no CPU implementation): point them at the simulation
            monkeypatch.setattr(R, '_require_gpu', lambda t: None)
            monkeypatch.setattr(R, 'default_backend', lambda: be)
        monkeypatch.setattr(A, 'default_backend', lambda: self.be)
        params, view = cases.wall_scene()
        _, self.RS = helpers.settings_pair(view, device=dev)
        self.gi = torch.from_numpy((np.random.default_rng(5).standard_normal((3, view.height, view.width)) / (3 * view.height * view.width)).astype(np.float32)).to(dev)
        self.PA = {k: params[k].to(dev).clone().requires_grad_(True) for k in ORDER}
        self.PB = {k: params[k].to(dev).clone().requires_grad_(True) for k in ORDER}
        self.A, self.B = self._optimizer(self.PA), self._optimizer(self.PB)

    def _optimizer(self, P):
        return self.FGS.FusedAdam([{'params': [P[k]], 'lr': lr, 'name': k} for k, lr in zip(ORDER, LRS)], lr=0.0, eps=EPS)

    def moments(self, opt, P):
        return {k: opt.state[P[k]]['exp_avg'] for k in ORDER}, {k: opt.state[P[k]]['exp_avg_sq'] for k in ORDER}

    def step(self, edit_gradients=None, what=''):
        P = self.PA
        image = self.FGS.diff_rasterize(P['means'], P['scales'], P['rotations'], P['opacities'], P['sh_coefficients_0'], P['sh_coefficients_rest'],
                                        torch.empty(0, device=self.dev), self.RS)
        (image * self.gi).sum().backward()
        if edit_gradients is not None:
            edit_gradients({k: P[k].grad for k in ORDER})
        for k in ORDER:
            self.PB[k].grad = P[k].grad.detach().clone()
        self.A.step()
        self.B.step()
        self.A.zero_grad()
        self.B.zero_grad()
        (ma, va), (mb, vb) = self.moments(self.A, self.PA), self.moments(self.B, self.PB)
        for k in ORDER:
            assert torch.equal(self.PA[k], self.PB[k]), (what, 'parameter', k)
            assert torch.equal(ma[k], mb[k]) and torch.equal(va[k], vb[k]), (what, 'moments', k)
        assert self.B.quiet_blocks() is None
        quiet = self.A.quiet_blocks()
        if quiet is not None:
            check_invariant(quiet, ma, va, self.PA['means'].shape[0])
        return quiet

    def both(self, edit):
        """The same edit of the optimizer state of A and of B."""
        edit(self.A, self.PA)
        edit(self.B, self.PB)


HIDDEN = (12, 14, 20, 23)          # wall scene: behind the wall, behind the camera, behind the wall, the ragged block behind the wall


def check_first_step(be, dev, monkeypatch):
    """Moments created in this very step: the flags start as all ones without a scan, and that is what a scan of those moments returns."""
    pair = _Pair(be, dev, monkeypatch)
    quiet = pair.step(what='first step')
    handed = [h for h in pair.be.handed if h is not None]
    assert len(handed) == 1 and pair.be.scans == 0
    assert bool((handed[0][0] == 1).all()) and torch.equal(handed[0][0], handed[0][1])
    assert quiet is not None and all(int(quiet[b]) == 1 for b in HIDDEN) and int(quiet[0]) == 0 and 0 < int(quiet.sum()) < quiet.numel()
    before = {k: pair.PA[k].detach().clone() for k in ORDER}
    again = pair.step(what='second step')
    assert pair.be.scans == 0 and again is quiet, 'the key did not survive a step of the library\'s own'
    rows = _rows_of([b for b in range(quiet.numel()) if int(again[b]) == 1], cases.N, dev)
    assert all(torch.equal(pair.PA[k][rows], before[k][rows]) for k in ORDER) and not torch.equal(pair.PA['means'], before['means'])


def check_invalidation(be, dev, monkeypatch):
    """Every way somebody else can write the moments changes the key: FusedAdam rescans, and the step equals the one of an optimizer that never had flags."""
    pair = _Pair(be, dev, monkeypatch)
    quiet = pair.step(what='first step')
    assert all(int(quiet[b]) == 1 for b in HIDDEN)

    def expect_rescan(what, hidden=HIDDEN, n_blocks=None):
        scans = pair.be.scans
        flags = pair.step(what=what)
        assert pair.be.scans == scans + 1, (what, 'no rescan')
        assert flags is not None and (n_blocks is None or flags.numel() == n_blocks)
        return flags

    # a torch in-place edit of a quiet block that the rasterizer does not reach: a stale flag would leave its momentum unapplied
    pair.both(lambda opt, P: opt.state[P['scales']]['exp_avg'][64 * 12 + 3].add_(0.01))
    flags = expect_rescan('exp_avg.add_')
    assert int(flags[12]) == 0 and all(int(flags[b]) == 1 for b in (14, 20, 23))

    def replace(opt, P):
        clone = opt.state[P['opacities']]['exp_avg'].clone()
        clone[64 * 20 + 63] = -0.02
        opt.state[P['opacities']]['exp_avg'] = clone
    pair.both(replace)
    flags = expect_rescan('replaced tensor')
    assert int(flags[20]) == 0 and all(int(flags[b]) == 1 for b in (14, 23))

    def round_trip(opt, P):
        saved = copy.deepcopy(opt.state_dict())
        saved['state'][5]['exp_avg_sq'][cases.N - 1, 3] = 1e-6               # rotations, the last Gaussian of the ragged block
        saved['state'][5]['exp_avg'][cases.N - 1, 3] = 1e-4
        opt.load_state_dict(saved)
    pair.both(round_trip)
    flags = expect_rescan('load_state_dict')
    assert int(flags[23]) == 0 and int(flags[14]) == 1

    # prune to a smaller N: new parameter and moment tensors, the blocks shift
    keep = torch.ones(cases.N, dtype=torch.bool)
    keep[:100] = False
    keep[900:937] = False
    keep = keep.to(dev)

    def prune(opt, P):
        for group in opt.param_groups:
            old = group['params'][0]
            entry = opt.state.pop(old)
            new = old.detach()[keep].clone().requires_grad_(True)
            group['params'][0] = new
            opt.state[new] = {'step': entry['step'], 'exp_avg': entry['exp_avg'][keep].clone(), 'exp_avg_sq': entry['exp_avg_sq'][keep].clone()}
            P[group['name']] = new
    pair.both(prune)
    n = int(keep.sum())
    flags = expect_rescan('prune', n_blocks=_blocks(n))
    ma, va = pair.moments(pair.A, pair.PA)
    assert pair.PA['means'].shape[0] == n and 0 < int(flags.sum()) < flags.numel()
    assert pair.step(what='after the prune') is flags


def check_hand_set_gradients(be, dev, monkeypatch):
    """`.grad` assigned by hand: no reached-block match, so no flags are handed over and nothing is skipped -- the result is the plain entry's."""
    import FasterGSCudaBackend as FGS
    from FasterGSCudaBackend import adam as A
    counting = _Counting(be)
    monkeypatch.setattr(A, 'default_backend', lambda: counting)
    n = 1483
    P, M, V = _state(n, dev)
    for k in ORDER:
        M[k].zero_()
        V[k].zero_()
    params = {k: P[k].clone().requires_grad_(True) for k in ORDER}
    opt = FGS.FusedAdam([{'params': [params[k]], 'lr': lr, 'name': k} for k, lr in zip(ORDER, LRS)], lr=0.0, eps=EPS)
    for step in (1, 2):
        G = _gradients(n, dev, (0, 7), seed=40 + step)
        for k in ORDER:
            params[k].grad = G[k].clone()
        opt.step()
        live_entry(be, G, P, M, V, step, None)
        assert opt.quiet_blocks() is None and counting.handed[-1] is None and counting.scans == 0
        for k in ORDER:
            assert torch.equal(params[k].detach(), P[k]) and torch.equal(opt.state[params[k]]['exp_avg'], M[k]) and torch.equal(opt.state[params[k]]['exp_avg_sq'], V[k]), k


def check_sentinel(be, dev, monkeypatch):
    """A gradient edit behind the version counter at the first element of a quiet, unreached block: the block is stepped after all and its flag cleared."""
    pair = _Pair(be, dev, monkeypatch)
    quiet = pair.step(what='first step')
    assert int(quiet[12]) == 1
    before = pair.PA['means'].detach().clone()

    def edit(grads):
        assert not bool(grads['means'][64 * 12:64 * 13].any())
        grads['means'].data[64 * 12, 0] += 0.5
    after = pair.step(edit_gradients=edit, what='sentinel')
    assert after is quiet and int(after[12]) == 0 and int(after[14]) == 1
    assert float((pair.PA['means'].detach()[64 * 12, 0] - before[64 * 12, 0]).abs()) > 0
    assert pair.be.handed[-2] is not None, 'the hand-over did not survive the edit behind the version counter: the sentinel was not exercised'


@pytest.mark.parametrize('n', [1483, 64, 1])
def test_sim_quiet_entry_equals_the_live_entry(sim_backend, n):
    check_equivalence(sim_backend, 'cpu', n)


def test_sim_scan_matches_a_torch_reduction(sim_backend):
    check_scan(sim_backend, 'cpu')


def test_sim_eps_zero_and_missing_live_flags_skip_nothing(sim_backend):
    check_eps_zero(sim_backend, 'cpu')


def test_sim_first_step_flags_are_ones_and_equal_the_scan(sim_backend, monkeypatch):
    check_first_step(sim_backend, 'cpu', monkeypatch)


def test_sim_foreign_writes_of_the_moments_rescan(sim_backend, monkeypatch):
    check_invalidation(sim_backend, 'cpu', monkeypatch)


def test_sim_hand_set_gradients_take_the_plain_step(sim_backend, monkeypatch):
    check_hand_set_gradients(sim_backend, 'cpu', monkeypatch)


def test_sim_sentinel_steps_a_quiet_block(sim_backend, monkeypatch):
    check_sentinel(sim_backend, 'cpu', monkeypatch)
