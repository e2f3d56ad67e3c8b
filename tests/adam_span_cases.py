"""Cases shared by tests/test_adam_spans.py (CPU simulation) and tests/test_gpu_adam_spans.py (MI355X): K13 with a workgroup per SPAN of C chunks of 1024
floats (csrc/adam.hip). The product library has C as a constant (1, at four pieces per thread: its chunk is 4096 floats, a span of 4 in the
terms of check_cases_bite); the dev library takes it from fgs_debug_set_option(15, C), and C = 1 there is the grid
of one workgroup per chunk that the kernel had before spans.

Expected values never come from the code under test:
  (a) oracle.adam_step applied densely to every element -- bit for bit on the simulation (+0 == -0 where flags let the kernel skip a store), rel_inf < 1e-6
      on the GPU (the bar of tests/test_gpu_parity.py);
  (b) the dev library at C = 1 -- the same values on both, flags included. This is the grid of one workgroup per chunk, not the kernel of before: it
      shares the prologue and the LDS plans with the code under test, so (a) is the independent reference and (b) holds the span lengths to each other.
      C = 32 is the one length at which the prologue's stride loop runs a second time (`opacities`: 512 blocks per span).
The flags a step must leave are worked out here from the reached sets alone.

Shapes, the smallest at which spans can go wrong for every C of SWEEP (no case depends on the product's constant):
  flagless groups of 1024 c - 1, 1024 c, 1024 c + 1 and 1024 c + 5 floats for c in SWEEP, 8 per launch: a ragged last span, a last span that is one tail
      piece, scalar tails of 1 and of 3 floats, groups of exactly one span;
  the six tensors of the model at N = 1483 (the scheme of tests/test_quiet_blocks.py) and N = 33 291 = 520 blocks + 11 rows, five steps with flags. What
      the reached sets of N = 33 291 put where is asserted for every C of SWEEP by check_cases_bite, without running any kernel."""
from __future__ import annotations

import contextlib
import re
from pathlib import Path

import numpy as np
import torch

import helpers
import unreached_cases as cases

ORDER, LRS = cases.ORDER, cases.LRS
ROW = {'means': (3,), 'sh_coefficients_0': (1, 3), 'sh_coefficients_rest': (15, 3), 'opacities': (1,), 'scales': (3,), 'rotations': (4,)}
ROW_LEN = {k: int(np.prod(ROW[k])) for k in ORDER}
GUARD, FILL = 5, 7               # bytes behind the flag array that must keep their fill value
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15
SPAN_OPTION, SWEEP = 15, (1, 2, 4, 8, 16, 32)
DEFAULT_SPAN = int(re.search(r'FGS_SWITCH\(g_adam_span,\s*(\d+)\)', (Path(__file__).resolve().parent.parent / 'faster-gaussian-splatting_amd' / 'csrc' /
                                                                      'fgs_kernels.h').read_text()).group(1))

# not_quiet: blocks that start with non-zero moments; reached: the blocks whose gradient is needed in step 1 .. 5; never: quiet and never reached, carries
# a -0.0 moment that only a store would turn into +0; sentinel: (step, tensor, block) -- the first gradient float of a quiet block with live flag 0 is set
# behind the flags, in that tensor alone.
# N = 33 291, per C of SWEEP (check_cases_bite): step 1 leaves every span of `opacities` but the one with blocks 496 .. 511 -- its LAST chunk -- idle;
# step 2 has block 0 as the only work of span 0 -- its FIRST chunk -- in `means`, with idle spans before the span of blocks 497 .. 501; 501 never gets a
# gradient (momentum only); block 11 of `sh_coefficients_rest` and block 170 of `means` lie across the span border at float 32 768; 520 is the ragged block.
SCENARIOS = {
    1483: dict(not_quiet=(1, 2, 5, 9), reached=((0, 1, 22), (1, 3), (7, 2, 23), (3,), (0, 9)), never=10, sentinel=(4, 'scales', 12)),
    33291: dict(not_quiet=(497, 501), reached=((497, 500), (0,), (11, 170, 520), (3,), (0, 11, 520)), never=400, sentinel=(4, 'scales', 250)),
}


@contextlib.contextmanager
def span(be, c):
    """The dev library's span length for the calls inside; c = None leaves the library as it is (the product has no option)."""
    if c is None:
        yield
        return
    assert be.lib.fgs_debug_set_option(SPAN_OPTION, c) == 0, be.lib.fgs_last_error()
    try:
        yield
    finally:
        be.lib.fgs_debug_set_option(SPAN_OPTION, DEFAULT_SPAN)


def blocks(n):
    return (n + 63) // 64


# ---- which chunks of which span have work: the model of the grid, for check_cases_bite ----------------------------------------------------------------
def span_work(n, row_len, c, busy):
    """{span: set of chunk indices inside the span that hold floats of a busy block}, and the number of chunks of every span, for a [n, row_len] tensor."""
    total, work = n * row_len, {}
    for b in busy:
        first, last = 64 * row_len * b, min(64 * row_len * (b + 1), total) - 1
        for chunk in range(first // 1024, last // 1024 + 1):
            work.setdefault(chunk // c, set()).add(chunk % c)
    n_chunks = (total + 1023) // 1024
    length = {s: min(c, n_chunks - s * c) for s in range((n_chunks + c - 1) // c)}
    return work, length


def check_cases_bite():
    n, sc = 33291, SCENARIOS[33291]
    nonquiet, per_step = set(sc['not_quiet']), []
    for reached in sc['reached']:
        per_step.append(nonquiet | set(reached))           # a span has work where a block is reached or carries momentum
        nonquiet |= set(reached)
    for c in SWEEP:
        first_only = last_only = gap = False
        for busy in per_step:
            for k in ORDER:
                work, length = span_work(n, ROW_LEN[k], c, busy)
                first_only |= any(length[s] > 1 and chunks == {0} for s, chunks in work.items())
                last_only |= any(length[s] > 1 and chunks == {length[s] - 1} for s, chunks in work.items())
                gap |= any(s not in work for s in range(min(work), max(work)))
        assert gap, ('no idle span between two busy ones', c)
        assert c == 1 or (first_only and last_only), ('no span whose only work is its first / its last chunk', c, first_only, last_only)
        for k, b in (('sh_coefficients_rest', 11), ('means', 170)):
            assert any(b in reached for reached in sc['reached'])
            assert (64 * ROW_LEN[k] * b) // (1024 * c) != (64 * ROW_LEN[k] * (b + 1) - 1) // (1024 * c), ('block not on a span border', k, b, c)
    assert any(blocks(n) - 1 in reached for reached in sc['reached']) and n % 64 != 0
    assert n * ROW_LEN['opacities'] > 1024 * max(SWEEP) and n * ROW_LEN['sh_coefficients_rest'] > 24 * 1024 * max(SWEEP)
    assert 501 in sc['not_quiet'] and not any(501 in reached for reached in sc['reached'])


# ---- flagless groups ------------------------------------------------------------------------------------------------------------------------------------
FLAGLESS_SIZES = tuple(1024 * c + d for c in SWEEP for d in (-1, 0, 1, 5))
FLAGLESS_STEPS = (3, 4)
_cache = {}


def _flagless_inputs():
    rng = np.random.default_rng(7)
    G = [[(rng.standard_normal(s) * 1e-2).astype(np.float32) for s in FLAGLESS_SIZES] for _ in FLAGLESS_STEPS]
    P, M = ([rng.standard_normal(s).astype(np.float32) * scale for s in FLAGLESS_SIZES] for scale in (1.0, 1e-3))
    V = [(rng.random(s) * 1e-6 + 1e-7).astype(np.float32) for s in FLAGLESS_SIZES]
    return G, P, M, V


def _lr(i):
    return LRS[i % len(LRS)]


def flagless_oracle(oracle):
    """(a): [params, exp_avgs, exp_avg_sqs] after FLAGLESS_STEPS, every element stepped by the oracle. Computed once."""
    if 'flagless' not in _cache:
        G, P, M, V = _flagless_inputs()
        for step, g in zip(FLAGLESS_STEPS, G):
            for i in range(len(FLAGLESS_SIZES)):
                oracle.adam_step(g[i], P[i], M[i], V[i], step, _lr(i), BETA1, BETA2, EPS)
        _cache['flagless'] = [np.concatenate(t) for t in (P, M, V)]
    return _cache['flagless']


def run_flagless(be, dev, c=None):
    G, P, M, V = _flagless_inputs()
    P, M, V = ([torch.from_numpy(x).to(dev) for x in t] for t in (P, M, V))
    with span(be, c):
        for step, g in zip(FLAGLESS_STEPS, G):
            g = [torch.from_numpy(x).to(dev) for x in g]
            for at in range(0, len(FLAGLESS_SIZES), 8):                       # at most 8 groups per launch
                sl = slice(at, at + 8)
                be.adam_step_multi(g[sl], P[sl], M[sl], V[sl], [step] * len(g[sl]), [_lr(i) for i in range(at, at + len(g[sl]))], BETA1, BETA2, EPS)
    return [np.concatenate([x.cpu().numpy() for x in t]) for t in (P, M, V)]


def same_bits(got, ref, label):
    for name, a, b in zip(('param', 'exp_avg', 'exp_avg_sq'), got, ref):
        assert a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (label, name)


def close_to_oracle(got, ref, label):
    for name, a, b in zip(('param', 'exp_avg', 'exp_avg_sq'), got, ref):
        assert helpers.rel_inf(a, b) < 1e-6, (label, name)


# ---- the six tensors with live and quiet flags ------------------------------------------------------------------------------------------------------------
def _rows_of(block_list, n):
    rows = np.zeros(blocks(n) * 64, dtype=bool)
    for b in block_list:
        rows[64 * b:64 * b + 64] = True
    return rows[:n]


def _model_inputs(n):
    """Initial P, M, V and the five steps' gradients and live flags, as numpy arrays."""
    sc, rng = SCENARIOS[n], np.random.default_rng(3)
    busy = _rows_of(sc['not_quiet'], n)
    P = {k: rng.standard_normal((n,) + ROW[k]).astype(np.float32) for k in ORDER}
    M = {k: (rng.standard_normal((n,) + ROW[k]) * 1e-3).astype(np.float32) for k in ORDER}
    V = {k: (rng.random((n,) + ROW[k]) * 1e-6 + 1e-7).astype(np.float32) for k in ORDER}
    for k in ORDER:
        M[k][~busy], V[k][~busy] = 0.0, 0.0
    M['sh_coefficients_rest'][64 * sc['never'] + 31, 7, 1] = -0.0
    steps = []
    for step, reached in enumerate(sc['reached'], start=1):
        rows = _rows_of(reached, n)
        G = {k: (rng.standard_normal((n,) + ROW[k]) * 1e-2).astype(np.float32) for k in ORDER}
        for k in ORDER:
            G[k][~rows] = 0.0
        live = np.zeros(blocks(n), np.uint8)
        live[list(reached)] = 1
        if sc['sentinel'][0] == step:
            _, tensor, b = sc['sentinel']
            assert live[b] == 0
            G[tensor][64 * b].reshape(-1)[0] = 0.5                           # the block's first float: the one the kernel looks at behind a 0 flag
        steps.append((G, live))
    return P, M, V, steps


def quiet_reference(M, V, n):
    busy = np.zeros(blocks(n) * 64, dtype=bool)
    for k in ORDER:
        for t in (M[k], V[k]):
            busy[:n] |= ~(t.reshape(n, -1) == 0).all(axis=1)
    return (~busy.reshape(-1, 64).any(axis=1)).astype(np.uint8)


def model_expected(oracle, n):
    """(a) per step: P, M, V with every element stepped by the oracle, and the quiet flags the step must leave. Computed once per n."""
    if ('model', n) not in _cache:
        P, M, V, steps = _model_inputs(n)
        quiet, out = quiet_reference(M, V, n), []
        assert int(quiet.sum()) == blocks(n) - len(SCENARIOS[n]['not_quiet'])
        for step, (G, live) in enumerate(steps, start=1):
            for k, lr in zip(ORDER, LRS):
                oracle.adam_step(G[k].reshape(-1), P[k].reshape(-1), M[k].reshape(-1), V[k].reshape(-1), step, lr, BETA1, BETA2, EPS)
            quiet = quiet * (1 - live)                                        # 1 -> 0 where a gradient is needed, never back, nothing else
            if SCENARIOS[n]['sentinel'][0] == step:
                quiet[SCENARIOS[n]['sentinel'][2]] = 0
            out.append(({k: P[k].copy() for k in ORDER}, {k: M[k].copy() for k in ORDER}, {k: V[k].copy() for k in ORDER}, quiet.copy()))
        _cache[('model', n)] = out
    return _cache[('model', n)]


def run_model(be, dev, n, c=None):
    """The five steps through adam_step_multi with live and quiet flags; per step (P, M, V, the flag buffer with its guard bytes) as numpy arrays."""
    P, M, V, steps = _model_inputs(n)
    nb = blocks(n)
    Q = torch.full((nb + GUARD,), FILL, dtype=torch.uint8)
    Q[:nb] = torch.from_numpy(quiet_reference(M, V, n))
    Q = Q.to(dev)
    P, M, V = ({k: torch.from_numpy(t[k]).to(dev) for k in ORDER} for t in (P, M, V))
    out = []
    with span(be, c):
        for step, (G, live) in enumerate(steps, start=1):
            G = {k: torch.from_numpy(G[k]).to(dev) for k in ORDER}
            be.adam_step_multi([G[k] for k in ORDER], *[[t[k] for k in ORDER] for t in (P, M, V)], [step] * 6, LRS, BETA1, BETA2, EPS,
                               live_blocks=torch.from_numpy(live).to(dev), quiet_blocks=Q[:nb])
            out.append(tuple({k: t[k].cpu().numpy().copy() for k in ORDER} for t in (P, M, V)) + (Q.cpu().numpy().copy(),))
    return out


def check_model(got, n, expected, exact, parent=None):
    """got against (a) `expected` (model_expected; exact: by value, else rel_inf < 1e-6) and, where given, against (b) `parent` (run_model at C = 1)."""
    nb, sc = blocks(n), SCENARIOS[n]
    at = (64 * sc['never'] + 31, 7, 1)
    for step, (P, M, V, Q) in enumerate(got, start=1):
        eP, eM, eV, quiet = expected[step - 1]
        for what, a, e in (('param', P, eP), ('exp_avg', M, eM), ('exp_avg_sq', V, eV)):
            for k in ORDER:
                assert not np.isnan(a[k]).any()
                if exact:
                    assert np.array_equal(a[k], e[k]), (n, step, what, k)      # value comparison: +0 == -0
                else:
                    assert helpers.rel_inf(a[k], e[k]) < 1e-6, (n, step, what, k)
        assert np.array_equal(Q[:nb], quiet), (n, step, 'flags', np.nonzero(Q[:nb] != quiet)[0][:8])
        assert (Q[nb:] == FILL).all(), 'the step wrote behind the flag array'
        assert (Q[:nb] <= quiet_reference(M, V, n)).all(), 'a block flagged quiet has a non-zero moment'
        # the never-reached quiet block was not stored to: its -0.0 moment is still -0.0 (the full step leaves +0 there)
        assert np.signbit(M['sh_coefficients_rest'][at]) and not np.signbit(eM['sh_coefficients_rest'][at])
        if parent is not None:
            for a, b, what in zip((P, M, V), parent[step - 1][:3], ('param', 'exp_avg', 'exp_avg_sq')):
                for k in ORDER:
                    assert np.array_equal(a[k], b[k]), (n, step, what, k, 'differs from C = 1')
            assert np.array_equal(Q, parent[step - 1][3]), (n, step, 'flags differ from C = 1')
    _, tensor, b = sc['sentinel']
    others = [k for k in ORDER if k != tensor]
    first = got[sc['sentinel'][0] - 2], got[sc['sentinel'][0] - 1]
    assert not np.array_equal(first[0][0][tensor][64 * b], first[1][0][tensor][64 * b]), 'the sentinel did not make its tensor step the block'
    assert all(np.array_equal(first[0][0][k][64 * b:64 * b + 64], first[1][0][k][64 * b:64 * b + 64]) for k in others)


def check_all_quiet(be, dev, c=None):
    """All moments zero (two of them -0.0), no live block, zero gradients, every flag 1: no byte of parameters, moments or flags changes."""
    n, nb = 1483, blocks(1483)
    rng = np.random.default_rng(11)
    P = {k: rng.standard_normal((n,) + ROW[k]).astype(np.float32) for k in ORDER}
    M = {k: np.zeros((n,) + ROW[k], np.float32) for k in ORDER}
    V = {k: np.zeros((n,) + ROW[k], np.float32) for k in ORDER}
    M['sh_coefficients_rest'][64 * 10 + 31, 7, 1] = -0.0
    M['means'][n - 1, 2] = -0.0                                               # the tensor's scalar tail (4449 floats)
    tP, tM, tV = ({k: torch.from_numpy(t[k].copy()).to(dev) for k in ORDER} for t in (P, M, V))
    G = {k: torch.zeros((n,) + ROW[k], device=dev) for k in ORDER}
    Q = torch.full((nb + GUARD,), FILL, dtype=torch.uint8)
    Q[:nb] = 1
    Q = Q.to(dev)
    with span(be, c):
        be.adam_step_multi([G[k] for k in ORDER], *[[t[k] for k in ORDER] for t in (tP, tM, tV)], [1] * 6, LRS, BETA1, BETA2, EPS,
                           live_blocks=torch.zeros(nb, dtype=torch.uint8, device=dev), quiet_blocks=Q[:nb])
    for before, after, what in ((P, tP, 'param'), (M, tM, 'exp_avg'), (V, tV, 'exp_avg_sq')):
        for k in ORDER:
            assert np.array_equal(before[k].view(np.uint32), after[k].cpu().numpy().view(np.uint32)), (what, k)
    q = Q.cpu().numpy()
    assert (q[:nb] == 1).all() and (q[nb:] == FILL).all()


def check_option_range(be):
    for bad in (0, -1, 33):
        assert be.lib.fgs_debug_set_option(SPAN_OPTION, bad) == -1 and b'span' in be.lib.fgs_last_error()
    for c in SWEEP:
        assert be.lib.fgs_debug_set_option(SPAN_OPTION, c) == 0
    assert be.lib.fgs_debug_set_option(SPAN_OPTION, DEFAULT_SPAN) == 0
