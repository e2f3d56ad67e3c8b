"""CPU test of bench.py's output contract: ONE JSON line on stdout and nothing else, whatever the libraries underneath print (RCCL writes a
version banner to stdout when it creates a communicator: file descriptor 1 points at stderr during the run, bench.py:main). Exercised here
through the only leg that needs no GPU, --cpu-baseline-only (the oracle timed on the S0 scene). Below it: the plain run (headline only) against
--full, and --dump-outputs, on the CPU simulation and (-m gpu) on the device."""
import json
import subprocess
import sys

import numpy as np
import pytest

import helpers


def test_cpu_baseline_only_prints_exactly_one_json_line_whatever_the_libraries_print():
    """np.sign (called inside the timed oracle loop) is wrapped to print a banner, as a library would: it must not reach stdout."""
    code = ("import sys, runpy; sys.argv = ['bench.py', '--cpu-baseline-only', '--scene', 'S0']; "
            "import numpy as _np; _orig = _np.sign\n"
            "def noisy(*a, **k):\n    print('BANNER: not json'); return _orig(*a, **k)\n"
            "_np.sign = noisy\n"
            f"runpy.run_path({str(helpers.REPO / 'bench.py')!r}, run_name='__main__')")
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert 'BANNER' in r.stderr
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[:500]
    d = json.loads(lines[0])
    assert d['kind'] == 'port' and d['unit'] == 'iters/s' and d['value'] > 0 and d['cores'] >= 1


def test_multi_rank_preflight_fails_fast_and_readably():
    """`bench.py --gpus N` on a node with fewer than N visible GPUs (here: none) stops before any rank is launched, with a message that names the
    remedy -- not a torchrun traceback or a hang in the first collective."""
    import subprocess
    import sys
    from pathlib import Path
    repo = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, str(repo / 'bench.py'), '--gpus', '2', '--no-extras', '--no-cpu-baseline'], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'GPU(s) visible' in r.stderr and '--shared-device' in r.stderr and r.stdout.strip() == ''


PLAIN_KEYS = {'metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data', 'config'}


def _bench_line(args, timeout=600):
    r = subprocess.run([sys.executable, str(helpers.REPO / 'bench.py')] + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[:500]
    return json.loads(lines[0])


def _check_dump(d, want_names):
    files = sorted(d.glob('*.npy'))
    assert {f.stem for f in files} == set(want_names)
    arrays = {f.stem: np.load(f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(f.stat().st_size for f in files) <= 64_000_000
    return arrays


def test_plain_run_times_the_headline_only_and_dumps_the_last_step_reproducibly(tmp_path):
    """A plain run (no --full) prints the headline and nothing that needs runs of its own; --steps sets the timed steps; --dump-outputs writes
    the outputs of the last two timed iterations, replayed on the seeded model, as float .npy, and two runs with the same arguments write the same arrays (the CPU simulation is deterministic).
    Through --sim: the multi-GPU step at world size 1, whose step returns the rendered image."""
    helpers.sim_backend()
    common = ['--sim', '--gpus', '1', '--scene', 'S0', '--n-gaussians', '300', '--steps', '2', '--warmup', '1']
    names = ['image', 'means', 'scales', 'rotations', 'opacities', 'sh_coefficients_0', 'sh_coefficients_rest', 'densification_info']
    runs = []
    for k in range(2):
        d = _bench_line(common + ['--dump-outputs', str(tmp_path / f'run{k}')])
        assert set(d) == PLAIN_KEYS and d['steps'] == 2 and d['warmup'] == 1 and 'SIMULATION' in d['data']
        assert d['metric'] == 'train_iters_per_sec' and d['higher_is_better'] is True and d['dtype'] == 'f32'
        assert d['ms_per_step'] > 0 and abs(d['value'] - 1e3 / d['ms_per_step']) < 1e-6 * d['value']
        runs.append(_check_dump(tmp_path / f'run{k}', names))
    assert runs[0]['means'].shape == (300, 3) and runs[0]['densification_info'].shape == (2, 300)
    assert all(np.array_equal(runs[0][k], runs[1][k]) for k in names)
    # the dump is the training path's: two Adam steps from the seeded scene moved the parameters (by at most two learning rates per step)
    # and the views' statistics were counted
    from harness.scenes import make_s0
    seeded, _view = make_s0(n=300)
    moved = np.abs(runs[0]['means'] - seeded['means'].numpy())
    assert 0 < moved.max() <= 2 * 2 * 1.6e-4 * 5.0 and runs[0]['densification_info'][0].max() >= 1


def test_full_run_keeps_the_measurements_beside_the_headline():
    helpers.sim_backend()
    d = _bench_line(['--sim', '--gpus', '1', '--scene', 'S0', '--n-gaussians', '300', '--steps', '1', '--warmup', '0', '--blocks', '2', '--full'])
    assert PLAIN_KEYS <= set(d) and d['steps'] == 1
    assert len(d['repeatability']['ms_per_step']) == 2 and d['roofline']['bound'] == 'hbm' and d['stage_ms_per_step']
    assert 'visible' in d['config'] and 'instances' in d['config']


@pytest.mark.gpu
def test_plain_run_on_the_device_dumps_the_single_gpu_iteration(tmp_path):
    """The single-GPU iteration (what `bench.py --gpus 1` times): the loss, parameters, Adam moments and densification statistics of the sampled
    Gaussians (all 1000 of S0 here). Two runs with the same arguments agree to rounding (the gradient sums use float atomics): 1e-5 of each
    array's scale, where chained training steps would drift by far more."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU visible')
    params = ['means', 'scales', 'rotations', 'opacities', 'sh_coefficients_0', 'sh_coefficients_rest']
    names = ['loss', 'densification_info'] + params + [f'{p}.{m}' for p in params for m in ('exp_avg', 'exp_avg_sq')]
    runs = []
    for k in range(2):
        d = _bench_line(['--gpus', '1', '--scene', 'S0', '--steps', '3', '--warmup', '1', '--dump-outputs', str(tmp_path / f'run{k}')])
        assert set(d) == PLAIN_KEYS and d['steps'] == 3 and d['config']['parallelism'] == 'single GPU' and d['data'] == 'synthetic'
        runs.append(_check_dump(tmp_path / f'run{k}', names))
    arrays = runs[0]
    assert arrays['loss'].size == 1 and 0 < float(arrays['loss'].reshape(-1)[0]) < 10
    assert arrays['means'].shape == (1000, 3) and arrays['sh_coefficients_rest.exp_avg_sq'].shape == (1000, 15, 3)
    assert float(abs(arrays['means.exp_avg']).max()) > 0
    for k in names:
        a, b = runs[0][k].astype(np.float64), runs[1][k].astype(np.float64)
        assert np.abs(a - b).max() <= 1e-5 * np.abs(a).max(), (k, np.abs(a - b).max(), np.abs(a).max())
