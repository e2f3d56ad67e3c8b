"""The CUDA-on-CPU stand-ins (oracle/cuda_on_cpu: what the reference's kernels are compiled against for tests/test_reference_pin.py) against the
documented behaviour of what they stand in for, on own kernels: two-dimensional blocks and grids, 32-wide tile collectives with work-items of the
tile that have returned, rank-ordered atomics, BlockReduce, the stable radix sort over a bit range, CUB's size-query convention, the scans, the
device intrinsics. Needs no reference tree. One g++ compile (3 s) and a run of milliseconds."""
import subprocess

import helpers
from oracle import build_ref


def test_stand_ins_behave_as_documented(tmp_path):
    root = helpers.REPO / 'oracle' / 'cuda_on_cpu'
    exe = tmp_path / 'cuda_on_cpu_selftest'
    subprocess.run(['g++', '-std=c++17', '-O1', '-ffp-contract=off', '-w', f'-I{root}', f'-I{helpers.REPO / "tests" / "sim" / "include"}',
                    str(root / 'selftest.cpp'), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == 'ok', run.stdout + run.stderr


def test_launch_rewrite_is_mechanical():
    """The recipe's only change to the reference's host files: the launch syntax, template arguments kept, nothing else touched."""
    text = 'a::k_cu<KeyT><<<div_round_up(n, c::b), c::b>>>(\n    x, y);\nfoo<<<grid, block>>>(z);\nint v = a << 3;'
    out, n = build_ref.rewrite_launches(text)
    assert n == 2 and out == ('cuda_on_cpu::launch(div_round_up(n, c::b), c::b).run(a::k_cu<KeyT>, \n    x, y);\n'
                              'cuda_on_cpu::launch(grid, block).run(foo, z);\nint v = a << 3;')
