"""CPU-simulation twin of tests/test_gpu_unreached.py: the same scenes and checks (tests/unreached_cases.py) on the simulation build of the kernel sources."""
import unreached_cases as cases


def test_sim_wall_scene_gradients_zeros_statistics_and_flags(sim_backend):
    cases.check_backward(sim_backend, 'cpu')


def test_sim_hot_gaussian_is_tested_behind_the_fold(sim_backend, oracle):
    cases.check_hot(sim_backend, oracle, 'cpu')


def test_sim_optimizers_match_the_oracle_steps(sim_backend, monkeypatch):
    cases.check_optimizers(sim_backend, 'cpu', monkeypatch)


def test_sim_depth_only_pass_keeps_its_gradients(sim_backend):
    cases.check_depth_only(sim_backend, 'cpu')
