"""test_gpu_adam_state.py's SEEDS on the CPU: on a pure float64 PyTorch trajectory (the module, the
update and torch.optim.Adam, no kernel) from each trajectory's ring and row seeds, the smallest top-2
gap of Q(s') stays above 1e-3 at all four updates, so the kernel's fp32 trajectory keeps the 1e-4
its test asserts; the clipping trajectory clips at every update."""
import pytest

from tests.adam_reference import STEPS
from tests.edge_updates import bdq_trajectory_gaps, ddqn_trajectory_gaps
from tests.test_gpu_adam_state import BDQ_TRAJ, DDQN_B, DDQN_TRAJ, SEEDS


@pytest.mark.parametrize("N,B,K,lr", BDQ_TRAJ)
def test_bdq_trajectory_seeds_keep_the_argmax_apart(N, B, K, lr):
    gaps = bdq_trajectory_gaps(N, B, K, lr, *SEEDS[("bdq", N, B, K, lr)], steps=STEPS)
    print(f"bdq N={N} B={B} K={K} lr={lr:g}: top-2 gaps {['%.3e' % g for g in gaps]}")
    assert len(gaps) == STEPS and min(gaps) > 1e-3, gaps


@pytest.mark.parametrize("N,arch,lr,clip", DDQN_TRAJ)
def test_ddqn_trajectory_seeds_keep_the_argmax_apart(N, arch, lr, clip):
    gaps, norms, max_norm = ddqn_trajectory_gaps(N, arch, DDQN_B, lr, *SEEDS[("ddqn", N, arch, lr, clip)], steps=STEPS,
                                                 clip_half=clip)
    print(f"ddqn N={N} {arch} lr={lr:g} clip={clip}: top-2 gaps {['%.3e' % g for g in gaps]}, norms "
          f"{['%.3e' % x for x in norms]}, max_norm {max_norm:.3e}")
    assert len(gaps) == STEPS and min(gaps) > 1e-3, gaps
    if clip:
        assert min(norms) > 1.1 * max_norm, (norms, max_norm)      # (a margin for the kernel's own trajectory)
