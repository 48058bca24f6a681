"""Shapes at which the learned-agent kernels change path, shared by the edge sweeps
(test_gpu_agent_edges.py, test_gpu_learn_edges.py, test_gpu_ddqn_edges.py) and by the Adam-state
tests (test_gpu_adam_state.py; the updates' shared inputs and float64 references: edge_updates.py).

The bundled networks pin N to 7, 28, 33 or 70, so A = N + 1 to {8, 29, 34, 71} and the state to
1-3 words.  The kernels are specialised on exactly these quantities; EDGE_N holds the last N
before and the first N after every boundary:
  a 16-tile of A          A = 16, 32, 64, 96, 128     (forward16, dqn_act_kernel, ddqn_fb_kernel, the
                                                      learner's Apad and its bilinear j-tile count NT)
  a 32-action qnet tile   A = 33, 65, 97              (qnet_tail_kernel<AT>)
  a state word            N = 32, 64, 96; 97 and 127 at W = 4

Float bounds.  The float comparisons of the sweeps are made against a float64 evaluation of the
PyTorch module on the same inputs, at the tolerances the project uses for the same quantity
(Q, y and heads rtol 1e-5 / atol 1e-5; loss and norm rtol 1e-5; gradients rtol 1e-3 / atol 1e-6).
Those were set for sums of at most 70 rows.  Where a shape's correct fp32 evaluation cannot meet
one, FLOAT_BOUNDS holds the bound used instead: 4 x the measured maximum error of the PyTorch fp32
module itself against the same float64 reference (the kernel evaluates the same sum in another
order at the same length), never anything derived from the kernel's output."""
import numpy as np

from tests.synthetic import random_spec

EDGE_N = [15, 16, 31, 32, 33, 64, 65, 95, 96, 97, 127]
ENVS = [96, 160]        # one qnet block with idle waves; a second, partial block
NO_TARGET = (5, 64)     # envs set to target 255

# (quantity, N[, arch]) -> (measured maximum error of the PyTorch fp32 module against float64, the
# bound used = 4 x that); absolute errors, except the priorities' (relative, as rtol).
# The DDQN priorities |w_b h_b| + rc of a row with a small TD error are ill-conditioned in fp32
# (h = delta^2 / 2 doubles delta's relative error, and delta is a difference of O(1) numbers): at
# these two shapes PyTorch's own fp32 update misses rtol 1e-5 (1.93e-5 and 3.64e-5; the kernel gave
# 3.62e-5 and 3.64e-5 on the same rows).  Every other figure of the sweeps met the project's
# tolerances.
FLOAT_BOUNDS = {
    ("ddqn_priorities", 64, (64, 16)): (1.93e-5, 7.72e-5),
    ("ddqn_priorities", 127, (16, 17)): (3.64e-5, 1.456e-4),
}

_SPECS = {}


def edge_spec(N, n_targets=4, **kw):
    """A seeded random PBN of N nodes with ``n_targets`` single-state targets (cached).  n_targets = 4
    keeps n_attr * N on pbn_bilinear_targets' LDS path up to N = 127; n_targets = 8 at N >= 70 takes
    its L2 path.  (random_spec never returns when n_targets > 2 ** N.)"""
    assert n_targets <= 2 ** N
    key = (N, n_targets, tuple(sorted(kw.items())))
    if key not in _SPECS:
        _SPECS[key] = random_spec(N, 50 + N, n_targets=n_targets, max_funcs=3, perturbation=0.05, **kw)
    return _SPECS[key]


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def check_close(name, got, ref64, mod32, rtol, atol, key=None):
    """``got`` (the kernel's fp32 result) against ``ref64`` (float64) at rtol / atol, or, where
    FLOAT_BOUNDS lists ``key``, within that absolute bound; prints the kernel's and the fp32
    module's (``mod32``) maximum errors first."""
    err = (got.double() - ref64).abs()
    e32 = (mod32.double() - ref64).abs().max().item() if mod32 is not None else float("nan")
    excess = (err - (atol + rtol * ref64.abs())).max().item()
    print(f"{name}: kernel max err {err.max().item():.3e}, fp32 module max err {e32:.3e}, "
          f"over rtol {rtol:g} / atol {atol:g} by {excess:.3e}")
    if key in FLOAT_BOUNDS:
        assert err.max().item() <= FLOAT_BOUNDS[key][1], (name, err.max().item(), FLOAT_BOUNDS[key])
    else:
        assert excess <= 0.0, (name, err.max().item(), e32)
