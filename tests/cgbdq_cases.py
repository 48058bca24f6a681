"""Shared pieces of the ControlGBDQ tests (test_cgbdq_host.py, test_gpu_cgbdq.py): the case list at the
tail layout's edges, seeded networks, the references (computed once per case and left unchanged), the
EXPLORE law and the stated dueling combination in numpy, csrc/cgbdq_tail.h's image restated in numpy,
and the raw ABI of the tail kernels with canaries behind every output."""
import copy
import ctypes

import numpy as np
import torch

from oracle import agent_oracle
from pbn_rl_amd import _lib
from pbn_rl_amd.attractors import find_attractors
from pbn_rl_amd.cgbdq import ControlGraphBranchingQNetwork, combine_heads, stacked_heads
from pbn_rl_amd.gbdq import edge_index
from pbn_rl_amd.network import Network
from pbn_rl_amd.spec import EnvSpec
from pbn_rl_amd.vector_env import control_to_flipmask
from tests import gbdq_cases as gc

CANARY, DEV = gc.CANARY, gc.DEV
MUSCLE_CTRL = [6, 7, 8, 10, 11, 12, 13, 14]      # train_control_gbdq.py:54 (node 14 of 14 genes: out of range)

# (network, C): K = N N = 1; 4 (no k tail); 9; 49; the 14-node muscle network with 17 head rows (crosses
# a 16-row tile); 15 rows; 31 and 33 rows; 33 nodes / 17 heads; 65 / 65; the ceiling (K = 16,384, 257 rows)
HEAD_CASES = [("size1", 1), ("size2", 2), ("size3", 3), ("pbn7", 3), ("muscle", 8), ("size16", 7), ("pbn28", 15),
              ("pbn28", 16), ("bb33", 17), ("size65", 65), ("size128", 128)]
# the cases whose greedy actions are held to float64 (n = 96)
ACTION_CASES = [("pbn7", 3), ("muscle", 8), ("pbn28", 16), ("bb33", 17), ("size65", 65)]
ACTION_N = 96
_SPECS = {}


def named_spec(name: str, **kw) -> EnvSpec:
    if name != "muscle":
        return gc.named_spec(name, **kw)
    key = (name, tuple(sorted(kw.items())))
    if key not in _SPECS:
        from tests.test_gpu_env import MUSCLE_FUNCS, MUSCLE_GENES
        net = Network.from_logic_functions(MUSCLE_GENES, MUSCLE_FUNCS, name="muscle")
        _SPECS[key] = EnvSpec(net, find_attractors(net, prob_bits=16), **kw)
    return _SPECS[key]


def ctrl_nodes(name: str, N: int, C: int):
    """The muscle network's own list (with its out-of-range entry); else C nodes spread over [0, N)."""
    return list(MUSCLE_CTRL) if name == "muscle" else [(k * N) // C for k in range(C)]


def make_cq(N: int, C: int, seed: int, bn: str = "random") -> ControlGraphBranchingQNetwork:
    """A seeded network, default-initialised tail; bn = "random" as gbdq_cases.make_q."""
    torch.manual_seed(seed)
    q = ControlGraphBranchingQNetwork(N, 2, C)
    with torch.no_grad():
        if bn == "random":
            for m in (q.bn1, q.bn2, q.bn3):
                m.weight.copy_((torch.rand(N) + 0.5) * torch.where(torch.rand(N) < 0.2, -1.0, 1.0))
                m.bias.copy_(torch.rand(N) - 0.5)
    return q


def heads64(q, front32: torch.Tensor) -> torch.Tensor:
    """The float64 module's stacked heads (B, 1 + 2 C) on the fp32 front."""
    q64 = copy.deepcopy(q).double()
    with torch.no_grad():
        return stacked_heads(q64.heads_raw(front32.double()))


def heads32(q, front32: torch.Tensor) -> torch.Tensor:
    with torch.no_grad():
        return stacked_heads(q.heads_raw(front32))


def e_ref_of(h32: torch.Tensor, h64: torch.Tensor) -> float:
    fin = torch.isfinite(h32) & torch.isfinite(h64)
    return float((h32.double() - h64)[fin].abs().max()) if bool(fin.any()) else 0.0


_REFS = {}


def case_q(name: str, C: int) -> ControlGraphBranchingQNetwork:
    """The network of a case (every n): make_cq(N, C, 60 + N + C); callers leave it unchanged."""
    key = (name, C)
    if key not in _REFS:
        N = named_spec(name).n
        _REFS[key] = make_cq(N, C, 60 + N + C)
    return _REFS[key]


def head_refs(name: str, C: int, n: int):
    """(spec, q, words, target, front32, h32, h64, e_ref) of one case: case_q(name, C), the fp32
    literal front of gbdq_cases.random_inputs(spec, n, 14) (the same tensor goes to both sides), the fp32
    CPU module's and the float64 module's stacked heads, and e_ref, their maximum distance."""
    key = (name, C, n)
    if key not in _REFS:
        spec = named_spec(name)
        q = case_q(name, C)
        words, target = gc.random_inputs(spec, n, 14)
        with torch.no_grad():
            front32 = gc.literal_front(q, gc.observation(spec, words, target), edge_index(spec), torch.float32).contiguous()
        h32, h64 = heads32(q, front32), heads64(q, front32)
        _REFS[key] = (spec, q, words, target, front32, h32, h64, e_ref_of(h32, h64))
    return _REFS[key]


def gap_keep(h64: torch.Tensor, e_ref: float) -> np.ndarray:
    """(n, C) bool: the float64 gap |q_0 - q_1| exceeds 16 e_ref (both values may be off by 8 e_ref)."""
    q = combine_heads(h64)
    return ((q[..., 0] - q[..., 1]).abs() > 16 * e_ref).numpy()


def greedy64(h64: torch.Tensor) -> np.ndarray:
    return torch.argmax(combine_heads(h64), dim=2).numpy()


# ---- the laws in numpy
def greedy_numpy(heads: np.ndarray) -> np.ndarray:
    """The stated combination and torch.argmax's rule in numpy fp32 on (n, 1 + 2 C) heads -> (n, C)."""
    f32 = np.float32
    h = np.asarray(heads, dtype=f32)
    with np.errstate(invalid="ignore", over="ignore"):
        v, a0, a1 = h[:, :1], h[:, 1::2], h[:, 2::2]
        mean = ((a0 + a1).astype(f32) / f32(2)).astype(f32)
        q0 = ((v + a0).astype(f32) - mean).astype(f32)
        q1 = ((v + a1).astype(f32) - mean).astype(f32)
    return agent_oracle.argmax_torch(np.stack([q0, q1], axis=-1)).astype(np.int32)


def explore_numpy(seed: int, step: int, env_offset: int, n: int, C: int, eps: float, mode: str):
    """(explore (n,) bool, values (n, C)) by the EXPLORE law: word 0 < floor(eps 2^32); "reference": zeros,
    "uniform": (word_{k + 1} 2) >> 32, words numbered across calls 0 .. ceil((C + 1) / 4) - 1."""
    w = agent_oracle.explore_words(seed, step, env_offset, n, calls=(C + 1 + 3) // 4)
    eps_u = int(np.floor(np.float64(np.float32(eps)) * 4294967296.0))
    explore = w[0].astype(np.uint64) < np.uint64(eps_u)
    vals = np.zeros((n, C), dtype=np.int32)
    if mode == "uniform":
        for k in range(C):
            vals[:, k] = (w[1 + k].astype(np.uint64) * np.uint64(2)) >> np.uint64(32)
    return explore, vals


def expected_actions(heads: np.ndarray, seed, step, env_offset, eps, mode) -> np.ndarray:
    n, C = heads.shape[0], (heads.shape[1] - 1) // 2
    explore, vals = explore_numpy(seed, step, env_offset, n, C, eps, mode)
    return np.where(explore[:, None], vals, greedy_numpy(heads)).astype(np.int32)


def expected_masks(state_words: np.ndarray, acts: np.ndarray, ctrl, N: int) -> np.ndarray:
    """control_to_flipmask of the in-range entries (an entry outside [0, N) sets no bit): (W, n) uint32."""
    valid = [k for k, c in enumerate(ctrl) if 0 <= c < N]
    st = torch.from_numpy(np.ascontiguousarray(state_words).view(np.int32))
    if not valid:
        return np.zeros_like(state_words)
    fm = control_to_flipmask(st, torch.from_numpy(np.ascontiguousarray(acts[:, valid])), [ctrl[k] for k in valid], N)
    return fm.numpy().view(np.uint32)


# ---- csrc/cgbdq_tail.h's image in numpy
def _al16(v):
    return (v + 15) & ~15


def _frag(Wm: np.ndarray) -> np.ndarray:
    """A dense layer (R, K) as MFMA fragments: element ((rt KG + kg) 64 + lane) 4 + j =
    W[rt 16 + (lane & 15)][kg 16 + 4 j + (lane >> 4)], zero beyond R and K."""
    R, K = Wm.shape
    Rp, Kp = _al16(R), _al16(K)
    P = np.zeros((Rp, Kp), dtype=np.float32)
    P[:R, :K] = Wm
    T = P.reshape(Rp // 16, 16, Kp // 16, 4, 4)          # rt, lane & 15, kg, j, lane >> 4
    return T.transpose(0, 2, 4, 1, 3).reshape(-1)        # rt, kg, lane >> 4, lane & 15, j


def tail_image_numpy(q) -> np.ndarray:
    w = lambda p: p.detach().cpu().numpy()  # noqa: E731
    wh = np.concatenate([w(q.value_head.weight)] + [w(h.weight) for h in q.adv_heads], axis=0)
    bh = np.concatenate([w(q.value_head.bias)] + [w(h.bias) for h in q.adv_heads])
    bhp = np.zeros(_al16(bh.shape[0]), dtype=np.float32)
    bhp[: bh.shape[0]] = bh
    parts = []
    for i in (0, 2, 4):
        parts += [_frag(w(q.model[i].weight)), w(q.model[i].bias)]
    parts += [_frag(wh), bhp]
    return np.concatenate(parts)


# ---- the raw ABI on the GPU
def _stream():
    return torch.cuda.current_stream().cuda_stream


def pack_tail(net, q, C: int):
    """pbn_cgbdq_pack into an image with 64 canary floats behind it: (image, its floats)."""
    L = _lib.load()
    nf = ctypes.c_int64()
    _lib.check(L.pbn_cgbdq_image_floats(net.handle, C, ctypes.byref(nf)), "pbn_cgbdq_image_floats")
    image = torch.full((nf.value + 64,), CANARY, dtype=torch.float32, device=DEV)
    flat = q.tail_flat().to(DEV)
    _lib.check(L.pbn_cgbdq_pack(net.handle, flat.data_ptr(), C, image.data_ptr(), _stream()), "pbn_cgbdq_pack")
    torch.cuda.synchronize()
    assert torch.equal(image[nf.value:].cpu(), torch.full((64,), CANARY))
    return image, nf.value


def run_heads(net, image, front: torch.Tensor, C: int) -> torch.Tensor:
    """pbn_cgbdq_heads on a (n, N N) front: (n, 1 + 2 C) on the CPU; 256 canary floats behind the output."""
    L = _lib.load()
    n, HR = front.shape[0], 1 + 2 * C
    fd = front.contiguous().to(DEV)
    out = torch.full((n * HR + 256,), CANARY, dtype=torch.float32, device=DEV)
    _lib.check(L.pbn_cgbdq_heads(net.handle, n, fd.data_ptr(), image.data_ptr(), C, out.data_ptr(), _stream()),
               "pbn_cgbdq_heads")
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[n * HR:], torch.full((256,), CANARY))
    return got[: n * HR].reshape(n, HR)


def run_flipmask(net, image, front: torch.Tensor, ctrl, state_words: np.ndarray, *, seed: int, step: int, eps: float,
                 mode: str, env_offset: int = 0, dev_scalars: bool = False):
    """pbn_cgbdq_flipmask: (actions (n, C) int32, masks (W, n) uint32) on the CPU, 64 canary words behind
    each.  ``dev_scalars``: the step and epsilon through d_step / d_epsilon (the by-value ones are then
    given as other values, which must not be read)."""
    from pbn_rl_amd.cgbdq import EXPLORE_MODES
    L = _lib.load()
    n, C = front.shape[0], len(ctrl)
    W = state_words.shape[0]
    fd = front.contiguous().to(DEV)
    cd = torch.tensor(list(ctrl), dtype=torch.int32, device=DEV)
    sd = torch.from_numpy(np.ascontiguousarray(state_words).view(np.int32)).to(DEV)
    acts = torch.full((n * C + 64,), -77, dtype=torch.int32, device=DEV)
    mask = torch.full((W * n + 64,), -78, dtype=torch.int32, device=DEV)
    step_t = torch.full((1,), step, dtype=torch.int64, device=DEV) if dev_scalars else None
    eps_t = torch.full((1,), eps, dtype=torch.float32, device=DEV) if dev_scalars else None
    _lib.check(L.pbn_cgbdq_flipmask(net.handle, seed, step + 5 if dev_scalars else step,
                                    step_t.data_ptr() if dev_scalars else None, env_offset, n, fd.data_ptr(),
                                    image.data_ptr(), C, cd.data_ptr(), EXPLORE_MODES[mode], 0.25 if dev_scalars else eps,
                                    eps_t.data_ptr() if dev_scalars else None, sd.data_ptr(), mask.data_ptr(),
                                    acts.data_ptr(), _stream()), "pbn_cgbdq_flipmask")
    torch.cuda.synchronize()
    a, m = acts.cpu(), mask.cpu()
    assert bool((a[n * C:] == -77).all()) and bool((m[W * n:] == -78).all())
    return a[: n * C].reshape(n, C).numpy(), m[: W * n].reshape(W, n).numpy().view(np.uint32)
