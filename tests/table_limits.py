"""What tests/test_table_limits_host.py (CPU) and tests/test_gpu_table_limits.py share: the specs at
the limits of the network descriptor (attractor hashes that need several probes, gate planes up
to the last one a byte addresses), the oracle chains the GPU tests compare with, and the
attractor hash restated in numpy.  Nothing here needs a GPU."""
import functools

import numpy as np

from oracle import oracle

from . import synthetic

HASH_CASES = ["hold28_a254", "hold40_a254", "hold70_a254", "hold100_a254", "hold20_s1000"]
COLLAPSE_CASES = ["collapse28", "collapse70"]
GATE_SIZES = [32, 64, 70, 96, 97, 128]
LDS_DEVICE_BYTES = 160 * 1024
# lds_settle of hold100_a254 is above LDS_DEVICE_BYTES: no pipelined settle launch exists for it
SETTLE_PIPE_CASES = [c for c in HASH_CASES if c != "hold100_a254"]
COLLAPSE_SEEDS = {28: 3, 70: 1}
# few perturbed env-steps (a perturbed env leaves the pattern family), yet enough for the gap bucket
# table, which the env_fast loops need (gap_exact 2: p above 2^-10 or so)
COLLAPSE_P = 0.002


@functools.lru_cache(maxsize=None)
def limit_spec(name: str, **kw):
    """The named spec; cached (a test must not change it)."""
    if name == "hold20_s1000":   # the seed: one state's probes run past the last slot and wrap to slot 0
        return synthetic.many_attractor_spec(20, 1000, [250, 1, 499, 250], seed=99, **kw)
    if name.startswith("hold"):
        n = int(name[4:name.index("_")])
        return synthetic.many_attractor_spec(n, 254, seed=n, **kw)
    if name.startswith("collapse"):
        n = int(name[8:])
        return synthetic.collapse_spec(n, COLLAPSE_SEEDS[n], **kw)
    if name == "gates70_a254":
        return synthetic.gate_hold_mix_spec(**kw)
    if name.startswith("gates"):
        return synthetic.gate_limit_spec(int(name[5:name.index("_")]), **kw)
    raise KeyError(name)


def attractor_words(spec):
    """(states (S, W) uint32, ids (S,), start (A + 1,)) in the descriptor's order."""
    start = spec.arrays["attractor_start"].astype(np.int64)
    S, W = int(start[-1]), spec.words
    states = spec.arrays["attractor_states"][:S * W].reshape(S, W).astype(np.uint32)
    ids = np.repeat(np.arange(len(start) - 1), np.diff(start))
    return states, ids, start


# ------------------------------------------------ the attractor hash, restated
def hash_table(scalars: dict, vectors: dict):
    """(keys (slots, W), ids (slots,)) of the image's hash section; the id of an empty slot is
    0xFFFFFFFF.  The slot stride is 2, 4, 4, 8 words for W = 1, 2, 3, 4."""
    W, bits = scalars["W"], scalars["hash_bits"]
    stride = {1: 2, 2: 4, 3: 4, 4: 8}[W]
    off = scalars["cdf_len"] + 4 * (scalars["n_nodes"] + 1)
    tab = np.asarray(vectors["tab"], dtype=np.uint32)[off:off + (stride << bits)].reshape(1 << bits, stride)
    assert off + (stride << bits) == scalars["att_off"]
    return tab[:, :W], tab[:, W]


def home_slots(scalars: dict, vectors: dict, states: np.ndarray) -> np.ndarray:
    """h = (sum_w s[w] * mult[w] mod 2^32) >> (32 - bits) of states (n, W)."""
    mult = np.asarray(vectors["hash_mult"], dtype=np.uint64)[:scalars["W"]]
    h = (states.astype(np.uint64) * mult).sum(axis=1) & np.uint64(0xFFFFFFFF)
    return (h >> np.uint64(32 - scalars["hash_bits"])).astype(np.int64)


def probe(scalars: dict, vectors: dict, states: np.ndarray):
    """(id or -1, slots read until found or hash_probes) of states (n, W): the lookup the kernels do,
    slot (h + p) & mask for p < hash_probes."""
    keys, ids = hash_table(scalars, vectors)
    mask = (1 << scalars["hash_bits"]) - 1
    h = home_slots(scalars, vectors, states)
    found = np.full(len(states), -1, dtype=np.int64)
    reads = np.full(len(states), scalars["hash_probes"], dtype=np.int64)
    for p in range(scalars["hash_probes"]):
        slot = (h + p) & mask
        hit = (keys[slot] == states).all(axis=1) & (ids[slot] != 0xFFFFFFFF) & (found < 0)
        found[hit] = ids[slot][hit]
        reads[hit] = p + 1
    return found, reads


def displaced_states(scalars: dict, vectors: dict, spec) -> np.ndarray:
    """Indices of the attractor states that do not sit in their home slot."""
    states, _, _ = attractor_words(spec)
    return np.nonzero(probe(scalars, vectors, states)[1] > 1)[0]


# ------------------------------------------------ given-mask chains on the hash cases
GIVEN_N, GIVEN_SEED, GIVEN_OFFSET, GIVEN_STEPS = 1024, 77, 64, 5


def given_targets(spec, n: int) -> np.ndarray:
    """Targets for the first landing (env e on state e mod S): alternately the attractor landed
    on and another one (every id comes up on either side, 0 and the last included), and no
    target (255) for every 64th env."""
    _, ids, _ = attractor_words(spec)
    S, A = len(ids), len(spec.attractors)
    e = np.arange(n)
    landed = ids[e % S]
    same = (e // S + e) % 2 == 0
    tg = np.where(same, landed, (landed + 1 + (e // 2) % (A - 1)) % A).astype(np.uint8)
    tg[5::64] = 255
    return tg


@functools.lru_cache(maxsize=None)
def given_chain(name: str, perturbation: float, settle: int, mode: int) -> dict:
    """GIVEN_STEPS oracle steps of GIVEN_N envs whose flip masks are chosen from the chain itself:
    step 0 puts env e on attractor state e mod S; step 1 on a near miss (another attractor state
    with one bit of word 0 flipped, or one bit of word W - 1, or a random state); step 2 on a
    state of the env's current target (every other env) or on some other attractor state; step 3
    on near misses again; step 4 on state (e + S / 2) mod S.  Under perturbation the env lands a
    few bits off.  Cached: the GPU tests of one case compare with the same chain."""
    spec = limit_spec(name, perturbation=perturbation, settle=settle)
    n, N, W = GIVEN_N, spec.n, spec.words
    states, ids, start = attractor_words(spec)
    S, A = len(ids), len(spec.attractors)
    sizes = np.diff(start)
    st, tg, t = oracle.reset(spec, GIVEN_SEED, 0, GIVEN_OFFSET, n)
    tg = given_targets(spec, n)
    init = (st.copy(), tg.copy(), t.copy())
    rng = np.random.default_rng(S + N)
    e = np.arange(n)
    last_bits = N - 32 * (W - 1)

    def near(k):
        want = states[(e * 5 + k) % S].T.copy()                       # (W, n)
        bit0 = np.uint32(1) << ((e // 3 + k) % min(32, N)).astype(np.uint32)
        bitl = np.uint32(1) << ((e // 3 + 3 * k) % last_bits).astype(np.uint32)
        want[0] ^= np.where(e % 3 == 0, bit0, 0).astype(np.uint32)
        want[W - 1] ^= np.where(e % 3 == 1, bitl, 0).astype(np.uint32)
        rnd = rng.integers(0, 2 ** 32, size=(W, n), dtype=np.uint64).astype(np.uint32)
        if N % 32:
            rnd[W - 1] &= np.uint32((1 << (N % 32)) - 1)
        return np.where(e % 3 == 2, rnd, want)

    flips, refs = [], []
    for k in range(GIVEN_STEPS):
        if k == 0:
            want = states[e % S].T
        elif k in (1, 3):
            want = near(k)
        elif k == 2:
            has = tg < A
            a = np.where(has, tg, 0).astype(np.int64)
            own = start[a] + e % sizes[a]
            want = states[np.where(has & (e % 2 == 0), own, (e * 7 + 3) % S)].T
        else:
            want = states[(e + S // 2) % S].T
        flip = np.ascontiguousarray(st ^ want)
        ref = oracle.step(spec, GIVEN_SEED, 1 + k, GIVEN_OFFSET, st, flip, tg, t, mode)
        flips.append(flip)
        refs.append(ref)
        st, tg, t = ref["state_out"], ref["target"], ref["t"]
    return {"spec": spec, "init": init, "flips": flips, "refs": refs, "mode": mode}


# ------------------------------------------------ random-action chains on collapse_spec
# (spec keywords, envs, steps) of the GPU tests' run_pair and run_rollout_pair calls, and those
# helpers' seeds and env offsets: the host test walks the same chains through the oracle alone
COLLAPSE_STEP = dict(n=2048, steps=6, seed=12345, env_offset=0)
COLLAPSE_ROLLOUT = dict(n=2048, steps=6, seed=4242, env_offset=2048)


def collapse_kw(settle: int = 0) -> dict:
    return dict(perturbation=COLLAPSE_P, horizon=20, settle=settle)


def random_action_chain(spec, mode: int, *, n: int, steps: int, seed: int, env_offset: int) -> list:
    """The oracle's outputs of every step of run_pair / run_rollout_pair in a random-action mode."""
    st, tg, t = oracle.reset(spec, seed, 0, env_offset, n)
    zero, refs = np.zeros_like(st), []
    for k in range(steps):
        ref = oracle.step(spec, seed, 1 + k, env_offset, st, zero, tg, t, mode)
        refs.append(ref)
        st, tg, t = ref["state_out"], ref["target"], ref["t"]
    return refs
