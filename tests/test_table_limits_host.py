"""The network descriptor at its documented limits, on the CPU: the attractor hash of images that
need more than one probe, restated in numpy and read back slot by slot, and the conditions that
tests/test_gpu_table_limits.py relies on, checked with the oracle alone (its attractor_of is a
linear scan over the descriptor's states: no hash)."""
import numpy as np
import pytest

from pbn_rl_amd import _lib

from . import table_limits as tl
from .test_net_image import build_shim, compile_raw

PROBE_CASES = tl.HASH_CASES + tl.COLLAPSE_CASES + ["gates70_a254"]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("table_limits"))


@pytest.fixture(scope="module")
def image(shim):
    cache = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in cache:
            rc, err, scalars, vectors = compile_raw(shim, tl.limit_spec(name, **kw))
            assert rc == 0, err
            cache[key] = (scalars, vectors)
        return cache[key]
    return get


@pytest.mark.parametrize("name", PROBE_CASES)
def test_hash_probe_restated(image, name):
    """hash_mult, hash_bits, hash_probes and the hash section of the image: every attractor state
    is found with its own id within hash_probes slots, some state needs all of them, every other
    slot is empty, and 4,096 random states that are no attractor states are found nowhere."""
    sc, vec = image(name)
    spec = tl.limit_spec(name)
    states, ids, _ = tl.attractor_words(spec)
    assert sc["hash_probes"] >= 2 and sc["hash_bits"] == 12
    found, reads = tl.probe(sc, vec, states)
    assert np.array_equal(found, ids)
    assert reads.max() == sc["hash_probes"] and reads.min() == 1
    keys, slot_ids = tl.hash_table(sc, vec)
    mask = (1 << sc["hash_bits"]) - 1
    taken = (tl.home_slots(sc, vec, states) + reads - 1) & mask
    assert len(set(taken.tolist())) == len(states)
    empty = np.ones(len(slot_ids), dtype=bool)
    empty[taken] = False
    assert (slot_ids[empty] == 0xFFFFFFFF).all() and not keys[empty].any()
    rng = np.random.default_rng(sc["n_nodes"])
    rnd = rng.integers(0, 2 ** 32, size=(4096, sc["W"]), dtype=np.uint64).astype(np.uint32)
    if sc["n_nodes"] % 32:
        rnd[:, -1] &= np.uint32((1 << (sc["n_nodes"] % 32)) - 1)
    known = {tuple(s) for s in states.tolist()}
    rnd = rnd[[tuple(s) not in known for s in rnd.tolist()]]
    assert len(rnd) >= 4000                                   # N = 20: a few of 2^20 states are attractor states
    assert (tl.probe(sc, vec, rnd)[0] == -1).all()
    # a lookup capped at one probe, or one that forgets the wrap, would miss states: both kinds exist
    assert (reads > 1).sum() >= 4


def test_a_probe_sequence_wraps(image):
    """(h + p) & mask: hold20_s1000's seed is chosen so that a state displaced past the last slot
    sits at the table's start (the given-mask chains visit it like every other state)."""
    sc, vec = image("hold20_s1000")
    states, _, _ = tl.attractor_words(tl.limit_spec("hold20_s1000"))
    h, reads = tl.home_slots(sc, vec, states), tl.probe(sc, vec, states)[1]
    assert (h + reads - 1 > (1 << sc["hash_bits"]) - 1).sum() >= 1
    assert sc["hash_probes"] == 4 and (reads == 4).any()


def test_lds_sizes_the_gpu_tests_assume(image):
    """Which pipelined launches exist: lds_pipe fits a CU's LDS for every hash case, lds_settle for
    all but hold100_a254 (tl.SETTLE_PIPE_CASES); every wave launch of a hash case is above what a
    kernel may ask for without raise_lds_limits from W = 2 on."""
    for name in tl.HASH_CASES:
        sc, _ = image(name)
        assert sc["lds_wave"] <= tl.LDS_DEVICE_BYTES and sc["lds_pipe"] <= tl.LDS_DEVICE_BYTES, name
        assert (sc["lds_settle"] <= tl.LDS_DEVICE_BYTES) == (name in tl.SETTLE_PIPE_CASES), name
        assert sc["lds_wave"] > 64 * 1024 or sc["W"] == 1, name
    assert image("hold100_a254")[0]["lds_pipe"] > 150 * 1024


@pytest.mark.parametrize("settle", [0, 8])
@pytest.mark.parametrize("name", tl.HASH_CASES)
def test_given_mask_chains_visit_every_attractor_state(image, name, settle):
    """Without perturbation step 0 of the chain puts env e exactly on attractor state e mod S: every
    state, the displaced ones among them, is looked up; both outcomes (target reached, another
    attractor) occur for attractor ids 0 and A - 1, and envs without a target never terminate."""
    sc, vec = image(name)
    spec = tl.limit_spec(name)
    states, ids, _ = tl.attractor_words(spec)
    A = len(spec.attractors)
    for mode in (0, 1):
        chain = tl.given_chain(name, 0.0, settle, mode)
        ref, tg0 = chain["refs"][0], chain["init"][1]
        S = len(ids)
        assert tl.GIVEN_N >= S
        e = np.arange(tl.GIVEN_N)
        assert np.array_equal(ref["final_state"].T, states[e % S])
        assert (ref["flags"] & _lib.FLAG_IN_ATTRACTOR).all()
        term = (ref["flags"] & _lib.FLAG_TERMINATED) != 0
        assert np.array_equal(term, tg0 == ids[e % S])
        for a in (0, A - 1):
            assert (term & (ids[e % S] == a)).any() and (~term & (ids[e % S] == a)).any()
            assert (~term & (tg0 == a)).any()
        assert (tg0 == 255).any() and not term[tg0 == 255].any()
        visited = {tuple(s) for s in ref["final_state"].T.tolist()}
        for k in tl.displaced_states(sc, vec, spec):
            assert tuple(states[k].tolist()) in visited
        # the near-miss steps find nothing, the landings after them do
        for k, want in ((1, 0.0), (3, 0.0), (2, 1.0), (4, 1.0)):
            hit = ((chain["refs"][k]["flags"] & _lib.FLAG_IN_ATTRACTOR) != 0).mean()
            assert abs(hit - want) < 0.01, (k, hit)    # N = 20: a random state is an attractor state 1 in 1,000
    # under perturbation (p = 0.02) about (1 - p)^N of the envs still land, the others a few bits off
    ref = tl.given_chain(name, 0.02, settle, 1)["refs"][0]
    assert ((ref["flags"] & _lib.FLAG_IN_ATTRACTOR) != 0).mean() > 0.5 * 0.98 ** spec.n
    assert ((ref["flags"] & _lib.FLAG_PERTURBED) != 0).any()


def collapse_figures(sc, vec, spec, refs) -> dict:
    """Over the env-steps of a chain: the share in an attractor, the count that landed on a state
    displaced from its home slot, the count that terminated."""
    states, _, _ = tl.attractor_words(spec)
    moved = {tuple(states[k].tolist()) for k in tl.displaced_states(sc, vec, spec)}
    flags = np.stack([r["flags"] for r in refs])
    on_moved = sum(tuple(s) in moved for r in refs for s in r["final_state"].T.tolist())
    return {"in_attractor": float(((flags & _lib.FLAG_IN_ATTRACTOR) != 0).mean()), "displaced": int(on_moved),
            "terminated": int(((flags & _lib.FLAG_TERMINATED) != 0).sum())}


@pytest.mark.parametrize("settle", [0, 8])
@pytest.mark.parametrize("mode", [3, 2])
@pytest.mark.parametrize("name", tl.COLLAPSE_CASES)
def test_collapse_chains_hit_displaced_states(image, name, mode, settle):
    """The random-action chains the GPU tests run on collapse_spec (run_pair's and
    run_rollout_pair's seeds and offsets): at least a quarter of the env-steps end in an attractor,
    at least 32 on a state displaced from its home slot, and some env reaches its target."""
    kw = tl.collapse_kw(settle)
    sc, vec = image(name, **kw)
    assert sc["hash_probes"] == 2 and sc["att_single"] == 1 and sc["gap_exact"] == 2   # the env_fast loops' nets
    spec = tl.limit_spec(name, **kw)
    for run in (tl.COLLAPSE_STEP, tl.COLLAPSE_ROLLOUT):
        got = collapse_figures(sc, vec, spec, tl.random_action_chain(spec, mode, **run))
        print(name, mode, settle, run["seed"], got)
        assert got["in_attractor"] >= 0.25 and got["displaced"] >= 32 and got["terminated"] >= 1, got


GATES_AT_THE_LIMIT = {32: 224, 64: 192, 70: 160, 96: 160, 97: 128, 128: 128}


@pytest.mark.parametrize("n_nodes", tl.GATE_SIZES)
def test_gate_limit_specs_fill_every_plane(image, n_nodes):
    """32 W + n_gates == 256: the last gate's output is plane 255, a node record reads it, and the
    gates stand four levels deep."""
    sc, vec = image(f"gates{n_nodes}_limit")
    assert sc["n_gates"] == GATES_AT_THE_LIMIT[n_nodes] and 32 * sc["W"] + sc["n_gates"] == 256
    assert sc["wave_words"] == 256 and sc["n_glayers"] == 4
    tab = np.asarray(vec["tab"], dtype=np.uint32)
    gates = tab[sc["gate_off"]:sc["gate_off"] + 4 * sc["n_gates"]].reshape(-1, 4)
    assert sorted(gates[:, 2].tolist()) == list(range(32 * sc["W"], 256))          # every output plane once
    inputs = np.asarray(vec["fcompact"], dtype=np.uint32).reshape(-1, 4)[:, 0]
    read = {int((w >> (8 * j)) & 0xFF) for w in inputs.tolist() for j in range(4)}
    assert 255 in read


def test_one_gate_more_is_refused():
    from pbn_rl_amd.spec import EnvSpec
    from .synthetic import gate_limit_network
    with pytest.raises(ValueError, match="130 gates.*more than the kernels address"):
        EnvSpec(gate_limit_network(128, extra=[5]), [])
