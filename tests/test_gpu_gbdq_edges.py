"""The GBDQ kernels at their edges (csrc/pbn_gbdq.hip, csrc/gbdq_front.h; DESIGN.md "GBDQ", "Non-finite
values"; the cases: tests/gbdq_cases.py, checked on the host by test_gbdq_edges_host.py).

pbn_gbdq_front keeps test_gpu_gbdq.py's rule everywhere: with e_ref the maximum distance of the fp32
literal forward to the float64 literal forward, the kernel's maximum distance to float64 is at most
8 e_ref; where a value was planted, over the entries finite in the reference, and the NaN / +inf / -inf
entries are the fp32 literal forward's, entry for entry.  The measured ratios are in DESIGN.md "GBDQ".
pbn_replay_store_split is held to the numpy partition byte for byte."""
import numpy as np
import pytest
import torch

from pbn_rl_amd import _lib
from pbn_rl_amd.replay import DeviceReplay
from tests import gbdq_cases as gc

pytestmark = pytest.mark.gpu

DEV, CANARY = gc.DEV, gc.CANARY


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(name):
        if name not in cache:
            spec = gc.named_spec(name)
            cache[name] = (spec, _lib.NetHandle(spec))
        return cache[name]
    yield get
    for _, h in cache.values():
        h.close()


def hold_to_the_rule(what, got, f32, f64, e_ref):
    """The pattern of the fp32 literal forward, and 8 e_ref over the entries finite in it."""
    for kind, g, r in zip(("NaN", "+inf", "-inf"), gc.pattern(got), gc.pattern(f32)):
        assert torch.equal(g, r), (what, kind, int(g.sum()), int(r.sum()), (g != r).nonzero()[:6].tolist())
    fin = torch.isfinite(f32)
    err = float((got.double() - f64)[fin].abs().max()) if bool(fin.any()) else 0.0
    ratio = err / e_ref if e_ref > 0 else float(err > 0)
    print(f"gbdq front {what}: finite {int(fin.sum())} of {fin.numel()} e_ref {e_ref:.3e} kernel {err:.3e} ratio {ratio:.2f}")
    assert err <= 8 * e_ref, (what, err, e_ref)
    return err


# ------------------------------------------------------------------------------------ node counts
@pytest.mark.parametrize("N", gc.SIZE_N)
def test_front_kernel_at_every_layout_edge(nets, N):
    """32 envs, random gamma / beta: the 8 e_ref rule (at N = 1 e_ref is 0: the exact relu(beta)),
    finite output, two runs with equal bits."""
    spec, net = nets(f"size{N}")
    _, q, edges, words, target, f32, f64, e_ref = gc.sweep_case(f"size{N}")
    image, _ = gc.pack_image(net, spec, q)
    got = gc.run_front(net, spec, image, words, target)
    assert torch.isfinite(got).all()
    hold_to_the_rule(f"size N={N}", got, f32, f64, e_ref)
    again = gc.run_front(net, spec, image, words, target)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))


# ------------------------------------------------------------------------------------ block reuse
@pytest.mark.parametrize("name", ["pbn7", "size65"])
def test_a_block_second_env_equals_the_same_input_alone(nets, name):
    """2048 + 32 envs on 2048 blocks: blocks 0..31 work on a second env, with another input than their
    first (stale u / v rows, act's padding zeroed once).  Every row is bit-equal to the row of the same
    input in a plain 32-env run, itself held to the rule.  size65: above 64 KB of LDS."""
    spec, net = nets(name)
    _, q, edges, words, target, f32, f64, e_ref, env_input = gc.reuse_case(name)
    image, _ = gc.pack_image(net, spec, q)
    plain = gc.run_front(net, spec, image, words, target)
    assert torch.isfinite(plain).all()
    hold_to_the_rule(f"reuse {name} n=32", plain, f32, f64, e_ref)
    n_attr = len(spec.attractors)
    assert {n_attr - 1, n_attr, 255} <= set(target.tolist())
    got = gc.run_front(net, spec, image, np.ascontiguousarray(words[:, env_input]), np.ascontiguousarray(target[env_input]))
    assert got.shape[0] == gc.REUSE_ENVS
    want = plain[torch.from_numpy(env_input)]
    differ = (got.view(torch.int32) != want.view(torch.int32)).any(1).nonzero().reshape(-1)
    assert differ.numel() == 0, (name, differ[:8].tolist())


# ------------------------------------------------------------------------------------ edge lists
@pytest.mark.parametrize("kind", gc.EDGE_KINDS)
@pytest.mark.parametrize("N", [17, 65])
def test_front_kernel_on_edge_lists_no_spec_gives(nets, N, kind):
    """Through the raw ABI: in-degree 0 (rows 0 and N - 1: exactly relu(bn3.bias)), in-degree 2 N, and
    no edge at all (a null d_csr_src; every row relu(beta))."""
    spec, net = nets(f"size{N}")
    _, q, edges, words, target, f32, f64, e_ref = gc.sweep_case(f"size{N}", kind)
    image, _ = gc.pack_image(net, spec, q, edges=edges)
    got = gc.run_front(net, spec, image, words, target)
    assert torch.isfinite(got).all()
    beta = torch.relu(q.bn3.bias.detach())[None, :, None].expand(32, N, N)
    rows = {"isolated": [0, N - 1], "dense": [], "empty": list(range(N))}[kind]
    assert torch.equal(got.reshape(32, N, N)[:, rows], beta[:, rows])
    if kind != "empty":
        hold_to_the_rule(f"edges N={N} {kind}", got, f32, f64, e_ref)


@pytest.mark.parametrize("N", [17, 65])
def test_pack_holds_a_bad_edge_list_to_its_ranges(nets, N):
    """csr_start with -5, E + 7, a decreasing pair and wrong ends; csr_src with -1, N and 2^30: the
    image holds np.clip of them, start[0] = 0 and start[N] = E.  (The front kernel indexes LDS with
    this list; it is not launched on this one.)"""
    spec, net = nets(f"size{N}")
    E = 40
    rng = np.random.default_rng(N)
    start = np.sort(rng.integers(0, E + 1, size=N + 1)).astype(np.int32)
    start[0], start[2], start[5], start[8], start[9], start[N] = 3, -5, E + 7, 30, 10, E - 4
    src = rng.integers(0, N, size=E).astype(np.int32)
    src[1], src[7], src[E - 1] = -1, N, 2 ** 30
    q = gc.make_q(N, 5, 17, bn="random")
    image, nf = gc.pack_image(net, spec, q, csr=(torch.from_numpy(start), torch.from_numpy(src)))     # (asserts its canary)
    off, _, _ = gc.image_offsets(N)
    img = image[:nf].cpu().numpy()
    ints = img.view(np.int32)
    want_start = np.clip(start, 0, E)
    want_start[0], want_start[N] = 0, E
    assert np.array_equal(ints[off["csr_start"]: off["csr_start"] + N + 1], want_start)
    assert np.array_equal(ints[off["csr_src"]: off["csr_src"] + E], np.clip(src, 0, N - 1))
    assert np.array_equal(img[off["csr_src"] + E:], np.full(nf - off["csr_src"] - E, CANARY, np.float32))     # E ints, no more


# ------------------------------------------------------------------------------------ non-finite values
@pytest.mark.parametrize("case", gc.NONFINITE_NAMES)
@pytest.mark.parametrize("name", ["pbn7", "size65"])
def test_front_kernel_keeps_a_planted_nan_or_infinity(nets, name, case):
    """One NaN or infinity in a graph-layer parameter: the kernel's NaN / +inf / -inf entries are the
    fp32 literal forward's, the finite entries within the rule, the canary behind ``out`` intact (in
    run_front).  For the conv_model1 cases the M1 table's NaNs are the unfused numpy statement's."""
    spec, net = nets(name)
    _, q, edges, words, target, f32, f64, e_ref = gc.sweep_case(name, None, case)
    image, nf = gc.pack_image(net, spec, q)
    got = gc.run_front(net, spec, image, words, target)
    hold_to_the_rule(f"nonfinite {name} {case}", got, f32, f64, e_ref)
    if "conv1" in case:
        N = spec.n
        m1 = image[: 16 * N].cpu().numpy().reshape(16, N)
        want = gc.m1_table_numpy(q)
        assert np.isnan(want).any() and np.array_equal(np.isnan(m1), np.isnan(want))
        assert np.array_equal(m1[~np.isnan(want)], want[~np.isnan(want)])


# ------------------------------------------------------------------------------------ the split store
def run_split_store(n, words, K, cap_p, cap_n, kinds, seed, term_mask=gc.TERM, done_mask=gc.TERM | gc.TRUNC,
                    flag_values=gc.SPLIT_FLAGS, term_value=1, other_value=2):
    """pbn_replay_store_split through the raw ABI on two DeviceReplay rings of capacities cap_p and
    cap_n, frame after frame against gc.expected_rings: counts, the four counters and every byte of
    both rings (rows never stored to keep their canary).  Returns the final fill levels."""
    L = _lib.load()
    rng = np.random.default_rng(seed)
    rp, rn = DeviceReplay(cap_p, words, K, DEV), DeviceReplay(cap_n, words, K, DEV)
    for r in (rp, rn):
        for f, v in gc.RING_CANARY.items():
            getattr(r, f).fill_(v)
    rings, pos, size, capd = gc.canary_rings(cap_p, cap_n, words, K)
    ctr = torch.zeros(4, dtype=torch.int64, device=DEV)
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    work = torch.full(((n + 255) // 256 + 16,), -3, dtype=torch.int32, device=DEV)
    ptrs = lambda r: tuple(getattr(r, f).data_ptr() for f in ("state", "next_state", "target", "action", "reward", "done"))  # noqa: E731
    for kind in kinds:
        fields, flags = gc.split_frame(rng, n, words, K, kind, flag_values, term_value, other_value)
        t = [torch.from_numpy(fields[f]).to(DEV) for f in ("state", "next_state", "target", "action", "reward")]
        t.append(torch.from_numpy(flags).to(DEV))
        _lib.check(L.pbn_replay_store_split(n, words, K, *(x.data_ptr() for x in t), term_mask, done_mask,
                                            cap_p, ctr[0:].data_ptr(), ctr[1:].data_ptr(), *ptrs(rp),
                                            cap_n, ctr[2:].data_ptr(), ctr[3:].data_ptr(), *ptrs(rn),
                                            work.data_ptr(), counts.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "pbn_replay_store_split")
        torch.cuda.synchronize()
        cp, cn = gc.expected_rings(rings, pos, size, capd, fields, flags, term_mask, done_mask)
        assert counts.tolist() == [cp, cn], kind
        assert ctr.tolist() == [pos["p"], size["p"], pos["n"], size["n"]], kind
        assert work[(n + 255) // 256:].tolist() == [-3] * 16, kind                  # one count per block, no more
        for key, r in (("p", rp), ("n", rn)):
            for f, want in rings[key].items():
                got = getattr(r, f).cpu().numpy()
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (kind, key, f)
    return size


@pytest.mark.parametrize("words", [2, 4])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_split_store_partly_filled_waves_and_blocks(n, words):
    """capacity_p = n and capacity_n = 3 n + 1, K = 1, two and four state words; eight frames (all,
    none, only env n - 1, only env 0, mixed) so that both rings wrap."""
    size = run_split_store(n, words, 1, n, 3 * n + 1, gc.SPLIT_FRAMES, seed=1000 * words + n)
    assert size["p"] == n and (size["n"] == 3 * n + 1 or n == 1)      # (n = 1 stores at most four negative rows)


def test_split_store_beyond_256_blocks():
    """n = 256 * 257 + 1: 258 blocks, so the prefix over the block counts takes a second stride in the
    last two blocks; about a third of the envs terminated, then all, then none; capacities n, n + 5."""
    n = 256 * 257 + 1
    size = run_split_store(n, 1, 1, n, n + 5, ["third", "all", "none"], seed=5)
    assert size == {"p": n, "n": n + 5}


def test_split_store_with_other_masks():
    """term_mask = 4, done_mask = 0x30, flags from all 256 byte values, n = 257."""
    n = 257
    size = run_split_store(n, 2, 1, n, 3 * n + 1, gc.SPLIT_FRAMES, seed=6, term_mask=4, done_mask=0x30,
                           flag_values=np.arange(256, dtype=np.uint8), term_value=4, other_value=0x30)
    assert size == {"p": n, "n": 3 * n + 1}
