"""GPU: the sampling kernels (csrc/sdp_sample.hip) against tests/sample_ref.py.  On the row-major states (float64 tensors,
arithmetic="reference") the state tensor is read back and every list, count, last row and visit count must equal the
restatement run on that very tensor.  On the skewed states (packed, exact) the restatement runs on the float64 oracle's weights:
a walk one of whose uniforms lies within DELTA of a threshold it was compared with is excluded, every other walk must match
exactly, at most 5 % of a case's walks may be excluded, and some compared walk must come within 10 DELTA of a threshold.

DELTA: measured on MI355X over all skewed cases below, the smallest of {1e-6, 3e-6, 1e-5, 3e-5} at which every non-excluded walk
matches is MEASURED_DELTA; the test uses the next value up."""
import functools

import numpy as np
import pytest
import torch

import sample_ref
import score_ref
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DELTAS = (1e-6, 3e-6, 1e-5, 3e-5)
MEASURED_DELTA = 1e-6
DELTA = 3e-6


def _decoders():
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder
    return NeedlemanWunschDecoder, SmithWatermanDecoder


def _engine():
    from deepblast_amd._engine import get_engine
    return get_engine()


@functools.lru_cache(maxsize=None)
def _scores(seed, B, N, M):
    """theta ~ U[0, 1), A ~ -U[0, 1)"""
    rng = np.random.RandomState(seed)
    th, a = rng.rand(B, N, M).astype(np.float32), (-rng.rand(B, N, M)).astype(np.float32)
    th.setflags(write=False), a.setflags(write=False)
    return th, a


def _dev(x, dtype=None):
    t = torch.from_numpy(np.array(x, copy=True, order="C"))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _lens(lens):
    return None if lens is None else torch.as_tensor(np.asarray(lens), dtype=torch.int32, device=DEV)


# ---- the row-major states, bit for bit ----
ROW_LENS = [(1, 1), (1, 37), (70, 1)]


@pytest.mark.parametrize("lens", [None, ROW_LENS], ids=["full", "lens"])
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("kind", ["f64", "ref"])
def test_row_major_states_bit_for_bit(kind, variant, lens):
    from deepblast_amd import _engine as E
    B, N, M, K = 3, 70, 37, 16
    th, a = _scores(1, B, N, M)
    eng = _engine()
    dtype = torch.float64 if kind == "f64" else torch.float32
    exact_state = E.REF if kind == "ref" else False
    _, state = eng.forward(_dev(th, dtype), _dev(a, dtype), variant, _lens(lens), exact_state=exact_state)
    Q = state.reshape(-1)[:B * N * M * 3].view(B, N, M, 3).cpu().numpy()
    assert Q.dtype == (np.float64 if kind == "f64" else np.float32)
    states, counts, visits = eng.sample_paths(state, (B, N, M), variant, K, _lens(lens), seed=2024, exact_state=exact_state,
                                              want_visits=True)
    ref = sample_ref.batch([Q[b] for b in range(B)], N, M, K, variant, lens, seed=2024)
    want, cn, on = sample_ref.right_aligned(ref, N, M)
    assert np.array_equal(counts.cpu().numpy(), cn)
    assert np.array_equal(states.cpu().numpy()[on], want[on])
    assert np.array_equal(visits.cpu().numpy(), ref["visits"])


# ---- the skewed states against the float64 oracle's weights ----
@functools.lru_cache(maxsize=None)
def _oracle_walks(seed, B, N, M, K, variant, lens):
    """the restatement on the float64 oracle's Q of every pair's own block -> sample_ref.batch's dict (computed once per case)"""
    th, a = _scores(seed, B, N, M)
    Qs = []
    for b, (n, m) in enumerate(sample_ref.clamp_lens(lens, B, N, M)):
        _, q = oracle.forward(np.ascontiguousarray(th[b:b + 1, :n, :m], np.float64), np.ascontiguousarray(a[b:b + 1, :n, :m], np.float64), variant)
        Qs.append(sample_ref.inner(q))
    return sample_ref.batch(Qs, N, M, K, variant, lens, seed=seed)


def compare(got_states, got_counts, ref, N, M, delta, left=False):
    """-> (walks excluded, walks compared that differ, the smallest margin among the compared walks, number of walks)"""
    want, cn, on = (sample_ref.left_aligned if left else sample_ref.right_aligned)(ref, N, M)
    keep = ref["margin"] >= delta
    same = (got_counts == cn) & ((got_states == want) | ~on[..., None]).all(axis=(2, 3))
    compared = ref["margin"][keep]
    return int((~keep).sum()), int((keep & ~same).sum()), float(compared.min()) if compared.size else np.inf, keep.size


def _held(got_states, got_counts, ref, N, M, left=False):
    excluded, differ, nearest, walks = compare(got_states, got_counts, ref, N, M, DELTA, left)
    print(f"excluded {excluded} of {walks}, differ {differ}, nearest compared margin {nearest:.3g}")
    assert differ == 0
    assert excluded <= 0.05 * walks


def run_engine_case(seed, B, N, M, K, variant, lens, exact_state):
    eng = _engine()
    th, a = _scores(seed, B, N, M)
    ln = None if lens is None else list(lens)
    _, state = eng.forward(_dev(th), _dev(a), variant, _lens(ln), exact_state=exact_state)
    states, counts, visits = eng.sample_paths(state, (B, N, M), variant, K, _lens(ln), seed=seed, exact_state=exact_state,
                                              want_visits=True)
    return states.cpu().numpy(), counts.cpu().numpy(), visits.cpu().numpy()


ENGINE_CASES = {
    "40x50": (21, 4, 40, 50, 64, None),
    "70x37": (22, 3, 70, 37, 64, None),                                    # crosses a strip boundary and the 16- / 32-step blocks
    "thin-routed": (23, 3, 70, 600, 16, ((70, 600), (5, 590), (70, 3))),   # a thin pair routed to float2 inside packed records
    "parts": (24, 2, 600, 64, 8, ((600, 64), (130, 50))),                  # a state written by a forward sweep in parts
}


@pytest.mark.parametrize("exact_state", [False, True], ids=["packed", "exact"])
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_skewed_states_against_the_float64_oracle(case, variant, exact_state):
    seed, B, N, M, K, lens = ENGINE_CASES[case]
    if case == "parts" and not exact_state:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert _engine().lib.sdp_plan_parts(0, B, N, M, 1, 0, cus) > 0      # the state really was written in parts
    got_states, got_counts, visits = run_engine_case(seed, B, N, M, K, variant, lens, exact_state)
    ref = _oracle_walks(seed, B, N, M, K, variant, lens)
    _held(got_states, got_counts, ref, N, M)
    # visits are the path cells of the lists the launch wrote, whatever they are
    cap = N + M + 2
    count = np.zeros((B, N, M), np.int64)
    for b in range(B):
        for k in range(K):
            c, npath = got_counts[b, k], got_states[b, k, cap - 1, 0]
            cells = got_states[b, k, cap - 1 - npath:cap - 1] if npath else np.zeros((0, 3), np.int32)
            assert npath <= c
            np.add.at(count[b], (cells[:, 0], cells[:, 1]), 1)
    assert np.array_equal(visits, count)


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_transposed_route_through_the_decoder(variant):
    seed, B, N, M, K = 25, 2, 5, 2100, 8
    th, a = _scores(seed, B, N, M)
    dec = _decoders()[variant]("softmax")
    Vt, states, counts, visits = dec.sample_paths(_dev(th), _dev(a), K, seed=seed, return_visits=True)
    assert tuple(states.shape) == (B, K, N + M + 2, 3) and tuple(visits.shape) == (B, N, M)
    ref = _oracle_walks(seed, B, N, M, K, variant, None)
    _held(states.cpu().numpy(), counts.cpu().numpy(), ref, N, M, left=True)
    assert int(visits.sum()) == int(states[:, :, -1, 0].sum())


def test_the_comparison_is_not_vacuous():
    """some walk that the tests above compare passes within 10 DELTA of a threshold"""
    nearest = np.inf
    for variant in (0, 1):
        refs = [_oracle_walks(seed, B, N, M, K, variant, lens) for (seed, B, N, M, K, lens) in ENGINE_CASES.values()]
        refs.append(_oracle_walks(25, 2, 5, 2100, 8, variant, None))
        for ref in refs:
            compared = ref["margin"][ref["margin"] >= DELTA]
            nearest = min(nearest, compared.min())
    print("nearest compared margin", nearest)
    assert nearest < 10 * DELTA


# ---- frequencies ----
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_visit_frequencies_are_the_expected_alignment(variant):
    """0.04 = 5 * 0.5 / sqrt(4096): five standard deviations of a Bernoulli mean at its widest"""
    B, N, M, K = 1, 8, 9, 4096
    th, a = _scores(31, B, N, M)
    dec = _decoders()[variant]("softmax")
    t = _dev(th).requires_grad_()
    dec(t, _dev(a)).sum().backward()
    E = t.grad.cpu().numpy()
    _, states, counts, visits = dec.sample_paths(_dev(th), _dev(a), K, seed=31, return_visits=True)
    freq = visits.cpu().numpy() / K
    print("max |visits / K - E| =", np.abs(freq - E).max())
    assert np.abs(freq - E).max() <= 0.04
    st, cn = states.cpu().numpy(), counts.cpu().numpy()
    count = np.zeros((N, M), np.int64)
    for k in range(K):
        cells = st[0, k, cn[0, k] - st[0, k, -1, 0]:cn[0, k]]
        np.add.at(count, (cells[:, 0], cells[:, 1]), 1)
    assert np.array_equal(visits.cpu().numpy()[0], count)


# ---- determinism ----
def test_same_call_same_samples_and_sample0_splits():
    th, a = _scores(41, 3, 33, 47)
    dec = _decoders()[0]("softmax")
    lens = torch.tensor([[33, 47], [20, 47], [33, 9]])
    one = dec.sample_paths(_dev(th), _dev(a), 64, lens, seed=7, return_visits=True)
    two = dec.sample_paths(_dev(th), _dev(a), 64, lens, seed=7, return_visits=True)
    for x, y in zip(one, two):
        assert torch.equal(x, y)
    head = dec.sample_paths(_dev(th), _dev(a), 32, lens, seed=7, return_visits=True)
    tail = dec.sample_paths(_dev(th), _dev(a), 32, lens, seed=7, sample0=32, return_visits=True)
    cn = torch.cat([head[2], tail[2]], dim=1)
    assert torch.equal(cn, one[2])
    st = torch.cat([head[1], tail[1]], dim=1)
    cap = st.shape[2]
    on = (torch.arange(cap, device=DEV)[None, None, :] < cn[..., None]) | (torch.arange(cap, device=DEV)[None, None, :] == cap - 1)
    assert torch.equal(st[on], one[1][on])
    assert torch.equal(head[3] + tail[3], one[3])
    other = dec.sample_paths(_dev(th), _dev(a), 64, lens, seed=8)
    assert not torch.equal(other[1][on], one[1][on])


# ---- forbidden gaps ----
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_forbidden_gaps_leave_the_diagonal(variant):
    th, _ = _scores(51, 2, 6, 6)
    a = np.full((2, 6, 6), -np.inf, np.float32)
    for dec in (_decoders()[variant]("softmax"), _decoders()[variant]("softmax", arithmetic="reference")):
        _, states, counts = dec.sample_paths(_dev(th), _dev(a), 40, seed=5)
        st, cn = states.cpu().numpy(), counts.cpu().numpy()
        for b in range(2):
            for k in range(40):
                npath = st[b, k, -1, 0]
                path = [tuple(r) for r in st[b, k, cn[b, k] - npath:cn[b, k]]]
                assert path == [(i, i, 1) for i in range(variant, 6)]
                if variant == 0:        # (SW: the padding leads from the corner to (1, 1))
                    assert cn[b, k] == 6


# ---- the samples are walks: they feed the scoring kernel unchanged ----
def test_samples_feed_alignment_stats():
    from deepblast_amd import score
    B, N, M, K = 3, 12, 15, 8
    th, a = _scores(61, B, N, M)
    dec = _decoders()[0]("softmax")
    _, states, counts = dec.sample_paths(_dev(th), _dev(a), K, seed=61)
    _, lists = dec.sample_alignments(_dev(th), _dev(a), K, seed=61)
    names = {0: "1", 1: ":", 2: "2"}
    truth = ["".join(names[s] for (_, _, s) in lists[b][0]) for b in range(B) for _ in range(K)]
    cap = states.shape[2]
    stats = score.alignment_stats(truth, (states.reshape(B * K, cap, 3), counts.reshape(B * K)), no_gaps=False, device=DEV).cpu().numpy()
    for r in range(B * K):
        pred = [s for (_, _, s) in lists[r // K][r % K]]
        assert np.array_equal(stats[r], np.array(score_ref.roc(truth[r], pred, no_gaps=False), np.float64)), r
    assert (stats[::K, 3] == 1).all() and len({tuple(s) for s in stats}) > B      # sample 0 against itself; the others spread
