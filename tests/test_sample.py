"""CPU: sampling alignments from the posterior -- the generator (sdp_sample_uniform against the known answers and against
tests/sample_ref.py), the argument checks of sdp_sample_paths_*, the host wiring (Decoder.sample_paths on a stand-in engine built
from sample_ref), and sample_ref itself against brute force: walking by Q is sampling the distribution whose marginals are E."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import sample_ref
from oracle import oracle
from sample_engine import SampleOracleEngine


@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def _scores(seed, B, N, M, dtype=np.float32):
    rng = np.random.RandomState(seed)
    return rng.rand(B, N, M).astype(dtype), (-rng.rand(B, N, M)).astype(dtype)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _decoders():
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder
    return NeedlemanWunschDecoder, SmithWatermanDecoder


# ---- the generator ----
def test_philox_known_answers():
    for counter, key, want in sample_ref.KNOWN:
        assert tuple(int(w) for w in sample_ref.philox(counter, key)) == want


def test_uniform_is_the_reference_generator(lib):
    """the red test: the symbol does not exist before the sampler does"""
    want = sample_ref.KNOWN[0][2]
    for t in range(4):     # counter (0, 0, 0, 0), key (0, 0)
        assert lib.sdp_sample_uniform(0, 0, 0, t) == (want[t] >> 8) * 2.0 ** -24
    # counter (t >> 2, sample, pair, 0) under key (seed & 0xffffffff, seed >> 32)
    c = sample_ref.philox((5, 0x85a308d3, 0x13198a2e, 0), (0xa4093822, 0x299f31d0))
    for t in range(20, 24):
        got = lib.sdp_sample_uniform((0x299f31d0 << 32) | 0xa4093822, 0x13198a2e, 0x85a308d3 - (1 << 32), t)
        assert got == (int(c[t & 3]) >> 8) * 2.0 ** -24
    for seed, pair, sample in itertools.product((0, 1, 12345, 1 << 32, (1 << 63) + 977, (1 << 64) - 1), (0, 1, 255, 70000), (0, 3, 64, 1 << 20)):
        us = sample_ref.uniforms(seed, pair, sample, 23)
        for t in (0, 1, 2, 3, 4, 5, 7, 10, 13, 22):
            got = lib.sdp_sample_uniform(seed, pair, sample, t)
            assert 0.0 <= got < 1.0 and np.float32(got) == us[t], (seed, pair, sample, t)
            assert got * 2.0 ** 24 == int(got * 2.0 ** 24)


# ---- the C ABI's argument checks need no GPU ----
def test_sample_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    for fn in (lib.sdp_sample_paths_f32, lib.sdp_sample_paths_f64):
        ok = (1, 1, 1, 1, 0, 0, None, 0, 0, None)     # B, N, M, K, sample0, seed, lens, variant, device, stream
        assert fn(None, one, one, one, *ok) == -1
        assert fn(one, None, None, None, *ok) == -1                  # neither states nor visits
        assert fn(one, one, None, None, *ok) == -1                   # states without counts
        assert fn(one, one, None, one, *ok) == -1
        assert fn(one, one, one, one, 1, 1, 1, 0, 0, 0, None, 0, 0, None) == -2        # K = 0
        assert fn(one, one, one, one, 1, 1, 1, -4, 0, 0, None, 0, 0, None) == -2
        assert fn(one, one, one, one, 1, 1, 1, 1, -1, 0, None, 0, 0, None) == -2       # sample0 < 0
        for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
            assert fn(one, one, one, one, *shape, 1, 0, 0, None, 0, 0, None) == -2, shape
        for flag in (0x200, 0x800, 0x10000, 0x20000, 0x1000, 6):      # a stray flag
            assert fn(one, one, one, one, 1, 1, 1, 1, 0, 0, None, flag, 0, None) == -4, hex(flag)
        assert fn(one, one, one, one, 1, 1, 2049, 1, 0, 0, None, 0, 0, None) == -3      # M = sdp_max_cols() + 1
        assert fn(one, one, one, one, 1, 1 << 15, 2048, 1 << 15, 0, 0, None, 0, 0, None) == -5     # states beyond 2^31 elements
        assert fn(one, None, None, one, 1 << 12, 1 << 10, 1 << 10, 1, 0, 0, None, 0, 0, None) == -5  # visits beyond 2^31 elements
    for flag in (0x100, 0x400):    # the state flags belong to the fp32 entry alone
        assert lib.sdp_sample_paths_f64(one, one, one, one, 1, 1, 1, 1, 0, 0, None, flag, 0, None) == -4
    assert [lib.sdp_kernel_name(k) for k in range(119, 124)] == [None, b"sdp_sample_kernel", b"sdp_sample_rows_kernel",
                                                                 b"sdp_sample_rows_f64_kernel", None]
    assert lib.sdp_version() == 106


# ---- sample_ref against brute force ----
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_walking_by_q_samples_the_posterior_whose_marginals_are_e(variant):
    lo = 2 if variant else 1
    for n, m in itertools.product(range(1, 5), range(1, 5)):
        th, a = _scores(50 + 7 * n + m, 1, n, m, np.float64)
        _, E, q, _ = oracle.fwd_bwd(th, a, None, variant)
        Q = sample_ref.inner(q)
        total, marg = 0.0, np.zeros((n, m))
        for path in sample_ref.all_paths(n, m, lo):
            w = sample_ref.path_weight(Q, path)
            total += w
            for (i, j, _) in path:
                marg[i - 1, j - 1] += w
        assert abs(total - 1.0) <= 1e-12, (n, m, total)
        assert np.abs(marg - E[0]).max() <= 1e-12, (n, m)


def test_reference_walks_are_well_formed_and_reproducible():
    th, a = _scores(3, 2, 6, 7, np.float64)
    for variant in (0, 1):
        Qs = [sample_ref.inner(oracle.forward(th[b:b + 1], a[b:b + 1], variant)[1]) for b in range(2)]
        ref = sample_ref.batch(Qs, 6, 7, 5, variant, seed=9)
        again = sample_ref.batch(Qs, 6, 7, 3, variant, seed=9, sample0=2)
        assert ref["lists"][1][2:] == again["lists"][1]
        assert ref["lists"][0][0] != ref["lists"][1][0] or ref["lists"][0][1] != ref["lists"][1][1]
        for lst, npath in zip(ref["lists"][0], ref["npath"][0]):
            assert lst[0][:2] == (0, 0) and lst[-1][:2] == (5, 6) and 6 <= len(lst) <= 12
            for (i0, j0, _), (i1, j1, s1) in list(zip(lst, lst[1:]))[len(lst) - npath:]:
                assert (i1 - i0, j1 - j0) == ((1, 0), (1, 1), (0, 1))[s1]    # a path cell's state names the step into it
        assert ref["visits"].sum() == ref["npath"].sum()


# ---- the host wiring ----
@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = SampleOracleEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_sample_paths_left_aligns_the_lists(eng, variant):
    N, M, K = 6, 8, 5
    th, a = _scores(11, 4, N, M)
    lens = [[6, 8], [1, 1], [1, 8], [4, 3]]
    dec = _decoders()[variant]("softmax")
    Vt, states, counts, visits = dec.sample_paths(_t(th).requires_grad_(), _t(a), K, torch.tensor(lens), seed=77, return_visits=True)
    assert Vt.grad_fn is None and states.dtype == torch.int32 and tuple(states.shape) == (4, K, N + M + 2, 3)
    assert tuple(counts.shape) == (4, K) and tuple(visits.shape) == (4, N, M)
    Qs = [sample_ref.inner(oracle.forward(th[b:b + 1, :n, :m], a[b:b + 1, :n, :m], variant)[1]) for b, (n, m) in enumerate(lens)]
    ref = sample_ref.batch(Qs, N, M, K, variant, lens, seed=77)
    want, cn, on = sample_ref.left_aligned(ref, N, M)
    assert np.array_equal(counts.numpy(), cn)
    assert np.array_equal(states.numpy()[on], want[on])
    assert np.array_equal(visits.numpy(), ref["visits"])
    Vt2, lists = dec.sample_alignments(_t(th), _t(a), K, torch.tensor(lens), seed=77)
    assert np.array_equal(Vt2.numpy(), Vt.numpy()) and lists == ref["lists"]
    for b, (n, m) in enumerate(lens):
        for lst in lists[b]:
            assert (not lst and n == 1 and m == 1 and variant == 1) or lst[0][:2] == (0, 0)
            assert len(lst) <= n + m - 1


def test_sample0_splits_a_batch_of_samples(eng):
    th, a = _scores(12, 2, 5, 6)
    dec = _decoders()[0]("softmax")
    _, whole = dec.sample_alignments(_t(th), _t(a), 6, seed=1 << 40)
    _, head = dec.sample_alignments(_t(th), _t(a), 2, seed=1 << 40)
    _, tail = dec.sample_alignments(_t(th), _t(a), 4, seed=1 << 40, sample0=2)
    assert [h + t for h, t in zip(head, tail)] == whole
    assert dec.sample_alignments(_t(th), _t(a), 6, seed=5)[1] != whole
    assert eng.sample_calls == [((2, 5, 6), False, 6, 0), ((2, 5, 6), False, 2, 0), ((2, 5, 6), False, 4, 2), ((2, 5, 6), False, 6, 0)]


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_transposed_route_swaps_the_columns_back(monkeypatch, variant):
    """swept as (n, m), and -- with the column limit lowered below m -- transposed: the same samples in the original's
    coordinates and names (float64 scores: the two sweeps' weights agree far below the spacing of the uniforms)"""
    from deepblast_amd import _engine
    th, a = _scores(13, 3, 6, 11, np.float64)
    lens = torch.tensor([[6, 11], [4, 9], [2, 11]])
    got = {}
    for cols in (2048, 8):
        e = SampleOracleEngine(cols)
        monkeypatch.setattr(_engine, "_ENGINE", e)
        dec = _decoders()[variant]("softmax")
        Vt, states, counts, visits = dec.sample_paths(_t(th), _t(a), 7, lens, seed=3, return_visits=True)
        _, lists = dec.sample_alignments(_t(th), _t(a), 7, lens, seed=3)
        got[cols] = (lists, counts.numpy(), visits.numpy(), states.numpy()[:, :, -1])
        assert e.sample_calls == [((3, 11, 6), True, 7, 0)] * 2 if cols == 8 else e.sample_calls == [((3, 6, 11), False, 7, 0)] * 2
    for x, y in zip(got[2048], got[8]):
        assert (x == y) if isinstance(x, list) else np.array_equal(x, y)
    assert got[8][2].shape == (3, 6, 11)
    e = SampleOracleEngine(4)     # both sides over the limit: the engine's error
    monkeypatch.setattr(_engine, "_ENGINE", e)
    with pytest.raises(ValueError):
        _decoders()[variant]("softmax").sample_paths(_t(th), _t(a), 2)


def test_sampling_needs_the_soft_operator(eng):
    th, a = _scores(14, 1, 3, 3)
    for dec in (_decoders()[0]("hardmax"), _decoders()[1]("hardmax", local=True)):
        with pytest.raises(ValueError, match="optimal_paths"):
            dec.sample_paths(_t(th), _t(a), 4)
        with pytest.raises(ValueError, match="optimal_paths"):
            dec.sample_alignments(_t(th), _t(a), 4)
    with pytest.raises(ValueError):
        _decoders()[0]("softmax").sample_paths(_t(th), _t(a), 0)


def test_engine_signature_is_declared():
    from deepblast_amd import _engine, _lib
    assert {"sdp_sample_paths_f32", "sdp_sample_paths_f64", "sdp_sample_uniform"} <= set(_lib.SIGNATURES)
    assert _lib.SDP_SAMPLE_TRANSPOSED == 0x40000
    assert callable(_engine.HipEngine.sample_paths)
