"""GPU: the affine-gap soft global sampler's kernel (csrc/sdp_affine_global_sample.hip) against tests/affine_global_sample_ref.py,
through the C entry with raw pointers into guarded buffers.  Two comparisons.

(A) Bit for bit, no exclusions, every case: every end plane, list, count, last row, `ends`, `visits`, `opens`, `extends` is the
fp32 restatement run on the records READ BACK from the device.
(B) Against the float64 definition, the cases up to 130 x 150: the walk of affine_global_ref.forward's q and w from the same
uniforms; a walk one of whose uniforms (t >= 2) lies within DELTA of a float64 threshold it was compared with is excluded, every
other walk must match exactly -- list, count, last row, end plane -- at most 6 % of a case's walks may be excluded, and compared
walks exist in every case.

DELTA: measured on MI355X over all cases of affine_global_sample_ref.COMPARED, the smallest of {1e-6, 3e-6, 1e-5, 3e-5} at which
every non-excluded walk matches is MEASURED_DELTA; the tests use the next value up (DESIGN.md 3.29 has both)."""
import functools

import numpy as np
import pytest
import torch

import affine_global_ref
import affine_global_sample_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, DELTA = ref.SEED, ref.DELTA
PAD = 1024                                      # words in front of and behind every output
PATTERN = 0x5A5AC3C3                            # what every output holds before a call
ALL = list(ref.CASES)
COUNTERS = ("visits", "opens", "extends")
OUTPUTS = ("states", "counts") + COUNTERS + ("ends",)
PM = ref.PM


def _engine():
    from deepblast_amd._engine import get_engine
    return get_engine()


def _decoder():
    from deepblast_amd.affine import AffineGlobalDecoder
    return AffineGlobalDecoder()


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True, order="C")).to(DEV)


def _guarded(n):
    """-> (buffer, view): `n` int32 words at PAD of a buffer filled with PATTERN"""
    buf = torch.full((n + 2 * PAD,), PATTERN, dtype=torch.int32, device=DEV)
    return buf, buf[PAD:PAD + n]


def _untouched(buf, n, what):
    assert bool((buf[:PAD] == PATTERN).all()) and bool((buf[PAD + n:] == PATTERN).all()), what


def _words(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _sample(lib, state, B, N, M, K, lp, sample0=0, seed=SEED, pairs=None):
    """one sample launch on `state`, every output a view into a buffer of PATTERN (the three counters: zeroed inside it) -> dict of
    numpy arrays (of the pairs `pairs` alone, where given); the guards round every output are checked here"""
    cap = lib.sdp_traceback_capacity(N, M)
    shapes = {"states": (B, K, cap, 3), "counts": (B, K), "visits": (B, N, M), "opens": (B, N, M), "extends": (B, N, M), "ends": (B, K, 3)}
    sizes = {k: int(np.prod(v)) for k, v in shapes.items()}
    bufs = {k: _guarded(n) for k, n in sizes.items()}
    for k in COUNTERS:
        bufs[k][1].zero_()
    assert lib.sdp_affine_global_sample_paths_f32(state.data_ptr(), *(bufs[k][1].data_ptr() for k in OUTPUTS), B, N, M, K, sample0, seed,
                                                  lp, 0, 0, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        _untouched(buf, sizes[k], k)
    pick = slice(None) if pairs is None else list(pairs)
    return {k: bufs[k][1].view(shapes[k])[pick].cpu().numpy() for k in bufs}


@functools.lru_cache(maxsize=None)
def launch(name, K=None, sample0=0, poison=False, seed=SEED):
    """One forward sweep and one sample launch of a case -> dict of numpy arrays, the state's words among them.  poison: the state
    buffer holds 0xFF bytes before the sweep.  Computed once per argument set and shared."""
    family, B, N, M, K0, lens, twist = ref.CASES[name]
    K = K0 if K is None else K
    eng = _engine()
    lib = eng.lib
    th, o, x = ref.scores(name)
    ln = None if lens is None else _dev(np.asarray(lens, np.int32))
    state_out = None
    if poison:
        nfloats = lib.sdp_affine_global_state_bytes(B, N, M) // 4
        state_out = torch.empty(nfloats * 4, dtype=torch.uint8, device=DEV).fill_(0xFF).view(torch.float32)
    Vt, state = eng.affine_global_forward(_dev(th), _dev(o), _dev(x), ln, state_out=state_out)
    assert state.numel() == B * ref.state_floats(N, M)
    out = _sample(lib, state, B, N, M, K, None if ln is None else ln.data_ptr(), sample0, seed)
    out["Vt"], out["state"] = Vt.cpu().numpy(), state.cpu().numpy()
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated(name, K=None, sample0=0, seed=SEED):
    """the fp32 restatement on the records the device wrote -> affine_global_sample_ref.batch's dict"""
    family, B, N, M, K0, lens, twist = ref.CASES[name]
    got = launch(name, K, sample0, False, seed)
    return ref.batch(ref.state_records(got["state"], B, N, M, lens), N, M, K0 if K is None else K, lens, seed=seed, sample0=sample0)


def assert_bit_for_bit(got, want, N, M, what):
    """every output of a launch against a dict of ref.batch(): no exclusions"""
    st, cn, on = ref.right_aligned(want, N, M)
    assert np.array_equal(got["counts"], cn), what
    assert np.array_equal(got["ends"], want["ends"]), what
    assert np.array_equal(got["states"][on], st[on]), what
    assert (_words(got["states"])[~on] == PATTERN).all(), what          # rows in front of a list are not written
    for key in COUNTERS:
        assert np.array_equal(got[key], want[key]), (what, key)


def compare(got, want, N, M, delta):
    """-> (walks excluded, compared walks that differ, the smallest margin among the compared walks, number of walks, number of
    compared non-empty walks)"""
    st, cn, on = ref.right_aligned(want, N, M)
    keep = want["margin"] >= delta
    same = (got["counts"] == cn) & ((got["states"] == st) | ~on[..., None]).all(axis=(2, 3)) & (got["ends"] == want["ends"]).all(axis=2)
    compared = want["margin"][keep & np.isfinite(want["margin"])]
    return int((~keep).sum()), int((keep & ~same).sum()), float(compared.min()) if compared.size else np.inf, keep.size, compared.size


# ---- (A): the stated draw on the device's own records, bit for bit ----
@pytest.mark.parametrize("name", ALL)
def test_every_output_is_the_restatement_on_the_device_records(name):
    family, B, N, M, K, lens, twist = ref.CASES[name]
    got = launch(name)
    assert_bit_for_bit(got, restated(name), N, M, name)
    # the formats: the last row, the end cell and plane, the start cell, empty samples, every step the one its plane names
    cap = N + M + 2
    empty = 0
    for b, (n, m) in enumerate(ref.clamp_lens(lens, B, N, M)):
        for k in range(K):
            c, last = int(got["counts"][b, k]), got["states"][b, k, cap - 1]
            lst = got["states"][b, k, cap - 1 - c:cap - 1]
            if c == 0:
                assert tuple(last) == (0, -1, -1) and tuple(got["ends"][b, k]) == (-1, -1, -1)
                empty += 1
                continue
            assert tuple(last) == (c, 0, 0) and tuple(lst[0]) == (0, 0, PM) and tuple(lst[-1]) == tuple(got["ends"][b, k])
            assert tuple(lst[-1][:2]) == (n - 1, m - 1) and max(n, m) <= c <= n + m - 1
            assert np.array_equal(np.diff(lst[:, :2], axis=0), np.asarray([(1, 0), (1, 1), (0, 1)])[lst[1:, 2]])
        if n < 1 or twist in ("closed", "cut") and b in ref.NO_PATH[name]:
            assert not got["counts"][b].any() and not any(got[key][b].any() for key in COUNTERS)
        else:
            assert (got["counts"][b] > 0).all() and (got["visits"][b, 0, 0], got["visits"][b, n - 1, m - 1]) == (K, K)
            assert not got["visits"][b, n:].any() and not got["visits"][b, :, m:].any()
    print(f"{name}: {empty} of {B * K} samples are empty")
    assert int(got["visits"].sum()) == int(got["counts"].sum())
    if twist in ("closed", "cut"):                  # Vt = -inf where there is no path; the diagonal, K times, where it is the one path
        for b in ref.NO_PATH[name]:
            assert np.isneginf(got["Vt"][b])
        for b in ref.DIAGONAL[name]:
            n = ref.clamp_lens(lens, B, N, M)[b][0]
            assert np.array_equal(got["visits"][b, :n, :n], K * np.eye(n, dtype=np.int32)) and (got["ends"][b] == (n - 1, n - 1, PM)).all()
    if twist == "forbidden":       # no path opens a gap into a cell whose opening is forbidden, or extends one where that is
        _, o, x = ref.scores(name)
        assert np.isinf(o).mean() > 0.25 and np.isinf(x).mean() > 0.25
        assert got["opens"].sum() > 0 and got["extends"].sum() > 0
        assert not got["opens"][np.isinf(o)].any() and not got["extends"][np.isinf(x)].any()


def test_records_past_four_gib_of_the_state():
    """one launch whose last pair's records lie wholly past 2^32 bytes of the state, at 513 x 2048: that pair's outputs against the
    restatement on that pair's slice of the state.  Pair b's scores are pair 0's rolled by b columns, so that no two pairs hold
    the same records"""
    N, M, K = 513, 2048, 64
    eng = _engine()
    lib = eng.lib
    one = lib.sdp_affine_global_state_bytes(1, N, M)
    B = -(-2 ** 32 // one) + 1
    assert one == ref.state_floats(N, M) * 4 and (B - 1) * one >= 2 ** 32 > (B - 2) * one
    th, o, x = (_dev(a[0]) for a in ref.scores("long-513x2048"))
    th, o, x = (torch.stack([a.roll(b, dims=1) for b in range(B)]) for a in (th, o, x))
    Vt, state = eng.affine_global_forward(th, o, x)
    assert state.numel() * 4 == B * one
    del th, o, x
    got = _sample(lib, state, B, N, M, K, None, pairs=[B - 1])
    raw = state[(B - 1) * (one // 4):].cpu().numpy()
    del state
    w, q = ref.pair_records(raw, N, M, N, M)
    assert_bit_for_bit(got, ref.batch([(w, q)], N, M, K, seed=SEED, pair0=B - 1), N, M, "the last pair")
    assert np.isfinite(float(Vt[B - 1])) and (got["counts"] >= M).all()


# ---- (B): the float64 definition ----
@pytest.mark.parametrize("name", list(ref.COMPARED))
def test_walks_against_the_float64_definition(name):
    family, B, N, M, K, lens, twist = ref.CASES[name]
    got, want = launch(name), ref.reference_walks(name)
    ladder = {d: compare(got, want, N, M, d)[:2] for d in ref.DELTAS}
    excluded, differ, nearest, walks, compared = compare(got, want, N, M, DELTA)
    print(f"{name}: excluded {excluded} of {walks}, differ {differ}, compared non-empty {compared}, nearest compared margin {nearest:.3g}; "
          f"(excluded, differ) by delta {ladder}")
    assert differ == 0
    assert excluded <= ref.EXCLUDED_CAP * walks
    assert compared > 0
    if excluded == 0:
        for key in COUNTERS:
            assert np.array_equal(got[key], want[key]), key
    for b, r in enumerate(ref.reference(name)):                     # the sweep's Vt beside the definition's, -inf where it is
        assert np.isneginf(got["Vt"][b]) == np.isneginf(r[2])


# ---- determinism ----
def test_the_same_call_twice_gives_the_same_bits():
    name = "drift-130x150"
    one, two = launch(name), launch.__wrapped__(name)
    assert one is not two
    for k in OUTPUTS + ("Vt",):                     # (the state itself: its unwritten records are whatever the allocation held)
        assert np.array_equal(_words(one[k]), _words(two[k])), k


def test_a_partial_wave_and_the_sample0_split():
    name = "drift-65x33"
    family, B, N, M, K, lens, twist = ref.CASES[name]
    assert K == 64 and ref.CASES["k70-65x33"][4] == 70
    one, head, tail = launch(name), launch(name, K=32), launch(name, K=32, sample0=32)
    cap = N + M + 2
    for k in ("counts", "ends"):
        assert np.array_equal(np.concatenate([head[k], tail[k]], axis=1), one[k]), k
    st = np.concatenate([head["states"], tail["states"]], axis=1)
    on = np.arange(cap)[None, None, :] >= cap - 1 - one["counts"][..., None]
    assert np.array_equal(st[on], one["states"][on])
    for k in COUNTERS:
        assert np.array_equal(head[k] + tail[k], one[k]), k
    other = launch(name, seed=SEED + 1)
    assert not np.array_equal(other["counts"], one["counts"])
    # the 70 samples of the partial second wave begin with the 64 of a full one
    part, full = launch("k70-65x33"), launch("k70-65x33", K=64)
    assert np.array_equal(part["counts"][:, :64], full["counts"]) and np.array_equal(part["ends"][:, :64], full["ends"])


@pytest.mark.parametrize("name", ["lens-130x150", "steep-65x33", "cut-40x41"])
def test_poisoned_state(name):
    """the kernel reads no record the forward sweep did not write: a state buffer of 0xFF bytes changes no bit of any output"""
    one, two = launch(name), launch(name, poison=True)
    for k in OUTPUTS + ("Vt",):
        assert np.array_equal(_words(one[k]), _words(two[k])), k


# ---- the module ----
def test_the_module_returns_the_same_samples_left_aligned():
    name = "lens-130x150"
    family, B, N, M, K, lens, twist = ref.CASES[name]
    raw = launch(name)
    th, o, x = (_dev(a) for a in ref.scores(name))
    ln = _dev(np.asarray(lens, np.int32))
    Vt, states, counts, visits, opens, extends, ends = _decoder().sample_paths(th, o, x, K, ln, seed=SEED, return_visits=True,
                                                                               return_gaps=True, return_ends=True)
    assert np.array_equal(_words(Vt.cpu().numpy()), _words(raw["Vt"]))
    for key, got in (("counts", counts), ("visits", visits), ("opens", opens), ("extends", extends), ("ends", ends)):
        assert np.array_equal(got.cpu().numpy(), raw[key]), key
    st, cap = states.cpu().numpy(), N + M + 2
    for b in range(B):
        for k in range(K):
            c = raw["counts"][b, k]
            assert np.array_equal(st[b, k, :c], raw["states"][b, k, cap - 1 - c:cap - 1]) and np.array_equal(st[b, k, -1], raw["states"][b, k, -1])
    _, lists = _decoder().sample_alignments(th, o, x, 4, ln, seed=SEED)
    full = int(np.argmax([n * m for (n, m) in lens]))
    assert lists[full][3] == [tuple(int(v) for v in r) for r in st[full, 3, :raw["counts"][full, 3]]] and lists[0] == [[]] * 4
    with pytest.raises(ValueError, match="transposed"):
        z = torch.zeros(1, 2, 2100, device=DEV)
        _decoder().sample_paths(z, z, z, 4)


# ---- frequencies ----
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_frequencies_are_the_posterior(family):
    """0.04 = 5 * 0.5 / sqrt(4096): five standard deviations of a Bernoulli mean at its widest"""
    B, N, M, K = 2, 8, 9, 4096
    th, o, x = affine_global_ref.inputs(family, 31, B, N, M)
    want = affine_global_ref.batch(th, o, x)
    w = affine_global_ref.forward(th, o, x)[1]
    Vt, states, counts, visits, opens, extends, ends = _decoder().sample_paths(_dev(th), _dev(o), _dev(x), K, seed=31, return_visits=True,
                                                                               return_gaps=True, return_ends=True)
    errs = {key: float(np.abs(got.cpu().numpy() / K - want[key]).max()) for key, got in (("E", visits), ("GO", opens), ("GX", extends))}
    planes = ends.cpu().numpy()[..., 2]
    errs["end plane"] = float(np.abs(np.stack([(planes == s).mean(axis=1) for s in range(3)], axis=1) - w).max())
    print(f"{family}: max |visits / K - E| = {errs['E']:.3g}, |opens / K - GO| = {errs['GO']:.3g}, |extends / K - GX| = {errs['GX']:.3g}, "
          f"|end-plane share - w_s| = {errs['end plane']:.3g}")
    assert all(e <= 0.04 for e in errs.values()), errs
    assert int(visits.sum()) == int(counts.sum())


# ---- the mode ----
def test_a_posterior_that_is_one_path_samples_that_path():
    th, o, x, best, share = ref.mode_case()
    assert min(share) >= ref.MODE_SHARE          # (asserted on the CPU first: tests/test_affine_global_sample.py)
    K = 64
    dec = _decoder()
    _, paths, lengths = dec.optimal_paths(_dev(th), _dev(o), _dev(x))
    _, states, counts = dec.sample_paths(_dev(th), _dev(o), _dev(x), K, seed=SEED)
    paths, lengths, states, counts = (t.cpu().numpy() for t in (paths, lengths, states, counts))
    for b in range(th.shape[0]):
        c = int(lengths[b])
        assert [tuple(int(v) for v in r) for r in paths[b, :c]] == best[b]
        assert (counts[b] == c).all() and (states[b, :, :c] == paths[b, :c]).all()


# ---- the ABI ----
def test_refused_calls_launch_nothing_and_the_kernel_has_a_name():
    from deepblast_amd import _engine as E
    name = "floor-1x33"
    family, B, N, M, K, lens, twist = ref.CASES[name]
    eng = _engine()
    lib = eng.lib
    assert {k: lib.sdp_kernel_name(k).decode() for k in E.AFFINE_GLOBAL_SAMPLE_KERNELS} == E.AFFINE_GLOBAL_SAMPLE_KERNELS == \
        {190: "sdp_affine_global_sample_kernel"}
    assert lib.sdp_kernel_name(189) is None and lib.sdp_kernel_name(191) is None
    th, o, x = ref.scores(name)
    Vt, state = eng.affine_global_forward(_dev(th), _dev(o), _dev(x))
    cap = lib.sdp_traceback_capacity(N, M)
    (sb, states), (nb, counts), (eb, ends), (vb, visits) = _guarded(B * K * cap * 3), _guarded(B * K), _guarded(B * K * 3), _guarded(B * N * M)
    s = state.data_ptr()
    st, cn, en, vs = states.data_ptr(), counts.data_ptr(), ends.data_ptr(), visits.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    smp = lib.sdp_affine_global_sample_paths_f32
    outs = (st, cn, vs, vs, vs, en)
    for bad in ((None, *outs), (s, st, None, vs, vs, vs, en), (s, None, None, None, None, None, None)):
        assert smp(*bad, B, N, M, K, 0, 1, None, 0, 0, stream) == -1, bad
    assert smp(s, *outs, B, N, M, 0, 0, 1, None, 0, 0, stream) == -2
    assert smp(s, *outs, B, N, M, K, -1, 1, None, 0, 0, stream) == -2
    assert smp(s, *outs, B, 0, M, K, 0, 1, None, 0, 0, stream) == -2
    assert smp(s, *outs, B, N, lib.sdp_max_cols() + 1, K, 0, 1, None, 0, 0, stream) == -3
    for flag in (1, 0x100, 0x10000, 0x40000, 1 << 30):
        assert smp(s, *outs, B, N, M, K, 0, 1, None, flag, 0, stream) == -4
    assert smp(s, *outs, 64, 1024, 1024, 8192, 0, 1, None, 0, 0, stream) == -5
    torch.cuda.synchronize()
    for buf in (sb, nb, eb, vb):
        assert bool((buf == PATTERN).all())
