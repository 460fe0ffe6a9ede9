"""GPU: the affine-gap soft semi-global sampler's two kernels (csrc/sdp_affine_semiglobal_sample.hip) against
tests/affine_semiglobal_sample_ref.py, through the C entries with raw pointers into guarded buffers.  Two comparisons.

(A) Bit for bit, no exclusions, every case: the table, every end cell and plane, list, count, last row, `ends`, `visits`, `opens`,
`extends` is the fp32 restatement run on the records READ BACK from the device.
(B) Against the float64 definition, the cases up to 130 x 150: the draw on affine_semiglobal_ref's q and w from the same uniforms; a
walk whose end-draw uniform lies within END_DELTA of one of the two float64 thresholds it fell between, or one of whose other
uniforms (t >= 2) lies within WALK_DELTA of a float64 threshold it was compared with, is excluded; every other walk must match
exactly -- list, count, last row, end cell and plane -- at most 6 % of a case's walks may be excluded, and compared walks exist in
every case that has a path.

The deltas: measured on MI355X over all cases of affine_semiglobal_sample_ref.COMPARED, separately for the end draw (whose
thresholds carry up to n + m sequential fp32 adds) and for the walk, the smallest of {1e-6, 3e-6, 1e-5, 3e-5, 1e-4} at which every
non-excluded walk matches is MEASURED_*_DELTA; the tests use the next value up (DESIGN.md 3.33 has both)."""
import functools

import numpy as np
import pytest
import torch

import affine_semiglobal_ref as sg
import affine_semiglobal_sample_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 1024                                      # words in front of and behind every output
PATTERN = 0x5A5AC3C3                            # what every output holds before a call
COUNTERS = ("visits", "opens", "extends")
OUTPUTS = ("states", "counts") + COUNTERS + ("ends",)
PM = ref.PM
FLAGS = ref.FLAG_SETS


def _engine():
    from deepblast_amd._engine import get_engine
    return get_engine()


def _sampler(free):
    from deepblast_amd.affine import AffineSemiGlobalSampler
    return AffineSemiGlobalSampler(free)


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


def _table(lib, state, B, N, M, lp, bits):
    """one table launch on `state` into a guarded buffer of PATTERN -> the (B, N + M) view (float32 words), still on the device"""
    buf, view = _guarded(B * (N + M))
    assert lib.sdp_affine_semiglobal_end_table_f32(state.data_ptr(), view.data_ptr(), B, N, M, lp, bits, 0, 0,
                                                   torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    _untouched(buf, B * (N + M), "ecdf")
    return view.view(torch.float32).view(B, N + M)


def _sample(lib, state, ecdf, B, N, M, K, lp, bits, sample0=0, seed=ref.SEED, pairs=None):
    """one sample launch on `state` and `ecdf`, every output a view into a buffer of PATTERN (the three counters: zeroed inside it)
    -> dict of numpy arrays (of the pairs `pairs` alone, where given); the guards round every output are checked here"""
    cap = lib.sdp_traceback_capacity(N, M)
    shapes = {"states": (B, K, cap, 3), "counts": (B, K), "visits": (B, N, M), "opens": (B, N, M), "extends": (B, N, M), "ends": (B, K, 3)}
    sizes = {k: int(np.prod(v)) for k, v in shapes.items()}
    bufs = {k: _guarded(n) for k, n in sizes.items()}
    for k in COUNTERS:
        bufs[k][1].zero_()
    assert lib.sdp_affine_semiglobal_sample_paths_f32(state.data_ptr(), ecdf.data_ptr(), *(bufs[k][1].data_ptr() for k in OUTPUTS), B, N, M,
                                                      K, sample0, seed, lp, bits, 0, 0, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        _untouched(buf, sizes[k], k)
    pick = slice(None) if pairs is None else list(pairs)
    return {k: bufs[k][1].view(shapes[k])[pick].cpu().numpy() for k in bufs}


@functools.lru_cache(maxsize=None)
def swept(name, free, poison=False):
    """one forward sweep and one table launch of a case under a flag set -> (Vt, state, ecdf, lens) on the device, shared by the
    sample launches of the case.  poison: the state buffer holds 0xFF bytes before the sweep"""
    family, B, N, M, K0, lens, twist, frees = ref.CASES[name]
    eng = _engine()
    bits = ref.bits(free)
    th, o, x = ref.scores(name)
    ln = None if lens is None else _dev(np.asarray(lens, np.int32))
    state_out = None
    if poison:
        nfloats = eng.lib.sdp_affine_semiglobal_state_bytes(B, N, M) // 4
        state_out = torch.empty(nfloats * 4, dtype=torch.uint8, device=DEV).fill_(0xFF).view(torch.float32)
    Vt, state = eng.affine_semiglobal_forward(_dev(th), _dev(o), _dev(x), bits, ln, state_out=state_out)
    assert state.numel() == B * ref.state_floats(N, M) + B * (N + M)
    ecdf = _table(eng.lib, state, B, N, M, None if ln is None else ln.data_ptr(), bits)
    return Vt, state, ecdf, ln


@functools.lru_cache(maxsize=None)
def launch(name, free, K=None, sample0=0, poison=False, seed=None):
    """the sample launch of a case on swept() -> dict of numpy arrays, the state's words and the table's among them.  Computed once
    per argument set and shared."""
    family, B, N, M, K0, lens, twist, frees = ref.CASES[name]
    K = K0 if K is None else K
    seed = ref.seed_of_case(name, free) if seed is None else seed
    Vt, state, ecdf, ln = swept(name, free, poison)
    out = _sample(_engine().lib, state, ecdf, B, N, M, K, None if ln is None else ln.data_ptr(), ref.bits(free), sample0, seed)
    out["Vt"], out["state"], out["ecdf"] = Vt.cpu().numpy(), state.cpu().numpy(), ecdf.cpu().numpy()
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated(name, free, K=None, sample0=0, seed=None):
    """the fp32 restatement on the records the device wrote -> affine_semiglobal_sample_ref.batch's dict"""
    family, B, N, M, K0, lens, twist, frees = ref.CASES[name]
    seed = ref.seed_of_case(name, free) if seed is None else seed
    got = launch(name, free, K, sample0, False, seed)
    return ref.batch(ref.state_records(got["state"], B, N, M, lens), N, M, K0 if K is None else K, free, lens, seed=seed, sample0=sample0)


def assert_table_bit_for_bit(ecdf, tables, lens, B, N, M, what):
    """the device's table against the restated running sums; the entries that are not written still hold PATTERN"""
    for b, (n, m) in enumerate(ref.clamp_lens(lens, B, N, M)):
        count = n + m - 1 if n >= 1 and m >= 1 else 0
        if count:
            assert tables[b].dtype == np.float32 and np.array_equal(_words(ecdf[b, :count]), _words(tables[b])), (what, b)
            assert (np.diff(ecdf[b, :count]) >= 0).all(), (what, b)
        assert (_words(ecdf[b, count:]) == PATTERN).all(), (what, b)


def assert_bit_for_bit(got, want, N, M, what):
    """every output of a launch against a dict of ref.batch(): no exclusions"""
    st, cn, on = ref.right_aligned(want, N, M)
    assert np.array_equal(got["counts"], cn), what
    assert np.array_equal(got["ends"], want["ends"]), what
    assert np.array_equal(got["states"][on], st[on]), what
    assert (_words(got["states"])[~on] == PATTERN).all(), what          # rows in front of a list are not written
    for key in COUNTERS:
        assert np.array_equal(got[key], want[key]), (what, key)


def compare(got, want, N, M, end_delta, walk_delta):
    """-> (walks excluded, compared walks that differ, number of walks, number of compared non-empty walks)"""
    st, cn, on = ref.right_aligned(want, N, M)
    keep = (want["end_margin"] >= end_delta) & (want["walk_margin"] >= walk_delta)
    same = (got["counts"] == cn) & ((got["states"] == st) | ~on[..., None]).all(axis=(2, 3)) & (got["ends"] == want["ends"]).all(axis=2)
    return int((~keep).sum()), int((keep & ~same).sum()), keep.size, int((keep & np.isfinite(want["margin"])).sum())


# ---- (A): the stated draw on the device's own records, bit for bit ----
@pytest.mark.parametrize("name,free", list(ref.ALL))
def test_every_output_is_the_restatement_on_the_device_records(name, free):
    family, B, N, M, K, lens, twist, frees = ref.CASES[name]
    bits = ref.bits(free)
    got, want = launch(name, free), restated(name, free)
    assert_table_bit_for_bit(got["ecdf"], want["ecdf"], lens, B, N, M, (name, free))
    assert_bit_for_bit(got, want, N, M, (name, free))
    # the formats: a walk starts in plane m at a start cell under the flags and ends at its `ends` cell, an end cell under the
    # flags; every step is the one its plane names; empty samples
    cap = N + M + 2
    empty = 0
    for b, (n, m) in enumerate(ref.clamp_lens(lens, B, N, M)):
        en = sg.ends(n, m, bits) if n >= 1 and m >= 1 else None
        for k in range(K):
            c, last = int(got["counts"][b, k]), got["states"][b, k, cap - 1]
            lst = got["states"][b, k, cap - 1 - c:cap - 1]
            if c == 0:
                assert tuple(last) == (0, -1, -1) and tuple(got["ends"][b, k]) == (-1, -1, -1)
                empty += 1
                continue
            i0, j0, s0 = (int(v) for v in lst[0])
            assert tuple(last) == (c, i0, j0) and s0 == PM and bool(ref.at_start(i0, j0, s0, free))
            assert tuple(lst[-1]) == tuple(got["ends"][b, k]) and en[lst[-1][0] + 1, lst[-1][1] + 1] and c <= n + m - 1
            assert np.array_equal(np.diff(lst[:, :2], axis=0), np.asarray([(1, 0), (1, 1), (0, 1)])[lst[1:, 2]])
            assert not any(bool(ref.at_start(int(i), int(j), int(s), free)) for (i, j, s) in lst[1:])      # it stopped at the first
        if n < 1 or m < 1 or name in ref.NO_PATH:
            assert not got["counts"][b].any() and not any(got[key][b].any() for key in COUNTERS)
        else:
            assert (got["counts"][b] > 0).all()
            assert not got["visits"][b, n:].any() and not got["visits"][b, :, m:].any()          # nothing outside the block
            assert not got["opens"][b, n:].any() and not got["opens"][b, :, m:].any()
            assert not got["extends"][b, n:].any() and not got["extends"][b, :, m:].any()
            assert got["visits"][b, n - 1, :m].sum() >= (K if bits == 2 else 0) and got["visits"][b, :n, m - 1].sum() >= (K if bits == 1 else 0)
    print(f"{name} {free}: {empty} of {B * K} samples are empty")
    assert int(got["visits"].sum()) == int(got["counts"].sum())
    if name in ref.NO_PATH:
        assert np.isneginf(got["Vt"]).all() and empty == B * K
    if twist == "closed-inside":   # every gap forbidden: whole diagonals of 33 cells, no gap anywhere
        assert (got["counts"] == N).all() and not got["opens"].any() and not got["extends"].any()
    if twist == "forbidden":       # no path opens a gap into a cell whose opening is forbidden, or extends one where that is
        _, o, x = ref.scores(name)
        assert np.isinf(o).mean() > 0.25 and np.isinf(x).mean() > 0.25
        assert got["opens"].sum() > 0 and got["extends"].sum() > 0
        assert not got["opens"][np.isinf(o)].any() and not got["extends"][np.isinf(x)].any()


@pytest.mark.parametrize("shape", [(65, 33), (130, 150)])
def test_no_free_end_is_the_global_sampler_bit_for_bit(shape):
    """free_ends = 0: one live candidate, and on a state of affine_semiglobal_forward(free_ends = 0) all six outputs are those of
    sdp_affine_global_sample_paths_f32 on the same state"""
    N, M = shape
    B, K = 3, 64
    eng = _engine()
    lib = eng.lib
    th, o, x = (_dev(a) for a in sg.case_inputs("drift", N, M, B))
    Vt, state = eng.affine_semiglobal_forward(th, o, x, 0)
    ecdf = _table(lib, state, B, N, M, None, 0)
    got = _sample(lib, state, ecdf, B, N, M, K, None, 0)
    cap = lib.sdp_traceback_capacity(N, M)
    shapes = {"states": (B, K, cap, 3), "counts": (B, K), "visits": (B, N, M), "opens": (B, N, M), "extends": (B, N, M), "ends": (B, K, 3)}
    bufs = {k: _guarded(int(np.prod(v))) for k, v in shapes.items()}
    for k in COUNTERS:
        bufs[k][1].zero_()
    assert lib.sdp_affine_global_sample_paths_f32(state.data_ptr(), *(bufs[k][1].data_ptr() for k in OUTPUTS), B, N, M, K, 0, ref.SEED,
                                                  None, 0, 0, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert np.array_equal(_words(got[k]), _words(bufs[k][1].view(shapes[k]).cpu().numpy())), k
    e = ecdf.cpu().numpy()
    assert (e[:, :N - 1] == 0).all() and (e[:, N - 1:N + M - 1] == e[:, N - 1:N]).all() and (e[:, N - 1] > 0.99).all()
    assert (got["ends"][..., :2] == (N - 1, M - 1)).all() and (got["counts"] >= max(N, M)).all()


def test_records_past_four_gib_of_the_state():
    """one launch whose last pair's records lie wholly past 2^32 bytes of the state, at 513 x 2048 under both flags: that pair's
    table and samples against the restatement on that pair's slice of the state.  Pair b's scores are pair 0's rolled by b columns,
    so that no two pairs hold the same records"""
    N, M, K = 513, 2048, 64
    eng = _engine()
    lib = eng.lib
    one = lib.sdp_affine_global_state_bytes(1, N, M)
    B = -(-2 ** 32 // one) + 1
    assert one == ref.state_floats(N, M) * 4 and (B - 1) * one >= 2 ** 32 > (B - 2) * one
    th, o, x = (_dev(a[0]) for a in ref.scores("long-513x2048"))
    th, o, x = (torch.stack([a.roll(b, dims=1) for b in range(B)]) for a in (th, o, x))
    Vt, state = eng.affine_semiglobal_forward(th, o, x, 3)
    assert state.numel() * 4 == B * one + B * (N + M) * 4
    del th, o, x
    ecdf = _table(lib, state, B, N, M, None, 3)
    got = _sample(lib, state, ecdf, B, N, M, K, None, 3, pairs=[B - 1])
    raw = state[(B - 1) * (one // 4):B * (one // 4)].cpu().numpy()
    del state
    want = ref.batch([ref.pair_records(raw, N, M, N, M)], N, M, K, 3, seed=ref.SEED, pair0=B - 1)
    assert np.array_equal(_words(ecdf[B - 1, :N + M - 1].cpu().numpy()), _words(want["ecdf"][0]))
    assert_bit_for_bit(got, want, N, M, "the last pair")
    assert np.isfinite(float(Vt[B - 1])) and (got["counts"] > 0).all() and len({tuple(e) for e in got["ends"][0, :, :2].tolist()}) > 1


# ---- (B): the float64 definition ----
@pytest.mark.parametrize("name,free", list(ref.COMPARED))
def test_walks_against_the_float64_definition(name, free):
    family, B, N, M, K, lens, twist, frees = ref.CASES[name]
    got, want = launch(name, free), ref.reference_walks(name, free)
    end_ladder = {d: compare(got, want, N, M, d, ref.DELTAS[-1])[:2] for d in ref.DELTAS}      # the walk held at its widest
    walk_ladder = {d: compare(got, want, N, M, ref.DELTAS[-1], d)[:2] for d in ref.DELTAS}     # the end draw held at its widest
    excluded, differ, walks, compared = compare(got, want, N, M, ref.END_DELTA, ref.WALK_DELTA)
    print(f"{name} {free}: excluded {excluded} of {walks}, differ {differ}, compared non-empty {compared}; (excluded, differ) by delta, "
          f"end draw {end_ladder}, walk {walk_ladder}")
    assert differ == 0
    assert excluded <= ref.EXCLUDED_CAP * walks
    assert compared > 0 or name in ref.NO_PATH
    if excluded == 0:
        for key in COUNTERS:
            assert np.array_equal(got[key], want[key]), key
    for b, r in enumerate(ref.reference(name, free)):               # the sweep's Vt beside the definition's, -inf where it is
        assert np.isneginf(got["Vt"][b]) == np.isneginf(r[2])
    for b, t64 in enumerate(want["ecdf"]):                          # the table beside the float64 one (a figure, no assertion)
        if t64 is not None and b == 0:
            print(f"    max |ecdf - float64 ecdf| of pair 0: {np.abs(got['ecdf'][0, :t64.size] - t64).max():.3g}")


# ---- determinism ----
@pytest.mark.parametrize("free", FLAGS)
def test_the_same_call_twice_gives_the_same_bits(free):
    name = "drift-130x150"
    swept.cache_clear()                             # a second sweep and a second table as well
    one = launch(name, free)
    swept.cache_clear()
    two = launch.__wrapped__(name, free)
    assert one is not two
    for k in OUTPUTS + ("Vt", "ecdf"):              # (the state itself: its unwritten records are whatever the allocation held)
        assert np.array_equal(_words(one[k]), _words(two[k])), k


@pytest.mark.parametrize("free", FLAGS)
def test_a_partial_wave_and_the_sample0_split(free):
    name = "drift-65x33"
    family, B, N, M, K, lens, twist, frees = ref.CASES[name]
    assert K == 64 and ref.CASES["k70-65x33"][4] == 70
    # 32 + 32 = 64, on ONE table (swept() is shared by the three launches)
    one, head, tail = launch(name, free), launch(name, free, K=32), launch(name, free, K=32, sample0=32)
    cap = N + M + 2
    for k in ("counts", "ends"):
        assert np.array_equal(np.concatenate([head[k], tail[k]], axis=1), one[k]), k
    st = np.concatenate([head["states"], tail["states"]], axis=1)
    on = np.arange(cap)[None, None, :] >= cap - 1 - one["counts"][..., None]
    assert np.array_equal(st[on], one["states"][on])
    for k in COUNTERS:
        assert np.array_equal(head[k] + tail[k], one[k]), k
    other = launch(name, free, seed=ref.SEED + 1)
    assert not np.array_equal(other["ends"], one["ends"])
    # the 70 samples of the partial second wave begin with the 64 of a full one
    part, full = launch("k70-65x33", free), launch("k70-65x33", free, K=64)
    assert np.array_equal(part["counts"][:, :64], full["counts"]) and np.array_equal(part["ends"][:, :64], full["ends"])


@pytest.mark.parametrize("name,free", [("lens-130x150", f) for f in FLAGS] + [("steep-65x33", f) for f in FLAGS] + [("closed-no-path", "y")])
def test_poisoned_state(name, free):
    """neither kernel reads a record the forward sweep did not write: a state buffer of 0xFF bytes changes no bit of any output,
    nor of the table"""
    one, two = launch(name, free), launch(name, free, poison=True)
    for k in OUTPUTS + ("Vt", "ecdf"):
        assert np.array_equal(_words(one[k]), _words(two[k])), k


# ---- the module ----
@pytest.mark.parametrize("free", FLAGS)
def test_the_module_returns_the_same_samples_left_aligned(free):
    name = "lens-130x150"
    family, B, N, M, K, lens, twist, frees = ref.CASES[name]
    raw = launch(name, free)
    th, o, x = (_dev(a) for a in ref.scores(name))
    ln = _dev(np.asarray(lens, np.int32))
    smp = _sampler(free)
    Vt, states, counts, visits, opens, extends, ends = smp.sample_paths(th, o, x, K, ln, seed=ref.seed_of_case(name, free),
                                                                        return_visits=True, return_gaps=True, return_ends=True)
    assert np.array_equal(_words(Vt.cpu().numpy()), _words(raw["Vt"]))
    for key, got in (("counts", counts), ("visits", visits), ("opens", opens), ("extends", extends), ("ends", ends)):
        assert np.array_equal(got.cpu().numpy(), raw[key]), key
    st, cap = states.cpu().numpy(), N + M + 2
    for b in range(B):
        for k in range(K):
            c = raw["counts"][b, k]
            assert np.array_equal(st[b, k, :c], raw["states"][b, k, cap - 1 - c:cap - 1]) and np.array_equal(st[b, k, -1], raw["states"][b, k, -1])
    _, lists = smp.sample_alignments(th, o, x, 4, ln, seed=ref.seed_of_case(name, free))
    assert lists[0][3] == [tuple(int(v) for v in r) for r in st[0, 3, :raw["counts"][0, 3]]] and lists[1] == [[]] * 4
    with pytest.raises(ValueError, match="transposed"):
        z = torch.zeros(1, 2, 2100, device=DEV)
        smp.sample_paths(z, z, z, 4)


# ---- frequencies ----
@pytest.mark.parametrize("free", FLAGS)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_frequencies_are_the_posterior(family, free):
    """0.04 = 5 * 0.5 / sqrt(4096): five standard deviations of a Bernoulli mean at its widest"""
    B, N, M, K = 2, 8, 9, 4096
    th, o, x = sg.inputs(family, 31, B, N, M)
    want = sg.batch(th, o, x, free)
    w = sg.forward(th, o, x, ref.bits(free))[1][:, 1:-1, 1:-1]           # (B, N, M, 3): the float64 end weights
    Vt, states, counts, visits, opens, extends, ends = _sampler(free).sample_paths(_dev(th), _dev(o), _dev(x), K, seed=31, return_visits=True,
                                                                                   return_gaps=True, return_ends=True)
    errs = {key: float(np.abs(got.cpu().numpy() / K - want[key]).max()) for key, got in (("E", visits), ("GO", opens), ("GX", extends))}
    ends = ends.cpu().numpy()
    share = np.zeros((B, N, M, 3))
    for b in range(B):
        np.add.at(share[b], (ends[b, :, 0], ends[b, :, 1], ends[b, :, 2]), 1.0 / K)
    errs["end cell and plane"] = float(np.abs(share - w).max())
    errs["end cell"] = float(np.abs(share.sum(axis=-1) - w.sum(axis=-1)).max())
    print(f"{family} {free}: max |visits / K - E| = {errs['E']:.3g}, |opens / K - GO| = {errs['GO']:.3g}, |extends / K - GX| = "
          f"{errs['GX']:.3g}, |end-cell share - ws| = {errs['end cell']:.3g}, |end (cell, plane) share - w_s| = {errs['end cell and plane']:.3g}")
    assert all(e <= 0.04 for e in errs.values()), errs
    assert int(visits.sum()) == int(counts.sum())


# ---- the mode ----
@pytest.mark.parametrize("free", FLAGS)
def test_a_posterior_that_is_one_path_samples_that_path(free):
    from deepblast_amd.affine import HardAffineSemiGlobalDecoder
    th, o, x, best, share, scale = ref.mode_case(free)
    assert min(share) >= ref.MODE_SHARE          # (asserted on the CPU first: tests/test_affine_semiglobal_sample.py)
    K = 64
    _, paths, lengths = HardAffineSemiGlobalDecoder(free).optimal_paths(_dev(th), _dev(o), _dev(x))
    _, states, counts = _sampler(free).sample_paths(_dev(th), _dev(o), _dev(x), K, seed=ref.SEED)
    paths, lengths, states, counts = (t.cpu().numpy() for t in (paths, lengths, states, counts))
    for b in range(th.shape[0]):
        c = int(lengths[b])
        assert [tuple(int(v) for v in r) for r in paths[b, :c]] == best[b]
        assert (counts[b] == c).all() and (states[b, :, :c] == paths[b, :c]).all()


# ---- the ABI ----
def test_refused_calls_launch_nothing_and_the_kernels_have_names():
    from deepblast_amd import _engine as E
    name = "floor-1x33"
    family, B, N, M, K, lens, twist, frees = ref.CASES[name]
    eng = _engine()
    lib = eng.lib
    assert {k: lib.sdp_kernel_name(k).decode() for k in E.AFFINE_SEMIGLOBAL_SAMPLE_KERNELS} == E.AFFINE_SEMIGLOBAL_SAMPLE_KERNELS == \
        {211: "sdp_affine_semiglobal_end_table_kernel", 212: "sdp_affine_semiglobal_sample_kernel"}
    assert lib.sdp_kernel_name(210) is None and lib.sdp_kernel_name(213) is None
    th, o, x = ref.scores(name)
    Vt, state = eng.affine_semiglobal_forward(_dev(th), _dev(o), _dev(x), 3)
    cap = lib.sdp_traceback_capacity(N, M)
    (sb, states), (nb, counts), (eb, ends), (vb, visits) = _guarded(B * K * cap * 3), _guarded(B * K), _guarded(B * K * 3), _guarded(B * N * M)
    tb, table = _guarded(B * (N + M))
    s, t = state.data_ptr(), table.data_ptr()
    st, cn, en, vs = states.data_ptr(), counts.data_ptr(), ends.data_ptr(), visits.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    tab, smp = lib.sdp_affine_semiglobal_end_table_f32, lib.sdp_affine_semiglobal_sample_paths_f32
    assert tab(None, t, B, N, M, None, 3, 0, 0, stream) == -1 and tab(s, None, B, N, M, None, 3, 0, 0, stream) == -1
    assert tab(s, t, B, 0, M, None, 3, 0, 0, stream) == -2
    assert tab(s, t, B, N, lib.sdp_max_cols() + 1, None, 3, 0, 0, stream) == -3
    for fe in (4, 8, -1):
        assert tab(s, t, B, N, M, None, fe, 0, 0, stream) == -4
    assert tab(s, t, B, N, M, None, 3, 1, 0, stream) == -4
    outs = (st, cn, vs, vs, vs, en)
    for bad in ((None, t, *outs), (s, None, *outs), (s, t, st, None, vs, vs, vs, en), (s, t, None, None, None, None, None, None)):
        assert smp(*bad, B, N, M, K, 0, 1, None, 3, 0, 0, stream) == -1, bad
    assert smp(s, t, *outs, B, N, M, 0, 0, 1, None, 3, 0, 0, stream) == -2
    assert smp(s, t, *outs, B, N, M, K, -1, 1, None, 3, 0, 0, stream) == -2
    assert smp(s, t, *outs, B, 0, M, K, 0, 1, None, 3, 0, 0, stream) == -2
    assert smp(s, t, *outs, B, N, lib.sdp_max_cols() + 1, K, 0, 1, None, 3, 0, 0, stream) == -3
    for fe in (4, 8, -1):
        assert smp(s, t, *outs, B, N, M, K, 0, 1, None, fe, 0, 0, stream) == -4
    for flag in (1, 0x100, 0x10000, 0x40000, 1 << 30):
        assert smp(s, t, *outs, B, N, M, K, 0, 1, None, 3, flag, 0, stream) == -4
    assert smp(s, t, *outs, 64, 1024, 1024, 8192, 0, 1, None, 3, 0, 0, stream) == -5
    torch.cuda.synchronize()
    for buf in (sb, nb, eb, vb, tb):
        assert bool((buf == PATTERN).all())
