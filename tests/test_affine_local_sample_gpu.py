"""GPU: the affine-gap soft local sampler's kernels (csrc/sdp_affine_local_sample.hip) against tests/affine_local_sample_ref.py,
through the two C entries with raw pointers into guarded buffers.

Tables: every written entry of cdf and rows within parity.TOL of the float64 definition, non-decreasing, rows the bit-exact running
sum of the totals cdf holds, nothing written outside the blocks or the tensors.  End cells: for EVERY sample the restatement's draw
on the tables read back from the device, bit for bit.  Planes and walks: the float64 reference's plane draw and walk from that same
end cell; a walk one of whose uniforms (t >= 2) lies within DELTA of a float64 threshold it was compared with is excluded, every
other walk must match exactly -- list, count, last row, end plane -- at most 6 % of a case's walks may be excluded, and in every
case compared walks exist and one of them comes within 10 DELTA of a threshold somewhere in the suite.

DELTA: measured on MI355X over all cases of affine_local_sample_ref.CASES, the smallest of {1e-6, 3e-6, 1e-5, 3e-5} at which every
non-excluded walk matches is MEASURED_DELTA; the tests use the next value up (DESIGN.md 3.25 has both, and the table errors)."""
import functools

import numpy as np
import pytest
import torch

import affine_local_ref
import affine_local_sample_ref as ref
import sample_ref
from parity import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, DELTA = ref.SEED, ref.DELTA
PAD = 1024                                      # words in front of and behind every output
PATTERN = 0x5A5AC3C3                            # what every output holds before a call (as a float: 1.5e16)
ALL = list(ref.CASES)
COUNTERS = ("visits", "opens", "extends")


def _engine():
    from deepblast_amd._engine import get_engine
    return get_engine()


def _decoder():
    from deepblast_amd.affine import AffineLocalDecoder
    return AffineLocalDecoder()


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True, order="C")).to(DEV)


def _guarded(n, dtype=torch.int32):
    """-> (buffer, view): `n` words at PAD of a buffer filled with PATTERN"""
    buf = torch.full((n + 2 * PAD,), PATTERN, dtype=torch.int32, device=DEV)
    return buf, buf[PAD:PAD + n].view(dtype)


def _untouched(buf, n, what):
    assert bool((buf[:PAD] == PATTERN).all()) and bool((buf[PAD + n:] == PATTERN).all()), what


def _words(x):
    return np.ascontiguousarray(x).view(np.uint32)


@functools.lru_cache(maxsize=None)
def launch(name, K=None, sample0=0, poison=False, seed=SEED):
    """One forward sweep, one table launch and one sample launch of a case, every output a view into a buffer of PATTERN (the three
    counters: zeroed inside it) -> dict of numpy arrays; the guards round every output are checked here.  poison: the state
    buffer holds 0xFF bytes before the sweep.  Computed once per argument set and shared."""
    family, B, N, M, K0, lens, twist = ref.CASES[name]
    K = K0 if K is None else K
    eng = _engine()
    lib = eng.lib
    th, o, x = ref.scores(name)
    ln = None if lens is None else _dev(np.asarray(lens, np.int32))
    lp = None if ln is None else ln.data_ptr()
    state_out = None
    if poison:
        nfloats = lib.sdp_affine_local_state_bytes(B, N, M) // 4
        state_out = torch.empty(nfloats * 4, dtype=torch.uint8, device=DEV).fill_(0xFF).view(torch.float32)
    Vt, state = eng.affine_local_forward(_dev(th), _dev(o), _dev(x), ln, state_out=state_out)
    cap = lib.sdp_traceback_capacity(N, M)
    sizes = {"cdf": B * N * M, "rows": B * (N + 1), "states": B * K * cap * 3, "counts": B * K, "visits": B * N * M,
             "opens": B * N * M, "extends": B * N * M, "ends": B * K * 3}
    bufs = {k: _guarded(n, torch.float32 if k in ("cdf", "rows") else torch.int32) for k, n in sizes.items()}
    for k in COUNTERS:
        bufs[k][1].zero_()
    p = {k: v[1].data_ptr() for k, v in bufs.items()}
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.sdp_affine_local_end_tables_f32(state.data_ptr(), Vt.data_ptr(), p["cdf"], p["rows"], B, N, M, lp, 0, 0, stream) == 0
    assert lib.sdp_affine_local_sample_paths_f32(state.data_ptr(), Vt.data_ptr(), p["cdf"], p["rows"], p["states"], p["counts"],
                                                 p["visits"], p["opens"], p["extends"], p["ends"], B, N, M, K, sample0, seed, lp, 0, 0,
                                                 stream) == 0
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        _untouched(buf, sizes[k], (name, k))
    shapes = {"cdf": (B, N, M), "rows": (B, N + 1), "states": (B, K, cap, 3), "counts": (B, K), "visits": (B, N, M),
              "opens": (B, N, M), "extends": (B, N, M), "ends": (B, K, 3)}
    out = {k: bufs[k][1].cpu().numpy().reshape(shapes[k]) for k in bufs}
    out["Vt"] = Vt.cpu().numpy()
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_walks(name, K=None, sample0=0, seed=SEED):
    """the float64 reference's planes and walks from the end cells the device drew -> affine_local_sample_ref.batch's dict"""
    family, B, N, M, K0, lens, twist = ref.CASES[name]
    got = launch(name, K, sample0, False, seed)
    return ref.batch(ref.records(name), N, M, K0 if K is None else K, lens, seed=seed, sample0=sample0, ends=got["ends"])


def compare(got, want, N, M, delta):
    """-> (walks excluded, compared walks that differ, the smallest margin among the compared walks, number of walks, number of
    compared non-empty walks)"""
    st, cn, on = ref.right_aligned(want, N, M)
    keep = want["margin"] >= delta
    same = (got["counts"] == cn) & ((got["states"] == st) | ~on[..., None]).all(axis=(2, 3)) & (got["ends"] == want["ends"]).all(axis=2)
    compared = want["margin"][keep & np.isfinite(want["margin"])]
    return int((~keep).sum()), int((keep & ~same).sum()), float(compared.min()) if compared.size else np.inf, keep.size, compared.size


def own_counters(got, N, M):
    """visits, opens and extends of the lists the launch wrote, whatever they are: a path cell; a cell in plane x or y whose
    predecessor on the list is in another plane / in the same plane"""
    B, K, cap, _ = got["states"].shape
    count = {k: np.zeros((B, N, M), np.int64) for k in COUNTERS}
    for b in range(B):
        for k in range(K):
            c = got["counts"][b, k]
            cells = got["states"][b, k, cap - 1 - c:cap - 1]
            np.add.at(count["visits"][b], (cells[:, 0], cells[:, 1]), 1)
            gap = cells[1:][cells[1:, 2] != 1]
            same = (cells[1:, 2] == cells[:-1, 2])[cells[1:, 2] != 1]
            np.add.at(count["extends"][b], (gap[same, 0], gap[same, 1]), 1)
            np.add.at(count["opens"][b], (gap[~same, 0], gap[~same, 1]), 1)
    return count


# ---- the tables ----
@pytest.mark.parametrize("name", ALL)
def test_tables_against_float64(name):
    family, B, N, M, K, lens, twist = ref.CASES[name]
    got = launch(name)
    worst = {"cdf": 0.0, "rows": 0.0}
    written_c, written_r = np.zeros((B, N, M), bool), np.zeros((B, N + 1), bool)
    for b, (n, m, Vt, V, q, cdf, rows) in enumerate(ref.reference(name)):
        written_c[b, :n, :m], written_r[b, :n + 1] = True, True
        c, r = got["cdf"][b, :n, :m], got["rows"][b, :n + 1]
        if n:
            worst["cdf"] = max(worst["cdf"], float(np.abs(c - cdf).max()))
            assert (np.diff(c, axis=1) >= 0).all() and c.min() >= 0, (name, b)
        worst["rows"] = max(worst["rows"], float(np.abs(r - rows).max()))
        assert (np.diff(r) >= 0).all(), (name, b)
        if n:       # rows is the running sum of the totals cdf holds, formed by sequential fp32 adds
            acc, seq = r[0], [r[0]]
            for i in range(n):
                acc = np.float32(acc + c[i, m - 1])
                seq.append(acc)
            assert np.array_equal(_words(np.asarray(seq, np.float32)), _words(r)), (name, b)
        else:
            assert r[0] == 1.0
    print(f"{name}: max |cdf - float64| = {worst['cdf']:.3g}, max |rows - float64| = {worst['rows']:.3g}")
    assert worst["cdf"] <= TOL and worst["rows"] <= TOL, worst
    # untouched outside the blocks
    assert (_words(got["cdf"])[~written_c] == PATTERN).all() and (_words(got["rows"])[~written_r] == PATTERN).all()
    assert np.isfinite(got["cdf"][written_c]).all() and np.isfinite(got["rows"][written_r]).all()


# ---- the end cells: bit for bit, every sample ----
@pytest.mark.parametrize("name", ALL)
def test_end_cells_are_the_stated_draw_on_the_device_tables(name):
    family, B, N, M, K, lens, twist = ref.CASES[name]
    got = launch(name)
    empty = 0
    for b, (n, m) in enumerate(ref.clamp_lens(lens, B, N, M)):
        for k in range(K):
            us = sample_ref.uniforms(SEED, b, k, 2)
            want = ref.end_draw(got["rows"][b], got["cdf"][b], n, m, us[0], us[1])
            assert tuple(got["ends"][b, k, :2]) == want, (name, b, k)
            assert (got["ends"][b, k, 2] == -1) == (want[0] < 0) and got["ends"][b, k, 2] in (-1, 0, 1, 2)
            empty += want[0] < 0
    print(f"{name}: {empty} of {B * K} samples are empty")
    if name == "cold-5x7":
        assert 0 < empty < B * K
    if lens is not None:
        assert all((got["ends"][b] == -1).all() for b, (n, m) in enumerate(ref.clamp_lens(lens, B, N, M)) if n == 0)


# ---- the planes and the walks ----
@pytest.mark.parametrize("name", ALL)
def test_planes_and_walks_against_the_float64_reference(name):
    family, B, N, M, K, lens, twist = ref.CASES[name]
    got = launch(name)
    want = reference_walks(name)
    excluded, differ, nearest, walks, compared = compare(got, want, N, M, DELTA)
    print(f"{name}: excluded {excluded} of {walks}, differ {differ}, compared non-empty {compared}, nearest compared margin {nearest:.3g}")
    assert differ == 0
    assert excluded <= ref.EXCLUDED_CAP * walks
    assert compared > 0
    # the formats: the last row, the end cell and plane, the start cell's plane, empty samples, rows in front of a list
    cap = N + M + 2
    for b in range(B):
        for k in range(K):
            c, last = int(got["counts"][b, k]), got["states"][b, k, cap - 1]
            lst = got["states"][b, k, cap - 1 - c:cap - 1]
            assert (_words(got["states"][b, k, :cap - 1 - c]) == PATTERN).all()
            if c == 0:
                assert tuple(last) == (0, -1, -1) and tuple(got["ends"][b, k]) == (-1, -1, -1)
                continue
            assert tuple(last) == (c, lst[0, 0], lst[0, 1]) and tuple(lst[-1]) == tuple(got["ends"][b, k]) and lst[0, 2] == 1
            step = np.diff(lst[:, :2], axis=0)
            assert np.array_equal(step, np.asarray([(1, 0), (1, 1), (0, 1)])[lst[1:, 2]])     # x, m, y: how a cell was entered
    # the counters are those of the lists the launch wrote; the reference's own where no walk is excluded
    own = own_counters(got, N, M)
    for key in COUNTERS:
        assert np.array_equal(got[key], own[key]), key
        if excluded == 0:
            assert np.array_equal(got[key], want[key]), key
    if twist == "forbidden":       # no path opens a gap into a cell whose opening is forbidden, or extends one where that is
        _, o, x = ref.scores(name)
        assert np.isinf(o).mean() > 0.25 and np.isinf(x).mean() > 0.25
        assert got["opens"].sum() > 0 and got["extends"].sum() > 0
        assert not got["opens"][np.isinf(o)].any() and not got["extends"][np.isinf(x)].any()


def test_the_comparison_is_not_vacuous():
    """some walk that the test above compares passes within 10 DELTA of a threshold"""
    nearest = np.inf
    for name in ALL:
        family, B, N, M, K, lens, twist = ref.CASES[name]
        nearest = min(nearest, compare(launch(name), reference_walks(name), N, M, DELTA)[2])
    print("nearest compared margin", nearest)
    assert nearest < 10 * DELTA


# ---- determinism ----
def test_the_same_call_twice_gives_the_same_bits():
    name = "drift-130x150"
    one, two = launch(name), launch.__wrapped__(name)
    assert one is not two
    for k in one:
        assert np.array_equal(_words(one[k]), _words(two[k])), k


def test_a_partial_wave_and_the_sample0_split():
    name = "k70-65x33"
    family, B, N, M, K, lens, twist = ref.CASES[name]
    assert K == 70
    one, head, tail = launch(name), launch(name, K=32), launch(name, K=38, sample0=32)
    cap = N + M + 2
    for k in ("counts", "ends"):
        assert np.array_equal(np.concatenate([head[k], tail[k]], axis=1), one[k]), k
    st = np.concatenate([head["states"], tail["states"]], axis=1)
    on = np.arange(cap)[None, None, :] >= cap - 1 - one["counts"][..., None]
    assert np.array_equal(st[on], one["states"][on])
    for k in COUNTERS:
        assert np.array_equal(head[k] + tail[k], one[k]), k
    assert np.array_equal(_words(head["cdf"]), _words(one["cdf"])) and np.array_equal(_words(head["rows"]), _words(one["rows"]))
    other = launch(name, seed=SEED + 1)
    assert not np.array_equal(other["ends"], one["ends"])


@pytest.mark.parametrize("name", ["lens-130x150", "steep-65x33"])
def test_poisoned_state(name):
    """neither kernel reads a record the forward sweep did not write: a state buffer of 0xFF bytes changes no bit"""
    one, two = launch(name), launch(name, poison=True)
    for k in one:
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
    eng = _engine()
    cdf, rows = eng.affine_local_end_tables(*eng.affine_local_forward(th, o, x, ln)[::-1], (B, N, M), ln)
    inside = _words(raw["cdf"]) != PATTERN
    assert np.array_equal(_words(cdf.cpu().numpy())[inside], _words(raw["cdf"])[inside]) and not cdf.cpu().numpy()[~inside].any()
    assert not rows.cpu().numpy()[_words(raw["rows"]) == PATTERN].any()
    with pytest.raises(ValueError, match="transposed"):
        z = torch.zeros(1, 2, 2100, device=DEV)
        _decoder().sample_paths(z, z, z, 4)


# ---- frequencies ----
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_frequencies_are_the_posterior(family):
    """0.04 = 5 * 0.5 / sqrt(4096): five standard deviations of a Bernoulli mean at its widest"""
    B, N, M, K = 2, 8, 9, 4096
    th, o, x = affine_local_ref.inputs(family, 31, B, N, M)
    want = affine_local_ref.batch(th, o, x)
    Vt, states, counts, visits, opens, extends = _decoder().sample_paths(_dev(th), _dev(o), _dev(x), K, seed=31, return_visits=True,
                                                                         return_gaps=True)
    errs = {key: float(np.abs(got.cpu().numpy() / K - want[key]).max()) for key, got in (("E", visits), ("GO", opens), ("GX", extends))}
    empty = (counts.cpu().numpy() == 0).mean(axis=1)
    errs["empty"] = float(np.abs(empty - np.exp(-want["Vt"])).max())
    print(f"{family}: max |visits / K - E| = {errs['E']:.3g}, |opens / K - GO| = {errs['GO']:.3g}, |extends / K - GX| = {errs['GX']:.3g}, "
          f"|empty share - exp(-Vt)| = {errs['empty']:.3g}")
    assert all(e <= 0.04 for e in errs.values()), errs
    assert int(visits.sum()) == int(counts.sum())


# ---- the ABI ----
def test_refused_calls_launch_nothing_and_the_kernels_have_names():
    from deepblast_amd import _engine as E
    name = "floor-1x33"
    family, B, N, M, K, lens, twist = ref.CASES[name]
    eng = _engine()
    lib = eng.lib
    assert {k: lib.sdp_kernel_name(k).decode() for k in (164, 165)} == E.AFFINE_LOCAL_SAMPLE_KERNELS
    th, o, x = ref.scores(name)
    Vt, state = eng.affine_local_forward(_dev(th), _dev(o), _dev(x))
    cap = lib.sdp_traceback_capacity(N, M)
    (cb, cdf), (rb, rows) = _guarded(B * N * M, torch.float32), _guarded(B * (N + 1), torch.float32)
    (sb, states), (nb, counts), (eb, ends), (vb, visits) = _guarded(B * K * cap * 3), _guarded(B * K), _guarded(B * K * 3), _guarded(B * N * M)
    s, v, c, r = state.data_ptr(), Vt.data_ptr(), cdf.data_ptr(), rows.data_ptr()
    st, cn, en, vs = states.data_ptr(), counts.data_ptr(), ends.data_ptr(), visits.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    tab, smp = lib.sdp_affine_local_end_tables_f32, lib.sdp_affine_local_sample_paths_f32
    assert tab(None, v, c, r, B, N, M, None, 0, 0, stream) == -1 and tab(s, None, c, r, B, N, M, None, 0, 0, stream) == -1
    assert tab(s, v, None, r, B, N, M, None, 0, 0, stream) == -1 and tab(s, v, c, None, B, N, M, None, 0, 0, stream) == -1
    assert tab(s, v, c, r, B, 0, M, None, 0, 0, stream) == -2 and tab(s, v, c, r, B, N, lib.sdp_max_cols() + 1, None, 0, 0, stream) == -3
    assert tab(s, v, c, r, B, N, M, None, 1, 0, stream) == -4 and tab(s, v, c, r, 9, 1 << 17, 2048, None, 0, 0, stream) == -5
    outs = (st, cn, vs, vs, vs, en)
    for bad in ((None, v, c, r, *outs), (s, None, c, r, *outs), (s, v, None, r, *outs), (s, v, c, None, *outs),
                (s, v, c, r, st, None, vs, vs, vs, en), (s, v, c, r, None, None, None, None, None, None)):
        assert smp(*bad, B, N, M, K, 0, 1, None, 0, 0, stream) == -1, bad
    assert smp(s, v, c, r, *outs, B, N, M, 0, 0, 1, None, 0, 0, stream) == -2
    assert smp(s, v, c, r, *outs, B, N, M, K, -1, 1, None, 0, 0, stream) == -2
    assert smp(s, v, c, r, *outs, B, N, lib.sdp_max_cols() + 1, K, 0, 1, None, 0, 0, stream) == -3
    assert smp(s, v, c, r, *outs, B, N, M, K, 0, 1, None, 0x40000, 0, stream) == -4
    assert smp(s, v, c, r, *outs, 64, 1024, 1024, 8192, 0, 1, None, 0, 0, stream) == -5
    torch.cuda.synchronize()
    for buf in (cb, rb, sb, nb, eb, vb):
        assert bool((buf == PATTERN).all())
