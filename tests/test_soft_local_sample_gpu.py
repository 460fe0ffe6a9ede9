"""GPU: the soft local sampler's kernels (csrc/sdp_soft_local_sample.hip) against tests/soft_local_sample_ref.py, through the two
C entries with raw pointers into guarded buffers.

Tables: every written entry of cdf and rows within parity.TOL of the float64 definition, non-decreasing, nothing written outside
the blocks or the tensors.  End cells: for EVERY sample the restatement's draw on the tables read back from the device, bit for
bit.  Walks: the float64 reference walk started from that same end cell; a walk one of whose uniforms (t >= 2) lies within DELTA
of a float64 threshold it was compared with is excluded, every other walk must match exactly -- list, count, last row -- at most
5 % of a case's walks may be excluded, and some compared walk must come within 10 DELTA of a threshold.

DELTA: measured on MI355X over all cases of soft_local_sample_ref.CASES, the smallest of {1e-6, 3e-6, 1e-5, 3e-5} at which every
non-excluded walk matches is MEASURED_DELTA; the tests use the next value up (DESIGN.md 3.18 has both, and the table errors)."""
import functools

import numpy as np
import pytest
import torch

import sample_ref
import soft_local_ref
import soft_local_sample_ref as ref
from parity import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, DELTA = ref.SEED, ref.DELTA
PAD = 1024                                      # words in front of and behind every output
PATTERN = 0x5A5AC3C3                            # what every output holds before a call (as a float: 1.5e16)
ALL = list(ref.CASES)


def _engine():
    from deepblast_amd._engine import get_engine
    return get_engine()


def _decoder():
    from deepblast_amd.local import SoftLocalDecoder
    return SoftLocalDecoder()


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
    """One forward sweep, one table launch and one sample launch of a case, every output a view into a buffer of PATTERN (visits:
    zeroed inside it) -> dict of numpy arrays; the guards round every output are checked here.  poison: the state buffer holds
    0xFF bytes before the sweep.  Computed once per argument set and shared."""
    family, B, N, M, K0, lens, twist = ref.CASES[name]
    K = K0 if K is None else K
    eng = _engine()
    lib = eng.lib
    th, a = ref.scores(name)
    ln = None if lens is None else _dev(np.asarray(lens, np.int32))
    lp = None if ln is None else ln.data_ptr()
    state_out = None
    if poison:
        nfloats = lib.sdp_soft_local_state_bytes(B, N, M) // 4
        state_out = torch.empty(nfloats * 4, dtype=torch.uint8, device=DEV).fill_(0xFF).view(torch.float32)
    Vt, state = eng.soft_local_forward(_dev(th), _dev(a), ln, state_out=state_out)
    cap = lib.sdp_traceback_capacity(N, M)
    sizes = {"cdf": B * N * M, "rows": B * (N + 1), "states": B * K * cap * 3, "counts": B * K, "visits": B * N * M, "ends": B * K * 2}
    bufs = {k: _guarded(n, torch.float32 if k in ("cdf", "rows") else torch.int32) for k, n in sizes.items()}
    bufs["visits"][1].zero_()
    p = {k: v[1].data_ptr() for k, v in bufs.items()}
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.sdp_soft_local_end_tables_f32(state.data_ptr(), Vt.data_ptr(), p["cdf"], p["rows"], B, N, M, lp, 0, 0, stream) == 0
    assert lib.sdp_soft_local_sample_paths_f32(state.data_ptr(), p["cdf"], p["rows"], p["states"], p["counts"], p["visits"], p["ends"],
                                               B, N, M, K, sample0, seed, lp, 0, 0, stream) == 0
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        _untouched(buf, sizes[k], (name, k))
    shapes = {"cdf": (B, N, M), "rows": (B, N + 1), "states": (B, K, cap, 3), "counts": (B, K), "visits": (B, N, M), "ends": (B, K, 2)}
    out = {k: bufs[k][1].cpu().numpy().reshape(shapes[k]) for k in bufs}
    out["Vt"] = Vt.cpu().numpy()
    for v in out.values():
        v.setflags(write=False)
    return out


def reference_walks(name, got, K=None, sample0=0, seed=SEED):
    """the float64 reference's walks from the end cells the device drew -> soft_local_sample_ref.batch's dict"""
    family, B, N, M, K0, lens, twist = ref.CASES[name]
    return ref.batch([r[4] for r in ref.reference(name)], N, M, K0 if K is None else K, lens, seed=seed, sample0=sample0,
                     ends=got["ends"])


def compare(got, want, N, M, delta):
    """-> (walks excluded, compared walks that differ, the smallest margin among the compared walks, number of walks)"""
    st, cn, on = ref.right_aligned(want, N, M)
    keep = want["margin"] >= delta
    same = (got["counts"] == cn) & ((got["states"] == st) | ~on[..., None]).all(axis=(2, 3))
    compared = want["margin"][keep & np.isfinite(want["margin"])]
    return int((~keep).sum()), int((keep & ~same).sum()), float(compared.min()) if compared.size else np.inf, keep.size


def own_visits(got, N, M):
    """the path cells of the lists the launch wrote, whatever they are"""
    B, K, cap, _ = got["states"].shape
    count = np.zeros((B, N, M), np.int64)
    for b in range(B):
        for k in range(K):
            c = got["counts"][b, k]
            cells = got["states"][b, k, cap - 1 - c:cap - 1]
            np.add.at(count[b], (cells[:, 0], cells[:, 1]), 1)
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
            assert tuple(got["ends"][b, k]) == want, (name, b, k)
            empty += want[0] < 0
    print(f"{name}: {empty} of {B * K} samples are empty")
    if name == "cold-5x7":
        assert 0 < empty < B * K
    if lens is not None:
        assert all((got["ends"][b] == -1).all() for b, (n, m) in enumerate(ref.clamp_lens(lens, B, N, M)) if n == 0)


# ---- the walks ----
@pytest.mark.parametrize("name", ALL)
def test_walks_against_the_float64_reference(name):
    family, B, N, M, K, lens, twist = ref.CASES[name]
    got = launch(name)
    want = reference_walks(name, got)
    excluded, differ, nearest, walks = compare(got, want, N, M, DELTA)
    print(f"{name}: excluded {excluded} of {walks}, differ {differ}, nearest compared margin {nearest:.3g}")
    assert differ == 0
    assert excluded <= 0.05 * walks
    # the formats: the last row, the end cell, the start cell's name, empty samples, rows in front of a list
    cap = N + M + 2
    for b in range(B):
        for k in range(K):
            c, last = int(got["counts"][b, k]), got["states"][b, k, cap - 1]
            lst = got["states"][b, k, cap - 1 - c:cap - 1]
            assert (_words(got["states"][b, k, :cap - 1 - c]) == PATTERN).all()
            if c == 0:
                assert tuple(last) == (0, -1, -1) and tuple(got["ends"][b, k]) == (-1, -1)
                continue
            assert tuple(last) == (c, lst[0, 0], lst[0, 1]) and tuple(lst[-1, :2]) == tuple(got["ends"][b, k]) and lst[0, 2] == 1
            step = np.diff(lst[:, :2], axis=0)
            assert np.array_equal(step, np.asarray([(1, 0), (1, 1), (0, 1)])[lst[1:, 2]])     # x, m, y: how a cell was entered
    # visits are the path cells of the lists the launch wrote; the reference's own where no walk is excluded
    assert np.array_equal(got["visits"], own_visits(got, N, M))
    if excluded == 0:
        assert np.array_equal(got["visits"], want["visits"])
    if twist == "masked":       # no path enters a masked cell through x or y
        _, a = ref.scores(name)
        entered = 0
        for b in range(B):
            for k in range(K):
                c = int(got["counts"][b, k])
                for (i, j, s) in got["states"][b, k, cap - 1 - c + 1:cap - 1] if c else []:
                    entered += s != 1
                    assert s == 1 or np.isfinite(a[b, i, j]), (b, k, i, j, s)
        assert entered > 0 and np.isinf(a).mean() > 0.25


def test_the_comparison_is_not_vacuous():
    """some walk that the test above compares passes within 10 DELTA of a threshold"""
    nearest = np.inf
    for name in ALL:
        family, B, N, M, K, lens, twist = ref.CASES[name]
        got = launch(name)
        nearest = min(nearest, compare(got, reference_walks(name, got), N, M, DELTA)[2])
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
    assert np.array_equal(head["visits"] + tail["visits"], one["visits"])
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
    th, a = ref.scores(name)
    Vt, states, counts, visits, ends = _decoder().sample_paths(_dev(th), _dev(a), K, _dev(np.asarray(lens, np.int32)), seed=SEED,
                                                               return_visits=True, return_ends=True)
    assert np.array_equal(_words(Vt.cpu().numpy()), _words(raw["Vt"]))
    assert np.array_equal(counts.cpu().numpy(), raw["counts"]) and np.array_equal(visits.cpu().numpy(), raw["visits"])
    assert np.array_equal(ends.cpu().numpy(), raw["ends"])
    st, cap = states.cpu().numpy(), N + M + 2
    for b in range(B):
        for k in range(K):
            c = raw["counts"][b, k]
            assert np.array_equal(st[b, k, :c], raw["states"][b, k, cap - 1 - c:cap - 1]) and np.array_equal(st[b, k, -1], raw["states"][b, k, -1])
    _, lists = _decoder().sample_alignments(_dev(th), _dev(a), 4, _dev(np.asarray(lens, np.int32)), seed=SEED)
    assert lists[2][3] == [tuple(int(v) for v in r) for r in st[2, 3, :raw["counts"][2, 3]]] and lists[0] == [[]] * 4
    eng = _engine()
    cdf, rows = eng.soft_local_end_tables(*eng.soft_local_forward(_dev(th), _dev(a), _dev(np.asarray(lens, np.int32)))[::-1], (B, N, M),
                                          _dev(np.asarray(lens, np.int32)))
    inside = _words(raw["cdf"]) != PATTERN
    assert np.array_equal(_words(cdf.cpu().numpy())[inside], _words(raw["cdf"])[inside]) and not cdf.cpu().numpy()[~inside].any()
    assert not rows.cpu().numpy()[_words(raw["rows"]) == PATTERN].any()
    with pytest.raises(ValueError, match="transposed"):
        _decoder().sample_paths(torch.zeros(1, 2, 2100, device=DEV), torch.zeros(1, 2, 2100, device=DEV), 4)


# ---- frequencies ----
def test_frequencies_are_the_posterior():
    """0.04 = 5 * 0.5 / sqrt(4096): five standard deviations of a Bernoulli mean at its widest"""
    B, N, M, K = 2, 8, 9, 4096
    th, a = soft_local_ref.family("drift", 31, B, N, M)
    dec = _decoder()
    E = dec.decode(_dev(th), _dev(a)).cpu().numpy()
    Vt, states, counts, visits, ends = dec.sample_paths(_dev(th), _dev(a), K, seed=31, return_visits=True, return_ends=True)
    freq = visits.cpu().numpy() / K
    print("max |visits / K - E| =", np.abs(freq - E).max())
    assert np.abs(freq - E).max() <= 0.04
    ends, counts = ends.cpu().numpy(), counts.cpu().numpy()
    for b in range(B):
        vt, V, _ = soft_local_ref.forward(th[b:b + 1], a[b:b + 1])
        w = np.exp(V[0, 1:-1, 1:-1] - vt[0])
        hist = np.zeros((N, M))
        full = ends[b][ends[b, :, 0] >= 0]
        np.add.at(hist, (full[:, 0], full[:, 1]), 1)
        share = float((counts[b] == 0).mean())
        print(f"pair {b}: max |end histogram - w| = {np.abs(hist / K - w).max():.3g}, empty {share:.4f} against {np.exp(-vt[0]):.4f}")
        assert np.abs(hist / K - w).max() <= 0.04 and abs(share - np.exp(-vt[0])) <= 0.04
        assert ((counts[b] == 0) == (ends[b, :, 0] < 0)).all()
    assert int(visits.sum()) == int(counts.sum())


# ---- the ABI ----
def test_refused_calls_launch_nothing_and_the_kernels_have_names():
    from deepblast_amd import _engine as E
    name = "floor-1x33"
    family, B, N, M, K, lens, twist = ref.CASES[name]
    eng = _engine()
    lib = eng.lib
    assert {k: lib.sdp_kernel_name(k).decode() for k in (134, 135)} == E.SOFT_LOCAL_SAMPLE_KERNELS
    th, a = ref.scores(name)
    Vt, state = eng.soft_local_forward(_dev(th), _dev(a))
    cap = lib.sdp_traceback_capacity(N, M)
    (cb, cdf), (rb, rows) = _guarded(B * N * M, torch.float32), _guarded(B * (N + 1), torch.float32)
    (sb, states), (nb, counts), (eb, ends) = _guarded(B * K * cap * 3), _guarded(B * K), _guarded(B * K * 2)
    s, v, c, r = state.data_ptr(), Vt.data_ptr(), cdf.data_ptr(), rows.data_ptr()
    st, cn, en = states.data_ptr(), counts.data_ptr(), ends.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    tab, smp = lib.sdp_soft_local_end_tables_f32, lib.sdp_soft_local_sample_paths_f32
    assert tab(None, v, c, r, B, N, M, None, 0, 0, stream) == -1 and tab(s, None, c, r, B, N, M, None, 0, 0, stream) == -1
    assert tab(s, v, None, r, B, N, M, None, 0, 0, stream) == -1 and tab(s, v, c, None, B, N, M, None, 0, 0, stream) == -1
    assert tab(s, v, c, r, B, 0, M, None, 0, 0, stream) == -2 and tab(s, v, c, r, B, N, lib.sdp_max_cols() + 1, None, 0, 0, stream) == -3
    assert tab(s, v, c, r, B, N, M, None, 1, 0, stream) == -4 and tab(s, v, c, r, 9, 1 << 17, 2048, None, 0, 0, stream) == -5
    for bad in ((None, c, r, st, cn, None, en), (s, None, r, st, cn, None, en), (s, c, None, st, cn, None, en),
                (s, c, r, st, None, None, en), (s, c, r, None, None, None, None)):
        assert smp(*bad, B, N, M, K, 0, 1, None, 0, 0, stream) == -1, bad
    assert smp(s, c, r, st, cn, None, en, B, N, M, 0, 0, 1, None, 0, 0, stream) == -2
    assert smp(s, c, r, st, cn, None, en, B, N, M, K, -1, 1, None, 0, 0, stream) == -2
    assert smp(s, c, r, st, cn, None, en, B, N, lib.sdp_max_cols() + 1, K, 0, 1, None, 0, 0, stream) == -3
    assert smp(s, c, r, st, cn, None, en, B, N, M, K, 0, 1, None, 0x40000, 0, stream) == -4
    assert smp(s, c, r, st, cn, None, en, 64, 1024, 1024, 8192, 0, 1, None, 0, 0, stream) == -5
    torch.cuda.synchronize()
    for buf in (cb, rb, sb, nb, eb):
        assert bool((buf == PATTERN).all())
