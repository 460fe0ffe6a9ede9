"""CPU: the value-only forward sweep (sdp_forward_value_f32, Decoder.score, deepblast_amd.search) -- its argument checks, its
launch policy (sdp_plan pass 4) beside the unchanged policy of passes 0-3, and the host logic on a stand-in engine."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from fake_engine import OracleEngine
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT_STATE, ET_BROADCAST, REF_ROUNDING, NO_FILL = 0x100, 0x200, 0x400, 0x10000   # include/sdp.h


@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def _plan(lib, pass_, B, N, M, lens=0, exact=0, cus=256):
    kid, chunk, waves, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    assert lib.sdp_plan(pass_, B, N, M, lens, exact, cus, ctypes.byref(kid), ctypes.byref(chunk), ctypes.byref(waves),
                        ctypes.byref(lds)) == 0
    return kid.value, chunk.value, waves.value, lds.value


def test_value_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    f = lib.sdp_forward_value_f32
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        assert f(*args, None, 1, 1, 1, None, 0, 0, None) == -1
        assert b"null" in lib.sdp_last_error_string()
    for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
        assert f(one, one, one, None, *shape, None, 0, 0, None) == -2, shape
    assert f(one, one, one, None, 1, 1, lib.sdp_max_cols() + 1, None, 0, 0, None) == -3
    assert f(one, one, one, None, 1, 1 << 15, 1 << 14, None, 0, 0, None) == -3   # (the column limit is met first)
    assert f(one, one, one, None, 1, 1 << 18, 2048, None, 0, 0, None) == -5      # more than 2^28 cells per pair
    for flag in (EXACT_STATE, REF_ROUNDING, ET_BROADCAST, NO_FILL):
        for base in (0, 1):
            assert f(one, one, one, one, 1, 1, 1, None, base | flag, 0, None) == -4, hex(flag)
    assert f(one, one, one, None, 1, 1, 1, None, 7, 0, None) == -4               # neither SDP_NW nor SDP_SW
    assert f(one, one, one, None, 0, 1, 1, None, 8 << 12, 0, None) == -2         # SDP_WAVES is stripped before validation
    # per-pair lengths need the workspace wherever its size is not zero
    assert lib.sdp_forward_value_ws_bytes(300, 64, 64) >= 300 * 4
    assert lib.sdp_forward_value_ws_bytes(0, 64, 64) == 0 and lib.sdp_forward_value_ws_bytes(3, 64, 4096) == 0
    assert f(one, one, one, None, 3, 64, 64, one, 0, 0, None) == -1
    assert b"workspace" in lib.sdp_last_error_string()


# the shapes of tests/test_abi.py::test_first_order_cases_reach_every_packed_state_build
GRID_BS = [1, 2, 3, 8, 40, 64, 72, 73, 74, 100, 127, 128, 200, 224, 225, 256, 257, 300, 384, 512, 513, 600, 768, 1024]
GRID_NS = [1, 2, 31, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 321, 384, 385, 448, 449, 512, 513, 576, 577, 640,
           768, 769, 1020, 1022, 1023, 1024, 1025, 2048, 4097]
GRID_MS = [1, 7, 31, 32, 33, 64, 65, 96, 100, 512, 513, 960, 1020, 1022, 1023, 1024, 1025, 1500, 1536, 2000, 2048]
VALUE_BUILDS = {41: ("sdp_val_kernel", 32, 4), 42: ("sdp_val_c_kernel", 32, 4), 43: ("sdp_val_g_kernel", 32, 4),
                44: ("sdp_val_lat_kernel", 16, 8), 45: ("sdp_val_lat_c_kernel", 16, 8)}


def value_build(lib, B, N, M, lens, offset=0):
    """(kernel id, waves) a value launch takes on 256 CUs: sdp_plan's answer, for general pitch (SDP_PLAN_GENERAL_PITCH) where M is
    not a multiple of 32 or a plane starts off a 128-byte line"""
    kid, _, waves, _ = _plan(lib, 4 | (0x200 if (M % 32 or offset % 32) else 0), B, N, M, lens)
    return kid, waves


def test_value_plan_names_a_build_and_fits(lib):
    table = {kid: lib.sdp_kernel_name(kid).decode() for kid in range(64) if lib.sdp_kernel_name(kid)}
    for kid, (sym, _, _) in VALUE_BUILDS.items():
        assert table[kid] == sym
    for B in GRID_BS:
        for N in GRID_NS:
            for M in GRID_MS:
                for lens in (0, 1):
                    kid, chunk, waves, lds = _plan(lib, 4, B, N, M, lens)
                    assert kid in VALUE_BUILDS and kid in table, (B, N, M, lens, kid)
                    assert chunk == VALUE_BUILDS[kid][1] and 1 <= waves <= VALUE_BUILDS[kid][2] and waves <= (N + 63) // 64
                    assert lds <= 160 * 1024, (B, N, M, lens, lds)
                    assert (kid in (42, 45)) == bool(lens or N % 64), (B, N, M, lens, kid)   # the cleaning twins, where something foreign can be met
    # what the policy is: the forward sweep's, one workgroup per pair
    assert _plan(lib, 4, 256, 512, 512)[:3] == (41, 32, 4) and _plan(lib, 4, 16, 512, 512)[:3] == (44, 16, 8)
    assert _plan(lib, 4, 512, 512, 512)[:3] == (41, 32, 2) and _plan(lib, 4, 256, 512, 2048)[0] == 44
    assert _plan(lib, 4, 256, 1024, 1024, lens=1)[:3] == (45, 16, 8) and _plan(lib, 4, 600, 512, 512, lens=1)[:3] == (42, 32, 4)
    assert lib.sdp_plan(4 | 0x100, 3, 40, 37, 0, 0, 256, None, None, None, None) != 0   # the fused-seed flag belongs to pass 2
    assert lib.sdp_plan(5, 3, 40, 37, 0, 0, 256, None, None, None, None) != 0
    assert lib.sdp_plan(4, 3, 40, 4096, 0, 0, 256, None, None, None, None) == -3


def test_plan_of_the_four_sweeps_is_the_parent_commits(lib):
    """passes 0-3 (and the fused-seed plan, and sdp_plan_parts) answer what tools/gen_golden_plan.py recorded from the library of
    the commit before the value sweep was added; pass 4 what it recorded from the library of the last commit on which the value
    sweep had a policy function of its own (plan_value), before that was merged into plan()"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_golden_plan", os.path.join(ROOT, "tools", "gen_golden_plan.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for path, passes, count in ((gen.OUT, gen.PASSES, 35200), (gen.OUT_VALUE, gen.PASSES_VALUE, 7040)):
        with open(path) as fh:
            want = json.load(fh)
        assert (want["Bs"], want["Ns"], want["Ms"], want["cus"]) == (gen.BS, gen.NS, gen.MS, gen.CUS)
        got = gen.table(lib, passes)
        assert len(got) == len(want["index"]) == count
        bad = [(i, g, want["rows"][k]) for i, (g, k) in enumerate(zip(got, want["index"])) if g != want["rows"][k]]
        assert not bad, (os.path.basename(path), bad[:5])


def test_value_cases_reach_every_value_build(lib):
    """tests/test_value_gpu.py runs FIRST_ORDER_CASES through forward_value: they must reach every (build, waves) the value policy
    gives over the grid, with the general-pitch twin taken as the launch takes it"""
    from test_parity_gpu import FIRST_ORDER_CASES
    from test_value_gpu import EXTRA_VALUE_CASES
    reachable = set()
    for B in GRID_BS:
        for N in GRID_NS:
            for M in GRID_MS:
                for lens in (0, 1):
                    for offset in (0, 1):
                        reachable.add(value_build(lib, B, N, M, lens, offset))
    covered = {value_build(lib, c[0], c[1], c[2], int(c[4]), c[9]) for c in FIRST_ORDER_CASES + EXTRA_VALUE_CASES}
    assert not reachable - covered, f"value builds no case reaches: {sorted(reachable - covered)}"
    assert not covered - reachable, sorted(covered - reachable)
    assert {(41, 2), (41, 4), (42, 4), (43, 2), (44, 8), (45, 8), (45, 1)} <= reachable


def test_same_bits_cases_run_the_stateful_sweeps_chunk_and_waves(lib):
    """the bit-pattern test of tests/test_value_gpu.py compares where pass 4 and pass 0 run the same chunk length and wave count,
    forcing SDP_WAVES where the policies differ (parts): check here that the forcing it uses makes them equal, and that at most a
    quarter of the cases is set aside"""
    from test_parity_gpu import FIRST_ORDER_CASES
    from test_value_gpu import VALUE_BUILDS_DIFFER, forced_waves_for
    assert len(VALUE_BUILDS_DIFFER) * 4 <= len(FIRST_ORDER_CASES)
    for c in FIRST_ORDER_CASES:
        if c[:3] in VALUE_BUILDS_DIFFER:
            continue
        B, N, M, lens = c[0], c[1], c[2], int(c[4])
        k0, chunk0, w0, _ = _plan(lib, 0, B, N, M, lens)
        k4, chunk4, w4, _ = _plan(lib, 4, B, N, M, lens)
        w = forced_waves_for(lib, c)
        if w == 0:
            assert (chunk0, w0) == (chunk4, w4), c
            assert lib.sdp_plan_parts(0, B, N, M, lens, 0, 256) == 0, c
        else:   # forced: both sweeps then take the K = 32 builds at w waves (w <= 4) -- a forced count keeps a pair on one workgroup
            assert 1 <= w <= 4 and w <= (N + 63) // 64 and M <= 1024, c


# ---- host logic on a stand-in engine ----
class ValueEngine(OracleEngine):
    """OracleEngine + the value entry: per-pair oracle.forward on the [:n, :m] slices; records what it was given"""

    def __init__(self):
        self.calls = []

    def forward_value(self, theta, A, variant, lens=None):
        th, a = self._np(theta), self._np(A)
        B, N, M = th.shape
        self.calls.append((B, N, M, None if lens is None else np.asarray(lens.cpu()).copy(), theta.requires_grad))
        Vt = np.zeros(B, np.float32)
        for b, (n, m) in enumerate(self._slices(B, N, M, lens)):
            Vt[b] = oracle.forward(np.ascontiguousarray(th[b:b + 1, :n, :m]), np.ascontiguousarray(a[b:b + 1, :n, :m]), variant)[0][0]
        return torch.from_numpy(Vt)


@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = ValueEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


def _scores(seed, B, N, M):
    rng = np.random.RandomState(seed)
    return rng.rand(B, N, M).astype(np.float32), (-rng.rand(B, N, M)).astype(np.float32)


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_score_has_no_graph_and_equals_forward(eng, variant):
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder
    dec = (NeedlemanWunschDecoder, SmithWatermanDecoder)[variant]("softmax")
    th, a = _scores(3, 3, 9, 11)
    t, A = torch.from_numpy(th).requires_grad_(), torch.from_numpy(a).requires_grad_()
    lens = torch.tensor([[9, 11], [4, 7], [1, 3]])
    for ln in (None, lens):
        got = dec.score(t, A, ln)
        assert got.grad_fn is None and not got.requires_grad and got.shape == (3,)
        assert not eng.calls[-1][4]                      # the engine saw detached tensors
        want = dec(t, A, ln) if ln is not None else dec(t, A)
        assert want.grad_fn is not None                  # forward() still builds the graph
        assert np.array_equal(got.numpy(), want.detach().numpy())
    with pytest.raises(NotImplementedError):
        NeedlemanWunschDecoder("sparsemax").score(t, A)
    with pytest.raises(ValueError):
        dec.score(t, A[:, :, :5])
    with pytest.raises(TypeError):
        dec.score(t.half(), A.half())


def test_score_transposes_above_the_column_limit(eng):
    from deepblast_amd import NeedlemanWunschDecoder
    dec = NeedlemanWunschDecoder("softmax")
    th, a = _scores(5, 2, 3, 2050)
    lens = torch.tensor([[3, 2050], [2, 1700]])
    got = dec.score(torch.from_numpy(th), torch.from_numpy(a), lens)
    B, N, M, seen, _ = eng.calls[-1]
    assert (B, N, M) == (2, 2050, 3) and seen.tolist() == [[2050, 3], [1700, 2]]
    for b, (n, m) in enumerate(lens.tolist()):
        want = oracle.forward(np.ascontiguousarray(th[b:b + 1, :n, :m]), np.ascontiguousarray(a[b:b + 1, :n, :m]), 0)[0][0]
        assert abs(float(got[b]) - float(want)) <= 1e-4 * max(1.0, abs(float(want))), b   # (the transposed recurrence sums in another order)
    dec.score(torch.from_numpy(th[:, :, :2048].copy()), torch.from_numpy(a[:, :, :2048].copy()))
    assert eng.calls[-1][:3] == (2, 3, 2048)             # at the limit: as it is


def _fake_alignment_scores(zx, zy, gx, gy):
    """the two lines of the reference (alignment.py:134-135) in torch"""
    theta = torch.nn.functional.softplus(torch.einsum("bid,bjd->bij", zx, zy))
    A = torch.nn.functional.logsigmoid(torch.einsum("bid,bjd->bij", gx, gy))
    return theta, A


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_search_scores_chunks_order_and_topk(eng, monkeypatch, variant):
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder, search
    monkeypatch.setattr(search, "alignment_scores", _fake_alignment_scores)
    dec = (NeedlemanWunschDecoder, SmithWatermanDecoder)[variant]("softmax")
    rng = np.random.RandomState(11)
    T, N, Mmax, D, qlen = 7, 6, 9, 4, 5
    zq, gq = (torch.from_numpy(rng.randn(N, D).astype(np.float32)) for _ in range(2))
    dlen = np.array([9, 3, 7, 1, 8, 5, 2])
    zdb, gdb = (torch.from_numpy(rng.randn(T, Mmax, D).astype(np.float32)) for _ in range(2))
    for t in range(T):
        zdb[t, dlen[t]:] = 0
        gdb[t, dlen[t]:] = 0
    want = np.zeros(T, np.float32)
    for t in range(T):   # the reference's loop: one pair at a time, on the pair's own slice
        th, a = _fake_alignment_scores(zq[None, :qlen], zdb[t:t + 1, :dlen[t]], gq[None, :qlen], gdb[t:t + 1, :dlen[t]])
        want[t] = oracle.forward(np.ascontiguousarray(th.numpy()), np.ascontiguousarray(a.numpy()), variant)[0][0]
    want_norm = want / (np.float32(qlen) * dlen.astype(np.float32))
    assert len(set(want_norm.tolist())) == T             # no ties: the order is defined
    for chunk in (3, 100, 1, 7):
        eng.calls.clear()
        res = search.search_scores(dec, zq.clone().requires_grad_(), gq, zdb, gdb, torch.from_numpy(dlen), query_length=qlen,
                                   chunk=chunk, topk=4)
        assert [c[0] for c in eng.calls] == [min(chunk, T - lo) for lo in range(0, T, min(chunk, T))]
        assert all(c[3][:, 0].tolist() == [qlen] * c[0] for c in eng.calls)
        assert np.concatenate([c[3][:, 1] for c in eng.calls]).tolist() == dlen.tolist()
        assert res.score.grad_fn is None and res.normalized.grad_fn is None
        assert np.allclose(res.score.numpy(), want, rtol=0, atol=2e-5)   # (the batched einsum sums like the per-pair one up to rounding)
        assert np.array_equal(res.normalized.numpy(), res.score.numpy() / (np.float32(qlen) * dlen.astype(np.float32)))
        order = np.argsort(-res.normalized.numpy(), kind="stable")[:4]
        assert res.indices.tolist() == order.tolist() == np.argsort(-want_norm, kind="stable")[:4].tolist()
        assert np.array_equal(res.values.numpy(), res.normalized.numpy()[order])
    res = search.search_scores(dec, zq, gq, zdb, gdb, dlen.tolist())
    assert res.indices is None and res.values is None
    assert np.allclose(res.normalized.numpy() * (N * dlen), res.score.numpy(), rtol=1e-6)   # query_length defaults to N
    for bad in (dict(chunk=0), dict(topk=0), dict(topk=8), dict(query_length=7)):
        with pytest.raises(ValueError):
            search.search_scores(dec, zq, gq, zdb, gdb, dlen, **bad)
    with pytest.raises(ValueError):
        search.search_scores(dec, zq, gq, zdb, gdb, dlen[:3])
