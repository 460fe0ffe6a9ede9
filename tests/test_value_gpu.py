"""GPU: the value-only forward sweep (HipEngine.forward_value / Decoder.score / deepblast_amd.search) against the float64 reference,
the fp32 oracle and the stateful forward sweep it is cut from."""
import ctypes

import numpy as np
import pytest

import datagen
import parity
from test_parity_gpu import (FIRST_ORDER_CASES, FIRST_ORDER_PAD, _bits, _first_order_lens, _first_order_sample, _plane_buffer,
                             first_order_case_inputs)

# shapes beside FIRST_ORDER_CASES that the value policy's builds need (tests/test_value.py::test_value_cases_reach_every_value_build):
# none -- the value policy is the forward sweep's with one workgroup per pair, and the imported cases reach each of its builds
EXTRA_VALUE_CASES = []
# cases whose value sweep and stateful sweep NECESSARILY run different chunk lengths, held to float64 instead of to the stateful
# sweep's bits: none.  (The two cases whose stateful forward sweep is a parts launch -- 4 x 600 x 96 and 4 x 700 x 100 with lengths --
# run both sweeps on four forced waves: forced_waves_for.)
VALUE_BUILDS_DIFFER = set()

CASE_IDS = lambda c: "x".join(str(v) for v in c[:3]) + ("-sw" if c[3] else "-nw") + ("-lens" if c[4] else "") + (f"-{c[8]}" if c[8] else "")


def _plan(lib, pass_, B, N, M, lens):
    kid, chunk, waves = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.sdp_plan(pass_, B, N, M, lens, 0, 256, ctypes.byref(kid), ctypes.byref(chunk), ctypes.byref(waves), None) == 0
    return kid.value, chunk.value, waves.value


def forced_waves_for(lib, case):
    """0 where sdp_plan gives the value sweep (pass 4) the chunk length and wave count it gives the forward sweep (pass 0) and the
    forward sweep keeps one workgroup per pair; otherwise the wave count to force on both (SDP_WAVES): the forward sweep's own --
    a forced count keeps a pair on one workgroup, on the K = 32 build of that many waves, and the value sweep follows"""
    B, N, M, lens = case[0], case[1], case[2], int(case[4])
    p0, p4 = _plan(lib, 0, B, N, M, lens), _plan(lib, 4, B, N, M, lens)
    if p0[1:] == p4[1:] and not lib.sdp_plan_parts(0, B, N, M, lens, 0, 256):
        return 0
    return p0[2]


def _oracles(th, a, variant, lens):
    """Vt of the reference in float64 and in fp32 on the same fp32 inputs (per-pair slices under lengths)"""
    out = []
    for cast in (parity.f64, lambda x: x):
        if lens is not None:
            out.append(parity.oracle_lens(cast(th), cast(a), None, None, variant, lens, threads=16)["Vt"])
        else:
            out.append(parity.oracle_all(cast(th), cast(a), None, None, variant, omp=True)["Vt"])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", FIRST_ORDER_CASES + EXTRA_VALUE_CASES, ids=CASE_IDS)
def test_value_tracks_float64_the_oracle_and_the_stateful_sweep(case):
    """Every case of test_first_order_tracks_float64 -- shape, variant, lengths, plane offset, data family -- through forward_value:
    Vt within TOL (relative) of the float64 reference and of the fp32 oracle on the checked pairs, finite everywhere; theta and A
    bit-identical after the call; and Vt equal AS BIT PATTERNS to sdp_forward_f32's wherever both run the same chunk length and
    wave count (forced where the policies differ).  Thin long pairs of a batch with lengths (min(n, m) < 32, max > 512) are set
    aside from the bit comparison: the stateful sweep routes them to its exact-state build, whose 2^theta carries a correction
    the packed arithmetic does not have (sdp_api.hip: exact_for) -- they are held to float64."""
    import torch
    from deepblast_amd._engine import get_engine
    eng = get_engine()
    B, N, M, variant, use_lens, ts, as_, ao, extra, offset = case
    dev = torch.device("cuda", 0)
    seed = 97000 + 10 * FIRST_ORDER_CASES.index(case)
    pairs = _first_order_sample(eng, case, _first_order_lens(case, seed) if use_lens else None)
    theta, A, _, lens, host = first_order_case_inputs(case, pairs)
    tbuf, t = _plane_buffer(theta, offset, seed + 6)
    abuf, a = _plane_buffer(A, offset, seed + 7)
    del theta, A
    t_before, a_before = tbuf.clone(), abuf.clone()
    ln = None if lens is None else torch.from_numpy(lens).to(dev)
    Vt = eng.forward_value(t, a, variant, ln)
    torch.cuda.synchronize()
    assert Vt.shape == (B,) and Vt.dtype == torch.float32 and bool(torch.isfinite(Vt).all())
    assert torch.equal(_bits(tbuf), _bits(t_before)) and torch.equal(_bits(abuf), _bits(a_before)), "the value sweep wrote to its inputs"
    del t_before, a_before
    th_s = np.concatenate([host[b][0] for b in pairs])
    a_s = np.concatenate([host[b][1] for b in pairs])
    ref64, ref32 = _oracles(th_s, a_s, variant, None if lens is None else lens[pairs])
    assert np.isfinite(ref64).all()
    got = Vt.index_select(0, torch.tensor(pairs, device=dev)).cpu().numpy()
    e64, e32 = parity.rel_err(got, ref64), parity.rel_err(got, ref32)
    w = forced_waves_for(eng.lib, case)
    print(f"\nvalue {case}: Vt vs float64 {e64:.2e}, vs the fp32 oracle {e32:.2e} over {len(pairs)} of {B} pairs; forced waves {w}")
    assert e64 <= parity.TOL and e32 <= parity.TOL, (case, e64, e32)
    # the stateful sweep on the same buffers
    try:
        eng.force_waves = {0: w, 4: w} if w else {}
        Vq, Q = eng.forward(t, a, variant, ln)
        Vv = eng.forward_value(t, a, variant, ln) if w else Vt
        torch.cuda.synchronize()
    finally:
        eng.force_waves = {}
    del Q
    if case[:3] in VALUE_BUILDS_DIFFER:
        return
    same = torch.ones(B, dtype=torch.bool, device=dev)
    if ln is not None:
        lo, hi = ln.min(dim=1).values, ln.max(dim=1).values
        same = ~((lo < 32) & (hi > 512))
        thin = [b for b in range(B) if not bool(same[b])]
        for b in thin:   # set aside from the bits: float64 instead
            n, m = lens[b]
            r = parity.oracle_all(parity.f64(t[b:b + 1, :n, :m].cpu().numpy()), parity.f64(a[b:b + 1, :n, :m].cpu().numpy()), None, None, variant, omp=False)
            assert parity.rel_err(Vv[b:b + 1].cpu().numpy(), r["Vt"]) <= parity.TOL, (case, b)
    if eng.lib.sdp_state_bytes(B, N, M) == eng.lib.sdp_state_d_bytes(B, N, M):
        pytest.fail(f"{case}: the stateful sweep takes the exact state for this shape -- not a packed-state case")
    assert torch.equal(_bits(Vv)[same], _bits(Vq)[same]), (case, int((_bits(Vv) != _bits(Vq))[same].sum()), "pairs differ from sdp_forward_f32 in Vt")
    if w:
        assert parity.rel_err(Vv.cpu().numpy(), Vt.cpu().numpy()) <= parity.TOL


@pytest.mark.gpu
def test_value_positive_and_forbidden_gaps_on_long_rows():
    """the 200 x 2048 NW pair with A = 0.5 - U[0,1) and 5 % of the gap scores -inf -- Vt finite and the oracle's, not -inf"""
    import torch
    from deepblast_amd._engine import get_engine
    seed, B, N, M, b = 97340, 74, 200, 2048, 12
    th, a = datagen.theta_A(seed, B, N, M, rows=(b, b + 1))
    a = (a + 0.5).astype(np.float32)
    a[datagen.uniform(seed + 1, (1, N, M), offset=b * N * M) < 0.05] = -np.inf
    ref64, ref32 = _oracles(th, a, 0, None)
    assert np.isfinite(ref64).all() and abs(float(ref64[0]) - 1874.7425) < 1e-3
    Vt = get_engine().forward_value(torch.from_numpy(th).cuda(), torch.from_numpy(a).cuda(), 0).cpu().numpy()
    assert np.isfinite(Vt).all(), Vt
    assert parity.rel_err(Vt, ref64) <= parity.TOL and parity.rel_err(Vt, ref32) <= parity.TOL, (Vt, ref64)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("shape", [(3, 512, 512), (1, 300, 1000), (80, 256, 64)], ids=lambda s: "x".join(map(str, s)))
def test_value_steep_scores(shape, variant):
    """theta x 30: blocks leave the windowed form's range and run per step"""
    import torch
    from deepblast_amd._engine import get_engine
    B, N, M = shape
    th, a = datagen.theta_A(4100 + B, B, N, M)
    th = (th * 30.0).astype(np.float32)
    ref64, ref32 = _oracles(th, a, variant, None)
    Vt = get_engine().forward_value(torch.from_numpy(th).cuda(), torch.from_numpy(a).cuda(), variant).cpu().numpy()
    assert parity.rel_err(Vt, ref64) <= parity.TOL and parity.rel_err(Vt, ref32) <= parity.TOL


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_value_thin_long_pair_alone_batch_of_one_and_inside_a_fat_batch(variant):
    """2 x 2048 alone (B = 1), and the same pair -- with other thin and fat pairs -- inside a padded 40 x 700 x 2048 batch with lengths:
    each pair against float64 and the fp32 oracle, and the in-batch value bit-identical to a call of the pair's own shape"""
    import torch
    from deepblast_amd._engine import get_engine
    eng = get_engine()
    B, N, M = 40, 700, 2048
    seed = 5200 + variant
    lens = datagen.lengths(seed, B, 40, 700)
    lens[:, 1] = np.minimum(lens[:, 1] * 3, M)
    lens[0], lens[3], lens[7], lens[11], lens[39] = (2, 2048), (700, 2048), (1, 1), (31, 600), (650, 5)
    g = torch.Generator(device="cuda").manual_seed(seed)
    theta = torch.rand((B, N, M), generator=g, device="cuda")
    A = -torch.rand((B, N, M), generator=g, device="cuda")
    blocks = []
    for b in range(B):
        n, m = map(int, lens[b])
        th, a = datagen.theta_A(seed * 100 + b, 1, n, m)
        theta[b, :n, :m].copy_(torch.from_numpy(th[0]))
        A[b, :n, :m].copy_(torch.from_numpy(a[0]))
        blocks.append((th, a))
    Vt = eng.forward_value(theta, A, variant, torch.from_numpy(lens).cuda())
    torch.cuda.synchronize()
    got = Vt.cpu().numpy()
    for b in range(B):
        th, a = blocks[b]
        ref64, ref32 = _oracles(th, a, variant, None)
        assert parity.rel_err(got[b:b + 1], ref64) <= parity.TOL and parity.rel_err(got[b:b + 1], ref32) <= parity.TOL, (b, lens[b], got[b], ref64)
        v1 = eng.forward_value(torch.from_numpy(th).cuda(), torch.from_numpy(a).cuda(), variant)   # B = 1, the pair's own shape
        assert torch.equal(_bits(v1), _bits(Vt[b:b + 1])), (b, lens[b].tolist(), float(v1[0]), got[b])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_value_more_pairs_than_cus_with_lengths_runs_through_the_workspace(variant):
    """B > CUs with per-pair lengths: the longest-first launch order goes through the caller's workspace.  Straight through the C
    ABI: Vt inside a poisoned buffer whose neighbours stay as they were, the workspace written only inside
    sdp_forward_value_ws_bytes, theta and A untouched; every pair compared with a call of its own shape, a sample with float64."""
    import torch
    from deepblast_amd import _lib
    from deepblast_amd._engine import get_engine
    eng = get_engine()
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B, N, M = cus + 90, 150, 96
    seed = 6300 + variant
    lens = datagen.lengths(seed, B, 1, 150)
    lens[:, 1] = np.minimum(lens[:, 1], M)
    lens[0] = (N, M)
    th, a = datagen.theta_A(seed, B, N, M)
    theta, A = torch.from_numpy(th).to(dev), torch.from_numpy(a).to(dev)
    t0, a0 = theta.clone(), A.clone()
    ln = torch.from_numpy(lens).to(dev)
    nws = eng.lib.sdp_forward_value_ws_bytes(B, N, M)
    assert B * 4 <= nws <= B * 4 + 256
    PAD = 64
    vbuf = torch.full((B + 2 * PAD,), float("nan"), device=dev)
    wbuf = torch.full((nws // 4 + 2 * PAD,), -12345, dtype=torch.int32, device=dev)
    Vt, ws = vbuf[PAD:PAD + B], wbuf[PAD:PAD + nws // 4]
    rc = eng.lib.sdp_forward_value_f32(theta.data_ptr(), A.data_ptr(), Vt.data_ptr(), ws.data_ptr(), B, N, M, ln.data_ptr(), variant, 0,
                                       torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "sdp_forward_value_f32")
    torch.cuda.synchronize()
    assert bool(torch.isnan(vbuf[:PAD]).all()) and bool(torch.isnan(vbuf[PAD + B:]).all()) and bool(torch.isfinite(Vt).all())
    assert bool((wbuf[:PAD] == -12345).all()) and bool((wbuf[PAD + nws // 4:] == -12345).all())
    assert sorted(ws[:B].tolist()) == list(range(B))            # the order: a permutation of the pairs, longest first
    cells = lens[:, 0].astype(np.int64) * lens[:, 1]
    assert (np.diff(cells[ws[:B].cpu().numpy()]) <= 0).all()
    assert torch.equal(_bits(theta), _bits(t0)) and torch.equal(_bits(A), _bits(a0))
    got = Vt.cpu().numpy()
    for b in range(B):
        n, m = map(int, lens[b])
        v1 = eng.forward_value(theta[b:b + 1, :n, :m].contiguous(), A[b:b + 1, :n, :m].contiguous(), variant)
        assert parity.rel_err(got[b:b + 1], v1.cpu().numpy()) <= parity.TOL, (b, n, m)
    sample = [0, 1, cus - 1, cus, cus + 1, B - 1, int(np.argmin(cells))]
    ref64 = parity.oracle_lens(parity.f64(th[sample]), parity.f64(a[sample]), None, None, variant, lens[sample], threads=8)["Vt"]
    assert parity.rel_err(got[sample], ref64) <= parity.TOL


@pytest.mark.gpu
def test_score_allocates_no_state():
    """Decoder.score on 256 x 512 x 512: peak memory rises by less than 1 % of the state the stateful sweep allocates (377 MB)"""
    import torch
    from deepblast_amd import NeedlemanWunschDecoder
    from deepblast_amd._engine import get_engine
    eng = get_engine()
    B, N, M = 256, 512, 512
    state = eng.lib.sdp_state_bytes(B, N, M)
    assert state > 370e6
    g = torch.Generator(device="cuda").manual_seed(1)
    theta = torch.rand((B, N, M), generator=g, device="cuda").requires_grad_()
    A = (-torch.rand((B, N, M), generator=g, device="cuda")).requires_grad_()
    dec = NeedlemanWunschDecoder("softmax")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    v = dec.score(theta, A)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert v.grad_fn is None and not v.requires_grad
    assert rise < 0.01 * state, (rise, state)
    with torch.no_grad():
        want = dec(theta, A)
    assert torch.cuda.max_memory_allocated() - before >= state   # (the stateful route does allocate it: the cap tells the two apart)
    assert torch.equal(_bits(v), _bits(want))                     # same build geometry (K = 32, 4 waves): same bits
    rv = NeedlemanWunschDecoder("softmax", arithmetic="reference").score(theta[:3, :70, :90], A[:3, :70, :90])
    assert rv.grad_fn is None
    ref = parity.oracle_all(theta[:3, :70, :90].detach().cpu().numpy().copy(), A[:3, :70, :90].detach().cpu().numpy().copy(), None, None, 0)["Vt"]
    assert parity.rel_err(rv.cpu().numpy(), ref) <= parity.TOL
    v64 = dec.score(theta[:3, :70, :90].double(), A[:3, :70, :90].double())
    assert v64.dtype == torch.float64 and parity.rel_err(v64.cpu().numpy(), ref) <= parity.TOL


def _search_problem(seed, T, N, D, lo, hi, dev):
    """query of N residues and T targets of lo..hi residues, embeddings ~ N(0, 1) / sqrt(D) scaled so that scores are O(1); the
    database holds no two targets of one length, ten short ones (lo, lo + 2, ... residues) and the rest from 120 residues on: the
    normalised score Vt / (qlen * dlen) falls with the target's length, so the ten best are the short ones, and the 11th lies far
    (many times the bound) below the 10th"""
    import torch
    rng = np.random.RandomState(seed)
    dlen = np.concatenate([np.arange(lo, lo + 20, 2), [hi], rng.permutation(np.arange(120, hi))[:T - 11]])
    dlen = rng.permutation(dlen).astype(np.int32)
    Mmax = int(dlen.max())
    g = torch.Generator(device=dev).manual_seed(seed)
    s = 2.0 / np.sqrt(D)
    zq, gq = (torch.randn((N, D), generator=g, device=dev) * s for _ in range(2))
    zdb, gdb = (torch.randn((T, Mmax, D), generator=g, device=dev) * s for _ in range(2))
    mask = (torch.arange(Mmax, device=dev)[None, :] < torch.from_numpy(dlen).to(dev)[:, None])[:, :, None]
    return zq, gq, zdb * mask, gdb * mask, dlen


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("D", [64, 512])
def test_search_end_to_end(D, variant):
    """search_scores for 300 targets of 40..700 residues against a 350-residue query, chunk 128, against the per-pair loop the
    parent commit offers: alignment_scores + Decoder.forward on each pair's own slice.  score within TOL (relative); the top 10
    identical, the 10th and 11th reference values being more than 2 TOL (relative) apart -- asserted."""
    import torch
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder
    from deepblast_amd.scores import alignment_scores
    from deepblast_amd.search import search_scores
    dev = torch.device("cuda", 0)
    dec = (NeedlemanWunschDecoder, SmithWatermanDecoder)[variant]("softmax")
    T, N = 300, 350
    zq, gq, zdb, gdb, dlen = _search_problem(7000 + D + variant, T, N, D, 40, 700, dev)
    res = search_scores(dec, zq, gq, zdb, gdb, dlen, chunk=128, topk=10)
    torch.cuda.synchronize()
    want = np.zeros(T, np.float32)
    with torch.no_grad():
        for t in range(T):
            m = int(dlen[t])
            th, a = alignment_scores(zq[None], zdb[t:t + 1, :m].contiguous(), gq[None], gdb[t:t + 1, :m].contiguous())
            want[t] = float(dec(th, a)[0])
    assert res.score.shape == (T,) and res.score.grad_fn is None
    e = parity.rel_err(res.score.cpu().numpy(), want)
    print(f"\nsearch D={D} variant={variant}: score vs the per-pair loop {e:.2e}")
    assert e <= parity.TOL, e
    want_norm = want / (np.float32(N) * dlen.astype(np.float32))
    assert np.array_equal(res.normalized.cpu().numpy(), res.score.cpu().numpy() / (np.float32(N) * dlen.astype(np.float32)))
    order = np.argsort(-want_norm, kind="stable")
    v10, v11 = float(want_norm[order[9]]), float(want_norm[order[10]])
    assert v10 - v11 > 2 * parity.TOL * max(1.0, abs(v10)), (v10, v11)    # the precondition: the cut is not a near tie
    gaps = -np.diff(want_norm[order[:11]])
    if gaps.min() > 2 * parity.TOL * max(1.0, float(np.abs(want_norm[order[:11]]).max())):
        assert res.indices.cpu().tolist() == order[:10].tolist()
    else:
        assert sorted(res.indices.cpu().tolist()) == sorted(order[:10].tolist())
    assert torch.equal(res.values, res.normalized[res.indices])


@pytest.mark.gpu
def test_score_can_be_captured_in_a_graph():
    import torch
    from deepblast_amd import NeedlemanWunschDecoder
    from deepblast_amd._engine import get_engine
    get_engine().init()
    dec = NeedlemanWunschDecoder("softmax")
    B, N, M = 24, 200, 160
    g = torch.Generator(device="cuda").manual_seed(3)
    theta = torch.rand((B, N, M), generator=g, device="cuda")
    A = -torch.rand((B, N, M), generator=g, device="cuda")
    lens = torch.from_numpy(np.minimum(datagen.lengths(9, B, 1, 200), [N, M]).astype(np.int32)).cuda()
    eager, eager_l = dec.score(theta, A), dec.score(theta, A, lens)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, out_l = dec.score(theta, A), dec.score(theta, A, lens)
    for _ in range(2):
        out.fill_(float("nan")), out_l.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(eager)) and torch.equal(_bits(out_l), _bits(eager_l))
    get_engine().check_device()
