"""GPU: the drop-in Python surface end to end (Decoder -> autograd.Function -> C ABI -> HIP),
written after the reference's own tests (deepblast/tests/test_nw.py, test_nw_cuda.py, test_sw.py)."""
import os

import numpy as np
import pytest
import torch

import datagen
import parity
from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder

pytestmark = pytest.mark.gpu
DEC = {"nw": NeedlemanWunschDecoder, "sw": SmithWatermanDecoder}


@pytest.mark.parametrize("kind", ["nw", "sw"])
def test_decoding_known_answer(golden_dir, kind):
    """test_nw_cuda.py:64-76 / test_sw_cuda.py:58-70 on the 5x4 fixture."""
    d = np.load(os.path.join(golden_dir, f"g2_known_{kind}_f32.npz"))
    theta = torch.from_numpy(d["theta"]).cuda().requires_grad_()
    A = torch.from_numpy(d["A"]).cuda().requires_grad_()
    dec = DEC[kind]("softmax")
    v = dec(theta, A)
    assert v.is_cuda and v.shape == (1,)
    v.backward()
    assert parity.rel_err(v.detach().cpu().numpy(), d["Vt"]) <= parity.TOL
    assert parity.abs_err(theta.grad.cpu().numpy(), d["E"]) <= parity.TOL
    assert dec.traceback(theta.grad.squeeze()) == [tuple(r) for r in d["traceback"].tolist()]


@pytest.mark.parametrize("kind", ["nw", "sw"])
def test_quirks_and_double_backward(golden_dir, kind):
    d = np.load(os.path.join(golden_dir, f"g1_{kind}_b4_64.npz"))
    dec = DEC[kind]("softmax")
    theta = torch.from_numpy(d["theta"]).cuda().requires_grad_()
    A = torch.from_numpy(d["A"]).cuda().requires_grad_()
    Z = torch.from_numpy(d["Z"]).cuda()
    Vt = dec(theta, A)
    Vt.backward(torch.from_numpy(d["Et"]).cuda())
    assert parity.abs_err(theta.grad.cpu().numpy(), d["E_et"]) <= parity.TOL
    assert torch.equal(A.grad, A.detach())                    # nw.py:337-339,355
    theta.grad = None
    A.grad = None
    aln = dec.decode(theta, A)                                 # alignment.py:124
    assert aln.is_cuda and aln.requires_grad and aln.shape == theta.shape
    (aln * Z).sum().backward()
    assert parity.abs_err(theta.grad.cpu().numpy(), d["Ed"], scale=True) <= parity.TOL
    assert A.grad is None                                      # nw.py:386
    ed = theta.grad.cpu().numpy()
    et = torch.from_numpy(d["Et"]).cuda().requires_grad_()
    g, _ = torch.autograd.grad(dec(theta, A), (theta, A), et, create_graph=True)
    (vtd,) = torch.autograd.grad((g * Z).sum(), et)
    assert parity.rel_err(vtd.cpu().numpy(), d["Vtd_et"]) <= parity.TOL
    # the plain rule as well (parity.check_second_order); the fixtures are fp32, the float64 reference is the C oracle's f64 path
    # on the same inputs (Ed from decode(): Et = 1; Vtd with the fixture's Et)
    variant = {"nw": 0, "sw": 1}[kind]

    def ref64():
        r1 = parity.oracle_f64(d["theta"], d["A"], None, d["Z"], variant)
        r2 = parity.oracle_f64(d["theta"], d["A"], d["Et"], d["Z"], variant)
        return {"Ed": r1["Ed"], "Vtd": r2["Vtd"]}
    parity.check_second_order({"Ed": ed, "Vtd": vtd.detach().cpu().numpy()}, {"Ed": d["Ed"], "Vtd": d["Vtd_et"]}, ref64,
                              f"double backward {kind}")


@pytest.mark.parametrize("kind", ["nw", "sw"])
def test_gradcheck_style_finite_differences(kind):
    """test_nw_cuda.py:51-61 uses gradcheck with eps=atol=rtol=1e-1 in fp32; here the directional
    derivative of sum(Vt) along a random direction is compared with <E, d> at matching tolerance,
    and the directional derivative of <E, Z> with <Ed, d> (gradgradcheck analogue)."""
    B, N, M = 3, 5, 5
    theta, A = datagen.theta_A(77, B, N, M)
    theta = torch.from_numpy(theta).cuda()
    A = torch.from_numpy(A).cuda().requires_grad_()  # decode() differentiates w.r.t. (theta, A) like the reference
    dirn = torch.from_numpy(datagen.normal(78, (B, N, M))).cuda()
    Z = torch.from_numpy(datagen.normal(79, (B, N, M))).cuda()
    dec = DEC[kind]("softmax")
    eps = 1e-2

    def f(t):
        return dec(t, A).sum()

    def g(t):
        t = t.detach().requires_grad_()
        return (dec.decode(t, A) * Z).sum()

    t = theta.clone().requires_grad_()
    (E,) = torch.autograd.grad(f(t), t)
    fd = (f(theta + eps * dirn) - f(theta - eps * dirn)) / (2 * eps)
    assert abs(float(fd.detach()) - float((E * dirn).sum())) < 2e-2
    if kind == "sw":
        # The reference has no gradgradcheck for SW (test_sw.py) and its SW double-backward is not the
        # true Hessian-vector product: the adjoint loops keep padded row/col 1 that forward/backward
        # skip (sw.py:150-151,199-202 vs 54-55,107-110; the CPU oracle gives -3.95 vs -3.23 here).
        # We match the reference (tests/test_parity_gpu.py), not the finite difference.
        return
    t = theta.clone().requires_grad_()
    (Ed,) = torch.autograd.grad((dec.decode(t, A) * Z).sum(), t)
    fd2 = (g(theta + eps * dirn) - g(theta - eps * dirn)) / (2 * eps)
    assert abs(float(fd2.detach()) - float((Ed * dirn).sum())) < 2e-2


def test_outputs_stay_on_input_device_and_no_grad_path():
    """nw_cuda.py:270-271 keeps results on the GPU; score() runs forward under no_grad (alignment.py:136)."""
    theta, A = datagen.theta_A(5, 2, 30, 20)
    theta, A = torch.from_numpy(theta).cuda(), torch.from_numpy(A).cuda()
    dec = NeedlemanWunschDecoder("softmax")
    with torch.no_grad():
        v = dec(theta, A)
    assert v.is_cuda and not v.requires_grad
    ref = parity.oracle_all(theta.cpu().numpy(), A.cpu().numpy(), None, None, 0)
    assert parity.rel_err(v.cpu().numpy(), ref["Vt"]) <= parity.TOL


def test_side_stream_ordering():
    """Kernels are enqueued on torch's current stream: results on a side stream are ordered with
    the producing ops without extra synchronisation."""
    theta, A = datagen.theta_A(6, 8, 200, 180)
    ref = parity.oracle_all(theta, A, None, None, 0)
    s = torch.cuda.Stream()
    dec = NeedlemanWunschDecoder("softmax")
    with torch.cuda.stream(s):
        t = torch.from_numpy(theta).cuda().requires_grad_()
        a = torch.from_numpy(A).cuda() * 1.0
        v = dec(t, a)
        v.sum().backward()
        E = t.grad.clone()
    s.synchronize()
    assert parity.abs_err(E.cpu().numpy(), ref["E"]) <= parity.TOL


def test_padded_batch_reference_semantics_and_lengths_extension():
    """BASELINE.json configs[2]: the reference runs the DP over the full padded matrix (no lengths
    argument, alignment.py:117-124); lengths-aware mode is an extension checked per item."""
    B, N, M = 5, 96, 130
    theta, A = datagen.theta_A(8, B, N, M)
    lens = datagen.lengths(9, B, 10, 96)
    dec = NeedlemanWunschDecoder("softmax")
    t = torch.from_numpy(theta).cuda().requires_grad_()
    a = torch.from_numpy(A).cuda()
    dec(t, a).sum().backward()
    ref = parity.oracle_all(theta, A, None, None, 0)
    assert parity.abs_err(t.grad.cpu().numpy(), ref["E"]) <= parity.TOL
    t.grad = None
    v = dec(t, a, torch.from_numpy(lens).cuda())
    v.sum().backward()
    refl = parity.oracle_lens(theta, A, None, None, 0, lens)
    assert parity.rel_err(v.detach().cpu().numpy(), refl["Vt"]) <= parity.TOL
    assert parity.abs_err(t.grad.cpu().numpy(), refl["E"]) <= parity.TOL


def test_batched_device_traceback_matches_host(golden_dir):
    """sdp_traceback_i32 (one wavefront per pair) is integer-identical to the per-pair host walk
    (nw.py:401-444), on real expected-alignment matrices, with per-pair lengths, and on the reference's
    traceback fixtures including the walks that raise IndexError."""
    import time
    from deepblast_amd._dp import traceback as host_traceback
    from deepblast_amd._engine import get_engine
    B, N, M = 48, 96, 130
    theta, A = datagen.theta_A(31, B, N, M)
    theta = (theta * 3.0).astype(np.float32)
    lens = datagen.lengths(32, B, 1, 96)
    lens[0] = (N, M)
    dec = NeedlemanWunschDecoder("softmax")
    for ln in (None, torch.from_numpy(lens).cuda()):
        t = torch.from_numpy(theta).cuda().requires_grad_()
        a = torch.from_numpy(A).cuda().requires_grad_()
        aln = dec.decode(t, a, ln).detach()
        states, counts = get_engine().traceback(aln, ln)
        states, counts = states.cpu().numpy(), counts.cpu().numpy()
        E = aln.cpu().numpy()
        n_ok = 0
        for b in range(B):
            n, m = (N, M) if ln is None else lens[b]
            try:  # degenerate blocks (e.g. a single row) make the reference walk leave the matrix
                want = host_traceback(E[b, :n, :m])
            except IndexError:
                assert counts[b] == -1, b
                continue
            assert [tuple(r) for r in states[b, :counts[b]].tolist()] == want, b
            n_ok += 1
        assert n_ok >= B - 8
        if ln is None:
            assert dec.traceback_batch(aln) == [host_traceback(E[b]) for b in range(B)]
    # fixtures from the reference (float32 and float64 inputs, some raising IndexError)
    d = np.load(os.path.join(golden_dir, "g8_tracebacks.npz"))
    for k in range(int(d["count"])):
        g = torch.from_numpy(d[f"t{k}_grad"].astype(np.float32)).cuda()[None]
        if bool(d[f"t{k}_ok"]):
            assert dec.traceback_batch(g)[0] == [tuple(r) for r in d[f"t{k}_states"].tolist()], k
        else:
            with pytest.raises(IndexError):
                dec.traceback_batch(g)
    # one launch for a large batch vs the per-pair host loop (alignment.py:165-170): timing for DESIGN.md
    B, N, M = 256, 512, 512
    theta, A = datagen.theta_A(33, B, N, M)
    t = torch.from_numpy(theta).cuda().requires_grad_()
    a = torch.from_numpy(A).cuda().requires_grad_()
    aln = dec.decode(t, a).detach()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    states, counts = get_engine().traceback(aln)
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0
    E = aln.cpu().numpy()
    t0 = time.perf_counter()
    host = [host_traceback(E[b]) for b in range(8)]
    t_host = (time.perf_counter() - t0) / 8 * B
    st, ct = states.cpu().numpy(), counts.cpu().numpy()
    for b in range(8):
        assert [tuple(r) for r in st[b, :ct[b]].tolist()] == host[b]
    print(f"traceback B={B} {N}x{M}: device {t_dev * 1e3:.2f} ms, host loop (extrapolated) {t_host * 1e3:.0f} ms")


def test_device_traceback_cuda_rule(golden_dir):
    """sdp_traceback_rule_i32(SDP_TRACEBACK_CUDA): the walk of the reference's GPU classes (nw_cuda.py:273-317) on the
    device -- integer-identical to the fixtures from the real classes, to the host walk on arbitrary matrices (shapes
    around the 32-cell window, per-pair lengths, sentinel values inside the matrix), and never -1."""
    import torch
    from deepblast_amd._dp import traceback as host_traceback
    from deepblast_amd._engine import get_engine
    dec = NeedlemanWunschDecoder("softmax", traceback_rule="cuda")
    d = np.load(os.path.join(golden_dir, "g12_tracebacks_cuda.npz"))
    for k in range(int(d["count"])):
        g = torch.from_numpy(d[f"t{k}_grad"].astype(np.float32)).cuda()[None]
        assert dec.traceback_batch(g)[0] == [tuple(r) for r in d[f"t{k}_nw"].tolist()], k
    rng = np.random.default_rng(12)
    n_diff = 0
    for (N, M) in [(1, 1), (1, 9), (9, 1), (2, 2), (31, 33), (32, 32), (33, 31), (64, 65), (5, 200), (200, 5), (150, 97), (70, 300)]:
        B = 24
        g = rng.normal(size=(B, N, M)).astype(np.float32)
        g[B // 3: 2 * B // 3] = np.abs(g[B // 3: 2 * B // 3])
        g[2 * B // 3:][rng.random((B - 2 * B // 3, N, M)) < 0.05] = -1e10            # the cuda rule's sentinel inside the matrix
        for b in range(0, B, 4):
            for k in range(min(N, M)):
                g[b, N - 1 - k, M - 1 - k] += 5.0
        lens = np.stack([rng.integers(1, N + 1, B), rng.integers(1, M + 1, B)], axis=1).astype(np.int32)
        for ln in (None, lens):
            states, counts = get_engine().traceback(torch.from_numpy(g).cuda(), None if ln is None else torch.from_numpy(ln).cuda(), rule="cuda")
            states, counts = states.cpu().numpy(), counts.cpu().numpy()
            assert (counts > 0).all()
            for b in range(B):
                n, m = (N, M) if ln is None else ln[b]
                want = host_traceback(g[b, :n, :m], "cuda")
                assert [tuple(int(v) for v in r) for r in states[b, :counts[b]]] == want, (N, M, b)
                try:
                    n_diff += want != host_traceback(g[b, :n, :m])
                except IndexError:
                    n_diff += 1
    assert n_diff > 0


def test_device_traceback_on_arbitrary_matrices_matches_host_walk():
    """The windowed walk against the host walk on matrices that are NOT alignment matrices: random values send the walk
    along edges, through python's index wrap (nw.py:423) and off the matrix (IndexError -> count -1); entries equal to
    the reference's floor value (-100000) trigger its stop rule anywhere.  Shapes around the 32-cell window."""
    import torch
    from deepblast_amd._dp import traceback as host_traceback
    from deepblast_amd._engine import get_engine
    rng = np.random.default_rng(11)
    shapes = [(1, 1), (1, 9), (9, 1), (2, 2), (31, 33), (32, 32), (33, 31), (64, 65), (5, 200), (200, 5), (150, 97), (70, 300)]
    n_bad = n_wrap = 0
    for (N, M) in shapes:
        B = 24
        g = rng.normal(size=(B, N, M)).astype(np.float32)
        g[B // 3: 2 * B // 3] = np.abs(g[B // 3: 2 * B // 3])                      # positive: no early stop
        g[2 * B // 3:][rng.random((B - 2 * B // 3, N, M)) < 0.3] = -100000.0        # floor values inside the matrix
        for b in range(0, B, 4):                                                     # a bright diagonal band: long interior walks
            for k in range(min(N, M)):
                g[b, N - 1 - k, M - 1 - k] += 5.0
        lens = np.stack([rng.integers(1, N + 1, B), rng.integers(1, M + 1, B)], axis=1).astype(np.int32)
        for ln in (None, lens):
            states, counts = get_engine().traceback(torch.from_numpy(g).cuda(), None if ln is None else torch.from_numpy(ln).cuda())
            states, counts = states.cpu().numpy(), counts.cpu().numpy()
            for b in range(B):
                n, m = (N, M) if ln is None else ln[b]
                try:
                    want = host_traceback(g[b, :n, :m])
                except IndexError:
                    assert counts[b] == -1, (N, M, b)
                    n_bad += 1
                    continue
                assert counts[b] == len(want), (N, M, b, counts[b], len(want))
                assert [tuple(int(v) for v in r) for r in states[b, :counts[b]]] == want, (N, M, b)
                n_wrap += any(i < 0 or j < 0 for i, j, _ in want)
    assert n_bad > 0 and n_wrap > 0, (n_bad, n_wrap)   # the fuzz reaches both quirks
