"""GPU: the true gap-score gradients G = E (Qx + Qy) and Gd = Ed (Qx + Qy) + E (Qdx + Qdy) (csrc/sdp_gap.hip, Decoder(...,
gap_gradient=True)) against finite differences in float64, against the CPU oracle in fp32 on every state layout the sweeps
produce, and the things that must not move: the sweeps' own results, the cells outside the blocks."""
import numpy as np
import pytest
import torch

import datagen
import gap_ref
import hard_ref
import parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXACT_FLAG, REF_FLAG, NO_FILL = 0x100, 0x400, 0x10000


def _decoders():
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder
    return NeedlemanWunschDecoder, SmithWatermanDecoder


def _eng():
    from deepblast_amd._engine import get_engine
    return get_engine()


def _d(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t.requires_grad_() if grad else t


# ---- 1. float64: gradcheck / gradgradcheck with respect to theta AND A, torch's default tolerances -------------------------
F64_CASES = {"2x5x4": (2, 5, 4, None), "7x9_lens": (2, 7, 9, [[7, 9], [3, 6]])}


def _f64_case(name, variant):
    B, N, M, lens = F64_CASES[name]
    theta, A = datagen.theta_A(31, B, N, M, dtype=np.float64)
    dec = _decoders()[variant]("softmax", gap_gradient=True)
    tl = None if lens is None else torch.tensor(lens)
    return (lambda t, a: dec(t, a, tl)), (_d(theta, True), _d(A, True))


@pytest.mark.parametrize("case", sorted(F64_CASES))
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_gradcheck_float64(variant, case):
    """fails on the parent for A: the gradient handed back for A was A itself"""
    fn, inputs = _f64_case(case, variant)
    assert torch.autograd.gradcheck(fn, inputs)


@pytest.mark.parametrize("case", sorted(F64_CASES))
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_gradgradcheck_float64(variant, case):
    """Second order with respect to theta, A and the cotangent of Vt.  Smith-Waterman: a flagged decoder runs the adjoint pair on
    tangents zeroed on row 0 / column 0 and zeroes Ed there (_dp.py); the reference's own pair, which the default decoder
    keeps, fails this check on those border entries (analytic -0.0381 where the numerical Jacobian is 0, measured)."""
    fn, inputs = _f64_case(case, variant)
    assert torch.autograd.gradgradcheck(fn, inputs)


# ---- 2. fp32 against the CPU oracle, on every layout path ---------------------------------------------------------------
def _engine_gap(theta, A, Et, variant, lens, Z=None, ZG=None, exact=False):
    """first order from the packed (exact=False) or the float2 state; with Z also second order (exact state) -> numpy dict"""
    eng = _eng()
    t, a = _d(theta), _d(A)
    B = t.shape[0]
    et = torch.ones(B, device=DEV) if Et is None else _d(Et)
    ln = None if lens is None else _d(np.asarray(lens, np.int32))
    _, Q = eng.forward(t, a, variant, ln, exact_state=exact)
    E = eng.backward(et, Q, tuple(t.shape), variant, ln, exact_state=exact)
    out = {"E": E, "G": eng.gap_gradient(E, Q, tuple(t.shape), variant, ln, exact_state=exact)}
    if Z is not None:
        assert exact
        Vtd, Qd = eng.adjoint_forward(Q, _d(Z), None if ZG is None else _d(ZG), variant, ln)
        Ed = eng.adjoint_backward(E, Q, Qd, variant, ln)
        out.update(Ed=Ed, Vtd=Vtd, Gd=eng.gap_gradient2(E, Ed, Q, Qd, variant, ln))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(theta, A, Et, variant, lens, Z, ZG, what, second=True):
    ref = gap_ref.reference(theta, A, Et, variant, lens, Z if second else None, ZG if second else None)
    for exact in (False, True):
        got = _engine_gap(theta, A, Et, variant, lens, Z if (exact and second) else None, ZG, exact)
        err = parity.abs_err(got["G"], ref["G"])
        print(f"{what} exact={exact}: max|dG| = {err:.3e} (max|G| = {float(np.max(np.abs(ref['G']))):.3f})")
        assert np.isfinite(got["G"]).all() and err <= parity.TOL, (what, exact, err)
        if lens is not None:   # +0 outside each pair's block
            for b, (n, m) in enumerate(lens):
                assert not got["G"][b, n:].view(np.uint32).any() and not got["G"][b, :, m:].view(np.uint32).any(), (what, b)
        if variant == 1:       # +0 on row 0 and column 0 of a Smith-Waterman block
            assert not got["G"][:, 0].view(np.uint32).any() and not got["G"][:, :, 0].view(np.uint32).any(), what
    if second:
        ref64 = lambda: {"Ed": gap_ref.reference(theta, A, Et, variant, lens, Z, ZG, dtype=np.float64)["Gd"]}   # noqa: E731
        rec = parity.check_second_order({"Ed": got["Gd"]}, {"Ed": ref["Gd"]}, ref64, f"{what} Gd")
        print(f"{what}: Gd {rec}")
        if lens is not None:
            for b, (n, m) in enumerate(lens):
                assert not got["Gd"][b, n:].any() and not got["Gd"][b, :, m:].any(), (what, b)


ROUTED_LENS = [[2, 2048], [190, 2040], [1, 1], [31, 600], [192, 9], [100, 100]]
#           single cell and thin | strip and chunk edges | strips in rounds | the 2048-column fallback, whole-shape float2
SHAPES = [(1, 1, 1), (2, 3, 5), (2, 64, 32), (2, 65, 33), (2, 63, 31), (3, 130, 170), (1, 70, 2048), (1, 40, 2048)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_fp32_against_the_oracle(variant, shape):
    B, N, M = shape
    theta, A = datagen.theta_A(41, B, N, M)
    Et = (0.5 + datagen.uniform(42, (B,))).astype(np.float32)          # non-uniform
    _check(theta, A, Et, variant, None, datagen.normal(43, shape), datagen.normal(44, shape), f"{shape} v{variant}")


def test_fp32_longer_than_the_packed_state_serves():
    """N + M > 4096: the float2 state whatever was asked"""
    shape = (1, 2100, 2000)
    theta, A = datagen.theta_A(45, *shape)
    _check(theta, A, None, 0, None, datagen.normal(46, shape), datagen.normal(47, shape), "2100x2000")


def test_fp32_per_pair_routing():
    """thin long pairs of a packed batch keep a float2 record inside their own packed slot"""
    shape = (6, 192, 2048)
    theta, A = datagen.theta_A(48, *shape)
    Et = (0.5 + datagen.uniform(49, (6,))).astype(np.float32)
    for variant in (0, 1):
        _check(theta, A, Et, variant, ROUTED_LENS, datagen.normal(50, shape), datagen.normal(70, shape), f"routed v{variant}")


def test_fp32_state_written_by_a_parts_launch():
    """16 x 1024 x 1024 with lengths: the forward sweep spreads every pair over several workgroups; first order (the second-order
    pass reads the float2 streams at the same addresses whoever wrote them)"""
    B, N, M = 16, 1024, 1024
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lib = _eng().lib
    assert lib.sdp_plan_parts(0, B, N, M, 1, 0, cus) > 1 and lib.sdp_plan_parts(0, B, N, M, 1, 1, cus) > 1
    theta, A = datagen.theta_A(51, B, N, M)
    lens = datagen.lengths(52, B, 700, 1024)
    lens[0] = (1024, 1024)
    _check(theta, A, None, 0, lens.tolist(), None, None, "parts", second=False)


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_decoder_routes(variant):
    """through the decoder: the transposed route (2 x 40 x 2100), reference arithmetic (2 x 37 x 101), and the broadcast scalar
    cotangent of Vt.sum().backward()"""
    for shape, kw in (((2, 40, 2100), {}), ((2, 37, 101), {"arithmetic": "reference"}), ((3, 130, 170), {})):
        theta, A = datagen.theta_A(54, *shape)
        Z = datagen.normal(55, shape)
        ref = gap_ref.reference(theta, A, None, variant, None, Z, None, decoder=True)
        dec = _decoders()[variant]("softmax", gap_gradient=True, **kw)
        t, a = _d(theta, True), _d(A, True)
        dec(t, a).sum().backward()
        assert parity.abs_err(a.grad.cpu().numpy(), ref["G"]) <= parity.TOL and parity.abs_err(t.grad.cpu().numpy(), ref["E"]) <= parity.TOL
        t, a = _d(theta, True), _d(A, True)
        (dec.decode(t, a) * _d(Z)).sum().backward()
        ref64 = lambda: {"Ed": gap_ref.reference(theta, A, None, variant, None, Z, None, dtype=np.float64, decoder=True)["Gd"]}   # noqa: E731
        parity.check_second_order({"Ed": a.grad.cpu().numpy()}, {"Ed": ref["Gd"]}, ref64, f"decoder {shape} {kw} Gd")


# ---- 3. forbidden gaps ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_forbidden_gaps_give_exact_zeros(variant):
    shape = (2, 70, 200)
    theta, A = datagen.theta_A(56, *shape)
    barred = datagen.uniform(57, shape) < 0.05
    A = np.where(barred, -np.inf, A).astype(np.float32)
    assert 0.03 < barred.mean() < 0.07
    for exact in (False, True):
        got = _engine_gap(theta, A, None, variant, None, exact=exact)
        assert np.isfinite(got["E"]).all() and np.isfinite(got["G"]).all()
        assert not got["G"][barred].any() and got["G"].any()


# ---- 4. fill=False with lengths ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [0, EXACT_FLAG, REF_FLAG], ids=["packed", "exact", "reference"])
def test_no_fill_leaves_the_outside_alone(flag):
    from deepblast_amd._engine import REF
    B, N, M = 3, 70, 100
    lens = [[70, 100], [33, 100], [64, 37]]
    theta, A = datagen.theta_A(58, B, N, M)
    ref = gap_ref.reference(theta, A, None, 0, lens)
    eng = _eng()
    ln = _d(np.asarray(lens, np.int32))
    exact = {0: False, EXACT_FLAG: True, REF_FLAG: REF}[flag]
    _, Q = eng.forward(_d(theta), _d(A), 0, ln, exact_state=exact)
    E = eng.backward(torch.ones(B, device=DEV), Q, (B, N, M), 0, ln, exact_state=exact, no_fill=True)
    poison = np.float32(-7.25e11)
    for fill in (False, True):
        G = torch.full((B, N, M), float(poison), device=DEV)
        eng.call("sdp_gap_gradient_f32", "sdp_gap_kernel", 0, E, Q, G, B, N, M, ln, flag | (0 if fill else NO_FILL))
        via_engine = eng.gap_gradient(E, Q, (B, N, M), 0, ln, exact_state=exact, no_fill=not fill).cpu().numpy()
        G = G.cpu().numpy()
        for b, (n, m) in enumerate(lens):
            assert parity.abs_err(G[b, :n, :m], ref["G"][b, :n, :m]) <= parity.TOL
            assert np.array_equal(G[b, :n, :m], via_engine[b, :n, :m])
            outside = np.concatenate([G[b, n:].ravel(), G[b, :n, m:].ravel()])
            assert (not outside.view(np.uint32).any()) if fill else (outside == poison).all(), (flag, fill, b)


# ---- 5. the sweeps are untouched ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["3x130x170", "routed"])
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_sweeps_results_are_the_same_bits_with_the_flag_on(variant, case):
    """Vt, E and Ed as uint32.  Smith-Waterman: a flagged decoder hands the adjoint pair the tangent without its row 0 / column 0
    and zeroes Ed there (the true Hessian-vector product, _dp.py), so its Ed is held to the bits of the DEFAULT decoder's Ed for
    that tangent, border zeroed: the same sweeps on the same inputs."""
    shape, lens = ((3, 130, 170), None) if case == "3x130x170" else ((6, 192, 2048), torch.tensor(ROUTED_LENS))
    theta, A = datagen.theta_A(59, *shape)
    Zn = datagen.normal(60, shape)
    got = []
    for flag in (False, True):
        dec = _decoders()[variant]("softmax", gap_gradient=flag)
        t, a = _d(theta, True), _d(A, True)
        Vt = dec(t, a, lens)
        Vt.sum().backward()
        E = t.grad.clone()
        t.grad = None
        Z = _d(Zn if (flag or variant == 0) else gap_ref.without_border(Zn))
        (dec.decode(t, a, lens) * Z).sum().backward()
        Ed = t.grad.detach().cpu().numpy()
        if variant == 1 and not flag:
            Ed[:, 0] = 0
            Ed[:, :, 0] = 0
        got.append([x.view(np.uint32) for x in (Vt.detach().cpu().numpy(), E.cpu().numpy(), Ed)])
    for name, x, y in zip(("Vt", "E", "Ed"), *got):
        assert np.array_equal(x, y), name


# ---- 6. end to end at the gap embeddings --------------------------------------------------------------------------------
def _soft_dp(theta, A, variant):
    """plain torch: V[i,j] = theta + logsumexp(A + V[i-1,j], V[i-1,j-1], A + V[i,j-1]); Smith-Waterman starts at row / column 2"""
    B, N, M = theta.shape
    lo = 2 if variant else 1
    V = [[theta.new_zeros(B) for _ in range(M + 1)] for _ in range(N + 1)]
    for i in range(lo, N + 1):
        for j in range(lo, M + 1):
            a = A[:, i - 1, j - 1]
            V[i][j] = theta[:, i - 1, j - 1] + torch.logsumexp(torch.stack([a + V[i - 1][j], V[i - 1][j - 1], a + V[i][j - 1]]), dim=0)
    return V[N][M]


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_gap_embeddings_get_the_true_gradient(variant):
    from deepblast_amd.scores import alignment_scores
    B, N, M, D = 2, 6, 7, 16
    emb = [datagen.normal(61 + k, s) * 0.5 for k, s in enumerate(((B, N, D), (B, M, D), (B, N, D), (B, M, D)))]
    zx, zy, gx, gy = (_d(e, True) for e in emb)
    theta, A = alignment_scores(zx, zy, gx, gy)
    _decoders()[variant]("softmax", gap_gradient=True)(theta, A).sum().backward()
    # float64 autograd through the scores' definition (theta = softplus(zx zy^T), A = logsigmoid(gx gy^T)) and the loop above
    zx64, zy64, gx64, gy64 = (torch.from_numpy(e.astype(np.float64)).requires_grad_() for e in emb)
    F = torch.nn.functional
    _soft_dp(F.softplus(zx64 @ zy64.transpose(1, 2)), F.logsigmoid(gx64 @ gy64.transpose(1, 2)), variant).sum().backward()
    for name, got, want in (("zx", zx, zx64), ("zy", zy, zy64), ("gx", gx, gx64), ("gy", gy, gy64)):
        scale = float(want.grad.abs().max())
        err = float((got.grad.cpu().double() - want.grad).abs().max())
        print(f"{name}: err {err:.3e} of max|grad| {scale:.3f}")
        assert scale > 0 and err <= parity.TOL * scale, (name, err, scale)


def test_decode_loss_reaches_the_gap_scores():
    """decode_loss with a gap_gradient decoder is the unfused composition: A gets Gd, not None"""
    from deepblast_amd import losses
    B, N, M = 2, 40, 50
    theta, A = datagen.theta_A(65, B, N, M)
    first, Gm = _d(datagen.uniform(66, (B, N, M))), torch.ones(B, N, M, device=DEV)
    lens = [[40, 50], [33, 20]]
    xl, yl = [40, 33], [50, 20]
    dec = _decoders()[0]("softmax", gap_gradient=True)
    t, a = _d(theta, True), _d(A, True)
    value, E = losses.decode_loss(dec, losses.SoftAlignmentLoss(), t, a, first, xl, yl, Gm, lens)
    value.backward()
    t2, a2 = _d(theta, True), _d(A, True)
    losses.SoftAlignmentLoss()(first, dec.decode(t2, a2, torch.tensor(lens)), xl, yl, Gm).backward()
    assert a.grad is not None and a.grad.abs().max() > 0 and torch.equal(a.grad, a2.grad) and torch.equal(t.grad, t2.grad)
    t3, a3 = _d(theta, True), _d(A, True)
    losses.decode_loss(_decoders()[0]("softmax"), losses.SoftAlignmentLoss(), t3, a3, first, xl, yl, Gm, lens)[0].backward()
    assert a3.grad is None and parity.abs_err(t3.grad.cpu().numpy(), t.grad.cpu().numpy()) <= parity.TOL


# ---- 7. hard-max ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_hardmax_gap_gradient_bit_for_bit(variant):
    B, N, M = 4, 70, 45
    th, a = hard_ref.quarter_scores(67, B, N, M)
    lens = [[70, 45], [1, 1], [65, 44], [3, 45]]
    Et = np.array([2.5, 1.0, -1.25, 0.5], np.float32)
    ref = hard_ref.batch(th, a, variant, lens, Et=Et)
    want = np.zeros((B, N, M), np.float32)
    for b, cells in enumerate(ref["cells"]):
        for (i, j, k) in cells:
            if k != 1:
                want[b, i, j] = Et[b]
    assert want.any()
    t, A = _d(th, True), _d(a, True)
    _decoders()[variant]("hardmax", gap_gradient=True)(t, A, torch.tensor(lens)).backward(_d(Et))
    assert np.array_equal(t.grad.cpu().numpy().view(np.uint32), ref["E"].view(np.uint32))
    assert np.array_equal(A.grad.cpu().numpy().view(np.uint32), want.view(np.uint32))
