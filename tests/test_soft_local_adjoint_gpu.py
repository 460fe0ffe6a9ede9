"""GPU: the soft local operator's adjoint pair (csrc/sdp_soft_local_adj.hip) against the float64 definition
(tests/soft_local_adjoint_ref.py, held to autograd by tests/test_soft_local_adjoint.py) on the same fp32 inputs, under
tests/parity.py's rules: plain abs_err(Ed) <= TOL, abs_err(Gd) <= TOL, rel_err(Vtd) <= TOL, cotangents uniform in [-1, 1].  On every
parity case plain fp32 arithmetic alone stays within TOL / 2 (tests/test_soft_local_adjoint.py asserts it; DESIGN.md 3.17 has the
figures)."""
import numpy as np
import pytest
import torch

import soft_local_adjoint_ref as adj
import soft_local_ref as ref
import strip_schedule
from parity import TOL, abs_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = [c for c in adj.CASES if c[3] == adj.B and c[1:3] != (3, 2100)]
WIDE = [c for c in adj.CASES if c[3] == 1]
LENS = ((0, 5), (5, 0), (1, 150), (130, 1), (137, 160), (130, 150), (65, 33))       # (137, 160): clamped to the tensor
WIDE_LENS = ((513, 2048), (449, 1983), (512, 1), (1, 2048), (0, 7))     # nine strips and eight; a column; a row; nothing


def _engine():
    from deepblast_amd._engine import get_engine
    return get_engine()


def _decoder():
    from deepblast_amd.local import SoftLocalDecoder
    return SoftLocalDecoder(second_order=True)


def _dev(x):
    return None if x is None else torch.from_numpy(np.array(x, copy=True, order="C")).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _run(th, a, ze, zg, lens=None, et=None, want_G=True):
    """the forward sweep and the adjoint pair through the engine -> numpy (Vtd, Ed, Gd)"""
    eng = _engine()
    t, A, ln = _dev(th), _dev(a), _dev(lens)
    shape = tuple(t.shape)
    Et = torch.ones(shape[0], device=DEV) if et is None else _dev(et)
    Vt, state = eng.soft_local_forward(t, A, ln)
    Vtd, state_d = eng.soft_local_adjoint_forward(state, Vt, _dev(ze), _dev(zg), shape, ln)
    Ed, Gd = eng.soft_local_adjoint_backward(state, state_d, Vt, Vtd, Et, shape, ln, want_G=want_G)
    torch.cuda.synchronize()
    return Vtd.cpu().numpy(), Ed.cpu().numpy(), None if Gd is None else Gd.cpu().numpy()


def _check(got, want, what):
    errs = {"Vtd": rel_err(got[0], want["Vtd"]), "Ed": abs_err(got[1], want["Ed"])}
    if got[2] is not None:
        errs["Gd"] = abs_err(got[2], want["Gd"])
    print(what, " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert all(np.isfinite(v) and v <= TOL for v in errs.values()), (what, errs)
    return errs


def _zero_outside(Ed, Gd, lens, what):
    N, M = Ed.shape[1:]
    for b, (n, m) in enumerate(lens):
        mask = np.ones((N, M), bool)
        mask[:max(min(n, N), 0), :max(min(m, M), 0)] = False
        assert not _bits(Ed[b])[mask].any() and not _bits(Gd[b])[mask].any(), (what, b, n, m)     # +0, by bit pattern


@pytest.mark.parametrize("family,n,m,k", SMALL, ids=[f"{f}-{n}x{m}" for (f, n, m, k) in SMALL])
def test_against_float64(family, n, m, k):
    _check(_run(*adj.case(family, n, m, k)), adj.want(family, n, m, k), f"{family} {n}x{m}")


def test_et_of_either_sign_and_zero():
    th, a, ze, zg = adj.case("model", 65, 33)
    et = np.asarray([1.0, -2.5, 0.0], np.float32)
    want = adj.batch(th, a, ze, zg, Et=et)
    one = adj.want("model", 65, 33)
    assert np.abs(want["Ed"] - one["Ed"] * et[:, None, None]).max() <= 1e-12 and np.abs(want["Vtd"] - one["Vtd"]).max() <= 1e-12
    Vtd, Ed, Gd = _run(th, a, ze, zg, et=et)
    _check((Vtd, Ed, Gd), want, "Et")
    assert not Ed[2].any() and not Gd[2].any() and abs(Vtd[2]) > 1e-3          # Et = 0: Ed = Gd = 0, Vtd is still the definition's


@pytest.mark.parametrize("family,n,m", [("model", 65, 33), ("floor", 130, 150)])
def test_one_cotangent_alone(family, n, m):
    th, a, ze, zg = adj.case(family, n, m)
    full = _run(th, a, ze, zg)
    for which, (e, g) in (("ZG = None", (ze, None)), ("ZE = None", (None, zg))):
        got = _run(th, a, e, g)
        _check(got, adj.batch(th, a, e, g), f"{family} {n}x{m} {which}")
        zeros = _run(th, a, e if e is not None else np.zeros_like(ze), g if g is not None else np.zeros_like(zg))
        for x, y in zip(got, zeros):          # NULL means zeros, bit for bit
            assert np.array_equal(_bits(x), _bits(y)), which
    Vtd, Ed, none = _run(th, a, ze, zg, want_G=False)
    assert none is None and np.array_equal(_bits(Ed), _bits(full[1])) and np.array_equal(_bits(Vtd), _bits(full[0]))


def _lens_case():
    th, a, ze, zg = adj.case("floor", 130, 150, len(LENS))
    return th, a, ze, zg, np.asarray(LENS, np.int32)


def test_lengths():
    th, a, ze, zg, lens = _lens_case()
    want = adj.batch(th, a, ze, zg, lens)
    Vtd, Ed, Gd = _run(th, a, ze, zg, lens)
    for b, (n, m) in enumerate(LENS):       # every pair against the definition on its own slice
        one = {k: v[b:b + 1] for k, v in want.items()}
        _check((Vtd[b:b + 1], Ed[b:b + 1], Gd[b:b + 1]), one, f"lens {n}x{m}")
        if n < 1 or m < 1:
            assert _bits(Vtd[b:b + 1])[0] == 0
    _zero_outside(Ed, Gd, LENS, "lens")
    full = adj.batch(th[4:6], a[4:6], ze[4:6], zg[4:6])
    assert all(np.array_equal(want[k][4:6], full[k]) for k in want)       # the clamped pair is the full pair


# ---- full width, the 64 KB (first order) / 128 KB (adjoint backward) launch and seven waves ----
@pytest.mark.parametrize("family,n,m,k", WIDE, ids=[f"{f}-{n}x{m}" for (f, n, m, k) in WIDE])
def test_full_width_against_float64(family, n, m, k):
    c = strip_schedule.check_wide_shapes("sdp_soft_local.h")
    assert (strip_schedule.strips(c, n), strip_schedule.waves(c, n, m)) == strip_schedule.WIDE[(n, m)]
    _check(_run(*adj.case(family, n, m, 1)), adj.want(family, n, m, 1), f"wide {family} {n}x{m}")


def test_full_width_lengths():
    """pairs of eight and of nine strips, a single column, a single row and an empty pair in one seven-wave launch"""
    N, M = 513, 2048
    th, a, ze, zg = adj.case("islands", N, M, len(WIDE_LENS))
    lens = np.asarray(WIDE_LENS, np.int32)
    want = adj.batch(th, a, ze, zg, lens)
    Vtd, Ed, Gd = _run(th, a, ze, zg, lens)
    for b, (n, m) in enumerate(WIDE_LENS):
        one = {k: v[b:b + 1] for k, v in want.items()}
        _check((Vtd[b:b + 1], Ed[b:b + 1], Gd[b:b + 1]), one, f"wide lens {n}x{m}")
    _zero_outside(Ed, Gd, WIDE_LENS, "wide lens")
    assert _bits(Vtd)[-1] == 0 and float(np.abs(want["Ed"][1]).max()) > 0.05


@pytest.mark.parametrize("family,n,m,k", [("floor", 130, 150, adj.B), ("islands", 513, 2048, 1)])
def test_two_calls_give_the_same_bits(family, n, m, k):
    args = adj.case(family, n, m, k)
    first, second = _run(*args), _run(*args)
    for x, y in zip(first, second):
        assert np.array_equal(_bits(x), _bits(y))


# ---- the C entries with raw pointers ----
PAD = 4096                                      # floats in front of and behind every tensor
POISON = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)


def _raw_pair(state, Vt, ze_ptr, zg_ptr, shape, lp, state_d=None):
    """the two adjoint entries with raw pointers; state_d, Ed and Gd start as 0xFF bytes (NaN) -> (Vtd, Ed, Gd, state_d) tensors"""
    lib = _engine().lib
    B, N, M = shape
    stream = torch.cuda.current_stream().cuda_stream
    nan = lambda n: torch.empty(n * 4, dtype=torch.uint8, device=DEV).fill_(0xFF).view(torch.float32)
    if state_d is None:
        state_d = nan(lib.sdp_soft_local_adjoint_state_bytes(B, N, M) // 4)
    Vtd, Ed, Gd = nan(B), nan(B * N * M), nan(B * N * M)
    assert torch.isnan(Ed).all() and torch.isnan(state_d).all()
    et = torch.ones(B, device=DEV)
    assert lib.sdp_soft_local_adjoint_forward_f32(state.data_ptr(), Vt.data_ptr(), ze_ptr, zg_ptr, state_d.data_ptr(), Vtd.data_ptr(),
                                                  B, N, M, lp, 0, 0, stream) == 0
    assert lib.sdp_soft_local_adjoint_backward_f32(state.data_ptr(), state_d.data_ptr(), Vt.data_ptr(), Vtd.data_ptr(), et.data_ptr(),
                                                   Ed.data_ptr(), Gd.data_ptr(), B, N, M, lp, 0, 0, stream) == 0
    torch.cuda.synchronize()
    return Vtd, Ed.view(B, N, M), Gd.view(B, N, M), state_d


@pytest.mark.parametrize("with_lens", [False, True], ids=["full", "lens"])
def test_poisoned_buffers(with_lens):
    """the adjoint sweeps read nothing that the sweeps before them did not write, and leave nothing unwritten: both state buffers
    start as 0xFF bytes (NaN), and so do Vtd, Ed and Gd -- no bit of a result changes, and no NaN is left in them"""
    eng = _engine()
    if with_lens:
        th, a, ze, zg, lens = _lens_case()
        ln = _dev(lens)
    else:
        (th, a, ze, zg), ln = adj.case("steep", 65, 33), None
    clean = _run(th, a, ze, zg, None if ln is None else lens)
    t, A, ZE, ZG = _dev(th), _dev(a), _dev(ze), _dev(zg)
    shape = tuple(t.shape)
    nstate = eng.lib.sdp_soft_local_state_bytes(*shape) // 4
    poison = torch.empty(nstate * 4, dtype=torch.uint8, device=DEV).fill_(0xFF).view(torch.float32)
    Vt, state = eng.soft_local_forward(t, A, ln, state_out=poison)
    assert state is poison
    Vtd, Ed, Gd, state_d = _raw_pair(state, Vt, ZE.data_ptr(), ZG.data_ptr(), shape, None if ln is None else ln.data_ptr())
    assert torch.isnan(state).any() and torch.isnan(state_d).any()      # (the ramps of every strip stay unwritten)
    for x, y in zip(clean, (Vtd, Ed, Gd)):
        y = y.cpu().numpy()
        assert np.isfinite(y).all() and np.array_equal(_bits(x), _bits(y))
    # the engine's own buffer argument
    Vtd2, sd2 = eng.soft_local_adjoint_forward(state, Vt, ZE, ZG, shape, ln, state_d_out=state_d.fill_(float("nan")))
    assert sd2 is state_d and np.array_equal(_bits(Vtd2.cpu().numpy()), _bits(clean[0]))


@pytest.mark.parametrize("with_lens", [True, False], ids=["lens", "full"])
def test_what_lies_beside_the_cotangents_takes_no_part(with_lens):
    """ZE and ZG at plane offsets of 0 .. 3 floats (the four-float loads are `packed, aligned(4)` for this), once among zeros and
    once among NaN, +-inf and +-1e30 -- in front, behind and in every pair's padding: the same bits of Vtd, Ed and Gd"""
    eng = _engine()
    th, a, ze, zg = adj.case("floor", 130, 150)
    lens = ((127, 145), (130, 150), (65, 33)) if with_lens else None
    B, N, M = th.shape
    size = B * N * M
    ln = None if lens is None else _dev(np.asarray(lens, np.int32))
    Vt, state = eng.soft_local_forward(_dev(th), _dev(a), ln)
    rng = np.random.RandomState(77)
    runs = []
    for offset in range(4):
        for dirty in (False, True):
            ptrs, keep = [], []
            for src in (ze, zg):
                fill = POISON[rng.randint(0, 5, size + 2 * PAD + 4)] if dirty else np.zeros(size + 2 * PAD + 4, np.float32)
                x = src.copy()
                if lens is not None:
                    for b, (n, m) in enumerate(lens):
                        pad = POISON[rng.randint(0, 5, (N, M))] if dirty else np.zeros((N, M), np.float32)
                        x[b, n:, :] = pad[n:, :]
                        x[b, :, m:] = pad[:, m:]
                fill[PAD + offset:PAD + offset + size] = x.reshape(-1)
                buf = torch.from_numpy(fill).to(DEV)
                keep.append(buf)
                ptrs.append(buf[PAD + offset:].data_ptr())
            assert ptrs[0] % 16 == 4 * offset
            Vtd, Ed, Gd, _ = _raw_pair(state, Vt, ptrs[0], ptrs[1], (B, N, M), None if ln is None else ln.data_ptr())
            runs.append(tuple(_bits(x.cpu().numpy()) for x in (Vtd, Ed, Gd)))
    for k, run in enumerate(runs[1:], 1):
        for x, y, what in zip(runs[0], run, ("Vtd", "Ed", "Gd")):
            assert np.array_equal(x, y), (what, "offset", k // 2, "dirty", k % 2, int((x != y).sum()))
    got = tuple(x.view(np.float32) for x in runs[0])
    _check(got, adj.batch(th, a, ze, zg, lens), "raw pointers")
    _zero_outside(got[1], got[2], lens if lens is not None else [(N, M)] * B, "raw pointers")


@pytest.mark.parametrize("mask", ["-inf", "-1e30"])
def test_masks(mask):
    """A = -inf is a forbidden gap: Gd is exactly +0 there and nothing is NaN; the large finite negatives callers use as masks
    behave the same.  V reaches 272 on these inputs and half an ulp of Vt is 1.5e-5: the case that shows whether the sweeps take
    their normaliser from the records -- with w = exp(V - Vt) on the rounded Vt alone, Ed is 1.0e-4 off."""
    th, a, ze, zg, gone, want = adj.masked_case(mask)
    Vtd, Ed, Gd = _run(th, a, ze, zg)
    assert np.isfinite(Vtd).all() and np.isfinite(Ed).all() and np.isfinite(Gd).all()
    assert not Gd[gone].any()
    _check((Vtd, Ed, Gd), want, f"mask {mask}")


def test_more_pairs_than_cus():
    th, a = ref.family("model", adj.FAMILY_SEED, 300, 8, 8)
    ze, zg = adj.cotangents(adj.COTANGENT_SEED, 300, 8, 8)
    _check(_run(th, a, ze, zg), adj.batch(th, a, ze, zg), "B=300")


# ---- through autograd on the device ----
def test_the_transposed_route_through_the_module():
    """3 x 2100 is swept as 2100 x 3; the gradients of a gradient come back in the caller's coordinates"""
    th, a, ze, zg = adj.case("drift", 3, 2100)
    lens = np.asarray([(3, 2100), (2, 1999), (3, 2100)], np.int32)
    want = adj.batch(th, a, ze, zg, lens)
    t, A = _dev(th).requires_grad_(), _dev(a).requires_grad_()
    c = torch.ones(3, device=DEV, requires_grad=True)             # a weight on Vt: its gradient is Vtd
    gt, ga = torch.autograd.grad((_decoder()(t, A, _dev(lens)) * c).sum(), (t, A), create_graph=True)
    Ed, Gd, Vtd = torch.autograd.grad((gt * _dev(ze)).sum() + (ga * _dev(zg)).sum(), (t, A, c))
    torch.cuda.synchronize()
    assert tuple(Ed.shape) == (3, 3, 2100) and tuple(Gd.shape) == (3, 3, 2100) and tuple(Vtd.shape) == (3,)
    Ed, Gd = Ed.cpu().numpy(), Gd.cpu().numpy()
    _check((Vtd.cpu().numpy(), Ed, Gd), want, "transposed")
    _zero_outside(Ed, Gd, [tuple(x) for x in lens], "transposed")


def _mce_inputs():
    rng = np.random.RandomState(31)
    B, N, M = 3, 9, 12
    th, a = ref.family("model", 31, B, N, M)
    Yt = (rng.rand(B, N, M) < 0.2).astype(np.float32)
    G = (rng.rand(B, N, M) < 0.8).astype(np.float32)
    return th, a, Yt, G, [9, 7, 9], [12, 12, 5]


def test_a_loss_on_the_posterior_matrix_trains_theta_and_A():
    """MatrixCrossEntropy on decode(), and the gradient of a gradient, against the torch float64 restatement differentiated twice"""
    import loss_ref
    from deepblast_amd.losses import MatrixCrossEntropy, decode_loss
    th, a, Yt, G, xl, yl = _mce_inputs()
    value, gt64, ga64 = adj.torch_batch(th, a, lambda E, _: loss_ref.torch_reference("mce", torch.from_numpy(Yt).double(), E, xl, yl,
                                                                                     torch.from_numpy(G)))
    dec = _decoder()
    t, A = _dev(th).requires_grad_(), _dev(a).requires_grad_()
    loss = MatrixCrossEntropy()(_dev(Yt), dec.decode(t, A), xl, yl, _dev(G))
    loss.backward()
    torch.cuda.synchronize()
    scale = max(1.0, float(np.abs(gt64).max()), float(np.abs(ga64).max()))
    errs = {"loss": rel_err(loss.item(), value), "theta": abs_err(t.grad.cpu().numpy(), gt64), "A": abs_err(A.grad.cpu().numpy(), ga64)}
    print("mce on decode()", " ".join(f"{k}={v:.2e}" for k, v in errs.items()), "scale", scale)
    assert errs["loss"] <= TOL and errs["theta"] <= TOL * scale and errs["A"] <= TOL * scale and np.abs(ga64).max() > 1e-3
    # decode_loss: the same composition, the same bits
    t2, A2 = _dev(th).requires_grad_(), _dev(a).requires_grad_()
    value2, E = decode_loss(dec, MatrixCrossEntropy(), t2, A2, _dev(Yt), xl, yl, _dev(G))
    value2.backward()
    assert not E.requires_grad and torch.equal(t2.grad, t.grad) and torch.equal(A2.grad, A.grad)
    # the gradient of a gradient, and the third order
    _, st64, sa64 = adj.torch_batch(th, a, lambda E, _: (E * E).sum())
    t3, A3 = _dev(th).requires_grad_(), _dev(a).requires_grad_()
    gt, _ = torch.autograd.grad(dec(t3, A3).sum(), (t3, A3), create_graph=True)
    st, sa = torch.autograd.grad((gt * gt).sum(), (t3, A3), create_graph=True)
    scale = max(1.0, float(np.abs(st64).max()), float(np.abs(sa64).max()))
    errs = {"theta": abs_err(st.detach().cpu().numpy(), st64), "A": abs_err(sa.detach().cpu().numpy(), sa64)}
    print("(gt * gt).sum()", " ".join(f"{k}={v:.2e}" for k, v in errs.items()), "scale", scale)
    assert errs["theta"] <= TOL * scale and errs["A"] <= TOL * scale
    with pytest.raises(NotImplementedError, match="third order.*is not built"):
        st.sum().backward()
