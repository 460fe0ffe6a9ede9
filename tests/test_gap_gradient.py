"""CPU: the opt-in true gap-score gradients (Decoder(..., gap_gradient=True)) -- the autograd wiring on an oracle-backed stand-in
engine (tests/gap_engine.py), the hard-max G on the stand-in of tests/hard_engine.py, and the argument checks of the four
sdp_gap_gradient* entries.  The kernels themselves: tests/test_gap_gradient_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import datagen
import gap_ref
import hard_ref
from gap_engine import GapOracleEngine
from hard_engine import HardOracleEngine

LENS = [[5, 7], [3, 4], [1, 6]]


def _decoders():
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder
    return NeedlemanWunschDecoder, SmithWatermanDecoder


def _t(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.requires_grad_() if grad else t


@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = GapOracleEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


def test_decoder_takes_gap_gradient():
    """the red test: the keyword was a TypeError before the feature existed"""
    NW, SW = _decoders()
    assert NW("softmax", gap_gradient=True).gap_gradient is True and SW("softmax", gap_gradient=True).gap_gradient is True
    assert NW("softmax").gap_gradient is False and NW("hardmax", gap_gradient=True).gap_gradient is True


def _close(got, want, what):
    assert got is not None, what
    err = float(np.max(np.abs(got.numpy().astype(np.float64) - want)))
    assert err <= 2e-6 * max(1.0, float(np.max(np.abs(want)))), (what, err)   # the stand-in forms the same fp32 products


@pytest.mark.parametrize("with_lens", [False, True], ids=["padded", "lens"])
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_wiring_first_and_second_order(eng, variant, with_lens):
    B, N, M = 3, 5, 7
    theta, A = datagen.theta_A(11, B, N, M)
    Z, ZG = datagen.normal(12, (B, N, M)), datagen.normal(13, (B, N, M))
    Et = np.array([1.7, -0.5, 1.0], np.float32)
    lens = LENS if with_lens else None
    tl = None if lens is None else torch.tensor(lens)
    dec = _decoders()[variant]("softmax", gap_gradient=True)

    # first order: A.grad = E (Qx + Qy)
    ref = gap_ref.reference(theta, A, Et, variant, lens, Z, ZG, decoder=True)
    t, a = _t(theta, True), _t(A, True)
    dec(t, a, tl).backward(_t(Et))
    _close(t.grad, ref["E"], "E")
    _close(a.grad, ref["G"], "G")

    # second order through decode(): theta.grad = Ed, A.grad = Ed (Qx + Qy) + E (Qdx + Qdy), with ZG = 0
    ref0 = gap_ref.reference(theta, A, None, variant, lens, Z, None, decoder=True)
    t, a = _t(theta, True), _t(A, True)
    (dec.decode(t, a, tl) * _t(Z)).sum().backward()
    _close(t.grad, ref0["Ed"], "Ed")
    _close(a.grad, ref0["Gd"], "Gd")

    # ... and with a cotangent on G as well: the adjoint pair runs with ZA = ZG
    t, a, et = _t(theta, True), _t(A, True), _t(Et, True)
    E, G = torch.autograd.grad(dec(t, a, tl), (t, a), grad_outputs=et, create_graph=True)
    ((E * _t(Z)).sum() + (G * _t(ZG)).sum()).backward()
    _close(t.grad, ref["Ed"], "Ed | ZG")
    _close(a.grad, ref["Gd"], "Gd | ZG")
    _close(et.grad, ref["Vtd"], "Vtd | ZG")

    # a default decoder beside it keeps the reference's conventions
    plain = _decoders()[variant]("softmax")
    t, a = _t(theta, True), _t(A, True)
    plain(t, a, tl).backward(_t(Et))
    assert np.array_equal(a.grad.numpy(), A)
    t, a = _t(theta, True), _t(A, True)
    (plain.decode(t, a, tl) * _t(Z)).sum().backward()
    assert a.grad is None
    _close(t.grad, gap_ref.reference(theta, A, None, variant, lens, Z, None)["Ed"], "Ed of the default decoder: the reference's pair")


def test_default_decoders_hand_the_functions_the_same_arguments(eng, monkeypatch):
    """gap_gradient=False changes nothing, the argument tuples of Function.apply included ("no trailing argument that has its
    default value"); gap_gradient=True appends itself behind fully spelt-out arguments"""
    from deepblast_amd import nw
    theta, A = datagen.theta_A(14, 2, 4, 4)
    seen = []
    real = nw.NeedlemanWunschFunction.apply
    monkeypatch.setattr(nw.NeedlemanWunschFunction, "apply", staticmethod(lambda *a: (seen.append(a[2:]), real(*a))[1]))
    NW = _decoders()[0]
    lens = torch.tensor([[4, 4], [2, 3]])
    NW("softmax")(_t(theta), _t(A))
    NW("softmax")(_t(theta), _t(A), lens)
    NW("softmax")(_t(theta), _t(A), lens, fill=False)
    NW("softmax").decode(_t(theta, True), _t(A, True))
    assert [len(s) for s in seen] == [1, 2, 4, 3] and seen[0] == ("softmax",) and seen[2][2:] == (False, True) and seen[3][1:] == (None, True)
    seen.clear()
    NW("softmax", gap_gradient=True)(_t(theta), _t(A))
    NW("softmax", gap_gradient=True).decode(_t(theta, True), _t(A, True), lens, fill=False)
    assert seen[0] == ("softmax", None, False, False, True) and seen[1][2:] == (True, True, True)


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_hardmax_gap_gradient_is_et_on_the_paths_gap_cells(monkeypatch, variant):
    from deepblast_amd import _engine
    monkeypatch.setattr(_engine, "_ENGINE", HardOracleEngine())
    N, M = 6, 8
    th, a = hard_ref.quarter_scores(3, 4, N, M)
    lens = [[6, 8], [1, 1], [4, 7], [6, 2]]
    Et = np.array([2.5, 1.0, -1.25, 0.5], np.float32)
    ref = hard_ref.batch(th, a, variant, lens, Et=Et)
    want = np.zeros((4, N, M), np.float32)
    for b, cells in enumerate(ref["cells"]):
        for (i, j, k) in cells:
            if k != 1:
                want[b, i, j] = Et[b]
    assert want.any()
    dec = _decoders()[variant]("hardmax", gap_gradient=True)
    t, A = _t(th, True), _t(a, True)
    dec(t, A, torch.tensor(lens)).backward(_t(Et))
    assert np.array_equal(t.grad.numpy().view(np.uint32), ref["E"].view(np.uint32))
    assert np.array_equal(A.grad.numpy().view(np.uint32), want.view(np.uint32))
    # second order: zeros for theta and for A
    t, A = _t(th, True), _t(a, True)
    (dec.decode(t, A, torch.tensor(lens)) * _t(datagen.normal(5, (4, N, M)))).sum().backward()
    assert not t.grad.numpy().any() and A.grad is not None and not A.grad.numpy().any()
    # the default decoder: A itself
    t, A = _t(th, True), _t(a, True)
    _decoders()[variant]("hardmax")(t, A, torch.tensor(lens)).backward(_t(Et))
    assert np.array_equal(A.grad.numpy(), a)


# ---- the C ABI's argument checks need no GPU ----
@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def test_gap_gradient_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    tail = (None, 0, 0, None)
    for first in (lib.sdp_gap_gradient_f32, lib.sdp_gap_gradient_f64):
        for args in ((None, one, one), (one, None, one), (one, one, None)):
            assert first(*args, 1, 1, 1, *tail) == -1
    for second in (lib.sdp_gap_gradient2_f32, lib.sdp_gap_gradient2_f64):
        for k in range(5):
            assert second(*[None if q == k else one for q in range(5)], 1, 1, 1, *tail) == -1
    over = lib.sdp_max_cols() + 1
    for fn, nptr in ((lib.sdp_gap_gradient_f32, 3), (lib.sdp_gap_gradient_f64, 3), (lib.sdp_gap_gradient2_f32, 5), (lib.sdp_gap_gradient2_f64, 5)):
        ptrs = [one] * nptr
        for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
            assert fn(*ptrs, *shape, *tail) == -2, shape
        assert fn(*ptrs, 1, 1, over, *tail) == -3
        assert fn(*ptrs, 1, 1 << 18, 2048, *tail) == -5
        assert fn(*ptrs, 1, 1, 1, None, 2, 0, None) == -4        # neither SDP_NW nor SDP_SW
    # flags: the first-order fp32 entry takes the state's flags and SDP_NO_FILL, the second-order one SDP_REF_ROUNDING only
    for flag in (0x200, 0x800, 0x1000, 0x20000):                 # SDP_ET_BROADCAST, SDP_NO_ZERO_SKIP, SDP_WAVES(1), SDP_HARD_TIES_YMX
        assert lib.sdp_gap_gradient_f32(one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
    for flag in (0x100, 0x200, 0x800, 0x1000, 0x10000, 0x20000):
        assert lib.sdp_gap_gradient2_f32(one, one, one, one, one, 1, 1, 1, None, 1 | flag, 0, None) == -4, hex(flag)
    for flag in (0x100, 0x400, 0x10000, 0x1000):
        assert lib.sdp_gap_gradient_f64(one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert lib.sdp_gap_gradient2_f64(one, one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
    assert b"sdp_gap_gradient" in lib.sdp_last_error_string()
    assert [lib.sdp_kernel_name(k) for k in range(100, 107)] == [b"sdp_gap_kernel", b"sdp_gap2_kernel", b"sdp_gap_rows_kernel", b"sdp_gap2_rows_kernel",
                                                                 b"sdp_gap_rows_f64_kernel", b"sdp_gap2_rows_f64_kernel", None]
    assert lib.sdp_version() == 106
