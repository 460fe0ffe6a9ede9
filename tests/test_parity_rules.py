"""CPU: the parity rules themselves (tests/parity.py) -- the second-order rule on synthetic results, and the float64 lengths
oracle the rule falls back on."""
import numpy as np
import pytest

import datagen
import parity


def _case(seed, ed_scale=1.0):
    """a float64 'truth' (ref64) for Ed (2, 30, 40) and Vtd (2,); the fp32 reference and the engine start equal to it"""
    ed = (ed_scale * datagen.normal(seed, (2, 30, 40))).astype(np.float64)
    vtd = np.array([3.5, -120.0])
    ref64 = {"Ed": ed, "Vtd": vtd}
    return {k: v.copy() for k, v in ref64.items()}, {k: v.copy() for k, v in ref64.items()}, ref64


def _never():
    raise AssertionError("the float64 reference was run for a case that passes on the fp32 one")


def test_second_order_rule_passes_without_the_float64_reference():
    got, ref32, _ = _case(1)
    got["Ed"][0, 3, 4] += 9e-5
    got["Vtd"][1] *= 1 + 9e-5
    rec = parity.check_second_order(got, ref32, _never, "pass")
    assert rec["status"] == "pass" and rec["Ed"] == pytest.approx(9e-5) and rec["Vtd"] == pytest.approx(9e-5)


def test_second_order_rule_exempts_where_the_fp32_reference_is_the_noisy_one():
    got, ref32, ref64 = _case(2, ed_scale=3.0)
    ref32["Ed"][1, 20, 7] += 1.6e-4          # the fp32 reference's own rounding noise ...
    ref32["Vtd"][0] *= 1 + 2e-4
    got["Ed"][1, 20, 7] += 1.2e-5            # ... the engine on the float64 answer
    calls = []
    rec = parity.check_second_order(got, ref32, lambda: calls.append(1) or ref64, "exempt")
    assert calls == [1] and rec["status"] == "exempt"
    assert rec["Ed"] == pytest.approx(1.48e-4) and rec["Ed64"] == pytest.approx(1.2e-5) and rec["Vtd64"] == 0.0
    assert rec["noise_Ed"] == pytest.approx(1.6e-4) and rec["noise_Vtd"] == pytest.approx(2e-4)


def test_second_order_rule_rejects_what_the_scaled_figure_let_through():
    """plain error 3e-4 where max|Ed_ref| = 9: the scaled figure (3.3e-5) passes, the plain rule must not -- the engine is 3e-4
    from the float64 answer too, so there is no exemption"""
    got, ref32, ref64 = _case(3)
    for r in (got, ref32, ref64):
        r["Ed"][0, 0, 0] = 9.0
    got["Ed"][1, 11, 22] += 3e-4
    assert parity.abs_err(got["Ed"], ref32["Ed"], scale=True) <= parity.TOL   # the old rule
    with pytest.raises(AssertionError) as ex:
        parity.check_second_order(got, ref32, lambda: ref64, "scaled-only")
    msg = str(ex.value)
    assert "engine vs fp32 reference Ed 3.000e-04" in msg and "engine vs float64 Ed 3.000e-04" in msg
    assert "fp32 reference vs float64 Ed 0.000e+00" in msg


def test_second_order_rule_fails_an_exemption_that_is_not_on_float64():
    # over the bound on the fp32 reference, closer to float64 -- but not within F64_TOL of it
    got, ref32, ref64 = _case(4)
    ref32["Ed"][0, 1, 1] += 8e-5
    got["Ed"][0, 1, 1] -= 3e-5
    with pytest.raises(AssertionError):
        parity.check_second_order(got, ref32, lambda: ref64, "Ed")
    # Vtd alone
    got, ref32, ref64 = _case(5)
    got["Vtd"][1] *= 1 + 1.5e-4
    with pytest.raises(AssertionError):
        parity.check_second_order(got, ref32, lambda: ref64, "Vtd")
    # NaN anywhere in the engine's Ed
    got, ref32, ref64 = _case(6)
    got["Ed"][1, 29, 39] = np.nan
    with pytest.raises(AssertionError):
        parity.check_second_order(got, ref32, lambda: ref64, "NaN")


def test_second_order_rule_without_vtd():
    got, ref32, ref64 = _case(7)
    del got["Vtd"], ref32["Vtd"], ref64["Vtd"]
    assert parity.check_second_order(got, ref32, _never)["status"] == "pass"
    ref32["Ed"][0, 2, 2] += 2e-4
    assert parity.check_second_order(got, ref32, lambda: ref64)["status"] == "exempt"


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_oracle_lens_keeps_float64(variant):
    """float64 in -> float64 out, each pair what a float64 oracle_all call on its slice gives (bit for bit), zero outside"""
    B, N, M = 4, 23, 31
    theta, A = datagen.theta_A(515, B, N, M, dtype=np.float64)
    theta *= 8.0
    Z = datagen.normal(516, (B, N, M), dtype=np.float64)
    Et = np.array([1.0, 0.5, -2.0, 3.0])
    lens = np.array([[23, 31], [1, 1], [7, 30], [22, 2]], np.int32)
    out = parity.oracle_lens(theta, A, Et, Z, variant, lens, threads=2)
    assert all(v.dtype == np.float64 for v in out.values())
    for b in range(B):
        n, m = lens[b]
        r = parity.oracle_all(np.ascontiguousarray(theta[b:b + 1, :n, :m]), np.ascontiguousarray(A[b:b + 1, :n, :m]), Et[b:b + 1],
                              np.ascontiguousarray(Z[b:b + 1, :n, :m]), variant, omp=False)
        assert r["Ed"].dtype == np.float64
        for k in ("Vt", "Vtd"):
            assert out[k][b] == r[k][0], (b, k)
        for k in ("E", "Ed"):
            assert np.array_equal(out[k][b, :n, :m], r[k][0]), (b, k)
            assert not out[k][b, n:, :].any() and not out[k][b, :, m:].any(), (b, k)
    # ... and parity.oracle_f64 promotes fp32 inputs to the same run
    t32, a32, z32 = theta.astype(np.float32), A.astype(np.float32), Z.astype(np.float32)
    o64 = parity.oracle_f64(t32, a32, Et.astype(np.float32), z32, variant, lens=lens)
    ref = parity.oracle_lens(t32.astype(np.float64), a32.astype(np.float64), Et, z32.astype(np.float64), variant, lens)
    assert all(np.array_equal(o64[k], ref[k]) for k in ref)


def test_second_order_rule_named_bounds_of_their_own():
    got, ref32, ref64 = _case(8)
    ref32["Vtd"][0] *= 1 + 2e-4
    got["Vtd"][0] *= 1 + 3e-5             # over F64_TOL, inside the named cases' own bound for Vtd
    with pytest.raises(AssertionError):
        parity.check_second_order(got, ref32, lambda: ref64)
    rec = parity.check_second_order(got, ref32, lambda: ref64, vtd_f64_tol=parity.F64_TOL_VTD_SUM)
    assert rec["status"] == "exempt" and rec["Vtd64"] == pytest.approx(3e-5)
    with pytest.raises(AssertionError):   # never above TOL
        parity.check_second_order(got, ref32, lambda: ref64, vtd_f64_tol=2 * parity.TOL)
