"""Shared parity helpers: run the HIP engine and the CPU oracle on the same inputs.

Tolerances (BASELINE.json north_star "<= 1e-4 fp32"):
  E, Ed : max-abs <= 1e-4 (E in [0,1]); Ed scaled by max(1, max|Ed_ref|)
  Vt,Vtd: |d| <= 1e-4 * max(1, |ref|)   (fp32 cannot hold Vt ~ 1000 to 1e-4 absolute)
Second order (check_second_order): plain max-abs Ed and Vtd within TOL of the fp32 reference, or else -- the exemption, where
the fp32 reference's own roundings are the noise -- within F64_TOL of the reference run in float64.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle  # noqa: E402  (test infrastructure)

TOL = 1e-4
# engine against the reference run in float64 (first screen: <= 1.4e-5 on the corners measured there; README: <= 2e-5)
F64_TOL = 2e-5
# Two quantities held to float64 by bounds of their own ("Against float64"), in the named long / steep cases:
# Vtd = <Z, E> sums the exact state's per-cell error of E (<= 7e-6) over the whole pair, where |Vtd| may be < 1 (measured 3.1e-5
# and 3.5e-5); plain Ed on pairs of ~4000 steps with max|Ed| ~ 40 (measured 7.3e-5; scaled, 1.7e-6, it is within F64_TOL)
F64_TOL_VTD_SUM = 5e-5
F64_TOL_ED_LONG = TOL


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))) if ref.size else 0.0


def abs_err(got, ref, scale=False):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not ref.size:
        return 0.0
    d = float(np.max(np.abs(got - ref)))
    if scale:
        d /= max(1.0, float(np.max(np.abs(ref))))
    return d


def oracle_all(theta, A, Et, Z, variant, ZA=None, omp=True):
    """Reference-semantics results for one padded batch (no lengths)."""
    Vt, E, Q, Efull = oracle.fwd_bwd(theta, A, Et, variant, omp=omp)
    out = {"Vt": Vt, "E": E}
    if Z is not None:
        Ed, Vtd, _ = oracle.double_backward(Q, Efull, Z, ZA, omp=omp)
        out["Ed"], out["Vtd"] = Ed, Vtd
    return out


def oracle_lens(theta, A, Et, Z, variant, lens, threads=1):
    """Lengths-aware semantics = per-item sliced calls (deepblast/alignment.py:165-170).  `threads` > 1 runs the
    items on a thread pool (the oracle is a C call that releases the GIL): whole config-sized batches in seconds.
    The oracle runs in theta's dtype (float32 or float64) and the outputs keep it."""
    B, N, M = theta.shape
    dt = np.dtype(theta.dtype)
    out = {"Vt": np.zeros(B, dt), "E": np.zeros((B, N, M), dt)}
    if Z is not None:
        out["Ed"] = np.zeros((B, N, M), dt)
        out["Vtd"] = np.zeros(B, dt)

    def one(b):
        n, m = int(lens[b, 0]), int(lens[b, 1])
        r = oracle_all(np.ascontiguousarray(theta[b:b + 1, :n, :m]), np.ascontiguousarray(A[b:b + 1, :n, :m]),
                       None if Et is None else Et[b:b + 1],
                       None if Z is None else np.ascontiguousarray(Z[b:b + 1, :n, :m]), variant, omp=False)
        out["Vt"][b] = r["Vt"][0]
        out["E"][b, :n, :m] = r["E"][0]
        if Z is not None:
            out["Ed"][b, :n, :m] = r["Ed"][0]
            out["Vtd"][b] = r["Vtd"][0]

    if threads > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, range(B)))
    else:
        for b in range(B):
            one(b)
    return out


def oracle_chunked(theta, A, Et, Z, variant, chunk=32):
    """oracle_all over a large padded batch in chunks of `chunk` pairs (the reference-layout Q of 32 pairs of
    1024 x 1024 is 400 MB in fp32; the OpenMP oracle spreads a chunk over the host's cores)."""
    parts = []
    for lo in range(0, theta.shape[0], chunk):
        sl = slice(lo, lo + chunk)
        parts.append(oracle_all(theta[sl], A[sl], None if Et is None else Et[sl], None if Z is None else Z[sl], variant, omp=True))
    return {k: np.concatenate([p_[k] for p_ in parts]) for k in parts[0]}


def engine_all(theta, A, Et, Z, variant, lens=None, ZA=None, device="cuda"):
    """The four HIP passes through the C ABI (no autograd), numpy in / numpy out."""
    import torch
    from deepblast_amd._engine import get_engine
    eng = get_engine()
    t = torch.from_numpy(np.ascontiguousarray(theta)).to(device)
    a = torch.from_numpy(np.ascontiguousarray(A)).to(device)
    B = t.shape[0]
    et = torch.ones(B, device=device) if Et is None else torch.from_numpy(Et).to(device)
    ln = None if lens is None else torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(device)
    Vt, Q = eng.forward(t, a, variant, ln)
    E = eng.backward(et, Q, tuple(t.shape), variant, ln)
    out = {"Vt": Vt.cpu().numpy(), "E": E.cpu().numpy()}
    if Z is not None:
        z = torch.from_numpy(np.ascontiguousarray(Z)).to(device)
        za = None if ZA is None else torch.from_numpy(np.ascontiguousarray(ZA)).to(device)
        # the training path: one exact (float2) state shared by the backward sweep and the two adjoint sweeps
        Vtx, Qx = eng.forward(t, a, variant, ln, exact_state=True)
        Ex = eng.backward(et, Qx, tuple(t.shape), variant, ln, exact_state=True)
        Vtd, Qd = eng.adjoint_forward(Qx, z, za, variant, ln)
        Ed = eng.adjoint_backward(Ex, Qx, Qd, variant, ln)
        out["Ed"], out["Vtd"] = Ed.cpu().numpy(), Vtd.cpu().numpy()
        out["Ex"], out["Vtx"] = Ex.cpu().numpy(), Vtx.cpu().numpy()
    torch.cuda.synchronize()
    return out


def engine_ref(theta, A, Et, Z, variant, lens=None, ZA=None, device="cuda"):
    """The four sweeps in the REFERENCE's arithmetic (variant | SDP_REF_ROUNDING, csrc/sdp_ref.hip) through the C ABI."""
    import torch
    from deepblast_amd._engine import REF, get_engine
    eng = get_engine()
    t = torch.from_numpy(np.ascontiguousarray(theta)).to(device)
    a = torch.from_numpy(np.ascontiguousarray(A)).to(device)
    B = t.shape[0]
    et = torch.ones(B, device=device) if Et is None else torch.from_numpy(Et).to(device)
    ln = None if lens is None else torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(device)
    Vt, Q = eng.forward(t, a, variant, ln, exact_state=REF)
    E = eng.backward(et, Q, tuple(t.shape), variant, ln, exact_state=REF)
    out = {"Vt": Vt.cpu().numpy(), "E": E.cpu().numpy()}
    if Z is not None:
        z = torch.from_numpy(np.ascontiguousarray(Z)).to(device)
        za = None if ZA is None else torch.from_numpy(np.ascontiguousarray(ZA)).to(device)
        Vtd, Qd = eng.adjoint_forward(Q, z, za, variant, ln, ref=True)
        Ed = eng.adjoint_backward(E, Q, Qd, variant, ln, ref=True)
        out["Ed"], out["Vtd"] = Ed.cpu().numpy(), Vtd.cpu().numpy()
    torch.cuda.synchronize()
    return out


def unscaled(got, ref, key="Ed"):
    """max |got - ref| with no scaling at all (SURVEY 8c states the Ed bound as a plain max-abs)."""
    return abs_err(got[key], ref[key], scale=False)


def compare(got, ref, plain=True):
    """-> dict of errors, already normalised so that each must be <= TOL.

    Second order: SURVEY 8c states the bound as a plain max-abs, and `Ed_plain` holds exactly that.  `plain=False` -- only
    the scaled figure `Ed` (error / max(1, max|Ed_ref|)) -- is for the NAMED steep cases whose Ed reaches 5-30 and whose plain
    error is 1.0-1.7e-4 (first screen: there the fp32 reference's own rounding against its float64 run is of
    that size; tests/test_parity_gpu.py::test_where_the_fp32_reference_is_the_noisy_one)."""
    errs = {"Vt": rel_err(got["Vt"], ref["Vt"]), "E": abs_err(got["E"], ref["E"])}
    if "Ed" in ref:
        errs["Ed"] = abs_err(got["Ed"], ref["Ed"], scale=True)
        if plain:
            errs["Ed_plain"] = abs_err(got["Ed"], ref["Ed"], scale=False)
        errs["Vtd"] = rel_err(got["Vtd"], ref["Vtd"])
    if "Ex" in got:  # backward sweep reading the exact state (training path) against the same reference E
        errs["Ex"] = abs_err(got["Ex"], ref["E"])
        errs["Vtx"] = rel_err(got["Vtx"], ref["Vt"])
    return errs


def f64(x):
    """x promoted to float64 (exact), None stays None: the inputs of a float64 oracle run."""
    return None if x is None else np.asarray(x).astype(np.float64)


def oracle_f64(theta, A, Et, Z, variant, lens=None, ZA=None, threads=1):
    """The reference in float64 on the same (fp32) inputs: oracle_lens with per-pair lengths, oracle_all without."""
    if lens is not None:
        assert ZA is None, "oracle_lens has no ZA"
        return oracle_lens(f64(theta), f64(A), f64(Et), f64(Z), variant, lens, threads=threads)
    return oracle_all(f64(theta), f64(A), f64(Et), f64(Z), variant, ZA=f64(ZA), omp=threads > 1)


def check_second_order(got, ref32, ref64_fn, what="", ed_f64_tol=F64_TOL, vtd_f64_tol=F64_TOL):
    """The one rule for second-order results (Ed as a PLAIN max-abs).

    Pass: plain max|Ed - Ed_ref| <= TOL and Vtd (rel_err) <= TOL against the fp32 reference `ref32`.
    Otherwise the exemption, checked and not assumed: `ref64_fn()` (called only then) gives the reference run in float64 on the
    same inputs, and the engine must be within F64_TOL of it on plain Ed and on Vtd -- which by the triangle inequality means
    the fp32 reference itself is more than TOL - F64_TOL from float64 there.  Anything else fails (AssertionError naming all
    three distances: engine vs fp32, engine vs float64, fp32 vs float64).  `ed_f64_tol` / `vtd_f64_tol`: the named cases' own
    bounds against float64 (F64_TOL_ED_LONG, F64_TOL_VTD_SUM; never above TOL).
    -> record: {"status": "pass" | "exempt", "Ed": plain vs fp32, "Vtd": vs fp32, and for an exemption "Ed64", "Vtd64" (engine
    vs float64), "noise_Ed", "noise_Vtd" (fp32 reference vs float64)}."""
    has_vtd = "Vtd" in got   # (a caller with no Vtd to compare -- a loss gradient -- leaves it out of all three dicts)
    assert ed_f64_tol <= TOL and vtd_f64_tol <= TOL
    ed, vtd = abs_err(got["Ed"], ref32["Ed"]), rel_err(got["Vtd"], ref32["Vtd"]) if has_vtd else 0.0
    rec = {"status": "pass", "Ed": ed, "Vtd": vtd}
    if np.isfinite(ed) and np.isfinite(vtd) and ed <= TOL and vtd <= TOL:
        return rec
    ref64 = ref64_fn()
    rec.update(status="exempt", Ed64=abs_err(got["Ed"], ref64["Ed"]), Vtd64=rel_err(got["Vtd"], ref64["Vtd"]) if has_vtd else 0.0,
               noise_Ed=abs_err(ref32["Ed"], ref64["Ed"]), noise_Vtd=rel_err(ref32["Vtd"], ref64["Vtd"]) if has_vtd else 0.0)
    ok = all(np.isfinite(rec[k]) for k in ("Ed64", "Vtd64")) and rec["Ed64"] <= ed_f64_tol and rec["Vtd64"] <= vtd_f64_tol
    assert ok, (f"{what} second order: engine vs fp32 reference Ed {ed:.3e} Vtd {vtd:.3e} (bound {TOL:g}); engine vs float64 "
                f"Ed {rec['Ed64']:.3e} Vtd {rec['Vtd64']:.3e} (bounds {ed_f64_tol:g} / {vtd_f64_tol:g}); fp32 reference vs float64 Ed {rec['noise_Ed']:.3e} "
                f"Vtd {rec['noise_Vtd']:.3e}; max|Ed_ref| = {float(np.max(np.abs(ref32['Ed']))) if np.size(ref32['Ed']) else 0.0:.2f}")
    return rec
