"""A stand-in engine for the affine-gap soft global operator's second order, from tests/affine_global_adjoint_ref.py -- TESTS ONLY
(tests/test_affine_global_adjoint.py).  It extends the first order's stand-in (tests/affine_global_engine.py)."""
import numpy as np
import torch

import affine_global_adjoint_ref as adj
from affine_global_engine import AffineGlobalOracleEngine


class AffineGlobalAdjointOracleEngine(AffineGlobalOracleEngine):
    """Results are the float64 definition's (the loops over cells), rounded to fp32.  The adjoint calls are logged as
    ("adjoint_forward", shape, which cotangents were given) and ("adjoint_backward", shape, want_GO, want_GX)."""

    name = "affine-global-adjoint-oracle"

    def affine_global_adjoint_forward(self, state, ZE, ZGO, ZGX, shape, lens=None, state_d_out=None):
        th, o, x, ln = state._inputs
        self.calls.append(("adjoint_forward", tuple(shape), tuple(z is not None for z in (ZE, ZGO, ZGX))))
        assert tuple(shape) == th.shape and (lens is None) == (ln is None)
        if ZE is None and ZGO is None and ZGX is None:
            raise ValueError("affine_global_adjoint_forward: ZE, ZGO and ZGX are all None")
        z = tuple(None if t is None else self._np(t) for t in (ZE, ZGO, ZGX))
        state_d = torch.zeros(1)
        state_d._cotangents = z
        r = adj.batch(th, o, x, *z, lens=ln, form="loops")          # (Vtd does not depend on Et)
        return torch.from_numpy(r["Vtd"].astype(np.float32)), state_d

    def affine_global_adjoint_backward(self, state, state_d, Vtd, Et, shape, lens=None, want_GO=True, want_GX=True):
        th, o, x, ln = state._inputs
        self.calls.append(("adjoint_backward", tuple(shape), bool(want_GO), bool(want_GX)))
        et = np.broadcast_to(self._np(Et).astype(np.float64).reshape(-1), (th.shape[0],))
        r = adj.batch(th, o, x, *state_d._cotangents, lens=ln, Et=et, form="loops")
        f = lambda k: torch.from_numpy(r[k].astype(np.float32))
        return f("Ed"), (f("GOd") if want_GO else None), (f("GXd") if want_GX else None)
