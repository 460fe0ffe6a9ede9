"""tests/sparsemax_engine.py's stand-in engine plus the two entries of the adjoint pair, from tests/sparsemax_adjoint_ref.py --
TESTS ONLY (tests/test_sparsemax_adjoint.py)."""
import numpy as np
import torch

import sparsemax_adjoint_ref as adj
from sparsemax_engine import SparsemaxOracleEngine


class SparsemaxAdjointOracleEngine(SparsemaxOracleEngine):
    """Results are the float64 definition's (the loops over cells), rounded to fp32; every call is logged with its shape and variant."""

    name = "sparsemax-adjoint-oracle"

    def sparsemax_adjoint_forward(self, state, ZE, ZG, shape, variant, lens=None, state_d_out=None):
        th, a, v, ln = state._inputs
        self.calls.append(("adjoint_forward", tuple(shape), variant))
        assert tuple(shape) == th.shape and (lens is None) == (ln is None) and v == variant and (ZE is not None or ZG is not None)
        ze, zg = (None if z is None else self._np(z) for z in (ZE, ZG))
        assert all(z is None or z.shape == th.shape for z in (ze, zg))
        state_d = torch.zeros(1)
        state_d._cotangents = (ze, zg)
        r = adj.batch(th, a, ze, zg, variant, ln, wavefront=False)       # (Vtd does not depend on Et)
        return torch.from_numpy(r["Vtd"].astype(np.float32)), state_d

    def sparsemax_adjoint_backward(self, state, state_d, Et, shape, variant, lens=None, want_G=True):
        th, a, v, ln = state._inputs
        ze, zg = state_d._cotangents
        self.calls.append(("adjoint_backward", tuple(shape), variant))
        assert tuple(shape) == th.shape and (lens is None) == (ln is None) and v == variant
        et = np.broadcast_to(self._np(Et).astype(np.float64).reshape(-1), (th.shape[0],))
        r = adj.batch(th, a, ze, zg, variant, ln, Et=et, wavefront=False)
        return torch.from_numpy(r["Ed"].astype(np.float32)), (torch.from_numpy(r["Gd"].astype(np.float32)) if want_G else None)
