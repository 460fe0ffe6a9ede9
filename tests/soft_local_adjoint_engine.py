"""tests/soft_local_engine.py's stand-in engine plus the two entries of the adjoint pair, from tests/soft_local_adjoint_ref.py --
TESTS ONLY (tests/test_soft_local_adjoint.py)."""
import numpy as np
import torch

import soft_local_adjoint_ref as adj
from soft_local_engine import SoftLocalOracleEngine


class SoftLocalAdjointOracleEngine(SoftLocalOracleEngine):
    """Results are the float64 definition's (the loops over cells), rounded to fp32; every call is logged with its shape."""

    name = "soft-local-adjoint-oracle"

    def soft_local_adjoint_forward(self, state, Vt, ZE, ZG, shape, lens=None, state_d_out=None):
        th, a, ln = state._inputs
        self.calls.append(("adjoint_forward", tuple(shape)))
        assert tuple(shape) == th.shape and (lens is None) == (ln is None) and (ZE is not None or ZG is not None)
        ze, zg = (None if z is None else self._np(z) for z in (ZE, ZG))
        assert all(z is None or z.shape == th.shape for z in (ze, zg))
        state_d = torch.zeros(1)
        state_d._cotangents = (ze, zg)
        r = adj.batch(th, a, ze, zg, ln, wavefront=False)       # (Vtd does not depend on Et)
        return torch.from_numpy(r["Vtd"].astype(np.float32)), state_d

    def soft_local_adjoint_backward(self, state, state_d, Vt, Vtd, Et, shape, lens=None, want_G=True):
        th, a, ln = state._inputs
        ze, zg = state_d._cotangents
        self.calls.append(("adjoint_backward", tuple(shape)))
        assert tuple(shape) == th.shape and (lens is None) == (ln is None)
        et = np.broadcast_to(self._np(Et).astype(np.float64).reshape(-1), (th.shape[0],))
        r = adj.batch(th, a, ze, zg, ln, Et=et, wavefront=False)
        return torch.from_numpy(r["Ed"].astype(np.float32)), (torch.from_numpy(r["Gd"].astype(np.float32)) if want_G else None)
