"""A stand-in engine for the soft local operator, from tests/soft_local_ref.py -- TESTS ONLY (tests/test_soft_local.py)."""
import numpy as np
import torch

import soft_local_ref


class SoftLocalOracleEngine:
    """`cols`: the column limit this stand-in reports (lowered by the test of the transposed route).  Results are the float64
    definition's, rounded to fp32; every call is logged with the shape it was handed."""

    name = "soft-local-oracle"

    def __init__(self, cols=2048):
        self.cols = cols
        self.calls = []          # (entry, shape)
        self.state_allocations = 0

    def max_cols(self):
        return self.cols

    @staticmethod
    def _np(t):
        return t.detach().cpu().numpy()

    def _run(self, entry, theta, A, lens):
        th, a = self._np(theta), self._np(A)
        self.calls.append((entry, tuple(th.shape)))
        if th.shape[2] > self.cols:
            raise ValueError("M exceeds sdp_max_cols()")
        if lens is not None:
            lens = np.asarray(lens.cpu() if isinstance(lens, torch.Tensor) else lens)
        return th, a, lens

    def soft_local_forward(self, theta, A, lens=None, state_out=None):
        th, a, lens = self._run("forward", theta, A, lens)
        self.state_allocations += 1
        state = torch.zeros(1)
        state._inputs = (th, a, lens)
        return torch.from_numpy(soft_local_ref.batch(th, a, lens)["Vt"].astype(np.float32)), state

    def soft_local_forward_value(self, theta, A, lens=None):
        th, a, lens = self._run("value", theta, A, lens)
        return torch.from_numpy(soft_local_ref.batch(th, a, lens)["Vt"].astype(np.float32))

    def soft_local_backward(self, state, Vt, Et, shape, lens=None, want_G=True):
        th, a, ln = state._inputs
        self.calls.append(("backward", tuple(shape)))
        assert tuple(shape) == th.shape and (lens is None) == (ln is None)
        et = np.broadcast_to(self._np(Et).astype(np.float64).reshape(-1), (th.shape[0],))
        r = soft_local_ref.batch(th, a, ln, Et=et)
        return torch.from_numpy(r["E"].astype(np.float32)), (torch.from_numpy(r["G"].astype(np.float32)) if want_G else None)
