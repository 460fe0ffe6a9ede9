"""A stand-in engine for the sparsemax operator, from tests/sparsemax_ref.py -- TESTS ONLY (tests/test_sparsemax.py)."""
import numpy as np
import torch

import sparsemax_ref


class SparsemaxOracleEngine:
    """`cols`: the column limit this stand-in reports (lowered by the test of the transposed route).  Results are the float64
    definition's, rounded to fp32; every call is logged with the shape and the variant it was handed."""

    name = "sparsemax-oracle"

    def __init__(self, cols=2048):
        self.cols = cols
        self.calls = []          # (entry, shape, variant)
        self.state_allocations = 0

    def max_cols(self):
        return self.cols

    @staticmethod
    def _np(t):
        return t.detach().cpu().numpy()

    def _run(self, entry, theta, A, variant, lens):
        th, a = self._np(theta), self._np(A)
        self.calls.append((entry, tuple(th.shape), variant))
        if th.shape[2] > self.cols:
            raise ValueError("M exceeds sdp_max_cols()")
        if lens is not None:
            lens = np.asarray(lens.cpu() if isinstance(lens, torch.Tensor) else lens)
        return th, a, lens

    def sparsemax_forward(self, theta, A, variant, lens=None, state_out=None):
        th, a, lens = self._run("forward", theta, A, variant, lens)
        self.state_allocations += 1
        state = torch.zeros(1)
        state._inputs = (th, a, variant, lens)
        return torch.from_numpy(sparsemax_ref.batch(th, a, variant, lens)["Vt"].astype(np.float32)), state

    def sparsemax_forward_value(self, theta, A, variant, lens=None):
        th, a, lens = self._run("value", theta, A, variant, lens)
        return torch.from_numpy(sparsemax_ref.batch(th, a, variant, lens)["Vt"].astype(np.float32))

    def sparsemax_backward(self, state, Vt, Et, shape, variant, lens=None, want_G=True):
        th, a, v, ln = state._inputs
        self.calls.append(("backward", tuple(shape), variant))
        assert tuple(shape) == th.shape and (lens is None) == (ln is None) and v == variant
        et = np.broadcast_to(self._np(Et).astype(np.float64).reshape(-1), (th.shape[0],))
        r = sparsemax_ref.batch(th, a, variant, ln, Et=et)
        return torch.from_numpy(r["E"].astype(np.float32)), (torch.from_numpy(r["G"].astype(np.float32)) if want_G else None)
