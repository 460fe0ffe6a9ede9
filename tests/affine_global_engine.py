"""A stand-in engine for the affine-gap soft global operator, from tests/affine_global_ref.py -- TESTS ONLY
(tests/test_affine_global.py)."""
import numpy as np
import torch

import affine_global_ref


class AffineGlobalOracleEngine:
    """`cols`: the column limit this stand-in reports (lowered by the test of the transposed route).  Results are the float64
    definition's, rounded to fp32; every call is logged with the shape it was handed."""

    name = "affine-global-oracle"

    def __init__(self, cols=2048):
        self.cols = cols
        self.calls = []          # (entry, shape) -- the backward entry: (entry, shape, want_GO, want_GX)
        self.state_allocations = 0

    def max_cols(self):
        return self.cols

    @staticmethod
    def _np(t):
        return t.detach().cpu().numpy()

    def _run(self, entry, theta, gap_open, gap_extend, lens):
        th, o, x = self._np(theta), self._np(gap_open), self._np(gap_extend)
        self.calls.append((entry, tuple(th.shape)))
        if th.shape[2] > self.cols:
            raise ValueError("M exceeds sdp_max_cols()")
        if lens is not None:
            lens = np.asarray(lens.cpu() if isinstance(lens, torch.Tensor) else lens)
        return th, o, x, lens

    def affine_global_forward(self, theta, gap_open, gap_extend, lens=None, state_out=None):
        th, o, x, lens = self._run("forward", theta, gap_open, gap_extend, lens)
        self.state_allocations += 1
        state = torch.zeros(1)
        state._inputs = (th, o, x, lens)
        return torch.from_numpy(affine_global_ref.batch(th, o, x, lens)["Vt"].astype(np.float32)), state

    def affine_global_forward_value(self, theta, gap_open, gap_extend, lens=None):
        th, o, x, lens = self._run("value", theta, gap_open, gap_extend, lens)
        return torch.from_numpy(affine_global_ref.batch(th, o, x, lens)["Vt"].astype(np.float32))

    def affine_global_backward(self, state, Et, shape, lens=None, want_GO=True, want_GX=True):
        th, o, x, ln = state._inputs
        self.calls.append(("backward", tuple(shape), bool(want_GO), bool(want_GX)))
        assert tuple(shape) == th.shape and (lens is None) == (ln is None)
        et = np.broadcast_to(self._np(Et).astype(np.float64).reshape(-1), (th.shape[0],))
        r = affine_global_ref.batch(th, o, x, ln, Et=et)
        f = lambda k: torch.from_numpy(r[k].astype(np.float32))
        return f("E"), (f("GO") if want_GO else None), (f("GX") if want_GX else None)
