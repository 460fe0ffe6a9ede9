"""fake_engine.OracleEngine + the sampling entry point, from tests/sample_ref.py on the oracle's own Q -- TESTS ONLY
(tests/test_sample.py)."""
import numpy as np
import torch

import sample_ref
from fake_engine import OracleEngine


class SampleOracleEngine(OracleEngine):
    """`cols`: the column limit this stand-in reports (lowered by the test of the transposed route).  The lists come back
    RIGHT-aligned, as the kernel leaves them; rows outside a list hold -7, so that a caller that reads them is caught."""

    def __init__(self, cols=2048):
        self.cols = cols
        self.sample_calls = []

    def max_cols(self):
        return self.cols

    def forward(self, theta, A, variant, lens=None, exact_state=False):
        if theta.shape[2] > self.cols:
            raise ValueError("M exceeds sdp_max_cols()")
        return super().forward(theta, A, variant, lens, exact_state)

    def sample_paths(self, state, shape, variant, K, lens=None, seed=0, sample0=0, exact_state=False, transposed=False,
                     want_states=True, want_visits=False):
        B, N, M = shape
        self.sample_calls.append((tuple(shape), bool(transposed), int(K), int(sample0)))
        Qs = [sample_ref.inner(q) for q in state._oracle_Q]
        if lens is not None:
            lens = np.asarray(lens.cpu() if isinstance(lens, torch.Tensor) else lens)
        ref = sample_ref.batch(Qs, N, M, K, variant, lens, seed, sample0, transposed)
        st, cn, on = sample_ref.right_aligned(ref, N, M)
        st[~on] = -7
        return (torch.from_numpy(st) if want_states else None, torch.from_numpy(cn) if want_states else None,
                torch.from_numpy(ref["visits"]) if want_visits else None)
