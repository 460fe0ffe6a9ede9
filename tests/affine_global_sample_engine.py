"""affine_global_engine.AffineGlobalOracleEngine + the sampling entry point, from tests/affine_global_sample_ref.py on the float64
definition's own weights -- TESTS ONLY (tests/test_affine_global_sample.py)."""
import numpy as np
import torch

import affine_global_sample_ref as ref
from affine_global_engine import AffineGlobalOracleEngine


class AffineGlobalSampleOracleEngine(AffineGlobalOracleEngine):
    """The end planes and the walks are drawn on the float64 definition's w and q.  The lists come back RIGHT-aligned, as the
    kernel leaves them; rows outside a list hold -7, so that a caller that reads them is caught."""

    def __init__(self, cols=2048):
        super().__init__(cols)
        self.sample_calls = []

    def _records(self, state, shape):
        th, o, x, lens = state._inputs
        B, N, M = shape
        assert th.shape == tuple(shape)
        return [ref._definition(th[b, :n, :m], o[b, :n, :m], x[b, :n, :m])[1:] if n >= 1 and m >= 1 else None
                for b, (n, m) in enumerate(ref.clamp_lens(lens, B, N, M))]

    def affine_global_sample_paths(self, state, shape, K, lens=None, seed=0, sample0=0, want_states=True, want_visits=False,
                                   want_opens=False, want_extends=False, want_ends=False):
        B, N, M = shape
        self.sample_calls.append((tuple(shape), int(K), int(sample0)))
        assert (lens is None) == (state._inputs[3] is None)
        got = ref.batch(self._records(state, shape), N, M, int(K), state._inputs[3], seed, sample0)
        st, cn, on = ref.right_aligned(got, N, M)
        st[~on] = -7
        give = lambda want, a: torch.from_numpy(np.ascontiguousarray(a)) if want else None      # noqa: E731
        return (give(want_states, st), give(want_states, cn), give(want_visits, got["visits"]), give(want_opens, got["opens"]),
                give(want_extends, got["extends"]), give(want_ends, got["ends"]))
