"""affine_semiglobal_ref.AffineSemiGlobalOracleEngine + the two sampling entry points, from tests/affine_semiglobal_sample_ref.py on
the float64 definition's own weights -- TESTS ONLY (tests/test_affine_semiglobal_sample.py)."""
import numpy as np
import torch

import affine_semiglobal_sample_ref as ref
from affine_semiglobal_ref import AffineSemiGlobalOracleEngine


class AffineSemiGlobalSampleOracleEngine(AffineSemiGlobalOracleEngine):
    """The end cells, the end planes and the walks are drawn on the float64 definition's w and q.  The lists come back
    RIGHT-aligned, as the kernel leaves them; rows outside a list hold -7 and table entries that are not written -7.0, so that a
    caller that reads them is caught.  Every call is logged with its arguments in the order they were handed over."""

    def __init__(self, cols=2048):
        super().__init__(cols)
        self.table_calls = []        # (shape, free_ends)
        self.sample_calls = []       # (shape, free_ends, K, sample0, seed)

    def _records(self, state, shape):
        th, o, x, lens, free_ends = state._inputs
        B, N, M = shape
        assert th.shape == tuple(shape)
        return [ref.definition(th[b, :n, :m], o[b, :n, :m], x[b, :n, :m], free_ends)[1:] if n >= 1 and m >= 1 else None
                for b, (n, m) in enumerate(ref.clamp_lens(lens, B, N, M))]

    def affine_semiglobal_end_table(self, state, shape, free_ends, lens=None):
        B, N, M = shape
        self.table_calls.append((tuple(shape), free_ends))
        assert (lens is None) == (state._inputs[3] is None) and free_ends == state._inputs[4]
        ecdf = np.full((B, N + M), -7.0, np.float32)
        for b, rec in enumerate(self._records(state, shape)):
            if rec is not None:
                t = ref.table(ref.candidate_weights(rec[0], free_ends))
                ecdf[b, :t.size] = t
        out = torch.from_numpy(ecdf)
        out._state = state
        return out

    def affine_semiglobal_sample_paths(self, state, ecdf, shape, free_ends, K, lens=None, seed=0, sample0=0, want_states=True,
                                       want_visits=False, want_opens=False, want_extends=False, want_ends=False):
        B, N, M = shape
        self.sample_calls.append((tuple(shape), free_ends, int(K), int(sample0), int(seed)))
        assert ecdf._state is state and tuple(ecdf.shape) == (B, N + M)
        assert (lens is None) == (state._inputs[3] is None) and free_ends == state._inputs[4]
        got = ref.batch(self._records(state, shape), N, M, int(K), free_ends, state._inputs[3], seed, sample0)
        st, cn, on = ref.right_aligned(got, N, M)
        st[~on] = -7
        give = lambda want, a: torch.from_numpy(np.ascontiguousarray(a)) if want else None      # noqa: E731
        return (give(want_states, st), give(want_states, cn), give(want_visits, got["visits"]), give(want_opens, got["opens"]),
                give(want_extends, got["extends"]), give(want_ends, got["ends"]))
