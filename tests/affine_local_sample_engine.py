"""affine_local_engine.AffineLocalOracleEngine + the two sampling entry points, from tests/affine_local_sample_ref.py on the float64
definition's own records -- TESTS ONLY (tests/test_affine_local_sample.py)."""
import numpy as np
import torch

import affine_local_sample_ref as ref
from affine_local_engine import AffineLocalOracleEngine


class AffineLocalSampleOracleEngine(AffineLocalOracleEngine):
    """The tables are the float64 definition's, rounded to fp32 (still non-decreasing: rounding is monotone), zero outside the
    blocks; the end cells are drawn from the tables HANDED OVER, the planes and the walks on the float64 records.  The lists come
    back RIGHT-aligned, as the kernel leaves them; rows outside a list hold -7, so that a caller that reads them is caught."""

    def __init__(self, cols=2048):
        super().__init__(cols)
        self.sample_calls = []

    def _records(self, state, shape):
        th, o, x, lens = state._inputs
        B, N, M = shape
        assert th.shape == tuple(shape)
        out = []
        for b, (n, m) in enumerate(ref.clamp_lens(lens, B, N, M)):
            if n < 1 or m < 1:
                out.append((0.0, np.zeros((0, 0, 3)), np.zeros((0, 0, 3, 3))))
                continue
            out.append(ref._definition(th[b, :n, :m], o[b, :n, :m], x[b, :n, :m]))
        return out

    def affine_local_end_tables(self, state, Vt, shape, lens=None, cdf_out=None, rows_out=None):
        B, N, M = shape
        self.calls.append(("tables", tuple(shape)))
        assert (lens is None) == (state._inputs[3] is None)
        cdf, rows = np.zeros((B, N, M), np.float32), np.zeros((B, N + 1), np.float32)
        for b, (vt, V, _) in enumerate(self._records(state, shape)):
            c, r = ref.tables64(V, vt)
            n, m = V.shape[:2]
            cdf[b, :n, :m], rows[b, :n + 1] = c, r
        return torch.from_numpy(cdf), torch.from_numpy(rows)

    def affine_local_sample_paths(self, state, Vt, cdf, rows, shape, K, lens=None, seed=0, sample0=0, want_states=True,
                                  want_visits=False, want_opens=False, want_extends=False, want_ends=False):
        B, N, M = shape
        self.sample_calls.append((tuple(shape), int(K), int(sample0)))
        assert tuple(Vt.shape) == (B,)
        cdf, rows = cdf.numpy(), rows.numpy()
        got = ref.batch(self._records(state, shape), N, M, int(K), state._inputs[3], seed, sample0,
                        tables=[(cdf[b], rows[b]) for b in range(B)])
        st, cn, on = ref.right_aligned(got, N, M)
        st[~on] = -7
        give = lambda want, a: torch.from_numpy(a) if want else None      # noqa: E731
        return (give(want_states, st), give(want_states, cn), give(want_visits, got["visits"]), give(want_opens, got["opens"]),
                give(want_extends, got["extends"]), give(want_ends, got["ends"]))
