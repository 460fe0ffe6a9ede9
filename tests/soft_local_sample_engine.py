"""soft_local_engine.SoftLocalOracleEngine + the two sampling entry points, from tests/soft_local_sample_ref.py on the float64
definition's own records -- TESTS ONLY (tests/test_soft_local_sample.py)."""
import numpy as np
import torch

import soft_local_ref
import soft_local_sample_ref as ref
from soft_local_engine import SoftLocalOracleEngine


class SoftLocalSampleOracleEngine(SoftLocalOracleEngine):
    """The tables are the float64 definition's, rounded to fp32 (still non-decreasing: rounding is monotone), zero outside the
    blocks; the end cells are drawn from the tables HANDED OVER, the walks run on the float64 records.  The lists come back
    RIGHT-aligned, as the kernel leaves them; rows outside a list hold -7, so that a caller that reads them is caught."""

    def __init__(self, cols=2048):
        super().__init__(cols)
        self.sample_calls = []

    def _records(self, state, shape):
        th, a, lens = state._inputs
        B, N, M = shape
        assert th.shape == tuple(shape)
        out = []
        for b, (n, m) in enumerate(ref.clamp_lens(lens, B, N, M)):
            if n < 1 or m < 1:
                out.append((n, m, 0.0, np.zeros((0, 0)), np.zeros((0, 0, 3))))
                continue
            Vt, V, q = soft_local_ref.forward(th[b:b + 1, :n, :m], a[b:b + 1, :n, :m])
            out.append((n, m, Vt[0], V[0, 1:-1, 1:-1], np.ascontiguousarray(q[0, 1:-1, 1:-1])))
        return out

    def soft_local_end_tables(self, state, Vt, shape, lens=None, cdf_out=None, rows_out=None):
        B, N, M = shape
        self.calls.append(("tables", tuple(shape)))
        assert (lens is None) == (state._inputs[2] is None)
        cdf, rows = np.zeros((B, N, M), np.float32), np.zeros((B, N + 1), np.float32)
        for b, (n, m, vt, V, _) in enumerate(self._records(state, shape)):
            c, r = ref.tables64(V, vt)
            cdf[b, :n, :m], rows[b, :n + 1] = c, r
        return torch.from_numpy(cdf), torch.from_numpy(rows)

    def soft_local_sample_paths(self, state, cdf, rows, shape, K, lens=None, seed=0, sample0=0, want_states=True, want_visits=False,
                                want_ends=False):
        B, N, M = shape
        self.sample_calls.append((tuple(shape), int(K), int(sample0)))
        recs = self._records(state, shape)
        cdf, rows = cdf.numpy(), rows.numpy()
        got = ref.batch([r[4] for r in recs], N, M, int(K), state._inputs[2], seed, sample0,
                        tables=[(cdf[b], rows[b]) for b in range(B)])
        st, cn, on = ref.right_aligned(got, N, M)
        st[~on] = -7
        return (torch.from_numpy(st) if want_states else None, torch.from_numpy(cn) if want_states else None,
                torch.from_numpy(got["visits"]) if want_visits else None, torch.from_numpy(got["ends"]) if want_ends else None)
