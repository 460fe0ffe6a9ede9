"""A numpy restatement of the reference's alignment scoring (deepblast/score.py, dataset/utils.py:states2edges), held to
tests/golden/g15_score.npz by test_align_stats.py and used by the GPU tests for everything the fixture does not hold.

Contract, per pair:
  states    TM-align characters through tmstate_f ('1' x = 0, '2' y = 2, anything else m = 1); int states as they are.
  edges     edge 0 = (0, 0); edge k = edge k-1 + step of state k alone (x (1, 0), m (1, 1), y (0, 1)).
  no_gaps   keep edge k only where state k is m (filter_gaps); an empty side raises ValueError, the prediction first.
  roc       tp = |T & P|, fp = |P - T|, fn = |T - P|, then tp / |T|, tp / (tp + fp), fn / (fn + tp), fp / (fp + tp) as
            Python float divisions.
  identity  the predicted edges shifted by (query_offset, hit_offset) before filtering; for each width w in order the
            predicted SET grows by its own snapshot moved by +-k along the diagonal, k < w (roc_edges_kernel_identity
            extends the caller's list in place, so widths accumulate); perc_id = |T & set| / |T|.
It does not read the reference checkout."""
import numpy as np

X, M, Y = 0, 1, 2


def states_of(a):
    """str / bytes (tmstate_f) or int states -> int64 array of 0 / 1 / 2."""
    if isinstance(a, str):
        a = a.encode("ascii")
    if isinstance(a, (bytes, bytearray)):
        c = np.frombuffer(bytes(a), dtype=np.uint8)
        return np.where(c == ord("1"), X, np.where(c == ord("2"), Y, M)).astype(np.int64)
    return np.asarray(a, dtype=np.int64).reshape(-1)


def edges(st):
    """(L, 2) int64: states2edges."""
    st = states_of(st)
    dr = (st != Y).astype(np.int64)
    dc = (st != X).astype(np.int64)
    dr[:1] = dc[:1] = 0
    return np.stack([np.cumsum(dr), np.cumsum(dc)], axis=1)


def _kept(st, e, no_gaps, what):
    st = states_of(st)
    if no_gaps:
        e = e[st == M]
        if not len(e):
            raise ValueError(f"filter_gaps: no match state in the {what}")
    return e


def _key(e):
    return e[:, 0].astype(np.complex128) + 1j * e[:, 1].astype(np.float64)   # exact for |coordinates| < 2^53


def roc(true_st, pred_st, no_gaps=True):
    """alignment_score -> (tp, fp, fn, perc_id, ppv, fnr, fdr) with Python ints and floats; raises as the reference."""
    pe = _kept(pred_st, edges(pred_st), no_gaps, "prediction")
    te = _kept(true_st, edges(true_st), no_gaps, "truth")
    tp = int(np.isin(_key(te), _key(pe)).sum())
    fp, fn = len(pe) - tp, len(te) - tp
    return tp, fp, fn, tp / len(te), tp / (tp + fp), fn / (fn + tp), fp / (fp + tp)


def identity(true_st, pred_st, widths, query_offset=0, hit_offset=0, no_gaps=True):
    """alignment_score_kernel -> list of floats, one per width (the accumulation included)."""
    pe = edges(pred_st) + np.array([query_offset, hit_offset], dtype=np.int64)
    pe = _kept(pred_st, pe, no_gaps, "prediction")
    te = _kept(true_st, edges(true_st), no_gaps, "truth")
    tk = _key(te)
    out = []
    for w in widths:
        snap = pe
        pe = np.unique(np.concatenate([snap] + [snap + s * k for k in range(max(int(w), 0)) for s in (1, -1)]), axis=0)
        out.append(int(np.isin(tk, _key(pe)).sum()) / len(te))
    return out


def half_widths(widths):
    """S_i = sum over t <= i of max(w_t - 1, 0): the diagonal reach of width i after the accumulation."""
    return np.cumsum([max(int(w) - 1, 0) for w in widths]).astype(np.int64)


def raised(fn, *args, **kw):
    """(result, None) or (None, exception type)."""
    try:
        return fn(*args, **kw), None
    except (ValueError, IndexError) as e:
        return None, type(e)
