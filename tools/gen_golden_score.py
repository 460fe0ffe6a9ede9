#!/usr/bin/env python
"""Golden vectors for deepblast_amd.score (tests/golden/g15_score.npz).

Provenance: runs the REAL reference scoring of flatironinstitute/deepblast -- deepblast/score.py (roc_edges :8-18,
roc_edges_kernel_identity :21-35, filter_gaps :37-41, alignment_score_kernel :44-75, alignment_score :76-97) on top of
the real deepblast/dataset/utils.py (tmstate_f, revstate_f, states2edges) -- and stores the inputs with what it returned
or raised.  utils.py is loaded on its own (deepblast/dataset/__init__.py needs Biopython) with oracle/_shim standing in
for numba and registered as deepblast.dataset.utils, so that score.py's own import finds it.  Needs the reference
checkout (default /root/reference, or $DEEPBLAST_REFERENCE), matplotlib and pandas (score.py imports them).

Sets (each a batch of pairs, true and predicted alignments as uint8 codes):
  strings   TM-align strings: '.', leading / trailing gaps, single states, all-gap strings (raising cases), random ones;
            alignment_score itself.
  ints      int states as the dataset builds them ([m] + ... + [m], and some without): the trainer's composition
            (states2edges -> filter_gaps -> roc_edges on the ints, trainer.py:208-213).
  walk_cpu  predictions = the CPU classes' walks of tests/golden/g8_tracebacks.npz (IndexError cases included), with
            their matrices, so that a test can walk them again; the trainer's composition.
  walk_cuda the same with the GPU classes' walks of tests/golden/g12_tracebacks_cuda.npz.
For every set: alignment_score with no_gaps True and False, and alignment_score_kernel for every width list of WIDTHS
with the set's per-pair offsets (zero, positive and negative), with no_gaps True and False.  Raised: 1 ValueError,
2 IndexError, 0 none (rows of a raising pair are NaN).

    python tools/gen_golden_score.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("DEEPBLAST_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "oracle", "_shim"))
sys.path.insert(1, REF)
_spec = importlib.util.spec_from_file_location("deepblast.dataset.utils", os.path.join(REF, "deepblast", "dataset", "utils.py"))
_u = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_u)
_pkg = types.ModuleType("deepblast.dataset")
_pkg.utils = _u
sys.modules["deepblast.dataset"] = _pkg
sys.modules["deepblast.dataset.utils"] = _u
_spec = importlib.util.spec_from_file_location("deepblast.score", os.path.join(REF, "deepblast", "score.py"))
_s = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_s)

WIDTHS = [[1, 2, 3], [3], [4], [0], [5, 0, 2], [2, 2, 2, 2], [], [1], [9, 1, 6]]
X, M, Y = 0, 1, 2


def _run(fn, *args, **kw):
    try:
        return fn(*args, **kw), 0
    except ValueError:
        return None, 1
    except IndexError:
        return None, 2


def _trainer_stats(true_st, pred_st, no_gaps):
    """trainer.py:208-213 (states2edges -> filter_gaps -> roc_edges on the int states); no_gaps=False skips the filter,
    as alignment_score does."""
    pe = _u.states2edges(pred_st)
    te = _u.states2edges(true_st)
    if no_gaps:
        pe = _s.filter_gaps(pred_st, pe)
        te = _s.filter_gaps(true_st, te)
    return _s.roc_edges(te, pe)


def _string(st):
    return "".join(_u.revstate_f(int(v)) for v in st)


def _random_string(rng, L, p_gap, run, p_dot=0.2):
    out = []
    while len(out) < L:
        if rng.random() < p_gap:
            out += [str(rng.choice(["1", "2"]))] * int(rng.geometric(1.0 / run))
        else:
            out += [":" if rng.random() >= p_dot else "."] * int(rng.integers(1, 6))
    return "".join(out[:L])


def _mutate(rng, s, p):
    """A prediction near `s`: characters replaced with probability p."""
    return "".join(str(rng.choice(["1", "2", ":", "."])) if rng.random() < p else c for c in s)


def _random_states(rng, L, ends=True):
    st = rng.choice([X, M, Y], size=L, p=[0.15, 0.7, 0.15])
    if ends:
        st[0] = st[-1] = M   # dataset.py: [m] + ... + [m]
    return st


def string_set(rng):
    a = _random_string(rng, 120, 0.2, 3.0)
    b = _random_string(rng, 300, 0.1, 10.0)
    pairs = [(":", ":"), (":", "1"), ("1", ":"), ("11112222", "::::"), (":::", "1212"), ("2222", "1111"),
             ("111::.:22", "22:.::11"), (".::1:2:.", "..:::."), ("::.:.::..::", "::.:.::..::"), ("1::::", "2::.."),
             (":" + "2" * 30 + "1" * 20, ":" * 40), (a, a), (a, _mutate(rng, a, 0.1)), (b, _mutate(rng, b, 0.3)),
             (b, _random_string(rng, 280, 0.15, 4.0)), ("." * 7, "." * 7), ("1" + ":" * 5 + "2", "2" + ":" * 5 + "1")]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def int_set(rng):
    t, p = [], []
    for L1, L2, ends in [(600, 600, True), (50, 80, True), (1, 1, True), (2, 3, True), (200, 150, False),
                         (300, 300, True), (17, 400, False), (64, 65, True)]:
        a = _random_states(rng, L1, ends)
        t.append(a)
        p.append(a.copy() if L1 == 300 else _random_states(rng, L2, ends))
    p[-1] = np.concatenate([t[-1][:40], _random_states(rng, 25, True)])
    t.append(np.array([X, Y, X, Y]))          # no match state: filter_gaps raises on the truth
    p.append(np.array([M, M, X, M]))
    return t, p


def walk_set(rng, fixture, key):
    d = np.load(os.path.join(ROOT, "tests", "golden", fixture))
    t, p, grads = [], [], []
    for k in range(int(d["count"])):
        g = d[f"t{k}_grad"]
        walk = d[f"t{k}_{key}"] if key != "states" else d[f"t{k}_states"]
        ok = bool(d[f"t{k}_ok"]) if f"t{k}_ok" in d else True
        N, M_ = g.shape
        t.append(_random_states(rng, int(rng.integers(1, N + M_ + 1)), True))
        p.append(walk[:, 2].astype(np.int64) if ok else None)
        grads.append(g)
    return t, p, grads


def codes(items):
    lens = np.array([len(s) if s is not None else -1 for s in items], dtype=np.int32)
    c = np.zeros((len(items), max(1, int(lens.max()))), dtype=np.uint8)
    for b, s in enumerate(items):
        if s is None:
            continue
        c[b, :len(s)] = np.frombuffer(s.encode(), dtype=np.uint8) if isinstance(s, str) else \
            np.frombuffer(_string(s).encode(), dtype=np.uint8)
    return c, lens


def main():
    rng = np.random.default_rng(1515)
    out = {"provenance": np.array(
        "deepblast/score.py alignment_score / alignment_score_kernel / roc_edges / filter_gaps and dataset/utils.py "
        "states2edges, trainer.py:208-213 composition for int states and walks; run by tools/gen_golden_score.py"),
        "n_widths": np.array(len(WIDTHS))}
    for j, w in enumerate(WIDTHS):
        out[f"widths{j}"] = np.array(w, dtype=np.int64)
    sets = {"strings": string_set(rng) + (None,), "ints": int_set(rng) + (None,),
            "walk_cpu": walk_set(rng, "g8_tracebacks.npz", "states"),
            "walk_cuda": walk_set(rng, "g12_tracebacks_cuda.npz", "nw")}
    for name, (tru, pred, grads) in sets.items():
        B = len(tru)
        is_str = isinstance(tru[0], str)
        tcodes, tlens = codes(tru)
        pcodes, plens = codes(pred)
        out[f"{name}_true_codes"], out[f"{name}_true_lens"] = tcodes, tlens
        out[f"{name}_pred_codes"], out[f"{name}_pred_lens"] = pcodes, plens
        offs = np.stack([rng.integers(-3, 4, B), rng.integers(-3, 4, B)], axis=1).astype(np.int32)
        offs[0] = 0
        out[f"{name}_offsets"] = offs
        if grads is not None:
            for b, g in enumerate(grads):
                out[f"{name}_grad{b}"] = g
        for ng, tag in ((True, "gaps"), (False, "all")):
            stats = np.full((B, 7), np.nan)
            raised = np.zeros(B, dtype=np.int8)
            for b in range(B):
                if pred[b] is None:                 # the walk raised IndexError before any scoring
                    raised[b] = 2
                    continue
                if is_str:
                    r, e = _run(_s.alignment_score, tru[b], pred[b], ng)
                else:
                    r, e = _run(_trainer_stats, tru[b], pred[b], ng)
                    r2, e2 = _run(_s.alignment_score, _string(tru[b]), _string(pred[b]), ng)
                    assert e == e2 and (r == r2 if r is not None else r2 is None)
                raised[b] = e
                if r is not None:
                    assert all(type(v) is int for v in r[:3]) and all(type(v) is float for v in r[3:])
                    stats[b] = r
            out[f"{name}_stats_{tag}"], out[f"{name}_raised_{tag}"] = stats, raised
            for j, w in enumerate(WIDTHS):
                ident = np.full((B, len(w)), np.nan)
                iraised = np.zeros(B, dtype=np.int8)
                for b in range(B):
                    if pred[b] is None:
                        iraised[b] = 2
                        continue
                    ts = tru[b] if is_str else _string(tru[b])
                    ps = pred[b] if is_str else _string(pred[b])
                    r, e = _run(_s.alignment_score_kernel, ts, ps, list(w), int(offs[b, 0]), int(offs[b, 1]), ng)
                    iraised[b] = e
                    if r is not None:
                        ident[b] = r
                out[f"{name}_ident{j}_{tag}"], out[f"{name}_ident_raised{j}_{tag}"] = ident, iraised
        print(name, B, "pairs; raised (no_gaps):", out[f"{name}_raised_gaps"].tolist())
    out["sets"] = np.array(list(sets))
    path = os.path.join(ROOT, "tests", "golden", "g15_score.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
