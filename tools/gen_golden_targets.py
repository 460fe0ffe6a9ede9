#!/usr/bin/env python
"""Golden vectors for deepblast_amd.targets (tests/golden/g13_targets.npz).

Provenance: runs the REAL reference dataset helpers of flatironinstitute/deepblast, deepblast/dataset/utils.py --
states2edges (:107-114), states2matrix (:117-134), path_distance_matrix (:315-339, scipy cKDTree), gap_mask (:393-409),
reshape (:465-473), collate_f (:254-279) -- on synthetic TM-align state strings, item by item as
AlignmentDataset.__getitem__ builds them (deepblast/dataset/dataset.py:157-179: tmstate_f states, lg, lp = len(gene),
len(pos)), once with mask_gaps=True and once with mask_gaps=False, and stores the strings, the lengths and what collate_f
returned.  utils.py is loaded on its own (deepblast/dataset/__init__.py needs Biopython) with oracle/_shim standing in
for numba, as oracle/gen_golden_batching.py does.  Data only; needs the reference checkout (default /root/reference,
or $DEEPBLAST_REFERENCE) and scipy.

    python tools/gen_golden_targets.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("DEEPBLAST_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "oracle", "_shim"))
sys.path.insert(1, REF)
_spec = importlib.util.spec_from_file_location("_ref_dataset_utils", os.path.join(REF, "deepblast", "dataset", "utils.py"))
_u = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_u)


def _item(st, lens, mask_gaps):
    """AlignmentDataset.__getitem__ (dataset.py:147-182) with construct_paths=True, clip_ends=False, pad_ends=False, the
    tokenizer replaced by placeholder sequences of the given lengths."""
    states = torch.Tensor(list(map(_u.tmstate_f, st))).long()
    alignment_matrix = torch.from_numpy(_u.states2matrix(states))
    lg, lp = lens
    path_matrix = _u.reshape(torch.from_numpy(_u.path_distance_matrix(_u.states2edges(states))), lg, lp)
    g_mask = torch.ones(*alignment_matrix.shape)
    if mask_gaps:
        g_mask = torch.from_numpy(_u.gap_mask(st)).bool()
    alignment_matrix = _u.reshape(alignment_matrix, lg, lp)
    g_mask = _u.reshape(g_mask, lg, lp)
    return (torch.zeros(lg), torch.zeros(lp), states, alignment_matrix, path_matrix, g_mask, torch.ones(lg), torch.ones(lp))


def _extent(st):
    m = _u.states2matrix(np.array(list(map(_u.tmstate_f, st))))
    return m.shape


def _random_string(rng, L, p_gap, run):
    """Match / mismatch runs with gap runs of mean length `run` in between."""
    out = []
    while len(out) < L:
        if rng.random() < p_gap:
            out += [rng.choice(["1", "2"])] * int(rng.geometric(1.0 / run))
        else:
            out += [":" if rng.random() < 0.8 else "."] * int(rng.integers(1, 6))
    return "".join(out[:L])


def batches():
    rng = np.random.default_rng(1313)
    T = "transpose"
    return {
        # single characters (the first state only marks (0, 0), whatever it is), a 1 x 1 pair among longer ones
        "single": [":", ".", "1", "2", "1:", "2:"],
        # leading and trailing gap runs, unclipped; '.' mismatches; a first character that is not ':'
        "ends": ["111::.:22", "22:.::11", ".::1:2:.", "1::::", "2::..", "::.:.::..::", "..:::."],
        # L-shaped paths both ways, a pure diagonal, a staircase
        "shapes": [":" + "2" * 30 + "1" * 20, ":" + "1" * 25 + "2" * 33, ":" * 40, "1" + "21" * 18,
                   "2" * 12 + "1" * 40 + ":" * 3],
        # extents that are the transpose of (len(gene), len(other)): reshape writes them transposed
        "transposed": [(":" + "1" * 6 + ":::", T), ("2" + "2" * 9 + ":.:", T), (":" * 5, None), ("1:2:2:2", T)],
        # a ragged batch of random strings with short and long gap runs, and a 1 x 1 pair in it
        "ragged": [_random_string(rng, 90, 0.2, 2.0), ":", _random_string(rng, 140, 0.1, 12.0),
                   _random_string(rng, 60, 0.5, 4.0), _random_string(rng, 120, 0.05, 30.0)],
    }


def main():
    out = {"provenance": np.array(
        "deepblast/dataset/utils.py states2edges/states2matrix/path_distance_matrix/gap_mask/reshape/collate_f and "
        "dataset.py:157-179 (item construction), run by tools/gen_golden_targets.py; scipy " + __import__("scipy").__version__)}
    names = []
    for name, items in batches().items():
        strings, lens = [], []
        for it in items:
            st, how = it if isinstance(it, tuple) else (it, None)
            n, m = _extent(st)
            strings.append(st)
            lens.append((m, n) if how == "transpose" else (n, m))
        for mask_gaps in (True, False):
            batch = [_item(st, ln, mask_gaps) for st, ln in zip(strings, lens)]
            _, _, _, dm, p, G, _, _ = _u.collate_f(batch)
            key = "G_gap" if mask_gaps else "G_plain"
            out[f"{name}_{key}"] = G.numpy()
        out[f"{name}_dm"] = dm.numpy()
        out[f"{name}_p"] = p.numpy()
        L = max(map(len, strings))
        codes = np.zeros((len(strings), L), dtype=np.uint8)
        for b, st in enumerate(strings):
            codes[b, :len(st)] = np.frombuffer(st.encode(), dtype=np.uint8)
        out[f"{name}_codes"] = codes
        out[f"{name}_code_lens"] = np.array(list(map(len, strings)), dtype=np.int32)
        out[f"{name}_lens"] = np.array(lens, dtype=np.int32)
        names.append(name)
        print(name, "dm", tuple(dm.shape), "lens", lens)
    out["batches"] = np.array(names)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "g13_targets.npz"), **out)


if __name__ == "__main__":
    main()
