"""Accuracy statistics of predicted alignments on the device: the reference's deepblast/score.py.

Named after the reference module it replaces; it lives beside `deepblast_amd.scores`, which builds the match and gap
score tensors the DP consumes (row f1), and has nothing to do with it.

The reference scores alignments per pair on the host: the validation and test steps walk every pair, pull the walk to
the host and run states2edges -> filter_gaps -> roc_edges (DeepBLAST.validation_stats, deepblast/trainer.py:190-233);
benchmark evaluation runs alignment_score_kernel per data-frame row (deepblast/score.py:44-75).  Here one launch scores
a whole batch (include/sdp.h: sdp_alignment_stats), and the walk of `Decoder.validation_stats` never leaves the device.

Alignments are given as
  - a list of TM-align state strings (str / bytes: '1' x, '2' y, anything else m -- tmstate_f);
  - a list of int state arrays / tensors (0 x, 1 m, 2 y; the dataset's `states`, taken as they are, as the trainer does);
  - a list of host walks [(i, j, state), ...] (Decoder.traceback): the state column is read;
  - (codes, code_lens): (B, L) uint8 and (B,) int32 tensors, the format of targets.encode_alignments;
  - for the prediction also (states, counts): the device walk of Engine.traceback, (B, cap, 3) int32 and (B,) int32.
Edges come from the states alone (states2edges): the walk's own (i, j) are not used, as in the trainer.
"""
import numpy as np
import torch

from . import _lib, targets
from ._engine import get_engine

MAX_STATES = 16383           # include/sdp.h: SDP_SCORE_MAX_STATES
MAX_WIDTHS = 1024            # SDP_SCORE_MAX_WIDTHS
NO_TRUE_MATCH, NO_PRED_MATCH, WALK_RAISED, BAD_LENGTH, TOO_LONG = -1, -2, -3, -4, -5   # SDP_SCORE_* statuses
_REASON = {NO_TRUE_MATCH: "no match state in the true alignment", NO_PRED_MATCH: "no match state in the prediction",
           WALK_RAISED: "the traceback walked off its matrix", BAD_LENGTH: "length outside the array",
           TOO_LONG: f"more than {MAX_STATES} states"}

COLUMNS = ("tp", "fp", "fn", "perc_id", "ppv", "fnr", "fdr")   # roc_edges' order (score.py:8-18)


def _host_states(a):
    """A host walk [(i, j, state), ...] or (L, 3) array -> its state column; anything else as it is."""
    if isinstance(a, (str, bytes, bytearray)):
        return a
    if isinstance(a, torch.Tensor):
        return a[:, 2] if a.dim() == 2 and a.shape[1] == 3 else a
    if isinstance(a, (list, tuple)) and a and isinstance(a[0], (tuple, list)):
        return np.asarray(a)[:, 2]
    arr = np.asarray(a)
    return arr[:, 2] if arr.ndim == 2 and arr.shape[1] == 3 else a


def _parse(x, what, allow_walk):
    """Check one side -> (data, lens, is_walk): tensors as given, or host-encoded numpy codes and lengths."""
    if isinstance(x, tuple) and len(x) == 2 and isinstance(x[0], torch.Tensor) and x[0].dim() in (2, 3):
        data, lens = x
        lens = torch.as_tensor(lens)
        walk = data.dim() == 3
        if walk and not allow_walk:
            raise ValueError(f"{what}: a device walk is accepted for the prediction only")
        if walk and (data.dtype != torch.int32 or data.shape[2] != 3):
            raise ValueError(f"{what}: a walk must be a (B, cap, 3) int32 tensor, got {tuple(data.shape)} {data.dtype}")
        if not walk and data.dtype != torch.uint8:
            raise ValueError(f"{what}: codes must be a (B, L) uint8 tensor, got {data.dtype}")
        if lens.shape != (data.shape[0],) or lens.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{what}: lengths must be a ({data.shape[0]},) integer tensor")
        return data, lens, walk
    codes, code_lens, _ = targets._encode([_host_states(a) for a in x])
    long_ = np.nonzero(code_lens > MAX_STATES)[0]
    if long_.size:
        raise ValueError(f"{what}: pairs {long_[:8].tolist()} have more than {MAX_STATES} states")
    return codes, code_lens, False


def _to(side, dev):
    data, lens, walk = side
    if isinstance(data, torch.Tensor):
        return data.to(dev).contiguous(), lens.to(dev, torch.int32).contiguous(), walk
    c, n = torch.from_numpy(data), torch.from_numpy(lens)
    if torch.cuda.is_available():
        c, n = c.pin_memory(), n.pin_memory()
    return c.to(dev, non_blocking=True), n.to(dev, non_blocking=True), False


def _raise_for(status):
    """The exception the reference raises for the first failing pair (it scores pairs in order), naming all of them."""
    bad = np.nonzero(status < 0)[0]
    if not bad.size:
        return
    desc = "; ".join(f"pair {b}: {_REASON.get(int(status[b]), f'status {int(status[b])}')}" for b in bad[:8])
    desc += " ..." if bad.size > 8 else ""
    if status[bad[0]] == WALK_RAISED:
        raise IndexError(f"traceback walked off the matrix ({desc})")
    raise ValueError(f"alignment statistics undefined ({desc})")


def _launch(true_states, pred_states, no_gaps, device, widths=None, offsets=None, want_stats=True):
    tside = _parse(true_states, "true_states", False)
    pside = _parse(pred_states, "pred_states", True)
    dev = torch.device(device) if device is not None else None
    if dev is not None and dev.type != "cuda":
        raise RuntimeError("deepblast_amd.score runs on a ROCm device only; there is no CPU fallback")
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        tc, tl, _ = _to(tside, dev)
        pd, pl, walk = _to(pside, dev)
        B = tc.shape[0]
        if pd.shape[0] != B:
            raise ValueError(f"{B} true alignments but {pd.shape[0]} predicted ones")
        w_d = None
        W = 0
        if widths is not None:
            w = np.asarray(list(widths), dtype=np.int64).reshape(-1)
            if w.size > MAX_WIDTHS:
                raise ValueError(f"at most {MAX_WIDTHS} kernel widths, got {w.size}")
            if w.size and (w.min() < -2 ** 31 or w.max() >= 2 ** 31):
                raise ValueError("kernel widths must fit in int32")
            W = int(w.size)
            w_d = torch.from_numpy(w.astype(np.int32)).to(dev) if W else None
        off_d = None
        if offsets is not None:
            off = torch.as_tensor(offsets)
            if off.shape != (B, 2):
                raise ValueError(f"offsets must have shape ({B}, 2), got {tuple(off.shape)}")
            if off.is_floating_point():
                raise ValueError("offsets must be integers")
            if not off.is_cuda and off.numel():
                o64 = off.to(torch.int64)
                if o64.min() < -2 ** 31 or o64.max() >= 2 ** 31:
                    raise ValueError("offsets must fit in int32")
            off_d = off.to(dev, torch.int32).contiguous()
        counts = torch.empty((B, 5), dtype=torch.int32, device=dev)
        stats = torch.empty((B, 7), dtype=torch.float64, device=dev) if want_stats else None
        ident = torch.empty((B, W), dtype=torch.float64, device=dev) if widths is not None else None
        status = torch.empty(B, dtype=torch.int32, device=dev)
        flags = (_lib.SDP_SCORE_NO_GAPS if no_gaps else 0) | (_lib.SDP_SCORE_PRED_WALK if walk else 0)
        get_engine().alignment_stats(tc, tl, pd, pl, off_d, w_d, flags, counts, stats, None, ident if W else None, status)
    return stats, ident, status


def alignment_stats(true_states, pred_states, no_gaps=True, device=None, strict=True):
    """roc_edges of every pair -> (B, 7) float64 on the device, columns COLUMNS (tp, fp, fn, perc_id, ppv, fnr, fdr).

    Row b equals deepblast.score.alignment_score(true[b], pred[b], no_gaps) for strings, and the trainer's
    states2edges -> filter_gaps -> roc_edges composition for int states and walks, bit for bit: the ratios are correctly
    rounded float64 divisions of the integer counts, as Python's.
    strict=True  : raises where the reference raises -- ValueError (filter_gaps: no match state on a side with
                   no_gaps) or IndexError (a walk that left its matrix) -- naming the pairs; this reads the per-pair
                   status back, so the call synchronises with the launch.
    strict=False : those rows are NaN, and nothing is read back (for a validation loop that must not stop).
    Empty alignments and alignments of more than 16 383 states are refused (ValueError) when given from the host;
    given as device tensors they become NaN rows (strict=False) or a ValueError."""
    stats, _, status = _launch(true_states, pred_states, no_gaps, device)
    if strict:
        _raise_for(status.cpu().numpy())
    return stats


def alignment_identity(true_states, pred_states, kernel_widths, offsets=None, no_gaps=True, device=None, strict=True):
    """deepblast.score.alignment_score_kernel of every pair -> (B, W) float64 on the device, W = len(kernel_widths).

    offsets: optional (B, 2) integers (query_offset, hit_offset), added to the predicted edges (score_local_identity
    passes a row's query_start / hit_start; its `query_start < 0 -> zeros` rule belongs to the caller).  Width i counts a
    true edge as hit if a predicted edge lies on its diagonal within a row distance S_i = sum over t <= i of
    max(w_t - 1, 0): the reference's roc_edges_kernel_identity widens the caller's list in place, so the widths of one
    call accumulate ([1, 2, 3] gives the values of [1], [2] and [4]), and this is reproduced.  strict: as alignment_stats."""
    _, ident, status = _launch(true_states, pred_states, no_gaps, device, widths=kernel_widths, offsets=offsets,
                               want_stats=False)
    if strict:
        _raise_for(status.cpu().numpy())
    return ident
