"""Alignment training targets on the device, from the state strings.

The reference builds the loss inputs per pair on the host, inside AlignmentDataset.__getitem__
(deepblast/dataset/dataset.py:157-179): the alignment matrix `dm` (states2matrix), the path-distance matrix `P`
(path_distance_matrix: a cKDTree query over all n*m cells) and the gap mask `G` (gap_mask), each transposed by
`reshape` when its shape is (len(other), len(gene)); collate_f then pads them into dense (B, N, M) tensors that are
copied to the GPU.  Here the strings are encoded on the host (a few KB per batch) and one kernel launch writes the
padded tensors (include/sdp.h: sdp_alignment_targets).  `P` is bit-identical to the reference's float32 tensor.
"""
import numpy as np
import torch

from . import _lib
from ._engine import get_engine

# tmstate_f inverted, indexed by the int state (deepblast.constants: x = 0, m = 1, y = 2): x -> '1', m -> ':', y -> '2'
_CODE_OF_STATE = np.frombuffer(b"1:2", dtype=np.uint8)


def _as_codes(a):
    """One alignment -> (uint8 codes, True if it came as int states)."""
    if isinstance(a, str):
        try:
            a = a.encode("ascii")
        except UnicodeEncodeError:
            raise ValueError("alignment strings must be ASCII (TM-align characters '1', '2', ':', '.')") from None
    if isinstance(a, (bytes, bytearray)):
        return np.frombuffer(bytes(a), dtype=np.uint8), False
    s = (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).reshape(-1)
    if s.size and not np.issubdtype(s.dtype, np.integer):
        raise ValueError(f"int states must have an integer dtype, got {s.dtype}")
    if s.size and (s.min() < 0 or s.max() > 2):
        raise ValueError("int states must be 0 (x), 1 (m) or 2 (y)")
    return _CODE_OF_STATE[s.astype(np.int64)], True


def _encode(alignments):
    parts = [_as_codes(a) for a in alignments]
    if not parts:
        raise ValueError("no alignments given")
    code_lens = np.array([len(p) for p, _ in parts], dtype=np.int32)
    empty = np.nonzero(code_lens == 0)[0]
    if empty.size:
        raise ValueError(f"empty alignment at pairs {empty.tolist()}")
    B, L = len(parts), int(code_lens.max())
    flat = np.concatenate([p for p, _ in parts])
    rows = np.repeat(np.arange(B), code_lens)
    cols = np.arange(flat.size) - np.repeat(np.cumsum(code_lens) - code_lens, code_lens)
    codes = np.zeros((B, L), dtype=np.uint8)
    codes[rows, cols] = flat
    return codes, code_lens, any(i for _, i in parts)


def encode_alignments(alignments, pin_memory=False):
    """alignments: list of str / bytes (TM-align state strings) or of int tensors / arrays of states 0 (x), 1 (m), 2 (y)
    -> (codes (B, L) uint8, code_lens (B,) int32), host tensors (pinned if asked).  Int states are written as
    '1' / ':' / '2'; they cannot tell ':' from '.', so gap-mask targets need the strings."""
    codes, code_lens, _ = _encode(alignments)
    codes, code_lens = torch.from_numpy(codes), torch.from_numpy(code_lens)
    if pin_memory:
        codes, code_lens = codes.pin_memory(), code_lens.pin_memory()
    return codes, code_lens


def extents(codes, code_lens):
    """(B, 2) int64 path extents (n, m) of encoded alignments: n = 1 + #{k >= 1: s_k != y}, m = 1 + #{k >= 1: s_k != x}
    (states2edges: the step of state k alone moves the path, state 0 marks cell (0, 0))."""
    codes = np.asarray(codes)
    code_lens = np.asarray(code_lens).reshape(-1)
    k = np.arange(codes.shape[1])
    live = (k[None, :] >= 1) & (k[None, :] < code_lens[:, None])
    nx = ((codes == ord("1")) & live).sum(1)
    ny = ((codes == ord("2")) & live).sum(1)
    return np.stack([code_lens - ny, code_lens - nx], axis=1).astype(np.int64)


def orientation(ext, lengths):
    """Per pair: 0 = written as is, 1 = transposed (reshape's quirk, dataset/utils.py:465-473), -1 = refused."""
    ext = np.asarray(ext)
    if lengths is None:
        return np.zeros(len(ext), dtype=np.int64)
    ln = np.asarray(lengths)
    same = (ext == ln).all(1)
    swapped = (ext[:, ::-1] == ln).all(1)
    return np.where(same, 0, np.where(swapped, 1, -1))


def alignment_targets(alignments, lengths=None, shape=None, device=None, path=True, alignment=True, gap_mask=False,
                      g_dtype=torch.bool):
    """Training targets of a batch on the device -> (dm, P, G), each (B, N, M) or None where not asked for.

    alignments : list of TM-align state strings (str / bytes), or of int state tensors / arrays (0 x, 1 m, 2 y)
    lengths    : optional (B, 2) (len(gene), len(other)): a pair whose path extent is the transpose of its lengths is
                 written transposed, as the reference's `reshape` does; any other mismatch raises ValueError
    shape      : (N, M) of the padded outputs; default the largest lengths (or the largest extents without lengths)
    path       : build P (the reference's path_distance_matrix, bit for bit)
    alignment  : build dm (states2matrix)
    gap_mask   : G is gap_mask(st) (':' path cells and cell (0, 0)) instead of ones over the block (mask_gaps=False);
                 needs the strings
    g_dtype    : torch.bool (collate_f's dtype) or torch.float32 (what the loss kernels read); None: no G
    Everything outside a pair's block is 0 in every output.  Runs on the current stream of `device` (default: the
    current device); validation is host-side, so the call does not synchronise."""
    if g_dtype not in (torch.bool, torch.float32, None):
        raise ValueError(f"g_dtype must be torch.bool, torch.float32 or None, got {g_dtype}")
    codes, code_lens, has_ints = _encode(alignments)
    if gap_mask and has_ints and g_dtype is not None:
        raise ValueError("gap_mask=True needs the alignment strings: int states cannot tell ':' from '.'")
    B = len(code_lens)
    ext = extents(codes, code_lens)
    lens_np = None
    if lengths is not None:
        lens_np = torch.as_tensor(lengths).detach().cpu().numpy().astype(np.int64).reshape(-1)
        if lens_np.size != 2 * B:
            raise ValueError(f"lengths must have shape ({B}, 2)")
        lens_np = lens_np.reshape(B, 2)
        bad = np.nonzero(orientation(ext, lens_np) < 0)[0]
        if bad.size:
            raise ValueError("alignment extent agrees neither with lengths nor with their transpose at pairs "
                             + ", ".join(f"{b} (extent {tuple(ext[b])}, lengths {tuple(lens_np[b])})" for b in bad[:8])
                             + (" ..." if bad.size > 8 else ""))
    block = lens_np if lens_np is not None else ext
    if shape is None:
        N, M = int(block[:, 0].max()), int(block[:, 1].max())
    else:
        N, M = (int(v) for v in shape)
        big = np.nonzero((block[:, 0] > N) | (block[:, 1] > M))[0]
        if big.size:
            raise ValueError(f"shape {(N, M)} is smaller than the blocks of pairs {big[:8].tolist()}")
    long_ = np.nonzero(ext.min(1) > 4096)[0]   # SDP_TARGETS_MAX_SHORT_SIDE: d2 of P must stay below 2^24
    if long_.size:
        raise ValueError(f"targets need min(n, m) <= 4096; pairs {long_[:8].tolist()} are larger")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("alignment_targets runs on a ROCm device only; there is no CPU fallback")
    pin = torch.cuda.is_available()
    codes_h = torch.from_numpy(codes)
    lens_h = torch.from_numpy(code_lens)
    if pin:
        codes_h, lens_h = codes_h.pin_memory(), lens_h.pin_memory()
    with torch.cuda.device(dev):
        codes_d = codes_h.to(dev, non_blocking=True)
        code_lens_d = lens_h.to(dev, non_blocking=True)
        lens_d = None
        if lens_np is not None:
            lh = torch.from_numpy(lens_np.astype(np.int32))
            lens_d = (lh.pin_memory() if pin else lh).to(dev, non_blocking=True)
        dm = torch.empty((B, N, M), dtype=torch.float32, device=dev) if alignment else None
        P = torch.empty((B, N, M), dtype=torch.float32, device=dev) if path else None
        G = torch.empty((B, N, M), dtype=g_dtype, device=dev) if g_dtype is not None else None
        status = torch.empty(B, dtype=torch.int32, device=dev)
        flags = (_lib.SDP_TARGETS_GAP_MASK if gap_mask else 0) | (_lib.SDP_TARGETS_G_F32 if g_dtype == torch.float32 else 0)
        get_engine().alignment_targets(codes_d, code_lens_d, lens_d, (B, N, M), dm, P, G, flags, status)
    return dm, P, G
