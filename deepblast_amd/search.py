"""Alignment scores of one query against a database, on the device (the loop of the reference's scripts/deepblast-search).

The reference's search script embeds a query and every database sequence, calls `NeuralAligner.score` per pair
(deepblast/alignment.py:127-137: theta and A from the embeddings, the DP under torch.no_grad(), only Vt kept) and writes
Vt and Vt / (qlen * dlen) per pair (scripts/deepblast-search:38-49).  `search_scores` is that loop for one query against
a padded database: per chunk of targets one score launch (`deepblast_amd.scores.alignment_scores`) and one value-only
forward sweep (`Decoder.score`: no state is formed or stored), the results written into (T,) tensors in database order.
Nothing is differentiated and nothing but the scores reaches the host.
"""
from collections import namedtuple

import torch

from .scores import alignment_scores

SearchResult = namedtuple("SearchResult", ["score", "normalized", "indices", "values"])
SearchResult.__doc__ = """score (T,): Vt per target; normalized (T,): Vt / (qlen * dlen) (deepblast-search:43-44);
indices / values (k,): the top-k targets by `normalized`, best first (None without topk)."""


def search_scores(decoder, zq, gq, zdb, gdb, db_lengths, query_length=None, chunk=256, topk=None):
    """One query against a padded database -> SearchResult.

    decoder       a NeedlemanWunschDecoder / SmithWatermanDecoder (its `score` is the value-only sweep).  A LOCAL decoder
                  (Decoder('hardmax', local=True)) gives local scores: the best cell of the max-plus table with a zero floor.
                  alignment_scores produces theta = softplus(.) >= 0, and with theta >= 0 nothing ever floors -- the result is
                  then the free-end-gaps optimum; for true locality shift theta by a threshold of your choosing (a decoder
                  wrapper whose score() subtracts it).  Any object with score(theta, A, lengths) -> (B,) serves:
                  deepblast_amd.sparse.SparsemaxDecoder and deepblast_amd.local.SoftLocalDecoder rank a database by their scores.
    zq, gq        (N, D) match / gap embeddings of the query.
    zdb, gdb      (T, Mmax, D) match / gap embeddings of the T targets, zero padded behind each target's length.
    db_lengths    (T,) int: residues per target (1 .. Mmax).
    query_length  residues of the query, <= N (default: N).
    chunk         targets per launch: the chunk's theta and A, 2 x chunk x N x Mmax floats, are the memory this takes.
    topk          also return the k best targets by `normalized`.

    The database is walked in chunks of `chunk` targets under torch.no_grad(); pair b of a chunk runs with lengths
    (query_length, db_lengths[b]), so the padding takes no part.  The query's embeddings are expanded to the chunk once and
    reused.  Everything stays on the device and is enqueued on the current stream: no host synchronisation happens here
    (reading the result is the caller's).  Padding costs score-kernel work in proportion to Mmax: sorting the database by
    length, so that a chunk's targets are about as long as each other, is the caller's business."""
    if zq.dim() != 2 or gq.shape != zq.shape:
        raise ValueError(f"zq and gq must both be (N, D); got {tuple(zq.shape)} and {tuple(gq.shape)}")
    if zdb.dim() != 3 or gdb.shape != zdb.shape or zdb.shape[2] != zq.shape[1]:
        raise ValueError(f"zdb and gdb must both be (T, Mmax, {zq.shape[1]}); got {tuple(zdb.shape)} and {tuple(gdb.shape)}")
    T, Mmax, _ = zdb.shape
    N = zq.shape[0]
    chunk = int(chunk)
    if T < 1 or chunk < 1:
        raise ValueError("search_scores needs at least one target and chunk >= 1")
    qlen = N if query_length is None else int(query_length)
    if not 1 <= qlen <= N:
        raise ValueError(f"query_length must be in 1..{N}, got {qlen}")
    dev = zq.device
    dlen = torch.as_tensor(db_lengths, device=dev).to(torch.int32).reshape(-1)
    if dlen.shape[0] != T:
        raise ValueError(f"db_lengths must have {T} entries, got {dlen.shape[0]}")
    if topk is not None and not 1 <= int(topk) <= T:
        raise ValueError(f"topk must be in 1..{T}, got {topk}")
    with torch.no_grad():
        lengths = torch.stack([torch.full_like(dlen, qlen), dlen], dim=1)
        score = torch.empty(T, dtype=zq.dtype, device=dev)
        C = min(chunk, T)
        zq_c = zq.detach().unsqueeze(0).expand(C, -1, -1).contiguous()
        gq_c = gq.detach().unsqueeze(0).expand(C, -1, -1).contiguous()
        for lo in range(0, T, C):
            hi = min(lo + C, T)
            c = hi - lo
            theta, A = alignment_scores(zq_c[:c], zdb[lo:hi].detach(), gq_c[:c], gdb[lo:hi].detach())
            score[lo:hi] = decoder.score(theta, A, lengths[lo:hi])
        normalized = score / (qlen * dlen).to(score.dtype)
        indices = values = None
        if topk is not None:
            values, indices = torch.topk(normalized, int(topk))
    return SearchResult(score, normalized, indices, values)
