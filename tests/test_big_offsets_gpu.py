"""GPU: every buffer of the strip-schedule families across the 2^31-byte and the 2^32-byte offset (tests/big_offsets.py has the
table and the harness; tests/test_big_offsets.py holds both to what they are there for, without a GPU).  One test per (family,
buffer, threshold): the engine's real entries on the smallest launch that puts WHOLE pairs wholly beyond the threshold -- forward
with state (into a buffer of 0xFF bytes where the entry takes one), value-only, backward or walk, the two adjoint sweeps for
the adjoint pairs; a `planes` case of a soft family runs the value-only sweep alone, which needs no state.  Every pair is held,
on the device, to the float64 reference of its class (the hard families: bit for bit) and to the first pair of its class as bit
patterns.  The `words` cases put the hard families' state past 2^31 pointer words; the three samplers' lists have a test of
their own at the end.  All launches run on one stream and none is captured."""
import time

import pytest
import torch

import big_offsets as bo
import family_fuzz as ff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _engine():
    from deepblast_amd._engine import get_engine
    return get_engine()


def _gather(blk, key, idx):
    """input `key` of the launch: the block's classes gathered on the device, pair b = class b % P"""
    return None if blk.get(key) is None else torch.from_numpy(blk[key]).to(DEV)[idx].contiguous()


def _prefilled(nbytes):
    """a state buffer of 0xFF bytes (NaN as floats): a record that is never written cannot pass for one that is"""
    return torch.full((max(nbytes, 4),), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float32)


def _run(c, blk):
    """the case through the engine's entries for its family -> dict of device tensors, as big_offsets.judge takes them"""
    eng, family, v = _engine(), c["family"], c["variant"]
    B, N, M = shape = (c["B"], c["N"], c["M"])
    idx = bo.classes(B, c["P"], DEV)
    t, A, X = (_gather(blk, k, idx) for k in ("theta", "A", "X"))       # (X: the affine families' gap_extend)
    ln, et = _gather(blk, "lens", idx), _gather(blk, "Et", idx)
    value_only = c["buffer"] == "planes" and family in ff.SOFT
    if family == bo.SWEEP:        # the main sweeps; the second order as training runs it: one exact state for all four sweeps
        exact = c["buffer"] != "packed"
        Vt, Q = eng.forward(t, A, v, ln, exact_state=exact)
        E = eng.backward(et, Q, shape, v, ln, exact_state=exact)
        if c["buffer"] != "state_d":
            return dict(Vt=Vt, E=E)
        del t, A
        Vtd, Qd = eng.adjoint_forward(Q, _gather(blk, "Z", idx), None, v, ln)
        Ed = eng.adjoint_backward(E, Q, Qd, v, ln)
        return dict(Vt=Vt, E=E, Vtd=Vtd, Ed=Ed)
    if family in bo.HARD:
        E = torch.full(shape, float("nan"), device=DEV)
        states = torch.full((B, eng.lib.sdp_traceback_capacity(N, M), 3), -1, dtype=torch.int32, device=DEV)
        if family == "hard":
            Vt, S = eng.hard_forward(t, A, v, ln)
            Vv = eng.hard_forward_value(t, A, v, ln)
            E, states, counts = eng.hard_walk(S, shape, v, ln, Et=et, E_out=E, states_out=states)
            return dict(Vt=Vt, Vv=Vv, E=E, states=states, counts=counts)
        if family == "hard_local":
            Vt, S, ends = eng.hard_local_forward(t, A, v, ln)
            Vv, ends_v = eng.hard_local_forward_value(t, A, v, ln)
            E, states, counts = eng.hard_local_walk(S, ends, shape, v, ln, Et=et, E_out=E, states_out=states)
            return dict(Vt=Vt, Vv=Vv, ends=ends, ends_v=ends_v, E=E, states=states, counts=counts)
        Vt, S, ends = eng.hard_affine_local_forward(t, A, X, ln)
        Vv, ends_v = eng.hard_affine_local_forward_value(t, A, X, ln)
        E, GO, GX, states, counts = eng.hard_affine_local_walk(S, ends, shape, ln, Et=et, want_GO=True, want_GX=True, E_out=E,
                                                               states_out=states)
        return dict(Vt=Vt, Vv=Vv, ends=ends, ends_v=ends_v, E=E, GO=GO, GX=GX, states=states, counts=counts)
    if family == ff.AFFINE:
        Vv = eng.affine_local_forward_value(t, A, X, ln)
        if value_only:
            return dict(Vv=Vv)
        Vt, state = eng.affine_local_forward(t, A, X, ln, state_out=_prefilled(eng.lib.sdp_affine_local_state_bytes(B, N, M)))
        E, GO, GX = eng.affine_local_backward(state, Vt, et, shape, ln)
        return dict(Vt=Vt, Vv=Vv, E=E, GO=GO, GX=GX)
    if family.startswith("soft_local"):
        Vv = eng.soft_local_forward_value(t, A, ln)
        if value_only:
            return dict(Vv=Vv)
        Vt, state = eng.soft_local_forward(t, A, ln, state_out=_prefilled(eng.lib.sdp_soft_local_state_bytes(B, N, M)))
        if family == "soft_local":
            E, G = eng.soft_local_backward(state, Vt, et, shape, ln)
            return dict(Vt=Vt, Vv=Vv, E=E, G=G)
        del t, A
        Vtd, state_d = eng.soft_local_adjoint_forward(state, Vt, _gather(blk, "ZE", idx), _gather(blk, "ZG", idx), shape, ln,
                                                      state_d_out=_prefilled(eng.lib.sdp_soft_local_adjoint_state_bytes(B, N, M)))
        Ed, Gd = eng.soft_local_adjoint_backward(state, state_d, Vt, Vtd, et, shape, ln)
        return dict(Vt=Vt, Vv=Vv, Vtd=Vtd, Ed=Ed, Gd=Gd)
    Vv = eng.sparsemax_forward_value(t, A, v, ln)
    if value_only:
        return dict(Vv=Vv)
    Vt, state = eng.sparsemax_forward(t, A, v, ln, state_out=_prefilled(eng.lib.sdp_sparsemax_state_bytes(B, N, M)))
    if family == "sparsemax":
        E, G = eng.sparsemax_backward(state, Vt, et, shape, v, ln)
        return dict(Vt=Vt, Vv=Vv, E=E, G=G)
    del t, A
    Vtd, state_d = eng.sparsemax_adjoint_forward(state, _gather(blk, "ZE", idx), _gather(blk, "ZG", idx), shape, v, ln,
                                                 state_d_out=_prefilled(eng.lib.sdp_sparsemax_adjoint_state_bytes(B, N, M)))
    Ed, Gd = eng.sparsemax_adjoint_backward(state, state_d, et, shape, v, ln)
    return dict(Vt=Vt, Vv=Vv, Vtd=Vtd, Ed=Ed, Gd=Gd)


_REFERENCES = {}


def _reference(c):
    """the block and its reference, computed once for the cases that share them (same family, shape, P and variant)"""
    key = (c["family"], c["N"], c["M"], c["P"], c["variant"])
    if key not in _REFERENCES:
        blk = bo.block(c)
        _REFERENCES[key] = (blk, bo.reference(c, blk))
    return _REFERENCES[key]


@pytest.mark.parametrize("case", bo.table()[0], ids=bo.case_ids())
def test_every_pair_of_a_launch_whose_buffer_crosses_the_threshold(case):
    c = case
    assert bo.layout(c["B"], c["threshold"], c["size"])[1:] == (1, bo.WHOLE) and c["bytes"] > c["threshold"]
    t0 = time.time()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    blk, want = _reference(c)
    t1 = time.time()
    got = None
    try:
        got = _run(c, blk)
        torch.cuda.synchronize()
        worst = bo.judge(c, blk, got, want)
        peak = torch.cuda.max_memory_allocated()
        print(f"\n[big offsets] {c['id']}: {c['N']} x {c['M']}, B = {c['B']}, P = {c['P']}, {c['bytes'] / 2 ** 30:.2f} GiB in the buffer, "
              f"peak {peak / 2 ** 30:.2f} GiB (estimate {c['peak'] / 2 ** 30:.2f}), reference {t1 - t0:.1f} s, all {time.time() - t0:.1f} s, worst "
              + " ".join(f"{k}={e:.2e}" for k, e in worst.items()))
        assert peak <= bo.CAP, (peak, bo.CAP)
    finally:
        del got
        torch.cuda.empty_cache()      # the caching allocator must not keep these GiB for the rest of the suite


# ---- the three samplers' lists: B K cap 3 int32 across the thresholds ----
def _guarded(n, dtype=torch.int32):
    """-> (buffer, view): `n` words at GUARD of a buffer filled with PATTERN"""
    buf = torch.full((n + 2 * bo.GUARD,), bo.PATTERN, dtype=torch.int32, device=DEV)
    return buf, buf[bo.GUARD:bo.GUARD + n].view(dtype)


SAMPLERS = bo.sampler_cases()


@pytest.mark.parametrize("case", SAMPLERS, ids=[c["id"] for c in SAMPLERS])
def test_every_list_of_a_sampler_launch_whose_lists_cross_the_threshold(case):
    """the forward sweep (into a state of 0xFF bytes where the entry takes one), the local samplers' tables, and K samples a pair
    through the C entries, every output a view into a buffer of PATTERN: every (pair, sample) list well-formed, the rows in front
    of it and the guards untouched, the counters a recount of the lists, on the device; the tables of a class the same bits in
    every pair; on CHOSEN pairs the end cells the restatement's draw on the device tables and the walks the float64 reference's"""
    from deepblast_amd._engine import EXACT_STATE
    c = case
    t0 = time.time()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    eng = _engine()
    lib = eng.lib
    kind, B, N, M, K, P = c["family"], c["B"], c["N"], c["M"], c["K"], c["P"]
    cap = lib.sdp_traceback_capacity(N, M)
    assert bo.layout(B, c["threshold"], c["size"])[1:] == (1, bo.WHOLE) and c["size"] == K * cap * 12
    blk = bo.sampler_block(c)
    bufs = got = state = None
    try:
        idx = bo.classes(B, P, DEV)
        ln = _gather(blk, "lens", idx)
        t, A = _gather(blk, "theta", idx), _gather(blk, "A", idx)
        if kind == bo.GLOBAL:
            Vt, state = eng.forward(t, A, c["variant"], ln, exact_state=c["exact"])
        elif kind == bo.SOFT_SAMPLER:
            Vt, state = eng.soft_local_forward(t, A, ln, state_out=_prefilled(lib.sdp_soft_local_state_bytes(B, N, M)))
        else:
            Vt, state = eng.affine_local_forward(t, A, _gather(blk, "X", idx), ln,
                                                 state_out=_prefilled(lib.sdp_affine_local_state_bytes(B, N, M)))
        del t, A
        shapes = {"states": (B, K, cap, 3), "counts": (B, K)}
        shapes.update({k: (B, N, M) for k in bo.SAMPLER_COUNTERS[kind]})
        if kind != bo.GLOBAL:
            shapes.update(cdf=(B, N, M), rows=(B, N + 1), ends=(B, K, bo.SAMPLER_ENDS[kind]))
        sizes = {k: int(torch.Size(v).numel()) for k, v in shapes.items()}
        bufs = {k: _guarded(n, torch.float32 if k in ("cdf", "rows") else torch.int32) for k, n in sizes.items()}
        for k in bo.SAMPLER_COUNTERS[kind]:
            bufs[k][1].zero_()
        p = {k: v[1].data_ptr() for k, v in bufs.items()}
        stream = torch.cuda.current_stream().cuda_stream
        s, v, lp = state.data_ptr(), Vt.data_ptr(), ln.data_ptr()
        if kind == bo.GLOBAL:
            rc = lib.sdp_sample_paths_f32(s, p["states"], p["counts"], p["visits"], B, N, M, K, 0, bo.SAMPLER_SEED, lp,
                                          c["variant"] | (EXACT_STATE if c["exact"] else 0), 0, stream)
        elif kind == bo.SOFT_SAMPLER:
            assert lib.sdp_soft_local_end_tables_f32(s, v, p["cdf"], p["rows"], B, N, M, lp, 0, 0, stream) == 0
            rc = lib.sdp_soft_local_sample_paths_f32(s, p["cdf"], p["rows"], p["states"], p["counts"], p["visits"], p["ends"], B, N, M, K,
                                                     0, bo.SAMPLER_SEED, lp, 0, 0, stream)
        else:
            assert lib.sdp_affine_local_end_tables_f32(s, v, p["cdf"], p["rows"], B, N, M, lp, 0, 0, stream) == 0
            rc = lib.sdp_affine_local_sample_paths_f32(s, v, p["cdf"], p["rows"], p["states"], p["counts"], p["visits"], p["opens"],
                                                       p["extends"], p["ends"], B, N, M, K, 0, bo.SAMPLER_SEED, lp, 0, 0, stream)
        assert rc == 0, lib.sdp_last_error_string()
        torch.cuda.synchronize()
        for k, (buf, _) in bufs.items():
            assert bool((buf[:bo.GUARD] == bo.PATTERN).all()) and bool((buf[bo.GUARD + sizes[k]:] == bo.PATTERN).all()), k
        got = {k: bufs[k][1].view(shapes[k]) for k in bufs}
        bo.judge_lists(c, blk, got)
        for k in ("cdf", "rows"):     # the tables of a class: the same bits in every pair (the draws are not: the counter has the pair)
            if k in got:
                bits = got[k].view(torch.int32)
                assert bool((bits == bits[:P][idx]).all()), k
        assert bool((got["states"][:B - P, :, -8:] != got["states"][P:, :, -8:]).any())
        pairs = bo.chosen_pairs(c)
        sub = {k: got[k][torch.tensor(pairs, device=DEV)].cpu().numpy() for k in ("states", "counts", "ends", "cdf", "rows") if k in got}
        excluded, walks, compared = bo.judge_walks(c, blk, pairs, sub)
        peak = torch.cuda.max_memory_allocated()
        print(f"\n[big offsets] {c['id']}: {N} x {M}, B = {B}, K = {K}, P = {P}, {c['bytes'] / 2 ** 30:.2f} GiB of lists, peak "
              f"{peak / 2 ** 30:.2f} GiB (estimate {c['peak'] / 2 ** 30:.2f}), all {time.time() - t0:.1f} s; pairs {pairs}: {excluded} of "
              f"{walks} walks excluded, {compared} non-empty walks compared")
        assert peak <= bo.CAP, (peak, bo.CAP)
    finally:
        del bufs, got, state
        torch.cuda.empty_cache()
