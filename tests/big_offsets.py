"""Buffers past 2^31 and 2^32 bytes in the strip-schedule families: the table of cases and the harness that judges a launch.  TESTS
ONLY, no GPU here: tests/test_big_offsets.py (CPU) and tests/test_big_offsets_gpu.py (GPU) see the same cases.

A case is (family, buffer, threshold): the smallest launch whose `buffer` has pairs wholly below the byte offset `threshold`, one
pair astride it and WHOLE pairs wholly above it.  B is derived from the library's own sdp_*_state_bytes(B, N, M) (`planes`: from
B N M 4), never hand-picked.  The shapes are the smallest padded pairs with a strip hand-off and more than one chunk: 65 x 66 (two
strips, five chunks) for the soft families, 65 x 3 for the hard ones, whose state is tiny per pair -- padding makes the state
large while the inputs stay small.  (65 x 34, four chunks, makes the 16-byte families' pair 2^18 bytes: no pair would lie astride.)

Inputs: a block of P distinct pairs (classes) drawn on the CPU -- P prime, scores from the SAFE score families of tests/
family_fuzz.py (the hard families: their exact ties / floors families), lengths full or -2 .. N + 3, Et from ET_VALUES, cotangents
-- and pair b of the launch is class b % P: the big tensors are an index gather on the device and never exist on the host.  The
alias distance -- threshold / one pair's bytes, rounded either way -- is never a multiple of P, so that a record offset truncated
to 32 bits lands on a pair of another class.  judge() then holds every pair to the float64 reference of its class (the hard
families: bit for bit) AND to the first pair of its class, which lies below every threshold, as bit patterns: one workgroup per
pair, the wave count a function of the shape alone (strip_waves, csrc/sdp_api.hip), no atomics in any sweep or walk.

table() -> (the cases, the cases that the memory cap -- CAP bytes of peak device memory, a condition on a shared machine and not a
measurement -- or the launch limit leaves out, with the bytes they would have needed).  Beside the strip-schedule families: the
main sweeps of csrc/sdp_kernels.hip (family "sweep": the packed, the exact and the second-order state; the float64 reference is
tests/parity.py's oracle), the hard families' state past 2^31 pointer WORDS (`words`: the one 32-bit element index the cap lets a
launch reach) and the `states` lists of the three samplers (sampler_cases(), judge_lists(), judge_walks()).
NOT_BUILT: what the issue names and the table does not cover (nothing).  DESIGN.md 3.21a has the measured table and what these cases cannot reach."""
import numpy as np
import torch

import datagen
import family_fuzz as ff
import hard_affine_ref
import parity
import soft_local_adjoint_ref
from parity import TOL

HARD_AFFINE = "hard_affine_local"
FAMILIES = ff.FAMILIES + (HARD_AFFINE,)
SWEEP = "sweep"                          # the main sweeps of csrc/sdp_kernels.hip, first and second order
HARD = ("hard", "hard_local", HARD_AFFINE)
THRESHOLDS = (2 ** 31, 2 ** 32)
WHOLE = 64                               # pairs wholly beyond the threshold
CAP = 20 * 2 ** 30                       # peak device bytes of a case
LIMIT = 2 ** 31                          # B N M of a launch (flagless_args and the hard families' check_shape)
PRIMES = (257, 263, 251, 269, 241)       # P: the first of these no alias distance is a multiple of
COMPARE = 1 << 24                        # elements of one comparison chunk in judge(): whole pairs, 128 MiB in float64
WIDE, THIN = (65, 66), (65, 3)
SEED = 20261020
STATE_BYTES = {"hard": "sdp_hard_state_bytes", "hard_local": "sdp_hard_state_bytes", "soft_local": "sdp_soft_local_state_bytes",
               "soft_local_adjoint": "sdp_soft_local_adjoint_state_bytes", "sparsemax": "sdp_sparsemax_state_bytes",
               "sparsemax_adjoint": "sdp_sparsemax_adjoint_state_bytes", "affine_local": "sdp_affine_local_state_bytes",
               HARD_AFFINE: "sdp_hard_affine_local_state_bytes"}
# the score families of a block, taking turns by class: SAFE n SCORES[family]; the hard families' exact ones
SCORES = {f: tuple(n for n, _ in ff.SCORES[f] if n in ff.SAFE) for f in ff.SOFT}
SCORES.update({"hard": ("ties",), "hard_local": ("ties", "floors"), HARD_AFFINE: ("ties", "floors")})
# the buffers of every family that the table puts across the thresholds.  `planes`: the (B, N, M) inputs and outputs themselves,
# past 2^31 bytes only (2^32 bytes of one plane are 2^30 elements: inputs and outputs of such a launch alone exceed CAP)
BUFFERS = {f: ("state", "planes") for f in FAMILIES}
# the kernels index their states in ELEMENTS, so an index held in a signed 32-bit int wraps at 2^31 of them.  The cap lets the hard
# families' 4-byte pointer words get there (`words`: the state past 2^31 words = 2^33 bytes); the soft families' 16-byte records
# would need a 32 GiB state
WORDS = 2 ** 33
BUFFERS.update({f: ("state", "planes", "words") for f in HARD})
BUFFERS.update({f: ("state_d",) for f in ff.ADJOINT})
# the main sweeps: the packed state past 2^31 bytes, the exact state (SDP_EXACT_STATE) past both, the second-order state past 2^31
SWEEP_BUFFERS = (("packed", THRESHOLDS[:1]), ("exact", THRESHOLDS), ("state_d", THRESHOLDS[:1]))
SWEEP_OUTPUTS = {"packed": ("Vt", "E"), "exact": ("Vt", "E"), "state_d": ("Vt", "E", "Vtd", "Ed")}
# what the issue asks for and this table does not hold (no case, no test): said here so that nobody reads the table as complete
NOT_BUILT = ()

# measured on the MI355X by tests/test_big_offsets_gpu.py: case id -> (seconds of the whole test, the references included -- they
# dominate, and a block that an earlier case of the family computed is shared --, peak device GiB as torch.cuda.max_memory_allocated
# reports them)
MEASURED = {"hard-state-2^31": (0.8, 4.09),
            "hard-state-2^32": (0.3, 8.18),
            "hard-planes-2^31": (0.1, 16.12),
            "hard-words-2^33": (0.1, 16.37),
            "hard_local-state-2^31": (0.2, 4.1),
            "hard_local-state-2^32": (0.2, 8.2),
            "hard_local-planes-2^31": (0.1, 16.16),
            "hard_local-words-2^33": (0.1, 16.41),
            "soft_local-state-2^31": (1.2, 2.44),
            "soft_local-state-2^32": (0.8, 4.86),
            "soft_local-planes-2^31": (0.0, 4.01),
            "soft_local_adjoint-state_d-2^31": (2.6, 4.25),
            "soft_local_adjoint-state_d-2^32": (2.7, 8.46),
            "sparsemax-state-2^31": (0.9, 2.44),
            "sparsemax-state-2^32": (0.9, 4.86),
            "sparsemax-planes-2^31": (0.0, 4.01),
            "sparsemax_adjoint-state_d-2^31": (2.9, 4.25),
            "sparsemax_adjoint-state_d-2^32": (2.9, 8.46),
            "affine_local-state-2^31": (1.8, 2.27),
            "affine_local-state-2^32": (1.8, 4.48),
            "affine_local-planes-2^31": (0.0, 6.01),
            "hard_affine_local-state-2^31": (0.4, 3.21),
            "hard_affine_local-state-2^32": (0.0, 6.42),
            "hard_affine_local-words-2^33": (0.1, 12.84),
            "sweep-packed-2^31": (0.1, 2.85),
            "sweep-exact-2^31": (0.1, 2.54),
            "sweep-exact-2^32": (0.0, 5.06),
            "sweep-state_d-2^31": (0.0, 4.38),
            "sample-lists-2^31": (1.0, 2.53),
            "sample-lists-2^32": (1.0, 5.25),
            "soft_local_sample-lists-2^31": (0.8, 3.09),
            "soft_local_sample-lists-2^32": (0.9, 6.0),
            "affine_local_sample-lists-2^31": (1.2, 4.83),
            "affine_local_sample-lists-2^32": (1.3, 9.43),}


def _lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def shape_of(family):
    return THIN if family in HARD else WIDE


def pair_bytes(family, buffer, N, M):
    """one pair's bytes in `buffer`, from the library's size functions (which are linear in B: asserted)"""
    if buffer == "planes":
        return N * M * 4
    if family == SWEEP:       # the distance between the records of consecutive pairs (order, bridge rows and map lie behind the last)
        one = int(_lib().sdp_state_pair_stride(N, M, 0 if buffer == "packed" else 1))
        assert one > 0
        return one
    f = getattr(_lib(), STATE_BYTES[family])
    one = int(f(1, N, M))
    assert one > 0 and int(f(1000, N, M)) == 1000 * one, (family, one)
    return one


def aliases(threshold, size):
    """the alias distances, in pairs, of a byte offset truncated at `threshold`: threshold / size rounded either way"""
    return tuple(sorted({threshold // size, -(-threshold // size)}))


def min_batch(threshold, size):
    """the smallest B with WHOLE pairs of `size` bytes wholly beyond `threshold`"""
    return -(-threshold // size) + WHOLE


def layout(B, threshold, size):
    """-> (pairs wholly below, pairs astride, pairs wholly above) the byte offset `threshold`"""
    below = threshold // size
    astride = 1 if threshold % size else 0
    return min(below, B), astride if below < B else 0, max(0, B - below - astride)


def plane_count(family, buffer):
    """(B, N, M) fp32 tensors alive at once in a case's launch: inputs, cotangents, outputs"""
    if buffer == "planes" and family not in HARD:
        return {"affine_local": 3}.get(family, 2)                    # the value-only sweep: the inputs alone
    if family == SWEEP:
        return 5 if buffer == "state_d" else 3
    return {"hard": 3, "hard_local": 3, HARD_AFFINE: 6, "soft_local": 4, "sparsemax": 4, "affine_local": 6,
            "soft_local_adjoint": 6, "sparsemax_adjoint": 6}[family]


def peak_bytes(family, buffer, B, N, M, P):
    """the estimate of a case's peak device bytes: inputs, outputs, states, lists, the P-class block and reference uploaded for the
    comparison, and the comparison's temporaries (chunks of COMPARE elements in float64 and as masks)"""
    planes = plane_count(family, buffer) * B * N * M * 4
    states = 0
    if family == SWEEP:
        states = B * pair_bytes(family, buffer, N, M) * (2 if buffer == "state_d" else 1)
    elif buffer != "planes" or family in HARD:
        states = B * pair_bytes(family, "state", N, M) * (2 if family in ff.ADJOINT else 1)
    lists = B * (N + M + 2) * 3 * 4 if family in HARD else 0
    block = P * N * M * (8 * 4 + 4 * 5)
    temporaries = COMPARE * 8 * 6
    return planes + states + lists + block + temporaries + B * 64


def _prime(distances):
    for p in PRIMES:
        if all(d % p for d in distances):
            return p
    raise AssertionError(f"every P of {PRIMES} divides one of the alias distances {distances}")


def thresholds_of(buffer):
    return {"planes": THRESHOLDS[:1], "words": (WORDS,)}.get(buffer, THRESHOLDS)


def _variant(family, threshold):
    return None if ff.VARIANTS.get(family, (None,)) == (None,) else (ff.NW, ff.SW)[threshold.bit_length() % 2]


def _case(family, buffer, threshold, N, M, B=None, P=None):
    size = pair_bytes(family, "state" if buffer == "words" else buffer, N, M)
    B = min_batch(threshold, size) if B is None else B
    P = _prime(aliases(threshold, size)) if P is None else P
    return dict(family=family, buffer=buffer, threshold=threshold, N=N, M=M, B=B, P=P, size=size, bytes=B * size,
                variant=_variant(family, threshold), peak=peak_bytes(family, buffer, B, N, M, P),
                id=f"{family}-{buffer}-2^{threshold.bit_length() - 1}")


def _table():
    cases, dropped = [], []
    for family in FAMILIES:
        N, M = shape_of(family)
        for buffer in BUFFERS[family]:
            for threshold in thresholds_of(buffer):
                c = _case(family, buffer, threshold, N, M)
                (cases if c["peak"] <= CAP and c["B"] * N * M <= LIMIT else dropped).append(c)
    for buffer, thresholds in SWEEP_BUFFERS:
        for threshold in thresholds:
            c = _case(SWEEP, buffer, threshold, *WIDE)
            c["variant"] = (ff.NW, ff.SW)[(THRESHOLDS.index(threshold) + (buffer != "packed")) % 2]
            (cases if c["peak"] <= CAP and c["B"] * c["N"] * c["M"] <= LIMIT else dropped).append(c)
    return tuple(cases), tuple(dropped)


_TABLE = None


def table():
    """-> (CASES, DROPPED): built once, on the first call.  It asks the library for the sizes, and the two test files call it
    when they are imported (the cases are their parameters): collecting them loads libsdp_hip.so, and builds it first if it is
    not there or older than its sources, as tests/test_abi.py's fixture does.  The CPU file takes about 100 s, of which the
    admission of the ten soft blocks -- both references of 257 or 263 pairs of 65 x 66, up to 9 s each -- is most"""
    global _TABLE
    if _TABLE is None:
        _TABLE = _table()
    return _TABLE


def case_ids():
    return [c["id"] for c in table()[0]]


def small(c):
    """the case scaled down for the CPU stand-in: B = 3 P pairs, and a threshold P + P/2 + 0.6 pairs into its buffer, so that it
    has pairs below, one astride, more than WHOLE above -- and alias distances that are no multiple of P, as in the table"""
    P = c["P"]
    threshold = c["size"] * (P + P // 2) + (c["size"] * 3) // 5
    s = dict(c, B=3 * P, threshold=threshold, bytes=3 * P * c["size"])
    assert all(d % P for d in aliases(threshold, c["size"])) and layout(s["B"], threshold, c["size"])[2] >= WHOLE
    return s


# ---- the block of P classes ----
def _block_scores(family, seed, P, N, M):
    """-> [theta, A(, X)] (P, N, M): class p from the score family SCORES[family][p % len]"""
    names = SCORES[family]
    assert names, family
    drawn = []
    for k, name in enumerate(names):
        if family == HARD_AFFINE:
            drawn.append(hard_affine_ref.FAMILIES[name](seed + k, P, N, M))
        else:
            drawn.append(ff._scores(family, name, seed + k, P, N, M)[:3 if family == ff.AFFINE else 2])
    turn = np.arange(P) % len(names)
    return [np.ascontiguousarray(np.choose(turn[:, None, None], [d[i] for d in drawn]), np.float32) for i in range(len(drawn[0]))]


def block(c, seed=SEED):
    """the P classes of a case as a case of tests/family_fuzz.py with B = P (family_fuzz.reference, admitted and blocks take
    it): theta, A (the affine families: gap_open) and X, lens (P, 2) -- the first class and every other one full pairs, the rest
    -2 .. N + 3 as in the fuzz --, Et from ET_VALUES, cotangents for the adjoint pairs; every sixth class of a soft family
    forbids a fifth of its gaps (-inf: the affine family's openings, extensions or both in turn)"""
    family, P, N, M = c["family"], c["P"], c["N"], c["M"]
    if family == SWEEP:
        return _sweep_block(c, seed)
    rng = np.random.default_rng([seed, FAMILIES.index(family), N, M, P])
    theta, A, *rest = _block_scores(family, int(rng.integers(1, 2 ** 30)), P, N, M)
    X = rest[0] if rest else None
    if family in ff.SOFT:
        for p in range(5, P, 6):
            on = ff.MASKED[(p // 6) % 3] if family == ff.AFFINE else "O"
            if on != "X":
                A[p][rng.random((N, M)) < 0.2] = -np.inf
            if on != "O":
                X[p][rng.random((N, M)) < 0.2] = -np.inf
    lens = np.stack([rng.integers(-2, N + 4, P), rng.integers(-2, M + 4, P)], axis=1).astype(np.int32)
    lens[::2] = (N, M)
    Et = ff.ET_VALUES[rng.integers(0, len(ff.ET_VALUES), P)]
    ZE = ZG = None
    if family in ff.ADJOINT:
        ZE, ZG = soft_local_adjoint_ref.cotangents(int(rng.integers(1, 2 ** 30)), P, N, M)
    return dict(family=family, B=P, N=N, M=M, variant=c["variant"], theta=theta, A=A, X=X, lens=lens, Et=Et, ZE=ZE, ZG=ZG,
                want_GO=True, want_GX=True, seed=seed, index=0, tag=c["id"], offsets={}, poison_seed=0, mask_on=None, equal=False)


def _sweep_block(c, seed):
    """the main sweeps' classes: the scores of tests/datagen.py, lengths 1 .. N x 1 .. M (what the sweeps' own lengths tests
    give them; every other class a full pair), Et from ET_VALUES, a cotangent Z for the second order"""
    P, N, M = c["P"], c["N"], c["M"]
    rng = np.random.default_rng([seed, len(FAMILIES), N, M, P])
    theta, A = datagen.theta_A(int(rng.integers(1, 2 ** 20)), P, N, M)
    lens = np.stack([rng.integers(1, N + 1, P), rng.integers(1, M + 1, P)], axis=1).astype(np.int32)
    lens[::2] = (N, M)
    lens[1] = (1, 1)
    Et = ff.ET_VALUES[rng.integers(0, len(ff.ET_VALUES), P)]
    Z = datagen.normal(int(rng.integers(1, 2 ** 20)), (P, N, M))
    return dict(family=SWEEP, B=P, N=N, M=M, variant=c["variant"], theta=theta, A=A, lens=lens, Et=Et, Z=Z, tag=c["id"])


def reference(c, blk):
    """the results of the block's P classes: family_fuzz.reference in float64 (the soft families); the hard families' references,
    with the lists as arrays -- states (P, cap, 3) int32 filled with -1 behind the list, counts (P,), last (P, 3): row cap - 1"""
    family = c["family"]
    if family == SWEEP:      # the reference's semantics in float64, every pair over its own slice (tests/parity.py)
        r = parity.oracle_f64(blk["theta"], blk["A"], blk["Et"], blk["Z"], blk["variant"], blk["lens"], threads=8)
        return {k: r[k] for k in ("Vt", "E", "Vtd", "Ed")}
    if family in ff.SOFT:
        r = ff.reference(family, blk)
        if family in ff.ADJOINT:         # the first-order sweep's Vt, which the adjoint pair's launches return too
            r["Vt"] = ff.reference(family.replace("_adjoint", ""), blk)["Vt"]
        return r
    cap = c["N"] + c["M"] + 2
    if family == HARD_AFFINE:
        r = hard_affine_ref.batch(blk["theta"], blk["A"], blk["X"], blk["lens"], blk["Et"], fwd=hard_affine_ref.forward_fast)
        lists, last = r["lists"], r["scratch"]
    else:
        r = ff.reference(family, blk)
        cells = r["cells"]
        lists = cells if family == "hard_local" else r["lists"]
        last = np.array([(len(x), x[0][0], x[0][1]) if x else (0, -1, -1) for x in cells], np.int32)
    states = np.full((c["P"], cap, 3), -1, np.int32)
    for p, rows in enumerate(lists):
        if rows:
            states[p, :len(rows)] = np.array([tuple(x)[:3] for x in rows], np.int32)
    out = {k: r[k] for k in ("Vt", "E", "ends", "GO", "GX") if k in r}
    out.update(states=states, counts=np.array([len(x) for x in lists], np.int32), last=last.astype(np.int32))
    return out


# ---- the harness: torch ops on whatever device the tensors are on; only scalars and failing indices come back ----
def classes(B, P, device):
    return torch.arange(B, device=device) % P


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _where(bad):
    return bad.nonzero().flatten()[:8].tolist()


def _fail(c, what, bad):
    raise AssertionError(f"{c['id']} (B = {c['B']}, P = {c['P']}, {c['size']} bytes a pair, aliases {aliases(c['threshold'], c['size'])}): "
                         f"{what}: {int(bad.sum())} pairs, the first {_where(bad)}")


def _chunks(B, elements):
    step = max(1, COMPARE // max(1, elements))
    return [(lo, min(lo + step, B)) for lo in range(0, B, step)]


def _per_pair(x):
    return x.flatten(1).any(1) if x.dim() > 1 else x


def judge(c, blk, got, want):
    """got: the launch's outputs, torch tensors with B leading -- the soft families: family_fuzz.OUTPUTS and `Vv` (the value-only
    sweep's Vt), either may be missing (a `planes` case has Vv alone); the main sweeps: SWEEP_OUTPUTS of the buffer; the hard
    families: Vt, Vv, E, states, counts, and ends, ends_v, GO, GX where the family has them.  want: reference() of the block.
    Every output of every pair against the first pair of its class as bit patterns; then against the class's reference -- the soft
    families and the main sweeps under tests/parity.py's rules (Vt, Vtd: rel_err, planes: plain abs_err, each <= TOL), zero outside
    the blocks, the hard families bit for bit.  -> the worst errors; a failure raises with the pairs."""
    family, B, P, N, M = c["family"], c["B"], c["P"], c["N"], c["M"]
    dev = next(iter(got.values())).device
    idx = classes(B, P, dev)
    nm = torch.from_numpy(ff.blocks(blk)).to(dev)[idx]
    n, m = nm[:, 0], nm[:, 1]
    rows, cols = torch.arange(N, device=dev)[None, :, None], torch.arange(M, device=dev)[None, None, :]
    worst = {}
    for k, g in got.items():
        assert g.shape[0] == B, (k, tuple(g.shape))
        # every pair against the first pair of its class, bit for bit
        bad = torch.cat([_per_pair(_bits(g[lo:hi]) != _bits(g[:P])[idx[lo:hi]]) for lo, hi in _chunks(B, g[0].numel())])
        if bad.any():
            _fail(c, f"{k} is not the bits of the class's first pair", bad)
    if family in ff.SOFT or family == SWEEP:
        soft = {k: torch.from_numpy(np.asarray(want[k], np.float64)).to(dev) for k in want}
        if "Vv" in got and "Vt" in got and (_bits(got["Vv"]) != _bits(got["Vt"])).any():
            _fail(c, "the value-only sweep's Vt is not the stateful sweep's", _bits(got["Vv"]) != _bits(got["Vt"]))
        for k, g in got.items():
            w = soft["Vt" if k == "Vv" else k]
            if g.dim() == 1:
                err = (g.double() - w[idx]).abs() / w[idx].abs().clamp(min=1.0)
                empty = (n < 1) | (m < 1)
                if (empty & (_bits(g) != 0)).any():
                    _fail(c, f"{k} of an empty pair is not +0", empty & (_bits(g) != 0))
            else:
                err, nonzero, open_ = [], [], []
                forbidden = None
                if family == ff.AFFINE and k in ("GO", "GX"):
                    forbidden = torch.from_numpy(np.isneginf(blk["A" if k == "GO" else "X"])).to(dev)
                for lo, hi in _chunks(B, N * M):
                    i = idx[lo:hi]
                    err.append((g[lo:hi].double() - w[i]).abs().amax((1, 2)))
                    outside = (rows >= n[lo:hi, None, None]) | (cols >= m[lo:hi, None, None])
                    # (the main sweeps' contract is a zero fill: any zero; the families': +0 by bit pattern)
                    nonzero.append((((g[lo:hi] if family == SWEEP else _bits(g[lo:hi])) != 0) & outside).flatten(1).any(1))
                    if forbidden is not None:
                        open_.append(((_bits(g[lo:hi]) != 0) & forbidden[i] & ~outside).flatten(1).any(1))
                err, nonzero = torch.cat(err), torch.cat(nonzero)
                if nonzero.any():
                    _fail(c, f"{k} is not +0 (by bit pattern) outside the pair's block", nonzero)
                if open_ and torch.cat(open_).any():
                    _fail(c, f"{k} is not +0 (by bit pattern) where its gap is forbidden", torch.cat(open_))
            bad = ~(err <= TOL)
            if bad.any():
                _fail(c, f"{k} is over the bound {TOL:g} against float64 (worst {float(err[bad].max()):.3e})", bad)
            worst[k] = float(err.max())
        return worst
    hard = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in want.items()}
    for k, g in got.items():
        if k == "states":
            continue
        w = hard[{"Vv": "Vt", "ends_v": "ends"}.get(k, k)]
        bad = torch.cat([_per_pair(_bits(g[lo:hi]) != _bits(w)[idx[lo:hi]]) for lo, hi in _chunks(B, g[0].numel())])
        if bad.any():
            _fail(c, f"{k} is not the reference's, bit for bit", bad)
    if "states" in got:
        cap = N + M + 2
        for lo, hi in _chunks(B, cap * 3):
            i = idx[lo:hi]
            g = got["states"][lo:hi]
            listed = torch.arange(cap, device=dev)[None, :, None] < hard["counts"][i][:, None, None]
            bad = ((g != hard["states"][i]) & listed).flatten(1).any(1)
            if bad.any():
                _fail(c, "a list row differs from the reference's", torch.cat([torch.zeros(lo, dtype=torch.bool, device=dev), bad]))
            last = g[:, cap - 1] != hard["last"][i]
            if family == "hard":          # the global walk: the number of path cells alone, and nothing for an empty pair
                last = last[:, :1] & ((n[lo:hi] >= 1) & (m[lo:hi] >= 1))[:, None]
            if last.any():
                _fail(c, "the last row differs from the reference's", torch.cat([torch.zeros(lo, dtype=torch.bool, device=dev), last.any(1)]))
    worst["bits"] = 0.0
    return worst


def standin(c, blk, want):
    """a launch that is right, without a GPU: every pair holds its class's reference, rounded to fp32 (CPU torch tensors)"""
    idx = classes(c["B"], c["P"], "cpu")
    if c["family"] == SWEEP:
        return {k: torch.from_numpy(np.asarray(want[k], np.float32))[idx].contiguous() for k in SWEEP_OUTPUTS[c["buffer"]]}
    if c["family"] in ff.SOFT:
        got = {k: torch.from_numpy(np.asarray(want[k], np.float32)) for k in want}
        if c["family"] == ff.AFFINE:      # (the definition leaves -0 or a denormal on a forbidden gap under some Et; the kernels +0)
            got["GO"][torch.from_numpy(np.isneginf(blk["A"]))] = 0.0
            got["GX"][torch.from_numpy(np.isneginf(blk["X"]))] = 0.0
        got = {k: g[idx].contiguous() for k, g in got.items()}
        got["Vv"] = got["Vt"].clone()
        return got
    got = {k: torch.from_numpy(np.ascontiguousarray(want[k]))[idx].contiguous() for k in want if k not in ("last",)}
    got["states"][:, -1] = torch.from_numpy(want["last"])[idx]
    got["Vv"] = got["Vt"].clone()
    if "ends" in got:
        got["ends_v"] = got["ends"].clone()
    return got


def truncated(c, got, key):
    """output `key` of a launch whose offsets into the case's buffer were formed in 32 bits (the threshold's, for the scaled-down
    stand-in): the forward and the backward sweep agree on the wrong address, so a pair beyond the threshold still looks right,
    and the pair its records land on -- an alias distance below it -- shows the output of the pair that overwrote it"""
    out = got[key].clone()
    for b in range(-(-c["threshold"] // c["size"]), c["B"]):
        out[b - aliases(c["threshold"], c["size"])[0]] = got[key][b]
    return out


# ---- the samplers' `states` output: B K cap 3 int32, one list per (pair, sample) ----
# the three samplers: sdp_sample_paths_f32 on the main sweeps' state (csrc/sdp_sample.hip: the lists carry their padding, no end
# tables, no empty sample), the soft local sampler (csrc/sdp_soft_local_sample.hip) and the affine local one
# (csrc/sdp_affine_local_sample.hip: a plane in every row, three counters)
GLOBAL, SOFT_SAMPLER, AFFINE_SAMPLER = "sample", "soft_local_sample", "affine_local_sample"
SAMPLERS = (GLOBAL, SOFT_SAMPLER, AFFINE_SAMPLER)
SAMPLER_BLOCK = {GLOBAL: SWEEP, SOFT_SAMPLER: "soft_local", AFFINE_SAMPLER: ff.AFFINE}      # the family whose block a sampler draws
SAMPLER_STATE = {GLOBAL: "exact", SOFT_SAMPLER: "state", AFFINE_SAMPLER: "state"}
SAMPLER_COUNTERS = {GLOBAL: ("visits",), SOFT_SAMPLER: ("visits",), AFFINE_SAMPLER: ("visits", "opens", "extends")}
SAMPLER_ENDS = {GLOBAL: 0, SOFT_SAMPLER: 2, AFFINE_SAMPLER: 3}          # columns of the `ends` output (0: there is none)
SAMPLER_K = 512                          # samples a pair: the lists of one pair are K cap 12 bytes, 80 % of a 48-byte state
SAMPLER_SEED = 2025
PATTERN = 0x5A5AC3C3                     # what every output holds before the launch (tests/test_affine_local_sample_gpu.py)
GUARD = 1024                             # words of PATTERN in front of and behind every output
CHOSEN = 16                              # pairs whose end cells and walks are held to the restatement and the float64 reference
COUNTERS = SAMPLER_COUNTERS[AFFINE_SAMPLER]
# a walk with a uniform within DELTA of a threshold it was compared with is excluded, at most this share of them (the samplers'
# own GPU tests: tests/test_sample_gpu.py, test_soft_local_sample_gpu.py, test_affine_local_sample_gpu.py)
DELTA = 3e-6
EXCLUDED_CAP = {GLOBAL: 0.05, SOFT_SAMPLER: 0.05, AFFINE_SAMPLER: 0.06}


def sampler_cases():
    """the three samplers' lists across both thresholds: B from B K cap 3 4 bytes, within the samplers' own SDP_E_TOOBIG rule.
    sdp_sample_paths: the packed state and NW at 2^31, the exact state and SW at 2^32"""
    out = []
    N, M = WIDE
    size = SAMPLER_K * (N + M + 2) * 3 * 4
    for kind in SAMPLERS:
        for t, threshold in enumerate(THRESHOLDS):
            B = min_batch(threshold, size)
            buffer = ("packed", "exact")[t] if kind == GLOBAL else "state"
            state = B * pair_bytes(SAMPLER_BLOCK[kind], buffer, N, M)
            peak = state + B * size + 7 * B * N * M * 4 + COMPARE * 8 * 6
            out.append(dict(family=kind, buffer="lists", threshold=threshold, N=N, M=M, B=B, K=SAMPLER_K, P=_prime(aliases(threshold, size)),
                            size=size, bytes=B * size, variant=(ff.NW, ff.SW)[t] if kind == GLOBAL else None, exact=bool(t), peak=peak,
                            id=f"{kind}-lists-2^{threshold.bit_length() - 1}"))
    return tuple(out)


def sampler_small(c, P=67, K=4):
    """the sampler's case scaled down for the CPU stand-in: P classes, 3 P pairs, K samples, the threshold P + P/2 + 0.6 pairs in"""
    size = K * (c["N"] + c["M"] + 2) * 12
    s = dict(c, P=P, B=3 * P, K=K, size=size, bytes=3 * P * size, threshold=size * (P + P // 2) + (size * 3) // 5)
    assert all(d % P for d in aliases(s["threshold"], size)) and layout(s["B"], s["threshold"], size)[1:] == (1, 3 * P - P - P // 2 - 1)
    return s


def sampler_block(c):
    """the block of the sampler's P classes: block() of the family it samples (scores, forbidden gaps, lengths by class)"""
    blk = block(dict(c, family=SAMPLER_BLOCK[c["family"]]))
    blk["definitions"] = {}          # class -> its float64 definition, computed once (_definition)
    return blk


def chosen_pairs(c):
    """the first pair, the last, those either side of and astride each threshold the buffer crosses, and their alias partners"""
    B, size = c["B"], c["size"]
    pairs = [0, B - 1]
    for T in [t for t in THRESHOLDS if t <= c["threshold"]] if c["threshold"] in THRESHOLDS else [c["threshold"]]:
        astride = T // size
        near = [astride - 1, astride, astride + 1]
        pairs += near + [b - a for b in near[1:] for a in aliases(T, size)]
    pairs = sorted({b for b in pairs if 0 <= b < B})
    assert len(pairs) <= CHOSEN, pairs
    rest = [b for b in range(B - 2, 0, -max(1, B // 23)) if b not in pairs]       # (filled up from the rest of the launch)
    return sorted(pairs + rest[:CHOSEN - len(pairs)])


def _sampler_blocks(c, blk):
    """(n, m) of every class as the sampler's kernels take them"""
    import sample_ref
    import soft_local_sample_ref
    clamp = sample_ref.clamp_lens if c["family"] == GLOBAL else soft_local_sample_ref.clamp_lens
    return clamp(blk["lens"], blk["B"], blk["N"], blk["M"])


def _definition(c, blk, p):
    """the float64 definition of class p over its own block, computed once and kept on the block: (Vt, V, q) of
    affine_local_sample_ref._definition / soft_local_ref.forward_wavefront; the global sampler: the oracle's weights (n, m, 3)"""
    if p not in blk["definitions"]:
        n, m = _sampler_blocks(c, blk)[p]
        th, a = blk["theta"][p:p + 1, :n, :m], blk["A"][p:p + 1, :n, :m]
        if n < 1 or m < 1:
            d = None
        elif c["family"] == AFFINE_SAMPLER:
            import affine_local_sample_ref
            d = affine_local_sample_ref._definition(th[0], a[0], blk["X"][p, :n, :m])
        elif c["family"] == SOFT_SAMPLER:
            import soft_local_ref
            Vt, V, q = soft_local_ref.forward_wavefront(th, a)
            d = (Vt[0], np.ascontiguousarray(V[0, 1:-1, 1:-1]), np.ascontiguousarray(q[0, 1:-1, 1:-1]))
        else:
            import sample_ref
            d = sample_ref.inner(parity.oracle.forward(np.ascontiguousarray(th, np.float64), np.ascontiguousarray(a, np.float64), c["variant"])[1])
        blk["definitions"][p] = d
    return blk["definitions"][p]


def reference_walks(c, blk, pairs, tables, seed=SAMPLER_SEED):
    """the sampler's restatement for the pairs `pairs` of the launch (pair b is class b % P, and its uniforms are pair b's).  The
    local samplers: the end cell by the restatement's draw on tables[x] = (cdf (N, M), rows (N + 1,)) -- the launch's own, read
    back --, the plane and the walk by the float64 definition; the global sampler: sample_ref.walk on the float64 oracle's weights.
    -> (states (len(pairs), K, cap, 3), counts, the mask of the rows that are specified, ends or None, margin)"""
    import affine_local_sample_ref as ar
    import sample_ref
    import soft_local_sample_ref as sr
    kind, K, N, M = c["family"], c["K"], c["N"], c["M"]
    cap = N + M + 2
    st, cn = np.zeros((len(pairs), K, cap, 3), np.int32), np.zeros((len(pairs), K), np.int32)
    on, margin = np.zeros((len(pairs), K, cap), bool), np.full((len(pairs), K), np.inf)
    ends = np.full((len(pairs), K, SAMPLER_ENDS[kind]), -1, np.int32) if SAMPLER_ENDS[kind] else None
    for x, b in enumerate(pairs):
        n, m = _sampler_blocks(c, blk)[b % c["P"]]
        for k in range(K):
            if kind == GLOBAL:
                lst, npath, first, margin[x, k] = sample_ref.walk(_definition(c, blk, b % c["P"]), n, m, 2 if c["variant"] else 1, seed, b, k)
                last = (npath, first[0], first[1])
            else:
                us = sample_ref.uniforms(seed, b, k, n + m + 3)
                cdf, rows = tables[x]
                i, j = sr.end_draw(rows, cdf, n, m, us[0], us[1])
                lst = []
                if i >= 0 and kind == AFFINE_SAMPLER:
                    Vt, V, q = _definition(c, blk, b % c["P"])
                    s, pm = ar.plane_draw(V[i, j], Vt, us[2])
                    ends[x, k] = (i, j, s)
                    lst, wm, _ = ar.walk(q[:n, :m], i, j, s, us)
                    margin[x, k] = min(pm, wm)
                elif i >= 0:
                    ends[x, k] = (i, j)
                    lst, margin[x, k] = sr.walk(_definition(c, blk, b % c["P"])[2], i, j, us)
                last = (len(lst), lst[0][0], lst[0][1]) if lst else (0, -1, -1)
            cn[x, k] = len(lst)
            if lst:
                st[x, k, cap - 1 - len(lst):cap - 1] = np.asarray(lst, np.int32)
            st[x, k, cap - 1] = last
            on[x, k, cap - 1 - len(lst):] = True
    return st, cn, on, ends, margin


def judge_walks(c, blk, pairs, got, seed=SAMPLER_SEED):
    """got: numpy arrays of the pairs `pairs` alone -- states (16, K, cap, 3), counts, and for the local samplers ends, cdf, rows.
    The end cells are the restatement's draw on the launch's own tables, every sample; the planes and walks the float64
    reference's, but for walks with a uniform within DELTA of a threshold, at most EXCLUDED_CAP of them (the rules of the
    samplers' own GPU tests) -> (excluded, walks, compared non-empty walks)"""
    tables = [(got["cdf"][x], got["rows"][x]) for x in range(len(pairs))] if c["family"] != GLOBAL else None
    st, cn, on, ends, margin = reference_walks(c, blk, pairs, tables, seed)
    same = (got["counts"] == cn) & ((got["states"] == st) | ~on[..., None]).all(axis=(2, 3))
    if ends is not None:
        assert np.array_equal(got["ends"][..., :2], ends[..., :2]), \
            f"{c['id']}: end cells differ from the stated draw on the device tables at (chosen pair, sample) " \
            f"{np.argwhere((got['ends'][..., :2] != ends[..., :2]).any(-1))[:4].tolist()} of pairs {pairs}"
        same &= (got["ends"] == ends).all(axis=2)
    keep = margin >= DELTA
    compared = int((keep & np.isfinite(margin)).sum())
    assert not (keep & ~same).any(), f"{c['id']}: walks differ from the float64 reference at (chosen pair, sample) " \
                                     f"{np.argwhere(keep & ~same)[:4].tolist()} of pairs {pairs}"
    assert int((~keep).sum()) <= EXCLUDED_CAP[c["family"]] * keep.size and compared > 0, (int((~keep).sum()), keep.size, compared)
    return int((~keep).sum()), keep.size, compared


def judge_lists(c, blk, got):
    """every (pair, sample) list of the launch, on the device: got = states (B, K, cap, 3), counts (B, K), the sampler's counters
    (B, N, M) and, where it has them, ends (B, K, 2 or 3), int32 torch tensors.  A count within the capacity; the rows in front
    of a list still PATTERN; every listed cell inside the pair's block; the counters a recount (scatter_add) of the path cells
    the launch listed.  The local samplers: the last row (count, i, j of the first cell), (0, -1, -1) and ends of -1 for an empty
    sample, the first cell in state m, the last row of the list the end cell (and plane), every step the one its state names.
    sdp_sample_paths: the last row (path cells, i, j of the first of them) with no more path cells than rows, the list from
    (0, 0) to the pair's corner, every padding row followed by the step its state names and every path row entered by it"""
    kind, B, K, N, M, P = c["family"], c["B"], c["K"], c["N"], c["M"], c["P"]
    cap = N + M + 2
    dev = got["states"].device
    assert tuple(got["states"].shape) == (B, K, cap, 3) and tuple(got["counts"].shape) == (B, K)
    idx = classes(B, P, dev)
    nm = torch.tensor(_sampler_blocks(c, blk), device=dev)[idx]
    steps = torch.tensor([[1, 0], [1, 1], [0, 1]], dtype=torch.int32, device=dev)
    r = torch.arange(cap - 1, device=dev)[None, None, :]

    def fail(what, bad, lo):
        where = (bad.nonzero()[:6] + torch.tensor([lo] + [0] * (bad.dim() - 1), device=dev)).tolist()
        raise AssertionError(f"{c['id']} (B = {B}, K = {K}, {c['size']} bytes a pair, aliases {aliases(c['threshold'], c['size'])}): "
                             f"{what} at (pair, sample) {where}")

    for lo, hi in _chunks(B, K * cap * 3 * 2):
        st, cn = got["states"][lo:hi], got["counts"][lo:hi].long()
        n, m = nm[lo:hi, 0, None, None], nm[lo:hi, 1, None, None]
        bad = (cn < 0) | (cn > cap - 1)
        if bad.any():
            fail("a count is outside the capacity", bad, lo)
        body, last = st[:, :, :cap - 1], st[:, :, cap - 1]
        on = r >= (cap - 1 - cn)[..., None]
        bad = ((body != PATTERN).any(-1) & ~on).any(-1)
        if bad.any():
            fail("rows in front of a list no longer hold the prefill pattern", bad, lo)
        i, j, s = body[..., 0], body[..., 1], body[..., 2]
        bad = (on & ((i < 0) | (i >= n) | (j < 0) | (j >= m) | (s < 0) | (s > 2))).any(-1)
        if bad.any():
            fail("a listed cell lies outside the pair's block or names no state", bad, lo)
        both = on[:, :, 1:] & on[:, :, :-1]
        step = body[:, :, 1:, :2] - body[:, :, :-1, :2]
        empty = cn == 0
        first = body.gather(2, (cap - 1 - cn).clamp(max=cap - 2)[..., None, None].expand(-1, -1, 1, 3)).squeeze(2)
        if kind == GLOBAL:
            npath = last[..., 0].long()
            bad = (npath < 0) | (npath > cn)
            if bad.any():
                fail("the last row counts more path cells than the list has rows", bad, lo)
            path = r >= (cap - 1 - npath)[..., None]
            head = body.gather(2, (cap - 1 - npath).clamp(max=cap - 2)[..., None, None].expand(-1, -1, 1, 3)).squeeze(2)
            corner = torch.stack([n[:, 0, 0] - 1, m[:, 0, 0] - 1], -1)[:, None, :].to(torch.int32)
            bad = (~empty & (first[..., :2] != 0).any(-1)) | ((npath > 0) & ((last[..., 1:] != head[..., :2]).any(-1)
                                                                              | (body[:, :, cap - 2, :2] != corner).any(-1)))
            if bad.any():
                fail("the last row, the list's first cell or its corner disagree with the list and its count", bad, lo)
            pad = on & ~path
            bad = ((step != steps[s[:, :, :-1].clamp(0, 2).long()]).any(-1) & both & pad[:, :, :-1]).any(-1) | (pad & (s == 1)).any(-1) \
                | ((step != steps[s[:, :, 1:].clamp(0, 2).long()]).any(-1) & path[:, :, 1:] & path[:, :, :-1]).any(-1)
            if bad.any():
                fail("a step is not the one its state names", bad, lo)
        else:
            en = got["ends"][lo:hi]
            path = on
            want_last = torch.stack([cn, first[..., 0].long(), first[..., 1].long()], -1)
            want_last[empty] = torch.tensor([0, -1, -1], device=dev)
            bad = (last != want_last).any(-1) | (empty & (en != -1).any(-1)) \
                | (~empty & ((first[..., 2] != 1) | (body[:, :, cap - 2, :en.shape[-1]] != en).any(-1)))
            if bad.any():
                fail("the last row, the first cell's state or the end cell disagree with the list and its count", bad, lo)
            bad = ((step != steps[s[:, :, 1:].clamp(0, 2).long()]).any(-1) & both).any(-1)
            if bad.any():
                fail("a step is not the one its state names", bad, lo)
        # the recount: the cells are inside their blocks (held above), so every index is inside its plane
        flat = (torch.arange(hi - lo, device=dev)[:, None, None] * N + i.long()) * M + j.long()
        gap, same = torch.zeros_like(on), torch.zeros_like(on)
        gap[:, :, 1:] = both & (s[:, :, 1:] != 1)
        same[:, :, 1:] = s[:, :, 1:] == s[:, :, :-1]
        for key, mask in (("visits", path), ("opens", gap & ~same), ("extends", gap & same)):
            if key in SAMPLER_COUNTERS[kind]:
                own = torch.zeros((hi - lo) * N * M, dtype=torch.int32, device=dev)
                own.scatter_add_(0, flat[mask], torch.ones(int(mask.sum()), dtype=torch.int32, device=dev))
                bad = (own.view(hi - lo, N, M) != got[key][lo:hi]).flatten(1).any(1)
                if bad.any():
                    fail(f"{key} is not the recount of the lists the launch wrote", bad, lo)


def sampler_standin(c, blk, seed=SAMPLER_SEED):
    """a launch of the sampler that is right, without a GPU: the restatement's tables in fp32, its draws and the float64 walks of
    every pair, in the kernel's formats over PATTERN -> dict of int32 / fp32 CPU torch tensors (cdf, rows: of all pairs)"""
    import affine_local_sample_ref as ar
    import soft_local_sample_ref as sr
    kind, B, N, M, P = c["family"], c["B"], c["N"], c["M"], c["P"]
    cap = N + M + 2
    tables = []
    for p in range(P if kind != GLOBAL else 0):
        n, m = _sampler_blocks(c, blk)[p]
        cdf, rows = np.zeros((N, M), np.float32), np.zeros(N + 1, np.float32)
        if n:
            Vt, V, q = _definition(c, blk, p)
            cdf[:n, :m], rows[:n + 1] = (ar if kind == AFFINE_SAMPLER else sr).tables32(V, Vt)
        tables.append((cdf, rows))
    pairs = list(range(B))
    st, cn, on, ends, _ = reference_walks(c, blk, pairs, [tables[b % P] for b in pairs] if tables else None, seed)
    st[~on] = np.int32(PATTERN)
    got = {"states": st, "counts": cn}
    if ends is not None:
        got["ends"] = ends
    for key in SAMPLER_COUNTERS[kind]:
        got[key] = np.zeros((B, N, M), np.int32)
    for b in range(B):
        for k in range(c["K"]):
            rows = st[b, k, cap - 1 - (st[b, k, cap - 1, 0] if kind == GLOBAL else cn[b, k]):cap - 1]
            for t, (i, j, s) in enumerate(rows):
                got["visits"][b, i, j] += 1
                if kind == AFFINE_SAMPLER and s != 1:
                    got["extends" if rows[t - 1][2] == s else "opens"][b, i, j] += 1
    if tables:
        got["cdf"] = np.stack([tables[b % P][0] for b in pairs])
        got["rows"] = np.stack([tables[b % P][1] for b in pairs])
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in got.items()}
