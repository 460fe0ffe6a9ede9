"""A seeded shape fuzz for the seven kernel families on the strip schedule (64-row strips, 32-step chunks, up to 8 waves, the LDS
boundary ring, progress keys): the generator of the cases and the harness that judges a run.  TESTS ONLY, no GPU here: the CPU
test (tests/test_family_fuzz.py) and the GPU test (tests/test_family_fuzz_gpu.py) see the same cases.

    hard, hard_local                    csrc/sdp_hard.hip          bit identity with hard_ref.batch / hard_local_ref.batch
    soft_local, soft_local_adjoint      csrc/sdp_soft_local*.hip   tests/parity.py's rules against the float64 definition
    sparsemax, sparsemax_adjoint        csrc/sdp_sparsemax*.hip    the same
    affine_local                        csrc/sdp_affine_local.hip  the same, and +0 gradients on forbidden openings / extensions

case(family, seed, index) draws one case: a shape class, a variant, a score family, per-pair lengths that run past both ends of
[0, N] x [0, M], Et, cotangents, and where every float input lies -- a plane offset of 0 .. 3 floats inside a buffer of NaN, +-inf
and +-1e30, the same poison in every pair's padding (placed()).  The affine family has a third input, X = gap_extend (A is its
gap_open), masks on either or both gap planes, and backward calls without GO or without GX.  check(family, case, got) applies the
rules and dumps a failing case to DUMP_DIR; admitted(family, case) is the project's admission rule for the soft families: a case
is compared only where the definition restated in plain fp32 (the float32 wavefront form of the same reference module) stays
within TOL / 4 of its float64 run on every output -- computed from the references alone.

The seed: DEFAULT_SEED, or SDP_FAMILY_FUZZ_SEED.  SDP_FAMILY_FUZZ_CASES multiplies every family's count (a deeper run).
SDP_FUZZ_DUMP_DIR: where failing cases go (default: fuzz_failures/ in the repository root)."""
import os

import numpy as np

import affine_local_ref
import hard_local_ref
import hard_ref
import soft_local_adjoint_ref
import soft_local_ref
import sparsemax_adjoint_ref
import sparsemax_ref
from parity import ROOT, TOL, abs_err, rel_err

DEFAULT_SEED = 6700417
SEED = int(os.environ.get("SDP_FAMILY_FUZZ_SEED", 0)) or DEFAULT_SEED
MULTIPLIER = max(1, int(os.environ.get("SDP_FAMILY_FUZZ_CASES", 0) or 1))
NW, SW = 0, 1
# (a family's index seeds its generator: a new family goes at the end)
FAMILIES = ("hard", "hard_local", "soft_local", "soft_local_adjoint", "sparsemax", "sparsemax_adjoint", "affine_local")
SOFT = ("soft_local", "soft_local_adjoint", "sparsemax", "sparsemax_adjoint", "affine_local")
ADJOINT = ("soft_local_adjoint", "sparsemax_adjoint")
AFFINE = "affine_local"
VARIANTS = {f: ((None,) if f.startswith("soft_local") or f == AFFINE else (NW, SW)) for f in FAMILIES}
# cases per family (all variants together; a test of one variant runs the cases that drew it), chosen so that every GPU test takes
# a few seconds -- the numpy references dominate -- and that the admission figures of tests/test_family_fuzz.py, which runs every
# soft case's references twice on a CPU, stay affordable.  Measured on the MI355X host, seconds per test (NW and SW where there are two):
COUNTS = {"hard": 200,                 # 0.9 s and 0.9 s
          "hard_local": 200,           # 0.7 s and 0.6 s
          "soft_local": 100,           # 1.9 s
          "soft_local_adjoint": 80,    # 3.3 s
          "sparsemax": 200,            # 2.1 s and 1.9 s
          "sparsemax_adjoint": 100,    # 2.4 s and 2.1 s
          "affine_local": 100}         # 2.5 s and 2.4 s: two tests of 50 consecutive cases (PARTS), 4.9 s in one
ADMISSION = TOL / 4
CAP = 0.10                            # of all cases of a family, at most this share may fail admission
SAFE = ("unit", "drift", "floor")     # score families none of whose cases may fail admission
# the score families of every kernel family's draw and their weights.  `model` and `steep` are where admission leaves cases out
# (tests/test_family_fuzz.py has the measured figures); a score family that pushed a kernel family over CAP is not drawn there.
SCORES = {"hard": (("ties", 0.5), ("continuous", 0.5)),
          "hard_local": (("ties", 0.4), ("floors", 0.4), ("continuous", 0.2)),
          "soft_local": (("floor", 0.3), ("drift", 0.3), ("model", 0.2), ("steep", 0.2)),
          "soft_local_adjoint": (("floor", 0.45), ("drift", 0.45), ("model", 0.1)),     # steep: 13 of 22 left out
          "sparsemax": (("unit", 0.3), ("drift", 0.3), ("model", 0.2), ("steep", 0.2)),
          "sparsemax_adjoint": (("unit", 0.85), ("model", 0.15)),                       # steep: 7 of 24; drift: not safe here
          "affine_local": (("floor", 0.3), ("drift", 0.3), ("model", 0.2), ("steep", 0.2))}
# the shape classes: the smallest shapes at which the schedule can still go wrong.  Six of them take turns, four draws each in
# every 25 cases, and the twenty-fifth is the crowd (more pairs than CUs), so that a list of 25 cases has met them all.
CLASSES = ("thin_wide", "thin_tall", "strips", "strip_edge", "many_small", "free", "crowd")
_TURNS = CLASSES[:6] * 4 + ("crowd",)
STRIP, CHUNK = 64, 32
CHUNK_EDGES = ((1, 2), (33, 34), (65, 66))       # the chunk count (tests/strip_schedule.py: chunks) changes between the two
ET_VALUES = np.array([-2.5, -1.0, 0.0, 0.5, 1.0], np.float32)
POISON = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)
PAD = 64                                          # floats of poison in front of and behind every input
INPUTS = ("theta", "A", "ZE", "ZG", "X")             # X: gap_extend of the affine family (A is its gap_open); None elsewhere
MASKED = ("O", "X", "both")                      # the affine family: the gap planes a case's mask falls on
# where a failing case is dumped: SDP_FUZZ_DUMP_DIR, or fuzz_failures/ in the repository root (git-ignored)
DUMP_DIR = os.environ.get("SDP_FUZZ_DUMP_DIR") or os.path.join(ROOT, "fuzz_failures")


def count(family):
    return COUNTS[family] * MULTIPLIER


def continuous_scores(seed, B, N, M):
    from test_hard_gpu import continuous_scores as f
    return f(seed, B, N, M)


def _scores(family, name, seed, B, N, M):
    if family in ("hard", "hard_local"):
        if name == "ties":       # hard local: negative on average, so that alignments stay local (tests/test_hard_local_gpu.py)
            return hard_ref.quarter_scores(seed, B, N, M, -1.0, 1.0 if family == "hard" else 0.5)
        return hard_local_ref.floor_scores(seed, B, N, M) if name == "floors" else continuous_scores(seed, B, N, M)
    if family.startswith("soft_local"):
        return soft_local_ref.family(name, seed, B, N, M)
    if family == AFFINE:
        return affine_local_ref.inputs(name, seed, B, N, M)
    return sparsemax_ref.family(name, seed, B, N, M)


def _between(rng, lo, hi):
    return int(rng.integers(lo, hi + 1))


def _shape(rng, cls, index):
    if cls == "thin_wide":
        return _between(rng, 1, 4), _between(rng, 1, 6), _between(rng, 1, 200)
    if cls == "thin_tall":
        return _between(rng, 1, 4), _between(rng, 1, 200), _between(rng, 1, 6)
    if cls == "strips":          # two, three or four strips with equal weight (four: 193 .. 200 rows)
        k = _between(rng, 2, 4)
        return _between(rng, 1, 3), _between(rng, STRIP * (k - 1) + 1, min(STRIP * k, 200)), _between(rng, 17, 200)
    if cls == "strip_edge":      # around one strip; of six such cases in a row four sit on the two sides of the chunk edges
        turn = (index // len(_TURNS)) * 4 + (index % len(_TURNS)) // 6
        M = (33, 34, 65, 66)[turn % 6] if turn % 6 < 4 else _between(rng, 28, 100)
        return _between(rng, 1, 3), _between(rng, 60, 70), M
    if cls == "many_small":
        return _between(rng, 1, 40), _between(rng, 1, 70), _between(rng, 1, 70)
    if cls == "crowd":
        return 300, _between(rng, 1, 12), _between(rng, 1, 12)
    return _between(rng, 1, 5), _between(rng, 1, 200), _between(rng, 1, 200)


def case(family, seed, index):
    """-> the case `index` of `family` under `seed`, a dict: the same whenever and wherever it is asked for.  theta, A, ZE, ZG are
    the clean (B, N, M) fp32 tensors the references take (ZE or ZG None: absent); placed() puts them among the poison.  The
    affine family: A is gap_open, X gap_extend (None elsewhere), equal: X = O, mask_on: the planes the mask fell on, want_GO and
    want_GX: the outputs its backward call asks for."""
    assert family in FAMILIES
    rng = np.random.default_rng([int(seed), FAMILIES.index(family), int(index)])
    cls = _TURNS[index % len(_TURNS)]
    B, N, M = _shape(rng, cls, index)
    variant = None if VARIANTS[family] == (None,) else int(rng.integers(0, 2))
    names, weights = zip(*SCORES[family])
    score = str(rng.choice(names, p=weights))
    theta, A, *rest = _scores(family, score, int(rng.integers(1, 2 ** 31 - 1)), B, N, M)
    A = A.copy()
    X, equal = None, False
    if family == AFFINE:                 # (every draw of this family alone stands in a branch of its own: the others' cases stay)
        equal = bool(rng.integers(0, 8) == 0)      # X = O: the soft local operator (before the masks, which fall where they fall)
        X = A.copy() if equal else rest[0].copy()
    mask = mask_on = None
    # the affine family's coverage asks for the finite mask, which one masked case in ten leaves out of one list in six (the
    # default seed's first is case 209): there one `strips` case in every fifty has it whatever is drawn
    forced = family == AFFINE and index % 50 == 14
    if rng.integers(0, 6) == 0 or forced:   # forbidden gaps; for the soft families one such case in ten uses the finite mask instead
        mask = "-1e30" if family in SOFT and (rng.integers(0, 10) == 0 or forced) else "-inf"
        value = -np.inf if mask == "-inf" else np.float32(-1e30)
        if family == AFFINE:             # on the openings only, on the extensions only, or on both with independent cells
            mask_on = MASKED[int(rng.integers(0, 3))]
            if mask_on != "X":
                A[rng.random(A.shape) < 0.2] = value
            if mask_on != "O":
                X[rng.random(X.shape) < 0.2] = value
        else:
            A[rng.random(A.shape) < 0.2] = value
    lens = None
    if rng.integers(0, 2):
        lens = np.stack([rng.integers(-2, N + 4, B), rng.integers(-2, M + 4, B)], axis=1).astype(np.int32)
        lens[int(rng.integers(0, B))] = (N, M)
    Et = np.ones(B, np.float32) if rng.integers(0, 2) else ET_VALUES[rng.integers(0, len(ET_VALUES), B)]
    ZE = ZG = None
    if family in ADJOINT:
        ZE, ZG = soft_local_adjoint_ref.cotangents(int(rng.integers(1, 2 ** 31 - 1)), B, N, M)
        absent = int(rng.integers(0, 4))     # one case in four without ZG, one in four without ZE
        if absent == 0:
            ZG = None
        elif absent == 1:
            ZE = None
    want_GO = want_GX = True
    if family == AFFINE:
        absent = int(rng.integers(0, 4))     # one case in four without GO, one in four without GX
        want_GO, want_GX = absent != 0, absent != 1
    offsets = {k: int(rng.integers(0, 4)) for k in INPUTS[:4]}
    if family == AFFINE:
        offsets["X"] = int(rng.integers(0, 4))
    name = {None: "", NW: " nw", SW: " sw"}[variant]
    tag = (f"{family} case {index} seed {seed}: {cls} {B}x{N}x{M}{name} {score}" + (" X=O" if equal else "")
           + (f" A={mask}" if mask else "") + (f" on {mask_on}" if mask_on else "")
           + (" lens" if lens is not None else "") + ("" if ZE is not None or family not in ADJOINT else " ZE=NULL")
           + ("" if ZG is not None or family not in ADJOINT else " ZG=NULL") + ("" if want_GO else " GO=NULL")
           + ("" if want_GX else " GX=NULL") + f" offsets {tuple(offsets.values())}")
    return dict(family=family, seed=int(seed), index=int(index), cls=cls, B=B, N=N, M=M, variant=variant, score=score, mask=mask,
                theta=theta, A=A, lens=lens, Et=Et, ZE=ZE, ZG=ZG, offsets=offsets, poison_seed=int(rng.integers(1, 2 ** 31 - 1)), tag=tag,
                X=X, equal=equal, mask_on=mask_on, want_GO=want_GO, want_GX=want_GX)


def cases(family, seed=None, n=None, variant="all", part=None):
    """the first `n` cases of a family (default: count(family)) under `seed` (default: SEED), those of one variant if asked;
    part = (k, of): the k-th of `of` runs of consecutive cases of that list (parts(): the affine family's two GPU tests)"""
    n = count(family) if n is None else n
    lo, hi = (0, n) if part is None else (part[0] * n // part[1], (part[0] + 1) * n // part[1])
    for index in range(lo, hi):
        c = case(family, SEED if seed is None else seed, index)
        if variant == "all" or c["variant"] == variant:
            yield c


PARTS = {AFFINE: 2}      # families whose list is split over several GPU tests, so that each takes a few seconds


def parts(family):
    """-> the `part` arguments of a family's GPU tests: (None,) or the runs of consecutive cases its list is split into"""
    return tuple((k, PARTS[family]) for k in range(PARTS[family])) if family in PARTS else (None,)


def blocks(c):
    """-> (B, 2) every pair's (n, m): the lengths clamped to [0, N] x [0, M] as the kernels' min(max(., 0), N) clamps them"""
    if c["lens"] is None:
        return np.tile(np.array([[c["N"], c["M"]]], np.int64), (c["B"], 1))
    return np.clip(c["lens"].astype(np.int64), 0, [c["N"], c["M"]])


def placed(c, key):
    """-> (buffer, start): input `key` of the case as the device sees it -- a flat fp32 buffer of poison with the tensor at
    [start, start + B N M), start = PAD + the case's plane offset for it, and with lengths the poison in every pair's padding too"""
    x = c[key]
    rng = np.random.default_rng([c["poison_seed"], INPUTS.index(key)])
    start = PAD + c["offsets"][key]
    buf = POISON[rng.integers(0, len(POISON), x.size + 2 * PAD + 4)]
    x = x.copy()
    if c["lens"] is not None:
        fill = POISON[rng.integers(0, len(POISON), x.shape)]
        for b, (n, m) in enumerate(blocks(c)):
            x[b, n:, :] = fill[b, n:, :]
            x[b, :, m:] = fill[b, :, m:]
    buf[start:start + x.size] = x.reshape(-1)
    return buf, start


# ---- the references ----
OUTPUTS = {"soft_local": ("Vt", "E", "G"), "sparsemax": ("Vt", "E", "G"), "soft_local_adjoint": ("Vtd", "Ed", "Gd"),
           "sparsemax_adjoint": ("Vtd", "Ed", "Gd"), "affine_local": ("Vt", "E", "GO", "GX")}


def asked(c):
    """-> the outputs the case's calls return: all of the family's, less the GO or GX an affine case does not ask for"""
    return tuple(k for k in OUTPUTS[c["family"]] if c.get("want_" + k, True))


def reference(family, c, dtype=np.float64):
    """the definition's results for a case.  The soft families: the wavefront form of the family's reference module in `dtype`
    (float64: the yardstick, held to the loops over cells at 1e-12 by that module's CPU test; float32: plain fp32 arithmetic, for
    admission).  The hard families: hard_ref.batch / hard_local_ref.batch through their forward_fast (held to the loops bit for
    bit), on the clamped lengths."""
    th, a, v, lens, Et = c["theta"], c["A"], c["variant"], c["lens"], c["Et"]
    with np.errstate(all="ignore"):
        if family == "hard":
            return hard_ref.batch(th, a, v, None if lens is None else blocks(c), Et, fwd=hard_ref.forward_fast)
        if family == "hard_local":
            return hard_local_ref.batch(th, a, v, None if lens is None else blocks(c), Et, fwd=hard_local_ref.forward_fast)
        if family == "soft_local":
            r = soft_local_ref.batch_wavefront(th, a, lens, Et, dtype)
        elif family == "sparsemax":
            r = sparsemax_ref.batch_wavefront(th, a, v, lens, Et, dtype)
        elif family == AFFINE:
            r = affine_local_ref.batch_wavefront(th, a, c["X"], lens, Et, dtype)
        elif family == "soft_local_adjoint":
            r = soft_local_adjoint_ref.batch(th, a, c["ZE"], c["ZG"], lens, Et, dtype=dtype)
        else:
            r = sparsemax_adjoint_ref.batch(th, a, c["ZE"], c["ZG"], v, lens, Et, dtype=dtype)
    return {k: r[k] for k in OUTPUTS[family]}


def errors(family, got, want, keys=None):
    """tests/parity.py's figures for a soft family: rel_err on Vt / Vtd, plain abs_err on the planes (the affine family:
    affine_local_ref.errors, the same); each must be <= TOL.  keys: the outputs to judge (default: all of the family's)"""
    return {k: (rel_err if k in ("Vt", "Vtd") else abs_err)(got[k], want[k]) for k in (OUTPUTS[family] if keys is None else keys)}


def admitted(family, c, want=None):
    """the admission rule -> (compared or left out, the fp32 restatement's distances from float64), on all of the family's outputs
    whichever the case asks for"""
    assert family in SOFT
    want = reference(family, c) if want is None else want
    e = errors(family, reference(family, c, np.float32), want)
    finite = all(np.isfinite(want[k]).all() for k in want)
    return finite and all(np.isfinite(v) and v <= ADMISSION for v in e.values()), e


# ---- the harness ----
def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def dump(c, why):
    """the failing case to DUMP_DIR (commit it under tests/golden/ with a test of its own) -> the message of the failure"""
    os.makedirs(DUMP_DIR, exist_ok=True)
    path = os.path.join(DUMP_DIR, f"family_fuzz_{c['family']}_seed{c['seed']}_case{c['index']}.npz")
    z0 = np.zeros(0, np.float32)
    np.savez(path, theta=c["theta"], A=c["A"], Et=c["Et"], ZE=z0 if c["ZE"] is None else c["ZE"], ZG=z0 if c["ZG"] is None else c["ZG"],
             lens=np.zeros(0, np.int32) if c["lens"] is None else c["lens"], variant=-1 if c["variant"] is None else c["variant"],
             offsets=np.array([c["offsets"][k] for k in INPUTS if k in c["offsets"]]), seed=c["seed"], index=c["index"],
             poison_seed=c["poison_seed"], X=z0 if c["X"] is None else c["X"], mask_on=c["mask_on"] or "", want_GO=c["want_GO"],
             want_GX=c["want_GX"])
    return f"{c['tag']}: {why}; case dumped to {path}"


def _fail(c, why):
    raise AssertionError(dump(c, why))


def _check_soft(family, c, got, want):
    keys = asked(c)
    for k in OUTPUTS[family]:                # what was asked for is there, and nothing else
        if (got.get(k) is not None) != (k in keys):
            _fail(c, f"{k} is {'missing' if k in keys else 'there though not asked for'}")
    errs = errors(family, got, want, keys)
    if not all(np.isfinite(v) and v <= TOL for v in errs.values()):
        _fail(c, "over the bound %g: %s" % (TOL, " ".join(f"{k}={v:.3e}" for k, v in errs.items())))
    for k in keys[1:]:                       # exact +0, by bit pattern, outside every pair's block
        bits = _bits(got[k])
        for b, (n, m) in enumerate(blocks(c)):
            outside = np.ones((c["N"], c["M"]), bool)
            outside[:n, :m] = False
            if bits[b][outside].any():
                _fail(c, f"{k} of pair {b} is not +0 outside its {n} x {m} block: {int((bits[b][outside] != 0).sum())} words")
    for b, (n, m) in enumerate(blocks(c)):   # an empty pair: Vt = +0 (include/sdp.h)
        if (n < 1 or m < 1) and _bits(got[OUTPUTS[family][0]])[b] != 0:
            _fail(c, f"{OUTPUTS[family][0]} of the empty pair {b} is not +0")
    if family == AFFINE:                     # a forbidden opening / extension: its gradient is +0 by bit pattern inside the block
        for k, plane in (("GO", c["A"]), ("GX", c["X"])):       # too, whatever the sign of Et (tests/test_affine_local_gpu.py)
            if k in keys:
                for b, (n, m) in enumerate(blocks(c)):
                    words = _bits(got[k])[b, :n, :m][np.isneginf(plane[b, :n, :m])]
                    if words.any():
                        _fail(c, f"{k} of pair {b} is not +0 where its gap is forbidden: {int((words != 0).sum())} words")
    return errs


def _check_hard(family, c, got, want):
    local = family == "hard_local"
    if not np.array_equal(_bits(got["Vt"]), _bits(want["Vt"])):
        _fail(c, f"Vt differs: {got['Vt']} against {want['Vt']}")
    if local and not np.array_equal(got["ends"], want["ends"]):
        _fail(c, f"ends differ: {got['ends'].tolist()} against {want['ends'].tolist()}")
    if not np.array_equal(_bits(got["E"]), _bits(want["E"])):
        _fail(c, f"E differs at {np.argwhere(_bits(got['E']) != _bits(want['E']))[:5].tolist()}")
    states, counts = got["states"], got["counts"]
    for b, (n, m) in enumerate(blocks(c)):
        cells = want["cells"][b]
        lst = cells if local else want["lists"][b]
        if counts[b] != len(lst):
            _fail(c, f"pair {b}: {counts[b]} list rows against {len(lst)}")
        if [tuple(r) for r in states[b, :counts[b]].tolist()] != [tuple(r) for r in lst]:
            _fail(c, f"pair {b}: the list differs")
        if local:                            # the last row: the number of path cells and the first of them
            last = (len(cells), cells[0][0], cells[0][1]) if cells else (0, -1, -1)
            if tuple(states[b, -1].tolist()) != last:
                _fail(c, f"pair {b}: the last row is {states[b, -1].tolist()}, not {last}")
        elif n >= 1 and m >= 1 and states[b, -1, 0] != len(cells):      # (an empty pair gets counts = 0 and nothing else)
            _fail(c, f"pair {b}: the last row counts {states[b, -1, 0]} path cells, not {len(cells)}")
    return {"bits": 0.0}


def check(family, c, got, want=None):
    """got: dict of numpy arrays, what the engine returned for the case -- Vt, E, G (the first-order soft families), Vt, E, GO, GX
    (the affine family; a GO or GX not asked for: None or missing), Vtd, Ed, Gd (the adjoint pairs), Vt, E, states, counts and for
    hard_local ends (the hard families); "Vv" (and "ends_v"): the value-only sweep's, which must be the stateful sweep's bit for bit.  -> the errors; a failure raises with the case dumped."""
    want = reference(family, c) if want is None else want
    errs = (_check_soft if family in SOFT else _check_hard)(family, c, got, want)
    if "Vv" in got and not np.array_equal(_bits(got["Vv"]), _bits(got["Vt"])):
        _fail(c, "the value-only sweep's Vt is not the stateful sweep's")
    if "ends_v" in got and not np.array_equal(got["ends_v"], got["ends"]):
        _fail(c, "the value-only sweep's ends are not the stateful sweep's")
    return errs


# ---- what a list of cases reaches ----
def coverage(family, cs):
    """-> dict of what the cases reach: shape classes, strip counts and effective column counts of the pairs that run, kinds of
    lengths, plane offsets, variants, masks (the affine family: and the planes they fall on), absent cotangents or outputs, how many
    cases have X = O"""
    cov = dict(classes=set(), strips=set(), cols=set(), lengths=set(), offsets=set(), variants=set(), masks=set(), masked=set(),
               absent=set(), scores={}, batch=set(), equal=0)
    for c in cs:
        cov["classes"].add(c["cls"])
        cov["variants"].add(c["variant"])
        cov["masks"].add(c["mask"])
        cov["batch"].add(c["B"])
        cov["scores"][c["score"]] = cov["scores"].get(c["score"], 0) + 1
        keys = [k for k in INPUTS if c[k] is not None]
        cov["offsets"].update((k, c["offsets"][k]) for k in keys)
        cov["absent"].update(k for k in ("ZE", "ZG") if family in ADJOINT and c[k] is None)
        cov["absent"].update(k for k in OUTPUTS.get(family, ()) if k not in asked(c))
        cov["masked"].add(c["mask_on"])
        cov["equal"] += bool(c["equal"])
        for n, m in blocks(c):
            if n >= 1 and m >= 1:
                cov["strips"].add(int((n + STRIP - 1) // STRIP))
                cov["cols"].add(int(m))
        if c["lens"] is not None:
            ln = c["lens"]
            cov["lengths"].update(k for k, hit in (("zero", (ln == 0).any()), ("negative", (ln < 0).any()),
                                                   ("over", (ln[:, 0] > c["N"]).any() or (ln[:, 1] > c["M"]).any())) if hit)
            if len({(int(n + STRIP - 1) // STRIP, int(m + STRIP + CHUNK - 2) // CHUNK) for n, m in blocks(c) if n >= 1 and m >= 1}) > 1:
                cov["lengths"].add("mixed")     # different strip and chunk counts side by side in one launch
    return cov
