"""CPU: the C-ABI library loads without a GPU and exports exactly what include/sdp.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()  # hipcc cross-compiles for gfx950 without a GPU
    return _lib.load()


def _declared(experiments=False):
    src = open(os.path.join(ROOT, "include", "sdp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    exp = re.findall(r"#ifdef SDP_EXPERIMENTS(.*?)#endif", src, flags=re.S)
    if experiments:
        src = "".join(exp)
    else:
        src = re.sub(r"#ifdef SDP_EXPERIMENTS.*?#endif", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sdp_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    from deepblast_amd import _lib
    names = _declared()
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/sdp.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert sorted(_lib.SIGNATURES) == names
    # the shipped library has no experiment switches (no wrong-results knob reachable through the ABI)
    for n in _declared(experiments=True):
        assert n in _lib.EXPERIMENT_SIGNATURES and not hasattr(lib, n), n
    for gone in ("sdp_set_waves", "sdp_probe"):
        assert not hasattr(lib, gone)


def test_version_and_limits(lib):
    assert lib.sdp_version() == 106
    assert lib.sdp_max_cols() == 2048  # reference GPU path: max_cols = 2048 (nw_cuda.py:11)


def test_state_bytes(lib):
    # Q: 5 B (two 20-bit weights) per cell of the skewed, padded layout; Qd: float2 per cell (+ a tail for the launch order of
    # variable-length batches: B ints, 256-byte granules)
    # ... and, for pairs of more than four strips, the bridge rows between the parts a pair may be cut into: per pair
    # (ceil(strips / 4) - 1) rows of roundup(M + 63, 64) + 64 granules of 8 bytes
    bridge = 256 * 1 * (576 + 64 + 40) * 8 + 256 * 2 * 4   # (+ the dispatch order of the parts: one int per workgroup)
    assert lib.sdp_state_bytes(256, 512, 512) == 256 * 8 * 576 * 64 * 5 + 1024 + bridge
    assert lib.sdp_state_bytes(1, 1, 1) == 1 * 1 * 64 * 64 * 5 + 256
    assert lib.sdp_state_bytes(3, 65, 2) == 3 * 2 * 128 * 64 * 5 + 256
    assert lib.sdp_state_bytes(2, 1024, 100) == 2 * 16 * 192 * 64 * 5 + 256 + 2 * 3 * (192 + 64 + 16) * 8 + 256
    assert lib.sdp_state_d_bytes(256, 512, 512) == 256 * 8 * 576 * 64 * 8 + 1024 + bridge
    assert lib.sdp_state_d_bytes(0, 5, 5) == 0
    assert lib.sdp_state_bytes(0, 5, 5) == 0


def test_header_states_the_packed_state_format_the_library_uses(lib):
    """include/sdp.h says how many bytes per cell the packed state takes (SDP_PACKED_STATE_BYTES_PER_CELL and the prose
    next to it): the number must be the one sdp_state_bytes is built on, so that the header cannot rot again (round 4: the
    header still said 6 bytes / 23-bit fields after the format had become 5 bytes / 20-bit)."""
    import re
    hdr = open(os.path.join(ROOT, "include", "sdp.h")).read()
    m = re.search(r"#define\s+SDP_PACKED_STATE_BYTES_PER_CELL\s+(\d+)", hdr)
    assert m, "include/sdp.h must define SDP_PACKED_STATE_BYTES_PER_CELL"
    per_cell = int(m.group(1))
    # (B, N, M) = (1, 64, 2): one strip, 2 + 63 -> 128 steps of 64 lanes; the tail (launch order) is 256 bytes
    assert lib.sdp_state_bytes(1, 64, 2) == 128 * 64 * per_cell + 256
    # two pairs more of 512 x 512 cost two records of 8 strips x 576 steps x 64 lanes (+ 1024 bytes of dispatch map for the
    # parts of the two extra pairs): the per-cell figure again, through a difference that drops the rest of the tail
    assert lib.sdp_state_pair_stride(1024, 1024, 0) == 16 * 1088 * 64 * per_cell
    assert lib.sdp_state_pair_stride(512, 512, 0) == 8 * 576 * 64 * per_cell
    assert f"{per_cell} bytes" in hdr and "20-bit" in hdr and "23-bit" not in hdr and "6 bytes" not in hdr
    for doc in ("INTEGRATION.md", os.path.join("deepblast_amd", "_engine.py"), os.path.join("deepblast_amd", "_dp.py")):
        text = open(os.path.join(ROOT, doc)).read()
        assert "6 bytes per cell" not in text and "6 B/cell" not in text, doc


def test_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    assert lib.sdp_forward_f32(None, one, one, one, 1, 1, 1, None, 0, 0, None) == -1
    assert b"null" in lib.sdp_last_error_string()
    assert lib.sdp_forward_f32(one, one, one, one, 0, 1, 1, None, 0, 0, None) == -2
    assert lib.sdp_forward_f32(one, one, one, one, 1, 1, 2049, None, 0, 0, None) == -3
    assert lib.sdp_forward_f32(one, one, one, one, 1, 1, 1, None, 7, 0, None) == -4
    assert lib.sdp_backward_f32(one, one, None, 1, 1, 1, None, 0, 0, None) == -1
    assert lib.sdp_adjoint_forward_f32(one, None, None, one, one, 1, 1, 1, None, 0, 0, None) == -1
    assert lib.sdp_adjoint_backward_f32(one, one, one, one, 1, 1, 1 << 20, None, 0, 0, None) == -3
    # flags in `variant` (SDP_EXACT_STATE, SDP_WAVES) are stripped before validation; junk above them is not
    assert lib.sdp_forward_f32(one, one, one, one, 0, 1, 1, None, 0x100 | (8 << 12), 0, None) == -2
    assert lib.sdp_forward_f32(one, one, one, one, 1, 1, 1, None, 1 << 20, 0, None) == -4
    info = (ctypes.c_int32 * 4)()
    assert lib.sdp_device_status(0, info) == 0 and list(info) == [0, 0, 0, 0]   # nothing launched: no status block


def _plan(lib, pass_, B, N, M, lens=0, exact=0, cus=256):
    import ctypes
    kid, chunk, waves, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    assert lib.sdp_plan(pass_, B, N, M, lens, exact, cus, ctypes.byref(kid), ctypes.byref(chunk), ctypes.byref(waves),
                        ctypes.byref(lds)) == 0
    return kid.value, chunk.value, waves.value, lds.value


def test_thin_long_problems_take_the_exact_state(lib):
    """Round 5: fewer than 32 rows (or columns) with more than 512 on the other axis -- the packed weights' rounding does not
    average out over many paths there (2 x 2048: 1.0e-4) -- use the float2 state, like problems with N + M > 4096; the sizing
    function follows (sdp_api.hip: exact_for).  Round 6: thin long PAIRS of a batch with per-pair lengths are routed to the float2
    build inside their own packed record, which needs more than 64 rows and more than 65 columns of padded shape to fit -- padded
    shapes with min(N, M) < 66 (and max > 512) therefore take the float2 state as a whole."""
    for (N, M, exact) in [(2, 1772, True), (1772, 2, True), (31, 513, True), (32, 2048, True), (65, 2048, True), (66, 2048, False), (2048, 65, True), (2048, 66, False),
                          (31, 512, False), (64, 512, False), (64, 960, True), (7, 1361, True),
                          (2048, 2048, False), (2049, 2048, True), (512, 512, False)]:
        assert (lib.sdp_state_bytes(3, N, M) == lib.sdp_state_d_bytes(3, N, M)) == exact, (N, M)


def test_launch_plan_policy(lib):
    """Which build / how many waves a launch uses, checked without a device."""
    LDS = 160 * 1024
    # headline: one pair per CU -> throughput builds, 4 waves, long chunks
    # (ids 29 .. 35 would be the builds of the 18-bit packed state, -DSDP_Q18=1: measured in round 5 and not adopted)
    assert _plan(lib, 0, 256, 512, 512)[:3] == (0, 32, 4)
    assert _plan(lib, 1, 256, 512, 512)[:3] == (1, 32, 4)
    # small batch -> latency builds, 8 waves, short chunks
    assert _plan(lib, 0, 16, 512, 512)[:3] == (6, 16, 8)
    # (backward sweep, round 5: the K = 32 packed build with 8 waves -- it needs < 256 registers now; the exact state keeps K = 16)
    assert _plan(lib, 1, 16, 512, 512)[:3] == (1, 32, 8) and _plan(lib, 1, 100, 512, 512)[:3] == (1, 32, 8)
    # the packed backward sweep's pipelined twin (id 36): only where every CU holds one pair of long rows (steady-state table, sdp_api.hip)
    assert _plan(lib, 1, 256, 512, 512)[:3] == (1, 32, 4) and _plan(lib, 1, 256, 1024, 1024)[:3] == (36, 32, 4)
    assert _plan(lib, 1, 256, 512, 1024)[0] == 36 and _plan(lib, 1, 256, 768, 640)[0] == 1 and _plan(lib, 1, 128, 1024, 1024)[:3] == (1, 32, 4)
    assert _plan(lib, 1, 1024, 512, 512)[:3] == (1, 32, 2) and _plan(lib, 1, 384, 1024, 1024)[0] == 1 and _plan(lib, 1, 256, 2048, 256)[0] == 1
    # (forward sweep: the throughput build from ~72 pairs on)
    assert _plan(lib, 0, 64, 512, 512)[:3] == (6, 16, 8) and _plan(lib, 0, 80, 512, 512)[:3] == (0, 32, 4)
    # a pair spread over several CUs, four strips (one per wave of the throughput builds) per workgroup: where it was
    # measured to pay -- per-pair lengths and a batch within the CU count: forward sweep from three parts on, backward sweep
    # from two; equal pairs: the backward sweep of a few pairs of more than twelve strips; never the adjoint pair
    pp = lambda pass_, B, N, M, lens, exact=0: lib.sdp_plan_parts(pass_, B, N, M, lens, exact, 256)
    # (round 5: the backward sweep no longer takes parts with per-pair lengths -- re-measured, profiles/r05_parts_table.txt)
    assert pp(0, 256, 1022, 1020, 1) == 4 and pp(1, 256, 1022, 1020, 1) == 0 and pp(0, 256, 640, 640, 1) == 4
    assert pp(0, 256, 512, 512, 1) == 0 and pp(1, 256, 512, 512, 1) == 0 and pp(1, 256, 256, 512, 1) == 0
    assert pp(0, 700, 1022, 1020, 1) == 0 and pp(1, 700, 1022, 1020, 1) == 0
    assert pp(0, 16, 1024, 1024, 0) == 0 and pp(1, 16, 1024, 1024, 0) == 4 and pp(1, 64, 640, 500, 0) == 0 and pp(1, 128, 1024, 512, 0) == 0
    assert pp(2, 16, 1024, 1024, 1, 1) == 0 and pp(3, 16, 1024, 1024, 1, 1) == 0
    assert _plan(lib, 1, 16, 1024, 1024)[:3] == (23, 32, 4)   # (the parts instantiation of the throughput build)
    # more pairs than CUs: two waves when that needs fewer rounds
    assert _plan(lib, 0, 512, 512, 512)[2] == 2 and _plan(lib, 0, 768, 512, 512)[2] == 4
    # per-pair lengths on a batch that does not queue up: long pairs in parts (above), otherwise treated like a small batch
    assert _plan(lib, 0, 256, 1024, 1024, lens=1)[:3] == (21, 32, 4)
    # (round 6: with per-pair lengths, or N not a multiple of 64, the forward builds' twins that clean what lies beside the
    #  matrix -- 37 / 38 / 39 / 40 for 0 / 9 / 6 / 5; the aligned no-lengths builds carry none of that code)
    assert _plan(lib, 0, 256, 512, 1024, lens=1)[:3] == (39, 16, 8)
    assert _plan(lib, 0, 600, 512, 512, lens=1)[0] == 37 and _plan(lib, 0, 256, 500, 512)[0] == 37 and _plan(lib, 0, 256, 500, 512, exact=1)[0] == 38
    assert _plan(lib, 0, 16, 500, 512)[0] == 39 and _plan(lib, 0, 16, 500, 512, exact=1)[0] == 40 and _plan(lib, 0, 16, 512, 512, lens=1)[0] == 39
    # exact state for the adjoint sweeps: its own build
    assert _plan(lib, 0, 256, 512, 512, exact=1)[0] == 9 and _plan(lib, 0, 16, 512, 512, exact=1)[0] == 5
    assert _plan(lib, 1, 256, 512, 512, exact=1)[:3] == (7, 32, 4) and _plan(lib, 1, 16, 512, 512, exact=1)[:3] == (8, 16, 8)
    # never more waves than strips; LDS always fits, also at the column limit
    assert _plan(lib, 0, 4, 100, 100)[2] == 2
    for pass_ in range(4):
        for (B, N, M) in [(256, 512, 512), (4, 64, 2048), (300, 2000, 2048), (1, 1, 1)]:
            kid, chunk, waves, lds = _plan(lib, pass_, B, N, M)
            assert 1 <= waves <= 8 and lds <= LDS, (pass_, B, N, M, kid, waves, lds)
    # the long-M fallback: throughput builds do not fit with 2048 columns
    assert _plan(lib, 0, 256, 512, 2048)[0] == 6 and _plan(lib, 1, 256, 512, 2048)[0] in (1, 4, 36)
    assert _plan(lib, 1, 256, 512, 2048, exact=1)[0] in (7, 8)


GENERAL_PITCH = 0x200   # include/sdp.h: SDP_PLAN_GENERAL_PITCH -- the build a launch takes when M is not a multiple of 32 or a plane starts off a 128-byte line


def _exact_state_builds(lib, B, N, M, lens):
    """{(pass, kernel id, waves)} of the four passes of the training path (exact state) on a 256-CU device"""
    out = set()
    for pass_ in range(4):
        kid, _, waves, _ = _plan(lib, pass_ | (GENERAL_PITCH if M % 32 else 0), B, N, M, lens, exact=1)
        out.add((pass_, kid, waves))
    return out


def test_second_order_cases_reach_every_exact_state_build(lib):
    """tests/test_parity_gpu.py::test_second_order_tracks_float64 holds the exact-state results to the float64 reference; its
    cases must reach every (pass, build, waves) the launch policy gives the exact-state passes over a grid of shapes -- batch
    sizes across the latency / throughput / two-wave / parts thresholds, 1 to 64+ strips, M on and off the 32 grid up to the
    column limit, with and without per-pair lengths.  A build or wave count added later with no case for it fails here."""
    from test_parity_gpu import F64_CASES
    Bs = [1, 2, 3, 8, 40, 64, 72, 73, 74, 100, 127, 128, 200, 256, 257, 300, 512, 513, 600, 1024]
    Ns = [1, 2, 31, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 321, 384, 385, 448, 449, 512, 513, 576, 577, 640,
          768, 769, 1024, 1025, 2048, 4097]
    Ms = [1, 7, 31, 32, 33, 64, 65, 96, 100, 512, 513, 960, 1024, 1025, 1500, 1536, 2000, 2048]
    reachable = set()
    for B in Bs:
        for N in Ns:
            for M in Ms:
                for lens in (0, 1):
                    reachable |= _exact_state_builds(lib, B, N, M, lens)
    covered = set()
    for c in F64_CASES:
        covered |= _exact_state_builds(lib, c[0], c[1], c[2], int(c[4]))
    assert not reachable - covered, f"exact-state builds no case of F64_CASES reaches: {sorted(reachable - covered)}"
    # (the grid does see all of them: forward 5 / 40 / adjoint forward at 1-8 waves, the throughput builds at 1-4, the parts twins)
    assert {(0, 5, 8), (0, 40, 5), (1, 19, 8), (2, 2, 8), (3, 14, 4), (0, 22, 4), (0, 26, 4), (1, 24, 4), (1, 28, 4), (0, 20, 2)} <= reachable


def _packed_state_builds(lib, B, N, M, lens, offset=0):
    """{(pass, kernel id, waves)} of the forward and backward sweeps on the packed state (256 CUs), or the empty set where the
    padded shape takes the exact state as a whole (sdp_api.hip: exact_for -- sdp_state_bytes then sizes the float2 state).  A
    launch takes the general-pitch twin when M is not a multiple of 32 or a plane does not start on a 128-byte line (`offset`
    floats: the cases of FIRST_ORDER_CASES offset theta, A and E alike)."""
    if lib.sdp_state_bytes(B, N, M) == lib.sdp_state_d_bytes(B, N, M):
        return set()
    out = set()
    for pass_ in (0, 1):
        kid, _, waves, _ = _plan(lib, pass_ | (GENERAL_PITCH if (M % 32 or offset % 32) else 0), B, N, M, lens)
        out.add((pass_, kid, waves))
    return out


def test_first_order_cases_reach_every_packed_state_build(lib):
    """tests/test_parity_gpu.py::test_first_order_tracks_float64 holds the packed state's E and Vt to the float64 reference; its
    cases must reach every (pass, build, waves) the launch policy gives the forward and backward sweeps on the packed state over a
    grid of shapes -- batch sizes across the latency / throughput / pipelined / two-wave / parts thresholds, 1 to 32 strips, N on
    and off the 64 grid, M on and off the 32 grid up to the column limit, with and without per-pair lengths, aligned and offset
    planes.  A build or wave count added later with no case for it fails here, and names it."""
    from test_parity_gpu import FIRST_ORDER_CASES
    Bs = [1, 2, 3, 8, 40, 64, 72, 73, 74, 100, 127, 128, 200, 224, 225, 256, 257, 300, 384, 512, 513, 600, 768, 1024]
    Ns = [1, 2, 31, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 321, 384, 385, 448, 449, 512, 513, 576, 577, 640,
          768, 769, 1020, 1022, 1023, 1024, 1025, 2048, 4097]
    Ms = [1, 7, 31, 32, 33, 64, 65, 96, 100, 512, 513, 960, 1020, 1022, 1023, 1024, 1025, 1500, 1536, 2000, 2048]
    reachable = set()
    for B in Bs:
        for N in Ns:
            for M in Ms:
                for lens in (0, 1):
                    for offset in (0, 1):
                        reachable |= _packed_state_builds(lib, B, N, M, lens, offset)
    covered = set()
    for c in FIRST_ORDER_CASES:
        covered |= _packed_state_builds(lib, c[0], c[1], c[2], int(c[4]), c[9])
    assert not reachable - covered, f"packed-state builds no case of FIRST_ORDER_CASES reaches: {sorted(reachable - covered)}"
    assert not covered - reachable, f"cases reach builds the grid does not see (widen the grid): {sorted(covered - reachable)}"
    # the grid does see the thin-margin builds: the pipelined backward sweep (36), the parts builds and their general-pitch twins,
    # two waves per pair, every wave count of the latency builds
    assert {(1, 36, 4), (0, 21, 4), (0, 25, 4), (1, 23, 4), (1, 27, 4), (0, 0, 2), (1, 1, 2), (0, 11, 2), (0, 6, 8), (0, 39, 8),
            (1, 12, 8)} <= reachable
    # ... and the cases reach the branches a key alone does not tell apart: two waves because of the batch size (more pairs than
    # CUs, four strips and more), the column-limit fallback of a full batch to the latency forward builds (6, 39), 36 on an
    # aligned batch
    two_waves = [c for c in FIRST_ORDER_CASES if c[0] > 256 and c[1] > 192 and _plan(lib, 0, c[0], c[1], c[2], int(c[4]))[2] == 2]
    assert len(two_waves) >= 2, two_waves
    fallback = [c for c in FIRST_ORDER_CASES if c[2] == 2048 and _plan(lib, 0, c[0], c[1], c[2], int(c[4]))[0] in (6, 39)
                and _plan(lib, 0, c[0], c[1], 1024, int(c[4]))[0] in (0, 37)]
    fallback_ids = {_plan(lib, 0, c[0], c[1], c[2], int(c[4]))[0] for c in fallback}
    for kid in (6, 39):
        assert kid in fallback_ids, f"no full-batch case of FIRST_ORDER_CASES reaches the 2048-column fallback to build {kid}"
    assert any(_plan(lib, 1, c[0], c[1], c[2], int(c[4]))[0] == 36 and not (c[2] % 32 or c[9]) for c in FIRST_ORDER_CASES)
    # (the packed backward sweep's latency build 4 / 15 is NOT reachable by the policy on its own since round 5: the K = 32 build
    #  runs eight waves and fits the column limit -- only a forced wave count above eight would take it)
    assert not any(k[0] == 1 and k[1] in (4, 15) for k in reachable)
    # shapes exact_for sends to the float2 state as a whole report exact-state builds, and are no packed build
    assert _packed_state_builds(lib, 3, 2049, 2048, 0) == set() and _packed_state_builds(lib, 3, 40, 1024, 1) == set()


# The one hand-written copy of the relation between a build and its general-pitch twin (deepblast_amd/csrc/sdp_builds.def states the
# builds, sdp_api.hip: plan / settle pick): a general-pitch build always cleans, so 0 and 37 share 11; the pipelined backward build
# has no twin of its own; the latency forward builds, the adjoint forward builds and the value sweep's latency builds keep the
# column-aligned geometry at any pitch and map to themselves.
GENERAL_PITCH_TWIN = {0: 11, 37: 11, 1: 12, 36: 12, 3: 14, 4: 15, 7: 18, 8: 19, 9: 20, 38: 20, 21: 25, 22: 26, 23: 27, 24: 28, 41: 43, 42: 43}


def test_general_pitch_plan_is_the_aligned_plan_with_the_twin_build(lib):
    """sdp_plan(pass | SDP_PLAN_GENERAL_PITCH) over the grid of test_first_order_cases_reach_every_packed_state_build, packed and
    exact state, every pass: chunk, waves and LDS are those of sdp_plan(pass) -- twins are compiled for the same chunk length and
    wave limit -- and the id is the twin's.  Without the flag the answer is pinned by tests/test_value.py against the golden plans."""
    hdr = open(os.path.join(ROOT, "include", "sdp.h")).read()
    assert re.search(r"#define\s+SDP_PLAN_GENERAL_PITCH\s+0x200\b", hdr)
    Bs = [1, 2, 3, 8, 40, 64, 72, 73, 74, 100, 127, 128, 200, 224, 225, 256, 257, 300, 384, 512, 513, 600, 768, 1024]
    Ns = [1, 2, 31, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 321, 384, 385, 448, 449, 512, 513, 576, 577, 640,
          768, 769, 1020, 1022, 1023, 1024, 1025, 2048, 4097]
    Ms = [1, 7, 31, 32, 33, 64, 65, 96, 100, 512, 513, 960, 1020, 1022, 1023, 1024, 1025, 1500, 1536, 2000, 2048]
    seen = set()
    for B in Bs:
        for N in Ns:
            for M in Ms:
                for lens in (0, 1):
                    for pass_, exact in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 1), (2 | 0x100, 1), (3, 1), (4, 0)):
                        kid, chunk, waves, lds = _plan(lib, pass_, B, N, M, lens, exact)
                        got = _plan(lib, pass_ | GENERAL_PITCH, B, N, M, lens, exact)
                        assert got == (GENERAL_PITCH_TWIN.get(kid, kid), chunk, waves, lds), (pass_, B, N, M, lens, exact, kid, got)
                        seen.add(kid)
    assert set(GENERAL_PITCH_TWIN) - {4} <= seen, sorted(set(GENERAL_PITCH_TWIN) - seen)   # (4: not reachable by the policy since round 5)
    assert lib.sdp_plan_parts(0 | GENERAL_PITCH, 256, 1022, 1020, 1, 0, 256) == 0   # (the flag is sdp_plan's)


def _table_rows():
    """[(id, symbol)] of the SDP_BUILD(id, symbol, ...) rows of deepblast_amd/csrc/sdp_builds.def"""
    src = open(os.path.join(ROOT, "deepblast_amd", "csrc", "sdp_builds.def")).read()
    return [(int(i), sym) for i, sym in re.findall(r"^SDP_BUILD\((\d+), (\w+),", src, flags=re.M)]


def test_kernel_names_are_the_builds_the_library_launches(lib, monkeypatch):
    """bench.py's per-kernel timers label a launch with sdp_kernel_name(sdp_plan's id): the library must name exactly the builds of
    its table -- no id of a build that is gone, none missing -- and every name must be a kernel it holds."""
    rows = _table_rows()
    ids = [i for i, _ in rows]
    assert len(rows) >= 36 and len(set(ids)) == len(ids) and {0, 4, 36, 40, 45} <= set(ids), rows
    for kid in range(-2, 80):
        name = lib.sdp_kernel_name(kid)
        assert (name is not None) == (kid in ids), kid
    for kid, sym in rows:
        assert lib.sdp_kernel_name(kid) == sym.encode(), (kid, sym)
        assert hasattr(lib, sym), f"{sym}: no such kernel in the library"   # (a kernel's host handle is an exported data symbol)
    # every id sdp_plan reports has a name (the grids of the coverage tests see every build but 4 / 15)
    for pass_ in (0, 1, 2, 2 | 0x100, 3, 4):
        for flag in (0, GENERAL_PITCH):
            for (B, N, M, lens, exact) in [(256, 512, 512, 0, 0), (16, 500, 100, 1, 1), (256, 1024, 1024, 1, 0), (16, 1024, 1024, 0, 1), (600, 512, 2048, 1, 0)]:
                assert lib.sdp_kernel_name(_plan(lib, pass_ | flag, B, N, M, lens, exact)[0]), (pass_, flag, B, N, M)
    # _label asks the library's own launch policy (sdp_plan) on the device's CU count
    from deepblast_amd._engine import HipEngine
    import torch

    class _Props:
        multi_processor_count = 256

    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda dev: _Props())
    eng = HipEngine()
    assert eng._label(0, 256, 500, 512, False, False, 0, "default") == "default"   # (no hook: no lookup)
    eng.launch_hook = lambda name: None
    assert eng._label(0, 256, 500, 512, False, False, 0, "default") == "sdp_fwd_c_kernel"
    assert eng._label(0, 16, 512, 512, True, False, 0, "default") == "sdp_fwd_lat_c_kernel"
    assert eng._label(0, 256, 512, 512, False, False, 0, "default") == "sdp_fwd_kernel"
    assert eng._label(1, 256, 1024, 1024, False, False, 0, "default") == "sdp_bwd_pipe_kernel"
    assert eng._label(0, 256, 512, 512, True, True, 0, "default") == "sdp_fwd_x_c_kernel"


def test_fused_seed_plan_keeps_four_waves_at_the_column_limit(lib):
    """The adjoint forward sweep with the fused loss seed (build 10) stages three planes (ref, pred, G) instead of two; by the
    LDS arithmetic of plan() with K = 16 it still keeps four waves at M = 2048, where it takes the most LDS.  The (N, M) grid is
    that of tests/test_end_to_end_gpu.py::test_fused_seed_tracks_float64, which runs every pair of it for NW and for SW: 1, 3 and
    4 waves, the last with strips taken in rounds."""
    FUSED = 0x100   # include/sdp.h: SDP_PLAN_FUSED_SEED
    hdr = open(os.path.join(ROOT, "include", "sdp.h")).read()
    assert re.search(r"#define\s+SDP_PLAN_FUSED_SEED\s+0x100\b", hdr)
    for N, waves in ((40, 1), (130, 3), (300, 4)):
        for M in (37, 170, 516, 1100, 2048):
            for B, lens in ((3, 0), (3, 1), (300, 1)):
                kid, chunk, w, lds = _plan(lib, 2 | FUSED, B, N, M, lens, 1)
                assert (kid, chunk, w) == (10, 16, waves), (N, M, B, lens, kid, chunk, w)
                assert lds <= 160 * 1024
                assert _plan(lib, 2, B, N, M, lens, 1)[0] != 10   # without the flag: the plain adjoint forward build
    assert lib.sdp_plan(0 | FUSED, 3, 40, 37, 0, 1, 256, None, None, None, None) != 0   # the flag belongs to pass 2 only
