"""CPU: the 'hardmax' operator's host logic (deepblast_amd/_dp.py: make_hard_functions, Decoder.optimal_paths, the transposed
route's tie rule) on a stand-in engine built from tests/hard_ref.py, the argument checks of the sdp_hard_* entries, and
hard_ref itself against brute force."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import hard_ref
import strip_schedule
from hard_engine import HardOracleEngine


@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = HardOracleEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


def _decoders():
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder
    return NeedlemanWunschDecoder, SmithWatermanDecoder


def _t(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.requires_grad_() if grad else t


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_hardmax_forward_returns_the_optimal_score(eng, variant):
    """the red test: 'hardmax' raised NotImplementedError before the operator existed"""
    th, a = hard_ref.quarter_scores(1, 3, 7, 9)
    dec = _decoders()[variant]("hardmax")
    Vt = dec(_t(th), _t(a))
    assert Vt.shape == (3,) and Vt.dtype == torch.float32
    assert np.array_equal(Vt.numpy().view(np.uint32), hard_ref.batch(th, a, variant)["Vt"].view(np.uint32))
    assert np.array_equal(dec.score(_t(th), _t(a)).numpy(), Vt.numpy())
    assert np.array_equal(_decoders()[variant]("hardmax", arithmetic="reference")(_t(th), _t(a)).numpy(), Vt.numpy())


def test_operator_table(eng):
    NW, SW = _decoders()
    th, a = hard_ref.quarter_scores(2, 1, 3, 3)
    with pytest.raises(NotImplementedError):
        NW("sparsemax")(_t(th), _t(a))
    with pytest.raises(NotImplementedError):
        NW(None)(_t(th), _t(a))
    with pytest.raises(TypeError):
        NW("hardmax")(_t(th).double(), _t(a).double())
    with pytest.raises(TypeError):
        NW("hardmax").score(_t(th).double(), _t(a).double())
    with pytest.raises(ValueError):
        NW("hardmax")(_t(th), _t(a)[:, :, :2])


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_backward_is_et_on_the_path_and_a_grad_is_a(eng, variant):
    th, a = hard_ref.quarter_scores(3, 4, 6, 8)
    dec = _decoders()[variant]("hardmax")
    t, A = _t(th, True), _t(a, True)
    Et = torch.tensor([2.5, 0.0, -1.25, 1.0])          # non-uniform, zero and negative
    dec(t, A).backward(Et)
    ref = hard_ref.batch(th, a, variant, Et=Et.numpy())
    assert np.array_equal(t.grad.numpy().view(np.uint32), ref["E"].view(np.uint32))
    assert np.array_equal(A.grad.numpy(), a)            # the pass-through convention of the soft pair
    for b, cells in enumerate(ref["cells"]):
        on = np.zeros((6, 8), bool)
        for (i, j, _) in cells:
            on[i, j] = True
        assert np.array_equal(t.grad.numpy()[b] != 0, on & (Et[b].item() != 0))


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("with_za", [False, True])
def test_decode_is_differentiable_with_zero_theta_gradient(eng, variant, with_za):
    from deepblast_amd import nw, sw
    th, a = hard_ref.quarter_scores(4, 3, 7, 5)
    dec = _decoders()[variant]("hardmax")
    t, A = _t(th, True), _t(a, True)
    aln = dec.decode(t, A)
    ref = hard_ref.batch(th, a, variant)
    assert np.array_equal(aln.detach().numpy(), ref["E"])
    rng = np.random.RandomState(5)
    Z = rng.randn(3, 7, 5).astype(np.float32)
    (aln * _t(Z)).sum().backward()
    assert t.grad is not None and not t.grad.numpy().any()
    # Vtd: the gradient with respect to Et, from the Function pair
    FB = (nw.NeedlemanWunschHardFunctionBackward, sw.SmithWatermanHardFunctionBackward)[variant]
    et = torch.tensor([1.0, 2.0, -0.5], requires_grad=True)
    _, P = eng.hard_forward(_t(th), _t(a), variant)
    E2, A2 = FB.apply(_t(th), _t(a), et, P, "hardmax", None, False)
    ZA = rng.randn(3, 7, 5).astype(np.float32)
    out = (E2 * _t(Z)).sum() + ((A2 * _t(ZA)).sum() if with_za else 0)
    (vtd,) = torch.autograd.grad(out, et)
    for b, cells in enumerate(ref["cells"]):
        want = sum(float(Z[b, i, j]) for (i, j, _) in cells)
        if with_za:
            want += sum(float(ZA[b, i, j]) for (i, j, k) in cells if k != 1)
        assert abs(float(vtd[b]) - want) <= 1e-6 * max(1.0, abs(want)), (b, float(vtd[b]), want)


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_lengths_and_the_padded_list(eng, variant):
    N, M = 6, 7
    th, a = hard_ref.quarter_scores(6, 5, N, M)
    lens = [[1, 1], [1, 7], [6, 1], [6, 7], [3, 4]]
    dec = _decoders()[variant]("hardmax")
    ref = hard_ref.batch(th, a, variant, lens)
    t = _t(th, True)
    Vt = dec(t, _t(a), torch.tensor(lens), fill=False)      # `fill` is accepted and ignored: E is always written in full
    assert np.array_equal(Vt.detach().numpy().view(np.uint32), ref["Vt"].view(np.uint32))
    Vt.sum().backward()
    assert np.array_equal(t.grad.numpy().view(np.uint32), ref["E"].view(np.uint32))
    Vo, paths = dec.optimal_alignments(_t(th), _t(a), torch.tensor(lens))
    assert Vo.grad_fn is None and np.array_equal(Vo.numpy(), ref["Vt"])
    assert paths == ref["lists"]
    for b, (n, m) in enumerate(lens):
        if ref["cells"][b]:
            assert paths[b][0][:2] == (0, 0) and paths[b][-1][:2] == (n - 1, m - 1)
        else:   # no cell exists: the padding alone, from (n-1, m-1) -- which is not itself recorded -- down to (0, 0)
            assert variant == 1 and len(paths[b]) == n + m - 2 and (not paths[b] or paths[b][0][:2] == (0, 0))
        if variant == 1 and (n < 2 or m < 2):
            assert not ref["cells"][b] and ref["Vt"][b] == 0 and not ref["E"][b].any()
        npad = len(paths[b]) - len(ref["cells"][b])
        for k, ((i0, j0, _), (i1, j1, s1)) in enumerate(zip(paths[b], paths[b][1:])):
            if k + 1 > npad:    # inside the path a cell's state names the step into it (the padding's names the step out of it)
                assert (i1 - i0, j1 - j0) == ((1, 0), (1, 1), (0, 1))[s1]
            elif k + 1 < npad:
                assert (i1 - i0, j1 - j0) == ((1, 0), (1, 1), (0, 1))[paths[b][k][2]]
            assert (i1 - i0, j1 - j0) in ((1, 0), (1, 1), (0, 1))
    # (score.alignment_stats launches a kernel: tests/test_hard_gpu.py hands it this list on the device)


def test_decode_loss_refuses_a_hard_decoder(eng):
    from deepblast_amd import losses
    th, a = hard_ref.quarter_scores(7, 2, 4, 4)
    with pytest.raises(NotImplementedError, match="identically zero"):
        losses.decode_loss(_decoders()[0]("hardmax"), losses.SoftAlignmentLoss(), _t(th), _t(a), _t(th), [4, 4], [4, 4], _t(th))


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_optimal_paths_on_a_soft_decoder(eng, variant):
    th, a = hard_ref.quarter_scores(8, 2, 5, 6)
    dec = _decoders()[variant]("softmax")
    Vt, states, counts = dec.optimal_paths(_t(th, True), _t(a, True))
    assert Vt.grad_fn is None and states.dtype == torch.int32 and tuple(states.shape) == (2, 5 + 6 + 2, 3)
    ref = hard_ref.batch(th, a, variant)
    for b in range(2):
        assert [tuple(r) for r in states[b, :counts[b]].tolist()] == ref["lists"][b]


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_transposed_route_finds_the_same_path(monkeypatch, variant):
    """many ties: swept as (n, m), and -- with the column limit lowered below m -- transposed, the path and E are identical"""
    from deepblast_amd import _engine
    th, a = hard_ref.quarter_scores(9, 3, 6, 11, lo=-0.25, hi=0.25)
    lens = torch.tensor([[6, 11], [4, 9], [2, 11]])
    got = {}
    for cols in (2048, 8):
        e = HardOracleEngine(cols)
        monkeypatch.setattr(_engine, "_ENGINE", e)
        dec = _decoders()[variant]("hardmax")
        t = _t(th, True)
        Vt = dec(t, _t(a), lens)
        Vt.sum().backward()
        _, paths = dec.optimal_alignments(_t(th), _t(a), lens)
        got[cols] = (Vt.detach().numpy(), t.grad.numpy(), paths, dec.score(_t(th), _t(a), lens).numpy())
        assert all(c == ((3, 11, 6), True) for c in e.hard_calls) if cols == 8 else all(c == ((3, 6, 11), False) for c in e.hard_calls)
    for x, y in zip(got[2048], got[8]):
        assert (x == y) if isinstance(x, list) else np.array_equal(x, y)
    ref = hard_ref.batch(th, a, variant, lens.numpy())
    assert got[8][2] == ref["lists"] and np.array_equal(got[8][1], ref["E"])
    # both sides over the limit: the engine's error, as for the soft operator
    e = HardOracleEngine(4)
    monkeypatch.setattr(_engine, "_ENGINE", e)
    with pytest.raises(ValueError):
        _decoders()[variant]("hardmax")(_t(th), _t(a))


def test_tie_flag_is_needed():
    """the family above does have ties that the two scan orders break differently: a transposed sweep with the DEFAULT order
    finds another path on at least one pair"""
    th, a = hard_ref.quarter_scores(9, 3, 6, 11, lo=-0.25, hi=0.25)
    differ = 0
    for b in range(3):
        _, cells, _ = hard_ref.pair(th[b], a[b], 0)
        _, cells_t, _ = hard_ref.pair(np.ascontiguousarray(th[b].T), np.ascontiguousarray(a[b].T), 0)
        differ += sorted((i, j) for (i, j, _) in cells) != sorted((j, i) for (i, j, _) in cells_t)
    assert differ > 0


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_hard_ref_against_brute_force(variant):
    for n, m in itertools.product(range(1, 5), range(1, 5)):
        for seed in range(3):
            th, a = hard_ref.quarter_scores(100 + seed, 1, n, m)
            Vt, cells, lst = hard_ref.pair(th[0], a[0], variant)
            assert Vt == hard_ref.brute_force_best(th[0], a[0], variant), (n, m, seed)
            assert (lst[0][:2] == (0, 0)) if lst else (n == 1 and m == 1 and variant == 1)


# the small shapes of tests/test_hard_gpu.py: SHAPES (the loop reference takes about a second per 50k cells)
SMALL = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (31, 33), (64, 64), (65, 130), (63, 16), (64, 17), (65, 1), (65, 2), (66, 33), (66, 34)]


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_fast_form_is_the_loop_bit_for_bit(variant):
    """hard_ref.forward_fast (one numpy operation per anti-diagonal) against hard_ref.forward: Vt, every pointer, path and list"""
    def cont(seed, B, N, M):
        rng = np.random.RandomState(seed)
        return np.logaddexp(0, rng.randn(B, N, M)).astype(np.float32), (-np.logaddexp(0, -rng.randn(B, N, M))).astype(np.float32)
    for family in (hard_ref.quarter_scores, cont):
        for (n, m) in SMALL:
            th, a = family(11, 1, n, m)
            Vt, P = hard_ref.forward(th[0], a[0], variant)
            Vf, Pf = hard_ref.forward_fast(th[0], a[0], variant)
            assert np.float32(Vt).view(np.uint32) == np.float32(Vf).view(np.uint32) and np.array_equal(P, Pf), (n, m)
    th, a = hard_ref.quarter_scores(13, 5, 40, 40)
    a[3, 5:, 7] = -np.inf
    lens = [(1, 1), (40, 40), (2, 39), (33, 17), (0, 4)]
    for ln in (None, lens):
        r, f = (hard_ref.batch(th, a, variant, ln, Et=[1.0, -2.5, 0.0, 1.0, 1.0], fwd=fw) for fw in (hard_ref.forward, hard_ref.forward_fast))
        assert np.array_equal(r["Vt"].view(np.uint32), f["Vt"].view(np.uint32)) and np.array_equal(r["E"].view(np.uint32), f["E"].view(np.uint32))
        assert r["cells"] == f["cells"] and r["lists"] == f["lists"]


def test_the_wide_shapes_are_on_the_routes_they_are_named_for():
    """seven waves from M = 1983 on, nine strips at 513 rows (csrc/sdp_hard.h, csrc/sdp_api.hip: hard_waves)"""
    c = strip_schedule.check_wide_shapes("sdp_hard.h")
    assert c["PTR_STEPS"] == 16


# ---- the C ABI's argument checks need no GPU ----
@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def test_hard_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    fwd, val, walk = lib.sdp_hard_forward_f32, lib.sdp_hard_forward_value_f32, lib.sdp_hard_walk_f32
    for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
        assert fwd(*args, 1, 1, 1, None, 0, 0, None) == -1
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        assert val(*args, 1, 1, 1, None, 0, 0, None) == -1
    assert walk(None, one, one, one, one, 1, 1, 1, None, 0, 0, None) == -1
    assert walk(one, one, None, None, None, 1, 1, 1, None, 0, 0, None) == -1     # neither E nor states
    assert walk(one, None, one, None, None, 1, 1, 1, None, 0, 0, None) == -1     # E without Et
    assert walk(one, None, None, one, None, 1, 1, 1, None, 0, 0, None) == -1     # states without counts
    for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
        assert fwd(one, one, one, one, *shape, None, 0, 0, None) == -2, shape
        assert val(one, one, one, *shape, None, 0, 0, None) == -2, shape
        assert walk(one, one, one, one, one, *shape, None, 0, 0, None) == -2, shape
        assert lib.sdp_hard_state_bytes(*shape) == 0
    over = lib.sdp_max_cols() + 1
    assert fwd(one, one, one, one, 1, 1, over, None, 0, 0, None) == -3
    assert val(one, one, one, 1, 1, over, None, 1, 0, None) == -3
    assert walk(one, one, one, one, one, 1, 1, over, None, 0, 0, None) == -3
    assert lib.sdp_hard_state_bytes(1, 1, over) == 0
    for flag in (0x100, 0x200, 0x400, 0x800, 0x10000, 7):
        assert fwd(one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
    assert fwd(one, one, one, one, 1, 1 << 18, 2048, None, 0, 0, None) == -5
    # 2 bits per cell, in whole 256-byte lines of a strip of 64 rows
    assert lib.sdp_hard_state_bytes(1, 512, 512) == 8 * 36 * 256
    assert lib.sdp_hard_state_bytes(3, 65, 1) == 3 * 2 * 4 * 256   # 1 + 63 steps: two chunks, four words
    assert lib.sdp_version() == 106
