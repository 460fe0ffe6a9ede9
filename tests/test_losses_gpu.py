"""GPU: fused masked losses against fixtures produced by the real reference
(deepblast/losses.py, oracle/gen_golden_losses.py) and against a plain-torch fp32 restatement at the
headline size.  Tolerance: 1e-5 relative on the scalar, 1e-5 * max|grad| absolute on the gradient
(the reference accumulates in fp32; the kernel in float64).  Against the float64 restatement (tests/loss_ref.py) at the
edges and over a grid of shapes: 1e-6 relative on values, 1e-6 * max|grad| on the gradient, and exact zeros wherever the
restatement's gradient is zero; the C entry points' per-pair sums, counts, determinism, writes and alignment rule."""
import os
import time

import numpy as np
import pytest
import torch

import datagen
import loss_ref
from deepblast_amd.losses import MatrixCrossEntropy, SoftAlignmentLoss, SoftPathLoss

pytestmark = pytest.mark.gpu
LOSS = {"mce": (MatrixCrossEntropy, "Yt"), "path": (SoftPathLoss, "P"), "align": (SoftAlignmentLoss, "Yt")}


_torch_reference = loss_ref.torch_reference   # the reference algorithm with the same torch ops (tests/loss_ref.py)


@pytest.mark.parametrize("name", ["mce", "path", "align"])
def test_against_reference_fixture(golden_dir, name):
    d = np.load(os.path.join(golden_dir, "g9_losses.npz"))
    cls, first = LOSS[name]
    pred = torch.from_numpy(d["Yp"]).cuda().requires_grad_()
    lens = d["lens"]
    loss = cls()(torch.from_numpy(d[first]).cuda(), pred, lens[:, 0].tolist(), lens[:, 1].tolist(),
                 torch.from_numpy(d["G"]).cuda())
    loss.backward()
    assert abs(float(loss) - float(d[name + "_loss"])) <= 1e-5 * max(1.0, abs(float(d[name + "_loss"])))
    gref = d[name + "_grad"]
    assert np.max(np.abs(pred.grad.cpu().numpy() - gref)) <= 1e-5 * max(1.0, np.abs(gref).max())


@pytest.mark.parametrize("name", ["mce", "path", "align"])
def test_headline_size_and_timing(name):
    B, N, M = 256, 512, 512
    lens = datagen.lengths(70, B, 64, 512)
    Yp = torch.from_numpy(datagen.uniform(71, (B, N, M)) * 0.98 + 0.01).cuda()
    Yt = torch.from_numpy((datagen.uniform(72, (B, N, M)) < 0.05).astype(np.float32)).cuda()
    P = torch.from_numpy(datagen.uniform(73, (B, N, M)) * 4).cuda()
    G = torch.from_numpy((datagen.uniform(74, (B, N, M)) < 0.8).astype(np.float32)).cuda()
    first = P if name == "path" else Yt
    xl, yl = lens[:, 0].tolist(), lens[:, 1].tolist()
    cls = LOSS[name][0]()

    def ours():
        p = Yp.detach().requires_grad_()
        loss = cls(first, p, xl, yl, G)
        loss.backward()
        return loss.detach(), p.grad

    def ref():
        p = Yp.detach().requires_grad_()
        loss = _torch_reference(name, first, p, xl, yl, G)
        loss.backward()
        return loss.detach(), p.grad

    l1, g1 = ours()
    l2, g2 = ref()
    assert abs(float(l1) - float(l2)) <= 2e-5 * max(1.0, abs(float(l2)))
    assert float((g1 - g2).abs().max()) <= 2e-5 * max(1.0, float(g2.abs().max()))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        ours()
    torch.cuda.synchronize()
    t_ours = (time.perf_counter() - t0) / 5
    t0 = time.perf_counter()
    ref()
    torch.cuda.synchronize()
    t_ref = time.perf_counter() - t0
    print(f"loss {name} B={B} {N}x{M}: fused {t_ours * 1e3:.2f} ms fwd+bwd, per-pair torch loop {t_ref * 1e3:.1f} ms")


# ----------------------------------------------------------------------------------------------------------------
# against the float64 restatement (tests/loss_ref.py)
# ----------------------------------------------------------------------------------------------------------------
NAMES = loss_ref.NAMES
KIND = loss_ref.KIND
DEV = "cuda:0"


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _c_forward(first, pred, G, lens, kind):
    """sdp_loss_forward_f32 -> (acc float64 (B,), cnt int32 (B,)) as numpy."""
    from deepblast_amd._engine import _ptr, get_engine
    eng = get_engine()
    B, N, M = pred.shape
    acc = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
    cnt = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    rc = eng.lib.sdp_loss_forward_f32(_ptr(first), _ptr(pred), _ptr(G), _ptr(lens), _ptr(acc), _ptr(cnt), B, N, M, kind, 0,
                                      eng._stream(0))
    assert rc == 0
    torch.cuda.synchronize()
    return acc.cpu().numpy(), cnt.cpu().numpy()


def _c_backward(first, pred, G, lens, scale, grad, kind):
    from deepblast_amd._engine import _ptr, get_engine
    eng = get_engine()
    B, N, M = pred.shape
    rc = eng.lib.sdp_loss_backward_f32(_ptr(first), _ptr(pred), _ptr(G), _ptr(lens), _ptr(scale), _ptr(grad), B, N, M, kind, 0,
                                       eng._stream(0))
    assert rc == 0
    torch.cuda.synchronize()


def _value_ok(got, ref, rel=1e-6):
    if np.isnan(ref):
        return np.isnan(got)
    return abs(got - ref) <= rel * abs(ref)


def _check_against_f64(name, first, pred, lens, G, what):
    """The class's value and gradient, and the C forward's per-pair sums and counts, against loss_ref.loss on the same
    inputs (numpy, float32).  -> the restatement's record."""
    B = pred.shape[0]
    xl, yl = lens[:, 0].tolist(), lens[:, 1].tolist()
    ref = loss_ref.loss(name, first, pred, xl, yl, G)
    f, G_, lens_ = _cuda(first), _cuda(G), _cuda(lens.astype(np.int32))
    p = _cuda(pred).requires_grad_()
    loss = LOSS[name][0]()(f, p, xl, yl, G_)
    loss.backward()
    got = p.grad.cpu().numpy().astype(np.float64)
    assert _value_ok(float(loss.detach()), ref["loss"]), (what, float(loss.detach()), ref["loss"])
    gref = ref["grad"]
    gmax = float(np.abs(gref).max()) if gref.size else 0.0
    assert np.max(np.abs(got - gref)) <= 1e-6 * gmax, (what, float(np.max(np.abs(got - gref))), gmax)
    # exactly zero where the float64 gradient is: outside G, outside the block, behind the clamp, a zero norm
    z = gref == 0
    assert not got[z].any(), (what, int(np.count_nonzero(got[z])))
    acc, cnt = _c_forward(f, p.detach(), G_, lens_, KIND[name])
    assert np.array_equal(cnt, ref["cnt"]), what
    bad = [b for b in range(B) if not (acc[b] == ref["acc"][b] if ref["acc"][b] == 0 else abs(acc[b] - ref["acc"][b]) <= 1e-6 * abs(ref["acc"][b]))]
    assert not bad, (what, [(b, acc[b], ref["acc"][b]) for b in bad[:5]])
    return ref


@pytest.mark.parametrize("name", NAMES)
def test_edge_fixture_against_reference_and_float64(golden_dir, name):
    """g14 (the real reference at its edges): M % 4 in {1, 2, 3} (the scalar branch) and 0, lengths 0 and beyond N / M, an empty
    mask (NaN), predictions on and one ulp either side of both clamp bounds, G of 0.5 / -1 / NaN, vectors of ~1e-20 and of zeros."""
    d = np.load(os.path.join(golden_dir, "g14_losses_edges.npz"))
    cls, fk = LOSS[name]
    for case in sorted({k.split("_")[0] for k in d.files}):
        lens = d[case + "_lens"]
        first, Yp, G = d[f"{case}_{fk}"], d[case + "_Yp"], d[case + "_G"]
        p = _cuda(Yp).requires_grad_()
        loss = cls()(_cuda(first), p, lens[:, 0].tolist(), lens[:, 1].tolist(), _cuda(G))
        loss.backward()
        ref, gref = float(d[f"{case}_{name}_loss"]), d[f"{case}_{name}_grad"]
        if np.isnan(ref):
            assert torch.isnan(loss), case
        else:
            assert abs(float(loss.detach()) - ref) <= 1e-5 * max(1.0, abs(ref)), (case, float(loss.detach()), ref)
        assert np.max(np.abs(p.grad.cpu().numpy() - gref)) <= 1e-5 * max(1.0, np.abs(gref).max()), case
        assert not p.grad.cpu().numpy()[gref == 0].any(), case
        _check_against_f64(name, first, Yp, lens, G, f"g14 {case}")


def _grid():
    Ms, Ns, Bs = [1, 2, 3, 5, 63, 64, 65, 127, 130, 512], [1, 7, 300], [1, 3, 700]
    out = []
    for i, M in enumerate(Ms):
        for j, N in enumerate(Ns):
            B = Bs[(i + j) % 3]
            if B * N * M > (1 << 21):
                B = 3
            out.append((B, N, M))
    assert {b for b, _, _ in out} == set(Bs)
    return out + [(1, 4096, 4096)]


@pytest.mark.parametrize("name", NAMES)
def test_grid_against_float64(name):
    """Every M from 1 to 512 around the float4 boundary, N of 1, 7 and 300, 1, 3 and 700 pairs (more than the CUs), and one
    4096 x 4096 pair (a single forward workgroup): ragged lengths with 0 and beyond N / M, soft and binary targets, predictions
    with and without the clamp edges planted."""
    for k, (B, N, M) in enumerate(_grid()):
        c = loss_ref.edge_case(7000 + 31 * k + KIND[name], B, N, M, planted=k % 2 == 0)
        if k % 3 == 1:
            c["Yt"] = (c["Yt"] > 0.5).astype(np.float32)       # binary targets
        lens = c["lens"]
        if B > 1:
            lens[0] = (N, M)
            lens[1] = (0, M) if k % 2 else (N, 0)
        first = c["P"] if name == "path" else c["Yt"]
        _check_against_f64(name, first, c["Yp"], lens, c["G"], f"B={B} N={N} M={M}")


@pytest.mark.parametrize("M", [12, 13])
@pytest.mark.parametrize("name", NAMES)
def test_forward_entry_point_counts_and_bits(name, M):
    """sdp_loss_forward_f32: cnt[b] is the count of G != 0 in the block, exactly; lens = NULL is lens = (N, M) bit for bit; a
    pair alone gives the bits it gives inside a batch; two calls give the same bits."""
    B, N = 9, 37
    c = loss_ref.edge_case(800 + M + KIND[name], B, N, M)
    first = _cuda(c["P"] if name == "path" else c["Yt"])
    pred, G = _cuda(c["Yp"]), _cuda(c["G"])
    kind = KIND[name]
    lens = c["lens"].astype(np.int32)
    acc, cnt = _c_forward(first, pred, G, _cuda(lens), kind)
    for b in range(B):
        n, m = min(lens[b, 0], N), min(lens[b, 1], M)
        assert cnt[b] == np.count_nonzero(c["G"][b, :n, :m] != 0), b
    full = np.tile(np.array([[N, M]], np.int32), (B, 1))
    a0, c0 = _c_forward(first, pred, G, None, kind)
    a1, c1 = _c_forward(first, pred, G, _cuda(full), kind)
    assert a0.tobytes() == a1.tobytes() and np.array_equal(c0, c1)
    a2, c2 = _c_forward(first, pred, G, _cuda(lens), kind)
    assert a2.tobytes() == acc.tobytes() and np.array_equal(c2, cnt)
    for b in (0, 4, B - 1):
        ab, cb = _c_forward(first[b:b + 1].contiguous(), pred[b:b + 1].contiguous(), G[b:b + 1].contiguous(),
                            _cuda(lens[b:b + 1]), kind)
        assert ab.tobytes() == acc[b:b + 1].tobytes() and cb[0] == cnt[b], b


@pytest.mark.parametrize("M", [16, 13], ids=["float4", "scalar"])
@pytest.mark.parametrize("name", NAMES)
def test_backward_entry_point_writes_every_cell_and_nothing_else(name, M):
    """sdp_loss_backward_f32 on a NaN-filled buffer: every cell of the padded (B, N, M) tensor is written (zero outside the
    blocks and G), and a guard zone of sentinels directly behind the tensor is untouched -- for the float4 branch (M % 4 == 0,
    aligned) and the scalar one."""
    B, N, GUARD = 5, 23, 256
    c = loss_ref.edge_case(900 + M + KIND[name], B, N, M)
    first = c["P"] if name == "path" else c["Yt"]
    lens = c["lens"].astype(np.int32)
    scale = np.array([0.5, -1.25, 3.0, 1e-3, -7.0], np.float32)
    buf = torch.full((B * N * M + GUARD,), float("nan"), device=DEV)
    buf[B * N * M:] = 12345.0
    grad = buf[:B * N * M].view(B, N, M)
    _c_backward(_cuda(first), _cuda(c["Yp"]), _cuda(c["G"]), _cuda(lens), _cuda(scale), grad, KIND[name])
    g = grad.cpu().numpy()
    assert not np.isnan(g).any()
    assert (buf[B * N * M:] == 12345.0).all()
    # and the values: scale[b] times the per-cell factor d(term)/d(pred), rebuilt here in float64
    inb = loss_ref.blocks(B, N, M, lens[:, 0], lens[:, 1]) & (c["G"] != 0)
    assert not g[~inb].any()
    r64, y64 = first.astype(np.float64), c["Yp"].astype(np.float64)
    with np.errstate(all="ignore"):
        if name == "mce":
            ok = (c["Yp"] >= loss_ref.EPS_LO) & (c["Yp"] <= loss_ref.EPS_HI)
            fac = np.where(ok, r64 / y64 - (1 - r64) / (1 - y64), 0.0)
        else:
            fac = r64 * r64 * y64 if name == "path" else r64 - y64
    want = np.where(inb, scale.astype(np.float64)[:, None, None] * fac, 0.0)
    assert np.max(np.abs(g - want)) <= 1e-6 * np.abs(want).max()
    assert not g[want == 0].any()


def _offset_view(a, off=1):
    """A contiguous view of `a`'s values that starts `off` floats (4 bytes each) into a fresh buffer: its data pointer is not
    16-byte aligned, although M may be a multiple of 4."""
    flat = torch.full((a.numel() + 4,), float("nan"), device=DEV)
    v = flat[off:off + a.numel()].view(a.shape)
    v.copy_(a)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return v


@pytest.mark.parametrize("name", NAMES)
def test_unaligned_views_give_the_bits_of_aligned_copies(name):
    """The float4 path is taken only when ref, pred, G (and grad) are 16-byte aligned (include/sdp.h).  Views at a 4-byte
    offset -- which .contiguous() passes on unchanged -- through the Python class and through both C entry points give the
    same bits as aligned copies."""
    B, N, M = 4, 19, 64
    c = loss_ref.edge_case(1100 + KIND[name], B, N, M)
    lens = c["lens"].astype(np.int32)
    xl, yl = lens[:, 0].tolist(), lens[:, 1].tolist()
    first, pred, G = _cuda(c["P"] if name == "path" else c["Yt"]), _cuda(c["Yp"]), _cuda(c["G"])
    cls = LOSS[name][0]()
    p0 = pred.clone().requires_grad_()
    l0 = cls(first, p0, xl, yl, G)
    l0.backward()
    for which in range(4):   # one operand misaligned at a time, then all three
        ops = [first, pred, G]
        if which < 3:
            ops[which] = _offset_view(ops[which], 1 + which)
        else:
            ops = [_offset_view(o, k + 1) for k, o in enumerate(ops)]
        p1 = ops[1].detach().requires_grad_()
        assert p1.data_ptr() == ops[1].data_ptr()
        l1 = cls(ops[0], p1, xl, yl, ops[2])
        l1.backward()
        assert l1.detach().cpu().numpy().tobytes() == l0.detach().cpu().numpy().tobytes(), which
        assert torch.equal(p1.grad, p0.grad), which
        a0, c0 = _c_forward(first, pred, G, _cuda(lens), KIND[name])
        a1, c1 = _c_forward(ops[0], ops[1], ops[2], _cuda(lens), KIND[name])
        assert a0.tobytes() == a1.tobytes() and np.array_equal(c0, c1), which
    # the backward entry point into a misaligned grad, with a guard zone behind it
    scale = _cuda(np.array([0.5, -2.0, 1.5, 3.0], np.float32))
    g0 = torch.empty(B, N, M, device=DEV)
    _c_backward(first, pred, G, _cuda(lens), scale, g0, KIND[name])
    buf = torch.full((B * N * M + 64,), float("nan"), device=DEV)
    buf[1 + B * N * M:] = -777.0
    g1 = buf[1:1 + B * N * M].view(B, N, M)
    _c_backward(_offset_view(first, 2), _offset_view(pred, 3), G, _cuda(lens), scale, g1, KIND[name])
    assert torch.equal(g0, g1) and float(buf[0]) != float(buf[0]) and (buf[1 + B * N * M:] == -777.0).all()


@pytest.mark.parametrize("name", NAMES)
def test_gradient_scales_with_the_incoming_gradient(name):
    """(3 * loss).backward() and autograd.grad with grad_outputs scale the gradient (the backward multiplies the per-pair factor
    by the incoming gradient); by a power of two, bit for bit."""
    B, N, M = 3, 21, 30
    c = loss_ref.edge_case(1200 + KIND[name], B, N, M, planted=False)
    lens = c["lens"]
    xl, yl = lens[:, 0].tolist(), lens[:, 1].tolist()
    first, G = _cuda(c["P"] if name == "path" else c["Yt"]), _cuda(c["G"])
    cls = LOSS[name][0]()
    ref = loss_ref.loss(name, c["P"] if name == "path" else c["Yt"], c["Yp"], xl, yl, c["G"])["grad"]
    p = _cuda(c["Yp"]).requires_grad_()
    (3 * cls(first, p, xl, yl, G)).backward()
    g3 = p.grad.cpu().numpy()
    assert np.max(np.abs(g3 - 3 * ref)) <= 1e-6 * 3 * np.abs(ref).max()
    p = _cuda(c["Yp"]).requires_grad_()
    loss = cls(first, p, xl, yl, G)
    (g25,) = torch.autograd.grad(loss, p, grad_outputs=torch.tensor(-2.5, device=DEV), retain_graph=True)
    assert np.max(np.abs(g25.cpu().numpy() + 2.5 * ref)) <= 1e-6 * 2.5 * np.abs(ref).max()
    (g1,) = torch.autograd.grad(loss, p, retain_graph=True)
    (g4,) = torch.autograd.grad(loss, p, grad_outputs=torch.tensor(4.0, device=DEV))
    assert torch.equal(g4, 4 * g1)


@pytest.mark.parametrize("name", NAMES)
def test_forward_keeps_small_terms_beside_large_ones(name):
    """Each thread of the forward kernel first meets a large term (rows 0-3: one group of four columns per thread), then 255
    groups of terms below half an fp32 ulp of its running sum.  Summed in float64 they add up to 1e-5 of the value; an fp32
    partial sum would drop every one of them."""
    B, N, M = 2, 1024, 1024
    G = np.ones((B, N, M), np.float32)
    if name == "mce":
        first, pred = np.zeros((B, N, M), np.float32), np.full((B, N, M), 1e-9, np.float32)   # -log(1 - 3e-8) each
        first[:, :4], pred[:, :4] = 1.0, 0.5                                                # -log(0.5) each
    else:
        first = np.ones((B, N, M), np.float32)
        pred = np.full((B, N, M), 3e-5, np.float32) if name == "path" else np.full((B, N, M), 1 - 3e-5, np.float32)
        pred[:, :4] = 0.1 if name == "path" else 0.9                                         # squares of 0.01 beside 9e-10
    lens = np.array([[N, M], [N, M - 4]], np.int64)
    ref = _check_against_f64(name, first, pred, lens, G, f"small beside large, {name}")
    small = ref["acc"] - np.array([4 * M, 4 * (M - 4)]) * (np.log(0.5) if name == "mce" else 0.01)
    assert np.all(np.abs(small) > 5e-6 * np.abs(ref["acc"]))   # (what an fp32 partial sum would lose)
