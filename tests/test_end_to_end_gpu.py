"""GPU: the widened path end to end (SURVEY 8 f4 -> a -> f3): reference-style collate with the lengths side-channel
-> decode(theta, A, lengths) -> fused masked loss with the same lengths -> backward.  Expected values: the reference's
per-item procedure (alignment.py:165-170 slices each pair; losses.py:26-46 loops over pairs) evaluated with the CPU
oracle in float64."""
import os

import numpy as np
import pytest
import torch

import datagen
import parity
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_collate_decode_loss_backward(golden_dir, variant):
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder
    from deepblast_amd.batching import collate_with_lengths
    from deepblast_amd.losses import MatrixCrossEntropy
    d = np.load(os.path.join(golden_dir, "g10_batching.npz"))
    batch = [tuple(torch.from_numpy(d[f"i{b}_{k}"]) for k in ("gene", "other", "states", "aln", "path", "mask", "gm", "om"))
             for b in range(len(d["sizes"]))]
    genes, others, states, dm, p, G, gM, oM, lengths = collate_with_lengths(batch)
    B, N, M = dm.shape
    G = G.clone()
    G[:, 0, 0] = True   # every pair counts at least one cell (an empty mask is mean([]) = NaN in the reference too)
    theta, A = datagen.theta_A(333, B, N, M)   # stands in for the language-model scores (alignment.py:122-123)
    Yt = (dm > 0.8).float()
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(theta).to(dev).requires_grad_()
    a = torch.from_numpy(A).to(dev).requires_grad_()
    dec = (NeedlemanWunschDecoder, SmithWatermanDecoder)[variant]("softmax")
    aln = dec.decode(t, a, lengths.to(dev))
    xl, yl = lengths[:, 0].tolist(), lengths[:, 1].tolist()
    loss = MatrixCrossEntropy()(Yt.to(dev), aln, xl, yl, G.to(dev))
    loss.backward()
    torch.cuda.synchronize()

    # reference procedure, pair by pair
    ref_loss, ref_grad, ref_aln = 0.0, np.zeros((B, N, M)), np.zeros((B, N, M), np.float32)
    seeds = []   # per pair: the loss gradient the adjoint pair is seeded with (for the float64 reference below)
    eps = 3e-8
    for b in range(B):
        n, m = xl[b], yl[b]
        th, ga = np.ascontiguousarray(theta[b:b + 1, :n, :m]), np.ascontiguousarray(A[b:b + 1, :n, :m])
        _, E, Q, Ef = oracle.fwd_bwd(th, ga, None, variant)
        ref_aln[b, :n, :m] = E[0]
        g = G[b, :n, :m].numpy().astype(bool)
        y = Yt[b, :n, :m].numpy().astype(np.float64)
        pr = np.clip(E[0].astype(np.float32), np.float32(eps), np.float32(1 - eps)).astype(np.float64)
        cnt = g.sum()
        ref_loss += -np.sum((y * np.log(pr) + (1 - y) * np.log(1 - pr))[g]) / cnt / B
        inside = (E[0] >= eps) & (E[0] <= 1 - eps)
        Z = np.where(g & inside, -(y / pr - (1 - y) / (1 - pr)) / (cnt * B), 0.0).astype(np.float32)
        Ed, _, _ = oracle.double_backward(Q, Ef, Z[None])
        ref_grad[b, :n, :m] = Ed[0]
        seeds.append(Z)
    assert parity.abs_err(aln.detach().cpu().numpy(), ref_aln) <= parity.TOL
    assert abs(float(loss) - ref_loss) <= 1e-4 * max(1.0, abs(ref_loss))
    assert parity.abs_err(t.grad.cpu().numpy(), ref_grad, scale=True) <= parity.TOL

    def ref64():   # the same procedure in float64 (the C oracle's f64 path), seeded with the same loss gradient
        g64 = np.zeros((B, N, M))
        for b in range(B):
            n, m = xl[b], yl[b]
            _, _, Q, Ef = oracle.fwd_bwd(parity.f64(theta[b:b + 1, :n, :m]), parity.f64(A[b:b + 1, :n, :m]), None, variant)
            g64[b, :n, :m] = oracle.double_backward(Q, Ef, parity.f64(seeds[b][None]))[0][0]
        return {"Ed": g64}
    parity.check_second_order({"Ed": t.grad.cpu().numpy()}, {"Ed": ref_grad}, ref64, f"collate -> decode -> loss, variant {variant}")
    # nothing leaks outside a pair's own block
    for b in range(B):
        assert not t.grad[b, xl[b]:, :].any() and not t.grad[b, :, yl[b]:].any()


@pytest.mark.parametrize("name", ["mce", "path", "align"])
@pytest.mark.parametrize("use_lengths", [False, True], ids=["padded-dp", "lengths-dp"])
def test_fused_decode_loss_equals_the_unfused_path(name, use_lengths):
    """SURVEY f3 as written: the masked loss's gradient seeds the adjoint forward sweep inside the kernel
    (sdp_adjoint_forward_loss_f32).  Same loss and the same gradient w.r.t. theta as decode() -> loss -> backward."""
    from deepblast_amd import NeedlemanWunschDecoder
    from deepblast_amd.losses import MatrixCrossEntropy, SoftAlignmentLoss, SoftPathLoss, decode_loss
    B, N, M = 5, 150, 170
    theta, A = datagen.theta_A(1234, B, N, M)
    lens = datagen.lengths(1235, B, 20, 150)
    lens[0] = (N, M)
    dev = torch.device("cuda", 0)
    Yt = torch.from_numpy((datagen.uniform(1236, (B, N, M)) < 0.1).astype(np.float32)).to(dev)
    P = torch.from_numpy(datagen.uniform(1237, (B, N, M)) * 3).to(dev)
    G = torch.from_numpy((datagen.uniform(1238, (B, N, M)) < 0.8).astype(np.float32)).to(dev)
    loss_fn, first = {"mce": (MatrixCrossEntropy(), Yt), "path": (SoftPathLoss(), P), "align": (SoftAlignmentLoss(), Yt)}[name]
    xl, yl = lens[:, 0].tolist(), lens[:, 1].tolist()
    ln = torch.from_numpy(lens).to(dev) if use_lengths else None
    dec = NeedlemanWunschDecoder("softmax")

    t1 = torch.from_numpy(theta).to(dev).requires_grad_()
    a1 = torch.from_numpy(A).to(dev).requires_grad_()
    aln = dec.decode(t1, a1, ln) if use_lengths else dec.decode(t1, a1)
    l1 = loss_fn(first, aln, xl, yl, G)
    l1.backward()

    t2 = torch.from_numpy(theta).to(dev).requires_grad_()
    a2 = torch.from_numpy(A).to(dev).requires_grad_()
    l2, E = decode_loss(dec, loss_fn, t2, a2, first, xl, yl, G, lengths=ln)
    l2.backward()
    torch.cuda.synchronize()
    if use_lengths:
        # decode_loss leaves E outside the pairs' blocks unwritten by default (SDP_NO_FILL: nothing in the op reads it); inside
        # the blocks it is the decoder's E bit for bit, and fill=True gives the whole tensor
        for b in range(B):
            assert torch.equal(E[b, :xl[b], :yl[b]], aln.detach()[b, :xl[b], :yl[b]]), b
        t3 = torch.from_numpy(theta).to(dev).requires_grad_()
        l3, E3 = decode_loss(dec, loss_fn, t3, torch.from_numpy(A).to(dev), first, xl, yl, G, lengths=ln, fill=True)
        assert torch.equal(E3, aln.detach()) and float(l3) == float(l2)
    else:
        assert torch.equal(E, aln.detach())
    assert abs(float(l1) - float(l2)) <= 1e-6 * max(1.0, abs(float(l1)))
    g1, g2 = t1.grad, t2.grad
    assert float((g1 - g2).abs().max()) <= 1e-6 * max(1.0, float(g1.abs().max())), float((g1 - g2).abs().max())
    assert a2.grad is None


@pytest.mark.parametrize("name", ["mce", "path", "align"])
def test_fused_decode_loss_when_the_loss_reads_beyond_the_dp_blocks(name):
    """decode_loss(lengths=...) with x_len / y_len LARGER than `lengths` -- the API allows the loss to slice by other
    lengths than the DP sweeps.  The loss kernel then reads E between the two blocks, which decode() zero-fills; the fused op
    must not leave it unwritten there (round 5 did, by default: garbage or NaN in the loss).  Same loss and gradient as the
    unfused path, with the buffers poisoned beforehand so that unwritten memory cannot pass for zeros."""
    from deepblast_amd import NeedlemanWunschDecoder
    from deepblast_amd.losses import MatrixCrossEntropy, SoftAlignmentLoss, SoftPathLoss, decode_loss
    B, N, M = 6, 140, 150
    theta, A = datagen.theta_A(4321, B, N, M)
    lens = datagen.lengths(4322, B, 20, 100)
    big = np.minimum(lens + np.array([[30, 40]]), np.array([[N, M]])).astype(lens.dtype)   # the loss's lengths: beyond the DP's
    dev = torch.device("cuda", 0)
    Yt = torch.from_numpy((datagen.uniform(4323, (B, N, M)) < 0.1).astype(np.float32)).to(dev)
    P = torch.from_numpy(datagen.uniform(4324, (B, N, M)) * 3).to(dev)
    G = torch.from_numpy((datagen.uniform(4325, (B, N, M)) < 0.8).astype(np.float32)).to(dev)
    loss_fn, first = {"mce": (MatrixCrossEntropy(), Yt), "path": (SoftPathLoss(), P), "align": (SoftAlignmentLoss(), Yt)}[name]
    xl, yl = big[:, 0].tolist(), big[:, 1].tolist()
    dec = NeedlemanWunschDecoder("softmax")
    t1 = torch.from_numpy(theta).to(dev).requires_grad_()
    a1 = torch.from_numpy(A).to(dev).requires_grad_()   # (decode differentiates w.r.t. both, like the reference)
    l1 = loss_fn(first, dec.decode(t1, a1, lens.tolist()), xl, yl, G)
    l1.backward()
    # poison the allocator's free blocks: whatever the fused op leaves unwritten is then NaN, not a lucky zero
    for _ in range(3):
        junk = torch.full((B, N, M), float("nan"), device=dev)
        del junk
    t2 = torch.from_numpy(theta).to(dev).requires_grad_()
    l2, E = decode_loss(dec, loss_fn, t2, torch.from_numpy(A).to(dev).requires_grad_(), first, xl, yl, G, lengths=lens.tolist())
    l2.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(l2) and torch.isfinite(E).all()
    assert abs(float(l1) - float(l2)) <= 1e-6 * max(1.0, abs(float(l1))), (float(l1), float(l2))
    assert float((t1.grad - t2.grad).abs().max()) <= 1e-6 * max(1.0, float(t1.grad.abs().max()))
    for b in range(B):
        assert not E[b, lens[b, 0]:, :].any() and not E[b, :, lens[b, 1]:].any()


# ----------------------------------------------------------------------------------------------------------------
# the fused loss seed (sdp_adj_fwd_loss_kernel, build 10) against float64
# ----------------------------------------------------------------------------------------------------------------
_DT = {"bool": torch.bool, "uint8": torch.uint8, "float64": torch.float64, "float32": torch.float32}


def _fused_against_f64(name, variant, B, N, M, use_lengths, peaked, dt_first, dt_G, seed, unfused=False):
    """decode_loss on (B, N, M) -> loss and theta.grad, held to the reference procedure built from the kernel's OWN E: the loss
    seed dLoss/dE in float64 (tests/loss_ref.py), then the adjoint pair of the CPU oracle seeded with it (fp32 reference and,
    for check_second_order's exemption, float64).  With `unfused`, decode() -> loss -> backward must also give the same loss
    and gradient."""
    import loss_ref
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder
    from deepblast_amd.losses import MatrixCrossEntropy, SoftAlignmentLoss, SoftPathLoss, decode_loss
    rng = np.random.default_rng(seed)
    theta, A = datagen.theta_A(seed, B, N, M)
    if peaked:
        theta = theta * 8   # E gets exact 0s and values that round to 1: the clamp mask acts inside the sweep
    lens = np.stack([rng.integers(1, N + 1, B), rng.integers(1, M + 1, B)], 1).astype(np.int64)
    lens[0] = (N, M)
    Yt = rng.uniform(size=(B, N, M)) < 0.1
    P = rng.uniform(0.0, 3.0, (B, N, M))
    G = rng.uniform(size=(B, N, M)) < 0.8
    dev = torch.device("cuda", 0)
    dec = (NeedlemanWunschDecoder, SmithWatermanDecoder)[variant]("softmax")
    xl, yl = lens[:, 0].tolist(), lens[:, 1].tolist()
    ln = lens.tolist() if use_lengths else None     # (a list equal to x_len / y_len: the lean path that shares one tensor)
    if name == "mce" and peaked:
        # Targets on the alignment itself, as in training.  Random targets on peaked scores put Yt = 1 on cells where E ~ 1e-7:
        # there the seed Yt / E turns E's fp32 error of ~1e-8 (absolute) into an O(1 / (cnt B)) error of Ed, which no reference
        # separates from the sweeps' own (measured: the fp32 reference is 3e-4 from float64 there, as the engine is)
        t0, a0 = (torch.from_numpy(x).to(dev).requires_grad_() for x in (theta, A))
        Yt = (dec.decode(t0, a0, ln) > 0.5).detach().cpu().numpy()
    first_np = (P if name == "path" else Yt).astype(np.float32)    # what the kernels read (the op converts to float32)
    first = torch.from_numpy(P if name == "path" else Yt).to(_DT[dt_first]).to(dev)
    Gt = torch.from_numpy(G).to(_DT[dt_G]).to(dev)
    loss_fn = {"mce": MatrixCrossEntropy(), "path": SoftPathLoss(), "align": SoftAlignmentLoss()}[name]
    t = torch.from_numpy(theta).to(dev).requires_grad_()
    loss, E = decode_loss(dec, loss_fn, t, torch.from_numpy(A).to(dev), first, xl, yl, Gt, lengths=ln)
    loss.backward()
    torch.cuda.synchronize()
    got = t.grad.cpu().numpy()
    what = f"{name} {('NW', 'SW')[variant]} {B}x{N}x{M} lengths={use_lengths} peaked={peaked}"
    if unfused:
        t1 = torch.from_numpy(theta).to(dev).requires_grad_()
        a1 = torch.from_numpy(A).to(dev).requires_grad_()   # (decode differentiates w.r.t. both, like the reference)
        aln = dec.decode(t1, a1, ln) if use_lengths else dec.decode(t1, a1)
        l1 = loss_fn(first, aln, xl, yl, Gt)
        l1.backward()
        assert abs(float(l1.detach()) - float(loss.detach())) <= 1e-6 * max(1.0, abs(float(l1.detach()))), what
        assert float((t1.grad - t.grad).abs().max()) <= 1e-6 * max(1.0, float(t1.grad.abs().max())), what
    inb = loss_ref.blocks(B, N, M, xl, yl)
    En = np.where(inb, E.detach().cpu().numpy(), 0.0).astype(np.float32)   # (outside the blocks E may be unwritten)
    ref = loss_ref.loss(name, first_np, En, xl, yl, G)
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-6 * abs(ref["loss"]), (what, float(loss.detach()), ref["loss"])
    Z = ref["grad"]
    ed32, ed64 = np.zeros((B, N, M)), np.zeros((B, N, M))
    dp = lens if use_lengths else np.tile([[N, M]], (B, 1))
    for b in range(B):
        n, m = int(dp[b, 0]), int(dp[b, 1])
        _, _, Q, Ef = oracle.fwd_bwd(np.ascontiguousarray(theta[b:b + 1, :n, :m]), np.ascontiguousarray(A[b:b + 1, :n, :m]), None, variant)
        ed32[b, :n, :m] = oracle.double_backward(Q, Ef, Z[b:b + 1, :n, :m].astype(np.float32))[0][0]

    def ref64():
        for b in range(B):
            n, m = int(dp[b, 0]), int(dp[b, 1])
            _, _, Q, Ef = oracle.fwd_bwd(parity.f64(theta[b:b + 1, :n, :m]), parity.f64(A[b:b + 1, :n, :m]), None, variant)
            ed64[b, :n, :m] = oracle.double_backward(Q, Ef, Z[b:b + 1, :n, :m])[0][0]
        return {"Ed": ed64}
    rec = parity.check_second_order({"Ed": got}, {"Ed": ed32}, ref64, what)
    if use_lengths:
        assert not got[~loss_ref.blocks(B, N, M, dp[:, 0], dp[:, 1])].any(), what
    return rec


def _fused_cases():
    """Both sweeps (NW, SW), each over every (N, M) of N in {40, 130, 300} x M in {37, 170, 516, 1100, 2048}: the fused build at
    1, 3 and 4 waves, the last with strips in rounds, up to its largest LDS (N = 300, M = 2048: tests/test_abi.py pins that plan
    to 4 waves).  The three losses, padded / lengths and plain / peaked theta rotate over the shapes so that each sweep runs every
    loss both padded and with lengths, and peaked theta both padded and with lengths; `first` and G as bool, uint8 and float64."""
    Ms, Ns, dts, names = [37, 170, 516, 1100, 2048], [40, 130, 300], ["bool", "uint8", "float64"], ("mce", "path", "align")
    cases = []
    for variant in (0, 1):
        for k, (N, M) in enumerate((N, M) for N in Ns for M in Ms):
            name = names[(k + variant) % 3]
            use_lengths = (N, M) == (300, 2048) or (k + variant) % 2 == 0
            peaked = (k // 2 + variant) % 2 == 1
            dt_first = ("float64" if k % 2 else "float32") if name == "path" else dts[k % 3]
            cases.append((name, variant, 2 if N * M > 200000 else 3, N, M, use_lengths, peaked, dt_first, dts[(k + 1) % 3]))
    for variant in (0, 1):
        mine = [c for c in cases if c[1] == variant]
        assert {(c[0], c[5]) for c in mine} == {(n, u) for n in names for u in (False, True)}, variant
        assert {c[5] for c in mine if c[6]} == {False, True}, variant
        assert any(c[3:6] == (300, 2048, True) for c in mine), variant
    return cases


@pytest.mark.parametrize("case", _fused_cases(), ids=lambda c: f"{c[0]}-{('nw', 'sw')[c[1]]}-{c[2]}x{c[3]}x{c[4]}-{'lens' if c[5] else 'padded'}"
                         f"{'-peaked' if c[6] else ''}")
def test_fused_seed_tracks_float64(case):
    name, variant, B, N, M, use_lengths, peaked, dt_first, dt_G = case
    _fused_against_f64(name, variant, B, N, M, use_lengths, peaked, dt_first, dt_G, seed=N * 7 + M + 100 * variant,
                       unfused=N * M <= 200000)


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_fused_seed_more_pairs_than_cus(variant):
    """B > CUs with per-pair lengths: the adjoint forward takes the pairs in the order of their records (order_in_state)."""
    _fused_against_f64("mce", variant, 300, 40, 37, True, True, "uint8", "bool", seed=31 + variant, unfused=True)


@pytest.mark.parametrize("name", ["mce", "path", "align"])
def test_decode_loss_on_pairs_wider_than_the_column_limit(name):
    """decode() transposes problems with M > sdp_max_cols() and N within it (_dp.py: _transposed); decode_loss does the same with
    the loss's operands and lengths.  2 x 300 x 3000 with lengths against the unfused path, one pair (SW, padded) against
    float64; both sides over the limit raise what decode() raises."""
    _fused_against_f64(name, 0, 2, 300, 3000, True, False, "float32" if name == "path" else "bool", "uint8", seed=3000, unfused=True)
    _fused_against_f64(name, 1, 1, 300, 3000, False, True, "float64", "float64", seed=3001, unfused=True)


def test_decode_loss_over_the_column_limit_on_both_sides_raises_like_decode():
    from deepblast_amd import NeedlemanWunschDecoder
    from deepblast_amd.losses import MatrixCrossEntropy, decode_loss
    dev = torch.device("cuda", 0)
    B, N, M = 1, 2049, 2050
    theta = torch.zeros(B, N, M, device=dev)
    A = torch.zeros(B, N, M, device=dev)
    dec = NeedlemanWunschDecoder("softmax")
    with pytest.raises(Exception) as e1:
        dec.decode(theta, A)
    with pytest.raises(type(e1.value)) as e2:
        decode_loss(dec, MatrixCrossEntropy(), theta, A, torch.zeros_like(theta), [N], [M], torch.ones_like(theta))
    assert str(e2.value) == str(e1.value)
