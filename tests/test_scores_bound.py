"""CPU tests of tests/scores_ref.py: the derived bounds of the scores GEMM hold for a plain fp32 computation with room to
spare (torch's fp32 ops on the CPU stay below HALF of every bound, on every input family the GPU tests use) and do NOT
hold for the bug they are there to catch (a three-piece product that loses one of its six piece products), so a kernel
that passes test_scores_edges_gpu.py has fp32 accuracy and one that drops a product cannot pass it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import datagen
import scores_ref as R

SMALL_FORWARD = [s for shapes in R.FORWARD_CASES.values() for s in shapes if s[0] * s[1] * s[2] <= 300 * 100 * 100] + [R.UNALIGNED_CASE]


def _tensors(family, shape, seed=100):
    B, N, M, D = shape
    return [R.make_inputs(family, seed + 10 * k, B, N, M, D, tensor=k) for k in (0, 1)]


def test_cut_is_exact_and_the_pieces_are_bf16():
    x = np.concatenate([datagen.normal(1, (4096,)) * s for s in (1.0, 1e-3, 1e5, 1e-30, 3e37)]).astype(np.float32)
    x = np.concatenate([x, np.array([0.0, -0.0, 1.0, -1.0, 20.0, np.float32(1) + np.float32(2.0 ** -23), 1e-38, 1e-45], np.float32)])
    h0, h1, h2 = R.cut3(x)
    normal = (np.abs(x) >= 2.0 ** -100) | (x == 0)   # (below ~2^-102 the last residual is subnormal and has bits under a bf16's: a loss < 2^-126)
    for h in (h0, h1, h2):
        assert not (h.view(np.uint32) & np.uint32(0xffff))[normal].any()   # 8 significant bits each: a bf16, exactly
    assert np.array_equal(h0.astype(np.float64) + h1.astype(np.float64) + h2.astype(np.float64), x.astype(np.float64))
    assert np.array_equal((h0 + h1) + h2, x)                            # (also in fp32: the partial sums are prefixes of x)


@pytest.mark.parametrize("D", [16, 32, 48, 64])
def test_six_pieces_inside_the_bound_and_five_pieces_outside(D):
    """Positive operands: the exact six-piece sum is far inside bound_s; with ANY one of the five small piece products left
    out it is outside -- so the forward tests at D <= 64 on the positive family would catch that kernel."""
    x, y = R.make_inputs("positive", 40 + D, 2, 48, 44, D)
    s64, S = R.products64(x, y)
    bs = R.bound_s(S, D)
    r = R.ratio(R.three_piece_product(x, y), s64, bs)
    print(f"D={D}: six pieces {r:.3f} of bound_s")
    assert r <= 0.5
    for drop in R.PIECE_PAIRS[1:]:
        mutant = R.three_piece_product(x, y, drop=drop)
        rm = np.abs(mutant - s64) / bs
        print(f"D={D}: without x{drop[0]} y{drop[1]}: {rm.min():.2f} .. {rm.max():.2f} of bound_s")
        assert rm.max() > 1.0, (D, drop)
        # ... and through the activation, where its slope is not small (theta of positive scores: slope ~1)
        a64 = R.softplus64(s64)
        assert (np.abs(R.softplus64(mutant) - a64) / R.bound_act(bs, a64)).max() > 1.0, (D, drop)
        # ... and A on the negative family (y negated: the scores and every piece product change sign, nothing else)
        a64 = R.logsigmoid64(-s64)
        assert (np.abs(R.logsigmoid64(-mutant) - a64) / R.bound_act(bs, a64)).max() > 1.0, (D, drop)


def test_backward_product_without_a_piece_is_outside_the_bound():
    """The backward's dropped-product case: positive inputs and cotangents, contractions over 44 and 48, theta GIVEN (so the
    factor's error is the dS bound, not the forward's)."""
    B, N, M, D = R.BACKWARD_DROP_SHAPE
    x, y = R.make_inputs("positive", 70, B, N, M, D)
    theta = R.softplus64(R.products64(x * 0.25, y * 0.25)[0]).astype(np.float32)   # scores ~1: factor ~0.7
    g = (0.5 + datagen.uniform(71, (B, N, M), np.float64)).astype(np.float32)
    (dx, bx), (dy, by) = R.backward_ref(x, y, g, 0, act=theta)
    ds32 = (g.astype(np.float64) * -np.expm1(-theta.astype(np.float64))).astype(np.float32)
    yt, dst = np.ascontiguousarray(np.swapaxes(y, 1, 2)), np.ascontiguousarray(np.swapaxes(ds32, 1, 2))
    xt = np.ascontiguousarray(np.swapaxes(x, 1, 2))
    assert R.ratio(R.three_piece_product(ds32, yt), dx, bx) <= 0.5 and R.ratio(R.three_piece_product(dst, xt), dy, by) <= 0.5
    for drop in R.PIECE_PAIRS[1:]:
        rx = (np.abs(R.three_piece_product(ds32, yt, drop=drop) - dx) / bx).max()
        ry = (np.abs(R.three_piece_product(dst, xt, drop=drop) - dy) / by).max()
        print(f"without piece pair {drop}: dzx {rx:.2f}, dzy {ry:.2f} of the bound")
        assert rx > 1.0 and ry > 1.0, drop


@pytest.mark.parametrize("family", R.FAMILIES)
def test_fp32_forward_stays_below_half_of_every_bound(family):
    worst = {"s": 0.0, "act": 0.0}
    for shape in SMALL_FORWARD:
        for kind, (x, y) in enumerate(_tensors(family, shape)):
            s32 = torch.matmul(torch.from_numpy(x), torch.from_numpy(y).transpose(1, 2))
            a32 = (F.logsigmoid if kind else F.softplus)(s32)
            a64, ba, s64 = R.forward_ref(x, y, kind)
            bs = R.bound_s(R.products64(x, y)[1], shape[3])
            # (a score of exactly zero products has S = 0 and an exact fp32 value: 0 / 0 counts as 0)
            rs = np.abs(s32.numpy().astype(np.float64) - s64) / np.where(bs > 0, bs, 1.0)
            worst["s"], worst["act"] = max(worst["s"], float(rs.max())), max(worst["act"], R.ratio(a32.numpy(), a64, ba))
    print(f"{family}: torch fp32 reaches {worst['s']:.3f} of bound_s, {worst['act']:.3f} of the activation bound")
    assert worst["s"] <= 0.5 and worst["act"] <= 0.5


def test_steep_family_spans_the_activations_and_plants_its_points():
    for shape in SMALL_FORWARD + R.BACKWARD_SHAPES:
        B, N, M, D = shape
        (zx, zy), (gx, gy) = _tensors("steep", shape)
        s = np.concatenate([R.products64(zx, zy)[0].ravel(), R.products64(gx, gy)[0].ravel()])
        assert R.regions_present(s), shape
        if N >= 4 and M >= 6:
            for x, y in ((zx, zy), (gx, gy)):
                row = R.products64(x, y)[0][B - 1, N - 1, M - 5:]
                # single products: exact (the sign of the -0 is lost in the sum with the row's other, +0, products)
                assert np.array_equal(row, R.PLANTED.astype(np.float64)), shape


def test_fp32_activations_over_the_whole_range():
    """torch's own fp32 softplus / logsigmoid against float64 over [-104, 104] and the special points: inside (4 + |y|) u,
    the activation's share of the bound, by itself."""
    s = np.concatenate([np.linspace(-104, 104, 200001), [0.0, -0.0, 20.0, -20.0, 1e-30, -1e-30, 88.0, -88.0, 103.9, -103.9],
                        np.nextafter(np.float32(20), np.float32([0, 30])).astype(np.float64)]).astype(np.float32)
    for kind, fn in enumerate((F.softplus, F.logsigmoid)):
        a64 = R.act64(s.astype(np.float64), kind)
        r = R.ratio(fn(torch.from_numpy(s)).numpy(), a64, R.bound_act(0.0, a64))
        print(f"kind {kind}: torch fp32 reaches {r:.3f} of (4 + |y|) u")
        assert r <= 1.0


@pytest.mark.parametrize("family", R.FAMILIES)
def test_fp32_backward_stays_below_half_of_the_bound(family):
    worst = 0.0
    for shape in R.BACKWARD_SHAPES + [R.BACKWARD_DROP_SHAPE]:
        B, N, M, D = shape
        for kind, (x, y) in enumerate(_tensors(family, shape)):
            g = datagen.normal(300 + kind, (B, N, M)) if family in ("signed", "steep") else (0.5 + datagen.uniform(300 + kind, (B, N, M)))
            g = g.astype(np.float32)
            tx, ty = torch.from_numpy(x).requires_grad_(), torch.from_numpy(y).requires_grad_()
            a32 = (F.logsigmoid if kind else F.softplus)(torch.matmul(tx, ty.transpose(1, 2)))
            (a32 * torch.from_numpy(g)).sum().backward()
            (dx, bx), (dy, by) = R.backward_ref(x, y, g, kind)
            worst = max(worst, R.ratio(tx.grad.numpy(), dx, bx), R.ratio(ty.grad.numpy(), dy, by))
            # from the given fp32 outputs, as the kernel forms it: g * -expm1(-+act), then fp32 products
            act = a32.detach()
            ds32 = torch.from_numpy(g) * -torch.expm1(act if kind else -act)
            (dx, bx), (dy, by) = R.backward_ref(x, y, g, kind, act=act.numpy())
            worst = max(worst, R.ratio(torch.matmul(ds32, ty.detach()).numpy(), dx, bx),
                        R.ratio(torch.matmul(ds32.transpose(1, 2), tx.detach()).numpy(), dy, by))
    print(f"{family}: torch fp32 backward reaches {worst:.3f} of the bound")
    assert worst <= 0.5


def test_fp32_ds_stays_below_half_of_the_bound_on_both_sides_of_the_switch():
    g, theta, A = R.ds_inputs(5, 2, 40, 36)
    assert (g == 0).any() and (g < 0).any()
    assert (np.abs(theta) < R.SERIES_SWITCH).any() and (theta == np.float32(R.SERIES_SWITCH)).any() and (theta > R.SERIES_SWITCH).any()
    for kind, act in enumerate((theta, A)):
        ds32 = torch.from_numpy(g) * -torch.expm1(torch.from_numpy(act if kind else -act))
        ref, bound = R.ds_ref(g, act, kind)
        nz = bound > 0
        assert np.array_equal(ds32.numpy()[~nz], np.zeros((~nz).sum(), np.float32))     # g = 0: exactly zero
        r = R.ratio(ds32.numpy()[nz], ref[nz], bound[nz])
        print(f"kind {kind}: torch fp32 dS reaches {r:.3f} of the bound")
        assert r <= 0.5
        # a factor without the series below the switch (1 - exp alone) is what the bound is there to catch
        naive = torch.from_numpy(g) * (1.0 - torch.exp(torch.from_numpy(act if kind else -act)))
        assert R.ratio(naive.numpy()[nz], ref[nz], bound[nz]) > 1.0
