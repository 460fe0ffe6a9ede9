"""Float64 reference and DERIVED error bounds for the scores GEMM (deepblast_amd/csrc/sdp_scores.hip), numpy only.

    theta = softplus(zx . zy^T),  A = logsigmoid(gx . gy^T)          (forward)
    dzx = dS . zy,  dzy = dS^T . zx,  dS = g * d act / d s           (backward; the same for gx, gy)

Nothing here is fitted to what a kernel returns.  With u = 2^-24 (half an ulp of a float in [1, 2)), s64 the float64
product of the fp32 operands and S = |x| . |y|^T:

* pre-activation: |s - s64| <= (D + 4) u S.  D u S is the standard bound for an fp32 sum of D products in any order
  (Higham, Accuracy and Stability of Numerical Algorithms, 3.1: gamma_D ~ D u); the other 4 u S covers the rounding of the
  products themselves and the three piece pairs that the three-piece bf16 product leaves out (x1 y2, x2 y1 <= 2^-24 |xy|
  each, x2 y2 <= 2^-32 |xy|: sdp_scores.hip, "The same product on the bf16 matrix pipe").
* activation: softplus and logsigmoid are 1-Lipschitz, so |got - act64(s64)| <= bound_s + (4 + |act64|) u; the second term
  is exp2 and log at 1 ulp each on values <= 1, the rounding of 1 + t, the ln 2 multiply and the final add.
* backward: with f64 = sigmoid(s64) (theta) or 1 - sigmoid(s64) (A) and dS64 = g f64, for a contraction over K indices
      bound = sum_k |g| (bound_fwd + 4u) |other| + (K + 4) u sum_k |dS64| |other|
  -- d(1 - e^-theta)/dtheta <= 1 and d(1 - e^A)/dA <= 1, so the forward's error enters the factor at most once.
* dS from GIVEN fp32 outputs, against g (-expm1(-+act)) in float64: |err| <= |g| (8u f + [|act| >= 2^-5] 4u) -- the series
  branch of the fused kernel is good to ~1e-8 relative plus four fp32 fmas, the 1 - exp2 branch to 1 ulp of a value < 1.
  `backward_ref(..., act=...)` uses this as the factor's error in place of bound_fwd + 4u: the reference then starts from
  the outputs the kernel was given, not from the scores.

The input families of the GPU tests and a numpy emulation of the three-piece cut live here too, so that the CPU tests
(test_scores_bound.py) pin the bounds on exactly what the GPU tests (test_scores_edges_gpu.py) feed the kernels.
"""
import numpy as np

import datagen

U = 2.0 ** -24
SERIES_SWITCH = 2.0 ** -5   # |act| below which the fused backward takes the series for 1 - exp (sdp_scores.hip, one_minus_exp)
FAMILIES = ("positive", "negative", "signed", "steep")


# ---------------------------------------------------------------------------------------------------------------- forward
def softplus64(s):
    return np.logaddexp(0.0, s)


def logsigmoid64(s):
    return -np.logaddexp(0.0, -s)


def act64(s, kind):
    """kind 0: softplus (theta), 1: logsigmoid (A)."""
    return logsigmoid64(s) if kind else softplus64(s)


def factor64(s, kind):
    """d act / d s: sigmoid(s) for theta, 1 - sigmoid(s) for A, to full relative accuracy on both tails."""
    return np.exp(-np.logaddexp(0.0, s if kind else -s))


def products64(x, y):
    """(s64, S) for fp32 (B, N, D) and (B, M, D): the float64 einsum and the einsum of absolute values."""
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)
    yt = np.swapaxes(y64, 1, 2)
    return np.matmul(x64, yt), np.matmul(np.abs(x64), np.abs(yt))


def bound_s(S, D):
    return (D + 4) * U * S


def bound_act(bs, a64):
    return bs + (4.0 + np.abs(a64)) * U


def forward_ref(x, y, kind):
    """-> (act64, bound, s64) for one tensor."""
    s, S = products64(x, y)
    a = act64(s, kind)
    return a, bound_act(bound_s(S, x.shape[-1]), a), s


def ratio(got, ref, bound):
    """max |got - ref| / bound; inf if anything is not finite where the reference is.  A bound of exactly zero (a zero
    cotangent, a factor that is exactly zero) asks for the exact value: 0 / 0 counts as 0, anything else / 0 as inf."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where((bound == 0) & (err == 0), 0.0, err / bound)
    if not np.isfinite(r).all():
        return float("inf")
    return float(r.max()) if r.size else 0.0


# --------------------------------------------------------------------------------------------------------------- backward
def ds_ref(g, act, kind):
    """dS from given fp32 outputs -> (dS64, bound): g * (1 - exp(-theta)) or g * (1 - exp(A))."""
    g64, a64 = np.asarray(g, np.float64), np.asarray(act, np.float64)
    f = -np.expm1(a64 if kind else -a64)
    return g64 * f, np.abs(g64) * ds_factor_bound(f, a64)


def ds_factor_bound(f, a64):
    return 8 * U * f + (np.abs(a64) >= SERIES_SWITCH) * 4 * U


def backward_ref(x, y, g, kind, act=None):
    """Gradients of sum(g * act(x . y^T)) in float64 -> ((dx, bound_dx), (dy, bound_dy)).

    act None: the factor comes from s64 and its error is the forward's (bound_fwd + 4u) -- for a backward that follows
    the kernel's own forward.  act given (the fp32 outputs handed to the kernel): the factor comes from them and its error
    is the dS bound."""
    x64, y64, g64 = (np.asarray(t, np.float64) for t in (x, y, g))
    N, M = x64.shape[1], y64.shape[1]
    if act is None:
        a, bf, s = forward_ref(x, y, kind)
        ds = g64 * factor64(s, kind)
        eds = np.abs(g64) * (bf + 4 * U)
    else:
        ds, eds = ds_ref(g, act, kind)
    ax, ay, ads = np.abs(x64), np.abs(y64), np.abs(ds)
    dx = np.matmul(ds, y64)                                     # contraction over M
    bx = np.matmul(eds, ay) + (M + 4) * U * np.matmul(ads, ay)
    dst, edst, adst = (np.swapaxes(t, 1, 2) for t in (ds, eds, ads))
    dy = np.matmul(dst, x64)                                    # contraction over N
    by = np.matmul(edst, ax) + (N + 4) * U * np.matmul(adst, ax)
    return (dx, bx), (dy, by)


# ----------------------------------------------------------------------------------------------------------- input families
def _base(seed, shape):
    return (0.5 + datagen.uniform(seed, shape, np.float64)).astype(np.float32)        # U[0.5, 1.5), exact in fp32


def _signs(seed, shape):
    return np.where(datagen.uniform(seed, shape) < 0.5, np.float32(-1), np.float32(1))


PLANTED = np.array([0.0, -0.0, 20.0, np.nextafter(np.float32(20), np.float32(30)), np.nextafter(np.float32(20), np.float32(0))], np.float32)


def make_inputs(family, seed, B, N, M, D, tensor=0):
    """(x, y) fp32, (B, N, D) and (B, M, D), of one tensor (0: zx, zy; 1: gx, gy).

    positive: U[0.5, 1.5) -- every product has the same sign, so a lost piece product of the three-piece GEMM is not
              hidden by cancellation (it is at random signs and D >= 128).  Its scores are all large and positive:
              softplus has slope 1 there and shows the loss in theta, logsigmoid is flat and hides it in A.
    negative: the same with y negated -- all scores large and negative, where A has slope 1 and theta is flat.
    signed:   the same with random signs.
    steep:    signed, rows of x scaled so that the scores leave the middle of the activations: row r = b N + i (+ tensor)
              is sign-matched to column 0 of its pair and scaled to a score there of < -40, < 0.25 or > 25 in turn (r % 3);
              its scores with the other columns are random-sign sums of the same scale.  Where N >= 4 and M >= 6, the last
              row of the last pair has ONE non-zero element (1.0), so its scores are single products: the last five columns
              get exact +0, -0, 20 and 20 -+ 1 ulp there (torch's softplus switches to the identity at 20)."""
    x, y = _base(seed, (B, N, D)), _base(seed + 1, (B, M, D))
    if family == "positive":
        return x, y
    if family == "negative":
        return x, -y
    x, y = x * _signs(seed + 2, x.shape), y * _signs(seed + 3, y.shape)
    if family == "signed":
        return x, y
    assert family == "steep", family
    # |x| . |y0| is in [0.25 D, 2.25 D]: -160 / D gives < -40, 0.1 / D gives < 0.225, 100 / D gives > 25
    scale = np.array([-160.0, 0.1, 100.0], np.float32) / np.float32(D)
    r = (np.arange(B * N).reshape(B, N) + tensor) % 3
    x = np.abs(x) * np.sign(y[:, :1, :]) * scale[r][:, :, None]
    x = x.astype(np.float32)
    if N >= 4 and M >= 6:
        d0 = D // 2
        x[B - 1, N - 1, :] = 0.0
        x[B - 1, N - 1, d0] = 1.0
        y[B - 1, M - 5:, d0] = PLANTED
    return x, y


# (B, N, M, D) of the GPU tests, by the forward build each is meant for on a 256-CU chip (sdp_api.hip, sdp_scores_f32)
FORWARD_CASES = {
    "sdp_scores_kernel": [(2, 1, 1, 1), (2, 5, 130, 3), (3, 127, 129, 15), (2, 129, 127, 17), (1, 128, 128, 33)],
    "sdp_scores_x6s_kernel": [(2, 1, 1, 16), (3, 127, 129, 16), (2, 129, 127, 32), (1, 128, 256, 48), (2, 130, 5, 64)],
    "sdp_scores_x6_kernel": [(300, 100, 97, 16), (300, 100, 100, 48)],
    "sdp_scores_x6w_kernel": [(256, 250, 254, 16), (256, 256, 256, 32), (140, 500, 500, 16)],
}
UNALIGNED_CASE = (2, 33, 70, 16)   # every embedding 4 bytes off a 16-byte boundary: sdp_scores_kernel although D % 16 == 0
BACKWARD_SHAPES = [(2, 40, 36, 260), (1, 300, 36, 20), (1, 20, 300, 20), (2, 17, 20, 16), (2, 33, 48, 32)]
BACKWARD_DROP_SHAPE = (2, 48, 44, 16)   # positive inputs and cotangents, contractions <= 48: a lost piece product shows

DS_VALUES = np.array([1e-30, 1e-7, 0.031, 0.03125, 0.0313, 1.0, 20.0, 100.0], np.float32)   # both sides of SERIES_SWITCH, and exactly on it


def ds_inputs(seed, B, N, M):
    """(g, theta, A) for the dS checks: theta is DS_VALUES tiled over the plane, A its negative, g is N(0, 1) (so some
    negative) with every seventh element zero."""
    n = B * N * M
    theta = DS_VALUES[np.arange(n) % len(DS_VALUES)].reshape(B, N, M)
    g = datagen.normal(seed, (B, N, M))
    g.reshape(-1)[::7] = 0.0
    return g, theta, -theta


def regions_present(s):
    """Do scores below -30, inside (-1, 1) and above 20 all occur?"""
    return bool((s < -30).any() and (np.abs(s) < 1).any() and (s > 20).any())


# ------------------------------------------------------------------------------------- the three-piece cut, emulated in numpy
PIECE_PAIRS = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))   # the six products the kernels form (sdp_scores.hip, PA / PB)


def cut3(x):
    """fp32 -> three bf16-representable pieces by truncation, as the kernels cut them: h0 = x & 0xffff0000,
    r1 = x - h0 (exact), h1 = r1 & 0xffff0000, h2 = r1 - h1 (exact, <= 8 significant bits)."""
    x = np.ascontiguousarray(x, np.float32)
    mask = np.uint32(0xffff0000)
    h0 = (x.view(np.uint32) & mask).view(np.float32)
    r1 = x - h0
    h1 = (r1.view(np.uint32) & mask).view(np.float32)
    h2 = r1 - h1
    return h0, h1, h2


def three_piece_product(x, y, drop=None):
    """sum over the six piece pairs (all but `drop`) of the float64 product of the pieces: the value the kernels' MFMAs
    would give with exact accumulation."""
    px, py = cut3(x), cut3(y)
    out = 0.0
    for pair in PIECE_PAIRS:
        if pair == drop:
            continue
        out = out + np.matmul(px[pair[0]].astype(np.float64), np.swapaxes(py[pair[1]].astype(np.float64), 1, 2))
    return out
