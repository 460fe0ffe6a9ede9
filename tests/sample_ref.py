"""numpy restatement of the sampler (include/sdp.h: sdp_sample_paths_*) -- TESTS ONLY: the Philox4x32-10 generator, the
stochastic traceback on a given Q, the padding, the visit counts, and the brute force that ties the walk to the posterior."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xffffffff

# (counter, key, output) of Philox4x32-10: the known answers of the Random123 distribution
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox(counter, key):
    """Philox4x32-10 on python ints or on uint64 arrays that hold 32-bit values -> the four output words"""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) for c in counter)
    k0, k1 = (np.asarray(k, np.uint64) for k in key)
    m = np.uint64(MASK)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m, (p0 >> s32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return c0, c1, c2, c3


def uniforms(seed, pair, sample, steps):
    """U(seed, pair, sample, t) for t = 0 .. steps-1 -> float32 array (exact multiples of 2^-24)"""
    groups = (steps + 3) // 4
    g = np.arange(groups, dtype=np.uint64)
    z = np.zeros(groups, np.uint64)
    words = philox((g, z + np.uint64(sample & MASK), z + np.uint64(pair & MASK), z), (np.uint64(seed & MASK), np.uint64((seed >> 32) & MASK)))
    w = np.stack(words, axis=1).reshape(-1)[:steps]
    return ((w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def uniform(seed, pair, sample, t):
    return uniforms(seed, pair, sample, t + 1)[t]


def walk(Q, n, m, lo, seed, pair, sample, transposed=False):
    """One sample on Q (rows, cols, 3), the weights x, m, y of the 0-based cells, in Q's dtype (the compares and the one add are
    rounded in it).  -> (list of (i, j, s) start first, padding included; number of path cells; the first path cell (i, j), or
    the padding's start where there is none; the smallest distance of a uniform from a threshold it was compared with)"""
    dt = Q.dtype.type
    us = uniforms(seed, pair, sample, n + m)
    rec = []
    i, j, t = n, m, 0
    li, lj = n - 1, m - 1
    margin = np.inf
    while i >= lo and j >= lo:
        u = dt(us[t])
        qx, qy = Q[i - 1, j - 1, 0], Q[i - 1, j - 1, 2]
        both = dt(qx + qy)
        if transposed:      # the column step takes the first interval and is named x
            first = qy
            s = 0 if u < first else (2 if u < both else 1)
            row, col = s == 2, s == 0
        else:
            first = qx
            s = 0 if u < first else (2 if u < both else 1)
            row, col = s == 0, s == 2
        margin = min(margin, abs(float(u) - float(first)), abs(float(u) - float(both)))
        li, lj = i - 1, j - 1
        rec.append((li, lj, s))
        i -= 0 if col else 1
        j -= 0 if row else 1
        t += 1
    npath, first_cell = len(rec), (li, lj)
    if transposed:
        while lj > 0:
            lj -= 1
            rec.append((li, lj, 0))
        while li > 0:
            li -= 1
            rec.append((li, lj, 2))
    else:
        while li > 0:
            li -= 1
            rec.append((li, lj, 0))
        while lj > 0:
            lj -= 1
            rec.append((li, lj, 2))
    return rec[::-1], npath, first_cell, margin


def clamp_lens(lens, B, N, M):
    if lens is None:
        return [(N, M)] * B
    return [(min(max(int(a), 1), N), min(max(int(b), 1), M)) for a, b in np.asarray(lens)]


def batch(Qs, N, M, K, variant, lens=None, seed=0, sample0=0, transposed=False):
    """Qs[b]: (>= n_b, >= m_b, 3) weights of pair b.  -> dict: lists[b][k], npath, first, margin (B, K), visits (B, N, M) int32"""
    B = len(Qs)
    lo = 2 if variant else 1
    out = {"lists": [], "npath": np.zeros((B, K), np.int32), "first": np.zeros((B, K, 2), np.int32),
           "margin": np.zeros((B, K)), "visits": np.zeros((B, N, M), np.int32)}
    for b, (n, m) in enumerate(clamp_lens(lens, B, N, M)):
        row = []
        for k in range(K):
            lst, npath, first, margin = walk(Qs[b], n, m, lo, seed, b, sample0 + k, transposed)
            row.append(lst)
            out["npath"][b, k], out["first"][b, k], out["margin"][b, k] = npath, first, margin
            for (i, j, _) in lst[len(lst) - npath:]:
                out["visits"][b, i, j] += 1
        out["lists"].append(row)
    return out


def right_aligned(ref, N, M):
    """ref of batch() in the kernel's own output format: (states (B, K, cap, 3) with the lists at rows cap-1-count .. cap-2 and
    (npath, first i, first j) in row cap-1, counts (B, K), mask (B, K, cap) of the rows that are specified)"""
    B, K = ref["npath"].shape
    cap = N + M + 2
    st = np.zeros((B, K, cap, 3), np.int32)
    cn = np.zeros((B, K), np.int32)
    on = np.zeros((B, K, cap), bool)
    for b in range(B):
        for k in range(K):
            lst = ref["lists"][b][k]
            c = len(lst)
            cn[b, k] = c
            if c:
                st[b, k, cap - 1 - c:cap - 1] = np.asarray(lst, np.int32)
            st[b, k, cap - 1] = (ref["npath"][b, k], *ref["first"][b, k])
            on[b, k, cap - 1 - c:] = True
    return st, cn, on


def left_aligned(ref, N, M):
    """... and in Decoder.sample_paths' format: the lists at rows 0 .. count-1"""
    st, cn, _ = right_aligned(ref, N, M)
    B, K, cap, _ = st.shape
    out = np.zeros_like(st)
    on = np.zeros((B, K, cap), bool)
    for b in range(B):
        for k in range(K):
            c = cn[b, k]
            out[b, k, :c] = st[b, k, cap - 1 - c:cap - 1]
            out[b, k, cap - 1] = st[b, k, cap - 1]
            on[b, k, :c] = True
            on[b, k, cap - 1] = True
    return out, cn, on


def inner(q):
    """the reference's padded (1, n+2, m+2, 3) weights -> (n, m, 3): cell (i, j), 1-based, at [i-1, j-1]"""
    return np.ascontiguousarray(q[0, 1:-1, 1:-1, :])


def all_paths(n, m, lo):
    """every path the walk can take from (n, m) until i < lo or j < lo, as lists of (i, j, s), 1-based, end first"""
    out = []

    def go(i, j, acc):
        if i < lo or j < lo:
            out.append(acc)
            return
        for s in (0, 1, 2):
            go(i - (s != 2), j - (s != 0), acc + [(i, j, s)])
    go(n, m, [])
    return out


def path_weight(Q, path):
    """the probability the walk gives a path: the product of the chosen weights (Q: (n, m, 3), match weight = 1 - x - y taken
    from the table itself)"""
    w = 1.0
    for (i, j, s) in path:
        w *= Q[i - 1, j - 1, s]
    return w
