"""numpy restatement of the soft local sampler (include/sdp.h: sdp_soft_local_end_tables_f32, sdp_soft_local_sample_paths_f32) --
TESTS ONLY.  Three parts: the end-cell tables (float64, and a float32 twin formed by the same sequential adds), the end draw from
given tables -- bit for bit as the header states it, in the tables' dtype -- and the walk from given records.  Then the brute
force that ties the draw to the distribution, the output formats, and the cases the CPU and the GPU tests share."""
import functools

import numpy as np

import sample_ref
import soft_local_ref

D, F = np.float64, np.float32


# ---- the tables ----
def tables64(V, Vt):
    """V (n, m): the cells' values (0-based), Vt a scalar -> (cdf (n, m), rows (n + 1,)) in float64"""
    V = np.asarray(V, D)
    cdf = np.cumsum(np.exp(V - D(Vt)), axis=1)
    rows = np.concatenate([[np.exp(-D(Vt))], np.exp(-D(Vt)) + np.cumsum(cdf[:, -1])]) if V.size else np.array([np.exp(-D(Vt))])
    return cdf, rows


def tables32(V, Vt):
    """the float32 twin: every exp, subtraction and add an fp32 operation, the adds sequential in increasing j, then in increasing i
    (numpy's accumulate is a plain loop) -> (cdf, rows) in float32"""
    V, Vt = np.asarray(V, F), F(Vt)
    w = np.exp(V - Vt)
    assert w.dtype == F
    cdf = np.add.accumulate(w, axis=1, dtype=F)
    rows = np.empty(V.shape[0] + 1, F)
    rows[0] = np.exp(-Vt)
    for i in range(V.shape[0]):
        rows[i + 1] = rows[i] + cdf[i, -1]
    return cdf, rows


# ---- the end draw ----
def first_index_scan(a, count, x):
    """the definition: the first index in [0, count) with x < a[index], or count - 1 if there is none"""
    for k in range(count):
        if x < a[k]:
            return k
    return count - 1


def first_index(a, count, x):
    """the kernel's search (csrc/sdp_soft_local_sample.hip: first_above), which equals the scan on a non-decreasing table"""
    lo, hi = 0, count
    while lo < hi:
        mid = (lo + hi) >> 1
        if x < a[mid]:
            hi = mid
        else:
            lo = mid + 1
    return lo if lo < count else count - 1


def end_draw(rows, cdf, n, m, u0, u1, first=first_index_scan):
    """rows (>= n + 1,), cdf (>= n, >= m) of ONE pair, in their own dtype (float32 read back from the device: the kernel's
    arithmetic bit for bit) -> the end cell (i, j), or (-1, -1) for the empty alignment"""
    if n < 1 or m < 1:
        return -1, -1
    dt = rows.dtype.type
    g = dt(u0) * rows[n]
    assert g.dtype == rows.dtype
    if g < rows[0]:
        return -1, -1
    i = first(rows[1:], n, g)
    h = dt(u1) * cdf[i, m - 1]
    return i, first(cdf[i], m, h)


# ---- the walk ----
def walk(q, i, j, us):
    """q (n, m, 3): the weights x, m, y of the 0-based cells, in q's dtype (the compares and the two adds are rounded in it); (i, j)
    the end cell; us[t] = U(.., t).  -> (cells [(i, j, state)] start first, the smallest distance of a uniform from a threshold it
    was compared with)"""
    dt = q.dtype.type
    rec, margin, t = [], np.inf, 2
    while i >= 0 and j >= 0:
        u = dt(us[t])
        qx, qm, qy = q[i, j, 0], q[i, j, 1], q[i, j, 2]
        xy = dt(qx + qy)
        xym = dt(xy + qm)
        margin = min(margin, abs(float(u) - float(qx)))
        if u < qx:
            rec.append((i, j, 0))
            i -= 1
        else:
            margin = min(margin, abs(float(u) - float(xy)))
            if u < xy:
                rec.append((i, j, 2))
                j -= 1
            else:
                margin = min(margin, abs(float(u) - float(xym)))
                if u < xym:
                    rec.append((i, j, 1))
                    i, j = i - 1, j - 1
                else:
                    rec.append((i, j, 1))      # the start cell: it pays no gap score and is named m
                    break
        t += 1
    return rec[::-1], margin


def clamp_lens(lens, B, N, M):
    """(n, m) of every pair as the kernels take them: clamped to the tensor, and (0, 0) for a pair without a cell"""
    if lens is None:
        return [(N, M)] * B
    out = [(min(max(int(a), 0), N), min(max(int(b), 0), M)) for a, b in np.asarray(lens)]
    return [(n, m) if n >= 1 and m >= 1 else (0, 0) for (n, m) in out]


def batch(qs, N, M, K, lens=None, seed=0, sample0=0, tables=None, ends=None):
    """qs[b]: (>= n_b, >= m_b, 3) weights of pair b.  The end cells come from `ends` (B, K, 2) where given -- the GPU tests hand over
    what the device drew -- else from end_draw on tables[b] = (cdf, rows).  -> dict: lists[b][k] (the path, start first), ends
    (B, K, 2), margin (B, K) (inf for an empty sample), visits (B, N, M) int32"""
    B = len(qs)
    out = {"lists": [], "ends": np.full((B, K, 2), -1, np.int32), "margin": np.full((B, K), np.inf),
           "visits": np.zeros((B, N, M), np.int32)}
    for b, (n, m) in enumerate(clamp_lens(lens, B, N, M)):
        row = []
        for k in range(K):
            us = sample_ref.uniforms(seed, b, sample0 + k, n + m + 2)
            if ends is not None:
                i, j = (int(v) for v in ends[b, k])
            else:
                cdf, rws = tables[b]
                i, j = end_draw(rws, cdf, n, m, us[0], us[1])
            out["ends"][b, k] = (i, j)
            lst, margin = walk(qs[b], i, j, us) if i >= 0 else ([], np.inf)
            row.append(lst)
            out["margin"][b, k] = margin
            for (ci, cj, _) in lst:
                out["visits"][b, ci, cj] += 1
        out["lists"].append(row)
    return out


def right_aligned(ref, N, M):
    """ref of batch() in the kernel's own output format: (states (B, K, cap, 3) with the lists at rows cap-1-count .. cap-2 and
    (count, first i, first j) in row cap-1, counts (B, K), mask (B, K, cap) of the rows that are specified)"""
    B, K = ref["margin"].shape
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
            st[b, k, cap - 1] = (c, lst[0][0], lst[0][1]) if c else (0, -1, -1)
            on[b, k, cap - 1 - c:] = True
    return st, cn, on


def left_aligned(ref, N, M):
    """... and in SoftLocalDecoder.sample_paths' format: the lists at rows 0 .. count-1"""
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


# ---- the brute force: every non-empty local path, enumerated as soft_local_ref.brute_force enumerates them ----
def all_local_paths(theta, A):
    """-> [(cells [(i, j, state it was entered through; 1 for the start)] start first, score)]"""
    theta, A = np.asarray(theta, D), np.asarray(A, D)
    n, m = theta.shape
    out = []

    def extend(cells, score):
        out.append((cells, score))
        i, j, _ = cells[-1]
        for k, (ni, nj) in enumerate(((i + 1, j), (i + 1, j + 1), (i, j + 1))):
            if ni < n and nj < m:
                extend(cells + [(ni, nj, k)], score + theta[ni, nj] + (A[ni, nj] if k != 1 else 0.0))

    for i in range(n):
        for j in range(m):
            extend([(i, j, 1)], theta[i, j])
    return out


def path_probability(w, q, cells):
    """the probability the draw gives a path: w[end] x the chosen q of every cell but the first x the stop weight of the first"""
    i, j, _ = cells[-1]
    p = w[i, j]
    for (ci, cj, s) in cells[1:]:
        p *= q[ci, cj, s]
    i, j, _ = cells[0]
    return p * (1.0 - q[i, j].sum())


# ---- the cases the CPU and the GPU tests share ----
DELTAS = (1e-6, 3e-6, 1e-5, 3e-5)
# measured on MI355X over all cases below: the smallest of DELTAS at which every compared walk matches is MEASURED_DELTA; the tests
# use the next value up
MEASURED_DELTA = 1e-6
DELTA = 3e-6
SEED = 2025
FAMILIES = ("floor", "drift", "model", "steep")
LENS = ((0, 7), (1, 1), (130, 150), (65, 33), (127, 145))
# name -> (family, B, N, M, K, lens, what is done to the scores)
CASES = {f"{f}-{n}x{m}": (f, 3, n, m, 64, None, None)
         for (n, m) in ((1, 1), (1, 33), (63, 31), (64, 32), (65, 33)) for f in FAMILIES}
CASES.update({
    "drift-130x150": ("drift", 3, 130, 150, 64, None, None),          # three strips, five chunks
    "islands-130x150": ("islands", 3, 130, 150, 64, None, None),
    "cold-5x7": ("drift", 3, 5, 7, 64, None, "cold"),                 # theta - 4: the empty alignment takes a large share
    "lens-130x150": ("drift", len(LENS), 130, 150, 64, LENS, None),
    "k70-65x33": ("model", 3, 65, 33, 70, None, None),                # a partial second wave
    "masked-65x33": ("model", 3, 65, 33, 64, None, "masked"),         # A = -inf on 30 % of the cells
    "wide-449x1983": ("islands", 1, 449, 1983, 64, None, None),       # seven waves; strip 7 is wave 0's second strip
})


@functools.lru_cache(maxsize=None)
def scores(name):
    """-> (theta, A) fp32 (B, N, M) of a case, read-only"""
    family, B, N, M, K, lens, twist = CASES[name]
    th, a = soft_local_ref.family(family, 4000 + 7 * N + M, B, N, M)
    th, a = th.copy(), a.copy()
    if twist == "cold":
        th -= F(4.0)
    if twist == "masked":
        a[np.random.RandomState(16).rand(*a.shape) < 0.3] = -np.inf
    th.setflags(write=False), a.setflags(write=False)
    return th, a


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 definition of a case, computed once: per pair (n, m, Vt, V (n, m), q (n, m, 3), cdf, rows), over its own block"""
    family, B, N, M, K, lens, twist = CASES[name]
    th, a = scores(name)
    fwd = soft_local_ref.forward if N * M <= 4096 else soft_local_ref.forward_wavefront
    out = []
    for b, (n, m) in enumerate(clamp_lens(lens, B, N, M)):
        if n < 1 or m < 1:
            out.append((n, m, D(0), np.zeros((0, 0)), np.zeros((0, 0, 3)), np.zeros((0, 0)), np.array([1.0])))
            continue
        Vt, V, q = fwd(th[b:b + 1, :n, :m], a[b:b + 1, :n, :m])
        V, q = np.ascontiguousarray(V[0, 1:-1, 1:-1]), np.ascontiguousarray(q[0, 1:-1, 1:-1])
        cdf, rows = tables64(V, Vt[0])
        for x in (V, q, cdf, rows):
            x.setflags(write=False)
        out.append((n, m, Vt[0], V, q, cdf, rows))
    return out


@functools.lru_cache(maxsize=None)
def reference_walks(name, seed=0):
    """the float64 reference's own samples of a case (end cells from the float64 tables) -> batch()'s dict"""
    family, B, N, M, K, lens, twist = CASES[name]
    ref = reference(name)
    return batch([r[4] for r in ref], N, M, K, lens, seed=seed, tables=[(r[5], r[6]) for r in ref])
