// sdp_targets.hip -- alignment training targets on the device (include/sdp.h: sdp_alignment_targets).
//
// Replaces what the reference builds per pair on the host inside AlignmentDataset.__getitem__
// (deepblast/dataset/dataset.py:157-179) and pads in collate_f (dataset/utils.py:254-279):
//   dm = states2matrix(states)                            utils.py:117-134
//   P  = path_distance_matrix(states2edges(states))       utils.py:315-339 (cKDTree over all n*m cells)
//   G  = gap_mask(st)                                     utils.py:393-409
//   reshape(x, len(gene), len(other))                     utils.py:465-473
//
// One wavefront per (pair, 64-column strip): every workgroup rescans the codes of its pair into LDS (row
// intervals [lo_r, hi_r] of the path and the code index of each row's first cell), then each lane owns one
// column and walks it top to bottom.  P is an exact separable distance transform (Meijster et al. 2000):
// the row pass is closed form from the intervals, g(r, c) = max(lo_r - c, c - hi_r, 0); the column pass
// builds the lower envelope of the parabolas (x - r)^2 + g(r, c)^2 down the column and reads it back bottom
// up.  The envelope's stack lives in the pair's own column of P (entry q at row q, packed s << 16 | t): an
// entry q is never read after row q has been written, because its start t_q >= q.  O(n) per column, integer
// arithmetic throughout, one correctly rounded square root per cell.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdp.h"
#include "sdp_kernels.h"

namespace {

// Correctly rounded sqrtf of an integer 0 <= d2 < 2^24 (bit-equal to the float64 square root rounded to float32,
// which is what the reference's cKDTree distance becomes in collate_f's float32 tensor).  v_sqrt_f32 alone is not
// correctly rounded: the estimate is moved to the float whose half-ulp neighbourhood holds sqrt(d2).  The midpoints
// between neighbouring floats have 25 significant bits and their squares 50, so the tests below are exact in
// float64, and no midpoint squares to an integer below 2^24 (no ties).
__device__ __forceinline__ float targets_sqrt(int d2)
{
    if (d2 == 0) return 0.0f;
    const double x = (double)d2;
    float y = __builtin_sqrtf((float)d2);
    for (int it = 0; it < 3; ++it) {
        const float up = __int_as_float(__float_as_int(y) + 1);
        const double mu = 0.5 * ((double)y + (double)up);
        if (mu * mu < x) {
            y = up;
            continue;
        }
        const float dn = __int_as_float(__float_as_int(y) - 1);
        const double md = 0.5 * ((double)y + (double)dn);
        if (md * md > x) {
            y = dn;
            continue;
        }
        break;
    }
    return y;
}

__device__ __forceinline__ int row_step(unsigned char c, bool trans) { return trans ? (c != '1') : (c != '2'); }
__device__ __forceinline__ int col_step(unsigned char c, bool trans) { return trans ? (c != '2') : (c != '1'); }

__device__ __forceinline__ int wave_sum(int v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

}  // namespace

// grid: strips * B workgroups of 64 lanes (pair b = blockIdx.x / strips, columns strip * 64 ..); dynamic LDS
// sdp::targets_lds_bytes(N, L)
__global__ void __launch_bounds__(sdp::TARGETS_TPB) sdp_targets_kernel(const uint8_t *codes, const int *code_lens, int L,
                                                                       const int *lens, int N, int M, int strips, float *dm,
                                                                       float *P, void *G, int flags, int *status)
{
    extern __shared__ unsigned char tg_lds[];
    unsigned short *lo = (unsigned short *)tg_lds;  // [N] first column of row r's path cells
    unsigned short *hi = lo + N;                     // [N] last column
    unsigned short *kst = hi + N;                    // [N] code index of the first path cell of row r
    unsigned char *cs = (unsigned char *)(kst + N);  // [L] the pair's codes

    const int b = blockIdx.x / strips, strip = blockIdx.x - b * strips;
    const int tid = threadIdx.x;
    const int Lb = code_lens[b];
    const bool len_ok = Lb >= 1 && Lb <= L;

    // ---- the pair's codes into LDS; extent of the path (state_diff_f: the step of state k >= 1 alone) ----
    int nx = 0, ny = 0;
    if (len_ok) {
        const uint8_t *src = codes + (size_t)b * L;
        for (int k = tid; k < Lb; k += sdp::TARGETS_TPB) {
            const unsigned char c = src[k];
            cs[k] = c;
            if (k > 0) {
                nx += c == '1';
                ny += c == '2';
            }
        }
    }
    nx = wave_sum(nx);
    ny = wave_sum(ny);
    const int n_e = Lb - ny, m_e = Lb - nx;  // 1 + #{k >= 1 : s_k != y}, 1 + #{k >= 1 : s_k != x}

    // ---- per-pair status: written as is (0), transposed (1, reshape's quirk), or refused (< 0) ----
    int st = 0;
    bool trans = false;
    if (!len_ok) {
        st = SDP_TARGETS_BAD_CODES;
    } else if (lens) {
        const int lg = lens[2 * b], lp = lens[2 * b + 1];
        if (n_e == lg && m_e == lp) trans = false;
        else if (m_e == lg && n_e == lp) trans = true;
        else st = SDP_TARGETS_BAD_LENS;
    }
    const int nr = trans ? m_e : n_e, nc = trans ? n_e : m_e;  // the block in output coordinates
    if (st == 0 && (nr > N || nc > M)) st = SDP_TARGETS_BAD_SHAPE;
    if (st == 0 && min(n_e, m_e) > SDP_TARGETS_MAX_SHORT_SIDE) st = SDP_TARGETS_TOO_LONG;
    if (strip == 0 && tid == 0) status[b] = st == 0 ? (int)trans : st;

    // ---- row intervals: one contiguous run of codes per lane, positions from a wave prefix sum ----
    if (st == 0) {
        const int seg = (Lb + sdp::TARGETS_TPB - 1) / sdp::TARGETS_TPB;
        const int k0 = min(tid * seg, Lb), k1 = min(k0 + seg, Lb);
        int own = 0;  // (rows, cols) advanced inside this lane's run, packed low / high 16 bits
        for (int k = max(k0, 1); k < k1; ++k) own += row_step(cs[k], trans) | (col_step(cs[k], trans) << 16);
        int incl = own;
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (tid >= o) incl += v;
        }
        int pos = incl - own;
        for (int k = k0; k < k1; ++k) {
            const int di = k > 0 ? row_step(cs[k], trans) : 1;
            if (k > 0) pos += di | (col_step(cs[k], trans) << 16);
            const int i = pos & 0xffff, j = pos >> 16;
            if (di) {
                lo[i] = (unsigned short)j;
                kst[i] = (unsigned short)k;
            }
            if (k == Lb - 1 || row_step(cs[k + 1], trans)) hi[i] = (unsigned short)j;
        }
    }
    __syncthreads();

    const int c = strip * sdp::TARGETS_TPB + tid;
    if (c >= M) return;
    const size_t base = (size_t)b * N * M + c;
    const bool gf32 = (flags & SDP_TARGETS_G_F32) != 0, gap = (flags & SDP_TARGETS_GAP_MASK) != 0;
    int *Pi = (int *)P;  // P and the envelope's stack: one type, so stores and loads of the two stay ordered
    auto put = [&](int r, float vdm, float vp, int vg) {
        const size_t o = base + (size_t)r * M;
        if (dm) dm[o] = vdm;
        if (P) Pi[o] = __float_as_int(vp);
        if (G) {
            if (gf32) ((float *)G)[o] = (float)vg;
            else ((uint8_t *)G)[o] = (uint8_t)vg;
        }
    };
    const bool live = st == 0 && c < nc;
    for (int r = live ? nr : 0; r < N; ++r) put(r, 0.0f, 0.0f, 0);  // padding (collate_f pads with zeros)
    if (!live) return;

    auto gcost = [&](int r) {  // squared horizontal distance from (r, c) to row r's path cells
        const int h = max(max((int)lo[r] - c, c - (int)hi[r]), 0);
        return h * h;
    };
    auto cell = [&](int r, float vp) {
        const int l = lo[r];
        const bool on = l <= c && c <= (int)hi[r];
        int vg = 1;
        if (gap) {
            const int k = kst[r] + (c - l);
            vg = on && (k == 0 || cs[k] == ':');  // gap_mask: ':' cells, and (0, 0) whatever its character (idx[0] = 1)
        }
        put(r, on ? 1.0f : 0.0f, vp, vg);
    };

    if (!P) {
        for (int r = 0; r < nr; ++r) cell(r, 0.0f);
        return;
    }

    // ---- column pass, forward: lower envelope of (x - r)^2 + g(r)^2, r < nr.  Stack entries 0 .. q-1 at rows 0 .. q-1
    // of this column (s << 16 | t), the top entry q in registers ----
    int *stk = Pi + base;
    const size_t rs = (size_t)M;
    int q = 0, ts = 0, tt = 0, fts = gcost(0);
    for (int u = 1; u < nr; ++u) {
        const int fu = gcost(u);
        for (;;) {
            const int a = tt - ts, d = tt - u;
            if (a * a + fts <= d * d + fu) break;
            if (q == 0) {
                q = -1;
                break;
            }
            --q;
            const int e = stk[q * rs];
            ts = e >> 16;
            tt = e & 0xffff;
            fts = gcost(ts);
        }
        if (q < 0) {
            q = 0;
            ts = u;
            tt = 0;
            fts = fu;
        } else {
            // Sep(ts, u): the last x at which parabola ts is not above parabola u (numerator >= 0: ts wins at tt >= 0)
            const int w = 1 + (u * u - ts * ts + fu - fts) / (2 * (u - ts));
            if (w < nr) {
                stk[q * rs] = (ts << 16) | tt;
                ++q;
                ts = u;
                tt = w;
                fts = fu;
            }
        }
    }
    // ---- backward: read the envelope bottom up, write every output of the row.  The entry below the top is loaded one
    // pop ahead: its row (< its start <= the top's start) is written only after it has been read ----
    int nxt = q > 0 ? stk[(q - 1) * rs] : 0;
    for (int u = nr - 1; u >= 0; --u) {
        const int du = u - ts;
        cell(u, targets_sqrt(du * du + fts));
        if (u == tt && q > 0) {
            --q;
            ts = nxt >> 16;
            tt = nxt & 0xffff;
            fts = gcost(ts);
            nxt = q > 0 ? stk[(q - 1) * rs] : 0;
        }
    }
}

// sdp_targets_selftest: every d2 in [0, 4096^2] through targets_sqrt, checked with integers alone.  r = Mr * 2^-k
// (Mr the 24-bit significand) is the correctly rounded sqrt(d2) iff (2 Mr - 1)^2 < d2 * 2^(2k+2) < (2 Mr + 1)^2.
__global__ void sdp_targets_selftest_kernel(int *bad)
{
    const int n = 4096 * 4096 + 1;
    int err = 0;
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
        const float r = targets_sqrt(v);
        const unsigned bits = __float_as_uint(r);
        if (v == 0) {
            err |= bits != 0u;
            continue;
        }
        const int ex = (int)((bits >> 23) & 0xff) - 127;
        if (bits >> 31 || ex < 0 || ex > 12) {  // 1 <= sqrt(v) <= 4096
            err = 1;
            continue;
        }
        const unsigned long long mr = (bits & 0x7fffffu) | 0x800000u;
        const int k = 23 - ex;  // r = mr * 2^-k, 11 <= k <= 23
        const unsigned long long lhs = (unsigned long long)v << (2 * k + 2);  // < 2^24 * 2^48: checked below
        if ((unsigned long long)v >= (1ull << (62 - 2 * k))) {
            err = 1;
            continue;
        }
        const unsigned long long a = 2 * mr - 1, c = 2 * mr + 1;
        err |= !(a * a < lhs && lhs < c * c);
    }
    if (err) atomicOr(bad, 1);
}
