// sdp_aux.hip -- the small kernels beside the sweep (declared in sdp_kernels.h, launched by sdp_api.hip): launch order and dispatch
// map of variable-length batches, bridge reset, batched traceback, masked alignment losses, device self-test.  gfx950.
#include "sdp_device.h"

#ifndef SDP_TB_WINDOW
#define SDP_TB_WINDOW 32  // traceback: edge of the LDS window of E (32 or 64 cells)
#endif

// ----------------------------------------------------------------------------------
// launch order for variable-length batches: order[r] = the pair with the r-th largest n*m (ties: lower index first).
// Rank by counting -- B is at most a few thousand, the (B,2) lengths sit in L2 -- so no sort, no scratch memory.
// ----------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256) sdp_order_kernel(const int *lens, int *order, int B, int N, int M)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    auto work = [&](int i) {
        int n = lens[2 * i], m = lens[2 * i + 1];
        n = n < 1 ? 1 : (n > N ? N : n);
        m = m < 1 ? 1 : (m > M ? M : m);
        return n * m;
    };
    const int mine = work(b);
    int rank = 0;
    for (int i = 0; i < B; ++i) {
        const int w = work(i);
        rank += (w > mine || (w == mine && i < b)) ? 1 : 0;
    }
    order[rank] = b;
}

// ----------------------------------------------------------------------------------
// bridge rows of a parts launch: every granule "not written yet" (sdp_kernels.h: XB_INVALID in both words)
// ----------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256) sdp_bridge_reset_kernel(unsigned long long *xb, size_t n8)
{
    const unsigned long long pattern = ((unsigned long long)sdp::XB_INVALID << 32) | sdp::XB_INVALID;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) xb[i] = pattern;
}

// ----------------------------------------------------------------------------------
// dispatch order when pairs are spread over several workgroups ("parts") and have their own lengths: map[h] = pair *
// nparts_max + part for workgroup h.  Workgroups are handed to CUs in index order as CUs free up, and a part that is on
// a CU before its producer has reached it only waits there.  So: every pair's part 0 first, then the parts 1, ... -- part
// k has nothing to do for the first k * 4 * 79 steps (~60 us each) of its pair, about the time the shortest pairs of the
// batch take to leave their CUs -- and within one k by the critical path that still hangs on the part, longest first
// ((P - 1 - k) * 4 * 79 + 3 * 79 + m + 63 steps for a pair of P parts and m columns).  A producer always precedes its
// consumer, so a waiting part never keeps its producer off the chip.  (Ranking by the critical path alone put all parts
// of the long pairs on CUs at once, most of them waiting: forward sweep of BASELINE configs[2] 600 us instead of 511.)
// Slots k of pairs with k parts or fewer come at the end of the parts k: in the forward sweep they exit at once, in the
// backward sweep they zero-fill E outside the pair's block (sorted behind everything else the fill ran at the very end,
// on the few CUs that were free: 483 instead of 3xx us).  Rank by counting, as above.
// ----------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256) sdp_parts_map_kernel(const int *lens, int *map, int B, int N, int M, int nparts_max, int strips)
{
    // one wavefront per workgroup-to-be: its 64 lanes share the scan over the list (ranking 1024 parts with one thread
    // each took ~50 us -- a tenth of the sweep it was meant to speed up)
    const int h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int total = B * nparts_max;
    if (h >= total) return;
    auto key = [&](int e) {
        const int pr = e / nparts_max, k = e % nparts_max;
        int n = lens[2 * pr], m = lens[2 * pr + 1];
        n = n < 1 ? 1 : (n > N ? N : n);
        m = m < 1 ? 1 : (m > M ? M : m);
        const int np = ((n + 63) / 64 + strips - 1) / strips;
        return (nparts_max - k) * 65536 + (k < np ? (np - 1 - k) * strips * 79 + (strips - 1) * 79 + m + 63 : 0);
    };
    const int mine = key(h);
    int cnt = 0;
    for (int e = lane; e < total; e += 64) {
        const int w = key(e);
        cnt += (w > mine || (w == mine && e < h)) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) map[cnt] = h;
}

// ----------------------------------------------------------------------------------
// batched traceback: the reference's greedy arg-max walk (deepblast/nw.py:401-444,
// sw.py:328-371).  Integer work, bit-identical to the host version in deepblast_amd/_dp.py::traceback,
// including Python's negative-index wrap when exactly one of (i, j) is 0; a walk that leaves the matrix
// (the reference raises IndexError) sets count = -1.
//
// One wavefront per pair.  The walk is a chain of <= N+M dependent steps, each reading three neighbours of the
// current cell; one lane per pair with three global loads per step (round 1) paid a full memory latency per step --
// 0.9 ms at 256 x 512 x 512, more than twice the two sweeps that produce E.  Here the wave keeps the 32 x 32 window
// of E whose bottom-right corner is the current cell in LDS (16 coalesced loads per lane, all in flight together);
// the walk only moves up and left, so it stays inside for 31 ... 62 steps, each three LDS broadcasts and a few scalar
// compares, before the window is re-centred.  Steps are collected one per lane and written 64 at a time from the END
// of the pair's buffer backwards (the reference returns the walk reversed; its length is not known in advance), then
// the wave moves them to the front.  The window is filled through python's index wrap, so the top row / left column
// (floor values, reads that wrap to the opposite edge) and already-wrapped walks use the same loop.
// ----------------------------------------------------------------------------------
// RULE 0: the CPU reference's walk (nw.py:401-444: stop when ALL three neighbours are off the matrix, sentinel -1e5,
// python's index wrap).  RULE 1: the walk of the reference's GPU classes (nw_cuda.py:273-317, sw_cuda.py:283-327: stop
// as soon as ANY neighbour is off the matrix -- or holds the sentinel -1e10; no wrap, never an IndexError).
template <int RULE>
__device__ __forceinline__ void traceback_walk(const float *grad, int *states, int *counts, const int *lens, int B, int N, int M, int cap)
{
    constexpr int TW = SDP_TB_WINDOW, TWL = TW == 64 ? 6 : 5;   // window edge (32 or 64 cells)
    __shared__ float tile[TW * TW];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    int n = N, m = M;
    if (lens) {
        n = __builtin_amdgcn_readfirstlane(lens[2 * b]);
        m = __builtin_amdgcn_readfirstlane(lens[2 * b + 1]);
        n = n < 1 ? 1 : (n > N ? N : n);
        m = m < 1 ? 1 : (m > M ? M : m);
    }
    const float *g = grad + (size_t)b * N * M;
    int *out = states + (size_t)b * cap * 3;
    const float floor_v = RULE ? -1e10f : -100000.f;
    // A walk has at most n + m - 1 steps: every step lowers i or j, a step that lowers only i needs i > 0, and j never
    // goes below 0.  The API passes cap = N + M + 2.
    if (cap < n + m) {
        if (lane == 0) counts[b] = -1;
        return;
    }
    bool bad = false;
    // every value the walk branches on is the same in all 64 lanes, but a load (LDS or global) is a divergent source to
    // the compiler: these keep the control flow scalar
    auto uni = [](float v) -> float { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    auto all = [](bool c) -> bool { return __builtin_amdgcn_ballot_w64(c) != 0; };   // c is uniform: any lane == all lanes
    // Steps are recorded as their state only, one per lane; a step moves by (state != 2, state != 0), so the positions
    // of a group of 64 follow from the position before the group and two prefix counts (the first record, state 1 at
    // (n-1, m-1), is "a diagonal step from (n, m)").  Groups go to the END of the pair's buffer, last step first.
    int cnt = 0, my_s = 0;
    int base_i = n, base_j = m;   // position before the first step of the current group
    auto flush = [&](int first, int count, int now_i, int now_j) {  // steps first .. first+count-1 -> positions cap-1-step
        const bool mine = lane < count;
        const unsigned long long mi = __builtin_amdgcn_ballot_w64(mine && my_s != 2), mj = __builtin_amdgcn_ballot_w64(mine && my_s != 0);
        const int pi = __builtin_amdgcn_mbcnt_hi((unsigned)(mi >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mi, 0)) + (int)((mi >> lane) & 1);
        const int pj = __builtin_amdgcn_mbcnt_hi((unsigned)(mj >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mj, 0)) + (int)((mj >> lane) & 1);
        if (mine) {
            int *o = out + 3 * (size_t)(cap - 1 - (first + lane));
            o[0] = base_i - pi, o[1] = base_j - pj, o[2] = my_s;
        }
        base_i = now_i, base_j = now_j;
    };
    auto record = [&](int st, int now_i, int now_j) {  // now = the position after this step
        if (lane == (cnt & 63)) my_s = st;
        ++cnt;
        if ((cnt & 63) == 0) flush(cnt - 64, 64, now_i, now_j);
    };

    // The walk in "virtual" coordinates: i and j only decrease and may go below 0, where python's indexing wraps them
    // to the other edge (nw.py:423 reads grad[i-1, j-1] with i = 0 or j = 0) -- at most once (below -n / -m the
    // reference raises IndexError: bad).  left is off the matrix for i <= 0, upper for j <= 0, all three for both.
    // The window is filled through the same wrap, so one loop serves the interior, the edges and the wrapped walk.
    int i = n - 1, j = m - 1;
    record(1, i, j);
    while (true) {
        if (RULE ? (i <= 0 || j <= 0) : (i <= 0 && j <= 0)) break;   // the reference's stop rule (all three / any one off the matrix)
        const int r0 = i - (TW - 1), c0 = j - (TW - 1);
        __syncthreads();  // one wave: orders the LDS reads of the old window before these writes
        {
            float v[TW * TW / 64];
            int vj = c0 + (lane & (TW - 1));
            vj += vj < 0 ? m : 0;
            const bool okj = vj >= 0;
#pragma unroll
            for (int k = 0; k < TW * TW / 64; ++k) {
                int vi = r0 + (lane >> TWL) + (64 / TW) * k;
                vi += vi < 0 ? n : 0;
                // rows / columns below -n / -m are never read (see `bad` below): clamped address, so that all loads
                // are in flight together
                v[k] = __builtin_nontemporal_load(g + (size_t)max(vi, 0) * M + (okj ? vj : 0));
            }
#pragma unroll
            for (int k = 0; k < TW * TW / 64; ++k) tile[((lane >> TWL) + (64 / TW) * k) * TW + (lane & (TW - 1))] = v[k];
        }
        __syncthreads();
        int ti = TW - 1, tj = TW - 1;   // the current cell; the walk stays in the window while both are >= 1
        bool stop = false;
        if (TW == 32 && r0 >= 0 && c0 >= 0) {
            // ---- the whole window is inside the matrix: no floor values, no wrap (round 6) ----
            // Which way a cell sends the walk depends on the cell alone, so the choices of all 31 x 31 cells of the window are made at
            // once -- the same three comparisons per cell as in the loop below, sixteen cells per lane -- and kept as two bits per cell
            // (0 / 1 / 2: the step; 3: the sentinel rule says stop) in ONE register: lane c + 32 h holds column c, rows 16 h .. 16 h + 15.
            // A step of the walk is then a v_readlane, a shift and a few scalar instructions -- no LDS round trip and no ballot in
            // the chain of <= N + M dependent steps (it was three broadcast reads and three ballots per step: ~360 cycles).
            const int cc = lane & 31, hh = lane >> 5;
            float colv[17];   // rows 16 hh - 1 .. 16 hh + 15 of column cc (row -1 is never a current cell's: clamped)
#pragma unroll
            for (int k = 0; k < 17; ++k) colv[k] = tile[max(16 * hh - 1 + k, 0) * TW + cc];
            unsigned code = 0;
#pragma unroll
            for (int k = 1; k < 17; ++k) {
                // cell (r, cc), r = 16 hh + k - 1: left = (r - 1, cc), diag = (r - 1, cc - 1), upper = (r, cc - 1); column cc - 1 is the
                // lane below's (column 0 has no current cells: the walk leaves the window at tj = 0)
                const float left = colv[k - 1];
                const float diag = __int_as_float(sdp::dpp_i32<sdp::DPP_WAVE_SHR1>(0, __float_as_int(colv[k - 1])));
                const float upper = __int_as_float(sdp::dpp_i32<sdp::DPP_WAVE_SHR1>(0, __float_as_int(colv[k])));
                const bool c1 = diag > left;
                const float bv1 = c1 ? diag : left;
                const bool c2 = upper > bv1;
                const bool halt = RULE ? (left == floor_v || diag == floor_v || upper == floor_v)
                                       : (left == floor_v && diag == floor_v && upper == floor_v);
                code |= (halt ? 3u : (c2 ? 2u : (c1 ? 1u : 0u))) << (2 * (k - 1));
            }
            // The steps themselves run in segments of at most 32 that end where a group of 64 records is complete: inside a segment
            // the states collect in a scalar (two bits per step) and nothing but the look-up, the move and the loop test is in the
            // chain; the lanes take their records -- and a complete group leaves -- between segments.
            while (true) {
                const int cnt0 = cnt;
                const int room = 64 - (cnt0 & 63), lim = room < 32 ? room : 32;
                unsigned long long acc = 0;
                int k = 0;
                bool halted = false;
                while (ti >= 1 && tj >= 1 && k < lim) {
                    const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)code, tj + 32 * (ti >> 4));
                    const int st = (int)((w >> (2 * (ti & 15))) & 3u);
                    if (st == 3) {
                        halted = true;
                        break;
                    }
                    ti -= st == 2 ? 0 : 1;
                    tj -= st == 0 ? 0 : 1;
                    acc = (acc << 2) | (unsigned long long)st;
                    ++k;
                }
                // step t of the segment (0 = first) sits in bits 2 (k - 1 - t) of acc; its record belongs to lane (cnt0 + t) mod 64
                const int t = (lane - cnt0) & 63;
                if (t < k) my_s = (int)((acc >> (2 * (k - 1 - t))) & 3ull);
                cnt = cnt0 + k;
                if (k > 0 && (cnt & 63) == 0) flush(cnt - 64, 64, r0 + ti, c0 + tj);
                if (halted) {
                    stop = true;
                    break;
                }
                if (!(ti >= 1 && tj >= 1)) break;
            }
        } else if (r0 >= 0 && c0 >= 0) {
            // ---- the same for the other window size: three LDS broadcasts and the comparisons per step ----
            while (ti >= 1 && tj >= 1) {
                const float *p = tile + ti * TW + tj;
                const float left = p[-TW], diag = p[-TW - 1], upper = p[-1];
                const bool c1 = all(diag > left);
                const float bv1 = c1 ? diag : left;
                const bool c2 = all(upper > bv1);
                const float bv = c2 ? upper : bv1;
                if constexpr (RULE) {
                    if (all(left == floor_v || diag == floor_v || upper == floor_v)) {   // a stored value equal to the sentinel stops the walk too
                        stop = true;
                        break;
                    }
                } else if (all(bv == floor_v)) {   // only then can all three be the floor value
                    if (all(left == floor_v && diag == floor_v && upper == floor_v)) {
                        stop = true;
                        break;
                    }
                }
                ti -= c2 ? 0 : 1;
                tj -= (c1 || c2) ? 1 : 0;
                record(c2 ? 2 : (c1 ? 1 : 0), r0 + ti, c0 + tj);
            }
        } else {
            while (ti >= 1 && tj >= 1) {
                const int vi = r0 + ti, vj = c0 + tj;
                const bool fl = vi <= 0, fu = vj <= 0;
                if (RULE ? (fl || fu) : (fl && fu)) {
                    stop = true;
                    break;
                }
                if (vi - 1 < -n || vj - 1 < -m) {   // the diagonal read would wrap twice: IndexError in the reference
                    bad = true;
                    break;
                }
                const float *p = tile + ti * TW + tj;
                const float t0 = p[-TW], t1 = p[-TW - 1], t2 = p[-1];
                const float left = fl ? floor_v : uni(t0), diag = uni(t1), upper = fu ? floor_v : uni(t2);
                if (RULE ? (left == floor_v || diag == floor_v || upper == floor_v) : (left == floor_v && diag == floor_v && upper == floor_v)) {
                    stop = true;
                    break;
                }
                int best = 0;
                float bv = left;
                if (diag > bv) best = 1, bv = diag;
                if (upper > bv) best = 2, bv = upper;
                ti -= best == 2 ? 0 : 1;
                tj -= best == 0 ? 0 : 1;
                record(best, r0 + ti, c0 + tj);
            }
        }
        i = r0 + ti, j = c0 + tj;
        if (stop || bad) break;
    }
    while (!bad && i > 0) {
        i -= 1;
        record(0, i, j);
    }
    while (!bad && j > 0) {
        j -= 1;
        record(2, i, j);
    }
    if (bad) {
        if (lane == 0) counts[b] = -1;
        return;
    }
    flush(cnt & ~63, cnt & 63, i, j);
    // the wave reads back what its own lanes stored: workgroup scope is enough (an agent-scope fence writes back and
    // invalidates the L2 on this chip -- tens of microseconds each)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    // steps sit reversed at out[cap-cnt .. cap): move them to the front (ascending groups of 64 never write where a
    // later group still has to read: the source is always at or above the destination)
    const int shift = cap - cnt;
    if (shift > 0) {
        for (int k0 = 0; k0 < cnt; k0 += 64) {
            const int k = k0 + lane;
            int v0 = 0, v1 = 0, v2 = 0;
            if (k < cnt) {
                const int *src = out + 3 * (size_t)(shift + k);
                v0 = __builtin_nontemporal_load(src), v1 = __builtin_nontemporal_load(src + 1), v2 = __builtin_nontemporal_load(src + 2);
            }
            __syncthreads();
            if (k < cnt) {
                int *dst = out + 3 * (size_t)k;
                dst[0] = v0, dst[1] = v1, dst[2] = v2;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        }
    }
    if (lane == 0) counts[b] = cnt;
}

extern "C" __global__ void __launch_bounds__(64) sdp_traceback_kernel(const float *grad, int *states, int *counts,
                                                                      const int *lens, int B, int N, int M, int cap)
{
    traceback_walk<0>(grad, states, counts, lens, B, N, M, cap);
}
extern "C" __global__ void __launch_bounds__(64) sdp_traceback_cuda_kernel(const float *grad, int *states, int *counts,
                                                                           const int *lens, int B, int N, int M, int cap)
{
    traceback_walk<1>(grad, states, counts, lens, B, N, M, cap);
}

// ----------------------------------------------------------------------------------
// masked alignment losses: the reference evaluates its losses with a Python loop over the
// batch -- slice [:x_len, :y_len], masked_select by G, reduce (deepblast/losses.py:9-48, 51-79, 82-118).
// Here one launch reduces every pair (one workgroup per pair, float64 accumulation, deterministic
// order), and one launch writes the gradient w.r.t. the predicted matrix.
//   kind 0 MatrixCrossEntropy : acc = sum_G [ Yt log p + (1-Yt) log(1-p) ],  p = clamp(Yp, 3e-8, 1-3e-8)
//   kind 1 SoftPathLoss       : acc = sum_G (P * Yp)^2
//   kind 2 SoftAlignmentLoss  : acc = sum_G (Yt - Yp)^2
// HBM-bound elementwise work: 12 B read per cell in the forward, 12 B read + 4 B written in the backward.
// ----------------------------------------------------------------------------------
// One workgroup per pair; a thread takes four consecutive columns of a row per iteration (one 16-byte load per
// tensor when every row of every tensor is 16-byte aligned: M a multiple of 4 and 16-byte aligned base pointers, which
// the host decides and passes as `vec4`), so the three tensors stream at full width and there is one index division per
// four cells.  Per-thread float64 partial sums, fixed reduction order: deterministic.
extern "C" __global__ void __launch_bounds__(1024) sdp_loss_fwd_kernel(const float *ref, const float *pred, const float *G,
                                                                       const int *lens, double *acc, int *cnt, int N, int M,
                                                                       int kind, int vec4)
{
    __shared__ double s_acc[16];
    __shared__ int s_cnt[16];
    const int b = blockIdx.x;
    int n = N, m = M;
    if (lens) {
        n = min(max(lens[2 * b], 0), N);
        m = min(max(lens[2 * b + 1], 0), M);
    }
    const size_t base = (size_t)b * N * M;
    double a = 0.0;
    int c = 0;
    const int q4 = (m + 3) >> 2;            // groups of four columns per row
    const int total = n * q4;
    const bool vec = vec4 != 0;   // (the host checked M % 4 == 0 and the pointers' alignment)
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int i = idx / q4, j = (idx - i * q4) << 2;
        const size_t o = base + (size_t)i * M + j;
        float g[4], r[4], y[4];
        if (vec && j + 4 <= m) {
            const float4 g4 = *reinterpret_cast<const float4 *>(G + o), r4 = *reinterpret_cast<const float4 *>(ref + o),
                         y4 = *reinterpret_cast<const float4 *>(pred + o);
            g[0] = g4.x, g[1] = g4.y, g[2] = g4.z, g[3] = g4.w;
            r[0] = r4.x, r[1] = r4.y, r[2] = r4.z, r[3] = r4.w;
            y[0] = y4.x, y[1] = y4.y, y[2] = y4.z, y[3] = y4.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = j + e < m;
                g[e] = in ? G[o + e] : 0.f;
                r[e] = in ? ref[o + e] : 0.f;
                y[e] = in ? pred[o + e] : 0.5f;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (g[e] != 0.f) {
                a += sdp::loss_term(r[e], y[e], kind);
                ++c;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off);
        c += __shfl_down(c, off);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_acc[w] = a, s_cnt[w] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        double ta = 0.0;
        int tc = 0;
        for (int k = 0; k < (int)(blockDim.x >> 6); ++k) ta += s_acc[k], tc += s_cnt[k];
        acc[b] = ta;
        cnt[b] = tc;
    }
}

// grid (x, B): the workgroups of a pair stride over groups of four columns of the FULL padded matrix (grad is written
// in full: zero outside the pair's block and where G is 0); `vec4` as in the forward, with grad's alignment too
extern "C" __global__ void __launch_bounds__(256) sdp_loss_bwd_kernel(const float *ref, const float *pred, const float *G,
                                                                      const int *lens, const float *scale, float *grad, int N,
                                                                      int M, int kind, int vec4)
{
    const int b = blockIdx.y;
    int n = N, m = M;
    if (lens) {
        n = min(max(lens[2 * b], 0), N);
        m = min(max(lens[2 * b + 1], 0), M);
    }
    const float sc = scale[b];
    const size_t base = (size_t)b * N * M;
    const int q4 = (M + 3) >> 2;
    const int total = N * q4;
    const bool vec = vec4 != 0;   // (the host checked M % 4 == 0 and the pointers' alignment)
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int i = idx / q4, j = (idx - i * q4) << 2;
        const size_t o = base + (size_t)i * M + j;
        float out[4] = {0.f, 0.f, 0.f, 0.f};
        if (i < n && j < m) {
            float g[4], r[4], y[4];
            if (vec) {   // j + 4 <= M: the group lies inside the row (cells at or beyond m are masked below)
                const float4 g4 = *reinterpret_cast<const float4 *>(G + o), r4 = *reinterpret_cast<const float4 *>(ref + o),
                             y4 = *reinterpret_cast<const float4 *>(pred + o);
                g[0] = g4.x, g[1] = g4.y, g[2] = g4.z, g[3] = g4.w;
                r[0] = r4.x, r[1] = r4.y, r[2] = r4.z, r[3] = r4.w;
                y[0] = y4.x, y[1] = y4.y, y[2] = y4.z, y[3] = y4.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool in = j + e < m;
                    g[e] = in ? G[o + e] : 0.f;
                    r[e] = in ? ref[o + e] : 0.f;
                    y[e] = in ? pred[o + e] : 0.5f;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j + e < m && g[e] != 0.f) out[e] = sdp::loss_dterm(r[e], y[e], sc, kind);
        }
        if (vec) {
            *reinterpret_cast<float4 *>(grad + o) = make_float4(out[0], out[1], out[2], out[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j + e < M) grad[o + e] = out[e];
        }
    }
}

// ----------------------------------------------------------------------------------
// device self-test of the cross-lane semantics the sweep relies on
// ----------------------------------------------------------------------------------
extern "C" __global__ void sdp_selftest_kernel(int *out)
{
    const int lane = threadIdx.x;
    const double v = 100.0 + lane;
    const double shr = sdp::dpp_f64<sdp::DPP_WAVE_SHR1>(-1.0, v);
    const double shl = sdp::dpp_f64<sdp::DPP_WAVE_SHL1>(-2.0, v);
    const double rol = sdp::dpp_f64<sdp::DPP_WAVE_ROL1>(-3.0, v);
    const double ror = sdp::dpp_f64<sdp::DPP_WAVE_ROR1>(-4.0, v);
    int bad = 0;
    bad |= (shr != (lane == 0 ? -1.0 : 100.0 + lane - 1)) ? 1 : 0;
    bad |= (shl != (lane == 63 ? -2.0 : 100.0 + lane + 1)) ? 2 : 0;
    bad |= (rol != 100.0 + ((lane + 1) & 63)) ? 4 : 0;
    bad |= (ror != 100.0 + ((lane + 63) & 63)) ? 8 : 0;
    // buffer addressing: out-of-range load returns 0, out-of-range store is dropped
    __amdgpu_buffer_rsrc_t r = sdp::make_rsrc(out + 64, 64 * 4);
    const unsigned oob = __builtin_amdgcn_raw_buffer_load_b32(r, sdp::OOB, 0, 0);
    const unsigned neg = __builtin_amdgcn_raw_buffer_load_b32(r, (unsigned)(-4 * (lane + 1)), 0, 0);
    const unsigned past = __builtin_amdgcn_raw_buffer_load_b32(r, 64 * 4 + lane * 4, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b32(0xdeadu, r, sdp::OOB, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b32(0xdeadu, r, 64 * 4 + lane * 4, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b32(1000u + lane, r, lane * 4, 0, 0);
    bad |= (oob != 0u) ? 16 : 0;
    bad |= (neg != 0u) ? 32 : 0;
    bad |= (past != 0u) ? 64 : 0;
    out[lane] = bad;
    // informational (sdp_probe): is the scalar offset part of the range check?  Read the word right
    // after the buffer through soffset; 0 = checked (out of range), 7777 = not checked.
    const unsigned via_s = __builtin_amdgcn_raw_buffer_load_b32(r, lane * 4, 64 * 4, 0);
    out[192 + lane] = (int)via_s;
}
