// sdp_sample.hip -- alignments drawn from the posterior by a stochastic traceback on the forward sweep's state, for gfx950.
//
// The soft-max weights Q[i,j,(x,m,y)] the forward sweep leaves are the transition probabilities of the Gibbs distribution over
// alignments, read backwards: from cell (i, j) the path came from (i-1, j) with probability Qx, from (i, j-1) with Qy and from
// (i-1, j-1) with the rest.  A sample is one walk from (n, m) that picks its predecessor by one uniform per step (include/sdp.h:
// sdp_sample_paths_f32 states the draw bit for bit); the marginals of the walks are E.
//   * lane = sample: a wave is 64 samples of one pair, the grid B x ceil(K / 64) waves.  The lanes walk on their own -- no
//     hand-off, no polling, no LDS; every step decrements i or j, so a lane is done after at most n + m - 1 steps.
//   * per step one gather of the cell's two weights from the state AS THE SWEEPS ADDRESS IT (sdp_kernels.h, "State layout";
//     csrc/sdp_gap.hip reads the same records a tile at a time): cell (r, c), 0-based, is lane r & 63 of strip r >> 6 at step
//     c + (r & 63).  float2 state: one 8-byte load.  Packed state: the cell's two 20-bit fields lie inside two consecutive dwords
//     of its five-dword record (bit 8 sub of dword sub, sub = step & 3), so two dword loads, decoded by sdp::q20_field and scaled
//     by QF_UNSCALE -- the bits the backward sweep works with.  Thin long pairs of a routed launch keep float2 records inside
//     their packed slot (sdp::thin_pair), a state written in parts holds the same records.
//   * the generator is counter based (csrc/sdp_sample.h: Philox4x32-10): four steps per call, nothing kept between launches, so
//     sample k of a launch at sample0 is sample k + sample0 of any other.
//   * the list leaves right-aligned -- record c goes to row cap - 2 - c -- so a lane never moves what it wrote; visits are
//     no-return integer adds, which commute: the counts do not depend on the order the lanes arrive in.
// The chain is one dependent load per step, and that is what ships: requesting the three possible successors as soon as a cell
// is known was not built (DESIGN.md 3.15 has the measured step latency it would have to beat, and why it needs the loop unrolled).
#include "sdp_device.h"

#include "sdp_sample.h"

namespace sdp_sample {

// the walk of one lane; `weights(b, n, m, r, c, qx, qy)` reads the x and y weights of cell (r, c), 0-based, of pair b (n x m) in T
template <typename T, typename W>
__device__ __forceinline__ void walk(const Params &p, W weights)
{
    const int kblocks = (p.K + LANES - 1) / LANES;
    const int b = blockIdx.x / (unsigned)kblocks, k = (blockIdx.x % (unsigned)kblocks) * LANES + threadIdx.x;
    if (k >= p.K) return;
    int n = p.N, m = p.M;
    if (p.lens) {   // clamped as the sweeps clamp them
        n = p.lens[2 * b], m = p.lens[2 * b + 1];
        n = n < 1 ? 1 : (n > p.N ? p.N : n);
        m = m < 1 ? 1 : (m > p.M ? p.M : m);
    }
    const int sample = p.sample0 + k;
    int32_t *out = p.states ? p.states + ((size_t)b * p.K + k) * p.cap * 3 : nullptr;
    int32_t *vis = p.visits ? p.visits + (size_t)b * p.N * p.M : nullptr;
    // a transposed problem: the column step is the original's x (named 0) and takes the first interval
    const int code_row = p.transposed ? 2 : 0, code_col = p.transposed ? 0 : 2;
    int cnt = 0;
    auto record = [&](int ri, int rj, int st) {
        if (out) {
            int32_t *dst = out + 3 * (size_t)(p.cap - 2 - cnt);
            dst[0] = ri, dst[1] = rj, dst[2] = st;
        }
        ++cnt;
    };

    int i = n, j = m, t = 0;        // 1-based cell of the walk, step number
    int li = n - 1, lj = m - 1;     // 0-based: the last cell recorded (the padding starts there)
    Words rnd = {};
    while (i >= p.lo && j >= p.lo) {
        T qx, qy;
        weights(b, n, m, i - 1, j - 1, qx, qy);
        if ((t & 3) == 0) rnd = step_words(p.seed, b, sample, t >> 2);
        const int sel = t & 3;
        const T u = (T)unit(sel == 0 ? rnd.w[0] : (sel == 1 ? rnd.w[1] : (sel == 2 ? rnd.w[2] : rnd.w[3])));
        const T first = p.transposed ? qy : qx;
        const T both = qx + qy;
        const bool row = p.transposed ? (!(u < first) && u < both) : u < first;
        const bool col = p.transposed ? u < first : (!(u < first) && u < both);
        li = i - 1, lj = j - 1;
        record(li, lj, row ? code_row : (col ? code_col : 1));
        if (vis) __hip_atomic_fetch_add(vis + (size_t)li * p.M + lj, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        i -= col ? 0 : 1;
        j -= row ? 0 : 1;
        ++t;
    }
    const int npath = cnt, fi = li, fj = lj;   // the path's cells and the first of them (the padding's start when there is none)
    if (p.transposed) {
        while (lj > 0) record(li, --lj, 0);
        while (li > 0) record(--li, lj, 2);
    } else {
        while (li > 0) record(--li, lj, 0);
        while (lj > 0) record(li, --lj, 2);
    }
    if (out) {
        // the last row is never part of a list (cnt <= n + m - 1 < cap - 1)
        int32_t *last = out + 3 * (size_t)(p.cap - 1);
        last[0] = npath, last[1] = fi, last[2] = fj;
    }
    if (p.counts) p.counts[(size_t)b * p.K + k] = cnt;
}

// the skewed states: packed (two 20-bit fields per cell) or float2, per pair
struct Skewed {
    const Params &p;
    __device__ __forceinline__ void operator()(int b, int n, int m, int r, int c, float &qx, float &qy) const
    {
        const int l = r & 63, st = c + l;
        const char *stream = static_cast<const char *>(p.state) + ((size_t)b * p.nstrips_max + (r >> 6)) * p.ps;
        if (p.whole_exact || (p.route && sdp::thin_pair(n, m))) {
            const sdp::f32x2 q = *reinterpret_cast<const sdp::f32x2 *>(stream + (size_t)(st >> 5) * p.us_x + (st & 31) * 512 + l * 8);
            qx = q[0], qy = q[1];
        } else {
            // dword d of the lane's 16-step block lies in row d >> 2 (1 KB each), column d & 3 of the lane's dwordx4
            const char *blk = stream + (size_t)(st >> 5) * p.us_q + ((st >> 4) & 1) * 5120 + l * 16;
            const int sub = st & 3, d = 5 * ((st & 15) >> 2) + sub;
            const unsigned w0 = *reinterpret_cast<const unsigned *>(blk + (d >> 2) * 1024 + (d & 3) * 4);
            const unsigned w1 = *reinterpret_cast<const unsigned *>(blk + ((d + 1) >> 2) * 1024 + ((d + 1) & 3) * 4);
            const unsigned long long v = (((unsigned long long)w1 << 32) | w0) >> (8 * sub);   // fields x, y from bit 0 up
            qx = sdp::q20_field((unsigned)v) * sdp::QF_UNSCALE;
            qy = sdp::q20_field((unsigned)(v >> 20)) * sdp::QF_UNSCALE;
        }
    }
};

// the row-major states (B, N, M, 3): weights x, m, y of cell (r, c)
template <typename T>
struct Rows {
    const Params &p;
    __device__ __forceinline__ void operator()(int b, int, int, int r, int c, T &qx, T &qy) const
    {
        const T *q = static_cast<const T *>(p.state) + (((size_t)b * p.N + r) * p.M + c) * 3;
        qx = q[0], qy = q[2];
    }
};

}  // namespace sdp_sample

extern "C" __global__ void __launch_bounds__(sdp_sample::LANES) sdp_sample_kernel(const sdp_sample::Params p)
{
    sdp_sample::walk<float>(p, sdp_sample::Skewed{p});
}
extern "C" __global__ void __launch_bounds__(sdp_sample::LANES) sdp_sample_rows_kernel(const sdp_sample::Params p)
{
    sdp_sample::walk<float>(p, sdp_sample::Rows<float>{p});
}
extern "C" __global__ void __launch_bounds__(sdp_sample::LANES) sdp_sample_rows_f64_kernel(const sdp_sample::Params p)
{
    sdp_sample::walk<double>(p, sdp_sample::Rows<double>{p});
}
