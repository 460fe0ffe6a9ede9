// sdp_gap.hip -- the true gradient of the alignment score with respect to the gap scores A, first and second order, for gfx950.
//
// In the reference's notation Q[i,j,(x,m,y)] are the soft-max weights of cell (i,j) and E = Et . dVt/dtheta; Qd, Ed are what the
// adjoint pair returns for a tangent (Ztheta, ZA).  A enters cell (i,j) through its x and y candidates only, so
//
//     G  = Et . dVt/dA             = E  (Qx + Qy)
//     Gd = d/deps G(theta + eps Ztheta, A + eps ZA) = Ed (Qx + Qy) + E (Qdx + Qdy)
//
// and the gradient of <Ztheta, E> + <ZG, G> with respect to (theta, A, Et) is (Ed, Gd, Vtd) of the adjoint pair run with ZA = ZG.
// No recurrence: one elementwise pass over buffers the sweeps already left behind.  The work is in reading the library-private
// state -- stored skewed, [pair][strip][step t][lane], cell (i0 + lane, t - lane) (sdp_kernels.hip, "Skewed state addressing") --
// at memory speed while E and G are row-major:
//   * a workgroup of four waves owns one TILE: TS steps of one (pair, strip).  Wave w takes the 16-step blocks w, w + 4, ... of the
//     tile; a lane reads its own records exactly as the sweeps do -- packed: five dwordx4 per block, each 1 KB contiguous per wave;
//     float2: one 512-byte row per step -- so every state access is whole lines in the order they lie in memory;
//   * the lane forms Qx + Qy of its 16 cells and writes them to LDS UNSKEWED: row r of the tile holds columns
//     t0 - (r & ~3) .. + TS - 1, a parallelogram whose rows all start on a 16-byte boundary of the row-major planes.  The tile
//     therefore needs steps t0 .. t0 + TS + 2: one block (packed) or three rows (float2) more than it owns;
//   * after one barrier the 256 threads walk the parallelogram four columns at a time: aligned 16-byte LDS reads, E loads (issued
//     before the state is decoded) and G stores, 32 consecutive threads on one 512-byte row segment.
// Both stored weights are the x and the y weight, so Qx + Qy is their plain sum: no cancellation, and exact when a packed weight
// decodes to exactly 0 or 1 (a saturated gap cell gives G = E, a forbidden one, A = -inf, G = +0).  Where E is exactly zero G is
// +0 whatever the stored weights are.  Cells outside a pair's n x m block (per-pair lengths) are written +0 by the tile that
// covers them, or left alone (SDP_NO_FILL, first order only); row 0 and column 0 of a Smith-Waterman block give +0.
//
// The packed-state decoder, the cache policies and the geometry are the sweeps' own: this file is the device helpers the sweep
// shares (sdp_device.h) plus the kernels below.
#include "sdp_device.h"

#include "sdp_gap.h"

namespace sdp_gap {

using sdp::q20_unpack;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float guarded(float e, float w) { return e == 0.f ? 0.f : e * w; }

// the 16 sums (x + y) of this lane's cells of the 16-step block that starts at step tb of a packed stream
__device__ __forceinline__ void block_packed(const char *stream, unsigned us, int tb, int lane, float *v)
{
    const char *blk = stream + (size_t)(tb >> 5) * us + ((tb >> 4) & 1) * 5120 + lane * 16;
    unsigned w[20];
#pragma unroll
    for (int jr = 0; jr < 5; ++jr) {
        const u32x4 row = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(blk + jr * 1024));
        w[4 * jr] = row[0], w[4 * jr + 1] = row[1], w[4 * jr + 2] = row[2], w[4 * jr + 3] = row[3];
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const float2 q = q20_unpack(w + 5 * (k >> 2), k & 3);
        v[k] = q.x * sdp::QF_UNSCALE + q.y * sdp::QF_UNSCALE;   // the weights as the backward sweep decodes them
    }
}

// ... of a float2 stream (Q in its exact form, or Qd); only the first `need` steps of the block are wanted
__device__ __forceinline__ void block_float2(const char *stream, unsigned us, int tb, int lane, int need, float *v)
{
    const char *blk = stream + (size_t)(tb >> 5) * us + (tb & 31) * 512 + lane * 8;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        v[k] = 0.f;
        if (k < need) {
            const sdp::f32x2 q = __builtin_nontemporal_load(reinterpret_cast<const sdp::f32x2 *>(blk + k * 512));
            v[k] = q[0] + q[1];
        }
    }
}

template <int TS, bool SECOND>
__device__ __forceinline__ void tile(const Params &p)
{
    constexpr int NBLK = TS / 16 + 1;          // 16-step blocks a tile reads: steps t0 .. t0 + TS + 2
    constexpr int PITCH = TS + 4;              // floats per row in LDS (a multiple of 4: aligned 16-byte reads)
    constexpr int GROUPS = 64 * (TS / 4) / THREADS;   // four-column groups per thread
    __shared__ float sq[64 * PITCH];
    __shared__ float sd[SECOND ? 64 * PITCH : 4];

    // grid: one workgroup per (pair, strip, tile), tiles fastest -- neighbours in the grid are neighbours in the state
    const int ntiles = tiles(p.M, TS);
    const int b = blockIdx.x / (unsigned)(p.nstrips_max * ntiles), s = blockIdx.x / (unsigned)ntiles % (unsigned)p.nstrips_max;
    const int t0 = blockIdx.x % (unsigned)ntiles * TS, i0 = s * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int n = p.N, m = p.M;
    if (p.lens) {   // clamped as the sweeps clamp them
        n = p.lens[2 * b], m = p.lens[2 * b + 1];
        n = n < 1 ? 1 : (n > p.N ? p.N : n);
        m = m < 1 ? 1 : (m > p.M ? p.M : m);
    }
    const bool live = i0 < n && t0 < m + 63;   // the tile holds cells of the pair's block
    if (!live && !p.fill) return;
    const size_t plane = (size_t)p.N * p.M, pb = (size_t)b * plane;

    // E (and Ed) of this thread's groups: requested before the state is touched
    int gi[GROUPS], gc[GROUPS], gx[GROUPS];
    f32x4 e4[GROUPS], ed4[SECOND ? GROUPS : 1];
#pragma unroll
    for (int q = 0; q < GROUPS; ++q) {
        const int g = threadIdx.x + THREADS * q, r = g / (TS / 4);
        gx[q] = (g % (TS / 4)) * 4;
        gi[q] = i0 + r;
        gc[q] = t0 - (r & ~3) + gx[q];
        gx[q] += r * PITCH;
        e4[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if constexpr (SECOND) ed4[q] = e4[q];
        if (!live || gi[q] >= n || gc[q] >= m || gc[q] + 3 < 0) continue;
        const size_t at = pb + (size_t)gi[q] * p.M + gc[q];
        if (p.vec4) {
            e4[q] = *reinterpret_cast<const f32x4 *>(p.E + at);
            if constexpr (SECOND) ed4[q] = *reinterpret_cast<const f32x4 *>(p.Ed + at);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (gc[q] + e >= 0 && gc[q] + e < m) {
                    e4[q][e] = p.E[at + e];
                    if constexpr (SECOND) ed4[q][e] = p.Ed[at + e];
                }
        }
    }

    if (live) {
        const size_t stream = (size_t)b * p.nstrips_max + s;
        const bool exact = SECOND || p.whole_exact || (p.route && sdp::thin_pair(n, m));
        const char *qs = static_cast<const char *>(p.state) + stream * p.ps;
        const char *ds = SECOND ? static_cast<const char *>(p.state_d) + stream * p.ps_d : nullptr;
#pragma unroll
        for (int blk0 = 0; blk0 < NBLK; blk0 += THREADS / 64) {
            const int blk = blk0 + wave, tb = t0 + 16 * blk;
            if (blk >= NBLK || tb >= m + 63) continue;   // (the block's cells live at steps 0 .. m + 62 <= tpad - 1)
            const int need = min(TS + 3 - 16 * blk, m + 63 - tb);   // steps of this block that hold cells of the tile
            float v[16], vd[16];
            if (exact) block_float2(qs, p.us_x, tb, lane, need, v);
            else block_packed(qs, p.us_q, tb, lane, v);
            if constexpr (SECOND) block_float2(ds, p.us_x, tb, lane, need, vd);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int x = 16 * blk + k - (lane & 3);   // column of cell (lane, tb + k) inside row `lane` of the tile
                if (x >= 0 && x < TS) {
                    sq[lane * PITCH + x] = v[k];
                    if constexpr (SECOND) sd[lane * PITCH + x] = vd[k];
                }
            }
        }
    }
    __syncthreads();

#pragma unroll
    for (int q = 0; q < GROUPS; ++q) {
        const int i = gi[q], c = gc[q];
        if (i >= p.N || c >= p.M || c + 3 < 0) continue;
        const bool row_in = live && i < n;
        f32x4 w4 = {0.f, 0.f, 0.f, 0.f}, wd4 = {0.f, 0.f, 0.f, 0.f}, out;
        if (row_in && c < m) {
            w4 = *reinterpret_cast<const f32x4 *>(sq + gx[q]);
            if constexpr (SECOND) wd4 = *reinterpret_cast<const f32x4 *>(sd + gx[q]);
        }
        bool in[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int col = c + e;
            in[e] = row_in && col >= 0 && col < m;
            const bool border = p.sw && (i == 0 || col == 0);
            float val = 0.f;
            if (in[e] && !border) {
                val = guarded(e4[q][e], w4[e]);
                if constexpr (SECOND) val = guarded(ed4[q][e], w4[e]) + guarded(e4[q][e], wd4[e]);
            }
            out[e] = val;
        }
        float *dst = p.G + pb + (size_t)i * p.M + c;
        if (p.vec4 && (p.fill || (in[0] && in[3]))) {
            __builtin_nontemporal_store(out, reinterpret_cast<f32x4 *>(dst));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e >= 0 && c + e < p.M && (p.fill || in[e])) dst[e] = out[e];
        }
    }
}

template <typename T>
__device__ __forceinline__ T guarded_t(T e, T w) { return e == (T)0 ? (T)0 : e * w; }

// the row-major states (B, N, M, 3): one thread per cell of the padded batch
template <typename T, bool SECOND>
__device__ __forceinline__ void rows(const T *E, const T *Ed, const T *Q, const T *Qd, T *G, const int *lens, int B, int N, int M, int sw, int fill)
{
    const size_t plane = (size_t)N * M, at = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (at >= plane * B) return;
    const int b = (int)(at / plane), i = (int)(at % plane / M), j = (int)(at % M);
    int n = N, m = M;
    if (lens) {
        n = lens[2 * b], m = lens[2 * b + 1];
        n = n < 1 ? 1 : (n > N ? N : n);
        m = m < 1 ? 1 : (m > M ? M : m);
    }
    T out = (T)0;
    if (i < n && j < m) {
        if (!(sw && (i == 0 || j == 0))) {
            const T w = Q[at * 3] + Q[at * 3 + 2];
            out = guarded_t(E[at], w);
            if constexpr (SECOND) out = guarded_t(Ed[at], w) + guarded_t(E[at], Qd[at * 3] + Qd[at * 3 + 2]);
        }
    } else if (!fill) {
        return;
    }
    G[at] = out;
}

}  // namespace sdp_gap

extern "C" __global__ void __launch_bounds__(sdp_gap::THREADS) sdp_gap_kernel(const sdp_gap::Params p)
{
    sdp_gap::tile<sdp_gap::TS1, false>(p);
}
extern "C" __global__ void __launch_bounds__(sdp_gap::THREADS) sdp_gap2_kernel(const sdp_gap::Params p)
{
    sdp_gap::tile<sdp_gap::TS2, true>(p);
}
extern "C" __global__ void __launch_bounds__(sdp_gap::THREADS) sdp_gap_rows_kernel(const float *E, const float *Q, float *G, const int *lens, int B,
                                                                                   int N, int M, int sw, int fill)
{
    sdp_gap::rows<float, false>(E, nullptr, Q, nullptr, G, lens, B, N, M, sw, fill);
}
extern "C" __global__ void __launch_bounds__(sdp_gap::THREADS) sdp_gap2_rows_kernel(const float *E, const float *Ed, const float *Q, const float *Qd,
                                                                                    float *Gd, const int *lens, int B, int N, int M, int sw)
{
    sdp_gap::rows<float, true>(E, Ed, Q, Qd, Gd, lens, B, N, M, sw, 1);
}
extern "C" __global__ void __launch_bounds__(sdp_gap::THREADS) sdp_gap_rows_f64_kernel(const double *E, const double *Q, double *G, const int *lens,
                                                                                       int B, int N, int M, int sw, int fill)
{
    sdp_gap::rows<double, false>(E, nullptr, Q, nullptr, G, lens, B, N, M, sw, fill);
}
extern "C" __global__ void __launch_bounds__(sdp_gap::THREADS) sdp_gap2_rows_f64_kernel(const double *E, const double *Ed, const double *Q,
                                                                                        const double *Qd, double *Gd, const int *lens, int B, int N,
                                                                                        int M, int sw)
{
    sdp_gap::rows<double, true>(E, Ed, Q, Qd, Gd, lens, B, N, M, sw, 1);
}
