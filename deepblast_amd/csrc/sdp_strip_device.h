// sdp_strip_device.h -- device helpers of the strip schedule, one copy for every kernel file
// that sweeps on it: the lane moves, the unaligned four-float access, and the loads and stores that move a lane's run of
// consecutive steps, and what the two samplers' end-cell tables share.  For .hip files only (internal linkage: every including file has its own copy).
#ifndef SDP_STRIP_DEVICE_H_
#define SDP_STRIP_DEVICE_H_

#include <hip/hip_runtime.h>

// the widths the helpers below are written for; every family header states them too (its tests read them there), and every
// including file asserts that the two agree
namespace sdp_strip {
constexpr int STRIP = 64;   // rows of a strip: one per lane of the wave that sweeps it
constexpr int CHUNK = 32;   // anti-diagonal steps between two barriers
}  // namespace sdp_strip

namespace {

constexpr int DPP_WAVE_SHL1 = 0x130;   // lane i <- lane i + 1; lane 63 keeps `old`
constexpr int DPP_WAVE_SHR1 = 0x138;   // lane i <- lane i - 1; lane 0 keeps `old`

__device__ __forceinline__ float from_upper_lane(float lane0, float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(lane0), __float_as_int(v), DPP_WAVE_SHR1, 0xf, 0xf, false));
}

__device__ __forceinline__ float from_lower_lane(float lane63, float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(lane63), __float_as_int(v), DPP_WAVE_SHL1, 0xf, 0xf, false));
}

__device__ __forceinline__ float of_lane(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

struct __attribute__((packed, aligned(4))) F4 {   // four floats at any 4-byte boundary
    float v[4];
};

// the scores lane `lane` of strip `s` needs in chunk `c`: columns 32 c - lane .. 32 c - lane + 31 of row 64 s + lane; 0 where
// the cell does not exist (the value is then never used)
__device__ __forceinline__ void load_chunk(const float *theta, const float *A, size_t plane, int M, int n, int m, int s, int c,
                                           int lane, float (&th)[sdp_strip::CHUNK], float (&a)[sdp_strip::CHUNK])
{
    using namespace sdp_strip;
    const int row = s * STRIP + lane, col0 = c * CHUNK - lane;
    const bool rowok = row < n;
    const size_t at = plane + (size_t)(rowok ? row : 0) * M;
    if (rowok && col0 >= 0 && col0 + CHUNK <= m) {
        const F4 *pt = reinterpret_cast<const F4 *>(theta + at + col0), *pa = reinterpret_cast<const F4 *>(A + at + col0);
#pragma unroll
        for (int g = 0; g < CHUNK / 4; ++g) {
            const F4 t4 = pt[g], a4 = pa[g];
#pragma unroll
            for (int e = 0; e < 4; ++e) th[4 * g + e] = t4.v[e], a[4 * g + e] = a4.v[e];
        }
    } else {
#pragma unroll
        for (int t = 0; t < CHUNK; ++t) {
            const int col = col0 + t;
            const bool ok = rowok && col >= 0 && col < m;
            th[t] = ok ? theta[at + col] : 0.f;
            a[t] = ok ? A[at + col] : 0.f;
        }
    }
}

// one plane of cotangents: what lane `lane` of strip `s` needs in half `h` of chunk `c`, columns 32 c + 16 h - lane .. + 15 of
// row 64 s + lane, into v[16 h ..]; 0 where the cell does not exist, and everywhere when z is NULL (uniform over the grid)
__device__ __forceinline__ void load_half(const float *z, size_t plane, int M, int n, int m, int s, int c, int h, int lane,
                                          float (&v)[sdp_strip::CHUNK])
{
    using namespace sdp_strip;
    constexpr int HALF = CHUNK / 2;
    const int row = s * STRIP + lane, col0 = c * CHUNK + h * HALF - lane;
    const bool rowok = z != nullptr && row < n;
    const size_t at = plane + (size_t)(rowok ? row : 0) * M;
    if (rowok && col0 >= 0 && col0 + HALF <= m) {
        const F4 *p = reinterpret_cast<const F4 *>(z + at + col0);
#pragma unroll
        for (int g = 0; g < HALF / 4; ++g) {
            const F4 z4 = p[g];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[h * HALF + 4 * g + e] = z4.v[e];
        }
    } else {
#pragma unroll
        for (int t = 0; t < HALF; ++t) {
            const int col = col0 + t;
            v[h * HALF + t] = (rowok && col >= 0 && col < m) ? z[at + col] : 0.f;
        }
    }
}

// the records lane `lane` of strip `s` reads in group `g` of chunk `c`: steps K g .. K g + K - 1 (`pair`: the pair's first strip)
template <int K>
__device__ __forceinline__ void load_records(const float4 *state, size_t pair, int CH, int s, int c, int g, int lane, float4 (&q)[K])
{
    using namespace sdp_strip;
    const float4 *src = state + (((pair + s) * CH + c) * CHUNK + g * K) * STRIP + lane;
#pragma unroll
    for (int t = 0; t < K; ++t) q[t] = src[(size_t)t * STRIP];
}

// K consecutive cells of row `row` from column col0 on; only cells of the pair's block are written
template <int K>
__device__ __forceinline__ void store_run(float *out, size_t plane, int M, int n, int m, int row, int col0, const float (&e)[K])
{
    if (row >= n) return;
    const size_t at = plane + (size_t)row * M;
    if (col0 >= 0 && col0 + K <= m) {
        F4 *p = reinterpret_cast<F4 *>(out + at + col0);
#pragma unroll
        for (int g = 0; g < K / 4; ++g) {
            F4 x;
#pragma unroll
            for (int k = 0; k < 4; ++k) x.v[k] = e[4 * g + k];
            p[g] = x;
        }
    } else {
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const int col = col0 + t;
            if (col >= 0 && col < m) out[at + col] = e[t];
        }
    }
}

// (max, sum) of a log-sum-exp joined with another: sum exp = s exp(m); an empty one is (-inf, 0).  Symmetric in its arguments
// bit for bit, so a butterfly leaves every lane with the same pair.
__device__ __forceinline__ void lse_join(float &m0, float &s0, float m1, float s1)
{
    const float mx = fmaxf(m0, m1);
    const float e0 = m0 == mx ? 1.f : expf(m0 - mx), e1 = m1 == mx ? 1.f : expf(m1 - mx);
    s0 = s0 * e0 + s1 * e1;
    m0 = mx;
}

// ---- the end-cell tables of the samplers (csrc/sdp_soft_local_sample.hip, csrc/sdp_affine_local_sample.hip) ----

// the first index i in [0, count) with x < a[i], or count - 1 if there is none; a non-decreasing (count >= 1)
__device__ __forceinline__ int first_above(const float *a, int count, float x)
{
    int lo = 0, hi = count;   // every index below lo has a[i] <= x, every index from hi on (if any) has x < a[i]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x < a[mid])
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo < count ? lo : count - 1;
}

// one wave: out[0] = first, out[i + 1] = out[i] + cdf[i, m - 1] for the n rows of a pair's (.., M) plane `cdf` -- the totals are
// loaded 64 at a time, the adds are sequential in i (a readlane per row)
__device__ __forceinline__ void running_row_totals(const float *cdf, int M, int n, int m, float first, float *out, int lane)
{
    using namespace sdp_strip;
    float acc = first;
    if (lane == 0) out[0] = acc;
    for (int base = 0; base < n; base += STRIP) {
        const int r = base + lane;
        const float tot = r < n ? cdf[(size_t)r * M + (m - 1)] : 0.f;   // (+ 0 behind the last row: nothing reads it)
        float mine = 0.f;
#pragma unroll 4
        for (int l = 0; l < STRIP; ++l) {   // (a chain of adds: unrolled in full it only keeps 64 totals in scalar registers)
            acc = acc + of_lane(tot, l);
            mine = (lane == l) ? acc : mine;
        }
        if (r < n) out[r + 1] = mine;
    }
}

}  // namespace

#endif  // SDP_STRIP_DEVICE_H_
