// sdp_sample.h -- sampling alignments from the posterior (csrc/sdp_sample.hip): the counter-based generator, shared by the kernels
// and the host (sdp_sample_uniform), and the launch parameters shared with the host side.
#ifndef SDP_SAMPLE_H_
#define SDP_SAMPLE_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdp_sample {

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of two 32 x 32 -> 64 bit
// products on a 128-bit counter under a 64-bit key that is bumped by the Weyl constants between rounds.  No state: the four
// output words are a pure function of (counter, key), so a sample's uniforms depend on nothing but (seed, pair, sample, step).
struct Words {
    uint32_t w[4];
};

__host__ __device__ inline Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return Words{{c0, c1, c2, c3}};
}

// the four words that serve steps 4 g .. 4 g + 3 of sample `sample` of pair `pair`
__host__ __device__ inline Words step_words(uint64_t seed, int pair, int sample, int g)
{
    return philox4x32_10((uint32_t)g, (uint32_t)sample, (uint32_t)pair, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// a word's top 24 bits as a float in [0, 1): exactly representable, so the compare against a weight is the only rounding-free step
__host__ __device__ inline float unit(uint32_t word) { return (float)(word >> 8) * 5.9604644775390625e-8f; }

// U(seed, pair, sample, t) of include/sdp.h
__host__ __device__ inline float uniform(uint64_t seed, int pair, int sample, int t)
{
    return unit(step_words(seed, pair, sample, t >> 2).w[t & 3]);
}

// kernel ids sdp_kernel_name answers for
enum { ID_SAMPLE = 120, ID_SAMPLE_ROWS = 121, ID_SAMPLE_ROWS_F64 = 122 };

constexpr int LANES = 64;   // one wave per workgroup: 64 samples of one pair

struct Params {
    const void *state;            // the forward sweep's state: skewed (packed or float2), or row-major (B, N, M, 3)
    int32_t *states;              // (B, K, cap, 3) or null
    int32_t *counts;              // (B, K); required with states
    int32_t *visits;              // (B, N, M) or null: + 1 per path cell
    const int32_t *lens;          // (B, 2) or null
    uint64_t seed;
    int B, N, M, K, sample0;
    int lo;                       // first row / column that holds cells: 1 (NW), 2 (SW), 1-based
    int cap;                      // sdp_traceback_capacity(N, M)
    int transposed;               // SDP_SAMPLE_TRANSPOSED
    int nstrips_max;              // skewed states: geometry as in sdp_gap::Params
    size_t ps;
    unsigned us_q, us_x;
    int whole_exact, route;
};

}  // namespace sdp_sample

extern "C" {
__global__ void sdp_sample_kernel(const sdp_sample::Params p);
__global__ void sdp_sample_rows_kernel(const sdp_sample::Params p);
__global__ void sdp_sample_rows_f64_kernel(const sdp_sample::Params p);
}

#endif  // SDP_SAMPLE_H_
