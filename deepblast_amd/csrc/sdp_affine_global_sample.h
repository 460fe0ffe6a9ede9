// sdp_affine_global_sample.h -- alignments sampled from the affine-gap soft global operator's posterior
// (csrc/sdp_affine_global_sample.hip): the kernel id and the launch parameters shared with the host side.  The geometry of the
// records is that of sdp_affine_global.h, the generator that of sdp_sample.h.
#ifndef SDP_AFFINE_GLOBAL_SAMPLE_H_
#define SDP_AFFINE_GLOBAL_SAMPLE_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdp_affine_global_sample {

// the kernel id sdp_kernel_name answers for (189 and 191 answer NULL: the hard global sweeps end at 188, and callers probe the ids
// on either side)
enum { ID_SAMPLE = 190 };

constexpr int LANES = 64;   // one wave per workgroup: 64 samples of a pair

struct Params {
    const float4 *state;          // the records of sdp_affine_global_forward_f32 (the end weights travel in them)
    int32_t *states;              // (B, K, cap, 3) or null
    int32_t *counts;              // (B, K) or null; required with states
    int32_t *visits;              // (B, N, M) or null: + 1 per path cell
    int32_t *opens;               // (B, N, M) or null: + 1 per gap cell of a path whose predecessor is in another plane
    int32_t *extends;             // (B, N, M) or null: + 1 per gap cell of a path whose predecessor is in the same plane
    int32_t *ends;                // (B, K, 3) or null
    const int32_t *lens;          // (B, 2) or null
    uint64_t seed;
    int B, N, M, K, sample0;
    int cap;                      // sdp_traceback_capacity(N, M)
};

}  // namespace sdp_affine_global_sample

extern "C" {
__global__ void sdp_affine_global_sample_kernel(const sdp_affine_global_sample::Params p);
}

#endif  // SDP_AFFINE_GLOBAL_SAMPLE_H_
