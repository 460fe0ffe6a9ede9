// sdp_hard.h -- the hard-max (max-plus) kernel family (csrc/sdp_hard.hip): launch geometry shared with the host side.
#ifndef SDP_HARD_H_
#define SDP_HARD_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdp_hard {

constexpr int STRIP = 64;        // rows of a strip: one per lane of the wave that sweeps it
constexpr int CHUNK = 32;        // anti-diagonal steps between two barriers; a lane's scores of a chunk are 32 consecutive floats
constexpr int PTR_STEPS = 16;    // steps whose 2-bit pointers fill one 32-bit word of a lane
constexpr int MAX_WAVES = 8;     // waves (strips in flight) of a workgroup
constexpr int KEY = 256;         // progress word of a wave: strip * KEY + chunks done (chunks of a strip <= 66 < KEY)
constexpr int LDS_BUDGET = 64 * 1024;

__host__ __device__ inline int strips(int N) { return (N + STRIP - 1) / STRIP; }
// chunks of a strip of m columns: the last lane starts 63 steps after the first
__host__ __device__ inline int chunks(int m) { return (m + STRIP - 1 + CHUNK - 1) / CHUNK; }
// pointer words per lane and strip (two per chunk); a word of all 64 lanes is one 256-byte line
__host__ __device__ inline int words(int M) { return (CHUNK / PTR_STEPS) * chunks(M); }
__host__ __device__ inline int row_pitch(int M) { return M + STRIP; }   // floats of one boundary row in LDS
__host__ __device__ inline size_t forward_lds_bytes(int waves, int M) { return (size_t)waves * row_pitch(M) * 4 + 2 * MAX_WAVES * 4; }
__host__ __device__ inline size_t walk_lds_bytes(int M) { return (size_t)words(M) * STRIP * 4; }

// kernel ids sdp_kernel_name answers for the local-alignment kernels (the sweeps' builds keep the numbers below 80, the
// gap-gradient kernels 100-105)
enum { ID_LOCAL_FWD = 110, ID_LOCAL_FWD_T = 111, ID_LOCAL_VAL = 112, ID_LOCAL_VAL_T = 113, ID_LOCAL_WALK = 114 };

}  // namespace sdp_hard

extern "C" {
__global__ void sdp_hard_fwd_kernel(const float *theta, const float *A, uint32_t *state, float *Vt, const int *lens, int N, int M,
                                    int lo, int waves);
__global__ void sdp_hard_fwd_t_kernel(const float *theta, const float *A, uint32_t *state, float *Vt, const int *lens, int N, int M,
                                      int lo, int waves);
__global__ void sdp_hard_val_kernel(const float *theta, const float *A, uint32_t *state, float *Vt, const int *lens, int N, int M,
                                    int lo, int waves);
__global__ void sdp_hard_val_t_kernel(const float *theta, const float *A, uint32_t *state, float *Vt, const int *lens, int N, int M,
                                      int lo, int waves);
__global__ void sdp_hard_walk_kernel(const uint32_t *state, const float *Et, float *E, int *states, int *counts, const int *lens,
                                     int N, int M, int lo, int cap, int ymx);
// local alignment: the zero floor, pointer code 3, Vt = the best cell, ends = the first cell that holds it
__global__ void sdp_hard_local_fwd_kernel(const float *theta, const float *A, uint32_t *state, float *Vt, int *ends, const int *lens,
                                          int N, int M, int lo, int waves);
__global__ void sdp_hard_local_fwd_t_kernel(const float *theta, const float *A, uint32_t *state, float *Vt, int *ends, const int *lens,
                                            int N, int M, int lo, int waves);
__global__ void sdp_hard_local_val_kernel(const float *theta, const float *A, uint32_t *state, float *Vt, int *ends, const int *lens,
                                          int N, int M, int lo, int waves);
__global__ void sdp_hard_local_val_t_kernel(const float *theta, const float *A, uint32_t *state, float *Vt, int *ends, const int *lens,
                                            int N, int M, int lo, int waves);
__global__ void sdp_hard_local_walk_kernel(const uint32_t *state, const int *ends, const float *Et, float *E, int *states, int *counts,
                                           const int *lens, int N, int M, int lo, int cap, int ymx);
}

#endif  // SDP_HARD_H_
