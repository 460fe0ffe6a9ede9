// sdp_hard_affine.h -- the hard (max-plus) affine-gap kernel family, local, global and semi-global (csrc/sdp_hard_affine.hip): launch geometry shared with the host side.
#ifndef SDP_HARD_AFFINE_H_
#define SDP_HARD_AFFINE_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdp_hard_affine {

constexpr int STRIP = 64;        // rows of a strip: one per lane of the wave that sweeps it
constexpr int CHUNK = 32;        // anti-diagonal steps between two barriers
constexpr int HALF = 16;         // steps of the sweeps' input prefetch: three inputs, half a chunk ahead
constexpr int PTR_STEPS = 16;    // steps whose 2-bit pointers fill one 32-bit word of a lane
constexpr int PLANES = 3;        // x, m, y = 0, 1, 2: the step that entered the cell
constexpr int START = 3;         // pointer code of plane m alone: the alignment begins at this cell
constexpr int FREE_X = 1;        // `free_ends` of the semi-global member: rows may hang over (start in column 1, end in column m)
constexpr int FREE_Y = 2;        // columns may hang over (start in row 1, end in row n)
constexpr int FREE_ENDS_MASK = 3;
constexpr int MAX_WAVES = 8;     // waves (strips in flight) of a workgroup
constexpr int KEY = 256;         // progress word of a wave: strip * KEY + chunks done (chunks of a strip <= 66 < KEY)
constexpr int LDS_BUDGET = 160 * 1024;   // all of a CU's LDS: every kernel of the family has its dynamic-LDS attribute raised

__host__ __device__ inline int strips(int N) { return (N + STRIP - 1) / STRIP; }
// chunks of a strip of m columns: the last lane starts 63 steps after the first
__host__ __device__ inline int chunks(int m) { return (m + STRIP - 1 + CHUNK - 1) / CHUNK; }
// pointer words per lane, strip and plane (two per chunk); a word of all 64 lanes is one 256-byte line
__host__ __device__ inline int words(int M) { return (CHUNK / PTR_STEPS) * chunks(M); }
__host__ __device__ inline int row_pitch(int M) { return M + STRIP; }   // floats of one boundary row of one plane in LDS
// the ring of boundary rows: the sweeps hand H_x, H_m, H_y of a strip's bottom row down, three floats per column, plus the
// progress words
__host__ __device__ inline size_t sweep_lds_bytes(int waves, int M) { return (size_t)PLANES * waves * row_pitch(M) * 4 + 2 * MAX_WAVES * 4; }
// waves of a workgroup of the four sweeps: one per strip in flight, lowered to `forced` if 0 < forced, then until the ring fits
// LDS_BUDGET -- eight up to M = 1642, seven up to 1885, six up to the column limit 2048
__host__ __device__ inline int waves_for(int N, int M, int forced)
{
    int w = strips(N) < MAX_WAVES ? strips(N) : MAX_WAVES;
    if (forced > 0 && forced < w) w = forced;
    while (w > 1 && sweep_lds_bytes(w, M) > (size_t)LDS_BUDGET) --w;
    return w;
}
// the walk's copy of one strip's pointer lines, three planes: 101376 bytes at M = 2048
__host__ __device__ inline size_t walk_lds_bytes(int M) { return (size_t)words(M) * PLANES * STRIP * 4; }
// 32-bit words of one pair's pointers: state[((((pair * strips(N) + S) * words(M) + q) * 3 + s) * 64 + lane]
__host__ __device__ inline size_t pair_words(int N, int M) { return (size_t)strips(N) * words(M) * PLANES * STRIP; }

// kernel ids sdp_kernel_name answers for (169 and 175 answer NULL)
enum { ID_FWD = 170, ID_FWD_T = 171, ID_VAL = 172, ID_VAL_T = 173, ID_WALK = 174 };
// the global member's sweeps (184 and 189 answer NULL); its walk is ID_WALK
enum { ID_GLOBAL_FWD = 185, ID_GLOBAL_FWD_T = 186, ID_GLOBAL_VAL = 187, ID_GLOBAL_VAL_T = 188 };
// the semi-global member's sweeps (204 and 209 answer NULL); its walk is ID_WALK
enum { ID_SEMIGLOBAL_FWD = 205, ID_SEMIGLOBAL_FWD_T = 206, ID_SEMIGLOBAL_VAL = 207, ID_SEMIGLOBAL_VAL_T = 208 };

}  // namespace sdp_hard_affine

extern "C" {
__global__ void sdp_hard_affine_local_fwd_kernel(const float *theta, const float *O, const float *X, uint32_t *state, float *Vt, int *ends,
                                                 const int *lens, int N, int M, int waves);
__global__ void sdp_hard_affine_local_fwd_t_kernel(const float *theta, const float *O, const float *X, uint32_t *state, float *Vt, int *ends,
                                                   const int *lens, int N, int M, int waves);
__global__ void sdp_hard_affine_local_val_kernel(const float *theta, const float *O, const float *X, uint32_t *state, float *Vt, int *ends,
                                                 const int *lens, int N, int M, int waves);
__global__ void sdp_hard_affine_local_val_t_kernel(const float *theta, const float *O, const float *X, uint32_t *state, float *Vt, int *ends,
                                                   const int *lens, int N, int M, int waves);
__global__ void sdp_hard_affine_global_fwd_kernel(const float *theta, const float *O, const float *X, uint32_t *state, float *Vt, int *ends,
                                                  const int *lens, int N, int M, int waves);
__global__ void sdp_hard_affine_global_fwd_t_kernel(const float *theta, const float *O, const float *X, uint32_t *state, float *Vt, int *ends,
                                                    const int *lens, int N, int M, int waves);
__global__ void sdp_hard_affine_global_val_kernel(const float *theta, const float *O, const float *X, uint32_t *state, float *Vt, int *ends,
                                                  const int *lens, int N, int M, int waves);
__global__ void sdp_hard_affine_global_val_t_kernel(const float *theta, const float *O, const float *X, uint32_t *state, float *Vt, int *ends,
                                                    const int *lens, int N, int M, int waves);
__global__ void sdp_hard_affine_semiglobal_fwd_kernel(const float *theta, const float *O, const float *X, uint32_t *state, float *Vt,
                                                      int *ends, const int *lens, int N, int M, int waves, int free_ends);
__global__ void sdp_hard_affine_semiglobal_fwd_t_kernel(const float *theta, const float *O, const float *X, uint32_t *state, float *Vt,
                                                        int *ends, const int *lens, int N, int M, int waves, int free_ends);
__global__ void sdp_hard_affine_semiglobal_val_kernel(const float *theta, const float *O, const float *X, uint32_t *state, float *Vt,
                                                      int *ends, const int *lens, int N, int M, int waves, int free_ends);
__global__ void sdp_hard_affine_semiglobal_val_t_kernel(const float *theta, const float *O, const float *X, uint32_t *state, float *Vt,
                                                        int *ends, const int *lens, int N, int M, int waves, int free_ends);
__global__ void sdp_hard_affine_local_walk_kernel(const uint32_t *state, const int *ends, const float *Et, float *E, float *GO, float *GX,
                                                  int *states, int *counts, const int *lens, int N, int M, int cap, int ymx);
}

#endif  // SDP_HARD_AFFINE_H_
