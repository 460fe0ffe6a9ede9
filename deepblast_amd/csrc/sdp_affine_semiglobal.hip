// sdp_affine_semiglobal.hip -- the affine-gap soft SEMI-GLOBAL operator: the global operator of csrc/sdp_affine_global.hip with free
// end gaps (include/sdp.h: sdp_affine_semiglobal_*).  The planes, the recurrences of Vx, Vm, Vy, of q, E, GO and GX
// and the scaled arithmetic are that file's, instantiated from the same templates (csrc/sdp_affine_global_device.h, FREE = true);
// two things change, under the two bits of the kernel argument `free_ends`:
//
//     bit 1, y: the columns of y that hang over either end of x cost nothing -- a path may start in any cell of row 1 and end in
//               any cell of row n;                 bit 0, x: the same for rows -- start in any cell of column 1, end in column m
//     start   a start cell is entered in plane m alone: START, exp V = 1, stands above-left of it and is seen by the diagonal step
//             only (no path begins with a gap step).  Above-left of (1,1) always, of (1,j) under y, of (i,1) under x.
//     end     Vt = log sum over the end cells (i,j) and the planes s of exp V_s[i,j];  Ends = {(n,m)}, row n under y, column m
//             under x;  the backward seed is Eb_s[i,j] += Et exp(V_s[i,j] - Vt) at every end cell.
//
// Both bits: overlap alignment.  Transposition swaps the bits and the planes x and y.
//
//   forward   the global sweep with two selects.  START: a lane whose cell is a start cell replaces the cell above-left -- zeros, it
//             lies outside the table -- by (dm, de) = (0.5, 1) before the sum of plane m is formed, as lane 0 of strip 0 does for
//             (1,1); the record then has q[m<-m] = 1, which the backward sweep pushes out of the block.  END: the lane at an end cell
//             adds ax + am + ay on the cell's exponent into a private sum, a float64 mantissa on an integer exponent (up to n + m
//             terms; 4000 sequential fp32 adds would not hold Vt).  Row n lives in one lane of the last strip, column m is one
//             step per lane and strip: a wave looks for end cells only in those chunks, behind one scalar branch.  After the
//             sweep the lanes' sums are added in a fixed order through LDS, and one lane writes Vt = log(sum) + e ln 2 in float64.
//   weights   the backward sweep wants w_s = exp(V_s - Vt) in the .w of an end cell's records, and no cell knows the total when
//             it is stored.  So the sweep leaves the raw mantissas a_s in .w and the cell's exponent in a tail behind the
//             records, N + M words a pair (one per row for column m, one per column for row n); once the total is known the
//             workgroup rewrites the .w of its n + m - 1 end cells to a_s 2^(e - e_total) / sum.  A weight that underflows is +0.
//   value     the same sweep with the records, the tail and the rewrite compiled out: the same bits of Vt.
//   backward  the global mirror sweep, seeded with Et w_s at every end cell instead of at (n,m) alone: no exp, no Vt, no load the
//             global sweep does not have.
#include "sdp_affine_global_device.h"

extern "C" __global__ void __launch_bounds__(512) sdp_affine_semiglobal_fwd_kernel(const float *theta, const float *O, const float *X,
                                                                                   float4 *state, float *Vt, const int *lens, int N, int M,
                                                                                   int waves, int free_ends)
{
    affine_global_forward<true, true>(theta, O, X, state, Vt, lens, N, M, waves, free_ends);
}
extern "C" __global__ void __launch_bounds__(512) sdp_affine_semiglobal_val_kernel(const float *theta, const float *O, const float *X,
                                                                                   float4 *state, float *Vt, const int *lens, int N, int M,
                                                                                   int waves, int free_ends)
{
    affine_global_forward<false, true>(theta, O, X, state, Vt, lens, N, M, waves, free_ends);
}

extern "C" __global__ void __launch_bounds__(512) sdp_affine_semiglobal_bwd_kernel(const float4 *state, const float *Et, float *E, float *GO,
                                                                                   float *GX, const int *lens, int N, int M, int W,
                                                                                   int free_ends)
{
    affine_global_backward<true>(state, Et, E, GO, GX, lens, N, M, W, free_ends);
}
