// sdp_affine_global.hip -- the affine-gap soft global operator: a differentiable Needleman-Wunsch in which opening a gap and
// extending it are priced separately, the Gotoh form (include/sdp.h: sdp_affine_global_*)
//
//     Vm[1,1] = theta[1,1];  elsewhere  Vm[i,j] = theta[i,j] + log(exp Vx[i-1,j-1] + exp Vm[i-1,j-1] + exp Vy[i-1,j-1])    planes x = 0, m = 1,
//     Vx[i,j] = theta[i,j] + log(exp(X[i,j] + Vx[i-1,j]) + exp(O[i,j] + Vm[i-1,j]) + exp(O[i,j] + Vy[i-1,j]))         y = 2: the step that
//     Vy[i,j] = theta[i,j] + log(exp(O[i,j] + Vx[i,j-1]) + exp(O[i,j] + Vm[i,j-1]) + exp(X[i,j] + Vy[i,j-1]))         entered the cell
//     q[s<-s'] = the term of plane s' over the sum in the log of plane s;  Vt = log(exp Vx[n,m] + exp Vm[n,m] + exp Vy[n,m])
//     Eb_s[i,j] = [(i,j) = (n,m)] Et w_s + q[x<-s][i+1,j] Eb_x[i+1,j] + q[m<-s][i+1,j+1] Eb_m[i+1,j+1] + q[y<-s][i,j+1] Eb_y[i,j+1],  w_s = exp(V_s[n,m] - Vt)
//     E = Eb_x + Eb_m + Eb_y;  GX = Eb_x q[x<-x] + Eb_y q[y<-y];  GO = Eb_x (q[x<-m] + q[x<-y]) + Eb_y (q[y<-x] + q[y<-m])
//
// a path starts at (1,1) and ends at (n,m): a V outside the table is -inf, and so is a plane without a predecessor.  The schedule is
// the strip schedule (csrc/sdp_strip_device.h) as csrc/sdp_affine_local.hip runs it; the ARITHMETIC is not that
// file's.  A global V is the score of a whole path, hundreds to thousands: one ulp of it reaches 5e-4, and a log-domain cell puts
// that error into every weight.  So a cell carries exp V, SCALED: three fp32 mantissas ax, am, ay on ONE shared integer exponent e,
//     exp V_s = a_s 2^e,   the largest of the three in [0.5, 1),   an all-zero cell (no path reaches it): a = 0, e = -2^29,
// the form of the main sweep's carries.  exp theta, exp O and exp X are split into a mantissa in [1, 2) and an integer
// power of two when the inputs arrive, off the dependent chain (the product theta log2e with its residual: exp2_parts); -inf, and
// any score below -2^24 / log2e, has mantissa 0.  A cell then is three short sums of products, an exact alignment of the three
// planes by powers of two (ldexp) and a renormalisation by the exponent (frexp) of its largest plane: no exp and no log in the
// sweep loop.  Three kernels:
//
//   forward   one workgroup per pair, one wave per strip of 64 rows (lane = row), swept along the anti-diagonals: at step s lane l
//             is at column s - l, the cell above arrives from lane l - 1 by DPP (four words: three mantissas and the exponent), the
//             cell above-left is what arrived one step before.  The waves of a workgroup run consecutive strips three chunks of 32
//             steps apart; a strip's bottom row crosses to the next strip through LDS, four words per column, and a barrier per
//             chunk is the only synchronisation.  The path's start is one value: lane 0 of strip 0 begins with the cell above-left
//             of (1,1) holding 1 in plane m.  The lane that sweeps cell (n,m) keeps it; after the sweep it rebuilds
//             Vt = log(ax + am + ay) + e ln 2 in float64, once per pair, and writes the end weights w_s = a_s / (ax + am + ay).
//   records   48 bytes per cell, one record {q[s<-x], q[s<-m], q[s<-y], w_s} per plane s, in the layout of the local family:
//             state[((((pair * strips(N) + S) * chunks(M) + c) * 32 + t) * 3 + s) * 64 + lane].  w_s is 0 except in the records of
//             the end cell (n,m), where the forward sweep leaves the end weights for the backward sweep.  Only cells of the pair's
//             block are written, and only those are used.
//   value     the forward sweep with the records compiled out: the same arithmetic, the same bits of Vt.
//   backward  the mirror sweep of the local family without its per-cell seed: the only seed is Et w_s at (n,m), so no exp and no
//             Vt.  GO and GX are by-products; the workgroup writes +0 outside the pair's block before it sweeps.
//
// The sweeps themselves are templates in csrc/sdp_affine_global_device.h, shared with the family's free-end-gap member
// (csrc/sdp_affine_semiglobal.hip); the three kernels here are their FREE = false instances.
#include "sdp_affine_global_device.h"

extern "C" __global__ void __launch_bounds__(512) sdp_affine_global_fwd_kernel(const float *theta, const float *O, const float *X, float4 *state,
                                                                               float *Vt, const int *lens, int N, int M, int waves)
{
    affine_global_forward<true, false>(theta, O, X, state, Vt, lens, N, M, waves, 0);
}
extern "C" __global__ void __launch_bounds__(512) sdp_affine_global_val_kernel(const float *theta, const float *O, const float *X, float4 *state,
                                                                               float *Vt, const int *lens, int N, int M, int waves)
{
    affine_global_forward<false, false>(theta, O, X, state, Vt, lens, N, M, waves, 0);
}

extern "C" __global__ void __launch_bounds__(512) sdp_affine_global_bwd_kernel(const float4 *state, const float *Et, float *E, float *GO,
                                                                               float *GX, const int *lens, int N, int M, int W)
{
    affine_global_backward<false>(state, Et, E, GO, GX, lens, N, M, W, 0);
}
