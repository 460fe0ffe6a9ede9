// sdp_device.h -- device helpers shared by the kernel files of this library: cross-lane moves, fast exp / log, buffer descriptors,
// explicit-DS LDS accessors, the pass descriptions (Traits, Kind), the packed-state codec, the carries, the cache-policy and
// ablation constants and the per-cell loss terms.  Included by sdp_kernels.hip (the sweep), sdp_aux.hip (the small kernels) and
// sdp_gap.hip (the gap-score gradients, which decode the packed state); device code only.
#ifndef SDP_DEVICE_H
#define SDP_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sdp_kernels.h"

namespace sdp {

// ----------------------------------------------------------------------------------
// cross-lane moves (DPP full-wave shifts/rotates; gfx9 family encodings)
// ----------------------------------------------------------------------------------
constexpr int DPP_WAVE_SHL1 = 0x130;  // lane i <- lane i+1 ; lane 63 keeps `old`
constexpr int DPP_WAVE_ROL1 = 0x134;  // lane i <- lane (i+1)%64
constexpr int DPP_WAVE_SHR1 = 0x138;  // lane i <- lane i-1 ; lane 0 keeps `old`
constexpr int DPP_WAVE_ROR1 = 0x13C;  // lane i <- lane (i-1)%64

template <int CTRL>
__device__ __forceinline__ int dpp_i32(int old, int src)
{
    return __builtin_amdgcn_update_dpp(old, src, CTRL, 0xf, 0xf, false);
}

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double old, double src)
{
    const int lo = dpp_i32<CTRL>(__double2loint(old), __double2loint(src));
    const int hi = dpp_i32<CTRL>(__double2hiint(old), __double2hiint(src));
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ float fast_exp(float x)  // e^x via v_exp_f32 (2^x)
{
    return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f);
}
__device__ __forceinline__ float fast_log(float x)  // ln x via v_log_f32 (log2 x)
{
    return __builtin_amdgcn_logf(x) * 0.69314718055994530942f;
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base, unsigned bytes)
{
    // raw buffer (stride 0), 32-bit data format; out-of-range loads return 0, stores are dropped
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)bytes, 0x00020000);
}

constexpr unsigned OOB = 0x80000000u;  // voffset that is out of range for every buffer we build

// Ablation switches for timing experiments (tools/gpu_tune.py builds variants with -DSDP_ABL=mask);
// results are wrong when any bit is set.  bit0: no global stores, bit1: no global loads, bit2: no strip
// hand-off waits, bit3: keep every load/store but replace the recurrence by a copy.
#ifndef SDP_ABL
#define SDP_ABL 0
#endif
#ifdef SDP_EXPERIMENTS
#define SDP_EXP_BUILD 1
#else
#define SDP_EXP_BUILD 0  // default library: Params::dbg is ignored, no wrong-results switch is reachable
#endif
// Everything below used to be a compile-time switch of its own (31 of them by round 5).  Each was measured, one setting won, and
// the losing code paths were deleted in round 6 (their measurements: DESIGN_HISTORY.md, "Switches retired in round 6"; the code:
// git history).  What is left are the constants the winning settings fold to.
//   * fp32 backward sweep: a chunk whose carries, boundary values and cotangent are all +0 produces +0 everywhere: its steps are
//     skipped and its state rows not loaded (bit-identical; the control is the run-time flag SDP_NO_ZERO_SKIP);
//   * adjoint backward sweep: chunks over which E, the carries and the boundary values are all zero are not run (ZSKIP_A);
//   * cache policies (gfx950 aux bits: 1 = sc0, 2 = nt, 16 = sc1), profiles/r04_store_policy.txt, r05_steady_policies.txt: every
//     stream is touched once per sweep -- line-aligned input blocks nt, state loads nt, state stores sc1 (what stays in the
//     Infinity Cache between the forward and the backward sweep matters), E / Ed stores nt sc1, zero-fill stores default.
constexpr int AUX_ST_STORE = 16, AUX_ST_LOAD = 2, AUX_IN_LOAD = 0, AUX_LINES_LOAD = 2, AUX_OUT_STORE = 18, AUX_ZERO_FILL = 0;
constexpr bool ABL_NOSTORE = (SDP_ABL & 1) != 0;
constexpr bool ABL_NOLOAD = (SDP_ABL & 2) != 0;
constexpr bool ABL_NOSYNC = (SDP_ABL & 4) != 0;
constexpr bool ABL_NOMATH = (SDP_ABL & 8) != 0;
constexpr bool ABL_NOLDS = (SDP_ABL & 16) != 0;  // staged inputs bypass LDS (wrong data, same dependencies)
// Progress words live in LDS and are polled by other waves.  They are accessed with explicit DS
// instructions: a volatile access through a generic pointer compiles to flat_load + vmcnt(0),
// which drains every outstanding prefetch at each poll.
__device__ __forceinline__ int lds_load_i32(unsigned addr)
{
    int v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
// split form: issue the read, do other LDS reads behind it (a wave's DS instructions execute in order), wait once
__device__ __forceinline__ int lds_issue_i32(unsigned addr)
{
    int v;
    asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
__device__ __forceinline__ void lds_wait(int &v)
{
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v) : : "memory");
}
__device__ __forceinline__ void lds_store_i32(unsigned addr, int v)
{
    asm volatile("ds_write_b32 %0, %1" : : "v"(addr), "v"(v) : "memory");
}

template <class X>
__device__ __forceinline__ void keep(X &x)
{
    asm volatile("" : "+v"(x));
}

// ----------------------------------------------------------------------------------
// pass descriptions
// ----------------------------------------------------------------------------------
// Q formats: the forward sweep writes the weights either compact (Q_PACKED, read by the backward sweep) or as
// float2 (Q_EXACT, read by the two adjoint sweeps, whose products with the -- possibly large -- directional
// derivatives need the relative precision of fp32 for small weights as well).
enum { Q_NONE = 0, Q_PACKED = 1, Q_EXACT = 2 };

template <int PASS, bool QX>
struct Traits;
template <bool QX>
struct Traits<PASS_FWD, QX> {  // nw.py:46-62
    static constexpr int SIN = 2, SOUT = 0;
    static constexpr int QIN = Q_NONE, QOUT = QX ? Q_EXACT : Q_PACKED;
    static constexpr bool DIN = false, DOUT = false;
    static constexpr bool REV = false;
};
template <bool QX>
struct Traits<PASS_BWD, QX> {  // nw.py:120-135
    static constexpr int SIN = 0, SOUT = 1;
    static constexpr int QIN = QX ? Q_EXACT : Q_PACKED, QOUT = Q_NONE;  // QX: the training path's float2 state
    static constexpr bool DIN = false, DOUT = false;
    static constexpr bool REV = true;
};
template <bool QX>
struct Traits<PASS_AFWD, QX> {  // nw.py:178-199
    // QX = true here means: the seed Ztheta is not read but formed from the loss's operands -- three staged planes
    // (ref, pred, G) instead of (Ztheta, ZA); see "fused loss seed" in the step body
    static constexpr int SIN = QX ? 3 : 2, SOUT = 0;
    static constexpr int QIN = Q_EXACT, QOUT = Q_NONE;
    static constexpr bool DIN = false, DOUT = true;
    static constexpr bool REV = false;
};
template <bool QX>
struct Traits<PASS_ABWD, QX> {  // nw.py:251-267
    static constexpr int SIN = 1, SOUT = 1;
    static constexpr int QIN = Q_EXACT, QOUT = Q_NONE;
    static constexpr bool DIN = true, DOUT = false;
    static constexpr bool REV = true;
};

// The packed state (read by the backward sweep only; see Q_EXACT above): two 20-bit fields per cell, 5 bytes (round 4; rounds
// 1-3 kept two 24-bit fields, 6 bytes; 18-bit fields were built in round 5, gated by emulation and NOT adopted -- one per cent of
// time for three quarters of the margin; two unorm16 per cell were rejected in round 1: their rounding error is carried along an
// alignment path like a random walk and passes 1e-4 on E beyond ~1000 residues.  DESIGN.md section 2, DESIGN_HISTORY.md).
// A field is the low 20 bits of the float f = 8 + q * (1 - 2^-19): in [8, 16) one ulp is 2^-20, so the fma's own rounding puts q on
// a grid of 2^-20 (absolute error <= 2^-21 = 4.8e-7 per weight; emulated on the float64 oracle's weights,
// tools/emu_state_formats.py: max |dE| 9e-7 on the benchmark's scores, 3.4e-6 on peaked ones at 512 x 512 -- the 1e-4 bound is 30x
// away, and problems with N + M > 4096 take the exact state).  The factor keeps the field below 2^20 for q <= 1 + 9e-7 -- a weight
// computed as c / sum * u can exceed 1 by a few ulp -- so no clamp is needed; a saturated weight (anything within 2^-21 of 1)
// decodes to exactly 1, a weight below 2^-21 to exactly 0, so a saturated path loses nothing.  Four cells -- eight fields, x0 y0 x1
// y1 x2 y2 x3 y3 from bit 0 up -- fill five dwords; the 20 dwords of a 16-step block are stored as five rows of one dwordx4 per
// lane (sdp_kernels.h).  The derivative state Qd is signed and unbounded and stays float2.
constexpr float QF_SCALE = 0.99999809265136718750f;    // 1 - 2^-19
constexpr float QF_UNSCALE = 1.0000019073486328125f;   // 1 + 2^-19 = 1 / (1 - 2^-19) to fp32
constexpr float QF_BASE = 8.0f;
// raw bits fx[k], fy[k] of the four cells' biased floats (0x41000000 | field) -> five dwords
__device__ __forceinline__ void q20_pack4(const unsigned *fx, const unsigned *fy, unsigned *w)
{
    // (a left shift pushes the exponent byte out of the dword, and bits 20-23 of a biased float are zero, so only fields
    //  that stay below bit 24 after their shift need masking)
    w[0] = (fx[0] & 0xfffffu) | (fy[0] << 20);
    w[1] = __builtin_amdgcn_ubfe(fy[0], 12, 8) | (fx[1] << 8) | (fy[1] << 28);
    w[2] = __builtin_amdgcn_ubfe(fy[1], 4, 16) | (fx[2] << 16);
    w[3] = __builtin_amdgcn_ubfe(fx[2], 16, 4) | ((fy[2] & 0xfffffu) << 4) | (fx[3] << 24);
    w[4] = __builtin_amdgcn_ubfe(fx[3], 8, 12) | (fy[3] << 12);
}
__device__ __forceinline__ float q20_field(unsigned u)  // field in the low 20 bits of u, anything above -> f - 8
{
    // gfx9 allows one constant-bus operand per VALU instruction, so the compiler, given two literals ((u & mask) | bias), emits
    // two instructions; with the bias in a register the bit-field insert does it in one (15.5 -> 13.75 VALU per step).  Same bits.
    unsigned r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "s"(0xfffffu), "v"(u), "v"(0x41000000u));
    return __uint_as_float(r) - 8.0f;
}
// (f - 8) of both weights of cell `sub` (0..3) of a five-dword record; the caller multiplies by QF_UNSCALE
__device__ __forceinline__ float2 q20_unpack(const unsigned *w, int sub)
{
    switch (sub) {
    case 0: return make_float2(q20_field(w[0]), q20_field(__builtin_amdgcn_alignbit(w[1], w[0], 20)));
    case 1: return make_float2(q20_field(w[1] >> 8), q20_field(__builtin_amdgcn_alignbit(w[2], w[1], 28)));
    case 2: return make_float2(q20_field(__builtin_amdgcn_alignbit(w[3], w[2], 16)), q20_field(w[3] >> 4));
    default: return make_float2(q20_field(__builtin_amdgcn_alignbit(w[4], w[3], 24)), q20_field(w[4] >> 12));
    }
}

// Exact-state weights: the largest of the three is formed as 1 - (the other two).  c/sum*u goes through an
// approximate reciprocal and two products (~1.5 ulp): harmless for a weight of 0.3, but a weight that the reference
// -- which divides in float64 and rounds once (nw.py:21-22,115) -- stores as exactly 1.0 would come out as
// 1 +- 1e-7, and the adjoint sweeps turn such an error into (1 - q) * a, relative to a difference that should be
// 0: on long, peaked alignments it reached 1e-3 of Ed.  The small weights carry the same relative error, so the
// complement is accurate to 1e-7 * (1 - q).  When the match weight qm is the largest nothing has to be done: the
// readers form qm = 1 - qx - qy anyway.
typedef float f32x2 __attribute__((ext_vector_type(2)));  // operand of the packed fp32 instructions (v_pk_mul / v_pk_fma)

// 2^(theta log2e) = 2^tt * (1 + c) where tt = fl(theta * fl(log2e)) is what v_exp_f32 was given and
// c = ln2 * (theta * log2e - tt), the rounding of the product recovered exactly (fma) plus the low part of log2(e).
// |c| <= |tt| 2^-24: the second-order term is below 1e-12.
__device__ __forceinline__ f32x2 exp2_residual(f32x2 theta, f32x2 tt)
{
    constexpr float L_HI = 1.44269502162933349609375f, L_LO = 1.92596299112661746e-8f, LN2 = 0.69314718055994530942f;
    f32x2 d = __builtin_elementwise_fma(theta, (f32x2){L_HI, L_HI}, -tt);
    d = __builtin_elementwise_fma(theta, (f32x2){L_LO, L_LO}, d);
    return d * (f32x2){LN2, LN2};
}

__device__ __forceinline__ void q_sharpen(float &wx, float &wy, float wm)
{
    const float big = __builtin_fmaxf(wx, wy), small = __builtin_fminf(wx, wy);
    const float o = 1.0f - (small + wm);
    const float nb = big > 0.5f ? o : big;
    const bool xbig = wx >= wy;
    wx = xbig ? nb : wx;
    wy = xbig ? wy : nb;
}

// ----------------------------------------------------------------------------------
// carries
// ----------------------------------------------------------------------------------
// How a pass represents the values that flow from cell to cell (and across strips):
//   CK_F64 : float64, as the reference does internally (nw.py:49-53,125,182-185,256).
//   CK_F32 : float32.  Used by the backward sweep: E is a sum of non-negative products of weights
//            in [0,1], so there is no cancellation and fp32 accumulation stays ~1e-6 of the result.
//   CK_EXP : scaled exp-domain pair (a, e) with V = e*ln2 + ln(a), a in [0.5,1).  The forward
//            recurrence  V = theta + log(e^(A+up) + e^diag + e^(A+left))  becomes
//            alpha = c_theta * (c_A*(u + l) + d): one fma chain with no exp/log on the dependency
//            chain (the HMM "scaled forward algorithm").  theta and A are split into an integer
//            power of two (added to the exponent) and a factor in [1,2), and the three operands are
//            aligned to their largest exponent, so no finite input can overflow or cancel; every
//            rescale is an exact power of two, so the only rounding is the fp32 fma chain itself.
// (the enum and boundary_slot_bytes live in sdp_kernels.h: the host sizes the LDS rows by them.  Which pass uses which kind was a
// build-time choice until round 6; the alternatives -- a float64 forward, a float64 backward, an fp32 adjoint backward -- lost by
// measurement or by parity in rounds 1-2 and are gone.)

template <int PASS>
struct Kind {
    static constexpr int value = PASS == PASS_FWD ? CK_EXP : (PASS == PASS_BWD ? CK_F32 : CK_F64);
};

typedef unsigned long long u64;  // one boundary slot (LDS) / one edge value in registers

__device__ __forceinline__ u64 pack2(unsigned lo, unsigned hi) { return ((u64)hi << 32) | lo; }
__device__ __forceinline__ unsigned lo32(u64 x) { return (unsigned)x; }
__device__ __forceinline__ unsigned hi32(u64 x) { return (unsigned)(x >> 32); }

// V = 0 in the exp-domain representation: 0.5 * 2^1
// Windowed form of the exp-domain forward (see steps_wf in sweep): values of one chunk are plain floats relative
// to a per-lane exponent ("frame").  After the K steps every value a lane produced must lie in [WF_LO, WF_HI]:
//   * overflow anywhere in a step gives inf (or NaN), which stays in the lane's value and trips the upper test;
//   * the factors 2^theta and 2^A of every step must not exceed WF_FMAX = 2^12 (|theta|, |A| <= 8.3; anything
//     else, including NaN, goes to the normalised form).  Then a value >= WF_LO = 2^-100 proves that the sum it
//     was made from was a normal float (>= 2^-112), and values <= WF_HI = 2^110 keep every sum below 2^124, so its
//     reciprocal is a normal float too.  A = -inf (2^A = 0) is fine.
// A chunk that fails a test is redone in the per-step-normalised form; nothing was committed before the test.
// WF_HI also leaves room for the consumers of published values (value * 2^A * 2 + ... stays below 2^128).
// Values mostly grow along a row (fastest in the lower left corner of the matrix: ~5 bits per step, and 10-20 in a row's first
// columns), so a lane's frame is placed WF_BIAS bits above the exponent of its current value: it starts the block at
// 2^-WF_BIAS, with 110 + WF_BIAS bits of room upwards and 100 - WF_BIAS downwards.  Round 4: 40 -> 64.  With 40 the head
// blocks of the two bottom strips of a 512 x 512 pair failed the range test (rows 400+ gain 152-158 bits in the 16 steps
// after their first column; cycle stamps: 6 + 5 blocks at 7-10k cycles instead of 2k, all on the pair's critical path --
// strip 7 cannot start before strip 6's head is through), ~11 % of the launch.  Blocks that fail, by bias (40 / 56 / 64 /
// 80) on 512 x 512: benchmark scores 8 / 0 / 0 / 0; theta x 8: 191 / 127 / 110 / 73; theta - 2: 0 / 0 / 0 / 159; theta x 8 - 4:
// 47 / 38 / 35 / 76; A + 0.5: 10 / 0 / 0 / 0 (emulated from the float64 V).  Which form a block runs in does not change a
// cell's value, and only in the packed state whether its weights are sharpened (see norm_block).
constexpr unsigned WF_HI = 0x76800000u;  // 2^110
constexpr unsigned WF_LO = 0x0d800000u;  // 2^-100
constexpr unsigned WF_FMAX = 0x45800000u;  // 2^12
#ifndef SDP_WF_BIAS
#define SDP_WF_BIAS 64
#endif
constexpr int WF_BIAS = SDP_WF_BIAS;
constexpr int WB = 16;  // steps per frame (every chunk length is a multiple)
constexpr int FRAME_NONE = (int)0x80000000;  // published chunk is not in one frame (per-value exponents apply)
constexpr float EXP_ONE_A = 0.5f;
constexpr int EXP_ONE_E = 1;
constexpr int ZERO_E = -(1 << 29);   // the exponent a zero operand takes in the normalised forward form: below every real one

template <int KIND>
__device__ __forceinline__ u64 edge_zero()
{
    if constexpr (KIND == CK_EXP) return pack2(__float_as_uint(EXP_ONE_A), (unsigned)EXP_ONE_E);
    else return 0ull;  // +0.0 as f64 and as f32
}

// bank-spreading permutation of the staged-input ring (see "Staged INPUT geometry"): 0,4,1,5,2,6,3,7
__device__ __forceinline__ constexpr int ring_pi(int x) { return ((x & 1) << 2) | (x >> 1); }

// per-lane recurrence state carried from step to step
struct Carry {
    // CK_F64: a = own V / value sent up, b = previous `up` / own py, c = pm of the previous step
    double a, b, c;
    // CK_F32 (reverse): same roles in fp32
    float fa, fb, fc;
    // CK_EXP (forward): own (alpha, exponent), and the diagonal predecessor's pair
    float xa;
    int xe;
    float da;
    int de;
};

// per-cell terms of the masked alignment losses (used by the loss kernels and by the fused seed of the adjoint forward)
__device__ __forceinline__ float loss_clamp(float p)
{
    const float eps = 3e-8f;  // losses.py:27
    return fminf(fmaxf(p, eps), 1.0f - eps);
}

// value of one counted cell (kind as above).  1 - p rounded to fp32 is off by up to 3e-8, which is all of log(1 - p) at
// p = 3e-8 and 3e-6 of it at p = 0.01 -- a pair whose counted cells are all such would miss the float64 value by that
// much.  So 1 - p = q + e exactly (Fast2Sum, p <= 1), and log(1 - p) = log(q) + e / q, with e / q taken as e: e != 0 only
// where p < 1/2, and there the difference, e * p / q, is below 6e-8 of log(1 - p).  (log1pf does the same job, but
// measured on MI355X at 256 x 512^2 the forward kernel then took 294-314 us instead of 142-146 us.)  The square of kinds 1 and 2 is formed in float64: d itself is an fp32
// value, so d * d is exact there, where in fp32 it would lose bits below 1e-19 (denormal squares) and vanish below 1e-23
// -- a pair whose vector is all that small would then get norm 0 instead of the reference's norm
__device__ __forceinline__ double loss_term(float r, float y, int kind)
{
    if (kind == 0) {
        const float p = loss_clamp(y);
        const float q = 1.0f - p, e = (1.0f - q) - p;
        return (double)(r * logf(p) + (1.0f - r) * (logf(q) + e));
    }
    const double d = (double)(kind == 1 ? r * y : r - y);
    return d * d;
}
// derivative factor of one counted cell w.r.t. the predicted value
__device__ __forceinline__ float loss_dterm(float r, float y, float sc, int kind)
{
    if (kind == 0) {
        const float eps = 3e-8f;
        return (y >= eps && y <= 1.0f - eps) ? sc * (r / y - (1.0f - r) / (1.0f - y)) : 0.f;  // clamp passes the gradient inside only
    }
    return kind == 1 ? sc * r * r * y : sc * (r - y);
}

}  // namespace sdp

#endif  // SDP_DEVICE_H
