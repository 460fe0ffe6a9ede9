// sdp_api.hip -- host side of the C ABI declared in include/sdp.h.
// Validates arguments, sizes the launch and enqueues one kernel per call on the
// caller's stream.  No device allocation, no synchronisation.  Process-wide state: one 64-byte block of
// host-pinned status words per device (created on the first launch there), through which a kernel reports a
// strip hand-off that timed out; the experiment switches (sdp_set_debug) exist only in -DSDP_EXPERIMENTS builds.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <initializer_list>
#include <mutex>

#include "sdp_gap.h"
#include "sdp_sample.h"
#include "sdp_hard.h"
#include "sdp_soft_local.h"
#include "sdp_soft_local_sample.h"
#include "sdp_sparsemax.h"
#include "sdp_affine_global.h"
#include "sdp_affine_global_sample.h"
#include "sdp_affine_semiglobal_sample.h"
#include "sdp_affine_local.h"
#include "sdp_affine_local_sample.h"
#include "sdp_hard_affine.h"
#include "sdp_kernels.h"

namespace {

thread_local char g_err[256] = "";
#ifdef SDP_EXPERIMENTS
std::atomic<int> g_dbg{0};
std::atomic<unsigned long long *> g_trace{nullptr};
#endif

// ---- per-device status words (host-pinned, device-visible) ----
// Published once per device under g_status_mu and read through atomics afterwards: launches from several host threads
// may race with the first launch on a device.  Created by sdp_init(device) -- or by the first launch there; a caller
// that captures launches into a hipGraph calls sdp_init first (an allocation inside a capture fails, and the launch
// would then run without a way to report a hand-off time-out).
constexpr int MAX_DEV = 64;
std::mutex g_status_mu;
std::atomic<int *> g_status_host[MAX_DEV];
std::atomic<int *> g_status_dev[MAX_DEV];
std::atomic<int> g_status_seen[MAX_DEV];  // time-outs already reported to the caller

int *status_words(int device)  // device pointer, or nullptr (then kernels cannot report)
{
    if (device < 0 || device >= MAX_DEV) return nullptr;
    if (int *d = g_status_dev[device].load(std::memory_order_acquire)) return d;
    std::lock_guard<std::mutex> lk(g_status_mu);
    if (int *d = g_status_dev[device].load(std::memory_order_relaxed)) return d;
    int *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    memset(h, 0, 64);
    if (hipHostGetDevicePointer((void **)&d, h, 0) != hipSuccess) {
        (void)hipHostFree(h);
        return nullptr;
    }
    g_status_seen[device].store(0);
    g_status_host[device].store(h, std::memory_order_release);
    g_status_dev[device].store(d, std::memory_order_release);
    return d;
}

int fail(int code, const char *msg)
{
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

int fail_hip(hipError_t e, const char *what)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return (int)e;
}

// One row of sdp_builds.def: what a build of the sweep is.  BUILDS is that table, and the only thing here that knows a build's
// number: the launch policy (plan) asks for a build by its properties (find).
struct Build {
    int id;
    const char *name;
    void (*kernel)(const sdp::Params);
    int pass, K, maxw, flags;   // flags: sdp::bf
};
using namespace sdp::bf;
#define SDP_IN_GROUP(g) 1
#define SDP_BUILD(ID, NAME, PASS, K, MAXW, FLAGS) {ID, #NAME, NAME, sdp::PASS, K, MAXW, FLAGS},
constexpr Build BUILDS[] = {
#include "sdp_builds.def"
};
#undef SDP_IN_GROUP
constexpr int NBUILDS = sizeof(BUILDS) / sizeof(BUILDS[0]);

// the columns that tell the builds of one pass apart (LINES follows from the pass and LAT)
constexpr int SELECT = QX | GEN | PARTS | NOPIPE | NOCLEAN | VALUE | LAT;
// ... and what a wanted property means to a pass whose builds do not have the column:
constexpr int settle(int pass, int want)
{
    // general pitch: builds whose staged blocks keep the column-aligned geometry at any pitch have no twin -- the latency forward
    // builds, the adjoint forward
    if ((pass == sdp::PASS_FWD && (want & LAT)) || pass == sdp::PASS_AFWD) want &= ~GEN;
    // only the forward sweep cleans, and its general-pitch and parts builds always do
    if (pass != sdp::PASS_FWD || (want & (GEN | PARTS))) want &= ~NOCLEAN;
    // only the packed throughput backward build exists with and without the pipelined chunk
    if (pass != sdp::PASS_BWD || (want & (QX | LAT | GEN | PARTS))) want &= ~NOPIPE;
    return want;
}
// the one build of `pass` with the wanted properties; nullptr if there is none, or more than one
constexpr const Build *find(int pass, int want)
{
    want = settle(pass, want);
    const Build *hit = nullptr;
    for (const Build &b : BUILDS)
        if (b.pass == pass && (b.flags & SELECT) == want) {
            if (hit) return nullptr;
            hit = &b;
        }
    return hit;
}
// Checked when this file is compiled: no id twice, and every build plan() can ask for exists exactly once -- any combination of
// `free` beside `fixed`.  A row added to or taken from sdp_builds.def that leaves the policy without its build, or with two, fails here.
constexpr bool served(int pass, int fixed, int free)
{
    for (int s = free;; s = (s - 1) & free) {
        if (!find(pass, fixed | s)) return false;
        if (!s) return true;
    }
}
constexpr bool ids_differ()
{
    for (int i = 0; i < NBUILDS; ++i)
        for (int j = 0; j < i; ++j)
            if (BUILDS[i].id == BUILDS[j].id) return false;
    return true;
}
static_assert(ids_differ(), "sdp_builds.def: two builds with one id");
static_assert(served(sdp::PASS_FWD, 0, LAT | QX | NOCLEAN | GEN | NOPIPE) && served(sdp::PASS_FWD, VALUE, LAT | NOCLEAN | GEN | NOPIPE) &&
                  served(sdp::PASS_BWD, 0, LAT | QX | NOCLEAN | GEN | NOPIPE) && served(sdp::PASS_FWD, PARTS, QX | GEN) &&
                  served(sdp::PASS_BWD, PARTS, QX | GEN) && served(sdp::PASS_AFWD, 0, QX | NOCLEAN | GEN | NOPIPE) &&
                  served(sdp::PASS_ABWD, 0, NOCLEAN | GEN | NOPIPE),
              "sdp_builds.def: the launch policy can ask for a build that does not exist, or exists twice");

int num_cus(int device)
{
    static thread_local int cached[64] = {0};
    if (device >= 0 && device < 64 && cached[device] > 0) return cached[device];
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0) n = 256;
    if (device >= 0 && device < 64) cached[device] = n;
    return n;
}

size_t lds_bytes(int pass, int K, int W, int mcap, size_t *stage_off, int nin = 0)
{
    const int nslot = 2;  // boundary rows are shared by alternate strips (see the kernel)
    size_t off = (size_t)nslot * mcap * sdp::boundary_slot_bytes(pass) + 64 + (size_t)nslot * sdp::FRAME_CAP * 4;  // boundary rows, progress words, frame words
    off = ((off + 15) & ~(size_t)15) + 16;   // (+ 16: the staged-output ring of wave 0 writes one float in front of itself, see FLUSH2)
    if (stage_off) *stage_off = off;
    return off + (size_t)W * sdp::stage_floats(pass, K, nin) * sizeof(float);
}

int check_shape(int B, int N, int M, int variant)
{
    if (B <= 0 || N <= 0 || M <= 0) return fail(SDP_E_SHAPE, "B, N and M must be positive");
    if (M > sdp::MAX_COLS) return fail(SDP_E_MAXCOLS, "M exceeds sdp_max_cols()");
    if (variant != SDP_NW && variant != SDP_SW) return fail(SDP_E_VARIANT, "variant must be SDP_NW or SDP_SW");
    if ((size_t)N * (size_t)M > ((size_t)1 << 28)) return fail(SDP_E_TOOBIG, "N*M exceeds 2^28 cells per pair");
    return 0;
}

// What a launch will use: which kernel build, how many waves per pair, how much LDS.  Pure function of the
// problem and the CU count (no device access), so that the policy can be tested without a GPU (sdp_plan).
struct Plan {
    const Build *v;
    int W;
    size_t lds, stage_off;
    int parts;   // strips per workgroup when the pairs are spread over several workgroups (0: one workgroup per pair)
};

// What a launch does about the state: the packed state (two 20-bit weights per cell), the exact (float2) state, the adjoint forward
// sweep's fused loss seed, or none at all -- the value-only forward sweep, which is the forward sweep without a state: no state
// format to pick, no state buffer to keep bridge rows in (no parts), nothing to route.
enum StateKind { ST_PACKED, ST_EXACT, ST_SEED, ST_VALUE };

// Strips per part when a pair is spread over several workgroups (sdp_kernels.hip, "PARTS"): one strip per wave of the
// 4-wave throughput builds.
constexpr int PART_STRIPS = 4;
inline int parts_per_pair(int N) { return (sdp::state_nstrips(N) + PART_STRIPS - 1) / PART_STRIPS; }

Plan plan(int pass, int B, int N, int M, bool has_lens, StateKind st, int cus, int forced_waves, bool general_pitch = false,
          int allow_parts = 1 /* 0 never, 1 where it pays, 2 wherever it is possible */)
{
    const bool exact_state = st == ST_EXACT;
    const int nstrips = sdp::state_nstrips(N);
    const int mcap = (M + 63) / 64 * 64;
    // Waves per pair.  A batch that occupies the GPU is bound by HBM/fabric traffic and runs best with one wave
    // per SIMD and long chunks; a smaller batch is bound by the length of the strip pipeline of a single pair,
    // which more waves (and the shorter-chunk latency builds) shorten.
    // With per-pair lengths the longest pairs set the time of a batch that does not queue up on the CUs, so such
    // a batch is treated like a small one (measured, 256 pairs with n, m ~ U[64,1024]: 1.27 ms vs 1.41 ms).
    const bool sweep12 = pass == sdp::PASS_FWD || pass == sdp::PASS_BWD;
    // measured crossover (round 5, 512 x 512, 256 CUs; profiles/r05_small_batches.txt): the forward sweep's latency build holds 133 us
    // up to 64 pairs and is at 170-190 us from 80 on, where the throughput build takes 148-151 -- ~72 pairs; the backward sweep's
    // 8-wave form is level with its 4-wave form up to 128 pairs
    const bool full = (pass == sdp::PASS_FWD ? B * 7 >= cus * 2 : B * 2 >= cus) && !(has_lens && B <= 2 * cus);
    // The build, by what it is (sdp_builds.def): the decisions below gather its properties in `want`, and find() settles the ones a
    // pass's builds do not have.  To begin with the pass's throughput build, without edge cleaning and without the pipelined chunk.
    int want = NOCLEAN | NOPIPE | (st == ST_VALUE ? VALUE : 0);
    const Build *v = find(pass, want);
    int W = forced_waves;
    if (W <= 0) {
        W = (sweep12 || pass == sdp::PASS_AFWD) ? (full ? 4 : 8) : SDP_DEFAULT_WAVES;  // (adj-bwd is compiled for <= 4)
        // More pairs than CUs: with 2 waves two workgroups share a CU (their LDS fits twice) and overlap each
        // other's ramps -- a round of 2*CUs pairs then takes 1.8x a 4-wave round of CUs pairs.  Pick the cheaper.
        const int r4 = (B + cus - 1) / cus, r2 = (B + 2 * cus - 1) / (2 * cus);
        if (full && sweep12 && B > cus && 181 * r2 < 100 * r4) W = 2;
    }
    if (sweep12) {
        // the throughput builds need 4 waves' worth of LDS for their longer chunks; fall back to the latency
        // builds when that does not fit (long M) or when more waves are wanted
        const int w4 = nstrips < 4 ? nstrips : 4;
        // (the packed backward build runs up to 8 waves since round 5, its general-pitch twin since round 6 -- the exact-state twins
        //  only 4: a launch that will end up in one of those is judged by their limit)
        const int maxw = (pass == sdp::PASS_BWD && exact_state) ? SDP_MAXW_BWD : v->maxw;
        if (W > maxw || lds_bytes(pass, v->K, w4, mcap, nullptr) > 160 * 1024) want |= LAT;
        if (exact_state) want |= QX;
    }
    const int nin = (pass == sdp::PASS_AFWD && st == ST_SEED) ? 3 : 0;   // three staged planes (ref, pred, G)
    if (nin) want |= QX;
    // the aligned-pitch forward builds come without any edge cleaning (sdp_kernels.hip "need_clean"); per-pair lengths or partial
    // strips take their twins that carry it
    if (pass == sdp::PASS_FWD && (has_lens || (N & 63) != 0)) want &= ~NOCLEAN;
    if (general_pitch) want |= GEN;
    // The packed backward sweep's pipelined twin (sdp_kernels.hip, sdp_bwd_pipe_kernel) trades instruction issue for memory
    // latency.  Steady-state A/B over 24 shapes (tools/steady.py, +- 0.3 us; profiles/r05_steady_pipe.txt): it pays 2.3 % where
    // every CU holds ONE pair of long rows (256 x 1024^2, 256 x 512 x 1024), is level at 256 x 768 x 640 / 300 x 2000 / 192 x 1024^2, and
    // costs 1.1-3.7 % everywhere else -- shorter rows (the headline 256 x 512^2: 279.0 vs 272.5 us; 256 x 2048 x 256: 2.7 %), fewer
    // pairs than CUs (128 x 1024^2), more (384 x 1024^2, 512 x 768^2), 8 waves per pair (64 x 512^2).  So: only there.
    const bool bwd_pipe_pays = W == 4 && B <= cus && B * 8 >= cus * 7 && M >= 1024 && (long long)N * M >= 450000;
    if (bwd_pipe_pays) want &= ~NOPIPE;   // (find: a general-pitch launch has no such twin and keeps its build)
    v = find(pass, want);
    // A pair over several workgroups (sdp_kernels.hip, "PARTS"): parts of four strips, each on a CU of its own, one strip
    // per wave of the 4-wave throughput builds, instead of one CU taking all the pair's strips in rounds.  It pays only
    // where CUs would otherwise idle AND the pair is long enough for the extra lag per bridge (measured, round 3, us
    // forward / backward, one workgroup per pair -> parts):
    //   per-pair lengths, 256 pairs: n, m <= 1022 x 1020 (BASELINE configs[2]) 640 / 610 -> 515 / 465; <= 640^2 301 / 245 ->
    //   287 / 240; <= 512^2 (two parts) 199 / 169 -> 210 / 148; 128 pairs <= 512^2 170 / 157 -> 194 / 146; 64 pairs <= 1022 x 1020
    //   532 / 385 -> 462 / 309; more pairs than CUs, <= 1022 x 1020: 384 pairs 752 / 761 -> 778 / 743, 512 pairs 832 / 1023 ->
    //   1000 / 950, 700 pairs 998 / 1188 -> 1250 / 1300;
    //   equal pairs: 16 x 1024^2 445 / 330 -> 451 / 291; 64 x 640 x 500 240 / 163 -> 260 / 183 (worse); 16 x 512^2 worse.
    // So (round 3; round 5's re-measurement below drops the backward sweep with per-pair lengths): with per-pair lengths whenever
    // the batch does not outnumber the CUs -- the forward sweep from three parts on, the backward sweep from two; equal pairs
    // only the backward sweep of pairs of four parts.  The adjoint pair (float64
    // carries) keeps one workgroup per pair.
    int parts = 0;
    const bool parts_fit = sweep12 && st != ST_VALUE && forced_waves <= 0 && nstrips > PART_STRIPS;
    // Round 5, re-measured after the backward sweep's changes (profiles/r05_parts_table.txt; us, one workgroup per pair -> parts):
    // with per-pair lengths the BACKWARD sweep no longer gains from parts anywhere but at BASELINE configs[2] (540 -> 512-522,
    // and 515 when only the forward sweep uses them) and loses elsewhere (<= 640^2: 213 -> 236, <= 512^2: 146 -> 160, 64 pairs
    // <= 1022 x 1020: 336 -> 355, 32 pairs <= 2000 x 1000: 528 -> 582): dropped.  The forward sweep keeps them from three parts
    // on (<= 1022 x 1020: 600 -> 514, <= 640^2: 277 -> 257, 64 pairs: 510 -> 400; <= 512^2: 176 -> 195, not taken), equal pairs
    // the backward sweep of a few pairs of more than twelve strips (16 x 1024^2: 303 -> 279).
    const bool parts_pay = B <= cus && (has_lens ? (pass == sdp::PASS_FWD && nstrips > 2 * PART_STRIPS)
                                                 : (pass == sdp::PASS_BWD && nstrips > 3 * PART_STRIPS && (long long)B * parts_per_pair(N) <= cus));
    if (parts_fit && (allow_parts == 2 || (allow_parts == 1 && parts_pay))) {
        const Build *tv = find(pass, (want & (QX | GEN)) | PARTS);
        if (lds_bytes(pass, tv->K, PART_STRIPS, mcap, nullptr) <= 160 * 1024) {
            v = tv;
            W = PART_STRIPS;
            parts = PART_STRIPS;
        }
    }
    if (W > v->maxw) W = v->maxw;
    if (W > nstrips) W = nstrips;
    size_t off = 0, lds = 0;
    for (;; --W) {  // fewer waves if the boundary rows (long M) plus staging exceed the 160 KiB of LDS
        lds = lds_bytes(pass, v->K, W, mcap, &off, nin);
        if (lds <= 160 * 1024 || W == 1) break;
    }
    // Two-wave workgroups (more pairs than CUs) are meant to share a CU in PAIRS, one wave per SIMD.  Since round 5 the backward
    // build needs fewer than 256 registers, so the hardware would also take four of them -- two waves per SIMD, each at half
    // speed, other CUs short of work: 247 -> 262 us at 512 x 512^2.  Asking for half a CU's LDS keeps it at two.
    if (sweep12 && W == 2 && B > cus && lds < 80 * 1024) lds = 80 * 1024;
    return {v, W, lds, off, parts};
}

// Where the 32-step units of the skewed state live (sdp_kernels.hip, "Skewed state addressing"): every (pair, strip) is one
// contiguous stream of units.  (A "marching" layout -- unit u of every (pair, strip) in one slab, so that a batch whose pairs
// advance in lockstep sweeps memory front to back -- measured equal in round 3 and was removed in round 6: the sweeps are not
// bound by the order in which memory is visited.  The two strides stay parameters of the kernels.)
// All four sweeps of a problem (B, N, M) derive the same layout from the same three numbers.
void state_layout(sdp::Params &p)
{
    const size_t units = (size_t)p.tpad / sdp::STATE_UNIT_STEPS;
    p.st_ps = units * sdp::STATEQ_UNIT_BYTES;
    p.st_us = sdp::STATEQ_UNIT_BYTES;
    p.st2_ps = units * sdp::STATE2_UNIT_BYTES;
    p.st2_us = sdp::STATE2_UNIT_BYTES;
}

// A kernel of an EARLIER call on this device gave up waiting for a strip hand-off: its results are wrong.  Reported
// once, by the next call on the device (or by sdp_device_status), as SDP_E_HANDOFF.
int pending_handoff_error(int device)
{
    if (device < 0 || device >= MAX_DEV) return 0;
    const volatile int *h = g_status_host[device].load(std::memory_order_acquire);
    if (!h) return 0;
    const int n = h[0];
    // exactly one caller reports a given count: the one whose exchange moves `seen` to it
    int seen = g_status_seen[device].load();
    do {
        if (n == seen) return 0;
    } while (!g_status_seen[device].compare_exchange_weak(seen, n));
    snprintf(g_err, sizeof(g_err),
             "a strip hand-off timed out in an earlier launch on device %d (%d so far; first: pair %d, strip %d, chunk %d, "
             "pass %d): the results of that launch are invalid",
             device, n, h[1], h[2], h[3] & 0xffffff, (h[3] >> 24) & 0xff);
    return SDP_E_HANDOFF;
}

// Variable-length batches with more pairs than CUs run longest-first.  The order is computed by the forward call
// (sdp_order_kernel) into the tail of the state buffer it fills, and the other sweeps -- which receive that state
// and must be given the same lengths -- read it from there.
size_t packed_body_bytes(int B, int N, int M)
{
    return (size_t)B * sdp::state_nstrips(N) * (sdp::state_tpad(M) / sdp::STATE_UNIT_STEPS) * sdp::STATEQ_UNIT_BYTES;
}
bool wants_order(int B, int N, const int32_t *lens, int device)
{
    (void)N;
    return lens != nullptr && B > num_cus(device);
}
const int *order_in_state(const void *state, int B, int N, int M, bool exact)
{
    const size_t body = exact ? (size_t)B * sdp::state_rows2(N, M) * 64 * sizeof(float2)
                              : packed_body_bytes(B, N, M);
    return reinterpret_cast<const int *>(static_cast<const char *>(state) + body);
}
// ... and behind the order: the bridge rows between the parts of a pair (8-byte granules; reset before every launch
// that uses them, so the forward and the backward sweep share the room)
size_t bridge_bytes(int B, int N, int M)
{
    const int np = parts_per_pair(N);
    return np > 1 ? (size_t)B * (np - 1) * sdp::xb_row_granules(M) * 8 : 0;
}
// ... and behind those the dispatch order of the parts of a batch with per-pair lengths (one int per workgroup)
size_t parts_map_bytes(int B, int N)
{
    const int np = parts_per_pair(N);
    return np > 1 ? ((size_t)B * np * 4 + 255) / 256 * 256 : 0;
}
unsigned long long *bridge_in_state(const void *state, int B, int N, int M, bool exact)
{
    return reinterpret_cast<unsigned long long *>(const_cast<char *>(reinterpret_cast<const char *>(order_in_state(state, B, N, M, exact))) +
                                                  sdp::state_order_bytes(B));
}

// flags or-ed into `variant` (include/sdp.h): SDP_EXACT_STATE, SDP_WAVES(w)
struct VariantBits {
    int variant, waves;
    bool exact, et_bcast, ref;
    int flags;   // Params::flags: bit 0 SDP_NO_ZERO_SKIP, bit 1 SDP_NO_FILL
};
// The packed state keeps two 20-bit weights per cell (absolute error <= 2^-21 per weight, sdp_device.h "The packed state").  Its
// rounding error travels along an alignment path like a random walk (the 24-bit format of rounds 1-3 instead lost 1.7e-8 of
// E per step of a SATURATED path, 7.5e-5 at N = M = 2048: the 20-bit fields decode a saturated weight to exactly 1 and do
// not have that term); tests/test_parity_gpu.py::test_packed_state_at_the_longest_paths_it_serves holds max |dE| at
// N = M = 2048 (N + M = 4096, the longest problem the packed state serves) on soft, steep and peaked scores to half the
// 1e-4 bound.  Longer problems always use the exact (float2) state, whose largest weight is the complement of the other
// two (q_sharpen): <= 1e-5 at N = 60000.  sdp_state_bytes covers either layout; forward and backward apply the same rule.
constexpr int PACKED_MAX_PATH = 4096;
// Thin problems as well (round 5): with fewer than 32 rows (or columns) the rounding errors of the packed weights along the long
// axis do not average out over many paths -- flat scores, max |dE| by shape, packed (exact), tools/thin_probe.py / profiles/
// r05_thin.txt: 2 x 2048 1.0e-4 (4.5e-6), 4 x 2048 7.8e-5, 8 x 2048 6.1e-5, 16 x 1772 5.0e-5, 32 x 2048 3.6e-5, 64 x 2048 1.6e-5;
// any N x 512 <= 3.0e-5.  The soak of round 5 met 1.17e-4 at 2 x 1772 (positive gap scores).  Such problems are tiny: the exact state.
// Round 6: the same holds for a thin PAIR inside a fat padded batch with per-pair lengths (the reference's inference loop slices
// every pair and calls the decoder on the slice, alignment.py:165-170: each pair gets what a call of its own shape would get).
// The state format is a property of the kernel build, so such pairs are ROUTED: a launch with per-pair lengths whose padded shape
// admits thin long pairs (sdp::thin_pair: min(n, m) < 32 and max(n, m) > 512) runs the packed-state build with those pairs
// skipped (Params::route = 1) and, behind it, the exact-state build for those pairs only (route = 2; its workgroups of all other
// pairs leave at once).  The thin pair's float2 state lives inside the pair's own packed record: strip s starts where the packed
// strip s starts (st2_ps = st_ps) -- a wide thin pair has one strip and needs <= tpad x 512 B of the nstrips x tpad x 320 B, a tall
// thin one <= 3 units x 16 KB per strip of the tpad x 320 B a packed strip owns -- which fits as soon as the padded shape has more
// than 64 rows and more than 65 columns; padded shapes below that (and long) take the exact state as a whole, like thin problems.
inline bool exact_for(bool flag, int N, int M)
{
    const int lo = N < M ? N : M, hi = N < M ? M : N;
    return flag || N + M > PACKED_MAX_PATH || (lo < sdp::THIN_FITS && hi > sdp::THIN_HI);
}
// does a launch of this padded shape with per-pair lengths have to route thin pairs to the exact-state build?
inline bool routes_thin(bool exact, int N, int M, const int32_t *lens)
{
#ifdef SDP_EXPERIMENTS
    if (g_dbg.load() & 32768) return false;   // sdp_set_debug(32768): no routing (A/B timing of the second launch; thin pairs then keep the packed state)
#endif
    return lens != nullptr && !exact && (N > sdp::THIN_HI || M > sdp::THIN_HI);
}

// SDP_WAVES(w) cut out of `variant`: returns w, 0 where the caller gave none
int take_waves(int &variant)
{
    const int w = (variant >> 12) & 0xf;
    variant &= ~(0xf << 12);
    return w;
}

VariantBits split_variant(int variant)
{
    VariantBits v;
    v.exact = (variant & SDP_EXACT_STATE) != 0;
    v.et_bcast = (variant & SDP_ET_BROADCAST) != 0;
    v.waves = take_waves(variant);
    v.ref = (variant & SDP_REF_ROUNDING) != 0;
    v.flags = ((variant & SDP_NO_ZERO_SKIP) ? 1 : 0) | ((variant & SDP_NO_FILL) ? 2 : 0);
    v.variant = variant & ~(SDP_EXACT_STATE | SDP_ET_BROADCAST | SDP_REF_ROUNDING | SDP_NO_ZERO_SKIP | SDP_NO_FILL);
    return v;
}

// raise the dynamic-LDS limit once per (thread, device, kernel) -- it is sticky, and the value is the
// 160 KiB the hardware has, so concurrent callers cannot disagree
int raise_lds_limit(const Build &v, int device)
{
    static thread_local unsigned long long lds_raised[NBUILDS] = {0};  // per row of BUILDS: bit d = done on device d
    const int row = (int)(&v - BUILDS);
    if (device >= 64 || !(lds_raised[row] >> device & 1ull)) {
        hipError_t e = hipFuncSetAttribute((const void *)v.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return fail_hip(e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
        if (device < 64) lds_raised[row] |= 1ull << device;
    }
    return 0;
}

// what a launch is told beside the pass and the kernel parameters
struct LaunchOpts {
    StateKind st = ST_PACKED;
    int forced_waves = 0;          // SDP_WAVES(w) of the caller's `variant`, or 0: the policy's
    const void *state = nullptr;   // the WHOLE batch's state buffer, in whose tail the bridge rows and the dispatch map of a parts launch
                                   // live; null where there is none, or only part of one: the launch then keeps one workgroup per pair
    int route = 0;                 // Params::route
};

int launch(int pass, sdp::Params &p, int device, void *stream, const LaunchOpts &o)
{
    const void *state = o.state;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    if (int rc = pending_handoff_error(device)) return rc;
    p.nstrips_max = sdp::state_nstrips(p.N);
    p.tpad = sdp::state_tpad(p.M);
    p.mcap = (p.M + 63) / 64 * 64;
    state_layout(p);
    p.route = o.route;
    if (o.route == 2) {   // thin pairs only, exact-state build, inside the packed records (see exact_for): one workgroup per pair, batch order
        p.st2_ps = p.st_ps;
        p.order = nullptr;
        state = nullptr;
    }
    p.status = status_words(device);
#ifdef SDP_EXPERIMENTS
    p.dbg = g_dbg.load();
    p.trace = g_trace.load();
#else
    p.dbg = 0;
#endif
    // rows and planes of the staged tensors on 128-byte lines?  (M a multiple of 32 makes every plane offset b*N*M a
    // multiple of 32 floats too; the tensors themselves come from an allocator that aligns far beyond 128 bytes, but a
    // caller may pass a view)
    auto misaligned = [](const void *ptr) { return ptr != nullptr && ((uintptr_t)ptr & 127u) != 0; };
    const bool general_pitch = (p.M & 31) != 0 || misaligned(p.sin0) || misaligned(p.sin1) || misaligned(p.sin2) || misaligned(p.sout);
    int allow_parts = state != nullptr ? 1 : 0;
#ifdef SDP_EXPERIMENTS
    if (allow_parts && (g_dbg.load() & 512)) allow_parts = 2;   // sdp_set_debug(512): parts wherever they are possible (bit-identity test)
    if (g_dbg.load() & 64) allow_parts = 0;   // sdp_set_debug(64): one workgroup per pair whatever the shape (A/B timing, bit-identity test)
    if ((g_dbg.load() & 128) && pass == sdp::PASS_BWD) allow_parts = 0;   // (128: ... in the backward sweep only)
    if ((g_dbg.load() & 256) && pass == sdp::PASS_FWD) allow_parts = 0;   // (256: ... in the forward sweep only)
#endif
    const Plan pl = plan(pass, p.B, p.N, p.M, p.lens != nullptr, o.st, num_cus(device), o.forced_waves, general_pitch, allow_parts);
    const Build &v = *pl.v;
    const int W = pl.W;
    const size_t lds = pl.lds, off = pl.stage_off;
    p.stage_off = (int)off;
    if (int rc = raise_lds_limit(v, device)) return rc;
    unsigned grid = (unsigned)p.B;
    if (pl.parts) {
        p.parts = pl.parts;
        p.nparts_max = parts_per_pair(p.N);
        p.xb = bridge_in_state(state, p.B, p.N, p.M, o.st == ST_EXACT);
        p.xb_row = sdp::xb_row_granules(p.M);
        // every granule "not written yet" (tag 0x7f7f7f7f): enqueued on the caller's stream like the launch itself.  A
        // kernel of our own, not hipMemsetAsync: captured into a graph (torch.cuda.graph) the memset node did not take effect
        // before the sweep on replay -- consumers then took whatever the buffer held for granules (NaN results; tests/
        // test_robustness_gpu.py::test_sweeps_can_be_captured_in_a_graph).
        {
            const size_t n8 = bridge_bytes(p.B, p.N, p.M) / 8;
            const unsigned blocks = (unsigned)((n8 + 1023) / 1024 < 4096 ? (n8 + 1023) / 1024 : 4096);
            hipLaunchKernelGGL(sdp_bridge_reset_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p.xb, n8);
            e = hipGetLastError();
            if (e != hipSuccess) return fail_hip(e, "sdp_bridge_reset_kernel");
        }
        grid = (unsigned)p.B * (unsigned)p.nparts_max;
        p.order = nullptr;
        if (p.lens != nullptr) {
            int *map = reinterpret_cast<int *>(reinterpret_cast<char *>(p.xb) + bridge_bytes(p.B, p.N, p.M));
            hipLaunchKernelGGL(sdp_parts_map_kernel, dim3((grid + 3) / 4), dim3(256), 0, (hipStream_t)stream, p.lens, map, p.B, p.N, p.M,
                               p.nparts_max, pl.parts);
            e = hipGetLastError();
            if (e != hipSuccess) return fail_hip(e, "sdp_parts_map_kernel");
            p.wg_map = map;
        }
    }
    void *args[] = {&p};
    if (pl.parts) {
        // Two parts launches must not share the chip.  Within ONE launch a consumer can never keep its producer off a CU
        // (index order, see sdp_parts_map_kernel); with two launches on two streams the waiting parts of one could hold
        // the CUs the other's producers are queued for, and vice versa -- a deadlock that the bounded spins would turn
        // into SDP_E_HANDOFF and wrong results.  So every parts launch waits for the previous one on this device,
        // whatever stream that was on (an event per device; the lock keeps wait + launch + record of two host threads
        // apart).  Not during stream capture, where an event of uncaptured work may not be waited on: launches inside one
        // graph are ordered by the graph, and concurrent graphs that both hold parts launches are the caller's to order.
        static std::mutex mtx;
        static hipEvent_t last[64];
        static bool have[64] = {false};
        std::lock_guard<std::mutex> lock(mtx);
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        const bool track = device < 64 && hipStreamIsCapturing((hipStream_t)stream, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone;
        if (track && have[device]) {
            e = hipStreamWaitEvent((hipStream_t)stream, last[device], 0);
            if (e != hipSuccess) return fail_hip(e, "hipStreamWaitEvent(previous parts launch)");
        }
        e = hipLaunchKernel((const void *)v.kernel, dim3(grid), dim3(64 * W), args, lds, (hipStream_t)stream);
        if (e != hipSuccess) return fail_hip(e, "hipLaunchKernel");
        if (track) {
            if (!have[device]) {
                e = hipEventCreateWithFlags(&last[device], hipEventDisableTiming);
                if (e != hipSuccess) return fail_hip(e, "hipEventCreateWithFlags");
                have[device] = true;
            }
            e = hipEventRecord(last[device], (hipStream_t)stream);
            if (e != hipSuccess) return fail_hip(e, "hipEventRecord(parts launch)");
        }
        return 0;
    }
    e = hipLaunchKernel((const void *)v.kernel, dim3(grid), dim3(64 * W), args, lds, (hipStream_t)stream);
    if (e != hipSuccess) return fail_hip(e, "hipLaunchKernel");
    return 0;
}

// The forward or the backward sweep on a state: one launch, or two where thin long pairs are routed to the exact-state build (exact_for)
int launch_on_state(int pass, sdp::Params &p, int device, void *stream, bool exact, int forced_waves, const void *state)
{
    LaunchOpts o;
    o.st = exact ? ST_EXACT : ST_PACKED, o.forced_waves = forced_waves, o.state = state;
    if (!routes_thin(exact, p.N, p.M, p.lens)) return launch(pass, p, device, stream, o);
    o.route = 1;
    if (int rc = launch(pass, p, device, stream, o)) return rc;
    LaunchOpts thin;
    thin.st = ST_EXACT, thin.route = 2;
    return launch(pass, p, device, stream, thin);
}

// dynamic-LDS limits of the scores kernels, once per (thread, device): sticky attributes, set before any launch that
// may be captured (sdp_init) or lazily by the first call
int raise_scores_limits(int device)
{
    static thread_local unsigned long long raised = 0;
    if (device < 64 && (raised >> device & 1ull)) return 0;
    const struct { const void *f; int bytes; const char *what; } ks[] = {
        {(const void *)sdp_scores_kernel, sdp::SCORES_LDS_BYTES, "hipFuncSetAttribute(sdp_scores_kernel)"},
        {(const void *)sdp_scores_x6_kernel, sdp::SCORES_X6_LDS_BYTES, "hipFuncSetAttribute(sdp_scores_x6_kernel)"},
        {(const void *)sdp_scores_x6s_kernel, sdp::SCORES_X6_LDS_BYTES, "hipFuncSetAttribute(sdp_scores_x6s_kernel)"},
        {(const void *)sdp_scores_x6w_kernel, sdp::SCORES_X6W_LDS_BYTES, "hipFuncSetAttribute(sdp_scores_x6w_kernel)"},
        {(const void *)sdp_scores_bwd_x_kernel, sdp::SCORES_X6W_LDS_BYTES, "hipFuncSetAttribute(sdp_scores_bwd_x_kernel)"},
        {(const void *)sdp_scores_bwd_y_kernel, sdp::SCORES_X6W_LDS_BYTES, "hipFuncSetAttribute(sdp_scores_bwd_y_kernel)"},
        {(const void *)sdp_scores_bwd_yf_kernel, sdp::SCORES_X6W_LDS_BYTES, "hipFuncSetAttribute(sdp_scores_bwd_yf_kernel)"},
    };
    for (const auto &k : ks) {
        const hipError_t e = hipFuncSetAttribute(k.f, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes);
        if (e != hipSuccess) return fail_hip(e, k.what);
    }
    if (device < 64) raised |= 1ull << device;
    return 0;
}

// the same for strip-schedule kernels whose ring outgrows the 64 KB a kernel gets unasked: `bytes` for every kernel of `ks`, once
// per (thread, device) of the family that owns the mask `raised` -- by sdp_init, or lazily by the first call
struct LimitKernel {
    const void *f;
    const char *what;
};
int raise_strip_limits(unsigned long long &raised, int device, std::initializer_list<LimitKernel> ks, int bytes)
{
    if (device < 64 && (raised >> device & 1ull)) return 0;
    for (const LimitKernel &k : ks) {
        const hipError_t e = hipFuncSetAttribute(k.f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return fail_hip(e, k.what);
    }
    if (device < 64) raised |= 1ull << device;
    return 0;
}

// the soft local operator's adjoint backward sweep keeps two boundary rows per wave (sdp_soft_local::adjoint_lds_bytes): up to
// 2 x 64 KB
int raise_soft_local_adjoint_limit(int device)
{
    static thread_local unsigned long long raised = 0;
    return raise_strip_limits(raised, device, {{(const void *)sdp_soft_local_adj_bwd_kernel, "hipFuncSetAttribute(sdp_soft_local_adj_bwd_kernel)"}},
                              160 * 1024);
}

// the same for the sparsemax operator's adjoint backward sweep (sdp_sparsemax::adjoint_lds_bytes)
int raise_sparsemax_adjoint_limit(int device)
{
    static thread_local unsigned long long raised = 0;
    return raise_strip_limits(raised, device, {{(const void *)sdp_sparsemax_adj_bwd_kernel, "hipFuncSetAttribute(sdp_sparsemax_adj_bwd_kernel)"}},
                              160 * 1024);
}

// the affine-gap soft local operator's three kernels keep three boundary rows per wave (sdp_affine_local::sweep_lds_bytes): up to
// 160 KB, forward sweeps included
int raise_affine_local_limit(int device)
{
    static thread_local unsigned long long raised = 0;
    return raise_strip_limits(raised, device,
                              {{(const void *)sdp_affine_local_fwd_kernel, "hipFuncSetAttribute(sdp_affine_local_fwd_kernel)"},
                               {(const void *)sdp_affine_local_val_kernel, "hipFuncSetAttribute(sdp_affine_local_val_kernel)"},
                               {(const void *)sdp_affine_local_bwd_kernel, "hipFuncSetAttribute(sdp_affine_local_bwd_kernel)"}},
                              sdp_affine_local::LDS_BUDGET);
}

// its adjoint pair: the adjoint forward sweep keeps the first order's ring, the adjoint backward sweep twice that
// (sdp_affine_local::adjoint_lds_bytes), both up to 160 KB
int raise_affine_local_adjoint_limit(int device)
{
    static thread_local unsigned long long raised = 0;
    return raise_strip_limits(raised, device,
                              {{(const void *)sdp_affine_local_adj_fwd_kernel, "hipFuncSetAttribute(sdp_affine_local_adj_fwd_kernel)"},
                               {(const void *)sdp_affine_local_adj_bwd_kernel, "hipFuncSetAttribute(sdp_affine_local_adj_bwd_kernel)"}},
                              sdp_affine_local::LDS_BUDGET);
}

// the hard affine-gap local operator's sweeps keep three boundary rows per wave (sdp_hard_affine::sweep_lds_bytes), and its walk
// three planes of a strip's pointer lines (sdp_hard_affine::walk_lds_bytes): up to 160 KB and 99 KB
int raise_hard_affine_limit(int device)
{
    static thread_local unsigned long long raised = 0;
    return raise_strip_limits(raised, device,
                              {{(const void *)sdp_hard_affine_local_fwd_kernel, "hipFuncSetAttribute(sdp_hard_affine_local_fwd_kernel)"},
                               {(const void *)sdp_hard_affine_local_fwd_t_kernel, "hipFuncSetAttribute(sdp_hard_affine_local_fwd_t_kernel)"},
                               {(const void *)sdp_hard_affine_local_val_kernel, "hipFuncSetAttribute(sdp_hard_affine_local_val_kernel)"},
                               {(const void *)sdp_hard_affine_local_val_t_kernel, "hipFuncSetAttribute(sdp_hard_affine_local_val_t_kernel)"},
                               {(const void *)sdp_hard_affine_local_walk_kernel, "hipFuncSetAttribute(sdp_hard_affine_local_walk_kernel)"},
                               {(const void *)sdp_hard_affine_global_fwd_kernel, "hipFuncSetAttribute(sdp_hard_affine_global_fwd_kernel)"},
                               {(const void *)sdp_hard_affine_global_fwd_t_kernel, "hipFuncSetAttribute(sdp_hard_affine_global_fwd_t_kernel)"},
                               {(const void *)sdp_hard_affine_global_val_kernel, "hipFuncSetAttribute(sdp_hard_affine_global_val_kernel)"},
                               {(const void *)sdp_hard_affine_global_val_t_kernel, "hipFuncSetAttribute(sdp_hard_affine_global_val_t_kernel)"},
                               {(const void *)sdp_hard_affine_semiglobal_fwd_kernel, "hipFuncSetAttribute(sdp_hard_affine_semiglobal_fwd_kernel)"},
                               {(const void *)sdp_hard_affine_semiglobal_fwd_t_kernel, "hipFuncSetAttribute(sdp_hard_affine_semiglobal_fwd_t_kernel)"},
                               {(const void *)sdp_hard_affine_semiglobal_val_kernel, "hipFuncSetAttribute(sdp_hard_affine_semiglobal_val_kernel)"},
                               {(const void *)sdp_hard_affine_semiglobal_val_t_kernel, "hipFuncSetAttribute(sdp_hard_affine_semiglobal_val_t_kernel)"}},
                              sdp_hard_affine::LDS_BUDGET);
}

// the affine-gap soft global operator's three kernels keep four words per column and wave (sdp_affine_global::sweep_lds_bytes): up to
// 160 KB, forward sweeps included
int raise_affine_global_limit(int device)
{
    static thread_local unsigned long long raised = 0;
    return raise_strip_limits(raised, device,
                              {{(const void *)sdp_affine_global_fwd_kernel, "hipFuncSetAttribute(sdp_affine_global_fwd_kernel)"},
                               {(const void *)sdp_affine_global_val_kernel, "hipFuncSetAttribute(sdp_affine_global_val_kernel)"},
                               {(const void *)sdp_affine_global_bwd_kernel, "hipFuncSetAttribute(sdp_affine_global_bwd_kernel)"}},
                              sdp_affine_global::LDS_BUDGET);
}

// the family's free-end-gap member (csrc/sdp_affine_semiglobal.hip): the same ring, the same budget
int raise_affine_semiglobal_limit(int device)
{
    static thread_local unsigned long long raised = 0;
    return raise_strip_limits(raised, device,
                              {{(const void *)sdp_affine_semiglobal_fwd_kernel, "hipFuncSetAttribute(sdp_affine_semiglobal_fwd_kernel)"},
                               {(const void *)sdp_affine_semiglobal_val_kernel, "hipFuncSetAttribute(sdp_affine_semiglobal_val_kernel)"},
                               {(const void *)sdp_affine_semiglobal_bwd_kernel, "hipFuncSetAttribute(sdp_affine_semiglobal_bwd_kernel)"}},
                              sdp_affine_global::LDS_BUDGET);
}

// its adjoint pair: the adjoint forward sweep keeps the first order's ring, the adjoint backward sweep six words per column
// (sdp_affine_global::adjoint_lds_bytes), both up to 160 KB
int raise_affine_global_adjoint_limit(int device)
{
    static thread_local unsigned long long raised = 0;
    return raise_strip_limits(raised, device,
                              {{(const void *)sdp_affine_global_adj_fwd_kernel, "hipFuncSetAttribute(sdp_affine_global_adj_fwd_kernel)"},
                               {(const void *)sdp_affine_global_adj_bwd_kernel, "hipFuncSetAttribute(sdp_affine_global_adj_bwd_kernel)"}},
                              sdp_affine_global::LDS_BUDGET);
}

// ---- what the entries of the strip-schedule families share ----
// waves of a workgroup: one per strip in flight, lowered to `forced` if 0 < forced, then until the family's ring fits its budget
int strip_waves(int strips, int max_waves, int forced, int M, size_t (*lds_bytes)(int, int), int budget)
{
    int w = strips < max_waves ? strips : max_waves;
    if (forced > 0 && forced < w) w = forced;
    while (w > 1 && lds_bytes(w, M) > (size_t)budget) --w;
    return w;
}

// the checks of a family whose entries take `flags` and define none: any bit is refused
int flagless_args(const char *family, int B, int N, int M, int flags)
{
    if (int rc = check_shape(B, N, M, SDP_NW)) return rc;
    if (flags != 0) {
        snprintf(g_err, sizeof(g_err), "%s_*: this family defines no flags", family);
        return SDP_E_VARIANT;
    }
    if ((size_t)B * (size_t)N * (size_t)M > ((size_t)1 << 31)) return fail(SDP_E_TOOBIG, "B*N*M exceeds 2^31 elements");
    return 0;
}

int use_device(int device)
{
    const hipError_t e = hipSetDevice(device);
    return e == hipSuccess ? 0 : fail_hip(e, "hipSetDevice");
}

// one launch of `grid` workgroups of W waves with `lds` bytes of dynamic LDS; `name` is what a failure reports
template <typename Kernel, typename... Args>
int strip_launch(Kernel kernel, const char *name, unsigned grid, int W, size_t lds, void *stream, Args... args)
{
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * W), lds, (hipStream_t)stream, args...);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail_hip(e, name);
}

// variant | SDP_REF_ROUNDING (sdp_ref.hip): one workgroup of 256 threads per pair, three rolling anti-diagonals of float64
size_t ref_lds(int M) { return (size_t)3 * (M + 2) * sizeof(double); }
size_t ref_state_bytes(int B, int N, int M) { return (size_t)B * N * M * 3 * sizeof(float); }
int ref_prepare(int device)
{
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    return pending_handoff_error(device);
}
int ref_launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail_hip(e, what);
}

}  // namespace

extern "C" {

int sdp_version(void) { return SDP_VERSION; }

const char *sdp_last_error_string(void) { return g_err; }

int sdp_max_cols(void) { return sdp::MAX_COLS; }

size_t sdp_state_bytes(int B, int N, int M)
{
    if (B <= 0 || N <= 0 || M <= 0) return 0;
    // 2 x 20 bits per cell, five dwords per four cells (ten rows of 1024 B per 32 steps of a strip); + the launch order of a
    // variable-length batch, the bridge rows and the dispatch map of a parts launch.  Problems longer than PACKED_MAX_PATH, and
    // thin long ones, keep the exact state (see exact_for).
    if (exact_for(false, N, M)) return sdp_state_d_bytes(B, N, M);
    return packed_body_bytes(B, N, M) + sdp::state_order_bytes(B) + bridge_bytes(B, N, M) + parts_map_bytes(B, N);
}

size_t sdp_state_d_bytes(int B, int N, int M)
{
    if (B <= 0 || N <= 0 || M <= 0) return 0;
    return (size_t)B * sdp::state_rows2(N, M) * 64 * sizeof(float2) + sdp::state_order_bytes(B) + bridge_bytes(B, N, M) + parts_map_bytes(B, N);
}

size_t sdp_state_bytes_v(int B, int N, int M, int variant)
{
    if (B <= 0 || N <= 0 || M <= 0) return 0;
    if (variant & SDP_REF_ROUNDING) return ref_state_bytes(B, N, M);
    return (variant & SDP_EXACT_STATE) ? sdp_state_d_bytes(B, N, M) : sdp_state_bytes(B, N, M);
}

size_t sdp_state_d_bytes_v(int B, int N, int M, int variant)
{
    if (B <= 0 || N <= 0 || M <= 0) return 0;
    return (variant & SDP_REF_ROUNDING) ? ref_state_bytes(B, N, M) : sdp_state_d_bytes(B, N, M);
}

int sdp_plan(int pass, int B, int N, int M, int has_lens, int exact_state, int cus, int *kernel_id, int *chunk,
             int *waves, size_t *lds)
{
    const bool fused_seed = (pass & SDP_PLAN_FUSED_SEED) != 0, general_pitch = (pass & SDP_PLAN_GENERAL_PITCH) != 0;
    pass &= ~(SDP_PLAN_FUSED_SEED | SDP_PLAN_GENERAL_PITCH);
    if (pass < 0 || pass > sdp::PLAN_VALUE) return fail(SDP_E_VARIANT, "sdp_plan: pass must be 0..3, or 4 for the value-only forward sweep");
    if (fused_seed && pass != sdp::PASS_AFWD) return fail(SDP_E_VARIANT, "sdp_plan: SDP_PLAN_FUSED_SEED needs pass 2 (adjoint forward)");
    if (int rc = check_shape(B, N, M, SDP_NW)) return rc;
    if (cus <= 0) return fail(SDP_E_SHAPE, "sdp_plan: cus must be positive");
    const bool exact = (pass == sdp::PASS_FWD || pass == sdp::PASS_BWD) ? exact_for(exact_state != 0, N, M) : exact_state != 0;
    // (the value-only forward sweep, sdp_forward_value_f32, is the forward sweep with no state; exact_state does not apply to it)
    const StateKind st = pass == sdp::PLAN_VALUE ? ST_VALUE : fused_seed ? ST_SEED : exact ? ST_EXACT : ST_PACKED;
    const Plan pl = plan(pass == sdp::PLAN_VALUE ? sdp::PASS_FWD : pass, B, N, M, has_lens != 0, st, cus, 0, general_pitch);
    if (kernel_id) *kernel_id = pl.v->id;
    if (chunk) *chunk = pl.v->K;
    if (waves) *waves = pl.W;
    if (lds) *lds = pl.lds;
    return 0;
}

const char *sdp_kernel_name(int kernel_id)
{
    for (const Build &b : BUILDS)
        if (b.id == kernel_id) return b.name;
    switch (kernel_id) {   // the gap-gradient kernels (csrc/sdp_gap.hip): no builds of the sweep, no rows of the table
    case sdp_gap::ID_GAP: return "sdp_gap_kernel";
    case sdp_gap::ID_GAP2: return "sdp_gap2_kernel";
    case sdp_gap::ID_GAP_ROWS: return "sdp_gap_rows_kernel";
    case sdp_gap::ID_GAP2_ROWS: return "sdp_gap2_rows_kernel";
    case sdp_gap::ID_GAP_ROWS_F64: return "sdp_gap_rows_f64_kernel";
    case sdp_gap::ID_GAP2_ROWS_F64: return "sdp_gap2_rows_f64_kernel";
    // the local-alignment kernels of the hard-max family (csrc/sdp_hard.hip)
    case sdp_hard::ID_LOCAL_FWD: return "sdp_hard_local_fwd_kernel";
    case sdp_hard::ID_LOCAL_FWD_T: return "sdp_hard_local_fwd_t_kernel";
    case sdp_hard::ID_LOCAL_VAL: return "sdp_hard_local_val_kernel";
    case sdp_hard::ID_LOCAL_VAL_T: return "sdp_hard_local_val_t_kernel";
    case sdp_hard::ID_LOCAL_WALK: return "sdp_hard_local_walk_kernel";
    // the sampling kernels (csrc/sdp_sample.hip)
    case sdp_sample::ID_SAMPLE: return "sdp_sample_kernel";
    case sdp_sample::ID_SAMPLE_ROWS: return "sdp_sample_rows_kernel";
    case sdp_sample::ID_SAMPLE_ROWS_F64: return "sdp_sample_rows_f64_kernel";
    // the soft local operator (csrc/sdp_soft_local.hip)
    case sdp_soft_local::ID_FWD: return "sdp_soft_local_fwd_kernel";
    case sdp_soft_local::ID_VAL: return "sdp_soft_local_val_kernel";
    case sdp_soft_local::ID_BWD: return "sdp_soft_local_bwd_kernel";
    // its adjoint pair (csrc/sdp_soft_local_adj.hip)
    case sdp_soft_local::ID_ADJ_FWD: return "sdp_soft_local_adj_fwd_kernel";
    case sdp_soft_local::ID_ADJ_BWD: return "sdp_soft_local_adj_bwd_kernel";
    // sampling from its posterior (csrc/sdp_soft_local_sample.hip)
    case sdp_soft_local_sample::ID_TABLES: return "sdp_soft_local_tables_kernel";
    case sdp_soft_local_sample::ID_SAMPLE: return "sdp_soft_local_sample_kernel";
    // the sparsemax operator (csrc/sdp_sparsemax.hip)
    case sdp_sparsemax::ID_FWD: return "sdp_sparsemax_fwd_kernel";
    case sdp_sparsemax::ID_VAL: return "sdp_sparsemax_val_kernel";
    case sdp_sparsemax::ID_BWD: return "sdp_sparsemax_bwd_kernel";
    // its adjoint pair (csrc/sdp_sparsemax_adj.hip)
    case sdp_sparsemax::ID_ADJ_FWD: return "sdp_sparsemax_adj_fwd_kernel";
    case sdp_sparsemax::ID_ADJ_BWD: return "sdp_sparsemax_adj_bwd_kernel";
    // the affine-gap soft local operator (csrc/sdp_affine_local.hip)
    case sdp_affine_local::ID_FWD: return "sdp_affine_local_fwd_kernel";
    case sdp_affine_local::ID_VAL: return "sdp_affine_local_val_kernel";
    case sdp_affine_local::ID_BWD: return "sdp_affine_local_bwd_kernel";
    // its adjoint pair (csrc/sdp_affine_local_adj.hip)
    case sdp_affine_local::ID_ADJ_FWD: return "sdp_affine_local_adj_fwd_kernel";
    case sdp_affine_local::ID_ADJ_BWD: return "sdp_affine_local_adj_bwd_kernel";
    // sampling from its posterior (csrc/sdp_affine_local_sample.hip)
    case sdp_affine_local_sample::ID_TABLES: return "sdp_affine_local_tables_kernel";
    case sdp_affine_local_sample::ID_SAMPLE: return "sdp_affine_local_sample_kernel";
    // the hard affine-gap local operator (csrc/sdp_hard_affine.hip)
    case sdp_hard_affine::ID_FWD: return "sdp_hard_affine_local_fwd_kernel";
    case sdp_hard_affine::ID_FWD_T: return "sdp_hard_affine_local_fwd_t_kernel";
    case sdp_hard_affine::ID_VAL: return "sdp_hard_affine_local_val_kernel";
    case sdp_hard_affine::ID_VAL_T: return "sdp_hard_affine_local_val_t_kernel";
    case sdp_hard_affine::ID_WALK: return "sdp_hard_affine_local_walk_kernel";
    // its global member's sweeps (the same file; the walk is the local member's)
    case sdp_hard_affine::ID_GLOBAL_FWD: return "sdp_hard_affine_global_fwd_kernel";
    case sdp_hard_affine::ID_GLOBAL_FWD_T: return "sdp_hard_affine_global_fwd_t_kernel";
    case sdp_hard_affine::ID_GLOBAL_VAL: return "sdp_hard_affine_global_val_kernel";
    case sdp_hard_affine::ID_GLOBAL_VAL_T: return "sdp_hard_affine_global_val_t_kernel";
    // its semi-global member's sweeps (free end gaps)
    case sdp_hard_affine::ID_SEMIGLOBAL_FWD: return "sdp_hard_affine_semiglobal_fwd_kernel";
    case sdp_hard_affine::ID_SEMIGLOBAL_FWD_T: return "sdp_hard_affine_semiglobal_fwd_t_kernel";
    case sdp_hard_affine::ID_SEMIGLOBAL_VAL: return "sdp_hard_affine_semiglobal_val_kernel";
    case sdp_hard_affine::ID_SEMIGLOBAL_VAL_T: return "sdp_hard_affine_semiglobal_val_t_kernel";
    // the affine-gap soft global operator (csrc/sdp_affine_global.hip)
    case sdp_affine_global::ID_FWD: return "sdp_affine_global_fwd_kernel";
    case sdp_affine_global::ID_VAL: return "sdp_affine_global_val_kernel";
    case sdp_affine_global::ID_BWD: return "sdp_affine_global_bwd_kernel";
    // sampling from its posterior (csrc/sdp_affine_global_sample.hip)
    case sdp_affine_global_sample::ID_SAMPLE: return "sdp_affine_global_sample_kernel";
    // the affine-gap soft global operator's adjoint pair (csrc/sdp_affine_global_adj.hip)
    case sdp_affine_global::ID_ADJ_FWD: return "sdp_affine_global_adj_fwd_kernel";
    case sdp_affine_global::ID_ADJ_BWD: return "sdp_affine_global_adj_bwd_kernel";
    // the affine-gap soft semi-global operator: free end gaps (csrc/sdp_affine_semiglobal.hip)
    case sdp_affine_global::ID_SEMI_FWD: return "sdp_affine_semiglobal_fwd_kernel";
    case sdp_affine_global::ID_SEMI_VAL: return "sdp_affine_semiglobal_val_kernel";
    case sdp_affine_global::ID_SEMI_BWD: return "sdp_affine_semiglobal_bwd_kernel";
    // sampling from its posterior (csrc/sdp_affine_semiglobal_sample.hip)
    case sdp_affine_semiglobal_sample::ID_END_TABLE: return "sdp_affine_semiglobal_end_table_kernel";
    case sdp_affine_semiglobal_sample::ID_SAMPLE: return "sdp_affine_semiglobal_sample_kernel";
    }
    return nullptr;
}

int sdp_plan_parts(int pass, int B, int N, int M, int has_lens, int exact_state, int cus)
{
    if (pass < 0 || pass > 3 || check_shape(B, N, M, SDP_NW) || cus <= 0) return 0;
    const bool exact = (pass == sdp::PASS_FWD || pass == sdp::PASS_BWD) ? exact_for(exact_state != 0, N, M) : exact_state != 0;
    return plan(pass, B, N, M, has_lens != 0, exact ? ST_EXACT : ST_PACKED, cus, 0).parts;
}

int sdp_init(int device)
{
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    if (device >= 0 && device < MAX_DEV && !status_words(device)) return fail(SDP_E_SELFTEST, "sdp_init: could not create the host-pinned status words");
    for (const Build &b : BUILDS)
        if (int rc = raise_lds_limit(b, device)) return rc;
    if (int rc = raise_scores_limits(device)) return rc;
    if (int rc = raise_soft_local_adjoint_limit(device)) return rc;
    if (int rc = raise_sparsemax_adjoint_limit(device)) return rc;
    if (int rc = raise_affine_local_limit(device)) return rc;
    if (int rc = raise_affine_local_adjoint_limit(device)) return rc;
    if (int rc = raise_hard_affine_limit(device)) return rc;
    if (int rc = raise_affine_global_limit(device)) return rc;
    if (int rc = raise_affine_semiglobal_limit(device)) return rc;
    return raise_affine_global_adjoint_limit(device);
}

int sdp_device_status(int device, int32_t info[4])
{
    const volatile int *h = (device >= 0 && device < MAX_DEV) ? g_status_host[device].load(std::memory_order_acquire) : nullptr;
    if (!h) {
        if (info) info[0] = info[1] = info[2] = info[3] = 0;
        return 0;
    }
    if (info) info[0] = h[0], info[1] = h[1], info[2] = h[2], info[3] = h[3];
    return pending_handoff_error(device);
}

#ifdef SDP_EXPERIMENTS
int sdp_set_debug(int mask)
{
    return g_dbg.exchange(mask);
}
// device buffer (>= 4 pairs x 4 waves x 4 strip rounds or parts x 40 blocks x 8 stamps x 8 B = 160 KiB) that the forward sweep of pairs
// 0, 64, 128, 192 fills with shader-cycle stamps per 16-step block; null = off
int sdp_set_trace(void *buf)
{
    g_trace.store(static_cast<unsigned long long *>(buf));
    return 0;
}
#endif

int sdp_forward_f32(const float *theta, const float *A, float *state, float *Vt, int B, int N, int M,
                    const int32_t *lens, int variant, int device, void *stream)
{
    if (!theta || !A || !state || !Vt) return fail(SDP_E_NULLPTR, "sdp_forward_f32: null pointer");
    const VariantBits vb = split_variant(variant);
    const bool exact = exact_for(vb.exact, N, M);
    variant = vb.variant;
    if (int rc = check_shape(B, N, M, variant)) return rc;
    if (vb.ref) {
        if (int rc = ref_prepare(device)) return rc;
        hipLaunchKernelGGL(sdp_ref_fwd_kernel, dim3(B), dim3(256), ref_lds(M), (hipStream_t)stream, theta, A, state, Vt, lens, N, M, variant == SDP_SW);
        return ref_launched("sdp_ref_fwd_kernel");
    }
    sdp::Params p = {};
    p.sin0 = theta;
    p.sin1 = A;
    p.dout = state;
    p.vout = Vt;
    p.lens = lens;
    p.B = B, p.N = N, p.M = M, p.variant = variant, p.flags = vb.flags;
    if (wants_order(B, N, lens, device)) {
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
        int *order = const_cast<int *>(order_in_state(state, B, N, M, exact));
        hipLaunchKernelGGL(sdp_order_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, lens, order, B, N, M);
        e = hipGetLastError();
        if (e != hipSuccess) return fail_hip(e, "sdp_order_kernel");
        if (B > num_cus(device)) p.order = order;   // (with parts the launch takes it from the state by itself)
    }
    return launch_on_state(sdp::PASS_FWD, p, device, stream, exact, vb.waves, state);
}

size_t sdp_forward_value_ws_bytes(int B, int N, int M)
{
    if (B <= 0 || N <= 0 || M <= 0 || M > sdp::MAX_COLS) return 0;
    return sdp::state_order_bytes(B);   // the launch order of a variable-length batch with more pairs than CUs: B ints
}

int sdp_forward_value_f32(const float *theta, const float *A, float *Vt, void *ws, int B, int N, int M, const int32_t *lens,
                          int variant, int device, void *stream)
{
    if (!theta || !A || !Vt) return fail(SDP_E_NULLPTR, "sdp_forward_value_f32: null pointer");
    if (variant & (SDP_EXACT_STATE | SDP_REF_ROUNDING | SDP_ET_BROADCAST | SDP_NO_FILL))
        return fail(SDP_E_VARIANT, "sdp_forward_value_f32: SDP_EXACT_STATE, SDP_REF_ROUNDING, SDP_ET_BROADCAST and SDP_NO_FILL do not apply to a sweep "
                                   "that writes no state and no E (SDP_NW / SDP_SW | SDP_WAVES(w) only)");
    const VariantBits vb = split_variant(variant);
    variant = vb.variant;
    if (int rc = check_shape(B, N, M, variant)) return rc;
    if (lens != nullptr && ws == nullptr && sdp_forward_value_ws_bytes(B, N, M) != 0)
        return fail(SDP_E_NULLPTR, "sdp_forward_value_f32: per-pair lengths need a workspace of sdp_forward_value_ws_bytes(B, N, M) bytes");
    sdp::Params p = {};
    p.sin0 = theta;
    p.sin1 = A;
    p.vout = Vt;
    p.lens = lens;
    p.B = B, p.N = N, p.M = M, p.variant = variant;
    if (wants_order(B, N, lens, device)) {   // longest first, as in the forward sweep; the order lives in the workspace
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
        int *order = static_cast<int *>(ws);
        hipLaunchKernelGGL(sdp_order_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, lens, order, B, N, M);
        e = hipGetLastError();
        if (e != hipSuccess) return fail_hip(e, "sdp_order_kernel");
        p.order = order;
    }
    LaunchOpts o;
    o.st = ST_VALUE, o.forced_waves = vb.waves;
    return launch(sdp::PASS_FWD, p, device, stream, o);
}

int sdp_backward_f32(const float *Et, const float *state, float *E, int B, int N, int M, const int32_t *lens,
                     int variant, int device, void *stream)
{
    if (!Et || !state || !E) return fail(SDP_E_NULLPTR, "sdp_backward_f32: null pointer");
    const VariantBits vb = split_variant(variant);
    const bool exact = exact_for(vb.exact, N, M);
    variant = vb.variant;
    if (int rc = check_shape(B, N, M, variant)) return rc;
    if (vb.ref) {
        if (int rc = ref_prepare(device)) return rc;
        hipLaunchKernelGGL(sdp_ref_bwd_kernel, dim3(B), dim3(256), ref_lds(M), (hipStream_t)stream, Et, state, E, lens, N, M, variant == SDP_SW, vb.et_bcast ? 1 : 0);
        return ref_launched("sdp_ref_bwd_kernel");
    }
    sdp::Params p = {};
    p.vin = Et;
    p.vin_bcast = vb.et_bcast ? 1 : 0;
    p.qin = reinterpret_cast<const uint32_t *>(state);
    p.sout = E;
    p.lens = lens;
    p.B = B, p.N = N, p.M = M, p.variant = variant, p.flags = vb.flags;
    if (lens != nullptr && B > num_cus(device)) p.order = order_in_state(state, B, N, M, exact);
    return launch_on_state(sdp::PASS_BWD, p, device, stream, exact, vb.waves, state);
}

size_t sdp_state_pair_stride(int N, int M, int exact_state)
{
    if (N <= 0 || M <= 0) return 0;
    // the body of the state buffer is B equal records, one per pair: nstrips streams of tpad / 32 units
    // (state_layout); order, bridge rows and dispatch map live behind the LAST pair's record, not between records
    const size_t units = (size_t)sdp::state_nstrips(N) * (sdp::state_tpad(M) / sdp::STATE_UNIT_STEPS);
    return units * (exact_for(exact_state != 0, N, M) ? sdp::STATE2_UNIT_BYTES : sdp::STATEQ_UNIT_BYTES);
}

int sdp_backward_range_f32(const float *Et, const float *state, float *E, int B, int N, int M, int first, int count,
                           int variant, int device, void *stream)
{
    if (!Et || !state || !E) return fail(SDP_E_NULLPTR, "sdp_backward_range_f32: null pointer");
    const VariantBits vb = split_variant(variant);
    const bool exact = exact_for(vb.exact, N, M);
    variant = vb.variant;
    if (int rc = check_shape(B, N, M, variant)) return rc;
    if (first < 0 || count <= 0 || first > B - count) return fail(SDP_E_SHAPE, "sdp_backward_range_f32: [first, first + count) is not inside the batch");
    if (vb.ref) {
        if (int rc = ref_prepare(device)) return rc;
        const size_t plane = (size_t)N * M;
        hipLaunchKernelGGL(sdp_ref_bwd_kernel, dim3(count), dim3(256), ref_lds(M), (hipStream_t)stream, vb.et_bcast ? Et : Et + first,
                           state + (size_t)first * plane * 3, E + (size_t)first * plane, (const int *)nullptr, N, M, variant == SDP_SW, vb.et_bcast ? 1 : 0);
        return ref_launched("sdp_ref_bwd_kernel");
    }
    sdp::Params p = {};
    p.vin = vb.et_bcast ? Et : Et + first;
    p.vin_bcast = vb.et_bcast ? 1 : 0;
    p.qin = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(state) + (size_t)first * sdp_state_pair_stride(N, M, exact));
    p.sout = E + (size_t)first * N * M;
    p.B = count, p.N = N, p.M = M, p.variant = variant, p.flags = vb.flags;
    // state = nullptr: a launch over part of the batch never spreads pairs over several workgroups -- the bridge rows
    // live behind the record of the batch's LAST pair, and located from a sub-range they would fall into the records of
    // the pairs that follow it
    LaunchOpts o;
    o.st = exact ? ST_EXACT : ST_PACKED, o.forced_waves = vb.waves;
    return launch(sdp::PASS_BWD, p, device, stream, o);
}

int sdp_adjoint_forward_f32(const float *state, const float *Ztheta, const float *ZA, float *Vtd, float *state_d,
                            int B, int N, int M, const int32_t *lens, int variant, int device, void *stream)
{
    if (!state || !Ztheta || !Vtd || !state_d) return fail(SDP_E_NULLPTR, "sdp_adjoint_forward_f32: null pointer");
    const VariantBits vb = split_variant(variant);
    variant = vb.variant;
    if (int rc = check_shape(B, N, M, variant)) return rc;
    if (vb.ref) {
        if (int rc = ref_prepare(device)) return rc;
        hipLaunchKernelGGL(sdp_ref_adj_fwd_kernel, dim3(B), dim3(256), ref_lds(M), (hipStream_t)stream, state, Ztheta, ZA, Vtd, state_d, lens, N, M);
        return ref_launched("sdp_ref_adj_fwd_kernel");
    }
    sdp::Params p = {};
    p.qin = reinterpret_cast<const uint32_t *>(state);
    p.sin0 = Ztheta;
    p.sin1 = ZA;
    p.dout = state_d;
    p.vout = Vtd;
    p.lens = lens;
    p.B = B, p.N = N, p.M = M, p.variant = variant, p.flags = vb.flags;
    if (lens != nullptr && B > num_cus(device)) p.order = order_in_state(state, B, N, M, true);
    LaunchOpts o;
    o.forced_waves = vb.waves;
    return launch(sdp::PASS_AFWD, p, device, stream, o);
}

int sdp_adjoint_forward_loss_f32(const float *state, const float *ref, const float *pred, const float *G, const float *scale,
                                 int kind, float *Vtd, float *state_d, int B, int N, int M, const int32_t *lens, int variant,
                                 int device, void *stream)
{
    if (!state || !ref || !pred || !G || !scale || !Vtd || !state_d)
        return fail(SDP_E_NULLPTR, "sdp_adjoint_forward_loss_f32: null pointer");
    if (kind < 0 || kind > 2) return fail(SDP_E_VARIANT, "loss kind must be 0 (cross entropy), 1 (path) or 2 (alignment)");
    const VariantBits vb = split_variant(variant);
    variant = vb.variant;
    if (vb.ref) return fail(SDP_E_VARIANT, "sdp_adjoint_forward_loss_f32: the fused loss seed has no reference-rounding form (use sdp_loss_backward_f32 + sdp_adjoint_forward_f32)");
    if (int rc = check_shape(B, N, M, variant)) return rc;
    sdp::Params p = {};
    p.qin = reinterpret_cast<const uint32_t *>(state);
    p.sin0 = ref;
    p.sin1 = pred;
    p.sin2 = G;
    p.vin = scale;
    p.loss_kind = kind;
    p.dout = state_d;
    p.vout = Vtd;
    p.lens = lens;
    p.B = B, p.N = N, p.M = M, p.variant = variant, p.flags = vb.flags;
    if (lens != nullptr && B > num_cus(device)) p.order = order_in_state(state, B, N, M, true);
    LaunchOpts o;
    o.st = ST_SEED, o.forced_waves = vb.waves;
    return launch(sdp::PASS_AFWD, p, device, stream, o);
}

int sdp_adjoint_backward_f32(const float *E, const float *state, const float *state_d, float *Ed, int B, int N,
                             int M, const int32_t *lens, int variant, int device, void *stream)
{
    if (!E || !state || !state_d || !Ed) return fail(SDP_E_NULLPTR, "sdp_adjoint_backward_f32: null pointer");
    const VariantBits vb = split_variant(variant);
    variant = vb.variant;
    if (int rc = check_shape(B, N, M, variant)) return rc;
    if (vb.ref) {
        if (int rc = ref_prepare(device)) return rc;
        hipLaunchKernelGGL(sdp_ref_adj_bwd_kernel, dim3(B), dim3(256), ref_lds(M), (hipStream_t)stream, E, state, state_d, Ed, lens, N, M);
        return ref_launched("sdp_ref_adj_bwd_kernel");
    }
    sdp::Params p = {};
    p.sin0 = E;
    p.qin = reinterpret_cast<const uint32_t *>(state);
    p.din = reinterpret_cast<const float2 *>(state_d);
    p.sout = Ed;
    p.lens = lens;
    p.B = B, p.N = N, p.M = M, p.variant = variant, p.flags = vb.flags;
    if (lens != nullptr && B > num_cus(device)) p.order = order_in_state(state, B, N, M, true);
    LaunchOpts o;
    o.forced_waves = vb.waves;
    return launch(sdp::PASS_ABWD, p, device, stream, o);
}

// ---- float64 tensors (sdp.h): the reference-arithmetic kernels of sdp_ref.hip with float64 storage ----
size_t sdp_state_bytes_f64(int B, int N, int M)
{
    if (B <= 0 || N <= 0 || M <= 0) return 0;
    return (size_t)B * N * M * 3 * sizeof(double);
}

static int f64_variant(int variant, const char *who, bool &et_bcast)
{
    et_bcast = (variant & SDP_ET_BROADCAST) != 0;
    const int v = variant & ~SDP_ET_BROADCAST;
    if (v != SDP_NW && v != SDP_SW) {
        snprintf(g_err, sizeof(g_err), "%s: variant must be SDP_NW or SDP_SW (float64 tensors take no state / rounding / wave flags)", who);
        return -1;
    }
    return v;
}

int sdp_forward_f64(const double *theta, const double *A, double *state, double *Vt, int B, int N, int M,
                    const int32_t *lens, int variant, int device, void *stream)
{
    if (!theta || !A || !state || !Vt) return fail(SDP_E_NULLPTR, "sdp_forward_f64: null pointer");
    bool bc;
    const int v = f64_variant(variant, "sdp_forward_f64", bc);
    if (v < 0 || bc) return v < 0 ? SDP_E_VARIANT : fail(SDP_E_VARIANT, "sdp_forward_f64: SDP_ET_BROADCAST belongs to the backward sweep");
    if (int rc = check_shape(B, N, M, v)) return rc;
    if (int rc = ref_prepare(device)) return rc;
    hipLaunchKernelGGL(sdp_f64_fwd_kernel, dim3(B), dim3(256), ref_lds(M), (hipStream_t)stream, theta, A, state, Vt, lens, N, M, v == SDP_SW);
    return ref_launched("sdp_f64_fwd_kernel");
}

int sdp_backward_f64(const double *Et, const double *state, double *E, int B, int N, int M,
                     const int32_t *lens, int variant, int device, void *stream)
{
    if (!Et || !state || !E) return fail(SDP_E_NULLPTR, "sdp_backward_f64: null pointer");
    bool bc;
    const int v = f64_variant(variant, "sdp_backward_f64", bc);
    if (v < 0) return SDP_E_VARIANT;
    if (int rc = check_shape(B, N, M, v)) return rc;
    if (int rc = ref_prepare(device)) return rc;
    hipLaunchKernelGGL(sdp_f64_bwd_kernel, dim3(B), dim3(256), ref_lds(M), (hipStream_t)stream, Et, state, E, lens, N, M, v == SDP_SW, bc ? 1 : 0);
    return ref_launched("sdp_f64_bwd_kernel");
}

int sdp_adjoint_forward_f64(const double *state, const double *Ztheta, const double *ZA, double *Vtd, double *state_d,
                            int B, int N, int M, const int32_t *lens, int variant, int device, void *stream)
{
    if (!state || !Ztheta || !Vtd || !state_d) return fail(SDP_E_NULLPTR, "sdp_adjoint_forward_f64: null pointer");
    bool bc;
    const int v = f64_variant(variant, "sdp_adjoint_forward_f64", bc);
    if (v < 0 || bc) return v < 0 ? SDP_E_VARIANT : fail(SDP_E_VARIANT, "sdp_adjoint_forward_f64: SDP_ET_BROADCAST belongs to the backward sweep");
    if (int rc = check_shape(B, N, M, v)) return rc;
    if (int rc = ref_prepare(device)) return rc;
    hipLaunchKernelGGL(sdp_f64_adj_fwd_kernel, dim3(B), dim3(256), ref_lds(M), (hipStream_t)stream, state, Ztheta, ZA, Vtd, state_d, lens, N, M);
    return ref_launched("sdp_f64_adj_fwd_kernel");
}

int sdp_adjoint_backward_f64(const double *E, const double *state, const double *state_d, double *Ed,
                             int B, int N, int M, const int32_t *lens, int variant, int device, void *stream)
{
    if (!E || !state || !state_d || !Ed) return fail(SDP_E_NULLPTR, "sdp_adjoint_backward_f64: null pointer");
    bool bc;
    const int v = f64_variant(variant, "sdp_adjoint_backward_f64", bc);
    if (v < 0 || bc) return v < 0 ? SDP_E_VARIANT : fail(SDP_E_VARIANT, "sdp_adjoint_backward_f64: SDP_ET_BROADCAST belongs to the backward sweep");
    if (int rc = check_shape(B, N, M, v)) return rc;
    if (int rc = ref_prepare(device)) return rc;
    hipLaunchKernelGGL(sdp_f64_adj_bwd_kernel, dim3(B), dim3(256), ref_lds(M), (hipStream_t)stream, E, state, state_d, Ed, lens, N, M);
    return ref_launched("sdp_f64_adj_bwd_kernel");
}

static bool scores_force_f32()
{
#ifdef SDP_EXPERIMENTS
    return (g_dbg.load() & 16) != 0;   // sdp_set_debug(16): the f32-input MFMA kernel for every shape (A/B timing, parity)
#else
    return false;
#endif
}

static bool scores_force_narrow()
{
#ifdef SDP_EXPERIMENTS
    return (g_dbg.load() & 32) != 0;   // sdp_set_debug(32): the 128 x 128 tiles for every shape (A/B timing, bit-identity test)
#else
    return false;
#endif
}
bool scores_unfused()
{
#ifdef SDP_EXPERIMENTS
    return (g_dbg.load() & 2048) != 0;   // sdp_set_debug(2048): backward of the scores with dS in a pass of its own (A/B timing, parity)
#else
    return false;
#endif
}

int sdp_scores_f32(const float *zx, const float *zy, const float *gx, const float *gy, float *theta, float *A, int B, int N,
                   int M, int D, int device, void *stream)
{
    if (!zx || !zy || !theta) return fail(SDP_E_NULLPTR, "sdp_scores_f32: null pointer");
    if ((gx || gy || A) && !(gx && gy && A)) return fail(SDP_E_NULLPTR, "sdp_scores_f32: gx, gy and A go together (all or none)");
    if (B <= 0 || N <= 0 || M <= 0 || D <= 0) return fail(SDP_E_SHAPE, "B, N, M and D must be positive");
    if ((size_t)N * M > ((size_t)1 << 28) || (size_t)N * D > ((size_t)1 << 28) || (size_t)M * D > ((size_t)1 << 28))
        return fail(SDP_E_TOOBIG, "a matrix of one pair exceeds 2^28 elements");
    const long long nz = (long long)(A ? 2 : 1) * B;
    if (nz > 65535) return fail(SDP_E_TOOBIG, "too many pairs for one launch (grid.z)");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    if (int rc = raise_scores_limits(device)) return rc;
    // whole 16-deep slabs of 16-byte aligned rows: the three-piece bf16 product (sdp_scores.hip); anything else: the
    // f32-input MFMA kernel, which takes ragged D and unaligned rows
    auto aligned16 = [](const void *q) { return q == nullptr || (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    const bool x6 = D % 16 == 0 && aligned16(zx) && aligned16(zy) && aligned16(gx) && aligned16(gy) && !scores_force_f32();
    const dim3 grid((M + 127) / 128, (N + 127) / 128, (unsigned)nz);
    // 256 x 256 tiles (8 waves, half the cuts and LDS traffic per MFMA) when they do not waste more than a quarter more
    // of the matrix pipe on rows and columns outside the matrices than the 128 x 128 tiles do, and when there are at
    // least two of them per CU (one workgroup per CU: a batch of few large tiles leaves CUs idle -- 3 x 1000 x 701:
    // 129 us against 85 us with the small tiles)
    const long long t128 = (long long)grid.x * grid.y, t256 = (long long)((M + 255) / 256) * ((N + 255) / 256) * 4;
    const bool wide = x6 && !scores_force_narrow() && 4 * t256 <= 5 * t128 && (t256 / 4) * nz >= 2LL * num_cus(device);
    if (wide)
        hipLaunchKernelGGL(sdp_scores_x6w_kernel, dim3((M + 255) / 256, (N + 255) / 256, (unsigned)nz), dim3(512), sdp::SCORES_X6W_LDS_BYTES,
                           (hipStream_t)stream, zx, zy, gx, gy, theta, A, B, N, M, D);
    else if (x6 && t128 * nz <= 2LL * num_cus(device))   // (no CU ever holds a third tile: the build with two workgroups' worth of registers, no scratch)
        hipLaunchKernelGGL(sdp_scores_x6s_kernel, grid, dim3(256), sdp::SCORES_X6_LDS_BYTES, (hipStream_t)stream, zx, zy, gx, gy, theta, A, B, N, M, D);
    else if (x6)
        hipLaunchKernelGGL(sdp_scores_x6_kernel, grid, dim3(256), sdp::SCORES_X6_LDS_BYTES, (hipStream_t)stream, zx, zy, gx, gy, theta, A, B, N, M, D);
    else
        hipLaunchKernelGGL(sdp_scores_kernel, grid, dim3(256), sdp::SCORES_LDS_BYTES, (hipStream_t)stream, zx, zy, gx, gy, theta, A, B, N, M, D);
    e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, x6 ? "sdp_scores_x6_kernel" : "sdp_scores_kernel");
    return 0;
}

size_t sdp_scores_backward_ws_bytes(int B, int N, int M)
{
    if (B <= 0 || N <= 0 || M <= 0) return 0;
    return (size_t)2 * B * N * M * sizeof(float);   // dS of theta, dS of A
}

int sdp_scores_backward_f32(const float *g_theta, const float *g_A, const float *theta, const float *A, const float *zx,
                            const float *zy, const float *gx, const float *gy, float *ws, float *dzx, float *dzy, float *dgx,
                            float *dgy, int B, int N, int M, int D, int device, void *stream)
{
    const bool has_t = g_theta != nullptr, has_a = g_A != nullptr;
    if (!has_t && !has_a) return fail(SDP_E_NULLPTR, "sdp_scores_backward_f32: neither g_theta nor g_A");
    if (!ws || (has_t && !(theta && zx && zy && dzx && dzy)) || (has_a && !(A && gx && gy && dgx && dgy)))
        return fail(SDP_E_NULLPTR, "sdp_scores_backward_f32: null pointer");
    if (B <= 0 || N <= 0 || M <= 0 || D <= 0) return fail(SDP_E_SHAPE, "B, N, M and D must be positive");
    if ((size_t)N * M > ((size_t)1 << 28) || (size_t)N * D > ((size_t)1 << 28) || (size_t)M * D > ((size_t)1 << 28))
        return fail(SDP_E_TOOBIG, "a matrix of one pair exceeds 2^28 elements");
    auto aligned16 = [](const void *q) { return q == nullptr || (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if (M % 4 != 0 || D % 4 != 0 || !(aligned16(g_theta) && aligned16(g_A) && aligned16(theta) && aligned16(A) && aligned16(zx) && aligned16(zy) &&
                                      aligned16(gx) && aligned16(gy) && aligned16(ws) && aligned16(dzx) && aligned16(dzy) && aligned16(dgx) && aligned16(dgy)))
        return fail(SDP_E_SHAPE, "sdp_scores_backward_f32 needs M and D multiples of 4 and 16-byte aligned tensors");
    const long long nz = (long long)(has_t && has_a ? 2 : 1) * B;
    if (nz > 65535) return fail(SDP_E_TOOBIG, "too many pairs for one launch (grid.z)");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    if (int rc = raise_scores_limits(device)) return rc;
    const size_t plane = (size_t)B * N * M;
    float *ds_t = ws, *ds_a = ws + plane;
    // tensor 0 / 1 of a launch: theta's operands first when both are asked for
    const float *d0 = has_t ? ds_t : ds_a, *d1 = ds_a;
    const float *y0 = has_t ? zy : gy, *y1 = gy, *x0 = has_t ? zx : gx, *x1 = gx;
    float *cx0 = has_t ? dzx : dgx, *cx1 = dgx, *cy0 = has_t ? dzy : dgy, *cy1 = dgy;
    const dim3 grid_y((D + 255) / 256, (M + 255) / 256, (unsigned)nz), grid_x((D + 255) / 256, (N + 255) / 256, (unsigned)nz);
    if (scores_unfused()) {
        // (experiments build, sdp_set_debug(2048): dS in a pass of its own, then the plain product -- what the fused kernel replaced)
        hipLaunchKernelGGL(sdp_scores_ds_kernel, dim3(num_cus(device) * 8), dim3(256), 0, (hipStream_t)stream, g_theta, g_A, theta, A, ds_t, ds_a, plane / 4);
        e = hipGetLastError();
        if (e != hipSuccess) return fail_hip(e, "sdp_scores_ds_kernel");
        hipLaunchKernelGGL(sdp_scores_bwd_y_kernel, grid_y, dim3(512), sdp::SCORES_X6W_LDS_BYTES, (hipStream_t)stream, d0, d1, x0, x1, cy0, cy1, B, N, M, D);
        e = hipGetLastError();
        if (e != hipSuccess) return fail_hip(e, "sdp_scores_bwd_y_kernel");
    } else {
        // dzy / dgy first: this product reads (g, act) and forms dS on the way into LDS; its first column of tiles writes dS
        // to `ws` for the other product, which follows on the same stream
        const float *g0 = has_t ? g_theta : g_A, *g1 = g_A, *a0 = has_t ? theta : A, *a1 = A;
        const float sg0 = has_t ? -1.0f : 1.0f, sg1 = 1.0f;
        float *w0 = has_t ? ds_t : ds_a, *w1 = ds_a;
        hipLaunchKernelGGL(sdp_scores_bwd_yf_kernel, grid_y, dim3(512), sdp::SCORES_X6W_LDS_BYTES, (hipStream_t)stream, g0, g1, a0, a1, sg0, sg1, x0, x1, w0, w1,
                           cy0, cy1, B, N, M, D);
        e = hipGetLastError();
        if (e != hipSuccess) return fail_hip(e, "sdp_scores_bwd_yf_kernel");
    }
    hipLaunchKernelGGL(sdp_scores_bwd_x_kernel, grid_x, dim3(512), sdp::SCORES_X6W_LDS_BYTES, (hipStream_t)stream, d0, d1, y0, y1, cx0, cx1, B, N, M, D);
    e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "sdp_scores_bwd_x_kernel");
    return 0;
}

int sdp_traceback_capacity(int N, int M) { return (N > 0 && M > 0) ? N + M + 2 : 0; }

int sdp_traceback_rule_i32(const float *grad, int32_t *states, int32_t *counts, int B, int N, int M, const int32_t *lens,
                           int rule, int device, void *stream)
{
    if (!grad || !states || !counts) return fail(SDP_E_NULLPTR, "sdp_traceback_i32: null pointer");
    if (B <= 0 || N <= 0 || M <= 0) return fail(SDP_E_SHAPE, "B, N and M must be positive");
    if (rule != SDP_TRACEBACK_CPU && rule != SDP_TRACEBACK_CUDA) return fail(SDP_E_VARIANT, "traceback rule must be SDP_TRACEBACK_CPU or SDP_TRACEBACK_CUDA");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    if (rule == SDP_TRACEBACK_CUDA)
        hipLaunchKernelGGL(sdp_traceback_cuda_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, grad, states, counts,
                           lens, B, N, M, sdp_traceback_capacity(N, M));
    else
        hipLaunchKernelGGL(sdp_traceback_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, grad, states, counts,
                           lens, B, N, M, sdp_traceback_capacity(N, M));
    e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "sdp_traceback_kernel");
    return 0;
}

int sdp_traceback_i32(const float *grad, int32_t *states, int32_t *counts, int B, int N, int M, const int32_t *lens,
                      int device, void *stream)
{
    return sdp_traceback_rule_i32(grad, states, counts, B, N, M, lens, SDP_TRACEBACK_CPU, device, stream);
}

// The loss kernels move four columns per 16-byte access only when every row of every tensor they touch starts on a 16-byte
// boundary: M a multiple of 4 AND 16-byte aligned base pointers (include/sdp.h).  A contiguous view at a 4-byte offset has
// M % 4 == 0 but misaligned rows; it takes the scalar path.
static int loss_vec4(int M, const float *ref, const float *pred, const float *G, const float *grad)
{
    auto aligned16 = [](const void *q) { return q == nullptr || (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    return (M & 3) == 0 && aligned16(ref) && aligned16(pred) && aligned16(G) && aligned16(grad);
}

int sdp_loss_forward_f32(const float *ref, const float *pred, const float *G, const int32_t *lens, double *acc, int32_t *cnt,
                         int B, int N, int M, int kind, int device, void *stream)
{
    if (!ref || !pred || !G || !acc || !cnt) return fail(SDP_E_NULLPTR, "sdp_loss_forward_f32: null pointer");
    if (B <= 0 || N <= 0 || M <= 0) return fail(SDP_E_SHAPE, "B, N and M must be positive");
    if (kind < 0 || kind > 2) return fail(SDP_E_VARIANT, "loss kind must be 0 (cross entropy), 1 (path) or 2 (alignment)");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    const int vec4 = loss_vec4(M, ref, pred, G, nullptr);
    hipLaunchKernelGGL(sdp_loss_fwd_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, ref, pred, G, lens, acc, cnt, N, M, kind,
                       vec4);
    e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "sdp_loss_fwd_kernel");
    return 0;
}

int sdp_loss_backward_f32(const float *ref, const float *pred, const float *G, const int32_t *lens, const float *scale,
                          float *grad, int B, int N, int M, int kind, int device, void *stream)
{
    if (!ref || !pred || !G || !scale || !grad) return fail(SDP_E_NULLPTR, "sdp_loss_backward_f32: null pointer");
    if (B <= 0 || N <= 0 || M <= 0) return fail(SDP_E_SHAPE, "B, N and M must be positive");
    if (kind < 0 || kind > 2) return fail(SDP_E_VARIANT, "loss kind must be 0 (cross entropy), 1 (path) or 2 (alignment)");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    const long long groups = (long long)N * ((M + 3) / 4);   // a thread writes four columns per iteration
    int gx = (int)((groups + 256 * 4 - 1) / (256 * 4));
    if (gx < 1) gx = 1;
    if (gx > 64) gx = 64;
    const int vec4 = loss_vec4(M, ref, pred, G, grad);
    hipLaunchKernelGGL(sdp_loss_bwd_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, ref, pred, G, lens, scale, grad, N, M,
                       kind, vec4);
    e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "sdp_loss_bwd_kernel");
    return 0;
}

int sdp_alignment_targets(const uint8_t *codes, const int32_t *code_lens, int L, const int32_t *lens, int B, int N, int M,
                          float *dm, float *P, void *G, int flags, int32_t *status, int device, void *stream)
{
    if (!codes || !code_lens || !status) return fail(SDP_E_NULLPTR, "sdp_alignment_targets: null pointer");
    if (B <= 0 || N <= 0 || M <= 0 || L <= 0) return fail(SDP_E_SHAPE, "B, N, M and L must be positive");
    if (N > SDP_TARGETS_MAX_DIM || M > SDP_TARGETS_MAX_DIM || L > 2 * SDP_TARGETS_MAX_DIM - 1)
        return fail(SDP_E_TOOBIG, "sdp_alignment_targets: N and M must be <= 8192 and L <= 16383");
    if (flags & ~(SDP_TARGETS_GAP_MASK | SDP_TARGETS_G_F32)) return fail(SDP_E_VARIANT, "sdp_alignment_targets: unknown flag");
    const int strips = (M + sdp::TARGETS_TPB - 1) / sdp::TARGETS_TPB;
    if ((long long)strips * B > 0x7fffffffLL) return fail(SDP_E_TOOBIG, "sdp_alignment_targets: too many pairs");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    hipLaunchKernelGGL(sdp_targets_kernel, dim3(strips * B), dim3(sdp::TARGETS_TPB), sdp::targets_lds_bytes(N, L),
                       (hipStream_t)stream, codes, code_lens, L, lens, N, M, strips, dm, P, G, flags, status);
    e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "sdp_targets_kernel");
    return 0;
}

int sdp_targets_selftest(int device)
{
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    int *d = nullptr;
    e = hipMalloc(&d, sizeof(int));
    if (e != hipSuccess) return fail_hip(e, "hipMalloc");
    int h = 0;
    e = hipMemcpy(d, &h, sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sdp_targets_selftest_kernel, dim3(1024), dim3(256), 0, 0, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(&h, d, sizeof(int), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail_hip(e, "sdp_targets_selftest_kernel");
    if (h) return fail(SDP_E_SELFTEST, "sdp_targets_selftest: a square root of P is not correctly rounded");
    return 0;
}

int sdp_alignment_stats(const uint8_t *true_codes, const int32_t *true_lens, int Lt, const void *pred, const int32_t *pred_lens,
                        int Lp, const int32_t *offsets, const int32_t *widths, int W, int B, int flags, int32_t *counts,
                        double *stats, int32_t *hits, double *identity, int32_t *status, int device, void *stream)
{
    if (!true_codes || !true_lens || !pred || !pred_lens || !counts || !status || (W > 0 && !widths))
        return fail(SDP_E_NULLPTR, "sdp_alignment_stats: null pointer");
    if (B <= 0 || Lt <= 0 || Lp <= 0) return fail(SDP_E_SHAPE, "B, Lt and Lp must be positive");
    if (W < 0 || W > SDP_SCORE_MAX_WIDTHS) return fail(SDP_E_SHAPE, "sdp_alignment_stats: W must be in 0 .. 1024");
    if (flags & ~(SDP_SCORE_NO_GAPS | SDP_SCORE_PRED_WALK)) return fail(SDP_E_VARIANT, "sdp_alignment_stats: unknown flag");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    const int rows = Lp < SDP_SCORE_MAX_STATES ? Lp : SDP_SCORE_MAX_STATES;  // a pair's rows <= its states
    hipLaunchKernelGGL(sdp_score_kernel, dim3(B), dim3(sdp::SCORE_TPB), sdp::score_lds_bytes(rows, W), (hipStream_t)stream,
                       true_codes, true_lens, Lt, pred, pred_lens, Lp, rows, offsets, widths, W, flags, counts, stats, hits,
                       identity, status);
    e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "sdp_score_kernel");
    return 0;
}

int sdp_selftest(int device)
{
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    int *d = nullptr;
    e = hipMalloc(&d, 256 * sizeof(int));
    if (e != hipSuccess) return fail_hip(e, "hipMalloc");
    int h[256];
    for (int i = 0; i < 256; ++i) h[i] = 7777;
    (void)hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice);
    hipLaunchKernelGGL(sdp_selftest_kernel, dim3(1), dim3(64), 0, 0, d);
    e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail_hip(e, "sdp_selftest_kernel");
    int bad = 0;
    for (int i = 0; i < 64; ++i) bad |= h[i];
    for (int i = 0; i < 64; ++i)
        if (h[64 + i] != 1000 + i) bad |= 128;   // in-range stores must land
    for (int i = 128; i < 192; ++i)
        if (h[i] != 7777) bad |= 256;            // out-of-range stores must be dropped
    if (bad) {
        snprintf(g_err, sizeof(g_err), "sdp_selftest: hardware semantics mismatch, mask 0x%x", bad);
        return SDP_E_SELFTEST;
    }
    return 0;
}

// ---- the hard-max operator (csrc/sdp_hard.hip) ----
// `variant` of the three entries: SDP_NW / SDP_SW | SDP_HARD_TIES_YMX | SDP_WAVES(w); anything else is refused
static int hard_variant(int variant, int B, int N, int M, bool &ymx, int &waves, int &lo)
{
    ymx = (variant & SDP_HARD_TIES_YMX) != 0;
    waves = take_waves(variant);
    variant &= ~SDP_HARD_TIES_YMX;
    if (int rc = check_shape(B, N, M, variant)) return rc;
    lo = variant == SDP_SW ? 2 : 1;
    return 0;
}

// waves of a workgroup: one per strip in flight, as many as the boundary rows fit LDS for
static int hard_waves(int forced, int N, int M)
{
    return strip_waves(sdp_hard::strips(N), sdp_hard::MAX_WAVES, forced, M, sdp_hard::forward_lds_bytes, sdp_hard::LDS_BUDGET);
}

size_t sdp_hard_state_bytes(int B, int N, int M)
{
    if (B <= 0 || N <= 0 || M <= 0 || M > sdp::MAX_COLS) return 0;
    return (size_t)B * sdp_hard::strips(N) * sdp_hard::words(M) * sdp_hard::STRIP * 4;
}

static int hard_forward(const float *theta, const float *A, void *state, float *Vt, int B, int N, int M, const int32_t *lens,
                        int variant, int device, void *stream, bool pointers)
{
    bool ymx;
    int waves, lo;
    if (int rc = hard_variant(variant, B, N, M, ymx, waves, lo)) return rc;
    if (int rc = use_device(device)) return rc;
    const int W = hard_waves(waves, N, M);
    auto kernel = pointers ? (ymx ? sdp_hard_fwd_t_kernel : sdp_hard_fwd_kernel) : (ymx ? sdp_hard_val_t_kernel : sdp_hard_val_kernel);
    return strip_launch(kernel, pointers ? "sdp_hard_fwd_kernel" : "sdp_hard_val_kernel", B, W, sdp_hard::forward_lds_bytes(W, M), stream,
                        theta, A, static_cast<uint32_t *>(state), Vt, lens, N, M, lo, W);
}

int sdp_hard_forward_f32(const float *theta, const float *A, void *state, float *Vt, int B, int N, int M, const int32_t *lens,
                         int variant, int device, void *stream)
{
    if (!theta || !A || !state || !Vt) return fail(SDP_E_NULLPTR, "sdp_hard_forward_f32: null pointer");
    return hard_forward(theta, A, state, Vt, B, N, M, lens, variant, device, stream, true);
}

int sdp_hard_forward_value_f32(const float *theta, const float *A, float *Vt, int B, int N, int M, const int32_t *lens, int variant,
                               int device, void *stream)
{
    if (!theta || !A || !Vt) return fail(SDP_E_NULLPTR, "sdp_hard_forward_value_f32: null pointer");
    return hard_forward(theta, A, nullptr, Vt, B, N, M, lens, variant, device, stream, false);
}

int sdp_hard_walk_f32(const void *state, const float *Et, float *E, int32_t *states, int32_t *counts, int B, int N, int M,
                      const int32_t *lens, int variant, int device, void *stream)
{
    if (!state || (!E && !states) || (E && !Et) || (states && !counts))
        return fail(SDP_E_NULLPTR, "sdp_hard_walk_f32: null pointer (state; E with Et, or states with counts, or both)");
    bool ymx;
    int waves, lo;
    if (int rc = hard_variant(variant, B, N, M, ymx, waves, lo)) return rc;
    if (int rc = use_device(device)) return rc;
    return strip_launch(sdp_hard_walk_kernel, "sdp_hard_walk_kernel", B, 1, sdp_hard::walk_lds_bytes(M), stream,
                        static_cast<const uint32_t *>(state), Et, E, states, counts, lens, N, M, lo, sdp_traceback_capacity(N, M),
                        ymx ? 1 : 0);
}

// ---- local alignment on the hard-max family: the zero floor, Vt = the best cell, ends = the first cell that holds it ----
static int hard_local_forward(const float *theta, const float *A, void *state, float *Vt, int32_t *ends, int B, int N, int M,
                              const int32_t *lens, int variant, int device, void *stream, bool pointers)
{
    bool ymx;
    int waves, lo;
    if (int rc = hard_variant(variant, B, N, M, ymx, waves, lo)) return rc;
    if (int rc = use_device(device)) return rc;
    const int W = hard_waves(waves, N, M);
    auto kernel = pointers ? (ymx ? sdp_hard_local_fwd_t_kernel : sdp_hard_local_fwd_kernel)
                           : (ymx ? sdp_hard_local_val_t_kernel : sdp_hard_local_val_kernel);
    return strip_launch(kernel, pointers ? "sdp_hard_local_fwd_kernel" : "sdp_hard_local_val_kernel", B, W,
                        sdp_hard::forward_lds_bytes(W, M), stream, theta, A, static_cast<uint32_t *>(state), Vt, ends, lens, N, M, lo, W);
}

int sdp_hard_local_forward_f32(const float *theta, const float *A, void *state, float *Vt, int32_t *ends, int B, int N, int M,
                               const int32_t *lens, int variant, int device, void *stream)
{
    if (!theta || !A || !state || !Vt || !ends) return fail(SDP_E_NULLPTR, "sdp_hard_local_forward_f32: null pointer");
    return hard_local_forward(theta, A, state, Vt, ends, B, N, M, lens, variant, device, stream, true);
}

int sdp_hard_local_forward_value_f32(const float *theta, const float *A, float *Vt, int32_t *ends, int B, int N, int M,
                                     const int32_t *lens, int variant, int device, void *stream)
{
    if (!theta || !A || !Vt) return fail(SDP_E_NULLPTR, "sdp_hard_local_forward_value_f32: null pointer");
    return hard_local_forward(theta, A, nullptr, Vt, ends, B, N, M, lens, variant, device, stream, false);
}

int sdp_hard_local_walk_f32(const void *state, const int32_t *ends, const float *Et, float *E, int32_t *states, int32_t *counts,
                            int B, int N, int M, const int32_t *lens, int variant, int device, void *stream)
{
    if (!state || !ends || (!E && !states) || (E && !Et) || (states && !counts))
        return fail(SDP_E_NULLPTR, "sdp_hard_local_walk_f32: null pointer (state, ends; E with Et, or states with counts, or both)");
    bool ymx;
    int waves, lo;
    if (int rc = hard_variant(variant, B, N, M, ymx, waves, lo)) return rc;
    if (int rc = use_device(device)) return rc;
    return strip_launch(sdp_hard_local_walk_kernel, "sdp_hard_local_walk_kernel", B, 1, sdp_hard::walk_lds_bytes(M), stream,
                        static_cast<const uint32_t *>(state), ends, Et, E, states, counts, lens, N, M, lo, sdp_traceback_capacity(N, M),
                        ymx ? 1 : 0);
}

// ---- the soft local operator (csrc/sdp_soft_local.hip): a differentiable Smith-Waterman, first order ----
// `flags` of the three entries: none is defined, any bit is refused
static int soft_local_args(int B, int N, int M, int flags) { return flagless_args("sdp_soft_local", B, N, M, flags); }

// waves of a workgroup: one per strip in flight, as many as the boundary rows fit LDS for
static int soft_local_waves(int N, int M)
{
    return strip_waves(sdp_soft_local::strips(N), sdp_soft_local::MAX_WAVES, 0, M, sdp_soft_local::sweep_lds_bytes, sdp_soft_local::LDS_BUDGET);
}

size_t sdp_soft_local_state_bytes(int B, int N, int M)
{
    if (B <= 0 || N <= 0 || M <= 0 || M > sdp::MAX_COLS) return 0;
    return (size_t)B * sdp_soft_local::pair_records(N, M) * sdp_soft_local::CELL_BYTES;
}

static int soft_local_forward(const float *theta, const float *A, void *state, float *Vt, int B, int N, int M, const int32_t *lens,
                              int flags, int device, void *stream, bool records)
{
    if (int rc = soft_local_args(B, N, M, flags)) return rc;
    if (int rc = use_device(device)) return rc;
    const int W = soft_local_waves(N, M);
    return strip_launch(records ? sdp_soft_local_fwd_kernel : sdp_soft_local_val_kernel,
                        records ? "sdp_soft_local_fwd_kernel" : "sdp_soft_local_val_kernel", B, W, sdp_soft_local::sweep_lds_bytes(W, M), stream,
                        theta, A, static_cast<float4 *>(state), Vt, lens, N, M, W);
}

int sdp_soft_local_forward_f32(const float *theta, const float *A, void *state, float *Vt, int B, int N, int M, const int32_t *lens,
                               int flags, int device, void *stream)
{
    if (!theta || !A || !state || !Vt) return fail(SDP_E_NULLPTR, "sdp_soft_local_forward_f32: null pointer");
    return soft_local_forward(theta, A, state, Vt, B, N, M, lens, flags, device, stream, true);
}

int sdp_soft_local_forward_value_f32(const float *theta, const float *A, float *Vt, int B, int N, int M, const int32_t *lens, int flags,
                                     int device, void *stream)
{
    if (!theta || !A || !Vt) return fail(SDP_E_NULLPTR, "sdp_soft_local_forward_value_f32: null pointer");
    return soft_local_forward(theta, A, nullptr, Vt, B, N, M, lens, flags, device, stream, false);
}

int sdp_soft_local_backward_f32(const void *state, const float *Vt, const float *Et, float *E, float *G, int B, int N, int M,
                                const int32_t *lens, int flags, int device, void *stream)
{
    if (!state || !Vt || !Et || !E) return fail(SDP_E_NULLPTR, "sdp_soft_local_backward_f32: null pointer (state, Vt, Et, E; G may be NULL)");
    if (int rc = soft_local_args(B, N, M, flags)) return rc;
    if (int rc = use_device(device)) return rc;
    const int W = soft_local_waves(N, M);
    return strip_launch(sdp_soft_local_bwd_kernel, "sdp_soft_local_bwd_kernel", B, W, sdp_soft_local::sweep_lds_bytes(W, M), stream,
                        static_cast<const float4 *>(state), Vt, Et, E, G, lens, N, M, W);
}

// ---- its second order (csrc/sdp_soft_local_adj.hip): the adjoint pair, on the launch geometry of the first order ----
size_t sdp_soft_local_adjoint_state_bytes(int B, int N, int M) { return sdp_soft_local_state_bytes(B, N, M); }

int sdp_soft_local_adjoint_forward_f32(const void *state, const float *Vt, const float *ZE, const float *ZG, void *state_d, float *Vtd,
                                       int B, int N, int M, const int32_t *lens, int flags, int device, void *stream)
{
    if (!state || !Vt || !state_d || !Vtd || (!ZE && !ZG))
        return fail(SDP_E_NULLPTR, "sdp_soft_local_adjoint_forward_f32: null pointer (state, Vt, state_d, Vtd; one of ZE, ZG may be NULL)");
    if (int rc = soft_local_args(B, N, M, flags)) return rc;
    if (int rc = use_device(device)) return rc;
    const int W = soft_local_waves(N, M);
    return strip_launch(sdp_soft_local_adj_fwd_kernel, "sdp_soft_local_adj_fwd_kernel", B, W, sdp_soft_local::sweep_lds_bytes(W, M), stream,
                        static_cast<const float4 *>(state), Vt, ZE, ZG, static_cast<float4 *>(state_d), Vtd, lens, N, M, W);
}

int sdp_soft_local_adjoint_backward_f32(const void *state, const void *state_d, const float *Vt, const float *Vtd, const float *Et,
                                        float *Ed, float *Gd, int B, int N, int M, const int32_t *lens, int flags, int device, void *stream)
{
    if (!state || !state_d || !Vt || !Vtd || !Et || !Ed)
        return fail(SDP_E_NULLPTR, "sdp_soft_local_adjoint_backward_f32: null pointer (state, state_d, Vt, Vtd, Et, Ed; Gd may be NULL)");
    if (int rc = soft_local_args(B, N, M, flags)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = raise_soft_local_adjoint_limit(device)) return rc;
    const int W = soft_local_waves(N, M);
    return strip_launch(sdp_soft_local_adj_bwd_kernel, "sdp_soft_local_adj_bwd_kernel", B, W, sdp_soft_local::adjoint_lds_bytes(W, M), stream,
                        static_cast<const float4 *>(state), static_cast<const float4 *>(state_d), Vt, Vtd, Et, Ed, Gd, lens, N, M, W);
}

// ---- alignments sampled from its posterior (csrc/sdp_soft_local_sample.hip): the end-cell tables, then one walk per sample ----
constexpr int SAMPLE_WAVES = sdp_soft_local_sample::LANES / 64;   // one wave per workgroup, in both kernels
static_assert(sdp_soft_local_sample::LANES % 64 == 0, "a workgroup of the sampling kernels is whole waves");
int sdp_soft_local_end_tables_f32(const void *state, const float *Vt, float *cdf, float *rows, int B, int N, int M, const int32_t *lens,
                                  int flags, int device, void *stream)
{
    if (!state || !Vt || !cdf || !rows) return fail(SDP_E_NULLPTR, "sdp_soft_local_end_tables_f32: null pointer (state, Vt, cdf, rows)");
    if (int rc = soft_local_args(B, N, M, flags)) return rc;
    if (int rc = use_device(device)) return rc;
    // cdf by one wave per (pair, strip); then, behind it on the stream, rows by one wave per pair
    const unsigned waves = (unsigned)B * (unsigned)sdp_soft_local::strips(N);   // <= B N <= 2^31 / M
    for (int pass = 0; pass < 2; ++pass)
        if (int rc = strip_launch(sdp_soft_local_tables_kernel, "sdp_soft_local_tables_kernel", pass ? (unsigned)B : waves, SAMPLE_WAVES, 0,
                                  stream, static_cast<const float4 *>(state), Vt, cdf, rows, lens, N, M, pass))
            return rc;
    return 0;
}

int sdp_soft_local_sample_paths_f32(const void *state, const float *cdf, const float *rows, int32_t *states, int32_t *counts,
                                    int32_t *visits, int32_t *ends, int B, int N, int M, int K, int sample0, uint64_t seed,
                                    const int32_t *lens, int flags, int device, void *stream)
{
    if (!state || !cdf || !rows || (states && !counts) || (!states && !counts && !visits && !ends))
        return fail(SDP_E_NULLPTR, "sdp_soft_local_sample_paths_f32: null pointer (state, cdf, rows; states with counts, or visits, or ends)");
    if (int rc = soft_local_args(B, N, M, flags)) return rc;
    if (K < 1 || sample0 < 0 || (long long)sample0 + K > 0x7fffffffLL)
        return fail(SDP_E_SHAPE, "sdp_soft_local_sample_paths_f32: K must be positive, sample0 non-negative and sample0 + K below 2^31");
    const int cap = sdp_traceback_capacity(N, M);
    const size_t lim = 0x7fffffffu, waves = (size_t)B * ((K + sdp_soft_local_sample::LANES - 1) / sdp_soft_local_sample::LANES);
    if ((states && (size_t)B * K * cap * 3 > lim) || (size_t)B * K * 2 > lim || waves > lim)
        return fail(SDP_E_TOOBIG, "sdp_soft_local_sample_paths_f32: an output exceeds 2^31 elements");
    if (int rc = use_device(device)) return rc;
    sdp_soft_local_sample::Params g = {};
    g.state = static_cast<const float4 *>(state), g.cdf = cdf, g.rows = rows;
    g.states = states, g.counts = counts, g.visits = visits, g.ends = ends, g.lens = lens, g.seed = seed;
    g.B = B, g.N = N, g.M = M, g.K = K, g.sample0 = sample0, g.cap = cap;
    return strip_launch(sdp_soft_local_sample_kernel, "sdp_soft_local_sample_kernel", (unsigned)waves, SAMPLE_WAVES, 0, stream, g);
}

// ---- the affine-gap soft local operator (csrc/sdp_affine_local.hip): gap open and gap extend priced separately, first order ----
// `flags` of the three entries: none is defined, any bit is refused
static int affine_local_args(int B, int N, int M, int flags) { return flagless_args("sdp_affine_local", B, N, M, flags); }

size_t sdp_affine_local_state_bytes(int B, int N, int M)
{
    if (B <= 0 || N <= 0 || M <= 0 || M > sdp::MAX_COLS) return 0;
    return (size_t)B * sdp_affine_local::pair_cells(N, M) * sdp_affine_local::CELL_BYTES;
}

static int affine_local_forward(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt, int B, int N,
                                int M, const int32_t *lens, int flags, int device, void *stream, bool records)
{
    if (int rc = affine_local_args(B, N, M, flags)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = raise_affine_local_limit(device)) return rc;
    const int W = sdp_affine_local::waves_for(N, M);
    return strip_launch(records ? sdp_affine_local_fwd_kernel : sdp_affine_local_val_kernel,
                        records ? "sdp_affine_local_fwd_kernel" : "sdp_affine_local_val_kernel", B, W, sdp_affine_local::sweep_lds_bytes(W, M),
                        stream, theta, gap_open, gap_extend, static_cast<float4 *>(state), Vt, lens, N, M, W);
}

int sdp_affine_local_forward_f32(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt, int B, int N,
                                 int M, const int32_t *lens, int flags, int device, void *stream)
{
    if (!theta || !gap_open || !gap_extend || !state || !Vt) return fail(SDP_E_NULLPTR, "sdp_affine_local_forward_f32: null pointer");
    return affine_local_forward(theta, gap_open, gap_extend, state, Vt, B, N, M, lens, flags, device, stream, true);
}

int sdp_affine_local_forward_value_f32(const float *theta, const float *gap_open, const float *gap_extend, float *Vt, int B, int N, int M,
                                       const int32_t *lens, int flags, int device, void *stream)
{
    if (!theta || !gap_open || !gap_extend || !Vt) return fail(SDP_E_NULLPTR, "sdp_affine_local_forward_value_f32: null pointer");
    return affine_local_forward(theta, gap_open, gap_extend, nullptr, Vt, B, N, M, lens, flags, device, stream, false);
}

int sdp_affine_local_backward_f32(const void *state, const float *Vt, const float *Et, float *E, float *GO, float *GX, int B, int N, int M,
                                  const int32_t *lens, int flags, int device, void *stream)
{
    if (!state || !Vt || !Et || !E)
        return fail(SDP_E_NULLPTR, "sdp_affine_local_backward_f32: null pointer (state, Vt, Et, E; GO and GX may be NULL)");
    if (int rc = affine_local_args(B, N, M, flags)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = raise_affine_local_limit(device)) return rc;
    const int W = sdp_affine_local::waves_for(N, M);
    return strip_launch(sdp_affine_local_bwd_kernel, "sdp_affine_local_bwd_kernel", B, W, sdp_affine_local::sweep_lds_bytes(W, M), stream,
                        static_cast<const float4 *>(state), Vt, Et, E, GO, GX, lens, N, M, W);
}

// ---- its second order (csrc/sdp_affine_local_adj.hip): the adjoint pair; the adjoint backward sweep has a wave count of its own ----
size_t sdp_affine_local_adjoint_state_bytes(int B, int N, int M) { return sdp_affine_local_state_bytes(B, N, M); }

int sdp_affine_local_adjoint_forward_f32(const void *state, const float *Vt, const float *ZE, const float *ZGO, const float *ZGX,
                                         void *state_d, float *Vtd, int B, int N, int M, const int32_t *lens, int flags, int device,
                                         void *stream)
{
    if (!state || !Vt || !state_d || !Vtd || (!ZE && !ZGO && !ZGX))
        return fail(SDP_E_NULLPTR, "sdp_affine_local_adjoint_forward_f32: null pointer (state, Vt, state_d, Vtd; ZE, ZGO, ZGX may be NULL, "
                                   "not all three)");
    if (int rc = affine_local_args(B, N, M, flags)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = raise_affine_local_adjoint_limit(device)) return rc;
    const int W = sdp_affine_local::waves_for(N, M);
    return strip_launch(sdp_affine_local_adj_fwd_kernel, "sdp_affine_local_adj_fwd_kernel", B, W, sdp_affine_local::sweep_lds_bytes(W, M),
                        stream, static_cast<const float4 *>(state), Vt, ZE, ZGO, ZGX, static_cast<float4 *>(state_d), Vtd, lens, N, M, W);
}

int sdp_affine_local_adjoint_backward_f32(const void *state, const void *state_d, const float *Vt, const float *Vtd, const float *Et,
                                          float *Ed, float *GOd, float *GXd, int B, int N, int M, const int32_t *lens, int flags,
                                          int device, void *stream)
{
    if (!state || !state_d || !Vt || !Vtd || !Et || !Ed)
        return fail(SDP_E_NULLPTR, "sdp_affine_local_adjoint_backward_f32: null pointer (state, state_d, Vt, Vtd, Et, Ed; GOd and GXd may "
                                   "be NULL)");
    if (int rc = affine_local_args(B, N, M, flags)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = raise_affine_local_adjoint_limit(device)) return rc;
    const int W = sdp_affine_local::adjoint_waves_for(N, M);
    return strip_launch(sdp_affine_local_adj_bwd_kernel, "sdp_affine_local_adj_bwd_kernel", B, W, sdp_affine_local::adjoint_lds_bytes(W, M),
                        stream, static_cast<const float4 *>(state), static_cast<const float4 *>(state_d), Vt, Vtd, Et, Ed, GOd, GXd, lens,
                        N, M, W);
}

// ---- alignments sampled from its posterior (csrc/sdp_affine_local_sample.hip): the end-cell tables, then one walk per sample ----
static_assert(sdp_affine_local_sample::LANES == sdp_soft_local_sample::LANES, "the two samplers launch the same workgroups");
int sdp_affine_local_end_tables_f32(const void *state, const float *Vt, float *cdf, float *rows, int B, int N, int M, const int32_t *lens,
                                    int flags, int device, void *stream)
{
    if (!state || !Vt || !cdf || !rows) return fail(SDP_E_NULLPTR, "sdp_affine_local_end_tables_f32: null pointer (state, Vt, cdf, rows)");
    if (int rc = affine_local_args(B, N, M, flags)) return rc;
    if (int rc = use_device(device)) return rc;
    // cdf by one wave per (pair, strip); then, behind it on the stream, rows by one wave per pair
    const unsigned waves = (unsigned)B * (unsigned)sdp_affine_local::strips(N);   // <= B N <= 2^31 / M
    for (int pass = 0; pass < 2; ++pass)
        if (int rc = strip_launch(sdp_affine_local_tables_kernel, "sdp_affine_local_tables_kernel", pass ? (unsigned)B : waves, SAMPLE_WAVES,
                                  0, stream, static_cast<const float4 *>(state), Vt, cdf, rows, lens, N, M, pass))
            return rc;
    return 0;
}

int sdp_affine_local_sample_paths_f32(const void *state, const float *Vt, const float *cdf, const float *rows, int32_t *states,
                                      int32_t *counts, int32_t *visits, int32_t *opens, int32_t *extends, int32_t *ends, int B, int N,
                                      int M, int K, int sample0, uint64_t seed, const int32_t *lens, int flags, int device, void *stream)
{
    if (!state || !Vt || !cdf || !rows || (states && !counts) || (!states && !counts && !visits && !opens && !extends && !ends))
        return fail(SDP_E_NULLPTR, "sdp_affine_local_sample_paths_f32: null pointer (state, Vt, cdf, rows; states with counts, or visits, "
                                   "or opens, or extends, or ends)");
    if (int rc = affine_local_args(B, N, M, flags)) return rc;
    if (K < 1 || sample0 < 0 || (long long)sample0 + K > 0x7fffffffLL)
        return fail(SDP_E_SHAPE, "sdp_affine_local_sample_paths_f32: K must be positive, sample0 non-negative and sample0 + K below 2^31");
    const int cap = sdp_traceback_capacity(N, M);
    const size_t lim = 0x7fffffffu, waves = (size_t)B * ((K + sdp_affine_local_sample::LANES - 1) / sdp_affine_local_sample::LANES);
    if ((states && (size_t)B * K * cap * 3 > lim) || (size_t)B * K * 3 > lim || waves > lim)
        return fail(SDP_E_TOOBIG, "sdp_affine_local_sample_paths_f32: an output exceeds 2^31 elements");
    if (int rc = use_device(device)) return rc;
    sdp_affine_local_sample::Params g = {};
    g.state = static_cast<const float4 *>(state), g.Vt = Vt, g.cdf = cdf, g.rows = rows;
    g.states = states, g.counts = counts, g.visits = visits, g.opens = opens, g.extends = extends, g.ends = ends, g.lens = lens;
    g.seed = seed, g.B = B, g.N = N, g.M = M, g.K = K, g.sample0 = sample0, g.cap = cap;
    return strip_launch(sdp_affine_local_sample_kernel, "sdp_affine_local_sample_kernel", (unsigned)waves, SAMPLE_WAVES, 0, stream, g);
}

// ---- the hard affine-gap local operator (csrc/sdp_hard_affine.hip): the max-plus member of the affine family ----
// `variant` of the three entries: SDP_HARD_TIES_YMX | SDP_WAVES(w); anything else, SDP_SW included, is refused
static int hard_affine_args(int variant, int B, int N, int M, bool &ymx, int &waves)
{
    ymx = (variant & SDP_HARD_TIES_YMX) != 0;
    waves = take_waves(variant);
    variant &= ~SDP_HARD_TIES_YMX;
    if (int rc = check_shape(B, N, M, SDP_NW)) return rc;
    if (variant != 0) return fail(SDP_E_VARIANT, "sdp_hard_affine_{local,global}_*: variant takes SDP_HARD_TIES_YMX and SDP_WAVES(w) only");
    if ((size_t)B * (size_t)N * (size_t)M > ((size_t)1 << 31)) return fail(SDP_E_TOOBIG, "B*N*M exceeds 2^31 elements");
    return 0;
}

size_t sdp_hard_affine_local_state_bytes(int B, int N, int M)
{
    if (B <= 0 || N <= 0 || M <= 0 || M > sdp::MAX_COLS) return 0;
    return (size_t)B * sdp_hard_affine::pair_words(N, M) * 4;
}

static int hard_affine_forward(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt, int32_t *ends,
                               int B, int N, int M, const int32_t *lens, int variant, int device, void *stream, bool pointers,
                               bool global = false)
{
    bool ymx;
    int waves;
    if (int rc = hard_affine_args(variant, B, N, M, ymx, waves)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = raise_hard_affine_limit(device)) return rc;
    const int W = sdp_hard_affine::waves_for(N, M, waves);
    auto kernel = pointers ? (ymx ? sdp_hard_affine_local_fwd_t_kernel : sdp_hard_affine_local_fwd_kernel)
                           : (ymx ? sdp_hard_affine_local_val_t_kernel : sdp_hard_affine_local_val_kernel);
    const char *name = pointers ? "sdp_hard_affine_local_fwd_kernel" : "sdp_hard_affine_local_val_kernel";
    if (global) {
        kernel = pointers ? (ymx ? sdp_hard_affine_global_fwd_t_kernel : sdp_hard_affine_global_fwd_kernel)
                          : (ymx ? sdp_hard_affine_global_val_t_kernel : sdp_hard_affine_global_val_kernel);
        name = pointers ? "sdp_hard_affine_global_fwd_kernel" : "sdp_hard_affine_global_val_kernel";
    }
    return strip_launch(kernel, name, B, W, sdp_hard_affine::sweep_lds_bytes(W, M), stream, theta, gap_open, gap_extend,
                        static_cast<uint32_t *>(state), Vt, ends, lens, N, M, W);
}

int sdp_hard_affine_local_forward_f32(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt,
                                      int32_t *ends, int B, int N, int M, const int32_t *lens, int variant, int device, void *stream)
{
    if (!theta || !gap_open || !gap_extend || !state || !Vt || !ends)
        return fail(SDP_E_NULLPTR, "sdp_hard_affine_local_forward_f32: null pointer");
    return hard_affine_forward(theta, gap_open, gap_extend, state, Vt, ends, B, N, M, lens, variant, device, stream, true);
}

int sdp_hard_affine_local_forward_value_f32(const float *theta, const float *gap_open, const float *gap_extend, float *Vt, int32_t *ends,
                                            int B, int N, int M, const int32_t *lens, int variant, int device, void *stream)
{
    if (!theta || !gap_open || !gap_extend || !Vt) return fail(SDP_E_NULLPTR, "sdp_hard_affine_local_forward_value_f32: null pointer");
    return hard_affine_forward(theta, gap_open, gap_extend, nullptr, Vt, ends, B, N, M, lens, variant, device, stream, false);
}

int sdp_hard_affine_local_walk_f32(const void *state, const int32_t *ends, const float *Et, float *E, float *GO, float *GX, int32_t *states,
                                   int32_t *counts, int B, int N, int M, const int32_t *lens, int variant, int device, void *stream)
{
    if (!state || !ends || (!E && !GO && !GX && !states) || ((E || GO || GX) && !Et) || (states && !counts))
        return fail(SDP_E_NULLPTR,
                    "sdp_hard_affine_local_walk_f32: null pointer (state, ends; E, GO or GX with Et, or states with counts, or both)");
    bool ymx;
    int waves;
    if (int rc = hard_affine_args(variant, B, N, M, ymx, waves)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = raise_hard_affine_limit(device)) return rc;
    return strip_launch(sdp_hard_affine_local_walk_kernel, "sdp_hard_affine_local_walk_kernel", B, 1, sdp_hard_affine::walk_lds_bytes(M),
                        stream, static_cast<const uint32_t *>(state), ends, Et, E, GO, GX, states, counts, lens, N, M,
                        sdp_traceback_capacity(N, M), ymx ? 1 : 0);
}

// ---- the hard affine-gap global operator (csrc/sdp_hard_affine.hip, GLOBAL builds): the local member's checks, state and walk ----
size_t sdp_hard_affine_global_state_bytes(int B, int N, int M) { return sdp_hard_affine_local_state_bytes(B, N, M); }

int sdp_hard_affine_global_forward_f32(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt,
                                       int32_t *ends, int B, int N, int M, const int32_t *lens, int variant, int device, void *stream)
{
    if (!theta || !gap_open || !gap_extend || !state || !Vt || !ends)
        return fail(SDP_E_NULLPTR, "sdp_hard_affine_global_forward_f32: null pointer");
    return hard_affine_forward(theta, gap_open, gap_extend, state, Vt, ends, B, N, M, lens, variant, device, stream, true, true);
}

int sdp_hard_affine_global_forward_value_f32(const float *theta, const float *gap_open, const float *gap_extend, float *Vt, int32_t *ends,
                                             int B, int N, int M, const int32_t *lens, int variant, int device, void *stream)
{
    if (!theta || !gap_open || !gap_extend || !Vt) return fail(SDP_E_NULLPTR, "sdp_hard_affine_global_forward_value_f32: null pointer");
    return hard_affine_forward(theta, gap_open, gap_extend, nullptr, Vt, ends, B, N, M, lens, variant, device, stream, false, true);
}

// (the state format, `ends` and the stop at START are the local member's: one walk kernel serves both)
int sdp_hard_affine_global_walk_f32(const void *state, const int32_t *ends, const float *Et, float *E, float *GO, float *GX, int32_t *states,
                                    int32_t *counts, int B, int N, int M, const int32_t *lens, int variant, int device, void *stream)
{
    return sdp_hard_affine_local_walk_f32(state, ends, Et, E, GO, GX, states, counts, B, N, M, lens, variant, device, stream);
}

// ---- the hard affine-gap semi-global operator (csrc/sdp_hard_affine.hip, SEMI builds): the global member with free end gaps ----
size_t sdp_hard_affine_semiglobal_state_bytes(int B, int N, int M) { return sdp_hard_affine_local_state_bytes(B, N, M); }

// free_ends: bit 0 = x, bit 1 = y (sdp_hard_affine::FREE_X, FREE_Y), any other bit is refused; 0 is the global member and launches its kernels, as the soft family does
static int hard_affine_semiglobal_forward(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt,
                                          int32_t *ends, int B, int N, int M, const int32_t *lens, int free_ends, int variant, int device,
                                          void *stream, bool pointers)
{
    bool ymx;
    int waves;
    if (int rc = hard_affine_args(variant, B, N, M, ymx, waves)) return rc;
    if (free_ends & ~sdp_hard_affine::FREE_ENDS_MASK)
        return fail(SDP_E_VARIANT, "sdp_hard_affine_semiglobal_*: free_ends must be 0 .. 3 (bit 0: x, bit 1: y)");
    if (free_ends == 0) return hard_affine_forward(theta, gap_open, gap_extend, state, Vt, ends, B, N, M, lens, variant, device, stream, pointers, true);
    if (int rc = use_device(device)) return rc;
    if (int rc = raise_hard_affine_limit(device)) return rc;
    const int W = sdp_hard_affine::waves_for(N, M, waves);
    auto kernel = pointers ? (ymx ? sdp_hard_affine_semiglobal_fwd_t_kernel : sdp_hard_affine_semiglobal_fwd_kernel)
                           : (ymx ? sdp_hard_affine_semiglobal_val_t_kernel : sdp_hard_affine_semiglobal_val_kernel);
    const char *name = pointers ? "sdp_hard_affine_semiglobal_fwd_kernel" : "sdp_hard_affine_semiglobal_val_kernel";
    return strip_launch(kernel, name, B, W, sdp_hard_affine::sweep_lds_bytes(W, M), stream, theta, gap_open, gap_extend,
                        static_cast<uint32_t *>(state), Vt, ends, lens, N, M, W, free_ends);
}

int sdp_hard_affine_semiglobal_forward_f32(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt,
                                           int32_t *ends, int B, int N, int M, const int32_t *lens, int free_ends, int variant, int device,
                                           void *stream)
{
    if (!theta || !gap_open || !gap_extend || !state || !Vt || !ends)
        return fail(SDP_E_NULLPTR, "sdp_hard_affine_semiglobal_forward_f32: null pointer");
    return hard_affine_semiglobal_forward(theta, gap_open, gap_extend, state, Vt, ends, B, N, M, lens, free_ends, variant, device, stream, true);
}

int sdp_hard_affine_semiglobal_forward_value_f32(const float *theta, const float *gap_open, const float *gap_extend, float *Vt, int32_t *ends,
                                                 int B, int N, int M, const int32_t *lens, int free_ends, int variant, int device,
                                                 void *stream)
{
    if (!theta || !gap_open || !gap_extend || !Vt) return fail(SDP_E_NULLPTR, "sdp_hard_affine_semiglobal_forward_value_f32: null pointer");
    return hard_affine_semiglobal_forward(theta, gap_open, gap_extend, nullptr, Vt, ends, B, N, M, lens, free_ends, variant, device, stream,
                                          false);
}

// (the local member's walk once more, so that the family is whole: it stops at START wherever that is)
int sdp_hard_affine_semiglobal_walk_f32(const void *state, const int32_t *ends, const float *Et, float *E, float *GO, float *GX,
                                        int32_t *states, int32_t *counts, int B, int N, int M, const int32_t *lens, int variant, int device,
                                        void *stream)
{
    return sdp_hard_affine_local_walk_f32(state, ends, Et, E, GO, GX, states, counts, B, N, M, lens, variant, device, stream);
}

// ---- the affine-gap soft global operator (csrc/sdp_affine_global.hip): the Gotoh form of Needleman-Wunsch, first order ----
// `flags` of the three entries: none is defined, any bit is refused
static int affine_global_args(int B, int N, int M, int flags) { return flagless_args("sdp_affine_global", B, N, M, flags); }

size_t sdp_affine_global_state_bytes(int B, int N, int M)
{
    if (B <= 0 || N <= 0 || M <= 0 || M > sdp::MAX_COLS) return 0;
    return (size_t)B * sdp_affine_global::pair_cells(N, M) * sdp_affine_global::CELL_BYTES;
}

static int affine_global_forward(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt, int B, int N,
                                 int M, const int32_t *lens, int flags, int device, void *stream, bool records)
{
    if (int rc = affine_global_args(B, N, M, flags)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = raise_affine_global_limit(device)) return rc;
    const int W = sdp_affine_global::waves_for(N, M);
    return strip_launch(records ? sdp_affine_global_fwd_kernel : sdp_affine_global_val_kernel,
                        records ? "sdp_affine_global_fwd_kernel" : "sdp_affine_global_val_kernel", B, W, sdp_affine_global::sweep_lds_bytes(W, M),
                        stream, theta, gap_open, gap_extend, static_cast<float4 *>(state), Vt, lens, N, M, W);
}

int sdp_affine_global_forward_f32(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt, int B, int N,
                                  int M, const int32_t *lens, int flags, int device, void *stream)
{
    if (!theta || !gap_open || !gap_extend || !state || !Vt) return fail(SDP_E_NULLPTR, "sdp_affine_global_forward_f32: null pointer");
    return affine_global_forward(theta, gap_open, gap_extend, state, Vt, B, N, M, lens, flags, device, stream, true);
}

int sdp_affine_global_forward_value_f32(const float *theta, const float *gap_open, const float *gap_extend, float *Vt, int B, int N, int M,
                                        const int32_t *lens, int flags, int device, void *stream)
{
    if (!theta || !gap_open || !gap_extend || !Vt) return fail(SDP_E_NULLPTR, "sdp_affine_global_forward_value_f32: null pointer");
    return affine_global_forward(theta, gap_open, gap_extend, nullptr, Vt, B, N, M, lens, flags, device, stream, false);
}

int sdp_affine_global_backward_f32(const void *state, const float *Et, float *E, float *GO, float *GX, int B, int N, int M,
                                   const int32_t *lens, int flags, int device, void *stream)
{
    if (!state || !Et || !E) return fail(SDP_E_NULLPTR, "sdp_affine_global_backward_f32: null pointer (state, Et, E; GO and GX may be NULL)");
    if (int rc = affine_global_args(B, N, M, flags)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = raise_affine_global_limit(device)) return rc;
    const int W = sdp_affine_global::waves_for(N, M);
    return strip_launch(sdp_affine_global_bwd_kernel, "sdp_affine_global_bwd_kernel", B, W, sdp_affine_global::sweep_lds_bytes(W, M), stream,
                        static_cast<const float4 *>(state), Et, E, GO, GX, lens, N, M, W);
}

// ---- its free-end-gap member (csrc/sdp_affine_semiglobal.hip): the same launches with one more kernel argument, `free_ends` ----
// `flags`: none is defined, any bit is refused; `free_ends`: bit 0 = x, bit 1 = y, any other bit is refused.  free_ends = 0 is the
// global operator: its kernels are launched (the tail of the state is then not used)
static int affine_semiglobal_args(int B, int N, int M, int free_ends, int flags)
{
    if (int rc = flagless_args("sdp_affine_semiglobal", B, N, M, flags)) return rc;
    if (free_ends & ~sdp_affine_global::FREE_ENDS_MASK)
        return fail(SDP_E_VARIANT, "sdp_affine_semiglobal_*: free_ends must be 0 .. 3 (bit 0: x, bit 1: y)");
    return 0;
}

size_t sdp_affine_semiglobal_state_bytes(int B, int N, int M)
{
    const size_t records = sdp_affine_global_state_bytes(B, N, M);
    return records ? records + (size_t)B * sdp_affine_global::end_tail_words(N, M) * sizeof(int32_t) : 0;
}

static int affine_semiglobal_forward(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt, int B, int N,
                                     int M, const int32_t *lens, int free_ends, int flags, int device, void *stream, bool records)
{
    if (int rc = affine_semiglobal_args(B, N, M, free_ends, flags)) return rc;
    if (free_ends == 0) return affine_global_forward(theta, gap_open, gap_extend, state, Vt, B, N, M, lens, flags, device, stream, records);
    if (int rc = use_device(device)) return rc;
    if (int rc = raise_affine_semiglobal_limit(device)) return rc;
    const int W = sdp_affine_global::waves_for(N, M);
    return strip_launch(records ? sdp_affine_semiglobal_fwd_kernel : sdp_affine_semiglobal_val_kernel,
                        records ? "sdp_affine_semiglobal_fwd_kernel" : "sdp_affine_semiglobal_val_kernel", B, W,
                        sdp_affine_global::sweep_lds_bytes(W, M), stream, theta, gap_open, gap_extend, static_cast<float4 *>(state), Vt, lens, N, M,
                        W, free_ends);
}

int sdp_affine_semiglobal_forward_f32(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt, int B,
                                      int N, int M, const int32_t *lens, int free_ends, int flags, int device, void *stream)
{
    if (!theta || !gap_open || !gap_extend || !state || !Vt) return fail(SDP_E_NULLPTR, "sdp_affine_semiglobal_forward_f32: null pointer");
    return affine_semiglobal_forward(theta, gap_open, gap_extend, state, Vt, B, N, M, lens, free_ends, flags, device, stream, true);
}

int sdp_affine_semiglobal_forward_value_f32(const float *theta, const float *gap_open, const float *gap_extend, float *Vt, int B, int N,
                                            int M, const int32_t *lens, int free_ends, int flags, int device, void *stream)
{
    if (!theta || !gap_open || !gap_extend || !Vt) return fail(SDP_E_NULLPTR, "sdp_affine_semiglobal_forward_value_f32: null pointer");
    return affine_semiglobal_forward(theta, gap_open, gap_extend, nullptr, Vt, B, N, M, lens, free_ends, flags, device, stream, false);
}

int sdp_affine_semiglobal_backward_f32(const void *state, const float *Et, float *E, float *GO, float *GX, int B, int N, int M,
                                       const int32_t *lens, int free_ends, int flags, int device, void *stream)
{
    if (!state || !Et || !E)
        return fail(SDP_E_NULLPTR, "sdp_affine_semiglobal_backward_f32: null pointer (state, Et, E; GO and GX may be NULL)");
    if (int rc = affine_semiglobal_args(B, N, M, free_ends, flags)) return rc;
    if (free_ends == 0) return sdp_affine_global_backward_f32(state, Et, E, GO, GX, B, N, M, lens, flags, device, stream);
    if (int rc = use_device(device)) return rc;
    if (int rc = raise_affine_semiglobal_limit(device)) return rc;
    const int W = sdp_affine_global::waves_for(N, M);
    return strip_launch(sdp_affine_semiglobal_bwd_kernel, "sdp_affine_semiglobal_bwd_kernel", B, W, sdp_affine_global::sweep_lds_bytes(W, M),
                        stream, static_cast<const float4 *>(state), Et, E, GO, GX, lens, N, M, W, free_ends);
}

// ---- its second order (csrc/sdp_affine_global_adj.hip): the adjoint pair; the adjoint backward sweep has a wave count of its own ----
size_t sdp_affine_global_adjoint_state_bytes(int B, int N, int M) { return sdp_affine_global_state_bytes(B, N, M); }

int sdp_affine_global_adjoint_forward_f32(const void *state, const float *ZE, const float *ZGO, const float *ZGX, void *state_d, float *Vtd,
                                          int B, int N, int M, const int32_t *lens, int flags, int device, void *stream)
{
    if (!state || !state_d || !Vtd || (!ZE && !ZGO && !ZGX))
        return fail(SDP_E_NULLPTR, "sdp_affine_global_adjoint_forward_f32: null pointer (state, state_d, Vtd; ZE, ZGO, ZGX may be NULL, not "
                                   "all three)");
    if (int rc = affine_global_args(B, N, M, flags)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = raise_affine_global_adjoint_limit(device)) return rc;
    const int W = sdp_affine_global::waves_for(N, M);
    return strip_launch(sdp_affine_global_adj_fwd_kernel, "sdp_affine_global_adj_fwd_kernel", B, W, sdp_affine_global::sweep_lds_bytes(W, M),
                        stream, static_cast<const float4 *>(state), ZE, ZGO, ZGX, static_cast<float4 *>(state_d), Vtd, lens, N, M, W);
}

// (Vtd holds the place it has in the local entry and is RESERVED: it is not read and may be NULL -- the sweep seeds from the
// differences d_s - sum w d of the end cell's dot records, which lose nothing to the size of Vtd)
int sdp_affine_global_adjoint_backward_f32(const void *state, const void *state_d, const float *Vtd, const float *Et, float *Ed, float *GOd,
                                           float *GXd, int B, int N, int M, const int32_t *lens, int flags, int device, void *stream)
{
    (void)Vtd;
    if (!state || !state_d || !Et || !Ed)
        return fail(SDP_E_NULLPTR, "sdp_affine_global_adjoint_backward_f32: null pointer (state, state_d, Et, Ed; Vtd, GOd and GXd may be "
                                   "NULL)");
    if (int rc = affine_global_args(B, N, M, flags)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = raise_affine_global_adjoint_limit(device)) return rc;
    const int W = sdp_affine_global::adjoint_waves_for(N, M);
    return strip_launch(sdp_affine_global_adj_bwd_kernel, "sdp_affine_global_adj_bwd_kernel", B, W, sdp_affine_global::adjoint_lds_bytes(W, M),
                        stream, static_cast<const float4 *>(state), static_cast<const float4 *>(state_d), Et, Ed, GOd, GXd, lens, N, M, W);
}

// ---- alignments sampled from its posterior (csrc/sdp_affine_global_sample.hip): one walk per sample, from the end cell (n,m) ----
static_assert(sdp_affine_global_sample::LANES == sdp_affine_local_sample::LANES, "the two samplers launch the same workgroups");
int sdp_affine_global_sample_paths_f32(const void *state, int32_t *states, int32_t *counts, int32_t *visits, int32_t *opens,
                                       int32_t *extends, int32_t *ends, int B, int N, int M, int K, int sample0, uint64_t seed,
                                       const int32_t *lens, int flags, int device, void *stream)
{
    if (!state || (states && !counts) || (!states && !counts && !visits && !opens && !extends && !ends))
        return fail(SDP_E_NULLPTR, "sdp_affine_global_sample_paths_f32: null pointer (state; states with counts, or visits, or opens, "
                                   "or extends, or ends)");
    if (int rc = affine_global_args(B, N, M, flags)) return rc;
    if (K < 1 || sample0 < 0 || (long long)sample0 + K > 0x7fffffffLL)
        return fail(SDP_E_SHAPE, "sdp_affine_global_sample_paths_f32: K must be positive, sample0 non-negative and sample0 + K below 2^31");
    const int cap = sdp_traceback_capacity(N, M);
    const size_t lim = 0x7fffffffu, waves = (size_t)B * ((K + sdp_affine_global_sample::LANES - 1) / sdp_affine_global_sample::LANES);
    if ((states && (size_t)B * K * cap * 3 > lim) || (size_t)B * K * 3 > lim || waves > lim)
        return fail(SDP_E_TOOBIG, "sdp_affine_global_sample_paths_f32: an output exceeds 2^31 elements");
    if (int rc = use_device(device)) return rc;
    sdp_affine_global_sample::Params g = {};
    g.state = static_cast<const float4 *>(state);
    g.states = states, g.counts = counts, g.visits = visits, g.opens = opens, g.extends = extends, g.ends = ends, g.lens = lens;
    g.seed = seed, g.B = B, g.N = N, g.M = M, g.K = K, g.sample0 = sample0, g.cap = cap;
    return strip_launch(sdp_affine_global_sample_kernel, "sdp_affine_global_sample_kernel", (unsigned)waves, SAMPLE_WAVES, 0, stream, g);
}

// ---- alignments sampled from the semi-global posterior (csrc/sdp_affine_semiglobal_sample.hip): the table of the end cells' running
// weights, one wave per pair, and one walk per sample from a drawn end cell to a start cell; free_ends = 0 is accepted (one candidate)
static_assert(sdp_affine_semiglobal_sample::LANES == sdp_affine_global_sample::LANES, "the samplers launch the same workgroups");
int sdp_affine_semiglobal_end_table_f32(const void *state, float *ecdf, int B, int N, int M, const int32_t *lens, int free_ends,
                                        int flags, int device, void *stream)
{
    if (!state || !ecdf) return fail(SDP_E_NULLPTR, "sdp_affine_semiglobal_end_table_f32: null pointer (state, ecdf)");
    if (int rc = affine_semiglobal_args(B, N, M, free_ends, flags)) return rc;
    if (int rc = use_device(device)) return rc;
    return strip_launch(sdp_affine_semiglobal_end_table_kernel, "sdp_affine_semiglobal_end_table_kernel", (unsigned)B, SAMPLE_WAVES, 0,
                        stream, static_cast<const float4 *>(state), ecdf, lens, N, M, free_ends);
}

int sdp_affine_semiglobal_sample_paths_f32(const void *state, const float *ecdf, int32_t *states, int32_t *counts, int32_t *visits,
                                           int32_t *opens, int32_t *extends, int32_t *ends, int B, int N, int M, int K, int sample0,
                                           uint64_t seed, const int32_t *lens, int free_ends, int flags, int device, void *stream)
{
    if (!state || !ecdf || (states && !counts) || (!states && !counts && !visits && !opens && !extends && !ends))
        return fail(SDP_E_NULLPTR, "sdp_affine_semiglobal_sample_paths_f32: null pointer (state, ecdf; states with counts, or visits, or "
                                   "opens, or extends, or ends)");
    if (int rc = affine_semiglobal_args(B, N, M, free_ends, flags)) return rc;
    if (K < 1 || sample0 < 0 || (long long)sample0 + K > 0x7fffffffLL)
        return fail(SDP_E_SHAPE, "sdp_affine_semiglobal_sample_paths_f32: K must be positive, sample0 non-negative and sample0 + K below 2^31");
    const int cap = sdp_traceback_capacity(N, M);
    const size_t lim = 0x7fffffffu, waves = (size_t)B * ((K + sdp_affine_semiglobal_sample::LANES - 1) / sdp_affine_semiglobal_sample::LANES);
    if ((states && (size_t)B * K * cap * 3 > lim) || (size_t)B * K * 3 > lim || waves > lim)
        return fail(SDP_E_TOOBIG, "sdp_affine_semiglobal_sample_paths_f32: an output exceeds 2^31 elements");
    if (int rc = use_device(device)) return rc;
    sdp_affine_semiglobal_sample::Params g = {};
    g.state = static_cast<const float4 *>(state), g.ecdf = ecdf;
    g.states = states, g.counts = counts, g.visits = visits, g.opens = opens, g.extends = extends, g.ends = ends, g.lens = lens;
    g.seed = seed, g.B = B, g.N = N, g.M = M, g.K = K, g.sample0 = sample0, g.cap = cap, g.free_ends = free_ends;
    return strip_launch(sdp_affine_semiglobal_sample_kernel, "sdp_affine_semiglobal_sample_kernel", (unsigned)waves, SAMPLE_WAVES, 0, stream, g);
}

// ---- the sparsemax operator (csrc/sdp_sparsemax.hip): the global recurrence under the sparse smoothed maximum, first order ----
// `variant` of the three entries: SDP_NW / SDP_SW | SDP_WAVES(w); anything else is refused
static int sparsemax_args(int variant, int B, int N, int M, int &waves, int &lo)
{
    waves = take_waves(variant);
    if (int rc = check_shape(B, N, M, variant)) return rc;
    if ((size_t)B * (size_t)N * (size_t)M > ((size_t)1 << 31)) return fail(SDP_E_TOOBIG, "B*N*M exceeds 2^31 elements");
    lo = variant == SDP_SW ? 2 : 1;
    return 0;
}

// waves of a workgroup: one per strip in flight, as many as the boundary rows fit LDS for
static int sparsemax_waves(int forced, int N, int M)
{
    return strip_waves(sdp_sparsemax::strips(N), sdp_sparsemax::MAX_WAVES, forced, M, sdp_sparsemax::sweep_lds_bytes, sdp_sparsemax::LDS_BUDGET);
}

size_t sdp_sparsemax_state_bytes(int B, int N, int M)
{
    if (B <= 0 || N <= 0 || M <= 0 || M > sdp::MAX_COLS) return 0;
    return (size_t)B * sdp_sparsemax::pair_records(N, M) * sdp_sparsemax::CELL_BYTES;
}

static int sparsemax_forward(const float *theta, const float *A, void *state, float *Vt, int B, int N, int M, const int32_t *lens,
                             int variant, int device, void *stream, bool records)
{
    int waves, lo;
    if (int rc = sparsemax_args(variant, B, N, M, waves, lo)) return rc;
    if (int rc = use_device(device)) return rc;
    const int W = sparsemax_waves(waves, N, M);
    return strip_launch(records ? sdp_sparsemax_fwd_kernel : sdp_sparsemax_val_kernel,
                        records ? "sdp_sparsemax_fwd_kernel" : "sdp_sparsemax_val_kernel", B, W, sdp_sparsemax::sweep_lds_bytes(W, M), stream,
                        theta, A, static_cast<float4 *>(state), Vt, lens, N, M, lo, W);
}

int sdp_sparsemax_forward_f32(const float *theta, const float *A, void *state, float *Vt, int B, int N, int M, const int32_t *lens,
                              int variant, int device, void *stream)
{
    if (!theta || !A || !state || !Vt) return fail(SDP_E_NULLPTR, "sdp_sparsemax_forward_f32: null pointer");
    return sparsemax_forward(theta, A, state, Vt, B, N, M, lens, variant, device, stream, true);
}

int sdp_sparsemax_forward_value_f32(const float *theta, const float *A, float *Vt, int B, int N, int M, const int32_t *lens, int variant,
                                    int device, void *stream)
{
    if (!theta || !A || !Vt) return fail(SDP_E_NULLPTR, "sdp_sparsemax_forward_value_f32: null pointer");
    return sparsemax_forward(theta, A, nullptr, Vt, B, N, M, lens, variant, device, stream, false);
}

int sdp_sparsemax_backward_f32(const void *state, const float *Vt, const float *Et, float *E, float *G, int B, int N, int M,
                               const int32_t *lens, int variant, int device, void *stream)
{
    // (Vt is part of the trio's call shape and must be what the forward entry wrote; the sweep itself starts from Et alone)
    if (!state || !Vt || !Et || !E) return fail(SDP_E_NULLPTR, "sdp_sparsemax_backward_f32: null pointer (state, Vt, Et, E; G may be NULL)");
    int waves, lo;
    if (int rc = sparsemax_args(variant, B, N, M, waves, lo)) return rc;
    if (int rc = use_device(device)) return rc;
    const int W = sparsemax_waves(waves, N, M);
    return strip_launch(sdp_sparsemax_bwd_kernel, "sdp_sparsemax_bwd_kernel", B, W, sdp_sparsemax::sweep_lds_bytes(W, M), stream,
                        static_cast<const float4 *>(state), Et, E, G, lens, N, M, lo, W);
}

// ---- its second order (csrc/sdp_sparsemax_adj.hip): the adjoint pair, on the launch geometry of the first order ----
size_t sdp_sparsemax_adjoint_state_bytes(int B, int N, int M) { return sdp_sparsemax_state_bytes(B, N, M); }

int sdp_sparsemax_adjoint_forward_f32(const void *state, const float *ZE, const float *ZG, void *state_d, float *Vtd, int B, int N, int M,
                                      const int32_t *lens, int variant, int device, void *stream)
{
    if (!state || !state_d || !Vtd || (!ZE && !ZG))
        return fail(SDP_E_NULLPTR, "sdp_sparsemax_adjoint_forward_f32: null pointer (state, state_d, Vtd; one of ZE, ZG may be NULL)");
    int waves, lo;
    if (int rc = sparsemax_args(variant, B, N, M, waves, lo)) return rc;
    if (int rc = use_device(device)) return rc;
    const int W = sparsemax_waves(waves, N, M);
    return strip_launch(sdp_sparsemax_adj_fwd_kernel, "sdp_sparsemax_adj_fwd_kernel", B, W, sdp_sparsemax::sweep_lds_bytes(W, M), stream,
                        static_cast<const float4 *>(state), ZE, ZG, static_cast<float4 *>(state_d), Vtd, lens, N, M, lo, W);
}

int sdp_sparsemax_adjoint_backward_f32(const void *state, const void *state_d, const float *Et, float *Ed, float *Gd, int B, int N, int M,
                                       const int32_t *lens, int variant, int device, void *stream)
{
    if (!state || !state_d || !Et || !Ed)
        return fail(SDP_E_NULLPTR, "sdp_sparsemax_adjoint_backward_f32: null pointer (state, state_d, Et, Ed; Gd may be NULL)");
    int waves, lo;
    if (int rc = sparsemax_args(variant, B, N, M, waves, lo)) return rc;
    if (int rc = use_device(device)) return rc;
    if (int rc = raise_sparsemax_adjoint_limit(device)) return rc;
    const int W = sparsemax_waves(waves, N, M);
    return strip_launch(sdp_sparsemax_adj_bwd_kernel, "sdp_sparsemax_adj_bwd_kernel", B, W, sdp_sparsemax::adjoint_lds_bytes(W, M), stream,
                        static_cast<const float4 *>(state), static_cast<const float4 *>(state_d), Et, Ed, Gd, lens, N, M, lo, W);
}

// ---- the gap-score gradient (csrc/sdp_gap.hip): G = E (Qx + Qy), Gd = Ed (Qx + Qy) + E (Qdx + Qdy) ----
// Elementwise passes over the state the sweeps left: where a pair's records live, and in which form, is decided by the code the
// sweeps decide it with (state_layout, exact_for, routes_thin).
static int gap_prepare(int device)
{
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    return pending_handoff_error(device);
}

static int gap_launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail_hip(e, what);
}

// threads of a one-thread-per-cell launch over the padded batch, in workgroups; 0 if the grid would not hold them
static unsigned gap_rows_grid(int B, int N, int M)
{
    const size_t wgs = ((size_t)B * N * M + sdp_gap::THREADS - 1) / sdp_gap::THREADS;
    return wgs > 0x7fffffffu ? 0u : (unsigned)wgs;
}

static int gap_tiles(void (*kernel)(const sdp_gap::Params), sdp_gap::Params &g, int TS, bool exact, bool route, void *stream, const char *what)
{
    sdp::Params p = {};
    p.N = g.N, p.M = g.M;
    p.tpad = sdp::state_tpad(g.M);
    state_layout(p);
    g.nstrips_max = sdp::state_nstrips(g.N), g.tpad = p.tpad;
    g.ps = exact ? p.st2_ps : p.st_ps, g.ps_d = p.st2_ps;
    g.us_q = p.st_us, g.us_x = p.st2_us;
    g.whole_exact = exact ? 1 : 0, g.route = route ? 1 : 0;
    auto unaligned = [](const void *ptr) { return ptr != nullptr && ((uintptr_t)ptr & 15u) != 0; };
    g.vec4 = ((g.M & 3) == 0 && !unaligned(g.E) && !unaligned(g.Ed) && !unaligned(g.G)) ? 1 : 0;
    const size_t wgs = (size_t)g.B * g.nstrips_max * sdp_gap::tiles(g.M, TS);
    if (wgs > 0x7fffffffu) return fail(SDP_E_TOOBIG, "too many tiles for one launch");
    hipLaunchKernelGGL(kernel, dim3((unsigned)wgs), dim3(sdp_gap::THREADS), 0, (hipStream_t)stream, g);
    return gap_launched(what);
}

int sdp_gap_gradient_f32(const float *E, const float *state, float *G, int B, int N, int M, const int32_t *lens, int variant, int device,
                         void *stream)
{
    if (!E || !state || !G) return fail(SDP_E_NULLPTR, "sdp_gap_gradient_f32: null pointer");
    if (variant & ~(SDP_SW | SDP_EXACT_STATE | SDP_REF_ROUNDING | SDP_NO_FILL))
        return fail(SDP_E_VARIANT, "sdp_gap_gradient_f32: variant is SDP_NW / SDP_SW | SDP_EXACT_STATE | SDP_REF_ROUNDING | SDP_NO_FILL");
    const VariantBits vb = split_variant(variant);
    if (int rc = check_shape(B, N, M, vb.variant)) return rc;
    const int sw = vb.variant == SDP_SW, fill = (vb.flags & 2) ? 0 : 1;
    if (vb.ref) {
        const unsigned grid = gap_rows_grid(B, N, M);
        if (!grid) return fail(SDP_E_TOOBIG, "sdp_gap_gradient_f32: too many cells for one launch");
        if (int rc = gap_prepare(device)) return rc;
        hipLaunchKernelGGL(sdp_gap_rows_kernel, dim3(grid), dim3(sdp_gap::THREADS), 0, (hipStream_t)stream, E, state, G, lens, B, N, M, sw, fill);
        return gap_launched("sdp_gap_rows_kernel");
    }
    const bool exact = exact_for(vb.exact, N, M);
    if (int rc = gap_prepare(device)) return rc;
    sdp_gap::Params g = {};
    g.E = E, g.state = state, g.G = G, g.lens = lens;
    g.B = B, g.N = N, g.M = M, g.sw = sw, g.fill = fill;
    return gap_tiles(sdp_gap_kernel, g, sdp_gap::TS1, exact, routes_thin(exact, N, M, lens), stream, "sdp_gap_kernel");
}

int sdp_gap_gradient2_f32(const float *E, const float *Ed, const float *state, const float *state_d, float *Gd, int B, int N, int M,
                          const int32_t *lens, int variant, int device, void *stream)
{
    if (!E || !Ed || !state || !state_d || !Gd) return fail(SDP_E_NULLPTR, "sdp_gap_gradient2_f32: null pointer");
    if (variant & ~(SDP_SW | SDP_REF_ROUNDING))
        return fail(SDP_E_VARIANT, "sdp_gap_gradient2_f32: variant is SDP_NW / SDP_SW | SDP_REF_ROUNDING (the state is always the exact one)");
    const VariantBits vb = split_variant(variant);
    if (int rc = check_shape(B, N, M, vb.variant)) return rc;
    const int sw = vb.variant == SDP_SW;
    if (vb.ref) {
        const unsigned grid = gap_rows_grid(B, N, M);
        if (!grid) return fail(SDP_E_TOOBIG, "sdp_gap_gradient2_f32: too many cells for one launch");
        if (int rc = gap_prepare(device)) return rc;
        hipLaunchKernelGGL(sdp_gap2_rows_kernel, dim3(grid), dim3(sdp_gap::THREADS), 0, (hipStream_t)stream, E, Ed, state, state_d, Gd, lens, B, N, M, sw);
        return gap_launched("sdp_gap2_rows_kernel");
    }
    if (int rc = gap_prepare(device)) return rc;
    sdp_gap::Params g = {};
    g.E = E, g.Ed = Ed, g.state = state, g.state_d = state_d, g.G = Gd, g.lens = lens;
    g.B = B, g.N = N, g.M = M, g.sw = sw, g.fill = 1;
    return gap_tiles(sdp_gap2_kernel, g, sdp_gap::TS2, true, false, stream, "sdp_gap2_kernel");
}

int sdp_gap_gradient_f64(const double *E, const double *state, double *G, int B, int N, int M, const int32_t *lens, int variant,
                         int device, void *stream)
{
    if (!E || !state || !G) return fail(SDP_E_NULLPTR, "sdp_gap_gradient_f64: null pointer");
    bool bc;
    const int v = f64_variant(variant, "sdp_gap_gradient_f64", bc);
    if (v < 0 || bc) return v < 0 ? SDP_E_VARIANT : fail(SDP_E_VARIANT, "sdp_gap_gradient_f64: SDP_ET_BROADCAST belongs to the backward sweep");
    if (int rc = check_shape(B, N, M, v)) return rc;
    const unsigned grid = gap_rows_grid(B, N, M);
    if (!grid) return fail(SDP_E_TOOBIG, "sdp_gap_gradient_f64: too many cells for one launch");
    if (int rc = gap_prepare(device)) return rc;
    hipLaunchKernelGGL(sdp_gap_rows_f64_kernel, dim3(grid), dim3(sdp_gap::THREADS), 0, (hipStream_t)stream, E, state, G, lens, B, N, M, v == SDP_SW, 1);
    return gap_launched("sdp_gap_rows_f64_kernel");
}

int sdp_gap_gradient2_f64(const double *E, const double *Ed, const double *state, const double *state_d, double *Gd, int B, int N,
                          int M, const int32_t *lens, int variant, int device, void *stream)
{
    if (!E || !Ed || !state || !state_d || !Gd) return fail(SDP_E_NULLPTR, "sdp_gap_gradient2_f64: null pointer");
    bool bc;
    const int v = f64_variant(variant, "sdp_gap_gradient2_f64", bc);
    if (v < 0 || bc) return v < 0 ? SDP_E_VARIANT : fail(SDP_E_VARIANT, "sdp_gap_gradient2_f64: SDP_ET_BROADCAST belongs to the backward sweep");
    if (int rc = check_shape(B, N, M, v)) return rc;
    const unsigned grid = gap_rows_grid(B, N, M);
    if (!grid) return fail(SDP_E_TOOBIG, "sdp_gap_gradient2_f64: too many cells for one launch");
    if (int rc = gap_prepare(device)) return rc;
    hipLaunchKernelGGL(sdp_gap2_rows_f64_kernel, dim3(grid), dim3(sdp_gap::THREADS), 0, (hipStream_t)stream, E, Ed, state, state_d, Gd, lens, B, N, M,
                       v == SDP_SW);
    return gap_launched("sdp_gap2_rows_f64_kernel");
}

// ---- alignments sampled from the posterior (csrc/sdp_sample.hip): a stochastic traceback on the forward sweep's state ----
// Where a pair's records live, and in which form, is decided by the code the sweeps decide it with, as for the gap gradient.
enum SampleState { SAMPLE_SKEWED, SAMPLE_ROWS, SAMPLE_ROWS_F64 };

static int sample_paths(const char *who, SampleState kind, const void *state, int32_t *states, int32_t *counts, int32_t *visits, int B,
                        int N, int M, int K, int sample0, uint64_t seed, const int32_t *lens, int variant, bool exact_flag, int device,
                        void *stream)
{
    char msg[160];
    if (!state || (!states && !visits) || (states && !counts)) {
        snprintf(msg, sizeof(msg), "%s: null pointer (state; states with counts, or visits, or both)", who);
        return fail(SDP_E_NULLPTR, msg);
    }
    const int transposed = (variant & SDP_SAMPLE_TRANSPOSED) ? 1 : 0;
    const int v = variant & ~SDP_SAMPLE_TRANSPOSED;
    if (int rc = check_shape(B, N, M, v)) return rc;
    if (K < 1 || sample0 < 0 || (long long)sample0 + K > 0x7fffffffLL) {
        snprintf(msg, sizeof(msg), "%s: K must be positive, sample0 non-negative and sample0 + K below 2^31", who);
        return fail(SDP_E_SHAPE, msg);
    }
    const int cap = sdp_traceback_capacity(N, M);
    const size_t lim = 0x7fffffffu, waves = (size_t)B * ((K + sdp_sample::LANES - 1) / sdp_sample::LANES);
    if ((states && (size_t)B * K * cap * 3 > lim) || (size_t)B * K > lim || (visits && (size_t)B * N * M > lim) || waves > lim) {
        snprintf(msg, sizeof(msg), "%s: an output exceeds 2^31 elements", who);
        return fail(SDP_E_TOOBIG, msg);
    }
    if (int rc = gap_prepare(device)) return rc;
    sdp_sample::Params g = {};
    g.state = state, g.states = states, g.counts = counts, g.visits = visits, g.lens = lens, g.seed = seed;
    g.B = B, g.N = N, g.M = M, g.K = K, g.sample0 = sample0;
    g.lo = v == SDP_SW ? 2 : 1, g.cap = cap, g.transposed = transposed;
    void (*kernel)(const sdp_sample::Params) = kind == SAMPLE_ROWS ? sdp_sample_rows_kernel : sdp_sample_rows_f64_kernel;
    const char *name = kind == SAMPLE_ROWS ? "sdp_sample_rows_kernel" : "sdp_sample_rows_f64_kernel";
    if (kind == SAMPLE_SKEWED) {
        const bool exact = exact_for(exact_flag, N, M);
        sdp::Params p = {};
        p.N = N, p.M = M;
        p.tpad = sdp::state_tpad(M);
        state_layout(p);
        g.nstrips_max = sdp::state_nstrips(N);
        g.ps = exact ? p.st2_ps : p.st_ps;
        g.us_q = p.st_us, g.us_x = p.st2_us;
        g.whole_exact = exact ? 1 : 0, g.route = routes_thin(exact, N, M, lens) ? 1 : 0;
        kernel = sdp_sample_kernel, name = "sdp_sample_kernel";
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)waves), dim3(sdp_sample::LANES), 0, (hipStream_t)stream, g);
    return gap_launched(name);
}

int sdp_sample_paths_f32(const void *state, int32_t *states, int32_t *counts, int32_t *visits, int B, int N, int M, int K, int sample0,
                         uint64_t seed, const int32_t *lens, int variant, int device, void *stream)
{
    if (variant & ~(SDP_SW | SDP_EXACT_STATE | SDP_REF_ROUNDING | SDP_SAMPLE_TRANSPOSED))
        return fail(SDP_E_VARIANT, "sdp_sample_paths_f32: variant is SDP_NW / SDP_SW | SDP_EXACT_STATE | SDP_REF_ROUNDING | SDP_SAMPLE_TRANSPOSED");
    const bool ref = (variant & SDP_REF_ROUNDING) != 0, exact = (variant & SDP_EXACT_STATE) != 0;
    return sample_paths("sdp_sample_paths_f32", ref ? SAMPLE_ROWS : SAMPLE_SKEWED, state, states, counts, visits, B, N, M, K, sample0, seed,
                        lens, variant & ~(SDP_EXACT_STATE | SDP_REF_ROUNDING), exact, device, stream);
}

int sdp_sample_paths_f64(const void *state, int32_t *states, int32_t *counts, int32_t *visits, int B, int N, int M, int K, int sample0,
                         uint64_t seed, const int32_t *lens, int variant, int device, void *stream)
{
    if (variant & ~(SDP_SW | SDP_SAMPLE_TRANSPOSED))
        return fail(SDP_E_VARIANT, "sdp_sample_paths_f64: variant is SDP_NW / SDP_SW | SDP_SAMPLE_TRANSPOSED (float64 states take no state / rounding flags)");
    return sample_paths("sdp_sample_paths_f64", SAMPLE_ROWS_F64, state, states, counts, visits, B, N, M, K, sample0, seed, lens, variant, false,
                        device, stream);
}

float sdp_sample_uniform(uint64_t seed, int pair, int sample, int t) { return sdp_sample::uniform(seed, pair, sample, t); }

}  // extern "C"
