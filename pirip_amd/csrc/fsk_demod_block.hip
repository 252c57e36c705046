// pirip_amd/csrc/fsk_demod_block.hip -- workgroup-per-stream FSK demodulator for LONG symbols on gfx950 (MI355X).
//
// `rtl_fsk -r 1000` at the default 240 kS/s (`-m 4 --mask 2000` likewise) means Ts = 240 samples per symbol, 12 000-sample frames and, by
// fsk_create_core's rule, a 4096-point estimator FFT. A wave-per-stream instance would need ~85 KB of LDS per wave (one wave per CU); the
// any-configuration kernel runs this shape with run-time loops at 45 G samples/s (profiles/r03_instance_rates.txt). This file is the shape
// as template arguments, one 256-thread workgroup per stream. The kernel is a frame loop that calls one force-inlined function per stage
// over a per-stream context (`Stream`); DESIGN.md 4.2 lists the stages. What the list does not say:
//   * estimator FFT: 16 points per thread, the six kiss_fft radix-4 stages as three register passes of two stages each with two
//     exchanges through one 34 KB LDS array -- the same butterfly network on the same operands with the same twiddles as kiss_fft
//     [UPSTREAM-RECALLED kiss_fft.c kf_bfly4], so Sf / f_est stay bit-identical; which thread computes which
//     butterfly is bookkeeping:
//       input index i = e0 + 4 e1 + 16 e2 + 64 e3 + 256 e4 + 1024 e5 (base-4 digits); stage s is a 4-point DFT over digit e(6-s)
//       pass A  thread (e3 e2 e1 e0) = t       holds inputs t + 256 n, n = e4 + 4 e5 (coalesced reads); stages m = 1, 4
//                                              -> R[K], K = k0 + 4 k1
//       pass B  thread (K, e1 e0)              collects R[K] over (e3, e2); stages m = 16, 64 with k = K and K + 16 k2
//                                              -> V[k3 + 4 k2] = slot K2 = K + 16 k2 + 64 k3
//       pass C  thread K2                      collects over (e1, e0); stages m = 256, 1024 with k = K2 and K2 + 256 k4
//                                              -> bins K2 + 256 k4 + 1024 k5: a thread ends up with 16 bins that are 256 apart, the
//                                              fftshift keeps them with it, so **Sf lives in 16 registers per thread**
//     exchange layouts: A->B xa[K * 272 + t], B->C xa[K2 * 17 + e10]: every wave-wide 8-byte access touches each LDS bank exactly twice
//     (the minimum) on both sides;
//   * correlator: per-thread restart of the upstream oscillator recursion (table phasor x first-order gain drift, then codec2's
//     float32-rounded per-sample multiplier); no f_dc memory: the last frame's 540 raw samples are kept (LDS, 1 KB) and mixed again with
//     last frame's tone estimates, both oscillators at the phase reference between the last old and the first new sample (see
//     fsk_demod_wave.hip, round 4).
// Numerics as DESIGN.md 5: Sf, f_est bit-exact; nin exact away from threshold ties; rx_filt within tolerance (scaled by N/2400).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../include/pirip_hip.h"
#include "demod_frame.hpp"
#include "demod_simd.hpp"
#include "fsk_device.hpp"

namespace pirip {

namespace {

constexpr int kWave = 64;
constexpr int NT = 256;                 // threads per stream
constexpr int TS = 240, NSYM = 50, P = 15, NDFT = 4096, LOG2N = 12;
constexpr int N = TS * NSYM, Q = TS / 4, NMEM = N + 2 * TS, HIST = 2 * TS + Q, STEP = TS / P, NINT = (NSYM + 1) * P;
constexpr int NFFT = (N - Q) / (NDFT / 2) - 1;
constexpr int NSTEP = NMEM / STEP;      // 780 sixteen-sample steps of integrator memory
// correlator: every thread owns a run of consecutive steps -- three each, and the 12 steps left over go to the first 12 threads of the last
// wave (four steps there): 13 wave-passes over a step instead of the 16 that 195 threads x 4 steps took
constexpr int CSTEPS = NSTEP / NT;      // 3
constexpr int CEXTRA = NSTEP - CSTEPS * NT;   // 12
static_assert(NFFT == 4 && (N + Q) / (NDFT / 2) - 1 == NFFT, "four FFTs per frame whatever nin");
static_assert(NSTEP * STEP == NMEM && CSTEPS * NT <= NSTEP && CEXTRA >= 0 && CEXTRA <= kWave, "integrator memory divides into steps; the left-over steps fit one wave");
static_assert(NINT + P - 1 <= NSTEP, "the last window ends inside the memory");
constexpr int XA_CF = 16 * 272;         // exchange array, complex floats (34 816 bytes)
// A stream's state block in dwords: the raw tail (HIST x 2 bytes), from STATE_TR on per tone last frame's phase step [M] and
// oscillator-table row [M], then its nin -- the trailer in the order of Stream::prev, which is its copy in LDS
constexpr int STATE_TAIL_DW = HIST / 2, STATE_TR = (HIST * 2 + 15) / 16 * 4;
// Tones two at a time in the correlator: four tones' oscillators, switch values and sums at once are 230 VGPR (two workgroups per CU); a
// second pass over the run converts its 64 samples again (+ 13 % instructions in this phase) and fits 168 (three).
constexpr int TPP = 2;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_a2 __attribute__((aligned(2)));      // 16 bytes at the alignment of an (I, Q) byte pair

// two radix-4 stages over 16 register values X[c + 4 dd]: first over dd for every c (twiddles t1[0..2], the same for every c; nullptr:
// trivial), results at X[c + 4 k]; then over c for every k with twiddles t2[3 k + 0..2], results k' at X[k' + 4 k]
__device__ __forceinline__ void radix16(v2f *X, const v2f *t1, const v2f *t2, bool first_trivial)
{
#pragma unroll
    for (int c = 0; c < 4; c++) {
        v2f f0 = X[c], f1 = X[c + 4], f2 = X[c + 8], f3 = X[c + 12];
        if (!first_trivial) { f1 = cmul_x(f1, t1[0]); f2 = cmul_x(f2, t1[1]); f3 = cmul_x(f3, t1[2]); }
        bfly4(f0, f1, f2, f3);
        X[c] = f0; X[c + 4] = f1; X[c + 8] = f2; X[c + 12] = f3;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v2f f0 = X[4 * k], f1 = X[4 * k + 1], f2 = X[4 * k + 2], f3 = X[4 * k + 3];
        if (!(first_trivial && k == 0)) { f1 = cmul_x(f1, t2[3 * k]); f2 = cmul_x(f2, t2[3 * k + 1]); f3 = cmul_x(f3, t2[3 * k + 2]); }
        bfly4(f0, f1, f2, f3);
        X[4 * k] = f0; X[4 * k + 1] = f1; X[4 * k + 2] = f2; X[4 * k + 3] = f3;
    }
}
template <int FMT>
__device__ __forceinline__ v2f cvt_sample_hi(uint32_t v)  // high 16 bits: (I, Q) bytes
{
    return cvt_u8_pair<FMT>(v2f{(float)((v >> 16) & 0xffu), (float)(v >> 24)});
}
template <int FMT>
__device__ __forceinline__ v2f cvt_sample(uint32_t v)     // low 16 bits: (I, Q) bytes
{
    return cvt_u8_pair<FMT>(v2f{(float)(v & 0xffu), (float)((v >> 8) & 0xffu)});
}

// The argument block is read from LDS, i.e. into vector registers; pointers and sizes in it are wave-uniform all the same. Moved to
// scalar registers, global accesses through them use the scalar-base + 32-bit-offset form instead of a 64-bit address pair per access.
template <class T>
__device__ __forceinline__ T *uni(T *p)
{
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return (T *)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
// ... and they point into device memory: read out of the LDS copy of the argument block the compiler only knows them as generic pointers
// and every access through them is a FLAT instruction (a 64-bit address per lane, an LDS-aperture check, and a slot in the LDS wait counter
// as well as the memory one: 196 of them in the first cut). gl() says "global", which gives scalar-base + 32-bit-offset global accesses.
#define PIRIP_GLOBAL __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ PIRIP_GLOBAL T *gl(T *p) { return (PIRIP_GLOBAL T *)uni(p); }
template <class T>
__device__ __forceinline__ PIRIP_GLOBAL T *gl(PIRIP_GLOBAL T *p) { return uni(p); }    // a global pointer advanced by a wave-uniform amount: back to scalar registers
// element idx of a global array. (Measured, interleaved A/B on one box: forming the byte offset in 32 bits -- scalar base + 32-bit lane
// offset for EVERY access of the kernel -- ran 13 % slower than plain indexing, 205 against 235 G samples/s, with fewer instructions; the
// row-base form below is used where the row is wave-uniform and kept because it measured faster there: DESIGN_NOTES.md 4.2b.)
template <class T>
__device__ __forceinline__ T ldg(const PIRIP_GLOBAL T *base, unsigned idx) { return base[(int)idx]; }
// the same with a wave-uniform row base: base and row advance in scalar registers, the lane's own offset is the only vector operand
template <class T>
__device__ __forceinline__ T ldrow(const PIRIP_GLOBAL T *row_base, unsigned lane_elem) { return *(const PIRIP_GLOBAL T *)((const PIRIP_GLOBAL char *)row_base + lane_elem * (unsigned)sizeof(T)); }

// Workgroup barrier that orders LDS traffic only: __syncthreads() also waits for every global load in flight (vmcnt(0)), which would
// put the latency of the twiddle loads issued in front of an exchange back on the critical path.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// block reduction over the 4 waves, two sums at once (one barrier pair); every thread gets the result. red: 16 words of LDS.
__device__ __forceinline__ void block_sum2(float &a, float &b, float *red, int tid)
{
    a = wave_sum(a); b = wave_sum(b);
    __syncthreads();
    if ((tid & 63) == 0) { red[tid >> 6] = a; red[4 + (tid >> 6)] = b; }
    __syncthreads();
    a = ((red[0] + red[1]) + red[2]) + red[3];
    b = ((red[4] + red[5]) + red[6]) + red[7];
}
// arg-max with codec2's tie rule (first maximum wins): candidate (ov, oi) replaces (v, idx) with the larger value, then the smaller index
__device__ __forceinline__ bool argmax_takes(float ov, int oi, float v, int idx) { return ov > v || (ov == v && oi < idx); }
// ... over the workgroup
__device__ __forceinline__ void block_argmax(float &v, int &idx, float *red, int tid)
{
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const float ov = __shfl_xor(v, s);
        const int oi = __shfl_xor(idx, s);
        if (argmax_takes(ov, oi, v, idx)) { v = ov; idx = oi; }
    }
    __syncthreads();
    if ((tid & 63) == 0) { red[tid >> 6] = v; ((int *)red)[8 + (tid >> 6)] = idx; }
    __syncthreads();
    v = red[0]; idx = ((int *)red)[8];
#pragma unroll
    for (int w = 1; w < 4; w++) {
        const float ov = red[w]; const int oi = ((int *)red)[8 + w];
        if (argmax_takes(ov, oi, v, idx)) { v = ov; idx = oi; }
    }
}

// ---- per-stream context ------------------------------------------------------------------------------------------------------------
// What a stage sees of its stream: the workgroup's LDS arrays (the work array s_xa and its aliases are handed to the stages by the frame
// loop), thread and stream ids, the call's extent and what is carried from frame to frame in registers.
// The argument block is copied to LDS once and `args` points at that copy. Every stage re-derives what it needs through stage_args(),
// which makes the pointer opaque, so nothing of the block stays live in registers across the frame loop: by value -- as a DemodArgs
// reference here, or as pointers read out of it and kept here -- it cost the general kernel 223 SGPR spills. (in_base is the one exception.)
struct Stream {
    const DemodArgs *args;
    uint16_t *tail;            // [HIST + 4] last frame's raw tail (I, Q bytes per sample)
    float *red;                // [16] reduction scratch
    uint32_t *dump;            // [kWave] where the line-touching prefetch of the next frame lands (a wave writes lane-linear: 64 dwords)
    uint32_t *prev;            // [2 M + 1] last frame's phase steps [M], oscillator-table rows [M], nin: read once per frame by the correlator
    float *sc;                 // [SC_N] stream scalars that only wave 0 touches, on observable frames
    float *fest;               // [kMaxTones] the latest frame's tone estimates (thread 0 writes them, and reads them back when the state is saved)
    float2 *twb;               // [16][16] pass-B twiddles of the FFT: [K][15], they depend on K = tid >> 4 only
    int tid, sid;
    const PIRIP_GLOBAL uint8_t *in_base;   // the stream's (segment's) first sample
    int64_t nsamp, out0;       // samples from in_base on; output row of the call's first frame
    int max_frames;
    int64_t pos;               // samples consumed by the frames made
    int frame, nin;            // frames made; samples the frame in hand consumes
    bool have_frames;
    float norm_rx_timing, ppm; // these two scalars of the stream live in registers
    float Sf[16];              // the smoothed spectrum at this thread's bins (owned_bin)
};
enum { SC_SNREST, SC_SNR_EST, SC_EBNODB, SC_V_EST, SC_SIG_POW, SC_NSE_POW, SC_N };
struct FrameOut { PIRIP_GLOBAL uint8_t *bits; PIRIP_GLOBAL float *filt; PIRIP_GLOBAL float *stats; int frame_bytes; bool packed; };   // a frame's output rows (nullptr: not requested)

__device__ __forceinline__ const DemodArgs &stage_args(const DemodArgs *ap)
{
    asm volatile("" : "+v"(ap));
    return *ap;
}
// thread tid's register r holds bin K2 + 256 k4 + 1024 k5 (r = k5 + 4 k4, K2 = tid); Sf is stored fftshifted: index (bin + Ndft/2) mod Ndft
__device__ __forceinline__ int owned_bin(int tid, int r) { return (tid + 256 * (r >> 2) + 1024 * (r & 3) + NDFT / 2) & (NDFT - 1); }

// ---- stream state: HBM <-> LDS and registers -----------------------------------------------------------------------------------------
// the state block (STATE_TAIL_DW, STATE_TR) in either direction
template <int M, bool SAVE>
__device__ __forceinline__ void move_state_block(Stream &c, PIRIP_GLOBAL uint32_t *st32)
{
    uint32_t *tail32 = (uint32_t *)c.tail;
    for (int i = c.tid; i < STATE_TAIL_DW; i += NT) { if constexpr (SAVE) st32[i] = tail32[i]; else tail32[i] = st32[i]; }
    if (c.tid == 0) {
#pragma unroll
        for (int i = 0; i < 2 * M + 1; i++) { if constexpr (SAVE) st32[STATE_TR + i] = c.prev[i]; else c.prev[i] = st32[STATE_TR + i]; }
    }
}
// false: this stream slot sits the launch out (SegDesc), its state untouched
template <int M>
__device__ __forceinline__ bool load_state(Stream &c)
{
    const DemodArgs &a = stage_args(c.args);
    const int tid = c.tid, sid = c.sid;
    if (a.io.seg && a.io.seg[sid].max_frames < 0) return false;
    const StreamScalars sc = a.s.scal[sid];
    c.nin = sc.nin; c.norm_rx_timing = sc.norm_rx_timing; c.ppm = sc.ppm;
    if (tid == 0) {
        c.sc[SC_SNREST] = sc.SNRest; c.sc[SC_SNR_EST] = sc.snr_est; c.sc[SC_EBNODB] = sc.EbNodB; c.sc[SC_V_EST] = sc.v_est;
        c.sc[SC_SIG_POW] = sc.rx_sig_pow; c.sc[SC_NSE_POW] = sc.rx_nse_pow;
    }
#pragma unroll
    for (int r = 0; r < 16; r++) c.Sf[r] = gl(a.s.Sf + (size_t)sid * NDFT)[owned_bin(tid, r)];
    move_state_block<M, false>(c, gl((uint32_t *)(a.s.hist + (size_t)sid * M * HIST)));
    {   // slot i of row K: i < 3: tw[K 64 r], r = i + 1 (stage m = 16); else tw[(K + 16 k2) 16 r], k2 = (i - 3) / 3, r = (i - 3) % 3 + 1 (m = 64)
        const int K = tid >> 4, i = tid & 15;
        const int k2 = i < 3 ? 0 : (i - 3) / 3, r = i < 3 ? i + 1 : (i - 3) % 3 + 1;
        const unsigned idx = i < 3 ? (unsigned)(K * 64 * r) : (unsigned)((K + 16 * k2) * 16 * r);
        c.twb[tid] = a.t.tw[i < 15 ? idx : 0];
    }
    return true;
}
// the call's extent for this stream: the batch entry points' own row of the input, or a segment (capture.hip, stream_rx.hip)
__device__ __forceinline__ void open_call(Stream &c)
{
    const DemodArgs &a = stage_args(c.args);
    c.max_frames = (int)(a.io.max_frames < 0x7fffffff ? a.io.max_frames : 0x7fffffff); c.nsamp = a.io.nsamp; c.out0 = 0;
    c.in_base = gl(a.io.in + (size_t)c.sid * a.io.in_stride);
    if (a.io.seg) { const SegDesc sd = a.io.seg[c.sid]; c.in_base += (size_t)sd.in_off * 2; c.nsamp -= sd.in_off; c.out0 = sd.out_frame0; c.max_frames = sd.max_frames; }
    c.pos = 0; c.frame = 0; c.have_frames = false;
}
// Workgroups that start together on a CU walk their frames in lockstep: all of them are in the FFT passes at once and all of them in
// the barrier-separated small phases at once. An experiment (PIRIP_BLOCK_STAGGER=<units>, 0 = off): each wave waits wave-slot x units
// x 8128 clocks before its first frame (HW_ID.wave_id: the workgroups of a CU's first round sit in slots 0, 1, 2 of every SIMD).
__device__ __forceinline__ void stagger_start(const Stream &c)
{
    const int stg = stage_args(c.args).d.block_stagger;
    if (stg > 0) {
        const unsigned slot = __builtin_amdgcn_s_getreg(0x1804) % 3u;
        for (unsigned i = 0; i < slot * (unsigned)stg; i++) __builtin_amdgcn_s_sleep(127);
    }
}
template <int M>
__device__ __forceinline__ void save_state(Stream &c)
{
    const DemodArgs &a = stage_args(c.args);
    const int tid = c.tid, sid = c.sid;
#pragma unroll
    for (int r = 0; r < 16; r++) gl(a.s.Sf + (size_t)sid * NDFT)[owned_bin(tid, r)] = c.Sf[r];
    __syncthreads();
    move_state_block<M, true>(c, gl((uint32_t *)(a.s.hist + (size_t)sid * M * HIST)));
    if (tid == 0) {
        StreamScalars sc = a.s.scal[sid];
        sc.nin = c.nin; sc.norm_rx_timing = c.norm_rx_timing; sc.ppm = c.ppm; sc.SNRest = c.sc[SC_SNREST]; sc.snr_est = c.sc[SC_SNR_EST];
        sc.EbNodB = c.sc[SC_EBNODB]; sc.v_est = c.sc[SC_V_EST]; sc.rx_sig_pow = c.sc[SC_SIG_POW]; sc.rx_nse_pow = c.sc[SC_NSE_POW];
        if (c.have_frames) for (int m = 0; m < kMaxTones; m++) sc.f_est[m] = c.fest[m];
        a.s.scal[sid] = sc;
        if (a.io.nframes) gl(a.io.nframes)[sid] = (int32_t)c.frame;
        if (a.io.consumed) gl(a.io.consumed)[sid] = c.pos;
    }
}

// ---- a-5: frequency estimator ----------------------------------------------------------------------------------------------------------
// the FFT's input: wave-uniform rows of 256 samples / 256 window values
template <int FMT>
__device__ __forceinline__ void load_windowed(v2f *X, const PIRIP_GLOBAL uint16_t *srow, const PIRIP_GLOBAL float *__restrict__ g_hann, int tq)
{
#pragma unroll
    for (int n = 0; n < 16; n++) {         // n = e4 + 4 e5 -> X[c + 4 dd], c = e4, dd = e5
        const v2f x = cvt_sample<FMT>((uint32_t)ldrow(srow + 256 * n, (unsigned)tq));
        const float hn = ldrow(g_hann + 256 * n, (unsigned)tq);
        X[n] = v2f{hn * x.x, hn * x.y};
    }
}
// pass A: m = 1 (trivial twiddles) over e5, then m = 4 over e4 with tw[256 k0 r]: wave-uniform twiddles (scalar loads).
// X[k1 + 4 k0] on return; R[K] with K = k0 + 4 k1 is X[(K >> 2) + 4 (K & 3)]
__device__ __forceinline__ void fft_pass_a(v2f *X, const PIRIP_GLOBAL v2f *__restrict__ g_tw)
{
    v2f t2[12];
#pragma unroll
    for (int i = 0; i < 3; i++) t2[i] = v2f{1.f, 0.f};
#pragma unroll
    for (int k = 1; k < 4; k++)
#pragma unroll
        for (int r = 1; r < 4; r++) t2[3 * k + (r - 1)] = ldg(g_tw, 256u * k * r);                 // m = 4: tw[k fs r], fs = 256
    radix16(X, nullptr, t2, true);
}
// exchange A->B, then pass B: m = 16 over e3 (k = K, fs = 64), then m = 64 over e2 (k = K + 16 k2, fs = 16); its 15 twiddles depend on K
// only and sit in LDS (2 KB for the workgroup: immediate-offset reads instead of 15 global loads with an address each).
// X[k3 + 4 k2] on return is slot K2 = Kb + 16 k2 + 64 k3
__device__ __forceinline__ void fft_pass_b(v2f *X, float2 *xa, const float2 *twb_all, int tid, int tq)
{
    const int Kb = tq >> 4, e10 = tq & 15;
    lds_barrier();                             // the previous FFT's (or frame's) reads of the array are done
#pragma unroll
    for (int K = 0; K < 16; K++) { const v2f v = X[(K >> 2) + 4 * (K & 3)]; xa[K * 272 + tid] = make_float2(v.x, v.y); }
    v2f tb1[3], tb2[12];
    lds_barrier();
    {
        const float2 *twb = twb_all + Kb * 16;
#pragma unroll
        for (int i = 0; i < 3; i++) { const float2 w = twb[i]; tb1[i] = v2f{w.x, w.y}; }
#pragma unroll
        for (int i = 0; i < 12; i++) { const float2 w = twb[3 + i]; tb2[i] = v2f{w.x, w.y}; }
    }
#pragma unroll
    for (int e = 0; e < 16; e++) { const float2 v = xa[Kb * 272 + e * 16 + e10]; X[e] = v2f{v.x, v.y}; }   // e = e2 + 4 e3
    radix16(X, tb1, tb2, false);
}
// exchange B->C, then pass C: m = 256 over e1 (k = K2, fs = 4), then m = 1024 over e0 (k = K2 + 256 k4, fs = 1); twiddles per thread, fetched
// from the 32 KB table g_twc [15][256] (fsk_plan.cpp; L1 / L2) right before the pass -- 30 loads per FFT with pass B's against 78 registers
// held for the whole frame. X[k5 + 4 k4] on return = bin K2 + 256 k4 + 1024 k5
__device__ __forceinline__ void fft_pass_c(v2f *X, float2 *xa, const PIRIP_GLOBAL v2f *__restrict__ g_twc, int tid, int tq)
{
    const int Kb = tq >> 4, e10 = tq & 15;
    lds_barrier();
#pragma unroll
    for (int k2 = 0; k2 < 4; k2++)
#pragma unroll
        for (int k3 = 0; k3 < 4; k3++) { const v2f v = X[k3 + 4 * k2]; xa[(Kb + 16 * k2 + 64 * k3) * 17 + e10] = make_float2(v.x, v.y); }
    v2f tc1[3], tc2[12];
#pragma unroll
    for (int i = 0; i < 3; i++) tc1[i] = ldrow(g_twc + 256 * i, (unsigned)tq);
#pragma unroll
    for (int i = 0; i < 12; i++) tc2[i] = ldrow(g_twc + 256 * (3 + i), (unsigned)tq);
    lds_barrier();
#pragma unroll
    for (int e = 0; e < 16; e++) { const float2 v = xa[tid * 17 + e]; X[e] = v2f{v.x, v.y}; }                // e = e0 + 4 e1
    radix16(X, tc1, tc2, false);
}
// |X| of the thread's 16 bins, correctly rounded in three tiers (demod_simd.hpp), folded into Sf
__device__ __forceinline__ void smooth_bins(float (&Sf)[16], const v2f *X, float k1mtc, float ktc)
{
    float mg[16];
    unsigned kmin = 0xffffffffu;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        mg[r] = (X[r].x * X[r].x) + (X[r].y * X[r].y);
        const unsigned key = __builtin_bit_cast(unsigned, mg[r]);       // (non-negative floats order as unsigned integers)
        kmin = key < kmin ? key : kmin;
    }
    if (__all(kmin >= 0x0f800000u)) {                                   // every |X|^2 >= 2^-96: roots without the zero guard
#pragma unroll
        for (int r = 0; r < 16; r++) mg[r] = sqrt_rn_normal<true, true>(mg[r]);
    } else {
        kmin = 0xffffffffu;
#pragma unroll
        for (int r = 0; r < 16; r++) { const unsigned key = __builtin_bit_cast(unsigned, mg[r]) - 1u; kmin = key < kmin ? key : kmin; }
        if (__all(kmin >= 0x0f800000u - 1u)) {                          // zeros among them (a silent input)
#pragma unroll
            for (int r = 0; r < 16; r++) mg[r] = sqrt_rn_normal<true>(mg[r]);
        } else {
#pragma unroll
            for (int r = 0; r < 16; r++) mg[r] = sqrtf(mg[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; r++) Sf[r] = (Sf[r] * k1mtc) + (mg[r] * ktc);
}
// NFFT half-overlapped Hann-windowed FFTs of the frame, each folded into Sf. xa: the exchange array.
// (no software prefetch and no register-resident Hann samples or twiddles: each is fetched from L1 / L2 where it is used. With
//  prefetches the kernel held 252 VGPR = two workgroups per CU and ran 193 G samples/s (2-FSK); at <= 168 VGPR a third
//  workgroup fits and its waves hide the same latencies: 228 G)
template <int FMT>
__device__ __forceinline__ void fft_frame(Stream &c, const PIRIP_GLOBAL uint16_t *gin, float2 *xa)
{
    const DemodArgs &a = stage_args(c.args);
    const PIRIP_GLOBAL v2f *__restrict__ g_tw = gl((const v2f *)a.t.tw);
    const PIRIP_GLOBAL float *__restrict__ g_hann = gl(a.t.hann);
    const PIRIP_GLOBAL v2f *__restrict__ g_twc = gl((const v2f *)a.t.fast_tab);
    const float k1mtc = a.d.one_minus_tc, ktc = a.d.tc;
    // (the thread index as a local of this stage, not c.tid at each use: measured, interleaved A/B -- read from the context the 4-FSK mask
    //  instance holds 152 VGPR instead of 150 and runs 0.6 % slower, 208.0 against 209.8 G samples/s: profiles/bk_stages_ab.txt)
    const int tid = c.tid;
#pragma unroll 1
    for (int j = 0; j < NFFT; j++) {
        // (an opaque copy of the thread index per FFT: the twiddle loads below are loop-invariant, and hoisted out of this
        //  loop they are 54 more live registers for the whole frame)
        int tq = tid; asm volatile("" : "+v"(tq));
        v2f X[16];
        load_windowed<FMT>(X, gin + (NDFT / 2) * j, g_hann, tq);
        fft_pass_a(X, g_tw);
        fft_pass_b(X, xa, c.twb, tid, tq);
        fft_pass_c(X, xa, g_twc, tid, tq);
        smooth_bins(c.Sf, X, k1mtc, ktc);
    }
}
// peak method: the M largest bins of Sf, each with its neighbourhood zeroed before the next is sought, then in ascending order -- on
// the registers that hold Sf
template <int M>
__device__ __forceinline__ void pick_peaks(Stream &c, Tones &tn)
{
    const FskDims &d = stage_args(c.args).d;
    const int tid = c.tid;
    int sfi[16], freqi[M];
    float w[16];
    const int est_st = uni(d.est_st), est_en = uni(d.est_en), f_zero = uni(d.f_zero);
#pragma unroll
    for (int r = 0; r < 16; r++) { sfi[r] = owned_bin(tid, r); w[r] = c.Sf[r]; }
#pragma unroll
    for (int m = 0; m < M; m++) {
        float best = 0.0f; int ib = 0;
#pragma unroll
        for (int r = 0; r < 16; r++)
            if (sfi[r] >= est_st && sfi[r] < est_en && (w[r] > best || (w[r] == best && best > 0.0f && sfi[r] < ib))) { best = w[r]; ib = sfi[r]; }
        block_argmax(best, ib, c.red, tid);
        int f_min = ib - f_zero; f_min = f_min < 0 ? 0 : f_min;
        int f_max = ib + f_zero; f_max = f_max > NDFT ? NDFT : f_max;
#pragma unroll
        for (int r = 0; r < 16; r++) if (sfi[r] >= f_min && sfi[r] < f_max) w[r] = 0.0f;
        freqi[m] = ib - NDFT / 2;
    }
#pragma unroll
    for (int x = 1; x < M; x++)
#pragma unroll
        for (int y = x; y > 0; y--)
            if (freqi[y] < freqi[y - 1]) { const int t = freqi[y]; freqi[y] = freqi[y - 1]; freqi[y - 1] = t; }
#pragma unroll
    for (int m = 0; m < M; m++) {
        tn.f_est[m] = (float)freqi[m] * d.bin_hz;
        tn.dtheta[m] = (uint32_t)freqi[m] << (32 - LOG2N); tn.drift_ix[m] = freqi[m] + NDFT / 2;
    }
}
// mask method: comb of 3-bin teeth slid over Sf, tooth sums in ascending order; the tones follow from the comb's position.
// sfl: [NDFT] floats for the linear spectrum (on the work array; the caller's barrier frees it again)
template <int M>
__device__ __forceinline__ void slide_mask(Stream &c, float *sfl, Tones &tn)
{
    const DemodArgs &a = stage_args(c.args);
    const FskDims &d = a.d;
    const int tid = c.tid;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; r++) sfl[owned_bin(tid, r)] = c.Sf[r];
    __syncthreads();
    const int est_st = uni(d.est_st), b_end = uni(d.est_en - d.mask_len), n_teeth = uni(d.n_teeth);
    const PIRIP_GLOBAL int16_t *__restrict__ g_teeth = gl(a.t.teeth);
    float best = 0.0f; int bb = est_st;
#pragma unroll 1
    for (int b = est_st + tid; b < b_end; b += NT) {
        float corr = 0.0f;
        for (int k = 0; k < n_teeth; k++) corr += sfl[b + g_teeth[k]];
        if (corr > best) { best = corr; bb = b; }
    }
    block_argmax(best, bb, c.red, tid);
#pragma unroll
    for (int m = 0; m < M; m++) {
        tn.f_est[m] = (float)((bb - NDFT / 2) * d.Fs / NDFT) + (float)(m * d.tone_spacing);
        tn.dtheta[m] = gl(a.t.mask_dtheta)[bb * M + m]; tn.drift_ix[m] = bb * M + m;
    }
}

// ---- a-6: down-convert, sums over the 16-sample window steps ---------------------------------------------------------------------------
// exp(+j theta), theta in 2^-32 turns: top LOG2N bits index the twiddle table, the remainder (mask method only: a peak's step is a whole
// bin) is a small-angle rotation
template <bool MASK>
__device__ __forceinline__ v2f phasor(const PIRIP_GLOBAL v2f *__restrict__ g_tw, uint32_t th)
{
    const v2f w = ldg(g_tw, th >> (32 - LOG2N));
    float pc = w.x, ps = -w.y;
    if constexpr (MASK) {
        const float bl = (float)(th & ((1u << (32 - LOG2N)) - 1u)) * 1.4629180792671596e-9f;
        const float b2 = bl * bl;
        const float cb = 1.0f - b2 * (0.5f - b2 * (1.0f / 24.0f));
        const float sb = bl * (1.0f - b2 * ((1.0f / 6.0f) - b2 * (1.0f / 120.0f)));
        const float c2 = pc * cb - ps * sb, s2 = ps * cb + pc * sb;
        pc = c2; ps = s2;
    }
    return v2f{pc, ps};
}
// The 16 raw samples of the step at memory position jb, two per dword: new ones from global memory -- 32 contiguous bytes per thread,
// fetched as two 16-byte loads (sample by sample it was 16 loads per step whose 64 lanes each touched a different cache line: 4096 line
// accesses per wave and frame, as much time in the texture path as the whole frame's arithmetic) -- old ones from the tail kept in LDS
__device__ __forceinline__ void load_step(const uint16_t *tail, const PIRIP_GLOBAL uint16_t *gin, int jb, int nold, uint32_t *dst)
{
    if (jb >= nold) {
        const PIRIP_GLOBAL char *p = (const PIRIP_GLOBAL char *)gin + 2u * (unsigned)(jb - nold);
#pragma unroll
        for (int q = 0; q < STEP / 8; q++) {
            const u32x4 v = *(const PIRIP_GLOBAL u32x4_a2 *)(p + 16 * q);
            dst[4 * q] = v.x; dst[4 * q + 1] = v.y; dst[4 * q + 2] = v.z; dst[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < STEP; k += 2) {
            uint32_t pair = 0;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int j = jb + k + h;
                const uint32_t w = j < nold ? (uint32_t)tail[HIST - nold + j] : (uint32_t)ldg(gin, (unsigned)(j < nold ? 0 : j - nold));
                pair |= w << (16 * h);
            }
            dst[k / 2] = pair;
        }
    }
}
// a tone pair's oscillators: phase and per-sample multiplier in hand, and the values the new oscillator starts with
struct Osc { v2f ph[TPP], dph[TPP], swp[TPP], swd[TPP]; };
// One step of a tone pair: its 16 samples mixed with the running oscillators into acc. SWITCH: the first new sample of the frame (nold is a
// multiple of 4) is where the new oscillator starts, at place sw_k of this step: one thread of the workgroup meets it, in one of its
// steps -- every other wave-pass runs the loop without the test and its selects
template <int FMT, bool SWITCH>
__device__ __forceinline__ void mix_step(const uint32_t *rawv, int sw_k, Osc &o, v2f *acc)
{
#pragma unroll
    for (int k = 0; k < STEP; k++) {
        if constexpr (SWITCH) {
            if ((k & 3) == 0 && k == sw_k) {
#pragma unroll
                for (int m = 0; m < TPP; m++) { o.ph[m] = o.swp[m]; o.dph[m] = o.swd[m]; }
            }
        }
        const v2f x = (k & 1) ? cvt_sample_hi<FMT>(rawv[k >> 1]) : cvt_sample<FMT>(rawv[k >> 1]);
#pragma unroll
        for (int m = 0; m < TPP; m++) {
            acc[m] = mix_conj_acc(x, o.ph[m], acc[m]);
            o.ph[m] = rot_step(o.ph[m], o.dph[m]);
        }
    }
}
// Every thread owns a run of CSTEPS consecutive 16-sample steps (the first CEXTRA threads of the last wave: one more), converts a step's
// samples once for two tones and leaves the sums over its steps in step[M][NSTEP]. Old positions (the last frame's tail) are mixed with
// the last frame's tone estimates (Stream::prev), new ones with tn.
template <int M, int FMT, bool MASK>
__device__ __forceinline__ void correlate(Stream &c, const PIRIP_GLOBAL uint16_t *gin, const Tones &tn, float2 (*step)[NSTEP])
{
    const DemodArgs &a = stage_args(c.args);
    const PIRIP_GLOBAL v2f *__restrict__ g_tw = gl((const v2f *)a.t.tw);
    const PIRIP_GLOBAL v2f *__restrict__ g_step = gl((const v2f *)a.t.osc_step), *__restrict__ g_drift = gl((const v2f *)a.t.osc_drift);
    const int tid = c.tid, nold = NMEM - c.nin;
    const int xt = tid - (NT - kWave);             // lane of the last wave
    const int step0 = CSTEPS * tid + (xt < 0 ? 0 : xt < CEXTRA ? xt : CEXTRA);     // this thread's first step
    const int nsteps = CSTEPS + (xt >= 0 && xt < CEXTRA ? 1 : 0);
    const int j0 = STEP * step0;                   // first memory position of this thread
    const int n0 = j0 - nold + 1;                  // recursion steps before it, counted from the frame's phase reference
    const int nold_run = nold - j0;                // positions of this run that are last frame's (<= 0: none, >= its length: all)
    const bool oldl = nold_run > 0;
    const int ninp = (int)c.prev[2 * M];
    const bool no_tail = ninp == 0;                // a stream's very first frame: integrator memory is zero
#pragma unroll
    for (int mp = 0; mp < M; mp += TPP) {
        Osc o;
#pragma unroll
        for (int m = 0; m < TPP; m++) {
            const uint32_t dthp = c.prev[mp + m], tixp = c.prev[M + mp + m];
            const v2f stn = ldg(g_step, (unsigned)tn.drift_ix[mp + m]), stp = ldg(g_step, tixp);
            const float dn = ldg(g_drift, (unsigned)tn.drift_ix[mp + m]).x, dp = ldg(g_drift, tixp).x;
            const uint32_t th = (uint32_t)n0 * (oldl ? dthp : tn.dtheta[mp + m]);
            const float g = 1.0f + (oldl ? dp * (float)(ninp + n0) : dn * (float)n0);
            const v2f pcs = phasor<MASK>(g_tw, th);
            o.ph[m] = v2f{pcs.x * g, pcs.y * g};
            if (no_tail && oldl) o.ph[m] = v2f{0.f, 0.f};    // no integrator memory yet: old positions contribute zeros (a zero phasor stays zero)
            o.dph[m] = oldl ? v2f{stp.x, stp.y} : v2f{stn.x, stn.y};
            const v2f p1 = phasor<MASK>(g_tw, tn.dtheta[mp + m]);
            const float g1 = 1.0f + dn;
            o.swp[m] = v2f{p1.x * g1, p1.y * g1};
            o.swd[m] = v2f{stn.x, stn.y};
        }
#pragma unroll 1
        for (int blk = 0; blk < CSTEPS + 1; blk++) {
            if (blk >= nsteps) continue;
            uint32_t rawv[STEP / 2];
            load_step(c.tail, gin, j0 + STEP * blk, nold, rawv);
            v2f acc[TPP];
#pragma unroll
            for (int m = 0; m < TPP; m++) acc[m] = v2f{0.f, 0.f};
            const int sw_k = nold_run - STEP * blk;        // the first new sample's place in this step
            if (__builtin_amdgcn_ballot_w64(oldl && sw_k >= 0 && sw_k < STEP)) mix_step<FMT, true>(rawv, sw_k, o, acc);
            else mix_step<FMT, false>(rawv, sw_k, o, acc);
#pragma unroll
            for (int m = 0; m < TPP; m++) step[mp + m][step0 + blk] = make_float2(acc[m].x, acc[m].y);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}
// Touch the next frame's cache lines (one dword of each 128-byte line, landing in a dump row of LDS nobody reads): they are on their
// way to L2 while the window sums, the timing estimate and the decisions run, instead of being fetched from HBM by the next FFT.
// (issued right after the FFTs instead, a whole correlator pass earlier, it measured the same)
__device__ __forceinline__ void prefetch_next(const Stream &c, const PIRIP_GLOBAL uint16_t *gin)
{
    const int64_t left = c.nsamp - (c.pos + c.nin);                      // samples behind this frame
    const unsigned off = (unsigned)c.tid * 128u;
    if ((int64_t)(off / 2 + 2) <= left && off < (unsigned)(N + Q) * 2u)
        __builtin_amdgcn_global_load_lds((const PIRIP_GLOBAL void *)((const PIRIP_GLOBAL char *)gin + 2u * (unsigned)c.nin + off),
                                         (__attribute__((address_space(3))) void *)c.dump, 4, 0, 0);
}
// the frame's last HIST raw samples are the next frame's old positions, mixed with this frame's tones and counted from this frame's nin
// (the correlator's reads are behind the caller's barrier; the next ones are a frame away)
template <int M>
__device__ __forceinline__ void keep_tail(Stream &c, const PIRIP_GLOBAL uint16_t *gin, const Tones &tn)
{
    for (int i = c.tid; i < HIST; i += NT) c.tail[i] = ldg(gin, (unsigned)(c.nin - HIST + i));
    if (c.tid == 0) {
        c.prev[2 * M] = (uint32_t)c.nin;
#pragma unroll
        for (int m = 0; m < M; m++) { c.prev[m] = tn.dtheta[m]; c.prev[M + m] = (uint32_t)tn.drift_ix[m]; }
    }
}

// ---- a-7: window sums (15 steps each), fine timing -------------------------------------------------------------------------------------
// f_int = 15 consecutive step sums per window and tone; returns this thread's share of t_c = sum of window power x the upstream
// recursion's timing phasor (the barriers of the workgroup sum that follows also publish fint)
template <int M>
__device__ __forceinline__ float2 window_sums(Stream &c, const float2 (*step)[NSTEP], float2 (*fint)[NINT])
{
    const PIRIP_GLOBAL v2f *__restrict__ g_trec = gl((const v2f *)stage_args(c.args).t.timing_rec);
    float tcr = 0.f, tci = 0.f;
    for (int w = c.tid; w < NINT; w += NT) {
        float ft1 = 0.f;
#pragma unroll
        for (int m = 0; m < M; m++) {
            v2f acc{0.f, 0.f};
#pragma unroll
            for (int q = 0; q < P; q++) { const float2 v = step[m][w + q]; acc = acc + v2f{v.x, v.y}; }
            fint[m][w] = make_float2(acc.x, acc.y);
            ft1 += (acc.x * acc.x) + (acc.y * acc.y);
        }
        const v2f tp = ldg(g_trec, (unsigned)w);
        tcr += ft1 * tp.x; tci += ft1 * tp.y;
    }
    return make_float2(tcr, tci);
}
// The timing estimate into the stream's scalars, ppm smoothing included, and what follows from it: the next frame's nin and where the
// symbols are sampled
__device__ __forceinline__ Timing update_timing(Stream &c, float2 tc)
{
    const float norm_rx_timing = atan2f(tc.y, tc.x) * 0.15915494309189535f;
    const float rx_timing = norm_rx_timing * (float)P;
    const float d_norm = norm_rx_timing - c.norm_rx_timing;
    c.norm_rx_timing = norm_rx_timing;
    if (fabsf(d_norm) < 0.2f) {
        const float appm = (1e6f * d_norm) / (float)NSYM;
        c.ppm = (0.9f * c.ppm) + (0.1f * appm);
    }
    Timing t;
    t.nin_next = N;
    if (!stage_args(c.args).d.burst_mode) {
        if (norm_rx_timing > 0.25f) t.nin_next = N + Q;
        else if (norm_rx_timing < -0.25f) t.nin_next = N - Q;
    }
    t.low_sample = (int)floorf(rx_timing);
    t.fract = rx_timing - (float)t.low_sample;
    t.high_sample = (int)ceilf(rx_timing);
    return t;
}

// ---- a-8: resample, decide, stats ------------------------------------------------------------------------------------------------------
// this frame's output rows
template <int M>
__device__ __forceinline__ FrameOut frame_out(const Stream &c)
{
    const DemodArgs &a = stage_args(c.args);
    const FskDims &d = a.d;
    FrameOut o;
    o.packed = d.pack_bits;
    o.frame_bytes = d.pack_bits ? (d.Nbits + 7) / 8 : d.Nbits;
    const size_t orow = (size_t)(c.frame + c.out0);
    o.bits = gl(a.io.bits ? a.io.bits + (size_t)c.sid * a.io.bits_stride + orow * o.frame_bytes : nullptr);
    o.filt = gl(a.io.filt ? a.io.filt + (size_t)c.sid * a.io.filt_stride + orow * M * NSYM : nullptr);
    o.stats = gl(a.io.stats ? a.io.stats + (size_t)c.sid * a.io.stats_stride + orow * PIRIP_STATS_PER_FRAME : nullptr);
    return o;
}
// Thread i < Nsym takes symbol i: its tone powers at the timing estimate, the hard decision (returned in sym; written here one bit per
// byte unless the frame's bits are packed), the soft magnitudes, and its terms of the power sums
template <int M>
__device__ __forceinline__ SymbolSums decide_symbols(const Stream &c, const Timing &t, const FrameOut &o, const float2 (*fint)[NINT], int &sym)
{
    const int tid = c.tid;
    const bool act = tid < NSYM;
    const int st = ((act ? tid : 0) + 1) * P;
    SymbolSums s = {0.f, 0.f, 0.f, 0.f};
    float tmax[M];
    float sum = 0.f;
#pragma unroll
    for (int m = 0; m < M; m++) {
        tmax[m] = tone_power(fint[m][st + t.low_sample], fint[m][st + t.high_sample], t.fract);
        sum += tmax[m];
    }
    float mx = tmax[0];
    sym = 0;
#pragma unroll
    for (int m = 1; m < M; m++) if (tmax[m] > mx) { mx = tmax[m]; sym = m; }
    if (act) { s.sig = mx; s.nse = (sum - mx) / (float)(M - 1); s.std_e = mx; s.mean_e = sqrtf(mx); }
    if (o.bits && !o.packed && act) {
        if (M == 2) o.bits[tid] = sym == 1;
        else { o.bits[2 * tid + 1] = sym & 1; o.bits[2 * tid] = (sym & 2) >> 1; }
    }
    if (act && o.filt) {
#pragma unroll
        for (int m = 0; m < M; m++) o.filt[m * NSYM + tid] = sqrtf(tmax[m]);
    }
    return s;
}
// packed bits, first bit in the MSB: wave 0 holds all Nsym decisions -- ballots, lane j assembles byte j
template <int M>
__device__ __forceinline__ void pack_bits(const Stream &c, const FrameOut &o, int sym)
{
    const int tid = c.tid;
    if (tid >= kWave) return;
    const bool act = tid < NSYM;
    const unsigned long long mlo = __ballot(act && (sym & 1)), mhi = __ballot(act && (sym & 2));
    if (tid < o.frame_bytes) {
        unsigned byte = 0;
        if (M == 2) byte = __builtin_bitreverse32((unsigned)(mlo >> (8 * tid)) & 0xffu) >> 24;
        else {
            const unsigned h4 = (unsigned)(mhi >> (4 * tid)) & 0xfu, l4 = (unsigned)(mlo >> (4 * tid)) & 0xfu;
#pragma unroll
            for (int q = 0; q < 4; q++) byte |= (((h4 >> q) & 1u) << (7 - 2 * q)) | (((l4 >> q) & 1u) << (6 - 2 * q));
        }
        o.bits[tid] = (uint8_t)byte;
    }
}
// SNRest / EbNodB / snr_est / v_est / rx_*_pow: per-frame outputs and stream state that only the LAST frame of a call leaves behind
// (the wave kernels' rule): computed on observable frames, by wave 0 alone (it holds all Nsym decisions, thread 0 is the only one that
// writes them anywhere) -- no workgroup barrier
__device__ __forceinline__ void update_snr(Stream &c, SymbolSums s)
{
    if (c.tid >= kWave) return;
    s.sig = wave_sum(s.sig); s.nse = wave_sum(s.nse) + 1e-12f;
    s.mean_e = wave_sum(s.mean_e); s.std_e = wave_sum(s.std_e);
    StreamScalars sc;
    sc.snr_est = c.sc[SC_SNR_EST];
    update_snr(sc, s, NSYM);
    if (c.tid == 0) {
        c.sc[SC_SNREST] = sc.SNRest; c.sc[SC_SNR_EST] = sc.snr_est; c.sc[SC_EBNODB] = sc.EbNodB; c.sc[SC_V_EST] = sc.v_est;
        c.sc[SC_SIG_POW] = sc.rx_sig_pow; c.sc[SC_NSE_POW] = sc.rx_nse_pow;
    }
}
// the frame's tone estimates and stats row; with a NaN timing estimate (upstream returns before touching the outputs) zeroed bits and
// magnitudes and zero powers in the row (u8 input cannot reach that)
template <int M>
__device__ __forceinline__ void finish_frame(const Stream &c, const FrameOut &o, const Tones &tn, int nin_next, bool bad)
{
    const int tid = c.tid;
    if (bad) {
        // (not unrolled or interleaved: by 8, the index vectors of these loops were hoisted out of the frame loop and spilled)
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (int i = tid; i < o.frame_bytes; i += NT) if (o.bits) o.bits[i] = 0;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (int i = tid; i < M * NSYM; i += NT) if (o.filt) o.filt[i] = 0.f;
    }
#pragma unroll
    for (int m = 0; m < kMaxTones; m++) if (tid == 0) c.fest[m] = tn.f_est[m];
    if (o.stats && tid == 0)
        write_stats_row(o.stats, tn.f_est, c.norm_rx_timing, c.sc[SC_SNREST], nin_next, c.ppm, bad ? 0.f : c.sc[SC_SIG_POW], bad ? 0.f : c.sc[SC_NSE_POW]);
}

}  // namespace

// Compiled for three workgroups per CU: the 2-FSK instances hold 36 KB of LDS each and <= 168 VGPR, the 4-FSK ones 51 KB (tones two at a
// time in the correlator). Round 5: with the down-conversion folded into the running sums the 4-FSK peak instances need 156 VGPR (were 216)
// and run at three as well.
template <int M, int FMT, bool MASK>
__global__ __launch_bounds__(NT, 3) void fsk_demod_block_kernel(DemodArgs a_by_value)
{
    __shared__ DemodArgs s_args;            // read through stage_args() (Stream::args)
    constexpr int WORK_CF = XA_CF > M * (NSTEP + NINT) ? XA_CF : M * (NSTEP + NINT);
    __shared__ __attribute__((aligned(16))) float2 s_xa[WORK_CF];
    __shared__ __attribute__((aligned(16))) uint16_t s_tail[HIST + 4];
    __shared__ float s_red[16];
    __shared__ uint32_t s_dump[kWave];
    __shared__ uint32_t s_prev[2 * kMaxTones + 1];
    __shared__ float s_sc[SC_N];
    __shared__ float s_fest[kMaxTones];
    __shared__ __attribute__((aligned(16))) float2 s_twb[16 * 16];

    if (threadIdx.x == 0) s_args = a_by_value;
    __syncthreads();
    Stream c;
    c.args = &s_args;
    c.tail = s_tail; c.red = s_red; c.dump = s_dump; c.prev = s_prev; c.sc = s_sc; c.fest = s_fest; c.twb = s_twb;
    c.tid = threadIdx.x; c.sid = blockIdx.x;
    // One work array, in turn: the FFT exchanges (XA_CF), the linear spectrum (mask estimator), then the sums over the 16-sample window
    // steps [M][NSTEP] with f_int [M][NINT] behind them
    float2 *const xa = s_xa;
    float *const sfl = (float *)s_xa;
    float2 (*const step)[NSTEP] = (float2 (*)[NSTEP])s_xa;
    float2 (*const fint)[NINT] = (float2 (*)[NINT])(s_xa + M * NSTEP);

    if (!load_state<M>(c)) return;                         // (workgroup-uniform: the barrier is behind it)
    __syncthreads();
    open_call(c);
    stagger_start(c);
    while (c.frame < c.max_frames && c.pos + c.nin <= c.nsamp) {
        const PIRIP_GLOBAL uint16_t *gin = gl((const PIRIP_GLOBAL uint16_t *)(c.in_base + 2 * c.pos));   // this frame's samples (I, Q bytes)
        fft_frame<FMT>(c, gin, xa);
        Tones tn = {};
        if constexpr (MASK) slide_mask<M>(c, sfl, tn); else pick_peaks<M>(c, tn);
        __syncthreads();                                   // (the linear spectrum on the work array has been read)
        correlate<M, FMT, MASK>(c, gin, tn, step);
        __syncthreads();
        prefetch_next(c, gin);
        keep_tail<M>(c, gin, tn);
        float2 tc = window_sums<M>(c, step, fint);
        block_sum2(tc.x, tc.y, c.red, c.tid);

        const FrameOut o = frame_out<M>(c);
        const bool bad = isnan(tc.x) || isnan(tc.y);       // (the same on every thread)
        int nin_next = c.nin;
        if (!bad) {
            const Timing t = update_timing(c, tc);
            nin_next = t.nin_next;
            int sym;
            const SymbolSums s = decide_symbols<M>(c, t, o, fint, sym);
            if (o.bits && o.packed) pack_bits<M>(c, o, sym);
            const bool last_frame = (c.frame + 1 >= c.max_frames) || (c.pos + c.nin + nin_next > c.nsamp);
            if (o.stats || last_frame) update_snr(c, s);
        }
        finish_frame<M>(c, o, tn, nin_next, bad);
        c.have_frames = true;
        c.pos += c.nin;
        c.nin = nin_next;
        c.frame++;
        __syncthreads();
    }
    save_state<M>(c);
}

// ---- instances and dispatch ----------------------------------------------------------------------------------------------
namespace {
struct BlockInst { int M, fmt, mask; void (*kern)(DemodArgs); };
#define PIRIP_BLOCK_INST(M, FMT, MASK) {M, FMT, MASK, fsk_demod_block_kernel<M, FMT, MASK>}
const BlockInst kBlockInst[] = {
    PIRIP_BLOCK_INST(2, PIRIP_IN_CU8_CSDR, false), PIRIP_BLOCK_INST(2, PIRIP_IN_CU8_CSDR, true),           // rtl_fsk -r 1000
    PIRIP_BLOCK_INST(4, PIRIP_IN_CU8_CSDR, false), PIRIP_BLOCK_INST(4, PIRIP_IN_CU8_CSDR, true),           // ... -m 4 --mask 2000
    PIRIP_BLOCK_INST(2, PIRIP_IN_CU8_FSKDEMOD, false), PIRIP_BLOCK_INST(2, PIRIP_IN_CU8_FSKDEMOD, true),   // fsk_demod -d -p 15 on the same signal
    PIRIP_BLOCK_INST(4, PIRIP_IN_CU8_FSKDEMOD, false), PIRIP_BLOCK_INST(4, PIRIP_IN_CU8_FSKDEMOD, true),
};
#undef PIRIP_BLOCK_INST
const BlockInst *find_block(const FskDims &d)
{
    if (!d.recalled_fast_ok) return nullptr;            // (the instances carry the recalled constants' default values: pirip_fsk_recalled)
    if (d.Ts != TS || d.P != P || d.Nsym != NSYM || d.Ndft != NDFT || d.fft_fma || d.est_band) return nullptr;
    for (const BlockInst &b : kBlockInst)
        if (b.M == d.M && b.fmt == d.in_format && b.mask == (d.freq_est_type != 0)) return &b;
    return nullptr;
}
}  // namespace

bool demod_block_applicable(const FskDims &d) { return find_block(d) != nullptr; }

int demod_block_describe(const FskDims &d, char *buf, size_t n)
{
    const BlockInst *b = find_block(d);
    if (!b) return 0;
    return snprintf(buf, n, "fsk_demod_block_kernel<M=%d,Ts=%d,P=%d,Nsym=%d,Ndft=%d,%s,%s256 threads/stream>", b->M, TS, P, NSYM, NDFT,
                    b->fmt == PIRIP_IN_CU8_CSDR ? "u8 csdr" : "u8 -d", b->mask ? "mask estimator," : "");
}

hipError_t launch_demod_block(const DemodArgs &a, int nstreams, hipStream_t stream)
{
    const BlockInst *b = find_block(a.d);
    if (!b) return hipErrorNotSupported;
    hipLaunchKernelGGL(b->kern, dim3(nstreams), dim3(NT), 0, stream, a);
    return hipGetLastError();
}

}  // namespace pirip
