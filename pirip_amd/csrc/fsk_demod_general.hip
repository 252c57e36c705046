// pirip_amd/csrc/fsk_demod_general.hip -- general-configuration FSK demodulator kernel (gfx950).
//
// One workgroup (64-256 lanes) owns one IQ stream and walks its frames in order, because codec2's
// demodulator is frame-serial: nin, the smoothed spectrum Sf, the tone estimates, the local
// oscillator phases and the integrator memory all chain from frame to frame
// [UPSTREAM-RECALLED codec2 fsk.c: fsk_demod_freq_est + fsk_demod_core; SURVEY.md 8a rows
//  a-1, a-4 ... a-8]. Parallelism comes from the batch of independent streams (one workgroup of two
// waves each, the read-only tables shared through L1/L2) and from the 128 lanes inside a frame.
// All per-frame intermediates (raw samples, FFT work array, grouped f_dc of the tone in hand,
// f_int) live in LDS; HBM sees the u8/s16 IQ stream once and the bits. Occupancy is LDS-bound at
// one wave per SIMD, so every loop issues its LDS reads in batches of four before the arithmetic
// and the next frame's input is read into registers a frame ahead. Per-frame cycle split measured
// with s_memtime (config 3, 1024-point FFTs): estimator 45 %, down-conversion + windows 38 %,
// staging 7 %, peak pick 4 %, timing 4 %, decisions 2 %.
//
// This kernel handles every configuration fsk_create_hbr() accepts (M in {2,4}, any Ts/P/Nsym,
// power-of-two Ndft, peak or mask estimator, four input formats). The specialised kernel in
// fsk_demod_wave.hip overtakes it for the reference's main command lines; this one stays as the
// on-device cross-check and as the path for every other configuration.
//
// Numerics contract (DESIGN.md "parity"): the frequency-estimator path (conversion, Hann,
// FFT butterflies, |X|, IIR, peak pick) performs the same float32 operations in the same
// order as the CPU restatement, so Sf and f_est are bit-identical; compiled with
// -ffp-contract=off so no multiply-add is fused behind our back. The down-conversion
// oscillator is NOT the upstream recursion (a 1200-step serial chain per tone): phases come
// from a 32-bit phase accumulator and the FFT twiddle table, so f_dc / f_int / rx_filt agree
// with the oracle to rounding (stated tolerance 1e-4 of the frame's peak magnitude), and the
// hard bits agree exactly wherever the decision margin exceeds that.
#include <hip/hip_runtime.h>
#include <cmath>

#include "../../include/pirip_hip.h"
#include "demod_frame.hpp"
#include "demod_simd.hpp"
#include "fsk_device.hpp"
#include "glibc_atan2f.hpp"

namespace pirip {

namespace {

constexpr int kWave = 64;
constexpr int kU = 2;   // independent items per thread per pass in the batched loops (reads first, then arithmetic)

// wave_sum (demod_simd.hpp) as one asm statement: the same additions in the same order, but v_add_f32_dpp on the partial sum itself
// (lanes whose DPP source is outside the row / masked keep their own partial sum: the row_shr steps build inclusive prefix sums inside
// each row of 16, the broadcasts add the preceding rows' totals -- lane 63 holds the wave total)
__device__ __forceinline__ float wave_sum_asm(float v)
{
    int tot;
    asm(PIRIP_DPP_REDUCE("v_add_f32_dpp") : "+v"(v), "=s"(tot));
    return __builtin_bit_cast(float, tot);
}

// LDS, per stream (= per workgroup; the read-only tables -- twiddles, Hann, digit-reversal -- are read from
// global memory and live in L1/L2). Kept small so several streams fit a CU: the input
// stays in its raw form for the u8 / s16 formats (converted where it is used -- all three conversions are
// exact in one to three FMAs), the peak-picking work copy of Sf aliases the FFT work array, and the
// down-converted samples are held for ONE tone at a time, summed in groups (tones are processed in sequence;
// only their last hist_len samples persist).
struct Lds {
    void *in;        // [nin_max]  raw input samples: float2, short2 or uchar2 (one dummy slot for direct input)
    float2 *X;       // [Ndft]     FFT work array; Sfw (float [Ndft]) and the step sums alias it
    float *Sf;       // [Ndft]
    float2 *fdc;     // [Nmem/grp] down-converted samples of the tone being processed, summed in groups of grp
    float2 *hist;    // [M][hist_len/grp] last entries of every tone's fdc (carried between frames)
    float2 *fint;    // [M][nint]
};

__host__ __device__ inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// Long frames of 8-bit samples (Ts = 240: 24 KB per frame) are not staged: the estimator and every tone's down-conversion read them
// from global memory (L2: the frame is read 2 + M times) -- with the 24 KB and the aliasing below two streams fit a CU instead of one.
__host__ __device__ inline bool direct_input(const FskDims &d)
{
    const bool u8 = d.in_format == PIRIP_IN_CU8_FSKDEMOD || d.in_format == PIRIP_IN_CU8_CSDR;
    return u8 && (size_t)(d.N + d.nin_step) * sizeof(uchar2) > 16384;
}

__host__ __device__ inline size_t carve(const FskDims &d, Lds *l, char *base)
{
    size_t off = 0;
    const int nin_max = d.N + d.nin_step;
    const bool u8 = d.in_format == PIRIP_IN_CU8_FSKDEMOD || d.in_format == PIRIP_IN_CU8_CSDR;
    auto take = [&](size_t bytes) { size_t o = off; off = align16(off + bytes); return o; };
    size_t o_in = take(direct_input(d) ? 16 : (u8 ? sizeof(uchar2) : d.in_format == PIRIP_IN_CS16 ? sizeof(short2) : sizeof(float2)) * nin_max);
    // X also stages packed bits (Nbits bytes)
    size_t xbytes = sizeof(float2) * d.Ndft;
    if (xbytes < (size_t)d.Nbits) xbytes = d.Nbits;
    size_t o_X = take(xbytes);
    size_t o_Sf = take(sizeof(float) * d.Ndft);
    // the down-converted samples of the tone in hand live in the FFT work array when they fit (the estimator is done with it by then,
    // the bit staging comes after the last tone)
    const size_t fdc_bytes = sizeof(float2) * (d.Nmem / d.grp);
    size_t o_fdc = fdc_bytes <= xbytes ? o_X : take(fdc_bytes);
    size_t o_hist = take(sizeof(float2) * d.M * (d.hist_len / d.grp));
    size_t o_fint = take(sizeof(float2) * d.M * d.nint);
    if (l) {
        l->in = base + o_in; l->X = (float2 *)(base + o_X); l->Sf = (float *)(base + o_Sf); l->fdc = (float2 *)(base + o_fdc);
        l->hist = (float2 *)(base + o_hist); l->fint = (float2 *)(base + o_fint);
    }
    return off;
}

// exp(+j theta), theta in 2^-32 turns: top log2(Ndft) bits index the twiddle table
// (tw[k] = exp(-j 2 pi k/Ndft)), the remainder is a small-angle rotation.
__device__ __forceinline__ float2 phasor(uint32_t theta, const float2 *tw, int log2n)
{
    const uint32_t idx = theta >> (32 - log2n);
    const uint32_t low = theta & ((1u << (32 - log2n)) - 1u);
    float2 w = tw[idx];
    float c = w.x, s = -w.y;
    if (low) {
        const float b = (float)low * 1.4629180792671596e-9f;   // 2*pi / 2^32
        const float b2 = b * b;
        const float cb = 1.0f - b2 * (0.5f - b2 * (1.0f / 24.0f));
        const float sb = b * (1.0f - b2 * ((1.0f / 6.0f) - b2 * (1.0f / 120.0f)));
        const float c2 = c * cb - s * sb;
        const float s2 = s * cb + c * sb;
        c = c2; s = s2;
    }
    return make_float2(c, s);
}

// One FFT stage over the LDS work array, U butterflies per lane per pass: all reads of the pass are issued
// before the arithmetic and all writes after it, so a lone wave on its SIMD overlaps the LDS round trips
// (butterflies of a stage touch disjoint slots). Arithmetic and its order are kiss_fft's kf_bfly4 (R = 4) / kf_bfly2 (R = 2) in
// demod_simd.hpp's one statement of them (cmul_x, bfly4; radix 2 is cmul_x and a packed subtract and add): each product and sum rounded once.
template <int R, int U>
__device__ __forceinline__ void fft_stage(v2f *X, const v2f *tw, int m, int fs, int nb, int tid, int NT)
{
    const int sh = 31 - __clz(m);
    for (int b0 = tid; b0 < nb; b0 += U * NT) {
        v2f f[U][R], t[U][R];
        v2f *F[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int b = (b0 + u * NT < nb) ? b0 + u * NT : b0;
            const int g = b >> sh, k = b - (g << sh);
            F[u] = X + ((g * R) << sh) + k;
#pragma unroll
            for (int r = 1; r < R; r++) t[u][r] = tw[r * k * fs];
#pragma unroll
            for (int r = 0; r < R; r++) f[u][r] = F[u][r * m];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
#pragma unroll
            for (int r = 1; r < R; r++) f[u][r] = cmul_x(f[u][r], t[u][r]);
            if constexpr (R == 4) bfly4(f[u][0], f[u][1], f[u][2], f[u][3]);
            else { const v2f s = f[u][1]; f[u][1] = f[u][0] - s; f[u][0] = f[u][0] + s; }
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            if (u == 0 || b0 + u * NT < nb) {
#pragma unroll
                for (int r = 0; r < R; r++) F[u][r * m] = f[u][r];
            }
    }
}

// Workgroup reductions (one stream = one workgroup of NT/64 waves): wave step on the VALU, then <= kMaxWaves partials
// through LDS. Every thread gets the same result. red points at 2 * kMaxWaves words of LDS scratch.
constexpr int kMaxWaves = 16;
constexpr int kRedBytes = 2 * kMaxWaves * 4;
__device__ __forceinline__ float block_sum(float v, float *red, int tid, int NT)
{
    v = wave_sum_asm(v);
    if (NT == kWave) return v;
    __syncthreads();
    if ((tid & (kWave - 1)) == 0) red[tid >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < (NT >> 6); w++) r += red[w];
    return r;
}
__device__ __forceinline__ void block_argmax(float &v, int &idx, float *red, int tid, int NT)
{
    wave_argmax(v, idx);
    if (NT == kWave) return;
    __syncthreads();
    if ((tid & (kWave - 1)) == 0) { red[tid >> 6] = v; ((int *)red)[kMaxWaves + (tid >> 6)] = idx; }
    __syncthreads();
    v = red[0]; idx = ((int *)red)[kMaxWaves];
    for (int w = 1; w < (NT >> 6); w++) {
        const float ov = red[w]; const int oi = ((int *)red)[kMaxWaves + w];
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
}

// ---- per-stream context ------------------------------------------------------------------------------------------------------------
// The sample reader: sample i of the frame in hand as complex float, converted from where its format keeps it.
struct SampleReader {
    const FskDims &d;
    const float *lut;          // a -d map other than the recalled (x - 127) / 128: the plan's table (d.u8_table)
    void *lds;                 // the staged frame, raw (Lds::in)
    const uchar2 *gin8;        // direct input: this frame's samples in global memory
    const uint8_t *base;       // the stream's (segment's) first sample: nsamp samples of bps bytes
    int64_t nsamp;
    int bps;
    bool u8, s16, direct;
    // exact u8 -> float, fma(x, lo, fma(x, hi, c)) with cvt_u8_pair's constants (demod_simd.hpp): fsk_demod -d is (x - 127)/128, csdr
    // convert_u8_f is x/127.5 - 1 (double, rounded) with hi a multiple of 2^-22 (see decim_kernels.hip)
    float hi, lo, c;
    __device__ __forceinline__ float2 operator()(int i) const
    {
        if (u8) {
            const uchar2 v = direct ? gin8[i] : ((const uchar2 *)lds)[i];
            if (d.u8_table) return make_float2(lut[v.x], lut[v.y]);
            const float xr = (float)v.x, xi = (float)v.y;
            return make_float2(__builtin_fmaf(xr, lo, __builtin_fmaf(xr, hi, c)), __builtin_fmaf(xi, lo, __builtin_fmaf(xi, hi, c)));
        }
        if (s16) {
            // x / FDMDV_SCALE, correctly rounded, without the divide: q = x*r, then one Newton step on the residual; equal to the IEEE
            // quotient for every int16 value (checked exhaustively, tests/: the divisor is plan data, 750 as recalled; checked for 750 and 1000)
            const short2 v = ((const short2 *)lds)[i];
            const float xr = (float)v.x, xi = (float)v.y, r = 1.0f / d.s16_scale;
            float qr = xr * r, qi = xi * r;
            qr = __builtin_fmaf(__builtin_fmaf(-d.s16_scale, qr, xr), r, qr);
            qi = __builtin_fmaf(__builtin_fmaf(-d.s16_scale, qi, xi), r, qi);
            return make_float2(qr, qi);
        }
        return ((const float2 *)lds)[i];
    }
};

// One workgroup (NT = 64..512 threads) per stream: all its waves run the same frame loop and meet at workgroup barriers. This is what a
// stage sees of its stream. The per-tone arrays stay in registers because every stage is force-inlined and indexes them inside loops
// unrolled over kMaxTones and guarded by m < M (with a run-time trip count they would live in scratch memory).
struct Stream {
    const DemodArgs &a;
    SampleReader sample;
    Lds L;
    float *red;                // 2 * kMaxWaves words of reduction scratch
    int tid, NT, sid;
    int log2n, G, hist_g, ng;  // integrator memory is kept as sums over groups of G samples: hist_g / ng entries of history / of a frame
    StreamScalars sc;
    uint32_t theta[kMaxTones]; // oscillator phase of every tone, 2^32 = one turn
    float2 phc[kMaxTones];     // oracle order, every frame: phi_c of every tone, carried frame to frame by thread 0
};
struct FrameOut { uint8_t *bits; float *filt; float *stats; int frame_bytes; };                  // a frame's output rows (nullptr: not requested)

__device__ __forceinline__ void open_stream(Stream &c, char *smem, int64_t seg_in)
{
    const FskDims &d = c.a.d;
    SampleReader &in = c.sample;
    c.red = (float *)smem;
    carve(d, &c.L, smem + kRedBytes);
    c.tid = threadIdx.x; c.NT = blockDim.x; c.sid = blockIdx.x;
    c.log2n = 31 - __clz(d.Ndft); c.G = d.grp; c.hist_g = d.hist_len / d.grp; c.ng = d.Nmem / d.grp;
    const bool dmap = d.in_format == PIRIP_IN_CU8_FSKDEMOD;
    in.u8 = dmap || d.in_format == PIRIP_IN_CU8_CSDR; in.s16 = d.in_format == PIRIP_IN_CS16; in.direct = direct_input(d);
    in.hi = dmap ? kU8dHi : kCsdrHi; in.lo = dmap ? kU8dLo : kCsdrLo; in.c = dmap ? kU8dC : kCsdrC;
    in.lds = c.L.in; in.gin8 = nullptr; in.bps = in.u8 ? 2 : in.s16 ? 4 : 8;
    in.base = c.a.io.in + (size_t)c.sid * c.a.io.in_stride + (size_t)seg_in * in.bps;
    in.nsamp = c.a.io.nsamp - seg_in;
}

// ---- stream state: HBM <-> LDS and registers -------------------------------------------------------------------------------------------
// CREATED (the prologue): a created stream's integrator memory and phases are zero, whatever layout the handle's kernel keeps there
template <bool CREATED>
__device__ __forceinline__ void load_state(Stream &c)
{
    const FskDims &d = c.a.d;
    for (int i = c.tid; i < d.Ndft; i += c.NT) c.L.Sf[i] = c.a.s.Sf[(size_t)c.sid * d.Ndft + i];
    for (int m = 0; m < d.M; m++)
        for (int h = c.tid; h < c.hist_g; h += c.NT)
            c.L.hist[m * c.hist_g + h] = CREATED ? make_float2(0.f, 0.f) : c.a.s.hist[((size_t)c.sid * d.M + m) * d.hist_len + h];
    c.sc = c.a.s.scal[c.sid];
#pragma unroll
    for (int m = 0; m < kMaxTones; m++) c.theta[m] = CREATED ? 0u : c.a.s.theta[(size_t)c.sid * kMaxTones + m];
    __syncthreads();
}
// the general layout
__device__ __forceinline__ void save_state(Stream &c)
{
    const FskDims &d = c.a.d;
    for (int m = 0; m < d.M; m++)
        for (int h = c.tid; h < c.hist_g; h += c.NT) c.a.s.hist[((size_t)c.sid * d.M + m) * d.hist_len + h] = c.L.hist[m * c.hist_g + h];
    if (c.tid == 0) for (int m = 0; m < kMaxTones; m++) c.a.s.theta[(size_t)c.sid * kMaxTones + m] = c.theta[m];
}
// The wave kernel's state block (fsk_demod_wave.hip, WaveCfg) as the prologue leaves it after its frame of `pos` samples: the guard area
// as it stands after a frame -- the frame's last 2 Ts + Ts/4 RAW samples right-aligned in GUARD_B bytes -- then per tone the phase step
// and oscillator-table row of the frame's tone estimates, then the frame's nin. (The wave kernel carries no oscillator phase: its
// handles' theta words stay as reset left them -- capture.hip compares whole states.)
__device__ __forceinline__ void save_state_wave(Stream &c, const Tones &tn, int64_t pos)
{
    const FskDims &d = c.a.d;
    const int M = d.M, bps = c.sample.bps, HIST = 2 * d.Ts + d.nin_step;
    const int guard_b = ((HIST * bps + 15) / 16) * 16, tail_b = HIST * bps;
    uint32_t *st32 = (uint32_t *)(c.a.s.hist + (size_t)c.sid * M * d.hist_len);
    const uint8_t *src = c.sample.base + (size_t)(pos - HIST) * bps;           // (byte copy: a stream's base need not be dword-aligned)
    for (int i = c.tid; i < tail_b; i += c.NT) ((uint8_t *)st32)[guard_b - tail_b + i] = src[i];
    // (the guard's padding in front of the tail holds what the wave kernel fills a created stream's guard with: its format's
    //  neutral sample -- capture.hip compares whole state blocks)
    const uint8_t neutral = d.in_format == PIRIP_IN_CU8_FSKDEMOD ? 0x7F : d.in_format == PIRIP_IN_CU8_CSDR ? 0x80 : 0x00;
    for (int i = c.tid; i < guard_b - tail_b; i += c.NT) ((uint8_t *)st32)[i] = neutral;
    if (c.tid == 0) {
#pragma unroll
        for (int m = 0; m < kMaxTones; m++) if (m < M) { st32[guard_b / 4 + m] = tn.dtheta[m]; st32[guard_b / 4 + M + m] = (uint32_t)tn.drift_ix[m]; }
        st32[guard_b / 4 + 2 * M] = (uint32_t)(pos);                 // = nin of the frame (pos counts from 0)
    }
}

// ---- a-1: nin samples of the frame into LDS, raw ---------------------------------------------------------------------------------------
// The u8 / s16 input of the NEXT frame is requested into registers right after this frame's input has landed in LDS (nin_max samples
// from pos + nin: the next nin is not known yet) and written to LDS at the top of the next iteration, so the HBM round trip is covered
// by a whole frame of work. f32 input, or frames longer than kPre * NT samples, are staged synchronously (eight loads per lane in
// flight); direct input is not staged at all.
constexpr int kPre = 12;                                  // input read-ahead registers per thread (12 x NT samples)
struct ReadAhead { bool can_pre, have_pre; uint32_t pre[kPre]; };

__device__ __forceinline__ void stage_input(Stream &c, ReadAhead &ra, int64_t pos, int nin)
{
    const int tid = c.tid, NT = c.NT, nin_max = c.a.d.N + c.a.d.nin_step;
    SampleReader &in = c.sample;
    auto stage = [&](auto *dst, const auto *src) {
        for (int i0 = tid; i0 < nin; i0 += 8 * NT) {
            decltype(src[0] + src[0]) v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { const int i = i0 + u * NT; v[u] = src[i < nin ? i : nin - 1]; }
#pragma unroll
            for (int u = 0; u < 8; u++) { const int i = i0 + u * NT; if (i < nin) dst[i] = v[u]; }
        }
    };
    if (in.direct) in.gin8 = (const uchar2 *)(in.base + 2 * pos);
    else if (ra.have_pre) {
#pragma unroll
        for (int u = 0; u < kPre; u++) {
            const int i = tid + u * NT;
            if (i < nin) { if (in.u8) ((uint16_t *)in.lds)[i] = (uint16_t)ra.pre[u]; else ((uint32_t *)in.lds)[i] = ra.pre[u]; }
        }
    } else if (in.u8) stage((uint16_t *)in.lds, (const uint16_t *)(in.base + 2 * pos));
    else if (in.s16) stage((uint32_t *)in.lds, (const uint32_t *)((const short2 *)in.base + pos));
    else stage((double *)in.lds, (const double *)((const float2 *)in.base + pos));
    __syncthreads();
    if (ra.can_pre) {
#pragma unroll
        for (int u = 0; u < kPre; u++) {
            if (u * NT < nin_max) {                     // wave-uniform
                const int64_t p1 = pos + nin + tid + u * NT, gi = p1 < in.nsamp ? p1 : in.nsamp - 1;
                ra.pre[u] = in.u8 ? (uint32_t)((const uint16_t *)in.base)[gi] : ((const uint32_t *)in.base)[gi];
            }
        }
        ra.have_pre = true;
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- a-5: frequency estimator ----------------------------------------------------------------------------------------------------------
// Half-overlapped Hann-windowed FFTs of the frame in the work array X, each folded into the smoothed spectrum Sf.
// (loops below: kU independent items per thread per pass, reads first -- see fft_stage)
__device__ __forceinline__ void smooth_spectrum(Stream &c, int nin, float2 *X)
{
    const DemodArgs &a = c.a;
    const FskDims &d = a.d;
    const int tid = c.tid, NT = c.NT, Ndft = d.Ndft, numffts = nin / (Ndft / 2) - 1;
    const float2 *__restrict__ g_tw = a.t.tw;
    const float *__restrict__ g_hann = a.t.hann;
    const uint16_t *__restrict__ g_perm = a.t.perm;
    for (int j = 0; j < numffts; j++) {
        const int off = j * Ndft / 2;
        for (int i0 = tid; i0 < Ndft; i0 += kU * NT) {   // natural order in, digit-reversed slot out
            float h[kU]; float2 x[kU]; int dst[kU];
#pragma unroll
            for (int u = 0; u < kU; u++) {
                const int i = (i0 + u * NT < Ndft) ? i0 + u * NT : i0;
                h[u] = g_hann[i]; x[u] = c.sample(off + i); dst[u] = g_perm[i];
            }
#pragma unroll
            for (int u = 0; u < kU; u++)
                if (u == 0 || i0 + u * NT < Ndft) X[dst[u]] = make_float2(h[u] * x[u].x, h[u] * x[u].y);
        }
        __syncthreads();
        for (int s = 0; s < d.nstages; s++) {
            const int p = a.stages[s].radix, m = a.stages[s].m, fs = a.stages[s].fstride, nb = Ndft / p;
            v2f *Xv = (v2f *)X; const v2f *tw = (const v2f *)g_tw;
            if (p == 4) { if (nb >= kU * NT) fft_stage<4, kU>(Xv, tw, m, fs, nb, tid, NT); else fft_stage<4, 1>(Xv, tw, m, fs, nb, tid, NT); }
            else { if (nb >= kU * NT) fft_stage<2, kU>(Xv, tw, m, fs, nb, tid, NT); else fft_stage<2, 1>(Xv, tw, m, fs, nb, tid, NT); }
            __syncthreads();
        }
        // fftshift + |X| + first-order smoothing
        for (int i0 = tid; i0 < Ndft; i0 += kU * NT) {
            float2 x[kU]; float sf[kU];
#pragma unroll
            for (int u = 0; u < kU; u++) {
                const int i = (i0 + u * NT < Ndft) ? i0 + u * NT : i0;
                x[u] = X[(i + Ndft / 2) & (Ndft - 1)]; sf[u] = c.L.Sf[i];
            }
#pragma unroll
            for (int u = 0; u < kU; u++) {
                const float mag2 = (x[u].x * x[u].x) + (x[u].y * x[u].y);
                if (u == 0 || i0 + u * NT < Ndft) c.L.Sf[i0 + u * NT] = (sf[u] * d.one_minus_tc) + ((d.sf_power ? mag2 : sqrtf(mag2)) * d.tc);
            }
        }
        __syncthreads();
    }
}
// peak method: the M largest bins of Sf, each with its neighbourhood zeroed before the next is sought, then in ascending order.
// Sfw: work copy of Sf (on X, which the FFTs are done with).
__device__ __forceinline__ void pick_peaks(Stream &c, float *Sfw, int (&freqi)[kMaxTones])
{
    const FskDims &d = c.a.d;
    const int tid = c.tid, NT = c.NT, M = d.M, Ndft = d.Ndft;
    for (int i = tid; i < Ndft; i += NT) Sfw[i] = c.L.Sf[i];
    __syncthreads();
#pragma unroll
    for (int m = 0; m < kMaxTones; m++) if (m < M) {
        float best = 0.0f; int ib = 0;
        for (int j = d.est_st + tid; j < d.est_en; j += NT) {
            const float v = Sfw[j];
            if (v > best) { best = v; ib = j; }
        }
        block_argmax(best, ib, c.red, tid, NT);
        int f_min = ib - d.f_zero; f_min = f_min < 0 ? 0 : f_min;
        int f_max = ib + d.f_zero; f_max = f_max > Ndft ? Ndft : f_max;
        __syncthreads();
        for (int j = f_min + tid; j < f_max; j += NT) Sfw[j] = 0.0f;
        __syncthreads();
        freqi[m] = ib - Ndft / 2;
    }
    // ascending sort of M <= 4 indices (insertion sort, fully unrolled)
#pragma unroll
    for (int x = 1; x < kMaxTones; x++)
#pragma unroll
        for (int y = x; y > 0; y--)
            if (x < M && freqi[y] < freqi[y - 1]) { const int t = freqi[y]; freqi[y] = freqi[y - 1]; freqi[y - 1] = t; }
}
// mask method: comb of 3-bin teeth slid over Sf, tooth sums in ascending order; the tones follow from the comb's position
__device__ __forceinline__ void slide_mask(Stream &c, Tones &tn)
{
    const DemodArgs &a = c.a;
    const FskDims &d = a.d;
    const int M = d.M, Ndft = d.Ndft;
    float best = 0.0f; int bb = d.est_st;
    for (int b = d.est_st + c.tid; b < d.est_en - d.mask_len; b += c.NT) {
        float corr = 0.0f;
        for (int k = 0; k < d.n_teeth; k++) corr += c.L.Sf[b + a.t.teeth[k]];
        if (corr > best) { best = corr; bb = b; }
    }
    // lanes that found nothing keep (0, est_st): smallest index wins ties, as upstream
    block_argmax(best, bb, c.red, c.tid, c.NT);
    const float foff = (float)((bb - Ndft / 2) * d.Fs / Ndft);
#pragma unroll
    for (int m = 0; m < kMaxTones; m++) if (m < M) {
        tn.f_est[m] = foff + (float)(m * d.tone_spacing); tn.dtheta[m] = a.t.mask_dtheta[bb * M + m]; tn.drift_ix[m] = bb * M + m;
    }
}
// X: the FFT work array, then the peak picker's work copy of Sf (Sfw on X)
__device__ __forceinline__ void estimate_tones(Stream &c, int nin, float2 *X, Tones &tn)
{
    const FskDims &d = c.a.d;
    smooth_spectrum(c, nin, X);
    int freqi[kMaxTones];
    pick_peaks(c, (float *)X, freqi);        // (always run: f_est is reported even when the mask method drives the demod)
#pragma unroll
    for (int m = 0; m < kMaxTones; m++) {
        const bool on = m < d.M;
        tn.f_est[m] = on ? (float)freqi[m] * d.bin_hz : 0.f;
        tn.dtheta[m] = on ? (uint32_t)freqi[m] << (32 - c.log2n) : 0u;
        tn.drift_ix[m] = on ? freqi[m] + d.Ndft / 2 : 0;
    }
    if (d.freq_est_type) slide_mask(c, tn);
}

// ---- a-6: shift integrator memory, down-convert, integrate -- one tone at a time -------------------------------------------------------
// The last nold samples of the previous frame come back from hist into fdc, the new samples are down-converted behind them, the tail
// is saved for the next frame, then the windows are summed. Integrator memory is kept as sums over groups of G samples (G = Ts/P when
// the frame shifts are whole groups, else 1): window i = P (or Ts) consecutive entries.
__device__ __forceinline__ void recall_history(Stream &c, int m, int nold_g, float2 *fdc)
{
    for (int i = c.tid; i < nold_g; i += c.NT) fdc[i] = c.L.hist[m * c.hist_g + c.hist_g - nold_g + i];
}
// A lane down-converts a run of consecutive samples: one table phasor at the run start, then the upstream's own rounded per-sample
// multiplier. upstream advances phi_c by a float32-rounded multiplier, so |phi_c| drifts as (1+a)^n inside a frame (renormalised at its
// end): track that gain to first order.
__device__ __forceinline__ void downconvert_tone(Stream &c, uint32_t th0, uint32_t dth, int drift_ix, int nin, int nold, float2 *fdc)
{
    const int tid = c.tid, NT = c.NT, G = c.G, nold_g = nold / G;
    const float2 *__restrict__ g_tw = c.a.t.tw;
    const float gain_slope = c.a.t.osc_drift[drift_ix].x;
    const float2 rot = c.a.t.osc_step[drift_ix];
    const int run = G > 1 ? G : (nin + NT - 1) / NT;   // samples per lane run (G: one stored entry per run)
    for (int j0 = tid * run; j0 < nin; j0 += NT * run) {
        float2 ph = phasor(th0 + (uint32_t)(j0 + 1) * dth, g_tw, c.log2n);
        float2 acc = make_float2(0.f, 0.f);
        const int j1 = (j0 + run < nin) ? j0 + run : nin;
        const float g = 1.0f + gain_slope * (float)(j0 + 1);   // drift up to the run start; the recursion adds its own
        for (int jb = j0; jb < j1; jb += 4) {
            float2 xs[4];
#pragma unroll
            for (int u = 0; u < 4; u++) xs[u] = c.sample(jb + u < j1 ? jb + u : j1 - 1);   // reads first
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = jb + u;
                if (j < j1) {
                    const float2 x = xs[u];
                    const float2 y = make_float2((x.x * ph.x + x.y * ph.y) * g, (x.y * ph.x - x.x * ph.y) * g);
                    if (G > 1) { acc.x += y.x; acc.y += y.y; }
                    else fdc[nold + j] = y;
                    const float2 nph = make_float2(ph.x * rot.x - ph.y * rot.y, ph.x * rot.y + ph.y * rot.x);
                    ph = nph;
                }
            }
        }
        if (G > 1) fdc[nold_g + j0 / G] = acc;
    }
}
// Oracle order [fsk_oracle.c:316-320]: phi_c[m] = cmult(phi_c[m], dphi_m); f_dc = cmult(in, cconj(phi_c[m])) -- one thread, sample by
// sample (G == 1 here: demod_exact0_applicable). CARRY: phi_c continues from the previous frame and is handed on normalised (every frame
// exact); without it phi_c starts at (1, 0): the prologue only runs on a stream in its created state.
template <bool CARRY>
__device__ __forceinline__ void downconvert_tone_serial(Stream &c, float2 &phi_c, int drift_ix, int nin, int nold, float2 *fdc)
{
    if (c.tid != 0) return;                           // (no barrier in here)
    const float2 rot = c.a.t.osc_step[drift_ix];
    float2 ph = CARRY ? phi_c : make_float2(1.0f, 0.0f);
    if (CARRY && ph.x == 0.0f && ph.y == 0.0f) ph = make_float2(1.0f, 0.0f);    // the created state (a normalised phasor is never 0)
    for (int j = 0; j < nin; j++) {
        const float2 np = make_float2((ph.x * rot.x) - (ph.y * rot.y), (ph.x * rot.y) + (ph.y * rot.x));
        ph = np;
        const float2 x = c.sample(j);
        const float ci = -ph.y;                       // cconj
        fdc[nold + j] = make_float2((x.x * ph.x) - (x.y * ci), (x.x * ci) + (x.y * ph.x));
    }
    if (CARRY) {                                      // phi_c[m] = comp_normalize(phi_c[m]), carried to the next frame
        const float av = sqrtf((ph.x * ph.x) + (ph.y * ph.y));
        phi_c = make_float2(ph.x / av, ph.y / av);
    }
}
// fdc complete (barrier): its tail into hist for the next frame, its windows into fint; fdc is free again on return (barrier)
__device__ __forceinline__ void integrate_tone(Stream &c, int m, const float2 *fdc)
{
    const FskDims &d = c.a.d;
    const int nint = d.nint, per_win = d.Ts / c.G, win_step = (d.Ts / d.P) / c.G;
    __syncthreads();
    for (int h = c.tid; h < c.hist_g; h += c.NT) c.L.hist[m * c.hist_g + h] = fdc[c.ng - c.hist_g + h];
    for (int i = c.tid; i < nint; i += c.NT) {
        const float2 *src = fdc + i * win_step;
        float2 acc = make_float2(0.f, 0.f);
        for (int q = 0; q < per_win; q++) { acc.x += src[q].x; acc.y += src[q].y; }
        c.L.fint[m * nint + i] = acc;
    }
    __syncthreads();
}

// ---- a-7: fine timing ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float window_power(const Stream &c, int i)   // window i's power over all tones
{
    float ft1 = 0.f;
    for (int m = 0; m < c.a.d.M; m++) {
        const float2 v = c.L.fint[m * c.a.d.nint + i];
        ft1 += (v.x * v.x) + (v.y * v.y);
    }
    return ft1;
}
// t_c = sum of window power x the upstream recursion's timing phasor (drift included): per-thread partial sums, workgroup reduction
__device__ __forceinline__ float2 timing_sum(Stream &c)
{
    float tcr = 0.f, tci = 0.f;
    for (int i = c.tid; i < c.a.d.nint; i += c.NT) {
        const float ft1 = window_power(c, i);
        const float2 ph = c.a.t.timing_rec[i];
        tcr += ft1 * ph.x; tci += ft1 * ph.y;
    }
    tcr = block_sum(tcr, c.red, c.tid, c.NT); tci = block_sum(tci, c.red, c.tid, c.NT);
    return make_float2(tcr, tci);
}
// Oracle order [fsk_oracle.c:338-348]: ft1 per window in parallel (same operations), the accumulation t_c += ft1 * phi_ft serially in
// window order. ft1s: nint floats of scratch.
__device__ __forceinline__ float2 timing_sum_serial(Stream &c, float *ft1s)
{
    const int nint = c.a.d.nint;
    __syncthreads();
    for (int i = c.tid; i < nint; i += c.NT) ft1s[i] = window_power(c, i);
    __syncthreads();
    if (c.tid == 0) {
        float tr = 0.f, ti = 0.f;
        for (int i = 0; i < nint; i++) {
            const float2 ph = c.a.t.timing_rec[i];
            tr = tr + (ft1s[i] * ph.x); ti = ti + (ft1s[i] * ph.y);
        }
        c.red[0] = tr; c.red[1] = ti;
    }
    __syncthreads();
    const float2 tc = make_float2(c.red[0], c.red[1]);
    __syncthreads();
    return tc;
}
// norm_rx_timing = atan2f(t_c.imag, t_c.real) / (2 pi). Single precision, as in the wave kernel: codec2 divides by 2 pi and smooths ppm
// in double; the results differ by at most an ulp, far inside what the summation order already moves them, and double-precision code in
// this once-per-frame block costs registers for the whole kernel. Oracle order: as C evaluates it -- glibc's atan2f, the division in double.
__device__ __forceinline__ float timing_angle(float2 tc) { return atan2f(tc.y, tc.x) * 0.15915494309189535f; }
__device__ __forceinline__ float timing_angle_oracle(float2 tc) { return (float)((double)glibc_atan2f(tc.y, tc.x) / (2 * 3.14159265358979323846)); }

// The timing estimate into the stream's scalars, ppm smoothing included, and what follows from it: the next frame's nin and where the
// symbols are sampled. DOUBLE_PPM [fsk_oracle.c]: appm = 1e6 * d / (float)nsym; ppm = .9 * ppm + .1 * appm: double arithmetic, float stores
template <bool DOUBLE_PPM>
__device__ __forceinline__ Timing update_timing(Stream &c, float norm_rx_timing)
{
    const FskDims &d = c.a.d;
    StreamScalars &sc = c.sc;
    const float rx_timing = norm_rx_timing * (float)d.P, d_norm = norm_rx_timing - sc.norm_rx_timing;
    sc.norm_rx_timing = norm_rx_timing;
    if (fabsf(d_norm) < 0.2f) {
        if (DOUBLE_PPM) {
            const float appm = (float)(1e6 * (double)d_norm / (double)(float)d.Nsym);
            sc.ppm = (float)(.9 * (double)sc.ppm + .1 * (double)appm);
        } else {
            const float appm = (1e6f * d_norm) / (float)d.Nsym;
            sc.ppm = (0.9f * sc.ppm) + (0.1f * appm);
        }
    }
    Timing t;
    t.nin_next = d.N;
    if (!d.burst_mode) {
        if (norm_rx_timing > d.nin_thresh) t.nin_next = d.N + d.nin_step;         // (plan: 0.25 and Ts / 4 as recalled)
        else if (norm_rx_timing < -d.nin_thresh) t.nin_next = d.N - d.nin_step;
    }
    t.low_sample = (int)floorf(rx_timing);
    t.fract = rx_timing - (float)t.low_sample;
    t.high_sample = (int)ceilf(rx_timing);
    return t;
}

// ---- MODEM_STATS.rx_eye (diagnostic output of fsk_get_demod_stats / fsk_demod -t; off unless asked for) --------------------------------
// [UPSTREAM-RECALLED fsk.c, end of fsk_demod_core]: ET_MAX / M traces per tone, two symbols of |f_int| each, every dec-th
// position kept, trace i of tone m in row i*M + m from position 2P(i + 1) + neyeoffset, neyeoffset = high_sample + 1
// (the trace centred on the timing estimate); unnormalised here (the reader normalises).
__device__ __forceinline__ void write_eye(const Stream &c, int high_sample)
{
    const int M = c.a.d.M, P = c.a.d.P, nint = c.a.d.nint;
    const int dec = (2 * P + kEyePoints - 1) / kEyePoints, npts = (2 * P) / dec;
    int traces = kEyeTraces / M;
    while (traces > 0 && 2 * P * traces + (P / 2 + 1) + (npts - 1) * dec >= nint) traces--;
    float *eo = c.a.io.eye + (size_t)c.sid * kEyeTraces * kEyePoints;
    for (int e = c.tid; e < traces * M * npts; e += c.NT) {
        const int row = e / npts, j = e - row * npts, i = row / M, m = row - i * M;
        const float2 v = c.L.fint[m * nint + 2 * P * (i + 1) + (high_sample + 1) + dec * j];
        eo[row * kEyePoints + j] = sqrtf((v.x * v.x) + (v.y * v.y));
    }
}

// ---- a-8: resample, decide, stats ------------------------------------------------------------------------------------------------------
// Every symbol's tone powers at the timing estimate: the hard decision (one bit per byte into bits_l when the frame's bits are packed
// afterwards), the soft magnitudes, and this thread's share of the power sums. KEEP_TERMS: the symbols' two power terms into
// pw[0 .. 2 Nsym) as well, for the oracle-order sums.
template <bool KEEP_TERMS>
__device__ __forceinline__ SymbolSums decide_symbols(const Stream &c, const Timing &t, const FrameOut &o, uint8_t *bits_l, float *pw)
{
    const FskDims &d = c.a.d;
    const int M = d.M, Nsym = d.Nsym, nint = d.nint;
    const float fract = t.fract;
    SymbolSums s = {0.f, 0.f, 0.f, 0.f};
    for (int i = c.tid; i < Nsym; i += c.NT) {
        const int st = (i + 1) * d.P;
        float tmax[kMaxTones] = {0.f, 0.f, 0.f, 0.f};
        float sum = 0.f;
#pragma unroll
        for (int m = 0; m < kMaxTones; m++) if (m < M) {
            const float2 lo = c.L.fint[m * nint + st + t.low_sample];
            const float2 hi = c.L.fint[m * nint + st + t.high_sample];
            tmax[m] = tone_power(lo, hi, fract);
            sum += tmax[m];
        }
        float mx = tmax[0]; int sym = 0;
#pragma unroll
        for (int m = 1; m < kMaxTones; m++) if (m < M && tmax[m] > mx) { mx = tmax[m]; sym = m; }
        if (o.bits) {
            uint8_t *bo = d.pack_bits ? bits_l : o.bits;
            if (M == 2) bo[i] = sym == 1;
            else { bo[2 * i + 1] = sym & 1; bo[2 * i] = (sym & 2) >> 1; }
        }
        if (o.filt) {
#pragma unroll
            for (int m = 0; m < kMaxTones; m++) if (m < M) o.filt[m * Nsym + i] = sqrtf(tmax[m]);
        }
        s.sig += mx;
        s.nse += (sum - mx) / (float)(M - 1);
        s.std_e += mx;
        s.mean_e += sqrtf(mx);
        if (KEEP_TERMS) { pw[i] = mx; pw[Nsym + i] = (sum - mx) / (float)(M - 1); }
    }
    return s;
}
// bits_l, one bit per byte -> eight to a byte, first bit in the MSB
__device__ __forceinline__ void pack_bits(const Stream &c, const FrameOut &o, const uint8_t *bits_l)
{
    __syncthreads();
    for (int j = c.tid; j < o.frame_bytes; j += c.NT) {
        unsigned byte = 0;
        for (int b = 0; b < 8; b++) if (8 * j + b < c.a.d.Nbits) byte |= (unsigned)(bits_l[8 * j + b] & 1) << (7 - b);
        o.bits[j] = (uint8_t)byte;
    }
}
// rx_sig_pow, rx_nse_pow (seeded 1e-12), meanebno, stdebno: the threads' partial sums through the workgroup reduction
__device__ __forceinline__ SymbolSums sum_symbols(Stream &c, SymbolSums s)
{
    s.sig = block_sum(s.sig, c.red, c.tid, c.NT); s.nse = block_sum(s.nse, c.red, c.tid, c.NT) + 1e-12f;
    s.mean_e = block_sum(s.mean_e, c.red, c.tid, c.NT); s.std_e = block_sum(s.std_e, c.red, c.tid, c.NT);
    return s;
}
// Oracle order [fsk_oracle.c]: the same four accumulated serially in symbol order, from the terms decide_symbols<true> kept in pw
__device__ __forceinline__ SymbolSums sum_symbols_serial(Stream &c, const float *pw)
{
    const int Nsym = c.a.d.Nsym;
    __syncthreads();
    if (c.tid == 0) {
        float rs = 0.0f, rn = 1e-12f, me = 0.0f, se = 0.0f;
        for (int i = 0; i < Nsym; i++) {
            const float mxv = pw[i];
            rs += mxv; rn += pw[Nsym + i];
            se += mxv; me += sqrtf(mxv);
        }
        c.red[0] = rs; c.red[1] = rn; c.red[2] = me; c.red[3] = se;
    }
    __syncthreads();
    const SymbolSums s = {c.red[0], c.red[1], c.red[2], c.red[3]};
    __syncthreads();
    return s;
}
// the frame's stats row; with a NaN timing estimate (upstream returns before touching the outputs) zeroed bits and magnitudes
__device__ __forceinline__ void finish_frame(const Stream &c, const FrameOut &o, int nin, bool bad)
{
    const StreamScalars &sc = c.sc;
    if (bad) {
        for (int i = c.tid; i < o.frame_bytes; i += c.NT) if (o.bits) o.bits[i] = 0;
        for (int i = c.tid; i < c.a.d.M * c.a.d.Nsym; i += c.NT) if (o.filt) o.filt[i] = 0.f;
    }
    if (!o.stats || c.tid != 0) return;
    write_stats_row(o.stats, sc.f_est, sc.norm_rx_timing, sc.SNRest, nin, sc.ppm, sc.rx_sig_pow, sc.rx_nse_pow);
}

}  // namespace

// One body, three arithmetic orders. EXACT: 0 = the kernel proper; 1 = the exact first frame (the prologue); 2 = EVERY frame in the
// oracle's operation order (PIRIP_KERNEL=exact: the on-device proof that the fast kernels' differences under noise are evaluation order
// and nothing else -- bits, soft magnitudes, timing, nin, SNRest bit for bit at any SNR; one thread walks the oscillator recursion and
// the timing sum of every frame, ~0.15 ms per frame and stream: a checker's speed, not a receiver's).
// The prologue is the first frame of a stream after fsk_create / reset with every operation in the ORACLE's order (fsk_oracle.c:300-400):
// the oscillator as the serial recursion phi_c *= dphi from (1, 0), the windows summed forward, the timing phasor sum accumulated
// serially in window order, atan2f as glibc's, the division by 2 pi in double. A recording that starts one sample before a symbol
// boundary hands the first decision (P == Ts) ONE sample; both tone magnitudes are then equal up to float rounding and the decision
// follows the last bit of the timing estimate -- only the same operations in the same order reproduce it. One frame,
// one launch, once per stream: cost does not matter; the demodulator proper (wave / block / this kernel) takes over at io.first.
// The stages with an oracle-order twin are chosen here and nowhere else: the oscillator walk, the timing sum, the timing angle, the
// symbol sums, and (as template arguments) the created state and the double ppm smoothing. Every other stage is one code for all three.
template <int EXACT>
__device__ __forceinline__ void fsk_demod_general_body(const DemodArgs &a)
{
    constexpr bool EXACT0 = EXACT == 1, EXACTM = EXACT != 0, EXACTALL = EXACT == 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const FskDims &d = a.d;
    // a segment (SegDesc: capture.hip, stream_rx.hip): own first sample, output row and frame budget, as the wave and block kernels
    // honour it; max_frames < 0: this stream slot sits the launch out, its state untouched. (The exact prologue is descriptor-free.)
    int64_t seg_in = 0, out0 = 0, seg_frames = a.io.max_frames;
    if (!EXACT0 && a.io.seg) {
        const SegDesc sd = a.io.seg[blockIdx.x];
        if (sd.max_frames < 0) return;                     // (workgroup-uniform: no barrier has been reached)
        seg_in = sd.in_off; out0 = sd.out_frame0; seg_frames = sd.max_frames;
    }
    Stream c{a, {d, a.t.lut}};
    open_stream(c, smem, seg_in);
    const int sid = c.sid, M = d.M;
    load_state<EXACT0>(c);
#pragma unroll
    for (int m = 0; m < kMaxTones; m++) c.phc[m] = (EXACTALL && a.s.phic) ? a.s.phic[(size_t)sid * kMaxTones + m] : make_float2(0.f, 0.f);
    ReadAhead ra;
    ra.can_pre = !EXACTM && !c.sample.direct && (c.sample.u8 || c.sample.s16) && d.N + d.nin_step <= kPre * c.NT;
    ra.have_pre = false;
    int64_t pos = 0, frame = 0;
    int nin = c.sc.nin;
    if (!EXACT0 && a.io.first) { pos = a.io.first[sid]; frame = pos ? 1 : 0; }      // an exact-first-frame prologue ran in this call
    const int64_t frame_limit = EXACT0 ? (a.io.max_frames < 1 ? a.io.max_frames : 1) : seg_frames;
    Tones tn = {};
    // The LDS aliases, as handed to the stages below. Sfw on X (estimate_tones). fdc, one tone's down-converted samples, on X where it
    // fits (carve()). bits_l on X: the FFT work array is free after the estimator (Nbits <= 8 Ndft). After the last tone fdc is dead
    // and holds the oracle-order scratch: ft1s at its start, and pw BEHIND the Nbits bytes of bits_l -- where fdc shares X, a row
    // starting at fdc[0] would overwrite the staged bits before pack_bits reads them ((Nbits + 3) / 4 + 2 Nsym floats <= 2 Nmem:
    // Nbits <= 2 Nsym, Ts >= 4). (hist and fint alias nothing.)
    float2 *const fdc = c.L.fdc;
    uint8_t *const bits_l = (uint8_t *)c.L.X;
    float *const ft1s = (float *)fdc, *const pw = (float *)fdc + (d.Nbits + 3) / 4;

    while (frame < frame_limit && pos + nin <= c.sample.nsamp) {
        stage_input(c, ra, pos, nin);
        estimate_tones(c, nin, c.L.X, tn);
        const int nold = d.Nmem - nin;
#pragma unroll
        for (int m = 0; m < kMaxTones; m++) if (m < M) {
            recall_history(c, m, nold / c.G, fdc);
            if constexpr (EXACTM) downconvert_tone_serial<EXACTALL>(c, c.phc[m], tn.drift_ix[m], nin, nold, fdc);
            else downconvert_tone(c, c.theta[m], tn.dtheta[m], tn.drift_ix[m], nin, nold, fdc);
            c.theta[m] += (uint32_t)nin * tn.dtheta[m];
            integrate_tone(c, m, fdc);
        }
        float2 tc;
        if constexpr (EXACTM) tc = timing_sum_serial(c, ft1s); else tc = timing_sum(c);

        FrameOut o;
        o.frame_bytes = d.pack_bits ? (d.Nbits + 7) / 8 : d.Nbits;
        o.bits = a.io.bits ? a.io.bits + (size_t)sid * a.io.bits_stride + (size_t)(out0 + frame) * o.frame_bytes : nullptr;
        o.filt = a.io.filt ? a.io.filt + (size_t)sid * a.io.filt_stride + (size_t)(out0 + frame) * M * d.Nsym : nullptr;
        o.stats = a.io.stats ? a.io.stats + (size_t)sid * a.io.stats_stride + (size_t)(out0 + frame) * PIRIP_STATS_PER_FRAME : nullptr;
        const bool bad = isnan(tc.x) || isnan(tc.y);       // (the same on every thread, like every condition around a barrier here)
        if (!bad) {
            float norm_rx_timing;
            if constexpr (EXACTM) norm_rx_timing = timing_angle_oracle(tc); else norm_rx_timing = timing_angle(tc);
            const Timing t = update_timing<EXACTALL>(c, norm_rx_timing);
            if (a.io.eye) write_eye(c, t.high_sample);
            SymbolSums s = decide_symbols<EXACTALL>(c, t, o, bits_l, pw);
            if (o.bits && d.pack_bits) pack_bits(c, o, bits_l);
            if constexpr (EXACTALL) s = sum_symbols_serial(c, pw); else s = sum_symbols(c, s);
            update_snr(c.sc, s, d.Nsym);
            nin = t.nin_next;
        }
        for (int m = 0; m < kMaxTones; m++) c.sc.f_est[m] = tn.f_est[m];
        finish_frame(c, o, nin, bad);
        pos += d.Nmem - nold;                              // (this frame's nin: `nin` is the next frame's by now)
        frame++;
        __syncthreads();
    }

    c.sc.nin = nin;
    for (int i = c.tid; i < d.Ndft; i += c.NT) a.s.Sf[(size_t)sid * d.Ndft + i] = c.L.Sf[i];
    if (EXACT0 && a.io.exact0_fmt == PIRIP_KERNEL_WAVE) {
        if (frame > 0) save_state_wave(c, tn, pos);        // (no frame yet: nothing is written and the stream stays in its created state)
    } else save_state(c);
    if (c.tid == 0) {
        a.s.scal[sid] = c.sc;
        if (EXACTALL && a.s.phic) for (int m = 0; m < kMaxTones; m++) a.s.phic[(size_t)sid * kMaxTones + m] = c.phc[m];
        if (EXACT0) { if (a.io.first_out) a.io.first_out[sid] = (int32_t)pos; }
        else {
            if (a.io.nframes) a.io.nframes[sid] = (int32_t)frame;
            if (a.io.consumed) a.io.consumed[sid] = pos;
        }
    }
}

// Launch bounds: up to 256 threads per stream at the register budget of three waves per SIMD (measured best of {2, 3, 4} x {128, 256})
// for frames of up to a few thousand samples; the wide build (up to 512 threads, two waves per SIMD, 256 VGPRs each) for long frames
// whose LDS footprint leaves one stream per CU anyway (Ts = 240 / Ndft = 4096: 111-126 KB) -- there the only occupancy is waves per stream.
__global__ __launch_bounds__(4 * kWave, 3) void fsk_demod_general_kernel(DemodArgs a) { fsk_demod_general_body<0>(a); }
__global__ __launch_bounds__(8 * kWave, 1) void fsk_demod_general_wide_kernel(DemodArgs a) { fsk_demod_general_body<0>(a); }
__global__ __launch_bounds__(4 * kWave, 1) void fsk_demod_exact0_kernel(DemodArgs a) { fsk_demod_general_body<1>(a); }
__global__ __launch_bounds__(4 * kWave, 1) void fsk_demod_exact_kernel(DemodArgs a) { fsk_demod_general_body<2>(a); }

size_t demod_general_lds_bytes(const FskDims &d) { return kRedBytes + carve(d, nullptr, nullptr); }

// the LDS attribute and the launch, for each of the four kernels
static hipError_t launch_build(void (*kernel)(DemodArgs), int nt, const DemodArgs &a, int nstreams, hipStream_t stream)
{
    const size_t lds = demod_general_lds_bytes(a.d);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    if (lds > 48 * 1024) {
        // per launch, not cached: the attribute belongs to the current device's copy of the kernel, and handles
        // on several devices / host threads may share this process
        hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(nstreams), dim3(nt), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_demod_general(const DemodArgs &a, int nstreams, hipStream_t stream)
{
    const size_t lds = demod_general_lds_bytes(a.d);
    // threads per stream: two waves (measured: 49 G samples/s at config 3 against 37 G with one wave and 36-40 G
    // with four -- barriers and the serial pieces stop scaling) unless the frame is too small to feed them
    // long frames (measured at Ts = 240 / Ndft = 4096, profiles/r03_instance_rates.txt): one stream per CU fits, so its workgroup is wide
    int nt = 2 * kWave;
    if (a.d.N + a.d.nin_step < 512) nt = kWave;
    else if (lds > 80 * 1024) nt = 8 * kWave;
    else if (direct_input(a.d)) nt = 4 * kWave;          // long frames, two streams per CU: 45 G at 256 threads against 27 G at 128, 36 G at 512 (one stream per CU)
    // PIRIP_GENERAL_THREADS (A/B runs): any whole number of waves up to 512 threads -- the body strides its loops by blockDim.x and adds its
    // per-wave partials in a plain loop, so each is a supported launch (another rounding of the workgroup sums); any other value is
    // ignored and the rule above stands
    if (const char *e = getenv("PIRIP_GENERAL_THREADS")) { const int v = atoi(e); if (v >= 64 && v <= 512 && v % 64 == 0) nt = v; }
    return launch_build(nt > 4 * kWave ? fsk_demod_general_wide_kernel : fsk_demod_general_kernel, nt, a, nstreams, stream);
}

hipError_t selftest_atan2(const float *d_y, const float *d_x, float *d_out, int n)
{
    hipLaunchKernelGGL(atan2_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, d_y, d_x, d_out, n);
    return hipGetLastError();
}

// The exact first frame exists where the structural tie does: a window of the integrator bank can hold a single sample only when the
// oversample factor equals the samples per symbol (Ts == P: `fsk_demod -p 24` at Ts = 24, the Ts = 8 / 10 shapes) -- there the group size
// of the integrator memory is 1, which the oracle-order window sums need; long frames that are not staged in LDS are left out.
bool demod_exact0_applicable(const FskDims &d) { return d.Ts == d.P && d.grp == 1 && !direct_input(d) && demod_general_lds_bytes(d) <= 160 * 1024; }
hipError_t launch_demod_exact0(const DemodArgs &a, int nstreams, hipStream_t stream) { return launch_build(fsk_demod_exact0_kernel, 2 * kWave, a, nstreams, stream); }
// every frame exact (PIRIP_KERNEL=exact): needs single-sample integrator memory (d.grp == 1, set by the handle) and staged input
bool demod_exact_applicable(const FskDims &d) { return d.grp == 1 && !direct_input(d) && demod_general_lds_bytes(d) <= 160 * 1024; }
hipError_t launch_demod_exact(const DemodArgs &a, int nstreams, hipStream_t stream) { return launch_build(fsk_demod_exact_kernel, 2 * kWave, a, nstreams, stream); }

}  // namespace pirip
