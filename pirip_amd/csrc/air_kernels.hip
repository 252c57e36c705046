// pirip_amd/csrc/air_kernels.hip -- include/pirip_hip.h section O: the channel.
//
// T transmitted wideband IQ streams onto R received ones, block after block. Path p = (receiver rx_p, transmitter t_p, gain a_p, delay d_p,
// offset f_p); with n the absolute sample index and x_t[k] = 0 below the last reset:
//     y_r[n] = sum_{p of receiver r, ascending} a_p e^{+j 2 pi f_p n / Fs} x_{t_p}[n - d_p]  +  sigma_r w_r[n]
// Every piece is the one definition of iq_device.hpp and noise_device.hpp: u8_to_float, the exact integer phase (mulmod_fs once per lane
// and path, then its exact integer increment f_p with one wrap per sample -- no recursion in floating point), unit_phasor, crot, one fma
// per component and path into a sum that starts at 0, add_awgn keyed by (seed, r, n), quant_u8_csdr.
//
// Mix kernel: one workgroup per (tile of kAirTile = 2048 outputs, receiver); thread t owns the 8 consecutive outputs 8 t .. 8 t + 7 of the
// tile, so a u8 row is stored 16 bytes per lane and 1024 consecutive bytes per wave, and a complex float row as four 16-byte stores per
// lane; rows that are only aligned to the sample, and a tile's ragged end, are stored sample by sample -- the same values.
// The paths of the receiver are taken one after the other, ascending. The tile's span of the path's transmitter -- cnt consecutive samples
// from call index j0 - d_p on -- is unaligned by construction, so it goes through LDS as the 16-byte units that hold it, loaded aligned:
// the part below the call's first sample from the transmitter's ring (units taken modulo the ring, which is a power of two of samples and so
// wraps on a unit), the rest from the call's row. The two parts keep their own byte shift in LDS; a lane reads its samples at
// shift + 16 u + BS k, two or eight bytes at a time, from the part its sample lies in: the choice between ring and row is an address, not a
// branch, and the staging loops are the only place where the two sources differ (each loop is uniform but for its last trip).
// An aligned unit that holds one byte of a row lies in that byte's page: the bytes it over-reads are never used.
// Samples below the last reset are zero by their index (for u8: the float zero, not byte 128), whatever the ring holds.
// Carry kernel, behind the mix kernel in stream order: the call's last min(n, ring) samples of every transmitter go to their ring slots
// (absolute index modulo the ring), sample by sample.
// Drift: a path with a clock offset reads its transmitter at a fractional position through a 16-tap polyphase
// interpolator, on a longer span and with the table. The slip budget is host state, checked when a call is enqueued.
// Fading: a path with a fade has its samples multiplied by a gain that moves, the sum of sixteen scatterers whose 32-bit
// phases are a function of the absolute index, made on a grid of 16 samples and a line between, the grid points of the tile in LDS behind
// the staging area.
// The mix kernel is one body, air_mix_body<bytes in, bytes out, DRIFT, FADE>, whose two compile-time switches say whether a path may have a
// clock offset and whether it may have a fade; per path it stages and reads (a static span or the interpolator's), applies the fade, mixes,
// and behind the paths adds the noise and stores. Three thin kernels name its instantiations: air_mix_kernel (neither switch; AirArgs)
// for handles without such paths, air_mix_drift_kernel (DRIFT; + AirDrift) for handles with a drifting path, air_mix_fade_kernel (both;
// + AirFade) for handles with a fading one. A path without offset and fade gives the same words in all three.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/pirip_hip.h"
#include "air_handle.hpp"
#include "hip_host.hpp"
#include "iq_device.hpp"
#include "noise_device.hpp"
#include "rate_host.hpp"

using namespace pirip;

namespace {

template <int BSI>
__device__ __forceinline__ v2f air_sample(const char *p, v2f chi, v2f clo)
{
    if (BSI == 2) {
        const uint32_t w = *(const uint16_t *)p;
        return u8_to_float(v2f{(float)(w & 0xffu), (float)(w >> 8)}, chi, clo);
    }
    return *(const v2f *)p;
}

// ---- the pieces of air_mix_body below, which owns the barrier between the reads of the path before and a path's staging

// A span of a transmitter staged in LDS: sample u of it is at (u < cnt_r ? off_r : off_w) + u * BSI, and the samples below vfirst lie
// below the last reset
struct AirSpan { int cnt_r, off_r, off_w, vfirst; };

// scnt consecutive samples of transmitter tx from call index s0 on, into LDS as the 16-byte units that hold them: the cnt_r below the
// call's first sample from the ring, the rest from the call's row. `limit` is what vfirst is clamped to on its way to an int: any value
// that no span position of a stored output reaches. Which one a caller passes is tuning, since it moves the compiler's register
// allocation: the tile's count for the kernel of static paths (72 VGPRs and 7 waves per SIMD with u8 input; 74 and 6 with the constant),
// the constants for the other two, which then compile to what they were before the kernels shared a body.
template <int BSI>
__device__ __forceinline__ AirSpan air_stage(const AirArgs &a, int tx, const AirRing &rg, int64_t s0, int scnt, int limit, int tid, char *smem)
{
    const int cnt_r = s0 >= 0 ? 0 : (-s0 < scnt ? (int)-s0 : scnt);     // samples from the ring
    const int cnt_w = scnt - cnt_r;                                     // samples from the call's row
    // span index of the first sample at or above the last reset
    const int64_t vf = a.first - (a.N0 + s0);
    const int vfirst = vf <= 0 ? 0 : (vf < limit ? (int)vf : limit);
    int shift_r = 0, units_r = 0;
    if (cnt_r > 0) {
        const uint32_t b0 = (uint32_t)((uint64_t)(a.N0 + s0) & rg.mask) * BSI;            // (a ring holds at most 2^20 samples of 8 bytes)
        const uint32_t umask = ((rg.mask + 1u) * BSI >> 4) - 1u;
        const uint4 *src = (const uint4 *)(a.ring + (size_t)rg.off * BSI);
        shift_r = (int)(b0 & 15u);
        units_r = (shift_r + cnt_r * BSI + 15) >> 4;
        for (int u = tid; u < units_r; u += kAirThreads) ((uint4 *)smem)[u] = src[((b0 >> 4) + (uint32_t)u) & umask];
    }
    int shift_w = 0;
    if (cnt_w > 0) {
        const char *p = a.in + (size_t)tx * a.in_stride + (size_t)(s0 + cnt_r) * BSI;
        shift_w = (int)((uintptr_t)p & 15);
        const uint4 *src = (const uint4 *)(p - shift_w);
        const int units_w = (shift_w + cnt_w * BSI + 15) >> 4;
        for (int u = tid; u < units_w; u += kAirThreads) ((uint4 *)smem)[units_r + u] = src[u];
    }
    __syncthreads();
    return AirSpan{cnt_r, shift_r, units_r * 16 + shift_w - cnt_r * BSI, vfirst};
}

template <int BSI>
__device__ __forceinline__ v2f air_span_sample(const char *smem, const AirSpan &sp, int u, v2f chi, v2f clo)
{
    v2f x = air_sample<BSI>(smem + (u < sp.cnt_r ? sp.off_r : sp.off_w) + u * BSI, chi, clo);
    if (u < sp.vfirst) x = v2f{0.f, 0.f};
    return x;
}

// a path with a clock offset q != 0 reads its transmitter at n - d_p + S + rho / Q through the interpolator. Its span is
// [i_first - 7, i_last + 8] with i = n - d_p + S: at most kAirTile + kAirSpanExtra samples, staged as a static path's is. A lane takes
// (S, rho) of its first output from the tile's by exact integers, steps them per output, and reads tap k of an output at span position
// j + (S - S_first) + k, from the part that position lies in; the table row of phase floor(1024 rho / Q) comes through the caches.
template <int BSI>
__device__ __forceinline__ void air_read_drift(const AirArgs &a, const AirDrift &d, const AirPath &pth, const AirRing &rg, int32_t q, int64_t j0, int cnt,
                                               int jl, int tid, v2f chi, v2f clo, char *smem, v2f (&v)[kAirPerThread])
{
    int64_t S0;
    int32_t rho0;
    clock_slip(d.age + j0, q, S0, rho0);                                // the tile's first output
    int32_t dS = 0, rho1 = rho0;
    clock_advance(cnt - 1, q, dS, rho1);                                // ... and how far S moves up to its last
    // the span's first sample, as an index of this call, and its length
    const AirSpan sp = air_stage<BSI>(a, pth.tx, rg, j0 - pth.delay + S0 - kAirLead, cnt + dS + kAirTaps - 1, kAirTile + kAirSpanExtra, tid, smem);
    int32_t S = 0, rho = rho0;                                          // S from here on: relative to the tile's first
    clock_advance(jl, q, S, rho);
#pragma unroll
    for (int k = 0; k < kAirPerThread; k++) {
        const int u0 = jl + k + S;                                      // span position of the output's first tap
        const float4 *row = (const float4 *)(d.taps + clock_phase_1024(rho) * kAirTaps);
        v2f s = {0.f, 0.f};
#pragma unroll
        for (int c = 0; c < kAirTaps / 4; c++) {
            const float4 t4 = row[c];
            const float t[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int e = 0; e < 4; e++) s = __builtin_elementwise_fma(v2f{t[e], t[e]}, air_span_sample<BSI>(smem, sp, u0 + 4 * c + e, chi, clo), s);
        }
        v[k] = s;
        clock_step(q, S, rho);
    }
}

// the mix of a path whose sample for the lane's output k is v(k): the rotation by the exact integer phase where f_p != 0, then
// acc = fma(a_p, v, acc)
template <typename V>
__device__ __forceinline__ void air_mix_path(const AirArgs &a, const AirPath &pth, uint32_t idx0, V v, v2f (&acc)[kAirPerThread])
{
    const v2f g = {pth.gain, pth.gain};
    if (pth.fres != 0) {
        uint32_t ph = (uint32_t)(int32_t)mulmod_fs((double)pth.fres, (double)idx0, a.Fs, a.inv_fs_d);
#pragma unroll
        for (int k = 0; k < kAirPerThread; k++) {
            float cs, sn;
            unit_phasor((int32_t)ph, a.Fs, a.two_over_fs, cs, sn);
            acc[k] = __builtin_elementwise_fma(g, crot(v(k), cs, sn), acc[k]);
            ph += (uint32_t)pth.fres;
            if (ph >= (uint32_t)a.Fs) ph -= (uint32_t)a.Fs;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kAirPerThread; k++) acc[k] = __builtin_elementwise_fma(g, v(k), acc[k]);
    }
}

// the receiver's noise on the lane's sums, and the store
template <int BSO>
__device__ __forceinline__ void air_finish(const AirArgs &a, int r, int64_t j0, int jl, int cnt, v2f (&acc)[kAirPerThread])
{
    const float sigma = a.sigma[r];
    if (sigma > 0.f) {
        const int64_t n_abs = a.N0 + j0 + jl;
#pragma unroll
        for (int k = 0; k < kAirPerThread; k++) {
            float xr = acc[k].x, xi = acc[k].y;
            add_awgn(a.seed, r, n_abs + k, sigma, xr, xi);
            acc[k] = v2f{xr, xi};
        }
    }

    if (jl >= cnt) return;
    char *row = a.out + (size_t)r * a.out_stride + (size_t)(j0 + jl) * BSO;
    const bool whole = a.aligned16 && jl + kAirPerThread <= cnt;
    if (BSO == 2) {
        uint32_t w[kAirPerThread];
#pragma unroll
        for (int k = 0; k < kAirPerThread; k++) w[k] = (uint32_t)quant_u8_csdr(acc[k].x) | ((uint32_t)quant_u8_csdr(acc[k].y) << 8);
        if (whole) {
            *(uint4 *)row = make_uint4(w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16));
        } else {
#pragma unroll
            for (int k = 0; k < kAirPerThread; k++) if (jl + k < cnt) ((uint16_t *)row)[k] = (uint16_t)w[k];
        }
    } else {
        if (whole) {
#pragma unroll
            for (int k = 0; k < kAirPerThread; k += 2) ((float4 *)row)[k >> 1] = make_float4(acc[k].x, acc[k].y, acc[k + 1].x, acc[k + 1].y);
        } else {
#pragma unroll
            for (int k = 0; k < kAirPerThread; k++) if (jl + k < cnt) ((float2 *)row)[k] = make_float2(acc[k].x, acc[k].y);
        }
    }
}

// ---- fading: a fading path's samples -- a static path's or the interpolator's -- are multiplied by the gain g[n] of the
// receiver's index n before the mix

// Grid point k of a fade, at absolute index 16 k: scatterer j has the 32-bit phase theta_j + w_j * (uint32)(16 k), plain wrap-around
// arithmetic on the absolute index; its top 24 bits are exact in a float, t in [-1, 1), and sincospif takes t half turns.
__device__ __forceinline__ v2f fade_grid_point(const AirFadeTable &f, uint32_t n16)
{
    float C = 0.f, D = 0.f;
#pragma unroll 4
    for (int j = 0; j < kAirScatter; j++) {
        const uint32_t psi = f.theta[j] + (uint32_t)f.w[j] * n16;
        const float t = (float)((int32_t)psi >> 8) * 0x1p-23f;
        float sn, cs;
        sincospif(t, &sn, &cs);
        C += cs; D += sn;
    }
    return v2f{__builtin_fmaf(f.scale, C, f.los), f.scale * D};
}

// the grid points of a tile of cnt outputs whose first has the absolute index n_tile (taken as uint32), into LDS: thread i makes grid
// point (first of the tile) + i; the tile needs at most kAirFadePoints
__device__ __forceinline__ void fade_grid_stage(const AirFadeTable &f, int64_t n_tile, int cnt, int tid, v2f *grid)
{
    const uint32_t nt = (uint32_t)(uint64_t)n_tile, into = nt & (uint32_t)(kAirFadeGrid - 1);
    const int points = (int)((into + (uint32_t)cnt - 1u) >> kAirFadeGridLog2) + 2;
    if (tid < points) grid[tid] = fade_grid_point(f, nt - into + (uint32_t)tid * (uint32_t)kAirFadeGrid);
}

// v[k] *= g[n] for the lane's outputs from tile index jl on: they lie in at most two cells, so the lane reads three grid points and forms
// the line per output
__device__ __forceinline__ void fade_apply(const v2f *grid, int64_t n_tile, int jl, v2f (&v)[kAirPerThread])
{
    // the lane's first output, in samples behind the tile's first grid point
    const uint32_t l0 = ((uint32_t)(uint64_t)n_tile & (uint32_t)(kAirFadeGrid - 1)) + (uint32_t)jl;
    const int c0 = (int)(l0 >> kAirFadeGridLog2);
    const int c2 = c0 + 2 < kAirFadePoints ? c0 + 2 : kAirFadePoints - 1;               // (needed only where the lane crosses into cell c0 + 1)
    const v2f ga = grid[c0], gb = grid[c0 + 1], gc = grid[c2];
#pragma unroll
    for (int k = 0; k < kAirPerThread; k++) {
        const uint32_t l = l0 + (uint32_t)k;
        const bool next = (int)(l >> kAirFadeGridLog2) != c0;
        const v2f lo = next ? gb : ga, hi = next ? gc : gb;
        const float mu = (float)(l & (uint32_t)(kAirFadeGrid - 1)) * (1.0f / kAirFadeGrid);
        const v2f g = __builtin_elementwise_fma(v2f{mu, mu}, hi - lo, lo);
        v[k] = crot(v[k], g.x, g.y);
    }
}

// The one body of the three mix kernels. DRIFT: a path may have a clock offset (d is read); FADE: a path may have a fade (f is read).
// Both branches are uniform per workgroup and path, and a path with neither takes a static path's steps in every instantiation. A fade's
// grid points go to LDS behind the staging area, between the barrier that separates the paths and the one that ends the staging, so a
// fade adds no barrier.
// LDS: the staging area, (kAirTile [+ kAirSpanExtra with DRIFT]) * BSI + 64 bytes (the span's units: two parts, each with a unit of slack at
// either end) [+ kAirFadePoints * 8 bytes with FADE]
template <int BSI, int BSO, bool DRIFT, bool FADE>
__device__ __forceinline__ void air_mix_body(const AirArgs &a, const AirDrift &d, const AirFade &f)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int r = blockIdx.y;
    const int64_t j0 = (int64_t)blockIdx.x * kAirTile;                 // first output of the tile (of this call)
    const int cnt = (int)((a.n - j0) < kAirTile ? (a.n - j0) : kAirTile);
    const int jl = tid * kAirPerThread;                                 // the thread's first output of the tile
    const v2f chi = {a.c_hi, a.c_hi}, clo = {a.c_lo, a.c_lo};
    // (n mod Fs) of the thread's first output
    const uint32_t base = (uint32_t)(((int64_t)a.n0m + j0 % a.Fs) % a.Fs);
    const uint32_t idx0 = (base + (uint32_t)jl) % (uint32_t)a.Fs;
    v2f acc[kAirPerThread];
#pragma unroll
    for (int k = 0; k < kAirPerThread; k++) acc[k] = v2f{0.f, 0.f};

    const int p0 = a.rx_start[r], p1 = a.rx_start[r + 1];
    for (int pi = p0; pi < p1; pi++) {
        const AirPath pth = a.paths[pi];
        const AirRing rg = a.rings[pth.tx];
        int32_t q = 0, fi = -1;                                         // (loaded in front of the barrier, with the path)
        if constexpr (DRIFT) q = d.ppb[pi];
        if constexpr (FADE) fi = f.index[pi];
        if (pi > p0) __syncthreads();                                   // the reads of the path before | this path's grid points and staging
        if constexpr (!DRIFT && !FADE) {
            // nothing lies between a sample's read and its mix, so each is read where it is mixed: the lane's 8 samples are not held in
            // registers over the rotation (u8 input: 72 VGPRs and 7 waves per SIMD, against 79 and 6)
            const AirSpan sp = air_stage<BSI>(a, pth.tx, rg, j0 - pth.delay, cnt, cnt, tid, smem);
            air_mix_path(a, pth, idx0, [&](int k) { return air_span_sample<BSI>(smem, sp, jl + k, chi, clo); }, acc);
        } else {
            v2f *grid = (v2f *)(smem + f.grid_off);
            v2f v[kAirPerThread];                                       // what the path reads for the lane's outputs
            if (fi >= 0) fade_grid_stage(f.table[fi], a.N0 + j0, cnt, tid, grid);
            if (q != 0) air_read_drift<BSI>(a, d, pth, rg, q, j0, cnt, jl, tid, chi, clo, smem, v);
            else {
                const AirSpan sp = air_stage<BSI>(a, pth.tx, rg, j0 - pth.delay, cnt, kAirTile, tid, smem);        // a static path: x_t[n - d_p]
#pragma unroll
                for (int k = 0; k < kAirPerThread; k++) v[k] = air_span_sample<BSI>(smem, sp, jl + k, chi, clo);
            }
            if (fi >= 0) fade_apply(grid, a.N0 + j0, jl, v);
            air_mix_path(a, pth, idx0, [&](int k) { return v[k]; }, acc);
        }
    }
    air_finish<BSO>(a, r, j0, jl, cnt, acc);
}

// the three kernels a handle can launch, by what its paths have: nothing more, a clock offset somewhere, a fade somewhere
template <int BSI, int BSO>
__global__ __launch_bounds__(kAirThreads) void air_mix_kernel(AirArgs a) { air_mix_body<BSI, BSO, false, false>(a, AirDrift{}, AirFade{}); }
template <int BSI, int BSO>
__global__ __launch_bounds__(kAirThreads) void air_mix_drift_kernel(AirArgs a, AirDrift d) { air_mix_body<BSI, BSO, true, false>(a, d, AirFade{}); }
template <int BSI, int BSO>
__global__ __launch_bounds__(kAirThreads) void air_mix_fade_kernel(AirArgs a, AirDrift d, AirFade f) { air_mix_body<BSI, BSO, true, true>(a, d, f); }

// the call's last min(n, ring) samples of transmitter blockIdx.y -> ring[absolute index & mask]
template <typename S>
__global__ __launch_bounds__(kAirThreads) void air_carry_kernel(AirArgs a)
{
    const int t = blockIdx.y;
    const AirRing rg = a.rings[t];
    const int64_t R = (int64_t)rg.mask + 1;
    const int64_t count = a.n < R ? a.n : R;
    const S *row = (const S *)(a.in + (size_t)t * a.in_stride);
    S *ring = (S *)a.ring + rg.off;
    for (int64_t i = (int64_t)blockIdx.x * kAirThreads + threadIdx.x; i < count; i += (int64_t)gridDim.x * kAirThreads) {
        const int64_t s = a.n - count + i;
        ring[(uint64_t)(a.N0 + s) & rg.mask] = row[s];
    }
}

bool sigma_ok(const float *sigma, int nrx)
{
    for (int r = 0; sigma && r < nrx; r++) if (!std::isfinite(sigma[r]) || sigma[r] < 0.f) return false;
    return true;
}

// ---- the interpolator's table (4.15a): T[phi][k] = sinc(k - 7 - mu) w((k - 7 - mu) / 8), mu = phi / 1024, w a Kaiser window of beta 6; every
// phase divided by its own sum; in double, rounded once to float

double bessel_i0(double x)
{
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 64; k++) {
        term *= (x / (2.0 * k)) * (x / (2.0 * k));
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

struct InterpTable {
    float t[kAirPhases][kAirTaps];
    InterpTable()
    {
        const double pi = 3.14159265358979323846, beta = 6.0, i0b = bessel_i0(beta);
        for (int phi = 0; phi < kAirPhases; phi++) {
            double row[kAirTaps], sum = 0.0;
            for (int k = 0; k < kAirTaps; k++) {
                const double x = (double)(k - kAirLead) - (double)phi / kAirPhases, u = x / (kAirTaps / 2);
                // (sinc of a whole number but 0 is 0, not what sin makes of a multiple of pi: phase 0 is the exact unit impulse)
                const double sinc = x == 0.0 ? 1.0 : (x == std::floor(x) ? 0.0 : std::sin(pi * x) / (pi * x));
                const double w = std::fabs(u) > 1.0 ? 0.0 : bessel_i0(beta * std::sqrt(1.0 - u * u)) / i0b;
                row[k] = sinc * w;
                sum += row[k];
            }
            for (int k = 0; k < kAirTaps; k++) t[phi][k] = (float)(row[k] / sum);
        }
    }
};

const InterpTable &interp_table()
{
    static const InterpTable table;
    return table;
}

// the last clock age the slip budget lets a sample have: q > 0: m q < (max_slip + 1) Q; q < 0: m |q| <= max_slip Q (no product above 2^51)
int64_t last_age_of(int32_t max_slip, int32_t q_fast, int32_t q_slow)
{
    int64_t last = INT64_MAX;
    if (q_fast > 0) last = (((int64_t)max_slip + 1) * kClockQ - 1) / q_fast;
    if (q_slow > 0 && (int64_t)max_slip * kClockQ / q_slow < last) last = (int64_t)max_slip * kClockQ / q_slow;
    return last;
}

// ---- a fade's table (4.15b): the integers and floats the kernel reads, made on the host in double and rounded once

int32_t max_doppler_millihz(int Fs) { return (int32_t)(1000 * (int64_t)Fs / 1024); }

bool fade_ok(const pirip_air_fade &f) { return f.doppler_millihz >= 0 && std::isfinite(f.rice_k) && f.rice_k >= 0.f; }

// scatterer j: the first draw of key (seed, key, j) is u_j (its top 53 bits), the draw of that draw gives theta_j (its top 32 bits)
AirFadeTable fade_table(int Fs, uint64_t seed, const pirip_air_fade &f)
{
    const double pi = 3.14159265358979323846, fd = (double)f.doppler_millihz / 1000.0, K = (double)f.rice_k;
    AirFadeTable t{};
    for (int j = 0; j < kAirScatter; j++) {
        const uint64_t r1 = splitmix(seed ^ splitmix(((uint64_t)f.key << 32) ^ (uint64_t)j));
        const uint64_t r2 = splitmix(r1);
        const double u = (double)(r1 >> 11) * 0x1p-53;
        const double alpha = 2.0 * pi * ((double)j + u) / kAirScatter;
        const double nu = fd * std::cos(alpha);
        t.w[j] = (int32_t)std::llrint(nu / (double)Fs * 4294967296.0);
        t.theta[j] = (uint32_t)(r2 >> 32);
    }
    t.scale = (float)std::sqrt(1.0 / (kAirScatter * (K + 1.0)));
    t.los = (float)std::sqrt(K / (K + 1.0));
    return t;
}

int air_create(int Fs, int in_format, int out_format, int ntx, int nrx, int npaths, const pirip_air_path_ex *paths, int nfades,
               const pirip_air_fade *fades, const float *sigma, uint64_t seed, int32_t max_slip, int device, pirip_hip_air **out)
{
    if (!out) return PIRIP_ERR_BAD_ARG;
    *out = nullptr;
    if (Fs < 2 || ntx < 1 || nrx < 1 || npaths < 0 || (npaths > 0 && !paths) || max_slip < 0) return PIRIP_ERR_BAD_ARG;
    if (nfades < 0 || (nfades > 0 && !fades)) return PIRIP_ERR_BAD_ARG;
    bool fast_fade = false;
    for (int i = 0; i < nfades; i++) {
        if (fades[i].path < 0 || fades[i].path >= npaths || !fade_ok(fades[i])) return PIRIP_ERR_BAD_ARG;
        for (int k = 0; k < i; k++) if (fades[k].path == fades[i].path) return PIRIP_ERR_BAD_ARG;
        if (Fs <= kMaxFs && fades[i].doppler_millihz > max_doppler_millihz(Fs)) fast_fade = true;
    }
    if (in_format != PIRIP_IN_CU8_CSDR && in_format != PIRIP_IN_CF32) return PIRIP_ERR_BAD_ARG;
    if (out_format != PIRIP_IN_CU8_CSDR && out_format != PIRIP_IN_CF32) return PIRIP_ERR_BAD_ARG;
    int max_delay = 0;
    int32_t q_fast = 0, q_slow = 0;                                     // the largest clock offset of either sign, as magnitudes
    bool unsupported = false;
    for (int p = 0; p < npaths; p++) {
        const pirip_air_path_ex &q = paths[p];
        const int64_t f2 = 2 * (int64_t)q.offset_hz;
        if (q.rx < 0 || q.rx >= nrx || q.tx < 0 || q.tx >= ntx || q.delay < 0 || f2 <= -(int64_t)Fs || f2 >= (int64_t)Fs) return PIRIP_ERR_BAD_ARG;
        if (!std::isfinite(q.gain)) return PIRIP_ERR_BAD_ARG;
        if (q.delay > max_delay) max_delay = q.delay;
        if (q.clock_ppb == 0) continue;
        // the taps never reach past sample n, and the lag with slip and leading taps stays inside the longest ring
        if (max_slip < 1 || (int64_t)q.delay < (int64_t)kAirLead + 1 + (q.clock_ppb > 0 ? max_slip : 0)) return PIRIP_ERR_BAD_ARG;
        if ((int64_t)q.delay + kAirLead + (q.clock_ppb < 0 ? max_slip : 0) > kAirMaxDelay) unsupported = true;
        if (q.clock_ppb > kAirMaxPpb || q.clock_ppb < -kAirMaxPpb) { unsupported = true; continue; }
        if (q.clock_ppb > q_fast) q_fast = q.clock_ppb;
        if (-q.clock_ppb > q_slow) q_slow = -q.clock_ppb;
    }
    if (!sigma_ok(sigma, nrx)) return PIRIP_ERR_BAD_ARG;
    if (unsupported || fast_fade || Fs > kMaxFs || max_delay > kAirMaxDelay || ntx > 65535 || nrx > 65535) return PIRIP_ERR_UNSUPPORTED;
    const U8Split u8 = csdr_u8_split();
    if (!u8.exact) return PIRIP_ERR_UNSUPPORTED;
    int dev = 0;
    PIRIP_TRY(select_device(device, &dev));
    pirip_hip_air *h = new (std::nothrow) pirip_hip_air();
    if (!h) return PIRIP_ERR_NOMEM;
    h->device = dev;
    h->Fs = Fs; h->ntx = ntx; h->nrx = nrx; h->npaths = npaths; h->in_format = in_format; h->out_format = out_format;
    h->bsi = bytes_per_sample(in_format); h->bso = bytes_per_sample(out_format);
    h->max_delay = max_delay; h->seed = seed; h->u8 = u8;
    h->max_slip = max_slip; h->drift = q_fast != 0 || q_slow != 0; h->last_age = last_age_of(max_slip, q_fast, q_slow);
    h->fade = nfades > 0;
    // the paths of every receiver, ascending; every transmitter's ring: the smallest power of two that holds its longest lag -- a static
    // path's delay, a drifting one's with its slip and the leading taps
    std::vector<int32_t> rx_start(1, 0);
    std::vector<AirPath> sorted;
    std::vector<int32_t> ppb;
    std::vector<int32_t> fade_index;                                    // per sorted path: its row of fade_tables, -1: none
    std::vector<AirFadeTable> fade_tables;
    std::vector<int32_t> longest((size_t)ntx, 0);
    for (int r = 0; r < nrx; r++) {
        for (int p = 0; p < npaths; p++) {
            if (paths[p].rx != r) continue;
            sorted.push_back(AirPath{paths[p].tx, paths[p].delay, (int32_t)fs_residue(paths[p].offset_hz, Fs), paths[p].gain});
            ppb.push_back(paths[p].clock_ppb);
            fade_index.push_back(-1);
            for (int i = 0; i < nfades; i++) {
                if (fades[i].path != p) continue;
                fade_index.back() = (int32_t)fade_tables.size();
                fade_tables.push_back(fade_table(Fs, seed, fades[i]));
            }
            const int32_t q = paths[p].clock_ppb;
            const int32_t lag = paths[p].delay + (q != 0 ? kAirLead : 0) + (q < 0 ? max_slip : 0);
            if (lag > longest[(size_t)paths[p].tx]) longest[(size_t)paths[p].tx] = lag;
        }
        rx_start.push_back((int32_t)sorted.size());
    }
    std::vector<AirRing> rings((size_t)ntx);
    uint64_t total = 0;
    for (int t = 0; t < ntx; t++) {
        uint32_t R = kAirMinRing;
        while (R < (uint32_t)longest[(size_t)t]) R <<= 1;
        rings[(size_t)t] = AirRing{total, R - 1u, 0u};
        if ((int)R > h->max_ring) h->max_ring = (int)R;
        total += R;
    }
    std::vector<float> sg((size_t)nrx, 0.f);
    for (int r = 0; sigma && r < nrx; r++) sg[(size_t)r] = sigma[r];
    auto tables = [&]() -> int {
        DevMem &m = h->mem;
        PIRIP_TRY(m.alloc_filled(&h->d_ring, 0, (size_t)total * (size_t)h->bsi));
        PIRIP_TRY(m.upload(&h->d_rings, rings.data(), sizeof(AirRing) * rings.size()));
        PIRIP_TRY(m.upload(&h->d_rx_start, rx_start.data(), sizeof(int32_t) * rx_start.size()));
        PIRIP_TRY(m.upload(&h->d_paths, sorted.data(), sizeof(AirPath) * sorted.size()));
        PIRIP_TRY(m.upload(&h->d_sigma, sg.data(), sizeof(float) * sg.size()));
        if (h->drift || h->fade) PIRIP_TRY(m.upload(&h->d_ppb, ppb.data(), sizeof(int32_t) * ppb.size()));
        if (h->drift) PIRIP_TRY(m.upload(&h->d_taps, &interp_table().t[0][0], sizeof(InterpTable)));
        if (h->fade) {
            PIRIP_TRY(m.upload(&h->d_fade_index, fade_index.data(), sizeof(int32_t) * fade_index.size()));
            PIRIP_TRY(m.upload(&h->d_fade_table, fade_tables.data(), sizeof(AirFadeTable) * fade_tables.size()));
        }
        return PIRIP_OK;
    };
    const int rc = tables();
    if (rc != PIRIP_OK) { delete h; return rc; }
    *out = h;
    return PIRIP_OK;
}

// what push will still take: the absolute index stays below 2^53, and a drifting handle's clock age inside its budget
int64_t samples_left(const pirip_hip_air *air)
{
    int64_t left = kAirMaxIndex - 1 - air->pos;
    if (air->drift) {
        const int64_t age = air->age0 + (air->pos - air->first);
        const int64_t by_slip = air->last_age < age ? 0 : air->last_age - age + 1;
        if (by_slip < left) left = by_slip;
    }
    return left < 0 ? 0 : left;
}

// the mix kernel of a handle's kind for one format pair; `lds` is the staging area's, a fade kernel has its grid points behind it
template <int BSI, int BSO>
void air_mix_launch(bool fade, bool drift, dim3 grid, size_t lds, hipStream_t st, const AirArgs &a, const AirDrift &d, const AirFade &f)
{
    const dim3 block(kAirThreads);
    if (fade) hipLaunchKernelGGL((air_mix_fade_kernel<BSI, BSO>), grid, block, lds + (size_t)kAirFadePoints * sizeof(float2), st, a, d, f);
    else if (drift) hipLaunchKernelGGL((air_mix_drift_kernel<BSI, BSO>), grid, block, lds, st, a, d);
    else hipLaunchKernelGGL((air_mix_kernel<BSI, BSO>), grid, block, lds, st, a);
}

}  // namespace

extern "C" {

int pirip_hip_air_create(int Fs, int in_format, int out_format, int ntx, int nrx, int npaths, const pirip_air_path *paths, const float *sigma,
                         uint64_t seed, int device, pirip_hip_air **out)
{
    std::vector<pirip_air_path_ex> ex;
    for (int p = 0; paths && p < npaths; p++) ex.push_back(pirip_air_path_ex{paths[p].rx, paths[p].tx, paths[p].delay, paths[p].offset_hz, paths[p].gain, 0});
    return air_create(Fs, in_format, out_format, ntx, nrx, npaths, paths ? ex.data() : nullptr, 0, nullptr, sigma, seed, 0, device, out);
}

int pirip_hip_air_create_ex(int Fs, int in_format, int out_format, int ntx, int nrx, int npaths, const pirip_air_path_ex *paths, const float *sigma,
                            uint64_t seed, int32_t max_slip, int device, pirip_hip_air **out)
{
    return air_create(Fs, in_format, out_format, ntx, nrx, npaths, paths, 0, nullptr, sigma, seed, max_slip, device, out);
}

int pirip_hip_air_create_fade(int Fs, int in_format, int out_format, int ntx, int nrx, int npaths, const pirip_air_path_ex *paths, int nfades,
                              const pirip_air_fade *fades, const float *sigma, uint64_t seed, int32_t max_slip, int device, pirip_hip_air **out)
{
    return air_create(Fs, in_format, out_format, ntx, nrx, npaths, paths, nfades, fades, sigma, seed, max_slip, device, out);
}

int pirip_hip_air_fade_table(int Fs, uint64_t seed, const pirip_air_fade *fade, int32_t w[16], uint32_t theta[16], float *scale, float *los)
{
    if (Fs < 2 || !fade || !w || !theta || !scale || !los || !fade_ok(*fade)) return PIRIP_ERR_BAD_ARG;
    if (fade->doppler_millihz > max_doppler_millihz(Fs)) return PIRIP_ERR_UNSUPPORTED;
    const AirFadeTable t = fade_table(Fs, seed, *fade);
    for (int j = 0; j < kAirScatter; j++) { w[j] = t.w[j]; theta[j] = t.theta[j]; }
    *scale = t.scale; *los = t.los;
    return PIRIP_OK;
}

int pirip_hip_air_interp_table(float *taps, int *nphases, int *ntaps)
{
    if (!taps) return PIRIP_ERR_BAD_ARG;
    const InterpTable &t = interp_table();
    for (int phi = 0; phi < kAirPhases; phi++)
        for (int k = 0; k < kAirTaps; k++) taps[phi * kAirTaps + k] = t.t[phi][k];
    if (nphases) *nphases = kAirPhases;
    if (ntaps) *ntaps = kAirTaps;
    return PIRIP_OK;
}

int pirip_hip_air_get_drift(const pirip_hip_air *air, int32_t *max_slip, int64_t *left)
{
    if (!air) return PIRIP_ERR_BAD_ARG;
    if (max_slip) *max_slip = air->max_slip;
    if (left) *left = samples_left(air);
    return PIRIP_OK;
}

int pirip_hip_air_reset_drift(pirip_hip_air *air, int64_t n0, int64_t age0, void *hip_stream)
{
    (void)hip_stream;                                                   // nothing to enqueue, as in pirip_hip_air_reset
    if (!air || n0 < 0 || age0 < 0) return PIRIP_ERR_BAD_ARG;
    if (n0 >= kAirMaxIndex || age0 >= kAirMaxIndex || (air->drift && age0 > air->last_age)) return PIRIP_ERR_UNSUPPORTED;
    air->pos = air->first = n0;
    air->age0 = age0;
    return PIRIP_OK;
}

int pirip_hip_air_destroy(pirip_hip_air *air) { return destroy_handle(air, air ? air->device : 0); }

int pirip_hip_air_get_info(const pirip_hip_air *air, pirip_air_info *info)
{
    if (!air || !info) return PIRIP_ERR_BAD_ARG;
    *info = pirip_air_info{air->Fs, air->ntx, air->nrx, air->npaths, air->in_format, air->out_format, air->max_delay, air->device};
    return PIRIP_OK;
}

int pirip_hip_air_set_sigma(pirip_hip_air *air, const float *sigma, void *hip_stream)
{
    if (!air || !sigma || !sigma_ok(sigma, air->nrx)) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(air->device)) return PIRIP_ERR_NO_DEVICE;
    PIRIP_HIPCHK(hipMemcpyAsync(air->d_sigma, sigma, sizeof(float) * (size_t)air->nrx, hipMemcpyHostToDevice, (hipStream_t)hip_stream));
    return PIRIP_OK;
}

int pirip_hip_air_push(pirip_hip_air *air, const void *d_in, size_t in_stride_bytes, int64_t n, void *d_out, size_t out_stride_bytes,
                       void *hip_stream)
{
    if (!air || !d_in || !d_out || n < 1) return PIRIP_ERR_BAD_ARG;
    PIRIP_TRY(iq_rows_check(d_in, in_stride_bytes, air->bsi, air->ntx, n));
    PIRIP_TRY(iq_rows_check(d_out, out_stride_bytes, air->bso, air->nrx, n));
    if (n >= kAirMaxIndex || air->pos + n >= kAirMaxIndex) return PIRIP_ERR_UNSUPPORTED;
    if (air->drift && n > samples_left(air)) return PIRIP_ERR_UNSUPPORTED;  // the call's last sample would take a path past max_slip
    const uintptr_t i0 = (uintptr_t)d_in, i1 = i0 + (size_t)(air->ntx - 1) * in_stride_bytes + (size_t)n * (size_t)air->bsi;
    const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + (size_t)(air->nrx - 1) * out_stride_bytes + (size_t)n * (size_t)air->bso;
    if (i0 < o1 && o0 < i1) return PIRIP_ERR_BAD_ARG;
    const int64_t ntiles = (n + kAirTile - 1) / kAirTile;
    if (ntiles > 0x7fffffff) return PIRIP_ERR_UNSUPPORTED;
    if (!bind_device(air->device)) return PIRIP_ERR_NO_DEVICE;
    AirArgs a{};
    a.in = (const char *)d_in; a.in_stride = in_stride_bytes;
    a.out = (char *)d_out; a.out_stride = out_stride_bytes;
    a.ring = air->d_ring; a.rings = air->d_rings; a.rx_start = air->d_rx_start; a.paths = air->d_paths; a.sigma = air->d_sigma;
    a.seed = air->seed; a.n = n; a.N0 = air->pos; a.first = air->first;
    a.n0m = (int32_t)fs_residue(air->pos, air->Fs);
    a.Fs = air->Fs; a.ntx = air->ntx;
    a.aligned16 = (((uintptr_t)d_out | out_stride_bytes) & 15) == 0;
    a.two_over_fs = 2.0f / (float)air->Fs; a.c_hi = air->u8.c_hi; a.c_lo = air->u8.c_lo;
    a.inv_fs_d = 1.0 / (double)air->Fs;
    hipStream_t st = (hipStream_t)hip_stream;
    const dim3 grid((unsigned)ntiles, (unsigned)air->nrx);
    // the staging area: a handle with a drifting path stages a longer span than the tile's
    const size_t lds = (size_t)(kAirTile + (air->drift ? kAirSpanExtra : 0)) * (size_t)air->bsi + 64;
    const AirDrift d{air->d_ppb, air->d_taps, air->age0 + (air->pos - air->first)};
    // a handle with a fading path: the tile's grid points behind the staging area
    const AirFade f{air->d_fade_index, air->d_fade_table, (int)lds};
    const auto launch = air->bsi == 2 ? (air->bso == 2 ? air_mix_launch<2, 2> : air_mix_launch<2, 8>)
                                      : (air->bso == 2 ? air_mix_launch<8, 2> : air_mix_launch<8, 8>);
    launch(air->fade, air->drift, grid, lds, st, a, d, f);
    // the carry: as many workgroups per transmitter as the longest ring and the call ask for (at most 64, which stride)
    const int64_t most = n < (int64_t)air->max_ring ? n : (int64_t)air->max_ring;
    int64_t cblocks = (most + kAirThreads - 1) / kAirThreads;
    if (cblocks > 64) cblocks = 64;
    const dim3 cgrid((unsigned)cblocks, (unsigned)air->ntx);
    if (air->bsi == 2) hipLaunchKernelGGL(air_carry_kernel<uint16_t>, cgrid, dim3(kAirThreads), 0, st, a);
    else hipLaunchKernelGGL(air_carry_kernel<float2>, cgrid, dim3(kAirThreads), 0, st, a);
    if (hipGetLastError() != hipSuccess) return PIRIP_ERR_HIP;
    air->pos += n;
    return PIRIP_OK;
}

int pirip_hip_air_reset(pirip_hip_air *air, int64_t n0, void *hip_stream)
{
    (void)hip_stream;                                                   // nothing to enqueue: the rings are masked by the index of the reset
    if (!air || n0 < 0) return PIRIP_ERR_BAD_ARG;
    if (n0 >= kAirMaxIndex) return PIRIP_ERR_UNSUPPORTED;
    air->pos = air->first = n0;
    air->age0 = 0;
    return PIRIP_OK;
}

}  // extern "C"
