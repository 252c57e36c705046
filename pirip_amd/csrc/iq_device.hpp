// pirip_amd/csrc/iq_device.hpp -- device primitives the rate changers share (gfx950 only): decimator, channelizer, multiplexer, modulator.
// One definition of each. The build has -ffp-contract=off: an explicit __builtin_fmaf, and an unfused product next to it, ARE the arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "demod_simd.hpp"   // v2f

namespace pirip {

typedef float v4f __attribute__((ext_vector_type(4)));
// ---- exact phase -----------------------------------------------------------------------------------------------------------------
// A stage that re-tunes by f Hz at rate Fs runs no phasor recursion: the phase of sample n is 2 pi p / Fs with the exact integer p = (f n) mod Fs,
// a function of the absolute index alone -- no drift, and any split of a row into calls gives the one-shot output bit for bit. Exact for
// Fs <= kMaxFs: residues fit a float, and the product of two a double.
constexpr int kMaxFs = 1 << 24;
// p mod Fs for an integer 0 <= p < 2^53 in a double (inv_fs = 1.0 / Fs): the quotient is right or one off, the remainder exact
__device__ __forceinline__ double mod_fs(double p, int Fs, double inv_fs)
{
    const double q = floor(p * inv_fs);
    double r = fma(-q, (double)Fs, p);
    if (r < 0.0) r += (double)Fs;
    if (r >= (double)Fs) r -= (double)Fs;
    return r;
}
// (a b) mod Fs for integers 0 <= a, b <= 2^24, whose product is exact in double; each caller converts its integer type at the call site
__device__ __forceinline__ double mulmod_fs(double a, double b, int Fs, double inv_fs) { return mod_fs(a * b, Fs, inv_fs); }

// (cos, sin)(pi p k_over_fs) for 0 <= p < Fs, centred into (-Fs/2, Fs/2] first: |p| <= 2^23 is exact in float and sincospi gets a fraction
// of pi in [-1, 1]. k_over_fs = 2 / Fs: e^{+j 2 pi p / Fs} (multiplexer, modulator); -2 / Fs: e^{-j 2 pi p / Fs} by negating the ARGUMENT
// (channelizer) -- not by conjugating the other result, which would be another sequence of float operations.
__device__ __forceinline__ void unit_phasor(int32_t p, int Fs, float k_over_fs, float &c, float &s)
{
    if (2 * p > Fs) p -= Fs;
    sincospif((float)p * k_over_fs, &s, &c);
}
// v (c + j s): one fma per component on an unfused product
__device__ __forceinline__ v2f crot(v2f v, float c, float s) { return v2f{__builtin_fmaf(v.x, c, -(v.y * s)), __builtin_fmaf(v.x, s, v.y * c)}; }

// ---- exact clock slip (the channel's drifting paths) -----------------------------------------------------------------------------------
// A stream read by a clock q parts per billion off is read, at clock age m, at m q / Q samples from where a static one is: S = floor(m q / Q)
// whole samples and rho = m q - Q S in [0, Q) billionths. Integers throughout: from one sample to the next rho moves by its exact
// increment q with one wrap (S +- 1), as the mixers' phase does -- no recursion in floating point. |m q| < 2^53 (mod_fs's way to a quotient).
constexpr int32_t kClockQ = 1000000000;
__device__ __forceinline__ void clock_slip(int64_t m, int32_t q, int64_t &S, int32_t &rho)
{
    const int64_t p = m * (int64_t)q;
    int64_t s = (int64_t)floor((double)p * 1e-9);                      // p is exact in a double: the quotient is right or one off
    int64_t r = p - s * kClockQ;                                        // ... and the remainder says which
    if (r < 0) { r += kClockQ; s -= 1; }
    if (r >= kClockQ) { r -= kClockQ; s += 1; }
    S = s; rho = (int32_t)r;
}
// one sample on, |q| <= kClockQ: rho + q stays inside an int32
__device__ __forceinline__ void clock_step(int32_t q, int32_t &S, int32_t &rho)
{
    rho += q;
    if (rho >= kClockQ) { rho -= kClockQ; S += 1; }
    if (rho < 0) { rho += kClockQ; S -= 1; }
}
// `steps` samples on in one go, for 0 <= steps |q| < 3 Q: at most three wraps
__device__ __forceinline__ void clock_advance(int32_t steps, int32_t q, int32_t &S, int32_t &rho)
{
    int64_t t = (int64_t)rho + (int64_t)steps * (int64_t)q;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (t >= kClockQ) { t -= kClockQ; S += 1; }
        if (t < 0) { t += kClockQ; S -= 1; }
    }
    rho = (int32_t)t;
}
// floor(phases rho / Q) for phases = 1024 = 2^10: Q / 2^10 = 1953125 / 2, so it is 2 rho / 1953125 in 32 bits (2 rho < 2^31)
__device__ __forceinline__ uint32_t clock_phase_1024(int32_t rho) { return (2u * (uint32_t)rho) / 1953125u; }

// ---- sample formats in -----------------------------------------------------------------------------------------------------------
// csdr's convert_u8_f, x / 127.5 - 1 in double rounded to float, as two fmas: c_hi is 1 / 127.5 rounded to a multiple of 2^-22 (the inner fma
// is then exact for every byte value), c_lo the float remainder; bit-identical to the double formula for all 256 bytes (rate_host.hpp's
// csdr_u8_split derives the constants and checks that). x: the byte's value as a float. v2f form: one v_pk_fma_f32 per fma for an (I, Q) pair,
// its constants splatted by the caller (once, outside its loops).
__device__ __forceinline__ float u8_to_float(float x, float c_hi, float c_lo) { return __builtin_fmaf(x, c_lo, __builtin_fmaf(x, c_hi, -1.0f)); }
__device__ __forceinline__ v2f u8_to_float(v2f x, v2f c_hi, v2f c_lo) { return __builtin_elementwise_fma(x, c_lo, __builtin_elementwise_fma(x, c_hi, v2f{-1.0f, -1.0f})); }

// ---- sample formats out: four conversions, each the arithmetic of what its stage stands in for. The differences are deliberate. ------
// csdr's convert_f_s16 as csdr does it (the decimator, section B): v * 32767 truncated, no clamp
__device__ __forceinline__ short f_to_s16_csdr(float v) { return (short)(v * (float)SHRT_MAX); }
// the channelizer's (section H): the same product clamped to the s16 range, then truncated
__device__ __forceinline__ short f_to_s16_clamped(float v) { return (short)fminf(fmaxf(v * (float)SHRT_MAX, -32768.0f), 32767.0f); }
// fsk_mod's byte (synthetic and batch transmitter): clamp(rintf(127 + amp v)); the byte's value, still a float
__device__ __forceinline__ float quant_u8(float v, float amp) { return fminf(fmaxf(rintf(127.0f + amp * v), 0.f), 255.f); }
// the multiplexer's csdr-style byte (section J), the inverse of convert_u8_f: clamp(rintf(127.5 v + 127.5)), product and sum rounded separately
__device__ __forceinline__ float quant_u8_csdr(float v) { return fminf(fmaxf(rintf(127.5f * v + 127.5f), 0.f), 255.f); }

}  // namespace pirip
