// pirip_amd/csrc/demod_frame.hpp -- per-frame values and arithmetic that the workgroup-per-stream demodulators (fsk_demod_block.hip,
// fsk_demod_general.hip) hand from stage to stage: one definition of what is the same expression in both (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "fsk_device.hpp"

namespace pirip {

struct Tones { float f_est[kMaxTones]; uint32_t dtheta[kMaxTones]; int drift_ix[kMaxTones]; };   // a frame's tone estimates: Hz, phase step, oscillator-table row
struct Timing { int nin_next, low_sample, high_sample; float fract; };
struct SymbolSums { float sig, nse, mean_e, std_e; };

// one tone's power in a symbol: f_int interpolated between the two windows round the timing estimate, squared
__device__ __forceinline__ float tone_power(float2 lo, float2 hi, float fract)
{
    float2 r;
    r.x = (1 - fract) * lo.x; r.y = (1 - fract) * lo.y;
    r.x = r.x + fract * hi.x; r.y = r.y + fract * hi.y;
    return (r.x * r.x) + (r.y * r.y);
}

// a frame's symbol sums (rx_nse_pow seeded with 1e-12 by the caller) into the SNR scalars
__device__ __forceinline__ void update_snr(StreamScalars &sc, SymbolSums s, int Nsym)
{
    const float sig = s.sig / (float)Nsym, nse = s.nse / (float)Nsym, mean_e = s.mean_e / (float)Nsym;
    sc.v_est = sqrtf(sig - nse);
    sc.SNRest = sig / nse;
    sc.rx_sig_pow = sig; sc.rx_nse_pow = nse;
    float std_e = (s.std_e / (float)Nsym) - (mean_e * mean_e);
    std_e = std_e > 0.0f ? sqrtf(std_e) : 0.0f;
    sc.EbNodB = -6.0f + (20.0f * log10f((1e-6f + mean_e) / (1e-6f + std_e)));
    sc.snr_est = (0.5f * sc.snr_est) + (0.5f * sc.EbNodB);
}

// a frame's stats row (PIRIP_STATS_PER_FRAME floats; P: a pointer to float in the caller's address space)
template <class P>
__device__ __forceinline__ void write_stats_row(P stats, const float (&f_est)[kMaxTones], float norm_rx_timing, float SNRest, int nin_next, float ppm,
                                                float rx_sig_pow, float rx_nse_pow)
{
    stats[0] = f_est[0]; stats[1] = f_est[1]; stats[2] = f_est[2]; stats[3] = f_est[3];
    stats[4] = norm_rx_timing; stats[5] = SNRest; stats[6] = (float)nin_next; stats[7] = ppm;
    stats[8] = rx_sig_pow; stats[9] = rx_nse_pow;
}

}  // namespace pirip
