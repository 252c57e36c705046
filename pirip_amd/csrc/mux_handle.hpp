// pirip_amd/csrc/mux_handle.hpp -- the multiplexer's handle behind include/pirip_hip.h's opaque pirip_hip_mux and the body of its kernel,
// shared by mux_kernels.hip (section J: the staged samples are read from modem-rate rows) and txs_kernels.hip (section K: they are
// computed from symbol rows). Library-private; the kernel's description is at the top of mux_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "hip_host.hpp"
#include "iq_device.hpp"
#include "rate_host.hpp"

// (hidden: a handle's implicit destructor is no dynamic symbol of the library)
#pragma GCC visibility push(hidden)
struct pirip_hip_mux {
    int Fs = 0, D = 0, kind = 0, L = 0, Q = 0, Dp = 0, Mt = 0, G = 0, out_format = 0, bs = 0, device = 0, noutputs = 0, nchan = 0;
    size_t lds = 0;
    std::vector<float> h;                  // prototype taps (L)
    pirip::DevMem mem;
    pirip::v2f *d_taps = nullptr;
    int32_t *d_out_start = nullptr, *d_out_ch = nullptr, *d_sc = nullptr;
};

namespace pirip {

constexpr int kMuxThreads = 256;
constexpr int kMuxPerThread = 8;           // outputs per thread and tile (accumulator pairs)
constexpr int kMuxTile = kMuxThreads * kMuxPerThread;
constexpr int kMuxMaxGroup = 8;            // channels staged together
constexpr size_t kMuxLdsMax = 64 * 1024;

struct MuxArgs {
    int64_t n_out;
    char *out; size_t out_stride;
    const v2f *taps;                       // [nchan][Q][Dp] g_c, each row of D followed by its first Dp - D entries
    const int32_t *out_start;              // [noutputs + 1]: the channels of output i are out_ch[out_start[i] .. out_start[i + 1])
    const int32_t *out_ch;                 // [nchan] channel indices, ascending within an output
    const int32_t *sc;                     // [nchan] (f_c mod Fs) D mod Fs
    int Fs, D, Dp, Q, Mt, G, aligned16;
    int step_m, step_p;                    // 256 div D, 256 mod D
    int32_t m0m;                           // m0 mod Fs
    float two_over_fs;
    double inv_fs_d;
};

// everything of a call's arguments that the handle and the output rows decide: n_out outputs per output from absolute input index m0 on
inline void mux_fill_args(const pirip_hip_mux *mx, int64_t n_out, int64_t m0, void *d_out, size_t out_stride_bytes, MuxArgs *a)
{
    a->n_out = n_out;
    a->out = (char *)d_out; a->out_stride = out_stride_bytes;
    a->taps = mx->d_taps; a->out_start = mx->d_out_start; a->out_ch = mx->d_out_ch; a->sc = mx->d_sc;
    a->Fs = mx->Fs; a->D = mx->D; a->Dp = mx->Dp; a->Q = mx->Q; a->Mt = mx->Mt; a->G = mx->G;
    a->aligned16 = (((uintptr_t)d_out | out_stride_bytes) & 15) == 0;
    a->step_m = kMuxThreads / mx->D; a->step_p = kMuxThreads % mx->D;
    a->m0m = (int32_t)fs_residue(m0, mx->Fs);
    a->two_over_fs = 2.0f / (float)mx->Fs; a->inv_fs_d = 1.0 / (double)mx->Fs;
}

// One workgroup, one (tile, output). BS: bytes per output sample, 2 (u8 IQ) or 8 (complex float). Stage: where input sample `at` of the
// call (absolute index m0 + at) of channel ch comes from -- st.begin(a0, tid) is the thread's cursor at input a0 + tid of the call,
// st.next moves it on by kMuxThreads inputs, st.sample(ch, cursor, at) is the sample; zero outside the call's row.
template <int BS, typename Stage>
__device__ __forceinline__ void mux_tile(const MuxArgs &a, const Stage &st)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *s_out = smem;                                                 // [kMuxTile] samples as they are stored
    v2f *s_g = (v2f *)(smem + (size_t)kMuxTile * BS);                   // [G][Q * Dp]
    const int tapsz = a.Q * a.Dp;
    v2f *s_z = s_g + (size_t)a.G * tapsz;                               // [G][Mt]
    const int tid = threadIdx.x;
    const int i = blockIdx.y;
    const int64_t j0 = (int64_t)blockIdx.x * kMuxTile;                  // first output of the tile (of this call)
    const int cnt = (int)((a.n_out - j0) < kMuxTile ? (a.n_out - j0) : kMuxTile);
    // output j of the call is absolute n = (m0 + Q - 1) D + j: p = j mod D, and its newest input sample is input Q - 1 + j div D of the call
    const int64_t a0 = j0 / a.D;
    const int p0 = (int)(j0 - a0 * a.D);
    const int mt = (p0 + cnt - 1) / a.D + a.Q;                          // input samples of the tile, from input a0 of the call on
    const int32_t base = (int32_t)(((int64_t)a.m0m + a0 % a.Fs) % a.Fs);
    const int m_first = (p0 + tid) / a.D, p_first = (p0 + tid) - m_first * a.D;
    const int lane32 = tid & 31;
    const typename Stage::Cursor cur0 = st.begin(a0, tid);
    v2f acc[kMuxPerThread];
#pragma unroll
    for (int k = 0; k < kMuxPerThread; k++) acc[k] = v2f{0.f, 0.f};

    const int c0 = a.out_start[i], c1 = a.out_start[i + 1];
    for (int cb = c0; cb < c1; cb += a.G) {
        const int ng = c1 - cb < a.G ? c1 - cb : a.G;
        if (cb > c0) __syncthreads();
        for (int m = 0; m < ng; m++) {
            const int ch = a.out_ch[cb + m];
            const v2f *g = a.taps + (size_t)ch * tapsz;
            for (int e = tid; e < tapsz; e += kMuxThreads) s_g[(size_t)m * tapsz + e] = g[e];
            const int32_t s = a.sc[ch];
            typename Stage::Cursor cur = cur0;
            for (int r = tid; r < mt; r += kMuxThreads, st.next(cur)) {
                const float2 v = st.sample(ch, cur, a0 + r);
                const int32_t idx = (int32_t)(((uint32_t)base + (uint32_t)r) % (uint32_t)a.Fs);
                float sn, cs;
                unit_phasor((int32_t)mulmod_fs(s, idx, a.Fs, a.inv_fs_d), a.Fs, a.two_over_fs, cs, sn);
                s_z[(size_t)m * a.Mt + r] = crot(v2f{v.x, v.y}, cs, sn);
            }
        }
        __syncthreads();
        int mm = m_first, pp = p_first;
#pragma unroll
        for (int k = 0; k < kMuxPerThread; k++) {
            if (k * kMuxThreads + tid < cnt) {
                const int e = (a.Dp != a.D && pp < lane32) ? pp + a.D : pp;
                for (int m = 0; m < ng; m++) {
                    const v2f *g = s_g + (size_t)m * tapsz + e;
                    const v2f *z = s_z + (size_t)m * a.Mt + mm + a.Q - 1;
                    v2f u = {0.f, 0.f};
                    for (int q = 0; q < a.Q; q++, g += a.Dp, z--) {
                        const v2f gg = *g, zz = *z;
                        u = __builtin_elementwise_fma(v2f{zz.x, zz.x}, gg, u);
                        u = __builtin_elementwise_fma(v2f{zz.y, zz.y}, v2f{-gg.y, gg.x}, u);
                    }
                    acc[k] += u;
                }
            }
            pp += a.step_p; mm += a.step_m;
            if (pp >= a.D) { pp -= a.D; mm++; }
        }
    }

    // the tile as it is stored, through LDS: thread t holds outputs k * 256 + t, and stores 16 consecutive bytes
#pragma unroll
    for (int k = 0; k < kMuxPerThread; k++) {
        const int n = k * kMuxThreads + tid;
        if (BS == 2) ((uint16_t *)s_out)[n] = (uint16_t)((uint32_t)quant_u8_csdr(acc[k].x) | ((uint32_t)quant_u8_csdr(acc[k].y) << 8));
        else ((v2f *)s_out)[n] = acc[k];
    }
    __syncthreads();
    constexpr int SPU = 16 / BS;                                        // samples per 16-byte unit
    char *row = a.out + (size_t)i * a.out_stride + (size_t)j0 * BS;
    for (int u = tid; u * SPU < cnt; u += kMuxThreads) {
        const int first = u * SPU;
        if (a.aligned16 && first + SPU <= cnt) {
            *(uint4 *)(row + (size_t)u * 16) = *(const uint4 *)(s_out + (size_t)u * 16);
        } else {
            for (int n = first; n < first + SPU && n < cnt; n++) {
                if (BS == 2) ((uint16_t *)row)[n] = ((const uint16_t *)s_out)[n];
                else ((float2 *)row)[n] = ((const float2 *)s_out)[n];
            }
        }
    }
}

}  // namespace pirip
#pragma GCC visibility pop
