// pirip_amd/csrc/tx_kernels.hip -- include/pirip_hip.h section I: the batch FSK_LDPC transmitter.
//
//   records (rpitx_fsk --code's stdin protocol)  --frame-->  channel symbols  --modulate-->  IQ (u8 or complex float)
//
// Stage 1, the framer: what fsk_ldpc_framer --packed does to a record stream, for every stream of the batch. A record is one burst-control
// byte and k/8 packed data bytes (1: preamble + frame, 0: frame, 2: carrier off for the stream's gap, nothing sent). tx_layout_kernel
// (one wave per stream) turns the control bytes into each record's place in the symbol row by a wave prefix sum; tx_frame_kernel
// (one wave per (stream, record)) forms UW | data + CRC16 | parity in LDS and writes symbols (and, on request, the framer's bits).
// The arithmetic is fsk_ldpc.cpp's: crc16_ccitt over the k/8 - 2 packed bytes (one lane: 30 bytes for the (512,256) code), and
// LdpcCode::encode -- parity[p] = parity[p-1] ^ (XOR of row p's data columns). Lane l forms the data-column XOR of rows 64c + l from the
// CSR; the running XOR across rows is then a prefix XOR inside the wave: one ballot per 64 rows, each lane takes the popcount parity of
// the lanes at or below it, and the carry into the next 64 rows is the ballot's own parity. No LDS round trip per row.
//
// Stage 2, the modulator: continuous-phase M-FSK, parallel in the samples. With f_i the tone of symbol i in Hz (an integer mod Fs) the
// phase after sample r of symbol i is 2 pi p / Fs with the exact integer
//     p = (A_i + (r + 1) f_i) mod Fs,      A_i = (phase carried in + Ts * sum_{q < i} f_q) mod Fs
// (the advance comes before the output, as in fsk_mod_c: the first sample is one step in). tx_prefix_kernel (one workgroup per stream)
// forms A_i by an exclusive scan of (Ts f_q mod Fs) in wave and across waves, in 32-bit integers, and leaves the row's final phase in
// the handle; tx_mod_kernel gives each lane one 16-byte unit of output (8 u8 samples or 2 complex floats): one exact (r + 1) f mod Fs
// in double, then p += f (mod Fs) from sample to sample, x = 2 (cospi, sinpi)(2p/Fs). Carrier-off symbols (0xFF) add nothing to the
// phase and give x = 0. No float recursion: a sample is a function of the symbols before it and of nothing else, so a row sent in one
// call or in several gives the same bytes. Optional AWGN is synth_kernels.hip's counter generator with its key (seed, stream, sample).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/pirip_hip.h"
#include "fsk_ldpc.hpp"
#include "hip_host.hpp"
#include "iq_device.hpp"
#include "noise_device.hpp"
#include "rate_host.hpp"
#include "repeat_device.hpp"
#include "tx_handle.hpp"

using namespace pirip;

namespace {

constexpr int kFrameWaves = 4;             // records per workgroup of the framer
constexpr int kModThreads = 256;
constexpr uint8_t kOff = 0xFF;             // carrier off

struct FrameArgs {
    const uint8_t *rec; size_t rec_stride; const int32_t *nrec; int max_rec;
    int32_t *off;                          // [nstreams][max_rec] first symbol of each record
    uint8_t *syms; size_t sym_stride; int64_t max_syms; int32_t *nsym;
    uint8_t *bits; size_t bits_stride;     // optional: one bit per byte, zeros over the gaps (fsk_ldpc_framer's output)
    const int32_t *row_ptr, *col_idx;      // CSR of H
    const int32_t *lead, *gap;             // [nstreams] carrier-off symbols in front of the first burst / for every `2` record
    uint32_t uw;                           // unique word, first bit in bit 31
    int k, m, kb, bpf, bps, pre_bits, nstreams, wave_lds, frame_lds;
};

// carrier off over symbols [from, from + n) of stream s, clipped to the row
__device__ __forceinline__ void write_off(const FrameArgs &a, int s, int64_t from, int64_t n, int lane)
{
    uint8_t *sy = a.syms + (size_t)s * a.sym_stride;
    for (int64_t i = from + lane; i < from + n && i < a.max_syms; i += 64) sy[i] = kOff;
    if (a.bits) {
        uint8_t *b = a.bits + (size_t)s * a.bits_stride;
        const int64_t b0 = from * a.bps, b1 = (from + n) * a.bps, bmax = a.max_syms * a.bps;
        for (int64_t i = b0 + lane; i < b1 && i < bmax; i += 64) b[i] = 0;
    }
}

__global__ __launch_bounds__(64) void tx_layout_kernel(FrameArgs a)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    const int nrec = row_count(a.nrec, s, a.max_rec);
    const int lead = a.lead[s] > 0 ? a.lead[s] : 0, gap = a.gap[s] > 0 ? a.gap[s] : 0;
    const int fsyms = a.bpf / a.bps, psyms = a.pre_bits / a.bps;
    write_off(a, s, 0, lead, lane);
    const uint8_t *rec = a.rec + (size_t)s * a.rec_stride;
    int64_t carry = lead;
    for (int base = 0; base < nrec; base += 64) {
        const int r = base + lane;
        int len = 0;
        if (r < nrec) len = tx_record_syms(rec[(size_t)r * (size_t)(1 + a.kb)], psyms, fsyms, gap);
        int64_t incl = len;
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        const int64_t o = carry + incl - len;
        if (r < nrec) a.off[(size_t)s * a.max_rec + r] = (int32_t)(o < a.max_syms ? o : a.max_syms);
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0 && a.nsym) a.nsym[s] = (int32_t)(carry < a.max_syms ? carry : a.max_syms);
}

__device__ __forceinline__ uint16_t crc16_step(uint16_t crc, uint8_t byte)   // fsk_ldpc.cpp: crc16_ccitt
{
    uint8_t x = (uint8_t)((uint8_t)(crc >> 8) ^ byte);
    x ^= x >> 4;
    return (uint16_t)((crc << 8) ^ ((uint16_t)x << 12) ^ ((uint16_t)x << 5) ^ (uint16_t)x);
}

// bits [0, nbits) at `src` (one per byte, LDS or generated) -> symbols from `sym0` on and bits from sym0 * bps on, clipped to the row
template <typename F>
__device__ __forceinline__ void emit(const FrameArgs &a, int s, int64_t sym0, int nbits, int lane, F bit)
{
    uint8_t *sy = a.syms + (size_t)s * a.sym_stride;
    const int ns = nbits / a.bps;
    for (int i = lane; i < ns && sym0 + i < a.max_syms; i += 64)
        sy[sym0 + i] = a.bps == 1 ? bit(i) : (uint8_t)((bit(2 * i) << 1) | bit(2 * i + 1));
    if (a.bits) {
        uint8_t *b = a.bits + (size_t)s * a.bits_stride;
        const int64_t b0 = sym0 * a.bps, bmax = a.max_syms * a.bps;
        for (int i = lane; i < nbits && b0 + i < bmax; i += 64) b[b0 + i] = bit(i);
    }
}

__global__ __launch_bounds__(kFrameWaves * 64) void tx_frame_kernel(FrameArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int s = blockIdx.y, r = blockIdx.x * kFrameWaves + wave;
    uint8_t *s_frame = smem + (size_t)wave * a.wave_lds;    // [bpf] UW | data | parity, one bit per byte
    uint8_t *s_bytes = s_frame + a.frame_lds;               // [kb] the record's packed data
    const bool live = r < row_count(a.nrec, s, a.max_rec);
    const uint8_t *rec = a.rec + (size_t)s * a.rec_stride + (size_t)(live ? r : 0) * (size_t)(1 + a.kb);
    const uint8_t ctl = live ? rec[0] : 3;
    const bool frame = ctl == 0 || ctl == 1;
    if (frame) for (int i = lane; i < a.kb; i += 64) s_bytes[i] = rec[1 + i];
    __syncthreads();
    if (frame && lane == 0) {                               // insert_crc: the last 16 data bits are the CRC16 of the bytes before them
        uint16_t crc = 0xFFFF;
        for (int i = 0; i < a.kb - 2; i++) crc = crc16_step(crc, s_bytes[i]);
        s_bytes[a.kb - 2] = (uint8_t)(crc >> 8);
        s_bytes[a.kb - 1] = (uint8_t)(crc & 0xff);
    }
    __syncthreads();
    if (frame)
        for (int i = lane; i < kUwBits + a.k; i += 64)
            s_frame[i] = i < kUwBits ? (uint8_t)((a.uw >> (31 - i)) & 1u)
                                     : (uint8_t)((s_bytes[(i - kUwBits) >> 3] >> (7 - ((i - kUwBits) & 7))) & 1);
    __syncthreads();
    if (frame) {                                            // LdpcCode::encode
        const uint8_t *data = s_frame + kUwBits;
        uint8_t *par = s_frame + kUwBits + a.k;
        unsigned carry = 0;
        for (int base = 0; base < a.m; base += 64) {
            const int p = base + lane;
            unsigned d = 0;
            if (p < a.m)
                for (int e = a.row_ptr[p]; e < a.row_ptr[p + 1]; e++) {
                    const int c = a.col_idx[e];
                    if (c < a.k) d ^= data[c];
                }
            const unsigned long long mask = __ballot(d & 1u);
            const unsigned long long below = lane == 63 ? mask : (mask & ((2ull << lane) - 1ull));
            if (p < a.m) par[p] = (uint8_t)((carry ^ (unsigned)__popcll(below)) & 1u);
            carry ^= (unsigned)__popcll(mask) & 1u;
        }
    }
    __syncthreads();
    if (!live) return;
    const int64_t o = a.off[(size_t)s * a.max_rec + r];
    if (ctl == 2) {
        write_off(a, s, o, a.gap[s] > 0 ? a.gap[s] : 0, lane);
    } else if (frame) {
        int64_t at = o;
        if (ctl == 1) {                                     // preamble_bits(M): symbols 0, 1, 2, 3, 0, ... two bits each
            emit(a, s, at, a.pre_bits, lane, [](int i) { const int sym = i >> 1; return (uint8_t)((i & 1) ? (sym & 1) : ((sym >> 1) & 1)); });
            at += a.pre_bits / a.bps;
        }
        emit(a, s, at, a.bpf, lane, [&](int i) { return s_frame[i]; });
    }
}

// ---------------------------------------------------------------- modulator

struct ModArgs {
    const uint8_t *syms; size_t sym_stride; const int32_t *nsym;
    int64_t total;                         // symbols sent per stream in this call (symbols from nsym[s] on are carrier off)
    uint32_t *prefix;                      // [nstreams][total] A_i
    uint32_t *phase;                       // [nstreams] phase integer carried from call to call
    const uint32_t *fm, *tm;               // [nstreams][4] tone m mod Fs, (Ts * tone m) mod Fs
    void *out; size_t out_stride;
    int64_t n0;                            // samples sent per stream before this call (the noise key)
    int Fs, Ts, M, nstreams, aligned16;
    float two_over_fs, amp, sigma;
    double inv_fs_d;
    uint64_t seed;
};

__device__ __forceinline__ int sym_at(const ModArgs &a, const uint8_t *sy, int valid, int64_t i)
{
    const int v = i < valid ? sy[i] : kOff;
    return v < a.M ? v : -1;               // -1: carrier off
}

__global__ __launch_bounds__(kScanThreads) void tx_prefix_kernel(ModArgs a)
{
    __shared__ uint32_t s_tot[kScanThreads / 64];
    const int s = blockIdx.x;
    const uint8_t *sy = a.syms + (size_t)s * a.sym_stride;
    int64_t valid = a.nsym ? a.nsym[s] : a.total;
    if (valid > a.total) valid = a.total;
    const uint32_t carry = tx_scan_row([&](int64_t i) { return sym_at(a, sy, (int)valid, i); }, a.total, a.tm + (size_t)s * 4, (uint32_t)a.Fs,
                                       a.phase[s], a.prefix + (size_t)s * (size_t)a.total, s_tot);
    if (threadIdx.x == 0) a.phase[s] = carry;
}

// One sample: x = 2 e^{j 2 pi p / Fs} (0 when the carrier is off), plus the noise of (stream, absolute sample)
__device__ __forceinline__ float2 sample(const ModArgs &a, bool on, uint32_t p, int s, int64_t nabs)
{
    float xr = 0.f, xi = 0.f;
    if (on) {
        float sn, cs;
        unit_phasor((int32_t)p, a.Fs, a.two_over_fs, cs, sn);
        xr = 2 * cs; xi = 2 * sn;
    }
    if (a.sigma > 0.f) add_awgn(a.seed, s, nabs, a.sigma, xr, xi);      // synth_kernels.hip's generator and key
    return make_float2(xr, xi);
}

__device__ __forceinline__ uint32_t quant(float v, float amp) { return (uint32_t)quant_u8(v, amp); }

// SPU samples per 16-byte unit: 8 (u8 IQ) or 2 (complex float)
template <int SPU>
__global__ __launch_bounds__(kModThreads) void tx_mod_kernel(ModArgs a)
{
    const int s = blockIdx.y + blockIdx.z * 65535;
    if (s >= a.nstreams) return;
    const int64_t nsamp = a.total * a.Ts;
    const int64_t first = ((int64_t)blockIdx.x * kModThreads + threadIdx.x) * SPU;
    if (first >= nsamp) return;
    const uint8_t *sy = a.syms + (size_t)s * a.sym_stride;
    const uint32_t *pre = a.prefix + (size_t)s * (size_t)a.total;
    int64_t valid = a.nsym ? a.nsym[s] : a.total;
    if (valid > a.total) valid = a.total;
    const uint32_t Fs = (uint32_t)a.Fs;
    int64_t i = first / a.Ts;
    int r = (int)(first - i * a.Ts);
    int sym = sym_at(a, sy, (int)valid, i);
    uint32_t f = sym < 0 ? 0u : a.fm[(size_t)s * 4 + sym];
    uint32_t p = pre[i] + (uint32_t)mulmod_fs((uint32_t)r, f, a.Fs, a.inv_fs_d);     // the phase after r samples of symbol i
    if (p >= Fs) p -= Fs;
    float2 x[SPU];
    const int cnt = (int)(nsamp - first < SPU ? nsamp - first : SPU);
#pragma unroll
    for (int j = 0; j < SPU; j++) {
        if (j < cnt) {
            if (r == a.Ts) {
                i++; r = 0;
                sym = sym_at(a, sy, (int)valid, i);
                f = sym < 0 ? 0u : a.fm[(size_t)s * 4 + sym];
                p = pre[i];
            }
            p += f;
            if (p >= Fs) p -= Fs;
            r++;
            x[j] = sample(a, sym >= 0, p, s, a.n0 + first + j);
        } else {
            x[j] = make_float2(0.f, 0.f);
        }
    }
    char *row = (char *)a.out + (size_t)s * a.out_stride;
    if (SPU == 8) {
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; q++)
            w[q] = quant(x[2 * q].x, a.amp) | (quant(x[2 * q].y, a.amp) << 8) | (quant(x[2 * q + 1].x, a.amp) << 16) | (quant(x[2 * q + 1].y, a.amp) << 24);
        if (a.aligned16 && cnt == SPU) {
            *(uint4 *)(row + 2 * first) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int j = 0; j < SPU; j++) if (j < cnt) *(uint16_t *)(row + 2 * (first + j)) = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
        }
    } else {
        if (a.aligned16 && cnt == SPU) {
            *(float4 *)(row + 8 * first) = make_float4(x[0].x, x[0].y, x[SPU - 1].x, x[SPU - 1].y);
        } else {
#pragma unroll
            for (int j = 0; j < SPU; j++) if (j < cnt) *(float2 *)(row + 8 * (first + j)) = x[j];
        }
    }
}


// ---------------------------------------------------------------- receiver records -> Tx records (tx/frame_repeater.c:68-107)

struct RepeatArgs {
    RepeatIn in;
    uint8_t *rec; size_t rec_stride; int max_rec; int32_t *nrec;
};

// One wave per stream: repeat_device.hpp's body, with the bursts where the walk laid them out in the stream's row of records.
__global__ __launch_bounds__(64) void tx_repeat_kernel(RepeatArgs a)
{
    const int s = blockIdx.x;
    uint8_t *out = a.rec + (size_t)s * a.rec_stride;
    const int rl = 1 + a.in.kb;
    const int nout = repeat_stream(a.in, s, [](uint8_t v, const uint8_t *) { return v; }, [](int, int32_t *, const int32_t *) {},
                                   [&](int base, int j) { return base + j < a.max_rec ? out + (size_t)(base + j) * rl : nullptr; });
    if (threadIdx.x == 0 && a.nrec) a.nrec[s] = nout;
}

}  // namespace

namespace {

// a work buffer of `want` elements at least; calls in flight may still use the one it replaces
template <typename T>
int tx_grow(pirip_hip_tx *h, T **buf, size_t *cap, size_t want)
{
    if (want <= *cap) return PIRIP_OK;
    return grow_dev(h->mem, cap, want, *buf ? GrowSync::device : GrowSync::none, nullptr, {grow_buf(buf, want * sizeof(T))});
}

// the code's CSR and the per-stream settings of a new handle, zeroed
int tx_alloc(pirip_hip_tx *h)
{
    const size_t S = (size_t)h->nstreams;
    DevMem &m = h->mem;
    PIRIP_TRY(m.upload(&h->d_row_ptr, h->code.row_ptr.data(), sizeof(int32_t) * h->code.row_ptr.size()));
    PIRIP_TRY(m.upload(&h->d_col_idx, h->code.col_idx.data(), sizeof(int32_t) * h->code.col_idx.size()));
    PIRIP_TRY(m.alloc_filled(&h->d_lead, 0, sizeof(int32_t) * S));
    PIRIP_TRY(m.alloc_filled(&h->d_gap, 0, sizeof(int32_t) * S));
    PIRIP_TRY(m.alloc(&h->d_nsym, sizeof(int32_t) * S));
    PIRIP_TRY(m.alloc_filled(&h->d_fm, 0, sizeof(uint32_t) * 4 * S));
    PIRIP_TRY(m.alloc_filled(&h->d_tm, 0, sizeof(uint32_t) * 4 * S));
    PIRIP_TRY(m.alloc_filled(&h->d_phase, 0, sizeof(uint32_t) * S));
    PIRIP_HIPCHK(hipDeviceSynchronize());
    return PIRIP_OK;
}

}  // namespace

// symbols a row of max_rec records can need behind max_lead symbols of lead
int64_t pirip::tx_row_syms(const pirip_hip_tx *h, int max_rec, int max_lead)
{
    const int64_t per_frame = tx_pre_syms(h) + tx_frame_syms(h);
    return (int64_t)max_lead + (int64_t)max_rec * (per_frame > h->max_gap ? per_frame : (int64_t)h->max_gap);
}

// what stage 1 asks of its rows, before anything touches the device
int pirip::tx_frame_check(const pirip_hip_tx *h, size_t rec_stride, int max_rec, size_t sym_stride, int64_t max_syms, bool bits, size_t bits_stride)
{
    if (sym_stride < (size_t)max_syms || (bits && bits_stride < (size_t)max_syms * h->bps)) return PIRIP_ERR_BAD_ARG;
    if (rec_stride < (size_t)max_rec * (size_t)(1 + h->code.data_bytes())) return PIRIP_ERR_BAD_ARG;
    if (max_syms > 0x7fffffff || (max_rec + kFrameWaves - 1) / kFrameWaves > 65535 || h->nstreams > 65535) return PIRIP_ERR_UNSUPPORTED;
    return PIRIP_OK;
}

// Stage 1 on rows, leads and a record-offset table ([nstreams][max_rec]) of the caller's, checked by tx_frame_check; the handle's device is current
int pirip::tx_frame_rows(pirip_hip_tx *h, const uint8_t *d_records, size_t rec_stride, const int32_t *d_nrec, int max_rec,
                         uint8_t *d_syms, size_t sym_stride, int64_t max_syms, int32_t *d_nsym, uint8_t *d_bits, size_t bits_stride,
                         const int32_t *d_lead, int32_t *d_off, hipStream_t st)
{
    FrameArgs a{};
    a.rec = d_records; a.rec_stride = rec_stride; a.nrec = d_nrec; a.max_rec = max_rec; a.off = d_off;
    a.syms = d_syms; a.sym_stride = sym_stride; a.max_syms = max_syms; a.nsym = d_nsym;
    a.bits = d_bits; a.bits_stride = bits_stride;
    a.row_ptr = h->d_row_ptr; a.col_idx = h->d_col_idx; a.lead = d_lead; a.gap = h->d_gap;
    a.uw = 0;
    for (int i = 0; i < kUwBits; i++) a.uw |= (uint32_t)(h->code.uw[i] & 1) << (31 - i);
    a.k = h->code.k; a.m = h->code.m; a.kb = h->code.data_bytes(); a.bpf = h->code.bits_per_frame(); a.bps = h->bps;
    a.pre_bits = h->pre_bits; a.nstreams = h->nstreams;
    a.frame_lds = (a.bpf + 15) & ~15;
    a.wave_lds = a.frame_lds + ((a.kb + 15) & ~15);
    hipLaunchKernelGGL(tx_layout_kernel, dim3((unsigned)h->nstreams), dim3(64), 0, st, a);
    if (max_rec > 0)
        hipLaunchKernelGGL(tx_frame_kernel, dim3((unsigned)((max_rec + kFrameWaves - 1) / kFrameWaves), (unsigned)h->nstreams), dim3(kFrameWaves * 64),
                           (size_t)kFrameWaves * a.wave_lds, st, a);
    PIRIP_HIPCHK(hipGetLastError());
    return PIRIP_OK;
}

extern "C" {

int pirip_hip_tx_create(const char *code_path, int Fs, int Rs, int M, int nstreams, int device, pirip_hip_tx **out)
{
    if (!out) return PIRIP_ERR_BAD_ARG;
    *out = nullptr;
    if (!code_path || nstreams <= 0) return PIRIP_ERR_BAD_ARG;
    if (Fs <= 0 || Rs <= 0 || Fs % Rs || (M != 2 && M != 4)) return PIRIP_ERR_BAD_CONFIG;
    pirip_hip_tx *h = new (std::nothrow) pirip_hip_tx();
    if (!h) return PIRIP_ERR_NOMEM;
    const std::string err = h->code.load(code_path);
    if (!err.empty()) { fprintf(stderr, "pirip_hip_tx_create: %s: %s\n", code_path, err.c_str()); delete h; return PIRIP_ERR_BAD_ARG; }
    if (!h->code.accumulator) { delete h; return PIRIP_ERR_BAD_CONFIG; }             // no linear-time encoder: the framer tool's refusal
    h->Fs = Fs; h->Rs = Rs; h->M = M; h->Ts = Fs / Rs; h->bps = M == 2 ? 1 : 2; h->nstreams = nstreams;
    h->pre_bits = (int)preamble_bits(M).size();
    // the kernels' tiling: whole symbols per frame and per preamble, 32-bit sample counts in the phase integers
    if (Fs > kMaxFs || h->code.bits_per_frame() % h->bps || h->pre_bits % h->bps) { delete h; return PIRIP_ERR_UNSUPPORTED; }
    int rc = select_device(device, &h->device);
    if (rc == PIRIP_OK) rc = tx_alloc(h);
    if (rc != PIRIP_OK) { delete h; return rc; }
    *out = h;
    return PIRIP_OK;
}

int pirip_hip_tx_destroy(pirip_hip_tx *h) { return destroy_handle(h, h ? h->device : 0); }

int pirip_hip_tx_get_info(const pirip_hip_tx *h, pirip_tx_info *info)
{
    if (!h || !info) return PIRIP_ERR_BAD_ARG;
    std::memset(info, 0, sizeof(*info));
    info->Fs = h->Fs; info->Rs = h->Rs; info->M = h->M; info->Ts = h->Ts;
    info->n = h->code.n; info->k = h->code.k; info->bits_per_frame = h->code.bits_per_frame(); info->data_bytes = h->code.data_bytes();
    info->preamble_syms = tx_pre_syms(h); info->frame_syms = tx_frame_syms(h);
    info->nstreams = h->nstreams; info->device = h->device;
    return PIRIP_OK;
}

int pirip_hip_tx_set_tones(pirip_hip_tx *h, const int32_t *f1_hz, int tone_spacing_hz)
{
    if (!h || !f1_hz) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    std::vector<uint32_t> fm((size_t)h->nstreams * 4, 0), tm((size_t)h->nstreams * 4, 0);
    for (int s = 0; s < h->nstreams; s++)
        for (int m = 0; m < h->M; m++) {
            const int64_t f = fs_residue((int64_t)f1_hz[s] + (int64_t)m * tone_spacing_hz, h->Fs);
            fm[(size_t)s * 4 + m] = (uint32_t)f;
            tm[(size_t)s * 4 + m] = (uint32_t)fs_step(f, h->Ts, h->Fs);
        }
    PIRIP_HIPCHK(hipDeviceSynchronize());                    // calls in flight still read the old tones
    PIRIP_HIPCHK(hipMemcpy(h->d_fm, fm.data(), sizeof(uint32_t) * fm.size(), hipMemcpyHostToDevice));
    PIRIP_HIPCHK(hipMemcpy(h->d_tm, tm.data(), sizeof(uint32_t) * tm.size(), hipMemcpyHostToDevice));
    return PIRIP_OK;
}

int pirip_hip_tx_set_gaps(pirip_hip_tx *h, const int32_t *lead_syms, const int32_t *gap_syms)
{
    if (!h) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    std::vector<int32_t> lead((size_t)h->nstreams, 0), gap((size_t)h->nstreams, 0);
    int ml = 0, mg = 0;
    for (int s = 0; s < h->nstreams; s++) {
        if ((lead_syms && lead_syms[s] < 0) || (gap_syms && gap_syms[s] < 0)) return PIRIP_ERR_BAD_ARG;
        if (lead_syms) { lead[(size_t)s] = lead_syms[s]; if (lead_syms[s] > ml) ml = lead_syms[s]; }
        if (gap_syms) { gap[(size_t)s] = gap_syms[s]; if (gap_syms[s] > mg) mg = gap_syms[s]; }
    }
    PIRIP_HIPCHK(hipDeviceSynchronize());
    PIRIP_HIPCHK(hipMemcpy(h->d_lead, lead.data(), sizeof(int32_t) * lead.size(), hipMemcpyHostToDevice));
    PIRIP_HIPCHK(hipMemcpy(h->d_gap, gap.data(), sizeof(int32_t) * gap.size(), hipMemcpyHostToDevice));
    h->max_lead = ml; h->max_gap = mg;
    return PIRIP_OK;
}

int pirip_hip_tx_reset(pirip_hip_tx *h, void *hip_stream)
{
    if (!h) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    PIRIP_HIPCHK(hipMemsetAsync(h->d_phase, 0, sizeof(uint32_t) * (size_t)h->nstreams, (hipStream_t)hip_stream));
    if (h->d_rep_state) PIRIP_HIPCHK(hipMemsetAsync(h->d_rep_state, 0, sizeof(int32_t) * 2 * (size_t)h->nstreams, (hipStream_t)hip_stream));
    h->samples_sent = 0;
    return PIRIP_OK;
}

int64_t pirip_hip_tx_max_syms(const pirip_hip_tx *h, int max_rec)
{
    if (!h || max_rec < 0) return 0;
    return tx_row_syms(h, max_rec, h->max_lead);
}

int pirip_hip_tx_frame(pirip_hip_tx *h, const uint8_t *d_records, size_t rec_stride, const int32_t *d_nrec, int max_rec,
                       uint8_t *d_syms, size_t sym_stride, int64_t max_syms, int32_t *d_nsym, uint8_t *d_bits, size_t bits_stride,
                       void *hip_stream)
{
    if (!h || !d_records || !d_syms || max_rec < 0 || max_syms < 0) return PIRIP_ERR_BAD_ARG;
    if (max_syms < pirip_hip_tx_max_syms(h, max_rec)) return PIRIP_ERR_BAD_ARG;
    PIRIP_TRY(tx_frame_check(h, rec_stride, max_rec, sym_stride, max_syms, d_bits != nullptr, bits_stride));
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    const int rc = tx_grow(h, &h->d_off, &h->off_cap, (size_t)h->nstreams * (size_t)(max_rec > 0 ? max_rec : 1));
    if (rc != PIRIP_OK) return rc;
    return tx_frame_rows(h, d_records, rec_stride, d_nrec, max_rec, d_syms, sym_stride, max_syms, d_nsym ? d_nsym : h->d_nsym, d_bits, bits_stride,
                         h->d_lead, h->d_off, (hipStream_t)hip_stream);
}

int pirip_hip_tx_modulate(pirip_hip_tx *h, const uint8_t *d_syms, size_t sym_stride, const int32_t *d_nsym, int64_t nsym,
                          int out_format, void *d_out, size_t out_stride_bytes, float amp, float sigma, uint64_t seed, void *hip_stream)
{
    if (!h || !d_syms || !d_out || nsym < 0) return PIRIP_ERR_BAD_ARG;
    if (out_format != PIRIP_IN_CU8_FSKDEMOD && out_format != PIRIP_IN_CF32) return PIRIP_ERR_UNSUPPORTED;
    const int bsamp = out_format == PIRIP_IN_CF32 ? 8 : 2, spu = 16 / bsamp;
    PIRIP_TRY(iq_rows_check(d_out, out_stride_bytes, bsamp, 1, 0));
    const int64_t nsamp = nsym * h->Ts;
    if (nsamp > 0x7fffffff) return PIRIP_ERR_UNSUPPORTED;
    PIRIP_TRY(iq_rows_check(d_out, out_stride_bytes, bsamp, h->nstreams, nsamp));
    if (nsym == 0) return PIRIP_OK;
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    const int rc = tx_grow(h, &h->d_prefix, &h->prefix_cap, (size_t)h->nstreams * (size_t)nsym);
    if (rc != PIRIP_OK) return rc;
    ModArgs a{};
    a.syms = d_syms; a.sym_stride = sym_stride; a.nsym = d_nsym; a.total = nsym;
    a.prefix = h->d_prefix; a.phase = h->d_phase; a.fm = h->d_fm; a.tm = h->d_tm;
    a.out = d_out; a.out_stride = out_stride_bytes; a.n0 = h->samples_sent;
    a.Fs = h->Fs; a.Ts = h->Ts; a.M = h->M; a.nstreams = h->nstreams;
    a.aligned16 = (((uintptr_t)d_out | out_stride_bytes) & 15) == 0;
    a.two_over_fs = 2.0f / (float)h->Fs; a.amp = amp; a.sigma = sigma; a.inv_fs_d = 1.0 / (double)h->Fs; a.seed = seed;
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(tx_prefix_kernel, dim3((unsigned)h->nstreams), dim3(kScanThreads), 0, st, a);
    const int64_t units = (nsamp + spu - 1) / spu;
    const dim3 grid((unsigned)((units + kModThreads - 1) / kModThreads), (unsigned)(h->nstreams < 65535 ? h->nstreams : 65535),
                    (unsigned)((h->nstreams + 65534) / 65535));
    if (spu == 8) hipLaunchKernelGGL(tx_mod_kernel<8>, grid, dim3(kModThreads), 0, st, a);
    else hipLaunchKernelGGL(tx_mod_kernel<2>, grid, dim3(kModThreads), 0, st, a);
    PIRIP_HIPCHK(hipGetLastError());
    h->samples_sent += nsamp;
    return PIRIP_OK;
}

int pirip_hip_tx_records_to_iq(pirip_hip_tx *h, const uint8_t *d_records, size_t rec_stride, const int32_t *d_nrec, int max_rec,
                               int64_t nsym, int out_format, void *d_out, size_t out_stride_bytes, float amp, float sigma, uint64_t seed,
                               int32_t *d_nsym, void *hip_stream)
{
    if (!h) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    int64_t cap = pirip_hip_tx_max_syms(h, max_rec);
    if (cap < 1) cap = 1;
    int rc = tx_grow(h, &h->d_syms, &h->syms_cap, (size_t)h->nstreams * (size_t)cap);
    if (rc != PIRIP_OK) return rc;
    int32_t *ns = d_nsym ? d_nsym : h->d_nsym;
    rc = pirip_hip_tx_frame(h, d_records, rec_stride, d_nrec, max_rec, h->d_syms, (size_t)cap, cap, ns, nullptr, 0, hip_stream);
    if (rc != PIRIP_OK) return rc;
    return pirip_hip_tx_modulate(h, h->d_syms, (size_t)cap, ns, nsym, out_format, d_out, out_stride_bytes, amp, sigma, seed, hip_stream);
}

int pirip_hip_tx_repeat_max_records(const pirip_hip_tx *h, int ncalls)
{
    if (!h || ncalls < 0) return 0;
    return PIRIP_TX_REPEAT_MAX_FRAMES + 2 * ncalls;          // held frames + a frame and (at worst) an end per call
}

int pirip_hip_tx_repeat_records(pirip_hip_tx *h, const uint8_t *d_status, size_t status_stride, const uint8_t *d_payload, size_t payload_stride,
                                const int32_t *d_ncalls, int ncalls, int source_byte, uint8_t *d_records, size_t rec_stride, int max_rec,
                                int32_t *d_nrec, void *hip_stream)
{
    if (!h || !d_status || !d_payload || !d_records || ncalls < 0 || max_rec < 0 || source_byte < 0 || source_byte > 255) return PIRIP_ERR_BAD_ARG;
    const int kb = h->code.data_bytes();
    if (status_stride < (size_t)ncalls || payload_stride < (size_t)ncalls * kb || rec_stride < (size_t)max_rec * (size_t)(1 + kb)) return PIRIP_ERR_BAD_ARG;
    if (max_rec < pirip_hip_tx_repeat_max_records(h, ncalls)) return PIRIP_ERR_BAD_ARG;
    if (ncalls > kRepeatMaxCalls) return PIRIP_ERR_UNSUPPORTED;
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    if (!h->d_rep_state) {
        // first use: both buffers, the state zeroed, and only then the handle's pointers -- a failure leaves neither behind
        const size_t S = (size_t)h->nstreams;
        int32_t *state = nullptr; uint8_t *held = nullptr;
        int rc = h->mem.alloc_filled(&state, 0, sizeof(int32_t) * 2 * S);
        if (rc == PIRIP_OK) rc = h->mem.alloc(&held, S * PIRIP_TX_REPEAT_MAX_FRAMES * (size_t)kb);
        if (rc != PIRIP_OK) { h->mem.release(&state); h->mem.release(&held); return rc; }
        h->d_rep_state = state; h->d_rep_held = held;
    }
    RepeatArgs a{};
    a.in = RepeatIn{d_status, status_stride, d_payload, payload_stride, d_ncalls, ncalls, h->d_rep_state, h->d_rep_held, kb, PIRIP_TX_REPEAT_MAX_FRAMES, source_byte};
    a.rec = d_records; a.rec_stride = rec_stride; a.max_rec = max_rec; a.nrec = d_nrec;
    hipLaunchKernelGGL(tx_repeat_kernel, dim3((unsigned)h->nstreams), dim3(64), repeat_lds_bytes(ncalls), (hipStream_t)hip_stream, a);
    PIRIP_HIPCHK(hipGetLastError());
    return PIRIP_OK;
}

}  // extern "C"
