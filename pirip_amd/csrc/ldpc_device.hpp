// pirip_amd/csrc/ldpc_device.hpp -- FSK_LDPC receive on the GPU (include/pirip_hip.h section E): constants, kernel
// argument blocks and device functions shared by the stage kernels (ldpc_stages.hip) and the three decoders (ldpc_decode.hip).
//   soft decisions (fsk_demod_sd's rx_filt) -> bit LLRs -> 32-bit unique-word search / sync state machine ->
//   sum-product LDPC decode (<= max_iter iterations, parity-check count, iteration count) -> CRC16 -> packed payload
//   bytes + rx_status, one record per demodulator call -- the stream `rtl_fsk --code ... -b` feeds to frame_repeater
//   (/root/reference/tx/frame_repeater.c:55-62,71,80,88; README.md:176-212).
// The parity-check matrix, the unique word and the sync thresholds are run-time DATA (fsk_ldpc.hpp): codec2's
// H_256_512_4 is not in /root/reference, nothing here is specific to a stand-in.
// Every floating-point step is written so that the CPU oracle can mirror it operation for operation (table look-ups,
// fixed summation order, no fused multiply-add: the files are built with -ffp-contract=off): hard outputs are bit-exact.
// Everything sits in the unnamed namespace, like the kernels: their mangled names (what tools/profile.sh and profiles/ match on)
// carry the argument blocks' types.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pirip_hip.h"
#include "fsk_ldpc.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kLnI0N = 256;              // ln I0 table: x = j/8, j = 0..256
// phi(x) = -ln tanh(x/2) over the range codec2's phi0() covers [UPSTREAM-RECALLED mpdecode_core.c / phi0.c, CML's MpDecode: "if (x > 10)
// return 0; else if (x < 9.08e-5) return 10; ..." -- the two end clamps are recalled, the staircase in between is not and is replaced
// by the function itself, 32 bins per octave]: messages saturate at 10 and vanish beyond 10. Rounds 2-4 ran [2^-24, 32) (saturation at
// 17.3); tools/ldpc_precision.py shows that this range, not the binary16 soft bits or the table's resolution, is what moves frames
// across the decoding edge against a double-precision receiver.
constexpr int kPhiLoExp = -14, kPhiHiExp = 4, kPhiSteps = 32;
constexpr int kPhiN = (kPhiHiExp - kPhiLoExp) * kPhiSteps;   // 576 bins, 32 per octave, x in [2^-14, 16)
constexpr float kPhiXLo = 9.08e-5f, kPhiXHi = 10.0f;        // below: phi = 10; from kPhiXHi up: phi = 0 (the table's bins from 10.0 on hold 0)
constexpr float kLlrMax = 24.0f;
constexpr int kDegFast = 8;
// "register-resident rows" decoder variant: each lane keeps the column lists of its <= kRowsPerLane check rows in VGPRs (packed
// u16) for the whole workgroup's life -- the code is fixed per handle, so these LDS reads would otherwise repeat in the check
// and parity passes of every iteration of every frame. (Doing the same for the variable-node edge lists spills at 128 VGPRs.)
constexpr int kRowsPerLane = 4;
constexpr int kInfoPerCall = PIRIP_LDPC_INFO_PER_CALL;   // state, uw_loc, uw_err, bad_uw, iter, pcc, decoded frame's window position (-1 none), crc_ok, eraw, 0

struct LdpcDev {
    int n, k, m, E, max_iter, uw_thresh1, uw_thresh2, bad_uw_thresh, M, Nsym, Nbits, bpf;
    int max_row_deg;                     // largest check-node degree (rows up to kDegFast keep their phi terms in registers)
    uint32_t uw_word;                    // unique word, first bit in the MSB
    const uint16_t *row_ptr, *col_idx, *col_ptr, *col_edge;
    const float *lnI0, *phi;
    int llr_map;                         // kLlrUpstream (codec2's fsk_rx_filt_to_llrs as recalled, the default) / kLlrRician (code file key `llr_map`)
};

struct FsmState { int32_t state, loc, bad_uw, uw_err; };

// Soft bits are exchanged as IEEE binary16, round to nearest even (ldpc_oracle.c, the checker, says why): h16 is the storage type.
typedef uint16_t h16;
__device__ __forceinline__ h16 f2h(float x) { return __builtin_bit_cast(h16, (_Float16)x); }
__device__ __forceinline__ float h2f(h16 u) { return (float)__builtin_bit_cast(_Float16, u); }
__device__ __forceinline__ float round16(float x) { return (float)(_Float16)x; }
template <typename OUT> __device__ __forceinline__ OUT to_out(float rounded);
template <> __device__ __forceinline__ h16 to_out<h16>(float rounded) { return f2h(rounded); }      // exact: the value is a binary16 already
template <> __device__ __forceinline__ float to_out<float>(float rounded) { return rounded; }

// ln I0(x), x >= 0: table at multiples of 1/8 up to 32 with linear interpolation, slope 1 beyond
// (branch-free: beyond 32 the argument is held at 32, where the interpolation gives tab[256] + 0 exactly, and x - 32 is added)
__device__ __forceinline__ float ln_i0(const float *tab, float x)
{
    const bool in = x < 32.0f;
    const float xs = (in ? x : 32.0f) * 8.0f;
    const int j = (int)xs;
    const float f = xs - (float)j;
    const float t0 = tab[j], t1 = tab[j + 1];
    return (t0 + (f * (t1 - t0))) + (in ? 0.0f : x - 32.0f);
}

// phi(x) = -ln tanh(x/2) by bins of the float's exponent and top five mantissa bits; x is clamped to [9.08e-5, 10]
__device__ __forceinline__ float phi_lookup(const float *tab, float x)
{
    const float lo = kPhiXLo;
    if (!(x >= lo)) x = lo;
    if (x >= kPhiXHi) return 0.0f;
    const int idx = (int)(__builtin_bit_cast(uint32_t, x) >> 18) - (int)((uint32_t)(127 + kPhiLoExp) << 5);
    return tab[idx];
}

// argument blocks of the fast and the persistent decoder (ldpc_decode.hip) and their LDS accesses by byte address
struct FastDev { const uint16_t *rcol, *vedge, *vsrc; int maxdeg; };
struct BankDev { const uint16_t *vcrc; uint32_t crc0, cps, cps_magic; };   // cps: chunks per stream; cps_magic = ceil(2^32 / cps): unit / cps = mulhi(unit, magic)
typedef __attribute__((address_space(3))) float lds_f32;
typedef __attribute__((address_space(3))) uint16_t lds_u16;
__device__ __forceinline__ float lds_ld(uint32_t a) { return *(lds_f32 *)(uintptr_t)a; }
__device__ __forceinline__ void lds_st(uint32_t a, float v) { *(lds_f32 *)(uintptr_t)a = v; }

// decode_kernel's dynamic LDS: [row_ptr m+1 | col_ptr n+1 | col_idx E | col_edge E] u16, [phi kPhiN] f32, per wave [Q n | r E] f32 + [hard n] u8
__host__ __device__ constexpr size_t dec_index_bytes(int m, int n, int E) { return (((size_t)(m + 1 + n + 1 + 2 * E) * 2) + 15) & ~(size_t)15; }
__host__ __device__ constexpr size_t dec_wave_bytes(int n, int E) { return ((size_t)(n + E) * 4 + (size_t)n + 15) & ~(size_t)15; }
__host__ __device__ constexpr size_t dec_lds_bytes(int m, int n, int E, int wpb) { return dec_index_bytes(m, n, E) + (size_t)kPhiN * 4 + (size_t)wpb * dec_wave_bytes(n, E); }

// ---- what the three decoders share: they must give the same records bit for bit, so each piece is defined once ------------------
// Ordering point for LDS traffic inside one wave (demod_simd.hpp says why no more is needed). Exactly these three builtins:
// wave_lds_sync() there carries a compiler barrier on top, with which hipcc schedules the generic and the fast decoder differently.
__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }
// The frame of a slot: direct mode = codeword `slot` of llr_src (parity tests / library entry), else entry `slot` of stream s's job
// list (demodulator call, window position): the demodulator call it belongs to and its n channel LLRs.
// (Returned as a struct: with a reference parameter for `call` hipcc schedules the fast decoder differently.)
struct Frame { int call; const h16 *llr; };
__device__ __forceinline__ Frame frame_of(int n, int s, int slot, int njob_slots, const int32_t *jobs, const h16 *llr_src, size_t llr_stride, int direct)
{
    Frame f;
    f.call = 0;
    if (direct) f.llr = llr_src + (size_t)slot * n;
    else {
        f.call = jobs[((size_t)s * njob_slots + slot) * 2];
        f.llr = llr_src + (size_t)s * llr_stride + jobs[((size_t)s * njob_slots + slot) * 2 + 1] + pirip::kUwBits;    // codeword LLRs follow the unique word
    }
    return f;
}
// direct mode's output: the decoded word and (iterations, parity checks satisfied)
__device__ __forceinline__ void put_direct(int n, int lane, int slot, const uint8_t *hard, int iter, int pcc, uint8_t *cw_out, int32_t *iter_pcc_out)
{
    for (int v = lane; v < n; v += kWave) cw_out[(size_t)slot * n + v] = hard[v];
    if (lane == 0) { iter_pcc_out[2 * slot] = iter; iter_pcc_out[2 * slot + 1] = pcc; }
}
// payload byte b of the decoded word, MSB first
__device__ __forceinline__ unsigned payload_byte(const uint8_t *hard, int b)
{
    unsigned byte = 0;
    for (int i = 0; i < 8; i++) byte |= (unsigned)hard[8 * b + i] << (7 - i);
    return byte;
}
// CRC-16/CCITT-FALSE (fsk_ldpc.cpp: crc16_ccitt) over all but the last two of the packed payload bytes against those two
__device__ __forceinline__ bool crc16_tail_ok(const uint8_t *bytes, int nbytes)
{
    uint16_t crc = 0xFFFF;
    for (int i = 0; i < nbytes - 2; i++) {
        uint8_t x = (uint8_t)(crc >> 8) ^ bytes[i];
        x ^= x >> 4;
        crc = (uint16_t)((crc << 8) ^ ((uint16_t)x << 12) ^ ((uint16_t)x << 5) ^ (uint16_t)x);
    }
    return crc == (uint16_t)((bytes[nbytes - 2] << 8) | bytes[nbytes - 1]);
}
// a decoded frame's status flags and its four info words (the state machine wrote the others)
__device__ __forceinline__ void put_info(int32_t *o, int iter, int pcc, bool crc_ok, int eraw) { o[4] = iter; o[5] = pcc; o[7] = crc_ok ? 1 : 0; o[8] = eraw; }
// ... of record `rec`, with the serial CRC over the packed payload `bytes` (one lane calls this)
__device__ __forceinline__ void put_record(uint8_t *status, int32_t *info, size_t rec, const uint8_t *bytes, int nbytes, int iter, int pcc, int m, int eraw)
{
    const bool crc_ok = crc16_tail_ok(bytes, nbytes);
    uint8_t stt = status[rec];
    if (crc_ok) stt |= pirip::kRxBits;
    if (pcc != m) stt |= pirip::kRxBitErrors;
    status[rec] = stt;
    put_info(info + rec * kInfoPerCall, iter, pcc, crc_ok, eraw);
}
// Check-node update of a row of weight <= kDegFast, each edge's phi(|q|) and sign kept in registers between the two passes:
// r_e = (product of the other signs) * phi(sum of the other phi(|q|)), q = Q - r (old). The row's edges are e0 .. e0 + deg - 1; their
// columns come two per register from rcol (PACKED: decode_kernel's register-resident rows) or from the list col_idx.
template <bool PACKED>
__device__ __forceinline__ void check_row(const float *s_phi, const float *Q, float *r, int e0, int deg, const uint32_t *rcol, const uint16_t *col_idx)
{
    float S = 0.0f, a[kDegFast];
    unsigned sg = 0, negs = 0;
#pragma unroll
    for (int j = 0; j < kDegFast; j++) {
        a[j] = 0.0f;
        if (j < deg) {
            const int col = PACKED ? (int)((rcol[j / 2] >> (16 * (j & 1))) & 0xffffu) : (int)col_idx[e0 + j];
            const float q = Q[col] - r[e0 + j];
            const unsigned ng = (q < 0.0f) ? 1u : 0u;
            sg ^= ng; negs |= ng << j;
            a[j] = phi_lookup(s_phi, fabsf(q));
            S = S + a[j];
        }
    }
#pragma unroll
    for (int j = 0; j < kDegFast; j++)
        if (j < deg) {
            const float mag = phi_lookup(s_phi, S - a[j]);
            r[e0 + j] = (sg ^ ((negs >> j) & 1u)) ? -mag : mag;
        }
}

}  // namespace
