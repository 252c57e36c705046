// pirip_amd/csrc/tx_handle.hpp -- the transmitter's handle behind include/pirip_hip.h's opaque pirip_hip_tx, and what the streaming
// transmitter (txs_kernels.hip, section K) and the streaming repeater (rpt_kernels.hip, section M) need of section I (library-private:
// tx_kernels.hip owns the life cycle and the entry points).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fsk_ldpc.hpp"
#include "hip_host.hpp"

// (hidden: a handle's implicit destructor is no dynamic symbol of the library)
#pragma GCC visibility push(hidden)
struct pirip_hip_tx {
    pirip::LdpcCode code;
    int Fs = 0, Rs = 0, M = 0, Ts = 0, bps = 1, nstreams = 0, device = 0;
    int pre_bits = 0;
    int64_t samples_sent = 0;              // per stream since create / reset (every stream sends the same count per call)
    int max_lead = 0, max_gap = 0;
    pirip::DevMem mem;
    int32_t *d_row_ptr = nullptr, *d_col_idx = nullptr, *d_lead = nullptr, *d_gap = nullptr, *d_nsym = nullptr;
    uint32_t *d_fm = nullptr, *d_tm = nullptr, *d_phase = nullptr;
    // work buffers, grown on demand
    int32_t *d_off = nullptr; size_t off_cap = 0;
    uint32_t *d_prefix = nullptr; size_t prefix_cap = 0;
    uint8_t *d_syms = nullptr; size_t syms_cap = 0;
    // record conversion (the repeater): per stream {receiving, frames held} and the held frames, made on first use
    int32_t *d_rep_state = nullptr; uint8_t *d_rep_held = nullptr;
};

namespace pirip {

constexpr int kScanThreads = 256;

// symbols a row of max_rec records can need behind max_lead symbols of lead, with the handle's gaps
int64_t tx_row_syms(const pirip_hip_tx *h, int max_rec, int max_lead);
// what stage 1 asks of its rows, before anything touches the device
int tx_frame_check(const pirip_hip_tx *h, size_t rec_stride, int max_rec, size_t sym_stride, int64_t max_syms, bool bits, size_t bits_stride);
// Stage 1 (pirip_hip_tx_frame) on rows, leads ([nstreams], device) and a record-offset table ([nstreams][max_rec], device) of the caller's,
// checked by tx_frame_check; the handle's device is current. Reads the handle's code, framer settings and gaps, writes nothing of it.
int tx_frame_rows(pirip_hip_tx *h, const uint8_t *d_records, size_t rec_stride, const int32_t *d_nrec, int max_rec,
                  uint8_t *d_syms, size_t sym_stride, int64_t max_syms, int32_t *d_nsym, uint8_t *d_bits, size_t bits_stride,
                  const int32_t *d_lead, int32_t *d_off, hipStream_t st);

// A_i of one row, by one workgroup of kScanThreads: pre[i] = (carry + sum_{q < i} tm[sym(q)]) mod Fs for i < total, an exclusive scan in
// wave and across waves in 32-bit integers; sym(i) is the symbol 0 .. 3, or -1 for carrier off, which adds nothing. Returns the row's final
// phase (every thread). s_tot: kScanThreads / 64 words of LDS.
template <typename SymAt>
__device__ __forceinline__ uint32_t tx_scan_row(SymAt sym, int64_t total, const uint32_t *tm_s, uint32_t Fs, uint32_t carry, uint32_t *pre, uint32_t *s_tot)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t tm[4];
    for (int m = 0; m < 4; m++) tm[m] = tm_s[m];
    for (int64_t base = 0; base < total; base += kScanThreads) {
        const int64_t i = base + tid;
        const int sm = i < total ? sym(i) : -1;
        const uint32_t v = sm < 0 ? 0u : tm[sm];
        uint32_t incl = v;                                   // < 64 * 2^24
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_tot[wave] = incl % Fs;
        __syncthreads();
        uint32_t before = carry, all = carry;                // carry + the waves in front: < 5 * 2^24
        for (int w = 0; w < kScanThreads / 64; w++) { if (w < wave) before += s_tot[w]; all += s_tot[w]; }
        if (i < total) pre[i] = (before + (incl - v)) % Fs;
        carry = all % Fs;
        __syncthreads();
    }
    return carry;
}

// The repeater's state machine (tx/frame_repeater.c:68-107) over nc status bytes, run by ONE lane: tx_repeat_kernel's walk, shared with
// the streaming repeater's intake (rpt_kernels.hip). status(c): the call's rx_status. receiving / n: the stream's state carried in (a burst
// is open; the frames it holds). A burst starts at a status of exactly SYNC | BITS, takes every later record with BITS while it holds
// fewer than max_burst frames (further frames are dropped where the original asserts) and ends at the first record without SYNC.
// Writes act[c] = -1, or (burst << 16) | slot of the call's frame; for every burst b that ended here base[b] = its first output record
// (bursts laid out one after the other, each followed by its end record) and nfr[b] = its frames; base[bursts] = -1 and nfr[bursts] = the
// frames of the burst still open. hdr = {bursts ended, records out, receiving, frames held at the end}.
template <typename StatusAt>
__device__ __forceinline__ void tx_repeat_walk(StatusAt status, int nc, int receiving, int n, int max_burst, int32_t *act_out, int32_t *base,
                                               int32_t *nfr, int32_t *hdr)
{
    int b = 0, nout = 0;
    for (int c = 0; c < nc; c++) {
        const int v = status(c);
        int act = -1;
        if (!receiving) {
            if (v == (PIRIP_RX_SYNC | PIRIP_RX_BITS)) { receiving = 1; n = 1; act = (b << 16) | 0; }
        } else {
            if ((v & PIRIP_RX_BITS) && n < max_burst) { act = (b << 16) | n; n++; }
            if (!(v & PIRIP_RX_SYNC)) { base[b] = nout; nfr[b] = n; nout += n + 1; b++; receiving = 0; n = 0; }
        }
        act_out[c] = act;
    }
    base[b] = -1; nfr[b] = n;
    hdr[0] = b; hdr[1] = nout; hdr[2] = receiving; hdr[3] = receiving ? n : 0;
}

}  // namespace pirip
#pragma GCC visibility pop
