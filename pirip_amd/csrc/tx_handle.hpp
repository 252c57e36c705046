// pirip_amd/csrc/tx_handle.hpp -- the transmitter's handle behind include/pirip_hip.h's opaque pirip_hip_tx, and what the streaming
// transmitter (txs_kernels.hip, section K) and the streaming repeater (rpt_kernels.hip, section M) need of section I on the host
// (library-private: tx_kernels.hip owns the life cycle and the entry points; the device code they share is repeat_device.hpp's).
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

// whole symbols of the preamble and of a frame (pirip_hip_tx_create refuses a code or a preamble that leaves a part of one)
static inline int tx_pre_syms(const pirip_hip_tx *h) { return h->pre_bits / h->bps; }
static inline int tx_frame_syms(const pirip_hip_tx *h) { return h->code.bits_per_frame() / h->bps; }

// symbols a row of max_rec records can need behind max_lead symbols of lead, with the handle's gaps
int64_t tx_row_syms(const pirip_hip_tx *h, int max_rec, int max_lead);
// what stage 1 asks of its rows, before anything touches the device
int tx_frame_check(const pirip_hip_tx *h, size_t rec_stride, int max_rec, size_t sym_stride, int64_t max_syms, bool bits, size_t bits_stride);
// Stage 1 (pirip_hip_tx_frame) on rows, leads ([nstreams], device) and a record-offset table ([nstreams][max_rec], device) of the caller's,
// checked by tx_frame_check; the handle's device is current. Reads the handle's code, framer settings and gaps, writes nothing of it.
int tx_frame_rows(pirip_hip_tx *h, const uint8_t *d_records, size_t rec_stride, const int32_t *d_nrec, int max_rec,
                  uint8_t *d_syms, size_t sym_stride, int64_t max_syms, int32_t *d_nsym, uint8_t *d_bits, size_t bits_stride,
                  const int32_t *d_lead, int32_t *d_off, hipStream_t st);

}  // namespace pirip
#pragma GCC visibility pop
