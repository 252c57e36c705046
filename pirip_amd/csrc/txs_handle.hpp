// pirip_amd/csrc/txs_handle.hpp -- the streaming transmitter's handle behind include/pirip_hip.h's opaque pirip_hip_txs, and what the
// streaming repeater (rpt_kernels.hip, section M) needs of section K (library-private: txs_kernels.hip owns the life cycle and the entry
// points).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_host.hpp"

#pragma GCC visibility push(hidden)
namespace pirip {

// a channel's queue and counters on the device
struct TxsChanState {
    uint64_t head, tail;                   // symbols dequeued / queued since create / reset; the ring holds [head, tail)
    int64_t sent, underrun, refused;
    uint32_t phase, pad;                   // the modulator's phase integer after the last dequeued symbol
};

}  // namespace pirip

// (hidden: a handle's implicit destructor is no dynamic symbol of the library)
struct pirip_hip_txs {
    pirip_hip_tx *tx = nullptr;
    pirip_hip_mux *mux = nullptr;
    int nchan = 0, device = 0, S = 0, H = 0;
    int64_t block = 0, queue_syms = 0;
    int64_t calls = 0;                     // process calls since create / reset: call k starts at modem sample k S Ts
    size_t row = 0;                        // H + S
    pirip::DevMem mem;
    uint8_t *d_ring = nullptr;             // [nchan][queue_syms]
    pirip::TxsChanState *d_state = nullptr;   // [nchan]
    uint8_t *d_sy = nullptr;               // [2][nchan][row]
    uint32_t *d_pre = nullptr;             // [2][nchan][row]
    int32_t *d_no_lead = nullptr;          // [nchan] zeros: a streaming transmitter's silence is its empty queue
    // the framer's rows of a send, grown on demand
    uint8_t *d_frm = nullptr; size_t frm_cap = 0;            // [nchan][frm_cap]
    int32_t *d_off = nullptr; size_t off_cap = 0;            // [nchan][off_cap]
    int32_t *d_nsym = nullptr;             // [nchan]
};

namespace pirip {
// the framer's rows for sends of up to max_rec records per channel, with tx's gaps as they are now: later sends of that size neither
// allocate nor synchronise. The handle's device is current.
int txs_reserve(pirip_hip_txs *t, int max_rec);
}  // namespace pirip
#pragma GCC visibility pop
