// pirip_amd/csrc/pkt_handle.hpp -- the packet link's handle behind include/pirip_hip.h's opaque pirip_hip_pkt (library-private:
// pkt_kernels.hip owns the life cycle and the entry points of section R).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "burst_ring.hpp"
#include "hip_host.hpp"
#include "rpt_handle.hpp"

#pragma GCC visibility push(hidden)
namespace pirip {

// a receive channel's open packet and counters; `delivered` entries were appended since create / reset
struct PktRxState {
    int64_t delivered, filtered, foreign, malformed, orphan, incomplete, crc_fail;
    int32_t open, src, id, nfrag, next, nbytes;
};
// a transmit channel's counters; the next id is sent mod 256
struct PktTxState {
    int64_t sent, refused, bad;
};

}  // namespace pirip

// (hidden: a handle's implicit destructor is no dynamic symbol of the library)
struct pirip_hip_pkt {
    pirip_hip_rx *rx = nullptr;
    pirip_hip_tx *tx = nullptr;
    pirip_hip_txs *txs = nullptr;
    int nrx = 0, ntx = 0, device = 0, kb = 0;
    int source = 0, filter = -1, address = -1, max_frags = 0, pending = 0, ring_entries = 0, cap = 0, max_packet = 0;
    int rx_rows = 0;                       // with rx: record rows per channel and call (pirip_hip_rx_max_frames)
    int64_t calls = 0;                     // calls since create / reset: the n of the entries and of the offers
    pirip::DevMem mem;
    pirip::PktRxState *d_rx_state = nullptr;        // [nrx]
    uint8_t *d_asm = nullptr;              // [nrx][max_frags * cap] the open packet's body so far
    pirip_pkt_entry *d_entries = nullptr;  // [nrx][ring_entries]
    uint8_t *d_data = nullptr;             // [nrx][ring_entries][max_packet]
    // with tx
    pirip::PktTxState *d_tx_state = nullptr;        // [ntx]
    pirip::BurstRings rings;               // [ntx] the pending rings (burst_ring.hpp), pending records of 1 + kb bytes each
    // with rx: the rows of the last call
    uint8_t *d_status = nullptr, *d_payload = nullptr;       // [nrx][rx_rows], [nrx][rx_rows][kb]
    int32_t *d_info = nullptr, *d_nframes = nullptr;         // [nrx][rx_rows][PIRIP_LDPC_INFO_PER_CALL], [nrx]
    // the rows the last call read (the caller's after push_records)
    const uint8_t *last_status = nullptr, *last_payload = nullptr;
    const int32_t *last_nframes = nullptr;
    size_t last_status_stride = 0, last_payload_stride = 0;
};
#pragma GCC visibility pop
