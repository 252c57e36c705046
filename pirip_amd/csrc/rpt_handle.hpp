// pirip_amd/csrc/rpt_handle.hpp -- the streaming repeater's handle behind include/pirip_hip.h's opaque pirip_hip_rpt, and what it needs
// of the receiver it borrows (library-private: rpt_kernels.hip owns the life cycle and the entry points of section M).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "burst_ring.hpp"
#include "hip_host.hpp"

#pragma GCC visibility push(hidden)
namespace pirip {

// a receive channel's counters
struct RptRxCount {
    int64_t bursts, frames, filtered, unrouted;
};

// (stream_rx.hip) channels, the FSK_LDPC receiver (NULL: none) and the device of a streaming receiver
void rx_handle_shape(const pirip_hip_rx *rx, int *nstreams, const pirip_hip_ldpc **ldpc, int *device);
// (stream_rx.hip) modem-rate samples the first demodulator call of a streaming receiver consumes: its demodulator's N
int rx_handle_nin0(const pirip_hip_rx *rx);

}  // namespace pirip

// (hidden: a handle's implicit destructor is no dynamic symbol of the library)
struct pirip_hip_rpt {
    pirip_hip_rx *rx = nullptr;
    pirip_hip_tx *tx = nullptr;
    pirip_hip_txs *txs = nullptr;
    int nrx = 0, ntx = 0, device = 0, kb = 0;
    int source = 0, filter = -1, holdoff = 0, max_burst = 0, pending = 0;
    int rx_rows = 0;                       // with rx: record rows per channel and call (pirip_hip_rx_max_frames)
    int64_t calls = 0;                     // calls since create / reset: the n of the ready tags
    pirip::DevMem mem;
    int32_t *d_route = nullptr;            // [nrx]
    int32_t *d_state = nullptr;            // [nrx][2] receiving, frames held
    uint8_t *d_held = nullptr;             // [nrx][max_burst][kb] the frames of a burst that is still being received
    pirip::RptRxCount *d_cnt = nullptr;    // [nrx]
    pirip::BurstRings rings;               // [ntx] the pending rings (burst_ring.hpp), pending records of 1 + kb bytes each
    // with rx: the records of the last call
    uint8_t *d_status = nullptr, *d_payload = nullptr;       // [nrx][rx_rows], [nrx][rx_rows][kb]
    int32_t *d_info = nullptr, *d_nframes = nullptr;         // [nrx][rx_rows][PIRIP_LDPC_INFO_PER_CALL], [nrx]
    // the rows the last call read (the caller's after push_records)
    const uint8_t *last_status = nullptr, *last_payload = nullptr;
    const int32_t *last_info = nullptr, *last_nframes = nullptr;
    size_t last_status_stride = 0, last_payload_stride = 0, last_info_stride = 0;
};
#pragma GCC visibility pop
