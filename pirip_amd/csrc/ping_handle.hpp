// pirip_amd/csrc/ping_handle.hpp -- the ping terminal's handle behind include/pirip_hip.h's opaque pirip_hip_ping (library-private:
// ping_kernels.hip owns the life cycle and the entry points of section N).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_host.hpp"
#include "rpt_handle.hpp"

#pragma GCC visibility push(hidden)
namespace pirip {

// a receive channel's sample clock, ring position and counters; `written` entries were appended since create / reset
struct PingRxState {
    int64_t samples;
    int32_t next_nin, pad;
    int64_t written, filtered, decoded, crc_fail, bit_errors;
};
// a transmit channel's counters
struct PingTxState {
    int64_t bursts_sent, frames_sent, skipped;
};

}  // namespace pirip

// (hidden: a handle's implicit destructor is no dynamic symbol of the library)
struct pirip_hip_ping {
    pirip_hip_rx *rx = nullptr;
    pirip_hip_tx *tx = nullptr;
    pirip_hip_txs *txs = nullptr;
    int nrx = 0, ntx = 0, device = 0, kb = 0;
    int source = 0, filter = -1, frames = 0, seq = 0, period = 1, log_entries = 0, nin0 = 0;
    int64_t max_bursts = 0;
    int rx_rows = 0;                       // with rx: record rows per channel and call (pirip_hip_rx_max_frames)
    int64_t calls = 0;                     // calls since create / reset: the n of the schedule and of the entries
    pirip::DevMem mem;
    pirip::PingRxState *d_rx_state = nullptr;       // [nrx]
    pirip::PingRxState *d_rx_init = nullptr;        // [nrx] the state after create / reset: {0, nin0, 0 ...}
    pirip_ping_entry *d_log = nullptr;     // [nrx][log_entries]
    uint8_t *d_want = nullptr;             // [kb] the test payload
    // with tx
    pirip::PingTxState *d_tx_state = nullptr;       // [ntx]
    int32_t *d_first = nullptr;            // [ntx]
    uint8_t *d_burst = nullptr;            // [frames + 1][1 + kb] the burst's records
    uint8_t *d_offered = nullptr;          // [ntx][frames + 1][1 + kb] the records offered in the last call
    int32_t *d_noffered = nullptr;         // [ntx]
    // with rx: the rows of the last call
    uint8_t *d_status = nullptr, *d_payload = nullptr;       // [nrx][rx_rows], [nrx][rx_rows][kb]
    int32_t *d_info = nullptr, *d_nframes = nullptr;         // [nrx][rx_rows][PIRIP_LDPC_INFO_PER_CALL], [nrx]
    float *d_stats = nullptr;              // [nrx][rx_rows][PIRIP_STATS_PER_FRAME]
    // the rows the last call read (the caller's after push_records)
    const uint8_t *last_status = nullptr, *last_payload = nullptr;
    const int32_t *last_info = nullptr, *last_nframes = nullptr;
    const float *last_stats = nullptr;
    size_t last_status_stride = 0, last_payload_stride = 0, last_info_stride = 0, last_stats_stride = 0;
};
#pragma GCC visibility pop
