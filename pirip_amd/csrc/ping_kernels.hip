// pirip_amd/csrc/ping_kernels.hip -- include/pirip_hip.h section N: the ping terminal.
// One call per block: received FSK_LDPC records -> rtl_fsk's --filter -> one log entry per frame that passed its CRC, in a ring per receive
// channel; on a schedule counted in calls a burst of test frames -> section K's symbol queue -> one block of wideband IQ.
//
//   log:      records + stats --ping_log_kernel (one wave per receive channel)--> log ring, sample clock, counters
//   schedule: ping_offer_kernel (one wave per transmit channel) --> record rows --section K's send path--> symbol queue
//   process:  pirip_hip_txs_process
//
// The sample clock of a channel is rtl_fsk -L's: every row consumed what the row in front of it announced (stats[6]), the first row of all
// nin0. The log kernel makes it a prefix sum over that shifted column, 64 rows at a time. The call index n is host state advanced when a
// call is enqueued, as in section M.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/pirip_hip.h"
#include "../tools/tx_records.hpp"
#include "hip_host.hpp"
#include "ldpc_handle.hpp"
#include "mux_handle.hpp"
#include "ping_handle.hpp"
#include "repeat_device.hpp"
#include "rpt_handle.hpp"
#include "tx_handle.hpp"
#include "txs_handle.hpp"

using namespace pirip;

namespace {

constexpr int kPingMaxRows = kRepeatMaxCalls;                // rows per channel and call, section M's limit

struct LogArgs {
    const uint8_t *status; size_t status_stride; const uint8_t *payload; size_t payload_stride;      // [nrx][rows], [nrx][rows][kb]
    const int32_t *info; size_t info_stride;                 // [nrx][rows][PIRIP_LDPC_INFO_PER_CALL]
    const uint32_t *stats; size_t stats_stride;              // [nrx][rows][PIRIP_STATS_PER_FRAME], the floats' bits
    const int32_t *nrows; int max_rows;    // rows per channel (NULL: max_rows), at most max_rows
    const uint8_t *want;                   // [kb] the test payload
    int kb, filter, log_entries;
    int32_t call;                          // n
    PingRxState *state;                    // [nrx]
    pirip_ping_entry *log;                 // [nrx][log_entries]
};

// One wave per receive channel. Pass 1 counts what the call logs, so that pass 2 writes only the entries the ring keeps: a slot has one
// writer per call, whatever log_entries is. Pass 2 takes 64 rows at a time: the clock by a wave scan, the logged rows compacted by ballot
// and rank, each logged row's payload compared by the whole wave.
__global__ __launch_bounds__(64) void ping_log_kernel(LogArgs a)
{
    const size_t c = blockIdx.x;
    const int lane = threadIdx.x;
    const int nf = row_count(a.nrows, c, a.max_rows);
    const uint8_t *st = a.status + c * a.status_stride;
    const uint8_t *pl = a.payload + c * a.payload_stride;
    const int32_t *info = a.info + c * a.info_stride;
    const uint32_t *stats = a.stats + c * a.stats_stride;
    const PingRxState s = a.state[c];
    auto filtered_out = [&](uint8_t v, int f) { return (v & PIRIP_RX_BITS) && a.filter >= 0 && pl[(size_t)f * a.kb] == (uint8_t)a.filter; };
    auto nin_of = [&](int f) { return (int)__uint_as_float(stats[(size_t)f * PIRIP_STATS_PER_FRAME + 6]); };

    int logged = 0, filtered = 0, decoded = 0, crc_fail = 0;
    for (int f = lane; f < nf; f += 64) {
        const uint8_t v = st[f];
        const bool dec = info[(size_t)f * PIRIP_LDPC_INFO_PER_CALL + 6] >= 0, hit = filtered_out(v, f);
        decoded += dec;
        crc_fail += dec && !(v & PIRIP_RX_BITS);
        filtered += hit;
        logged += (v & PIRIP_RX_BITS) && !hit;
    }
    logged = wave_sum(logged); filtered = wave_sum(filtered); decoded = wave_sum(decoded); crc_fail = wave_sum(crc_fail);
    const int keep_from = logged - a.log_entries;            // this call's entries in front of that one are overwritten by its own later ones

    pirip_ping_entry *ring = a.log + c * (size_t)a.log_entries;
    int64_t samples = s.samples;
    int before = 0, errors = 0;                              // logged rows in front of this chunk; the sum of their ecdd (per lane)
    for (int base = 0; base < nf; base += 64) {
        const int f = base + lane;
        const bool in = f < nf;
        // the shifted nin column: row f consumed what row f - 1 announced, row 0 what the call before left
        const int nin = !in ? 0 : f == 0 ? s.next_nin : nin_of(f - 1);
        const int64_t t = samples + wave_scan((int64_t)nin);
        samples = __shfl(t, 63, 64);
        const uint8_t v = in ? st[f] : 0;
        const bool log = in && (v & PIRIP_RX_BITS) && !filtered_out(v, f);
        const unsigned long long mask = __ballot(log);
        int ecdd = 0;
        for (unsigned long long m = mask; m; m &= m - 1) {   // (the same in every lane)
            const int r = __builtin_ctzll(m);
            const uint8_t *p = pl + (size_t)(base + r) * a.kb;
            int e = 0;
            for (int b = 2 + lane; b < a.kb - 2; b += 64) e += __popc((uint32_t)(p[b] ^ a.want[b]));
            e = wave_sum(e);
            if (lane == r) ecdd = e;
        }
        if (log) {
            const int i = before + wave_rank(mask);
            errors += ecdd;
            if (i >= keep_from) {
                const uint8_t *p = pl + (size_t)f * a.kb;
                const int32_t *in_f = info + (size_t)f * PIRIP_LDPC_INFO_PER_CALL;
                const uint32_t *s_f = stats + (size_t)f * PIRIP_STATS_PER_FRAME;
                pirip_ping_entry e;
                e.t_samples = t; e.call = a.call; e.row = f;
                e.S = __uint_as_float(s_f[8]); e.N = __uint_as_float(s_f[9]); e.SNRest = __uint_as_float(s_f[5]);
                e.ecdd = ecdd; e.eraw = in_f[8];
                e.source = p[0]; e.seq = p[1]; e.status = v; e.iters = (uint8_t)(in_f[4] < 0 ? 0 : in_f[4] > 255 ? 255 : in_f[4]);
                ring[(size_t)((uint64_t)(s.written + i) % (uint64_t)a.log_entries)] = e;
            }
        }
        before += __popcll(mask);
    }
    errors = wave_sum(errors);
    if (lane == 0) {
        PingRxState o = s;
        o.samples = samples;
        if (nf > 0) o.next_nin = nin_of(nf - 1);
        o.written += logged; o.filtered += filtered; o.decoded += decoded; o.crc_fail += crc_fail; o.bit_errors += errors;
        a.state[c] = o;
    }
}

struct OfferArgs {
    PingTxState *state;                    // [ntx]
    const int32_t *first;                  // [ntx]
    const TxsChanState *queue; int64_t queue_syms;           // section K's queues: free space = queue_syms - (tail - head)
    const int32_t *gap;                    // [ntx] tx's gaps (device)
    const uint8_t *burst;                  // [frames + 1][rl]
    uint8_t *rec; int32_t *nrec;           // [ntx][frames + 1][rl] and [ntx]: what section K's send path reads
    int frames, rl, psyms, fsyms, period;
    int64_t max_bursts, now;               // now: n
};

// One wave per transmit channel: every lane makes the same decision, then the wave copies the burst's records into the channel's row.
__global__ __launch_bounds__(64) void ping_offer_kernel(OfferArgs a)
{
    const int t = blockIdx.x, lane = threadIdx.x;
    const PingTxState s = a.state[t];
    const int64_t since = a.now - (int64_t)a.first[t];
    const bool due = since >= 0 && since % a.period == 0 && (a.max_bursts == 0 || s.bursts_sent < a.max_bursts);
    const int gap = a.gap[t] > 0 ? a.gap[t] : 0;              // tx_layout_kernel's rule
    const int64_t room = a.queue_syms - (int64_t)(a.queue[t].tail - a.queue[t].head);
    const int64_t cost = tx_record_syms(1, a.psyms, a.fsyms, gap) + (int64_t)(a.frames - 1) * tx_record_syms(0, a.psyms, a.fsyms, gap) +
                         tx_record_syms(2, a.psyms, a.fsyms, gap);                               // records 1, 0, ..., 0, 2
    const bool send = due && cost <= room;
    const int n = (a.frames + 1) * a.rl;
    uint8_t *out = a.rec + (size_t)t * n;
    if (send) for (int i = lane; i < n; i += 64) out[i] = a.burst[i];
    if (lane == 0) {
        a.nrec[t] = send ? a.frames + 1 : 0;
        if (due) {
            PingTxState o = s;
            if (send) { o.bursts_sent++; o.frames_sent += a.frames; } else o.skipped++;
            a.state[t] = o;
        }
    }
}

int ping_clear(pirip_hip_ping *p, hipStream_t st)
{
    // (next_nin starts at nin0: the states come from a device copy made at create, so that a reset enqueues a copy and no upload)
    PIRIP_HIPCHK(hipMemcpyAsync(p->d_rx_state, p->d_rx_init, sizeof(PingRxState) * (size_t)p->nrx, hipMemcpyDeviceToDevice, st));
    PIRIP_HIPCHK(hipMemsetAsync(p->d_log, 0, sizeof(pirip_ping_entry) * (size_t)p->nrx * (size_t)p->log_entries, st));
    if (p->tx) {
        PIRIP_HIPCHK(hipMemsetAsync(p->d_tx_state, 0, sizeof(PingTxState) * (size_t)p->ntx, st));
        PIRIP_HIPCHK(hipMemsetAsync(p->d_noffered, 0, sizeof(int32_t) * (size_t)p->ntx, st));
    }
    p->calls = 0;
    return PIRIP_OK;
}

int ping_alloc(pirip_hip_ping *p, const int32_t *first_call)
{
    const size_t nrx = (size_t)p->nrx, ntx = (size_t)p->ntx, kb = (size_t)p->kb, rl = 1 + kb;
    DevMem &m = p->mem;
    const std::vector<PingRxState> init(nrx, PingRxState{0, p->nin0, 0, 0, 0, 0, 0, 0});
    PIRIP_TRY(m.upload(&p->d_rx_init, init.data(), sizeof(PingRxState) * nrx));
    PIRIP_TRY(m.alloc(&p->d_rx_state, sizeof(PingRxState) * nrx));
    PIRIP_TRY(m.alloc(&p->d_log, sizeof(pirip_ping_entry) * nrx * (size_t)p->log_entries));
    std::vector<uint8_t> want(kb);
    PIRIP_TRY(pirip_hip_tbits_testframe_payload(8 * p->kb, want.data()));
    PIRIP_TRY(m.upload(&p->d_want, want.data(), kb));
    if (p->tx) {
        // one definition of the test frame: the records fsk_ldpc_framer --testframes makes (tools/tx_records.hpp)
        std::vector<uint8_t> burst;
        testframe_records(8 * p->kb, p->frames, 1, p->source, p->seq, burst);
        if (burst.size() != (size_t)(p->frames + 1) * rl) return PIRIP_ERR_BAD_ARG;
        std::vector<int32_t> first(ntx, 0);
        if (first_call) std::memcpy(first.data(), first_call, sizeof(int32_t) * ntx);
        PIRIP_TRY(m.upload(&p->d_burst, burst.data(), burst.size()));
        PIRIP_TRY(m.upload(&p->d_first, first.data(), sizeof(int32_t) * ntx));
        PIRIP_TRY(m.alloc(&p->d_tx_state, sizeof(PingTxState) * ntx));
        PIRIP_TRY(m.alloc_filled(&p->d_offered, 0, ntx * burst.size()));
        PIRIP_TRY(m.alloc(&p->d_noffered, sizeof(int32_t) * ntx));
        PIRIP_TRY(txs_reserve(p->txs, p->frames + 1));
    }
    if (p->rx) {
        const size_t R = (size_t)p->rx_rows;
        PIRIP_TRY(m.alloc_filled(&p->d_status, 0, nrx * R));
        PIRIP_TRY(m.alloc_filled(&p->d_payload, 0, nrx * R * kb));
        PIRIP_TRY(m.alloc_filled(&p->d_info, 0, sizeof(int32_t) * nrx * R * PIRIP_LDPC_INFO_PER_CALL));
        PIRIP_TRY(m.alloc_filled(&p->d_stats, 0, sizeof(float) * nrx * R * PIRIP_STATS_PER_FRAME));
        PIRIP_TRY(m.alloc_filled(&p->d_nframes, 0, sizeof(int32_t) * nrx));
    }
    PIRIP_TRY(ping_clear(p, nullptr));
    PIRIP_HIPCHK(hipDeviceSynchronize());
    return PIRIP_OK;
}

// txs_process's own checks, made before anything is enqueued: a call either runs whole or not at all. A logger has no output.
int ping_check_out(const pirip_hip_ping *p, const void *d_out, size_t out_stride_bytes)
{
    if (!p->tx) return d_out ? PIRIP_ERR_BAD_ARG : PIRIP_OK;
    if (!d_out) return PIRIP_ERR_BAD_ARG;
    return iq_rows_check(d_out, out_stride_bytes, p->txs->mux->bs, p->txs->mux->noutputs, p->txs->block);
}

// the steps over rows that are on the device; the handle's device is current
int ping_run(pirip_hip_ping *p, const uint8_t *d_status, size_t status_stride, const uint8_t *d_payload, size_t payload_stride, const int32_t *d_info,
             size_t info_stride, const float *d_stats, size_t stats_stride, const int32_t *d_ncalls, int ncalls, void *d_out, size_t out_stride_bytes,
             hipStream_t st)
{
    LogArgs la{};
    la.status = d_status; la.status_stride = status_stride; la.payload = d_payload; la.payload_stride = payload_stride;
    la.info = d_info; la.info_stride = info_stride; la.stats = (const uint32_t *)d_stats; la.stats_stride = stats_stride;
    la.nrows = d_ncalls; la.max_rows = ncalls;
    la.want = p->d_want; la.kb = p->kb; la.filter = p->filter; la.log_entries = p->log_entries;
    la.call = (int32_t)p->calls;
    la.state = p->d_rx_state; la.log = p->d_log;
    hipLaunchKernelGGL(ping_log_kernel, dim3((unsigned)p->nrx), dim3(64), 0, st, la);
    PIRIP_HIPCHK(hipGetLastError());
    if (p->tx) {
        const pirip_hip_tx *tx = p->tx;
        const size_t rl = 1 + (size_t)p->kb;
        OfferArgs oa{};
        oa.state = p->d_tx_state; oa.first = p->d_first;
        oa.queue = p->txs->d_state; oa.queue_syms = p->txs->queue_syms; oa.gap = tx->d_gap;
        oa.burst = p->d_burst; oa.rec = p->d_offered; oa.nrec = p->d_noffered;
        oa.frames = p->frames; oa.rl = (int)rl; oa.psyms = tx_pre_syms(tx); oa.fsyms = tx_frame_syms(tx); oa.period = p->period;
        oa.max_bursts = p->max_bursts; oa.now = p->calls;
        hipLaunchKernelGGL(ping_offer_kernel, dim3((unsigned)p->ntx), dim3(64), 0, st, oa);
        PIRIP_HIPCHK(hipGetLastError());
        PIRIP_TRY(pirip_hip_txs_send(p->txs, p->d_offered, (size_t)(p->frames + 1) * rl, p->d_noffered, p->frames + 1, nullptr, st));
        PIRIP_TRY(pirip_hip_txs_process(p->txs, d_out, out_stride_bytes, nullptr, st));
    }
    p->calls++;
    return PIRIP_OK;
}

int ping_receive(pirip_hip_ping *p, const void *d_in, size_t in_stride_bytes, void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    if (!p || !p->rx) return PIRIP_ERR_BAD_ARG;
    PIRIP_TRY(ping_check_out(p, d_out, out_stride_bytes));
    if (!bind_device(p->device)) return PIRIP_ERR_NO_DEVICE;
    const size_t R = (size_t)p->rx_rows, kb = (size_t)p->kb;
    if (d_in)
        PIRIP_TRY(pirip_hip_rx_push(p->rx, d_in, in_stride_bytes, nullptr, 0, nullptr, 0, p->d_status, p->d_payload, p->d_info, p->d_stats,
                                    R * PIRIP_STATS_PER_FRAME, p->d_nframes, hip_stream));
    else
        PIRIP_TRY(pirip_hip_rx_process(p->rx, nullptr, 0, nullptr, 0, p->d_status, p->d_payload, p->d_info, p->d_stats, R * PIRIP_STATS_PER_FRAME,
                                       p->d_nframes, hip_stream));
    p->last_status = p->d_status; p->last_status_stride = R; p->last_payload = p->d_payload; p->last_payload_stride = R * kb;
    p->last_info = p->d_info; p->last_info_stride = R * PIRIP_LDPC_INFO_PER_CALL; p->last_stats = p->d_stats;
    p->last_stats_stride = R * PIRIP_STATS_PER_FRAME; p->last_nframes = p->d_nframes;
    return ping_run(p, p->d_status, R, p->d_payload, R * kb, p->d_info, R * PIRIP_LDPC_INFO_PER_CALL, p->d_stats, R * PIRIP_STATS_PER_FRAME, p->d_nframes,
                    p->rx_rows, d_out, out_stride_bytes, (hipStream_t)hip_stream);
}

}  // namespace

extern "C" {

int pirip_hip_ping_create(pirip_hip_rx *rx, pirip_hip_tx *tx, pirip_hip_txs *txs, const pirip_ping_config *cfg, pirip_hip_ping **out)
{
    if (!out) return PIRIP_ERR_BAD_ARG;
    *out = nullptr;
    if (!cfg || (!tx) != (!txs) || (!rx && !tx)) return PIRIP_ERR_BAD_ARG;
    if (tx && (txs->tx != tx || txs->device != tx->device)) return PIRIP_ERR_BAD_ARG;
    if (cfg->nrx < 1 || cfg->source_byte < 0 || cfg->source_byte > 255 || cfg->filter_byte < -1 || cfg->filter_byte > 255) return PIRIP_ERR_BAD_ARG;
    if (cfg->frames_per_burst < 1 || cfg->frames_per_burst > PIRIP_TX_REPEAT_MAX_FRAMES || cfg->period_calls < 1 || cfg->max_bursts < 0 ||
        cfg->log_entries < 1)
        return PIRIP_ERR_BAD_ARG;
    const int ntx = tx ? tx->nstreams : 0, frames = cfg->frames_per_burst;
    if (tx && cfg->first_call) for (int t = 0; t < ntx; t++) if (cfg->first_call[t] < 0) return PIRIP_ERR_BAD_ARG;
    int kb = tx ? tx->code.data_bytes() : 0, device = tx ? tx->device : 0, rx_rows = 0, nin0 = cfg->nin0;
    if (tx && tx_pre_syms(tx) + (int64_t)frames * tx_frame_syms(tx) + tx->max_gap > txs->queue_syms) return PIRIP_ERR_BAD_ARG;
    if (rx) {
        int ns = 0, dev = 0;
        const pirip_hip_ldpc *ldpc = nullptr;
        rx_handle_shape(rx, &ns, &ldpc, &dev);
        if (!ldpc || ns != cfg->nrx || (tx && (dev != device || ldpc->code.data_bytes() != kb))) return PIRIP_ERR_BAD_ARG;
        const int64_t rows = pirip_hip_rx_max_frames(rx);
        if (rows < 1) return PIRIP_ERR_BAD_ARG;
        if (rows > kPingMaxRows) return PIRIP_ERR_UNSUPPORTED;
        rx_rows = (int)rows; kb = ldpc->code.data_bytes(); device = dev; nin0 = rx_handle_nin0(rx);
    }
    if (nin0 < 0 || kb < 4) return PIRIP_ERR_BAD_ARG;
    if (tx) {                                                // what section K's send path asks of rows of frames + 1 records
        int64_t cap = tx_row_syms(tx, frames + 1, 0);
        if (cap < 1) cap = 1;
        PIRIP_TRY(tx_frame_check(tx, (size_t)(frames + 1) * (size_t)(1 + kb), frames + 1, (size_t)cap, cap, false, 0));
    }
    if (!bind_device(device)) return PIRIP_ERR_NO_DEVICE;
    pirip_hip_ping *p = new (std::nothrow) pirip_hip_ping();
    if (!p) return PIRIP_ERR_NOMEM;
    p->rx = rx; p->tx = tx; p->txs = txs; p->nrx = cfg->nrx; p->ntx = ntx; p->device = device; p->kb = kb;
    p->source = cfg->source_byte; p->filter = cfg->filter_byte; p->frames = frames; p->seq = cfg->seq ? 1 : 0; p->period = cfg->period_calls;
    p->log_entries = cfg->log_entries; p->nin0 = nin0; p->max_bursts = cfg->max_bursts; p->rx_rows = rx_rows;
    const int rc = ping_alloc(p, cfg->first_call);
    if (rc != PIRIP_OK) { delete p; return rc; }
    *out = p;
    return PIRIP_OK;
}

int pirip_hip_ping_destroy(pirip_hip_ping *p) { return destroy_handle(p, p ? p->device : 0); }

int pirip_hip_ping_get_info(const pirip_hip_ping *p, pirip_ping_info *info)
{
    if (!p || !info) return PIRIP_ERR_BAD_ARG;
    *info = pirip_ping_info{p->nrx, p->ntx, p->source, p->filter, p->frames, p->seq, p->period, p->log_entries, p->nin0, p->rx ? 1 : 0, p->rx_rows,
                            p->kb, p->device, p->max_bursts};
    return PIRIP_OK;
}

int pirip_hip_ping_push_records(pirip_hip_ping *p, const uint8_t *d_status, size_t status_stride, const uint8_t *d_payload, size_t payload_stride,
                                const int32_t *d_info, size_t info_stride, const float *d_stats, size_t stats_stride, const int32_t *d_ncalls,
                                int ncalls, void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    if (!p || !d_status || !d_payload || !d_info || !d_stats || ncalls < 0) return PIRIP_ERR_BAD_ARG;
    const size_t nc = (size_t)ncalls;
    if (p->nrx > 1 && (status_stride < nc || payload_stride < nc * (size_t)p->kb || info_stride < nc * PIRIP_LDPC_INFO_PER_CALL ||
                       stats_stride < nc * PIRIP_STATS_PER_FRAME))
        return PIRIP_ERR_BAD_ARG;
    if (ncalls > kPingMaxRows) return PIRIP_ERR_UNSUPPORTED;
    PIRIP_TRY(ping_check_out(p, d_out, out_stride_bytes));
    if (!bind_device(p->device)) return PIRIP_ERR_NO_DEVICE;
    PIRIP_TRY(ping_run(p, d_status, status_stride, d_payload, payload_stride, d_info, info_stride, d_stats, stats_stride, d_ncalls, ncalls, d_out,
                       out_stride_bytes, (hipStream_t)hip_stream));
    p->last_status = d_status; p->last_status_stride = status_stride; p->last_payload = d_payload; p->last_payload_stride = payload_stride;
    p->last_info = d_info; p->last_info_stride = info_stride; p->last_stats = d_stats; p->last_stats_stride = stats_stride; p->last_nframes = d_ncalls;
    return PIRIP_OK;
}

int pirip_hip_ping_process(pirip_hip_ping *p, void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    return ping_receive(p, nullptr, 0, d_out, out_stride_bytes, hip_stream);
}

int pirip_hip_ping_push(pirip_hip_ping *p, const void *d_in, size_t in_stride_bytes, void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    if (!d_in) return PIRIP_ERR_BAD_ARG;
    return ping_receive(p, d_in, in_stride_bytes, d_out, out_stride_bytes, hip_stream);
}

int pirip_hip_ping_records(pirip_hip_ping *p, const uint8_t **d_status, size_t *status_stride, const uint8_t **d_payload, size_t *payload_stride,
                           const int32_t **d_info, size_t *info_stride, const float **d_stats, size_t *stats_stride, const int32_t **d_nframes)
{
    if (!p || !p->last_status) return PIRIP_ERR_BAD_ARG;
    if (d_status) *d_status = p->last_status;
    if (status_stride) *status_stride = p->last_status_stride;
    if (d_payload) *d_payload = p->last_payload;
    if (payload_stride) *payload_stride = p->last_payload_stride;
    if (d_info) *d_info = p->last_info;
    if (info_stride) *info_stride = p->last_info_stride;
    if (d_stats) *d_stats = p->last_stats;
    if (stats_stride) *stats_stride = p->last_stats_stride;
    if (d_nframes) *d_nframes = p->last_nframes;
    return PIRIP_OK;
}

int pirip_hip_ping_offered(pirip_hip_ping *p, const uint8_t **d_records, size_t *rec_stride, const int32_t **d_nrec)
{
    if (!p || !p->tx) return PIRIP_ERR_BAD_ARG;
    if (d_records) *d_records = p->d_offered;
    if (rec_stride) *rec_stride = (size_t)(p->frames + 1) * (size_t)(1 + p->kb);
    if (d_nrec) *d_nrec = p->d_noffered;
    return PIRIP_OK;
}

int pirip_hip_ping_get_counters(pirip_hip_ping *p, int64_t *frames, int64_t *filtered, int64_t *decoded, int64_t *crc_fail, int64_t *bit_errors,
                                int64_t *lost, int64_t *bursts_sent, int64_t *frames_sent, int64_t *skipped)
{
    if (!p) return PIRIP_ERR_BAD_ARG;
    std::vector<PingRxState> rs((size_t)p->nrx);
    PIRIP_TRY(read_back(p->device, p->d_rx_state, rs));
    for (size_t c = 0; c < rs.size(); c++) {
        if (frames) frames[c] = rs[c].written;
        if (filtered) filtered[c] = rs[c].filtered;
        if (decoded) decoded[c] = rs[c].decoded;
        if (crc_fail) crc_fail[c] = rs[c].crc_fail;
        if (bit_errors) bit_errors[c] = rs[c].bit_errors;
        if (lost) lost[c] = rs[c].written > p->log_entries ? rs[c].written - p->log_entries : 0;      // what the ring no longer holds
    }
    if (!p->tx) return PIRIP_OK;
    std::vector<PingTxState> ts((size_t)p->ntx);
    PIRIP_TRY(read_back(p->device, p->d_tx_state, ts));
    for (size_t t = 0; t < ts.size(); t++) {
        if (bursts_sent) bursts_sent[t] = ts[t].bursts_sent;
        if (frames_sent) frames_sent[t] = ts[t].frames_sent;
        if (skipped) skipped[t] = ts[t].skipped;
    }
    return PIRIP_OK;
}

int pirip_hip_ping_get_log(pirip_hip_ping *p, int chan, pirip_ping_entry *entries, int max, int *written)
{
    if (!p || chan < 0 || chan >= p->nrx || max < 0 || (max > 0 && !entries)) return PIRIP_ERR_BAD_ARG;
    std::vector<PingRxState> rs((size_t)p->nrx);
    PIRIP_TRY(read_back(p->device, p->d_rx_state, rs));
    const int64_t total = rs[(size_t)chan].written;
    int64_t n = total < p->log_entries ? total : p->log_entries;
    if (n > max) n = max;
    if (n > 0) {
        std::vector<pirip_ping_entry> ring((size_t)p->log_entries);
        PIRIP_TRY(read_back(p->device, p->d_log + (size_t)chan * (size_t)p->log_entries, ring));
        for (int64_t i = 0; i < n; i++) entries[i] = ring[(size_t)((total - n + i) % p->log_entries)];
    }
    if (written) *written = (int)n;
    return PIRIP_OK;
}

int pirip_hip_ping_reset(pirip_hip_ping *p, void *hip_stream)
{
    if (!p) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(p->device)) return PIRIP_ERR_NO_DEVICE;
    PIRIP_TRY(ping_clear(p, (hipStream_t)hip_stream));
    if (p->txs) PIRIP_TRY(pirip_hip_txs_reset(p->txs, hip_stream));
    if (p->rx) PIRIP_TRY(pirip_hip_rx_reset(p->rx, hip_stream));
    p->last_status = nullptr;
    return PIRIP_OK;
}

}  // extern "C"
