// pirip_amd/csrc/rpt_kernels.hip -- include/pirip_hip.h section M: the streaming repeater.
// One call per block: received FSK_LDPC records -> rtl_fsk's --filter -> frame_repeater.c's state machine -> finished bursts in a pending
// ring per transmit channel -> whole bursts into section K's symbol queue when they are due and fit -> one block of wideband IQ.
//
//   intake:  records --rpt_intake_kernel (one wave per receive channel)--> pending ring of route[c]
//   offer:   pending ring --rpt_offer_kernel (one wave per transmit channel)--> record rows --section K's send path--> symbol queue
//   process: pirip_hip_txs_process
//
// The pending rings and the offer step are burst_ring.hpp's, shared with the packet link (section R). route's non-negative entries are
// distinct, so a ring has one writer: the intake.
// The call index n is host state advanced when a call is enqueued, as the sample index of section K.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/pirip_hip.h"
#include "hip_host.hpp"
#include "ldpc_handle.hpp"
#include "mux_handle.hpp"
#include "burst_ring.hpp"
#include "repeat_device.hpp"
#include "rpt_handle.hpp"
#include "tx_handle.hpp"
#include "txs_handle.hpp"

using namespace pirip;

namespace {

struct IntakeArgs {
    RepeatIn in;
    const int32_t *route;                  // [nrx]
    RptRxCount *cnt;                       // [nrx]
    BurstRingView v;
    int filter;
    int64_t ready_at;                      // n + holdoff
};

// One wave per receive channel: repeat_device.hpp's body with the filter applied to the status bytes it stages. Behind the walk lane 0
// places every burst that ended: its first record's offset behind the ring's tail, or nowhere (-2: no route, or no room for all of it).
// The wave's copies then go into the ring of route[c], across its wrap.
__global__ __launch_bounds__(64) void rpt_intake_kernel(IntakeArgs a)
{
    __shared__ int32_t s_start;                              // the ring slot of the tail
    const int c = blockIdx.x, t = a.route[c];
    int nfilt = 0;
    auto status = [&](uint8_t v, const uint8_t *frame) {     // rtl_fsk --filter: a frame of the repeater's own is no frame
        if ((v & PIRIP_RX_BITS) && a.filter >= 0 && frame[0] == (uint8_t)a.filter) { v = (uint8_t)(v & ~PIRIP_RX_BITS); nfilt++; }
        return v;
    };
    auto place = [&](int nb, int32_t *base, const int32_t *nfr) {
        int64_t frames = 0, unrouted = 0, dropped = 0;
        int off = 0, start = 0;
        if (t >= 0) {
            const uint64_t head = a.v.rs[t].head, tail = a.v.rs[t].tail;
            int64_t room = (int64_t)a.v.pending - (int64_t)(tail - head);
            start = (int)(tail % (uint64_t)a.v.pending);
            for (int b = 0; b < nb; b++) {
                frames += nfr[b];
                base[b] = burst_ring_place(a.v, t, nfr[b] + 1, a.ready_at, start, off, room);
                dropped += base[b] < 0;
            }
            a.v.rs[t].tail = tail + (uint64_t)off;
            a.v.rs[t].dropped += dropped;
        } else {
            for (int b = 0; b < nb; b++) { frames += nfr[b]; base[b] = -2; unrouted++; }
        }
        s_start = start;
        a.cnt[c].bursts += nb; a.cnt[c].frames += frames; a.cnt[c].unrouted += unrouted;
    };
    repeat_stream(a.in, c, status, place, [&](int base, int j) { return base >= 0 ? burst_ring_record(a.v, t, s_start, base + j) : nullptr; });
    nfilt = wave_sum(nfilt);
    if (threadIdx.x == 0) a.cnt[c].filtered += nfilt;
}

int rpt_clear(pirip_hip_rpt *r, hipStream_t st)
{
    PIRIP_HIPCHK(hipMemsetAsync(r->d_state, 0, sizeof(int32_t) * 2 * (size_t)r->nrx, st));
    PIRIP_HIPCHK(hipMemsetAsync(r->d_cnt, 0, sizeof(RptRxCount) * (size_t)r->nrx, st));
    PIRIP_TRY(r->rings.clear(st));
    r->calls = 0;
    return PIRIP_OK;
}

int rpt_alloc(pirip_hip_rpt *r, const int32_t *route)
{
    const size_t nrx = (size_t)r->nrx;
    DevMem &m = r->mem;
    PIRIP_TRY(m.upload(&r->d_route, route, sizeof(int32_t) * nrx));
    PIRIP_TRY(m.alloc(&r->d_state, sizeof(int32_t) * 2 * nrx));
    PIRIP_TRY(m.alloc_filled(&r->d_held, 0, nrx * (size_t)r->max_burst * (size_t)r->kb));
    PIRIP_TRY(m.alloc(&r->d_cnt, sizeof(RptRxCount) * nrx));
    PIRIP_TRY(r->rings.alloc(m, r->ntx, r->pending, 1 + r->kb));
    if (r->rx) {
        const size_t R = (size_t)r->rx_rows;
        PIRIP_TRY(m.alloc_filled(&r->d_status, 0, nrx * R));
        PIRIP_TRY(m.alloc_filled(&r->d_payload, 0, nrx * R * (size_t)r->kb));
        PIRIP_TRY(m.alloc_filled(&r->d_info, 0, sizeof(int32_t) * nrx * R * PIRIP_LDPC_INFO_PER_CALL));
        PIRIP_TRY(m.alloc_filled(&r->d_nframes, 0, sizeof(int32_t) * nrx));
    }
    PIRIP_TRY(txs_reserve(r->txs, r->pending));
    PIRIP_TRY(rpt_clear(r, nullptr));
    PIRIP_HIPCHK(hipDeviceSynchronize());
    return PIRIP_OK;
}

// steps 1 - 3 over record rows that are on the device; the handle's device is current
int rpt_run(pirip_hip_rpt *r, const uint8_t *d_status, size_t status_stride, const uint8_t *d_payload, size_t payload_stride, const int32_t *d_ncalls,
            int ncalls, void *d_out, size_t out_stride_bytes, hipStream_t st)
{
    IntakeArgs ia{};
    ia.in = RepeatIn{d_status, status_stride, d_payload, payload_stride, d_ncalls, ncalls, r->d_state, r->d_held, r->kb, r->max_burst, r->source};
    ia.route = r->d_route; ia.cnt = r->d_cnt; ia.v = r->rings.view();
    ia.filter = r->filter;
    ia.ready_at = r->calls + r->holdoff;
    hipLaunchKernelGGL(rpt_intake_kernel, dim3((unsigned)r->nrx), dim3(64), repeat_lds_bytes(ncalls), st, ia);
    PIRIP_TRY(r->rings.offer_and_process(r->tx, r->txs, r->calls, d_out, out_stride_bytes, st));
    r->calls++;
    return PIRIP_OK;
}

// txs_process's own checks, made before anything is enqueued: a call either runs whole or not at all
int rpt_check_out(const pirip_hip_rpt *r, const void *d_out, size_t out_stride_bytes)
{
    if (!d_out) return PIRIP_ERR_BAD_ARG;
    return iq_rows_check(d_out, out_stride_bytes, r->txs->mux->bs, r->txs->mux->noutputs, r->txs->block);
}

}  // namespace

extern "C" {

int pirip_hip_rpt_create(pirip_hip_rx *rx, pirip_hip_tx *tx, pirip_hip_txs *txs, int nrx, const int32_t *route, int source_byte, int filter_byte,
                         int holdoff_calls, int max_burst_frames, int pending_records, pirip_hip_rpt **out)
{
    if (!out) return PIRIP_ERR_BAD_ARG;
    *out = nullptr;
    if (!tx || !txs || !route || nrx < 1 || txs->tx != tx || txs->device != tx->device) return PIRIP_ERR_BAD_ARG;
    if (source_byte < 0 || source_byte > 255 || filter_byte < -1 || filter_byte > 255 || holdoff_calls < 0) return PIRIP_ERR_BAD_ARG;
    if (max_burst_frames < 1 || max_burst_frames > PIRIP_TX_REPEAT_MAX_FRAMES || pending_records < max_burst_frames + 1) return PIRIP_ERR_BAD_ARG;
    const int ntx = tx->nstreams, kb = tx->code.data_bytes();
    for (int c = 0; c < nrx; c++) {
        if (route[c] >= ntx) return PIRIP_ERR_BAD_ARG;
        for (int q = 0; q < c; q++) if (route[c] >= 0 && route[q] == route[c]) return PIRIP_ERR_BAD_ARG;
    }
    const int64_t psyms = tx_pre_syms(tx), fsyms = tx_frame_syms(tx);
    if (psyms + (int64_t)max_burst_frames * fsyms + tx->max_gap > txs->queue_syms) return PIRIP_ERR_BAD_ARG;
    int rx_rows = 0;
    if (rx) {
        int ns = 0, dev = 0;
        const pirip_hip_ldpc *ldpc = nullptr;
        rx_handle_shape(rx, &ns, &ldpc, &dev);
        if (!ldpc || ns != nrx || dev != tx->device || ldpc->code.data_bytes() != kb) return PIRIP_ERR_BAD_ARG;
        const int64_t rows = pirip_hip_rx_max_frames(rx);
        if (rows < 1) return PIRIP_ERR_BAD_ARG;
        if (rows > kRepeatMaxCalls) return PIRIP_ERR_UNSUPPORTED;
        rx_rows = (int)rows;
    }
    PIRIP_TRY(burst_rings_check(tx, pending_records));
    if (!bind_device(tx->device)) return PIRIP_ERR_NO_DEVICE;
    pirip_hip_rpt *r = new (std::nothrow) pirip_hip_rpt();
    if (!r) return PIRIP_ERR_NOMEM;
    r->rx = rx; r->tx = tx; r->txs = txs; r->nrx = nrx; r->ntx = ntx; r->device = tx->device; r->kb = kb;
    r->source = source_byte; r->filter = filter_byte; r->holdoff = holdoff_calls; r->max_burst = max_burst_frames; r->pending = pending_records;
    r->rx_rows = rx_rows;
    const int rc = rpt_alloc(r, route);
    if (rc != PIRIP_OK) { delete r; return rc; }
    *out = r;
    return PIRIP_OK;
}

int pirip_hip_rpt_destroy(pirip_hip_rpt *r) { return destroy_handle(r, r ? r->device : 0); }

int pirip_hip_rpt_get_info(const pirip_hip_rpt *r, pirip_rpt_info *info)
{
    if (!r || !info) return PIRIP_ERR_BAD_ARG;
    *info = pirip_rpt_info{r->nrx, r->ntx, r->source, r->filter, r->holdoff, r->max_burst, r->pending, r->rx ? 1 : 0, r->rx_rows, r->device};
    return PIRIP_OK;
}

int pirip_hip_rpt_push_records(pirip_hip_rpt *r, const uint8_t *d_status, size_t status_stride, const uint8_t *d_payload, size_t payload_stride,
                               const int32_t *d_ncalls, int ncalls, void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    if (!r || !d_status || !d_payload || ncalls < 0) return PIRIP_ERR_BAD_ARG;
    if (r->nrx > 1 && (status_stride < (size_t)ncalls || payload_stride < (size_t)ncalls * (size_t)r->kb)) return PIRIP_ERR_BAD_ARG;
    if (ncalls > kRepeatMaxCalls) return PIRIP_ERR_UNSUPPORTED;
    PIRIP_TRY(rpt_check_out(r, d_out, out_stride_bytes));
    if (!bind_device(r->device)) return PIRIP_ERR_NO_DEVICE;
    PIRIP_TRY(rpt_run(r, d_status, status_stride, d_payload, payload_stride, d_ncalls, ncalls, d_out, out_stride_bytes, (hipStream_t)hip_stream));
    r->last_status = d_status; r->last_status_stride = status_stride; r->last_payload = d_payload; r->last_payload_stride = payload_stride;
    r->last_info = nullptr; r->last_info_stride = 0; r->last_nframes = d_ncalls;
    return PIRIP_OK;
}

static int rpt_receive(pirip_hip_rpt *r, const void *d_in, size_t in_stride_bytes, void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    if (!r || !r->rx) return PIRIP_ERR_BAD_ARG;
    PIRIP_TRY(rpt_check_out(r, d_out, out_stride_bytes));
    if (!bind_device(r->device)) return PIRIP_ERR_NO_DEVICE;
    const size_t R = (size_t)r->rx_rows;
    if (d_in)
        PIRIP_TRY(pirip_hip_rx_push(r->rx, d_in, in_stride_bytes, nullptr, 0, nullptr, 0, r->d_status, r->d_payload, r->d_info, nullptr, 0, r->d_nframes,
                                    hip_stream));
    else
        PIRIP_TRY(pirip_hip_rx_process(r->rx, nullptr, 0, nullptr, 0, r->d_status, r->d_payload, r->d_info, nullptr, 0, r->d_nframes, hip_stream));
    r->last_status = r->d_status; r->last_status_stride = R; r->last_payload = r->d_payload; r->last_payload_stride = R * (size_t)r->kb;
    r->last_info = r->d_info; r->last_info_stride = R * PIRIP_LDPC_INFO_PER_CALL; r->last_nframes = r->d_nframes;
    return rpt_run(r, r->d_status, R, r->d_payload, R * (size_t)r->kb, r->d_nframes, r->rx_rows, d_out, out_stride_bytes, (hipStream_t)hip_stream);
}

int pirip_hip_rpt_process(pirip_hip_rpt *r, void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    return rpt_receive(r, nullptr, 0, d_out, out_stride_bytes, hip_stream);
}

int pirip_hip_rpt_push(pirip_hip_rpt *r, const void *d_in, size_t in_stride_bytes, void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    if (!d_in) return PIRIP_ERR_BAD_ARG;
    return rpt_receive(r, d_in, in_stride_bytes, d_out, out_stride_bytes, hip_stream);
}

int pirip_hip_rpt_records(pirip_hip_rpt *r, const uint8_t **d_status, size_t *status_stride, const uint8_t **d_payload, size_t *payload_stride,
                          const int32_t **d_info, size_t *info_stride, const int32_t **d_nframes)
{
    if (!r || !r->last_status) return PIRIP_ERR_BAD_ARG;
    if (d_status) *d_status = r->last_status;
    if (status_stride) *status_stride = r->last_status_stride;
    if (d_payload) *d_payload = r->last_payload;
    if (payload_stride) *payload_stride = r->last_payload_stride;
    if (d_info) *d_info = r->last_info;
    if (info_stride) *info_stride = r->last_info_stride;
    if (d_nframes) *d_nframes = r->last_nframes;
    return PIRIP_OK;
}

int pirip_hip_rpt_offered(pirip_hip_rpt *r, const uint8_t **d_records, size_t *rec_stride, const int32_t **d_nrec)
{
    if (!r) return PIRIP_ERR_BAD_ARG;
    if (d_records) *d_records = r->rings.d_offered;
    if (rec_stride) *rec_stride = r->rings.row_bytes();
    if (d_nrec) *d_nrec = r->rings.d_noffered;
    return PIRIP_OK;
}

int pirip_hip_rpt_get_counters(pirip_hip_rpt *r, int64_t *bursts_in, int64_t *frames_in, int64_t *filtered, int64_t *unrouted,
                               int64_t *bursts_out, int64_t *pending, int64_t *dropped)
{
    if (!r) return PIRIP_ERR_BAD_ARG;
    std::vector<RptRxCount> rc((size_t)r->nrx);
    std::vector<BurstRing> rs((size_t)r->ntx);
    PIRIP_TRY(read_back(r->device, r->d_cnt, rc));
    PIRIP_TRY(read_back(r->device, r->rings.d_state, rs));
    for (size_t c = 0; c < rc.size(); c++) {
        if (bursts_in) bursts_in[c] = rc[c].bursts;
        if (frames_in) frames_in[c] = rc[c].frames;
        if (filtered) filtered[c] = rc[c].filtered;
        if (unrouted) unrouted[c] = rc[c].unrouted;
    }
    for (size_t t = 0; t < rs.size(); t++) {
        if (bursts_out) bursts_out[t] = rs[t].bursts_out;
        if (pending) pending[t] = (int64_t)(rs[t].tail - rs[t].head);
        if (dropped) dropped[t] = rs[t].dropped;
    }
    return PIRIP_OK;
}

int pirip_hip_rpt_reset(pirip_hip_rpt *r, void *hip_stream)
{
    if (!r) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(r->device)) return PIRIP_ERR_NO_DEVICE;
    PIRIP_TRY(rpt_clear(r, (hipStream_t)hip_stream));
    PIRIP_TRY(pirip_hip_txs_reset(r->txs, hip_stream));
    if (r->rx) PIRIP_TRY(pirip_hip_rx_reset(r->rx, hip_stream));
    r->last_status = nullptr;
    return PIRIP_OK;
}

}  // extern "C"
