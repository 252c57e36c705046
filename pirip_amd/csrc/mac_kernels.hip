// pirip_amd/csrc/mac_kernels.hip -- include/pirip_hip.h section T: half-duplex medium access over a packet handle.
//
//   sense: the call's status (and stats) rows --mac_sense_kernel (one wave per receive channel)--> carrier / own, the idle run, and the
//          rows as the reassembly reads them: a copy, without PIRIP_RX_BITS while the own transmitter was on air
//   gate:  the pending ring's head, section K's queue, the paired idle run --mac_gate_kernel (one thread per transmit channel)--> the
//          gate's state and the offer's limit (burst_ring.hpp: BurstLimit, which the offer itself advances by what it took)
// pkt_kernels.hip enqueues both in front of its own launches of a call while a handle is attached (mac_before). Step 0's `air` is read off
// section K's queue: the gate of call n - 1 keeps the head it saw, in front of that call's process, and call n compares. The sense kernel
// works step 0 out for the paired channel without storing it (the gate, which runs behind it, stores it for every channel), so no launch
// writes what another wave of the same launch reads.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <vector>

#include "../../include/pirip_hip.h"
#include "burst_ring.hpp"
#include "hip_host.hpp"
#include "mac_device.hpp"
#include "mac_handle.hpp"
#include "pkt_handle.hpp"
#include "repeat_device.hpp"
#include "rows_device.hpp"
#include "txs_handle.hpp"

using namespace pirip;

namespace {

// step 0 for one transmit channel: its quiet run in this call
__device__ __forceinline__ int mac_quiet_now(const MacTxState &s, const TxsChanState &q)
{
    const bool air = s.have_prev && q.head != s.prev_head;
    return mac_run_next(s.quiet, air);
}

// One wave per receive channel: the lanes stride over the rows, each ORs its rows' carrier, counts its rows' BITS and writes its rows of
// the copy; one wave reduction; the decision and the state live in scalars.
__global__ __launch_bounds__(64) void mac_sense_kernel(MacSenseArgs a)
{
    const size_t c = blockIdx.x;
    const int lane = threadIdx.x;
    const int nf = __builtin_amdgcn_readfirstlane(row_count(a.nrows, c, a.max_rows));
    const int t = __builtin_amdgcn_readfirstlane(a.tx_of_rx[c]);
    int own = 0;
    if (t >= 0) own = mac_quiet_now(a.tx[t], a.queue[t]) < a.mute_calls;
    own = __builtin_amdgcn_readfirstlane(own);
    const uint8_t *st = a.status + c * a.status_stride;
    const float *ss = a.stats ? a.stats + c * a.stats_stride : nullptr;
    uint8_t *out = a.status_out + c * a.out_stride;
    const uint8_t keep = own ? (uint8_t)~PIRIP_RX_BITS : (uint8_t)0xff;
    int heard = 0, bits = 0;
    for (int f = lane; f < nf; f += 64) {
        const uint8_t v = st[f];
        if ((a.sense_mask & 1) && (v & PIRIP_RX_SYNC)) heard = 1;
        if ((a.sense_mask & 2) && ss && ss[(size_t)f * PIRIP_STATS_PER_FRAME + 5] >= a.sense_snr) heard = 1;      // (a NaN compares false)
        bits += (v & PIRIP_RX_BITS) != 0;
        out[f] = v & keep;
    }
    const int carrier = !own && __builtin_amdgcn_readfirstlane(wave_sum(heard)) != 0;
    const int muted = own ? __builtin_amdgcn_readfirstlane(wave_sum(bits)) : 0;
    if (lane == 0) {
        MacRxState s = a.rx[c];
        s.carrier += carrier; s.own += own; s.muted += muted;
        s.idle = mac_run_next(s.idle, own || carrier);
        a.rx[c] = s;
    }
}

// create / reset: nothing was on air for as long as the run counts
__global__ __launch_bounds__(64) void mac_quiet_kernel(MacTxState *tx, int ntx)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < ntx) tx[t].quiet = kMacRunMax;
}

// One thread per transmit channel: step 0's state, then step 2.
__global__ __launch_bounds__(64) void mac_gate_kernel(MacGateArgs a, int ntx)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= ntx) return;
    MacTxState s = a.tx[t];
    const TxsChanState q = a.queue[t];
    s.quiet = mac_quiet_now(s, q);
    s.prev_head = q.head; s.have_prev = 1;
    const int c = a.rx_of_tx[t];
    BurstLimit lim = a.limit[t];
    if (c < 0) {
        lim.limit = -1;                                          // ungated: the offer's own rules alone
    } else {
        const uint64_t head = a.v.rs[t].head, tail = a.v.rs[t].tail;
        const bool due = head < tail && a.v.ready[(size_t)t * a.v.pending + (size_t)(head % (uint64_t)a.v.pending)] <= a.now;
        s.g.run = lim.run;
        lim.limit = mac_gate_step(s.g, a.r, t, due, q.tail != q.head, a.rx[c].idle);
        lim.run = s.g.run;
    }
    a.limit[t] = lim;
    a.tx[t] = s;
}

}  // namespace

int pirip::mac_before(pirip_hip_mac *m, const uint8_t *d_status, size_t status_stride, const float *d_stats, size_t stats_stride,
                      const int32_t *d_ncalls, int ncalls, int64_t now, const uint8_t **status_out, size_t *out_stride, BurstLimit **limit,
                      hipStream_t st)
{
    const pirip_hip_pkt *p = m->pkt;
    MacSenseArgs sa{};
    sa.status = d_status; sa.status_stride = status_stride; sa.stats = d_stats; sa.stats_stride = stats_stride;
    sa.nrows = d_ncalls; sa.max_rows = ncalls;
    sa.status_out = m->d_status; sa.out_stride = (size_t)kRepeatMaxCalls;
    sa.tx_of_rx = m->d_tx_of_rx; sa.tx = m->d_tx; sa.queue = p->txs->d_state; sa.rx = m->d_rx;
    sa.sense_mask = m->cfg.sense_mask; sa.mute_calls = m->cfg.mute_calls; sa.sense_snr = m->cfg.sense_snr;
    hipLaunchKernelGGL(mac_sense_kernel, dim3((unsigned)m->nrx), dim3(64), 0, st, sa);
    PIRIP_HIPCHK(hipGetLastError());
    MacGateArgs ga{};
    ga.v = p->rings.view(); ga.queue = p->txs->d_state; ga.rx_of_tx = m->d_rx_of_tx; ga.rx = m->d_rx; ga.tx = m->d_tx; ga.limit = m->d_limit;
    ga.r = MacRules{m->cfg.slot_calls, m->cfg.cw, m->cfg.ifs_calls, m->cfg.txop_bursts, m->cfg.key};
    ga.now = now;
    hipLaunchKernelGGL(mac_gate_kernel, dim3((unsigned)((m->ntx + 63) / 64)), dim3(64), 0, st, ga, m->ntx);
    PIRIP_HIPCHK(hipGetLastError());
    *status_out = m->d_status; *out_stride = (size_t)kRepeatMaxCalls; *limit = m->d_limit;
    return PIRIP_OK;
}

int pirip::mac_clear(pirip_hip_mac *m, hipStream_t st)
{
    PIRIP_HIPCHK(hipMemsetAsync(m->d_tx, 0, sizeof(MacTxState) * (size_t)m->ntx, st));
    hipLaunchKernelGGL(mac_quiet_kernel, dim3((unsigned)((m->ntx + 63) / 64)), dim3(64), 0, st, m->d_tx, m->ntx);
    PIRIP_HIPCHK(hipGetLastError());
    PIRIP_HIPCHK(hipMemsetAsync(m->d_rx, 0, sizeof(MacRxState) * (size_t)m->nrx, st));
    PIRIP_HIPCHK(hipMemsetAsync(m->d_limit, 0, sizeof(BurstLimit) * (size_t)m->ntx, st));
    return PIRIP_OK;
}

extern "C" {

int pirip_hip_mac_create(pirip_hip_pkt *pkt, const pirip_mac_config *cfg, const int32_t *rx_of_tx, pirip_hip_mac **out)
{
    if (!out) return PIRIP_ERR_BAD_ARG;
    *out = nullptr;
    if (!pkt || !cfg || !rx_of_tx || !pkt->tx || pkt->mac) return PIRIP_ERR_BAD_ARG;
    if (cfg->sense_mask < 1 || cfg->sense_mask > 3 || cfg->slot_calls < 1 || cfg->slot_calls > kMacMaxSlotCalls || cfg->cw < 1 || cfg->cw > kMacMaxCw ||
        cfg->ifs_calls < 0 || cfg->ifs_calls >= kMacRunMax || cfg->mute_calls < 0 || cfg->mute_calls > kMacRunMax || cfg->txop_bursts < 1 ||
        cfg->txop_bursts > kMacRunMax)
        return PIRIP_ERR_BAD_ARG;
    std::vector<int32_t> tx_of_rx((size_t)pkt->nrx, -1);
    for (int t = 0; t < pkt->ntx; t++) {
        const int c = rx_of_tx[t];
        if (c < -1 || c >= pkt->nrx) return PIRIP_ERR_BAD_ARG;
        if (c < 0) continue;
        if (tx_of_rx[(size_t)c] >= 0) return PIRIP_ERR_BAD_ARG;
        tx_of_rx[(size_t)c] = t;
    }
    if (!bind_device(pkt->device)) return PIRIP_ERR_NO_DEVICE;
    pirip_hip_mac *m = new (std::nothrow) pirip_hip_mac();
    if (!m) return PIRIP_ERR_NOMEM;
    m->pkt = pkt; m->ntx = pkt->ntx; m->nrx = pkt->nrx; m->device = pkt->device; m->cfg = *cfg;
    auto alloc = [&]() {
        DevMem &mem = m->mem;
        PIRIP_TRY(mem.alloc(&m->d_tx, sizeof(MacTxState) * (size_t)m->ntx));
        PIRIP_TRY(mem.alloc(&m->d_rx, sizeof(MacRxState) * (size_t)m->nrx));
        PIRIP_TRY(mem.alloc(&m->d_limit, sizeof(BurstLimit) * (size_t)m->ntx));
        PIRIP_TRY(mem.upload(&m->d_rx_of_tx, rx_of_tx, sizeof(int32_t) * (size_t)m->ntx));
        PIRIP_TRY(mem.upload(&m->d_tx_of_rx, tx_of_rx.data(), sizeof(int32_t) * (size_t)m->nrx));
        PIRIP_TRY(mem.alloc_filled(&m->d_status, 0, (size_t)m->nrx * (size_t)kRepeatMaxCalls));
        if (pkt->rx && (cfg->sense_mask & 2))
            PIRIP_TRY(mem.alloc_filled(&m->d_stats, 0, sizeof(float) * (size_t)m->nrx * (size_t)pkt->rx_rows * PIRIP_STATS_PER_FRAME));
        PIRIP_TRY(mac_clear(m, nullptr));
        PIRIP_HIPCHK(hipDeviceSynchronize());
        return (int)PIRIP_OK;
    };
    const int rc = alloc();
    if (rc != PIRIP_OK) { delete m; return rc; }
    pkt->mac = m;
    *out = m;
    return PIRIP_OK;
}

int pirip_hip_mac_destroy(pirip_hip_mac *m)
{
    if (!m) return PIRIP_ERR_BAD_ARG;
    (void)bind_device(m->device);
    (void)hipDeviceSynchronize();                                // the packet handle's enqueued calls still read this handle's memory
    m->pkt->mac = nullptr;
    delete m;
    return PIRIP_OK;
}

int pirip_hip_mac_get_info(const pirip_hip_mac *m, pirip_mac_info *info)
{
    if (!m || !info) return PIRIP_ERR_BAD_ARG;
    const pirip_mac_config &c = m->cfg;
    *info = pirip_mac_info{m->ntx, m->nrx, c.sense_mask, c.sense_snr, c.slot_calls, c.cw, c.ifs_calls, c.mute_calls, c.txop_bursts, c.key, m->device};
    return PIRIP_OK;
}

int pirip_hip_mac_set_stats(pirip_hip_mac *m, const float *d_stats, size_t stats_stride)
{
    if (!m || (m->pkt->rx && (m->cfg.sense_mask & 2))) return PIRIP_ERR_BAD_ARG;
    m->user_stats = d_stats; m->user_stats_stride = stats_stride;
    return PIRIP_OK;
}

int pirip_hip_mac_stats(pirip_hip_mac *m, const float **d_stats, size_t *stats_stride)
{
    if (!m) return PIRIP_ERR_BAD_ARG;
    if (d_stats) *d_stats = m->d_stats ? m->d_stats : m->user_stats;
    if (stats_stride) *stats_stride = m->d_stats ? (size_t)m->pkt->rx_rows * PIRIP_STATS_PER_FRAME : m->user_stats_stride;
    return PIRIP_OK;
}

int pirip_hip_mac_get_counters(pirip_hip_mac *m, int64_t *accesses, int64_t *won, int64_t *backoff, int64_t *deferred, int64_t *bursts,
                               int64_t *carrier, int64_t *own, int64_t *muted)
{
    if (!m) return PIRIP_ERR_BAD_ARG;
    std::vector<MacTxState> tx((size_t)m->ntx);
    std::vector<BurstLimit> lim((size_t)m->ntx);
    std::vector<MacRxState> rx((size_t)m->nrx);
    PIRIP_TRY(read_back(m->device, m->d_tx, tx));
    PIRIP_TRY(read_back(m->device, m->d_limit, lim));
    PIRIP_TRY(read_back(m->device, m->d_rx, rx));
    for (size_t t = 0; t < tx.size(); t++) {
        if (accesses) accesses[t] = tx[t].g.accesses;
        if (won) won[t] = tx[t].g.won;
        if (backoff) backoff[t] = tx[t].g.backoff;
        if (deferred) deferred[t] = tx[t].g.deferred;
        if (bursts) bursts[t] = lim[t].bursts;
    }
    for (size_t c = 0; c < rx.size(); c++) {
        if (carrier) carrier[c] = rx[c].carrier;
        if (own) own[c] = rx[c].own;
        if (muted) muted[c] = rx[c].muted;
    }
    return PIRIP_OK;
}

int pirip_hip_mac_get_state(pirip_hip_mac *m, int t, int *phase, int *counter, int *run, int *quiet, int *idle)
{
    if (!m || t < 0 || t >= m->ntx) return PIRIP_ERR_BAD_ARG;
    std::vector<MacTxState> tx(1);
    std::vector<BurstLimit> lim(1);
    std::vector<int32_t> c(1);
    PIRIP_TRY(read_back(m->device, m->d_tx + t, tx));
    PIRIP_TRY(read_back(m->device, m->d_limit + t, lim));
    PIRIP_TRY(read_back(m->device, m->d_rx_of_tx + t, c));
    if (phase) *phase = tx[0].g.phase;
    if (counter) *counter = tx[0].g.counter;
    if (run) *run = lim[0].run;
    if (quiet) *quiet = tx[0].quiet;
    if (idle) {
        *idle = -1;
        if (c[0] >= 0) {
            std::vector<MacRxState> rx(1);
            PIRIP_TRY(read_back(m->device, m->d_rx + c[0], rx));
            *idle = rx[0].idle;
        }
    }
    return PIRIP_OK;
}

int pirip_hip_mac_reset(pirip_hip_mac *m, void *hip_stream)
{
    if (!m) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(m->device)) return PIRIP_ERR_NO_DEVICE;
    return mac_clear(m, (hipStream_t)hip_stream);
}

}  // extern "C"
