// pirip_amd/csrc/txs_kernels.hip -- include/pirip_hip.h section K: the streaming transmitter, section G's mirror image.
// Every channel has a queue of channel symbols on the device; one call turns the next S symbols of every queue into `block` wideband
// samples per output. It borrows a transmitter (section I: code, framer, tones, gap) and a multiplexer (section J: taps, offsets, gains,
// outputs, format) and keeps its own phases, history and counters.
//
//   send:     records --tx_layout_kernel, tx_frame_kernel (section I's, into this handle's rows)--> symbols --txs_append_kernel--> ring
//   process:  ring --txs_take_kernel--> the call's symbol row and its A_i --txs_mux_kernel--> wideband IQ
//
// Queue: one ring of queue_syms bytes per channel, head and tail 64-bit counts of symbols on the device (the host never knows the fill
// level). Append is all or nothing per channel: the symbols of a call's records go in, in order and across the wrap, when they fit the free
// space; else nothing does and the channel's refused count goes up.
// Symbol row of a channel and call:  [H | S]  with their A_i (tx_kernels.hip's exact phase integers) beside them
//   the last H = ceil((Q - 1) / Ts) symbols of the previous call (carrier off before the first), then up to S dequeued symbols padded with
//   carrier off. H symbols cover the Q - 1 modem samples the multiplexer's filter reaches back over: with e0 = H Ts - (Q - 1), input
//   sample `at` of the call is sample (e0 + at) mod Ts of symbol (e0 + at) div Ts of the row. Two such rows per channel, used in turn: a
//   call copies its history out of the other row and never reads what it writes.
// The fused multiplexer is mux_handle.hpp's mux_tile with another staging rule: instead of loading z[at] from a modem-rate row it forms
//   p = (A_i + (r + 1) f_i) mod Fs,  x = 2 (cospi, sinpi)(2p / Fs), 0 when the carrier is off
// -- the integer tx_mod_kernel reaches by its steps, and the same float operations on it -- so that a block equals, byte for byte, what
// pirip_hip_tx_modulate (complex float, no noise) and pirip_hip_mux_batch make of the same symbols. No modem-rate sample reaches memory.
// One division by Ts per thread and tile; from staged sample to staged sample the cursor moves by (256 div Ts, 256 mod Ts) with one carry.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/pirip_hip.h"
#include "hip_host.hpp"
#include "iq_device.hpp"
#include "mux_handle.hpp"
#include "repeat_device.hpp"
#include "tx_handle.hpp"
#include "txs_handle.hpp"

using namespace pirip;

namespace {

constexpr int kAppendThreads = 256;
constexpr uint8_t kOff = PIRIP_TX_CARRIER_OFF;

using ChanState = TxsChanState;

struct AppendArgs {
    const uint8_t *frm; size_t frm_stride; const int32_t *nsym;      // the framer's rows of this call
    const int32_t *nrec; int max_rec;
    uint8_t *ring; int64_t cap;
    ChanState *st;
    int32_t *taken;
};

__global__ __launch_bounds__(kAppendThreads) void txs_append_kernel(AppendArgs a)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    const uint64_t head = a.st[c].head, tail = a.st[c].tail;
    const int64_t n = a.nsym[c];
    const bool fits = n <= a.cap - (int64_t)(tail - head);
    if (fits) {
        const uint8_t *src = a.frm + (size_t)c * a.frm_stride;
        uint8_t *ring = a.ring + (size_t)c * (size_t)a.cap;
        const int64_t start = (int64_t)(tail % (uint64_t)a.cap);
        for (int64_t j = tid; j < n; j += kAppendThreads) ring[ring_slot(start, j, a.cap)] = src[j];
    }
    __syncthreads();                                         // every thread has read the counters
    if (tid == 0) {
        if (fits) a.st[c].tail = tail + (uint64_t)n;
        else a.st[c].refused++;
        if (a.taken) a.taken[c] = fits ? row_count(a.nrec, c, a.max_rec) : 0;
    }
}

struct TakeArgs {
    const uint8_t *ring; int64_t cap;
    ChanState *st;
    const uint8_t *prev_sy; uint8_t *cur_sy;                 // [nchan][row] symbols of the previous call and of this one
    const uint32_t *prev_pre; uint32_t *cur_pre;             // [nchan][row] their A_i
    size_t row;                                              // H + S
    int H, S, M, Fs;
    const uint32_t *tm;                                      // [nchan][4] (Ts * tone m) mod Fs
    int32_t *sent;
};

__global__ __launch_bounds__(kScanThreads) void txs_take_kernel(TakeArgs a)
{
    __shared__ uint32_t s_tot[kScanThreads / 64];
    const int c = blockIdx.x, tid = threadIdx.x;
    const uint64_t head = a.st[c].head, tail = a.st[c].tail;
    const uint32_t phase = a.st[c].phase;
    const int n = (int)(tail - head < (uint64_t)a.S ? tail - head : (uint64_t)a.S);
    uint8_t *sy = a.cur_sy + (size_t)c * a.row;
    uint32_t *pre = a.cur_pre + (size_t)c * a.row;
    for (int j = tid; j < a.H; j += kScanThreads) {
        sy[j] = a.prev_sy[(size_t)c * a.row + a.S + j];
        pre[j] = a.prev_pre[(size_t)c * a.row + a.S + j];
    }
    const uint8_t *ring = a.ring + (size_t)c * (size_t)a.cap;
    const int64_t start = (int64_t)(head % (uint64_t)a.cap);
    for (int j = tid; j < a.S; j += kScanThreads) sy[a.H + j] = j < n ? ring[ring_slot(start, (int64_t)j, a.cap)] : kOff;
    __syncthreads();
    const uint8_t *cur = sy + a.H;
    const uint32_t carry = tx_scan_row([&](int64_t i) { const int v = cur[i]; return v < a.M ? v : -1; }, a.S, a.tm + (size_t)c * 4, (uint32_t)a.Fs,
                                       phase, pre + a.H, s_tot);
    if (tid == 0) {
        a.st[c].head = head + (uint64_t)n;
        a.st[c].sent += n;
        a.st[c].underrun += a.S - n;
        a.st[c].phase = carry;
        if (a.sent) a.sent[c] = n;
    }
}

// mux_tile's staging rule: input sample `at` of the call, computed from the call's symbol rows
struct SymStage {
    const uint8_t *sy; const uint32_t *pre; size_t row;      // [nchan][row] symbols and A_i
    const uint32_t *fm;                                      // [nchan][4] tone m mod Fs
    int Ts, M, Fs, nrow;                                     // the modem's Fs; nrow = H + S
    int e0;                                                  // H Ts - (Q - 1): the row's sample that is input 0 of the call
    int step_i, step_r;                                      // 256 div Ts, 256 mod Ts
    float two_over_fs;
    double inv_fs_d;
    struct Cursor { int i, r; };                             // symbol of the row, sample of the symbol
    __device__ __forceinline__ Cursor begin(int64_t a0, int tid) const
    {
        const int e = (int)a0 + tid + e0;
        const int i = e / Ts;
        return Cursor{i, e - i * Ts};
    }
    __device__ __forceinline__ void next(Cursor &c) const
    {
        c.i += step_i; c.r += step_r;
        if (c.r >= Ts) { c.r -= Ts; c.i++; }
    }
    __device__ __forceinline__ float2 sample(int ch, const Cursor &c, int64_t) const
    {
        if (c.i >= nrow) return make_float2(0.f, 0.f);
        const int sym = sy[(size_t)ch * row + c.i];
        if (sym >= M) return make_float2(0.f, 0.f);          // carrier off
        const uint32_t f = fm[(size_t)ch * 4 + sym];
        uint32_t p = pre[(size_t)ch * row + c.i] + (uint32_t)mulmod_fs((uint32_t)(c.r + 1), f, Fs, inv_fs_d);
        if (p >= (uint32_t)Fs) p -= (uint32_t)Fs;
        float sn, cs;
        unit_phasor((int32_t)p, Fs, two_over_fs, cs, sn);
        return make_float2(2 * cs, 2 * sn);
    }
};

template <int BS>
__global__ __launch_bounds__(kMuxThreads) void txs_mux_kernel(MuxArgs a, SymStage st) { mux_tile<BS>(a, st); }

}  // namespace

namespace {

int txs_clear(pirip_hip_txs *t, hipStream_t st)
{
    const size_t rows = 2 * (size_t)t->nchan * t->row;
    PIRIP_HIPCHK(hipMemsetAsync(t->d_state, 0, sizeof(ChanState) * (size_t)t->nchan, st));
    PIRIP_HIPCHK(hipMemsetAsync(t->d_sy, kOff, rows, st));
    PIRIP_HIPCHK(hipMemsetAsync(t->d_pre, 0, sizeof(uint32_t) * rows, st));
    t->calls = 0;
    return PIRIP_OK;
}

int txs_alloc(pirip_hip_txs *t)
{
    const size_t K = (size_t)t->nchan, rows = 2 * K * t->row;
    DevMem &m = t->mem;
    PIRIP_TRY(m.alloc_filled(&t->d_ring, kOff, K * (size_t)t->queue_syms));
    PIRIP_TRY(m.alloc(&t->d_state, sizeof(ChanState) * K));
    PIRIP_TRY(m.alloc(&t->d_sy, rows));
    PIRIP_TRY(m.alloc(&t->d_pre, sizeof(uint32_t) * rows));
    PIRIP_TRY(m.alloc_filled(&t->d_no_lead, 0, sizeof(int32_t) * K));
    PIRIP_TRY(m.alloc(&t->d_nsym, sizeof(int32_t) * K));
    PIRIP_TRY(txs_clear(t, nullptr));
    PIRIP_HIPCHK(hipDeviceSynchronize());
    return PIRIP_OK;
}

}  // namespace

// the framer's rows of a send of max_rec records per channel (rows of a call larger than any before it: calls in flight may still use
// the ones they replace); the handle's device is current
int pirip::txs_reserve(pirip_hip_txs *t, int max_rec)
{
    int64_t cap = tx_row_syms(t->tx, max_rec, 0);
    if (cap < 1) cap = 1;
    if ((size_t)cap > t->frm_cap)
        PIRIP_TRY(grow_dev(t->mem, &t->frm_cap, (size_t)cap, t->d_frm ? GrowSync::device : GrowSync::none, nullptr,
                           {grow_buf(&t->d_frm, (size_t)t->nchan * (size_t)cap)}));
    if ((size_t)max_rec > t->off_cap)
        PIRIP_TRY(grow_dev(t->mem, &t->off_cap, (size_t)max_rec, t->d_off ? GrowSync::device : GrowSync::none, nullptr,
                           {grow_buf(&t->d_off, sizeof(int32_t) * (size_t)t->nchan * (size_t)max_rec)}));
    return PIRIP_OK;
}

extern "C" {

int pirip_hip_txs_create(pirip_hip_tx *tx, pirip_hip_mux *mux, int64_t block, int64_t queue_syms, pirip_hip_txs **out)
{
    if (!out) return PIRIP_ERR_BAD_ARG;
    *out = nullptr;
    if (!tx || !mux || block <= 0) return PIRIP_ERR_BAD_ARG;
    if (tx->nstreams != mux->nchan || (int64_t)tx->Fs * mux->D != mux->Fs || tx->device != mux->device) return PIRIP_ERR_BAD_ARG;
    const int64_t per_sym = (int64_t)mux->D * tx->Ts;
    if (block % per_sym) return PIRIP_ERR_BAD_ARG;
    const int64_t S = block / per_sym, H = ((int64_t)mux->Q - 1 + tx->Ts - 1) / tx->Ts;
    if (queue_syms < S) return PIRIP_ERR_BAD_ARG;
    // the staging cursor counts row samples in an int: it starts at most at (H + S) Ts and moves on over a tile's span of at most
    // kMuxTile + Q inputs, one step of kMuxThreads past it
    if ((H + S) * tx->Ts > (int64_t)0x7fffffff - kMuxTile - mux->Q - kMuxThreads || (block + kMuxTile - 1) / kMuxTile > 0x7fffffff) return PIRIP_ERR_UNSUPPORTED;
    if (!bind_device(tx->device)) return PIRIP_ERR_NO_DEVICE;
    pirip_hip_txs *t = new (std::nothrow) pirip_hip_txs();
    if (!t) return PIRIP_ERR_NOMEM;
    t->tx = tx; t->mux = mux; t->nchan = tx->nstreams; t->device = tx->device;
    t->S = (int)S; t->H = (int)H; t->row = (size_t)(H + S); t->block = block; t->queue_syms = queue_syms;
    const int rc = txs_alloc(t);
    if (rc != PIRIP_OK) { delete t; return rc; }
    *out = t;
    return PIRIP_OK;
}

int pirip_hip_txs_destroy(pirip_hip_txs *t) { return destroy_handle(t, t ? t->device : 0); }

int pirip_hip_txs_get_info(const pirip_hip_txs *t, pirip_txs_info *info)
{
    if (!t || !info) return PIRIP_ERR_BAD_ARG;
    *info = pirip_txs_info{t->block, t->queue_syms, t->S, t->H, t->nchan, t->mux->noutputs, t->mux->out_format, t->device};
    return PIRIP_OK;
}

int pirip_hip_txs_send(pirip_hip_txs *t, const uint8_t *d_records, size_t rec_stride, const int32_t *d_nrec, int max_rec, int32_t *d_taken,
                       void *hip_stream)
{
    if (!t || !d_records || max_rec < 0) return PIRIP_ERR_BAD_ARG;
    pirip_hip_tx *tx = t->tx;
    int64_t cap = tx_row_syms(tx, max_rec, 0);
    if (cap < 1) cap = 1;
    PIRIP_TRY(tx_frame_check(tx, rec_stride, max_rec, (size_t)cap, cap, false, 0));
    if (!bind_device(t->device)) return PIRIP_ERR_NO_DEVICE;
    PIRIP_TRY(txs_reserve(t, max_rec));
    hipStream_t st = (hipStream_t)hip_stream;
    PIRIP_TRY(tx_frame_rows(tx, d_records, rec_stride, d_nrec, max_rec, t->d_frm, t->frm_cap, cap, t->d_nsym, nullptr, 0, t->d_no_lead, t->d_off, st));
    const AppendArgs a{t->d_frm, t->frm_cap, t->d_nsym, d_nrec, max_rec, t->d_ring, t->queue_syms, t->d_state, d_taken};
    hipLaunchKernelGGL(txs_append_kernel, dim3((unsigned)t->nchan), dim3(kAppendThreads), 0, st, a);
    PIRIP_HIPCHK(hipGetLastError());
    return PIRIP_OK;
}

int pirip_hip_txs_process(pirip_hip_txs *t, void *d_out, size_t out_stride_bytes, int32_t *d_sent, void *hip_stream)
{
    if (!t || !d_out) return PIRIP_ERR_BAD_ARG;
    const pirip_hip_tx *tx = t->tx;
    const pirip_hip_mux *mx = t->mux;
    PIRIP_TRY(iq_rows_check(d_out, out_stride_bytes, mx->bs, mx->noutputs, t->block));
    if (!bind_device(t->device)) return PIRIP_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t half = (size_t)t->nchan * t->row, cur = (size_t)(t->calls & 1) * half, prev = half - cur;
    const TakeArgs ta{t->d_ring, t->queue_syms, t->d_state, t->d_sy + prev, t->d_sy + cur, t->d_pre + prev, t->d_pre + cur, t->row,
                      t->H, t->S, tx->M, tx->Fs, tx->d_tm, d_sent};
    hipLaunchKernelGGL(txs_take_kernel, dim3((unsigned)t->nchan), dim3(kScanThreads), 0, st, ta);
    // the block as pirip_hip_mux_batch would make it of block / D + Q - 1 modem samples, the first Q - 1 of them the previous call's
    MuxArgs a{};
    mux_fill_args(mx, t->block, t->calls * (t->block / mx->D) - (mx->Q - 1), d_out, out_stride_bytes, &a);
    SymStage sg{};
    sg.sy = t->d_sy + cur; sg.pre = t->d_pre + cur; sg.row = t->row; sg.fm = tx->d_fm;
    sg.Ts = tx->Ts; sg.M = tx->M; sg.Fs = tx->Fs; sg.nrow = (int)t->row;
    sg.e0 = t->H * tx->Ts - (mx->Q - 1);
    sg.step_i = kMuxThreads / tx->Ts; sg.step_r = kMuxThreads % tx->Ts;
    sg.two_over_fs = 2.0f / (float)tx->Fs; sg.inv_fs_d = 1.0 / (double)tx->Fs;
    const dim3 grid((unsigned)((t->block + kMuxTile - 1) / kMuxTile), (unsigned)mx->noutputs);
    if (mx->bs == 2) hipLaunchKernelGGL(txs_mux_kernel<2>, grid, dim3(kMuxThreads), mx->lds, st, a, sg);
    else hipLaunchKernelGGL(txs_mux_kernel<8>, grid, dim3(kMuxThreads), mx->lds, st, a, sg);
    PIRIP_HIPCHK(hipGetLastError());
    t->calls++;
    return PIRIP_OK;
}

int pirip_hip_txs_get_counters(pirip_hip_txs *t, int64_t *queued, int64_t *sent, int64_t *underrun, int64_t *refused)
{
    if (!t) return PIRIP_ERR_BAD_ARG;
    std::vector<ChanState> cs((size_t)t->nchan);
    PIRIP_TRY(read_back(t->device, t->d_state, cs));
    for (size_t c = 0; c < cs.size(); c++) {
        if (queued) queued[c] = (int64_t)(cs[c].tail - cs[c].head);
        if (sent) sent[c] = cs[c].sent;
        if (underrun) underrun[c] = cs[c].underrun;
        if (refused) refused[c] = cs[c].refused;
    }
    return PIRIP_OK;
}

int pirip_hip_txs_reset(pirip_hip_txs *t, void *hip_stream)
{
    if (!t) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(t->device)) return PIRIP_ERR_NO_DEVICE;
    return txs_clear(t, (hipStream_t)hip_stream);
}

}  // extern "C"
