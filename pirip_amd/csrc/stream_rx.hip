// pirip_amd/csrc/stream_rx.hip -- include/pirip_hip.h section G: the streaming receiver.
// N live channels, one block per channel per call, on the handles the caller already has (demodulator, optionally the FSK_LDPC
// receivers and the csdr front end). Each channel's unconsumed tail stays where it is on the device: the advance kernel moves it,
// right-aligned, in front of the landing zone of the next block and writes the segment descriptor (SegDesc, fsk_device.hpp) the next
// call's demodulator starts the channel at. No host round trip, no repacking, and fewer than nin_max samples carried per channel.
//
// Modem-rate staging row of a channel:  [C_pre | m]   (C_pre >= nin_max, C_pre * bytes per sample a multiple of 256)
//   the carried tail of L_s samples at [C_pre - L_s, C_pre), the call's m new samples at C_pre (the same m for every channel).
// With a decimator, a tuner-rate row per channel:  [Hpad | block]   (Hpad = H u8 samples rounded up to 256 bytes)
//   the decimator's history of H samples (the same H for every channel and every call: block % D == 0) right-aligned in front of the
//   block; the decimator writes straight into the modem rows at C_pre through its output stride.
// With a channelizer (section H), the same tuner-rate rows, one per wideband INPUT instead of one per channel; the channelizer writes
// every channel of an input into that channel's modem row at C_pre, and the absolute index of each call's first input sample (t0) is
// tracked here on the host: it only depends on the number of calls.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "../../include/pirip_hip.h"
#include "fsk_device.hpp"
#include "demod_handle.hpp"
#include "rate_host.hpp"
#include "rpt_handle.hpp"

using namespace pirip;

namespace {

constexpr int kWave = 64;
constexpr int kChannelsPerBlock = 4;       // one wave per channel

struct AdvanceArgs {
    uint8_t *rows; size_t row_bytes;       // modem-rate staging rows
    int bps;                               // bytes per modem-rate sample
    int64_t c_pre, m;                      // landing zone, new samples of this call
    int32_t nin_max, budget;
    const int64_t *consumed;               // [s] what the demodulator consumed in this call (from row + C_pre - L_s)
    int32_t *carry;                        // [s] L_s in, L'_s out (the backlog)
    int64_t *total;                        // [s] consumed since create / reset
    SegDesc *seg;                          // [s] the next call's descriptor
    int32_t *flag;                         // raised when a carry reaches nin_max
    int nstreams;
};

// n units of T from src to dst (both T-aligned), lane-strided; the ranges do not overlap
template <typename T>
__device__ __forceinline__ void copy_units(uint8_t *dst, const uint8_t *src, size_t n, int lane)
{
    for (size_t i = lane; i < n; i += kWave) ((T *)dst)[i] = ((const T *)src)[i];
}

// The carried tail [C_pre + m - L', C_pre + m) -> [C_pre - L', C_pre). Source and destination are m samples apart and m >= nin_max > L'
// (create enforces the first, the frame budget the second): the ranges never overlap, so every lane copies its own units with no order
// among them. 16-byte units where the distance allows (it fixes the alignment of one end relative to the other), byte-exact edges.
__device__ __forceinline__ void move_tail(uint8_t *row, size_t d0, size_t s0, size_t len, int lane)
{
    const size_t dist = s0 - d0;
    const int g = (dist & 15) == 0 ? 16 : (dist & 7) == 0 ? 8 : (dist & 3) == 0 ? 4 : (dist & 1) == 0 ? 2 : 1;
    size_t head = (g - (d0 & (g - 1))) & (g - 1);
    if (head > len) head = len;
    const size_t body = (len - head) / g, tail0 = head + body * g;
    if (lane < (int)head) row[d0 + lane] = row[s0 + lane];
    uint8_t *dst = row + d0 + head;
    const uint8_t *src = row + s0 + head;
    switch (g) {                                           // (wave-uniform)
    case 16: copy_units<uint4>(dst, src, body, lane); break;
    case 8: copy_units<uint2>(dst, src, body, lane); break;
    case 4: copy_units<uint32_t>(dst, src, body, lane); break;
    case 2: copy_units<uint16_t>(dst, src, body, lane); break;
    default: copy_units<uint8_t>(dst, src, body, lane); break;
    }
    if (tail0 + lane < len) row[d0 + tail0 + lane] = row[s0 + tail0 + lane];   // (< 16 bytes)
}

__global__ __launch_bounds__(kWave * kChannelsPerBlock) void rx_advance_kernel(AdvanceArgs a)
{
    const int lane = threadIdx.x % kWave;
    const int s = blockIdx.x * kChannelsPerBlock + threadIdx.x / kWave;
    if (s >= a.nstreams) return;
    const int64_t cons = a.consumed[s];
    int64_t carry = (int64_t)a.carry[s] + a.m - cons;
    bool bad = false;
    if (carry < 0 || carry >= a.nin_max) { bad = true; carry = 0; }     // (cannot happen with the budget's rows: reported, the carry dropped)
    uint8_t *row = a.rows + (size_t)s * a.row_bytes;
    const size_t d0 = (size_t)(a.c_pre - carry) * a.bps, s0 = (size_t)(a.c_pre + a.m - carry) * a.bps;
    move_tail(row, d0, s0, (size_t)carry * a.bps, lane);
    if (lane == 0) {
        if (bad) *a.flag = 1;
        a.carry[s] = (int32_t)carry;
        a.total[s] += cons;
        a.seg[s] = SegDesc{a.c_pre - carry, 0, a.budget, 0};
    }
}

inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

}  // namespace

// (hidden: a handle's implicit destructor is no dynamic symbol of the library)
#pragma GCC visibility push(hidden)
struct pirip_hip_rx {
    pirip_hip_demod *dem = nullptr;
    pirip_hip_ldpc *ldpc = nullptr;
    pirip_hip_decim *dec = nullptr;
    pirip_hip_chan *chan = nullptr;
    int nstreams = 0, bps = 0, nin_max = 0;
    int nraw = 0;                          // tuner-rate rows: nstreams with a decimator, the channelizer's inputs with a channelizer
    int64_t t_in = 0;                      // channelizer: input samples per input before this call's block
    int64_t block = 0;                     // input samples per channel per call
    int64_t m = 0, m_first = 0;            // modem-rate samples per call (the first call after create / reset: m_first)
    int64_t c_pre = 0, budget = 0;
    size_t row_bytes = 0;
    int D = 1;
    int64_t H = 0;                         // decimator history (u8 samples)
    size_t raw_pre = 0, raw_row_bytes = 0; // tuner-rate rows: block at raw_pre bytes
    DevMem mem;
    uint8_t *d_rows = nullptr, *d_raw = nullptr;
    int64_t *d_consumed = nullptr, *d_total = nullptr;
    int32_t *d_carry = nullptr, *d_flag = nullptr;
    SegDesc *d_seg = nullptr;
    bool first = true;                     // the next call runs without descriptors (every carry is 0)
};
#pragma GCC visibility pop

namespace {

int rx_clear(pirip_hip_rx *rx, hipStream_t st)
{
    const size_t ns = (size_t)rx->nstreams;
    PIRIP_HIPCHK(hipMemsetAsync(rx->d_carry, 0, sizeof(int32_t) * ns, st));
    PIRIP_HIPCHK(hipMemsetAsync(rx->d_total, 0, sizeof(int64_t) * ns, st));
    PIRIP_HIPCHK(hipMemsetAsync(rx->d_flag, 0, sizeof(int32_t), st));
    rx->first = true;
    rx->t_in = 0;
    return PIRIP_OK;
}

int rx_run(pirip_hip_rx *rx, uint8_t *d_bits, size_t bits_stride, float *d_rx_filt, size_t filt_stride, uint8_t *d_status, uint8_t *d_payload,
           int32_t *d_info, float *d_stats, size_t stats_stride, int32_t *d_nframes, hipStream_t st)
{
    if (rx->ldpc ? (d_bits || d_rx_filt || !d_status || !d_payload || !d_info || !d_nframes) : (d_status || d_payload || d_info)) return PIRIP_ERR_BAD_ARG;
    if (!demod_bind(rx->dem)) return PIRIP_ERR_NO_DEVICE;
    const int64_t mc = rx->first ? rx->m_first : rx->m;
    uint8_t *land = rx->d_rows + (size_t)rx->c_pre * rx->bps;
    // 1. front end: decimate into the modem rows at C_pre, then keep the last H tuner-rate samples in front of the next block
    if (rx->dec || rx->chan) {
        const uint8_t *in = rx->d_raw + rx->raw_pre - (rx->first ? 0 : (size_t)rx->H * 2);
        const int64_t n_in = rx->block + (rx->first ? 0 : rx->H);
        int rc = rx->dec ? pirip_hip_decim_batch(rx->dec, in, rx->raw_row_bytes, n_in, land, rx->row_bytes, rx->nstreams, st)
                         : pirip_hip_chan_batch(rx->chan, in, rx->raw_row_bytes, n_in, rx->first ? 0 : rx->t_in - rx->H, land, rx->row_bytes, st);
        if (rc != PIRIP_OK) return rc;
        if (rx->H > 0) PIRIP_HIPCHK(hipMemcpy2DAsync(rx->d_raw + rx->raw_pre - (size_t)rx->H * 2, rx->raw_row_bytes,
                                                     rx->d_raw + rx->raw_pre + (size_t)(rx->block - rx->H) * 2, rx->raw_row_bytes,
                                                     (size_t)rx->H * 2, (size_t)rx->nraw, hipMemcpyDeviceToDevice, st));
    }
    // 2. demodulator (or the FSK_LDPC chain): the first call on row + C_pre without descriptors -- the exact-first-frame prologue then
    //    applies as in pirip_hip_demod_batch --, every later one from each channel's carried tail
    const void *in = rx->first ? (const void *)land : (const void *)rx->d_rows;
    const int64_t nsamp = rx->first ? mc : rx->c_pre + mc;
    const SegDesc *seg = rx->first ? nullptr : rx->d_seg;
    int rc = rx->ldpc ? fsk_ldpc_rx_batch_seg(rx->dem, rx->ldpc, in, rx->row_bytes, nsamp, d_status, d_payload, d_info, d_stats, stats_stride,
                                              d_nframes, rx->d_consumed, rx->budget, seg, st)
                      : demod_batch_seg(rx->dem, in, rx->row_bytes, nsamp, d_bits, bits_stride, d_rx_filt, filt_stride, d_stats, stats_stride,
                                        d_nframes, rx->d_consumed, rx->budget, seg, st);
    if (rc != PIRIP_OK) return rc;
    // 3. carries and the next call's descriptors
    AdvanceArgs a{rx->d_rows, rx->row_bytes, rx->bps, rx->c_pre, mc, rx->nin_max, (int32_t)rx->budget, rx->d_consumed, rx->d_carry, rx->d_total,
                  rx->d_seg, rx->d_flag, rx->nstreams};
    hipLaunchKernelGGL(rx_advance_kernel, dim3((rx->nstreams + kChannelsPerBlock - 1) / kChannelsPerBlock), dim3(kWave * kChannelsPerBlock), 0, st, a);
    PIRIP_HIPCHK(hipGetLastError());
    rx->first = false;
    rx->t_in += rx->block;
    return PIRIP_OK;
}

// the rows and the per-channel bookkeeping of a new receiver, zeroed
int rx_alloc(pirip_hip_rx *rx)
{
    const size_t ns = (size_t)rx->nstreams, raw_bytes = rx->raw_row_bytes * (size_t)rx->nraw;
    DevMem &m = rx->mem;
    // (rows start zeroed: nothing reads bytes the caller or the decimator did not write, but a fresh buffer is not left to chance)
    PIRIP_TRY(m.alloc_filled(&rx->d_rows, 0, rx->row_bytes * ns));
    if (raw_bytes) PIRIP_TRY(m.alloc_filled(&rx->d_raw, 0, raw_bytes));
    PIRIP_TRY(m.alloc(&rx->d_consumed, sizeof(int64_t) * ns));
    PIRIP_TRY(m.alloc(&rx->d_total, sizeof(int64_t) * ns));
    PIRIP_TRY(m.alloc(&rx->d_carry, sizeof(int32_t) * ns));
    PIRIP_TRY(m.alloc(&rx->d_flag, sizeof(int32_t)));
    PIRIP_TRY(m.alloc_filled(&rx->d_seg, 0, sizeof(SegDesc) * ns));
    PIRIP_TRY(rx_clear(rx, nullptr));
    PIRIP_HIPCHK(hipDeviceSynchronize());
    return PIRIP_OK;
}

int rx_create_impl(pirip_hip_demod *dem, pirip_hip_ldpc *ldpc, pirip_hip_decim *dec, pirip_hip_chan *chan, int64_t block, pirip_hip_rx **out)
{
    if (!out) return PIRIP_ERR_BAD_ARG;
    *out = nullptr;
    if (!dem || block <= 0) return PIRIP_ERR_BAD_ARG;
    if (!demod_bind(dem)) return PIRIP_ERR_NO_DEVICE;
    const FskDims &d = dem->plan.d;
    if (ldpc) {
        int M = 0, Nsym = 0, ns = 0, dev = 0;
        if (ldpc_handle_shape(ldpc, &M, &Nsym, &ns, &dev) != PIRIP_OK) return PIRIP_ERR_BAD_ARG;
        if (M != d.M || Nsym != d.Nsym || ns != dem->nstreams || dev != dem->device) return PIRIP_ERR_BAD_ARG;
    }
    int Lp = 0, D = 1, out_s16 = 0, nraw = dem->nstreams;
    if (dec) {
        if (d.in_format != PIRIP_IN_CF32 && d.in_format != PIRIP_IN_CS16) return PIRIP_ERR_BAD_ARG;
        decim_handle_shape(dec, &Lp, &D, &out_s16);
        if (out_s16 != (d.in_format == PIRIP_IN_CS16)) return PIRIP_ERR_BAD_ARG;
        if (block % D != 0) return PIRIP_ERR_BAD_ARG;
    }
    if (chan) {
        pirip_chan_info ci{};
        if (d.in_format != PIRIP_IN_CF32 && d.in_format != PIRIP_IN_CS16) return PIRIP_ERR_BAD_ARG;
        if (pirip_hip_chan_get_info(chan, &ci) != PIRIP_OK) return PIRIP_ERR_BAD_ARG;
        if (ci.out_s16 != (d.in_format == PIRIP_IN_CS16) || ci.nchan != dem->nstreams || ci.device != dem->device) return PIRIP_ERR_BAD_ARG;
        D = ci.D; Lp = ci.ntaps_padded; nraw = ci.ninputs;
        if (block % D != 0) return PIRIP_ERR_BAD_ARG;
    }
    auto fe_nout = [&](int64_t n) { return dec ? pirip_hip_decim_nout(dec, n) : pirip_hip_chan_nout(chan, n); };
    pirip_hip_rx *rx = new (std::nothrow) pirip_hip_rx();
    if (!rx) return PIRIP_ERR_NOMEM;
    rx->dem = dem; rx->ldpc = ldpc; rx->dec = dec; rx->chan = chan; rx->block = block; rx->D = D;
    rx->nstreams = dem->nstreams;
    rx->nraw = nraw;
    rx->bps = bytes_per_sample(d.in_format);
    rx->nin_max = d.N + d.nin_step;
    const int nin_min = 2 * d.N - rx->nin_max;
    rx->m = block / D;
    rx->m_first = rx->m;
    if (dec || chan) {
        // the first call's D-spaced outputs stop where the filter runs out of input; from then on the leftover H is the same every call
        rx->m_first = fe_nout(block);
        rx->H = block - rx->m_first * D;
        if (rx->H < 0 || rx->H > block || fe_nout(block + rx->H) != rx->m) { delete rx; return PIRIP_ERR_BAD_ARG; }
    }
    // every call hands the demodulator at least nin_max new samples: the carry (< nin_max) is then never overwritten by its own move
    if (rx->m_first < rx->nin_max || nin_min <= 0) { delete rx; return PIRIP_ERR_BAD_ARG; }
    rx->c_pre = (int64_t)(round_up((size_t)rx->nin_max * rx->bps, 256) / rx->bps);
    rx->budget = (rx->nin_max - 1 + rx->m) / nin_min + 1;     // (the shortest frames from the longest carry: binding.py's rule)
    if (dem->kernel == PIRIP_KERNEL_WAVE && rx->c_pre + rx->m > demod_wave_max_samples(d)) { delete rx; return PIRIP_ERR_UNSUPPORTED; }
    if (rx->budget > (1 << 24)) { delete rx; return PIRIP_ERR_UNSUPPORTED; }
    rx->row_bytes = round_up((size_t)(rx->c_pre + rx->m) * rx->bps, 256);
    if (dec || chan) {
        rx->raw_pre = round_up((size_t)rx->H * 2, 256);
        rx->raw_row_bytes = round_up(rx->raw_pre + (size_t)block * 2, 256);
    }
    int rc = rx_alloc(rx);
    // the FSK_LDPC receiver grows its work rows with the largest call it has seen: every call of this receiver has the same size, known now
    if (rc == PIRIP_OK && ldpc) rc = ldpc_reserve(dem, ldpc, rx->c_pre + rx->m, rx->budget);
    if (rc != PIRIP_OK) { delete rx; return rc; }
    *out = rx;
    return PIRIP_OK;
}

}  // namespace

// what the streaming repeater (rpt_kernels.hip) asks of a receiver it borrows
void pirip::rx_handle_shape(const pirip_hip_rx *rx, int *nstreams, const pirip_hip_ldpc **ldpc, int *device)
{
    *nstreams = rx->nstreams; *ldpc = rx->ldpc; *device = rx->dem->device;
}

// ... and the ping terminal (ping_kernels.hip): what the first demodulator call consumes
int pirip::rx_handle_nin0(const pirip_hip_rx *rx) { return rx->dem->plan.d.N; }

extern "C" {

int pirip_hip_rx_create(pirip_hip_demod *dem, pirip_hip_ldpc *ldpc, pirip_hip_decim *dec, int64_t block, pirip_hip_rx **out)
{
    return rx_create_impl(dem, ldpc, dec, nullptr, block, out);
}

int pirip_hip_rx_create_chan(pirip_hip_demod *dem, pirip_hip_ldpc *ldpc, pirip_hip_chan *chan, int64_t block, pirip_hip_rx **out)
{
    if (!chan) { if (out) *out = nullptr; return PIRIP_ERR_BAD_ARG; }
    return rx_create_impl(dem, ldpc, nullptr, chan, block, out);
}

int pirip_hip_rx_destroy(pirip_hip_rx *rx) { return destroy_handle(rx, rx ? rx->dem->device : 0); }

int64_t pirip_hip_rx_max_frames(const pirip_hip_rx *rx) { return rx ? rx->budget : PIRIP_ERR_BAD_ARG; }

int pirip_hip_rx_input(pirip_hip_rx *rx, void **d_block, size_t *stride_bytes)
{
    if (!rx || !d_block || !stride_bytes) return PIRIP_ERR_BAD_ARG;
    if (rx->dec || rx->chan) { *d_block = rx->d_raw + rx->raw_pre; *stride_bytes = rx->raw_row_bytes; }
    else { *d_block = rx->d_rows + (size_t)rx->c_pre * rx->bps; *stride_bytes = rx->row_bytes; }
    return PIRIP_OK;
}

int pirip_hip_rx_process(pirip_hip_rx *rx, uint8_t *d_bits, size_t bits_stride, float *d_rx_filt, size_t filt_stride,
                         uint8_t *d_status, uint8_t *d_payload, int32_t *d_info, float *d_stats, size_t stats_stride,
                         int32_t *d_nframes, void *hip_stream)
{
    if (!rx) return PIRIP_ERR_BAD_ARG;
    return rx_run(rx, d_bits, bits_stride, d_rx_filt, filt_stride, d_status, d_payload, d_info, d_stats, stats_stride, d_nframes, (hipStream_t)hip_stream);
}

int pirip_hip_rx_push(pirip_hip_rx *rx, const void *d_in, size_t in_stride_bytes,
                      uint8_t *d_bits, size_t bits_stride, float *d_rx_filt, size_t filt_stride,
                      uint8_t *d_status, uint8_t *d_payload, int32_t *d_info, float *d_stats, size_t stats_stride,
                      int32_t *d_nframes, void *hip_stream)
{
    if (!rx || !d_in) return PIRIP_ERR_BAD_ARG;
    if (!demod_bind(rx->dem)) return PIRIP_ERR_NO_DEVICE;
    void *dst = nullptr; size_t dpitch = 0;
    (void)pirip_hip_rx_input(rx, &dst, &dpitch);
    const size_t width = (size_t)rx->block * (rx->dec || rx->chan ? 2 : rx->bps);
    const int rows = rx->chan ? rx->nraw : rx->nstreams;
    if (in_stride_bytes < width && rows > 1) return PIRIP_ERR_BAD_ARG;
    PIRIP_HIPCHK(hipMemcpy2DAsync(dst, dpitch, d_in, in_stride_bytes ? in_stride_bytes : width, width, (size_t)rows, hipMemcpyDeviceToDevice,
                                  (hipStream_t)hip_stream));
    return rx_run(rx, d_bits, bits_stride, d_rx_filt, filt_stride, d_status, d_payload, d_info, d_stats, stats_stride, d_nframes, (hipStream_t)hip_stream);
}

int pirip_hip_rx_get_counters(pirip_hip_rx *rx, int64_t *consumed_total, int32_t *backlog)
{
    if (!rx) return PIRIP_ERR_BAD_ARG;
    if (!demod_bind(rx->dem)) return PIRIP_ERR_NO_DEVICE;
    const size_t ns = (size_t)rx->nstreams;
    int32_t flag = 0;
    PIRIP_HIPCHK(hipDeviceSynchronize());
    if (consumed_total) PIRIP_HIPCHK(hipMemcpy(consumed_total, rx->d_total, sizeof(int64_t) * ns, hipMemcpyDeviceToHost));
    if (backlog) PIRIP_HIPCHK(hipMemcpy(backlog, rx->d_carry, sizeof(int32_t) * ns, hipMemcpyDeviceToHost));
    PIRIP_HIPCHK(hipMemcpy(&flag, rx->d_flag, sizeof(flag), hipMemcpyDeviceToHost));
    return flag ? PIRIP_ERR_HIP : PIRIP_OK;
}

int pirip_hip_rx_reset(pirip_hip_rx *rx, void *hip_stream)
{
    if (!rx) return PIRIP_ERR_BAD_ARG;
    if (!demod_bind(rx->dem)) return PIRIP_ERR_NO_DEVICE;
    int rc = pirip_hip_reset(rx->dem, hip_stream);
    if (rc == PIRIP_OK && rx->ldpc) rc = pirip_hip_ldpc_reset(rx->ldpc, hip_stream);
    if (rc == PIRIP_OK) rc = rx_clear(rx, (hipStream_t)hip_stream);
    return rc;
}

}  // extern "C"
