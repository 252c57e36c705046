// pirip_amd/csrc/testbits_kernels.hip -- include/pirip_hip.h section L: the test-frame counter. fsk_put_test_bits
// (pirip::PutBits, fsk_plan.cpp) and the ecdd tally of rtl_fsk --code --testframes for a batch of streams, on the device.
//
// Uncoded. A stream's bits of one call are t = 0 .. L - 1 (L = rows * row_bits), the F - 1 bits before them t = -(F - 1) .. -1. Position t
// compares the window [t - F + 1, t] with the frame; every position is independent and every sum is an integer, so the grid is
// (stream, tile of kTile positions) in any order. One wave per workgroup:
//   stage    [history | tile] as packed words in LDS, stream bit t at bit (t mod 32) of its word (LSB first): 64 bits per step, one
//            lane per bit (a byte, or a bit of an MSB-first packed row, or a bit of the carried history) and one ballot
//   count    lane l owns positions T0 + 32 l .. + 31. Frame word w (frame bit k at bit k mod 32 of word k div 32) faces the 63 stream
//            bits from p0 - (F - 1) + 32 w on: one more LDS word per w, one funnel shift to align them, and per position one funnel
//            shift, XOR, AND (the last word's mask) and a population count into that position's sum
//   reduce   within the wave, then lane 0 adds packets, bits, errors (and, tile 0, the bits pushed) with one 64-bit atomic each
//   carry    the workgroup of a stream's last tile writes the next call's history -- the last 32 HW bits (HW = ceil((F - 1) / 32) words)
//            up to t = L - 1 -- into the OTHER of the handle's two history rows: a launch reads one row and writes the other.
// Coded. One wave per stream, one lane per record: info[6] >= 0 counts, popcount of payload ^ test payload over bytes 2 .. data_bytes - 3.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/pirip_hip.h"
#include "fsk_ldpc.hpp"
#include "fsk_plan.hpp"
#include "hip_host.hpp"
#include "rows_device.hpp"

using namespace pirip;

namespace {

constexpr int kTile = 2048;                                    // positions per workgroup: 32 per lane
constexpr int kLanes = 64;
constexpr int kMaxHW = (PIRIP_TBITS_MAX_FRAMESIZE - 1 + 31) / 32;          // 128 history words
constexpr int kLdsWords = kMaxHW + kTile / 32 + 2;             // the count loop reads two words past the tile (shifted out or masked)
constexpr int kCnt = 4, kRecCnt = 5;

typedef unsigned long long u64;

struct PushArgs {
    const uint8_t *bits; size_t stride;
    uint32_t row_bits, row_pitch; int packed;
    const int32_t *nframes; uint32_t max_frames;
    const uint32_t *frame;                                     // [W] packed frame
    int F, W, HW; uint32_t last_mask; float thr;
    const uint32_t *hist_prev; uint32_t *hist_cur; size_t hist_row;        // [nstreams][hist_row]
    u64 *cnt;                                                  // [nstreams][kCnt]
    uint32_t ntiles;
};

__global__ __launch_bounds__(kLanes) void tbits_count_kernel(PushArgs a)
{
    __shared__ uint32_t sw[kLdsWords];
    const uint32_t s = blockIdx.x / a.ntiles, tile = blockIdx.x - s * a.ntiles;
    const int lane = threadIdx.x;
    const uint32_t L = (uint32_t)row_count(a.nframes, s, (int)a.max_frames) * a.row_bits;      // < 2^31
    const uint32_t my_tiles = L ? (L + kTile - 1) / kTile : 1;  // (a stream without rows still moves its history to the other row)
    if (tile >= my_tiles) return;
    const uint32_t T0 = tile * kTile;
    const int64_t t_first = (int64_t)T0 - 32 * a.HW;           // stream bit of LDS bit 0
    const uint8_t *in = a.bits + (size_t)s * a.stride;
    const uint32_t *hist = a.hist_prev + (size_t)s * a.hist_row;

    const int nw = a.HW + kTile / 32 + 2;
    for (int c = 0; 2 * c < nw; c++) {
        const int64_t t = t_first + 64 * c + lane;
        uint32_t bit = 0;
        if (t < 0) {
            const uint32_t ht = (uint32_t)(t + 32 * a.HW);     // 0 .. 32 HW - 1
            bit = hist[ht >> 5] >> (ht & 31);
        } else if (t < (int64_t)L) {
            const uint32_t u = (uint32_t)t;
            if (a.packed) {
                const uint32_t row = u / a.row_bits, col = u - row * a.row_bits;
                bit = in[(size_t)row * a.row_pitch + (col >> 3)] >> (7 - (col & 7));
            } else {
                bit = in[u];
            }
        }
        const u64 m = __ballot(bit & 1);
        if (lane < 2 && 2 * c + lane < kLdsWords) sw[2 * c + lane] = lane ? (uint32_t)(m >> 32) : (uint32_t)m;
    }
    __syncthreads();

    const uint32_t p0 = T0 + 32 * (uint32_t)lane;
    int pk = 0, er = 0;
    if (p0 < L) {
        const int sh0 = 32 * a.HW - (a.F - 1);                 // 0 .. 31: LDS bit of p0 - (F - 1) inside word `lane`
        int errs[32];
#pragma unroll
        for (int i = 0; i < 32; i++) errs[i] = 0;
        uint32_t x1 = sw[lane + 1];
        uint32_t lo = __funnelshift_r(sw[lane], x1, sh0);
        for (int w = 0; w < a.W; w++) {
            const uint32_t x2 = sw[lane + w + 2];
            const uint32_t hi = __funnelshift_r(x1, x2, sh0);
            const uint32_t fr = a.frame[w], mk = w == a.W - 1 ? a.last_mask : 0xffffffffu;
#pragma unroll
            for (int i = 0; i < 32; i++) errs[i] += __popc((__funnelshift_r(lo, hi, i) ^ fr) & mk);
            lo = hi; x1 = x2;
        }
#pragma unroll
        for (int i = 0; i < 32; i++) {
            const bool valid = p0 + i < L && (float)errs[i] < a.thr;
            pk += valid;
            er += valid ? errs[i] : 0;
        }
    }
    pk = wave_sum(pk);
    er = wave_sum(er);
    if (lane == 0) {
        u64 *cnt = a.cnt + (size_t)s * kCnt;
        if (pk) {
            atomicAdd(cnt + 0, (u64)pk);
            atomicAdd(cnt + 1, (u64)pk * (u64)a.F);
            atomicAdd(cnt + 2, (u64)er);
        }
        if (tile == 0 && L) atomicAdd(cnt + 3, (u64)L);
    }

    if (tile == my_tiles - 1) {
        uint32_t *out = a.hist_cur + (size_t)s * a.hist_row;
        for (int q = lane; q < a.HW; q += kLanes) {
            const uint32_t o = L - T0 + 32 * (uint32_t)q;      // LDS bit of stream bit L - 32 HW + 32 q: at most kTile + 32 (HW - 1)
            out[q] = __funnelshift_r(sw[o >> 5], sw[(o >> 5) + 1], o & 31);
        }
    }
}

struct RecArgs {
    const uint8_t *status; size_t status_stride;
    const uint8_t *payload; size_t payload_stride;
    const int32_t *info; size_t info_stride;
    const int32_t *ncalls; int max_calls;
    const uint8_t *want; int data_bytes;
    u64 *cnt;                                                  // [nstreams][kRecCnt]
};

__global__ __launch_bounds__(kLanes) void tbits_records_kernel(RecArgs a)
{
    const size_t s = blockIdx.x;
    const int lane = threadIdx.x;
    const int nc = row_count(a.ncalls, s, a.max_calls);
    int frames = 0, errors = 0, bad = 0, crc = 0;
    for (int r = lane; r < nc; r += kLanes) {
        crc += (a.status[s * a.status_stride + (size_t)r] & PIRIP_RX_BITS) != 0;
        if (a.info[s * a.info_stride + (size_t)r * PIRIP_LDPC_INFO_PER_CALL + 6] < 0) continue;
        const uint8_t *pl = a.payload + s * a.payload_stride + (size_t)r * (size_t)a.data_bytes;
        int e = 0;
        for (int b = 2; b < a.data_bytes - 2; b++) e += __popc((uint32_t)(pl[b] ^ a.want[b]));
        frames++; errors += e; bad += e > 0;
    }
    frames = wave_sum(frames); errors = wave_sum(errors); bad = wave_sum(bad); crc = wave_sum(crc);
    if (lane == 0) {
        u64 *cnt = a.cnt + s * kRecCnt;
        const int per = a.data_bytes > 4 ? 8 * (a.data_bytes - 4) : 0;
        if (frames) {
            atomicAdd(cnt + 0, (u64)frames);
            atomicAdd(cnt + 1, (u64)frames * (u64)per);
            atomicAdd(cnt + 2, (u64)errors);
            atomicAdd(cnt + 3, (u64)bad);
        }
        if (crc) atomicAdd(cnt + 4, (u64)crc);
    }
}

}  // namespace

// (hidden: a handle's implicit destructor is no dynamic symbol of the library)
#pragma GCC visibility push(hidden)
struct pirip_hip_tbits {
    int F = 0, W = 0, HW = 0, nstreams = 0, device = 0;
    uint32_t last_mask = 0;
    float thr = 0;                         // valid_thresh * framesize, in float
    int64_t calls = 0;                     // pushes since create / reset: call k reads history row (k + 1) & 1 and writes row k & 1
    size_t hist_row = 0;                   // words per stream: max(HW, 1)
    int data_bytes = 0;
    DevMem mem;
    uint32_t *d_frame = nullptr;           // [W]
    uint32_t *d_hist = nullptr;            // [2][nstreams][hist_row]
    u64 *d_cnt = nullptr;                  // [nstreams][kCnt]
    u64 *d_rcnt = nullptr;                 // [nstreams][kRecCnt]
    uint8_t *d_want = nullptr;             // [data_bytes] the payload records are compared with
};
#pragma GCC visibility pop

namespace {

int tbits_clear(pirip_hip_tbits *t, hipStream_t st)
{
    const size_t K = (size_t)t->nstreams;
    PIRIP_HIPCHK(hipMemsetAsync(t->d_hist, 0, sizeof(uint32_t) * 2 * K * t->hist_row, st));
    PIRIP_HIPCHK(hipMemsetAsync(t->d_cnt, 0, sizeof(u64) * K * kCnt, st));
    PIRIP_HIPCHK(hipMemsetAsync(t->d_rcnt, 0, sizeof(u64) * K * kRecCnt, st));
    t->calls = 0;
    return PIRIP_OK;
}

int tbits_alloc(pirip_hip_tbits *t, const std::vector<uint32_t> &frame)
{
    const size_t K = (size_t)t->nstreams;
    DevMem &m = t->mem;
    PIRIP_TRY(m.upload(&t->d_frame, frame.data(), sizeof(uint32_t) * frame.size()));
    PIRIP_TRY(m.alloc(&t->d_hist, sizeof(uint32_t) * 2 * K * t->hist_row));
    PIRIP_TRY(m.alloc(&t->d_cnt, sizeof(u64) * K * kCnt));
    PIRIP_TRY(m.alloc(&t->d_rcnt, sizeof(u64) * K * kRecCnt));
    PIRIP_TRY(tbits_clear(t, nullptr));
    PIRIP_HIPCHK(hipDeviceSynchronize());
    return PIRIP_OK;
}

// per-stream columns of a [nstreams][ncol] counter block into the host arrays that were asked for
int tbits_read(pirip_hip_tbits *t, const u64 *d_cnt, int ncol, int64_t *const *cols)
{
    std::vector<u64> c((size_t)t->nstreams * (size_t)ncol);
    PIRIP_TRY(read_back(t->device, d_cnt, c));
    for (int k = 0; k < ncol; k++)
        if (cols[k]) for (int s = 0; s < t->nstreams; s++) cols[k][s] = (int64_t)c[(size_t)s * (size_t)ncol + (size_t)k];
    return PIRIP_OK;
}

}  // namespace

extern "C" {

int pirip_hip_tbits_create(int framesize, float valid_thresh, const uint8_t *frame_bits, int nstreams, int device, pirip_hip_tbits **out)
{
    if (!out) return PIRIP_ERR_BAD_ARG;
    *out = nullptr;
    if (framesize < 1 || nstreams < 1) return PIRIP_ERR_BAD_ARG;
    if (framesize > PIRIP_TBITS_MAX_FRAMESIZE) return PIRIP_ERR_UNSUPPORTED;
    std::vector<uint8_t> fb((size_t)framesize);
    if (frame_bits) {
        for (int i = 0; i < framesize; i++) if (frame_bits[i] > 1) return PIRIP_ERR_BAD_ARG;
        std::memcpy(fb.data(), frame_bits, fb.size());
    } else {
        test_frame_bits(fb.data(), framesize);
    }
    int chosen = 0;
    PIRIP_TRY(select_device(device, &chosen));
    pirip_hip_tbits *t = new (std::nothrow) pirip_hip_tbits();
    if (!t) return PIRIP_ERR_NOMEM;
    t->F = framesize; t->W = (framesize + 31) / 32; t->HW = (framesize - 1 + 31) / 32;
    t->nstreams = nstreams; t->device = chosen;
    t->last_mask = framesize % 32 ? (1u << (framesize % 32)) - 1u : 0xffffffffu;
    t->thr = valid_thresh * framesize;                         // PutBits::push's expression, evaluated once
    t->hist_row = (size_t)(t->HW > 0 ? t->HW : 1);
    std::vector<uint32_t> frame((size_t)t->W, 0u);
    for (int i = 0; i < framesize; i++) frame[(size_t)(i >> 5)] |= (uint32_t)fb[(size_t)i] << (i & 31);
    const int rc = tbits_alloc(t, frame);
    if (rc != PIRIP_OK) { delete t; return rc; }
    *out = t;
    return PIRIP_OK;
}

int pirip_hip_tbits_destroy(pirip_hip_tbits *t) { return destroy_handle(t, t ? t->device : 0); }

int pirip_hip_tbits_push(pirip_hip_tbits *t, const uint8_t *d_bits, size_t bits_stride, int row_bits, int packed, const int32_t *d_nframes,
                         int64_t max_frames, void *hip_stream)
{
    if (!t || row_bits < 1 || max_frames < 0 || max_frames > 0x7fffffff || max_frames * (int64_t)row_bits >= ((int64_t)1 << 31)) return PIRIP_ERR_BAD_ARG;
    if (max_frames == 0) return PIRIP_OK;                      // no stream has a row: counters and history stay
    if (!d_bits) return PIRIP_ERR_BAD_ARG;
    const int64_t ntiles = (max_frames * row_bits + kTile - 1) / kTile;
    if (ntiles * t->nstreams > 0x7fffffff) return PIRIP_ERR_UNSUPPORTED;
    if (!bind_device(t->device)) return PIRIP_ERR_NO_DEVICE;
    const size_t half = (size_t)t->nstreams * t->hist_row, cur = (size_t)(t->calls & 1) * half, prev = half - cur;
    PushArgs a{};
    a.bits = d_bits; a.stride = bits_stride;
    a.row_bits = (uint32_t)row_bits; a.row_pitch = packed ? (uint32_t)((row_bits + 7) / 8) : (uint32_t)row_bits; a.packed = packed ? 1 : 0;
    a.nframes = d_nframes; a.max_frames = (uint32_t)max_frames;
    a.frame = t->d_frame; a.F = t->F; a.W = t->W; a.HW = t->HW; a.last_mask = t->last_mask; a.thr = t->thr;
    a.hist_prev = t->d_hist + prev; a.hist_cur = t->d_hist + cur; a.hist_row = t->hist_row;
    a.cnt = t->d_cnt; a.ntiles = (uint32_t)ntiles;
    hipLaunchKernelGGL(tbits_count_kernel, dim3((unsigned)(ntiles * t->nstreams)), dim3(kLanes), 0, (hipStream_t)hip_stream, a);
    PIRIP_HIPCHK(hipGetLastError());
    t->calls++;
    return PIRIP_OK;
}

int pirip_hip_tbits_get_counters(pirip_hip_tbits *t, int64_t *packets, int64_t *bits, int64_t *errors, int64_t *pushed)
{
    if (!t) return PIRIP_ERR_BAD_ARG;
    int64_t *const cols[kCnt] = {packets, bits, errors, pushed};
    return tbits_read(t, t->d_cnt, kCnt, cols);
}

int pirip_hip_tbits_counters_device(pirip_hip_tbits *t, int64_t **d_counters)
{
    if (!t || !d_counters) return PIRIP_ERR_BAD_ARG;
    *d_counters = (int64_t *)t->d_cnt;
    return PIRIP_OK;
}

int pirip_hip_tbits_reset(pirip_hip_tbits *t, void *hip_stream)
{
    if (!t) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(t->device)) return PIRIP_ERR_NO_DEVICE;
    return tbits_clear(t, (hipStream_t)hip_stream);
}

int pirip_hip_tbits_testframe_payload(int k, uint8_t *bytes_out)
{
    if (k < 8 || k % 8 || !bytes_out) return PIRIP_ERR_BAD_ARG;
    std::vector<uint8_t> bits((size_t)k);
    testframe_payload(bits.data(), k);
    pack_bits_msb(bytes_out, bits.data(), k);
    return PIRIP_OK;
}

int pirip_hip_tbits_set_payload(pirip_hip_tbits *t, int data_bytes, const uint8_t *payload)
{
    if (!t || data_bytes < 1) return PIRIP_ERR_BAD_ARG;
    std::vector<uint8_t> want((size_t)data_bytes);
    if (payload) std::memcpy(want.data(), payload, want.size());
    else PIRIP_TRY(pirip_hip_tbits_testframe_payload(8 * data_bytes, want.data()));
    if (!bind_device(t->device)) return PIRIP_ERR_NO_DEVICE;
    PIRIP_HIPCHK(hipDeviceSynchronize());                      // (a push_records in flight may still read the old one)
    t->mem.release(&t->d_want);
    t->data_bytes = 0;
    PIRIP_TRY(t->mem.upload(&t->d_want, want.data(), want.size()));
    t->data_bytes = data_bytes;
    return PIRIP_OK;
}

int pirip_hip_tbits_push_records(pirip_hip_tbits *t, const uint8_t *d_status, size_t status_stride, const uint8_t *d_payload, size_t payload_stride,
                                 const int32_t *d_info, size_t info_stride, const int32_t *d_ncalls, int ncalls, void *hip_stream)
{
    if (!t || ncalls < 0 || !t->d_want) return PIRIP_ERR_BAD_ARG;
    if (ncalls == 0) return PIRIP_OK;
    if (!d_status || !d_payload || !d_info) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(t->device)) return PIRIP_ERR_NO_DEVICE;
    const RecArgs a{d_status, status_stride, d_payload, payload_stride, d_info, info_stride, d_ncalls, ncalls, t->d_want, t->data_bytes, t->d_rcnt};
    hipLaunchKernelGGL(tbits_records_kernel, dim3((unsigned)t->nstreams), dim3(kLanes), 0, (hipStream_t)hip_stream, a);
    PIRIP_HIPCHK(hipGetLastError());
    return PIRIP_OK;
}

int pirip_hip_tbits_get_record_counters(pirip_hip_tbits *t, int64_t *frames, int64_t *bits, int64_t *errors, int64_t *frames_in_error,
                                        int64_t *crc_ok)
{
    if (!t) return PIRIP_ERR_BAD_ARG;
    int64_t *const cols[kRecCnt] = {frames, bits, errors, frames_in_error, crc_ok};
    return tbits_read(t, t->d_rcnt, kRecCnt, cols);
}

}  // extern "C"
