// pirip_amd/csrc/spec_kernels.hip -- section P of include/pirip_hip.h: the band monitor. Averaged wideband power spectra of a batch of IQ
// streams and the power, peak and peak bin of a list of bands, block after block, exact against kiss_fft.
//
// One kernel per push. Its grid is (rows the call touches + 1, nstreams):
//   workgroup x < touched  row row0 + x of stream y: the carried leading row, a complete row, or the trailing incomplete one. It takes its
//                          segments in ascending order. Per segment: w x goes straight into LDS in kiss_fft's leaf order (slot = the base-4
//                          digit reversal of the sample's index), the radix-4 stages run there in place, one butterfly per thread and stage
//                          (four with nfft = 4096), each stage behind a barrier, and the last stage's outputs stay in registers: a thread
//                          holds the same bins of every segment and adds |X|^2 to its running row. A complete row goes to d_rows and, through
//                          LDS, to the band walk: one lane per band of the stream, serially in the walking order the contract fixes. An
//                          incomplete row goes to the handle's running row.
//   workgroup x == touched the carry: the samples of the segments the call leaves incomplete, from the old tail and the call's input, into the
//                          new tail.
// The tail and the running row are kept twice: a call reads one half and writes the other (another workgroup of the same call may still
// read what this one replaces), and the host remembers which half is current. Samples of a segment that starts before the call come from
// the tail, so every output is a function of the stream's samples alone, however they were cut into calls.
// Arithmetic: the twiddle multiply is demod_simd.hpp's cmul_x on EVERY butterfly operand, the trivial twiddle (1, 0) of the first stage
// included, so that the sequence of float operations is kiss_fft's; -ffp-contract=off keeps the products of |X|^2 unfused.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "demod_simd.hpp"
#include "iq_device.hpp"
#include "spec_handle.hpp"

using namespace pirip;

namespace {

template <int NFFT> struct SpecShape {
    static constexpr int NT = NFFT / 4 < kSpecMaxThreads ? NFFT / 4 : kSpecMaxThreads;
    static constexpr int BPT = NFFT / 4 / NT;                        // butterflies per thread and stage
    static constexpr int LOG4 = NFFT == 256 ? 4 : NFFT == 1024 ? 5 : 6;
    static_assert((1 << (2 * LOG4)) == NFFT, "nfft is a power of 4");
};

// base-4 digit reversal of i < 4^LOG4: the bits reversed, then the two bits of every digit put back in order
template <int LOG4>
__device__ __forceinline__ int digit_reverse(int i)
{
    const uint32_t r = __brev((uint32_t)i) >> (32 - 2 * LOG4);
    return (int)(((r & 0x55555555u) << 1) | ((r >> 1) & 0x55555555u));
}

// Where slot s of the transform's work array lies in LDS: the low six bits exchanged by the bits above them. The 64 consecutive samples a
// wave stages differ in their three low base-4 digits, which leaf order makes the three HIGH digits of the slot: unswizzled, the 64 stores
// of one instruction fall into one bank. A permutation of addresses only: every value and every operation stay what they were.
// Not at 256 points: there the unswizzled stores are 8-way at worst, and the kernel measured no faster with the exchange.
template <int NFFT>
__device__ __forceinline__ int lds_slot(int s) { return NFFT > 256 ? s ^ ((s >> 6) & 63) : s; }

// where sample `rel` of the stream lies, counted from the call's first sample: in the call's input, or (rel < 0) in the tail of tail_len samples
template <int BSI>
__device__ __forceinline__ const char *spec_sample_ptr(const char *in, const char *tail, int64_t rel, int64_t tail_len)
{
    return rel >= 0 ? in + rel * BSI : tail + (rel + tail_len) * BSI;
}

template <int NFFT, int BSI>
__global__ __launch_bounds__(SpecShape<NFFT>::NT) void spec_kernel(SpecArgs a)
{
    using S = SpecShape<NFFT>;
    constexpr int NT = S::NT, BPT = S::BPT, LOG4 = S::LOG4, M = NFFT / 4;
    __shared__ __attribute__((aligned(16))) v2f s_x[NFFT];
    const int tid = threadIdx.x, r = blockIdx.y;
    const char *in = a.in + (size_t)r * a.in_stride;
    const char *tail = a.tail_in + (size_t)r * (size_t)(NFFT * BSI);
    const int64_t tail_len = a.pos - a.seg0 * a.hop;                 // samples of the old tail, < nfft

    if ((int)blockIdx.x == a.touched) {
        // the carry: samples seg1 hop .. pos + n - 1 of the stream are the new tail
        char *out = a.tail_out + (size_t)r * (size_t)(NFFT * BSI);
        const int64_t rel0 = a.seg1 * a.hop - a.pos;
        int64_t len = a.n - rel0;
        if (len > NFFT) len = NFFT;                                  // (never: segment seg1 is incomplete)
        for (int i = tid; i < (int)len; i += NT) {
            const char *p = spec_sample_ptr<BSI>(in, tail, rel0 + i, tail_len);
            if (BSI == 2) ((uint16_t *)out)[i] = *(const uint16_t *)p;
            else ((v2f *)out)[i] = *(const v2f *)p;
        }
        return;
    }

    const int64_t row = a.row0 + blockIdx.x;
    const int64_t k_first = row * a.avg;
    const int64_t k_lo = k_first > a.seg0 ? k_first : a.seg0;
    const int64_t k_hi = k_first + a.avg < a.seg1 ? k_first + a.avg : a.seg1;
    const bool carried = k_first < a.seg0, complete = k_first + a.avg <= a.seg1;

    // the thread's bins: butterfly u = tid + NT bb of the last stage gives the bins u + M j
    float acc[BPT][4];
#pragma unroll
    for (int bb = 0; bb < BPT; bb++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[bb][j] = carried ? a.acc_in[(size_t)r * NFFT + tid + NT * bb + M * j] : 0.f;

    const v2f c_hi{a.c_hi, a.c_hi}, c_lo{a.c_lo, a.c_lo};
    const v2f *__restrict__ tw = (const v2f *)a.twiddle;
    for (int64_t k = k_lo; k < k_hi; k++) {
        const int64_t rel0 = k * a.hop - a.pos;
#pragma unroll 4
        for (int i = tid; i < NFFT; i += NT) {
            const char *p = spec_sample_ptr<BSI>(in, tail, rel0 + i, tail_len);
            v2f x;
            if (BSI == 2) {
                const uint32_t b = *(const uint16_t *)p;
                x = u8_to_float(v2f{(float)(b & 255u), (float)(b >> 8)}, c_hi, c_lo);
            } else {
                x = *(const v2f *)p;
            }
            const float w = a.window[i];
            s_x[lds_slot<NFFT>(digit_reverse<LOG4>(i))] = x * v2f{w, w};
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < LOG4; s++) {
            const int m = 1 << (2 * s), fstride = NFFT >> (2 * s + 2);
#pragma unroll
            for (int bb = 0; bb < BPT; bb++) {
                const int u = tid + NT * bb, kk = u & (m - 1), base = ((u >> (2 * s)) << (2 * s + 2)) + kk;
                const int a0 = lds_slot<NFFT>(base), a1 = lds_slot<NFFT>(base + m), a2 = lds_slot<NFFT>(base + 2 * m), a3 = lds_slot<NFFT>(base + 3 * m);
                v2f f0 = s_x[a0], f1 = s_x[a1], f2 = s_x[a2], f3 = s_x[a3];
                f1 = cmul_x(f1, tw[kk * fstride]);
                f2 = cmul_x(f2, tw[2 * kk * fstride]);
                f3 = cmul_x(f3, tw[3 * kk * fstride]);
                bfly4(f0, f1, f2, f3);
                if (s < LOG4 - 1) {
                    s_x[a0] = f0; s_x[a1] = f1; s_x[a2] = f2; s_x[a3] = f3;
                } else {
                    // the last stage: base = u, the outputs are the bins u + M j
                    const v2f q0 = f0 * f0, q1 = f1 * f1, q2 = f2 * f2, q3 = f3 * f3;
                    acc[bb][0] = acc[bb][0] + (q0.x + q0.y);
                    acc[bb][1] = acc[bb][1] + (q1.x + q1.y);
                    acc[bb][2] = acc[bb][2] + (q2.x + q2.y);
                    acc[bb][3] = acc[bb][3] + (q3.x + q3.y);
                }
            }
            __syncthreads();
        }
    }

    if (!complete) {
#pragma unroll
        for (int bb = 0; bb < BPT; bb++)
#pragma unroll
            for (int j = 0; j < 4; j++) a.acc_out[(size_t)r * NFFT + tid + NT * bb + M * j] = acc[bb][j];
        return;
    }
    // a complete row: entry blockIdx.x of this call's output
    float *s_row = (float *)s_x;
    float *g_row = a.rows ? a.rows + (size_t)r * a.stream_stride + (size_t)blockIdx.x * a.row_stride : nullptr;
#pragma unroll
    for (int bb = 0; bb < BPT; bb++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int b = tid + NT * bb + M * j;
            s_row[b] = acc[bb][j];
            if (g_row) g_row[b] = acc[bb][j];
        }
    __syncthreads();
    for (int q = a.band_start[r] + tid; q < a.band_start[r + 1]; q += NT) {
        const SpecBand band = a.bands[q];
        int b = band.first, peak_bin = b;
        float power = 0.f, peak = s_row[b];
        for (int c = 0; c < band.count; c++) {
            const float v = s_row[b];
            power = power + v;
            if (v > peak) { peak = v; peak_bin = b; }
            b = (b + 1) & (NFFT - 1);
        }
        a.band_rows[(size_t)band.index * a.band_stride + blockIdx.x] = pirip_spec_band_row{power, peak, peak_bin};
    }
}

template <int NFFT>
void spec_launch(int bsi, dim3 grid, hipStream_t st, const SpecArgs &a)
{
    const dim3 block(SpecShape<NFFT>::NT);
    if (bsi == 2) hipLaunchKernelGGL((spec_kernel<NFFT, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((spec_kernel<NFFT, 8>), grid, block, 0, st, a);
}

bool nfft_ok(int nfft) { return nfft == 256 || nfft == 1024 || nfft == 4096; }

// complete segments of a stream of t samples
int64_t segments(int64_t t, int nfft, int hop) { return t < nfft ? 0 : (t - nfft) / hop + 1; }

void make_window(int nfft, float *w)
{
    // the upper half is the lower half mirrored: w[i] == w[nfft - i] whatever cos() gives
    for (int i = 0; i <= nfft / 2; i++) w[i] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)i / (double)nfft));
    for (int i = nfft / 2 + 1; i < nfft; i++) w[i] = w[nfft - i];
}

// bin(f) = floor((2 f nfft + Fs) / (2 Fs)) mod nfft, floor toward minus infinity
int32_t bin_of(int64_t f, int nfft, int Fs)
{
    const int64_t num = 2 * f * nfft + Fs, den = 2 * (int64_t)Fs;
    int64_t q = num / den;
    if (num % den < 0) q -= 1;
    return (int32_t)(((q % nfft) + nfft) % nfft);
}

}  // namespace

extern "C" {

int pirip_hip_spec_window(int nfft, float *w)
{
    if (!w) return PIRIP_ERR_BAD_ARG;
    if (!nfft_ok(nfft)) return PIRIP_ERR_UNSUPPORTED;
    make_window(nfft, w);
    return PIRIP_OK;
}

int pirip_hip_spec_create(int Fs, int in_format, int nfft, int hop, int avg, int nstreams, int nbands, const pirip_spec_band *bands, int device,
                          pirip_hip_spec **out)
{
    if (!out) return PIRIP_ERR_BAD_ARG;
    *out = nullptr;
    if (Fs < 2 || nstreams < 1 || nbands < 0 || avg < 1 || (nbands > 0 && !bands)) return PIRIP_ERR_BAD_ARG;
    if (in_format != PIRIP_IN_CU8_CSDR && in_format != PIRIP_IN_CF32) return PIRIP_ERR_BAD_ARG;
    for (int q = 0; q < nbands; q++) {
        const int64_t lo2 = 2 * (int64_t)bands[q].lo_hz, hi2 = 2 * (int64_t)bands[q].hi_hz;
        if (bands[q].stream < 0 || bands[q].stream >= nstreams || lo2 > hi2 || lo2 < -(int64_t)Fs || hi2 >= (int64_t)Fs) return PIRIP_ERR_BAD_ARG;
    }
    if (!nfft_ok(nfft) || (hop != nfft && hop != nfft / 2) || avg > kSpecMaxAvg || Fs > kMaxFs || nstreams > kSpecMaxStreams)
        return PIRIP_ERR_UNSUPPORTED;
    int dev = 0;
    PIRIP_TRY(select_device(device, &dev));

    pirip_hip_spec *h = new pirip_hip_spec;
    h->Fs = Fs; h->in_format = in_format; h->nfft = nfft; h->hop = hop; h->avg = avg; h->nstreams = nstreams; h->nbands = nbands; h->device = dev;
    h->bsi = bytes_per_sample(in_format);
    h->u8 = csdr_u8_split();
    if (!h->u8.exact) { delete h; return PIRIP_ERR_UNSUPPORTED; }
    std::vector<float> w((size_t)nfft), tw;
    make_window(nfft, w.data());
    fft_twiddles(nfft, &tw);
    double sum = 0.0;
    for (int i = 0; i < nfft; i++) sum += (double)w[i] * (double)w[i];
    h->scale = 1.0 / ((double)avg * sum);
    // the bands by stream, ascending band index within one
    std::vector<int32_t> start((size_t)nstreams + 1, 0);
    for (int q = 0; q < nbands; q++) {
        const int32_t first = bin_of(bands[q].lo_hz, nfft, Fs), last = bin_of(bands[q].hi_hz, nfft, Fs);
        h->bands.push_back(SpecBand{first, ((last - first + nfft) % nfft) + 1, q});
        start[(size_t)bands[q].stream + 1]++;
    }
    for (int r = 0; r < nstreams; r++) start[(size_t)r + 1] += start[(size_t)r];
    std::vector<SpecBand> sorted((size_t)nbands);
    {
        std::vector<int32_t> at(start.begin(), start.end() - 1);
        for (int q = 0; q < nbands; q++) sorted[(size_t)at[(size_t)bands[q].stream]++] = h->bands[(size_t)q];
    }
    const size_t state = (size_t)nstreams * (size_t)nfft;
    int rc = h->mem.alloc_filled(&h->d_tail, 0, 2 * state * (size_t)h->bsi);
    if (rc == PIRIP_OK) rc = h->mem.alloc_filled(&h->d_acc, 0, 2 * state * sizeof(float));
    if (rc == PIRIP_OK) rc = h->mem.upload(&h->d_window, w.data(), sizeof(float) * w.size());
    if (rc == PIRIP_OK) rc = h->mem.upload(&h->d_twiddle, tw.data(), sizeof(float) * tw.size());
    if (rc == PIRIP_OK) rc = h->mem.upload(&h->d_band_start, start.data(), sizeof(int32_t) * start.size());
    if (rc == PIRIP_OK) rc = h->mem.upload(&h->d_bands, sorted.data(), sizeof(SpecBand) * sorted.size());
    if (rc != PIRIP_OK) { delete h; return rc; }
    *out = h;
    return PIRIP_OK;
}

int pirip_hip_spec_destroy(pirip_hip_spec *h) { return destroy_handle(h, h ? h->device : 0); }

int pirip_hip_spec_get_info(const pirip_hip_spec *h, pirip_spec_info *info)
{
    if (!h || !info) return PIRIP_ERR_BAD_ARG;
    *info = pirip_spec_info{h->Fs, h->in_format, h->nfft, h->hop, h->avg, h->nstreams, h->nbands, h->device, h->scale};
    return PIRIP_OK;
}

int pirip_hip_spec_band_bins(const pirip_hip_spec *h, int band, int32_t *first_bin, int32_t *nbins)
{
    if (!h || band < 0 || band >= h->nbands) return PIRIP_ERR_BAD_ARG;
    if (first_bin) *first_bin = h->bands[(size_t)band].first;
    if (nbins) *nbins = h->bands[(size_t)band].count;
    return PIRIP_OK;
}

int64_t pirip_hip_spec_nrows(const pirip_hip_spec *h, int64_t n)
{
    if (!h || n < 0) return PIRIP_ERR_BAD_ARG;
    if (n >= kSpecMaxIndex || h->pos + n >= kSpecMaxIndex) return PIRIP_ERR_UNSUPPORTED;
    return segments(h->pos + n, h->nfft, h->hop) / h->avg - segments(h->pos, h->nfft, h->hop) / h->avg;
}

int pirip_hip_spec_push(pirip_hip_spec *h, const void *d_in, size_t in_stride_bytes, int64_t n, float *d_rows, size_t row_stride,
                        size_t stream_stride, pirip_spec_band_row *d_bands, size_t band_stride, void *hip_stream)
{
    if (!h || !d_in || n < 1 || (h->nbands > 0 && !d_bands)) return PIRIP_ERR_BAD_ARG;
    PIRIP_TRY(iq_rows_check(d_in, in_stride_bytes, h->bsi, h->nstreams, n));
    if (n >= kSpecMaxIndex || h->pos + n >= kSpecMaxIndex) return PIRIP_ERR_UNSUPPORTED;
    const int64_t seg0 = segments(h->pos, h->nfft, h->hop), seg1 = segments(h->pos + n, h->nfft, h->hop);
    const int64_t row0 = seg0 / h->avg, m = seg1 / h->avg - row0;
    const int64_t touched = seg1 > seg0 ? (seg1 - 1) / h->avg - row0 + 1 : 0;
    // output rows: whole floats (band entries: whole words), and strides that keep rows, streams and bands apart
    if (d_rows) {
        if ((uintptr_t)d_rows & 3) return PIRIP_ERR_BAD_ARG;
        if (m > 1 && row_stride < (size_t)h->nfft) return PIRIP_ERR_BAD_ARG;
        if (m > 0 && h->nstreams > 1 && stream_stride < (size_t)(m - 1) * row_stride + (size_t)h->nfft) return PIRIP_ERR_BAD_ARG;
    }
    if (d_bands) {
        if ((uintptr_t)d_bands & 3) return PIRIP_ERR_BAD_ARG;
        if (h->nbands > 1 && band_stride < (size_t)m) return PIRIP_ERR_BAD_ARG;
    }
    if (touched > 0x7ffffffe) return PIRIP_ERR_UNSUPPORTED;
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    const size_t state = (size_t)h->nstreams * (size_t)h->nfft;
    const bool segs = seg1 > seg0;
    SpecArgs a{};
    a.in = (const char *)d_in; a.in_stride = in_stride_bytes;
    a.tail_in = h->d_tail + (size_t)h->tail_cur * state * (size_t)h->bsi;
    a.tail_out = h->d_tail + (size_t)(h->tail_cur ^ 1) * state * (size_t)h->bsi;
    a.acc_in = h->d_acc + (size_t)h->acc_cur * state;
    a.acc_out = h->d_acc + (size_t)(h->acc_cur ^ 1) * state;
    a.window = h->d_window; a.twiddle = h->d_twiddle; a.band_start = h->d_band_start; a.bands = h->d_bands;
    a.rows = d_rows; a.row_stride = row_stride; a.stream_stride = stream_stride;
    a.band_rows = d_bands; a.band_stride = band_stride;
    a.pos = h->pos; a.n = n; a.seg0 = seg0; a.seg1 = seg1; a.row0 = row0; a.touched = (int32_t)touched;
    a.hop = h->hop; a.avg = h->avg; a.c_hi = h->u8.c_hi; a.c_lo = h->u8.c_lo;
    const dim3 grid((unsigned)touched + 1, (unsigned)h->nstreams);
    hipStream_t st = (hipStream_t)hip_stream;
    if (h->nfft == 256) spec_launch<256>(h->bsi, grid, st, a);
    else if (h->nfft == 1024) spec_launch<1024>(h->bsi, grid, st, a);
    else spec_launch<4096>(h->bsi, grid, st, a);
    if (hipGetLastError() != hipSuccess) return PIRIP_ERR_HIP;
    h->pos += n;
    h->tail_cur ^= 1;
    if (segs) h->acc_cur ^= 1;
    return PIRIP_OK;
}

int pirip_hip_spec_reset(pirip_hip_spec *h, void *hip_stream)
{
    (void)hip_stream;                                                   // nothing to enqueue: an empty tail and no running row are host state
    if (!h) return PIRIP_ERR_BAD_ARG;
    h->pos = 0;
    return PIRIP_OK;
}

}  // extern "C"
