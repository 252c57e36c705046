/* include/pirip_hip.h -- C-ABI of the MI355X-native FSK receive path (libpirip_hip.so).
 *
 * This is the drop-in boundary for pirip's IQ->bits hot path. pirip itself has no
 * plugin/operator API; the path sits behind (1) process boundaries -- the executables and
 * byte streams its scripts drive -- and (2) the libcodec2 / libcsdr C APIs that `rtl_fsk`
 * links (/root/reference/build_rtlsdr.sh:9). Both levels are served from this library:
 *
 *   section A  batch-of-streams device API (pirip_hip_*)  : what bench.py / a multi-channel
 *              receiver binds; device pointers in, device pointers out, explicit HIP stream.
 *   section B  csdr front end (pirip_hip_decim_*)          : convert_u8_f | fir_decimate_cc D
 *              | convert_f_s16 of /root/reference/README.md:109,162 as one device stage.
 *   section C  libcodec2-compatible single-stream shim      : fsk_create_hbr / fsk_nin /
 *              fsk_demod / fsk_demod_sd ... with codec2's own names and calling convention
 *              [UPSTREAM-RECALLED codec2 src/fsk.h], so `rtl_fsk` and `fsk_demod` link
 *              against libpirip_hip.so instead of libcodec2.so.
 *   section G  streaming receiver (pirip_hip_rx_*)         : sections A, B and E as a live
 *              N-channel receiver, each channel's tail carried on the device.
 *   section H  channelizer (pirip_hip_chan_*)              : K channels out of W wideband u8 IQ
 *              captures (shift_addition_cc | fir_decimate_cc D per channel), one pass over
 *              the input; also the front end of a section G receiver.
 *   section I  FSK_LDPC transmit (pirip_hip_tx_*)           : rpitx_fsk --code's record protocol ->
 *              channel symbols -> continuous-phase M-FSK IQ for a batch of streams.
 *   section J  multiplexer (pirip_hip_mux_*)               : K modem-rate channels interpolated,
 *              shifted, scaled and summed onto W wideband u8 / complex float IQ streams.
 *   section K  streaming transmitter (pirip_hip_txs_*)      : section G's mirror image, queued records to wideband IQ block after block.
 *   section L  test-frame counter (pirip_hip_tbits_*)       : fsk_put_test_bits / rtl_fsk --testframes for a batch of streams,
 *              counted on the device behind the demodulator or the receiver.
 *   section O  channel (pirip_hip_air_*)                    : T transmitted wideband IQ streams onto R received ones: paths with
 *              gain, delay, carrier offset, sample-clock offset and Rayleigh / Rician fading, AWGN per receiver, block after block.
 *   section P  band monitor (pirip_hip_spec_*)              : averaged wideband power spectra of a batch of IQ streams and the power,
 *              peak and peak bin of a list of bands, block after block, exact against kiss_fft.
 *   section D  libcsdr-compatible entry points              : convert_u8_f, convert_f_s16,
 *              firdes_*, fir_decimate_cc
 *              [UPSTREAM-RECALLED csdr libcsdr.h].
 *
 * No torch types, no C++ types: plain pointers and sizes. Every function returns
 * PIRIP_OK (0) or a negative error; nothing here falls back to a CPU implementation --
 * without a usable HIP device every compute entry point returns PIRIP_ERR_NO_DEVICE.
 *
 * Reference call sites that pin the behaviour (arguments, byte formats):
 *   fsk_demod -d -p 24 2 240000 10000   /root/reference/test/loopback_rtl_sdr.sh:16
 *   fsk_demod --fsk_lower 500 --fsk_upper 25000 -d -p 24 ...  /root/reference/README.md:105
 *   csdr convert_u8_f | fir_decimate_cc 45 | convert_f_s16 | fsk_demod -c 2 40000 1000
 *                                        /root/reference/README.md:109
 *   rtl_fsk ... (in-process convert_u8_f + fsk_demod)  /root/reference/test/loopback_rtl_fsk.sh:10
 */
#ifndef PIRIP_HIP_H
#define PIRIP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ----------------------------------------------------------------------------------- */
/* status codes                                                                         */
/* ----------------------------------------------------------------------------------- */
#define PIRIP_OK               0
#define PIRIP_ERR_BAD_ARG     (-1)   /* NULL pointer / size out of range                  */
#define PIRIP_ERR_BAD_CONFIG  (-2)   /* what codec2's fsk_create_core() would assert on   */
#define PIRIP_ERR_NO_DEVICE   (-3)   /* no HIP device / HIP runtime error at create       */
#define PIRIP_ERR_HIP         (-4)   /* HIP runtime error during a call                   */
#define PIRIP_ERR_NOMEM       (-5)
#define PIRIP_ERR_UNSUPPORTED (-6)

/* input sample formats (what the front end hands to the demodulator) */
#define PIRIP_IN_CU8_FSKDEMOD 0   /* fsk_demod -d : interleaved u8 IQ, (x-127)/128         */
#define PIRIP_IN_CU8_CSDR     1   /* csdr convert_u8_f / rtl_fsk : u8 IQ, x/127.5-1        */
#define PIRIP_IN_CS16         2   /* fsk_demod -c : interleaved s16 IQ, x/FDMDV_SCALE      */
#define PIRIP_IN_CF32         3   /* COMP {float real, imag}                               */

#define PIRIP_MODE_M_MAX 4
#define PIRIP_FSK_DEFAULT_P 8
#define PIRIP_FSK_DEFAULT_NSYM 50
#define PIRIP_FDMDV_SCALE 750
#define PIRIP_STATS_PER_FRAME 10  /* f_est[0..3], norm_rx_timing, SNRest, nin_next, ppm, rx_sig_pow, rx_nse_pow
                                     (the last two: what freedv_get_fsk_S_and_N() hands rtl_fsk -L, README.md:59) */

/* ----------------------------------------------------------------------------------- */
/* section A : batch-of-streams demodulator                                             */
/* ----------------------------------------------------------------------------------- */

/* Modem configuration: the arguments of codec2 fsk_create_hbr() + fsk_set_freq_est_limits()
 * + fsk_set_freq_est_alg() [UPSTREAM-RECALLED fsk.h], as driven by fsk_demod's argv
 * (/root/reference/README.md:105). */
typedef struct pirip_fsk_params {
    int Fs;             /* sample rate, Hz                                                */
    int Rs;             /* symbol rate; Fs % Rs == 0                                      */
    int M;              /* 2 or 4 tones                                                   */
    int P;              /* timing oversample (-p); (Fs/Rs) % P == 0, P >= 4               */
    int Nsym;           /* symbols per demod frame (default 50)                           */
    int est_min;        /* --fsk_lower, Hz                                                */
    int est_max;        /* --fsk_upper, Hz (est_min == est_max == 0: fsk_create defaults) */
    int freq_est_type;  /* 0 = peak picker, 1 = --mask comb                               */
    int tone_spacing;   /* --mask spacing, Hz (only read when freq_est_type == 1)         */
    int in_format;      /* PIRIP_IN_*                                                     */
} pirip_fsk_params;

/* Derived constants (what codec2 keeps in struct FSK). */
typedef struct pirip_fsk_info {
    int Ts, N, Nmem, Ndft, Nbits, nin_max, nstreams;
    int bytes_per_sample;   /* of the configured in_format (one complex sample)           */
} pirip_fsk_info;

typedef struct pirip_hip_demod pirip_hip_demod;   /* opaque: nstreams x struct FSK on device */

/* Create `nstreams` independent demodulators (one struct FSK each, all the same
 * configuration) resident on HIP device `device` (-1 = current device). Replaces
 * nstreams x fsk_create_hbr()+fsk_set_freq_est_limits()+fsk_set_freq_est_alg(). Every later call on
 * the handle runs on that device (the library selects it), whatever the caller's current device is. */
int pirip_hip_create(const pirip_fsk_params *params, int nstreams, int device, pirip_hip_demod **out);

/* Every constant of the demodulator that this repository holds FROM RECALL of codec2's fsk.c / fsk_demod.c rather than from a source it
 * could read (SURVEY.md 8c's verify-when-source-appears list; /root/reference/build_codec2.sh:3-5 clones an un-pinned HEAD, so any of
 * them may differ on the day the oracle is pinned). Each is one field here and in the CPU restatement (oracle/fsk_oracle.h:
 * fsk_oracle_recalled, same layout); pirip_hip_recalled_defaults() fills in today's values, which is what pirip_hip_create() runs.
 * The specialised kernels (PIRIP_KERNEL_WAVE / _BLOCK) are built around the defaults of the fields marked [k]: a handle created
 * with another value of one of those is served by the any-configuration kernel, which reads all of them from the plan. The others
 * are table / plan data for every kernel. oracle/pin_against_ref.py names, per failing case, the field whose other value repairs it. */
typedef struct pirip_fsk_recalled {
    int hann_denominator_ndft;  /* Hann window 0.5 - 0.5 cos(2 pi i / D): 0: D = Ndft - 1 (recalled), 1: D = Ndft                      */
    float tc;                   /* smoothing of Sf, 0.1                                                                                 */
    float est_space_rs;         /* blanking around a found peak, in symbol rates: 0.75                                                  */
    float nin_threshold;        /* [k] |norm_rx_timing| beyond which nin moves: 0.25                                                    */
    int nin_step_div;           /* [k] nin moves by Ts / nin_step_div samples: 4 (older fsk.c: 2)                                       */
    float s16_scale;            /* [k] FDMDV_SCALE, the divisor of `fsk_demod -c` int16 samples: 750 (codec2_fdmdv.h; 1000 elsewhere)   */
    float u8d_offset;           /* [k] fsk_demod -d: (x - u8d_offset) / u8d_scale: 127                                                  */
    float u8d_scale;            /* [k]                                              128                                                 */
    int ndft_rule;              /* [k] 0: bins of 0.1 Rs, next power of two (recalled); 1: largest power of two <= N (older fsk.c)      */
    int sf_power;               /* [k] what is smoothed into Sf: 0: |X| (recalled), 1: |X|^2                                            */
} pirip_fsk_recalled;
void pirip_hip_recalled_defaults(pirip_fsk_recalled *r);
/* pirip_hip_create with the recalled constants spelled out (recalled == NULL: the defaults). PIRIP_ERR_BAD_CONFIG for values no
 * demodulator can run (tc outside (0, 1], scales <= 0, nin_step_div < 2 or a step of 0 samples, a threshold outside (0, 0.5)). */
int pirip_hip_create_recalled(const pirip_fsk_params *params, const pirip_fsk_recalled *recalled, int nstreams, int device, pirip_hip_demod **out);
int pirip_hip_destroy(pirip_hip_demod *h);
int pirip_hip_get_info(const pirip_hip_demod *h, pirip_fsk_info *info);
/* Which device kernel serves this handle (chosen once at create): PIRIP_KERNEL_WAVE = a specialised wave-per-stream instance
 * (the reference's command-line shapes), PIRIP_KERNEL_GENERAL = the any-configuration kernel. Diagnostics: lets
 * a test or an operator confirm that a configuration is on the fast path. */
#define PIRIP_KERNEL_GENERAL 0
#define PIRIP_KERNEL_WAVE 2
#define PIRIP_KERNEL_EXACT 4    /* PIRIP_KERNEL=exact only: every frame in the CPU algorithm's own operation order (one thread walks the
                                 * oscillator and timing sums) -- bits, soft magnitudes, timing, nin, SNRest bit-equal to the CPU path at
                                 * any SNR; a cross-check at ~0.15 ms per frame and stream, never chosen by default */
#define PIRIP_KERNEL_BLOCK 3    /* workgroup-per-stream instance for long symbols (Ts = 240 / Ndft = 4096: rtl_fsk -r 1000 at 240 kS/s) */
int pirip_hip_get_kernel(const pirip_hip_demod *h);
/* The first frame of a stream after create / reset is demodulated, where the shape has P == Ts (`fsk_demod -p 24` at 24 samples per
 * symbol: a window of the integrator bank can then hold a single sample and the very first decision of a recording that starts one
 * sample before a symbol boundary is a float-rounding tie), by a prologue kernel that performs the CPU restatement's operations in its
 * order -- serial oscillator recursion, forward window sums, serial timing sum, glibc's atan2f -- so that frame is bit for bit the
 * oracle's (bits, soft magnitudes, timing). On by default; 0 switches it off (measurement A/B). Also PIRIP_EXACT0=0 at create. */
int pirip_hip_set_exact_first_frame(pirip_hip_demod *h, int enable);
/* The same as text: the instance (template arguments, streams per workgroup, waves per SIMD) or the general kernel with its
 * run-time shape -- what bench.py prints as config.kernel. */
int pirip_hip_get_kernel_name(const pirip_hip_demod *h, char *buf, size_t n);
/* Back to the state fsk_create_hbr() leaves (Sf = 0, oscillators at phase 0, nin = N). Enqueued on hip_stream (NULL = default stream);
 * never synchronises -- the streaming handles' resets (sections G, M, N, R, S) come through here. */
int pirip_hip_reset(pirip_hip_demod *h, void *hip_stream);
/* fsk_clear_estimators() for every stream [UPSTREAM-RECALLED codec2 fsk.c]: the smoothed spectrum Sf back to zero and nin back
 * to N -- oscillator phases, integrator memory, timing and ppm estimates stay, as upstream leaves them. Enqueued on hip_stream; never
 * synchronises. */
int pirip_hip_clear_estimators(pirip_hip_demod *h, void *hip_stream);

/* Demodulate one batch. Stream s reads complex samples from
 *     (const char*)d_in + s*in_stride_bytes,  nsamp samples of the configured in_format,
 * and runs codec2's read loop on it: while nin samples remain (and frames < max_frames)
 * { fsk_demod(); advance by nin; nin = fsk_nin() }. State carries to the next call, so a
 * caller streams by re-presenting the unconsumed tail (see d_consumed) ahead of new data.
 * All d_* pointers are DEVICE pointers; outputs may be NULL when not wanted:
 *   d_bits    [s][frame][Nbits]  one bit per byte (fsk_demod's stdout format)
 *   d_rx_filt [s][frame][M*Nsym] soft magnitudes, fsk_demod_sd() layout [m][sym]
 *   d_stats   [s][frame][PIRIP_STATS_PER_FRAME]
 *   d_nframes [s] frames produced;  d_consumed [s] samples consumed (int64)
 * Strides are in elements of the respective array (bytes / floats / floats) per stream.
 * Work is enqueued on `hip_stream` (a hipStream_t, NULL = default stream); the call does
 * not synchronise. */
int pirip_hip_demod_batch(pirip_hip_demod *h,
                          const void *d_in, size_t in_stride_bytes, int64_t nsamp,
                          uint8_t *d_bits, size_t bits_stride,
                          float *d_rx_filt, size_t filt_stride,
                          float *d_stats, size_t stats_stride,
                          int32_t *d_nframes, int64_t *d_consumed,
                          int64_t max_frames, void *hip_stream);

/* ONE long capture -- what `fsk_demod` gets when its input is a file ([UPSTREAM-RECALLED] fsk_demod.c usage: InputModemRawFile
 * OutputOneBitPerByteFile; the reference's own command lines give it pipes, /root/reference/README.md:105,109) -- demodulated on
 * many wavefronts with results identical to the read loop of pirip_hip_demod_batch on a one-stream handle: same frames, same bits / soft magnitudes / statistics rows, same d_consumed,
 * same state left behind (fsk_demod()'s frame-to-frame chain is cut into segments that are demodulated speculatively and kept only
 * where their start state proves, bit for bit, to be the state the segment before ended in; pirip_amd/csrc/capture.hip).
 * The handle's streams are the work slots: create it with nstreams = how many segments may run at once (>= 4; a few hundred to a
 * few thousand fill the GPU); stream slot 0 holds the capture's state between calls, so a capture too big for one call is
 * presented in pieces exactly like a stream (unconsumed tail ahead of the next piece). Handles served by the general kernel, short
 * inputs and nstreams < 4 take the sequential loop on slot 0 -- the results do not depend on the route.
 *   d_in       nsamp samples of the configured in_format (DEVICE pointer)
 *   d_bits     [frame][Nbits] (or packed, pirip_hip_set_bit_packing), d_rx_filt [frame][M*Nsym], d_stats [frame][PIRIP_STATS_PER_FRAME]:
 *              room for max_frames frames each; d_rx_filt and d_stats may be NULL
 *   nframes / consumed: frames produced and samples consumed (host)
 *   report     optional: how the call went
 * The call synchronises `hip_stream` (it decides on the host what to re-run). */
typedef struct pirip_capture_report {
    int32_t segments;            /* segments the capture was cut into (1: sequential route)                         */
    int32_t segment_frames;      /* frames per segment (0: sequential route)                                         */
    int32_t passes;              /* launches of the segment set: 1 = every speculative start verified at once        */
    int32_t segments_rerun;      /* segment runs in passes after the first                                           */
    int64_t frames_demodulated;  /* frames demodulated in all, warm-ups and re-runs included (>= nframes)            */
} pirip_capture_report;
int pirip_hip_demod_capture(pirip_hip_demod *h, const void *d_in, int64_t nsamp, uint8_t *d_bits, float *d_rx_filt, float *d_stats,
                            int64_t max_frames, int64_t *nframes, int64_t *consumed, pirip_capture_report *report, void *hip_stream);
/* The same with HOST buffers (upload, demodulate, download): what the fsk_demod tool calls when its input is a file. */
int pirip_hip_demod_capture_host(pirip_hip_demod *h, const void *in, int64_t nsamp, uint8_t *bits, float *rx_filt, float *stats,
                                 int64_t max_frames, int64_t *nframes, int64_t *consumed, pirip_capture_report *report);

/* Host-buffer convenience for one-stream callers (the CLI tools and section C): uploads
 * `nsamp` samples, runs stream 0, downloads. bits/rx_filt/stats sized for max_frames. */
int pirip_hip_demod_host(pirip_hip_demod *h, const void *in, int64_t nsamp,
                         uint8_t *bits, float *rx_filt, float *stats,
                         int64_t max_frames, int64_t *nframes, int64_t *consumed);
/* nin of stream 0 as of the last synchronised call (fsk_nin()). */
int pirip_hip_nin0(pirip_hip_demod *h);

/* Output format of d_bits / bits for subsequent calls: packed = 0 (default) one byte per bit, the
 * reference's stdout format; packed = 1: ceil(Nbits/8) bytes per frame, 8 bits per byte, MSB first --
 * codec2's freedv_pack order, the order `rpitx_fsk --packed` consumes (/root/reference/tx/rpitx_fsk.cpp:75-83,
 * script/frame_repeater:38). Strides and frame offsets are then in packed bytes. */
int pirip_hip_set_bit_packing(pirip_hip_demod *h, int packed);

/* Band-only frequency estimator (OPT-IN, default off). codec2's fsk_demod_freq_est smooths |X| of all Ndft FFT bins into Sf and
 * then searches the peaks in [est_min, est_max] only [UPSTREAM-RECALLED fsk.c]: bins outside that range cannot reach any output
 * of fsk_demod (bits, soft decisions, f_est, timing, SNR figures). With enable = 1 the demodulator computes and smooths only the
 * FFT bins the search can read -- today: Ndft = 256 handles on a wave instance built for it, peak estimator, 0 <= est_min: the 2-FSK
 * `fsk_demod -p 24` shape with est_max < 32 Fs/256 (bins 0 .. 31: up to 30 kHz at 240 kS/s) and the 4-FSK P = 8 shape with est_max <= 64 Fs/256
 * (bins 0 .. 63), both 8-bit input formats; PIRIP_ERR_UNSUPPORTED elsewhere. The surviving
 * bins go through the same butterflies on the same operands: Sf inside the band, f_est and every output stay bit-identical to the
 * full estimator's (tests/test_gpu_parity.py::test_band_only_estimator_*). What changes: Sf OUTSIDE the band is no longer updated
 * (pirip_hip_get_Sf returns stale values there -- leave it off where the whole spectrum is an output, as for rtl_fsk's dashboard),
 * pirip_hip_set_freq_est_limits() refuses a range that leaves the band, and switching it off again resets the streams. */
int pirip_hip_set_estimator_band_only(pirip_hip_demod *h, int enable);

/* Launch tail of the wave-per-stream demodulator. A launch of more workgroups than the device holds at once ends with its queue run
 * dry: the workgroups dispatched last have their whole stream ahead of them while the waves they share a SIMD with are nearly done, and
 * the hardware issues the oldest wave first. With enable = 1 (the default) the workgroups of the launch's last residency -- the highest
 * block indices, as many as the device holds at once -- start at wave priority 1; a launch of one residency or less raises nothing.
 * Every output word is the same either way: only the order in which the hardware issues the waves' instructions changes. Applies to
 * every later launch of the handle (batch, chunked, capture and segment calls); 0 switches it off (measurement A/B). */
int pirip_hip_set_launch_tail_first(pirip_hip_demod *h, int enable);
/* Workgroups of the handle's wave instance that its device holds at once (streams per CU / streams per workgroup x compute units);
 * 0 for a handle on another kernel. */
int pirip_hip_get_launch_resident_blocks(const pirip_hip_demod *h);
/* The rule itself, as a pure function (no device): a launch of `nblocks` workgroups of `streams_per_block` streams on `cus` compute
 * units that hold `streams_per_cu` streams each. Returns the first block index that starts at the raised priority (nblocks: none), or a
 * negative PIRIP_ERR_*. */
int pirip_hip_launch_first_tail_block(int nblocks, int streams_per_cu, int streams_per_block, int cus);

/* fsk_enable_burst_mode() for every stream of the handle [UPSTREAM-RECALLED fsk.c]: nin is reset to N
 * and no longer follows the timing estimate. */
int pirip_hip_set_burst_mode(pirip_hip_demod *h, int enable);

/* Frequency-estimator spectrum of stream `s` (Ndft floats, DC at Ndft/2): the `SfdB`
 * source of rtl_fsk's dashboard JSON (/root/reference/script/dash.py:41). Synchronises. */
int pirip_hip_get_Sf(pirip_hip_demod *h, int s, float *Sf_host);
/* Eye diagram, the rx_eye / neyetr / neyesamp members of codec2's MODEM_STATS that fsk_demod_core fills for `fsk_demod -t`'s GUI
 * [UPSTREAM-RECALLED codec2 src/fsk.c, end of fsk_demod_core; src/modem_stats.h]: 8 / M traces per tone, each two symbols of
 * |f_int| (at most 160 points), trace i of tone m in row i*M + m. pirip_hip_enable_eye(h, 1) makes every later demodulator call
 * keep the traces of each stream's latest frame; it moves the handle to the any-configuration kernel (the only one that holds a
 * frame's integrator outputs) and RESETS the stream state, so call it right after pirip_hip_create. A diagnostic, as upstream's
 * is: not for throughput. pirip_hip_get_eye copies stream s's traces to rx_eye[8][160] (row stride 160), divided by their
 * largest value when `normalise` is set (upstream's default, fsk_stats_normalise_eye). Synchronises. */
int pirip_hip_enable_eye(pirip_hip_demod *h, int enable);
int pirip_hip_get_eye(pirip_hip_demod *h, int s, int normalise, float *rx_eye, int *neyetr, int *neyesamp);
/* Scalar state of stream `s` after the last call: f_est[0..3], norm_rx_timing, SNRest,
 * nin (as float), ppm -- the fields rtl_fsk reads out of struct FSK for its -v log line and
 * UDP JSON (/root/reference/script/dash.py:26-45). Synchronises. */
int pirip_hip_get_scalars(pirip_hip_demod *h, int s, float out8[8]);
/* All of it: what codec2 keeps in struct FSK between calls. snr_est / EbNodB / v_est are refreshed on OBSERVABLE frames --
 * frames whose per-frame stats are written, and the last frame of a call -- (the wave-per-stream kernel skips their
 * reductions elsewhere), so they equal codec2's values whenever d_stats is requested or calls carry one frame. */
typedef struct pirip_stream_state {
    int nin;
    float norm_rx_timing, ppm, snr_est, SNRest, EbNodB, v_est, f_est[4];
    float rx_sig_pow, rx_nse_pow;      /* mean power of the decided tone / of the other tones over the last observable frame */
} pirip_stream_state;
int pirip_hip_get_stream_state(pirip_hip_demod *h, int s, pirip_stream_state *out);
/* fsk_set_freq_est_limits() on a live handle: the search range changes, Sf / oscillators / timing state are kept. */
int pirip_hip_set_freq_est_limits(pirip_hip_demod *h, int est_min, int est_max);

/* ----------------------------------------------------------------------------------- */
/* section B : csdr front end  (convert_u8_f | fir_decimate_cc D [tbw] | convert_f_s16)  */
/* ----------------------------------------------------------------------------------- */
typedef struct pirip_hip_decim pirip_hip_decim;

/* decimation D, transition_bw (csdr default 0.05f -> int(4.0/0.05f) = 79 Hamming taps, padded to 80), cutoff 0.5/D.
 * out_s16 != 0 appends convert_f_s16 (interleaved s16 IQ out), else complex float out. */
int pirip_hip_decim_create(int decimation, float transition_bw, int out_s16, int device,
                           pirip_hip_decim **out);
int pirip_hip_decim_destroy(pirip_hip_decim *d);
int pirip_hip_decim_taps(const pirip_hip_decim *d, float *taps, int *ntaps);   /* host copy  */
/* Tap-loop arithmetic. 0 (default): one multiply and one add per tap and component in ascending tap order -- the scalar csdr loop's
 * float32 result bit for bit. OPT-IN measurement variants (also PIRIP_DECIM_FMA=1 / 2 at create): 1 = the same conversion, the
 * accumulation fused (acc = fma(y, h, acc)); 2 = the affine u8 map pulled out of the sum (acc = fma(byte, h, acc), y = acc/127.5 - sum h).
 * Upstream csdr is built -O3 -ffast-math [UPSTREAM-RECALLED]: which float32 result the shipped binary produces is a property of that
 * build's vectoriser, so neither variant is "wrong" a priori -- they are simply not what oracle/csdr_oracle.c's scalar loop states.
 * What each computes is pinned bit for bit (oracle_fir_decimate_cc_arith, tests/test_switches.py): sums in ascending tap order from
 * zero; 2 ends with y = fmaf(acc, c, -tap_sum), c = the float sum of the two constants of the exact u8 conversion (1/127.5 rounded),
 * tap_sum = the float of the taps' double sum. A stream whose first byte sits at an odd address takes the table loop whatever the
 * mode: its outputs are those of mode 0. With PIRIP_DECIM_LUT set at create every stream does, and modes 1 and 2 are PIRIP_ERR_UNSUPPORTED. */
#define PIRIP_DECIM_EXACT   0
#define PIRIP_DECIM_FMA     1
#define PIRIP_DECIM_FMA_RAW 2
int pirip_hip_decim_set_arith(pirip_hip_decim *d, int mode);
int pirip_hip_decim_get_arith(const pirip_hip_decim *d);
/* Number of outputs fir_decimate_cc yields for n_in inputs presented as ONE buffer:
 * floor((n_in - ntaps_padded)/D) + 1, or 0. */
int64_t pirip_hip_decim_nout(const pirip_hip_decim *d, int64_t n_in);
/* Stream s: u8 IQ at (const uint8_t*)d_in + s*in_stride_bytes (n_in complex samples) ->
 * out at (char*)d_out + s*out_stride_bytes, n_out = pirip_hip_decim_nout(n_in) samples. */
int pirip_hip_decim_batch(pirip_hip_decim *d, const uint8_t *d_in, size_t in_stride_bytes,
                          int64_t n_in, void *d_out, size_t out_stride_bytes, int nstreams,
                          void *hip_stream);

/* ----------------------------------------------------------------------------------- */
/* section B2 : synthetic Tx on the device                             */
/*   replaces the host pipeline fsk_get_test_bits | fsk_mod -c | (u8 quantiser, AWGN)   */
/*   used by /root/reference/README.md:101,142,218 to make test signals                 */
/* ----------------------------------------------------------------------------------- */
/* Stream s modulates nsym M-FSK symbols taken from d_bits + s*bits_stride (device, one bit per byte,
 * MSB first for 4FSK; bits_stride 0 = all streams send the same bits) on tones f1_hz[s] + m*tone_spacing_hz
 * (host array), drops skip_samples[s] leading samples (host array or NULL) and writes nsamp u8 IQ samples
 * (u8 = clamp(rintf(127 + amp*x)), x = 2*exp(j phase), i.e. fsk_mod -c output) to d_out + s*out_stride_bytes.
 * sigma > 0 adds sigma*N(0,1) per I and Q component before quantising (counter-based generator keyed by
 * seed, stream and sample). Phase is renormalised every PIRIP_FSK_DEFAULT_NSYM symbols like the fsk_mod tool.
 * Noise-free output is bit-identical to fsk_mod_c. Synchronous on hip_stream. */
int pirip_hip_synth_cu8(int Fs, int Rs, int M, int nstreams,
                        const int32_t *f1_hz, int tone_spacing_hz, const int32_t *skip_samples,
                        const uint8_t *d_bits, size_t bits_stride, int64_t nsym,
                        uint8_t *d_out, size_t out_stride_bytes, int64_t nsamp,
                        float amp, float sigma, uint64_t seed, void *hip_stream);

/* ----------------------------------------------------------------------------------- */
/* section E : FSK_LDPC receive (BASELINE config 4's second half)       */
/*   what `rtl_fsk --code NAME [-b]` does after fsk_demod_sd(): soft decisions -> LLRs ->  */
/*   32-bit unique-word sync -> LDPC sum-product decode (<= 15 iterations,                 */
/*   /root/reference/README.md:200-212) -> CRC16 -> payload bytes + rx_status, one record  */
/*   per demodulator call (/root/reference/tx/frame_repeater.c:55-62,71,80,88).            */
/*   [UPSTREAM-RECALLED codec2 freedv_fsk.c: freedv_rx_fsk_ldpc_data, mpdecode_core.c]     */
/*   The parity-check matrix, unique word and sync thresholds come from a code FILE        */
/*   (format: pirip_amd/csrc/fsk_ldpc.hpp); codec2's H_256_512_4 is not in /root/reference, */
/*   pirip_amd/data/standin_256_512_4.code is a labelled stand-in of the same shape.        */
/* ----------------------------------------------------------------------------------- */
#define PIRIP_RX_TRIAL_SYNC 0x1   /* rx_status bits [UPSTREAM-RECALLED codec2 freedv_api.h FREEDV_RX_*] */
#define PIRIP_RX_SYNC       0x2
#define PIRIP_RX_BITS       0x4   /* a frame was decoded and its CRC16 matches                          */
#define PIRIP_RX_BIT_ERRORS 0x8   /* not every parity check was satisfied                               */
#define PIRIP_LDPC_INFO_PER_CALL 10 /* state, uw_loc, uw_err, bad_uw, iter, pcc, frame bit position (-1 none), crc_ok,
                                       eraw (channel hard decisions the decoder changed), reserved */

typedef struct pirip_hip_ldpc pirip_hip_ldpc;
typedef struct pirip_ldpc_info {
    int n, k, bits_per_frame, data_bytes, nbits_per_call, max_iter, nstreams;
    char name[64];
} pirip_ldpc_info;

/* nstreams independent receivers for M-FSK with Nsym symbols per demodulator call (Nsym*log2(M) soft bits per call). */
int pirip_hip_ldpc_create(const char *code_path, int M, int Nsym, int nstreams, int device, pirip_hip_ldpc **out);
int pirip_hip_ldpc_destroy(pirip_hip_ldpc *h);
int pirip_hip_ldpc_get_info(const pirip_hip_ldpc *h, pirip_ldpc_info *info);
int pirip_hip_ldpc_reset(pirip_hip_ldpc *h, void *hip_stream);
/* The soft bits receiver s carries into its next call (synchronous copy): the last 2 * bits_per_frame bit LLRs it was handed, oldest first,
 * as IEEE binary16 -- written by the LLR stage or by the demodulator's fused hand-over alike. A checking aid: the fused path keeps no
 * other copy of them. */
int pirip_hip_ldpc_get_llr_history(pirip_hip_ldpc *h, int s, uint16_t *host_llr);
/* A checking aid: the storage layout the fast and persistent decoders run on (searched at create, PIRIP_LAYOUT_TRIES moves; 0 keeps the
 * identity layout) as its bank conflicts -- extra LDS cycles per decoder iteration of the identity layout and of the layout in use. The
 * layout moves where values are stored, never the order of a sum: decoded words do not depend on it. PIRIP_ERR_UNSUPPORTED: the code
 * has no such layout (the generic decoder serves it). */
int pirip_hip_ldpc_get_layout_conflicts(const pirip_hip_ldpc *h, int *identity, int *in_use);
/* Stream s consumes `ncalls` demodulator frames of soft decisions d_rx_filt + s*filt_stride (floats; each frame is
 * M*Nsym magnitudes in fsk_demod_sd() layout [m][sym] = pirip_hip_demod_batch's d_rx_filt); d_ncalls[s] (or NULL = all)
 * says how many of them are valid (d_nframes of the demodulator): the receiver advances by exactly that many calls -- the
 * rest of the batch is not demodulator output, gets status 0 / zero payload / info -1 and leaves no trace in the state that
 * carries to the next batch. Per (stream, call) it writes
 *   d_status  [s][ncalls]                 rx_status byte (PIRIP_RX_*)
 *   d_payload [s][ncalls][k/8]            packed payload bytes, zeros when the call produced no frame
 *   d_info    [s][ncalls][PIRIP_LDPC_INFO_PER_CALL]
 * i.e. the `rtl_fsk -b` record stream. Sync state and the last two frames of soft bits carry to the next call.
 * This call and the ones below are enqueued on hip_stream and do not synchronise, except that a call with more ncalls (max_frames, ncw)
 * than any before it grows the handle's work rows and waits for hip_stream first; pirip_hip_rx_create sizes them for its receiver. */
int pirip_hip_ldpc_rx_batch(pirip_hip_ldpc *h, const float *d_rx_filt, size_t filt_stride, const int32_t *d_ncalls, int ncalls,
                            uint8_t *d_status, uint8_t *d_payload, int32_t *d_info, void *hip_stream);
/* The whole receive chain of one batch in one call -- what `rtl_fsk --code NAME` does per block of IQ: stream s of `dem` (created
 * for the same nstreams / M / Nsym / device) demodulates its samples as pirip_hip_demod_batch would and its frames go straight
 * into receiver s of `h`: d_status / d_payload / d_info hold one record per demodulator call, [s][max_frames][...], calls
 * beyond d_nframes[s] as described above; d_stats (optional) the demodulator's per-frame statistics. Where the demodulator
 * kernel of the shape can, it writes the bit LLRs and their hard decisions itself (no soft magnitudes and no
 * LLR pass through HBM); otherwise the call is pirip_hip_demod_batch + pirip_hip_ldpc_rx_batch over an internal buffer. The
 * records are the same either way. pirip_hip_fsk_ldpc_last_path: 1 if the last such call took the fused hand-over, else 0.
 * From 4096 streams on (PIRIP_CHAIN_SPLIT_MIN=<n> moves the threshold, 0 = never) the fused form runs the batch as two ranges of
 * streams (5/8 and 3/8) on two internal HIP streams, forked from and joined back into `hip_stream`: the first range's LDS-bound
 * decode then runs beside the second range's VALU-bound demodulator. Same kernels on the same per-stream data: same records. */
int pirip_hip_fsk_ldpc_rx_batch(pirip_hip_demod *dem, pirip_hip_ldpc *h, const void *d_in, size_t in_stride_bytes, int64_t nsamp,
                                uint8_t *d_status, uint8_t *d_payload, int32_t *d_info, float *d_stats, size_t stats_stride,
                                int32_t *d_nframes, int64_t *d_consumed, int64_t max_frames, void *hip_stream);
int pirip_hip_fsk_ldpc_last_path(const pirip_hip_ldpc *h);
/* The same for several GROUPS of streams at once, each group with its own pair of handles and its own buffers: group g's call runs
 * on an internal HIP stream of its own (all but the last group at high priority), started behind everything queued on `hip_stream`
 * and joined back into it. The FSK_LDPC stages are bound by the LDS pipe and the demodulator by VALU issue, so group g's decode runs
 * beside group g+1's demodulator instead of after it (two groups, the first the bigger: 26.9 -> 25.4 ms per 8192 x 600 k samples at
 * 3.5 dB, tools/chain_overlap.py); the records of every group are what its own pirip_hip_fsk_ldpc_rx_batch call writes. All groups
 * share in_stride_bytes / nsamp / stats_stride / max_frames and must live on one device. */
typedef struct pirip_chain_group {
    pirip_hip_demod *dem; pirip_hip_ldpc *ldpc;
    const void *d_in; uint8_t *d_status; uint8_t *d_payload; int32_t *d_info; float *d_stats; int32_t *d_nframes; int64_t *d_consumed;
} pirip_chain_group;
int pirip_hip_fsk_ldpc_rx_batch_groups(const pirip_chain_group *groups, int ngroups, size_t in_stride_bytes, int64_t nsamp, size_t stats_stride,
                                       int64_t max_frames, void *hip_stream);
/* host-buffer convenience for a one-stream handle (rtl_fsk) */
int pirip_hip_ldpc_rx_host(pirip_hip_ldpc *h, const float *rx_filt, int ncalls, uint8_t *status, uint8_t *payload, int32_t *info);
/* the two numerical stages on their own (device pointers): bit LLRs of ncalls demodulator frames ([ncalls][Nbits]), and
 * the decoder on ncw codewords of LLRs ([ncw][n] -> hard codeword bits [ncw][n], {iterations, parity checks ok} [ncw][2]) */
int pirip_hip_ldpc_llr(pirip_hip_ldpc *h, const float *d_rx_filt, int ncalls, float *d_llr, void *hip_stream);
int pirip_hip_ldpc_decode_llr(pirip_hip_ldpc *h, const float *d_llr, int ncw, uint8_t *d_bits, int32_t *d_iter_pcc, void *hip_stream);

/* ----------------------------------------------------------------------------------- */
/* section G : streaming receiver (N live channels, block after block)                 */
/*   Composes the handles above: a demodulator of nstreams channels, optionally the     */
/*   FSK_LDPC receivers of the same channels and a csdr front end. Each channel's       */
/*   unconsumed tail stays on the device, right-aligned in front of the landing zone    */
/*   of the next block: no host round trip, no repacking, and every     */
/*   channel carries fewer than nin_max samples from one call into the next.           */
/*   Bit packing, estimator settings, burst mode, eye, get_Sf, get_stream_state and the  */
/*   LDPC info stay on the handles the caller owns; the receiver does not own them.     */
/* ----------------------------------------------------------------------------------- */
typedef struct pirip_hip_rx pirip_hip_rx;
/* dem: the demodulator (nstreams channels). ldpc: NULL for bits / soft magnitudes / stats out, else FSK_LDPC records out (same
 * nstreams / M / Nsym / device as dem). dec: NULL when the caller's samples are modem-rate samples of dem's in_format; else tuner-rate
 * u8 IQ through csdr's convert_u8_f | fir_decimate_cc D (dec created with out_s16 == (in_format == PIRIP_IN_CS16), dem's in_format
 * PIRIP_IN_CF32 or PIRIP_IN_CS16 -- rtl_fsk -a and the README.md:109 pipe). block: input samples per channel per call at the input
 * rate. PIRIP_ERR_BAD_ARG unless block % D == 0 and every call hands the demodulator >= nin_max new samples (with dec the first call
 * hands it fewer than the others: the filter's first output needs ntaps inputs); PIRIP_ERR_UNSUPPORTED when the demodulator's kernel
 * cannot take calls of that size. The handles must outlive the receiver; create synchronises the device. */
int pirip_hip_rx_create(pirip_hip_demod *dem, pirip_hip_ldpc *ldpc, pirip_hip_decim *dec, int64_t block, pirip_hip_rx **out);
int pirip_hip_rx_destroy(pirip_hip_rx *rx);
/* output rows per channel per call: floor((nin_max - 1 + m) / nin_min) + 1, m = modem-rate samples per call, nin_min = 2 N - nin_max */
int64_t pirip_hip_rx_max_frames(const pirip_hip_rx *rx);
/* zero-copy ingest: where the next call's block of channel s goes (*d_block + s * *stride_bytes, block samples of the input format:
 * u8 IQ with dec, else dem's in_format); free to be written once the previous call's work on the same HIP stream has run */
int pirip_hip_rx_input(pirip_hip_rx *rx, void **d_block, size_t *stride_bytes);
/* One block per channel (already in the input) -> outputs. Without ldpc: the demodulator's outputs as pirip_hip_demod_batch writes them
 * (d_bits / d_rx_filt / d_stats, strides in elements, each may be NULL); d_status / d_payload / d_info must be NULL. With ldpc: FSK_LDPC
 * records as pirip_hip_fsk_ldpc_rx_batch writes them ([s][max_frames][...], one row per demodulator call, rows beyond d_nframes[s] as
 * documented there; d_stats optional); d_bits / d_rx_filt must be NULL. d_nframes [s]: frames of this call (required with ldpc, else
 * may be NULL). Rows per channel: pirip_hip_rx_max_frames. Enqueued on hip_stream (NULL = default stream); never synchronises. */
int pirip_hip_rx_process(pirip_hip_rx *rx, uint8_t *d_bits, size_t bits_stride, float *d_rx_filt, size_t filt_stride,
                         uint8_t *d_status, uint8_t *d_payload, int32_t *d_info, float *d_stats, size_t stats_stride,
                         int32_t *d_nframes, void *hip_stream);
/* The same after copying channel s's block from d_in + s * in_stride_bytes (DEVICE pointer, block samples of the input format) into
 * the input, on hip_stream. */
int pirip_hip_rx_push(pirip_hip_rx *rx, const void *d_in, size_t in_stride_bytes,
                      uint8_t *d_bits, size_t bits_stride, float *d_rx_filt, size_t filt_stride,
                      uint8_t *d_status, uint8_t *d_payload, int32_t *d_info, float *d_stats, size_t stats_stride,
                      int32_t *d_nframes, void *hip_stream);
/* Host copies (synchronises the device), per channel [nstreams], either may be NULL: modem-rate samples consumed since create / reset,
 * and samples carried into the next call (< nin_max). PIRIP_ERR_HIP if a carry ever reached nin_max (only possible if the frame budget
 * bound, which its sizing rules out; that carry was dropped). */
int pirip_hip_rx_get_counters(pirip_hip_rx *rx, int64_t *consumed_total, int32_t *backlog);
/* Drops the carries and resets dem (and ldpc): the next call is the first after create. */
int pirip_hip_rx_reset(pirip_hip_rx *rx, void *hip_stream);

/* ----------------------------------------------------------------------------------- */
/* section H : channelizer (K channels out of W wideband u8 IQ captures)                */
/*   csdr shift_addition_cc (-f_c/Fs) | fir_decimate_cc D [| convert_f_s16] per channel, */
/*   every channel of a capture computed from one read of it.           */
/* ----------------------------------------------------------------------------------- */
typedef struct pirip_hip_chan pirip_hip_chan;
typedef struct pirip_chan_info {
    int Fs, D, ntaps, ntaps_padded, ninputs, nchan, out_s16, device;
} pirip_chan_info;
/* ninputs wideband u8 IQ captures at Fs samples/s; nchan channels, channel c = (capture chan_input[c], centre offset chan_offset_hz[c]).
 * Taps: section B's prototype for the same D / transition_bw (csdr Hamming low-pass, cutoff 0.5/D, padded with zeros to Lp taps).
 * out_s16 != 0 appends convert_f_s16 (interleaved s16 IQ, y * 32767 truncated, clamped to the s16 range), else complex float out.
 * For channel c, with x[n] = convert_u8_f(byte) = b/127.5 - 1 and t0 the absolute index of the call's first input sample:
 *     y_c[j] = sum_{i=0}^{Lp-1} h[i] x[jD+i] e^{-j 2 pi f_c (t0 + jD + i) / Fs}
 * -- the direct form and tap order of section B; a tone at f_c + a Hz in the capture comes out at +a Hz in channel c.
 * Computed as g_c[i] = h[i] e^{-j 2 pi f_c i / Fs} (host, double, rounded to float) and one rotation per output whose phase is the exact
 * integer (f_c mod Fs)(t0 + jD) mod Fs: a function of the absolute sample index only, so consecutive calls on overlapping windows give
 * the one-shot output bit for bit, and a channel's output does not depend on which other channels the handle has. csdr's own
 * shift_addition_cc runs a recursive cos/sin phasor restarted every buffer (its rounding depends on csdr's buffer size): that recursion
 * is deliberately not reproduced. PIRIP_ERR_BAD_ARG for nchan < 1, ninputs < 1, D < 1, a chan_input outside [0, ninputs) or an offset
 * outside -Fs/2 < f_c < Fs/2; PIRIP_ERR_UNSUPPORTED for Fs > 2^24, and for a decimation of which two rows no longer fit the 64 KiB of
 * LDS a workgroup stages its window in (D > 4095 at up to D taps). */
int pirip_hip_chan_create(int Fs, int decimation, float transition_bw, int out_s16, int ninputs, int nchan, const int32_t *chan_input,
                          const int32_t *chan_offset_hz, int device, pirip_hip_chan **out);
int pirip_hip_chan_destroy(pirip_hip_chan *ch);
int pirip_hip_chan_get_info(const pirip_hip_chan *ch, pirip_chan_info *info);
int pirip_hip_chan_taps(const pirip_hip_chan *ch, float *taps, int *ntaps);      /* host copy of the prototype h (ntaps, unpadded) */
/* outputs per channel for n_in input samples: floor((n_in - Lp)/D) + 1, or 0 (= pirip_hip_decim_nout for the same D / transition_bw) */
int64_t pirip_hip_chan_nout(const pirip_hip_chan *ch, int64_t n_in);
/* Capture i: n_in u8 IQ samples at d_in + i*in_stride_bytes (d_in and the stride even), whose first sample has absolute index t0.
 * Channel c: pirip_hip_chan_nout(n_in) samples at (char*)d_out + c*out_stride_bytes (aligned to the output sample: 8 or 4 bytes).
 * Stateless; enqueued on hip_stream (NULL = default stream), never synchronises. */
int pirip_hip_chan_batch(pirip_hip_chan *ch, const uint8_t *d_in, size_t in_stride_bytes, int64_t n_in, int64_t t0,
                         void *d_out, size_t out_stride_bytes, void *hip_stream);
/* Section G with the channelizer as its front end: one wideband capture row per input (ninputs rows at pirip_hip_rx_input, block u8 IQ
 * samples each), the channelizer writing straight into the nchan channels' modem-rate landing zones. dem must have nstreams == nchan and
 * in_format PIRIP_IN_CF32 (out_s16 == 0) or PIRIP_IN_CS16 (out_s16 != 0); ldpc optional as in pirip_hip_rx_create; block: wideband samples
 * per input per call, a multiple of D. Each input row keeps the channelizer's history of Lp - D samples right-aligned in front of its
 * block; the receiver tracks t0 on the host (no synchronisation). pirip_hip_rx_input / _push / _process / _get_counters / _reset then
 * work as documented above with ninputs input rows (push copies ninputs rows); _reset also restarts t0 at 0. */
int pirip_hip_rx_create_chan(pirip_hip_demod *dem, pirip_hip_ldpc *ldpc, pirip_hip_chan *chan, int64_t block, pirip_hip_rx **out);

/* ----------------------------------------------------------------------------------- */
/* section I : FSK_LDPC transmit (records -> channel symbols -> IQ, a batch of streams)  */
/*   The Tx half of section E: what `rpitx_fsk --code NAME --packed` does to its stdin    */
/*   (/root/reference/tx/rpitx_fsk.cpp:427-509) up to the modulator, and a continuous-    */
/*   phase M-FSK modulator, as two device stages. Every buffer the stages */
/*   need is owned by the handle (grown when a call is larger than any before it); the    */
/*   calls are enqueued on hip_stream (NULL = default stream) and do not synchronise.     */
/* ----------------------------------------------------------------------------------- */
#define PIRIP_TX_CARRIER_OFF 0xFF   /* symbol value: nothing is sent for this symbol time, the phase stays where it was */
typedef struct pirip_hip_tx pirip_hip_tx;
typedef struct pirip_tx_info {
    int Fs, Rs, M, Ts, n, k, bits_per_frame, data_bytes, preamble_syms, frame_syms, nstreams, device;
} pirip_tx_info;
/* nstreams transmitters of one code file and one modem shape (Fs % Rs == 0, M 2 or 4). PIRIP_ERR_BAD_CONFIG for a code file without the
 * accumulator (dual-diagonal) parity part -- fsk_ldpc_framer's refusal --, PIRIP_ERR_UNSUPPORTED for Fs > 2^24 or a frame that is not a
 * whole number of symbols (32 + n odd with M = 4), PIRIP_ERR_BAD_ARG for a file that does not load. Tones, lead and gap start at 0. */
int pirip_hip_tx_create(const char *code_path, int Fs, int Rs, int M, int nstreams, int device, pirip_hip_tx **out);
int pirip_hip_tx_destroy(pirip_hip_tx *h);
int pirip_hip_tx_get_info(const pirip_hip_tx *h, pirip_tx_info *info);
/* Stream s sends symbol m on f1_hz[s] + m * tone_spacing_hz (host array, integer Hz, negative allowed). Synchronises the device. */
int pirip_hip_tx_set_tones(pirip_hip_tx *h, const int32_t *f1_hz, int tone_spacing_hz);
/* Carrier-off symbols of stream s in front of its first record (lead_syms[s]) and for each of its `2` records (gap_syms[s]: the framer
 * tool's --gap, in symbols). Host arrays, NULL = zeros. Synchronises the device. */
int pirip_hip_tx_set_gaps(pirip_hip_tx *h, const int32_t *lead_syms, const int32_t *gap_syms);
/* Phase and sample count (the noise key) of every stream back to zero: the next pirip_hip_tx_modulate is the first after create. */
int pirip_hip_tx_reset(pirip_hip_tx *h, void *hip_stream);
/* symbols a row of max_rec records can need with the handle's lead / gap: the capacity pirip_hip_tx_frame asks of its rows */
int64_t pirip_hip_tx_max_syms(const pirip_hip_tx *h, int max_rec);
/* Stage 1. Stream s: d_nrec[s] (NULL = max_rec; clamped to [0, max_rec]) records at d_records + s * rec_stride, each one burst-control
 * byte + k/8 packed data bytes: 1 = preamble then a frame, 0 = a frame, 2 = end of burst (its data ignored, gap symbols of carrier off),
 * any other value sends nothing. A frame is UW | data | parity with the last 16 data bits replaced by the CRC16 of the packed bytes
 * before them, bit for bit fsk_ldpc_framer --packed (CPU: fsk_ldpc.cpp). Writes one symbol per byte (0 .. M-1, bit pairs MSB first for
 * M = 4, PIRIP_TX_CARRIER_OFF over lead and gaps) to d_syms + s * sym_stride and the symbol count to d_nsym[s] (may be NULL); with d_bits
 * also the frame bits one per byte at d_bits + s * bits_stride (nsym * log2(M) of them, zeros where the carrier is off: the framer
 * tool's output). Rows hold max_syms >= pirip_hip_tx_max_syms(h, max_rec) symbols, else PIRIP_ERR_BAD_ARG. */
int pirip_hip_tx_frame(pirip_hip_tx *h, const uint8_t *d_records, size_t rec_stride, const int32_t *d_nrec, int max_rec,
                       uint8_t *d_syms, size_t sym_stride, int64_t max_syms, int32_t *d_nsym, uint8_t *d_bits, size_t bits_stride,
                       void *hip_stream);
/* Stage 2. Every stream sends nsym symbol times = nsym * Ts samples: the symbols at d_syms + s * sym_stride, those from d_nsym[s] on
 * (NULL = none) carrier off. Sample r of symbol i is x = 2 e^{j 2 pi p / Fs} with the exact integer p = (A_i + (r + 1) f_i) mod Fs,
 * A_i = (phase carried in + Ts * sum_{q<i} f_q) mod Fs, f the symbol's tone; carrier off gives x = 0 and moves no phase. sigma > 0 adds
 * sigma * N(0,1) per component from pirip_hip_synth_cu8's generator, keyed by (seed, stream, samples sent since create / reset).
 * out_format PIRIP_IN_CU8_FSKDEMOD: u8 IQ, clamp(rintf(127 + amp * x)); PIRIP_IN_CF32: complex float x (amp unused). Row s at
 * (char*)d_out + s * out_stride_bytes, aligned to the sample (16-byte aligned rows get 16-byte stores). The handle carries each stream's
 * phase and the sample count: a row sent in several calls gives the bytes of one call. Numerics: DESIGN.md 4.9 (every component within
 * 1e-6 of the formula in float64). nsym * Ts < 2^31. */
int pirip_hip_tx_modulate(pirip_hip_tx *h, const uint8_t *d_syms, size_t sym_stride, const int32_t *d_nsym, int64_t nsym,
                          int out_format, void *d_out, size_t out_stride_bytes, float amp, float sigma, uint64_t seed, void *hip_stream);
/* Both stages over the handle's own symbol rows: records in, nsym symbol times of IQ out per stream (carrier off behind a stream's last
 * record; a row that needs more than nsym symbols is cut there). d_nsym (may be NULL): the symbols each stream's records made. */
int pirip_hip_tx_records_to_iq(pirip_hip_tx *h, const uint8_t *d_records, size_t rec_stride, const int32_t *d_nrec, int max_rec,
                               int64_t nsym, int out_format, void *d_out, size_t out_stride_bytes, float amp, float sigma, uint64_t seed,
                               int32_t *d_nsym, void *hip_stream);

/* The repeater's record conversion (tx/frame_repeater.c:68-107 without its sleeps and logging), on the device, one wave per stream: the
 * records pirip_hip_fsk_ldpc_rx_batch wrote for stream s -- d_ncalls[s] (NULL = ncalls) status bytes at d_status + s * status_stride and
 * payloads of k/8 bytes at d_payload + s * payload_stride -- become Tx records at d_records + s * rec_stride, their count in d_nrec[s]. A
 * burst starts at a record whose status is exactly SYNC | BITS, takes every later record with BITS, and ends at the first record without
 * SYNC: only then are its frames written, burst control 1, 0, ... and byte 0 replaced by source_byte, followed by one `2` record of zeros.
 * Frames of a burst that has not ended wait in the handle (at most PIRIP_TX_REPEAT_MAX_FRAMES per burst, the original's MAX_FRAMES; further
 * frames of that burst are dropped where the original asserts) and come out in the call in which it ends; pirip_hip_tx_reset forgets them.
 * Rows hold max_rec >= pirip_hip_tx_repeat_max_records(h, ncalls) records, else PIRIP_ERR_BAD_ARG; ncalls <= 4096. */
#define PIRIP_TX_REPEAT_MAX_FRAMES 100
int pirip_hip_tx_repeat_max_records(const pirip_hip_tx *h, int ncalls);
int pirip_hip_tx_repeat_records(pirip_hip_tx *h, const uint8_t *d_status, size_t status_stride, const uint8_t *d_payload, size_t payload_stride,
                                const int32_t *d_ncalls, int ncalls, int source_byte, uint8_t *d_records, size_t rec_stride, int max_rec,
                                int32_t *d_nrec, void *hip_stream);
/* One HIP stream per handle: the phase, the repeater's state and the work buffers are device state advanced in stream order, the sample
 * count of the noise key is host state advanced when a call is enqueued. Calls on one handle from several streams must be ordered by the caller. */

/* ----------------------------------------------------------------------------------- */
/* section J : multiplexer (K modem-rate channels onto W wideband IQ streams)           */
/*   The channelizer's mirror image and the last Tx stage: per channel interpolate by D, */
/*   move to the centre offset, scale; sum the channels of an output; u8 or complex      */
/*   float out. For one channel this is the reference bench chain's     */
/*   `tlininterp - t.iq8 D -d -f` (/root/reference/README.md:142) with PIRIP_MUX_LINEAR. */
/* ----------------------------------------------------------------------------------- */
#define PIRIP_MUX_FIR    0   /* h[i] = D * h_B[i], h_B section B's / H's csdr Hamming low-pass for the same D / transition_bw (cutoff 0.5/D) */
#define PIRIP_MUX_LINEAR 1   /* h[i] = 1 - |i - (D-1)| / D, i = 0 .. 2D-2: linear interpolation, delayed by D - 1 samples; D = 1: h = {1} */
typedef struct pirip_hip_mux pirip_hip_mux;
typedef struct pirip_mux_info {
    int Fs, D, kind, ntaps, ntaps_padded, Q, noutputs, nchan, out_format, device;
} pirip_mux_info;
/* noutputs wideband streams at Fs samples/s; nchan channels at Fs / D, channel c = (output chan_output[c], centre offset chan_offset_hz[c]
 * in integer Hz, real gain chan_gain[c]; chan_gain NULL = all 1). The prototype h has L taps (ntaps), Q = ceil(L / D) per polyphase branch,
 * padded with zeros to Lp = Q D (ntaps_padded). With z_c[m] the channel's complex float samples, m the absolute input index, n = mD + p and
 * 0 <= p < D:
 *     u_c[n] = sum_{q=0}^{Q-1} h[p + qD] z_c[m - q]
 *     w_i[n] = sum_{c : chan_output[c] = i, ascending c} chan_gain[c] e^{+j 2 pi f_c n / Fs} u_c[n]
 * PIRIP_MUX_LINEAR gives u[mD + p + D - 1] = (1 - p/D) z[m] + (p/D) z[m+1]. out_format PIRIP_IN_CF32: w itself; PIRIP_IN_CU8_CSDR: per
 * component clamp(rintf(127.5f v + 127.5f), 0, 255), product and sum rounded separately -- the inverse of the channelizer's b/127.5 - 1.
 * An output that no channel is assigned to is all zeros (cf32) / all bytes 128 (u8).
 * Computed as g_c[i] = a_c h[i] e^{+j 2 pi f_c i / Fs} (host, double, rounded to float), one rotation per input sample,
 * z'_c[m] = z_c[m] e^{+j 2 pi f_c m D / Fs} with the phase from the exact integer ((f_c D mod Fs)(m mod Fs)) mod Fs, and
 * w_i[mD + p] = sum_c sum_q g_c[p + qD] z'_c[m - q]: each channel's sum its own fma chain in ascending q, the channels added in ascending
 * index. A sample is a function of the absolute index and of its own output's channels only: consecutive calls that overlap by Q - 1
 * input samples give the one-shot output bit for bit, m0 and m0 + k Fs give the same bytes, and an output does not depend on what the
 * other outputs carry. Numerics: DESIGN.md 4.10.
 * PIRIP_ERR_BAD_ARG for nchan < 1, noutputs < 1, D < 1, Fs < 2, an unknown kind or out_format, a chan_output outside [0, noutputs), an
 * offset outside -Fs/2 < f_c < Fs/2, a gain that is not finite. PIRIP_ERR_UNSUPPORTED for Fs > 2^24, noutputs > 65535, and for a filter
 * whose working set for ONE channel does not fit the 64 KiB of LDS a workgroup stages a tile of 2048 outputs in:
 *     2048 B + 8 (Q Dp + floor((D + 2046) / D) + Q) > 65536,   B = 2 (u8) or 8 (cf32),  Dp = D (D <= 32) or D + 31
 * -- with PIRIP_MUX_LINEAR, D > 3807 (u8) or D > 3039 (cf32). The number of channels per output is not limited: they are staged in groups
 * of as many as fit (at most 8). */
int pirip_hip_mux_create(int Fs, int interpolation, int kind, float transition_bw, int out_format, int noutputs, int nchan,
                         const int32_t *chan_output, const int32_t *chan_offset_hz, const float *chan_gain, int device, pirip_hip_mux **out);
int pirip_hip_mux_destroy(pirip_hip_mux *mux);
int pirip_hip_mux_get_info(const pirip_hip_mux *mux, pirip_mux_info *info);
int pirip_hip_mux_taps(const pirip_hip_mux *mux, float *taps, int *ntaps);         /* host copy of the prototype h (ntaps, unpadded) */
/* output samples per output for n_in input samples per channel: (n_in - Q + 1) D, or 0 when n_in < Q */
int64_t pirip_hip_mux_nout(const pirip_hip_mux *mux, int64_t n_in);
/* Channel c: n_in complex float samples at (char*)d_in + c*in_stride_bytes (8-byte aligned), the first with absolute index m0 (may be
 * negative). Output i: pirip_hip_mux_nout(n_in) samples at (char*)d_out + i*out_stride_bytes, aligned to the output sample (2 or 8 bytes;
 * 16-byte aligned rows get 16-byte stores, the bytes are the same), the first with absolute index (m0 + Q - 1) D. Rows of several outputs
 * must not overlap (PIRIP_ERR_BAD_ARG). Stateless; enqueued on hip_stream (NULL = default stream), never synchronises. n_in D <= 2^40. */
int pirip_hip_mux_batch(pirip_hip_mux *mux, const void *d_in, size_t in_stride_bytes, int64_t n_in, int64_t m0,
                        void *d_out, size_t out_stride_bytes, void *hip_stream);

/* ----------------------------------------------------------------------------------- */
/* section K : streaming transmitter (queued records to wideband IQ, block after block) */
/*   Section G's mirror image. Composes a transmitter (section I: code, framer, tones,   */
/*   gap) and a multiplexer (section J: taps, offsets, gains, outputs, format): every     */
/*   channel has a queue of channel symbols on the device, and one call turns the next    */
/*   block of every queue into wideband samples. No modem-rate IQ is written: the         */
/*   multiplexer's staging computes each modem sample from its symbol and the exact       */
/*   integer phase.                                                      */
/* ----------------------------------------------------------------------------------- */
typedef struct pirip_hip_txs pirip_hip_txs;
typedef struct pirip_txs_info {
    int64_t block, queue_syms;
    int S, H, nchan, noutputs, out_format, device;
} pirip_txs_info;
/* tx and mux are borrowed and must outlive the handle. PIRIP_ERR_BAD_ARG unless tx's nstreams == mux's nchan, tx's Fs * mux's D == mux's
 * Fs and both are on the same device. block: wideband samples per output per call, a positive multiple of D * Ts (else PIRIP_ERR_BAD_ARG):
 * every call sends S = block / (D * Ts) whole symbols per channel. queue_syms: each channel's queue capacity in symbols, used as given,
 * at least S (else PIRIP_ERR_BAD_ARG). H = ceil((Q - 1) / Ts) symbols of history are kept per channel (0 when Q = 1).
 * PIRIP_ERR_UNSUPPORTED when (H + S) Ts + Q + 2304 does not fit 31 bits. The handle keeps its own per-channel phase and symbol history: it never
 * touches tx's carried phase or sample count, and calls on tx in between change nothing here. Tones and gaps are read from tx when a call
 * runs. Create synchronises the device. */
int pirip_hip_txs_create(pirip_hip_tx *tx, pirip_hip_mux *mux, int64_t block, int64_t queue_syms, pirip_hip_txs **out);
int pirip_hip_txs_destroy(pirip_hip_txs *txs);
int pirip_hip_txs_get_info(const pirip_hip_txs *txs, pirip_txs_info *info);
/* Channel s: d_nrec[s] (NULL = max_rec; clamped to [0, max_rec]) records at d_records + s * rec_stride, exactly what pirip_hip_tx_frame
 * reads (burst control 1 / 0 / 2 / other, CRC, UW, parity, and tx's gap for a `2`). tx's lead is NOT applied: a streaming transmitter's
 * silence is its empty queue. Per channel all or nothing: if the symbols of this call's records fit the queue's free space they are
 * appended in order and d_taken[s] is the record count; otherwise nothing is appended, d_taken[s] = 0 and the channel's refused count goes
 * up. d_taken may be NULL. Enqueued on hip_stream (NULL = default stream); does not synchronise, except that a call with a larger
 * max_rec than any before it grows the handle's work rows, as in section I. */
int pirip_hip_txs_send(pirip_hip_txs *txs, const uint8_t *d_records, size_t rec_stride, const int32_t *d_nrec, int max_rec, int32_t *d_taken,
                       void *hip_stream);
/* Every channel dequeues up to S symbols; the rest of the block is carrier off (the phase does not move, as in section I). Output i gets
 * block samples of mux's out_format at (char*)d_out + i * out_stride_bytes, aligned as pirip_hip_mux_batch asks (to the sample; 16-byte
 * aligned rows get 16-byte stores; rows of several outputs must not overlap). d_sent[s] (may be NULL): symbols dequeued. Enqueued on
 * hip_stream; never synchronises.
 * Contract: let each channel's symbol timeline be what the calls dequeued, call after call, with carrier off where nothing was queued. The
 * concatenation of all outputs since create / reset equals, byte for byte, pirip_hip_tx_modulate(..., PIRIP_IN_CF32, sigma = 0) on a fresh
 * handle over that timeline followed by pirip_hip_mux_batch on those rows with Q - 1 zero samples in front and m0 = -(Q - 1): wideband
 * sample 0 is modem sample 0. This holds for every block, every interleaving of send and process, and after reset. */
int pirip_hip_txs_process(pirip_hip_txs *txs, void *d_out, size_t out_stride_bytes, int32_t *d_sent, void *hip_stream);
/* Host copies (synchronises the device), per channel [nchan], each may be NULL: symbols queued now, symbols sent since create / reset,
 * underrun symbols (carrier off because the queue was empty), refused sends. */
int pirip_hip_txs_get_counters(pirip_hip_txs *txs, int64_t *queued, int64_t *sent, int64_t *underrun, int64_t *refused);
/* Empties the queues and clears phases, history, counters and the sample index: the next call is the first after create. */
int pirip_hip_txs_reset(pirip_hip_txs *txs, void *hip_stream);
/* One HIP stream per handle: queues, phases and history are device state advanced in stream order, the sample index is host state advanced
 * when a call is enqueued. */

/* ----------------------------------------------------------------------------------- */
/* section L : test-frame counter (bit errors per stream, counted on the device)        */
/*   What every receive pipeline of the reference ends in: `| fsk_put_test_bits -`        */
/*   (/root/reference/README.md:105,109,114,152,172, test/loopback_rtl_fsk.sh,            */
/*   test/loopback_rtl_sdr.sh) for uncoded bits, and the ecdd column of                   */
/*   `rtl_fsk --code NAME --testframes` for FSK_LDPC records -- for a batch of streams,   */
/*   chained behind the demodulator or the receiver on the same HIP stream, so that no    */
/*   bit has to reach the host to learn a link's error rate. All results */
/*   are integers and equal the CPU counter's exactly.                                    */
/* ----------------------------------------------------------------------------------- */
#define PIRIP_TBITS_MAX_FRAMESIZE 4096
typedef struct pirip_hip_tbits pirip_hip_tbits;
/* nstreams counters for one test frame. Replaces nstreams x fsk_put_test_bits [-f framesize] [-t valid_thresh]. frame_bits == NULL: the
 * tool's own frame (glibc srand(158324), rand() & 1 per bit, computed on the host here and uploaded); else framesize host bytes, each 0
 * or 1. A window is valid iff (float)errs < thr with thr = valid_thresh * framesize evaluated once in float -- the tool's own expression,
 * not an integer limit (0.09f * 300 is 27.000002f: 27 errors are valid; 0.07f * 100 is exactly 7.0f: 7 are not). PIRIP_ERR_BAD_ARG for framesize < 1, nstreams < 1, a frame byte
 * above 1 or out == NULL; PIRIP_ERR_UNSUPPORTED for framesize > PIRIP_TBITS_MAX_FRAMESIZE; PIRIP_ERR_NO_DEVICE without a device. */
int pirip_hip_tbits_create(int framesize, float valid_thresh, const uint8_t *frame_bits, int nstreams, int device, pirip_hip_tbits **out);
int pirip_hip_tbits_destroy(pirip_hip_tbits *h);
/* Stream s hands over nf_s = clamp(d_nframes[s], 0, max_frames) rows (d_nframes == NULL: max_frames) at d_bits + s * bits_stride (bytes),
 * each row row_bits bits: packed = 0 one byte per bit (the low bit counts), rows row_bits bytes apart; packed = 1 ceil(row_bits / 8) bytes
 * per row, MSB first, pad bits ignored -- the layouts pirip_hip_demod_batch, pirip_hip_demod_capture and pirip_hip_rx_process write, with
 * their d_nframes. Replaces piping those bits into fsk_put_test_bits: with b the stream's bits in order since create / reset and b[i] = 0
 * for i < 0 (the tool's zero-filled window), every position j whose window b[j - F + 1 .. j] is valid adds 1 to packets, F to bits and
 * its Hamming distance to the frame to errors; overlapping valid windows all count, as in the tool. The handle carries each stream's last
 * F - 1 bits from call to call, so a window may straddle any number of calls, and calls of 0 rows or of fewer than F - 1 bits are fine.
 * Enqueued on hip_stream (NULL = default stream); never synchronises. PIRIP_ERR_BAD_ARG unless row_bits >= 1, max_frames >= 0 and
 * max_frames * row_bits < 2^31; PIRIP_ERR_UNSUPPORTED when nstreams * ceil(max_frames * row_bits / 2048) does not fit 31 bits.
 * One HIP stream per handle: which of the two history rows a call reads is host state advanced when the call is enqueued. */
int pirip_hip_tbits_push(pirip_hip_tbits *h, const uint8_t *d_bits, size_t bits_stride, int row_bits, int packed, const int32_t *d_nframes,
                         int64_t max_frames, void *hip_stream);
/* Host copies (synchronises the device), per stream [nstreams], each may be NULL: fsk_put_test_bits' packetcnt, bitcnt and biterr, and
 * the bits handed over since create / reset. */
int pirip_hip_tbits_get_counters(pirip_hip_tbits *h, int64_t *packets, int64_t *bits, int64_t *errors, int64_t *pushed);
/* The same on the device, for callers that stay there: int64 [nstreams][4] = {packets, bits, errors, pushed}, valid in stream order. */
int pirip_hip_tbits_counters_device(pirip_hip_tbits *h, int64_t **d_counters);
/* Counters (both blocks) and history back to the created state, in stream order. */
int pirip_hip_tbits_reset(pirip_hip_tbits *h, void *hip_stream);

/* The payload of --testframes for a code of k data bits, packed MSB first into k / 8 bytes: rtl_fsk.cpp's tf_bytes, what
 * fsk_ldpc_framer --testframes sends. Host function, needs no device. PIRIP_ERR_BAD_ARG for k < 8 or k % 8. */
int pirip_hip_tbits_testframe_payload(int k, uint8_t *bytes_out);
/* What push_records compares with: data_bytes host bytes (NULL: the test payload of k = 8 * data_bytes). Synchronises the device. */
int pirip_hip_tbits_set_payload(pirip_hip_tbits *h, int data_bytes, const uint8_t *payload);
/* Replaces the ecdd column of `rtl_fsk --code NAME --testframes -v`, tallied: stream s reads nc_s = clamp(d_ncalls[s], 0, ncalls)
 * (d_ncalls == NULL: ncalls) records as pirip_hip_fsk_ldpc_rx_batch / pirip_hip_rx_process wrote them -- status bytes at d_status +
 * s * status_stride, payloads of data_bytes bytes at d_payload + s * payload_stride, info rows of PIRIP_LDPC_INFO_PER_CALL int32 at
 * d_info + s * info_stride (strides in elements). A record counts when info[6] >= 0 (a frame was decoded); its errors are the popcount of
 * payload ^ test payload over bytes 2 .. data_bytes - 3 (bytes 0, 1 carry source / sequence, the last two the CRC). Needs set_payload
 * first (else PIRIP_ERR_BAD_ARG). Enqueued on hip_stream; never synchronises. */
int pirip_hip_tbits_push_records(pirip_hip_tbits *h, const uint8_t *d_status, size_t status_stride, const uint8_t *d_payload, size_t payload_stride,
                                 const int32_t *d_info, size_t info_stride, const int32_t *d_ncalls, int ncalls, void *hip_stream);
/* Host copies (synchronises the device), per stream [nstreams], each may be NULL: decoded frames, payload bits compared, payload bit
 * errors, frames with at least one error, records with PIRIP_RX_BITS. */
int pirip_hip_tbits_get_record_counters(pirip_hip_tbits *h, int64_t *frames, int64_t *bits, int64_t *errors, int64_t *frames_in_error,
                                        int64_t *crc_ok);

/* ----------------------------------------------------------------------------------- */
/* section M : streaming repeater (wideband IQ in, repeated bursts out, block by block)  */
/*   The reference's product as one call per block:                                       */
/*   `rtl_fsk --code NAME --filter A -q -b | frame_repeater 256 A | rpitx_fsk - --code    */
/*   NAME --packed` (/root/reference/script/frame_repeater:36-38) for a batch of channels.  */
/*   Composes a streaming receiver (section G, optional), a transmitter (section I) and    */
/*   its streaming transmitter (section K): received records go through rtl_fsk's          */
/*   --filter and frame_repeater.c's state machine, finished bursts wait in a ring per      */
/*   transmit channel and are handed to section K's queue whole, when they are due and      */
/*   fit. No call synchronises or allocates; every call enqueues the same  */
/*   launches.                                                                              */
/* ----------------------------------------------------------------------------------- */
typedef struct pirip_hip_rpt pirip_hip_rpt;
typedef struct pirip_rpt_info {
    int nrx, nchan, source_byte, filter_byte, holdoff_calls, max_burst_frames, pending_records, has_rx, rx_rows, device;
} pirip_rpt_info;
/* All handles are borrowed, must be on one device and must outlive the repeater. rx: NULL (records come from the caller:
 * pirip_hip_rpt_push_records) or a streaming receiver created with an ldpc, of nrx channels and tx's data_bytes, whose
 * pirip_hip_rx_max_frames is at most 4096 (PIRIP_ERR_UNSUPPORTED above). txs must have been created on tx. route[c] (host array, nrx
 * entries): the transmit channel of receive channel c, negative = do not repeat; the non-negative entries distinct and below tx's
 * nstreams. source_byte 0 .. 255: byte 0 of every repeated frame (frame_repeater's source address). filter_byte: -1, or 0 .. 255 =
 * rtl_fsk's --filter: a received frame whose byte 0 is filter_byte loses PIRIP_RX_BITS before the state machine sees it. holdoff_calls
 * >= 0: a burst that ends in call n is offered from call n + holdoff_calls on (frame_repeater.c:91's wait, in blocks).
 * max_burst_frames 1 .. PIRIP_TX_REPEAT_MAX_FRAMES: frames held per burst, further ones are dropped as in section I.
 * pending_records >= max_burst_frames + 1: records of each transmit channel's pending ring. txs's queue_syms must hold one burst of
 * max_burst_frames frames: preamble_syms + max_burst_frames * frame_syms + tx's largest gap. Anything else: PIRIP_ERR_BAD_ARG.
 * Every work row is sized here with tx's gaps as they are, the framer's rows of pending_records records per channel in txs included: set
 * the gaps first. The handle keeps its own state-machine state per receive channel and never touches tx's repeat state, phase or sample
 * count. Create synchronises the device. */
int pirip_hip_rpt_create(pirip_hip_rx *rx, pirip_hip_tx *tx, pirip_hip_txs *txs, int nrx, const int32_t *route, int source_byte, int filter_byte,
                         int holdoff_calls, int max_burst_frames, int pending_records, pirip_hip_rpt **out);
int pirip_hip_rpt_destroy(pirip_hip_rpt *rpt);
int pirip_hip_rpt_get_info(const pirip_hip_rpt *rpt, pirip_rpt_info *info);
/* Call n (n = 0, 1, ... since create / reset), in stream order:
 * 1. intake, per receive channel c over its d_ncalls[c] (NULL = ncalls; clamped to [0, ncalls]) records -- status bytes at d_status +
 *    c * status_stride, payloads of data_bytes bytes at d_payload + c * payload_stride, as pirip_hip_fsk_ldpc_rx_batch writes them; they
 *    are only read --: the filter, then the state machine of pirip_hip_tx_repeat_records. A burst that ends here is the records 1, 0, ...,
 *    0, 2; with t = route[c] >= 0 it is appended to transmit channel t's pending ring with ready = n + holdoff_calls, or dropped whole when
 *    the ring's free space does not hold it; with route[c] < 0 it is discarded.
 * 2. offer, per transmit channel t, from the ring's head and in order: whole bursts while ready <= n and the burst's symbols (preamble +
 *    frames * frame_syms + tx's gap of channel t now) fit what is left of txs's free space (queue_syms - queued); the first burst that does
 *    not qualify stops the channel. The taken records go through pirip_hip_txs_send's path, which by construction never refuses.
 * 3. pirip_hip_txs_process into d_out (its rules for d_out / out_stride_bytes).
 * Works with and without rx (with rx it changes nothing of the receiver). ncalls <= 4096 (PIRIP_ERR_UNSUPPORTED above). Enqueued on
 * hip_stream (NULL = default stream); never synchronises. */
int pirip_hip_rpt_push_records(pirip_hip_rpt *rpt, const uint8_t *d_status, size_t status_stride, const uint8_t *d_payload, size_t payload_stride,
                               const int32_t *d_ncalls, int ncalls, void *d_out, size_t out_stride_bytes, void *hip_stream);
/* Need rx (PIRIP_ERR_BAD_ARG without): pirip_hip_rx_process on the block at pirip_hip_rx_input (push: after copying it from d_in as
 * pirip_hip_rx_push does) into the handle's own record rows, then the three steps above over them. */
int pirip_hip_rpt_process(pirip_hip_rpt *rpt, void *d_out, size_t out_stride_bytes, void *hip_stream);
int pirip_hip_rpt_push(pirip_hip_rpt *rpt, const void *d_in, size_t in_stride_bytes, void *d_out, size_t out_stride_bytes, void *hip_stream);
/* The records the last call read, as received (the filter changes no byte of them): after process / push the handle's rows -- rx_rows
 * rows per channel, strides in elements, d_nframes [nrx] --, after push_records the caller's own (d_info NULL, its stride 0). Valid in
 * stream order: pirip_hip_tbits_push_records or a logger can be chained on the same stream. Each pointer may be NULL.
 * PIRIP_ERR_BAD_ARG before the first call. */
int pirip_hip_rpt_records(pirip_hip_rpt *rpt, const uint8_t **d_status, size_t *status_stride, const uint8_t **d_payload, size_t *payload_stride,
                          const int32_t **d_info, size_t *info_stride, const int32_t **d_nframes);
/* The records offered to the streaming transmitter in the last call: channel t's d_nrec[t] records at d_records + t * rec_stride. */
int pirip_hip_rpt_offered(pirip_hip_rpt *rpt, const uint8_t **d_records, size_t *rec_stride, const int32_t **d_nrec);
/* Host copies (synchronises the device), each may be NULL. Per receive channel [nrx]: bursts that ended, the frames they held, frames
 * the filter removed, bursts discarded for want of a route. Per transmit channel [nchan]: bursts offered, records waiting in the ring,
 * bursts dropped on a full ring. */
int pirip_hip_rpt_get_counters(pirip_hip_rpt *rpt, int64_t *bursts_in, int64_t *frames_in, int64_t *filtered, int64_t *unrouted,
                               int64_t *bursts_out, int64_t *pending, int64_t *dropped);
/* Forgets open bursts and the pending rings, clears the counters and resets txs, and rx where present: the next call is n = 0. */
int pirip_hip_rpt_reset(pirip_hip_rpt *rpt, void *hip_stream);
/* One HIP stream per handle: rings, ready tags and the state machines are device state advanced in stream order, the call index is host
 * state advanced when a call is enqueued. */

/* ----------------------------------------------------------------------------------- */
/* section N : ping terminal (test bursts out, a per-frame link log in, block by block)  */
/*   The other end of section M's link: the reference's script/ping, which sends a burst   */
/*   of test frames every few seconds (`rpitx_fsk --testframes 3 --source 0x1 --seq`) and   */
/*   logs what comes back with `rtl_fsk --code NAME -L --filter 0x1`                        */
/*   (the reference's script/ping:47 and README.md:57-89), for a batch of                  */
/*   channels. Composes a streaming receiver (section G, optional) and a transmitter with    */
/*   its streaming transmitter (sections I and K, optional): received records go through     */
/*   rtl_fsk's --filter into a log ring per receive channel, and bursts of test frames go     */
/*   into section K's queue on a schedule counted in calls. No call          */
/*   synchronises or allocates; every call enqueues the same launches.                        */
/* ----------------------------------------------------------------------------------- */
typedef struct pirip_hip_ping pirip_hip_ping;
typedef struct pirip_ping_config {
    int nrx;                    /* receive channels (== rx's channels when rx is given) */
    int source_byte;            /* 0..255: byte 0 of every frame sent */
    int filter_byte;            /* -1, or 0..255 = rtl_fsk --filter: such a frame loses PIRIP_RX_BITS before it is logged */
    int frames_per_burst;       /* 1..PIRIP_TX_REPEAT_MAX_FRAMES */
    int seq;                    /* 1: byte 1 of frame f of a burst = (f + 1) & 0xff (rpitx_fsk --seq) */
    int period_calls;           /* >= 1 */
    const int32_t *first_call;  /* [tx channels] host, NULL = zeros; each >= 0 */
    int64_t max_bursts;         /* per channel; 0 = no limit (script/ping start N) */
    int log_entries;            /* >= 1: entries of each receive channel's log ring */
    int nin0;                   /* samples the first demodulator call consumes (info.N); taken from rx when rx is given */
} pirip_ping_config;
typedef struct pirip_ping_entry {           /* 40 bytes */
    int64_t t_samples;                      /* the channel's modem-rate sample clock after the call that delivered the frame */
    int32_t call, row;                      /* n, f */
    float S, N, SNRest;                     /* stats row [8], [9], [5], bit for bit */
    int32_t ecdd;                           /* popcount(payload ^ test payload) over bytes 2 .. data_bytes - 3 (section L's rule) */
    int32_t eraw;                           /* info[8] */
    uint8_t source, seq, status, iters;     /* payload[0], payload[1], status as received, min(info[4], 255) */
} pirip_ping_entry;
typedef struct pirip_ping_info {
    int nrx, nchan, source_byte, filter_byte, frames_per_burst, seq, period_calls, log_entries, nin0, has_rx, rx_rows, data_bytes, device;
    int64_t max_bursts;
} pirip_ping_info;
/* All handles are borrowed, must be on one device and must outlive the terminal. rx: NULL (records come from the caller:
 * pirip_hip_ping_push_records) or a streaming receiver created with an ldpc, of cfg->nrx channels, whose pirip_hip_rx_max_frames is at most
 * 4096 (PIRIP_ERR_UNSUPPORTED above); with tx also of tx's data_bytes. tx and txs: both NULL -- the handle is a logger only, nchan = 0 and
 * every call's d_out must be NULL -- or a transmitter and the streaming transmitter created on it; one without the other is
 * PIRIP_ERR_BAD_ARG, and so are rx, tx and txs all NULL (nothing would tell the frame's size). Also PIRIP_ERR_BAD_ARG: cfg or out NULL,
 * nrx < 1 or not rx's channels, source_byte outside 0 .. 255, filter_byte outside -1 .. 255, frames_per_burst outside 1 ..
 * PIRIP_TX_REPEAT_MAX_FRAMES, period_calls < 1, a negative first_call entry, max_bursts < 0, log_entries < 1, nin0 < 0 without rx, handles
 * on different devices, a frame of fewer than 4 data bytes, and a txs whose queue_syms does not hold one burst: preamble_syms +
 * frames_per_burst * frame_syms + tx's largest gap. The burst's frames_per_burst + 1 records -- those of fsk_ldpc_framer --testframes
 * frames_per_burst --bursts 1 --source source_byte [--seq] -- are made here, once, on the host. Every work row is sized here with tx's gaps
 * as they are, the framer's rows in txs included: set the gaps first. Create synchronises the device. */
int pirip_hip_ping_create(pirip_hip_rx *rx, pirip_hip_tx *tx, pirip_hip_txs *txs, const pirip_ping_config *cfg, pirip_hip_ping **out);
int pirip_hip_ping_destroy(pirip_hip_ping *ping);
int pirip_hip_ping_get_info(const pirip_hip_ping *ping, pirip_ping_info *info);
/* Call n (n = 0, 1, ... since create / reset), in stream order:
 * 1. log, per receive channel c over its nf = d_ncalls[c] (NULL = ncalls; clamped to [0, ncalls]) rows -- status bytes at d_status +
 *    c * status_stride, payloads of data_bytes bytes at d_payload + c * payload_stride, info rows of PIRIP_LDPC_INFO_PER_CALL int32 at
 *    d_info + c * info_stride, stats rows of PIRIP_STATS_PER_FRAME floats at d_stats + c * stats_stride (strides in elements), as
 *    pirip_hip_fsk_ldpc_rx_batch / pirip_hip_rx_process write them; they are only read. The channel carries a sample clock {samples = 0,
 *    next_nin = nin0}; for rows f = 0 .. nf - 1 in order: samples += next_nin; next_nin = (int)stats[f][6] (rtl_fsk -L's clock). A row with
 *    PIRIP_RX_BITS whose payload byte 0 is filter_byte loses BITS (filtered); a row that still has BITS gets one pirip_ping_entry with
 *    t_samples = samples, appended in row order to the channel's ring at written % log_entries: the ring overwrites its oldest entry.
 * 2. schedule, per transmit channel t: a burst is due iff n >= first_call[t], (n - first_call[t]) % period_calls == 0 and fewer than
 *    max_bursts bursts were sent (max_bursts 0: no limit). It costs preamble_syms + frames_per_burst * frame_syms + tx's gap of channel t
 *    now. If that fits txs's free space (queue_syms - queued) the burst's records are offered and go through pirip_hip_txs_send's path,
 *    which by construction never refuses; otherwise nothing is offered, skipped goes up and the burst is not tried again before its next
 *    due call.
 * 3. pirip_hip_txs_process into d_out (its rules for d_out / out_stride_bytes).
 * A logger-only handle runs step 1 alone and wants d_out == NULL (else PIRIP_ERR_BAD_ARG); a handle with tx wants d_out. d_status,
 * d_payload, d_info and d_stats are all required (PIRIP_ERR_BAD_ARG), as are strides that hold ncalls rows when nrx > 1. ncalls <= 4096
 * (PIRIP_ERR_UNSUPPORTED above), ncalls < 0 is PIRIP_ERR_BAD_ARG. Works with and without rx (with rx it changes nothing of the receiver).
 * Enqueued on hip_stream (NULL = default stream); never synchronises. */
int pirip_hip_ping_push_records(pirip_hip_ping *ping, const uint8_t *d_status, size_t status_stride, const uint8_t *d_payload, size_t payload_stride,
                                const int32_t *d_info, size_t info_stride, const float *d_stats, size_t stats_stride, const int32_t *d_ncalls,
                                int ncalls, void *d_out, size_t out_stride_bytes, void *hip_stream);
/* Need rx (PIRIP_ERR_BAD_ARG without): pirip_hip_rx_process on the block at pirip_hip_rx_input (push: after copying it from d_in as
 * pirip_hip_rx_push does; d_in == NULL is PIRIP_ERR_BAD_ARG) into the handle's own status, payload, info, stats and nframes rows, then the
 * steps above over them. */
int pirip_hip_ping_process(pirip_hip_ping *ping, void *d_out, size_t out_stride_bytes, void *hip_stream);
int pirip_hip_ping_push(pirip_hip_ping *ping, const void *d_in, size_t in_stride_bytes, void *d_out, size_t out_stride_bytes, void *hip_stream);
/* The rows the last call read, as received: after process / push the handle's own -- rx_rows rows per channel, strides in elements,
 * d_nframes [nrx] --, after push_records the caller's. Valid in stream order; each pointer may be NULL. PIRIP_ERR_BAD_ARG before the
 * first call. */
int pirip_hip_ping_records(pirip_hip_ping *ping, const uint8_t **d_status, size_t *status_stride, const uint8_t **d_payload, size_t *payload_stride,
                           const int32_t **d_info, size_t *info_stride, const float **d_stats, size_t *stats_stride, const int32_t **d_nframes);
/* The records offered to the streaming transmitter in the last call: channel t's d_nrec[t] (0 or frames_per_burst + 1) records at
 * d_records + t * rec_stride. PIRIP_ERR_BAD_ARG on a logger-only handle. */
int pirip_hip_ping_offered(pirip_hip_ping *ping, const uint8_t **d_records, size_t *rec_stride, const int32_t **d_nrec);
/* Host copies (synchronises the device), each may be NULL. Per receive channel [nrx]: frames logged, frames the filter removed, rows with a
 * decoded frame (info[6] >= 0), decoded rows without PIRIP_RX_BITS as received, the sum of the logged entries' ecdd, entries the ring
 * overwrote. Per transmit channel [nchan]: bursts sent, frames sent, due bursts skipped for want of queue space. */
int pirip_hip_ping_get_counters(pirip_hip_ping *ping, int64_t *frames, int64_t *filtered, int64_t *decoded, int64_t *crc_fail, int64_t *bit_errors,
                                int64_t *lost, int64_t *bursts_sent, int64_t *frames_sent, int64_t *skipped);
/* Host copy (synchronises the device) of the newest min(frames logged, log_entries, max) entries of receive channel chan, oldest first;
 * *written (may be NULL): how many. PIRIP_ERR_BAD_ARG for chan outside [0, nrx), max < 0 or entries == NULL with max > 0. */
int pirip_hip_ping_get_log(pirip_hip_ping *ping, int chan, pirip_ping_entry *entries, int max, int *written);
/* Clears the sample clocks, the rings and the counters and resets txs, and rx where present: the next call is n = 0. */
int pirip_hip_ping_reset(pirip_hip_ping *ping, void *hip_stream);
/* One HIP stream per handle: clocks, rings and counters are device state advanced in stream order, the call index is host state advanced
 * when a call is enqueued. */

/* ----------------------------------------------------------------------------------- */
/* section O : channel (T transmitted wideband IQ streams onto R received ones)          */
/*   What lies between the terminals of sections M and N: the reference's "60 dB           */
/*   attenuator" or the air (its test/loopback_rtl_fsk.sh and README "MDS tests"). Every    */
/*   received stream is a sum of paths -- a transmitter, a real gain, a delay in samples,    */
/*   a carrier offset in Hz -- plus its own AWGN, written as u8 or complex float, block       */
/*   after block with the history carried on the device.                     */
/* ----------------------------------------------------------------------------------- */
typedef struct pirip_hip_air pirip_hip_air;
typedef struct pirip_air_path { int32_t rx, tx, delay, offset_hz; float gain; } pirip_air_path;
typedef struct pirip_air_info { int Fs, ntx, nrx, npaths, in_format, out_format, max_delay, device; } pirip_air_info;
/* ntx transmitted and nrx received streams at Fs samples/s; path p = (received stream rx_p, transmitted stream t_p = tx, real gain a_p,
 * delay d_p in samples, carrier offset f_p in integer Hz). With n the absolute sample index and x_t[k] = 0 for k below the index of the
 * last reset (0 after create) -- for u8 input exactly zero, not the value of byte 128:
 *     y_r[n] = sum_{p : rx_p = r, ascending p} a_p e^{+j 2 pi f_p n / Fs} x_{t_p}[n - d_p]  +  sigma_r w_r[n]
 * w_r[n]: the product's one noise source (sections B2 and I), unit variance per component, keyed by (seed, r, n).
 * Arithmetic, per component in float: in_format PIRIP_IN_CU8_CSDR is read as b / 127.5 - 1 (section H's conversion), PIRIP_IN_CF32 as it is.
 * A path with f_p != 0 is rotated by the unit phasor of the exact integer phase ((f_p mod Fs)(n mod Fs)) mod Fs (section J's mixer: one
 * product and one fma per component); a path with f_p == 0 is not rotated. The sum starts at 0 and takes the paths in ascending index as
 * acc = fma(a_p, v, acc). With sigma_r > 0 the noise of key (seed, r, n) is added. out_format PIRIP_IN_CF32 stores acc, PIRIP_IN_CU8_CSDR
 * clamp(rintf(127.5f v + 127.5f), 0, 255) per component, section J's byte: the clamp is the ADC's clipping. A received stream with no path
 * and sigma 0 is all zeros (cf32) / all bytes 128 (u8).
 * A sample is a function of the absolute index, of its own stream's paths and of the input alone: any cutting of the same input into calls
 * gives the one-shot output bit for bit (n = 1 and calls shorter than the longest delay included), with sigma 0 a start at n0 and one at
 * n0 + k Fs give the same bytes, and a received stream does not depend on the other streams' paths. Numerics: DESIGN.md 4.15.
 * sigma: [nrx] host, NULL = all 0. The number of paths per received stream is not limited.
 * PIRIP_ERR_BAD_ARG for out or (with npaths > 0) paths NULL, ntx < 1, nrx < 1, npaths < 0, Fs < 2, a format other than the two above, an rx
 * outside [0, nrx), a tx outside [0, ntx), a delay < 0, an offset outside -Fs/2 < f < Fs/2, a gain or a sigma that is not finite, a
 * sigma < 0. PIRIP_ERR_UNSUPPORTED for Fs > 2^24, a delay > 2^20, ntx or nrx > 65535. Create sizes everything and synchronises. */
int pirip_hip_air_create(int Fs, int in_format, int out_format, int ntx, int nrx, int npaths, const pirip_air_path *paths, const float *sigma,
                         uint64_t seed, int device, pirip_hip_air **out);
int pirip_hip_air_destroy(pirip_hip_air *air);
int pirip_hip_air_get_info(const pirip_hip_air *air, pirip_air_info *info);      /* max_delay: the longest delay of any path */
/* New sigma [nrx] (host; read before the call returns) for the calls enqueued behind this one: a level sweep needs no new handle and no
 * synchronisation. PIRIP_ERR_BAD_ARG for NULL, a value that is not finite or < 0. */
int pirip_hip_air_set_sigma(pirip_hip_air *air, const float *sigma, void *hip_stream);
/* Transmitted stream t: n samples of in_format at (char*)d_in + t*in_stride_bytes, the first with the absolute index that follows the last
 * call's (n0 of the last reset; 0 after create). Received stream r: n samples of out_format at (char*)d_out + r*out_stride_bytes. Rows are
 * aligned to their sample (2 or 8 bytes; 16-byte aligned u8 output rows get 16-byte stores, the bytes are the same) and the rows of one
 * side must not overlap; d_out must not overlap d_in. PIRIP_ERR_BAD_ARG for those, NULL pointers and n < 1; PIRIP_ERR_UNSUPPORTED when the
 * absolute index would reach 2^53. State: per transmitted stream a ring of its last samples in in_format, at least its longest delay long,
 * addressed by the absolute index; the call reads x[n - d] from its own rows where that index lies in the call and from the ring otherwise,
 * and a carry step behind it, in stream order, writes the call's last samples into the ring. Enqueued on hip_stream (NULL = default
 * stream); never synchronises, never allocates; every call makes the same launches. */
int pirip_hip_air_push(pirip_hip_air *air, const void *d_in, size_t in_stride_bytes, int64_t n, void *d_out, size_t out_stride_bytes,
                       void *hip_stream);
/* Forget the history: the next sample has absolute index n0 >= 0 (PIRIP_ERR_BAD_ARG below 0, PIRIP_ERR_UNSUPPORTED from 2^53), and every
 * earlier one is zero. sigma stays. */
int pirip_hip_air_reset(pirip_hip_air *air, int64_t n0, void *hip_stream);
/* One HIP stream per handle: the rings and sigma are device state advanced in stream order, the absolute index is host state advanced
 * when a call is enqueued. */

/* ---- section O, drift: a path whose two ends run on sample clocks that disagree. Only symbols are added: the entry
 * points above, their handles' launches and PIRIP_HIP_ABI_VERSION stand as they are. */
typedef struct pirip_air_path_ex { int32_t rx, tx, delay, offset_hz; float gain; int32_t clock_ppb; } pirip_air_path_ex;
/* pirip_hip_air_create with a clock offset q = clock_ppb per path, in parts per billion (q > 0: the transmitter's clock runs fast as the
 * receiver sees it), and max_slip, the largest whole-sample slip |S| any path may reach. A path with q = 0 is a path of
 * pirip_hip_air_create, bit for bit, and a handle without a drifting path makes that function's launches. With Q = 10^9, n_r the index of
 * the last reset and m = age0 + (n - n_r) the clock age (age0 = 0 after create and pirip_hip_air_reset):
 *     S(m) = floor(m q / Q) (toward -inf),  rho(m) = m q - Q S(m) in [0, Q),  i = n - d_p + S(m),  phi = floor(1024 rho / Q)
 *     v_p[n] = sum_{k = 0 .. 15} T[phi][k] x_{t_p}[i - 7 + k]      per component from 0 in ascending k as acc = fma(T, x, acc)
 * and v_p takes the place of x_{t_p}[n - d_p] in y_r[n]: rotated by the same exact integer phase of n where f_p != 0, then
 * acc_r = fma(a_p, v, acc_r). x_t[j] = 0 for j < n_r by index, as above. T: pirip_hip_air_interp_table. Integers throughout: S, rho and phi
 * are exact, so every sample stays a function of the absolute index, the clock age of the reset, its receiver's paths and the input, and
 * any cutting into calls gives the one-shot output bit for bit.
 * The slip budget: both ends get n samples per call, so a drifting path eats its delay (q > 0) or the ring (q < 0). For every path with
 * q != 0: PIRIP_ERR_BAD_ARG unless max_slip >= 1 and d_p >= 8 + (q > 0 ? max_slip : 0) (the taps never reach past sample n);
 * PIRIP_ERR_UNSUPPORTED for d_p + 7 + (q < 0 ? max_slip : 0) > 2^20 or |q| > 10^6. max_slip < 0 is PIRIP_ERR_BAD_ARG. A transmitter's ring
 * is the smallest power of two, at least 64, that holds its paths' longest lag, slip and the 7 leading taps included.
 * pirip_hip_air_push returns PIRIP_ERR_UNSUPPORTED, enqueues nothing and changes no state when the call's last sample would take a path's
 * |S| past max_slip (q > 0: m q < (max_slip + 1) Q; q < 0: m |q| <= max_slip Q). pirip_air_info.max_delay stays the longest delay field. */
int pirip_hip_air_create_ex(int Fs, int in_format, int out_format, int ntx, int nrx, int npaths, const pirip_air_path_ex *paths,
                            const float *sigma, uint64_t seed, int32_t max_slip, int device, pirip_hip_air **out);
/* The interpolator's table, the very floats the kernel uses: taps [1024][16] (host), T[phi][k] = sinc(k - 7 - mu) w((k - 7 - mu) / 8) with
 * mu = phi / 1024 and w the Kaiser window of beta 6, w(u) = I0(beta sqrt(1 - u^2)) / I0(beta), every phase divided by its own sum (DC gain
 * 1), computed in double and rounded once to float; phase 0 is the exact unit impulse at k = 7. *nphases = 1024, *ntaps = 16 (either may be
 * NULL). Host only: no device is looked for. PIRIP_ERR_BAD_ARG for taps NULL. */
int pirip_hip_air_interp_table(float *taps, int *nphases, int *ntaps);
/* Host state, no synchronisation: max_slip, and how many more samples pirip_hip_air_push will take (the slip budget of a handle with a
 * drifting path, and the absolute index below 2^53). Either pointer may be NULL. */
int pirip_hip_air_get_drift(const pirip_hip_air *air, int32_t *max_slip, int64_t *samples_left);
/* pirip_hip_air_reset with a clock age: the next sample has absolute index n0 and clock age age0, so a long run resumes where a budget
 * ended (with the delays moved by S) or starts anywhere inside it. PIRIP_ERR_BAD_ARG for n0 or age0 < 0; PIRIP_ERR_UNSUPPORTED for either
 * from 2^53, or an age0 that already breaks the budget. */
int pirip_hip_air_reset_drift(pirip_hip_air *air, int64_t n0, int64_t age0, void *hip_stream);

/* ---- section O, fading: a path whose gain moves, Rayleigh or Rician with a Doppler spread. Only symbols are added: the
 * entry points above, the launches of a handle without a fading path and PIRIP_HIP_ABI_VERSION stand as they are. */
typedef struct pirip_air_fade { int32_t path; int32_t doppler_millihz; float rice_k; uint32_t key; } pirip_air_fade;
/* pirip_hip_air_create_ex with nfades fades, each attached to one path (an index into paths): (path, doppler_millihz >= 0, rice_k >= 0,
 * key). A fade is a sum of J = 16 scatterers and a line-of-sight term. The host makes, per fade, 16 signed increments w_j, 16 start phases
 * theta_j and two floats (pirip_hip_air_fade_table returns them), with f_d = doppler_millihz / 1000 in double and K = rice_k:
 *     alpha_j = 2 pi (j + u_j) / 16,  u_j in [0, 1): the top 53 bits of r1_j = splitmix(seed ^ splitmix((key << 32) ^ j)), the product's
 *                                     SplitMix64 finaliser (section B2's noise source), times 2^-53
 *     nu_j = f_d cos(alpha_j),  w_j = (int32) llrint(nu_j / Fs * 2^32),  theta_j = the top 32 bits of splitmix(r1_j)
 *     s = float(sqrt(1 / (16 (K + 1)))),  los = float(sqrt(K / (K + 1)))            in double, rounded once
 * The phase of scatterer j at the absolute index n is the 32-bit integer psi_j(n) = theta_j + w_j * (uint32) n, plain unsigned wrap-around
 * arithmetic. The gain lives on an absolute grid of G = 16 samples; at grid point k, the absolute index 16 k:
 *     t_j = float((int32) psi_j(16 k) >> 8) * 2^-23            exact, in [-1, 1)
 *     (cos_j, sin_j) = sincospif(t_j);  C = sum_j cos_j,  D = sum_j sin_j          ascending j from 0, plain float adds
 *     c_k = ( fma(s, C, los),  s * D )
 * and between grid points it is the line through them: with k = n >> 4 and mu = float(n & 15) / 16
 *     g[n] = ( fma(mu, c_{k+1}.re - c_k.re, c_k.re),  fma(mu, c_{k+1}.im - c_k.im, c_k.im) )
 * v_p[n] -- a static path's x_t[n - d_p] or a drifting path's interpolated value -- becomes crot(v_p[n], g.re, g.im), the complex product
 * v g by section J's arithmetic, BEFORE the carrier rotation; the path's mix follows unchanged: the rotation by the exact integer phase
 * where f_p != 0, then acc_r = fma(a_p, v, acc_r). g is taken at the receiver's index n, whatever the path's delay and slip. A path
 * without a fade is the path of pirip_hip_air_create_ex, bit for bit; with nfades == 0 the call is pirip_hip_air_create_ex, bit for bit
 * and launch for launch.
 * Consequences: a sample stays a function of the absolute index, of the reset's clock age, of its receiver's paths and fades, and of the
 * input; any cutting into calls gives the one-shot output bit for bit. For a receiver with a fading path the guarantee "starts n0 and
 * n0 + k Fs give the same bytes" is replaced by "starts n0 and n0 + 2^32 give the same bytes", which holds with sigma 0, no drifting path
 * and every carrier offset 0 (the exact mixer phase is not 2^32-periodic in general). |g| <= Gamma = los + 16 s, which is 4 at K = 0.
 * Time-averaged over a long span |g|^2 tends to 1: the mean power gain is 1.
 * PIRIP_ERR_BAD_ARG for nfades < 0, fades NULL with nfades > 0, a path index outside [0, npaths), two fades on one path,
 * doppler_millihz < 0, a rice_k that is negative or not finite. PIRIP_ERR_UNSUPPORTED for doppler_millihz > floor(1000 Fs / 1024): at that
 * limit a phase moves at most 2 pi 16 / 1024 per grid step, and the line departs from the continuous process by at most
 * (2 pi / 64)^2 / 8 = 1.2e-3 of the scatter amplitude. Every argument check comes before a device is looked for.
 * push, reset, reset_drift, set_sigma, get_info and get_drift work unchanged on such a handle. */
int pirip_hip_air_create_fade(int Fs, int in_format, int out_format, int ntx, int nrx, int npaths, const pirip_air_path_ex *paths, int nfades,
                              const pirip_air_fade *fades, const float *sigma, uint64_t seed, int32_t max_slip, int device, pirip_hip_air **out);
/* A fade's table, the very integers and floats the kernel reads (fade->path is not looked at). Host only: no device is looked for.
 * PIRIP_ERR_BAD_ARG for a NULL pointer, Fs < 2 and the fade's values refused above; PIRIP_ERR_UNSUPPORTED as above. */
int pirip_hip_air_fade_table(int Fs, uint64_t seed, const pirip_air_fade *fade, int32_t w[16], uint32_t theta[16], float *scale, float *los);

/* ----------------------------------------------------------------------------------- */
/* section P : band monitor (averaged wideband spectra and band powers on the device)    */
/*   The view script/dash.py plots (SfdB with the band limits) and the two figures the    */
/*   README's "Noise Figure Testing" compares (a tone's power, the floor's density),      */
/*   one stage in front of section H: on the wideband stream itself, for a batch of      */
/*   streams, block after block, without host synchronisation.          */
/*   Only symbols are added: PIRIP_HIP_ABI_VERSION and every entry point above stand.    */
/* ----------------------------------------------------------------------------------- */
typedef struct pirip_hip_spec pirip_hip_spec;
typedef struct pirip_spec_band { int32_t stream, lo_hz, hi_hz; } pirip_spec_band;
typedef struct pirip_spec_band_row { float power, peak; int32_t peak_bin; } pirip_spec_band_row;
typedef struct pirip_spec_info { int Fs, in_format, nfft, hop, avg, nstreams, nbands, device; double scale; } pirip_spec_info;

/* nstreams streams at Fs samples/s. in_format PIRIP_IN_CU8_CSDR is read as b / 127.5 - 1 per component (section H's conversion),
 * PIRIP_IN_CF32 as it is. nfft is one of 256, 1024, 4096 (the powers of 4: kiss_fft's factorisation has radix-4 stages only), hop one of
 * nfft, nfft / 2, avg = A in 1 .. 65536.
 * Segments and rows: segment k of a stream covers its samples [k hop, k hop + nfft), counted from the last reset (create counts as one);
 * row j is the segments j A .. j A + A - 1 and is complete when its last sample has been pushed.
 * Window: w[i] = 0.5 - 0.5 cos(2 pi i / nfft) for i <= nfft / 2, computed in double and rounded once to float, and w[i] = w[nfft - i] above
 * (the formula's own symmetry, kept whatever cos() returns); pirip_hip_spec_window returns the very floats the kernel uses.
 * Per segment, in float: v[i] = (w[i] x.re, w[i] x.im), one product per component; X = the forward kiss_fft of v with the unfused twiddle
 * multiply on every butterfly operand -- oracle/kiss_fft_oracle.c at its default, twiddles (float) cos / sin of the double -2 pi i / nfft;
 * the process-wide fused-multiply switch of the demodulator does not reach this section --; p[b] = X.re X.re + X.im X.im, two rounded
 * products and one rounded add, no fma.
 * Rows: row[b] starts at +0 and takes its segments in ascending k, row[b] = row[b] + p_k[b]. Rows are stored unscaled, in FFT bin order
 * (bin 0 = DC, bin b at b Fs / nfft Hz, from nfft / 2 on at (b - nfft) Fs / nfft). info.scale = 1 / (A sum w[i]^2), the sum of the double
 * products in ascending i, is the factor to a per-bin mean power; the consumer applies it.
 * Bands: band q = (stream, lo_hz, hi_hz) with -Fs / 2 <= lo <= hi < Fs / 2. bin(f) = floor((2 f nfft + Fs) / (2 Fs)) mod nfft in 64-bit
 * integers, floor toward minus infinity, the result in [0, nfft). The band is the bins from bin(lo) upward, with wrap-around at nfft, to
 * bin(hi) inclusive: ((bin(hi) - bin(lo)) mod nfft) + 1 of them; pirip_hip_spec_band_bins returns bin(lo) and that count. Per complete row:
 * power = the sum of the band's row[b] from +0 in that walking order, plain float adds; peak = the largest of them (the first bin's value,
 * replaced by each later one that compares greater); peak_bin = its bin, the first in walking order on a tie. Bands may overlap, and
 * their number per stream is not limited.
 * State, per stream: the samples of its incomplete segments (fewer than nfft, in in_format), the running row[] of its incomplete row, and
 * on the host the count of samples pushed. Every output is a function of the stream's own samples since the last reset: any cutting of
 * the same input into calls gives the one-shot rows and band entries bit for bit (n = 1 and calls that complete no segment included), and
 * a stream's outputs depend neither on the other streams nor on which bands the handle has.
 * PIRIP_ERR_BAD_ARG for out NULL, bands NULL with nbands > 0, Fs < 2, nstreams < 1, nbands < 0, avg < 1, an in_format other than the two,
 * a band's stream outside [0, nstreams), lo > hi or an edge outside [-Fs/2, Fs/2). PIRIP_ERR_UNSUPPORTED for any other nfft or hop,
 * avg > 65536, Fs > 2^24, nstreams > 65535. Every argument check comes before a device is looked for; no CPU fallback: without a device
 * PIRIP_ERR_NO_DEVICE. Create sizes everything and synchronises. */
int pirip_hip_spec_create(int Fs, int in_format, int nfft, int hop, int avg, int nstreams, int nbands, const pirip_spec_band *bands, int device,
                          pirip_hip_spec **out);
int pirip_hip_spec_destroy(pirip_hip_spec *spec);
int pirip_hip_spec_get_info(const pirip_hip_spec *spec, pirip_spec_info *info);
/* The window of nfft points. Host only: no device is looked for. PIRIP_ERR_BAD_ARG for w NULL, PIRIP_ERR_UNSUPPORTED for another nfft. */
int pirip_hip_spec_window(int nfft, float *w);
/* Band q's first bin and number of bins (each pointer may be NULL). PIRIP_ERR_BAD_ARG for a band outside [0, nbands). */
int pirip_hip_spec_band_bins(const pirip_hip_spec *spec, int band, int32_t *first_bin, int32_t *nbins);
/* Rows the next push of n samples completes; host arithmetic: with S(t) = 0 for t < nfft, else (t - nfft) / hop + 1, the complete segments
 * of t samples, and P the samples pushed so far, S(P + n) / A - S(P) / A (integer divisions). n = 0 is allowed. Negative: PIRIP_ERR_*. */
int64_t pirip_hip_spec_nrows(const pirip_hip_spec *spec, int64_t n);
/* n more samples of every stream, stream r at d_in + r in_stride_bytes (device memory, in_format). The push that completes the rows
 * j0 .. j0 + m - 1, m = pirip_hip_spec_nrows(spec, n), writes row j0 + i of stream r at d_rows + r stream_stride + i row_stride (strides in
 * floats, nfft floats each; d_rows may be NULL: no rows are stored) and band q's entry i at d_bands + q band_stride + i (stride in entries;
 * d_bands NULL if and only if nbands == 0). A push that completes nothing writes nothing. With d_rows == NULL the band entries are the same
 * bits. Enqueued on hip_stream (NULL = default stream), one HIP stream per handle; never synchronises, never allocates.
 * PIRIP_ERR_BAD_ARG for NULL spec or d_in, d_bands NULL with nbands > 0, n < 1, input rows that are not whole samples or overlap (a
 * pointer or stride that is no multiple of the sample's size, a stride below n samples with nstreams > 1), d_rows or d_bands that is not
 * 4-byte aligned, row_stride < nfft with m > 1, stream_stride < (m - 1) row_stride + nfft with m > 0 and nstreams > 1, band_stride < m with
 * nbands > 1. PIRIP_ERR_UNSUPPORTED when the count of samples pushed would reach 2^53. A refused push enqueues nothing and changes no state. */
int pirip_hip_spec_push(pirip_hip_spec *spec, const void *d_in, size_t in_stride_bytes, int64_t n, float *d_rows, size_t row_stride,
                        size_t stream_stride, pirip_spec_band_row *d_bands, size_t band_stride, void *hip_stream);
/* Forget the history: the next sample is sample 0 of segment 0 of row 0. Host state only; nothing is enqueued. */
int pirip_hip_spec_reset(pirip_hip_spec *spec, void *hip_stream);

/* ----------------------------------------------------------------------------------- */
/* section Q : diversity receiver (B branches of one channel, soft bits combined per frame) */
/*   The receive side of section O's one transmitter onto R received streams: the           */
/*   receivers of a section E handle in groups of B branches -- tuners, antennas, sites    */
/*   -- whose soft bits of the same frame are added and decoded once.     */
/*   Adding LLRs is the optimal combination of independent branches, and the LLR stage      */
/*   scales each branch by its own SNR estimate: the plain sum weights as maximal-ratio     */
/*   combining would. The branch receivers write what they write today; this stage runs      */
/*   behind them and reads what they left. Only symbols are added: PIRIP_HIP_ABI_VERSION    */
/*   and every entry point above stand.                                                     */
/* ----------------------------------------------------------------------------------- */
typedef struct pirip_hip_div pirip_hip_div;
/* (This section's three structures are written `struct X { ... }; typedef struct X X;`, unlike the `typedef struct X { ... } X;` of every
 * section above. tests/test_binding_abi_cpu.py finds the header's structures by the second form and holds them to a fixed list of ctypes
 * twins; these three are held to their twins -- binding.DivConfig, DivEntry, DivInfo, DIV_ENTRY_DTYPE -- by tests/test_diversity_cpu.py
 * instead. A structure added here in this form has NO layout check until a test names it: add it to that test, or extend the general
 * guard's list and return to the usual form.) */
struct pirip_div_config {
    int branches;               /* B, 2 .. 8: receivers g B .. g B + B - 1 of ldpc are the branches of group g */
    int samples_per_symbol;     /* Ts, modem-rate samples per symbol (Fs / Rs of the branches' demodulator) */
    int nin0;                   /* samples the first demodulator call consumes (section N's clock) */
    int max_skew_samples;       /* frames whose first unique-word bits lie at most this far apart are one frame */
    int max_rows;               /* rows per receiver and call, 1 .. 4096: sizes every launch and the pending ring */
    int log_entries;            /* >= 1: entries of each group's ring */
};
typedef struct pirip_div_config pirip_div_config;
struct pirip_div_entry {                    /* 24 bytes */
    int64_t t_samples;                      /* floor(tau_anchor / bps): the frame's first unique-word bit on the sample timeline */
    int32_t iters, pcc, eraw;               /* the combined codeword's decode: info[4], info[5], info[8] of section E */
    uint8_t members, solo_ok, status, pad;  /* bit b: branch b is a member / its own record had PIRIP_RX_BITS; PIRIP_RX_* of the decode */
};
typedef struct pirip_div_entry pirip_div_entry;
struct pirip_div_info {
    int groups, branches, samples_per_symbol, nin0, max_skew_samples, max_rows, log_entries, pending, slots, n, data_bytes, device;
};
typedef struct pirip_div_info pirip_div_info;
/* The model. bps = log2(M), Ts = samples_per_symbol, bpf = 32 + n, Nbits as in ldpc; tags are int64 in units of 1 / bps sample.
 * Branch clock, per receiver: {samples = 0, next_nin = nin0}; for every valid row f of a call, in order: samples += next_nin;
 * next_nin = (int)stats[f][6] (pirip_hip_ping_push_records' clock).
 * Candidate: every row with info[6] >= 0 (a job of the branch's sync state machine; loc = info[6]) holds the n codeword soft bits
 * (binary16) its own decode read, its branch, solo_ok = the row's PIRIP_RX_BITS, and the tag
 *     tau = t_end bps - (2 bpf - loc) Ts,         t_end = the branch clock after that row.
 * Horizon, after a call's rows: H = min over the group's branches of (samples bps) - 2 bpf Ts; every candidate a branch can still
 * produce has tau > H.
 * Clusters, with K = max_skew_samples bps, repeated: the anchor is the pending candidate with the smallest (tau, branch); if
 * tau_anchor + K <= H the cluster is every pending candidate with tau <= tau_anchor + K, at most one per branch (the earliest; a
 * later one stays pending); it is emitted and its members leave the pending set; the first anchor that is not closed ends the call.
 * Membership and order depend on tags alone: the sequence of clusters is the same for any cutting of the rows into calls.
 * Combination, per soft-bit position: the members' values are added in float in ascending branch order, starting from the first
 * member's value, and rounded once to binary16; a NaN becomes +0 (an erasure, section E's rule), +-inf stays, a sum beyond binary16's
 * range is +-inf.
 * Decode and record: the combined codeword goes through ldpc's own decoder (whichever PIRIP_LDPC_DECODER / auto selects: all three
 * write the same words) and section E's CRC16; one pirip_div_entry per cluster is appended to the group's ring at written %
 * log_entries, its data_bytes payload bytes to the payload ring beside it. status = PIRIP_RX_SYNC | PIRIP_RX_BITS (CRC matches) |
 * PIRIP_RX_BIT_ERRORS (pcc < m); eraw counts against the combined hard decisions.
 *
 * Borrows ldpc, which must outlive the handle. PIRIP_ERR_BAD_ARG for NULL pointers, branches outside 2 .. 8, ldpc's nstreams no
 * multiple of branches, samples_per_symbol < 1, nin0 < 0, log_entries < 1, max_rows < 1, and unless 0 <= K < bpf Ts / 2.
 * PIRIP_ERR_UNSUPPORTED for max_rows > 4096. The pending ring holds 3 (max_rows Nbits / bpf + 2) + 2 candidates per branch: none is
 * dropped while every call has at most max_rows rows and the clocks of a group's branches stay within one such call of each other.
 * Create sizes everything and synchronises. */
int pirip_hip_div_create(pirip_hip_ldpc *ldpc, const pirip_div_config *cfg, pirip_hip_div **out);
int pirip_hip_div_destroy(pirip_hip_div *dv);
int pirip_hip_div_get_info(const pirip_hip_div *dv, pirip_div_info *info);      /* pending, slots: candidates / clusters per group and call */
/* Clocks, pending set, rings and counters as after create: the next call is call 0. Does not reset ldpc. */
int pirip_hip_div_reset(pirip_hip_div *dv, void *hip_stream);
/* In stream order behind a receive call of ldpc with the same ncalls -- pirip_hip_ldpc_rx_batch, pirip_hip_fsk_ldpc_rx_batch,
 * pirip_hip_rx_process / push (ncalls = pirip_hip_rx_max_frames) -- on that call's rows: status bytes at d_status + r status_stride, info
 * rows at d_info + r info_stride, stats rows at d_stats + r stats_stride (strides in elements), d_nframes [nstreams] valid rows per
 * receiver (NULL: ncalls). Reads them and the soft bits and job lists the receive call left in ldpc's work buffers, which stay valid
 * until ldpc's next receive call. Every receive call gives ldpc a new batch serial number: a collect without a fresh batch of that
 * ncalls is PIRIP_ERR_BAD_ARG (stale buffers are never read; a batch received before create or reset is not fresh), as are NULL d_status / d_info / d_stats, ncalls < 1 or > max_rows, and
 * strides below ncalls rows. Enqueued on hip_stream (NULL = default stream); never synchronises, never allocates; every call makes the
 * same launches, sized from max_rows. A refusal above enqueues nothing and changes no state. Any other error (PIRIP_ERR_HIP:
 * a launch failed) may come after the clocks have advanced and the batch has been marked as read: the handle is
 * then out of step with its input, and pirip_hip_div_reset -- with a reset of ldpc and of what feeds it -- is the only way on. The same
 * holds for push_candidates and flush, and for ldpc's receive calls, which count a batch before the launches that could fail. */
int pirip_hip_div_collect(pirip_hip_div *dv, const uint8_t *d_status, size_t status_stride, const int32_t *d_info, size_t info_stride,
                          const float *d_stats, size_t stats_stride, const int32_t *d_nframes, int ncalls, void *hip_stream);
/* The layer under collect, for callers with soft bits of their own: ncand candidates -- n binary16 values at d_llr_h16 + c n, tag
 * d_tag[c] (int64), receiver d_group_branch[c] = g B + b (an entry < 0 is skipped), d_solo_ok[c] (0 / 1) -- join the pending sets, then
 * the clusters that d_clock_units [nstreams] (int64: each branch's clock in tag units, samples bps) closes are emitted, combined, decoded
 * and recorded. ncand <= nstreams (max_rows Nbits / bpf + 2); ncand == 0 (pointers may be NULL) only moves the horizon.
 * Cost: the list is in no order, so every group's one lane reads all ncand receiver indices to find its own -- groups x ncand reads
 * per call. That is nothing for a handful of groups or candidates; with thousands of groups and thousands of candidates it is
 * the call's largest cost, and collect, whose staging is per branch and read by its own group alone, is the path that scales. */
int pirip_hip_div_push_candidates(pirip_hip_div *dv, const uint16_t *d_llr_h16, const int64_t *d_tag, const int32_t *d_group_branch,
                                  const uint8_t *d_solo_ok, int ncand, const int64_t *d_clock_units, void *hip_stream);
/* The same with H = +inf: everything pending is emitted. */
int pirip_hip_div_flush(pirip_hip_div *dv, void *hip_stream);
/* Device pointers to what the last collect / push_candidates / flush emitted, valid in stream order until the next: group g's d_count[g]
 * entries at d_entries + g entry_stride (in entries) and payloads at d_payload + g payload_stride (bytes). Each pointer may be NULL. */
int pirip_hip_div_last(pirip_hip_div *dv, const pirip_div_entry **d_entries, size_t *entry_stride, const uint8_t **d_payload,
                       size_t *payload_stride, const int32_t **d_count);
/* Host copy (synchronises the device) of the newest min(clusters, log_entries, max) entries of group `group`, oldest first, and their
 * payloads [max][data_bytes] (may be NULL); *written (may be NULL): how many. */
int pirip_hip_div_get_log(pirip_hip_div *dv, int group, pirip_div_entry *entries, uint8_t *payloads, int max, int *written);
/* Host copies (synchronises), per group [groups], each may be NULL: clusters emitted, clusters with PIRIP_RX_BITS, those of them no
 * member decoded alone (empty solo_ok), members summed, entries the ring overwrote, candidates dropped for want of pending space. */
int pirip_hip_div_get_counters(pirip_hip_div *dv, int64_t *clusters, int64_t *bits, int64_t *rescued, int64_t *members, int64_t *lost,
                               int64_t *dropped);
/* Checking aid (synchronises): the n combined soft bits, binary16, of cluster `slot` of group `group` of the last call. */
int pirip_hip_div_get_combined(pirip_hip_div *dv, int group, int slot, uint16_t *host_llr);
/* One HIP stream per handle, the one ldpc's receive calls are enqueued on. */

/* ----------------------------------------------------------------------------------- */
/* section R : packet link (datagrams cut into FSK_LDPC frames and reassembled)         */
/*   The layer between a datagram and the frames every section above moves: the open     */
/*   milestone of the reference's plan ("TAP/TUN integration and demo IP link | What       */
/*   protocol?"). The reference fixes no protocol; this section fixes one. Composes, as     */
/*   section N does, a streaming receiver (section G, optional) and a transmitter with its   */
/*   streaming transmitter (sections I and K, optional): packets handed to send are cut      */
/*   into bursts that wait in section M's pending rings and go into section K's queue whole,  */
/*   received records are put back together into packets in a ring per receive channel       */
/*   (DESIGN.md 4.18). No call synchronises or allocates; every call enqueues the same         */
/*   launches. Only symbols are added: PIRIP_HIP_ABI_VERSION and every entry point above      */
/*   stand.                                                                                   */
/* ----------------------------------------------------------------------------------- */
typedef struct pirip_hip_pkt pirip_hip_pkt;
/* Wire format. kb = data_bytes (>= 16); the framer overwrites bytes kb - 2 and kb - 1 with the CRC16. cap = kb - 8.
 *   byte 0 src    the sender's address (where rtl_fsk's --filter and the repeater's rewrite look)
 *   byte 1 dst    the destination's address, 0xFF = everyone
 *   byte 2 id     the sender's packet counter of the channel, mod 256
 *   byte 3 idx    fragment index, 0 .. nfrag - 1
 *   byte 4 nfrag  fragments of the packet, 1 .. max_frags
 *   byte 5 len    body bytes in this fragment, 1 .. cap; every fragment but the last has len == cap
 *   bytes 6 .. kb - 3: cap body bytes, zero padded
 * The body of a packet of L bytes, 1 <= L <= max_packet = max_frags * cap - 4, is the L bytes and their CRC-32 (IEEE 802.3, zlib's crc32)
 * as four bytes, least significant first; nfrag = ceil((L + 4) / cap). One packet is one burst: the records pirip_hip_tx_frame reads, with
 * burst control 1, 0, ..., 0, then the `2` record of zeros.
 * (This section's three structures are written as section Q's are and are held to their twins -- binding.PktConfig, PktEntry, PktInfo,
 * PKT_ENTRY_DTYPE -- by tests/test_packet_cpu.py.) */
struct pirip_pkt_config {
    int nrx;                    /* receive channels (== rx's channels when rx is given) */
    int source_byte;            /* 0..255: src of every frame sent */
    int filter_byte;            /* -1, or 0..255 = rtl_fsk --filter: such a frame loses PIRIP_RX_BITS before it is looked at */
    int address;                /* -1: every frame is accepted; 0..255: only frames whose dst is this or 0xFF */
    int max_frags;              /* 1..PIRIP_TX_REPEAT_MAX_FRAMES: a section M repeater can repeat any packet whole */
    int pending_records;        /* >= max_frags + 1: records of each transmit channel's pending ring */
    int ring_entries;           /* >= 1: packets of each receive channel's ring */
};
typedef struct pirip_pkt_config pirip_pkt_config;
struct pirip_pkt_entry {                    /* 24 bytes */
    int64_t seq;                            /* packets delivered on the channel before this one */
    int32_t call, row, length;              /* n and f of the packet's last fragment; L */
    uint8_t src, dst, id, nfrag;            /* of the last fragment */
};
typedef struct pirip_pkt_entry pirip_pkt_entry;
struct pirip_pkt_info {
    int nrx, nchan, source_byte, filter_byte, address, max_frags, pending_records, ring_entries, cap, max_packet, has_rx, rx_rows, data_bytes,
        device;
};
typedef struct pirip_pkt_info pirip_pkt_info;
/* rx, tx and txs as in pirip_hip_ping_create, with its error codes: rx NULL or a streaming receiver created with an ldpc, of cfg->nrx
 * channels, at most 4096 rows per call (PIRIP_ERR_UNSUPPORTED above) and, with tx, of tx's data_bytes; tx and txs both NULL -- the handle
 * only receives, nchan = 0 and every call's d_out must be NULL -- or a transmitter and the streaming transmitter created on it. One of tx /
 * txs without the other, all three NULL, handles on different devices, cfg or out NULL, nrx < 1 or not rx's channels, source_byte outside
 * 0 .. 255, filter_byte or address outside -1 .. 255, max_frags outside 1 .. PIRIP_TX_REPEAT_MAX_FRAMES, pending_records < max_frags + 1,
 * ring_entries < 1, data_bytes < 16, and a txs whose queue_syms does not hold one burst of max_frags frames (preamble_syms + max_frags *
 * frame_syms + tx's largest gap) are PIRIP_ERR_BAD_ARG. Every work row is sized here with tx's gaps as they are: set the gaps first.
 * Create synchronises the device. */
int pirip_hip_pkt_create(pirip_hip_rx *rx, pirip_hip_tx *tx, pirip_hip_txs *txs, const pirip_pkt_config *cfg, pirip_hip_pkt **out);
int pirip_hip_pkt_destroy(pirip_hip_pkt *pkt);
int pirip_hip_pkt_get_info(const pirip_hip_pkt *pkt, pirip_pkt_info *info);
/* Transmit channel t hands over d_npk[t] (NULL = max_pk; clamped to [0, max_pk]) packets: packet j's bytes at d_bytes + t * chan_stride +
 * j * pkt_stride, its length d_len[t * max_pk + j] (int32) and its destination d_dst[t * max_pk + j] (uint8). They are taken in order: a
 * length outside 1 .. max_packet stops the channel and raises `bad`; a packet whose nfrag + 1 records do not fit the free space of the
 * channel's pending ring stops the channel and raises `refused`. Each packet taken gets id = (packets sent on the channel) mod 256 and is
 * written as its burst into the pending ring, from where the next calls' offers take it. d_taken[t] (may be NULL): packets taken, always
 * a prefix. Needs tx; NULL d_bytes / d_len / d_dst, max_pk < 0: PIRIP_ERR_BAD_ARG. Enqueued on hip_stream; never synchronises. */
int pirip_hip_pkt_send(pirip_hip_pkt *pkt, const uint8_t *d_bytes, size_t chan_stride, size_t pkt_stride, const int32_t *d_npk, int max_pk,
                       const int32_t *d_len, const uint8_t *d_dst, int32_t *d_taken, void *hip_stream);
/* Call n (n = 0, 1, ... since create / reset), in stream order:
 * 1. reassemble, per receive channel c over its d_ncalls[c] (NULL = ncalls; clamped to [0, ncalls]) rows in row order -- status bytes at
 *    d_status + c * status_stride, payloads of data_bytes bytes at d_payload + c * payload_stride, as pirip_hip_fsk_ldpc_rx_batch writes
 *    them; they are only read. The channel carries an open packet {src, id, nfrag, next, nbytes} and an assembly buffer of max_frags * cap
 *    bytes on the device, so a packet may straddle any number of calls. Every row goes through these rules, in this order:
 *    a. a row without PIRIP_RX_SYNC closes an open packet (incomplete);
 *    b. a row with PIRIP_RX_BITS whose byte 0 is filter_byte loses BITS (filtered);
 *    c. a row without BITS is done;
 *    d. a bad header -- nfrag outside 1 .. max_frags, idx >= nfrag, len outside 1 .. cap, or len != cap on a fragment that is not the
 *       last -- closes an open packet (incomplete), counts malformed, and the row is done;
 *    e. with address >= 0, a dst that is neither address nor 0xFF counts foreign, and the row is done: nothing else changes;
 *    f. idx == 0 closes an open packet (incomplete), opens {src, id, nfrag, next = 1, nbytes = len} and copies the len body bytes;
 *    g. idx > 0 with a packet open whose src, id and nfrag are the row's and whose next == idx appends the len body bytes: next += 1,
 *       nbytes += len; any other idx > 0 closes an open packet (incomplete), counts orphan, and the row is done;
 *    h. when next == nfrag the packet closes: nbytes < 5 or a CRC-32 that does not match counts crc_fail, else the packet is delivered.
 *    Delivery writes one pirip_pkt_entry at slot delivered % ring_entries of the channel's ring and the packet's length bytes at the same
 *    slot of a data ring with max_packet bytes per slot: the ring overwrites its oldest entry (lost).
 * 2. offer: section M's step 2 with a hold-off of 0 over the pending rings that pirip_hip_pkt_send fills.
 * 3. pirip_hip_txs_process into d_out (its rules for d_out / out_stride_bytes).
 * A handle without tx runs step 1 alone and wants d_out == NULL (else PIRIP_ERR_BAD_ARG); a handle with tx wants d_out. d_status and
 * d_payload are required (PIRIP_ERR_BAD_ARG), as are strides that hold ncalls rows when nrx > 1. ncalls <= 4096 (PIRIP_ERR_UNSUPPORTED
 * above), ncalls < 0 is PIRIP_ERR_BAD_ARG. Works with and without rx (with rx it changes nothing of the receiver). Enqueued on
 * hip_stream (NULL = default stream); never synchronises. */
int pirip_hip_pkt_push_records(pirip_hip_pkt *pkt, const uint8_t *d_status, size_t status_stride, const uint8_t *d_payload, size_t payload_stride,
                               const int32_t *d_ncalls, int ncalls, void *d_out, size_t out_stride_bytes, void *hip_stream);
/* Need rx (PIRIP_ERR_BAD_ARG without): pirip_hip_rx_process on the block at pirip_hip_rx_input (push: after copying it from d_in as
 * pirip_hip_rx_push does; d_in == NULL is PIRIP_ERR_BAD_ARG) into the handle's own record rows, then the steps above over them. */
int pirip_hip_pkt_process(pirip_hip_pkt *pkt, void *d_out, size_t out_stride_bytes, void *hip_stream);
int pirip_hip_pkt_push(pirip_hip_pkt *pkt, const void *d_in, size_t in_stride_bytes, void *d_out, size_t out_stride_bytes, void *hip_stream);
/* The rows the last call read, as received: after process / push the handle's own -- rx_rows rows per channel, strides in elements,
 * d_nframes [nrx] --, after push_records the caller's. Valid in stream order; each pointer may be NULL. PIRIP_ERR_BAD_ARG before the
 * first call. */
int pirip_hip_pkt_records(pirip_hip_pkt *pkt, const uint8_t **d_status, size_t *status_stride, const uint8_t **d_payload, size_t *payload_stride,
                          const int32_t **d_nframes);
/* The records offered to the streaming transmitter in the last call: channel t's d_nrec[t] records at d_records + t * rec_stride.
 * PIRIP_ERR_BAD_ARG on a handle without tx. */
int pirip_hip_pkt_offered(pirip_hip_pkt *pkt, const uint8_t **d_records, size_t *rec_stride, const int32_t **d_nrec);
/* Host copies (synchronises the device), each may be NULL. Per receive channel [nrx]: packets delivered, frames the filter removed, frames
 * for another address, frames with a bad header, fragments that fitted no open packet, packets closed before their last fragment, packets
 * whose body failed its check, entries the ring overwrote. Per transmit channel [nchan]: packets sent, sends stopped by a full ring,
 * sends stopped by a bad length, records waiting in the ring. */
int pirip_hip_pkt_get_counters(pirip_hip_pkt *pkt, int64_t *delivered, int64_t *filtered, int64_t *foreign, int64_t *malformed, int64_t *orphan,
                               int64_t *incomplete, int64_t *crc_fail, int64_t *lost, int64_t *sent, int64_t *refused, int64_t *bad,
                               int64_t *pending);
/* Host copy (synchronises the device) of the newest min(delivered, ring_entries, max) entries of receive channel chan, oldest first, and
 * their bytes at bytes + i * max_packet (bytes may be NULL); *written (may be NULL): how many. PIRIP_ERR_BAD_ARG for chan outside
 * [0, nrx), max < 0 or entries == NULL with max > 0. */
int pirip_hip_pkt_get_packets(pirip_hip_pkt *pkt, int chan, pirip_pkt_entry *entries, uint8_t *bytes, int max, int *written);
/* Forgets open packets, the rings and the counters and resets txs, and rx where present: the next call is n = 0, the next id 0. */
int pirip_hip_pkt_reset(pirip_hip_pkt *pkt, void *hip_stream);
/* One HIP stream per handle: open packets, rings and counters are device state advanced in stream order, the call index is host state
 * advanced when a call is enqueued. */

/* Parity fragments (opt-in, per handle). The link loses frames, and a plain handle loses the packet with any of them.
 * A handle created with pirip_hip_pkt_create_fec sends, behind the k = nfrag data fragments of a packet, r(k) = max(1, min(max_parity,
 * ceil(k * parity_pct / 100))) parity fragments, and puts a packet together from any k of its k + r fragments. Both ends are configured
 * alike. There is still no acknowledgement and no retransmission in this section: section S adds them above it.
 *   Data fragments are a plain handle's, header and body, except that the padding behind the CRC-32 in the last fragment is not zeros:
 *   body byte q of the packet (q counted over its k * cap body bytes, q >= L + 4) is pad(id, q), in uint32 arithmetic
 *       x = ((id << 16) | q) * 2654435761u; x ^= x >> 16; x *= 2246822519u; x ^= x >> 13; pad = x >> 24
 *   so that a short last fragment is no run of equal symbols. No reader looks at these bytes.
 *   Parity fragment j (0 <= j < r) has idx = k + j, nfrag = k, the packet's src, dst and id, and len = the last data fragment's len: the
 *   packet's length is known whenever one parity fragment is. Its cap body bytes are P_j[b] = XOR_i C[j][i] * D_i[b], b = 0 .. cap - 1,
 *   over the full cap-byte bodies D_i of the data fragments as sent, CRC-32 and padding included, in GF(2^8) with the polynomial
 *   x^8 + x^4 + x^3 + x^2 + 1 (0x11D). C is the Cauchy matrix C[j][i] = 1 / (j XOR (max_parity + i)), 0 <= j < max_parity, 0 <= i <
 *   max_frags, of which a packet uses the first r(k) rows and k columns: every square submatrix of it is regular. The header bytes
 *   are not covered: a repeater rewrites src and the parity stays valid.
 *   One packet is one burst of k + r frames and the `2` record, placed whole: k + r + 1 records of room, else `refused`.
 * A plain handle receives an undamaged burst of an FEC handle as before and then counts its r parity frames malformed; an FEC handle
 * receives a plain sender's burst, for which no parity is needed when nothing is lost.
 *
 * Step 1 of a call on an FEC handle. The channel carries the key {src, id, nfrag} of one packet, a phase (none / collecting / closed),
 * a bitmap of the k + r fragments seen and their count, lastlen (the last data fragment's len, 0 = not yet stated) and an assembly
 * buffer of (max_frags + max_parity) * cap bytes with fragment idx at idx * cap. Every row goes through these rules, in this order:
 *    A. a row without PIRIP_RX_SYNC changes nothing and counts nothing (unlike rule a: a fade that drops sync in the middle of a burst is
 *       what the parity is for);
 *    B. a row with PIRIP_RX_BITS whose byte 0 is filter_byte loses BITS (filtered);
 *    C. a row without BITS is done;
 *    D. a bad header counts malformed and the row is done, nothing else changes: nfrag outside 1 .. max_frags; idx >= nfrag + r(nfrag);
 *       a data fragment (idx < nfrag) with len outside 1 .. cap, or with len != cap when it is not the last; a parity fragment with len
 *       outside 1 .. cap; a fragment that states lastlen (the last data fragment or a parity fragment) differently from the lastlen that
 *       the packet being collected, if the fragment's key is its key, already holds;
 *    E. with address >= 0, a dst that is neither address nor 0xFF counts foreign, and the row is done;
 *    F. the key is the channel's and the phase is closed: surplus, done. The key is the channel's, the phase collecting and the
 *       fragment's bit set: duplicate, done. The key is the channel's, the phase collecting and the bit clear: store. Any other key:
 *       a packet being collected is counted incomplete, the channel's state opens on this fragment -- any fragment may open a packet
 *       -- and stores it. Store: all cap body bytes go to the buffer, the bit is set, the count goes up, and the last data fragment
 *       or a parity fragment sets lastlen;
 *    G. when the count reaches k the phase becomes closed. The m missing data fragments are rebuilt from the m parity fragments present
 *       (there are exactly m): S_p = P_p XOR XOR_{i present} C[p][i] * D_i per parity row p, then the m x m system over the missing
 *       columns is solved by Gauss-Jordan elimination. L = (k - 1) * cap + lastlen - 4; L < 1 or a CRC-32 that does not match counts
 *       crc_fail, else the packet is delivered exactly as by rule h (entry, data ring, row = this row), and with m > 0 recovered
 *       goes up by 1 and repaired by m.
 * One packet is open per channel: fragments of two senders interleaved on one channel throw each other out, which is counted
 * incomplete. A packet whose key is that of the packet before it on the channel (the same sender, nfrag and id, 256 packets on with
 * nothing heard between) is taken for surplus.
 * The two structures are written as the three above are and are held to their twins -- binding.PktFecConfig, PktFecInfo -- by
 * tests/test_packet_fec_cpu.py. */
struct pirip_pkt_fec_config {
    int max_parity;             /* R, 1..16: parity fragments of a packet at most */
    int parity_pct;             /* 1..100: parity fragments per 100 data fragments, rounded up */
};
typedef struct pirip_pkt_fec_config pirip_pkt_fec_config;
struct pirip_pkt_fec_info {
    int enabled, max_parity, parity_pct;
    int max_burst_frames;       /* max_frags + r(max_frags); max_frags on a plain handle */
};
typedef struct pirip_pkt_fec_info pirip_pkt_fec_info;
/* pirip_hip_pkt_create with parity fragments: every rule of it, and fec NULL, max_parity outside 1 .. 16, parity_pct outside 1 .. 100,
 * max_frags + max_parity > PIRIP_TX_REPEAT_MAX_FRAMES (a repeater can hold any burst whole, and idx stays a byte), pending_records <
 * max_burst_frames + 1 and a txs whose queue_syms does not hold one burst of max_burst_frames frames (preamble_syms + max_burst_frames *
 * frame_syms + tx's largest gap) are PIRIP_ERR_BAD_ARG. max_packet is max_frags * cap - 4 as before. Every other entry point of this
 * section works on the handle unchanged; pirip_hip_pkt_get_counters reports orphan = 0 on it, always. */
int pirip_hip_pkt_create_fec(pirip_hip_rx *rx, pirip_hip_tx *tx, pirip_hip_txs *txs, const pirip_pkt_config *cfg,
                             const pirip_pkt_fec_config *fec, pirip_hip_pkt **out);
/* enabled = 0 on a plain handle (max_parity = parity_pct = 0, max_burst_frames = max_frags). */
int pirip_hip_pkt_get_fec_info(const pirip_hip_pkt *pkt, pirip_pkt_fec_info *info);
/* Host copies (synchronises the device), each may be NULL, per receive channel [nrx]: packets delivered that needed a decode, data
 * fragments rebuilt in them, fragments seen twice while their packet was collected, fragments of a packet that was closed already.
 * PIRIP_ERR_BAD_ARG on a plain handle. */
int pirip_hip_pkt_get_fec_counters(pirip_hip_pkt *pkt, int64_t *recovered, int64_t *repaired, int64_t *duplicate, int64_t *surplus);

/* ----------------------------------------------------------------------------------- */
/* section S : ARQ sessions (acknowledged in-order delivery with retransmission)        */
/*   Section R loses a packet with a lost fragment and asks nobody again; parity raises   */
/*   the threshold and does not close the loop. This section closes it: a selective-repeat */
/*   session per channel over one packet handle, plain or FEC, whose every terminal both    */
/*   sends and receives. ARQ segments travel as the payload of section R packets: R's wire   */
/*   format, its src byte, --filter, parity and whitening apply unchanged.   */
/*   No call synchronises or allocates; time is counted in calls; every byte and counter is a  */
/*   function of the inputs. Only symbols are added: PIRIP_HIP_ABI_VERSION stands.             */
/* ----------------------------------------------------------------------------------- */
typedef struct pirip_hip_arq pirip_hip_arq;
/* Wire format: the payload bytes of a section R packet.
 *   byte 0  type   0xD0 DATA, 0xA0 ACK
 *   byte 1  seq    DATA: the segment's sequence number mod 256
 *                  ACK:  base = the next sequence number the receiver wants in order, mod 256
 *   DATA:   bytes 2 .. : 1 .. max_payload user bytes, max_payload = pkt's max_packet - 2
 *   ACK:    bytes 2 .. 5: bitmap, least significant byte first; bit i set = segment base + 1 + i is held out of order
 *           bytes 6 .. acklen - 1: filler, byte q = (31 * base + 73 * q + 0x5A) & 0xFF
 *           acklen = max(6, min(cap - 4, max_packet)): an ACK fills its one fragment up to the CRC-32, so that it is no run of equal
 *           symbols on a plain handle (section R). A receiver accepts an ACK of any length >= 6 and reads six bytes.
 * The window W is 1 .. 32, so sequence numbers mod 256 are unambiguous; the state keeps absolute int64 counters.
 * (This section's three structures are written as section R's are and are held to their twins -- binding.ArqConfig, ArqEntry, ArqInfo,
 * ARQ_ENTRY_DTYPE -- by tests/test_arq_cpu.py.) */
struct pirip_arq_config {
    int window;                 /* W, 1..32: segments in flight per channel */
    int rto_calls;              /* >= 1: calls after which an unacknowledged segment is sent again */
    int max_tries;              /* >= 1: transmissions of one segment before the session is broken */
    int queue_entries;          /* >= window: segments of each channel's submit queue, which is its retransmission store */
    int out_entries;            /* >= 1: segments of each channel's output ring */
};
typedef struct pirip_arq_config pirip_arq_config;
struct pirip_arq_entry {                    /* 16 bytes */
    int64_t seq;                            /* the segment's absolute sequence number */
    int32_t call, length;                   /* n of the call that delivered it; user bytes */
};
typedef struct pirip_arq_entry pirip_arq_entry;
struct pirip_arq_info {
    int nchan, window, rto_calls, max_tries, queue_entries, out_entries, max_payload, acklen, device;
};
typedef struct pirip_arq_info pirip_arq_info;
/* A handle over one packet handle, which it borrows as the packet handle borrows rx / tx / txs: pkt must outlive it, and WHILE AN ARQ
 * HANDLE LIVES ITS PACKET HANDLE MUST NOT BE DRIVEN DIRECTLY (send, push_records, process, push, reset); that is not enforced. Transmit
 * channel t and receive channel t of pkt form one session with the peer address peers[t] (host int[nchan]): 0 .. 255, or -1 for "whoever
 * answers". DATA and ACK go to dst = peers[t], or 0xFF when it is -1. PIRIP_ERR_BAD_ARG: pkt, cfg, peers or out NULL; a packet handle
 * without tx or with nrx != nchan; window outside 1 .. 32; rto_calls < 1; max_tries < 1; queue_entries < window; out_entries < 1; a peer
 * outside -1 .. 255; pkt's max_packet < 6. Create synchronises the device.
 * Sessions through a section M repeater are out of scope: it rewrites src, so a terminal's own DATA would come back as the peer's. */
int pirip_hip_arq_create(pirip_hip_pkt *pkt, const pirip_arq_config *cfg, const int *peers, pirip_hip_arq **out);
int pirip_hip_arq_destroy(pirip_hip_arq *arq);
int pirip_hip_arq_get_info(const pirip_hip_arq *arq, pirip_arq_info *info);
/* Sender state of a channel: sub_nxt (segments accepted from the user), snd_nxt (segments sent at least once), snd_una (the oldest
 * unacknowledged segment), broken, per window slot (segment s at s % W) acked, tries, due, and a segment ring of queue_entries slots of
 * max_payload bytes with its lengths: segment s lives at slot s % queue_entries from submit until snd_una passes it.
 * Channel t hands over d_nseg[t] (NULL = max_seg; clamped to [0, max_seg]) segments: segment j's bytes at d_bytes + t * chan_stride +
 * j * seg_stride, its length d_len[t * max_seg + j] (int32). They are taken in order, and what is taken is a prefix: a length outside
 * 1 .. max_payload stops the channel and raises `bad`; a full ring (sub_nxt - snd_una == queue_entries) or a broken session stops the
 * channel and raises `refused`. d_taken[t] (may be NULL): segments taken. NULL d_bytes / d_len, max_seg < 0: PIRIP_ERR_BAD_ARG. Enqueued
 * on hip_stream; never synchronises. */
int pirip_hip_arq_submit(pirip_hip_arq *arq, const uint8_t *d_bytes, size_t chan_stride, size_t seg_stride, const int32_t *d_nseg, int max_seg,
                         const int32_t *d_len, int32_t *d_taken, void *hip_stream);
/* Call n (n = 0, 1, ... since create / reset), in stream order:
 * 1. stage. From the session state as call n - 1 left it, each channel lists what it sends now, into a device staging area of 1 + W
 *    packets per channel, in this order:
 *    (a) one ACK {base = rcv_nxt, bitmap of the reorder buffer} if ack_pending;
 *    (b) if any in-flight slot (snd_una <= s < snd_nxt) has !acked, due <= n and tries == max_tries, the session becomes broken, counted
 *        once; a broken session stages nothing but (a);
 *    (c) otherwise every in-flight slot with !acked and due <= n, ascending;
 *    (d) then new segments snd_nxt .. while snd_nxt - snd_una < W and snd_nxt < sub_nxt, ascending.
 * 2. send. pirip_hip_pkt_send from the staging area; what it takes is a prefix (section R's contract).
 * 3. commit. The state changes of the staged items that were taken, and of those only; `deferred` goes up by the count of the others.
 *    ACK: ack_pending = 0, acks_sent += 1. Retransmission: tries += 1, due = n + rto_calls, retransmitted += 1. New segment: tries = 1,
 *    due = n + rto_calls, snd_nxt += 1, sent += 1.
 * 4. the packet handle's own call of the same name with the same arguments and rules: reassemble, offer, pirip_hip_txs_process into
 *    d_out.
 * 5. receive. The packets step 4 delivered on each channel, in the packet ring's seq order; the handle keeps seen[c], the count of packets
 *    it has consumed, and when delivered - seen > pkt's ring_entries the overwritten packets are skipped and counted `overrun`
 *    (retransmission recovers them). Receiver state: rcv_nxt, a held bitmap and a reorder buffer of W slots (segment s at s % W),
 *    ack_pending, and an output ring of out_entries slots of max_payload bytes with pirip_arq_entry entries, which overwrites its oldest
 *    entry (lost). Each packet of length L from source src goes through these rules, in this order:
 *    R1. L < 2, or a type that is neither 0xD0 nor 0xA0: alien, done (plain datagrams may share the channel; pkt's ring still holds them).
 *    R2. peer[c] >= 0 and src != peer[c]: stranger, done.
 *    R3. DATA. L < 3: malformed, done. Let d = (seq - rcv_nxt) & 255. d == 0: deliver with entry seq = rcv_nxt, call = n, and
 *        rcv_nxt += 1, then deliver held successors while the next one is held; ack_pending = 1. 0 < d < W: a held segment counts
 *        duplicate, another is held; ack_pending = 1. Else let back = (rcv_nxt - seq) & 255: 1 <= back <= min(W, rcv_nxt) counts
 *        duplicate, ack_pending = 1. Else outside, done.
 *    R4. ACK. L < 6: malformed, done. Let a = (base - snd_una) & 255. a > snd_nxt - snd_una: stale, done. Otherwise snd_una += a;
 *        every bit i with base + 1 + i < snd_nxt sets that slot's acked; `acked` goes up by the number of segments acknowledged for the
 *        first time, cumulatively or by bit, each once.
 * Section R's checks of the handle, of d_status / d_payload, their strides and ncalls, of d_in and of d_out / out_stride_bytes are made
 * before anything is enqueued; the packet handle needs rx for process / push as there. Enqueued on hip_stream; never synchronises. */
int pirip_hip_arq_push_records(pirip_hip_arq *arq, const uint8_t *d_status, size_t status_stride, const uint8_t *d_payload, size_t payload_stride,
                               const int32_t *d_ncalls, int ncalls, void *d_out, size_t out_stride_bytes, void *hip_stream);
int pirip_hip_arq_process(pirip_hip_arq *arq, void *d_out, size_t out_stride_bytes, void *hip_stream);
int pirip_hip_arq_push(pirip_hip_arq *arq, const void *d_in, size_t in_stride_bytes, void *d_out, size_t out_stride_bytes, void *hip_stream);
/* Host copies (synchronises the device), each may be NULL, per channel [nchan]. Sender: segments sent for the first time, sent again,
 * acknowledged, ACKs sent, staged items pirip_hip_pkt_send did not take, submits stopped by a full ring or a broken session, submits
 * stopped by a bad length, broken (0 / 1), waiting = sub_nxt - snd_nxt, inflight = snd_nxt - snd_una. Receiver: segments delivered, DATA
 * seen before, DATA outside the window, ACKs outside the window, packets that are no segment, packets of another source, segments too
 * short, packets the packet ring overwrote unseen, entries the output ring overwrote. */
int pirip_hip_arq_get_counters(pirip_hip_arq *arq, int64_t *sent, int64_t *retransmitted, int64_t *acked, int64_t *acks_sent, int64_t *deferred,
                               int64_t *refused, int64_t *bad, int64_t *broken, int64_t *waiting, int64_t *inflight, int64_t *delivered,
                               int64_t *duplicate, int64_t *outside, int64_t *stale, int64_t *alien, int64_t *stranger, int64_t *malformed,
                               int64_t *overrun, int64_t *lost);
/* Host copy (synchronises the device) of the newest min(delivered, out_entries, max) entries of channel chan, oldest first, and their
 * bytes at bytes + i * max_payload (bytes may be NULL); *written (may be NULL): how many. PIRIP_ERR_BAD_ARG as pirip_hip_pkt_get_packets. */
int pirip_hip_arq_get_delivered(pirip_hip_arq *arq, int chan, pirip_arq_entry *entries, uint8_t *bytes, int max, int *written);
/* Checking aid (synchronises), each pointer may be NULL: the absolute counters of channel chan, the held bitmap (bit i: segment
 * rcv_nxt + 1 + i) and ack_pending. */
int pirip_hip_arq_get_state(pirip_hip_arq *arq, int chan, int64_t *sub_nxt, int64_t *snd_nxt, int64_t *snd_una, int64_t *rcv_nxt,
                            uint32_t *held, int *ack_pending);
/* Forgets the sessions, the rings and the counters and resets the packet handle too: the next call is n = 0, the next segment 0. */
int pirip_hip_arq_reset(pirip_hip_arq *arq, void *hip_stream);
/* One HIP stream per handle, the packet handle's: the sessions are device state advanced in stream order, the call index is host state
 * advanced when a call is enqueued. */

/* ----------------------------------------------------------------------------------- */
/* section T : half-duplex medium access (carrier sense, backoff, T/R mute)             */
/*   The reference radio is half duplex on one frequency: a terminal that transmits      */
/*   hears itself, and two that start together destroy each other's bursts. Sections R    */
/*   and S offer a burst in the first call in which it is due and fits. This section       */
/*   attaches to a packet handle and decides, per call and on the device: whether a         */
/*   receive channel carries somebody's carrier, whether the rows it brought are the own     */
/*   transmitter's (they lose PIRIP_RX_BITS), and how many bursts the offer may take after a  */
/*   slotted random backoff. No call synchronises or allocates; time is       */
/*   counted in calls; every decision is a function of the inputs and the key. A packet handle  */
/*   without this layer makes the launches and the bytes it made before. Only symbols are       */
/*   added: PIRIP_HIP_ABI_VERSION stands.                                                        */
/* ----------------------------------------------------------------------------------- */
typedef struct pirip_hip_mac pirip_hip_mac;
/* (This section's two structures are written as section R's are and are held to their twins -- binding.MacConfig, MacInfo -- by
 * tests/test_mac_cpu.py.) */
struct pirip_mac_config {
    int sense_mask;             /* 1..3: bit 0 = a row with PIRIP_RX_SYNC is carrier; bit 1 = a row whose stats[5] (SNRest) >= sense_snr is carrier */
    float sense_snr;            /* compared as the float it is; a NaN row is no carrier */
    int slot_calls;             /* 1..2^20: calls per backoff slot */
    int cw;                     /* 1..1024: every access draws b in [0, cw) slots */
    int ifs_calls;              /* 0..2^30 - 1: the countdown runs only in a call that ends a run of more than ifs_calls idle calls */
    int mute_calls;             /* 0..2^30: see step 1 */
    int txop_bursts;            /* 1..2^30: bursts one access may put on air */
    uint32_t key;               /* seeds the draws; the two ends of a link take different keys */
};
typedef struct pirip_mac_config pirip_mac_config;
struct pirip_mac_info {
    int ntx, nrx, sense_mask;
    float sense_snr;
    int slot_calls, cw, ifs_calls, mute_calls, txop_bursts;
    uint32_t key;
    int device;
};
typedef struct pirip_mac_info pirip_mac_info;
#define PIRIP_MAC_IDLE    0
#define PIRIP_MAC_CONTEND 1
#define PIRIP_MAC_HOLD    2
/* Attaches a medium-access layer to pkt, which it borrows: pkt must outlive it, must have a transmitter, and has at most one such layer.
 * rx_of_tx (host int32 [pkt's transmit channels]): -1 for an ungated transmit channel, which is offered exactly as without the layer, or
 * the receive channel 0 .. nrx - 1 that the transmit channel listens on and whose rows its own bursts come back in. While attached every
 * call of pkt -- push_records, process, push, driven directly or by a section S handle -- runs steps 0 - 2 below in front of its own, in
 * stream order; on a pkt with rx and bit 1 of sense_mask, process / push also ask the receiver for its stats rows, into a buffer this
 * handle owns. PIRIP_ERR_BAD_ARG: pkt, cfg, rx_of_tx or out NULL; a pkt without tx or with a layer already; a configuration value outside
 * the limits stated at pirip_mac_config; an rx_of_tx outside -1 .. nrx - 1; two transmit channels that name one receive channel. Create
 * synchronises the device.
 *
 * Call n (pkt's n), per channel:
 * 0. air, per transmit channel t: air = 1 iff section K dequeued at least one symbol of t in call n - 1's process (PIRIP_TX_CARRIER_OFF
 *    symbols inside a burst count: the antenna switch stays on Tx); 0 in this layer's first call. quiet[t] = 0 if air, else
 *    min(quiet[t] + 1, 2^30); it starts at 2^30.
 * 1. sense and mute, per receive channel c, in front of section R's reassembly; t = the transmit channel with rx_of_tx[t] == c, if any.
 *    own = t exists and quiet[t] < mute_calls. If own: every row of the call loses PIRIP_RX_BITS before rule a / A reads it and keeps
 *    PIRIP_RX_SYNC (the caller's rows are only read: the reassembly reads a copy), `muted` goes up by the rows that had BITS, carrier = 0.
 *    Otherwise carrier = 1 iff some row f < nf has PIRIP_RX_SYNC with bit 0 of sense_mask, or stats[f][5] >= sense_snr with bit 1 and
 *    stats rows given. idle[c] = 0 if own or carrier, else min(idle[c] + 1, 2^30); it starts at 0. `own` and `carrier` count the calls.
 * 2. gate, per transmit channel t with c = rx_of_tx[t] >= 0. State: phase (PIRIP_MAC_IDLE at first), counter, run, accesses. due = the
 *    pending ring's head burst exists and its ready tag <= n; queued = section K's queue of t is not empty before the offer. In this order:
 *    1. HOLD and not queued: phase = IDLE.
 *    2. IDLE and due: phase = CONTEND, counter = slot_calls * draw(key, t, accesses), accesses += 1.
 *    3. CONTEND: if idle[c] > ifs_calls and counter == 0: phase = HOLD, run = 0, won += 1; if idle[c] > ifs_calls and counter > 0:
 *       counter -= 1, backoff += 1; otherwise deferred += 1.
 *    4. limit = HOLD ? txop_bursts - run : 0: section R's offer takes at most `limit` bursts beside its own rules; run and `bursts` go up
 *       by what it took.
 *    draw(key, t, a), in uint32 with a truncated to 32 bits:
 *        x = key ^ t * 0x9E3779B9 ^ a * 0x85EBCA6B;  x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16;
 *        draw = ((uint64_t)x * cw) >> 32.
 *    There is no exponential window: this layer sees no ACKs. */
int pirip_hip_mac_create(pirip_hip_pkt *pkt, const pirip_mac_config *cfg, const int32_t *rx_of_tx, pirip_hip_mac **out);
/* Detaches (synchronises the device): pkt then behaves as if no layer had ever been attached. */
int pirip_hip_mac_destroy(pirip_hip_mac *mac);
int pirip_hip_mac_get_info(const pirip_hip_mac *mac, pirip_mac_info *info);
/* pirip_hip_pkt_push_records only: the stats rows that go with the status rows of the calls that follow, PIRIP_STATS_PER_FRAME floats per
 * row, channel c's at d_stats + c * stats_stride (device, stride in floats, as pirip_hip_rx_process writes them; only read). NULL (the
 * state after create): bit 1 senses nothing. PIRIP_ERR_BAD_ARG on a pkt with rx when bit 1 of sense_mask is set: the layer owns them. */
int pirip_hip_mac_set_stats(pirip_hip_mac *mac, const float *d_stats, size_t stats_stride);
/* The stats rows the next call's step 1 reads, as pirip_hip_pkt_records gives the status rows: what pirip_hip_mac_set_stats named, or on
 * a pkt with rx and bit 1 the handle's own buffer, which holds the rows of the last process / push. *d_stats NULL: none. Each may be NULL. */
int pirip_hip_mac_stats(pirip_hip_mac *mac, const float **d_stats, size_t *stats_stride);
/* Host copies (synchronises the device), each may be NULL. Per transmit channel [ntx]: accesses, accesses won, calls counted down, calls
 * deferred, bursts offered through the gate. Per receive channel [nrx]: calls with carrier, calls that were the own transmitter's, rows
 * that lost PIRIP_RX_BITS. */
int pirip_hip_mac_get_counters(pirip_hip_mac *mac, int64_t *accesses, int64_t *won, int64_t *backoff, int64_t *deferred, int64_t *bursts,
                               int64_t *carrier, int64_t *own, int64_t *muted);
/* Checking aid (synchronises), each pointer may be NULL: transmit channel t's phase, counter, run and quiet, and the idle run of the
 * receive channel it listens on (-1 for an ungated channel). PIRIP_ERR_BAD_ARG for a t outside 0 .. ntx - 1. */
int pirip_hip_mac_get_state(pirip_hip_mac *mac, int t, int *phase, int *counter, int *run, int *quiet, int *idle);
/* Forgets the state and the counters: the next call is the layer's first. pirip_hip_pkt_reset (and with it pirip_hip_arq_reset) does the
 * same to an attached layer. Enqueued on hip_stream. */
int pirip_hip_mac_reset(pirip_hip_mac *mac, void *hip_stream);

/* ----------------------------------------------------------------------------------- */
/* section C : libcodec2-compatible single-stream API (host buffers)                    */
/*             names and signatures as codec2 src/fsk.h [UPSTREAM-RECALLED]              */
/* ----------------------------------------------------------------------------------- */
#ifndef PIRIP_NO_CODEC2_SHIM
typedef struct { float real; float imag; } COMP;
#define MODE_M_MAX 4

/* struct FSK: the fields codec2's own programs read directly (fsk_demod.c, rtl_fsk.c: fsk->Nbits, fsk->Ndft, fsk->f_est[],
 * fsk->Sf[], fsk->norm_rx_timing, fsk->SNRest, fsk->ppm ...) are PUBLIC here, in codec2's order and with codec2's names
 * [UPSTREAM-RECALLED codec2 src/fsk.h], and are refreshed after every fsk_demod()/fsk_demod_sd() (Sf is downloaded on
 * demand through fsk->Sf: a host copy the library owns). Fields that have no host-side meaning in this build are kept for
 * source compatibility and left NULL/zero (hann_table, f_dc, fft_cfg, phi_c). Code must be recompiled against this header:
 * the layout follows the recalled upstream order but codec2 is not in /root/reference to check it against. The demodulator
 * state itself lives on the GPU behind `pirip_priv`. */
struct MODEM_STATS;
struct FSK {
    /* static parameters set up by fsk_create_hbr */
    int Ndft, Fs, N, Rs, Ts, Nmem, P, Nsym, Nbits, f1_tx, tone_spacing, mode;
    float tc;
    int est_min, est_max, est_space;
    float *hann_table;                 /* NULL: the window lives on the device */
    /* parameters used by the demodulator */
    float *Sf;                         /* [Ndft] smoothed magnitude spectrum, host copy refreshed by fsk_demod*() */
    COMP phi_c[MODE_M_MAX];            /* not mirrored (oscillators are device-side phase accumulators) */
    COMP *f_dc;                        /* NULL */
    void *fft_cfg;                     /* NULL */
    float norm_rx_timing;
    COMP tx_phase_c;                   /* modulator phase (fsk_mod / fsk_mod_c run on the CPU) */
    /* statistics generated by the demodulator */
    float EbNodB;
    float f_est[MODE_M_MAX];           /* peak-method tone estimates, Hz */
    float f2_est[MODE_M_MAX];          /* mask-method tone estimates, Hz (equal to f_est when the peak method drives the demod) */
    int freq_est_type;
    float ppm, SNRest, v_est, rx_sig_pow, rx_nse_pow;
    /* parameters used by mod/demod and the driving code */
    int nin, burst_mode, lock_nin;
    struct MODEM_STATS *stats;
    int normalise_eye;
    void *pirip_priv;                  /* library-private: device handle, staging buffers */
};

struct FSK *fsk_create(int Fs, int Rs, int M, int tx_f1, int tx_fs);
struct FSK *fsk_create_hbr(int Fs, int Rs, int M, int P, int Nsym, int f1_tx, int tone_spacing);
void fsk_destroy(struct FSK *fsk);
void fsk_set_freq_est_limits(struct FSK *fsk, int est_min, int est_max);
void fsk_set_freq_est_alg(struct FSK *fsk, int est_type);
uint32_t fsk_nin(struct FSK *fsk);
void fsk_demod(struct FSK *fsk, uint8_t rx_bits[], COMP fsk_in[]);
void fsk_demod_sd(struct FSK *fsk, float rx_filt[], COMP fsk_in[]);
void fsk_clear_estimators(struct FSK *fsk);
void fsk_enable_burst_mode(struct FSK *fsk);
/* Demod statistics, codec2's layout [UPSTREAM-RECALLED codec2 src/modem_stats.h]. The FSK demodulator fills Nc, snr_est
 * (the smoothed EbNodB, as upstream), foff, rx_timing, clock_offset, f_est and the eye diagram of the latest frame (rx_eye,
 * neyetr, neyesamp). The eye is OPT-IN here: a section C handle runs on its specialised kernel and leaves neyetr = 0 until
 * the program calls fsk_stats_normalise_eye() (either value) or the environment holds PIRIP_SHIM_EYE=1 -- from then on it runs
 * with pirip_hip_enable_eye (any-configuration kernel; asked for after the first fsk_demod() the demodulator state restarts,
 * with a note on stderr). The scatter (rx_symbols) / FFT members exist so that
 * code written against codec2 compiles and indexes them, and stay zero -- the FSK demodulator does not fill them upstream either. */
#define MODEM_STATS_NC_MAX      50
#define MODEM_STATS_NR_MAX      160
#define MODEM_STATS_ET_MAX      8
#define MODEM_STATS_EYE_IND_MAX 160
#define MODEM_STATS_NSPEC       512
#define MODEM_STATS_MAX_F_HZ    4000
#define MODEM_STATS_MAX_F_EST   4
struct MODEM_STATS {
    int Nc;
    float snr_est;
    COMP rx_symbols[MODEM_STATS_NR_MAX][MODEM_STATS_NC_MAX + 1];
    int nr, sync;
    float foff, rx_timing, clock_offset, sync_metric;
    int pre, post, uw_fails;
    float rx_eye[MODEM_STATS_ET_MAX][MODEM_STATS_EYE_IND_MAX];
    int neyetr, neyesamp;
    float f_est[MODEM_STATS_MAX_F_EST];
    float fft_buf[2 * MODEM_STATS_NSPEC];
    void *fft_cfg;
};
void fsk_get_demod_stats(struct FSK *fsk, struct MODEM_STATS *stats);
void fsk_stats_normalise_eye(struct FSK *fsk, int normalise_enable);   /* default on, as upstream */
void fsk_mod(struct FSK *fsk, float fsk_out[], uint8_t tx_bits[], int nbits);      /* CPU: Tx side */
void fsk_mod_c(struct FSK *fsk, COMP fsk_out[], uint8_t tx_bits[], int nbits);     /* CPU: Tx side */
/* accessors (kept from round 1; the public fields above carry the same values) */
int fsk_get_Nbits(struct FSK *fsk);
int fsk_get_Nsym(struct FSK *fsk);
int fsk_get_N(struct FSK *fsk);
int fsk_get_Ts(struct FSK *fsk);
int fsk_get_Ndft(struct FSK *fsk);
float fsk_get_norm_rx_timing(struct FSK *fsk);
float fsk_get_SNRest(struct FSK *fsk);
void fsk_get_f_est(struct FSK *fsk, float f_est[/*M*/]);
void fsk_get_Sf(struct FSK *fsk, float Sf[/*Ndft*/]);
#endif


/* ----------------------------------------------------------------------------------- */
/* section F : the FreeDV API calls `rtl_fsk --code` and `rpitx_fsk --code` bind          */
/*             [UPSTREAM-RECALLED codec2 src/freedv_api.h, freedv_fsk.c]                  */
/*   What upstream's rtl_fsk.c does in coded mode is libcodec2's FreeDV API in              */
/*   FREEDV_MODE_FSK_LDPC: freedv_open_advanced / freedv_nin / freedv_rawdatacomprx /       */
/*   freedv_get_rx_status / freedv_get_bits_per_modem_frame / freedv_close. The shape of    */
/*   that API is in the reference itself: struct freedv_advanced members Rs, Fs, M,         */
/*   codename (/root/reference/tx/rpitx_fsk.cpp:165,222,319-322), the Tx-side helpers it    */
/*   declares by hand (:33-40) and uses (:75-83,324-325,395,443,474), the rx_status bits    */
/*   (/root/reference/tx/frame_repeater.c:71,80,88). Each entry is a thin shim over         */
/*   sections C and E: one handle = one stream, caller owns every buffer, no error codes    */
/*   (NULL from open, as upstream).                                                          */
/*   codename -> code file: a path, else $PIRIP_CODE_DIR/<codename>.code, else               */
/*   <dir of libpirip_hip.so>/../data/<codename>.code (rtl_fsk --code's rule). codec2's      */
/*   H_256_512_4 is not part of this build: open returns NULL with a note unless a file of   */
/*   that name has been dropped in.                                                           */
/* ----------------------------------------------------------------------------------- */
#ifndef PIRIP_NO_CODEC2_SHIM
#define FREEDV_MODE_FSK_LDPC 9
#define FREEDV_RX_TRIAL_SYNC 0x1
#define FREEDV_RX_SYNC       0x2
#define FREEDV_RX_BITS       0x4
#define FREEDV_RX_BIT_ERRORS 0x8
struct freedv;
struct freedv_advanced {
    int interleave_frames;     /* unused, kept for layout */
    int M;                     /* 2 or 4 */
    int Rs;                    /* symbol rate, Hz */
    int Fs;                    /* sample rate, Hz */
    int first_tone;            /* Tx only; rpitx_fsk leaves it unset: any value is accepted */
    int tone_spacing;          /* Tx, and the comb of the mask estimator */
    char *codename;            /* LDPC code name, see above */
};
struct freedv *freedv_open_advanced(int mode, struct freedv_advanced *adv);   /* mode must be FREEDV_MODE_FSK_LDPC */
void freedv_close(struct freedv *f);
int freedv_nin(struct freedv *f);                          /* samples the next freedv_rawdatacomprx() reads */
int freedv_get_n_max_modem_samples(struct freedv *f);     /* upper bound of freedv_nin() */
/* one demodulator call: nin complex float samples in; returns the number of payload bytes written to packed_payload_bits --
 * freedv_get_bits_per_modem_frame()/8 when a frame with a good CRC16 came out of this call (FREEDV_RX_BITS), else 0 */
int freedv_rawdatacomprx(struct freedv *f, unsigned char *packed_payload_bits, COMP demod_in[]);
int freedv_get_rx_status(struct freedv *f);                /* FREEDV_RX_* of the last call */
int freedv_get_bits_per_modem_frame(struct freedv *f);    /* data bits per frame, CRC16 included (256 for a (512,256) code) */
void freedv_set_frames_per_burst(struct freedv *f, int framesperburst);   /* Tx-side burst length; stored */
void freedv_set_verbose(struct freedv *f, int verbosity);  /* >= 2: one line per decoded frame on stderr, README.md:200-208's columns */
void freedv_set_test_frames(struct freedv *f, int test_frames);            /* the ecdd column of that line counts payload bit errors */
struct FSK *freedv_get_fsk(struct freedv *f);              /* the demodulator: fsk_set_freq_est_limits / _alg, f_est[], Sf[] ... */
int freedv_get_sync(struct freedv *f);                     /* 1 while the receiver holds frame sync (FREEDV_RX_SYNC of the last call) */
void freedv_get_modem_stats(struct freedv *f, int *sync, float *snr_est);
void freedv_get_modem_extended_stats(struct freedv *f, struct MODEM_STATS *stats);   /* fsk_get_demod_stats + sync */
/* Tx-side helpers "not normally exposed by the FreeDV API" that rpitx_fsk declares itself (tx/rpitx_fsk.cpp:33-40); CPU */
int freedv_tx_fsk_ldpc_bits_per_frame(struct freedv *f);   /* 32 + n */
void freedv_tx_fsk_ldpc_framer(struct freedv *f, uint8_t frame[], uint8_t payload_data[]);   /* UW + data + parity, one bit per byte */
unsigned short freedv_gen_crc16(unsigned char *data_p, int length);
void freedv_pack(unsigned char *bytes, unsigned char *bits, int nbits);
void freedv_unpack(unsigned char *bits, unsigned char *bytes, int nbits);
/* --testframes payload: upstream's generator constants are not in the reference; this is the repo's own sequence, usable Tx + Rx together */
void ofdm_generate_payload_data_bits(uint8_t payload_data_bits[], int n);
#endif
/* codename -> code file by the rule above; 1 and the path in buf when found */
int pirip_hip_find_code(const char *codename, char *buf, size_t n);

/* ----------------------------------------------------------------------------------- */
/* section D : libcsdr-compatible entry points (host buffers) [UPSTREAM-RECALLED libcsdr.h] */
/* ----------------------------------------------------------------------------------- */
#ifndef PIRIP_NO_CSDR_SHIM
typedef struct { float i; float q; } complexf;
/* Element-wise format hops of the three-process pipe (/root/reference/README.md:109), run as
 * device kernels over host buffers (upload, convert, download) -- there is no host loop. In a
 * fused receiver use section B instead, which folds both into the decimator. */
void convert_u8_f(unsigned char *input, float *output, int length);
void convert_f_s16(float *input, short *output, int length);
int  firdes_filter_len(float transition_bw);
typedef enum window_s { WINDOW_BOXCAR, WINDOW_BLACKMAN, WINDOW_HAMMING } window_t;   /* [UPSTREAM-RECALLED libcsdr.h] */
#define WINDOW_DEFAULT WINDOW_HAMMING
void firdes_lowpass_f(float *output, int length, float cutoff_rate, window_t window);
void firdes_lowpass_f_hamming(float *output, int length, float cutoff_rate); /* = firdes_lowpass_f(..., WINDOW_HAMMING) */
/* Direct-form decimating FIR on the GPU; same contract as csdr: returns outputs written,
 * consumed input = returned * decimation. Input/output are host buffers of complex float. */
int  fir_decimate_cc(complexf *input, complexf *output, int input_size, int decimation,
                     float *taps, int taps_length);
#endif

/* ----------------------------------------------------------------------------------- */
/* misc                                                                                 */
/* ----------------------------------------------------------------------------------- */
const char *pirip_hip_version(void);        /* "pirip_hip 0.2 (gfx950)": 0.2 = PIRIP_STATS_PER_FRAME 10, pirip_stream_state with rx_sig_pow / rx_nse_pow */
/* ABI check for callers that were compiled earlier than the library they are linked against (the CMake relink of INTEGRATION.md):
 * compare with the PIRIP_HIP_ABI_VERSION / PIRIP_STATS_PER_FRAME / sizeof(pirip_stream_state) of the header the caller was built with
 * and refuse to run on a mismatch -- the library writes stats_per_frame floats per frame and a stream state of that many bytes. */
#define PIRIP_HIP_ABI_VERSION 2
int pirip_hip_abi(int *abi_version, int *stats_per_frame, size_t *stream_state_bytes);
/* 1 when the arguments -- the caller's compile-time PIRIP_HIP_ABI_VERSION, PIRIP_STATS_PER_FRAME and sizeof(pirip_stream_state) -- are
 * this library's; call once at start-up: pirip_hip_abi_check(PIRIP_HIP_ABI_VERSION, PIRIP_STATS_PER_FRAME, sizeof(pirip_stream_state)) */
int pirip_hip_abi_check(int abi_version, int stats_per_frame, size_t stream_state_bytes);
/* 16 hex digits of the sha256 of the wave demodulator kernels' gfx950 code object: identifies the kernel build a measurement file
 * (profiles/hbm_traffic.json) was taken on */
const char *pirip_hip_kernel_source_hash(void);
const char *pirip_hip_strerror(int status);
int pirip_hip_device_count(void);          /* 0 when no usable HIP device                  */
/* Device self-test of the estimator's correctly rounded square roots (the |X| in Sf = Sf (1-tc) + |X| tc,
 * [UPSTREAM-RECALLED codec2 fsk.c: fsk_demod_freq_est] uses sqrtf): both device variants against (float)sqrt((double)x) for
 * x = 0 and every float in [2^-96, FLT_MAX]; *mismatches = (v_sqrt variant's count << 32) | rsq variant's count, 0 on a
 * device where the kernels' fast path is valid. ~1 s. */
int pirip_hip_selftest_sqrt(uint64_t *mismatches);
/* Device self-test of the fused FSK_LDPC hand-over's divisions by constants (the frame's sums / Nsym = 50, the other tones' power / 3:
 * x * RN(1/c) corrected by one residual step instead of the 11-instruction IEEE quotient) against the device's own x / c for x = 0 and
 * every float in [2^-125, FLT_MAX]; *mismatches = (count for / 50 << 32) | count for / 3, 0 where the kernels' quick path is valid. ~1 s. */
int pirip_hip_selftest_div(uint64_t *mismatches);
/* The exact first frame's fine-timing angle is libm's atan2f restated in device code (fdlibm's float algorithm, which glibc ships):
 * this evaluates that restatement on device arrays so that a test can compare it with the host's atan2f bit for bit. */
int pirip_hip_selftest_atan2(const float *d_y, const float *d_x, float *d_out, int n);

#ifdef __cplusplus
}
#endif
#endif /* PIRIP_HIP_H */
