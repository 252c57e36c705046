/* tests/cprog/chan_like_multichannel.c -- one wideband capture -> K FSK channels -> bits, written against include/pirip_hip.h sections H
 * and G only, as plain C: a 2.4 MS/s u8 IQ capture, eight channels 250 kHz apart, each decimated by 30 to 80 kS/s complex float and
 * demodulated as rtl_fsk -a 80000 -r 10000 would, blocks landed straight in the receiver's input. Compiled and linked by
 * tests/test_channelizer_cpu.py (syntax and link only): it is the shape of a caller, not a test that runs. */
#include <stdint.h>
#include <stdio.h>

#include "pirip_hip.h"

int receive(int blocks, uint8_t *d_bits, int32_t *d_nframes, void *hip_stream, void (*capture)(void *d_block, size_t stride, int64_t block))
{
    const int32_t offsets[8] = {-875000, -625000, -375000, -125000, 125000, 375000, 625000, 875000};
    const int32_t inputs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t block = 30 * 20000;
    pirip_fsk_params p = {80000, 10000, 2, 8, PIRIP_FSK_DEFAULT_NSYM, 5000, 40000, 0, 0, PIRIP_IN_CF32};
    pirip_hip_chan *chan = NULL;
    pirip_hip_demod *dem = NULL;
    pirip_hip_rx *rx = NULL;
    int rc = pirip_hip_chan_create(2400000, 30, 0.05f, 0, 1, 8, inputs, offsets, -1, &chan);
    if (rc == PIRIP_OK) rc = pirip_hip_create(&p, 8, -1, &dem);
    if (rc == PIRIP_OK) rc = pirip_hip_rx_create_chan(dem, NULL, chan, block, &rx);
    if (rc != PIRIP_OK) { fprintf(stderr, "create: %s\n", pirip_hip_strerror(rc)); return rc; }
    pirip_chan_info ci;
    pirip_fsk_info info;
    pirip_hip_chan_get_info(chan, &ci);
    pirip_hip_get_info(dem, &info);
    fprintf(stderr, "%d channels of %d input(s), D %d, %d taps (%d padded), %lld outputs per channel per block\n", ci.nchan, ci.ninputs, ci.D,
            ci.ntaps, ci.ntaps_padded, (long long)(block / ci.D));
    const int64_t rows = pirip_hip_rx_max_frames(rx);
    for (int b = 0; b < blocks && rc == PIRIP_OK; b++) {
        void *d_block = NULL;
        size_t stride = 0;
        rc = pirip_hip_rx_input(rx, &d_block, &stride);
        if (rc != PIRIP_OK) break;
        capture(d_block, stride, block);
        rc = pirip_hip_rx_process(rx, d_bits, (size_t)(rows * info.Nbits), NULL, 0, NULL, NULL, NULL, NULL, 0, d_nframes, hip_stream);
    }
    if (rc == PIRIP_OK) rc = pirip_hip_rx_reset(rx, hip_stream);
    pirip_hip_rx_destroy(rx);
    pirip_hip_destroy(dem);
    pirip_hip_chan_destroy(chan);
    return rc;
}

/* the stateless form: every channel of every capture of one call */
int channelize(const uint8_t *d_captures, size_t capture_stride, int64_t n_in, int64_t t0, float *d_out, size_t out_stride, void *hip_stream)
{
    const int32_t offsets[3] = {-300000, 0, 450001};
    const int32_t inputs[3] = {1, 0, 1};
    pirip_hip_chan *chan = NULL;
    int rc = pirip_hip_chan_create(1800000, 45, 0.05f, 0, 2, 3, inputs, offsets, -1, &chan);
    if (rc != PIRIP_OK) return rc;
    fprintf(stderr, "%lld outputs per channel\n", (long long)pirip_hip_chan_nout(chan, n_in));
    rc = pirip_hip_chan_batch(chan, d_captures, capture_stride, n_in, t0, d_out, out_stride, hip_stream);
    pirip_hip_chan_destroy(chan);
    return rc;
}

int main(void) { return 0; }
