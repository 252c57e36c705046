/* tests/cprog/stream_rx_like_multichannel.c -- a live N-channel receive loop written against include/pirip_hip.h section G only,
 * as plain C: a csdr front end (u8 IQ at 240 kS/s, /6 -> complex float) into an rtl_fsk -a 40000 -r 1000 demodulator per channel,
 * blocks landed straight in the receiver's input, frames out of every call. Compiled and linked by tests/test_stream_rx_cpu.py
 * (syntax and link only): it is the shape of a caller, not a test that runs. Device buffers come from the caller's allocator
 * (hipMalloc in a real program), so the loop takes them as arguments. */
#include <stdint.h>
#include <stdio.h>

#include "pirip_hip.h"

int receive(int nch, int blocks, uint8_t *d_bits, int32_t *d_nframes, void *hip_stream,
            void (*capture)(void *d_block, size_t stride, int nch, int64_t block))
{
    pirip_fsk_params p = {40000, 1000, 2, 10, PIRIP_FSK_DEFAULT_NSYM, 500, 15000, 0, 0, PIRIP_IN_CF32};
    pirip_hip_demod *dem = NULL;
    pirip_hip_decim *dec = NULL;
    pirip_hip_rx *rx = NULL;
    int rc = pirip_hip_create(&p, nch, -1, &dem);
    if (rc == PIRIP_OK) rc = pirip_hip_decim_create(6, 0.05f, 0, -1, &dec);
    if (rc == PIRIP_OK) rc = pirip_hip_rx_create(dem, NULL, dec, 6 * 4000, &rx);
    if (rc != PIRIP_OK) { fprintf(stderr, "create: %s\n", pirip_hip_strerror(rc)); return rc; }
    pirip_fsk_info info;
    pirip_hip_get_info(dem, &info);
    const int64_t rows = pirip_hip_rx_max_frames(rx);
    for (int b = 0; b < blocks && rc == PIRIP_OK; b++) {
        void *d_block = NULL;
        size_t stride = 0;
        rc = pirip_hip_rx_input(rx, &d_block, &stride);
        if (rc != PIRIP_OK) break;
        capture(d_block, stride, nch, 6 * 4000);
        rc = pirip_hip_rx_process(rx, d_bits, (size_t)(rows * info.Nbits), NULL, 0, NULL, NULL, NULL, NULL, 0, d_nframes, hip_stream);
    }
    int64_t consumed = 0;
    int32_t backlog = 0;
    if (rc == PIRIP_OK && nch == 1) rc = pirip_hip_rx_get_counters(rx, &consumed, &backlog);
    if (rc == PIRIP_OK) fprintf(stderr, "consumed %lld backlog %d (< %d)\n", (long long)consumed, backlog, info.nin_max);
    if (rc == PIRIP_OK) rc = pirip_hip_rx_reset(rx, hip_stream);
    pirip_hip_rx_destroy(rx);
    pirip_hip_decim_destroy(dec);
    pirip_hip_destroy(dem);
    return rc;
}

int main(void) { return 0; }
