// iq_spectrum -- the band monitor on a wideband IQ file, on the GPU: averaged power spectra and the power and peak of a list of bands, one
// call per block (include/pirip_hip.h section P). What the reference shows with script/dash.py behind rtl_fsk, one stage earlier: on the
// capture itself, before any channel is picked.
//
//   iq_spectrum --fs FS [--format u8|cf32] --nfft N [--half-overlap] [--avg A] [--band lo:hi]... [--block SAMPLES] [--dash] in|-
//
// --band (repeated): a band from lo to hi Hz, integers, -FS/2 <= lo <= hi < FS/2. Per complete row and band one line on stdout:
//   row R band Q power_db P peak_hz F
// P: the band's mean power per bin, 10 log10(power scale / bins); F: the frequency of its largest bin. With --dash, instead, one JSON line per
// row with the keys script/dash.py reads: SfdB (the row in dB, from -FS/2 upward) and Fs_Hz, f_est_Hz (the bands' peak frequencies),
// fsk_lower_Hz / fsk_upper_Hz (the first band's edges, 0 without a band), SNRest_lin 0 and norm_rx_timing []: iq_spectrum --dash ... | dash.py
// shows the wideband view. --block: samples per call (default 65536).
// Exit codes: 1 arguments / files, 2 a handle that cannot be made, 3 a device error.
#include <getopt.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tool_common.hpp"

static int usage()
{
    fprintf(stderr, "iq_spectrum (pirip_hip): --fs FS [--format u8|cf32] --nfft N [--half-overlap] [--avg A] [--band lo:hi]... [--block SAMPLES] [--dash] in|-\n");
    return 1;
}

static const ToolErrors kTool{"iq_spectrum", [](int status) { return status == PIRIP_ERR_HIP ? 3 : 2; }};
using SpecHandle = Owned<pirip_hip_spec, pirip_hip_spec_destroy>;

// the frequency of FFT bin b: bins from nfft / 2 on are the negative frequencies
static double bin_hz(int b, int nfft, long Fs) { return (double)(b < nfft / 2 ? b : b - nfft) * (double)Fs / (double)nfft; }

int main(int argc, char **argv)
{
    if (!abi_ok(argv[0])) return 2;
    long Fs = 0;
    int in_format = PIRIP_IN_CU8_CSDR, nfft = 0, half = 0, avg = 1, dash = 0;
    long long block = 65536;
    std::vector<pirip_spec_band> bands;
    static struct option lopts[] = {{"fs", required_argument, 0, 1000}, {"format", required_argument, 0, 1001}, {"nfft", required_argument, 0, 1002},
                                    {"half-overlap", no_argument, 0, 1003}, {"avg", required_argument, 0, 1004}, {"band", required_argument, 0, 1005},
                                    {"block", required_argument, 0, 1006}, {"dash", no_argument, 0, 1007}, {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};
    int o, oi;
    while ((o = getopt_long(argc, argv, "h", lopts, &oi)) != -1) {
        switch (o) {
        case 1000: Fs = (long)atof(optarg); break;
        case 1001:
            if (!strcmp(optarg, "u8")) in_format = PIRIP_IN_CU8_CSDR;
            else if (!strcmp(optarg, "cf32")) in_format = PIRIP_IN_CF32;
            else return usage();
            break;
        case 1002: nfft = atoi(optarg); break;
        case 1003: half = 1; break;
        case 1004: avg = atoi(optarg); break;
        case 1005: {
            char *e = nullptr;
            const long lo = strtol(optarg, &e, 10);
            if (e == optarg || *e != ':') { fprintf(stderr, "iq_spectrum: --band wants lo:hi in integer Hz\n"); return 1; }
            const char *s = e + 1;
            const long hi = strtol(s, &e, 10);
            if (e == s || *e) { fprintf(stderr, "iq_spectrum: --band wants lo:hi in integer Hz\n"); return 1; }
            bands.push_back(pirip_spec_band{0, (int32_t)lo, (int32_t)hi});
            break;
        }
        case 1006: block = atoll(optarg); break;
        case 1007: dash = 1; break;
        default: return usage();
        }
    }
    if (Fs <= 0 || nfft <= 0 || block <= 0 || optind + 1 != argc) return usage();
    File fin(!strcmp(argv[optind], "-") ? stdin : fopen(argv[optind], "rb"));
    if (!fin) { fprintf(stderr, "iq_spectrum: can't open %s\n", argv[optind]); return 1; }

    const int hop = half ? nfft / 2 : nfft, nbands = (int)bands.size();
    SpecHandle spec;
    PIRIPOK(pirip_hip_spec_create((int)Fs, in_format, nfft, hop, avg, 1, nbands, bands.data(), -1, spec.out()), "band monitor (--fs / --nfft / --avg / --band)");
    pirip_spec_info info;
    PIRIPOK(pirip_hip_spec_get_info(spec, &info), "info");
    std::vector<int32_t> nbins((size_t)nbands);
    for (int q = 0; q < nbands; q++) PIRIPOK(pirip_hip_spec_band_bins(spec, q, nullptr, &nbins[(size_t)q]), "band");

    const size_t bsi = in_format == PIRIP_IN_CF32 ? 8 : 2;
    const size_t max_rows = (size_t)(block / hop / avg) + 1;           // a block completes at most this many rows
    DevBuf<void> d_in;
    DevBuf<float> d_rows;
    DevBuf<pirip_spec_band_row> d_bands;
    HIPOK(hipMalloc(d_in.out(), (size_t)block * bsi));
    HIPOK(hipMalloc((void **)d_rows.out(), max_rows * (size_t)nfft * sizeof(float)));
    HIPOK(hipMalloc((void **)d_bands.out(), (max_rows * (size_t)nbands + 1) * sizeof(pirip_spec_band_row)));
    std::vector<uint8_t> raw((size_t)block * bsi);
    std::vector<float> rows(max_rows * (size_t)nfft);
    std::vector<pirip_spec_band_row> entries(max_rows * (size_t)nbands + 1);
    long long row = 0;
    for (;;) {
        const size_t n = fread(raw.data(), bsi, (size_t)block, fin);
        if (n == 0) break;
        HIPOK(hipMemcpy(d_in, raw.data(), n * bsi, hipMemcpyHostToDevice));
        const int64_t m = pirip_hip_spec_nrows(spec, (int64_t)n);
        if (m < 0) return status_fail(kTool, "rows", (int)m);
        PIRIPOK(pirip_hip_spec_push(spec, d_in, 0, (int64_t)n, dash ? (float *)d_rows : nullptr, (size_t)nfft, 0, nbands ? (pirip_spec_band_row *)d_bands : nullptr,
                                    max_rows, nullptr), "push");
        if (m > 0 && dash) HIPOK(hipMemcpy(rows.data(), d_rows, (size_t)m * (size_t)nfft * sizeof(float), hipMemcpyDeviceToHost));
        if (m > 0 && nbands) HIPOK(hipMemcpy(entries.data(), d_bands, max_rows * (size_t)nbands * sizeof(pirip_spec_band_row), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < m; i++, row++) {
            if (!dash) {
                for (int q = 0; q < nbands; q++) {
                    const pirip_spec_band_row &e = entries[(size_t)q * max_rows + (size_t)i];
                    printf("row %lld band %d power_db %.4f peak_hz %.3f\n", row, q, 10.0 * log10((double)e.power * info.scale / (double)nbins[(size_t)q] + 1e-30),
                           bin_hz(e.peak_bin, nfft, Fs));
                }
                continue;
            }
            printf("{\"SfdB\": [");
            for (int k = 0; k < nfft; k++)
                printf("%s%.3f", k ? ", " : "", 10.0 * log10((double)rows[(size_t)i * (size_t)nfft + (size_t)((k + nfft / 2) % nfft)] * info.scale + 1e-30));
            printf("], \"Fs_Hz\": %ld, \"f_est_Hz\": [", Fs);
            for (int q = 0; q < nbands; q++) printf("%s%.3f", q ? ", " : "", bin_hz(entries[(size_t)q * max_rows + (size_t)i].peak_bin, nfft, Fs));
            printf("], \"fsk_lower_Hz\": %d, \"fsk_upper_Hz\": %d, \"SNRest_lin\": 0, \"norm_rx_timing\": []}\n", nbands ? bands[0].lo_hz : 0,
                   nbands ? bands[0].hi_hz : 0);
        }
        fflush(stdout);
        if (n < (size_t)block) break;
    }
    return 0;
}
