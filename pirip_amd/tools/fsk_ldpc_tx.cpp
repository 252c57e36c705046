// fsk_ldpc_tx -- pirip's transmitter without the RF, on the GPU: what `rpitx_fsk --code NAME` does to its stdin
// (/root/reference/tx/rpitx_fsk.cpp:427-509) and the FSK modulator behind it, through include/pirip_hip.h section I.
// fsk_ldpc_framer's arguments, plus the modem's and an output format:
//
//   fsk_ldpc_tx --code FILE [-m M] [--packed] [--source BYTE] [--seq] [--gap BITS] [--lead BITS] [--format u8|cf32] [--amp A]
//               Fs Rs f1 shift In|- Out|-
//       In: records of one burst-control byte + data_bits_per_frame bits (one per byte) or, with --packed, /8 bytes
//       (1 = preamble + frame, 0 = frame, 2 = end of burst: carrier off for --gap). This is what tx/frame_repeater.c:92-104 writes.
//   fsk_ldpc_tx --code FILE --testframes N [--bursts B] [...] Fs Rs f1 shift /dev/zero Out|-
//       rpitx_fsk's test-frame mode (:366-421), as fsk_ldpc_framer --testframes.
// Out: IQ at Fs -- u8 (127 + amp * x rounded, `fsk_demod -d` / rtl_fsk input) or complex float -- of the whole input in one piece, with
// zero signal over --lead, over every --gap and nowhere else, so that `fsk_ldpc_tx ... | rtl_fsk --code ...` runs as a pipe.
// Not a streaming pipe: the whole input is read, framed and modulated in one piece before the first byte is written (right for the finite
// --testframes and file cases; a live repeater drives the handle block after block through the library instead).
// Exit codes: 1 arguments / files, 2 the code file (as fsk_ldpc_framer), 3 no usable HIP device or a device error (nothing is written).
#include <getopt.h>
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pirip_hip.h"
#include "fsk_ldpc.hpp"

using namespace pirip;

static int usage(const char *a0)
{
    fprintf(stderr, "usage: %s --code FILE [-m 2|4] [--packed] [--testframes N [--bursts B]] [--source BYTE] [--seq] [--gap BITS] [--lead BITS]\n"
                    "          [--format u8|cf32] [--amp A] Fs Rs f1 shift in|- out|-\n", a0);
    return 1;
}

int main(int argc, char **argv)
{
    std::string code_path, format = "u8";
    int M = 2, packed = 0, testframes = 0, bursts = 1, source = -1, seq = 0, gap = 0, lead = 0;
    float amp = 32.0f;
    static struct option lopts[] = {{"code", required_argument, 0, 1000}, {"packed", no_argument, 0, 1001},
                                    {"testframes", required_argument, 0, 1002}, {"bursts", required_argument, 0, 1003},
                                    {"source", required_argument, 0, 1004}, {"seq", no_argument, 0, 1005},
                                    {"gap", required_argument, 0, 1006}, {"lead", required_argument, 0, 1007},
                                    {"format", required_argument, 0, 1008}, {"amp", required_argument, 0, 1009}, {0, 0, 0, 0}};
    int o, oi;
    while ((o = getopt_long(argc, argv, "m:h", lopts, &oi)) != -1) {
        switch (o) {
        case 'm': M = atoi(optarg); break;
        case 1000: code_path = optarg; break;
        case 1001: packed = 1; break;
        case 1002: testframes = atoi(optarg); break;
        case 1003: bursts = atoi(optarg); break;
        case 1004: source = (int)strtol(optarg, nullptr, 0); break;
        case 1005: seq = 1; break;
        case 1006: gap = atoi(optarg); break;
        case 1007: lead = atoi(optarg); break;
        case 1008: format = optarg; break;
        case 1009: amp = (float)atof(optarg); break;
        default: return usage(argv[0]);
        }
    }
    if (argc - optind < 6 || code_path.empty() || (M != 2 && M != 4)) { fprintf(stderr, "fsk_ldpc_tx: need --code FILE, -m 2|4, Fs Rs f1 shift, input and output\n"); return usage(argv[0]); }
    const int Fs = atoi(argv[optind]), Rs = atoi(argv[optind + 1]), f1 = atoi(argv[optind + 2]), shift = atoi(argv[optind + 3]);
    const int bps = M == 2 ? 1 : 2;
    if (Fs <= 0 || Rs <= 0 || Fs % Rs || shift <= 0) { fprintf(stderr, "fsk_ldpc_tx: need Fs > 0, Rs > 0, Fs %% Rs == 0 and shift > 0\n"); return 1; }
    if (format != "u8" && format != "cf32") { fprintf(stderr, "fsk_ldpc_tx: --format u8|cf32\n"); return 1; }
    if (gap < 0 || lead < 0 || gap % bps || lead % bps || bursts < 1 || testframes < 0) { fprintf(stderr, "fsk_ldpc_tx: --gap / --lead are whole symbols, --bursts >= 1\n"); return 1; }
    LdpcCode code;
    const std::string err = code.load(code_path);
    if (!err.empty()) { fprintf(stderr, "fsk_ldpc_tx: %s: %s\n", code_path.c_str(), err.c_str()); return 2; }
    if (!code.accumulator) { fprintf(stderr, "fsk_ldpc_tx: %s has no dual-diagonal parity part: no linear-time encoder\n", code.name.c_str()); return 2; }
    FILE *fin = strcmp(argv[optind + 4], "-") ? fopen(argv[optind + 4], "rb") : stdin;
    if (!fin) { fprintf(stderr, "fsk_ldpc_tx: couldn't open the input\n"); return 1; }

    // the record stream, packed
    const int k = code.k, kb = k / 8, rl = 1 + kb;
    std::vector<uint8_t> recs, data((size_t)k), bytes((size_t)kb);
    auto push = [&](uint8_t ctl) { recs.push_back(ctl); recs.insert(recs.end(), bytes.begin(), bytes.end()); };
    if (testframes > 0) {
        testframe_payload(data.data(), k);
        for (int b = 0; b < bursts; b++) {
            for (int f = 0; f < testframes; f++) {
                if (source >= 0) for (int i = 0; i < 8; i++) data[i] = (source >> (7 - i)) & 1;
                if (seq) { const int s = (f + 1) & 0xff; for (int i = 0; i < 8; i++) data[8 + i] = (s >> (7 - i)) & 1; }
                pack_bits_msb(bytes.data(), data.data(), k);
                push(f == 0 ? 1 : 0);
            }
            std::fill(bytes.begin(), bytes.end(), 0);
            push(2);
        }
    } else {
        for (;;) {
            uint8_t ctl;
            if (fread(&ctl, 1, 1, fin) != 1) break;
            size_t nread;
            if (packed) nread = fread(bytes.data(), 1, bytes.size(), fin) * 8;
            else { nread = fread(data.data(), 1, (size_t)k, fin); pack_bits_msb(bytes.data(), data.data(), k); }
            if ((int)nread != k) break;
            push(ctl);
        }
    }
    const int nrec = (int)(recs.size() / (size_t)rl);
    fprintf(stderr, "fsk_ldpc_tx: code %s data_bits_per_frame %d bits_per_frame %d M %d records %d\n", code.name.c_str(), k, code.bits_per_frame(), M, nrec);

    pirip_hip_tx *tx = nullptr;
    int rc = pirip_hip_tx_create(code_path.c_str(), Fs, Rs, M, 1, -1, &tx);
    if (rc != PIRIP_OK) { fprintf(stderr, "fsk_ldpc_tx: pirip_hip_tx_create: %s\n", pirip_hip_strerror(rc)); return rc == PIRIP_ERR_BAD_CONFIG || rc == PIRIP_ERR_UNSUPPORTED ? 2 : 3; }
    const int32_t f1a = f1, leada = lead / bps, gapa = gap / bps;
    auto fail = [&](const char *what, int status) { fprintf(stderr, "fsk_ldpc_tx: %s: %s\n", what, pirip_hip_strerror(status)); pirip_hip_tx_destroy(tx); return 3; };
    if ((rc = pirip_hip_tx_set_tones(tx, &f1a, shift)) != PIRIP_OK) return fail("pirip_hip_tx_set_tones", rc);
    if ((rc = pirip_hip_tx_set_gaps(tx, &leada, &gapa)) != PIRIP_OK) return fail("pirip_hip_tx_set_gaps", rc);
    const int64_t cap = pirip_hip_tx_max_syms(tx, nrec) > 0 ? pirip_hip_tx_max_syms(tx, nrec) : 1;
    const int bsamp = format == "u8" ? 2 : 8, Ts = Fs / Rs;
    uint8_t *d_rec = nullptr, *d_syms = nullptr; int32_t *d_nsym = nullptr; void *d_out = nullptr;
    if (hipMalloc((void **)&d_rec, recs.size() + 1) != hipSuccess || hipMalloc((void **)&d_syms, (size_t)cap) != hipSuccess ||
        hipMalloc((void **)&d_nsym, sizeof(int32_t)) != hipSuccess) return fail("hipMalloc", PIRIP_ERR_NOMEM);
    if (!recs.empty() && hipMemcpy(d_rec, recs.data(), recs.size(), hipMemcpyHostToDevice) != hipSuccess) return fail("hipMemcpy", PIRIP_ERR_HIP);
    if ((rc = pirip_hip_tx_frame(tx, d_rec, recs.size() + 1, nullptr, nrec, d_syms, (size_t)cap, cap, d_nsym, nullptr, 0, nullptr)) != PIRIP_OK)
        return fail("pirip_hip_tx_frame", rc);
    int32_t nsym = 0;
    if (hipMemcpy(&nsym, d_nsym, sizeof(nsym), hipMemcpyDeviceToHost) != hipSuccess) return fail("hipMemcpy", PIRIP_ERR_HIP);
    const size_t out_bytes = (size_t)nsym * (size_t)Ts * (size_t)bsamp;
    std::vector<uint8_t> out(out_bytes);
    if (nsym > 0) {
        if (hipMalloc(&d_out, out_bytes) != hipSuccess) return fail("hipMalloc", PIRIP_ERR_NOMEM);
        rc = pirip_hip_tx_modulate(tx, d_syms, (size_t)cap, d_nsym, nsym, format == "u8" ? PIRIP_IN_CU8_FSKDEMOD : PIRIP_IN_CF32, d_out, out_bytes,
                                   amp, 0.0f, 0, nullptr);
        if (rc != PIRIP_OK) return fail("pirip_hip_tx_modulate", rc);
        if (hipMemcpy(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail("hipMemcpy", PIRIP_ERR_HIP);
    }
    (void)hipFree(d_rec); (void)hipFree(d_syms); (void)hipFree(d_nsym); if (d_out) (void)hipFree(d_out);
    pirip_hip_tx_destroy(tx);
    FILE *fout = strcmp(argv[optind + 5], "-") ? fopen(argv[optind + 5], "wb") : stdout;
    if (!fout) { fprintf(stderr, "fsk_ldpc_tx: couldn't open the output\n"); return 1; }
    if (fwrite(out.data(), 1, out.size(), fout) != out.size()) { fprintf(stderr, "fsk_ldpc_tx: short write\n"); return 1; }
    if (fout != stdout) fclose(fout);
    fprintf(stderr, "fsk_ldpc_tx: %d symbols, %zu samples\n", nsym, (size_t)nsym * Ts);
    return 0;
}
