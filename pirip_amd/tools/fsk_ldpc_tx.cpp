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

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tool_common.hpp"
#include "tx_records.hpp"

using namespace pirip;

static int usage(const char *a0)
{
    fprintf(stderr, "usage: %s --code FILE [-m 2|4] [--packed] [--testframes N [--bursts B]] [--source BYTE] [--seq] [--gap BITS] [--lead BITS]\n"
                    "          [--format u8|cf32] [--amp A] Fs Rs f1 shift in|- out|-\n", a0);
    return 1;
}

// every failure behind pirip_hip_tx_create is the device's
static const ToolErrors kTool{"fsk_ldpc_tx", [](int) { return 3; }};

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
    File fin(strcmp(argv[optind + 4], "-") ? fopen(argv[optind + 4], "rb") : stdin);
    if (!fin) { fprintf(stderr, "fsk_ldpc_tx: couldn't open the input\n"); return 1; }

    // the record stream, packed
    const int k = code.k, rl = 1 + k / 8;
    std::vector<uint8_t> recs;
    if (testframes > 0) testframe_records(k, testframes, bursts, source, seq, recs);
    else read_records(fin, k, packed, recs);
    const int nrec = (int)(recs.size() / (size_t)rl);
    fprintf(stderr, "fsk_ldpc_tx: code %s data_bits_per_frame %d bits_per_frame %d M %d records %d\n", code.name.c_str(), k, code.bits_per_frame(), M, nrec);

    TxHandle tx;
    const int rc = pirip_hip_tx_create(code_path.c_str(), Fs, Rs, M, 1, -1, tx.out());
    if (rc != PIRIP_OK) return status_fail(ToolErrors{kTool.name, tx_create_exit_code}, "pirip_hip_tx_create", rc);
    const int32_t f1a = f1, leada = lead / bps, gapa = gap / bps;
    PIRIPOK(pirip_hip_tx_set_tones(tx, &f1a, shift), "pirip_hip_tx_set_tones");
    PIRIPOK(pirip_hip_tx_set_gaps(tx, &leada, &gapa), "pirip_hip_tx_set_gaps");
    const int64_t cap = pirip_hip_tx_max_syms(tx, nrec) > 0 ? pirip_hip_tx_max_syms(tx, nrec) : 1;
    const int bsamp = format == "u8" ? 2 : 8, Ts = Fs / Rs;
    DevBuf<uint8_t> d_rec, d_syms;
    DevBuf<int32_t> d_nsym;
    DevBuf<void> d_out;
    if (hipMalloc((void **)d_rec.out(), recs.size() + 1) != hipSuccess || hipMalloc((void **)d_syms.out(), (size_t)cap) != hipSuccess ||
        hipMalloc((void **)d_nsym.out(), sizeof(int32_t)) != hipSuccess) return status_fail(kTool, "hipMalloc", PIRIP_ERR_NOMEM);
    if (!recs.empty() && hipMemcpy(d_rec, recs.data(), recs.size(), hipMemcpyHostToDevice) != hipSuccess) return status_fail(kTool, "hipMemcpy", PIRIP_ERR_HIP);
    PIRIPOK(pirip_hip_tx_frame(tx, d_rec, recs.size() + 1, nullptr, nrec, d_syms, (size_t)cap, cap, d_nsym, nullptr, 0, nullptr), "pirip_hip_tx_frame");
    int32_t nsym = 0;
    if (hipMemcpy(&nsym, d_nsym, sizeof(nsym), hipMemcpyDeviceToHost) != hipSuccess) return status_fail(kTool, "hipMemcpy", PIRIP_ERR_HIP);
    const size_t out_bytes = (size_t)nsym * (size_t)Ts * (size_t)bsamp;
    std::vector<uint8_t> out(out_bytes);
    if (nsym > 0) {
        if (hipMalloc(d_out.out(), out_bytes) != hipSuccess) return status_fail(kTool, "hipMalloc", PIRIP_ERR_NOMEM);
        PIRIPOK(pirip_hip_tx_modulate(tx, d_syms, (size_t)cap, d_nsym, nsym, format == "u8" ? PIRIP_IN_CU8_FSKDEMOD : PIRIP_IN_CF32, d_out, out_bytes,
                                      amp, 0.0f, 0, nullptr), "pirip_hip_tx_modulate");
        if (hipMemcpy(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost) != hipSuccess) return status_fail(kTool, "hipMemcpy", PIRIP_ERR_HIP);
    }
    File fout(strcmp(argv[optind + 5], "-") ? fopen(argv[optind + 5], "wb") : stdout);
    if (!fout) { fprintf(stderr, "fsk_ldpc_tx: couldn't open the output\n"); return 1; }
    if (fwrite(out.data(), 1, out.size(), fout) != out.size()) { fprintf(stderr, "fsk_ldpc_tx: short write\n"); return 1; }
    fprintf(stderr, "fsk_ldpc_tx: %d symbols, %zu samples\n", nsym, (size_t)nsym * Ts);
    return 0;
}
