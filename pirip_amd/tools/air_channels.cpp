// air_channels -- the radio channel between wideband IQ files, on the GPU: what lies between the reference's terminals, "a 60 dB attenuator"
// or the air (its test/loopback_rtl_fsk.sh and README "MDS tests"), as one call per block of the channel (include/pirip_hip.h section O).
//
//   air_channels --fs Fs [--in-format u8|cf32] [--out-format u8|cf32] [--path rx,tx,gain,delay,offset[,ppb]]... [--max-slip N]
//                [--fade path,doppler_millihz,rice_k[,key]]... [--sigma s0,s1,...] [--seed N] [--block N] [--start n0] [-q] IN_0 ... IN_{T-1} -- OUT_0 ... OUT_{R-1}
//
// T input files, one per transmitter, and behind "--" R output files, one per receiver. --path (repeated, in path order): received stream,
// transmitted stream, real gain, delay in samples, carrier offset in integer Hz and, optionally, the clock offset of the path's transmitter
// in parts per billion, which wants --max-slip N: the whole samples such a path may slip before the tool stops (section O, drift; without
// either the tool makes what it made before them). --fade (repeated): the path of that index, counted in --path order from 0, gets a
// Rayleigh (rice_k 0) or Rician gain with a Doppler spread in millihertz, drawn with the key (default 0) (section O, fading; without it
// the tool makes what it makes without). --sigma: one value for every receiver, or one per receiver
// (default 0). --start: the absolute index of the first sample (default 0; earlier samples are zero). --block: samples per call (default
// 65536); the files are read block by block to the end of the shortest input, the last block as long as what is left, and every block is
// written as it is made.
// Exit codes: 1 arguments / files, 2 a handle that cannot be made, 3 a device error.
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "tool_common.hpp"

static int usage()
{
    fprintf(stderr,
            "air_channels (pirip_hip): --fs Fs [--in-format u8|cf32] [--out-format u8|cf32] [--path rx,tx,gain,delay,offset[,ppb]]...\n"
            "        [--max-slip N] [--fade path,doppler_millihz,rice_k[,key]]... [--sigma s0,s1,...] [--seed N] [--block N] [--start n0] [-q] IN_0 ... IN_{T-1} -- OUT_0 ... OUT_{R-1}\n");
    return 1;
}

static const ToolErrors kTool{"air_channels", [](int status) { return status == PIRIP_ERR_HIP ? 3 : 2; }};
using AirHandle = Owned<pirip_hip_air, pirip_hip_air_destroy>;

static bool parse_format(const char *s, int *fmt)
{
    if (!strcmp(s, "u8")) { *fmt = PIRIP_IN_CU8_CSDR; return true; }
    if (!strcmp(s, "cf32")) { *fmt = PIRIP_IN_CF32; return true; }
    return false;
}

int main(int argc, char **argv)
{
    if (!abi_ok(argv[0])) return 2;
    long Fs = 0;
    int in_format = PIRIP_IN_CU8_CSDR, out_format = PIRIP_IN_CU8_CSDR, quiet = 0;
    long long block = 65536, start = 0, max_slip = 0;
    bool drift = false;
    unsigned long long seed = 1;
    std::vector<pirip_air_path_ex> paths;
    std::vector<pirip_air_fade> fades;
    std::vector<float> sigma;
    static struct option lopts[] = {{"fs", required_argument, 0, 1000}, {"in-format", required_argument, 0, 1001},
                                    {"out-format", required_argument, 0, 1002}, {"path", required_argument, 0, 1003},
                                    {"sigma", required_argument, 0, 1004}, {"seed", required_argument, 0, 1005}, {"block", required_argument, 0, 1006},
                                    {"start", required_argument, 0, 1007}, {"max-slip", required_argument, 0, 1008}, {"fade", required_argument, 0, 1009}, {"help", no_argument, 0, 'h'},
                                    {0, 0, 0, 0}};
    int o, oi;
    // ("+": the first file name ends the options, so that "--" stays where it separates inputs from outputs)
    while ((o = getopt_long(argc, argv, "+qh", lopts, &oi)) != -1) {
        switch (o) {
        case 'q': quiet = 1; break;
        case 1000: Fs = (long)atof(optarg); break;
        case 1001: if (!parse_format(optarg, &in_format)) return usage(); break;
        case 1002: if (!parse_format(optarg, &out_format)) return usage(); break;
        case 1003: {
            std::vector<double> v;
            if (!parse_list(optarg, v, strtod) || (v.size() != 5 && v.size() != 6) || v[0] != (double)(int32_t)v[0] || v[1] != (double)(int32_t)v[1] ||
                v[3] != (double)(int32_t)v[3] || v[4] != (double)(int32_t)v[4] || (v.size() == 6 && v[5] != (double)(int32_t)v[5])) {
                fprintf(stderr, "air_channels: --path wants rx,tx,gain,delay,offset[,ppb]: integers but for the gain\n");
                return 1;
            }
            paths.push_back(pirip_air_path_ex{(int32_t)v[0], (int32_t)v[1], (int32_t)v[3], (int32_t)v[4], (float)v[2], v.size() == 6 ? (int32_t)v[5] : 0});
            drift = drift || paths.back().clock_ppb != 0;
            break;
        }
        case 1004: if (!parse_list(optarg, sigma, conv_float)) { fprintf(stderr, "air_channels: --sigma s or --sigma s0,s1,...\n"); return 1; } break;
        case 1005: seed = strtoull(optarg, nullptr, 0); break;
        case 1006: block = atoll(optarg); break;
        case 1007: start = atoll(optarg); break;
        case 1008: max_slip = atoll(optarg); break;
        case 1009: {
            std::vector<double> v;
            if (!parse_list(optarg, v, strtod) || (v.size() != 3 && v.size() != 4) || v[0] != (double)(int32_t)v[0] || v[1] != (double)(int32_t)v[1] ||
                (v.size() == 4 && v[3] != (double)(uint32_t)v[3])) {
                fprintf(stderr, "air_channels: --fade wants path,doppler_millihz,rice_k[,key]: integers but for rice_k\n");
                return 1;
            }
            fades.push_back(pirip_air_fade{(int32_t)v[0], (int32_t)v[1], (float)v[2], v.size() == 4 ? (uint32_t)v[3] : 0u});
            break;
        }
        default: return usage();
        }
    }
    // getopt stops at the first file name; a "--" in front of the file names (none was an option) is skipped by it, the one between the
    // two lists is found here
    std::vector<std::string> in_names, out_names;
    bool behind = false;
    for (int i = optind; i < argc; i++) {
        if (!behind && !strcmp(argv[i], "--")) { behind = true; continue; }
        (behind ? out_names : in_names).push_back(argv[i]);
    }
    const int T = (int)in_names.size(), R = (int)out_names.size();
    if (Fs <= 0 || T == 0 || R == 0 || block <= 0 || start < 0 || max_slip < 0 || max_slip > 0x7fffffff) return usage();
    if (sigma.size() == 1) sigma.assign((size_t)R, sigma[0]);
    if (!sigma.empty() && (int)sigma.size() != R) { fprintf(stderr, "air_channels: one --sigma, or one per output (%d)\n", R); return 1; }
    std::vector<std::unique_ptr<File>> fin, fout;
    for (const std::string &nm : in_names) {
        fin.emplace_back(new File(fopen(nm.c_str(), "rb")));
        if (!*fin.back()) { fprintf(stderr, "air_channels: can't open %s\n", nm.c_str()); return 1; }
    }
    for (const std::string &nm : out_names) {
        fout.emplace_back(new File(fopen(nm.c_str(), "wb")));
        if (!*fout.back()) { fprintf(stderr, "air_channels: can't open %s\n", nm.c_str()); return 1; }
    }

    AirHandle air;
    if (!fades.empty()) {
        PIRIPOK(pirip_hip_air_create_fade((int)Fs, in_format, out_format, T, R, (int)paths.size(), paths.data(), (int)fades.size(), fades.data(),
                                          sigma.empty() ? nullptr : sigma.data(), (uint64_t)seed, (int32_t)max_slip, -1, air.out()),
                "channel (--path / --fade / --max-slip / --sigma / --fs)");
    } else if (drift || max_slip) {
        PIRIPOK(pirip_hip_air_create_ex((int)Fs, in_format, out_format, T, R, (int)paths.size(), paths.data(), sigma.empty() ? nullptr : sigma.data(),
                                        (uint64_t)seed, (int32_t)max_slip, -1, air.out()), "channel (--path / --max-slip / --sigma / --fs)");
    } else {
        std::vector<pirip_air_path> plain;
        for (const pirip_air_path_ex &p : paths) plain.push_back(pirip_air_path{p.rx, p.tx, p.delay, p.offset_hz, p.gain});
        PIRIPOK(pirip_hip_air_create((int)Fs, in_format, out_format, T, R, (int)plain.size(), plain.data(), sigma.empty() ? nullptr : sigma.data(),
                                     (uint64_t)seed, -1, air.out()), "channel (--path / --sigma / --fs)");
    }
    PIRIPOK(pirip_hip_air_reset(air, start, nullptr), "--start");
    const size_t bsi = in_format == PIRIP_IN_CF32 ? 8 : 2, bso = out_format == PIRIP_IN_CF32 ? 8 : 2;
    const size_t in_stride = ((size_t)block * bsi + 15) / 16 * 16, out_stride = ((size_t)block * bso + 15) / 16 * 16;
    DevBuf<void> d_in, d_out;
    HIPOK(hipMalloc(d_in.out(), in_stride * (size_t)T));
    HIPOK(hipMalloc(d_out.out(), out_stride * (size_t)R));
    std::vector<uint8_t> raw(in_stride * (size_t)T), out(out_stride * (size_t)R);
    long long total = 0;
    long blocks = 0;
    for (;;) {
        size_t n = (size_t)block;
        for (int t = 0; t < T; t++) {
            const size_t got = fread(raw.data() + (size_t)t * in_stride, bsi, (size_t)block, *fin[(size_t)t]);
            if (got < n) n = got;
        }
        if (n == 0) break;
        HIPOK(hipMemcpy(d_in, raw.data(), raw.size(), hipMemcpyHostToDevice));
        PIRIPOK(pirip_hip_air_push(air, d_in, in_stride, (int64_t)n, d_out, out_stride, nullptr), drift ? "channel (the slip budget, --max-slip?)" : "channel");
        HIPOK(hipMemcpy(out.data(), d_out, out.size(), hipMemcpyDeviceToHost));
        for (int r = 0; r < R; r++)
            if (fwrite(out.data() + (size_t)r * out_stride, bso, n, *fout[(size_t)r]) != n) { fprintf(stderr, "air_channels: short write\n"); return 1; }
        total += (long long)n;
        blocks++;
        if (n < (size_t)block) break;
    }
    for (int r = 0; r < R; r++) if (fflush(*fout[(size_t)r]) != 0) { fprintf(stderr, "air_channels: short write\n"); return 1; }
    if (!quiet)
        fprintf(stderr, "air_channels: Fs %ld inputs %d outputs %d paths %d start %lld: %lld samples in %ld blocks of %lld\n", Fs, T, R, (int)paths.size(),
                start, total, blocks, block);
    return 0;
}
