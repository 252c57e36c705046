// tool_common.hpp -- the host code the command-line tools share: a new tool starts from this header (and tx_records.hpp when it reads
// or makes transmit records) instead of from a copy of another tool. Header-only; a function that is not called leaves no reference
// behind, so a program that uses only the argument helpers links neither libpirip_hip.so nor the HIP runtime. The last part, device
// buffers and HIPOK, is there for the tools that see the HIP runtime API: those the Makefile builds with -D__HIP_PLATFORM_AMD__.
#pragma once
#include <sys/stat.h>
#include <unistd.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/pirip_hip.h"
#ifdef __HIP_PLATFORM_AMD__
#include <hip/hip_runtime_api.h>
#endif

namespace {

// ---- arguments ------------------------------------------------------------------------------------------------------------------------
static inline bool file_exists(const std::string &p) { struct stat st; return !p.empty() && stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode); }

// --code NAME: NAME as a file path, then $PIRIP_CODE_DIR/NAME.code, then <exe>/../data/NAME.code; empty when none of them is a file.
// codec2's H_256_512_4 table is not in the reference, it is a data drop in the format of csrc/fsk_ldpc.hpp.
static inline std::string resolve_code(const std::string &name, const char *argv0)
{
    if (file_exists(name)) return name;
    if (const char *d = getenv("PIRIP_CODE_DIR")) { const std::string p = std::string(d) + "/" + name + ".code"; if (file_exists(p)) return p; }
    char exe[4096];
    const ssize_t n = readlink("/proc/self/exe", exe, sizeof(exe) - 1);
    std::string base = n > 0 ? std::string(exe, (size_t)n) : std::string(argv0);
    const size_t s = base.rfind('/');
    base = s == std::string::npos ? "." : base.substr(0, s);
    const std::string p = base + "/../data/" + name + ".code";
    return file_exists(p) ? p : std::string();
}

// "a,b,c" appended to out, every token through conv(token, &end) (strtol's shape). False for an empty token -- so for a leading or
// trailing comma and for an empty text -- and for a token conv does not read to its end.
template <typename T, typename F>
static bool parse_list(const char *s, std::vector<T> &out, F conv)
{
    const std::string all(s);
    for (size_t pos = 0; pos <= all.size();) {
        size_t end = all.find(',', pos);
        if (end == std::string::npos) end = all.size();
        const std::string tok = all.substr(pos, end - pos);
        if (tok.empty()) return false;
        char *e = nullptr;
        const T v = conv(tok.c_str(), &e);
        if (*e) return false;
        out.push_back(v);
        pos = end + 1;
    }
    return !out.empty();
}
static inline int32_t conv_i32(const char *t, char **e) { return (int32_t)strtol(t, e, 10); }     // -c offsets, --route
static inline long conv_long0(const char *t, char **e) { return strtol(t, e, 0); }                // --source: 0x.. allowed
static inline float conv_float(const char *t, char **e) { return strtof(t, e); }                  // --gains

// A binary compiled against another header generation must not run against this library (stats rows, stream state sizes):
//   if (!abi_ok(argv[0])) return 2;
static inline bool abi_ok(const char *argv0)
{
    if (pirip_hip_abi_check(PIRIP_HIP_ABI_VERSION, PIRIP_STATS_PER_FRAME, sizeof(pirip_stream_state))) return true;
    fprintf(stderr, "%s: built against a different pirip_hip.h than %s\n", argv0, pirip_hip_version());
    return false;
}

// ---- rtl_fsk's receive defaults ---------------------------------------------------------------------------------------------------------
// The two rules of upstream's rtl_fsk.c held from recall, as data (the tool-level part of the pin-day drill; the demodulator's own
// recalled constants are pirip_fsk_recalled / PIRIP_RECALLED). rtl_fsk flips them without a rebuild through
//   PIRIP_RTL_FSK_RULES="p_rule=0|1|2,p_max=10,default_rate=240000,wide_rate=1800000,min_rate=900001"
// (from_env); the tools that only borrow rtl_fsk's modem settings use the defaults and do not read the variable.
struct RtlFskRules {
    int p_rule = 0;                 // timing oversample: 0: halve Ts while it is > p_max and even (recalled); 1: P = Ts; 2: P = 8 (fsk_demod's default)
    int p_max = 10;
    long default_rate = 240000;     // RTL rate when -s is absent and the modem rate is absent or divides it
    long wide_rate = 1800000;       // ... else this one when the modem rate divides it
    long min_rate = 900001;         // ... else the smallest multiple of the modem rate from here up
    bool from_env()
    {
        const char *e = getenv("PIRIP_RTL_FSK_RULES");
        if (!e) return true;
        std::string all(e);
        for (size_t pos = 0; pos < all.size();) {
            size_t end = all.find(',', pos);
            if (end == std::string::npos) end = all.size();
            const std::string tok = all.substr(pos, end - pos);
            pos = end + 1;
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) return false;
            const std::string k = tok.substr(0, eq);
            const long v = atol(tok.c_str() + eq + 1);
            if (k == "p_rule") p_rule = (int)v; else if (k == "p_max") p_max = (int)v; else if (k == "default_rate") default_rate = v;
            else if (k == "wide_rate") wide_rate = v; else if (k == "min_rate") min_rate = v; else return false;
        }
        return p_rule >= 0 && p_rule <= 2 && p_max >= 4 && default_rate > 0 && wide_rate > 0 && min_rate > 0;
    }
};

// timing oversample P of a symbol of Ts samples: the oversample reduction rule [UPSTREAM-RECALLED, unverified: RtlFskRules]
static inline int rtl_fsk_oversample(int Ts, const RtlFskRules &rules = RtlFskRules())
{
    int P = Ts;
    if (rules.p_rule == 0) while (P > rules.p_max && (P % 2) == 0) P /= 2;
    else if (rules.p_rule == 2 && Ts % 8 == 0) P = 8;
    return P < 4 ? Ts : P;
}

// rtl_fsk's modem settings: P by the rule above, the estimator from Rs / 2 (off the dongle's DC spur, README.md:116 of the reference)
// to Fs / 2 unless the user gave a limit (null = not given), the --mask comb when mask is not 0.
static inline pirip_fsk_params rtl_fsk_params(int Fs, int Rs, int M, int mask, const int *user_lower, const int *user_upper, int in_format,
                                              const RtlFskRules &rules = RtlFskRules())
{
    return pirip_fsk_params{Fs, Rs, M, rtl_fsk_oversample(Fs / Rs, rules), PIRIP_FSK_DEFAULT_NSYM, user_lower ? *user_lower : Rs / 2,
                            user_upper ? *user_upper : Fs / 2, mask ? 1 : 0, mask ? mask : 100, in_format};
}

// The fewest samples a frame takes (nin = N - Ts / 4 with the default constants; PIRIP_RECALLED can change the step): what sizes
// max_frames for a buffer of samples, as binding.py's max_frames_for does.
static inline int shortest_frame(const pirip_fsk_info &info) { return 2 * info.N - info.nin_max; }

// ---- failures -------------------------------------------------------------------------------------------------------------------------
// A tool's name and which exit code a failed library call (a PIRIP_* status) ends it with; each tool has one, kTool, that the
// check macros read:   static const ToolErrors kTool{"rtl_fsk", [](int) { return 2; }};
struct ToolErrors { const char *name; int (*exit_code)(int status); };

// "<tool>: <what>: <the status in words>" on stderr; gives the exit code
static inline int status_fail(const ToolErrors &t, const char *what, int status)
{
    fprintf(stderr, "%s: %s: %s\n", t.name, what, pirip_hip_strerror(status));
    return t.exit_code(status);
}
// pirip_hip_tx_create refuses what the framer refuses (exit 2, the code file); anything else is the device (3)
static inline int tx_create_exit_code(int status) { return status == PIRIP_ERR_BAD_CONFIG || status == PIRIP_ERR_UNSUPPORTED ? 2 : 3; }

#define PIRIPOK(expr, what) do { const int rc_ = (expr); if (rc_ != PIRIP_OK) return status_fail(kTool, what, rc_); } while (0)

// ---- owners: every return releases what the tool holds, in reverse order of declaration -------------------------------------------------
// Declare handles in the order channelizer, demodulator, LDPC, receiver, transmitter, multiplexer, streaming transmitter, repeater (a
// later one uses the earlier ones). Reads as the pointer it holds; out() is the `T **` of a *_create call.
template <typename T, auto Release>
struct Owned {
    T *p = nullptr;
    Owned() = default;
    explicit Owned(T *q) : p(q) {}
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { if (p) (void)Release(p); }
    operator T *() const { return p; }
    T **out() { return &p; }
};
using DemodHandle = Owned<pirip_hip_demod, pirip_hip_destroy>;
using DecimHandle = Owned<pirip_hip_decim, pirip_hip_decim_destroy>;
using LdpcHandle = Owned<pirip_hip_ldpc, pirip_hip_ldpc_destroy>;
using ChanHandle = Owned<pirip_hip_chan, pirip_hip_chan_destroy>;
using RxHandle = Owned<pirip_hip_rx, pirip_hip_rx_destroy>;
using TbitsHandle = Owned<pirip_hip_tbits, pirip_hip_tbits_destroy>;
using TxHandle = Owned<pirip_hip_tx, pirip_hip_tx_destroy>;
using MuxHandle = Owned<pirip_hip_mux, pirip_hip_mux_destroy>;
using TxsHandle = Owned<pirip_hip_txs, pirip_hip_txs_destroy>;
using RptHandle = Owned<pirip_hip_rpt, pirip_hip_rpt_destroy>;
using PingHandle = Owned<pirip_hip_ping, pirip_hip_ping_destroy>;

// ---- the ping terminal's log (ping_channels, rtl_fsk_channels -L) ------------------------------------------------------------------------
// rtl_fsk -L's line without the wall clock, the channel in front; the dB value is computed here as in rtl_fsk.cpp
static inline void print_ping_entry(FILE *f, int chan, const pirip_ping_entry &e, int Fs)
{
    const double S = e.S, N = e.N;
    fprintf(f, "%d: Rx frame src: 0x%02x seq: %3d S: %e N: %e SNR: %5.2f dB t_rx: %.4f s\n", chan, e.source, e.seq, S, N,
            10.0 * log10(S / (N + 1e-30) + 1e-30), (double)e.t_samples / (double)Fs);
}
// The entries logged since the last look, per receive channel, on stderr: seen [nrx] = the frames printed so far (zeros at first), buf a
// work array. A channel that logged more than its ring holds since then says so and prints what the ring kept. Synchronises the device.
static inline int print_new_ping_entries(pirip_hip_ping *ping, int Fs, std::vector<int64_t> &seen, std::vector<pirip_ping_entry> &buf)
{
    pirip_ping_info pi;
    int rc = pirip_hip_ping_get_info(ping, &pi);
    if (rc != PIRIP_OK) return rc;
    std::vector<int64_t> frames((size_t)pi.nrx);
    if ((rc = pirip_hip_ping_get_counters(ping, frames.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) != PIRIP_OK) return rc;
    buf.resize((size_t)pi.log_entries);
    for (int c = 0; c < pi.nrx; c++) {
        int64_t fresh = frames[(size_t)c] - seen[(size_t)c];
        if (fresh > pi.log_entries) { fprintf(stderr, "%d: %lld log entries lost\n", c, (long long)(fresh - pi.log_entries)); fresh = pi.log_entries; }
        int got = 0;
        if (fresh > 0 && (rc = pirip_hip_ping_get_log(ping, c, buf.data(), (int)fresh, &got)) != PIRIP_OK) return rc;
        for (int i = 0; i < got; i++) print_ping_entry(stderr, c, buf[(size_t)i], Fs);
        seen[(size_t)c] = frames[(size_t)c];
    }
    return PIRIP_OK;
}

// an input or output file; the process's own stdin / stdout stay open
static inline int close_file(FILE *f) { return f == stdin || f == stdout ? 0 : fclose(f); }
using File = Owned<FILE, close_file>;

#ifdef __HIP_PLATFORM_AMD__
// device memory:   DevBuf<float> d_stats;  HIPOK(hipMalloc((void **)d_stats.out(), bytes));
template <typename T> using DevBuf = Owned<T, hipFree>;
#endif

}  // namespace

#ifdef __HIP_PLATFORM_AMD__
#define HIPOK(expr) do { if ((expr) != hipSuccess) { fprintf(stderr, "%s: HIP error at %s:%d\n", kTool.name, __FILE__, __LINE__); return kTool.exit_code(PIRIP_ERR_HIP); } } while (0)
#endif
