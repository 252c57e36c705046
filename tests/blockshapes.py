"""Shape table and inputs shared by tests/test_block_demod_cpu.py (no GPU: on the oracle alone, the inputs reach the paths they claim) and
tests/test_block_demod.py (the device): the workgroup-per-stream demodulator of pirip_amd/csrc/fsk_demod_block.hip, `rtl_fsk -r 1000` at
240 kS/s -- Ts = 240, P = 15, Ndft = 4096, frames of N = 12000 samples, nin = N - 60, N or N + 60."""
import numpy as np

import parity
import sigutil
from demodrun import resample_at

FS, RS, P, F1, SHIFT, MASK = 240000, 1000, 15, 11000, 2000, 2000
TS, NSYM = FS // RS, 50
N, Q = TS * NSYM, TS // 4
EST_MIN, EST_MAX = 500, FS // 2 - RS
NDFT = 4096
NINS = (N - Q, N, N + Q)

# The u8 quantiser's amplitude per input format (u8 = round(127 + amp x), |x| = 2), as the block test of tests/test_gpu_parity.py uses. With
# it no frame of the 240-offset sweep has |norm_rx_timing| within 5 TIMING_TOL = 2.5e-4 of the 0.25 threshold, so every stream is held to
# an exact nin sequence. Smallest distance found (tests/test_block_demod_cpu.py prints them):
#   u8d   M = 2: 5.06e-4   M = 4: 1.19e-3
#   csdr  M = 2: 5.05e-4   M = 4: 1.19e-3
# (csdr needed no other amplitude than u8d.)
AMP = {"csdr": 20.0, "u8d": 20.0}

# the eight instances: name -> (M, format, mask spacing, start offset of the streams of test a)
ROWS = {
    "m2_csdr_peak": (2, "csdr", 0, 7),
    "m2_csdr_mask": (2, "csdr", MASK, 33),
    "m4_csdr_peak": (4, "csdr", 0, 61),
    "m4_csdr_mask": (4, "csdr", MASK, 98),
    "m2_u8d_peak": (2, "u8d", 0, 131),
    "m2_u8d_mask": (2, "u8d", MASK, 164),      # the two instances no test launched before this table
    "m4_u8d_peak": (4, "u8d", 0, 202),
    "m4_u8d_mask": (4, "u8d", MASK, 239),
}

# Start offsets of the sweep (clean test bits) whose oracle nin sequence holds a short frame (N - Q) / a long one (N + Q) / neither, the same
# for both formats and both M (tests/test_block_demod_cpu.py asserts it): the canary test's three streams with three different consumed
# counts, and the burst-mode stream (OFF_SHORT: without burst mode its nin leaves N).
OFF_SHORT, OFF_LONG, OFF_EVEN = 90, 150, 20

SWEEP_FRAMES = 5
SWEEP_LEN = SWEEP_FRAMES * N + 300
CLOCK_PPM = 300e-6


def cfg(M):
    return dict(Fs=FS, Rs=RS, M=M, P=P, f1=F1, shift=SHIFT, est_min=EST_MIN, est_max=EST_MAX)


def fmt_of(mod, name):
    """the format constant of `mod` (oracle.binding or pirip_amd: the same names and values)"""
    return mod.IN_CU8_CSDR if name == "csdr" else mod.IN_CU8_FSKDEMOD


def oracle_of(ob, M, mask=0, est_min=EST_MIN, est_max=EST_MAX):
    return ob.OracleFsk(FS, RS, M, P=P, est_min=est_min, est_max=est_max, tone_spacing=mask if mask else 100, mask=bool(mask))


def handle_of(pirip_amd, M, fmt, mask=0, nstreams=1, est_min=EST_MIN, est_max=EST_MAX):
    return pirip_amd.HipDemod(FS, RS, M, P=P, est_min=est_min, est_max=est_max, mask=mask, in_format=fmt_of(pirip_amd, fmt), nstreams=nstreams)


_cache = {}


def _memo(key, make):
    if key not in _cache:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def sweep_base(ob, M, fmt):
    """the sweep's one recording: 350 symbols of test bits, noise-free; stream `off` is [off : off + SWEEP_LEN] of it"""
    bps = 1 if M == 2 else 2
    return _memo(("sweep", M, fmt), lambda: ob.quantise_cu8(sigutil.mod_complex(ob, cfg(M), ob.get_test_bits(350 * bps)), amp=AMP[fmt]))


def sweep_stream(ob, M, fmt, off):
    return sweep_base(ob, M, fmt)[off:off + SWEEP_LEN]


def sweep_oracle(ob, M, fmt):
    """the oracle's result on each of the 240 streams of the sweep, computed once per (M, format)"""
    return _memo(("sweep_o", M, fmt), lambda: [_with_Sf(ob, oracle_of(ob, M), sweep_stream(ob, M, fmt, off), fmt) for off in range(TS)])


def _with_Sf(ob, o, u8, fmt):
    r = o.demod(u8, fmt_of(ob, fmt))
    r["Sf"] = oracle_Sf(ob, o)
    return r


def oracle_Sf(ob, o):
    return parity.oracle_Sf(ob, o, NDFT)


def resample(x, ppm):
    """a sample clock off by ppm, by linear interpolation (test_sample_clock_offset_exercises_nin_feedback's resampler)"""
    return resample_at(x, np.arange(int(x.shape[0] / (1 + abs(ppm)) - 2)) * (1 + ppm))


def clock_stream(ob, M, fmt, ppm):
    """2000 symbols of test bits on a sample clock off by ppm, noise-free: 39 frames. (2000 bits for M = 2; for M = 4 as many symbols, 4000
    bits: with 2000 bits -- 19 frames -- the oracle steps nin once per direction, and the tests ask for two frames.)"""
    bps = 1 if M == 2 else 2
    return _memo(("clock", M, fmt, ppm),
                 lambda: ob.quantise_cu8(resample(sigutil.mod_complex(ob, cfg(M), ob.get_test_bits(2000 * bps)), ppm), amp=AMP[fmt]))


def noisy_stream(ob, M, fmt, nsym, seed, offset=0, ebno_db=9.0):
    """random bits, nsym symbols, the first `offset` samples dropped; ebno_db None: noise-free"""
    def make():
        rng = np.random.default_rng(seed)
        x = sigutil.mod_complex(ob, cfg(M), rng.integers(0, 2, nsym * (1 if M == 2 else 2)).astype(np.uint8))[offset:]
        if ebno_db is not None:
            x = sigutil.add_awgn(x, ebno_db, cfg(M), rng)
        return ob.quantise_cu8(x, amp=AMP[fmt])
    return _memo(("noisy", M, fmt, nsym, seed, offset, ebno_db), make)


def chunk_sizes(seed, total):
    """ragged chunk sizes of 1 ... 40000 samples, drawn once from a seeded generator, that add up to at least `total`"""
    rng = np.random.default_rng(seed)
    out = []
    while sum(out) < total:
        out.append(int(rng.integers(1, 40001)))
    return out


def clock_counts_ok(ro, ppm):
    """at least two short frames on a fast clock, two long ones on a slow clock (an oracle result)"""
    return int((ro["stats"][:, 6] == (N - Q if ppm > 0 else N + Q)).sum()) >= 2


def _seed(name, k):
    return 1000 * (k + 1) + sorted(ROWS).index(name)


def row_streams(ob, name):
    """test a: one noise-free stream and one at 9 dB, 1560 symbols (31 frames) from the row's start offset"""
    M, fmt, _, off = ROWS[name]
    return noisy_stream(ob, M, fmt, 1560, _seed(name, 0), off, None), noisy_stream(ob, M, fmt, 1560, _seed(name, 1), off, 9.0)


# test d (packed bits): 2-FSK and 4-FSK, a mask row of each, both formats
PACKED_ROWS = ("m2_u8d_mask", "m4_csdr_peak", "m4_u8d_mask", "m2_csdr_peak")


def packed_streams(ob, name):
    """two streams of 600 symbols at 9 dB (11 frames), the second 37 samples later in its symbol"""
    M, fmt, _, off = ROWS[name]
    return [noisy_stream(ob, M, fmt, 600, _seed(name, 2 + s), off + 37 * s, 9.0) for s in range(2)]


# test f (scalar state without a stats output)
SCALAR_ROWS = ("m2_csdr_peak", "m4_u8d_mask")
SCALAR_MAX_FRAMES = 8


def scalar_stream(ob, name):
    M, fmt, _, off = ROWS[name]
    return noisy_stream(ob, M, fmt, 660, _seed(name, 4), off, 9.0)          # 12 frames


# tests h and k: two recordings (A then B; eight streams share them out) of a 2-FSK and a 4-FSK mask handle
PAIR_ROWS = ("m2_u8d_peak", "m4_csdr_mask")


def pair_streams(ob, name, n=2):
    M, fmt, _, off = ROWS[name]
    return [noisy_stream(ob, M, fmt, 560, _seed(name, 5 + s), (off + 53 * s) % TS, 9.0 if s % 2 == 0 else None) for s in range(n)]


# test j (capture): 25 frames at 9 dB
CAPTURE_ROW = "m2_csdr_mask"


def capture_stream(ob):
    M, fmt, _, off = ROWS[CAPTURE_ROW]
    return noisy_stream(ob, M, fmt, 1300, _seed(CAPTURE_ROW, 13), off, 9.0)


# test i: pirip_hip_set_freq_est_limits(500, 12000) leaves the upper tone (13 kHz) outside the search range
LIMITS = (500, 12000)


def limits_stream(ob):
    return noisy_stream(ob, 2, "csdr", 400, 77, 11, 9.0)                    # 7 frames
