"""Shapes, inputs and expected outputs for tests/test_spectrum_cpu.py (no GPU: the inputs reach what they claim, on the statement alone)
and tests/test_spectrum.py (the device). Everything is memoised: a case's inputs and its reference rows are made once per process."""
import functools

import numpy as np

import chanref
import specref

FS = 240000
NSTREAMS = 3
CASES = [(nfft, hop, fmt, avg) for nfft in specref.NFFTS for hop in (nfft, nfft // 2) for fmt in ("u8", "cf32") for avg in (1, 3)]
FMT = {"u8": specref.U8, "cf32": specref.CF32}
BS = {"u8": 2, "cf32": 8}

# stream 2: three 2-FSK channels (tones 10 and 20 kHz above the centre, as tests/test_channelizer.py's modem) and an empty stretch
CHAN_OFFSETS = [-90000, -30000, 30001]
MODEM = dict(Rs=10000, M=2, f1=10000, shift=10000)
CHAN_STEPS, NOISE_STEPS = 20.0, 3.0        # amplitudes in u8 steps
TONE_STEPS = 40.0                          # stream 0's two tones


def length(nfft, hop, avg):
    """two complete rows and part of a third: with half overlap and avg > 1 a complete segment of the third row and part of the next, else
    part of its first segment; at most 7 * 4096 samples"""
    extra = hop + hop // 2 + 7 if (hop < nfft and avg > 1) else hop // 2 + 7
    n = (2 * avg - 1) * hop + nfft + extra
    assert n <= 7 * 4096
    return n


def on_bin(nfft):
    return nfft // 8                       # stream 0's first tone: exactly this bin (30 kHz)


def half_bin(nfft):
    return -nfft // 4 + 0.5                # stream 0's second tone: halfway between two bins, in bins


def bands(nfft):
    """(stream, lo_hz, hi_hz); the names index BAND"""
    f_on = int(round(on_bin(nfft) * FS / nfft))
    top = int((nfft // 2 - 1) * FS / nfft)                  # inside the last bin below Fs / 2
    ch = [(2, c - 5000, c + 35000) for c in CHAN_OFFSETS]   # the second one runs from negative to positive frequency, too
    return ch + [(2, 80000, 110000),                        # 3 empty
                 (0, -3000, 3000),                          # 4 wraps across bin 0
                 (0, f_on, f_on),                           # 5 one bin
                 (1, -FS // 2, top),                        # 6 every bin, from the middle of the row round to the middle
                 (0, 20000, 40000), (0, 30000, 50000)]      # 7, 8 overlap, the tone in both


BAND = dict(chan=(0, 1, 2), empty=3, wrap=4, one=5, all=6, overlap=(7, 8))


@functools.lru_cache(maxsize=None)
def inputs(nfft, hop, fmt, avg):
    """the three streams as the device takes them: uint8 [3, n, 2] or complex64 [3, n]"""
    n = length(nfft, hop, avg)
    rng = np.random.default_rng(CASES.index((nfft, hop, fmt, avg)) + 500)
    t = np.arange(n)
    noise = lambda s: s * (rng.normal(size=n) + 1j * rng.normal(size=n))
    z0 = TONE_STEPS * np.exp(2j * np.pi * on_bin(nfft) * t / nfft) + TONE_STEPS * np.exp(2j * np.pi * (half_bin(nfft) * t / nfft + 0.3)) + noise(4.0)
    z2 = noise(NOISE_STEPS)
    for c, fc in enumerate(CHAN_OFFSETS):
        bits = rng.integers(0, 2, n // (FS // MODEM["Rs"]) + 2)
        z2 = z2 + chanref.fsk_wideband(FS, MODEM["Rs"], MODEM["M"], fc + MODEM["f1"], MODEM["shift"], bits, n, CHAN_STEPS, phase0=rng.uniform(0, 2 * np.pi))
    if fmt == "u8":
        x1 = rng.integers(0, 256, (n, 2)).astype(np.uint8)
        x1[5] = (0, 255)
        x1[nfft + 1] = (255, 0)
        x = np.stack([chanref.quantise_u8(z0), x1, chanref.quantise_u8(z2)])
    else:
        z1 = noise(30.0) + (25.0 - 12.0j)                  # a DC offset
        x = (np.stack([z0, z1, z2]) / 127.5).astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def expected(nfft, hop, fmt, avg):
    """(rows float32 [3, m, nfft], band entries [nbands, m]) of the statement; read-only"""
    x = inputs(nfft, hop, fmt, avg)
    rws = np.stack([specref.rows(x[r], FMT[fmt], nfft, hop, avg) for r in range(NSTREAMS)])
    bnd = np.stack([specref.band_rows(rws[s], lo, hi, nfft, FS) for s, lo, hi in bands(nfft)])
    rws.setflags(write=False)
    bnd.setflags(write=False)
    return rws, bnd


def two_calls(n):
    """two uneven calls"""
    return [2 * n // 5 + 1, n - (2 * n // 5 + 1)]


CUT_AVG = 3                                # the cutting test's cases: two rows of 3 segments are longer than 2 nfft + 3 samples, two of 1 are not
CUT_CASES = [c for i, c in enumerate(c for c in CASES if c[3] == CUT_AVG) if (i + i // 2) % 2 == 0]    # per nfft and hop one format, alternating


def cuttings(nfft, hop, avg, n):
    """the three cuttings of the cutting test, as lists of call lengths"""
    ones = 2 * nfft + 3
    assert n > ones
    a = [1] * ones + [n - ones]
    b = [997] * (n // 997) + ([n % 997] if n % 997 else [])
    first_row = (avg - 1) * hop + nfft                     # samples that complete row 0
    c = [first_row - 1, 1, n - first_row]
    return [a, b, c]
