"""Shapes, inputs and parameters for tests/test_air_fade_cpu.py (no GPU: the inputs reach what they claim, on the model alone) and
tests/test_air_fade.py (the device): the channel's fading paths."""
import numpy as np

import airref
import airshapes as sh
import driftshapes as ds
import muxshapes as ms
import sigutil

FS24 = 1 << 24
FSS = [240000, FS24]
FORMATS = sh.FORMATS
FMT, BS = sh.FMT, sh.BS

# ---- 1. the model shapes: two transmitters, four receivers -------------------------------------------------------------------------------
NTX, NRX = 2, 4
N = 6300                                   # three tiles and a ragged one
CALLS = [4500, 1800]                       # the second call reads the rings
SIGMA = [0.05, 0.02, 0.0, 0.03]            # the run with noise: receiver 2, the K = 10^6 one, stays without
SEED = 79
MAX_SLIP = 8
K_LOS = 1.0e6                              # a fade that is all line of sight
# the starts: a grid point on every tile's first sample; n0 & 15 == 15; a grid point on every tile's last sample; the 32-bit wrap of the
# phase's index inside the first call; 2^31 + 3; the last samples below 2^53
STARTS = [0, (1 << 20) + 15, (1 << 24) + 1, 2 ** 32 - 100, 2 ** 31 + 3, 2 ** 53 - 1 - N]


def doppler_limit_hz(Fs):
    """the largest Doppler spread create_fade takes: floor(1000 Fs / 1024) millihertz"""
    return (1000 * Fs // 1024) / 1000.0


def layout(Fs):
    """((rx, tx, delay, offset_hz, clock_ppb) of every path, the fades (path, doppler_hz, rice_k, key)).
    Receiver 0: a static path without a fade, a fading static path, and two fading rotated paths of transmitter 1 at delays 1 and 65,
    offsets +-(Fs/2 - 1), with different keys. Receiver 1: two fading drifting paths, +-300000 ppb, the slow one at the Doppler limit, and
    a static path without a fade. Receiver 2: one path whose fade is all line of sight (K = 10^6). Receiver 3: a fade with Doppler 0 and a
    rotated path past a tile at the Doppler limit, beside a static one. Every receiver has a path of delay 0: a sample without any input is
    exactly 0, which is a tie of the u8 quantiser."""
    e = ms.edge(Fs)
    lim = doppler_limit_hz(Fs)
    paths = [(0, 0, 0, 0, 0), (0, 0, 5, 0, 0), (0, 1, 1, e, 0), (0, 1, 65, -e, 0),
             (1, 0, 8 + MAX_SLIP, 0, 300000), (1, 1, 8, 3, -300000), (1, 0, 0, 0, 0),
             (2, 1, 0, 0, 0),
             (3, 0, 64, 0, 0), (3, 1, airref.TILE + 1, 12345, 0), (3, 1, 0, -7, 0)]
    fades = [(1, 20.0, 0.0, 1), (2, 20.0, 1.0, 2), (3, 7.0, 0.0, 3), (4, 20.0, 0.0, 4), (5, lim, 1.0, 5), (7, 20.0, K_LOS, 6), (8, 0.0, 0.0, 7),
             (9, lim, 0.0, 8)]
    return paths, fades


def inputs(Fs, in_fmt, seed=0):
    """(x as airshapes.inputs draws it, paths with their gains, fades). The gains are a quarter of airshapes': a Rayleigh fade can
    reach Gamma = 4, and the sums stay small enough for the u8 cases to keep clear of the quantiser's ties (tests/test_air_fade_cpu.py)."""
    x, _ = sh.inputs(Fs, in_fmt, n=N, ntx=NTX, seed=400 + seed)
    lay, fades = layout(Fs)
    rng = np.random.default_rng(500 + FSS.index(Fs) * 2 + (in_fmt == "cf32") + seed)
    g = sh.gains(rng, len(lay)) * 0.25
    g[7] *= 4.0                            # the K = 10^6 path has Gamma = 1 + 16 s = 1.004
    scale = 1.0 if in_fmt == "u8" else 0.2
    return x, [(rx, tx, float(np.float32(g[i] * scale)), d, f, q) for i, (rx, tx, d, f, q) in enumerate(lay)], fades


# ---- 2. cutting ------------------------------------------------------------------------------------------------------------------------
CUTS, CUT_N, CUT_START = sh.CUTS, sh.CUT_N, sh.CUT_START
CUT_SLIP, CUT_AGE = ds.CUT_SLIP, ds.CUT_AGE
CUT_SIGMA = [0.05, 0.08]
CUT_SEED = 9


def cut_paths(Fs):
    """driftshapes.cut_paths -- a longest delay of 150, rings of 256 and 128 samples -- at a third of its gains, with fades on a drifting
    rotated path, a drifting unrotated one, a static one and a rotated one at the edge"""
    paths = [p[:2] + (p[2] / 3.0,) + p[3:] for p in ds.cut_paths(Fs)]
    return paths, [(0, 20.0, 0.0, 11), (1, 33.0, 1.0, 12), (2, 5.0, 0.0, 13), (3, doppler_limit_hz(Fs), 4.0, 14)]


# ---- 3. a period of 2^32 samples: static paths, no carrier offset, no noise ------------------------------------------------------------------
WRAP_PATHS = [(0, 0, 0.05, 0, 0), (0, 1, -0.04, 77, 0), (1, 1, 0.06, 3, 0)]
WRAP_FADES = [(0, 20.0, 0.0, 21), (1, 11.0, 2.0, 22)]


# ---- 4. the reason for the feature: the headline shape through one Rayleigh and one Rician path ------------------------------------------------
DEMOD_HZ = 20.0
DEMOD_NSYM = ds.CLOCK_NSYM
DEMOD_FLOOR = 0.05                         # a frame counts when its smallest |g| exceeds this
DEMOD_SEED = 1
# (gain 0.5: the test signal's amplitude of 0.5 times Gamma = 4 stays inside the u8 range)
DEMOD_PATHS = [(0, 0, 0.5, 0, 0), (1, 0, 0.5, 0, 0)]
DEMOD_FADES = [(0, DEMOD_HZ, 0.0, 0), (1, DEMOD_HZ, 4.0, 0)]     # receiver 0 Rayleigh, receiver 1 Rician K = 4


def demod_input(ob):
    return ds.clock_input(ob, DEMOD_NSYM)


def demod_check(ro, nmem, tx_bits, gmag):
    """The expectation on a demodulator's result `ro` (the oracle's or the device's) for the received stream whose gain has the modulus
    gmag [n]: frame f decides its bits on the nmem samples that end with its last one (the nin it reports, summed), and it counts when the
    smallest |g| over them exceeds DEMOD_FLOOR. A frame that counts, after the first, must be a stretch of the transmitted test bits
    (periodic in 100) without a bit error. Returns (frames, frames left out, frames with an error)."""
    nin = ro["stats"][:, 6].astype(np.int64)
    end = np.cumsum(nin)
    period = np.concatenate([tx_bits[:100], tx_bits[:100]])
    out, bad = 0, []
    for f in range(1, ro["nframes"]):
        lo, hi = max(0, int(end[f]) - nmem), min(int(end[f]), gmag.shape[0])
        if gmag[lo:hi].min() <= DEMOD_FLOOR:
            out += 1
            continue
        b = np.asarray(ro["bits"][f]).reshape(-1)
        if not any(np.array_equal(b, period[o:o + b.size]) for o in range(100)):
            bad.append(f)
    return ro["nframes"], out, bad


# ---- 5. the shared-medium loop with Rician far paths ---------------------------------------------------------------------------------------
LOOP_HZ, LOOP_K = 5.0, 4.0
LOOP_PATHS = sh.LOOP_PATHS
LOOP_FADES = [(0, LOOP_HZ, LOOP_K, 31), (2, LOOP_HZ, LOOP_K, 32)]  # the far paths: repeater -> terminal and terminal -> repeater
