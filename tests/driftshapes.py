"""Shapes, inputs and parameters for tests/test_air_drift_cpu.py (no GPU: the inputs reach what they claim, on the model alone) and
tests/test_air_drift.py (the device): the channel's drifting paths."""
import numpy as np

import airref
import airshapes as sh
import muxshapes as ms
import sigutil

FS24 = 1 << 24
FSS = [240000, FS24]
FORMATS = sh.FORMATS
FMT, BS = sh.FMT, sh.BS

# ---- 1. the model shapes: two transmitters, two receivers, each mixing static and drifting paths ---------------------------------------
NTX, NRX = 2, 2
N = 6300                                   # three tiles and a ragged one
CALLS = [4500, 1800]                       # the second call reads the rings
SIGMA = [0.05, 0.02]
SEED = 78
TILE_PAST = airref.TILE + 1                # a delay one past a tile
SLIP_SMALL = 12
SLIP_LARGE = (1 << 20) - 4096 - 7          # a slow path of delay up to 4096 still fits the longest ring with it: d + 7 + max_slip <= 2^20
# (max_slip, clock age of the reset, absolute index of the reset). For +-300000 ppb S steps at the clock ages 3334 and 6667: age 0 puts
# the first step inside tile 1, age 1286 on the first sample of tile 1 (a tile edge), age 2167 the second on the first sample of the second
# call and the first inside tile 0. +-10^6 ppb steps every 1000 samples, inside every tile. The last run ends on clock age
# 1000 SLIP_LARGE: |S| = max_slip for +-10^6 ppb on the call's last sample.
RUNS = [(SLIP_SMALL, 0, 0), (SLIP_SMALL, 1286, 240000 - 5), (SLIP_SMALL, 2167, 2 ** 31 + 3), (SLIP_LARGE, 1000 * SLIP_LARGE - (N - 1), 2 ** 31 + 3)]


def layout(Fs, max_slip):
    """(rx, tx, delay, offset_hz, clock_ppb) of every path. A fast path (q > 0) needs a delay of 8 + max_slip at least: the delays 63 and 65
    are kept where max_slip lets them."""
    e = ms.edge(Fs)
    fast = lambda d: max(d, 8 + max_slip)
    return [(0, 0, 0, 0, 0), (0, 0, fast(0), 1, 300000), (0, 0, 8, 0, -300000), (0, 1, fast(63), -7, 1), (0, 1, 64, e, -1), (0, 0, 300, -e, 0),
            (1, 1, 0, -1, 0), (1, 0, fast(65), 12345, 1000000), (1, 0, TILE_PAST, 0, -1000000), (1, 1, 63, 5, -300000)]


def inputs(Fs, in_fmt, max_slip, seed=0):
    """(x as airshapes.inputs draws it, paths with their gains)"""
    x, _ = sh.inputs(Fs, in_fmt, n=N, ntx=NTX, seed=200 + seed)
    lay = layout(Fs, max_slip)
    rng = np.random.default_rng(300 + FSS.index(Fs) * 2 + (in_fmt == "cf32") + seed)
    g = sh.gains(rng, len(lay))
    scale = 1.0 if in_fmt == "u8" else 0.2
    return x, [(rx, tx, float(np.float32(g[i] * scale)), d, f, q) for i, (rx, tx, d, f, q) in enumerate(lay)]


# ---- 2. cutting ------------------------------------------------------------------------------------------------------------------------
CUTS, CUT_N, CUT_START = sh.CUTS, sh.CUT_N, sh.CUT_START
CUT_SLIP, CUT_AGE = 8, 3000                # clock ages 3000 .. 5599: S steps for every offset but +-1 ppb


def cut_paths(Fs):
    """airshapes.cut_paths with clock offsets: rings of 256 (transmitter 0: lags 157 and 116) and 128 samples (transmitter 1: 71 and 48)"""
    return [(0, 0, 0.11, 150, 1234, 300000), (0, 1, -0.07, 33, 0, -1000000), (0, 0, 0.05, 0, -5, 0), (1, 1, 0.09, 64, -(Fs // 2 - 1), 1),
            (1, 0, -0.04, 101, 0, -300000)]


# ---- 6 / 11. the reason for the feature: the headline shape on a clock 300 ppm off ----------------------------------------------------------
CLOCK_PPB = 300000
CLOCK_NSYM = 2000
CLOCK_SLIP = 24                            # 48000 samples at 300 ppm slip by 14.4


def clock_paths():
    """receiver 0 hears the transmitter on a fast clock, receiver 1 on a slow one"""
    return [(0, 0, 1.0, 8 + CLOCK_SLIP, 0, CLOCK_PPB), (1, 0, 1.0, 8, 0, -CLOCK_PPB)]


def clock_input(ob, nsym=CLOCK_NSYM):
    """noise-free test bits on the headline shape as u8 [n, 2], and the bits"""
    bits = ob.get_test_bits(nsym)
    return ob.quantise_cu8(sigutil.mod_complex(ob, sigutil.CFG1, bits), amp=32.0), bits


def clock_demod(ob, u8):
    """(the oracle demodulator's result on u8 [n, 2] of the headline shape, its nominal nin N)"""
    c = sigutil.CFG1
    o = ob.OracleFsk(c["Fs"], c["Rs"], c["M"], P=c["P"], est_min=c["est_min"], est_max=c["est_max"])
    ro = o.demod(np.ascontiguousarray(u8, dtype=np.uint8), ob.IN_CU8_FSKDEMOD)
    return ro, o.N


# ---- 12. the shared-medium loop on two clocks -----------------------------------------------------------------------------------------------
LOOP_PPB = 20000
LOOP_SLIP = 64
LOOP_PATHS = [(0, 1, sh.FAR["gain"], sh.FAR["delay"], sh.FAR["offset"], LOOP_PPB), (0, 0, sh.LEAK["gain"], sh.LEAK["delay"], sh.LEAK["offset"], 0),
              (1, 0, sh.FAR["gain"], sh.FAR["delay"], sh.FAR["offset"], -LOOP_PPB), (1, 1, sh.LEAK["gain"], sh.LEAK["delay"], sh.LEAK["offset"], 0)]
