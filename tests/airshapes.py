"""Shapes, inputs and the shared-medium loop's parameters for tests/test_air_cpu.py (no GPU: the inputs reach what they claim, on the
model alone) and tests/test_air.py (the device)."""
import numpy as np

import airref
import muxshapes as ms

FS24 = 1 << 24
FSS = [240000, FS24, FS24 - 1]
FORMATS = [(i, o) for i in ("u8", "cf32") for o in ("u8", "cf32")]
FMT = {"u8": airref.U8, "cf32": airref.CF32}
BS = {"u8": 2, "cf32": 8}

# ---- 1. the model shapes: three transmitters, four receivers ------------------------------------------------------------------------------
NTX, NRX = 3, 4
N = 6300                                   # three tiles and a ragged one that is no whole 16-byte unit; the delay of 4097 leaves two tiles
CALLS = [4500, 1800]                       # the second call reads every delay's first samples from the rings
SIGMA = [0.05, 0.0, 0.1, 0.02]             # the run with noise: receiver 1 stays without
SEED = 77


def starts(Fs):
    return [0, Fs - 5, 2 ** 31 + 3]


def layout(Fs):
    """(rx, tx, delay, offset_hz) of every path; the gains come with the inputs. Receiver 0 has no path, receiver 1 one unrotated path,
    receiver 2 five paths with two of transmitter 0 at delays 1 and 65 and the offsets 0, 1, -1 and both edges, receiver 3 the delays
    0, 63, 64 and 4097."""
    e = ms.edge(Fs)
    return [(1, 1, 0, 0),
            (2, 0, 1, 0), (2, 0, 65, 1), (2, 1, 0, -1), (2, 2, 7, e), (2, 1, 300, -e),
            (3, 0, 0, 5), (3, 1, 63, 0), (3, 2, 64, -7), (3, 0, 4097, 12345)]


def gains(rng, K):
    """as muxshapes.inputs draws them: 0.02 .. 0.12 in magnitude, both signs, never dyadic"""
    return (rng.uniform(0.02, 0.12, K) * np.where(np.arange(K) % 2, -1.0, 1.0)).astype(np.float32)


def inputs(Fs, in_fmt, n=N, ntx=NTX, seed=0):
    """(x as the device takes it -- uint8 [ntx, n, 2] over all 256 values, or unit-variance complex64 [ntx, n] --, paths with their gains)"""
    rng = np.random.default_rng(FSS.index(Fs) * 2 + (in_fmt == "cf32") + 100 + seed)
    if in_fmt == "u8":
        x = rng.integers(0, 256, (ntx, n, 2)).astype(np.uint8)
    else:
        x = (rng.normal(size=(ntx, n)) + 1j * rng.normal(size=(ntx, n))).astype(np.complex64)
    lay = layout(Fs)
    g = gains(rng, len(lay))
    # complex float input has modulus up to 4: a fifth of the u8 gains keeps five paths well inside the u8 output's range
    scale = 1.0 if in_fmt == "u8" else 0.2
    return x, [(rx, tx, float(np.float32(g[i] * scale)), d, f) for i, (rx, tx, d, f) in enumerate(lay)]


# ---- 2. cutting ------------------------------------------------------------------------------------------------------------------------
CUTS = [1, 3, 7, 29, 64, 100]              # and the rest
CUT_N = 2600
CUT_START = 2 ** 31 + 3


def cut_paths(Fs):
    """two receivers over two transmitters; the longest delay, 150, is above every cut but the last: calls shorter than the delay read
    samples that earlier calls carried, through rings of 256 (transmitter 0) and 64 samples (transmitter 1)"""
    return [(0, 0, 0.11, 150, 1234), (0, 1, -0.07, 33, 0), (0, 0, 0.05, 0, -5), (1, 1, 0.09, 64, -(Fs // 2 - 1)), (1, 0, -0.04, 101, 0)]


# ---- 4. clipping: gains that drive the sum of two u8 transmitters far beyond +-1 ----------------------------------------------------------------
CLIP_PATHS = [(0, 0, 3.1, 0, 0), (0, 1, -2.3, 5, 1000)]
CLIP_N = 2100


# ---- 7. the shared-medium loop: terminal (transmitter 0, receiver 0) and repeater (1, 1) over tests/muxshapes.py's LOOP --------------------
FAR = dict(gain=1.0, delay=1234, offset=137)
LEAK = dict(gain=0.5, delay=0, offset=0)
LOOP_SIGMA = 0.1
LOOP_SEED = 5
LOOP_PATHS = [(0, 1, FAR["gain"], FAR["delay"], FAR["offset"]), (0, 0, LEAK["gain"], LEAK["delay"], LEAK["offset"]),
              (1, 0, FAR["gain"], FAR["delay"], FAR["offset"]), (1, 1, LEAK["gain"], LEAK["delay"], LEAK["offset"])]
