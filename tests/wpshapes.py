"""Inputs shared by tests/test_wave_window_power_cpu.py and tests/test_wave_window_power.py: the wave kernel's packed window powers and
the ppm smoother's constant divide ("packed window powers").

Every batch is 6 streams (one full workgroup of four and a partial one). The CPU test establishes on the oracle alone that every
stream's norm_rx_timing keeps 5e-4 symbols away from +-0.25 (where nin steps) and +-0.5 (where the angle wraps) in every frame, so
the device test demands the oracle's nin sequence exactly and exempts no stream.
"""
import numpy as np

import sigutil
from demodrun import resample_at

U8D, CSDR = 0, 1                                  # pirip_amd.IN_* == oracle.IN_*
NSYM = 50


def shape(M, P, fmt, est_max, band=False):
    return dict(Fs=240000, Rs=10000, M=M, P=P, f1=10000, shift=10000, est_min=500, est_max=est_max, fmt=fmt, band=band)


# the instances wave_packed_power_instance (fsk_demod_wave.hip) names ...
# (the band-only twin goes with the headline: the band-only estimator must not change an output word of the full one)
PACKED = {"headline_u8": shape(2, 24, U8D, 25000), "band_only": shape(2, 24, U8D, 25000, band=True)}
# ... and instances outside it, which must compute what they computed before the change, word for word
UNCHANGED = {"csdr_u8": shape(2, 24, CSDR, 25000), "4fsk_p8": shape(4, 8, U8D, 60000)}

CLEAN_FRAMES, PPM_FRAMES = 12, 40
CLEAN_OFFSETS = (0, 5, 11, 17, 23, 20)            # samples of Ts = 24: floor(rx_timing) is -1, -6, -6, 0, 0 and 3
PPM = (300.0, -300.0, 300.0, -300.0, 300.0, -300.0)
PPM_OFFSETS = (12, 11, 18, 5, 13, 10)             # (chosen so that no frame's timing lands within TIMING_MARGIN of a threshold)
EBNO_DB = 9.0
TIMING_MARGIN = 5e-4


def _resample(x, ratio):
    """x read at positions 0, ratio, 2 ratio, ... (linear interpolation)"""
    return resample_at(x, np.arange(int((x.shape[0] - 2) / ratio)) * ratio)


def clean(oracle, c):
    """noise-free, every stream at its own start offset"""
    return sigutil.batch(oracle, c, [sigutil.mod_frames(oracle, c, CLEAN_FRAMES + 2, 100 + s)[off:] for s, off in enumerate(CLEAN_OFFSETS)])


def drifting(oracle, c):
    """+ 300 / - 300 ppm of sample-clock offset over 40 frames: 0.36 samples per frame, so nin steps at least once in each direction"""
    return sigutil.batch(oracle, c, [_resample(sigutil.mod_frames(oracle, c, PPM_FRAMES + 2, 200 + s), 1.0 + ppm * 1e-6)[off:]
                                  for s, (ppm, off) in enumerate(zip(PPM, PPM_OFFSETS))])


def noisy(oracle, c):
    rng = np.random.default_rng(300)
    return sigutil.batch(oracle, c, [sigutil.add_awgn(sigutil.mod_frames(oracle, c, CLEAN_FRAMES + 2, 300 + s), EBNO_DB, c, rng)[off:] * np.float32(0.5)
                                  for s, off in enumerate(CLEAN_OFFSETS)])


CASES = {"clean": clean, "drifting": drifting, "noisy": noisy}
