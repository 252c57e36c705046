"""Float64 statement of the transmitter's modulator (include/pirip_hip.h section I) and record helpers, for
tests/test_tx*.py.

    sample r of symbol i:  x = 2 exp(j 2 pi p / Fs),  p = (A_i + (r + 1) f_i) mod Fs,  A_i = (p0 + Ts * sum_{q<i} f_q) mod Fs

with f_i = (f1 + sym_i * shift) mod Fs in exact integers; a carrier-off symbol (0xFF) gives x = 0 and moves no phase."""
import numpy as np

OFF = 0xFF
# DESIGN.md 4.9, derived: the angle 2p/Fs as a fraction of pi is formed as float(p) * float(2/Fs) -- p < 2^24 exact, two roundings of
# 2^-24 relative on |t| <= 1 -> pi * 2^-23 (1 + 2^-25) in the angle; sincospif is documented to 1 ulp, at most 2^-23 for results in [-1, 1];
# the factor 2 is exact and doubles both.
BOUND = 2.0 * (np.pi * 2.0 ** -23 * (1 + 2.0 ** -25) + 2.0 ** -23)


def phase_ints(syms, f1, shift, Fs, Ts, p0=0):
    """syms: uint8 [nsym] -> (p int64 [nsym * Ts], on bool [nsym * Ts], final phase)"""
    syms = np.asarray(syms, dtype=np.int64)
    on = syms != OFF
    f = np.where(on, (f1 + syms * shift) % Fs, 0)
    A = (p0 + np.concatenate([[0], np.cumsum((f * Ts) % Fs)])) % Fs
    r = np.arange(1, Ts + 1, dtype=np.int64)
    p = (A[:-1, None] + r[None, :] * f[:, None]) % Fs
    return p.reshape(-1), np.repeat(on, Ts), int(A[-1])


def mod_f64(syms, f1, shift, Fs, Ts, p0=0):
    """complex128 [nsym * Ts]"""
    p, on, _ = phase_ints(syms, f1, shift, Fs, Ts, p0)
    return np.where(on, 2.0 * np.exp(2j * np.pi * p.astype(np.float64) / Fs), 0.0)


def quantise(x, amp):
    """the u8 quantiser clamp(rint(127 + amp x)) on float64 components [n, 2]; also returns the unrounded values"""
    v = 127.0 + amp * np.stack([x.real, x.imag], axis=-1)
    return np.clip(np.rint(v), 0, 255).astype(np.int64), v


def near_tie(v, amp, bound=BOUND):
    """where the float64 value lies within bound * amp of a rounding tie k + 1/2"""
    return np.abs(np.abs(v - np.floor(v)) - 0.5) <= bound * amp


def bits_to_syms(bits, M):
    b = np.asarray(bits, dtype=np.uint8)
    return b.copy() if M == 2 else (b[0::2] << 1 | b[1::2]).astype(np.uint8)


def burst_plan(rng, nbursts, max_frames):
    """burst-control bytes of nbursts bursts of 1..max_frames frames: 1 0 ... 0 2 per burst"""
    ctl = []
    for _ in range(nbursts):
        ctl += [1] + [0] * int(rng.integers(0, max_frames)) + [2]
    return ctl


def records(rng, ctl, kb):
    """uint8 [len(ctl), 1 + kb]: random payloads, zeros for the end-of-burst records (as frame_repeater.c:101 writes them)"""
    rec = rng.integers(0, 256, (len(ctl), 1 + kb)).astype(np.uint8)
    rec[:, 0] = ctl
    rec[np.asarray(ctl) == 2, 1:] = 0
    return rec


def carrier_mask(ctl, lead, gap, pre_syms, frame_syms):
    """bool [nsym]: True where the carrier is off, for one stream's control bytes"""
    m = [np.ones(lead, dtype=bool)]
    for c in ctl:
        if c == 1:
            m.append(np.zeros(pre_syms + frame_syms, dtype=bool))
        elif c == 0:
            m.append(np.zeros(frame_syms, dtype=bool))
        elif c == 2:
            m.append(np.ones(gap, dtype=bool))
    return np.concatenate(m)
