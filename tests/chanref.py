"""Float64 statement of the channelizer (include/pirip_hip.h section H) and wideband test captures, for tests/test_channelizer*.py.

    y_c[j] = sum_{i=0}^{Lp-1} h[i] x[jD+i] e^{-j 2 pi f_c (t0 + jD + i) / Fs},   x = b / 127.5 - 1

evaluated in double on the same bytes and the same h, with the mixer's phase taken from the exact integer (f_c mod Fs)(t0 + n) mod Fs."""
import numpy as np


def lp_of(h):
    """csdr pads the taps with zeros to a multiple of 4"""
    L = len(h)
    return L + 3 - ((L + 3) % 4)


def nout(n_in, Lp, D):
    return 0 if n_in < Lp else (n_in - Lp) // D + 1


def channel(u8, h, D, Fs, fc, t0=0):
    """u8: [n, 2] uint8 IQ; h: prototype taps (float32, unpadded) -> complex128 [nout]"""
    Lp = lp_of(h)
    hp = np.zeros(Lp, dtype=np.float64)
    hp[:len(h)] = np.asarray(h, dtype=np.float64)
    n = u8.shape[0]
    no = nout(n, Lp, D)
    x = u8[:, 0].astype(np.float64) / 127.5 - 1.0 + 1j * (u8[:, 1].astype(np.float64) / 127.5 - 1.0)
    idx = (int(t0) % Fs + np.arange(n, dtype=np.int64)) % Fs
    p = (idx * (int(fc) % Fs)) % Fs
    xm = x * np.exp(-2j * np.pi * p.astype(np.float64) / Fs)
    if no == 0:
        return np.zeros(0, dtype=np.complex128)
    win = np.lib.stride_tricks.sliding_window_view(xm, Lp)[::D][:no]
    return win @ hp


def bound(h):
    """contract 1: every complex-float component within 1e-5 * sum |h| of the float64 value"""
    return 1e-5 * float(np.sum(np.abs(np.asarray(h, dtype=np.float64))))


def to_s16(y):
    """convert_f_s16 of the float64 value (truncation), clamped to the s16 range"""
    v = np.clip(np.stack([y.real, y.imag], axis=-1) * 32767.0, -32768.0, 32767.0)
    return np.trunc(v).astype(np.int64)


def fsk_wideband(Fs, Rs, M, f_tone0, spacing, bits, nsamp, amp, phase0=0.0):
    """complex128 [nsamp]: phase-continuous M-FSK at the wideband rate, tones f_tone0 + m * spacing, symbols MSB first (fsk_mod's map);
    amp is the amplitude in u8 steps; bits shorter than the capture are followed by zeros"""
    ts = Fs // Rs
    bps = 1 if M == 2 else 2
    nsym = -(-nsamp // ts)
    b = np.zeros(nsym * bps, dtype=np.int64)
    nb = min(len(bits), nsym * bps)
    b[:nb] = np.asarray(bits, dtype=np.int64)[:nb]
    b = b.reshape(nsym, bps)
    sym = b[:, 0] if M == 2 else 2 * b[:, 0] + b[:, 1]
    f = np.repeat(f_tone0 + spacing * sym, ts)[:nsamp].astype(np.float64)
    ph = phase0 + 2 * np.pi * np.cumsum(f) / Fs
    return amp * np.exp(1j * ph)


def quantise_u8(z):
    """complex (u8 steps around 127.5) -> [n, 2] uint8"""
    return np.stack([np.clip(np.rint(127.5 + z.real), 0, 255), np.clip(np.rint(127.5 + z.imag), 0, 255)], axis=-1).astype(np.uint8)


def bit_errors(rx, tx, skip):
    """errors of rx[skip:] against tx at the best alignment (tx repeats); returns (errors, compared bits)"""
    rx = np.asarray(rx, dtype=np.uint8)[skip:]
    tx = np.asarray(tx, dtype=np.uint8)
    n = len(rx)
    reps = np.resize(tx, n + len(tx))
    best = None
    for s in range(len(tx)):
        e = int(np.count_nonzero(rx != reps[s:s + n]))
        if best is None or e < best:
            best = e
            if e == 0:
                break
    return best, n
