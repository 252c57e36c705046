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
    """contract 1: every complex-float component within 1e-5 * sum |h| of the float64 value. Past Lp = 84 the same derivation at its worst
    case: each component is one chain of 2 Lp float fmas, each rounding at most 2^-24 of a partial sum that sum |h| bounds, then a
    handful of roundings from the rotation -- (2 Lp + 8) 2^-24 sum |h|."""
    s = float(np.sum(np.abs(np.asarray(h, dtype=np.float64))))
    Lp = lp_of(h)
    return 1e-5 * s if Lp <= 84 else (2 * Lp + 8) * 2.0 ** -24 * s


def filter_len(transition_bw):
    """csdr's firdes_filter_len on the float the C entry point receives: 0.05f lies above 0.05, so the default is 79 taps, not 81"""
    L = int(4.0 / float(np.float32(transition_bw)))
    return L + 1 - L % 2


# The two functions below mirror the constants of pirip_hip_chan_create (pirip_amd/csrc/chan_kernels.hip: kThreads 256, kMaxGroup 8,
# kLdsTarget 40 KiB, kLdsMax 64 KiB) and must move with them. They compute nothing that a test compares with the device: they exist so
# that a shape table can assert which of the kernel's paths each of its shapes reaches.
def tile_geometry(D, Lp):
    """(P, Tpad, T, lds_bytes) of the host rule, or None where it answers PIRIP_ERR_UNSUPPORTED: row pitch P = D | 1, Tpad the most
    outputs (256 down to 64 in steps of 64) whose staged window fits 40 KiB, T = Tpad lowered until the window fits 64 KiB"""
    P = D | 1
    lds = lambda T: (T + -(-Lp // D)) * P * 8
    Tpad = 256
    while Tpad > 64 and lds(Tpad) > 40 * 1024:
        Tpad -= 64
    T = Tpad
    while T > 1 and lds(T) > 64 * 1024:
        T -= 1
    return None if lds(T) > 64 * 1024 else (P, Tpad, T, lds(T))


def group_sizes(K, Tpad):
    """the sizes of the balanced groups (at most 8 channels each) that K channels of one capture are split into: at least
    ceil(256 / Tpad) of them, so that every wave of the workgroup has work"""
    fill = -(-256 // Tpad)
    ng = -(-K // 8)
    if ng < fill:
        ng = min(K, fill)
    return [K // ng + (1 if g < K % ng else 0) for g in range(ng)]


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
