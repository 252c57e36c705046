"""Float64 statement of the channel (include/pirip_hip.h section O), for tests/test_air*.py.

    y_r[n] = sum_{p : rx_p = r, ascending p} a_p e^{+j 2 pi f_p n / Fs} x_{t_p}[n - d_p]  +  sigma_r w_r[n]

with n the absolute sample index and x_t[k] = 0 below the index of the last reset, evaluated in double on the same float32 inputs (a u8
byte is the float csdr's convert_u8_f makes of it), the same float32 gains and sigma, the mixer's phase from the exact integer
((f_p mod Fs)(n mod Fs)) mod Fs and w from txref.noise_f64 on the kernel's own uniforms. A path is a tuple (rx, tx, gain, delay,
offset_hz), the order of pirip_amd.HipAir's."""
import numpy as np

import muxref
import txref

U8, CF32 = 1, 3                            # PIRIP_IN_CU8_CSDR, PIRIP_IN_CF32
E = 2.0 ** -24
# The constants below mirror pirip_amd/csrc/air_handle.hpp (kAirTile, kAirMinRing) and must move with them. They compute nothing that a
# test compares with the device: they exist so that a shape table can assert which of the kernel's corners each of its shapes reaches.
TILE = 2048
MIN_RING = 64
MAX_DELAY = 1 << 20


def widen(x, fmt):
    """the call's input rows as the kernel reads them, complex128 [ntx, n]: uint8 [ntx, n, 2] through float32(b / 127.5 - 1) -- csdr's
    convert_u8_f, which iq_device.hpp's u8_to_float equals for all 256 bytes -- or complex64 [ntx, n] as it is"""
    if fmt == U8:
        v = (np.asarray(x, dtype=np.float64) / 127.5 - 1.0).astype(np.float32).astype(np.float64)
        return v[..., 0] + 1j * v[..., 1]
    return np.asarray(x, dtype=np.complex64).astype(np.complex128)


def paths_of(paths, r):
    return [p for p in paths if p[0] == r]


def mixer(f, Fs, idx):
    """e^{+j 2 pi f n / Fs} at the absolute indices idx (int64), the phase from exact integers"""
    p = ((idx % Fs) * (int(f) % Fs)) % Fs
    return np.exp(2j * np.pi * p.astype(np.float64) / Fs)


def signal(xw, Fs, paths, r, n0):
    """the noise-free y_r, complex128 [n]: xw complex128 [ntx, n] holds the samples n0 .. n0 + n - 1 since the last reset"""
    n = xw.shape[1]
    idx = int(n0) + np.arange(n, dtype=np.int64)
    y = np.zeros(n, dtype=np.complex128)
    for _, tx, gain, delay, off in paths_of(paths, r):
        xd = np.zeros(n, dtype=np.complex128)
        if delay < n:
            xd[delay:] = xw[tx, :n - delay]
        y += float(np.float32(gain)) * (mixer(off, Fs, idx) if off else 1.0) * xd
    return y


def noise(seed, r, n0, n, sigma):
    """sigma_r w_r[n0 .. n0 + n - 1], complex128 (zeros for sigma 0: the kernel adds nothing then)"""
    s = float(np.float32(sigma))
    if s <= 0.0:
        return np.zeros(n, dtype=np.complex128)
    return txref.noise_f64(seed, r, int(n0) + np.arange(n, dtype=np.int64), s)


def receive(xw, Fs, paths, r, n0, sigma=0.0, seed=1):
    return signal(xw, Fs, paths, r, n0) + noise(seed, r, n0, xw.shape[1], sigma)


def amplitude(xw, paths, r):
    """A_r = sum_p |a_p| max |x_{t_p}|: what bounds every partial sum of the receiver, per component"""
    return float(sum(abs(float(np.float32(g))) * float(np.abs(xw[tx]).max(initial=0.0)) for _, tx, g, _, _ in paths_of(paths, r)))


def bound(xw, paths, r, noise_mag=None):
    """DESIGN.md 4.15, derived (e = 2^-24, one rounding to nearest; the input and the gains are the kernel's own floats, so they carry no
    error). Per component of y_r, relative to A_r = sum_p |a_p| max |x_{t_p}|, and per path of modulus |x| <= max |x_t|:
      rotated path   the angle float(p) * float(2 / Fs): p < 2^24 exact, two roundings of e on |t| <= 1, times pi        2 pi (1 + 2^-25)
                     sincospif to 1 ulp, at most 2e on [-1, 1], on both c and s: sqrt(2) |x| 2e per component            2 sqrt 2
                     crot: fma(xr, c, -(xi s)) and its twin -- one product and one fma                                   2
                     (an unrotated path has none of the three; it is counted as rotated)
      every path     acc = fma(a_p, v, acc): one rounding of a partial sum that A_r bounds                               1
    = (K_r + 11.12) e A_r; the 12 used leaves 0.88 e A_r for the terms of second order, which stay below 2e times the sum of the first
    order ones ((K_r + 12) <= 100 at anything tested here: 2 * 100^2 e^2 < 0.01 e). That is the issue's (K_r + 12) e A_r.
    With noise (noise_mag = |sigma_r w_r[n]| per sample): add_awgn's product is within txref.NOISE_REL_BOUND of the sample's magnitude, and
    its sum with acc rounds once, at most e (A_r + |sigma w|). Returns a scalar, or with noise_mag float64 [n]."""
    K = len(paths_of(paths, r))
    A = amplitude(xw, paths, r)
    b = (K + 12) * E * A if K else 0.0
    if noise_mag is None:
        return b
    return b + txref.NOISE_REL_BOUND * noise_mag + E * (A + noise_mag)


def quantise_u8(y):
    """clamp(rint(127.5 v + 127.5), 0, 255) of the float64 value per component: (bytes int64 [n, 2], the unrounded arguments [n, 2])"""
    return muxref.quantise_u8(y)


def tie_window(v, b):
    """where a byte may differ from quantise_u8 of the float64 value: the argument within 127.5 b + 2^-16 of a tie (b: scalar or [n])"""
    b = np.asarray(b, dtype=np.float64)
    return muxref.tie_window(v, b[..., None] if b.ndim else b)


def ring_size(longest_delay):
    """samples of a transmitter's ring: the smallest power of two, at least MIN_RING, that holds its longest delay"""
    R = MIN_RING
    while R < longest_delay:
        R *= 2
    return R


def rings(paths, ntx):
    return [ring_size(max([p[3] for p in paths if p[1] == t] + [0])) for t in range(ntx)]
