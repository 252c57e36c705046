"""Float64 statement of the multiplexer (include/pirip_hip.h section J), for tests/test_mux*.py.

    u_c[n] = sum_{q=0}^{Q-1} h[p + qD] z_c[m - q],    n = mD + p, 0 <= p < D,  Q = ceil(L / D)
    w[n]   = sum_c a_c e^{+j 2 pi f_c n / Fs} u_c[n]

evaluated in double on the same float inputs, the same h (the handle's taps(), widened) and the same gains, with the mixer's phase taken
from the exact integer ((f_c mod Fs)(n mod Fs)) mod Fs. A call hands every channel n_in samples whose first has absolute index m0 and
gives (n_in - Q + 1) D outputs, the first at absolute index (m0 + Q - 1) D."""
import numpy as np

FIR, LINEAR = 0, 1


def q_of(L, D):
    return -(-L // D)


def nout(n_in, Q, D):
    return 0 if n_in < Q else (n_in - Q + 1) * D


def linear_taps(D):
    """PIRIP_MUX_LINEAR: h[i] = 1 - |i - (D-1)| / D, i = 0 .. 2D-2 (D = 1: one tap of 1), as the float the handle holds"""
    i = np.arange(2 * D - 1, dtype=np.float64)
    return (1.0 - np.abs(i - (D - 1)) / D).astype(np.float32)


def padded(h, D):
    Q = q_of(len(h), D)
    hp = np.zeros(Q * D, dtype=np.float64)
    hp[:len(h)] = np.asarray(h, dtype=np.float64)
    return hp, Q


def interp(z, h, D):
    """u over the call's outputs, complex128 [nout]: z zero-stuffed to the wideband rate and convolved with h -- output j of the call is
    index (Q-1) D + j of that convolution, where every tap p + qD meets z[m - q] with m - q >= 0"""
    hp, Q = padded(h, D)
    z = np.asarray(z, dtype=np.complex128)
    no = nout(len(z), Q, D)
    if no == 0:
        return np.zeros(0, dtype=np.complex128)
    x = np.zeros(len(z) * D, dtype=np.complex128)
    x[::D] = z
    return np.convolve(x, hp)[(Q - 1) * D:(Q - 1) * D + no]


def mixer(fc, Fs, n0, count):
    """e^{+j 2 pi f_c n / Fs} for n = n0 .. n0 + count - 1, the phase from exact integers"""
    n = (int(n0) % Fs + np.arange(count, dtype=np.int64)) % Fs
    p = (n * (int(fc) % Fs)) % Fs
    return np.exp(2j * np.pi * p.astype(np.float64) / Fs)


def mux(z, h, D, Fs, offsets, gains, m0=0):
    """one output: z [K, n_in] complex (the float inputs, widened), offsets [K] Hz, gains [K] -> complex128 [nout]"""
    z = np.asarray(z, dtype=np.complex128)
    Q = q_of(len(h), D)
    no = nout(z.shape[1], Q, D) if z.shape[0] else 0
    w = np.zeros(no, dtype=np.complex128)
    n0 = (int(m0) + Q - 1) * D
    for c in range(z.shape[0]):
        w += float(gains[c]) * mixer(offsets[c], Fs, n0, no) * interp(z[c], h, D)
    return w


def quantise_u8(w):
    """clamp(rint(127.5 v + 127.5), 0, 255) of the float64 value per component: (bytes int64 [n, 2], the unrounded arguments [n, 2])"""
    v = 127.5 * np.stack([w.real, w.imag], axis=-1) + 127.5
    return np.clip(np.rint(v), 0, 255).astype(np.int64), v


def amplitude(z, h, D, gains):
    """A = sum_c |a_c| max|z_c| max_p sum_q |h[p + qD]|: what bounds every partial sum of an output"""
    hp, Q = padded(h, D)
    branch = float(np.abs(hp).reshape(Q, D).sum(axis=0).max())
    z = np.asarray(z, dtype=np.complex128)
    return float(sum(abs(float(gains[c])) * float(np.abs(z[c]).max(initial=0.0)) for c in range(z.shape[0]))) * branch


def bound(z, h, D, gains):
    """DESIGN.md 4.10, derived (e = 2^-24, one rounding to nearest; every term relative to A). Per component of an output:
      accumulation   each channel's sum is 2 Q fmas per component, each rounding at most e of a partial sum that A bounds;
                     K - 1 additions of channel sums (the first is added to zero, exactly)                        2 K Q + K - 1
      pre-rotation   the angle float(r) * float(2 / Fs): r < 2^24 exact, two roundings of e on |t| <= 1, times pi      2 pi (1 + 2^-25)
                     sincospif to 1 ulp, at most 2e on [-1, 1], on both c and s: sqrt(2) |z| 2e per component           2 sqrt 2
                     z' = fma(zr, c, -(zi s)) and its twin: a product and an fma                                       2
      taps           g_c's components as stored: e of |g| each, |d gr zr| + |d gi zi| <= e |g| |z|                      1
    = (2 K Q + K + 12.2) e A; the 13 used leaves 0.8 e A for the terms of second order, which stay below 2e times the sum of the first
    order ones (2 K Q + K + 13 <= 1500 at the largest shape tested: 1500^2 e^2 < 0.14 e). The issue's (4 K Q + 16) e A is never
    smaller: it counts 4 Q roundings per channel where a component meets 2 Q."""
    K = len(gains)
    Q = q_of(len(h), D)
    return (2 * K * Q + K + 13) * 2.0 ** -24 * amplitude(z, h, D, gains)


def issue_bound(z, h, D, gains):
    """(4 K Q + 16) 2^-24 A, as first stated for this stage; bound() must never exceed it"""
    return (4 * len(gains) * q_of(len(h), D) + 16) * 2.0 ** -24 * amplitude(z, h, D, gains)


def tie_window(v, b):
    """where a byte may differ from quantise_u8 of the float64 value: the argument within 127.5 b + 2^-16 of a tie k + 1/2 (2^-16: the two
    float roundings of the quantiser below 256)"""
    return np.abs(np.abs(v - np.floor(v)) - 0.5) <= 127.5 * b + 2.0 ** -16


# The function below mirrors the constants of pirip_hip_mux_create (pirip_amd/csrc/mux_kernels.hip: 256 threads, 8 outputs per thread,
# groups of at most 8 channels, 64 KiB of LDS) and must move with them. It computes nothing that a test compares with the device: it
# exists so that a shape table can assert which of the kernel's paths each of its shapes reaches.
TILE = 2048


def geometry(D, L, bytes_per_sample):
    """(Q, Dp, Mt, G, lds_bytes) of the host rule, or None where it answers PIRIP_ERR_UNSUPPORTED: Dp the tap row's pitch (D, or D + 31
    past D = 32), Mt the most input samples a tile of 2048 outputs touches, G the channels staged together"""
    Q = q_of(L, D)
    Dp = D + 31 if D > 32 else D
    Mt = (D + TILE - 2) // D + Q
    lds = lambda G: TILE * bytes_per_sample + 8 * G * (Q * Dp + Mt)
    if lds(1) > 64 * 1024:
        return None
    G = 8
    while G > 1 and lds(G) > 64 * 1024:
        G -= 1
    return Q, Dp, Mt, G, lds(G)
