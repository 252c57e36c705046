"""The statement of include/pirip_hip.h section P (the band monitor) in plain numpy float32, written from the header alone: segments, rows,
band walks, bin(f), scale and nrows. The transform is the oracle's (oracle/kiss_fft_oracle.c at its default, the unfused twiddle multiply)."""
import ctypes as C
import math

import numpy as np

from oracle import binding as ob

U8, CF32 = 1, 3                      # PIRIP_IN_CU8_CSDR, PIRIP_IN_CF32
NFFTS = (256, 1024, 4096)
BAND_ROW = [("power", "<f4"), ("peak", "<f4"), ("peak_bin", "<i4")]

_cfg = {}


def _lib():
    l = ob.lib()
    l.kiss_fft_oracle_alloc.restype = C.c_void_p
    l.kiss_fft_oracle_alloc.argtypes = [C.c_int, C.c_int]
    l.kiss_fft_oracle.restype = None
    l.kiss_fft_oracle.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    l.kiss_fft_oracle_free.restype = None
    l.kiss_fft_oracle_free.argtypes = [C.c_void_p]
    return l


def fft(v):
    """forward kiss_fft of complex64 [nfft] (the configurations are kept for the life of the process)"""
    l = _lib()
    assert l.kiss_fft_oracle_get_fused_mul() == 0, "section P is stated on the unfused multiply"
    v = np.ascontiguousarray(v, dtype=np.complex64)
    n = v.shape[0]
    if n not in _cfg:
        _cfg[n] = l.kiss_fft_oracle_alloc(n, 0)
    out = np.zeros(n, dtype=np.complex64)
    l.kiss_fft_oracle(_cfg[n], v.ctypes.data, out.ctypes.data)
    return out


def window(nfft):
    """w[i] = 0.5 - 0.5 cos(2 pi i / nfft) in double, rounded once, for i <= nfft / 2; the upper half mirrors the lower"""
    w = np.zeros(nfft, dtype=np.float32)
    for i in range(nfft // 2 + 1):
        w[i] = np.float32(0.5 - 0.5 * math.cos(2.0 * math.pi * i / nfft))
    for i in range(nfft // 2 + 1, nfft):
        w[i] = w[nfft - i]
    return w


def scale(nfft, avg, w=None):
    w = window(nfft) if w is None else w
    s = 0.0
    for i in range(nfft):
        s += float(w[i]) * float(w[i])
    return 1.0 / (float(avg) * s)


def to_float(x, fmt):
    """the samples as the kernel reads them: complex64 [n]. u8 [n, 2]: b / 127.5 - 1 in double, rounded to float (csdr's convert_u8_f)"""
    if fmt == U8:
        f = (x.astype(np.float64) / 127.5 - 1.0).astype(np.float32)
        return (f[:, 0] + 1j * f[:, 1]).astype(np.complex64)
    return np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)


def segments(t, nfft, hop):
    """complete segments of a stream of t samples"""
    return 0 if t < nfft else (t - nfft) // hop + 1


def nrows(pos, n, nfft, hop, avg):
    """rows a push of n samples completes when pos samples were pushed before it"""
    return segments(pos + n, nfft, hop) // avg - segments(pos, nfft, hop) // avg


def segment_parts(x, k, nfft, hop, w):
    """(v, X, p) of segment k of complex64 x, each rounded as the contract says"""
    s = x[k * hop: k * hop + nfft]
    v = np.empty(nfft, dtype=np.complex64)
    v.real = w * s.real
    v.imag = w * s.imag
    X = fft(v)
    p = (X.real * X.real).astype(np.float32) + (X.imag * X.imag).astype(np.float32)
    return v, X, p.astype(np.float32)


def rows(x, fmt, nfft, hop, avg, w=None):
    """every complete row of one stream: float32 [m, nfft], unscaled, FFT bin order"""
    w = window(nfft) if w is None else w
    z = to_float(x, fmt)
    m = segments(len(z), nfft, hop) // avg
    out = np.zeros((m, nfft), dtype=np.float32)
    for j in range(m):
        row = np.zeros(nfft, dtype=np.float32)
        for k in range(j * avg, j * avg + avg):
            row = (row + segment_parts(z, k, nfft, hop, w)[2]).astype(np.float32)
        out[j] = row
    return out


def bin_of(f, nfft, Fs):
    """floor((2 f nfft + Fs) / (2 Fs)) mod nfft (Python's // floors toward minus infinity and its % gives [0, nfft))"""
    return ((2 * int(f) * nfft + Fs) // (2 * Fs)) % nfft


def band_bins(lo, hi, nfft, Fs):
    """(first bin, number of bins)"""
    first = bin_of(lo, nfft, Fs)
    return first, (bin_of(hi, nfft, Fs) - first) % nfft + 1


def band_rows(rws, lo, hi, nfft, Fs):
    """power, peak and peak_bin of one band in every row of rws [m, nfft]: a structured array [m]"""
    first, count = band_bins(lo, hi, nfft, Fs)
    out = np.zeros(rws.shape[0], dtype=BAND_ROW)
    for j, row in enumerate(rws):
        power, peak, peak_bin = np.float32(0.0), row[first], first
        b = first
        for _ in range(count):
            v = row[b]
            power = np.float32(power + v)
            if v > peak:
                peak, peak_bin = v, b
            b = (b + 1) % nfft
        out[j] = (power, peak, peak_bin)
    return out


def db(rws, scl):
    """10 log10(rows scale), bins shifted to dash.py's axis: entry i at -Fs/2 + i Fs/nfft"""
    with np.errstate(divide="ignore"):
        return np.fft.fftshift(10.0 * np.log10(np.asarray(rws, dtype=np.float64) * scl), axes=-1)


def bin_hz(b, nfft, Fs):
    return (b if b < nfft // 2 else b - nfft) * Fs / nfft
