"""Float64 statement of the channel with drifting paths (include/pirip_hip.h section O, drift), for tests/test_air_drift*.py:
tests/airref.py's model with the interpolator on the library's own float table.

A path is a tuple (rx, tx, gain, delay, offset_hz, clock_ppb), the order of pirip_amd.HipAir's; five elements mean clock_ppb = 0. With
Q = 10^9, n_r the index of the last reset and m = age0 + (n - n_r) the clock age, a path with q = clock_ppb != 0 reads

    S = floor(m q / Q),  rho = m q - Q S,  i = n - d + S,  phi = floor(1024 rho / Q),   v[n] = sum_{k = 0 .. 15} T[phi][k] x_t[i - 7 + k]

with x_t[j] = 0 for j < n_r, and v takes the place of x_t[n - d] in airref's sum. S, rho and phi are int64 integers (|m q| < 2^50 inside the
slip budget); the taps are the library's floats, everything else is float64."""
import ctypes as C

import numpy as np

import airref
import txref

Q = 10 ** 9
PHASES, TAPS, LEAD = 1024, 16, 7
MAX_PPB = 10 ** 6
E = airref.E
_TABLE = None


def table():
    """the library's table, float32 [1024, 16]: pirip_hip_air_interp_table (host only, no device)"""
    global _TABLE
    if _TABLE is None:
        import pirip_amd
        t = np.zeros((PHASES, TAPS), dtype=np.float32)
        nph, ntp = C.c_int(0), C.c_int(0)
        assert pirip_amd.lib().pirip_hip_air_interp_table(t.ctypes.data, C.byref(nph), C.byref(ntp)) == 0
        assert (nph.value, ntp.value) == (PHASES, TAPS)
        _TABLE = t
    return _TABLE


def table_f64():
    """the definition in float64: T[phi][k] = sinc(k - 7 - mu) w((k - 7 - mu) / 8), mu = phi / 1024, w the Kaiser window of beta 6, every
    phase divided by its own sum"""
    mu = np.arange(PHASES, dtype=np.float64)[:, None] / PHASES
    x = np.arange(TAPS, dtype=np.float64)[None, :] - LEAD - mu
    u = x / (TAPS // 2)
    w = np.where(np.abs(u) <= 1.0, np.i0(6.0 * np.sqrt(np.maximum(1.0 - u * u, 0.0))) / np.i0(6.0), 0.0)
    t = np.sinc(x) * w
    return t / t.sum(axis=1, keepdims=True)


def lam(T=None):
    """Lambda = max_phi sum_k |T[phi][k]|: what the interpolator can make of a unit input"""
    T = table() if T is None else T
    return float(np.abs(np.asarray(T, dtype=np.float64)).sum(axis=1).max())


def ppb_of(p):
    return int(p[5]) if len(p) > 5 else 0


def slip(m, q):
    """(S, rho, phi) at the clock ages m (int64 array or Python int) of a clock q ppb off: exact integers"""
    mq = m * int(q)
    S = mq // Q                                                  # floor toward -inf, numpy's and Python's alike
    rho = mq - Q * S
    return S, rho, (PHASES * rho) // Q


def last_age(max_slip, q):
    """the last clock age the budget accepts for one path: q > 0: m q < (max_slip + 1) Q; q < 0: m |q| <= max_slip Q (Python integers)"""
    q = int(q)
    if q > 0:
        return ((int(max_slip) + 1) * Q - 1) // q
    return (int(max_slip) * Q) // -q


def samples_left(paths, max_slip, age):
    """how many samples from clock age `age` on the budget accepts (None without a drifting path)"""
    qs = [ppb_of(p) for p in paths if ppb_of(p)]
    if not qs:
        return None
    return max(0, min(last_age(max_slip, q) for q in qs) - int(age) + 1)


def interpolate(x, delay, q, age0, T=None):
    """v[n0 .. n0 + n - 1] of one drifting path: x complex128 [n] holds its transmitter's samples since the last reset"""
    T = np.asarray(table() if T is None else T, dtype=np.float64)
    n = x.shape[0]
    j = np.arange(n, dtype=np.int64)
    S, _, phi = slip(int(age0) + j, q)
    first = j - int(delay) + S - LEAD                            # index of tap 0, relative to the reset
    v = np.zeros(n, dtype=np.complex128)
    for k in range(TAPS):                                        # ascending, as the kernel accumulates
        idx = first + k
        assert idx.max(initial=-1) < n, "a tap past the newest sample: the delay is below 8 (+ max_slip for q > 0)"
        v += T[phi, k] * np.where(idx >= 0, x[np.clip(idx, 0, n - 1)], 0.0)
    return v


def signal(xw, Fs, paths, r, n0, age0=0, T=None):
    """the noise-free y_r, complex128 [n]: airref.signal with the drifting paths read through the interpolator"""
    n = xw.shape[1]
    idx = int(n0) + np.arange(n, dtype=np.int64)
    y = np.zeros(n, dtype=np.complex128)
    for p in airref.paths_of(paths, r):
        _, tx, gain, delay, off = p[:5]
        q = ppb_of(p)
        if q:
            xd = interpolate(xw[tx], delay, q, age0, T)
        else:
            xd = np.zeros(n, dtype=np.complex128)
            if delay < n:
                xd[delay:] = xw[tx, :n - delay]
        y += float(np.float32(gain)) * (airref.mixer(off, Fs, idx) if off else 1.0) * xd
    return y


def receive(xw, Fs, paths, r, n0, sigma=0.0, seed=1, age0=0):
    return signal(xw, Fs, paths, r, n0, age0) + airref.noise(seed, r, n0, xw.shape[1], sigma)


def bound(xw, paths, r, noise_mag=None, T=None):
    """airref.bound with two changes per drifting path (e = 2^-24): the path's |x| becomes Lambda max |x| -- what its sixteen
    taps can make of the input, so A_r = sum_p |a_p| L_p max |x_{t_p}| with L_p = Lambda or 1 --, and 16 e Lambda |a_p| max |x| is added:
    sixteen fma roundings of partial sums that Lambda max |x| bounds. The table's floats, S, rho and phi are the kernel's own and carry no
    error. Returns a scalar, or with noise_mag float64 [n]."""
    L = lam(T)
    mine = airref.paths_of(paths, r)
    A, extra = 0.0, 0.0
    for p in mine:
        a = abs(float(np.float32(p[2]))) * float(np.abs(xw[p[1]]).max(initial=0.0))
        if ppb_of(p):
            A += L * a
            extra += TAPS * E * L * a
        else:
            A += a
    b = (len(mine) + 12) * E * A + extra if mine else 0.0
    if noise_mag is None:
        return b
    return b + txref.NOISE_REL_BOUND * noise_mag + E * (A + noise_mag)


def rings(paths, ntx, max_slip):
    """samples of every transmitter's ring: the smallest power of two, at least 64, that holds its longest lag -- a static path's delay,
    a drifting one's with the 7 leading taps and, for q < 0, the slip"""
    out = []
    for t in range(ntx):
        lags = [p[3] + (LEAD if ppb_of(p) else 0) + (max_slip if ppb_of(p) < 0 else 0) for p in paths if p[1] == t]
        out.append(airref.ring_size(max(lags + [0])))
    return out
