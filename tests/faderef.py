"""Float64 statement of the channel with fading paths (include/pirip_hip.h section O, fading), for tests/test_air_fade*.py:
tests/airref.py's and tests/driftref.py's model with a path's value multiplied by the gain g[n] of the receiver's index, built from the
integers and floats pirip_hip_air_fade_table returns.

A fade is a tuple (path, doppler_hz, rice_k, key), the order of pirip_amd.HipAir's `fades`; path is an index into the list of paths. Per
fade the table is (w int32 [16], theta uint32 [16], s, los). The phase of scatterer j at absolute index n is the integer
psi_j(n) = (theta_j + w_j (n mod 2^32)) mod 2^32, in Python / int64 integers. At grid point k (absolute index 16 k) the definition takes the
top 24 bits of psi_j as a signed number of half turns, t_j = ((int32) psi_j >> 8) 2^-23 -- the angle 2 pi psi_j / 2^32 cut to the 24 bits a
float holds exactly, so that the angle carries no error --, and

    c_k = los + s sum_j e^{j pi t_j},        g[n] = c_k + mu (c_{k+1} - c_k)   with k = n >> 4, mu = (n & 15) / 16

in double: np.exp at the grid points and the line between them. v_p[n] g[n] then takes the place of v_p[n] in airref's / driftref's sum,
before the rotation, the gain and the noise, which are airref's."""
import numpy as np

import airref
import driftref
import txref

J, G = 16, 16
E = airref.E
M32 = 1 << 32
_TABLES = {}


def fade_of(f):
    """(path, doppler_millihz, rice_k as the float32 the library takes, key) of a fade tuple (path, doppler_hz, rice_k, key)"""
    path, hz, k, key = (tuple(f) + (0.0, 0))[:4]
    return int(path), int(round(float(hz) * 1000.0)), float(np.float32(k)), int(key)


def table(Fs, seed, fade):
    """the library's table of one fade (pirip_hip_air_fade_table: host only, no device): (w int64 [16], theta int64 [16], s, los)"""
    key = (int(Fs), int(seed)) + fade_of(fade)[1:]
    if key not in _TABLES:
        import pirip_amd
        w, theta, s, los = pirip_amd.air_fade_table(Fs, seed, fade)
        _TABLES[key] = (w.astype(np.int64), theta.astype(np.int64), float(s), float(los))
    return _TABLES[key]


def _splitmix(z):
    return int(txref._splitmix(np.array([z % (1 << 64)], dtype=np.uint64))[0])


def table_py(Fs, seed, fade):
    """the definition restated: alpha_j = 2 pi (j + u_j) / 16, nu_j = f_d cos alpha_j, w_j = rint(nu_j / Fs 2^32); u_j the top 53 bits of
    r1 = splitmix(seed ^ splitmix((key << 32) ^ j)) times 2^-53, theta_j the top 32 bits of splitmix(r1); s and los rounded once to float"""
    _, mhz, K, key = fade_of(fade)
    fd = mhz / 1000.0
    w, theta = [], []
    for j in range(J):
        r1 = _splitmix(int(seed) ^ _splitmix((key << 32) ^ j))
        u = (r1 >> 11) * 2.0 ** -53
        nu = fd * np.cos(2.0 * np.pi * (j + u) / J)
        w.append(int(np.rint(nu / Fs * 4294967296.0)))
        theta.append(_splitmix(r1) >> 32)
    return (np.array(w, dtype=np.int64), np.array(theta, dtype=np.int64), float(np.float32(np.sqrt(1.0 / (J * (K + 1.0))))),
            float(np.float32(np.sqrt(K / (K + 1.0)))))


def gamma(tab):
    """Gamma = los + 16 s: what bounds |g|"""
    return tab[3] + J * tab[2]


def phases(tab, k):
    """psi_j(16 k) for the grid points k (int64 array): int64 [len(k), 16] in [0, 2^32); |w| < 2^22, so no product passes 2^54"""
    w, theta = tab[0], tab[1]
    n16 = (np.asarray(k, dtype=np.int64) * G) % M32
    return (theta[None, :] + w[None, :] * n16[:, None]) % M32


def scatter(tab, k):
    """sum_j e^{j pi t_j} at the grid points k, complex128: the scatter part before the scale"""
    psi = phases(tab, k)
    signed = np.where(psi >= M32 // 2, psi - M32, psi)
    t = (signed >> 8).astype(np.float64) * 2.0 ** -23
    return np.exp(1j * np.pi * t).sum(axis=1)


def grid(tab, k):
    """c_k at the grid points k (int64 array), complex128"""
    return tab[3] + tab[2] * scatter(tab, k)


def gain(tab, idx):
    """g[n] at the absolute indices idx (int64, ascending and consecutive or not), complex128"""
    idx = np.asarray(idx, dtype=np.int64)
    k = idx >> 4
    k0 = int(k.min())
    c = grid(tab, np.arange(k0, int(k.max()) + 2, dtype=np.int64))
    mu = (idx & 15).astype(np.float64) / G
    lo, hi = c[k - k0], c[k - k0 + 1]
    return lo + mu * (hi - lo)


def fade_on(fades, pi):
    for f in fades or ():
        if int(f[0]) == pi:
            return f
    return None


def signal(xw, Fs, paths, fades, seed, r, n0, age0=0, tabs=None):
    """the noise-free y_r, complex128 [n]: driftref.signal with the fading paths multiplied by their gain at the receiver's index
    (tabs: {path index: table} to take the place of the library's, for a case worked by hand)"""
    n = xw.shape[1]
    idx = int(n0) + np.arange(n, dtype=np.int64)
    y = np.zeros(n, dtype=np.complex128)
    for pi, p in enumerate(paths):
        if p[0] != r:
            continue
        _, tx, gn, delay, off = p[:5]
        q = driftref.ppb_of(p)
        if q:
            xd = driftref.interpolate(xw[tx], delay, q, age0)
        else:
            xd = np.zeros(n, dtype=np.complex128)
            if delay < n:
                xd[delay:] = xw[tx, :n - delay]
        f = fade_on(fades, pi)
        if f is not None:
            xd = xd * gain(tabs[pi] if tabs and pi in tabs else table(Fs, seed, f), idx)
        y += float(np.float32(gn)) * (airref.mixer(off, Fs, idx) if off else 1.0) * xd
    return y


def receive(xw, Fs, paths, fades, seed, r, n0, sigma=0.0, age0=0):
    return signal(xw, Fs, paths, fades, seed, r, n0, age0) + airref.noise(seed, r, n0, xw.shape[1], sigma)


def fade_terms(tab):
    """what a fade adds to a path's error, per component, in units of e |a_p| L_p max |x| (e = 2^-24; derivation: bound below)"""
    s, Gm = tab[2], gamma(tab)
    grid_point = (2 * J + (J - 1) * J) * s + Gm                     # 272 s + Gamma
    line = grid_point + 3.0 * Gm                                    # the subtraction (2 Gamma) and the fma (Gamma)
    return 2.0 * line + 2.0 * np.sqrt(2.0) * Gm


def bound(xw, Fs, paths, fades, seed, r, noise_mag=None):
    """driftref.bound with the fading paths (e = 2^-24, one rounding to nearest). Derived, per component; nothing is
    measured to set it. With Gamma_p = los + 16 s for a fading path (1 otherwise) and L_p = Lambda for a drifting one (1 otherwise), a
    path's |x| becomes Gamma_p L_p max |x|: A_r = sum_p |a_p| Gamma_p L_p max |x_{t_p}|, and airref's (K_r + 12) e A_r covers the
    rotation, crot and the fma into the sum on that larger value. A fade adds, relative to |v| <= L_p max |x|:
      grid point   16 sincospif to 1 ulp, each at most 2 e on [-1, 1]: 32 e on C and on D; the angle t_j is exact (24 integer bits)
                   15 float adds of partial sums that 16 bounds: 15 * 16 e = 240 e
                   the scale: s * (32 + 240) e from C or D, and one rounding of fma(s, C, los) or s D, a value Gamma bounds: Gamma e
                   -> delta_c = (272 s + Gamma) e per component
      the line     c_{k+1} - c_k rounds once on a value 2 Gamma bounds: 2 Gamma e; fma(mu, d, c_k) rounds once on a value Gamma bounds:
                   Gamma e; (1 - mu) delta_c + mu delta_c = delta_c comes through  -> delta_g = (272 s + 4 Gamma) e per component
      crot(v, g)   delta_g on both components of g: (|v.re| + |v.im|) delta_g <= sqrt 2 |v| delta_g; its product and its fma on a
                   value |v| Gamma bounds: 2 Gamma e |v|
      -> (sqrt 2 (272 s + 4 Gamma) + 2 Gamma) e |v| per component of v g, which the carrier rotation can spread over both components of
      its result: times sqrt 2  ->  (2 (272 s + 4 Gamma) + 2 sqrt 2 Gamma) e |a_p| L_p max |x|        (fade_terms)
    A drifting path's 16 e Lambda |a_p| max |x| (driftref.bound) passes through crot(v, g) and the rotation when the path fades: times
    sqrt 2 Gamma and sqrt 2, 32 Gamma e Lambda |a_p| max |x|. Terms of second order stay inside the 0.88 e A_r that airref.bound leaves.
    The table's integers and floats, S, rho and phi are the kernel's own and carry no error. Returns a scalar, or with noise_mag
    float64 [n]."""
    L = driftref.lam()
    A, extra, K = 0.0, 0.0, 0
    for pi, p in enumerate(paths):
        if p[0] != r:
            continue
        K += 1
        a = abs(float(np.float32(p[2]))) * float(np.abs(xw[p[1]]).max(initial=0.0))
        Lp = L if driftref.ppb_of(p) else 1.0
        f = fade_on(fades, pi)
        Gm = 1.0
        if f is not None:
            tab = table(Fs, seed, f)
            Gm = gamma(tab)
            extra += fade_terms(tab) * E * Lp * a
        A += Gm * Lp * a
        if driftref.ppb_of(p):
            extra += driftref.TAPS * E * L * a * (2.0 * Gm if f is not None else 1.0)
    b = (K + 12) * E * A + extra if K else 0.0
    if noise_mag is None:
        return b
    return b + txref.NOISE_REL_BOUND * noise_mag + E * (A + noise_mag)
